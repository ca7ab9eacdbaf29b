// libd2d_hud.so -- frames with the text overlay, the angle arcs and the drone shades (include/d2d_hud.h).
//
// Three kernels over the shared code of d2d_hud_core.h and csrc/render/d2d_raster.h:
//   setup_kernel    one lane per (frame, extended slot): the frame's extended primitive list into the ctx
//                   workspace; behind the slots, one lane per (frame, text line) formats the line
//   raster_kernel   d2d_raster.h's tile walk over the extended list; a pixel no primitive covers takes
//                   the text's colour (a lookup in the frame's formatted lines and the font)
//   shade_kernel    the shade recorder, one lane per tracked env
// No call allocates or synchronises; all launches are ordered on the caller's stream.  No scratch, no
// atomics.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <new>
#include <string>

#include "d2d_hud_core.h"

using namespace d2dh;

namespace {

thread_local std::string g_err;

int32_t fail(int32_t code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

struct FrameArgs {
    const d2d_scn* scn;
    const double* state;
    const float* obs;
    const float* act;
    const float* trail;
    const int32_t* trail_len;
    const float* info;  // NULL unless the text is drawn
    const double* shade;
    const int32_t* shade_count;
    int32_t n_frames, max_trail, max_shades;  // max_shades: 0 without shade buffers
};

__device__ __forceinline__ int32_t list_len(const int32_t* trail_len, int32_t max_trail, int32_t max_shades, int32_t f) {
    return ext_len(trail_len ? clamp_len(trail_len[f], max_trail) : 0, max_shades);
}

__global__ __launch_bounds__(NT) void setup_kernel(Prim* __restrict__ prims, int32_t cap, uint8_t* __restrict__ text,
                                                   View v, FrameArgs a) {
    const int32_t slot = (int32_t)(blockIdx.x * NT + threadIdx.x), f = (int32_t)blockIdx.y;
    const int32_t np = list_len(a.trail_len, a.max_trail, a.max_shades, f);  // <= cap (checked at the entry point)
    if (slot >= np) {
        const int32_t line = slot - np;
        if (a.info != nullptr && line < D2DH_TEXT_LINES)
            format_line(a.info + (size_t)D2D_INFO_DIM * (size_t)f, line,
                        text + ((size_t)f * D2DH_TEXT_LINES + (size_t)line) * D2DH_LINE_CHARS);
        return;
    }
    FrameIn in;
    in.scn = a.scn + f;
    in.state = a.state, in.stride = a.n_frames, in.frame = f;
    in.obs = a.obs ? a.obs + (size_t)D2D_OBS_DIM * (size_t)f : nullptr;
    in.act = a.act ? a.act + (size_t)D2D_ACT_DIM * (size_t)f : nullptr;
    in.trail = a.trail ? a.trail + 2 * (size_t)a.max_trail * (size_t)f : nullptr;
    in.trail_len = a.trail_len ? clamp_len(a.trail_len[f], a.max_trail) : 0;
    HudIn h;
    h.max_shades = a.max_shades;
    h.shade = a.shade ? a.shade + 3 * (size_t)a.max_shades * (size_t)f : nullptr;
    h.n_shades = a.shade ? clamp_len(a.shade_count[f], a.max_shades) : 0;
    prims[(size_t)f * (size_t)cap + (size_t)slot] = ext_prim(in, h, v, slot);
}

__global__ __launch_bounds__(NT) void raster_kernel(const Prim* __restrict__ prims, int32_t cap,
                                                    const uint8_t* __restrict__ text, View v,
                                                    const int32_t* __restrict__ trail_len, int32_t max_trail,
                                                    int32_t max_shades, uint8_t* __restrict__ out) {
    __shared__ TileLds lds;
    const int32_t f = (int32_t)blockIdx.y;
    const uint8_t* lines = text ? text + (size_t)f * D2DH_TEXT_LINES * D2DH_LINE_CHARS : nullptr;
    const int32_t s = text_scale(v.H);
    walk_tile(
        prims + (size_t)f * (size_t)cap, v, f, [&](int32_t fr) { return list_len(trail_len, max_trail, max_shades, fr); },
        [&](int32_t row, int32_t col) { return text_colour(lines, s, row, col); }, lds, out);
}

__global__ __launch_bounds__(64) void shade_kernel(int32_t n_tracked, const int32_t* __restrict__ env_ids, int32_t n_envs,
                                                   const double* __restrict__ state, const uint8_t* __restrict__ term,
                                                   const uint8_t* __restrict__ trunc, double distance, int32_t max_shades,
                                                   double* __restrict__ shade, int32_t* __restrict__ count,
                                                   double* __restrict__ last) {
    const int32_t k = (int32_t)(blockIdx.x * 64 + threadIdx.x);
    if (k >= n_tracked) return;
    shade_step(k, env_ids, n_envs, state, term, trunc, distance, max_shades, shade, count, last);
}

struct DeviceGuard {  // launches go to the given device; the caller's current device is put back
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        ok = hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess);
        if (prev == dev) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int32_t check_view(const d2dr_view* v) {
    if (!v) return fail(D2DH_E_ARG, "view is NULL");
    if (v->width < D2DR_MIN_SIZE || v->width > D2DR_MAX_SIZE || v->height < D2DR_MIN_SIZE || v->height > D2DR_MAX_SIZE)
        return fail(D2DH_E_ARG, "picture %d x %d: width and height must be %d..%d", v->width, v->height, D2DR_MIN_SIZE,
                    D2DR_MAX_SIZE);
    if (!(v->screen_w > 0.0) || !(v->screen_h > 0.0) || !finite_d(v->screen_w) || !finite_d(v->screen_h))
        return fail(D2DH_E_ARG, "screen_w and screen_h must be positive and finite");
    return D2DH_OK;
}

int32_t check_update(int32_t n_tracked, const void* ids, int32_t n_envs, const void* state, const void* term,
                     const void* trunc, double distance, int32_t max_shades, const void* shade, const void* count,
                     const void* last) {
    if (n_tracked < 0 || n_envs < 1) return fail(D2DH_E_ARG, "n_tracked must not be negative and n_envs must be positive");
    if (max_shades < 1 || max_shades > D2DH_MAX_SHADES)
        return fail(D2DH_E_ARG, "max_shades %d: must be 1..%d", max_shades, D2DH_MAX_SHADES);
    if (!(distance >= 0.0)) return fail(D2DH_E_ARG, "distance must not be negative or NaN");
    if (n_tracked == 0) return D2DH_OK;
    if (!ids || !state || !shade || !count || !last)
        return fail(D2DH_E_ARG, "env_ids, state, shade, shade_count and last must not be NULL");
    if ((term == nullptr) != (trunc == nullptr)) return fail(D2DH_E_ARG, "term and trunc must both be given or both be NULL");
    return D2DH_OK;
}

int32_t launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? D2DH_OK : fail(D2DH_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace

struct d2dh_ctx {
    int32_t device, max_frames, max_trail, max_shades, max_width, max_height;
    int32_t cap;  // extended list slots per frame
    Prim* prims;
    uint8_t* text;
};

extern "C" {

int32_t d2dh_abi_version(void) { return D2DH_ABI_VERSION; }
const char* d2dh_last_error(void) { return g_err.c_str(); }

int32_t d2dh_create(int32_t device, int32_t max_frames, int32_t max_trail, int32_t max_shades, int32_t max_width,
                    int32_t max_height, d2dh_t** out) {
    if (!out) return fail(D2DH_E_ARG, "out is NULL");
    *out = nullptr;
    if (max_frames < 1 || max_frames > 65535) return fail(D2DH_E_ARG, "max_frames %d: must be 1..65535", max_frames);
    if (max_trail < 0 || max_trail > (1 << 20)) return fail(D2DH_E_ARG, "max_trail %d: must be 0..2^20", max_trail);
    if (max_shades < 0 || max_shades > D2DH_MAX_SHADES)
        return fail(D2DH_E_ARG, "max_shades %d: must be 0..%d", max_shades, D2DH_MAX_SHADES);
    if (max_width < D2DR_MIN_SIZE || max_width > D2DR_MAX_SIZE || max_height < D2DR_MIN_SIZE || max_height > D2DR_MAX_SIZE)
        return fail(D2DH_E_ARG, "max size %d x %d: width and height must be %d..%d", max_width, max_height,
                    D2DR_MIN_SIZE, D2DR_MAX_SIZE);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(D2DH_E_HIP, "cannot select HIP device %d", device);
    d2dh_ctx* c = new (std::nothrow) d2dh_ctx();
    if (!c) return fail(D2DH_E_NOMEM, "out of host memory");
    c->device = device, c->max_frames = max_frames, c->max_trail = max_trail, c->max_shades = max_shades;
    c->max_width = max_width, c->max_height = max_height;
    c->cap = ext_len(max_trail, max_shades);
    c->prims = nullptr, c->text = nullptr;
    const size_t pb = (size_t)max_frames * (size_t)c->cap * sizeof(Prim);
    const size_t tb = (size_t)max_frames * D2DH_TEXT_LINES * D2DH_LINE_CHARS;
    if (hipMalloc((void**)&c->prims, pb) != hipSuccess || hipMalloc((void**)&c->text, tb) != hipSuccess) {
        (void)hipGetLastError();
        d2dh_destroy(c);
        return fail(D2DH_E_NOMEM, "cannot allocate %zu + %zu bytes of device workspace", pb, tb);
    }
    *out = c;
    return D2DH_OK;
}

void d2dh_destroy(d2dh_t* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->prims) (void)hipFree(c->prims);
    if (c->text) (void)hipFree(c->text);
    delete c;
}

int32_t d2dh_render(d2dh_t* c, const d2dr_view* view, int32_t n_frames, const d2d_scn* scn_dev, const double* state_dev,
                    const float* obs_dev, const float* act_dev, const float* trail_dev, const int32_t* trail_len_dev,
                    const float* info_dev, const double* shade_dev, const int32_t* shade_count_dev, uint8_t* out_dev,
                    void* stream) {
    if (!c) return fail(D2DH_E_ARG, "ctx is NULL");
    if (int32_t rc = check_view(view)) return rc;
    if (view->width > c->max_width || view->height > c->max_height)
        return fail(D2DH_E_ARG, "picture %d x %d exceeds the ctx capacity %d x %d", view->width, view->height,
                    c->max_width, c->max_height);
    if (n_frames < 0 || n_frames > c->max_frames)
        return fail(D2DH_E_ARG, "n_frames %d exceeds the ctx capacity %d", n_frames, c->max_frames);
    if (n_frames == 0) return D2DH_OK;
    if (!scn_dev || !state_dev || !out_dev) return fail(D2DH_E_ARG, "scn_dev, state_dev and out_dev must not be NULL");
    if ((trail_dev == nullptr) != (trail_len_dev == nullptr))
        return fail(D2DH_E_ARG, "trail_dev and trail_len_dev must both be given or both be NULL");
    if (trail_dev && c->max_trail < 1) return fail(D2DH_E_ARG, "a trail needs a ctx created with max_trail >= 1");
    if ((shade_dev == nullptr) != (shade_count_dev == nullptr))
        return fail(D2DH_E_ARG, "shade_dev and shade_count_dev must both be given or both be NULL");
    if (shade_dev && c->max_shades < 1) return fail(D2DH_E_ARG, "shades need a ctx created with max_shades >= 1");
    DeviceGuard guard(c->device);
    if (!guard.ok) return fail(D2DH_E_HIP, "cannot select HIP device %d", c->device);
    const View v = make_view(view, 0);
    const bool text = info_dev != nullptr && (v.layers & D2DH_L_TEXT);
    const int32_t ms = shade_dev ? c->max_shades : 0;
    const FrameArgs a{scn_dev,   state_dev,       obs_dev,  act_dev,      trail_dev, trail_len_dev, text ? info_dev : nullptr,
                      shade_dev, shade_count_dev, n_frames, c->max_trail, ms};
    hipStream_t s = (hipStream_t)stream;
    // the longest list of this call (<= cap) and the text lanes behind a frame's own list
    const int32_t slots = ext_len(trail_dev ? c->max_trail : 0, ms) + D2DH_TEXT_LINES;
    setup_kernel<<<dim3((unsigned)((slots + NT - 1) / NT), (unsigned)n_frames), NT, 0, s>>>(c->prims, c->cap, c->text, v, a);
    if (int32_t rc = launched("setup_kernel")) return rc;
    const unsigned tiles = (unsigned)(((v.W + TW - 1) / TW) * ((v.H + TH - 1) / TH));
    raster_kernel<<<dim3(tiles, (unsigned)n_frames), NT, 0, s>>>(c->prims, c->cap, text ? c->text : nullptr, v,
                                                                 trail_len_dev, c->max_trail, ms, out_dev);
    return launched("raster_kernel");
}

int32_t d2dh_shade_update(int32_t device, int32_t n_tracked, const int32_t* env_ids_dev, int32_t n_envs,
                          const double* state_dev, const uint8_t* term_dev, const uint8_t* trunc_dev, double distance,
                          int32_t max_shades, double* shade_dev, int32_t* shade_count_dev, double* last_dev, void* stream) {
    if (int32_t rc = check_update(n_tracked, env_ids_dev, n_envs, state_dev, term_dev, trunc_dev, distance, max_shades,
                                  shade_dev, shade_count_dev, last_dev))
        return rc;
    if (n_tracked == 0) return D2DH_OK;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(D2DH_E_HIP, "cannot select HIP device %d", device);
    shade_kernel<<<dim3((unsigned)((n_tracked + 63) / 64)), 64, 0, (hipStream_t)stream>>>(
        n_tracked, env_ids_dev, n_envs, state_dev, term_dev, trunc_dev, distance, max_shades, shade_dev, shade_count_dev,
        last_dev);
    return launched("shade_kernel");
}

int32_t d2dh_render_host(const d2dr_view* view, int32_t n_frames, const d2d_scn* scn, const double* state,
                         const float* obs, const float* act, const float* trail, const int32_t* trail_len,
                         int32_t max_trail, const float* info, const double* shade, const int32_t* shade_count,
                         int32_t max_shades, uint8_t* out) {
    if (int32_t rc = check_view(view)) return rc;
    if (n_frames < 0) return fail(D2DH_E_ARG, "n_frames %d is negative", n_frames);
    if (n_frames == 0) return D2DH_OK;
    if (!scn || !state || !out) return fail(D2DH_E_ARG, "scn, state and out must not be NULL");
    if ((trail == nullptr) != (trail_len == nullptr))
        return fail(D2DH_E_ARG, "trail and trail_len must both be given or both be NULL");
    if (trail && max_trail < 1) return fail(D2DH_E_ARG, "a trail needs max_trail >= 1");
    if ((shade == nullptr) != (shade_count == nullptr))
        return fail(D2DH_E_ARG, "shade and shade_count must both be given or both be NULL");
    if (shade && (max_shades < 1 || max_shades > D2DH_MAX_SHADES))
        return fail(D2DH_E_ARG, "shades need max_shades 1..%d", D2DH_MAX_SHADES);
    render_host(view, n_frames, scn, state, obs, act, trail, trail_len, max_trail, info, shade, shade_count, max_shades,
                out);
    return D2DH_OK;
}

int32_t d2dh_shade_update_host(int32_t n_tracked, const int32_t* env_ids, int32_t n_envs, const double* state,
                               const uint8_t* term, const uint8_t* trunc, double distance, int32_t max_shades,
                               double* shade, int32_t* shade_count, double* last) {
    if (int32_t rc = check_update(n_tracked, env_ids, n_envs, state, term, trunc, distance, max_shades, shade,
                                  shade_count, last))
        return rc;
    for (int32_t k = 0; k < n_tracked; ++k)
        if (env_ids[k] < 0 || env_ids[k] >= n_envs)
            return fail(D2DH_E_ARG, "env_ids[%d] = %d is outside the batch of %d envs", k, env_ids[k], n_envs);
    for (int32_t k = 0; k < n_tracked; ++k)
        shade_step(k, env_ids, n_envs, state, term, trunc, distance, max_shades, shade, shade_count, last);
    return D2DH_OK;
}

int32_t d2dh_format_host(float value, char out[16]) {
    if (!out) return fail(D2DH_E_ARG, "out is NULL");
    format_value(value, out);
    return D2DH_OK;
}

int32_t d2dh_glyph_host(int32_t ch, uint8_t rows[7]) {
    if (!rows) return fail(D2DH_E_ARG, "rows is NULL");
    for (int r = 0; r < 7; ++r) rows[r] = (uint8_t)d2dh_glyph_row((int)ch, r);
    return D2DH_OK;
}

}  // extern "C"
