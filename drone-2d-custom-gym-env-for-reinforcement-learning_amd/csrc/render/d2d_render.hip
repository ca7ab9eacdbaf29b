// libd2d_render.so -- batched pictures of Drone2dEnv episodes (include/d2d_render.h).
//
// Three kernels over the shared code of d2d_raster.h:
//   setup_kernel    one lane per (frame, list slot): the frame's primitive list, fp64 -> fp32, into the
//                   ctx workspace (the per-frame work: trigonometry, path samples, nearest obstacle)
//   raster_kernel   one workgroup per 64 x 4 pixel tile (d2d_raster.h's tile walk, shared with
//                   libd2d_hud.so): culls the list against the tile 256 primitives at a time (ballot +
//                   compact into LDS, top of the list first), every pixel scans the survivors and stops
//                   at its first hit; the tile's RGB bytes are staged in LDS and leave as dwords (bytes
//                   only at a row's unaligned ends)
//   scatter_kernel  the plot: one lane per path segment, atomicMax(id[pixel], path + 1); the raster
//                   kernel's plot form resolves id -> rgb between the background and the colour bar
// No render call allocates or synchronises; all launches are ordered on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <new>
#include <string>

#include "d2d_raster.h"

using namespace d2dr;

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
    int32_t n_frames, max_trail;
};

__device__ __forceinline__ int32_t list_len(const View& v, const int32_t* trail_len, int32_t max_trail, int32_t f) {
    if (v.plot) return N_FIXED + D2DR_BAR_ROWS;
    const int32_t tl = trail_len ? clamp_len(trail_len[f], max_trail) : 0;
    return N_FIXED + (tl > 1 ? tl - 1 : 0);
}

__global__ __launch_bounds__(NT) void setup_kernel(Prim* __restrict__ prims, int32_t cap, View v, FrameArgs a) {
    const int32_t slot = (int32_t)(blockIdx.x * NT + threadIdx.x), f = (int32_t)blockIdx.y;
    if (slot >= list_len(v, a.trail_len, a.max_trail, f)) return;  // list_len <= cap (checked at the entry point)
    FrameIn in;
    in.scn = a.scn ? a.scn + f : nullptr;
    in.state = a.state, in.stride = a.n_frames, in.frame = f;
    in.obs = a.obs ? a.obs + (size_t)D2D_OBS_DIM * (size_t)f : nullptr;
    in.act = a.act ? a.act + (size_t)D2D_ACT_DIM * (size_t)f : nullptr;
    in.trail = a.trail ? a.trail + 2 * (size_t)a.max_trail * (size_t)f : nullptr;
    in.trail_len = a.trail_len ? clamp_len(a.trail_len[f], a.max_trail) : 0;
    prims[(size_t)f * (size_t)cap + (size_t)slot] = build_prim(in, v, slot);
}

// One tile of one frame (d2d_raster.h has the walk).  A frame's picture is its list over the background;
// the plot's is the colour bar, then the path ids, then the background list.
__global__ __launch_bounds__(NT) void raster_kernel(const Prim* __restrict__ prims, int32_t cap, View v,
                                                    const int32_t* __restrict__ trail_len, int32_t max_trail,
                                                    const uint32_t* __restrict__ ids, const uint8_t* __restrict__ rgb,
                                                    uint8_t* __restrict__ out) {
    __shared__ TileLds lds;
    const int32_t f = (int32_t)blockIdx.y;
    const Prim* fp = prims + (size_t)f * (size_t)cap;
    if (!v.plot) {
        walk_tile(
            fp, v, f, [&](int32_t fr) { return list_len(v, trail_len, max_trail, fr); },
            [](int32_t, int32_t) { return C_BG; }, lds, out);
        return;
    }
    const Tile q = tile_of(v);
    uint32_t colour = C_BG;
    bool hit = !q.inside;  // pixels past the picture's edge have nothing to find
    scan_range(fp, N_FIXED, list_len(v, trail_len, max_trail, f), q, hit, colour, lds);  // colour bar
    if (!hit) {
        const uint32_t id = ids[(size_t)q.row * (size_t)v.W + (size_t)q.col];
        if (id > 0u) {
            const uint8_t* c = rgb + 3 * (size_t)(id - 1u);
            colour = D2DR_RGB(c[0], c[1], c[2]);
            hit = true;
        }
    }
    scan_range(fp, 0, N_FIXED, q, hit, colour, lds);
    store_tile(v, q, f, colour, lds, out);
}

__global__ __launch_bounds__(NT) void scatter_kernel(View v, const float* __restrict__ xy, const int32_t* __restrict__ len,
                                                     int32_t n_paths, int32_t max_len, uint32_t* __restrict__ ids) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (size_t)(max_len - 1) * (size_t)n_paths) return;
    const int32_t m = (int32_t)(i % (size_t)n_paths), j = (int32_t)(i / (size_t)n_paths);
    const int32_t n = clamp_len(len[m], max_len);
    if (j + 1 >= n) return;
    const Prim q = plot_segment(xy, n, n_paths, m, j, v);
    if ((q.rgbk >> 24) == K_NONE) return;
    for (int32_t r = q.r0; r <= q.r1; ++r)  // the pixel box lies inside the picture (d2d_raster.h finish)
        for (int32_t c = q.c0; c <= q.c1; ++c)
            if (covers(q, r, c, pixel_x(v, c), pixel_y(v, r)))
                atomicMax(&ids[(size_t)r * (size_t)v.W + (size_t)c], (uint32_t)m + 1u);
}

struct DeviceGuard {  // launches go to the ctx's device; the caller's current device is put back
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
    if (!v) return fail(D2DR_E_ARG, "view is NULL");
    if (v->width < D2DR_MIN_SIZE || v->width > D2DR_MAX_SIZE || v->height < D2DR_MIN_SIZE || v->height > D2DR_MAX_SIZE)
        return fail(D2DR_E_ARG, "picture %d x %d: width and height must be %d..%d", v->width, v->height, D2DR_MIN_SIZE,
                    D2DR_MAX_SIZE);
    if (!(v->screen_w > 0.0) || !(v->screen_h > 0.0) || !finite_d(v->screen_w) || !finite_d(v->screen_h))
        return fail(D2DR_E_ARG, "screen_w and screen_h must be positive and finite");
    return D2DR_OK;
}

int32_t launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? D2DR_OK : fail(D2DR_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace

struct d2dr_ctx {
    int32_t device, max_frames, max_trail, max_width, max_height;
    int32_t cap;  // list slots per frame
    Prim* prims;
    uint32_t* ids;
};

extern "C" {

int32_t d2dr_abi_version(void) { return D2DR_ABI_VERSION; }
const char* d2dr_last_error(void) { return g_err.c_str(); }

int32_t d2dr_create(int32_t device, int32_t max_frames, int32_t max_trail, int32_t max_width, int32_t max_height,
                    d2dr_t** out) {
    if (!out) return fail(D2DR_E_ARG, "out is NULL");
    *out = nullptr;
    if (max_frames < 1 || max_frames > 65535) return fail(D2DR_E_ARG, "max_frames %d: must be 1..65535", max_frames);
    if (max_trail < 0 || max_trail > (1 << 20)) return fail(D2DR_E_ARG, "max_trail %d: must be 0..2^20", max_trail);
    if (max_width < D2DR_MIN_SIZE || max_width > D2DR_MAX_SIZE || max_height < D2DR_MIN_SIZE || max_height > D2DR_MAX_SIZE)
        return fail(D2DR_E_ARG, "max size %d x %d: width and height must be %d..%d", max_width, max_height,
                    D2DR_MIN_SIZE, D2DR_MAX_SIZE);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(D2DR_E_HIP, "cannot select HIP device %d", device);
    d2dr_ctx* c = new (std::nothrow) d2dr_ctx();
    if (!c) return fail(D2DR_E_NOMEM, "out of host memory");
    c->device = device, c->max_frames = max_frames, c->max_trail = max_trail;
    c->max_width = max_width, c->max_height = max_height;
    const int32_t extra = max_trail - 1 > D2DR_BAR_ROWS ? max_trail - 1 : D2DR_BAR_ROWS;
    c->cap = N_FIXED + extra;
    c->prims = nullptr, c->ids = nullptr;
    const size_t pb = (size_t)max_frames * (size_t)c->cap * sizeof(Prim);
    const size_t ib = (size_t)max_width * (size_t)max_height * sizeof(uint32_t);
    if (hipMalloc((void**)&c->prims, pb) != hipSuccess || hipMalloc((void**)&c->ids, ib) != hipSuccess) {
        (void)hipGetLastError();
        d2dr_destroy(c);
        return fail(D2DR_E_NOMEM, "cannot allocate %zu + %zu bytes of device workspace", pb, ib);
    }
    *out = c;
    return D2DR_OK;
}

void d2dr_destroy(d2dr_t* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    if (c->prims) (void)hipFree(c->prims);
    if (c->ids) (void)hipFree(c->ids);
    delete c;
}

int32_t d2dr_render(d2dr_t* c, const d2dr_view* view, int32_t n_frames, const d2d_scn* scn_dev, const double* state_dev,
                    const float* obs_dev, const float* act_dev, const float* trail_dev, const int32_t* trail_len_dev,
                    uint8_t* out_dev, void* stream) {
    if (!c) return fail(D2DR_E_ARG, "ctx is NULL");
    if (int32_t rc = check_view(view)) return rc;
    if (view->width > c->max_width || view->height > c->max_height)
        return fail(D2DR_E_ARG, "picture %d x %d exceeds the ctx capacity %d x %d", view->width, view->height,
                    c->max_width, c->max_height);
    if (n_frames < 0 || n_frames > c->max_frames)
        return fail(D2DR_E_ARG, "n_frames %d exceeds the ctx capacity %d", n_frames, c->max_frames);
    if (n_frames == 0) return D2DR_OK;
    if (!scn_dev || !state_dev || !out_dev) return fail(D2DR_E_ARG, "scn_dev, state_dev and out_dev must not be NULL");
    if ((trail_dev == nullptr) != (trail_len_dev == nullptr))
        return fail(D2DR_E_ARG, "trail_dev and trail_len_dev must both be given or both be NULL");
    if (trail_dev && c->max_trail < 1) return fail(D2DR_E_ARG, "a trail needs a ctx created with max_trail >= 1");
    DeviceGuard guard(c->device);
    if (!guard.ok) return fail(D2DR_E_HIP, "cannot select HIP device %d", c->device);
    const View v = make_view(view, 0);
    const FrameArgs a{scn_dev, state_dev, obs_dev, act_dev, trail_dev, trail_len_dev, n_frames, c->max_trail};
    hipStream_t s = (hipStream_t)stream;
    const int32_t slots = N_FIXED + (trail_dev && c->max_trail > 1 ? c->max_trail - 1 : 0);  // <= cap
    setup_kernel<<<dim3((unsigned)((slots + NT - 1) / NT), (unsigned)n_frames), NT, 0, s>>>(c->prims, c->cap, v, a);
    if (int32_t rc = launched("setup_kernel")) return rc;
    const unsigned tiles = (unsigned)(((v.W + TW - 1) / TW) * ((v.H + TH - 1) / TH));
    raster_kernel<<<dim3(tiles, (unsigned)n_frames), NT, 0, s>>>(c->prims, c->cap, v, trail_len_dev, c->max_trail,
                                                                 nullptr, nullptr, out_dev);
    return launched("raster_kernel");
}

int32_t d2dr_plot_paths(d2dr_t* c, const d2dr_view* view, const d2d_scn* scn_dev, const float* xy_dev,
                        const int32_t* len_dev, const uint8_t* rgb_dev, int32_t n_paths, int32_t max_len,
                        uint8_t* out_dev, void* stream) {
    if (!c) return fail(D2DR_E_ARG, "ctx is NULL");
    if (int32_t rc = check_view(view)) return rc;
    if (view->width > c->max_width || view->height > c->max_height)
        return fail(D2DR_E_ARG, "picture %d x %d exceeds the ctx capacity %d x %d", view->width, view->height,
                    c->max_width, c->max_height);
    if (n_paths < 0 || max_len < 0) return fail(D2DR_E_ARG, "n_paths and max_len must not be negative");
    if (n_paths == 0) return D2DR_OK;
    if (!out_dev || !xy_dev || !len_dev || !rgb_dev)
        return fail(D2DR_E_ARG, "out_dev, xy_dev, len_dev and rgb_dev must not be NULL");
    const size_t segs = (max_len > 1) ? (size_t)(max_len - 1) * (size_t)n_paths : 0;
    if (segs > (size_t)0x7fffffff * (size_t)NT / 2) return fail(D2DR_E_ARG, "too many path segments");
    DeviceGuard guard(c->device);
    if (!guard.ok) return fail(D2DR_E_HIP, "cannot select HIP device %d", c->device);
    const View v = make_view(view, 1);
    const FrameArgs a{scn_dev, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0};
    hipStream_t s = (hipStream_t)stream;
    const int32_t slots = N_FIXED + D2DR_BAR_ROWS;  // <= cap
    setup_kernel<<<dim3((unsigned)((slots + NT - 1) / NT), 1u), NT, 0, s>>>(c->prims, c->cap, v, a);
    if (int32_t rc = launched("setup_kernel")) return rc;
    if (hipMemsetAsync(c->ids, 0, (size_t)v.W * (size_t)v.H * sizeof(uint32_t), s) != hipSuccess)
        return fail(D2DR_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(hipGetLastError()));
    if (segs > 0) {
        scatter_kernel<<<dim3((unsigned)((segs + NT - 1) / NT)), NT, 0, s>>>(v, xy_dev, len_dev, n_paths, max_len, c->ids);
        if (int32_t rc = launched("scatter_kernel")) return rc;
    }
    const unsigned tiles = (unsigned)(((v.W + TW - 1) / TW) * ((v.H + TH - 1) / TH));
    raster_kernel<<<dim3(tiles, 1u), NT, 0, s>>>(c->prims, c->cap, v, nullptr, 0, c->ids, rgb_dev, out_dev);
    return launched("raster_kernel");
}

int32_t d2dr_render_host(const d2dr_view* view, int32_t n_frames, const d2d_scn* scn, const double* state,
                         const float* obs, const float* act, const float* trail, const int32_t* trail_len,
                         int32_t max_trail, uint8_t* out) {
    if (int32_t rc = check_view(view)) return rc;
    if (n_frames < 0) return fail(D2DR_E_ARG, "n_frames %d is negative", n_frames);
    if (n_frames == 0) return D2DR_OK;
    if (!scn || !state || !out) return fail(D2DR_E_ARG, "scn, state and out must not be NULL");
    if ((trail == nullptr) != (trail_len == nullptr))
        return fail(D2DR_E_ARG, "trail and trail_len must both be given or both be NULL");
    if (trail && max_trail < 1) return fail(D2DR_E_ARG, "a trail needs max_trail >= 1");
    render_host(view, n_frames, scn, state, obs, act, trail, trail_len, max_trail, out);
    return D2DR_OK;
}

int32_t d2dr_plot_paths_host(const d2dr_view* view, const d2d_scn* scn, const float* xy, const int32_t* len,
                             const uint8_t* rgb, int32_t n_paths, int32_t max_len, uint8_t* out) {
    if (int32_t rc = check_view(view)) return rc;
    if (n_paths < 0 || max_len < 0) return fail(D2DR_E_ARG, "n_paths and max_len must not be negative");
    if (n_paths == 0) return D2DR_OK;
    if (!out || !xy || !len || !rgb) return fail(D2DR_E_ARG, "out, xy, len and rgb must not be NULL");
    plot_paths_host(view, scn, xy, len, rgb, n_paths, max_len, out);
    return D2DR_OK;
}

int32_t d2dr_path_samples_host(const d2d_scn* scn, double* xy) {
    if (!scn || !xy) return fail(D2DR_E_ARG, "scn and xy must not be NULL");
    for (int32_t k = 0; k < D2DR_PATH_SAMPLES; ++k) path_sample(scn, k, xy + 2 * k, xy + 2 * k + 1);
    return D2DR_OK;
}

}  // extern "C"
