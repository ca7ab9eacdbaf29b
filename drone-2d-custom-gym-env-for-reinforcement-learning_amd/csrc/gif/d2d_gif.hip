// libd2d_gif.so -- device frames into GIF89a frame chunks (include/d2d_gif.h).
//
// Two kernels over the shared code of d2d_gif_core.h:
//   index_kernel   one lane per pixel: RGB -> palette index (the palette and its hash in LDS), the compare with
//                  the stream's canvas, the delta image; the changed bounding box by wave min / max and one
//                  integer atomic per wave; the `inexact` count by ballot and one integer atomic per wave
//   lzw_kernel     one wave per stream: lane s compresses segment s with its own dictionary (global
//                  workspace) into its own staging buffer; a wave prefix sum of the bit lengths; then the
//                  lanes write the chunk byte by byte, each byte gathered from the staging buffers (a
//                  two-pass merge: no atomics on the output, the bytes do not depend on timing)
// No call allocates or synchronises; all launches are ordered on the caller's stream.  Integer atomics only.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <new>
#include <string>

#include "d2d_gif_core.h"

using namespace d2dg;

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

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void index_kernel(const PalTable* __restrict__ pal, int32_t W, int32_t H,
                                                   const uint8_t* __restrict__ frames,
                                                   const uint8_t* __restrict__ active, const uint8_t* __restrict__ has,
                                                   uint8_t* __restrict__ canvas, uint8_t* __restrict__ delta,
                                                   int32_t* __restrict__ bbox, int32_t* __restrict__ inexact) {
    __shared__ uint32_t rgb[256];
    __shared__ uint16_t hash[PAL_HASH];
    const int32_t k = (int32_t)blockIdx.y;
    if (active != nullptr && active[k] == 0) return;  // uniform over the block
    const int32_t tid = (int32_t)threadIdx.x;
    rgb[tid] = pal->rgb[tid];
    hash[tid] = pal->hash[tid];
    hash[tid + NT] = pal->hash[tid + NT];
    __syncthreads();
    const int32_t n = pal->n;
    const bool hf = has[k] != 0;
    const int64_t n_all = (int64_t)W * H;
    const int64_t p = (int64_t)blockIdx.x * NT + tid;
    bool inex = false, ch = false;
    int32_t x = 0, y = 0;
    if (p < n_all) {
        const int64_t q = n_all * k + p;
        delta[q] = index_pixel(rgb, hash, n, frames + 3 * q, hf, canvas + q, &inex, &ch);
        y = (int32_t)(p / W), x = (int32_t)(p - (int64_t)y * W);
    }
    const int32_t lane = tid & 63;
    const unsigned long long miss = __ballot(inex);
    if (inexact != nullptr && miss != 0ull && lane == 0) atomicAdd(inexact + k, (int32_t)__popcll(miss));
    if (!hf) return;  // a first frame is the whole picture (uniform)
    int32_t x0 = ch ? x : INT_MAX, y0 = ch ? y : INT_MAX, x1 = ch ? x : -1, y1 = ch ? y : -1;
    for (int d = 32; d >= 1; d >>= 1) {
        x0 = min(x0, __shfl_xor(x0, d));
        y0 = min(y0, __shfl_xor(y0, d));
        x1 = max(x1, __shfl_xor(x1, d));
        y1 = max(y1, __shfl_xor(y1, d));
    }
    if (lane == 0 && x1 >= 0) {
        atomicMin(bbox + 4 * k, x0);
        atomicMin(bbox + 4 * k + 1, y0);
        atomicMax(bbox + 4 * k + 2, x1);
        atomicMax(bbox + 4 * k + 3, y1);
    }
}

__global__ __launch_bounds__(D2DG_SEGMENTS) void lzw_kernel(const PalTable* __restrict__ pal, int32_t W, int32_t H,
                                                             const uint8_t* __restrict__ active, uint8_t* __restrict__ has,
                                                             const uint8_t* __restrict__ delta, int32_t* __restrict__ bbox,
                                                             uint16_t* __restrict__ slots, uint32_t* __restrict__ ents,
                                                             uint32_t* __restrict__ stages, int64_t sw, int32_t delay_cs,
                                                             uint8_t* __restrict__ chunk, int64_t cap,
                                                             int32_t* __restrict__ len) {
    __shared__ uint32_t off[D2DG_SEGMENTS + 1];
    const int32_t k = (int32_t)blockIdx.x, lane = (int32_t)threadIdx.x;
    if (active != nullptr && active[k] == 0) {  // uniform
        if (lane == 0) len[k] = 0;
        return;
    }
    const bool hf = has[k] != 0;
    int32_t* bb = bbox + 4 * k;
    const Rect rc = frame_rect(hf, W, H, bb[0], bb[1], bb[2], bb[3]);
    __syncthreads();  // every lane has read the box and the flag
    if (lane == 0) {  // ready for the stream's next frame
        bb[0] = INT_MAX, bb[1] = INT_MAX, bb[2] = -1, bb[3] = -1;
        has[k] = 1;
    }
    const int32_t m = pal->m;
    const int64_t n = (int64_t)rc.w * rc.h, seg = seg_pixels(n);
    const int32_t live = (int32_t)((n + seg - 1) / seg);
    const int64_t p0 = lane * seg, p1 = (p0 + seg < n) ? p0 + seg : n;
    const size_t me = (size_t)k * D2DG_SEGMENTS + (size_t)lane;
    uint32_t bits = 0u;
    if (p0 < n)
        bits = lzw_segment(delta + (int64_t)W * H * k, W, rc, p0, p1, m, lane == 0, lane == live - 1, slots + me * SLOTS,
                           ents + me * D2DG_DICT_CAP, stages + me * (size_t)sw, nullptr);
    uint32_t v = bits;  // inclusive wave prefix sum
    for (int d = 1; d < D2DG_SEGMENTS; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    off[lane + 1] = v;
    if (lane == 0) off[0] = 0u;
    __syncthreads();  // the offsets, and every lane's staging words (global, workgroup scope)
    const uint32_t data = data_bytes(off[D2DG_SEGMENTS]);
    uint8_t* out = chunk + cap * k;  // chunk_len(data) <= d2dg_frame_cap(W, H) <= cap (checked at the entry point)
    if (lane < HDR) out[lane] = header_byte(lane, rc, hf, delay_cs, pal->n, m);
    const uint32_t* st = stages + (size_t)k * D2DG_SEGMENTS * (size_t)sw;
    for (uint32_t j = (uint32_t)lane; j < data; j += D2DG_SEGMENTS) out[data_pos(j)] = merge_byte(st, sw, off, j);
    for (uint32_t t = (uint32_t)lane; t < n_blocks(data); t += D2DG_SEGMENTS)
        out[(uint32_t)HDR + 256u * t] = (uint8_t)(data - 255u * t < 255u ? data - 255u * t : 255u);
    if (lane == 0) {
        out[chunk_len(data) - 1u] = 0;
        len[k] = (int32_t)chunk_len(data);
    }
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

int32_t check_size(int32_t w, int32_t h) {
    if (w < D2DG_MIN_SIZE || w > D2DG_MAX_SIZE || h < D2DG_MIN_SIZE || h > D2DG_MAX_SIZE)
        return fail(D2DG_E_ARG, "picture %d x %d: width and height must be %d..%d", w, h, D2DG_MIN_SIZE, D2DG_MAX_SIZE);
    return D2DG_OK;
}

int32_t check_palette(const uint8_t* rgb, int32_t n) {
    if (n < 1 || n > D2DG_MAX_COLOURS) return fail(D2DG_E_ARG, "palette of %d colours: must be 1..%d", n, D2DG_MAX_COLOURS);
    if (!rgb) return fail(D2DG_E_ARG, "palette_rgb is NULL");
    return D2DG_OK;
}

int32_t check_encode(int32_t n_streams, int32_t w, int32_t h, const void* frames, int32_t delay_cs, const void* chunk,
                     int64_t cap, const void* len) {
    if (n_streams < 0) return fail(D2DG_E_ARG, "n_streams %d is negative", n_streams);
    if (int32_t rc = check_size(w, h)) return rc;
    if (delay_cs < 0 || delay_cs > 65535) return fail(D2DG_E_ARG, "delay_cs %d: must be 0..65535", delay_cs);
    if (cap < frame_cap(w, h))
        return fail(D2DG_E_ARG, "chunk rows of %lld bytes: a %d x %d frame needs d2dg_frame_cap = %lld", (long long)cap, w, h,
                    (long long)frame_cap(w, h));
    if (n_streams > 0 && (!frames || !chunk || !len)) return fail(D2DG_E_ARG, "frames, chunk and len must not be NULL");
    return D2DG_OK;
}

int32_t launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? D2DG_OK : fail(D2DG_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace

struct d2dg_ctx {
    int32_t device, max_streams, max_width, max_height;
    int32_t w, h;  // the size of the running GIFs (0: none yet)
    int64_t sw;    // staging words per lane
    PalTable* pal;
    uint8_t *has, *canvas, *delta;
    int32_t* bbox;
    uint16_t* slots;
    uint32_t *ents, *stages;
};

extern "C" {

int32_t d2dg_abi_version(void) { return D2DG_ABI_VERSION; }
const char* d2dg_last_error(void) { return g_err.c_str(); }
int32_t d2dg_dict_cap(void) { return D2DG_DICT_CAP; }

int64_t d2dg_frame_cap(int32_t width, int32_t height) {
    if (width < D2DG_MIN_SIZE || width > D2DG_MAX_SIZE || height < D2DG_MIN_SIZE || height > D2DG_MAX_SIZE) return 0;
    return frame_cap(width, height);
}

int32_t d2dg_create(int32_t device, int32_t max_streams, int32_t max_width, int32_t max_height, const uint8_t* palette_rgb,
                    int32_t n_colours, d2dg_t** out) {
    if (!out) return fail(D2DG_E_ARG, "out is NULL");
    *out = nullptr;
    if (max_streams < 1 || max_streams > D2DG_MAX_STREAMS)
        return fail(D2DG_E_ARG, "max_streams %d: must be 1..%d", max_streams, D2DG_MAX_STREAMS);
    if (int32_t rc = check_size(max_width, max_height)) return rc;
    if (int32_t rc = check_palette(palette_rgb, n_colours)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(D2DG_E_HIP, "cannot select HIP device %d", device);
    d2dg_ctx* c = new (std::nothrow) d2dg_ctx();
    if (!c) return fail(D2DG_E_NOMEM, "out of host memory");
    c->device = device, c->max_streams = max_streams, c->max_width = max_width, c->max_height = max_height;
    const size_t K = (size_t)max_streams, px = (size_t)max_width * (size_t)max_height, lanes = K * D2DG_SEGMENTS;
    c->sw = stage_words(seg_pixels((int64_t)px));
    const size_t bytes[8] = {sizeof(PalTable), K,           K * px, K * px, K * 4 * sizeof(int32_t), lanes * SLOTS * sizeof(uint16_t),
                             lanes * D2DG_DICT_CAP * sizeof(uint32_t), lanes * (size_t)c->sw * sizeof(uint32_t)};
    void** ptrs[8] = {(void**)&c->pal,  (void**)&c->has,   (void**)&c->canvas, (void**)&c->delta,
                      (void**)&c->bbox, (void**)&c->slots, (void**)&c->ents,   (void**)&c->stages};
    size_t total = 0;
    bool ok = true;
    for (int i = 0; i < 8 && ok; ++i) total += bytes[i], ok = hipMalloc(ptrs[i], bytes[i]) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        d2dg_destroy(c);
        return fail(D2DG_E_NOMEM, "cannot allocate %zu bytes of device workspace", total);
    }
    PalTable pal;
    build_pal(palette_rgb, n_colours, &pal);
    std::string box(K * 4 * sizeof(int32_t), '\0');
    for (size_t k = 0; k < K; ++k) {
        const int32_t b[4] = {INT_MAX, INT_MAX, -1, -1};
        memcpy(&box[k * sizeof b], b, sizeof b);
    }
    // (the dictionaries and staging buffers need no initial value: d2d_gif_core.h)
    if (hipMemcpy(c->pal, &pal, sizeof pal, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->bbox, box.data(), box.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(c->has, 0, K) != hipSuccess) {
        const hipError_t e = hipGetLastError();
        d2dg_destroy(c);
        return fail(D2DG_E_HIP, "cannot initialise the workspace: %s", hipGetErrorString(e));
    }
    *out = c;
    return D2DG_OK;
}

void d2dg_destroy(d2dg_t* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    void* ptrs[8] = {c->pal, c->has, c->canvas, c->delta, c->bbox, c->slots, c->ents, c->stages};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete c;
}

int32_t d2dg_restart(d2dg_t* c, void* stream) {
    if (!c) return fail(D2DG_E_ARG, "ctx is NULL");
    DeviceGuard guard(c->device);
    if (!guard.ok) return fail(D2DG_E_HIP, "cannot select HIP device %d", c->device);
    const hipError_t e = hipMemsetAsync(c->has, 0, (size_t)c->max_streams, (hipStream_t)stream);
    if (e != hipSuccess) return fail(D2DG_E_HIP, "restart: %s", hipGetErrorString(e));
    c->w = c->h = 0;
    return D2DG_OK;
}

int32_t d2dg_encode(d2dg_t* c, int32_t n_streams, int32_t width, int32_t height, const uint8_t* frames_dev,
                    const uint8_t* active_dev, int32_t delay_cs, uint8_t* chunk_dev, int64_t cap, int32_t* len_dev,
                    int32_t* inexact_dev, void* stream) {
    if (!c) return fail(D2DG_E_ARG, "ctx is NULL");
    if (int32_t rc = check_encode(n_streams, width, height, frames_dev, delay_cs, chunk_dev, cap, len_dev)) return rc;
    if (width > c->max_width || height > c->max_height)
        return fail(D2DG_E_ARG, "picture %d x %d exceeds the ctx capacity %d x %d", width, height, c->max_width,
                    c->max_height);
    if (n_streams > c->max_streams)
        return fail(D2DG_E_ARG, "n_streams %d exceeds the ctx capacity %d", n_streams, c->max_streams);
    if (c->w != 0 && (c->w != width || c->h != height))
        return fail(D2DG_E_ARG, "picture %d x %d: the running GIFs are %d x %d (d2dg_restart begins new ones)", width, height,
                    c->w, c->h);
    if (n_streams == 0) return D2DG_OK;
    DeviceGuard guard(c->device);
    if (!guard.ok) return fail(D2DG_E_HIP, "cannot select HIP device %d", c->device);
    hipStream_t s = (hipStream_t)stream;
    const int64_t px = (int64_t)width * height;
    index_kernel<<<dim3((unsigned)((px + NT - 1) / NT), (unsigned)n_streams), NT, 0, s>>>(
        c->pal, width, height, frames_dev, active_dev, c->has, c->canvas, c->delta, c->bbox, inexact_dev);
    if (int32_t rc = launched("index_kernel")) return rc;
    c->w = width, c->h = height;
    lzw_kernel<<<dim3((unsigned)n_streams), D2DG_SEGMENTS, 0, s>>>(c->pal, width, height, active_dev, c->has, c->delta,
                                                                    c->bbox, c->slots, c->ents, c->stages, c->sw, delay_cs,
                                                                    chunk_dev, cap, len_dev);
    return launched("lzw_kernel");
}

int32_t d2dg_encode_host(int32_t n_streams, int32_t width, int32_t height, const uint8_t* palette_rgb, int32_t n_colours,
                         const uint8_t* frames, const uint8_t* active, int32_t delay_cs, uint8_t* canvas,
                         uint8_t* has_frame, uint8_t* chunk, int64_t cap, int32_t* len, int32_t* inexact,
                         int32_t* mid_clears) {
    if (int32_t rc = check_palette(palette_rgb, n_colours)) return rc;
    if (int32_t rc = check_encode(n_streams, width, height, frames, delay_cs, chunk, cap, len)) return rc;
    if (n_streams == 0) return D2DG_OK;
    if (!canvas || !has_frame) return fail(D2DG_E_ARG, "canvas and has_frame must not be NULL");
    PalTable pal;
    build_pal(palette_rgb, n_colours, &pal);
    encode_host(n_streams, width, height, pal, frames, active, delay_cs, canvas, has_frame, chunk, cap, len, inexact,
                mid_clears);
    return D2DG_OK;
}

int32_t d2dg_file_header_host(int32_t width, int32_t height, const uint8_t* palette_rgb, int32_t n_colours, int32_t loop,
                              uint8_t* out, int32_t out_cap, int32_t* out_len) {
    if (int32_t rc = check_palette(palette_rgb, n_colours)) return rc;
    if (int32_t rc = check_size(width, height)) return rc;
    if (!out || !out_len) return fail(D2DG_E_ARG, "out and out_len must not be NULL");
    if (loop > 65535) return fail(D2DG_E_ARG, "loop %d: must be at most 65535", loop);
    PalTable pal;
    build_pal(palette_rgb, n_colours, &pal);
    const int32_t need = 13 + 3 * (1 << pal.bits) + (loop >= 0 ? 19 : 0);
    if (out_cap < need) return fail(D2DG_E_ARG, "out holds %d bytes: the header needs %d", out_cap, need);
    *out_len = file_header(width, height, pal, loop, out);
    return D2DG_OK;
}

int32_t d2dg_model_palette(uint8_t* out) {
    if (!out) return fail(D2DG_E_ARG, "out is NULL");
    for (int i = 0; i < D2DG_MODEL_COLOURS; ++i) {
        const uint32_t c = MODEL_PALETTE[i];
        out[3 * i] = (uint8_t)(c & 255u), out[3 * i + 1] = (uint8_t)((c >> 8) & 255u), out[3 * i + 2] = (uint8_t)((c >> 16) & 255u);
    }
    return D2DG_OK;
}

}  // extern "C"
