// libd2d_heat.so -- arena maps (include/d2d_heat.h): one launch per env step bins every live env's
// position, and every finished episode's spawn and end, into uint32 planes over the arena.  Equal keys
// are combined in the wave (ballot) and in the workgroup (an LDS hash table) before one integer atomic
// per distinct key reaches the planes; d2d_heat_colour paints the planes over background frames.
#include <hip/hip_runtime.h>

#include "d2d_heat.h"
#include "drone2d.h"
#include "d2d_heat_core.h"

namespace {

constexpr int BLOCK = D2D_HEAT_CHUNK;  // four waves, one env per lane
constexpr int PLANES = D2D_HEAT_PLANES;
constexpr int TABLE = D2D_HEAT_TABLE;
constexpr int DEPOSITS = 4;  // per env and step at most: visit, spawn, spawn by class, end
constexpr unsigned EMPTY = 0xFFFFFFFFu;
// a chunk inserts at most BLOCK * DEPOSITS new keys: the table is emptied before a chunk that could
// take it past TABLE - 1 slots, so a probe always finds its key or a free slot
constexpr unsigned FLUSH_ABOVE = TABLE - 1 - BLOCK * DEPOSITS;
static_assert((TABLE & (TABLE - 1)) == 0 && BLOCK * DEPOSITS < TABLE - 1, "table size");
static_assert((long long)D2D_HEAT_MAX_GROUPS * PLANES * (D2D_HEAT_MAX_GRID * D2D_HEAT_MAX_GRID + 1) < 0x7FFFFFFFll,
              "a key fits 31 bits");
static_assert(D2D_OBS_DIM == 27 && D2D_INFO_DIM == 12, "row strides");

// key = (group * 6 + plane) * (cells + 1) + slot, slot = the cell, or `cells` for outside
__device__ __forceinline__ unsigned make_key(int group, int plane, int cell, int cells) {
    return (unsigned)(group * PLANES + plane) * (unsigned)(cells + 1) + (unsigned)(cell < 0 ? cells : cell);
}

__device__ __forceinline__ void global_add(const d2d_heat_args& A, int cells, unsigned key, unsigned count) {
    const unsigned gp = key / (unsigned)(cells + 1), slot = key - gp * (unsigned)(cells + 1);
    unsigned* dst = slot == (unsigned)cells ? A.outside + gp : A.planes + (size_t)gp * cells + slot;
    atomicAdd(dst, count);  // (result unused: a non-returning atomic)
}

struct Table {
    unsigned* keys;
    unsigned* counts;
    unsigned* used;
};

__device__ __forceinline__ void table_add(const Table& T, unsigned key, unsigned count) {
    unsigned h = (key * 2654435761u) >> 20;  // 12 bits: TABLE slots
    static_assert(TABLE == 4096, "the hash keeps 12 bits");
    for (;;) {
        const unsigned prev = atomicCAS(&T.keys[h], EMPTY, key);
        if (prev == EMPTY) atomicAdd(T.used, 1u);
        if (prev == EMPTY || prev == key) {
            atomicAdd(&T.counts[h], count);
            return;
        }
        h = (h + 1) & (TABLE - 1);
    }
}

// Lanes of the wave with `active` and equal keys are found by ballot; the first of them adds for all.
template <bool LDS>
__device__ __forceinline__ void deposit(const d2d_heat_args& A, const Table& T, int cells, int lane, bool active,
                                        unsigned key) {
    unsigned long long left = __ballot(active);
    while (left != 0ull) {  // wave-uniform
        const int l = __builtin_amdgcn_readfirstlane(__ffsll(left) - 1);
        const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)key, l);
        const unsigned long long same = __ballot(active && key == k0);
        if (lane == l) {
            const unsigned count = (unsigned)__popcll(same);
            if (LDS)
                table_add(T, k0, count);
            else
                global_add(A, cells, k0, count);
        }
        left &= ~same;
    }
}

__device__ __forceinline__ void table_flush(const d2d_heat_args& A, const Table& T, int cells) {
    for (int s = threadIdx.x; s < TABLE; s += BLOCK) {
        const unsigned k = T.keys[s];
        if (k != EMPTY) {
            global_add(A, cells, k, T.counts[s]);
            T.keys[s] = EMPTY;
            T.counts[s] = 0u;
        }
    }
    if (threadIdx.x == 0) *T.used = 0u;
}

template <bool LDS>
__global__ __launch_bounds__(BLOCK) void d2d_heat_step_kernel(d2d_heat_args A) {
    __shared__ unsigned keys[LDS ? TABLE : 1];
    __shared__ unsigned counts[LDS ? TABLE : 1];
    __shared__ unsigned used;
    const Table T = {keys, counts, &used};
    const int tid = threadIdx.x, lane = tid & 63;
    const int cells = A.gx * A.gy;
    const int n_chunks = (A.n + BLOCK - 1) / BLOCK;
    if (LDS) {
        for (int s = tid; s < TABLE; s += BLOCK) {
            keys[s] = EMPTY;
            counts[s] = 0u;
        }
        if (tid == 0) used = 0u;
        __syncthreads();
    }
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        if (LDS) {
            if (used > FLUSH_ABOVE) {  // block-uniform: read between two barriers
                __syncthreads();
                table_flush(A, T, cells);
            }
            __syncthreads();
        }
        const int i = chunk * BLOCK + tid;
        bool live = false, done = false;
        int group = 0, cell = -1, spawn = -1, cls = D2D_HEAT_OTHER;
        if (i < A.n && A.alive[i] != 0) {
            live = true;
            done = (A.term[i] | A.trunc[i]) != 0;
            const float* p = (done ? A.terminal_obs : A.obs) + (size_t)i * D2D_OBS_DIM + 6;
            cell = d2d_heat_cell2(p[0], p[1], A.gx, A.gy);
            group = A.env_group != nullptr ? A.env_group[i] : 0;
            if (done) {
                spawn = A.spawn_cell[i];
                spawn = spawn < cells ? spawn : -1;
                cls = d2d_heat_class((int)A.info[(size_t)i * D2D_INFO_DIM + D2D_INFO_CAUSE]);
                A.alive[i] = 0;
            }
        }
        deposit<LDS>(A, T, cells, lane, live, make_key(group, D2D_HEAT_VISIT, cell, cells));
        if (__ballot(done) != 0ull) {  // wave-uniform; most steps end no episode in most waves
            deposit<LDS>(A, T, cells, lane, done, make_key(group, D2D_HEAT_SPAWN, spawn, cells));
            deposit<LDS>(A, T, cells, lane, done && cls != D2D_HEAT_OTHER,
                         make_key(group, cls == D2D_HEAT_SUCCESS ? D2D_HEAT_SPAWN_SUCCESS : D2D_HEAT_SPAWN_COLLISION,
                                  spawn, cells));
            deposit<LDS>(A, T, cells, lane, done && cls != D2D_HEAT_SUCCESS,
                         make_key(group, cls == D2D_HEAT_COLLIDED ? D2D_HEAT_END_COLLISION : D2D_HEAT_END_OTHER, cell,
                                  cells));
        }
        if (LDS) __syncthreads();  // `used` is final for this chunk
    }
    if (LDS) table_flush(A, T, cells);
}

__global__ __launch_bounds__(256) void d2d_heat_begin_kernel(d2d_heat_args A, const float* obs0) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += gridDim.x * blockDim.x) {
        const float* p = obs0 + (size_t)i * D2D_OBS_DIM + 6;
        A.alive[i] = 1;
        A.spawn_cell[i] = d2d_heat_cell2(p[0], p[1], A.gx, A.gy);
    }
}

// one workgroup per group: the maximum of plane_a, by integer max
__global__ __launch_bounds__(256) void d2d_heat_peak_kernel(d2d_heat_colour_args C) {
    __shared__ unsigned wmax[4];
    const int cells = C.gx * C.gy;
    const uint32_t* plane = C.planes + ((size_t)blockIdx.x * PLANES + C.plane_a) * cells;
    unsigned m = 0u;
    for (int c = threadIdx.x; c < cells; c += 256) m = plane[c] > m ? plane[c] : m;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) m = wmax[w] > m ? wmax[w] : m;
        C.peak[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(256) void d2d_heat_colour_kernel(d2d_heat_colour_args C) {
    const int cells = C.gx * C.gy;
    const size_t frame = (size_t)C.h * C.w, total = frame * (size_t)C.n_groups;
    for (size_t px = (size_t)blockIdx.x * 256 + threadIdx.x; px < total; px += (size_t)gridDim.x * 256) {
        const int k = (int)(px / frame);
        const size_t r = px - (size_t)k * frame;
        const int y = (int)(r / (size_t)C.w), x = (int)(r - (size_t)y * C.w);
        const int cell = (int)((int64_t)y * C.gy / C.h) * C.gx + (int)((int64_t)x * C.gx / C.w);
        const uint32_t* group = C.planes + (size_t)k * PLANES * cells;
        const uint32_t a = group[(size_t)C.plane_a * cells + cell];
        const uint8_t* bg = C.bg + (C.bg_shared ? r : px) * 3;
        int cr = 0, cg = 0, cb = 0;
        bool paint;
        if (C.mode == D2D_HEAT_DENSITY) {
            const int level = d2d_heat_level(a, C.peak[k]);
            paint = level > 0;
            d2d_heat_ramp(level, &cr, &cg, &cb);
        } else {
            const uint32_t den = group[(size_t)C.plane_b * cells + cell];
            paint = den >= (C.min_count > 1u ? C.min_count : 1u);
            if (paint) d2d_heat_rate_colour(d2d_heat_rate_level(a, den), &cr, &cg, &cb);
        }
        uint8_t* out = C.out + px * 3;
        out[0] = (uint8_t)(paint ? d2d_heat_blend(bg[0], cr, C.alpha) : bg[0]);
        out[1] = (uint8_t)(paint ? d2d_heat_blend(bg[1], cg, C.alpha) : bg[1]);
        out[2] = (uint8_t)(paint ? d2d_heat_blend(bg[2], cb, C.alpha) : bg[2]);
    }
}

bool grid_ok(int gx, int gy, int n_groups) {
    return gx >= 1 && gx <= D2D_HEAT_MAX_GRID && gy >= 1 && gy <= D2D_HEAT_MAX_GRID && n_groups >= 1 &&
           n_groups <= D2D_HEAT_MAX_GROUPS;
}

bool state_ok(const d2d_heat_args& A) {
    return A.n > 0 && A.n <= (1 << 30) && grid_ok(A.gx, A.gy, A.n_groups) && A.obs_dim == D2D_OBS_DIM && A.info_dim == D2D_INFO_DIM &&
           A.alive && A.spawn_cell && ((uintptr_t)A.spawn_cell & 3u) == 0 && ((uintptr_t)A.env_group & 3u) == 0;
}

bool planes_ok(const d2d_heat_args& A) {
    return A.planes && A.outside && ((uintptr_t)A.planes & 3u) == 0 && ((uintptr_t)A.outside & 3u) == 0;
}

int blocks_for(int n) {
    const int chunks = (n + BLOCK - 1) / BLOCK;
    return chunks < D2D_HEAT_MAX_BLOCKS ? chunks : D2D_HEAT_MAX_BLOCKS;
}

}  // namespace

extern "C" {

int32_t d2d_heat_abi_version(void) { return D2D_HEAT_ABI_VERSION; }

int32_t d2d_heat_begin(const d2d_heat_args* args, const float* obs0, void* stream) {
    if (args == nullptr || obs0 == nullptr || !state_ok(*args) || ((uintptr_t)obs0 & 3u) != 0)
        return (int32_t)hipErrorInvalidValue;
    hipLaunchKernelGGL(d2d_heat_begin_kernel, dim3(blocks_for(args->n)), dim3(256), 0, (hipStream_t)stream, *args, obs0);
    return (int32_t)hipGetLastError();
}

int32_t d2d_heat_step(const d2d_heat_args* args, void* stream) {
    if (args == nullptr) return (int32_t)hipErrorInvalidValue;
    const d2d_heat_args& A = *args;
    bool ok = state_ok(A) && planes_ok(A) && A.obs && A.terminal_obs && A.term && A.trunc && A.info;
    ok = ok && (((uintptr_t)A.obs | (uintptr_t)A.terminal_obs | (uintptr_t)A.info) & 3u) == 0;
    ok = ok && A.path >= D2D_HEAT_PATH_AUTO && A.path <= D2D_HEAT_PATH_GLOBAL;
    if (!ok) return (int32_t)hipErrorInvalidValue;
    const bool lds = A.path == D2D_HEAT_PATH_LDS || (A.path == D2D_HEAT_PATH_AUTO && A.gx * A.gy <= D2D_HEAT_LDS_MAX_CELLS);
    if (lds)
        hipLaunchKernelGGL(d2d_heat_step_kernel<true>, dim3(blocks_for(A.n)), dim3(BLOCK), 0, (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL(d2d_heat_step_kernel<false>, dim3(blocks_for(A.n)), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return (int32_t)hipGetLastError();
}

int32_t d2d_heat_clear(const d2d_heat_args* args, void* stream) {
    if (args == nullptr || !grid_ok(args->gx, args->gy, args->n_groups) || !planes_ok(*args))
        return (int32_t)hipErrorInvalidValue;
    const size_t rows = (size_t)args->n_groups * PLANES;
    hipError_t rc = hipMemsetAsync(args->planes, 0, rows * (size_t)args->gx * args->gy * sizeof(uint32_t), (hipStream_t)stream);
    if (rc == hipSuccess) rc = hipMemsetAsync(args->outside, 0, rows * sizeof(uint32_t), (hipStream_t)stream);
    return (int32_t)rc;
}

int32_t d2d_heat_colour(const d2d_heat_colour_args* args, void* stream) {
    if (args == nullptr) return (int32_t)hipErrorInvalidValue;
    const d2d_heat_colour_args& C = *args;
    bool ok = grid_ok(C.gx, C.gy, C.n_groups) && C.h >= 1 && C.h <= 16384 && C.w >= 1 && C.w <= 16384;
    ok = ok && (C.mode == D2D_HEAT_DENSITY || C.mode == D2D_HEAT_RATE) && C.plane_a >= 0 && C.plane_a < PLANES;
    ok = ok && (C.mode == D2D_HEAT_DENSITY || (C.plane_b >= 0 && C.plane_b < PLANES));
    ok = ok && C.alpha >= 0 && C.alpha <= 255 && (C.bg_shared == 0 || C.bg_shared == 1);
    ok = ok && C.planes && C.bg && C.out && ((uintptr_t)C.planes & 3u) == 0;
    ok = ok && (C.mode == D2D_HEAT_RATE || (C.peak && ((uintptr_t)C.peak & 3u) == 0));
    if (!ok) return (int32_t)hipErrorInvalidValue;
    if (C.mode == D2D_HEAT_DENSITY) {
        hipLaunchKernelGGL(d2d_heat_peak_kernel, dim3(C.n_groups), dim3(256), 0, (hipStream_t)stream, C);
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return (int32_t)rc;
    }
    const size_t total = (size_t)C.h * C.w * C.n_groups;
    const size_t want = (total + 255) / 256;
    hipLaunchKernelGGL(d2d_heat_colour_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0,
                       (hipStream_t)stream, C);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
