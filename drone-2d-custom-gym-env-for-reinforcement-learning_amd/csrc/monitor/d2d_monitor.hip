// libd2d_monitor.so -- the episode monitor (include/d2d_monitor.h): one launch per env step digests the
// step's term / trunc / info rows into per-env running sums and, at episode ends, into per-workgroup
// partial rows, summed in the fixed order the header states (no float atomics).
#include <hip/hip_runtime.h>

#include <math.h>

#include "d2d_monitor.h"
#include "drone2d.h"

namespace {

constexpr int K = D2D_MON_K, TERMS = D2D_MON_TERMS;
constexpr int BLOCK = D2D_MON_CHUNK;  // four waves, one env per lane
constexpr int WAVES = BLOCK / 64;
static_assert(D2D_INFO_DIM == 12 && D2D_INFO_CA == 0 && D2D_INFO_AA == TERMS - 1, "a row is three float4 words");

// v of lane l (wave-uniform l) in every lane
__device__ __forceinline__ double lane_get(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(BLOCK) void d2d_monitor_step_kernel(d2d_monitor_step_args A) {
    __shared__ double wsum[WAVES][K];
    __shared__ int wany[WAVES];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const size_t n = (size_t)A.n;
    const int n_chunks = (A.n + BLOCK - 1) / BLOCK;
    double row = tid < K ? A.part[(size_t)blockIdx.x * K + tid] : 0.0;  // thread k carries column k of the row
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const size_t i = (size_t)chunk * BLOCK + tid;
        bool event = false, was_live = false;
        float4 a = {}, b = {}, c = {};
        double r[TERMS] = {};
        float m = 0.0f;
        if (i < n) {
            const float4* p = reinterpret_cast<const float4*>(A.info) + 3 * i;
            a = p[0];  // CA PA PP COLL
            b = p[1];  // REACH AA DCLOSE STEPS
            c = p[2];  // CAUSE APE TOTREW REWARD
            const float t[TERMS] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
            for (int f = 0; f < TERMS; ++f) r[f] = A.run[f * n + i] + (double)t[f];
            m = A.minclr[i];
            m = b.z < m ? b.z : m;
            event = (A.term[i] | A.trunc[i]) != 0;
            if (event) {
                was_live = A.live[i] != 0;
#pragma unroll
                for (int f = 0; f < TERMS; ++f) A.run[f * n + i] = 0.0;
                A.minclr[i] = INFINITY;
                A.live[i] = 1;
            } else {
#pragma unroll
                for (int f = 0; f < TERMS; ++f) A.run[f * n + i] = r[f];
                A.minclr[i] = m;
            }
        }
        const unsigned long long events = __ballot(event);
        if (events != 0ull) {  // wave-uniform
            double v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = 0.0;
            if (event && was_live) {
                const int cause = (int)c.x;
                const bool c1 = cause & D2D_END_COLLISION, c2 = cause & D2D_END_REACH;
                const bool c4 = cause & D2D_END_TIMEUP, c5 = cause & D2D_END_AA;
                const float t[TERMS] = {a.x, a.y, a.z, a.w, b.x, b.y};
                v[D2D_MON_EPISODES] = 1.0;
                v[D2D_MON_SUCCESS] = c2 ? 1.0 : 0.0;
                v[D2D_MON_FAIL] = (c1 || c4 || c5) ? 1.0 : 0.0;
                v[D2D_MON_COLLISION] = (c1 && !c2 && !c4 && !c5) ? 1.0 : 0.0;
                v[D2D_MON_TIMEUP] = c4 ? 1.0 : 0.0;
                v[D2D_MON_AA] = c5 ? 1.0 : 0.0;
                v[D2D_MON_LEN] = (double)b.w;
                v[D2D_MON_TOTREW] = (double)c.z;
                v[D2D_MON_APE] = (double)c.y;
#pragma unroll
                for (int f = 0; f < TERMS; ++f) {
                    v[D2D_MON_RUN + f] = r[f];
                    v[D2D_MON_LAST + f] = (double)t[f];
                }
                v[D2D_MON_LAST_REWARD] = (double)c.w;
                const bool fin = isfinite(m);
                v[D2D_MON_MINCLR] = fin ? (double)m : 0.0;
                v[D2D_MON_MINCLR_N] = fin ? 1.0 : 0.0;
            } else if (event) {
                v[D2D_MON_SKIPPED] = 1.0;
            }
            double acc[K];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = 0.0;
            for (unsigned long long left = events; left != 0ull; left &= left - 1ull) {  // ascending lanes
                const int l = __builtin_amdgcn_readfirstlane(__ffsll(left) - 1);
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] = acc[k] + lane_get(v[k], l);
            }
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) wsum[w][k] = acc[k];
            }
        }
        if (lane == 0) wany[w] = events != 0ull;
        __syncthreads();
        if (tid < K) {
            bool any = false;
            double t = 0.0;
#pragma unroll
            for (int ww = 0; ww < WAVES; ++ww) {
                if (wany[ww]) {
                    t = t + wsum[ww][tid];
                    any = true;
                }
            }
            if (any) row = row + t;
        }
        __syncthreads();  // wsum / wany are rewritten by the next chunk
    }
    if (tid < K) A.part[(size_t)blockIdx.x * K + tid] = row;
}

__global__ __launch_bounds__(64) void d2d_monitor_flush_kernel(double* part, int n_blocks, double* out) {
    const int k = threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b) {
        s = s + part[(size_t)b * K + k];
        part[(size_t)b * K + k] = 0.0;
    }
    out[k] = s != s ? __longlong_as_double(0x7FF8000000000000ll) : s;
}

__global__ __launch_bounds__(256) void d2d_monitor_reset_kernel(int n, double* run, float* minclr, uint8_t* live,
                                                                uint8_t live_value) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int f = 0; f < TERMS; ++f) run[(size_t)f * n + i] = 0.0;
        minclr[i] = INFINITY;
        live[i] = live_value;
    }
}

bool blocks_ok(int n_blocks) { return n_blocks >= 1 && n_blocks <= D2D_MON_MAX_BLOCKS; }

}  // namespace

extern "C" {

int32_t d2d_monitor_abi_version(void) { return D2D_MON_ABI_VERSION; }

int32_t d2d_monitor_step(const d2d_monitor_step_args* args, void* stream) {
    if (args == nullptr) return (int32_t)hipErrorInvalidValue;
    const d2d_monitor_step_args& A = *args;
    bool ok = A.n > 0 && A.info_dim == D2D_INFO_DIM && blocks_ok(A.n_blocks);
    ok = ok && A.term && A.trunc && A.info && A.run && A.minclr && A.live && A.part;
    ok = ok && ((uintptr_t)A.info & 15u) == 0 && ((uintptr_t)A.run & 7u) == 0 && ((uintptr_t)A.part & 7u) == 0 &&
         ((uintptr_t)A.minclr & 3u) == 0;
    if (!ok) return (int32_t)hipErrorInvalidValue;
    hipLaunchKernelGGL(d2d_monitor_step_kernel, dim3(A.n_blocks), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return (int32_t)hipGetLastError();
}

int32_t d2d_monitor_flush(double* part, int32_t n_blocks, double* out, void* stream) {
    if (!part || !out || !blocks_ok(n_blocks) || ((uintptr_t)part & 7u) || ((uintptr_t)out & 7u))
        return (int32_t)hipErrorInvalidValue;
    hipLaunchKernelGGL(d2d_monitor_flush_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, (int)n_blocks, out);
    return (int32_t)hipGetLastError();
}

int32_t d2d_monitor_reset(int32_t n, double* run, float* minclr, uint8_t* live, int32_t live_value, void* stream) {
    if (n <= 0 || !run || !minclr || !live || (live_value != 0 && live_value != 1) || ((uintptr_t)run & 7u) ||
        ((uintptr_t)minclr & 3u))
        return (int32_t)hipErrorInvalidValue;
    const int grid = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
    hipLaunchKernelGGL(d2d_monitor_reset_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (int)n, run, minclr, live,
                       (uint8_t)live_value);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
