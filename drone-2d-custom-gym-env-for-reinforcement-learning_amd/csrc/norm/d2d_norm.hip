// libd2d_norm.so -- reward normalisation in the rollout (include/d2d_norm.h): per env step one launch
// that advances the discounted returns and sums their moments per workgroup, and one that folds the
// moments into the running statistics and scales, clips and stores the rewards.  Every sum is taken in
// the fixed order the header states (no float atomics); the only atomic is an integer ticket.
#include <hip/hip_runtime.h>

#include <math.h>

#include "d2d_norm.h"

namespace {

constexpr int BLOCK = D2D_NORM_CHUNK;  // four waves, one env per lane
constexpr int WAVES = BLOCK / 64;
static_assert(WAVES == 4, "the chunk sum below adds four wave sums");

// the shuffle-down tree: lane 0 ends with the header's wave sum (the other lanes' values are not used)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
    return v;
}

__device__ __forceinline__ int chunks_of(int n) { return (n - 1) / BLOCK + 1; }

// steps 1 and 2 up to part[b]
__global__ __launch_bounds__(BLOCK) void d2d_norm_accumulate_kernel(d2d_norm_step_args A) {
    __shared__ double wsum[WAVES][2];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const size_t n = (size_t)A.n;
    const int n_chunks = chunks_of(A.n);
    const double c = A.rms[0];
    double row1 = 0.0, row2 = 0.0;  // thread 0 carries the workgroup's row
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const size_t i = (size_t)chunk * BLOCK + tid;
        double d = 0.0;
        if (i < n) {
            const double r = A.ret[i] * A.gamma + (double)A.rew[i];
            A.ret[i] = r;
            d = r - c;
        }
        const double s1 = wave_sum(d);
        const double s2 = wave_sum(d * d);
        if (lane == 0) {
            wsum[w][0] = s1;
            wsum[w][1] = s2;
        }
        __syncthreads();
        if (tid == 0) {
            row1 = row1 + (((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0]);
            row2 = row2 + (((wsum[0][1] + wsum[1][1]) + wsum[2][1]) + wsum[3][1]);
        }
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    if (tid == 0) {
        A.part[2 * (size_t)blockIdx.x] = row1;
        A.part[2 * (size_t)blockIdx.x + 1] = row2;
    }
}

// the fold and steps 3 to 5 (TRAINING), or step 4 with the stored variance
template <bool TRAINING>
__global__ __launch_bounds__(BLOCK) void d2d_norm_apply_kernel(d2d_norm_step_args A) {
    __shared__ double sh_scale;
    __shared__ double rows[TRAINING ? D2D_NORM_MAX_BLOCKS : 1][2];
    const int tid = threadIdx.x;
    const size_t n = (size_t)A.n;
    const int n_chunks = chunks_of(A.n);
    if (TRAINING) {
        // all lanes fetch the rows (one pass of independent loads); lane 0 then adds them in order
        for (int b = tid; b < A.n_blocks; b += BLOCK) {
            rows[b][0] = A.part[2 * (size_t)b];
            rows[b][1] = A.part[2 * (size_t)b + 1];
        }
        __syncthreads();
    }
    double mean = 0.0, var = 0.0, count = 0.0;  // thread 0: the new statistics
    if (tid == 0) {
        var = A.rms[1];
        if (TRAINING) {
            mean = A.rms[0];
            count = A.rms[2];
            double S1 = 0.0, S2 = 0.0;
            for (int b = 0; b < A.n_blocks; ++b) {
                S1 = S1 + rows[b][0];
                S2 = S2 + rows[b][1];
            }
            const double nn = (double)A.n;
            const double bm = S1 / nn;
            double bv = S2 / nn - bm * bm;
            if (bv < 0.0) bv = 0.0;
            const double tot = count + nn;
            const double M2 = var * count + bv * nn + bm * bm * count * nn / tot;
            mean = mean + bm * nn / tot;
            var = M2 / tot;
            count = tot;
        }
        sh_scale = sqrt(var + A.epsilon);
    }
    __syncthreads();
    if (TRAINING && tid == 0) {
        // Every workgroup has read the old rms by the time it draws its ticket (the release orders
        // this lane's reads before the add), so whoever draws the last one may overwrite it.  All
        // workgroups computed the same bits.
        const int t = __hip_atomic_fetch_add(A.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == (int)gridDim.x - 1) {
            A.rms[0] = mean;
            A.rms[1] = var;
            A.rms[2] = count;
            *A.ticket = 0;
        }
    }
    const double scale = sh_scale, clip = A.clip;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const size_t i = (size_t)chunk * BLOCK + tid;
        if (i < n) {
            double x = (double)A.rew[i] / scale;
            if (x < -clip) x = -clip;
            if (x > clip) x = clip;
            A.rew_out[i] = (float)x;
            if (TRAINING && (A.term[i] | A.trunc[i]) != 0) A.ret[i] = 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void d2d_norm_reset_kernel(int n, double* ret, double* rms) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * blockDim.x)
        ret[i] = 0.0;
    if (rms != nullptr && blockIdx.x == 0 && threadIdx.x < 3) rms[threadIdx.x] = threadIdx.x == 0 ? 0.0 : threadIdx.x == 1 ? 1.0 : 1e-4;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) == 0; }

}  // namespace

extern "C" {

int32_t d2d_norm_abi_version(void) { return D2D_NORM_ABI_VERSION; }

int32_t d2d_norm_step(const d2d_norm_step_args* args, void* stream) {
    if (args == nullptr) return (int32_t)hipErrorInvalidValue;
    const d2d_norm_step_args& A = *args;
    bool ok = A.n >= 1 && A.n_blocks >= 1 && A.n_blocks <= D2D_NORM_MAX_BLOCKS && (A.training == 0 || A.training == 1);
    ok = ok && A.clip >= 0.0 && A.epsilon >= 0.0 && A.gamma == A.gamma;  // (a NaN fails each comparison)
    ok = ok && A.rew && A.rew_out && A.rms && aligned(A.rew, 4) && aligned(A.rew_out, 4) && aligned(A.rms, 8);
    if (ok && A.training)
        ok = A.term && A.trunc && A.ret && A.part && A.ticket && aligned(A.ret, 8) && aligned(A.part, 8) &&
             aligned(A.ticket, 4);
    if (!ok) return (int32_t)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    if (A.training) {
        hipLaunchKernelGGL(d2d_norm_accumulate_kernel, dim3(A.n_blocks), dim3(BLOCK), 0, st, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int32_t)e;
        hipLaunchKernelGGL(d2d_norm_apply_kernel<true>, dim3(A.n_blocks), dim3(BLOCK), 0, st, A);
    } else {
        hipLaunchKernelGGL(d2d_norm_apply_kernel<false>, dim3(A.n_blocks), dim3(BLOCK), 0, st, A);
    }
    return (int32_t)hipGetLastError();
}

int32_t d2d_norm_reset(int32_t n, double* ret, double* rms, void* stream) {
    if (n < 1 || !ret || !aligned(ret, 8) || !aligned(rms, 8)) return (int32_t)hipErrorInvalidValue;
    const int grid = (n - 1) / 256 + 1 < 1024 ? (n - 1) / 256 + 1 : 1024;
    hipLaunchKernelGGL(d2d_norm_reset_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (int)n, ret, rms);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
