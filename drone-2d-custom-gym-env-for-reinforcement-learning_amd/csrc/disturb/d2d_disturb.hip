// libd2d_disturb.so -- disturbed evaluation (include/d2d_disturb.h): sensor noise and obstacle-sensor
// dropout on the observations the policy sees (d2d_disturb_obs), actuator noise, lag and motor loss on the
// actions the env gets (d2d_disturb_act); env i under level env_level[i] of a small parameter table.
#include <hip/hip_runtime.h>

#include "d2d_disturb.h"

namespace {

constexpr int OBS = D2D_DISTURB_OBS_DIM, ACT = D2D_DISTURB_ACT_DIM, NP = D2D_DISTURB_PARAMS;
constexpr int ROWS = D2D_DISTURB_HIST_ROWS, SLOTS = D2D_DISTURB_SLOTS;
constexpr int BLOCK = 256;      // four waves, one env per lane
constexpr int MAX_GRID = 2048;  // workgroups; a larger batch walks its chunks with this stride

// Philox4x32-10: the env library's function (csrc/d2d_device.h philox), as csrc/eval/d2d_eval_math.h has it
__device__ __forceinline__ void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                       uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// a 24-bit uniform in (0, 1]: (w >> 8) + 0.5 rounds to 2^24 for the largest w, so u = 1 there; never 0
__device__ __forceinline__ float uniform(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f; }

// Box-Muller in float32 on two uniforms, d2d_eval.h's formulas word for word
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, float& z0, float& z1) {
    const float u0 = uniform(w0), u1 = uniform(w1);
    const float r = sqrtf(-2.0f * logf(u0));
    const float a = 6.28318530717958647692f * u1;
    z0 = r * cosf(a);
    z1 = r * sinf(a);
}

__device__ __forceinline__ float clip1(float x) { return fminf(fmaxf(x, -1.0f), 1.0f); }

// The level of env i, or -1 for one outside the table (which then never indexes it).
__device__ __forceinline__ int level_of(const d2d_disturb_args& A, size_t i) {
    const int l = A.env_level[i];
    return (uint32_t)l < (uint32_t)A.n_levels ? l : -1;
}

// Observations: a workgroup takes 256 envs.  Their rows are 108 B each and contiguous, so the chunk comes in
// and goes out as one flat run of floats, lane after lane (the eval kernel's staging); in between lane l owns
// row l in LDS, where the odd row length keeps the 64 lanes of a wave on different banks.  The draws of mode 1
// and the returned draws are rows of the same kind read and written by their own lane: they serve tests, not
// the loop.
__global__ __launch_bounds__(BLOCK) void d2d_disturb_obs_kernel(d2d_disturb_args A) {
    __shared__ float xs[BLOCK * OBS];
    const int tid = threadIdx.x;
    const size_t n = (size_t)A.n;
    const size_t n_chunks = (n + BLOCK - 1) / BLOCK;
    for (size_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const size_t sb = chunk * BLOCK;
        const int rows = (int)(n - sb < (size_t)BLOCK ? n - sb : (size_t)BLOCK);
        const float* src = A.obs_in + sb * OBS;
        for (int e = tid; e < rows * OBS; e += BLOCK) xs[e] = src[e];
        __syncthreads();
        if (tid < rows) {
            const size_t i = sb + tid;
            float* x = xs + tid * OBS;
            const int level = level_of(A, i);
            float sigma = 0.0f, p_drop = 0.0f;
            if (level >= 0 && A.noise_mode != D2D_DISTURB_NOISE_NONE) {
                sigma = A.params[(size_t)level * NP + D2D_DISTURB_P_OBS_SIGMA];
                p_drop = A.params[(size_t)level * NP + D2D_DISTURB_P_DROPOUT];
            }
            const uint32_t g = (uint32_t)(A.env_id_base + (int64_t)i);
            const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
            const bool noisy = sigma != 0.0f;
#pragma unroll
            for (int b = 0; b < D2D_DISTURB_OBS_BLOCKS; ++b) {
                const uint32_t mb = noisy ? (A.obs_mask >> (4 * b)) & 0xFu : 0u;
                float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (mb != 0u) {
                    if (A.noise_mode == D2D_DISTURB_NOISE_GIVEN) {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (4 * b + k < OBS && ((mb >> k) & 1u)) z[k] = A.z_obs[i * OBS + 4 * b + k];
                    } else {
                        uint32_t w[4];
                        philox(g, (uint32_t)A.t, D2D_DISTURB_TAG_OBS, (uint32_t)b, k0, k1, w);
                        if (mb & 0x3u) box_muller(w[0], w[1], z[0], z[1]);
                        if (mb & 0xCu) box_muller(w[2], w[3], z[2], z[3]);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (4 * b + k < OBS) {
                            if ((mb >> k) & 1u) x[4 * b + k] = __fadd_rn(x[4 * b + k], __fmul_rn(sigma, z[k]));
                            else z[k] = 0.0f;  // a normal of the pair that no channel took
                        }
                    }
                }
                if (A.z_obs_out != nullptr) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (4 * b + k < OBS) A.z_obs_out[i * OBS + 4 * b + k] = z[k];
                }
            }
            float u[SLOTS] = {0.0f, 0.0f, 0.0f};
            if (p_drop != 0.0f) {
                if (A.noise_mode == D2D_DISTURB_NOISE_GIVEN) {
#pragma unroll
                    for (int j = 0; j < SLOTS; ++j) u[j] = A.u_drop[i * SLOTS + j];
                } else {
                    uint32_t w[4];
                    philox(g, (uint32_t)A.t, D2D_DISTURB_TAG_DROP, 0u, k0, k1, w);
#pragma unroll
                    for (int j = 0; j < SLOTS; ++j) u[j] = uniform(w[j]);
                }
#pragma unroll
                for (int j = 0; j < SLOTS; ++j) {
                    if (u[j] < p_drop) {
                        x[D2D_DISTURB_SLOT0 + 3 * j] = 1.0f;
                        x[D2D_DISTURB_SLOT0 + 3 * j + 1] = 0.0f;
                        x[D2D_DISTURB_SLOT0 + 3 * j + 2] = 0.0f;
                    }
                }
            }
            if (A.u_drop_out != nullptr) {
#pragma unroll
                for (int j = 0; j < SLOTS; ++j) A.u_drop_out[i * SLOTS + j] = u[j];
            }
        }
        __syncthreads();
        float* dst = A.obs_out + sb * OBS;
        for (int e = tid; e < rows * OBS; e += BLOCK) dst[e] = xs[e];
        __syncthreads();  // the next chunk's load overwrites xs
    }
}

// Actions: rows of 8 B, one float2 per lane, coalesced as they are.
__global__ __launch_bounds__(BLOCK) void d2d_disturb_act_kernel(d2d_disturb_args A) {
    const size_t n = (size_t)A.n;
    float2* act = reinterpret_cast<float2*>(A.act);
    float2* hist = reinterpret_cast<float2*>(A.hist);
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) {
        const int level = level_of(A, i);
        float z0 = 0.0f, z1 = 0.0f;
        if (level >= 0) {
            const float* p = A.params + (size_t)level * NP;
            const float sigma = A.noise_mode != D2D_DISTURB_NOISE_NONE ? p[D2D_DISTURB_P_ACT_SIGMA] : 0.0f;
            const float gl = p[D2D_DISTURB_P_GAIN_L], gr = p[D2D_DISTURB_P_GAIN_R];
            // clamped: whatever the table holds, the history is indexed inside its rows (NaN gives 0)
            const int delay = (int)fminf(fmaxf(p[D2D_DISTURB_P_DELAY], 0.0f), (float)D2D_DISTURB_MAX_DELAY);
            float2 a = act[i];
            if (sigma != 0.0f) {
                if (A.noise_mode == D2D_DISTURB_NOISE_GIVEN) {
                    z0 = A.z_act[i * ACT];
                    z1 = A.z_act[i * ACT + 1];
                } else {
                    uint32_t w[4];
                    philox((uint32_t)(A.env_id_base + (int64_t)i), (uint32_t)A.t, D2D_DISTURB_TAG_ACT, 0u, (uint32_t)A.seed,
                           (uint32_t)(A.seed >> 32), w);
                    box_muller(w[0], w[1], z0, z1);
                }
                a.x = clip1(__fadd_rn(a.x, __fmul_rn(sigma, z0)));
                a.y = clip1(__fadd_rn(a.y, __fmul_rn(sigma, z1)));
            }
            const int cur = A.t % ROWS;
            hist[(size_t)cur * n + i] = a;
            if (delay != 0) {
                const int from = (A.t > delay ? A.t - delay : 0) % ROWS;
                if (from != cur) a = hist[(size_t)from * n + i];  // (from == cur only at t = 0: the row just written)
            }
            if (gl != 1.0f) a.x = clip1(__fadd_rn(__fmul_rn(__fadd_rn(a.x, 1.0f), gl), -1.0f));
            if (gr != 1.0f) a.y = clip1(__fadd_rn(__fmul_rn(__fadd_rn(a.y, 1.0f), gr), -1.0f));
            act[i] = a;
        }
        if (A.z_act_out != nullptr) {
            A.z_act_out[i * ACT] = z0;
            A.z_act_out[i * ACT + 1] = z1;
        }
    }
}

bool common_ok(const d2d_disturb_args& A) {
    bool ok = A.n > 0 && A.t >= 0 && A.n_levels >= 1 && A.params && A.env_level;
    ok = ok && A.noise_mode >= D2D_DISTURB_NOISE_NONE && A.noise_mode <= D2D_DISTURB_NOISE_PHILOX;
    ok = ok && A.env_id_base >= 0 && A.env_id_base + (int64_t)A.n <= ((int64_t)1 << 32);
    return ok;
}

int grid_for(int n) {
    const int chunks = (n + BLOCK - 1) / BLOCK;
    return chunks < MAX_GRID ? chunks : MAX_GRID;
}

}  // namespace

extern "C" {

int32_t d2d_disturb_abi_version(void) { return D2D_DISTURB_ABI_VERSION; }

int32_t d2d_disturb_obs(const d2d_disturb_args* args, void* stream) {
    if (args == nullptr) return (int32_t)hipErrorInvalidValue;
    const d2d_disturb_args& A = *args;
    bool ok = common_ok(A) && A.obs_in && A.obs_out && A.obs_in != A.obs_out && (A.obs_mask >> OBS) == 0u;
    if (A.noise_mode == D2D_DISTURB_NOISE_GIVEN) ok = ok && A.z_obs && A.u_drop;
    if (!ok) return (int32_t)hipErrorInvalidValue;
    hipLaunchKernelGGL(d2d_disturb_obs_kernel, dim3(grid_for(A.n)), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return (int32_t)hipGetLastError();
}

int32_t d2d_disturb_act(const d2d_disturb_args* args, void* stream) {
    if (args == nullptr) return (int32_t)hipErrorInvalidValue;
    const d2d_disturb_args& A = *args;
    bool ok = common_ok(A) && A.act && A.hist && ((uintptr_t)A.act & 7u) == 0 && ((uintptr_t)A.hist & 7u) == 0;
    if (A.noise_mode == D2D_DISTURB_NOISE_GIVEN) ok = ok && A.z_act;
    if (!ok) return (int32_t)hipErrorInvalidValue;
    hipLaunchKernelGGL(d2d_disturb_act_kernel, dim3(grid_for(A.n)), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
