// libd2d_eval.so -- the fused evaluation step (include/d2d_eval.h): the first-episode recorder over env
// step t-1's outputs and the SB3 MlpPolicy actor + policy noise + clip for step t, one launch.
#include <hip/hip_runtime.h>

#include "d2d_eval.h"
#include "d2d_eval_math.h"

namespace {

using namespace d2d_eval;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int OBS = D2D_EVAL_OBS_DIM, HID = D2D_EVAL_HIDDEN, ACT = D2D_EVAL_ACT_DIM;
constexpr int BLOCK = 256;            // four waves
constexpr int TILE = 32, CHUNK = 64;  // a workgroup pass takes 64 envs: two 32-row matrix-core tiles
constexpr int XS = OBS + 2, HS = HID + 1;  // LDS row strides (odd: a 32-lane half never shares a bank)
constexpr int MAX_GRID = 1024;        // workgroups; a larger batch walks its chunks with this stride

// The record half for env i (one lane of wave 0 each); returns whether the env finished its first
// episode at step t-1.
__device__ __forceinline__ bool record_env(const d2d_eval_step_args& A, int i) {
    const bool done = (A.prev_term[i] | A.prev_trunc[i]) != 0;
    const bool fin = A.finished[i] != 0;
    const bool fresh = done && !fin;
    if (fresh) {
        const float* src = A.prev_info + (size_t)i * A.info_dim;
        float* dst = A.rows + (size_t)i * A.info_dim;
        for (int k = 0; k < A.info_dim; ++k) dst[k] = src[k];
    }
    if (A.flight != nullptr && !fin) {
        const float* src = (done ? A.prev_term_obs : A.obs) + (size_t)i * OBS + 6;
        float* dst = A.flight + ((size_t)(A.t - 1) * A.n + i) * 2;
        dst[0] = src[0];
        dst[1] = src[1];
    }
    if (fresh) A.finished[i] = 1;
    return fresh;
}

// The actor on the matrix cores (v_mfma_f32_32x32x2_f32, the tiling of the PPO library's forward):
// wave w computes the 32 (envs) x 32 (units) tile [envs 32 (w / 2) .., units 32 (w % 2) ..] of each hidden
// layer, D[i = env][j = unit] = sum_k A[i][k] B[k][j] with A = the layer input and B = W^T, both read
// from LDS (lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]).  Each D[i][j] is one fmaf
// chain over k = 0, 1, 2, ... whatever the tile holds elsewhere; the output layer is a 64-term fmaf
// loop per (env, action).  The weights (W1 [64][27], W2 [64][64] padded to 65, W3, biases: ~24 KB) are
// staged in LDS once per workgroup.
__global__ __launch_bounds__(BLOCK) void d2d_eval_step_kernel(d2d_eval_step_args A) {
    __shared__ float w1s[HID * OBS];
    __shared__ float w2s[HID * HS];
    __shared__ float w3s[ACT][HID];
    __shared__ float b1s[HID], b2s[HID], b3s[ACT];
    __shared__ float xs[CHUNK][XS];
    __shared__ float hs[CHUNK][HS];
    __shared__ float outs[ACT][CHUNK];
    const int tid = threadIdx.x, n = A.n;
    const int w = tid >> 6, lane = tid & 63, ci = lane & 31, h = lane >> 5;
    const int r0 = (w >> 1) * TILE, j0 = (w & 1) * TILE;  // this wave's env rows and units
    const bool record = A.prev_term != nullptr;
    if (A.act) {
        for (int e = tid; e < HID * OBS; e += BLOCK) w1s[e] = A.w1[e];
        for (int e = tid; e < HID * HID; e += BLOCK) w2s[(e >> 6) * HS + (e & 63)] = A.w2[e];
        if (tid < ACT * HID) w3s[tid >> 6][tid & 63] = A.w3[tid];
        if (tid < HID) {
            b1s[tid] = A.b1[tid];
            b2s[tid] = A.b2[tid];
        }
        if (tid < ACT) b3s[tid] = A.b3[tid];
    }
    const int n_chunks = (n + CHUNK - 1) / CHUNK;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int sb = chunk * CHUNK;
        if (record && w == 0) {  // wave 0, one env per lane
            const int i = sb + lane;
            const bool fresh = i < n && record_env(A, i);
            const int cnt = __popcll(__ballot(fresh));
            if (lane == 0 && cnt) atomicSub(A.remaining, cnt);
        }
        if (!A.act) continue;  // uniform over the grid
        __syncthreads();       // the previous chunk's epilogue has read outs; (first pass) weights staged
        for (int e = tid; e < CHUNK * OBS; e += BLOCK) {
            const int sl = e / OBS, k = e - sl * OBS;
            xs[sl][k] = sb + sl < n ? A.obs[(size_t)sb * OBS + e] : 0.0f;
        }
        if (tid < CHUNK) xs[tid][OBS] = 0.0f;  // the k padding of the 28-deep layer-1 product
        __syncthreads();
        // layer 1 (k = 27 inputs, padded to 28)
        f32x16 acc = {};
#pragma unroll
        for (int t = 0; t < (OBS + 1) / 2; ++t) {
            const int k = 2 * t + h;
            const float b = k < OBS ? w1s[(j0 + ci) * OBS + k] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[r0 + ci][k], b, acc, 0, 0, 0);
        }
        {
            const float b1 = b1s[j0 + ci];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = (v & 3) + 8 * (v >> 2) + 4 * h;  // env row of register v (C/D map)
                hs[r0 + i][j0 + ci] = ftanh(acc[v] + b1);
            }
        }
        __syncthreads();
        // layer 2
        acc = f32x16{};
#pragma unroll
        for (int t = 0; t < HID / 2; ++t) {
            const int k = 2 * t + h;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(hs[r0 + ci][k], w2s[(j0 + ci) * HS + k], acc, 0, 0, 0);
        }
        __syncthreads();  // every wave has read h1 before h2 overwrites it
        {
            const float b2 = b2s[j0 + ci];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = (v & 3) + 8 * (v >> 2) + 4 * h;
                hs[r0 + i][j0 + ci] = ftanh(acc[v] + b2);
            }
        }
        __syncthreads();
        // output layer: thread -> (action tid / 64, env tid % 64)
        if (tid < ACT * CHUNK) {
            const int d = tid >> 6, sl = tid & 63;
            float o = b3s[d];
#pragma unroll 16
            for (int j = 0; j < HID; ++j) o = fmaf(w3s[d][j], hs[sl][j], o);
            outs[d][sl] = o;
        }
        __syncthreads();
        if (tid < CHUNK && sb + tid < n) {  // the epilogue: one env per lane of wave 0
            const int i = sb + tid;
            float a0 = outs[0][tid], a1 = outs[1][tid];
            if (A.noise_mode != D2D_EVAL_NOISE_NONE) {
                float z0, z1;
                if (A.noise_mode == D2D_EVAL_NOISE_GIVEN) {
                    z0 = A.noise[2 * (size_t)i];
                    z1 = A.noise[2 * (size_t)i + 1];
                } else {
                    policy_noise(A.seed, (uint32_t)(A.env_id_base + i), (uint32_t)A.t, D2D_EVAL_NOISE_TAG, z0, z1);
                }
                if (A.noise_out != nullptr) {
                    A.noise_out[2 * (size_t)i] = z0;
                    A.noise_out[2 * (size_t)i + 1] = z1;
                }
                a0 = fmaf(expf(A.log_std[0]), z0, a0);
                a1 = fmaf(expf(A.log_std[1]), z1, a1);
            }
            A.act_env[2 * (size_t)i] = fminf(fmaxf(a0, -1.0f), 1.0f);
            A.act_env[2 * (size_t)i + 1] = fminf(fmaxf(a1, -1.0f), 1.0f);
        }
    }
}

}  // namespace

extern "C" {

int32_t d2d_eval_abi_version(void) { return D2D_EVAL_ABI_VERSION; }

int32_t d2d_eval_step(const d2d_eval_step_args* args, void* stream) {
    if (args == nullptr) return (int32_t)hipErrorInvalidValue;
    const d2d_eval_step_args& A = *args;
    const bool record = A.prev_term != nullptr;
    bool ok = A.n > 0 && A.t >= 0 && (A.act != 0 || record);
    if (A.act) {
        ok = ok && A.obs && A.w1 && A.b1 && A.w2 && A.b2 && A.w3 && A.b3 && A.act_env;
        ok = ok && A.noise_mode >= D2D_EVAL_NOISE_NONE && A.noise_mode <= D2D_EVAL_NOISE_PHILOX;
        if (A.noise_mode != D2D_EVAL_NOISE_NONE) ok = ok && A.log_std;
        if (A.noise_mode == D2D_EVAL_NOISE_GIVEN) ok = ok && A.noise;
        ok = ok && A.env_id_base >= 0 && A.env_id_base + (int64_t)A.n <= ((int64_t)1 << 32);
    }
    if (record) {
        ok = ok && A.prev_trunc && A.prev_info && A.finished && A.rows && A.remaining && A.info_dim > 0;
        if (A.flight) ok = ok && A.obs && A.prev_term_obs && A.t >= 1 && A.t <= A.flight_cap;
    } else {
        // a partly given record half is a caller's mistake, not a request to skip it
        ok = ok && !A.prev_trunc && !A.prev_info;
    }
    if (!ok) return (int32_t)hipErrorInvalidValue;
    const int n_chunks = (A.n + CHUNK - 1) / CHUNK;
    const int grid = n_chunks < MAX_GRID ? n_chunks : MAX_GRID;
    hipLaunchKernelGGL(d2d_eval_step_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
