// libd2d_eval.so -- the fused evaluation step (include/d2d_eval.h): the first-episode recorder over env
// step t-1's outputs and the SB3 MlpPolicy actor + policy noise + clip for step t, one launch; with a
// policy bank (d2d_eval_step_bank) every env acts under the policy its map entry names; the sequenced
// step (d2d_eval_step_seq) reads the call index from device memory, so a captured loop replays.
#include <hip/hip_runtime.h>

#include <climits>

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
// a policy's image in the bank (include/d2d_eval.h): float offsets into its D2D_EVAL_BANK_STRIDE floats
constexpr int BK_B1 = HID * OBS, BK_W2 = BK_B1 + HID, BK_B2 = BK_W2 + HID * HID, BK_W3 = BK_B2 + HID;
constexpr int BK_B3 = BK_W3 + ACT * HID, BK_LOG_STD = BK_B3 + ACT;
static_assert(BK_LOG_STD + ACT == D2D_EVAL_BANK_STRIDE, "the bank's layout is the header's");
// How a bank launch deals chunks to workgroups once there are more than MAX_GRID of them: 1 = contiguous
// ranges of floor or ceil (chunks / workgroups) chunks each (a workgroup crosses few policy boundaries, so
// it rarely restages), 0 = the stride above.  Ranges measured faster (DESIGN.md "Policy bank");
// tools/bank_probe.py builds the other deal to measure it again.
#ifndef D2D_EVAL_BANK_DEAL
#define D2D_EVAL_BANK_DEAL 1
#endif

// The record half for env i (one lane of wave 0 each); returns whether the env finished its first
// episode at step t-1.  `flight_ok`: t - 1 is a row of flight (the host checked it for a by-value t).
__device__ __forceinline__ bool record_env(const d2d_eval_step_args& A, int i, int t, bool flight_ok) {
    const bool done = (A.prev_term[i] | A.prev_trunc[i]) != 0;
    const bool fin = A.finished[i] != 0;
    const bool fresh = done && !fin;
    if (fresh) {
        const float* src = A.prev_info + (size_t)i * A.info_dim;
        float* dst = A.rows + (size_t)i * A.info_dim;
        for (int k = 0; k < A.info_dim; ++k) dst[k] = src[k];
    }
    if (A.flight != nullptr && flight_ok && !fin) {
        const float* src = (done ? A.prev_term_obs : A.obs) + (size_t)i * OBS + 6;
        float* dst = A.flight + ((size_t)(t - 1) * A.n + i) * 2;
        dst[0] = src[0];
        dst[1] = src[1];
    }
    if (fresh) A.finished[i] = 1;
    return fresh;
}

__device__ __forceinline__ int wave_min(int v) {
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return __builtin_amdgcn_readfirstlane(v);
}

// The actor on the matrix cores (v_mfma_f32_32x32x2_f32, the tiling of the PPO library's forward):
// wave w computes the 32 (envs) x 32 (units) tile [envs 32 (w / 2) .., units 32 (w % 2) ..] of each hidden
// layer, D[i = env][j = unit] = sum_k A[i][k] B[k][j] with A = the layer input and B = W^T, both read
// from LDS (lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]).  Each D[i][j] is one fmaf
// chain over k = 0, 1, 2, ... whatever the tile holds elsewhere; the output layer is a 64-term fmaf
// loop per (env, action).  The weights (W1 [64][27], W2 [64][64] padded to 65, W3, biases: ~24 KB) are
// staged in LDS once per workgroup.
//
// BANK: env i acts under policy B.env_policy[i].  A chunk gets one pass per distinct policy among its
// rows, in ascending order (every wave finds the next one by the same min over the same 64 map
// entries, so the pass loop is uniform over the workgroup); a pass restages the LDS image when the
// policy is not the one already there, computes all 64 rows and keeps those whose policy it is.  A
// kept row therefore went through exactly the chains above with its own policy's weights: the action
// d2d_eval_step gives it under that policy alone.  An id outside [0, P) joins no pass.
//
// SEQ (d2d_eval_step_seq): the call index is *t_dev, read here by every workgroup, and what the host
// checks of a by-value t is decided here: the record half runs for t >= 1, flight is written for
// 1 <= t <= flight_cap only.  Nothing in this launch writes *t_dev (d2d_eval_seq_bump does, afterwards).
template <bool BANK, bool SEQ>
__global__ __launch_bounds__(BLOCK) void d2d_eval_step_kernel(d2d_eval_step_args A, d2d_eval_bank B,
                                                              const int32_t* t_dev) {
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
    const int t_call = SEQ ? *t_dev : A.t;
    const bool record = A.prev_term != nullptr && (!SEQ || t_call >= 1);
    const bool flight_ok = !SEQ || t_call <= A.flight_cap;
    auto stage = [&](const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                     const float* b3) {
        for (int e = tid; e < HID * OBS; e += BLOCK) w1s[e] = w1[e];
        for (int e = tid; e < HID * HID; e += BLOCK) w2s[(e >> 6) * HS + (e & 63)] = w2[e];
        if (tid < ACT * HID) w3s[tid >> 6][tid & 63] = w3[tid];
        if (tid < HID) {
            b1s[tid] = b1[tid];
            b2s[tid] = b2[tid];
        }
        if (tid < ACT) b3s[tid] = b3[tid];
    };
    if (!BANK && A.act) stage(A.w1, A.b1, A.w2, A.b2, A.w3, A.b3);
    int staged = -1;  // BANK: the policy whose image is in LDS
    const int n_chunks = (n + CHUNK - 1) / CHUNK;
    int c0 = blockIdx.x, c1 = n_chunks, dc = gridDim.x;
    if (BANK && D2D_EVAL_BANK_DEAL == 1) {
        c0 = (int)((int64_t)blockIdx.x * n_chunks / gridDim.x);
        c1 = (int)((int64_t)(blockIdx.x + 1) * n_chunks / gridDim.x);
        dc = 1;
    }
    // One pass over the chunk at env sb with the staged weights (BANK: policy cur's, staged here when
    // another's are in LDS; only the rows whose policy pid is cur are kept).
    auto pass = [&](int sb, bool first, int pid, int cur) {
        __syncthreads();       // the previous pass's epilogue has read outs; (first pass) weights staged
        if (BANK && cur != staged) {
            const float* p = B.params + (size_t)cur * D2D_EVAL_BANK_STRIDE;
            stage(p, p + BK_B1, p + BK_W2, p + BK_B2, p + BK_W3, p + BK_B3);
            staged = cur;
        }
        if (first) {
            for (int e = tid; e < CHUNK * OBS; e += BLOCK) {
                const int sl = e / OBS, k = e - sl * OBS;
                xs[sl][k] = sb + sl < n ? A.obs[(size_t)sb * OBS + e] : 0.0f;
            }
            if (tid < CHUNK) xs[tid][OBS] = 0.0f;  // the k padding of the 28-deep layer-1 product
        }
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
        if (tid < CHUNK && sb + tid < n && (!BANK || pid == cur)) {  // the epilogue: one env per lane of wave 0
            const int i = sb + tid;
            const float* log_std = BANK ? B.params + (size_t)cur * D2D_EVAL_BANK_STRIDE + BK_LOG_STD : A.log_std;
            float a0 = outs[0][tid], a1 = outs[1][tid];
            if (A.noise_mode != D2D_EVAL_NOISE_NONE) {
                float z0, z1;
                if (A.noise_mode == D2D_EVAL_NOISE_GIVEN) {
                    z0 = A.noise[2 * (size_t)i];
                    z1 = A.noise[2 * (size_t)i + 1];
                } else {
                    policy_noise(A.seed, (uint32_t)(A.env_id_base + i), (uint32_t)t_call, D2D_EVAL_NOISE_TAG, z0, z1);
                }
                if (A.noise_out != nullptr) {
                    A.noise_out[2 * (size_t)i] = z0;
                    A.noise_out[2 * (size_t)i + 1] = z1;
                }
                a0 = fmaf(expf(log_std[0]), z0, a0);
                a1 = fmaf(expf(log_std[1]), z1, a1);
            }
            A.act_env[2 * (size_t)i] = fminf(fmaxf(a0, -1.0f), 1.0f);
            A.act_env[2 * (size_t)i + 1] = fminf(fmaxf(a1, -1.0f), 1.0f);
        }
    };
    for (int chunk = c0; chunk < c1; chunk += dc) {
        const int sb = chunk * CHUNK;
        int pid = -1;  // BANK: this lane's row's policy, asked for first (the weight loads wait for it)
        if (BANK && A.act && sb + lane < n) pid = B.env_policy[sb + lane];
        if (record && w == 0) {  // wave 0, one env per lane
            const int i = sb + lane;
            const bool fresh = i < n && record_env(A, i, t_call, flight_ok);
            const int cnt = __popcll(__ballot(fresh));
            if (lane == 0 && cnt) atomicSub(A.remaining, cnt);
        }
        if (!A.act) continue;  // uniform over the grid
        if constexpr (!BANK) {
            pass(sb, true, 0, 0);
        } else {  // one pass per distinct policy of the chunk, ascending
            if ((uint32_t)pid >= (uint32_t)B.n_policies) pid = -1;  // no row, or an id outside the bank
            bool first = true;
            for (int cur = -1; (cur = wave_min(pid > cur ? pid : INT_MAX)) != INT_MAX; first = false)
                pass(sb, first, pid, cur);
        }
    }
}

// d2d_eval_step_seq's second launch: one thread moves the call index on once every workgroup of the step
// has read it (stream order), as d2d_ppo_permute's trailing launch moves its shuffle counter.
__global__ void d2d_eval_seq_bump(int32_t* t_dev) { t_dev[0] = t_dev[0] + 1; }

}  // namespace

extern "C" {

int32_t d2d_eval_abi_version(void) { return D2D_EVAL_ABI_VERSION; }

int32_t d2d_eval_bank_version(void) { return D2D_EVAL_BANK_VERSION; }

// Arguments that do not contradict each other; the actor comes from A (bank == nullptr) or from the bank.
// seq: the call index lives on the device, so what depends on it is the kernel's to decide.
static bool args_ok(const d2d_eval_step_args& A, const d2d_eval_bank* bank, bool seq = false) {
    const bool record = A.prev_term != nullptr;
    bool ok = A.n > 0 && A.t >= 0 && (A.act != 0 || record);
    if (bank) {
        ok = ok && bank->n_policies >= 1;
        ok = ok && !A.w1 && !A.b1 && !A.w2 && !A.b2 && !A.w3 && !A.b3 && !A.log_std;
    }
    if (A.act) {
        ok = ok && A.obs && A.act_env;
        if (bank) ok = ok && bank->params && bank->env_policy;
        else ok = ok && A.w1 && A.b1 && A.w2 && A.b2 && A.w3 && A.b3;
        ok = ok && A.noise_mode >= D2D_EVAL_NOISE_NONE && A.noise_mode <= D2D_EVAL_NOISE_PHILOX;
        if (A.noise_mode != D2D_EVAL_NOISE_NONE && !bank) ok = ok && A.log_std;
        if (A.noise_mode == D2D_EVAL_NOISE_GIVEN) ok = ok && A.noise;
        ok = ok && A.env_id_base >= 0 && A.env_id_base + (int64_t)A.n <= ((int64_t)1 << 32);
    }
    if (record) {
        ok = ok && A.prev_trunc && A.prev_info && A.finished && A.rows && A.remaining && A.info_dim > 0;
        if (A.flight) ok = ok && A.obs && A.prev_term_obs && (seq ? A.flight_cap >= 0 : A.t >= 1 && A.t <= A.flight_cap);
    } else {
        // a partly given record half is a caller's mistake, not a request to skip it
        ok = ok && !A.prev_trunc && !A.prev_info;
    }
    return ok;
}

static int grid_for(int n) {
    const int n_chunks = (n + CHUNK - 1) / CHUNK;
    return n_chunks < MAX_GRID ? n_chunks : MAX_GRID;
}

int32_t d2d_eval_step(const d2d_eval_step_args* args, void* stream) {
    if (args == nullptr || !args_ok(*args, nullptr)) return (int32_t)hipErrorInvalidValue;
    hipLaunchKernelGGL((d2d_eval_step_kernel<false, false>), dim3(grid_for(args->n)), dim3(BLOCK), 0, (hipStream_t)stream,
                       *args, d2d_eval_bank{}, (const int32_t*)nullptr);
    return (int32_t)hipGetLastError();
}

int32_t d2d_eval_step_bank(const d2d_eval_step_args* args, const d2d_eval_bank* bank, void* stream) {
    if (args == nullptr || bank == nullptr || !args_ok(*args, bank)) return (int32_t)hipErrorInvalidValue;
    hipLaunchKernelGGL((d2d_eval_step_kernel<true, false>), dim3(grid_for(args->n)), dim3(BLOCK), 0, (hipStream_t)stream,
                       *args, *bank, (const int32_t*)nullptr);
    return (int32_t)hipGetLastError();
}

int32_t d2d_eval_seq_version(void) { return D2D_EVAL_SEQ_VERSION; }

int32_t d2d_eval_step_seq(const d2d_eval_step_args* args, const d2d_eval_bank* bank, int32_t* t_dev, void* stream) {
    if (args == nullptr || t_dev == nullptr || args->t != 0 || !args_ok(*args, bank, true))
        return (int32_t)hipErrorInvalidValue;
    const dim3 grid(grid_for(args->n)), block(BLOCK);
    if (bank)
        hipLaunchKernelGGL((d2d_eval_step_kernel<true, true>), grid, block, 0, (hipStream_t)stream, *args, *bank,
                           (const int32_t*)t_dev);
    else
        hipLaunchKernelGGL((d2d_eval_step_kernel<false, true>), grid, block, 0, (hipStream_t)stream, *args,
                           d2d_eval_bank{}, (const int32_t*)t_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int32_t)e;
    hipLaunchKernelGGL(d2d_eval_seq_bump, dim3(1), dim3(1), 0, (hipStream_t)stream, t_dev);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
