// d2d_eval_math.h -- device helpers of libd2d_eval.so: the actor's tanh and the policy-noise stream.
#ifndef D2D_EVAL_MATH_H
#define D2D_EVAL_MATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace d2d_eval {

// tanh as the PPO library's matrix-core forward computes it (csrc/d2d_ppo.hip ftanh): |x| < 0.25 an
// odd Taylor polynomial (next term < 3e-8 relative), else (1 - t) / (1 + t) with t = exp(-2 |x|)
// from v_exp_f32 and v_rcp_f32 (no cancellation: 1 - t >= 0.39); a few ulp.
__device__ __forceinline__ float ftanh(float x) {
    const float ax = fabsf(x), x2 = x * x;
    const float p = x * (1.0f + x2 * (-0.333333333f + x2 * (0.133333333f + x2 * (-0.0539682540f + x2 * 0.0218694885f))));
    const float t = __builtin_amdgcn_exp2f(ax * -2.88539008f);  // exp(-2 |x|)
    const float r = (1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t);
    return ax < 0.25f ? p : copysignf(r, x);
}

// Philox4x32-10: the env library's function (csrc/d2d_device.h philox, the oracle's d2dcpu_philox)
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

// The two N(0, 1) draws of global env g at step t (include/d2d_eval.h, mode 2): Box-Muller in float32
// on two 24-bit uniforms in (0, 1] -- (w >> 8) + 0.5 rounds to 2^24 for the largest w, so u = 1 and
// log u = 0 there; u is never 0.
__device__ __forceinline__ void policy_noise(uint64_t seed, uint32_t g, uint32_t t, uint32_t tag, float& z0, float& z1) {
    uint32_t o[4];
    philox(g, t, tag, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    const float u0 = ((float)(o[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;  // 2^-24
    const float u1 = ((float)(o[1] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u0));
    const float a = 6.28318530717958647692f * u1;
    z0 = r * cosf(a);
    z1 = r * sinf(a);
}

}  // namespace d2d_eval

#endif  // D2D_EVAL_MATH_H
