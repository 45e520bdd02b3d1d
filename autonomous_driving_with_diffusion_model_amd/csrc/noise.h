// Noise stream v1 (DESIGN.md "Noise stream", include/adx.h): standard normals as a pure function of
// (seed, tick, slot, element).  One __device__ definition, shared by the scheduler step kernels and the fill kernels of
// csrc/sched.hip, so that every consumer agrees bit for bit.
//
//   words   Philox4x32-10, key = (seed lo, seed hi), counter = (e >> 2, slot, tick lo, tick hi)
//   normal  element e takes z[e & 3] of the Box-Muller pairs (w0, w1) -> z0, z1 and (w2, w3) -> z2, z3 with
//           u = ((w >> 8) + 0.5) * 2^-24, r = sqrt(-2 ln u_a), z = r cos(2 pi u_b) | r sin(2 pi u_b)
//
// u = (2k + 1) * 2^-25 needs 25 significand bits once k >= 2^23, one more than fp32 has.  The evaluation below therefore folds
// the upper half onto the lower one, where every quantity IS exact in fp32: with m = 2^24 - 1 - k and v = (m + 0.5) * 2^-24
// = 1 - u,  ln u = log1p(-v),  cos(2 pi u) = cos(2 pi v),  sin(2 pi u) = -sin(2 pi v).  The angle goes through the pi-scaled
// functions (cos(2 pi v) = cospi(2 v), 2 v exact), so no rounded multiple of pi enters.  Accurate libm calls only.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace adx {

struct NoiseWords { uint32_t w[4]; };

// state: {seed_lo, seed_hi, tick_lo, tick_hi} in device memory, read on every launch (a captured graph sees the current values)
__device__ __forceinline__ NoiseWords noise_words_at(const uint32_t* state, uint32_t slot, uint64_t e) {
  uint32_t k0 = state[0], k1 = state[1];
  uint32_t c0 = (uint32_t)(e >> 2), c1 = slot, c2 = state[2], c3 = state[3];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1;
    c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  NoiseWords o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

__device__ __forceinline__ uint32_t noise_word_at(const uint32_t* state, uint32_t slot, uint64_t e) {
  const NoiseWords o = noise_words_at(state, slot, e);
  const uint32_t l = (uint32_t)e & 3u;
  return l == 0 ? o.w[0] : (l == 1 ? o.w[1] : (l == 2 ? o.w[2] : o.w[3]));
}

__device__ __forceinline__ float noise_normal_at(const uint32_t* state, uint32_t slot, uint64_t e) {
#pragma clang fp contract(off)
  const NoiseWords o = noise_words_at(state, slot, e);
  const uint32_t l = (uint32_t)e & 3u;
  const uint32_t ka = ((l & 2u) ? o.w[2] : o.w[0]) >> 8, kb = ((l & 2u) ? o.w[3] : o.w[1]) >> 8;
  const bool fa = ka >= (1u << 23), fb = kb >= (1u << 23);
  const uint32_t ma = fa ? 0xFFFFFFu - ka : ka, mb = fb ? 0xFFFFFFu - kb : kb;
  const float va = ((float)ma + 0.5f) * 0x1p-24f;        // u_a (or 1 - u_a), exact
  const float vb2 = ((float)mb + 0.5f) * 0x1p-23f;       // 2 u_b (or 2 (1 - u_b)), exact, in (0, 1)
  const float lg = fa ? log1pf(-va) : logf(va);
  const float r = sqrtf(-2.0f * lg);
  float t;
  if (l & 1u) {
    const float s = sinpif(vb2);
    t = fb ? -s : s;
  } else {
    t = cospif(vb2);
  }
  return r * t;
}

}  // namespace adx
