// Counter-based Gaussian noise for the ancestral samplers (vx_overlap_ancestral_step).
//
// Generator: Philox4x32-10 exactly as in Random123 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
// key increments 0x9E3779B9 / 0xBB67AE85, 10 rounds.  Known answers (counter; key -> output):
//   0 0 0 0;  0 0                                     -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
//   ffffffff x4;  ffffffff x2                         -> 408f276d 41c83b0e a20bc7c6 6d5451fd
//   243f6a88 85a308d3 13198a2e 03707344;  a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
//
// Mapping (restated on the host by tests/ancestral_restated.py; INTEGRATION.md, Samplers):
//   key     = (seed & 0xffffffff, seed >> 32)           seed: 64 bits
//   counter = (q, ch, frame, step)                      q = px >> 2 (pixel quad; hw % 4 == 0), frame = absolute frame
//                                                       index of the clip, step = index in the scheduler's full schedule
//   (r0, r1, r2, r3) -> four normals by Box-Muller: (r0, r1) -> pixels 4q, 4q+1; (r2, r3) -> 4q+2, 4q+3, with
//   u1 = ((r0 >> 8) + 1) 2^-24 in (0, 1], u2 = (r1 >> 8) 2^-24, rho = sqrt(-2 ln u1), z = rho (cos 2 pi u2, sin 2 pi u2).
// fp32 with the precise library functions (logf, sqrtf, sincospif): the noise of a pixel depends on nothing but
// (seed, step, frame, channel, pixel), so it is the same for any window layout, call merging, rank or frame shard.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct vx_u32x4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ vx_u32x4 vx_philox4x32_10(vx_u32x4 ctr, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t hi0 = __umulhi(0xD2511F53u, ctr.x), lo0 = 0xD2511F53u * ctr.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, ctr.z), lo1 = 0xCD9E8D57u * ctr.z;
    ctr = vx_u32x4{hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0};
  }
  return ctr;
}

// Box-Muller of one pair of 32-bit words: two standard normals
__device__ __forceinline__ void vx_box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f;     // 2^-24: (0, 1], exact in fp32
  const float u2 = (float)(b >> 8) * 5.9604644775390625e-8f;            // [0, 1)
  const float rho = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  z0 = rho * c;
  z1 = rho * s;
}

// the four normals of pixel quad q of (channel, frame) at schedule step `step`: pixels 4q .. 4q+3
__device__ __forceinline__ float4 vx_normal4(uint32_t q, uint32_t ch, uint32_t frame, uint32_t step, uint32_t seed_lo,
                                             uint32_t seed_hi) {
  const vx_u32x4 r = vx_philox4x32_10(vx_u32x4{q, ch, frame, step}, seed_lo, seed_hi);
  float4 z;
  vx_box_muller(r.x, r.y, z.x, z.y);
  vx_box_muller(r.z, r.w, z.z, z.w);
  return z;
}
