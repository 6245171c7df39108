// What the noisy-layer kernels share (csrc/noisy.hip, csrc/noisy_actor.hip): the layer sizes, the index plan of
// the concatenated draw and the draw itself (learner/noisy.py is the host mirror and the definition).
#pragma once
#include "apex_common.h"

#define NZ_FC_IN 3136
#define NZ_FC_OUT 1024
#define NZ_HID 512
#define NZ_STREAMS 64

// offsets of the seven parts of the concatenated draw (learner/noisy.py xi_offsets)
struct XiOff {
  int fc_out, v_in, a_in, v_out, a_out, K;
};
__host__ __device__ inline XiOff xi_off(int A, int N) {
  XiOff o;
  o.fc_out = 2 * NZ_FC_IN;
  o.v_in = o.fc_out + NZ_FC_OUT;
  o.a_in = o.v_in + NZ_HID;
  o.v_out = o.a_in + NZ_HID;
  o.a_out = o.v_out + N;
  o.K = o.a_out + A * N;
  return o;
}

// xi = sign(g) sqrt(|g|), g = sqrt(-2 ln u1) cos(2 pi u2) from the counter RNG's uniforms.
// Accurate logf / sqrtf / cospif (no fast-math variants): the mirror evaluates g in fp64.
__device__ __forceinline__ float noisy_xi(uint64_t seed, uint64_t c, uint32_t k) {
  const float u1 = 1.0f - apex_uniform(seed, c, 2ull * k);        // (0, 1], exact
  const float u2 = apex_uniform(seed, c, 2ull * k + 1ull);
  const float g = sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
  return copysignf(sqrtf(fabsf(g)), g);
}
