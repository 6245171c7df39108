// Invertible value rescaling of the n-step target (Pohlen et al. 2018, "Observe and Look Further"; R2D2's
// eps = 1e-3): the network learns h(Q), the target is T = h(R + Gamma h^-1(y)) with y the target net's value
// (or one quantile sample / one support atom of it):
//
//   h(x)     = sign(x) (sqrt(|x| + 1) - 1) + eps x
//   h^-1(y)  = sign(y) (((sqrt(1 + 4 eps (|y| + 1 + eps)) - 1) / (2 eps))^2 - 1)
//   T(R,G,y) = h(R + G h^-1(y))                              (G = 0 at terminals: T = h(R), no special case)
//
// Evaluated in fp64 on the fp32 inputs and rounded to fp32 once, as noisy_compose_kernel forms its values
// (learner/rescale.py is the host mirror).  The textbook fp32 form of h^-1 is not used: at eps = 1e-3 its
// sqrt(1 + s) - 1 cancels about eight bits.  Both functions are evaluated in forms without a cancelling
// difference (sqrt(1 + a) - 1 = a / (sqrt(1 + a) + 1)), the mirror's own:
//
//   h(x)    = x / (sqrt(|x| + 1) + 1) + eps x
//   h^-1(y) = sign(y) t (t + 2),  t = 2 |y| / (sqrt(1 + 4 eps (|y| + 1 + eps)) + 1 + 2 eps)    (t = r - 1)
//
// Two fp64 square roots per target value: one per sample on the scalar head, at most 64 per sample on the
// distributional ones.
#pragma once
#include "apex_common.h"

__device__ __forceinline__ double value_rescale_h(double x, double eps) {
  return x / (sqrt(fabs(x) + 1.0) + 1.0) + eps * x;
}

__device__ __forceinline__ double value_rescale_h_inv(double y, double eps) {
  const double ay = fabs(y);
  const double t = 2.0 * ay / (sqrt(1.0 + 4.0 * eps * (ay + 1.0 + eps)) + 1.0 + 2.0 * eps);
  return copysign(t * (t + 2.0), y);
}

__device__ __forceinline__ float value_rescale_target(float R, float G, float y, float eps) {
  const double e = (double)eps;
  return (float)value_rescale_h((double)R + (double)G * value_rescale_h_inv((double)y, e), e);
}
