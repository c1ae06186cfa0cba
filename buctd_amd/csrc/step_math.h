// Per-element update expressions of the optimizer steps.  The plain kernels (loss_decode.hip: adam_kernel, sgd_kernel) and
// the grouped ones (optim_groups.hip) call these and nothing else on an element, and the build uses -ffp-contract=off, so the
// same operands give the same bits on either path.
#pragma once
#include "common.h"

// torch.optim.Adam (no amsgrad), g already scaled:
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= step_size * m / (sqrt(v)/sqrt(bc2) + eps)        (step_size = lr / bc1)
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float b1, float b2, float eps,
                                            float step_size, float bc2_sqrt) {
  m = b1 * m + (1.f - b1) * g;
  v = b2 * v + (1.f - b2) * g * g;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p -= step_size * (m / denom);
}

// torch.optim.SGD (dampening 0), g already scaled:
//   g += wd p ;  buf = g (first step) | mu buf + g ;  g = nesterov ? g + mu buf : buf ;  p -= lr g
// b: the element's momentum buffer, read when mu != 0 and not first, written when mu != 0 (the caller loads and stores it
// under the same conditions)
__device__ __forceinline__ void sgd_update(float& p, float g, float& b, float lr, float mu, float wd, int nesterov, int first) {
  float gg = g + wd * p;
  if (mu != 0.f) {
    b = first ? gg : mu * b + gg;
    gg = nesterov ? gg + mu * b : b;
  }
  p = p - lr * gg;
}
