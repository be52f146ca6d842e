// The terms the loss kernels share.  Floating-point expressions here are whole statements on purpose: -ffp-contract=on fuses
// inside one source expression only, so splitting or joining them changes bits.
#pragma once
#include <hip/hip_runtime.h>

namespace eat {

// ONE expression for a probability across the library
__device__ __forceinline__ float sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// Row b of a mixed batch: target = lam * row b + (1 - lam) * row pb.  Without perm the row is itself (pb = b, lam = 1).
struct MixRow {
  int pb;
  double lam;
  bool mixed;     // perm was given
  bool bad;       // perm[b] lies outside [0, B)
};

// A bad permutation poisons its row (lam = NaN) and points it at itself: nothing outside the batch is read.
__device__ __forceinline__ MixRow mix_row(const int* __restrict__ perm, const float* __restrict__ lam, int b, int B) {
  MixRow m{b, 1.0, false, false};
  if (perm != nullptr) {
    m.pb = perm[b];
    m.lam = (double)lam[b];
    m.mixed = true;
    if (m.pb < 0 || m.pb >= B) m.pb = b, m.lam = __builtin_nan(""), m.bad = true;
  }
  return m;
}

// BCE-with-logits of a logit v in fp64, stable at both ends: p = s(v), q = s(-v), e = exp(-|v|).  A NaN logit gives NaN.
struct BceTerm {
  double p, q, e;
  // max(v, 0) - v t + softplus(-|v|): the loss of logit v against target t
  __device__ __forceinline__ double loss(double v, double t) const { return (v > 0.0 ? v : 0.0) - v * t + log1p(e); }
};
__device__ __forceinline__ BceTerm bce_term(double v) {
  const double e = exp(-fabs(v));
  const double a = 1.0 / (1.0 + e), b = e / (1.0 + e);
  return BceTerm{v >= 0.0 ? a : b, v >= 0.0 ? b : a, e};
}

}  // namespace eat
