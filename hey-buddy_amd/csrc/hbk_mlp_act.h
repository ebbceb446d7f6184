// Activations of the classifier's MLP blocks (reference util/modeling_util.py:74-115,
// get_activation: relu, gelu, silu / swish, mish, tanh, sigmoid, identity / None), with
// torch's semantics, for hbk_mlp_act.hip: the enum shared by host and device (its values are
// hbk.h's HBK_ACT_*), and f(x) / f'(x) in f32.
//
// Every function and derivative is finite for every finite input (checked on [-100, 100]) and
// lands on the correct limit where expf leaves the f32 range: every exponential here has a
// non-positive argument, except mish's, which is only taken for x <= 20. No form subtracts two
// nearly equal values where the result is then scaled up (1 - sigma, 1 - tanh^2 and 1 + erf are
// written as the products / quotients they equal), so the error stays a few ulp of the RESULT
// over the whole range, not of 1.
#pragma once

#include <stdint.h>

#include "hbk.h"

namespace hbk {

enum class Act : int32_t {
  Silu = HBK_ACT_SILU,
  Relu = HBK_ACT_RELU,
  Gelu = HBK_ACT_GELU,
  Mish = HBK_ACT_MISH,
  Tanh = HBK_ACT_TANH,
  Sigmoid = HBK_ACT_SIGMOID,
  Identity = HBK_ACT_IDENTITY,
};
constexpr int kActCount = HBK_ACT_IDENTITY + 1;

inline bool act_valid(int32_t code) { return code >= 0 && code < kActCount; }

#if defined(__HIPCC__)

// sigma(x) and sigma(-x) = 1 - sigma(x) from q = e^{-|x|} in (0, 1]
struct SigPair {
  float s, c;
};
__device__ __forceinline__ SigPair sig_pair(float x) {
  const float q = expf(-fabsf(x));
  const float big = 1.f / (1.f + q), small = q * big;
  return x >= 0.f ? SigPair{big, small} : SigPair{small, big};
}

// Phi(x), the standard normal distribution function (nn.GELU(): the exact, erf form):
// 0.5 erfc(-x / sqrt 2) keeps the left tail, where 1 + erf(x / sqrt 2) cancels
__device__ __forceinline__ float norm_cdf(float x) { return 0.5f * erfcf(-x * 0.70710678118654752f); }

// mish, x <= 20: with w = e^x, tanh(log1p(w)) = n / (n + 2) for n = w (w + 2), and
// 1 - tanh = 2 / (n + 2) (w <= 4.9e8, n <= 2.4e17: finite). Above 20 softplus(x) = x
// (F.softplus's threshold) and tanh(x) is 1 in f32.
struct MishT {
  float t, one_minus_t, sig;
};
__device__ __forceinline__ MishT mish_t(float x) {
  const float w = expf(fminf(x, 20.f));
  const float n = w * (w + 2.f);
  const float inv = 1.f / (n + 2.f);
  return MishT{n * inv, 2.f * inv, w / (1.f + w)};
}

template <Act A>
__device__ __forceinline__ float act_f(float x) {
  if constexpr (A == Act::Relu) {
    return x > 0.f ? x : 0.f;
  } else if constexpr (A == Act::Gelu) {
    return x * norm_cdf(x);
  } else if constexpr (A == Act::Silu) {
    return x * sig_pair(x).s;
  } else if constexpr (A == Act::Mish) {
    return x > 20.f ? x : x * mish_t(x).t;
  } else if constexpr (A == Act::Tanh) {
    return tanhf(x);
  } else if constexpr (A == Act::Sigmoid) {
    return sig_pair(x).s;
  } else {
    return x;
  }
}

template <Act A>
__device__ __forceinline__ float act_df(float x) {
  if constexpr (A == Act::Relu) {
    return x > 0.f ? 1.f : 0.f;
  } else if constexpr (A == Act::Gelu) {
    // Phi(x) + x phi(x); e^{-x^2 / 2} underflows to 0 from |x| = 15 on
    return norm_cdf(x) + x * (0.3989422804014327f * expf(-0.5f * x * x));
  } else if constexpr (A == Act::Silu) {
    const SigPair p = sig_pair(x);
    return p.s * (1.f + x * p.c);
  } else if constexpr (A == Act::Mish) {
    if (x > 20.f) return 1.f;
    const MishT m = mish_t(x);
    return m.t + x * m.sig * ((1.f + m.t) * m.one_minus_t);  // t + x sigma (1 - t^2)
  } else if constexpr (A == Act::Tanh) {
    // 1 - tanh^2 = 4 q / (1 + q)^2 with q = e^{-2 |x|}
    const float q = expf(-2.f * fabsf(x));
    const float r = 1.f / (1.f + q);
    return 4.f * q * r * r;
  } else if constexpr (A == Act::Sigmoid) {
    const SigPair p = sig_pair(x);
    return p.s * p.c;
  } else {
    return 1.f;
  }
}

#endif  // __HIPCC__

}  // namespace hbk
