// Device helpers that more than one family of speech-embedding kernels uses: the MFMA operand
// and accumulator vectors, the split of an f32 value into its hi / lo fp16 pair, the three
// products of one split-f16 step (mma3), the LeakyReLU that keeps NaN, the hi / lo store of a
// 16-channel tile and the range guard of the f16 planes. The kernels are in hbk_embed_exact.hip,
// hbk_embed_x3.hip, hbk_embed_band.hip and hbk_embed_stream.hip (hbk_embed_internal.h says what
// each holds); what only one family uses stays in its unit.
#pragma once

#include "hbk_common.h"
#include "hbk_embed_args.h"

namespace hbk {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __fp16 h2 __attribute__((ext_vector_type(2)));
typedef float f16x __attribute__((ext_vector_type(16)));

// ---- range guard (kF16Max and the range flag: hbk_embed_args.h) ----
// (one v_max3 through asm: fmaxf / fabsf put canonicalising v_max ops in front)
__device__ __forceinline__ void track(float& amax, float a, float b) {
  asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(a), "v"(b));
}
__device__ __forceinline__ void raise_range(int* flag, float amax) {
  if (amax >= kF16Max) *flag = 1;  // vector store: any writer, same value
}
// (the generic kernel runs at its VGPR cap: it checks each group of values
// where it splits them instead of carrying amax, guard4)
__device__ __forceinline__ void guard4(int* flag, float a, float b, float c, float d) {
  float m = 0.f;
  track(m, a, b);
  track(m, c, d);
  if (m >= kF16Max) *flag = 1;
}

// ---- the hi / lo split ----
// hi = v rounded toward zero to fp16 (11 significant bits in fp16's normal
// range), lo = (v - hi) rounded to fp16 by v_fma_mix{lo,hi}_f16 (v - hi is
// exact in f32); two values, packed: 3 VALU instructions per pair
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b));
  uint32_t l;  // mixlo writes bits 15:0, mixhi bits 31:16: no initial value needed
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(a), "v"(hi));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(b), "v"(hi));
  lo = l;
}
// ... with the pair added to the caller's amax (track)
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo, float& amax) {
  track(amax, a, b);
  split2(a, b, hi, lo);
}
// ... as fp16 pairs
__device__ __forceinline__ void split2(float a, float b, h2& hi, h2& lo) {
  uint32_t h, l;
  split2(a, b, h, l);
  hi = __builtin_bit_cast(h2, h);
  lo = __builtin_bit_cast(h2, l);
}
__device__ __forceinline__ uint32_t h2_bits(h2 v) { return __builtin_bit_cast(uint32_t, v); }

// ---- one split-f16 step: acc += W_hi X_hi + W_hi X_lo + W_lo X_hi, in this order ----
// (weights are the A operand, activations the B operand; the dropped W_lo X_lo is 2^-22 relative)
__device__ __forceinline__ f16x mma3(h8 wh, h8 wl, h8 xh, h8 xl, f16x acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh, acc, 0, 0, 0);
}
__device__ __forceinline__ f4 mma3(h8 wh, h8 wl, h8 xh, h8 xl, f4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc, 0, 0, 0);
}

// ---- LeakyReLU with 0 <= alpha <= 1 as max(v, alpha v); LEAKY false: identity ----
// (v_max_f32 through asm: fmaxf on MFMA results gets a canonicalising v_max in
// front of it; both operands are NaN for a NaN v, so NaN propagates)
template <bool LEAKY>
__device__ __forceinline__ float leaky_max(float v, float alpha) {
  if (!LEAKY) return v;
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(v * alpha));
  return r;
}
// ... of two values in place: one packed multiply, two maxes (its own spelling: as two
// leaky_max calls the streaming kernels compile to two multiplies and other code)
typedef float f2v __attribute__((ext_vector_type(2)));
template <bool LEAKY>
__device__ __forceinline__ void leaky_max2(float& a, float& b, float alpha) {
  if (!LEAKY) return;
  const f2v m = f2v{a, b} * alpha;
  asm("v_max_f32 %0, %0, %1" : "+v"(a) : "v"(m.x));
  asm("v_max_f32 %0, %0, %1" : "+v"(b) : "v"(m.y));
}

// ---- activation, split and store of one 16-channel tile of a 16x16x32 accumulator ----
// channels 16 mb + 4 kq + j of position p go to the hi plane at oh (CS fp16 per position) and
// to the lo plane PL fp16 behind it; the split values are added to amax
template <bool LEAKY, int CS, int PL>
__device__ __forceinline__ void store_tile(f4 acc, _Float16* oh, int p, int mb, int kq, float alpha, float& amax) {
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
  leaky_max2<LEAKY>(v[0], v[1], alpha);
  leaky_max2<LEAKY>(v[2], v[3], alpha);
  uint32_t h01, l01, h23, l23;
  split2(v[0], v[1], h01, l01, amax);
  split2(v[2], v[3], h23, l23, amax);
  const int o = p * CS + 16 * mb + 4 * kq;
  *reinterpret_cast<uint2*>(oh + o) = uint2{h01, h23};
  *reinterpret_cast<uint2*>(oh + PL + o) = uint2{l01, l23};
}
// ... of the NB tiles of one position; a position outside the stage's valid
// range (track_it false) is stored but kept out of amax
template <bool LEAKY, int NB, int CS, int PL>
__device__ __forceinline__ void store_tiles(const f4 (&acc)[NB], _Float16* oh, int p, int kq, float alpha,
                                            bool track_it, float& amax) {
  float m = 0.f;
#pragma unroll
  for (int mb = 0; mb < NB; ++mb) store_tile<LEAKY, CS, PL>(acc[mb], oh, p, mb, kq, alpha, m);
  asm("v_max_f32 %0, %0, %1" : "+v"(amax) : "v"(track_it ? m : 0.f));
}

}  // namespace
}  // namespace hbk
