// Device helpers shared by the fused classifier's translation units: the train
// step (hbk_mlp_fused.hip) and the evaluation passes (hbk_mlp_eval.hip). Vector
// types, the split-f16 MFMA products, wave reductions, barriers, the fragment
// loaders of the LDS-resident network stages, the dropout hash and the weight
// cache's description. Everything here is __device__ __forceinline__, constexpr
// or a plain struct, in the unnamed namespace the kernels themselves live in.
// (The step's trace and bounds machinery -- HBK_MT*, BCK and their __device__
// globals -- stays in hbk_mlp_fused.hip: the library is built without relocatable
// device code, so a __device__ global belongs to one translation unit.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hbk_mlp_dims.h"

namespace hbk {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mma(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// wave sum through DPP: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror leave each 16-lane row's sum in all of its lanes (rsum16); the
// four rows are then added from readlane (a bpermute-based __shfl_xor chain
// costs an LDS round trip per step)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float rsum16(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return v;
}
__device__ __forceinline__ float wsum(float v) {
  v = rsum16(v);
  const int b = __builtin_bit_cast(int, v);
  return (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)) +
          __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16))) +
         (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)) +
          __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48)));
}
__device__ __forceinline__ float wmax(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  const int b = __builtin_bit_cast(int, v);
  return fmaxf(fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)),
                     __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16))),
               fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)),
                     __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48))));
}
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
// The gates (train step and evaluation) and the evaluation's output: the hardware
// exp2 and reciprocal (1 ulp each) instead of expf's range reduction and the IEEE
// division sequence (~20 VALU instructions per sigmoid, on k2's dependent
// stages); values move by ~1e-7 relative (the tests' tolerances are >= 1e-5, and
// their counts allow predictions that near the threshold). The train step's loss
// stage keeps sigm (its high-loss filter compares p with thresholds).
__device__ __forceinline__ float sigm_fast(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}

// Barrier of a loop with global->LDS DMA in flight (its waits counted by hand
// before it): a fenced barrier would wait vmcnt(0), as the DMA writes LDS. The
// empty asm statements keep the compiler from moving memory accesses across.
__device__ __forceinline__ void dma_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// Workgroup barrier for LDS traffic only (the evaluation network's stages):
// the release / acquire fences are restricted to the local address space, so
// the barrier waits for the wave's LDS operations (lgkmcnt) but not for the
// next stage's weight loads in flight (a plain __syncthreads() waits vmcnt(0)
// too). Its waves hand nothing to each other through global memory. (In the
// train step's k2 the same change measured no difference: 36.89 vs 36.89 us.)
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// 32-bit counter hash for the input dropout mask (murmur3's finaliser over
// the element-pair index mixed with the step's 64-bit seed): one hash gives
// the 16-bit uniforms of elements 2 i and 2 i + 1 (p resolved to 2^-16).
__device__ __forceinline__ uint32_t drop_hash(uint32_t s0, uint32_t s1, uint32_t i) {
  uint32_t h = i * 0x9E3779B1u + s0;
  h ^= s1;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// Split-f16 products on v_mfma_f32_16x16x32_f16: v = hi + lo with hi = f16(v)
// and lo = f16(v - hi) (v - hi is exact in f32), so
// a . b ~ hi_a hi_b + hi_a lo_b + lo_a hi_b: three f16 MFMAs (16 cycles each
// per 16x16x32) for the 8 f32 MFMAs (32 cycles each) of the same 32-deep
// product. hi is rounded to nearest (v_cvt_pk_f16_f32), so |lo| <= 2^-11 |x|
// with either sign and the dropped lo_a lo_b is an unbiased ~2^-22 relative
// term (a round-toward-zero hi makes it up to 2^-20 and one-signed, a bias that
// survives long sums). lo = x - hi is exact in f32 before its rounding to f16.
// Plain vector code (cvt_pk, two cvt back, pk_fma, cvt_pk per pair): the
// compiler sees every operand and places the wait states itself. Callers keep
// |x| < 2^15.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
  const h2v h = __builtin_convertvector(f2v{a, b}, h2v);
  const f2v r = f2v{a, b} - __builtin_convertvector(h, f2v);
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, h2v));
}
// 8 floats (two f4) -> hi / lo h8
__device__ __forceinline__ void split8(const f4& x0, const f4& x1, h8& hi, h8& lo) {
  uint32_t h[4], l[4];
  split_pair(x0[0], x0[1], h[0], l[0]);
  split_pair(x0[2], x0[3], h[1], l[1]);
  split_pair(x1[0], x1[1], h[2], l[2]);
  split_pair(x1[2], x1[3], h[3], l[3]);
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  hi = __builtin_bit_cast(h8, u4{h[0], h[1], h[2], h[3]});
  lo = __builtin_bit_cast(h8, u4{l[0], l[1], l[2], l[3]});
}
__device__ __forceinline__ f4 mma3(const h8& ah, const h8& al, const h8& bh, const h8& bl, f4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);
}

// Weight fragments come pre-split from the step's weight cache (WSplit below:
// f16 hi / lo planes of 16 W, written by k4 with every update): T tiles of a
// [N][K] matrix (k contiguous), lane (n, kq) of block i holding k = 32 i + 8 kq
// .. + 7 of row n. Loads are unconditional: a tile past N reads a clamped
// (valid) row and its product is discarded by the caller.
template <int K, int T>
struct WFrag {
  h8 h[T][K / 32], l[T][K / 32];
};
template <int K, int N, int T>
__device__ __forceinline__ void load_wf(WFrag<K, T>& w, const _Float16* __restrict__ hi, int wave, int lane) {
  const int m = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int tt = 0; tt < T; ++tt) {
    const int n = min(16 * (wave + 4 * tt) + m, N - 1);
#pragma unroll
    for (int i = 0; i < K / 32; ++i) {
      w.h[tt][i] = *reinterpret_cast<const h8*>(hi + n * K + 32 * i + 8 * kq);
      w.l[tt][i] = *reinterpret_cast<const h8*>(hi + N * K + n * K + 32 * i + 8 * kq);
    }
  }
}

// 2^p and 2^-p with max |a| 2^p in [2^14, 2^15) (p clamped to +-100: a zero tile
// gets 2^100; inf / NaN propagate through the products)
__device__ __forceinline__ void pow2_scale(float amax, float& s, float& inv) {
  const int e = (__builtin_bit_cast(int, amax) >> 23) & 255;
  const int p = max(-100, min(100, 141 - e));
  s = __builtin_bit_cast(float, (127 + p) << 23);
  inv = __builtin_bit_cast(float, (127 - p) << 23);
}

// split-f16 A fragments of a [16][kLd] f32 LDS tile; inv undoes the A scale and
// the 16 on W
template <int K>
struct AFrag {
  h8 h[K / 32], l[K / 32];
  float inv;
};
template <int K, int LD = kLd>
__device__ __forceinline__ AFrag<K> load_a(const float* A, int lane) {
  const int m = lane & 15, kq = lane >> 4;
  f4 v[K / 32][2];
  float mx = 0.f;
#pragma unroll
  for (int i = 0; i < K / 32; ++i) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      v[i][h] = *reinterpret_cast<const f4*>(A + m * LD + 32 * i + 8 * kq + 4 * h);
#pragma unroll
      for (int s = 0; s < 4; ++s) mx = fmaxf(mx, fabsf(v[i][h][s]));
    }
  }
  float sc, inv;
  pow2_scale(wmax(mx), sc, inv);
  AFrag<K> f;
  f.inv = inv * (1.f / 16.f);
#pragma unroll
  for (int i = 0; i < K / 32; ++i) split8(v[i][0] * sc, v[i][1] * sc, f.h[i], f.l[i]);
  return f;
}

// two tiles (w, w + 4), two interleaved accumulation chains
template <int K>
__device__ __forceinline__ void gemm2(const WFrag<K, 2>& w, const AFrag<K>& a, f4& c0, f4& c1) {
  c0 = f4{0.f, 0.f, 0.f, 0.f};
  c1 = c0;
#pragma unroll
  for (int i = 0; i < K / 32; ++i) {
    c0 = mma3(a.h[i], a.l[i], w.h[0][i], w.l[0][i], c0);
    c1 = mma3(a.h[i], a.l[i], w.h[1][i], w.l[1][i], c1);
  }
  c0 *= a.inv;
  c1 *= a.inv;
}
// one tile (w), two chains over the even / odd k blocks
template <int K>
__device__ __forceinline__ f4 gemm1(const WFrag<K, 1>& w, const AFrag<K>& a) {
  f4 c[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int i = 0; i < K / 32; ++i) c[i & 1] = mma3(a.h[i], a.l[i], w.h[0][i], w.l[0][i], c[i & 1]);
  return (c[0] + c[1]) * a.inv;
}

// The step's weight cache: the matrices k2 multiplies by (W_o_k, k < NG - 1:
// [96][64]; W_hg_k, k >= 1: [128][96]) as f16 hi / lo planes of 16 W, each
// twice: as stored ([N][K], the forward's NT operand) and transposed (the
// backward's NN operand dx = dy W, again with k contiguous). Segment s at
// halves dst: hi [R][C], lo [R][C], hi^T [C][R], lo^T [C][R]. Written from the
// parameters by k0_wsplit (a step whose predecessor did not run k4 on this
// workspace) and by k4 with every update, so k2 reads its fragments with no
// conversion (the split of the f32 weights used to cost each of the ~70
// workgroups ~700 VALU cycles per matrix stage).
constexpr int kMaxSeg = 2 * kMaxG;
struct WSeg {
  int64_t src;  // float offset of the matrix in the parameters
  int rows, cols;
  int64_t dst;  // halves from the cache base
  int64_t q0;   // first float4 of the segment in the k0 grid
};
struct WSplit {
  int n;
  WSeg s[kMaxSeg];
};

}  // namespace
}  // namespace hbk
