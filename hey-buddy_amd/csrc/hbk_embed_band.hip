// Speech-embedding conv stack: the banded pattern kernels p0_chain_kernel and p1_chain_kernel
// (fixed shapes of SE20's first two chains; one task = one image x a band of pooled rows, with
// the band's halo rows recomputed). hbk_embed.hip launches them through embed_band_kernel;
// P0Args / P0Geo / P1Args / P1Geo are in hbk_embed_args.h, plan_p0_band / plan_p1 in
// hbk_embed_plan.h, the split / activation / mma3 / range-flag helpers in hbk_embed_dev.h. The
// streaming forms of the same chains are in hbk_embed_stream.hip, the generic kernel of any
// chain in hbk_embed_x3.hip.
#include "hbk_embed_dev.h"
#include "hbk_embed_internal.h"
#include "hbk_embed_plan.h"  // Kern, and the shapes the plans pick (kP0W, kP0C, kP1W, kP1CI, kP1Band)

namespace hbk {
namespace {

// ------------------------------------------------------------------- p0 ----
// Pattern kernel for the chain  conv 3x3 (1 -> C) . conv 1x3 (C -> C) .
// conv 3x1 (C -> C) . max-pool 2x2  on a fixed input width WI (the SE20
// prefix's first group: 136 x 32 mel rows -> 66 x 14 x 24, ~55 % of the
// embedding MACs). Same split-f16 numerics as conv_chain_x3_kernel
// (hbk_embed_x3.hip: 3 fp16
// products per f32-accurate MAC on v_mfma_f32_32x32x16_f16, f32 accumulate),
// but every shape is a compile-time constant, so the position / tap address
// math folds to shifts and immediates (the generic kernel spends ~20 VALU
// instructions per MFMA on runtime index math and SGPR spills):
//   * stage 0 builds its B fragments straight from the f32 input rows in LDS
//     (taps 0-4 in the lane's first K half, 5-8 in the second): no im2col
//     buffer;
//   * every stage's A fragments (weights) and bias are loaded once per block
//     and stay in VGPRs (4-wave blocks, 2 waves / SIMD); the bias is the first
//     MFMA's accumulator input;
//   * the hi/lo split of each output is v_cvt_pkrtz (hi, round toward zero)
//     plus v_fma_mix{lo,hi}_f16 (lo = x - hi rounded to fp16);
//   * one task = one image x BAND pooled rows (4 waves, 32-position tiles
//     round-robin over the waves), 2 blocks / CU.
// (P0Args, P0Geo: hbk_embed_args.h)

// bias of this lane's accumulator rows (channels 8 q + 4 khalf + j, register 4 q + j)
__device__ __forceinline__ f16x p0_bias(const float* b, int khalf) {
  f16x v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 t = *reinterpret_cast<const float4*>(b + 8 * q + 4 * khalf);
    v[4 * q] = t.x;
    v[4 * q + 1] = t.y;
    v[4 * q + 2] = t.z;
    v[4 * q + 3] = t.w;
  }
  return v;
}

// activation + split of a finished tile into the hi / lo planes at position p
template <int C, int CS, bool LEAKY>
__device__ __forceinline__ void p0_store_planes(const f16x& acc, int p, int khalf, _Float16* oh, _Float16* ol,
                                                float alpha, float& amax) {
#pragma unroll
  for (int q = 0; q < C / 8; ++q) {
    float v[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) v[jj] = leaky_max<LEAKY>(acc[4 * q + jj], alpha);
    uint32_t h01, l01, h23, l23;
    split2(v[0], v[1], h01, l01, amax);
    split2(v[2], v[3], h23, l23, amax);
    const int o = p * CS + 8 * q + 4 * khalf;
    *reinterpret_cast<uint2*>(oh + o) = uint2{h01, h23};
    *reinterpret_cast<uint2*>(ol + o) = uint2{l01, l23};
  }
}

// Stage 1 (1x3, ST = 1: grid R0 x W0 -> R1 x W1, planes out) or stage 2
// (3x1, ST = 2: R1 x W1 -> R2 x W2, f32 out) of a task; K = tap * C + ci.
// A fragments (hi, lo) and bias of stage ST for this lane, loaded ahead of use
template <int KS>
struct P0W {
  h8 ah[KS], al[KS];
  f16x bias;
};
template <int WI, int C, int BAND, int ST>
__device__ __forceinline__ P0W<P0Geo<WI, C, BAND>::KS> p0_load_w(const P0Args& a, int r32, int khalf) {
  using G = P0Geo<WI, C, BAND>;
  P0W<G::KS> w;
  const _Float16* wp = a.w + (ST == 1 ? G::WOFF1 : G::WOFF2) + r32 * (16 * G::KS) + 8 * khalf;
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) {
    w.ah[ks] = *reinterpret_cast<const h8*>(wp + 16 * ks);
    w.al[ks] = *reinterpret_cast<const h8*>(wp + 32 * 16 * G::KS + 16 * ks);
  }
  w.bias = p0_bias(a.bias + 32 * ST, khalf);
  return w;
}

template <int WI, int C, int BAND, int ST, bool LEAKY>
__device__ __forceinline__ void p0_stage12(const P0Args& a, const P0W<P0Geo<WI, C, BAND>::KS>& W,
                                           const _Float16* xh_, const _Float16* xl_, _Float16* oh, _Float16* ol,
                                           float* of, int wave, int r32, int khalf, float& amax) {
  using G = P0Geo<WI, C, BAND>;
  constexpr int M = ST == 1 ? G::M1 : G::M2, T = ST == 1 ? G::T1 : G::T2;
  constexpr int Wout = ST == 1 ? G::W1 : G::W2, Win = ST == 1 ? G::W0 : G::W1;
  constexpr int TAPSTRIDE = ST == 1 ? G::CS : G::W1 * G::CS;  // fp16 between taps in the input grid
  const float alpha = a.alpha;
  // Software pipeline over this wave's tiles: the epilogue (activation, split,
  // LDS stores) of tile t - 1 is issued in the same block as tile t's MFMA
  // chain, so its VALU work fills the MFMA issue gaps.
  auto load = [&](int t, int ks, h8& xh, h8& xl) {
    const int p = min(t * 32 + r32, M - 1);
    const int y = p / Wout, x = p - y * Wout;
    // this lane's 8-channel group: K = 16 ks + 8 khalf (groups past 3 C read group 0; weights 0)
    const int ka = 16 * ks < 3 * C ? 16 * ks : 0;
    const int kb = 16 * ks + 8 < 3 * C ? 16 * ks + 8 : 0;
    const int oa = (ka / C) * TAPSTRIDE + ka % C, ob = (kb / C) * TAPSTRIDE + kb % C;
    const int o = (y * Win + x) * G::CS + (khalf ? ob : oa);
    xh = *reinterpret_cast<const h8*>(xh_ + o);
    xl = *reinterpret_cast<const h8*>(xl_ + o);
  };
  auto epilogue = [&](int t, const f16x& acc) {
    const int pp = t * 32 + r32;
    if (pp >= M) return;
    if (ST == 1) {
      p0_store_planes<C, G::CS, LEAKY>(acc, pp, khalf, oh, ol, alpha, amax);
    } else {
#pragma unroll
      for (int q = 0; q < C / 8; ++q) {
        float4 v;
        v.x = leaky_max<LEAKY>(acc[4 * q], alpha);
        v.y = leaky_max<LEAKY>(acc[4 * q + 1], alpha);
        v.z = leaky_max<LEAKY>(acc[4 * q + 2], alpha);
        v.w = leaky_max<LEAKY>(acc[4 * q + 3], alpha);
        *reinterpret_cast<float4*>(of + pp * C + 8 * q + 4 * khalf) = v;
      }
    }
  };
  f16x prev;
  int tprev = -1;
  for (int t = wave; t < T; t += kP0Waves) {
    h8 xh[G::KS], xl[G::KS];
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) load(t, ks, xh[ks], xl[ks]);
    f16x acc = W.bias;
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) acc = mma3(W.ah[ks], W.al[ks], xh[ks], xl[ks], acc);
    if (tprev >= 0) epilogue(tprev, prev);
    prev = acc;
    tprev = t;
  }
  if (tprev >= 0) epilogue(tprev, prev);
}

template <int WI, int C, int BAND, bool LEAKY>
__global__ void __launch_bounds__(kP0Threads) __attribute__((amdgpu_waves_per_eu(2)))
p0_chain_kernel(P0Args a) {
  using G = P0Geo<WI, C, BAND>;
  extern __shared__ __attribute__((aligned(16))) unsigned char p0mem[];
  float* raw = reinterpret_cast<float*>(p0mem);
  _Float16* s1h = reinterpret_cast<_Float16*>(p0mem);
  _Float16* s1l = s1h + G::M1 * G::CS;
  _Float16* s0h = reinterpret_cast<_Float16*>(p0mem + G::XB);
  _Float16* s0l = s0h + G::M0 * G::CS;
  float* s2 = reinterpret_cast<float*>(p0mem + G::XB);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, khalf = lane >> 5;
  const int n_tasks = static_cast<int>(a.n_img) * a.n_bands;

  // the task's input rows (RI x WI floats = RI * WI / 4 float4, one per thread
  // while it fits) are loaded one task ahead into registers
  constexpr int kRawV = G::RI * WI / 4;
  constexpr int kRawPer = (kRawV + kP0Threads - 1) / kP0Threads;
  float4 rawv[kRawPer];
  auto load_raw = [&](int task) {
    const int img = task / a.n_bands, band = task - img * a.n_bands;
    const float* src = a.in + static_cast<int64_t>(img) * a.src_img_stride;
#pragma unroll
    for (int u = 0; u < kRawPer; ++u) {
      const int i = tid + u * kP0Threads;
      if (i < kRawV) {
        const int r = i / (WI / 4), c4 = i - r * (WI / 4);
        const int rr = min(band * G::R2 + r, a.H_in - 1);
        rawv[u] = *reinterpret_cast<const float4*>(src + static_cast<int64_t>(rr) * WI + 4 * c4);
      }
    }
  };
  if (static_cast<int>(blockIdx.x) < n_tasks) load_raw(blockIdx.x);
  // every stage's A fragments and bias stay in VGPRs for the whole kernel
  const _Float16* wp0 = a.w + r32 * 16 + 8 * khalf;
  const h8 a0h = *reinterpret_cast<const h8*>(wp0), a0l = *reinterpret_cast<const h8*>(wp0 + 32 * 16);
  const f16x b0 = p0_bias(a.bias, khalf);
  const auto W1 = p0_load_w<WI, C, BAND, 1>(a, r32, khalf);
  const auto W2 = p0_load_w<WI, C, BAND, 2>(a, r32, khalf);
  float amax = 0.f;

  for (int task = blockIdx.x; task < n_tasks; task += gridDim.x) {
    const int img = task / a.n_bands, band = task - img * a.n_bands;
    __syncthreads();  // the previous task's readers are done
    // 1) input rows [row0, row0 + RI) (clamped to the image) -> raw; prefetch the next task's
#pragma unroll
    for (int u = 0; u < kRawPer; ++u) {
      const int i = tid + u * kP0Threads;
      if (i < kRawV) *reinterpret_cast<float4*>(raw + 4 * i) = rawv[u];
    }
    if (task + static_cast<int>(gridDim.x) < n_tasks) load_raw(task + gridDim.x);
    __syncthreads();
    // 2) stage 0: 3x3, 1 -> C; B fragments straight from the f32 rows
    //    (taps 0-4 in the first K half, 5-8 and a zero in the second)
    {
      for (int t = wave; t < G::T0; t += kP0Waves) {
        const int pp = t * 32 + r32, p = min(pp, G::M0 - 1);
        const int y = p / G::W0, x = p - y * G::W0;
        const float* rp = raw + y * WI + x;
        float v[8];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const int t1 = 5 + i < 9 ? 5 + i : 0;
          v[i] = rp[khalf ? (t1 / 3) * WI + t1 % 3 : (i / 3) * WI + i % 3];
        }
        if (khalf) v[4] = 0.f;
        v[5] = v[6] = v[7] = 0.f;
        uint32_t hb[4], lb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split2(v[2 * i], v[2 * i + 1], hb[i], lb[i], amax);
        const h8 xh = __builtin_bit_cast(h8, uint4{hb[0], hb[1], hb[2], hb[3]});
        const h8 xl = __builtin_bit_cast(h8, uint4{lb[0], lb[1], lb[2], lb[3]});
        const f16x acc = mma3(a0h, a0l, xh, xl, b0);
        if (pp < G::M0) p0_store_planes<C, G::CS, LEAKY>(acc, p, khalf, s0h, s0l, a.alpha, amax);
      }
    }
    __syncthreads();
    p0_stage12<WI, C, BAND, 1, LEAKY>(a, W1, s0h, s0l, s1h, s1l, nullptr, wave, r32, khalf, amax);
    __syncthreads();
    p0_stage12<WI, C, BAND, 2, LEAKY>(a, W2, s1h, s1l, nullptr, nullptr, s2, wave, r32, khalf, amax);
    __syncthreads();
    // 3) 2x2 max-pool of the stage-2 rows -> the band's BAND output rows
    {
      constexpr int PW = G::W2 / 2, C4 = C / 4;
      float* dst = a.out + static_cast<int64_t>(img) * a.H_out * PW * C;
      for (int i = tid; i < BAND * PW * C4; i += kP0Threads) {
        const int c4 = i % C4, rest = i / C4, px = rest % PW, py = rest / PW;
        const int orow = band * BAND + py;
        if (orow >= a.H_out) continue;
        const float* q0 = s2 + ((2 * py) * G::W2 + 2 * px) * C + 4 * c4;
        const float4 v00 = *reinterpret_cast<const float4*>(q0);
        const float4 v01 = *reinterpret_cast<const float4*>(q0 + C);
        const float4 v10 = *reinterpret_cast<const float4*>(q0 + G::W2 * C);
        const float4 v11 = *reinterpret_cast<const float4*>(q0 + G::W2 * C + C);
        float4 m;
        m.x = nan_max(nan_max(v00.x, v01.x), nan_max(v10.x, v11.x));
        m.y = nan_max(nan_max(v00.y, v01.y), nan_max(v10.y, v11.y));
        m.z = nan_max(nan_max(v00.z, v01.z), nan_max(v10.z, v11.z));
        m.w = nan_max(nan_max(v00.w, v01.w), nan_max(v10.w, v11.w));
        *reinterpret_cast<float4*>(dst + (static_cast<int64_t>(orow) * PW + px) * C + 4 * c4) = m;
      }
    }
  }
  raise_range(a.range_flag, amax);
}

// ------------------------------------------------------------------- p1 ----
// Pattern kernel for the chain  conv 1x3 (CI -> 32) . conv 3x1 (32 -> 32) .
// conv 1x3 (32 -> 32) . conv 3x1 (32 -> 32) . max-pool 2x2  on an NHWC f32
// input of fixed width WI (SE20 chain 1: 66 x 14 x 24 -> 31 x 5 x 32). Same
// split-f16 numerics and tile / epilogue scheme as p0_chain_kernel; the
// stage weights do not all fit in VGPRs, so each stage's A fragments are
// loaded (from L2) one stage ahead, while the previous stage runs.
// (P1Args, P1Geo: hbk_embed_args.h)

template <int KS>
__device__ __forceinline__ P0W<KS> p1_load_w(const _Float16* w, const float* bias, int r32, int khalf) {
  P0W<KS> W;
  const _Float16* wp = w + r32 * (16 * KS) + 8 * khalf;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    W.ah[ks] = *reinterpret_cast<const h8*>(wp + 16 * ks);
    W.al[ks] = *reinterpret_cast<const h8*>(wp + 32 * 16 * KS + 16 * ks);
  }
  W.bias = p0_bias(bias, khalf);
  return W;
}

// One conv stage on LDS planes: kernel KH x KW over CIN channels (fp16 stride
// CSI per position, input grid width WIN), output grid (M positions, width
// WOUT), 32 output channels -> planes (CSO) or f32 (F32OUT, stride 32).
template <int KH, int KW, int CIN, int CSI, int WIN, int WOUT, int M, int KS, int CSO, bool F32OUT, bool LEAKY>
__device__ __forceinline__ void p1_stage(const P0W<KS>& W, const _Float16* xh_, const _Float16* xl_,
                                         _Float16* oh, _Float16* ol, float* of, float alpha, int wave, int r32,
                                         int khalf, float& amax) {
  constexpr int T = (M + 31) / 32;
  auto epilogue = [&](int t, const f16x& acc) {
    const int pp = t * 32 + r32;
    if (pp >= M) return;
    if (!F32OUT) {
      p0_store_planes<kP1C, CSO, LEAKY>(acc, pp, khalf, oh, ol, alpha, amax);
    } else {
#pragma unroll
      for (int q = 0; q < kP1C / 8; ++q) {
        float4 v;
        v.x = leaky_max<LEAKY>(acc[4 * q], alpha);
        v.y = leaky_max<LEAKY>(acc[4 * q + 1], alpha);
        v.z = leaky_max<LEAKY>(acc[4 * q + 2], alpha);
        v.w = leaky_max<LEAKY>(acc[4 * q + 3], alpha);
        *reinterpret_cast<float4*>(of + pp * kP1C + 8 * q + 4 * khalf) = v;
      }
    }
  };
  f16x prev;
  int tprev = -1;
  for (int t = wave; t < T; t += kP0Waves) {
    const int p = min(t * 32 + r32, M - 1);
    const int y = p / WOUT, x = p - y * WOUT;
    const int base = (y * WIN + x) * CSI;
    h8 xh[KS], xl[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      // K = tap * CIN + ci, tap = dy * KW + dx; groups past KH KW CIN read group 0 (weights 0)
      const int ka = 16 * ks < KH * KW * CIN ? 16 * ks : 0;
      const int kb = 16 * ks + 8 < KH * KW * CIN ? 16 * ks + 8 : 0;
      const int ta = ka / CIN, tb = kb / CIN;
      const int oa = ((ta / KW) * WIN + ta % KW) * CSI + ka % CIN;
      const int ob = ((tb / KW) * WIN + tb % KW) * CSI + kb % CIN;
      const int o = base + (khalf ? ob : oa);
      xh[ks] = *reinterpret_cast<const h8*>(xh_ + o);
      xl[ks] = *reinterpret_cast<const h8*>(xl_ + o);
    }
    f16x acc = W.bias;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = mma3(W.ah[ks], W.al[ks], xh[ks], xl[ks], acc);
    if (tprev >= 0) epilogue(tprev, prev);
    prev = acc;
    tprev = t;
  }
  if (tprev >= 0) epilogue(tprev, prev);
}

template <int WI, int CI, int BAND, bool LEAKY>
__global__ void __launch_bounds__(kP0Threads) __attribute__((amdgpu_waves_per_eu(2)))
p1_chain_kernel(P1Args a) {
  using G = P1Geo<WI, CI, BAND>;
  constexpr int C = kP1C;
  extern __shared__ __attribute__((aligned(16))) unsigned char p1mem[];
  _Float16* inh = reinterpret_cast<_Float16*>(p1mem);
  _Float16* inl = inh + G::R0 * G::W0 * G::CSI;
  _Float16* s2h = reinterpret_cast<_Float16*>(p1mem);
  _Float16* s2l = s2h + G::M2 * G::CS;
  float* s4 = reinterpret_cast<float*>(p1mem);
  _Float16* s1h = reinterpret_cast<_Float16*>(p1mem + G::XB);
  _Float16* s1l = s1h + G::M1 * G::CS;
  _Float16* s3h = reinterpret_cast<_Float16*>(p1mem + G::XB);
  _Float16* s3l = s3h + G::M3 * G::CS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, khalf = lane >> 5;
  const int n_tasks = static_cast<int>(a.n_img) * a.n_bands;
  const float alpha = a.alpha;

  P0W<G::KS1> W1 = p1_load_w<G::KS1>(a.w + G::WOFF1, a.bias, r32, khalf);
  float amax = 0.f;
  for (int task = blockIdx.x; task < n_tasks; task += gridDim.x) {
    const int img = task / a.n_bands, band = task - img * a.n_bands;
    const int row0 = band * G::R4;
    __syncthreads();  // the previous task's readers are done
    // 1) input rows [row0, row0 + R0) (clamped) -> hi / lo planes, 8 channels per unit
    {
      const float* src = a.in + static_cast<int64_t>(img) * a.src_img_stride;
      constexpr int U = G::R0 * WI * (CI / 8);
      for (int u = tid; u < U; u += kP0Threads) {
        const int c8 = u % (CI / 8), pos = u / (CI / 8);
        const int r = pos / WI, x = pos - r * WI;
        const int rr = min(row0 + r, a.H_in - 1);
        const float* q = src + (static_cast<int64_t>(rr) * WI + x) * CI + 8 * c8;
        const float4 v0 = *reinterpret_cast<const float4*>(q), v1 = *reinterpret_cast<const float4*>(q + 4);
        uint32_t h[4], l[4];
        split2(v0.x, v0.y, h[0], l[0], amax);
        split2(v0.z, v0.w, h[1], l[1], amax);
        split2(v1.x, v1.y, h[2], l[2], amax);
        split2(v1.z, v1.w, h[3], l[3], amax);
        const int o = pos * G::CSI + 8 * c8;
        *reinterpret_cast<uint4*>(inh + o) = uint4{h[0], h[1], h[2], h[3]};
        *reinterpret_cast<uint4*>(inl + o) = uint4{l[0], l[1], l[2], l[3]};
      }
    }
    __syncthreads();
    P0W<G::KS> W2 = p1_load_w<G::KS>(a.w + G::WOFF2, a.bias + 32, r32, khalf);
    p1_stage<1, 3, CI, G::CSI, G::W0, G::W1, G::M1, G::KS1, G::CS, false, LEAKY>(W1, inh, inl, s1h, s1l, nullptr,
                                                                                  alpha, wave, r32, khalf, amax);
    __syncthreads();
    P0W<G::KS> W3 = p1_load_w<G::KS>(a.w + G::WOFF3, a.bias + 64, r32, khalf);
    p1_stage<3, 1, C, G::CS, G::W1, G::W2, G::M2, G::KS, G::CS, false, LEAKY>(W2, s1h, s1l, s2h, s2l, nullptr,
                                                                               alpha, wave, r32, khalf, amax);
    __syncthreads();
    P0W<G::KS> W4 = p1_load_w<G::KS>(a.w + G::WOFF4, a.bias + 96, r32, khalf);
    p1_stage<1, 3, C, G::CS, G::W2, G::W3, G::M3, G::KS, G::CS, false, LEAKY>(W3, s2h, s2l, s3h, s3l, nullptr,
                                                                               alpha, wave, r32, khalf, amax);
    __syncthreads();
    W1 = p1_load_w<G::KS1>(a.w + G::WOFF1, a.bias, r32, khalf);  // the next task's stage 1
    p1_stage<3, 1, C, G::CS, G::W3, G::W4, G::M4, G::KS, G::CS, true, LEAKY>(W4, s3h, s3l, nullptr, nullptr, s4,
                                                                              alpha, wave, r32, khalf, amax);
    __syncthreads();
    // 2x2 max-pool of the stage-4 rows -> BAND output rows
    {
      constexpr int PW = G::W4 / 2, C4 = C / 4;
      float* dst = a.out + static_cast<int64_t>(img) * a.H_out * PW * C;
      for (int i = tid; i < BAND * PW * C4; i += kP0Threads) {
        const int c4 = i % C4, rest = i / C4, px = rest % PW, py = rest / PW;
        const int orow = band * BAND + py;
        if (orow >= a.H_out) continue;
        const float* q0 = s4 + ((2 * py) * G::W4 + 2 * px) * C + 4 * c4;
        const float4 v00 = *reinterpret_cast<const float4*>(q0);
        const float4 v01 = *reinterpret_cast<const float4*>(q0 + C);
        const float4 v10 = *reinterpret_cast<const float4*>(q0 + G::W4 * C);
        const float4 v11 = *reinterpret_cast<const float4*>(q0 + G::W4 * C + C);
        float4 m;
        m.x = nan_max(nan_max(v00.x, v01.x), nan_max(v10.x, v11.x));
        m.y = nan_max(nan_max(v00.y, v01.y), nan_max(v10.y, v11.y));
        m.z = nan_max(nan_max(v00.z, v01.z), nan_max(v10.z, v11.z));
        m.w = nan_max(nan_max(v00.w, v01.w), nan_max(v10.w, v11.w));
        *reinterpret_cast<float4*>(dst + (static_cast<int64_t>(orow) * PW + px) * C + 4 * c4) = m;
      }
    }
  }
  raise_range(a.range_flag, amax);
}

}  // namespace

// n = band (p0), f = LeakyReLU
const void* embed_band_kernel(int kind, int n, bool f) {
  switch (static_cast<Kern>(kind)) {
    case Kern::p0_band:
      switch (n) {
        case 5: return f ? addr(p0_chain_kernel<kP0W, kP0C, 5, true>) : addr(p0_chain_kernel<kP0W, kP0C, 5, false>);
        case 7: return f ? addr(p0_chain_kernel<kP0W, kP0C, 7, true>) : addr(p0_chain_kernel<kP0W, kP0C, 7, false>);
        default: return f ? addr(p0_chain_kernel<kP0W, kP0C, 6, true>) : addr(p0_chain_kernel<kP0W, kP0C, 6, false>);
      }
    case Kern::p1:
      return f ? addr(p1_chain_kernel<kP1W, kP1CI, kP1Band, true>) : addr(p1_chain_kernel<kP1W, kP1CI, kP1Band, false>);
    default: return nullptr;
  }
}

}  // namespace hbk
