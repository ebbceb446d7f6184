// Speech-embedding conv stack: the streaming pattern kernels of the SE20 graph's four chains,
// p0s_chain_kernel, p1s_chain_kernel, p2s_chain_kernel and t3s_chain_kernel (rows streamed top
// to bottom through LDS rings, no halo recomputation; the default route). hbk_embed.hip
// launches them through embed_stream_kernel; the kP0s* / kP1s* / kP2s* / kT3* geometry and the
// argument structs are in hbk_embed_args.h, plan_p0s .. plan_t3s in hbk_embed_plan.h, the
// split / activation / mma3 / tile-store / range-flag helpers in hbk_embed_dev.h. The banded
// forms of chains 0 and 1 are in hbk_embed_band.hip, the generic kernel of any chain in
// hbk_embed_x3.hip.
#include "hbk_embed_dev.h"
#include "hbk_embed_internal.h"
#include "hbk_embed_plan.h"  // Kern

namespace hbk {
namespace {

// ------------------------------------------------------------------ p0s ----
// Streaming form of the p0 chain (SE20 chain 0 on a 32-wide mel image:
// 3x3 1 -> 24, 1x3 24 -> 24, 3x1 24 -> 24, max-pool 2x2): ONE WAVE PER CLIP,
// the clip's rows streamed top to bottom, no halo recomputation and no
// workgroup barrier. A tile is one row (32 positions; 30 / 28 / 28 valid).
// Iteration y runs three independent MFMA chains:
//   stage 0 of row y      B from the raw rows in registers      -> s0[y & 1]
//   stage 1 of row y - 1  B from s0[(y - 1) & 1] (LDS)          -> s1[(y - 1) & 3]
//   stage 2 of row y - 4  B from s1 rows y - 4 .. y - 2 (LDS)   -> registers
// Every LDS row an iteration reads was written by an earlier iteration of the
// same wave, and a wave's LDS instructions execute in order, so a compiler
// barrier between iterations is the only synchronisation. Stage-2 rows 2i and
// 2i + 1 are max-pooled in registers, the column pairs by a DPP lane swap,
// and the pooled row is stored as f32 [66][14][24] (the p1 chain's input).
// Raw rows: one dword per lane per row, loaded 8-11 rows ahead; the three
// column taps come from two DPP wave shifts. Biases ride in a padding slot
// of K whose B value is 1 (hi 1, lo 0), so every accumulator starts at 0.
// (the kP0s* geometry: hbk_embed_args.h)
struct P0sW {
  h8 h[kP0sKS], l[kP0sKS];
};

__device__ __forceinline__ float wave_shl1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

// activation, split and LDS store of one finished stage-0 / stage-1 tile
template <bool LEAKY>
__device__ __forceinline__ void p0s_store(const f16x& acc, _Float16* oh, int x, int khalf, float alpha, bool track_it,
                                          float& amax, int plane) {
  float m = 0.f;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    float v[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    leaky_max2<LEAKY>(v[0], v[1], alpha);
    leaky_max2<LEAKY>(v[2], v[3], alpha);
    uint32_t h01, l01, h23, l23;
    split2(v[0], v[1], h01, l01, m);
    split2(v[2], v[3], h23, l23, m);
    const int o = x * kP0sCS + 8 * q + 4 * khalf;
    *reinterpret_cast<uint2*>(oh + o) = uint2{h01, h23};
    *reinterpret_cast<uint2*>(oh + plane + o) = uint2{l01, l23};
  }
  asm("v_max_f32 %0, %0, %1" : "+v"(amax) : "v"(track_it ? m : 0.f));
}

template <bool LEAKY>
struct P0sCtx {
  h8 a0h, a0l;
  P0sW w1, w2;
  float r[2][3];   // raw rows y + khalf, y + 1 + khalf at columns x, x + 1, x + 2
  float q[8];      // raw rows loaded ahead (column x; row + khalf)
  f16x pool;       // stage-2 row 2i (even) awaiting its partner
  float amax;
  float alpha;
};

template <int PAR, bool LEAKY>
__device__ __forceinline__ void p0s_iter(P0sCtx<LEAKY>& c, int y, int qi, _Float16* wl, float* orow_base, int x,
                                         int khalf) {
  // raw window: rows y + khalf, y + 1 + khalf (the second from the load queue)
  c.r[0][0] = c.r[1][0]; c.r[0][1] = c.r[1][1]; c.r[0][2] = c.r[1][2];
  c.r[1][0] = c.q[qi];
  c.r[1][1] = wave_shl1(c.r[1][0]);
  c.r[1][2] = wave_shl1(c.r[1][1]);

  _Float16* s0w = wl + (PAR & 1) * 2 * kP0sS0Plane;        // stage 0 writes row y
  _Float16* s0r = wl + ((PAR + 1) & 1) * 2 * kP0sS0Plane;  // stage 1 reads row y - 1
  _Float16* s1 = wl + 4 * kP0sS0Plane;

  // B fragments of stage 1 (row y - 1) and stage 2 (row y - 4), one K step
  // ahead of their MFMAs. Stage 1: K group g = 2 ks + khalf = tap * 3 + c sits
  // at s0 fp16 offset 24 (x + tap) + 8 c = 24 x + 8 g, one per-lane base plus
  // immediates; group 9 is the bias slot (B = 1). Stage 2: the groups (dy, c)
  // are paired within a row for ks < 3 (khalf = c), then (0, 2) | (1, 2) and
  // (2, 2) | bias (mirrored by plan_p0s's packing).
  const _Float16* base1 = s0r + x * kP0sCS + 8 * khalf;
  const _Float16* base2 = s1 + x * kP0sCS + 8 * khalf;
  auto load1 = [&](int ks, h8& bh, h8& bl) {
    const bool one = ks == 4 && khalf;
    const _Float16* p1 = one ? wl + kP0sOnes : base1 + 16 * ks;
    bh = *reinterpret_cast<const h8*>(p1);
    bl = *reinterpret_cast<const h8*>(p1 + (one ? 8 : kP0sS0Plane));
  };
  auto load2 = [&](int ks, h8& bh, h8& bl) {
    const _Float16* p2;
    if (ks < 3) {
      p2 = base2 + ((PAR + ks) & 3) * 2 * kP0sS1Plane;
    } else if (ks == 3) {
      p2 = s1 + x * kP0sCS + 16 + (khalf ? ((PAR + 1) & 3) : (PAR & 3)) * 2 * kP0sS1Plane;
    } else {
      p2 = khalf ? wl + kP0sOnes : s1 + x * kP0sCS + 16 + ((PAR + 2) & 3) * 2 * kP0sS1Plane;
    }
    const bool one = ks == 4 && khalf;
    bh = *reinterpret_cast<const h8*>(p2);
    bl = *reinterpret_cast<const h8*>(p2 + (one ? 8 : kP0sS1Plane));
  };
  h8 f[2][2];
  load1(0, f[0][0], f[0][1]);

  // stage 0 (row y): K slots {r0[0..2], r1[0..2], 1, 0} in both lane halves, the
  // window one row lower in the upper half (taps (0, *), (1, 0), (1, 1) and the
  // bias in the lower half's weights, (1, 2), (2, *) in the upper half's)
  uint32_t hb[3], lb[3];
  float m0 = 0.f;
  split2(c.r[0][0], c.r[0][1], hb[0], lb[0], m0);
  split2(c.r[0][2], c.r[1][0], hb[1], lb[1], m0);
  split2(c.r[1][1], c.r[1][2], hb[2], lb[2], m0);
  const h8 xh = __builtin_bit_cast(h8, uint4{hb[0], hb[1], hb[2], 0x3C00u});  // slot 6 = 1.0 (f16)
  const h8 xl = __builtin_bit_cast(h8, uint4{lb[0], lb[1], lb[2], 0u});
  const f16x zero = {};
  const f16x acc0 = mma3(c.a0h, c.a0l, xh, xl, zero);
  const bool raw_ok = y < kP0sRows - 2;

  // The three stages' MFMA chains run one after another (stage 1, then stage
  // 2), and each finished stage's epilogue is issued between the next stage's
  // MFMAs (sched_group_barrier: 1 MFMA, then up to 5 VALU), so a wave keeps its
  // own matrix pipe busy while it activates, splits and stores: stage 0's
  // epilogue beside stage 1's MFMAs, stage 1's beside stage 2's.
  f16x acc1 = zero;
#pragma unroll
  for (int ks = 0; ks < kP0sKS; ++ks) {
    h8* cur = f[ks & 1];
    if (ks + 1 < kP0sKS) load1(ks + 1, f[(ks + 1) & 1][0], f[(ks + 1) & 1][1]);
    else load2(0, f[(ks + 1) & 1][0], f[(ks + 1) & 1][1]);
    acc1 = mma3(c.w1.h[ks], c.w1.l[ks], cur[0], cur[1], acc1);
    if (ks == 1) {
      asm("v_max_f32 %0, %0, %1" : "+v"(c.amax) : "v"(raw_ok ? m0 : 0.f));
      p0s_store<LEAKY>(acc0, s0w, x, khalf, c.alpha, raw_ok && x < 30, c.amax, kP0sS0Plane);
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
  }
  // stage 2 accumulates into c.pool for an even row y - 4 (held for its odd partner)
  f16x acc2 = zero;
  f16x& a2 = (PAR & 1) == 0 ? c.pool : acc2;
  a2 = zero;
#pragma unroll
  for (int ks = 0; ks < kP0sKS; ++ks) {
    h8* cur = f[(ks + kP0sKS) & 1];
    if (ks + 1 < kP0sKS) load2(ks + 1, f[(ks + 1 + kP0sKS) & 1][0], f[(ks + 1 + kP0sKS) & 1][1]);
    a2 = mma3(c.w2.h[ks], c.w2.l[ks], cur[0], cur[1], a2);
    if (ks == 0)
      p0s_store<LEAKY>(acc1, s1 + ((PAR + 3) & 3) * 2 * kP0sS1Plane, x, khalf, c.alpha,
                       y >= 1 && y <= kP0sRows - 2 && x < 28, c.amax, kP0sS1Plane);
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
  }

  // stage 2 (row y - 4): rows 2i and 2i + 1 pooled (max commutes with the
  // monotone activation; v_maximum3 propagates NaN, as the reference's max-pool)
  if ((PAR & 1) == 1) {
    float pv[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const float t = __builtin_elementwise_maximum(c.pool[i], acc2[i]);
      // column pair (x, x ^ 1): DPP quad_perm [1, 0, 3, 2]
      const float u = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, t), 0xB1, 0xf, 0xf,
                                                                         false));
      pv[i] = __builtin_elementwise_maximum(t, u);
    }
#pragma unroll
    for (int i = 0; i < 12; i += 2) leaky_max2<LEAKY>(pv[i], pv[i + 1], c.alpha);
    if (y >= 5 && !(x & 1) && x < 28) {
      float* o = orow_base + static_cast<int64_t>((y - 4) >> 1) * (kP0sWout * kP0sC) + (x >> 1) * kP0sC + 4 * khalf;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        *reinterpret_cast<float4*>(o + 8 * q) = float4{pv[4 * q], pv[4 * q + 1], pv[4 * q + 2], pv[4 * q + 3]};
    }
  }
  asm volatile("" ::: "memory");  // this iteration's LDS writes before the next one's reads (in-order LDS)
}

template <bool LEAKY>
__global__ void __launch_bounds__(kP0sThreads) __attribute__((amdgpu_waves_per_eu(2)))
p0s_chain_kernel(P0Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char p0smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = lane & 31, khalf = lane >> 5;
  _Float16* wl = reinterpret_cast<_Float16*>(p0smem) + wave * kP0sWaveHalfs;
  // constant slots: hi {1, 0, ..} and lo {0, ..}; s0 positions 32, 33 (never written) = 0
  if (lane < 16) wl[kP0sOnes + lane] = static_cast<_Float16>(lane == 0 ? 1.f : 0.f);
  for (int i = lane; i < 2 * 2 * 2 * kP0sCS; i += 64) {  // [buffer][plane][pos 32, 33][24]
    const int b = i / (4 * kP0sCS), rest = i - b * 4 * kP0sCS, pl = rest / (2 * kP0sCS);
    wl[b * 2 * kP0sS0Plane + pl * kP0sS0Plane + 32 * kP0sCS + rest % (2 * kP0sCS)] = static_cast<_Float16>(0.f);
  }
  P0sCtx<LEAKY> c;
  c.alpha = a.alpha;
  c.amax = 0.f;
  {
    const _Float16* w0 = a.w + x * 16 + 8 * khalf;
    c.a0h = *reinterpret_cast<const h8*>(w0);
    c.a0l = *reinterpret_cast<const h8*>(w0 + 32 * 16);
    const _Float16* w1 = a.w + 2 * 32 * 16 + x * (16 * kP0sKS) + 8 * khalf;
    const _Float16* w2 = w1 + 2 * 32 * 16 * kP0sKS;
#pragma unroll
    for (int ks = 0; ks < kP0sKS; ++ks) {
      c.w1.h[ks] = *reinterpret_cast<const h8*>(w1 + 16 * ks);
      c.w1.l[ks] = *reinterpret_cast<const h8*>(w1 + 32 * 16 * kP0sKS + 16 * ks);
      c.w2.h[ks] = *reinterpret_cast<const h8*>(w2 + 16 * ks);
      c.w2.l[ks] = *reinterpret_cast<const h8*>(w2 + 32 * 16 * kP0sKS + 16 * ks);
    }
  }
  asm volatile("" ::: "memory");
  const int64_t stride_w = static_cast<int64_t>(gridDim.x) * kP0sWaves;
  for (int64_t img = static_cast<int64_t>(blockIdx.x) * kP0sWaves + wave; img < a.n_img; img += stride_w) {
    const float* src = a.in + img * a.src_img_stride + x;
    const int hmax = a.H_in - 1;
    auto raw = [&](int row) { return src[min(row, hmax) * 32]; };
    float* orow_base = a.out + img * (static_cast<int64_t>(kP0sHout) * kP0sWout * kP0sC);
    // window row khalf (the first iteration shifts it down and brings row 1 + khalf); queue rows 1 .. 4 (+ khalf)
    c.r[1][0] = raw(khalf);
    c.r[1][1] = wave_shl1(c.r[1][0]);
    c.r[1][2] = wave_shl1(c.r[1][1]);
#pragma unroll
    for (int i = 0; i < 4; ++i) c.q[i] = raw(1 + khalf + i);
    for (int y0 = 0; y0 < kP0sRows; y0 += 4) {
      // rows y0 + 5 .. y0 + 8 (+ khalf; the next four iterations') into the queue's second half
#pragma unroll
      for (int i = 0; i < 4; ++i) c.q[4 + i] = raw(y0 + 5 + khalf + i);
      p0s_iter<0, LEAKY>(c, y0, 0, wl, orow_base, x, khalf);
      p0s_iter<1, LEAKY>(c, y0 + 1, 1, wl, orow_base, x, khalf);
      p0s_iter<2, LEAKY>(c, y0 + 2, 2, wl, orow_base, x, khalf);
      p0s_iter<3, LEAKY>(c, y0 + 3, 3, wl, orow_base, x, khalf);
#pragma unroll
      for (int i = 0; i < 4; ++i) c.q[i] = c.q[i + 4];
    }
  }
  raise_range(a.range_flag, c.amax);
}

// ------------------------------------------------------------------ p1s ----
// Streaming form of the p1 chain (SE20 chain 1 on the 66 x 14 x 24 chain-0
// output: 1x3 24 -> 32, 3x1, 1x3, 3x1 32 -> 32, max-pool 2x2 -> 31 x 5 x 32),
// rows streamed top to bottom through a TWO-WAVE STAGE PIPELINE per clip:
// wave 0 runs stages a and b, wave 1 stages c and d, so each wave keeps only
// its two stages' weights in VGPRs (96) and a CU runs two waves per SIMD.
// v_mfma_f32_16x16x32_f16 with a tile of one row (16 positions; 12 / 12 /
// 10 / 10 valid: a 32-position tile would be under half full) and two
// 16-channel output blocks. Iteration y (one workgroup barrier after it):
//   wave 0: stage input row y + 1; a(y) -> A[y & 3]; b(y - 3) -> B[(y - 3) & 1]
//   wave 1: c(y - 4) from B[(y - 4) & 1] -> C[(y - 4) & 3]; d(y - 7), pooled
// Every row a wave reads was written before the previous barrier or earlier
// by itself (a wave's LDS instructions execute in order). Stage a's bias
// rides in its K padding (slot 72, B = 1); b, c and d start their
// accumulators at the bias. K groups of 8 (g = 4 ks + kq, kq = lane / 16):
//   a: g = tap * 3 + c   -> input position x + tap, channels 8 c   (24 x + 8 g)
//   b: g = dy * 4 + c    -> A row (r + dy), position x, channels 8 c
//   c: g = dx * 4 + c    -> B position x + dx, channels 8 c
//   d: g = dy * 4 + c    -> C row (r + dy), position x, channels 8 c
// (the kP1s* geometry: hbk_embed_args.h)
struct P1sW {
  h8 h[2][3], l[2][3];  // [output block][K step]
};

struct P1sCtx {
  P1sW w[2];           // this wave's two stages
  f4 bias[2][2];       // wave 0: [b][mb] in bias[1]; wave 1: c, d
  float4 q[4][2];      // wave 0: input rows y + 1 .. y + 4 (two float4 per lane)
  f4 pool[2];          // wave 1: stage-d row 2i awaiting its partner
  float amax, alpha;
};

// one stage of one row: 2 output blocks x 3 K steps x 3 products
// (spelled out: through mma3, p1s_chain_kernel<true> is allocated other registers)
__device__ __forceinline__ void p1s_mma(f4 (&acc)[2], const P1sW& w, const h8 (&bh)[3], const h8 (&bl)[3]) {
#pragma unroll
  for (int ks = 0; ks < 3; ++ks)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[mb][ks], bh[ks], acc[mb], 0, 0, 0);
      acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[mb][ks], bl[ks], acc[mb], 0, 0, 0);
      acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.l[mb][ks], bh[ks], acc[mb], 0, 0, 0);
    }
}

// activation, split and LDS store of a finished stage row (channels 16 mb + 4 kq + j at position x;
// the lo plane PL behind the hi plane)
template <bool LEAKY, int PL>
__device__ __forceinline__ void p1s_store(const f4 (&acc)[2], _Float16* oh, int x, int kq, float alpha, bool track_it,
                                          float& amax) {
  store_tiles<LEAKY, 2, kP1sCS, PL>(acc, oh, x, kq, alpha, track_it, amax);
}

// the input row in registers (two float4 per lane: entries lane, lane + 64 of 84) -> hi / lo planes
__device__ __forceinline__ void p1s_stage_row(const float4 (&v)[2], _Float16* in_w, int lane, float& amx) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = lane + 64 * u;
    if (u == 0 || lane < kP1sWi * 6 - 64) {
      uint32_t h01, l01, h23, l23;
      split2(v[u].x, v[u].y, h01, l01, amx);
      split2(v[u].z, v[u].w, h23, l23, amx);
      const int o = (i / 6) * kP1sCSI + (i % 6) * 4;
      *reinterpret_cast<uint2*>(in_w + o) = uint2{h01, h23};
      *reinterpret_cast<uint2*>(in_w + kP1sInPlane + o) = uint2{l01, l23};
    }
  }
}

// wave 0, iteration y: stage input row y + 1, a(y), b(y - 3)
template <int PAR, bool LEAKY>
__device__ __forceinline__ void p1s_iter0(P1sCtx& c, int y, _Float16* sm, const float* src, int hmax, int x, int kq,
                                          int lane, int a2h, int a2l) {
  const _Float16* in_r = sm + kP1sIn + (PAR & 1) * kP1sInSlot;
  _Float16* A = sm + kP1sA;
  h8 bh[2][3], bl[2][3];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const int oa = ks < 2 ? x * kP1sCSI + 32 * ks + 8 * kq : a2h;  // 24 x + 8 g; ks 2: the lane's slot
    const int la = ks < 2 ? kP1sInPlane : a2l;
    bh[0][ks] = *reinterpret_cast<const h8*>(in_r + oa);
    bl[0][ks] = *reinterpret_cast<const h8*>(in_r + oa + la);
    const _Float16* pb = A + ((PAR + 1 + ks) & 3) * 2 * kP1sPlane + x * kP1sCS + 8 * kq;  // row y - 3 + ks
    bh[1][ks] = *reinterpret_cast<const h8*>(pb);
    bl[1][ks] = *reinterpret_cast<const h8*>(pb + kP1sPlane);
  }
  {  // input row y + 1 (loaded four iterations ago) -> the other input slot; load row y + 5
    const int slot = (PAR + 1) & 3;
    float amx = 0.f;
    p1s_stage_row(c.q[slot], sm + kP1sIn + ((PAR + 1) & 1) * kP1sInSlot, lane, amx);
    asm("v_max_f32 %0, %0, %1" : "+v"(c.amax) : "v"(y + 1 < kP1sHin ? amx : 0.f));
    const float* r = src + static_cast<int64_t>(min(y + 5, hmax)) * (kP1sWi * kP1sCSI);
    c.q[slot][0] = *reinterpret_cast<const float4*>(r + 4 * lane);
    c.q[slot][1] = *reinterpret_cast<const float4*>(r + 4 * min(lane + 64, kP1sWi * 6 - 1));
  }
  const f4 zero = {};
  f4 acca[2] = {zero, zero}, accb[2] = {c.bias[1][0], c.bias[1][1]};
  p1s_mma(acca, c.w[0], bh[0], bl[0]);
  p1s_mma(accb, c.w[1], bh[1], bl[1]);
  p1s_store<LEAKY, kP1sPlane>(acca, A + (PAR & 3) * 2 * kP1sPlane, x, kq, c.alpha, y < kP1sHin && x < 12, c.amax);
  p1s_store<LEAKY, kP1sBPlane>(accb, sm + kP1sB + ((PAR + 1) & 1) * 2 * kP1sBPlane, x, kq, c.alpha,
                   y >= 3 && y - 3 < kP1sHin - 2 && x < 12, c.amax);
}

// wave 1, iteration y: c(y - 4), d(y - 7) pooled with row y - 8 when y - 7 is odd
template <int PAR, bool LEAKY>
__device__ __forceinline__ void p1s_iter1(P1sCtx& c, int y, _Float16* sm, float* obase, int x, int kq) {
  const _Float16* B = sm + kP1sB + (PAR & 1) * 2 * kP1sBPlane;  // row y - 4
  _Float16* C = sm + kP1sCr;
  h8 bh[2][3], bl[2][3];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const _Float16* pc = B + (x + ks) * kP1sCS + 8 * kq;
    bh[0][ks] = *reinterpret_cast<const h8*>(pc);
    bl[0][ks] = *reinterpret_cast<const h8*>(pc + kP1sBPlane);
    const _Float16* pd = C + ((PAR + 1 + ks) & 3) * 2 * kP1sPlane + x * kP1sCS + 8 * kq;  // row y - 7 + ks
    bh[1][ks] = *reinterpret_cast<const h8*>(pd);
    bl[1][ks] = *reinterpret_cast<const h8*>(pd + kP1sPlane);
  }
  f4 accc[2] = {c.bias[0][0], c.bias[0][1]};
  f4 accd_odd[2] = {c.bias[1][0], c.bias[1][1]};
  f4(&accd)[2] = ((PAR & 1) == 1) ? c.pool : accd_odd;  // row y - 7 even (y odd): accumulate into the pool
  if ((PAR & 1) == 1) {
    c.pool[0] = c.bias[1][0];
    c.pool[1] = c.bias[1][1];
  }
  p1s_mma(accc, c.w[0], bh[0], bl[0]);
  p1s_mma(accd, c.w[1], bh[1], bl[1]);
  p1s_store<LEAKY, kP1sPlane>(accc, C + (PAR & 3) * 2 * kP1sPlane, x, kq, c.alpha,
                   y >= 4 && y - 4 < kP1sHin - 2 && x < 10, c.amax);
  if ((PAR & 1) == 0) {  // row y - 7 odd: pool with row y - 8, store pooled row (y - 8) / 2
    float pv[2][4];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = __builtin_elementwise_maximum(c.pool[mb][j], accd[mb][j]);
        const float u = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, t), 0xB1, 0xf, 0xf,
                                                                           false));
        pv[mb][j] = __builtin_elementwise_maximum(t, u);
      }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      leaky_max2<LEAKY>(pv[mb][0], pv[mb][1], c.alpha);
      leaky_max2<LEAKY>(pv[mb][2], pv[mb][3], c.alpha);
    }
    if (y >= 8 && y - 8 < 2 * kP1sHout && !(x & 1) && x < 2 * kP1sWo) {
      float* o = obase + static_cast<int64_t>((y - 8) >> 1) * (kP1sWo * kP1sCo) + (x >> 1) * kP1sCo + 4 * kq;
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
        *reinterpret_cast<float4*>(o + 16 * mb) = float4{pv[mb][0], pv[mb][1], pv[mb][2], pv[mb][3]};
    }
  }
}

template <bool LEAKY>
__global__ void __launch_bounds__(kP1sThreads) __attribute__((amdgpu_waves_per_eu(2)))
p1s_chain_kernel(P1Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char p1smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = lane & 15, kq = lane >> 4;
  _Float16* sm = reinterpret_cast<_Float16*>(p1smem);
  // never-written positions: input 14 .. 17 (both slots, planes), B 16, 17; the ones / zeros slots
  for (int i = threadIdx.x; i < 2 * 2 * 4 * kP1sCSI; i += kP1sThreads) {
    const int s = i / (8 * kP1sCSI), rest = i - s * 8 * kP1sCSI, pl = rest / (4 * kP1sCSI);
    sm[kP1sIn + s * kP1sInSlot + pl * kP1sInPlane + 14 * kP1sCSI + rest % (4 * kP1sCSI)] = static_cast<_Float16>(0.f);
  }
  for (int i = threadIdx.x; i < 2 * 2 * 2 * kP1sCS; i += kP1sThreads) {
    const int s = i / (4 * kP1sCS), rest = i - s * 4 * kP1sCS, pl = rest / (2 * kP1sCS);
    sm[kP1sB + s * 2 * kP1sBPlane + pl * kP1sBPlane + 16 * kP1sCS + rest % (2 * kP1sCS)] = static_cast<_Float16>(0.f);
  }
  if (threadIdx.x < 64) {
    const int s = lane >> 5, k = lane & 31;
    sm[kP1sIn + s * kP1sInSlot + 2 * kP1sInPlane + k] = static_cast<_Float16>(k == 0 ? 1.f : 0.f);
  }
  // stage a's K step 2: lanes kq 0 read group 8 (tap 2, c 2), kq 1 the ones slot (bias), kq 2, 3 zeros
  const int a2h = kq == 0 ? x * kP1sCSI + 64 : 2 * kP1sInPlane + (kq == 1 ? 0 : 16);
  const int a2l = kq == 0 ? kP1sInPlane : 8;
  P1sCtx c;
  c.alpha = a.alpha;
  c.amax = 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        const _Float16* wp = a.w + (2 * wave + s) * kP1sStageHalfs + (16 * mb + x) * 96 + 32 * ks + 8 * kq;
        c.w[s].h[mb][ks] = *reinterpret_cast<const h8*>(wp);
        c.w[s].l[mb][ks] = *reinterpret_cast<const h8*>(wp + 32 * 96);
      }
  // biases of stages b, c, d ([3][32]): wave 0 keeps b's in bias[1], wave 1 c's and d's
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int st = wave == 0 ? 0 : s + 1;
      const float4 b = *reinterpret_cast<const float4*>(a.bias + 32 * st + 16 * mb + 4 * kq);
      c.bias[wave == 0 ? 1 : s][mb] = f4{b.x, b.y, b.z, b.w};
    }
  __syncthreads();
  const int hmax = a.H_in - 1;
  for (int64_t img = blockIdx.x; img < a.n_img; img += gridDim.x) {
    const float* src = a.in + img * a.src_img_stride;
    float* obase = a.out + img * (static_cast<int64_t>(kP1sHout) * kP1sWo * kP1sCo);
    if (wave == 0) {  // input row 0 straight into slot 0; rows 1 .. 4 into the queue (slot = row & 3)
      float4 v[2];
      v[0] = *reinterpret_cast<const float4*>(src + 4 * lane);
      v[1] = *reinterpret_cast<const float4*>(src + 4 * min(lane + 64, kP1sWi * 6 - 1));
      float amx = 0.f;
      p1s_stage_row(v, sm + kP1sIn, lane, amx);
      asm("v_max_f32 %0, %0, %1" : "+v"(c.amax) : "v"(amx));
#pragma unroll
      for (int r = 1; r <= 4; ++r) {
        const float* rp = src + static_cast<int64_t>(min(r, hmax)) * (kP1sWi * kP1sCSI);
        c.q[r & 3][0] = *reinterpret_cast<const float4*>(rp + 4 * lane);
        c.q[r & 3][1] = *reinterpret_cast<const float4*>(rp + 4 * min(lane + 64, kP1sWi * 6 - 1));
      }
    }
    __syncthreads();
    for (int y0 = 0; y0 < 72; y0 += 4) {
#define HBK_P1S_STEP(P)                                                              \
  if (wave == 0)                                                                     \
    p1s_iter0<P, LEAKY>(c, y0 + P, sm, src, hmax, x, kq, lane, a2h, a2l);            \
  else                                                                               \
    p1s_iter1<P, LEAKY>(c, y0 + P, sm, obase, x, kq);                                \
  __syncthreads();
      HBK_P1S_STEP(0)
      HBK_P1S_STEP(1)
      HBK_P1S_STEP(2)
      HBK_P1S_STEP(3)
#undef HBK_P1S_STEP
    }
  }
  raise_range(a.range_flag, c.amax);
}

// ------------------------------------------------------------------ p2s ----
// Streaming form of SE20's chain 2 (the prefix's last chain, no output pool:
// 31 x 5 x 32 -> 1x3 32 -> 48 -> 3x1 -> 1x3 -> 3x1 48 -> 48 -> 27 x 1 x 48).
// Its rows are 3 or 1 positions wide, so a tile packs CLIPS: a workgroup
// streams the rows of 16 clips at once, and a 16-position tile of
// v_mfma_f32_16x16x32_f16 is (clip, column) for stages a, b (48 positions: 3
// tiles) and the clip for stages c, d (1 tile). Eight waves, one unit each,
// with that unit's weights in VGPRs: waves 0-2 stage a tiles 0-2, waves 3-5
// stage b tiles 0-2, wave 6 stage c, wave 7 stage d. Tick y (one workgroup
// barrier after it): a(y), b(y - 3), c(y - 4), d(y - 7), and every wave
// stages its share of input row y + 1. Rings as in p1s. K groups of 8
// (g = 4 ks + kq): a: g = dx * 4 + c (32 input channels); b, c, d: g = tap * 6
// + c (48 channels), g = 18 the bias slot (B = 1), g = 19 zeros; stage a
// starts its accumulators at the bias.
// (the kP2s* geometry and P2sArgs: hbk_embed_args.h)

// the wave's weights: [output block][K step] hi / lo
template <int KS>
struct P2sW {
  h8 h[3][KS], l[3][KS];
};

// (the three products spelled out: through mma3, p2s_chain_kernel<false> is scheduled differently)
template <int KS>
__device__ __forceinline__ void p2s_mma(f4 (&acc)[3], const P2sW<KS>& w, int ks, const h8& bh, const h8& bl) {
#pragma unroll
  for (int mb = 0; mb < 3; ++mb) {
    acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[mb][ks], bh, acc[mb], 0, 0, 0);
    acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[mb][ks], bl, acc[mb], 0, 0, 0);
    acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.l[mb][ks], bh, acc[mb], 0, 0, 0);
  }
}

// activation, split and LDS store of a finished tile (channels 16 mb + 4 kq + j at position p;
// the lo plane PL behind the hi plane)
template <bool LEAKY, int PL>
__device__ __forceinline__ void p2s_store(const f4 (&acc)[3], _Float16* oh, int p, int kq, float alpha, bool track_it,
                                          float& amax) {
  store_tiles<LEAKY, 3, kP2sCS, PL>(acc, oh, p, kq, alpha, track_it, amax);
}

// every thread's share of input row `row` of the group's clips (640 float4): load / stage
struct P2sRow {
  float4 v[2];
};
__device__ __forceinline__ void p2s_load_row(P2sRow& r, const P2sArgs& a, int64_t img0, int row, int tid) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = min(tid + kP2sThreads * u, kP2sClips * kP2sWi * kP2sCi / 4 - 1);
    const int c = i / 40, rem = i - 40 * c;
    const int64_t img = min(img0 + c, a.n_img - 1);
    r.v[u] = *reinterpret_cast<const float4*>(a.in + img * a.src_img_stride + min(row, kP2sHin - 1) *
                                              (kP2sWi * kP2sCi) + 4 * rem);
  }
}
__device__ __forceinline__ void p2s_stage_row(const P2sRow& r, _Float16* slot, int tid, float& amax) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = tid + kP2sThreads * u;
    if (u == 0 || i < kP2sClips * kP2sWi * kP2sCi / 4) {
      const int c = i / 40, rem = i - 40 * c, col = rem >> 3, c4 = rem & 7;
      uint32_t h01, l01, h23, l23;
      split2(r.v[u].x, r.v[u].y, h01, l01, amax);
      split2(r.v[u].z, r.v[u].w, h23, l23, amax);
      const int o = (c * kP2sWi + col) * kP2sCSI + 4 * c4;
      *reinterpret_cast<uint2*>(slot + o) = uint2{h01, h23};
      *reinterpret_cast<uint2*>(slot + kP2sInPlane + o) = uint2{l01, l23};
    }
  }
}

template <bool LEAKY>
__global__ void __launch_bounds__(kP2sThreads) __attribute__((amdgpu_waves_per_eu(2)))
p2s_chain_kernel(P2sArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char p2smem[];
  _Float16* sm = reinterpret_cast<_Float16*>(p2smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pl = lane & 15, kq = lane >> 4;
  if (tid < 32) sm[kP2sOnes + tid] = static_cast<_Float16>(tid == 0 ? 1.f : 0.f);  // ones (hi, lo), zeros
  const int64_t n_groups = (a.n_img + kP2sClips - 1) / kP2sClips;
  float amax = 0.f;
  const float alpha = a.alpha;
  const _Float16* ones = sm + kP2sOnes;
  // K groups g = 4 ks + kq of stages b, c, d: tap g / 6, channel group g % 6; g >= 18: bias / zeros slot
  auto tap_of = [&](int ks) { return (4 * ks + kq) / 6; };
  auto cg_of = [&](int ks) { return (4 * ks + kq) % 6; };

  if (wave < 3) {  // ---------------- stage a, tile t = wave: positions p = 3 clip + column
    const int t = wave, p = 16 * t + pl, c = p / 3, x = p - 3 * c;
    P2sW<3> W;
#pragma unroll
    for (int mb = 0; mb < 3; ++mb)
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        const _Float16* wp = a.w + (16 * mb + pl) * kP2sKa + 32 * ks + 8 * kq;
        W.h[mb][ks] = *reinterpret_cast<const h8*>(wp);
        W.l[mb][ks] = *reinterpret_cast<const h8*>(wp + kP2sCo * kP2sKa);
      }
    f4 bias[3];
#pragma unroll
    for (int mb = 0; mb < 3; ++mb) {
      const float4 b = *reinterpret_cast<const float4*>(a.bias_a + 16 * mb + 4 * kq);
      bias[mb] = f4{b.x, b.y, b.z, b.w};
    }
    const int base = (c * kP2sWi + x) * kP2sCSI + 8 * kq;  // + 40 ks: column x + ks, channels 8 kq
    for (int64_t gi = blockIdx.x; gi < n_groups; gi += gridDim.x) {
      const int64_t img0 = gi * kP2sClips;
      P2sRow q0, q1;
      p2s_load_row(q0, a, img0, 0, tid);
      p2s_load_row(q1, a, img0, 1, tid);
      p2s_stage_row(q0, sm + kP2sIn, tid, amax);
      p2s_load_row(q0, a, img0, 2, tid);
      __syncthreads();
      for (int y = 0; y < kP2sTicks; ++y) {
        const _Float16* in = sm + kP2sIn + (y & 1) * 2 * kP2sInPlane;
        h8 bh[3], bl[3];
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
          bh[ks] = *reinterpret_cast<const h8*>(in + base + kP2sCSI * ks);
          bl[ks] = *reinterpret_cast<const h8*>(in + kP2sInPlane + base + kP2sCSI * ks);
        }
        {  // input row y + 1 (loaded a tick ago) -> the other slot; load row y + 3
          float m = 0.f;
          p2s_stage_row((y & 1) ? q0 : q1, sm + kP2sIn + ((y + 1) & 1) * 2 * kP2sInPlane, tid, m);
          asm("v_max_f32 %0, %0, %1" : "+v"(amax) : "v"(y + 1 < kP2sHin ? m : 0.f));
          if (y & 1) p2s_load_row(q0, a, img0, y + 3, tid);
          else p2s_load_row(q1, a, img0, y + 3, tid);
        }
        f4 acc[3] = {bias[0], bias[1], bias[2]};
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) p2s_mma<3>(acc, W, ks, bh[ks], bl[ks]);
        p2s_store<LEAKY, kP2sAPlane>(acc, sm + kP2sA + (y & 3) * 2 * kP2sAPlane, p, kq, alpha, y < kP2sHin, amax);
        __syncthreads();
      }
    }
  } else if (wave < 6) {  // ---------------- stage b (3x1 on the A ring), tile t = wave - 3
    const int t = wave - 3, p = 16 * t + pl;
    P2sW<5> W;
#pragma unroll
    for (int mb = 0; mb < 3; ++mb)
#pragma unroll
      for (int ks = 0; ks < 5; ++ks) {
        const _Float16* wp = a.w + 2 * kP2sCo * kP2sKa + (16 * mb + pl) * kP2sK + 32 * ks + 8 * kq;
        W.h[mb][ks] = *reinterpret_cast<const h8*>(wp);
        W.l[mb][ks] = *reinterpret_cast<const h8*>(wp + kP2sCo * kP2sK);
      }
    for (int64_t gi = blockIdx.x; gi < n_groups; gi += gridDim.x) {
      const int64_t img0 = gi * kP2sClips;
      P2sRow q0, q1;
      p2s_load_row(q0, a, img0, 0, tid);
      p2s_load_row(q1, a, img0, 1, tid);
      p2s_stage_row(q0, sm + kP2sIn, tid, amax);
      p2s_load_row(q0, a, img0, 2, tid);
      __syncthreads();
      for (int y = 0; y < kP2sTicks; ++y) {
        f4 acc[3] = {};
#pragma unroll
        for (int ks = 0; ks < 5; ++ks) {
          const int tap = tap_of(ks), cg = cg_of(ks);
          const bool bias_slot = 4 * ks + kq >= 18;
          const _Float16* pb = bias_slot ? ones + (kq == 2 ? 0 : 16)
                                         : sm + kP2sA + ((y + 1 + tap) & 3) * 2 * kP2sAPlane + p * kP2sCS + 8 * cg;
          const int lo = bias_slot ? 8 : kP2sAPlane;
          const h8 bh = *reinterpret_cast<const h8*>(pb), bl = *reinterpret_cast<const h8*>(pb + lo);
          p2s_mma<5>(acc, W, ks, bh, bl);
        }
        {
          float m = 0.f;
          p2s_stage_row((y & 1) ? q0 : q1, sm + kP2sIn + ((y + 1) & 1) * 2 * kP2sInPlane, tid, m);
          asm("v_max_f32 %0, %0, %1" : "+v"(amax) : "v"(y + 1 < kP2sHin ? m : 0.f));
          if (y & 1) p2s_load_row(q0, a, img0, y + 3, tid);
          else p2s_load_row(q1, a, img0, y + 3, tid);
        }
        p2s_store<LEAKY, kP2sAPlane>(acc, sm + kP2sB + ((y + 1) & 1) * 2 * kP2sAPlane, p, kq, alpha,
                         y >= 3 && y - 3 < kP2sHin - 2, amax);
        __syncthreads();
      }
    }
  } else {  // ---------------- stage c (wave 6: 1x3 on B) or d (wave 7: 3x1 on the C ring); position = clip
    const bool is_c = wave == 6;
    P2sW<5> W;
#pragma unroll
    for (int mb = 0; mb < 3; ++mb)
#pragma unroll
      for (int ks = 0; ks < 5; ++ks) {
        const _Float16* wp = a.w + 2 * kP2sCo * kP2sKa + (is_c ? 1 : 2) * 2 * kP2sCo * kP2sK + (16 * mb + pl) * kP2sK +
                             32 * ks + 8 * kq;
        W.h[mb][ks] = *reinterpret_cast<const h8*>(wp);
        W.l[mb][ks] = *reinterpret_cast<const h8*>(wp + kP2sCo * kP2sK);
      }
    for (int64_t gi = blockIdx.x; gi < n_groups; gi += gridDim.x) {
      const int64_t img0 = gi * kP2sClips;
      P2sRow q0, q1;
      p2s_load_row(q0, a, img0, 0, tid);
      p2s_load_row(q1, a, img0, 1, tid);
      p2s_stage_row(q0, sm + kP2sIn, tid, amax);
      p2s_load_row(q0, a, img0, 2, tid);
      __syncthreads();
      for (int y = 0; y < kP2sTicks; ++y) {
        f4 acc[3] = {};
#pragma unroll
        for (int ks = 0; ks < 5; ++ks) {
          const int tap = tap_of(ks), cg = cg_of(ks);
          const bool bias_slot = 4 * ks + kq >= 18;
          const _Float16* src;
          int lo;
          if (is_c) {  // B row y - 4, position (clip, tap), channels 8 cg
            src = sm + kP2sB + (y & 1) * 2 * kP2sAPlane + (3 * pl + tap) * kP2sCS + 8 * cg;
            lo = kP2sAPlane;
          } else {     // C ring row y - 7 + tap, position clip
            src = sm + kP2sC + ((y + 1 + tap) & 3) * 2 * kP2sCPlane + pl * kP2sCS + 8 * cg;
            lo = kP2sCPlane;
          }
          const _Float16* pb = bias_slot ? ones + (kq == 2 ? 0 : 16) : src;
          if (bias_slot) lo = 8;
          const h8 bh = *reinterpret_cast<const h8*>(pb), bl = *reinterpret_cast<const h8*>(pb + lo);
          p2s_mma<5>(acc, W, ks, bh, bl);
        }
        {
          float m = 0.f;
          p2s_stage_row((y & 1) ? q0 : q1, sm + kP2sIn + ((y + 1) & 1) * 2 * kP2sInPlane, tid, m);
          asm("v_max_f32 %0, %0, %1" : "+v"(amax) : "v"(y + 1 < kP2sHin ? m : 0.f));
          if (y & 1) p2s_load_row(q0, a, img0, y + 3, tid);
          else p2s_load_row(q1, a, img0, y + 3, tid);
        }
        if (is_c) {
          p2s_store<LEAKY, kP2sCPlane>(acc, sm + kP2sC + (y & 3) * 2 * kP2sCPlane, pl, kq, alpha,
                           y >= 4 && y - 4 < kP2sHin - 2, amax);
        } else if (y >= 7 && y - 7 < kP2sHout && img0 + pl < a.n_img) {
          float* o = a.out + (img0 + pl) * (kP2sHout * kP2sCo) + (y - 7) * kP2sCo + 4 * kq;
#pragma unroll
          for (int mb = 0; mb < 3; ++mb) {
            float v[4] = {acc[mb][0], acc[mb][1], acc[mb][2], acc[mb][3]};
            leaky_max2<LEAKY>(v[0], v[1], alpha);
            leaky_max2<LEAKY>(v[2], v[3], alpha);
            *reinterpret_cast<float4*>(o + 16 * mb) = float4{v[0], v[1], v[2], v[3]};
          }
        }
        __syncthreads();
      }
    }
  }
  raise_range(a.range_flag, amax);
}

// ------------------------------------------------------------------ t3s ----
// Streaming form of SE20's tail (chain 3 over the phase images of the tail
// deduplication): the input pool 2x1 over p2s's 27 x 1 x 48 rows, then
// 3x1 (48 -> 64), 1x1, 3x1, 1x1 (64), 2x1 (64 -> 96), four 1x1 (96; the last
// without activation): 8 x 1 x 96 per phase image. The rows are one position
// wide, so a tile packs IMAGES: 16 positions = 8 clips x 2 phase images
// (position p = image img0 + p, image = 2 clip + phase). The weights are the A
// operand in VGPRs (hi / lo f16), the activations the B operand from LDS rings
// (hi / lo planes [position][channel]); the bias starts the accumulator. Waves
// 0-3 run the four 64-channel stages for output block mb = wave, waves 4-9 the
// five 96-channel stages for mb = wave - 4. Tick y (one barrier after it):
// pooled row y is staged (waves 0-2, loaded a tick ahead), stage s computes its
// row y - kT3Delay[s] (each stage reads only rows written in earlier ticks).
// (the kT3* geometry and T3sArgs: hbk_embed_args.h)

// one output block (16 channels) of one row: KS K-steps of 32, B from the
// ring rows `rows` (tap t -> rows[t]), channel group 8 cg of tap g / (CIN / 8)
template <int KS, int CIN, int CS, int PL>
__device__ __forceinline__ f4 t3_block(const h8 (&wh)[KS], const h8 (&wl)[KS], f4 acc, const _Float16* sm,
                                       const int (&rowoff)[3], int pos, int kq, const _Float16* zero) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int g = 4 * ks + kq, tap = g / (CIN / 8), cg = g - tap * (CIN / 8);
    const bool pad = tap >= 3;  // stage 1's K padding (groups 18, 19)
    const _Float16* src = pad ? zero : sm + rowoff[tap < 3 ? tap : 0] + pos * CS + 8 * cg;
    const h8 bh = *reinterpret_cast<const h8*>(src), bl = *reinterpret_cast<const h8*>(pad ? zero : src + PL);
    acc = mma3(wh[ks], wl[ks], bh, bl, acc);
  }
  return acc;
}
// (a block's tile goes to its ring through store_tile, hbk_embed_dev.h)

template <int KS, int K>
__device__ __forceinline__ void t3_load_w(h8 (&wh)[KS], h8 (&wl)[KS], const _Float16* w, int cout, int n, int kq) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    wh[ks] = *reinterpret_cast<const h8*>(w + n * K + 32 * ks + 8 * kq);
    wl[ks] = *reinterpret_cast<const h8*>(w + cout * K + n * K + 32 * ks + 8 * kq);
  }
}

__device__ __forceinline__ f4 t3_bias(const float* b) {
  const float4 v = *reinterpret_cast<const float4*>(b);
  return f4{v.x, v.y, v.z, v.w};
}

template <bool LEAKY>
__global__ void __launch_bounds__(kT3Threads) __attribute__((amdgpu_waves_per_eu(3)))
t3s_chain_kernel(T3sArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char t3smem[];
  _Float16* sm = reinterpret_cast<_Float16*>(t3smem);
  float* sb = reinterpret_cast<float*>(t3smem + kT3BiasOff);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pos = lane & 15, kq = lane >> 4;
  for (int i = tid; i < 16; i += kT3Threads) sm[kT3Zero + i] = static_cast<_Float16>(0.f);
  for (int i = tid; i < 4 * kT3C1 + 5 * kT3C2; i += kT3Threads) sb[i] = a.bias[i];
  const _Float16* zero = sm + kT3Zero;
  const int64_t n_groups = (a.n_img + kT3Pos - 1) / kT3Pos;
  const float alpha = a.alpha;
  float amax = 0.f;
  // staging: threads 0..191 take 4 channels (c4) of position sp
  const int sp = tid / 12, c4 = tid - 12 * sp;
  const bool stager = tid < kT3Pos * 12;
  float4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0;
  auto load_row = [&](int64_t img0, int y) {  // pooled row y's two source rows, this thread's share
    const int64_t img = min(img0 + sp, a.n_img - 1);
    const int64_t clip = img >> 1;
    const int row = static_cast<int>(img & 1) + 2 * min(y, kT3Hp - 1);
    const float* src = a.in + clip * a.src_clip_stride + row * kT3C0 + 4 * c4;
    r0 = *reinterpret_cast<const float4*>(src);
    r1 = *reinterpret_cast<const float4*>(src + kT3C0);
  };
  auto stage_row = [&](int y) {
    const float4 v = {nan_max(r0.x, r1.x), nan_max(r0.y, r1.y), nan_max(r0.z, r1.z), nan_max(r0.w, r1.w)};
    uint32_t h01, l01, h23, l23;
    split2(v.x, v.y, h01, l01, amax);
    split2(v.z, v.w, h23, l23, amax);
    _Float16* d = sm + kT3P + (y & 3) * 2 * kT3PlP + sp * kT3CS0 + 4 * c4;
    *reinterpret_cast<uint2*>(d) = uint2{h01, h23};
    *reinterpret_cast<uint2*>(d + kT3PlP) = uint2{l01, l23};
  };
  __syncthreads();

  if (wave < 4) {  // ---------------- the 64-channel stages, block mb = wave
    const int mb = wave, n = 16 * mb + pos;
    h8 w1h[5], w1l[5], w2h[2], w2l[2], w3h[6], w3l[6], w4h[2], w4l[2];
    t3_load_w<5, 160>(w1h, w1l, a.w + kT3W[0], kT3C1, n, kq);
    t3_load_w<2, 64>(w2h, w2l, a.w + kT3W[1], kT3C1, n, kq);
    t3_load_w<6, 192>(w3h, w3l, a.w + kT3W[2], kT3C1, n, kq);
    t3_load_w<2, 64>(w4h, w4l, a.w + kT3W[3], kT3C1, n, kq);
    const int bo = 16 * mb + 4 * kq;
    for (int64_t gi = blockIdx.x; gi < n_groups; gi += gridDim.x) {
      const int64_t img0 = gi * kT3Pos;
      if (stager) load_row(img0, 0);
      for (int y = 0; y < kT3Ticks; ++y) {
        if (stager && y < kT3Hp) {
          stage_row(y);
          load_row(img0, y + 1);
        }
        if (y >= 3 && y < 3 + 11) {  // stage 1: row r from pooled rows r .. r + 2
          const int r = y - 3;
          const int ro[3] = {kT3P + (r & 3) * 2 * kT3PlP, kT3P + ((r + 1) & 3) * 2 * kT3PlP,
                             kT3P + ((r + 2) & 3) * 2 * kT3PlP};
          const f4 acc = t3_block<5, kT3C0, kT3CS0, kT3PlP>(w1h, w1l, t3_bias(sb + bo), sm, ro, pos, kq, zero);
          store_tile<LEAKY, kT3CS1, kT3Pl1>(acc, sm + kT3A1 + (r & 1) * 2 * kT3Pl1, pos, mb, kq, alpha, amax);
        }
        if (y >= 4 && y < 4 + 11) {  // stage 2 (1x1)
          const int r = y - 4;
          const int ro[3] = {kT3A1 + (r & 1) * 2 * kT3Pl1, 0, 0};
          const f4 acc = t3_block<2, kT3C1, kT3CS1, kT3Pl1>(w2h, w2l, t3_bias(sb + kT3C1 + bo), sm, ro, pos, kq, zero);
          store_tile<LEAKY, kT3CS1, kT3Pl1>(acc, sm + kT3A2 + (r & 3) * 2 * kT3Pl1, pos, mb, kq, alpha, amax);
        }
        if (y >= 7 && y < 7 + 9) {  // stage 3 (3x1)
          const int r = y - 7;
          const int ro[3] = {kT3A2 + (r & 3) * 2 * kT3Pl1, kT3A2 + ((r + 1) & 3) * 2 * kT3Pl1,
                             kT3A2 + ((r + 2) & 3) * 2 * kT3Pl1};
          const f4 acc = t3_block<6, kT3C1, kT3CS1, kT3Pl1>(w3h, w3l, t3_bias(sb + 2 * kT3C1 + bo), sm, ro, pos, kq,
                                                           zero);
          store_tile<LEAKY, kT3CS1, kT3Pl1>(acc, sm + kT3A3 + (r & 1) * 2 * kT3Pl1, pos, mb, kq, alpha, amax);
        }
        if (y >= 8 && y < 8 + 9) {  // stage 4 (1x1)
          const int r = y - 8;
          const int ro[3] = {kT3A3 + (r & 1) * 2 * kT3Pl1, 0, 0};
          const f4 acc = t3_block<2, kT3C1, kT3CS1, kT3Pl1>(w4h, w4l, t3_bias(sb + 3 * kT3C1 + bo), sm, ro, pos, kq,
                                                           zero);
          store_tile<LEAKY, kT3CS1, kT3Pl1>(acc, sm + kT3A4 + (r & 3) * 2 * kT3Pl1, pos, mb, kq, alpha, amax);
        }
        __syncthreads();
      }
    }
  } else {  // ---------------- the 96-channel stages, block mb = wave - 4
    const int mb = wave - 4, n = 16 * mb + pos;
    h8 w5h[4], w5l[4], w6h[3], w6l[3], w7h[3], w7l[3], w8h[3], w8l[3], w9h[3], w9l[3];
    t3_load_w<4, 128>(w5h, w5l, a.w + kT3W[4], kT3C2, n, kq);
    t3_load_w<3, 96>(w6h, w6l, a.w + kT3W[5], kT3C2, n, kq);
    t3_load_w<3, 96>(w7h, w7l, a.w + kT3W[6], kT3C2, n, kq);
    t3_load_w<3, 96>(w8h, w8l, a.w + kT3W[7], kT3C2, n, kq);
    t3_load_w<3, 96>(w9h, w9l, a.w + kT3W[8], kT3C2, n, kq);
    const float* bb = sb + 4 * kT3C1 + 16 * mb + 4 * kq;
    constexpr int A5 = kT3A5, A6 = A5 + 2 * 2 * kT3Pl2, A7 = A6 + 2 * 2 * kT3Pl2, A8 = A7 + 2 * 2 * kT3Pl2;
    for (int64_t gi = blockIdx.x; gi < n_groups; gi += gridDim.x) {
      const int64_t img0 = gi * kT3Pos;
      for (int y = 0; y < kT3Ticks; ++y) {
        if (y >= 10 && y < 10 + 8) {  // stage 5 (2x1, 64 -> 96) from rows r, r + 1 of A4
          const int r = y - 10;
          const int ro[3] = {kT3A4 + (r & 3) * 2 * kT3Pl1, kT3A4 + ((r + 1) & 3) * 2 * kT3Pl1, 0};
          const f4 acc = t3_block<4, kT3C1, kT3CS1, kT3Pl1>(w5h, w5l, t3_bias(bb), sm, ro, pos, kq, zero);
          store_tile<LEAKY, kT3CS2, kT3Pl2>(acc, sm + A5 + (r & 1) * 2 * kT3Pl2, pos, mb, kq, alpha, amax);
        }
        if (y >= 11 && y < 11 + 8) {  // stage 6
          const int r = y - 11;
          const int ro[3] = {A5 + (r & 1) * 2 * kT3Pl2, 0, 0};
          const f4 acc = t3_block<3, kT3C2, kT3CS2, kT3Pl2>(w6h, w6l, t3_bias(bb + kT3C2), sm, ro, pos, kq, zero);
          store_tile<LEAKY, kT3CS2, kT3Pl2>(acc, sm + A6 + (r & 1) * 2 * kT3Pl2, pos, mb, kq, alpha, amax);
        }
        if (y >= 12 && y < 12 + 8) {  // stage 7
          const int r = y - 12;
          const int ro[3] = {A6 + (r & 1) * 2 * kT3Pl2, 0, 0};
          const f4 acc = t3_block<3, kT3C2, kT3CS2, kT3Pl2>(w7h, w7l, t3_bias(bb + 2 * kT3C2), sm, ro, pos, kq, zero);
          store_tile<LEAKY, kT3CS2, kT3Pl2>(acc, sm + A7 + (r & 1) * 2 * kT3Pl2, pos, mb, kq, alpha, amax);
        }
        if (y >= 13 && y < 13 + 8) {  // stage 8
          const int r = y - 13;
          const int ro[3] = {A7 + (r & 1) * 2 * kT3Pl2, 0, 0};
          const f4 acc = t3_block<3, kT3C2, kT3CS2, kT3Pl2>(w8h, w8l, t3_bias(bb + 3 * kT3C2), sm, ro, pos, kq, zero);
          store_tile<LEAKY, kT3CS2, kT3Pl2>(acc, sm + A8 + (r & 1) * 2 * kT3Pl2, pos, mb, kq, alpha, amax);
        }
        if (y >= 14 && y < 14 + 8) {  // stage 9 (no activation) -> out
          const int r = y - 14;
          const int ro[3] = {A8 + (r & 1) * 2 * kT3Pl2, 0, 0};
          const f4 acc = t3_block<3, kT3C2, kT3CS2, kT3Pl2>(w9h, w9l, t3_bias(bb + 4 * kT3C2), sm, ro, pos, kq, zero);
          if (img0 + pos < a.n_img) {
            float* o = a.out + (img0 + pos) * a.out_img_stride + r * kT3C2 + 16 * mb + 4 * kq;
            *reinterpret_cast<float4*>(o) = float4{acc[0], acc[1], acc[2], acc[3]};
          }
        }
        __syncthreads();
      }
    }
  }
  raise_range(a.range_flag, amax);
}

}  // namespace

// f = LeakyReLU
const void* embed_stream_kernel(int kind, bool f) {
  switch (static_cast<Kern>(kind)) {
    case Kern::p0s: return f ? addr(p0s_chain_kernel<true>) : addr(p0s_chain_kernel<false>);
    case Kern::p1s: return f ? addr(p1s_chain_kernel<true>) : addr(p1s_chain_kernel<false>);
    case Kern::p2s: return f ? addr(p2s_chain_kernel<true>) : addr(p2s_chain_kernel<false>);
    case Kern::t3s: return f ? addr(t3s_chain_kernel<true>) : addr(t3s_chain_kernel<false>);
    default: return nullptr;
  }
}

}  // namespace hbk
