// Speech-embedding conv stack: the generic split-f16 chain kernel (conv_chain_x3_kernel, any
// chain the planner lays out) with its profiling hooks: the phase counters (HBK_PHASE,
// g_phase_cycles, hbk_debug_phase_cycles; read by tools/probe_embed.py), the phase ablation
// (HBK_SKIP) and the HBK_X3_WAVES_PER_EU / HBK_X3_PF build macros. hbk_embed.hip launches it
// through embed_x3_kernel; XArgs / XStage are in hbk_embed_args.h, their planner in
// hbk_embed_plan.h, the split / activation / range-flag helpers in hbk_embed_dev.h. The
// fixed-shape kernels of the same numerics are in hbk_embed_band.hip and hbk_embed_stream.hip,
// the exact-f32 kernel in hbk_embed_exact.hip.
#include "hbk_embed_dev.h"
#include "hbk_embed_internal.h"

namespace hbk {
namespace {

// ------------------------------------------------- split-f16 conv chain ----
// Same task structure as conv_chain_kernel (hbk_embed_exact.hip); the arithmetic is an fp16 pair per
// value, x = hi + lo (hi = x with its 13 low mantissa bits cleared, i.e. x
// rounded toward zero to fp16's 11 bits; lo = fp16(x - hi)), and each GEMM is
//   acc = W_hi X_hi + W_hi X_lo + W_lo X_hi
// on v_mfma_f32_32x32x16_f16 (f32 accumulation): ~2^-22 relative per operand
// (lo loses bits only below fp16's subnormal step, 2^-24 absolute; the
// dropped W_lo X_lo is 2^-22 relative). WEIGHTS are the A
// operand (32 output channels) and 32 output POSITIONS as the B operand, so a
// lane of the accumulator holds 4 consecutive channels of one position: the
// epilogue packs them (v_cvt_pkrtz) and stores 8 B per plane.
// Activations live in LDS as two fp16 planes [pos][cs] (cs = channels rounded
// to 8, with cs / 8 odd so the 16-B fragment reads of 32 consecutive positions
// are conflict-free); a K-group is 8 consecutive channels of one tap, the unit
// of one lane's ds_read_b128. Weights are [n][wrow] fp16 planes (k contiguous
// per output channel). A first stage whose cin is not a multiple of 8 (the
// mel input, cin 1) is expanded im2col-style during staging and runs as a
// 1x1 conv. Staging / store loops use a per-kernel 2-D thread mapping (row x
// unit) so no integer division runs per element.
constexpr int kXWaves = kXThreads / 64;

#if defined(HBK_PHASE_TIMING) || defined(HBK_ABLATE)
#define HBK_SKIP(bit) (a.dbg_skip & (1 << (bit)))
#else
#define HBK_SKIP(bit) false
#endif
#ifdef HBK_PHASE_TIMING
// Profiling build only (build.py --phase-timing): wave 0 of every block adds
// the s_memtime cycles of each task phase (staging, im2col, stage s, store;
// barrier waits included in the phase before them) into g_phase_cycles.
__device__ unsigned long long g_phase_cycles[64];  // [chain slot (4)][phase (16)]
#define HBK_PHASE(i)                                                          \
  do {                                                                        \
    if (threadIdx.x == 0) {                                                   \
      const unsigned long long t_ = __builtin_amdgcn_s_memtime();             \
      atomicAdd(&g_phase_cycles[a.dbg_slot * 16 + (i)], t_ - phase_t0);      \
      phase_t0 = t_;                                                          \
    }                                                                         \
  } while (0)
#else
#define HBK_PHASE(i) \
  do {               \
  } while (0)
#endif

constexpr int kXStageInts = sizeof(XStage) / 4;
constexpr int kI2cLds = 256;  // im2col tap table entries kept in LDS

// A stage descriptor from the block's LDS copy, as uniform (scalar) values.
__device__ __forceinline__ XStage lds_stage(const int* p) {
  XStage S;
  int* d = reinterpret_cast<int*>(&S);
#pragma unroll
  for (int i = 0; i < kXStageInts; ++i) d[i] = __builtin_amdgcn_readfirstlane(p[i]);
  return S;
}

// q = n / d for 0 <= n < 2^24, d >= 1, from a float reciprocal (one
// correction step covers its rounding); inv = 1.f / d
__device__ __forceinline__ int div_small(int n, int d, float inv) {
  int q = static_cast<int>(static_cast<float>(n) * inv);
  const int r = n - q * d;
  q += (r >= d) ? 1 : 0;
  q -= (r < 0) ? 1 : 0;
  return q;
}

// 2-D mapping of kXThreads threads onto rows of `units` work items: rpp rows
// per pass; this thread takes unit t_u of row t_row (+ rpp per pass). When a
// row has more units than threads, rpp = 1 and the unit loop strides by
// kXThreads.
struct RowMap {
  int rpp, t_row, t_u, u_step;
  __device__ __forceinline__ RowMap(int units, int tid) {
    if (units <= kXThreads) {
      rpp = kXThreads / units;
      t_row = tid / units;
      t_u = tid - t_row * units;
      u_step = units;  // one unit per row per thread
      if (t_row >= rpp) t_row = 1 << 30;  // idle thread
    } else {
      rpp = 1;
      t_row = 0;
      t_u = tid;
      u_step = kXThreads;
    }
  }
};

// Yf != nullptr: the chain's last stage, written as f32 [m][coutr] for the
// pooled store (no split / reconstruct).
template <int NB, int RB>
__device__ __forceinline__ void xstage(const _Float16* __restrict__ Xh, const _Float16* __restrict__ Xl,
                                       _Float16* __restrict__ Yh, _Float16* __restrict__ Yl,
                                       float* __restrict__ Yf, const _Float16* __restrict__ Wh,
                                       const int* __restrict__ kt, const float* __restrict__ bias, int M,
                                       int hA, int wA, int ho, int wo, const XStage& S, int lane, int wave,
                                       int* flag, int cb) {
  // output channels 32 (cb + c) + ..., c < NB: one group of at most 3 blocks of a wider stage
  const int img_pos = ho * wo;
  const int nrb = (M + 31) >> 5;
  const int r32 = lane & 31, khalf = lane >> 5;
  const int cstride = 32 * S.wrow;
  const _Float16* wp = Wh + cb * cstride + r32 * S.wrow + khalf * 8;
  // input position of output m = (g, y, x): with ytot = g ho + y = m / wo,
  // (g hA + y) wA + x = m + ytot (wA - wo) + g (hA - ho) wA
  const float inv_wo = 1.f / static_cast<float>(wo), inv_ho = 1.f / static_cast<float>(ho);
  const bool one_img = M <= img_pos;
  // this lane's biases, channels n = 32 c + 8 q + 4 khalf + j (register 4 q + j)
  f16x bl[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 b = *reinterpret_cast<const float4*>(bias + (cb + c) * 32 + 8 * q + 4 * khalf);
      bl[c][4 * q] = b.x;
      bl[c][4 * q + 1] = b.y;
      bl[c][4 * q + 2] = b.z;
      bl[c][4 * q + 3] = b.w;
    }
  for (int rb0 = wave * RB; rb0 < nrb; rb0 += kXWaves * RB) {
    int xoff[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int m = min((rb0 + r) * 32 + r32, M - 1);
      const int ytot = div_small(m, wo, inv_wo);
      const int g = one_img ? 0 : div_small(ytot, ho, inv_ho);
      xoff[r] = (m + ytot * (wA - wo) + g * (hA - ho) * wA) * S.cs_in;
    }
    (void)img_pos;
    f16x acc[RB][NB];
    // software-pipelined K loop over two fragment sets: the LDS reads of step
    // ks + 1 are in flight while the MFMAs of step ks run (the prefetch index
    // is clamped, so the last step re-reads its own fragments harmlessly)
    struct Frag {
      h8 xh[RB], xl[RB], wh[NB], wl[NB];
    };
    auto load = [&](Frag& f, int ks) {
      const int ko = kt[2 * ks + khalf];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        f.xh[r] = *reinterpret_cast<const h8*>(Xh + xoff[r] + ko);
        f.xl[r] = *reinterpret_cast<const h8*>(Xl + xoff[r] + ko);
      }
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        f.wh[c] = *reinterpret_cast<const h8*>(wp + c * cstride + ks * 16);
        f.wl[c] = *reinterpret_cast<const h8*>(wp + S.w_lo + c * cstride + ks * 16);
      }
    };
    // three products per tile, the tiles interleaved so that consecutive
    // MFMAs never chain on one accumulator (so not mma3, which chains its three:
    // through it every conv_chain_x3_kernel compiles to other code)
    auto mma = [&](const Frag& f, bool first) {
#pragma unroll
      for (int c = 0; c < NB; ++c) {
#pragma unroll
        for (int r = 0; r < RB; ++r)
          acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.wh[c], f.xh[r], first ? bl[c] : acc[r][c], 0, 0,
                                                              0);
#pragma unroll
        for (int r = 0; r < RB; ++r)
          acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.wh[c], f.xl[r], acc[r][c], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < RB; ++r)
          acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.wl[c], f.xh[r], acc[r][c], 0, 0, 0);
      }
    };
    const int last = S.ksteps - 1;
    Frag fa, fb;
    load(fa, 0);
    load(fb, min(1, last));
    mma(fa, true);
    int ks = 1;
    for (; ks < last; ks += 2) {
      load(fa, ks + 1);
      mma(fb, false);
      load(fb, min(ks + 2, last));
      mma(fa, false);
    }
    if (ks == last) mma(fb, false);
    // D[n][m]: this lane holds position m = tile + (lane & 31) and channels
    // n = 32 c + 8 q + 4 (lane >> 5) + j for register i = 4 q + j
    float m4 = 0.f;  // range guard over this epilogue's split values
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int m = (rb0 + r) * 32 + r32;
      if (m >= M) continue;
      _Float16* yh = Yh + m * S.cs_out;
      _Float16* yl = Yl + m * S.cs_out;
#pragma unroll
      for (int c = 0; c < NB; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // coutr is a multiple of 8, so this test is the same for both lane halves (uniform)
          if ((cb + c) * 32 + 8 * q >= S.coutr) continue;
          const int n0 = (cb + c) * 32 + 8 * q + 4 * khalf;
          // (the bias is the first MFMA's accumulator input)
          float v[4] = {acc[r][c][4 * q], acc[r][c][4 * q + 1], acc[r][c][4 * q + 2], acc[r][c][4 * q + 3]};
          if (S.act == 1) {  // LeakyReLU, 0 <= alpha <= 1: max(v, alpha v) (NaN stays NaN)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = leaky_max<true>(v[j], S.alpha);
          } else if (S.act == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] >= 0.f ? v[j] : v[j] * S.alpha;
          }
          if (Yf) {
            *reinterpret_cast<float4*>(Yf + m * S.coutr + n0) = float4{v[0], v[1], v[2], v[3]};
            continue;
          }
          h2 h01, l01, h23, l23;
          track(m4, v[0], v[1]);
          track(m4, v[2], v[3]);
          split2(v[0], v[1], h01, l01);
          split2(v[2], v[3], h23, l23);
          *reinterpret_cast<uint2*>(yh + n0) = uint2{h2_bits(h01), h2_bits(h23)};
          *reinterpret_cast<uint2*>(yl + n0) = uint2{h2_bits(l01), h2_bits(l23)};
        }
    }
    if (m4 >= kF16Max) *flag = 1;
  }
}

#ifndef HBK_X3_WAVES_PER_EU
#define HBK_X3_WAVES_PER_EU 2
#endif
template <int NBMAX, bool WG>
__global__ void __launch_bounds__(kXThreads) __attribute__((amdgpu_waves_per_eu(HBK_X3_WAVES_PER_EU)))
conv_chain_x3_kernel(XArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char xsmem[];
  unsigned char* Xb = xsmem + a.lds_x;
  unsigned char* Yb = xsmem + a.lds_y;
  _Float16* Wl = reinterpret_cast<_Float16*>(xsmem + a.lds_w);
  float* Bl = reinterpret_cast<float*>(xsmem + a.lds_b);
  int* kt = reinterpret_cast<int*>(xsmem + a.lds_k);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // per-block LDS copies of the stage descriptors and the im2col tap table
  // (read every task; kernel arguments are not re-read in the task loop)
  __shared__ int s_st[kMaxStages * kXStageInts];
  __shared__ int s_i2c[kI2cLds];
  for (int i = tid; i < a.n_stages * kXStageInts; i += kXThreads)
    s_st[i] = reinterpret_cast<const int*>(a.st)[i];
  for (int i = tid; i < kI2cLds; i += kXThreads) s_i2c[i] = a.i2c_off[min(i, a.i2c_n - 1)];
  if (!WG)
    for (int i = tid; i < a.w_halfs / 8; i += kXThreads)
      reinterpret_cast<h8*>(Wl)[i] = reinterpret_cast<const h8*>(a.wblob)[i];
  for (int i = tid; i < a.b_floats; i += kXThreads) Bl[i] = a.bblob[i];
  for (int i = tid; i < a.kt_n; i += kXThreads) kt[i] = a.ktab[i];

  // task indices fit in 32 bits (at most kChunkClips x 32 windows x bands)
  const int n_tasks = static_cast<int>((a.n_img + a.G - 1) / a.G) * a.n_bands;
  const int C = a.C_src;
  const XStage& S0 = a.st[0];
  // per-kernel thread mappings
  //  staging (no im2col): units of 8 channels, W_in * C / 8 per row
  //  staging (im2col):    raw f32, W_in * C per row
  //  im2col expansion:    positions, wo0 per row
  //  store:               units of 4 channels (vec_out) or 1, W_out * C_out / (4|1) per row
  const int st_units = a.im2col ? (a.raw_vec ? a.W_in * C / 4 : a.W_in * C) : a.W_in * (C / 8);
  const int raw_len = a.W_in * C;  // floats per raw row (im2col)
  const RowMap ms(st_units, tid);
  const int st_w = a.im2col ? 0 : ms.t_u / (C / 8);
  const int wo0 = a.W_in - S0.kw + 1;
  const RowMap mi(wo0, tid);
  const int cu = a.vec_out ? 4 : 1;
  const RowMap mo(a.W_out * a.C_out / cu, tid);
  const int o_w = mo.t_u / (a.C_out / cu), o_c = (mo.t_u - o_w * (a.C_out / cu)) * cu;

  struct Geo {
    int64_t img0;
    int G, orow0, orows, r0, rows_in, nrows;
  };
  auto geo = [&](int task) {
    Geo t;
    const int grp = task / a.n_bands;
    const int band = task - grp * a.n_bands;
    t.img0 = static_cast<int64_t>(grp) * a.G;
    t.G = static_cast<int>(min<int64_t>(a.G, a.n_img - t.img0));
    t.orow0 = band * a.band;
    t.orows = min(a.band, a.H_out - t.orow0);
    t.r0 = t.orow0 * a.out_ph;
    t.rows_in = t.orows * a.out_ph + a.shrink;
    t.nrows = t.G * t.rows_in;
    return t;
  };
  // one staging unit of row `row` (image g, band row r), max-pooled on load:
  // im2col: 4 raw floats (raw_vec) or 1; otherwise 8 channels of position w
  auto load_unit = [&](const Geo& t, int row, int u, float4& v0, float4& v1) {
    const int g = row / t.rows_in;
    const int r = row - g * t.rows_in;
    const int64_t im = t.img0 + g;
    const int64_t clip = im / a.ipc;
    const int roff = a.row_off[im - clip * a.ipc];
    const float* srow = a.in + clip * a.src_clip_stride +
                        static_cast<int64_t>(roff + (t.r0 + r) * a.in_ph) * a.src_row_stride;
    if (a.im2col) {
      if (a.raw_vec) {  // in_pw == 1
        const float* src = srow + u * 4;
        v0 = *reinterpret_cast<const float4*>(src);
        for (int i = 1; i < a.in_ph; ++i) {
          const float4 q = *reinterpret_cast<const float4*>(src + i * a.src_row_stride);
          v0 = float4{nan_max(v0.x, q.x), nan_max(v0.y, q.y), nan_max(v0.z, q.z), nan_max(v0.w, q.w)};
        }
      } else {
        const int w = u / C, c = u - w * C;
        const float* src = srow + (w * a.in_pw) * C + c;
        float v = src[0];
        for (int i = 0; i < a.in_ph; ++i)
          for (int j = 0; j < a.in_pw; ++j) v = nan_max(v, src[i * a.src_row_stride + j * C]);
        v0.x = v;
      }
      return;
    }
    const int w = (ms.u_step == st_units) ? st_w : u / (C / 8);
    const int c8 = (u - w * (C / 8)) * 8;
    const float* src = srow + (w * a.in_pw) * C + c8;
    if (a.in_ph <= 2 && a.in_pw <= 2) {
      // window of at most 2 x 2: all four taps are loaded unconditionally (a tap
      // outside the window re-reads tap (0, 0); the max is idempotent), so no
      // load sits in a predicated branch or a runtime loop that would wait on it
      const int di = a.in_ph > 1 ? a.src_row_stride : 0, dj = a.in_pw > 1 ? C : 0;
      const float4 p00 = *reinterpret_cast<const float4*>(src), q00 = *reinterpret_cast<const float4*>(src + 4);
      const float4 p01 = *reinterpret_cast<const float4*>(src + dj);
      const float4 q01 = *reinterpret_cast<const float4*>(src + dj + 4);
      const float4 p10 = *reinterpret_cast<const float4*>(src + di);
      const float4 q10 = *reinterpret_cast<const float4*>(src + di + 4);
      const float4 p11 = *reinterpret_cast<const float4*>(src + di + dj);
      const float4 q11 = *reinterpret_cast<const float4*>(src + di + dj + 4);
      auto mx = [](const float4& x, const float4& y) {
        return float4{nan_max(x.x, y.x), nan_max(x.y, y.y), nan_max(x.z, y.z), nan_max(x.w, y.w)};
      };
      v0 = mx(mx(p00, p01), mx(p10, p11));
      v1 = mx(mx(q00, q01), mx(q10, q11));
      return;
    }
    v0 = *reinterpret_cast<const float4*>(src);
    v1 = *reinterpret_cast<const float4*>(src + 4);
    for (int i = 0; i < a.in_ph; ++i)
      for (int j = 0; j < a.in_pw; ++j) {
        if (i == 0 && j == 0) continue;
        const float* q = src + i * a.src_row_stride + j * C;
        const float4 p0 = *reinterpret_cast<const float4*>(q);
        const float4 p1 = *reinterpret_cast<const float4*>(q + 4);
        v0 = float4{nan_max(v0.x, p0.x), nan_max(v0.y, p0.y), nan_max(v0.z, p0.z), nan_max(v0.w, p0.w)};
        v1 = float4{nan_max(v1.x, p1.x), nan_max(v1.y, p1.y), nan_max(v1.z, p1.z), nan_max(v1.w, p1.w)};
      }
  };
  auto store_unit = [&](const Geo& t, int row, int u, const float4& v0, const float4& v1) {
    if (a.im2col) {
      float* R = reinterpret_cast<float*>(Yb) + row * raw_len;
      if (a.raw_vec)
        *reinterpret_cast<float4*>(R + u * 4) = v0;
      else
        R[u] = v0.x;
      return;
    }
    const int w = (ms.u_step == st_units) ? st_w : u / (C / 8);
    const int c8 = (u - w * (C / 8)) * 8;
    h2 a0, b0, a1, b1, a2, b2, a3, b3;
    guard4(a.range_flag, v0.x, v0.y, v0.z, v0.w);
    guard4(a.range_flag, v1.x, v1.y, v1.z, v1.w);
    split2(v0.x, v0.y, a0, b0);
    split2(v0.z, v0.w, a1, b1);
    split2(v1.x, v1.y, a2, b2);
    split2(v1.z, v1.w, a3, b3);
    _Float16* Sh = reinterpret_cast<_Float16*>(Xb);
    const int idx = (row * a.W_in + w) * a.cs0 + c8;
    *reinterpret_cast<uint4*>(Sh + idx) = uint4{h2_bits(a0), h2_bits(a1), h2_bits(a2), h2_bits(a3)};
    *reinterpret_cast<uint4*>(Sh + t.nrows * a.W_in * a.cs0 + idx) =
        uint4{h2_bits(b0), h2_bits(b1), h2_bits(b2), h2_bits(b3)};
  };
  // The first kPF row passes of a task's staging are loaded into registers
  // one task ahead (their global loads overlap the current task's compute);
  // further passes, or rows wider than the block, load synchronously.
#ifndef HBK_X3_PF
#define HBK_X3_PF (NBMAX == 1 ? 4 : 2)
#endif
  constexpr int kPF = HBK_X3_PF;
  const bool pf_ok = ms.u_step == st_units;
  float4 pv0[kPF], pv1[kPF];
  auto prefetch = [&](const Geo& t) {
#pragma unroll
    for (int p = 0; p < kPF; ++p) {
      // clamped, not predicated: rows past the task re-read its last row (unused)
      const int row = min(ms.t_row + p * ms.rpp, t.nrows - 1);
      load_unit(t, row, ms.t_u, pv0[p], pv1[p]);
    }
  };

  int task = blockIdx.x;
  Geo tg{};
  if (task < n_tasks) {
    tg = geo(task);
    if (pf_ok) prefetch(tg);
  }
  for (; task < n_tasks; task += gridDim.x) {
    const Geo t = tg;
    const int64_t img0 = t.img0;
    const int G = t.G, orow0 = t.orow0, orows = t.orows, rows_in = t.rows_in;

    // 1) stage the band's input rows (max-pooled on the fly)
    __syncthreads();  // previous task's readers of X / Y are done (kt, Wl, Bl on the first task)
#ifdef HBK_PHASE_TIMING
    unsigned long long phase_t0 = __builtin_amdgcn_s_memtime();
#endif
    if (HBK_SKIP(3)) {
    } else if (pf_ok) {
#pragma unroll
      for (int p = 0; p < kPF; ++p) {
        const int row = ms.t_row + p * ms.rpp;
        if (row < t.nrows) store_unit(t, row, ms.t_u, pv0[p], pv1[p]);
      }
      for (int row = ms.t_row + kPF * ms.rpp; row < t.nrows; row += ms.rpp) {
        float4 v0, v1;
        load_unit(t, row, ms.t_u, v0, v1);
        store_unit(t, row, ms.t_u, v0, v1);
      }
    } else {
      for (int row = ms.t_row; row < t.nrows; row += ms.rpp)
        for (int u = ms.t_u; u < st_units; u += ms.u_step) {
          float4 v0, v1;
          load_unit(t, row, u, v0, v1);
          store_unit(t, row, u, v0, v1);
        }
    }
    if (task + static_cast<int>(gridDim.x) < n_tasks) {
      tg = geo(task + gridDim.x);
      if (pf_ok && !HBK_SKIP(3)) prefetch(tg);  // in flight during this task's compute
    }
    int hin = rows_in, win = a.W_in;
    if (a.im2col && !HBK_SKIP(1)) {
      // expand stage 0's taps: position (g, y, x) of its OUTPUT holds k = (dh kw + dw) C + ci
      __syncthreads();
      HBK_PHASE(0);
      const int ho = hin - S0.kh + 1;
      const int K0 = S0.kh * S0.kw * C, K8 = (K0 + 7) & ~7;
      const float* R = reinterpret_cast<const float*>(Yb);
      _Float16* Ih = reinterpret_cast<_Float16*>(Xb);
      _Float16* Il = Ih + G * ho * wo0 * a.cs0;
      for (int prow = mi.t_row; prow < G * ho; prow += mi.rpp)
      for (int x = mi.t_u; x < wo0; x += mi.u_step) {
        const int g = prow / ho, y = prow - g * ho;
        const float* base = R + ((g * rows_in + y) * win + x) * C;
        _Float16* dh_ = Ih + (prow * wo0 + x) * a.cs0;
        _Float16* dl_ = Il + (prow * wo0 + x) * a.cs0;
        for (int k8 = 0; k8 < K8; k8 += 8) {  // one 8-channel group: 16 B per plane
          uint32_t hb[4], lb[4];
          float m = 0.f;
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int k = k8 + 2 * p;  // tap offsets: uniform table (scalar loads)
            const int o0 = k < kI2cLds ? s_i2c[k] : a.i2c_off[k];
            const int o1 = k + 1 < kI2cLds ? s_i2c[k + 1] : a.i2c_off[k + 1];
            const float v0 = k < K0 ? base[o0] : 0.f;
            const float v1 = k + 1 < K0 ? base[o1] : 0.f;
            h2 hh, ll;
            track(m, v0, v1);
            split2(v0, v1, hh, ll);
            hb[p] = h2_bits(hh);
            lb[p] = h2_bits(ll);
          }
          if (m >= kF16Max) *a.range_flag = 1;
          *reinterpret_cast<uint4*>(dh_ + k8) = uint4{hb[0], hb[1], hb[2], hb[3]};
          *reinterpret_cast<uint4*>(dl_ + k8) = uint4{lb[0], lb[1], lb[2], lb[3]};
        }
      }
    }

    // 2) the chain's convs, ping-ponging between X and Y
    unsigned char* cur = Xb;
    unsigned char* nxt = Yb;
    for (int s = 0; s < a.n_stages; ++s) {
      const XStage S = lds_stage(s_st + s * kXStageInts);
      const int ho = hin - S.kh + 1, wo = win - S.kw + 1;
      const bool i2c = a.im2col && s == 0;
      const int hA = i2c ? ho : hin, wA = i2c ? wo : win;
      const int M = G * ho * wo;
      __syncthreads();  // stage input complete
      HBK_PHASE(s == 0 ? 1 : 1 + s);
      const _Float16* Xh = reinterpret_cast<const _Float16*>(cur);
      const _Float16* Xl = Xh + G * hA * wA * S.cs_in;
      _Float16* Yh = reinterpret_cast<_Float16*>(nxt);
      _Float16* Yl = Yh + M * S.cs_out;
      const _Float16* Wst = WG ? a.wblob + S.w_off : Wl + S.w_off;
      const int* kts = kt + S.kt_off;
      const float* bs = Bl + S.b_off;
      float* Yf = s + 1 == a.n_stages ? reinterpret_cast<float*>(nxt) : nullptr;
      // RB x NB tiles of one 16-register accumulator each. NBMAX 4 (plans with
      // a stage wider than 96 channels): groups of 3 blocks, each re-reading
      // the stage input (a separate instantiation: the loop costs the others
      // spills)
      if (HBK_SKIP(0)) {
      } else if constexpr (NBMAX > 3) {
        for (int cb = 0; cb < S.nblk; cb += 3) {
          const int nb = min(3, S.nblk - cb);
          if (nb == 3)
            xstage<3, 1>(Xh, Xl, Yh, Yl, Yf, Wst, kts, bs, M, hA, wA, ho, wo, S, lane, wave, a.range_flag, cb);
          else if (nb == 2)
            xstage<2, 2>(Xh, Xl, Yh, Yl, Yf, Wst, kts, bs, M, hA, wA, ho, wo, S, lane, wave, a.range_flag, cb);
          else
            xstage<1, 2>(Xh, Xl, Yh, Yl, Yf, Wst, kts, bs, M, hA, wA, ho, wo, S, lane, wave, a.range_flag, cb);
        }
      } else if (NBMAX >= 3 && S.nblk == 3) {
        xstage<3, 1>(Xh, Xl, Yh, Yl, Yf, Wst, kts, bs, M, hA, wA, ho, wo, S, lane, wave, a.range_flag, 0);
      } else if (NBMAX >= 2 && S.nblk == 2) {
        xstage<2, 2>(Xh, Xl, Yh, Yl, Yf, Wst, kts, bs, M, hA, wA, ho, wo, S, lane, wave, a.range_flag, 0);
      } else {
        xstage<1, 2>(Xh, Xl, Yh, Yl, Yf, Wst, kts, bs, M, hA, wA, ho, wo, S, lane, wave, a.range_flag, 0);
      }
      unsigned char* t = cur;
      cur = nxt;
      nxt = t;
      hin = ho;
      win = wo;
    }
    __syncthreads();
    HBK_PHASE(1 + a.n_stages);

    // 3) store the band (max-pooled on the fly) from the last stage's f32 output
    const int cso = __builtin_amdgcn_readfirstlane(s_st[(a.n_stages - 1) * kXStageInts + 4]);  // coutr
    const float* O = reinterpret_cast<const float*>(cur);
    const int units = a.W_out * a.C_out / cu;
    for (int orow = HBK_SKIP(2) ? (1 << 30) : mo.t_row; orow < G * orows; orow += mo.rpp) {
      const int g = orow / orows, r = orow - g * orows;
      float* drow = a.out + (img0 + g) * a.out_img_stride + static_cast<int64_t>(orow0 + r) * a.W_out * a.C_out;
      for (int u = mo.t_u; u < units; u += mo.u_step) {
        const int w = (mo.u_step == units) ? o_w : u / (a.C_out / cu);
        const int c = (mo.u_step == units) ? o_c : (u - w * (a.C_out / cu)) * cu;
        const int base = ((g * hin + r * a.out_ph) * win + w * a.out_pw) * cso + c;
        if (a.vec_out) {
          float4 v = *reinterpret_cast<const float4*>(O + base);
          for (int i = 0; i < a.out_ph; ++i)
            for (int j = 0; j < a.out_pw; ++j) {
              if (i == 0 && j == 0) continue;
              const float4 t = *reinterpret_cast<const float4*>(O + base + (i * win + j) * cso);
              v = float4{nan_max(v.x, t.x), nan_max(v.y, t.y), nan_max(v.z, t.z), nan_max(v.w, t.w)};
            }
          *reinterpret_cast<float4*>(drow + w * a.C_out + c) = v;
        } else {
          float v = O[base];
          for (int i = 0; i < a.out_ph; ++i)
            for (int j = 0; j < a.out_pw; ++j) v = nan_max(v, O[base + (i * win + j) * cso]);
          drow[w * a.C_out + c] = v;
        }
      }
    }
    HBK_PHASE(2 + a.n_stages);
  }
}

}  // namespace

// n = NBMAX, f = weights read from global memory (WG)
const void* embed_x3_kernel(int n, bool f) {
  switch (n) {
    case 1: return f ? addr(conv_chain_x3_kernel<1, true>) : addr(conv_chain_x3_kernel<1, false>);
    case 2: return f ? addr(conv_chain_x3_kernel<2, true>) : addr(conv_chain_x3_kernel<2, false>);
    case 3: return f ? addr(conv_chain_x3_kernel<3, true>) : addr(conv_chain_x3_kernel<3, false>);
    default: return f ? addr(conv_chain_x3_kernel<4, true>) : addr(conv_chain_x3_kernel<4, false>);  // > 3 blocks: groups of 3
  }
}

}  // namespace hbk

#ifdef HBK_PHASE_TIMING
extern "C" int hbk_debug_phase_cycles(unsigned long long* out, int n) {
  unsigned long long h[64];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(hbk::g_phase_cycles), sizeof(h)) != hipSuccess) return -2;
  for (int i = 0; i < n && i < 64; ++i) out[i] = h[i];
  unsigned long long z[64] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(hbk::g_phase_cycles), z, sizeof(z));
  return 0;
}
#endif
