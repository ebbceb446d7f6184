// Speech-embedding conv stack for gfx950: fused conv chains on MFMA (f32).
//
// Replaces the speech-embedding ONNX graph run by SpeechEmbeddingModel.__call__
// (embeddings.py:32-42) over the 76-frame windows that
// SpeechEmbeddings.spectrograms_to_embeddings cuts (embeddings.py:86-151).
//
// Execution model
//   * The graph (Keras Conv2D 'valid' stride 1 + LeakyReLU, MaxPool2D) is cut
//     into CHAINS: [optional input pool] conv ... conv [optional output pool].
//     One launch runs a whole chain; its activations live in LDS.
//   * A task = G images x one band of output rows. The band's input rows are
//     staged into LDS once (NHWC, channels padded to an odd count so that the
//     16 rows of an MFMA A-fragment hit 16 different banks), then every conv
//     runs as an implicit GEMM  out[m, n] = sum_k A[m, k] W[k, n]  with
//     m = (image, y, x), k = (dh, dw, ci) gathered from LDS through a per-stage
//     offset table, on v_mfma_f32_16x16x4f32 (exact f32, fmaf-chain numerics).
//   * Clip path: layers before the first pool that breaks the alignment of the
//     window starts run ONCE per clip over the whole 136-frame sequence
//     ("prefix"); windows are then cut from the prefix output (row offsets) for
//     the per-window "tail". The per-window API runs every layer per window.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "hbk_common.h"
#include "hbk_embed_args.h"  // kernel-argument structs and geometry constants
#include "hbk_embed_plan.h"  // the host planner (no device call)

namespace hbk {
namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kChunkClips = 16384;     // clips per workspace chunk (default; HBK_EMBED_CHUNK overrides)
// clips per workspace chunk (HBK_EMBED_CHUNK: 256 .. 32,768): every chain kernel runs once per chunk (its last round of waves
// partly filled); measured: 100 k clips in 16,384-clip chunks 24.30 ms, in 32,768-clip chunks
// 24.43 ms, bit-identical (tools/embed_chunk_check.py), so the smaller workspace stays
inline int64_t chunk_clips() {
  static const int64_t c = [] {
    const char* e = getenv("HBK_EMBED_CHUNK");
    const long long v = e ? atoll(e) : 0;
    // (capped at 32,768, the size tools/embed_chunk_check.py validated: the chain kernels'
    // task counts are 32-bit and assume at most that many clips x windows x bands)
    return v >= 256 && v <= 32768 ? int64_t(v) : int64_t(kChunkClips);
  }();
  return c;
}

typedef float f4 __attribute__((ext_vector_type(4)));

template <int NB, int RB, bool WG>
__device__ __forceinline__ void conv_stage(const float* __restrict__ X, float* __restrict__ Y,
                                           const float* __restrict__ Wst,
                                           const int* __restrict__ ktab,
                                           const float* __restrict__ bias, int G, int hin, int win,
                                           const StageDesc& S, int wstride, int lane, int wave) {
  const int ho = hin - S.kh + 1, wo = win - S.kw + 1;
  const int img_pos = ho * wo, M = G * img_pos;
  const int nrb = (M + 15) >> 4;
  const int r16 = lane & 15, kq = lane >> 4;
  // output channels in groups of NB 16-column blocks (more than NB * 16 channels: several passes)
  const int nblk = (S.cout + 15) >> 4;
  for (int cb = 0; cb < nblk; cb += NB)
  for (int rb0 = wave * RB; rb0 < nrb; rb0 += kWaves * RB) {
    int moff[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      int m = min((rb0 + r) * 16 + r16, M - 1);
      const int g = m / img_pos;
      const int rem = m - g * img_pos;
      const int y = rem / wo;
      const int x = rem - y * wo;
      moff[r] = ((g * hin + y) * win + x) * S.cinp;
    }
    f4 acc[RB][NB];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int c = 0; c < NB; ++c) acc[r][c] = f4{0.f, 0.f, 0.f, 0.f};
    const float* wp = Wst + kq * wstride + cb * 16 + r16;
#pragma unroll 2
    for (int ks = 0; ks < S.ksteps; ++ks) {
      const int koff = ktab[ks * 4 + kq];
      float av[RB], bv[NB];
#pragma unroll
      for (int r = 0; r < RB; ++r) av[r] = X[moff[r] + koff];
#pragma unroll
      for (int c = 0; c < NB; ++c) bv[c] = wp[ks * 4 * wstride + min(c, nblk - 1 - cb) * 16];
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int c = 0; c < NB; ++c)
          acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv[c], acc[r][c], 0, 0, 0);
    }
    // C/D layout: row (lane >> 4) * 4 + i, column lane & 15
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      const int n = (cb + c) * 16 + r16;
      if (n >= S.cout) continue;
      const float bb = bias[n];
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = (rb0 + r) * 16 + kq * 4 + i;
          if (m < M) {
            float v = acc[r][c][i] + bb;
            if (S.act) v = v >= 0.f ? v : v * S.alpha;
            Y[m * S.coutp + n] = v;
          }
        }
    }
  }
  (void)WG;
}

template <int NB, int RB, bool WG>
__global__ void __launch_bounds__(kThreads) conv_chain_kernel(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* X = smem + a.lds_x;
  float* Y = smem + a.lds_y;
  float* Wl = smem + a.lds_w;
  int* ktab = reinterpret_cast<int*>(smem + a.lds_k);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!WG)
    for (int i = tid; i < a.wblob_floats; i += kThreads) Wl[i] = a.wblob[i];  // resident weights

  const int64_t n_groups = (a.n_img + a.G - 1) / a.G;
  const int64_t n_tasks = n_groups * a.n_bands;
  const int C = a.C_src;
  const int cinp0 = a.st[0].cinp;
  for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
    const int64_t grp = task / a.n_bands;
    const int band = static_cast<int>(task - grp * a.n_bands);
    const int64_t img0 = grp * a.G;
    const int G = static_cast<int>(min<int64_t>(a.G, a.n_img - img0));
    const int orow0 = band * a.band;
    const int orows = min(a.band, a.H_out - orow0);
    const int r0 = orow0 * a.out_ph;           // first chain-input row of the band
    const int rows_in = orows * a.out_ph + a.shrink;

    // 1) stage the band's input rows (max-pooled on the fly) into X
    const int row_elems = a.W_in * C;
    const int per_img = rows_in * row_elems;
    for (int e = tid; e < G * per_img; e += kThreads) {
      const int g = e / per_img;
      int rem = e - g * per_img;
      const int r = rem / row_elems;
      rem -= r * row_elems;
      const int w = rem / C;
      const int c = rem - w * C;
      const int64_t im = img0 + g;
      const int64_t clip = im / a.ipc;
      const int roff = a.row_off[im - clip * a.ipc];
      const float* src = a.in + clip * a.src_clip_stride +
                         static_cast<int64_t>(roff + (r0 + r) * a.in_ph) * a.src_row_stride +
                         (w * a.in_pw) * C + c;
      float v = src[0];
      for (int i = 0; i < a.in_ph; ++i)
        for (int j = 0; j < a.in_pw; ++j) v = nan_max(v, src[i * a.src_row_stride + j * C]);
      X[((g * rows_in + r) * a.W_in + w) * cinp0 + c] = v;
    }

    // 2) the chain's convs, ping-ponging between X and Y
    int hin = rows_in, win = a.W_in;
    float* cur = X;
    float* nxt = Y;
    for (int s = 0; s < a.n_stages; ++s) {
      const StageDesc S = a.st[s];
      __syncthreads();  // stage input complete; previous stage done with ktab
      for (int k = tid; k < S.ksteps * 4; k += kThreads) {
        int v = 0;  // padded k: weight 0, read the (finite) own-position value
        if (k < S.K) {
          const int tap = k / S.cin;
          const int ci = k - tap * S.cin;
          const int dh = tap / S.kw;
          const int dw = tap - dh * S.kw;
          v = (dh * win + dw) * S.cinp + ci;
        }
        ktab[k] = v;
      }
      __syncthreads();
      const float* Wst = WG ? a.wblob + S.w_off : Wl + S.w_off;
      conv_stage<NB, RB, WG>(cur, nxt, Wst, ktab, a.wblob + S.b_off, G, hin, win, S, a.wstride,
                             lane, wave);
      float* t = cur;
      cur = nxt;
      nxt = t;
      hin -= S.kh - 1;
      win -= S.kw - 1;
    }
    __syncthreads();

    // 3) store the band (max-pooled on the fly)
    const int coutp = a.st[a.n_stages - 1].coutp;
    const int orow_elems = a.W_out * a.C_out;
    const int per_out = orows * orow_elems;
    for (int e = tid; e < G * per_out; e += kThreads) {
      const int g = e / per_out;
      int rem = e - g * per_out;
      const int r = rem / orow_elems;
      rem -= r * orow_elems;
      const int w = rem / a.C_out;
      const int c = rem - w * a.C_out;
      const float* p = cur + ((g * hin + r * a.out_ph) * win + w * a.out_pw) * coutp + c;
      float v = p[0];
      for (int i = 0; i < a.out_ph; ++i)
        for (int j = 0; j < a.out_pw; ++j) v = nan_max(v, p[(i * win + j) * coutp]);
      a.out[(img0 + g) * a.out_img_stride + static_cast<int64_t>(orow0 + r) * orow_elems + w * a.C_out + c] = v;
    }
    __syncthreads();  // the next task restages X
  }
}

// ------------------------------------------------- split-f16 conv chain ----
// Same task structure as conv_chain_kernel; the arithmetic is an fp16 pair per
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

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __fp16 h2 __attribute__((ext_vector_type(2)));
typedef float f16x __attribute__((ext_vector_type(16)));

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

#ifdef HBK_TRACE
// Tracing build only: lane 0 of waves of the first 4 blocks records
// s_memtime at marks of the first tasks into g_trace[block][wave][event].
__device__ unsigned long long g_trace[4][4][256];
__device__ int g_trace_n[4][4];
#define HBK_MARK(id)                                                                        \
  do {                                                                                      \
    if (blockIdx.x < 4 && (threadIdx.x & 63) == 0) {                                        \
      const int w_ = threadIdx.x >> 6, b_ = blockIdx.x;                                     \
      const int n_ = g_trace_n[b_][w_];                                                     \
      if (n_ < 255) {                                                                       \
        g_trace[b_][w_][n_] = (__builtin_amdgcn_s_memtime() << 8) | static_cast<unsigned>(id); \
        g_trace_n[b_][w_] = n_ + 1;                                                         \
      }                                                                                     \
    }                                                                                       \
  } while (0)
#else
#define HBK_MARK(id) \
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

// hi = v rounded toward zero to fp16 (11 significant bits in fp16's normal
// range), lo = (v - hi) rounded to fp16 by v_fma_mix{lo,hi}_f16 (v - hi is
// exact in f32); two values, packed: 3 VALU instructions per pair
// (kF16Max and the range flag: hbk_embed_args.h)
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
__device__ __forceinline__ void split2(float a, float b, h2& hi, h2& lo) {
  hi = __builtin_amdgcn_cvt_pkrtz(a, b);
  const uint32_t hb = __builtin_bit_cast(uint32_t, hi);
  uint32_t l;  // mixlo writes bits 15:0, mixhi bits 31:16: no initial value needed
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(a), "v"(hb));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(b), "v"(hb));
  lo = __builtin_bit_cast(h2, l);
}

// max(v, alpha v) through asm: fmaxf on MFMA results gets a canonicalising
// v_max in front of it; both operands are NaN for a NaN v, so NaN propagates
__device__ __forceinline__ float leaky_max(float v, float alpha) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(v * alpha));
  return r;
}

__device__ __forceinline__ uint32_t h2_bits(h2 v) { return __builtin_bit_cast(uint32_t, v); }

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
    HBK_MARK(10);
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
    // MFMAs never chain on one accumulator
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
    HBK_MARK(11);
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
#ifdef HBK_TRACE
    // make the mark wait for the accumulators (MFMA completion)
    asm volatile("" ::"v"(acc[0][0][0]));
#endif
    HBK_MARK(12);
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
            for (int j = 0; j < 4; ++j) v[j] = leaky_max(v[j], S.alpha);
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
    HBK_MARK(13);
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
    HBK_MARK(1);
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
      HBK_MARK(19);
      __syncthreads();  // stage input complete
      HBK_PHASE(s == 0 ? 1 : 1 + s);
      HBK_MARK(20 + s);
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
    HBK_MARK(19);
    __syncthreads();
    HBK_PHASE(1 + a.n_stages);
    HBK_MARK(5);

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
    HBK_MARK(6);
  }
}

// ------------------------------------------------------------------- p0 ----
// Pattern kernel for the chain  conv 3x3 (1 -> C) . conv 1x3 (C -> C) .
// conv 3x1 (C -> C) . max-pool 2x2  on a fixed input width WI (the SE20
// prefix's first group: 136 x 32 mel rows -> 66 x 14 x 24, ~55 % of the
// embedding MACs). Same split-f16 numerics as conv_chain_x3_kernel (3 fp16
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

// hi = v rounded toward zero to fp16, lo = (v - hi) rounded to fp16; two values, packed
__device__ __forceinline__ void split2_mix(float a, float b, uint32_t& hi, uint32_t& lo, float& amax) {
  track(amax, a, b);
  hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b));
  uint32_t l;  // mixlo writes bits 15:0, mixhi bits 31:16: no initial value needed
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(a), "v"(hi));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(b), "v"(hi));
  lo = l;
}

// LEAKY: every conv of the chain is LeakyReLU with 0 <= alpha <= 1 (max(v, alpha v)); else identity
// (v_max_f32 through asm: fmaxf on MFMA results gets a canonicalising v_max in
// front of it; both operands are NaN for a NaN input, so NaN propagates)
template <bool LEAKY>
__device__ __forceinline__ float p0_act(float v, float alpha) {
  if (!LEAKY) return v;
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(v * alpha));
  return r;
}

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
    for (int jj = 0; jj < 4; ++jj) v[jj] = p0_act<LEAKY>(acc[4 * q + jj], alpha);
    uint32_t h01, l01, h23, l23;
    split2_mix(v[0], v[1], h01, l01, amax);
    split2_mix(v[2], v[3], h23, l23, amax);
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
        v.x = p0_act<LEAKY>(acc[4 * q], alpha);
        v.y = p0_act<LEAKY>(acc[4 * q + 1], alpha);
        v.z = p0_act<LEAKY>(acc[4 * q + 2], alpha);
        v.w = p0_act<LEAKY>(acc[4 * q + 3], alpha);
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
    for (int ks = 0; ks < G::KS; ++ks) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.ah[ks], xh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.ah[ks], xl[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.al[ks], xh[ks], acc, 0, 0, 0);
    }
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
    HBK_MARK(1);
    __syncthreads();  // the previous task's readers are done
    // 1) input rows [row0, row0 + RI) (clamped to the image) -> raw; prefetch the next task's
#pragma unroll
    for (int u = 0; u < kRawPer; ++u) {
      const int i = tid + u * kP0Threads;
      if (i < kRawV) *reinterpret_cast<float4*>(raw + 4 * i) = rawv[u];
    }
    if (task + static_cast<int>(gridDim.x) < n_tasks) load_raw(task + gridDim.x);
    __syncthreads();
    HBK_MARK(40);
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
        for (int i = 0; i < 4; ++i) split2_mix(v[2 * i], v[2 * i + 1], hb[i], lb[i], amax);
        const h8 xh = __builtin_bit_cast(h8, uint4{hb[0], hb[1], hb[2], hb[3]});
        const h8 xl = __builtin_bit_cast(h8, uint4{lb[0], lb[1], lb[2], lb[3]});
        f16x acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, xh, b0, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, xl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0l, xh, acc, 0, 0, 0);
        if (pp < G::M0) p0_store_planes<C, G::CS, LEAKY>(acc, p, khalf, s0h, s0l, a.alpha, amax);
      }
    }
    HBK_MARK(50);
    __syncthreads();
    HBK_MARK(41);
    p0_stage12<WI, C, BAND, 1, LEAKY>(a, W1, s0h, s0l, s1h, s1l, nullptr, wave, r32, khalf, amax);
    HBK_MARK(51);
    __syncthreads();
    HBK_MARK(42);
    p0_stage12<WI, C, BAND, 2, LEAKY>(a, W2, s1h, s1l, nullptr, nullptr, s2, wave, r32, khalf, amax);
    HBK_MARK(52);
    __syncthreads();
    HBK_MARK(43);
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
    HBK_MARK(6);
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
        v.x = p0_act<LEAKY>(acc[4 * q], alpha);
        v.y = p0_act<LEAKY>(acc[4 * q + 1], alpha);
        v.z = p0_act<LEAKY>(acc[4 * q + 2], alpha);
        v.w = p0_act<LEAKY>(acc[4 * q + 3], alpha);
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
    for (int ks = 0; ks < KS; ++ks) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.ah[ks], xh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.ah[ks], xl[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(W.al[ks], xh[ks], acc, 0, 0, 0);
    }
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
        split2_mix(v0.x, v0.y, h[0], l[0], amax);
        split2_mix(v0.z, v0.w, h[1], l[1], amax);
        split2_mix(v1.x, v1.y, h[2], l[2], amax);
        split2_mix(v1.z, v1.w, h[3], l[3], amax);
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

typedef float f2v __attribute__((ext_vector_type(2)));

// LeakyReLU of two values: one packed multiply, two maxes (NaN stays NaN)
template <bool LEAKY>
__device__ __forceinline__ void p0s_act2(float& a, float& b, float alpha) {
  if (!LEAKY) return;
  const f2v m = f2v{a, b} * alpha;
  asm("v_max_f32 %0, %0, %1" : "+v"(a) : "v"(m.x));
  asm("v_max_f32 %0, %0, %1" : "+v"(b) : "v"(m.y));
}

// activation, split and LDS store of one finished stage-0 / stage-1 tile
template <bool LEAKY>
__device__ __forceinline__ void p0s_store(const f16x& acc, _Float16* oh, int x, int khalf, float alpha, bool track_it,
                                          float& amax, int plane) {
  float m = 0.f;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    float v[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    p0s_act2<LEAKY>(v[0], v[1], alpha);
    p0s_act2<LEAKY>(v[2], v[3], alpha);
    uint32_t h01, l01, h23, l23;
    split2_mix(v[0], v[1], h01, l01, m);
    split2_mix(v[2], v[3], h23, l23, m);
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
  split2_mix(c.r[0][0], c.r[0][1], hb[0], lb[0], m0);
  split2_mix(c.r[0][2], c.r[1][0], hb[1], lb[1], m0);
  split2_mix(c.r[1][1], c.r[1][2], hb[2], lb[2], m0);
  const h8 xh = __builtin_bit_cast(h8, uint4{hb[0], hb[1], hb[2], 0x3C00u});  // slot 6 = 1.0 (f16)
  const h8 xl = __builtin_bit_cast(h8, uint4{lb[0], lb[1], lb[2], 0u});
  const f16x zero = {};
  f16x acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.a0h, xh, zero, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.a0h, xl, acc0, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.a0l, xh, acc0, 0, 0, 0);
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
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.w1.h[ks], cur[0], acc1, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.w1.h[ks], cur[1], acc1, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.w1.l[ks], cur[0], acc1, 0, 0, 0);
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
    a2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.w2.h[ks], cur[0], a2, 0, 0, 0);
    a2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.w2.h[ks], cur[1], a2, 0, 0, 0);
    a2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(c.w2.l[ks], cur[0], a2, 0, 0, 0);
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
    for (int i = 0; i < 12; i += 2) p0s_act2<LEAKY>(pv[i], pv[i + 1], c.alpha);
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

// activation, split and LDS store of a finished stage row (channels 16 mb + 4 kq + j at position x)
template <bool LEAKY>
__device__ __forceinline__ void p1s_store(const f4 (&acc)[2], _Float16* oh, int plane, int x, int kq, float alpha,
                                          bool track_it, float& amax) {
  float m = 0.f;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    float v[4] = {acc[mb][0], acc[mb][1], acc[mb][2], acc[mb][3]};
    p0s_act2<LEAKY>(v[0], v[1], alpha);
    p0s_act2<LEAKY>(v[2], v[3], alpha);
    uint32_t h01, l01, h23, l23;
    split2_mix(v[0], v[1], h01, l01, m);
    split2_mix(v[2], v[3], h23, l23, m);
    const int o = x * kP1sCS + 16 * mb + 4 * kq;
    *reinterpret_cast<uint2*>(oh + o) = uint2{h01, h23};
    *reinterpret_cast<uint2*>(oh + plane + o) = uint2{l01, l23};
  }
  asm("v_max_f32 %0, %0, %1" : "+v"(amax) : "v"(track_it ? m : 0.f));
}

// the input row in registers (two float4 per lane: entries lane, lane + 64 of 84) -> hi / lo planes
__device__ __forceinline__ void p1s_stage_row(const float4 (&v)[2], _Float16* in_w, int lane, float& amx) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = lane + 64 * u;
    if (u == 0 || lane < kP1sWi * 6 - 64) {
      uint32_t h01, l01, h23, l23;
      split2_mix(v[u].x, v[u].y, h01, l01, amx);
      split2_mix(v[u].z, v[u].w, h23, l23, amx);
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
  p1s_store<LEAKY>(acca, A + (PAR & 3) * 2 * kP1sPlane, kP1sPlane, x, kq, c.alpha, y < kP1sHin && x < 12, c.amax);
  p1s_store<LEAKY>(accb, sm + kP1sB + ((PAR + 1) & 1) * 2 * kP1sBPlane, kP1sBPlane, x, kq, c.alpha,
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
  p1s_store<LEAKY>(accc, C + (PAR & 3) * 2 * kP1sPlane, kP1sPlane, x, kq, c.alpha,
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
      p0s_act2<LEAKY>(pv[mb][0], pv[mb][1], c.alpha);
      p0s_act2<LEAKY>(pv[mb][2], pv[mb][3], c.alpha);
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

template <int KS>
__device__ __forceinline__ void p2s_mma(f4 (&acc)[3], const P2sW<KS>& w, int ks, const h8& bh, const h8& bl) {
#pragma unroll
  for (int mb = 0; mb < 3; ++mb) {
    acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[mb][ks], bh, acc[mb], 0, 0, 0);
    acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[mb][ks], bl, acc[mb], 0, 0, 0);
    acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.l[mb][ks], bh, acc[mb], 0, 0, 0);
  }
}

// activation, split and LDS store of a finished tile (channels 16 mb + 4 kq + j at position p)
template <bool LEAKY>
__device__ __forceinline__ void p2s_store(const f4 (&acc)[3], _Float16* oh, int plane, int p, int kq, float alpha,
                                          bool track_it, float& amax) {
  float m = 0.f;
#pragma unroll
  for (int mb = 0; mb < 3; ++mb) {
    float v[4] = {acc[mb][0], acc[mb][1], acc[mb][2], acc[mb][3]};
    p0s_act2<LEAKY>(v[0], v[1], alpha);
    p0s_act2<LEAKY>(v[2], v[3], alpha);
    uint32_t h01, l01, h23, l23;
    split2_mix(v[0], v[1], h01, l01, m);
    split2_mix(v[2], v[3], h23, l23, m);
    const int o = p * kP2sCS + 16 * mb + 4 * kq;
    *reinterpret_cast<uint2*>(oh + o) = uint2{h01, h23};
    *reinterpret_cast<uint2*>(oh + plane + o) = uint2{l01, l23};
  }
  asm("v_max_f32 %0, %0, %1" : "+v"(amax) : "v"(track_it ? m : 0.f));
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
      split2_mix(r.v[u].x, r.v[u].y, h01, l01, amax);
      split2_mix(r.v[u].z, r.v[u].w, h23, l23, amax);
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
        p2s_store<LEAKY>(acc, sm + kP2sA + (y & 3) * 2 * kP2sAPlane, kP2sAPlane, p, kq, alpha, y < kP2sHin, amax);
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
        p2s_store<LEAKY>(acc, sm + kP2sB + ((y + 1) & 1) * 2 * kP2sAPlane, kP2sAPlane, p, kq, alpha,
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
          p2s_store<LEAKY>(acc, sm + kP2sC + (y & 3) * 2 * kP2sCPlane, kP2sCPlane, pl, kq, alpha,
                           y >= 4 && y - 4 < kP2sHin - 2, amax);
        } else if (y >= 7 && y - 7 < kP2sHout && img0 + pl < a.n_img) {
          float* o = a.out + (img0 + pl) * (kP2sHout * kP2sCo) + (y - 7) * kP2sCo + 4 * kq;
#pragma unroll
          for (int mb = 0; mb < 3; ++mb) {
            float v[4] = {acc[mb][0], acc[mb][1], acc[mb][2], acc[mb][3]};
            p0s_act2<LEAKY>(v[0], v[1], alpha);
            p0s_act2<LEAKY>(v[2], v[3], alpha);
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
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ks], bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ks], bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[ks], bh, acc, 0, 0, 0);
  }
  return acc;
}

// activation, split and ring store of one block's tile (channels 16 mb + 4 kq + j of position pos)
template <bool ACT, int CS, int PL>
__device__ __forceinline__ void t3_store(f4 acc, _Float16* oh, int pos, int mb, int kq, float alpha, float& amax) {
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
  p0s_act2<ACT>(v[0], v[1], alpha);
  p0s_act2<ACT>(v[2], v[3], alpha);
  uint32_t h01, l01, h23, l23;
  split2_mix(v[0], v[1], h01, l01, amax);
  split2_mix(v[2], v[3], h23, l23, amax);
  const int o = pos * CS + 16 * mb + 4 * kq;
  *reinterpret_cast<uint2*>(oh + o) = uint2{h01, h23};
  *reinterpret_cast<uint2*>(oh + PL + o) = uint2{l01, l23};
}

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
    split2_mix(v.x, v.y, h01, l01, amax);
    split2_mix(v.z, v.w, h23, l23, amax);
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
          t3_store<LEAKY, kT3CS1, kT3Pl1>(acc, sm + kT3A1 + (r & 1) * 2 * kT3Pl1, pos, mb, kq, alpha, amax);
        }
        if (y >= 4 && y < 4 + 11) {  // stage 2 (1x1)
          const int r = y - 4;
          const int ro[3] = {kT3A1 + (r & 1) * 2 * kT3Pl1, 0, 0};
          const f4 acc = t3_block<2, kT3C1, kT3CS1, kT3Pl1>(w2h, w2l, t3_bias(sb + kT3C1 + bo), sm, ro, pos, kq, zero);
          t3_store<LEAKY, kT3CS1, kT3Pl1>(acc, sm + kT3A2 + (r & 3) * 2 * kT3Pl1, pos, mb, kq, alpha, amax);
        }
        if (y >= 7 && y < 7 + 9) {  // stage 3 (3x1)
          const int r = y - 7;
          const int ro[3] = {kT3A2 + (r & 3) * 2 * kT3Pl1, kT3A2 + ((r + 1) & 3) * 2 * kT3Pl1,
                             kT3A2 + ((r + 2) & 3) * 2 * kT3Pl1};
          const f4 acc = t3_block<6, kT3C1, kT3CS1, kT3Pl1>(w3h, w3l, t3_bias(sb + 2 * kT3C1 + bo), sm, ro, pos, kq,
                                                           zero);
          t3_store<LEAKY, kT3CS1, kT3Pl1>(acc, sm + kT3A3 + (r & 1) * 2 * kT3Pl1, pos, mb, kq, alpha, amax);
        }
        if (y >= 8 && y < 8 + 9) {  // stage 4 (1x1)
          const int r = y - 8;
          const int ro[3] = {kT3A3 + (r & 1) * 2 * kT3Pl1, 0, 0};
          const f4 acc = t3_block<2, kT3C1, kT3CS1, kT3Pl1>(w4h, w4l, t3_bias(sb + 3 * kT3C1 + bo), sm, ro, pos, kq,
                                                           zero);
          t3_store<LEAKY, kT3CS1, kT3Pl1>(acc, sm + kT3A4 + (r & 3) * 2 * kT3Pl1, pos, mb, kq, alpha, amax);
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
          t3_store<LEAKY, kT3CS2, kT3Pl2>(acc, sm + A5 + (r & 1) * 2 * kT3Pl2, pos, mb, kq, alpha, amax);
        }
        if (y >= 11 && y < 11 + 8) {  // stage 6
          const int r = y - 11;
          const int ro[3] = {A5 + (r & 1) * 2 * kT3Pl2, 0, 0};
          const f4 acc = t3_block<3, kT3C2, kT3CS2, kT3Pl2>(w6h, w6l, t3_bias(bb + kT3C2), sm, ro, pos, kq, zero);
          t3_store<LEAKY, kT3CS2, kT3Pl2>(acc, sm + A6 + (r & 1) * 2 * kT3Pl2, pos, mb, kq, alpha, amax);
        }
        if (y >= 12 && y < 12 + 8) {  // stage 7
          const int r = y - 12;
          const int ro[3] = {A6 + (r & 1) * 2 * kT3Pl2, 0, 0};
          const f4 acc = t3_block<3, kT3C2, kT3CS2, kT3Pl2>(w7h, w7l, t3_bias(bb + 2 * kT3C2), sm, ro, pos, kq, zero);
          t3_store<LEAKY, kT3CS2, kT3Pl2>(acc, sm + A7 + (r & 1) * 2 * kT3Pl2, pos, mb, kq, alpha, amax);
        }
        if (y >= 13 && y < 13 + 8) {  // stage 8
          const int r = y - 13;
          const int ro[3] = {A7 + (r & 1) * 2 * kT3Pl2, 0, 0};
          const f4 acc = t3_block<3, kT3C2, kT3CS2, kT3Pl2>(w8h, w8l, t3_bias(bb + 3 * kT3C2), sm, ro, pos, kq, zero);
          t3_store<LEAKY, kT3CS2, kT3Pl2>(acc, sm + A8 + (r & 1) * 2 * kT3Pl2, pos, mb, kq, alpha, amax);
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

// ------------------------------------------------------------------ host ----

// Planning is hbk_embed_plan.h (pure host); here a plan is realised on the
// device and launched.
static_assert(kPlanOk == HBK_OK && kPlanErrArg == HBK_ERR_ARG && kPlanErrUnsupported == HBK_ERR_UNSUPPORTED &&
                  kOpConv == HBK_OP_CONV && kOpMaxPool == HBK_OP_MAXPOOL,
              "hbk_embed_plan.h mirrors include/hbk.h");

// One Launch of the host plan on the device: its kernel, its blob and its
// arguments with the blob's pointers in place.
struct Slot {
  const Launch* plan = nullptr;
  const void* fn = nullptr;  // null: nothing planned, or a pattern kernel the device refused
  void* d_blob = nullptr;
  int blocks_per_cu = 0;
  KernelArgs args;
};

struct ChainPlan {
  Slot pattern, base;  // tried in this order at launch
};

}  // namespace
}  // namespace hbk

struct hbk_embed_plan {
  hbk::EmbedHostPlan host;
  std::vector<hbk::ChainPlan> clip, win;  // beside host.clip.chains / host.win.chains
  int* d_gather = nullptr;                // host.clip.gather_src
  int* d_range = nullptr;                 // range flag of the split-f16 kernels (hbk_embed_range_status)
};

namespace hbk {
namespace {

// out[u][i][:] = src[u][gather_src[i]][:] (rows of `row` floats, row % 4 == 0);
// one wave per unit, all of a unit's reads ahead of its writes (distinct buffers)
__global__ void __launch_bounds__(256) embed_gather_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                           const int* __restrict__ map, int64_t n_units, int n_src,
                                                           int n_out, int row) {
  const int lane = threadIdx.x & 63;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (u >= n_units) return;
  const int r4 = row / 4, n4 = n_out * r4;
  const float4* s = reinterpret_cast<const float4*>(src + u * n_src * row);
  float4* d = reinterpret_cast<float4*>(out + u * n_out * row);
  for (int f = lane; f < n4; f += 64) {
    const int i = f / r4, c = f - i * r4;
    d[f] = s[map[i] * r4 + c];
  }
}

// The one reader of the planning knobs, called at every plan creation
// (HBK_EMBED_CHUNK is latched per process in chunk_clips).
EmbedKnobs read_embed_knobs() {
  EmbedKnobs k;
  if (const char* e = getenv("HBK_EMBED_LDS_KB")) {
    k.lds_kb_set = true;
    k.lds_kb = atoi(e);
  }
  if (const char* e = getenv("HBK_EMBED_WEIGHTS")) k.weights = !strcmp(e, "lds") ? 1 : !strcmp(e, "global") ? 2 : 0;
  k.no_p0 = getenv("HBK_EMBED_NO_P0") != nullptr;
  k.no_p0s = getenv("HBK_EMBED_NO_P0S") != nullptr;
  k.no_p1 = getenv("HBK_EMBED_NO_P1") != nullptr;
  k.no_p1s = getenv("HBK_EMBED_NO_P1S") != nullptr;
  k.no_p2s = getenv("HBK_EMBED_NO_P2S") != nullptr;
  k.no_t3s = getenv("HBK_EMBED_NO_T3S") != nullptr;
  k.no_dedup = getenv("HBK_EMBED_NO_DEDUP") != nullptr;
  if (const char* e = getenv("HBK_P0_BAND")) k.p0_band = atoi(e);
  k.debug = getenv("HBK_DEBUG_EMBED") != nullptr;
  if (const char* e = getenv("HBK_DEBUG_SKIP")) k.debug_skip = atoi(e);
  return k;
}

template <class A>
const void* addr(void (*kernel)(A)) {
  return reinterpret_cast<const void*>(kernel);
}

// The kernel that a KernelChoice names.
const void* kernel_address(KernelChoice k) {
  const bool f = k.flag;
  switch (k.kind) {
    case Kern::exact:  // RB x NB accumulators of 4 VGPRs: keep RB * NB <= 12
      switch (k.n) {
        case 1: return f ? addr(conv_chain_kernel<1, 4, true>) : addr(conv_chain_kernel<1, 4, false>);
        case 2: return f ? addr(conv_chain_kernel<2, 4, true>) : addr(conv_chain_kernel<2, 4, false>);
        case 3: return f ? addr(conv_chain_kernel<3, 4, true>) : addr(conv_chain_kernel<3, 4, false>);
        case 4: return f ? addr(conv_chain_kernel<4, 2, true>) : addr(conv_chain_kernel<4, 2, false>);
        case 5: return f ? addr(conv_chain_kernel<5, 2, true>) : addr(conv_chain_kernel<5, 2, false>);
        default: return f ? addr(conv_chain_kernel<6, 2, true>) : addr(conv_chain_kernel<6, 2, false>);
      }
    case Kern::x3:
      switch (k.n) {
        case 1: return f ? addr(conv_chain_x3_kernel<1, true>) : addr(conv_chain_x3_kernel<1, false>);
        case 2: return f ? addr(conv_chain_x3_kernel<2, true>) : addr(conv_chain_x3_kernel<2, false>);
        case 3: return f ? addr(conv_chain_x3_kernel<3, true>) : addr(conv_chain_x3_kernel<3, false>);
        default: return f ? addr(conv_chain_x3_kernel<4, true>) : addr(conv_chain_x3_kernel<4, false>);  // > 3 blocks: groups of 3
      }
    case Kern::p0_band:
      switch (k.n) {
        case 5: return f ? addr(p0_chain_kernel<kP0W, kP0C, 5, true>) : addr(p0_chain_kernel<kP0W, kP0C, 5, false>);
        case 7: return f ? addr(p0_chain_kernel<kP0W, kP0C, 7, true>) : addr(p0_chain_kernel<kP0W, kP0C, 7, false>);
        default: return f ? addr(p0_chain_kernel<kP0W, kP0C, 6, true>) : addr(p0_chain_kernel<kP0W, kP0C, 6, false>);
      }
    case Kern::p0s: return f ? addr(p0s_chain_kernel<true>) : addr(p0s_chain_kernel<false>);
    case Kern::p1:
      return f ? addr(p1_chain_kernel<kP1W, kP1CI, kP1Band, true>) : addr(p1_chain_kernel<kP1W, kP1CI, kP1Band, false>);
    case Kern::p1s: return f ? addr(p1s_chain_kernel<true>) : addr(p1s_chain_kernel<false>);
    case Kern::p2s: return f ? addr(p2s_chain_kernel<true>) : addr(p2s_chain_kernel<false>);
    case Kern::t3s: return f ? addr(t3s_chain_kernel<true>) : addr(t3s_chain_kernel<false>);
  }
  return nullptr;
}

// Dynamic-LDS limit of a kernel raised to what the CU holds beside its static
// LDS (set once to the maximum, so plans sharing the kernel never lower it).
hipError_t set_max_dynamic_lds(const void* fn) {
  hipFuncAttributes at;
  hipError_t e = hipFuncGetAttributes(&at, fn);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                             int(160 * 1024 - static_cast<int>(at.sharedSizeBytes)));
}

// The blob's addresses in the argument struct (Launch::ptr_off).
void set_pointers(ChainArgs& a, const Launch&, const unsigned char* blob) {
  a.wblob = reinterpret_cast<const float*>(blob);
}
void set_pointers(XArgs& x, const Launch& L, const unsigned char* blob) {
  x.wblob = reinterpret_cast<const _Float16*>(blob);
  x.bblob = reinterpret_cast<const float*>(blob + L.ptr_off[1]);
  x.ktab = reinterpret_cast<const int*>(blob + L.ptr_off[2]);
  x.i2c_off = reinterpret_cast<const int*>(blob + L.ptr_off[3]);
}
template <class A>
void set_pointers(A& p, const Launch& L, const unsigned char* blob) {  // the pattern kernels
  p.w = reinterpret_cast<const _Float16*>(blob);
  if (L.ptr_off[1] >= L.blob.size()) return;  // (p0s: its biases ride in the weights)
  const float* bias = reinterpret_cast<const float*>(blob + L.ptr_off[1]);
  if constexpr (std::is_same_v<A, P2sArgs>) p.bias_a = bias;
  else p.bias = bias;
}

// Uploads a Launch's bytes, points its arguments at them, resolves its kernel,
// raises the kernel's dynamic-LDS limit and prints the debug line. A pattern
// kernel whose upload, attribute or occupancy call fails is dropped silently
// (its slot stays empty and the chain runs on its generic kernel).
int realise(const Launch& L, bool pattern, bool debug, Slot& s) {
  const void* fn = kernel_address(L.kernel);
  hipError_t e = hipMalloc(&s.d_blob, L.blob.size());
  if (e != hipSuccess && !pattern) return hip_error(e, "hipMalloc chain weights");
  if (e == hipSuccess) e = hipMemcpy(s.d_blob, L.blob.data(), L.blob.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess && !pattern) return hip_error(e, "copy chain weights");
  if (pattern) {
    if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(L.lds_bytes));
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&s.blocks_per_cu, fn, L.threads, L.lds_bytes);
    if (e != hipSuccess || s.blocks_per_cu < 1) {
      (void)hipGetLastError();
      if (s.d_blob) (void)hipFree(s.d_blob);
      s.d_blob = nullptr;
      return HBK_OK;
    }
  } else {
    if (L.lds_bytes > 64 * 1024) {  // the CU maximum: chains sharing a kernel never lower it
      e = set_max_dynamic_lds(fn);
      if (e != hipSuccess) return hip_error(e, "hipFuncSetAttribute(max dynamic LDS)");
    }
    s.blocks_per_cu = L.kernel.kind == Kern::exact
                          ? 2
                          : std::max<int>(1, std::min<int>(4, int((160 * 1024) / std::max<size_t>(L.lds_bytes, 1))));
  }
  s.plan = &L;
  s.fn = fn;
  s.args = L.args;
  std::visit([&](auto& a) { set_pointers(a, L, static_cast<const unsigned char*>(s.d_blob)); }, s.args);
  if (debug && pattern) fprintf(stderr, "%s, %d blocks/CU\n", L.debug.c_str(), s.blocks_per_cu);
  if (debug && !pattern) fputs(L.debug.c_str(), stderr);
  return HBK_OK;
}

int realise_program(const ProgramPlan& prog, bool debug, std::vector<ChainPlan>& dev) {
  dev.resize(prog.chains.size());  // (all slots exist before the first allocation: destroy frees what was made)
  for (size_t k = 0; k < dev.size(); ++k) {
    const int rc = realise(prog.chains[k].base, false, debug, dev[k].base);
    if (rc) return rc;
    if (prog.chains[k].pattern) realise(*prog.chains[k].pattern, true, debug, dev[k].pattern);
  }
  return HBK_OK;
}

// The per-call fields of an argument struct.
void bind(ChainArgs& a, const float* in, int64_t stride, float* out, int64_t n_img, int*) {
  a.in = in;
  a.src_clip_stride = stride;
  a.out = out;
  a.n_img = n_img;
}
void bind(XArgs& x, const float* in, int64_t stride, float* out, int64_t n_img, int* range_flag) {
  x.range_flag = range_flag;
  x.in = in;
  x.src_clip_stride = stride;
  x.out = out;
  if ((reinterpret_cast<uintptr_t>(x.out) & 15) || (x.out_img_stride & 3)) x.vec_out = 0;
  if ((reinterpret_cast<uintptr_t>(x.in) & 15) || (x.src_clip_stride & 3) || (x.src_row_stride & 3)) x.raw_vec = 0;
  x.n_img = n_img;
}
template <class A>
void bind(A& p, const float* in, int64_t stride, float* out, int64_t n_img, int* range_flag) {  // the pattern kernels
  p.range_flag = range_flag;
  p.in = in;
  if constexpr (std::is_same_v<A, T3sArgs>) p.src_clip_stride = stride;
  else p.src_img_stride = stride;
  p.out = out;
  p.n_img = n_img;
}

// Runs chains [k_begin, k_end) of the program (k_end < 0: to the end). The
// first chain run reads `in` (the call's input, or for k_begin > 0 the output
// of chain k_begin - 1 in its workspace layout); the last writes `out` (for
// k_end < n: chain k_end - 1's output in its workspace layout, no gather).
// A chain runs on its pattern kernel when the buffers allow it, else on its
// generic kernel (split-f16 x3 or exact f32).
int run_program(const ProgramPlan& prog, const std::vector<ChainPlan>& dev, const int* d_gather, const float* in,
                int64_t n_units, int64_t in_unit_stride, float* out, int64_t out_unit_floats, float* ws,
                int64_t chunk, hipStream_t stream, int* range_flag, int k_begin = 0, int k_end = -1) {
  const int n_ch = static_cast<int>(prog.chains.size());
  if (k_end < 0) k_end = n_ch;
  for (int64_t u0 = 0; u0 < n_units; u0 += chunk) {
    const int64_t nu = std::min(chunk, n_units - u0);
    float* bufs[2] = {ws, ws + chunk * prog.buf_floats[0]};
    for (int k = k_begin; k < k_end; ++k) {
      const ChainHost& h = prog.chains[k];
      const int src_buf = (k == k_begin && k_begin > 0) ? -1 : h.src_buf;  // the caller's copy of chain k - 1's output
      const int dst_buf = (k == k_end - 1 && k_end < n_ch) ? -1 : h.dst_buf;  // handed to the caller (no gather)
      const float* src = src_buf < 0 ? in + u0 * in_unit_stride : bufs[src_buf];
      const int64_t stride = src_buf < 0 ? in_unit_stride : h.src_clip_stride;
      float* dst = dst_buf < 0 ? out + u0 * out_unit_floats : bufs[dst_buf];
      const int64_t n_img = nu * h.imgs_per_unit;
      for (const Slot* s : {&dev[k].pattern, &dev[k].base}) {
        if (!s->fn) continue;
        const Launch& L = *s->plan;
        if (s == &dev[k].pattern) {
          const bool aligned = !(reinterpret_cast<uintptr_t>(src) & 15) && !(stride & 3) &&
                               !(reinterpret_cast<uintptr_t>(dst) & 15) && !(L.out_stride_4 & 3);
          if (!aligned || stride < L.min_src_stride) continue;
          if (L.tasks_below_2_31 && n_img * L.n_bands >= (int64_t(1) << 31)) continue;
        }
        KernelArgs args = s->args;
        void* argp = std::visit(
            [&](auto& a) -> void* {
              bind(a, src, stride, dst, n_img, range_flag);
              return &a;
            },
            args);
        const int64_t tasks = ((n_img + L.imgs_per_task - 1) / L.imgs_per_task) * L.n_bands;
        const int64_t blocks = std::min<int64_t>(tasks, persistent_blocks(s->blocks_per_cu, stream));
        if (blocks > 0) {
          (void)hipLaunchKernel(s->fn, dim3(unsigned(blocks)), dim3(L.threads), &argp, L.lds_bytes, stream);
          HBK_LAUNCH_CHECK(L.name);
        }
        break;
      }
    }
    if (prog.gather_buf >= 0 && k_end == n_ch) {
      const int n_out = static_cast<int>(prog.gather_src.size());
      const int row = static_cast<int>(out_unit_floats / n_out);
      hipLaunchKernelGGL(embed_gather_kernel, dim3(unsigned((nu + 3) / 4)), dim3(256), 0, stream,
                         bufs[prog.gather_buf], out + u0 * out_unit_floats, d_gather, nu, prog.n_src, n_out, row);
      HBK_LAUNCH_CHECK("embed_gather_kernel");
    }
  }
  return HBK_OK;
}

// The clip / window entry points past their plan check: chains [k_begin, k_end)
// of the clip program (or the window program) over n units in workspace chunks.
int run_units(const hbk_embed_plan* p, bool clips, const float* in, int64_t n, int64_t in_stride, int64_t min_stride,
              float* out, int64_t out_floats, void* workspace, int64_t workspace_bytes, void* stream, int k_begin = 0,
              int k_end = -1) {
  if (n < 0) return arg_error(clips ? "negative n_clips" : "negative n");
  if (n == 0) return HBK_OK;
  if (!in || !out || !workspace) return arg_error("NULL pointer");
  if (in_stride < min_stride) return arg_error("mel_clip_stride < seq_frames * in_w");
  int64_t need = 0;
  hbk_embed_workspace_size(p, n, &need);
  if (workspace_bytes < need) return arg_error("workspace too small");
  return run_program(clips ? p->host.clip : p->host.win, clips ? p->clip : p->win, p->d_gather, in, n, in_stride, out,
                     out_floats, static_cast<float*>(workspace), std::min<int64_t>(n, chunk_clips()),
                     as_stream(stream), p->d_range, k_begin, k_end);
}

}  // namespace
}  // namespace hbk

extern "C" {

int hbk_embed_plan_create(const hbk_graph_op* ops, int32_t n_ops, int32_t in_h, int32_t in_w,
                          const int32_t* win_start, int32_t n_win, hbk_embed_plan** plan) {
  return hbk_embed_plan_create_ex(ops, n_ops, in_h, in_w, win_start, n_win, HBK_PREC_SPLIT_F16, plan);
}

int hbk_embed_plan_create_ex(const hbk_graph_op* ops, int32_t n_ops, int32_t in_h, int32_t in_w,
                             const int32_t* win_start, int32_t n_win, int32_t precision,
                             hbk_embed_plan** plan) {
  using namespace hbk;
  if (!plan) return arg_error("plan is NULL");
  *plan = nullptr;
  if (precision != HBK_PREC_SPLIT_F16 && precision != HBK_PREC_EXACT_F32) return arg_error("unknown precision");
  if (!ops || n_ops <= 0) return arg_error("empty graph");
  if (in_h <= 0 || in_w <= 0) return arg_error("bad window size");
  if (!win_start || n_win <= 0 || n_win > kMaxWin) return arg_error("n_win must be in [1, 32]");
  auto* p = new hbk_embed_plan();
  auto fail = [&](int rc) {
    hbk_embed_plan_destroy(p);
    return rc;
  };
  // the whole plan on the host, with every planning error, before the first device call
  const EmbedKnobs knobs = read_embed_knobs();
  std::vector<OpIn> graph;
  for (int i = 0; i < n_ops; ++i) {
    const hbk_graph_op& o = ops[i];
    graph.push_back(OpIn{o.kind, o.kh, o.kw, o.cin, o.cout, o.act, o.alpha, o.weight, o.bias});
  }
  int rc = plan_embed(graph, in_h, in_w, std::vector<int>(win_start, win_start + n_win),
                      precision == HBK_PREC_SPLIT_F16, knobs, p->host);
  if (rc) {
    set_error("%s", p->host.error.c_str());
    return fail(rc);
  }
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_range), sizeof(int));
  if (e == hipSuccess) e = hipMemset(p->d_range, 0, sizeof(int));
  if (e != hipSuccess) return fail(hip_error(e, "hipMalloc range flag"));
  rc = realise_program(p->host.clip, knobs.debug, p->clip);
  if (rc) return fail(rc);
  if (const std::vector<int>& map = p->host.clip.gather_src; !map.empty()) {
    e = hipMalloc(reinterpret_cast<void**>(&p->d_gather), map.size() * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(p->d_gather, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(hip_error(e, "embed gather map"));
    if (knobs.debug) fputs(p->host.dedup_debug.c_str(), stderr);
  }
  rc = realise_program(p->host.win, knobs.debug, p->win);
  if (rc) return fail(rc);
  *plan = p;
  return HBK_OK;
}

int hbk_embed_plan_destroy(hbk_embed_plan* p) {
  if (!p) return HBK_OK;
  for (auto* dev : {&p->clip, &p->win})
    for (auto& c : *dev)
      for (hbk::Slot* s : {&c.pattern, &c.base})
        if (s->d_blob) (void)hipFree(s->d_blob);
  if (p->d_gather) (void)hipFree(p->d_gather);
  if (p->d_range) (void)hipFree(p->d_range);
  delete p;
  return HBK_OK;
}

int hbk_embed_plan_info(const hbk_embed_plan* p, int32_t* out_dim, int32_t* n_prefix_ops,
                        int32_t* n_chains, double* prefix_macs, double* tail_macs,
                        int32_t* seq_frames) {
  if (!p) return hbk::arg_error("plan is NULL");
  if (out_dim) *out_dim = p->host.out_dim;
  if (n_prefix_ops) *n_prefix_ops = p->host.n_prefix;
  if (n_chains) *n_chains = static_cast<int32_t>(p->host.clip.chains.size());
  if (prefix_macs) *prefix_macs = p->host.prefix_macs;
  if (tail_macs) *tail_macs = p->host.tail_macs;
  if (seq_frames) *seq_frames = p->host.seq_frames;
  return HBK_OK;
}

}  // extern "C"

namespace hbk {

// ---- NaN rows (embeddings.py:209-234): in place, no host synchronisation ----
// Three grid-wide launches, each a no-op past one load when the batch has no NaN row:
// nan_flags_kernel: block b owns the contiguous rows [b*per, (b+1)*per) (one wave per row,
//   float4 loads): flags[r] = 1 for a NaN row, which is appended to bad[] (meta[0] counts
//   them; the order is free, a row's draw depends on (seed, row) only), and blk_good[b] counts
//   the block's NaN-free rows.
// nan_list_kernel: block b lists its NaN-free rows in order at the offset sum(blk_good[< b])
//   (ballot scans over 256-row slices), so good[] is every NaN-free row, ascending.
// nan_patch_kernel: one wave per NaN row copies good[h % n_good], h a hash of (seed, row) — a
//   uniformly drawn NaN-free clip, as the reference's np.random.choice — or writes zeros when
//   every row is NaN.
constexpr int kNanBlocks = 2048;  // flags / list blocks at most (blk_good's length)
constexpr int kNanPatchBlocks = 512;

__global__ void __launch_bounds__(256) nan_flags_kernel(const float* __restrict__ rows, int64_t n, int64_t row_len,
                                                        int64_t per, int32_t* __restrict__ flags,
                                                        int32_t* __restrict__ blk_good, int32_t* __restrict__ bad,
                                                        int32_t* __restrict__ meta) {
  __shared__ int32_t s_good;
  if (threadIdx.x == 0) s_good = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * per, hi = min<int64_t>(n, lo + per);
  int32_t n_good = 0;
  for (int64_t r = lo + wave; r < hi; r += 4) {
    const float4* p = reinterpret_cast<const float4*>(rows + r * row_len);
    bool nan = false;
    for (int64_t j = lane; j < row_len / 4; j += 64) {
      const float4 v = p[j];
      nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
    }
    const bool any = __ballot(nan) != 0;
    if (lane == 0) {
      flags[r] = any ? 1 : 0;
      if (any)
        bad[atomicAdd(meta, 1)] = static_cast<int32_t>(r);
      else
        ++n_good;
    }
  }
  if (lane == 0) atomicAdd(&s_good, n_good);
  __syncthreads();
  if (threadIdx.x == 0) blk_good[blockIdx.x] = s_good;
}

__global__ void __launch_bounds__(256) nan_list_kernel(int64_t n, int64_t per, const int32_t* __restrict__ flags,
                                                       const int32_t* __restrict__ blk_good,
                                                       int32_t* __restrict__ good, const int32_t* __restrict__ meta) {
  __shared__ int32_t s_w[4];
  __shared__ int32_t s_off;
  if (meta[0] == 0) return;  // uniform: the common case
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t off = 0;  // NaN-free rows of the blocks before this one
  for (int i = tid; i < static_cast<int>(blockIdx.x); i += 256) off += blk_good[i];
  for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
  if (lane == 0) s_w[wave] = off;
  __syncthreads();
  if (tid == 0) s_off = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  __syncthreads();
  off = s_off;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * per, hi = min<int64_t>(n, lo + per);
  for (int64_t base = lo; base < hi; base += 256) {
    const int64_t r = base + tid;
    const bool keep = r < hi && flags[r] == 0;
    const uint64_t m = __ballot(keep);
    const int32_t below = __popcll(m & ((uint64_t(1) << lane) - 1));
    __syncthreads();  // s_w of the previous slice has been read
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int32_t pre = 0;
    for (int w = 0; w < wave; ++w) pre += s_w[w];
    if (keep) good[off + pre + below] = static_cast<int32_t>(r);
    off += s_w[0] + s_w[1] + s_w[2] + s_w[3];
  }
}

__device__ __forceinline__ uint64_t nan_hash(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) nan_patch_kernel(float* __restrict__ rows, int64_t n, int64_t row_len,
                                                        const int32_t* __restrict__ bad,
                                                        const int32_t* __restrict__ good,
                                                        const int32_t* __restrict__ meta, uint64_t seed) {
  const int64_t n_bad = meta[0];
  if (n_bad == 0) return;
  const int64_t n_good = n - n_bad;
  const int lane = threadIdx.x & 63;
  const int64_t nw = static_cast<int64_t>(gridDim.x) * 4;
  for (int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 6; i < n_bad; i += nw) {
    const int64_t r = bad[i];
    float4* dst = reinterpret_cast<float4*>(rows + r * row_len);
    if (n_good == 0) {
      for (int64_t j = lane; j < row_len / 4; j += 64) dst[j] = float4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const uint64_t h = nan_hash(seed ^ (0x9E3779B97F4A7C15ull * static_cast<uint64_t>(r + 1)));
    const int64_t src = good[static_cast<int64_t>((static_cast<unsigned __int128>(h) * static_cast<uint64_t>(n_good)) >> 64)];
    const float4* sp = reinterpret_cast<const float4*>(rows + src * row_len);
    for (int64_t j = lane; j < row_len / 4; j += 64) dst[j] = sp[j];
  }
}

}  // namespace hbk

extern "C" {

int hbk_embed_workspace_size(const hbk_embed_plan* p, int64_t n, int64_t* bytes) {
  using namespace hbk;
  if (!p || !bytes) return arg_error("plan/bytes is NULL");
  if (n < 0) return arg_error("negative n");
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, chunk_clips()));
  const int64_t *bc = p->host.clip.buf_floats, *bw = p->host.win.buf_floats;
  *bytes = chunk * std::max(bc[0] + bc[1], bw[0] + bw[1]) * int64_t(sizeof(float)) + 256;
  return HBK_OK;
}

int hbk_embed_clips(const hbk_embed_plan* p, const float* mel, int64_t n_clips, int64_t mel_clip_stride,
                    float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  if (!p) return arg_error("plan is NULL");
  return run_units(p, true, mel, n_clips, mel_clip_stride, int64_t(p->host.seq_frames) * p->host.in_w, out,
                   int64_t(p->host.n_win) * p->host.out_dim, workspace, workspace_bytes, stream);
}

int hbk_embed_split_info(const hbk_embed_plan* p, int32_t n_front, int64_t* mid_floats_per_clip) {
  using namespace hbk;
  if (!p || !mid_floats_per_clip) return arg_error("plan/mid_floats_per_clip is NULL");
  const int n = static_cast<int>(p->host.clip.chains.size());
  if (n_front < 1 || n_front >= n) return arg_error("n_front must be in [1, n_chains - 1]");
  const ChainHost& c = p->host.clip.chains[n_front - 1];
  *mid_floats_per_clip = c.out_img_stride * c.imgs_per_unit;
  return HBK_OK;
}

int hbk_embed_clips_front(const hbk_embed_plan* p, const float* mel, int64_t n_clips, int64_t mel_clip_stride,
                          int32_t n_front, float* mid, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  int64_t mid_floats = 0;
  int rc = hbk_embed_split_info(p, n_front, &mid_floats);
  if (rc) return rc;
  return run_units(p, true, mel, n_clips, mel_clip_stride, int64_t(p->host.seq_frames) * p->host.in_w, mid,
                   mid_floats, workspace, workspace_bytes, stream, 0, n_front);
}

int hbk_embed_clips_back(const hbk_embed_plan* p, const float* mid, int64_t n_clips, int32_t n_front, float* out,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  int64_t mid_floats = 0;
  int rc = hbk_embed_split_info(p, n_front, &mid_floats);
  if (rc) return rc;
  return run_units(p, true, mid, n_clips, mid_floats, 0, out, int64_t(p->host.n_win) * p->host.out_dim, workspace,
                   workspace_bytes, stream, n_front, -1);
}

int hbk_embed_windows(const hbk_embed_plan* p, const float* windows, int64_t n, float* out,
                      void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  if (!p) return arg_error("plan is NULL");
  return run_units(p, false, windows, n, int64_t(p->host.in_h) * p->host.in_w, 0, out, p->host.out_dim, workspace,
                   workspace_bytes, stream);
}

int64_t hbk_nan_rows_workspace_size(int64_t n) {
  return n < 0 ? 0 : (3 * n + hbk::kNanBlocks + 1) * int64_t(sizeof(int32_t));
}

int hbk_nan_rows_fix(float* rows, int64_t n, int64_t row_len, uint64_t seed, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  if (n < 0 || row_len <= 0 || row_len % 4) return arg_error("n >= 0, row_len a positive multiple of 4");
  if (n == 0) return HBK_OK;
  if (n >= (int64_t(1) << 31)) return arg_error("n >= 2^31 rows");
  if (!rows || !workspace) return arg_error("NULL pointer");
  if ((reinterpret_cast<uintptr_t>(rows) & 15)) return arg_error("rows must be 16-B aligned");
  if (workspace_bytes < hbk_nan_rows_workspace_size(n)) return arg_error("workspace too small");
  int32_t* flags = static_cast<int32_t*>(workspace);  // [n]
  int32_t* good = flags + n;                          // [n]
  int32_t* bad = good + n;                            // [n]
  int32_t* blk_good = bad + n;                        // [kNanBlocks]
  int32_t* meta = blk_good + kNanBlocks;              // [1]: NaN rows
  hipStream_t st = as_stream(stream);
  hipError_t e = hipMemsetAsync(meta, 0, sizeof(int32_t), st);
  if (e != hipSuccess) return hip_error(e, "hbk_nan_rows_fix");
  const int64_t blocks = std::min<int64_t>(kNanBlocks, (n + 3) / 4);
  const int64_t per = (n + blocks - 1) / blocks;
  const int64_t used = (n + per - 1) / per;  // every launched block owns at least one row
  hipLaunchKernelGGL(nan_flags_kernel, dim3(unsigned(used)), dim3(256), 0, st, rows, n, row_len, per, flags,
                     blk_good, bad, meta);
  HBK_LAUNCH_CHECK("nan_flags_kernel");
  hipLaunchKernelGGL(nan_list_kernel, dim3(unsigned(used)), dim3(256), 0, st, n, per, flags, blk_good, good, meta);
  HBK_LAUNCH_CHECK("nan_list_kernel");
  const int64_t pblocks = std::min<int64_t>(kNanPatchBlocks, (n + 3) / 4);
  hipLaunchKernelGGL(nan_patch_kernel, dim3(unsigned(pblocks)), dim3(256), 0, st, rows, n, row_len, bad, good, meta,
                     seed);
  HBK_LAUNCH_CHECK("nan_patch_kernel");
  return HBK_OK;
}

int hbk_embed_range_status(const hbk_embed_plan* p, int32_t* tripped, int32_t reset, void* stream) {
  using namespace hbk;
  if (!p || !tripped) return arg_error("plan/tripped is NULL");
  int32_t h = 0;
  hipError_t e = hipMemcpyAsync(&h, p->d_range, sizeof(int32_t), hipMemcpyDeviceToHost, as_stream(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
  if (e == hipSuccess && reset && h) e = hipMemsetAsync(p->d_range, 0, sizeof(int32_t), as_stream(stream));
  if (e != hipSuccess) return hip_error(e, "hbk_embed_range_status");
  *tripped = h;
  return HBK_OK;
}

}  // extern "C"

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

#ifdef HBK_TRACE
extern "C" int hbk_debug_trace(unsigned long long* out, int* counts) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hbk::g_trace), sizeof(unsigned long long) * 4 * 4 * 256) != hipSuccess)
    return -2;
  if (hipMemcpyFromSymbol(counts, HIP_SYMBOL(hbk::g_trace_n), sizeof(int) * 16) != hipSuccess) return -2;
  int z[16] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(hbk::g_trace_n), z, sizeof(z));
  return 0;
}
#endif
