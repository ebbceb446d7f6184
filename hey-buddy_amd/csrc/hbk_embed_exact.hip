// Speech-embedding conv stack: the exact-f32 chain kernel (HBK_PREC_EXACT_F32, and the base
// kernel of a chain the split-f16 planner cannot take). The execution model (chains, tasks,
// bands, the clip path) is described in hbk_embed.hip, which launches this kernel through
// embed_exact_kernel; ChainArgs / StageDesc are in hbk_embed_args.h, their planner in
// hbk_embed_plan.h; the split-f16 kernels are in hbk_embed_x3.hip, hbk_embed_band.hip and
// hbk_embed_stream.hip.
#include "hbk_embed_dev.h"
#include "hbk_embed_internal.h"

namespace hbk {
namespace {

constexpr int kWaves = kThreads / 64;

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

}  // namespace

// n = output-channel blocks (NB), f = weights read from global memory (WG)
const void* embed_exact_kernel(int n, bool f) {
  // RB x NB accumulators of 4 VGPRs: keep RB * NB <= 12
  switch (n) {
    case 1: return f ? addr(conv_chain_kernel<1, 4, true>) : addr(conv_chain_kernel<1, 4, false>);
    case 2: return f ? addr(conv_chain_kernel<2, 4, true>) : addr(conv_chain_kernel<2, 4, false>);
    case 3: return f ? addr(conv_chain_kernel<3, 4, true>) : addr(conv_chain_kernel<3, 4, false>);
    case 4: return f ? addr(conv_chain_kernel<4, 2, true>) : addr(conv_chain_kernel<4, 2, false>);
    case 5: return f ? addr(conv_chain_kernel<5, 2, true>) : addr(conv_chain_kernel<5, 2, false>);
    default: return f ? addr(conv_chain_kernel<6, 2, true>) : addr(conv_chain_kernel<6, 2, false>);
  }
}

}  // namespace hbk
