// Half-layer bank of the wake-word classifier for gfx950 (use_half_layers,
// wakeword.py:211-223, :278-302, :334-348): n_half branches
//   states += GatedMLP_h(LayerNorm_h(flatten(x_d[:, idx_h, :])))
// that all read the dropped-out input of norm_in; branch h takes n_tokens / 2 of the row's
// n_tokens chunks in the order idx_h lists them. Numerics are f32 (v_mfma_f32_16x16x4f32).
//
// Parameter layout: the bank is appended to the flat buffer of hbk_mlp.hip; branch h owns one
// run of `stride` floats (hbk_mlp_half_plan.h: HalfOffsets), in this order:
//   half_layers.h.0.weight, .0.bias        [K] x 2, K = d_in / 2, columns in gathered order
//   W_hg [2H, K]   rows 0..H-1 = half_layers.h.1.hidden.weight, H..2H-1 = .1.gate.weight
//   b_hg [2H]      .1.hidden.bias, .1.gate.bias
//   W_o  [L, H]    .1.output.weight,  b_o [L] .1.output.bias
// so every state-dict tensor is one contiguous run.
//
// Forward (5 launches, no atomics: two runs give the same bits):
//   half_stats_kernel  mean / rstd of every (row, branch) from per-chunk two-pass sums
//                      (each chunk's mean and centred square sum once, combined per branch);
//                      with dropout on it also keeps the dropped-out input [B, d_in], so that
//                      the products below hash no element again
//   half_hg_kernel     HG_h = Xn_h W_hg_h^T + b_hg_h over (row tile, column tile, branch);
//                      Xn is rebuilt from x and the statistics while staging, never stored
//   gate_fwd_kernel    U = silu(H) * G over [B n_half, H]: the generic path's kernel (mlp_gate_forward)
//   half_out_kernel    part_h = U_h W_o_h^T over (row tile, column tile, branch): the GEMM of depth
//                      n_half * H over [U_0 .. U_{n-1}], its depth split by branch
//   half_sum_kernel    s0 += sum_h (part_h + b_o_h), branches in order
// Backward (4 launches; branch inputs are leaves, no dx), from dS0 = gradient at s0:
//   half_colsum_kernel db_o_h = colsum dS0 (every h)
//   half_dwo_kernel    dW_o = dS0^T [U_0 ..], batch split over workgroups (atomics)
//   half_du_kernel     dU = dS0 W_o, the gate's backward into dHG, and cs_h = colsum dHG_h = db_hg_h
//   half_dwhg_kernel   T_h = dHG_h^T Xhat_h (Xhat rebuilt while staging), then
//                      dW_hg = T g + cs b^T, dg = sum_n W_hg o T, db = sum_n W_hg cs
#include "hbk_common.h"
#include "hbk_mlp_half_plan.h"
#include "hbk_mlp_internal.h"

namespace hbk {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int TM = kHalfTile, TN = kHalfTile, TK = kHalfTileK;

// what the kernels need of the plan, by value
struct HalfDev {
  int d_in, chunk, per, K, H, L, nh, n_tokens;
  int64_t base, stride, o_b, o_whg, o_bhg, o_wo, o_bo;
  unsigned char tok[kHalfMaxIdx];  // [nh][per]
};

struct Drop {
  float p, ks;
  uint64_t seed;
};

__device__ __forceinline__ Drop make_drop(float p, uint64_t seed, const double* step_sc) {
  if (step_sc) seed = static_cast<uint64_t>(step_sc[2]);  // graph replays: per-step seed from the device
  return Drop{p, p > 0.f ? 1.f / (1.f - p) : 1.f, seed};
}

// element (row, col) of the dropped-out input (dropout_elem): the mask is a function of the
// element's place in the ungathered row, so every branch and norm_in see one mask
__device__ __forceinline__ float xval(const float* __restrict__ x, int64_t row, int col, int d_in, const Drop& d) {
  const int64_t e = row * d_in + col;
  return dropout_elem(x[e], d.seed, static_cast<uint64_t>(e), d.p, d.ks);
}

// gathered column c of branch h -> column of the flattened row
__device__ __forceinline__ int src_col(const HalfDev& hd, int h, int c) {
  const int t = c / hd.chunk;
  return hd.tok[h * hd.per + t] * hd.chunk + (c - t * hd.chunk);
}

// One 64 x 64 output tile, 4 waves as 2 x 2 of 32 x 32, over k in [kb, ke): acc += A B with
// A(m, k) = la(m, k), B(k, n) = lb(n, k), m / n tile-local; the loaders return 0 outside their
// matrices. AK / BK: the loader's memory is contiguous along k (else along m / n).
// The loaders read unconditionally, from indices clamped into their matrices, and select 0
// afterwards: a load under a bounds branch cannot be hoisted, and the 32 loads of a slice would
// wait for one another instead of being in flight together.
// acc[i][j][q] is element (32 wr + 16 i + 4 (lane >> 4) + q, 32 wc + 16 j + (lane & 15)).
template <bool AK, bool BK, class LA, class LB>
__device__ __forceinline__ void mma_tile(f4 (&acc)[2][2], const LA& la, const LB& lb, int kb, int ke) {
  // rows padded by one float: a k-contiguous loader writes a column (stride TM + 1: 2-way bank
  // conflicts at most), the MFMA operands read along rows
  __shared__ float As[TK][TM + 1];
  __shared__ float Bs[TK][TN + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  constexpr int NA = TM * TK / 256, NB = TN * TK / 256;
  for (int k0 = kb; k0 < ke; k0 += TK) {
    float va[NA], vb[NB];
#pragma unroll
    for (int it = 0; it < NA; ++it) {
      const int e = tid + 256 * it;
      int m, k;
      if (AK) { m = e / TK; k = e - m * TK; } else { k = e / TM; m = e - k * TM; }
      const float v = la(m, min(k0 + k, ke - 1));
      va[it] = (k0 + k < ke) ? v : 0.f;
    }
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      const int e = tid + 256 * it;
      int n, k;
      if (BK) { n = e / TK; k = e - n * TK; } else { k = e / TN; n = e - k * TN; }
      const float v = lb(n, min(k0 + k, ke - 1));
      vb[it] = (k0 + k < ke) ? v : 0.f;
    }
#pragma unroll
    for (int it = 0; it < NA; ++it) {
      const int e = tid + 256 * it;
      if (AK) As[e % TK][e / TK] = va[it]; else As[e / TM][e % TM] = va[it];
    }
#pragma unroll
    for (int it = 0; it < NB; ++it) {
      const int e = tid + 256 * it;
      if (BK) Bs[e % TK][e / TK] = vb[it]; else Bs[e / TN][e % TN] = vb[it];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TK; kk += 4) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = As[kk + kq][32 * wr + 16 * i + r16];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = Bs[kk + kq][32 * wc + 16 * j + r16];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
}

// tile-local coordinates of this lane's accumulators
struct Lane {
  int wr, wc, r16, kq;
  __device__ Lane() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wr = wave >> 1;
    wc = wave & 1;
    r16 = lane & 15;
    kq = lane >> 4;
  }
  __device__ int m(int i, int q) const { return 32 * wr + 16 * i + 4 * kq + q; }
  __device__ int n(int j) const { return 32 * wc + 16 * j + r16; }
};

// ------------------------------------------------------------- forward -----
// One workgroup per row, its 4 waves taking the chunks in turn. Chunk t: mean_t and
// q_t = sum (x - mean_t)^2 (two passes); branch h over its chunks: mu = mean of mean_t,
// M2 = sum_t q_t + chunk (mean_t - mu)^2 (the pairwise update of Chan et al.), var = M2 / K biased:
// ln_fwd_kernel's two-pass accuracy without a pass per branch.
__global__ void __launch_bounds__(256) half_stats_kernel(HalfDev hd, const float* __restrict__ x,
                                                         float* __restrict__ stats, float* __restrict__ xd,
                                                         int rows, float drop_p, uint64_t seed,
                                                         const double* __restrict__ step_sc) {
  __shared__ float cm[kHalfMaxTokens], cq[kHalfMaxTokens];
  const Drop dr = make_drop(drop_p, seed, step_sc);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x;  // (the grid is the batch)
  const float* xs = xd ? xd : x;
  for (int t = wave; t < hd.n_tokens; t += 4) {
    const int c0 = t * hd.chunk;
    float s = 0.f;
    for (int i = lane; i < hd.chunk; i += 64) {
      const float v = xval(x, row, c0 + i, hd.d_in, dr);
      if (xd) xd[row * hd.d_in + c0 + i] = v;  // (read back below by the lane that wrote it)
      s += v;
    }
    const float mean = wave_sum(s) / hd.chunk;
    float q = 0.f;
    for (int i = lane; i < hd.chunk; i += 64) {
      const float d = xs[row * hd.d_in + c0 + i] - mean;
      q += d * d;
    }
    q = wave_sum(q);
    if (lane == 0) {
      cm[t] = mean;
      cq[t] = q;
    }
  }
  __syncthreads();
  for (int h = threadIdx.x; h < hd.nh; h += 256) {
    float mu = 0.f;
    for (int t = 0; t < hd.per; ++t) mu += cm[hd.tok[h * hd.per + t]];
    mu /= hd.per;
    float m2 = 0.f;
    for (int t = 0; t < hd.per; ++t) {
      const int tk = hd.tok[h * hd.per + t];
      const float d = cm[tk] - mu;
      m2 += cq[tk] + hd.chunk * d * d;
    }
    float* o = stats + (row * hd.nh + h) * 2;
    o[0] = mu;
    o[1] = 1.f / sqrtf(m2 / hd.K + kLnEps);
  }
}

// HG[b, h, :] = Xn_h[b, :] W_hg_h^T + b_hg_h; grid (tiles of 2H, tiles of B, branch)
__global__ void __launch_bounds__(256) half_hg_kernel(HalfDev hd, const float* __restrict__ P,
                                                      const float* __restrict__ xs, const float* __restrict__ stats,
                                                      float* __restrict__ hg, int rows) {
  const int h = blockIdx.z, N = 2 * hd.H;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const float* ph = P + hd.base + h * hd.stride;
  const float *gam = ph, *bet = ph + hd.o_b, *W = ph + hd.o_whg, *bias = ph + hd.o_bhg;
  auto la = [&](int m, int k) -> float {
    const int64_t row = min(m0 + m, rows - 1);
    const float* st = stats + (row * hd.nh + h) * 2;
    const float v = (xs[row * hd.d_in + src_col(hd, h, k)] - st[0]) * st[1] * gam[k] + bet[k];
    return m0 + m < rows ? v : 0.f;
  };
  auto lb = [&](int n, int k) -> float {
    const float v = W[int64_t(min(n0 + n, N - 1)) * hd.K + k];
    return n0 + n < N ? v : 0.f;
  };
  f4 acc[2][2];
  mma_tile<true, true>(acc, la, lb, 0, hd.K);
  const Lane ln;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + ln.n(j);
    if (n >= N) continue;
    const float bb = bias[n];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t row = m0 + ln.m(i, q);
        if (row < rows) hg[(row * hd.nh + h) * N + n] = acc[i][j][q] + bb;
      }
  }
}

// part[h, b, :] = U_h[b, :] W_o_h^T; grid (tiles of L, tiles of B, branch)
__global__ void __launch_bounds__(256) half_out_kernel(HalfDev hd, const float* __restrict__ P,
                                                       const float* __restrict__ u, float* __restrict__ part,
                                                       int rows) {
  const int h = blockIdx.z;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int KU = hd.nh * hd.H;
  const float* W = P + hd.base + h * hd.stride + hd.o_wo;
  auto la = [&](int m, int k) -> float {
    const float v = u[int64_t(min(m0 + m, rows - 1)) * KU + h * hd.H + k];
    return m0 + m < rows ? v : 0.f;
  };
  auto lb = [&](int n, int k) -> float {
    const float v = W[int64_t(min(n0 + n, hd.L - 1)) * hd.H + k];
    return n0 + n < hd.L ? v : 0.f;
  };
  f4 acc[2][2];
  mma_tile<true, true>(acc, la, lb, 0, hd.H);
  const Lane ln;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + ln.n(j);
    if (n >= hd.L) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t row = m0 + ln.m(i, q);
        if (row < rows) part[(int64_t(h) * rows + row) * hd.L + n] = acc[i][j][q];
      }
  }
}

// s0[b, n] += sum_h (part[h, b, n] + b_o_h[n]), h ascending: the same bits every run
__global__ void half_sum_kernel(HalfDev hd, const float* __restrict__ P, const float* __restrict__ part,
                                float* __restrict__ s0, int64_t rows) {
  const int64_t n = rows * hd.L;
  for (int64_t e = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; e < n; e += int64_t(gridDim.x) * blockDim.x) {
    const int c = static_cast<int>(e % hd.L);
    float v = s0[e];
    for (int h = 0; h < hd.nh; ++h) v += part[h * n + e] + P[hd.base + h * hd.stride + hd.o_bo + c];
    s0[e] = v;
  }
}

// ------------------------------------------------------------ backward -----
// db_o_h = colsum dS0 [rows, L], the same vector for every h: this workgroup's rows, added to all copies
__global__ void half_colsum_kernel(HalfDev hd, const float* __restrict__ ds0, float* __restrict__ G, int rows,
                                   int rows_per_block) {
  const int64_t r0 = int64_t(blockIdx.x) * rows_per_block;
  const int64_t r1 = min(r0 + rows_per_block, int64_t(rows));
  for (int c = threadIdx.x; c < hd.L; c += blockDim.x) {
    float s = 0.f;
    for (int64_t r = r0; r < r1; ++r) s += ds0[r * hd.L + c];
    for (int h = 0; h < hd.nh; ++h) atomicAdd(G + hd.base + h * hd.stride + hd.o_bo + c, s);
  }
}

// dW_o_h[l, j] += sum_b dS0[b, l] U[b, h, j]; grid (tiles of n_half H, tiles of L, batch splits)
__global__ void __launch_bounds__(256) half_dwo_kernel(HalfDev hd, const float* __restrict__ ds0,
                                                       const float* __restrict__ u, float* __restrict__ G, int rows,
                                                       int k_split) {
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int NU = hd.nh * hd.H;
  const int kb = blockIdx.z * k_split, ke = min(rows, kb + k_split);
  auto la = [&](int m, int k) -> float {
    const float v = ds0[int64_t(k) * hd.L + min(m0 + m, hd.L - 1)];
    return m0 + m < hd.L ? v : 0.f;
  };
  auto lb = [&](int n, int k) -> float {
    const float v = u[int64_t(k) * NU + min(n0 + n, NU - 1)];
    return n0 + n < NU ? v : 0.f;
  };
  f4 acc[2][2];
  mma_tile<false, false>(acc, la, lb, kb, ke);
  const Lane ln;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + ln.n(j);
    if (n >= NU) continue;
    const int h = n / hd.H, jj = n - h * hd.H;
    float* g = G + hd.base + h * hd.stride + hd.o_wo + jj;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int l = m0 + ln.m(i, q);
        if (l < hd.L) atomicAdd(g + int64_t(l) * hd.H, acc[i][j][q]);
      }
  }
}

// dU[b, h, j] = sum_l dS0[b, l] W_o_h[l, j], then dH = dU G silu'(H), dG = dU silu(H) into dHG, and the
// tile's share of cs_h = colsum dHG_h = db_hg_h into the bucket; grid (tiles of n_half H, tiles of B)
__global__ void __launch_bounds__(256) half_du_kernel(HalfDev hd, const float* __restrict__ P,
                                                      const float* __restrict__ ds0, const float* __restrict__ hg,
                                                      float* __restrict__ dhg, float* __restrict__ G, int rows) {
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int NU = hd.nh * hd.H;
  auto la = [&](int m, int k) -> float {
    const float v = ds0[int64_t(min(m0 + m, rows - 1)) * hd.L + k];
    return m0 + m < rows ? v : 0.f;
  };
  auto lb = [&](int n, int k) -> float {
    const int c = min(n0 + n, NU - 1);
    const int h = c / hd.H, j = c - h * hd.H;
    const float v = P[hd.base + h * hd.stride + hd.o_wo + int64_t(k) * hd.H + j];
    return n0 + n < NU ? v : 0.f;
  };
  f4 acc[2][2];
  mma_tile<true, false>(acc, la, lb, 0, hd.L);
  const Lane ln;
  const int H = hd.H;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + ln.n(j);
    const bool col = n < NU;
    const int h = col ? n / H : 0, jj = col ? n - h * H : 0;
    float sh = 0.f, sgt = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t row = m0 + ln.m(i, q);
        if (!col || row >= rows) continue;
        const int64_t o = (row * hd.nh + h) * 2 * H;
        const float hv = hg[o + jj], gv = hg[o + H + jj];
        const float sg = sigmoidf_(hv), d = acc[i][j][q];
        const float dh = d * gv * (sg * (1.f + hv * (1.f - sg))), dg = d * hv * sg;
        dhg[o + jj] = dh;
        dhg[o + H + jj] = dg;
        sh += dh;
        sgt += dg;
      }
    // the 4 lane groups (lane >> 4) hold other rows of the same column
    sh += __shfl_xor(sh, 16, 64);
    sh += __shfl_xor(sh, 32, 64);
    sgt += __shfl_xor(sgt, 16, 64);
    sgt += __shfl_xor(sgt, 32, 64);
    if (col && ln.kq == 0) {
      float* g = G + hd.base + h * hd.stride + hd.o_bhg + jj;
      atomicAdd(g, sh);
      atomicAdd(g + H, sgt);
    }
  }
}

// T_h[n, c] = sum_b dHG[b, h, n] Xhat_h[b, c] over the whole batch, then (cs_h = db_hg_h is
// already in the bucket): dW_hg_h[n, c] = T g_h[c] + cs_h[n] b_h[c],
// dg_h[c] += sum_n W_hg_h[n, c] T[n, c], db_h[c] += sum_n W_hg_h[n, c] cs_h[n];
// grid (tiles of K, tiles of 2H, branch)
__global__ void __launch_bounds__(256) half_dwhg_kernel(HalfDev hd, const float* __restrict__ P,
                                                        const float* __restrict__ xs, const float* __restrict__ stats,
                                                        const float* __restrict__ dhg, float* __restrict__ G,
                                                        int rows) {
  const int h = blockIdx.z, N = 2 * hd.H;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  auto la = [&](int m, int k) -> float {
    const float v = dhg[(int64_t(k) * hd.nh + h) * N + min(m0 + m, N - 1)];
    return m0 + m < N ? v : 0.f;
  };
  auto lb = [&](int n, int k) -> float {
    const float* st = stats + (int64_t(k) * hd.nh + h) * 2;
    const float v = (xs[int64_t(k) * hd.d_in + src_col(hd, h, min(n0 + n, hd.K - 1))] - st[0]) * st[1];
    return n0 + n < hd.K ? v : 0.f;
  };
  f4 acc[2][2];
  mma_tile<false, false>(acc, la, lb, 0, rows);
  const Lane ln;
  const int64_t ob = hd.base + h * hd.stride;
  const float *gam = P + ob, *bet = P + ob + hd.o_b, *W = P + ob + hd.o_whg;
  const float* cs = G + ob + hd.o_bhg;
  float* dW = G + ob + hd.o_whg;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = n0 + ln.n(j);
    const bool col = c < hd.K;
    const float gc = col ? gam[c] : 0.f, bc = col ? bet[c] : 0.f;
    float pg = 0.f, pb = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = m0 + ln.m(i, q);
        if (!col || n >= N) continue;
        const float t = acc[i][j][q], csn = cs[n], w = W[int64_t(n) * hd.K + c];
        dW[int64_t(n) * hd.K + c] = t * gc + csn * bc;
        pg += w * t;
        pb += w * csn;
      }
    // the 4 lane groups (lane >> 4) hold other rows of the same column
    pg += __shfl_xor(pg, 16, 64);
    pg += __shfl_xor(pg, 32, 64);
    pb += __shfl_xor(pb, 16, 64);
    pb += __shfl_xor(pb, 32, 64);
    if (col && ln.kq == 0) {
      atomicAdd(G + ob + c, pg);
      atomicAdd(G + ob + hd.o_b + c, pb);
    }
  }
}

HalfDev half_dev(const hbk_mlp_plan& p) {
  HalfDev hd{};
  const HalfDims& d = p.half;
  const HalfOffsets& o = p.half_off;
  hd.d_in = d.d_in;
  hd.chunk = d.chunk();
  hd.per = d.per();
  hd.K = d.k();
  hd.H = d.hid;
  hd.L = d.layer;
  hd.nh = d.n_half;
  hd.n_tokens = d.n_tokens;
  hd.base = o.base;
  hd.stride = o.stride;
  hd.o_b = o.b;
  hd.o_whg = o.w_hg;
  hd.o_bhg = o.b_hg;
  hd.o_wo = o.w_o;
  hd.o_bo = o.b_o;
  for (size_t i = 0; i < p.half_idx.size() && i < size_t(kHalfMaxIdx); ++i)
    hd.tok[i] = static_cast<unsigned char>(p.half_idx[i]);
  return hd;
}

inline dim3 d3(const HalfGrid& g) { return dim3(g.x, g.y, g.z); }

}  // namespace

int mlp_half_forward(const hbk_mlp_plan& p, const float* params, const float* x, int B, float* s0, float* ws,
                     float drop_p, uint64_t seed, const double* step_sc, hipStream_t s) {
  const HalfDev hd = half_dev(p);
  const HalfWs w = half_ws_layout(p.half, B);
  const HalfGrids g = half_grids(p.half, B);
  float* xd = drop_p > 0.f ? ws + w.xd : nullptr;  // the dropped-out input, when it differs from x
  const float* xs = xd ? xd : x;
  hipLaunchKernelGGL(half_stats_kernel, d3(g.stats), dim3(256), 0, s, hd, x, ws + w.stats, xd, B, drop_p, seed,
                     step_sc);
  HBK_LAUNCH_CHECK("half_stats_kernel");
  hipLaunchKernelGGL(half_hg_kernel, d3(g.hg), dim3(256), 0, s, hd, params, xs, ws + w.stats, ws + w.hg, B);
  HBK_LAUNCH_CHECK("half_hg_kernel");
  // (B n_half <= 2^20 * 256 rows: hbk_mlp_forward / hbk_mlp_train_fwd_bwd bound a half plan's batch)
  const int rc = mlp_gate_forward(ws + w.hg, ws + w.u, B * hd.nh, hd.H, s);
  if (rc != HBK_OK) return rc;
  hipLaunchKernelGGL(half_out_kernel, d3(g.out), dim3(256), 0, s, hd, params, ws + w.u, ws + w.part, B);
  HBK_LAUNCH_CHECK("half_out_kernel");
  hipLaunchKernelGGL(half_sum_kernel, d3(g.sum), dim3(256), 0, s, hd, params, ws + w.part, s0, int64_t(B));
  HBK_LAUNCH_CHECK("half_sum_kernel");
  return HBK_OK;
}

int mlp_half_backward(const hbk_mlp_plan& p, const float* params, const float* x, int B, const float* ds0,
                      float* G, float* ws, float drop_p, hipStream_t s) {
  const HalfDev hd = half_dev(p);
  const HalfWs w = half_ws_layout(p.half, B);
  const HalfGrids g = half_grids(p.half, B);
  hipLaunchKernelGGL(half_colsum_kernel, d3(g.cs), dim3(128), 0, s, hd, ds0, G, B, g.cs_rows);
  HBK_LAUNCH_CHECK("half_colsum_kernel");
  hipLaunchKernelGGL(half_dwo_kernel, d3(g.dwo), dim3(256), 0, s, hd, ds0, ws + w.u, G, B, g.dwo_k_split);
  HBK_LAUNCH_CHECK("half_dwo_kernel");
  hipLaunchKernelGGL(half_du_kernel, d3(g.du), dim3(256), 0, s, hd, params, ds0, ws + w.hg, ws + w.dhg, G, B);
  HBK_LAUNCH_CHECK("half_du_kernel");
  // (the forward of this step left the dropped-out input in the workspace)
  hipLaunchKernelGGL(half_dwhg_kernel, d3(g.dwhg), dim3(256), 0, s, hd, params, drop_p > 0.f ? ws + w.xd : x,
                     ws + w.stats, ws + w.dhg, G, B);
  HBK_LAUNCH_CHECK("half_dwhg_kernel");
  return HBK_OK;
}

}  // namespace hbk
