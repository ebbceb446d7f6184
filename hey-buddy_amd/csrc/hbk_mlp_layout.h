// Layout and launch geometry of the classifier's generic path (hbk_mlp.hip), host-only: the
// flat parameter buffer, the workspace regions and every launch grid follow from the dims and
// the batch alone, so a stand-alone program can check them (tests/mlp_layout_check.cpp). No HIP
// header is needed here. The half-layer bank's own geometry is in hbk_mlp_half_plan.h, the fused
// step's in hbk_mlp_plan.h.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hbk_mlp_half_plan.h"

namespace hbk {

// ------------------------------------------------------------ parameters ----
struct Gmlp {
  int in, hid, out;
  int64_t w_hg, b_hg, w_o, b_o;  // float offsets into the flat parameter buffer
  // rows of W_hg = columns of HG: 2 hid (hidden rows then gate rows), or hid in a plain plan
  // (hbk_mlp_plan_create_ex with gated = 0: W_hg / b_hg are hidden.weight / hidden.bias alone)
  int wid = 0;
};
struct Ln {
  int d;
  int64_t g, b;
};

// One flat f32 buffer, blocks in the order of the forward pass:
//   ln_in  norm_in.{weight, bias}                          [d_in] x 2
//   g[0]   mlp_in:  W_hg [wid, d_in], b_hg [wid], W_o [layer, hid], b_o [layer]
//   per hidden layer l: ln[l] [layer] x 2, then g[l + 1] (layer -> hid -> layer)
//   ln[n_layers]  norm_out [layer] x 2, then g[n_layers + 1] = mlp_out (layer -> hid -> 1)
// wid = 2 hid when gated (rows 0..hid-1 hidden.weight, hid..2 hid-1 gate.weight), else hid.
struct MlpParams {
  Ln ln_in{};
  std::vector<Gmlp> g;  // mlp_in, layers..., mlp_out
  std::vector<Ln> ln;   // layers' LNs..., norm_out
  int64_t n_params = 0;
};

inline MlpParams mlp_param_layout(int d_in, int layer, int hid, int n_layers, bool gated) {
  MlpParams p;
  const int wid = gated ? 2 * hid : hid;
  int64_t o = 0;
  p.ln_in = Ln{d_in, o, o + d_in};
  o += 2 * int64_t(d_in);
  auto add_gmlp = [&](int in, int out) {
    Gmlp gm{in, hid, out, 0, 0, 0, 0, wid};
    gm.w_hg = o; o += int64_t(wid) * in;
    gm.b_hg = o; o += wid;
    gm.w_o = o; o += int64_t(out) * hid;
    gm.b_o = o; o += out;
    p.g.push_back(gm);
  };
  auto add_ln = [&](int d) {
    p.ln.push_back(Ln{d, o, o + d});
    o += 2 * int64_t(d);
  };
  add_gmlp(d_in, layer);
  for (int l = 0; l < n_layers; ++l) {
    add_ln(layer);
    add_gmlp(layer, layer);
  }
  add_ln(layer);
  add_gmlp(layer, 1);
  p.n_params = o;
  return p;
}

// ------------------------------------------------------------- workspace ----
// Workspace of the generic path for a batch of B rows (float offsets, every region 64-float
// aligned); the forward keeps its activations there for the backward.
struct Ws {
  int64_t xn_in, xhat_in, rstd_in;  // [B, D_in] x2, [B]
  std::vector<int64_t> hg, u, s;    // per GMLP: [B,wid], [B,H], [B,out]
  std::vector<int64_t> xn, xhat, rstd;  // per LN (layers + norm_out): [B,L], [B,L], [B]
  int64_t z, dz, prob, dtmp_a, dtmp_b, dhg, half, total;  // half: the bank's own region (half_ws_layout)
};

inline Ws ws_layout(const MlpParams& p, const HalfDims& half, int64_t B) {
  Ws w;
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t r = o; o += (n + 63) & ~int64_t(63); return r; };
  const int64_t d_in = p.ln_in.d, layer = p.g.front().out;
  w.xn_in = take(B * d_in);
  w.xhat_in = take(B * d_in);
  w.rstd_in = take(B);
  for (const auto& gm : p.g) {
    w.hg.push_back(take(B * gm.wid));
    w.u.push_back(take(B * gm.hid));
    w.s.push_back(take(B * gm.out));
  }
  for (const auto& l : p.ln) {
    w.xn.push_back(take(B * l.d));
    w.xhat.push_back(take(B * l.d));
    w.rstd.push_back(take(B));
  }
  w.z = w.s.back();
  w.dz = take(B);
  w.prob = take(B);
  const int64_t wid = p.g.front().wid;  // every block's Gmlp::wid
  const int64_t wide = std::max<int64_t>(d_in, wid);
  w.dtmp_a = take(B * std::max<int64_t>(wide, layer));
  w.dtmp_b = take(B * std::max<int64_t>(wide, layer));
  w.dhg = take(B * wid);
  w.half = take(half.n_half > 0 ? half_ws_layout(half, B).total : 0);
  w.total = o;
  return w;
}

// ------------------------------------------------------- launch geometry ----
struct MlpGrid {
  unsigned x, y, z;
};

// gemm_kernel: one workgroup per 64 x 64 tile of C [M, N], its depth K staged 16 rows at a time.
constexpr int kGemmTileM = 64, kGemmTileN = 64, kGemmTileK = 16;

// grid (tiles of N, tiles of M, splits of K). Split-K when the output has too few tiles to fill
// the chip (the weight gradients: K = batch; the input layer: K = 1536), >= 16 K rows per split:
// split z covers K rows [z k_split, (z + 1) k_split) and adds its partial product with atomics,
// so C must be contiguous (the memset below) or accumulated into (the caller zeroed it).
struct GemmLaunch {
  MlpGrid grid;
  int k_split;    // a multiple of kGemmTileK
  bool memset_c;  // zero C [M, N] first: split-K into a C that is not accumulated into
};

inline GemmLaunch gemm_launch(int M, int N, int K, bool contiguous, bool acc, bool may_split) {
  GemmLaunch g{};
  g.grid.x = (N + kGemmTileN - 1) / kGemmTileN;
  g.grid.y = (M + kGemmTileM - 1) / kGemmTileM;
  int splits = 1;
  const int tiles = int(g.grid.x * g.grid.y);
  if (may_split && tiles < 256 && K >= 256 && (contiguous || acc)) splits = std::min(std::max(1, 512 / tiles), K / 16);
  g.k_split = ((K + splits - 1) / splits + kGemmTileK - 1) / kGemmTileK * kGemmTileK;
  splits = (K + g.k_split - 1) / g.k_split;
  g.grid.z = splits;
  g.memset_c = splits > 1 && !acc;
  return g;
}

// Grid of an elementwise grid-stride kernel over n elements, 256 threads per block
inline unsigned mlp_ew_grid(int64_t n) { return static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 4096)); }

// The launches whose grid follows from the batch alone.
struct RowGrids {
  unsigned ln;    // ln_fwd_kernel: one wave per row, 4 rows per 256-thread workgroup
  unsigned loss;  // loss_kernel: grid-stride over the rows, at most 64 workgroups of 256
  // the column reductions (colsum_kernel, ln_bwd_kernel: LN dgamma / dbeta, bias gradients): rpb rows
  // per workgroup, ~256 workgroups at the stage batch sizes (32 rows gave 35 workgroups at B = 1100)
  int rpb;
  unsigned cs;
};

inline RowGrids mlp_row_grids(int B) {
  RowGrids g{};
  g.ln = (B + 3) / 4;
  g.loss = std::min<unsigned>((B + 255) / 256, 64);
  g.rpb = std::max(4, (B + 255) / 256);
  g.cs = (B + g.rpb - 1) / g.rpb;
  return g;
}

}  // namespace hbk
