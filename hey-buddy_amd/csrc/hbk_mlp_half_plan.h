// Geometry of the classifier's half-layer bank (hbk_mlp_half.hip), host-only: parameter
// offsets, workspace layout and launch grids follow from the dims alone, so a stand-alone
// program can check them (tests/half_plan_check.cpp). No HIP header is needed here.
//
// The bank: n_half branches LayerNorm(K) -> gated MLP(K -> hid -> layer), K = d_in / 2; branch
// h reads n_tokens / 2 of the n_tokens chunks (each d_in / n_tokens wide) of a flattened
// input row, in the order its index list names them.
#pragma once

#include <stdint.h>

namespace hbk {

constexpr int kHalfTile = 64;   // rows and columns of one workgroup's output tile
constexpr int kHalfTileK = 64;  // depth of one staged slice (16 loads in flight per thread and operand)
constexpr int kHalfMaxTokens = 64;
constexpr int kHalfMaxIdx = 256;  // n_half * (n_tokens / 2): the index table travels as a kernel argument

struct HalfDims {
  int d_in = 0, layer = 0, hid = 0, n_tokens = 0, n_half = 0;
  int chunk() const { return d_in / n_tokens; }  // width of one token
  int per() const { return n_tokens / 2; }       // tokens per branch
  int k() const { return d_in / 2; }             // features per branch
};

// 0 when the dims and the n_half * (n_tokens / 2) token indices describe a bank, else the
// number of the rule they break (hbk_mlp_plan_create_half turns it into a message)
inline int half_validate(const HalfDims& d, const int32_t* idx) {
  if (d.d_in <= 0 || d.layer <= 0 || d.hid <= 0 || d.n_half <= 0) return 1;
  if (d.n_tokens <= 0 || d.n_tokens > kHalfMaxTokens || d.n_tokens % 2 != 0) return 2;
  if (d.d_in % d.n_tokens != 0) return 3;
  if (!idx) return 4;
  if (d.n_half * d.per() > kHalfMaxIdx) return 6;
  for (int i = 0; i < d.n_half * d.per(); ++i)
    if (idx[i] < 0 || idx[i] >= d.n_tokens) return 5;
  return 0;
}

// Parameters of the bank, appended to the flat buffer at `base`; branch h owns the run
// [base + h * stride, base + (h + 1) * stride) and inside it, in this order:
//   g, b      [K] x 2   LayerNorm weight, bias (columns in the gathered order)
//   w_hg      [2 hid, K] rows 0..hid-1 hidden.weight, hid..2 hid-1 gate.weight
//   b_hg      [2 hid]    hidden.bias, gate.bias
//   w_o       [layer, hid], b_o [layer]
struct HalfOffsets {
  int64_t base, stride, g, b, w_hg, b_hg, w_o, b_o;  // g .. b_o relative to the branch's run
  int64_t total;                                     // floats of the whole bank
};

inline HalfOffsets half_offsets(const HalfDims& d, int64_t base) {
  HalfOffsets o{};
  const int64_t K = d.k();
  o.base = base;
  o.g = 0;
  o.b = K;
  o.w_hg = 2 * K;
  o.b_hg = o.w_hg + int64_t(2) * d.hid * K;
  o.w_o = o.b_hg + 2 * d.hid;
  o.b_o = o.w_o + int64_t(d.layer) * d.hid;
  o.stride = o.b_o + d.layer;
  o.total = o.stride * d.n_half;
  return o;
}

// Workspace of the bank for B rows (floats from the bank's base, every region 64-float aligned):
//   stats [B, n_half, 2]     mean, 1 / sqrt(var + eps) of each (row, branch)
//   hg    [B, n_half, 2 hid] pre-activations, kept for the backward
//   u     [B, n_half, hid]   silu(h) * g, kept for the backward
//   dhg   [B, n_half, 2 hid] backward only
//   xd    [B, d_in]          the dropped-out input (written only when dropout is on)
//   part  [n_half, B, layer] each branch's output product, summed onto s0 in a fixed order
struct HalfWs {
  int64_t stats, hg, u, dhg, xd, part, total;
};

inline HalfWs half_ws_layout(const HalfDims& d, int64_t B) {
  HalfWs w{};
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t r = o; o += (n + 63) & ~int64_t(63); return r; };
  const int64_t rows = B * d.n_half;
  w.stats = take(rows * 2);
  w.hg = take(rows * 2 * d.hid);
  w.u = take(rows * d.hid);
  w.dhg = take(rows * 2 * d.hid);
  w.xd = take(B * d.d_in);
  w.part = take(rows * d.layer);
  w.total = o;
  return w;
}

struct HalfGrid {
  unsigned x, y, z;
};
// One launch each; x tiles the output's columns, y its rows, z the branches or the batch splits.
struct HalfGrids {
  HalfGrid stats;  // one workgroup per row
  HalfGrid hg;     // HG_h = Xn_h W_hg_h^T: (2 hid, B, n_half)
  HalfGrid gate;   // element-wise over [B n_half, hid]: what mlp_gate_forward launches gate_fwd_kernel with
  HalfGrid out;    // part_h = U_h W_o_h^T: (layer, B, n_half)
  HalfGrid sum;    // s0 += sum_h part_h + b_o_h: element-wise over [B, layer]
  HalfGrid dwo;    // dW_o = dS0^T U: (n_half hid, layer, batch splits)
  HalfGrid du;     // dU = dS0 W_o, then the gate's backward: (n_half hid, B, 1)
  HalfGrid cs;     // column sums of dS0: row chunks
  HalfGrid dwhg;   // T_h = dHG_h^T Xhat_h and its epilogue: (K, 2 hid, n_half)
  int dwo_k_split;  // batch rows per split of dwo (a multiple of kHalfTileK)
  int cs_rows;      // rows per workgroup of cs
};

inline unsigned half_tiles(int64_t n) { return static_cast<unsigned>((n + kHalfTile - 1) / kHalfTile); }

inline HalfGrids half_grids(const HalfDims& d, int64_t B) {
  HalfGrids g{};
  const int64_t nh = d.n_half;
  g.stats = {static_cast<unsigned>(B), 1, 1};
  g.hg = {half_tiles(2 * d.hid), half_tiles(B), static_cast<unsigned>(nh)};
  const int64_t ew = (B * nh * d.hid + 255) / 256;
  g.gate = {static_cast<unsigned>(ew < 4096 ? ew : 4096), 1, 1};
  g.out = {half_tiles(d.layer), half_tiles(B), static_cast<unsigned>(nh)};
  const int64_t sm = (B * d.layer + 255) / 256;
  g.sum = {static_cast<unsigned>(sm < 4096 ? sm : 4096), 1, 1};
  // dW_o has few tiles: split the batch so that about 256 workgroups run, >= 64 rows each
  const int64_t tiles = int64_t(half_tiles(nh * d.hid)) * half_tiles(d.layer);
  int64_t splits = tiles < 256 ? (256 + tiles - 1) / tiles : 1;
  if (splits > (B + 63) / 64) splits = (B + 63) / 64;
  if (splits < 1) splits = 1;
  int64_t ks = ((B + splits - 1) / splits + kHalfTileK - 1) / kHalfTileK * kHalfTileK;
  if (ks < kHalfTileK) ks = kHalfTileK;
  g.dwo_k_split = static_cast<int>(ks);
  g.dwo = {half_tiles(nh * d.hid), half_tiles(d.layer), static_cast<unsigned>((B + ks - 1) / ks)};
  g.du = {half_tiles(nh * d.hid), half_tiles(B), 1};
  // about 64 workgroups: each adds its sums to all n_half copies of db_o with atomics
  const int64_t rpb = (B + 63) / 64 > 4 ? (B + 63) / 64 : 4;
  g.cs_rows = static_cast<int>(rpb);
  g.cs = {static_cast<unsigned>((B + rpb - 1) / rpb), 1, 1};
  g.dwhg = {half_tiles(d.k()), half_tiles(2 * d.hid), static_cast<unsigned>(nh)};
  return g;
}

}  // namespace hbk
