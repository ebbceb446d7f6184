// Stand-alone check of the generic classifier path's layout and launch geometry
// (hbk_mlp_layout.h), run by tests/test_mlp_layout.py as a child process built with
// -fsanitize=address,undefined. For (d_in, layer, hid, n_layers) = (1536, 96, 64, 0..3),
// (1536, 32, 24, 1) and (40, 8, 5, 0), gated and plain, and the two half plans of the golden
// file, at B in {1, 17, 300, 1100}, it asserts with arithmetic of its own: the parameter blocks
// tile [0, n_params) in forward order; the workspace regions are aligned, disjoint and end at
// `total`; every GEMM the forward and the backward issue gets a grid that covers its output and a
// split of K without an empty or a short part; the row, column and element-wise grids cover
// their work. Then it prints one line per plan and one per (plan, B) for the test to compare.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "hbk_mlp_layout.h"

using namespace hbk;

namespace {

int g_failed = 0;
struct Case {
  int d_in, layer, hid, n_layers;
  bool gated, half;
};
#define CHECK(cond)                                                                                     \
  do {                                                                                                  \
    if (!(cond)) {                                                                                      \
      fprintf(stderr, "mlp_layout_check: %s fails (%d %d %d %d gated %d half %d, B %d)\n", #cond, c.d_in, \
              c.layer, c.hid, c.n_layers, int(c.gated), int(c.half), int(B));                           \
      ++g_failed;                                                                                       \
    }                                                                                                   \
  } while (0)

int64_t up64(int64_t n) { return (n + 63) / 64 * 64; }
bool covers(int64_t blocks, int64_t per, int64_t n) {  // blocks of `per` cover n with no spare block
  return blocks * per >= n && (blocks - 1) * per < n;
}

MlpParams check_params(const Case& c) {
  const int64_t B = 0;
  const MlpParams p = mlp_param_layout(c.d_in, c.layer, c.hid, c.n_layers, c.gated);
  const int wid = c.gated ? 2 * c.hid : c.hid;
  CHECK(int(p.g.size()) == c.n_layers + 2 && int(p.ln.size()) == c.n_layers + 1);
  // forward order: norm_in, mlp_in, then (LayerNorm, block) per hidden layer and for the output
  std::vector<std::pair<int64_t, int64_t>> runs;  // (offset, floats)
  runs.push_back({p.ln_in.g, c.d_in});
  runs.push_back({p.ln_in.b, c.d_in});
  CHECK(p.ln_in.d == c.d_in);
  for (size_t k = 0; k < p.g.size(); ++k) {
    const Gmlp& g = p.g[k];
    if (k > 0) {
      const Ln& l = p.ln[k - 1];
      CHECK(l.d == c.layer);
      runs.push_back({l.g, c.layer});
      runs.push_back({l.b, c.layer});
    }
    CHECK(g.in == (k == 0 ? c.d_in : c.layer) && g.hid == c.hid && g.wid == wid);
    CHECK(g.out == (k + 1 == p.g.size() ? 1 : c.layer));
    runs.push_back({g.w_hg, int64_t(wid) * g.in});
    runs.push_back({g.b_hg, wid});
    runs.push_back({g.w_o, int64_t(g.out) * c.hid});
    runs.push_back({g.b_o, g.out});
  }
  int64_t end = 0;
  for (const auto& r : runs) {
    CHECK(r.first == end);
    end = r.first + r.second;
  }
  CHECK(end == p.n_params);
  if (c.d_in == 1536 && c.layer == 96 && c.hid == 64 && c.n_layers == 2) CHECK(p.n_params == (c.gated ? 256417 : 139425));
  printf("params %d %d %d %d %d %d | %lld |", c.d_in, c.layer, c.hid, c.n_layers, int(c.gated), int(c.half),
         (long long)p.n_params);
  // (the order of hbk_mlp_layout: ln_in, every block, then every LayerNorm)
  printf(" %lld %lld", (long long)p.ln_in.g, (long long)p.ln_in.b);
  for (const Gmlp& g : p.g) printf(" %lld %lld %lld %lld", (long long)g.w_hg, (long long)g.b_hg, (long long)g.w_o, (long long)g.b_o);
  for (const Ln& l : p.ln) printf(" %lld %lld", (long long)l.g, (long long)l.b);
  printf("\n");
  return p;
}

struct Gemm {
  int M, N, K;
  bool contiguous, acc, may_split;
};

void check_gemm(const Case& c, int64_t B, const Gemm& q) {
  const GemmLaunch g = gemm_launch(q.M, q.N, q.K, q.contiguous, q.acc, q.may_split);
  const int64_t splits = g.grid.z;
  CHECK(covers(g.grid.x, 64, q.N) && covers(g.grid.y, 64, q.M));
  CHECK(g.grid.y <= 65535 && g.grid.z >= 1 && g.grid.z <= 65535);
  CHECK(g.k_split >= 16 && g.k_split % 16 == 0);
  CHECK(splits * g.k_split >= q.K && (splits - 1) * g.k_split < q.K);  // K covered, no empty split
  if (splits > 1) {
    CHECK(q.may_split && (q.contiguous || q.acc));
    CHECK(q.K / splits >= 16);  // never below 16 K rows per split
  }
  CHECK(g.memset_c == (splits > 1 && !q.acc));
  printf(" %d,%d,%d,%d:%u,%u,%u,%d,%d", q.M, q.N, q.K, int(q.acc), g.grid.x, g.grid.y, g.grid.z, g.k_split,
         int(g.memset_c));
}

void check_batch(const Case& c, const MlpParams& p, int64_t B) {
  HalfDims hd;
  if (c.half) {
    hd.d_in = c.d_in;
    hd.layer = c.layer;
    hd.hid = c.hid;
    hd.n_tokens = 16;
    hd.n_half = 16;
  }
  const int wid = c.gated ? 2 * c.hid : c.hid;
  // workspace
  const Ws w = ws_layout(p, hd, B);
  std::vector<std::pair<int64_t, int64_t>> reg;  // (start, floats)
  reg.push_back({w.xn_in, B * c.d_in});
  reg.push_back({w.xhat_in, B * c.d_in});
  reg.push_back({w.rstd_in, B});
  CHECK(w.hg.size() == p.g.size() && w.u.size() == p.g.size() && w.s.size() == p.g.size());
  CHECK(w.xn.size() == p.ln.size() && w.xhat.size() == p.ln.size() && w.rstd.size() == p.ln.size());
  for (size_t k = 0; k < p.g.size(); ++k) {
    reg.push_back({w.hg[k], B * wid});
    reg.push_back({w.u[k], B * c.hid});
    reg.push_back({w.s[k], B * p.g[k].out});
  }
  for (size_t k = 0; k < p.ln.size(); ++k) {
    reg.push_back({w.xn[k], B * c.layer});
    reg.push_back({w.xhat[k], B * c.layer});
    reg.push_back({w.rstd[k], B});
  }
  CHECK(w.z == w.s.back());
  reg.push_back({w.dz, B});
  reg.push_back({w.prob, B});
  // the backward's two turn-about buffers hold dU [B, hid], dX [B, in] and dx [B, layer]
  const int64_t turn = B * std::max({c.d_in, c.layer, wid});
  reg.push_back({w.dtmp_a, turn});
  reg.push_back({w.dtmp_b, turn});
  reg.push_back({w.dhg, B * wid});
  reg.push_back({w.half, c.half ? half_ws_layout(hd, B).total : 0});
  std::sort(reg.begin(), reg.end());
  int64_t end = 0;
  for (size_t i = 0; i < reg.size(); ++i) {
    CHECK(reg[i].first >= 0 && reg[i].first % 64 == 0);
    if (i + 1 < reg.size()) CHECK(reg[i].first + reg[i].second <= reg[i + 1].first);  // disjoint
    end = std::max(end, reg[i].first + up64(reg[i].second));
  }
  CHECK(reg.front().first == 0 && w.total == end);
  // rows, columns, elements
  const RowGrids rg = mlp_row_grids(int(B));
  CHECK(covers(rg.ln, 4, B));
  CHECK(rg.loss >= 1 && rg.loss <= 64 && (B > 64 * 256 || covers(rg.loss, 256, B)));
  CHECK(rg.rpb == (B <= 1024 ? 4 : 5) && covers(rg.cs, rg.rpb, B));
  for (int64_t n : {B, B * c.hid, B * 16 * c.hid, p.n_params, int64_t(4096) * 256 + 1}) {
    const unsigned e = mlp_ew_grid(n);
    CHECK(e >= 1 && e <= 4096 && (n > 4096 * 256 ? e == 4096 : covers(e, 256, n)));
  }
  // the bank's gate runs through mlp_gate_forward on the element-wise grid: the one its own planner names
  if (c.half) CHECK(mlp_ew_grid(B * hd.n_half * hd.hid) == half_grids(hd, B).gate.x);
  printf("batch %d %d %d %d %d %d %lld | %lld | %u %u %d %u |", c.d_in, c.layer, c.hid, c.n_layers, int(c.gated),
         int(c.half), (long long)B, (long long)w.total, rg.ln, rg.loss, rg.rpb, rg.cs);
  // the GEMMs of forward() and of the backward loop, block by block
  const int b = int(B);
  for (const Gmlp& g : p.g) {
    check_gemm(c, B, {b, g.wid, g.in, true, false, !c.half});   // HG = in W_hg^T
    check_gemm(c, B, {b, g.out, g.hid, true, false, !c.half});  // S = U W_o^T
    check_gemm(c, B, {g.out, g.hid, b, true, true, true});      // dW_o = dS^T U, into the bucket
    check_gemm(c, B, {b, g.hid, g.out, true, false, true});     // dU = dS W_o
    check_gemm(c, B, {g.wid, g.in, b, true, true, true});       // dW_hg = dHG^T X, into the bucket
    check_gemm(c, B, {b, g.in, g.wid, true, false, true});      // dX = dHG W_hg
  }
  printf("\n");
  // a strided C that is not accumulated into, and a caller that forbids it, never split
  CHECK(gemm_launch(b, c.hid, 4096, false, false, true).grid.z == 1);
  CHECK(gemm_launch(b, c.hid, 4096, true, true, false).grid.z == 1);
  CHECK(gemm_launch(c.hid, c.hid, 4096, false, true, true).grid.z > 1);
}

}  // namespace

int main() {
  std::vector<Case> cases;
  for (int gated = 1; gated >= 0; --gated) {
    for (int L = 0; L <= 3; ++L) cases.push_back({1536, 96, 64, L, gated != 0, false});
    cases.push_back({1536, 32, 24, 1, gated != 0, false});
    cases.push_back({40, 8, 5, 0, gated != 0, false});
  }
  cases.push_back({1536, 96, 64, 2, true, true});
  cases.push_back({1536, 32, 24, 1, true, true});
  for (const Case& c : cases) {
    const MlpParams p = check_params(c);
    for (int64_t B : {1, 17, 300, 1100}) check_batch(c, p, B);
  }
  return g_failed ? 1 : 0;
}
