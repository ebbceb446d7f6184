// Stand-alone check of the fused train step's planning (hbk_mlp_plan.h), run by
// tests/test_step_plan.py as a child process built with -fsanitize=address,undefined.
// For every row of a grid of (knobs, B, NG, CUs) it asserts the plan's invariants and
// prints the plan as integers; the test compares the output with the table recorded
// from the tree before the planning was split out (tests/golden/step_plan_parent.json).
#include <cstdio>
#include <vector>

#include "hbk_mlp_plan.h"

using namespace hbk;

namespace {

// hbk_mlp_plan_create's parameter layout for NG gated MLPs (n_layers = NG - 2)
int64_t n_params_of(int NG) {
  int64_t o = 2 * int64_t(kD);
  auto gmlp = [&](int in, int out) { o += int64_t(2) * kH * in + 2 * kH + int64_t(out) * kH + out; };
  gmlp(kD, kL);
  for (int l = 0; l < NG - 2; ++l) {
    o += 2 * kL;
    gmlp(kL, kL);
  }
  o += 2 * kL;
  gmlp(kL, 1);
  return o;
}

int g_failed = 0;
#define CHECK(cond)                                                                                     \
  do {                                                                                                  \
    if (!(cond)) {                                                                                      \
      fprintf(stderr, "step_plan_check: %s fails (knobs %d, B %d, NG %d, CUs %d)\n", #cond, knob, B, NG, cus); \
      ++g_failed;                                                                                       \
    }                                                                                                   \
  } while (0)

void invariants(const StepPlan& pl, int knob, int B, int NG, int cus, int64_t n_params) {
  const FusedWs& w = pl.ws;
  const int64_t Bp = pl.Bp;
  CHECK(Bp % kR == 0 && Bp >= B && Bp - B < kR && pl.rt == Bp / kR);
  // the layout: regions ascend, 64-float aligned, and each holds its array
  const int64_t off[] = {w.wsplit, w.part,     w.hg_part,  w.xhat[0], w.xhat[1], w.U,    w.Xn,   w.dS,
                         w.dHG,    w.rinfo[0], w.rinfo[1], w.mask[0], w.mask[1], w.maxS, w.total};
  const int64_t size[] = {wsplit_halves(NG) / 2, w.pstride * part_slabs(Bp), int64_t(24) * B * kH2, Bp * kD, Bp * kD,
                          int64_t(NG) * Bp * kH, int64_t(NG) * Bp * kL, int64_t(NG) * Bp * kL, int64_t(NG) * Bp * kH2,
                          Bp * 4, Bp * 4, Bp * kMaskW, Bp * kMaskW, maxs_floats(NG, pl.rt)};
  int64_t need = 0;  // the arrays (and k3s's overread) packed at 64-float granularity, summed here on its own
  for (int i = 0; i < 14; ++i) {
    CHECK(off[i] % 64 == 0 && off[i] >= 0);
    CHECK(off[i] + size[i] <= off[i + 1]);
    if (i >= 5 && i <= 8) CHECK(off[i] + size[i] + kK3sMaxR <= off[i + 1]);  // k3s reads past U, Xn, dS, dHG
    need += (size[i] + (i >= 5 && i <= 8 ? kK3sMaxR : 0) + 63) / 64 * 64;
  }
  CHECK(w.pstride >= n_params && w.pstride % 64 == 0);
  CHECK(w.total == need);  // what mlp_fused_ws_floats reports: no more than the arrays need
  const FusedFixed f = fused_fixed(NG, n_params);  // what the update finds without B
  CHECK(w.wsplit == f.wsplit && w.part == f.part && w.pstride == f.pstride);
  // every split count a launch can take fits the slabs (and the HG0 partials their 24)
  const int64_t slabs = part_slabs(Bp);
  CHECK(k3_splits(Bp, true) <= slabs && k3_splits(Bp, false) <= slabs);
  CHECK(pl.slabs <= slabs && pl.S0 <= slabs && pl.S1 <= slabs);
  CHECK(pl.KS >= 1 && pl.KS <= 24);
  // the job table
  CHECK(pl.n_jobs == 2 * NG && pl.n_jobs <= kMaxJobs);
  int wgs = 0;
  for (int i = 0; i < pl.n_jobs; ++i) {
    CHECK(pl.job_start[i] == wgs && pl.job_tiles[i] >= 1 && pl.job_splits[i] >= 1 && pl.job_splits[i] <= pl.slabs);
    wgs += pl.job_tiles[i] * pl.job_splits[i];
  }
  CHECK(pl.job_start[pl.n_jobs] == wgs);
  if (pl.variant == 2) {
    CHECK(pl.k3s_pair >= 0 && pl.k3s_pair < kK3sNPairs);
    CHECK(int64_t(pl.S0) * 32 * kK3sPairs[pl.k3s_pair][0] >= Bp && int64_t(pl.S1) * 32 * kK3sPairs[pl.k3s_pair][1] >= Bp);
    CHECK(pl.job_splits[0] == pl.S0 && pl.job_splits[1] == pl.S1 && pl.S1 <= pl.S0 && pl.slabs == pl.S0);
    CHECK(pl.rt <= kK3sMaxTiles || !pl.sparse);
    if (knob != 7) CHECK(pl.sparse == (pl.rt <= kK3sMaxTiles ? 1 : 0));  // (7: HBK_STEP_DENSE)
    CHECK(pl.k1c.RT >= 1 && pl.k1c.RT <= k1c_rtmax(pl.k1c.KC) && pl.k1c.KC * pl.k1c.KS == kD);
    CHECK(pl.k1c.blocks == (B + 16 * pl.k1c.RT - 1) / (16 * pl.k1c.RT) * pl.k1c.KS);
    CHECK(pl.KS == pl.k1c.KS && pl.k1_grid == pl.k1c.blocks);
  } else {
    CHECK(pl.variant == 1 && int64_t(pl.slabs) * pl.k3_rows >= Bp);
    CHECK(pl.k1_grid == k1_blocks(B) * pl.KS && k1_blocks(B) * kRB >= B);
  }
  // k2's prefetch workgroups cover every row tile of the next step
  CHECK(pl.pre_tiles >= 1 && pl.k2_grid == pl.rt && (pl.k2_grid_pre - pl.rt) * pl.pre_tiles >= pl.rt);
}

void print_row(const StepPlan& pl, int knob, int B, int NG, int cus, int64_t n_params, bool first) {
  std::vector<long long> v = {knob, B, NG, cus, n_params, pl.variant, pl.Bp, pl.rt, pl.KS, pl.k1_grid,
                              pl.k1c.KC, pl.k1c.RT, pl.k1c.KS, pl.k1c.blocks, pl.k3_rows, pl.k3_narrow,
                              pl.k3s_pair, pl.S0, pl.S1, pl.sparse, pl.slabs, pl.pre_tiles, pl.k2_grid,
                              pl.k2_grid_pre, pl.n_jobs};
  for (int i = 0; i < kMaxJobs; ++i) v.push_back(pl.job_tn[i]);
  for (int i = 0; i < kMaxJobs; ++i) v.push_back(pl.job_tiles[i]);
  for (int i = 0; i < kMaxJobs; ++i) v.push_back(pl.job_splits[i]);
  for (int i = 0; i <= kMaxJobs; ++i) v.push_back(pl.job_start[i]);
  const FusedWs& w = pl.ws;
  for (int64_t x : {w.wsplit, w.part, w.pstride, w.hg_part, w.xhat[0], w.xhat[1], w.U, w.Xn, w.dS, w.dHG, w.rinfo[0],
                    w.rinfo[1], w.mask[0], w.mask[1], w.maxS, w.total})
    v.push_back(x);
  printf("%s\n[", first ? "" : ",");
  for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", v[i]);
  printf("]");
}

}  // namespace

int main() {
  static_assert(kMaxJobs == 8, "the row format below");
  if (n_params_of(4) != 256417) {  // (tests/test_abi.py pins the same number on the library)
    fprintf(stderr, "step_plan_check: n_params_of(4) = %lld\n", static_cast<long long>(n_params_of(4)));
    return 1;
  }
  // the environment of the test holds no HBK_ knob: the defaults
  const StepKnobs env = read_step_knobs(), dflt;
  if (env.step != dflt.step || env.v2_min_b != dflt.v2_min_b || env.k1_ks != dflt.k1_ks || env.k3_wide != dflt.k3_wide ||
      env.dense != dflt.dense || env.kv_waves8 != dflt.kv_waves8 || env.k1_kc != dflt.k1_kc || env.k1_rt != dflt.k1_rt ||
      env.k3_r != dflt.k3_r || env.k3_pair != dflt.k3_pair || env.pre_tiles != dflt.pre_tiles ||
      env.plan_log != dflt.plan_log || env.eval_laps != dflt.eval_laps) {
    fprintf(stderr, "step_plan_check: read_step_knobs() without knobs differs from the defaults\n");
    return 1;
  }
  const std::vector<int> all_b = {1, 16, 17, 128, 129, 138, 273, 550, 799, 800, 1100, 1101, 2048, 4099};
  const std::vector<int> all_cus = {1, 32, 64, 96, 97, 128, 129, 256}, all_ng = {2, 3, 4};
  const std::vector<int> few_b = {138, 800, 1100, 4099}, few_cus = {64, 128, 256}, few_ng = {2, 4};
  // knob sets: 0 the defaults over the whole grid; then the forced rows
  struct Case {
    StepKnobs kn;
    std::vector<int> b, cus, ng;
  };
  std::vector<Case> cases(9);
  cases[8] = {dflt, {8192, 8193}, {64, 256}, few_ng};  // rt = 512, 513: either side of kK3sMaxTiles (sparse on / off)
  cases[0] = {dflt, all_b, all_cus, all_ng};
  cases[1] = {dflt, {17, 138}, all_cus, all_ng};  // HBK_STEP=2
  cases[1].kn.step = 2;
  cases[2] = {dflt, {1100}, {64}, all_ng};  // HBK_STEP=1
  cases[2].kn.step = 1;
  cases[3] = {dflt, few_b, few_cus, few_ng};  // HBK_K3_R=128
  cases[3].kn.k3_r = 128;
  cases[4] = {dflt, few_b, few_cus, few_ng};  // HBK_K3_PAIR=0
  cases[4].kn.k3_pair = 0;
  cases[5] = {dflt, few_b, few_cus, few_ng};  // HBK_K1_KC=64 HBK_K1_RT=1
  cases[5].kn.k1_kc = 64;
  cases[5].kn.k1_rt = 1;
  cases[6] = {dflt, few_b, few_cus, few_ng};  // HBK_K3_WIDE=1
  cases[6].kn.k3_wide = true;
  cases[7] = {dflt, few_b, few_cus, few_ng};  // HBK_STEP_DENSE=1
  cases[7].kn.dense = true;
  printf("{\"fields\": [\"knobs\", \"B\", \"NG\", \"cus\", \"n_params\", \"variant\", \"Bp\", \"rt\", \"KS\", \"k1_grid\", "
         "\"k1c_KC\", \"k1c_RT\", \"k1c_KS\", \"k1c_blocks\", \"k3_rows\", \"k3_narrow\", \"k3s_pair\", \"S0\", \"S1\", "
         "\"sparse\", \"slabs\", \"pre_tiles\", \"k2_grid\", \"k2_grid_pre\", \"n_jobs\", \"job_tn[8]\", \"job_tiles[8]\", "
         "\"job_splits[8]\", \"job_start[9]\", \"wsplit\", \"part\", \"pstride\", \"hg_part\", \"xhat[2]\", \"U\", \"Xn\", "
         "\"dS\", \"dHG\", \"rinfo[2]\", \"mask[2]\", \"maxS\", \"total\"],\n\"rows\": [");
  bool first = true;
  for (size_t c = 0; c < cases.size(); ++c)
    for (int B : cases[c].b)
      for (int NG : cases[c].ng)
        for (int cus : cases[c].cus) {
          const int64_t n_params = n_params_of(NG);
          const StepPlan pl = plan_step(B, NG, n_params, cus, cases[c].kn);
          invariants(pl, static_cast<int>(c), B, NG, cus, n_params);
          print_row(pl, static_cast<int>(c), B, NG, cus, n_params, first);
          first = false;
        }
  printf("\n]}\n");
  return g_failed ? 1 : 0;
}
