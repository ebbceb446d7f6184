// Stand-alone planner query for tests/test_step_routes.py (built with -fsanitize=address,undefined
// and run as a child process): hbk_mlp_plan.h alone, no HIP. Each line of stdin is one case,
//   name B NG cus step k1_ks k1_kc k1_rt k3_r k3_pair pre_tiles
// (the knobs as StepKnobs holds them: 0 / -1 / 3 are the defaults), and the output is a JSON list
// of the plans plan_step() returns for them, with the fields of hbk_mlp_step_plan_info.
#include <cstdio>

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

}  // namespace

int main() {
  char name[128];
  int B, NG, cus, step, ks, kc, rt, k3r, pair, pre;
  bool first = true;
  printf("[");
  for (;;) {
    const int n =
        scanf("%127s %d %d %d %d %d %d %d %d %d %d", name, &B, &NG, &cus, &step, &ks, &kc, &rt, &k3r, &pair, &pre);
    if (n == EOF) break;
    if (n != 11 || B < 1 || B > (1 << 22) || NG < 2 || NG > kMaxG || cus < 1) {
      fprintf(stderr, "step_routes_check: bad case line (%d fields read)\n", n);
      return 1;
    }
    StepKnobs kn;
    kn.step = step;
    kn.k1_ks = ks;
    kn.k1_kc = kc;
    kn.k1_rt = rt;
    kn.k3_r = k3r;
    kn.k3_pair = pair;
    kn.pre_tiles = pre;
    const StepPlan pl = plan_step(B, NG, n_params_of(NG), cus, kn);
    const bool v2 = pl.variant == 2;
    printf("%s\n{\"name\": \"%s\", \"variant\": %d, \"Bp\": %lld, \"rt\": %d, \"KS\": %d, \"k1_grid\": %d, \"KC\": %d, "
           "\"RT\": %d, \"k3s_pair\": %d, \"NST0\": %d, \"NST1\": %d, \"S0\": %d, \"S1\": %d, \"sparse\": %d, "
           "\"slabs\": %d, \"pre_tiles\": %d, \"k3_rows\": %d, \"k3_narrow\": %d, \"NG\": %d, \"cus\": %d}",
           first ? "" : ",", name, pl.variant, static_cast<long long>(pl.Bp), pl.rt, pl.KS, pl.k1_grid, pl.k1c.KC,
           pl.k1c.RT, v2 ? pl.k3s_pair : -1, v2 ? kK3sPairs[pl.k3s_pair][0] : 0, v2 ? kK3sPairs[pl.k3s_pair][1] : 0,
           pl.S0, pl.S1, pl.sparse, pl.slabs, pl.pre_tiles, pl.k3_rows, pl.k3_narrow, NG, cus);
    first = false;
  }
  printf("\n]\n");
  return 0;
}
