// Stand-alone check of the half-layer bank's geometry (hbk_mlp_half_plan.h), run by
// tests/test_half_plan.py as a child process built with -fsanitize=address,undefined.
// For the default dims and a non-default architecture (layer 32, hidden 24) and B in
// {1, 17, 130, 1100} it asserts, independently of the header's arithmetic: the parameter
// offsets (every tensor one run, branches back to back, the counts of the reference), the
// workspace regions (ascending, aligned, disjoint, large enough) and that every launch grid
// covers its output exactly once; then it prints one line per case for the test to compare.
#include <cstdio>
#include <vector>

#include "hbk_mlp_half_plan.h"

using namespace hbk;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      fprintf(stderr, "half_plan_check: %s fails (layer %d, hid %d, B %d)\n", #cond, d.layer, \
              d.hid, int(B));                                                                \
      ++g_failed;                                                                            \
    }                                                                                        \
  } while (0)

const int32_t kIdx[16][8] = {
    {0, 1, 2, 3, 4, 5, 6, 7},     {8, 9, 10, 11, 12, 13, 14, 15}, {0, 1, 2, 3, 8, 9, 10, 11},   {4, 5, 6, 7, 12, 13, 14, 15},
    {4, 5, 6, 7, 8, 9, 10, 11},   {0, 1, 2, 3, 12, 13, 14, 15},   {0, 1, 4, 5, 8, 9, 12, 13},   {2, 3, 6, 7, 10, 11, 14, 15},
    {0, 1, 6, 7, 8, 9, 14, 15},   {2, 3, 4, 5, 10, 11, 12, 13},   {0, 2, 4, 6, 8, 10, 12, 14},  {1, 3, 5, 7, 9, 11, 13, 15},
    {0, 3, 4, 7, 8, 11, 12, 15},  {1, 2, 5, 6, 9, 10, 13, 14},    {0, 5, 2, 7, 8, 13, 10, 15},  {1, 4, 3, 6, 9, 12, 11, 14}};

bool tiles_cover(unsigned tiles, int64_t n) {  // tiles of kHalfTile cover n with no spare tile
  return int64_t(tiles) * kHalfTile >= n && (int64_t(tiles) - 1) * kHalfTile < n;
}

void check(const HalfDims& d, int64_t base, int64_t B) {
  CHECK(half_validate(d, &kIdx[0][0]) == 0);
  const int64_t K = d.d_in / 2, H = d.hid, L = d.layer, nh = d.n_half;
  // parameters: the reference's count per branch, in state-dict runs
  const HalfOffsets o = half_offsets(d, base);
  const int64_t per_branch = 2 * K + 2 * (H * K + H) + L * H + L;
  CHECK(o.base == base && o.stride == per_branch && o.total == nh * per_branch);
  CHECK(o.g == 0 && o.b == K && o.w_hg == 2 * K && o.b_hg == o.w_hg + 2 * H * K);
  CHECK(o.w_o == o.b_hg + 2 * H && o.b_o == o.w_o + L * H && o.b_o + L == o.stride);
  // workspace
  const HalfWs w = half_ws_layout(d, B);
  const int64_t off[] = {w.stats, w.hg, w.u, w.dhg, w.xd, w.part, w.total};
  const int64_t size[] = {B * nh * 2, B * nh * 2 * H, B * nh * H, B * nh * 2 * H, B * d.d_in, nh * B * L};
  int64_t need = 0;
  for (int i = 0; i < 6; ++i) {
    CHECK(off[i] >= 0 && off[i] % 64 == 0 && off[i] + size[i] <= off[i + 1]);
    need += (size[i] + 63) / 64 * 64;
  }
  CHECK(w.stats == 0 && w.total == need);
  // grids
  const HalfGrids g = half_grids(d, B);
  CHECK(int64_t(g.stats.x) == B && g.stats.y == 1 && g.stats.z == 1);
  CHECK(tiles_cover(g.hg.x, 2 * H) && tiles_cover(g.hg.y, B) && g.hg.z == nh);
  CHECK(g.gate.x >= 1 && g.gate.x <= 4096 && g.gate.y == 1 && g.gate.z == 1);
  CHECK(tiles_cover(g.out.x, L) && tiles_cover(g.out.y, B) && g.out.z == nh);  // a tile of part_h each: no atomics
  CHECK(g.sum.x >= 1 && g.sum.x <= 4096 && g.sum.y == 1 && g.sum.z == 1);
  CHECK(tiles_cover(g.dwo.x, nh * H) && tiles_cover(g.dwo.y, L));
  CHECK(g.dwo_k_split >= kHalfTileK && g.dwo_k_split % kHalfTileK == 0);
  CHECK(int64_t(g.dwo.z) * g.dwo_k_split >= B && (int64_t(g.dwo.z) - 1) * g.dwo_k_split < B);  // no empty split
  CHECK(tiles_cover(g.du.x, nh * H) && tiles_cover(g.du.y, B) && g.du.z == 1);
  CHECK(g.cs_rows >= 1 && int64_t(g.cs.x) * g.cs_rows >= B && (int64_t(g.cs.x) - 1) * g.cs_rows < B);
  CHECK(tiles_cover(g.dwhg.x, K) && tiles_cover(g.dwhg.y, 2 * H) && g.dwhg.z == nh);  // the whole batch per tile
  for (const HalfGrid* q : {&g.stats, &g.hg, &g.gate, &g.out, &g.sum, &g.dwo, &g.du, &g.cs, &g.dwhg})
    CHECK(q->x >= 1 && q->y >= 1 && q->y <= 65535 && q->z >= 1 && q->z <= 65535);
  printf("%d %d %lld | %lld %lld | %lld %lld %lld %lld %lld %lld %lld | hg %u %u %u out %u %u %u dwo %u %u %u/%d du %u %u cs %u/%d dwhg %u %u %u\n",
         d.layer, d.hid, (long long)B, (long long)o.stride, (long long)o.total, (long long)w.stats, (long long)w.hg,
         (long long)w.u, (long long)w.dhg, (long long)w.xd, (long long)w.part, (long long)w.total, g.hg.x, g.hg.y,
         g.hg.z, g.out.x, g.out.y, g.out.z, g.dwo.x,
         g.dwo.y, g.dwo.z, g.dwo_k_split, g.du.x, g.du.y, g.cs.x, g.cs_rows, g.dwhg.x, g.dwhg.y, g.dwhg.z);
}

}  // namespace

int main() {
  HalfDims d;
  d.d_in = 1536;
  d.n_tokens = 16;
  d.n_half = 16;
  const int64_t Bs[] = {1, 17, 130, 1100};
  d.layer = 96;
  d.hid = 64;
  for (int64_t B : Bs) check(d, 256417, B);
  d.layer = 32;
  d.hid = 24;
  for (int64_t B : Bs) check(d, 81769, B);
  // what hbk_mlp_plan_create_half must reject
  {
    const int64_t B = 0;
    HalfDims e = d;
    e.d_in = 1540;
    CHECK(half_validate(e, &kIdx[0][0]) == 3);
    e = d;
    e.n_tokens = 15;
    CHECK(half_validate(e, &kIdx[0][0]) == 2);
    e = d;
    e.n_half = 40;  // 320 indices: more than the kernels' table
    CHECK(half_validate(e, &kIdx[0][0]) == 6);
    std::vector<int32_t> bad(&kIdx[0][0], &kIdx[0][0] + 128);
    bad[127] = 16;
    CHECK(half_validate(d, bad.data()) == 5);
    bad[127] = -1;
    CHECK(half_validate(d, bad.data()) == 5);
    CHECK(half_validate(d, nullptr) == 4);
  }
  return g_failed ? 1 : 0;
}
