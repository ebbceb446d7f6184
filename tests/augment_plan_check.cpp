// Stand-alone check of csrc/hbk_augment_plan.h (tests/test_augment_plan.py builds it with
// AddressSanitizer + UBSan and runs it): asserts the invariants of the pitch-shift geometry,
// workspace layout and launch grids, of the band-stop and colored-noise layouts and of the
// reverb tables, and prints the geometry, layouts and grids as JSON for the comparison with
// the recorded table. An invariant that fails is reported on stderr and the exit status is 1.
// With `L sample_rate num den` quadruples as arguments it checks and prints those pitch cases alone
// (tests/test_pitch_shapes.py).
#include "hbk_augment_plan.h"

#include <cinttypes>
#include <cstdlib>
#include <cstring>

using namespace hbk;

static int g_failed = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      fprintf(stderr, "FAILED %s: ", #cond);          \
      fprintf(stderr, __VA_ARGS__);                   \
      fprintf(stderr, "\n");                          \
      g_failed = 1;                                   \
    }                                                 \
  } while (0)

struct Region {
  const char* name;
  int64_t off, bytes;  // bytes: what the kernels address in it
  int64_t align = 256;
};

// offsets ascend and are aligned (256 B unless the region says otherwise), regions are disjoint and inside total
static void check_regions(const char* what, const Region* r, int n, int64_t total) {
  for (int i = 0; i < n; ++i) {
    CHECK(r[i].off % r[i].align == 0, "%s.%s at %" PRId64, what, r[i].name, r[i].off);
    CHECK(r[i].bytes >= 0, "%s.%s", what, r[i].name);
    const int64_t end = i + 1 < n ? r[i + 1].off : total;
    CHECK(r[i].off <= end, "%s.%s does not ascend", what, r[i].name);
    CHECK(r[i].off + r[i].bytes <= end, "%s.%s: %" PRId64 " bytes do not fit before %" PRId64, what, r[i].name,
          r[i].bytes, end);
  }
}

static void json_string(const std::string& s) {
  putchar('"');
  for (char c : s) {
    if (c == '"' || c == '\\') putchar('\\');
    putchar(c);
  }
  putchar('"');
}

static void print_grid(const char* name, const Grid& g, bool last = false) {
  printf("\"%s\": [%u, %u, %u]%s", name, g.x, g.y, g.block, last ? "" : ", ");
}

static void pitch_case(int64_t L, int32_t rate, int32_t num, int32_t den, bool last) {
  PitchGeometry g;
  std::string err;
  const int rc = pitch_geometry(L, rate, num, den, g, err);
  printf("  {\"L\": %" PRId64 ", \"sample_rate\": %d, \"num\": %d, \"den\": %d, \"rc\": %d, \"error\": ", L, rate, num,
         den, rc);
  json_string(err);
  CHECK((rc == kPlanOk) == err.empty(), "a refusal carries a message");
  if (rc == kPlanOk) {
    CHECK(g.nw <= 128 && g.nw <= kPsPhaseMax, "nw %d", g.nw);
    CHECK(2 * g.width + g.orig <= kPsTapMax, "taps %d", 2 * g.width + g.orig);
    CHECK(g.L == L && g.f_in > 0 && g.f_out > 0 && g.l1 > 0 && g.target > 0, "geometry");
    printf(", \"geometry\": {\"L\": %d, \"f_in\": %d, \"f_out\": %d, \"l1\": %d, \"orig\": %d, \"nw\": %d, "
           "\"width\": %d, \"target\": %d, \"rate\": %.17g},\n   \"calls\": [\n",
           g.L, g.f_in, g.f_out, g.l1, g.orig, g.nw, g.width, g.target, g.rate);
    const int64_t ns[] = {1, 2, 3, 65535};
    for (int i = 0; i < 4; ++i) {
      const int64_t n = ns[i];
      const PitchLayout w = pitch_layout(g, n);
      const int64_t groups = (n + kPvClips - 1) / kPvClips;
      const Region r[] = {{"y", w.y, n * g.l1 * 4},   {"taps", w.taps, int64_t(kPsPhaseMax) * kPsTapMax * 4},
                          {"yr", w.yr, n * 8},        {"sp", w.sp, n * 8},
                          {"key", w.key, n * 8},      {"ord", w.ord, n * 4},
                          {"gord", w.gord, groups * 4}};
      check_regions("pitch", r, 7, w.total);
      CHECK(w.y == 0 && groups <= n, "y leads the workspace; the group keys reuse the clips' slots");
      printf("    {\"n\": %" PRId64 ", \"y\": %" PRId64 ", \"taps\": %" PRId64 ", \"yr\": %" PRId64 ", \"sp\": %" PRId64
             ", \"key\": %" PRId64 ", \"ord\": %" PRId64 ", \"gord\": %" PRId64 ", \"total\": %" PRId64 ",\n",
             n, w.y, w.taps, w.yr, w.sp, w.key, w.ord, w.gord, w.total);
      // the default knobs, then the A/B pair without spans on the VALU resampler
      for (int kset = 0; kset < 2; ++kset) {
        PitchKnobs k;
        if (kset) k.span = false, k.resample_valu = true;
        const PitchLaunches p = pitch_launches(g, n, k);
        const Grid* all[] = {&p.taps, &p.span, &p.rank_clips, &p.group, &p.rank_groups, &p.vocoder, &p.resample};
        for (const Grid* q : all)
          CHECK(q->x > 0 && q->y > 0 && q->block > 0 && q->block <= 1024 && q->y <= 65535, "grid %u x %u x %u", q->x,
                q->y, q->block);
        CHECK(p.groups == groups && p.vocoder.x == unsigned(groups), "one vocoder workgroup per group");
        CHECK(p.pair == (kset == 0) && p.resample_mfma == (kset == 0), "knobs");
        CHECK(int64_t(p.taps.x) * p.taps.block >= int64_t(g.nw) * kPsTapMax, "a thread per tap");
        CHECK(int64_t(p.span.x) * 4 >= n && int64_t(p.rank_clips.x) * 64 >= n, "a wave / a lane per clip");
        CHECK(int64_t(p.group.x) * 256 >= groups && int64_t(p.rank_groups.x) * 64 >= groups, "a lane per group");
        const int per = p.resample_mfma ? kRsFrames : kPsResFrames;
        CHECK(int64_t(p.resample.x) * per * g.nw >= g.L && p.resample.y == unsigned(n), "the resampler covers the clip");
        printf("     \"%s\": {\"pair\": %d, \"groups\": %d, \"mfma\": %d, ", kset ? "launches_ab" : "launches", int(p.pair),
               p.groups, int(p.resample_mfma));
        print_grid("taps", p.taps);
        print_grid("span", p.span);
        print_grid("rank_clips", p.rank_clips);
        print_grid("group", p.group);
        print_grid("rank_groups", p.rank_groups);
        print_grid("vocoder", p.vocoder);
        print_grid("resample", p.resample, true);
        printf("}%s\n", kset ? "" : ",");
      }
      printf("    }%s\n", i < 3 ? "," : "");
    }
    printf("   ]");
  }
  printf("}%s\n", last ? "" : ",");
}

static void colored_case(int64_t n_clips, int64_t cpn, bool last) {
  const ColoredLayout w = colored_layout(n_clips, cpn);
  const Region r[] = {{"gbuf", w.gbuf, w.groups * kN1 * 4}, {"grms", w.grms, w.groups * 4}};
  check_regions("colored", r, 2, w.total);
  CHECK((w.groups == 0) == (w.total == 0), "no groups, no workspace");
  if (w.groups) CHECK(w.groups * cpn >= n_clips && (w.groups - 1) * cpn < n_clips, "groups cover the clips");
  printf("  {\"n_clips\": %" PRId64 ", \"clips_per_noise\": %" PRId64 ", \"groups\": %" PRId64 ", \"gbuf\": %" PRId64
         ", \"grms\": %" PRId64 ", \"total\": %" PRId64 "}%s\n",
         n_clips, cpn, w.groups, w.gbuf, w.grms, w.total, last ? "" : ",");
}

static void band_stop_case(int64_t n, int32_t filters, int32_t spectra, int64_t blocks, bool last) {
  const BandStopLayout w = band_stop_layout(n, filters, spectra, blocks);
  const Region r[] = {{"sums", w.sums, int64_t(filters) * 8},
                      {"taps", w.taps, int64_t(filters) * (kBsCirc + 1) * 4},
                      {"spectra", w.spectra, int64_t(spectra) * kHSlots * 8},
                      // (a spectrum is 92,288 bytes, 360.5 x 256: the float rows behind them are 128-B aligned)
                      {"scratch", w.scratch, blocks * kT * 4, 128}};
  check_regions("band_stop", r, 4, w.total);
  printf("  {\"n\": %" PRId64 ", \"filters\": %d, \"spectra\": %d, \"blocks\": %" PRId64 ", \"sums\": %" PRId64
         ", \"taps\": %" PRId64 ", \"spectra_off\": %" PRId64 ", \"scratch\": %" PRId64 ", \"total\": %" PRId64 "}%s\n",
         n, filters, spectra, blocks, w.sums, w.taps, w.spectra, w.scratch, w.total, last ? "" : ",");
}

// every float of the six tables against the formula restated here: (cos, sin)(-2 pi e / N) in double
static int64_t check_tables() {
  const ReverbTables t = reverb_tables();
  const int count[kTabCount] = {90, 128, 11521, 80, 100, 4001};
  const int step[kTabCount] = {128, 1, 1, 100, 1, 1};
  const int period[kTabCount] = {11520, 11520, 23040, 8000, 8000, 16000};
  CHECK(kTwHi == 90 && kTwLo == 128 && kM + 1 == 11521 && kTw8Hi == 80 && kTw8Lo == 100 && kM1 / 2 + 1 == 4001, "sizes");
  int64_t checked = 0;
  for (int i = 0; i < kTabCount; ++i) {
    const size_t slots = i == kTabN ? size_t(16 * 721) : size_t(count[i]);
    CHECK(t.off[i] % 256 == 0, "table %d at %zu", i, t.off[i]);
    CHECK(t.pairs[i] == slots, "table %d holds %zu pairs", i, t.pairs[i]);
    const size_t end = i + 1 < kTabCount ? t.off[i + 1] : t.bytes();
    CHECK(t.off[i] + slots * 8 <= end && end <= t.bytes(), "table %d inside the allocation", i);
    if (t.off[i] + slots * 8 > t.bytes()) continue;
    const float* tab = t.host.data() + t.off[i] / sizeof(float);
    std::vector<char> mapped(slots, 0);
    for (int k = 0; k < count[i]; ++k) {
      const size_t slot = i == kTabN ? size_t(k % 16) * 721 + size_t(k / 16) : size_t(k);
      const double a = -2.0 * M_PI * (double(k) * double(step[i])) / double(period[i]);
      const float re = float(cos(a)), im = float(sin(a));
      CHECK(slot < slots && !mapped[slot], "table %d bin %d", i, k);
      CHECK(memcmp(&tab[2 * slot], &re, 4) == 0 && memcmp(&tab[2 * slot + 1], &im, 4) == 0, "table %d bin %d: (%a, %a)", i,
            k, double(tab[2 * slot]), double(tab[2 * slot + 1]));
      mapped[slot] = 1;
      ++checked;
    }
    for (size_t s = 0; s < slots; ++s)
      if (!mapped[s]) CHECK(tab[2 * s] == 0.f && tab[2 * s + 1] == 0.f, "table %d: unmapped slot %zu is not zero", i, s);
  }
  CHECK(t.bytes() % 256 == 0 && t.bytes() < (size_t(1) << 18), "one small allocation: %zu bytes", t.bytes());
  return checked;
}

int main(int argc, char** argv) {
  if (argc > 1) {  // L rate num den quadruples: those pitch cases alone (tests/test_pitch_shapes.py)
    if ((argc - 1) % 4 != 0) {
      fprintf(stderr, "usage: %s [L sample_rate num den]...\n", argv[0]);
      return 2;
    }
    printf("{\n \"pitch\": [\n");
    for (int i = 1; i < argc; i += 4)
      pitch_case(strtoll(argv[i], nullptr, 10), int32_t(strtol(argv[i + 1], nullptr, 10)),
                 int32_t(strtol(argv[i + 2], nullptr, 10)), int32_t(strtol(argv[i + 3], nullptr, 10)), i + 4 >= argc);
    printf(" ]\n}\n");
    return g_failed;
  }
  printf("{\n \"pitch\": [\n");
  const int64_t kMax = int64_t(1) << 24;
  pitch_case(23040, 16000, 128, 125, false);
  pitch_case(23040, 16000, 125, 128, false);
  pitch_case(126, 16000, 128, 125, false);  // the shortest accepted clip
  pitch_case(125, 16000, 128, 125, false);
  pitch_case(kMax, 16000, 128, 125, false);
  pitch_case(kMax + 1, 16000, 128, 125, false);
  pitch_case(23040, 22050, 128, 125, false);
  pitch_case(23040, 16000, 3, 2, false);
  pitch_case(23040, 16000, 0, 125, false);
  pitch_case(23040, 16000, 128, 0, true);
  printf(" ],\n \"colored\": [\n");
  colored_case(0, 4, false);
  colored_case(5, 1, false);
  colored_case(5, 2, false);
  colored_case(4, 4, false);
  colored_case(5, 4, false);
  colored_case(int64_t(1) << 20, 3, true);
  printf(" ],\n \"band_stop\": [\n");
  band_stop_case(1, 1, 1, 1, false);
  band_stop_case(5, 2, 3, 5, false);
  band_stop_case(300, 3, 7, 256, true);
  printf(" ],\n \"lds\": {\"augment\": %zu, \"band_stop\": %zu, \"colored\": %zu},\n", kAugLds, kBandStopLds, kColoredLds);
  printf(" \"table_values_checked\": %" PRId64 "\n}\n", check_tables());
  return g_failed;
}
