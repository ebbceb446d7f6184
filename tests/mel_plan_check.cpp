// Stand-alone check of csrc/hbk_mel_plan.h (tests/test_mel_plan.py builds it with
// AddressSanitizer + UBSan and runs it on a file of raw f32: the windows W0-W2, then the banks
// B0-B5 and M2 of tests/test_mel_routes.py). It asserts the invariants of the table buffer
// (offsets ascending, 256-B aligned, regions as large as the kernels' indexing of them), of both
// filter layouts (read windows in range, every non-zero bin inside its window, weights the
// filterbank's), of the twiddle tables (the formula restated here) and of the SoA table's rows, and
// prints status, scalars, routes, offsets, start bins, table hashes and launch grids as JSON for
// the comparison with the recorded table. An invariant that fails is reported on stderr and the
// exit status is 1.
#include "hbk_mel_plan.h"

#include <cinttypes>
#include <cstdlib>

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

static const char* const kTableName[kMelTableCount] = {"win", "tw256", "tw512", "lo", "w",
                                                       "twsm", "lo2", "w2", "fbt", "t4"};
static const int kBankMels[7] = {32, 30, 32, 30, 32, 32, 2};
static const char* const kBankName[7] = {"B0", "B1", "B2", "B3", "B4", "B5", "M2"};
static const float kInScale = 32767.f, kLogFloor = 1e-10f, kOutDiv = 10.f, kOutAdd = 2.f;

struct Knobs {
  const char* name;
  MelKnobs k;
};

static void json_string(const std::string& s) {
  putchar('"');
  for (char c : s) {
    if (c == '"' || c == '\\') putchar('\\');
    putchar(c);
  }
  putchar('"');
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

static uint64_t fnv(const float* p, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
  for (size_t i = 0; i < 4 * n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

static void print_ints(const char* name, const float* p, int n) {
  printf("\"%s\": [", name);
  for (int i = 0; i < n; ++i) {
    int v;
    memcpy(&v, p + i, 4);
    printf("%s%d", i ? ", " : "", v);
  }
  printf("]");
}

// (cos, sin)(-2 pi i / N): the twiddle formula, restated
static void twiddle(int i, int N, float& re, float& im) {
  const double ang = -2.0 * M_PI * i / double(N);
  re = static_cast<float>(cos(ang));
  im = static_cast<float>(sin(ang));
}

static void check_tables(const MelTables& t, const float* window, const float* fb, int n_mels) {
  const MelScalars& s = t.s;
  const size_t need[kMelTableCount] = {512 * 4, 256 * 8, 257 * 8, size_t(n_mels) * 4, size_t(n_mels) * s.taps * 4,
                                       size_t(kBins2) * 8, 32 * 4, size_t(16 * (kTapsA + kTapsB)) * 4,
                                       size_t(32 * kBins2) * 4, size_t(kE4N) * 8 * 16};
  for (int i = 0; i < kMelTableCount; ++i) {
    const size_t end = i + 1 < kMelTableCount ? t.off[i + 1] : t.bytes();
    const bool present = i < kMelTwsm || s.v2;
    CHECK(t.off[i] % 256 == 0, "%s at %zu", kTableName[i], t.off[i]);
    CHECK(t.off[i] <= end && end <= t.bytes(), "%s does not ascend", kTableName[i]);
    CHECK(t.size[i] == (present ? need[i] : 0), "%s holds %zu bytes, the kernels index %zu", kTableName[i], t.size[i],
          present ? need[i] : 0);
    CHECK(t.off[i] + t.size[i] <= end, "%s overlaps the next table", kTableName[i]);
  }
  CHECK(t.bytes() % 256 == 0 && t.bytes() < (size_t(1) << 16), "one small allocation: %zu bytes", t.bytes());
  if (g_failed) return;

  for (int i = 0; i < 512; ++i) CHECK(same_bits(t.f(kMelWin)[i], window[i] * kInScale), "win[%d]", i);
  float re, im;
  for (int i = 0; i < 256; ++i) {
    twiddle(i, 256, re, im);
    CHECK(same_bits(t.f(kMelTw256)[2 * i], re) && same_bits(t.f(kMelTw256)[2 * i + 1], im), "tw256[%d]", i);
  }
  for (int i = 0; i < 257; ++i) {
    twiddle(i, 512, re, im);
    CHECK(same_bits(t.f(kMelTw512)[2 * i], re) && same_bits(t.f(kMelTw512)[2 * i + 1], im), "tw512[%d]", i);
  }
  // v1 layout: bins [lo, lo + taps) of every filter, inside [0, 257), holding all its non-zero bins
  CHECK(s.taps >= 1 && s.taps <= kMaxTaps, "taps %d", s.taps);
  int kmax = 0;
  for (int m = 0; m < n_mels; ++m) {
    int lo;
    memcpy(&lo, t.f(kMelLo) + m, 4);
    CHECK(lo >= 0 && lo + s.taps <= 257, "lo[%d] = %d", m, lo);
    if (lo < 0 || lo + s.taps > 257) continue;
    kmax = std::max(kmax, lo + s.taps - 1);
    for (int k = 0; k < 257; ++k) {
      const float f = fb[k * n_mels + m];
      if (k >= lo && k < lo + s.taps)
        CHECK(same_bits(t.f(kMelW)[m * s.taps + k - lo], f), "w[%d][%d]", m, k - lo);
      else
        CHECK(f == 0.f, "mel %d: bin %d lies outside [%d, %d)", m, k, lo, lo + s.taps);
    }
  }
  CHECK(s.need256 == (kmax >= 256) && 16 * s.nk2 > std::min(kmax, 255) && s.nk2 <= 16, "nk2 %d need256 %d kmax %d", s.nk2,
        s.need256, kmax);
  if (!s.v2) {
    CHECK(s.edge0 == 0 && s.variant == 0 && s.v4 == 0, "a v1 plan has no v2 scalars");
    return;
  }
  CHECK(n_mels == 32, "v2 is the 32-mel layout");
  bool edge0 = true;
  for (int i = 0; i < 32; ++i) edge0 = edge0 && window[i] == 0.f && window[511 - i] == 0.f;
  CHECK(s.edge0 == int(edge0), "edge0");
  for (int k = 0; k < kBins2; ++k) {  // -i W512^k = (sin, -cos)
    const double ang = -2.0 * M_PI * k / 512.0;
    CHECK(same_bits(t.f(kMelTwsm)[2 * k], float(sin(ang))) && same_bits(t.f(kMelTwsm)[2 * k + 1], float(-cos(ang))),
          "twsm[%d]", k);
  }
  // v2 layout: filter m < 16 at A slot m (8 taps), filter m >= 16 at B slot 31 - m (16 taps)
  const float* w2 = t.f(kMelW2);
  for (int m = 0; m < 32; ++m) {
    const int T = m < 16 ? 8 : 16, slot = m < 16 ? m : 31 - m;
    int lo2;
    memcpy(&lo2, t.f(kMelLo2) + (m < 16 ? slot : 16 + slot), 4);
    CHECK(lo2 >= 0 && lo2 % 2 == 0 && lo2 + T <= 128, "lo2 of mel %d = %d", m, lo2);
    if (lo2 < 0 || lo2 + T > 128) continue;
    const float* w = w2 + (m < 16 ? 8 * slot : 16 * 8 + 16 * slot);
    for (int k = 0; k < 257; ++k) {
      const float f = fb[k * 32 + m];
      if (k >= lo2 && k < lo2 + T)
        CHECK(same_bits(w[k - lo2], 0.25f * f), "w2 of mel %d tap %d", m, k - lo2);
      else
        CHECK(f == 0.f, "mel %d: bin %d lies outside [%d, %d)", m, k, lo2, lo2 + T);
    }
    for (int k = 0; k < kBins2; ++k) CHECK(same_bits(t.f(kMelFbt)[m * kBins2 + k], 0.25f * fb[k * 32 + m]), "fbt[%d][%d]", m, k);
  }
  // the SoA table, [entry][lane jj] of float4
  const float* win = t.f(kMelWin);
  const float* twsm = t.f(kMelTwsm);
  for (int jj = 0; jj < 8; ++jj) {
    auto row = [&](int e) { return t.f(kMelT4) + 4 * (e * 8 + jj); };
    for (int n1 = 0; n1 < 16; ++n1) {
      const float* r = row(kE4Win + n1);
      const int s0 = 32 * n1 + 2 * jj;
      CHECK(same_bits(r[0], win[s0]) && same_bits(r[1], win[s0 + 16]) && same_bits(r[2], win[s0 + 1]) &&
                same_bits(r[3], win[s0 + 17]), "t4 window row %d lane %d", n1, jj);
    }
    for (int k1 = 0; k1 < 16; ++k1) {
      const float* r = row(kE4Tw + k1);
      float re1, im1;
      twiddle(jj * k1, 256, re, im);
      twiddle((jj + 8) * k1, 256, re1, im1);
      if (k1 == 0)
        CHECK(r[0] == 0.f && r[1] == 0.f && r[2] == 0.f && r[3] == 0.f, "t4 twiddle row 0 is unused");
      else
        CHECK(same_bits(r[0], re) && same_bits(r[1], re1) && same_bits(r[2], im) && same_bits(r[3], im1),
              "t4 twiddle row %d lane %d", k1, jj);
    }
    const int ra = jj == 0 ? 0 : jj, rb = jj == 0 ? 8 : 16 - jj;
    for (int k2 = 0; k2 < 8; ++k2) {
      const float* r = row(kE4Ws + k2);
      const float* a = twsm + 2 * (ra + 16 * k2);
      const float* b = twsm + 2 * (rb + 16 * k2);
      CHECK(same_bits(r[0], a[0]) && same_bits(r[1], b[0]) && same_bits(r[2], a[1]) && same_bits(r[3], b[1]),
            "t4 split row %d lane %d", k2, jj);
    }
    const float* src[4] = {w2 + 8 * jj, w2 + 8 * (jj + 8), w2 + 128 + 16 * jj, w2 + 128 + 16 * (jj + 8)};
    const int first[4] = {kE4Mel, kE4Mel + 2, kE4Mel + 4, kE4Mel + 8}, count[4] = {2, 2, 4, 4};
    for (int g = 0; g < 4; ++g)
      for (int q = 0; q < count[g]; ++q)
        for (int c = 0; c < 4; ++c)
          CHECK(same_bits(row(first[g] + q)[c], src[g][4 * q + c]), "t4 mel row %d lane %d", first[g] + q - kE4Mel, jj);
  }
}

static void print_case(const char* label, int rc, const std::string& err, const MelTables& t, int n_mels) {
  printf("  {\"case\": \"%s\", \"rc\": %d, \"error\": ", label, rc);
  json_string(err);
  CHECK((rc == kPlanOk) == err.empty(), "%s: a refusal carries a message", label);
  if (rc == kPlanOk) {
    const MelScalars& s = t.s;
    printf(", \"taps\": %d, \"nk2\": %d, \"need256\": %d, \"v2\": %d, \"edge0\": %d, \"variant\": %d, \"v4\": %d, "
           "\"route\": [%d, %d],\n   \"off\": [",
           s.taps, s.nk2, s.need256, s.v2, s.edge0, s.variant, s.v4, mel_route(s, 0), mel_route(s, 1));
    for (int i = 0; i < kMelTableCount; ++i) printf("%s%zu", i ? ", " : "", t.off[i]);
    printf("], \"total\": %zu,\n   ", t.bytes());
    print_ints("lo", t.f(kMelLo), n_mels);
    printf(",\n   \"hash\": {\"win\": \"%016" PRIx64 "\", \"w\": \"%016" PRIx64 "\"", fnv(t.f(kMelWin), 512),
           fnv(t.f(kMelW), size_t(n_mels) * s.taps));
    if (s.v2) {
      const float* t4 = t.f(kMelT4);
      printf(", \"w2\": \"%016" PRIx64 "\", \"fbt\": \"%016" PRIx64 "\", \"t4_win\": \"%016" PRIx64 "\", \"t4_mel\": \"%016" PRIx64
             "\"},\n   ",
             fnv(t.f(kMelW2), 16 * (kTapsA + kTapsB)), fnv(t.f(kMelFbt), 32 * kBins2), fnv(t4 + 4 * 8 * kE4Win, 4 * 8 * 16),
             fnv(t4 + 4 * 8 * kE4Mel, 4 * 8 * 12));
      print_ints("lo2", t.f(kMelLo2), 32);
    } else {
      printf("}");
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::vector<float> in;
  size_t want = 3 * 512;
  for (int m : kBankMels) want += size_t(257) * m;
  if (FILE* f = fopen(argv[1], "rb")) {
    in.resize(want + 1);
    in.resize(fread(in.data(), 4, want + 1, f));
    fclose(f);
  }
  if (in.size() != want) {
    fprintf(stderr, "%s: %zu floats, expected %zu\n", argv[1], in.size(), want);
    return 2;
  }
  const float* window[3] = {in.data(), in.data() + 512, in.data() + 1024};
  const float* bank[7];
  size_t at = 3 * 512;
  for (int b = 0; b < 7; ++b) {
    bank[b] = in.data() + at;
    at += size_t(257) * kBankMels[b];
  }
  Knobs knobs[6] = {{"none", {}}, {"V1", {}}, {"MFMA", {}}, {"V4=1", {}}, {"V4=8", {}}, {"V4=0", {}}};
  knobs[1].k.force_v1 = true;
  knobs[2].k.mfma = true;
  knobs[3].k.v4 = 4;  // read_mel_knobs: 0 or unset -> 0, 8 -> 8, any other value -> 4
  knobs[4].k.v4 = 8;

  printf("{\n \"plans\": [\n");
  bool first = true;
  for (int w = 0; w < 3; ++w)
    for (int b = 0; b < 7; ++b)
      for (const Knobs& k : knobs) {
        MelTables t;
        std::string err;
        const int rc = mel_tables(window[w], bank[b], 512, 160, kBankMels[b], kInScale, kLogFloor, kOutDiv, kOutAdd, k.k,
                                  t, err);
        printf("%s", first ? "" : ",\n");
        first = false;
        const std::string label = strf("W%d %s %s", w, kBankName[b], k.name);
        print_case(label.c_str(), rc, err, t, kBankMels[b]);
        printf("}");
        CHECK(rc == kPlanOk, "%s is refused", label.c_str());
        if (rc == kPlanOk) check_tables(t, window[w], bank[b], kBankMels[b]);
      }

  // the refusals of hbk_mel_plan_create, in the order of its checks
  printf("\n ],\n \"refusals\": [\n");
  std::vector<float> zeros(257 * 34, 0.f), wide(257 * 32, 0.f);
  for (int k = 40; k < 57; ++k) wide[k * 32 + 7] = 1.f;  // 17 taps
  struct Refusal {
    const char* label;
    const float* window;
    const float* fbank;
    int n_fft, hop, n_mels;
    float out_div;
  };
  const Refusal refusals[] = {
      {"window NULL", nullptr, bank[0], 512, 160, 32, 10.f}, {"fbank NULL", window[0], nullptr, 512, 160, 32, 10.f},
      {"n_fft 256", window[0], bank[0], 256, 160, 32, 10.f}, {"hop 0", window[0], bank[0], 512, 0, 32, 10.f},
      {"hop -160", window[0], bank[0], 512, -160, 32, 10.f}, {"n_mels 0", window[0], zeros.data(), 512, 160, 0, 10.f},
      {"n_mels 34", window[0], zeros.data(), 512, 160, 34, 10.f}, {"n_mels 3", window[0], bank[3], 512, 160, 3, 10.f},
      {"out_div 0", window[0], bank[0], 512, 160, 32, 0.f},  {"17 taps", window[0], wide.data(), 512, 160, 32, 10.f}};
  const int n_refusals = int(sizeof(refusals) / sizeof(refusals[0]));
  for (int i = 0; i < n_refusals; ++i) {
    const Refusal& r = refusals[i];
    MelTables t;
    std::string err;
    const int rc = mel_tables(r.window, r.fbank, r.n_fft, r.hop, r.n_mels, kInScale, kLogFloor, r.out_div, kOutAdd,
                              MelKnobs(), t, err);
    CHECK(rc != kPlanOk, "%s is accepted", r.label);
    print_case(r.label, rc, err, t, 0);
    printf("}%s\n", i + 1 < n_refusals ? "," : "");
  }

  // the argument checks of hbk_mel_frames, in their order (pointers: 8-byte aligned, + 4 is not)
  printf(" ],\n \"calls\": [\n");
  alignas(8) static float buf[4];
  struct Call {
    const char* label;
    int hop;
    const void* pcm;
    const void* out;
    int64_t n_clips, clip_stride, n_frames;
  };
  const Call calls[] = {{"13 x 141", 160, buf, buf, 13, 23040, 141},    {"n_clips -1", 160, buf, buf, -1, 23040, 141},
                        {"n_frames -1", 160, buf, buf, 13, 23040, -1},  {"n_clips 0, pcm NULL", 160, nullptr, buf, 0, 23040, 141},
                        {"n_frames 0", 161, buf, buf, 13, 23041, 0},    {"pcm NULL", 160, nullptr, buf, 13, 23040, 141},
                        {"out NULL", 160, buf, nullptr, 13, 23040, 141}, {"odd stride", 160, buf, buf, 13, 23041, 141},
                        {"odd hop", 161, buf, buf, 13, 23040, 2},       {"pcm + 4", 160, buf + 1, buf, 13, 23040, 141},
                        {"out + 4", 160, buf, buf + 1, 13, 23040, 141}, {"one frame too many", 160, buf, buf, 2, 1024, 5},
                        {"frames fit", 160, buf, buf, 2, 1024, 4},      {"2^31 frames", 2, buf, buf, int64_t(1) << 20, 5000, 2048},
                        {"2^31 - 1024 frames", 2, buf, buf, (int64_t(1) << 20) - 1, 5000, 2048}};
  const int n_calls = int(sizeof(calls) / sizeof(calls[0]));
  for (int i = 0; i < n_calls; ++i) {
    const Call& c = calls[i];
    std::string err;
    int64_t total = -1;
    const int rc = mel_call_check(c.hop, 512, c.pcm, c.out, c.n_clips, c.clip_stride, c.n_frames, total, err);
    CHECK((rc == kPlanOk) == err.empty(), "%s: a refusal carries a message", c.label);
    CHECK(total == (rc == kPlanOk ? c.n_clips * c.n_frames : 0) && total < (int64_t(1) << 31), "%s: total", c.label);
    printf("  {\"case\": \"%s\", \"rc\": %d, \"total\": %" PRId64 ", \"error\": ", c.label, rc, total);
    json_string(err);
    printf("}%s\n", i + 1 < n_calls ? "," : "");
  }

  // the launch of every route: [frames per block, groups, blocks, threads]
  printf(" ],\n \"launches\": [\n");
  const int routes[] = {1, 2, 3, 4, 8};
  const int64_t totals[] = {1, 15, 16, 17, 1833, (int64_t(1) << 31) - 1}, cus[] = {4, 64, 256};
  for (int r = 0; r < 5; ++r) {
    printf("  {\"route\": %d, \"grids\": [", routes[r]);
    for (int i = 0; i < 6; ++i)
      for (int c = 0; c < 3; ++c) {
        const MelLaunch l = mel_launch(routes[r], totals[i], cus[c]);
        CHECK(l.frames_per_block > 0 && l.groups * l.frames_per_block >= totals[i] &&
                  (l.groups - 1) * l.frames_per_block < totals[i], "route %d: the groups cover the frames", routes[r]);
        CHECK(l.blocks >= 1 && l.blocks <= l.groups && l.blocks < (int64_t(1) << 31) && l.threads % 64 == 0 &&
                  l.threads <= 1024, "route %d: grid", routes[r]);
        printf("%s[%d, %" PRId64 ", %" PRId64 ", %d]", i + c ? ", " : "", l.frames_per_block, l.groups, l.blocks, l.threads);
      }
    printf("]}%s\n", r < 4 ? "," : "");
  }
  printf(" ]\n}\n");
  return g_failed;
}
