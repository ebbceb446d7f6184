// Host side of the mel unit (hbk_mel.hip): the constants the kernels and their
// launcher share, the routing rule, every table a plan holds (one buffer, named
// offsets), the argument checks of a call and the launch grid of each route.
// Plain C++17 over the standard library: no HIP, no environment, no output; a
// refusal comes back as a status and a message. tests/mel_plan_check.cpp runs
// this header on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace hbk {
namespace {

// hbk_status of include/hbk.h (the unit asserts that they agree)
constexpr int kPlanOk = 0, kPlanErrArg = -1, kPlanErrUnsupported = -3;

inline std::string strf(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

inline int arg_fail(std::string& err, const char* what) {
  err = strf("hbk: invalid argument: %s", what);
  return kPlanErrArg;
}

inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// ---- constants of the kernels -------------------------------------------------
constexpr int kNfft = 512;
constexpr int kNfreq = kNfft / 2 + 1;     // bins 0..256
constexpr int kMaxTaps = 16;              // widest mel filter supported
constexpr int kMaxMels = 32;
constexpr int kFramesPerWave = 4;         // v1, v2, MFMA: 16 lanes per frame
// v1
constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kFramesPerBlock = kFramesPerWave * kWaves;
constexpr int kBlocksPerCU = 8;           // persistent grid: CUs x this
// v2: 32 mels on bins < kBins2; lane j computes filter j from kTapsA bins and filter 31 - j from kTapsB
constexpr int kTapsA = 8;                 // filters 0..15
constexpr int kTapsB = 16;                // filters 16..31
constexpr int kBins2 = 128;
constexpr int kWaves2 = 8;                // 512-thread blocks sharing one constant table
constexpr int kThreads2 = 64 * kWaves2;
constexpr int kFramesPerBlock2 = kFramesPerWave * kWaves2;
constexpr int kBlocksPerCU2 = 2;          // <= 128 VGPRs, 80 KB LDS: 4 waves / SIMD
// MFMA
constexpr int kWaves3 = 6;
constexpr int kThreads3 = 64 * kWaves3;
constexpr int kFramesPerBlock3 = kFramesPerWave * kWaves3;
constexpr int kBlocksPerCU3 = 2;
// SoA, W = 4 or 8 waves per block, 8 lanes per frame
constexpr int kFramesPerWave4 = 8;
constexpr int kBlocksPerCU4 = 3;          // W = 4: 3 x (35 KB frames + 6.5 KB table) of LDS, <= 168 VGPRs
constexpr int kBlocksPerCU8 = 2;          // W = 8: two 8-wave blocks share a CU's LDS
// ... its constant table [entry][8 lanes] of float4
constexpr int kE4Win = 0;                 // 16: (w[32 n1 + 2jj], w[.. + 16], w[.. + 1], w[.. + 17])
constexpr int kE4Tw = 16;                 // 16 (k1 = 0 unused): (Re W^(jj k1), Re W^((jj+8) k1), Im .., Im ..)
constexpr int kE4Ws = 32;                 // 8: -i W512^k for bins (ra + 16 k2, rb + 16 k2), re pair, im pair
constexpr int kE4Mel = 40;                // 12: weights of A slots jj, jj + 8 (8 each), B slots jj, jj + 8 (16 each)
constexpr int kE4N = 52;
static_assert(kE4Mel + 2 * (kTapsA + kTapsB) / 4 == kE4N, "the mel rows close the table");

// The filter of mel m in the v2 layout: its taps, and its slot in lo2 / w2 ([16] A slots, then
// [16] B slots: lane j's narrow filter j and wide filter 31 - j).
inline int v2_taps(int m) { return m < 16 ? kTapsA : kTapsB; }
inline int v2_lo_slot(int m) { return m < 16 ? m : 16 + (31 - m); }
inline int v2_w_offset(int m) { return m < 16 ? m * kTapsA : 16 * kTapsA + (31 - m) * kTapsB; }

// ---- routing --------------------------------------------------------------------
// The environment of one hbk_mel_plan_create call (read_mel_knobs in hbk_mel.hip).
struct MelKnobs {
  bool force_v1 = false;  // HBK_MEL_V1 set: the v1 kernel for every plan
  bool mfma = false;      // HBK_MEL_MFMA set: a v2 plan starts on variant 1
  int v4 = 0;             // HBK_MEL_V4: 0 off, else 4 or 8 waves per block of the SoA kernel
};

struct MelScalars {
  int taps = 0, nk2 = 0, need256 = 0;  // v1: filter width, 16-bin blocks read, bin 256 read
  int v2 = 0, edge0 = 0;               // the v2 layout fits; with it, a window zero on its first and last 32 samples
  int variant = 0, v4 = 0;             // v2 plans: the variant at creation; SoA waves per block
};

// The kernel hbk_mel_frames launches (hbk_mel_plan_info's numbering):
// 1 = v1, 2 = v2, 3 = MFMA, 4 / 8 = SoA with 4 / 8 waves per block.
inline int mel_route(const MelScalars& s, int variant) {
  if (!s.v2) return 1;
  if (variant == 1) return 3;
  if (s.v4) return s.v4 == 8 ? 8 : 4;
  return 2;
}

// ---- the tables -------------------------------------------------------------------
// One buffer, each table on a 256-B boundary:
//   win    float [512]           window x in_scale
//   tw256  float2 [256]          W256^i                          tw512  float2 [257]   W512^i
//   lo     int [n_mels]          v1 start bins, lo + taps <= 257  w      float [n_mels][taps]
// and for a v2 plan
//   twsm   float2 [128]          -i W512^k
//   lo2    int [32]              even start bins at v2_lo_slot(m), lo2 + T <= 128
//   w2     float [16][8] [16][16]  x 1/4, at v2_w_offset(m), zero outside the filter
//   fbt    float [32][128]       filterbank^T x 1/4 (MFMA)
//   t4     float4 [kE4N][8]      the SoA kernel's per-lane constants
enum MelTable { kMelWin, kMelTw256, kMelTw512, kMelLo, kMelW, kMelTwsm, kMelLo2, kMelW2, kMelFbt, kMelT4, kMelTableCount };

struct MelTables {
  MelScalars s;
  std::vector<float> host;            // the block (lo and lo2 hold ints)
  size_t off[kMelTableCount] = {};    // byte offset of each table
  size_t size[kMelTableCount] = {};   // its bytes; 0: the plan has no such table
  size_t bytes() const { return host.size() * sizeof(float); }
  float* f(MelTable t) { return host.data() + off[t] / sizeof(float); }
  const float* f(MelTable t) const { return host.data() + off[t] / sizeof(float); }
};

// (cos, sin)(-2 pi i / N), i < count: double cos / sin rounded to float
inline void twiddle_table(float* dst, int count, int N) {
  for (int i = 0; i < count; ++i) {
    const double ang = -2.0 * M_PI * i / double(N);
    dst[2 * i] = static_cast<float>(cos(ang));
    dst[2 * i + 1] = static_cast<float>(sin(ang));
  }
}

// -i W512^k = (sin, -cos)(-2 pi k / 512), k < kBins2
inline void split_twiddle_table(float* dst) {
  for (int k = 0; k < kBins2; ++k) {
    const double ang = -2.0 * M_PI * k / 512.0;
    dst[2 * k] = static_cast<float>(sin(ang));
    dst[2 * k + 1] = static_cast<float>(-cos(ang));
  }
}

// Start bin of mel m's T-tap read window in the v2 layout: even (8-B LDS pairs), inside
// [0, kBins2); -1 if the filter [lo, hi] does not fit it.
inline int v2_start(int m, int lo, int hi) {
  const int T = v2_taps(m);
  int l = lo & ~1;
  if (hi - l + 1 > T) return -1;
  if (l + T > kBins2) l = kBins2 - T;  // even: T is even
  return l;
}

// lo2 and w2 (weights x 1/4: the split's 1/2, squared) of a bank that fits
inline void v2_filter_tables(const float* fbank, int n_mels, const int* lo, const int* hi, int* lo2, float* w2) {
  for (int m = 0; m < n_mels; ++m) {
    const int l = v2_start(m, lo[m], hi[m]);
    lo2[v2_lo_slot(m)] = l;
    for (int t = 0; t < v2_taps(m); ++t) w2[v2_w_offset(m) + t] = 0.25f * fbank[(l + t) * n_mels + m];
  }
}

// the dense filterbank^T [32][kBins2] x 1/4
inline void fbt_table(const float* fbank, int n_mels, float* fbt) {
  for (int m = 0; m < kMaxMels; ++m)
    for (int k = 0; k < kBins2; ++k) fbt[m * kBins2 + k] = 0.25f * fbank[k * n_mels + m];
}

// The SoA kernel's table [entry][lane jj] of float4, from the tables the v2 kernel reads: lane jj owns
// columns jj and jj + 8 of the transform, rows (ra, rb) of its second stage and the filters of slots jj, jj + 8.
inline void t4_table(const float* win, const float* tw256, const float* twsm, const float* w2, float* t4) {
  auto put = [&](int entry, int jj, float x, float y, float z, float w) {
    float* d = t4 + 4 * (entry * 8 + jj);
    d[0] = x, d[1] = y, d[2] = z, d[3] = w;
  };
  for (int jj = 0; jj < 8; ++jj) {
    for (int n1 = 0; n1 < 16; ++n1) {
      const float* s = win + 32 * n1 + 2 * jj;
      put(kE4Win + n1, jj, s[0], s[16], s[1], s[17]);
    }
    for (int k1 = 1; k1 < 16; ++k1) {
      const float* a0 = tw256 + 2 * (jj * k1);
      const float* a1 = tw256 + 2 * ((jj + 8) * k1);
      put(kE4Tw + k1, jj, a0[0], a1[0], a0[1], a1[1]);
    }
    const int ra = jj == 0 ? 0 : jj, rb = jj == 0 ? 8 : 16 - jj;
    for (int k2 = 0; k2 < 8; ++k2) {
      const float* s0 = twsm + 2 * (ra + 16 * k2);
      const float* s1 = twsm + 2 * (rb + 16 * k2);
      put(kE4Ws + k2, jj, s0[0], s1[0], s0[1], s1[1]);
    }
    // mel rows: A slot jj (2 float4), A slot jj + 8 (2), B slot jj (4), B slot jj + 8 (4)
    const float* rows[4] = {w2 + jj * kTapsA, w2 + (jj + 8) * kTapsA, w2 + 16 * kTapsA + jj * kTapsB,
                            w2 + 16 * kTapsA + (jj + 8) * kTapsB};
    int entry = kE4Mel;
    for (int r = 0; r < 4; ++r)
      for (int q = 0; q < (r < 2 ? kTapsA : kTapsB) / 4; ++q, ++entry)
        put(entry, jj, rows[r][4 * q], rows[r][4 * q + 1], rows[r][4 * q + 2], rows[r][4 * q + 3]);
  }
}

// What hbk_mel_plan_create decides and uploads. fbank is [257][n_mels].
inline int mel_tables(const float* window, const float* fbank, int n_fft, int hop, int n_mels, float in_scale,
                      float log_floor, float out_div, float out_add, const MelKnobs& knobs, MelTables& t,
                      std::string& err) {
  (void)log_floor, (void)out_add;  // any value is a valid clamp / offset
  if (!window || !fbank) return arg_fail(err, "window/fbank is NULL");
  if (n_fft != kNfft) return arg_fail(err, "n_fft must be 512");
  if (hop <= 0) return arg_fail(err, "hop must be positive");
  if (n_mels <= 0 || n_mels > kMaxMels || (n_mels & 1)) return arg_fail(err, "n_mels must be even and <= 32");
  if (out_div == 0.f) return arg_fail(err, "out_div must be non-zero");

  // Sparse filterbank: each filter's non-zero bins form one contiguous run [lo, hi].
  std::vector<int> lo(n_mels, 0), hi(n_mels, -1);
  int taps = 1, top = 0;
  for (int m = 0; m < n_mels; ++m) {
    for (int k = 0; k < kNfreq; ++k) {
      if (fbank[k * n_mels + m] != 0.f) {
        if (hi[m] < 0) lo[m] = k;
        hi[m] = k;
      }
    }
    if (hi[m] < 0) lo[m] = hi[m] = 0;  // all-zero filter: weights stay 0
    taps = std::max(taps, hi[m] - lo[m] + 1);
    top = std::max(top, hi[m]);
  }
  bool v2 = n_mels == kMaxMels && top < kBins2 && !knobs.force_v1;
  for (int m = 0; v2 && m < n_mels; ++m) v2 = v2_start(m, lo[m], hi[m]) >= 0;
  if (taps > kMaxTaps) {
    err = strf("hbk: mel filter spans %d bins (> %d supported)", taps, kMaxTaps);
    return kPlanErrUnsupported;
  }

  t = MelTables();
  const size_t size[kMelTableCount] = {
      kNfft * sizeof(float),      256 * 2 * sizeof(float),       257 * 2 * sizeof(float),
      n_mels * sizeof(int),       size_t(n_mels) * taps * sizeof(float),
      kBins2 * 2 * sizeof(float), kMaxMels * sizeof(int),        16 * (kTapsA + kTapsB) * sizeof(float),
      size_t(kMaxMels) * kBins2 * sizeof(float),                 size_t(kE4N) * 8 * 4 * sizeof(float)};
  size_t bytes = 0;
  for (int i = 0; i < kMelTableCount; ++i) {
    t.off[i] = bytes;
    t.size[i] = i < kMelTwsm || v2 ? size[i] : 0;
    bytes += up256(t.size[i]);
  }
  t.host.assign(bytes / sizeof(float), 0.f);

  for (int i = 0; i < kNfft; ++i) t.f(kMelWin)[i] = window[i] * in_scale;
  twiddle_table(t.f(kMelTw256), 256, 256);
  twiddle_table(t.f(kMelTw512), 257, 512);
  // v1: every filter reads `taps` bins from lo, moved down where that would pass bin 256
  float* w = t.f(kMelW);
  int kmax = 0;
  for (int m = 0; m < n_mels; ++m) {
    const int l = std::min(lo[m], kNfreq - taps);
    std::memcpy(t.f(kMelLo) + m, &l, sizeof(int));
    for (int k = 0; k < taps; ++k) w[m * taps + k] = fbank[(l + k) * n_mels + m];
    kmax = std::max(kmax, l + taps - 1);
  }
  t.s.taps = taps;
  t.s.need256 = kmax >= 256 ? 1 : 0;
  t.s.nk2 = std::min(16, (std::min(kmax, 255) + 16) / 16);
  if (!v2) return kPlanOk;

  bool edge0 = true;
  for (int i = 0; i < 32; ++i) edge0 = edge0 && window[i] == 0.f && window[n_fft - 1 - i] == 0.f;
  t.s.v2 = 1;
  t.s.edge0 = edge0 ? 1 : 0;
  t.s.variant = knobs.mfma ? 1 : 0;
  t.s.v4 = knobs.v4;
  split_twiddle_table(t.f(kMelTwsm));
  int lo2[kMaxMels];
  v2_filter_tables(fbank, n_mels, lo.data(), hi.data(), lo2, t.f(kMelW2));
  std::memcpy(t.f(kMelLo2), lo2, sizeof(lo2));
  fbt_table(fbank, n_mels, t.f(kMelFbt));
  t4_table(t.f(kMelWin), t.f(kMelTw256), t.f(kMelTwsm), t.f(kMelW2), t.f(kMelT4));
  return kPlanOk;
}

// ---- one hbk_mel_frames call -----------------------------------------------------------
// The argument checks. total: the frames of the call; 0 with kPlanOk: nothing to do.
inline int mel_call_check(int hop, int n_fft, const void* pcm, const void* out, int64_t n_clips, int64_t clip_stride,
                          int64_t n_frames, int64_t& total, std::string& err) {
  total = 0;
  if (n_clips < 0 || n_frames < 0) return arg_fail(err, "negative size");
  if (n_clips == 0 || n_frames == 0) return kPlanOk;
  if (!pcm || !out) return arg_fail(err, "pcm/out is NULL");
  if ((clip_stride & 1) || (hop & 1)) return arg_fail(err, "clip_stride and hop must be even (float2 loads)");
  if ((reinterpret_cast<uintptr_t>(pcm) & 7) || (reinterpret_cast<uintptr_t>(out) & 7))
    return arg_fail(err, "pcm/out must be 8-byte aligned");
  if (hop * (n_frames - 1) + n_fft > clip_stride) return arg_fail(err, "frames exceed clip_stride");
  if (n_clips * n_frames >= (int64_t(1) << 31)) return arg_fail(err, "more than 2^31 frames in one call");
  total = n_clips * n_frames;
  return kPlanOk;
}

struct MelLaunch {
  int frames_per_block = 0;  // a group: the frames one block transforms per round of its loop
  int64_t groups = 0;
  int64_t blocks = 0;        // persistent grid: min(groups, CUs x the route's blocks per CU)
  int threads = 0;
};

// cus: the CUs the stream may use
inline MelLaunch mel_launch(int route, int64_t total_frames, int64_t cus) {
  struct Shape {
    int frames, per_cu, threads;
  };
  const Shape s = route == 1   ? Shape{kFramesPerBlock, kBlocksPerCU, kThreads}
                  : route == 2 ? Shape{kFramesPerBlock2, kBlocksPerCU2, kThreads2}
                  : route == 3 ? Shape{kFramesPerBlock3, kBlocksPerCU3, kThreads3}
                  : route == 4 ? Shape{kFramesPerWave4 * 4, kBlocksPerCU4, 64 * 4}
                               : Shape{kFramesPerWave4 * 8, kBlocksPerCU8, 64 * 8};
  MelLaunch l;
  l.frames_per_block = s.frames;
  l.groups = (total_frames + s.frames - 1) / s.frames;
  l.blocks = std::min<int64_t>(l.groups, cus * s.per_cu);
  l.threads = s.threads;
  return l;
}

}  // namespace
}  // namespace hbk
