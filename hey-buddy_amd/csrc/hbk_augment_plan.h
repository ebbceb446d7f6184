// Host side of the augmentation units (hbk_augment.hip, hbk_clip_ops.hip,
// hbk_pitch.hip): the constants the kernels and their launchers share, the
// pitch shift's geometry, workspace layout and launch grids, the band-stop and
// colored-noise workspace layouts, and the reverb plan's twiddle tables. Plain
// C++17 over the standard library: no HIP, no environment, no output; a refusal
// comes back as a status and a message. tests/augment_plan_check.cpp runs this
// header on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

namespace hbk {
namespace {

// hbk_status of include/hbk.h (the units assert that they agree)
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

inline int64_t up256(int64_t b) { return (b + 255) & ~int64_t(255); }

// ---- the reverb family ------------------------------------------------------
constexpr int kT = 23040;        // clip length (1.44 s @ 16 kHz, augmented.py:31)
constexpr int kM = kT / 2;       // complex FFT length
constexpr int kThreads = 1024;   // 16 waves: one clip per CU (92 KB of LDS)
constexpr int kN1 = 16000;       // colored noise: torch_audiomentations' noise length = sample_rate
constexpr int kM1 = kN1 / 2;     // 8000

// Two-level twiddle table in LDS: W_M^e = hi[e >> 7] * lo[e & 127], e < kM.
constexpr int kTwLo = 128, kTwHi = kM / kTwLo;  // 128 x 90
static_assert(kTwLo * kTwHi == kM, "twiddle split");
// ... of the 8000-point transform: W_8000^e = HI8[e / 100] LO8[e % 100]
constexpr int kTw8Lo = 100, kTw8Hi = kM1 / kTw8Lo;  // 100 x 80
static_assert(kTw8Lo * kTw8Hi == kM1, "twiddle split");

// spectrum / W_N^k slot of bin k <= kM: [k % 16][k / 16] (HBK_REVERB_SPECTRUM_SLOTS):
// the pair loop's lanes walk k in steps of 16, i.e. consecutive slots
constexpr int kHRow = kM / 16 + 1;  // 721
constexpr int kHSlots = 16 * kHRow;

constexpr int kBsHalf = kT / 2;             // outputs per overlap-save block
constexpr int kBsPart = kT - kBsHalf + 1;   // 11521 taps per partition (HBK_BAND_STOP_PARTITION_TAPS)
constexpr int kBsCirc = 512;                // HBK_BAND_STOP_CIRCULAR_MAX_HALF
static_assert(2 * kBsCirc <= kThreads, "one edge sample per thread");

// dynamic LDS (sizeof(float2) = 8): z, the reduction slots, the two twiddle tables
constexpr size_t kAugLds = (size_t(2 * kM + 32) * sizeof(float)) + (kTwHi + kTwLo) * 8;
constexpr size_t kBandStopLds = kAugLds + (5 * kBsCirc + 1) * sizeof(float);  // + taps g[0..h], the edges
constexpr size_t kColoredLds = (size_t(2 * kM1 + 32) * sizeof(float)) + (kTw8Hi + kTw8Lo) * 8;

// ---- pitch shift ------------------------------------------------------------
constexpr int kPsFft = 250, kPsHop = 7, kPsBins = kPsFft / 2 + 1, kPsPad = kPsFft / 2;
constexpr int kPsTapMax = 144;                         // HBK_PITCH_SHIFT_MAX_TAPS: 2 width + orig (142 / 139 at 16 kHz)
constexpr int kPsPhaseMax = 128;                       // new (resampler phases)
constexpr int kPsResFrames = 32;                       // resampler frames per workgroup
#ifndef HBK_PV_CLIPS
#define HBK_PV_CLIPS 2  // measured: 1.79 us/clip at 2, 1.95 at 4, 2.33 at 1 (12,800 clips)
#endif
constexpr int kPvClips = HBK_PV_CLIPS;                 // clips per workgroup (128 lanes each)
constexpr int kPvGroup = 8;                            // output frames per istft step (lane 8u + .: frame u)
constexpr int kPvRows = 64;                            // input frames of d rows held in LDS
constexpr int kPvGh = 64;                              // ring of G(t, .) rows (>= 36 + kPvGroup)
constexpr int kRsFrames = 64, kRsK = 160, kRsLd = kRsK + 8;  // the MFMA resampler: 336-B rows (odd 16-B count)
static_assert(kPsTapMax <= kRsK && kPsPhaseMax <= 128, "the MFMA resampler's K padding and 8 phase tiles");

struct PitchGeometry {
  int L = 0, f_in = 0, f_out = 0, l1 = 0, orig = 0, nw = 0, width = 0, target = 0;
  double rate = 0;
};

// The frame and resampler geometry of one call, or why the kernels do not run it.
inline int pitch_geometry(int64_t L, int32_t sample_rate, int32_t num, int32_t den, PitchGeometry& a,
                          std::string& err) {
  if (sample_rate != 16000) {
    err = strf("hbk: pitch shift supports 16 kHz (n_fft 250, hop 7), got %d", sample_rate);
    return kPlanErrUnsupported;
  }
  if (num <= 0 || den <= 0) return arg_fail(err, "shift num / den must be positive");
  if (L <= kPsPad || L > (int64_t(1) << 24)) return arg_fail(err, "clip length must be in (125, 2^24]");
  a.L = static_cast<int>(L);
  a.rate = double(den) / double(num);
  a.f_in = 1 + a.L / kPsHop;
  a.f_out = static_cast<int>(std::ceil(double(a.f_in) / a.rate));
  a.l1 = kPsHop * (a.f_out - 1);
  const int64_t new_sr = int64_t(sample_rate) * den / num;
  const int64_t g = std::gcd(int64_t(sample_rate), new_sr);
  if (new_sr <= 0 || g <= 0) return arg_fail(err, "shift out of range");
  a.orig = static_cast<int>(sample_rate / g);
  a.nw = static_cast<int>(new_sr / g);
  a.width = static_cast<int>(std::ceil(6.0 * a.orig / (std::min(a.orig, a.nw) * 0.99)));
  a.target = static_cast<int>(std::ceil(double(a.nw) * a.l1 / a.orig));
  if (a.nw > kPsPhaseMax || 2 * a.width + a.orig > kPsTapMax || a.l1 <= 0) {
    err = strf("hbk: pitch shift %d/%d resamples %d -> %d (%d taps): the kernel holds <= %d phases of <= %d taps "
               "(torch_pitch_shift's fast shifts at 16 kHz)", num, den, a.orig, a.nw, 2 * a.width + a.orig,
               kPsPhaseMax, kPsTapMax);
    return kPlanErrUnsupported;
  }
  // ps_vocoder_kernel advances the source frame by at most two per output frame (so a group of kPvGroup
  // output frames reads at most 2 kPvGroup + 2 new source frames); torch_pitch_shift.get_fast_shifts
  // keeps ratios in [0.5, 2], so the reference never asks for more
  static_assert(2 * kPvGroup + 3 <= kPvRows, "the d rows of a group at rate 2");
  if (a.rate > 2.0) {
    err = strf("hbk: pitch shift %d/%d has rate %g > 2: the vocoder steps at most two source frames per output "
               "frame (torch_pitch_shift keeps ratios in [0.5, 2])", num, den, a.rate);
    return kPlanErrUnsupported;
  }
  return kPlanOk;
}

// Byte offsets of the workspace's regions (each 256-B aligned) for n listed clips.
struct PitchLayout {
  int64_t y = 0;     // float [n][l1]: the istft output
  int64_t taps = 0;  // float [kPsPhaseMax][kPsTapMax]
  int64_t yr = 0;    // int2 [n]: the clips' computed y ranges
  int64_t sp = 0;    // span pairing: int2 [n], the clips' spans,
  int64_t key = 0;   //   uint64 [n] (then [groups]), the sort keys,
  int64_t ord = 0;   //   int32 [n], the clips' order
  int64_t gord = 0;  //   int32 [groups], and the groups'
  int64_t total = 0;
};

inline PitchLayout pitch_layout(const PitchGeometry& a, int64_t n) {
  PitchLayout w;
  w.y = 0;
  w.taps = up256(n * a.l1 * 4);
  w.yr = w.taps + up256(int64_t(kPsPhaseMax) * kPsTapMax * 4);
  w.sp = w.yr + up256(n * 8);
  w.key = w.sp + up256(n * 8);
  w.ord = w.key + up256(n * 8);
  w.gord = w.ord + up256(n * 4);
  w.total = w.gord + up256(n * 4);
  return w;
}

// The environment of one hbk_pitch_shift call (read_pitch_knobs in hbk_pitch.hip).
struct PitchKnobs {
  bool span = true;            // HBK_PS_SPAN=0: every frame of every clip, the full resampler (A/B)
  bool pair = true;            // HBK_PS_PAIR=0: workgroups take list neighbours and scan their own rows (A/B)
  bool resample_valu = false;  // HBK_PS_RESAMPLE_VALU: the f32 VALU resampler (A/B)
};

struct Grid {
  unsigned x = 1, y = 1, block = 0;
};

// Every launch of one call, in stream order: taps; with pairing span, rank (clips), group, rank (groups);
// vocoder; one of the two resamplers.
struct PitchLaunches {
  bool pair = false;  // without spans there is nothing to pair by
  int groups = 0;     // vocoder workgroups
  Grid taps, span, rank_clips, group, rank_groups, vocoder, resample;
  bool resample_mfma = true;
};

inline PitchLaunches pitch_launches(const PitchGeometry& a, int64_t n, const PitchKnobs& k) {
  PitchLaunches p;
  p.pair = k.span && k.pair;
  p.groups = static_cast<int>((n + kPvClips - 1) / kPvClips);
  p.taps = Grid{unsigned((a.nw * kPsTapMax + 255) / 256), 1, 256};
  p.span = Grid{unsigned((n + 3) / 4), 1, 256};
  p.rank_clips = Grid{unsigned((n + 63) / 64), 1, 1024};
  p.group = Grid{unsigned((p.groups + 255) / 256), 1, 256};
  p.rank_groups = Grid{unsigned((p.groups + 63) / 64), 1, 1024};
  p.vocoder = Grid{unsigned(p.groups), 1, unsigned(128 * kPvClips)};
  const int res_frames = (a.L + a.nw - 1) / a.nw;
  p.resample_mfma = !(k.resample_valu || a.nw > 128);
  p.resample = p.resample_mfma ? Grid{unsigned((res_frames + kRsFrames - 1) / kRsFrames), unsigned(n), 256}
                               : Grid{unsigned((res_frames + kPsResFrames - 1) / kPsResFrames), unsigned(n), 128};
  return p;
}

// ---- band-stop and colored-noise workspaces ----------------------------------
struct BandStopLayout {
  int64_t sums = 0;     // float2 [n_filters]: the two lowpass sums
  int64_t taps = 0;     // float [n_filters][kBsCirc + 1]: g[0..h] of circular filters
  int64_t spectra = 0;  // float2 [n_spectra][kHSlots]
  int64_t scratch = 0;  // float [blocks][kT]: overlap-save clips
  int64_t total = 0;
};

// blocks: the clip kernel's grid. n <= 0: no workspace.
inline BandStopLayout band_stop_layout(int64_t n, int32_t n_filters, int32_t n_spectra, int64_t blocks) {
  BandStopLayout w;
  if (n <= 0) return w;
  w.taps = w.sums + up256(int64_t(n_filters) * 8);
  w.spectra = w.taps + up256(int64_t(n_filters) * (kBsCirc + 1) * 4);
  w.scratch = w.spectra + int64_t(n_spectra) * kHSlots * 8;
  w.total = w.scratch + blocks * kT * 4;
  return w;
}

struct ColoredLayout {
  int64_t groups = 0;  // 0: every clip colours its own second, no workspace
  int64_t gbuf = 0;    // float [groups][kN1]: the coloured second x kM1
  int64_t grms = 0;    // float [groups]
  int64_t total = 0;
};

inline ColoredLayout colored_layout(int64_t n_clips, int64_t clips_per_noise) {
  ColoredLayout w;
  w.groups = clips_per_noise > 1 && n_clips > 0 ? (n_clips + clips_per_noise - 1) / clips_per_noise : 0;
  if (!w.groups) return w;
  w.grms = w.groups * kN1 * int64_t(sizeof(float));
  w.total = w.grms + up256(w.groups * int64_t(sizeof(float)));
  return w;
}

// ---- the reverb plan's tables --------------------------------------------------
// Six tables of (cos, sin) pairs in one buffer, each on a 256-B boundary:
//   hi   W_M^(128 h), h < 90        lo   W_M^l, l < 128        n    W_N^k, k <= kM, at [k % 16][k / 16]
//   hi8  W_8000^(100 h), h < 80     lo8  W_8000^l, l < 100     n16  W_16000^k, k <= 4000
// Double cos / sin rounded to float; the slots of n that no bin maps to are zero.
enum ReverbTable { kTabHi, kTabLo, kTabN, kTabHi8, kTabLo8, kTabN16, kTabCount };

struct ReverbTables {
  std::vector<float> host;       // the block, (re, im) pairs
  size_t off[kTabCount] = {};    // byte offset of each table
  size_t pairs[kTabCount] = {};  // its length in pairs (slots, for n)
  size_t bytes() const { return host.size() * sizeof(float); }
};

// W_N^(step i), i < count, at pair i (slotted: at (i % 16) * kHRow + i / 16)
inline void twiddle_table(float* dst, int count, int step, int N, bool slotted) {
  for (int i = 0; i < count; ++i) {
    const double a = -2.0 * M_PI * (double(i) * step) / double(N);
    float* p = dst + 2 * size_t(slotted ? (i % 16) * kHRow + i / 16 : i);
    p[0] = float(cos(a));
    p[1] = float(sin(a));
  }
}

inline ReverbTables reverb_tables() {
  struct Spec {
    int count, step, N, pairs;
    bool slotted;
  };
  const Spec spec[kTabCount] = {
      {kTwHi, kTwLo, kM, kTwHi, false},        {kTwLo, 1, kM, kTwLo, false},      {kM + 1, 1, kT, kHSlots, true},
      {kTw8Hi, kTw8Lo, kM1, kTw8Hi, false},    {kTw8Lo, 1, kM1, kTw8Lo, false},   {kM1 / 2 + 1, 1, kN1, kM1 / 2 + 1, false},
  };
  ReverbTables t;
  size_t bytes = 0;
  for (int i = 0; i < kTabCount; ++i) {
    t.off[i] = bytes;
    t.pairs[i] = size_t(spec[i].pairs);
    bytes += size_t(up256(int64_t(spec[i].pairs) * 8));
  }
  t.host.assign(bytes / sizeof(float), 0.f);
  for (int i = 0; i < kTabCount; ++i)
    twiddle_table(t.host.data() + t.off[i] / sizeof(float), spec[i].count, spec[i].step, spec[i].N, spec[i].slotted);
  return t;
}

}  // namespace
}  // namespace hbk
