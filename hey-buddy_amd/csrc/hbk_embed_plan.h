// Host planner of the speech-embedding conv stack: maps (ops, window size,
// window starts, precision, knobs) to an EmbedHostPlan — per chain the kernel
// choice as a value, its argument struct with null device pointers, the packed
// weight / bias / table bytes and the launch geometry — and every planning
// error, before any device call. Plain C++17 over hbk_embed_args.h and the
// standard library: no HIP, no environment, no output. hbk_embed.hip realises a
// plan on the device (the kernels a KernelChoice names are in the family units,
// hbk_embed_internal.h); tests/embed_plan_check.cpp runs this header on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <numeric>
#include <optional>
#include <string>
#include <variant>
#include <vector>

#include "hbk_embed_args.h"

namespace hbk {
namespace {

// hbk_status and hbk_op_kind of include/hbk.h (hbk_embed.hip asserts that they agree)
constexpr int kPlanOk = 0, kPlanErrArg = -1, kPlanErrUnsupported = -3;
constexpr int kOpConv = 0, kOpMaxPool = 1;

// The environment of one plan creation (read_embed_knobs in hbk_embed.hip, the host unit).
struct EmbedKnobs {
  bool lds_kb_set = false;  // HBK_EMBED_LDS_KB: LDS per block of the split-f16 kernel (16 .. 160), for tuning
  int lds_kb = 0;
  int weights = 0;          // HBK_EMBED_WEIGHTS: 1 lds, 2 global, else by halo cost
  bool no_p0 = false, no_p0s = false, no_p1 = false, no_p1s = false, no_p2s = false, no_t3s = false;
  bool no_dedup = false;    // HBK_EMBED_NO_DEDUP: per-window tail
  int p0_band = 6;          // HBK_P0_BAND: pooled rows per task of the banded p0 kernel (5 | 7, else 6)
  bool debug = false;       // HBK_DEBUG_EMBED: the plan's lines on stderr
  int debug_skip = 0;       // HBK_DEBUG_SKIP (profiling builds)
};

struct OpIn {  // hbk_graph_op
  int kind, kh, kw, cin, cout, act;
  float alpha;
  const float *weight, *bias;
};

struct OpInfo {
  int kind, kh, kw, cin, cout, act;
  float alpha;
  std::vector<float> w, b;  // HWIO, [cout]
};

struct Dims {
  int h, w, c;
};

enum class Kern { exact, x3, p0_band, p0s, p1, p1s, p2s, t3s };

// A kernel as a value. exact: n = output-channel blocks (NB), flag = weights
// read from global memory (WG); x3: n = NBMAX, flag = WG; p0_band: n = band;
// the pattern kernels: flag = LeakyReLU.
struct KernelChoice {
  Kern kind;
  int n;
  bool flag;
};

using KernelArgs = std::variant<ChainArgs, XArgs, P0Args, P1Args, P2sArgs, T3sArgs>;

// One kernel of one chain, ready to upload and launch.
struct Launch {
  KernelChoice kernel{Kern::exact, 1, false};
  KernelArgs args;            // device pointers null; ptr_off says where they will point
  const char* name = "";      // for the launch check
  int threads = 0;
  size_t lds_bytes = 0;       // dynamic LDS
  int imgs_per_task = 1;      // tasks = ceil(n_img / imgs_per_task) * n_bands
  int n_bands = 1;
  // pattern kernels run only on 16-B aligned buffers with a source stride that
  // is a multiple of 4 floats, and:
  bool tasks_below_2_31 = false;  // n_img * n_bands < 2^31
  int64_t min_src_stride = 0;     // source stride >= this many floats
  int64_t out_stride_4 = 0;       // this output stride is a multiple of 4 floats
  std::vector<unsigned char> blob;  // one device allocation
  size_t ptr_off[4] = {0, 0, 0, 0}; // exact: wblob; x3: wblob, bblob, ktab, i2c_off; patterns: w, bias
  std::string debug;          // the HBK_DEBUG_EMBED line (patterns: up to the device's blocks / CU)
};

struct ChainHost {
  Launch base;                    // the exact-f32 or the split-f16 (x3) kernel
  std::optional<Launch> pattern;  // the pattern kernel the chain matches; base is its fall-back at launch
  int src_buf = -1;               // -1: the call's input, else workspace buffer index
  int dst_buf = -1;               // -1: the call's output
  int ipc = 1;                    // images per source clip
  int64_t src_clip_stride = 0, out_img_stride = 0;
  int64_t out_floats = 0;        // per source clip (clip path) or per window
  double macs_per_img = 0;        // algorithmic MACs per image of this chain
  int64_t imgs_per_unit = 1;      // images per clip (clip program) or window
};

struct ProgramPlan {
  std::vector<ChainHost> chains;
  int64_t buf_floats[2] = {0, 0};  // ping-pong workspace buffers, per unit (clip or window)
  // phase-deduplicated tail: the last chain writes [n_src rows][out_dim] per clip
  // into workspace buffer gather_buf; output row i is source row gather_src[i]
  int gather_buf = -1, n_src = 0;
  std::vector<int> gather_src;
};

struct EmbedHostPlan {
  int in_h = 0, in_w = 0, out_dim = 0, n_win = 0;
  bool split_f16 = true;
  int n_prefix = 0;      // the split point: ops before it run once per clip
  int split_stride = 1;  // cumulative time stride at the split
  int seq_frames = 0;
  double prefix_macs = 0, tail_macs = 0;
  ProgramPlan clip, win;
  std::string dedup_debug;  // the "hbk tail dedup" line
  std::string error;        // of a failed plan_embed
};

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

// hi = v rounded toward zero to 11 bits, as on the device; lo = v - hi (exact in f32), rounded to fp16
struct HiLo {
  _Float16 hi, lo;
};
inline HiLo split_f16(float v) {
  uint32_t bits;
  memcpy(&bits, &v, 4);
  bits &= 0xFFFFE000u;
  float hv;
  memcpy(&hv, &bits, 4);
  return {static_cast<_Float16>(hv), static_cast<_Float16>(v - hv)};
}
inline void put_split(std::vector<_Float16>& w, size_t at, size_t lo, float v) {
  const HiLo s = split_f16(v);
  w[at] = s.hi;
  w[at + lo] = s.lo;
}

inline size_t pad16(size_t bytes) { return (bytes + 15) & ~size_t(15); }

// The source / pooling side of a chain, filled by plan_segment.
struct ChainIo {
  int ipc;
  int row_off[kMaxWin];
  int64_t src_clip_stride;
  int src_row_stride;
  int C_src, in_ph, in_pw, W_in, out_ph, out_pw;
};

template <class A>  // ChainArgs or XArgs
void set_io(A& a, const ChainIo& io) {
  a.ipc = io.ipc;
  for (int k = 0; k < kMaxWin; ++k) a.row_off[k] = io.row_off[k];
  a.src_clip_stride = io.src_clip_stride;
  a.src_row_stride = io.src_row_stride;
  a.C_src = io.C_src;
  a.in_ph = io.in_ph;
  a.in_pw = io.in_pw;
  a.W_in = io.W_in;
  a.out_ph = io.out_ph;
  a.out_pw = io.out_pw;
}

inline int odd_pad(int c) { return (c % 2 == 0) ? c + 1 : c; }

// Exact-f32 layout of one chain: packs the weights and biases and picks
// images-per-task and band for the LDS budget.
inline int layout_exact(const std::vector<OpInfo>& ops, const std::vector<int>& stage_ops, Dims d, const ChainIo& io,
                        Launch& L, Dims& od_out, double& macs_out, std::string& err) {
  ChainArgs a{};
  set_io(a, io);
  int nb = 1;
  int cin = d.c, h = d.h, w = d.w;
  a.n_stages = static_cast<int>(stage_ops.size());
  a.shrink = 0;
  double macs = 0;
  for (int s = 0; s < a.n_stages; ++s) {
    const OpInfo& op = ops[stage_ops[s]];
    if (op.cin != cin) {
      err = strf("hbk: graph channel mismatch at op %d (%d != %d)", stage_ops[s], op.cin, cin);
      return kPlanErrArg;
    }
    StageDesc& S = a.st[s];
    S.kh = op.kh;
    S.kw = op.kw;
    S.cin = op.cin;
    S.cinp = odd_pad(op.cin);
    S.cout = op.cout;
    S.coutp = odd_pad(op.cout);
    S.K = op.kh * op.kw * op.cin;
    S.ksteps = (S.K + 3) / 4;
    S.act = op.act;
    S.alpha = op.alpha;
    nb = std::max(nb, (op.cout + 15) / 16);
    a.shrink += op.kh - 1;
    h -= op.kh - 1;
    w -= op.kw - 1;
    if (h <= 0 || w <= 0) {
      err = strf("hbk: graph collapses the image at op %d", stage_ops[s]);
      return kPlanErrArg;
    }
    macs += double(h) * w * op.cout * S.K;
    cin = op.cout;
  }
  a.wstride = nb * 16 + ((nb * 16) % 32 == 0 ? 16 : 0);  // kq rows on different bank halves
  // pack weights: per stage [ksteps*4][wstride] then bias [nb*16]
  std::vector<float> blob;
  int max_k = 0;
  for (int s = 0; s < a.n_stages; ++s) {
    const OpInfo& op = ops[stage_ops[s]];
    StageDesc& S = a.st[s];
    S.w_off = static_cast<int>(blob.size());
    const int rows = S.ksteps * 4;
    blob.resize(blob.size() + size_t(rows) * a.wstride, 0.f);
    for (int k = 0; k < S.K; ++k)
      for (int n = 0; n < op.cout; ++n) blob[S.w_off + size_t(k) * a.wstride + n] = op.w[size_t(k) * op.cout + n];
    max_k = std::max(max_k, rows);
  }
  for (int s = 0; s < a.n_stages; ++s) {
    const OpInfo& op = ops[stage_ops[s]];
    a.st[s].b_off = static_cast<int>(blob.size());
    for (int n = 0; n < nb * 16; ++n) blob.push_back(n < op.cout ? op.b[n] : 0.f);
  }
  a.wblob_floats = static_cast<int>(blob.size());
  const Dims od{h / a.out_ph, w / a.out_pw, cin};
  a.H_out = od.h;
  a.W_out = od.w;
  a.C_out = od.c;
  a.out_img_stride = int64_t(od.h) * od.w * od.c;
  if (od.h <= 0 || od.w <= 0) {
    err = "hbk: pooling collapses the image";
    return kPlanErrArg;
  }
  // LDS (floats): tensor t (stage t input; t = n_stages: last output) alternates X / Y
  auto regions = [&](int G, int band, int64_t& xf, int64_t& yf) {
    int rows = band * a.out_ph;  // rows of the last conv output
    std::vector<int64_t> t(a.n_stages + 1);
    for (int s = a.n_stages - 1; s >= 0; --s) {
      int wo = d.w;
      for (int q = 0; q <= s; ++q) wo -= a.st[q].kw - 1;
      t[s + 1] = int64_t(G) * rows * wo * a.st[s].coutp;
      rows += a.st[s].kh - 1;
    }
    t[0] = int64_t(G) * rows * d.w * a.st[0].cinp;
    xf = yf = 0;
    for (int s = 0; s <= a.n_stages; ++s) (s % 2 == 0 ? xf : yf) = std::max(s % 2 == 0 ? xf : yf, t[s]);
    xf = (xf + 3) & ~3;
    yf = (yf + 3) & ~3;
  };
  const int64_t k_floats = (max_k + 3) & ~3;
  auto lds_floats = [&](int G, int band, bool resident) -> int64_t {
    int64_t xf, yf;
    regions(G, band, xf, yf);
    return xf + yf + (resident ? ((a.wblob_floats + 3) & ~3) : 0) + k_floats;
  };
  // choose G (images per task) and band (output rows per task) for the LDS budget
  const int64_t budget = kLdsBudget / 4;
  const bool resident = lds_floats(1, 1, true) <= budget;
  int band = 0, G = 1;
  for (int b = od.h; b >= 1; --b)
    if (lds_floats(1, b, resident) <= budget) { band = b; break; }
  if (band == 0) {
    err = "hbk: one output row of a chain does not fit in LDS";
    return kPlanErrUnsupported;
  }
  if (band == od.h)
    while (G < 64 && lds_floats(G * 2, band, resident) <= budget) G *= 2;
  a.G = G;
  a.band = band;
  a.n_bands = (od.h + band - 1) / band;
  int64_t xf, yf;
  regions(G, band, xf, yf);
  a.lds_x = 0;
  a.lds_y = static_cast<int>(xf);
  a.lds_w = a.lds_y + static_cast<int>(yf);
  a.lds_k = a.lds_w + (resident ? ((a.wblob_floats + 3) & ~3) : 0);
  L.kernel = {Kern::exact, nb, !resident};  // > 6 blocks: the 6-block kernel loops over channel groups
  L.name = "conv_chain_kernel";
  L.threads = kThreads;
  L.lds_bytes = size_t(a.lds_k + k_floats) * 4;
  L.imgs_per_task = G;
  L.n_bands = a.n_bands;
  L.blob.resize(blob.size() * sizeof(float));
  memcpy(L.blob.data(), blob.data(), L.blob.size());
  L.args = a;
  od_out = od;
  macs_out = macs;
  return kPlanOk;
}

// fp16 elements per position for c channels: rounded up to 8, with an odd
// number of 16-B groups (conflict-free ds_read_b128 over consecutive positions).
inline int x_cs(int c) {
  int cs = (c + 7) & ~7;
  if ((cs / 8) % 2 == 0) cs += 8;
  return cs;
}

// Split-f16 layout of one chain: packs the fp16 weight planes, biases and
// group-offset tables, and picks images-per-task and band for the LDS budget.
inline int layout_split(const std::vector<OpInfo>& ops, const std::vector<int>& stage_ops, Dims d, const ChainIo& io,
                        const EmbedKnobs& knobs, Launch& L, Dims& od_out, double& macs_out, std::string& err) {
  XArgs x{};
  // LDS per block (default 78 KB: two blocks per CU); HBK_EMBED_LDS_KB for tuning
  // (a chain that fits fewer than kMinG whole images per task at that budget
  // takes a whole CU instead: measured on SE20's chain 2, 2 -> 6 images,
  // 0.96 -> 0.81 ms per 16384 clips; the tail chain, 30 images, keeps 2 / CU)
  constexpr int kMinG = 8;
  int64_t lds_budget = kLdsBudget;
  if (knobs.lds_kb_set) lds_budget = std::min<int64_t>(160, std::max(16, knobs.lds_kb)) * 1024;
  set_io(x, io);
  x.n_stages = static_cast<int>(stage_ops.size());
  x.shrink = 0;
  x.im2col = (d.c % 8) != 0;

  std::vector<_Float16> wb;  // hi/lo planes per stage
  std::vector<float> bb;
  std::vector<int> kt;
  int cin = d.c, h = d.h, w = d.w, nbmax = 1;
  double macs = 0;
  for (int s = 0; s < x.n_stages; ++s) {
    const OpInfo& op = ops[stage_ops[s]];
    if (op.cin != cin) {
      err = strf("hbk: graph channel mismatch at op %d (%d != %d)", stage_ops[s], op.cin, cin);
      return kPlanErrArg;
    }
    XStage& S = x.st[s];
    S.kh = op.kh;
    S.kw = op.kw;
    S.cin = op.cin;
    S.cout = op.cout;
    S.coutr = (op.cout + 7) & ~7;
    S.act = op.act ? ((op.alpha >= 0.f && op.alpha <= 1.f) ? 1 : 2) : 0;
    S.alpha = op.alpha;
    const bool i2c = x.im2col && s == 0;
    const int K0 = op.kh * op.kw * op.cin;
    const int cin8 = (op.cin + 7) & ~7;
    const int groups = i2c ? (K0 + 7) / 8 : op.kh * op.kw * cin8 / 8;
    S.cs_in = i2c ? x_cs(K0) : x_cs(op.cin);
    S.cs_out = x_cs(op.cout);
    S.ksteps = (groups + 1) / 2;
    S.nblk = (op.cout + 31) / 32;
    nbmax = std::max(nbmax, S.nblk);
    S.wrow = S.ksteps * 16 + 8;
    const int wo_in = w;  // this stage's input width (group offsets)
    h -= op.kh - 1;
    w -= op.kw - 1;
    x.shrink += op.kh - 1;
    if (h <= 0 || w <= 0) {
      err = strf("hbk: graph collapses the image at op %d", stage_ops[s]);
      return kPlanErrArg;
    }
    macs += double(h) * w * op.cout * K0;
    // weights [n][k] (k = group * 8 + j), hi then lo plane
    const int rows = S.nblk * 32;
    S.w_off = static_cast<int>(wb.size());
    S.w_lo = rows * S.wrow;
    wb.resize(wb.size() + size_t(2) * rows * S.wrow, static_cast<_Float16>(0.f));
    for (int n = 0; n < op.cout; ++n)
      for (int k = 0; k < S.ksteps * 16; ++k) {
        const int g = k / 8, j = k - g * 8;
        int src = -1;  // index into HWIO weights (k' = tap * cin + ci)
        if (i2c) {
          if (k < K0) src = k;
        } else if (g < groups) {
          const int tap = g / (cin8 / 8), ci = (g - tap * (cin8 / 8)) * 8 + j;
          if (ci < op.cin) src = tap * op.cin + ci;
        }
        if (src >= 0) put_split(wb, S.w_off + size_t(n) * S.wrow + k, S.w_lo, op.w[size_t(src) * op.cout + n]);
      }
    S.b_off = static_cast<int>(bb.size());
    for (int n = 0; n < rows; ++n) bb.push_back(n < op.cout ? op.b[n] : 0.f);
    // group offsets (fp16 elements into the stage's input tensor); pad groups read offset 0
    S.kt_off = static_cast<int>(kt.size());
    for (int g = 0; g < 2 * S.ksteps; ++g) {
      int v = 0;
      if (g < groups) {
        if (i2c) {
          v = g * 8;
        } else {
          const int tap = g / (cin8 / 8), cg = g - tap * (cin8 / 8);
          const int dh = tap / op.kw, dw = tap - dh * op.kw;
          v = (dh * wo_in + dw) * S.cs_in + cg * 8;
        }
      }
      kt.push_back(v);
    }
    cin = op.cout;
  }
  x.cs0 = x.st[0].cs_in;
  std::vector<int> i2c;  // im2col tap offsets into the raw rows (stage-0 input width)
  if (x.im2col) {
    const XStage& S = x.st[0];
    for (int dh = 0; dh < S.kh; ++dh)
      for (int dw = 0; dw < S.kw; ++dw)
        for (int ci = 0; ci < S.cin; ++ci) i2c.push_back((dh * d.w + dw) * S.cin + ci);
  }
  i2c.push_back(0);
  const Dims od{h / x.out_ph, w / x.out_pw, cin};
  if (od.h <= 0 || od.w <= 0) {
    err = "hbk: pooling collapses the image";
    return kPlanErrArg;
  }
  x.H_out = od.h;
  x.W_out = od.w;
  x.C_out = od.c;
  x.out_img_stride = int64_t(od.h) * od.w * od.c;
  x.kt_n = static_cast<int>(kt.size());
  while (wb.size() % 8) wb.push_back(static_cast<_Float16>(0.f));

  // LDS: tensor t (stage t input; t = n_stages: last output) alternates X / Y
  auto region_bytes = [&](int G, int band, int64_t& xb, int64_t& yb) {
    const int n = x.n_stages;
    std::vector<int> rows(n + 1), wid(n + 1);
    rows[n] = band * x.out_ph;
    wid[0] = d.w;
    for (int s = 0; s < n; ++s) wid[s + 1] = wid[s] - (x.st[s].kw - 1);
    for (int s = n - 1; s >= 0; --s) rows[s] = rows[s + 1] + x.st[s].kh - 1;
    xb = yb = 0;
    for (int t = 0; t <= n; ++t) {
      int64_t bytes;
      if (t == 0 && x.im2col)  // stage 0 input = im2col tensor at its output geometry
        bytes = int64_t(G) * rows[1] * wid[1] * x.st[0].cs_in * 4;
      else
        bytes = int64_t(G) * rows[t] * wid[t] * (t == 0 ? x.st[0].cs_in : x.st[t - 1].cs_out) * 4;
      int64_t& r = (t % 2 == 0) ? xb : yb;
      r = std::max(r, bytes);
    }
    if (x.im2col) yb = std::max(yb, int64_t(G) * rows[0] * wid[0] * d.c * 4);  // raw f32 rows
    xb = (xb + 15) & ~int64_t(15);
    yb = (yb + 15) & ~int64_t(15);
  };
  const int64_t w_bytes = int64_t(wb.size()) * 2, k_bytes = (int64_t(kt.size()) * 4 + 15) & ~int64_t(15);
  const int64_t b_bytes = int64_t(bb.size()) * 4;  // multiple of 128
  auto lds_total = [&](int G, int band, bool resident) {
    int64_t xb, yb;
    region_bytes(G, band, xb, yb);
    return xb + yb + (resident ? w_bytes : 0) + b_bytes + k_bytes;
  };
  // MACs computed per output row of the whole image for a band of b rows
  // (halo rows recomputed by every band): useful / computed = efficiency.
  auto efficiency = [&](int b) {
    const int n = x.n_stages, nb = (od.h + b - 1) / b;
    double useful = 0, done = 0;
    int rows_b = b * x.out_ph, rows_full = od.h * x.out_ph;
    for (int s = n - 1; s >= 0; --s) {
      const XStage& S = x.st[s];
      int wo = d.w;
      for (int q = 0; q <= s; ++q) wo -= x.st[q].kw - 1;
      const double per_row = double(wo) * S.cout * S.kh * S.kw * S.cin;
      useful += per_row * rows_full;
      done += per_row * rows_b * nb;
      rows_b += S.kh - 1;
      rows_full += S.kh - 1;
    }
    return useful / done;
  };
  auto best_band = [&](bool res) {
    for (int b = od.h; b >= 1; --b)
      if (lds_total(1, b, res) <= lds_budget) return b;
    return 0;
  };
  bool resident = false;
  int band = 0, G = 1;
  for (int attempt = 0; attempt < 2; ++attempt) {
    // resident weights unless they cost more than 5 % of the work in halo rows
    // (HBK_EMBED_WEIGHTS=lds|global overrides, for tuning)
    const int band_r = lds_total(1, 1, true) <= lds_budget ? best_band(true) : 0;
    const int band_g = best_band(false);
    resident = band_r > 0 && (band_g == 0 || efficiency(band_r) >= 0.95 * efficiency(band_g));
    if (knobs.weights == 2 && band_g > 0) resident = false;
    if (knobs.weights == 1 && band_r > 0) resident = true;
    band = resident ? band_r : band_g;
    G = 1;
    if (band == 0) {
      err = "hbk: one output row of a chain does not fit in LDS";
      return kPlanErrUnsupported;
    }
    if (band == od.h)
      while (G < 64 && lds_total(G + 1, band, resident) <= lds_budget) ++G;  // any G: fill the LDS budget
    if (attempt == 0 && !knobs.lds_kb_set && band == od.h && G < kMinG) {
      lds_budget = kLdsBudgetCU;
      continue;
    }
    break;
  }
  x.G = G;
  x.band = band;
  x.n_bands = (od.h + band - 1) / band;
  int64_t xb, yb;
  region_bytes(G, band, xb, yb);
  x.lds_x = 0;
  x.lds_y = static_cast<int>(xb);
  x.lds_w = static_cast<int>(xb + yb);
  x.lds_b = x.lds_w + static_cast<int>(resident ? w_bytes : 0);
  x.lds_k = x.lds_b + static_cast<int>(b_bytes);
  x.w_halfs = resident ? static_cast<int>(wb.size()) : 0;
  x.b_floats = static_cast<int>(bb.size());
  x.vec_out = od.c % 4 == 0;  // cleared at launch for an unaligned output
  x.raw_vec = x.im2col && x.in_pw == 1 && (x.W_in * x.C_src) % 4 == 0;  // and at launch: alignment
  x.i2c_n = static_cast<int>(i2c.size());
  x.dbg_skip = knobs.debug_skip;
  L.kernel = {Kern::x3, nbmax, !resident};
  L.name = "conv_chain_x3_kernel";
  L.threads = kXThreads;
  L.lds_bytes = size_t(x.lds_k + k_bytes);
  L.imgs_per_task = G;
  L.n_bands = x.n_bands;
  // device blob: weights (fp16), biases (f32), group offsets (int), im2col taps (int)
  L.ptr_off[1] = size_t(w_bytes);
  L.ptr_off[2] = L.ptr_off[1] + pad16(size_t(b_bytes));
  L.ptr_off[3] = L.ptr_off[2] + size_t(k_bytes);
  L.blob.assign(L.ptr_off[3] + i2c.size() * 4, 0);
  memcpy(L.blob.data(), wb.data(), size_t(w_bytes));
  memcpy(L.blob.data() + L.ptr_off[1], bb.data(), size_t(b_bytes));
  memcpy(L.blob.data() + L.ptr_off[2], kt.data(), kt.size() * 4);
  memcpy(L.blob.data() + L.ptr_off[3], i2c.data(), i2c.size() * 4);
  L.debug = strf("hbk split chain: %d stages, in %dx%dx%d (pool %dx%d, im2col %d) -> %dx%dx%d (pool %dx%d); "
                 "G %d band %d/%d (eff %.3f), weights %s %lld B, LDS %zu B, nb %d\n",
                 x.n_stages, d.h, d.w, d.c, x.in_ph, x.in_pw, x.im2col, od.h, od.w, od.c, x.out_ph, x.out_pw, G,
                 band, od.h, efficiency(band), resident ? "LDS" : "global", (long long)w_bytes, L.lds_bytes, nbmax);
  L.args = x;
  od_out = od;
  macs_out = macs;
  return kPlanOk;
}

// ---- pattern kernels: a chain of one exact shape gets a kernel written for it ----

struct ConvShape {
  int kh, kw, cin, cout;
};

inline bool convs_are(const std::vector<OpInfo>& ops, const std::vector<int>& st,
                      std::initializer_list<ConvShape> want) {
  if (st.size() != want.size()) return false;
  size_t i = 0;
  for (const ConvShape& s : want) {
    const OpInfo& o = ops[st[i++]];
    if (o.kh != s.kh || o.kw != s.kw || o.cin != s.cin || o.cout != s.cout) return false;
  }
  return true;
}

// All of the chain's convs (but the last, if last_linear) LeakyReLU with one
// slope in [0, 1], or all linear.
inline bool uniform_act(const std::vector<OpInfo>& ops, const std::vector<int>& st, bool last_linear, bool& leaky) {
  const OpInfo& o0 = ops[st[0]];
  leaky = o0.act != 0;
  for (size_t i = 0; i < st.size(); ++i) {
    const OpInfo& o = ops[st[i]];
    const bool act = leaky && !(last_linear && i + 1 == st.size());
    if ((o.act != 0) != act) return false;
    if (act && (o.alpha != o0.alpha || !(o.alpha >= 0.f && o.alpha <= 1.f))) return false;
  }
  return true;
}

// The chain reads ipc images per clip through an in_ph x 1 input pool from rows
// of `row` floats of c channels, and pools its output out_p x out_p.
inline bool reads(const ChainIo& a, int ipc, int in_ph, int out_p, int c, int row) {
  return a.ipc == ipc && a.in_ph == in_ph && a.in_pw == 1 && a.out_ph == out_p && a.out_pw == out_p &&
         a.C_src == c && a.src_row_stride == row;
}

inline bool is(Dims d, int h, int w, int c) { return d.h == h && d.w == w && d.c == c; }

// The blob of a pattern kernel: the f16 weight planes, then the f32 biases at the next 16 B.
template <class Args>
Launch pattern_launch(KernelChoice kernel, const char* name, const Args& args, int threads, size_t lds,
                      int imgs_per_task, int n_bands, const std::vector<_Float16>& w, const float* bias,
                      size_t n_bias, std::string debug) {
  Launch L;
  L.kernel = kernel;
  L.name = name;
  L.args = args;
  L.threads = threads;
  L.lds_bytes = lds;
  L.imgs_per_task = imgs_per_task;
  L.n_bands = n_bands;
  L.ptr_off[1] = pad16(w.size() * 2);
  L.blob.assign(n_bias ? L.ptr_off[1] + n_bias * 4 : w.size() * 2, 0);
  memcpy(L.blob.data(), w.data(), w.size() * 2);
  if (n_bias) memcpy(L.blob.data() + L.ptr_off[1], bias, n_bias * 4);
  L.debug = std::move(debug);
  return L;
}

// The p0 pattern: [3x3 (1 -> C), 1x3 (C -> C), 3x1 (C -> C)] + output pool 2x2
// on input width 32, C = 24, one image per source clip.
constexpr int kP0W = 32, kP0C = 24;

inline bool is_p0(const std::vector<OpInfo>& ops, const std::vector<int>& st, const ChainIo& a, Dims d,
                  bool& leaky) {
  const int C = kP0C;
  return reads(a, 1, 1, 2, 1, kP0W) && d.w == kP0W && convs_are(ops, st, {{3, 3, 1, C}, {1, 3, C, C}, {3, 1, C, C}}) &&
         uniform_act(ops, st, false, leaky);
}

// The streaming p0 form (p0s_chain_kernel): the chain on a 136-row input, one
// wave per clip. Weights hi / lo of 16 W rounded toward zero, with each
// stage's bias in K slot 6 (stage 0) or 72 (stages 1, 2).
inline std::optional<Launch> plan_p0s(const std::vector<OpInfo>& ops, const std::vector<int>& st, const ChainIo& a,
                                      Dims d, Dims od) {
  bool leaky;
  if (!is_p0(ops, st, a, d, leaky) || d.h != kP0sRows || !is(od, kP0sHout, kP0sWout, kP0C)) return std::nullopt;
  const OpInfo &o0 = ops[st[0]], &o1 = ops[st[1]], &o2 = ops[st[2]];
  const int C = kP0C;
  const int woff1 = 2 * 32 * 16, woff2 = woff1 + 2 * 32 * 16 * kP0sKS, total = woff2 + 2 * 32 * 16 * kP0sKS;
  std::vector<_Float16> w(total, static_cast<_Float16>(0.f));
  auto put = [&](int off, int ks, int n, int k, float v) { put_split(w, off + n * 16 * ks + k, 32 * 16 * ks, v); };
  for (int n = 0; n < C; ++n) {
    // K slots (p0s_iter): lower half 0-5 = window (y, y + 1) x (dx 0-2), upper half 8-13 = window
    // (y + 1, y + 2); taps 0-4 in the lower half, 5-8 in the upper, the bias in slot 6 (B = 1)
    for (int k = 0; k < 16; ++k) {
      const int tap = k < 5 ? k : (k >= 10 && k < 14 ? k - 5 : -1);
      if (tap >= 0) put(0, 1, n, k, o0.w[size_t(tap) * C + n]);
    }
    put(0, 1, n, 6, o0.b[n]);
    for (int k = 0; k < 3 * C; ++k) put(woff1, kP0sKS, n, k, o1.w[size_t(k) * C + n]);  // HWIO: (tap C + ci) C + n
    put(woff1, kP0sKS, n, 3 * C, o1.b[n]);
    // stage 2: K step ks, lane half h holds group (dy, c) = G2[ks][h] (p0s_iter), channels 8 c .. 8 c + 7
    static const int G2[5][2][2] = {{{0, 0}, {0, 1}}, {{1, 0}, {1, 1}}, {{2, 0}, {2, 1}}, {{0, 2}, {1, 2}},
                                    {{2, 2}, {-1, -1}}};
    for (int ks = 0; ks < kP0sKS; ++ks)
      for (int h = 0; h < 2; ++h)
        for (int i = 0; i < 8; ++i) {
          const int k = 16 * ks + 8 * h + i, dy = G2[ks][h][0], cg = G2[ks][h][1];
          put(woff2, kP0sKS, n, k, dy < 0 ? (i == 0 ? o2.b[n] : 0.f) : o2.w[size_t(dy * C + 8 * cg + i) * C + n]);
        }
  }
  P0Args p{};
  p.H_in = d.h;
  p.H_out = od.h;
  p.n_bands = 1;
  p.alpha = leaky ? o0.alpha : 0.f;
  Launch L = pattern_launch({Kern::p0s, 0, leaky}, "p0_chain_kernel", p, kP0sThreads, kP0sLds, kP0sWaves, 1, w, nullptr,
                            0, strf("hbk p0s chain: %dx%dx1 -> %dx%dx%d, one wave per clip, LDS %zu B", d.h, d.w,
                                    od.h, od.w, od.c, size_t(kP0sLds)));
  L.tasks_below_2_31 = true;
  return L;
}

// The banded p0 form (p0_chain_kernel): weights of stage s = hi [32][16 ks_s]
// then lo; K of stage 0 = taps 0-4 | pad | taps 5-8 | pad. Pooled rows per
// task: 6 (78 KB of LDS, two blocks per CU); HBK_P0_BAND=5|7 for tuning.
inline std::optional<Launch> plan_p0_band(const std::vector<OpInfo>& ops, const std::vector<int>& st,
                                          const ChainIo& a, Dims d, Dims od, int band_knob) {
  const int band = band_knob == 5 || band_knob == 7 ? band_knob : 6;
  using P0G = P0Geo<kP0W, kP0C, 6>;  // (the weight layout does not depend on the band)
  const size_t lds = band == 5 ? P0Geo<kP0W, kP0C, 5>::LDS : band == 7 ? P0Geo<kP0W, kP0C, 7>::LDS : P0G::LDS;
  bool leaky;
  if (!is_p0(ops, st, a, d, leaky) || !is(od, (d.h - 4) / 2, (d.w - 4) / 2, kP0C)) return std::nullopt;
  const OpInfo &o0 = ops[st[0]], &o1 = ops[st[1]], &o2 = ops[st[2]];
  const int C = kP0C;
  std::vector<_Float16> w(P0G::WHALFS, static_cast<_Float16>(0.f));
  auto put = [&](int off, int ks, int n, int k, float v) { put_split(w, off + n * 16 * ks + k, 32 * 16 * ks, v); };
  for (int n = 0; n < C; ++n) {
    for (int k = 0; k < 16; ++k) {
      const int tap = k < 5 ? k : (k >= 8 && k < 12 ? k - 3 : -1);
      if (tap >= 0) put(0, 1, n, k, o0.w[size_t(tap) * C + n]);
    }
    for (int k = 0; k < 3 * C; ++k) {
      put(P0G::WOFF1, P0G::KS, n, k, o1.w[size_t(k) * C + n]);  // HWIO: (tap * C + ci) * C + n
      put(P0G::WOFF2, P0G::KS, n, k, o2.w[size_t(k) * C + n]);
    }
  }
  std::vector<float> b(96, 0.f);
  for (int n = 0; n < C; ++n) {
    b[n] = o0.b[n];
    b[32 + n] = o1.b[n];
    b[64 + n] = o2.b[n];
  }
  P0Args p{};
  p.H_in = d.h;
  p.H_out = od.h;
  p.n_bands = (od.h + band - 1) / band;
  p.alpha = leaky ? o0.alpha : 0.f;
  Launch L = pattern_launch({Kern::p0_band, band, leaky}, "p0_chain_kernel", p, kP0Threads, lds, 1, p.n_bands, w,
                            b.data(), b.size(),
                            strf("hbk p0 chain: %dx%dx1 -> %dx%dx%d, band %d (%d bands), LDS %zu B", d.h, d.w, od.h,
                                 od.w, od.c, band, p.n_bands, lds));
  L.tasks_below_2_31 = true;
  return L;
}

// The p1 pattern: [1x3 (CI -> 32), 3x1, 1x3, 3x1 (32 -> 32)] + output pool 2x2,
// NHWC input of width 14 with CI = 24, one image per source image.
constexpr int kP1W = 14, kP1CI = 24, kP1Band = 8;
using P1G = P1Geo<kP1W, kP1CI, kP1Band>;

// [1x3 (ci -> c), 3x1, 1x3, 3x1 (c -> c)] with one activation: the p1 and p2s chains
inline bool is_1313(const std::vector<OpInfo>& ops, const std::vector<int>& st, int ci, int c, bool& leaky) {
  return convs_are(ops, st, {{1, 3, ci, c}, {3, 1, c, c}, {1, 3, c, c}, {3, 1, c, c}}) &&
         uniform_act(ops, st, false, leaky);
}

// The streaming p1 form (p1s_chain_kernel) for a 66-row input: weights per
// stage s as hi / lo [32][96] (K = tap * cin + ci; stage a's bias at K 72),
// biases of stages b, c, d as [3][32] f32.
inline std::optional<Launch> plan_p1s(const std::vector<OpInfo>& ops, const std::vector<int>& st, const ChainIo& a,
                                      Dims d, Dims od) {
  bool leaky;
  if (!reads(a, 1, 1, 2, kP1sCSI, kP1sWi * kP1sCSI) || !is(d, kP1sHin, kP1sWi, kP1sCSI) ||
      !is_1313(ops, st, kP1sCSI, kP1sCo, leaky) || !is(od, kP1sHout, kP1sWo, kP1sCo))
    return std::nullopt;
  std::vector<_Float16> w(4 * kP1sStageHalfs, static_cast<_Float16>(0.f));
  auto put = [&](int s, int n, int k, float v) { put_split(w, s * kP1sStageHalfs + n * 96 + k, 32 * 96, v); };
  for (int s = 0; s < 4; ++s) {
    const OpInfo& o = ops[st[s]];
    const int K = 3 * o.cin;
    for (int n = 0; n < kP1sCo; ++n) {
      for (int k = 0; k < K; ++k) put(s, n, k, o.w[size_t(k) * kP1sCo + n]);  // HWIO: (tap cin + ci) cout + n
      if (s == 0) put(0, n, K, o.b[n]);
    }
  }
  std::vector<float> b(3 * 32, 0.f);
  for (int s = 1; s < 4; ++s)
    for (int n = 0; n < kP1sCo; ++n) b[32 * (s - 1) + n] = ops[st[s]].b[n];
  P1Args p{};
  p.H_in = d.h;
  p.H_out = od.h;
  p.n_bands = 1;
  p.alpha = leaky ? ops[st[0]].alpha : 0.f;
  Launch L = pattern_launch({Kern::p1s, 0, leaky}, "p1_chain_kernel", p, kP1sThreads, kP1sLds, 1, 1, w, b.data(),
                            b.size(),
                            strf("hbk p1s chain: %dx%dx%d -> %dx%dx%d, two-wave stage pipeline per clip, LDS %zu B",
                                 d.h, d.w, d.c, od.h, od.w, od.c, size_t(kP1sLds)));
  L.tasks_below_2_31 = true;
  return L;
}

// The banded p1 form (p1_chain_kernel, on kP0Threads): weights of stage s at
// woff[s] as hi [32][16 ks_s] then lo, biases [4][32].
inline std::optional<Launch> plan_p1(const std::vector<OpInfo>& ops, const std::vector<int>& st, const ChainIo& a,
                                     Dims d, Dims od) {
  const int C = kP1C;
  bool leaky;
  if (!reads(a, 1, 1, 2, kP1CI, kP1W * kP1CI) || d.w != kP1W || d.c != kP1CI || !is_1313(ops, st, kP1CI, C, leaky) ||
      !is(od, (d.h - 4) / 2, (d.w - 4) / 2, C))
    return std::nullopt;
  std::vector<_Float16> w(P1G::WHALFS, static_cast<_Float16>(0.f));
  const int woff[4] = {P1G::WOFF1, P1G::WOFF2, P1G::WOFF3, P1G::WOFF4};
  for (int i = 0; i < 4; ++i) {
    const OpInfo& o = ops[st[i]];
    const int ks = i ? P1G::KS : P1G::KS1, K = 3 * o.cin;
    for (int n = 0; n < C; ++n)
      for (int k = 0; k < K; ++k)  // HWIO: (tap * cin + ci) * cout + n
        put_split(w, woff[i] + n * 16 * ks + k, 32 * 16 * ks, o.w[size_t(k) * C + n]);
  }
  std::vector<float> b(128, 0.f);
  for (int i = 0; i < 4; ++i)
    for (int n = 0; n < C; ++n) b[32 * i + n] = ops[st[i]].b[n];
  P1Args p{};
  p.H_in = d.h;
  p.H_out = od.h;
  p.n_bands = (od.h + kP1Band - 1) / kP1Band;
  p.alpha = leaky ? ops[st[0]].alpha : 0.f;
  Launch L = pattern_launch({Kern::p1, 0, leaky}, "p1_chain_kernel", p, kP0Threads, P1G::LDS, 1, p.n_bands, w, b.data(),
                            b.size(),
                            strf("hbk p1 chain: %dx%dx%d -> %dx%dx%d, band %d (%d bands), LDS %zu B", d.h, d.w, d.c,
                                 od.h, od.w, od.c, kP1Band, p.n_bands, size_t(P1G::LDS)));
  L.tasks_below_2_31 = true;
  return L;
}

// The p2s pattern (SE20 chain 2): [1x3 (32 -> 48), 3x1, 1x3, 3x1 (48 -> 48)] on a
// 31 x 5 x 32 input, no output pool, one image per source image. Weights hi /
// lo [48][96] (stage a) and [48][160] (b, c, d: K = tap * 48 + ci, the bias at
// K 144); stage a's bias as f32.
inline std::optional<Launch> plan_p2s(const std::vector<OpInfo>& ops, const std::vector<int>& st, const ChainIo& a,
                                      Dims d, Dims od) {
  bool leaky;
  if (!reads(a, 1, 1, 1, kP2sCi, kP2sWi * kP2sCi) || !is(d, kP2sHin, kP2sWi, kP2sCi) ||
      !is_1313(ops, st, kP2sCi, kP2sCo, leaky) || !is(od, kP2sHout, 1, kP2sCo))
    return std::nullopt;
  const size_t wa = size_t(2) * kP2sCo * kP2sKa, wsz = size_t(2) * kP2sCo * kP2sK;
  std::vector<_Float16> w(wa + 3 * wsz, static_cast<_Float16>(0.f));
  for (int s = 0; s < 4; ++s) {
    const OpInfo& o = ops[st[s]];
    const size_t off = s == 0 ? 0 : wa + (s - 1) * wsz;
    const int Kp = s == 0 ? kP2sKa : kP2sK, K = 3 * o.cin;
    auto put = [&](int n, int k, float v) { put_split(w, off + size_t(n) * Kp + k, size_t(kP2sCo) * Kp, v); };
    for (int n = 0; n < kP2sCo; ++n) {
      for (int k = 0; k < K; ++k) put(n, k, o.w[size_t(k) * kP2sCo + n]);  // HWIO: (tap cin + ci) cout + n
      if (s > 0) put(n, K, o.b[n]);
    }
  }
  P2sArgs p{};
  p.alpha = leaky ? ops[st[0]].alpha : 0.f;
  return pattern_launch({Kern::p2s, 0, leaky}, "p2s_chain_kernel", p, kP2sThreads, kP2sLds, kP2sClips, 1, w,
                        ops[st[0]].b.data(), kP2sCo,
                        strf("hbk p2s chain: %dx%dx%d -> %dx%dx%d, %d clips per workgroup, LDS %zu B", d.h, d.w, d.c,
                             od.h, od.w, od.c, kP2sClips, size_t(kP2sLds)));
}

// The t3s pattern (SE20's tail over its two phase images per clip): an input
// pool 2x1 of the 27 x 1 x 48 chain-2 rows, 3x1 (48 -> 64), 1x1, 3x1, 1x1 (64),
// 2x1 (64 -> 96), four 1x1 (96), the last without activation. Weights hi / lo
// [cout][K] per stage (K = tap * cin + ci; stage 1 zero-padded to 160), biases f32.
inline std::optional<Launch> plan_t3s(const std::vector<OpInfo>& ops, const std::vector<int>& st, const ChainIo& a,
                                      Dims d, Dims od, int64_t out_img_stride) {
  const int c0 = kT3C0, c1 = kT3C1, c2 = kT3C2;
  bool leaky;
  if (!reads(a, 2, 2, 1, c0, c0) || a.row_off[0] != 0 || a.row_off[1] != 1 ||
      a.src_clip_stride != int64_t(kT3Hin) * c0 || !is(d, kT3Hp, 1, c0) || !is(od, kT3Hout, 1, c2) ||
      out_img_stride != int64_t(kT3Hout) * c2)
    return std::nullopt;
  if (!convs_are(ops, st, {{3, 1, c0, c1}, {1, 1, c1, c1}, {3, 1, c1, c1}, {1, 1, c1, c1}, {2, 1, c1, c2},
                           {1, 1, c2, c2}, {1, 1, c2, c2}, {1, 1, c2, c2}, {1, 1, c2, c2}}) ||
      !uniform_act(ops, st, true, leaky))
    return std::nullopt;
  std::vector<_Float16> w(kT3WHalfs, static_cast<_Float16>(0.f));
  std::vector<float> b(4 * c1 + 5 * c2, 0.f);
  int boff = 0;
  for (int i = 0; i < 9; ++i) {
    const OpInfo& o = ops[st[i]];
    const int K = o.kh * o.cin, Kp = kT3K[i];
    for (int n = 0; n < o.cout; ++n) {
      for (int k = 0; k < K; ++k)  // HWIO: (tap cin + ci) cout + n
        put_split(w, kT3W[i] + size_t(n) * Kp + k, size_t(o.cout) * Kp, o.w[size_t(k) * o.cout + n]);
      b[boff + n] = o.b[n];
    }
    boff += o.cout;
  }
  T3sArgs p{};
  p.out_img_stride = out_img_stride;
  p.alpha = leaky ? ops[st[0]].alpha : 0.f;
  Launch L = pattern_launch({Kern::t3s, 0, leaky}, "t3s_chain_kernel", p, kT3Threads, kT3Lds, kT3Pos, 1, w, b.data(),
                            b.size(),
                            strf("hbk t3s chain: %dx%dx%d (pool 2x1) -> %dx%dx%d, %d images per workgroup, LDS %zu B",
                                 d.h, d.w, d.c, od.h, od.w, od.c, kT3Pos, size_t(kT3Lds)));
  L.min_src_stride = int64_t(kT3Hin) * c0;
  L.out_stride_4 = out_img_stride;
  return L;
}

// The first pattern the chain matches, in the order p0s, p0 band, p1s, p1, p2s, t3s.
inline std::optional<Launch> plan_pattern(const std::vector<OpInfo>& ops, const std::vector<int>& st,
                                          const ChainIo& a, Dims d, Dims od, int64_t out_img_stride,
                                          const EmbedKnobs& kn) {
  std::optional<Launch> L;
  if (!kn.no_p0) {
    if (!kn.no_p0s) L = plan_p0s(ops, st, a, d, od);
    if (!L) L = plan_p0_band(ops, st, a, d, od, kn.p0_band);
  }
  if (!L && !kn.no_p1) {
    if (!kn.no_p1s) L = plan_p1s(ops, st, a, d, od);
    if (!L) L = plan_p1(ops, st, a, d, od);
  }
  if (!L && !kn.no_p2s) L = plan_p2s(ops, st, a, d, od);
  if (!L && !kn.no_t3s) L = plan_t3s(ops, st, a, d, od, out_img_stride);
  return L;
}

// Appends the chains for ops [o0, o1) applied to images of dims `in`, reading
// image i from row_off[i % ipc] of source clip i / ipc.
inline int plan_segment(const std::vector<OpInfo>& ops, int o0, int o1, Dims in, int ipc,
                        const std::vector<int>& row_off, int64_t src_clip_floats, int src_row_floats, bool split,
                        const EmbedKnobs& knobs, ProgramPlan& prog, std::vector<Dims>* out_dims_per_chain,
                        std::string& err) {
  int i = o0;
  Dims cur = in;
  bool first = true;
  while (i < o1) {
    ChainIo a{};
    a.ipc = first ? ipc : 1;
    if (first)
      for (size_t k = 0; k < row_off.size(); ++k) a.row_off[k] = row_off[k];
    a.src_clip_stride = first ? src_clip_floats : int64_t(cur.h) * cur.w * cur.c;
    a.src_row_stride = first ? src_row_floats : cur.w * cur.c;
    a.C_src = cur.c;
    a.in_ph = a.in_pw = 1;
    if (ops[i].kind == kOpMaxPool) {
      a.in_ph = ops[i].kh;
      a.in_pw = ops[i].kw;
      ++i;
    }
    const Dims d{cur.h / a.in_ph, cur.w / a.in_pw, cur.c};
    a.W_in = d.w;
    std::vector<int> stage_ops;
    while (i < o1 && ops[i].kind == kOpConv && int(stage_ops.size()) < kMaxStages) {
      stage_ops.push_back(i);
      ++i;
    }
    if (stage_ops.empty()) {
      err = "hbk: unsupported graph: a max-pool must be followed by a conv";
      return kPlanErrUnsupported;
    }
    a.out_ph = a.out_pw = 1;
    if (i < o1 && ops[i].kind == kOpMaxPool && (i + 1 >= o1 || ops[i + 1].kind == kOpConv)) {
      // keep the pool as this chain's output pool unless the next chain needs it as input pool
      a.out_ph = ops[i].kh;
      a.out_pw = ops[i].kw;
      ++i;
    }
    ChainHost ch;
    Dims od;
    const int rc = split ? layout_split(ops, stage_ops, d, a, knobs, ch.base, od, ch.macs_per_img, err)
                         : layout_exact(ops, stage_ops, d, a, ch.base, od, ch.macs_per_img, err);
    if (rc) return rc;
    ch.ipc = a.ipc;
    ch.src_clip_stride = a.src_clip_stride;
    ch.out_img_stride = int64_t(od.h) * od.w * od.c;
    ch.out_floats = ch.out_img_stride * (first ? ipc : 1);
    if (split) {
      ch.pattern = plan_pattern(ops, stage_ops, a, d, od, ch.out_img_stride, knobs);
      std::get<XArgs>(ch.base.args).dbg_slot = static_cast<int>(prog.chains.size() % 4);
    }
    prog.chains.push_back(std::move(ch));
    if (out_dims_per_chain) out_dims_per_chain->push_back(od);
    cur = od;
    first = false;
  }
  return kPlanOk;
}

// Ping-pong workspace buffers (chain k writes buffer k % 2, the last writes
// the call's output, or the gather's source), the images per unit of each
// chain and the per-unit buffer sizes.
inline void assign_buffers(ProgramPlan& prog, bool clip_path, int n_win) {
  const size_t n = prog.chains.size();
  bool tail = false;
  int tail_imgs = n_win;
  for (size_t k = 0; k < n; ++k) {
    ChainHost& c = prog.chains[k];
    c.src_buf = (k == 0) ? -1 : int((k - 1) % 2);
    c.dst_buf = (k + 1 == n && prog.gather_src.empty()) ? -1 : int(k % 2);
    if (clip_path && c.ipc > 1 && !tail) {
      tail = true;
      tail_imgs = c.ipc;  // n_win, or the phase images of a deduplicated tail
    }
    c.imgs_per_unit = tail ? tail_imgs : 1;
    if (c.dst_buf >= 0)
      prog.buf_floats[c.dst_buf] = std::max(prog.buf_floats[c.dst_buf], c.out_img_stride * c.imgs_per_unit);
  }
  if (!prog.gather_src.empty()) prog.gather_buf = int((n - 1) % 2);
}

// The whole plan. Returns kPlanOk, or the status with the text in plan.error.
inline int plan_embed(const std::vector<OpIn>& graph, int in_h, int in_w, const std::vector<int>& starts,
                      bool split_f16, const EmbedKnobs& knobs, EmbedHostPlan& p) {
  std::string& err = p.error;
  const int n_ops = static_cast<int>(graph.size()), n_win = static_cast<int>(starts.size());
  p.in_h = in_h;
  p.in_w = in_w;
  p.n_win = n_win;
  p.split_f16 = split_f16;
  for (int s : starts)
    if (s < 0) return arg_fail(err, "negative window start");
  std::vector<OpInfo> ops;
  Dims d{in_h, in_w, 1};
  std::vector<Dims> dims;  // per op, for one window
  for (int i = 0; i < n_ops; ++i) {
    const OpIn& o = graph[i];
    OpInfo op{o.kind, o.kh, o.kw, o.cin, o.cout, o.act, o.alpha, {}, {}};
    if (o.kh <= 0 || o.kw <= 0) return arg_fail(err, "kernel / pool size must be positive");
    if (o.kind == kOpConv) {
      if (o.cin != d.c || o.cout <= 0 || !o.weight || !o.bias) return arg_fail(err, "bad conv op");
      op.w.assign(o.weight, o.weight + size_t(o.kh) * o.kw * o.cin * o.cout);
      op.b.assign(o.bias, o.bias + o.cout);
      if (split_f16)
        for (float w : op.w)
          if (!(std::fabs(w) < kF16Max)) {
            err = strf("hbk: op %d has a weight |w| >= 65504 (or NaN), outside the split-f16 range; "
                       "use HBK_PREC_EXACT_F32", i);
            return kPlanErrUnsupported;
          }
      d = Dims{d.h - o.kh + 1, d.w - o.kw + 1, o.cout};
    } else if (o.kind == kOpMaxPool) {
      d = Dims{d.h / o.kh, d.w / o.kw, d.c};
    } else {
      return arg_fail(err, "unknown op kind");
    }
    if (d.h <= 0 || d.w <= 0) return arg_fail(err, "graph collapses the window");
    ops.push_back(std::move(op));
    dims.push_back(d);
  }
  if (d.h != 1 || d.w != 1) return arg_fail(err, "graph output must be 1 x 1 x C");
  p.out_dim = d.c;

  // prefix: ops shared across the windows of a clip. A pool of height ph keeps
  // the windows aligned iff the cumulative time stride divides every start.
  int g = 0;
  for (int s : starts) g = std::gcd(g, s);
  // If every pool keeps the alignment, split at the last pool (any earlier
  // split is equally valid; the tail must start with a pool).
  int stride = 1, split = n_ops, last_pool = -1, stride_before_last = 1;
  for (int i = 0; i < n_ops; ++i) {
    if (ops[i].kind == kOpMaxPool) {
      const int ns = stride * ops[i].kh;
      if (g % ns != 0) {
        split = i;
        break;
      }
      last_pool = i;
      stride_before_last = stride;
      stride = ns;
    }
  }
  if (split == n_ops && last_pool > 0) {
    split = last_pool;
    stride = stride_before_last;
  }
  // the tail must start with a pool (its input pool) and contain a conv
  if (split == n_ops || split == 0) {
    err = "hbk: graph has no window-splitting pool; use hbk_embed_windows";
    return kPlanErrUnsupported;
  }
  p.n_prefix = split;
  p.split_stride = stride;
  p.seq_frames = *std::max_element(starts.begin(), starts.end()) + in_h;

  int rc;
  // ---- clip program: prefix over [seq_frames, in_w, 1] per clip ----
  {
    std::vector<Dims> od;
    rc = plan_segment(ops, 0, split, Dims{p.seq_frames, in_w, 1}, 1, {0}, 0, in_w, split_f16, knobs, p.clip, &od, err);
    if (rc) return rc;
    const Dims pre = od.back();
    // window rows at the split, for one window
    const Dims wd = dims[split - 1];
    std::vector<int> roff;
    for (int s : starts) roff.push_back(s / stride);
    for (int r : roff)
      if (r + wd.h > pre.h) return arg_fail(err, "window start beyond the frame sequence");
    const size_t n_pre = p.clip.chains.size();
    // Phase deduplication of the tail: with S = the tail's cumulative pool
    // stride, windows whose prefix-row offsets are congruent mod S see the same
    // pool grid, and the tail's valid convs are translation-equivariant, so
    // ONE "phase image" per residue (rows [phi, phi + H)) yields every such
    // window as output row (r - phi) / S. Used when the phase images' output
    // fits the per-clip output (n_phase x rows <= n_win) and HBK_EMBED_NO_DEDUP
    // is unset; the output rows are gathered into window order afterwards.
    std::vector<int> phases, win_src;
    int H = 0;
    {
      int S = 1;
      for (int i = split; i < n_ops; ++i)
        if (ops[i].kind == kOpMaxPool) S *= ops[i].kh;
      for (int r : roff)
        if (std::find(phases.begin(), phases.end(), r % S) == phases.end()) phases.push_back(r % S);
      std::sort(phases.begin(), phases.end());
      for (int r : roff) H = std::max(H, r - r % S + wd.h);
      bool ok = S > 1 && !knobs.no_dedup && int(phases.size()) < n_win;
      for (int ph : phases) ok = ok && ph + H <= pre.h;
      // tail output rows for an H-row phase image
      Dims t{H, wd.w, wd.c};
      for (int i = split; i < n_ops && ok; ++i) {
        const OpInfo& o = ops[i];
        t = o.kind == kOpConv ? Dims{t.h - o.kh + 1, t.w - o.kw + 1, o.cout} : Dims{t.h / o.kh, t.w / o.kw, t.c};
        ok = t.h > 0 && t.w > 0;
      }
      ok = ok && t.w == 1 && int(phases.size()) * t.h <= n_win;
      if (ok) {
        for (int r : roff) {
          const int ph = int(std::find(phases.begin(), phases.end(), r % S) - phases.begin());
          const int row = (r - r % S) / S;
          ok = ok && row < t.h;
          win_src.push_back(ph * t.h + row);
        }
        p.clip.n_src = int(phases.size()) * t.h;
      }
      if (!ok) phases.clear();
    }
    const int64_t pre_floats = int64_t(pre.h) * pre.w * pre.c;
    if (!phases.empty()) {
      p.clip.gather_src = win_src;
      rc = plan_segment(ops, split, n_ops, Dims{H, wd.w, wd.c}, int(phases.size()), phases, pre_floats,
                        pre.w * pre.c, split_f16, knobs, p.clip, nullptr, err);
      p.dedup_debug = strf("hbk tail dedup: %zu phase images of %d rows per clip for %d windows\n", phases.size(), H,
                           n_win);
    } else {
      rc = plan_segment(ops, split, n_ops, Dims{wd.h, wd.w, wd.c}, n_win, roff, pre_floats, pre.w * pre.c, split_f16,
                        knobs, p.clip, nullptr, err);
    }
    if (rc) return rc;
    for (size_t k = 0; k < p.clip.chains.size(); ++k)
      (k < n_pre ? p.prefix_macs : p.tail_macs) += p.clip.chains[k].macs_per_img;
    // tail_macs is reported per window: with phase images, their MACs per clip / n_win
    if (!phases.empty()) p.tail_macs *= double(phases.size()) / double(n_win);
    assign_buffers(p.clip, true, n_win);
  }
  // ---- window program: every op per window ----
  rc = plan_segment(ops, 0, n_ops, Dims{in_h, in_w, 1}, 1, {0}, int64_t(in_h) * in_w, in_w, split_f16, knobs, p.win,
                    nullptr, err);
  if (rc) return rc;
  assign_buffers(p.win, false, 1);
  return kPlanOk;
}

}  // namespace
}  // namespace hbk
