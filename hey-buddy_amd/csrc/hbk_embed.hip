// Speech-embedding conv stack for gfx950: fused conv chains on MFMA (f32).
//
// Replaces the speech-embedding ONNX graph run by SpeechEmbeddingModel.__call__
// (embeddings.py:32-42) over the 76-frame windows that
// SpeechEmbeddings.spectrograms_to_embeddings cuts (embeddings.py:86-151).
//
// Execution model
//   * The graph (Keras Conv2D 'valid' stride 1 + LeakyReLU, MaxPool2D) is cut
//     into CHAINS: [optional input pool] conv ... conv [optional output pool].
//     One launch runs a whole chain; its activations live in LDS.
//   * A task = G images x one band of output rows. The band's input rows are
//     staged into LDS once (NHWC, channels padded to an odd count so that the
//     16 rows of an MFMA A-fragment hit 16 different banks), then every conv
//     runs as an implicit GEMM  out[m, n] = sum_k A[m, k] W[k, n]  with
//     m = (image, y, x), k = (dh, dw, ci) gathered from LDS through a per-stage
//     offset table, on v_mfma_f32_16x16x4f32 (exact f32, fmaf-chain numerics).
//   * Clip path: layers before the first pool that breaks the alignment of the
//     window starts run ONCE per clip over the whole 136-frame sequence
//     ("prefix"); windows are then cut from the prefix output (row offsets) for
//     the per-window "tail". The per-window API runs every layer per window.
//
// This unit is the host side: a host plan (hbk_embed_plan.h) realised on the
// device, the launcher, the gather kernel of the tail deduplication and the
// hbk_embed_* entry points. The chain kernels are reached through their
// addresses (hbk_embed_internal.h) and live by family: hbk_embed_exact.hip
// (exact f32, as described above), hbk_embed_x3.hip (generic split-f16, with
// the phase counters), hbk_embed_band.hip (banded patterns p0, p1) and
// hbk_embed_stream.hip (streaming patterns p0s, p1s, p2s, t3s); their shared
// device helpers are in hbk_embed_dev.h. The NaN-row repair is hbk_nan_rows.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "hbk_common.h"
#include "hbk_embed_args.h"      // kernel-argument structs and geometry constants
#include "hbk_embed_internal.h"  // one kernel-address function per family unit
#include "hbk_embed_plan.h"      // the host planner (no device call)

namespace hbk {
namespace {

constexpr int kChunkClips = 16384;     // clips per workspace chunk (default; HBK_EMBED_CHUNK overrides)
// clips per workspace chunk (HBK_EMBED_CHUNK: 256 .. 32,768): every chain kernel runs once per chunk (its last round of waves
// partly filled); measured: 100 k clips in 16,384-clip chunks 24.30 ms, in 32,768-clip chunks
// 24.43 ms, bit-identical (tools/embed_chunk_check.py), so the smaller workspace stays
inline int64_t chunk_clips() {
  static const int64_t c = [] {
    const char* e = getenv("HBK_EMBED_CHUNK");
    const long long v = e ? atoll(e) : 0;
    // (capped at 32,768, the size tools/embed_chunk_check.py validated: the chain kernels'
    // task counts are 32-bit and assume at most that many clips x windows x bands)
    return v >= 256 && v <= 32768 ? int64_t(v) : int64_t(kChunkClips);
  }();
  return c;
}

// ------------------------------------------------------------------ host ----

// Planning is hbk_embed_plan.h (pure host); here a plan is realised on the
// device and launched.
static_assert(kPlanOk == HBK_OK && kPlanErrArg == HBK_ERR_ARG && kPlanErrUnsupported == HBK_ERR_UNSUPPORTED &&
                  kOpConv == HBK_OP_CONV && kOpMaxPool == HBK_OP_MAXPOOL,
              "hbk_embed_plan.h mirrors include/hbk.h");

// One Launch of the host plan on the device: its kernel, its blob and its
// arguments with the blob's pointers in place.
struct Slot {
  const Launch* plan = nullptr;
  const void* fn = nullptr;  // null: nothing planned, or a pattern kernel the device refused
  void* d_blob = nullptr;
  int blocks_per_cu = 0;
  KernelArgs args;
};

struct ChainPlan {
  Slot pattern, base;  // tried in this order at launch
};

}  // namespace
}  // namespace hbk

struct hbk_embed_plan {
  hbk::EmbedHostPlan host;
  std::vector<hbk::ChainPlan> clip, win;  // beside host.clip.chains / host.win.chains
  int* d_gather = nullptr;                // host.clip.gather_src
  int* d_range = nullptr;                 // range flag of the split-f16 kernels (hbk_embed_range_status)
};

namespace hbk {
namespace {

// out[u][i][:] = src[u][gather_src[i]][:] (rows of `row` floats, row % 4 == 0);
// one wave per unit, all of a unit's reads ahead of its writes (distinct buffers)
__global__ void __launch_bounds__(256) embed_gather_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                           const int* __restrict__ map, int64_t n_units, int n_src,
                                                           int n_out, int row) {
  const int lane = threadIdx.x & 63;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (u >= n_units) return;
  const int r4 = row / 4, n4 = n_out * r4;
  const float4* s = reinterpret_cast<const float4*>(src + u * n_src * row);
  float4* d = reinterpret_cast<float4*>(out + u * n_out * row);
  for (int f = lane; f < n4; f += 64) {
    const int i = f / r4, c = f - i * r4;
    d[f] = s[map[i] * r4 + c];
  }
}

// The one reader of the planning knobs, called at every plan creation
// (HBK_EMBED_CHUNK is latched per process in chunk_clips).
EmbedKnobs read_embed_knobs() {
  EmbedKnobs k;
  if (const char* e = getenv("HBK_EMBED_LDS_KB")) {
    k.lds_kb_set = true;
    k.lds_kb = atoi(e);
  }
  if (const char* e = getenv("HBK_EMBED_WEIGHTS")) k.weights = !strcmp(e, "lds") ? 1 : !strcmp(e, "global") ? 2 : 0;
  k.no_p0 = getenv("HBK_EMBED_NO_P0") != nullptr;
  k.no_p0s = getenv("HBK_EMBED_NO_P0S") != nullptr;
  k.no_p1 = getenv("HBK_EMBED_NO_P1") != nullptr;
  k.no_p1s = getenv("HBK_EMBED_NO_P1S") != nullptr;
  k.no_p2s = getenv("HBK_EMBED_NO_P2S") != nullptr;
  k.no_t3s = getenv("HBK_EMBED_NO_T3S") != nullptr;
  k.no_dedup = getenv("HBK_EMBED_NO_DEDUP") != nullptr;
  if (const char* e = getenv("HBK_P0_BAND")) k.p0_band = atoi(e);
  k.debug = getenv("HBK_DEBUG_EMBED") != nullptr;
  if (const char* e = getenv("HBK_DEBUG_SKIP")) k.debug_skip = atoi(e);
  return k;
}

// The kernel that a KernelChoice names: each family unit knows its own.
const void* kernel_address(KernelChoice k) {
  switch (k.kind) {
    case Kern::exact: return embed_exact_kernel(k.n, k.flag);
    case Kern::x3: return embed_x3_kernel(k.n, k.flag);
    case Kern::p0_band:
    case Kern::p1: return embed_band_kernel(int(k.kind), k.n, k.flag);
    case Kern::p0s:
    case Kern::p1s:
    case Kern::p2s:
    case Kern::t3s: return embed_stream_kernel(int(k.kind), k.flag);
  }
  return nullptr;
}

// Dynamic-LDS limit of a kernel raised to what the CU holds beside its static
// LDS (set once to the maximum, so plans sharing the kernel never lower it).
hipError_t set_max_dynamic_lds(const void* fn) {
  hipFuncAttributes at;
  hipError_t e = hipFuncGetAttributes(&at, fn);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                             int(160 * 1024 - static_cast<int>(at.sharedSizeBytes)));
}

// The blob's addresses in the argument struct (Launch::ptr_off).
void set_pointers(ChainArgs& a, const Launch&, const unsigned char* blob) {
  a.wblob = reinterpret_cast<const float*>(blob);
}
void set_pointers(XArgs& x, const Launch& L, const unsigned char* blob) {
  x.wblob = reinterpret_cast<const _Float16*>(blob);
  x.bblob = reinterpret_cast<const float*>(blob + L.ptr_off[1]);
  x.ktab = reinterpret_cast<const int*>(blob + L.ptr_off[2]);
  x.i2c_off = reinterpret_cast<const int*>(blob + L.ptr_off[3]);
}
template <class A>
void set_pointers(A& p, const Launch& L, const unsigned char* blob) {  // the pattern kernels
  p.w = reinterpret_cast<const _Float16*>(blob);
  if (L.ptr_off[1] >= L.blob.size()) return;  // (p0s: its biases ride in the weights)
  const float* bias = reinterpret_cast<const float*>(blob + L.ptr_off[1]);
  if constexpr (std::is_same_v<A, P2sArgs>) p.bias_a = bias;
  else p.bias = bias;
}

// Uploads a Launch's bytes, points its arguments at them, resolves its kernel,
// raises the kernel's dynamic-LDS limit and prints the debug line. A pattern
// kernel whose upload, attribute or occupancy call fails is dropped silently
// (its slot stays empty and the chain runs on its generic kernel).
int realise(const Launch& L, bool pattern, bool debug, Slot& s) {
  const void* fn = kernel_address(L.kernel);
  hipError_t e = hipMalloc(&s.d_blob, L.blob.size());
  if (e != hipSuccess && !pattern) return hip_error(e, "hipMalloc chain weights");
  if (e == hipSuccess) e = hipMemcpy(s.d_blob, L.blob.data(), L.blob.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess && !pattern) return hip_error(e, "copy chain weights");
  if (pattern) {
    if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(L.lds_bytes));
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&s.blocks_per_cu, fn, L.threads, L.lds_bytes);
    if (e != hipSuccess || s.blocks_per_cu < 1) {
      (void)hipGetLastError();
      if (s.d_blob) (void)hipFree(s.d_blob);
      s.d_blob = nullptr;
      return HBK_OK;
    }
  } else {
    if (L.lds_bytes > 64 * 1024) {  // the CU maximum: chains sharing a kernel never lower it
      e = set_max_dynamic_lds(fn);
      if (e != hipSuccess) return hip_error(e, "hipFuncSetAttribute(max dynamic LDS)");
    }
    s.blocks_per_cu = L.kernel.kind == Kern::exact
                          ? 2
                          : std::max<int>(1, std::min<int>(4, int((160 * 1024) / std::max<size_t>(L.lds_bytes, 1))));
  }
  s.plan = &L;
  s.fn = fn;
  s.args = L.args;
  std::visit([&](auto& a) { set_pointers(a, L, static_cast<const unsigned char*>(s.d_blob)); }, s.args);
  if (debug && pattern) fprintf(stderr, "%s, %d blocks/CU\n", L.debug.c_str(), s.blocks_per_cu);
  if (debug && !pattern) fputs(L.debug.c_str(), stderr);
  return HBK_OK;
}

int realise_program(const ProgramPlan& prog, bool debug, std::vector<ChainPlan>& dev) {
  dev.resize(prog.chains.size());  // (all slots exist before the first allocation: destroy frees what was made)
  for (size_t k = 0; k < dev.size(); ++k) {
    const int rc = realise(prog.chains[k].base, false, debug, dev[k].base);
    if (rc) return rc;
    if (prog.chains[k].pattern) realise(*prog.chains[k].pattern, true, debug, dev[k].pattern);
  }
  return HBK_OK;
}

// The per-call fields of an argument struct.
void bind(ChainArgs& a, const float* in, int64_t stride, float* out, int64_t n_img, int*) {
  a.in = in;
  a.src_clip_stride = stride;
  a.out = out;
  a.n_img = n_img;
}
void bind(XArgs& x, const float* in, int64_t stride, float* out, int64_t n_img, int* range_flag) {
  x.range_flag = range_flag;
  x.in = in;
  x.src_clip_stride = stride;
  x.out = out;
  if ((reinterpret_cast<uintptr_t>(x.out) & 15) || (x.out_img_stride & 3)) x.vec_out = 0;
  if ((reinterpret_cast<uintptr_t>(x.in) & 15) || (x.src_clip_stride & 3) || (x.src_row_stride & 3)) x.raw_vec = 0;
  x.n_img = n_img;
}
template <class A>
void bind(A& p, const float* in, int64_t stride, float* out, int64_t n_img, int* range_flag) {  // the pattern kernels
  p.range_flag = range_flag;
  p.in = in;
  if constexpr (std::is_same_v<A, T3sArgs>) p.src_clip_stride = stride;
  else p.src_img_stride = stride;
  p.out = out;
  p.n_img = n_img;
}

// Runs chains [k_begin, k_end) of the program (k_end < 0: to the end). The
// first chain run reads `in` (the call's input, or for k_begin > 0 the output
// of chain k_begin - 1 in its workspace layout); the last writes `out` (for
// k_end < n: chain k_end - 1's output in its workspace layout, no gather).
// A chain runs on its pattern kernel when the buffers allow it, else on its
// generic kernel (split-f16 x3 or exact f32).
int run_program(const ProgramPlan& prog, const std::vector<ChainPlan>& dev, const int* d_gather, const float* in,
                int64_t n_units, int64_t in_unit_stride, float* out, int64_t out_unit_floats, float* ws,
                int64_t chunk, hipStream_t stream, int* range_flag, int k_begin = 0, int k_end = -1) {
  const int n_ch = static_cast<int>(prog.chains.size());
  if (k_end < 0) k_end = n_ch;
  for (int64_t u0 = 0; u0 < n_units; u0 += chunk) {
    const int64_t nu = std::min(chunk, n_units - u0);
    float* bufs[2] = {ws, ws + chunk * prog.buf_floats[0]};
    for (int k = k_begin; k < k_end; ++k) {
      const ChainHost& h = prog.chains[k];
      const int src_buf = (k == k_begin && k_begin > 0) ? -1 : h.src_buf;  // the caller's copy of chain k - 1's output
      const int dst_buf = (k == k_end - 1 && k_end < n_ch) ? -1 : h.dst_buf;  // handed to the caller (no gather)
      const float* src = src_buf < 0 ? in + u0 * in_unit_stride : bufs[src_buf];
      const int64_t stride = src_buf < 0 ? in_unit_stride : h.src_clip_stride;
      float* dst = dst_buf < 0 ? out + u0 * out_unit_floats : bufs[dst_buf];
      const int64_t n_img = nu * h.imgs_per_unit;
      for (const Slot* s : {&dev[k].pattern, &dev[k].base}) {
        if (!s->fn) continue;
        const Launch& L = *s->plan;
        if (s == &dev[k].pattern) {
          const bool aligned = !(reinterpret_cast<uintptr_t>(src) & 15) && !(stride & 3) &&
                               !(reinterpret_cast<uintptr_t>(dst) & 15) && !(L.out_stride_4 & 3);
          if (!aligned || stride < L.min_src_stride) continue;
          if (L.tasks_below_2_31 && n_img * L.n_bands >= (int64_t(1) << 31)) continue;
        }
        KernelArgs args = s->args;
        void* argp = std::visit(
            [&](auto& a) -> void* {
              bind(a, src, stride, dst, n_img, range_flag);
              return &a;
            },
            args);
        const int64_t tasks = ((n_img + L.imgs_per_task - 1) / L.imgs_per_task) * L.n_bands;
        const int64_t blocks = std::min<int64_t>(tasks, persistent_blocks(s->blocks_per_cu, stream));
        if (blocks > 0) {
          (void)hipLaunchKernel(s->fn, dim3(unsigned(blocks)), dim3(L.threads), &argp, L.lds_bytes, stream);
          HBK_LAUNCH_CHECK(L.name);
        }
        break;
      }
    }
    if (prog.gather_buf >= 0 && k_end == n_ch) {
      const int n_out = static_cast<int>(prog.gather_src.size());
      const int row = static_cast<int>(out_unit_floats / n_out);
      hipLaunchKernelGGL(embed_gather_kernel, dim3(unsigned((nu + 3) / 4)), dim3(256), 0, stream,
                         bufs[prog.gather_buf], out + u0 * out_unit_floats, d_gather, nu, prog.n_src, n_out, row);
      HBK_LAUNCH_CHECK("embed_gather_kernel");
    }
  }
  return HBK_OK;
}

// The clip / window entry points past their plan check: chains [k_begin, k_end)
// of the clip program (or the window program) over n units in workspace chunks.
int run_units(const hbk_embed_plan* p, bool clips, const float* in, int64_t n, int64_t in_stride, int64_t min_stride,
              float* out, int64_t out_floats, void* workspace, int64_t workspace_bytes, void* stream, int k_begin = 0,
              int k_end = -1) {
  if (n < 0) return arg_error(clips ? "negative n_clips" : "negative n");
  if (n == 0) return HBK_OK;
  if (!in || !out || !workspace) return arg_error("NULL pointer");
  if (in_stride < min_stride) return arg_error("mel_clip_stride < seq_frames * in_w");
  int64_t need = 0;
  hbk_embed_workspace_size(p, n, &need);
  if (workspace_bytes < need) return arg_error("workspace too small");
  return run_program(clips ? p->host.clip : p->host.win, clips ? p->clip : p->win, p->d_gather, in, n, in_stride, out,
                     out_floats, static_cast<float*>(workspace), std::min<int64_t>(n, chunk_clips()),
                     as_stream(stream), p->d_range, k_begin, k_end);
}

}  // namespace
}  // namespace hbk

extern "C" {

int hbk_embed_plan_create(const hbk_graph_op* ops, int32_t n_ops, int32_t in_h, int32_t in_w,
                          const int32_t* win_start, int32_t n_win, hbk_embed_plan** plan) {
  return hbk_embed_plan_create_ex(ops, n_ops, in_h, in_w, win_start, n_win, HBK_PREC_SPLIT_F16, plan);
}

int hbk_embed_plan_create_ex(const hbk_graph_op* ops, int32_t n_ops, int32_t in_h, int32_t in_w,
                             const int32_t* win_start, int32_t n_win, int32_t precision,
                             hbk_embed_plan** plan) {
  using namespace hbk;
  if (!plan) return arg_error("plan is NULL");
  *plan = nullptr;
  if (precision != HBK_PREC_SPLIT_F16 && precision != HBK_PREC_EXACT_F32) return arg_error("unknown precision");
  if (!ops || n_ops <= 0) return arg_error("empty graph");
  if (in_h <= 0 || in_w <= 0) return arg_error("bad window size");
  if (!win_start || n_win <= 0 || n_win > kMaxWin) return arg_error("n_win must be in [1, 32]");
  auto* p = new hbk_embed_plan();
  auto fail = [&](int rc) {
    hbk_embed_plan_destroy(p);
    return rc;
  };
  // the whole plan on the host, with every planning error, before the first device call
  const EmbedKnobs knobs = read_embed_knobs();
  std::vector<OpIn> graph;
  for (int i = 0; i < n_ops; ++i) {
    const hbk_graph_op& o = ops[i];
    graph.push_back(OpIn{o.kind, o.kh, o.kw, o.cin, o.cout, o.act, o.alpha, o.weight, o.bias});
  }
  int rc = plan_embed(graph, in_h, in_w, std::vector<int>(win_start, win_start + n_win),
                      precision == HBK_PREC_SPLIT_F16, knobs, p->host);
  if (rc) {
    set_error("%s", p->host.error.c_str());
    return fail(rc);
  }
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_range), sizeof(int));
  if (e == hipSuccess) e = hipMemset(p->d_range, 0, sizeof(int));
  if (e != hipSuccess) return fail(hip_error(e, "hipMalloc range flag"));
  rc = realise_program(p->host.clip, knobs.debug, p->clip);
  if (rc) return fail(rc);
  if (const std::vector<int>& map = p->host.clip.gather_src; !map.empty()) {
    e = hipMalloc(reinterpret_cast<void**>(&p->d_gather), map.size() * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(p->d_gather, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(hip_error(e, "embed gather map"));
    if (knobs.debug) fputs(p->host.dedup_debug.c_str(), stderr);
  }
  rc = realise_program(p->host.win, knobs.debug, p->win);
  if (rc) return fail(rc);
  *plan = p;
  return HBK_OK;
}

int hbk_embed_plan_destroy(hbk_embed_plan* p) {
  if (!p) return HBK_OK;
  for (auto* dev : {&p->clip, &p->win})
    for (auto& c : *dev)
      for (hbk::Slot* s : {&c.pattern, &c.base})
        if (s->d_blob) (void)hipFree(s->d_blob);
  if (p->d_gather) (void)hipFree(p->d_gather);
  if (p->d_range) (void)hipFree(p->d_range);
  delete p;
  return HBK_OK;
}

int hbk_embed_plan_info(const hbk_embed_plan* p, int32_t* out_dim, int32_t* n_prefix_ops,
                        int32_t* n_chains, double* prefix_macs, double* tail_macs,
                        int32_t* seq_frames) {
  if (!p) return hbk::arg_error("plan is NULL");
  if (out_dim) *out_dim = p->host.out_dim;
  if (n_prefix_ops) *n_prefix_ops = p->host.n_prefix;
  if (n_chains) *n_chains = static_cast<int32_t>(p->host.clip.chains.size());
  if (prefix_macs) *prefix_macs = p->host.prefix_macs;
  if (tail_macs) *tail_macs = p->host.tail_macs;
  if (seq_frames) *seq_frames = p->host.seq_frames;
  return HBK_OK;
}

}  // extern "C"

extern "C" {

int hbk_embed_workspace_size(const hbk_embed_plan* p, int64_t n, int64_t* bytes) {
  using namespace hbk;
  if (!p || !bytes) return arg_error("plan/bytes is NULL");
  if (n < 0) return arg_error("negative n");
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, chunk_clips()));
  const int64_t *bc = p->host.clip.buf_floats, *bw = p->host.win.buf_floats;
  *bytes = chunk * std::max(bc[0] + bc[1], bw[0] + bw[1]) * int64_t(sizeof(float)) + 256;
  return HBK_OK;
}

int hbk_embed_clips(const hbk_embed_plan* p, const float* mel, int64_t n_clips, int64_t mel_clip_stride,
                    float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  if (!p) return arg_error("plan is NULL");
  return run_units(p, true, mel, n_clips, mel_clip_stride, int64_t(p->host.seq_frames) * p->host.in_w, out,
                   int64_t(p->host.n_win) * p->host.out_dim, workspace, workspace_bytes, stream);
}

int hbk_embed_split_info(const hbk_embed_plan* p, int32_t n_front, int64_t* mid_floats_per_clip) {
  using namespace hbk;
  if (!p || !mid_floats_per_clip) return arg_error("plan/mid_floats_per_clip is NULL");
  const int n = static_cast<int>(p->host.clip.chains.size());
  if (n_front < 1 || n_front >= n) return arg_error("n_front must be in [1, n_chains - 1]");
  const ChainHost& c = p->host.clip.chains[n_front - 1];
  *mid_floats_per_clip = c.out_img_stride * c.imgs_per_unit;
  return HBK_OK;
}

int hbk_embed_clips_front(const hbk_embed_plan* p, const float* mel, int64_t n_clips, int64_t mel_clip_stride,
                          int32_t n_front, float* mid, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  int64_t mid_floats = 0;
  int rc = hbk_embed_split_info(p, n_front, &mid_floats);
  if (rc) return rc;
  return run_units(p, true, mel, n_clips, mel_clip_stride, int64_t(p->host.seq_frames) * p->host.in_w, mid,
                   mid_floats, workspace, workspace_bytes, stream, 0, n_front);
}

int hbk_embed_clips_back(const hbk_embed_plan* p, const float* mid, int64_t n_clips, int32_t n_front, float* out,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  int64_t mid_floats = 0;
  int rc = hbk_embed_split_info(p, n_front, &mid_floats);
  if (rc) return rc;
  return run_units(p, true, mid, n_clips, mid_floats, 0, out, int64_t(p->host.n_win) * p->host.out_dim, workspace,
                   workspace_bytes, stream, n_front, -1);
}

int hbk_embed_windows(const hbk_embed_plan* p, const float* windows, int64_t n, float* out,
                      void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  if (!p) return arg_error("plan is NULL");
  return run_units(p, false, windows, n, int64_t(p->host.in_h) * p->host.in_w, 0, out, p->host.out_dim, workspace,
                   workspace_bytes, stream);
}

int hbk_embed_range_status(const hbk_embed_plan* p, int32_t* tripped, int32_t reset, void* stream) {
  using namespace hbk;
  if (!p || !tripped) return arg_error("plan/tripped is NULL");
  int32_t h = 0;
  hipError_t e = hipMemcpyAsync(&h, p->d_range, sizeof(int32_t), hipMemcpyDeviceToHost, as_stream(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(as_stream(stream));
  if (e == hipSuccess && reset && h) e = hipMemsetAsync(p->d_range, 0, sizeof(int32_t), as_stream(stream));
  if (e != hipSuccess) return hip_error(e, "hbk_embed_range_status");
  *tripped = h;
  return HBK_OK;
}

}  // extern "C"
