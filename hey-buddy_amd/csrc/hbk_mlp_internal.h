// The classifier plan shared by hbk_mlp.hip (generic GEMM path, any dims) and the
// fused path for the default architecture: hbk_mlp_fused.hip (train step) and
// hbk_mlp_eval.hip (evaluation passes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hbk_mlp_act.h"
#include "hbk_mlp_dims.h"
#include "hbk_mlp_half_plan.h"

namespace hbk {

struct Gmlp {
  int in, hid, out;
  int64_t w_hg, b_hg, w_o, b_o;  // float offsets into the flat parameter buffer
  // rows of W_hg = columns of HG: 2 hid (hidden rows then gate rows), or hid in a plain plan
  // (hbk_mlp_plan_create_ex with gated = 0: W_hg / b_hg are hidden.weight / hidden.bias alone)
  int wid = 0;
};
struct Ln {
  int d;
  int64_t g, b;
};

}  // namespace hbk

struct hbk_mlp_plan {
  int d_in = 0, layer = 0, hid = 0, n_layers = 0;
  hbk::Ln ln_in;
  std::vector<hbk::Gmlp> g;  // mlp_in, layers..., mlp_out
  std::vector<hbk::Ln> ln;   // layers' LNs..., norm_out
  int64_t n_params = 0;
  // hbk_mlp_plan_create_ex: MultiLayerPerceptron blocks (no gate) when false; the activation
  // (HBK_ACT_*). Gated SiLU is the default architecture, the only one the fused kernels, the
  // evaluation passes and the half-layer bank cover.
  bool gated = true;
  int act = HBK_ACT_SILU;
  bool default_block() const { return gated && act == HBK_ACT_SILU; }
  // the half-layer bank (hbk_mlp_plan_create_half; half.n_half = 0: none), its parameters after
  // the block above, and each branch's token indices [n_half][n_tokens / 2]
  hbk::HalfDims half;
  hbk::HalfOffsets half_off{};
  std::vector<int32_t> half_idx;
  // hbk_mlp_set_step_scalars: device [lr, neg_weight, seed] read by the train
  // kernels in place of their by-value arguments (graph-captured steps)
  const double* step_scalars = nullptr;
  // hbk_mlp_step_fwd_bwd with HBK_STEP_DEFER_PARTIALS left its weight-gradient
  // slabs (deferred_ks of them) in this workspace for the next hbk_mlp_step_update
  mutable const void* deferred_ws = nullptr;
  mutable int deferred_ks = 0;
  // ... and with HBK_STEP_GATE_SKIP (the knob of that name's value then; 0: without): on a step
  // that does not fire the slabs are an earlier step's, and the update must not use them
  mutable int deferred_gate = 0;
};

namespace hbk {
// Counter-based uniform in [0, 1) (splitmix64 of seed ^ index): the input
// dropout mask of element i of a step is a pure function of (seed, i).
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t i) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return static_cast<float>(z >> 40) * (1.f / 16777216.f);
}

// Adam's parameter step, torch's step_size * m / (sqrt(v) / bc2s + eps), on the
// hardware v_sqrt_f32 / v_rcp_f32 (1 ulp each) instead of the IEEE square root
// and two IEEE divisions; shared by k4 and the generic adam_kernel so that the
// two update paths stay bit-identical (k4: 12.0 -> 10.9 us per step on 64 CUs)
__device__ __forceinline__ float adam_step(float mi, float vi, float step_size, float inv_bc2s, float eps) {
  return step_size * mi * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(vi) * inv_bc2s + eps);
}

// Grid of an elementwise grid-stride kernel over n elements, 256 threads per block
inline unsigned mlp_ew_grid(int64_t n) { return static_cast<unsigned>(std::min<int64_t>((n + 255) / 256, 4096)); }

// The activation step of one MLP block for any (HBK_ACT_*, gated) pair (hbk_mlp_act.hip).
// Forward: u [rows, H] = f(H) (* G) from hg [rows, gated ? 2H : H]; backward: dhg of hg's shape
// from du [rows, H] and the same hg.
int mlp_act_forward(int act, bool gated, const float* hg, float* u, int rows, int H, hipStream_t s);
int mlp_act_backward(int act, bool gated, const float* du, const float* hg, float* dhg, int rows, int H,
                     hipStream_t s);

// True when the fused kernels (train step: hbk_mlp_fused.hip; evaluation passes:
// hbk_mlp_eval.hip) cover this plan.
bool mlp_fused_supported(const hbk_mlp_plan& p);
// The weight cache both read (f16 hi / lo planes of W_o_k, k < NG - 1, and W_hg_k, k >= 1, as
// stored and transposed; hbk_mlp_dev.h: WSplit): its planes' offsets in halves from the cache
// base, and its fill from the parameters (k0_wsplit_kernel, in hbk_mlp_fused.hip)
struct WCacheOffsets {
  int64_t c_o[kMaxG], c_oT[kMaxG], c_hg[kMaxG], c_hgT[kMaxG];
};
WCacheOffsets mlp_wcache_offsets(const hbk_mlp_plan& p);
int mlp_wcache_fill(const hbk_mlp_plan& p, const float* params, float* cache, hipStream_t s);
int64_t mlp_fused_ws_floats(const hbk_mlp_plan& p, int64_t B);
// 1 (k1a / k1b / k3) or 2 (k1s / k1c / k3s): the train step mlp_fused_run takes for B rows on s
int mlp_fused_step_variant(int64_t B, hipStream_t s);
// The plan mlp_fused_run takes for B rows on s (hbk_mlp_step_plan_info's fields); launches nothing
constexpr int kStepPlanInfo = 19;
void mlp_fused_step_plan_info(const hbk_mlp_plan& p, int64_t B, hipStream_t s, int32_t info[kStepPlanInfo]);
int mlp_fused_run(const hbk_mlp_plan& p, const float* params, const float* pool32, int64_t n32,
                  const void* pool16, int64_t n16, const int32_t* idx, int64_t idx_stride, int64_t idx_steps,
                  const float* y, int64_t y_stride, int B, const float* state, int parity, const float* sched,
                  int sched_len, float neg_weight, float thr, float act_thr, float drop_p, uint64_t seed,
                  float* bucket, float* prob, float* logit, float* ws, bool train, int flags, hipStream_t s);
int mlp_fused_update(const hbk_mlp_plan& p, float* params, float* bucket, float* m, float* v, float* state,
                     int parity, const float* sched, int sched_len, float lr, float b1, float b2, float eps,
                     float* hist, int hist_cap, float* ws, hipStream_t s);
// Half-layer bank (hbk_mlp_half.hip), called from the generic forward / backward of hbk_mlp.hip.
// ws: the bank's workspace (half_ws_layout). Forward: s0 [B, layer] += sum_h branch_h(x) and keeps
// statistics, HG, U and (drop_p > 0) the dropped-out input; backward, after that forward on the same ws
// with the same drop_p: the bank's gradients from ds0 [B, layer] into bucket G (zeroed).
int mlp_half_forward(const hbk_mlp_plan& p, const float* params, const float* x, int B, float* s0, float* ws,
                     float drop_p, uint64_t seed, const double* step_sc, hipStream_t s);
int mlp_half_backward(const hbk_mlp_plan& p, const float* params, const float* x, int B, const float* ds0,
                      float* G, float* ws, float drop_p, hipStream_t s);
// Evaluation passes (validation / testing forwards reduced to prediction counts)
int64_t mlp_eval_ws_floats(const hbk_mlp_plan& p, int64_t rows);
int mlp_eval_prepare(const hbk_mlp_plan& p, const float* params, float* ws, hipStream_t s);
int mlp_eval_count(const hbk_mlp_plan& p, const float* params, const void* pool, bool f16, int64_t n_pool,
                   const int32_t* idx, int64_t rows, int64_t r0, int label, float act_thr, float drop_p,
                   uint64_t seed, float* counts, float* prob, float* ws, hipStream_t s);
// the rows mlp_eval_count evaluates in the lap form (two laps of the pool together) and in the plain form
void mlp_eval_lap_plan(int64_t rows, int64_t n_pool, bool f16, bool has_idx, int64_t part[2]);
// one pool of an evaluation launch (mlp_eval_count_multi: several pools of one dtype in one launch)
struct EvalSeg {
  const void* pool;
  int64_t n_pool, rows, r0;
  uint64_t seed;
  float* counts;
  int label;
};
constexpr int kEvalMaxSeg = 4;
int mlp_eval_count_multi(const hbk_mlp_plan& p, const float* params, bool f16, const EvalSeg* seg, int nseg,
                         float act_thr, float drop_p, float* ws, hipStream_t s);
int mlp_eval_finish(const float* cv, const float* ct, const double* sizes, float target, float ratio, float* sched,
                    int64_t sched_len, int64_t next_step, float* out, hipStream_t s);
}  // namespace hbk
