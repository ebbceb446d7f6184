// What the classifier's translation units share. hbk_mlp.hip: the generic GEMM path (any dims), the
// plan constructors and its entry points; hbk_mlp_act.hip: the activation step of plans other than
// gated SiLU; hbk_mlp_half.hip: the half-layer bank; hbk_mlp_fused.hip: the fused train step of the
// default architecture; hbk_mlp_eval.hip: its evaluation passes. Every extern "C" entry point lives
// beside the kernels it launches, so only these cross a unit: the plan itself, the device helpers
// that hbk_mlp.hip and hbk_mlp_half.hip both use, the activation, gate and half-bank calls of the
// generic forward / backward, the three fused calls behind hbk_mlp_forward / hbk_mlp_workspace_size,
// and the weight cache the evaluation unit borrows from the train step.
// The host-only geometry is in hbk_mlp_layout.h (generic path), hbk_mlp_half_plan.h (bank) and
// hbk_mlp_plan.h (fused step).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "hbk_mlp_act.h"
#include "hbk_mlp_dims.h"
#include "hbk_mlp_half_plan.h"
#include "hbk_mlp_layout.h"

// ln_in, g, ln, n_params: hbk_mlp_layout.h (a half plan's n_params also counts the bank)
struct hbk_mlp_plan : hbk::MlpParams {
  int d_in = 0, layer = 0, hid = 0, n_layers = 0;
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

// The three helpers below are shared by hbk_mlp.hip and hbk_mlp_half.hip (the fused units have
// their own forms in hbk_mlp_dev.h: another reduction order, other instructions, other bits).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// Input dropout (nn.Dropout, wakeword.py:197/338: zero with prob p, scale by 1/(1-p)) of the value v
// at element e of the flattened [B, d_in] input: norm_in and every half-layer branch see one mask.
__device__ __forceinline__ float dropout_elem(float v, uint64_t seed, uint64_t e, float p, float keep_scale) {
  if (p <= 0.f) return v;
  return uniform01(seed, e) < p ? 0.f : v * keep_scale;
}

// fused-only entry points on a plan they do not cover: sets the message, returns HBK_ERR_UNSUPPORTED
// (hbk_mlp_fused.hip)
int mlp_unsupported(const hbk_mlp_plan& p, const char* what);

// The activation step of one MLP block for any (HBK_ACT_*, gated) pair (hbk_mlp_act.hip).
// Forward: u [rows, H] = f(H) (* G) from hg [rows, gated ? 2H : H]; backward: dhg of hg's shape
// from du [rows, H] and the same hg.
int mlp_act_forward(int act, bool gated, const float* hg, float* u, int rows, int H, hipStream_t s);
int mlp_act_backward(int act, bool gated, const float* du, const float* hg, float* dhg, int rows, int H,
                     hipStream_t s);
// The gated SiLU block's own forward, u [rows, H] = silu(H) * G from hg [rows, 2H] (gate_fwd_kernel in
// hbk_mlp.hip), which the half-layer bank runs over its [B n_half, H] too.
int mlp_gate_forward(const float* hg, float* u, int rows, int H, hipStream_t s);

// True when the fused kernels (train step: hbk_mlp_fused.hip; evaluation passes:
// hbk_mlp_eval.hip) cover this plan.
bool mlp_fused_supported(const hbk_mlp_plan& p);
// hbk_mlp_forward on such a plan (train = false) and hbk_mlp_step_fwd_bwd: hbk_mlp_fused.hip
int64_t mlp_fused_ws_floats(const hbk_mlp_plan& p, int64_t B);
int mlp_fused_run(const hbk_mlp_plan& p, const float* params, const float* pool32, int64_t n32,
                  const void* pool16, int64_t n16, const int32_t* idx, int64_t idx_stride, int64_t idx_steps,
                  const float* y, int64_t y_stride, int B, const float* state, int parity, const float* sched,
                  int sched_len, float neg_weight, float thr, float act_thr, float drop_p, uint64_t seed,
                  float* bucket, float* prob, float* logit, float* ws, bool train, int flags, hipStream_t s);
// The weight cache the train step and the evaluation passes read (f16 hi / lo planes of W_o_k,
// k < NG - 1, and W_hg_k, k >= 1, as stored and transposed; hbk_mlp_dev.h: WSplit): its planes'
// offsets in halves from the cache base, and its fill from the parameters (k0_wsplit_kernel, in
// hbk_mlp_fused.hip)
struct WCacheOffsets {
  int64_t c_o[kMaxG], c_oT[kMaxG], c_hg[kMaxG], c_hgT[kMaxG];
};
WCacheOffsets mlp_wcache_offsets(const hbk_mlp_plan& p);
int mlp_wcache_fill(const hbk_mlp_plan& p, const float* params, float* cache, hipStream_t s);

// Half-layer bank (hbk_mlp_half.hip), called from the generic forward / backward of hbk_mlp.hip.
// ws: the bank's workspace (half_ws_layout). Forward: s0 [B, layer] += sum_h branch_h(x) and keeps
// statistics, HG, U and (drop_p > 0) the dropped-out input; backward, after that forward on the same ws
// with the same drop_p: the bank's gradients from ds0 [B, layer] into bucket G (zeroed).
int mlp_half_forward(const hbk_mlp_plan& p, const float* params, const float* x, int B, float* s0, float* ws,
                     float drop_p, uint64_t seed, const double* step_sc, hipStream_t s);
int mlp_half_backward(const hbk_mlp_plan& p, const float* params, const float* x, int B, const float* ds0,
                      float* G, float* ws, float drop_p, hipStream_t s);
}  // namespace hbk
