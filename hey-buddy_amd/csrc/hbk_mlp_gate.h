// The < 128-sample accumulation gate of a train step (trainer.py:443-465), once: the
// generic gate_kernel (hbk_mlp.hip), the fused update k4_update_kernel and, with
// HBK_STEP_GATE_SKIP, the weight-gradient kernels (hbk_mlp_fused.hip) all decide with
// this function, from the same device words, so they cannot disagree. No HIP include:
// tests/gate_rule_check.cpp compiles this header alone and walks it on a CPU.
#pragma once

#if defined(__HIPCC__)
#define HBK_GATE_HD __host__ __device__
#else
#define HBK_GATE_HD
#endif

namespace hbk {

constexpr float kGateSamples = 128.f;  // the reference's minimum of accumulated selected rows per update

struct StepGate {
  float acc_samples, acc_steps, adam_t;  // the state after the step
  float fire;                            // 1: the optimizer steps (else 0)
  float scale;                           // ... on grads * scale = grads / (n_sel * accumulation steps used)
};

// A step that selected n_sel rows (the bucket's statistic 0), from the state before it.
// n_sel = 0 leaves everything alone (the reference `continue`s before the gate).
HBK_GATE_HD inline StepGate step_gate(float acc_samples, float acc_steps, float adam_t, float n_sel) {
  StepGate g{acc_samples, acc_steps, adam_t, 0.f, 0.f};
  if (n_sel > 0.f) {
    g.acc_samples = acc_samples + n_sel;
    if (g.acc_samples < kGateSamples) {
      g.acc_steps = acc_steps + 1.f;
    } else {
      g.fire = 1.f;
      g.scale = 1.f / (n_sel * acc_steps);
      g.acc_steps = 1.f;
      g.acc_samples = 0.f;
      g.adam_t = adam_t + 1.f;
    }
  }
  return g;
}

}  // namespace hbk
