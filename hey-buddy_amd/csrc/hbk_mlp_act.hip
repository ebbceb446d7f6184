// The activation step of a classifier MLP block for every (activation, gated) pair the
// reference builds (modules/multi_layer_perceptron.py:18-124), forward and backward, for the
// generic path of hbk_mlp.hip. A gated SiLU plan keeps gate_fwd_kernel / gate_bwd_kernel there.
//
// One element per thread and iteration, as in those two kernels: the arrays are B x H with
// H = 64 at the defaults (281 KB at B = 1,100), so a launch is bound by its latency and by the
// transcendental calls per element, not by the number of load instructions; 16-byte accesses
// would need H % 4 == 0 and aligned bases, which the ABI (any hidden > 0, caller-owned
// buffers) does not promise.
#include "hbk_common.h"
#include "hbk_mlp_act.h"
#include "hbk_mlp_internal.h"

namespace hbk {
namespace {

// Gated: U = f(H) * G from HG [rows, 2H]. Plain: U = f(H) from H [rows, H].
template <Act A, bool GATED>
__global__ void act_fwd_kernel(const float* __restrict__ hg, float* __restrict__ u, int rows, int H) {
  const int64_t n = static_cast<int64_t>(rows) * H;
  for (int64_t e = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; e < n; e += int64_t(gridDim.x) * blockDim.x) {
    if constexpr (GATED) {
      const int64_t r = e / H;
      const int j = static_cast<int>(e - r * H);
      const float h = hg[r * 2 * H + j], g = hg[r * 2 * H + H + j];
      u[e] = act_f<A>(h) * g;
    } else {
      u[e] = act_f<A>(hg[e]);
    }
  }
}

// Gated: dH = dU * G * f'(H), dG = dU * f(H) into dHG [rows, 2H]. Plain: dH = dU * f'(H) into [rows, H].
template <Act A, bool GATED>
__global__ void act_bwd_kernel(const float* __restrict__ du, const float* __restrict__ hg,
                               float* __restrict__ dhg, int rows, int H) {
  const int64_t n = static_cast<int64_t>(rows) * H;
  for (int64_t e = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; e < n; e += int64_t(gridDim.x) * blockDim.x) {
    const float d = du[e];
    if constexpr (GATED) {
      const int64_t r = e / H;
      const int j = static_cast<int>(e - r * H);
      const float h = hg[r * 2 * H + j], g = hg[r * 2 * H + H + j];
      dhg[r * 2 * H + j] = d * g * act_df<A>(h);
      dhg[r * 2 * H + H + j] = d * act_f<A>(h);
    } else {
      dhg[e] = d * act_df<A>(hg[e]);
    }
  }
}

template <Act A, bool GATED>
int launch(const float* du, const float* hg, float* out, int rows, int H, hipStream_t s) {
  const dim3 grid(mlp_ew_grid(int64_t(rows) * H)), block(256);
  if (du) {
    hipLaunchKernelGGL((act_bwd_kernel<A, GATED>), grid, block, 0, s, du, hg, out, rows, H);
    HBK_LAUNCH_CHECK("act_bwd_kernel");
  } else {
    hipLaunchKernelGGL((act_fwd_kernel<A, GATED>), grid, block, 0, s, hg, out, rows, H);
    HBK_LAUNCH_CHECK("act_fwd_kernel");
  }
  return HBK_OK;
}

template <Act A>
int launch_g(bool gated, const float* du, const float* hg, float* out, int rows, int H, hipStream_t s) {
  return gated ? launch<A, true>(du, hg, out, rows, H, s) : launch<A, false>(du, hg, out, rows, H, s);
}

// du == nullptr: forward (out = U); else backward (out = dHG)
int dispatch(int act, bool gated, const float* du, const float* hg, float* out, int rows, int H, hipStream_t s) {
  if (rows <= 0) return HBK_OK;
  switch (static_cast<Act>(act)) {
    case Act::Silu: return launch_g<Act::Silu>(gated, du, hg, out, rows, H, s);
    case Act::Relu: return launch_g<Act::Relu>(gated, du, hg, out, rows, H, s);
    case Act::Gelu: return launch_g<Act::Gelu>(gated, du, hg, out, rows, H, s);
    case Act::Mish: return launch_g<Act::Mish>(gated, du, hg, out, rows, H, s);
    case Act::Tanh: return launch_g<Act::Tanh>(gated, du, hg, out, rows, H, s);
    case Act::Sigmoid: return launch_g<Act::Sigmoid>(gated, du, hg, out, rows, H, s);
    case Act::Identity: return launch_g<Act::Identity>(gated, du, hg, out, rows, H, s);
  }
  return arg_error("unknown activation code");
}

int check_args(int64_t rows, int32_t hidden, int32_t gated, int32_t activation) {
  if (rows < 0 || rows > (1 << 24)) return arg_error("rows out of range");
  if (hidden <= 0 || hidden > (1 << 20)) return arg_error("hidden out of range");
  if (gated != 0 && gated != 1) return arg_error("gated must be 0 or 1");
  if (!act_valid(activation)) return arg_error("unknown activation code");
  return HBK_OK;
}

}  // namespace

int mlp_act_forward(int act, bool gated, const float* hg, float* u, int rows, int H, hipStream_t s) {
  return dispatch(act, gated, nullptr, hg, u, rows, H, s);
}

int mlp_act_backward(int act, bool gated, const float* du, const float* hg, float* dhg, int rows, int H,
                     hipStream_t s) {
  return dispatch(act, gated, du, hg, dhg, rows, H, s);
}

}  // namespace hbk

extern "C" {

int hbk_mlp_act_forward(const float* hg, int64_t rows, int32_t hidden, int32_t gated, int32_t activation, float* u,
                        void* stream) {
  using namespace hbk;
  const int rc = check_args(rows, hidden, gated, activation);
  if (rc) return rc;
  if (rows == 0) return HBK_OK;
  if (!hg || !u) return arg_error("NULL pointer");
  return mlp_act_forward(activation, gated != 0, hg, u, static_cast<int>(rows), hidden, as_stream(stream));
}

int hbk_mlp_act_backward(const float* du, const float* hg, int64_t rows, int32_t hidden, int32_t gated,
                         int32_t activation, float* dhg, void* stream) {
  using namespace hbk;
  const int rc = check_args(rows, hidden, gated, activation);
  if (rc) return rc;
  if (rows == 0) return HBK_OK;
  if (!du || !hg || !dhg) return arg_error("NULL pointer");
  return mlp_act_backward(activation, gated != 0, du, hg, dhg, static_cast<int>(rows), hidden, as_stream(stream));
}

}  // extern "C"
