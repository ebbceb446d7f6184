// Dimensions of the fused classifier (default architecture: d_in = 16 x 96 =
// 1536, layer_dim 96, hidden get_normalized_dim(96) = 64, 0..2 layers), shared by
// the device code (hbk_mlp_dev.h) and the step's host planning (hbk_mlp_plan.h), and
// the one constant every classifier unit shares. Plain C++: no HIP include.
#pragma once

namespace hbk {

constexpr int kD = 1536, kL = 96, kH = 64, kH2 = 128;
constexpr int kR = 16;            // rows per tile = MFMA M
constexpr int kMaxG = 4;          // gated MLPs held by k2 (n_layers <= 2: the LDS budget)
constexpr int kLd = 132;          // LDS row stride of [16][<=128] activation tiles
constexpr int kMaskW = kD / 32;   // dropout mask words per row (v2 step)
constexpr float kLnEps = 1e-5f;   // nn.LayerNorm's eps, in every LayerNorm of every path

}  // namespace hbk
