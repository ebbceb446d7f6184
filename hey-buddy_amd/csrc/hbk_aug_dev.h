// Device helpers that more than one augmentation unit uses (hbk_augment.hip,
// hbk_clip_ops.hip): the small DFTs in registers, the DPP wave sum and the block
// sums over a kThreads block, the opaque thread id, and the register copy of a
// clip. Everything is internal to the unit that includes it.
#pragma once

#include "hbk_augment_plan.h"
#include "hbk_common.h"

namespace hbk {
namespace {

// ---- small DFTs in registers (constant twiddles) --------------------------
template <bool INV>
__device__ __forceinline__ cf tw_const(double frac) {  // exp(-+2 pi i frac)
  const double a = (INV ? 2.0 : -2.0) * M_PI * frac;
  return cf{static_cast<float>(cos(a)), static_cast<float>(sin(a))};
}

template <bool INV>
__device__ __forceinline__ void dft3(cf& a, cf& b, cf& c) {
  // X0 = a+b+c; X1 = a + w b + w^2 c; X2 = a + w^2 b + w c, w = exp(-+2pi i/3)
  constexpr float h = 0.5f, s = 0.86602540378443865f;
  const cf t = b + c;
  const cf d = b - c;
  const cf m = a - h * t;
  // (-+) i s d
  const cf r = INV ? cf{-s * d.y, s * d.x} : cf{s * d.y, -s * d.x};
  a = a + t;
  b = m + r;
  c = m - r;
}

template <bool INV>
__device__ __forceinline__ void dft5(cf (&x)[5]) {
  cf y[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    cf acc = x[0];
#pragma unroll
    for (int n = 1; n < 5; ++n) acc = acc + cmul(x[n], tw_const<INV>(double((n * k) % 5) / 5.0));
    y[k] = acc;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) x[k] = y[k];
}

// DFT-9 as 3 x 3: n = 3u + v, k = c + 3d
template <bool INV>
__device__ __forceinline__ void dft9(cf (&x)[9]) {
#pragma unroll
  for (int v = 0; v < 3; ++v) dft3<INV>(x[v], x[3 + v], x[6 + v]);  // x[3c + v] = A[v][c]
#pragma unroll
  for (int c = 1; c < 3; ++c)
#pragma unroll
    for (int v = 1; v < 3; ++v) x[3 * c + v] = cmul(x[3 * c + v], tw_const<INV>(double(v * c) / 9.0));
#pragma unroll
  for (int c = 0; c < 3; ++c) dft3<INV>(x[3 * c + 0], x[3 * c + 1], x[3 * c + 2]);  // x[3c + d] = X[c + 3d]
  cf t[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = x[3 * (k % 3) + k / 3];
#pragma unroll
  for (int k = 0; k < 9; ++k) x[k] = t[k];
}

// DFT-45 as 5 x 9: n = 5p + q, k = r + 9s; natural order in and out.
template <bool INV>
__device__ __forceinline__ void dft45(cf (&x)[45]) {
  cf a[5][9];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    cf col[9];
#pragma unroll
    for (int p = 0; p < 9; ++p) col[p] = x[5 * p + q];
    dft9<INV>(col);
#pragma unroll
    for (int r = 0; r < 9; ++r) a[q][r] = (q && r) ? cmul(col[r], tw_const<INV>(double(q * r) / 45.0)) : col[r];
  }
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    cf v[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) v[q] = a[q][r];
    dft5<INV>(v);
#pragma unroll
    for (int s = 0; s < 5; ++s) x[r + 9 * s] = v[s];
  }
}

template <bool INV>
__device__ __forceinline__ void fft4v(cf& a0, cf& a1, cf& a2, cf& a3) {
  const cf t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3;
  const cf d = a1 - a3;
  const cf t3 = INV ? cf{-d.y, d.x} : cf{d.y, -d.x};  // (+-i) d
  a0 = t0 + t2;
  a2 = t0 - t2;
  a1 = t1 + t3;
  a3 = t1 - t3;
}

template <bool INV>
__device__ __forceinline__ void fft16v(cf (&v)[16]) {
#pragma unroll
  for (int m2 = 0; m2 < 4; ++m2) fft4v<INV>(v[m2], v[4 + m2], v[8 + m2], v[12 + m2]);
#pragma unroll
  for (int l1 = 1; l1 < 4; ++l1)
#pragma unroll
    for (int m2 = 1; m2 < 4; ++m2) v[4 * l1 + m2] = cmul(v[4 * l1 + m2], tw_const<INV>(double(m2 * l1) / 16.0));
#pragma unroll
  for (int l1 = 0; l1 < 4; ++l1) fft4v<INV>(v[4 * l1 + 0], v[4 * l1 + 1], v[4 * l1 + 2], v[4 * l1 + 3]);
  cf t[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) t[k] = v[4 * (k & 3) + (k >> 2)];
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = t[k];
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// wave sum through DPP (no lane-index VGPRs, unlike __shfl_xor's bpermute
// addresses, which the compiler hoists and spills): quad_perm [1,0,3,2],
// [2,3,0,1], row_half_mirror, row_mirror leave each 16-lane row's sum in all
// of its lanes; the four rows are added from readlane
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  const int b = __builtin_bit_cast(int, v);
  return (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)) +
          __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16))) +
         (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)) +
          __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48)));
}

// (results and the wave index are uniform: SGPRs, so nothing here takes a
// VGPR that could be spilled and reloaded behind the next clip's prefetch)
__device__ __forceinline__ float sgpr_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < kThreads / 64; ++w) s += red[w];
  return sgpr_f(s);  // summed here, not sunk to the use with 16 live partials
}

// opaque copy of the thread id: index math derived from it stays inside the
// clip loop (the compiler otherwise hoists dozens of per-element offsets out of
// it and spills them)
__device__ __forceinline__ int opaque_tid() {
  int t;
  asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(static_cast<int>(threadIdx.x)));
  return t;
}

// Optional source view of a kernel's input clips (placement on first touch):
// clip i with pre[i] >= 0 has not been placed yet and is read from its source
// row src[i] (len[i] valid samples) through load_placed; pre[i] < 0 (or pre
// NULL): the row is placed, the kernel reads its x as without a view.
struct SrcView {
  const float* src;
  int64_t stride;
  const int32_t* len;
  const int32_t* pre;
};

// the entry points' view arguments: all NULL / 0 (no view) or all given
inline int src_view(const float* src, int64_t stride, const int32_t* len, const int32_t* pre, SrcView& v) {
  v = SrcView{nullptr, 0, nullptr, nullptr};
  if (!src && !len && !pre) return HBK_OK;
  if (!src || !len || !pre) return arg_error("source view needs src, src_len and src_pre");
  if (stride < 0) return arg_error("negative src_stride");
  v = SrcView{src, stride, len, pre};
  return HBK_OK;
}

// Sample t of a clip placed on first touch (place_kernel's load, shared with the
// kernels that read a source row through its placement instead of the placed
// row): row[t - pre] for pre <= t < pre + n, else 0, where n = min(len, T). The
// load is unconditional (its index clamped into the row, the value selected
// after), so a thread's loads are in flight together. row[0] must be readable
// even when n <= 0 (the caller passes any valid row then; every sample is 0).
// 32-bit byte offset from a uniform base: global_load's saddr form.
// (In two halves for a kernel that loads a clip ahead and consumes it later: the select
// then sits at the use, not behind the load.)
__device__ __forceinline__ uint32_t placed_index(int pre, int n, int t) {
  return static_cast<uint32_t>(min(max(t - pre, 0), max(n - 1, 0)));
}
__device__ __forceinline__ float placed_select(float v, int pre, int n, int t) {
  const int u = t - pre;
  return (u >= 0 && u < n) ? v : 0.f;
}
__device__ __forceinline__ float load_placed(const float* row, int pre, int n, int t) {
  const float v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row) + (placed_index(pre, n, t) << 2));
  return placed_select(v, pre, n, t);
}

// A wave's 64 consecutive samples w0 .. w0 + 63 (w0 uniform, a multiple of 64) of such a
// clip lie inside the source clip (1), outside it (0) or across one of its ends (2). The
// class is uniform and depends on (pre, n, w0) alone, so a branch on it waits on no load;
// a wave inside the clip has nothing to select (the tanh and augment kernels are bound by
// their VALU work: a select on every sample showed in their times).
__device__ __forceinline__ int placed_class(int pre, int n, int w0) {
  const int rel = w0 - pre;
  return (rel >= 0 && rel + 63 < n) ? 1 : ((rel + 63 < 0 || rel >= n) ? 0 : 2);
}
// sample w0 + lane of the clip: load_placed's value (the same load where one is needed)
__device__ __forceinline__ float load_placed_wave(const float* row, int pre, int n, int w0, int lane) {
  // (a wave outside the clip loads nothing; the other two classes share one load
  // instruction: a second one behind a branch made the compiler wait for every load in
  // flight before it)
  const int cls = placed_class(pre, n, w0);
  if (cls == 0) return 0.f;
  const uint32_t i = cls == 1 ? static_cast<uint32_t>(w0 - pre + lane) : placed_index(pre, n, w0 + lane);
  const float v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row) + (i << 2));
  return cls == 1 ? v : placed_select(v, pre, n, w0 + lane);
}

// two block sums in one barrier round (red holds 2 x 16 wave partials)
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  __syncthreads();
  if (lane == 0) {
    red[wave] = a;
    red[16 + wave] = b;
  }
  __syncthreads();
  a = b = 0.f;
  for (int w = 0; w < kThreads / 64; ++w) {
    a += red[w];
    b += red[16 + w];
  }
  a = sgpr_f(a);
  b = sgpr_f(b);
}

// a clip copied through registers: all loads issued before the first store
// (a load -> store loop waits out one memory latency per element, since x and
// out may alias)
// (groups of 8 slots: few live VGPRs in the 64-VGPR tanh kernel)
__device__ __forceinline__ void copy_clip(const float* x, float* out, int tid) {
  constexpr int kPer = (kT + kThreads - 1) / kThreads, kG = 8;
#pragma unroll 1
  for (int u0 = 0; u0 < kPer; u0 += kG) {
    float v[kG];
#pragma unroll
    for (int u = 0; u < kG; ++u) {
      const int s = tid + (u0 + u) * kThreads;
      v[u] = s < kT ? *reinterpret_cast<const float*>(reinterpret_cast<const char*>(x) + (static_cast<uint32_t>(s) << 2))
                    : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kG; ++u) {
      const int s = tid + (u0 + u) * kThreads;
      if (s < kT) *reinterpret_cast<float*>(reinterpret_cast<char*>(out) + (static_cast<uint32_t>(s) << 2)) = v[u];
    }
  }
}

}  // namespace
}  // namespace hbk
