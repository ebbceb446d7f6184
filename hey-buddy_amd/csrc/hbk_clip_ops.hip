// The per-clip operations of the augmentation chain that need no transform:
// tanh distortion, clip placement and the seven-band parametric EQ, with their
// entry points (hbk_tanh_distortion, hbk_place_clips, hbk_seven_band_eq).
#include <algorithm>

#include "hbk_aug_dev.h"

namespace hbk {
namespace {

// ---- tanh distortion ------------------------------------------------------
// audiomentations TanhDistortion (the reference's per-clip Compose,
// augmented.py:79-90; p 0.25, distortion ~ U[1e-4, 0.1], constants.py:122-124):
//   q = 100 - 99 amount; th = percentile(|x|, q) (numpy's linear interpolation);
//   y = tanh(0.5 / (th + 1e-6) x); if rms(x) > 1e-9: y *= rms(x) / rms(y).
// One workgroup per clip, the clip in registers. The two order statistics of
// |x| around the percentile come from an LDS radix select over the f32 bit
// patterns (non-negative floats order like their bits): four 8-bit histogram
// passes for rank lo, then its successor from one count + min reduction.
struct TanhArgs {
  const float* x;
  int64_t x_stride;
  float* out;
  int64_t out_stride;
  int64_t n_clips;
  const float* amount;  // per clip; NaN = clip unchanged
  const int32_t* idx;   // NULL: every clip; else the n_entries listed clip rows (balanced launch)
  int64_t n_entries;
  SrcView view;         // pre NULL: none (a clip read through it has a non-NaN amount)
};

// |x| bits of slot u (u < kPer), or ~0 past the end of the clip (above every value);
// recomputed per pass instead of held (2 blocks / CU need <= 64 VGPRs)
__device__ __forceinline__ unsigned abs_bits(float v, int s) {
  return s < kT ? (__builtin_bit_cast(unsigned, v) & 0x7FFFFFFFu) : 0xFFFFFFFFu;
}

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8)))
tanh_distortion_kernel(TanhArgs a) {
  // radix-select digits over |x|'s bits 30..0 (bit 31 is 0): 12 + 10 + 9 bits. The first
  // digit spans the exponent and 4 mantissa bits, so a clip's values spread over ~200 bins
  // instead of crowding the ~9 of an 8-bit top digit (LDS atomics to one address serialise)
  __shared__ unsigned hist[4096];
  __shared__ float red[32];
  __shared__ unsigned pick[2];  // selected digit, rank left within it
  constexpr int kPer = (kT + kThreads - 1) / kThreads;
  const int64_t n_iter = a.idx ? a.n_entries : a.n_clips;
  for (int64_t e = blockIdx.x; e < n_iter; e += gridDim.x) {
    const int64_t clip = a.idx ? a.idx[e] : e;
    const int tid = opaque_tid();
    const float* x = a.x + clip * a.x_stride;
    float* out = a.out + clip * a.out_stride;
    const float amt = a.amount[clip];
    if (amt != amt) {
      if (out != x) copy_clip(x, out, tid);
      continue;
    }
    // uniform base + 32-bit byte offsets (global_load's saddr form): one VGPR per
    // address instead of a hoisted 64-bit pointer per slot
    float xr[kPer];
    // (pre: uniform, read with amt before any load; a clip placed on first touch comes from
    // its source row, the others from x as before)
    // (len: loaded with pre, not behind the branch on it: one latency)
    const int pre = a.view.pre ? a.view.pre[clip] : -1, len = a.view.pre ? a.view.len[clip] : 0;
    if (pre >= 0) {
      const int n = min(len, kT);
      const float* row = n > 0 ? a.view.src + clip * a.view.stride : x;
      const int t = opaque_tid();
      const int w0 = __builtin_amdgcn_readfirstlane(t & ~63);
#pragma unroll
      for (int u = 0; u < kPer; ++u) xr[u] = load_placed_wave(row, pre, n, w0 + u * kThreads, t & 63);
    } else {
    const int t = opaque_tid();
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int s = t + u * kThreads;
      xr[u] = s < kT ? *reinterpret_cast<const float*>(reinterpret_cast<const char*>(x) + (static_cast<uint32_t>(s) << 2))
                     : 0.f;
    }
    }
    // numpy percentile, method "linear": position q/100 (N - 1)
    const double pos = (100.0 - 99.0 * static_cast<double>(amt)) / 100.0 * (kT - 1);
    const int lo = min(max(static_cast<int>(floor(pos)), 0), kT - 1);
    const double frac = pos - lo;
    unsigned prefix = 0, mask = 0, rank = static_cast<unsigned>(lo);
#pragma unroll 1
    for (int p = 0; p < 3; ++p) {
      const int shift = p == 0 ? 19 : (p == 1 ? 9 : 0), bins = p == 0 ? 4096 : (p == 1 ? 1024 : 512);
      const int per_lane = bins >> 6;  // bins per lane of wave 0's scan
      for (int i = tid; i < bins; i += kThreads) hist[i] = 0;
      __syncthreads();
      const int t = opaque_tid();
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const unsigned b = abs_bits(xr[u], t + u * kThreads);
        if ((b & mask) == prefix && b != 0xFFFFFFFFu) atomicAdd(&hist[(b >> shift) & (bins - 1)], 1u);
      }
      __syncthreads();
      if (tid < 64) {  // wave 0: per_lane bins per lane, inclusive scan over lanes, first lane past rank
        unsigned own = 0;
        for (int i = 0; i < per_lane; ++i) own += hist[per_lane * tid + i];
        unsigned inc = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned v = __shfl_up(inc, d, 64);
          if (tid >= d) inc += v;
        }
        const unsigned long long hit = __ballot(inc > rank);
        const int l = __ffsll(static_cast<long long>(hit)) - 1;
        if (tid == l) {
          unsigned r = rank - (inc - own), dsel = per_lane * l;
          for (int i = 0; i < per_lane - 1; ++i) {
            const unsigned h = hist[dsel];
            if (r < h) break;
            r -= h;
            ++dsel;
          }
          pick[0] = dsel;
          pick[1] = r;
        }
      }
      __syncthreads();
      prefix |= pick[0] << shift;
      mask |= static_cast<unsigned>(bins - 1) << shift;
      rank = pick[1];
    }
    // successor: v_lo again if more than lo + 1 values are <= v_lo, else min{|x| > v_lo}
    float cnt = 0.f, mg = __builtin_inff();
    const int t2 = opaque_tid();
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const unsigned b = abs_bits(xr[u], t2 + u * kThreads);
      if (b == 0xFFFFFFFFu) continue;
      if (b <= prefix) cnt += 1.f;
      else mg = fminf(mg, __builtin_bit_cast(float, b));
    }
    cnt = block_sum(cnt, red);
    {  // block min (wave min through shuffles, then the 16 partials)
      for (int d = 32; d >= 1; d >>= 1) mg = fminf(mg, __shfl_xor(mg, d, 64));
      __syncthreads();
      if ((tid & 63) == 0) red[tid >> 6] = mg;
      __syncthreads();
      mg = red[0];
      for (int w = 1; w < kThreads / 64; ++w) mg = fminf(mg, red[w]);
    }
    const double v_lo = __builtin_bit_cast(float, prefix);
    const double v_hi = (cnt >= lo + 2 || lo + 1 >= kT) ? v_lo : static_cast<double>(mg);
    const double d = v_hi - v_lo;
    const double th = frac >= 0.5 ? v_hi - d * (1.0 - frac) : v_lo + d * frac;  // numpy _lerp
    const float g = static_cast<float>(0.5 / (th + 1e-6));
    float ex = 0.f, ey = 0.f;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      ex += xr[u] * xr[u];
      // tanh(v) = 1 - 2 / (e^(2v) + 1) on the transcendental unit (+-1 at the
      // overflow ends; absolute error ~1e-7, tanhf's polynomial cost ~4x more);
      // past-the-end slots hold 0 -> 0
      xr[u] = 1.f - __fdividef(2.f, __expf(2.f * g * xr[u]) + 1.f);
      ey += xr[u] * xr[u];
    }
    block_sum2(ex, ey, red);
    const float rms_x = sqrtf(ex / kT);
    const float post = rms_x > 1e-9f ? rms_x / sqrtf(ey / kT) : 1.f;
    const int t3 = opaque_tid();
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int s = t3 + u * kThreads;
      if (s < kT) *reinterpret_cast<float*>(reinterpret_cast<char*>(out) + (static_cast<uint32_t>(s) << 2)) = xr[u] * post;
    }
    __syncthreads();  // red / hist reuse by the next clip
  }
}

// Clip placement (AugmentedAudioGenerator.to_target_length, augmented.py:200-232):
// out[i, t] = src[i, t - pre[i]] for pre[i] <= t < pre[i] + min(len[i], T), else 0.
// One 256-thread block per (clip, 4096-sample span): every thread writes one
// float4 of out (T % 4 == 0); the shifted source is read with scalar loads
// (pre[i] is arbitrary, so the 4 samples are not 16-B aligned in src).
constexpr int kPlaceSpan = 4096;
__global__ void __launch_bounds__(256) place_kernel(const float* __restrict__ src, int64_t src_stride,
                                                    const int32_t* __restrict__ src_len,
                                                    const int32_t* __restrict__ pre,
                                                    const int32_t* __restrict__ idx, float* __restrict__ out,
                                                    int64_t out_stride, int64_t n_clips, int T) {
  // workgroup b takes (clip, span) item b (one 4,096-sample span of one clip; a 1-D grid, so
  // no 65,535-clip launch limit); every load is unconditional (clamped into the clip, zeroed by
  // a select), so a thread's 16 loads are in flight together instead of each behind its own
  // branch
  // (idx: the clip rows to place, n_clips of them; NULL: rows 0 .. n_clips - 1. The other
  // rows of out are placed by their first consumer, which loads what is loaded here:
  // load_placed, hbk_aug_dev.h.)
  const int spans = (T + kPlaceSpan - 1) / kPlaceSpan;
  const int64_t items = n_clips * spans;
  constexpr int kR = kPlaceSpan / 1024;
  // (measured: the same 3.1 ms per 100 k clips, 4.85 TB/s, as the round-4 2-D grid with
  // predicated loads, tools/probe_place.py: the kernel is bound by HBM's write rate)
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {  // (one pass: grid = items)
    const int64_t e = it / spans;
    const int sp = static_cast<int>(it - e * spans);
    const int64_t clip = idx ? idx[e] : e;
    const int p = pre[clip];
    const int n = min(src_len[clip], T);
    const int last = max(n - 1, 0);
    const float* s = src + clip * src_stride;
    float* o = out + clip * out_stride;
    const int t0 = sp * kPlaceSpan + 4 * static_cast<int>(threadIdx.x);
    float v[kR][4];
#pragma unroll
    for (int r = 0; r < kR; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int u = t0 + r * 1024 + q - p;
        const float x = n > 0 ? s[min(max(u, 0), last)] : 0.f;  // (n: uniform per item)
        v[r][q] = (u >= 0 && u < n) ? x : 0.f;
      }
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const int t = t0 + r * 1024;
      if (t < T) *reinterpret_cast<float4*>(o + t) = make_float4(v[r][0], v[r][1], v[r][2], v[r][3]);
    }
  }
}

// ---------------------------------------------------------------------------
// Seven-band parametric EQ: audiomentations SevenBandParametricEQ, the
// reference's per-clip transform ahead of tanh (dataset/augmented.py:79-84):
// seven RBJ biquads in series (low shelf, five peaks, high shelf), each the
// direct form II transposed recursion of scipy sosfilt in float64 with its
// output rounded to float32 before the next stage (audiomentations casts each
// filter's output). One lane per clip: the recursion is sequential in time,
// and clips are the parallel axis. A wave owns 64 clips; 64-sample tiles are
// loaded coalesced (16 lanes per clip row, float4), transposed through LDS to
// [sample][clip] (conflict-free column reads), filtered in place and stored
// back the same way; the next tile's loads are issued before the current one
// is filtered. A clip whose first b0 is NaN is copied.
constexpr int kEqTile = 64;
struct EqArgs {
  const float* x;
  int64_t x_stride;
  const double* coef;  // [n][7][5]: b0, b1, b2, a1, a2 (a0 = 1)
  const int32_t* idx;  // clip of entry j (NULL: j)
  float* out;
  int64_t out_stride;
  int64_t n;
  SrcView view;  // pre NULL: none
};

// Systolic over the cascade: a wave filters 8 clips, 8 lanes per clip; lane
// s < 7 holds section s's coefficients and state and, at step t, filters sample
// t - s: its input is section s - 1's output of step t - 1 (DPP row_shr:1),
// section 0 reads x[t] from the LDS tile, section 6's output is y[t - 6]. Each
// section runs the same float64 recursion, in the same order, as a one-lane
// cascade (float32 between sections), so the result is bitwise that of the
// sequential filter; eight times as many waves fill the chip (the filter is
// sequential in time, so one lane per clip left most SIMDs idle). A clip whose
// coefficients are NaN passes through an identity cascade (a copy). A clip
// placed on first touch (a.view) loads its tile samples from the source row
// with scalar loads instead of the two aligned float4 (the same values:
// load_tile below).
constexpr int kEqClips = 8;  // clips per wave
__global__ void __launch_bounds__(64) eq_kernel(EqArgs a) {
  constexpr int kRow = kEqTile + 4;  // 16-B aligned rows (b128 reads / writes of 8 steps)
  __shared__ __attribute__((aligned(16))) float tin[kEqClips][kRow];
  __shared__ __attribute__((aligned(16))) float tout[kEqClips][kRow];
  const int lane = threadIdx.x, c = lane >> 3, sec = lane & 7;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kEqClips;
  const int64_t jc = min(j0 + c, a.n - 1);
  const double* cf0 = a.coef + jc * 35;
  const bool copy = cf0[0] != cf0[0];
  const int k = min(sec, 6);
  double b0 = cf0[5 * k], b1 = cf0[5 * k + 1], b2 = cf0[5 * k + 2], a1 = cf0[5 * k + 3], a2 = cf0[5 * k + 4];
  if (copy) b0 = 1.0, b1 = b2 = a1 = a2 = 0.0;
  double s1 = 0.0, s2 = 0.0;
  // tile I/O mapping: lane -> clip lc = lane >> 3, float4 column lq = lane & 7 (samples 4 lq, 32 + 4 lq)
  const int lc = lane >> 3, lq = lane & 7;
  const int64_t jl = min(j0 + lc, a.n - 1);
  const int64_t clip_l = a.idx ? static_cast<int64_t>(a.idx[jl]) : jl;
  const float* xl = a.x + clip_l * a.x_stride;
  float* ol = a.out + clip_l * a.out_stride;
  const bool store_l = j0 + lc < a.n;
  // (pre_l / n_l are read once, here: no tile load waits on them)
  const int pre_l = a.view.pre ? a.view.pre[clip_l] : -1, len_l = a.view.pre ? a.view.len[clip_l] : 0;
  const int n_l = pre_l >= 0 ? min(len_l, kT) : 0;
  const float* sl = n_l > 0 ? a.view.src + clip_l * a.view.stride : xl;
  float4 p0, p1;
  auto load_tile = [&](int t) {  // samples t + 4 lq .. + 3 and t + 32 + 4 lq .. + 3 of the lane's clip
    // (the branches depend on pre_l / n_l / t alone; a lane's eight samples lie inside the
    // source clip, outside it, or across one of its ends: the last case alone pays for the
    // clamps and selects, which this kernel, bound by its VALU work, would feel on every tile)
    const int u0 = t + 4 * lq - pre_l;
    if (pre_l >= 0 && u0 >= 0 && u0 + 35 < n_l) {
      const float* q = sl + u0;
      p0 = float4{q[0], q[1], q[2], q[3]};
      p1 = float4{q[32], q[33], q[34], q[35]};
    } else if (pre_l >= 0 && (u0 + 35 < 0 || u0 >= n_l)) {
      p0 = p1 = float4{0.f, 0.f, 0.f, 0.f};
    } else if (pre_l >= 0) {
      const int ta = t + 4 * lq, tb = ta + 32;
      p0 = float4{load_placed(sl, pre_l, n_l, ta), load_placed(sl, pre_l, n_l, ta + 1),
                  load_placed(sl, pre_l, n_l, ta + 2), load_placed(sl, pre_l, n_l, ta + 3)};
      p1 = float4{load_placed(sl, pre_l, n_l, tb), load_placed(sl, pre_l, n_l, tb + 1),
                  load_placed(sl, pre_l, n_l, tb + 2), load_placed(sl, pre_l, n_l, tb + 3)};
    } else {
      p0 = *reinterpret_cast<const float4*>(xl + t + 4 * lq);
      p1 = *reinterpret_cast<const float4*>(xl + t + 32 + 4 * lq);
    }
  };
  load_tile(0);
  float prev = 0.f;
  for (int t0 = 0; t0 <= kT; t0 += kEqTile) {  // the last tile only drains the pipeline
    tin[lc][4 * lq] = p0.x;
    tin[lc][4 * lq + 1] = p0.y;
    tin[lc][4 * lq + 2] = p0.z;
    tin[lc][4 * lq + 3] = p0.w;
    tin[lc][32 + 4 * lq] = p1.x;
    tin[lc][32 + 4 * lq + 1] = p1.y;
    tin[lc][32 + 4 * lq + 2] = p1.z;
    tin[lc][32 + 4 * lq + 3] = p1.w;
    __syncthreads();
    const int tn = min(t0 + kEqTile, kT - kEqTile);  // next tile (clamped: the drain re-reads the last)
    load_tile(tn);
    // 8 steps per group: their section-0 inputs read ahead (two b128 reads, one
    // wait), section 6's outputs written after (branch-free steps in between)
    for (int st0 = 0; st0 < kEqTile; st0 += 8) {
      const float4 ia = *reinterpret_cast<const float4*>(&tin[c][st0]);
      const float4 ib = *reinterpret_cast<const float4*>(&tin[c][st0 + 4]);
      const float in8[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
      float o8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float u = sec == 0 ? in8[q] : prev;
        const double vd = u;
        const double y = fma(b0, vd, s1);
        s1 = fma(b1, vd, fma(-a1, y, s2));
        s2 = fma(b2, vd, -a2 * y);
        const float v = static_cast<float>(y);
        o8[q] = v;  // section 6: sample t0 + st0 + q - 6
        prev = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, prev),
                                                                     __builtin_bit_cast(int, v), 0x111, 0xF, 0xF,
                                                                     false));
      }
      if (sec == 6) {
        *reinterpret_cast<float4*>(&tout[c][st0]) = float4{o8[0], o8[1], o8[2], o8[3]};
        *reinterpret_cast<float4*>(&tout[c][st0 + 4]) = float4{o8[4], o8[5], o8[6], o8[7]};
      }
    }
    __syncthreads();
    if (store_l) {
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int kk = lq + 8 * m;
        const int n = t0 - 6 + kk;
        if (n >= 0 && n < kT) ol[n] = tout[lc][kk];
      }
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace hbk

extern "C" {

int hbk_place_clips_idx(const float* src, int64_t n_clips, int64_t src_stride, const int32_t* src_len,
                        const int32_t* pre, const int32_t* idx, int64_t n_entries, float* out, int64_t out_stride,
                        int64_t T, void* stream) {
  using namespace hbk;
  if (n_clips < 0 || (idx && n_entries < 0)) return arg_error("negative count");
  const int64_t n_rows = idx ? n_entries : n_clips;  // rows placed: the listed ones, or all
  if (n_rows == 0) return HBK_OK;
  if (!src || !src_len || !pre || !out) return arg_error("NULL pointer");
  if (T <= 0 || T % 4 || T > (int64_t(1) << 30)) return arg_error("T must be a positive multiple of 4");
  if (out_stride < T || out_stride % 4 || (reinterpret_cast<uintptr_t>(out) & 15))
    return arg_error("out rows must be 16-B aligned with stride >= T");
  const int64_t items = n_rows * ((T + kPlaceSpan - 1) / kPlaceSpan);
  if (items >= (int64_t(1) << 31)) return arg_error("too many clips for one launch");
  const int64_t blocks = items;
  hipLaunchKernelGGL(place_kernel, dim3(unsigned(blocks)), dim3(256), 0, as_stream(stream), src, src_stride, src_len,
                     pre, idx, out, out_stride, n_rows, int(T));
  HBK_LAUNCH_CHECK("place_kernel");
  return HBK_OK;
}

int hbk_place_clips(const float* src, int64_t n_clips, int64_t src_stride, const int32_t* src_len,
                    const int32_t* pre, float* out, int64_t out_stride, int64_t T, void* stream) {
  return hbk_place_clips_idx(src, n_clips, src_stride, src_len, pre, nullptr, 0, out, out_stride, T, stream);
}

int hbk_tanh_distortion_src(const float* x, int64_t n_clips, int64_t x_stride, const float* amount,
                            const int32_t* idx, int64_t n_entries, float* out, int64_t out_stride,
                            const float* src, int64_t src_stride, const int32_t* src_len, const int32_t* src_pre,
                            void* stream) {
  using namespace hbk;
  if (n_clips < 0) return arg_error("negative n_clips");
  if (n_clips == 0) return HBK_OK;
  if (!x || !out || !amount) return arg_error("NULL pointer");
  if (x_stride < kT || out_stride < kT) return arg_error("stride < 23040");
  TanhArgs a;
  a.x = x;
  a.x_stride = x_stride;
  a.out = out;
  a.out_stride = out_stride;
  a.n_clips = n_clips;
  a.amount = amount;
  a.idx = idx;
  a.n_entries = idx ? n_entries : n_clips;
  const int st = src_view(src, src_stride, src_len, src_pre, a.view);
  if (st != HBK_OK) return st;
  if (a.n_entries <= 0) return n_entries < 0 ? arg_error("negative n_entries") : HBK_OK;
  const int64_t blocks = std::min<int64_t>(a.n_entries, persistent_blocks(2, stream));
  hipLaunchKernelGGL(tanh_distortion_kernel, dim3(unsigned(blocks)), dim3(kThreads), 0, as_stream(stream), a);
  HBK_LAUNCH_CHECK("tanh_distortion_kernel");
  return HBK_OK;
}

int hbk_tanh_distortion(const float* x, int64_t n_clips, int64_t x_stride, const float* amount,
                        const int32_t* idx, int64_t n_entries, float* out, int64_t out_stride, void* stream) {
  return hbk_tanh_distortion_src(x, n_clips, x_stride, amount, idx, n_entries, out, out_stride, nullptr, 0, nullptr,
                                 nullptr, stream);
}

int hbk_seven_band_eq_src(const float* x, int64_t n_clips, int64_t x_stride, const double* coef, const int32_t* idx,
                          int64_t n_entries, float* out, int64_t out_stride, const float* src, int64_t src_stride,
                          const int32_t* src_len, const int32_t* src_pre, void* stream) {
  using namespace hbk;
  if (n_clips < 0 || n_entries < 0) return arg_error("negative count");
  if (!idx) n_entries = n_clips;
  if (n_entries == 0) return HBK_OK;
  if (!x || !out || !coef) return arg_error("NULL pointer");
  if (x_stride < kT || out_stride < kT) return arg_error("stride < 23040");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) % 16 || x_stride % 4 || out_stride % 4)
    return arg_error("x / out rows must be 16-B aligned");
  EqArgs a;
  a.x = x;
  a.x_stride = x_stride;
  a.coef = coef;
  a.idx = idx;
  a.out = out;
  a.out_stride = out_stride;
  a.n = n_entries;
  const int st = src_view(src, src_stride, src_len, src_pre, a.view);
  if (st != HBK_OK) return st;
  hipLaunchKernelGGL(eq_kernel, dim3(unsigned((n_entries + kEqClips - 1) / kEqClips)), dim3(64), 0,
                     as_stream(stream), a);
  HBK_LAUNCH_CHECK("eq_kernel");
  return HBK_OK;
}

int hbk_seven_band_eq(const float* x, int64_t n_clips, int64_t x_stride, const double* coef, const int32_t* idx,
                      int64_t n_entries, float* out, int64_t out_stride, void* stream) {
  return hbk_seven_band_eq_src(x, n_clips, x_stride, coef, idx, n_entries, out, out_stride, nullptr, 0, nullptr,
                               nullptr, stream);
}

}  // extern "C"
