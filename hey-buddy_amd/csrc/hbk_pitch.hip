// Pitch shift for gfx950: the span pairing, the phase vocoder and the two
// resamplers, with hbk_pitch_shift and hbk_pitch_shift_workspace_size. The
// geometry, the workspace layout and the launch grids come from
// hbk_augment_plan.h (host only, checked on the CPU).
#include <atomic>
#include <cstdlib>

#include "hbk_augment_plan.h"
#include "hbk_common.h"

namespace hbk {
namespace {

// ----------------------------------------------------------------------------
// PitchShift (torch_audiomentations PitchShift -> torch_pitch_shift.pitch_shift,
// augmented.py:93-100): stft (n_fft 250, hop 7, rectangular window, center,
// reflect) -> phase vocoder (torchaudio TimeStretch, rate = 1 / shift) ->
// istft -> sinc resample (torchaudio Resample(sr, int(sr / shift))), cropped or
// zero-padded to the clip length. One ratio per call (per_batch mode).
//
// ps_vocoder_kernel: ONE pass per clip, 128 lanes = 126 bins, sequential over
// the clip's frames (kPvClips clips per workgroup in lockstep: every clip of a
// call has the same frame geometry). No spectrogram is stored, no segment is
// recomputed:
//  * analysis: a sliding DFT (hop 7: X_f = w^-7 (X_{f-1} + sum_j d_j w^j),
//    d_j = xp[7f+243+j] - xp[7f-7+j], w = e^{-2 pi i k/250}) whose state X is
//    float64 and whose increment sum_j d_j w^j is float32 (packed FMAs); a
//    direct float64 DFT restarts it every kPvRestart frames. A frame whose 250
//    samples are all zero is exactly 0 (angle 0) as in the FFT (a running
//    count of non-zero samples);
//  * vocoder without angles: the accumulated phase e^{i phi_t} is kept as a unit
//    complex P_t = u_0 prod (u_{i0+1} conj u_{i0}) of the frames' unit vectors
//    u = X / |X| (u = 1 for X = 0, angle 0 as in torch), since
//    e^{i (angle(X1) - angle(X0))} = u_1 conj u_0 whatever 2 pi wrap the
//    reference applies. The product telescopes while the source frame steps by
//    one: P_t = R u_{i0(t)} with R constant, changed only by a repeated source
//    frame (R *= u_{i0+1} conj u_{i0}) or a double step. The phase advance
//    2 pi 7k/250 cancels against the istft's frame rotation, so
//    Z_t = Y_t e^{-2 pi i 7kt/250} = m_t P_t e^{-2 pi i qz_t/250} with
//    qz_t = 7kt mod 250 an exact integer counter (no atan2, no sin / cos; R is
//    renormalised once per frame group);
//  * synthesis without inverse transforms: with Q_t = sum_{t' <= t} Z_t' (a
//    prefix per bin) and G(t, s) = Re sum_k c_k e^{2 pi i k (7t + s)/250} Q_t[k],
//    s < 7, the overlap-added istft sample p = 7t + r is
//      (G(t, r) - G(t - 36, r + 2)) / (250 env)   r <= 4 (frames t-35 .. t)
//      (G(t, r) - G(t - 35, r - 5)) / (250 env)   r = 5, 6 (frames t-34 .. t)
//    so a bin keeps no window of past frames. The 7 G(t, .) of a frame are
//    reduced over the bins in registers: lane k forms its 7 products
//    Re(Q_t e^{2 pi i 7kt/250} c_k e^{2 pi i ks/250}) and an 8-lane
//    reduce-scatter by DPP leaves s = g(lane & 7) on each lane; after the
//    group's 8 frames a reduce-scatter over the octets (DPP row_ror:8,
//    v_permlane16/32_swap) leaves frame u of the wave's 64 bins on octet u. No
//    LDS in the per-frame path; per kPvGroup frames one float per lane goes to
//    LDS for the istft samples.
//  * only the non-silent span: a clip placed into the window is mostly exact zeros, and a frame of 250
//    zeros is 0 up to the overlap-added sample. The workgroup scans its rows once for the first / last
//    non-zero sample and runs the groups from the first whose source frames can be non-zero to 36
//    frames past the last (HBK_PS_SPAN=0: every frame); the resamplers read zeros outside the clip's
//    own range of y samples (PitchArgs::yr), and a workgroup wholly outside it only stores zeros.
// ps_resample_kernel (frame group, clip): polyphase sinc, taps in registers.
// (The frame, vocoder and resampler geometry, kPs* / kPv* / kRs*: hbk_augment_plan.h.)
static_assert(kPsTapMax == HBK_PITCH_SHIFT_MAX_TAPS, "the resampler's tap rows");
static_assert(kPlanOk == HBK_OK && kPlanErrArg == HBK_ERR_ARG && kPlanErrUnsupported == HBK_ERR_UNSUPPORTED,
              "the planner's status values");
#ifndef HBK_PV_ABLATE
#define HBK_PV_ABLATE 0  // profiling builds: 1 skips the bin reduction, 2 the per-bin vocoder
#endif
#ifndef HBK_PV_F32STATE
#define HBK_PV_F32STATE 0  // 1: the sliding DFT's state in float32, restarted every 128 frames (variant pv32)
#endif
#ifndef HBK_PV_RESTART
#if HBK_PV_F32STATE
#define HBK_PV_RESTART 128
#else
#define HBK_PV_RESTART 1024  // measured L2 vs the float64 oracle: 3.8e-5 at 128, 5.6e-5 at 256, 6.5e-5 at 1024
#endif
#endif
constexpr int kPvRestart = HBK_PV_RESTART;             // sliding-DFT frames between direct DFTs
#if HBK_PV_F32STATE
typedef float pv_t;   // sliding-DFT state
#else
typedef double pv_t;
#endif

struct PitchArgs {
  const float* x;
  int64_t x_stride;
  const int32_t* idx;
  int n;
  float* out;
  int64_t out_stride;
  int L, f_in, f_out, l1, orig, nw, width, target;
  double rate;
  float* y;       // [n][l1]: istft output (resampler input), written over the frames the vocoder ran
  float* taps;    // [nw][kPsTapMax]
  int2* yr;       // [n]: the y samples [x, y) of the clip's own span (all written); y is zero outside, unread
  int span;       // 1: the vocoder runs over the workgroup's non-silent span only (0: every frame)
  // span pairing (NULL: workgroup b takes list positions kPvClips b + cl and scans its rows itself):
  int2* sp;            // [n]: first / last non-zero sample of list position e (x > y: all zero), ps_span_kernel
  uint64_t* key;       // [n] list positions, then [groups]: the sort keys (unique: the index is the low bits)
  int32_t* ord;        // [n]: list positions sorted by (quantised last sample, first sample)
  int32_t* gord;       // [groups]: groups of kPvClips neighbours of ord, most frames first
};

__device__ __forceinline__ int ps_i0(const PitchArgs& a, int t, float& alpha) {
  // torch.arange(0, f_in, rate, dtype=float32): start + step * i in double, cast
  const float ts = static_cast<float>(static_cast<double>(t) * a.rate);
  const float fl = floorf(ts);
  alpha = ts - fl;
  return static_cast<int>(fl);
}

struct PvClip {
  float d[kPvRows][8];        // row f - fb: d_j (j < 7) of frame f, [7] = the non-zero-count change
  float xs[256];              // xp[0, 250) (frame 0's direct DFT)
  float gh[2][kPvGh][8];      // G(t, s) over wave w's 64 bins, row t mod kPvGh (s = 7: unused)
  int cnt0;
  int lo, hi;                 // first / last non-zero sample of the clip (lo > hi: all zero)
};
struct PvShared {
  cf tw[256];                 // e^{+2 pi i q / 250}
  double tw64[256][2];        // e^{-2 pi i q / 250}, float64
  float4 wt[3][128];          // w^j, w^{j+1} (j = 1, 3, 5) of bin lane, lane-major (one ds_read_b128 per wave)
  PvClip c[kPvClips];
};

// the s of register r on lane b (b = lane & 7) is r ^ pv_g(b): with partners
// b ^ 1, b ^ 2, b ^ 7 (DPP quad_perm / row_half_mirror) each reduce-scatter step
// pairs equal s (pv_g(1) = 1, pv_g(2) = 2, pv_g(7) = 4), and lane b ends with s = pv_g(b)
__device__ __forceinline__ int pv_g(int b) { return (b & 3) ^ ((b & 4) ? 7 : 0); }

template <int kCtrl>
__device__ __forceinline__ float pv_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), kCtrl, 0xF, 0xF, true));
}

// reduce-scatter of (x, y) across lane ^ 16 (kSwap16) or lane ^ 32: lanes with
// that bit clear get x + x', the others y + y'. (inline asm: the compiler's
// builtin for the swap returns one register for both results in this
// toolchain; s_nop covers the VALU-write -> permlane hazard)
template <bool kSwap16>
__device__ __forceinline__ float pv_swap_add(float x, float y) {
  if (kSwap16)
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
  else
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
  return x + y;
}

// Complex products as two packed instructions with the operand swaps and the sign in the
// VOP3P op_sel / neg modifiers (the compiler materialises a negated or swapped pair with
// extra moves): a b = (a.x b.x - a.y b.y, a.x b.y + a.y b.x) and a conj(b)
__device__ __forceinline__ cf pv_cmul(cf a, cf b) {
  cf t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));  // (a.x b.x, a.x b.y)
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
  return r;
}
__device__ __forceinline__ cf pv_cmul_conj(cf a, cf b) {
  cf t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));  // (a.x b.x, -a.x b.y)
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
  return r;
}

typedef float pv_v4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const pv_v4 pv_lds_v4;  // an LDS float4 (32-bit address)
__device__ __forceinline__ float4 pv_f4(pv_v4 v) { return float4{v.x, v.y, v.z, v.w}; }

// sum_{j = 1..6} d_j w^j of a slide (d_j in da.yzw, db.xyz; w^j pairs in w12, w34, w56): one packed
// product and five packed FMAs, each d_j broadcast by op_sel (no register copies)
__device__ __forceinline__ cf pv_inc(float4 da, float4 db, float4 w12, float4 w34, float4 w56) {
  const cf dxy = {da.x, da.y}, dzw = {da.z, da.w}, exy = {db.x, db.y}, ez = {db.z, db.w};
  const cf w1 = {w12.x, w12.y}, w2 = {w12.z, w12.w}, w3 = {w34.x, w34.y}, w4 = {w34.z, w34.w};
  const cf w5 = {w56.x, w56.y}, w6 = {w56.z, w56.w};
  cf acc;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(acc) : "v"(dxy), "v"(w1));
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(dzw), "v"(w2));
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(dzw), "v"(w3));
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(exy), "v"(w4));
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(exy), "v"(w5));
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(ez), "v"(w6));
  return acc;
}

// padded sample p of clip row xr (reflect padding by n_fft / 2)
__device__ __forceinline__ float ps_xp(const float* xr, int L, int p) {
  int i = p - kPsPad;
  i = i < 0 ? -i : i;
  i = i >= L ? 2 * (L - 1) - i : i;
  return xr[i];
}

// rows [fb, fb + kPvRows) of every clip of the workgroup (frames >= f_in: zero rows)
__device__ __forceinline__ void pv_load_rows(const PitchArgs& a, PvShared& sh, const float* xr, int cl, int lane,
                                             int fb) {
  for (int q = lane; q < 2 * kPvRows; q += 128) {
    const int row = q >> 1, h = q & 1, f = fb + row;
    float* dr = sh.c[cl].d[row];
    if (f >= a.f_in) {
      for (int j = 4 * h; j < 4 * h + 4; ++j) dr[j] = 0.f;
      continue;
    }
    if (h == 0) {
      for (int j = 0; j < 4; ++j) dr[j] = ps_xp(xr, a.L, 7 * f + 243 + j) - ps_xp(xr, a.L, 7 * f - 7 + j);
    } else {
      int delta = 0;
      for (int j = 0; j < 7; ++j) {
        const float vin = ps_xp(xr, a.L, 7 * f + 243 + j), vout = ps_xp(xr, a.L, 7 * f - 7 + j);
        delta += (vin != 0.f) - (vout != 0.f);
        if (j >= 4) dr[j] = vin - vout;
      }
      dr[7] = __builtin_bit_cast(float, delta);  // the count change as int bits (read by SALU)
    }
  }
}

// first / last sample of the clip row with v != 0.f (the predicate of the frames' non-zero count: NaN is
// non-zero, -0 is zero), merged into the workgroup's span. One read of the row, 8 loads in flight per lane.
__device__ __forceinline__ void pv_scan_span(PvClip& C, const float* xr, int L, int lane) {
  int lo = INT_MAX, hi = -1;
  int done = 0;  // samples covered by the aligned part
  if ((reinterpret_cast<uintptr_t>(xr) & 15) == 0) {
    const float4* x4 = reinterpret_cast<const float4*>(xr);
    const int n4 = L >> 2;
    for (int q0 = 0; q0 < n4; q0 += 128 * 8) {
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int q = q0 + 128 * j + lane;
        v[j] = q < n4 ? x4[q] : float4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int p = 4 * (q0 + 128 * j + lane);
        const bool b0 = v[j].x != 0.f, b1 = v[j].y != 0.f, b2 = v[j].z != 0.f, b3 = v[j].w != 0.f;
        if (b0 || b1 || b2 || b3) {
          lo = min(lo, p + (b0 ? 0 : b1 ? 1 : b2 ? 2 : 3));
          hi = max(hi, p + (b3 ? 3 : b2 ? 2 : b1 ? 1 : 0));
        }
      }
    }
    done = 4 * n4;
  }
  for (int p = done + lane; p < L; p += 128) {
    if (xr[p] != 0.f) {
      lo = min(lo, p);
      hi = max(hi, p);
    }
  }
  if (hi >= 0) {
    atomicMin(&C.lo, lo);
    atomicMax(&C.hi, hi);
  }
}

// the output frames [tb, tl] the vocoder runs for a span of samples [lo, hi] (lo > hi: none), tb a group's
// first frame (ps_vocoder_kernel, "The groups to run", says why these are enough)
__device__ __forceinline__ void pv_frames_of(const PitchArgs& a, int lo, int hi, int& tb, int& tl) {
  const int jmax = (a.l1 + kPsPad - 1) / kPsHop;  // the frame of the last istft sample
  tb = 0;
  tl = jmax;
  float al;
  if (lo > hi) {
    tl = -1;  // silent: no frames, y is zero everywhere
    return;
  }
  if (lo > 2 * kPsPad && a.rate < 2.0) {  // (rate < 2: c steps by at most 2 per frame, c = i0(t) after frame t)
    const int fz = (lo - kPsPad) / kPsHop - 1;  // source frames <= fz are all zero (7 f + 124 < lo)
    int tg = min(static_cast<int>((fz - 2) / a.rate), a.f_out - 1) & ~(kPvGroup - 1);
    while (tg > 0 && ps_i0(a, tg - 1, al) + 2 > fz) tg -= kPvGroup;  // sf = c + 2 <= fz at the group's top
    tb = max(tg, 0);
  }
  if (hi < a.L - 1 - 2 * kPsPad) {
    const int fn = min((hi + kPsPad) / kPsHop, a.f_in - 1);  // the last source frame that can be non-zero
    int t = max(min(a.f_out - 1, static_cast<int>((fn + 1) / a.rate) + 1), 0);
    while (t > 0 && ps_i0(a, t, al) > fn) --t;  // the last output frame with i0 <= fn
    while (t + 1 < a.f_out && ps_i0(a, t + 1, al) <= fn) ++t;
    tl = min(jmax, t + 36);
  }
}

// Span pairing (HBK_PS_PAIR=0: off). A vocoder workgroup runs the union of its clips' spans, and list
// neighbours are unrelated: on the training clips the union is 0.64 of the window against 0.51 for a
// clip's own span. So a call orders its clips before the vocoder, on the stream, with fixed grids and no
// host round trip:
//  1. ps_span_kernel: one wave per list position scans its row for the first / last non-zero sample (the
//     scan the vocoder did; from both ends, so the silence is all it reads) and writes the sort key
//     (1 + last / kPsQuant, first, position): clips that end together and start together are neighbours;
//  2. ps_rank_kernel: position in sorted order = the number of smaller keys (the keys are unique, so the
//     order is total and the same on every run: no atomics), ord[rank] = position;
//  3. ps_group_kernel: each group of kPvClips neighbours of ord gets the key (frames of its union,
//     descending; group) and ps_rank_kernel orders the groups: the longest workgroups start first.
// The vocoder's workgroup b takes group gord[b]; y and yr stay indexed by list position.
constexpr int kPsQuant = 360;  // samples per bucket of the last non-zero sample

__global__ void __launch_bounds__(256) ps_span_kernel(PitchArgs a) {
  const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= a.n) return;  // (wave-uniform)
  const float* xr = a.x + static_cast<int64_t>(a.idx[e]) * a.x_stride;
  constexpr int kChunk = 64 * 8;  // samples per step: 8 loads in flight per lane
  int lo = INT_MAX, hi = -1;
  for (int p0 = 0; p0 < a.L; p0 += kChunk) {  // forward to the first chunk with a non-zero sample
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int p = p0 + 64 * j + lane;
      v[j] = p < a.L ? xr[p] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (v[j] != 0.f) {
        lo = min(lo, p0 + 64 * j + lane);
        hi = max(hi, p0 + 64 * j + lane);
      }
    if (__any(hi >= 0)) break;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  if (hi >= 0) {
    // backward from the end to the first chunk with a non-zero sample (at the latest the chunk of lo)
    for (int p1 = a.L; p1 > hi + 1; p1 -= kChunk) {
      float v[8];
      int h = -1;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int p = p1 - kChunk + 64 * j + lane;
        v[j] = (p > hi && p < a.L) ? xr[max(p, 0)] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (v[j] != 0.f) h = max(h, p1 - kChunk + 64 * j + lane);
      if (__any(h >= 0)) {
        for (int o = 32; o >= 1; o >>= 1) h = max(h, __shfl_xor(h, o, 64));
        hi = h;
        break;
      }
    }
  }
  if (lane == 0) {
    a.sp[e] = int2{lo, hi};
    const uint64_t q = hi < 0 ? 0 : 1 + static_cast<uint64_t>(hi / kPsQuant), f = hi < 0 ? 0 : static_cast<uint64_t>(lo);
    a.key[e] = (q << 40) | (f << 16) | static_cast<uint64_t>(e);  // hi, lo < 2^24, e < 2^16
  }
}

// ord[number of keys below key[i]] = i: 64 keys per workgroup, each of its 16 waves counts over a 16th of
// the keys, 64 at a time: one load, then each lane's key in turn (v_readlane) against every lane's own
__global__ void __launch_bounds__(1024) ps_rank_kernel(const uint64_t* __restrict__ key, int n,
                                                       int32_t* __restrict__ ord) {
  __shared__ int part[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * 64 + lane;
  const uint64_t mine = key[min(i, n - 1)];
  const int per = (n + 15) / 16, j0 = min(w * per, n), j1 = min(j0 + per, n);
  int below = 0;
  for (int jb = j0; jb < j1; jb += 64) {
    const uint64_t kl = jb + lane < j1 ? key[jb + lane] : ~uint64_t(0);  // (past the range: below no key)
#pragma unroll
    for (int q = 0; q < 64; ++q) {
      const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(kl >> 32), q);
      const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(kl), q);
      below += ((static_cast<uint64_t>(hi) << 32) | lo) < mine;
    }
  }
  part[w][lane] = below;
  __syncthreads();
  if (w == 0 && i < n) {
    int r = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) r += part[q][lane];
    ord[r] = i;
  }
}

// the key of each group of kPvClips neighbours of ord: the groups of its union's frames, descending
__global__ void __launch_bounds__(256) ps_group_kernel(PitchArgs a, int groups) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  int lo = INT_MAX, hi = -1;
  for (int c = 0; c < kPvClips; ++c) {
    const int2 s = a.sp[a.ord[min(kPvClips * g + c, a.n - 1)]];
    lo = min(lo, s.x);
    hi = max(hi, s.y);
  }
  int tb, tl;
  pv_frames_of(a, lo, hi, tb, tl);
  const int steps = tl < tb ? 0 : (tl - tb) / kPvGroup + 1;  // < 2^24 / (7 * 8)
  a.key[g] = (static_cast<uint64_t>((1 << 24) - steps) << 16) | static_cast<uint64_t>(g);
}

#ifdef HBK_PHASE_TIMING
// profiling build: wave 0 of each block sums the s_memtime cycles of the
// vocoder's phases locally, adds them to g_pv_phase[i] at the end (read by
// hbk_debug_aug_phase in hbk_augment.hip as its slots 16 + i, through pv_phase_take)
__device__ unsigned long long g_pv_phase[5];
#define HBK_PVT(i)                                    \
  do {                                                 \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    pvt[i] += t_ - pvt_t0;                             \
    pvt_t0 = t_;                                       \
  } while (0)
#else
#define HBK_PVT(i) \
  do {             \
  } while (0)
#endif

#ifndef HBK_PV_UNROLL_TAIL
#define HBK_PV_UNROLL_TAIL 1  // 0: the non-FULL groups' frames in a loop (A/B)
#endif
#ifndef HBK_PV_WAVES
#define HBK_PV_WAVES 4  // waves per SIMD the vocoder is register-limited to
#endif
__global__ void __launch_bounds__(128 * kPvClips) __attribute__((amdgpu_waves_per_eu(HBK_PV_WAVES)))
ps_vocoder_kernel(PitchArgs a) {
#ifdef HBK_PHASE_TIMING
  unsigned long long pvt[5] = {0, 0, 0, 0, 0}, pvt_t0 = __builtin_amdgcn_s_memtime();
#endif
  extern __shared__ __attribute__((aligned(16))) unsigned char pv_smem[];
  PvShared& sh = *reinterpret_cast<PvShared*>(pv_smem);
  const int tid = threadIdx.x, cl = tid >> 7, lane = tid & 127;
  // the workgroup's clips: list positions kPvClips b + cl, or group gord[b] of the span order (a.sp != NULL)
  const int slot = (a.sp ? a.gord[blockIdx.x] : static_cast<int>(blockIdx.x)) * kPvClips + cl;
  const int e = a.sp ? a.ord[min(slot, a.n - 1)] : min(slot, a.n - 1);  // padding slots repeat the last clip
  const bool live = slot < a.n;
  const float* xr = a.x + static_cast<int64_t>(a.idx[e]) * a.x_stride;
  PvClip& C = sh.c[cl];
  // tables
  for (int q = tid; q < 256; q += blockDim.x) {
    double sn, cs;
    sincospi(2.0 * q / kPsFft, &sn, &cs);
    sh.tw[q] = cf{static_cast<float>(cs), static_cast<float>(sn)};
    sh.tw64[q][0] = cs;
    sh.tw64[q][1] = -sn;
  }
  if (lane == 0) C.cnt0 = 0;
  if (lane == 0) {
    const int2 s = a.sp ? a.sp[e] : int2{INT_MAX, -1};  // scanned by ps_span_kernel, or below
    C.lo = s.x;
    C.hi = s.y;
  }
  __syncthreads();
  if (a.span && !a.sp) pv_scan_span(C, xr, a.L, lane);
  int nz = 0;
  for (int q = lane; q < kPsFft; q += 128) {
    const float v = ps_xp(xr, a.L, q);
    C.xs[q] = v;
    nz += v != 0.f;
  }
  if (nz) atomicAdd(&C.cnt0, nz);
  for (int q = tid; q < 3 * 128; q += blockDim.x) {
    const int j = 2 * (q / 128) + 1, kk = min(q % 128, kPsBins - 1), q1 = (kk * j) % kPsFft,
              q2 = (kk * (j + 1)) % kPsFft;
    sh.wt[q / 128][q % 128] = float4{static_cast<float>(sh.tw64[q1][0]), static_cast<float>(sh.tw64[q1][1]),
                                     static_cast<float>(sh.tw64[q2][0]), static_cast<float>(sh.tw64[q2][1])};
  }
  int fb = 1;
  pv_load_rows(a, sh, xr, cl, lane, fb);
  __syncthreads();

  const int k = min(lane, kPsBins - 1);
  // per-bin constants: w^-7 in float64 (w^j, j < 7, read from sh.wt per slide), the synthesis weight
  const int q7 = (7 * k) % kPsFft;
  const pv_t rr = static_cast<pv_t>(sh.tw64[q7][0]), ri = static_cast<pv_t>(-sh.tw64[q7][1]);
  const float ck = lane < kPsBins ? ((lane == 0 || lane == kPsBins - 1) ? 1.f : 2.f) : 0.f;
  // synthesis weights c_k e^{2 pi i k s / 250} of the lane's registers (s = r ^ pv_g(lane & 7); s = 7: 0)
  const int gb = pv_g(lane & 7), w = lane >> 6, ou = (lane >> 3) & 7;
  cf esr[4], esi[4];  // (re, im) of registers 2j, 2j + 1 as pairs (packed products)
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int sr = r ^ gb;
    const cf ev = sr < kPsHop ? ck * sh.tw[(k * sr) % kPsFft] : cf{0.f, 0.f};
    esr[r >> 1][r & 1] = ev.x;
    esi[r >> 1][r & 1] = -ev.y;
  }
  const bool b3 = lane & 8;
  // direct DFT (float64) of the frame staged in C.xs: frame 0, and every
  // kPvRestart frames a restart of the sliding DFT (its float32 increments'
  // rounding then accumulates over at most kPvRestart frames)
  auto direct = [&](double& re, double& im) {
    re = im = 0.0;
    int q = 0;
    for (int n = 0; n < kPsFft; ++n) {
      const double v = static_cast<double>(C.xs[n]);
      re = fma(v, sh.tw64[q][0], re);
      im = fma(v, sh.tw64[q][1], im);
      q += k;
      q -= q >= kPsFft ? kPsFft : 0;
    }
  };
  pv_t xre = pv_t(0), xim = pv_t(0);
  int cnt = __builtin_amdgcn_readfirstlane(C.cnt0);
  if (cnt != 0) {  // (a clip's count is wave-uniform; an all-zero frame is 0 without the 250-term sum)
    double dre, dim;
    direct(dre, dim);
    xre = static_cast<pv_t>(dre);
    xim = static_cast<pv_t>(dim);
  }
  int sf = 0;  // last slid frame
  int anchor = 0;  // frame of the last direct DFT
  static_assert(sizeof(sh.wt[0]) == 128 * sizeof(float4), "wt rows of 128 lanes");
  uint32_t wt_addr = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((const pv_lds_v4*)&sh.wt[0][lane]));
  // the sliding DFT's next frame (sf + 1) from the current state, as a candidate
  // (xre, xim, cnt are committed by the caller): two partial sums per component
  // keep the float64 dependency chain short
  // drow: frame sf + 1's d row (C.d[sf + 1 - fb]; a FULL group passes its rows at constant offsets)
  auto slide_to = [&](pv_t& nre, pv_t& nim, int& ncnt, const float* drow) {
    const int f = sf + 1;
    if (f >= a.f_in) {
      nre = nim = pv_t(0);
      ncnt = cnt;
      return;
    }
    // the increment sum_j d_j w^j in float32 (packed; d_j rounded once to float32): its
    // rounding enters the float64 state as a random walk far below the state's level
    // the (loop-invariant) table reads stay in the loop, out of VGPRs: the lane's LDS address is
    // made opaque in place (no copy, no address arithmetic per frame: ds_read_b128 wt_addr offset:..)
    asm volatile("" : "+v"(wt_addr));
    const pv_lds_v4* wtp = (const pv_lds_v4*)static_cast<uintptr_t>(wt_addr);
    const float4 w12 = pv_f4(wtp[0]), w34 = pv_f4(wtp[128]), w56 = pv_f4(wtp[256]);
    const float4* drv = reinterpret_cast<const float4*>(drow);
    const float4 da = drv[0], db = drv[1];
    cf acc = pv_inc(da, db, w12, w34, w56);
    acc.x += da.x;  // w^0 = 1
    ncnt = cnt + __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, db.w));  // a clip's count: wave-uniform
    const pv_t ar = xre + static_cast<pv_t>(acc.x), ai = xim + static_cast<pv_t>(acc.y);
    nre = ar * rr - ai * ri;
    nim = ar * ri + ai * rr;
    if (ncnt == 0) nre = nim = pv_t(0);
  };
  auto commit = [&](pv_t nre, pv_t nim, int ncnt) {
    xre = nre;
    xim = nim;
    cnt = ncnt;
    ++sf;
  };
  // unit vector and magnitude of a frame's bin (X = 0: u = 1, |X| = 0)
  auto polar_of = [&](pv_t re, pv_t im, cf& u, float& mag) {
    const float fr = static_cast<float>(re), fi = static_cast<float>(im);
    const float n2 = fmaf(fr, fr, fi * fi);
    // no selects: for X = 0, rs = rsq(2^-126) = 2^63 and (0 + 2^-63, 0) rs = (1, 0), n2 rs = 0; elsewhere
    // (|X| > 2^-38) both offsets are below half an ulp, so rs and u are those of X itself
    const float rs = __builtin_amdgcn_rsqf(n2 + 0x1p-126f);  // v_rsq_f32 (1 ulp)
    u = cf{fr + 0x1p-63f, fi} * rs;
    mag = n2 * rs;
  };
  auto polar = [&](cf& u, float& mag) { polar_of(xre, xim, u, mag); };
  // frames c, c + 1 in (ca, cm), (na, nm); frame c + 2 = sf ahead in (pa, pm)
  cf ca, na, pa;
  float cm, nm, pm;
  polar(ca, cm);
  // the non-zero counts of frames c, c + 1 (cnt: frame sf), and the last frame of the last group in which
  // an output frame had a source frame with a non-zero sample (wave-uniform): an istft sample none of whose
  // 36 frames' groups had one is exactly 0, as in the FFT path (else G(t, r) - G(t - 36, r + 2), two
  // roundings of one value, leaves a residue)
  int cntc = cnt, cntn, lastnz = INT_MIN / 2;
  {
    pv_t nre, nim;
    int ncnt;
    slide_to(nre, nim, ncnt, C.d[sf + 1 - fb]);
    commit(nre, nim, ncnt);
    cntn = cnt;
    polar(na, nm);
    slide_to(nre, nim, ncnt, C.d[sf + 1 - fb]);
    commit(nre, nim, ncnt);
    polar(pa, pm);
  }
  int c = 0;
  // The accumulated phase at frame t is e^{i phi_t} = P_t e^{-2 pi i qz_t / 250} with
  // P_t = R u_c (P_0 = u_0: R = 1); R changes only when the source frame repeats or
  // double-steps (the float32 products' rounding is a random walk; |R| is reset to 1
  // once per group), and t * 7k / 250 mod 1 = qz_t / 250 comes from the integer
  // counter qz exactly.
  cf R = {1.f, 0.f};
  cf Q = {0.f, 0.f};
  int qz = 0;
  const int dq = q7;
  // the istft rotation tw[qz] advances by e7 = tw[7k mod 250] per frame: rotated in registers
  // (tz and i tz), re-read from the table once per group (no drift, no scattered LDS read per frame)
  const cf e7 = sh.tw[q7];
  const int jmax = (a.l1 + kPsPad - 1) / kPsHop;  // the frame of the last istft sample
  float* y = a.y + static_cast<int64_t>(e) * a.l1;
  // The groups to run: [t_beg, t_last], over the union of the workgroup's clips' non-silent spans
  // (workgroup-uniform: the loop holds barriers). A frame whose 250 samples are zero has X = 0, so
  //  * before the first non-zero sample every output frame adds Z = 0: at the first group whose source
  //    frames (up to c + 2) can be non-zero the state is exactly X = 0, cnt = 0, u = (1, 0), |X| = 0,
  //    R = (1, 0), Q = 0, G = 0, and the loop starts there with the integer state of the full loop;
  //  * after the last output frame with a non-zero source frame Q is constant, and 36 frames on
  //    G(t, r) - G(t - 36, r + 2) is zero: the loop ends there, and the resampler reads zeros.
  // A span that comes within 250 samples of either end reaches into the reflect padding: no skip there.
  // frames_of: the output frames [tb, tl] of a span of samples [lo, hi] (lo > hi: none), tb a group's first
  auto frames_of = [&](int lo, int hi, int& tb, int& tl) { pv_frames_of(a, lo, hi, tb, tl); };
  int t_beg = 0, t_last = jmax;
  {
    // the clip's own frames give the y range its resampler reads (the rest of y is zero, whatever a
    // partner's longer span made this workgroup compute there)
    int tb = 0, tl = jmax;
    if (a.span) {
      int lo = INT_MAX, hi = -1;
      for (int i = 0; i < kPvClips; ++i) {
        lo = min(lo, sh.c[i].lo);
        hi = max(hi, sh.c[i].hi);
      }
      frames_of(lo, hi, t_beg, t_last);
      frames_of(C.lo, C.hi, tb, tl);
    }
    if (lane == 0 && live)
      a.yr[e] = tl < tb ? int2{0, 0}
                        : int2{max(kPsHop * tb - kPsPad, 0), min(kPsHop * (tl + 1) - kPsPad, a.l1)};
  }
  if (t_beg > 0) {
    // the full loop's restart frames up to t_beg (sf = c + 2 = i0(t0 - 1) + 2 at the top of group t0)
    for (int t0 = kPvGroup; t0 < t_beg; t0 += kPvGroup) {
      float al;
      const int s = ps_i0(a, t0 - 1, al) + 2;
      if (s - anchor >= kPvRestart && s < a.f_in) anchor = s;
    }
    float al;
    c = ps_i0(a, t_beg - 1, al);
    sf = c + 2;
    xre = xim = pv_t(0);
    cnt = cntc = cntn = 0;
    ca = na = pa = cf{1.f, 0.f};
    cm = nm = pm = 0.f;
    qz = ((t_beg % kPsFft) * dq) % kPsFft;
    __syncthreads();  // the prologue's reads of the d rows
    for (int q = lane; q < 2 * kPvGh * 8; q += 128) (&C.gh[0][0][0])[q] = 0.f;  // G(t, .) = 0 for t < t_beg
    fb = sf + 1;
    pv_load_rows(a, sh, xr, cl, lane, fb);
    __syncthreads();
  }
  HBK_PVT(0);  // init: the span, tables, frame 0, the first rows

  for (int t0 = t_beg; t0 <= t_last; t0 += kPvGroup) {
    // the group's source frames (and one ahead) must be resident: refill the d rows
    {
      float al;
      const int tl = min(t0 + kPvGroup - 1, a.f_out - 1);
      const int need = t0 < a.f_out ? min(ps_i0(a, tl, al) + 3, a.f_in - 1) : 0;
      if (need >= fb + kPvRows) {  // uniform across the workgroup
        __syncthreads();
        fb = sf + 1;
        pv_load_rows(a, sh, xr, cl, lane, fb);
        __syncthreads();
      }
    }
    if (sf - anchor >= kPvRestart && sf < a.f_in) {  // uniform across the workgroup
      __syncthreads();
      for (int q = lane; q < kPsFft; q += 128) C.xs[q] = ps_xp(xr, a.L, kPsHop * sf + q);
      __syncthreads();
      xre = xim = pv_t(0);
      if (cnt != 0) {
        double dre, dim;
        direct(dre, dim);
        xre = static_cast<pv_t>(dre);
        xim = static_cast<pv_t>(dim);
      }
      anchor = sf;
    }
    HBK_PVT(1);  // row refills, restarts
    R *= __builtin_amdgcn_rsqf(fmaf(R.x, R.x, R.y * R.y));
    cf tz = sh.tw[qz];  // tw[qz]; i tw[qz] = (-y, x) is read through the packed ops' neg / op_sel modifiers
    const float* dg = C.d[0] + 8 * (sf + 1 - fb);  // FULL groups: frame u slides to row sf + 1 + u
    int gor = 0;  // != 0: a frame of the group had a source frame with a non-zero sample
    float gr[kPvGroup];  // frame u: G(t0 + u, pv_g(lane & 7)) over the lane's octet
    float al_lane = 0.f;  // the source frame i0 and alpha of frame t0 + (lane & 7), read by frame u as lane u
    int i0_lane = 0;
    // one output frame; FULL: t < f_out and i0(t) = c + 1 are known for the whole group
    auto frame = [&](int u, auto full) {
      constexpr bool FULL = decltype(full)::value;
      const int t = t0 + u;
#if HBK_PV_ABLATE & 2  // profiling build: the per-bin vocoder replaced by a stand-in
      if (t < a.f_out) {
        float al;
        ps_i0(a, t, al);
        Q.x += al * tz.x;
      }
      if (false) {
#else
      if (FULL || t < a.f_out) {
#endif
        float al;
        int i0;
        if (FULL) {  // i0 = c + 1; the group's alphas were computed once, lane u -> frame u
          i0 = c + 1;
          al = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, al_lane), u));
        } else {
          i0 = __builtin_amdgcn_readlane(i0_lane, u);
          al = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, al_lane), u));
        }
        if (!FULL && i0 > c + 1) {  // rate > 1: a second source frame this step (rare)
          ++c;
          cntc = cntn;
          cntn = cnt;
          ca = na;
          cm = nm;
          na = pa;
          nm = pm;
          R = cmul(R, cmul_conj(ca, na));  // P_t = P_{t-1} u_{c+1} conj u_c = R u_{c+1}, and c + 2 becomes the frame
          pv_t nre, nim;
          int ncnt;
          slide_to(nre, nim, ncnt, C.d[sf + 1 - fb]);
          commit(nre, nim, ncnt);
          polar(pa, pm);
        }
        // the common step (i0 = c + 1): in a FULL group every frame steps (the source
        // frames rename through the unrolled frames: no selects), elsewhere selects
        const bool step = FULL || i0 > c;
        if (!FULL && !step && t > 0) R = cmul(R, cmul_conj(na, ca));  // the source frame repeats (uniform)
        c += step ? 1 : 0;
        cntc = step ? cntn : cntc;
        cntn = step ? cnt : cntn;
        gor |= cntc | cntn;
        ca = step ? na : ca;
        cm = step ? nm : cm;
        na = step ? pa : na;
        nm = step ? pm : nm;
        pv_t nre, nim;
        int ncnt;
        // candidate frame sf + 1 and its polar form, kept only when stepping (FULL: frame u
        // slides to the group's first row + u)
        slide_to(nre, nim, ncnt, FULL ? dg + 8 * u : C.d[sf + 1 - fb]);
        cf qa;
        float qm;
        polar_of(nre, nim, qa, qm);
        const float m = fmaf(al, nm - cm, cm);
        const cf P = pv_cmul(R, ca);
        // Z_t = m P e^{-2 pi i qz / 250} = m (P.x (x, -y) + P.y (y, x))
        const cf Z = pv_cmul_conj(P, tz);
        Q = __builtin_elementwise_fma(cf{m, m}, Z, Q);
        xre = step ? nre : xre;
        xim = step ? nim : xim;
        cnt = step ? ncnt : cnt;
        sf += step ? 1 : 0;
        pa = step ? qa : pa;
        pm = step ? qm : pm;
      }
      // G(t, .) over the wave's bins: 7 products, reduce-scatter over the lane octet,
      // all-reduce over the 8 octets
      const cf vq = pv_cmul(Q, tz);  // Q tw[qz]
#if HBK_PV_ABLATE & 1  // profiling build: no bin reduction
      gr[u] = vq.x * esr[u & 3].x;
#else
      cf pr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) pr[j] = __builtin_elementwise_fma(cf{vq.x, vq.x}, esr[j], cf{vq.y, vq.y} * esi[j]);
      const float q0 = pr[0].x + pv_dpp<0xB1>(pr[0].y), q1 = pr[1].x + pv_dpp<0xB1>(pr[1].y);  // lane ^ 1
      const float q2 = pr[2].x + pv_dpp<0xB1>(pr[2].y), q3 = pr[3].x + pv_dpp<0xB1>(pr[3].y);
      const float h0 = q0 + pv_dpp<0x4E>(q1), h1 = q2 + pv_dpp<0x4E>(q3);                     // lane ^ 2
      const float gv = h0 + pv_dpp<0x141>(h1);                                                 // lane ^ 7
      if (FULL) {
        gr[u] = gv;  // u is a constant of the unrolled group
      } else {
#pragma unroll
        for (int j = 0; j < kPvGroup; ++j) gr[j] = j == u ? gv : gr[j];
      }
#endif
      tz = pv_cmul(tz, e7);
    };
    // (not the group of frame 0, which has no step: there c = i0(0), not i0(t0 - 1), and at a rate in
    // [8/7, 9/7), 4/5 and 25/32 of the fast shifts, the seven steps of frames 1 .. 7 total kPvGroup as well)
    bool full = t0 > 0 && t0 + kPvGroup <= a.f_out;
    if (full) {  // per-frame advances are all >= 1 (rate > 1) or all <= 1 (rate < 1): a total of
      float al;  // kPvGroup means every frame of the group steps exactly once
      full = ps_i0(a, t0 + kPvGroup - 1, al) - c == kPvGroup;
    }
    i0_lane = ps_i0(a, t0 + (lane & 7), al_lane);
    if (full) {
#pragma unroll
      for (int u = 0; u < kPvGroup; ++u) frame(u, std::true_type{});
    } else {  // tail, repeat or double-step group (about a fifth of the groups at 125/128, 128/125)
#if HBK_PV_UNROLL_TAIL  // unrolled too: the frame's result lands in gr[u] without a select chain
#pragma unroll
#else
#pragma unroll 1
#endif
      for (int u = 0; u < kPvGroup; ++u) frame(u, std::false_type{});
    }
    qz = (qz + kPvGroup * dq) % kPsFft;  // the next group's first frame
    // reduce-scatter over the octets: octet o keeps frame o (lane ^ 8, ^ 16, ^ 32)
    float h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float keep = b3 ? gr[2 * i + 1] : gr[2 * i], send = b3 ? gr[2 * i] : gr[2 * i + 1];
      h[i] = keep + pv_dpp<0x128>(send);  // frame 2i + b3
    }
    const float h02 = pv_swap_add<true>(h[0], h[1]), h13 = pv_swap_add<true>(h[2], h[3]);
    const float gsum = pv_swap_add<false>(h02, h13);
    HBK_PVT(2);  // the group's frames
    // rows t0 .. t0 + 7 of the ring; the previous group's istft step read other rows
    if (gb < kPsHop) C.gh[w][(t0 + ou) % kPvGh][gb] = gsum;
    __syncthreads();
    HBK_PVT(3);  // G rows to LDS + barrier wait
    // the group's istft samples p = 7 t + r
    if (lane < kPsHop * kPvGroup && live) {
      const int t = t0 + lane / kPsHop, r = lane % kPsHop;
      const int m = kPsHop * t + r - kPsPad;
      if (t <= jmax && m >= 0 && m < a.l1) {
        const float g1 = C.gh[0][t % kPvGh][r] + C.gh[1][t % kPvGh][r];
        float g2 = 0.f;
        if (r <= 4) {
          if (t >= 36) g2 = C.gh[0][(t - 36) % kPvGh][r + 2] + C.gh[1][(t - 36) % kPvGh][r + 2];
        } else if (t >= 35) {
          g2 = C.gh[0][(t - 35) % kPvGh][r - 5] + C.gh[1][(t - 35) % kPvGh][r - 5];
        }
        const int lo = max(0, t - 35 + (r >= 5 ? 1 : 0)), hi = min(a.f_out - 1, t);
        // / (250 env) as a product with v_rcp_f32 (1 ulp; the IEEE division's scale / fixup
        // sequence is ~10 VALU per sample)
        const float v = (g1 - g2) * __builtin_amdgcn_rcpf(static_cast<float>(kPsFft) * static_cast<float>(hi - lo + 1));
        y[m] = (gor == 0 && t - lastnz > 35) ? 0.f : v;
      }
    }
    if (gor) lastnz = t0 + kPvGroup - 1;
    HBK_PVT(4);  // istft samples
  }
#ifdef HBK_PHASE_TIMING
  if (tid == 0)
    for (int i = 0; i < 5; ++i) atomicAdd(&g_pv_phase[i], pvt[i]);
#endif
}

__global__ void ps_taps_kernel(PitchArgs a) {
  // torchaudio _get_sinc_resample_kernel: sinc_interp_hann, width 6, rolloff 0.99
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nw * kPsTapMax) return;
  const int ph = i / kPsTapMax, q = i % kPsTapMax;
  float v = 0.f;
  if (q < 2 * a.width + a.orig) {
    const double lpw = 6.0, base = min(a.orig, a.nw) * 0.99;
    double t = static_cast<double>(static_cast<float>(-ph) / static_cast<float>(a.nw)) +
               static_cast<double>(q - a.width) / a.orig;
    t = fmin(fmax(t * base, -lpw), lpw);
    const double c = cos(t * M_PI / lpw / 2);
    t *= M_PI;
    v = static_cast<float>((t == 0.0 ? 1.0 : sin(t) / t) * c * c * (base / a.orig));
  }
  a.taps[i] = v;
}

// A resampler workgroup (clip e, frames [f0, f0 + frames), whose windows of kPsTapMax samples start at
// y index j0) with no sample of the clip's computed y range [yr.x, yr.y) in its windows: every output
// is zero. Stores them and returns true (workgroup-uniform), without reading y.
__device__ __forceinline__ bool ps_window_silent(const PitchArgs& a, int2 yr, int e, int j0, int f0, int frames,
                                                 int tid, int threads) {
  if (j0 < yr.y && j0 + (frames - 1) * a.orig + kPsTapMax > yr.x) return false;
  float* out = a.out + static_cast<int64_t>(a.idx[e]) * a.out_stride;
  const int i1 = static_cast<int>(min(static_cast<int64_t>(f0 + frames) * a.nw, static_cast<int64_t>(a.L)));
  for (int i = f0 * a.nw + tid; i < i1; i += threads) out[i] = 0.f;
  return true;
}

__global__ void __launch_bounds__(128) ps_resample_kernel(PitchArgs a) {
  // frames in pairs (f, f + 1): ys2[p] interleaves their windows, (f q, f+1 q, f q+1, f+1 q+1) per
  // float4, so one packed FMA per tap serves both frames (the taps of a phase are the same)
  static_assert(kPsTapMax % 2 == 0 && kPsResFrames % 2 == 0, "resampler pairs");
  constexpr int kPairs = kPsResFrames / 2;
  __shared__ __attribute__((aligned(16))) float ys2[kPairs][2 * kPsTapMax];
  const int ph = threadIdx.x, e = blockIdx.y;
  const int f0 = blockIdx.x * kPsResFrames;
  const float* y = a.y + static_cast<int64_t>(e) * a.l1;
  // y padded by (width, width + orig) zeros; frame f reads ypad[f orig + q]
  // (the window is read to kPsTapMax, past 2 width + orig, against zero taps)
  const int j0 = f0 * a.orig - a.width;
  const int2 yr = a.yr[e];  // y is zero (and not written) outside [yr.x, yr.y)
  if (ps_window_silent(a, yr, e, j0, f0, kPsResFrames, ph, 128)) return;
  for (int el = ph; el < kPsResFrames * kPsTapMax; el += 128) {
    const int fr = el / kPsTapMax, q = el - fr * kPsTapMax;  // q fastest: coalesced reads
    const int src = j0 + fr * a.orig + q;
    ys2[fr >> 1][2 * q + (fr & 1)] = (src >= yr.x && src < yr.y) ? y[src] : 0.f;
  }
  float tp[kPsTapMax];
  const float* tr = a.taps + min(ph, a.nw - 1) * kPsTapMax;
#pragma unroll
  for (int q = 0; q < kPsTapMax; ++q) tp[q] = tr[q];
  __syncthreads();
  if (ph >= a.nw) return;
  float* out = a.out + static_cast<int64_t>(a.idx[e]) * a.out_stride;
  for (int p = 0; p < kPairs; ++p) {
    const int i = (f0 + 2 * p) * a.nw + ph, i1 = i + a.nw;
    if (i >= a.L) break;
    cf v = {0.f, 0.f};
    if (i < a.target) {
      const float4* w = reinterpret_cast<const float4*>(ys2[p]);
#pragma unroll
      for (int q2 = 0; q2 < kPsTapMax / 2; ++q2) {
        const float4 ww = w[q2];
        v = __builtin_elementwise_fma(cf{tp[2 * q2], tp[2 * q2]}, cf{ww.x, ww.y}, v);
        v = __builtin_elementwise_fma(cf{tp[2 * q2 + 1], tp[2 * q2 + 1]}, cf{ww.z, ww.w}, v);
      }
    }
    out[i] = v.x;
    if (i1 < a.L) out[i1] = i1 < a.target ? v.y : 0.f;
  }
}


// The resampler as a GEMM on the matrix cores: out[f nw + ph] = sum_q taps[ph][q]
// ypad[f orig - width + q] is [frames x 160] x [160 x nw] per clip (K = the taps,
// zero-padded from kPsTapMax to 5 blocks of 32). v_mfma_f32_16x16x32_f16 in split
// f16 (hi*hi + hi*lo + lo*hi, f32 accumulation: ~2^-22 relative per product, as
// the f32 FMAs it replaces). A workgroup takes 64 frames of one clip: their
// windows are staged once into LDS as f16 hi / lo planes (one row per frame, the
// overlapping samples duplicated so every A fragment is one aligned 16-B read)
// after a power-of-two scale that puts the block's largest |sample| in
// [2^14, 2^15); the taps (x 2^10) are each wave's B fragments in VGPRs, two
// 16-phase tiles per wave.
typedef _Float16 rs_h8 __attribute__((ext_vector_type(8)));
typedef float rs_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void rs_split(float v, _Float16& h, _Float16& l) {
  h = static_cast<_Float16>(v);
  l = static_cast<_Float16>(v - static_cast<float>(h));
}
__global__ void __launch_bounds__(256) ps_resample_mfma_kernel(PitchArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 wh[kRsFrames][kRsLd];
  __shared__ __attribute__((aligned(16))) _Float16 wl[kRsFrames][kRsLd];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e = blockIdx.y, f0 = blockIdx.x * kRsFrames;
  const float* y = a.y + static_cast<int64_t>(e) * a.l1;
  const int2 yr = a.yr[e];  // y is zero (and not written) outside [yr.x, yr.y)
  if (ps_window_silent(a, yr, e, f0 * a.orig - a.width, f0, kRsFrames, tid, 256)) return;
  // staging: pair p = tid + 256 u of (frame p / 80, taps 2 (p % 80) and + 1)
  constexpr int kPairs = kRsFrames * kRsK / 2, kPer = kPairs / 256;
  float v0[kPer], v1[kPer];
  float mx = 0.f;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int p = tid + 256 * u, fr = p / (kRsK / 2), q = 2 * (p - fr * (kRsK / 2));
    const int src = (f0 + fr) * a.orig - a.width + q;
    const int s0 = min(max(src, 0), a.l1 - 1), s1 = min(max(src + 1, 0), a.l1 - 1);
    const float x0 = y[s0], x1 = y[s1];
    v0[u] = (src >= yr.x && src < yr.y && q < kPsTapMax) ? x0 : 0.f;
    v1[u] = (src + 1 >= yr.x && src + 1 < yr.y && q + 1 < kPsTapMax) ? x1 : 0.f;
    mx = fmaxf(mx, fmaxf(fabsf(v0[u]), fabsf(v1[u])));
  }
  // B fragments: phases 16 (2 wave + t) + (lane & 15), taps 32 ks + 8 (lane >> 4) ..
  const int n = lane & 15, kq = lane >> 4;
  rs_h8 bh[2][5], bl[2][5];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int ph = min(16 * (2 * wave + t) + n, a.nw - 1);
    const float* tr = a.taps + ph * kPsTapMax;
#pragma unroll
    for (int ks = 0; ks < 5; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int q = 32 * ks + 8 * kq + j;
        const float tv = tr[min(q, kPsTapMax - 1)];
        _Float16 h, l;
        rs_split(q < kPsTapMax ? tv * 1024.f : 0.f, h, l);
        bh[t][ks][j] = h;
        bl[t][ks][j] = l;
      }
  }
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const int ex = mx > 0.f ? min(14 - ilogbf(mx), 100) : 0;
  const float scale = ldexpf(1.f, ex), unscale = ldexpf(1.f, -ex - 10);
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int p = tid + 256 * u, fr = p / (kRsK / 2), q = 2 * (p - fr * (kRsK / 2));
    _Float16 h0, l0, h1, l1;
    rs_split(v0[u] * scale, h0, l0);
    rs_split(v1[u] * scale, h1, l1);
    wh[fr][q] = h0;
    wh[fr][q + 1] = h1;
    wl[fr][q] = l0;
    wl[fr][q + 1] = l1;
  }
  __syncthreads();
  float* out = a.out + static_cast<int64_t>(a.idx[e]) * a.out_stride;
#pragma unroll
  for (int ft = 0; ft < kRsFrames / 16; ++ft) {
    rs_f4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      const rs_h8 ah = *reinterpret_cast<const rs_h8*>(&wh[16 * ft + n][32 * ks + 8 * kq]);
      const rs_h8 al = *reinterpret_cast<const rs_h8*>(&wl[16 * ft + n][32 * ks + 8 * kq]);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[t][ks], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[t][ks], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[t][ks], acc[t], 0, 0, 0);
      }
    }
    // lane (n, kq) holds frames 16 ft + 4 kq + j of phase 16 (2 wave + t) + n
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int ph = 16 * (2 * wave + t) + n;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = (f0 + 16 * ft + 4 * kq + j) * a.nw + ph;
        if (ph < a.nw && i < a.L) out[i] = i < a.target ? acc[t][j] * unscale : 0.f;
      }
    }
  }
}

// The A/B knobs, read once per hbk_pitch_shift call (the only getenv of this unit), so one
// process can compare any two settings.
PitchKnobs read_pitch_knobs() {
  PitchKnobs k;
  const char* s = getenv("HBK_PS_SPAN");
  k.span = !(s && s[0] == '0');
  s = getenv("HBK_PS_PAIR");
  k.pair = !(s && s[0] == '0');
  k.resample_valu = getenv("HBK_PS_RESAMPLE_VALU") != nullptr;
  return k;
}

// ps_vocoder_kernel's > 64 KB of dynamic LDS needs the opt-in, a per-device function
// attribute: set once per device (idempotent, so a race of two first calls is harmless).
int vocoder_lds_opt_in() {
  constexpr int kDevices = 64;
  static std::atomic<bool> done[kDevices];
  int dev = -1;
  HBK_HIP(hipGetDevice(&dev));
  const bool tracked = dev >= 0 && dev < kDevices;
  if (tracked && done[dev].load(std::memory_order_acquire)) return HBK_OK;
  HBK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ps_vocoder_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, int(sizeof(PvShared))));
  if (tracked) done[dev].store(true, std::memory_order_release);
  return HBK_OK;
}

template <typename... Params, typename... Args>
void launch(void (*kernel)(Params...), const Grid& g, size_t lds, hipStream_t st, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(g.x, g.y), dim3(g.block), lds, st, args...);
}

}  // namespace

#ifdef HBK_PHASE_TIMING
// the vocoder's five phase counters, read and cleared (hbk_debug_aug_phase)
int pv_phase_take(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pv_phase), sizeof(unsigned long long) * 5) != hipSuccess) return -2;
  unsigned long long z[5] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_pv_phase), z, sizeof(z));
  return 0;
}
#endif

}  // namespace hbk

extern "C" {

int64_t hbk_pitch_shift_workspace_size(int64_t n, int64_t T, int32_t sample_rate, int32_t num, int32_t den) {
  hbk::PitchGeometry g;
  std::string err;
  if (n <= 0 || hbk::pitch_geometry(T, sample_rate, num, den, g, err) != HBK_OK) return 0;
  return hbk::pitch_layout(g, n).total;
}

int hbk_pitch_shift(const float* x, int64_t x_stride, int64_t n, const int32_t* idx, int64_t T, int32_t sample_rate,
                    int32_t num, int32_t den, float* out, int64_t out_stride, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  if (n < 0) return arg_error("negative n");
  if (n == 0) return HBK_OK;
  if (n > 65535) return arg_error("n > 65535 per call");
  if (!x || !idx || !out || !workspace) return arg_error("NULL pointer");
  PitchGeometry g;
  std::string err;
  const int rc = pitch_geometry(T, sample_rate, num, den, g, err);
  if (rc != HBK_OK) {
    set_error("%s", err.c_str());
    return rc;
  }
  if (x_stride < T || out_stride < T) return arg_error("stride < T");
  const PitchLayout off = pitch_layout(g, n);
  if (workspace_bytes < off.total) return arg_error("workspace too small (hbk_pitch_shift_workspace_size)");
  const PitchKnobs knobs = read_pitch_knobs();
  const PitchLaunches L = pitch_launches(g, n, knobs);
  unsigned char* w = static_cast<unsigned char*>(workspace);
  PitchArgs a{};
  a.x = x;
  a.x_stride = x_stride;
  a.idx = idx;
  a.n = static_cast<int>(n);
  a.out = out;
  a.out_stride = out_stride;
  a.L = g.L, a.f_in = g.f_in, a.f_out = g.f_out, a.l1 = g.l1;
  a.orig = g.orig, a.nw = g.nw, a.width = g.width, a.target = g.target;
  a.rate = g.rate;
  a.y = reinterpret_cast<float*>(w + off.y);
  a.taps = reinterpret_cast<float*>(w + off.taps);
  a.yr = reinterpret_cast<int2*>(w + off.yr);
  a.span = knobs.span ? 1 : 0;
  if (L.pair) {
    a.sp = reinterpret_cast<int2*>(w + off.sp);
    a.key = reinterpret_cast<uint64_t*>(w + off.key);
    a.ord = reinterpret_cast<int32_t*>(w + off.ord);
    a.gord = reinterpret_cast<int32_t*>(w + off.gord);
  }
  const int lds_rc = vocoder_lds_opt_in();
  if (lds_rc != HBK_OK) return lds_rc;
  hipStream_t st = as_stream(stream);
  launch(ps_taps_kernel, L.taps, 0, st, a);
  HBK_LAUNCH_CHECK("ps_taps_kernel");
  if (L.pair) {
    launch(ps_span_kernel, L.span, 0, st, a);
    HBK_LAUNCH_CHECK("ps_span_kernel");
    launch(ps_rank_kernel, L.rank_clips, 0, st, static_cast<const uint64_t*>(a.key), a.n, a.ord);
    HBK_LAUNCH_CHECK("ps_rank_kernel");
    launch(ps_group_kernel, L.group, 0, st, a, L.groups);
    HBK_LAUNCH_CHECK("ps_group_kernel");
    launch(ps_rank_kernel, L.rank_groups, 0, st, static_cast<const uint64_t*>(a.key), L.groups, a.gord);
    HBK_LAUNCH_CHECK("ps_rank_kernel");
  }
  launch(ps_vocoder_kernel, L.vocoder, sizeof(PvShared), st, a);
  HBK_LAUNCH_CHECK("ps_vocoder_kernel");
  launch(L.resample_mfma ? ps_resample_mfma_kernel : ps_resample_kernel, L.resample, 0, st, a);
  HBK_LAUNCH_CHECK(L.resample_mfma ? "ps_resample_mfma_kernel" : "ps_resample_kernel");
  return HBK_OK;
}

}  // extern "C"
