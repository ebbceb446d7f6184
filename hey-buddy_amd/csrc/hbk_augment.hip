// Fused batch augmentation for gfx950: gain + background-noise mix + IR reverb.
//
// Gain: torch_audiomentations Gain (per-batch dB ~ U[-18, 6], p 1.0 in the
// reference's batch chain, augmented.py:114-118), a per-clip factor applied
// to x on load.
// Replaces add_background_noise_to_batch -> torchaudio.functional.add_noise
// (augmented.py:234-276, :383-384) and speechbrain's reverberate(batch, ir)
// (augmented.py:386-392) of AugmentedAudioGenerator.execute_augment_batch.
//
// One workgroup (1024 threads) per clip, the whole clip resident in LDS:
//   x and the clip's noise segment arrive in registers (loaded after the
//   previous clip's inverse FFT) -> E_x, E_n ->
//   y = x + 10^((10 log10(E_x/E_n) - snr)/20) n -> LDS, a_in = mean|y|
//   circular convolution with the batch's IR kernel of length T = 23040:
//     z[n] = y[2n] + i y[2n+1], an 11520-point complex FFT done in place in
//     LDS as four mixed-radix decimation-in-frequency passes 16 x 16 x 9 x 5
//     (720, 720, 1280 and 2304 independent DFTs per pass, one per thread and
//     round, radix-16 / 9 / 5 in VGPRs); twiddles W_M^e = HI[e >> 7] LO[e & 127]
//     from two small LDS tables. Z lands in digit-reversed order (zaddr); the
//     real-FFT split, * H[k] and the inverse split run on (k, M-k) pairs (H and
//     W_N^k stored bin-major, [k % 16][k / 16], so those loads coalesce); the
//     inverse transform is the passes reversed (decimation in time, conjugate
//     twiddles) and lands back in natural order.
//   y <- a_in * y / (mean|y| + 1e-14), store.
// The IR spectrum H (one per batch) comes from the same transform run on the
// rotated kernel [ir[d:], 0..., ir[:d]] (hbk_reverb_spectrum).
//
// This unit holds the reverb family: augment, spectrum, band-stop and colored
// noise, which share the LDS transforms and the plan's twiddle tables. The
// constants, the workspace layouts and the tables' values come from
// hbk_augment_plan.h (host only, checked on the CPU); the helpers shared with
// hbk_clip_ops.hip from hbk_aug_dev.h. Pitch shift lives in hbk_pitch.hip.
#include <algorithm>

#include "hbk_aug_dev.h"

namespace hbk {
namespace {

static_assert(kHSlots == HBK_REVERB_SPECTRUM_SLOTS, "spectrum slot layout");
static_assert(kBsCirc == HBK_BAND_STOP_CIRCULAR_MAX_HALF && kBsPart == HBK_BAND_STOP_PARTITION_TAPS,
              "the band-stop constants of hbk.h");

// The two LDS transforms: kN complex points, twiddles W_kN^e = hi[e / kLo] * lo[e % kLo] from two small
// tables (kN / kLo and kLo entries).
struct Fft11520 {  // reverb, band-stop: passes 16 x 16 x 9 x 5, tables 90 x 128
  static constexpr int kN = kM, kLo = kTwLo;
  // the radix-16 twiddles as 4 lookups and products; lanes walk blocks over the short span of 5
  static constexpr bool kR16Products = true, kShortSpanWalksBlocks = true;
};
struct Fft8000 {  // colored noise: passes 16 x 5 x 5 x 5 x 4, tables 80 x 100
  static constexpr int kN = kM1, kLo = kTw8Lo;
  static constexpr bool kR16Products = false, kShortSpanWalksBlocks = false;
};

template <class F, bool INV>
__device__ __forceinline__ cf twiddle(const cf* thi, const cf* tlo, int e) {
  if constexpr ((F::kLo & (F::kLo - 1)) == 0) {  // (e >= 0: a shift and a mask, which a signed division is not)
    const cf w = cmul(thi[e >> __builtin_ctz(F::kLo)], tlo[e & (F::kLo - 1)]);
    return INV ? cf{w.x, -w.y} : w;
  } else {
    const int h = e / F::kLo;
    const cf w = cmul(thi[h], tlo[e - h * F::kLo]);
    return INV ? cf{w.x, -w.y} : w;
  }
}

template <int R, bool INV>
__device__ __forceinline__ void dftr(cf (&v)[R]) {
  if constexpr (R == 16) fft16v<INV>(v);
  else if constexpr (R == 9) dft9<INV>(v);
  else if constexpr (R == 4) fft4v<INV>(v[0], v[1], v[2], v[3]);
  else dft5<INV>(v);
}

// One in-place pass of radix R over span L (blocks of R L elements): task
// (blk, i) owns elements blk R L + i + L m, m < R. Forward (DIF): DFT-R, then
// output k times W_N^(S i k). Inverse (DIT): input k times conj W_N^(S i k),
// then the inverse DFT-R. Independent tasks, so one barrier per pass.
template <class F, int R, int L, int S, bool INV>
__device__ __forceinline__ void pass(cf* z, const cf* thi, const cf* tlo) {
  constexpr int kTasks = F::kN / R;
  // (the opaque thread id keeps the per-pass index math inside the clip loop)
  for (int t = opaque_tid(); t < kTasks; t += kThreads) {
    // lanes walk i (contiguous addresses) when L is large, blocks (stride R L =
    // 45 complex: conflict-free over 32 lanes) when L is the short span of 5
    constexpr int kBlocks = F::kN / (R * L);
    int blk, i;
    if constexpr (F::kShortSpanWalksBlocks && L < 16) {
      i = t / kBlocks;
      blk = t - i * kBlocks;
    } else {
      blk = t / L;
      i = t - blk * L;
    }
    cf* q = z + blk * (R * L) + i;
    cf v[R];
#pragma unroll
    for (int m = 0; m < R; ++m) v[m] = q[L * m];
    cf w[R];  // w[k] = W_N^(S i k) (conjugated for INV)
    if constexpr (S != 0) {
      if constexpr (R == 16 && F::kR16Products) {
        // 4 table lookups (k = 1, 2, 4, 8), the other powers as products (<= 3 deep)
        w[1] = twiddle<F, INV>(thi, tlo, S * i);
        w[2] = twiddle<F, INV>(thi, tlo, 2 * S * i);
        w[4] = twiddle<F, INV>(thi, tlo, 4 * S * i);
        w[8] = twiddle<F, INV>(thi, tlo, 8 * S * i);
        w[3] = cmul(w[1], w[2]);
        w[5] = cmul(w[1], w[4]);
        w[6] = cmul(w[2], w[4]);
        w[7] = cmul(w[3], w[4]);
#pragma unroll
        for (int k = 9; k < 16; ++k) w[k] = cmul(w[k - 8], w[8]);
      } else {
#pragma unroll
        for (int k = 1; k < R; ++k) w[k] = twiddle<F, INV>(thi, tlo, S * i * k);
      }
    }
    if (INV && S)
#pragma unroll
      for (int k = 1; k < R; ++k) v[k] = cmul(v[k], w[k]);
    dftr<R, INV>(v);
    if (!INV && S)
#pragma unroll
      for (int k = 1; k < R; ++k) v[k] = cmul(v[k], w[k]);
#pragma unroll
    for (int m = 0; m < R; ++m) q[L * m] = v[m];
  }
}

#ifdef HBK_PHASE_TIMING
// Profiling build only (build.py variant "phase"): thread 0 of every block adds
// the s_memtime cycles of each augment phase (barrier waits included in the
// phase before them) into g_aug_phase; read by hbk_debug_aug_phase.
__device__ unsigned long long g_aug_phase[32];
#define HBK_APH(i)                                                  \
  do {                                                              \
    if (threadIdx.x == 0) {                                         \
      const unsigned long long t_ = __builtin_amdgcn_s_memtime();   \
      atomicAdd(&g_aug_phase[i], t_ - ph_t0);                       \
      ph_t0 = t_;                                                   \
    }                                                               \
  } while (0)
#else
#define HBK_APH(i) \
  do {             \
  } while (0)
#endif

// Forward: natural z -> Z[f] at zaddr(f); inverse: the reverse (x kM).
// (ph_t0 / ph: phase-timing build only, phases ph .. ph + 3)
template <bool INV>
__device__ __forceinline__ void transform(cf* z, const cf* thi, const cf* tlo,
                                          [[maybe_unused]] unsigned long long& ph_t0,
                                          [[maybe_unused]] int ph) {
  if (!INV) {
    pass<Fft11520, 16, 720, 1, false>(z, thi, tlo);
    __syncthreads();
    HBK_APH(ph);
    pass<Fft11520, 16, 45, 16, false>(z, thi, tlo);
    __syncthreads();
    HBK_APH(ph + 1);
    pass<Fft11520, 9, 5, 256, false>(z, thi, tlo);
    __syncthreads();
    HBK_APH(ph + 2);
    pass<Fft11520, 5, 1, 0, false>(z, thi, tlo);
    __syncthreads();
    HBK_APH(ph + 3);
  } else {
    pass<Fft11520, 5, 1, 0, true>(z, thi, tlo);
    __syncthreads();
    HBK_APH(ph);
    pass<Fft11520, 9, 5, 256, true>(z, thi, tlo);
    __syncthreads();
    HBK_APH(ph + 1);
    pass<Fft11520, 16, 45, 16, true>(z, thi, tlo);
    __syncthreads();
    HBK_APH(ph + 2);
    pass<Fft11520, 16, 720, 1, true>(z, thi, tlo);
    __syncthreads();
    HBK_APH(ph + 3);
  }
}

// Position of frequency f = k1 + 16 k2 + 256 k3 + 2304 k4 after the forward
// passes: 720 k1 + 45 k2 + 5 k3 + k4 (mixed-radix digit reversal).
__device__ __forceinline__ int zaddr(int f) {
  const int k1 = f & 15, r = f >> 4;
  const int k2 = r & 15, r2 = r >> 4;
  const int k4 = r2 / 9, k3 = r2 - 9 * k4;
  return 720 * k1 + 45 * k2 + 5 * k3 + k4;
}

// Frequency stored at position p (inverse of zaddr).
__device__ __forceinline__ int zfreq(int p) {
  const int k1 = p / 720, r = p - 720 * k1;
  const int k2 = r / 45, r2 = r - 45 * k2;
  const int k3 = r2 / 5, k4 = r2 - 5 * k3;
  return k1 + 16 * k2 + 256 * k3 + 2304 * k4;
}

// the twiddle tables into LDS (after z and the reduction slots)
__device__ __forceinline__ void load_tw(cf* thi, cf* tlo, const float2* ghi, const float2* glo) {
  for (int i = threadIdx.x; i < kTwHi; i += kThreads) thi[i] = cf{ghi[i].x, ghi[i].y};
  for (int i = threadIdx.x; i < kTwLo; i += kThreads) tlo[i] = cf{glo[i].x, glo[i].y};
}

// spectrum / W_N^k slot of bin k <= kM: [k % 16][k / 16] (HBK_REVERB_SPECTRUM_SLOTS):
// the pair loop's lanes walk k in steps of 16, i.e. consecutive slots
__device__ __forceinline__ int hslot(int k) { return (k & 15) * kHRow + (k >> 4); }

struct AugArgs {
  const float* x;
  int64_t x_stride;
  float* out;
  int64_t out_stride;
  int64_t n_clips;
  const float* ring;        // background-noise ring (all noise clips back to back)
  int64_t ring_len;
  const int64_t* noise_off; // per clip: ring offset of its segment, < 0 = no noise
  const float* snr_db;      // per clip
  const float2* spectra;    // [n_spec][kHSlots], bin k at hslot(k)
  const int* spec_idx;      // per clip: spectrum index, < 0 = no reverb
  const float* gain;        // per clip linear gain, or NULL
  const float2* thi;        // W_M^(128 h), h < 90
  const float2* tlo;        // W_M^l, l < 128
  const float2* twn;        // W_N^k, k <= kM, at hslot(k)
  // colored noise folded into the prologue (hbk_augment_colored; c_snr NULL: none). A clip
  // with a non-NaN c_snr whose group's coloured second was made (c_grms[g] not NaN) and
  // whose f_decay equals its group's first clip's is mixed here, exactly as
  // colored_mix_kernel mixes it; any other coloured clip was written to out by
  // colored_noise_kernel beforehand and is read from out instead of x.
  const float* c_snr;
  const float* c_fd;
  int64_t c_group;
  const float* c_gbuf;      // [groups][16000]: the coloured second x 8000
  const float* c_grms;      // [groups], NULL: no group path
  // placement on first touch (hbk_reverb_plan_set_source; pre NULL: none): a clip with
  // pre >= 0 is read from its source row through load_placed instead of from x. A clip
  // coloured by colored_noise_kernel (colored_mode 2) is placed: that kernel reads x.
  SrcView view;
};

// (pre, n = min(len, T)) of a clip read through the view, packed into one uniform word
// (both < 2^15: T = 23,040) so that the read-ahead costs this kernel one SGPR; < 0: placed
__device__ __forceinline__ int view_word(const AugArgs& a, int64_t clip) {
  if (!a.view.pre) return -1;
  const int pre = a.view.pre[clip], len = a.view.len[clip];  // (two independent loads: one latency)
  return pre < 0 ? -1 : (min(pre, kT) << 16) | max(min(len, kT), 0);
}

// 0: no colored noise, 1: mixed in augment_kernel's prologue, 2: coloured by
// colored_noise_kernel into out (uniform per clip)
__device__ __forceinline__ int colored_mode(const AugArgs& a, int64_t clip) {
  if (!a.c_snr) return 0;
  const float snr = a.c_snr[clip];
  if (snr != snr) return 0;
  if (a.c_grms) {
    const int64_t g = clip / a.c_group;
    const float r = a.c_grms[g];
    if (r == r && a.c_fd[clip] == a.c_fd[g * a.c_group]) return 1;
  }
  return 2;
}

__global__ void __launch_bounds__(kThreads) augment_kernel(AugArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cf* z = reinterpret_cast<cf*>(smem);                      // kM complex
  float* red = smem + 2 * kM;                               // 32 floats
  cf* thi = reinterpret_cast<cf*>(smem + 2 * kM + 32);
  cf* tlo = thi + kTwHi;
  load_tw(thi, tlo, a.thi, a.tlo);
  const cf* twn = reinterpret_cast<const cf*>(a.twn);
  float* zf = smem;
  const int tid = threadIdx.x;
  // the next clip's samples are loaded into registers while this clip's
  // transforms run (one clip per CU: otherwise every load is exposed); the
  // noise segment is read twice (energy, then mix; the 2nd read hits L2)
  constexpr int kPer = (kT + kThreads - 1) / kThreads;
  float xr[kPer], nr[kPer];
  // the next clip's samples and noise segment  are loaded after this clip's inverse FFT,
  // so their latency hides behind the |y| sum and the stores without holding
  // VGPRs through the FFT passes
  // (noff: the clip's noise offset, read well before, so that no branch waits
  // on a load queued behind these; vmcnt retires loads in order)
  // (cmode: colored_mode of the clip, read ahead like noff; 2 = read the clip from out)
  // (vw: view_word of the clip, read ahead like them; >= 0: the loads go to the source row,
  // at place_kernel's clamped indices, one load per slot whatever the wave's placed_class (a
  // second load instruction per slot behind a branch made the compiler wait for every load in
  // flight before it); the clip's loop turn selects the zeros around the source clip)
  auto prefetch = [&](int64_t clip, int64_t noff, int cmode, int vw) {
    // uniform base + 32-bit per-lane offsets from an opaque thread id (keeps
    // the 46 per-load addresses from being hoisted out of the clip loop)
    const int t = opaque_tid();
    // one uniform element offset from a.x. (The colored fold pushes this kernel's SGPRs over
    // the limit: 2 x 8 B of VGPR spills, stored and reloaded once per clip, outside the passes.)
    const int64_t row = cmode == 2 ? (a.out - a.x) + clip * a.out_stride : clip * a.x_stride;
    const float* x = a.x + row;
    // 32-bit BYTE offsets from a uniform base: global_load's saddr form, one
    // VGPR per address (ring_len < 2^30, checked on the host)
    auto at = [](const float* base, uint32_t i) {
      return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + (i << 2));
    };
    if (vw >= 0 && cmode != 2) {
      const int pre = vw >> 16, n = vw & 0xFFFF;
      // (an empty source clip: any readable row, every sample is selected to 0)
      const float* s = n > 0 ? a.view.src + clip * a.view.stride : x;
#pragma unroll
      for (int u = 0; u < kPer; ++u) xr[u] = at(s, placed_index(pre, n, min(t + u * kThreads, kT - 1)));
    } else {
#pragma unroll
      for (int u = 0; u < kPer; ++u) xr[u] = at(x, static_cast<uint32_t>(min(t + u * kThreads, kT - 1)));
    }
    if (noff >= 0) {
      const uint32_t rlen = static_cast<uint32_t>(a.ring_len), r0 = static_cast<uint32_t>(noff);
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        uint32_t r = r0 + static_cast<uint32_t>(min(t + u * kThreads, kT - 1));
        r = r >= rlen ? r - rlen : r;
        nr[u] = at(a.ring, r);
      }
    }
  };
  // (the clip's own word is carried from the turn that read it ahead: no load at the loop's top)
  int vw_cur = blockIdx.x < a.n_clips ? __builtin_amdgcn_readfirstlane(view_word(a, blockIdx.x)) : -1;
  if (blockIdx.x < a.n_clips) prefetch(blockIdx.x, a.noise_off[blockIdx.x], colored_mode(a, blockIdx.x), vw_cur);
  unsigned long long ph_t0 = 0;
#ifdef HBK_PHASE_TIMING
  ph_t0 = __builtin_amdgcn_s_memtime();
#endif
  for (int64_t clip = blockIdx.x; clip < a.n_clips; clip += gridDim.x) {
    // 1) y = x + scale n (torchaudio add_noise: snr0 = 10 (log10 Ex - log10 En),
    //    scale = 10^((snr0 - snr)/20)) in registers; y goes to LDS once and
    //    a_in = mean|y| is summed on the way
    const int64_t noff = a.noise_off[clip];
    const int sp = a.spec_idx[clip];
    const float gain = a.gain ? a.gain[clip] : 1.f;
    const bool next = clip + gridDim.x < a.n_clips;
    const int64_t noff_next = __builtin_amdgcn_readfirstlane(static_cast<int>(next ? a.noise_off[clip + gridDim.x] : -1));
    const int cmode = __builtin_amdgcn_readfirstlane(colored_mode(a, clip));
    const int cmode_next = __builtin_amdgcn_readfirstlane(next ? colored_mode(a, clip + gridDim.x) : 0);
    const int vw = vw_cur;
    const int vw_next = __builtin_amdgcn_readfirstlane(next ? view_word(a, clip + gridDim.x) : -1);
    vw_cur = vw_next;
    float ex = 0.f, aa = 0.f;
    if (vw >= 0 && cmode != 2) {  // read through the view: the zeros around the source clip (a wave
      // whose 64 samples lie inside it has none to select: placed_class, uniform)
      const int t = opaque_tid(), pre = vw >> 16, n = vw & 0xFFFF;
      const int w0 = __builtin_amdgcn_readfirstlane(t & ~63);
#pragma unroll
      for (int u = 0; u < kPer; ++u)
        if (placed_class(pre, n, w0 + u * kThreads) != 1)
          xr[u] = placed_select(xr[u], pre, n, min(w0 + u * kThreads + (t & 63), kT - 1));
    }
    if (cmode == 1) {
      // colored noise (the group path), in colored_mix_kernel's per-thread order and block
      // sum: bit-identical to hbk_colored_noise_ws followed by hbk_augment
      const int64_t g = clip / a.c_group;
      const float* gb = a.c_gbuf + g * kN1;
      const int t = opaque_tid();
      // explicit fmaf, as colored_mix_kernel: a plain `ec += x * x` here was SLP-vectorised
      // into v_pk_mul + v_add (two roundings) and moved 1 in ~30 clips by an ulp
      float ec = 0.f, ez = 0.f;
#pragma unroll
      for (int u = 0; u < kPer; ++u)
        if (t + u * kThreads < kT) ec = fmaf(xr[u], xr[u], ec);
      block_sum2(ec, ez, red);
      const float rms_x = sqrtf(ec / kT);
      const float scale = rms_x / powf(10.f, a.c_snr[clip] / 20.f) / (a.c_grms[g] + 1e-8f) * (1.f / kM1);
      // the coloured second from L2 (64 KB per batch), loaded after the sum: held across it,
      // its 23 registers spilled
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int s = min(t + u * kThreads, kT - 1);
        const int sn = s < kN1 ? s : s - kN1;
        xr[u] = fmaf(scale,
                     *reinterpret_cast<const float*>(reinterpret_cast<const char*>(gb) + (static_cast<uint32_t>(sn) << 2)),
                     xr[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      xr[u] *= gain;
      if (tid + u * kThreads < kT) ex += xr[u] * xr[u];
    }
    HBK_APH(0);
    if (noff >= 0) {
      float en = 0.f;
#pragma unroll
      for (int u = 0; u < kPer; ++u)
        if (tid + u * kThreads < kT) en += nr[u] * nr[u];
      HBK_APH(1);
      block_sum2(ex, en, red);
      HBK_APH(2);
      const float snr0 = 10.f * (log10f(ex) - log10f(en));
      const float scale = powf(10.f, (snr0 - a.snr_db[clip]) / 20.f);
#pragma unroll
      for (int u = 0; u < kPer; ++u) xr[u] += scale * nr[u];
    }
    {
      const int t = opaque_tid();
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int s = t + u * kThreads;
        if (s < kT) {
          zf[s] = xr[u];
          aa += fabsf(xr[u]);
        }
      }
    }
    HBK_APH(3);
    float* out = a.out + clip * a.out_stride;
    if (sp < 0) {  // no reverb: each thread stores the samples it wrote
      if (next) prefetch(clip + gridDim.x, noff_next, cmode_next, vw_next);
      for (int s = opaque_tid(); s < kT; s += kThreads) out[s] = zf[s];
      __syncthreads();
      continue;
    }
    // 2) a_in = mean |y| (block_sum's first barrier also publishes zf)
    const float a_in = block_sum(aa, red) / kT;
    HBK_APH(4);
    // 3) forward FFT (natural -> permuted)
    transform<false>(z, thi, tlo, ph_t0, 5);
    // 4) split, multiply by H, inverse split, on (k, M-k) pairs
    const cf* H = reinterpret_cast<const cf*>(a.spectra) + static_cast<int64_t>(sp) * kHSlots;
    // one thread per pair (k, M - k), k <= M / 2; consecutive lanes take k in
    // steps of 16 (k = c + 16 r, c = idx / 361), so their positions zaddr(k)
    // step by 45 complex instead of 720 (no 16-way bank conflicts)
    // All of a thread's H[k], H[M - k], W_N^k (L2-resident) are loaded in one
    // batch before the loop: one exposed latency instead of one per pair.
    constexpr int kRest = kM / 2 / 16 + 1;  // 361
    constexpr int kSplitIt = (16 * kRest + kThreads - 1) / kThreads;
    cf hk[kSplitIt], hc[kSplitIt], wn[kSplitIt];
    const int ts = opaque_tid();
    auto pair_k = [&](int it) {
      const int idx = min(ts + it * kThreads, 16 * kRest - 1);
      const int c = idx / kRest;
      return min(c + 16 * (idx - c * kRest), kM / 2);
    };
#pragma unroll
    for (int it = 0; it < kSplitIt; ++it) {
      const int k = pair_k(it);
      hk[it] = H[hslot(k)];
      hc[it] = H[hslot(kM - k)];
      wn[it] = twn[hslot(k)];
    }
#pragma unroll
    for (int it = 0; it < kSplitIt; ++it) {
      const int idx = ts + it * kThreads;
      const int c = idx / kRest;
      const int k = c + 16 * (idx - c * kRest);
      if (idx >= 16 * kRest || k > kM / 2) continue;
      const int kc = (kM - k) % kM;
      const int p = zaddr(k);
      const cf zk = z[p];
      const cf zc = z[zaddr(kc)];
      const cf fe = 0.5f * cf{zk.x + zc.x, zk.y - zc.y};
      const cf fo = 0.5f * cf{zk.y + zc.y, zc.x - zk.x};
      const cf wk = wn[it];
      const cf Xk = fe + cmul(wk, fo);
      // partner: Fe' = conj(fe), Fo' = conj(fo), W_N^(M-k) = -conj(W_N^k)
      const cf fe2 = cf{fe.x, -fe.y};
      const cf fo2 = cf{fo.x, -fo.y};
      const cf wk2 = cf{-wk.x, wk.y};
      const cf Xc = fe2 + cmul(wk2, fo2);  // X[M - k] (X[M] when k = 0)
      const cf Yk = cmul(Xk, hk[it]);
      const cf Yc = cmul(Xc, hc[it]);
      // inverse split: Z'[k] = (Y[k] + conj Y[M-k])/2 + i W_N^-k (Y[k] - conj Y[M-k])/2
      const cf s1 = 0.5f * cf{Yk.x + Yc.x, Yk.y - Yc.y};
      const cf d1 = 0.5f * cf{Yk.x - Yc.x, Yk.y + Yc.y};
      const cf wd = cmul(cf{wk.x, -wk.y}, d1);
      const cf zk2 = s1 + cf{-wd.y, wd.x};
      // partner k' = M - k: Y[k'] = Yc, Y[M-k'] = Yk, W_N^-(M-k) = -W_N^k
      const cf s2 = 0.5f * cf{Yc.x + Yk.x, Yc.y - Yk.y};
      const cf d2 = 0.5f * cf{Yc.x - Yk.x, Yc.y + Yk.y};
      const cf wd2 = cmul(cf{-wk.x, -wk.y}, d2);
      const cf zc2 = s2 + cf{-wd2.y, wd2.x};
      z[p] = zk2;
      if (kc != k) z[zaddr(kc)] = zc2;
    }
    __syncthreads();
    HBK_APH(9);
    // 5) inverse FFT (permuted -> natural), 1/M
    transform<true>(z, thi, tlo, ph_t0, 10);
    if (next) prefetch(clip + gridDim.x, noff_next, cmode_next, vw_next);
    float ay = 0.f;
    for (int s = opaque_tid(); s < kT; s += kThreads) ay += fabsf(zf[s]);
    const float a_out = block_sum(ay, red) / kT / kM;
    HBK_APH(14);
    const float g = a_in / (a_out + 1e-14f) / kM;
    for (int s = opaque_tid(); s < kT; s += kThreads) out[s] = zf[s] * g;
    __syncthreads();
    HBK_APH(15);
  }
}

// Spectrum of one rotated IR kernel k [kT] -> H[k], k = 0..kM (natural order).
__global__ void __launch_bounds__(kThreads) spectrum_kernel(const float* kern, int64_t kern_stride,
                                                            float2* spectra, const float2* thi_,
                                                            const float2* tlo_, const float2* twn_) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  cf* thi = reinterpret_cast<cf*>(smem + 2 * kM + 32);
  cf* tlo = thi + kTwHi;
  load_tw(thi, tlo, thi_, tlo_);
  const cf* twn = reinterpret_cast<const cf*>(twn_);
  const float* k = kern + blockIdx.x * kern_stride;
  for (int s = threadIdx.x; s < kT; s += kThreads) smem[s] = k[s];
  __syncthreads();
  unsigned long long ph_t0 = 0;
  transform<false>(z, thi, tlo, ph_t0, 16);
  float2* H = spectra + static_cast<int64_t>(blockIdx.x) * kHSlots;
  for (int q = threadIdx.x; q <= kM; q += kThreads) {
    const int qq = q % kM, qc = (kM - q) % kM;
    const cf zk = z[zaddr(qq)];
    const cf zc = z[zaddr(qc)];
    const cf fe = 0.5f * cf{zk.x + zc.x, zk.y - zc.y};
    const cf fo = 0.5f * cf{zk.y + zc.y, zc.x - zk.x};
    const cf X = fe + cmul(twn[hslot(q)], fo);
    H[hslot(q)] = make_float2(X.x, X.y);
  }
}

// ---- band-stop ------------------------------------------------------------
// torch_audiomentations BandStopFilter (the reference's batch chain,
// augmented.py:101-105; p 0.25 per batch, one parameter set per batch):
//   y = x - julius.bandpass_filter(x, cut_lo, cut_hi)
// julius: the difference of two windowed-sinc lowpasses of half size
// h = int(8 / cut_lo / 2) over the clip padded by h replicated edge samples,
//   f_c[t] = 2 c hann[t + h] sinc(2 pi c t) / sum, t in [-h, h]
// (taps in float32 arithmetic, as torch computes them); g = f_hi - f_lo.
// Three launches per call: per filter (batch) the two lowpass sums and, for
// short filters, the taps g[0..h]; per filter spectrum (the reverb transform);
// per clip the convolution:
//  * h <= HBK_BAND_STOP_CIRCULAR_MAX_HALF (about 80 % of the reference's draws):
//    the clip's circular convolution with g (one forward and one inverse
//    transform, like the reverb), then the 2h edge samples corrected directly:
//    for n < h the taps that wrapped to the clip's end are replaced by the
//    replicated first sample, sum_{d < -n} g[d] (x[0] - x[T + n + d]), and
//    likewise at the other end;
//  * longer filters: overlap-save. f[k] = g[k - h], k < 2h + 1, in partitions
//    of kBsPart taps, each with its own spectrum; for partition p and output
//    half b the segment s[j] = xpad[11520 b + p kBsPart + j] (xpad[m] =
//    x[clamp(m - h, 0, T - 1)]) is transformed, multiplied, transformed back:
//    samples 0..11519 are the partition's sum for n = 11520 b + i (i + k <
//    23040: nothing wraps); the clip sits in a per-block global scratch row
//    (the output may alias the input).

// unnormalised julius lowpass tap t in [-h, h] (float32 as torch: hann from
// arange * f32(2 pi / (2h)), arg = f32(2 pi c) * t, 2c * w * sinc)
struct BsLowpass {
  float two_c, two_pi_c, wstep;
  int h;
  __device__ __forceinline__ BsLowpass(float c, int h_) : h(h_) {
    two_c = static_cast<float>(2.0 * double(c));
    two_pi_c = static_cast<float>(2.0 * double(c) * M_PI);
    wstep = static_cast<float>(2.0 * M_PI / double(2 * h_));
  }
  __device__ __forceinline__ float tap(int t) const {
    const float w = 0.5f - 0.5f * cosf(static_cast<float>(t + h) * wstep);
    const float arg = two_pi_c * static_cast<float>(t);
    const float sinc = arg == 0.f ? 1.f : sinf(arg) / arg;
    return two_c * w * sinc;
  }
};

struct BandStopArgs {
  const float* x;
  int64_t x_stride;
  float* out;
  int64_t out_stride;
  int64_t n;               // filtered clips
  const int32_t* idx;      // clip row of entry e
  const int32_t* filt;     // filter of entry e
  int n_filters;
  const float* f_lo;       // per filter: cutoffs (fraction of the sample rate), half size,
  const float* f_hi;       //   first spectrum slot
  const int32_t* f_half;
  const int32_t* f_spec0;
  int n_spectra;
  const int32_t* s_filt;   // per spectrum: filter, partition (-1: circular kernel)
  const int32_t* s_part;
  float2* sums;            // [n_filters]: the two lowpass sums (lo, hi)
  float* taps;             // [n_filters][kBsCirc + 1]: g[0..h] of circular filters
  float2* spectra;         // [n_spectra][kHSlots]
  float* scratch;          // [gridDim.x][kT]: overlap-save clips
  const float2* thi;
  const float2* tlo;
  const float2* twn;
};

// g[t] from the normalised lowpasses
__device__ __forceinline__ float bs_g(const BsLowpass& lo, const BsLowpass& hi, float2 s, int t) {
  return hi.tap(t) / s.y - lo.tap(t) / s.x;
}

// launch 1: one block per filter
__global__ void __launch_bounds__(kThreads) band_stop_sums_kernel(BandStopArgs a) {
  __shared__ float red[32];
  const int f = blockIdx.x;
  const int h = a.f_half[f];
  const BsLowpass lo(a.f_lo[f], h), hi(a.f_hi[f], h);
  double sl = 0.0, sh = 0.0;
  for (int t = static_cast<int>(threadIdx.x) - h; t <= h; t += kThreads) {
    sl += lo.tap(t);
    sh += hi.tap(t);
  }
  float fl = static_cast<float>(sl), fh = static_cast<float>(sh);
  block_sum2(fl, fh, red);
  const float2 sm = make_float2(fl, fh);
  if (threadIdx.x == 0) a.sums[f] = sm;
  if (h <= kBsCirc)
    for (int t = threadIdx.x; t <= h; t += kThreads) a.taps[int64_t(f) * (kBsCirc + 1) + t] = bs_g(lo, hi, sm, t);
}

// launch 2: one block per spectrum: circular kernel kappa[m] = g[(-m) mod T]
// (|t| <= h) or overlap-save partition p: kappa[0] = f_p[0], kappa[T - k] = f_p[k]
__global__ void __launch_bounds__(kThreads) band_stop_spectrum_kernel(BandStopArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  cf* thi = reinterpret_cast<cf*>(smem + 2 * kM + 32);
  cf* tlo = thi + kTwHi;
  load_tw(thi, tlo, a.thi, a.tlo);
  const cf* twn = reinterpret_cast<const cf*>(a.twn);
  const int sidx = blockIdx.x, f = a.s_filt[sidx], p = a.s_part[sidx];
  const int h = a.f_half[f], L = 2 * h + 1;
  const BsLowpass lo(a.f_lo[f], h), hi(a.f_hi[f], h);
  const float2 sm = a.sums[f];
  for (int m = threadIdx.x; m < kT; m += kThreads) {
    float v = 0.f;
    if (p < 0) {  // circular: tap t = -m or T - m
      const int t = m <= kT / 2 ? -m : kT - m;
      if (t >= -h && t <= h) v = bs_g(lo, hi, sm, t);
    } else {
      const int k = m == 0 ? 0 : kT - m;
      const int kk = p * kBsPart + k;
      if (k < kBsPart && kk < L) v = bs_g(lo, hi, sm, kk - h);
    }
    smem[m] = v;
  }
  __syncthreads();
  unsigned long long ph_t0 = 0;
  transform<false>(z, thi, tlo, ph_t0, 16);
  cf* H = reinterpret_cast<cf*>(a.spectra) + static_cast<int64_t>(sidx) * kHSlots;
  for (int q = threadIdx.x; q <= kM; q += kThreads) {
    const int qq = q % kM, qc = (kM - q) % kM;
    const cf zk = z[zaddr(qq)];
    const cf zc = z[zaddr(qc)];
    const cf fe = 0.5f * cf{zk.x + zc.x, zk.y - zc.y};
    const cf fo = 0.5f * cf{zk.y + zc.y, zc.x - zk.x};
    H[hslot(q)] = fe + cmul(twn[hslot(q)], fo);
  }
}

// the split, x H, inverse split on (k, M - k) pairs (as augment_kernel)
__device__ __forceinline__ void bs_multiply(cf* z, const cf* H, const cf* twn) {
  constexpr int kRest = kM / 2 / 16 + 1;
  for (int idx = opaque_tid(); idx < 16 * kRest; idx += kThreads) {
    const int c = idx / kRest;
    const int k = c + 16 * (idx - c * kRest);
    if (k > kM / 2) continue;
    const int kc = (kM - k) % kM;
    const int pz = zaddr(k);
    const cf zk = z[pz];
    const cf zc = z[zaddr(kc)];
    const cf fe = 0.5f * cf{zk.x + zc.x, zk.y - zc.y};
    const cf fo = 0.5f * cf{zk.y + zc.y, zc.x - zk.x};
    const cf wk = twn[hslot(k)];
    const cf Xk = fe + cmul(wk, fo);
    const cf Xc = cf{fe.x, -fe.y} + cmul(cf{-wk.x, wk.y}, cf{fo.x, -fo.y});
    const cf Yk = cmul(Xk, H[hslot(k)]);
    const cf Yc = cmul(Xc, H[hslot(kM - k)]);
    const cf s1 = 0.5f * cf{Yk.x + Yc.x, Yk.y - Yc.y};
    const cf d1 = 0.5f * cf{Yk.x - Yc.x, Yk.y + Yc.y};
    const cf wd = cmul(cf{wk.x, -wk.y}, d1);
    const cf s2 = 0.5f * cf{Yc.x + Yk.x, Yc.y - Yk.y};
    const cf d2 = 0.5f * cf{Yc.x - Yk.x, Yc.y + Yk.y};
    const cf wd2 = cmul(cf{-wk.x, -wk.y}, d2);
    z[pz] = s1 + cf{-wd.y, wd.x};
    if (kc != k) z[zaddr(kc)] = s2 + cf{-wd2.y, wd2.x};
  }
}

// launch 3: one block per clip (grid-strided)
__global__ void __launch_bounds__(kThreads) band_stop_kernel(BandStopArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  cf* thi = reinterpret_cast<cf*>(smem + 2 * kM + 32);
  cf* tlo = thi + kTwHi;
  float* gt = reinterpret_cast<float*>(tlo + kTwLo);  // [kBsCirc + 1] taps g[0..h]
  float* xe = gt + kBsCirc + 1;                        // [4 kBsCirc]: x[0, 2h), x[T - 2h, T)
  load_tw(thi, tlo, a.thi, a.tlo);
  const cf* twn = reinterpret_cast<const cf*>(a.twn);
  float* zf = smem;
  float* xs = a.scratch + static_cast<int64_t>(blockIdx.x) * kT;
  unsigned long long ph_t0 = 0;
  for (int64_t e = blockIdx.x; e < a.n; e += gridDim.x) {
    const int64_t clip = a.idx[e];
    const float* x = a.x + clip * a.x_stride;
    float* out = a.out + clip * a.out_stride;
    const int f = a.filt[e];
    const int h = a.f_half[f];
    const cf* H0 = reinterpret_cast<const cf*>(a.spectra) + static_cast<int64_t>(a.f_spec0[f]) * kHSlots;
    __syncthreads();  // the previous clip's readers of LDS / xs are done
    if (h <= kBsCirc) {
      // circular convolution + direct correction of the 2h edge samples
      for (int s = opaque_tid(); s < kT; s += kThreads) zf[s] = x[s];
      for (int t = threadIdx.x; t <= h; t += kThreads) gt[t] = a.taps[int64_t(f) * (kBsCirc + 1) + t];
      for (int i = threadIdx.x; i < 2 * h; i += kThreads) {
        xe[i] = x[i];
        xe[2 * kBsCirc + i] = x[kT - 2 * h + i];
      }
      __syncthreads();
      // edge sample of this thread (n < h, or n >= T - h), computed before the
      // transform overwrites nothing it needs (x edges and taps live apart from z)
      const int tid = threadIdx.x;
      float corr = 0.f;
      int n_edge = -1;
      if (tid < 2 * h) {
        const float* xb = xe + 2 * kBsCirc;  // xb[j] = x[T - 2h + j]
        if (tid < h) {  // n = tid: taps d = -h .. -n-1 wrapped to x[T + n + d]
          n_edge = tid;
          const float x0 = xe[0];
          for (int d = -h; d < -n_edge; ++d) corr += gt[-d] * (x0 - xb[2 * h + n_edge + d]);
        } else {  // n = T - 2h + tid: taps d = T - n .. h wrapped to x[n + d - T]
          n_edge = kT - 2 * h + tid;
          const float x1 = xb[2 * h - 1];
          for (int d = kT - n_edge; d <= h; ++d) corr += gt[d] * (x1 - xe[n_edge + d - kT]);
        }
      }
      transform<false>(z, thi, tlo, ph_t0, 16);
      bs_multiply(z, H0, twn);
      __syncthreads();
      transform<true>(z, thi, tlo, ph_t0, 16);
      // out = x - conv (x re-read from global: each thread reads then writes only its own samples)
      for (int s = opaque_tid(); s < kT; s += kThreads) {
        const bool edge = s < h || s >= kT - h;
        if (!edge) out[s] = x[s] - zf[s] * (1.f / kM);
      }
      if (n_edge >= 0) {
        const float xv = n_edge < h ? xe[n_edge] : xe[2 * kBsCirc + n_edge - (kT - 2 * h)];
        out[n_edge] = xv - (zf[n_edge] * (1.f / kM) + corr);
      }
      continue;
    }
    // overlap-save over partitions of kBsPart taps
    for (int s = opaque_tid(); s < kT; s += kThreads) xs[s] = x[s];
    const int parts = (2 * h + 1 + kBsPart - 1) / kBsPart;
    for (int p = 0; p < parts; ++p) {
      const cf* Hp = H0 + static_cast<int64_t>(p) * kHSlots;
      for (int b = 0; b < 2; ++b) {
        __syncthreads();  // xs published; the previous transform's readers of z are done
        const int base = b * kBsHalf + p * kBsPart - h;
        for (int j = opaque_tid(); j < kT; j += kThreads) zf[j] = xs[min(max(base + j, 0), kT - 1)];
        __syncthreads();
        transform<false>(z, thi, tlo, ph_t0, 16);
        bs_multiply(z, Hp, twn);
        __syncthreads();
        transform<true>(z, thi, tlo, ph_t0, 16);
        // y = x - sum_p c_p: each thread revisits only the samples it wrote before
        for (int i = opaque_tid(); i < kBsHalf; i += kThreads) {
          const int n = b * kBsHalf + i;
          const float c = zf[i] * (1.f / kM);
          out[n] = (p == 0 ? xs[n] : out[n]) - c;
        }
      }
    }
  }
}

// ---- colored noise --------------------------------------------------------
// torch_audiomentations AddColoredNoise (the reference's batch chain,
// augmented.py:107-113; p 0.25 per batch, snr ~ U[10, 30] dB and f_decay ~
// U[-1, 2] per clip, constants.py:128-132). Per clip:
//   w ~ N(0, 1) [T]; S = rfft(w) / linspace(1, sqrt(sr / 2), T/2 + 1)^f_decay;
//   n = irfft(S); n /= rms(n) + 1e-8; y = x + rms(x) / 10^(snr / 20) n.
// One workgroup per clip on the augment kernel's LDS transform: white noise
// into LDS, forward FFT, the real-FFT split x mask x inverse split on (k, M-k)
// pairs, inverse FFT, then rms(n) and rms(x) in one block sum and the mix.
// White noise comes from the caller (parity tests) or from a counter-based
// Box-Muller stream (seed, clip, sample): no RNG state, any grid.
struct ColoredArgs {
  const float* x;
  int64_t x_stride;
  float* out;
  int64_t out_stride;
  int64_t n_clips;
  const float* white;     // [n_clips, white_stride >= 16000] N(0,1) or NULL (generated from seed)
  int64_t white_stride;
  uint64_t seed;
  int64_t group;          // clips per white-noise vector (per_batch: the batch size)
  const float* f_decay;   // per clip
  const float* snr_db;    // per clip
  float lin_step;         // (sqrt(8000) - 1) / 8000: linspace step over the 8001 bins
  const int32_t* idx;     // NULL: every clip; else the n_entries listed clip rows (balanced launch)
  int64_t n_entries;
  const float2* thi;
  const float2* tlo;
  const float2* twn;
  // group path (clips_per_noise > 1, hbk_colored_noise_ws): colored_group_kernel writes each
  // group's coloured second (x kM1) and its rms; a clip whose f_decay equals its group's first
  // clip's mixes from it (NULL: every clip colours its own second)
  float* gbuf;            // [n_groups][kN1]
  float* grms;            // [n_groups]: rms of the coloured second, NaN where not made
  int64_t n_groups;
  int no_copy;            // hbk_augment_colored: clips this kernel does not colour are left alone
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// standard normals 2i and 2i + 1 of the stream (Box-Muller on two 24-bit
// uniforms of one hash: both the cosine and the sine branch)
__device__ __forceinline__ float2 gauss2(uint64_t seed, uint64_t i) {
  const uint64_t h = mix64(seed + 0x9E3779B97F4A7C15ull * (i + 1));
  const float u1 = (static_cast<float>(h >> 40) + 0.5f) * (1.f / 16777216.f);
  const float u2 = static_cast<float>((h >> 16) & 0xFFFFFF) * (1.f / 16777216.f);
  const float r = sqrtf(-2.f * __logf(u1));
  float sn, cs;
  __sincosf(6.283185307179586f * u2, &sn, &cs);
  return make_float2(r * cs, r * sn);
}

// ---- 8000-point complex FFT (the 16,000-sample real FFT of one second of
// noise): DIF passes 16 x 5 x 5 x 5 x 4 in LDS, twiddles W_8000^e =
// HI8[e / 100] LO8[e % 100]; frequency f = k1 + 16 k2 + 80 k3 + 400 k4 + 2000 k5
// lands at 500 k1 + 100 k2 + 20 k3 + 4 k4 + k5.
template <bool INV>
__device__ __forceinline__ void transform8(cf* z, const cf* thi, const cf* tlo) {
  if (!INV) {
    pass<Fft8000, 16, 500, 1, false>(z, thi, tlo);
    __syncthreads();
    pass<Fft8000, 5, 100, 16, false>(z, thi, tlo);
    __syncthreads();
    pass<Fft8000, 5, 20, 80, false>(z, thi, tlo);
    __syncthreads();
    pass<Fft8000, 5, 4, 400, false>(z, thi, tlo);
    __syncthreads();
    pass<Fft8000, 4, 1, 0, false>(z, thi, tlo);
    __syncthreads();
  } else {
    pass<Fft8000, 4, 1, 0, true>(z, thi, tlo);
    __syncthreads();
    pass<Fft8000, 5, 4, 400, true>(z, thi, tlo);
    __syncthreads();
    pass<Fft8000, 5, 20, 80, true>(z, thi, tlo);
    __syncthreads();
    pass<Fft8000, 5, 100, 16, true>(z, thi, tlo);
    __syncthreads();
    pass<Fft8000, 16, 500, 1, true>(z, thi, tlo);
    __syncthreads();
  }
}

__device__ __forceinline__ int zaddr8(int f) {
  const int k1 = f & 15, r = f >> 4;  // r = k2 + 5 k3 + 25 k4 + 125 k5
  const int k2 = r % 5, r2 = r / 5;
  const int k3 = r2 % 5, r3 = r2 / 5;
  const int k4 = r3 % 5, k5 = r3 / 5;
  return 500 * k1 + 100 * k2 + 20 * k3 + 4 * k4 + k5;
}

// 1) + 2): group grp's second of white noise -> LDS, forward FFT, the real-FFT split x the
// 1 / linspace^f_decay mask x inverse split, inverse FFT: zf = the coloured second x kM1
// (natural order). Entered and left at a barrier.
__device__ __forceinline__ void colored_second(const ColoredArgs& a, cf* z, const cf* thi, const cf* tlo, int tid,
                                               int64_t grp, float fd) {
  float* zf = reinterpret_cast<float*>(z);
  // 1) one second of white noise -> LDS (the previous clip's readers finished at its last barrier)
  if (a.white) {
    const float* w = a.white + grp * a.white_stride;
    for (int s = tid; s < kN1; s += kThreads) zf[s] = w[s];
  } else {
    for (int q = tid; q < kN1 / 2; q += kThreads) {
      const float2 g = gauss2(a.seed, static_cast<uint64_t>(grp) * (kN1 / 2) + q);
      *reinterpret_cast<float2*>(zf + 2 * q) = g;
    }
  }
  __syncthreads();
  transform8<false>(z, thi, tlo);
  // 2) X = split(Z); Y = X / lin^f_decay; Z' = inverse split(Y), pairs (k, M - k), k <= M / 2
  for (int k = tid; k <= kM1 / 2; k += kThreads) {
    const int kc = (kM1 - k) % kM1;
    const int p = zaddr8(k), pc = zaddr8(kc);
    const cf zk = z[p];
    const cf zc = z[pc];
    const cf fe = 0.5f * cf{zk.x + zc.x, zk.y - zc.y};
    const cf fo = 0.5f * cf{zk.y + zc.y, zc.x - zk.x};
    const cf wk = cf{a.twn[k].x, a.twn[k].y};  // W_16000^k
    const float mk = exp2f(-fd * __log2f(fmaf(a.lin_step, static_cast<float>(k), 1.f)));
    const float mc = exp2f(-fd * __log2f(fmaf(a.lin_step, static_cast<float>(kM1 - k), 1.f)));  // bin M - k
    const cf Yk = mk * (fe + cmul(wk, fo));
    const cf Yc = mc * (cf{fe.x, -fe.y} + cmul(cf{-wk.x, wk.y}, cf{fo.x, -fo.y}));
    const cf s1 = 0.5f * cf{Yk.x + Yc.x, Yk.y - Yc.y};
    const cf d1 = 0.5f * cf{Yk.x - Yc.x, Yk.y + Yc.y};
    const cf wd = cmul(cf{wk.x, -wk.y}, d1);
    const cf s2 = 0.5f * cf{Yc.x + Yk.x, Yc.y - Yk.y};
    const cf d2 = 0.5f * cf{Yc.x - Yk.x, Yc.y + Yk.y};
    const cf wd2 = cmul(cf{-wk.x, -wk.y}, d2);
    z[p] = s1 + cf{-wd.y, wd.x};
    if (kc != k) z[pc] = s2 + cf{-wd2.y, wd2.x};
  }
  __syncthreads();
  transform8<true>(z, thi, tlo);  // natural order, x kM1
}

// torch_audiomentations AddColoredNoise (per clip, white noise w of ONE second):
//   n1 = irfft(rfft(w[:16000]) / linspace(1, sqrt(sr/2), 8001)^f_decay)      (16,000)
//   n1 /= rms(n1) + 1e-8;  noise[t] = n1[t mod 16000], t < T (tiled, not renormalised)
//   y = x + rms(x) / 10^(snr/20) noise
// The 16,000 noise samples as 8000 complex pairs in LDS, forward FFT, the
// real-FFT split x mask x inverse split on (k, M - k) pairs, inverse FFT.
__global__ void __launch_bounds__(kThreads) colored_noise_kernel(ColoredArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cf* z = reinterpret_cast<cf*>(smem);                 // kM1 complex
  float* red = smem + 2 * kM1;                         // 32 floats
  cf* thi = reinterpret_cast<cf*>(smem + 2 * kM1 + 32);
  cf* tlo = thi + kTw8Hi;
  for (int i = threadIdx.x; i < kTw8Hi; i += kThreads) thi[i] = cf{a.thi[i].x, a.thi[i].y};
  for (int i = threadIdx.x; i < kTw8Lo; i += kThreads) tlo[i] = cf{a.tlo[i].x, a.tlo[i].y};
  float* zf = smem;
  constexpr int kPer = (kT + kThreads - 1) / kThreads;
  const int64_t n_iter = a.idx ? a.n_entries : a.n_clips;
  for (int64_t e = blockIdx.x; e < n_iter; e += gridDim.x) {
    const int64_t clip = a.idx ? a.idx[e] : e;
    const int tid = opaque_tid();
    const float snr = a.snr_db[clip];
    if (snr != snr) {  // NaN: this clip's batch drew no colored noise (uniform per block)
      if (!a.no_copy && (a.out != a.x || a.out_stride != a.x_stride))
        copy_clip(a.x + clip * a.x_stride, a.out + clip * a.out_stride, tid);
      continue;
    }
    const int64_t grp = clip / a.group;  // clips of one batch share the noise vector (per_batch)
    float rms_g = __builtin_nanf("");
    if (a.grms && a.f_decay[clip] == a.f_decay[grp * a.group]) rms_g = a.grms[grp];  // uniform per block
    if (rms_g == rms_g) continue;  // the group's coloured second is made: colored_mix_kernel mixes it
    colored_second(a, z, thi, tlo, tid, grp, a.f_decay[clip]);
    // 3) rms(n1) over 16,000 and rms(x) over T in one block sum; tile and mix
    const float* x = a.x + clip * a.x_stride;
    float xr[kPer];
    float ex = 0.f, en = 0.f;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int s = tid + u * kThreads;
      xr[u] = 0.f;
      if (s < kT) {
        xr[u] = x[s];
        ex = fmaf(xr[u], xr[u], ex);
      }
      if (s < kN1) {
        const float nv = zf[s] * (1.f / kM1);
        en += nv * nv;
      }
    }
    block_sum2(ex, en, red);
    const float rms_x = sqrtf(ex / kT), rms_n = sqrtf(en / kN1);
    const float scale = rms_x / powf(10.f, snr / 20.f) / (rms_n + 1e-8f) * (1.f / kM1);
    float* out = a.out + clip * a.out_stride;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int s = tid + u * kThreads;
      if (s < kT) out[s] = fmaf(scale, zf[s < kN1 ? s : s - kN1], xr[u]);
    }
    __syncthreads();  // zf is rewritten by the next clip
  }
}

// The coloured second of every group whose first clip draws noise (clips_per_noise > 1:
// per_batch mode shares the white noise and, in the reference's chain, f_decay across the
// batch), with its rms computed exactly as the clip kernel does.
__global__ void __launch_bounds__(kThreads) colored_group_kernel(ColoredArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cf* z = reinterpret_cast<cf*>(smem);
  float* red = smem + 2 * kM1;
  cf* thi = reinterpret_cast<cf*>(smem + 2 * kM1 + 32);
  cf* tlo = thi + kTw8Hi;
  for (int i = threadIdx.x; i < kTw8Hi; i += kThreads) thi[i] = cf{a.thi[i].x, a.thi[i].y};
  for (int i = threadIdx.x; i < kTw8Lo; i += kThreads) tlo[i] = cf{a.tlo[i].x, a.tlo[i].y};
  const float* zf = smem;
  constexpr int kPer = (kT + kThreads - 1) / kThreads;
  for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const int tid = opaque_tid();
    const int64_t c0 = g * a.group;
    if (a.snr_db[c0] != a.snr_db[c0]) {  // the group's first clip draws no noise: not made
      if (tid == 0) a.grms[g] = __builtin_nanf("");
      continue;
    }
    __syncthreads();  // tables loaded / the previous group's readers of zf are done
    colored_second(a, z, thi, tlo, tid, g, a.f_decay[c0]);
    float ex = 0.f, en = 0.f;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int s = tid + u * kThreads;
      if (s < kN1) {
        const float nv = zf[s] * (1.f / kM1);
        en += nv * nv;
      }
    }
    block_sum2(ex, en, red);
    float* gb = a.gbuf + g * kN1;
    for (int s = tid; s < kN1; s += kThreads) gb[s] = zf[s];
    if (tid == 0) a.grms[g] = sqrtf(en / kN1);
    __syncthreads();
  }
}

// The clips of made groups (colored_group_kernel): rms(x) and the mix, from the group's
// coloured second in global memory (L2-resident across its clips). The same per-thread
// order and block sum as colored_noise_kernel, so the result is bit-identical; no
// transform LDS, so two 1024-thread blocks (two clips in flight) per CU.
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8))) colored_mix_kernel(ColoredArgs a) {
  __shared__ float red[32];
  constexpr int kPer = (kT + kThreads - 1) / kThreads;
  const int64_t n_iter = a.idx ? a.n_entries : a.n_clips;
  for (int64_t e = blockIdx.x; e < n_iter; e += gridDim.x) {
    const int64_t clip = a.idx ? a.idx[e] : e;
    const int tid = opaque_tid();
    const float snr = a.snr_db[clip];
    const int64_t grp = clip / a.group;
    float rms_g = __builtin_nanf("");
    if (snr == snr && a.f_decay[clip] == a.f_decay[grp * a.group]) rms_g = a.grms[grp];
    if (rms_g != rms_g) continue;  // uniform per block: colored_noise_kernel's clip
    const float* gb = a.gbuf + grp * kN1;
    const float* x = a.x + clip * a.x_stride;
    // two passes over x (the second from the cache): nothing is held across the block sum,
    // so the kernel fits 64 VGPRs without spills; ex in colored_noise_kernel's order
    float ex = 0.f, en = 0.f;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int s = tid + u * kThreads;
      if (s < kT) {  // 32-bit byte offsets on uniform bases
        const float v = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(x) + (static_cast<uint32_t>(s) << 2));
        ex = fmaf(v, v, ex);
      }
    }
    block_sum2(ex, en, red);
    const float rms_x = sqrtf(ex / kT);
    const float scale = rms_x / powf(10.f, snr / 20.f) / (rms_g + 1e-8f) * (1.f / kM1);
    float* out = a.out + clip * a.out_stride;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int s = tid + u * kThreads;
      if (s < kT) {
        const int sn = s < kN1 ? s : s - kN1;
        const float xv = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(x) + (static_cast<uint32_t>(s) << 2));
        const float nv =
            *reinterpret_cast<const float*>(reinterpret_cast<const char*>(gb) + (static_cast<uint32_t>(sn) << 2));
        *reinterpret_cast<float*>(reinterpret_cast<char*>(out) + (static_cast<uint32_t>(s) << 2)) = fmaf(scale, nv, xv);
      }
    }
    __syncthreads();  // red is reused by the next clip
  }
}

}  // namespace

#ifdef HBK_PHASE_TIMING
int pv_phase_take(unsigned long long* out);  // hbk_pitch.hip
#endif

}  // namespace hbk

struct hbk_reverb_plan {
  void* tables = nullptr;  // one allocation (reverb_tables); the six below point into it
  const float2* thi = nullptr;
  const float2* tlo = nullptr;
  const float2* twn = nullptr;
  const float2* thi8 = nullptr;  // colored noise: W_8000^(100 h), W_8000^l, W_16000^k (k <= 4000)
  const float2* tlo8 = nullptr;
  const float2* twn16 = nullptr;
  // placement on first touch: the source view hbk_augment / hbk_augment_colored read their
  // clips through (hbk_reverb_plan_set_source; pre NULL: none)
  hbk::SrcView view = {nullptr, 0, nullptr, nullptr};
};

extern "C" {

int hbk_reverb_plan_create(int64_t T, hbk_reverb_plan** plan) {
  using namespace hbk;
  if (!plan) return arg_error("plan is NULL");
  *plan = nullptr;
  if (T != kT) {
    set_error("hbk: reverb supports clips of %d samples (1.44 s @ 16 kHz), got %lld", kT, (long long)T);
    return HBK_ERR_UNSUPPORTED;
  }
  const ReverbTables t = reverb_tables();
  auto* p = new hbk_reverb_plan();
  hipError_t e;
  if ((e = hipMalloc(&p->tables, t.bytes())) != hipSuccess ||
      (e = hipMemcpy(p->tables, t.host.data(), t.bytes(), hipMemcpyHostToDevice)) != hipSuccess) {
    hbk_reverb_plan_destroy(p);
    return hip_error(e, "reverb plan tables");
  }
  auto table = [&](ReverbTable i) {
    return reinterpret_cast<const float2*>(static_cast<const unsigned char*>(p->tables) + t.off[i]);
  };
  p->thi = table(kTabHi), p->tlo = table(kTabLo), p->twn = table(kTabN);
  p->thi8 = table(kTabHi8), p->tlo8 = table(kTabLo8), p->twn16 = table(kTabN16);
  // > 64 KB of dynamic LDS needs the opt-in (a per-device attribute: set with every plan)
  const struct {
    const void* kernel;
    size_t lds;
  } opt_in[] = {
      {reinterpret_cast<const void*>(augment_kernel), kAugLds},
      {reinterpret_cast<const void*>(spectrum_kernel), kAugLds},
      {reinterpret_cast<const void*>(band_stop_kernel), kBandStopLds},
      {reinterpret_cast<const void*>(band_stop_spectrum_kernel), kAugLds},
      {reinterpret_cast<const void*>(colored_noise_kernel), kColoredLds},
      {reinterpret_cast<const void*>(colored_group_kernel), kColoredLds},
  };
  for (const auto& o : opt_in)
    if ((e = hipFuncSetAttribute(o.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(o.lds))) != hipSuccess) {
      hbk_reverb_plan_destroy(p);
      return hip_error(e, "hipFuncSetAttribute(augment LDS)");
    }
  *plan = p;
  return HBK_OK;
}

int hbk_reverb_plan_destroy(hbk_reverb_plan* p) {
  if (!p) return HBK_OK;
  (void)hipFree(p->tables);
  delete p;
  return HBK_OK;
}

int hbk_reverb_plan_set_source(hbk_reverb_plan* p, const float* src, int64_t src_stride, const int32_t* src_len,
                               const int32_t* src_pre) {
  if (!p) return hbk::arg_error("plan is NULL");
  return hbk::src_view(src, src_stride, src_len, src_pre, p->view);
}

int hbk_reverb_spectrum(const hbk_reverb_plan* p, const float* kernels, int64_t n_kernels, int64_t stride,
                        float* spectra, void* stream) {
  using namespace hbk;
  if (!p) return arg_error("plan is NULL");
  if (n_kernels < 0) return arg_error("negative n_kernels");
  if (n_kernels == 0) return HBK_OK;
  if (!kernels || !spectra) return arg_error("NULL pointer");
  if (stride < kT) return arg_error("kernel stride < 23040");
  hipLaunchKernelGGL(spectrum_kernel, dim3(unsigned(n_kernels)), dim3(kThreads), kAugLds, as_stream(stream),
                     kernels, stride, reinterpret_cast<float2*>(spectra), p->thi, p->tlo, p->twn);
  HBK_LAUNCH_CHECK("spectrum_kernel");
  return HBK_OK;
}

static int augment_args(const hbk_reverb_plan* p, const float* x, int64_t n_clips, int64_t x_stride,
                        const float* noise_ring, int64_t ring_len, const int64_t* noise_off, const float* snr_db,
                        const float* spectra, const int32_t* spec_idx, const float* gain, float* out,
                        int64_t out_stride, hbk::AugArgs& a) {
  using namespace hbk;
  if (!p) return arg_error("plan is NULL");
  if (n_clips < 0) return arg_error("negative n_clips");
  if (!x || !out || !noise_off || !snr_db || !spec_idx) return arg_error("NULL pointer");
  if (x_stride < kT || out_stride < kT) return arg_error("stride < 23040");
  if (!noise_ring && ring_len > 0) return arg_error("noise ring is NULL");
  if (ring_len >= (int64_t(1) << 30)) return arg_error("noise ring longer than 2^30 samples");
  a = AugArgs{};
  a.x = x;
  a.x_stride = x_stride;
  a.out = out;
  a.out_stride = out_stride;
  a.n_clips = n_clips;
  a.ring = noise_ring;
  a.ring_len = ring_len;
  a.noise_off = noise_off;
  a.snr_db = snr_db;
  a.spectra = reinterpret_cast<const float2*>(spectra);
  a.spec_idx = spec_idx;
  a.gain = gain;
  a.thi = p->thi;
  a.tlo = p->tlo;
  a.twn = p->twn;
  a.view = p->view;
  return HBK_OK;
}

static void augment_launch(const hbk::AugArgs& a, void* stream) {
  using namespace hbk;
  const int64_t blocks = std::min<int64_t>(a.n_clips, persistent_blocks(1, stream));
  hipLaunchKernelGGL(augment_kernel, dim3(unsigned(blocks)), dim3(kThreads), kAugLds, as_stream(stream), a);
}

int hbk_augment(const hbk_reverb_plan* p, const float* x, int64_t n_clips, int64_t x_stride,
                const float* noise_ring, int64_t ring_len, const int64_t* noise_off, const float* snr_db,
                const float* spectra, const int32_t* spec_idx, const float* gain, float* out,
                int64_t out_stride, void* stream) {
  using namespace hbk;
  if (n_clips == 0 && p) return HBK_OK;
  AugArgs a;
  const int st = augment_args(p, x, n_clips, x_stride, noise_ring, ring_len, noise_off, snr_db, spectra, spec_idx,
                              gain, out, out_stride, a);
  if (st != HBK_OK) return st;
  augment_launch(a, stream);
  HBK_LAUNCH_CHECK("augment_kernel");
  return HBK_OK;
}

int64_t hbk_colored_noise_workspace_size(int64_t n_clips, int64_t clips_per_noise) {
  return hbk::colored_layout(n_clips, clips_per_noise).total;
}

int hbk_colored_noise(const hbk_reverb_plan* p, const float* x, int64_t n_clips, int64_t x_stride,
                      const float* white, int64_t white_stride, uint64_t seed, int64_t clips_per_noise,
                      const float* f_decay, const float* snr_db, float sample_rate, const int32_t* idx,
                      int64_t n_entries, float* out, int64_t out_stride, void* stream) {
  return hbk_colored_noise_ws(p, x, n_clips, x_stride, white, white_stride, seed, clips_per_noise, f_decay, snr_db,
                              sample_rate, idx, n_entries, out, out_stride, nullptr, 0, stream);
}

static int colored_args(const hbk_reverb_plan* p, const float* x, int64_t n_clips, int64_t x_stride,
                        const float* white, int64_t white_stride, uint64_t seed, int64_t clips_per_noise,
                        const float* f_decay, const float* snr_db, float sample_rate, const int32_t* idx,
                        int64_t n_entries, float* out, int64_t out_stride, void* workspace, int64_t workspace_bytes,
                        hbk::ColoredArgs& a) {
  using namespace hbk;
  if (!p) return arg_error("plan is NULL");
  if (n_clips < 0) return arg_error("negative n_clips");
  if (!x || !out || !f_decay || !snr_db) return arg_error("NULL pointer");
  if (x_stride < kT || out_stride < kT) return arg_error("stride < 23040");
  if (white && white_stride < kN1) return arg_error("white_stride < 16000");
  if (clips_per_noise < 1) return arg_error("clips_per_noise < 1");
  if (idx && n_entries < 0) return arg_error("negative n_entries");
  if (sample_rate != float(kN1)) {
    set_error("hbk: colored noise is generated at 16 kHz (one second = 16000 samples), got %g", double(sample_rate));
    return HBK_ERR_UNSUPPORTED;
  }
  a = ColoredArgs{};
  a.x = x;
  a.x_stride = x_stride;
  a.out = out;
  a.out_stride = out_stride;
  a.n_clips = n_clips;
  a.white = white;
  a.white_stride = white_stride;
  a.seed = seed;
  a.group = clips_per_noise;
  a.f_decay = f_decay;
  a.snr_db = snr_db;
  a.lin_step = static_cast<float>((std::sqrt(double(kN1) / 2.0) - 1.0) / double(kM1));
  a.idx = idx;
  a.n_entries = idx ? n_entries : n_clips;
  a.thi = p->thi8;
  a.tlo = p->tlo8;
  a.twn = p->twn16;
  a.gbuf = a.grms = nullptr;
  a.n_groups = 0;
  a.no_copy = 0;
  const ColoredLayout w = colored_layout(n_clips, clips_per_noise);
  if (workspace && w.total > 0) {
    if (workspace_bytes < w.total) return arg_error("workspace too small (hbk_colored_noise_workspace_size)");
    unsigned char* base = static_cast<unsigned char*>(workspace);
    a.n_groups = w.groups;
    a.gbuf = reinterpret_cast<float*>(base + w.gbuf);
    a.grms = reinterpret_cast<float*>(base + w.grms);
  }
  return HBK_OK;
}

static void colored_group_launch(const hbk::ColoredArgs& a, void* stream) {
  using namespace hbk;
  const int64_t gblocks = std::min<int64_t>(a.n_groups, persistent_blocks(1, stream));
  hipLaunchKernelGGL(colored_group_kernel, dim3(unsigned(gblocks)), dim3(kThreads), kColoredLds, as_stream(stream), a);
}

static void colored_clip_launch(const hbk::ColoredArgs& a, void* stream) {
  using namespace hbk;
  const int64_t blocks = std::min<int64_t>(a.n_entries, persistent_blocks(1, stream));
  hipLaunchKernelGGL(colored_noise_kernel, dim3(unsigned(blocks)), dim3(kThreads), kColoredLds, as_stream(stream), a);
}

int hbk_colored_noise_ws(const hbk_reverb_plan* p, const float* x, int64_t n_clips, int64_t x_stride,
                         const float* white, int64_t white_stride, uint64_t seed, int64_t clips_per_noise,
                         const float* f_decay, const float* snr_db, float sample_rate, const int32_t* idx,
                         int64_t n_entries, float* out, int64_t out_stride, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  using namespace hbk;
  if (n_clips == 0 && p) return HBK_OK;
  ColoredArgs a;
  const int st = colored_args(p, x, n_clips, x_stride, white, white_stride, seed, clips_per_noise, f_decay, snr_db,
                              sample_rate, idx, n_entries, out, out_stride, workspace, workspace_bytes, a);
  if (st != HBK_OK) return st;
  if (a.n_entries <= 0) return HBK_OK;
  if (a.grms) {
    colored_group_launch(a, stream);
    HBK_LAUNCH_CHECK("colored_group_kernel");
    const int64_t mblocks = std::min<int64_t>(a.n_entries, persistent_blocks(2, stream));
    hipLaunchKernelGGL(colored_mix_kernel, dim3(unsigned(mblocks)), dim3(kThreads), 0, as_stream(stream), a);
    HBK_LAUNCH_CHECK("colored_mix_kernel");
  }
  colored_clip_launch(a, stream);
  HBK_LAUNCH_CHECK("colored_noise_kernel");
  return HBK_OK;
}

int hbk_augment_colored(const hbk_reverb_plan* p, const float* x, int64_t n_clips, int64_t x_stride,
                        const float* noise_ring, int64_t ring_len, const int64_t* noise_off, const float* snr_db,
                        const float* spectra, const int32_t* spec_idx, const float* gain, const float* white,
                        int64_t white_stride, uint64_t seed, int64_t clips_per_noise, const float* c_f_decay,
                        const float* c_snr_db, float sample_rate, const int32_t* c_idx, int64_t c_n_entries,
                        float* out, int64_t out_stride, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace hbk;
  if (n_clips == 0 && p) return HBK_OK;
  AugArgs a;
  int st = augment_args(p, x, n_clips, x_stride, noise_ring, ring_len, noise_off, snr_db, spectra, spec_idx, gain,
                        out, out_stride, a);
  if (st != HBK_OK) return st;
  ColoredArgs c;
  st = colored_args(p, x, n_clips, x_stride, white, white_stride, seed, clips_per_noise, c_f_decay, c_snr_db,
                    sample_rate, c_idx, c_n_entries, out, out_stride, workspace, workspace_bytes, c);
  if (st != HBK_OK) return st;
  if (out != x && out + n_clips * out_stride > x && x + n_clips * x_stride > out)
    return arg_error("out overlaps x without being x");
  c.no_copy = 1;
  if (c.grms) {
    colored_group_launch(c, stream);
    HBK_LAUNCH_CHECK("colored_group_kernel");
  }
  if (c.n_entries > 0) {  // the clips the group path does not cover, coloured into out
    colored_clip_launch(c, stream);
    HBK_LAUNCH_CHECK("colored_noise_kernel");
  }
  a.c_snr = c_snr_db;
  a.c_fd = c_f_decay;
  a.c_group = clips_per_noise;
  a.c_gbuf = c.gbuf;
  a.c_grms = c.grms;
  augment_launch(a, stream);
  HBK_LAUNCH_CHECK("augment_kernel");
  return HBK_OK;
}

int64_t hbk_band_stop_workspace_size(int64_t n, int32_t n_filters, int32_t n_spectra, void* stream) {
  using namespace hbk;
  if (n <= 0) return 0;
  return band_stop_layout(n, n_filters, n_spectra, std::min<int64_t>(n, persistent_blocks(1, stream))).total;
}

int hbk_band_stop(const hbk_reverb_plan* p, const float* x, int64_t x_stride, int64_t n, const int32_t* idx,
                  const int32_t* filt, int32_t n_filters, const float* f_lo, const float* f_hi,
                  const int32_t* f_half, const int32_t* f_spec0, int32_t n_spectra, const int32_t* s_filt,
                  const int32_t* s_part, float* out, int64_t out_stride, void* workspace, int64_t workspace_bytes,
                  void* stream) {
  using namespace hbk;
  if (!p) return arg_error("plan is NULL");
  if (n < 0 || n_filters < 0 || n_spectra < 0) return arg_error("negative count");
  if (n == 0) return HBK_OK;
  if (n_filters == 0 || n_spectra < n_filters) return arg_error("every filter needs at least one spectrum");
  if (!x || !idx || !filt || !f_lo || !f_hi || !f_half || !f_spec0 || !s_filt || !s_part || !out || !workspace)
    return arg_error("NULL pointer");
  if (x_stride < kT || out_stride < kT) return arg_error("stride < 23040");
  const int64_t blocks = std::min<int64_t>(n, persistent_blocks(1, stream));
  const BandStopLayout off = band_stop_layout(n, n_filters, n_spectra, blocks);
  if (workspace_bytes < off.total) return arg_error("workspace too small (hbk_band_stop_workspace_size)");
  BandStopArgs a;
  a.x = x;
  a.x_stride = x_stride;
  a.out = out;
  a.out_stride = out_stride;
  a.n = n;
  a.idx = idx;
  a.filt = filt;
  a.n_filters = n_filters;
  a.f_lo = f_lo;
  a.f_hi = f_hi;
  a.f_half = f_half;
  a.f_spec0 = f_spec0;
  a.n_spectra = n_spectra;
  a.s_filt = s_filt;
  a.s_part = s_part;
  unsigned char* w = static_cast<unsigned char*>(workspace);
  a.sums = reinterpret_cast<float2*>(w + off.sums);
  a.taps = reinterpret_cast<float*>(w + off.taps);
  a.spectra = reinterpret_cast<float2*>(w + off.spectra);
  a.scratch = reinterpret_cast<float*>(w + off.scratch);
  a.thi = p->thi;
  a.tlo = p->tlo;
  a.twn = p->twn;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(band_stop_sums_kernel, dim3(unsigned(n_filters)), dim3(kThreads), 0, st, a);
  HBK_LAUNCH_CHECK("band_stop_sums_kernel");
  hipLaunchKernelGGL(band_stop_spectrum_kernel, dim3(unsigned(n_spectra)), dim3(kThreads), kAugLds, st, a);
  HBK_LAUNCH_CHECK("band_stop_spectrum_kernel");
  hipLaunchKernelGGL(band_stop_kernel, dim3(unsigned(blocks)), dim3(kThreads), kBandStopLds, st, a);
  HBK_LAUNCH_CHECK("band_stop_kernel");
  return HBK_OK;
}

}  // extern "C"

#ifdef HBK_PHASE_TIMING
extern "C" int hbk_debug_aug_phase(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hbk::g_aug_phase), sizeof(unsigned long long) * 32) != hipSuccess)
    return -2;
  unsigned long long z[32] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(hbk::g_aug_phase), z, sizeof(z));
  unsigned long long pv[5];  // the vocoder's phases (hbk_pitch.hip): slots 16 ..
  if (hbk::pv_phase_take(pv) != 0) return -2;
  for (int i = 0; i < 5; ++i) out[16 + i] += pv[i];
  return 0;
}
#endif
