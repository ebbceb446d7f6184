// The fused classifier's evaluation passes for gfx950 (default architecture, as
// the train step of hbk_mlp_fused.hip): kv_prep (the pass's W' planes), kv_gemm
// (the input GEMM and the rest of the network per row tile, reduced to prediction
// counts) and kv_finish (rates and the dynamic negative weight). The weight cache
// is the train step's (k0_wsplit_kernel in hbk_mlp_fused.hip, reached through
// mlp_wcache_fill); the shared device helpers are in hbk_mlp_dev.h. The passes'
// entry points (hbk_mlp_eval_*), argument checks included, are at the end of this
// file; nothing of it is called from another unit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hbk_common.h"
#include "hbk_mlp_dev.h"
#include "hbk_mlp_internal.h"
#include "hbk_mlp_plan.h"

namespace hbk {
namespace {

// ---------------------------------------------------------- evaluation ----
// The validation / testing passes of train_epoch (trainer.py:496-566): a
// forward with input dropout over hundreds of thousands of rows (the default
// validation pass is 500 batches of 50 + 1,000 rows, the testing pass 500 of
// 50 + 50), reduced to prediction counts. The input layer is a real GEMM here
// ([rows, 1536] x [1536, 128]), so it gets a throughput kernel of its own,
// kv_gemm: the LayerNorm is folded into the GEMM's epilogue,
//   (LN(x) g + b) W^T = rs (x W'^T - mu c1) + c0,  W' = W o g (columns scaled),
//   c1[n] = sum_k W'[n][k],  c0[n] = sum_k b[k] W[n][k],
// so the product runs on the raw (dropped-out) rows: an f16 pool row is exact
// in f16 (its hi part; no lo), two products per 32-deep block instead of
// three. mu / rs come from the same loaded values (per-lane float sums of 8,
// accumulated in double). W' (f16 hi / lo planes of 16 W') is staged through
// LDS in 64-deep chunks, double-buffered, shared by 8 waves of 32 rows each;
// the rows stream from HBM straight into MFMA A fragments, prefetched two
// chunks ahead. The pre-bias HG0 rows go to a slab that k2_rows_kernel
// <false> (the inference chain, with its counters) reads as its one K-split.
constexpr int kKvKC = 64, kKvChunks = kD / kKvKC;
constexpr int kKvMaxSeg = 4;
// one pool of an evaluation launch (mlp_eval_count_multi: several pools of one dtype in one launch)
struct EvalSeg {
  const void* pool;
  int64_t n_pool, rows, r0;
  uint64_t seed;
  float* counts;
  int label;
};
struct KvArgs {
  const void* pool;      // f32 or f16 rows of 1536
  int64_t n_pool;
  const int32_t* idx;    // row r -> pool row idx[r]; NULL: r0 + r modulo n_pool
  int64_t rows, r0;      // this launch's rows; r0 = their first index in the pass (dropout counter)
  const _Float16* wq;    // [2][128][1536] hi / lo planes of 16 W'
  const float* c0;
  const float* c1;
  float drop_p;
  uint64_t seed;
  // the rest of the network (parameter offsets; weight cache planes as k2 reads them)
  const float* P;
  int64_t b_hg[kMaxG], b_o[kMaxG], w_o[kMaxG], ln_g[kMaxG], ln_b[kMaxG];
  const _Float16* wc;
  int64_t c_o[kMaxG], c_hg[kMaxG];
  float act_thr;
  float* counts;  // [4]: counts[2 label] += #(p >= act_thr), counts[2 label + 1] += #(p > act_thr)
  int label;
  float* prob;    // [rows] or NULL
  // several pools in one launch (hbk_mlp_eval_count_multi; nseg = 0: the fields above): workgroup
  // b of segment s = the first segment with b < seg_tile0[s + 1] takes pool s's tile b - seg_tile0[s]
  int nseg;
  int seg_tile0[kKvMaxSeg + 1];
  const void* seg_pool[kKvMaxSeg];
  int64_t seg_npool[kKvMaxSeg], seg_rows[kKvMaxSeg], seg_r0[kKvMaxSeg];
  uint64_t seg_seed[kKvMaxSeg];
  float* seg_counts[kKvMaxSeg];
  int seg_label[kKvMaxSeg];
  int lap_tiles;  // the lap form (kLap > 0): workgroups per lap set, ceil(n_pool / 128); rows = whole sets
};

__global__ void __launch_bounds__(256) kv_prep_kernel(const float* __restrict__ P, int64_t w0, int64_t g_in,
                                                      int64_t b_in, _Float16* __restrict__ wq, float* c0,
                                                      float* c1) {
  __shared__ double red[2][4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* W = P + w0 + int64_t(n) * kD;
  double s0 = 0.0, s1 = 0.0;
  for (int k = 2 * tid; k < kD; k += 512) {
    const float wa = W[k], wb = W[k + 1];
    const float ga = wa * P[g_in + k], gb = wb * P[g_in + k + 1];
    uint32_t hi, lo;
    split_pair(16.f * ga, 16.f * gb, hi, lo);
    *reinterpret_cast<uint32_t*>(wq + int64_t(n) * kD + k) = hi;
    *reinterpret_cast<uint32_t*>(wq + int64_t(kH2) * kD + int64_t(n) * kD + k) = lo;
    s1 += double(ga) + double(gb);
    s0 += double(P[b_in + k]) * wa + double(P[b_in + k + 1]) * wb;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64);
    s1 += __shfl_xor(s1, o, 64);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = s0;
    red[1][tid >> 6] = s1;
  }
  __syncthreads();
  if (tid == 0) {
    c0[n] = static_cast<float>((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
    c1[n] = static_cast<float>((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
  }
}

#ifndef HBK_KV_ABLATE
#define HBK_KV_ABLATE 0  // profiling builds: 1 skips the network phase, 2 the dropout mask
#endif
// The streamed rows are read once: non-temporal loads (HBK_KV_NT, default on)
// keep them from evicting W', which every tile re-reads, from the XCD's L2.
#ifndef HBK_KV_NT
#define HBK_KV_NT 1
#endif
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 load_rows4(const uint4* p) {
#if HBK_KV_NT
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return uint4{v[0], v[1], v[2], v[3]};
#else
  return *p;
#endif
}

// kF16: the rows are f16 (exact in hi); else f32 (split hi / lo).
// W' chunks reach LDS by global->LDS DMA (global_load_lds_dwordx4: no register
// staging, so no spills at 8 waves x ~240 VGPRs), issued two chunks ahead. The
// DMA writes a wave's 64 x 16 B contiguously, so the image is unpadded
// [plane][n][64 halves] rows with the 16-B pieces XOR-swizzled by (n >> 1) & 7
// on the SOURCE address (the B-fragment reads of 16 lanes then hit 16
// distinct 4-bank groups). The chunk's barrier waits with a counted vmcnt
// (the DMA retired, the next rows' loads still in flight) and a raw s_barrier:
// __syncthreads() would emit vmcnt(0) and drain the row prefetch.
constexpr int kKvPiece = 8;  // 16-B pieces per 64-deep row of a chunk
__device__ __forceinline__ int kv_swz(int n) { return (n >> 1) & 7; }
constexpr int kNetWLd = 104, kAld = 100;  // LDS row strides: weight halves (K <= 96), activation floats
// W: waves per workgroup, 8 (f16 rows: two 16-row tiles per wave) or 16 (one tile per wave:
// twice the waves per CU to hide the stream's latency, at most 128 VGPRs each)
// kLap = 2, the lap form (f16 pools read in order, 8 waves): a pass that reads its pool several times
// over evaluates every pool row once per lap, and only the dropout mask (a hash of the row's index in the
// pass) differs between the laps. So a wave's two tiles are two laps of the SAME 16 pool rows: one load
// of the raw rows per chunk, masked and converted once per lap: 1.5 + 3 KB per row evaluation against
// 3 + 3 KB. The launch covers whole lap sets: set q is the row evaluations [2 q n_pool, 2 (q + 1) n_pool)
// of the launch, its workgroup t the pool rows (r0 + 16 W t ..) % n_pool (a wrap inside a tile is per
// lane; the last tile's rows past n_pool are dead). Every row evaluation keeps its values, chunk order
// and MFMA sequence, so prob and the counts are those of the plain form, bit for bit. (Four laps per wave
// need 128 accumulator registers of the 256: hipcc spills inside the chunk loop)
template <bool kF16, int NG, int W, int kLap = 0>
__global__ void __launch_bounds__(64 * W) kv_gemm_kernel(KvArgs a0) {
  static_assert(kLap == 0 || (kF16 && W == 8 && kLap == 2), "the lap form: f16 rows, 8 waves of two laps");
  // this workgroup's pool (segment): its fields replace the single-pool ones (uniform)
  KvArgs a = a0;
  int blk = static_cast<int>(blockIdx.x);
  if (a0.nseg > 0) {
    int sg = 0;
#pragma unroll
    for (int q = 1; q < kKvMaxSeg; ++q) sg += (q < a0.nseg && blk >= a0.seg_tile0[q]) ? 1 : 0;
    blk -= a0.seg_tile0[sg];
    a.pool = a0.seg_pool[sg];
    a.n_pool = a0.seg_npool[sg];
    a.idx = nullptr;
    a.rows = a0.seg_rows[sg];
    a.r0 = a0.seg_r0[sg];
    a.seed = a0.seg_seed[sg];
    a.counts = a0.seg_counts[sg];
    a.label = a0.seg_label[sg];
    a.prob = nullptr;
  }
  // ONE __shared__ object: beside a second one hipcc drains the DMA (vmcnt(0))
  // before every chunk's first LDS read. GEMM phase: the W' ring (the row
  // statistics reuse buffer 0 after it); network phase: a stage's weight planes
  // at 0, the waves' activation tiles after them, two counters last.
  constexpr int kWBuf = 3;  // W' ring: chunk c + 2's DMA is issued during chunk c (kWBuf - 1 == 2 assumed below)
  constexpr int kRT = kLap ? kLap : (kF16 && W == 8) ? 2 : 1;  // 16-row tiles per wave (f32 rows: one, for the split's registers)
  constexpr int kAT = kLap ? 1 : kRT;         // of them loaded: the laps share one tile of raw rows
  constexpr int kThr = 64 * W;
  constexpr int kGemmBytes = kWBuf * 2 * kH2 * kKvKC * 2;
  constexpr int kWsBytes = 2 * kH2 * kNetWLd * 2;
  constexpr int kActBytes = W * 16 * kRT * kAld * 4;
  constexpr int kLdsBytes = (kGemmBytes > kWsBytes + kActBytes ? kGemmBytes : kWsBytes + kActBytes) + 16;
  static_assert(kLdsBytes <= 160 * 1024, "one workgroup's LDS");
  __shared__ __attribute__((aligned(16))) unsigned char smem[kLdsBytes];
  auto wb = reinterpret_cast<_Float16 (*)[2][kH2][kKvKC]>(smem);  // [buf][hi / lo][n][k] (swizzled pieces)
  float (*stS)[16 * kRT][2] = reinterpret_cast<float (*)[16 * kRT][2]>(smem);
  static_assert(sizeof(float) * W * 16 * kRT * 2 <= kWsBytes, "statistics: below the activation tiles");
#ifndef HBK_KV_DEPTH
#define HBK_KV_DEPTH 2
#endif
  constexpr int kDepth = kF16 ? HBK_KV_DEPTH : 2;  // A chunks in flight (this one + kDepth - 1 ahead)
  constexpr int kBGroup = kDepth > 2 ? 2 : 4;       // column tiles whose B fragments may be in flight together
  constexpr int kU = kF16 ? 1 : 2;  // 16-B loads per 8 elements
  constexpr int kALoads = kAT * 2 * kU;  // per chunk
  constexpr int kTile = W * 16 * kRT;
  constexpr int kDma = 32 / W;  // W' DMA instructions per wave and chunk (2 planes x 128 rows of 128 B)
  static_assert(kALoads * (kDepth - 1) + kDma < 16, "the counted waits use vmcnt's low field");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
  const int64_t tile0 = int64_t(blk) * kTile;
  // the lap form: the set's first row evaluation, and the wave's first row of the set's lap 0
  const int64_t lap_s = kLap ? int64_t(blk / max(a.lap_tiles, 1)) * kLap * a.n_pool : 0;
  const int64_t lap_b = kLap ? int64_t(blk % max(a.lap_tiles, 1)) * (16 * W) + 16 * wave : 0;
  // row j of the wave's tile rt: its row evaluation in the launch, and whether there is one
  auto row_of = [&](int rt, int j, bool& live) -> int64_t {
    if constexpr (kLap > 0) {
      const int64_t r = lap_s + rt * a.n_pool + lap_b + j;
      live = lap_b + j < a.n_pool && r < a.rows;
      return r;
    } else {
      const int64_t r = tile0 + 16 * kRT * wave + 16 * rt + j;
      live = r < a.rows;
      return r;
    }
  };
  const char* rp[kAT];
  uint32_t rid[kRT];
  if constexpr (kLap > 0) {
    const int64_t b = min(lap_b + m, a.n_pool - 1);  // (dead rows repeat the pool's last one)
    const int64_t pr = min(max((a.r0 + b) % a.n_pool, int64_t(0)), a.n_pool - 1);  // lap_s is whole laps
    rp[0] = static_cast<const char*>(a.pool) + pr * kD * 2;
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) rid[rt] = static_cast<uint32_t>(a.r0 + lap_s + rt * a.n_pool + b);
  } else {
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt) {
    const int64_t r = min(tile0 + 16 * kRT * wave + 16 * rt + m, a.rows - 1);
    int64_t pr = a.idx ? static_cast<int64_t>(a.idx[r]) : (a.r0 + r) % a.n_pool;
    pr = min(max(pr, int64_t(0)), a.n_pool - 1);
    rp[rt] = static_cast<const char*>(a.pool) + pr * kD * (kF16 ? 2 : 4);
    rid[rt] = static_cast<uint32_t>(a.r0 + r);
  }
  }
  const uint64_t seed = a.seed;
  const uint32_t s0 = static_cast<uint32_t>(seed), s1 = static_cast<uint32_t>(seed >> 32) * 0x27D4EB2Fu;
  const uint32_t thr = static_cast<uint32_t>(a.drop_p * 65536.f + 0.5f);
  const float keep = a.drop_p > 0.f ? 1.f / (1.f - a.drop_p) : 1.f;
  uint4 ar[kDepth][kAT][2][kU];
  auto load_rows = [&](int c, int slot) {
#pragma unroll
    for (int rt = 0; rt < kAT; ++rt)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int k = kKvKC * c + 32 * kb + 8 * kq;
#pragma unroll
        for (int u = 0; u < kU; ++u)
          ar[slot][rt][kb][u] = load_rows4(reinterpret_cast<const uint4*>(rp[rt] + int64_t(k) * (kF16 ? 2 : 4) + 16 * u));
      }
  };
  // W' chunk c -> buffer buf: 2 planes x 128 rows x 8 pieces = 2,048 pieces, 4 DMA
  // instructions per wave (8 rows each); lane l of instruction j writes piece
  // (row 8 (4 wave + j) + l / 8, slot l % 8), reading the source piece slot ^ swz(row)
  auto dma_w = [&](int c, int buf) {
#pragma unroll
    for (int j = 0; j < kDma; ++j) {
      const int row8 = kDma * wave + j;              // 0 .. 31: plane row8 / 16, rows 8 (row8 % 16) ..
      const int pl = row8 >> 4, n = 8 * (row8 & 15) + (lane >> 3), pc = (lane & 7) ^ kv_swz(n);
      const _Float16* src = a.wq + int64_t(pl) * kH2 * kD + int64_t(n) * kD + kKvKC * c + kKvPiece * pc;
      __builtin_amdgcn_global_load_lds(src, &wb[buf][pl][8 * (row8 & 15)][0], 16, 0, 0);
    }
  };
  // prologue: chunks 0 and 1 (W' buffers 0, 1; A slots 0, 1); chunk 0 waited for here,
  // chunk 1 at the end of chunk 0
  dma_w(0, 0);
  load_rows(0, 0);
  dma_w(1, 1);
#pragma unroll
  for (int d = 1; d < kDepth; ++d) load_rows(d, d);
  __builtin_amdgcn_s_waitcnt((kALoads * (kDepth - 1) + kDma) | (0x7 << 4) | (0xF << 8));  // chunk 0 in (the later chunks' DMA and rows may fly)
  dma_barrier();
  f4 acc[kRT][8];
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) acc[rt][ct] = f4{0.f, 0.f, 0.f, 0.f};
  double sd1[kRT], sd2[kRT];
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt) sd1[rt] = sd2[rt] = 0.0;
  static_assert(kKvChunks % kDepth == 0, "the A ring's slots must be compile-time");
  int buf = 0;  // W' buffer of chunk c (c % kWBuf; a run-time LDS offset, the A slot is unrolled)
#pragma unroll 1
  for (int cb = 0; cb < kKvChunks; cb += kDepth)
#pragma unroll
  for (int slot = 0; slot < kDepth; ++slot) {
    const int c = cb + slot;
    const int bnext = buf == 0 ? kWBuf - 1 : buf - 1;  // (c + 2) % kWBuf
    // this chunk's A values (dropout mask, row sums, split) first: their loads are
    // ordinary global loads, so no DMA may be outstanding when they are used
    h8 ah[kRT][2], al[kRT][2];
    float t1[kRT], t2[kRT];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) t1[rt] = t2[rt] = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) {
        float v[8];
        if (kF16) {
          const h8 hv = __builtin_bit_cast(h8, ar[slot][kLap ? 0 : rt][kb][0]);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = static_cast<float>(hv[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = __builtin_bit_cast(float, (&ar[slot][kLap ? 0 : rt][kb][e >> 2].x)[e & 3]);
        }
        if (!(HBK_KV_ABLATE & 2) && a.drop_p > 0.f) {  // nn.Dropout's mask (the 1 / (1 - p) scale is applied after the GEMM)
          const uint32_t base = rid[rt] * (kD / 2) + ((kKvKC * c + 32 * kb + 8 * kq) >> 1);
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            const uint32_t hsh = drop_hash(s0, s1, base + (e >> 1));
            v[e] = (hsh & 0xFFFFu) < thr ? 0.f : v[e];
            v[e + 1] = (hsh >> 16) < thr ? 0.f : v[e + 1];
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          t1[rt] += v[e];
          t2[rt] += v[e] * v[e];
        }
        if (kF16) {
#pragma unroll
          for (int e = 0; e < 8; ++e) ah[rt][kb][e] = static_cast<_Float16>(v[e]);  // exact
        } else {
          split8(f4{v[0], v[1], v[2], v[3]}, f4{v[4], v[5], v[6], v[7]}, ah[rt][kb], al[rt][kb]);
        }
      }
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) {
      sd1[rt] += double(t1[rt]);
      sd2[rt] += double(t2[rt]);
    }
    // unconditional (past the end: a clamped re-read) so that the loop has no
    // branches and hipcc's counted waits stay exact across the back edge
    dma_w(min(c + 2, kKvChunks - 1), bnext);  // its readers (chunk c - 1) passed the last barrier
    load_rows(min(c + kDepth, kKvChunks - 1), slot);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
        const int n = 16 * ct + m, pc = (4 * kb + kq) ^ kv_swz(n);
        const h8 bh = *reinterpret_cast<const h8*>(&wb[buf][0][n][kKvPiece * pc]);
        const h8 bl = *reinterpret_cast<const h8*>(&wb[buf][1][n][kKvPiece * pc]);
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) {
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt][kb], bh, acc[rt][ct], 0, 0, 0);
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt][kb], bl, acc[rt][ct], 0, 0, 0);
          if (!kF16) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rt][kb], bh, acc[rt][ct], 0, 0, 0);
        }
        if ((ct & (kBGroup - 1)) == kBGroup - 1) __builtin_amdgcn_sched_barrier(0);  // bound the B fragments in flight (registers)
      }
    // chunk c + 1's DMA and rows retired (chunk c + 2's, issued above, may still fly), then the barrier.
    // The sched_barriers keep the next chunk's conversions below the counted wait: hoisted
    // above it, hipcc guards them with vmcnt(0) (DMA and row loads pending together)
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt((kALoads * (kDepth - 1) + kDma) | (0x7 << 4) | (0xF << 8));  // chunk c + 1 in
    __builtin_amdgcn_s_waitcnt((0x3F & 0xF) | ((0x3F >> 4) << 14) | (0x7 << 4) | (0x0 << 8));  // lgkmcnt(0)
    dma_barrier();
    __builtin_amdgcn_sched_barrier(0);
    buf = buf == kWBuf - 1 ? 0 : buf + 1;
  }
  __builtin_amdgcn_s_waitcnt((0x7 << 4) | (0xF << 8));  // vmcnt(0): the clamped re-reads (into buffers 0, 1) in
  dma_barrier();
  // row statistics: the 4 lanes m + 16 kq hold a row's parts
  // (buffer 0's last readers, chunk kKvChunks - 2, passed that chunk's barrier)
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt) {
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      sd1[rt] += __shfl_xor(sd1[rt], o, 64);
      sd2[rt] += __shfl_xor(sd2[rt], o, 64);
    }
    if (kq == 0) {
      const double mu = sd1[rt] * (1.0 / kD);
      const double var = fmax(sd2[rt] * (1.0 / kD) - mu * mu, 0.0);
      const double kp = double(keep);
      stS[wave][16 * rt + m][0] = static_cast<float>(kp * mu);                              // mean of the dropped-out row
      stS[wave][16 * rt + m][1] = static_cast<float>(1.0 / sqrt(kp * kp * var + double(kLnEps)));  // its 1 / std
    }
  }
  dma_barrier();
#if HBK_KV_ABLATE & 1  // profiling build: the input GEMM only (no network, no counts)
  if (a.rows > 0) return;
#endif
  // ---- the rest of the network, per wave on its kRT row tiles ----
  // HG0 = rs (acc / 16 keep - mu c1) + c0 + b; U0 = silu(H) G into the wave's
  // activation tile (the lane holds hidden column j = 16 ct + m and gate column
  // 64 + j: ct and ct + 4)
  float* A = reinterpret_cast<float*>(smem + kWsBytes) + wave * (16 * kRT * kAld);
  {
    const float ks = keep * (1.f / 16.f);
    float mu[kRT][4], rs[kRT][4];
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        mu[rt][e] = stS[wave][16 * rt + 4 * kq + e][0];
        rs[rt][e] = stS[wave][16 * rt + 4 * kq + e][1];
      }
    lds_barrier();  // every wave has its statistics: the activation tiles may overwrite them
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int j = 16 * ct + m;
      const float c0h = a.c0[j] + a.P[a.b_hg[0] + j], c0g = a.c0[kH + j] + a.P[a.b_hg[0] + kH + j];
      const float c1h = a.c1[j], c1g = a.c1[kH + j];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float h = rs[rt][e] * (acc[rt][ct][e] * ks - mu[rt][e] * c1h) + c0h;
          const float g = rs[rt][e] * (acc[rt][ct + 4][e] * ks - mu[rt][e] * c1g) + c0g;
          A[(16 * rt + 4 * kq + e) * kAld + j] = h * sigm_fast(h) * g;
        }
    }
  }
  // weight stages: W_o_0, W_hg_1, W_o_1, ..., W_hg_{NG-1}: (cache offset, N, K); each
  // stage's f16 hi / lo planes staged into LDS once for the 8 waves, the next
  // stage's loaded into registers while the current one runs
  _Float16 (*wS)[kH2][kNetWLd] = reinterpret_cast<_Float16 (*)[kH2][kNetWLd]>(smem);
  constexpr int kStages = 2 * (NG - 1);
  auto st_off = [&](int st) { return (st & 1) ? a.c_hg[st / 2 + 1] : a.c_o[st / 2]; };
  auto st_n = [](int st) { return (st & 1) ? kH2 : kL; };
  auto st_k = [](int st) { return (st & 1) ? kL : kH; };
  // (six named registers, not an array: an array here stays in scratch memory
  // beside the GEMM phase's register pressure)
  uint4 wr0, wr1, wr2, wr3, wr4, wr5;
  constexpr int kWr = 3072 / kThr;  // staged 16-B pieces per thread (W_hg: 2 planes x 1,536)
  auto piece = [&](int st, int j, int& pl, int& n, int& k) {
    const int N = st_n(st), K = st_k(st), pieces = N * K / 8;  // per plane
    const int q = min(tid + kThr * j, 2 * pieces - 1), e0 = q % pieces;
    pl = q / pieces;
    n = (8 * e0) / K;
    k = 8 * e0 - n * K;
  };
  auto load1 = [&](int st, int j, uint4& v) {
    int pl, n, k;
    piece(st, j, pl, n, k);
    v = *reinterpret_cast<const uint4*>(a.wc + st_off(st) + int64_t(pl) * st_n(st) * st_k(st) + n * st_k(st) + k);
  };
  auto store1 = [&](int st, int j, const uint4& v) {  // (threads past the pieces repeat the last one)
    int pl, n, k;
    piece(st, j, pl, n, k);
    *reinterpret_cast<uint4*>(&wS[pl][n][k]) = v;
  };
  auto load_w = [&](int st) {
    load1(st, 0, wr0);
    load1(st, 1, wr1);
    load1(st, 2, wr2);
    if constexpr (kWr > 3) {
      load1(st, 3, wr3);
      load1(st, 4, wr4);
      load1(st, 5, wr5);
    }
  };
  auto store_w = [&](int st) {
    store1(st, 0, wr0);
    store1(st, 1, wr1);
    store1(st, 2, wr2);
    if constexpr (kWr > 3) {
      store1(st, 3, wr3);
      store1(st, 4, wr4);
      store1(st, 5, wr5);
    }
  };
  load_w(0);
  store_w(0);
  lds_barrier();
  const float* P = a.P;
#pragma unroll
  for (int st = 0; st < kStages; ++st) {
    if (st + 1 < kStages) load_w(st + 1);  // the next stage's planes, in flight during this one
    if ((st & 1) == 0) {
      // S = U W_o^T + b_o (K 64, N 96: 6 column tiles), then LayerNorm k -> X (A, K 96)
      const int k = st / 2;
      AFrag<kH> af[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) af[rt] = load_a<kH, kAld>(A + 16 * rt * kAld, lane);
      f4 c[kRT][6];
#pragma unroll
      for (int ct = 0; ct < 6; ++ct) {
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) c[rt][ct] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < kH / 32; ++i) {
          const h8 bh = *reinterpret_cast<const h8*>(&wS[0][16 * ct + m][32 * i + 8 * kq]);
          const h8 bl = *reinterpret_cast<const h8*>(&wS[1][16 * ct + m][32 * i + 8 * kq]);
#pragma unroll
          for (int rt = 0; rt < kRT; ++rt) c[rt][ct] = mma3(af[rt].h[i], af[rt].l[i], bh, bl, c[rt][ct]);
        }
      }
      float bo[6], gm[6], bt[6];
#pragma unroll
      for (int ct = 0; ct < 6; ++ct) {
        bo[ct] = P[a.b_o[k] + 16 * ct + m];
        gm[ct] = P[a.ln_g[k] + 16 * ct + m];
        bt[ct] = P[a.ln_b[k] + 16 * ct + m];
      }
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) {
        float sm[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ct = 0; ct < 6; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            c[rt][ct][e] = c[rt][ct][e] * af[rt].inv + bo[ct];
            sm[e] += c[rt][ct][e];
          }
        float mu[4], sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) mu[e] = rsum16(sm[e]) * (1.f / kL);
#pragma unroll
        for (int ct = 0; ct < 6; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e) sq[e] += (c[rt][ct][e] - mu[e]) * (c[rt][ct][e] - mu[e]);
#pragma unroll
        for (int e = 0; e < 4; ++e) sq[e] = __builtin_amdgcn_rsqf(rsum16(sq[e]) * (1.f / kL) + kLnEps);
#pragma unroll
        for (int ct = 0; ct < 6; ++ct)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            A[(16 * rt + 4 * kq + e) * kAld + 16 * ct + m] = (c[rt][ct][e] - mu[e]) * sq[e] * gm[ct] + bt[ct];
      }
    } else {
      // HG = X W_hg^T + b (K 96, N 128), gate in the epilogue -> U (A, K 64)
      const int k = st / 2 + 1;
      AFrag<kL> af[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) af[rt] = load_a<kL, kAld>(A + 16 * rt * kAld, lane);
      f4 c[kRT][8];
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) {
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) c[rt][ct] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < kL / 32; ++i) {
          const h8 bh = *reinterpret_cast<const h8*>(&wS[0][16 * ct + m][32 * i + 8 * kq]);
          const h8 bl = *reinterpret_cast<const h8*>(&wS[1][16 * ct + m][32 * i + 8 * kq]);
#pragma unroll
          for (int rt = 0; rt < kRT; ++rt) c[rt][ct] = mma3(af[rt].h[i], af[rt].l[i], bh, bl, c[rt][ct]);
        }
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int col = 16 * ct + m;
        const float bh = P[a.b_hg[k] + col], bg = P[a.b_hg[k] + kH + col];
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float h = c[rt][ct][e] * af[rt].inv + bh, g = c[rt][ct + 4][e] * af[rt].inv + bg;
            A[(16 * rt + 4 * kq + e) * kAld + col] = h * sigm_fast(h) * g;
          }
      }
    }
    if (st + 1 < kStages) {
      lds_barrier();  // every wave is done with this stage's planes
      store_w(st + 1);
      lds_barrier();
    }
  }
  // z = U w_out + b_out: lane -> row lane / 4 of a tile, 16 columns; sigmoid, counts
  float* cntS = reinterpret_cast<float*>(smem + kWsBytes + kActBytes);
  if (tid < 2) cntS[tid] = 0.f;
  lds_barrier();
  {
    const int r = lane >> 2, c0 = 16 * (lane & 3);
    float wo[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) wo[q] = P[a.w_o[NG - 1] + c0 + q];
    const float bz = P[a.b_o[NG - 1]];
    int ge = 0, gt = 0;
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) {
      float z = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) z = fmaf(A[(16 * rt + r) * kAld + c0 + q], wo[q], z);
      z += dpp_f<0xB1>(z);  // quad_perm: lanes ^ 1, ^ 2 hold the row's other columns
      z += dpp_f<0x4E>(z);
      z += bz;
      bool live;
      const int64_t row = row_of(rt, r, live);
      live = live && (lane & 3) == 0;
      const float p = sigm_fast(z);
      if (live && a.prob) a.prob[row] = p;
      ge += __popcll(__ballot(live && p >= a.act_thr));
      gt += __popcll(__ballot(live && p > a.act_thr));
    }
    if (lane == 0) {
      if (ge) atomicAdd(&cntS[0], static_cast<float>(ge));
      if (gt) atomicAdd(&cntS[1], static_cast<float>(gt));
    }
  }
  lds_barrier();
  if (tid < 2 && cntS[tid] != 0.f) atomicAdd(a.counts + 2 * a.label + tid, cntS[tid]);
}


// After the passes (trainer.py:509-536, :549-566): the validation false
// positives per hour (count / hours in float32, as torch divides an integer
// count tensor by a Python float), recall, the testing rates, and the dynamic
// negative weight (x ratio above the target rate, / ratio with a floor of 1
// otherwise) written into the schedule rows of every later step.
struct EvalFinish {
  const float* cv;  // validation counts [4] (label 0: >=, >; label 1: >=, >)
  const float* ct;  // testing counts [4] or NULL
  float n_neg_v, n_pos_v, n_neg_t, n_pos_t;
  float hours_v;    // n_neg_v * 1.44 / 3600, rounded to float32 on the host
  float target, ratio;  // ratio <= 0: no dynamic adjustment
  float* sched;
  int64_t sched_len, next_step;
  float* out;       // [8]
};
__global__ void __launch_bounds__(256) kv_finish_kernel(EvalFinish f) {
  const float cur = f.sched ? f.sched[2 * max(int64_t(0), min(f.next_step - 1, f.sched_len - 1)) + 1] : 1.f;
  float fph = 0.f, rec = 0.f, nw = cur;
  if (f.cv) {
    fph = f.cv[0] / f.hours_v;  // float32 division (x / 0 -> inf, 0 / 0 -> nan, as torch)
    rec = f.n_pos_v > 0.f ? f.cv[3] / f.n_pos_v : 0.f;
    if (f.ratio > 0.f) nw = fph > f.target ? cur * f.ratio : fmaxf(1.f, cur / f.ratio);
  }
  if (threadIdx.x == 0 && f.out) {
    f.out[0] = fph;
    f.out[1] = rec;
    if (f.ct) {
      f.out[2] = f.ct[0] / fmaxf(f.n_neg_t, 1.f);
      f.out[3] = f.n_pos_t > 0.f ? f.ct[3] / f.n_pos_t : 0.f;
      f.out[4] = (f.ct[3] + (f.n_neg_t - f.ct[1])) / fmaxf(f.n_neg_t + f.n_pos_t, 1.f);
    } else {
      f.out[2] = f.out[3] = f.out[4] = 0.f;
    }
    f.out[5] = nw;
    f.out[6] = cur;
    f.out[7] = 0.f;
  }
  if (f.cv && f.ratio > 0.f && f.sched)
    for (int64_t s = f.next_step + threadIdx.x; s < f.sched_len; s += blockDim.x) f.sched[2 * s + 1] = nw;
}

// kv_gemm_kernel<kF16, NG, W, kLap> for a plan's NG
template <bool kF16, int W, int kLap = 0>
auto kv_kernel(int NG) {
  return NG == 2 ? kv_gemm_kernel<kF16, 2, W, kLap> : NG == 3 ? kv_gemm_kernel<kF16, 3, W, kLap>
                                                                : kv_gemm_kernel<kF16, 4, W, kLap>;
}

// evaluation workspace: the weight cache (as the fused layout's first region),
// W' planes, c0, c1
struct EvalWs {
  int64_t wsplit, wq, c0, c1, total;  // float offsets
};
EvalWs eval_layout(int NG) {
  EvalWs w;
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t r = o; o += (n + 63) & ~int64_t(63); return r; };
  w.wsplit = take(wsplit_halves(NG) / 2);
  w.wq = take(int64_t(kH2) * kD);  // 2 planes of halves
  w.c0 = take(kH2);
  w.c1 = take(kH2);
  w.total = o;
  return w;
}

// Evaluation passes (validation / testing forwards reduced to prediction counts): the launchers
// behind the entry points below.
int64_t mlp_eval_ws_floats(const hbk_mlp_plan& p, int64_t rows) {
  (void)rows;  // the passes need no per-row workspace
  return eval_layout(static_cast<int>(p.g.size())).total;
}

int mlp_eval_prepare(const hbk_mlp_plan& p, const float* params, float* ws, hipStream_t s) {
  const int NG = static_cast<int>(p.g.size());
  const EvalWs w = eval_layout(NG);
  const int rc = mlp_wcache_fill(p, params, ws + w.wsplit, s);
  if (rc != HBK_OK) return rc;
  hipLaunchKernelGGL(kv_prep_kernel, dim3(kH2), dim3(256), 0, s, params, p.g[0].w_hg, p.ln_in.g, p.ln_in.b,
                     reinterpret_cast<_Float16*>(ws + w.wq), ws + w.c0, ws + w.c1);
  HBK_LAUNCH_CHECK("kv_prep_kernel");
  return HBK_OK;
}

// The rows mlp_eval_count evaluates in the lap form (two laps of the pool together) and in the plain form.
// How a single-pool pass of `rows` row evaluations is launched: part[0] rows in the lap form (whole sets
// of two laps, so no set carries a dead lap), part[1] in the plain form. Laps are for f16 pools read in
// order that the pass covers at least twice. HBK_EVAL_LAPS=0 (read per call, so one process can compare)
// restores the plain form everywhere.
void mlp_eval_lap_plan(int64_t rows, int64_t n_pool, bool f16, bool has_idx, int64_t part[2]) {
  part[0] = 0;
  part[1] = rows;
  if (!read_step_knobs().eval_laps || !f16 || has_idx || n_pool <= 0 || rows <= 0) return;
  part[0] = rows / (2 * n_pool) * (2 * n_pool);
  part[1] = rows - part[0];
}

// One kv_gemm_kernel launch over nseg pools of one dtype (nseg = 1: the single-pool fields,
// which also allow idx / prob; nseg > 1: the segment table, workgroups in pool order).
int mlp_eval_launch(const hbk_mlp_plan& p, const float* params, bool f16, const EvalSeg* seg, int nseg,
                           const int32_t* idx, float act_thr, float drop_p, float* prob, float* ws, hipStream_t s) {
  const int NG = static_cast<int>(p.g.size());
  const EvalWs w = eval_layout(NG);
  const WCacheOffsets kc = mlp_wcache_offsets(p);
  KvArgs ka{};
  ka.pool = seg[0].pool;
  ka.n_pool = seg[0].n_pool;
  ka.idx = idx;
  ka.rows = seg[0].rows;
  ka.r0 = seg[0].r0;
  ka.wq = reinterpret_cast<const _Float16*>(ws + w.wq);
  ka.c0 = ws + w.c0;
  ka.c1 = ws + w.c1;
  ka.drop_p = drop_p;
  ka.seed = seg[0].seed;
  ka.P = params;
  for (int i = 0; i < kMaxG; ++i) {
    const int g = std::min(i, NG - 1);
    ka.b_hg[i] = p.g[g].b_hg;
    ka.b_o[i] = p.g[g].b_o;
    ka.w_o[i] = p.g[g].w_o;
    ka.ln_g[i] = i + 1 < NG ? p.ln[i].g : 0;
    ka.ln_b[i] = i + 1 < NG ? p.ln[i].b : 0;
    ka.c_o[i] = kc.c_o[i];
    ka.c_hg[i] = kc.c_hg[i];
  }
  ka.wc = reinterpret_cast<const _Float16*>(ws + w.wsplit);
  ka.act_thr = act_thr;
  ka.counts = seg[0].counts;
  ka.label = seg[0].label;
  ka.prob = prob;
  // f16 rows: 16 waves of one 16-row tile each (126 VGPRs); f32 rows (the split's registers
  // spill at 128): 8 waves. HBK_KV_WAVES=8: 8 waves of two tiles for f16 rows too (A/B)
  const int waves = f16 && !read_step_knobs().kv_waves8 ? 16 : 8;
  const int tile = (f16 ? 256 : 128);  // kv_gemm_kernel's rows per workgroup
  int64_t tiles = (seg[0].rows + tile - 1) / tile;
  ka.nseg = 0;
  if (nseg > 1) {
    ka.nseg = nseg;
    tiles = 0;
    for (int i = 0; i < nseg; ++i) {
      ka.seg_tile0[i] = static_cast<int>(tiles);
      ka.seg_pool[i] = seg[i].pool;
      ka.seg_npool[i] = seg[i].n_pool;
      ka.seg_rows[i] = seg[i].rows;
      ka.seg_r0[i] = seg[i].r0;
      ka.seg_seed[i] = seg[i].seed;
      ka.seg_counts[i] = seg[i].counts;
      ka.seg_label[i] = seg[i].label;
      tiles += (seg[i].rows + tile - 1) / tile;
    }
    ka.seg_tile0[nseg] = static_cast<int>(tiles);
  }
  // the lap form first, over the pass's whole lap sets; what is left goes to the plain form
  if (nseg == 1) {
    int64_t part[2];
    mlp_eval_lap_plan(seg[0].rows, seg[0].n_pool, f16, idx != nullptr, part);
    if (part[0] > 0) {
      ka.lap_tiles = static_cast<int>((seg[0].n_pool + 127) / 128);
      ka.rows = part[0];
      const dim3 lgrid(static_cast<unsigned>(part[0] / (2 * seg[0].n_pool) * ka.lap_tiles));
      hipLaunchKernelGGL((kv_kernel<true, 8, 2>(NG)), lgrid, dim3(512), 0, s, ka);
      HBK_LAUNCH_CHECK("kv_gemm_kernel (laps)");
      ka.r0 += part[0];
      if (ka.prob) ka.prob += part[0];
      ka.lap_tiles = 0;
      ka.rows = part[1];
      if (part[1] == 0) return HBK_OK;
      tiles = (part[1] + tile - 1) / tile;
    }
  }
  const dim3 grid(static_cast<unsigned>(tiles));
  void (*kern)(KvArgs) = waves == 16 ? kv_kernel<true, 16>(NG) : f16 ? kv_kernel<true, 8>(NG) : kv_kernel<false, 8>(NG);
  hipLaunchKernelGGL(kern, grid, dim3(64 * waves), 0, s, ka);
  HBK_LAUNCH_CHECK("kv_gemm_kernel");
  return HBK_OK;
}

int mlp_eval_count(const hbk_mlp_plan& p, const float* params, const void* pool, bool f16, int64_t n_pool,
                   const int32_t* idx, int64_t rows, int64_t r0, int label, float act_thr, float drop_p,
                   uint64_t seed, float* counts, float* prob, float* ws, hipStream_t s) {
  if (rows <= 0) return HBK_OK;
  const EvalSeg seg{pool, n_pool, rows, r0, seed, counts, label};
  return mlp_eval_launch(p, params, f16, &seg, 1, idx, act_thr, drop_p, prob, ws, s);
}

int mlp_eval_count_multi(const hbk_mlp_plan& p, const float* params, bool f16, const EvalSeg* seg, int nseg,
                         float act_thr, float drop_p, float* ws, hipStream_t s) {
  EvalSeg live[kKvMaxSeg];
  int n = 0;
  for (int i = 0; i < nseg; ++i)
    if (seg[i].rows > 0) live[n++] = seg[i];
  if (n == 0) return HBK_OK;
  return mlp_eval_launch(p, params, f16, live, n, nullptr, act_thr, drop_p, nullptr, ws, s);
}

int mlp_eval_finish(const float* cv, const float* ct, const double* sizes, float target, float ratio, float* sched,
                    int64_t sched_len, int64_t next_step, float* out, hipStream_t s) {
  EvalFinish f;
  f.cv = cv;
  f.ct = ct;
  f.n_neg_v = static_cast<float>(sizes[0]);
  f.n_pos_v = static_cast<float>(sizes[1]);
  f.n_neg_t = static_cast<float>(sizes[2]);
  f.n_pos_t = static_cast<float>(sizes[3]);
  f.hours_v = static_cast<float>(sizes[0] * 1.44 / 3600.0);
  f.target = target;
  f.ratio = ratio;
  f.sched = sched;
  f.sched_len = sched_len;
  f.next_step = next_step;
  f.out = out;
  hipLaunchKernelGGL(kv_finish_kernel, dim3(1), dim3(256), 0, s, f);
  HBK_LAUNCH_CHECK("kv_finish_kernel");
  return HBK_OK;
}

}  // namespace
}  // namespace hbk

// The passes' entry points: argument checks, then the launchers above.
extern "C" {

int hbk_mlp_eval_workspace_size(const hbk_mlp_plan* p, int64_t rows, int64_t* bytes) {
  using namespace hbk;
  if (!p || !bytes) return arg_error("NULL");
  if (!mlp_fused_supported(*p)) return mlp_unsupported(*p, "the evaluation pass");
  *bytes = mlp_eval_ws_floats(*p, std::max<int64_t>(rows, 1)) * int64_t(sizeof(float));
  return HBK_OK;
}

int hbk_mlp_eval_prepare(const hbk_mlp_plan* p, const float* params, void* workspace, int64_t ws_bytes,
                         void* stream) {
  using namespace hbk;
  if (!p || !params || !workspace) return arg_error("NULL pointer");
  if (!mlp_fused_supported(*p)) return mlp_unsupported(*p, "the evaluation pass");
  if (ws_bytes < mlp_eval_ws_floats(*p, 1) * int64_t(sizeof(float))) return arg_error("workspace too small");
  return mlp_eval_prepare(*p, params, static_cast<float*>(workspace), as_stream(stream));
}

int hbk_mlp_eval_count(const hbk_mlp_plan* p, const float* params, const void* pool, int32_t pool_is_f16,
                       int64_t n_pool, const int32_t* idx, int64_t rows, int64_t row_offset, int32_t label,
                       float activation_threshold, float dropout_p, uint64_t seed, float* counts, float* prob,
                       void* workspace, int64_t ws_bytes, void* stream) {
  using namespace hbk;
  if (!p || !params || !workspace || !counts) return arg_error("NULL pointer");
  if (!mlp_fused_supported(*p)) return mlp_unsupported(*p, "the evaluation pass");
  if (rows < 0 || row_offset < 0 || rows + row_offset > (int64_t(1) << 31) / 768) return arg_error("rows out of range");
  if (rows == 0) return HBK_OK;
  if (!pool || n_pool <= 0) return arg_error("empty pool");
  if (label != 0 && label != 1) return arg_error("label must be 0 or 1");
  if (dropout_p < 0.f || dropout_p >= 1.f) return arg_error("dropout_p must be in [0, 1)");
  if (ws_bytes < mlp_eval_ws_floats(*p, rows) * int64_t(sizeof(float))) return arg_error("workspace too small");
  return mlp_eval_count(*p, params, pool, pool_is_f16 != 0, n_pool, idx, rows, row_offset, label,
                        activation_threshold, dropout_p, seed, counts, prob, static_cast<float*>(workspace),
                        as_stream(stream));
}

int hbk_mlp_eval_laps(int64_t rows, int64_t n_pool, int32_t pool_is_f16, int32_t has_idx, int64_t* parts) {
  using namespace hbk;
  if (!parts) return arg_error("NULL pointer");
  if (rows < 0 || n_pool <= 0) return arg_error("rows / n_pool out of range");
  mlp_eval_lap_plan(rows, n_pool, pool_is_f16 != 0, has_idx != 0, parts);
  return HBK_OK;
}

int hbk_mlp_eval_count_multi(const hbk_mlp_plan* p, const float* params, int32_t n_pools,
                             const void* const* pools, int32_t pools_are_f16, const int64_t* n_pool,
                             const int64_t* rows, const int64_t* row_offsets, const int32_t* labels,
                             const uint64_t* seeds, float* const* counts, float activation_threshold,
                             float dropout_p, void* workspace, int64_t ws_bytes, void* stream) {
  using namespace hbk;
  if (!p || !params || !workspace) return arg_error("NULL pointer");
  if (!mlp_fused_supported(*p)) return mlp_unsupported(*p, "the evaluation pass");
  if (n_pools < 0 || n_pools > kKvMaxSeg) return arg_error("n_pools must be in [0, 4]");
  if (n_pools == 0) return HBK_OK;
  if (!pools || !n_pool || !rows || !row_offsets || !labels || !seeds || !counts) return arg_error("NULL array");
  if (dropout_p < 0.f || dropout_p >= 1.f) return arg_error("dropout_p must be in [0, 1)");
  EvalSeg seg[kKvMaxSeg];
  int64_t max_rows = 0;
  for (int i = 0; i < n_pools; ++i) {
    if (rows[i] < 0 || row_offsets[i] < 0 || rows[i] + row_offsets[i] > (int64_t(1) << 31) / 768)
      return arg_error("rows out of range");
    if (rows[i] > 0 && (!pools[i] || n_pool[i] <= 0)) return arg_error("empty pool");
    if (labels[i] != 0 && labels[i] != 1) return arg_error("label must be 0 or 1");
    if (rows[i] > 0 && !counts[i]) return arg_error("counts is NULL");
    seg[i] = EvalSeg{pools[i], n_pool[i], rows[i], row_offsets[i], seeds[i], counts[i], labels[i]};
    max_rows = std::max(max_rows, rows[i]);
  }
  if (ws_bytes < mlp_eval_ws_floats(*p, max_rows) * int64_t(sizeof(float))) return arg_error("workspace too small");
  return mlp_eval_count_multi(*p, params, pools_are_f16 != 0, seg, n_pools, activation_threshold, dropout_p,
                              static_cast<float*>(workspace), as_stream(stream));
}

int hbk_mlp_eval_finish(const float* counts_val, const float* counts_test, const double* sizes,
                        float target_false_positives_per_hour, float adjust_ratio, float* sched, int64_t sched_len,
                        int64_t next_step, float* out, void* stream) {
  using namespace hbk;
  if (!sizes) return arg_error("sizes is NULL");
  if (sched && (sched_len <= 0 || next_step < 0)) return arg_error("schedule range");
  return mlp_eval_finish(counts_val, counts_test, sizes, target_false_positives_per_hour, adjust_ratio, sched,
                         sched_len, next_step, out, as_stream(stream));
}

}  // extern "C"
