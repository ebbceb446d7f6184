// The fused train step's planning (hbk_mlp_fused.hip) as pure host C++: which
// step variant runs, every kernel's geometry, the weight-gradient job table's
// shape and the workspace layout, as functions of (B, NG, n_params, the stream's
// CUs, the environment knobs). No HIP include: tests/step_plan_check.cpp compiles
// this header alone and checks it on a CPU.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "hbk_mlp_dims.h"

namespace hbk {

// ------------------------------------------------------------- constants ---
constexpr int kRB = 64;         // k1b: rows per block
constexpr int kPreTiles = 2;    // k1a row tiles per prefetch workgroup of k2 (v1)
constexpr int kPreTiles2 = 3;   // k1s (v2: statistics and mask only) row tiles per prefetch workgroup (2: 84.0, 3: 83.6, 4: 86.0 us per step)
constexpr int kK2Waves = 4;     // k2: waves per workgroup (its launch bounds; each publishes its gradient maxima: maxS)

// k3 (v1): tile 128 x 32; one job per weight matrix (dW_hg of every GMLP, dW_o of every GMLP)
constexpr int kTM = 128, kTN = 32, kMaxJobs = 2 * kMaxG;
constexpr int step_jobs(int NG) { return 2 * NG; }
static_assert(step_jobs(kMaxG) <= kMaxJobs, "the job tables of K3Args / K3sArgs hold every job");
// batch rows per split: measured 4 / 5 / 6 / 9 steps (124 / 152 / 180 / 248 VGPRs) at 60.2 / 60.3 /
// 61.6 / 58.9 us per step on 256 CUs and 88.7 / 88.9 / 94.8 / 92.1 on a 64-CU stream
#ifndef HBK_K3_STEPS
#define HBK_K3_STEPS 9
#endif
constexpr int kK3Steps = HBK_K3_STEPS;  // 32-row steps per split on a wide stream (B = 1100: 4 splits)
constexpr int kK3StepsNarrow = 4, kK3NarrowCUs = 96;
// narrow streams: one workgroup may walk this many consecutive 128-row splits
// (one partial slab per group). Measured at 3 on a 64-CU stream: k3 23.8 ->
// 38.9 us (256 VGPRs, two workgroups per CU, the splits' latencies in series)
// and k4 unchanged at 11.7 us with 3 slabs instead of 9, so it stays 1.
#ifndef HBK_K3_GROUP
#define HBK_K3_GROUP 1
#endif
constexpr int kK3GroupNarrow = HBK_K3_GROUP;

// k3s (v2)
constexpr int kK3sMaxR = 512;      // rows per split
constexpr int kK3sMaxTiles = 512;  // row tiles of a batch whose live tiles are listed (one thread each)
// N tile widths (in 16-column tiles): the input layer's 256 columns, the generic jobs' 128
constexpr int kK3sNbtRaw = 16, kK3sNbtGen = 8;
// The step counts of a split are compile-time (fully unrolled steps): {input layer's, generic jobs'}
constexpr int kK3sPairs[][2] = {{1, 1}, {2, 2}, {3, 3}, {3, 5}, {4, 4}, {4, 9}, {4, 12}, {5, 12},
                                {6, 14}, {7, 16}, {8, 8}, {9, 16}, {12, 12}, {16, 16}};
constexpr int kK3sNPairs = sizeof(kK3sPairs) / sizeof(kK3sPairs[0]);
constexpr bool k3s_pairs_ok() {
  for (int q = 0; q < kK3sNPairs; ++q)  // (st0 <= st1: the generic jobs never take more splits than the input layer)
    if (kK3sPairs[q][0] > kK3sPairs[q][1] || 32 * kK3sPairs[q][1] > kK3sMaxR) return false;
  return kK3sPairs[kK3sNPairs - 1][0] * 32 == kK3sMaxR;  // the fallback pair: the fewest splits
}
static_assert(k3s_pairs_ok(), "k3s step-count pairs");

// HBK_STEP=2: the v2 step (k1s -> k1c / k3s from the pool rows); 1: the k1a -> xhat^T ->
// k1b / k3 path. By default the faster one as measured for the batch (tools/ab_step.sh, 64
// CUs, r06: B = 1,100 v2 83.2 / v1 87.3 us; 550 65.1 / 63.5; 273 59.8 / 56.7; 138 57.2 /
// 51.4 -- k3s's fixed prologue and its 2 splits at ceil(Bp / 128) slabs cost it the small
// batches): v2 from kStepV2MinB rows (HBK_STEP_V2_MIN_B), on a stream of at most
// kStepV2MaxCUs CUs -- on the whole GPU v1 is faster (B = 1,100: 59.1 against 66.1 us; its
// 288-row splits and 32-column tiles spread over 256 CUs, where k3s's 256-column tiles and
// fixed prologue do not)
constexpr int kStepV2MinB = 800, kStepV2MaxCUs = 128;

// ----------------------------------------------------------------- knobs ---
// Every environment knob of the train step and the evaluation passes. "once": read by the
// process's first read_step_knobs() call and kept; "call": read again by every call. The once
// knobs are latched together, by whichever comes first of a step, a step-variant query, an
// evaluation launch or a lap query (each used to be latched by the first use of its own
// function): set them before the process's first classifier call.
//   HBK_STEP            1 / 2 forces the v1 / v2 step; 0 = by batch and stream width   0     once
//   HBK_STEP_V2_MIN_B   the smallest batch that takes v2 by default                    800   once
//   HBK_K1_KS           k1b's K splits (4 6 8 12 16 24; else by the batch)             0     once
//   HBK_K3_WIDE         set: k3's 288-row splits on narrow streams too                 unset once
//   HBK_STEP_DENSE      != 0: k3s walks every row tile, not the live ones only         0     once
//   HBK_KV_WAVES        8: kv_gemm with 8 waves of two tiles for f16 rows too          16    once
//   HBK_K1_KC           k1c's K chunk (64 96 192 384; 0 = by the cost model)           0     call
//   HBK_K1_RT           k1c's row tiles per block (0 = by the cost model)              0     call
//   HBK_K3_R            k3s: the first pair whose input-layer split has >= R rows      0     call
//   HBK_K3_PAIR         k3s: this pair of kK3sPairs (-1 = by the cost model)           -1    call
//   HBK_PRE_TILES       k1s row tiles per prefetch workgroup of k2 (>= 1)              3     call
//   HBK_PLAN_LOG        set: print the k3s plan of each distinct batch to stderr       unset call
//   HBK_EVAL_LAPS       0: the evaluation passes never take the lap form               on    call
//   HBK_STEP_GATE_SKIP  0: the flag of that name is ignored (the step computes and     1     call
//                       sums every gradient, as without it); 2: k3 / k3s leave on a
//                       step that does not fire, k4 keeps its unconditional loads (A/B
//                       of k4's two forms). Read by hbk_mlp_step_fwd_bwd; the update
//                       that follows takes the form that call settled (a captured
//                       graph keeps its capture's value)
struct StepKnobs {
  int step = 0, v2_min_b = kStepV2MinB, k1_ks = 0;
  bool k3_wide = false, dense = false, kv_waves8 = false;
  int k1_kc = 0, k1_rt = 0, k3_r = 0, k3_pair = -1, pre_tiles = kPreTiles2, gate_skip = 1;
  bool plan_log = false, eval_laps = true;
};
inline StepKnobs read_step_knobs() {
  auto env_int = [](const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
  };
  static const StepKnobs once = [&] {
    StepKnobs k;
    k.step = env_int("HBK_STEP", 0);
    k.v2_min_b = env_int("HBK_STEP_V2_MIN_B", kStepV2MinB);
    k.k1_ks = env_int("HBK_K1_KS", 0);
    k.k3_wide = getenv("HBK_K3_WIDE") != nullptr;
    k.dense = env_int("HBK_STEP_DENSE", 0) != 0;
    k.kv_waves8 = env_int("HBK_KV_WAVES", 0) == 8;
    return k;
  }();
  StepKnobs k = once;
  k.k1_kc = env_int("HBK_K1_KC", 0);
  k.k1_rt = env_int("HBK_K1_RT", 0);
  k.k3_r = env_int("HBK_K3_R", 0);
  k.k3_pair = env_int("HBK_K3_PAIR", -1);
  k.pre_tiles = env_int("HBK_PRE_TILES", kPreTiles2);
  k.gate_skip = env_int("HBK_STEP_GATE_SKIP", 1);
  k.plan_log = getenv("HBK_PLAN_LOG") != nullptr;
  const char* laps = getenv("HBK_EVAL_LAPS");
  k.eval_laps = !(laps && laps[0] == '0');
  return k;
}

// ------------------------------------------------------------- workspace ---
struct FusedWs {
  int64_t wsplit, part, pstride, hg_part, xhat[2], U, Xn, dS, dHG, rinfo[2], mask[2], maxS, total;  // float offsets
};
inline int64_t ws_align(int64_t n) { return (n + 63) & ~int64_t(63); }
// the weight cache (WSplit): f16 hi / lo planes of W_o_k (k < NG - 1) and W_hg_k (k >= 1), as stored and transposed
inline int64_t wsplit_halves(int NG) { return int64_t(NG - 1) * 4 * (kL * kH + kH2 * kL); }
// The partial slabs part[split][pstride] of the weight gradients (k3 / k3s write them, k4 or
// k3_fold_kernel sums them): one per kPartRows batch rows, the most splits any launch takes
constexpr int kPartRows = 32 * (kK3StepsNarrow < kK3Steps ? kK3StepsNarrow : kK3Steps);
inline int64_t part_slabs(int64_t Bp) { return (Bp + kPartRows - 1) / kPartRows; }
static_assert(32 * kK3StepsNarrow * kK3GroupNarrow >= kPartRows && 32 * kK3Steps >= kPartRows,
              "k3's splits at either width fit the slabs");
// The regions whose offsets do not move with the batch: the update (k4) finds the weight
// cache and the slabs a step left without knowing that step's B
struct FusedFixed {
  int64_t wsplit, part, pstride;
};
inline FusedFixed fused_fixed(int NG, int64_t n_params) {
  return FusedFixed{0, ws_align(wsplit_halves(NG) / 2), ws_align(n_params)};
}
inline int64_t maxs_floats(int NG, int64_t rt) { return int64_t(2) * NG * rt * kK2Waves; }  // [2 NG][rt][wave]
inline FusedWs fused_layout(int64_t B, int NG, int64_t n_params = 0) {
  FusedWs w;
  const FusedFixed f = fused_fixed(NG, n_params);
  int64_t o = f.part;
  auto take = [&](int64_t n) { const int64_t r = o; o += ws_align(n); return r; };
  const int64_t Bp = (B + kR - 1) / kR * kR;
  w.wsplit = f.wsplit;
  w.pstride = f.pstride;
  w.part = take(w.pstride * part_slabs(Bp));
  w.hg_part = take(int64_t(24) * B * kH2);
  w.xhat[0] = take(Bp * kD);
  w.xhat[1] = take(Bp * kD);
  // k3s reads these four unclamped, up to kK3sMaxR floats past an array's end (zeroed at use):
  // each is followed by that many floats that nothing writes, whatever the order of the arrays
  auto take_k3s = [&](int64_t n) { return take(n + kK3sMaxR); };
  w.U = take_k3s(int64_t(NG) * Bp * kH);
  w.Xn = take_k3s(int64_t(NG) * Bp * kL);
  w.dS = take_k3s(int64_t(NG) * Bp * kL);
  w.dHG = take_k3s(int64_t(NG) * Bp * kH2);
  w.rinfo[0] = take(Bp * 4);
  w.rinfo[1] = take(Bp * 4);
  w.mask[0] = take(Bp * kMaskW);
  w.mask[1] = take(Bp * kMaskW);
  w.maxS = take(maxs_floats(NG, Bp / kR));
  w.total = o;
  return w;
}

// -------------------------------------------------------------- geometry ---
inline bool step_v2(int64_t B, int64_t cus, const StepKnobs& kn) {
  if (kn.step) return kn.step == 2;
  return B >= kn.v2_min_b && cus <= kStepV2MaxCUs;
}
inline int k1_blocks(int B) { return ((B + kRB - 1) / kRB + 7) / 8 * 8; }  // row blocks, XCD-aware
inline int k1_splits(int B, const StepKnobs& kn) {  // (one round of three per CU on a 64-CU stream, KS 8, measured 92.1 vs 88.4 us per step)
  const int forced = kn.k1_ks;  // (A/B: 4 6 8 12 16 24)
  if (forced == 4 || forced == 6 || forced == 8 || forced == 12 || forced == 16 || forced == 24) return forced;
  static const int ks_opts[] = {4, 6, 8, 12, 16, 24};
  for (int ks : ks_opts)
    if (k1_blocks(B) * ks >= 256) return ks;
  return 24;
}
// k3's batch splits: rows per split by the stream's width (see kK3Steps). HBK_K3_WIDE: the
// 288-row splits on narrow streams too (4 instead of 9 splits at B = 1100: fewer partial
// slabs, more time on a small partition)
inline bool k3_narrow(int64_t cus, const StepKnobs& kn) { return !kn.k3_wide && cus <= kK3NarrowCUs; }
inline int k3_rows(bool narrow) { return 32 * (narrow ? kK3StepsNarrow * kK3GroupNarrow : kK3Steps); }
inline int k3_splits(int64_t Bp, bool narrow) { return static_cast<int>((Bp + k3_rows(narrow) - 1) / k3_rows(narrow)); }
// k1c's geometry: K chunk KC (KS = 1536 / KC chunks) and row tiles RT per block, by a
// per-CU byte model: the block's pool rows (~2.2 B per element at the training mix),
// its W slice and its partial slab, times the rounds of blocks per CU, plus the KS
// slabs each k2 row tile sums first (HBK_K1_KC / HBK_K1_RT override)
struct K1cGeom {
  int KC, RT, KS, blocks;
};
template <int KC>
constexpr int k1c_rt_max() {  // k1c's LDS: two f16 planes of 16 RT rows x (KC + 16)
  return 16 * (KC + 16) * 4 * 9 <= 150 * 1024 ? 9 : (150 * 1024) / (16 * (KC + 16) * 4);
}
inline int k1c_rtmax(int KC) {
  switch (KC) {
    case 64: return k1c_rt_max<64>();
    case 96: return k1c_rt_max<96>();
    case 192: return k1c_rt_max<192>();
    default: return k1c_rt_max<384>();
  }
}
inline K1cGeom k1c_geom(int B, int64_t cus_raw, const StepKnobs& kn) {
  const int cus = static_cast<int>(std::max<int64_t>(1, cus_raw));
  const int fkc = kn.k1_kc, frt = kn.k1_rt;
  K1cGeom best{192, 9, 8, 0};
  double best_cost = 1e30;
  for (int KC : {64, 96, 192, 384}) {
    if (fkc && KC != fkc) continue;
    const int rtm = k1c_rtmax(KC);
    const double lds = 16.0 * rtm * (KC + 16) * 4 + 8.0 * KC;
    const int per_cu = std::max(1, std::min(2, static_cast<int>(160.0 * 1024 / lds)));
    for (int RT = 1; RT <= rtm; ++RT) {
      if (frt && RT != std::min(frt, rtm)) continue;
      const int KS = kD / KC, nrb = (B + 16 * RT - 1) / (16 * RT), blocks = nrb * KS;
      const int rounds = (blocks + cus * per_cu - 1) / (cus * per_cu);
      const int on_cu = std::min(per_cu, (blocks + cus - 1) / cus);
      const double rows = std::min(16 * RT, B);
      const double per_wg = rows * KC * 2.2 + 128.0 * KC * 4 + rows * 128 * 4;
      const double cost = per_wg * on_cu * rounds + KS * 16.0 * 128 * 4;
      if (cost < best_cost) {
        best_cost = cost;
        best = K1cGeom{KC, RT, KS, blocks};
      }
    }
  }
  return best;
}
// k3s's batch splits: the input layer's job (most of the launch's tiles and the bulk of its
// FLOPs) gets S0 splits of NST0 32-row steps, the small generic jobs S1 <= S0 of NST1, so
// that the launch fits the CUs in one round and its longest workgroup (steps x the job's
// relative step cost: the generic tiles have 4 or 6 of 8 column tiles live) is shortest.
// One of kK3sPairs; at most part_slabs(Bp) splits (the workspace's slabs; the last pair's
// 512-row splits always fit them). HBK_K3_R forces one pair by its rows.
struct K3sPlan {
  int S0, S1, pair;
};
static_assert(kK3sMaxR >= kPartRows, "the fallback pair's splits fit the slabs");
// per-workgroup time model (units of ~0.78 us, the generic jobs' 32-row step of r06, fitted
// to the traced spans): the input layer's 3 + 1.6 x steps, a generic job's 2.5 + 0.65 x steps
inline K3sPlan k3s_plan(int64_t Bp, int tiles0, int tiles1, int64_t cus_raw, const StepKnobs& kn) {
  const int cus = static_cast<int>(std::max<int64_t>(1, cus_raw));
  const int64_t max_s = part_slabs(Bp);
  const int fr = kn.k3_r, fq = kn.k3_pair;
  auto splits = [&](int st) { return static_cast<int>((Bp + 32 * st - 1) / (32 * st)); };
  K3sPlan best{splits(16), splits(16), kK3sNPairs - 1};
  double best_cost = 1e30;
  for (int q = 0; q < kK3sNPairs; ++q) {
    const int st0 = kK3sPairs[q][0], st1 = kK3sPairs[q][1];
    if (fr > 0 && 32 * st0 < fr) continue;
    if (fq >= 0 && q != fq) continue;
    const int s0 = splits(st0), s1 = splits(st1);
    if (s0 > max_s && st0 < 16) continue;  // (the workspace's slabs)
    const int wgs = tiles0 * s0 + tiles1 * s1, rounds = (wgs + cus - 1) / cus;
    const double cost = rounds * std::max(3.0 + 1.6 * st0, 2.5 + 0.65 * st1) + 1e-3 * wgs;
    if (cost < best_cost) {
      best_cost = cost;
      best = K3sPlan{s0, s1, q};
    }
    if (fr > 0) break;
  }
  return best;
}

// The weight-gradient jobs dW [M][N] = dY^T X, in launch order: job 0 the input layer
// (dW_hg0), then dW_hg of GMLPs 1 .. NG - 1, then dW_o of every GMLP (the last one's M is
// the single output unit)
struct JobShape {
  int M, N;
};
inline JobShape step_job(int NG, int i) {
  if (i == 0) return JobShape{kH2, kD};
  if (i < NG) return JobShape{kH2, kL};
  return JobShape{i - NG + 1 < NG ? kL : 1, kH};
}

// ------------------------------------------------------------------ plan ---
struct StepPlan {
  int variant;  // 1: k1a / k1b / k3, 2: k1s / k1c / k3s
  int64_t Bp;   // B rounded up to the 16-row tile
  int rt;       // row tiles
  int KS;       // HG0 partial slabs of the input GEMM (k1b's K splits / k1c's K chunks): k2 sums them
  int k1_grid;  // k1b / k1c workgroups
  K1cGeom k1c;  // v2 (zeros in v1)
  int k3_rows, k3_narrow;        // v1: batch rows per split, the narrow-stream kernel (zeros in v2)
  int k3s_pair, S0, S1, sparse;  // v2: kK3sPairs index, the input layer's / generic jobs' splits, live tiles only
  int slabs;                     // partial slabs the weight-gradient launch writes (v1: its splits, v2: S0)
  int pre_tiles;                 // row tiles per prefetch workgroup of k2
  int k2_grid, k2_grid_pre;      // k2 workgroups without / with the next step's rows prefetched
  int n_jobs, job_tn[kMaxJobs], job_tiles[kMaxJobs], job_splits[kMaxJobs], job_start[kMaxJobs + 1];  // start[n_jobs] = workgroups
  FusedWs ws;
};
inline StepPlan plan_step(int B, int NG, int64_t n_params, int64_t cus, const StepKnobs& kn) {
  StepPlan pl{};
  pl.variant = step_v2(B, cus, kn) ? 2 : 1;
  pl.Bp = (int64_t(B) + kR - 1) / kR * kR;
  pl.rt = (B + kR - 1) / kR;
  pl.ws = fused_layout(B, NG, n_params);
  const bool v2 = pl.variant == 2;
  if (v2) {
    pl.k1c = k1c_geom(B, cus, kn);
    pl.KS = pl.k1c.KS;
    pl.k1_grid = pl.k1c.blocks;
  } else {
    pl.KS = k1_splits(B, kn);
    pl.k1_grid = k1_blocks(B) * pl.KS;
  }
  pl.pre_tiles = v2 ? std::max(1, kn.pre_tiles) : kPreTiles;
  pl.k2_grid = pl.rt;
  pl.k2_grid_pre = pl.rt + (pl.rt + pl.pre_tiles - 1) / pl.pre_tiles;
  // the job table: tiles of 128 x (v1: 32, v2: 256 input layer / 128) per job, times the job's splits
  pl.n_jobs = step_jobs(NG);
  const int tile_n[2] = {v2 ? 16 * kK3sNbtRaw : kTN, v2 ? 16 * kK3sNbtGen : kTN};
  int tiles_gen = 0;
  for (int i = 0; i < pl.n_jobs; ++i) {
    const JobShape js = step_job(NG, i);
    pl.job_tn[i] = (js.N + tile_n[i ? 1 : 0] - 1) / tile_n[i ? 1 : 0];
    pl.job_tiles[i] = ((js.M + kTM - 1) / kTM) * pl.job_tn[i];
    if (i) tiles_gen += pl.job_tiles[i];
  }
  if (v2) {
    const K3sPlan k3 = k3s_plan(pl.Bp, pl.job_tiles[0], tiles_gen, cus, kn);
    pl.k3s_pair = k3.pair;
    pl.S0 = k3.S0;
    pl.S1 = k3.S1;
    pl.sparse = !kn.dense && pl.rt <= kK3sMaxTiles ? 1 : 0;
    pl.slabs = k3.S0;
  } else {
    pl.k3_narrow = k3_narrow(cus, kn) ? 1 : 0;
    pl.k3_rows = k3_rows(pl.k3_narrow != 0);
    pl.slabs = k3_splits(pl.Bp, pl.k3_narrow != 0);
  }
  int wgs = 0;
  for (int i = 0; i < pl.n_jobs; ++i) {
    pl.job_splits[i] = v2 ? (i == 0 ? pl.S0 : pl.S1) : pl.slabs;
    pl.job_start[i] = wgs;
    wgs += pl.job_tiles[i] * pl.job_splits[i];
  }
  pl.job_start[pl.n_jobs] = wgs;
  return pl;
}

}  // namespace hbk
