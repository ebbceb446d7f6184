// Kernel-argument structs and geometry constants of the speech-embedding conv
// stack, shared by the kernels (hbk_embed_exact.hip, hbk_embed_x3.hip,
// hbk_embed_band.hip, hbk_embed_stream.hip), their launcher (hbk_embed.hip) and
// the host planner (hbk_embed_plan.h). Plain C++17, no HIP header: the planner and its check
// (tests/embed_plan_check.cpp) build for the CPU. The unnamed namespace is part
// of the kernels' mangled names (their parameters are these structs), so it stays.
#pragma once

#include <cstdint>

namespace hbk {
namespace {

// ------------------------------------------------- generic chain kernels ----
constexpr int kThreads = 256;
constexpr int kMaxStages = 10;
constexpr int kMaxWin = 32;
constexpr int kLdsBudget = 78 * 1024;     // bytes per block: 2 blocks per CU
constexpr int kLdsBudgetCU = 156 * 1024;  // one block per CU

struct StageDesc {
  int kh, kw, cin, cinp, cout, coutp;
  int K, ksteps, act;
  float alpha;
  int w_off, b_off;  // floats into the chain's weight blob
};

struct ChainArgs {
  const float* in;
  float* out;
  const float* wblob;
  int64_t n_img;            // images (clips or windows)
  int64_t src_clip_stride;  // floats between source clips
  int src_row_stride;       // floats between source rows
  int ipc;                  // images per source clip
  int row_off[kMaxWin];     // source row offset of image (i % ipc)
  int C_src;
  int in_ph, in_pw;         // input max-pool
  int W_in;                 // chain input width after the input pool
  int out_ph, out_pw;       // output max-pool
  int H_out, W_out, C_out;  // chain output per image
  int64_t out_img_stride;   // floats between output images
  int G;                    // images per task
  int band;                 // output rows per task
  int n_bands;
  int shrink;               // sum over stages of kh - 1
  int n_stages;
  StageDesc st[kMaxStages];
  int wblob_floats;
  int wstride;              // row stride of packed weights
  int lds_x, lds_y, lds_w, lds_k;  // float offsets into dynamic LDS
};

constexpr int kXThreads = 256;

struct XStage {
  int kh, kw, cin, cout;
  int coutr;          // output channels written (cout rounded up to 8; the pad is exactly 0)
  int cs_in, cs_out;  // fp16 elements per position of the input / output tensor
  int ksteps;         // K steps of 16 (two 8-channel groups)
  int nblk;           // 32-wide output-channel blocks
  int act;
  float alpha;
  int w_off;          // fp16 offset of the hi plane [nblk * 32][wrow]
  int w_lo;           // fp16 distance hi -> lo plane
  int wrow;
  int b_off;          // float offset into the bias blob
  int kt_off;         // int offset of the stage's group-offset table
};

struct XArgs {
  const float* in;
  float* out;
  const _Float16* wblob;   // global weights (WG mode reads them here)
  const float* bblob;      // biases [per stage nblk * 32]
  const int* ktab;         // group offsets, all stages
  const int* i2c_off;      // im2col: raw-row offset of tap k = (dh kw + dw) C + ci
  int i2c_n;
  int64_t n_img;
  int64_t src_clip_stride;
  int src_row_stride;
  int ipc;
  int row_off[kMaxWin];
  int C_src, cs0;          // source channels; fp16 stride of the staged tensor
  int im2col;              // stage 0 input is the im2col expansion (K0 = kh kw cin)
  int in_ph, in_pw, W_in;
  int out_ph, out_pw, H_out, W_out, C_out;
  int64_t out_img_stride;
  int vec_out;             // C_out % 4 == 0 and 16-B aligned output: float4 stores
  int raw_vec;             // im2col staging reads float4 (in_pw == 1, aligned rows)
  int G, band, n_bands, shrink, n_stages;
  XStage st[kMaxStages];
  int w_halfs;             // resident weights (0: WG mode)
  int b_floats, kt_n;
  int lds_x, lds_y, lds_w, lds_b, lds_k;  // byte offsets into dynamic LDS
  int dbg_slot;            // phase-timing slot (chain index mod 4; profiling build only)
  int dbg_skip;            // profiling build only: bit 0 stages, 1 im2col, 2 store, 3 staging
  int* range_flag;         // set to 1 when an f16-split value reaches kF16Max
};

// The f16 planes hold |v| < 65504 (kF16Max): amax keeps the largest |v| a
// thread split (one v_max3 per pair; fmaxf drops NaN, which is not a range
// fault) and the kernel raises its plan's range flag when it reaches kF16Max.
constexpr float kF16Max = 65504.f;

// ------------------------------------------------------------------- p0 ----
constexpr int kP0Waves = 4;
constexpr int kP0Threads = 64 * kP0Waves;

struct P0Args {
  const float* in;          // [img][rows][WI] f32, row stride WI
  float* out;               // [img][H_out][W2 / 2][C] f32
  const _Float16* w;        // stage s: hi [32][16 ks_s], lo [32][16 ks_s]
  const float* bias;        // [3][32] (rows >= C are 0)
  int64_t n_img;
  int64_t src_img_stride;   // floats
  int H_in;                 // valid input rows per image
  int H_out;                // pooled output rows per image
  int n_bands;
  float alpha;              // LeakyReLU slope of all three convs (LEAKY kernels)
  int* range_flag;          // set to 1 when an f16-split value reaches kF16Max
};

template <int WI, int C, int BAND>
struct P0Geo {
  static constexpr int W0 = WI - 2, W1 = W0 - 2, W2 = W1;
  static constexpr int R2 = 2 * BAND, R1 = R2 + 2, R0 = R1, RI = R0 + 2;
  static constexpr int CS = ((C / 8) % 2 == 0) ? C + 8 : C;  // odd number of 16-B groups per position
  static constexpr int M0 = R0 * W0, M1 = R1 * W1, M2 = R2 * W2;
  static constexpr int T0 = (M0 + 31) / 32, T1 = (M1 + 31) / 32, T2 = (M2 + 31) / 32;
  static constexpr int KS = (3 * C + 15) / 16;  // K steps of stages 1 and 2
  static constexpr int RAW = RI * WI * 4;
  static constexpr int S0B = M0 * CS * 4, S1B = M1 * CS * 4, S2B = M2 * C * 4;
  static constexpr int XB = ((RAW > S1B ? RAW : S1B) + 15) & ~15;  // raw input, then stage-1 output
  static constexpr int YB = ((S0B > S2B ? S0B : S2B) + 15) & ~15;  // stage-0 output, then stage-2 f32
  static constexpr int LDS = XB + YB;
  static constexpr int WOFF1 = 2 * 32 * 16, WOFF2 = WOFF1 + 2 * 32 * 16 * KS;  // fp16 offsets
  static constexpr int WHALFS = WOFF2 + 2 * 32 * 16 * KS;
};

// ------------------------------------------------------------------- p1 ----
constexpr int kP1C = 32;

struct P1Args {
  const float* in;          // [img][H_in][WI][CI] f32
  float* out;               // [img][H_out][W4 / 2][32] f32
  const _Float16* w;        // stage s at woff[s]: hi [32][16 ks_s], lo [32][16 ks_s]
  const float* bias;        // [4][32]
  int64_t n_img;
  int64_t src_img_stride;   // floats
  int H_in, H_out, n_bands;
  float alpha;
  int* range_flag;          // set to 1 when an f16-split value reaches kF16Max
};

template <int WI, int CI, int BAND>
struct P1Geo {
  static constexpr int C = kP1C;
  static constexpr int W0 = WI, W1 = WI - 2, W2 = W1, W3 = W1 - 2, W4 = W3;
  static constexpr int R4 = 2 * BAND, R3 = R4 + 2, R2 = R3, R1 = R2 + 2, R0 = R1;
  static constexpr int CSI = ((CI / 8) % 2 == 0) ? CI + 8 : CI;
  static constexpr int CS = ((C / 8) % 2 == 0) ? C + 8 : C;
  static constexpr int M1 = R1 * W1, M2 = R2 * W2, M3 = R3 * W3, M4 = R4 * W4;
  static constexpr int KS1 = (3 * CI + 15) / 16, KS = (3 * C + 15) / 16;
  static constexpr int KSMAX = KS1 > KS ? KS1 : KS;
  static constexpr int INB = R0 * W0 * CSI * 4, S1B = M1 * CS * 4, S2B = M2 * CS * 4, S3B = M3 * CS * 4,
                       S4B = M4 * C * 4;
  static constexpr int mx(int a, int b) { return a > b ? a : b; }
  static constexpr int XB = (mx(mx(INB, S2B), S4B) + 15) & ~15;  // input, stage-2 out, stage-4 out (f32)
  static constexpr int YB = (mx(S1B, S3B) + 15) & ~15;            // stage-1 out, stage-3 out
  static constexpr int LDS = XB + YB;
  static constexpr int WOFF1 = 0, WOFF2 = WOFF1 + 2 * 32 * 16 * KS1, WOFF3 = WOFF2 + 2 * 32 * 16 * KS,
                       WOFF4 = WOFF3 + 2 * 32 * 16 * KS, WHALFS = WOFF4 + 2 * 32 * 16 * KS;
};

// ------------------------------------------------------------------ p0s ----
constexpr int kP0sWaves = 4;
constexpr int kP0sThreads = 64 * kP0sWaves;
constexpr int kP0sCS = 24;                         // fp16 per position (3 odd 16-B groups)
constexpr int kP0sS0Plane = 34 * kP0sCS;           // positions 0..33 (x + tap <= 33)
constexpr int kP0sS1Plane = 32 * kP0sCS;
constexpr int kP0sOnes = 4 * kP0sS0Plane + 8 * kP0sS1Plane;  // fp16 offset of the ones / zeros slots
constexpr int kP0sWaveHalfs = kP0sOnes + 16;
constexpr int kP0sLds = kP0sWaves * kP0sWaveHalfs * 2;
constexpr int kP0sKS = 5;                          // K steps of stages 1 and 2 (72 + bias slot)
constexpr int kP0sRows = 136, kP0sHout = 66, kP0sWout = 14, kP0sC = 24;

// ------------------------------------------------------------------ p1s ----
constexpr int kP1sThreads = 128;
constexpr int kP1sCSI = 24, kP1sCS = 40;          // fp16 per position: input (24 ch), stage outputs (32 ch)
constexpr int kP1sInPlane = 18 * kP1sCSI;         // 18 positions (14 valid; x + tap <= 17)
constexpr int kP1sInSlot = 2 * kP1sInPlane + 32;  // hi, lo, then ones (hi 8, lo 8) and zeros (hi 8, lo 8)
constexpr int kP1sPlane = 16 * kP1sCS;            // A / C rows
constexpr int kP1sBPlane = 18 * kP1sCS;           // B rows (c reads x + dx <= 17)
constexpr int kP1sIn = 0, kP1sA = kP1sIn + 2 * kP1sInSlot, kP1sB = kP1sA + 4 * 2 * kP1sPlane,
              kP1sCr = kP1sB + 2 * 2 * kP1sBPlane;
constexpr int kP1sHalfs = kP1sCr + 4 * 2 * kP1sPlane;
constexpr int kP1sLds = kP1sHalfs * 2;
constexpr int kP1sHin = 66, kP1sHout = 31, kP1sWi = 14, kP1sWo = 5, kP1sCo = 32;
constexpr int kP1sStageHalfs = 2 * 32 * 96;       // weights per stage: hi [32][96], lo [32][96]

// ------------------------------------------------------------------ p2s ----
constexpr int kP2sThreads = 512, kP2sClips = 16;
constexpr int kP2sHin = 31, kP2sWi = 5, kP2sCi = 32, kP2sCo = 48, kP2sHout = 27;
constexpr int kP2sCSI = 40, kP2sCS = 56;                      // fp16 per position (odd 16-B groups)
constexpr int kP2sInPlane = kP2sClips * kP2sWi * kP2sCSI;     // one input row of 16 clips
constexpr int kP2sAPlane = kP2sClips * 3 * kP2sCS;            // stage a / b output rows (3 columns)
constexpr int kP2sCPlane = kP2sClips * kP2sCS;                // stage c output rows (1 column)
constexpr int kP2sIn = 0, kP2sA = kP2sIn + 2 * 2 * kP2sInPlane, kP2sB = kP2sA + 4 * 2 * kP2sAPlane,
              kP2sC = kP2sB + 2 * 2 * kP2sAPlane, kP2sOnes = kP2sC + 4 * 2 * kP2sCPlane;
constexpr int kP2sHalfs = kP2sOnes + 32;
constexpr int kP2sLds = kP2sHalfs * 2;
constexpr int kP2sKa = 96, kP2sK = 160;                       // packed K of stage a / stages b, c, d
constexpr int kP2sTicks = 36;                                 // rows 0 .. 30 through a 7-tick pipeline

struct P2sArgs {
  const float* in;        // [img][31][5][32] f32
  float* out;             // [img][27][48] f32
  const _Float16* w;      // a: hi / lo [48][96]; b, c, d: hi / lo [48][160]
  const float* bias_a;    // [48]
  int64_t n_img, src_img_stride;
  float alpha;
  int* range_flag;
};

// ------------------------------------------------------------------ t3s ----
constexpr int kT3Waves = 10, kT3Threads = 64 * kT3Waves, kT3Pos = 16;
constexpr int kT3Hin = 27, kT3C0 = 48, kT3Hp = 13, kT3C1 = 64, kT3C2 = 96, kT3Hout = 8;
constexpr int kT3Ticks = 22;
constexpr int kT3CS0 = 56, kT3CS1 = 72, kT3CS2 = 104;  // f16 per position (odd 16-B groups)
// ring slots (rows) and LDS offsets (f16): P (pooled, 4), A1 (2), A2 (4), A3 (2), A4 (4), A5..A8 (2 each)
constexpr int kT3PlP = kT3Pos * kT3CS0, kT3Pl1 = kT3Pos * kT3CS1, kT3Pl2 = kT3Pos * kT3CS2;
constexpr int kT3P = 0, kT3A1 = kT3P + 4 * 2 * kT3PlP, kT3A2 = kT3A1 + 2 * 2 * kT3Pl1,
              kT3A3 = kT3A2 + 4 * 2 * kT3Pl1, kT3A4 = kT3A3 + 2 * 2 * kT3Pl1, kT3A5 = kT3A4 + 4 * 2 * kT3Pl1;
constexpr int kT3Zero = kT3A5 + 4 * 2 * 2 * kT3Pl2;  // 16 zero halfs (stage 1's K padding)
constexpr int kT3Halfs = kT3Zero + 16;
constexpr int kT3BiasOff = kT3Halfs * 2;            // bytes: biases [4][64] then [5][96] f32
constexpr int kT3Lds = kT3BiasOff + (4 * kT3C1 + 5 * kT3C2) * 4;
// weights (f16, hi plane then lo plane per stage, [cout][K], K = tap * cin + ci)
constexpr int kT3K[9] = {160, 64, 192, 64, 128, 96, 96, 96, 96};  // stage 1: 144 + 16 zero
constexpr int kT3W[9] = {0,
                         2 * 64 * 160,
                         2 * 64 * (160 + 64),
                         2 * 64 * (160 + 64 + 192),
                         2 * 64 * (160 + 64 + 192 + 64),
                         2 * 64 * 480 + 2 * 96 * 128,
                         2 * 64 * 480 + 2 * 96 * (128 + 96),
                         2 * 64 * 480 + 2 * 96 * (128 + 192),
                         2 * 64 * 480 + 2 * 96 * (128 + 288)};
constexpr int kT3WHalfs = 2 * 64 * 480 + 2 * 96 * 512;

struct T3sArgs {
  const float* in;      // [clip][27][48] f32 (p2s output)
  float* out;           // [image][8][96] f32, image = 2 clip + phase
  const _Float16* w;    // kT3WHalfs
  const float* bias;    // [4][64] + [5][96]
  int64_t n_img, src_clip_stride, out_img_stride;
  float alpha;
  int* range_flag;
};

}  // namespace
}  // namespace hbk
