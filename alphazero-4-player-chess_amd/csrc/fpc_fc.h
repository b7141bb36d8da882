// fpc_fc.h -- the policy Linear (net.py:25: A -> A, 553 M weights at 14x14 = 1.1 GB in 16 bit) as a weight-streaming
// GEMM for M = 256 rows: every weight byte is used once per forward, so the kernels are bound by the HBM stream
// (1.11 GB per launch; 283 GFLOP ride on it) and by whatever else travels the same L1 / L2 / LDS-DMA path.
//   k_fcw   (round 5; blob fc_layout 2; the default wherever its one-round K-split exists: every board of 8..14 a side on
//           a 256-CU part): 256 x 384 block tiles, one round of blocks -- see below.
//   k_fc16  (round 3; fc_layout 1; the fallback): 256 x 256 block tiles, long and short blocks in two rounds.
//   (k_fc, rounds 1-4: the same on v_mfma_f32_32x32x16 with its own fragment order -- retired in round 5; what it
//   established is kept in the notes below.)
// Common to both:
//   * W is stored by the exporter in MFMA FRAGMENT ORDER  [k-step of 32][column tile of 16][lane = 16 q + c][8]
//     (element (k32, nt, q, c, e) = W'[16 nt + c][32 k32 + 8 q + e]; k-step major: all waves advance through K together,
//     so what the chip reads at any moment is a few contiguous regions spread over every HBM channel): one A operand of a
//     wave is one contiguous, perfectly coalesced 1-KiB piece.
//   * A block is 4 waves, one per SIMD, each with the whole register file; a wave owns 64 (k_fc16) or 96 (k_fcw) output
//     columns for all 256 rows, issued as W x X^T: a lane owns ONE activation row and four consecutive output columns
//     per accumulator, so a partial tile leaves as one 16-byte store per lane.
//   * The weight pieces carry the non-temporal hint: 1.1 GB read once per launch would otherwise push the
//     activations, the tower's weights and the tree out of L2 / MALL (same-box A/B: +2.6 % on the whole step).
//   * Both operands arrive by LDS-DMA (global_load_lds_dwordx4, no VGPR hop): the activations X[256][K]
//     (12 MB, L2 resident, re-read by every column group) in full 128-byte lines into 32 KiB stage buffers shared by
//     the block (XOR-swizzled through the source address), the weights into a private ring per wave from which each
//     lane reads back exactly the 16 bytes it stored.
//   * Work = column group x K-split; block ids put the K-split in the low bits, so one XCD (id mod 8) only ever walks
//     one K window of X and keeps it in its own L2.  Every block writes its f32 partial slab [Mtot][group width];
//     k_fc_reduce adds a group's slabs and the bias in a fixed order (deterministic, no atomics).
//   * The first MFMA on every accumulator takes C = 0 as an inline constant.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "fpc_tower.h"   // M16: the 16x16x32 MFMA wrappers

namespace fpc {

struct FcArgs {
  const uint16_t *X;      // [Mpad][Kp]
  const uint16_t *Wf;     // fragment order
  float *part;            // [slabs][Mtot][256]
  int Kp, Np, ksteps, Mtot;
  int G1, s1, s2;         // groups [0,G1): s1 splits; groups [G1, Np/256): s2 splits
  // live-row numbering (fpc_search_set_live_rows; null: off, or a single row tile): rows *n_live.. of X are dead, and a
  // block whose 256-row tile holds none of the live ones returns before it touches memory -- the weights are streamed
  // ceil(*n_live / 256) times, not once per tile of the batch.  The dead tiles' slabs keep what they held; nobody reads them.
  // The host launches the LIVE instantiation of the kernels only with a non-null pointer: behind a null TEST the compiler
  // holds every other kernel-argument load back until the pointer has arrived (a second scalar round trip at the head of
  // every block), so the null case is a kernel of its own whose instruction stream is the one it was before.
  const int *n_live;
};

constexpr int FC_THREADS = 256;
constexpr int FC_XBUF = 256 * 64 * 2;             // one BK = 64 stage of activations: 32 KiB
constexpr int FC_WRING = 16 * 1024;               // per wave: 2 stages x 4 k-steps x 2 column tiles x 1 KiB
constexpr int FC_LDS = 3 * FC_XBUF + 4 * FC_WRING;   // 163840: the whole LDS of a CU

// one 1-KiB LDS-DMA piece (64 lanes x 16 B): global (SGPR base + per-lane byte offset) -> LDS, no VGPR
// destination.  Inline asm on purpose: every wait for these pieces is an explicit counted s_waitcnt in
// k_fc16.  M0 carries the wave-uniform LDS byte address and is restored inside the statement.  (k_fc16's form; k_fcw and
// k_fcw8 own M0 and write it once per group of pieces: fcw_set_m0 below.)
__device__ __forceinline__ void fc_dma(const void *gsrc_uniform, uint32_t lane_off, uint32_t lds_addr_uniform) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(lane_off), "s"(gsrc_uniform), "s"(lds_addr_uniform) : "memory");
}
// two consecutive pieces (source and destination both advance by 1 KiB: the instruction's immediate moves BOTH
// addresses, tools/micro/dma_imm_check.cpp) behind ONE write of M0: an s_mov to M0 waits for the wave's LDS reads
// in flight (~20 cycles beside a fragment stream, tools/micro/dma_stagger.cpp), the piece itself costs ~6
__device__ __forceinline__ void fc_dma2_nt(const void *gsrc_uniform, uint32_t lane_off, uint32_t lds_addr_uniform) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\t"
               "global_load_lds_dwordx4 %1, %2 offset:1024 nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(lane_off), "s"(gsrc_uniform), "s"(lds_addr_uniform) : "memory");
}

// k_fcw / k_fcw8: the kernel OWNS M0 from its first piece to its last -- no save, no restore (the compiler has no use
// for M0 in these kernels: no other M0 in their ISA).  M0 is written once per GROUP of pieces that lie back to back in
// LDS (fcw_set_m0: the group's LDS byte address + MID), and every piece of the group is one instruction whose immediate
// I * 1024 - MID (within -4096 .. 3072) moves the LDS destination AND the global source: the caller's source address
// (scalar base + per-lane offset) is the piece's own minus that immediate.
__device__ __forceinline__ void fcw_set_m0(uint32_t lds_addr_uniform) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(lds_addr_uniform) : "memory");
}
template <int OFF, bool NT>
__device__ __forceinline__ void fcw_piece(const void *gsrc_uniform, uint32_t lane_off) {
  static_assert(OFF >= -4096 && OFF <= 3072 && OFF % 1024 == 0, "a piece's immediate");
  if (NT) asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2 nt" : : "v"(lane_off), "s"(gsrc_uniform), "i"(OFF) : "memory");
  else asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" : : "v"(lane_off), "s"(gsrc_uniform), "i"(OFF) : "memory");
}
// piece i of a group of N (i is a constant wherever this is called: the tile-row loops are unrolled)
template <int MID, int N, bool NT, int I = 0>
__device__ __forceinline__ void fcw_piece_at(int i, const void *gsrc_uniform, uint32_t lane_off) {
  if constexpr (I < N) {
    if (i == I) fcw_piece<I * 1024 - MID, NT>(gsrc_uniform, lane_off);
    else fcw_piece_at<MID, N, NT, I + 1>(i, gsrc_uniform, lane_off);
  }
}
constexpr int FCW_XMID = 4096;    // the 8 activation pieces of a wave and stage: immediates -4096 .. 3072
constexpr int FCW_WMID = 3072;    // k_fcw: the 6 weight pieces of a k-step: -3072 .. 2048
constexpr int FCW8_WMID = 1024;   // k_fcw8: the 3 weight pieces of a k-step: -1024 .. 1024

// ------------------------------------------------------------------------------------------------------------
// k_fc16: the Linear on v_mfma_f32_16x16x32 (the shape the chip holds the higher clock on under load,
// MI355X_MICROARCH.md "DVFS give-back" item 7; k_tower uses it for the same reason) with 256 x 256 block tiles:
//   * a wave owns 64 columns x 256 rows = 16 x 4 accumulator tiles (256 AGPRs); every activation fragment read from LDS
//     feeds four MFMAs, and the fragment reads run a whole k-step ahead of their use (two sets of 16);
//   * three 32 KiB activation stages + a 16 KiB weight ring per wave (2 stages x 2 k-steps x 4 tiles); BOTH streams run
//     the same two stages ahead: vmcnt retires in issue order, so waiting for a young activation piece would otherwise
//     force every older, deeper weight fragment to have landed and cut the weight prefetch to a fraction of its ring;
//   * column groups [0, G1) are cut into s1 K-splits, the remaining groups into s2 = 2 * s1 half-length ones, G1
//     chosen by the host so that the short blocks fill the tail of the last round (plan_fc);
//   * a k-step is 32 deep: 64 MFMAs on 16 activation fragments x 4 weight fragments; 8 DMA pieces per k-step in the
//     fixed order  X, W, W, X, X, W, W, X  (the weight pieces in pairs behind one M0 write).  Counted waits:
//     first k-step of a stage: the weights of its second k-step were issued three k-steps ago; behind their last
//     piece came 1 + 8 + 8 pieces -> vmcnt(17); second k-step: the activations of the next stage (last piece: two
//     k-steps ago) and everything older -> vmcnt(8), then THE stage barrier.
template <int DT, bool LIVE = false>
__global__ void __launch_bounds__(FC_THREADS, 1) k_fc16(FcArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [3 X buffers][4 per-wave weight rings]
  if (LIVE && (int)blockIdx.y * 256 >= *g.n_live) return;    // block-uniform: a tile without a live row
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nbig = g.G1 * g.s1;
  const int id = blockIdx.x;
  const bool big = id < nbig;
  const int idr = big ? id : id - nbig;
  const int sk = big ? g.s1 : g.s2;
  const int group = big ? idr / sk : g.G1 + idr / sk;
  const int split = idr % sk;
  const int ntile = group * 16 + wave * 4;        // this wave's four 16-column tiles
  const int KS = g.ksteps / sk;                   // k-steps of 16 handled by this block; multiple of 8
  const int ks0 = split * KS;
  const int S = KS / 4;                           // stages of BK = 64 (even, >= 4)
  const long mrow0 = (long)blockIdx.y * 256;
  // weight stream of this wave: fragment (k32-step k, tile ntile + n) = 1 KiB at wbase + (k * Np/16 + n) KiB
  const unsigned char *wbase = reinterpret_cast<const unsigned char *>(g.Wf) + ((long)(ks0 / 2) * (g.Np / 16) + ntile) * 1024;
  const long wk32 = (long)(g.Np / 16) * 1024;
  const uint32_t wlane = (uint32_t)lane * 16u;
  const unsigned char *xbase = reinterpret_cast<const unsigned char *>(g.X) + ((mrow0 + wave * 64) * g.Kp + (long)ks0 * 16) * 2;
  const long xpiece = 8L * g.Kp * 2;
  uint32_t xlane[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int j = (lane & 7) ^ ((par * 4 + (lane >> 4)) & 7);
    xlane[par] = (uint32_t)((lane >> 3) * g.Kp * 2 + j * 16);
  }
  const uint32_t lds_x = 0, lds_w = (uint32_t)(3 * FC_XBUF + wave * FC_WRING);
  const unsigned char *wr = smem + 3 * FC_XBUF + wave * FC_WRING + lane * 16;

  f32x4_t acc[16][4];
  u32x4_t xf[2][16], wf[2][4];
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  const std::integral_constant<int, 0> c0{};
  const std::integral_constant<int, 1> c1{};

  auto issue_x = [&](int s, int p) {              // piece p (8 rows) of activation stage s
    const int sc = s < S ? s : S - 1;
    fc_dma(xbase + (long)p * xpiece + (long)sc * 128, xlane[p & 1],
           (uint32_t)__builtin_amdgcn_readfirstlane(lds_x + (s % 3) * FC_XBUF + (wave * 64 + p * 8) * 128));
  };
  auto issue_w2 = [&](int s, int j, int n0) {      // column tiles n0, n0 + 1 of k32-step j of stage s
    const int sc = s < S ? s : S - 1;
    fc_dma2_nt(wbase + (long)(2 * sc + j) * wk32 + n0 * 1024, wlane,
               (uint32_t)__builtin_amdgcn_readfirstlane(lds_w + ((s & 1) * 8 + j * 4 + n0) * 1024));
  };
  auto xfrag = [&](int b, int t, const unsigned char *ab, int j) {
    xf[b][t] = *reinterpret_cast<const u32x4_t *>(ab + lds_off<64>(t * 16 + (lane & 15), j * 4 + (lane >> 4)));
  };
  auto wfrag = [&](int b, int s, int j) {
#pragma unroll
    for (int n = 0; n < 4; ++n) wf[b][n] = *reinterpret_cast<const u32x4_t *>(wr + ((s & 1) * 8 + j * 4 + n) * 1024);
  };
  auto kstep = [&](auto j_c, auto z_c, int s) {
    constexpr int J = decltype(j_c)::value;
    constexpr bool Z = decltype(z_c)::value != 0;
    constexpr int CUR = J, NXT = J ^ 1;
    if (J == 0) asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
    if (J == 1) { asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); __syncthreads(); }
    const unsigned char *ab = smem + ((J == 1 ? s + 1 : s) % 3) * FC_XBUF;
    constexpr int JN = J ^ 1;
    __builtin_amdgcn_sched_barrier(0);
    wfrag(NXT, J == 1 ? s + 1 : s, JN);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[t][n] = M16<DT>::mfma(wf[CUR][n], xf[CUR][t], Z ? zero4 : acc[t][n]);
      __builtin_amdgcn_sched_barrier(0);
      xfrag(NXT, t, ab, JN);
      if (t == 1) issue_x(s + 2, J * 4 + 0);
      if (t == 5) issue_w2(s + 2, J, 0);
      if (t == 7) issue_x(s + 2, J * 4 + 1);
      if (t == 9) issue_x(s + 2, J * 4 + 2);
      if (t == 13) issue_w2(s + 2, J, 2);
      if (t == 15) issue_x(s + 2, J * 4 + 3);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // prologue: stages 0 and 1 of both streams, then the fragments of (0, 0)
#pragma unroll
  for (int st = 0; st < 2; ++st) {
#pragma unroll
    for (int p = 0; p < 8; ++p) issue_x(st, p);
#pragma unroll
    for (int j = 0; j < 2; ++j) { issue_w2(st, j, 0); issue_w2(st, j, 2); }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 16; ++t) xfrag(0, t, smem, 0);
  wfrag(0, 0, 0);

  kstep(c0, c1, 0);                               // (0, 0): C = 0
  kstep(c1, c0, 0);
#pragma unroll 1
  for (int s = 1; s < S; ++s) {
    kstep(c0, c0, s);
    kstep(c1, c0, s);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped tail pieces: nothing may still target LDS at exit

  const int slab = big ? id : nbig + idr;
  float *out = g.part + ((long)slab * g.Mtot + mrow0) * 256;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int m = t * 16 + (lane & 15);
#pragma unroll
    for (int n = 0; n < 4; ++n)
      *reinterpret_cast<f32x4_t *>(out + (long)m * 256 + wave * 64 + n * 16 + (lane >> 4) * 4) = acc[t][n];
  }
}

// ------------------------------------------------------------------------------------------------------------
// k_fcw (round 5): the same Linear on 256 x 384 block tiles -- the default (blob header fc_layout = 2).
//
// Why.  tools/micro/fc_stream.cpp replays k_fc16's memory pattern with the arithmetic taken out or left in (register
// operands, no LDS reads) and reproduces its 250 us; taken apart on one box: the weight stream alone 168 us (6.6 TB/s, the
// HBM rate), + the activation re-reads 214 (X is L2-resident, but its 1.1 GB -- every column group reads all of X --
// go through the same L1 / L2 / LDS-DMA path as the weights, at the core clock), + the MFMAs 252 (the clock drops under
// them and that path with it), + the 126 MB of split-K slabs 279.  Row pitch, a tiled X, rotated K order, deeper
// run-ahead, store flavours: within 3 %.  What does move it is the BYTES on that path:
//   * a block owns 384 columns instead of 256: 62 column groups instead of 92 read X -> 0.74 GB of re-reads (-1/3);
//   * 62 groups x 4 K-splits = 248 blocks = ONE round on 256 CUs (k_fc16: 256 long + 224 short blocks, two rounds
//     with a second ramp-up), every block the same length;
//   * 248 slabs of 256 x 384 f32 = 97 MB instead of 126 MB, four per column, all groups alike.
//   Same-box micro-benchmark with slabs and MFMAs: 308 -> 243 us.
// How.  A wave owns 96 columns x 256 rows = 16 x 6 accumulator tiles of 16 x 16 (384 registers), so the operand
// registers had to shrink: the activation fragments are a RING OF FOUR quads (fragment t + 3 is read while tile row t
// multiplies; k_fc16 holds two whole k-steps of 16), the six weight fragments are double-buffered as before.
// LDS: two activation stages (64 KiB; k_fc16: three) + a 24 KiB weight ring per wave (2 stages x 2 k-steps x 6 tiles)
// = 160 KiB.  The activations therefore run ONE stage ahead and the weights two; vmcnt retires in issue order, so
// within a stage the activation pieces go out FIRST (k-step 0, tile rows 0..7) and the weight pieces behind them:
// waiting for the youngest activation piece then leaves the twelve weight pieces issued behind it in flight.
// Issue pattern per stage and wave: k-step 0: 8 X pieces (behind tile rows 0..7), then 3 weight pairs (rows 8, 10, 12);
// k-step 1: 3 weight pairs (rows 2, 6, 10).  The 20 pieces are three GROUPS, each contiguous in LDS, each behind ONE write
// of M0 (fcw_set_m0 + fcw_piece_at above; the kernel owns M0, nothing saves or restores it):
//   X  -- the wave's 64 rows of the next stage, 8 KiB; M0 = its middle, immediates -4096 .. 3072.  In memory the eight
//         pieces are 8 rows (8 * Kp * 2 bytes) apart, not 1 KiB: piece p's scalar base carries p * (8 * Kp * 2 - 1024),
//         strength-reduced by the compiler to eight loop-invariant SGPR pairs + the stage offset (no VGPR more: 206 + 256);
//   W0 -- the six tiles of k-step 0 two stages ahead, 6 KiB of the ring and 6 KiB of the weight stream, both advancing by
//         1 KiB per tile: one base, M0 = middle, immediates -3072 .. 2048;
//   W1 -- the same for k-step 1 (the source a k-step of wk32 bytes further on).
// 3 M0 writes per stage where the per-statement form had 28 (save, set, restore per statement; an s_mov to M0 beside the
// fragment stream waits for the wave's LDS reads in flight).  Piece count, order and tile rows are unchanged, so the
// counted waits are:
//   start of k-step (s, 0): the weights of (s, 1), issued in (s - 2, 1); behind them a whole stage       -> vmcnt(20)
//   start of k-step (s, 1): the weights of (s + 1, 0), issued in (s - 1, 0); behind them 6 + 8 + 6       -> vmcnt(20)
//   k-step (s, 1) behind tile row 13: the activations of stage s + 1, issued in (s, 0); behind them 6 + 6 -> vmcnt(12),
//   then THE stage barrier: every wave's pieces of stage s + 1 have landed, and every wave has read its last fragment
//   of stage s (fragment 15 of k-step 1 is read behind tile row 12), so the buffer of stage s may be refilled.
// Weight order in memory: as k_fc16's, [k-step of 32][column tile of 16][lane][8] over Np = 384 * groups columns.
// Summation order: a column's K quarter in ascending k inside the MFMA accumulators, then bias + the four slabs
// ascending (k_fc_reduce / logit_at): other last bits than k_fc16's where that used eight slabs.
// One v_mfma_f32_16x16x32 with its accumulator PINNED to a register class: AG = true -> an AGPR quad, false -> a VGPR quad.
// k_fcw keeps 384 accumulator registers per lane; left to itself hipcc parks all of them in the 256 AGPRs by turns and
// moves 66 tiles through v_accvgpr_read / _write on every stage (528 moves + 142 s_nop per 192 MFMAs).  With the class
// in the constraint, 64 tiles live in a0..a255, 32 in VGPRs, and nothing moves.  (Inline asm: the compiler adds the
// lgkmcnt wait for the fragment registers it loaded itself; there is no MFMA -> MFMA dependency closer than 95 MFMAs.)
template <int DT, bool AG, bool Z>
__device__ __forceinline__ void fcw_mfma(f32x4_t &acc, const u32x4_t &a, const u32x4_t &b) {
  if (DT == 1) {
    if (AG) { if (Z) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b)); else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b)); }
    else    { if (Z) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=v"(acc) : "v"(a), "v"(b)); else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b)); }
  } else {
    if (AG) { if (Z) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b)); else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b)); }
    else    { if (Z) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=v"(acc) : "v"(a), "v"(b)); else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b)); }
  }
}

constexpr int FCW_COLS = 384;
constexpr int FCW_WRING = 24 * 1024;
constexpr int FCW_LDS = 2 * FC_XBUF + 4 * FCW_WRING;   // 163840

template <int DT, bool LIVE = false>
__global__ void __launch_bounds__(FC_THREADS, 1) k_fcw(FcArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2 X buffers][4 per-wave weight rings]
  if (LIVE && (int)blockIdx.y * 256 >= *g.n_live) return;    // block-uniform: a tile without a live row
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sk = g.s1;                            // K-splits per column group (every group alike)
  const int id = blockIdx.x;
  const int group = id / sk, split = id % sk;     // the K-split in the low bits: an XCD walks one K window of X
  const int ntile = group * 24 + wave * 6;        // this wave's six 16-column tiles
  const int KS = g.ksteps / sk;                   // k-steps of 16 handled by this block
  const int ks0 = split * KS;
  const int S = KS / 4;                           // stages of BK = 64
  const long mrow0 = (long)blockIdx.y * 256;
  const unsigned char *wbase = reinterpret_cast<const unsigned char *>(g.Wf) + ((long)(ks0 / 2) * (g.Np / 16) + ntile) * 1024;
  const long wk32 = (long)(g.Np / 16) * 1024;
  const uint32_t wlane = (uint32_t)lane * 16u;
  const unsigned char *xbase = reinterpret_cast<const unsigned char *>(g.X) + ((mrow0 + wave * 64) * g.Kp + (long)ks0 * 16) * 2;
  const long xpiece = 8L * g.Kp * 2;
  uint32_t xlane[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int j = (lane & 7) ^ ((par * 4 + (lane >> 4)) & 7);
    xlane[par] = (uint32_t)((lane >> 3) * g.Kp * 2 + j * 16);
  }
  const uint32_t lds_w = (uint32_t)(2 * FC_XBUF + wave * FCW_WRING);
  const unsigned char *wr = smem + 2 * FC_XBUF + wave * FCW_WRING + lane * 16;

  f32x4_t acc[16][6];
  u32x4_t xr[4], wf[2][6];
  const std::integral_constant<int, 0> c0{};
  const std::integral_constant<int, 1> c1{};

  // Group X: M0 = the middle of the wave's 8 KiB of stage s; piece p (8 rows) lands at M0 + (p * 1024 - FCW_XMID) and
  // comes from the scalar base + the same immediate: the base carries p * xpiece minus that immediate
  auto m0_x = [&](int s) { fcw_set_m0((uint32_t)__builtin_amdgcn_readfirstlane((s & 1) * FC_XBUF + wave * 64 * 128 + FCW_XMID)); };
  auto issue_x = [&](int s, int p) {              // piece p of activation stage s
    const int sc = s < S ? s : S - 1;
    fcw_piece_at<FCW_XMID, 8, false>(p, xbase + (long)p * (xpiece - 1024) + FCW_XMID + (long)sc * 128, xlane[p & 1]);
  };
  // Groups W0 / W1: M0 = the middle of the six tiles of k32-step j of stage s in the ring; source and ring both advance
  // by 1 KiB per tile, so one base (+ FCW_WMID) serves the six pieces
  auto m0_w = [&](int s, int j) { fcw_set_m0((uint32_t)__builtin_amdgcn_readfirstlane(lds_w + ((s & 1) * 12 + j * 6) * 1024 + FCW_WMID)); };
  auto issue_w2 = [&](int s, int j, int n0) {      // column tiles n0, n0 + 1 of k32-step j of stage s
    const int sc = s < S ? s : S - 1;
    const unsigned char *src = wbase + (long)(2 * sc + j) * wk32 + FCW_WMID;
    fcw_piece_at<FCW_WMID, 6, true>(n0, src, wlane);
    fcw_piece_at<FCW_WMID, 6, true>(n0 + 1, src, wlane);
  };
  auto xfrag = [&](int slot, int t, const unsigned char *ab, int j) {
    xr[slot] = *reinterpret_cast<const u32x4_t *>(ab + lds_off<64>(t * 16 + (lane & 15), j * 4 + (lane >> 4)));
  };
  auto wfrag = [&](int b, int s, int j) {
#pragma unroll
    for (int n = 0; n < 6; ++n) wf[b][n] = *reinterpret_cast<const u32x4_t *>(wr + ((s & 1) * 12 + j * 6 + n) * 1024);
  };
  auto kstep = [&](auto j_c, auto z_c, int s) {
    constexpr int J = decltype(j_c)::value;
    constexpr bool Z = decltype(z_c)::value != 0;
    constexpr int CUR = J, NXT = J ^ 1;
    asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    const unsigned char *ab = smem + (s & 1) * FC_XBUF;                                  // this stage's activations
    const unsigned char *abn = J == 1 ? smem + ((s + 1) & 1) * FC_XBUF : ab;             // the next k-step's
    __builtin_amdgcn_sched_barrier(0);
    wfrag(NXT, J == 1 ? s + 1 : s, NXT);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
#pragma unroll
      for (int n = 0; n < 6; ++n) {
        if (n < 4) fcw_mfma<DT, true, Z>(acc[t][n], wf[CUR][n], xr[t & 3]);
        else fcw_mfma<DT, false, Z>(acc[t][n], wf[CUR][n], xr[t & 3]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (J == 1 && t == 13) { asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); __syncthreads(); }
      if (t + 3 < 16) xfrag((t + 3) & 3, t + 3, ab, J);
      else xfrag((t + 3) & 3, t + 3 - 16, abn, NXT);
      if (J == 0 && t == 0) m0_x(s + 1);
      if (J == 0 && t < 8) issue_x(s + 1, t);
      if (J == 0 && t == 8) m0_w(s + 2, 0);
      if (J == 0 && (t == 8 || t == 10 || t == 12)) issue_w2(s + 2, 0, t - 8);
      if (J == 1 && t == 2) m0_w(s + 2, 1);
      if (J == 1 && (t == 2 || t == 6 || t == 10)) issue_w2(s + 2, 1, (t - 2) / 2);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // prologue: the activations of stage 0, the weights of stages 0 and 1, then the first fragments
  m0_x(0);
#pragma unroll
  for (int p = 0; p < 8; ++p) issue_x(0, p);
#pragma unroll
  for (int st = 0; st < 2; ++st)
#pragma unroll
    for (int j = 0; j < 2; ++j) { m0_w(st, j); issue_w2(st, j, 0); issue_w2(st, j, 2); issue_w2(st, j, 4); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 3; ++t) xfrag(t, t, smem, 0);
  wfrag(0, 0, 0);

  kstep(c0, c1, 0);                               // (0, 0): C = 0
  kstep(c1, c0, 0);
#pragma unroll 1
  for (int s = 1; s < S; ++s) {
    kstep(c0, c0, s);
    kstep(c1, c0, s);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped tail pieces: nothing may still target LDS at exit
  // The MFMAs above are inline asm: hipcc's hazard recogniser does not see them, so the wait states the ISA asks for between
  // an 8-pass MFMA writing a register and a store / v_accvgpr_read reading it (11) are spelt out here, once, behind the loop.
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");

  float *out = g.part + ((long)id * g.Mtot + mrow0) * FCW_COLS;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int m = t * 16 + (lane & 15);
#pragma unroll
    for (int n = 0; n < 6; ++n)
      *reinterpret_cast<f32x4_t *>(out + (long)m * FCW_COLS + wave * 96 + n * 16 + (lane >> 4) * 4) = acc[t][n];
  }
}

// ------------------------------------------------------------------------------------------------------------
// Round 4, built, measured and NOT kept (same-box A/Bs, both variants bit-identical to k_fc16): the recipe that took the hidden-256 tower from 0.36 to 0.49 of peak (fpc_towerw.h: two waves
// per SIMD, weights straight from memory into registers three k-steps ahead by counted-vmcnt inline-asm loads, no
// weight ring in LDS, activations by LDS-DMA as here) does NOT carry over to this Linear:
//   * k_fc16w, wave = 128 rows x 64 columns (two waves share every weight fragment): 0.364 ms with the non-temporal hint
//     on the weight loads (the second wave's request misses too: HBM sees the weights twice), 0.307 ms without it;
//   * k_fc16n, wave = 256 rows x 32 columns (every fragment has one owner, nt kept, twice the activation reads per
//     MFMA): 0.277-0.292 ms against k_fc16's 0.272-0.280 ms, and k_tower beside it 2 % slower (power).
// So the issue port is not what holds this kernel (k_fc16's MFMA pipe is idle 48 % of the time WAITING FOR DATA): the
// bound is the memory side -- 1.17 GB of weights from HBM + 1.1 GB of activation re-reads and 0.13 GB of slab writes
// through the same L2s.
// A lesson worth keeping from the one GPU fault of that work: an inline-asm load into a register the compiler considers
// DEAD (the clamped tail prefetches behind the last k-step) is still in flight when hipcc hands that register to later
// code -- the epilogue's address arithmetic sat in front of the plain `s_waitcnt vmcnt(0)` statement, a late-landing
// fragment overwrote a store address, the kernel faulted.  A wait that must cover asm loads has to be TIED to their
// destination registers ("+v" operands of the s_waitcnt statement), also for loads whose data nobody reads.
// ------------------------------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------------------------------
// k_fcw8 (opt-in, blob version 4 / fc_wtype 1, fp16 operands): k_fcw with the weight stream in int8 -- half the bytes of
// the one stream the kernel is bound by (0.55 GB instead of 1.11 GB at 14x14), everything behind the slabs unchanged.
// Numbers: q = the exporter's int8 with one f32 scale s_n per output column; a block accumulates
// X . fp16(q)^T over its K part in the MFMAs (the conversion is exact), multiplies every accumulator element ONCE by its
// column's s_n in f32 and stores the slab where and how k_fcw does: slab_k = fl(s_n * acc_k); k_fc_reduce / logit_at add
// bias + slabs as before.
// Weight order in memory: FRAGMENT PAIRS [k-step of 32][column pair of 32][lane = 16 q + c][2 tiles][8] bytes -- one
// 1-KiB LDS-DMA piece is 64 lanes x 16 B = the fragments of TWO column tiles, and a lane reads back exactly the 16 bytes
// it stored (the property the private ring rests on).  A wave's six tiles of a k-step are three contiguous pieces
// (ntile = group * 24 + wave * 6 is even).
// Schedule: k_fcw's.  Two activation stages (64 KiB) + a 12 KiB ring per wave (2 stages x 2 k-steps x 3 pieces) =
// 112 KiB of LDS; the 48 KiB this frees are NOT spent (a deeper ring only behind a same-box A/B).  Issue pattern per
// stage and wave: k-step 0: 8 X pieces (tile rows 0..7), then 3 weight pieces (rows 8, 10, 12); k-step 1: 3 weight pieces
// (rows 2, 6, 10) -- k_fcw's three groups behind one M0 write each, a weight group being the 3 KiB of a k-step's three
// pair pieces (M0 = the second piece, immediates -1024 .. 1024).  Counted waits, derived as k_fcw's:
//   start of k-step (s, 0): the weights of (s, 1), issued in (s - 2, 1); behind them stage s - 1: 8 + 3 + 3   -> vmcnt(14)
//   start of k-step (s, 1): the weights of (s + 1, 0), issued in (s - 1, 0); behind them 3 + 8 + 3             -> vmcnt(14)
//   k-step (s, 1) behind tile row 13: the activations of stage s + 1, issued in (s, 0); behind them 3 + 3      -> vmcnt(6),
//   then the stage barrier, as in k_fcw.
// All of these loads are LDS-DMA pieces: none has a destination register, so the lesson above (waits tied to the
// registers of asm loads) has nothing to tie here; the plain statements with a memory clobber are k_fcw's.
// Fragments: at the start of k-step j the three raw pieces of k-step j + 1 are read (one u32x4 per lane and tile pair)
// and converted during tile rows 1, 3 and 5 of k-step j into the six fp16 fragments the MFMAs of k-step j + 1 take:
// per 32-bit word of four bytes  x = w ^ 0x80808080 (q + 128 as an unsigned byte), two v_perm_b32 put each byte under a
// 0x64 (fp16 0x64uu = 1024 + u), one v_pk_add_f16 per pair subtracts 1152 -- exact for all 256 bytes.  The MFMAs are
// inline asm, which the compiler's hazard recogniser does not look into: no converted register is consumed sooner than
// 60 MFMAs after the VALU instruction that wrote it.
struct Fc8Args {
  FcArgs f;               // Wf: the int8 weights in pair order
  const float *scale;     // [Np]
};

constexpr int FCW8_WRING = 12 * 1024;
constexpr int FCW8_LDS = 2 * FC_XBUF + 4 * FCW8_WRING;   // 114688

// four int8 (one 32-bit word, two's complement) -> four fp16 in two words, element order kept
__device__ __forceinline__ void fc8_cvt4(uint32_t w, uint32_t &lo, uint32_t &hi) {
  typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
  const uint32_t x = w ^ 0x80808080u;
  const h2_t bias = {(_Float16)-1152.f, (_Float16)-1152.f};
  const h2_t a = __builtin_bit_cast(h2_t, __builtin_amdgcn_perm(0x64646464u, x, 0x04010400u)) + bias;
  const h2_t b = __builtin_bit_cast(h2_t, __builtin_amdgcn_perm(0x64646464u, x, 0x04030402u)) + bias;
  lo = __builtin_bit_cast(uint32_t, a);
  hi = __builtin_bit_cast(uint32_t, b);
}

template <bool LIVE = false>
__global__ void __launch_bounds__(FC_THREADS, 1) k_fcw8(Fc8Args g8) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2 X buffers][4 per-wave weight rings]
  const FcArgs &g = g8.f;
  if (LIVE && (int)blockIdx.y * 256 >= *g.n_live) return;    // block-uniform: a tile without a live row
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sk = g.s1;
  const int id = blockIdx.x;
  const int group = id / sk, split = id % sk;
  const int npair = group * 12 + wave * 3;        // this wave's three column pairs (six 16-column tiles)
  const int KS = g.ksteps / sk;
  const int ks0 = split * KS;
  const int S = KS / 4;                           // stages of BK = 64
  const long mrow0 = (long)blockIdx.y * 256;
  const unsigned char *wbase = reinterpret_cast<const unsigned char *>(g.Wf) + ((long)(ks0 / 2) * (g.Np / 32) + npair) * 1024;
  const long wk32 = (long)(g.Np / 32) * 1024;
  const uint32_t wlane = (uint32_t)lane * 16u;
  const unsigned char *xbase = reinterpret_cast<const unsigned char *>(g.X) + ((mrow0 + wave * 64) * g.Kp + (long)ks0 * 16) * 2;
  const long xpiece = 8L * g.Kp * 2;
  uint32_t xlane[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int j = (lane & 7) ^ ((par * 4 + (lane >> 4)) & 7);
    xlane[par] = (uint32_t)((lane >> 3) * g.Kp * 2 + j * 16);
  }
  const uint32_t lds_w = (uint32_t)(2 * FC_XBUF + wave * FCW8_WRING);
  const unsigned char *wr = smem + 2 * FC_XBUF + wave * FCW8_WRING + lane * 16;

  f32x4_t acc[16][6];
  u32x4_t xr[4], wf[2][6], raw[3];
  const std::integral_constant<int, 0> c0{};
  const std::integral_constant<int, 1> c1{};

  // the groups and their M0 as in k_fcw; a weight group is the three pair pieces of a k-step
  auto m0_x = [&](int s) { fcw_set_m0((uint32_t)__builtin_amdgcn_readfirstlane((s & 1) * FC_XBUF + wave * 64 * 128 + FCW_XMID)); };
  auto issue_x = [&](int s, int p) {              // piece p (8 rows) of activation stage s
    const int sc = s < S ? s : S - 1;
    fcw_piece_at<FCW_XMID, 8, false>(p, xbase + (long)p * (xpiece - 1024) + FCW_XMID + (long)sc * 128, xlane[p & 1]);
  };
  auto m0_w = [&](int s, int j) { fcw_set_m0((uint32_t)__builtin_amdgcn_readfirstlane(lds_w + ((s & 1) * 6 + j * 3) * 1024 + FCW8_WMID)); };
  auto issue_w = [&](int s, int j, int p) {        // column pair p of k32-step j of stage s
    const int sc = s < S ? s : S - 1;
    fcw_piece_at<FCW8_WMID, 3, true>(p, wbase + (long)(2 * sc + j) * wk32 + FCW8_WMID, wlane);
  };
  auto xfrag = [&](int slot, int t, const unsigned char *ab, int j) {
    xr[slot] = *reinterpret_cast<const u32x4_t *>(ab + lds_off<64>(t * 16 + (lane & 15), j * 4 + (lane >> 4)));
  };
  auto wraw = [&](int s, int j) {
#pragma unroll
    for (int p = 0; p < 3; ++p) raw[p] = *reinterpret_cast<const u32x4_t *>(wr + ((s & 1) * 6 + j * 3 + p) * 1024);
  };
  auto wcvt = [&](int b, int p) {                  // raw pair p -> the fragments of tiles 2 p and 2 p + 1
    uint32_t o[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) fc8_cvt4(raw[p][i], o[2 * i], o[2 * i + 1]);
    wf[b][2 * p] = u32x4_t{o[0], o[1], o[2], o[3]};
    wf[b][2 * p + 1] = u32x4_t{o[4], o[5], o[6], o[7]};
  };
  auto kstep = [&](auto j_c, auto z_c, int s) {
    constexpr int J = decltype(j_c)::value;
    constexpr bool Z = decltype(z_c)::value != 0;
    constexpr int CUR = J, NXT = J ^ 1;
    asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
    const unsigned char *ab = smem + (s & 1) * FC_XBUF;                                  // this stage's activations
    const unsigned char *abn = J == 1 ? smem + ((s + 1) & 1) * FC_XBUF : ab;             // the next k-step's
    __builtin_amdgcn_sched_barrier(0);
    wraw(J == 1 ? s + 1 : s, NXT);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
#pragma unroll
      for (int n = 0; n < 6; ++n) {
        if (n < 4) fcw_mfma<1, true, Z>(acc[t][n], wf[CUR][n], xr[t & 3]);
        else fcw_mfma<1, false, Z>(acc[t][n], wf[CUR][n], xr[t & 3]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (J == 1 && t == 13) { asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); __syncthreads(); }
      if (t + 3 < 16) xfrag((t + 3) & 3, t + 3, ab, J);
      else xfrag((t + 3) & 3, t + 3 - 16, abn, NXT);
      if (t == 1 || t == 3 || t == 5) wcvt(NXT, (t - 1) / 2);
      if (J == 0 && t == 0) m0_x(s + 1);
      if (J == 0 && t < 8) issue_x(s + 1, t);
      if (J == 0 && t == 8) m0_w(s + 2, 0);
      if (J == 0 && (t == 8 || t == 10 || t == 12)) issue_w(s + 2, 0, (t - 8) / 2);
      if (J == 1 && t == 2) m0_w(s + 2, 1);
      if (J == 1 && (t == 2 || t == 6 || t == 10)) issue_w(s + 2, 1, (t - 2) / 4);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // prologue: the activations of stage 0, the weights of stages 0 and 1, then the first fragments
  m0_x(0);
#pragma unroll
  for (int p = 0; p < 8; ++p) issue_x(0, p);
#pragma unroll
  for (int st = 0; st < 2; ++st)
#pragma unroll
    for (int j = 0; j < 2; ++j) { m0_w(st, j); issue_w(st, j, 0); issue_w(st, j, 1); issue_w(st, j, 2); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 3; ++t) xfrag(t, t, smem, 0);
  wraw(0, 0);
#pragma unroll
  for (int p = 0; p < 3; ++p) wcvt(0, p);
  // the converted fragments of (0, 0) come out of VALU instructions right here: the wait states between a VALU write and
  // an MFMA read the compiler cannot count across the asm boundary
  asm volatile("s_nop 7" ::: "memory");

  kstep(c0, c1, 0);                               // (0, 0): C = 0
  kstep(c1, c0, 0);
#pragma unroll 1
  for (int s = 1; s < S; ++s) {
    kstep(c0, c0, s);
    kstep(c1, c0, s);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped tail pieces: nothing may still target LDS at exit
  // as in k_fcw: the wait states between an 8-pass MFMA writing a register and a v_accvgpr_read / VALU reading it
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");

  // the lane's 24 scales: six tiles x four consecutive columns
  f32x4_t sc[6];
  const float *scl = g8.scale + (long)group * FCW_COLS + wave * 96 + (lane >> 4) * 4;
#pragma unroll
  for (int n = 0; n < 6; ++n) sc[n] = *reinterpret_cast<const f32x4_t *>(scl + n * 16);
  float *out = g.part + ((long)id * g.Mtot + mrow0) * FCW_COLS;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int m = t * 16 + (lane & 15);
#pragma unroll
    for (int n = 0; n < 6; ++n)
      *reinterpret_cast<f32x4_t *>(out + (long)m * FCW_COLS + wave * 96 + n * 16 + (lane >> 4) * 4) = acc[t][n] * sc[n];
  }
}

// logits[m][n] = bias[n] + slab[base][m][n%256] + slab[base+1][m][n%256] + ...   (fixed order)
// Sums a column group's K-split slabs and the bias in fixed order, writes the logits, and -- while the
// block still holds its 1024 logits of the row in registers -- leaves that chunk's softmax statistics
// (softmax_chunk_stats, fpc_tree_kernels.h) for the expansion, which then never sweeps the row again.
// LIVE (n_live non-null, FcArgs): the rows at or beyond *n_live are dead -- their blocks return at once, their records stay.
template <bool LIVE = false>
__global__ void __launch_bounds__(256) k_fc_reduce(const float *part, const float *bias, int G1, int s1, int s2, int gw, int Mtot, int A,
                                                   int n_rows, const int *n_live, float *logits, float *stats) {
  __shared__ float red[8];
  const int q = blockIdx.x * 256 + threadIdx.x;         // float4 index within a row
  const int m = blockIdx.y;
  if (m >= n_rows || (LIVE && m >= *n_live)) return;
  const bool valid = q * 4 < A;
  float4 v{0.f, 0.f, 0.f, 0.f};
  if (valid) {
    const int j = gw == 256 ? q >> 6 : (q * 4) / gw;    // column group of gw columns (256: k_fc / k_fc16; 384: k_fcw)
    const int col = q * 4 - j * gw;
    const int base = j < G1 ? j * s1 : G1 * s1 + (j - G1) * s2, cnt = j < G1 ? s1 : s2;
    // logit_at's shape: the bias and all of the group's slab quads (at most LOGIT_MAX_SLABS = 2 * FC_SPLITK, plan_fc)
    // are requested before the first is added -- one memory round trip per thread, not 1 + cnt dependent ones (a
    // run-time trip count, one load and a full wait per trip, held the kernel at latency x concurrency: 5.2 TB/s
    // of slabs that k_fcw wrote microseconds earlier).  The additions and their order are what they were.
    float4 p[LOGIT_MAX_SLABS];
#pragma unroll
    for (int k = 0; k < LOGIT_MAX_SLABS; ++k)
      p[k] = k < cnt ? *reinterpret_cast<const float4 *>(part + ((long)(base + k) * Mtot + m) * gw + col) : float4{0.f, 0.f, 0.f, 0.f};
    v = *reinterpret_cast<const float4 *>(bias + q * 4);
#pragma unroll
    for (int k = 0; k < LOGIT_MAX_SLABS; ++k) {
      v.x = k < cnt ? v.x + p[k].x : v.x; v.y = k < cnt ? v.y + p[k].y : v.y;
      v.z = k < cnt ? v.z + p[k].z : v.z; v.w = k < cnt ? v.w + p[k].w : v.w;
    }
    if (logits) *reinterpret_cast<float4 *>(logits + (long)m * A + q * 4) = v;     // null: the fused search keeps only the records
  }
  softmax_chunk_stats(v, valid, red, stats + ((long)m * SM_MAXCH + blockIdx.x) * SM_REC);
}

}  // namespace fpc
