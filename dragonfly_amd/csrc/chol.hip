// Blocked right-looking Cholesky and the inverses of its diagonal blocks (the triangular solves built on them are
// trsolve.hip; the one-workgroup tuning objective, which shares the 64 x 64 machinery of factor64.h, is lml_wg.h,
// compiled as part of this unit).
//
// Replaces np.linalg.cholesky (LAPACK dpotrf) at dragonfly/utils/general_utils.py:178,190 as used by
// GP.build_posterior (dragonfly/gp/gp_core.py:159-160).
//
// Structure (row-major lower, n x n):
//   outer panels of CHOL_NB = 512 columns; inside a panel the 512 x 512 diagonal block is
//   factored with 64-wide steps: one launch (diag_step64) factors the 64 x 64 pivot block in
//   registers and solves the 64-wide column below it by substitution, then the rest of the
//   diagonal block is updated by an MFMA SYRK.  The eight 64-block inverses (trtri64, one
//   launch) are then merged into the inverse of the 512 block by three
//   levels of batched GEMMs ([[A,0],[B,C]]^-1 = [[A^-1,0],[-C^-1 B A^-1, C^-1]]), so the panel
//   solve  L21 = A21 L11^-T  and the trailing update  A22 -= L21 L21^T  are two large MFMA_F64
//   GEMMs -- where n^3/3 of the flops are.  The 512-block inverses are kept: the posterior
//   solve (trsm_rows) and the alpha solves (trsv_*) of trsolve.hip reuse them, which turns every
//   triangular solve on the hot path into GEMM / GEMV work.
#include "common.h"
#include <cmath>
#include <functional>
#include <utility>
#include <math.h>
#include <stdlib.h>

namespace {

#include "factor64.h"   // factor64_waves and its helpers (PB, PBP, SPP, SYNC_ST_*, fast_rcp, perm16, quad_sum, ...)

// One 64-wide step of the diagonal-block factorisation, one launch:
//   workgroup 0     : factors the nb x nb pivot block at D and writes the factor to Lout;
//   workgroup b >= 1: factors the same block redundantly (bit-identical, no inter-workgroup
//                     hand-off needed) and solves 64 rows of the column below it,
//                     P[r,:] <- P[r,:] L^-T, by forward substitution with four lanes per row.
// info[0] <- pivot_base + j + 1 for the first non-positive / NaN pivot.
__global__ __launch_bounds__(256) void diag_step64_kernel(double* __restrict__ D, long lda, int nb,
                                                          int rows_below, long pivot_base,
                                                          long long* info, double* __restrict__ Lout,
                                                          long strideD, long strideL,
                                                          double* __restrict__ LinvOut, long strideI) {
  // batch element = blockIdx.y
  D += (long)blockIdx.y * strideD;
  Lout += (long)blockIdx.y * strideL;
  if (LinvOut) LinvOut += (long)blockIdx.y * strideI;
  long long* const info_dbg = info + CHOL_MAX_BATCH;   // debug words follow the pivot flags
  info += blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  double* Sp = dsm;                       // [64][SPP] factor, columns permuted by perm16
  double* R = dsm + PB * SPP;             // [64][65] panel rows
  double* colbuf = dsm + PB * SPP + PB * PBP;      // [64] reciprocal diagonal, then the column ring and its flags
  const int tid = threadIdx.x;
  const int k = tid & 63, w = tid >> 6;

  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  // stage the pivot block (identity padding beyond nb, zero above the diagonal), coalesced; it
  // sits in the Sp region, which wave 0 overwrites with the factor image only after reading it
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = w + 4 * r;
    double v = (i == k) ? 1.0 : 0.0;
    if (i < nb && k < nb) v = (k <= i) ? D[i * lda + k] : 0.0;
    Sp[i * SPP + k] = v;
  }
  __shared__ int s_badv[4];
  __shared__ int s_ring_timeout;
  double* ring = colbuf + PB;                      // [64][64] published (unscaled) columns
  double* tbuf0 = ring + PB * PB;                  // 3 x [64][17] layout buffers (later 4 x [16][17] solve tiles)
  double* lbb = tbuf0 + 3 * PB * 17;               // 4 x [16][17] diagonal 16-blocks of the factor
  double* linv = lbb + 4 * 16 * 17;                // 4 x [16][17] their inverses
  double* rdiag = colbuf;                          // [64] 1 / L[c][c]
  if (tid < PB) ring[tid * PB] = 0.0;              // row-0 entries double as the "published" flags
  if (tid == 0) s_ring_timeout = 0;
  __syncthreads();
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  const int r0 = ((int)blockIdx.x - 1) * PB;
  double* Pn = D + (long)(nb + r0) * lda;
  {
    double a[16];
    long long stamp[4] = {0, 0, 0, 0};
    const bool dbg = info_dbg[7] != 0 && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0;
    double* tbuf = tbuf0 + (w > 0 ? (w - 1) : 0) * PB * 17;
    const int bad = factor64_waves(a, k, w, Sp, tbuf, ring, lbb, linv, rdiag, &s_ring_timeout, dbg ? stamp : nullptr);
    if (k == 0) s_badv[w] = bad;
    if (dbg && k == 0) {
      // wave 3: start / end of its own 16 columns, end of scaling, end of the 16 x 16 inverse (debug hook only)
      if (w == 3) { info_dbg[0] = stamp[0] - (long long)t1; info_dbg[1] = stamp[1] - (long long)t1;
                    info_dbg[5] = stamp[2] - (long long)t1; info_dbg[6] = stamp[3] - (long long)t1; }
    }
    // factor image for the row solves: Sp[row][perm16(col)], and the reciprocal diagonal
#pragma unroll
    for (int j = 0; j < 16; ++j) Sp[k * SPP + perm16(16 * w + j)] = a[j];
    if (w == 0 && blockIdx.x > 0) {
      // wave 0 is done after the first 16 columns: it stages this workgroup's 64 panel rows
      // (coalesced along the row) while the other waves go on with the factorisation
      // (16 loads in flight at a time: one load per iteration would cost a full memory latency each)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double tmp[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 16 * c + r;
          tmp[r] = (r0 + i < rows_below && k < nb) ? Pn[i * lda + k] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) R[(16 * c + r) * PBP + k] = tmp[r];
      }
    }
  }
  __syncthreads();
  const unsigned long long t2 = __builtin_amdgcn_s_memtime();
  if (info_dbg[7] != 0 && tid == 0 && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0) { info_dbg[2] = (long long)(t1 - t0); info_dbg[3] = (long long)(t2 - t1); }
  const int s_bad = (s_badv[0] >= 0) ? s_badv[0] : (s_badv[1] >= 0) ? s_badv[1] : (s_badv[2] >= 0) ? s_badv[2] : s_badv[3];
  if (s_ring_timeout && tid == 0) atomicOr((unsigned long long*)(info_dbg + 8), (unsigned long long)SYNC_ST_RING);
  if (s_bad >= 0) {
    if (blockIdx.x == 0 && tid == 0 && info[0] == 0) info[0] = pivot_base + s_bad + 1;
    return;
  }
  if (blockIdx.x == 0) {
    // The factor goes to a scratch block (64 x 64, ld 64), NOT back into D: the other workgroups
    // of this launch re-read the unfactored pivot block from D and may start arbitrarily later.
    // trtri64_kernel moves it into place once the whole diagonal block is done.
    const int pk = perm16(k);
#pragma unroll
    for (int r = 0; r < 16; ++r) Lout[(w + 4 * r) * PB + k] = Sp[(w + 4 * r) * SPP + pk];
    // ... and the inverses of its four 16 x 16 diagonal blocks, for the strip kernel (same layout as in LDS)
    if (LinvOut)
      for (int i = tid; i < 4 * 16 * 17; i += 256) LinvOut[i] = linv[i];
    return;
  }
  {
    // Row solve X L^T = P on the matrix cores, 16-column blocks: for b = 0..3
    //     X_b = (P_b - sum_{b' < b} X_b' L[b][b']^T) Linv_bb^T
    // with the inverses of the four 16 x 16 diagonal blocks (computed by the waves that own them,
    // see factor64_waves).  Wave w takes rows 16w .. 16w+15 of the workgroup's 64: no dependence
    // between waves.  X_b goes back into R, from where the later blocks read it as an A operand;
    // the only layout change is accumulator -> A operand for the multiplication by Linv_bb^T, through
    // a 16 x 16 LDS tile private to the wave.  40 MFMAs per wave; the substitution this replaces was
    // a 64-step dependent chain (16k cycles).
    double* Tt = tbuf0 + w * (16 * 17);
    const int kq = k >> 4, l15 = k & 15;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      // two accumulators per product: a dependent MFMA waits ~64 cycles for its predecessor
      double4_t acc, acc2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = R[(16 * w + kq + 4 * r) * PBP + 16 * b + l15];
#pragma unroll
      for (int bp = 0; bp < b; ++bp)
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          const double av = R[(16 * w + l15) * PBP + 16 * bp + 4 * st + kq];                 // X_b'[i][k]
          const double bv = -Sp[(16 * b + l15) * SPP + perm16(16 * bp + 4 * st + kq)];       // -L[16b+j][16b'+k]
          if (st & 1) acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc2, 0, 0, 0);
          else acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
      for (int r = 0; r < 4; ++r) Tt[(kq + 4 * r) * 17 + l15] = acc[r] + acc2[r];
      COMPILER_BARRIER();                            // same wave: LDS executes its operations in order
      double4_t x = {0.0, 0.0, 0.0, 0.0}, x2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const double av = Tt[l15 * 17 + 4 * st + kq];                                        // T[i][k]
        const double bv = linv[b * (16 * 17) + l15 * 17 + 4 * st + kq];                      // Linv_bb[j][k]
        if (st & 1) x2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, x2, 0, 0, 0);
        else x = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, x, 0, 0, 0);
      }
      COMPILER_BARRIER();
#pragma unroll
      for (int r = 0; r < 4; ++r) R[(16 * w + kq + 4 * r) * PBP + 16 * b + l15] = x[r] + x2[r];
      COMPILER_BARRIER();
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = w + 4 * r;
    if (r0 + i < rows_below && k < nb) Pn[i * lda + k] = R[i * PBP + k];
  }
  if (info_dbg[7] != 0 && tid == 0 && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0) info_dbg[4] = (long long)(__builtin_amdgcn_s_memtime() - t2);
}

}  // namespace

#include "lml_wg.h"   // the one-workgroup / team tuning objective: its own file, this translation unit (see there for why)

namespace {

// ---------------------------------------------------------------------------------------------
// Panel strips.  Once the 512 x 512 diagonal block of a panel is factored, the rows below it are
//     L21 = A21 L11^-T ,
// and a strip of 64 of those rows needs nothing from any other strip: workgroup s keeps its
// 64 x 512 strip in the MFMA accumulators (16 rows x 512 columns per wave, 128 doubles per lane)
// and runs the eight 64-column steps locally --
//     X_j = (A_j - sum_{i<j} X_i L_ji^T) L_jj^-T      (the sum is already in the accumulators)
//     A_c -= X_j L_cj^T  for the later blocks c > j   (right-looking inside the strip)
// -- with the SAME row solve as diag_step64_kernel (16-column sub-blocks, the inverses of the
// 16 x 16 diagonal blocks exported by the workgroup that factored L_jj).  One launch replaces, for
// the rows below the diagonal block, the eight pivot steps (each workgroup re-factoring the pivot
// block) and the eight K = 64 updates that stream the rows x 448 panel through HBM.  Used for
// lock-step batches, where those two are what the pivot steps cost (cholesky_device); for a single
// matrix the chain is bound by launch latency and the strips do not pay.
// One wave per SIMD (the strip fills the register file): the 28 updates run at the fp64 matrix
// pipe's rate (64 cycles per MFMA), the row solves and the tile hand-over are latency -- 134 us per
// strip against 61 us of MFMA time.  Fully unrolled over (j, c): the accumulator index has to be
// static.
// LDS strides: an MFMA operand read takes element (row l15, column 4 st + kq) of a tile; with a
// row stride = 4 mod 32 doubles the 64 lanes cover all banks exactly twice (the minimum for 8 B).
constexpr int SK_LD = 68;      // 64-column tiles
constexpr int SK_TD = 20;      // 16-column tiles
constexpr int STRIP_SMEM = (2 * PB * SK_LD + 4 * 16 * SK_LD + 4 * 16 * SK_TD + 4 * 16 * SK_TD) * 8;

// The 36 tiles of L a strip consumes, in order: for j = 0..7 the diagonal factor block L_jj (with the
// inverses of its 16 x 16 diagonal blocks), then the sub-diagonal blocks L_cj, c = j+1..7.  They are
// fetched two tiles ahead into registers and handed over through two LDS buffers, one barrier per
// tile: the blocks were written by other XCDs a moment ago, every fetch is a full fabric round trip.
constexpr int SK_TILES = 36;
constexpr int sk_tile_j(int q) { int j = 0; while (q >= 8 - j) { q -= 8 - j; ++j; } return j; }
constexpr int sk_tile_c(int q) { int j = 0; while (q >= 8 - j) { q -= 8 - j; ++j; } return j + q; }

struct StripCtx {
  const double* Dblk; long lda; const double* Lfac; const double* Linv16;
  double* Pw; long rows_left;
  double* buf;        // 2 x [64][SK_LD]
  double* Xw; double* Tt; double* li;
};

template <int Q>
__device__ __forceinline__ void strip_fetch(const StripCtx& s, double (&pre)[16], double (&prei)[4]) {
  constexpr int J = sk_tile_j(Q), C = sk_tile_c(Q);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if constexpr (C == J) {
#pragma unroll
    for (int r = 0; r < 16; ++r) pre[r] = s.Lfac[J * PB * PB + (w + 4 * r) * PB + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = tid + 256 * r;                   // element of the [4][16][16] inverses
      prei[r] = s.Linv16[J * (4 * 16 * 17) + (i >> 8) * (16 * 17) + ((i >> 4) & 15) * 17 + (i & 15)];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) pre[r] = s.Dblk[(long)(C * PB + w + 4 * r) * s.lda + J * PB + lane];
  }
}

template <int Q>
__device__ __forceinline__ void strip_tile(const StripCtx& s, double4_t (&acc)[32], double (&xa)[16],
                                           double (&pre)[2][16], double (&prei)[2][4]) {
  constexpr int J = sk_tile_j(Q), C = sk_tile_c(Q);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, l15 = lane & 15;
  double* L = s.buf + (Q & 1) * (PB * SK_LD);
  // hand the prefetched tile over (the buffer was last read two tiles ago: one barrier in between)
#pragma unroll
  for (int r = 0; r < 16; ++r) L[(w + 4 * r) * SK_LD + lane] = pre[Q & 1][r];
  if constexpr (C == J) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = tid + 256 * r;
      s.li[(i >> 8) * (16 * SK_TD) + ((i >> 4) & 15) * SK_TD + (i & 15)] = prei[Q & 1][r];
    }
  }
  if constexpr (Q + 2 < SK_TILES) strip_fetch<Q + 2>(s, pre[Q & 1], prei[Q & 1]);
  __syncthreads();
  if constexpr (C == J) {
    // ---- row solve of block J: X_b = (T_b - sum_{b'<b} X_b' L[b][b']^T) Linv_bb^T, b = 0..3 ----
    double* Xw = s.Xw; double* Tt = s.Tt;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      double4_t a1 = acc[4 * J + b], a2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int bp = 0; bp < b; ++bp)
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          const double av = Xw[l15 * SK_LD + 16 * bp + 4 * st + kq];
          const double bv = -L[(16 * b + l15) * SK_LD + 16 * bp + 4 * st + kq];
          if (st & 1) a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, a2, 0, 0, 0);
          else a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, a1, 0, 0, 0);
        }
#pragma unroll
      for (int r = 0; r < 4; ++r) Tt[(kq + 4 * r) * SK_TD + l15] = a1[r] + a2[r];
      COMPILER_BARRIER();                            // same wave: LDS executes its operations in order
      double4_t x = {0.0, 0.0, 0.0, 0.0}, x2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const double av = Tt[l15 * SK_TD + 4 * st + kq];
        const double bv = s.li[b * (16 * SK_TD) + l15 * SK_TD + 4 * st + kq];
        if (st & 1) x2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, x2, 0, 0, 0);
        else x = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, x, 0, 0, 0);
      }
      COMPILER_BARRIER();
#pragma unroll
      for (int r = 0; r < 4; ++r) Xw[(kq + 4 * r) * SK_LD + 16 * b + l15] = x[r] + x2[r];
      COMPILER_BARRIER();
    }
    // ---- the solved block is final: out to HBM, a full 512-byte row segment per store ----
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < s.rows_left) s.Pw[(long)i * s.lda + J * PB + lane] = Xw[i * SK_LD + lane];
    if constexpr (J < 7) {
#pragma unroll
      for (int st = 0; st < 16; ++st) xa[st] = -Xw[l15 * SK_LD + 4 * st + kq];   // -X_j: A operand of the later blocks
    }
  } else {
    // one wave per SIMD: nothing else hides the LDS latency, so the B operands are read a few MFMAs
    // ahead of their use (software pipeline pinned with scheduling groups; reading further ahead
    // only adds spills: 152 spilled VGPRs at sixteen ahead, 61 at four, same time)
    constexpr int AHEAD = 4;
    double bq[64];
#pragma unroll
    for (int i = 0; i < AHEAD; ++i) bq[i] = L[(16 * (i & 3) + l15) * SK_LD + 4 * (i >> 2) + kq];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      if (i + AHEAD < 64) bq[i + AHEAD] = L[(16 * ((i + AHEAD) & 3) + l15) * SK_LD + 4 * ((i + AHEAD) >> 2) + kq];
      acc[4 * C + (i & 3)] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[i >> 2], bq[i], acc[4 * C + (i & 3)], 0, 0, 0);
      if (i + AHEAD < 64) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // one DS read ...
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          // ... one MFMA
    }
  }
  if constexpr (Q + 1 < SK_TILES) strip_tile<Q + 1>(s, acc, xa, pre, prei);
}

__global__ __launch_bounds__(256, 1) void panel_strip_kernel(const double* __restrict__ Dblk, long lda,
                                                             const double* __restrict__ Lfac,
                                                             const double* __restrict__ Linv16,
                                                             double* __restrict__ P, int rows, long strideD,
                                                             long strideL, long strideI) {
  extern __shared__ __attribute__((aligned(16))) double ssm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int kq = lane >> 4, l15 = lane & 15;
  StripCtx s;
  s.Dblk = Dblk + (long)blockIdx.y * strideD; s.lda = lda;
  s.Lfac = Lfac + (long)blockIdx.y * strideL;
  s.Linv16 = Linv16 + (long)blockIdx.y * strideI;
  const long r0 = (long)blockIdx.x * PB + 16 * w;    // this wave's first row
  s.Pw = P + (long)blockIdx.y * strideD + r0 * lda;
  s.rows_left = (long)rows - r0;
  s.buf = ssm;                                                       // 2 x [64][SK_LD] tiles of L
  s.Xw = ssm + 2 * PB * SK_LD + w * (16 * SK_LD);                    // per wave: [16][SK_LD] the solved block X_j
  s.Tt = ssm + 2 * PB * SK_LD + 4 * 16 * SK_LD + w * (16 * SK_TD);   // per wave: [16][SK_TD]
  s.li = ssm + 2 * PB * SK_LD + 4 * 16 * SK_LD + 4 * 16 * SK_TD;     // [4][16][SK_TD] inverses
  double pre[2][16], prei[2][4], xa[16];
  strip_fetch<0>(s, pre[0], prei[0]);
  strip_fetch<1>(s, pre[1], prei[1]);
  double4_t acc[32];
#pragma unroll
  for (int t = 0; t < 32; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      acc[t][r] = (kq + 4 * r < s.rows_left) ? s.Pw[(long)(kq + 4 * r) * lda + 16 * t + l15] : 0.0;
  strip_tile<0>(s, acc, xa, pre, prei);
}

// ---------------------------------------------------------------------------------------------
// One launch per panel (single matrices).  Workgroup g < 8 owns the 64-row strip g of the 512 x 512
// diagonal block, workgroup g >= 8 a strip of the rows below it; every strip lives in the MFMA
// accumulators as in panel_strip_kernel.  The eight diagonal strips form the dependent chain,
//   strip s:  for j < s: wait for L_jj, X_sj = (A_sj - ...) L_jj^-T, update the blocks (j, s];
//             then factor its own 64 x 64 diagonal block (factor64_waves) and publish L_ss,
// handing data on through HBM with two sets of per-matrix counters: flag[s] = epoch once L_ss and
// the inverses of its 16 x 16 blocks are out, prog[s] = j + 1 once X_sj is.  What is handed over goes
// out with write-through stores and comes in with agent-coherent loads (sc1); the counters are relaxed
// atomics: no cache-wide maintenance on the chain.  Workgroups only ever wait for workgroups with a
// smaller index of the same launch, which the dispatcher starts first.  This replaces the sixteen
// dependent launches of a panel (eight pivot steps, eight K = 64 updates) whose gaps and HBM round
// trips were the factorisation's chain.
constexpr int FUSED_SYNC_INTS = 24;
struct FusedArgs {
  double* D; long lda;
  double* Lfac; double* Linv16;
  int* sync;                 // per matrix: flag[8], prog[8], flag2[8] (the inverse of L_ss's last 16 x 16 block, published late)
  int epoch;
  int nbk;                   // order of the diagonal block (512, or less for the last panel: identity padding)
  int rows_below;            // rows under the diagonal block (only below a full one)
  long long* info; long pivot_base;
  long strideD, strideL, strideI;
  unsigned long long* status;   // hand-off status word (SYNC_ST_*)
  int spin_limit;               // polls before a wait gives up (and reports)
  // resident look-ahead schedule (cholesky_device): the launch announces every workgroup that has
  // started in *resident, and -- wait_ptr != null -- only then waits for *wait_ptr >= wait_target
  // (the trailing update of another stream has written the diagonal block) before touching the matrix
  int* resident; const int* wait_ptr; int wait_target;
  int prog_sleep;               // s_sleep argument of the polls that are not on the chain (waits for another strip's X_cJ)
#ifdef DFH_DEBUG_HOOKS
  long long* stamps = nullptr;  // dfh_debug_panel_stamps: [strip][64] s_memrealtime (100 MHz) at the points marked FSTAMP
#endif
};
#ifdef DFH_DEBUG_HOOKS
#define FSTAMP(a, g, i) do { if ((a).stamps && threadIdx.x == 0) (a).stamps[(g) * 64 + (i)] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FSTAMP(a, g, i) do {} while (0)
#endif

// Bounded: a workgroup only ever waits for workgroups of the same launch with a smaller index (started
// before it by the dispatcher as observed, not by contract) or for another launch that needs none of
// its resources; should a wait expire all the same, the status word says so, the strip goes on with
// whatever it finds (nobody hangs) and the host repeats the factorisation without hand-offs.
__device__ __forceinline__ void fused_wait(const int* p, int target, const FusedArgs& a, unsigned what = SYNC_ST_FUSED) {
  if (threadIdx.x == 0) {
    int spins = 0;
    while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (++spins > a.spin_limit) { atomicOr(a.status, (unsigned long long)what); break; }
      // somebody else has already given up: this factorisation is going to be repeated anyway
      if ((spins & 63) == 0 && __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
      __builtin_amdgcn_s_sleep(2);
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // later loads see what the writer released
}

// the sc1 protocol of the one-launch panel: data with write-through stores / agent-coherent loads ...
__device__ __forceinline__ void st_out(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_in(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// ... the flag goes up once every wave's write-through stores have been acknowledged (s_barrier alone does not
// wait for outstanding stores on gfx950: each wave drains its own first), and is read without a fence
__device__ __forceinline__ void fused_publish_sc1(int* p, int value) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(p, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (relaxed: true for the waits off the chain -- every poll is a round trip to the memory side of the fabric, and
//  sixty strips polling one line at full rate slow the loads and stores of the strip that IS on the chain)
__device__ __forceinline__ void fused_wait_sc1(const int* p, int target, const FusedArgs& a, bool relaxed = false,
                                               unsigned what = SYNC_ST_FUSED) {
  if (threadIdx.x == 0) {
    int spins = 0;
    while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (++spins > a.spin_limit) { atomicOr(a.status, (unsigned long long)what); break; }
      if ((spins & 63) == 0 && __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
      if (relaxed) {
        for (int z = 0; z < a.prog_sleep; ++z) __builtin_amdgcn_s_sleep(1);
      } else {
        __builtin_amdgcn_s_sleep(1);
      }
    }
  }
  __syncthreads();
}

// One column step J of a strip (round 4), the strip held TRANSPOSED in the accumulators,
//     accT[t][r] of lane (kq, l15) = strip element (row l15 of the wave's 16, column 16 t + kq + 4 r),
// i.e. the D layout of v_mfma_f64_16x16x4 for the transposed tile: D[kq + 4 r][l15] = T[l15][kq + 4 r].  In
// that layout an accumulator tile IS the B operand of a product that contracts over the strip's columns
// (B[k][n], k = kq + 4 r for the r-th of four MFMAs, n = l15), so
//     X_b^T = Linv_bb T_b^T,     T_b'^T -= L_b'b X_b^T  (b' > b, right-looking),     A_c^T -= L_cJ X^T
// take their A operands (rows of L / Linv, one ds_read_b64 per lane) from LDS and their B operands straight
// from registers: the row solve no longer changes layout through LDS between its four 16-column stages.
// Measured on the round-3 row-per-accumulator form (tools/dbg_panel.py, 100 MHz stamps): 4.25 us of a 22.5 us hop
// were this solve -- 40 MFMAs at ~200 cycles each, eight LDS write -> read round trips.
// acc^T[4 C + i] -= L_i X^T over the k-steps [KS0, KS1) of a 64-column block (k-step ks: columns 4 ks + kq of
// X = -xn), i = 0 .. 3: the order of panel_strip_kernel's update (k-step outer, the four tiles inner, ONE
// accumulator chain per tile), with the A operands read AHEAD MFMAs early: one wave per SIMD, nothing else
// hides the LDS latency.
// (C: the block; a compile-time constant at every call site after unrolling -- the accumulator index must be static)
template <int KS0, int KS1>
__device__ __forceinline__ void strip_update_t(double4_t (&acc)[32], const int C, const double* L, const double4_t (&xn)[4], int l15, int kq) {
  constexpr int N = (KS1 - KS0) * 4, AHEAD = 6;
  double aq[N];
#pragma unroll
  for (int q = 0; q < AHEAD && q < N; ++q) aq[q] = L[(16 * (q & 3) + l15) * SK_LD + 4 * (KS0 + (q >> 2)) + kq];
#pragma unroll
  for (int q = 0; q < N; ++q) {
    if (q + AHEAD < N) aq[q + AHEAD] = L[(16 * ((q + AHEAD) & 3) + l15) * SK_LD + 4 * (KS0 + ((q + AHEAD) >> 2)) + kq];
    const int ks = KS0 + (q >> 2);
    acc[4 * C + (q & 3)] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq[q], xn[ks >> 2][ks & 3], acc[4 * C + (q & 3)], 0, 0, 0);
#ifndef DFH_NO_SGB
    if (q + AHEAD < N) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // one DS read ...
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // ... one MFMA
#endif
  }
}

template <int J>
__device__ __forceinline__ void fused_step_t(const FusedArgs& a, double4_t (&acc)[32], int s, bool diag, double* Rw,
                                             long rows_left, double* ssm) {
  const int tid = threadIdx.x, lane = tid & 63;
  // wave-uniform, and known to be: the row-store addresses built on it stay scalar.  (With a vector w the strip's
  // row pointer was spilled and every one of the sixteen X row stores waited -- vmcnt(0) -- for its reload behind
  // the previous write-through store: 5 us per step.)
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, l15 = lane & 15;
  double* Lj = ssm;                                                // [64][SK_LD]
  double* Lc = ssm + PB * SK_LD;                                   // [64][SK_LD]
  double* Xall = ssm + 2 * PB * SK_LD;                             // [64][SK_LD]: the four waves' solved rows
  double* Xw = Xall + w * (16 * SK_LD);
  // (the [4][16][SK_TD] before li is unused: the round-3 step's transpose buffer, still reserved in FUSED_SMEM)
  double* li = ssm + 2 * PB * SK_LD + 4 * 16 * SK_LD + 4 * 16 * SK_TD;
  int* flag = a.sync; int* prog = a.sync + 8;
  if (J < s) {
    fused_wait_sc1(flag + J, a.epoch, a, !(diag && J == s - 1));
    FSTAMP(a, blockIdx.x, 1 + 4 * J);
    {
      double pre[16], prei[4];                         // all loads in flight before the first LDS write
#pragma unroll
      for (int r = 0; r < 16; ++r) pre[r] = ld_in(a.Lfac + J * PB * PB + (w + 4 * r) * PB + lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = tid + 256 * r;
        prei[r] = ld_in(a.Linv16 + J * (4 * 16 * 17) + (i >> 8) * (16 * 17) + ((i >> 4) & 15) * 17 + (i & 15));
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) Lj[(w + 4 * r) * SK_LD + lane] = pre[r];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = tid + 256 * r;
        li[(i >> 8) * (16 * SK_TD) + ((i >> 4) & 15) * SK_TD + (i & 15)] = prei[r];
      }
    }
    __syncthreads();
    FSTAMP(a, blockIdx.x, 2 + 4 * J);
    // ---- row solve of block J, 16-column stages, right-looking; xn[b] = -X_b^T ----
    // (the accumulator tiles of block J are only ever read from here on: the solved block lives in xn and in LDS, so
    //  that no accumulator tile is written by the vector unit -- they stay in the AGPR half of the register file)
    double4_t xn[4], odd[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) odd[b] = (double4_t){0.0, 0.0, 0.0, 0.0};
    // the strip's LAST step (the one on the chain): X_s,s-1 is announced late, and three quarters of the
    // own-block product A_ss -= X X^T run BEFORE the fourth solve stage, while the inverse that stage needs is
    // still on its way (second flag of strip J)
    const bool last_step = diag && J == s - 1;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (b == 3 && last_step) {
        FSTAMP(a, blockIdx.x, 48);
        __syncthreads();                               // columns 0 .. 47 of all four waves' X_sJ are in Xall
        FSTAMP(a, blockIdx.x, 49);
        if constexpr (J + 1 < 8) strip_update_t<0, 12>(acc, J + 1, Xall, xn, l15, kq);
      }
      if (b == 3 && last_step) FSTAMP(a, blockIdx.x, 50);
      // T_b^T = the tile (which carries the even-numbered k-steps of the earlier stages' updates) + the odd chain:
      // the association of panel_strip_kernel / diag_step64_kernel (two accumulators per product,
      // added at the end), so that every schedule of the factorisation rounds alike -- results do not depend on
      // how a candidate set is cut into shards, chunks and lock-step groups (tests/test_gpu_mgpu.py).
      // It leaves the accumulator file for the vector registers here: the tile is dead from now on, so the
      // product below does not need a 33rd tile of accumulators (which the compiler found by spilling one)
      const double4_t tsum = (b == 0) ? acc[4 * J + b] : acc[4 * J + b] + odd[b];
      double tb0 = tsum[0], tb1 = tsum[1], tb2 = tsum[2], tb3 = tsum[3];
      asm volatile("" : "+v"(tb0), "+v"(tb1), "+v"(tb2), "+v"(tb3));
      double i0, i1, i2, i3;                                       // Linv_bb[l15][k], k = kq + 4 r
      if (b < 3) {
        const double* lib = li + b * (16 * SK_TD) + l15 * SK_TD + kq;
        i0 = lib[0]; i1 = lib[4]; i2 = lib[8]; i3 = lib[12];
      } else {
        // the last block's inverse arrives under its own flag (see the end of panel_fused_kernel), straight
        // into registers: every wave polls for itself, no workgroup barrier on the way
        if (lane == 0) {
          int spins = 0;
          while (__hip_atomic_load(a.sync + 16 + J, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < a.epoch) {
            if (++spins > a.spin_limit) { atomicOr(a.status, (unsigned long long)SYNC_ST_FUSED); break; }
            if ((spins & 63) == 0 && __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
            __builtin_amdgcn_s_sleep(1);
          }
        }
        // (the inverse's loads below are coherent loads issued after the poll in program order; the compiler must
        //  not move them above it either)
        asm volatile("" ::: "memory");
        if (last_step) FSTAMP(a, blockIdx.x, 51);
        const double* gi = a.Linv16 + J * (4 * 16 * 17) + 3 * (16 * 17) + l15 * 17 + kq;
        i0 = ld_in(gi); i1 = ld_in(gi + 4); i2 = ld_in(gi + 8); i3 = ld_in(gi + 12);
      }
      double4_t p = {0.0, 0.0, 0.0, 0.0}, p2 = {0.0, 0.0, 0.0, 0.0};
      p = __builtin_amdgcn_mfma_f64_16x16x4f64(i0, tb0, p, 0, 0, 0);
      p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(i1, tb1, p2, 0, 0, 0);
      p = __builtin_amdgcn_mfma_f64_16x16x4f64(i2, tb2, p, 0, 0, 0);
      p2 = __builtin_amdgcn_mfma_f64_16x16x4f64(i3, tb3, p2, 0, 0, 0);
      p = p + p2;                                                  // X_b^T
      xn[b] = -p;
      // the solved block's row-major image in LDS (coalesced store below; A operand of the own-block product)
#pragma unroll
      for (int r = 0; r < 4; ++r) Xw[l15 * SK_LD + 16 * b + kq + 4 * r] = p[r];
#pragma unroll
      for (int b2 = b + 1; b2 < 4; ++b2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double lv = Lj[(16 * b2 + l15) * SK_LD + 16 * b + kq + 4 * r];                 // L[16 b2 + l15][16 b + k]
          if (r & 1) odd[b2] = __builtin_amdgcn_mfma_f64_16x16x4f64(lv, xn[b][r], odd[b2], 0, 0, 0);
          else acc[4 * J + b2] = __builtin_amdgcn_mfma_f64_16x16x4f64(lv, xn[b][r], acc[4 * J + b2], 0, 0, 0);
        }
    }
    COMPILER_BARRIER();                              // same wave: LDS executes its operations in order
    if (rows_left >= 16) {                             // (wave-uniform)
#pragma unroll
      for (int i = 0; i < 16; ++i) st_out(Rw + (long)i * a.lda + J * PB + lane, Xw[i * SK_LD + lane]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < rows_left) st_out(Rw + (long)i * a.lda + J * PB + lane, Xw[i * SK_LD + lane]);
    }
    // X_sJ is out (later diagonal strips and the rows below read it).  In the strip's LAST step -- the one on the
    // chain -- the announcement waits until the own-block product below has been issued: nobody needs X_s,s-1
    // before L_ss exists, and the wait for the stores' acknowledgement (1.5 us) leaves the chain.
    if (diag && !last_step) fused_publish_sc1(prog + s, a.epoch * 16 + J + 1);
    FSTAMP(a, blockIdx.x, 3 + 4 * J);
    const int c_hi = diag ? s : 7;                     // last block this strip still needs
#pragma unroll
    for (int c = J + 1; c < 8; ++c) {
      if (c > c_hi) break;
      const double* L;
      const bool own = diag && c == s;
      if (own) {
        if (last_step) FSTAMP(a, blockIdx.x, 52);
        __syncthreads();                               // all four waves' rows of X_sJ are in Xall
        if (last_step) FSTAMP(a, blockIdx.x, 53);
        L = Xall;                                      // own diagonal block: A_ss -= X_sJ X_sJ^T (lower tiles only)
      } else {
        // strip c has published X_cJ (its barrier also frees Lc)
        fused_wait_sc1(prog + c, a.epoch * 16 + J + 1, a, true);
        double pre[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) pre[r] = ld_in(a.D + (long)(c * PB + w + 4 * r) * a.lda + J * PB + lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) Lc[(w + 4 * r) * SK_LD + lane] = pre[r];
        __syncthreads();
        L = Lc;
      }
      // (the own block's tiles right of the diagonal are computed too -- garbage nobody reads, as in the other
      //  schedules; the waves that would skip them wait for wave 3 at the next barrier anyway)
      if (own && last_step) strip_update_t<12, 16>(acc, c, L, xn, l15, kq);      // k-steps 0 .. 11: before the fourth solve stage (above)
      else strip_update_t<0, 16>(acc, c, L, xn, l15, kq);
    }
    // (the last step's X_s,s-1 is announced from the kernel's tail, behind the staging barrier: by then the
    //  stores' acknowledgement, 1.5 - 2 us for write-through, has arrived without anybody waiting for it)
    if (last_step) FSTAMP(a, blockIdx.x, 54);
    __syncthreads();                                   // Xall / Lj / li are free for the next step
    FSTAMP(a, blockIdx.x, 4 + 4 * J);
  }
}

__global__ __launch_bounds__(256, 1) void panel_fused_kernel(FusedArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ssm[];
  a.D += (long)blockIdx.y * a.strideD;
  a.Lfac += (long)blockIdx.y * a.strideL;
  a.Linv16 += (long)blockIdx.y * a.strideI;
  a.sync += (long)blockIdx.y * FUSED_SYNC_INTS;
  a.info += blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  // (NOT through readfirstlane here, unlike in fused_step_t.  With a scalar w the diagnostics build of this kernel
  //  came out with columns 0..3 of strip 0's block right and NaN from column 4 on.  Root cause, read off the ISA
  //  (docs/NOTES_r05.md section 2): a register-allocation fault of the compiler under this kernel's pressure (512 of
  //  512 registers, 288 spilled dwords).  The spill of acc[0] was split into scratch_store_dwordx3 (dwords 0-2), an
  //  AGPR copy a191 of dword 3 and four AGPR copies of dwords 4-7; the reload in the strip-0 leaf of the block select
  //  below restores seven of the eight -- a191 is written once and read nowhere -- so the high half of acc[0][1],
  //  i.e. columns 4..7 of the staged block, is whatever a195 last held.  Nothing in the source or the hardware; it
  //  comes and goes with the allocation, so tools/isa_audit.py looks for its signature (a register written and never
  //  read) in every function of the built library and tests/test_isa_audit.py runs that on each build.)
  const int w = tid >> 6;
  const int kq = lane >> 4, l15 = lane & 15;
  const int g = blockIdx.x;
  const int nd = (a.nbk + PB - 1) / PB;              // diagonal strips (8 for a full panel)
  if (a.resident) {
    if (tid == 0) __hip_atomic_fetch_add(a.resident, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.wait_ptr) fused_wait(a.wait_ptr, a.wait_target, a, SYNC_ST_GATE);
  }
  const bool diag = g < nd;
  const int s = diag ? g : nd;
  double* Rw = a.D + ((long)g * PB + 16 * w) * a.lda;               // this wave's 16 rows of the panel
  const long rows_left = (long)(a.nbk + a.rows_below) - ((long)g * PB + 16 * w);
  double4_t acc[32];
  const bool full = a.nbk == 8 * PB && rows_left >= 16;      // (wave-uniform)
  if (full) {
    // full panel, all sixteen rows present: one base address per lane and immediate offsets; the blocks a
    // diagonal strip never touches are not loaded, its own block is cut to the lower triangle
    const double* rp = Rw + (long)l15 * a.lda + kq;
    const int row = 16 * w + l15;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bool need = !diag || c <= s;
      const bool own = diag && c == s;
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        double4_t v = {0.0, 0.0, 0.0, 0.0};
        if (need) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = rp[16 * (4 * c + ti) + 4 * r];
          if (own) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (16 * ti + kq + 4 * r <= row) ? v[r] : 0.0;
          }
        }
        acc[4 * c + ti] = v;
      }
    }
  } else
#pragma unroll
  for (int t = 0; t < 32; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // lane (kq, l15) holds row l15, columns 16 t + kq + 4 r
      const int rl = l15;                                // row within the wave's 16
      const int cl = kq + 4 * r;                         // column within the 16-column tile
      const int row = 16 * w + rl, c = t >> 2, col = 16 * (t & 3) + cl;
      // a diagonal strip needs its blocks up to its own, of that one only the lower triangle; rows and
      // columns beyond the block's order (last panel) are identity padding
      const bool want = (rl < rows_left) && (16 * t + cl < a.nbk) && (!diag || c < s || (c == s && col <= row));
      const bool pad_one = diag && c == s && col == row && (rl >= rows_left);
      acc[t][r] = want ? Rw[(long)rl * a.lda + 16 * t + cl] : (pad_one ? 1.0 : 0.0);
    }
  FSTAMP(a, g, 0);
  fused_step_t<0>(a, acc, s, diag, Rw, rows_left, ssm);
  fused_step_t<1>(a, acc, s, diag, Rw, rows_left, ssm);
  fused_step_t<2>(a, acc, s, diag, Rw, rows_left, ssm);
  fused_step_t<3>(a, acc, s, diag, Rw, rows_left, ssm);
  fused_step_t<4>(a, acc, s, diag, Rw, rows_left, ssm);
  fused_step_t<5>(a, acc, s, diag, Rw, rows_left, ssm);
  fused_step_t<6>(a, acc, s, diag, Rw, rows_left, ssm);
  fused_step_t<7>(a, acc, s, diag, Rw, rows_left, ssm);
  if (!diag) return;
  // ---- factor the strip's own diagonal block and publish it (LDS of the strip machinery is free) ----
  double* Sp = ssm;                                  // [64][SPP] staged block, then the factor image
  double* colbuf = ssm + PB * SPP;                   // [64]
  double* ring = colbuf + PB;                        // [64][64]
  double* tbuf0 = ring + PB * PB;                    // 3 x [64][17]
  double* lbb = tbuf0 + 3 * PB * 17;                 // 4 x [16][17]
  double* linv = lbb + 4 * 16 * 17;                  // 4 x [16][17]
  double* rdiag = colbuf;
  __shared__ int s_badv[4];
  __shared__ int s_ring_timeout;
  if (tid == 0) s_ring_timeout = 0;
  // the 64 x 64 block s of the accumulators -> staged block (lower triangle, zero above)
#pragma unroll
  for (int t4 = 0; t4 < 4; ++t4) {
    double4_t v;
    // accumulator index has to be static: select the block by a chain of uniform branches
    switch (s) {
      case 0: v = acc[0 + t4]; break; case 1: v = acc[4 + t4]; break; case 2: v = acc[8 + t4]; break;
      case 3: v = acc[12 + t4]; break; case 4: v = acc[16 + t4]; break; case 5: v = acc[20 + t4]; break;
      case 6: v = acc[24 + t4]; break; default: v = acc[28 + t4]; break;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * w + l15, col = 16 * t4 + kq + 4 * r;
      Sp[row * SPP + col] = (col <= row) ? v[r] : 0.0;
    }
  }
  if (tid < PB) ring[tid * PB] = 0.0;
  if (s > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows of X_s,s-1 are out
  __syncthreads();
  if (s > 0 && tid == 0)                         // ... all four waves': announce them (see fused_step_t)
    __hip_atomic_store(a.sync + 8 + s, a.epoch * 16 + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  FSTAMP(a, g, 40);
  double av[16];
  double* tbuf = tbuf0 + (w > 0 ? (w - 1) : 0) * PB * 17;
  // The inverse of the last 16 x 16 block -- the only one of the four that is not hidden behind later columns,
  // ~4.3k cycles at the end of the chain -- is computed AFTER the factor has been handed on, and published under a
  // second flag: the next strip needs it for the last of its four solve stages only, ~3 us after it saw the first
  double my_r3 = 1.0;
  const int bad = factor64_waves<true>(av, lane, w, Sp, tbuf, ring, lbb, linv, rdiag, &s_ring_timeout, nullptr, &my_r3);
  if (lane == 0) s_badv[w] = bad;
#pragma unroll
  for (int j = 0; j < 16; ++j) Sp[lane * SPP + perm16(16 * w + j)] = av[j];
  FSTAMP(a, g, 41);        // (thread 0 = wave 0: done with its columns long before wave 3)
  __syncthreads();
  FSTAMP(a, g, 42);
  const int s_bad = (s_badv[0] >= 0) ? s_badv[0] : (s_badv[1] >= 0) ? s_badv[1] : (s_badv[2] >= 0) ? s_badv[2] : s_badv[3];
  if (s_ring_timeout && tid == 0) atomicOr(a.status, (unsigned long long)SYNC_ST_RING);
  if (s_bad >= 0 && tid == 0) {
    // first failing pivot of the matrix: strips run in order, so the first writer wins
    unsigned long long expect = 0ull;
    __hip_atomic_compare_exchange_strong((unsigned long long*)a.info, &expect,
                                         (unsigned long long)(a.pivot_base + (long)s * PB + s_bad + 1), __ATOMIC_RELAXED,
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  {
    double* Lout = a.Lfac + (long)s * PB * PB;
    const int pk = perm16(lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) st_out(Lout + (w + 4 * r) * PB + lane, Sp[(w + 4 * r) * SPP + pk]);
    double* Iout = a.Linv16 + (long)s * (4 * 16 * 17);
    for (int i = tid; i < 3 * 16 * 17; i += 256) st_out(Iout + i, linv[i]);
  }
  // published even after a failed pivot: nobody may hang
  fused_publish_sc1(a.sync + s, a.epoch);
  FSTAMP(a, g, 43);
  if (w == 3) {
    factor64_inverse16(av, lane, 3, lbb, linv, rdiag, my_r3);
    COMPILER_BARRIER();                              // same wave: LDS executes its operations in order
    double* Iout3 = a.Linv16 + (long)s * (4 * 16 * 17) + 3 * (16 * 17);
    for (int i = lane; i < 16 * 17; i += 64) st_out(Iout3 + i, linv[3 * (16 * 17) + i]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the whole wave's stores are acknowledged
    if (lane == 0) __hip_atomic_store(a.sync + 16 + s, a.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

constexpr int FUSED_SMEM_STRIP = (2 * PB * SK_LD + 4 * 16 * SK_LD + 4 * 16 * SK_TD + 4 * 16 * SK_TD) * 8;
constexpr int FUSED_SMEM_FACTOR = (PB * SPP + PB + PB * PB + 3 * PB * 17 + 8 * 16 * 17) * 8;
constexpr int FUSED_SMEM = FUSED_SMEM_STRIP > FUSED_SMEM_FACTOR ? FUSED_SMEM_STRIP : FUSED_SMEM_FACTOR;

// Stream gate: the launches behind it in its stream start only once *p >= target -- another stream's
// kernel has reached the point that raises the word.  One wave, polling politely; bounded like every
// wait of the factorisation (status word, then the host's fallback).
__global__ __launch_bounds__(64) void k_gate(const int* __restrict__ p, int target, unsigned long long* status, int spin_limit) {
  if (threadIdx.x == 0) {
    int spins = 0;
    while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (++spins > spin_limit) { atomicOr(status, (unsigned long long)SYNC_ST_GATE); break; }
      if ((spins & 63) == 0 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
      __builtin_amdgcn_s_sleep(8);
    }
  }
}

// p[b * stride + i] = 0 for i < count, b = blockIdx.y: one launch instead of one memset per batch matrix
__global__ void k_zero_strided(double* __restrict__ p, long count, long stride) {
  double* q = p + (long)blockIdx.y * stride;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x) q[i] = 0.0;
}

// Inverses of the 64 x 64 lower-triangular diagonal blocks of an nbk x nbk factor block (one
// workgroup per block).  Padded rows/cols are identity so the full 64-block is safe.
// Lscr != null: block b's factor is read from Lscr + b*64*64 (ld 64) and also copied into its
// place on the diagonal of D (upper part zero); Lscr == null: the factor is read from D.
// (two waves per SIMD in the bounds: at most 256 registers, so that a workgroup fits beside ONE resident
//  GEMM workgroup -- with 340 registers it had to wait for a CU to drain completely: 1 - 1.8 ms behind a
//  running trailing update, against 36 us alone)
__global__ __launch_bounds__(256, 2) void trtri64_kernel(double* __restrict__ D, long lda, int nbk,
                                                      double* __restrict__ inv, long ldinv,
                                                      const double* __restrict__ Lscr, long strideD,
                                                      long strideInv, long strideL, int zero_rest) {
  __shared__ double S[PB * PBP];
  __shared__ double Tt[32 * 33];
  __builtin_amdgcn_s_setprio(3);      // beside a GEMM wave on the same SIMD the chain's kernel goes first
  D += (long)blockIdx.y * strideD;
  if (inv) inv += (long)blockIdx.y * strideInv;
  if (Lscr) Lscr += (long)blockIdx.y * strideL;
  const int tid = threadIdx.x;
  const int k = tid & 63, w = tid >> 6;
  const int j0 = blockIdx.x * PB;
  const int nb = min(PB, nbk - j0);
  double* A = D + (long)j0 * lda + j0;
  if (zero_rest && inv) {
    // this block's 64 rows of the 512-wide inverse, except the diagonal block written below
    for (int idx = tid; idx < PB * (int)CHOL_NB; idx += 256) {
      const int i = idx / (int)CHOL_NB, c = idx - i * (int)CHOL_NB;
      if (c < j0 || c >= j0 + PB) inv[(long)(j0 + i) * ldinv + c] = 0.0;
    }
  }
  double a[16];
  if (Lscr) {
    const double* src = Lscr + (long)blockIdx.x * PB * PB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = w + 4 * r;
      a[r] = src[i * PB + k];
      if (i < nb && k < nb) A[i * lda + k] = a[r];
    }
    if (!inv) return;                 // commit of the factor only (no inverses wanted)
  } else {
    load_block64(A, lda, nb, w, k, a);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) S[(w + 4 * r) * PBP + k] = a[r];
  __syncthreads();
  // [[A, 0], [B, C]]^-1 = [[A^-1, 0], [-C^-1 B A^-1, C^-1]] with 32 x 32 blocks: the two triangular
  // inverses by back substitution on rows (x_r L = e_r) in the two halves of wave 0 -- 32 values per
  // lane instead of 64: the kernel stays far below 256 registers --, the off-diagonal block by two
  // 32^3 products of the whole workgroup; everything in place in S.
  if (tid < 64) {
    const int r = tid & 31, o = 32 * (tid >> 5);
    double x[32];
#pragma unroll
    for (int c = 31; c >= 0; --c) {
      double s = (r == c) ? 1.0 : 0.0;
#pragma unroll
      for (int kk = c + 1; kk < 32; ++kk) s = fma(-x[kk], S[(o + kk) * PBP + o + c], s);
      x[c] = s / S[(o + c) * PBP + o + c];
    }
    // (one wave, identical trip counts: every lane has read the factor entries before any is overwritten)
#pragma unroll
    for (int c = 0; c < 32; ++c) S[(o + r) * PBP + o + c] = (c <= r) ? x[c] : 0.0;
  }
  __syncthreads();
  {
    double t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                     // T = B A^-1  (A^-1 lower: k >= j)
      const int idx = tid + 256 * q, i = idx >> 5, j = idx & 31;
      double acc = 0.0;
      for (int kk = j; kk < 32; ++kk) acc = fma(S[(32 + i) * PBP + kk], S[kk * PBP + j], acc);
      t[q] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + 256 * q, i = idx >> 5, j = idx & 31;
      Tt[i * 33 + j] = t[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {                     // X = -C^-1 T  (C^-1 lower: k <= i)
      const int idx = tid + 256 * q, i = idx >> 5, j = idx & 31;
      double acc = 0.0;
      for (int kk = 0; kk <= i; ++kk) acc = fma(-S[(32 + i) * PBP + 32 + kk], Tt[kk * 33 + j], acc);
      S[(32 + i) * PBP + j] = acc;
    }
  }
  __syncthreads();
  double* out = inv + (long)j0 * ldinv + j0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = w + 4 * r;
    if (i < nb && k < nb) out[(long)i * ldinv + k] = (k <= i) ? S[i * PBP + k] : 0.0;
  }
}

// Merge the 64-block inverses on the diagonal of Linv (ld = CHOL_NB) into the inverse of the
// nbk x nbk lower-triangular block D (ld = lda) by recursive doubling:
//   [[A,0],[B,C]]^-1 = [[A^-1,0],[-C^-1 B A^-1, C^-1]]
int assemble_block_inverse(dfh_ctx* ctx, const double* D, int64_t lda, int64_t nbk, double* Linv,
                           double* T, int nbatch = 1, int64_t strideD = 0, int64_t strideInv = 0,
                           int64_t strideT = 0) {
  const int64_t NB = CHOL_NB;
  for (int64_t s = PB; s < nbk; s *= 2) {
    const int64_t full_pairs = nbk / (2 * s);
    if (full_pairs > 0) {
      GemmBatch b1, b2;
      b1.count = b2.count = (int)full_pairs;
      b1.count2 = b2.count2 = nbatch;
      b1.sA2 = strideD; b1.sB2 = strideInv; b1.sCout2 = strideT;
      b2.sA2 = strideInv; b2.sB2 = strideT; b2.sCout2 = strideInv;
      // T_q = B_q * A_q^-1 : B_q = D[hi rows, lo cols], A_q^-1 = Linv[lo, lo]
      b1.sA = 2 * s * (lda + 1); b1.sB = 2 * s * (NB + 1); b1.sCout = s * s;
      DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, s, s, s, 1.0, D + s * lda, lda, Linv, NB, 0.0, nullptr, 0,
                       T, s, &b1));
      // X_q = -C_q^-1 * T_q -> Linv[hi rows, lo cols]
      b2.sA = 2 * s * (NB + 1); b2.sB = s * s; b2.sCout = 2 * s * (NB + 1);
      DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, s, s, s, -1.0, Linv + s * (NB + 1), NB, T, s, 0.0, nullptr,
                       0, Linv + s * NB, NB, &b2));
    }
    const int64_t lo = full_pairs * 2 * s, hi = lo + s;
    if (hi < nbk) {                                   // trailing partial pair
      const int64_t hs = nbk - hi;
      GemmBatch c1, c2;
      c1.count = c2.count = nbatch;
      c1.sA = strideD; c1.sB = strideInv; c1.sCout = strideT;
      c2.sA = strideInv; c2.sB = strideT; c2.sCout = strideInv;
      DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, hs, s, s, 1.0, D + hi * lda + lo, lda, Linv + lo * (NB + 1),
                       NB, 0.0, nullptr, 0, T, s, &c1));
      DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, hs, s, hs, -1.0, Linv + hi * (NB + 1), NB, T, s, 0.0,
                       nullptr, 0, Linv + hi * NB + lo, NB, &c2));
    }
  }

  return DFH_OK;
}


// ---------------------------------------------------------------------------------------------
// Quality of an explicit block inverse, and what the solves do about it.
// Multiplying by the explicit inverse M of a 512 x 512 diagonal block L_bb leaves a residual of
// order eps * cond(L_bb) instead of the order eps of a substitution.  For the matrices a GP with
// noise >= Var(Y)/20 produces that is invisible; the reference's tuners also pick noise variances
// of 1e-8 Var(Y), where cond(L_bb) reaches 1e5 and more (tests/test_gpu_conditioning.py).  Per
// block the factorisation therefore keeps, next to M, a clean copy of L_bb (lower triangle, zero
// elsewhere, row stride NB) and measures delta = max |I - M L_bb|.  A solve with block b then runs
// refine_steps(delta) steps of iterative refinement in working precision, x <- x + M (r - L_bb x):
// each step multiplies the residual by delta, and it bottoms out at the residual of a backward
// stable solve (the rounding of r - L_bb x itself) -- the same GEMM / GEMV kernels, no
// substitution chain.  Well-conditioned blocks (delta <= tol) take no step and cost nothing.
// ---------------------------------------------------------------------------------------------
__global__ void k_copy_lower_block(const double* __restrict__ D, long lda, int nbk, double* __restrict__ out,
                                   long strideD, long strideOut) {
  __builtin_amdgcn_s_setprio(3);
  D += (long)blockIdx.z * strideD;
  out += (long)blockIdx.z * strideOut;
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= (int)CHOL_NB) return;
  out[(long)i * CHOL_NB + j] = (i < nbk && j <= i) ? D[(long)i * lda + j] : 0.0;
}

// delta[blockIdx.x * strideDelta] = max_ij |E_ij - [i == j]| over the nbk x nbk block E (ld NB); +inf if any
// NaN.  blockIdx.y = slice of the elements; the slices combine through an atomic max on the bit
// pattern (non-negative doubles order like their bit patterns; the slot is zeroed beforehand).
constexpr int DELTA_SLICES = 32;
__global__ __launch_bounds__(256) void k_inv_delta(const double* __restrict__ E, int nbk, long strideE,
                                                    double* __restrict__ delta, long strideDelta) {
  __shared__ double sm[256];
  __builtin_amdgcn_s_setprio(3);
  E += (long)blockIdx.x * strideE;
  double m = 0.0;
  bool bad = false;
  const long total = (long)nbk * nbk;
  for (long idx = (long)blockIdx.y * 256 + threadIdx.x; idx < total; idx += (long)DELTA_SLICES * 256) {
    const int i = (int)(idx / nbk), j = (int)(idx % nbk);
    const double v = fabs(E[(long)i * CHOL_NB + j] - (i == j ? 1.0 : 0.0));
    if (v != v) bad = true;
    m = v > m ? v : m;
  }
  sm[threadIdx.x] = bad ? INFINITY : m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0)
    atomicMax(reinterpret_cast<unsigned long long*>(delta + (long)blockIdx.x * strideDelta),
              (unsigned long long)__double_as_longlong(sm[0]));
}

// clean copy of the diagonal block + delta, asynchronous on ctx->stream (T: NB*NB doubles per matrix)
int block_inverse_quality(dfh_ctx* ctx, const double* D, int64_t lda, int64_t nbk, const double* Linv, double* Ldiag,
                          double* T, double* d_delta, int nbatch = 1, int64_t strideD = 0, int64_t strideInv = 0,
                          int64_t strideT = 0, int64_t strideDelta = 0) {
  const int64_t NB = CHOL_NB;
  hipLaunchKernelGGL(k_copy_lower_block, dim3((unsigned)(NB / 256), (unsigned)NB, (unsigned)nbatch), dim3(256), 0,
                     ctx->stream, D, (long)lda, (int)nbk, Ldiag, (long)strideD, (long)strideInv);
  DFH_LAUNCH_CHECK();
  GemmBatch b;
  b.count = nbatch; b.sA = strideInv; b.sB = strideInv; b.sCout = strideT;
  DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, nbk, nbk, nbk, 1.0, Linv, NB, Ldiag, NB, 0.0, nullptr, 0, T, NB, &b));
  hipLaunchKernelGGL(k_zero_strided, dim3(1, (unsigned)nbatch), dim3(64), 0, ctx->stream, d_delta, 1L, (long)strideDelta);
  DFH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_inv_delta, dim3((unsigned)nbatch, DELTA_SLICES), dim3(256), 0, ctx->stream, T, (int)nbk,
                     (long)strideT, d_delta, (long)strideDelta);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

// The factorisation's run-time switches, read once per process at the first factorisation.
// chol_plan, below, turns them into one call's choices.
struct CholSwitches {
  // test hook: DFH_TEST_SPIN_LIMIT=0 makes every inter-workgroup wait expire at once (the fallback's test)
  int spin_limit = env_int("DFH_TEST_SPIN_LIMIT", SPIN_LIMIT_DEFAULT);
  int lr_on = env_int("DFH_CHOL_LR", 1);
  long lr_min_rem = env_int("DFH_CHOL_LR_MIN_REM", 7680);
  int fused_on = env_int("DFH_CHOL_FUSED", 1);
  int fused_max_batch = env_int("DFH_CHOL_FUSED_MAX_BATCH", -1);      // < 0: by size (chol_plan)
  int prog_sleep = env_int("DFH_CHOL_PROG_SLEEP", 8);
  int strips_on = env_int("DFH_CHOL_STRIPS", 1);
  int strips_max_wg = env_int("DFH_CHOL_STRIPS_MAX_WG", 1 << 30);
  int strips_min_wg = env_int("DFH_CHOL_STRIPS_MIN_WG", -1);          // < 0: by batch size (chol_plan)
  bool pair_on = env_flag("DFH_CHOL_PAIR", true);
  long pair_min_rem = env_long("DFH_CHOL_PAIR_MIN_REM", 6144L);
  double refine_tol = env_double("DFH_REFINE_TOL", 1e-13);
};
const CholSwitches& chol_switches() {
  static const CholSwitches sw;
  return sw;
}

int refine_steps(double delta) {
  const double tol = chol_switches().refine_tol;
  // test hook (tests/trsolve_forced_check.py, started by tests/test_gpu_trsolve.py): every block takes this many steps whatever its inverse is like
  static const int forced = env_int("DFH_REFINE_FORCE_STEPS", -1);
  if (forced >= 0) return forced > 8 ? 8 : forced;
  if (!(delta > tol)) return 0;
  if (!(delta < 0.25)) return 8;                    // the inverse is barely an inverse: as many steps as we allow
  const int k = (int)ceil(log(1e-15) / log(delta)) - 1;
  return k < 1 ? 1 : (k > 8 ? 8 : k);
}

}  // namespace

// Look-ahead schedule.  Two streams: P (high priority, "panel") and M (the context's main
// stream, "trailing").  For panel k
//   P: factor the 512 diagonal block, invert it, solve the panel L21(k), then update ONLY block
//      column k+1 with it (after M's trailing update k-1, which also wrote that column);
//   M: once L21(k) is ready, update the rest of the trailing matrix (columns >= k+2, lower).
// P therefore factors panel k+1 while M is still busy with the big SYRK of panel k: the
// latency-bound diagonal work leaves the critical path while the trailing update is long enough
// to cover it.
//
// Resident look-ahead (round 3; single matrices while at least DFH_CHOL_LR_MIN_REM rows are left).
// The schedule above does not overlap in practice: a panel kernel needs whole CUs (122 KB of LDS, all
// 512 registers of its lanes) and the trailing update refills every slot the moment it frees, so
// the panel of k+1 used to start when the update of k had drained.  Now
//   * the diagonal block of panel k+1 is factored by a launch of its own (panel_fused_kernel with no
//     rows below: eight workgroups) that is enqueued BEFORE the trailing update of panel k may start:
//     a one-wave gate kernel holds stream M until all eight have announced themselves (resident
//     counter).  They then wait -- bounded -- for the update's first sixteen tiles, the next
//     diagonal block, which the update computes first (look-ahead tile order, gemm_f64.hip) and
//     announces through a counter; 3 % of the CUs idle for ~0.1 ms per panel;
//   * the rows below the diagonal block are solved by GEMM with the explicit 512-block inverse the
//     posterior keeps anyway, L21 = A21 M^T, refined in working precision when the inverse's measured
//     quality asks for it (device-side condition: the refinement launches exit at once for a
//     well-conditioned block) -- GEMM workgroups share the CUs with the update's, which the panel
//     strips (one per CU) could not;
//   * the update of panel k is ONE launch over the whole trailing matrix (the look-ahead block
//     column is its first tiles instead of a launch of its own behind a stream barrier).
// The chain diag(k+1) -> inverse -> solve then runs beside update(k), and the updates follow each
// other on M as long as one lasts longer than the chain (~0.6 ms: n - k0 > ~8000).  Below that the
// schedule above takes over (it is the faster one when the chain is all there is).
namespace {

// refinement step s (1-based) of a solve with a block inverse of quality delta is due iff
// refine_steps(delta) >= s  <=>  delta > LR_REFINE_THR[s - 1]   (a NaN delta runs every step)
constexpr int LR_REFINE_MAX = 1;   // (each step is two launches on the chain, usually no-ops of ~45 us beside the update)
const double LR_REFINE_THR[3] = {0.0 /* = the tolerance, filled in at run time */, 3.1622776601683794e-8, 1e-5};

// What one call does with the switches: the only place that knows the thresholds.
struct CholPlan {
  int nbatch;
  int spin_limit;
  // One launch per panel (panel_fused_kernel) for single matrices / small batches: n = 4096 2.92 -> 2.50 ms,
  // 8192 8.05 -> 7.07, 16384 34.8 -> 33.4.  Large lock-step batches keep the pivot steps + strips: their
  // workgroups would spend the diagonal chain's 190 us spinning.
  // (round 3: lock-step batches of up to 16 gained 5-14 % from it as well, 32 and more lost.  Round 4, with the
  //  transposed panel -- tools/time_lml_batch.py, tools/r4_run18.sh: 32 matrices gain 4 % (n = 3000) to 20 % (n = 600),
  //  64 matrices 7-21 % up to n = 1500 and nothing at n = 3000: up to 32 matrices always, up to 64 while n <= 2048)
  int fused_max_batch;
  bool fused_mode;
  // Panel strips (panel_strip_kernel) for lock-step batches: there the pivot steps are throughput-bound
  // (64 matrices x 64 workgroups, each re-factoring the pivot block, one workgroup per CU) and the
  // K = 64 panel updates HBM-bound (1.85 GB per step).  A single matrix keeps the pivot-step / GEMM
  // pairs: its chain is bound by launch latency, which the strips do not shorten.
  // from how many row strips on: 129 in a lock-step batch (round 3, tools/prof_lml.py: 20 - 64 matrices of
  // n = 600 ... 2000 gain 5 - 20 % over the 513 of round 2; below ~100 strips the pivot steps win), 513 for a
  // single matrix (which takes the one-launch panel anyway unless that is switched off)
  int strips_min_wg;
  // the resident schedule solves the panels with the 512-block inverses: a caller that keeps none gets them from scratch
  bool borrow_inv;
  int64_t kb_lr;                              // panels [0, kb_lr) take the resident schedule

  bool strips(int64_t rem, int64_t nbk) const {
    const CholSwitches& sw = chol_switches();
    const int64_t wgs = (int64_t)nbatch * ((rem + PB - 1) / PB);
    return sw.strips_on && rem > 0 && nbk == CHOL_NB && wgs <= sw.strips_max_wg && wgs >= strips_min_wg;
  }
  // paired trailing updates while the trailing matrix is large (decided per pair, on the rows left
  // below its FIRST panel, so that both panels of a pair see the same answer)
  bool paired(int64_t kb, int64_t rem) const {
    const CholSwitches& sw = chol_switches();
    return sw.pair_on && ((kb & 1) ? rem + CHOL_NB : rem) > sw.pair_min_rem;
  }
};

CholPlan chol_plan(int64_t n, int nbatch, bool has_keep_inv, bool inv64_only, bool allow_lr, bool safe) {
  const CholSwitches& sw = chol_switches();
  const int64_t NB = CHOL_NB;
  CholPlan p;
  p.nbatch = nbatch;
  p.spin_limit = sw.spin_limit;
  p.fused_max_batch = sw.fused_max_batch >= 0 ? sw.fused_max_batch : (n <= 2048 ? 64 : 32);
  p.fused_mode = sw.fused_on && nbatch <= p.fused_max_batch && !safe;   // safe: no inter-workgroup hand-offs
  p.strips_min_wg = sw.strips_min_wg >= 0 ? sw.strips_min_wg : (nbatch > 1 ? 129 : 513);
  const int64_t lr_floor = sw.lr_min_rem > 640 ? sw.lr_min_rem : 640;     // >= 5 tile rows for the look-ahead order
  const bool lr_allowed = sw.lr_on && allow_lr && !safe && nbatch == 1 && !inv64_only;
  p.borrow_inv = !has_keep_inv && lr_allowed && n - NB >= lr_floor;
  p.kb_lr = 0;
  if (lr_allowed && (has_keep_inv || p.borrow_inv) && p.fused_mode) {
    while (n - (p.kb_lr + 1) * NB >= lr_floor) ++p.kb_lr;
    p.kb_lr &= ~(int64_t)1;                   // the chain schedule pairs panels from an even index on
  }
  return p;
}

// The buffers and strides of one call, and the panel the loop is at.
struct CholCall {
  dfh_ctx* ctx;
  CholPlan plan;
  double* A; int64_t n, lda, strideA; int nbatch;
  double* keep_inv; int64_t strideInv; bool inv64_only;
  int64_t nblk_all, clean_blocks;
  // Three streams.  P (high priority): the dependent chain -- 64-wide pivot steps over the panel,
  // each solving ALL rows below it by substitution, then the update of the next block column.
  // M (the caller's stream): the big trailing updates.  X (aux): everything the chain does not
  // need -- moving the pivot-block factors into place and the explicit 512-block inverses kept
  // for the triangular solves of the posterior.
  hipStream_t M, P, X;
  long long* d_info; unsigned long long* d_status;
  double *Lscr_all, *Iscr_all;                // factor scratch [parity][8][64][64] per matrix; the 16 x 16 inverses of those blocks, same parity scheme
  int* fsync_all;                             // [nbatch][FUSED_SYNC_INTS] counters of the fused panels
  int64_t strideL, strideT, strideI;
  double* T;
  double* d_delta;                            // [nbatch][nblk] quality of the kept block inverses
  GemmBatch bA;                               // every operand inside the batch matrices
  int* lr_sync;                               // per panel {diag workgroups resident, next diagonal block's tiles done, next block column's tiles done, -}
  double *lr_X, *lr_R;                        // the solved rows (two buffers, alternating), their residual (rows below the first panel x 512 each)
  int64_t lr_xstride;
  // the panel
  int64_t kb, k0, nbk, rem;                   // index, first column, width, rows below
  double *D, *Linv, *Lscr, *Iscr;             // diagonal block, its inverse's slot (or null), this parity's scratch
};

// The context's event slots of the factorisation (common.h: two per call, then five per panel).
enum CholEvent { CE_PANEL = 0, CE_TRAIL, CE_AUX, CE_DIAG, CE_COPY };
int call_event(dfh_ctx* ctx, int which, hipEvent_t* out) { return ctx_event(ctx, EV_CHOL_BASE + (size_t)which, out); }   // 0: start, 1: done
// (null for a panel before the first: nothing to wait for)
int panel_event(dfh_ctx* ctx, int64_t kb, CholEvent which, hipEvent_t* out) {
  *out = nullptr;
  return kb < 0 ? DFH_OK : ctx_event(ctx, EV_CHOL_BASE + 2 + 5 * (size_t)kb + (size_t)which, out);
}

FusedArgs fused_args(const CholCall& c) {
  FusedArgs fa;
  fa.D = c.D; fa.lda = c.lda; fa.Lfac = c.Lscr; fa.Linv16 = c.Iscr; fa.sync = c.fsync_all; fa.epoch = (int)c.kb + 1;
  fa.nbk = (int)c.nbk; fa.rows_below = (int)c.rem; fa.info = c.d_info; fa.pivot_base = (long)c.k0;
  fa.strideD = c.strideA; fa.strideL = c.strideL; fa.strideI = c.strideI;
  fa.status = c.d_status; fa.spin_limit = c.plan.spin_limit;
  fa.resident = nullptr; fa.wait_ptr = nullptr; fa.wait_target = 0; fa.prog_sleep = chol_switches().prog_sleep;
  return fa;
}

// ---- off the chain: factor blocks into place, 64-block inverses, 512-block inverse, its quality ----
// (X: the stream it runs on; after: what it waits for, or null)
int aux_block(const CholCall& c, hipEvent_t after, hipStream_t X) {
  dfh_ctx* ctx = c.ctx;
  const int64_t NB = CHOL_NB;
  hipEvent_t e_aux;
  DFH_TRY(panel_event(ctx, c.kb, CE_AUX, &e_aux));
  StreamSwap on_x(ctx, X);
  if (after) DFH_HIP(hipStreamWaitEvent(X, after, 0));
  const bool zero_in_trtri = X != ctx->aux && c.nbk == NB;     // resident panels: one launch less on the chain
  if (c.Linv && !zero_in_trtri) {
    if (c.nbatch == 1) {
      DFH_HIP(hipMemsetAsync(c.Linv, 0, (size_t)NB * NB * 8, X));
    } else {
      hipLaunchKernelGGL(k_zero_strided, dim3(64, (unsigned)c.nbatch), dim3(256), 0, X, c.Linv, (long)(NB * NB), (long)c.strideInv);
      DFH_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(trtri64_kernel, dim3((unsigned)((c.nbk + PB - 1) / PB), (unsigned)c.nbatch), dim3(256), 0, X,
                     c.D, (long)c.lda, (int)c.nbk, c.Linv, (long)NB, c.Lscr, (long)c.strideA, (long)c.strideInv,
                     (long)c.strideL, zero_in_trtri ? 1 : 0);
  DFH_LAUNCH_CHECK();
  if (c.Linv && !c.inv64_only) {
    DFH_TRY(assemble_block_inverse(ctx, c.D, c.lda, c.nbk, c.Linv, c.T, c.nbatch, c.strideA, c.strideInv, c.strideT));
    // clean copy of the block behind the inverses (keep_inv + nblk*NB*NB + ...) and delta = max|I - M L_bb|
    DFH_TRY(block_inverse_quality(ctx, c.D, c.lda, c.nbk, c.Linv, c.Linv + c.clean_blocks * NB * NB, c.T, c.d_delta + c.kb, c.nbatch,
                                  c.strideA, c.strideInv, c.strideT, c.nblk_all));
  }
  DFH_HIP(hipEventRecord(e_aux, X));
  return DFH_OK;
}

// =============== resident look-ahead panel (see the comment above this namespace) ===============
int panel_resident(const CholCall& c) {
  dfh_ctx* ctx = c.ctx;
  const int64_t NB = CHOL_NB, kb = c.kb, k0 = c.k0, rem = c.rem, lda = c.lda;
  const hipStream_t M = c.M, P = c.P, X = c.X;
  double* const A = c.A;
  const int spin_limit = c.plan.spin_limit;
  hipEvent_t e_panel, e_trail, e_diag, e_copy, e_aux_prev2, e_trail_prev2, e_copy_prev2;
  DFH_TRY(panel_event(ctx, kb, CE_PANEL, &e_panel));
  DFH_TRY(panel_event(ctx, kb, CE_TRAIL, &e_trail));
  DFH_TRY(panel_event(ctx, kb, CE_DIAG, &e_diag));
  DFH_TRY(panel_event(ctx, kb, CE_COPY, &e_copy));
  DFH_TRY(panel_event(ctx, kb - 2, CE_AUX, &e_aux_prev2));
  DFH_TRY(panel_event(ctx, kb - 2, CE_TRAIL, &e_trail_prev2));
  DFH_TRY(panel_event(ctx, kb - 2, CE_COPY, &e_copy_prev2));
  int* sy = c.lr_sync + 4 * kb;
  double* A21 = A + (k0 + NB) * lda + k0;          // rem x 512: the rows below the diagonal block
  double* Xk = c.lr_X + (kb & 1) * c.lr_xstride;
  {
    StreamSwap on_p(ctx, P);
    if (e_aux_prev2) DFH_HIP(hipStreamWaitEvent(P, e_aux_prev2, 0));     // factor scratch of this parity is free again
    // Not before update(kb-2) has finished: the eight workgroups need whole CUs, and a high-priority
    // launch that is PENDING because it does not fit throttles the dispatch of the running update
    // (measured: update(0) 2.42 ms with this launch enqueued after it, 2.52 / 2.71 ms with it pending
    // for the last 0.45 / 1.2 ms).  update(kb-1) cannot start before update(kb-2) has ended anyway.
    if (e_trail_prev2) DFH_HIP(hipStreamWaitEvent(P, e_trail_prev2, 0));
    FusedArgs fa = fused_args(c);
    fa.nbk = (int)NB; fa.rows_below = 0;
    fa.resident = sy;
    fa.wait_ptr = kb > 0 ? sy - 4 + 1 : nullptr;   // the sixteen... ten lower tiles of this diagonal block, out of update(kb-1)
    fa.wait_target = 10;
    hipLaunchKernelGGL(panel_fused_kernel, dim3((unsigned)(NB / PB), 1), dim3(256), FUSED_SMEM, P, fa);
    DFH_LAUNCH_CHECK();
    DFH_HIP(hipEventRecord(e_diag, P));
  }
  // the inverse is ON the chain here (the panel solve multiplies by it): it runs on the priority
  // stream -- on the auxiliary stream its small kernels wait for a slot behind the trailing update's
  // pending workgroups (trtri64: 36 us alone, 1.3 - 1.8 ms beside the update)
  DFH_TRY(aux_block(c, nullptr, P));
  {
    StreamSwap on_p(ctx, P);
    if (kb > 0) {
      // the whole block column has to be out of update(kb-1): 4 T - 6 look-ahead tiles over T tile rows
      const int64_t Tprev = (rem + NB + 127) / 128;
      hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, P, (const int*)(sy - 4 + 2), (int)(4 * Tprev - 6), c.d_status, spin_limit);
      DFH_LAUNCH_CHECK();
    }
    const double* Mi = c.Linv;                               // inverse of the diagonal block (lower, ld NB)
    const double* Lbb = c.Linv + c.clean_blocks * NB * NB;   // its clean copy
    // the solved rows go to a panel buffer of their own (two, alternating): the trailing update reads
    // them from there (contiguous, ld 512) and the copy into the factor happens off the chain
    if (e_copy_prev2) DFH_HIP(hipStreamWaitEvent(P, e_copy_prev2, 0));      // the buffer's previous contents are in place
    DFH_TRY(gemm_f64(ctx, GEMM_KTRI_B, rem, NB, NB, 1.0, A21, lda, Mi, NB, 0.0, nullptr, 0, Xk, NB));
    for (int st = 0; st < LR_REFINE_MAX; ++st) {
      // X <- X + (A21 - X L_bb^T) M^T, the right-hand side untouched; skipped on the device unless due
      ctx->gemm_cond = c.d_delta + kb;
      ctx->gemm_cond_thr = st == 0 ? chol_switches().refine_tol : LR_REFINE_THR[st];
      int rc_r = gemm_f64(ctx, GEMM_KTRI_B, rem, NB, NB, -1.0, Xk, NB, Lbb, NB, 1.0, A21, lda, c.lr_R, NB);
      if (rc_r == DFH_OK) rc_r = gemm_f64(ctx, GEMM_KTRI_B, rem, NB, NB, 1.0, c.lr_R, NB, Mi, NB, 1.0, Xk, NB, Xk, NB);
      ctx->gemm_cond = nullptr;
      DFH_TRY(rc_r);
    }
    DFH_HIP(hipEventRecord(e_panel, P));
  }
  {
    StreamSwap on_x(ctx, X);
    DFH_HIP(hipStreamWaitEvent(X, e_panel, 0));
    DFH_TRY(copy_matrix(ctx, Xk, NB, A21, lda, rem, NB));
    DFH_HIP(hipEventRecord(e_copy, X));
  }
  // ---- M: the whole trailing update with this panel, next block column first ----
  DFH_HIP(hipStreamWaitEvent(M, e_panel, 0));
  const bool next_resident = kb + 1 < c.plan.kb_lr;
  if (next_resident) {
    hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, M, (const int*)(sy + 4), (int)(NB / PB), c.d_status, spin_limit);
    DFH_LAUNCH_CHECK();
  }
  {
    double* C = A + (k0 + NB) * lda + (k0 + NB);
    ctx->gemm_la_cnt = next_resident ? sy + 1 : nullptr;
    const int rc_u = gemm_f64(ctx, GEMM_LOWER, rem, rem, NB, -1.0, Xk, NB, Xk, NB, 1.0, C, lda, C, lda);
    ctx->gemm_la_cnt = nullptr;
    DFH_TRY(rc_u);
  }
  DFH_HIP(hipEventRecord(e_trail, M));
  return DFH_OK;
}

// =============== chain panel: the look-ahead schedule of the comment above this namespace ===============
int panel_chain(const CholCall& c) {
  dfh_ctx* ctx = c.ctx;
  const int64_t NB = CHOL_NB, kb = c.kb, k0 = c.k0, nbk = c.nbk, rem = c.rem, lda = c.lda;
  const hipStream_t M = c.M, P = c.P;
  double* const A = c.A;
  const int nbatch = c.nbatch;
  const bool paired = c.plan.paired(kb, rem), strips = c.plan.strips(rem, nbk);
  hipEvent_t e_panel, e_trail, e_trail_prev, e_aux_prev2, e_copy_prev, e_copy_prev2;
  DFH_TRY(panel_event(ctx, kb, CE_PANEL, &e_panel));
  DFH_TRY(panel_event(ctx, kb, CE_TRAIL, &e_trail));
  DFH_TRY(panel_event(ctx, kb - 1, CE_TRAIL, &e_trail_prev));
  DFH_TRY(panel_event(ctx, kb - 2, CE_AUX, &e_aux_prev2));
  DFH_TRY(panel_event(ctx, kb - 1, CE_COPY, &e_copy_prev));
  DFH_TRY(panel_event(ctx, kb - 2, CE_COPY, &e_copy_prev2));
  {
    StreamSwap on_p(ctx, P);
    if (e_aux_prev2) DFH_HIP(hipStreamWaitEvent(P, e_aux_prev2, 0));     // factor scratch of this parity is free again
    // the last resident panel's update covered this block column too: it has to be complete, and
    // the last two resident panels' solved rows have to be in place
    if (kb == c.plan.kb_lr && kb > 0 && e_trail_prev) {
      DFH_HIP(hipStreamWaitEvent(P, e_trail_prev, 0));
      if (e_copy_prev) DFH_HIP(hipStreamWaitEvent(P, e_copy_prev, 0));
      if (e_copy_prev2) DFH_HIP(hipStreamWaitEvent(P, e_copy_prev2, 0));
    }
    const bool fused = c.plan.fused_mode;           // full panels, and the (last) partial one: identity padding
    if (fused) {
      // ---- the whole panel in one launch: diagonal block by eight flag-synchronised strips, rows below alongside ----
      const FusedArgs fa = fused_args(c);
      hipLaunchKernelGGL(panel_fused_kernel, dim3((unsigned)((nbk + PB - 1) / PB + (rem + PB - 1) / PB), (unsigned)nbatch),
                         dim3(256), FUSED_SMEM, P, fa);
      DFH_LAUNCH_CHECK();
    }
    // ---- 64-wide pivot steps: factor, solve every row below, update the rest of the panel ----
    for (int64_t j0 = 0; j0 < (fused ? 0 : nbk); j0 += PB) {
      const int w = (int)((nbk - j0 < PB) ? nbk - j0 : PB);
      double* Djj = c.D + j0 * lda + j0;
      const int64_t cols_left = nbk - j0 - w;            // panel columns still to be factored
      // every row below the pivot block -- or, with strips, only those inside the diagonal block
      const int64_t rows = cols_left + (strips ? 0 : rem);
      const unsigned nwg = 1 + (unsigned)((rows + PB - 1) / PB);
      hipLaunchKernelGGL(diag_step64_kernel, dim3(nwg, (unsigned)nbatch), dim3(256), DIAG_STEP_SMEM, P, Djj,
                         (long)lda, w, (int)rows, (long)(k0 + j0), c.d_info, c.Lscr + (j0 / PB) * PB * PB,
                         (long)c.strideA, (long)c.strideL, strips ? c.Iscr + (j0 / PB) * (4 * 16 * 17) : (double*)nullptr,
                         (long)c.strideI);
      DFH_LAUNCH_CHECK();
      if (cols_left > 0) {
        // A[r, c] -= L[r, j] L[c, j]^T for the rows below and the panel columns to the right
        // (the part above the diagonal of the block is scratch: only the lower triangle is L)
        double* Pn = c.D + (j0 + w) * lda + j0;                      // rows x w, already solved
        double* D22 = c.D + (j0 + w) * lda + (j0 + w);
        DFH_TRY(gemm_f64(ctx, 0, rows, cols_left, w, -1.0, Pn, lda, Pn, lda, 1.0, D22, lda, D22, lda, &c.bA));
      }
    }
    if (strips && !fused) {
      // ---- the rows below the diagonal block: L21 = A21 L11^-T, 64 rows per workgroup, one launch ----
      hipLaunchKernelGGL(panel_strip_kernel, dim3((unsigned)((rem + PB - 1) / PB), (unsigned)nbatch), dim3(256),
                         STRIP_SMEM, P, c.D, (long)lda, c.Lscr, c.Iscr, A + (k0 + nbk) * lda + k0, (int)rem,
                         (long)c.strideA, (long)c.strideL, (long)c.strideI);
      DFH_LAUNCH_CHECK();
    }
    DFH_HIP(hipEventRecord(e_panel, P));
    // ---- the next block column, so that the next panel can start before the trailing update ----
    if (rem > 0) {
      // kw = width of the panels whose contribution is still missing to the right of this one:
      // this panel alone, or -- in paired mode, after the second panel of a pair -- both
      const int64_t kw = (paired && (kb & 1)) ? nbk + NB : nbk;
      const double* A21 = A + (k0 + nbk) * lda + (k0 + nbk - kw);    // rem x kw, final
      if (e_trail_prev) DFH_HIP(hipStreamWaitEvent(P, e_trail_prev, 0));
      const int64_t nb1 = rem < NB ? rem : NB;
      double* C1 = A + (k0 + nbk) * lda + (k0 + nbk);   // rows k+1.., block column k+1
      DFH_TRY(gemm_f64(ctx, 0, rem, nb1, kw, -1.0, A21, lda, A21, lda, 1.0, C1, lda, C1, lda, &c.bA));
    }
  }
  DFH_TRY(aux_block(c, e_panel, c.X));
  // Paired mode: the trailing update runs after every SECOND panel, 1024 wide (the K = 512 update
  // reads and writes the C tile once per 512 columns of operand: 54 TF/s at n = 15872 against 63 for
  // K = 1024, tools/syrk_k.py).  The first panel of a pair only updates the next block column (the
  // look-ahead product above).  Its pivot chain then has no trailing update to run beside, which
  // costs most of what the wider update wins: n = 16384 35.2 -> 34.6 ms, n = 4096 2.82 -> 2.90 ms
  // -- hence only while more than DFH_CHOL_PAIR_MIN_REM rows are left.
  const bool trail_now = !paired || (kb & 1) || rem <= NB;
  if (rem > NB && trail_now) {
    const int64_t rem2 = rem - NB;
    const int64_t kw = (paired && (kb & 1)) ? nbk + NB : nbk;
    const double* A31 = A + (k0 + nbk + NB) * lda + (k0 + nbk - kw);   // rows k+2.. of the panel(s)
    double* A33 = A + (k0 + nbk + NB) * lda + (k0 + nbk + NB);
    DFH_HIP(hipStreamWaitEvent(M, e_panel, 0));
    DFH_TRY(gemm_f64(ctx, GEMM_LOWER, rem2, rem2, kw, -1.0, A31, lda, A31, lda, 1.0, A33, lda, A33, lda, &c.bA));
  }
  // (with nothing for M to do, the record keeps the event chain well-formed for the next panel's wait)
  DFH_HIP(hipEventRecord(e_trail, M));
  return DFH_OK;
}

}  // namespace

static int cholesky_device_impl(dfh_ctx* ctx, double* A, int64_t n, int64_t lda, double* keep_inv,
                                int64_t* info_pivot, int nbatch, int64_t strideA, int64_t strideKeep, int* refine_out,
                                bool inv64_only, bool allow_lr, bool safe, int64_t clean_blocks = 0) {
  DFH_ARG(nbatch >= 1 && nbatch <= CHOL_MAX_BATCH);
  if (info_pivot) for (int b = 0; b < nbatch; ++b) info_pivot[b] = 0;
  if (n <= 0) return DFH_OK;
  const int64_t NB = CHOL_NB;
  CholCall c;
  c.ctx = ctx; c.A = A; c.n = n; c.lda = lda; c.strideA = strideA; c.nbatch = nbatch; c.inv64_only = inv64_only;
  c.d_info = reinterpret_cast<long long*>(ctx->d_info);
  c.d_status = reinterpret_cast<unsigned long long*>(c.d_info + CHOL_MAX_BATCH + 8);
  const hipStream_t M = c.M = ctx->stream, P = c.P = ctx->side, X = c.X = ctx->aux;
  DFH_HIP(hipMemsetAsync(c.d_info, 0, 8 * (size_t)nbatch, M));
  DFH_HIP(hipMemsetAsync(c.d_status, 0, 8, M));
  const CholPlan plan = c.plan = chol_plan(n, nbatch, keep_inv != nullptr, inv64_only, allow_lr, safe);
  if (plan.borrow_inv) {
    DFH_TRY(scratch_get(ctx, SCR_CHOLKEEP, (size_t)inv_buffer_doubles(n) * 8, (void**)&keep_inv));
    refine_out = nullptr;
  }
  c.keep_inv = keep_inv;
  c.strideInv = keep_inv ? strideKeep : 0;          // between the batch matrices' inverse blocks
  c.strideL = 2 * (NB / PB) * PB * PB;               // factor scratch: [parity][8][64][64] per matrix
  c.strideT = NB * NB;
  c.strideI = 2 * (NB / PB) * (4 * 16 * 17);         // 16 x 16 inverses of those blocks, same parity scheme
  DFH_TRY(scratch_get(ctx, SCR_CHOLINV, ((size_t)nbatch * (c.strideL + c.strideI) + (size_t)nbatch * FUSED_SYNC_INTS / 2 + 2) * 8, (void**)&c.Lscr_all));
  c.Iscr_all = c.Lscr_all + (int64_t)nbatch * c.strideL;
  c.fsync_all = reinterpret_cast<int*>(c.Iscr_all + (int64_t)nbatch * c.strideI);
  if (plan.fused_mode) DFH_HIP(hipMemsetAsync(c.fsync_all, 0, (size_t)nbatch * FUSED_SYNC_INTS * sizeof(int), ctx->stream));
  c.T = nullptr;
  if (keep_inv) DFH_TRY(scratch_get(ctx, SCR_CHOLT, (size_t)nbatch * c.strideT * 8, (void**)&c.T));
  const int64_t nblk = c.nblk_all = (n + NB - 1) / NB;
  // blocks between an inverse and the clean copy of its diagonal block: the block count of the matrix
  // keep_inv was laid out for (this one, unless the call factors a diagonal sub-block of a larger one)
  c.clean_blocks = clean_blocks > 0 ? clean_blocks : nblk;
  c.d_delta = nullptr;
  if (keep_inv) DFH_TRY(scratch_get(ctx, SCR_DELTA, (size_t)nbatch * nblk * 8, (void**)&c.d_delta));
  c.bA.count = nbatch; c.bA.sA = c.bA.sB = c.bA.sCin = c.bA.sCout = strideA;

  static bool attr_set_dev[DFH_MAX_DEVICES] = {false};
  bool& attr_set = attr_set_dev[ctx->device];
  if (!attr_set) {
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(diag_step64_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, DIAG_STEP_SMEM));
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(panel_strip_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, STRIP_SMEM));
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(panel_fused_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, FUSED_SMEM));
    attr_set = true;
  }

  // ---- what the resident look-ahead needs (nothing may allocate inside the loop:
  //      hipMalloc can wait for the device, and a gate kernel may be waiting for a launch not yet enqueued) ----
  const int64_t kb_lr = plan.kb_lr;
  c.lr_sync = nullptr; c.lr_X = c.lr_R = nullptr;
  c.lr_xstride = (n - NB) * NB;
  if (kb_lr > 0) {
    DFH_TRY(scratch_get(ctx, SCR_CHOLSYNC, (size_t)kb_lr * 4 * sizeof(int), (void**)&c.lr_sync));
    DFH_HIP(hipMemsetAsync(c.lr_sync, 0, (size_t)kb_lr * 4 * sizeof(int), M));
    DFH_TRY(scratch_get(ctx, SCR_CHOLX, (size_t)2 * c.lr_xstride * 8, (void**)&c.lr_X));
    DFH_TRY(scratch_get(ctx, SCR_CHOLR, (size_t)(n - NB) * NB * 8, (void**)&c.lr_R));
  }
  hipEvent_t ev_start, ev_done, e_aux_last;
  DFH_TRY(call_event(ctx, 0, &ev_start));
  DFH_TRY(call_event(ctx, 1, &ev_done));
  DFH_HIP(hipEventRecord(ev_start, M));
  DFH_HIP(hipStreamWaitEvent(P, ev_start, 0));
  DFH_HIP(hipStreamWaitEvent(X, ev_start, 0));

  for (int64_t kb = 0; kb < nblk; ++kb) {
    c.kb = kb;
    c.k0 = kb * NB;
    c.nbk = (n - c.k0 < NB) ? n - c.k0 : NB;
    c.rem = n - c.k0 - c.nbk;
    c.Linv = keep_inv ? keep_inv + kb * NB * NB : nullptr;
    c.D = A + c.k0 * lda + c.k0;
    c.Lscr = c.Lscr_all + (kb & 1) * (NB / PB) * PB * PB;
    c.Iscr = c.Iscr_all + (kb & 1) * (NB / PB) * (4 * 16 * 17);
    DFH_TRY(kb < kb_lr ? panel_resident(c) : panel_chain(c));
  }
  DFH_HIP(hipEventRecord(ev_done, P));
  DFH_HIP(hipStreamWaitEvent(M, ev_done, 0));
  DFH_TRY(panel_event(ctx, nblk - 1, CE_AUX, &e_aux_last));
  DFH_HIP(hipStreamWaitEvent(M, e_aux_last, 0));

  DFH_HIP(hipMemcpyAsync(ctx->h_info, c.d_info, 8 * (size_t)nbatch, hipMemcpyDeviceToHost, M));
  DFH_HIP(hipMemcpyAsync(ctx->h_info + CHOL_MAX_BATCH + 8, c.d_status, 8, hipMemcpyDeviceToHost, M));
  std::vector<double> deltas;
  if (keep_inv && refine_out && inv64_only) {
    for (size_t i = 0; i < (size_t)nbatch * nblk; ++i) refine_out[i] = 0;
  } else if (keep_inv && (refine_out || kb_lr > 0)) {
    deltas.resize((size_t)nbatch * nblk);
    DFH_HIP(hipMemcpyAsync(deltas.data(), c.d_delta, deltas.size() * 8, hipMemcpyDeviceToHost, M));
  }
  DFH_HIP(hipStreamSynchronize(M));
  if (refine_out) for (size_t i = 0; i < deltas.size(); ++i) refine_out[i] = refine_steps(deltas[i]);
  const unsigned long long sync_status = (unsigned long long)ctx->h_info[CHOL_MAX_BATCH + 8];
  if (sync_status != 0) {
    // a bounded wait expired: whatever was computed after it is not to be trusted
    dfh_set_error("Cholesky: an inter-workgroup hand-off timed out (status %llx)", sync_status);
    return DFH_INTERNAL_RETRY;
  }
  int rc = DFH_OK;
  for (int b = 0; b < nbatch; ++b) {
    const int64_t piv = ctx->h_info[b];
    if (info_pivot) info_pivot[b] = piv;
    if (piv != 0 && rc == DFH_OK) {
      dfh_set_error("Matrix is not positive definite (pivot %lld)", (long long)piv);
      rc = DFH_ERR_NOT_PD;
    }
  }
  if (kb_lr > 0 && (rc == DFH_OK || rc == DFH_ERR_NOT_PD)) {
    // a resident panel solved its rows with the block inverse and at most LR_REFINE_MAX refinement steps
    // on the device; an inverse so poor that more are due sends the matrix through the substitution
    // schedule.  That also holds when a LATER pivot came out non-positive: the inaccurately solved
    // panel may be what broke it, and whether the matrix is positive definite (whether the caller's
    // stable_cholesky ladder adds jitter, general_utils.py:183-203) is for the substitution schedule
    // to decide.  The failed pivot's own block and those after it hold no meaningful delta.
    int64_t kb_hi = kb_lr;
    if (rc == DFH_ERR_NOT_PD) kb_hi = std::min<int64_t>(kb_lr, (ctx->h_info[0] - 1) / CHOL_NB);  // pivots are 1-based
    for (int64_t kb = 0; kb < kb_hi; ++kb)
      if (refine_steps(deltas[(size_t)kb]) > LR_REFINE_MAX) {
        dfh_set_error("Cholesky: diagonal block %lld too ill-conditioned for the inverse-based panel solve", (long long)kb);
        return DFH_INTERNAL_RETRY_COND;
      }
  }
  return rc;
}

// rebuild (optional): re-creates the input matrix in A (a failed or abandoned factorisation destroys
// it).  With it the call may use the schedules whose rare failure modes need a second attempt -- the
// resident look-ahead with its inverse-based panel solve; a hand-off timeout -- and repeats itself on
// the conservative schedule (no inter-workgroup waits, substitution only) when one occurs.  Without
// it such a failure is DFH_ERR_HIP.
int cholesky_device(dfh_ctx* ctx, double* A, int64_t n, int64_t lda, double* keep_inv,
                    int64_t* info_pivot, int nbatch, int64_t strideA, int64_t strideKeep, int* refine_out,
                    bool inv64_only, const std::function<int()>* rebuild) {
  static const bool force_safe = env_int("DFH_CHOL_SAFE", 0) != 0;
  // (Tried and dropped, round 3: a two-way recursion -- L11, the posterior's GEMM-based row solve for
  //  L21, ONE update of depth n/2, L22.  The deep update does run at 66 TF/s, but the row solve of only
  //  n/2 rows is a chain of 256-tile launches at half occupancy: n = 16384 34.6 ms against 31.8 with
  //  the resident look-ahead, n = 8192 8.7 against 7.0.)
  auto attempt = [&](bool allow_lr, bool safe) -> int {
    return cholesky_device_impl(ctx, A, n, lda, keep_inv, info_pivot, nbatch, strideA, strideKeep, refine_out,
                                inv64_only, allow_lr, safe);
  };
  const bool cooling = ctx->chol_cooldown > 0;
  if (cooling) --ctx->chol_cooldown;
  const bool safe_first = force_safe || cooling;
  int rc = attempt(rebuild != nullptr && !cooling, safe_first);
  static const bool verbose = env_int("DFH_CHOL_VERBOSE", 0) != 0;
  if (rc != DFH_INTERNAL_RETRY && rc != DFH_INTERNAL_RETRY_COND) { if (!cooling) ctx->chol_fallback_streak = 0; return rc; }
  ++ctx->chol_fallbacks;
  // only hand-off time-outs (a crowded device) feed the cool-down: an ill-conditioned block is a property of the
  // matrix, and two of those in a row -- common at the extremes of a hyper-parameter search -- must not push the next
  // 32 factorisations onto the slow schedule
  if (rc == DFH_INTERNAL_RETRY && ++ctx->chol_fallback_streak >= 2) { ctx->chol_cooldown = 32; ctx->chol_fallback_streak = 0; }
  if (verbose) fprintf(stderr, "dfhip: factorisation of n = %lld repeated on the safe schedule: %s\n", (long long)n, dfh_last_error());
  if (!rebuild || force_safe) return DFH_ERR_HIP;
  DFH_TRY((*rebuild)());
  rc = attempt(false, true);
  return (rc == DFH_INTERNAL_RETRY || rc == DFH_INTERNAL_RETRY_COND) ? DFH_ERR_HIP : rc;
}

static int ladder_pow(int p, double max_M, double* out) {
  *out = pow(10.0, (double)p) * max_M;      // (10 ** diag_noise_power) * max_M, general_utils.py:189
  return DFH_OK;
}

// factor dL (holding M) in place with the stable_cholesky ladder; M is re-created by `rebuild`
// when a retry is needed (the failed factorisation destroys it).
int stable_cholesky_device(dfh_ctx* ctx, double* dL, int64_t n, double* keep_inv, bool allow_jitter,
                           const std::function<int()>& rebuild, int32_t* jitter_power, double* jitter_added,
                           int64_t ld, int* refine_out) {
  if (ld == 0) ld = n;
  if (jitter_power) *jitter_power = INT32_MIN;
  if (jitter_added) *jitter_added = 0.0;
  int64_t piv = 0;
  int rc = cholesky_device(ctx, dL, n, ld, keep_inv, &piv, 1, 0, 0, refine_out, false, &rebuild);
  if (rc != DFH_ERR_NOT_PD || !allow_jitter) return rc;
  // general_utils.py:183-203
  DFH_TRY(rebuild());
  double max_M = 0.0;
  DFH_TRY(diag_max(ctx, dL, n, ld, &max_M));
  bool first = true;
  for (int p = -11; p < 5; ++p) {
    double diag_noise;
    ladder_pow(p, max_M, &diag_noise);
    if (!first) DFH_TRY(rebuild());
    first = false;
    DFH_TRY(add_diag(ctx, dL, n, ld, diag_noise));      // M + diag_noise * np.eye(n)
    const std::function<int()> rebuild_jit = [&]() -> int { DFH_TRY(rebuild()); return add_diag(ctx, dL, n, ld, diag_noise); };
    rc = cholesky_device(ctx, dL, n, ld, keep_inv, &piv, 1, 0, 0, refine_out, false, &rebuild_jit);
    if (rc == DFH_OK) {
      if (jitter_power) *jitter_power = p;
      if (jitter_added) *jitter_added = diag_noise;
      return DFH_OK;
    }
    if (rc != DFH_ERR_NOT_PD) return rc;
    if (p + 1 >= 5) {
      dfh_set_error("Could not compute Cholesky decomposition despite adding %0.4f to the diagonal. "
                    "This is likely because the M is not positive semi-definite or has infinities/nans.",
                    diag_noise);
      return DFH_ERR_JITTER;
    }
  }
  return DFH_ERR_JITTER;
}

int tri_block_inverses(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, double* inv, int* refine_out,
                       double* diag) {
  const int64_t NB = CHOL_NB;
  const int64_t nblk = (n + NB - 1) / NB;
  double* T = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_CHOLT, (size_t)NB * NB * 8, (void**)&T));
  double* d_delta = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_DELTA, (size_t)nblk * 8, (void**)&d_delta));
  if (!diag) diag = inv + nblk * NB * NB;
  for (int64_t k0 = 0; k0 < n; k0 += NB) {
    const int64_t nbk = (n - k0 < NB) ? n - k0 : NB;
    double* Linv = inv + (k0 / NB) * NB * NB;
    DFH_HIP(hipMemsetAsync(Linv, 0, (size_t)NB * NB * 8, ctx->stream));
    const double* D = L + k0 * ldl + k0;
    hipLaunchKernelGGL(trtri64_kernel, dim3((unsigned)((nbk + PB - 1) / PB)), dim3(256), 0, ctx->stream,
                       const_cast<double*>(D), (long)ldl, (int)nbk, Linv, (long)NB, (const double*)nullptr, 0L, 0L, 0L, 0);
    DFH_LAUNCH_CHECK();
    DFH_TRY(assemble_block_inverse(ctx, D, ldl, nbk, Linv, T));
    DFH_TRY(block_inverse_quality(ctx, D, ldl, nbk, Linv, diag + (k0 / NB) * NB * NB, T, d_delta + k0 / NB));
  }
  if (refine_out) {
    std::vector<double> deltas((size_t)nblk);
    DFH_HIP(hipMemcpyAsync(deltas.data(), d_delta, (size_t)nblk * 8, hipMemcpyDeviceToHost, ctx->stream));
    DFH_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t b = 0; b < nblk; ++b) refine_out[b] = refine_steps(deltas[b]);
  }
  return DFH_OK;
}

#ifdef DFH_DEBUG_HOOKS      // diagnostics: built only with `python -m dragonfly_amd.build --debug-hooks` (include/dfhip_debug.h)
// Diagnostics hook (not part of the product path): times `reps` back-to-back launches of the
// 64-wide diagonal step on a synthetic SPD block and returns in-kernel cycle stamps.
extern "C" int dfh_debug_diag_step(dfh_ctx* ctx, int reps, int rows_below, double* ms_per_launch,
                                   long long* cycles_out /* [7]: load, factor, trsm, waves 0-3 */) {
  DFH_ARG(ctx && reps > 0 && rows_below >= 0 && rows_below <= 448);
  DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(diag_step64_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, DIAG_STEP_SMEM));
  const int64_t nn = 512;
  double* A = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)nn * nn * 8, (void**)&A));
  std::vector<double> h((size_t)nn * nn, 0.01);
  for (int64_t i = 0; i < nn; ++i) h[i * nn + i] = 10.0 + (double)(i % 7);
  DFH_HIP(hipMemcpyAsync(A, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  long long* d_info = reinterpret_cast<long long*>(ctx->d_info);
  long long init[8] = {0, 0, 0, 0, 0, 0, 0, 1};
  DFH_HIP(hipMemcpyAsync(d_info + CHOL_MAX_BATCH, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  const unsigned nwg = 1 + (unsigned)((rows_below + PB - 1) / PB);
  hipEvent_t e0, e1;
  DFH_HIP(hipEventCreate(&e0));
  DFH_HIP(hipEventCreate(&e1));
  DFH_HIP(hipEventRecord(e0, ctx->stream));
  for (int r = 0; r < reps; ++r) {
    // the block is re-factored from its own output (still SPD: L has a dominant diagonal)
    hipLaunchKernelGGL(diag_step64_kernel, dim3(nwg), dim3(256), DIAG_STEP_SMEM, ctx->stream, A, (long)nn, 64,
                       rows_below, 0L, d_info, A + 256 * nn, 0L, 0L, (double*)nullptr, 0L);
  }
  DFH_HIP(hipEventRecord(e1, ctx->stream));
  DFH_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  DFH_HIP(hipEventElapsedTime(&ms, e0, e1));
  long long out[8];
  DFH_HIP(hipMemcpy(out, d_info + CHOL_MAX_BATCH, sizeof(out), hipMemcpyDeviceToHost));
  if (ms_per_launch) *ms_per_launch = ms / reps;
  if (cycles_out) { cycles_out[0] = out[2]; cycles_out[1] = out[3]; cycles_out[2] = out[4];
                    cycles_out[3] = out[0]; cycles_out[4] = out[1]; cycles_out[5] = out[5]; cycles_out[6] = out[6]; }
  long long zero[8] = {0};
  DFH_HIP(hipMemcpy(d_info + CHOL_MAX_BATCH, zero, sizeof(zero), hipMemcpyHostToDevice));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return DFH_OK;
}
// Diagnostics hook: `reps` launches of the one-launch panel on a synthetic SPD 512 x 512 block with `rows_below`
// rows under it; ms_out[reps] per launch (HIP events), stamps_out [(8 + strips below)][64] from the last launch.
// A_out (optional, [(512 + rows_below) x 512]): the input block; Lfac_out (optional, [8][64][64]): the factored
// 64 x 64 diagonal blocks as the strips published them -- for a host-side comparison with LAPACK.
extern "C" int dfh_debug_panel_data(double* A_out, double* Lfac_out);
static std::vector<double> g_dbg_A, g_dbg_L;
extern "C" int dfh_debug_panel_data(double* A_out, double* Lfac_out) {
  if (A_out) for (size_t i = 0; i < g_dbg_A.size(); ++i) A_out[i] = g_dbg_A[i];
  if (Lfac_out) for (size_t i = 0; i < g_dbg_L.size(); ++i) Lfac_out[i] = g_dbg_L[i];
  return (int)g_dbg_A.size();
}
extern "C" int dfh_debug_panel_stamps(dfh_ctx* ctx, int reps, int rows_below, double* ms_out, long long* stamps_out) {
  DFH_ARG(ctx && reps > 0 && rows_below >= 0 && ms_out && stamps_out);
  DFH_HIP(hipSetDevice(ctx->device));
  DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(panel_fused_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, FUSED_SMEM));
  const int64_t nn = 512, rows = nn + rows_below;
  const int nwg = (int)(nn / PB + (rows_below + PB - 1) / PB);
  std::vector<double> h((size_t)rows * nn);
  unsigned long long st = 88172645463325252ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) / 9007199254740992.0; };
  for (int64_t i = 0; i < rows; ++i)
    for (int64_t j = 0; j < nn; ++j) h[i * nn + j] = (i < nn && j > i) ? 0.0 : 0.02 * (rnd() - 0.5);
  for (int64_t i = 0; i < nn; ++i) { for (int64_t j = 0; j < i; ++j) h[j * nn + i] = h[i * nn + j]; h[i * nn + i] = 3.0 + rnd(); }
  double *master = nullptr, *D = nullptr, *scr = nullptr;
  long long* d_st = nullptr;
  DFH_HIP(hipMalloc(&master, h.size() * 8));
  DFH_HIP(hipMalloc(&D, h.size() * 8));
  const size_t scr_doubles = 8 * PB * PB + 8 * (4 * 16 * 17) + 64;
  DFH_HIP(hipMalloc(&scr, scr_doubles * 8));
  DFH_HIP(hipMalloc(&d_st, (size_t)nwg * 64 * 8));
  DFH_HIP(hipMemcpy(master, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  DFH_HIP(hipMemset(scr, 0, scr_doubles * 8));
  long long* d_info = reinterpret_cast<long long*>(ctx->d_info);
  hipEvent_t e0, e1;
  DFH_HIP(hipEventCreate(&e0)); DFH_HIP(hipEventCreate(&e1));
  hipStream_t S = ctx->side;
  for (int r = 0; r < reps; ++r) {
    DFH_HIP(hipMemcpyAsync(D, master, h.size() * 8, hipMemcpyDeviceToDevice, S));
    DFH_HIP(hipMemsetAsync(d_info, 0, 8 * (CHOL_MAX_BATCH + 16), S));
    DFH_HIP(hipMemsetAsync(d_st, 0, (size_t)nwg * 64 * 8, S));
    FusedArgs fa;
    fa.D = D; fa.lda = nn; fa.Lfac = scr; fa.Linv16 = scr + 8 * PB * PB;
    fa.sync = reinterpret_cast<int*>(scr + 8 * PB * PB + 8 * (4 * 16 * 17)); fa.epoch = r + 1;
    fa.nbk = (int)nn; fa.rows_below = rows_below; fa.info = d_info; fa.pivot_base = 0;
    fa.strideD = 0; fa.strideL = 0; fa.strideI = 0;
    fa.status = reinterpret_cast<unsigned long long*>(d_info + CHOL_MAX_BATCH + 8); fa.spin_limit = SPIN_LIMIT_DEFAULT;
    fa.resident = nullptr; fa.wait_ptr = nullptr; fa.wait_target = 0;
    fa.prog_sleep = chol_switches().prog_sleep;
    fa.stamps = d_st;
    DFH_HIP(hipEventRecord(e0, S));
    hipLaunchKernelGGL(panel_fused_kernel, dim3((unsigned)nwg, 1), dim3(256), FUSED_SMEM, S, fa);
    DFH_HIP(hipEventRecord(e1, S));
    DFH_HIP(hipStreamSynchronize(S));
    float ms = 0.f;
    DFH_HIP(hipEventElapsedTime(&ms, e0, e1));
    ms_out[r] = ms;
  }
  DFH_HIP(hipMemcpy(stamps_out, d_st, (size_t)nwg * 64 * 8, hipMemcpyDeviceToHost));
  g_dbg_A = h;
  g_dbg_L.resize((size_t)8 * PB * PB);
  DFH_HIP(hipMemcpy(g_dbg_L.data(), scr, g_dbg_L.size() * 8, hipMemcpyDeviceToHost));
  long long bad = 0;
  DFH_HIP(hipMemcpy(&bad, d_info, 8, hipMemcpyDeviceToHost));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(master); (void)hipFree(D); (void)hipFree(scr); (void)hipFree(d_st);
  if (bad != 0) { dfh_set_error("debug panel: pivot %lld failed", bad); return DFH_ERR_NOT_PD; }
  return DFH_OK;
}
#endif  // DFH_DEBUG_HOOKS
