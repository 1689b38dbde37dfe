// The triangular solves built on the factorisation's 512-block inverses (chol.hip keeps them, tri_block_inverses
// rebuilds them for an existing factor): the alpha solves trsv_* of GP.build_posterior (gp_core.py:161-163, replacing
// scipy.linalg.solve_triangular at general_utils.py:213) and the rows-as-right-hand-sides solves trsm_rows* of GP.eval
// (gp_core.py:180).  Every solve is GEMM / GEMV work; a block whose inverse is poor takes refinement steps
// (chol.hip: refine_steps).
#include "common.h"
#include <cmath>
#include <functional>
#include <utility>
#include <math.h>
#include <stdlib.h>

// Right-looking block substitution: once x_i is final it is pushed into every remaining row
// (wide, short GEMVs -> thousands of independent rows per launch instead of one long dependent
// chain).  The pass is HBM-bound: the lower triangle of L is read once per solve.
// ---------------------------------------------------------------------------------------------
// The two substitutions of GP.build_posterior (gp_core.py:161-163) on the 512-block inverses, round 6.
// A step of either direction is a chain of two dependent launches -- the block's solve by its explicit inverse, then the
// block's contribution to everything it feeds -- and the old steps spent their time INSIDE their kernels (trace of round
// 5: one workgroup per row of 4 KB in the forward update, 15 us; a partial + reduce pair of 16 + 6 us per transposed
// product; a device-to-device copy per step because the block's solve ran in place).  Here: r is updated in place, the
// solution goes to a vector of its own (no copy), and each kernel is shaped for its operand:
//   k_trsv_blk_fwd   z_b = M_b r_b             one wave per row of the lower-triangular inverse, columns <= row only
//   k_trsv_upd_fwd   r_i -= L[i, b] z_b        eight rows per wave, z_b in registers, 32 KB of loads in flight per wave
//   k_trsv_blk_bwd   a_b = M_b^T r_b           64 columns per workgroup, rows dealt to sixteen waves, one LDS reduce
//   k_trsv_upd_bwd   r_j -= L[b, j]^T a_b      64 columns per workgroup, a_b in LDS, sixteen row loads in flight per wave
// Sums run in a fixed order (deterministic); a block that needs refinement steps takes the general route below.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_trsv_blk_fwd(const double* __restrict__ M, int w, const double* __restrict__ r,
                                                      double* __restrict__ z) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= w) return;
  const double2_t* a = reinterpret_cast<const double2_t*>(M + (long)row * CHOL_NB);
  const double2_t* x = reinterpret_cast<const double2_t*>(r);
  double s0 = 0.0, s1 = 0.0;
  for (int j = lane; 2 * j <= row; j += 64) {          // (the inverse is exactly zero above its diagonal)
    const double2_t av = a[j], xv = x[j];
    s0 = fma(av.x, xv.x, s0);
    s1 = fma(av.y, (2 * j + 1 < w) ? xv.y : 0.0, s1);
  }
  double sum = s0 + s1;
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (lane == 0) z[row] = sum;
}

template <int TRSV_RPW>                                // rows per wave of the forward update
__global__ __launch_bounds__(256) void k_trsv_upd_fwd(const double* __restrict__ Lp, long ldl, long rows,
                                                      const double* __restrict__ z, double* __restrict__ r) {
  // Lp: the panel below the block (rows x 512, stride ldl); z: the block's solution (512); r: the rows' residuals
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long row0 = ((long)blockIdx.x * 4 + wv) * TRSV_RPW;
  if (row0 >= rows) return;
  double2_t zv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) zv[k] = reinterpret_cast<const double2_t*>(z)[lane + 64 * k];
  double2_t av[TRSV_RPW][4];
#pragma unroll
  for (int q = 0; q < TRSV_RPW; ++q) {
    const long row = row0 + q < rows ? row0 + q : rows - 1;     // (clamped: unconditional loads, results of the extra rows dropped)
    const double2_t* a = reinterpret_cast<const double2_t*>(Lp + row * ldl);
#pragma unroll
    for (int k = 0; k < 4; ++k) av[q][k] = a[lane + 64 * k];
  }
  double sum[TRSV_RPW];
#pragma unroll
  for (int q = 0; q < TRSV_RPW; ++q) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { s0 = fma(av[q][k].x, zv[k].x, s0); s1 = fma(av[q][k].y, zv[k].y, s1); }
    sum[q] = s0 + s1;
  }
#pragma unroll
  for (int q = 0; q < TRSV_RPW; ++q)
    for (int off = 32; off > 0; off >>= 1) sum[q] += __shfl_down(sum[q], off, 64);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < TRSV_RPW; ++q)
      if (row0 + q < rows) r[row0 + q] -= sum[q];
  }
}

// (the two transposed products walk DOWN 512 rows per column: with four waves a lane's chain of row loads is eight memory
//  latencies long -- 9.4 us even for the smallest update; sixteen waves of 32 rows each make it two)
constexpr int TRSV_BW = 16;                            // waves per workgroup of the backward kernels
// CW columns per workgroup (64: a lane per column; 16: four row phases inside the wave as well, for the block's own solve
// and the short updates -- eight workgroups of 256 KB each are bound by what ONE CU can pull from HBM, 8 us a launch)
template <int CW>
__device__ __forceinline__ void trsv_colsum(const double* __restrict__ p0, long ld, int row0, int w, const double* s_x,
                                            double (*s_p)[64], double& out, bool& writer) {
  // p0: column `cc` of the first row; rows row0 .. w - 1; lane (rp, c): row phase rp of 64 / CW, column c
  constexpr int RP = 64 / CW, PH = TRSV_BW * RP;       // row phases: per wave, per workgroup
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int rp = lane / CW;
  double s0 = 0.0, s1 = 0.0;
  int i = row0 + wv * RP + rp;
  for (; i + 15 * PH < w; i += 16 * PH) {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p0[(long)(i + PH * u) * ld];
#pragma unroll
    for (int u = 0; u < 16; u += 2) { s0 = fma(v[u], s_x[i + PH * u], s0); s1 = fma(v[u + 1], s_x[i + PH * (u + 1)], s1); }
  }
  for (; i < w; i += PH) s0 = fma(p0[(long)i * ld], s_x[i], s0);
  s_p[wv][lane] = s0 + s1;
  __syncthreads();
  writer = threadIdx.x < CW;
  double t = 0.0;
  if (writer) {
#pragma unroll
    for (int q = 0; q < TRSV_BW; ++q)
#pragma unroll
      for (int h = 0; h < RP; ++h) t += s_p[q][h * CW + lane];
  }
  out = t;
}

template <int CW>
__global__ __launch_bounds__(1024) void k_trsv_blk_bwd(const double* __restrict__ M, int w, const double* __restrict__ r,
                                                       double* __restrict__ out) {
  __shared__ double s_r[CHOL_NB];
  __shared__ double s_p[TRSV_BW][64];
  for (int i = threadIdx.x; i < CHOL_NB; i += 64 * TRSV_BW) s_r[i] = i < w ? r[i] : 0.0;
  __syncthreads();
  // out[col] = sum_{i >= col} M[i][col] r[i]: the inverse is exactly zero above its diagonal, so the rows start at
  // the workgroup's first column
  const int col = blockIdx.x * CW + (threadIdx.x & 63) % CW;
  const int cc = col < w ? col : w - 1;
  double t; bool writer;
  trsv_colsum<CW>(M + cc, CHOL_NB, blockIdx.x * CW, w, s_r, s_p, t, writer);
  if (writer && col < w) out[col] = t;
}

template <int CW>
__global__ __launch_bounds__(1024) void k_trsv_upd_bwd(const double* __restrict__ Lr, long ldl, int w, long cols,
                                                       const double* __restrict__ a, double* __restrict__ r) {
  // Lr: the block row (w x cols, stride ldl); a: the block's solution (w); r: the residuals of the columns before it
  __shared__ double s_a[CHOL_NB];
  __shared__ double s_p[TRSV_BW][64];
  for (int i = threadIdx.x; i < CHOL_NB; i += 64 * TRSV_BW) s_a[i] = i < w ? a[i] : 0.0;
  __syncthreads();
  const long col = (long)blockIdx.x * CW + (threadIdx.x & 63) % CW;
  const long cc = col < cols ? col : cols - 1;
  double t; bool writer;
  trsv_colsum<CW>(Lr + cc, ldl, 0, w, s_a, s_p, t, writer);
  if (writer && col < cols) r[col] -= t;
}

static bool trsv_fast_applies(const double* L, int64_t n, int64_t ldl, const double* inv, const double* x, const int* refine) {
  static const int on = env_int("DFH_TRSV_FAST", 1);
  if (!on || (ldl & 1) || ((reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(inv) | reinterpret_cast<uintptr_t>(x)) & 15)) return false;
  for (int64_t b = 0; refine && b < (n + CHOL_NB - 1) / CHOL_NB; ++b)
    if (refine[b] > 0) return false;
  return true;
}

// z = L^-1 r (r is used up) -- the forward half
static int trsv_fast_forward(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv, double* r, double* z) {
  const int64_t NB = CHOL_NB;
  for (int64_t c0 = 0; c0 < n; c0 += NB) {
    const int64_t w = std::min<int64_t>(NB, n - c0), below = n - c0 - w;
    hipLaunchKernelGGL(k_trsv_blk_fwd, dim3((unsigned)((w + 3) / 4)), dim3(256), 0, ctx->stream, inv + (c0 / NB) * NB * NB,
                       (int)w, r + c0, z + c0);
    DFH_LAUNCH_CHECK();
    ++ctx->solve_launches[SOLVE_TRSV_BLK_FWD];
    if (below > 4 * NB) {
      hipLaunchKernelGGL(k_trsv_upd_fwd<8>, dim3((unsigned)((below + 31) / 32)), dim3(256), 0, ctx->stream,
                         L + (c0 + w) * ldl + c0, (long)ldl, (long)below, z + c0, r + c0 + w);
      DFH_LAUNCH_CHECK();
      ++ctx->solve_launches[SOLVE_TRSV_UPD_FWD8];
    } else if (below > 0) {                            // a short panel: two rows per wave, four times the workgroups
      hipLaunchKernelGGL(k_trsv_upd_fwd<2>, dim3((unsigned)((below + 7) / 8)), dim3(256), 0, ctx->stream,
                         L + (c0 + w) * ldl + c0, (long)ldl, (long)below, z + c0, r + c0 + w);
      DFH_LAUNCH_CHECK();
      ++ctx->solve_launches[SOLVE_TRSV_UPD_FWD2];
    }
  }
  return DFH_OK;
}

// a = L^-T r (r is used up) -- the backward half
static int trsv_fast_backward(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv, double* r, double* a) {
  const int64_t NB = CHOL_NB, nblk = (n + NB - 1) / NB;
  for (int64_t b = nblk - 1; b >= 0; --b) {
    const int64_t c0 = b * NB, w = std::min<int64_t>(NB, n - c0);
    hipLaunchKernelGGL(k_trsv_blk_bwd<16>, dim3((unsigned)((w + 15) / 16)), dim3(64 * TRSV_BW), 0, ctx->stream, inv + b * NB * NB,
                       (int)w, r + c0, a + c0);
    DFH_LAUNCH_CHECK();
    ++ctx->solve_launches[SOLVE_TRSV_BLK_BWD];
    if (c0 > 0 && c0 < 8 * NB) {                       // fewer than 64 workgroups of 64 columns: 16 columns each
      hipLaunchKernelGGL(k_trsv_upd_bwd<16>, dim3((unsigned)((c0 + 15) / 16)), dim3(64 * TRSV_BW), 0, ctx->stream, L + c0 * ldl,
                         (long)ldl, (int)w, (long)c0, a + c0, r);
      DFH_LAUNCH_CHECK();
      ++ctx->solve_launches[SOLVE_TRSV_UPD_BWD16];
    } else if (c0 > 0) {
      hipLaunchKernelGGL(k_trsv_upd_bwd<64>, dim3((unsigned)((c0 + 63) / 64)), dim3(64 * TRSV_BW), 0, ctx->stream, L + c0 * ldl,
                         (long)ldl, (int)w, (long)c0, a + c0, r);
      DFH_LAUNCH_CHECK();
      ++ctx->solve_launches[SOLVE_TRSV_UPD_BWD64];
    }
  }
  return DFH_OK;
}

// x <- L^-T L^-1 x  (gp_core.py:161-163): the forward half leaves z in a scratch vector, the backward half reads it
// there and writes alpha to x -- no copy in between
int trsv_both(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv, double* x, const int* refine) {
  if (!trsv_fast_applies(L, n, ldl, inv, x, refine)) {
    DFH_TRY(trsv_forward(ctx, L, n, ldl, inv, x, refine));
    return trsv_backward(ctx, L, n, ldl, inv, x, refine);
  }
  double* z = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC3, (size_t)std::max<int64_t>(2 * CHOL_NB, n) * 8, (void**)&z));
  DFH_TRY(trsv_fast_forward(ctx, L, n, ldl, inv, x, z));
  return trsv_fast_backward(ctx, L, n, ldl, inv, z, x);
}

int trsv_forward(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv,
                 double* x, const int* refine) {
  const int64_t NB = CHOL_NB;
  if (trsv_fast_applies(L, n, ldl, inv, x, refine)) {
    double* z = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_VEC3, (size_t)std::max<int64_t>(2 * NB, n) * 8, (void**)&z));
    DFH_TRY(trsv_fast_forward(ctx, L, n, ldl, inv, x, z));
    DFH_HIP(hipMemcpyAsync(x, z, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return DFH_OK;
  }
  const int64_t nblk = (n + NB - 1) / NB;
  const double* diag = inv + nblk * NB * NB;
  double* tmp = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC3, (size_t)NB * 8 * 2, (void**)&tmp));
  double* res = tmp + NB;
  for (int64_t c0 = 0; c0 < n; c0 += NB) {
    const int64_t w = (n - c0 < NB) ? n - c0 : NB;
    const double* Mi = inv + (c0 / NB) * NB * NB;
    const double* Lbb = diag + (c0 / NB) * NB * NB;
    // x_i <- Linv_ii x_i
    DFH_TRY(gemv_rows(ctx, Mi, w, w, NB, x + c0, 1.0, nullptr, 0.0, tmp));
    ++ctx->solve_launches[SOLVE_TRSV_GENERAL_BLOCKS];
    for (int s = 0; s < (refine ? refine[c0 / NB] : 0); ++s) {
      // res = b_i - L_ii x ; x += Linv_ii res
      DFH_TRY(gemv_rows(ctx, Lbb, w, w, NB, tmp, -1.0, x + c0, 1.0, res, true));
      DFH_TRY(gemv_rows(ctx, Mi, w, w, NB, res, 1.0, tmp, 1.0, tmp));
      ++ctx->solve_launches[SOLVE_REFINE_STEPS];
    }
    DFH_HIP(hipMemcpyAsync(x + c0, tmp, (size_t)w * 8, hipMemcpyDeviceToDevice, ctx->stream));
    // x[i+1:] <- x[i+1:] - L[i+1:, i] x_i
    const int64_t below = n - c0 - w;
    if (below > 0)
      DFH_TRY(gemv_rows(ctx, L + (c0 + w) * ldl + c0, below, w, ldl, x + c0, -1.0, x + c0 + w, 1.0, x + c0 + w));
  }
  return DFH_OK;
}

int trsv_backward(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv,
                  double* x, const int* refine) {
  const int64_t NB = CHOL_NB;
  if (trsv_fast_applies(L, n, ldl, inv, x, refine)) {
    double* a = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_VEC3, (size_t)std::max<int64_t>(2 * NB, n) * 8, (void**)&a));
    DFH_TRY(trsv_fast_backward(ctx, L, n, ldl, inv, x, a));
    DFH_HIP(hipMemcpyAsync(x, a, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return DFH_OK;
  }
  const int64_t nblk = (n + NB - 1) / NB;
  const double* diag = inv + nblk * NB * NB;
  double* tmp = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC3, (size_t)NB * 8 * 2, (void**)&tmp));
  double* res = tmp + NB;
  for (int64_t b = nblk - 1; b >= 0; --b) {
    const int64_t c0 = b * NB;
    const int64_t w = (n - c0 < NB) ? n - c0 : NB;
    const double* Mi = inv + b * NB * NB;
    const double* Lbb = diag + b * NB * NB;
    // x_i <- Linv_ii^T x_i
    DFH_TRY(gemv_cols(ctx, Mi, w, w, NB, x + c0, 1.0, nullptr, 0.0, tmp));
    ++ctx->solve_launches[SOLVE_TRSV_GENERAL_BLOCKS];
    for (int s = 0; s < (refine ? refine[b] : 0); ++s) {
      // res = b_i - L_ii^T x ; x += Linv_ii^T res
      DFH_TRY(gemv_cols(ctx, Lbb, w, w, NB, tmp, -1.0, x + c0, 1.0, res));
      DFH_TRY(gemv_cols(ctx, Mi, w, w, NB, res, 1.0, tmp, 1.0, tmp));
      ++ctx->solve_launches[SOLVE_REFINE_STEPS];
    }
    DFH_HIP(hipMemcpyAsync(x + c0, tmp, (size_t)w * 8, hipMemcpyDeviceToDevice, ctx->stream));
    // x[:i] <- x[:i] - L[i, :i]^T x_i
    if (c0 > 0) DFH_TRY(gemv_cols(ctx, L + c0 * ldl, w, c0, ldl, x + c0, -1.0, x, 1.0, x));
  }
  return DFH_OK;
}

// residual buffer of the refined row solves (m x NB), only when some block takes a step
static int refine_scratch(dfh_ctx* ctx, const int* refine, int64_t nblk, int64_t m, double** out) {
  *out = nullptr;
  bool any = false;
  for (int64_t b = 0; refine && b < nblk; ++b) any = any || refine[b] > 0;
  if (any) DFH_TRY(scratch_get(ctx, SCR_REFINE, (size_t)m * CHOL_NB * 8, (void**)out));
  return DFH_OK;
}

// at most this many right-hand rows take the right-looking (wide, shallow) form of trsm_rows
constexpr int64_t TRSM_FEW_ROWS = 256;

int trsm_rows(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv,
              double* Kct, int64_t m, int64_t ldk, const int* refine, const double* diag_override) {
  if (m <= 0 || n <= 0) return DFH_OK;
  const int64_t NB = CHOL_NB;
  const double* diag = diag_override ? diag_override : inv + ((n + NB - 1) / NB) * NB * NB;      // clean copies of the diagonal blocks
  double *T = nullptr, *R2 = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_TMP, (size_t)m * NB * 8, (void**)&T));
  DFH_TRY(refine_scratch(ctx, refine, (n + NB - 1) / NB, m, &R2));
  if (m <= TRSM_FEW_ROWS) {
    // A handful of rows (single-point GP.eval calls, tree-search frontiers, hallucinated batches):
    // the left-looking form below would run each block as ONE tile row with a K loop over every
    // earlier column -- a few workgroups walking all of L serially.  Right-looking instead: solve
    // the block, then subtract its contribution from ALL later columns at once, a GEMM that is
    // (n - c0) / 128 tiles wide with K = 512, so L streams from HBM across the whole chip.
    for (int64_t c0 = 0; c0 < n; c0 += NB) {
      const int64_t w = (n - c0 < NB) ? n - c0 : NB;
      const int64_t rest = n - c0 - w;
      const double* Linv = inv + (c0 / NB) * NB * NB;
      const double* Lpanel = L + (c0 + w) * ldl + c0;
      // (the inverse block has an exactly zero upper part, so the full K range gives the same sum)
      // the solved block goes to T (a GEMM may not overwrite what other workgroups still read) and
      // has to end up in place as well: the few-row update below stages T anyway and writes the
      // copy on the side; only the last block, which has nothing to update, needs a copy launch
      const bool skinny_update = rest > 0 && gemm_skinny_applies(m, rest, w, T, NB, Lpanel, ldl) && (ldk % 2) == 0;
      if (gemm_skinny_applies(m, w, w, Kct + c0, ldk, Linv, NB))
        DFH_TRY(gemm_skinny_nt(ctx, m, w, w, 1.0, Kct + c0, ldk, Linv, NB, 0.0, nullptr, 0, T, NB));
      else
        DFH_TRY(gemm_f64(ctx, GEMM_KTRI_B, m, w, w, 1.0, Kct + c0, ldk, Linv, NB, 0.0, nullptr, 0, T, NB));
      for (int s = 0; s < (refine ? refine[c0 / NB] : 0); ++s) {
        // R <- B - X L_bb^T from the untouched right-hand side (it is only overwritten by the solution
        // below) ; X <- X + R Linv^T.  (Round 2 kept the residual IN PLACE of the right-hand side, which
        // is right for one step only: the second would subtract X0 L^T twice.)
        const double* Lbb = diag + (c0 / NB) * NB * NB;
        DFH_TRY(gemm_f64(ctx, GEMM_KTRI_B, m, w, w, -1.0, T, NB, Lbb, NB, 1.0, Kct + c0, ldk, R2, NB));
        DFH_TRY(gemm_f64(ctx, GEMM_KTRI_B, m, w, w, 1.0, R2, NB, Linv, NB, 1.0, T, NB, T, NB));
        ++ctx->solve_launches[SOLVE_REFINE_STEPS];
      }
      if (skinny_update) {
        DFH_TRY(gemm_skinny_nt(ctx, m, rest, w, -1.0, T, NB, Lpanel, ldl, 1.0, Kct + c0 + w, ldk,
                               Kct + c0 + w, ldk, Kct + c0, ldk));
      } else {
        DFH_TRY(copy_matrix(ctx, T, NB, Kct + c0, ldk, m, w));
        if (rest > 0)
          DFH_TRY(gemm_f64(ctx, 0, m, rest, w, -1.0, T, NB, Lpanel, ldl, 1.0, Kct + c0 + w, ldk,
                           Kct + c0 + w, ldk));
      }
    }
    return DFH_OK;
  }
  for (int64_t c0 = 0; c0 < n; c0 += NB) {
    const int64_t w = (n - c0 < NB) ? n - c0 : NB;
    // T = Kct[:, c0:c0+w] - Vt[:, 0:c0] * L[c0:c0+w, 0:c0]^T      (K = 0 degenerates to a copy)
    DFH_TRY(gemm_f64(ctx, 0, m, w, c0, -1.0, Kct, ldk, L + c0 * ldl, ldl, 1.0, Kct + c0, ldk, T, NB));
    // Vt[:, c0:c0+w] = T * Linv_ii^T
    const double* Linv = inv + (c0 / NB) * NB * NB;
    DFH_TRY(gemm_f64(ctx, GEMM_KTRI_B, m, w, w, 1.0, T, NB, Linv, NB, 0.0, nullptr, 0, Kct + c0, ldk));
    for (int s = 0; s < (refine ? refine[c0 / NB] : 0); ++s) {
      // R <- T - X L_bb^T (the residual of the right-hand side T, which stays) ; X <- X + R Linv^T
      const double* Lbb = diag + (c0 / NB) * NB * NB;
      DFH_TRY(gemm_f64(ctx, GEMM_KTRI_B, m, w, w, -1.0, Kct + c0, ldk, Lbb, NB, 1.0, T, NB, R2, NB));
      DFH_TRY(gemm_f64(ctx, GEMM_KTRI_B, m, w, w, 1.0, R2, NB, Linv, NB, 1.0, Kct + c0, ldk, Kct + c0, ldk));
      ++ctx->solve_launches[SOLVE_REFINE_STEPS];
    }
  }
  return DFH_OK;
}

int trsm_rows_backward(dfh_ctx* ctx, const double* L, int64_t n, int64_t ldl, const double* inv,
                       double* Bt, int64_t m, int64_t ldb, const int* refine) {
  if (m <= 0 || n <= 0) return DFH_OK;
  const int64_t NB = CHOL_NB;
  const double* diag = inv + ((n + NB - 1) / NB) * NB * NB;
  double *T = nullptr, *R2 = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_TMP, (size_t)m * NB * 8, (void**)&T));
  const int64_t nblk = (n + NB - 1) / NB;
  DFH_TRY(refine_scratch(ctx, refine, nblk, m, &R2));
  for (int64_t b = nblk - 1; b >= 0; --b) {
    const int64_t c0 = b * NB;
    const int64_t w = (n - c0 < NB) ? n - c0 : NB;
    const int64_t below = n - c0 - w;
    // T = Bt[:, c0:c0+w] - Xt[:, c0+w:] * L[c0+w:, c0:c0+w]
    DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, m, w, below, -1.0, Bt + c0 + w, ldb, L + (c0 + w) * ldl + c0, ldl,
                     1.0, Bt + c0, ldb, T, NB));
    // Xt[:, c0:c0+w] = T * Linv_ii
    DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, m, w, w, 1.0, T, NB, inv + b * NB * NB, NB, 0.0, nullptr, 0,
                     Bt + c0, ldb));
    for (int s = 0; s < (refine ? refine[b] : 0); ++s) {
      // R <- T - X L_bb (the residual of the right-hand side T, which stays) ; X <- X + R Linv
      DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, m, w, w, -1.0, Bt + c0, ldb, diag + b * NB * NB, NB, 1.0, T, NB, R2, NB));
      DFH_TRY(gemm_f64(ctx, GEMM_TRANSB, m, w, w, 1.0, R2, NB, inv + b * NB * NB, NB, 1.0, Bt + c0, ldb, Bt + c0, ldb));
      ++ctx->solve_launches[SOLVE_REFINE_STEPS];
    }
  }
  return DFH_OK;
}

extern "C" int dfh_ctx_solve_launches(dfh_ctx* ctx, int64_t* out) {
  DFH_ARG(ctx != nullptr && out != nullptr);
  for (int i = 0; i < SOLVE_COUNTERS; ++i) out[i] = ctx->solve_launches[i];
  return DFH_OK;
}
