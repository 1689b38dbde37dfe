// Thompson sampling, the joint draw with points in progress and the multi-objective acquisitions (include/dfhip.h).
#include "gp.h"
#include "argmax.h"
#include <algorithm>

namespace {

// S joint draws of one Thompson block in one launch: out[s][i] = mu[i] + sum_{j <= i} L[i][j] Ut[s][j], L the B x B lower
// factor (row-major; its strict upper triangle holds stale covariance and is never read), Ut the block's normals
// sample-major (row s at s * ldu).  One 256-thread workgroup per (tile of DRAW_TILE draws, row of L): the row is read
// once per tile, each element multiplied into the tile's DRAW_TILE accumulator pairs, and the tiles of a row are
// neighbours in the grid, so all but the first find the row in L2.  Per draw the arithmetic is k_gemv_rows' with
// tri_lower (runtime.hip) operation for operation -- the thread's strided fma chain (even / odd elements apart when
// `vec`, the condition under which that kernel takes its double2 path), the wave's shuffle tree, the four wave sums as
// (w0 + w1) + (w2 + w3), then + mu -- so draw s is bit for bit the single draw with column s of the normals.
#define DRAW_TILE 8
__global__ __launch_bounds__(256) void k_tri_draw(const double* __restrict__ L, long B, const double* __restrict__ Ut,
                                                  long ldu, int S, const double* __restrict__ mu,
                                                  double* __restrict__ out, long ldo, int vec) {
  __shared__ double sm[DRAW_TILE][4];
  const long row = blockIdx.y;
  const int s_lo = (int)blockIdx.x * DRAW_TILE;
  const int nt = S - s_lo < DRAW_TILE ? S - s_lo : DRAW_TILE;
  const double* a = L + row * B;
  const long n = row + 1;                                   // only columns j <= row
  const double* x[DRAW_TILE];                               // a short tile repeats its last draw: no branch in the loop
#pragma unroll
  for (int t = 0; t < DRAW_TILE; ++t) x[t] = Ut + (long)(s_lo + (t < nt ? t : nt - 1)) * ldu;
  double s0[DRAW_TILE], s1[DRAW_TILE];
#pragma unroll
  for (int t = 0; t < DRAW_TILE; ++t) { s0[t] = 0.0; s1[t] = 0.0; }
  if (vec) {
    const bool x2 = ((reinterpret_cast<uintptr_t>(Ut) & 15) == 0) && ((ldu & 1) == 0);
    const long n2 = n >> 1;
    for (long j = threadIdx.x; j < n2; j += 256) {
      const double2_t av = reinterpret_cast<const double2_t*>(a)[j];
#pragma unroll
      for (int t = 0; t < DRAW_TILE; ++t) {
        double2_t xv;
        if (x2) xv = reinterpret_cast<const double2_t*>(x[t])[j];
        else { xv.x = x[t][2 * j]; xv.y = x[t][2 * j + 1]; }
        s0[t] = fma(av.x, xv.x, s0[t]);
        s1[t] = fma(av.y, xv.y, s1[t]);
      }
    }
    if ((n & 1) && threadIdx.x == 0) {
      const double al = a[n - 1];
#pragma unroll
      for (int t = 0; t < DRAW_TILE; ++t) s0[t] = fma(al, x[t][n - 1], s0[t]);
    }
  } else {
    for (long j = threadIdx.x; j < n; j += 256) {
      const double aj = a[j];
#pragma unroll
      for (int t = 0; t < DRAW_TILE; ++t) s0[t] = fma(aj, x[t][j], s0[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < DRAW_TILE; ++t) {
    double s = s0[t] + s1[t];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) sm[t][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < nt) {
    const int t = threadIdx.x;
    const double v = (sm[t][0] + sm[t][1]) + (sm[t][2] + sm[t][3]);
    out[(long)(s_lo + t) * ldo + row] = v + mu[row];
  }
}

__global__ void k_add_vec(double* __restrict__ y, const double* __restrict__ a, double c, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = (a ? a[i] : 0.0) + c + y[i];
}

}  // namespace

// y[i] = (a ? a[i] : 0) + c + y[i]: the prior mean, per candidate or constant, onto K_tetr alpha
int add_vec(dfh_ctx* ctx, double* y, const double* a, double c, int64_t n) {
  hipLaunchKernelGGL(k_add_vec, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, y, a, c, (long)n);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

namespace {

// Multi-objective scalarisations (opt/multiobjective_gpb_acquisitions.py:19-107), one value per candidate from the k
// rows of A (posterior means, or joint draws) and S (posterior standard deviations; UCB only), row i at i * ld.
// The reference's order of operations, quirks included: the Tchebychev UCB takes the square root of the standard
// deviation (:102-103); np.minimum gives NaN when either operand is NaN.
struct MoParams { double w[DFH_MO_MAX_OBJECTIVES]; double ref[DFH_MO_MAX_OBJECTIVES]; };
__device__ __forceinline__ double np_minimum(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return a < b ? a : b;
}
__global__ void k_mo_scalarise(int scal, int ucb, int k, double beta, MoParams par, const double* __restrict__ A,
                               const double* __restrict__ S, long ld, long m, double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double v;
  if (scal == DFH_MO_LIN) {
    double tot = 0.0, s2 = 0.0;
    for (int j = 0; j < k; ++j) {
      const double w = par.w[j];
      tot = tot + A[j * ld + i] * w;                         // :38 (s += sample * weight), :86 (mu_tot += mu * weight)
      if (ucb) { const double sd = S[j * ld + i]; s2 = s2 + (sd * sd) * (w * w); }   // :87
    }
    v = ucb ? tot + beta * sqrt(s2) : tot;                   // :88
  } else {
    v = INFINITY;                                            // :61, :99
    for (int j = 0; j < k; ++j) {
      double t = A[j * ld + i];
      if (ucb) t = t + beta * sqrt(S[j * ld + i]);           // :103, the square root of 'std' as there
      v = np_minimum(v, (t - par.ref[j]) / par.w[j]);        // :64, :103-104
    }
  }
  out[i] = v;
}

// Point-wise multi-objective Thompson sampling (dfh_mo_ts_pointwise), all m candidates in one launch, one candidate per
// thread: from objective j's posterior mean MU[j * ld + i] and unclipped standard deviation SD[j * ld + i]
// (k_posterior_acq's) and the normal U[i * k + j] -- POINT-major, the order the reference's loops draw them in -- the
// one-point draw s = sd u + mu of k_ts_pointwise (product and sum rounded apart), written to S[j * ld + i] where wanted;
// the k draws scalarised in registers by k_mo_scalarise's TS formulas, in its order; then the first stage of the arg-max,
// one partial winner per workgroup (argmax_finish does the rest).  *bad is set when some sd is not > 0 (NaN included),
// where the reference's 1 x 1 stable_cholesky fails on every rung of its ladder.
__global__ __launch_bounds__(256) void k_mo_ts_pointwise(
    int scal, int k, MoParams par, const double* __restrict__ MU, const double* __restrict__ SD, long ld,
    const double* __restrict__ U, long m, double* __restrict__ S, double* __restrict__ vals, double* __restrict__ pv,
    long* __restrict__ pi, int* __restrict__ bad) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double bv = -INFINITY; long bi = ARGMAX_NONE;
  int not_pd = 0;
  if (i < m) {
    double v = scal == DFH_MO_LIN ? 0.0 : INFINITY;            // :33 / :58
    for (int j = 0; j < k; ++j) {
      const double sd = SD[j * ld + i];
      not_pd |= !(sd > 0.0);
      const double s = sd * U[i * k + j] + MU[j * ld + i];
      if (S) S[j * ld + i] = s;
      if (scal == DFH_MO_LIN) v = v + s * par.w[j];            // :38
      else v = np_minimum(v, (s - par.ref[j]) / par.w[j]);     // :64
    }
    bv = v; bi = i;
    vals[i] = v;
  }
  not_pd = __syncthreads_or(not_pd);
  block_argmax(bv, bi);
  if (threadIdx.x == 0) {
    pv[blockIdx.x] = bv; pi[blockIdx.x] = bi;
    if (not_pd) atomicOr(bad, 1);
  }
}

// What the multi-objective entry points demand of their arguments (include/dfhip.h)
int mo_check(dfh_gp* const* gps, int32_t k, int scal, const double* weights, const double* refs, MoParams* par) {
  DFH_ARG(gps && k >= 1 && k <= DFH_MO_MAX_OBJECTIVES && weights);
  DFH_ARG(scal == DFH_MO_LIN || scal == DFH_MO_TCH);
  DFH_ARG(scal == DFH_MO_LIN || refs);
  for (int i = 0; i < k; ++i) {
    DFH_ARG(gps[i] && !gps[i]->gram);            // needs the kernels
    DFH_ARG(gps[i]->ctx == gps[0]->ctx && gps[i]->d == gps[0]->d);
    DFH_ARG(scal == DFH_MO_LIN || weights[i] != 0.0);
    par->w[i] = weights[i];
    par->ref[i] = (scal == DFH_MO_TCH) ? refs[i] : 0.0;
  }
  for (int i = k; i < DFH_MO_MAX_OBJECTIVES; ++i) { par->w[i] = 0.0; par->ref[i] = 0.0; }
  return DFH_OK;
}

// Rows per posterior chunk with K fitted GPs resident: pick_chunk's figure, and never more than an eighth of what
// is free NOW -- with the K factors (K x n^2 x 8 bytes), their block inverses and everything else the caller keeps in
// HBM already taken out -- plus the context's own scratch, which the chunk reuses.
int64_t mo_pick_chunk(dfh_ctx* ctx, int64_t n_max, int64_t m) {
  int64_t mc = pick_chunk(ctx, n_max, m);
  size_t avail = 0;
  if (free_plus_own_scratch(ctx, &avail)) {
    int64_t cap = (int64_t)(avail / 8 / ((size_t)(n_max > 0 ? n_max : 1) * 8));
    cap = std::max<int64_t>(512, (cap / 512) * 512);
    if (mc > cap) mc = cap;
  }
  return mc;
}

// The blocked-joint draw of dfh_gp_ts (include/dfhip.h) for one GP.  `gp` gives the mean; the block covariances come from
// `cov_gp`'s factor -- gp itself, or the augmented GP of the hallucination's fall-back (HallucScope) -- and, with `hq` rows
// (the block form of the q in-progress points, gp_core.py:192-220), lose the rank-q term V2^T V2 as well.
// samples_dev (optional, device [m]) receives the draw without a trip to the host; the arg-max is skipped when neither
// best_val nor best_idx is wanted (the multi-objective call scalarises K draws first).
// S > 1 (dfh_gp_draw): U is [m x S] row-major, np.random.normal(size=(m, S)), and every block's factor serves all S draws
// in one launch of k_tri_draw; samples_dev / samples_out are then [S x m] and best_val / best_idx [S].  S == 1 runs the
// code, kernels and synchronisation points it always ran.
struct Stage1 { ChunkOut co; double* mu; };      // what the bulk-stream half left for one parity
struct TsRun {
  // the call: filled by the caller
  const HallucScope& hs;                         // the points in progress, resolved
  dfh_gp* gp; dfh_gp* cov_gp;
  int64_t hq;                                    // rows of the block form's second block row (0: none)
  const double* Xs = nullptr; int64_t m = 0, block = 0;
  const double* U = nullptr;
  double mean_const = 0.0; const double* mean_vals = nullptr;
  double* samples_dev = nullptr; double* samples_out = nullptr;
  double* best_val = nullptr; int64_t* best_idx = nullptr;
  int32_t* jitter_powers_out = nullptr;
  int32_t S = 1;
  // ts_setup
  dfh_ctx* ctx; int64_t n = 0;
  int64_t mc_max = 0, nchunks = 0, lb_slots = 0;
  ChunkStager stage; bool u_dev = false;
  double* vec[2] = {nullptr, nullptr};           // per parity: mu | draw | spare (ss2 / unused mean)
  double* Lb = nullptr;                          // lb_slots block factors
  DevBlock multi; int64_t ldu = 0;               // S > 1 only
  double* Ut = nullptr; double* sampS = nullptr; double* win_v = nullptr; long* win_i = nullptr;
  std::vector<double> hv; std::vector<long> hi;
  hipStream_t mainS = nullptr, bulkS = nullptr;
  hipEvent_t ev_in = nullptr, ev_ready[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
  Stage1 st[2];
  // the chunk in stage 2
  int p = 0; int64_t i0 = 0, mc = 0;
  const double* u_c = nullptr; double* mu_raw = nullptr; double* samp = nullptr;
  int64_t blk_idx = 0;                           // blocks of the chunks before it
  Winner win; std::vector<Winner> winS;          // the single draw's winner / one per draw
  explicit TsRun(const HallucScope& scope)
      : hs(scope), gp(scope.gp), cov_gp(scope.cov_gp()), hq(scope.block_q()), ctx(scope.gp->ctx), multi(scope.gp->ctx) {}
};

// sizes, scratch, the S > 1 block, the events
int ts_setup(TsRun& r) {
  dfh_ctx* ctx = r.ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  r.n = r.cov_gp->n;
  const int32_t S = r.S;
  if (r.block > r.m) r.block = r.m;
  DFH_ARG((double)r.block * (double)r.block * 8.0 < 32e9);
  // several TS blocks share one posterior chunk so the TRSM runs on big GEMMs
  int64_t bpc = std::max<int64_t>(1, pick_chunk(ctx, r.n, r.m) / r.block);
  r.mc_max = std::min(r.m, bpc * r.block);
  r.nchunks = (r.m + r.mc_max - 1) / r.mc_max;
  r.stage = ChunkStager(ctx, r.Xs, r.gp->d, r.mean_vals);
  r.u_dev = is_device_ptr(r.U);
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)r.mc_max * 8 * 3, (void**)&r.vec[0]));      // mu | draw | spare (ss2 / unused mean)
  DFH_TRY(scratch_get(ctx, SCR_VECB, (size_t)r.mc_max * 8 * 3, (void**)&r.vec[1]));
  // up to DFH_TS_BATCH (64) blocks of a chunk are factored as one lock-step batch
  static const int ts_batch = std::min(std::max(env_int("DFH_TS_BATCH", 64), 1), CHOL_MAX_BATCH);
  r.lb_slots = std::max<int64_t>(1, std::min<int64_t>(ts_batch, r.mc_max / r.block));
  DFH_TRY(scratch_get(ctx, SCR_TSL, (size_t)r.lb_slots * r.block * r.block * 8, (void**)&r.Lb));
  // S > 1: the chunk's normals sample-major (even leading dimension: a block's offset alone decides the 16-byte
  // alignment, as it does for the single draw's vector) | its S draws, rows tight | the per-draw winners
  r.ldu = (r.mc_max + 1) & ~(int64_t)1;
  if (S > 1) {
    DFH_TRY(dev_alloc(ctx, ((size_t)S * r.ldu + (size_t)S * r.mc_max + 2 * (size_t)S) * 8, &r.multi.p));
    r.Ut = static_cast<double*>(r.multi.p);
    r.sampS = r.Ut + (int64_t)S * r.ldu;
    r.win_v = r.sampS + (int64_t)S * r.mc_max;
    r.win_i = reinterpret_cast<long*>(r.win_v + S);
    r.hv.resize(S); r.hi.resize(S); r.winS.assign(S, Winner());
  }
  r.mainS = ctx->stream; r.bulkS = ctx->bulk;
  DFH_TRY(ctx_event(ctx, EV_TS_BASE, &r.ev_in));
  for (int p = 0; p < 2; ++p) {
    DFH_TRY(ctx_event(ctx, EV_TS_BASE + 1 + p, &r.ev_ready[p]));
    DFH_TRY(ctx_event(ctx, EV_TS_BASE + 3 + p, &r.ev_free[p]));
  }
  DFH_HIP(hipEventRecord(r.ev_in, r.mainS));
  DFH_HIP(hipStreamWaitEvent(r.bulkS, r.ev_in, 0));        // inputs produced on the main stream are ready
  return DFH_OK;
}

// the bulk-stream half of chunk c: cross kernel matrix, mu and the posterior TRSM into its parity's buffers
int ts_stage1(TsRun& r, int64_t c) {
  dfh_ctx* ctx = r.ctx;
  dfh_gp* gp = r.gp;
  const int p = (int)(c & 1);
  const int64_t i0 = c * r.mc_max;
  const int64_t mc = std::min(r.mc_max, r.m - i0);
  StreamSwap on_bulk(ctx, r.bulkS);
  if (c >= 2) DFH_HIP(hipStreamWaitEvent(r.bulkS, r.ev_free[p], 0));   // parity buffers released by stage 2
  const double* xs_c = nullptr;
  DFH_TRY(r.stage.xs(i0, mc, p ? SCR_STAGE_A2 : SCR_STAGE_A, &xs_c));
  Stage1& st = r.st[p];
  st.mu = r.vec[p];
  st.co = ChunkOut();
  ChunkReq rq;
  rq.parity = p;
  // V^T of the factor the covariances come from; the last third of the parity's vector is ss2 or the unused mean
  double* spare = r.vec[p] + 2 * r.mc_max;
  DFH_TRY(halluc_chunk(r.hs, xs_c, mc, gp->d, rq, st.mu, nullptr, spare, spare, &st.co));
  DFH_HIP(hipEventRecord(r.ev_ready[p], r.bulkS));
  return DFH_OK;
}

// one TS block: Sigma = K(Xb,Xb) - V^T V (gp_core.py:179-181; chol reads the lower triangle),
// stable_cholesky (general_utils.py:229), s = L u + mu (general_utils.py:231)
int ts_sigma_kernel(TsRun& r, int64_t b0, int64_t B, double* dst) {
  const KernDev& kd = r.cov_gp->kd;
  const double* Xbp = r.st[r.p].co.Xsp + b0 * kd.P;
  const double* Nbp = r.st[r.p].co.Nsp + b0 * kd.n_parts;
  return kernmat_gram(r.ctx, kd, 0, kd.n_parts, true, KmPts{Xbp, Nbp, B}, 0.0, dst, B);
}

int ts_single_block(TsRun& r, int64_t b0, int64_t B, double* dst, int64_t bidx) {
  dfh_ctx* ctx = r.ctx;
  const int64_t n = r.n, hq = r.hq;
  const double* Vt = r.st[r.p].co.Kct + b0 * n;
  auto build_sigma = [&]() -> int {
    DFH_TRY(ts_sigma_kernel(r, b0, B, dst));
    DFH_TRY(gemm_f64(ctx, GEMM_LOWER, B, B, n, -1.0, Vt, n, Vt, n, 1.0, dst, B, dst, B));
    if (hq == 0) return DFH_OK;
    const double* V2t = r.st[r.p].co.T + b0 * hq;           // second block row of the augmented solve: Sigma -= V2^T V2
    return gemm_f64(ctx, GEMM_LOWER, B, B, hq, -1.0, V2t, hq, V2t, hq, 1.0, dst, B, dst, B);
  };
  DFH_TRY(build_sigma());
  int32_t jp = INT32_MIN;
  DFH_TRY(stable_cholesky_device(ctx, dst, B, nullptr, true, build_sigma, &jp, nullptr));
  if (r.jitter_powers_out) r.jitter_powers_out[bidx] = jp;
  return DFH_OK;
}

// s = L u + mu of one factored block: the single draw's kernel, or all S draws in one launch.  `vec` is the single
// draw's choice of summation order for this block (gemv_rows: even leading dimension, factor and normals 16-byte
// aligned -- the caller's U taken to be aligned as a whole), so that draw s is that call's with column s.
int ts_draw_block(TsRun& r, const double* Lf, int64_t b0, int64_t B) {
  dfh_ctx* ctx = r.ctx;
  if (r.S == 1) return gemv_rows(ctx, Lf, B, B, B, r.u_c + b0, 1.0, r.mu_raw + b0, 1.0, r.samp + b0, true);
  const int vec = ((B & 1) == 0) && ((reinterpret_cast<uintptr_t>(Lf) & 15) == 0) && ((((r.u_dev ? r.i0 : 0) + b0) & 1) == 0);
  hipLaunchKernelGGL(k_tri_draw, dim3((unsigned)((r.S + DRAW_TILE - 1) / DRAW_TILE), (unsigned)B), dim3(256), 0, ctx->stream,
                     Lf, (long)B, (const double*)(r.Ut + b0), (long)r.ldu, (int)r.S, (const double*)(r.mu_raw + b0), r.sampS + b0,
                     (long)r.mc, vec);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

// the blocks of the chunk in stage 2, factored and drawn: full blocks in lock-step groups, then the ragged one
int ts_factor_chunk(TsRun& r) {
  dfh_ctx* ctx = r.ctx;
  const int64_t n = r.n, hq = r.hq, block = r.block, lb_slots = r.lb_slots;
  double* Lb = r.Lb;
  const double* Kct = r.st[r.p].co.Kct;
  const int64_t nfull = r.mc / block;
  for (int64_t g0 = 0; g0 < nfull; g0 += lb_slots) {
    // the equal-sized blocks of the chunk are factored in lock-step: one batched launch sequence
    // instead of `nb` latency-bound ones
    const int nb = (int)std::min<int64_t>(lb_slots, nfull - g0);
    const int64_t B = block;
    SectionTimer t(ctx, DFH_T_TS);
    if (nb == 1) {
      DFH_TRY(ts_single_block(r, g0 * B, B, Lb, r.blk_idx + g0));
    } else {
      // (also the rebuild closure of the factorisation: small groups take the one-launch panels, whose
      //  hand-offs are bounded waits -- on expiry, e.g. with other contexts crowding the device, the group
      //  is rebuilt and factored on the schedule without inter-workgroup waits)
      const std::function<int()> build_group = [&]() -> int {
        for (int b = 0; b < nb; ++b) DFH_TRY(ts_sigma_kernel(r, (g0 + b) * B, B, Lb + b * B * B));
        GemmBatch bs;
        bs.count = nb; bs.sA = bs.sB = B * n; bs.sCin = bs.sCout = B * B;
        const double* Vt = Kct + g0 * B * n;
        DFH_TRY(gemm_f64(ctx, GEMM_LOWER, B, B, n, -1.0, Vt, n, Vt, n, 1.0, Lb, B, Lb, B, &bs));
        if (hq == 0) return DFH_OK;
        GemmBatch bh;
        bh.count = nb; bh.sA = bh.sB = B * hq; bh.sCin = bh.sCout = B * B;
        const double* V2t = r.st[r.p].co.T + g0 * B * hq;
        return gemm_f64(ctx, GEMM_LOWER, B, B, hq, -1.0, V2t, hq, V2t, hq, 1.0, Lb, B, Lb, B, &bh);
      };
      DFH_TRY(build_group());
      int64_t piv[CHOL_MAX_BATCH] = {0};
      int rc = cholesky_device(ctx, Lb, B, B, nullptr, piv, nb, B * B, 0, nullptr, false, &build_group);
      if (rc != DFH_OK && rc != DFH_ERR_NOT_PD) return rc;
      for (int b = 0; b < nb; ++b) {
        if (piv[b] == 0) { if (r.jitter_powers_out) r.jitter_powers_out[r.blk_idx + g0 + b] = INT32_MIN; continue; }
        // this block needs the jitter ladder: redo it alone (rebuilds Sigma first)
        DFH_TRY(ts_single_block(r, (g0 + b) * B, B, Lb + b * B * B, r.blk_idx + g0 + b));
      }
    }
    for (int b = 0; b < nb; ++b) {
      const int64_t b0 = (g0 + b) * B;
      DFH_TRY(ts_draw_block(r, Lb + b * B * B, b0, B));
    }
  }
  if (nfull * block < r.mc) {           // ragged last block
    const int64_t b0 = nfull * block, B = r.mc - b0;
    SectionTimer t(ctx, DFH_T_TS);
    DFH_TRY(ts_single_block(r, b0, B, Lb, r.blk_idx + nfull));
    DFH_TRY(ts_draw_block(r, Lb, b0, B));
  }
  r.blk_idx += (r.mc + block - 1) / block;
  return DFH_OK;
}

// the finished chunk's winners and samples: the single draw, or the S draws
int ts_collect(TsRun& r) {
  dfh_ctx* ctx = r.ctx;
  const int64_t m = r.m, mc = r.mc, i0 = r.i0;
  const int32_t S = r.S;
  hipStream_t mainS = r.mainS;
  const bool want_best = r.best_val || r.best_idx;
  if (S > 1) {
    if (want_best) {
      DFH_TRY(argmax_rows(ctx, mainS, r.sampS, S, mc, mc, r.win_v, r.win_i));
      DFH_HIP(hipMemcpyAsync(r.hv.data(), r.win_v, (size_t)S * 8, hipMemcpyDeviceToHost, mainS));
      DFH_HIP(hipMemcpyAsync(r.hi.data(), r.win_i, (size_t)S * 8, hipMemcpyDeviceToHost, mainS));
      DFH_HIP(hipStreamSynchronize(mainS));
      for (int32_t si = 0; si < S; ++si) r.winS[si].merge(r.hv[si], i0 + (int64_t)r.hi[si]);
    }
    if (r.samples_dev)
      DFH_HIP(hipMemcpy2DAsync(r.samples_dev + i0, (size_t)m * 8, r.sampS, (size_t)mc * 8, (size_t)mc * 8, (size_t)S,
                               hipMemcpyDeviceToDevice, mainS));
    if (r.samples_out) {
      const bool out_dev = is_device_ptr(r.samples_out);
      DFH_HIP(hipMemcpy2DAsync(r.samples_out + i0, (size_t)m * 8, r.sampS, (size_t)mc * 8, (size_t)mc * 8, (size_t)S,
                               out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, mainS));
      if (!out_dev) DFH_HIP(hipStreamSynchronize(mainS));
    }
  } else {
    if (want_best) DFH_TRY(r.win.update(ctx, r.samp, mc, i0));
    if (r.samples_dev) DFH_HIP(hipMemcpyAsync(r.samples_dev + i0, r.samp, (size_t)mc * 8, hipMemcpyDeviceToDevice, mainS));
    if (r.samples_out) DFH_TRY(from_device(ctx, r.samples_out + i0, r.samp, (size_t)mc * 8));
  }
  return DFH_OK;
}

// Two-stage software pipeline over chunks.  Stage 1 (low-priority `bulk` stream): cross kernel
// matrix, mu, and the posterior TRSM of chunk c+1 -- large MFMA GEMMs.  Stage 2 (main + panel
// streams): per TS block of chunk c the covariance SYRK, its stable_cholesky (latency-bound
// look-ahead factorisation, host-synchronous because of the jitter ladder) and the draw.
// The factorisations hide behind the next chunk's TRSM instead of idling the GPU.
int ts_run(TsRun& r) {
  dfh_ctx* ctx = r.ctx;
  DFH_TRY(ts_setup(r));
  const int32_t S = r.S;
  DFH_TRY(ts_stage1(r, 0));
  for (int64_t c = 0; c < r.nchunks; ++c) {
    r.p = (int)(c & 1);
    r.i0 = c * r.mc_max;
    r.mc = std::min(r.mc_max, r.m - r.i0);
    if (c + 1 < r.nchunks) DFH_TRY(ts_stage1(r, c + 1));        // enqueue ahead: overlaps with the blocks below
    DFH_HIP(hipStreamWaitEvent(r.mainS, r.ev_ready[r.p], 0));
    if (r.u_dev) r.u_c = r.U + r.i0 * S;
    else DFH_TRY(to_device(ctx, r.U + r.i0 * S, (size_t)r.mc * S * 8, SCR_STAGE_C, &r.u_c));
    if (S > 1) DFH_TRY(transpose_matrix(ctx, r.u_c, S, r.Ut, r.ldu, r.mc, S));
    const double* mv_c = nullptr;
    DFH_TRY(r.stage.mean(r.i0, r.mc, &mv_c));
    r.mu_raw = r.st[r.p].mu;
    r.samp = r.vec[r.p] + r.mc_max;
    // mean_vals = test_mean + K_tetr alpha
    DFH_TRY(add_vec(ctx, r.mu_raw, mv_c, mv_c ? 0.0 : r.mean_const, r.mc));
    DFH_TRY(ts_factor_chunk(r));
    DFH_TRY(ts_collect(r));
    DFH_HIP(hipEventRecord(r.ev_free[r.p], r.mainS));
  }
  DFH_HIP(hipStreamSynchronize(r.mainS));
  DFH_HIP(hipStreamSynchronize(r.bulkS));
  if (S > 1) {
    for (int32_t si = 0; si < S; ++si) r.winS[si].store(r.best_val ? r.best_val + si : nullptr, r.best_idx ? r.best_idx + si : nullptr);
    return DFH_OK;
  }
  r.win.store(r.best_val, r.best_idx);
  return DFH_OK;
}

}  // namespace

extern "C" int dfh_gp_ts(dfh_gp* gp, const double* Xs, int64_t m, int64_t block, const double* U,
                         double mean_const, const double* mean_vals, double* samples_out, double* best_val,
                         int64_t* best_idx, int32_t* jitter_powers_out) {
  DFH_ARG(gp && Xs && U && m >= 1 && block >= 1);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  HallucScope hs;          // no points in progress
  DFH_TRY(halluc_resolve(gp, nullptr, 0, &hs));
  // (the arg-max always ran here, whatever the caller asked for: keep its synchronisation points)
  double bv = 0.0; int64_t bi = -1;
  TsRun r(hs);
  r.Xs = Xs; r.m = m; r.block = block; r.U = U;
  r.mean_const = mean_const; r.mean_vals = mean_vals;
  r.samples_out = samples_out;
  r.best_val = &bv; r.best_idx = &bi;
  r.jitter_powers_out = jitter_powers_out;
  DFH_TRY(ts_run(r));
  if (best_val) *best_val = bv;
  if (best_idx) *best_idx = bi;
  return DFH_OK;
}

// The joint draw of one GP with points in progress and S samples (include/dfhip.h): gp.draw_samples(S, Xs) and
// gp.draw_samples_with_hallucinated_observations(S, Xs, Xh) (gp_core.py:250-261) block by block.  One covariance and one
// stable_cholesky per block, shared by the S draws.
extern "C" int dfh_gp_draw(dfh_gp* gp, const double* Xs, int64_t m, int64_t block, const double* Xh, int64_t q,
                           const double* U, int32_t S, double mean_const, const double* mean_vals, double* samples_out,
                           double* best_vals, int64_t* best_idx, int32_t* jitter_powers_out) {
  DFH_ARG(gp && Xs && U && m >= 1 && block >= 1);
  DFH_ARG(S >= 1 && q >= 0 && (q == 0 || Xh));
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  DFH_HIP(hipSetDevice(gp->ctx->device));
  // the augmentation: block form, or the augmented GP factored from scratch with the ladder
  HallucScope hs;
  DFH_TRY(halluc_resolve(gp, Xh, q, &hs));
  TsRun r(hs);
  r.Xs = Xs; r.m = m; r.block = block; r.U = U; r.S = S;
  r.mean_const = mean_const; r.mean_vals = mean_vals;
  r.samples_out = samples_out;
  r.best_val = best_vals; r.best_idx = best_idx;
  r.jitter_powers_out = jitter_powers_out;
  return ts_run(r);
}

// ---- multi-objective acquisitions: K fitted GPs, one call -------------------------------------------------------
extern "C" int dfh_mo_ucb_argmax(dfh_gp* const* gps, int32_t k, int scal, double beta, const double* weights,
                                 const double* refs, const double* Xs, int64_t m, const double* mean_consts,
                                 const double* mean_vals, double* vals_out, double* best_val, int64_t* best_idx) {
  MoParams par;
  DFH_TRY(mo_check(gps, k, scal, weights, refs, &par));
  DFH_ARG(Xs && m >= 1 && (mean_consts || mean_vals));
  dfh_ctx* ctx = gps[0]->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t d = gps[0]->d;
  int64_t n_max = 0;
  for (int i = 0; i < k; ++i) n_max = std::max(n_max, gps[i]->n);
  const int64_t mc_max = mo_pick_chunk(ctx, n_max, m);
  // the candidates (and per-candidate prior means) go to HBM once, not once per objective
  DevBlock stage(ctx);
  const bool xs_dev = is_device_ptr(Xs), mv_dev = mean_vals ? is_device_ptr(mean_vals) : true;
  const size_t b_xs = xs_dev ? 0 : (size_t)m * d * 8, b_mv = mv_dev ? 0 : (size_t)k * m * 8;
  if (b_xs + b_mv) {
    DFH_TRY(dev_alloc(ctx, b_xs + b_mv, &stage.p));
    char* sp = static_cast<char*>(stage.p);
    if (b_xs) { DFH_HIP(hipMemcpyAsync(sp, Xs, b_xs, hipMemcpyHostToDevice, ctx->stream)); Xs = reinterpret_cast<const double*>(sp); }
    if (b_mv) { DFH_HIP(hipMemcpyAsync(sp + b_xs, mean_vals, b_mv, hipMemcpyHostToDevice, ctx->stream)); mean_vals = reinterpret_cast<const double*>(sp + b_xs); }
    DFH_HIP(hipStreamSynchronize(ctx->stream));      // pageable sources: staged before the caller's buffers may change
  }
  double* vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * (4 + 2 * (size_t)k), (void**)&vec));
  double* mu_raw = vec; double* ss = vec + mc_max; double* kss_w = vec + 2 * mc_max; double* val_c = vec + 3 * mc_max;
  double* MU = vec + 4 * mc_max; double* SD = MU + (int64_t)k * mc_max;       // [k][mc_max] each
  Winner best;
  for (int64_t i0 = 0; i0 < m; i0 += mc_max) {
    const int64_t mc = std::min(mc_max, m - i0);
    const unsigned grid = (unsigned)((mc + 255) / 256);
    for (int i = 0; i < k; ++i) {
      dfh_gp* gp = gps[i];
      ChunkOut co;
      // gp.eval(x, 'std'), :85 / :102 -- each objective packs the shared candidates with its own bandwidths
      DFH_TRY(posterior_chunk(gp, Xs + i0 * d, mc, d, ChunkReq(), mu_raw, ss, nullptr, &co));
      double* kss = gp->kd.stationary ? nullptr : kss_w;
      if (kss) DFH_TRY(prior_diag(ctx, gp->kd, co.Xsp, co.Nsp, mc, kss));
      SectionTimer t(ctx, DFH_T_ACQ);
      AcqArgs a;                 // the mean and the standard deviation of objective i
      a.kxx = gp->kd.kxx; a.kss = kss;
      a.mean_const = mean_consts ? mean_consts[i] : 0.0;
      a.mean_vals = mean_vals ? mean_vals + (int64_t)i * m + i0 : nullptr;
      a.mu_raw = mu_raw; a.ss = ss; a.m = mc;
      a.mu_out = MU + (int64_t)i * mc_max; a.sd_out = SD + (int64_t)i * mc_max;
      DFH_TRY(posterior_acq(ctx, a));
    }
    SectionTimer t(ctx, DFH_T_ACQ);
    hipLaunchKernelGGL(k_mo_scalarise, dim3(grid), dim3(256), 0, ctx->stream, scal, 1, (int)k, beta, par, (const double*)MU,
                       (const double*)SD, (long)mc_max, (long)mc, val_c);
    DFH_LAUNCH_CHECK();
    if (best_val || best_idx) DFH_TRY(best.update(ctx, val_c, mc, i0));
    if (vals_out) DFH_TRY(from_device(ctx, vals_out + i0, val_c, (size_t)mc * 8));
  }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  best.store(best_val, best_idx);
  return DFH_OK;
}

extern "C" int dfh_mo_ts_argmax(dfh_gp* const* gps, int32_t k, int scal, const double* weights, const double* refs,
                                const double* Xs, int64_t m, int64_t block, const double* Xh, int64_t q, const double* U,
                                const double* mean_consts, const double* mean_vals, double* vals_out, double* best_val,
                                int64_t* best_idx, int32_t* jitter_powers_out) {
  MoParams par;
  DFH_TRY(mo_check(gps, k, scal, weights, refs, &par));
  DFH_ARG(Xs && U && m >= 1 && block >= 1 && q >= 0 && (q == 0 || Xh) && (mean_consts || mean_vals));
  dfh_ctx* ctx = gps[0]->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t d = gps[0]->d;
  if (block > m) block = m;
  const int64_t nblk = (m + block - 1) / block;
  // candidates (if they come from the host) | the K draws, objective-major | the scalarised values.  Memory of this
  // call's own, not scratch: the hallucination's fall-back re-fits a GP between two objectives.
  DevBlock hold(ctx);
  const bool xs_dev = is_device_ptr(Xs);
  const size_t b_xs = xs_dev ? 0 : (size_t)m * d * 8;
  DFH_TRY(dev_alloc(ctx, b_xs + (size_t)(k + 1) * m * 8, &hold.p));
  char* hp = static_cast<char*>(hold.p);
  if (b_xs) { DFH_HIP(hipMemcpyAsync(hp, Xs, b_xs, hipMemcpyHostToDevice, ctx->stream)); Xs = reinterpret_cast<const double*>(hp); DFH_HIP(hipStreamSynchronize(ctx->stream)); }
  double* S = reinterpret_cast<double*>(hp + b_xs);
  double* vals = S + (int64_t)k * m;
  for (int i = 0; i < k; ++i) {
    dfh_gp* gp = gps[i];
    // get_gp_sampler_for_parallel_strategy (:29, :54): the draw of the GP augmented with the points in progress
    // (gp_core.py:256-261) -- block form, or the augmented GP factored from scratch where that is not positive definite
    HallucScope hs;
    DFH_TRY(halluc_resolve(gp, Xh, q, &hs));
    TsRun r(hs);
    r.Xs = Xs; r.m = m; r.block = block;
    r.U = U + (int64_t)i * m;
    r.mean_const = mean_consts ? mean_consts[i] : 0.0;
    r.mean_vals = mean_vals ? mean_vals + (int64_t)i * m : nullptr;
    r.samples_dev = S + (int64_t)i * m;
    r.jitter_powers_out = jitter_powers_out ? jitter_powers_out + (int64_t)i * nblk : nullptr;
    DFH_TRY(ts_run(r));
  }
  SectionTimer t(ctx, DFH_T_ACQ);
  hipLaunchKernelGGL(k_mo_scalarise, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, scal, 0, (int)k, 0.0, par,
                     (const double*)S, (const double*)nullptr, (long)m, (long)m, vals);
  DFH_LAUNCH_CHECK();
  Winner best;
  if (best_val || best_idx) DFH_TRY(best.update(ctx, vals, m, 0));
  if (vals_out) DFH_TRY(from_device(ctx, vals_out, vals, (size_t)m * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  best.store(best_val, best_idx);
  return DFH_OK;
}

// mo_lin_asy_ts / mo_tch_asy_ts on a Cartesian-product domain (include/dfhip.h): per objective the chunked posterior of
// dfh_gp_ts_pointwise, its points in progress included, leaves mean and unclipped standard deviation; one launch of
// k_mo_ts_pointwise then draws, scalarises and takes the first arg-max stage for all m candidates.
extern "C" int dfh_mo_ts_pointwise(dfh_gp* const* gps, int32_t k, int scal, const double* weights, const double* refs,
                                   const double* Xs, int64_t m, const double* Xh, int64_t q, const double* U,
                                   const double* mean_consts, const double* mean_vals, double* samples_out,
                                   double* vals_out, double* best_val, int64_t* best_idx) {
  MoParams par;
  DFH_TRY(mo_check(gps, k, scal, weights, refs, &par));
  DFH_ARG(Xs && U && m >= 1 && q >= 0 && (q == 0 || Xh) && (mean_consts || mean_vals));
  dfh_ctx* ctx = gps[0]->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t d = gps[0]->d;
  // candidates and normals (where they come from the host) | the K means | the K standard deviations | the K draws
  // (where wanted) | the scalarised values.  Memory of this call's own, not scratch: the hallucination's fall-back
  // re-fits a GP between two objectives.
  DevBlock hold(ctx);
  const size_t b_xs = is_device_ptr(Xs) ? 0 : (size_t)m * d * 8, b_u = is_device_ptr(U) ? 0 : (size_t)m * k * 8;
  const size_t rows = 2 * (size_t)k + (samples_out ? (size_t)k : 0) + 1;
  DFH_TRY(dev_alloc(ctx, b_xs + b_u + rows * m * 8, &hold.p));
  char* hp = static_cast<char*>(hold.p);
  if (b_xs) { DFH_HIP(hipMemcpyAsync(hp, Xs, b_xs, hipMemcpyHostToDevice, ctx->stream)); Xs = reinterpret_cast<const double*>(hp); }
  if (b_u) { DFH_HIP(hipMemcpyAsync(hp + b_xs, U, b_u, hipMemcpyHostToDevice, ctx->stream)); U = reinterpret_cast<const double*>(hp + b_xs); }
  if (b_xs + b_u) DFH_HIP(hipStreamSynchronize(ctx->stream));      // pageable sources: staged before the caller's buffers may change
  double* MU = reinterpret_cast<double*>(hp + b_xs + b_u);
  double* SD = MU + (int64_t)k * m;
  double* S = samples_out ? SD + (int64_t)k * m : nullptr;
  double* vals = SD + (int64_t)k * m * (samples_out ? 2 : 1);
  for (int j = 0; j < k; ++j) {
    // get_gp_sampler_for_parallel_strategy (:29, :54) per point: the posterior of the GP augmented with the points in
    // progress, the mean from the real data (gp_core.py:256-261)
    EvalReq rq;
    rq.Xs = Xs; rq.m = m; rq.ldxs = d; rq.kxx = gps[j]->kd.kxx;
    rq.Xh = Xh; rq.q = q;
    rq.mean_const = mean_consts ? mean_consts[j] : 0.0;
    rq.mean_vals = mean_vals ? mean_vals + (int64_t)j * m : nullptr;
    rq.mu_out = MU + (int64_t)j * m; rq.sd_out = SD + (int64_t)j * m;
    DFH_TRY(gp_eval_driver(gps[j], rq));
  }
  double hv = 0.0; int64_t hi = -1; int hbad = 0;
  {
    SectionTimer t(ctx, DFH_T_ACQ);
    ArgmaxParts p;
    const int nparts = (int)((m + 255) / 256);
    DFH_TRY(argmax_parts(ctx, nparts, &p));
    DFH_HIP(hipMemsetAsync(p.flag, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_mo_ts_pointwise, dim3((unsigned)nparts), dim3(256), 0, ctx->stream, scal, (int)k, par, (const double*)MU,
                       (const double*)SD, (long)m, U, (long)m, S, vals, p.pv, p.pi, p.flag);
    DFH_LAUNCH_CHECK();
    DFH_TRY(argmax_finish(ctx, p, nparts, &hv, &hi, &hbad));      // winner and flag in one synchronisation
  }
  if (hbad) return pointwise_variance_error();
  if (samples_out) DFH_TRY(from_device(ctx, samples_out, S, (size_t)k * m * 8));
  if (vals_out) DFH_TRY(from_device(ctx, vals_out, vals, (size_t)m * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  if (best_val) *best_val = hv;
  if (best_idx) *best_idx = hi;
  return DFH_OK;
}
