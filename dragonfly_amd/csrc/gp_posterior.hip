// The chunked posterior of a fitted GP and the acquisitions on it: predict, acquisition arg-max, point-wise Thompson
// sampling, covariance, with the points in progress hallucinated (include/dfhip.h).  The arg-max reductions are in
// gp_argmax.hip, the algebra of the points in progress in gp_halluc.hip, the add-UCB stack in gp_adducb.hip.
#include "gp.h"
#include "argmax.h"
#include <algorithm>

bool free_plus_own_scratch(dfh_ctx* ctx, size_t* bytes) {
  size_t f = 0, t = 0;
  if (hipMemGetInfo(&f, &t) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  size_t own = 0;
  for (const DevBuf& b : ctx->scratch) own += b.bytes;
  *bytes = f + own;
  return true;
}

int64_t pick_chunk(dfh_ctx* ctx, int64_t n, int64_t m) {
  // candidate rows per posterior chunk: the m_c x n cross matrix (solved in place into V^T) is sized
  // for a 288 GB part -- DFH_CHUNK_GIB (32) GiB, two of them alive in the pipelined Thompson
  // sampling.  Measured on the bench step (n = 16384, 262144 candidates, TS blocks factored in
  // lock-step batches of DFH_TS_BATCH): 4 GiB / 8 blocks 1434 ms, 8 GiB / 16 1403-1412, 16 GiB / 32
  // 1397, 32 GiB / 64 1389 -- bigger chunks mean taller TRSM products (1048 -> 1021 ms) and more
  // Thompson blocks per latency-bound factorisation chain (332 -> 310 ms).
  // The cap is per CONTEXT (its device, and whoever else is on it): an eighth of what was free on the
  // context's device when the context first asked, plus what the context's own scratch pool already
  // held then -- not an eighth of the first device's total memory for the whole process.
  static const double chunk_env = env_double("DFH_CHUNK_GIB", 32.0), chunk_gib = chunk_env > 0.0 ? chunk_env : 32.0;
  if (ctx->chunk_cap_gib <= 0.0) {
    size_t avail = 0;
    double cap = 36.0;
    if (free_plus_own_scratch(ctx, &avail)) cap = (double)avail / 8.0 / 1073741824.0;
    ctx->chunk_cap_gib = cap > 0.25 ? cap : 0.25;
  }
  const double gib = chunk_gib < ctx->chunk_cap_gib ? chunk_gib : ctx->chunk_cap_gib;
  int64_t mc = (int64_t)(gib * (double)(1LL << 27)) / (n > 0 ? n : 1);
  mc = std::max<int64_t>(512, std::min<int64_t>(mc, 262144));
  mc = (mc / 512) * 512;
  if (mc > m) mc = m;
  return mc;
}

namespace {

// Phi(x): scipy.special.ndtr structure (xsf/cephes/ndtr.h) on the device erf/erfc
__device__ __forceinline__ double ndtr_dev(double a) {
  if (a != a) return a;
  const double x = a * 0.70710678118654752440;   // M_SQRT1_2
  const double z = fabs(x);
  double y;
  if (z < 1.0) {
    y = 0.5 + 0.5 * erf(x);
  } else {
    y = 0.5 * erfc(z);
    if (x > 0) y = 1.0 - y;
  }
  return y;
}
__device__ __forceinline__ double norm_pdf_dev(double x) {
  return exp(-(x * x) / 2.0) / 2.5066282746310002;   // scipy _norm_pdf: exp(-x**2/2.0)/sqrt(2*pi)
}
__device__ __forceinline__ double ei_norm_diff(double nd) {
  const double v = nd * ndtr_dev(nd) + norm_pdf_dev(nd);       // gpb_acquisitions.py:247-249
  // z Phi + phi > 0 for every z.  Below z = -38 both terms are subnormal and their rounding can leave -2^-1074, where the
  // reference (whose Phi has flushed to 0 there) returns phi >= 0: such a value is 0.  NaN stays NaN.
  return v < 0.0 ? 0.0 : v;
}

// mu/sd/acquisition for one chunk.
//   mu_raw = K(Xs,X) alpha ; ss = ||L^-1 k||^2 ; ss2 = extra hallucination term (or null)
//   kss = prior variances k(x_i, x_i) of a kernel that is not stationary (else null: kxx)
__global__ void k_posterior_acq(int acq, double p0, double p1, double kxx, const double* __restrict__ kss,
                                double mean_const, const double* __restrict__ mean_vals, const double* __restrict__ mu_raw,
                                const double* __restrict__ ss, const double* __restrict__ ss2, long m,
                                double* __restrict__ mu_out, double* __restrict__ sd_out,
                                double* __restrict__ val_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double mu = (mean_vals ? mean_vals[i] : mean_const) + mu_raw[i];   // gp_core.py:173-175
  double sd = 0.0;
  if (ss) {
    if (kss) kxx = kss[i];
    double var = kxx - ss[i];                               // diag(K_tete - V^T V), gp_core.py:181
    if (ss2) var = kxx - (ss[i] + ss2[i]);
    sd = sqrt(var);                                         // gp_core.py:187 (NaN if var < 0)
  }
  if (mu_out) mu_out[i] = mu;
  if (sd_out) sd_out[i] = sd;
  if (!val_out) return;
  double v;
  switch (acq) {
    case DFH_ACQ_MEAN: v = mu; break;
    case DFH_ACQ_STD: v = sd; break;
    case DFH_ACQ_UCB: v = mu + p0 * sd; break;              // gpb_acquisitions.py:222
    case DFH_ACQ_EI: {                                      // :256-260
      const double nd = (mu - p0) / sd;
      v = sd * ei_norm_diff(nd);
      break;
    }
    case DFH_ACQ_PI: v = ndtr_dev((mu - p0) / sd); break;   // :238
    case DFH_ACQ_TTEI: {                                    // :275-279
      const double comb = sqrt(p1 * p1 + sd * sd);
      const double nd = (mu - p0) / comb;
      v = comb * ei_norm_diff(nd);
      break;
    }
    default: v = mu;
  }
  val_out[i] = v;
}

// Epilogue of one chunk of the point-wise Thompson sampling (dfh_gp_ts_pointwise): per candidate the one-point draw
// s = sqrt(var) u + mu -- draw_gaussian_samples on a 1 x 1 covariance (general_utils.py:224-232: L.dot(U).T + mu, the
// product and the sum rounded apart; the build has no implicit fusion) -- with var the unclipped posterior variance
// of k_posterior_acq, and the first stage of the arg-max: one partial winner per workgroup (one element per thread;
// argmax_finish does the rest).  *bad is set when some var is not > 0, where the 1 x 1 stable_cholesky fails on every
// rung of its ladder.
__global__ __launch_bounds__(256) void k_ts_pointwise(
    double kxx, const double* __restrict__ kss, double mean_const, const double* __restrict__ mean_vals,
    const double* __restrict__ mu_raw, const double* __restrict__ ss, const double* __restrict__ ss2, const double* __restrict__ u,
    long m, long idx_base, double* __restrict__ samp, double* __restrict__ pv, long* __restrict__ pi, int* __restrict__ bad) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double bv = -INFINITY; long bi = ARGMAX_NONE;
  int not_pd = 0;
  if (i < m) {
    const double mu = (mean_vals ? mean_vals[i] : mean_const) + mu_raw[i];   // gp_core.py:173-175
    if (kss) kxx = kss[i];
    const double var = ss2 ? kxx - (ss[i] + ss2[i]) : kxx - ss[i];           // gp_core.py:181 / :211, one point
    not_pd = !(var > 0.0);                                                   // (NaN included)
    bv = sqrt(var) * u[i] + mu;
    bi = idx_base + i;
    samp[i] = bv;
  }
  not_pd = __syncthreads_or(not_pd);
  block_argmax(bv, bi);
  if (threadIdx.x == 0) {
    pv[blockIdx.x] = bv; pi[blockIdx.x] = bi;
    if (not_pd) atomicOr(bad, 1);
  }
}

}  // namespace

// A one-point draw whose variance is not positive: the exhausted ladder of the reference's 1 x 1 stable_cholesky
int pointwise_variance_error() {
  dfh_set_error("Could not compute Cholesky decomposition of a candidate's 1 x 1 posterior covariance: the variance is "
                "not positive. This is likely because the M is not positive semi-definite or has infinities/nans.");
  return DFH_ERR_JITTER;
}

int posterior_acq(dfh_ctx* ctx, const AcqArgs& a) {
  hipLaunchKernelGGL(k_posterior_acq, dim3((unsigned)((a.m + 255) / 256)), dim3(256), 0, ctx->stream, a.acq, a.p0, a.p1, a.kxx,
                     a.kss, a.mean_const, a.mean_vals, a.mu_raw, a.ss, a.ss2, (long)a.m, a.mu_out, a.sd_out, a.val_out);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

int posterior_chunk(dfh_gp* gp, const double* Xs_dev, int64_t mc, int64_t ldxs, const ChunkReq& rq, double* mu_raw,
                    double* ss, double* ss2, ChunkOut* out) {
  dfh_ctx* ctx = gp->ctx;
  const KernDev& kd = gp->kd;
  const int part_hi = rq.part_hi < 0 ? kd.n_parts : rq.part_hi;
  ChunkOut o;
  char* xs = nullptr;
  const PackedXs lay = packed_xs_layout(kd, mc);
  DFH_TRY(scratch_get(ctx, rq.parity ? SCR_XS2 : SCR_XS, lay.bytes, (void**)&xs));
  o.Xsp = reinterpret_cast<double*>(xs);
  o.Nsp = reinterpret_cast<double*>(xs + lay.nsp_off);
  DFH_TRY(scratch_get(ctx, rq.parity ? SCR_KCT2 : SCR_KCT, (size_t)mc * gp->n * 8, (void**)&o.Kct));
  {
    SectionTimer t(ctx, DFH_T_CROSS);
    DFH_TRY(pack_scaled(ctx, kd, rq.part_lo, part_hi, rq.pre_gathered, Xs_dev, mc, ldxs, o.Xsp, o.Nsp));
    KmMean mean{gp->alpha, mu_raw, false};      // gp_core.py:174, from the same pass where the kernel can
    DFH_TRY(kernmat_cross(ctx, kd, rq.part_lo, part_hi, true, KmPts{o.Xsp, o.Nsp, mc}, KmPts{gp->Xp, gp->Np, gp->n}, o.Kct, gp->n,
                          &mean, rq.col_w));
    if (!mean.done) DFH_TRY(gemv_rows(ctx, o.Kct, mc, gp->n, gp->n, gp->alpha, 1.0, nullptr, 0.0, mu_raw));
  }
  if (rq.want_var) {
    {
      SectionTimer t(ctx, DFH_T_TRSM);
      DFH_TRY(trsm_rows(ctx, gp->L, gp->n, gp->n, gp->inv, o.Kct, mc, gp->n, gp->refine.data()));                // gp_core.py:180
    }
    SectionTimer t(ctx, DFH_T_ACQ);
    if (ss) DFH_TRY(row_sumsq(ctx, o.Kct, mc, gp->n, gp->n, ss));
    if (rq.h && rq.h->q > 0)
      DFH_TRY(halluc_second_row(gp, *rq.h, o.Xsp, o.Nsp, o.Kct, mc, rq.parity ? SCR_AUG2B : SCR_AUG2, ss2, &o.T));
  }
  if (out) *out = o;
  return DFH_OK;
}

namespace {

// The driver's vectors of one chunk, mc_max doubles each, in one scratch block
struct ChunkVecs {
  int64_t mc_max;
  double *mu_raw, *ss, *ss2;       // K(Xs, X) alpha | ||L^-1 k||^2 | the second block row's share (posterior_chunk)
  double *mu, *sd, *val;           // what the epilogue makes of them: mean, standard deviation, acquisition value or draw
  double *spare, *kss;             // the augmented GP's own mean, unread (halluc_chunk) | k(x, x) of a non-stationary kernel
  static constexpr int slots = 8;
  ChunkVecs(double* vec, int64_t mc_max_)
      : mc_max(mc_max_), mu_raw(vec), ss(vec + mc_max), ss2(vec + 2 * mc_max), mu(vec + 3 * mc_max), sd(vec + 4 * mc_max),
        val(vec + 5 * mc_max), spare(vec + 6 * mc_max), kss(vec + 7 * mc_max) {}
};

// One chunk in the driver: its rows, what was staged for it, its posterior as the epilogues read it (null: it has none)
struct Chunk {
  int64_t i0 = 0, mc = 0;
  const double *xs = nullptr, *mean_vals = nullptr, *u = nullptr, *kss = nullptr, *ss = nullptr, *ss2 = nullptr;
};

// The acquisition's epilogue: mean, standard deviation and value per candidate, the chunk's winner, the copies back
int acq_epilogue(dfh_ctx* ctx, const EvalReq& rq, const ChunkVecs& v, const Chunk& c, Winner* best) {
  const bool want_best = rq.best_val || rq.best_idx;
  {
    SectionTimer t(ctx, DFH_T_ACQ);
    AcqArgs a;
    a.acq = rq.acq; a.p0 = rq.params ? rq.params[0] : 0.0; a.p1 = rq.params ? rq.params[1] : 0.0;
    a.kxx = rq.kxx; a.kss = c.kss; a.mean_const = rq.mean_const; a.mean_vals = c.mean_vals;
    a.mu_raw = v.mu_raw; a.ss = c.ss; a.ss2 = c.ss2; a.m = c.mc;
    a.mu_out = rq.mu_out ? v.mu : nullptr; a.sd_out = rq.sd_out ? v.sd : nullptr;
    a.val_out = (rq.vals_out || want_best) ? v.val : nullptr;
    DFH_TRY(posterior_acq(ctx, a));
    if (want_best) DFH_TRY(best->update(ctx, v.val, c.mc, c.i0));
  }
  if (rq.mu_out) DFH_TRY(from_device(ctx, rq.mu_out + c.i0, v.mu, (size_t)c.mc * 8));
  if (rq.sd_out) DFH_TRY(from_device(ctx, rq.sd_out + c.i0, v.sd, (size_t)c.mc * 8));
  if (rq.vals_out) DFH_TRY(from_device(ctx, rq.vals_out + c.i0, v.val, (size_t)c.mc * 8));
  return DFH_OK;
}

// The epilogue of the point-wise Thompson sampling: the draws and the first stage of their arg-max in one kernel.  One
// synchronisation per chunk: the chunk's winner and its flag come back together.
int ts_epilogue(dfh_ctx* ctx, const EvalReq& rq, const ChunkVecs& v, const Chunk& c, Winner* best) {
  double hv = 0.0; int64_t hi = -1; int hbad = 0;
  {
    SectionTimer t(ctx, DFH_T_ACQ);
    ArgmaxParts p;
    const int nparts = (int)((c.mc + 255) / 256);
    DFH_TRY(argmax_parts(ctx, (int)((v.mc_max + 255) / 256), &p));      // (the pair's slot does not move with the chunk's size)
    DFH_HIP(hipMemsetAsync(p.flag, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_ts_pointwise, dim3((unsigned)nparts), dim3(256), 0, ctx->stream, rq.kxx, c.kss, rq.mean_const,
                       c.mean_vals, (const double*)v.mu_raw, c.ss, c.ss2, c.u, (long)c.mc, (long)c.i0, v.val, p.pv, p.pi, p.flag);
    DFH_LAUNCH_CHECK();
    DFH_TRY(argmax_finish(ctx, p, nparts, &hv, &hi, &hbad));
  }
  if (hbad) return pointwise_variance_error();
  best->merge(hv, hi);
  if (rq.vals_out) DFH_TRY(from_device(ctx, rq.vals_out + c.i0, v.val, (size_t)c.mc * 8));
  return DFH_OK;
}

}  // namespace

// shared driver of predict / acquisition arg-max / point-wise Thompson sampling: per chunk its posterior, then its epilogue
int gp_eval_driver(dfh_gp* gp, const EvalReq& rq) {
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t m = rq.m;
  const bool want_var = rq.want_var;
  HallucScope hs;                           // (hs.aug: the variance comes from the re-factored augmented GP)
  DFH_TRY(halluc_resolve(gp, rq.Xh, want_var ? rq.q : 0, &hs));
  const int64_t mc_max = pick_chunk(gp->ctx, gp->n + (hs.aug ? rq.q : 0), m);
  const ChunkStager stage(ctx, rq.Xs, rq.ldxs, rq.mean_vals);
  double* vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * ChunkVecs::slots, (void**)&vec));
  const ChunkVecs v(vec, mc_max);
  // a kernel with a polynomial / exponential-decay factor: k(x, x) per candidate; on the add-UCB group path
  // (pre_gathered: one group of an additive kernel) the group's own prior variance, if it is such a group
  bool range_stationary = gp->kd.stationary;
  if (rq.pre_gathered) {
    range_stationary = true;
    for (int g = rq.part_lo; g < rq.part_hi; ++g) range_stationary = range_stationary && part_is_stationary(gp->kd, g);
  }
  Winner best;
  ChunkReq creq;
  creq.part_lo = rq.part_lo; creq.part_hi = rq.part_hi; creq.pre_gathered = rq.pre_gathered;
  creq.col_w = rq.col_w; creq.want_var = want_var;
  Chunk c;
  c.kss = (want_var && !range_stationary) ? v.kss : nullptr;
  c.ss = want_var ? v.ss : nullptr;
  c.ss2 = (want_var && hs.block_q() > 0) ? v.ss2 : nullptr;
  for (c.i0 = 0; c.i0 < m; c.i0 += mc_max) {
    c.mc = std::min(mc_max, m - c.i0);
    // the chunk's posterior: what it needs staged, the step with the points in progress, k(x, x)
    DFH_TRY(stage.xs(c.i0, c.mc, SCR_STAGE_A, &c.xs));
    DFH_TRY(stage.mean(c.i0, c.mc, &c.mean_vals));
    if (rq.U) DFH_TRY(to_device(ctx, rq.U + c.i0, (size_t)c.mc * 8, SCR_STAGE_C, &c.u));
    ChunkOut co;
    DFH_TRY(halluc_chunk(hs, c.xs, c.mc, rq.ldxs, creq, v.mu_raw, v.ss, v.ss2, v.spare, &co));
    if (c.kss) DFH_TRY(prior_diag(ctx, hs.cov_gp()->kd, co.Xsp, co.Nsp, c.mc, v.kss, rq.part_lo, rq.part_hi));
    // its epilogue
    DFH_TRY(rq.U ? ts_epilogue(ctx, rq, v, c, &best) : acq_epilogue(ctx, rq, v, c, &best));
  }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  best.store(rq.best_val, rq.best_idx);
  return DFH_OK;
}

extern "C" int dfh_gp_predict(dfh_gp* gp, const double* Xs, int64_t m, const double* Xh, int64_t q,
                              double* mu_out, double* sd_out) {
  DFH_ARG(gp && m >= 0 && q >= 0);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  if (m == 0) return DFH_OK;
  DFH_ARG(Xs && mu_out && (q == 0 || Xh));
  EvalReq rq;
  rq.Xs = Xs; rq.m = m; rq.ldxs = gp->d;
  rq.kxx = gp->kd.kxx;
  rq.Xh = Xh; rq.q = q;
  rq.want_var = sd_out != nullptr;
  rq.mu_out = mu_out; rq.sd_out = sd_out;
  return gp_eval_driver(gp, rq);
}

extern "C" int dfh_gp_acq_argmax(dfh_gp* gp, int acq, const double* params, const double* Xs, int64_t m,
                                 const double* Xh, int64_t q, double mean_const, const double* mean_vals,
                                 double* vals_out, double* best_val, int64_t* best_idx) {
  DFH_ARG(gp && m >= 1 && Xs && q >= 0 && (q == 0 || Xh));
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  DFH_ARG(acq >= DFH_ACQ_MEAN && acq <= DFH_ACQ_STD);
  DFH_ARG(params || acq == DFH_ACQ_MEAN || acq == DFH_ACQ_STD);
  EvalReq rq;
  rq.acq = acq; rq.params = params;
  rq.Xs = Xs; rq.m = m; rq.ldxs = gp->d;
  rq.kxx = gp->kd.kxx;
  rq.Xh = Xh; rq.q = q;
  rq.mean_const = mean_const; rq.mean_vals = mean_vals;
  rq.want_var = acq != DFH_ACQ_MEAN;
  rq.vals_out = vals_out; rq.best_val = best_val; rq.best_idx = best_idx;
  return gp_eval_driver(gp, rq);
}

// Point-wise Thompson sampling (include/dfhip.h): the posterior of dfh_gp_acq_argmax, points in progress included, with
// k_ts_pointwise as the driver's epilogue.
extern "C" int dfh_gp_ts_pointwise(dfh_gp* gp, const double* Xs, int64_t m, const double* Xh, int64_t q, const double* U,
                                   double mean_const, const double* mean_vals, double* samples_out, double* best_val,
                                   int64_t* best_idx) {
  DFH_ARG(gp && Xs && U && m >= 1 && q >= 0 && (q == 0 || Xh));
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  EvalReq rq;
  rq.Xs = Xs; rq.m = m; rq.ldxs = gp->d; rq.kxx = gp->kd.kxx;
  rq.Xh = Xh; rq.q = q; rq.U = U;
  rq.mean_const = mean_const; rq.mean_vals = mean_vals;
  rq.vals_out = samples_out; rq.best_val = best_val; rq.best_idx = best_idx;
  return gp_eval_driver(gp, rq);
}

extern "C" int dfh_gp_predict_covar(dfh_gp* gp, const double* Xs, int64_t m, const double* Xh, int64_t q,
                                    double* mu_out, double* cov_out) {
  DFH_ARG(gp && m >= 0 && q >= 0);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  if (m == 0) return DFH_OK;
  DFH_ARG(Xs && mu_out && cov_out && (q == 0 || Xh));
  DFH_ARG((double)m * (double)gp->n * 8.0 < 64e9);
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const KernDev& kd = gp->kd;
  HallucScope hs;
  DFH_TRY(halluc_resolve(gp, Xh, q, &hs));
  if (hs.aug) {
    // covariance from the augmented GP factored from scratch, mean from the real data
    DFH_TRY(dfh_gp_predict_covar(hs.aug, Xs, m, nullptr, 0, mu_out, cov_out));
    return dfh_gp_predict(gp, Xs, m, nullptr, 0, mu_out, nullptr);
  }
  const double* dXs = nullptr;
  DFH_TRY(to_device(ctx, Xs, (size_t)m * gp->d * 8, SCR_STAGE_A, &dXs));
  double* vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)m * 8 * 3, (void**)&vec));
  ChunkOut co;                              // V^T and the packed Xs
  DFH_TRY(posterior_chunk(gp, dXs, m, gp->d, ChunkReq(), vec, vec + m, vec + 2 * m, &co));
  DFH_TRY(from_device(ctx, mu_out, vec, (size_t)m * 8));
  // cov = K(Xs,Xs) - V^T V     (gp_core.py:179-181)
  const bool dev_out = is_device_ptr(cov_out);
  double* C = cov_out;
  if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)m * m * 8, (void**)&C));
  DFH_TRY(kernmat_gram(ctx, kd, 0, kd.n_parts, true, KmPts{co.Xsp, co.Nsp, m}, 0.0, C, m));
  DFH_TRY(gemm_f64(ctx, 0, m, m, gp->n, -1.0, co.Kct, gp->n, co.Kct, gp->n, 1.0, C, m, C, m));
  if (hs.block_q() > 0) {
    // second block row of the augmented solve: V2t = (k(Xs,Xh) - V1t Wt^T) Lh^-T ; cov -= V2t V2t^T
    DFH_TRY(halluc_second_row(gp, hs.h, co.Xsp, co.Nsp, co.Kct, m, SCR_AUG2, vec + 2 * m, &co.T));
    DFH_TRY(gemm_f64(ctx, 0, m, m, q, -1.0, co.T, q, co.T, q, 1.0, C, m, C, m));
  }
  if (!dev_out) DFH_TRY(from_device(ctx, cov_out, C, (size_t)m * m * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}
