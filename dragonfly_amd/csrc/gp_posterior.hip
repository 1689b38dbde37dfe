// The chunked posterior of a fitted GP and the acquisitions on it: predict, acquisition arg-max, point-wise Thompson
// sampling, add-UCB, covariance, with the points in progress hallucinated (include/dfhip.h).
#include "gp.h"
#include <limits.h>
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

// numpy argmax ordering: a NaN beats everything, earlier index wins ties
__device__ __forceinline__ bool better(double va, long ia, double vb, long ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) {
    if (na && nb) return ia < ib;
    return na;
  }
  if (va > vb) return true;
  if (va < vb) return false;
  return ia < ib;
}

__global__ void k_argmax_stage1(const double* __restrict__ v, long m, long idx_base,
                                double* __restrict__ pv, long* __restrict__ pi) {
  __shared__ double sv[256];
  __shared__ long si[256];
  double bv = -INFINITY;
  long bi = LONG_MAX;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long)gridDim.x * blockDim.x) {
    const double x = v[i];
    if (bi == LONG_MAX || better(x, idx_base + i, bv, bi)) { bv = x; bi = idx_base + i; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { pv[blockIdx.x] = sv[0]; pi[blockIdx.x] = si[0]; }
}

__global__ void k_argmax_stage2(const double* pv, const long* pi, int nparts, double* out_v, long* out_i) {
  __shared__ double sv[256];
  __shared__ long si[256];
  double bv = -INFINITY; long bi = LONG_MAX;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    if (pi[i] != LONG_MAX && (bi == LONG_MAX || better(pv[i], pi[i], bv, bi))) { bv = pv[i]; bi = pi[i]; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out_v[0] = sv[0]; out_i[0] = si[0]; }
}

// One workgroup per segment [off[g], off[g+1]) of v: its arg-max (np.argmax rule, index local to the segment)
__global__ void k_argmax_segments(const double* __restrict__ v, const long* __restrict__ off,
                                  double* __restrict__ out_v, long* __restrict__ out_i) {
  __shared__ double sv[256];
  __shared__ long si[256];
  const long lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
  double bv = -INFINITY;
  long bi = LONG_MAX;
  for (long i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const double x = v[i];
    if (bi == LONG_MAX || better(x, i - lo, bv, bi)) { bv = x; bi = i - lo; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out_v[blockIdx.x] = sv[0]; out_i[blockIdx.x] = si[0]; }
}

bool host_better(double va, int64_t ia, double vb, int64_t ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) { if (na && nb) return ia < ib; return na; }
  if (va > vb) return true;
  if (va < vb) return false;
  return ia < ib;
}

}  // namespace

void Winner::merge(double ov, int64_t oi) {
  if (!have || host_better(ov, oi, v, i)) { v = ov; i = oi; have = true; }
}

// arg-max of vals[0..m) (device), indices offset by idx_base; merges into the running best
int Winner::update(dfh_ctx* ctx, const double* vals, int64_t m, int64_t idx_base) {
  if (m <= 0) return DFH_OK;
  const int nblocks = (int)std::min<int64_t>(1024, (m + 255) / 256);
  char* buf = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_RED, (size_t)(nblocks + 1) * 16 + 64, (void**)&buf));
  double* pv = reinterpret_cast<double*>(buf);
  long* pi = reinterpret_cast<long*>(buf + (size_t)(nblocks + 1) * 8);
  hipLaunchKernelGGL(k_argmax_stage1, dim3(nblocks), dim3(256), 0, ctx->stream, vals, (long)m, (long)idx_base, pv, pi);
  DFH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_argmax_stage2, dim3(1), dim3(256), 0, ctx->stream, pv, pi, nblocks, pv + nblocks, pi + nblocks);
  DFH_LAUNCH_CHECK();
  double hv; long hi;
  DFH_HIP(hipMemcpyAsync(&hv, pv + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipMemcpyAsync(&hi, pi + nblocks, 8, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  merge(hv, (int64_t)hi);
  return DFH_OK;
}

// arg-max of every row of v [rows x ld] (np.argmax rule, index local to the row): one workgroup per row
__global__ void k_argmax_rows(const double* __restrict__ v, long ld, long m, double* __restrict__ out_v,
                              long* __restrict__ out_i) {
  __shared__ double sv[256];
  __shared__ long si[256];
  const double* r = v + (long)blockIdx.x * ld;
  double bv = -INFINITY;
  long bi = LONG_MAX;
  for (long i = threadIdx.x; i < m; i += blockDim.x) {
    const double x = r[i];
    if (bi == LONG_MAX || better(x, i, bv, bi)) { bv = x; bi = i; }
  }
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out_v[blockIdx.x] = sv[0]; out_i[blockIdx.x] = si[0]; }
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

}  // namespace

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

namespace {

// hallucination tail: T[m x q] holds k(x, Xh) - V1 W^T ; solve rows with Lh (q x q lower) and
// return the squared norms.
__global__ void k_halluc_rows(double* __restrict__ T, long m, int q, const double* __restrict__ Lh,
                              double* __restrict__ ss2) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double* t = T + i * q;
  double acc = 0.0;
  for (int c = 0; c < q; ++c) {
    double s = t[c];
    for (int k = 0; k < c; ++k) s = fma(-Lh[c * q + k], t[k], s);
    s = s / Lh[c * q + c];
    t[c] = s;
    acc = fma(s, s, acc);
  }
  ss2[i] = acc;
}

// The reference factors the whole augmented matrix with stable_cholesky (gp_core.py:199-206).  The
// block form below gives the same factor as long as that factorisation needs no jitter; when the
// Schur complement is not positive definite, or the base fit itself needed the ladder (its jitter
// was chosen for the n x n matrix, the reference would re-run the ladder on the (n+q) x (n+q) one),
// DFH_ERR_NOT_PD is returned and the callers fall back to halluc_augmented_gp.
int halluc_prepare(dfh_gp* gp, const double* Xh_user, int64_t q, Halluc* h) {
  dfh_ctx* ctx = gp->ctx;
  h->q = q;
  if (q <= 0) return DFH_OK;
  DFH_ARG(q <= 4096);
  if (gp->diag_jitter != 0.0) return DFH_ERR_NOT_PD;
  if (gp->psd_flags) return DFH_ERR_NOT_PD;      // the reference projects the whole augmented matrix (gp_core.py:199-206)
  const KernDev& kd = gp->kd;
  const double* Xh = nullptr;
  DFH_TRY(to_device(ctx, Xh_user, (size_t)q * gp->d * 8, SCR_STAGE_C, &Xh));
  char* buf = nullptr;
  const size_t b_xhp = (size_t)q * kd.P * 8, b_nhp = (size_t)q * kd.n_parts * 8;
  const size_t b_wt = (size_t)q * gp->n * 8, b_lh = (size_t)q * q * 8;
  DFH_TRY(scratch_get(ctx, SCR_AUG, b_xhp + b_nhp + b_wt + b_lh + 1024, (void**)&buf));
  h->Xhp = reinterpret_cast<double*>(buf);
  h->Nhp = reinterpret_cast<double*>(buf + ((b_xhp + 255) / 256) * 256);
  h->Wt = reinterpret_cast<double*>(reinterpret_cast<char*>(h->Nhp) + ((b_nhp + 255) / 256) * 256);
  h->Lh = reinterpret_cast<double*>(reinterpret_cast<char*>(h->Wt) + ((b_wt + 255) / 256) * 256);
  DFH_TRY(pack_scaled(ctx, kd, 0, kd.n_parts, false, Xh, q, gp->d, h->Xhp, h->Nhp));
  // Wt = K(Xh, X) L^-T
  DFH_TRY(kernmat_cross(ctx, kd, 0, kd.n_parts, true, KmPts{h->Xhp, h->Nhp, q}, KmPts{gp->Xp, gp->Np, gp->n}, h->Wt, gp->n));
  DFH_TRY(trsm_rows(ctx, gp->L, gp->n, gp->n, gp->inv, h->Wt, q, gp->n, gp->refine.data()));
  // S = K(Xh,Xh) + (noise + jitter) I - Wt Wt^T ; Lh = chol(S)
  const std::function<int()> build_S = [&]() -> int {
    DFH_TRY(kernmat_gram(ctx, kd, 0, kd.n_parts, true, KmPts{h->Xhp, h->Nhp, q}, gp->noise_var, h->Lh, q));
    return gemm_f64(ctx, 0, q, q, gp->n, -1.0, h->Wt, gp->n, h->Wt, gp->n, 1.0, h->Lh, q, h->Lh, q);
  };
  DFH_TRY(build_S());
  int64_t piv = 0;
  int rc = cholesky_device(ctx, h->Lh, q, q, nullptr, &piv, 1, 0, 0, nullptr, false, &build_S);
  if (rc == DFH_ERR_NOT_PD)
    dfh_set_error("augmented (hallucinated) kernel matrix is not positive definite at pivot %lld",
                  (long long)(gp->n + piv));
  return rc;
}

// Second block row of the augmented solve for `rows` candidates whose first block row Kct (V1^T) is solved:
// T = k(Xs, Xh) - V1t Wt^T in scratch `slot`, its rows solved against Lh in place (V2^T), their squared norms in ss2.
int halluc_second_row(dfh_gp* gp, const Halluc& h, const double* Xsp, const double* Nsp, const double* Kct, int64_t rows,
                      int slot, double* ss2, double** T_out) {
  dfh_ctx* ctx = gp->ctx;
  const KernDev& kd = gp->kd;
  const int64_t q = h.q;
  double* T = nullptr;
  DFH_TRY(scratch_get(ctx, slot, (size_t)rows * q * 8, (void**)&T));
  // T = k(Xs, Xh) - V1t Wt^T
  DFH_TRY(kernmat_cross(ctx, kd, 0, kd.n_parts, true, KmPts{Xsp, Nsp, rows}, KmPts{h.Xhp, h.Nhp, q}, T, q));
  DFH_TRY(gemm_f64(ctx, 0, rows, q, gp->n, -1.0, Kct, gp->n, h.Wt, gp->n, 1.0, T, q, T, q));
  hipLaunchKernelGGL(k_halluc_rows, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, T, (long)rows, (int)q, h.Lh, ss2);
  DFH_LAUNCH_CHECK();
  *T_out = T;        // V2^T: the rows solved against Lh
  return DFH_OK;
}

// Fallback of the hallucinated posterior: the GP over (X, Xh) factored from scratch with the
// stable_cholesky ladder -- literally gp_core.py:196-206; only its variance is used (the labels
// are irrelevant: zeros).  The caller frees *aug.
int halluc_augmented_gp(dfh_gp* gp, const double* Xh, int64_t q, dfh_gp** aug) {
  std::vector<double> y0((size_t)(gp->n + q), 0.0);
  return dfh_gp_append(gp, Xh, q, y0.data(), 0, aug, nullptr, nullptr);
}

}  // namespace

int halluc_resolve(dfh_gp* gp, const double* Xh, int64_t q, HallucScope* s) {
  s->gp = gp;
  if (q <= 0) return DFH_OK;
  int rc = halluc_prepare(gp, Xh, q, &s->h);
  if (rc == DFH_ERR_NOT_PD) {
    s->h.q = 0;
    rc = halluc_augmented_gp(gp, Xh, q, &s->aug);
  }
  return rc;
}

// One chunk of candidates (device pointer Xs_dev, mc rows): fills mu_raw, ss (and, with rq.h, ss2).
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

// shared driver for predict / acquisition arg-max
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
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * 8, (void**)&vec));
  // a kernel with a polynomial / exponential-decay factor: k(x, x) per candidate; on the add-UCB group path
  // (pre_gathered: one group of an additive kernel) the group's own prior variance, if it is such a group
  bool range_stationary = gp->kd.stationary;
  if (rq.pre_gathered) {
    range_stationary = true;
    for (int g = rq.part_lo; g < rq.part_hi; ++g) range_stationary = range_stationary && part_is_stationary(gp->kd, g);
  }
  double* kss = (want_var && !range_stationary) ? vec + 7 * mc_max : nullptr;
  double* mu_raw = vec; double* ss = vec + mc_max; double* ss2 = vec + 2 * mc_max;
  double* mu_c = vec + 3 * mc_max; double* sd_c = vec + 4 * mc_max; double* val_c = vec + 5 * mc_max;
  const bool want_best = rq.best_val || rq.best_idx;
  Winner best;
  const double p0 = rq.params ? rq.params[0] : 0.0, p1 = rq.params ? rq.params[1] : 0.0;
  ChunkReq creq;
  creq.part_lo = rq.part_lo; creq.part_hi = rq.part_hi; creq.pre_gathered = rq.pre_gathered;
  creq.col_w = rq.col_w;
  for (int64_t i0 = 0; i0 < m; i0 += mc_max) {
    const int64_t mc = std::min(mc_max, m - i0);
    const double* xs_c = nullptr;
    DFH_TRY(stage.xs(i0, mc, SCR_STAGE_A, &xs_c));
    const double* mv_c = nullptr;
    DFH_TRY(stage.mean(i0, mc, &mv_c));
    ChunkOut co;
    if (hs.aug) {
      // mean from the real data, variance from the augmented factor (gp_core.py:195, 207-213)
      creq.want_var = true; creq.h = nullptr;
      DFH_TRY(posterior_chunk(hs.aug, xs_c, mc, rq.ldxs, creq, vec + 6 * mc_max, ss, ss2));
      creq.want_var = false;
      DFH_TRY(posterior_chunk(gp, xs_c, mc, rq.ldxs, creq, mu_raw, nullptr, nullptr, &co));
    } else {
      creq.want_var = want_var; creq.h = &hs.h;
      DFH_TRY(posterior_chunk(gp, xs_c, mc, rq.ldxs, creq, mu_raw, ss, ss2, &co));
    }
    if (kss) DFH_TRY(prior_diag(ctx, gp->kd, co.Xsp, co.Nsp, mc, kss, rq.part_lo, rq.part_hi));
    {
      SectionTimer t(ctx, DFH_T_ACQ);
      const bool need_val = rq.vals_out || want_best;
      hipLaunchKernelGGL(k_posterior_acq, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, ctx->stream, rq.acq, p0, p1,
                         rq.kxx, kss, rq.mean_const, mv_c, mu_raw, want_var ? ss : nullptr,
                         (want_var && hs.block_q() > 0) ? ss2 : nullptr, (long)mc, rq.mu_out ? mu_c : nullptr,
                         rq.sd_out ? sd_c : nullptr, need_val ? val_c : nullptr);
      DFH_LAUNCH_CHECK();
      if (want_best) DFH_TRY(best.update(ctx, val_c, mc, i0));
    }
    if (rq.mu_out) DFH_TRY(from_device(ctx, rq.mu_out + i0, mu_c, (size_t)mc * 8));
    if (rq.sd_out) DFH_TRY(from_device(ctx, rq.sd_out + i0, sd_c, (size_t)mc * 8));
    if (rq.vals_out) DFH_TRY(from_device(ctx, rq.vals_out + i0, val_c, (size_t)mc * 8));
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
  rq.acq = DFH_ACQ_MEAN;
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

namespace {

// Epilogue of one chunk of the point-wise Thompson sampling (dfh_gp_ts_pointwise): per candidate the one-point draw
// s = sqrt(var) u + mu -- draw_gaussian_samples on a 1 x 1 covariance (general_utils.py:224-232: L.dot(U).T + mu, the
// product and the sum rounded apart; the build has no implicit fusion) -- with var the unclipped posterior variance
// of k_posterior_acq, and the first stage of the arg-max: one partial winner per workgroup (k_argmax_stage1's rule on
// one element per thread; k_argmax_stage2 finishes).  *bad is set when some var is not > 0, where the 1 x 1
// stable_cholesky fails on every rung of its ladder.
__global__ __launch_bounds__(256) void k_ts_pointwise(double kxx, const double* __restrict__ kss, double mean_const,
                                                      const double* __restrict__ mean_vals,
                                                      const double* __restrict__ mu_raw, const double* __restrict__ ss,
                                                      const double* __restrict__ ss2, const double* __restrict__ u, long m,
                                                      long idx_base, double* __restrict__ samp, double* __restrict__ pv,
                                                      long* __restrict__ pi, int* __restrict__ bad) {
  __shared__ double sv[256];
  __shared__ long si[256];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  double bv = -INFINITY;
  long bi = LONG_MAX;
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
  sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s]; const long oi = si[threadIdx.x + s];
      if (oi != LONG_MAX && (si[threadIdx.x] == LONG_MAX || better(ov, oi, sv[threadIdx.x], si[threadIdx.x]))) {
        sv[threadIdx.x] = ov; si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    pv[blockIdx.x] = sv[0]; pi[blockIdx.x] = si[0];
    if (not_pd) atomicOr(bad, 1);
  }
}

}  // namespace

// Point-wise Thompson sampling (include/dfhip.h): gp_eval_driver's chunk loop -- the posterior of dfh_gp_acq_argmax,
// points in progress included -- with k_ts_pointwise as the epilogue.  One synchronisation per chunk: the chunk's
// winner and its flag come back together.
extern "C" int dfh_gp_ts_pointwise(dfh_gp* gp, const double* Xs, int64_t m, const double* Xh, int64_t q, const double* U,
                                   double mean_const, const double* mean_vals, double* samples_out, double* best_val,
                                   int64_t* best_idx) {
  DFH_ARG(gp && Xs && U && m >= 1 && q >= 0 && (q == 0 || Xh));
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  HallucScope hs;                           // (hs.aug: the variance comes from the re-factored augmented GP)
  DFH_TRY(halluc_resolve(gp, Xh, q, &hs));
  const int64_t d = gp->d;
  const int64_t mc_max = pick_chunk(ctx, gp->n + (hs.aug ? q : 0), m);
  const ChunkStager stage(ctx, Xs, d, mean_vals);
  double* vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * 6, (void**)&vec));
  double* mu_raw = vec; double* ss = vec + mc_max; double* ss2 = vec + 2 * mc_max;
  double* samp = vec + 3 * mc_max; double* mu_aug = vec + 4 * mc_max;
  double* kss = gp->kd.stationary ? nullptr : vec + 5 * mc_max;
  const int nblocks_max = (int)((mc_max + 255) / 256);
  char* red = nullptr;                      // partial winners [nblocks] and the chunk's | their indices | the flag
  DFH_TRY(scratch_get(ctx, SCR_RED, (size_t)(nblocks_max + 1) * 16 + 64, (void**)&red));
  double* pv = reinterpret_cast<double*>(red);
  long* pi = reinterpret_cast<long*>(red + (size_t)(nblocks_max + 1) * 8);
  int* bad = reinterpret_cast<int*>(red + (size_t)(nblocks_max + 1) * 16);
  Winner best;
  ChunkReq creq;
  for (int64_t i0 = 0; i0 < m; i0 += mc_max) {
    const int64_t mc = std::min(mc_max, m - i0);
    const double* xs_c = nullptr;
    DFH_TRY(stage.xs(i0, mc, SCR_STAGE_A, &xs_c));
    const double* mv_c = nullptr;
    DFH_TRY(stage.mean(i0, mc, &mv_c));
    const double* u_c = nullptr;
    DFH_TRY(to_device(ctx, U + i0, (size_t)mc * 8, SCR_STAGE_C, &u_c));
    ChunkOut co;
    if (hs.aug) {
      // mean from the real data, variance from the augmented factor (gp_core.py:195, 207-213)
      creq.want_var = true; creq.h = nullptr;
      DFH_TRY(posterior_chunk(hs.aug, xs_c, mc, d, creq, mu_aug, ss, ss2));
      creq.want_var = false;
      DFH_TRY(posterior_chunk(gp, xs_c, mc, d, creq, mu_raw, nullptr, nullptr, &co));
    } else {
      creq.want_var = true; creq.h = &hs.h;
      DFH_TRY(posterior_chunk(gp, xs_c, mc, d, creq, mu_raw, ss, ss2, &co));
    }
    if (kss) DFH_TRY(prior_diag(ctx, gp->kd, co.Xsp, co.Nsp, mc, kss));
    const int nblocks = (int)((mc + 255) / 256);
    double hv = 0.0; long hi = -1; int hbad = 0;
    {
      SectionTimer t(ctx, DFH_T_ACQ);
      DFH_HIP(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
      hipLaunchKernelGGL(k_ts_pointwise, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, gp->kd.kxx, (const double*)kss,
                         mean_const, mv_c, (const double*)mu_raw, (const double*)ss,
                         hs.block_q() > 0 ? (const double*)ss2 : (const double*)nullptr, u_c, (long)mc, (long)i0, samp, pv, pi, bad);
      DFH_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_argmax_stage2, dim3(1), dim3(256), 0, ctx->stream, (const double*)pv, (const long*)pi, nblocks,
                         pv + nblocks_max, pi + nblocks_max);
      DFH_LAUNCH_CHECK();
      DFH_HIP(hipMemcpyAsync(&hv, pv + nblocks_max, 8, hipMemcpyDeviceToHost, ctx->stream));
      DFH_HIP(hipMemcpyAsync(&hi, pi + nblocks_max, 8, hipMemcpyDeviceToHost, ctx->stream));
      DFH_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      DFH_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (hbad) {
      dfh_set_error("Could not compute Cholesky decomposition of a candidate's 1 x 1 posterior covariance: the variance is "
                    "not positive. This is likely because the M is not positive semi-definite or has infinities/nans.");
      return DFH_ERR_JITTER;
    }
    best.merge(hv, (int64_t)hi);
    if (samples_out) DFH_TRY(from_device(ctx, samples_out + i0, samp, (size_t)mc * 8));
  }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  best.store(best_val, best_idx);
  return DFH_OK;
}

extern "C" int dfh_gp_add_ucb_group(dfh_gp* gp, int32_t group, double beta, const double* Xg, int64_t m,
                                    double* vals_out, double* best_val, int64_t* best_idx) {
  DFH_ARG(gp && Xg && m >= 1);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  DFH_ARG(gp->kd.multi && !gp->kd.product && !gp->kd.esp && group >= 0 && group < gp->kd.n_parts);   // additive kernels only
  const PartDev& pd = gp->kd.parts[group];
  int gdim = 0;
  for (int c = 0; c < pd.kc; ++c) gdim += gp->kd.cols[pd.poff + c] >= 0;
  const double params[2] = {beta, 0.0};
  EvalReq rq;
  rq.acq = DFH_ACQ_UCB; rq.params = params;
  rq.Xs = Xg; rq.m = m; rq.ldxs = gdim;
  rq.part_lo = group; rq.part_hi = group + 1; rq.pre_gathered = true;
  rq.kxx = gp->kd.outer_scale * kerndev_part_kxx(gp->kd, group);   // kern_scale * kernel_j(x,x)
  rq.want_var = true;
  rq.vals_out = vals_out; rq.best_val = best_val; rq.best_idx = best_idx;
  return gp_eval_driver(gp, rq);
}

// The groups of an additive model at once: the per-group cross matrices are stacked into one (sum m_g) x n
// matrix so that the posterior solve is ONE triangular solve with sum(m_g) right-hand sides instead
// of G small ones (the reference issues G solve_lower_triangular calls, gpb_acquisitions.py:161-176).
// Xg_all: group g's candidates [m_g x |group g|], back to back.  Falls back to the per-group
// route when the stack does not fit one posterior chunk.
int add_ucb_stacked(dfh_gp* gp, const StackedGroups& sg, const double* betas, const double* Xg_all, const int64_t* m_per_group,
                    double* vals_out, double* best_vals, int64_t* best_idx) {
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const KernDev& kd = gp->kd;
  const int G = sg.G, p0 = sg.part0;
  const int64_t n = gp->n;
  std::vector<int64_t> off(G + 1, 0), xoff(G + 1, 0);
  std::vector<int> gdim(G, 0);
  for (int g = 0; g < G; ++g) {
    DFH_ARG(m_per_group[g] >= 1);
    for (int c = 0; c < kd.parts[p0 + g].kc; ++c) gdim[g] += kd.cols[kd.parts[p0 + g].poff + c] >= 0;
    off[g + 1] = off[g] + m_per_group[g];
    xoff[g + 1] = xoff[g] + m_per_group[g] * gdim[g];
  }
  const int64_t M = off[G];
  if (M > pick_chunk(ctx, n, M)) {
    for (int g = 0; g < G; ++g)
      DFH_TRY(sg.one_group(g, betas[g], Xg_all + xoff[g], m_per_group[g], vals_out ? vals_out + off[g] : nullptr,
                           &best_vals[g], &best_idx[g]));
    return DFH_OK;
  }
  const double* dXg = nullptr;
  DFH_TRY(to_device(ctx, Xg_all, (size_t)xoff[G] * 8, SCR_STAGE_A, &dXg));
  static_assert(sizeof(long) == sizeof(int64_t), "offsets travel as int64");
  const double* d_off = nullptr;                     // segment offsets for the per-group arg-max
  DFH_TRY(to_device(ctx, reinterpret_cast<const double*>(off.data()), (size_t)(G + 1) * 8, SCR_STAGE_B, &d_off));
  char* xs = nullptr;
  const PackedXs lay = packed_xs_layout(kd, M);
  DFH_TRY(scratch_get(ctx, SCR_XS, lay.bytes, (void**)&xs));
  double* Xsp = reinterpret_cast<double*>(xs);
  double* Nsp = reinterpret_cast<double*>(xs + lay.nsp_off);
  double *Kct = nullptr, *vec = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)M * n * 8, (void**)&Kct));
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)M * 8 * 4, (void**)&vec));
  double* mu_raw = vec; double* ss = vec + M; double* val = vec + 2 * M; double* kss_w = vec + 3 * M;
  {
    SectionTimer t(ctx, DFH_T_CROSS);
    bool mu_all = true;          // posterior means from the cross-matrix pass itself where the kernel can
    for (int g = 0; g < G; ++g) {
      double* Xsp_g = Xsp + off[g] * kd.P; double* Nsp_g = Nsp + off[g] * kd.n_parts;
      DFH_TRY(pack_scaled(ctx, kd, p0 + g, p0 + g + 1, true, dXg + xoff[g], m_per_group[g], gdim[g], Xsp_g, Nsp_g));
      // K_j(X*_j, X[:, group j]) with the outer scale        (gpb_acquisitions.py:166-168; weighted: :364-366)
      KmMean mean{gp->alpha, mu_raw + off[g], false};
      DFH_TRY(kernmat_cross(ctx, kd, p0 + g, p0 + g + 1, true, KmPts{Xsp_g, Nsp_g, m_per_group[g]}, KmPts{gp->Xp, gp->Np, n},
                            Kct + off[g] * n, n, &mean, sg.col_w));
      mu_all = mu_all && mean.done;
    }
    if (!mu_all) DFH_TRY(gemv_rows(ctx, Kct, M, n, n, gp->alpha, 1.0, nullptr, 0.0, mu_raw));
  }
  {
    SectionTimer t(ctx, DFH_T_TRSM);
    DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, Kct, M, n, gp->refine.data()));
  }
  SectionTimer t(ctx, DFH_T_ACQ);
  DFH_TRY(row_sumsq(ctx, Kct, M, n, n, ss));
  for (int g = 0; g < G; ++g) {
    const double kxx = sg.prior_scale * kerndev_part_kxx(kd, p0 + g);   // kern_scale * kernel_j(x, x)
    const int64_t mg = m_per_group[g];
    const double* kss_g = nullptr;
    if (!part_is_stationary(kd, p0 + g)) {
      // a polynomial group: its prior variance depends on the point
      DFH_TRY(prior_diag(ctx, kd, Xsp + off[g] * kd.P, Nsp + off[g] * kd.n_parts, mg, kss_w + off[g], p0 + g, p0 + g + 1));
      kss_g = kss_w + off[g];
    }
    hipLaunchKernelGGL(k_posterior_acq, dim3((unsigned)((mg + 255) / 256)), dim3(256), 0, ctx->stream, (int)DFH_ACQ_UCB,
                       betas[g], 0.0, kxx, kss_g, 0.0, (const double*)nullptr, mu_raw + off[g], ss + off[g],
                       (const double*)nullptr, (long)mg, (double*)nullptr, (double*)nullptr, val + off[g]);
    DFH_LAUNCH_CHECK();
  }
  {   // the G arg-maxes in one launch and one copy back (each used to cost a stream synchronisation)
    char* red = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_RED, (size_t)G * 16, (void**)&red));
    double* d_bv = reinterpret_cast<double*>(red);
    long* d_bi = reinterpret_cast<long*>(red + (size_t)G * 8);
    hipLaunchKernelGGL(k_argmax_segments, dim3((unsigned)G), dim3(256), 0, ctx->stream, val,
                       reinterpret_cast<const long*>(d_off), d_bv, d_bi);
    DFH_LAUNCH_CHECK();
    DFH_HIP(hipMemcpyAsync(best_vals, d_bv, (size_t)G * 8, hipMemcpyDeviceToHost, ctx->stream));
    DFH_HIP(hipMemcpyAsync(best_idx, d_bi, (size_t)G * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (vals_out) DFH_TRY(from_device(ctx, vals_out, val, (size_t)M * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

// Every group of the additive kernel: parts [0, n_parts), the kernel's outer scale, no weights
extern "C" int dfh_gp_add_ucb_all(dfh_gp* gp, const double* betas, const double* Xg_all, const int64_t* m_per_group,
                                  double* vals_out, double* best_vals, int64_t* best_idx) {
  DFH_ARG(gp && betas && Xg_all && m_per_group && best_vals && best_idx);
  DFH_ARG(!gp->gram);
  DFH_ARG(gp->kd.multi && !gp->kd.product && !gp->kd.esp);     // additive kernels only
  StackedGroups sg;
  sg.part0 = 0; sg.G = gp->kd.n_parts; sg.prior_scale = gp->kd.outer_scale;
  sg.one_group = [gp](int g, double beta, const double* Xg, int64_t m, double* vals, double* bv, int64_t* bi) {
    return dfh_gp_add_ucb_group(gp, g, beta, Xg, m, vals, bv, bi);
  };
  return add_ucb_stacked(gp, sg, betas, Xg_all, m_per_group, vals_out, best_vals, best_idx);
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
