// The points in progress of a call (gp_core.py:192-220): the block form of the augmented solve on the GP's own factor,
// the augmented GP factored from scratch where that form does not hold, and the one chunk step that chooses between them.
#include "gp.h"

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

// Fallback of the hallucinated posterior: the GP over (X, Xh) factored from scratch with the
// stable_cholesky ladder -- literally gp_core.py:196-206; only its variance is used (the labels
// are irrelevant: zeros).  The caller frees *aug.
int halluc_augmented_gp(dfh_gp* gp, const double* Xh, int64_t q, dfh_gp** aug) {
  std::vector<double> y0((size_t)(gp->n + q), 0.0);
  return dfh_gp_append(gp, Xh, q, y0.data(), 0, aug, nullptr, nullptr);
}

}  // namespace

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

// The posterior of one chunk with the scope's points in progress: fills mu_raw, and with rq.want_var ss (and, in block
// form, ss2).  Augmented route: the mean from hs.gp first, then V^T and ss from hs.aug, whose own mean goes to `spare` --
// both calls fill the same buffers (rq.parity), and hs.aug's clone of the kernel packs the candidates to the same bytes,
// so only the cross matrix remembers which call came last: it must be the one of the factor.  Block route: the one call,
// with the second block row.  *out is what hs.cov_gp()'s call left; k(x, x) per candidate is that GP's kd on out->Xsp.
int halluc_chunk(const HallucScope& hs, const double* Xs_dev, int64_t mc, int64_t ldxs, ChunkReq rq, double* mu_raw,
                 double* ss, double* ss2, double* spare, ChunkOut* out) {
  if (hs.aug) {
    // mean from the real data, variance from the augmented factor (gp_core.py:195, 207-213)
    rq.h = nullptr; rq.want_var = false;
    DFH_TRY(posterior_chunk(hs.gp, Xs_dev, mc, ldxs, rq, mu_raw, nullptr, nullptr));
    rq.want_var = true;
    return posterior_chunk(hs.aug, Xs_dev, mc, ldxs, rq, spare, ss, ss2, out);
  }
  rq.h = hs.block();
  return posterior_chunk(hs.gp, Xs_dev, mc, ldxs, rq, mu_raw, ss, ss2, out);
}
