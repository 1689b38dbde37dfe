// The GP object: its fits from a kernel descriptor or a Gram matrix, the incremental update, the posterior from
// caller-evaluated kernel matrices, and the getters (include/dfhip.h).
#include "gp.h"
#include <algorithm>

// ---------------------------------------------------------------------------------------------
extern "C" int dfh_gp_free(dfh_gp* gp) {
  if (!gp) return DFH_OK;
  if (gp->ctx && ctx_is_live(gp->ctx)) {      // the context may already be gone (teardown order)
    (void)hipSetDevice(gp->ctx->device);
    (void)hipStreamSynchronize(gp->ctx->stream);
  }
  kerndev_free(&gp->kd);
  dev_release(gp->ctx, gp->Xp);
  dev_release(gp->ctx, gp->Np);
  dev_release(gp->ctx, gp->L);
  dev_release(gp->ctx, gp->inv);
  dev_release(gp->ctx, gp->alpha);
  delete gp;
  return DFH_OK;
}

extern "C" int64_t dfh_gp_n(dfh_gp* gp) { return gp ? gp->n : -1; }

extern "C" int dfh_gp_refine_steps(dfh_gp* gp, int32_t* steps_out) {
  DFH_ARG(gp && steps_out);
  for (int64_t b = 0; b < gp->nblk; ++b) steps_out[b] = b < (int64_t)gp->refine.size() ? gp->refine[b] : 0;
  return DFH_OK;
}

// alpha = L^T \ (L \ y_centred) (gp_core.py:161-163) and the log marginal likelihood (:224-226)
static int gp_alpha_and_lml(dfh_gp* gp, const double* dy, double* lml) {
  dfh_ctx* ctx = gp->ctx;
  const int64_t n = gp->n;
  SectionTimer t(ctx, DFH_T_SOLVE);
  DFH_HIP(hipMemcpyAsync(gp->alpha, dy, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
  DFH_TRY(trsv_both(ctx, gp->L, n, n, gp->inv, gp->alpha, gp->refine.data()));
  double logdet = 0.0, dot = 0.0;
  DFH_TRY(logdet_and_dot(ctx, gp->L, n, n, dy, gp->alpha, &logdet, &dot));
  gp->lml = lml_value(logdet, dot, n);
  if (lml) *lml = gp->lml;
  return DFH_OK;
}

// gp->L <- the factor of K + noise_var I for the n x n kernel matrix dK (device, without noise, left as it is) under
// _get_cholesky_decomp's three branches (gp_core.py:827-847); shared by dfh_gp_fit_gram and the flagged dfh_gp_fit / dfh_gp_append
static int factor_gram_psd(dfh_gp* gp, const double* dK, int flags, int32_t* jitter_power) {
  dfh_ctx* ctx = gp->ctx;
  const int64_t n = gp->n;
  const double noise_var = gp->noise_var;
  auto build_M = [&]() -> int {     // K + noise_var * I     (gp_core.py:843)
    DFH_TRY(copy_matrix(ctx, dK, n, gp->L, n, n, n));
    return add_diag(ctx, gp->L, n, n, noise_var);
  };
  bool project = (flags & DFH_FIT_PROJECT_FIRST) != 0;
  if (flags & DFH_FIT_TRY_BEFORE_PROJECT) {
    // gp_core.py:829-837: plain Cholesky of K + noise I (no ladder); only if that fails, project
    DFH_TRY(build_M());
    SectionTimer t(ctx, DFH_T_CHOL);
    int64_t piv = 0;
    const std::function<int()> rebuild_M = build_M;      // (a hand-off time-out repeats on the safe schedule)
    const int rc = cholesky_device(ctx, gp->L, n, n, gp->inv, &piv, 1, 0, 0, gp->refine.data(), false, &rebuild_M);
    if (rc == DFH_OK) return DFH_OK;
    if (rc != DFH_ERR_NOT_PD) return rc;
    project = true;
  }
  if (project) {
    // gp_core.py:838-841: the kernel matrix (without noise) goes to the PSD cone first
    double* Kp = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)n * n * 8, (void**)&Kp));
    DFH_TRY(psd_project_device(ctx, dK, n, n, 0.0, Kp, n));
    dK = Kp;
  }
  DFH_TRY(build_M());
  {
    SectionTimer t(ctx, DFH_T_CHOL);
    DFH_TRY(stable_cholesky_device(ctx, gp->L, n, gp->inv, !(flags & DFH_FIT_NO_JITTER), build_M,
                                   jitter_power, &gp->diag_jitter, 0, gp->refine.data()));
  }
  return DFH_OK;
}

extern "C" int dfh_gp_fit(dfh_ctx* ctx, const dfh_kernel_desc* k, const double* X, int64_t n, int64_t d,
                          const double* y_centred, double noise_var, int flags, dfh_gp** out,
                          double* lml, int32_t* jitter_power) {
  DFH_ARG(ctx && k && out && n >= 1 && d >= 1 && X && y_centred);
  DFH_ARG(k->dim == d);
  *out = nullptr;
  if (jitter_power) *jitter_power = INT32_MIN;
  DFH_HIP(hipSetDevice(ctx->device));
  dfh_gp* gp = new dfh_gp();
  gp->ctx = ctx; gp->n = n; gp->d = d; gp->noise_var = noise_var;
  gp->nblk = (n + CHOL_NB - 1) / CHOL_NB;
  auto body = [&]() -> int {
    DFH_TRY(kerndev_build(ctx, k, &gp->kd));
    const KernDev& kd = gp->kd;
    DFH_TRY(dev_alloc(ctx, (size_t)n * kd.P * 8, (void**)&gp->Xp));
    DFH_TRY(dev_alloc(ctx, (size_t)n * kd.n_parts * 8, (void**)&gp->Np));
    DFH_TRY(dev_alloc(ctx, (size_t)n * n * 8, (void**)&gp->L));
    DFH_TRY(dev_alloc(ctx, (size_t)inv_buffer_doubles(n) * 8, (void**)&gp->inv));
    gp->refine.assign((size_t)gp->nblk, 0);
    DFH_TRY(dev_alloc(ctx, (size_t)n * 8, (void**)&gp->alpha));
    const double *dX = nullptr, *dy = nullptr;
    DFH_TRY(to_device(ctx, X, (size_t)n * d * 8, SCR_STAGE_A, &dX));
    DFH_TRY(to_device(ctx, y_centred, (size_t)n * 8, SCR_STAGE_B, &dy));
    // From n = 2048 on only the lower triangle of the Gram matrix is written (the factorisation, in place in this buffer,
    // reads nothing else; whoever asks for GP.L gets a zeroed upper part, dfh_gp_get): half the bytes of the
    // HBM-write-bound build.  DFH_KM_LOWER_ONLY=0: the full symmetric matrix as before.
    static const bool lower_env = env_flag("DFH_KM_LOWER_ONLY", true);
    static const bool poison_l = env_flag("DFH_TEST_POISON_L", false);
    auto build_M = [&]() -> int {     // K + noise_var * I     (gp_core.py:843)
      SectionTimer t(ctx, DFH_T_KERNMAT);
      // test hook (tests/test_gpu_upper_triangle_unread.py): the buffer comes recycled from the pool, and with the
      // lower-triangle-only build the tiles above the diagonal keep whatever it held -- correctness rests on no schedule
      // of the factorisation or the solves ever reading them.  DFH_TEST_POISON_L=1 fills the buffer with NaN first.
      if (poison_l) DFH_HIP(hipMemsetAsync(gp->L, 0xFF, (size_t)n * n * 8, ctx->stream));
      return kernmat_gram(ctx, kd, 0, kd.n_parts, true, KmPts{gp->Xp, gp->Np, n}, noise_var, gp->L, n, lower_env && n >= 2048);
    };
    {
      SectionTimer t(ctx, DFH_T_KERNMAT);
      DFH_TRY(pack_scaled(ctx, kd, 0, kd.n_parts, false, dX, n, d, gp->Xp, gp->Np));
    }
    if (flags & DFH_FIT_PSD_FLAGS) {
      // gp_core.py:827-841 from the descriptor: the whole kernel matrix (no noise, both triangles: the projection
      // multiplies with it) is built in a workspace, and the factor comes from it as dfh_gp_fit_gram's does
      gp->psd_flags = flags & DFH_FIT_PSD_FLAGS;
      double* Kw = nullptr;
      DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n * n * 8, (void**)&Kw));
      {
        SectionTimer t(ctx, DFH_T_KERNMAT);
        DFH_TRY(kernmat_gram(ctx, kd, 0, kd.n_parts, true, KmPts{gp->Xp, gp->Np, n}, 0.0, Kw, n));
      }
      DFH_TRY(factor_gram_psd(gp, Kw, flags, jitter_power));
      return gp_alpha_and_lml(gp, dy, lml);
    }
    DFH_TRY(build_M());
    {
      SectionTimer t(ctx, DFH_T_CHOL);
      DFH_TRY(stable_cholesky_device(ctx, gp->L, n, gp->inv, !(flags & DFH_FIT_NO_JITTER), build_M,
                                     jitter_power, &gp->diag_jitter, 0, gp->refine.data()));
    }
    return gp_alpha_and_lml(gp, dy, lml);
  };
  int rc = body();
  if (rc != DFH_OK) { dfh_gp_free(gp); return rc; }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  *out = gp;
  return DFH_OK;
}

// ---------------------------------------------------------------------------------------------
// Posterior for an arbitrary positive semi-definite kernel evaluated by the caller:
// GP.build_posterior with the Gram matrix coming from the documented override hook
// GP._get_training_kernel_matrix (gp_core.py:149-163), and GP.eval with the caller's K(X*, X)
// (gp_core.py:165-190).  The O(n^3) / O(n^2 m) linear algebra is the same device path as for the
// built-in kernels; only the kernel evaluations stay with the caller.
__global__ void k_sd_from_prior(const double* __restrict__ kss, const double* __restrict__ ss,
                                double* __restrict__ sd, long m) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) sd[i] = sqrt(kss[i] - ss[i]);        // no clipping: NaN as in np.sqrt(np.diag(.)), gp_core.py:187
}

extern "C" int dfh_gp_fit_gram(dfh_ctx* ctx, const double* K, int64_t n, const double* y_centred,
                               double noise_var, int flags, dfh_gp** out, double* lml, int32_t* jitter_power) {
  DFH_ARG(ctx && K && out && n >= 1 && y_centred);
  *out = nullptr;
  if (jitter_power) *jitter_power = INT32_MIN;
  DFH_HIP(hipSetDevice(ctx->device));
  dfh_gp* gp = new dfh_gp();
  gp->ctx = ctx; gp->n = n; gp->d = 0; gp->noise_var = noise_var; gp->gram = true;
  gp->nblk = (n + CHOL_NB - 1) / CHOL_NB;
  auto body = [&]() -> int {
    DFH_TRY(dev_alloc(ctx, (size_t)n * n * 8, (void**)&gp->L));
    DFH_TRY(dev_alloc(ctx, (size_t)inv_buffer_doubles(n) * 8, (void**)&gp->inv));
    gp->refine.assign((size_t)gp->nblk, 0);
    DFH_TRY(dev_alloc(ctx, (size_t)n * 8, (void**)&gp->alpha));
    const double *dK = nullptr, *dy = nullptr;
    DFH_TRY(to_device(ctx, K, (size_t)n * n * 8, SCR_KCT, &dK));
    DFH_TRY(to_device(ctx, y_centred, (size_t)n * 8, SCR_STAGE_B, &dy));
    DFH_TRY(factor_gram_psd(gp, dK, flags, jitter_power));
    return gp_alpha_and_lml(gp, dy, lml);
  };
  int rc = body();
  if (rc != DFH_OK) { dfh_gp_free(gp); return rc; }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  *out = gp;
  return DFH_OK;
}

// mu = Kcross alpha (+ mean), sd = sqrt(kss - rowsumsq(Kcross L^-T)); Kcross is m x n, row i = k(x*_i, X)
extern "C" int dfh_gp_predict_gram(dfh_gp* gp, const double* Kcross, int64_t m, const double* kss,
                                   double mean_const, const double* mean_vals, double* mu_out, double* sd_out) {
  DFH_ARG(gp && m >= 0 && (sd_out == nullptr || kss != nullptr));
  if (m == 0) return DFH_OK;
  DFH_ARG(Kcross && mu_out);
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n;
  const int64_t mc_max = pick_chunk(ctx, n, m);
  const bool k_dev = is_device_ptr(Kcross), s_dev = kss ? is_device_ptr(kss) : true;
  const ChunkStager stage(ctx, nullptr, 0, mean_vals);
  double *vec = nullptr, *Kct = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)mc_max * 8 * 4, (void**)&vec));
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)mc_max * n * 8, (void**)&Kct));
  double* mu = vec; double* ss = vec + mc_max; double* sd = vec + 2 * mc_max; double* ks = vec + 3 * mc_max;
  for (int64_t i0 = 0; i0 < m; i0 += mc_max) {
    const int64_t mc = std::min(mc_max, m - i0);
    // the chunk of K(X*, X) is solved in place, so it always goes through the workspace
    DFH_HIP(hipMemcpyAsync(Kct, Kcross + i0 * n, (size_t)mc * n * 8,
                           k_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    {
      SectionTimer t(ctx, DFH_T_CROSS);
      DFH_TRY(gemv_rows(ctx, Kct, mc, n, n, gp->alpha, 1.0, nullptr, 0.0, mu));     // gp_core.py:174
    }
    const double* mv_c = nullptr;
    DFH_TRY(stage.mean(i0, mc, &mv_c));
    DFH_TRY(add_vec(ctx, mu, mv_c, mv_c ? 0.0 : mean_const, mc));
    DFH_TRY(from_device(ctx, mu_out + i0, mu, (size_t)mc * 8));
    if (sd_out) {
      {
        SectionTimer t(ctx, DFH_T_TRSM);
        DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, Kct, mc, n, gp->refine.data()));                  // gp_core.py:180
      }
      SectionTimer t(ctx, DFH_T_ACQ);
      DFH_TRY(row_sumsq(ctx, Kct, mc, n, n, ss));
      const double* ks_c = kss + i0;
      if (!s_dev) {
        DFH_HIP(hipMemcpyAsync(ks, kss + i0, (size_t)mc * 8, hipMemcpyHostToDevice, ctx->stream));
        ks_c = ks;
      }
      hipLaunchKernelGGL(k_sd_from_prior, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, ctx->stream, ks_c, ss, sd, (long)mc);
      DFH_LAUNCH_CHECK();
      DFH_TRY(from_device(ctx, sd_out + i0, sd, (size_t)mc * 8));
    }
    DFH_HIP(hipStreamSynchronize(ctx->stream));      // host source buffers may be reused by the caller
  }
  return DFH_OK;
}

// mu_out = Kcross alpha (raw, no mean), cov_out = Ktete - V^T V with V^T = Kcross L^-T  (gp_core.py:179-181)
extern "C" int dfh_gp_predict_covar_gram(dfh_gp* gp, const double* Kcross, int64_t m, const double* Ktete,
                                         double* mu_out, double* cov_out) {
  DFH_ARG(gp && m >= 0);
  if (m == 0) return DFH_OK;
  DFH_ARG(Kcross && Ktete && mu_out && cov_out);
  DFH_ARG((double)m * (double)gp->n * 8.0 < 64e9 && (double)m * (double)m * 8.0 < 64e9);
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n;
  double *vec = nullptr, *Kct = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_VEC, (size_t)m * 8, (void**)&vec));
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)m * n * 8, (void**)&Kct));
  DFH_HIP(hipMemcpyAsync(Kct, Kcross, (size_t)m * n * 8,
                         is_device_ptr(Kcross) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  DFH_TRY(gemv_rows(ctx, Kct, m, n, n, gp->alpha, 1.0, nullptr, 0.0, vec));
  DFH_TRY(from_device(ctx, mu_out, vec, (size_t)m * 8));
  DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, Kct, m, n, gp->refine.data()));
  const bool dev_out = is_device_ptr(cov_out);
  double* C = cov_out;
  if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)m * m * 8, (void**)&C));
  DFH_HIP(hipMemcpyAsync(C, Ktete, (size_t)m * m * 8,
                         is_device_ptr(Ktete) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  DFH_TRY(gemm_f64(ctx, 0, m, m, n, -1.0, Kct, n, Kct, n, 1.0, C, m, C, m));
  if (!dev_out) DFH_TRY(from_device(ctx, cov_out, C, (size_t)m * m * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

// ---------------------------------------------------------------------------------------------
// Incremental posterior update.  GP.add_data_multiple (gp_core.py:139-146)
// extends X, Y and rebuilds the posterior from scratch -- O((n+q)^3).  With the same kernel,
// noise and data order the factor of the extended matrix is
//     L' = [ L  0 ; B  Ls ],  B = K(Xnew, X) L^-T,  Ls = chol(K(Xnew,Xnew) + noise I - B B^T)
// (the Cholesky factor is unique), which costs O(n^2 q).  A NEW handle is returned; `gp` is left
// untouched (shallow copies of a GP share the handle).  When the reference's rebuild would leave
// the plain-Cholesky branch -- the existing fit needed the stable_cholesky ladder, or the Schur
// complement is not positive definite -- the extended matrix is rebuilt and factored from
// scratch with the ladder, exactly what build_posterior would do.
extern "C" int dfh_gp_append(dfh_gp* gp, const double* Xnew, int64_t q, const double* y_centred, int flags,
                             dfh_gp** out, double* lml, int32_t* jitter_power) {
  DFH_ARG(gp && out && q >= 1 && Xnew && y_centred);
  DFH_ARG(!gp->gram);      // needs the kernel: this posterior was built from a Gram matrix
  *out = nullptr;
  if (jitter_power) *jitter_power = INT32_MIN;
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n, n2 = gp->n + q, d = gp->d, NB = CHOL_NB;
  dfh_gp* g2 = new dfh_gp();
  g2->ctx = ctx; g2->n = n2; g2->d = d; g2->noise_var = gp->noise_var;
  g2->nblk = (n2 + NB - 1) / NB;
  auto body = [&]() -> int {
    DFH_TRY(kerndev_clone(ctx, gp->kd, &g2->kd));
    const KernDev& kd = g2->kd;
    const int64_t P = kd.P, parts = kd.n_parts;
    DFH_TRY(dev_alloc(ctx, (size_t)n2 * P * 8, (void**)&g2->Xp));
    DFH_TRY(dev_alloc(ctx, (size_t)n2 * parts * 8, (void**)&g2->Np));
    DFH_TRY(dev_alloc(ctx, (size_t)n2 * n2 * 8, (void**)&g2->L));
    DFH_TRY(dev_alloc(ctx, (size_t)inv_buffer_doubles(n2) * 8, (void**)&g2->inv));
    g2->refine.assign((size_t)g2->nblk, 0);
    DFH_TRY(dev_alloc(ctx, (size_t)n2 * 8, (void**)&g2->alpha));
    const double *dXn = nullptr, *dy = nullptr;
    DFH_TRY(to_device(ctx, Xnew, (size_t)q * d * 8, SCR_STAGE_A, &dXn));
    DFH_TRY(to_device(ctx, y_centred, (size_t)n2 * 8, SCR_STAGE_B, &dy));
    double* Xpn = g2->Xp + n * P; double* Npn = g2->Np + n * parts;
    {
      SectionTimer t(ctx, DFH_T_KERNMAT);
      DFH_HIP(hipMemcpyAsync(g2->Xp, gp->Xp, (size_t)n * P * 8, hipMemcpyDeviceToDevice, ctx->stream));
      DFH_HIP(hipMemcpyAsync(g2->Np, gp->Np, (size_t)n * parts * 8, hipMemcpyDeviceToDevice, ctx->stream));
      DFH_TRY(pack_scaled(ctx, kd, 0, parts, false, dXn, q, d, Xpn, Npn));
    }
    auto full_refit = [&]() -> int {             // what build_posterior does: K' + noise I, ladder
      if (gp->psd_flags) {                       // ... or the projection branches, as the fit this handle came from
        g2->psd_flags = gp->psd_flags;
        double* Kw = nullptr;
        DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n2 * n2 * 8, (void**)&Kw));
        {
          SectionTimer t(ctx, DFH_T_KERNMAT);
          DFH_TRY(kernmat_gram(ctx, kd, 0, parts, true, KmPts{g2->Xp, g2->Np, n2}, 0.0, Kw, n2));
        }
        return factor_gram_psd(g2, Kw, gp->psd_flags | (flags & DFH_FIT_NO_JITTER), jitter_power);
      }
      auto build_M = [&]() -> int {
        SectionTimer t(ctx, DFH_T_KERNMAT);
        return kernmat_gram(ctx, kd, 0, parts, true, KmPts{g2->Xp, g2->Np, n2}, g2->noise_var, g2->L, n2);
      };
      DFH_TRY(build_M());
      SectionTimer t(ctx, DFH_T_CHOL);
      return stable_cholesky_device(ctx, g2->L, n2, g2->inv, !(flags & DFH_FIT_NO_JITTER), build_M,
                                    jitter_power, &g2->diag_jitter, 0, g2->refine.data());
    };
    bool appended = false;
    if (gp->diag_jitter == 0.0 && !gp->psd_flags) {       // (a projection is not a block-row update)
      double* Bm = g2->L + n * n2;               // rows n.., columns 0..n-1
      double* S = g2->L + n * n2 + n;            // the new diagonal block (ld n2)
      DFH_TRY(copy_matrix(ctx, gp->L, n, g2->L, n2, n, n));
      {
        SectionTimer t(ctx, DFH_T_CROSS);
        DFH_TRY(kernmat_cross(ctx, kd, 0, parts, true, KmPts{Xpn, Npn, q}, KmPts{g2->Xp, g2->Np, n}, Bm, n2));
      }
      {
        SectionTimer t(ctx, DFH_T_TRSM);
        DFH_TRY(trsm_rows(ctx, gp->L, n, n, gp->inv, Bm, q, n2, gp->refine.data()));
      }
      {
        SectionTimer t(ctx, DFH_T_CHOL);
        const std::function<int()> build_S = [&]() -> int {
          DFH_TRY(kernmat_gram(ctx, kd, 0, parts, true, KmPts{Xpn, Npn, q}, g2->noise_var, S, n2));
          return gemm_f64(ctx, GEMM_LOWER, q, q, n, -1.0, Bm, n2, Bm, n2, 1.0, S, n2, S, n2);
        };
        DFH_TRY(build_S());
        int64_t piv = 0;
        const int rc = cholesky_device(ctx, S, q, n2, nullptr, &piv, 1, 0, 0, nullptr, false, &build_S);
        if (rc == DFH_OK) {
          // inverses of the 512-blocks: untouched blocks are copied, the rest recomputed from L'
          const int64_t kb0 = n / NB;            // first diagonal block that contains a new row
          double* diag2 = g2->inv + g2->nblk * NB * NB;
          if (kb0 > 0) {
            DFH_HIP(hipMemcpyAsync(g2->inv, gp->inv, (size_t)kb0 * NB * NB * 8, hipMemcpyDeviceToDevice, ctx->stream));
            DFH_HIP(hipMemcpyAsync(diag2, gp->inv + gp->nblk * NB * NB, (size_t)kb0 * NB * NB * 8,
                                   hipMemcpyDeviceToDevice, ctx->stream));
            std::copy(gp->refine.begin(), gp->refine.begin() + kb0, g2->refine.begin());
          }
          DFH_TRY(tri_block_inverses(ctx, g2->L + kb0 * NB * (n2 + 1), n2 - kb0 * NB, n2, g2->inv + kb0 * NB * NB,
                                     g2->refine.data() + kb0, diag2 + kb0 * NB * NB));
          appended = true;
        } else if (rc != DFH_ERR_NOT_PD) {
          return rc;
        }
      }
    }
    if (!appended) DFH_TRY(full_refit());
    return gp_alpha_and_lml(g2, dy, lml);
  };
  int rc = body();
  if (rc != DFH_OK) { dfh_gp_free(g2); return rc; }
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  *out = g2;
  return DFH_OK;
}

extern "C" int dfh_gp_get(dfh_gp* gp, int what, double* out) {
  DFH_ARG(gp && out);
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const int64_t n = gp->n;
  if (what == DFH_GET_ALPHA) return from_device(ctx, out, gp->alpha, (size_t)n * 8);
  if (what == DFH_GET_L) {
    if (!gp->upper_zeroed) { DFH_TRY(zero_upper(ctx, gp->L, n, n)); gp->upper_zeroed = true; }
    return from_device(ctx, out, gp->L, (size_t)n * n * 8);
  }
  if (what == DFH_GET_K) {
    DFH_ARG(!gp->gram);      // the caller evaluated the Gram matrix and still has it
    const bool dev_out = is_device_ptr(out);
    double* Kd = out;
    if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n * n * 8, (void**)&Kd));
    DFH_TRY(kernmat_gram(ctx, gp->kd, 0, gp->kd.n_parts, true, KmPts{gp->Xp, gp->Np, n}, 0.0, Kd, n));
    if (!dev_out) DFH_TRY(from_device(ctx, out, Kd, (size_t)n * n * 8));
    return DFH_OK;
  }
  dfh_set_error("dfh_gp_get: unknown selector %d", what);
  return DFH_ERR_BAD_ARG;
}
