// add-UCB on an additive kernel (include/dfhip.h): one group at a time through the chunked driver, or every group
// stacked into one posterior solve; gp_mf.hip runs the same stack at a fixed fidelity.
#include "gp.h"
#include <algorithm>

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
  const double* d_off = nullptr;                     // segment offsets for the per-group arg-max (argmax.h: long is int64_t)
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
    AcqArgs a;
    a.acq = DFH_ACQ_UCB; a.p0 = betas[g];
    a.kxx = kxx; a.kss = kss_g;
    a.mu_raw = mu_raw + off[g]; a.ss = ss + off[g]; a.m = mg;
    a.val_out = val + off[g];
    DFH_TRY(posterior_acq(ctx, a));
  }
  {   // the G arg-maxes in one launch and one copy back (each used to cost a stream synchronisation)
    char* red = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_RED, (size_t)G * 16, (void**)&red));
    double* d_bv = reinterpret_cast<double*>(red);
    long* d_bi = reinterpret_cast<long*>(red + (size_t)G * 8);
    DFH_TRY(argmax_segments(ctx, val, reinterpret_cast<const long*>(d_off), G, d_bv, d_bi));
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
