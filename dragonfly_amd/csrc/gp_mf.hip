// BOCA's decision step on a multi-fidelity GP (opt/gpb_acquisitions.py:313-439): add-UCB over the groups of the additive
// domain model at a fixed fidelity z*, and the joint candidates [z*, x] of every other acquisition.
//
// The GP's kernel is kern_scale * k_fid(z, z') * (fscale * sum_j k_j(x_j, x'_j)).  At a fixed z* the fidelity factor of
// the cross matrix depends on the training row alone, so group j's posterior (:364-373) is the additive add-UCB
// posterior with a weight per training row:
//   K_tetr_j[a][i] = (kern_scale * k_fid(z*, Z_i)) * k_j(x_a, X_i[group j])        (the weight: k_fid_weights)
//   prior variance = (kern_scale * k_fid(z*, z*)) * k_j(x, x)
// The additive factor's own scale does not enter: the reference uses the group kernels directly.  The weight goes
// into the cross matrix where it is stored (kernmat_cross: col_w), the mean, the row solve, the acquisition and the
// arg-max are the drivers of gp_posterior.hip.
#include "gp.h"
#include <algorithm>
#include "kernmat.h"      // kerneval.h's part evaluators, in this unit's anonymous namespace

namespace {

// w[i] = scale * k_fid(Z_i, z*) for the n training rows, w[n] = scale * k_fid(z*, z*): part 0 of the kernel between the
// packed training inputs and the packed fidelity zp (one row).  The dot product adds its terms one by one, as the row
// norms do below 8 columns (np_sumsq), so that a training row at z* itself has squared distance exactly 0.
__global__ void k_fid_weights(const PartDev* __restrict__ parts, int n_parts, int P, double scale, ExpConsts ec,
                              const double* __restrict__ zp, const double* __restrict__ znp, const double* __restrict__ Xp,
                              const double* __restrict__ Np, long n, double* __restrict__ w) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const PartDev& pd = parts[0];
  const double* x = zp + pd.poff;
  const double* y = i < n ? Xp + i * P + pd.poff : x;
  const double ny = i < n ? Np[i * n_parts] : znp[0];
  double kv;
  if (pd.kind == DFH_KERNEL_EXPDECAY) {
    kv = expdecay_eval(pd, y, x);                                    // kernel.py:418-432
  } else {
    double dot = 0.0;
    for (int c = 0; c < pd.kc; ++c) dot += y[c] * x[c];
    if (pd.kind == DFH_KERNEL_POLY) {
      kv = poly_eval(pd, dot);                                       // kernel.py:381-386
    } else {
      double dsq = (znp[0] + ny) - 2.0 * dot;                        // general_utils.py:66-68
      dsq = dsq < 0.0 ? 0.0 : dsq;
      if (i == n) dsq = 0.0;
      kv = kern_eval(pd, dsq, ec);
    }
  }
  w[i] = scale * kv;                                                 // gpb_acquisitions.py:366, 368
}

// out[a] = [z, Xd[a]]
__global__ void k_join_fixed(const double* __restrict__ z, int p, const double* __restrict__ Xd, long m, int d,
                             double* __restrict__ out) {
  const long w = (long)p + d, total = m * w;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const long a = idx / w;
    const int c = (int)(idx - a * w);
    out[idx] = c < p ? z[c] : Xd[a * d + (c - p)];
  }
}

// The shape the multi-fidelity add-UCB needs of a fitted GP: a product of exactly two factors, a plain fidelity factor
// (part 0) and a sum of SE / Matern groups (parts 1 .. n_parts - 1), fitted without projections.
int mf_shape(const dfh_gp* gp, int* n_groups, int* fid_dim) {
  DFH_ARG(!gp->gram);
  const KernDev& kd = gp->kd;
  DFH_ARG(kd.multi && kd.product && kd.nested && !kd.esp && kd.n_parts >= 2);
  DFH_ARG(gp->psd_flags == 0);       // L is the factor of the kernel's own matrix
  const PartDev& fid = kd.parts[0];
  DFH_ARG(fid.fmode == 0 && fid.kind != DFH_KERNEL_HAMMING);
  for (int g = 1; g < kd.n_parts; ++g) {
    const PartDev& pd = kd.parts[g];
    DFH_ARG((pd.fmode & FM_IN) && part_is_stationary(kd, g));
    DFH_ARG(((pd.fmode & FM_BEGIN) != 0) == (g == 1) && ((pd.fmode & FM_END) != 0) == (g == kd.n_parts - 1));
  }
  int p = 0;
  for (int c = 0; c < fid.kc; ++c) p += kd.cols[fid.poff + c] >= 0;
  *n_groups = kd.n_parts - 1;
  *fid_dim = p;
  return DFH_OK;
}

// The weights of the training rows at the fidelity z (host, [fid_dim]) in `blk` (n doubles at *w), and kern_scale * k_ff
int mf_weights(dfh_gp* gp, const double* z, int fid_dim, DevBlock* blk, const double** w, double* kff_scaled) {
  dfh_ctx* ctx = gp->ctx;
  DFH_HIP(hipSetDevice(ctx->device));
  const KernDev& kd = gp->kd;
  const int64_t n = gp->n;
  const size_t b_w = ((size_t)(n + 1) * 8 + 255) / 256 * 256, b_zp = ((size_t)kd.P * 8 + 255) / 256 * 256;
  DFH_TRY(dev_alloc(ctx, b_w + b_zp + (size_t)kd.n_parts * 8, &blk->p));
  double* dw = static_cast<double*>(blk->p);
  double* zp = reinterpret_cast<double*>(static_cast<char*>(blk->p) + b_w);
  double* znp = reinterpret_cast<double*>(static_cast<char*>(blk->p) + b_w + b_zp);
  const double* dz = nullptr;
  DFH_TRY(to_device(ctx, z, (size_t)fid_dim * 8, SCR_STAGE_C, &dz));
  DFH_TRY(pack_scaled(ctx, kd, 0, 1, true, dz, 1, fid_dim, zp, znp));
  hipLaunchKernelGGL(k_fid_weights, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, ctx->stream, kd.d_parts, kd.n_parts,
                     kd.P, kd.outer_scale, kExpConsts, zp, znp, gp->Xp, gp->Np, (long)n, dw);
  DFH_LAUNCH_CHECK();
  DFH_HIP(hipMemcpyAsync(kff_scaled, dw + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  *w = dw;
  return DFH_OK;
}

int mf_group_eval(dfh_gp* gp, const double* w, double kff_scaled, int group, double beta, const double* Xg, int64_t m,
                  double* vals_out, double* best_val, int64_t* best_idx) {
  const KernDev& kd = gp->kd;
  const int part = 1 + group;
  const PartDev& pd = kd.parts[part];
  int gdim = 0;
  for (int c = 0; c < pd.kc; ++c) gdim += kd.cols[pd.poff + c] >= 0;
  const double params[2] = {beta, 0.0};
  EvalReq rq;
  rq.acq = DFH_ACQ_UCB; rq.params = params;
  rq.Xs = Xg; rq.m = m; rq.ldxs = gdim;
  rq.part_lo = part; rq.part_hi = part + 1; rq.pre_gathered = true;
  rq.col_w = w;
  rq.kxx = kff_scaled * kerndev_part_kxx(kd, part);        // (kern_scale * k_ff) * kernel_j(x, x), gpb_acquisitions.py:368
  rq.want_var = true;
  rq.vals_out = vals_out; rq.best_val = best_val; rq.best_idx = best_idx;
  return gp_eval_driver(gp, rq);
}

}  // namespace

extern "C" int dfh_mf_add_ucb_group(dfh_gp* gp, const double* z_opt, int32_t group, double beta, const double* Xg, int64_t m,
                                    double* vals_out, double* best_val, int64_t* best_idx) {
  DFH_ARG(gp && z_opt && Xg && m >= 1);
  int G = 0, p = 0;
  DFH_TRY(mf_shape(gp, &G, &p));
  DFH_ARG(group >= 0 && group < G);
  DevBlock blk(gp->ctx);
  const double* w = nullptr;
  double kff = 0.0;
  DFH_TRY(mf_weights(gp, z_opt, p, &blk, &w, &kff));
  return mf_group_eval(gp, w, kff, group, beta, Xg, m, vals_out, best_val, best_idx);
}

extern "C" int dfh_mf_add_ucb_all(dfh_gp* gp, const double* z_opt, const double* betas, const double* Xg_all,
                                  const int64_t* m_per_group, double* vals_out, double* best_vals, int64_t* best_idx) {
  DFH_ARG(gp && z_opt && betas && Xg_all && m_per_group && best_vals && best_idx);
  int G = 0, p = 0;
  DFH_TRY(mf_shape(gp, &G, &p));
  DevBlock blk(gp->ctx);
  const double* w = nullptr;
  double kff = 0.0;
  DFH_TRY(mf_weights(gp, z_opt, p, &blk, &w, &kff));
  StackedGroups sg;
  sg.part0 = 1; sg.G = G; sg.col_w = w; sg.prior_scale = kff;
  sg.one_group = [gp, w, kff](int g, double beta, const double* Xg, int64_t m, double* vals, double* bv, int64_t* bi) {
    return mf_group_eval(gp, w, kff, g, beta, Xg, m, vals, bv, bi);
  };
  return add_ucb_stacked(gp, sg, betas, Xg_all, m_per_group, vals_out, best_vals, best_idx);
}

extern "C" int dfh_join_fixed_columns(dfh_ctx* ctx, const double* z, int64_t p, const double* Xd, int64_t m, int64_t d,
                                      double* out) {
  DFH_ARG(ctx && p >= 1 && d >= 1 && m >= 0 && p <= 4096 && d < (1LL << 30));
  if (m == 0) return DFH_OK;
  DFH_ARG(z && Xd && out && !is_device_ptr(z) && is_device_ptr(Xd) && is_device_ptr(out));
  DFH_HIP(hipSetDevice(ctx->device));
  const double* dz = nullptr;
  DFH_TRY(to_device(ctx, z, (size_t)p * 8, SCR_STAGE_D, &dz));
  const int64_t total = m * (p + d);
  const int64_t blocks = std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_join_fixed, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, dz, (int)p, Xd, (long)m, (int)d, out);
  DFH_LAUNCH_CHECK();
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}
