// Kernel-matrix construction: SE / Matern / additive Gram and cross matrices in fp64.
//
// Replaces, fused into one pass over the output,
//   get_scaled_repr                 dragonfly/gp/kernel.py:179-181, 255-257   (pack_scaled)
//   dist_squared (+ clip at 0)      dragonfly/utils/general_utils.py:58-70
//   SEKernel._child_evaluate        dragonfly/gp/kernel.py:171-177
//   MaternKernel._child_evaluate    dragonfly/gp/kernel.py:259-270, 292-299
//   AdditiveKernel._child_evaluate  dragonfly/gp/kernel.py:484-494
//   K + noise_var*np.eye(n)         dragonfly/gp/gp_core.py:843               (diag_add)
//
// The reference materialises three n1 x n2 temporaries plus the dgemm output; here each
// 128 x 128 (128 x 64 for additive) output tile is produced in registers: the -2 X1 X2^T term
// runs on the fp64 matrix cores (same expansion as the reference, so the same rounding
// behaviour), the norms / clip / exp / Matern polynomial run on the VALU beside it, and the
// only HBM traffic is the coalesced write of K (the pass is HBM-write bound:
// 8*(n1*n2 + (n1+n2)*d) algorithmic bytes).
//
// This unit chooses the route of a call; the kernels and their launch code are in km_sym.hip (single part, LDS-staged
// stores; symmetric multi-part), km_strip.hip (cross matrices, no LDS, fused posterior mean), km_generic.hip (any
// parts, any alignment) and km_esp.hip; the inputs they read are packed in km_pack.hip from the descriptors of kerndev.hip.
#include "kernmat.h"

const KmSwitches& km_switches() {
  static const KmSwitches sw;
  return sw;
}

static int kernmat_dispatch(dfh_ctx* ctx, const KmCall& c) {
  if (c.mean) c.mean->done = false;
  if (c.a.n <= 0 || c.b.n <= 0) return DFH_OK;
  DFH_ARG(c.a.n < (1LL << 31) && c.b.n < (1LL << 31));
  ctx->km_dispatches += 1;               // the booking of dfh_ctx_counters (host only)
  KmRoute route;
  if (c.col_w) route = KM_ROUTE_COLW;                    // weighted columns: one route knows them
  else if (c.kd->esp) route = KM_ROUTE_ESP;              // the whole ESP kernel in one kernel of its own; no fused posterior mean
  else if (km_single_aligned(c)) route = c.symmetric ? KM_ROUTE_SYM : (km_strip_ok(c) ? KM_ROUTE_STRIP : KM_ROUTE_CROSS_LDS);
  else route = km_symmulti_ok(c) ? KM_ROUTE_SYMMULTI : KM_ROUTE_GENERIC;
  ctx->km_route = route;
  switch (route) {
    case KM_ROUTE_COLW: return km_launch_colw(ctx, c);
    case KM_ROUTE_ESP:
      DFH_ARG(c.part_lo == 0 && c.part_hi == c.kd->n_parts && c.apply_outer);
      return km_launch_esp(ctx, c);
    case KM_ROUTE_SYM: return km_launch_sym(ctx, c);
    case KM_ROUTE_STRIP: return km_launch_strip(ctx, c);      // books KM_ROUTE_STRIP_MEAN where the mean rides along
    case KM_ROUTE_CROSS_LDS: return km_launch_cross_lds(ctx, c);
    case KM_ROUTE_SYMMULTI: return km_launch_symmulti(ctx, c);
    default: return km_launch_generic(ctx, c);
  }
}

int kernmat_gram(dfh_ctx* ctx, const KernDev& kd, int part_lo, int part_hi, bool apply_outer, KmPts pts, double diag_add,
                 double* K, int64_t ldk, bool lower_only) {
  return kernmat_dispatch(ctx, KmCall{&kd, part_lo, part_hi, apply_outer, pts, pts, true, diag_add, lower_only, K, ldk, nullptr});
}

int kernmat_cross(dfh_ctx* ctx, const KernDev& kd, int part_lo, int part_hi, bool apply_outer, KmPts pts1, KmPts pts2,
                  double* K, int64_t ldk, KmMean* mean, const double* col_w) {
  return kernmat_dispatch(ctx, KmCall{&kd, part_lo, part_hi, apply_outer, pts1, pts2, false, 0.0, false, K, ldk, mean, col_w});
}
