// What the units of the kernel-matrix builder share: one request as the dispatcher (kernmat.hip) hands it to a kernel
// family's launcher, the switches, the route predicates and launchers of the families (km_generic.hip, km_sym.hip,
// km_strip.hip, km_esp.hip), and -- in the including unit's anonymous namespace, with kerneval.h -- the argument block
// the kernels take and the one function that fills it.  Internal: common.h declares what the rest of the library calls.
#pragma once
#include "common.h"

#pragma GCC visibility push(hidden)      // what the units share: none of it joins the library's exported symbols

// One kernel matrix: K[a.n x b.n] (ldk) of parts [part_lo, part_hi) of kd between the packed points a (rows) and b (columns).
struct KmCall {
  const KernDev* kd;
  int part_lo, part_hi;
  bool apply_outer;
  KmPts a, b;
  bool symmetric;              // b is a, and diag_add goes on the diagonal
  double diag_add;
  bool lower_only;             // (symmetric) the tiles on and below the diagonal only
  double* K; int64_t ldk;
  KmMean* mean;                // (cross) the product with a vector is wanted from the same pass, or null
  const double* col_w = nullptr;   // (cross, one stationary part) K[a][i] = col_w[i] * k_part(a, i): the part alone, no outer scale
};

// The route a call took, as dfh_ctx_counters reports it (out[2]; 0: no call yet).  Booked on the host by the dispatcher;
// km_launch_strip books KM_ROUTE_STRIP_MEAN where the posterior mean rode along.
enum KmRoute {
  KM_ROUTE_SYM = 1, KM_ROUTE_CROSS_LDS, KM_ROUTE_STRIP, KM_ROUTE_STRIP_MEAN, KM_ROUTE_SYMMULTI, KM_ROUTE_GENERIC, KM_ROUTE_ESP,
  KM_ROUTE_COLW
};

// DFH_KM_* / DFH_PACK_FUSED, read once per process
struct KmSwitches {
  int nt = env_int("DFH_KM_NT", -1);                        // streaming stores of kernmat_sym_kernel: < 0 = by size (km_args)
  int sym_cfg = env_int("DFH_KM_CFG", 0);                   // tile configuration of the symmetric single-part kernel (km_sym.hip)
  bool strip = env_flag("DFH_KM_STRIP", true);              // cross matrices by the strip kernel where it applies
  bool fused_mean = env_flag("DFH_KM_FUSED_MEAN", true);    // ... with the posterior mean riding along
  bool symmulti = env_flag("DFH_KM_SYMMULTI", true);        // symmetric multi-part matrices by kernmat_symmulti_kernel
  long waves = env_long("DFH_KM_WAVES", 8192);              // waves the strip kernel's grid aims at
  bool pack_fused = env_flag("DFH_PACK_FUSED", true);       // scaling and norms in one launch (km_pack.hip)
};

const KmSwitches& km_switches();                            // kernmat.hip
// km_sym.hip: one part, even ldk, 16-byte aligned K -- kernmat_sym_kernel (symmetric, or a cross matrix the strip kernel
// does not take); a symmetric matrix of adjacent narrow stationary parts -- kernmat_symmulti_kernel
bool km_single_aligned(const KmCall& c);
int km_launch_sym(dfh_ctx* ctx, const KmCall& c);
int km_launch_cross_lds(dfh_ctx* ctx, const KmCall& c);
bool km_symmulti_ok(const KmCall& c);
int km_launch_symmulti(dfh_ctx* ctx, const KmCall& c);
// km_strip.hip: cross matrix of a single-part aligned call (km_single_aligned), SE / Matern of packed width 8 .. 32
bool km_strip_ok(const KmCall& c);
int km_launch_strip(dfh_ctx* ctx, const KmCall& c);         // sets c.mean->done where the mean rode along
// km_esp.hip, km_generic.hip: every call of an ESP kernel; whatever no other route takes
int km_launch_esp(dfh_ctx* ctx, const KmCall& c);
int km_launch_generic(dfh_ctx* ctx, const KmCall& c);
int km_launch_colw(dfh_ctx* ctx, const KmCall& c);          // km_generic.hip: a call with col_w
#pragma GCC visibility pop

namespace {

constexpr int KM_BM = 128;
constexpr int KM_KC = 32;          // packed columns per LDS chunk
constexpr int KM_KP = 34;          // LDS row stride (doubles); 34 = 2 mod 32 -> conflict-free b64 frag reads

#include "kerneval.h"   // ExpConsts, exp_fast, kern_eval, combine_nested, np_sumsq, TinyCand

struct KmArgs {
  ExpConsts ec;
  const double* Xp1; const double* Np1;
  const double* Xp2; const double* Np2;
  int n1, n2, P, n_parts_total;
  const PartDev* parts;
  int part_lo, part_hi;
  double outer;
  int apply_outer, symmetric;
  int product;                 // MULTI: parts are multiplied (CoordinateProductKernel) instead of summed
  int nt_stores;               // kernmat_sym_kernel: write the matrix with streaming stores
  int lower_only;              // kernmat_sym_kernel: tiles of the lower triangle only, no mirror images (the fit path: the factorisation reads nothing else)
  double diag_add;
  double* K; long ldk;
  // lock-step batch over blockIdx.z (symmetric single-part kernel only): element strides of the
  // packed inputs / output, byte stride between the device images of the kernels, one diagonal
  // term per batch element (NULL: diag_add)
  long sXp, sNp, sK, sBlob;
  const double* diag_adds;
  // strip kernel with the posterior mean fused in: mu_part[row][blk] = sum over the columns of block
  // blk (KM_MU_BLOCK columns) of K[row][col] * mu_alpha[col]
  const double* mu_alpha;
  double* mu_part;
  double* mu_out;
  int mu_nblk;
};
constexpr int KM_MU_BLOCK = 512;

// The one place a KmArgs is filled, every field: a single matrix (no batch strides), no fused mean.
inline KmArgs km_args(const KmCall& c) {
  const KernDev& kd = *c.kd;
  KmArgs a;
  a.ec = kExpConsts;
  a.Xp1 = c.a.Xp; a.Np1 = c.a.Np; a.Xp2 = c.b.Xp; a.Np2 = c.b.Np;
  a.n1 = (int)c.a.n; a.n2 = (int)c.b.n; a.P = kd.P; a.n_parts_total = kd.n_parts;
  a.parts = kd.d_parts; a.part_lo = c.part_lo; a.part_hi = c.part_hi;
  a.outer = kd.outer_scale; a.apply_outer = c.apply_outer ? 1 : 0; a.symmetric = c.symmetric ? 1 : 0;
  a.product = kd.product ? 1 : 0;
  const int nt = km_switches().nt;
  a.nt_stores = nt >= 0 ? (nt != 0) : (kd.P >= 16 && c.a.n * c.b.n >= (int64_t)4096 * 4096);
  a.lower_only = (c.symmetric && c.lower_only) ? 1 : 0;
  a.diag_add = c.diag_add;
  a.K = c.K; a.ldk = c.ldk;
  a.sXp = a.sNp = a.sK = a.sBlob = 0; a.diag_adds = nullptr;
  a.mu_alpha = nullptr; a.mu_part = nullptr; a.mu_out = nullptr; a.mu_nblk = 0;
  return a;
}

}  // namespace
