// What the units of the tuning objective share -- lml.hip (the entry, its route chooser and the two schedules), lml_tiny.hip
// (the one-launch small-problem kernels) and lml_wg.h (one workgroup or a team per candidate, compiled inside chol.hip):
// the size limits of the routes, the one call as the entry hands it on, the staging blob and result words of the
// one-launch forms, and the launchers.  Internal: common.h declares what the rest of the library calls.
#pragma once
#include "common.h"

#pragma GCC visibility push(hidden)      // what the units share: none of it joins the library's exported symbols

// ---- the limits lml_route (lml.hip) chooses by; LMLWG_MAX_N, which mgpu.hip reads too, is in common.h ----
constexpr int64_t TINY_MAX_N = 128;       // k_lml_tiny: the whole system of a candidate in LDS
constexpr int64_t TINY64_MAX_N = 63;      // k_lml_tiny64: the system (n + 1 rows) is one 64 x 64 tile
constexpr int TINY_MAX_P = 64, TINY_MAX_PARTS = 16;
// lml_wgf_kernel takes TINY64_MAX_N < n <= LMLF_KERNEL_MAX_N; by default the route stops at LMLF_MAX_N (beyond, the team
// schedule -- one copy up, one memset, one copy back per group -- is as fast: 101 us at n = 129 .. 191 against the one
// workgroup's 105 .. 143; DFH_LML_FUSED_MAX_N moves the limit, and the kernel is tested up to 255 through it)
constexpr int64_t LMLF_MAX_N = 128, LMLF_KERNEL_MAX_N = 255;
constexpr int LMLT_SYNC_INTS = 64;        // flags of a team, per candidate (lml_wg.h: diag[j], then brow[j])

// the arguments of dfh_gp_lml_batch, X resolved to the device and the host descriptors built (kds[c] of descs[c]; the
// schedules point them at the device images they upload); cand_base: index of descs[0] in the caller's list (error messages)
struct LmlCall {
  dfh_ctx* ctx; const dfh_kernel_desc* descs; KernDev* kds; int32_t nb; const double* dX; int64_t n, d; const double* y;
  const double* mean_consts; const double* noise_vars; int flags; double* lml_out; int32_t* jitter_powers;
  int cand_base;
};

// what the one-launch forms evaluate in LDS: SE / Matern parts (no ESP) within the packed width and part count they hold
inline bool lml_one_launch_kernels(const KernDev* kds, int count) {
  for (int c = 0; c < count; ++c)
    if (kds[c].P > TINY_MAX_P || kds[c].n_parts > TINY_MAX_PARTS || kds[c].P < 1 || !kds[c].stationary || kds[c].esp) return false;
  return true;
}

// ---- lml_tiny.hip ----
// The blob of a one-launch tuning call in the context's pinned (mapped, coherent) buffer:
// TinyCand[count] | kernel images | y[n] | 10^-11 .. 10^4 | (64-byte aligned) results [count][4]
struct TinyBlob {
  char* host = nullptr; size_t bytes = 0, y_off = 0, pow_off = 0;
  double* res = nullptr;
  int Pmax = 1, parts_max = 1;
};
int tiny_blob_build(dfh_ctx* ctx, const KernDev* kds, int count, int64_t n, const double* y_host,
                    const double* noise_vars, const double* mean_consts, TinyBlob* tb);
// A launch that writes its results straight into the pinned buffer, status word (res[4 c + 3]: 0, 1 or 2) last: armed
// before the launch ("not there yet"), polled after it -- no copy, no stream synchronisation
void tiny_arm_results(volatile double* vres, int count);
int tiny_poll_results(dfh_ctx* ctx, volatile double* vres, int count, const char* what);
// k_lml_tiny / k_lml_tiny64, n <= TINY_MAX_N: logdet_dot[2c], [2c+1] = sum(log(diag(L_c))), |L_c^-1 (y - m_c)|^2 with the
// stable_cholesky ladder inside the kernel; powers[c] = jitter power used (INT32_MIN: none)
int lml_tiny_batch(dfh_ctx* ctx, const KernDev* kds, int count, const double* dX, int64_t n, int64_t ldx,
                   const double* y_host, const double* noise_vars, const double* mean_consts,
                   bool allow_jitter, double* logdet_dot, int32_t* powers);

// ---- lml_wg.h ----
// lml_wgf_kernel, a handful of candidates at TINY64_MAX_N < n <= LMLF_KERNEL_MAX_N: Gram matrix, factorisation and
// forward solve of each in ONE launch by one workgroup, descriptors and results through the pinned buffer.
// info[c]: 0 = logdet_dot[2c], [2c+1] are valid; otherwise the candidate is for the lock-step schedule (a failed pivot:
// the ladder; no noise: nothing bounds the augmented pivot).
struct LmlFusedLimits { int max_count; int64_t max_n; };   // DFH_LML_FUSED (0: off), DFH_LML_FUSED_MAX_N
LmlFusedLimits lml_fused_limits();
bool lml_fused_fits_lds(const KernDev* kds, int count, int64_t n);     // the packed inputs beside the factorisation's images
int lml_wg_fused_batch(dfh_ctx* ctx, const KernDev* kds, int count, const double* dX, int64_t n, int64_t ldx,
                       const double* y_host, const double* noise_vars, const double* mean_consts,
                       double* logdet_dot, long long* info);
// lml_wg_kernel / lml_team_kernel, n <= LMLWG_MAX_N: Cholesky of the augmented matrix [[K, .], [(y - m)^T, c]] of each of
// `count` candidates, sum(log L_ii) and |L^-1 (y - m)|^2 out.  K: matrices padded to order 64 * ceil((n + 1) / 64) (only the
// n x n part has to be filled), sK doubles apart, row stride ld.  team > 1: that many workgroups per candidate (for
// groups far smaller than the device); *d_status != 0 afterwards means a hand-off between them timed out and the launch's
// results are void (repeat with team = 1).  d_info, d_status and d_sync ([count][LMLT_SYNC_INTS]) are zeroed by the caller.
int lml_wg_batch(dfh_ctx* ctx, double* K, int64_t sK, int64_t ld, int64_t n, int count, const double* d_y,
                 const double* d_par, double* d_out2, long long* d_info, int team, unsigned long long* d_status, int* d_sync);

#pragma GCC visibility pop
