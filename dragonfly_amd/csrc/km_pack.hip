// Packed scaled inputs with their row norms (pack_scaled: what every kernel-matrix kernel reads), and the prior
// variance k(x, x) of packed points (prior_diag).
#include "kernmat.h"

namespace {

// ---- packing -----------------------------------------------------------------------------
__global__ void k_pack_cols(const double* __restrict__ X, long n, long ldx, int P, int c_lo, int c_hi,
                            const int* __restrict__ cols, const double* __restrict__ bw,
                            double* __restrict__ Xp, long sBlob, long sXp) {
  // batch element blockIdx.y: its kernel image sits sBlob bytes further, its output sXp doubles
  cols = reinterpret_cast<const int*>(reinterpret_cast<const char*>(cols) + (long)blockIdx.y * sBlob);
  bw = reinterpret_cast<const double*>(reinterpret_cast<const char*>(bw) + (long)blockIdx.y * sBlob);
  Xp += (long)blockIdx.y * sXp;
  const int w = c_hi - c_lo;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = n * w;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; idx < total; idx += stride) {
    const long row = idx / w;
    const int pc = c_lo + (int)(idx - row * w);
    const int c = cols[pc];
    // kernel.py:181 (X / bandwidths); a negative entry is a polynomial kernel's scaling: X * s (kernel.py:383)
    const double b = bw[pc];
    Xp[row * P + pc] = c >= 0 ? (b < 0.0 ? X[row * ldx + c] * -b : X[row * ldx + c] / b) : 0.0;
  }
}


__global__ void k_pack_norms(const double* __restrict__ Xp, long n, int P, int n_parts_total,
                             const PartDev* __restrict__ parts, const int* __restrict__ cols,
                             int part_lo, int part_hi, double* __restrict__ Np, long sBlob, long sXp,
                             long sNp) {
  parts = reinterpret_cast<const PartDev*>(reinterpret_cast<const char*>(parts) + (long)blockIdx.y * sBlob);
  cols = reinterpret_cast<const int*>(reinterpret_cast<const char*>(cols) + (long)blockIdx.y * sBlob);
  Xp += (long)blockIdx.y * sXp;
  Np += (long)blockIdx.y * sNp;
  const int np = part_hi - part_lo;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = n * np;
  if (idx >= total) return;
  const long row = idx / np;
  const int part = part_lo + (int)(idx - row * np);
  const PartDev pd = parts[part];
  int nreal = 0;
  for (int c = 0; c < pd.kc; ++c) nreal += cols[pd.poff + c] >= 0;   // padding is trailing
  Np[row * n_parts_total + part] = np_sumsq(Xp + row * P + pd.poff, nreal);
}

// Both passes in one launch (round 3: the Gram-matrix section of a fit is packing + norms + the Gram
// kernel, and at n = 16384 the two packing launches with the gaps around them were 3 - 4 % of it): a
// workgroup scales R rows, coalesced as k_pack_cols does, keeps the packed values in LDS and takes the
// norms from there -- the same operations in the same order, so Xp / Np are bit for bit what the two
// kernels above produce.
__global__ __launch_bounds__(256) void k_pack_fused(const double* __restrict__ X, long n, long ldx, int P, int c_lo, int c_hi,
                                                    const int* __restrict__ cols, const int* __restrict__ cols_all,
                                                    const double* __restrict__ bw, const PartDev* __restrict__ parts,
                                                    int part_lo, int part_hi, int n_parts_total, int R,
                                                    double* __restrict__ Xp, double* __restrict__ Np, long sBlob,
                                                    long sXp, long sNp) {
  extern __shared__ double pk[];               // [R][w]
  cols = reinterpret_cast<const int*>(reinterpret_cast<const char*>(cols) + (long)blockIdx.y * sBlob);
  cols_all = reinterpret_cast<const int*>(reinterpret_cast<const char*>(cols_all) + (long)blockIdx.y * sBlob);
  bw = reinterpret_cast<const double*>(reinterpret_cast<const char*>(bw) + (long)blockIdx.y * sBlob);
  parts = reinterpret_cast<const PartDev*>(reinterpret_cast<const char*>(parts) + (long)blockIdx.y * sBlob);
  Xp += (long)blockIdx.y * sXp;
  Np += (long)blockIdx.y * sNp;
  const int w = c_hi - c_lo;
  const long r0 = (long)blockIdx.x * R;
  const int rows = (int)((n - r0 < R) ? n - r0 : R);
  for (int idx = threadIdx.x; idx < rows * w; idx += blockDim.x) {
    const int lr = idx / w, pc = c_lo + (idx - lr * w);
    const long row = r0 + lr;
    const int c = cols[pc];
    const double b = bw[pc];
    const double v = c >= 0 ? (b < 0.0 ? X[row * ldx + c] * -b : X[row * ldx + c] / b) : 0.0;    // as k_pack_cols
    Xp[row * P + pc] = v;
    pk[idx] = v;
  }
  __syncthreads();
  const int np = part_hi - part_lo;
  for (int idx = threadIdx.x; idx < rows * np; idx += blockDim.x) {
    const int lr = idx / np, part = part_lo + (idx - lr * np);
    const PartDev pd = parts[part];
    int nreal = 0;
    for (int c = 0; c < pd.kc; ++c) nreal += cols_all[pd.poff + c] >= 0;   // padding is trailing
    Np[(r0 + lr) * n_parts_total + part] = np_sumsq(pk + lr * w + (pd.poff - c_lo), nreal);          // as k_pack_norms
  }
}

}  // namespace

int pack_scaled(dfh_ctx* ctx, const KernDev& kd, int part_lo, int part_hi, bool pre_gathered,
                const double* X, int64_t n, int64_t ldx, double* Xp, double* Np, int count,
                int64_t sBlob, int64_t sXp, int64_t sNp) {
  if (n <= 0 || count <= 0) return DFH_OK;
  DFH_ARG(part_lo >= 0 && part_hi <= kd.n_parts && part_lo < part_hi);
  DFH_ARG(!pre_gathered || part_hi == part_lo + 1);
  const int c_lo = kd.parts[part_lo].poff;
  const int c_hi = kd.parts[part_hi - 1].poff + kd.parts[part_hi - 1].kc;
  if (km_switches().pack_fused && c_hi - c_lo <= 2048) {
    const int w = c_hi - c_lo;
    int R = 4096 / w;                          // <= 32 KB of LDS
    R = R < 1 ? 1 : (R > 64 ? 64 : R);
    hipLaunchKernelGGL(k_pack_fused, dim3((unsigned)((n + R - 1) / R), (unsigned)count), dim3(256), (size_t)R * w * 8,
                       ctx->stream, X, (long)n, (long)ldx, kd.P, c_lo, c_hi, pre_gathered ? kd.d_lcols : kd.d_cols,
                       kd.d_cols, kd.d_bw, kd.d_parts, part_lo, part_hi, kd.n_parts, R, Xp, Np, (long)sBlob, (long)sXp,
                       (long)sNp);
    DFH_LAUNCH_CHECK();
    return DFH_OK;
  }
  const int64_t total = n * (c_hi - c_lo);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  // pre-gathered input: local column index c - poff ; d_lcols holds that mapping
  hipLaunchKernelGGL(k_pack_cols, dim3((unsigned)blocks, (unsigned)count), dim3(256), 0, ctx->stream, X, (long)n,
                     (long)ldx, kd.P, c_lo, c_hi, pre_gathered ? kd.d_lcols : kd.d_cols, kd.d_bw, Xp,
                     (long)sBlob, (long)sXp);
  DFH_LAUNCH_CHECK();
  const int64_t tn = n * (part_hi - part_lo);
  hipLaunchKernelGGL(k_pack_norms, dim3((unsigned)((tn + 255) / 256), (unsigned)count), dim3(256), 0, ctx->stream,
                     Xp, (long)n, kd.P, kd.n_parts, kd.d_parts, kd.d_cols, part_lo, part_hi, Np,
                     (long)sBlob, (long)sXp, (long)sNp);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

// k(x_i, x_i) for every packed point: what the diagonal of kernel(X, X) holds in the reference
// (gp_core.py:181 takes it from the full test Gram matrix).
__global__ void k_prior_diag(const PartDev* __restrict__ parts, int n_parts, int multi, int product, double outer,
                             const double* __restrict__ Xp, const double* __restrict__ Np, long m, int P,
                             double* __restrict__ out, int g_lo, int g_hi) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double res = (multi && product) ? outer : 0.0;
  double fsum = 0.0;
  for (int g = g_lo; g < g_hi; ++g) {
    const PartDev& pd = parts[g];
    double kv;
    if (pd.kind == DFH_KERNEL_POLY) kv = poly_eval(pd, Np[i * n_parts + g]);
    else if (pd.kind == DFH_KERNEL_EXPDECAY) kv = expdecay_eval(pd, Xp + i * P + pd.poff, Xp + i * P + pd.poff);
    else kv = pd.k0;
    if (!multi) res = kv;
    else if (!product) res = res + kv;
    else combine_nested(pd, kv, res, fsum);
  }
  if (multi && !product) res = outer * res;
  out[i] = res;
}

__global__ void k_fill_value(double* __restrict__ out, long m, double v) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] = v;
}

int prior_diag(dfh_ctx* ctx, const KernDev& kd, const double* Xp, const double* Np, int64_t m, double* out, int part_lo,
               int part_hi) {
  if (m <= 0) return DFH_OK;
  if (kd.esp) {                // stationary: every point's k(x, x) is kd.kxx (the recursion on the parts' k0)
    DFH_ARG(part_lo == 0 && (part_hi < 0 || part_hi == kd.n_parts));
    hipLaunchKernelGGL(k_fill_value, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, out, (long)m, kd.kxx);
    DFH_LAUNCH_CHECK();
    return DFH_OK;
  }
  if (part_hi < 0) { part_lo = 0; part_hi = kd.n_parts; }
  hipLaunchKernelGGL(k_prior_diag, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, kd.d_parts,
                     kd.n_parts, kd.multi ? 1 : 0, kd.product ? 1 : 0, kd.outer_scale, Xp, Np, (long)m, kd.P, out, part_lo,
                     part_hi);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}
