// Kernel matrices, the generic kernel: any part kinds, symmetric or cross, any leading dimension -- whatever no other
// route of kernmat.hip takes.  128 x 128 output tiles for a single part, 128 x 64 for several.
#include "kernmat.h"

namespace {

// NS: the parts may be polynomial / exponential-decay kernels (an instance of its own: their pow()
// calls cost the stationary multi-part kernel its registers).  NESTED (with NS): a product kernel
// with additive factors.  HAM (with MULTI): the parts may also be Hamming kernels (a product with a Hamming factor is
// the reference's CartesianProductKernel, kernel.py:504-538) -- instances of their own again, so that the kernels of
// every description without a Hamming part stay what they were.  A Hamming part is a code region of its own ahead of
// the dot-product accumulators: compares and selects on its columns in the operand tiles, no MFMA and no exponential,
// and the matrix is still one launch.  The instance without the polynomial / exponential-decay branches (NS false:
// SE / Matern x Hamming, Hamming alone) has no scratch; the two with them carry the call frame of pow() as their twins
// without Hamming do (profiles/cp_kernel_resource_usage.txt).
template <int TJ, bool MULTI, bool NS = false, bool NESTED = false, bool HAM = false>
__global__ __launch_bounds__(256, 2) void kernmat_kernel(KmArgs p) {
  constexpr int BN = 2 * TJ * 16;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* As = smem;                           // [128][KM_KP]
  double* Bs = As + KM_BM * KM_KP;             // [BN][KM_KP]
  double* na = Bs + BN * KM_KP;                // [128]
  double* nb = na + KM_BM;                     // [BN]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  const long m0 = (long)blockIdx.y * KM_BM, n0 = (long)blockIdx.x * BN;

  double4_t res[4][TJ];
  double4_t fsum[NESTED ? 4 : 1][NESTED ? TJ : 1];
  if (MULTI) {
    // additive: 0 + k_1 + k_2 ...; product: scale * k_1 * k_2 ... in the reference's order
    // (kernel.py:584-588: K = scale * ones; K *= kernel(...))
    const double r0 = p.product ? p.outer : 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) res[i][j] = (double4_t){r0, r0, r0, r0};
  }
  if (NESTED) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) fsum[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  }

  // the Hamming columns' weights: a section of the kernel's device image (uniform scalar loads like the parts)
  const double* hw = HAM ? reinterpret_cast<const double*>(reinterpret_cast<const char*>(p.parts) + blob_hw_offset(p.n_parts_total, p.P))
                         : nullptr;
  for (int part = p.part_lo; part < p.part_hi; ++part) {
    const PartDev& pd = p.parts[part];          // stays in global memory: uniform scalar loads
    if (HAM && pd.kind == DFH_KERNEL_HAMMING) {      // (uniform)
      // A region of its own, before the accumulators of the dot products exist: the part's columns (kc <= KM_KC: one
      // chunk) go to the operand tiles as below, and sum_c w_c [x_c == y_c] is taken there for the TJ entries this
      // lane holds of a row, a row at a time (the barrier), so that the temporaries stay a row's beside res.
      const int kh = pd.kc >> 1;
      __syncthreads();
      for (int idx = tid; idx < KM_BM * kh; idx += 256) {
        const int r = idx / kh, c2 = (idx - r * kh) * 2;
        const long row = m0 + r;
        double2_t v = (double2_t){0.0, 0.0};
        if (row < p.n1) v = *reinterpret_cast<const double2_t*>(p.Xp1 + row * p.P + pd.poff + c2);
        *reinterpret_cast<double2_t*>(As + r * KM_KP + c2) = v;
      }
      for (int idx = tid; idx < BN * kh; idx += 256) {
        const int r = idx / kh, c2 = (idx - r * kh) * 2;
        const long row = n0 + r;
        double2_t v = (double2_t){0.0, 0.0};
        if (row < p.n2) v = *reinterpret_cast<const double2_t*>(p.Xp2 + row * p.P + pd.poff + c2);
        *reinterpret_cast<double2_t*>(Bs + r * KM_KP + c2) = v;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lr = wm * 64 + i * 16 + l4 + 4 * r;
          double hk[1][TJ];
          hamming_eval<1, TJ>(hw + pd.poff, pd.p, As + lr * KM_KP, 0, Bs + (wn * TJ * 16 + l15) * KM_KP, 16 * KM_KP, hk);
#pragma unroll
          for (int j = 0; j < TJ; ++j) {
            const double kv = hk[0][j];
            if (NESTED) {
              double rr = res[i][j][r], ff = fsum[i][j][r];
              combine_nested(pd, kv, rr, ff);
              res[i][j][r] = rr; fsum[i][j][r] = ff;
            } else {
              res[i][j][r] = p.product ? res[i][j][r] * kv : res[i][j][r] + kv;
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      continue;
    }
    double4_t acc[4][TJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

    for (int k0 = 0; k0 < pd.kc; k0 += KM_KC) {
      const int kc = min(KM_KC, pd.kc - k0);     // multiple of 4
      const int kh = kc >> 1;                    // double2 per row
      __syncthreads();                           // previous readers of As/Bs/na/nb are done
      for (int idx = tid; idx < KM_BM * kh; idx += 256) {
        const int r = idx / kh, c2 = (idx - r * kh) * 2;
        const long row = m0 + r;
        double2_t v = (double2_t){0.0, 0.0};
        if (row < p.n1) v = *reinterpret_cast<const double2_t*>(p.Xp1 + row * p.P + pd.poff + k0 + c2);
        *reinterpret_cast<double2_t*>(As + r * KM_KP + c2) = v;
      }
      for (int idx = tid; idx < BN * kh; idx += 256) {
        const int r = idx / kh, c2 = (idx - r * kh) * 2;
        const long row = n0 + r;
        double2_t v = (double2_t){0.0, 0.0};
        if (row < p.n2) v = *reinterpret_cast<const double2_t*>(p.Xp2 + row * p.P + pd.poff + k0 + c2);
        *reinterpret_cast<double2_t*>(Bs + r * KM_KP + c2) = v;
      }
      if (k0 == 0) {
        if (tid < KM_BM) {
          const long row = m0 + tid;
          na[tid] = row < p.n1 ? p.Np1[row * p.n_parts_total + part] : 0.0;
        } else if (tid - KM_BM < BN) {
          const long row = n0 + tid - KM_BM;
          nb[tid - KM_BM] = row < p.n2 ? p.Np2[row * p.n_parts_total + part] : 0.0;
        }
      }
      __syncthreads();
      const double* as = As + (wm * 64 + l15) * KM_KP + l4;
      const double* bs = Bs + (wn * TJ * 16 + l15) * KM_KP + l4;
      for (int kk = 0; kk < kc; kk += 4) {
        double a[4], b[TJ];
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = as[t * 16 * KM_KP + kk];
#pragma unroll
        for (int t = 0; t < TJ; ++t) b[t] = bs[t * 16 * KM_KP + kk];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }

    // distances -> kernel values for this part
    const ExpConsts& ec = p.ec;                  // kernel arguments: scalar loads, SGPR-resident
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wm * 64 + i * 16 + l4 + 4 * r;
        const double nai = na[lr];
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          const int lc = wn * TJ * 16 + j * 16 + l15;
          double kv;
          if (NS && pd.kind == DFH_KERNEL_POLY) {
            kv = poly_eval(pd, acc[i][j][r]);
          } else if (NS && pd.kind == DFH_KERNEL_EXPDECAY) {
            // the part's columns (kc <= KM_KC: one chunk) are still in the operand tiles
            kv = expdecay_eval(pd, As + lr * KM_KP, Bs + lc * KM_KP);
          } else {
            double dsq = (nb[lc] + nai) - 2.0 * acc[i][j][r];     // general_utils.py:66-68
            dsq = dsq < 0.0 ? 0.0 : dsq;                           // np.clip(.,0,inf), NaN kept
            kv = kern_eval(pd, dsq, ec);
          }
          if (NESTED) {
            double rr = res[i][j][r], ff = fsum[i][j][r];
            combine_nested(pd, kv, rr, ff);
            res[i][j][r] = rr; fsum[i][j][r] = ff;
          } else if (MULTI) {
            res[i][j][r] = p.product ? res[i][j][r] * kv : res[i][j][r] + kv;   // kernel.py:493 / :588
          } else {
            acc[i][j][r] = kv;
          }
        }
      }
    }
    if (!MULTI) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) res[i][j] = acc[i][j];
    }
  }

  // store
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long row = m0 + wm * 64 + i * 16 + l4 + 4 * r;
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const long col = n0 + wn * TJ * 16 + j * 16 + l15;
        if (row < p.n1 && col < p.n2) {
          double v = res[i][j][r];
          if (MULTI && p.apply_outer && !p.product) v = p.outer * v;   // kernel.py:494
          if (p.symmetric && row == col) v += p.diag_add;         // gp_core.py:843
          p.K[row * p.ldk + col] = v;
        }
      }
    }
  }
}

// One SE / Matern part on its own with a weight per column: K[a][i] = col_w[i] * k_part(a, i), no outer scale and no
// other part -- the cross matrix of one group of a multi-fidelity GP's additive domain model at a fixed fidelity, where
// col_w[i] = kern_scale * k_fid(z*, Z_i) (opt/gpb_acquisitions.py:364-366; gp_mf.hip).  The single-part path of
// kernmat_kernel<4, false> -- its 128 x 128 tile, operand staging, distance expansion and kern_eval -- with one load and one
// multiplication more per element, right before the store, so that no m x n scaling pass reads and writes the matrix
// again ahead of the solve.  A kernel of its own: kernmat_kernel's instances stay the code objects they were.
__global__ __launch_bounds__(256, 2) void kernmat_colw_kernel(KmArgs p, const double* __restrict__ col_w) {
  constexpr int TJ = 4, BN = 2 * TJ * 16;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* As = smem;                           // [128][KM_KP]
  double* Bs = As + KM_BM * KM_KP;             // [BN][KM_KP]
  double* na = Bs + BN * KM_KP;                // [128]
  double* nb = na + KM_BM;                     // [BN]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  const long m0 = (long)blockIdx.y * KM_BM, n0 = (long)blockIdx.x * BN;
  const int part = p.part_lo;
  const PartDev& pd = p.parts[part];            // stays in global memory: uniform scalar loads

  double4_t acc[4][TJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < pd.kc; k0 += KM_KC) {
    const int kc = min(KM_KC, pd.kc - k0);     // multiple of 4
    const int kh = kc >> 1;                    // double2 per row
    __syncthreads();                           // previous readers of As/Bs are done
    for (int idx = tid; idx < KM_BM * kh; idx += 256) {
      const int r = idx / kh, c2 = (idx - r * kh) * 2;
      const long row = m0 + r;
      double2_t v = (double2_t){0.0, 0.0};
      if (row < p.n1) v = *reinterpret_cast<const double2_t*>(p.Xp1 + row * p.P + pd.poff + k0 + c2);
      *reinterpret_cast<double2_t*>(As + r * KM_KP + c2) = v;
    }
    for (int idx = tid; idx < BN * kh; idx += 256) {
      const int r = idx / kh, c2 = (idx - r * kh) * 2;
      const long row = n0 + r;
      double2_t v = (double2_t){0.0, 0.0};
      if (row < p.n2) v = *reinterpret_cast<const double2_t*>(p.Xp2 + row * p.P + pd.poff + k0 + c2);
      *reinterpret_cast<double2_t*>(Bs + r * KM_KP + c2) = v;
    }
    if (k0 == 0) {
      if (tid < KM_BM) {
        const long row = m0 + tid;
        na[tid] = row < p.n1 ? p.Np1[row * p.n_parts_total + part] : 0.0;
      } else {
        const long row = n0 + tid - KM_BM;
        nb[tid - KM_BM] = row < p.n2 ? p.Np2[row * p.n_parts_total + part] : 0.0;
      }
    }
    __syncthreads();
    const double* as = As + (wm * 64 + l15) * KM_KP + l4;
    const double* bs = Bs + (wn * TJ * 16 + l15) * KM_KP + l4;
    for (int kk = 0; kk < kc; kk += 4) {
      double a[4], b[TJ];
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] = as[t * 16 * KM_KP + kk];
#pragma unroll
      for (int t = 0; t < TJ; ++t) b[t] = bs[t * 16 * KM_KP + kk];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  const ExpConsts& ec = p.ec;                  // kernel arguments: scalar loads, SGPR-resident
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int lc = wn * TJ * 16 + j * 16 + l15;
    const long col = n0 + lc;
    if (col >= p.n2) continue;
    const double w = col_w[col], nbj = nb[lc];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wm * 64 + i * 16 + l4 + 4 * r;
        const long row = m0 + lr;
        double dsq = (nbj + na[lr]) - 2.0 * acc[i][j][r];       // general_utils.py:66-68
        dsq = dsq < 0.0 ? 0.0 : dsq;                             // np.clip(.,0,inf), NaN kept
        if (row < p.n1) p.K[row * p.ldk + col] = w * kern_eval(pd, dsq, ec);
      }
    }
  }
}

using KmKernel = void (*)(KmArgs);
constexpr int SM4 = ((KM_BM + 128) * KM_KP + KM_BM + 128) * 8;
constexpr int SM2 = ((KM_BM + 64) * KM_KP + KM_BM + 64) * 8;

// Which instance knows every part of the kernel: the single-part one, or one of the six multi-part ones.
KmKernel generic_instance(const KernDev& kd) {
  if (!kd.multi) return kernmat_kernel<4, false>;
  bool ham_pow = false;       // a Hamming part next to a polynomial / exponential-decay one: the instance with their pow()
  for (const PartDev& pd : kd.parts) ham_pow = ham_pow || pd.kind == DFH_KERNEL_POLY || pd.kind == DFH_KERNEL_EXPDECAY;
  if (kd.hamming && kd.nested) return kernmat_kernel<2, true, true, true, true>;
  if (kd.hamming && ham_pow) return kernmat_kernel<2, true, true, false, true>;
  if (kd.hamming) return kernmat_kernel<2, true, false, false, true>;
  if (kd.nested) return kernmat_kernel<2, true, true, true>;
  if (kd.stationary) return kernmat_kernel<2, true>;
  return kernmat_kernel<2, true, true>;
}

// every instance needs more than the default 64 KiB of dynamic LDS allowed: once per device
int set_lds_limits(dfh_ctx* ctx) {
  static bool attr_set_dev[DFH_MAX_DEVICES] = {false};
  bool& attr_set = attr_set_dev[ctx->device];
  if (attr_set) return DFH_OK;
  DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_kernel<4, false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, SM4));
  const KmKernel multi[6] = {kernmat_kernel<2, true>, kernmat_kernel<2, true, true>, kernmat_kernel<2, true, true, true>,
                             kernmat_kernel<2, true, false, false, true>, kernmat_kernel<2, true, true, false, true>,
                             kernmat_kernel<2, true, true, true, true>};
  for (KmKernel fn : multi)
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, SM2));
  DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_colw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              SM4));
  attr_set = true;
  return DFH_OK;
}

}  // namespace

int km_launch_generic(dfh_ctx* ctx, const KmCall& c) {
  DFH_TRY(set_lds_limits(ctx));
  const KernDev& kd = *c.kd;
  const KmArgs a = km_args(c);
  const KmKernel fn = generic_instance(kd);
  const int64_t n1 = c.a.n, n2 = c.b.n;
  const int bn = kd.multi ? 64 : 128, smem = kd.multi ? SM2 : SM4;
  const int64_t rows_per_launch = 65535LL * KM_BM;
  for (int64_t r0 = 0; r0 < n1; r0 += rows_per_launch) {
    const int64_t rr = n1 - r0 < rows_per_launch ? n1 - r0 : rows_per_launch;
    KmArgs b = a;
    b.Xp1 = a.Xp1 + r0 * kd.P; b.Np1 = a.Np1 + r0 * kd.n_parts; b.n1 = (int)rr; b.K = a.K + r0 * a.ldk;
    if (r0 != 0) b.symmetric = 0;    // only reachable for n1 > 8M rows; diagonal handled in slab 0
    dim3 grid((unsigned)((n2 + bn - 1) / bn), (unsigned)((rr + KM_BM - 1) / KM_BM));
    hipLaunchKernelGGL(fn, grid, dim3(256), smem, ctx->stream, b);
    DFH_LAUNCH_CHECK();
  }
  return DFH_OK;
}

// A weighted cross matrix (KmCall::col_w): one stationary part of any kernel, alone
int km_launch_colw(dfh_ctx* ctx, const KmCall& c) {
  DFH_ARG(c.col_w && !c.symmetric && !c.kd->esp && c.part_hi == c.part_lo + 1 && part_is_stationary(*c.kd, c.part_lo));
  DFH_ARG((c.a.n + KM_BM - 1) / KM_BM <= 65535 && c.kd->P % 2 == 0 && c.kd->parts[c.part_lo].poff % 2 == 0);
  DFH_TRY(set_lds_limits(ctx));
  const KmArgs a = km_args(c);
  dim3 grid((unsigned)((c.b.n + 127) / 128), (unsigned)((c.a.n + KM_BM - 1) / KM_BM));
  hipLaunchKernelGGL(kernmat_colw_kernel, grid, dim3(256), SM4, ctx->stream, a, c.col_w);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}
