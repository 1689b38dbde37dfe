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
#include "common.h"
#include <cstring>
#include <math.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>

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

// Symmetric Gram matrix K(X, X) + diag_add I, single-part kernels: only the tiles on and below the
// diagonal are computed; each off-diagonal tile is written twice, as itself and transposed into its
// mirror position.  Both images go through an LDS staging buffer so that every global store is a
// full 16-byte-per-lane row segment (the natural MFMA accumulator layout only offers 8-byte stores
// in 128-byte segments, and none at all for the transposed image).
// TS = tile edge: 64 (2x2 MFMA tiles per wave, ~35 KB LDS, 4 workgroups per CU -- the phases
// load / MFMA / exp / store of different workgroups overlap) or 128.
template <int TS, int KC, int SR, int OCC, bool SYM>
__global__ __launch_bounds__(256, OCC) void kernmat_sym_kernel(KmArgs p) {
  constexpr int WT = TS / 32;            // MFMA tiles per wave per dimension
  constexpr int WS = TS / 2;             // wave tile edge
  constexpr int SP = TS + 2;             // staging row stride (doubles): 16-byte aligned rows
  constexpr int NH = TS / SR;            // SR-row staging passes per image
  constexpr int KP = KC + 2;             // operand row stride: = 2 (mod 32) for KC = 32, 18 for KC = 16
  constexpr int OPER = 2 * TS * KP;      // doubles of the two operand tiles
  constexpr int STAGE = SR * SP;
  constexpr int BODY = (OPER > STAGE) ? OPER : STAGE;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* As = smem;                     // [TS][KP]
  double* Bs = As + TS * KP;             // [TS][KP]
  double* na = smem + BODY;              // [TS]
  double* nb = na + TS;                  // [TS]
  double* St = smem;                     // [SR][SP] staging, reuses the operand tiles

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  unsigned ti, tj;
  if (SYM) {                              // lower-triangular tile enumeration
    const unsigned lin = blockIdx.x;
    ti = (unsigned)((sqrt(8.0 * (double)lin + 1.0) - 1.0) * 0.5);
    while ((unsigned long long)ti * (ti + 1) / 2 > lin) --ti;
    while ((unsigned long long)(ti + 1) * (ti + 2) / 2 <= lin) ++ti;
    tj = lin - (unsigned)((unsigned long long)ti * (ti + 1) / 2);
  } else {                                // cross matrix: plain 2-D grid
    ti = blockIdx.y; tj = blockIdx.x;
  }
  const long m0 = (long)ti * TS, n0 = (long)tj * TS;
  const long bz = SYM ? (long)blockIdx.z : 0;       // batch element (strides are 0 for a single matrix)
  const PartDev& pd = reinterpret_cast<const PartDev*>(reinterpret_cast<const char*>(p.parts) + bz * p.sBlob)[p.part_lo];
  const double* __restrict__ XpA = p.Xp1 + bz * p.sXp;
  const double* __restrict__ NpA = p.Np1 + bz * p.sNp;
  double* __restrict__ Kout = p.K + bz * p.sK;
  const double diag_add = p.diag_adds ? p.diag_adds[bz] : p.diag_add;
  const double* __restrict__ XpB = SYM ? XpA : p.Xp2;
  const double* __restrict__ NpB = SYM ? NpA : p.Np2;
  const long nB = SYM ? p.n1 : p.n2;

  double4_t acc[WT][WT];
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < pd.kc; k0 += KC) {
    const int kc = min(KC, pd.kc - k0);
    const int kh = kc >> 1;
    __syncthreads();
    for (int idx = tid; idx < TS * kh; idx += 256) {
      const int r = idx / kh, c2 = (idx - r * kh) * 2;
      const long rowa = m0 + r, rowb = n0 + r;
      double2_t va = (double2_t){0.0, 0.0}, vb = (double2_t){0.0, 0.0};
      if (rowa < p.n1) va = *reinterpret_cast<const double2_t*>(XpA + rowa * p.P + pd.poff + k0 + c2);
      if (rowb < nB) vb = *reinterpret_cast<const double2_t*>(XpB + rowb * p.P + pd.poff + k0 + c2);
      *reinterpret_cast<double2_t*>(As + r * KP + c2) = va;
      *reinterpret_cast<double2_t*>(Bs + r * KP + c2) = vb;
    }
    if (k0 == 0) {
      if (tid < TS) {
        const long row = m0 + tid;
        na[tid] = row < p.n1 ? NpA[row * p.n_parts_total + p.part_lo] : 0.0;
      } else if (tid - TS < TS) {
        const long row = n0 + tid - TS;
        nb[tid - TS] = row < nB ? NpB[row * p.n_parts_total + p.part_lo] : 0.0;
      }
    }
    __syncthreads();
    const double* as = As + (wm * WS + l15) * KP + l4;
    const double* bs = Bs + (wn * WS + l15) * KP + l4;
    for (int kk = 0; kk < kc; kk += 4) {
      double a[WT], b[WT];
#pragma unroll
      for (int t = 0; t < WT; ++t) a[t] = as[t * 16 * KP + kk];
#pragma unroll
      for (int t = 0; t < WT; ++t) b[t] = bs[t * 16 * KP + kk];
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // distances -> kernel values (in the accumulator registers).  SE: -dsq/2 is formed directly as
  // acc - (na/2 + nb/2): scaling by powers of two commutes with rounding, so this is bit-identical
  // to ((nb + na) - 2 acc) clipped at 0 and then halved and negated (general_utils.py:66-69,
  // kernel.py:176).  The diagonal term only exists in diagonal tiles.
  const bool se = (pd.kind == DFH_KERNEL_SE);
  const bool diag_tile = SYM && (ti == tj);
  const ExpConsts& ec = p.ec;                    // kernel arguments: scalar loads, SGPR-resident
#pragma unroll
  for (int i = 0; i < WT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = wm * WS + i * 16 + l4 + 4 * r;
      const double nai = na[lr];
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        const int lc = wn * WS + j * 16 + l15;
        double kv;
        if (se) {
          double t = acc[i][j][r] - (0.5 * nb[lc] + 0.5 * nai);
          t = t > 0.0 ? 0.0 : t;
          kv = pd.scale_c * exp_fast_neg(t, ec);       // t <= 0: no exponent clamp needed (two VALU ops of ~26)
        } else {
          double dsq = (nb[lc] + nai) - 2.0 * acc[i][j][r];
          dsq = dsq < 0.0 ? 0.0 : dsq;
          kv = kern_eval(pd, dsq, ec);
        }
        if (diag_tile && lr == lc) kv += diag_add;
        acc[i][j][r] = kv;
      }
    }
  }

  // staged stores: passes [0, NH) = the tile itself, SR rows at a time; passes [NH, 2 NH) = the
  // mirror image (rows = original columns)
  const int npass = (!SYM || ti == tj || p.lower_only) ? NH : 2 * NH;
  for (int pass = 0; pass < npass; ++pass) {
    const bool mirror = pass >= NH;
    const int h = mirror ? pass - NH : pass;
    __syncthreads();                                   // staging buffer free (and operands dead)
    // image row of an accumulator element: direct -> wm*WS + i*16 + l4 + 4r ; mirror -> wn*WS + j*16 + l15
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < WT; ++j) {
          const int irow = mirror ? (wn * WS + j * 16 + l15) : (wm * WS + i * 16 + l4 + 4 * r);
          const int icol = mirror ? (wm * WS + i * 16 + l4 + 4 * r) : (wn * WS + j * 16 + l15);
          if (irow / SR == h) St[(irow - h * SR) * SP + icol] = acc[i][j][r];
        }
    __syncthreads();
    const long row_base = (mirror ? n0 : m0) + h * SR;
    const long col_base = mirror ? m0 : n0;
    constexpr int RP = TS / 2;                         // double2 per staged row
#pragma unroll
    for (int q = 0; q < (SR * RP) / 256; ++q) {
      const int idx = tid + 256 * q;
      const int r = idx / RP, c2 = (idx % RP) * 2;
      const long row = row_base + r, col = col_base + c2;
      const long nrow = mirror ? nB : p.n1, ncol = mirror ? p.n1 : nB;
      if (row < nrow && col + 1 < ncol) {
        // streaming (non-temporal) stores for the wide kernels: the matrix is written once and is far larger than
        // L2 + MALL; measured 16384^2: d = 32 SE 0.444 -> 0.428 ms, Matern 0.554 -> 0.53, but d = 6 Matern 0.402 ->
        // 0.418 (tools/r4_run15.sh) -- hence only from a packed width of 16 on (KmArgs::nt_stores)
        if (p.nt_stores)
          __builtin_nontemporal_store(*reinterpret_cast<const double2_t*>(St + r * SP + c2),
                                      reinterpret_cast<double2_t*>(Kout + row * p.ldk + col));
        else
          *reinterpret_cast<double2_t*>(Kout + row * p.ldk + col) =
              *reinterpret_cast<const double2_t*>(St + r * SP + c2);
      } else if (row < nrow && col < ncol) {
        Kout[row * p.ldk + col] = St[r * SP + c2];
        if (col + 1 < ncol) Kout[row * p.ldk + col + 1] = St[r * SP + c2 + 1];
      }
    }
  }
}

// Symmetric Gram matrix of a multi-part kernel with stationary parts (additive: scale * sum_g k_g,
// kernel.py:484-494; coordinate product of SE / Matern factors: kernel.py:578-589): the lower
// triangle of 64 x 64 tiles only, each tile stored twice through the LDS staging buffer as in
// kernmat_sym_kernel.  The parts' packed columns are adjacent, so one LDS fill takes as many whole
// parts as fit into KC columns (the groups of an additive model are a few columns wide: two barriers
// per KC columns instead of two per part), then each part runs its own MFMA dot product, its
// epilogue, and is combined into the running result in the reference's order.
// Half the tiles of the generic kernel, a quarter of its LDS, 20 KB per workgroup.
template <int KC, int SR, int OCC>
__global__ __launch_bounds__(256, OCC) void kernmat_symmulti_kernel(KmArgs p) {
  constexpr int TS = 64, WT = 2, WS = 32;
  constexpr int SP = TS + 2;
  constexpr int NH = TS / SR;
  constexpr int KP = KC + 2;
  constexpr int OPER = 2 * TS * KP;
  constexpr int STAGE = SR * SP;
  constexpr int BODY = (OPER > STAGE) ? OPER : STAGE;
  constexpr int MAXP = KC / 4;           // parts per fill (a part is at least 4 packed columns)
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* As = smem;                     // [TS][KP]
  double* Bs = As + TS * KP;             // [TS][KP]
  double* na = smem + BODY;              // [MAXP][TS]
  double* nb = na + MAXP * TS;           // [MAXP][TS]
  double* St = smem;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, l4 = lane >> 4;
  const unsigned lin = blockIdx.x;
  unsigned ti = (unsigned)((sqrt(8.0 * (double)lin + 1.0) - 1.0) * 0.5);
  while ((unsigned long long)ti * (ti + 1) / 2 > lin) --ti;
  while ((unsigned long long)(ti + 1) * (ti + 2) / 2 <= lin) ++ti;
  const unsigned tj = lin - (unsigned)((unsigned long long)ti * (ti + 1) / 2);
  const long m0 = (long)ti * TS, n0 = (long)tj * TS;
  const ExpConsts& ec = p.ec;

  double4_t res[WT][WT];
  {
    const double r0 = p.product ? p.outer : 0.0;
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int j = 0; j < WT; ++j) res[i][j] = (double4_t){r0, r0, r0, r0};
  }

  int part = p.part_lo;
  while (part < p.part_hi) {
    int pe = part, cols = 0;
    while (pe < p.part_hi && cols + p.parts[pe].kc <= KC) { cols += p.parts[pe].kc; ++pe; }
    const int c0 = p.parts[part].poff;
    const int ch = cols >> 1;
    __syncthreads();
    for (int idx = tid; idx < TS * ch; idx += 256) {
      const int r = idx / ch, c2 = (idx - r * ch) * 2;
      const long rowa = m0 + r, rowb = n0 + r;
      double2_t va = (double2_t){0.0, 0.0}, vb = (double2_t){0.0, 0.0};
      if (rowa < p.n1) va = *reinterpret_cast<const double2_t*>(p.Xp1 + rowa * p.P + c0 + c2);
      if (rowb < p.n1) vb = *reinterpret_cast<const double2_t*>(p.Xp1 + rowb * p.P + c0 + c2);
      *reinterpret_cast<double2_t*>(As + r * KP + c2) = va;
      *reinterpret_cast<double2_t*>(Bs + r * KP + c2) = vb;
    }
    for (int idx = tid; idx < (pe - part) * TS; idx += 256) {
      const int q = idx / TS, r = idx - q * TS;
      const long rowa = m0 + r, rowb = n0 + r;
      na[idx] = rowa < p.n1 ? p.Np1[rowa * p.n_parts_total + part + q] : 0.0;
      nb[idx] = rowb < p.n1 ? p.Np1[rowb * p.n_parts_total + part + q] : 0.0;
    }
    __syncthreads();
    for (int q = part; q < pe; ++q) {
      const PartDev& pd = p.parts[q];
      const int off = pd.poff - c0;
      double4_t acc[WT][WT];
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
      const double* as = As + (wm * WS + l15) * KP + off + l4;
      const double* bs = Bs + (wn * WS + l15) * KP + off + l4;
      for (int kk = 0; kk < pd.kc; kk += 4) {
        double a[WT], b[WT];
#pragma unroll
        for (int t = 0; t < WT; ++t) a[t] = as[t * 16 * KP + kk];
#pragma unroll
        for (int t = 0; t < WT; ++t) b[t] = bs[t * 16 * KP + kk];
#pragma unroll
        for (int i = 0; i < WT; ++i)
#pragma unroll
          for (int j = 0; j < WT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      const bool se = (pd.kind == DFH_KERNEL_SE);
      const double* naq = na + (q - part) * TS;
      const double* nbq = nb + (q - part) * TS;
#pragma unroll
      for (int i = 0; i < WT; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double nai = naq[wm * WS + i * 16 + l4 + 4 * r];
#pragma unroll
          for (int j = 0; j < WT; ++j) {
            const double nbj = nbq[wn * WS + j * 16 + l15];
            double kv;
            if (se) {                    // -dsq/2 = acc - (na/2 + nb/2), see kernmat_sym_kernel
              double t = acc[i][j][r] - (0.5 * nbj + 0.5 * nai);
              t = t > 0.0 ? 0.0 : t;
              kv = pd.scale_c * exp_fast(t, ec);
            } else {
              double dsq = (nbj + nai) - 2.0 * acc[i][j][r];
              dsq = dsq < 0.0 ? 0.0 : dsq;
              kv = kern_eval(pd, dsq, ec);
            }
            res[i][j][r] = p.product ? res[i][j][r] * kv : res[i][j][r] + kv;   // kernel.py:588 / :493
          }
        }
      }
    }
    part = pe;
  }

  const bool diag_tile = (ti == tj);
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < WT; ++j) {
        double v = res[i][j][r];
        if (p.apply_outer && !p.product) v = p.outer * v;                       // kernel.py:494
        if (diag_tile && (wm * WS + i * 16 + l4 + 4 * r) == (wn * WS + j * 16 + l15)) v += p.diag_add;
        res[i][j][r] = v;
      }

  const int npass = diag_tile ? NH : 2 * NH;
  for (int pass = 0; pass < npass; ++pass) {
    const bool mirror = pass >= NH;
    const int h = mirror ? pass - NH : pass;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < WT; ++j) {
          const int irow = mirror ? (wn * WS + j * 16 + l15) : (wm * WS + i * 16 + l4 + 4 * r);
          const int icol = mirror ? (wm * WS + i * 16 + l4 + 4 * r) : (wn * WS + j * 16 + l15);
          if (irow / SR == h) St[(irow - h * SR) * SP + icol] = res[i][j][r];
        }
    __syncthreads();
    const long row_base = (mirror ? n0 : m0) + h * SR;
    const long col_base = mirror ? m0 : n0;
    constexpr int RP = TS / 2;
#pragma unroll
    for (int q = 0; q < (SR * RP) / 256; ++q) {
      const int idx = tid + 256 * q;
      const int r = idx / RP, c2 = (idx % RP) * 2;
      const long row = row_base + r, col = col_base + c2;
      if (row < p.n1 && col + 1 < p.n1) {
        *reinterpret_cast<double2_t*>(p.K + row * p.ldk + col) = *reinterpret_cast<const double2_t*>(St + r * SP + c2);
      } else if (row < p.n1 && col < p.n1) {
        p.K[row * p.ldk + col] = St[r * SP + c2];
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Cross matrix K(X1, X2), single-part SE / Matern kernels, packed width 8..32: "strip" kernel.
//
// What was measured on gfx950 (tools/km_bench.hip, 32768 x 16384, d = 32): the fp64 MFMA work of
// the distance expansion alone takes 0.56 ms, the fp64 VALU epilogue (clip, exp) alone 0.43 ms,
// both together 0.89 ms -- fp64 matrix and fp64 vector instructions share the SIMD's fp64 pipe on
// this part, they do not overlap -- and the 4.3 GB of output 0.72 ms.  The pass is bound by that
// pipe, so the kernel is organised to keep it fed: no LDS, no barriers, a wave keeps the operand
// fragments of its 32 rows in registers and walks along the columns in tiles of 64, loading the
// next tile's column fragments a whole tile ahead (register double buffer) while the current tile
// runs its 8 * C MFMAs and its epilogue; stores are fire-and-forget; two such waves per SIMD.
// Operand fragments come straight from L2: lane (l15, l4) of an MFMA holds, for row l15 of a
// 16-row tile, the packed columns [l4 * C, (l4 + 1) * C) -- which k of the dot product sits in
// which MFMA slot is free as long as both operands agree -- i.e. contiguous 16-byte loads.
// Same expansion as the reference ((|a|^2 + |b|^2) - 2 a.b, clipped at 0; general_utils.py:66-69),
// only the summation order inside a.b differs from the LDS kernel's.
// The 64 x 64-tile LDS kernel (kernmat_sym_kernel<..., false>) took 1.45 ms on this shape and
// 0.84 ms (Matern-2.5) for 65536 x 4096 at d = 6, this one 1.1-1.2 ms and 0.5 ms.
// ---------------------------------------------------------------------------------------------
// MU: the product of the strip with a vector (the posterior mean K(X*, X) alpha, gp_core.py:174) rides
// along: every lane accumulates K[row][col] * alpha[col] over the columns it owns, tile after tile;
// at the end of every block of KM_MU_BLOCK columns the 16 lanes that share a row add up (fixed
// butterfly) and the row's partial sum of that block is written out.  A second, tiny kernel adds
// the blocks in order.  Blocks are cut by column index alone and segments consist of whole blocks,
// so a row's mean does not depend on how many rows the call has or where they start (chunks,
// shards, Thompson blocks all give the same bits) -- and the 8 n m bytes of the cross matrix are
// not read again for it.
template <int KIND, int C, int MP, bool MU = false>
__global__ __launch_bounds__(256, 2) void kernmat_strip_kernel(KmArgs p, int tiles_per_seg) {
  // 32 rows x 64 (wide packed inputs: 32) columns per wave and tile, at least 2 waves per SIMD (measured
  // 1.40 -> 1.12 ms against 64 x 32 at one wave per SIMD: a lone wave has nothing to cover its own stalls)
  // (with the mean riding along, the 64-column tile of the narrow packings would spill registers)
  constexpr int WI = 2, WJ = ((C >= 6 || MU) ? 2 : 4);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const long m0 = ((long)blockIdx.y * 4 + wave) * (16 * WI);
  if (m0 >= p.n1) return;
  const long ntile = ((long)p.n2 + 16 * WJ - 1) / (16 * WJ);
  const long t0 = (long)blockIdx.x * tiles_per_seg;
  const long t1 = t0 + tiles_per_seg < ntile ? t0 + tiles_per_seg : ntile;
  if (t0 >= t1) return;
  const PartDev& pd = p.parts[p.part_lo];
  const ExpConsts& ec = p.ec;              // SE: scale_c already folded into the coefficients
  const int npt = p.n_parts_total, part = p.part_lo;
  const double* __restrict__ A = p.Xp1 + pd.poff + l4 * C;
  const double* __restrict__ B = p.Xp2 + pd.poff + l4 * C;
  double a[WI][C];
  double nah[WI][4];                       // SE: |a|^2 / 2 ; Matern: |a|^2
#pragma unroll
  for (int i = 0; i < WI; ++i) {
    long row = m0 + i * 16 + l15;
    row = row < p.n1 ? row : p.n1 - 1;
    const double* src = A + row * p.P;
#pragma unroll
    for (int c = 0; c < C; c += 2) {
      const double2_t v = *reinterpret_cast<const double2_t*>(src + c);
      a[i][c] = v.x; a[i][c + 1] = v.y;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      long rr = m0 + i * 16 + l4 + 4 * r;
      rr = rr < p.n1 ? rr : p.n1 - 1;
      const double v = p.Np1[rr * npt + part];
      nah[i][r] = KIND == DFH_KERNEL_SE ? 0.5 * v : v;
    }
  }
  // Matern constants (uniform)
  constexpr int mp = MP;                   // Matern: int(nu), compile time
  const double s8 = pd.s8, s2 = pd.s2, gsc = pd.scale_c * pd.gfac;
  const double c0 = pd.coeff[0], c1 = pd.coeff[1], c2 = pd.coeff[2], c3 = pd.coeff[3];
  double b[WJ][C], nbh[WJ];
  double alh[WJ], mu_acc[WI][4];
  constexpr int TPB = KM_MU_BLOCK / (16 * WJ);        // tiles per mean block
  if (MU) {
#pragma unroll
    for (int i = 0; i < WI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) mu_acc[i][r] = 0.0;
  }
  auto load_b = [&](long t, double (&bb)[WJ][C], double (&nn)[WJ]) {
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      // MFMA tile j, lane column l15 <-> matrix column n0 + WJ l15 + j: a lane then owns WJ ADJACENT
      // columns of every row it holds and stores them with 16-byte instructions
      long col = t * (16 * WJ) + WJ * l15 + j;
      col = col < p.n2 ? col : p.n2 - 1;
      const double* src = B + col * p.P;
#pragma unroll
      for (int c = 0; c < C; c += 2) {
        const double2_t v = *reinterpret_cast<const double2_t*>(src + c);
        bb[j][c] = v.x; bb[j][c + 1] = v.y;
      }
      const double v = p.Np2[col * npt + part];
      nn[j] = KIND == DFH_KERNEL_SE ? 0.5 * v : v;
    }
  };
  // per-lane element offset inside a 4-row group: the store address is a wave-uniform row-group base
  // plus this
  const unsigned voff = (unsigned)(l4 * p.ldk + WJ * l15);
  double* __restrict__ Kstrip = p.K + m0 * p.ldk;
  const bool rows_full = m0 + 16 * WI <= p.n1;
  load_b(t0, b, nbh);
  for (long t = t0; t < t1; ++t) {
    double bn[WJ][C], nbn[WJ];
    load_b(t + 1 < t1 ? t + 1 : t, bn, nbn);
    if (MU) {               // this tile's alpha (L2-resident): issued here, used after the MFMAs
#pragma unroll
      for (int j = 0; j < WJ; ++j) {
        const long col = t * (16 * WJ) + WJ * l15 + j;
        alh[j] = col < p.n2 ? p.mu_alpha[col] : 0.0;
      }
    }
    double4_t acc[WI][WJ];
#pragma unroll
    for (int i = 0; i < WI; ++i)
#pragma unroll
      for (int j = 0; j < WJ; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int i = 0; i < WI; ++i)
#pragma unroll
        for (int j = 0; j < WJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][c], b[j][c], acc[i][j], 0, 0, 0);
    const long n0 = t * (16 * WJ);
    double* __restrict__ Kt = Kstrip + n0;
    auto epilogue = [&](auto full_tag) {
      constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
      for (int i = 0; i < WI; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double kvs[WJ];
#pragma unroll
          for (int j = 0; j < WJ; ++j) {
            double kv;
            if (KIND == DFH_KERNEL_SE) {
              // -dsq/2 directly: acc - (|b|^2/2 + |a|^2/2), clipped at 0 (scaling by 2 commutes with
              // rounding: the same number as ((nb + na) - 2 acc) clipped, halved and negated)
              double tt = acc[i][j][r] - (nbh[j] + nah[i][r]);
              tt = tt > 0.0 ? 0.0 : tt;
              kv = exp_fast_neg(tt, ec);                               // kernel.py:176, scale inside ec
            } else {
              double dsq = (nbh[j] + nah[i][r]) - 2.0 * acc[i][j][r];   // general_utils.py:66-68
              dsq = dsq < 0.0 ? 0.0 : dsq;
              const double dist = sqrt_fast(dsq);                       // kernel.py:296
              const double mult = s8 * dist;                            // kernel.py:265
              double u;                                                 // sum_i coeff_i mult^(p-i), kernel.py:266
              if (mp == 0) u = c0;
              else if (mp == 1) u = fma(c0, mult, c1);
              else if (mp == 2) u = fma(fma(c0, mult, c1), mult, c2);
              else u = fma(fma(fma(c0, mult, c1), mult, c2), mult, c3);
              kv = u * (gsc * exp_fast_neg(-s2 * dist, ec));             // kernel.py:268-269, 298
            }
            kvs[j] = kv;
            if (MU) mu_acc[i][r] = fma(kv, alh[j], mu_acc[i][r]);
          }
          double* __restrict__ rowp = Kt + (long)(i * 16 + 4 * r) * p.ldk;      // wave-uniform
          if (FULL) {
#pragma unroll
            for (int j = 0; j < WJ; j += 2)
              *reinterpret_cast<double2_t*>(rowp + voff + j) = (double2_t){kvs[j], kvs[j + 1]};
          } else {
            const long row = m0 + i * 16 + l4 + 4 * r, col = n0 + WJ * l15;
#pragma unroll
            for (int j = 0; j < WJ; ++j)
              if (row < p.n1 && col + j < p.n2) rowp[voff + j] = kvs[j];
          }
        }
      }
    };
    if (rows_full && n0 + 16 * WJ <= p.n2) epilogue(std::true_type{});
    else epilogue(std::false_type{});
    if (MU && ((t + 1) % TPB == 0 || t + 1 == t1)) {          // a mean block is complete
      const long blk = t / TPB;
#pragma unroll
      for (int i = 0; i < WI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double v = mu_acc[i][r];
          v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
          const long row = m0 + i * 16 + l4 + 4 * r;
          if (l15 == 0 && row < p.n1) p.mu_part[row * p.mu_nblk + blk] = v;
          mu_acc[i][r] = 0.0;
        }
    }
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      nbh[j] = nbn[j];
#pragma unroll
      for (int c = 0; c < C; ++c) b[j][c] = bn[j][c];
    }
  }
}

// mu[row] = the mean blocks of the row added in order
__global__ void k_mu_finish(const double* __restrict__ part, long n, int nblk, double* __restrict__ mu) {
  const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[row * nblk + b];
  mu[row] = s;
}

template <int KIND, int MP>
int launch_strip(dfh_ctx* ctx, KmArgs a, int C) {
  // enough waves for 256 CUs x 4 SIMDs x 2: split the columns of a 64-row strip into segments
  const long strips = ((long)a.n1 + 31) / 32;
  const int tile_cols = (C >= 6 || a.mu_part) ? 32 : 64;
  const long ntile = ((long)a.n2 + tile_cols - 1) / tile_cols;
  static const long waves_env = env_long("DFH_KM_WAVES", 8192), want_waves = waves_env > 0 ? waves_env : 8192;
  long segs = (want_waves + strips - 1) / strips;
  if (segs > ntile) segs = ntile;
  if (segs < 1) segs = 1;
  int tps = (int)((ntile + segs - 1) / segs);
  if (a.mu_part) {                                   // segments of whole mean blocks
    const int tpb = KM_MU_BLOCK / tile_cols;
    tps = (tps + tpb - 1) / tpb * tpb;
  }
  segs = (ntile + tps - 1) / tps;
  dim3 grid((unsigned)segs, (unsigned)((strips + 3) / 4));
  if (a.mu_part) {
    switch (C) {
      case 2: hipLaunchKernelGGL((kernmat_strip_kernel<KIND, 2, MP, true>), grid, dim3(256), 0, ctx->stream, a, tps); break;
      case 4: hipLaunchKernelGGL((kernmat_strip_kernel<KIND, 4, MP, true>), grid, dim3(256), 0, ctx->stream, a, tps); break;
      case 6: hipLaunchKernelGGL((kernmat_strip_kernel<KIND, 6, MP, true>), grid, dim3(256), 0, ctx->stream, a, tps); break;
      default: hipLaunchKernelGGL((kernmat_strip_kernel<KIND, 8, MP, true>), grid, dim3(256), 0, ctx->stream, a, tps); break;
    }
    DFH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mu_finish, dim3((unsigned)((a.n1 + 255) / 256)), dim3(256), 0, ctx->stream, a.mu_part, (long)a.n1,
                       a.mu_nblk, a.mu_out);
    DFH_LAUNCH_CHECK();
    return DFH_OK;
  }
  switch (C) {
    case 2: hipLaunchKernelGGL((kernmat_strip_kernel<KIND, 2, MP>), grid, dim3(256), 0, ctx->stream, a, tps); break;
    case 4: hipLaunchKernelGGL((kernmat_strip_kernel<KIND, 4, MP>), grid, dim3(256), 0, ctx->stream, a, tps); break;
    case 6: hipLaunchKernelGGL((kernmat_strip_kernel<KIND, 6, MP>), grid, dim3(256), 0, ctx->stream, a, tps); break;
    default: hipLaunchKernelGGL((kernmat_strip_kernel<KIND, 8, MP>), grid, dim3(256), 0, ctx->stream, a, tps); break;
  }
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

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

double factorial_d(int n) {
  double r = 1.0;
  for (int i = 2; i <= n; ++i) r *= (double)i;
  return r;
}

double part_value_at_zero(const PartDev& pd);

int fill_part(PartDev& pd, int kind, double scale, double nu) {
  pd.kind = kind;
  pd.p = 0; pd.s8 = pd.s2 = pd.gfac = 0.0; pd.k0 = 0.0;
  for (int i = 0; i < 8; ++i) pd.coeff[i] = 0.0;
  if (kind == DFH_KERNEL_SE || kind == DFH_KERNEL_DIST) {
    pd.scale_c = scale;
    pd.k0 = part_value_at_zero(pd);
    return DFH_OK;
  }
  if (kind == DFH_KERNEL_POLY) {               // nu carries the order
    if (!(nu >= 0.0 && nu <= 64.0 && nu == floor(nu))) {
      dfh_set_error("polynomial kernel: the order has to be an integer in [0, 64] (got %g)", nu);
      return DFH_ERR_BAD_ARG;
    }
    pd.p = (int)nu; pd.scale_c = scale;
    return DFH_OK;
  }
  if (kind == DFH_KERNEL_EXPDECAY) {           // nu carries the offset; powers are set by the caller
    pd.scale_c = scale; pd.gfac = nu;
    return DFH_OK;
  }
  if (kind == DFH_KERNEL_HAMMING) {            // the weights go to the image's hw section, their sum to k0 (make_part)
    pd.scale_c = 1.0;
    return DFH_OK;
  }
  // Matern: kernel.py:242-253, 259-270
  double frac = fmod(nu, 1.0);
  if (!(frac == 0.5) || nu < 0.5) {
    dfh_set_error("Matern kernel: nu has to be p + 0.5 where p is an integer (got %g)", nu);
    return DFH_ERR_BAD_ARG;
  }
  const int p = (int)nu;
  if (p > 7) {
    dfh_set_error("Matern kernel: nu = %g not supported (p <= 7)", nu);
    return DFH_ERR_BAD_ARG;
  }
  pd.p = p;
  for (int i = 0; i <= p; ++i)
    pd.coeff[i] = factorial_d(p + i) / (factorial_d(i) * factorial_d(p - i));
  pd.s8 = sqrt(8.0 * nu);
  pd.s2 = sqrt(2.0 * nu);
  pd.gfac = tgamma((double)p + 1.0) / tgamma(2.0 * p + 1.0);
  // norm_constant = 1 / _eval_kernel_values_unnormalised(0)   (kernel.py:253)
  double u0 = 0.0;
  const double mult0 = pd.s8 * 0.0;
  for (int i = 0; i <= p; ++i) u0 += pd.coeff[i] * pow(mult0, (double)(p - i));
  u0 *= (pd.gfac * exp(-pd.s2 * 0.0));
  const double norm_constant = 1.0 / u0;
  pd.scale_c = scale * norm_constant;
  pd.k0 = part_value_at_zero(pd);
  return DFH_OK;
}

double part_value_at_zero(const PartDev& pd) {
  // k_part(x, x): distance 0
  if (pd.kind == DFH_KERNEL_SE) return pd.scale_c * exp(-0.0 / 2);
  if (pd.kind == DFH_KERNEL_MATERN) {
    double u = 0.0;
    for (int i = 0; i <= pd.p; ++i) u += pd.coeff[i] * pow(0.0, (double)(pd.p - i));
    u *= (pd.gfac * exp(-pd.s2 * 0.0));
    return pd.scale_c * u;
  }
  return 0.0;
}

// device image of a KernDev: [parts | bw | cols | lcols | hw], each section 16-byte aligned (hw: the weight of
// every packed column of a Hamming part, 0 elsewhere; the kernels find it with blob_hw_offset)
static size_t pad16(size_t x) { return (x + 15) & ~(size_t)15; }
static void blob_layout(const KernDev& kd, size_t off[5], size_t* total) {
  const size_t P = kd.P ? kd.P : 1;
  off[0] = 0;
  off[1] = off[0] + pad16(sizeof(PartDev) * kd.parts.size());
  off[2] = off[1] + pad16(sizeof(double) * P);
  off[3] = off[2] + pad16(sizeof(int) * P);
  off[4] = blob_hw_offset((int)kd.parts.size(), kd.P);
  *total = off[4] + pad16(sizeof(double) * P);
}
static void blob_fill(const KernDev& kd, char* host) {
  size_t off[5], total;
  blob_layout(kd, off, &total);
  std::memcpy(host + off[0], kd.parts.data(), sizeof(PartDev) * kd.parts.size());
  std::memcpy(host + off[1], kd.bw.data(), sizeof(double) * kd.P);
  std::memcpy(host + off[2], kd.cols.data(), sizeof(int) * kd.P);
  std::memcpy(host + off[3], kd.lcols.data(), sizeof(int) * kd.P);
  std::memcpy(host + off[4], kd.hw.data(), sizeof(double) * kd.P);
}
static void blob_point(KernDev* kd, char* dev) {
  size_t off[5], total;
  blob_layout(*kd, off, &total);
  kd->d_parts = reinterpret_cast<PartDev*>(dev + off[0]);
  kd->d_bw = reinterpret_cast<double*>(dev + off[1]);
  kd->d_cols = reinterpret_cast<int*>(dev + off[2]);
  kd->d_lcols = reinterpret_cast<int*>(dev + off[3]);
}

int upload(dfh_ctx* ctx, KernDev* kd) {
  size_t off[5], total;
  blob_layout(*kd, off, &total);
  std::vector<char> host(total, 0);
  blob_fill(*kd, host.data());
  DFH_HIP(hipMalloc(&kd->d_blob, total));
  blob_point(kd, static_cast<char*>(kd->d_blob));
  DFH_HIP(hipMemcpyAsync(kd->d_blob, host.data(), total, hipMemcpyHostToDevice, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

void add_part_cols(KernDev* kd, PartDev& pd, const int* cols, const double* bw, int ncols) {
  pd.poff = kd->P;
  pd.kc = (ncols + 3) & ~3;
  for (int c = 0; c < pd.kc; ++c) {
    kd->cols.push_back(c < ncols ? cols[c] : -1);
    kd->lcols.push_back(c < ncols ? c : -1);
    kd->bw.push_back(c < ncols ? bw[c] : 1.0);
    kd->hw.push_back(0.0);
  }
  kd->P += pd.kc;
}

}  // namespace

// (eq * wts).sum(axis=1) of a row whose entries all compare equal: NumPy's pairwise order (hamming_eval on the device)
static double np_sum_host(const double* a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// One part from (kind, scale, nu, per-column parameters): SE / Matern bandwidths divide the inputs,
// polynomial scalings multiply them (stored negated, see k_pack_cols), exponential-decay powers go
// into the part and its inputs stay as they are.
static int make_part(KernDev* kd, int kind, double scale, double nu, const int* cols, const double* par, int ncols) {
  PartDev pd;
  DFH_TRY(fill_part(pd, kind, scale, nu));
  pd.fmode = 0; pd.fpad = 0; pd.fscale = 1.0;
  std::vector<double> bw((size_t)ncols);
  if (kind == DFH_KERNEL_POLY) {
    for (int c = 0; c < ncols; ++c) {
      if (!(par[c] > 0.0)) { dfh_set_error("polynomial kernel: dim_scalings must be positive"); return DFH_ERR_BAD_ARG; }
      bw[c] = -par[c];
    }
  } else if (kind == DFH_KERNEL_EXPDECAY) {
    if (ncols > EXPDECAY_MAX_DIM) {
      dfh_set_error("exponential-decay kernel: at most %d dimensions (got %d)", EXPDECAY_MAX_DIM, ncols);
      return DFH_ERR_BAD_ARG;
    }
    pd.p = ncols;
    for (int c = 0; c < ncols; ++c) { pd.coeff[c] = par[c]; bw[c] = 1.0; }
  } else if (kind == DFH_KERNEL_HAMMING) {
    if (ncols > HAMMING_MAX_DIM) {
      dfh_set_error("Hamming kernel: at most %d dimensions (got %d)", HAMMING_MAX_DIM, ncols);
      return DFH_ERR_BAD_ARG;
    }
    if (scale != 1.0 || nu != 0.0) {
      dfh_set_error("Hamming kernel: scale must be 1 and nu 0 (got %g, %g)", scale, nu);
      return DFH_ERR_BAD_ARG;
    }
    pd.p = ncols;
    for (int c = 0; c < ncols; ++c) bw[c] = 1.0;         // the category codes stay as they are (x / 1.0)
    pd.k0 = np_sum_host(par, ncols);                      // k(x, x) = sum_c w_c whatever x
  } else {
    for (int c = 0; c < ncols; ++c) bw[c] = par[c];
  }
  add_part_cols(kd, pd, cols, bw.data(), ncols);
  if (kind == DFH_KERNEL_HAMMING)
    for (int c = 0; c < ncols; ++c) kd->hw[(size_t)pd.poff + c] = par[c];
  kd->parts.push_back(pd);
  return DFH_OK;
}

int kerndev_build_host(const dfh_kernel_desc* k, KernDev* kd) {
  DFH_ARG(k != nullptr && kd != nullptr);
  DFH_ARG(k->dim >= 1);
  kd->kind = k->kind; kd->dim = k->dim; kd->P = 0;
  kd->parts.clear(); kd->cols.clear(); kd->lcols.clear(); kd->bw.clear(); kd->hw.clear();
  kd->stationary = true; kd->kxx = 0.0;
  kd->esp = false; kd->esp_order = 0; kd->hamming = false;
  if (k->kind == DFH_KERNEL_SE || k->kind == DFH_KERNEL_MATERN) {
    DFH_ARG(k->bw != nullptr);
    std::vector<int> ident(k->dim);
    for (int i = 0; i < k->dim; ++i) ident[i] = i;
    DFH_TRY(make_part(kd, k->kind, k->scale, k->nu, ident.data(), k->bw, k->dim));
    kd->multi = false; kd->product = false; kd->outer_scale = 1.0; kd->nested = false;
    kd->kxx = kd->parts[0].k0;
  } else if (k->kind == DFH_KERNEL_POLY || k->kind == DFH_KERNEL_EXPDECAY || k->kind == DFH_KERNEL_HAMMING) {
    // a product with one factor and outer scale 1 (1.0 * k is exact): the generic multi-part
    // kernel-matrix kernel is the only one that knows these kinds
    DFH_ARG(k->bw != nullptr);
    kd->hamming = k->kind == DFH_KERNEL_HAMMING;
    std::vector<int> ident(k->dim);
    for (int i = 0; i < k->dim; ++i) ident[i] = i;
    DFH_TRY(make_part(kd, k->kind, k->scale, k->nu, ident.data(), k->bw, k->dim));
    kd->multi = true; kd->product = true; kd->outer_scale = 1.0; kd->nested = false;
    kd->stationary = false;
  } else if (k->kind == DFH_KERNEL_ADDITIVE || k->kind == DFH_KERNEL_PRODUCT) {
    DFH_ARG(k->n_groups >= 1 && k->group_off && k->group_dims && k->sub_kind && k->sub_scale && k->sub_bw);
    const bool product = (k->kind == DFH_KERNEL_PRODUCT);
    const bool nested = product && k->group_factor != nullptr;
    if (k->group_factor || k->factor_is_sum || k->factor_scale)
      DFH_ARG(product && k->group_factor && k->factor_is_sum && k->factor_scale);
    double acc = product ? k->scale : 0.0;
    double facc = 0.0;                              // k(x, x) of the additive factor under way
    for (int g = 0; g < k->n_groups; ++g) {
      const int lo = k->group_off[g], hi = k->group_off[g + 1];
      DFH_ARG(hi > lo);
      for (int c = lo; c < hi; ++c) DFH_ARG(k->group_dims[c] >= 0 && k->group_dims[c] < k->dim);
      const int sk = k->sub_kind[g];
      // polynomial groups also in an additive kernel (the reference's factory builds them: euclidean_gp.py:870-879)
      DFH_ARG(kind_is_stationary(sk) || sk == DFH_KERNEL_POLY || (product && (sk == DFH_KERNEL_EXPDECAY || sk == DFH_KERNEL_HAMMING)));
      if (sk == DFH_KERNEL_HAMMING) kd->hamming = true;
      DFH_TRY(make_part(kd, sk, k->sub_scale[g], k->sub_nu ? k->sub_nu[g] : 0.0, k->group_dims + lo,
                        k->sub_bw + lo, hi - lo));
      if (!kind_is_stationary(sk)) kd->stationary = false;
      const double k0 = kd->parts.back().k0;
      PartDev& pd = kd->parts.back();
      pd.fmode = 0; pd.fpad = 0; pd.fscale = 1.0;
      if (nested) {
        const int f = k->group_factor[g];
        DFH_ARG(f >= 0 && f <= g && (g == 0 ? f == 0 : (f == k->group_factor[g - 1] || f == k->group_factor[g - 1] + 1)));
        const bool first = g == 0 || k->group_factor[g - 1] != f;
        const bool last = g + 1 == k->n_groups || k->group_factor[g + 1] != f;
        if (k->factor_is_sum[f]) {
          DFH_ARG(sk != DFH_KERNEL_EXPDECAY && sk != DFH_KERNEL_HAMMING);       // an additive kernel's groups: SE / Matern / polynomial
          pd.fmode = FM_IN | (first ? FM_BEGIN : 0) | (last ? FM_END : 0);
          pd.fscale = k->factor_scale[f];
          facc = first ? 0.0 + k0 : facc + k0;
          if (last) acc *= pd.fscale * facc;
        } else {
          DFH_ARG(first && last);                   // a plain factor is one group
          acc *= k0;
        }
      } else if (product) {
        acc *= k0;                                    // K *= kernel(...)        kernel.py:588
      } else {
        acc += k0;                                    // result += kernel(...)   kernel.py:493
      }
    }
    kd->multi = true; kd->product = product; kd->outer_scale = k->scale; kd->nested = nested;
    kd->kxx = !kd->stationary ? 0.0 : (product ? acc : k->scale * acc);        // kernel.py:494
  } else if (k->kind == DFH_KERNEL_ESP) {
    // kernel.py:671-744: one 1-D SE / Matern kernel per column, kernel_list[i] on column i
    if (!(k->n_groups == k->dim && k->group_off && k->group_dims && k->sub_kind && k->sub_scale && k->sub_bw)) {
      dfh_set_error("ESP kernel: needs n_groups == dim (%d) with group_off, group_dims, sub_kind, sub_scale, sub_bw",
                    k->dim);
      return DFH_ERR_BAD_ARG;
    }
    if (k->group_factor || k->factor_is_sum || k->factor_scale) {
      dfh_set_error("ESP kernel: group_factor / factor_is_sum / factor_scale must be NULL");
      return DFH_ERR_BAD_ARG;
    }
    if (k->dim > ESP_MAX_DIM) {
      dfh_set_error("ESP kernel: at most %d dimensions on the device (got %d)", ESP_MAX_DIM, k->dim);
      return DFH_ERR_BAD_ARG;
    }
    if (!(k->nu >= 1.0 && k->nu <= (double)k->dim && k->nu == floor(k->nu))) {
      dfh_set_error("ESP kernel: order must be an integer between 1 and dim = %d (got %g)", k->dim, k->nu);
      return DFH_ERR_BAD_ARG;
    }
    const int order = (int)k->nu;
    if (order > ESP_MAX_ORDER) {
      dfh_set_error("ESP kernel: order %d is above the device's %d", order, ESP_MAX_ORDER);
      return DFH_ERR_BAD_ARG;
    }
    if (k->group_off[0] != 0) {
      dfh_set_error("ESP kernel: group_off[0] must be 0");
      return DFH_ERR_BAD_ARG;
    }
    for (int g = 0; g < k->dim; ++g) {
      if (k->group_off[g + 1] != g + 1 || k->group_dims[g] != g) {
        dfh_set_error("ESP kernel: group %d must be column %d alone (group_off = 0..dim, group_dims[g] = g)", g, g);
        return DFH_ERR_BAD_ARG;
      }
      if (!kind_is_stationary(k->sub_kind[g])) {
        dfh_set_error("ESP kernel: the kernel of column %d must be SE or Matern (kind %d)", g, k->sub_kind[g]);
        return DFH_ERR_BAD_ARG;
      }
      DFH_TRY(make_part(kd, k->sub_kind[g], k->sub_scale[g], k->sub_nu ? k->sub_nu[g] : 0.0, &g, k->sub_bw + g, 1));
    }
    // k(x, x): the device's power sums and Newton-Girard steps on the parts' values at distance 0
    // (a Matern part's k0 is norm_constant * unnorm(0), not necessarily exactly 1)
    double ps[ESP_MAX_ORDER] = {0.0};
    for (int g = 0; g < k->dim; ++g) {
      const double kv = kd->parts[g].k0;
      double kp = kv;
      for (int i = 0; i < order; ++i) { ps[i] = ps[i] + kp; kp = kp * kv; }
    }
    double e[ESP_MAX_ORDER + 1];
    e[0] = 1.0;
    for (int m = 1; m <= order; ++m) {
      double acc = 0.0;
      for (int i = 1; i <= m; ++i) {
        const double t = e[m - i] * ps[i - 1];
        acc = (i & 1) ? acc + t : acc - t;
      }
      e[m] = acc / (double)m;
    }
    kd->multi = true; kd->product = false; kd->outer_scale = k->scale; kd->nested = false;
    kd->esp = true; kd->esp_order = order;
    kd->kxx = k->scale * e[order];
  } else {
    dfh_set_error("unknown kernel kind %d", k->kind);
    return DFH_ERR_BAD_ARG;
  }
  kd->n_parts = (int)kd->parts.size();
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

int kerndev_build(dfh_ctx* ctx, const dfh_kernel_desc* k, KernDev* kd) {
  DFH_TRY(kerndev_build_host(k, kd));
  return upload(ctx, kd);
}

size_t kerndev_blob_bytes(const KernDev& kd) {
  size_t off[5], total;
  blob_layout(kd, off, &total);
  return total;
}
void kerndev_blob_fill(const KernDev& kd, char* host) { blob_fill(kd, host); }

// The same without the copy: the images are laid out in `host` (the caller's pinned staging memory, copied up by the
// caller together with whatever else the launch needs) and the descriptors pointed at where they WILL be on the device.
int kerndev_stage_many(KernDev* kds, int count, char* host, void* d_blob, size_t blob_bytes) {
  std::memset(host, 0, blob_bytes);
  size_t at = 0;
  for (int c = 0; c < count; ++c) {
    const size_t sz = kerndev_blob_bytes(kds[c]);
    DFH_ARG(at + sz <= blob_bytes);
    blob_fill(kds[c], host + at);
    kds[c].d_blob = nullptr;                    // not owned
    blob_point(&kds[c], static_cast<char*>(d_blob) + at);
    at += sz;
  }
  return DFH_OK;
}

int kerndev_upload_many(dfh_ctx* ctx, KernDev* kds, int count, void* d_blob, size_t blob_bytes) {
  std::vector<char> host(blob_bytes, 0);
  size_t at = 0;
  for (int c = 0; c < count; ++c) {
    const size_t sz = kerndev_blob_bytes(kds[c]);
    DFH_ARG(at + sz <= blob_bytes);
    blob_fill(kds[c], host.data() + at);
    kds[c].d_blob = nullptr;                    // not owned
    blob_point(&kds[c], static_cast<char*>(d_blob) + at);
    at += sz;
  }
  DFH_HIP(hipMemcpyAsync(d_blob, host.data(), at, hipMemcpyHostToDevice, ctx->stream));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}


int kerndev_build_dist(dfh_ctx* ctx, int dim, KernDev* kd) {
  DFH_ARG(dim >= 1);
  kd->kind = DFH_KERNEL_DIST; kd->dim = dim; kd->P = 0;
  kd->parts.clear(); kd->cols.clear(); kd->lcols.clear(); kd->bw.clear(); kd->hw.clear();
  PartDev pd;
  DFH_TRY(fill_part(pd, DFH_KERNEL_DIST, 1.0, 0.0));
  std::vector<int> ident(dim);
  std::vector<double> ones(dim, 1.0);
  for (int i = 0; i < dim; ++i) ident[i] = i;
  add_part_cols(kd, pd, ident.data(), ones.data(), dim);
  kd->parts.push_back(pd);
  kd->multi = false; kd->outer_scale = 1.0; kd->kxx = 0.0;
  kd->esp = false; kd->esp_order = 0; kd->hamming = false;
  kd->n_parts = 1;
  return upload(ctx, kd);
}

int kerndev_clone(dfh_ctx* ctx, const KernDev& src, KernDev* out) {
  *out = src;
  out->d_blob = nullptr; out->d_parts = nullptr; out->d_cols = nullptr; out->d_lcols = nullptr; out->d_bw = nullptr;
  return upload(ctx, out);
}

void kerndev_free(KernDev* kd) {
  if (!kd) return;
  if (kd->d_blob) (void)hipFree(kd->d_blob);
  kd->d_blob = nullptr;
  kd->d_parts = nullptr; kd->d_cols = nullptr; kd->d_lcols = nullptr; kd->d_bw = nullptr;
}

double kerndev_part_kxx(const KernDev& kd, int part) { return part_value_at_zero(kd.parts[part]); }

int pack_scaled(dfh_ctx* ctx, const KernDev& kd, int part_lo, int part_hi, bool pre_gathered,
                const double* X, int64_t n, int64_t ldx, double* Xp, double* Np, int count,
                int64_t sBlob, int64_t sXp, int64_t sNp) {
  if (n <= 0 || count <= 0) return DFH_OK;
  DFH_ARG(part_lo >= 0 && part_hi <= kd.n_parts && part_lo < part_hi);
  DFH_ARG(!pre_gathered || part_hi == part_lo + 1);
  const int c_lo = kd.parts[part_lo].poff;
  const int c_hi = kd.parts[part_hi - 1].poff + kd.parts[part_hi - 1].kc;
  static const bool fused_pack = env_flag("DFH_PACK_FUSED", true);
  if (fused_pack && c_hi - c_lo <= 2048) {
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

// `count` symmetric Gram matrices of structurally identical single-part kernels in one launch
// (blockIdx.z): kernel images sBlob bytes apart starting at kd's, packed inputs sXp / sNp doubles
// apart, outputs sK doubles apart, diag_adds[count] on the device.  Needs an even ldk.
int kernmat_sym_batch(dfh_ctx* ctx, const KernDev& kd, int count, int64_t sBlob, const double* Xp,
                      int64_t sXp, const double* Np, int64_t sNp, int64_t n, const double* d_diag_adds,
                      double* K, int64_t sK, int64_t ldk) {
  if (n <= 0 || count <= 0) return DFH_OK;
  DFH_ARG(!kd.multi && kd.n_parts == 1 && (ldk & 1) == 0 && (sK & 1) == 0 &&
          (reinterpret_cast<uintptr_t>(K) & 15) == 0 && count <= 65535);
  KmArgs a;
  a.lower_only = 0;
  a.ec = kExpConsts;
  a.Xp1 = Xp; a.Np1 = Np; a.Xp2 = Xp; a.Np2 = Np;
  a.n1 = (int)n; a.n2 = (int)n; a.P = kd.P; a.n_parts_total = kd.n_parts;
  a.parts = kd.d_parts; a.part_lo = 0; a.part_hi = 1;
  a.outer = kd.outer_scale; a.apply_outer = 1; a.symmetric = 1; a.diag_add = 0.0; a.product = 0;
  a.nt_stores = 0;             // (lock-step batches of small matrices: they are factored right away, out of the caches)
  a.K = K; a.ldk = ldk;
  a.sXp = sXp; a.sNp = sNp; a.sK = sK; a.sBlob = sBlob; a.diag_adds = d_diag_adds;
  const int64_t T = (n + 63) / 64;
  const int smem = ((2 * 64 * (16 + 2) > 32 * (64 + 2) ? 2 * 64 * (16 + 2) : 32 * (64 + 2)) + 2 * 64) * 8;
  hipLaunchKernelGGL((kernmat_sym_kernel<64, 16, 32, 7, true>), dim3((unsigned)(T * (T + 1) / 2), 1, (unsigned)count),
                     dim3(256), smem, ctx->stream, a);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

namespace {

// ---------------------------------------------------------------------------------------
// ESP kernel matrix (DFH_KERNEL_ESP; ESPKernel._child_evaluate, dragonfly/gp/kernel.py:693-726):
//   k_c      = the 1-D SE / Matern kernel of column c on X1[:, c], X2[:, c]   (kern_eval, dist_squared's expansion)
//   p_i      = ((0 + k_0**i) + k_1**i) + ...                                    i = 1..order
//   e_m      = (sum_{i=1..m} (-1)**(i-1) e_{m-i} p_i) / m                       e_0 = 1
//   K[i][j]  = scale * e_order
// No MFMA: every dot product is 1-D, the element is ~d (exp + order) + order^2 fp64 VALU operations with
// nothing to share, so this is a VALU kernel.  A 32 x 32 tile: both operands' scaled columns in LDS
// (x * x is recomputed -- it is the one product the reference's row norm of a single column is), each
// thread 4 elements of one output column; the power sums p_1..p_KB (KB >= order, a register bucket) and,
// in the epilogue, e_0..e_KB live in registers.  k_c**i is a running product (NumPy: pow for i >= 3, so
// ~1 ulp per term apart); the recursion is separate multiply / add / true division, rounding where NumPy
// rounds (the library builds with -ffp-contract=off).
// ---------------------------------------------------------------------------------------
constexpr int ESP_TILE = 32;

struct EspArgs {
  ExpConsts ec;
  const double* Xp1; const double* Xp2;    // packed scaled inputs: one part per column, column c at c * 4
  int n1, n2, P, dim, order;
  const PartDev* parts;                    // [dim] the columns' 1-D kernels
  double scale, diag_add;
  int symmetric, lower_only;
  double* K; long ldk;
};

template <int KB, bool ALL_SE>
__global__ __launch_bounds__(256) void kernmat_esp_kernel(EspArgs p) {
  constexpr int U = KB <= 4 ? 4 : (KB <= 8 ? 2 : 1);   // elements in flight per thread (registers: ~2 KB doubles each)
  extern __shared__ __attribute__((aligned(16))) double esm[];
  double* xa = esm;                                      // [dim][32] the tile's rows of X1
  double* xb = esm + (size_t)p.dim * ESP_TILE;           // [dim][32] the tile's rows of X2
  unsigned ti, tj;
  if (p.symmetric) {                                     // lower-triangular tile enumeration
    const unsigned lin = blockIdx.x;
    ti = (unsigned)((sqrt(8.0 * (double)lin + 1.0) - 1.0) * 0.5);
    while ((unsigned long long)ti * (ti + 1) / 2 > lin) --ti;
    while ((unsigned long long)(ti + 1) * (ti + 2) / 2 <= lin) ++ti;
    tj = lin - (unsigned)((unsigned long long)ti * (ti + 1) / 2);
  } else {
    ti = blockIdx.y; tj = blockIdx.x;
  }
  const long r0 = (long)ti * ESP_TILE, c0 = (long)tj * ESP_TILE;
  for (int idx = threadIdx.x; idx < p.dim * ESP_TILE; idx += 256) {
    const int c = idx >> 5, r = idx & (ESP_TILE - 1);
    const long ra = r0 + r, rb = c0 + r;
    xa[idx] = ra < p.n1 ? p.Xp1[ra * p.P + 4 * c] : 0.0;
    xb[idx] = rb < p.n2 ? p.Xp2[rb * p.P + 4 * c] : 0.0;
  }
  __syncthreads();
  const int tx = threadIdx.x & (ESP_TILE - 1), ty = threadIdx.x >> 5;    // output column; rows ty + 8 a
  const long col = c0 + tx;
  const int order = p.order;
  for (int a0 = 0; a0 < 4; a0 += U) {
    double ps[U][KB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < KB; ++i) ps[u][i] = 0.0;
    for (int c = 0; c < p.dim; ++c) {
      const double y = xb[c * ESP_TILE + tx];
      const double ny = y * y;
      const PartDev& pd = p.parts[c];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const double x = xa[c * ESP_TILE + ty + 8 * (a0 + u)];
        double dsq = (ny + x * x) - 2.0 * (x * y);                          // general_utils.py:66-68
        dsq = dsq < 0.0 ? 0.0 : dsq;
        const double kv = ALL_SE ? pd.scale_c * exp_fast(-dsq / 2, p.ec) : kern_eval(pd, dsq, p.ec);
        double kp = kv;
#pragma unroll
        for (int i = 0; i < KB; ++i) {
          if (i < order) {                                                   // power_sum[i + 1] += k_c ** (i + 1)
            ps[u][i] = ps[u][i] + kp;
            kp = kp * kv;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      double e[KB + 1];
      e[0] = 1.0;
      double last = 1.0;
#pragma unroll
      for (int m = 1; m <= KB; ++m) {
        if (m <= order) {                                                    // kernel.py:718-722
          double acc = 0.0;
#pragma unroll
          for (int i = 1; i <= m; ++i) {
            const double t = e[m - i] * ps[u][i - 1];
            acc = (i & 1) ? acc + t : acc - t;
          }
          e[m] = acc / (double)m;
          last = e[m];
        }
      }
      const long row = r0 + ty + 8 * (a0 + u);
      if (row >= p.n1 || col >= p.n2) continue;
      double res = p.scale * last;                                           // kernel.py:726
      if (p.symmetric) {
        if (row < col) continue;                                             // (diagonal tile: its lower half)
        if (row == col) res = res + p.diag_add;
        p.K[row * p.ldk + col] = res;
        if (!p.lower_only && row != col) p.K[col * p.ldk + row] = res;
      } else {
        p.K[row * p.ldk + col] = res;
      }
    }
  }
}

template <int KB>
int launch_esp(dfh_ctx* ctx, const EspArgs& a, bool all_se, dim3 grid, size_t smem) {
  auto fn = all_se ? reinterpret_cast<const void*>(kernmat_esp_kernel<KB, true>)
                   : reinterpret_cast<const void*>(kernmat_esp_kernel<KB, false>);
  static bool attr_set[DFH_MAX_DEVICES][2] = {};
  if (smem > 64 * 1024 && !attr_set[ctx->device][all_se]) {
    DFH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(2 * sizeof(double) * ESP_MAX_DIM * ESP_TILE)));
    attr_set[ctx->device][all_se] = true;
  }
  if (all_se) hipLaunchKernelGGL((kernmat_esp_kernel<KB, true>), grid, dim3(256), smem, ctx->stream, a);
  else hipLaunchKernelGGL((kernmat_esp_kernel<KB, false>), grid, dim3(256), smem, ctx->stream, a);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

}  // namespace

// K (ldk) = the ESP kernel between two packed inputs; symmetric: Xp1 == Xp2, n1 == n2, diag_add on the
// diagonal, and lower-triangle tiles only (mirrored unless the context builds the lower triangle only).
static int kernmat_esp(dfh_ctx* ctx, const KernDev& kd, const double* Xp1, int64_t n1, const double* Xp2, int64_t n2,
                       bool symmetric, double diag_add, double* K, int64_t ldk) {
  DFH_ARG(kd.esp && kd.n_parts == kd.dim && kd.dim <= ESP_MAX_DIM && kd.P == 4 * kd.dim);
  DFH_ARG(kd.esp_order >= 1 && kd.esp_order <= ESP_MAX_ORDER && kd.esp_order <= kd.dim);
  DFH_ARG(!symmetric || n1 == n2);
  bool all_se = true;
  for (int c = 0; c < kd.n_parts; ++c) all_se = all_se && kd.parts[c].kind == DFH_KERNEL_SE;
  EspArgs a;
  a.ec = kExpConsts;
  a.Xp1 = Xp1; a.Xp2 = Xp2; a.n2 = (int)n2; a.P = kd.P; a.dim = kd.dim; a.order = kd.esp_order;
  a.parts = kd.d_parts; a.scale = kd.outer_scale; a.diag_add = diag_add;
  a.symmetric = symmetric ? 1 : 0;
  a.lower_only = (symmetric && ctx->km_lower_only) ? 1 : 0;
  a.ldk = ldk;
  const size_t smem = 2 * sizeof(double) * (size_t)kd.dim * ESP_TILE;
  const int ord = kd.esp_order;
  auto launch = [&](const EspArgs& b, dim3 grid) -> int {
    if (ord <= 2) return launch_esp<2>(ctx, b, all_se, grid, smem);
    if (ord <= 4) return launch_esp<4>(ctx, b, all_se, grid, smem);
    if (ord <= 8) return launch_esp<8>(ctx, b, all_se, grid, smem);
    if (ord <= 16) return launch_esp<16>(ctx, b, all_se, grid, smem);
    return launch_esp<32>(ctx, b, all_se, grid, smem);
  };
  if (symmetric) {
    const int64_t T = (n1 + ESP_TILE - 1) / ESP_TILE;
    DFH_ARG(T * (T + 1) / 2 < (1LL << 31));
    a.n1 = (int)n1; a.K = K;
    return launch(a, dim3((unsigned)(T * (T + 1) / 2)));
  }
  const int64_t rows_per_launch = 65535LL * ESP_TILE;
  for (int64_t r0 = 0; r0 < n1; r0 += rows_per_launch) {
    const int64_t rr = n1 - r0 < rows_per_launch ? n1 - r0 : rows_per_launch;
    EspArgs b = a;
    b.Xp1 = Xp1 + r0 * kd.P; b.n1 = (int)rr; b.K = K + r0 * ldk;
    DFH_TRY(launch(b, dim3((unsigned)((n2 + ESP_TILE - 1) / ESP_TILE), (unsigned)((rr + ESP_TILE - 1) / ESP_TILE))));
  }
  return DFH_OK;
}

int kernmat_packed(dfh_ctx* ctx, const KernDev& kd, int part_lo, int part_hi, bool apply_outer,
                   const double* Xp1, const double* Np1, int64_t n1, const double* Xp2,
                   const double* Np2, int64_t n2, bool symmetric, double diag_add, double* K,
                   int64_t ldk, const double* mu_alpha, double* mu_out, bool* mu_done) {
  if (mu_done) *mu_done = false;
  if (n1 <= 0 || n2 <= 0) return DFH_OK;
  DFH_ARG(n1 < (1LL << 31) && n2 < (1LL << 31));
  if (kd.esp) {                // the whole ESP kernel in one kernel of its own; no fused posterior mean
    DFH_ARG(part_lo == 0 && part_hi == kd.n_parts && apply_outer);
    return kernmat_esp(ctx, kd, Xp1, n1, Xp2, n2, symmetric, diag_add, K, ldk);
  }
  KmArgs a;
  a.lower_only = 0;
  a.mu_alpha = nullptr; a.mu_part = nullptr; a.mu_out = nullptr; a.mu_nblk = 0;
  a.ec = kExpConsts;
  a.sXp = a.sNp = a.sK = a.sBlob = 0; a.diag_adds = nullptr;
  a.Xp1 = Xp1; a.Np1 = Np1; a.Xp2 = Xp2; a.Np2 = Np2;
  a.n1 = (int)n1; a.n2 = (int)n2; a.P = kd.P; a.n_parts_total = kd.n_parts;
  a.parts = kd.d_parts; a.part_lo = part_lo; a.part_hi = part_hi;
  a.outer = kd.outer_scale; a.apply_outer = apply_outer ? 1 : 0; a.product = kd.product ? 1 : 0;
  a.symmetric = symmetric ? 1 : 0; a.diag_add = diag_add;
  a.lower_only = (symmetric && ctx->km_lower_only) ? 1 : 0;
  a.K = K; a.ldk = ldk;
  {
    static const int nt_env = env_int("DFH_KM_NT", -1);
    a.nt_stores = nt_env >= 0 ? (nt_env != 0) : (kd.P >= 16 && n1 * n2 >= (int64_t)4096 * 4096);
  }
  const bool multi = kd.multi;
  static bool attr_set_dev[DFH_MAX_DEVICES] = {false};
  bool& attr_set = attr_set_dev[ctx->device];
  constexpr int SM4 = ((KM_BM + 128) * KM_KP + KM_BM + 128) * 8;
  constexpr int SM2 = ((KM_BM + 64) * KM_KP + KM_BM + 64) * 8;
  if (!attr_set) {
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_kernel<4, false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, SM4));
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_kernel<2, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, SM2));
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_kernel<2, true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, SM2));
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_kernel<2, true, true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, SM2));
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_kernel<2, true, false, false, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, SM2));
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_kernel<2, true, true, false, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, SM2));
    DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_kernel<2, true, true, true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, SM2));
    attr_set = true;
  }
  if (!multi && part_hi == part_lo + 1 && (ldk & 1) == 0 && (reinterpret_cast<uintptr_t>(K) & 15) == 0 &&
      (n1 + 63) / 64 <= 65535) {
    // 64 x 64 tiles, 16-column operand chunks, 32-row staging: ~20 KB of LDS and 69 VGPRs per
    // workgroup -> 7-8 workgroups per CU whose load / MFMA / exp / store phases overlap.
    static const int sym_cfg = env_int("DFH_KM_CFG", 0);
    auto smem_bytes = [](int TS, int KC, int SR) {
      const int oper = 2 * TS * (KC + 2), stage = SR * (TS + 2);
      return ((oper > stage ? oper : stage) + 2 * TS) * 8;
    };
    if (symmetric) {
      if (sym_cfg == 2) {
        static bool attr_dev[DFH_MAX_DEVICES] = {false};
        bool& attr = attr_dev[ctx->device];
        if (!attr) { DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_sym_kernel<128, 32, 64, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, smem_bytes(128, 32, 64))); attr = true; }
        const int64_t T = (n1 + 127) / 128;
        hipLaunchKernelGGL((kernmat_sym_kernel<128, 32, 64, 2, true>), dim3((unsigned)(T * (T + 1) / 2)), dim3(256), smem_bytes(128, 32, 64), ctx->stream, a);
      } else if (sym_cfg == 1) {
        const int64_t T = (n1 + 63) / 64;
        hipLaunchKernelGGL((kernmat_sym_kernel<64, 32, 64, 4, true>), dim3((unsigned)(T * (T + 1) / 2)), dim3(256), smem_bytes(64, 32, 64), ctx->stream, a);
      } else {
        const int64_t T = (n1 + 63) / 64;
        hipLaunchKernelGGL((kernmat_sym_kernel<64, 16, 32, 7, true>), dim3((unsigned)(T * (T + 1) / 2)), dim3(256), smem_bytes(64, 16, 32), ctx->stream, a);
      }
    } else {
      // strip kernel: SE / Matern (nu = 0.5, 1.5, 2.5), packed width 8 / 16 / 24 / 32, 32-bit in-strip offsets
      static const bool strip_on = env_flag("DFH_KM_STRIP", true);
      const PartDev& hp = kd.parts[part_lo];
      const bool strip_ok = strip_on && (hp.kind == DFH_KERNEL_SE || (hp.kind == DFH_KERNEL_MATERN && hp.p <= 2)) &&
                            hp.kc >= 8 && hp.kc <= 32 && hp.kc % 8 == 0 && kd.P % 2 == 0 && hp.poff % 2 == 0 &&
                            32 * ldk + 64 < (1LL << 31) && (n1 + 127) / 128 <= 65535 &&
                            (reinterpret_cast<uintptr_t>(Xp1) & 15) == 0 && (reinterpret_cast<uintptr_t>(Xp2) & 15) == 0;
      static const bool mu_fused = env_flag("DFH_KM_FUSED_MEAN", true);
      if (strip_ok && mu_fused && mu_alpha && mu_out && mu_done) {
        a.mu_nblk = (int)((n2 + KM_MU_BLOCK - 1) / KM_MU_BLOCK);
        DFH_TRY(scratch_get(ctx, SCR_MUPART, (size_t)n1 * a.mu_nblk * 8, (void**)&a.mu_part));
        a.mu_alpha = mu_alpha; a.mu_out = mu_out;
        *mu_done = true;
      }
      if (strip_ok) {
        if (hp.kind == DFH_KERNEL_SE) {
          for (int i = 0; i < 12; ++i) a.ec.c[i] *= hp.scale_c;      // scale folded into the exp polynomial
          return launch_strip<DFH_KERNEL_SE, 0>(ctx, a, hp.kc / 4);
        }
        if (hp.p == 0) return launch_strip<DFH_KERNEL_MATERN, 0>(ctx, a, hp.kc / 4);
        if (hp.p == 1) return launch_strip<DFH_KERNEL_MATERN, 1>(ctx, a, hp.kc / 4);
        return launch_strip<DFH_KERNEL_MATERN, 2>(ctx, a, hp.kc / 4);
      }
      dim3 grid((unsigned)((n2 + 63) / 64), (unsigned)((n1 + 63) / 64));
      hipLaunchKernelGGL((kernmat_sym_kernel<64, 16, 32, 7, false>), grid, dim3(256), smem_bytes(64, 16, 32), ctx->stream, a);
    }
    DFH_LAUNCH_CHECK();
    return DFH_OK;
  }
  if (multi && symmetric && kd.stationary && !kd.nested && (ldk & 1) == 0 && (reinterpret_cast<uintptr_t>(K) & 15) == 0 &&
      (n1 + 63) / 64 <= 65535 && kd.P % 2 == 0 && (reinterpret_cast<uintptr_t>(Xp1) & 15) == 0) {
    // symmetric Gram of an additive / product kernel: lower-triangle tiles, parts adjacent and <= 16 columns wide
    static const bool symmulti_on = env_flag("DFH_KM_SYMMULTI", true);
    bool ok = symmulti_on;
    for (int g = part_lo; g < part_hi && ok; ++g) {
      ok = kd.parts[g].kc <= 16 && kd.parts[g].poff % 2 == 0 &&
           (g == part_lo || kd.parts[g].poff == kd.parts[g - 1].poff + kd.parts[g - 1].kc);
    }
    if (ok) {
      constexpr int KCM = 16, SRM = 32;
      constexpr int oper = 2 * 64 * (KCM + 2), stage = SRM * 66;
      constexpr int smem = ((oper > stage ? oper : stage) + 2 * (KCM / 4) * 64) * 8;
      const int64_t T = (n1 + 63) / 64;
      hipLaunchKernelGGL((kernmat_symmulti_kernel<KCM, SRM, 5>), dim3((unsigned)(T * (T + 1) / 2)), dim3(256), smem,
                         ctx->stream, a);
      DFH_LAUNCH_CHECK();
      return DFH_OK;
    }
  }
  bool ham_pow = false;       // a Hamming part next to a polynomial / exponential-decay one: the instance with their pow()
  for (const PartDev& pd : kd.parts) ham_pow = ham_pow || pd.kind == DFH_KERNEL_POLY || pd.kind == DFH_KERNEL_EXPDECAY;
  const int64_t rows_per_launch = 65535LL * KM_BM;
  for (int64_t r0 = 0; r0 < n1; r0 += rows_per_launch) {
    const int64_t rr = n1 - r0 < rows_per_launch ? n1 - r0 : rows_per_launch;
    KmArgs b = a;
    b.Xp1 = Xp1 + r0 * kd.P; b.Np1 = Np1 + r0 * kd.n_parts; b.n1 = (int)rr; b.K = K + r0 * ldk;
    if (r0 != 0) b.symmetric = 0;    // only reachable for n1 > 8M rows; diagonal handled in slab 0
    if (multi) {
      dim3 grid((unsigned)((n2 + 63) / 64), (unsigned)((rr + KM_BM - 1) / KM_BM));
      if (kd.hamming && kd.nested) hipLaunchKernelGGL((kernmat_kernel<2, true, true, true, true>), grid, dim3(256), SM2, ctx->stream, b);
      else if (kd.hamming && ham_pow) hipLaunchKernelGGL((kernmat_kernel<2, true, true, false, true>), grid, dim3(256), SM2, ctx->stream, b);
      else if (kd.hamming) hipLaunchKernelGGL((kernmat_kernel<2, true, false, false, true>), grid, dim3(256), SM2, ctx->stream, b);
      else if (kd.nested) hipLaunchKernelGGL((kernmat_kernel<2, true, true, true>), grid, dim3(256), SM2, ctx->stream, b);
      else if (kd.stationary) hipLaunchKernelGGL((kernmat_kernel<2, true>), grid, dim3(256), SM2, ctx->stream, b);
      else hipLaunchKernelGGL((kernmat_kernel<2, true, true>), grid, dim3(256), SM2, ctx->stream, b);
    } else {
      dim3 grid((unsigned)((n2 + 127) / 128), (unsigned)((rr + KM_BM - 1) / KM_BM));
      hipLaunchKernelGGL((kernmat_kernel<4, false>), grid, dim3(256), SM4, ctx->stream, b);
    }
    DFH_LAUNCH_CHECK();
  }
  return DFH_OK;
}
