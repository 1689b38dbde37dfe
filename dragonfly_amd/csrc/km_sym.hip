// Kernel matrices through LDS-staged 16-byte stores: the single-part kernel (symmetric Gram matrices as their lower
// triangle of tiles, mirrored; cross matrices the strip kernel does not take; lock-step batches of small Gram matrices)
// and the symmetric kernel of several adjacent stationary parts.
#include "kernmat.h"

namespace {

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

constexpr int sym_smem_bytes(int TS, int KC, int SR) {
  const int oper = 2 * TS * (KC + 2), stage = SR * (TS + 2);
  return ((oper > stage ? oper : stage) + 2 * TS) * 8;
}

unsigned lower_tiles(int64_t n, int ts) {
  const int64_t T = (n + ts - 1) / ts;
  return (unsigned)(T * (T + 1) / 2);
}

}  // namespace

bool km_single_aligned(const KmCall& c) {
  return !c.kd->multi && c.part_hi == c.part_lo + 1 && (c.ldk & 1) == 0 && (reinterpret_cast<uintptr_t>(c.K) & 15) == 0 &&
         (c.a.n + 63) / 64 <= 65535;
}

// DFH_KM_CFG: 0 = 64 x 64 tiles, 16-column operand chunks, 32-row staging: ~20 KB of LDS and 69 VGPRs per
// workgroup -> 7-8 workgroups per CU whose load / MFMA / exp / store phases overlap; 1 = 32-column chunks, 64-row
// staging; 2 = 128 x 128 tiles
int km_launch_sym(dfh_ctx* ctx, const KmCall& c) {
  const KmArgs a = km_args(c);
  const int cfg = km_switches().sym_cfg;
  if (cfg == 2) {
    static bool attr_dev[DFH_MAX_DEVICES] = {false};
    bool& attr = attr_dev[ctx->device];
    if (!attr) {
      DFH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernmat_sym_kernel<128, 32, 64, 2, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, sym_smem_bytes(128, 32, 64)));
      attr = true;
    }
    hipLaunchKernelGGL((kernmat_sym_kernel<128, 32, 64, 2, true>), dim3(lower_tiles(c.a.n, 128)), dim3(256),
                       sym_smem_bytes(128, 32, 64), ctx->stream, a);
  } else if (cfg == 1) {
    hipLaunchKernelGGL((kernmat_sym_kernel<64, 32, 64, 4, true>), dim3(lower_tiles(c.a.n, 64)), dim3(256),
                       sym_smem_bytes(64, 32, 64), ctx->stream, a);
  } else {
    hipLaunchKernelGGL((kernmat_sym_kernel<64, 16, 32, 7, true>), dim3(lower_tiles(c.a.n, 64)), dim3(256),
                       sym_smem_bytes(64, 16, 32), ctx->stream, a);
  }
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

int km_launch_cross_lds(dfh_ctx* ctx, const KmCall& c) {
  const KmArgs a = km_args(c);
  dim3 grid((unsigned)((c.b.n + 63) / 64), (unsigned)((c.a.n + 63) / 64));
  hipLaunchKernelGGL((kernmat_sym_kernel<64, 16, 32, 7, false>), grid, dim3(256), sym_smem_bytes(64, 16, 32), ctx->stream, a);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}

// symmetric Gram of an additive / product kernel: lower-triangle tiles, parts adjacent and <= 16 columns wide
bool km_symmulti_ok(const KmCall& c) {
  const KernDev& kd = *c.kd;
  if (!(kd.multi && c.symmetric && kd.stationary && !kd.nested && (c.ldk & 1) == 0 &&
        (reinterpret_cast<uintptr_t>(c.K) & 15) == 0 && (c.a.n + 63) / 64 <= 65535 && kd.P % 2 == 0 &&
        (reinterpret_cast<uintptr_t>(c.a.Xp) & 15) == 0))
    return false;
  bool ok = km_switches().symmulti;
  for (int g = c.part_lo; g < c.part_hi && ok; ++g) {
    ok = kd.parts[g].kc <= 16 && kd.parts[g].poff % 2 == 0 &&
         (g == c.part_lo || kd.parts[g].poff == kd.parts[g - 1].poff + kd.parts[g - 1].kc);
  }
  return ok;
}

int km_launch_symmulti(dfh_ctx* ctx, const KmCall& c) {
  constexpr int KCM = 16, SRM = 32;
  constexpr int oper = 2 * 64 * (KCM + 2), stage = SRM * 66;
  constexpr int smem = ((oper > stage ? oper : stage) + 2 * (KCM / 4) * 64) * 8;
  const KmArgs a = km_args(c);
  hipLaunchKernelGGL((kernmat_symmulti_kernel<KCM, SRM, 5>), dim3(lower_tiles(c.a.n, 64)), dim3(256), smem, ctx->stream, a);
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
  const KmPts pts{Xp, Np, n};
  KmArgs a = km_args(KmCall{&kd, 0, 1, true, pts, pts, true, 0.0, false, K, ldk, nullptr});
  a.nt_stores = 0;             // (lock-step batches of small matrices: they are factored right away, out of the caches)
  a.sXp = sXp; a.sNp = sNp; a.sK = sK; a.sBlob = sBlob; a.diag_adds = d_diag_adds;
  hipLaunchKernelGGL((kernmat_sym_kernel<64, 16, 32, 7, true>), dim3(lower_tiles(n, 64), 1, (unsigned)count), dim3(256),
                     sym_smem_bytes(64, 16, 32), ctx->stream, a);
  DFH_LAUNCH_CHECK();
  return DFH_OK;
}
