// Kernel matrices, the strip kernel: cross matrices of single-part SE / Matern kernels without LDS, with the posterior
// mean riding along where the caller wants it.
#include "kernmat.h"
#include <type_traits>

namespace {

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
  const long waves_env = km_switches().waves, want_waves = waves_env > 0 ? waves_env : 8192;
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

}  // namespace

// SE / Matern (nu = 0.5, 1.5, 2.5), packed width 8 / 16 / 24 / 32, 32-bit in-strip offsets
bool km_strip_ok(const KmCall& c) {
  const PartDev& hp = c.kd->parts[c.part_lo];
  return km_switches().strip && (hp.kind == DFH_KERNEL_SE || (hp.kind == DFH_KERNEL_MATERN && hp.p <= 2)) &&
         hp.kc >= 8 && hp.kc <= 32 && hp.kc % 8 == 0 && c.kd->P % 2 == 0 && hp.poff % 2 == 0 &&
         32 * c.ldk + 64 < (1LL << 31) && (c.a.n + 127) / 128 <= 65535 &&
         (reinterpret_cast<uintptr_t>(c.a.Xp) & 15) == 0 && (reinterpret_cast<uintptr_t>(c.b.Xp) & 15) == 0;
}

int km_launch_strip(dfh_ctx* ctx, const KmCall& c) {
  const PartDev& hp = c.kd->parts[c.part_lo];
  KmArgs a = km_args(c);
  if (km_switches().fused_mean && c.mean && c.mean->alpha && c.mean->out) {      // the mean rides along
    a.mu_nblk = (int)((c.b.n + KM_MU_BLOCK - 1) / KM_MU_BLOCK);
    DFH_TRY(scratch_get(ctx, SCR_MUPART, (size_t)c.a.n * a.mu_nblk * 8, (void**)&a.mu_part));
    a.mu_alpha = c.mean->alpha; a.mu_out = c.mean->out;
    c.mean->done = true;
    ctx->km_route = KM_ROUTE_STRIP_MEAN;
  }
  if (hp.kind == DFH_KERNEL_SE) {
    for (int i = 0; i < 12; ++i) a.ec.c[i] *= hp.scale_c;      // scale folded into the exp polynomial
    return launch_strip<DFH_KERNEL_SE, 0>(ctx, a, hp.kc / 4);
  }
  if (hp.p == 0) return launch_strip<DFH_KERNEL_MATERN, 0>(ctx, a, hp.kc / 4);
  if (hp.p == 1) return launch_strip<DFH_KERNEL_MATERN, 1>(ctx, a, hp.kc / 4);
  return launch_strip<DFH_KERNEL_MATERN, 2>(ctx, a, hp.kc / 4);
}
