// extern "C" entry points of libdfhip.so that work on plain matrices (see include/dfhip.h for the contract and the
// reference functions each one replaces); the GP object is in gp_fit.hip, gp_posterior.hip and gp_draw.hip.
#include "common.h"
#ifdef DFH_DEBUG_HOOKS
#include <chrono>
#endif

// ---------------------------------------------------------------------------------------------
// What dfh_kernel_matrix and dfh_dist_squared share: stage X1 (and X2, null for the symmetric case), pack them for kd,
// let `build` make the matrix on the device from the packed points (the same twice: symmetric) and copy it back;
// kd is freed.
static int matrix_of_inputs(dfh_ctx* ctx, KernDev& kd, int64_t d, const double* X1, int64_t n1, const double* X2, int64_t n2,
                            double* out, const std::function<int(KmPts, KmPts, double*)>& build) {
  const bool sym = (X2 == nullptr);
  auto body = [&]() -> int {
    const double *dX1 = nullptr, *dX2 = nullptr;
    DFH_TRY(to_device(ctx, X1, (size_t)n1 * d * 8, SCR_STAGE_A, &dX1));
    if (!sym) DFH_TRY(to_device(ctx, X2, (size_t)n2 * d * 8, SCR_STAGE_B, &dX2));
    char* buf = nullptr;
    const size_t b1 = ((size_t)n1 * kd.P * 8 + 255) / 256 * 256, bn1 = ((size_t)n1 * kd.n_parts * 8 + 255) / 256 * 256;
    const size_t b2 = sym ? 0 : ((size_t)n2 * kd.P * 8 + 255) / 256 * 256, bn2 = sym ? 0 : (size_t)n2 * kd.n_parts * 8;
    DFH_TRY(scratch_get(ctx, SCR_XS, b1 + bn1 + b2 + bn2 + 256, (void**)&buf));
    double* Xp1 = reinterpret_cast<double*>(buf);
    double* Np1 = reinterpret_cast<double*>(buf + b1);
    double* Xp2 = sym ? Xp1 : reinterpret_cast<double*>(buf + b1 + bn1);
    double* Np2 = sym ? Np1 : reinterpret_cast<double*>(buf + b1 + bn1 + b2);
    DFH_TRY(pack_scaled(ctx, kd, 0, kd.n_parts, false, dX1, n1, d, Xp1, Np1));
    if (!sym) DFH_TRY(pack_scaled(ctx, kd, 0, kd.n_parts, false, dX2, n2, d, Xp2, Np2));
    const bool dev_out = is_device_ptr(out);
    double* Kd = out;
    if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n1 * n2 * 8, (void**)&Kd));
    DFH_TRY(build(KmPts{Xp1, Np1, n1}, KmPts{Xp2, Np2, n2}, Kd));
    if (!dev_out) DFH_TRY(from_device(ctx, out, Kd, (size_t)n1 * n2 * 8));
    return DFH_OK;
  };
  const int rc = body();
  (void)hipStreamSynchronize(ctx->stream);
  kerndev_free(&kd);
  return rc;
}

extern "C" int dfh_kernel_matrix(dfh_ctx* ctx, const dfh_kernel_desc* k, const double* X1, int64_t n1,
                                 const double* X2, int64_t n2, double diag_add, double* K_out) {
  DFH_ARG(ctx && k && K_out);
  DFH_ARG(n1 >= 0 && (X2 == nullptr || n2 >= 0));
  const bool sym = (X2 == nullptr);
  if (sym) n2 = n1;
  if (n1 == 0 || n2 == 0) return DFH_OK;     // kernel.py:81-82: empty result
  DFH_ARG(X1 != nullptr);
  DFH_HIP(hipSetDevice(ctx->device));
  KernDev kd;
  const int rc = kerndev_build(ctx, k, &kd);
  if (rc != DFH_OK) { kerndev_free(&kd); return rc; }
  return matrix_of_inputs(ctx, kd, k->dim, X1, n1, X2, n2, K_out, [&](KmPts p1, KmPts p2, double* Kd) -> int {
    SectionTimer t(ctx, sym ? DFH_T_KERNMAT : DFH_T_CROSS);
    if (sym) return kernmat_gram(ctx, kd, 0, kd.n_parts, true, p1, diag_add, Kd, n2);
    return kernmat_cross(ctx, kd, 0, kd.n_parts, true, p1, p2, Kd, n2);
  });
}

extern "C" int dfh_dist_squared(dfh_ctx* ctx, const double* X1, int64_t n1, const double* X2, int64_t n2,
                                int64_t d, double* D_out) {
  DFH_ARG(ctx && D_out && d >= 1 && n1 >= 0 && n2 >= 0);
  if (n1 == 0 || n2 == 0) return DFH_OK;
  DFH_ARG(X1 && X2);
  DFH_HIP(hipSetDevice(ctx->device));
  KernDev kd;
  const int rc = kerndev_build_dist(ctx, (int)d, &kd);
  if (rc != DFH_OK) { kerndev_free(&kd); return rc; }
  return matrix_of_inputs(ctx, kd, d, X1, n1, X2, n2, D_out, [&](KmPts p1, KmPts p2, double* Kd) -> int {
    return kernmat_cross(ctx, kd, 0, 1, false, p1, p2, Kd, n2);
  });
}

extern "C" int dfh_gemm(dfh_ctx* ctx, int transb, int64_t M, int64_t N, int64_t K, double alpha,
                        const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
                        double* C, int64_t ldc, int lower_only) {
  DFH_ARG(ctx && C && M >= 0 && N >= 0 && K >= 0);
  if (M == 0 || N == 0) return DFH_OK;
  DFH_ARG((K == 0 || (A && B)) && lda >= K && ldc >= N && ldb >= (transb ? N : K));
  DFH_HIP(hipSetDevice(ctx->device));
  const double *dA = nullptr, *dB = nullptr, *dCin = nullptr;
  DFH_TRY(to_device(ctx, A, (size_t)M * lda * 8, SCR_STAGE_A, &dA));
  DFH_TRY(to_device(ctx, B, (size_t)(transb ? K : N) * ldb * 8, SCR_STAGE_B, &dB));
  const bool dev_out = is_device_ptr(C);
  double* dC = C;
  if (!dev_out) {
    DFH_TRY(scratch_get(ctx, SCR_STAGE_C, (size_t)M * ldc * 8, (void**)&dC));
    DFH_HIP(hipMemcpyAsync(dC, C, (size_t)M * ldc * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  dCin = dC;
  int flags = (transb ? GEMM_TRANSB : 0) | (lower_only ? GEMM_LOWER : 0);
  DFH_TRY(gemm_f64(ctx, flags, M, N, K, alpha, dA, lda, dB, ldb, beta, dCin, ldc, dC, ldc));
  if (!dev_out) DFH_TRY(from_device(ctx, C, dC, (size_t)M * ldc * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

extern "C" int dfh_cholesky(dfh_ctx* ctx, double* A, int64_t n, int64_t* info_pivot) {
  DFH_ARG(ctx && n >= 0);
  if (info_pivot) *info_pivot = 0;
  if (n == 0) return DFH_OK;
  DFH_ARG(A != nullptr);
  DFH_HIP(hipSetDevice(ctx->device));
  const bool dev = is_device_ptr(A);
  double* dA = A;
  if (!dev) {
    DFH_TRY(scratch_get(ctx, SCR_TSL, (size_t)n * n * 8, (void**)&dA));
    DFH_HIP(hipMemcpyAsync(dA, A, (size_t)n * n * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  int rc;
  {
    SectionTimer t(ctx, DFH_T_CHOL);
    // a host matrix can be uploaded again: the schedules that may need a second attempt are open to it
    const std::function<int()> reupload = [&]() -> int {
      DFH_HIP(hipMemcpyAsync(dA, A, (size_t)n * n * 8, hipMemcpyHostToDevice, ctx->stream));
      return DFH_OK;
    };
    rc = cholesky_device(ctx, dA, n, n, nullptr, info_pivot, 1, 0, 0, nullptr, false, dev ? nullptr : &reupload);
  }
  if (rc != DFH_OK) return rc;
  DFH_TRY(zero_upper(ctx, dA, n, n));
  if (!dev) DFH_TRY(from_device(ctx, A, dA, (size_t)n * n * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

extern "C" int dfh_stable_cholesky(dfh_ctx* ctx, const double* M_in, int64_t n, double* L_out,
                                   int32_t* jitter_power) {
  DFH_ARG(ctx && n >= 0);
  if (jitter_power) *jitter_power = INT32_MIN;
  if (n == 0) return DFH_OK;                         // general_utils.py:174-175
  DFH_ARG(M_in && L_out);
  DFH_HIP(hipSetDevice(ctx->device));
  const double* dM = nullptr;
  DFH_TRY(to_device(ctx, M_in, (size_t)n * n * 8, SCR_TSK, &dM));
  const bool dev_out = is_device_ptr(L_out);
  double* dL = L_out;
  if (!dev_out) DFH_TRY(scratch_get(ctx, SCR_TSL, (size_t)n * n * 8, (void**)&dL));
  auto rebuild = [&]() -> int { return copy_matrix(ctx, dM, n, dL, n, n, n); };
  DFH_TRY(rebuild());
  int rc;
  {
    SectionTimer t(ctx, DFH_T_CHOL);
    rc = stable_cholesky_device(ctx, dL, n, nullptr, true, rebuild, jitter_power, nullptr);
  }
  if (rc != DFH_OK) return rc;
  DFH_TRY(zero_upper(ctx, dL, n, n));
  if (!dev_out) DFH_TRY(from_device(ctx, L_out, dL, (size_t)n * n * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

extern "C" int dfh_solve_triangular(dfh_ctx* ctx, const double* L, int64_t n, int upper, const double* b,
                                    int64_t nrhs, double* x_out) {
  DFH_ARG(ctx && n >= 0 && nrhs >= 1);
  if (n == 0) return DFH_OK;
  DFH_ARG(L && b && x_out);
  DFH_HIP(hipSetDevice(ctx->device));
  const double *dL = nullptr, *dB = nullptr;
  DFH_TRY(to_device(ctx, L, (size_t)n * n * 8, SCR_TSL, &dL));
  DFH_TRY(to_device(ctx, b, (size_t)n * nrhs * 8, SCR_STAGE_B, &dB));
  const int64_t nblk = (n + CHOL_NB - 1) / CHOL_NB;
  double* inv = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_CHOLINV, (size_t)inv_buffer_doubles(n) * 8, (void**)&inv));
  std::vector<int> refine((size_t)nblk, 0);
  DFH_TRY(tri_block_inverses(ctx, dL, n, n, inv, refine.data()));
  double* dX = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_OUT, (size_t)n * nrhs * 8, (void**)&dX));
  if (nrhs == 1) {
    DFH_HIP(hipMemcpyAsync(dX, dB, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (!upper) DFH_TRY(trsv_forward(ctx, dL, n, n, inv, dX, refine.data()));
    else DFH_TRY(trsv_backward(ctx, dL, n, n, inv, dX, refine.data()));
  } else {
    double* Bt = nullptr;
    DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n * nrhs * 8, (void**)&Bt));
    DFH_TRY(transpose_matrix(ctx, dB, nrhs, Bt, n, n, nrhs));       // Bt[nrhs][n]
    {
      SectionTimer t(ctx, DFH_T_TRSM);
      if (!upper) DFH_TRY(trsm_rows(ctx, dL, n, n, inv, Bt, nrhs, n, refine.data()));
      else DFH_TRY(trsm_rows_backward(ctx, dL, n, n, inv, Bt, nrhs, n, refine.data()));
    }
    DFH_TRY(transpose_matrix(ctx, Bt, n, dX, nrhs, nrhs, n));
  }
  DFH_TRY(from_device(ctx, x_out, dX, (size_t)n * nrhs * 8));
  DFH_HIP(hipStreamSynchronize(ctx->stream));
  return DFH_OK;
}

#ifdef DFH_DEBUG_HOOKS      // diagnostics: built only with `python -m dragonfly_amd.build --debug-hooks` (include/dfhip_debug.h)
// Diagnostics hook (not part of the product path): do kernels on the bulk stream and on the main /
// panel streams actually run concurrently?  Enqueues `n_big` large GEMMs on stream A and `n_small`
// tiny kernels on stream B and reports the time of each alone and together.
// which: 0 = A is bulk, B is main; 1 = A is main, B is side; 2 = A is bulk, B is side
extern "C" int dfh_debug_overlap(dfh_ctx* ctx, int which, int n_big, int n_small, double* out_ms /*[4]*/) {
  DFH_ARG(ctx && out_ms);
  hipStream_t A = (which == 1) ? ctx->main_stream : ctx->bulk;
  hipStream_t B = (which == 0) ? ctx->main_stream : ctx->side;
  const int64_t M = 16384, N = 512, K = 4096;
  double *a = nullptr, *b = nullptr, *c = nullptr, *v = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)M * K * 8, (void**)&a));
  DFH_TRY(scratch_get(ctx, SCR_TSK, (size_t)N * K * 8, (void**)&b));
  DFH_TRY(scratch_get(ctx, SCR_TMP, (size_t)M * N * 8, (void**)&c));
  DFH_TRY(scratch_get(ctx, SCR_VEC, 1 << 20, (void**)&v));
  DFH_TRY(fill_f64(ctx, a, M * K, 0.5));
  DFH_TRY(fill_f64(ctx, b, N * K, 0.25));
  DFH_HIP(hipDeviceSynchronize());
  int least = 0, greatest = 0;
  DFH_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  out_ms[3] = least * 100.0 + greatest;
  auto run = [&](bool big, bool small, double* ms) -> int {
    DFH_HIP(hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    if (big) {
      StreamSwap sw(ctx, A);
      for (int i = 0; i < n_big; ++i) DFH_TRY(gemm_f64(ctx, 0, M, N, K, 1.0, a, K, b, K, 0.0, nullptr, 0, c, N));
    }
    if (small) {
      StreamSwap sw(ctx, B);
      for (int i = 0; i < n_small; ++i) {
        if (which >= 10) DFH_TRY(fill_f64(ctx, v, 4096, 1.0));
        else DFH_TRY(gemm_f64(ctx, 0, 64, 64, 64, 1.0, a, K, b, K, 0.0, nullptr, 0, v, 64));   // 38 KB LDS, 1 workgroup
      }
    }
    DFH_HIP(hipStreamSynchronize(B));
    auto t1 = std::chrono::steady_clock::now();
    DFH_HIP(hipDeviceSynchronize());
    auto t2 = std::chrono::steady_clock::now();
    ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    ms[1] = std::chrono::duration<double, std::milli>(t2 - t0).count();
    return DFH_OK;
  };
  double m[2];
  DFH_TRY(run(true, false, m));  out_ms[0] = m[1];            // big alone
  DFH_TRY(run(false, true, m));  out_ms[1] = m[1];            // small alone
  DFH_TRY(run(true, true, m));   out_ms[2] = m[0];            // small-stream completion time when both run
  out_ms[3] += m[1] * 1e6;                                    // total together (packed: ms*1e6 + prio)
  return DFH_OK;
}

// Diagnostics hook: achievable pure-write HBM bandwidth (the kernel-matrix build is write-only).
__global__ void k_dbg_fill16(double2_t* p, long n2, double v) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const double2_t vv = (double2_t){v, v};
  for (; i < n2; i += stride) p[i] = vv;
}
__global__ void k_dbg_copy16(const double2_t* __restrict__ s, double2_t* __restrict__ d, long n2) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < n2; i += stride) d[i] = s[i];
}
extern "C" int dfh_debug_write_bw(dfh_ctx* ctx, double gbytes, double* out /*[3]: fill16 TB/s, memset TB/s, copy TB/s (r+w)*/) {
  DFH_ARG(ctx && out && gbytes > 0.01 && gbytes < 16);
  const long n2 = (long)(gbytes * 1e9 / 16);
  double2_t *a = nullptr, *b = nullptr;
  DFH_TRY(scratch_get(ctx, SCR_KCT, (size_t)n2 * 16, (void**)&a));
  DFH_TRY(scratch_get(ctx, SCR_KCT2, (size_t)n2 * 16, (void**)&b));
  hipEvent_t e0, e1;
  DFH_HIP(hipEventCreate(&e0)); DFH_HIP(hipEventCreate(&e1));
  float ms;
  for (int grid : {2048, 8192}) {
    hipLaunchKernelGGL(k_dbg_fill16, dim3(grid), dim3(256), 0, ctx->stream, a, n2, 1.0);
  }
  DFH_HIP(hipEventRecord(e0, ctx->stream));
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(k_dbg_fill16, dim3(4096), dim3(256), 0, ctx->stream, a, n2, 2.0);
  DFH_HIP(hipEventRecord(e1, ctx->stream)); DFH_HIP(hipEventSynchronize(e1));
  DFH_HIP(hipEventElapsedTime(&ms, e0, e1)); out[0] = 5.0 * n2 * 16 / (ms * 1e-3) / 1e12;
  DFH_HIP(hipEventRecord(e0, ctx->stream));
  for (int r = 0; r < 5; ++r) DFH_HIP(hipMemsetAsync(a, 0, (size_t)n2 * 16, ctx->stream));
  DFH_HIP(hipEventRecord(e1, ctx->stream)); DFH_HIP(hipEventSynchronize(e1));
  DFH_HIP(hipEventElapsedTime(&ms, e0, e1)); out[1] = 5.0 * n2 * 16 / (ms * 1e-3) / 1e12;
  DFH_HIP(hipEventRecord(e0, ctx->stream));
  for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(k_dbg_copy16, dim3(4096), dim3(256), 0, ctx->stream, a, b, n2);
  DFH_HIP(hipEventRecord(e1, ctx->stream)); DFH_HIP(hipEventSynchronize(e1));
  DFH_HIP(hipEventElapsedTime(&ms, e0, e1)); out[2] = 5.0 * 2.0 * n2 * 16 / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return DFH_OK;
}
#endif  // DFH_DEBUG_HOOKS
