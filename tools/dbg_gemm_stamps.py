# needs a library built with the diagnostics hooks: python -m dragonfly_amd.build --force --debug-hooks (include/dfhip_debug.h)
# Where a wave of the 128-tile fp64 GEMM spends its K loop: shares of the s_memtime stamps of the stamped instantiation.
# The stamps wait for their own value and perturb the loop: the shares are the result, not this build's run time.
import ctypes as C, sys, os
sys.path.insert(0, os.environ.get('DFH_ROOT', os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from dragonfly_amd.engine import get_engine
from dragonfly_amd._lib import check
eng = get_engine()
lib = eng.lib
lib.dfh_debug_gemm_stamps.restype = C.c_int
lib.dfh_debug_gemm_stamps.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
NAMES = ['loads out + LDS reads + MFMA group 0', 'wait for the global loads', 'LDS writes + lgkmcnt(0)', 'barrier', 'LDS reads + MFMA group 1']
shapes = [tuple(int(v) for v in s.split('x')) for s in os.environ.get('SHAPES', '8192x8192x8192,262144x512x8192').split(',')]
for M, N, K in shapes:
  A = eng.empty((M, K)); B = eng.empty((N, K)); Cd = eng.empty((M, N))
  gen = np.random.Generator(np.random.Philox(K))
  eng.random_candidates(M, K, bounds=[[-0.5, 0.5]] * K, rng=gen, out=A)
  eng.random_candidates(N, K, bounds=[[-0.5, 0.5]] * K, rng=gen, out=B)
  eng.random_candidates(M, N, rng=gen, out=Cd)
  out = (C.c_double * 8)()
  for prio in (0, 1):
    for rep in range(2):              # the second launch is the one reported (warm caches, clocks up)
      check(lib.dfh_debug_gemm_stamps(eng.ctx, M, N, K, A.ptr, B.ptr, Cd.ptr, prio, out))
    tot = sum(out[:5])
    print('%d x %d x %d, priority flips %s: %d waves, %.0f chunks per wave, %.1f shader cycles per chunk' % (
      M, N, K, 'on' if prio else 'off', out[6], out[5] / out[6], tot / max(out[5], 1)))
    for name, v in zip(NAMES, out[:5]):
      print('  %-40s %6.2f %%   %7.1f cycles per chunk' % (name, 100.0 * v / tot, v / max(out[5], 1)))
    sys.stdout.flush()
  if K % 32 == 0:
    # the solo kernel (one workgroup per CU, chunks of 32 = 128 MFMAs per wave): the barrier and the whole chunk only
    for rep in range(2):
      check(lib.dfh_debug_gemm_stamps(eng.ctx, M, N, K, A.ptr, B.ptr, Cd.ptr, 2, out))
    print('%d x %d x %d, solo kernel: %d waves, %.0f stamped chunks per wave, %.1f shader cycles per chunk of 32, barrier %.1f cycles (%.2f %%)' % (
      M, N, K, out[6], out[5] / out[6], out[1] / max(out[5], 1), out[0] / max(out[5], 1), 100.0 * out[0] / max(out[1], 1)))
    sys.stdout.flush()
  A.free(); B.free(); Cd.free()
