"""Long-K LOWER products C -= A.A^T (the covariance SYRK of a Thompson block, one matrix of the batch): time per
launch for one tree (DFH_ROOT).  SHAPES = comma-separated NxK."""
import os, sys
root = os.environ.get('DFH_ROOT', os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root)
import numpy as np
from dragonfly_amd.engine import get_engine
from dragonfly_amd._lib import check
eng = get_engine()
reps = int(os.environ.get('REPS', '3'))
for n, K in [tuple(int(v) for v in s.split('x')) for s in os.environ.get('SHAPES', '4096x16384,16384x4096').split(',')]:
  A = eng.empty((n, K)); Cd = eng.empty((n, n))
  gen = np.random.Generator(np.random.Philox(n + K))
  eng.random_candidates(n, K, bounds=[[-0.5, 0.5]] * K, rng=gen, out=A)
  eng.random_candidates(n, n, rng=gen, out=Cd)
  def run():
    check(eng.lib.dfh_gemm(eng.ctx, 0, n, n, K, -1.0, A.ptr, K, A.ptr, K, 1.0, Cd.ptr, n, 1))
  run()
  ts = []
  for _ in range(reps):
    eng.timer_begin(); run(); ts.append(eng.timer_end())
  ms = sorted(ts)[len(ts) // 2]
  print('%s  LOWER %d x %d x %d: %8.3f ms  %5.1f TF/s' % (os.path.basename(root), n, n, K, ms,
        n * (n + 1.0) * K / (ms * 1e-3) / 1e12), flush=True)
  A.free(); Cd.free()
