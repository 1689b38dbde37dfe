"""Times the joint draw with evaluations in progress on one GPU: the fused device route (dfh_gp_draw) against the host
route it replaces, and one draw against 64 draws of the same block.

    python tools/draw_timing.py [--n 2048 --d 6 --m 8192 --q 3] [--out profiles/draw_timing.json] [--time-limit 600]

  host_route   GP.draw_samples_with_hallucinated_observations(1, Xs, Xh) with the fitted handle's capability masked:
               the code path before the fused draw -- the m x m covariance to the host, back for stable_cholesky, the
               factor to the host, back for the product with the normals
  fused        the same call on the fused route: covariance, factor and product stay in HBM
  draws_1 / draws_64   FittedGP.draw of one block of m candidates with S = 1 and S = 64 (samples returned to the host)

Medians of 5 wall-clock samples after one warm-up call; every call ends with its result on the host, so each sample
ends in a device synchronise.  The process ends itself at the time limit (SIGALRM).  Prints one JSON line.
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 5, 1


def median_ms(fn):
  for _ in range(WARM):
    fn()
  ts = []
  for _ in range(REPS):
    t0 = time.perf_counter()
    fn()
    ts.append((time.perf_counter() - t0) * 1e3)
  return {'median_ms': float(np.median(ts)), 'min_ms': float(np.min(ts)), 'max_ms': float(np.max(ts))}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=2048)
  ap.add_argument('--d', type=int, default=6)
  ap.add_argument('--m', type=int, default=8192)
  ap.add_argument('--q', type=int, default=3)
  ap.add_argument('--out', default=None)
  ap.add_argument('--time-limit', type=int, default=600)
  args = ap.parse_args()
  signal.alarm(args.time_limit)
  from dragonfly_amd.engine import FittedGP
  from dragonfly_amd.euclidean_gp import EuclideanGP
  from dragonfly_amd.gp_core import ConstantMean
  from dragonfly_amd.kernel import SEKernel
  rs = np.random.RandomState(0)
  X = rs.random_sample((args.n, args.d))
  Y = np.sin(3 * X.sum(axis=1)) + 0.05 * rs.standard_normal(args.n)
  gp = EuclideanGP(X, Y, SEKernel(args.d, float(Y.var()), np.full(args.d, 0.4)), ConstantMean(float(np.median(Y))),
                   float(Y.var()) / 20)
  Xs, Xh = rs.random_sample((args.m, args.d)), rs.random_sample((args.q, args.d))
  res = {'n': args.n, 'd': args.d, 'm': args.m, 'q': args.q, 'reps': REPS, 'warmup': WARM}

  def one_draw():
    np.random.seed(1)
    return gp.draw_samples_with_hallucinated_observations(1, Xs, Xh)

  fused = one_draw()
  res['fused'] = median_ms(one_draw)
  FittedGP.fused_draws = False          # the capability masked: the route of the code before the fused draw
  try:
    host = one_draw()
    res['host_route'] = median_ms(one_draw)
  finally:
    FittedGP.fused_draws = True
  res['host_over_fused'] = res['host_route']['median_ms'] / res['fused']['median_ms']
  res['routes_relerr'] = float(np.max(np.abs(fused - host)) / np.max(np.abs(host)))
  fit = gp.device_gp
  mean = gp.mean_func(Xs)
  for S in (1, 64):
    U = rs.standard_normal((args.m, S))
    res['draws_%d' % S] = median_ms(lambda: fit.draw(Xs, U, num_samples=S, X_halluc=Xh, mean_vals=mean))
  res['draws_64_over_1'] = res['draws_64']['median_ms'] / res['draws_1']['median_ms']
  line = json.dumps(res)
  print(line)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(line + '\n')


if __name__ == '__main__':
  main()
