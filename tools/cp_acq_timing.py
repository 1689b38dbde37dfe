"""Times one acquisition step on a Cartesian-product domain on the MI355X, fused route against the per-point route, and
writes profiles/cp_acq_timing.json.

    python tools/cp_acq_timing.py [out.json]

The per-point route is what runs without install(cp_acquisitions=True): the reference's maximiser calls the acquisition
on one point at a time (opt/gpb_acquisitions.py:35-37, exd/exd_utils.py:265), each call one posterior -- or one single-point
draw -- of the device GP.  It is reproduced here by that loop over the mirror GP's own eval / draw_samples, because the
reference is not needed for it: the candidates are given, and both routes get the same ones, the same fitted GP and
the same seed.  Drawing the candidates (the reference's sampler, identical on both routes) is not in either figure;
packing them is in the fused one.  The per-point route is timed three times: the spread of those repeats is the noise a
row is judged by.  Engine calls are counted on the fitted handle.
"""
import json
import os
import sys
import time

from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_EVALS = 2000
REPEATS = 3


class Part(object):
  def __init__(self, bounds):
    self.bounds = np.asarray(bounds, dtype=float)
    self.dim = len(self.bounds)

  def get_type(self):
    return 'euclidean'


class CPDomain(object):
  def __init__(self, parts=()):
    self.list_of_domains = list(parts)

  def get_type(self):
    return 'cartesian_product'

  def has_constraints(self):
    return False


def mirror_gp(kern, X, Y, noise):
  from dragonfly_amd.gp_core import GP

  class PackedCPGP(GP):
    _generic = False

    def _points_array(self, pts):
      return self.kernel.pack(pts)
  mean_c = float(np.mean(Y))
  return PackedCPGP(X, list(Y), kern, lambda x: np.array([mean_c] * len(x)), noise, handle_non_psd_kernels='project_first')


def mixed_points(rs, n):
  x, k, c = rs.random_sample((n, 2)), rs.randint(1, 8, (n, 1)), rs.randint(0, 3, (n, 2))
  pts = [[x[i].copy(), [int(k[i, 0])], ['abc'[c[i, 0]], 'uvw'[c[i, 1]]]] for i in range(n)]
  y = np.sin(3 * x[:, 0]) + x[:, 1] ** 2 - 0.05 * (k[:, 0] - 4) ** 2 + 0.3 * (c[:, 0] == c[:, 1])
  return pts, y


class Counter(object):
  """ counts the calls of a fitted handle's methods """
  NAMES = ('predict', 'predict_covar', 'acq_argmax', 'thompson', 'draw', 'thompson_pointwise')

  def __init__(self, handle):
    self.count = {}
    for name in self.NAMES:
      setattr(handle, name, self._wrap(name, getattr(handle, name)))

  def _wrap(self, name, fn):
    def call(*args, **kwargs):
      self.count[name] = self.count.get(name, 0) + 1
      return fn(*args, **kwargs)
    return call

  def take(self):
    out, self.count = dict(self.count), {}
    return out


def timed(fn, engine):
  engine.sync()
  t0 = time.perf_counter()
  out = fn()
  engine.sync()
  return out, (time.perf_counter() - t0) * 1e3


def anc_data(domain, method, max_evals):
  return Namespace(domain=domain, acq_opt_method=method, max_evals=max_evals, t=100, curr_max_val=None, is_mf=False,
                   handle_parallel='halluc', eval_points_in_progress=[])


def row(name, n, per_point, fused, engine, counter, same):
  """ per_point / fused: callables returning the chosen point; `same`: compares two of them """
  fused()                                                   # (first call: scratch buffers, code objects)
  counter.take()
  ref_pts, ref_ms = [], []
  for _ in range(REPEATS):
    pt, ms = timed(per_point, engine)
    ref_pts.append(pt)
    ref_ms.append(ms)
  ref_calls = counter.take()
  got_ms = []
  for _ in range(REPEATS):
    pt, ms = timed(fused, engine)
    got_ms.append(ms)
  calls = counter.take()
  out = dict(row=name, n=n, per_point_ms=[round(v, 3) for v in ref_ms], fused_ms=[round(v, 3) for v in got_ms],
             per_point_engine_calls={k: v // REPEATS for k, v in ref_calls.items()},
             fused_engine_calls={k: v // REPEATS for k, v in calls.items()},
             per_point_spread=round((max(ref_ms) - min(ref_ms)) / min(ref_ms), 4),
             speedup_median=round(float(np.median(ref_ms) / np.median(got_ms)), 2), same_point=bool(same(pt, ref_pts[0])))
  out['within_noise'] = bool(abs(np.median(ref_ms) - np.median(got_ms)) <= max(ref_ms) - min(ref_ms))
  print(json.dumps(out), flush=True)
  return out


def main():
  from dragonfly_amd import gpb_acquisitions as A, kernel as K
  from dragonfly_amd.doo import pdoo_maximise
  from dragonfly_amd.engine import get_engine
  engine = get_engine()
  rows = []
  for n in (70, 1000):
    rs = np.random.RandomState(100 + n)
    X, Y = mixed_points(rs, n)
    cands, _ = mixed_points(rs, MAX_EVALS)
    kern = K.CartesianProductKernel(1.7, [K.SEKernel(2, 1.0, [0.45, 0.8]), K.MaternKernel(1, 2.5, 1.0, [2.5]), K.HammingKernel([0.6, 0.4])])
    gp = mirror_gp(kern, X, Y + 0.05 * rs.standard_normal(n), 0.02)
    counter = Counter(gp.device_gp)
    A._cp_candidates = lambda anc, _c=cands: _c[:anc.max_evals]      # pylint: disable=protected-access
    anc = anc_data(CPDomain(), 'rand', MAX_EVALS)
    beta = A._get_ucb_beta_th(3.0, anc.t)                             # pylint: disable=protected-access

    def ucb_per_point():
      def acq(x):
        mu, sd = gp.eval([x], 'std')
        return mu + beta * sd
      return cands[int(np.argmax([acq(x) for x in cands]))]

    def ts_per_point():
      np.random.seed(5)
      return cands[int(np.argmax([gp.draw_samples(1, [x]).ravel() for x in cands]))]

    def ts_fused():
      np.random.seed(5)
      return A.asy.ts(gp, anc)
    rows.append(row('rand ucb, %d candidates' % MAX_EVALS, n, ucb_per_point, lambda: A.asy.ucb(gp, anc), engine, counter, lambda a, b: a is b))
    rows.append(row('rand ts, %d candidates' % MAX_EVALS, n, ts_per_point, ts_fused, engine, counter, lambda a, b: a is b))
    if n == 70:
      # the C-ABI alone: the point-wise draw against the block = 1 joint draw, 8000 candidates
      m = 8000
      P = kern.pack_many(mixed_points(rs, m)[0])
      U = rs.standard_normal(m)
      fit = gp.device_gp
      mean_c = float(np.mean(gp.Y))
      rows.append(row('dfh_gp_ts_pointwise against dfh_gp_draw(block=1), %d candidates' % m, n,
                      lambda: fit.draw(P, U, 1, block=1, mean_const=mean_c, return_samples=False)[2][0],
                      lambda: fit.thompson_pointwise(P, U, mean_const=mean_c)[1], engine, counter, lambda a, b: int(a) == int(b)))
    # the all-float product: two Euclidean parts, the tree search with 2000 evaluations
    P = np.hstack([rs.random_sample((n, 2)), -1 + 3 * rs.random_sample((n, 1))])
    Yf = -np.sum((P[:, :2] - 0.3) ** 2, axis=1) - 0.5 * (P[:, 2] - 0.7) ** 2
    kern_f = K.CartesianProductKernel(1.2, [K.SEKernel(2, 1.0, [0.5, 0.7]), K.MaternKernel(1, 2.5, 1.0, [1.1])])
    gp_f = mirror_gp(kern_f, [[r[:2].copy(), r[2:].copy()] for r in P], Yf, 0.01)
    counter_f = Counter(gp_f.device_gp)
    anc_f = anc_data(CPDomain([Part([[0, 1], [0, 1]]), Part([[-1, 2]])]), 'pdoo', MAX_EVALS)
    bounds = np.array([[0, 1], [0, 1], [-1, 2]], dtype=float)

    def tree_per_point():
      def acq(x):
        mu, sd = gp_f.eval([[x[:2], x[2:]]], 'std')
        return float(mu[0] + beta * sd[0])
      pt = pdoo_maximise(acq, bounds, MAX_EVALS)[1]
      return [pt[:2], pt[2:]]
    rows.append(row('tree search (pdoo) on an all-float product, %d evaluations' % MAX_EVALS, n, tree_per_point,
                    lambda: A.asy.ucb(gp_f, anc_f), engine, counter_f,
                    lambda a, b: all(np.array_equal(u, v) for u, v in zip(a, b))))
  out = dict(device=engine.name(), what='one acquisition step on a Cartesian-product domain: per-point route (today, flag off) '
             'against the fused route (install(cartesian_product=True, cp_acquisitions=True)); wall-clock ms of %d repeats each, '
             'engine calls per step' % REPEATS, rows=rows)
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'cp_acq_timing.json')
  os.makedirs(os.path.dirname(path), exist_ok=True)
  with open(path, 'w') as f:
    json.dump(out, f, indent=1)
  print('wrote', path)


if __name__ == '__main__':
  main()
