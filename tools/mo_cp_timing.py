"""Times one multi-objective acquisition step on a Cartesian-product domain on the MI355X, the fused route against the
per-point route, and writes profiles/mo_cp_acq_timing.json.

    python tools/mo_cp_timing.py [out.json]

The per-point route is what runs with install(multi_objective=True, cartesian_product=True) alone: the reference's
maximiser calls the closure on one point at a time (opt/gpb_acquisitions.py:35-37, exd/exd_utils.py:265), and the closure
makes one posterior -- or one single-point draw -- of the device GP per objective (opt/multiobjective_gpb_acquisitions.py:
32-39, 57-65, 80-89).  It is reproduced here by the mirror's own closure route over the same GPs (the route chooser told
that no fused call applies), because the reference is not needed for it: the candidates are given, and both routes get
the same ones, the same fitted GPs and the same seed.  The fused route is what the three flags install.  Drawing the
candidates (the reference's sampler, identical on both routes) is in neither figure; packing them is in the fused one.

The step: max_evals = 500 with the GA configured, the reference's default on mixed domains -- so a Thompson step takes
4 x 500 = 2000 random candidates (:24-26) -- and for UCB 500 candidates of 'rand'.  K = 2 and K = 3 objectives, n = 70
and n = 1000 training points.  Both routes are warmed up, then timed alternately REPEATS times, every window ending in a
device synchronise; a fused window holds INNER steps, so that it is not a fraction of a millisecond.  Medians, the
spread of the repeats and the ratio are recorded; engine calls are counted per step.
"""
import json
import os
import sys
import time

from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_EVALS = 500
REPEATS = 5
INNER = 10
SCALES, SE_BWS, NUS, MATERN_BWS = [1.7, 0.9, 2.4], [[0.45, 0.8], [0.3, 0.55], [0.9, 0.6]], [2.5, 1.5, 0.5], [[2.5], [1.6], [3.2]]
HAMMING_WS, NOISES = [[0.6, 0.4], [0.5, 0.5], [0.25, 0.75]], [0.02, 0.05, 0.01]
WEIGHTS, REFERENCE_POINT = [0.5, 0.3, 0.2], [-1.5, -2.0, -1.0]


class CPDomain(object):
  dim = 5
  list_of_domains = ()

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
  ys = [np.sin(3 * x[:, 0]) + x[:, 1] ** 2 - 0.05 * (k[:, 0] - 4) ** 2 + 0.3 * (c[:, 0] == c[:, 1]),
        np.cos(4 * x[:, 1]) - (x[:, 0] - 0.6) ** 2 + 0.1 * k[:, 0] - 0.2 * (c[:, 0] == 2),
        x[:, 0] * x[:, 1] - 0.03 * (k[:, 0] - 2) ** 2 + 0.25 * (c[:, 1] == 0) - 0.1 * (c[:, 0] == 1)]
  return pts, ys


class Counter(object):
  """ counts the calls of the engine's multi-objective methods and of the fitted handles' per-objective ones """

  def __init__(self, engine, handles):
    self.count = {}
    for obj, names in [(engine, ('mo_thompson_pointwise', 'mo_ucb_argmax'))] + \
                      [(h, ('predict', 'predict_covar', 'thompson', 'draw', 'thompson_pointwise')) for h in handles]:
      for name in names:
        setattr(obj, name, self._wrap(name, getattr(obj, name)))

  def _wrap(self, name, fn):
    if getattr(fn, 'counted', False):      # (the engine is shared by the runs)
      fn = fn.inner
    def call(*args, **kwargs):
      self.count[name] = self.count.get(name, 0) + 1
      return fn(*args, **kwargs)
    call.counted, call.inner = True, fn
    return call

  def take(self):
    out, self.count = dict(self.count), {}
    return out


def timed(fn, engine, inner=1):
  engine.sync()
  t0 = time.perf_counter()
  for _ in range(inner):
    out = fn()
  engine.sync()
  return out, (time.perf_counter() - t0) * 1e3 / inner


def row(name, n, k, m, per_point, fused, engine, counter):
  fused()
  counter.take()
  want = per_point()                                        # (warm-up of both: scratch buffers, code objects)
  per_point_calls = counter.take()
  got = fused()
  fused_calls = counter.take()
  ref_ms, got_ms = [], []
  for _ in range(REPEATS):                                  # alternately: whatever else the host does meets both
    ref_ms.append(timed(per_point, engine)[1])
    got_ms.append(timed(fused, engine, INNER)[1])
  spread = lambda ms: round((max(ms) - min(ms)) / float(np.median(ms)), 4)
  out = dict(row=name, n=n, objectives=k, candidates=m, per_point_ms=[round(v, 3) for v in ref_ms], fused_ms=[round(v, 4) for v in got_ms],
             per_point_median_ms=round(float(np.median(ref_ms)), 3), fused_median_ms=round(float(np.median(got_ms)), 4),
             per_point_spread=spread(ref_ms), fused_spread=spread(got_ms),
             ratio_of_medians=round(float(np.median(ref_ms) / np.median(got_ms)), 1),
             per_point_engine_calls=per_point_calls, fused_engine_calls=fused_calls, same_point=bool(got is want))
  print(json.dumps(out), flush=True)
  return out


def main():
  from dragonfly_amd import gpb_acquisitions as A, kernel as K, multiobjective_gpb_acquisitions as MO
  from dragonfly_amd.engine import get_engine
  engine = get_engine()
  device_gps = MO._device_gps                              # pylint: disable=protected-access
  rows = []
  for n in (70, 1000):
    rs = np.random.RandomState(100 + n)
    X, Ys = mixed_points(rs, n)
    cands, _ = mixed_points(rs, 4 * MAX_EVALS)
    A._cp_candidates = lambda anc, _c=cands: _c[:anc.max_evals]      # pylint: disable=protected-access
    all_gps = []
    for j in range(3):
      kern = K.CartesianProductKernel(SCALES[j], [K.SEKernel(2, 1.0, SE_BWS[j]), K.MaternKernel(1, NUS[j], 1.0, MATERN_BWS[j]),
                                                  K.HammingKernel(HAMMING_WS[j])])
      all_gps.append(mirror_gp(kern, X, Ys[j] + 0.05 * rs.standard_normal(n), NOISES[j]))
    counter = Counter(engine, [gp.device_gp for gp in all_gps])
    for k in (2, 3):
      gps = all_gps[:k]
      for acq, method, m in (('lin_ts', 'ga', 4 * MAX_EVALS), ('tch_ts', 'ga', 4 * MAX_EVALS), ('lin_ucb', 'rand', MAX_EVALS)):
        anc = Namespace(domain=CPDomain(), acq_opt_method=method, max_evals=MAX_EVALS, t=100, is_mf=False, handle_parallel='halluc',
                        eval_points_in_progress=[], obj_weights=WEIGHTS[:k], reference_point=REFERENCE_POINT[:k])
        assert MO.mo_cp_acquisition_applies(acq, gps, anc)
        step = getattr(MO.asy, acq)

        def fused(_step=step, _gps=gps, _anc=anc):
          np.random.seed(5)
          return _step(_gps, _anc)

        def per_point(_step=step, _gps=gps, _anc=anc, _acq=acq, _m=m):
          if _acq.endswith('_ucb'):
            # the reference's loop over its samples (exd_utils.py:265): the closure of :80-89 on one point per call
            beta = MO._get_ucb_beta_th(CPDomain.dim, _anc.t)     # pylint: disable=protected-access
            closure = MO._host_ucb_acquisition(_acq[:3], _gps, _anc, beta)      # pylint: disable=protected-access
            return cands[int(np.argmax([closure([x]) for x in cands[:_m]]))]
          MO._device_gps = lambda gps_, anc_: None           # pylint: disable=protected-access
          try:
            np.random.seed(5)
            return _step(_gps, _anc)                         # (a sampler: the closure route calls it point by point)
          finally:
            MO._device_gps = device_gps                      # pylint: disable=protected-access
        rows.append(row('%s, acq_opt_method=%s, max_evals=%d' % (acq, method, MAX_EVALS), n, k, m, per_point, fused, engine, counter))
  out = dict(device=engine.name(), what='one multi-objective acquisition step on a Cartesian-product domain (mixed: 2-D SE, integer '
             'Matern, two-column Hamming): the per-point route of install(multi_objective=True, cartesian_product=True) against the '
             'fused route of the three flags; wall-clock ms, %d alternating repeats (a fused window: %d steps), medians, engine calls '
             'per step' % (REPEATS, INNER), rows=rows)
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'mo_cp_acq_timing.json')
  os.makedirs(os.path.dirname(path), exist_ok=True)
  with open(path, 'w') as f:
    json.dump(out, f, indent=1)
  print('wrote', path)


if __name__ == '__main__':
  main()
