"""Writes tests/golden/moo_*.npz: the reference's four multi-objective acquisitions
(dragonfly/opt/multiobjective_gpb_acquisitions.py:19-107) under the 'rand' maximiser, for tests/test_moo_cpu.py and
tests/test_gpu_moo.py.  Runs the real reference on the CPU (oracle.make_golden.import_reference: its NumPy-2
shim); nothing under oracle/ is changed.

    python tools/make_moo_golden.py [/path/to/dragonfly-checkout]   (default: oracle.make_golden.REF)

Each fixture holds numbers only: the objectives' training data and hyper-parameters, weights, reference point,
time step, the generator state before the call, the candidates and normals the reference drew from it, the
per-candidate values of the reference's own closure, the chosen index and point, the generator state afterwards.
The kernels are rebuilt from the hyper-parameters by build_kernel() below, here and in the tests alike.

Per fixture the generator asserts that the reference's best and second-best value differ by more than 1e-8
relative -- so that "the same index" is a fair demand of values that agree to 1e-10 -- and re-seeds until it holds.
"""
import os
import sys

from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')

DIM = 3
M = 2000            # candidates, one joint block for Thompson sampling
MIN_GAP = 1e-8
# (name, scalarisation, acquisition, objectives' kernels, points in progress)
#   kernels: 'se' | 'm25' | 'm15' (Matern) | 'add' (additive: SE on columns [0, 2], Matern-2.5 on column [1])
CASES = [
  ('lin_ucb_k2', 'lin', 'ucb', ['se', 'm25'], 0),
  ('tch_ucb_k3', 'tch', 'ucb', ['m25', 'se', 'add'], 0),
  ('lin_ts_k3_q0', 'lin', 'ts', ['se', 'm15', 'add'], 0),
  ('tch_ts_k2_q0', 'tch', 'ts', ['m25', 'se'], 0),
  ('lin_ts_k2_q3', 'lin', 'ts', ['se', 'm25'], 3),
  ('tch_ts_k3_q3', 'tch', 'ts', ['se', 'add', 'm25'], 3),
]
ADD_GROUPS = [[0, 2], [1]]


def case_data(idx):
  """ Training inputs, labels and hyper-parameters of every objective of case idx (seeded, no reference needed) """
  _, _, _, kinds, q = CASES[idx]
  rng = np.random.RandomState(9100 + idx)
  n = 40 + 7 * idx
  X = rng.random_sample((n, DIM))
  objs = []
  for j, kind in enumerate(kinds):
    centre = rng.random_sample(DIM)
    Y = -np.sum((X - centre) ** 2, axis=1) + 0.3 * np.sin(5 * X[:, j % DIM]) + 0.02 * rng.randn(n)
    objs.append(dict(kind=kind, Y=Y, scale=float(np.exp(rng.uniform(-0.5, 0.5))), bw=np.exp(rng.uniform(np.log(0.25), np.log(1.0), DIM)),
                     noise=float(np.exp(rng.uniform(np.log(2e-3), np.log(2e-2)))), mean=float(np.median(Y))))
  weights = rng.uniform(0.3, 1.0, len(kinds))
  ref_point = np.array([float(np.min(o['Y'])) - 0.1 for o in objs])
  Xh = rng.random_sample((q, DIM))
  return X, objs, weights, ref_point, Xh, 5 + idx


def build_kernel(gk, obj):
  """ gk: the kernel module (the reference's or dragonfly_amd.kernel) """
  kind, scale, bw = obj['kind'], obj['scale'], obj['bw']
  if kind == 'se':
    return gk.SEKernel(DIM, scale, bw)
  if kind in ('m25', 'm15'):
    return gk.MaternKernel(DIM, 2.5 if kind == 'm25' else 1.5, scale, bw)
  return gk.AdditiveKernel(scale, [gk.SEKernel(2, 1.0, bw[ADD_GROUPS[0]]), gk.MaternKernel(1, 2.5, 1.0, bw[ADD_GROUPS[1]])],
                           ADD_GROUPS)


def const_mean(value):
  func = lambda x: np.array([value] * len(x))
  func.constant_value = value         # (how the mirror's fitters mark a constant mean)
  return func


def build_gps(gk, gp_cls, X, objs):
  return [gp_cls(list(X), list(o['Y']), build_kernel(gk, o), const_mean(o['mean']), o['noise']) for o in objs]


def anc_data_for(domain, scal, weights, ref_point, Xh, t, method='rand', max_evals=M):
  return Namespace(domain=domain, acq_opt_method=method, max_evals=max_evals, obj_weights=list(weights),
                   reference_point=list(ref_point), t=t, handle_parallel='halluc', is_mf=False,
                   eval_points_in_progress=[row for row in Xh], curr_max_val=None)


def pack_state(state):
  """ np.random.get_state() as numbers: (key[624], [pos, has_gauss], cached gaussian) """
  return np.asarray(state[1], dtype=np.uint32), np.array([state[2], state[3]], dtype=np.int64), float(state[4])


def unpack_state(key, pos_has, gauss):
  return ('MT19937', np.asarray(key, dtype=np.uint32), int(pos_has[0]), int(pos_has[1]), float(gauss))


def main(argv):
  from oracle import make_golden
  if len(argv) > 1:
    make_golden.REF = argv[1]
  make_golden.import_reference()
  from dragonfly.gp import kernel as gk
  from dragonfly.gp.euclidean_gp import EuclideanGP
  from dragonfly.exd.domains import EuclideanDomain
  from dragonfly.opt import multiobjective_gpb_acquisitions as ref_moo
  from dragonfly.exd import exd_utils
  os.makedirs(OUT, exist_ok=True)
  for idx, (name, scal, acq, kinds, q) in enumerate(CASES):
    X, objs, weights, ref_point, Xh, t = case_data(idx)
    gps = build_gps(gk, EuclideanGP, X, objs)
    domain = EuclideanDomain([[0, 1]] * DIM)
    seed = 3000 + 17 * idx
    while True:
      # the maximiser's own random_maximise, recorded: candidates and per-candidate values of the reference's closure
      seen = {}
      orig = exd_utils.random_maximise         # (the name maximise_with_method_on_euclidean_domain calls it by)
      def recording(obj, *args, **kwargs):
        def recorded_obj(x):
          vals = obj(x)
          seen['cands'], seen['vals'] = np.array(x), np.array(vals, dtype=float).ravel()
          return vals
        return orig(recorded_obj, *args, **kwargs)
      exd_utils.random_maximise = recording
      np.random.seed(seed)
      before = np.random.get_state()
      try:
        point = getattr(ref_moo.asy, '%s_%s' % (scal, acq))(gps, anc_data_for(domain, scal, weights, ref_point, Xh, t))
      finally:
        exd_utils.random_maximise = orig
      after = np.random.get_state()
      vals = seen['vals']
      assert not np.isnan(vals).any()
      top = np.sort(vals)[::-1]
      gap = (top[0] - top[1]) / abs(top[0])
      if gap > MIN_GAP:
        break
      seed += 1
    best = int(np.argmax(vals))
    cands = seen['cands']
    assert cands.shape == (M, DIM) and np.array_equal(np.asarray(point), cands[best])
    # the candidates and normals once more from the recorded state, as plain draws: what the fixture stores
    np.random.set_state(before)
    redraw = np.random.random((M, DIM))       # (unit-cube bounds: map_to_bounds is the identity up to * 1 + 0)
    assert np.array_equal(redraw * 1.0 + 0.0, cands)
    normals = np.array([np.random.normal(size=(M, 1)).ravel() for _ in kinds]) if acq == 'ts' else np.zeros((0, M))
    k0, p0, g0 = pack_state(before)
    k1, p1, g1 = pack_state(after)
    s1 = np.random.get_state()
    assert np.array_equal(s1[1], after[1]) and s1[2:] == after[2:]
    np.savez_compressed(
        os.path.join(OUT, 'moo_%s.npz' % name), X=X, Y=np.array([o['Y'] for o in objs]), scale=np.array([o['scale'] for o in objs]),
        bw=np.array([o['bw'] for o in objs]), noise=np.array([o['noise'] for o in objs]), mean=np.array([o['mean'] for o in objs]),
        weights=weights, ref_point=ref_point, t=t, Xh=Xh, seed=seed, state_key=k0, state_pos=p0, state_gauss=g0,
        after_key=k1, after_pos=p1, after_gauss=g1, cands=cands, normals=normals, vals=vals, best_idx=best, point=np.asarray(point),
        gap=gap)
    print('moo_%s: seed %d, best %d, gap %.2e' % (name, seed, best, gap))
  print('wrote the moo_*.npz fixtures to', OUT)


if __name__ == '__main__':
  sys.path.insert(0, ROOT)
  main(sys.argv)
