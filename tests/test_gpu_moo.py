"""MI355X: the fused multi-objective acquisitions (dfh_mo_ucb_argmax / dfh_mo_ts_argmax) through the C-ABI, against
the REAL reference's outputs (tests/golden/moo_*.npz, tools/make_moo_golden.py) and against the single-objective
entry points.  One tolerance, the project's: 1e-10 norm-wise, or max(1e-10, 2 err(reference, long-double truth))
per case where the reference's own joint draw is further than that from the truth (tests/truth_bounds.py)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, relerr
from oracle import ref_numpy as O

import truth_bounds as tb
from oracle_engine_moo import scalarise_ts, scalarise_ucb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def _gen():
  spec = importlib.util.spec_from_file_location('make_moo_golden', os.path.join(ROOT, 'tools', 'make_moo_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


G = _gen()
MATERN_NU = {'m25': 2.5, 'm15': 1.5}


def _device_gps(idx):
  """ the objectives of fixture idx as mirror GPs fitted on the device, and everything else of the case """
  from dragonfly_amd import kernel as K
  from dragonfly_amd.gp_core import GP
  X, objs, weights, ref_point, Xh, t = G.case_data(idx)
  gps = G.build_gps(K, GP, X, objs)
  return gps, [gp.device_gp for gp in gps], X, objs, weights, ref_point, Xh, t


def _beta(t):
  return np.sqrt(0.2 * G.DIM * np.log(2 * G.DIM * t + 1))


def _oracle(X, obj):
  if obj['kind'] == 'add':
    subs = [O.KernelSpec('se', 2, 1.0, obj['bw'][G.ADD_GROUPS[0]]), O.KernelSpec('matern', 1, 1.0, obj['bw'][G.ADD_GROUPS[1]], nu=2.5)]
    spec = O.KernelSpec('additive', G.DIM, obj['scale'], groups=G.ADD_GROUPS, subs=subs)
  elif obj['kind'] == 'se':
    spec = O.KernelSpec('se', G.DIM, obj['scale'], obj['bw'])
  else:
    spec = O.KernelSpec('matern', G.DIM, obj['scale'], obj['bw'], nu=MATERN_NU[obj['kind']])
  return O.GPOracle(X, obj['Y'], spec, obj['mean'], obj['noise'])


def _truth_draw(X, obj, Xs, Xh, U):
  """ (objective's joint draw in extended precision, the reference arithmetic's jitter power).  Single SE / Matern
      kernels: from the kernel itself (the covariance of 2000 candidates behind some 50 points is numerically singular,
      so the draw is sensitive to the rounding of the covariance; tests/truth_bounds.py: kernel_draw_bound) -- with
      points in progress, the factor of the GP over (X, Xh) with zero labels and the mean of the real one.  The
      additive objective has no such truth: the extended-precision draw from the oracle's own mean and covariance. """
  from oracle import ref_longdouble as T
  og = _oracle(X, obj)
  if len(Xh):
    mu, cov = og.eval_with_hallucinated_observations(Xs, Xh, 'covar')
  else:
    mu, cov = og.eval(Xs, 'covar')
  _, pw = O.stable_cholesky(cov, return_power=True)
  jit = 0.0 if pw is None else (10.0 ** pw) * float(np.diag(cov).max())
  if obj['kind'] == 'add':
    return T.gaussian_draw(mu, cov, U, jit), pw
  kind, nu = ('se', 0.0) if obj['kind'] == 'se' else ('matern', MATERN_NU[obj['kind']])
  if not len(Xh):
    return T.gp_truth(kind, obj['bw'], obj['scale'], X, obj['Y'] - obj['mean'], obj['noise'], Xs, obj['mean'], 0.0, nu=nu,
                      ts_normals=U, ts_jitter=jit)['draw'], pw
  Xa = np.concatenate([X, Xh], axis=0)
  spread = T.gp_truth(kind, obj['bw'], obj['scale'], Xa, np.zeros(len(Xa)), obj['noise'], Xs, 0.0, 0.0, nu=nu, ts_normals=U,
                      ts_jitter=jit)['draw']
  mean = T.gp_truth(kind, obj['bw'], obj['scale'], X, obj['Y'] - obj['mean'], obj['noise'], Xs, obj['mean'], 0.0, nu=nu)['mu']
  return mean + spread, pw


@pytest.mark.parametrize('idx', range(len(G.CASES)))
def test_fixtures_of_the_reference(engine, idx):
  name, scal, acq, kinds, q = G.CASES[idx]
  gold = load_golden('moo_' + name)
  gps, fitted, X, objs, weights, ref_point, Xh, t = _device_gps(idx)
  Xs, means = gold['cands'], [o['mean'] for o in objs]
  refs = ref_point if scal == 'tch' else None
  if acq == 'ucb':
    bv, bi, vals = engine.mo_ucb_argmax(fitted, scal, _beta(t), weights, refs, Xs, mean_consts=means, return_vals=True)
    bound = TOL
  else:
    bv, bi, vals, powers = engine.mo_thompson(fitted, scal, weights, refs, Xs, gold['normals'], block=len(Xs), X_halluc=Xh,
                                              mean_consts=means, return_vals=True)
    truths = [_truth_draw(X, o, Xs, Xh, gold['normals'][i]) for i, o in enumerate(objs)]
    bound = tb.bound(gold['vals'], scalarise_ts(scal, weights, ref_point, [d for d, _ in truths]))
    print(name, 'jitter powers', powers, 'reference arithmetic', [pw for _, pw in truths])
    assert powers == [[pw] for _, pw in truths]
  err = relerr(vals, gold['vals'])
  print(name, 'relerr', err, 'bound', bound, 'index', bi, 'reference', int(gold['best_idx']), 'gap', float(gold['gap']))
  assert err <= bound, (name, err, bound)
  assert bi == int(gold['best_idx']) and bv == vals[bi]
  assert np.array_equal(Xs[bi], gold['point'])


@pytest.mark.parametrize('idx', [0, 1])
def test_fused_ucb_equals_the_single_objective_calls(engine, idx):
  _, scal, _, _, _ = G.CASES[idx]
  gps, fitted, X, objs, weights, ref_point, _, t = _device_gps(idx)
  Xs = np.random.RandomState(50 + idx).random_sample((1500, G.DIM))
  mus, sds = [], []
  for f, o in zip(fitted, objs):
    mu, sd = f.predict(Xs)
    mus.append(o['mean'] + mu)
    sds.append(sd)
  want = scalarise_ucb(scal, _beta(t), weights, ref_point, mus, sds)
  bv, bi, vals = engine.mo_ucb_argmax(fitted, scal, _beta(t), weights, ref_point, Xs, mean_consts=[o['mean'] for o in objs],
                                      return_vals=True)
  print('ucb', scal, 'relerr', relerr(vals, want), 'bit-identical', np.array_equal(vals, want))
  assert np.array_equal(vals, want)             # the same kernels, then IEEE multiply / add / sqrt / divide
  assert bi == int(np.argmax(want)) and bv == want[bi]
  # prior means as values per candidate instead of constants
  mv = np.array([np.full(len(Xs), o['mean']) for o in objs])
  assert np.array_equal(engine.mo_ucb_argmax(fitted, scal, _beta(t), weights, ref_point, Xs, mean_vals=mv, return_vals=True)[2], want)


@pytest.mark.parametrize('idx', [2, 3])
def test_fused_thompson_equals_the_single_objective_calls(engine, idx):
  _, scal, _, _, _ = G.CASES[idx]
  gps, fitted, X, objs, weights, ref_point, _, _ = _device_gps(idx)
  rs = np.random.RandomState(60 + idx)
  m, block = 1300, 256
  Xs, U = rs.random_sample((m, G.DIM)), rs.standard_normal((len(objs), m))
  draws, powers = [], []
  for i, (f, o) in enumerate(zip(fitted, objs)):
    _, _, samples, jps = f.thompson(Xs, U[i], block=block, mean_const=o['mean'], return_samples=True)
    draws.append(samples)
    powers.append(jps)
  want = scalarise_ts(scal, weights, ref_point, draws)
  bv, bi, vals, got_powers = engine.mo_thompson(fitted, scal, weights, ref_point, Xs, U, block=block,
                                                mean_consts=[o['mean'] for o in objs], return_vals=True)
  print('ts', scal, 'relerr', relerr(vals, want), 'bit-identical', np.array_equal(vals, want))
  assert np.array_equal(vals, want) and got_powers == powers
  assert bi == int(np.argmax(want)) and bv == want[bi]


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_moo as M
from dragonfly_amd.engine import get_engine
np.savez(%(out)r, **M.chunk_case(get_engine()))
'''


def chunk_case(engine):
  """ both fused calls on more candidates than one small chunk holds (run in this process and in a child) """
  out = {}
  for idx, key in ((1, 'ucb'), (5, 'ts')):
    _, scal, _, _, _ = G.CASES[idx]
    gps, fitted, X, objs, weights, ref_point, Xh, t = _device_gps(idx)
    rs = np.random.RandomState(70 + idx)
    m = 2300
    Xs, U = rs.random_sample((m, G.DIM)), rs.standard_normal((len(objs), m))
    means = [o['mean'] for o in objs]
    if key == 'ucb':
      bv, bi, vals = engine.mo_ucb_argmax(fitted, scal, _beta(t), weights, ref_point, Xs, mean_consts=means, return_vals=True)
    else:
      bv, bi, vals, _ = engine.mo_thompson(fitted, scal, weights, ref_point, Xs, U, block=32, X_halluc=Xh, mean_consts=means,
                                           return_vals=True)
    out[key + '_vals'], out[key + '_best'] = vals, np.array([bv, bi])
  return out


def test_results_do_not_depend_on_the_chunk(engine, tmp_path):
  """ DFH_CHUNK_GIB is read once per process: the small-chunk run is a child (512-row chunks, five of them) """
  here = chunk_case(engine)
  out = str(tmp_path / 'child.npz')
  env = dict(os.environ, DFH_CHUNK_GIB='0.0001')
  res = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), out=out)], env=env,
                       capture_output=True, text=True, timeout=600)
  assert res.returncode == 0, res.stderr[-2000:]
  child = np.load(out)
  for key in ('ucb', 'ts'):
    err = relerr(child[key + '_vals'], here[key + '_vals'])
    print(key, 'small chunks vs one chunk: relerr', err, 'bit-identical', np.array_equal(child[key + '_vals'], here[key + '_vals']))
    assert err <= TOL and np.array_equal(child[key + '_best'], here[key + '_best'])


@pytest.mark.parametrize('idx', [2, 5])
def test_thompson_is_block_aligned_shard_invariant(engine, idx):
  """ blocks are independent: the fused call on block-aligned slices of the candidates gives the whole call's values,
      with points in progress (idx 5) and without """
  _, scal, _, _, q = G.CASES[idx]
  gps, fitted, X, objs, weights, ref_point, Xh, _ = _device_gps(idx)
  rs = np.random.RandomState(80 + idx)
  m, block = 5 * 200 + 70, 200
  Xs, U = rs.random_sample((m, G.DIM)), rs.standard_normal((len(objs), m))
  means = [o['mean'] for o in objs]
  bv, bi, vals, powers = engine.mo_thompson(fitted, scal, weights, ref_point, Xs, U, block=block, X_halluc=Xh, mean_consts=means,
                                            return_vals=True)
  assert len(powers) == len(objs) and len(powers[0]) == 6 and np.all(np.isfinite(vals))
  got = np.empty(m)
  for lo in (0, 2 * block, 3 * block):
    hi = {0: 2 * block, 2 * block: 3 * block, 3 * block: m}[lo]
    got[lo:hi] = engine.mo_thompson(fitted, scal, weights, ref_point, Xs[lo:hi], U[:, lo:hi], block=block, X_halluc=Xh,
                                    mean_consts=means, return_vals=True)[2]
  assert np.array_equal(got, vals)
  assert bi == int(np.argmax(vals)) and bv == vals[bi]
  if q:     # the points in progress matter: without them the draw is another one
    assert relerr(engine.mo_thompson(fitted, scal, weights, ref_point, Xs, U, block=block, mean_consts=means, return_vals=True)[2],
                  vals) > 1e-6


def test_a_nan_sigma_wins_the_argmax(engine):
  """ unclipped negative variance (gp_core.py:187): candidates equal to training points of a noise-free, heavily
      correlated fit give var = k(x,x) - ||V||^2 slightly below zero -> NaN; both UCB scalarisations carry it and
      np.argmax returns the first NaN. """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(9)
  d = 2
  X = rs.rand(60, d)
  y = rs.randn(60)
  Xs = np.vstack((rs.rand(50, d), X, rs.rand(50, d)))
  good = engine.gp_fit(KernelSpec('matern', d, 1.0, np.full(d, 0.5), nu=2.5), X, y, 1e-2)
  bad, nan_at = None, []
  for bw, noise in ((2.0, 1e-13), (3.0, 1e-12), (4.0, 1e-11), (2.0, 1e-10)):     # (the first that rounds below zero somewhere)
    bad = engine.gp_fit(KernelSpec('se', d, 1.0, np.full(d, bw)), X, y, noise)
    nan_at = np.flatnonzero(np.isnan(bad.predict(Xs)[1]))
    if len(nan_at):
      break
  if not len(nan_at):
    # that construction rounds below zero on some devices and not on others (test_gpu_oracle_parity.py treats it as
    # optional too).  One that cannot miss: a product kernel whose Hamming factor has weights summing below zero
    # (fitted with 'project_first', as tests/test_gpu_cp.py does) has the prior variance k(x, x) = 1.3 * (0.6 - 0.9) < 0,
    # so k(x, x) - ||V||^2 is negative for every candidate
    P = lambda A: np.hstack([A, np.floor(3 * A)])
    spec = KernelSpec('product', 4, 1.3, groups=[[0, 1], [2, 3]], sub_kinds=['se', 'hamming'], sub_scales=[1.0, 1.0],
                      sub_nus=[0.0, 0.0], sub_bandwidths=[[0.7, 0.9], [0.6, -0.9]])
    X, Xs = P(X), P(Xs)
    good = engine.gp_fit(KernelSpec('matern', 4, 1.0, np.full(4, 0.5), nu=2.5), X, y, 1e-2)
    bad = engine.gp_fit(spec, X, y, 1e-3, handle_non_psd_kernels='project_first')
    nan_at = np.flatnonzero(np.isnan(bad.predict(Xs)[1]))
  print('NaN standard deviations:', len(nan_at), 'first at', nan_at[:1])
  assert len(nan_at) > 0                       # the construction gives what it is for
  for scal in ('lin', 'tch'):
    bv, bi, vals = engine.mo_ucb_argmax([good, bad], scal, 1.3, [0.6, 0.4], [-2.0, -2.0], Xs, mean_consts=[0.0, 0.0], return_vals=True)
    assert np.array_equal(np.flatnonzero(np.isnan(vals)), nan_at), scal
    assert bi == nan_at[0] and np.isnan(bv), scal


def test_bad_arguments(engine):
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(4)
  X, X4, y = rs.random_sample((30, 3)), rs.random_sample((30, 4)), rs.standard_normal(30)
  gp = engine.gp_fit(KernelSpec('se', 3, 1.0, np.full(3, 0.5)), X, y, 0.01)
  gp4 = engine.gp_fit(KernelSpec('se', 4, 1.0, np.full(4, 0.5)), X4, y, 0.01)
  Xs, U = rs.random_sample((10, 3)), rs.standard_normal((9, 10))
  ucb = lambda gps, scal, w, r: engine.mo_ucb_argmax(gps, scal, 1.0, w, r, Xs, mean_consts=np.zeros(len(gps)))
  ts = lambda gps, scal, w, r: engine.mo_thompson(gps, scal, w, r, Xs, U[:len(gps)], block=10, mean_consts=np.zeros(len(gps)))
  for call in (ucb, ts):
    call([gp, gp], 'tch', [0.5, 0.5], [0.0, 0.0])                       # fine
    with pytest.raises(ValueError):
      call([], 'lin', [], None)                                         # k < 1
    with pytest.raises(ValueError):
      call([gp] * 9, 'lin', [0.1] * 9, None)                            # k > 8
    with pytest.raises(ValueError):
      call([gp, gp], 'tch', [0.5, 0.0], [0.0, 0.0])                     # a zero weight under Tchebychev
    with pytest.raises(ValueError):
      call([gp, gp], 'tch', [0.5, 0.5], None)                           # no reference point under Tchebychev
    with pytest.raises(ValueError):
      call([gp, gp4], 'lin', [0.5, 0.5], None)                          # input dimensions differ
    call([gp, gp], 'lin', [0.5, 0.0], None)                             # a zero weight is fine for the linear one
  from dragonfly_amd.engine import Engine
  other = Engine()
  try:
    foreign = other.gp_fit(KernelSpec('se', 3, 1.0, np.full(3, 0.5)), X, y, 0.01)
    with pytest.raises(ValueError):
      ucb([gp, foreign], 'lin', [0.5, 0.5], None)                       # handles of two contexts
    foreign.free()
  finally:
    other.close()


@pytest.mark.parametrize('idx', [1, 5])
def test_candidates_and_normals_as_device_buffers(engine, idx):
  _, scal, acq, _, _ = G.CASES[idx]
  gps, fitted, X, objs, weights, ref_point, Xh, t = _device_gps(idx)
  rs = np.random.RandomState(90 + idx)
  m = 900
  Xs, U = rs.random_sample((m, G.DIM)), rs.standard_normal((len(objs), m))
  means = [o['mean'] for o in objs]
  dXs, dU = engine.to_device(Xs), engine.to_device(U)
  if acq == 'ucb':
    want = engine.mo_ucb_argmax(fitted, scal, _beta(t), weights, ref_point, Xs, mean_consts=means, return_vals=True)
    got = engine.mo_ucb_argmax(fitted, scal, _beta(t), weights, ref_point, dXs, mean_consts=means, return_vals=True)
  else:
    want = engine.mo_thompson(fitted, scal, weights, ref_point, Xs, U, block=m, X_halluc=Xh, mean_consts=means, return_vals=True)
    got = engine.mo_thompson(fitted, scal, weights, ref_point, dXs, dU, block=m, X_halluc=Xh, mean_consts=means, return_vals=True)
  assert got[0] == want[0] and got[1] == want[1] and np.array_equal(got[2], want[2])
  assert np.array_equal(dXs.row(got[1]), Xs[want[1]])
