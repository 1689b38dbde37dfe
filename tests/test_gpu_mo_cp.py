"""MI355X: the fused multi-objective acquisitions on Cartesian-product domains -- dfh_mo_ts_pointwise (per candidate and
objective the one-point draw the reference makes on these domains, scalarised, and the arg-max) and dfh_mo_ucb_argmax on
packed mixed candidates -- against what the REAL reference's own closures compute one point per call
(tests/golden/mo_cp_acq_n70.npz, tools/record_mo_cp_acq_golden.py), and the fused host route of
dragonfly_amd.multiobjective_gpb_acquisitions against the per-point closure route on the same fitted GPs.

K = 3 GPs on 70 points (one past the 64-row tile) of a 2-D SE part, an integer Matern column (nu 2.5 / 1.5 / 0.5) and a
Hamming part of two columns, fitted with 'project_first'; 257 candidates (one past a 256-thread workgroup), one of them a
training row; the m K normals POINT-major.  One tolerance against the reference, the project's: 1e-10 norm-wise.  Every
arg-max in the fixture is decided by more than 1e-8 of the largest value (checked when it was recorded), so winners are
compared for equality.  What cannot drift is checked bit for bit."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-10
M, K = 257, 3
CHUNK = 262144                 # pick_chunk's rows per posterior chunk at n = 70 (and n = 72 with two points in progress)


@pytest.fixture(scope='module')
def gold():
  return load_golden('mo_cp_acq_n70')


def _spec(g, j):
  from dragonfly_amd.engine import KernelSpec
  return KernelSpec('product', 5, float(g['scales'][j]), groups=[[0, 1], [2], [3, 4]], sub_kinds=['se', 'matern', 'hamming'],
                    sub_scales=[1.0, 1.0, 1.0], sub_nus=[0.0, float(g['matern_nus'][j]), 0.0],
                    sub_bandwidths=[g['se_bws'][j], g['matern_bws'][j], g['hamming_ws'][j]])


@pytest.fixture(scope='module')
def fits(engine, gold):
  g = gold
  assert g['Xp'].shape == (70, 5) and g['Cp'].shape == (M, 5) and g['U'].shape == (M, K)
  assert np.array_equal(g['Cp'][int(g['dup_cand'])], g['Xp'][int(g['dup_train'])])
  return [engine.gp_fit(_spec(g, j), g['Xp'], g['Y'][j] - float(g['mean_consts'][j]), float(g['noises'][j]),
                        handle_non_psd_kernels='project_first') for j in range(K)]


def _halluc(g, q):
  return g['Hp'] if q else None


def _np_scalarise(scal, samples, w, refs):
  """ the reference's loops (opt/multiobjective_gpb_acquisitions.py:36-39, :61-65) on the rows of `samples` """
  if scal == 'lin':
    s = 0.0
    for sample, weight in zip(samples, w):
      s = s + sample * weight
    return s
  s = np.full((samples.shape[1],), np.inf)
  for sample, weight, ref in zip(samples, w, refs):
    s = np.minimum(s, (sample - ref) / weight)
  return s


def _call(engine, fits, g, scal, q=0, **kwargs):
  args = dict(normals=g['U'], X_halluc=_halluc(g, q), mean_consts=g['mean_consts'], return_vals=True, return_samples=True)
  args.update(kwargs)
  k = len(fits)
  return engine.mo_thompson_pointwise(fits, scal, g['weights'][:k], g['reference_point'][:k], g['Cp'], **args)


# ---- 1. the reference's values --------------------------------------------------------------------------------------
@pytest.mark.parametrize('scal', ['lin', 'tch'])
@pytest.mark.parametrize('q', [0, 2])
def test_mo_ts_pointwise_returns_the_reference_values(engine, fits, gold, q, scal):
  g = gold
  bv, bi, vals, samples = _call(engine, fits, g, scal, q)
  want = g['%s_ts_q%d' % (scal, q)]
  err, err_s = relerr(vals, want), max(relerr(samples[j], g['draws_q%d' % q][j]) for j in range(K))
  print('mo_ts_pointwise %s q=%d relerr values %.3e draws %.3e winner %d (reference %d, its top-two gap %.2e)'
        % (scal, q, err, err_s, bi, int(g['%s_ts_win_q%d' % (scal, q)]), float(g['%s_ts_gap_q%d' % (scal, q)])))
  assert err <= TOL
  assert err_s <= TOL
  assert bi == int(g['%s_ts_win_q%d' % (scal, q)]) and bv == vals[bi]


# ---- 2. bit-identities ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scal', ['lin', 'tch'])
@pytest.mark.parametrize('q', [0, 2])
def test_mo_ts_pointwise_is_the_single_objective_draws_scalarised(engine, fits, gold, q, scal):
  g = gold
  bv, bi, vals, samples = _call(engine, fits, g, scal, q)
  for j in range(K):
    one = fits[j].thompson_pointwise(g['Cp'], np.ascontiguousarray(g['U'][:, j]), X_halluc=_halluc(g, q),
                                     mean_const=float(g['mean_consts'][j]), return_samples=True)[2]
    assert np.array_equal(samples[j], one), j
  assert np.array_equal(vals, _np_scalarise(scal, samples, g['weights'], g['reference_point']))
  assert bi == int(np.argmax(vals)) and bv == vals[bi]


@pytest.mark.parametrize('q', [0, 2])
def test_one_objective_with_weight_one_is_dfh_gp_ts_pointwise(engine, fits, gold, q):
  g = gold
  u = np.ascontiguousarray(g['U'][:, 1])
  want = fits[1].thompson_pointwise(g['Cp'], u, X_halluc=_halluc(g, q), mean_const=float(g['mean_consts'][1]), return_samples=True)
  bv, bi, vals, samples = engine.mo_thompson_pointwise([fits[1]], 'lin', [1.0], None, g['Cp'], u, X_halluc=_halluc(g, q),
                                                       mean_consts=[g['mean_consts'][1]], return_vals=True, return_samples=True)
  assert (bv, bi) == want[:2]
  assert np.array_equal(vals, want[2]) and np.array_equal(samples[0], want[2])


# ---- 3. mo_ucb_argmax on packed mixed candidates --------------------------------------------------------------------
@pytest.mark.parametrize('scal', ['lin', 'tch'])
def test_mo_ucb_argmax_on_packed_mixed_candidates(engine, fits, gold, scal):
  g = gold
  call = lambda rows: engine.mo_ucb_argmax(fits, scal, float(g['beta']), g['weights'], g['reference_point'], rows,
                                           mean_consts=g['mean_consts'], return_vals=True)
  bv, bi, vals = call(g['Cp'])
  want, win = g['%s_ucb_q0' % scal], int(g['%s_ucb_win_q0' % scal])
  err = relerr(vals, want)
  print('mo_ucb_argmax %s relerr %.3e winner %d (reference %d, gap %.2e)' % (scal, err, bi, win, float(g['%s_ucb_gap_q0' % scal])))
  assert err <= TOL
  assert bi == win == int(np.argmax(vals)) and bv == vals[bi]
  # one row alone, as Dragonfly's own maximisers (the GA) ask for it: the value it has in the batch, bit for bit
  for i in (0, win, int(g['dup_cand']), M - 1):
    alone = call(g['Cp'][i:i + 1])
    print('row %d alone %.17g in the batch %.17g' % (i, alone[2][0], vals[i]))
    assert alone[1] == 0 and alone[2][0] == vals[i] and alone[0] == vals[i], i


# ---- 4. argument and pointer edges ----------------------------------------------------------------------------------
def test_pointer_kinds_and_null_outputs(engine, fits, gold):
  g = gold
  bv, bi, vals, samples = _call(engine, fits, g, 'tch', 2)
  mv = np.array([np.full(M, c) for c in g['mean_consts']])
  dX, dU, dmv = engine.to_device(g['Cp']), engine.to_device(g['U']), engine.to_device(mv)
  for Xs, U, means in ((dX, dU, dict(mean_vals=dmv)), (dX, g['U'], dict(mean_vals=mv)), (g['Cp'], dU, dict(mean_consts=g['mean_consts']))):
    got = engine.mo_thompson_pointwise(fits, 'tch', g['weights'], g['reference_point'], Xs, U, X_halluc=g['Hp'], return_vals=True,
                                       return_samples=True, **means)
    assert got[:2] == (bv, bi) and np.array_equal(got[2], vals) and np.array_equal(got[3], samples)
    assert engine.mo_thompson_pointwise(fits, 'tch', g['weights'], g['reference_point'], Xs, U, X_halluc=g['Hp'], **means) == (bv, bi)
  # the raw entry point with samples_out and vals_out NULL, then with no optional output at all
  handles = (C.c_void_p * K)(*[f.handle for f in fits])
  w, r, mc = [np.ascontiguousarray(g[key], dtype=np.float64) for key in ('weights', 'reference_point', 'mean_consts')]
  rbv, rbi = C.c_double(0), C.c_int64(-1)
  rc = engine.lib.dfh_mo_ts_pointwise(handles, K, 1, w.ctypes.data, r.ctypes.data, g['Cp'].ctypes.data, M, g['Hp'].ctypes.data, 2,
                                      g['U'].ctypes.data, mc.ctypes.data, None, None, None, C.byref(rbv), C.byref(rbi))
  assert rc == 0 and (rbv.value, rbi.value) == (bv, bi)
  rc = engine.lib.dfh_mo_ts_pointwise(handles, K, 1, w.ctypes.data, r.ctypes.data, g['Cp'].ctypes.data, M, g['Hp'].ctypes.data, 2,
                                      g['U'].ctypes.data, mc.ctypes.data, None, None, None, None, None)
  assert rc == 0


def test_draws_its_own_normals_from_the_global_stream(engine, fits, gold):
  """ normals=None: Engine.random_normals(m K) -- the stream of m K calls of np.random.normal(size=(1, 1)), the cached
      second Gaussian included (m K is odd), and the state those calls leave """
  g = gold
  np.random.seed(991)
  U = np.array([np.random.normal(size=(1, 1))[0, 0] for _ in range(M * K)])
  state = np.random.get_state()
  want = _call(engine, fits, g, 'lin', normals=U)
  np.random.seed(991)
  got = _call(engine, fits, g, 'lin', normals=None)
  after = np.random.get_state()
  assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
  assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]
  with pytest.raises(ValueError):
    _call(engine, fits, g, 'lin', normals=U[:-1])              # a wrong number of normals


@pytest.mark.parametrize('scal', ['lin', 'tch'])
def test_one_candidate_and_eight_objectives(engine, fits, gold, scal):
  g = gold
  full = _call(engine, fits, g, scal)
  for i in (0, M - 1):                                         # m = 1
    bv, bi, vals, samples = engine.mo_thompson_pointwise(fits, scal, g['weights'], g['reference_point'], g['Cp'][i:i + 1], g['U'][i:i + 1],
                                                         mean_consts=g['mean_consts'], return_vals=True, return_samples=True)
    assert bi == 0 and bv == vals[0] and vals.shape == (1,) and samples.shape == (K, 1)
    assert relerr(samples[:, 0], full[3][:, i]) <= TOL and relerr(vals, full[2][i:i + 1]) <= TOL
  # K = 8: the three fits in turn, m = 257 (one full workgroup plus one row)
  k8 = [fits[j % K] for j in range(8)]
  rs = np.random.RandomState(5)
  U8, w8, r8 = rs.standard_normal((M, 8)), 0.05 + rs.random_sample(8), -2.0 + rs.random_sample(8)
  mc8 = [float(g['mean_consts'][j % K]) for j in range(8)]
  bv, bi, vals, samples = engine.mo_thompson_pointwise(k8, scal, w8, r8, g['Cp'], U8, X_halluc=g['Hp'], mean_consts=mc8,
                                                       return_vals=True, return_samples=True)
  for j in range(8):
    one = k8[j].thompson_pointwise(g['Cp'], np.ascontiguousarray(U8[:, j]), X_halluc=g['Hp'], mean_const=mc8[j], return_samples=True)[2]
    assert np.array_equal(samples[j], one), j
  assert np.array_equal(vals, _np_scalarise(scal, samples, w8, r8))
  assert bi == int(np.argmax(vals)) and bv == vals[bi]


# ---- 5. the arg-max rule and the errors -----------------------------------------------------------------------------
def test_argmax_rule_first_nan_else_first_maximum(engine, fits, gold):
  g = gold
  base = np.array([np.full(M, c) for c in g['mean_consts']])
  inf_twice = base.copy()
  inf_twice[1, [70, 256]] = np.inf                   # the maximum twice, in two workgroups: the first one
  bv, bi, vals, _ = _call(engine, fits, g, 'lin', mean_consts=None, mean_vals=inf_twice)
  assert bi == 70 and bv == np.inf and vals[256] == np.inf
  nan_late = inf_twice.copy()
  nan_late[2, [200, 256]] = np.nan                   # a NaN beats every number, the first NaN the second
  for scal in ('lin', 'tch'):
    bv, bi, vals, samples = _call(engine, fits, g, scal, mean_consts=None, mean_vals=nan_late)
    assert bi == 200 and np.isnan(bv), scal
    # np.minimum: a NaN in one objective makes the Tchebychev value NaN, whatever the others are
    assert np.isnan(vals[200]) and np.isnan(vals[256]) and np.isnan(samples[2, 200]) and np.isfinite(samples[0, 200])
    assert np.array_equal(np.isnan(vals), np.isnan(nan_late[2]))


def test_variance_not_positive_in_one_objective_is_the_ladders_error(engine):
  """ objective 1 of 2 the noise-0 GP of test_ts_pointwise_variance_not_positive_is_the_ladders_error, the candidates its
      training rows: where a variance is not positive the call raises the exhausted ladder's ValueError """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(3)
  X = rs.random_sample((70, 2))
  spec = KernelSpec('se', 2, 1.0, [0.5, 0.5])
  zero = engine.gp_fit(spec, X[:12], np.sin(4 * X[:12, 0]), 0.0)
  fine = engine.gp_fit(spec, X[:12], np.cos(3 * X[:12, 1]), 0.05)
  assert zero.jitter_power is None
  U = rs.standard_normal((12, 2))
  _, sd = zero.predict(X[:12])
  bad = ~(sd * sd > 0)
  print('variance not positive at %d of 12 training rows' % int(bad.sum()), sd)
  call = lambda rows, normals: engine.mo_thompson_pointwise([fine, zero], 'lin', [0.5, 0.5], None, rows, normals, return_vals=True)
  if bad.any():
    with pytest.raises(ValueError, match='Cholesky'):
      call(X[:12], U)
  if (~bad).any():                                   # the rows whose variances are positive alone draw fine
    assert np.all(np.isfinite(call(X[:12][~bad], U[~bad])[2]))


def test_bad_arguments_leave_the_outputs_alone(engine, fits, gold):
  from dragonfly_amd import _lib
  from dragonfly_amd.engine import Engine, KernelSpec
  g = gold
  w, r, mc = [np.ascontiguousarray(g[key], dtype=np.float64) for key in ('weights', 'reference_point', 'mean_consts')]
  w0 = w.copy()
  w0[1] = 0.0
  Cp, U, Hp = g['Cp'], np.ascontiguousarray(g['U']), g['Hp']
  gram = engine.gp_fit_gram(np.eye(70) * 2.0, g['Y'][0], 0.1)
  rs = np.random.RandomState(1)
  narrow = engine.gp_fit(KernelSpec('se', 4, 1.0, np.full(4, 0.5)), rs.random_sample((20, 4)), rs.standard_normal(20), 0.01)
  other = Engine()
  try:
    foreign = other.gp_fit(_spec(g, 0), g['Xp'], g['Y'][0] - mc[0], float(g['noises'][0]), handle_non_psd_kernels='project_first')
    p = lambda a: None if a is None else a.ctypes.data
    def raw(gps, scal=0, weights=w, refs=r, Xs=Cp, m=M, Xh=None, q=0, normals=U, consts=mc, means=None):
      k = len(gps)
      handles = (C.c_void_p * max(k, 1))(*[f.handle for f in gps])
      samples, vals = np.full((max(k, 1), M), -7.0), np.full(M, -7.0)
      bv, bi = C.c_double(-7.0), C.c_int64(-7)
      rc = engine.lib.dfh_mo_ts_pointwise(handles, k, scal, p(weights), p(refs), p(Xs), m, p(Xh), q, p(normals), p(consts), p(means),
                                          samples.ctypes.data, vals.ctypes.data, C.byref(bv), C.byref(bi))
      untouched = np.all(samples == -7.0) and np.all(vals == -7.0) and bv.value == -7.0 and bi.value == -7
      return rc, untouched
    assert raw(fits)[0] == 0 and raw(fits, scal=1, Xh=Hp, q=2)[0] == 0
    assert raw(fits, weights=w0)[0] == 0                       # a zero weight is fine for the linear scalarisation
    bad = dict(
      no_objective=raw([]), nine_objectives=raw([fits[0]] * 9, weights=np.full(9, 0.1), consts=np.zeros(9)),
      two_contexts=raw([fits[0], foreign, fits[2]]), two_dimensions=raw([fits[0], narrow, fits[2]]),
      gram_fitted=raw([fits[0], gram, fits[2]]), zero_weight_tch=raw(fits, scal=1, weights=w0), no_refs_tch=raw(fits, scal=1, refs=None),
      no_weights=raw(fits, weights=None), unknown_scalarisation=raw(fits, scal=2),
      no_candidate=raw(fits, m=0), no_candidates_pointer=raw(fits, Xs=None), negative_q=raw(fits, Xh=Hp, q=-1),
      q_without_points=raw(fits, Xh=None, q=2), no_normals=raw(fits, normals=None), no_prior_mean=raw(fits, consts=None, means=None))
    for name, (rc, untouched) in bad.items():
      assert rc == _lib.DFH_ERR_BAD_ARG and untouched, name
    foreign.free()
  finally:
    other.close()
  # the same through the engine: ValueError
  with pytest.raises(ValueError):
    engine.mo_thompson_pointwise(fits, 'tch', w0, r, Cp, U, mean_consts=mc)
  with pytest.raises(ValueError):
    engine.mo_thompson_pointwise(fits, 'tch', w, None, Cp, U, mean_consts=mc)


# ---- 6. more candidates than one posterior chunk --------------------------------------------------------------------
def test_across_posterior_chunks(engine, fits, gold):
  """ one chunk plus 257 rows, K = 2: the second chunk's draws and indices continue the first's """
  g = gold
  rs = np.random.RandomState(77)
  m = CHUNK + 257
  Cp = np.hstack([rs.random_sample((m, 2)), rs.randint(1, 8, (m, 1)).astype(float), rs.randint(0, 3, (m, 2)).astype(float)])
  U = rs.standard_normal((m, 2))
  two, w, r, mc = fits[:2], g['weights'][:2], g['reference_point'][:2], g['mean_consts'][:2]
  call = lambda rows, normals, **kw: engine.mo_thompson_pointwise(two, 'tch', w, r, rows, normals, mean_consts=mc, **kw)
  bv, bi, vals, samples = call(Cp, U, return_vals=True, return_samples=True)
  assert bi == int(np.argmax(vals)) and bv == vals[bi]
  assert np.array_equal(vals, _np_scalarise('tch', samples, w, r))
  tail = call(Cp[CHUNK:], U[CHUNK:], return_vals=True, return_samples=True)
  head = call(Cp[:1000], U[:1000], return_vals=True, return_samples=True)
  assert relerr(vals[CHUNK:], tail[2]) <= TOL and relerr(vals[:1000], head[2]) <= TOL
  assert relerr(samples[:, CHUNK:], tail[3]) <= TOL and relerr(samples[:, :1000], head[3]) <= TOL
  # a winner planted in the second chunk
  U2 = U.copy()
  U2[CHUNK + 200] = 1e3             # (every objective's draw there: its standard deviation is at least 0.07)
  assert call(Cp, U2)[1] == CHUNK + 200


# ---- 7. the fused host route against the per-point closure route, on the device -------------------------------------
class _CPDomain(object):
  """ what the route reads of the reference's CartesianProductDomain (there is no reference on the GPU machine) """
  dim = 5
  list_of_domains = ()

  def get_type(self):
    return 'cartesian_product'

  def has_constraints(self):
    return False


def _mirror_gps(g):
  from dragonfly_amd import kernel as Kn
  from dragonfly_amd.gp_core import GP

  class PackedCPGP(GP):
    _generic = False

    def _points_array(self, pts):
      return self.kernel.pack(pts)
  X = _unpack(g['Xp'])
  gps = []
  for j in range(K):
    kern = Kn.CartesianProductKernel(float(g['scales'][j]), [Kn.SEKernel(2, 1.0, g['se_bws'][j]),
                                                             Kn.MaternKernel(1, float(g['matern_nus'][j]), 1.0, g['matern_bws'][j]),
                                                             Kn.HammingKernel(g['hamming_ws'][j])])
    gps.append(PackedCPGP(X, list(g['Y'][j]), kern, lambda x, _c=float(g['mean_consts'][j]): np.array([_c] * len(x)),
                          float(g['noises'][j]), handle_non_psd_kernels='project_first'))
  return gps


def _unpack(P):
  return [[row[0:2].copy(), [int(row[2])], [int(row[3]), int(row[4])]] for row in P]


class _EngineSpy(object):
  """ counts the calls of the engine's multi-objective methods and of the fitted handles' per-objective ones """

  def __init__(self, monkeypatch, engine, handles):
    self.count = {}
    for obj, names in [(engine, ['mo_thompson_pointwise', 'mo_ucb_argmax', 'mo_thompson'])] + \
                      [(h, ['predict', 'thompson_pointwise', 'thompson', 'draw', 'predict_covar']) for h in handles]:
      for name in names:
        monkeypatch.setattr(obj, name, self._wrap(name, getattr(obj, name)), raising=False)

  def _wrap(self, name, fn):
    def call(*args, **kwargs):
      self.count[name] = self.count.get(name, 0) + 1
      return fn(*args, **kwargs)
    return call


@pytest.mark.parametrize('kind', ['lin_ts', 'tch_ts-halluc', 'lin_ucb', 'tch_ucb'])
def test_fused_step_is_the_per_point_step(engine, gold, kind, monkeypatch):
  """ one step on the mixed domain, the reference's sampler replaced by a stub that returns the fixture's candidates: ONE
      fused engine call returns the point that the same callable returns through the closure route, one posterior or draw
      per objective and call """
  from dragonfly_amd import gpb_acquisitions as A, multiobjective_gpb_acquisitions as MO
  g = gold
  gps = _mirror_gps(g)
  acq = kind.split('-')[0]
  pts = _unpack(g['Hp']) if kind.endswith('halluc') else []
  anc = Namespace(domain=_CPDomain(), acq_opt_method='rand', max_evals=M, t=int(g['t']), is_mf=False, handle_parallel='halluc',
                  eval_points_in_progress=pts, obj_weights=list(g['weights']), reference_point=list(g['reference_point']))
  cands = _unpack(g['Cp'])
  monkeypatch.setattr(A, '_cp_candidates', lambda anc_data: cands[:anc_data.max_evals])
  assert MO.mo_cp_acquisition_applies(acq, gps, anc)
  seed = 4322
  # the closure route of the same callable
  with monkeypatch.context() as mp:
    mp.setattr(MO, '_device_gps', lambda gps_, anc_: None)
    np.random.seed(seed)
    want = getattr(MO.asy, acq)(gps, anc)                    # (a sampler is called point by point; UCB on the whole list)
    state = np.random.get_state()
  if acq.endswith('_ucb'):
    # ... and the closure on one point per call, as the reference's maximiser calls it
    closure = MO._host_ucb_acquisition(acq[:3], gps, anc, MO._get_ucb_beta_th(5, anc.t))      # pylint: disable=protected-access
    assert want is cands[int(np.argmax([closure([x]) for x in cands]))]
  spy = _EngineSpy(monkeypatch, gps[0].device_gp.engine, [gp.device_gp for gp in gps])
  np.random.seed(seed)
  point = getattr(MO.asy, acq)(gps, anc)
  after = np.random.get_state()
  print(kind, 'engine calls', spy.count, 'winner', [i for i, c in enumerate(cands) if c is point])
  assert point is want and any(point is c for c in cands)
  assert spy.count == {'mo_thompson_pointwise' if acq.endswith('_ts') else 'mo_ucb_argmax': 1}
  assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]
