"""MI355X: the fused acquisitions on Cartesian-product domains through the C-ABI -- dfh_gp_ts_pointwise (per candidate
the one-point draw the reference makes on these domains) and dfh_gp_acq_argmax on packed mixed candidates -- against what
the REAL reference computes one point per call (tests/golden/cp_acq_n70.npz, tools/record_cp_acq_golden.py), and the
fused host route of dragonfly_amd.gpb_acquisitions against today's per-point closure route on the same fitted GP.

The GP: 70 training points (one past the 64-row tile), a 2-D SE part, an integer Matern-2.5 column and a Hamming part of
two columns, fitted with 'project_first'; 257 candidates (one past a 256-thread workgroup), one of them a training row.
One tolerance, the project's: 1e-10 norm-wise.  Every arg-max in the fixture is decided by more than 1e-8 of the largest
value (checked when it was recorded), so winners are compared for equality."""
from argparse import Namespace
import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-10
ACQS = ('ucb', 'ei', 'pi', 'ttei')


@pytest.fixture(scope='module')
def gold():
  return load_golden('cp_acq_n70')


def _spec(g):
  from dragonfly_amd.engine import KernelSpec
  return KernelSpec('product', 5, float(g['scale']), groups=[[0, 1], [2], [3, 4]], sub_kinds=['se', 'matern', 'hamming'],
                    sub_scales=[1.0, 1.0, 1.0], sub_nus=[0.0, 2.5, 0.0], sub_bandwidths=[g['se_bw'], g['matern_bw'], g['hamming_w']])


@pytest.fixture(scope='module')
def fit(engine, gold):
  g = gold
  assert g['Xp'].shape == (70, 5) and g['Cp'].shape == (257, 5)
  assert np.array_equal(g['Cp'][int(g['dup_cand'])], g['Xp'][int(g['dup_train'])])
  return engine.gp_fit(_spec(g), g['Xp'], g['Y'] - float(g['mean_const']), float(g['noise']), handle_non_psd_kernels='project_first')


def _halluc(g, q):
  return g['Hp'] if q else None


@pytest.mark.parametrize('q', [0, 2])
def test_ts_pointwise_draws_the_reference_samples(fit, gold, q):
  g = gold
  bv, bi, samples = fit.thompson_pointwise(g['Cp'], g['U'], X_halluc=_halluc(g, q), mean_const=float(g['mean_const']), return_samples=True)
  want = g['ts_q%d' % q]
  err = relerr(samples, want)
  print('ts_pointwise q=%d relerr %.3e winner %d (reference %d, its top-two gap %.2e)' % (q, err, bi, int(g['ts_win_q%d' % q]),
                                                                                   float(g['ts_gap_q%d' % q])))
  assert err <= TOL
  assert bi == int(g['ts_win_q%d' % q]) == int(np.argmax(samples)) and bv == samples[bi]


def _host_truth_bound(engine, g, q):
  """ tests/truth_bounds.py's bound for the posterior mean and standard deviation of THIS conditioning: twice the distance
      of the reference's own double-precision values from the extended-precision posterior of the same (projected) Gram
      matrix, at least 1e-10.  A draw mu + sd u inherits the larger of the two. """
  from oracle import ref_numpy as O
  from truth_bounds import gram_bounds
  spec, X, Cp = _spec(g), g['Xp'], g['Cp']
  mean_c, noise = float(g['mean_const']), float(g['noise'])
  k_ss = np.diag(engine.kernel_matrix(spec, Cp)).copy()
  K = O.project_symmetric_to_psd_cone(engine.kernel_matrix(spec, X))
  b = gram_bounds(K, noise, g['Y'] - mean_c, dict(mu=g['mu_q0'], sd=g['sd_q0']), engine.kernel_matrix(spec, Cp, X), k_ss, mean_const=mean_c)
  out = max(b['mu'], b['sd'])
  if q:
    Xa = np.vstack([X, g['Hp']])
    Ka = O.project_symmetric_to_psd_cone(engine.kernel_matrix(spec, Xa))
    ba = gram_bounds(Ka, noise, np.zeros(len(Xa)), dict(sd=g['sd_q%d' % q]), engine.kernel_matrix(spec, Cp, Xa), k_ss)
    out = max(out, ba['sd'])
  return out


@pytest.mark.parametrize('q', [0, 2])
def test_ts_pointwise_agrees_with_the_block_one_draw(engine, fit, gold, q):
  """ dfh_gp_draw with block = 1 forms and factors a 1 x 1 covariance per candidate: the same draw by another route, its
      variance summed in another order -- not bit for bit, but within the bound of the posterior's own conditioning """
  g = gold
  mean_c = float(g['mean_const'])
  _, _, pointwise = fit.thompson_pointwise(g['Cp'], g['U'], X_halluc=_halluc(g, q), mean_const=mean_c, return_samples=True)
  blocks, bvs, bis, _ = fit.draw(g['Cp'], g['U'], 1, block=1, X_halluc=_halluc(g, q), mean_const=mean_c)
  bound = _host_truth_bound(engine, g, q)
  diff = relerr(pointwise, blocks[0])
  print('ts_pointwise against draw(block=1) q=%d: largest difference %.3e (norm-wise), bound %.3e' % (q, diff, bound))
  assert diff <= bound
  assert int(bis[0]) == int(np.argmax(pointwise))


def test_ts_pointwise_pointer_kinds_and_null_samples(engine, fit, gold):
  """ Xs and U as host and as device pointers, samples_out NULL: the same winner and the same bits """
  g = gold
  mean_c = float(g['mean_const'])
  bv, bi, samples = fit.thompson_pointwise(g['Cp'], g['U'], mean_const=mean_c, return_samples=True)
  dX, dU = engine.to_device(g['Cp']), engine.to_device(g['U'])
  for Xs, U in ((dX, dU), (dX, g['U']), (g['Cp'], dU)):
    got = fit.thompson_pointwise(Xs, U, mean_const=mean_c)                       # samples_out = NULL
    assert got == (bv, bi)
    assert np.array_equal(fit.thompson_pointwise(Xs, U, mean_const=mean_c, return_samples=True)[2], samples)
  # the raw entry point without any optional output
  rc = engine.lib.dfh_gp_ts_pointwise(fit.handle, g['Cp'].ctypes.data, 257, None, 0, g['U'].ctypes.data, mean_c, None, None, None, None)
  assert rc == 0
  # per-candidate prior means instead of the constant
  mv = np.full(257, mean_c)
  assert np.array_equal(fit.thompson_pointwise(g['Cp'], g['U'], mean_vals=mv, return_samples=True)[2], samples)


def test_ts_pointwise_draws_its_own_normals_from_the_global_stream(fit, gold):
  """ normals=None: Engine.random_normals(m) -- the stream of m calls of np.random.normal(size=(1, 1)), the cached second
      Gaussian included (m is odd), and the state those calls leave """
  g = gold
  mean_c = float(g['mean_const'])
  np.random.seed(991)
  U = np.array([np.random.normal(size=(1, 1))[0, 0] for _ in range(257)])
  state = np.random.get_state()
  want = fit.thompson_pointwise(g['Cp'], U, mean_const=mean_c, return_samples=True)
  np.random.seed(991)
  got = fit.thompson_pointwise(g['Cp'], None, mean_const=mean_c, return_samples=True)
  after = np.random.get_state()
  assert got[:2] == want[:2] and np.array_equal(got[2], want[2])
  assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_ts_pointwise_across_posterior_chunks(engine, fit, gold):
  """ more candidates than one posterior chunk holds (262144 rows): the second chunk's samples and indices continue the first's """
  g = gold
  rs = np.random.RandomState(77)
  m = 262144 + 257
  Cp = np.hstack([rs.random_sample((m, 2)), rs.randint(1, 8, (m, 1)).astype(float), rs.randint(0, 3, (m, 2)).astype(float)])
  U = rs.standard_normal(m)
  mean_c = float(g['mean_const'])
  bv, bi, samples = fit.thompson_pointwise(Cp, U, mean_const=mean_c, return_samples=True)
  assert bi == int(np.argmax(samples)) and bv == samples[bi]
  tail = fit.thompson_pointwise(Cp[262144:], U[262144:], mean_const=mean_c, return_samples=True)[2]
  head = fit.thompson_pointwise(Cp[:1000], U[:1000], mean_const=mean_c, return_samples=True)[2]
  assert relerr(samples[262144:], tail) <= TOL and relerr(samples[:1000], head) <= TOL
  # a winner planted in the second chunk
  U2 = U.copy()
  U2[262144 + 200] = 50.0
  assert fit.thompson_pointwise(Cp, U2, mean_const=mean_c)[1] == 262144 + 200


def test_ts_pointwise_variance_not_positive_is_the_ladders_error(engine):
  """ noise 0 and candidates that are the training rows: the posterior variances are rounding noise around zero, and a
      1 x 1 stable_cholesky fails on every rung for v <= 0 -- the ValueError of the exhausted ladder, from the fused call
      as from the block = 1 draw """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(3)
  n = 70
  X = rs.random_sample((n, 2))
  spec = KernelSpec('se', 2, 1.0, [0.5, 0.5])
  zero = engine.gp_fit(spec, X[:12], np.sin(4 * X[:12, 0]), 0.0)          # (condition 6e5: factors without the ladder)
  assert zero.jitter_power is None
  U = rs.standard_normal(12)
  _, sd = zero.predict(X[:12])
  bad = ~(sd * sd > 0)
  print('variance not positive at %d of 12 training rows' % int(bad.sum()), sd)
  assert bad.any()
  with pytest.raises(ValueError, match='Cholesky'):
    zero.thompson_pointwise(X[:12], U)
  with pytest.raises(ValueError, match='Cholesky'):
    zero.draw(X[:12], U, 1, block=1)
  # ... and the rows whose variance is positive alone draw fine
  if (~bad).any():
    _, _, s = zero.thompson_pointwise(X[:12][~bad], U[~bad], return_samples=True)
    assert np.all(np.isfinite(s))


@pytest.mark.parametrize('q', [0, 2])
@pytest.mark.parametrize('acq', ACQS)
def test_acq_argmax_on_packed_mixed_candidates(fit, gold, acq, q):
  g = gold
  tag = '%s_%%sq%d' % (acq, q)
  bv, bi, vals = fit.acq_argmax(acq, g['Cp'], params=tuple(g[tag % 'params_']), mean_const=float(g['mean_const']),
                                X_halluc=_halluc(g, q), return_vals=True)
  err = relerr(vals, g[tag % ''])
  print('%s q=%d relerr %.3e winner %d (reference %d, gap %.2e)' % (acq, q, err, bi, int(g[tag % 'win_']), float(g[tag % 'gap_'])))
  assert err <= TOL
  assert bi == int(g[tag % 'win_']) == int(np.argmax(vals)) and bv == vals[bi]


def test_argmax_rule_first_nan_else_first_maximum(fit, gold):
  g = gold
  m = 257
  base = np.full(m, float(g['mean_const']))
  inf_twice = base.copy()
  inf_twice[[70, 256]] = np.inf                      # the maximum twice, in two workgroups: the first one
  assert fit.thompson_pointwise(g['Cp'], g['U'], mean_vals=inf_twice)[1] == 70
  nan_late = inf_twice.copy()
  nan_late[[200, 256]] = np.nan                      # a NaN beats every number, the first NaN the second
  assert fit.thompson_pointwise(g['Cp'], g['U'], mean_vals=nan_late)[1] == 200
  # a duplicated candidate with the same normal: whatever the two samples are, the winner is np.argmax's
  w = int(g['ts_win_q0'])
  Cp, U = g['Cp'].copy(), g['U'].copy()
  Cp[w + 40], U[w + 40] = Cp[w], U[w]
  _, bi, samples = fit.thompson_pointwise(Cp, U, mean_const=float(g['mean_const']), return_samples=True)
  print('duplicated winner: samples', samples[w], samples[w + 40], 'winner', bi)
  assert bi == int(np.argmax(samples)) and bi in (w, w + 40)
  for acq in ('ucb', 'ei'):
    params = tuple(g['%s_params_q0' % acq])
    assert fit.acq_argmax(acq, g['Cp'], params=params, mean_vals=nan_late)[1] == 200


# ---- the fused host route against today's per-point route, on the device -------------------------------------------
class _Part(object):
  def __init__(self, bounds):
    self.bounds = np.asarray(bounds, dtype=float)
    self.dim = len(self.bounds)

  def get_type(self):
    return 'euclidean'


class _CPDomain(object):
  """ what the route reads of the reference's CartesianProductDomain (there is no reference on the GPU machine) """

  def __init__(self, parts=()):
    self.list_of_domains = list(parts)

  def get_type(self):
    return 'cartesian_product'

  def has_constraints(self):
    return False


def _mirror_gp(kern, X, Y, mean_c, noise):
  from dragonfly_amd.gp_core import GP

  class PackedCPGP(GP):
    _generic = False

    def _points_array(self, pts):
      return self.kernel.pack(pts)
  return PackedCPGP(X, list(Y), kern, lambda x: np.array([mean_c] * len(x)), noise, handle_non_psd_kernels='project_first')


def _unpack(P):
  return [[row[0:2].copy(), [int(row[2])], [int(row[3]), int(row[4])]] for row in P]


def _anc(domain, method, pts_in_progress=()):
  return Namespace(domain=domain, acq_opt_method=method, max_evals=257, t=71, curr_max_val=None, is_mf=False,
                   handle_parallel='halluc', eval_points_in_progress=list(pts_in_progress))


class _Spy(object):
  """ counts the calls of a fitted handle's methods and keeps the last result """

  def __init__(self, monkeypatch, handle, names):
    self.count, self.last = {}, {}
    for name in names:
      if hasattr(handle, name):
        monkeypatch.setattr(handle, name, self._wrap(name, getattr(handle, name)), raising=False)

  def _wrap(self, name, fn):
    def call(*args, **kwargs):
      self.count[name] = self.count.get(name, 0) + 1
      self.last[name] = fn(*args, **kwargs)
      return self.last[name]
    return call


@pytest.mark.parametrize('kind', ['ucb', 'ei', 'ttei', 'ts', 'ts-halluc'])
def test_fused_rand_step_is_the_per_point_step(engine, gold, kind, monkeypatch):
  """ one 'rand' step on the mixed domain: ONE fused engine call returns the point the per-point closures choose -- what
      maximise_acquisition's lambda x: acq_fn([x]) does today, candidate by candidate -- and its value to 1e-10 """
  from dragonfly_amd import gpb_acquisitions as A, kernel as K
  g = gold
  mean_c = float(g['mean_const'])
  kern = K.CartesianProductKernel(float(g['scale']), [K.SEKernel(2, 1.0, g['se_bw']), K.MaternKernel(1, 2.5, 1.0, g['matern_bw']),
                                                       K.HammingKernel(g['hamming_w'])])
  gp = _mirror_gp(kern, _unpack(g['Xp']), g['Y'], mean_c, float(g['noise']))
  pts = _unpack(g['Hp']) if kind == 'ts-halluc' else []
  acq = kind.split('-')[0]
  anc = _anc(_CPDomain(), 'rand', pts)
  anc.curr_max_val = float(np.max(g['Y']))
  cands = _unpack(g['Cp'])[:anc.max_evals]
  assert A.cp_acquisition_applies(acq, gp, anc)
  monkeypatch.setattr(A, '_cp_candidates', lambda anc_data: cands[:anc_data.max_evals])
  # today's route: one posterior (one draw) per candidate
  seed = 4322
  np.random.seed(seed)
  if acq == 'ts':
    sampler = A.get_gp_sampler_for_parallel_strategy(gp, anc)
    vals = np.array([float(sampler([x])[0]) for x in cands])
  else:
    gp_eval = A._get_gp_eval_for_parallel_strategy(gp, anc, 'std')      # pylint: disable=protected-access
    one = lambda x: tuple(float(v[0]) for v in gp_eval([x]))
    best = anc.curr_max_val
    ei = lambda mu, sd, ref: sd * A._expected_improvement_for_norm_diff((mu - ref) / sd)      # pylint: disable=protected-access
    if acq == 'ttei':
      coin = np.random.random()
      assert coin >= 0.5                                     # (this seed takes the two-step branch)
      post = [one(x) for x in cands[:128]]               # (half the budget, twice: max_evals // 2)
      ref_pt = cands[int(np.argmax([ei(mu, sd, best) for mu, sd in post]))]
      ref_mean, ref_std = one(ref_pt)
      vals = np.array([np.sqrt(ref_std ** 2 + sd ** 2) * A._expected_improvement_for_norm_diff(                  # pylint: disable=protected-access
          (mu - ref_mean) / np.sqrt(ref_std ** 2 + sd ** 2)) for mu, sd in post])
    else:
      post = [one(x) for x in cands]
      beta = A._get_ucb_beta_th(3.0, anc.t)                  # pylint: disable=protected-access
      vals = np.array([mu + beta * sd if acq == 'ucb' else ei(mu, sd, best) for mu, sd in post])
  want_idx = int(np.argmax(vals))
  # the fused route
  spy = _Spy(monkeypatch, gp.device_gp, ['acq_argmax', 'thompson_pointwise', 'predict', 'thompson', 'draw', 'predict_covar'])
  np.random.seed(seed)
  point = getattr(A.asy, acq)(gp, anc)
  fused = 'thompson_pointwise' if acq == 'ts' else 'acq_argmax'
  print(kind, 'engine calls', spy.count, 'winner', want_idx, 'value', spy.last[fused][0], 'per-point', vals[want_idx])
  assert point is cands[want_idx]
  assert relerr([spy.last[fused][0]], [vals[want_idx]]) <= TOL
  if acq == 'ttei':
    assert spy.count == {'acq_argmax': 2, 'predict': 1}
  else:
    assert spy.count == {fused: 1}


@pytest.mark.parametrize('method', ['direct', 'pdoo'])
def test_tree_search_on_an_all_float_product_is_the_per_point_search(engine, method, monkeypatch):
  """ two Euclidean parts (dimensions 2 and 1): the batched tree search over the flattened bounds visits the boxes of the
      one-callback-per-box search and returns its point, regrouped as the reference regroups it """
  from dragonfly_amd import gpb_acquisitions as A, kernel as K
  from dragonfly_amd.doo import pdoo_maximise
  rs = np.random.RandomState(8)
  n = 70
  P = np.hstack([rs.random_sample((n, 2)), -1 + 3 * rs.random_sample((n, 1))])
  Y = -np.sum((P[:, :2] - 0.3) ** 2, axis=1) - 0.5 * (P[:, 2] - 0.7) ** 2
  kern = K.CartesianProductKernel(1.2, [K.SEKernel(2, 1.0, [0.5, 0.7]), K.MaternKernel(1, 2.5, 1.0, [1.1])])
  X = [[row[:2].copy(), row[2:].copy()] for row in P]
  gp = _mirror_gp(kern, X, Y, float(np.mean(Y)), 0.01)
  domain = _CPDomain([_Part([[0, 1], [0, 1]]), _Part([[-1, 2]])])
  anc = _anc(domain, method)
  anc.max_evals = 400
  monkeypatch.setattr(A, '_fortran_direct_available', lambda: False)
  assert A.cp_acquisition_applies('ucb', gp, anc)
  beta = A._get_ucb_beta_th(3.0, anc.t)                      # pylint: disable=protected-access
  calls = []
  def per_point(x):
    calls.append(1)
    mu, sd = gp.eval([[x[:2], x[2:]]], 'std')
    return float(mu[0] + beta * sd[0])
  want_val, want_pt, _ = pdoo_maximise(per_point, np.array([[0, 1], [0, 1], [-1, 2]], dtype=float), anc.max_evals)
  spy = _Spy(monkeypatch, gp.device_gp, ['predict'])
  got = A.asy.ucb(gp, anc)
  print(method, 'per-point callbacks', len(calls), 'batched engine calls', spy.count)
  assert len(got) == 2 and np.array_equal(got[0], want_pt[:2]) and np.array_equal(got[1], want_pt[2:])
  mu, sd = gp.eval([got], 'std')
  assert relerr([mu[0] + beta * sd[0]], [want_val]) <= TOL
  assert spy.count['predict'] < len(calls) / 4
