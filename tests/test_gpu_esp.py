"""MI355X: the ESP kernel (dragonfly/gp/kernel.py:671-744; DFH_KERNEL_ESP, csrc/km_esp.hip kernmat_esp_kernel) on the
device, against the REAL reference's outputs (tests/golden/esp_*.npz, tools/make_esp_golden.py).

Numerics: the reference's Newton-Girard recursion cancels as the order approaches d.  Where the order is at most
max(3, d/2), or d <= 10, the device agrees with the fixture within 1e-10 norm-wise; elsewhere its distance from the
truth -- the all-positive recursion e_m += k_c e_{m-1} in long double, computed here -- is at most
max(1e-10, 4 x the reference's own distance from it)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, relerr
from esp_fitter_replay import CASE_NAMES as FITTER_CASE_NAMES, check_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-10

KERNEL_CASES = ['se_d6_o1', 'se_d6_o2', 'se_d6_o3', 'se_d6_o6', 'm05_d5_o2', 'm05_d5_o5', 'm15_d5_o2', 'm15_d5_o5',
                'm25_d5_o2', 'm25_d5_o5', 'mix_d4_o3', 'se_d20_o10', 'se_d20_o20']
GP_CASES = ['gp_se_d6_o2', 'gp_m25_d5_o3']


def _esp(kind, dim, scale, order, bws, nus=None):
  from dragonfly_amd import kernel as K
  if kind == 'se':
    return K.ESPKernelSE(dim, scale, order, bws)
  return K.ESPKernelMatern(dim, list(nus), scale, order, bws)


def _first_rule(dim, order):
  return order <= max(3, dim / 2.0) or dim <= 10


def _truth(X1, X2, kind, scale, order, bws, nus):
  """ scale * e_order of the exact 1-D kernel values, by the all-positive recursion, in long double """
  ld = np.longdouble
  A, B = np.asarray(X1, dtype=ld) / np.asarray(bws, dtype=ld), np.asarray(X2, dtype=ld) / np.asarray(bws, dtype=ld)
  e = [np.ones((len(A), len(B)), dtype=ld)] + [np.zeros((len(A), len(B)), dtype=ld) for _ in range(order)]
  for c in range(A.shape[1]):
    dist = np.abs(A[:, c][:, None] - B[:, c][None, :])
    if kind == 'se':
      kc = np.exp(-dist * dist / 2)
    else:                     # norm_constant * unnormalised value (kernel.py:253, 259-270): u(dist) / u(0)
      nu, p = ld(nus[c]), int(nus[c])
      mult = np.sqrt(8 * nu) * dist
      u = np.zeros_like(dist)
      for i in range(p + 1):
        u += ld(math.factorial(p + i)) / ld(math.factorial(i) * math.factorial(p - i)) * mult ** (p - i)
      kc = u * np.exp(-np.sqrt(2 * nu) * dist) / (ld(math.factorial(2 * p)) / ld(math.factorial(p)))
    for m in range(order, 0, -1):
      e[m] = e[m] + kc * e[m - 1]
  return ld(scale) * e[order]


def _check_matrix(got, ref, truth, first_rule, what):
  if first_rule:
    assert relerr(got, ref) <= TOL, (what, relerr(got, ref))
  else:
    t = truth.astype(float)
    ref_err = float(np.max(np.abs(ref.astype(np.longdouble) - truth)) / np.max(np.abs(t)))
    dev_err = float(np.max(np.abs(got.astype(np.longdouble) - truth)) / np.max(np.abs(t)))
    assert dev_err <= max(TOL, 4 * ref_err), (what, dev_err, ref_err)


@pytest.mark.parametrize('case', KERNEL_CASES)
def test_kernel_matrix_matches_reference(engine, case):
  g = load_golden('esp_kernel_' + case)
  kind, dim, order = str(g['kind']), int(g['dim']), int(g['order'])
  kern = _esp(kind, dim, float(g['scale']), order, g['bws'], g['nus'])
  assert kern.has_device_spec()
  first = _first_rule(dim, order)
  for X2, ref in ((g['X1'], g['K11']), (g['X2'], g['K12'])):
    got = kern(g['X1'], g['X1'] if X2 is g['X1'] else X2)
    truth = None if first else _truth(g['X1'], X2, kind, float(g['scale']), order, g['bws'], g['nus'])
    _check_matrix(got, ref, truth, first, case)
  # the symmetric Gram matrix is symmetric bit for bit, with diag_add on its diagonal only
  K = engine.kernel_matrix(kern.to_spec(dim), g['X1'], None, diag_add=0.25)
  assert np.array_equal(K, K.T)
  K0 = kern(g['X1'], g['X1'])
  assert np.array_equal(np.diag(K), np.diag(K0) + 0.25)
  off = ~np.eye(len(K), dtype=bool)
  assert np.array_equal(K[off], K0[off])


def _gp(g):
  from dragonfly_amd.gp_core import GP
  kind, dim, order = str(g['kind']), int(g['dim']), int(g['order'])
  nus = [float(g['nu'])] * dim
  kern = _esp(kind, dim, float(g['scale']), order, g['bws'], nus)
  mean = float(g['mean'])
  return GP(list(g['X']), list(g['Y']), kern, lambda x, _c=mean: np.array([_c] * len(x)), float(g['noise']))


@pytest.mark.parametrize('case', GP_CASES)
def test_gp_matches_reference(engine, case):
  g = load_golden('esp_' + case)
  gp = _gp(g)
  assert not gp._generic           # pylint: disable=protected-access
  n = len(g['Y'])
  K = gp.kernel(g['X'], g['X']) + float(g['noise']) * np.eye(n)
  assert relerr(K, g['K']) <= TOL
  assert relerr(np.tril(gp.L), np.tril(g['L'])) <= TOL
  assert relerr(gp.alpha, g['alpha']) <= TOL
  assert abs(gp.compute_log_marginal_likelihood() - float(g['lml'])) <= TOL * abs(float(g['lml']))
  mu, sd = gp.eval(list(g['Xt']), uncert_form='std')
  assert relerr(mu, g['mu']) <= TOL and relerr(sd, g['sd']) <= TOL
  mu, cov = gp.eval(list(g['Xt']), uncert_form='covar')
  assert relerr(mu, g['mu']) <= TOL and relerr(cov, g['cov']) <= TOL


@pytest.mark.parametrize('kind', ['se', 'matern'])
def test_prior_variance_far_from_data(engine, kind):
  """ sd far from the data is sqrt(k(x, x)) = sqrt(kd.kxx): scale * e_order of the parts' values at distance 0 """
  from dragonfly_amd.gp_core import GP
  rs = np.random.RandomState(3)
  dim, order, scale = 7, 3, 1.7
  nus = [0.5, 1.5, 2.5, 2.5, 1.5, 0.5, 2.5]
  kern = _esp(kind, dim, scale, order, rs.uniform(0.2, 1.0, dim), nus)
  X = rs.rand(50, dim)
  gp = GP(list(X), list(np.sin(X.sum(axis=1))), kern, lambda x: np.zeros(len(x)), 0.01)
  far = list(1e4 + rs.rand(5, dim))
  _, sd = gp.eval(far, uncert_form='std')
  kxx = float(kern(np.zeros((1, dim)), np.zeros((1, dim)))[0, 0])
  assert np.allclose(sd ** 2, kxx, rtol=1e-12, atol=0), (sd ** 2, kxx)
  assert abs(kxx - scale * 35.0) <= 1e-12 * scale * 35.0        # C(7, 3) with every part 1 at distance 0


@pytest.mark.parametrize('n', [40, 100, 500, 3000])
def test_lml_batch_mixed_orders(engine, n):
  """ one dfh_gp_lml_batch over ESP candidates of mixed order and nu equals each candidate's own fit; at n <= 500
      also the host evaluation of the reference's formula (NumPy) """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(n)
  dim = 6
  X = rs.rand(n, dim)
  Y = np.sin(3 * X.sum(axis=1)) + 0.05 * rs.randn(n)
  specs, kerns, means, noises = [], [], [], []
  for c in range(12):
    order = 1 + c % dim
    kind = 'se' if c % 3 == 0 else 'matern'
    nus = [[0.5, 1.5, 2.5][(c + j) % 3] for j in range(dim)]
    kern = _esp(kind, dim, float(rs.uniform(0.5, 2.0)), order, rs.uniform(0.3, 1.5, dim), nus)
    kerns.append(kern)
    specs.append(kern.to_spec(dim))
    means.append(float(rs.uniform(-0.2, 0.2)))
    noises.append(float(rs.uniform(0.01, 0.1)))
  lml = engine.gp_lml_batch(specs, X, Y, means, noises)
  for c, spec in enumerate(specs):
    single = engine.gp_fit(spec, X, Y - means[c], noises[c]).lml
    assert abs(lml[c] - single) <= 1e-12 * max(1.0, abs(single)), (c, lml[c], single)
    if n <= 500:
      K = kerns[c]._host_compose(X, X) + noises[c] * np.eye(n)      # pylint: disable=protected-access
      L = np.linalg.cholesky(K)
      r = Y - means[c]
      a = np.linalg.solve(L.T, np.linalg.solve(L, r))
      want = -0.5 * r.dot(a) - np.log(np.diag(L)).sum() - n / 2.0 * np.log(2 * np.pi)
      assert abs(lml[c] - want) <= 1e-9 * max(1.0, abs(want)), (c, lml[c], want)


def test_large_gram_sampled_entries(engine):
  """ n = 8192, d = 16, order 4: a few thousand entries of the symmetric Gram matrix and of a cross matrix against
      the long-double truth """
  rs = np.random.RandomState(8192)
  n, dim, order = 8192, 16, 4
  bws = rs.uniform(0.3, 1.5, dim)
  kern = _esp('se', dim, 1.3, order, bws)
  X = rs.rand(n, dim)
  K = engine.kernel_matrix(kern.to_spec(dim), X, None)
  i, j = rs.randint(0, n, 3000), rs.randint(0, n, 3000)
  got = K[i, j]
  del K
  truth = np.array([_truth(X[a:a + 1], X[b:b + 1], 'se', 1.3, order, bws, None)[0, 0] for a, b in zip(i, j)])
  assert float(np.max(np.abs(got - truth)) / np.max(np.abs(truth.astype(float)))) <= TOL
  Xs = rs.rand(1000, dim)
  Kc = engine.kernel_matrix(kern.to_spec(dim), Xs, X)
  a, b = rs.randint(0, 1000, 2000), rs.randint(0, n, 2000)
  truth = np.array([_truth(Xs[p:p + 1], X[q:q + 1], 'se', 1.3, order, bws, None)[0, 0] for p, q in zip(a, b)])
  assert float(np.max(np.abs(Kc[a, b] - truth)) / np.max(np.abs(truth.astype(float)))) <= TOL


@pytest.mark.parametrize('n', [2111, 2625])
def test_poisoned_upper_triangle_changes_nothing(tmp_path, n):
  """ the lower-triangle-only fit build (n >= 2048) of an ESP kernel reads nothing above the diagonal """
  def run(path, extra):
    env = dict(os.environ)
    env.update(extra)
    res = subprocess.run([sys.executable, os.path.join(HERE, 'esp_upper_check.py'), str(n), path], env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith('OK'), (res.stdout[-2000:], res.stderr[-4000:])
    return dict(np.load(path))
  full = run(str(tmp_path / 'full.npz'), {'DFH_KM_LOWER_ONLY': '0'})
  poisoned = run(str(tmp_path / 'poisoned.npz'), {'DFH_TEST_POISON_L': '1'})
  for key, want in full.items():
    got = poisoned[key]
    assert np.all(np.isfinite(got)), key
    assert np.array_equal(got, want), (key, float(np.max(np.abs(got - want))))


def test_refusals(engine):
  """ add-UCB refuses an ESP GP; malformed ESP descriptors are refused with DFH_ERR_BAD_ARG (ValueError) """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(1)
  X = rs.rand(30, 4)
  good = dict(sub_kinds=['se'] * 4, sub_scales=[1.0] * 4, sub_nus=[0.0] * 4, sub_bandwidths=[[0.5]] * 4)
  gp = engine.gp_fit(KernelSpec('esp', 4, 1.0, nu=2, **good), X, np.sin(X.sum(axis=1)), 0.01)
  with pytest.raises(ValueError):
    gp.add_ucb_group(0, 1.0, rs.rand(10, 1))
  for order in (0, 5, 2.5):
    with pytest.raises(ValueError):
      engine.kernel_matrix(KernelSpec('esp', 4, 1.0, nu=order, **good), X)
  two_col = dict(good, sub_kinds=['se'] * 3, sub_scales=[1.0] * 3, sub_nus=[0.0] * 3,
                 sub_bandwidths=[[0.5, 0.5], [0.5], [0.5]])
  with pytest.raises(ValueError):
    engine.kernel_matrix(KernelSpec('esp', 4, 1.0, nu=2, groups=[[0, 1], [2], [3]], **two_col), X)
  with pytest.raises(ValueError):
    engine.kernel_matrix(KernelSpec('esp', 4, 1.0, nu=2, groups=[[1], [0], [2], [3]], **good), X)


def test_order_above_device_bucket_runs_on_host(engine):
  """ order 33 (d = 40): no device spec.  The kernel matrix is the reference's formula (kernel.py:693-726) over the
      columns' 1-D kernel matrices, bit for bit, and a GP with it is fitted in host-kernel mode (Gram matrix from the
      host, factorisation and posterior on the device) """
  from oracle_engine_esp import newton_girard
  from dragonfly_amd.gp_core import GP
  rs = np.random.RandomState(33)
  dim, order = 40, 33
  bws = rs.uniform(2.0, 4.0, dim)
  scale = 1.0 / math.comb(dim, order)
  kern = _esp('se', dim, scale, order, bws)
  assert not kern.has_device_spec()
  X = rs.rand(12, dim)
  got = kern(X, X)
  cols = [k(X[:, c:c + 1], X[:, c:c + 1]) for c, k in enumerate(kern.kernel_list)]
  assert np.array_equal(got, newton_girard(cols, order, scale))
  truth = _truth(X, X, 'se', scale, order, bws, None)
  assert float(np.max(np.abs(got - truth)) / np.max(np.abs(truth.astype(float)))) <= 1e-3     # cancellation at order d
  Y = np.sin(X.sum(axis=1))
  gp = GP(list(X), list(Y), kern, lambda x: np.zeros(len(x)), 0.5)
  assert gp._generic                  # pylint: disable=protected-access
  K = got + 0.5 * np.eye(len(X))
  L = np.linalg.cholesky(K)
  a = np.linalg.solve(L.T, np.linalg.solve(L, Y))
  want = -0.5 * Y.dot(a) - np.log(np.diag(L)).sum() - len(X) / 2.0 * np.log(2 * np.pi)
  assert abs(gp.compute_log_marginal_likelihood() - want) <= 1e-10 * abs(want)
  mu, _ = gp.eval(list(X[:3]), uncert_form='std')
  assert relerr(mu, got[:3].dot(a)) <= 1e-10


@pytest.mark.parametrize('name', FITTER_CASE_NAMES)
def test_standalone_fitter_reproduces_the_reference_choice(engine, name):
  """ kernel_type='esp' (se / matern members, tuned and fixed order, ML by 'rand' and 'pdoo', posterior sampling):
      under the reference's seed the fitter on the device chooses the reference's hyper-parameters, order and nu """
  check_case(name, load_golden('esp_fitter_d4_n30'), TOL)


def _anc(g, max_evals, in_progress=()):
  from argparse import Namespace
  from dragonfly_amd.oper_utils import EuclideanDomain
  bounds = np.array([[0.0, 1.0]] * int(g['dim']))
  return Namespace(max_evals=max_evals, t=len(g['Y']), domain=EuclideanDomain(bounds),
                   curr_max_val=float(g['Y'].max()), eval_points_in_progress=list(in_progress),
                   acq_opt_method='rand', handle_parallel='halluc', is_mf=False, domain_bounds=bounds)


@pytest.mark.parametrize('case', GP_CASES)
def test_gp_acquisitions_match_reference(engine, case):
  """ hallucinated sd; UCB / EI / PI / TTEI values and arg-max on the test points; the reference's asynchronous
      acquisitions recommend the same points under the same seed; a joint Thompson draw from the recorded normals """
  from dragonfly_amd import gpb_acquisitions as A
  g = load_golden('esp_' + case)
  gp = _gp(g)
  Xt = g['Xt']
  muh, sd_h = gp.eval_with_hallucinated_observations(list(Xt), list(g['Xh']), 'std')
  assert relerr(sd_h, g['sd_h']) <= TOL and relerr(muh, g['mu']) <= TOL
  best, mean_c = float(g['Y'].max()), float(g['mean'])
  for acq, params, key in (('ucb', (float(g['beta_th']), 0.0), 'val_ucb'), ('ei', (best, 0.0), 'val_ei'),
                           ('pi', (best, 0.0), 'val_pi'), ('ttei', (best, 0.3), 'val_ttei')):
    bv, bi, vals = gp.device_gp.acq_argmax(acq, Xt, params=params, mean_const=mean_c, return_vals=True)
    assert relerr(vals, g[key]) <= TOL, (acq, relerr(vals, g[key]))
    assert bi == int(np.argmax(g[key])) and bv == vals[bi], acq
  ci = GP_CASES.index(case)
  for ai, acq in enumerate(['ucb', 'ei', 'pi', 'ttei', 'ts']):
    np.random.seed(5100 + 10 * ci + ai)
    assert np.array_equal(getattr(A.asy, acq)(gp, _anc(g, 64)), g['asy_' + acq]), acq
  np.random.seed(6100 + ci)
  assert np.array_equal(A.asy.ucb(gp, _anc(g, 64, in_progress=[g['Xh'][0], g['Xh'][1]])), g['asy_ucb_halluc'])
  np.random.seed(9100 + ci)
  s = gp.draw_samples(1, list(Xt)).ravel()
  assert relerr(s, g['ts_sample']) <= 1e-8, relerr(s, g['ts_sample'])
  bv, bi, s2, _ = gp.device_gp.thompson(Xt, g['ts_U'], block=len(Xt), mean_const=mean_c, return_samples=True)
  assert np.array_equal(s2, s) and bi == int(np.argmax(s2)) and bv == s2[bi]
