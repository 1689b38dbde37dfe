"""MI355X: product kernels whose factors are products themselves (factor_is_sum == DFH_FACTOR_PRODUCT, the joint kernel
of a multi-fidelity GP on a Cartesian-product domain) through the C-ABI.

 - Kernel VALUES in ulps, the rule of tests/kernel_value_check.py: on exact-argument inputs (its lattice: every squared
   distance is exact in fp64 on every route) the device is within max(2 ulp, 2 x the error of the NumPy restatement of
   the reference's order, tests/oracle_engine_cpmf.py), both against the long-double truth; 70 x 70 symmetric and
   37 x 70 cross, with and without Hamming parts, each on the route it names.  The prior variance k(x, x) of packed
   points (km_pack.hip) is held through the posterior standard deviation it enters.
 - Golden parity with the unmodified reference's CPMFGP and its BOCA step (tests/golden/cpmf_A_n70.npz, cpmf_B_n70.npz,
   tools/record_cpmf_golden.py): Gram and cross matrices under the same ulp rule, the truth from the fixture's own
   inputs in long double; alpha, lml, mu, sigma, acquisition values and point-wise draws at 1e-10 norm-wise, or the
   bound of the posterior's own conditioning (truth_bounds.gram_bounds) where that is larger; every arg-max and BOCA's
   (fidelity, point) equal -- every recorded decision has a relative margin above 1e-8.
 - The tuning routes: dfh_gp_lml_batch on nested candidates against per-candidate fits at 1e-12, at n = 50, 100 and 200,
   with the projection flag and without it (the one-launch forms build the Gram matrix inside the kernel).
 - Argument checks: what may not stand inside a product factor is DFH_ERR_BAD_ARG before any launch."""
from argparse import Namespace

import numpy as np
import pytest

from conftest import load_golden, relerr

import cpmf_cases as cases

pytestmark = pytest.mark.gpu
TOL = 1e-10
LD = np.longdouble


# ---- truth and the reference's order -----------------------------------------------------------------------------------
def _kvc():
  import kernel_value_check as kvc
  return kvc


def _truth(spec, X1, X2, exact):
  """ (long-double truth of a nested product descriptor, the largest Matern arg per entry, the 'tail' mask) """
  kvc = _kvc()
  X1 = X2 if X1 is None else X1
  shape = (len(X1), len(X2))
  factors = [LD(s) * np.ones(shape, dtype=LD) for s in spec.factor_scales]
  arg_max, arg_any = np.zeros(shape, dtype=LD), np.zeros(shape, dtype=LD)
  for kind, scale, nu, cols, par, f in zip(spec.sub_kinds, spec.sub_scales, spec.sub_nus, spec.groups, spec.sub_bandwidths,
                                           spec.group_factors):
    par = np.ravel(np.asarray(par, dtype=float))
    A, B = X1[:, cols], X2[:, cols]
    if kind == 'hamming':
      v = ((A[:, None, :] == B[None, :, :]) * par.astype(LD)).sum(axis=2)
    else:
      part = (kind, scale, nu, list(cols), par)
      if exact:
        v, arg = kvc.part_truth(part, *kvc.dsq_exact(part, X1, X2))
      else:
        diff = (A.astype(LD) / par.astype(LD))[:, None, :] - (B.astype(LD) / par.astype(LD))[None, :, :]
        v, arg = kvc.part_truth(part, (diff * diff).sum(axis=2), 0)
      arg_any = np.maximum(arg_any, arg)
      if kind == 'matern':
        arg_max = np.maximum(arg_max, arg)
    factors[f] = factors[f] * v
  out = LD(spec.scale) * np.ones(shape, dtype=LD)
  for fac in factors:
    out = out * fac
  has_matern = 'matern' in spec.sub_kinds
  return out, (arg_max if has_matern else None), np.asarray(arg_any > kvc.TAIL_ARG)


def _hold_to_ulp_rule(engine, spec, X1, X2, exact, what, route='generic'):
  from oracle_engine_cpmf import nested_product_matrix
  kvc = _kvc()
  K = kvc.km(engine, route, spec, X1, X2)
  truth, scale_by, tail = _truth(spec, X1, X2, exact)
  oracle = nested_product_matrix(spec, X2 if X1 is None else X1, X2)
  err_dev, err_ref = kvc.ulps(K, truth, scale_by), kvc.ulps(oracle, truth, scale_by)
  kvc.assert_clean(K, what)
  for name, mask in (('head', ~tail), ('tail', tail)):
    if not mask.any():
      continue
    limit = max(kvc.FLOOR_ULP, 2 * float(err_ref[mask].max()))
    print('%-34s %s: device %.3g ulp, reference order %.3g ulp, limit %.3g (%d entries, %d nonzero)'
          % (what, name, float(err_dev[mask].max()), float(err_ref[mask].max()), limit, int(mask.sum()), int((K[mask] != 0).sum())))
    assert float(err_dev[mask].max()) <= limit, (what, name)
  if X1 is None:
    assert np.array_equal(K, K.T)
  return K


def _lattice_spec(ham):
  """ fidelity factor: SE on column 0 (and a Hamming part of 2 columns); domain factor: Matern 2.5 on three columns, SE on
      one (and a Hamming part of 9 columns).  Bandwidths are powers of two, scales are not. """
  from dragonfly_amd.engine import KernelSpec
  groups, kinds, nus, bws, gf = [[0]], ['se'], [0.0], [np.array([1.0])], [0]
  at = 1
  if ham:
    groups.append([1, 2]); kinds.append('hamming'); nus.append(0.0); bws.append(np.array([0.7, 0.3])); gf.append(0)
    at = 3
  groups.append([at, at + 1, at + 2]); kinds.append('matern'); nus.append(2.5); bws.append(np.array([2.0, 1.0, 0.5])); gf.append(1)
  groups.append([at + 3]); kinds.append('se'); nus.append(0.0); bws.append(np.array([2.0])); gf.append(1)
  at += 4
  if ham:
    groups.append(list(range(at, at + 9))); kinds.append('hamming'); nus.append(0.0)
    bws.append(np.array([0.16, 0.08, 0.12, 0.1, 0.14, 0.06, 0.09, 0.11, 0.14])); gf.append(1)
    at += 9
  return KernelSpec('product', at, 1.6, groups=groups, sub_kinds=kinds, sub_scales=[1.0] * len(groups), sub_nus=nus,
                    sub_bandwidths=bws, group_factors=gf, factor_sums=[2, 2], factor_scales=[0.9, 1.25])


def _lattice_inputs(spec, n, seed):
  kvc = _kvc()
  X = np.zeros((n, spec.dim))
  rs = np.random.RandomState(seed)
  for kind, cols in zip(spec.sub_kinds, spec.groups):
    if kind == 'hamming':
      X[:, cols] = rs.randint(0, 3, size=(n, len(cols)))
    else:
      X[:, cols] = kvc.lattice_points(seed + cols[0], n, len(cols), 5, 2)
  return X


@pytest.mark.parametrize('ham', [False, True], ids=['euclidean-parts', 'with-hamming'])
@pytest.mark.parametrize('shape', ['sym70', 'cross37x70'])
def test_nested_descriptor_values_on_exact_arguments(engine, ham, shape):
  spec = _lattice_spec(ham)
  X2 = _lattice_inputs(spec, 70, 101)
  X1 = None if shape == 'sym70' else _lattice_inputs(spec, 37, 202)
  K = _hold_to_ulp_rule(engine, spec, X1, X2, True, 'nested-%s-%s' % ('ham' if ham else 'euc', shape))
  assert np.count_nonzero(K) > K.size // 10
  if X1 is None:
    # equal rows: the reference's bits (scale * 1.0, then every part's value at distance 0, in its order)
    from oracle_engine_cpmf import nested_product_matrix
    want = nested_product_matrix(spec, X2[:3])
    assert np.array_equal(np.diag(K)[:3], np.diag(want))


@pytest.mark.parametrize('ham', [False, True], ids=['euclidean-parts', 'with-hamming'])
def test_prior_variance_of_packed_points_enters_the_posterior(engine, ham):
  """ k(x, x) of a nested descriptor: the host's kxx without Hamming parts, k_prior_diag of km_pack.hip with them """
  from scipy.linalg import solve_triangular
  spec = _lattice_spec(ham)
  X, Xs = _lattice_inputs(spec, 70, 101), _lattice_inputs(spec, 37, 202)
  y = np.sin(X[:, 0]) + 0.1 * X[:, -1]
  fit = engine.gp_fit(spec, X, y, 0.05, handle_non_psd_kernels='project_first')
  _, sd = fit.predict(Xs)
  V = solve_triangular(fit.get_L(), engine.kernel_matrix(spec, Xs, X).T, lower=True)
  want = np.sqrt(np.diag(engine.kernel_matrix(spec, Xs)) - (V * V).sum(axis=0))
  print('posterior sd against diag(K) - |V|^2: %.3e' % relerr(sd, want))
  assert relerr(sd, want) <= TOL


# ---- golden parity -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['A', 'B'])
def gold(request):
  return request.param, load_golden('cpmf_%s_n70' % request.param)


@pytest.fixture(scope='module')
def fitted(engine, gold):
  name, g = gold
  spec = cases.spec_of(name, g)
  fit = engine.gp_fit(spec, g['Xp'], g['Y'] - float(g['mean_const']), float(g['noise']), handle_non_psd_kernels='project_first')
  joint = np.hstack([np.tile(g['f2o'], (len(g['Cp']), 1)), g['Cp']])
  return spec, fit, joint


@pytest.fixture(scope='module')
def bounds(engine, gold, fitted):
  """ truth_bounds.gram_bounds for this fixture's conditioning, as tests/test_gpu_cp_acq.py takes them """
  from oracle import ref_numpy as O
  from truth_bounds import gram_bounds
  name, g = gold
  spec, _, joint = fitted
  mean_c, noise = float(g['mean_const']), float(g['noise'])
  k_ss = np.diag(engine.kernel_matrix(spec, joint)).copy()
  K = O.project_symmetric_to_psd_cone(g['K'])
  out = gram_bounds(K, noise, g['Y'] - mean_c, dict(alpha=g['alpha'], lml=float(g['lml']), mu=g['mu_q0'], sd=g['sd_q0']),
                    engine.kernel_matrix(spec, joint, g['Xp']), k_ss, mean_const=mean_c)
  Xa = np.vstack([g['Xp'], g['Hp']])
  Ka = O.project_symmetric_to_psd_cone(engine.kernel_matrix(spec, Xa))
  out['sd_q2'] = gram_bounds(Ka, noise, np.zeros(len(Xa)), dict(sd=g['sd_q2']), engine.kernel_matrix(spec, joint, Xa), k_ss)['sd']
  print('bounds of fixture %s: %s' % (name, {k: '%.2e' % v for k, v in out.items()}))
  return out


def test_golden_gram_and_cross_matrices(engine, gold):
  name, g = gold
  spec = cases.spec_of(name, g)
  K = _hold_to_ulp_rule(engine, spec, None, g['Xp'], False, 'golden-%s-sym70' % name)
  Kc = _hold_to_ulp_rule(engine, spec, g['Tp'], g['Xp'], False, 'golden-%s-cross37x70' % name)
  assert relerr(K, g['K']) <= TOL and relerr(Kc, g['K_cross']) <= TOL


def test_golden_posterior(gold, fitted, bounds):
  name, g = gold
  _, fit, joint = fitted
  mean_c = float(g['mean_const'])
  errs = dict(alpha=relerr(fit.get_alpha(), g['alpha']), lml=relerr([fit.lml], [float(g['lml'])]))
  mu, sd = fit.predict(joint)
  errs['mu'], errs['sd'] = relerr(mu + mean_c, g['mu_q0']), relerr(sd, g['sd_q0'])
  _, sd2 = fit.predict(joint, X_halluc=g['Hp'])
  errs['sd_q2'] = relerr(sd2, g['sd_q2'])
  print('fixture %s: %s' % (name, {k: '%.2e' % v for k, v in errs.items()}))
  for key, err in errs.items():
    assert err <= bounds[key], (key, err, bounds[key])


def _fidelity_choice(g, fit, point_row):
  rows = np.hstack([g['Fp'], np.tile(point_row, (len(g['Fp']), 1))])
  _, stds = fit.predict(rows)
  return cases.boca_fidelity(g, stds / np.sqrt(float(g['kernel_scale'])))


@pytest.mark.parametrize('q', [0, 2])
@pytest.mark.parametrize('acq', ['ucb', 'ei', 'pi', 'ttei'])
def test_golden_acquisition_values_and_bocas_choice(gold, fitted, bounds, acq, q):
  name, g = gold
  _, fit, joint = fitted
  key = '%s_q%d' % (acq, q)
  best = float(np.max(g['Y']))
  params = {'ucb': (float(g['beta_q%d' % q]), 0.0), 'ei': (best, 0.0), 'pi': (best, 0.0)}.get(acq)
  rows = joint
  if acq == 'ttei':
    rows, params = joint[:128], tuple(g['ttei_params_q%d' % q])
    _, first, ei = fit.acq_argmax('ei', rows, params=(best, 0.0), mean_const=float(g['mean_const']),
                                  X_halluc=g['Hp'] if q else None, return_vals=True)
    assert relerr(ei, g['ttei_ei_q%d' % q]) <= max(TOL, bounds['mu'], bounds['sd_q2' if q else 'sd'])
    assert first == int(np.argmax(g['ttei_ei_q%d' % q]))
  bv, bi, vals = fit.acq_argmax(acq, rows, params=params, mean_const=float(g['mean_const']), X_halluc=g['Hp'] if q else None,
                                return_vals=True)
  err, bound = relerr(vals, g[key]), max(TOL, bounds['mu'], bounds['sd_q2' if q else 'sd'])
  print('%s %s relerr %.3e (bound %.2e) winner %d (reference %d, gap %.2e)' % (name, key, err, bound, bi, int(g[key + '_win']), float(g[key + '_gap'])))
  assert err <= bound
  assert bi == int(g[key + '_win']) == int(np.argmax(vals)) and bv == vals[bi]
  assert _fidelity_choice(g, fit, g['Cp'][bi]) == int(g[key + '_fidel'])


@pytest.mark.parametrize('q', [0, 2])
def test_golden_pointwise_draws_and_bocas_choice(gold, fitted, bounds, q):
  name, g = gold
  _, fit, joint = fitted
  key = 'ts_q%d' % q
  bv, bi, samples = fit.thompson_pointwise(joint, g['U'], X_halluc=g['Hp'] if q else None, mean_const=float(g['mean_const']),
                                           return_samples=True)
  err, bound = relerr(samples, g[key]), max(TOL, bounds['mu'], bounds['sd_q2' if q else 'sd'])
  print('%s %s relerr %.3e (bound %.2e) winner %d (reference %d, gap %.2e)' % (name, key, err, bound, bi, int(g[key + '_win']), float(g[key + '_gap'])))
  assert err <= bound
  assert bi == int(g[key + '_win']) == int(np.argmax(samples)) and bv == samples[bi]
  assert _fidelity_choice(g, fit, g['Cp'][bi]) == int(g[key + '_fidel'])


# ---- BOCA's step through the host route ------------------------------------------------------------------------------
class _CPDomain(object):
  def get_type(self):
    return 'cartesian_product'


class _Caller(object):
  def __init__(self, fidel_to_opt, fidels, g):
    self.fidel_to_opt, self.fidels, self.g = fidel_to_opt, fidels, g

  def get_candidate_fidels_and_cost_ratios(self, point, filter_by_cost=True):     # pylint: disable=unused-argument
    return list(self.fidels), list(self.g['cost_ratios'])

  def get_information_gap(self, fidels):
    return list(self.g['info_gaps'])


@pytest.mark.parametrize('acq,q', [('ucb', 0), ('ei', 2), ('ts', 2)])
def test_boca_step_on_a_product_domain_is_one_fused_call(engine, gold, acq, q, monkeypatch):
  """ dragonfly_amd.gpb_acquisitions.boca on the device GP of a product domain: the candidates packed by the domain
      kernel and joined with the packed fidel_to_opt in HBM, the pairs in progress packed jointly, ONE fused call for
      the point and one posterior call for the fidelity -- the reference's (fidelity, point).  (The class
      device_cpmfgp_class makes needs the reference's class body; a stand-in with the same hooks is registered.) """
  from dragonfly_amd import gpb_acquisitions as A, cartesian_product_gp as cpgp, kernel as K
  from dragonfly_amd.mf_gp import MFGP
  name, g = gold
  fidel, domain = cases.mirror_kernels(name, g)
  w = cases.fidel_width(name)

  class PackedCPMFGP(MFGP):
    _generic = False

    def _points_array(self, pts):
      return self.kernel.pack(pts)
  monkeypatch.setitem(cpgp._mf_classes, 'test', PackedCPMFGP)          # pylint: disable=protected-access
  mean_c = float(g['mean_const'])
  gp = PackedCPMFGP(cases.unpack(name, g['Xp'][:, :w], 'fidel'), cases.unpack(name, g['Xp'][:, w:], 'domain'), list(g['Y']),
                    K.CartesianProductKernel(float(g['kernel_scale']), [fidel, domain]), lambda x: np.array([mean_c] * len(x)),
                    float(g['noise']), handle_non_psd_kernels='project_first')
  gp.domain_kernel = domain
  cands = cases.unpack(name, g['Cp'], 'domain')
  fidels = cases.unpack(name, g['Fp'], 'fidel')
  f2o = cases.unpack(name, g['f2o'], 'fidel')[0]
  pairs = cases.unpack_pairs(name, g['Hp']) if q else []
  anc = Namespace(domain=_CPDomain(), acq_opt_method='rand', max_evals=len(cands), t=int(g['t']), is_mf=True, curr_acq=acq,
                  handle_parallel='halluc', eval_points_in_progress=[p[1] for p in pairs], eval_fidel_points_in_progress=pairs,
                  curr_max_val=float(np.max(g['Y'])), boca_thresh_coeff=float(g['thresh_coeff']), y_range=float(g['y_range']), boca_max_low_fidel_cost_ratio=0.9)
  assert A.cp_boca_applies(gp, anc) and A.cp_boca_view_applies(acq, A.FidelToOptGP(gp, f2o), anc)
  monkeypatch.setattr(A, '_cp_candidates', lambda anc_data: cands[:anc_data.max_evals])
  count = {}
  handle = gp.device_gp
  for meth in ('acq_argmax', 'thompson_pointwise', 'predict', 'thompson', 'draw', 'predict_covar'):
    def spy(*args, _fn=getattr(handle, meth), _m=meth, **kwargs):
      count[_m] = count.get(_m, 0) + 1
      return _fn(*args, **kwargs)
    monkeypatch.setattr(handle, meth, spy, raising=False)
  # the normals of the point-wise draw: the stream the fixture recorded
  monkeypatch.setattr(A, '_normals_in_hbm', lambda fitted: False)
  monkeypatch.setattr(A, '_standard_normals', lambda fitted, m, draws=1: np.asarray(g['U'][:m]))
  fidel_chosen, point = A.boca(getattr(A.asy, acq), gp, anc, _Caller(f2o, fidels, g))
  key = '%s_q%d' % (acq, q)
  print(name, key, 'engine calls', count)
  assert point is cands[int(g[key + '_win'])]
  want = int(g[key + '_fidel'])
  assert (fidel_chosen is f2o) if want < 0 else (fidel_chosen is fidels[want])
  assert count == {'thompson_pointwise' if acq == 'ts' else 'acq_argmax': 1, 'predict': 1}


# ---- tuning routes ---------------------------------------------------------------------------------------------------
def _nested_candidates(rs, nb, y_var):
  from dragonfly_amd.engine import KernelSpec
  specs, means, noises = [], [], []
  for c in range(nb):
    bw = lambda k: np.exp(rs.uniform(np.log(0.2), np.log(2.0), size=k))
    specs.append(KernelSpec('product', 6, float(np.exp(rs.uniform(np.log(0.3 * y_var), np.log(3 * y_var)))),
                            groups=[[0], [1], [2, 3, 4], [5]], sub_kinds=['se', 'matern', 'matern' if c % 2 else 'se', 'se'],
                            sub_scales=[1.0] * 4, sub_nus=[0.0, 1.5, 2.5 if c % 2 else 0.0, 0.0],
                            sub_bandwidths=[bw(1), bw(1), bw(3), bw(1)], group_factors=[0, 0, 1, 1], factor_sums=[2, 2],
                            factor_scales=[float(rs.uniform(0.7, 1.4)), float(rs.uniform(0.7, 1.4))]))
    means.append(float(0.2 * rs.randn()))
    noises.append(float(np.exp(rs.uniform(np.log(0.01 * y_var), np.log(0.2 * y_var)))))
  return specs, means, noises


@pytest.mark.parametrize('mode', ['project_first', 'guaranteed_psd'])
@pytest.mark.parametrize('n', [50, 100, 200])
def test_lml_batch_of_nested_candidates_is_the_single_fits(engine, n, mode):
  """ n = 50: the 64 x 64 one-launch form; n = 100: the Gram matrix built by the candidate's workgroup; n = 200: the Gram
      matrix from the kernel-matrix kernel.  With the projection flag every candidate is projected first. """
  rs = np.random.RandomState(7 * n)
  X = rs.rand(n, 6)
  Y = np.sin(4 * X[:, 2:].sum(axis=1)) * (0.5 + X[:, 0]) + 0.1 * rs.randn(n)
  specs, means, noises = _nested_candidates(rs, 5, float(Y.var()))
  lml = engine.gp_lml_batch(specs, X, Y, means, noises, handle_non_psd_kernels=mode)
  for c in range(5):
    one = engine.gp_fit(specs[c], X, Y - means[c], noises[c], handle_non_psd_kernels=mode)
    print('n = %d %s candidate %d: batch %.15g single %.15g' % (n, mode, c, lml[c], one.lml))
    assert abs(lml[c] - one.lml) <= 1e-12 * abs(one.lml)
    one.free()


# ---- argument checks ---------------------------------------------------------------------------------------------------
def test_what_may_not_stand_inside_a_product_factor_is_rejected_before_any_launch(engine):
  from dragonfly_amd.engine import KernelSpec
  X = np.random.RandomState(0).random_sample((6, 4))
  base = dict(groups=[[0], [1, 2], [3]], sub_scales=[1.0] * 3, sub_bandwidths=[np.ones(1), np.ones(2), np.ones(1)])
  kinds, nus = ['se', 'matern', 'se'], [0.0, 2.5, 0.0]
  ok = KernelSpec('product', 4, 1.0, sub_kinds=kinds, sub_nus=nus, group_factors=[0, 1, 1], factor_sums=[2, 2],
                  factor_scales=[1.0, 2.0], **base)
  assert engine.kernel_matrix(ok, X).shape == (6, 6)
  before = engine.counters()['km_dispatches']
  bad = [
    KernelSpec('product', 4, 1.0, sub_kinds=['se', 'poly', 'se'], sub_nus=[0.0, 2.0, 0.0], group_factors=[0, 1, 1],
               factor_sums=[2, 2], factor_scales=[1.0, 1.0], **base),                  # a polynomial group
    KernelSpec('product', 4, 1.0, sub_kinds=kinds, sub_nus=nus, group_factors=[0, 1, 0], factor_sums=[2, 2],
               factor_scales=[1.0, 1.0], **base),                                      # a factor's groups are adjacent
    KernelSpec('product', 4, 1.0, sub_kinds=kinds, sub_nus=nus, group_factors=[0, 2, 2], factor_sums=[2, 2, 2],
               factor_scales=[1.0] * 3, **base),                                       # ... and no factor is skipped
    KernelSpec('additive', 4, 1.0, sub_kinds=kinds, sub_nus=nus, group_factors=[0, 1, 1], factor_sums=[2, 2],
               factor_scales=[1.0, 1.0], **base),                                      # product factors in an additive kernel
  ]
  for spec in bad:
    with pytest.raises(ValueError):
      engine.kernel_matrix(spec, X)
    with pytest.raises(ValueError):
      engine.gp_fit(spec, X, np.zeros(6), 0.1)
  assert engine.counters()['km_dispatches'] == before


def test_mf_add_ucb_rejects_a_descriptor_with_product_factors(engine):
  """ BOCA's add-UCB is Euclidean-only in the reference: a plain fidelity factor and ONE additive domain factor """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(1)
  X = rs.random_sample((20, 4))
  spec = KernelSpec('product', 4, 1.0, groups=[[0], [1, 2], [3]], sub_kinds=['se', 'se', 'se'], sub_scales=[1.0] * 3,
                    sub_nus=[0.0] * 3, sub_bandwidths=[np.ones(1), np.ones(2), np.ones(1)], group_factors=[0, 1, 1],
                    factor_sums=[2, 2], factor_scales=[1.0, 1.0])
  fit = engine.gp_fit(spec, X, np.sin(X.sum(axis=1)), 0.1)
  with pytest.raises(ValueError):
    fit.mf_add_ucb_group([0.5], 0, 1.0, rs.random_sample((8, 2)))
  with pytest.raises(ValueError):
    fit.mf_add_ucb_all([0.5], [1.0, 1.0], [rs.random_sample((8, 2)), rs.random_sample((8, 1))])
