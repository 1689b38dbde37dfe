"""dfh_gp_lml_grad_groups on the device: the gradient of the log marginal likelihood of additive and product kernels of
SE / Matern groups, one entry per bandwidth of every group, against the analytic gradient in np.longdouble with its own
Cholesky and inverse (tests/lml_grad_group_cases.py; checked against central differences of its own lml in
tests/test_lml_grad_groups_cpu.py).  Bound, norm-wise against max|g|: max(1e-10, twice the distance of the formula
evaluated in NumPy double precision from that truth) -- what is measured is the formula in double, never the device; the
bound applied is printed, and a bound above 1e-8 fails outright.
Shapes: n = 70 (one past the 64-row tile) with a one-column group padded to four and permuted columns; a group of 17
columns (past one 16-column LDS chunk) beside one of 3; 20 groups; n = 513 (one past the 512-block of the inverse), 1030
once; a duplicated row with a nu = 0.5 group; a fit that took jitter; a handle of dfh_gp_append.  Then the single kernels
bit for bit against dfh_gp_lml_grad, two calls bit for bit, the rejections, and the mirror's GPs."""
import ctypes as C

import numpy as np
import pytest

import lml_grad_cases as single_cases
import lml_grad_group_cases as cases

pytestmark = pytest.mark.gpu

TOL = 1e-10
WORST_BOUND = 1e-8                       # past this the rule would be hiding a defect, not measuring a rounding scale


def _fit(engine, case, **kwargs):
  data = case.data
  return engine.gp_fit(case.spec(), data['X'], data['y'] - data['mean'], data['noise'], **kwargs)


def _held_to_the_truth(grad, name, label, jitter=0.0):
  case, true_grad, _, bound, ref_dist = cases.truth_and_bound(name, jitter)
  assert grad.shape == true_grad.shape and np.all(np.isfinite(grad))
  err = cases.nwise(grad, true_grad)
  n, d = case.data['X'].shape
  print('%s: n %d d %d groups %d: device %.2e from the truth, the formula in double %.2e, bound applied %.2e'
        % (label, n, d, len(case.groups), err, ref_dist, bound))
  assert bound <= WORST_BOUND
  assert err <= bound
  return bound


def _check(engine, name):
  case = cases.make(name)
  fit = _fit(engine, case)
  assert fit.jitter_power is None
  grad, lml = fit.lml_grad_groups()
  assert lml == fit.lml
  assert fit.lml_grad_layout() == [(g, c) for g, grp in enumerate(case.groups) for c in grp]
  return _held_to_the_truth(grad, name, name)


@pytest.mark.parametrize('name', ['additive_n70', 'product_n70', 'product3_n70', 'additive_permuted_n70'])
def test_gradient_against_the_truth_n70(engine, name):
  assert _check(engine, name) == TOL


@pytest.mark.parametrize('name', ['additive_wide_n70', 'product_wide_n70'])
def test_gradient_with_a_group_past_one_chunk(engine, name):
  _check(engine, name)


def test_gradient_with_twenty_groups(engine):
  assert _check(engine, 'additive_20groups_n130') == TOL


@pytest.mark.parametrize('name', ['additive_n513', 'product_n513'])
def test_gradient_with_two_blocks_of_the_inverse(engine, name):
  assert _check(engine, name) == TOL


def test_gradient_with_three_blocks_of_the_inverse(engine):
  assert _check(engine, 'additive_n1030') == TOL


def test_a_duplicated_row_adds_nothing_to_a_nu05_group(engine):
  """ nu = 0.5, where dk/d(dsq) is unbounded at 0: finite, and the truth with that pair's bandwidth terms zero """
  assert _check(engine, 'additive_dup_nu05') == TOL


def test_gradient_of_a_fit_that_took_jitter(engine):
  """ noise 0 and two rows 1e-9 apart (one label): the factored matrix is K + jitter I, and the gradient is that matrix's """
  case = cases.make('product_jitter')
  fit = _fit(engine, case)
  assert fit.jitter_power is not None
  max_diag = case.data['scale'] * float(np.prod(case.sub_scales)) + case.data['noise']
  jitter = 10.0 ** fit.jitter_power * max_diag           # general_utils.py:166-203
  print('jitter power', fit.jitter_power)
  _held_to_the_truth(fit.lml_grad_groups()[0], 'product_jitter', 'product jitter', jitter)


def test_gradient_of_an_appended_handle(engine):
  """ dfh_gp_append's handle holds the rebuilt fit: the gradient of all 70 rows """
  case = cases.make('additive_n70')
  X, yc = case.data['X'], case.data['y'] - case.data['mean']
  first = engine.gp_fit(case.spec(), X[:65], yc[:65], case.data['noise'])
  grown = first.append(X[65:], yc)
  assert grown.n == 70
  assert _held_to_the_truth(grown.lml_grad_groups()[0], 'additive_n70', 'appended') == TOL


@pytest.mark.parametrize('kind,nu', [('se', 0.0), ('matern', 2.5)])
def test_single_kernels_return_the_bits_of_lml_grad(engine, kind, nu):
  from dragonfly_amd.engine import KernelSpec
  case = single_cases.make_case(70, 5, 21, 1e-2)
  fit = engine.gp_fit(KernelSpec(kind, 5, case['scale'], case['bw'], nu=nu), case['X'], case['y'] - case['mean'], case['noise'])
  assert fit.lml_grad_layout() == [(0, c) for c in range(5)]
  grouped, lml = fit.lml_grad_groups()
  plain, lml_plain = fit.lml_grad()
  assert lml == lml_plain
  assert np.array_equal(grouped, plain)


def test_the_gradient_is_the_same_bits_on_every_call(engine):
  fit = _fit(engine, cases.make('additive_n513'))
  first, _ = fit.lml_grad_groups()
  second, _ = fit.lml_grad_groups()
  assert np.array_equal(first, second)


# ---- rejections -------------------------------------------------------------------------------------------------------
def _rejected(engine, fit, nbw, length=None):
  from dragonfly_amd import _lib
  grad = np.zeros(nbw + 3)
  rc = engine.lib.dfh_gp_lml_grad_groups(fit.handle, grad.ctypes.data_as(C.c_void_p), nbw + 3 if length is None else length, None)
  msg = _lib.last_error()
  print(msg)
  assert rc == _lib.DFH_ERR_BAD_ARG and msg.startswith('dfh_gp_lml_grad_groups')
  return msg


def test_rejections_name_their_case(engine):
  from dragonfly_amd.engine import KernelSpec
  case = single_cases.make_case(40, 3, 21, 1e-2)
  X, yc, bw = case['X'], case['y'] - case['mean'], case['bw']

  def grouped(kind, sub_kinds, sub_nus=(0.0, 0.0), sub_bandwidths=None, data=X, **kwargs):
    spec = KernelSpec(kind, 3, 1.5, groups=[[0, 1], [2]], sub_kinds=list(sub_kinds), sub_scales=[1.0, 1.0], sub_nus=list(sub_nus),
                      sub_bandwidths=[bw[:2], bw[2:]] if sub_bandwidths is None else sub_bandwidths, **kwargs)
    return engine.gp_fit(spec, data, yc, 1e-2)

  K = engine.kernel_matrix(KernelSpec('se', 3, case['scale'], bw), X)
  assert 'Gram' in _rejected(engine, engine.gp_fit_gram(K, yc, 1e-2), 0)
  se = KernelSpec('se', 3, case['scale'], bw)
  assert 'project_first' in _rejected(engine, engine.gp_fit(se, X, yc, 1e-2, handle_non_psd_kernels='project_first'), 3)
  assert 'try_before_project' in _rejected(engine, engine.gp_fit(se, X, yc, 1e-2, handle_non_psd_kernels='try_before_project'), 3)
  assert 'POLY' in _rejected(engine, engine.gp_fit(KernelSpec('poly', 3, 1.0, [1.0, 1.0, 1.0], nu=2), X, yc, 1e-2), 3)
  assert 'POLY part' in _rejected(engine, grouped('additive', ['se', 'poly'], (0.0, 2.0), [bw[:2], [1.0]]), 3)
  assert 'EXPDECAY part' in _rejected(engine, grouped('product', ['se', 'expdecay'], (0.0, 1.0), [bw[:2], [2.0]]), 3)
  Xh = X.copy()
  Xh[:, 2] = np.floor(3 * Xh[:, 2])                      # category codes for the Hamming column
  assert 'HAMMING part' in _rejected(engine, grouped('product', ['se', 'hamming'], sub_bandwidths=[bw[:2], [1.0]], data=Xh), 3)
  assert 'nu above 2.5' in _rejected(engine, grouped('additive', ['se', 'matern'], (0.0, 3.5)), 3)
  esp = KernelSpec('esp', 3, 1.5, nu=2, sub_kinds=['se'] * 3, sub_scales=[1.0] * 3, sub_nus=[0.0] * 3, sub_bandwidths=[[b] for b in bw])
  assert 'ESP' in _rejected(engine, engine.gp_fit(esp, X, yc, 1e-2), 3)
  nested = grouped('product', ['se', 'se'], group_factors=[0, 1], factor_sums=[False, True], factor_scales=[1.0, 1.0])
  assert 'nested factor' in _rejected(engine, nested, 3)
  msg = _rejected(engine, grouped('additive', ['se', 'matern'], (0.0, 2.5)), 3, length=5)
  assert 'len' in msg and '6' in msg
  assert 'len' in _rejected(engine, engine.gp_fit(se, X, yc, 1e-2), 3, length=7)


def test_the_engine_raises_what_the_library_rejects(engine):
  from dragonfly_amd.engine import KernelSpec
  case = single_cases.make_case(40, 3, 21, 1e-2)
  fit = engine.gp_fit(KernelSpec('poly', 3, 1.0, [1.0, 1.0, 1.0], nu=2), case['X'], case['y'] - case['mean'], 1e-2)
  with pytest.raises(ValueError, match='POLY'):
    fit.lml_grad_groups()


# ---- the mirror -------------------------------------------------------------------------------------------------------
def _count_calls(monkeypatch, handle, names):
  """ wraps the fitted handle's methods; the returned dict counts their calls """
  count = {}

  def wrap(name, fn):
    def call(*args, **kwargs):
      count[name] = count.get(name, 0) + 1
      return fn(*args, **kwargs)
    return call
  for name in names:
    monkeypatch.setattr(handle, name, wrap(name, getattr(handle, name)), raising=False)
  return count


def test_additive_mirror_gp_against_the_truth(engine, monkeypatch):
  case, true_grad, _, bound, _ = cases.truth_and_bound('additive_permuted_n70')
  gp = cases.additive_mirror_gp(case)
  count = _count_calls(monkeypatch, gp.device_gp, ['lml_grad_groups', 'lml_grad'])
  got = cases.named_components(gp, case, [('dim_bandwidths', c) for c in case.columns])
  assert count == {'lml_grad_groups': 1}
  err = cases.nwise(got, cases.wanted(case, true_grad))
  print('additive mirror: device %.2e from the truth, bound applied %.2e' % (err, bound))
  assert bound == TOL and err <= bound
  gp.add_data_single(np.full(6, 0.4), 0.1)               # new data: the cached gradient goes with the posterior
  assert gp.compute_grad_log_marginal_likelihood('scale') != got[0]


def test_mf_mirror_gp_against_the_truth(engine, monkeypatch):
  case, true_grad, _, bound, _ = cases.truth_and_bound('product_n70')
  gp = cases.mf_mirror_gp(case)
  count = _count_calls(monkeypatch, gp.device_gp, ['lml_grad_groups', 'lml_grad'])
  names = [('fidel_dim_bandwidths', c) for c in range(2)] + [('domain_dim_bandwidths', c) for c in range(3)]
  got = cases.named_components(gp, case, names)
  assert count == {'lml_grad_groups': 1}
  err = cases.nwise(got, cases.wanted(case, true_grad))
  print('multi-fidelity mirror: device %.2e from the truth, bound applied %.2e' % (err, bound))
  assert bound == TOL and err <= bound


def test_mirror_gp_says_what_the_device_cannot_differentiate(engine):
  from dragonfly_amd import kernel as K
  case = cases.make('product_n70')
  bw = case.data['bw']
  additive_domain = K.AdditiveKernel(1.0, [K.SEKernel(2, 1.0, bw[2:4]), K.SEKernel(1, 1.0, bw[4:5])], [[0, 1], [2]])
  with pytest.raises(NotImplementedError, match='nested factor'):
    cases.mf_mirror_gp(case, domain_kernel=additive_domain).compute_grad_log_marginal_likelihood('scale')
