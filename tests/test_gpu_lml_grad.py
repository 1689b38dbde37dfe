"""dfh_gp_lml_grad on the device: the gradient of the log marginal likelihood of a fitted GP in the tuner's coordinates
(log scale, log bandwidths, log noise variance, constant mean), against
 - the reference's own GP.compute_grad_log_marginal_likelihood (tests/golden/lml_grad_ref.npz, recorded by
   tools/record_lml_grad_golden.py), to the project's 1e-10 norm-wise.  Matern nu = 0.5 is NOT compared with the
   reference: its recorded value is 2.3e-8 (norm-wise) from the extended-precision truth -- the rounding of the
   diagonal's squared distance, 1e-16 instead of 0, moves a kernel that is not smooth at 0 by 1e-8 -- so nu = 0.5 is
   held to the truth only;
 - the analytic gradient in np.longdouble with its own Cholesky and inverse (tests/lml_grad_cases.py), itself checked
   against central differences of its own lml to 1e-6.  Bound, norm-wise against max|g|: max(1e-10, twice the distance of
   the reference's formula evaluated in NumPy double precision from that truth) -- what is measured is the formula in
   double, never the device; the bound applied is printed.
Shapes: n = 70 (one past the 64-row tile), 513 (one past the 512-block of the inverse), 1030 once; d = 3 and 33 (packed
width past 32); SE and the three nu; a fit that took jitter; a duplicated row with nu = 0.5.  Then the rejections, and
GP.compute_grad_log_marginal_likelihood on the mirror with its one engine call per GP."""
import ctypes as C

import numpy as np
import pytest

import lml_grad_cases as cases
from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-10
KERNELS = {'se': ('se', 0.0), 'matern05': ('matern', 0.5), 'matern15': ('matern', 1.5), 'matern25': ('matern', 2.5)}


@pytest.fixture(scope='module')
def gold():
  return load_golden('lml_grad_ref')


def _gold_case(gold, same=False):
  bw = np.full(3, float(gold['same_bw'])) if same else gold['bw']
  return dict(X=gold['X'], y=gold['y'], bw=bw, scale=float(gold['scale']), noise=float(gold['noise']), mean=float(gold['mean']))


def _fit(engine, kind, nu, case, **kwargs):
  from dragonfly_amd.engine import KernelSpec
  d = case['X'].shape[1]
  return engine.gp_fit(KernelSpec(kind, d, case['scale'], case['bw'], nu=nu), case['X'], case['y'] - case['mean'],
                       case['noise'], **kwargs)


def _nwise(got, want):
  """ norm-wise distance against max|want|, in extended precision """
  want = np.asarray(want, dtype=np.longdouble)
  return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize('name', ['se', 'matern15', 'matern25'])
def test_gradient_is_the_reference_s(engine, gold, name):
  kind, nu = KERNELS[name]
  case = _gold_case(gold)
  fit = _fit(engine, kind, nu, case)
  grad, lml = fit.lml_grad()
  assert lml == fit.lml
  got = grad.copy()
  got[1:4] /= case['bw']                                 # the reference differentiates in bw, not in log bw
  print(name, 'lml', relerr([lml], [gold[name + '_lml']]), 'gradient', relerr(got, gold[name + '_grad']))
  assert relerr([lml], [gold[name + '_lml']]) <= TOL
  assert relerr(got, gold[name + '_grad']) <= TOL


def test_the_truth_is_the_derivative_of_its_own_lml(gold):
  """ once per kernel: the analytic gradient in extended precision against central differences of the same lml """
  for name, (kind, nu) in KERNELS.items():
    case = _gold_case(gold)
    true_grad, _ = cases.truth(kind, nu, case)
    err = _nwise(cases.central_differences(kind, nu, case), true_grad)
    print(name, 'truth against central differences', err)
    assert err <= 1e-6


def _check_against_truth(engine, kind, nu, case, label, expect_jitter=False):
  fit = _fit(engine, kind, nu, case)
  jitter = 0.0
  if expect_jitter:
    assert fit.jitter_power is not None
    jitter = 10.0 ** fit.jitter_power * (case['scale'] + case['noise'])      # general_utils.py:166-203
  else:
    assert fit.jitter_power is None
  grad, _ = fit.lml_grad()
  assert np.all(np.isfinite(grad))
  true_grad, _ = cases.truth(kind, nu, case, jitter)
  bound, ref_dist = cases.gradient_bound(kind, nu, case, true_grad, jitter)
  err = _nwise(grad, true_grad)
  print('%s: n %d d %d condition %.1e: device %.2e from the truth, the formula in double %.2e, bound applied %.2e'
        % (label, case['X'].shape[0], case['X'].shape[1], cases.condition_number(kind, nu, case, jitter), err, ref_dist, bound))
  assert err <= bound
  return bound


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_gradient_against_the_truth_n70(engine, gold, name):
  kind, nu = KERNELS[name]
  bound = _check_against_truth(engine, kind, nu, _gold_case(gold), name)
  if name != 'matern05':
    assert bound == TOL                                  # these sit under the flat 1e-10


@pytest.mark.parametrize('name', ['se', 'matern25'])
def test_gradient_with_a_packed_width_past_32(engine, name):
  kind, nu = KERNELS[name]
  assert _check_against_truth(engine, kind, nu, cases.make_case(70, 33, 5, 1e-2), name + ' d33') == TOL


@pytest.mark.parametrize('name', ['se', 'matern05', 'matern25'])
def test_gradient_with_two_blocks_of_the_inverse(engine, name):
  kind, nu = KERNELS[name]
  bound = _check_against_truth(engine, kind, nu, cases.make_case(513, 3, 7, 1e-2), name + ' n513')
  if name != 'matern05':
    assert bound == TOL


def test_gradient_with_three_blocks_of_the_inverse(engine):
  _check_against_truth(engine, 'se', 0.0, cases.make_case(1030, 3, 9, 1e-2), 'se n1030')


def test_gradient_of_a_fit_that_took_jitter(engine):
  """ noise 0 and two rows 1e-9 apart (one label): the factored matrix is K + jitter I, and the gradient is that matrix's.
      At condition 2.8e12 the entries of A^-1 reach 1 / jitter: the scale component holds its bound only because
      tr(A^-1 K) is taken as tr(L^-1 K L^-T), never as a sum over the entries of A^-1 (4.89e-9 from the truth that way,
      1.46e-10 now, against the reference's formula in double at 1.26e-10 and a bound of 2.51e-10). """
  _check_against_truth(engine, 'se', 0.0, cases.make_case(70, 3, 13, 0.0, near_dup=1e-9), 'se jitter', expect_jitter=True)


def test_a_duplicated_row_adds_nothing_to_the_bandwidth_components(engine):
  """ nu = 0.5, where dK/d(dsq) is unbounded at 0: finite, and the truth with that pair's bandwidth terms zero """
  _check_against_truth(engine, 'matern', 0.5, cases.make_case(70, 3, 17, 1e-2, dup=True), 'matern05 duplicate')


def test_the_gradient_is_the_same_bits_on_every_call(engine, gold):
  fit = _fit(engine, 'matern', 2.5, cases.make_case(513, 3, 7, 1e-2))
  first, _ = fit.lml_grad()
  second, _ = fit.lml_grad()
  assert np.array_equal(first, second)


# ---- rejections -------------------------------------------------------------------------------------------------------
def _rejected(engine, fit, d):
  from dragonfly_amd import _lib
  grad = np.zeros(d + 3)
  rc = engine.lib.dfh_gp_lml_grad(fit.handle, grad.ctypes.data_as(C.c_void_p), None)
  return rc, _lib.last_error()


def test_rejections_name_their_case(engine, gold):
  from dragonfly_amd import _lib
  from dragonfly_amd.engine import KernelSpec
  case = _gold_case(gold)
  X, yc = case['X'], case['y'] - case['mean']
  additive = KernelSpec('additive', 3, 1.5, groups=[[0, 1], [2]], sub_kinds=['se', 'matern'], sub_scales=[1.25, 0.8],
                        sub_nus=[0.0, 2.5], sub_bandwidths=[[0.5, 0.6], [0.7]])
  rc, msg = _rejected(engine, engine.gp_fit(additive, X, yc, 1e-2), 3)
  print(msg)
  assert rc == _lib.DFH_ERR_BAD_ARG and 'ADDITIVE' in msg
  Xh = X.copy()
  Xh[:, 2] = np.floor(3 * Xh[:, 2])                      # category codes for the Hamming column
  product = KernelSpec('product', 3, 1.5, groups=[[0, 1], [2]], sub_kinds=['se', 'hamming'], sub_scales=[1.0, 1.0],
                       sub_nus=[0.0, 0.0], sub_bandwidths=[[0.5, 0.6], [1.0]])
  rc, msg = _rejected(engine, engine.gp_fit(product, Xh, yc, 1e-2), 3)
  print(msg)
  assert rc == _lib.DFH_ERR_BAD_ARG and 'PRODUCT' in msg
  K = engine.kernel_matrix(KernelSpec('se', 3, case['scale'], case['bw']), X)
  rc, msg = _rejected(engine, engine.gp_fit_gram(K, yc, 1e-2), 0)
  print(msg)
  assert rc == _lib.DFH_ERR_BAD_ARG and 'Gram' in msg
  rc, msg = _rejected(engine, _fit(engine, 'se', 0.0, case, handle_non_psd_kernels='project_first'), 3)
  print(msg)
  assert rc == _lib.DFH_ERR_BAD_ARG and 'project_first' in msg


# ---- the mirror -------------------------------------------------------------------------------------------------------
class _Spy(object):
  """ counts the calls of a fitted handle's methods """

  def __init__(self, monkeypatch, handle, names):
    self.count = {}
    for name in names:
      monkeypatch.setattr(handle, name, self._wrap(name, getattr(handle, name)), raising=False)

  def _wrap(self, name, fn):
    def call(*args, **kwargs):
      self.count[name] = self.count.get(name, 0) + 1
      return fn(*args, **kwargs)
    return call


def _mirror_gp(kind, nu, case, bandwidths):
  from dragonfly_amd import kernel as K
  from dragonfly_amd.euclidean_gp import EuclideanGP
  from dragonfly_amd.gp_core import ConstantMean
  kern = K.SEKernel(3, case['scale'], bandwidths) if kind == 'se' else K.MaternKernel(3, nu, case['scale'], bandwidths)
  return EuclideanGP(case['X'], case['y'], kern, ConstantMean(case['mean']), case['noise'])


@pytest.mark.parametrize('name', ['se', 'matern25'])
def test_mirror_gp_returns_the_reference_s_values_from_one_engine_call(engine, gold, name, monkeypatch):
  kind, nu = KERNELS[name]
  case = _gold_case(gold)
  gp = _mirror_gp(kind, nu, case, case['bw'])
  spy = _Spy(monkeypatch, gp.device_gp, ['lml_grad'])
  got = [gp.compute_grad_log_marginal_likelihood('scale')]
  got += [gp.compute_grad_log_marginal_likelihood('dim_bandwidths', c) for c in range(3)]
  got += [gp.compute_grad_log_marginal_likelihood('noise_var'), gp.compute_grad_log_marginal_likelihood('noise_mean')]
  assert spy.count == {'lml_grad': 1}
  print(name, 'mirror against the reference', relerr(got, gold[name + '_grad']))
  assert relerr(got, gold[name + '_grad']) <= TOL
  # new data: the cached gradient goes with the posterior
  gp.add_data_single(np.array([0.3, 0.4, 0.5]), 0.1)
  assert gp.compute_grad_log_marginal_likelihood('scale') != got[0]
  # one bandwidth for every dimension
  same = _mirror_gp(kind, nu, _gold_case(gold, same=True), float(gold['same_bw']))
  value = same.compute_grad_log_marginal_likelihood('same_dim_bandwidths')
  print(name, 'same_dim_bandwidths', value, gold[name + '_same_grad'])
  assert relerr([value], [gold[name + '_same_grad']]) <= TOL


def test_mirror_gp_says_what_it_cannot_differentiate(engine, gold):
  from dragonfly_amd import kernel as K
  from dragonfly_amd.euclidean_gp import EuclideanGP
  from dragonfly_amd.gp_core import ConstantMean, GP
  case = _gold_case(gold)
  poly = EuclideanGP(case['X'], case['y'], K.PolyKernel(3, 2, 1.0, [1.0, 1.0, 1.0]), ConstantMean(0.0), 1e-2)
  with pytest.raises(NotImplementedError, match='POLY'):
    poly.compute_grad_log_marginal_likelihood('scale')
  host = GP(case['X'], case['y'], K.SEKernel(3, 1.0, case['bw']), ConstantMean(0.0), 1e-2, handle_non_psd_kernels='project_first')
  with pytest.raises(NotImplementedError, match='host'):
    host.compute_grad_log_marginal_likelihood('scale')
