"""The ESP kernel's host side, without a GPU: the mirrors of ESPKernel / ESPKernelSE / ESPKernelMatern
(dragonfly/gp/kernel.py:671-744), their device description (DFH_KERNEL_ESP), the fitter's set-up and the kernel factory
(dragonfly/gp/euclidean_gp.py:244-300, 777-900) against the real reference where it is present, and install()."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference():
  try:
    from oracle.make_golden import REF, import_reference
  except ImportError:
    return None
  if not os.path.isdir(os.path.join(REF, 'dragonfly')):
    return None
  try:
    return import_reference()
  except Exception:       # pylint: disable=broad-except
    return None


def test_header_and_binding_agree():
  from dragonfly_amd import _lib
  text = open(os.path.join(ROOT, 'include', 'dfhip.h')).read()
  assert int(re.search(r'^#define\s+DFH_KERNEL_ESP\s+(\d+)', text, flags=re.M).group(1)) == _lib.KERNEL_ESP == 6
  assert int(re.search(r'^#define\s+DFH_ABI_VERSION\s+(\d+)', text, flags=re.M).group(1)) == 2


def test_constructors_attributes_and_validation():
  from dragonfly_amd import kernel as K
  kern = K.ESPKernelSE(4, 2.0, 3, np.array([0.5, 1.0, 1.5, 2.0]))
  assert kern.dim == 4 and len(kern.kernel_list) == 4
  assert set(kern.hyperparams) == {'scale', 'order'} and kern.hyperparams['order'] == 3
  assert all(isinstance(k, K.SEKernel) and k.dim == 1 and k.hyperparams['scale'] == 1.0 for k in kern.kernel_list)
  assert [float(np.ravel(k.hyperparams['dim_bandwidths'])[0]) for k in kern.kernel_list] == [0.5, 1.0, 1.5, 2.0]
  assert kern.is_guaranteed_psd()
  mat = K.ESPKernelMatern(3, [0.5, 1.5, 2.5], 1.0, 2, [1.0, 1.0, 1.0])
  assert [k.hyperparams['nu'] for k in mat.kernel_list] == [0.5, 1.5, 2.5]
  with pytest.raises(ValueError, match='order must be less than or equal to dim'):
    K.ESPKernelSE(3, 1.0, 4, [1.0] * 3)
  with pytest.raises(ValueError, match='order must be an integer between 1 and dim'):
    K.ESPKernelSE(3, 1.0, 0, [1.0] * 3)

  class _NotPSD(K.SEKernel):
    def is_guaranteed_psd(self):
      return False
  assert not K.ESPKernel(1.0, 1, [K.SEKernel(1, 1.0, 1.0), _NotPSD(1, 1.0, 1.0)]).is_guaranteed_psd()


def test_to_spec_descriptor():
  from dragonfly_amd import _lib, kernel as K
  kern = K.ESPKernelMatern(3, [0.5, 1.5, 2.5], 1.7, 2, [0.3, 0.4, 0.5])
  assert kern.has_device_spec()
  desc = kern.to_spec(3).to_desc()
  assert desc.kind == _lib.KERNEL_ESP and desc.dim == 3 and desc.scale == 1.7 and desc.nu == 2.0
  assert desc.n_groups == 3
  assert [desc.group_off[i] for i in range(4)] == [0, 1, 2, 3]
  assert [desc.group_dims[i] for i in range(3)] == [0, 1, 2]
  assert [desc.sub_kind[i] for i in range(3)] == [_lib.KERNEL_MATERN] * 3
  assert [desc.sub_nu[i] for i in range(3)] == [0.5, 1.5, 2.5]
  assert [desc.sub_bw[i] for i in range(3)] == [0.3, 0.4, 0.5]
  assert [desc.sub_scale[i] for i in range(3)] == [1.0] * 3
  assert not desc.group_factor and not desc.factor_is_sum and not desc.factor_scale
  # orders above the device's register bucket stay in host-kernel mode
  assert not K.ESPKernelSE(40, 1.0, 33, [1.0] * 40).has_device_spec()
  assert K.ESPKernelSE(40, 1.0, 32, [1.0] * 40).has_device_spec()


def test_host_formula_is_the_reference_recursion():
  """ _host_compose (host-kernel mode) on a kernel list of plain NumPy 1-D kernels equals the textbook elementary
      symmetric polynomial for a small case """
  from dragonfly_amd import kernel as K

  class _Const(object):
    def __init__(self, v):
      self.v = v

    def __call__(self, X1, X2):
      return self.v * np.ones((len(X1), len(X2)))

    def is_guaranteed_psd(self):
      return True
  vals = [0.3, 0.7, 0.2, 0.9]
  kern = K.ESPKernel(2.0, 2, [_Const(v) for v in vals])
  assert not kern.has_device_spec()
  got = kern(np.zeros((2, 4)), np.zeros((3, 4)))
  want = 2.0 * sum(vals[a] * vals[b] for a in range(4) for b in range(a + 1, 4))
  assert np.allclose(got, want, rtol=1e-14)


def test_euclidean_gp_kernel_from_type_and_str():
  from dragonfly_amd import kernel as K
  from dragonfly_amd.euclidean_gp import EuclideanGP
  kern = EuclideanGP._get_kernel_from_type('esp', {'dim': 3, 'scale': 1.5, 'order': 2, 'dim_bandwidths': [1, 2, 3]})
  assert isinstance(kern, K.ESPKernelSE) and kern.hyperparams == {'scale': 1.5, 'order': 2}
  assert EuclideanGP._get_kernel_str(kern) == ''


OPTION_SETS = [
  dict(kernel_type='esp', esp_kernel_type='se', esp_order=-1),
  dict(kernel_type='esp', esp_kernel_type='se', esp_order=2),
  dict(kernel_type='esp', esp_kernel_type='matern', esp_order=-1),
  dict(kernel_type='esp', esp_kernel_type='matern', esp_order=3, esp_matern_nu=1.5),
  dict(kernel_type='esp', esp_kernel_type='matern', esp_order=-1, use_same_bandwidth=True),
  dict(kernel_type='esp', esp_kernel_type='se', esp_order=-1, use_additive_gp=True),
]


@pytest.mark.parametrize('opts', OPTION_SETS)
def test_fitter_set_up_and_factory_match_reference(opts):
  ref = _reference()
  if ref is None:
    pytest.skip('the reference Dragonfly is not present')
  from argparse import Namespace
  from dragonfly.gp import euclidean_gp as ref_egp
  from dragonfly.utils.option_handler import load_options
  from dragonfly_amd import euclidean_gp as our_egp
  rs = np.random.RandomState(7)
  X = [x for x in rs.rand(25, 4)]
  Y = list(np.sin(np.sum(X, axis=1)))
  ref_opts = load_options(ref_egp.euclidean_gp_args, partial_options=Namespace(**opts))
  ref_fit = ref_egp.EuclideanGPFitter(X, Y, ref_opts)
  ours = our_egp.EuclideanGPFitter(X, Y, dict(opts))
  assert np.allclose(np.array(ours.cts_hp_bounds), np.array(ref_fit.cts_hp_bounds), rtol=0, atol=0)
  assert ours.dscr_hp_vals == ref_fit.dscr_hp_vals
  assert ours.param_order == ref_fit.param_order
  # the factory decodes the same candidate vectors to the same kernel
  for trial in range(4):
    cts = [rs.uniform(lo, hi) for lo, hi in ref_fit.cts_hp_bounds]
    dscr = [vals[rs.randint(len(vals))] for vals in ref_fit.dscr_hp_vals]
    mean_noise = len(ref_fit.cts_hp_bounds) - 1 - 4      # mean / noise entries in front of scale + 4 bandwidths
    kh_ref = ref_egp.prep_euclidean_integral_kernel_hyperparams('esp', ref_opts, 4)
    kh_our = our_egp.prep_euclidean_integral_kernel_hyperparams('esp', ours.options, 4)
    assert kh_ref == kh_our
    rk, rc, rd = ref_egp.get_euclidean_integral_gp_kernel('esp', kh_ref, cts[mean_noise:], list(dscr),
                                                          ref_opts.use_same_bandwidth, None, ref_opts.esp_kernel_type)
    ok, oc, od = our_egp.get_euclidean_integral_gp_kernel('esp', kh_our, cts[mean_noise:], list(dscr),
                                                          ours.options.use_same_bandwidth, None,
                                                          ours.options.esp_kernel_type)
    assert type(rk).__name__ == type(ok).__name__, trial
    assert list(rc) == list(oc) and list(rd) == list(od)
    assert rk.hyperparams['scale'] == ok.hyperparams['scale'] and int(rk.hyperparams['order']) == ok.hyperparams['order']
    for a, b in zip(rk.kernel_list, ok.kernel_list):
      assert np.array_equal(np.ravel(a.hyperparams['dim_bandwidths']), np.ravel(b.hyperparams['dim_bandwidths']))
      assert a.hyperparams.get('nu') == b.hyperparams.get('nu')


def test_install_rebinds_and_restores_esp_kernels():
  ref = _reference()
  if ref is None:
    pytest.skip('the reference Dragonfly is not present')
  import dragonfly.gp.kernel as ref_kernel
  from dragonfly_amd import install, kernel as ours
  before = (ref_kernel.ESPKernelSE, ref_kernel.ESPKernelMatern)
  try:
    install.install()
    assert ref_kernel.ESPKernelSE is ours.ESPKernelSE and ref_kernel.ESPKernelMatern is ours.ESPKernelMatern
  finally:
    install.uninstall()
  assert (ref_kernel.ESPKernelSE, ref_kernel.ESPKernelMatern) == before
