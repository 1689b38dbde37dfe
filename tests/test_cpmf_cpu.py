"""CPU: multi-fidelity GPs on Cartesian-product domains above the C-ABI, on the engine's CPU stand-in
(tests/oracle_engine_cpmf.py):
 - the nested CartesianProductKernel mirror -- a part that is itself a product -- gives ONE product descriptor with
   factor_sums == 2 and the inner kernels' scales, packs (z, x) pairs side by side, and declines a third level or a
   member the device does not know;
 - the descriptor's value in the reference's order IS the reference's CPMFGP training and cross matrix, bit for bit
   (tests/golden/cpmf_A_n70.npz, cpmf_B_n70.npz, recorded from the unmodified reference);
 - with the real reference present (skipped otherwise, like tests/test_cp_fitter_cpu.py): install(cp_multi_fidelity=True)
   needs its two companions, rebinds CPMFGP and the bandit's CPMFGPFitter and uninstall() restores them; the reference's
   CPMFGPFitter chooses the same hyper-parameters installed; its CPGPBandit(is_mf=True) asks for the same
   (fidelity, point) sequence with BOCA's step fused, one engine call per step; the class pickles."""
import os
import pickle
from argparse import Namespace

import numpy as np
import pytest

from conftest import load_golden, relerr

import cpmf_cases as cases

REF = os.environ.get('DRAGONFLY_REFERENCE', '/root/reference')
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'dragonfly')), reason='the reference checkout is not present')
FLAGS = dict(multi_fidelity=True, cartesian_product=True, cp_multi_fidelity=True)


def _reference():
  from oracle.make_golden import import_reference
  import_reference()


def _nested(name, g):
  from dragonfly_amd import kernel as K
  fidel, domain = cases.mirror_kernels(name, g)
  return K.CartesianProductKernel(float(g['kernel_scale']), [fidel, domain])


def test_to_spec_and_pack_of_the_nested_mirror(monkeypatch):
  from oracle_engine_cpmf import patch_engine_cpmf
  patch_engine_cpmf(monkeypatch)
  g = load_golden('cpmf_A_n70')
  kern = _nested('A', g)
  assert kern.has_device_spec() and kern.is_guaranteed_psd()
  assert kern.part_offsets() == ([0, 3], 16)
  spec = kern.to_spec()
  assert spec.kind == 'product' and spec.dim == 16 and spec.scale == float(g['kernel_scale'])
  assert spec.groups == [[0], [1, 2], [3, 4, 5], [6], list(range(7, 16))]
  assert list(spec.sub_kinds) == ['se', 'hamming', 'matern', 'se', 'hamming'] and list(spec.sub_nus) == [0.0, 0.0, 2.5, 0.0, 0.0]
  assert list(spec.group_factors) == [0, 0, 1, 1, 1] and list(spec.factor_sums) == [2, 2]
  assert list(spec.factor_scales) == [float(g['fidel_scale']), float(g['domain_scale'])]
  assert spec.signature() == cases.spec_of('A', g).signature()
  # a pair's parts side by side, the categories coded by first appearance in each column
  pairs = cases.unpack_pairs('A', g['Xp'][:9])
  P = kern.pack(pairs)
  assert P.shape == (9, 16) and np.array_equal(P, kern.pack_many(pairs))
  euclid = [0, 3, 4, 5, 6]
  assert np.array_equal(P[:, euclid], g['Xp'][:9][:, euclid])
  for c in set(range(16)) - set(euclid):                       # same partition of the rows, whatever the code values
    assert np.array_equal(P[:, c][:, None] == P[:, c][None, :], g['Xp'][:9, c][:, None] == g['Xp'][:9, c][None, :])
  # a plain part beside a product factor: value 0 describes it
  from dragonfly_amd import kernel as K
  mixed = K.CartesianProductKernel(2.0, [K.SEKernel(1, 1.0, [0.5]), cases.mirror_kernels('B', load_golden('cpmf_B_n70'))[1]])
  ms = mixed.to_spec()
  assert list(ms.factor_sums) == [0, 2] and list(ms.group_factors) == [0, 1] and list(ms.factor_scales) == [1.0, 1.0]
  # the descriptor travels to the C struct with the value 2
  desc = spec.to_desc()
  assert [desc.factor_is_sum[i] for i in range(2)] == [2, 2] and [desc.group_factor[i] for i in range(5)] == [0, 0, 1, 1, 1]


def test_a_third_level_or_an_unknown_member_has_no_device_spec(monkeypatch):
  from oracle_engine_cpmf import patch_engine_cpmf
  from dragonfly_amd import kernel as K
  patch_engine_cpmf(monkeypatch)
  g = load_golden('cpmf_B_n70')
  fidel, domain = cases.mirror_kernels('B', g)
  third = K.CartesianProductKernel(1.0, [K.CartesianProductKernel(1.0, [fidel]), domain])
  assert not third.has_device_spec()
  with pytest.raises(TypeError):
    third.to_spec()

  class PolyKernel(K.Kernel):
    def __init__(self):
      super(PolyKernel, self).__init__()
      self.dim = 2
      self.add_hyperparams(order=2, scale=1.0, dim_scalings=np.array([1.0, 2.0]))

    def is_guaranteed_psd(self):
      return True
  poly = K.CartesianProductKernel(1.0, [fidel, K.CartesianProductKernel(1.0, [PolyKernel()])])
  assert not poly.has_device_spec()
  empty = K.CartesianProductKernel(1.0, [fidel, K.CartesianProductKernel(1.0, [])])
  assert not empty.has_device_spec()
  assert K.CartesianProductKernel(1.0, [fidel, domain]).has_device_spec()


@pytest.mark.parametrize('name', ['A', 'B'])
def test_host_order_value_is_the_reference_cpmfgp_matrix_bit_for_bit(name):
  from oracle_engine_cpmf import nested_product_matrix
  g = load_golden('cpmf_%s_n70' % name)
  spec = cases.spec_of(name, g)
  assert np.array_equal(nested_product_matrix(spec, g['Xp']), g['K'])
  assert np.array_equal(nested_product_matrix(spec, g['Tp'], g['Xp']), g['K_cross'])
  assert g['K'].shape == (70, 70) and g['K_cross'].shape == (37, 70)


@pytest.mark.parametrize('name', ['A', 'B'])
def test_device_class_runs_from_the_descriptor(name, monkeypatch):
  """ the class device_cpmfgp_class makes, here over a stand-in for the reference module: the descriptor route, the
      reference's Gram matrix bit for bit, its posterior and log marginal likelihood; distance lists put it in
      host-kernel mode """
  from oracle_engine_cpmf import patch_engine_cpmf
  patch_engine_cpmf(monkeypatch)
  if not os.path.isdir(os.path.join(REF, 'dragonfly')):
    pytest.skip('the reference checkout is not present')
  _reference()
  import dragonfly.gp.cartesian_product_gp as ref_cpgp
  from dragonfly_amd import cartesian_product_gp as our_cpgp
  g = load_golden('cpmf_%s_n70' % name)
  cls = our_cpgp.device_cpmfgp_class(ref_cpgp)
  assert cls is our_cpgp.device_cpmfgp_class(ref_cpgp) and cls is our_cpgp.CPMFGP and ref_cpgp.CPMFGP is not cls
  fidel, domain = cases.mirror_kernels(name, g)
  w = cases.fidel_width(name)
  ZZ, XX = cases.unpack(name, g['Xp'][:, :w], 'fidel'), cases.unpack(name, g['Xp'][:, w:], 'domain')
  mean_c = float(g['mean_const'])
  gp = cls(ZZ, XX, list(g['Y']), None, lambda x: np.array([mean_c] * len(x)), float(g['noise']), float(g['kernel_scale']),
           fidel, domain, [None] * len(fidel.kernel_list), [None] * len(domain.kernel_list))
  assert not gp._generic and gp.handle_non_psd_kernels == 'project_first'      # pylint: disable=protected-access
  assert gp.kernel.kernel_list == [fidel, domain] and our_cpgp.is_device_cpmfgp(gp)
  assert np.array_equal(gp.K_trtr_wo_noise, g['K'])
  assert relerr(gp.compute_log_marginal_likelihood(), g['lml']) <= 1e-10 and relerr(gp.alpha, g['alpha']) <= 1e-9
  m = 40
  cands = cases.unpack(name, g['Cp'][:m], 'domain')
  f2o = cases.unpack(name, g['f2o'], 'fidel')[0]
  mu, sd = gp.eval_at_fidel([f2o] * m, cands, uncert_form='std')
  assert relerr(mu, g['mu_q0'][:m]) <= 1e-9 and relerr(sd, g['sd_q0'][:m]) <= 1e-9
  # it pickles by the published name, data and kernel with it
  assert pickle.loads(pickle.dumps(cls)) is cls
  plain = cls(ZZ, XX, list(g['Y']), None, None, float(g['noise']), float(g['kernel_scale']), fidel, domain,
              [None] * len(fidel.kernel_list), [None] * len(domain.kernel_list), build_posterior=False)
  clone = pickle.loads(pickle.dumps(plain))
  assert type(clone) is cls and clone.num_tr_data == 70 and clone.kernel.to_spec().signature() == gp.kernel.to_spec().signature()
  assert clone.kernel.kernel_list[0] is clone.fidel_space_kernel and not clone._generic      # pylint: disable=protected-access
  # distance lists: the reference's hook evaluates the kernel
  gp.set_domain_lists_of_dists([np.zeros((70, 70))] + [None] * (len(domain.kernel_list) - 1))
  assert gp._generic                                                        # pylint: disable=protected-access


@needs_reference
def test_install_flag_needs_its_companions_and_uninstall_restores():
  _reference()
  import dragonfly.gp.cartesian_product_gp as ref_cpgp
  import dragonfly.opt.gp_bandit as ref_gp_bandit
  from dragonfly_amd import install
  for flags in (dict(), dict(cartesian_product=True), dict(multi_fidelity=True)):
    with pytest.raises(ValueError):
      install.install(cp_multi_fidelity=True, **flags)
    assert install._saved == []                                # pylint: disable=protected-access
  before = (ref_cpgp.CPMFGP, ref_gp_bandit.CPMFGPFitter)
  plain = install.install(multi_fidelity=True, cartesian_product=True)
  try:
    assert (ref_cpgp.CPMFGP, ref_gp_bandit.CPMFGPFitter) == before and not any('CPMFGP' in p for p in plain)
  finally:
    install.uninstall()
  patched = install.install(**FLAGS)
  try:
    assert 'dragonfly.gp.cartesian_product_gp.CPMFGP' in patched and 'dragonfly.opt.gp_bandit.CPMFGPFitter' in patched
    assert set(patched) - set(plain) == {'dragonfly.gp.cartesian_product_gp.CPMFGP', 'dragonfly.opt.gp_bandit.CPMFGPFitter'}
    assert ref_cpgp.CPMFGP is not before[0] and issubclass(ref_gp_bandit.CPMFGPFitter, before[1])
    assert ref_cpgp.CPMFGP.__module__ == 'dragonfly_amd.cartesian_product_gp'
  finally:
    install.uninstall()
  assert (ref_cpgp.CPMFGP, ref_gp_bandit.CPMFGPFitter) == before
  unbatched = install.install(batched_tuning=False, **FLAGS)
  try:
    assert 'dragonfly.opt.gp_bandit.CPMFGPFitter' not in unbatched and ref_gp_bandit.CPMFGPFitter is before[1]
  finally:
    install.uninstall()


def _fit(seed=3):
  """ the reference's CPMFGPFitter (by the name the bandit constructs it by) on 30 pairs of cases.CONFIG's spaces """
  from dragonfly import load_config
  from dragonfly.exd.exd_utils import sample_from_cp_domain
  import dragonfly.opt.gp_bandit as ref_gp_bandit
  config = load_config(cases.CONFIG)
  np.random.seed(seed)
  ZZ = sample_from_cp_domain(config.fidel_space, 30)
  XX = sample_from_cp_domain(config.domain, 30)
  YY = [float(np.sum(np.asarray(x[0], dtype=float) ** 2) - 0.1 * float(np.ravel(x[1])[0]) + 0.3 * float(np.ravel(z[0])[0])
              + 0.2 * (x[-1][0] == 'a')) for z, x in zip(ZZ, XX)]
  options = Namespace(ml_hp_tune_opt='rand', hp_tune_max_evals=40, hp_tune_criterion='ml')
  fitter = ref_gp_bandit.CPMFGPFitter(ZZ, XX, YY, config=config, options=options)
  _, gp, _ = fitter.fit_gp()
  return gp


@needs_reference
def test_fitter_chooses_the_reference_hyper_parameters(monkeypatch):
  _reference()
  from oracle_engine_cpmf import patch_engine_cpmf
  from dragonfly_amd import install, kernel as K
  want = _fit()
  eng = patch_engine_cpmf(monkeypatch)
  eng.lml_batch_sizes = []
  install.install(**FLAGS)
  try:
    got = _fit()
    assert isinstance(got.kernel, K.CartesianProductKernel) and got.kernel.has_device_spec() and not got._generic   # pylint: disable=protected-access
    assert all(isinstance(part, K.CartesianProductKernel) for part in got.kernel.kernel_list)
  finally:
    install.uninstall()
  assert len(eng.lml_batch_sizes) >= 1 and max(eng.lml_batch_sizes) > 1        # the tuner saw a batch objective
  assert got.noise_var == want.noise_var and float(got.mean_func([got.X[0]])[0]) == float(want.mean_func([want.X[0]])[0])
  assert got.kernel.hyperparams['scale'] == want.kernel.hyperparams['scale']
  for ours, theirs in zip(got.kernel.kernel_list, want.kernel.kernel_list):
    for a, b in zip(ours.kernel_list, theirs.kernel_list):
      for key in b.hyperparams:
        assert np.array_equal(np.asarray(a.hyperparams[key]), np.asarray(b.hyperparams[key])), key


_WANT = {}


@needs_reference
@pytest.mark.parametrize('acq', ['ucb', 'ei', 'ts'])
def test_mf_bandit_asks_for_the_same_fidelities_and_points_installed(acq, monkeypatch):
  _reference()
  from oracle_engine_cpmf import patch_engine_cpmf
  from dragonfly_amd import install
  if acq not in _WANT:
    _WANT[acq] = cases.run_mf_bandit(acq)
  want = _WANT[acq]
  assert len(want[2]) == len(want[3]) >= 12
  eng = patch_engine_cpmf(monkeypatch)
  install.install(boca=True, cp_acquisitions=True, **FLAGS)
  try:
    got = cases.run_mf_bandit(acq)
  finally:
    install.uninstall()
  assert got == want
  calls = eng.calls
  fused = 'thompson_pointwise' if acq == 'ts' else 'acq_argmax'
  print(acq, calls)
  # every model-based step: the candidates joined once, ONE fused call for the point, one posterior call for the fidelity
  assert calls.get(fused, 0) >= 5 and calls.get('join_fixed', 0) == calls[fused] == calls.get('predict', 0)
  assert 'thompson' not in calls and 'predict_covar' not in calls
  # without the two BOCA flags the same run keeps the reference's per-point stream on the device posterior
  eng.calls.clear()
  install.install(**FLAGS)
  try:
    assert cases.run_mf_bandit(acq) == want
  finally:
    install.uninstall()
  assert fused not in eng.calls and 'join_fixed' not in eng.calls and sum(eng.calls.values()) > 60 * 5
