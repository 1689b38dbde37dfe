"""The Hamming / Cartesian-product kernels' host side, without a GPU: the mirrors of HammingKernel and
CartesianProductKernel (dragonfly/gp/kernel.py:436-457, 504-538), the packing of list-of-lists points with category
codes, their device description (DFH_KERNEL_HAMMING inside DFH_KERNEL_PRODUCT) and the CP GP class, against the real
reference's outputs (tests/golden/cp_*.npz, tools/make_cp_golden.py) on the CPU stand-in engine."""
import copy
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest

from conftest import load_golden, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
  spec = importlib.util.spec_from_file_location('make_cp_golden', os.path.join(ROOT, 'tools', 'make_cp_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


G = _gen()


def test_header_and_binding_agree():
  from dragonfly_amd import _lib
  text = open(os.path.join(ROOT, 'include', 'dfhip.h')).read()
  assert int(re.search(r'^#define\s+DFH_KERNEL_HAMMING\s+(\d+)', text, flags=re.M).group(1)) == _lib.KERNEL_HAMMING == 7
  assert int(re.search(r'^#define\s+DFH_ABI_VERSION\s+(\d+)', text, flags=re.M).group(1)) == 2


def test_hamming_constructor_and_spec(monkeypatch):
  from dragonfly_amd import kernel as K
  from oracle_engine_cp import patch_engine_cp
  patch_engine_cp(monkeypatch)
  kern = K.HammingKernel(4)
  assert np.array_equal(kern.hyperparams['dim_weights'], np.ones(4) / 4.0) and kern.is_guaranteed_psd()
  kern = K.HammingKernel([0.5, 0.25, 0.25])
  assert str(kern) == 'Hamming: wts=[0.500 0.250 0.250]'
  spec = kern.to_spec()
  assert spec.kind == 'hamming' and spec.dim == 3 and spec.scale == 1.0 and spec.nu == 0.0
  assert np.array_equal(spec.bandwidths, [0.5, 0.25, 0.25])
  desc = spec.to_desc()
  assert desc.kind == 7 and desc.dim == 3 and desc.n_groups == 0
  assert not K.HammingKernel(33).has_device_spec() and K.HammingKernel(32).has_device_spec()


def test_codes_follow_the_reference_equality():
  """ the reference compares the items of np.array(X, dtype=object) with np.equal, i.e. with their own ==:
      1 == 1.0 (also beside strings), 1 != '1'; an np.str_ out of a string-coerced array equals the str """
  from dragonfly_amd import kernel as K
  coder = K.CategoryCoder()
  codes = coder.encode([[1, 'a'], [1.0, 'b'], [2, 'a'], [True, np.str_('b')]])
  assert codes[:, 0].tolist() == [0.0, 0.0, 1.0, 0.0] and codes[:, 1].tolist() == [0.0, 1.0, 0.0, 1.0]
  mixed = K.CategoryCoder().encode([[1], ['1'], [1.0], ['b']])
  assert mixed[:, 0].tolist() == [0.0, 1.0, 0.0, 2.0]
  coerced = np.array([[1, 'b'], ['1', 'c']])            # NumPy makes strings of both columns
  both = K.CategoryCoder().encode(list(coerced) + [['1', 'b']])
  assert both[:, 0].tolist() == [0.0, 0.0, 0.0] and both[:, 1].tolist() == [0.0, 1.0, 0.0]
  # later calls share the dictionary: a new category gets the next code, old ones keep theirs
  assert coder.encode([[2, 'zz'], [1, 'a']]).tolist() == [[1.0, 2.0], [0.0, 0.0]]
  with pytest.raises(ValueError):
    coder.encode([[float('nan'), 'a']])
  with pytest.raises(ValueError):
    coder.encode([[[1, 2], 'a']])


def test_an_engine_object_of_the_earlier_interface_keeps_host_kernel_mode(monkeypatch):
  """ without 'hamming' among the engine's kernel_kinds the Hamming part is composed on the host from the codes """
  from dragonfly_amd import kernel as K
  from oracle_engine import patch_engine
  from oracle_engine_cp import hamming_matrix
  patch_engine(monkeypatch)
  kern = K.HammingKernel([0.5, 0.3, 0.2])
  cp = K.CartesianProductKernel(1.0, [K.SEKernel(1, 1.0, [0.5]), kern])
  assert not kern.has_device_spec() and not cp.has_device_spec()
  X1, X2 = G.hamming_points(['str', 'int', 'mixnum'], 9, 1), G.hamming_points(['str', 'int', 'mixnum'], 5, 2)
  A, B = kern.pack(X1), kern.pack(X2)
  assert np.array_equal(kern(X1, X2), hamming_matrix([0.5, 0.3, 0.2], A, B))
  assert np.array_equal(kern(X2, X1), hamming_matrix([0.5, 0.3, 0.2], B, A))


@pytest.mark.parametrize('idx', range(len(G.HAMMING_CASES)))
def test_hamming_packing_reproduces_the_fixture(idx):
  """ the codes of the packed points, compared as doubles in NumPy's order, give the reference's matrices: bit for
      bit (the terms are w or 0; the same order) """
  from dragonfly_amd import kernel as K
  from oracle_engine_cp import hamming_matrix
  name, dim, weights, cats, n1, n2 = G.HAMMING_CASES[idx]
  gold = load_golden('cp_' + name)
  kern = K.HammingKernel(G.hamming_weights(weights, dim))
  assert np.array_equal(kern.hyperparams['dim_weights'], gold['weights'])
  A = kern.pack(G.hamming_points(cats, n1, 100 + idx))
  B = kern.pack(G.hamming_points(cats, n2, 200 + idx, unseen=True))
  assert np.array_equal(hamming_matrix(gold['weights'], A, A), gold['K11'])
  assert np.array_equal(hamming_matrix(gold['weights'], A, B), gold['K12'])
  assert np.array_equal(hamming_matrix(gold['weights'], B, A), gold['K21'])


@pytest.mark.parametrize('idx', range(len(G.CP_CASES)))
def test_cp_mirror_on_the_stand_in_engine_reproduces_the_fixture(idx, monkeypatch):
  from dragonfly_amd import kernel as K
  from oracle_engine_cp import patch_engine_cp
  patch_engine_cp(monkeypatch)
  name, parts, n1, n2 = G.CP_CASES[idx]
  gold = load_golden(name)
  scale, pars = G.cp_hyperparams(parts, 500 + idx)
  kern = G.build_cp_kernel(K, parts, scale, pars)
  assert kern.has_device_spec() and kern.is_guaranteed_psd()
  X1, X2 = G.cp_points(parts, n1, 300 + idx), G.cp_points(parts, n2, 400 + idx, unseen=True)
  for got, key in ((kern(X1, X1), 'K11'), (kern(X1, X2), 'K12'), (kern(X2, X1), 'K21')):
    assert relerr(got, gold[key]) <= 1e-13, (name, key)


def test_to_spec_lays_the_parts_side_by_side(monkeypatch):
  from dragonfly_amd import kernel as K
  from oracle_engine_cp import patch_engine_cp
  patch_engine_cp(monkeypatch)
  kern = K.CartesianProductKernel(1.5, [K.MaternKernel(2, 2.5, 1.0, [0.3, 0.4]), K.SEKernel(2, 1.0, [2.0, 3.0]),
                                        K.HammingKernel([0.6, 0.4])])
  spec = kern.to_spec()
  assert spec.kind == 'product' and spec.dim == 6 and spec.scale == 1.5
  assert spec.groups == [[0, 1], [2, 3], [4, 5]] and spec.sub_kinds == ['matern', 'se', 'hamming']
  assert list(spec.sub_scales) == [1.0, 1.0, 1.0] and list(spec.sub_nus) == [2.5, 0.0, 0.0]
  assert [list(b) for b in spec.sub_bandwidths] == [[0.3, 0.4], [2.0, 3.0], [0.6, 0.4]]
  desc = spec.to_desc()
  assert desc.kind == 3 and desc.n_groups == 3 and [desc.sub_kind[g] for g in range(3)] == [1, 0, 7]
  packed = kern.pack([[[0.1, 0.2], [3, 4], ['a', 7]], [[0.5, 0.6], [1, 2], ['b', 7]]])
  assert packed.tolist() == [[0.1, 0.2, 3.0, 4.0, 0.0, 0.0], [0.5, 0.6, 1.0, 2.0, 1.0, 0.0]]
  assert str(kern).startswith('DomProd scale=1.50, Matern: nu=2.5')


class _OtherKernel(object):
  """ a part the device does not know: any object with the Kernel interface """
  hyperparams = {}
  dim = 1

  def is_guaranteed_psd(self):
    return True

  def __call__(self, X1, X2=None):
    X2 = X1 if X2 is None else X2
    return np.array([[1.0 / (1.0 + abs(a[0] - b[0])) for b in X2] for a in X1])


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


needs_reference = pytest.mark.skipif(_reference() is None, reason='the reference checkout is not present')


def _cp_gp_class():
  """ the class install(cartesian_product=True) makes, over the real reference module """
  from dragonfly_amd.cartesian_product_gp import device_cpgp_class
  import dragonfly.gp.cartesian_product_gp as mod
  return device_cpgp_class(mod), mod


@needs_reference
def test_host_kernel_mode_with_an_undescribed_part_or_distance_lists(monkeypatch):
  from dragonfly_amd import kernel as K
  from oracle_engine_cp import patch_engine_cp
  patch_engine_cp(monkeypatch)
  cls, _ = _cp_gp_class()
  X = [[[0.1 * i], ['a' if i % 2 else 'b']] for i in range(8)]
  Y = [float(i % 3) for i in range(8)]
  mean = lambda x: np.zeros(len(x))
  described = K.CartesianProductKernel(1.0, [K.SEKernel(1, 1.0, [0.5]), K.HammingKernel([1.0])])
  other = K.CartesianProductKernel(1.0, [_OtherKernel(), K.HammingKernel([1.0])])
  assert described.has_device_spec() and not other.has_device_spec()
  assert not cls(X, Y, described, mean, 0.1)._generic
  assert cls(X, Y, other, mean, 0.1)._generic
  assert cls(X, Y, described, mean, 0.1, domain_lists_of_dists=[None, None], build_posterior=False)._generic is False
  gp = cls(X, Y, described, mean, 0.1, build_posterior=False)
  gp.domain_lists_of_dists = [np.zeros((8, 8)), None]
  assert gp._generic
  # the two modes agree: the described kernel from the descriptor, and composed on the host
  a = cls(X, Y, described, mean, 0.1)
  ref_K = described._host_compose(X, X)
  assert relerr(a.K_trtr_wo_noise, ref_K) <= 1e-13
  b = cls(X, Y, other, mean, 0.1)
  assert relerr(b.K_trtr_wo_noise, other._host_compose(X, X)) <= 1e-15


@needs_reference
def test_codes_are_stable_across_add_data_multiple(monkeypatch):
  from dragonfly_amd import kernel as K
  from oracle_engine_cp import patch_engine_cp
  patch_engine_cp(monkeypatch)
  cls, _ = _cp_gp_class()
  kern = K.CartesianProductKernel(1.0, [K.SEKernel(1, 1.0, [0.5]), K.HammingKernel([0.7, 0.3])])
  X = [[[0.1 * i], ['a' if i % 2 else 'b', i % 3]] for i in range(9)]
  Y = [np.sin(i) for i in range(9)]
  gp = cls(X[:6], Y[:6], kern, lambda x: np.zeros(len(x)), 0.05)
  first = dict(kern.kernel_list[1].coder.columns[0])
  gp.add_data_multiple([[[0.95], ['c', 7]]] + X[6:], [0.3] + Y[6:])
  assert all(kern.kernel_list[1].coder.columns[0][k] == v for k, v in first.items())
  assert kern.kernel_list[1].coder.columns[0]['c'] == 2
  fresh = cls(X[:6] + [[[0.95], ['c', 7]]] + X[6:], Y[:6] + [0.3] + Y[6:],
              K.CartesianProductKernel(1.0, [K.SEKernel(1, 1.0, [0.5]), K.HammingKernel([0.7, 0.3])]),
              lambda x: np.zeros(len(x)), 0.05)
  assert relerr(gp.alpha, fresh.alpha) <= 1e-12 and relerr(gp.L, fresh.L) <= 1e-12


@needs_reference
@pytest.mark.parametrize('idx', range(len(G.GP_CASES)))
def test_cp_gp_from_the_descriptor_reproduces_the_fixture(idx, monkeypatch):
  """ project_first travels to the fit as a flag; L, alpha, lml, mean and sd are the reference's """
  from dragonfly_amd import kernel as K
  from oracle_engine_cp import patch_engine_cp
  patch_engine_cp(monkeypatch)
  cls, _ = _cp_gp_class()
  name, parts, n, m = G.GP_CASES[idx]
  gold = load_golden(name)
  scale, pars = G.cp_hyperparams(parts, 1000 + idx)
  kern = G.build_cp_kernel(K, parts, scale, pars)
  X, Xt = G.cp_points(parts, n, 600 + idx), G.cp_points(parts, m, 700 + idx, unseen=True)
  mean = float(gold['mean'])
  gp = cls(X, list(gold['Y']), kern, lambda x: np.array([mean] * len(x)), float(gold['noise']))
  assert gp.handle_non_psd_kernels == 'project_first' and not gp._generic
  mu, sd = gp.eval(Xt, 'std')
  for got, key in ((gp.K_trtr_wo_noise, 'K'), (gp.L, 'L'), (gp.alpha, 'alpha'), (gp.compute_log_marginal_likelihood(), 'lml'),
                   (mu, 'mu'), (sd, 'sd')):
    assert relerr(got, gold[key]) <= 1e-9, (name, key, relerr(got, gold[key]))


@needs_reference
def test_pickle_and_deepcopy_round_trip_of_the_cp_gp_class(monkeypatch):
  from dragonfly_amd import kernel as K
  from dragonfly_amd import cartesian_product_gp
  from oracle_engine_cp import patch_engine_cp
  patch_engine_cp(monkeypatch)
  cls, mod = _cp_gp_class()
  assert cartesian_product_gp.device_cpgp_class(mod) is cls          # one class per reference module
  assert pickle.loads(pickle.dumps(cls)) is cls
  kern = K.CartesianProductKernel(1.0, [K.SEKernel(1, 1.0, [0.5]), K.HammingKernel([1.0])])
  X = [[[0.1 * i], ['a' if i % 2 else 'b']] for i in range(6)]
  gp = cls(X, [0.0, 1.0, 0.5, 0.2, 0.9, 0.4], kern, K.SEKernel, 0.1, build_posterior=False)
  gp.mean_func = None
  for clone in (pickle.loads(pickle.dumps(gp)), copy.deepcopy(gp)):
    assert type(clone) is cls and clone.X == gp.X and clone.noise_var == 0.1
    assert clone.kernel.kernel_list[1].coder.columns == kern.kernel_list[1].coder.columns
