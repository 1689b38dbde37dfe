"""MI355X: the Hamming kernel (DFH_KERNEL_HAMMING) and Cartesian-product kernels on the device, and GPs built from
their descriptor with 'project_first', against the REAL reference's outputs (tests/golden/cp_*.npz,
tools/make_cp_golden.py).  One tolerance, the project's: 1e-10 norm-wise; Hamming matrices of at most 7 columns
bit for bit (the sum is sequential there and every term is a weight or 0)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def _gen():
  spec = importlib.util.spec_from_file_location('make_cp_golden', os.path.join(ROOT, 'tools', 'make_cp_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


G = _gen()


@pytest.mark.parametrize('idx', range(len(G.HAMMING_CASES)))
def test_hamming_matrices_equal_the_reference(engine, idx):
  from dragonfly_amd import kernel as K
  name, dim, weights, cats, n1, n2 = G.HAMMING_CASES[idx]
  gold = load_golden('cp_' + name)
  kern = K.HammingKernel(G.hamming_weights(weights, dim))
  X1, X2 = G.hamming_points(cats, n1, 100 + idx), G.hamming_points(cats, n2, 200 + idx, unseen=True)
  for got, key in ((kern(X1, X1), 'K11'), (kern(X1, X2), 'K12'), (kern(X2, X1), 'K21')):
    err = relerr(got, gold[key])
    print(name, key, 'relerr', err, 'bit-identical', np.array_equal(got, gold[key]))
    if dim <= 7:
      assert np.array_equal(got, gold[key]), (name, key, err)
    assert err <= TOL, (name, key, err)


@pytest.mark.parametrize('idx', range(len(G.CP_CASES)))
def test_cp_kernel_matrices_agree_with_the_reference(engine, idx):
  from dragonfly_amd import kernel as K
  name, parts, n1, n2 = G.CP_CASES[idx]
  gold = load_golden(name)
  scale, pars = G.cp_hyperparams(parts, 500 + idx)
  kern = G.build_cp_kernel(K, parts, scale, pars)
  assert kern.has_device_spec()
  X1, X2 = G.cp_points(parts, n1, 300 + idx), G.cp_points(parts, n2, 400 + idx, unseen=True)
  for got, key in ((kern(X1, X1), 'K11'), (kern(X1, X2), 'K12'), (kern(X2, X1), 'K21')):
    err = relerr(got, gold[key])
    print(name, key, 'relerr', err)
    assert err <= TOL, (name, key, err)


def _cp_gp(parts, X, Y, kern, mean, noise, **kwargs):
  """ the device GP of a CP kernel from its descriptor: gp_core.GP with the packing and the flag, as the class
      install(cartesian_product=True) makes (tests/test_cp_cpu.py checks that class on the stand-in engine) """
  from dragonfly_amd.gp_core import GP

  class PackedCPGP(GP):
    _generic = False

    def _points_array(self, pts):
      return self.kernel.pack(pts)
  return PackedCPGP(X, Y, kern, lambda x: np.array([mean] * len(x)), noise, handle_non_psd_kernels='project_first', **kwargs)


@pytest.mark.parametrize('idx', range(len(G.GP_CASES)))
def test_cp_gp_with_project_first_agrees_with_the_reference(engine, idx):
  from dragonfly_amd import kernel as K
  name, parts, n, m = G.GP_CASES[idx]
  gold = load_golden(name)
  scale, pars = G.cp_hyperparams(parts, 1000 + idx)
  kern = G.build_cp_kernel(K, parts, scale, pars)
  X, Xt, Xh = G.cp_points(parts, n, 600 + idx), G.cp_points(parts, m, 700 + idx, unseen=True), G.cp_points(parts, 5, 800 + idx)
  gp = _cp_gp(parts, X, list(gold['Y']), kern, float(gold['mean']), float(gold['noise']))
  mu, sd = gp.eval(Xt, 'std')
  _, cov = gp.eval(Xt, 'covar')
  _, sd_h = gp.eval_with_hallucinated_observations(Xt, Xh, 'std')
  _, _, draw, _ = gp.device_gp.thompson(gp._points_array(Xt), gold['U'], block=m, mean_vals=gp.mean_func(Xt), return_samples=True)
  figures = [('K', gp.K_trtr_wo_noise), ('L', gp.L), ('alpha', gp.alpha), ('lml', gp.compute_log_marginal_likelihood()),
             ('mu', mu), ('sd', sd), ('cov', cov), ('sd_halluc', sd_h), ('draw', draw)]
  errs = {key: relerr(got, gold[key]) for key, got in figures}
  print(name, errs)
  for key, err in errs.items():
    assert err <= TOL, (name, key, err)


def test_dfh_gp_fit_honours_the_projection_flags(engine):
  """ a Hamming weight below zero makes the kernel matrix indefinite (smallest eigenvalue about -3 here), so the
      projection moves it by far more than the tolerance: a fit that ignored the flag cannot pass.  project_first
      gives the factor of the projected matrix; try_before_project reaches its projection branch, because
      K + noise I is not positive definite; a handle fitted so keeps its kernel. """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(5)
  n = 128
  P = np.hstack([rs.random_sample((n, 2)), rs.randint(0, 3, (n, 2)).astype(float)])
  y = rs.randn(n)
  spec = KernelSpec('product', 4, 1.3, groups=[[0, 1], [2, 3]], sub_kinds=['se', 'hamming'], sub_scales=[1.0, 1.0],
                    sub_nus=[0.0, 0.0], sub_bandwidths=[[0.7, 0.9], [0.6, -0.9]])
  Kmat = engine.kernel_matrix(spec, P)
  eigs = np.linalg.eigvalsh(Kmat)
  assert eigs.min() < -0.5
  Lhost = np.linalg.cholesky(_project(Kmat) + 1e-3 * np.eye(n))
  with pytest.raises(ValueError):                           # the ladder cannot repair it: what the parent's dfh_gp_fit does with any flag
    engine.gp_fit(spec, P, y, 1e-3)
  for mode in ('project_first', 'try_before_project'):
    a = engine.gp_fit(spec, P, y, 1e-3, handle_non_psd_kernels=mode)
    b = engine.gp_fit_gram(Kmat, y, 1e-3, handle_non_psd_kernels=mode)
    errs = dict(L_vs_gram=relerr(a.get_L(), b.get_L()), alpha_vs_gram=relerr(a.get_alpha(), b.get_alpha()),
                lml_vs_gram=abs(a.lml - b.lml) / abs(b.lml), L_vs_host_eigh=relerr(a.get_L(), Lhost))
    print(mode, errs)
    for key, err in errs.items():
      assert err <= TOL, (mode, key, err)
    assert np.array_equal(a.get_K(), Kmat)                # the unprojected kernel matrix
    # the handle keeps kernel and inputs: predictions, with and without hallucinated points, as from the projected Gram
    shift = np.array([1.0, 1.0, 0.0, 0.0])             # (the Euclidean columns only: the codes stay codes)
    Pt, Ph = P[:9] + 0.01 * shift, P[40:43] + 0.02 * shift
    mu, sd = a.predict(Pt, want_std=True)
    mu_b, sd_b = b.predict_gram(engine.kernel_matrix(spec, Pt, P), np.diag(engine.kernel_matrix(spec, Pt)).copy())
    # (mean only beyond agreement of the two routes: with an indefinite kernel the raw posterior variance is negative, NaN in both)
    assert np.all(np.isfinite(mu_b)) and relerr(mu, mu_b) <= TOL and np.allclose(sd, sd_b, rtol=TOL, atol=0, equal_nan=True)
    ext = a.append(Ph, np.concatenate([y, [0.1, 0.2, 0.3]]))
    Pall = np.vstack([P, Ph])
    whole = engine.gp_fit(spec, Pall, np.concatenate([y, [0.1, 0.2, 0.3]]), 1e-3, handle_non_psd_kernels=mode)
    assert relerr(ext.get_L(), whole.get_L()) <= TOL and relerr(ext.get_alpha(), whole.get_alpha()) <= TOL
  lml = engine.gp_lml_batch([spec, spec], P, y, [0.0, 0.1], [1e-3, 2e-3], handle_non_psd_kernels='project_first')
  ref = [engine.gp_fit_gram(Kmat, y - mc, nv, handle_non_psd_kernels='project_first').lml for mc, nv in ((0.0, 1e-3), (0.1, 2e-3))]
  assert relerr(lml, ref) <= TOL


def test_rand_tuner_batch_and_fitted_gp_agree_with_the_reference_fitter(engine):
  """ tests/golden/cp_fitter_mixed_n60.npz: the 100 candidates the reference's 'rand' tuner asked for (mean, log noise,
      log scale, 3 + 2 log bandwidths, 3 Hamming weights), their log marginal likelihoods, the winner's index, and the
      fitted GP's posterior -- the candidates in ONE dfh_gp_lml_batch call with project_first """
  from dragonfly_amd import kernel as K
  gold = load_golden('cp_fitter_mixed_n60')
  X, Y = G.fitter_data()
  Xt = G.fitter_data(12)[0]

  def kernel_of(c):
    w = c[8:11]
    return K.CartesianProductKernel(np.exp(c[2]), [K.MaternKernel(3, 2.5, 1.0, np.exp(c[3:6])), K.MaternKernel(2, 2.5, 1.0, np.exp(c[6:8])),
                                                   K.HammingKernel(w / w.sum())])
  cands = gold['rand_cands']
  kerns = [kernel_of(c) for c in cands]
  P = kerns[0].pack(X)
  lmls = engine.gp_lml_batch([k.to_spec() for k in kerns], P, np.asarray(Y), cands[:, 0], np.exp(cands[:, 1]),
                             handle_non_psd_kernels='project_first')
  err = relerr(lmls, gold['rand_lmls'])
  print('lml batch relerr', err, 'argmax', int(np.argmax(lmls)), int(gold['rand_argmax']))
  assert err <= TOL
  assert int(np.argmax(lmls)) == int(gold['rand_argmax'])
  best = kerns[int(np.argmax(lmls))]
  assert best.hyperparams['scale'] == float(gold['scale'])
  assert np.array_equal(best.kernel_list[2].hyperparams['dim_weights'], gold['weights'])
  gp = _cp_gp(None, X, Y, best, float(gold['mean']), float(gold['noise']))
  mu, sd = gp.eval(Xt, 'std')
  errs = dict(lml=relerr(gp.compute_log_marginal_likelihood(), gold['lml']), mu=relerr(mu, gold['mu']), sd=relerr(sd, gold['sd']))
  print(errs)
  for key, e in errs.items():
    assert e <= TOL, (key, e)


def _project(M):
  vals, vecs = np.linalg.eigh(M)
  return (vecs * np.clip(vals, 0, np.inf)).dot(vecs.T)


def test_descriptor_path_agrees_with_the_host_kernel_path_at_size(engine):
  """ n = 2048: the blocked factorisation and the projection at size; the Gram matrix of the second GP is composed
      in NumPy from the packed points """
  from dragonfly_amd import kernel as K
  rs = np.random.RandomState(11)
  n, m = 2048, 64
  letters = ['a', 'b', 'c', 'd', 'e']
  def points(k):
    return [[list(rs.random_sample(3)), [letters[rs.randint(5)], int(rs.randint(4)), letters[rs.randint(3)]]] for _ in range(k)]
  X, Xt = points(n), points(m)
  y = np.array([np.sin(4 * sum(x[0])) + 0.2 * (x[1][0] == 'a') for x in X]) + 0.05 * rs.randn(n)
  bws, w = np.array([0.3, 0.5, 0.8]), np.array([0.5, 0.3, 0.2])
  kern = K.CartesianProductKernel(0.9, [K.SEKernel(3, 1.0, bws), K.HammingKernel(w)])
  P, Pt = kern.pack(X), kern.pack(Xt)

  def host_kernel(A, B):
    A3, B3 = A[:, :3] / bws, B[:, :3] / bws
    d2 = np.clip((A3 ** 2).sum(axis=1)[:, None] + (B3 ** 2).sum(axis=1)[None, :] - 2 * A3.dot(B3.T), 0, np.inf)
    ham = np.zeros((len(A), len(B)))
    for j in range(len(B)):
      ham[:, j] = (np.equal(A[:, 3:], B[j, 3:]) * w).sum(axis=1)
    return 0.9 * np.ones((len(A), len(B))) * np.exp(-d2 / 2) * ham
  a = engine.gp_fit(kern.to_spec(), P, y, 0.01, handle_non_psd_kernels='project_first')
  b = engine.gp_fit_gram(host_kernel(P, P), y, 0.01, handle_non_psd_kernels='project_first')
  mu_a, sd_a = a.predict(Pt, want_std=True)
  Kc = host_kernel(Pt, P)
  mu_b, sd_b = b.predict_gram(Kc, np.diag(host_kernel(Pt, Pt)).copy())
  errs = dict(K=relerr(a.get_K(), host_kernel(P, P)), alpha=relerr(a.get_alpha(), b.get_alpha()), lml=abs(a.lml - b.lml) / abs(b.lml),
              mu=relerr(mu_a, mu_b), sd=relerr(sd_a, sd_b))
  print(errs)
  for key, err in errs.items():
    assert err <= TOL, (key, err)


class _PlainKernel(object):
  """ a part the device does not know, as a plain Python class """
  hyperparams = {}
  dim = 1

  def is_guaranteed_psd(self):
    return True

  def __call__(self, X1, X2=None):
    X2 = X1 if X2 is None else X2
    return np.array([[1.0 / (1.0 + abs(a[0] - b[0])) for b in X2] for a in X1])


def test_a_kernel_with_an_undescribed_part_takes_host_kernel_mode(engine):
  from dragonfly_amd import kernel as K
  from dragonfly_amd.gp_core import GP
  rs = np.random.RandomState(3)
  X = [[[rs.random_sample()], [['a', 'b', 'c'][rs.randint(3)]]] for _ in range(50)]
  Xt = [[[rs.random_sample()], [['a', 'b', 'zz'][rs.randint(3)]]] for _ in range(12)]
  y = rs.randn(50)
  kern = K.CartesianProductKernel(1.1, [_PlainKernel(), K.HammingKernel([1.0])])
  assert not kern.has_device_spec()
  gp = GP(X, list(y), kern, lambda x: np.zeros(len(x)), 0.05, handle_non_psd_kernels='project_first')
  assert gp._generic
  Kh = kern._host_compose(X, X)
  ref = engine.gp_fit_gram(Kh, y, 0.05, handle_non_psd_kernels='project_first')
  mu_ref, sd_ref = ref.predict_gram(kern._host_compose(Xt, X), np.diag(kern._host_compose(Xt, Xt)).copy())
  mu, sd = gp.eval(Xt, 'std')
  assert relerr(gp.alpha, ref.get_alpha()) <= TOL and relerr(mu, mu_ref) <= TOL and relerr(sd, sd_ref) <= TOL


def _desc(kind, dim, scale=1.0, nu=0.0, bw=None):
  from dragonfly_amd import _lib
  d = _lib.KernelDesc()
  d.kind, d.dim, d.scale, d.nu = kind, dim, scale, nu
  keep = None
  if bw is not None:
    keep = np.ascontiguousarray(bw, dtype=np.float64)
    d.bw = keep.ctypes.data_as(_lib.c_double_p)
  return d, keep


def _kernel_matrix_status(engine, desc, dim):
  X = np.zeros((4, dim))
  out = np.empty((4, 4))
  return engine.lib.dfh_kernel_matrix(engine.ctx, C.byref(desc), X.ctypes.data_as(C.c_void_p), 4, None, 0, C.c_double(0.0),
                                      out.ctypes.data_as(C.c_void_p))


def test_descriptor_validation(engine):
  from dragonfly_amd import _lib
  from dragonfly_amd.engine import KernelSpec
  BAD = 2
  ok, keep = _desc(_lib.KERNEL_HAMMING, 3, bw=[0.5, 0.3, 0.2])
  assert _kernel_matrix_status(engine, ok, 3) == 0
  for bad in (_desc(_lib.KERNEL_HAMMING, 0, bw=[1.0]), _desc(_lib.KERNEL_HAMMING, 3), _desc(_lib.KERNEL_HAMMING, 3, scale=2.0, bw=[1, 1, 1]),
              _desc(_lib.KERNEL_HAMMING, 3, nu=1.0, bw=[1, 1, 1]), _desc(_lib.KERNEL_HAMMING, 33, bw=np.ones(33))):
    assert _kernel_matrix_status(engine, bad[0], max(bad[0].dim, 1)) == BAD
  X = np.zeros((4, 3))
  additive = KernelSpec('additive', 3, 1.0, groups=[[0], [1, 2]], sub_kinds=['se', 'hamming'], sub_scales=[1.0, 1.0],
                        sub_nus=[0.0, 0.0], sub_bandwidths=[[1.0], [0.5, 0.5]])
  esp = KernelSpec('esp', 2, 1.0, nu=1, sub_kinds=['se', 'hamming'], sub_scales=[1.0, 1.0], sub_nus=[0.0, 0.0],
                   sub_bandwidths=[[1.0], [1.0]])
  nested = KernelSpec('product', 3, 1.0, groups=[[0], [1], [2]], sub_kinds=['se', 'se', 'hamming'], sub_scales=[1.0] * 3,
                      sub_nus=[0.0] * 3, sub_bandwidths=[[1.0], [1.0], [1.0]], group_factors=[0, 1, 1], factor_sums=[False, True],
                      factor_scales=[1.0, 1.0])
  for spec in (additive, esp, nested):
    with pytest.raises(ValueError):
      engine.kernel_matrix(spec, X[:, :spec.dim])
  # a Hamming kernel has no additive groups: the add-UCB entry points refuse its handle
  gp = engine.gp_fit(KernelSpec('hamming', 3, 1.0, [0.5, 0.3, 0.2]), np.array([[0., 1, 2], [1, 1, 0], [2, 0, 0], [0, 0, 1]]),
                     np.array([0.1, 0.2, -0.1, 0.3]), 0.1)
  with pytest.raises(ValueError):
    gp.add_ucb_group(0, 1.0, np.zeros((2, 1)))


def test_small_tuning_calls_with_hamming_parts_take_the_per_candidate_path(engine):
  """ the one-launch small-n tuning kernels do not know the Hamming part; such candidates must give the same values
      as single fits """
  from dragonfly_amd import kernel as K
  rs = np.random.RandomState(9)
  for n in (40, 100):
    X = [[list(rs.random_sample(2)), [['a', 'b'][rs.randint(2)], int(rs.randint(3))]] for _ in range(n)]
    y = rs.randn(n)
    kerns = [K.CartesianProductKernel(s, [K.MaternKernel(2, 2.5, 1.0, [b, 2 * b]), K.HammingKernel([w, 1 - w])])
             for s, b, w in ((0.8, 0.4, 0.3), (1.4, 0.7, 0.6), (1.0, 1.1, 0.5))]
    P = kerns[0].pack(X)
    specs = [k.to_spec() for k in kerns]
    lml = engine.gp_lml_batch(specs, P, y, [0.0, 0.1, -0.1], [0.01, 0.02, 0.05])
    ref = [engine.gp_fit(s, P, y - mc, nv).lml for s, mc, nv in zip(specs, (0.0, 0.1, -0.1), (0.01, 0.02, 0.05))]
    assert relerr(lml, ref) <= TOL, (n, lml, ref)
