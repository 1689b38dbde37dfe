"""post_hp_tune_method='nuts' under dragonfly_amd.install(), on the engine's CPU stand-in: the unmodified reference's
EuclideanGPFitter samples its hyper-parameters with its own NUTS sampler, every gradient coming from the mirror's
GP.compute_grad_log_marginal_likelihood.  The stand-in (tests/oracle_engine.py) is subclassed here with lml_grad in
NumPy -- the device's route, not the reference's: one inverse, W = alpha alpha^T - A^-1, F = -2 W dK/d(dsq), and the
bandwidth components from F's row sums and F Xs.  Without install() the same run dies in the reference's kernel gradient
(kernel.py:216: a 2-D index into the 1-D bandwidth array), which is why the feature exists.  Needs the reference tree."""
import os
import warnings

import numpy as np
import pytest

import oracle_engine as OE

REF = os.environ.get('DRAGONFLY_REFERENCE', '/root/reference')
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'dragonfly')),
                                reason='needs the reference tree (build container only)')

N, DIM, BURN, NUM_SAMPLES = 30, 3, 5, 2


class GradFittedGP(OE.OracleFittedGP):
  """ the stand-in's fitted GP with FittedGP.lml_grad """

  def lml_grad(self):
    spec, og = self.spec, self.oracle
    if spec is None or spec.kind not in ('se', 'matern') or spec.nu > 2.5:
      raise ValueError('lml_grad: a single SE or MATERN kernel only')
    X, bw = np.asarray(og.X, dtype=float), np.ravel(spec.bandwidths)
    n, d = X.shape
    Xs = X / bw
    sq = (Xs ** 2).sum(axis=1)
    dsq = np.clip(sq[:, None] + sq[None, :] - 2 * Xs.dot(Xs.T), 0.0, np.inf)
    np.fill_diagonal(dsq, 0.0)
    K = og.K_trtr_wo_noise
    if spec.kind == 'se':
      dk2 = K.copy()                                     # -2 dK/d(dsq)
    else:
      dist, s2 = np.sqrt(dsq), np.sqrt(2 * spec.nu)
      e = spec.scale * np.exp(-s2 * dist)
      p = int(spec.nu)
      if p == 0:
        dk2 = s2 * e / np.where(dist == 0, 1.0, dist)
      elif p == 1:
        dk2 = s2 * s2 * e
      else:
        dk2 = (s2 * s2 / 3) * (1 + s2 * dist) * e
    Linv = np.linalg.inv(og.L)
    W = np.outer(og.alpha, og.alpha) - Linv.T.dot(Linv)
    F = np.where(dsq == 0, 0.0, W * dk2)
    r, G = F.sum(axis=1), F.dot(Xs)
    grad = np.zeros(d + 3)
    grad[0] = 0.5 * (W * K).sum()
    grad[1:d + 1] = (Xs * (Xs * r[:, None] - G)).sum(axis=0)
    grad[d + 1] = 0.5 * og.noise_var * np.trace(W)
    grad[d + 2] = og.alpha.sum()
    return grad, self.lml


class GradEngine(OE.OracleEngine):
  def gp_fit(self, spec, X, y_centred, noise_var, allow_jitter=True):
    return GradFittedGP(self, spec, X, y_centred, noise_var)


def _patch_engine(monkeypatch):
  """ oracle_engine.patch_engine with the engine above """
  from dragonfly_amd import euclidean_gp, general_utils, gp_core, gpb_acquisitions, kernel
  from dragonfly_amd import engine as engine_mod
  eng = GradEngine()
  for mod in (engine_mod, euclidean_gp, general_utils, gp_core, kernel):
    monkeypatch.setattr(mod, 'get_engine', lambda _e=eng: _e)
  monkeypatch.setattr(gpb_acquisitions, 'DEVICE_CANDIDATES', False)
  return eng


def _data():
  rs = np.random.RandomState(5)
  X = [rs.rand(DIM) for _ in range(N)]
  Y = [float(np.sin(3 * x).sum() + 0.1 * rs.randn()) for x in X]
  return X, Y


def _run_nuts():
  """ EuclideanGPFitter.fit_gp with post_sampling / nuts, as the bandit would hold it """
  import dragonfly.opt.gp_bandit as GB
  from dragonfly.gp.euclidean_gp import euclidean_gp_args
  from dragonfly.utils.option_handler import load_options
  X, Y = _data()
  options = load_options(euclidean_gp_args, partial_options={
    'kernel_type': 'se', 'hp_tune_criterion': 'post_sampling', 'post_hp_tune_method': 'nuts', 'post_hp_tune_burn': BURN,
    'post_hp_tune_offset': 1, 'num_post_samples': NUM_SAMPLES})
  np.random.seed(11)
  fitter = GB.EuclideanGPFitter(X, Y, options=options)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    ret = fitter.fit_gp(num_samples=NUM_SAMPLES)
  return fitter, ret


def test_reference_nuts_tuning_runs_on_the_mirror_s_gradient(monkeypatch):
  from oracle.make_golden import import_reference
  import_reference()
  from dragonfly.gp import kernel as ref_kernel
  from dragonfly.gp.gp_core import GP as RefGP
  from dragonfly_amd import install
  from dragonfly_amd.gp_core import GP as MirrorGP
  ref_se = ref_kernel.SEKernel                         # the reference's own classes, whatever install() rebinds
  _patch_engine(monkeypatch)
  calls = []
  mirror_grad = MirrorGP.compute_grad_log_marginal_likelihood

  def recorded(self, param, param_num=None):
    value = mirror_grad(self, param, param_num)
    hp = self.kernel.hyperparams
    calls.append((param, param_num, float(hp['scale']), np.ravel(hp['dim_bandwidths']).astype(float).copy(),
                  float(self.noise_var), float(self.mean_func([np.zeros(DIM)])[0]), value))
    return value
  monkeypatch.setattr(MirrorGP, 'compute_grad_log_marginal_likelihood', recorded)
  install.install()
  try:
    fitter, ret = _run_nuts()
  finally:
    install.uninstall()
  assert ret[0] == 'post_sample_hps_with_probs'
  cts = np.array(ret[1], dtype=float)                    # one row of continuous hyper-parameters per sample
  assert cts.shape == (NUM_SAMPLES, len(fitter.cts_hp_bounds))
  lo, hi = np.array(fitter.cts_hp_bounds, dtype=float).T
  assert np.all(np.isfinite(cts)) and np.all(cts >= lo) and np.all(cts <= hi)
  assert len(calls) > 50
  # (the default options tune the constant mean and the noise variance with the kernel's scale and bandwidths)
  assert {c[0] for c in calls} == {'scale', 'dim_bandwidths', 'noise_var', 'noise_mean'}
  assert {c[1] for c in calls if c[0] == 'dim_bandwidths'} == set(range(DIM))
  X, Y = _data()
  worst = 0.0
  for param, param_num, scale, bw, noise_var, mean, got in calls:
    kern = ref_se(DIM, scale, bw)
    kern.hyperparams['dim_bandwidths'] = bw.reshape(1, -1)
    ref_gp = RefGP(X, Y, kern, lambda x, _m=mean: np.array([_m] * len(x)), noise_var)
    want = ref_gp.compute_grad_log_marginal_likelihood(param, param_num)
    worst = max(worst, abs(got - want) / max(abs(want), 1.0))
  print('gradient calls', len(calls), 'largest distance from the reference', worst)
  assert worst <= 1e-9


def test_reference_nuts_tuning_fails_without_install():
  from oracle.make_golden import import_reference
  import_reference()
  with pytest.raises(IndexError):
    _run_nuts()
