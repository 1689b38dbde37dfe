"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

tests/oracle_engine_cp.py's CPU stand-in for the engine, extended with what the fused acquisitions on Cartesian-product
domains use of a fitted GP (dragonfly_amd.engine.FittedGP): points in progress under a projection flag -- the whole
augmented matrix goes through _get_cholesky_decomp's branch, gp_core.py:199-206 -- and thompson_pointwise, the
per-candidate one-point draw.  Every call of a fitted GP is counted in the engine's `calls` dictionary."""
import numpy as np

import oracle_engine
import oracle_engine_cp
from oracle import ref_numpy as O


class CpAcqOracleFittedGP(oracle_engine.OracleFittedGP):
  """ OracleFittedGP that remembers the branch of _get_cholesky_decomp it was fitted by """

  def __init__(self, engine, spec, X, y_centred, noise_var, gram=None, handle_non_psd_kernels='guaranteed_psd'):
    oracle_engine.OracleFittedGP.__init__(self, engine, spec, X, y_centred, noise_var, gram=gram,
                                          handle_non_psd_kernels=handle_non_psd_kernels)
    self.mode = handle_non_psd_kernels

  def _count(self, name):
    calls = getattr(self.engine, 'calls', None)
    if calls is not None:
      calls[name] = calls.get(name, 0) + 1

  def _halluc_std(self, Xs, X_halluc):
    """ gp_core.py:199-217 for a kernel that is guaranteed PSD: the diagonal of the augmented posterior covariance """
    og = self.oracle
    Xs, Xh = np.asarray(Xs, dtype=np.float64), np.asarray(X_halluc, dtype=np.float64)
    X_aug = np.vstack((og.X, Xh))
    K_haha, K_trha = og.kernel(Xh, Xh), og.kernel(og.X, Xh)
    aug_K = np.vstack((np.hstack((og.K_trtr_wo_noise, K_trha)), np.hstack((K_trha.T, K_haha))))
    aug_L = O.get_cholesky_decomp(aug_K, og.noise_var, self.mode)
    aug_V = O.solve_lower_triangular(aug_L, og.kernel(Xs, X_aug).T)
    return np.sqrt(np.diag(og.kernel(Xs, Xs) - aug_V.T.dot(aug_V)))

  def _posterior(self, Xs, want_std, X_halluc):
    if want_std and X_halluc is not None and len(X_halluc) > 0:
      self._count('with_points_in_progress')
      return self.oracle.eval(np.asarray(Xs, dtype=np.float64), 'none')[0], self._halluc_std(Xs, X_halluc)
    return oracle_engine.OracleFittedGP.predict(self, Xs, want_std, X_halluc)

  def predict(self, Xs, want_std=True, X_halluc=None):
    self._count('predict')
    return self._posterior(Xs, want_std, X_halluc)

  def acq_argmax(self, acq, Xs, params=(0.0, 0.0), mean_const=0.0, mean_vals=None, X_halluc=None, return_vals=False):
    self._count('acq_argmax')
    mu, sd = self._posterior(Xs, True, X_halluc)
    mu = mu + (mean_const if mean_vals is None else np.asarray(mean_vals))
    vals = O.acq_values(acq, mu, sd, params[0], params[1] if len(params) > 1 else 0.0)
    best_val, best_idx = O.argmax_first(vals)
    return (best_val, best_idx, vals) if return_vals else (best_val, best_idx)

  def thompson_pointwise(self, Xs, normals=None, X_halluc=None, mean_const=0.0, mean_vals=None, return_samples=False):
    """ per candidate draw_gaussian_samples(1, [mu_i], [[v_i]]) (general_utils.py:224-232): sqrt(v_i) u_i + mu_i, and
        the ValueError of the ladder where v_i is not positive """
    self._count('thompson_pointwise')
    mu, sd = self._posterior(Xs, True, X_halluc)
    mu = mu + (mean_const if mean_vals is None else np.asarray(mean_vals))
    if not np.all(sd * sd > 0):
      raise ValueError('Could not compute Cholesky decomposition of a 1 x 1 posterior covariance.')
    normals = np.random.normal(size=(len(mu), 1)).ravel() if normals is None else np.ravel(normals)
    samples = sd * normals + mu
    best_val, best_idx = O.argmax_first(samples)
    return (best_val, best_idx, samples) if return_samples else (best_val, best_idx)

  def thompson(self, *args, **kwargs):
    self._count('thompson')
    return oracle_engine.OracleFittedGP.thompson(self, *args, **kwargs)

  def predict_covar(self, Xs, X_halluc=None):
    self._count('predict_covar')
    if X_halluc is not None and len(X_halluc) > 0 and self.mode != 'guaranteed_psd':
      raise NotImplementedError('the stand-in has no joint covariance with points in progress under a projection flag')
    return oracle_engine.OracleFittedGP.predict_covar(self, Xs, X_halluc)


def patch_engine_cp_acq(monkeypatch):
  """ oracle_engine_cp.patch_engine_cp with fitted GPs of the class above and a call counter `eng.calls` """
  eng = oracle_engine_cp.patch_engine_cp(monkeypatch)
  eng.calls = {}

  def gp_fit(spec, X, y_centred, noise_var, allow_jitter=True, handle_non_psd_kernels='guaranteed_psd'):
    return CpAcqOracleFittedGP(eng, spec, X, y_centred, noise_var, handle_non_psd_kernels=handle_non_psd_kernels)
  monkeypatch.setattr(eng, 'gp_fit', gp_fit, raising=False)
  return eng
