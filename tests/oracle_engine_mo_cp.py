"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

tests/oracle_engine_cp_acq.py's CPU stand-in for the engine, extended with the two multi-objective methods the fused
acquisitions on Cartesian-product domains use of dragonfly_amd.engine.Engine: mo_ucb_argmax on packed rows and
mo_thompson_pointwise -- per candidate and objective the one-point draw sqrt(v) u + mu, the normals POINT-major, scalarised
by the reference's arithmetic (tests/oracle_engine_moo.py).  Both are counted in the engine's `calls` dictionary, beside
the fitted GPs' own calls.  oracle_engine_cp_acq.py itself is left as it is."""
import numpy as np

import oracle_engine
import oracle_engine_cp_acq
from oracle import ref_numpy as O
from oracle_engine_moo import _means, scalarise_ts, scalarise_ucb


def patch_engine_mo_cp(monkeypatch):
  """ oracle_engine_cp_acq.patch_engine_cp_acq plus the two multi-objective calls, spied on in eng.calls """
  eng = oracle_engine_cp_acq.patch_engine_cp_acq(monkeypatch)

  def count(name):
    eng.calls[name] = eng.calls.get(name, 0) + 1

  def posteriors(gps, Xs, X_halluc, mean_consts, mean_vals):
    Xs = np.asarray(Xs, dtype=np.float64)
    means = _means(len(gps), len(Xs), mean_consts, mean_vals)
    mus, sds = [], []
    for gp, mean in zip(gps, means):
      mu, sd = gp._posterior(Xs, True, X_halluc)       # pylint: disable=protected-access
      mus.append(mean + mu)                            # test_mean + K_tetr.dot(alpha), gp_core.py:173-175
      sds.append(sd)
    return mus, sds

  def mo_ucb_argmax(gps, scal, beta, weights, refs, Xs, mean_consts=None, mean_vals=None, return_vals=False):
    count('mo_ucb_argmax')
    mus, sds = posteriors(gps, Xs, None, mean_consts, mean_vals)
    vals = scalarise_ucb(scal, beta, weights, refs, mus, sds)
    best_val, best_idx = O.argmax_first(vals)
    return (best_val, best_idx, vals) if return_vals else (best_val, best_idx)

  def mo_thompson_pointwise(gps, scal, weights, refs, Xs, normals=None, X_halluc=None, mean_consts=None, mean_vals=None,
                            return_vals=False, return_samples=False):
    count('mo_thompson_pointwise')
    mus, sds = posteriors(gps, Xs, X_halluc, mean_consts, mean_vals)
    k, m = len(gps), len(mus[0])
    if not all(np.all(sd * sd > 0) for sd in sds):
      raise ValueError('Could not compute Cholesky decomposition of a 1 x 1 posterior covariance.')
    if normals is None:                                # m k calls of np.random.normal(size=(1, 1)), as one stream
      normals = np.random.normal(size=m * k)
    normals = np.asarray(normals, dtype=np.float64)
    if normals.size != m * k:
      raise ValueError('normals must hold one standard normal per candidate and objective.')
    U = normals.reshape(m, k)
    samples = np.array([sds[j] * U[:, j] + mus[j] for j in range(k)])
    vals = scalarise_ts(scal, weights, refs, samples)
    best_val, best_idx = O.argmax_first(vals)
    return (best_val, best_idx) + ((vals,) if return_vals else ()) + ((samples,) if return_samples else ())

  def append(self, X_new, y_centred_all, allow_jitter=True):      # pylint: disable=unused-argument
    """ OracleFittedGP.append that keeps the class above and the fit's branch: appended GPs count their calls too """
    X_all = np.vstack([self.oracle.X, np.asarray(X_new, dtype=np.float64)])
    return oracle_engine_cp_acq.CpAcqOracleFittedGP(self.engine, self.spec, X_all, y_centred_all, self.oracle.noise_var,
                                                    handle_non_psd_kernels=getattr(self, 'mode', 'guaranteed_psd'))
  monkeypatch.setattr(oracle_engine.OracleFittedGP, 'append', append)
  monkeypatch.setattr(eng, 'mo_ucb_argmax', mo_ucb_argmax, raising=False)
  monkeypatch.setattr(eng, 'mo_thompson_pointwise', mo_thompson_pointwise, raising=False)
  return eng
