"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

tests/oracle_engine.py's CPU stand-in for the engine, extended with the two multi-objective methods of
dragonfly_amd.engine.Engine (mo_ucb_argmax / mo_thompson): the reference's arithmetic
(opt/multiobjective_gpb_acquisitions.py:19-107) over the stand-in's per-objective posteriors and joint draws.
oracle_engine.py itself is left as it is."""
import numpy as np

import oracle_engine
from oracle import ref_numpy as O


def scalarise_ucb(scal, beta, weights, refs, mus, sds):
  """ :80-89 / :97-105 from the objectives' (mu, sd) """
  if scal == 'lin':
    mu_tot, sigma2_tot = 0.0, 0.0
    for mu, sigma, weight in zip(mus, sds, weights):
      mu_tot += mu * weight
      sigma2_tot += sigma * sigma * weight**2
    return mu_tot + beta * np.sqrt(sigma2_tot)
  ret = np.asarray([np.inf for _ in range(len(mus[0]))])
  for mu, sigma2, weight, ref in zip(mus, sds, weights, refs):
    ucb = mu + beta * np.sqrt(sigma2) - ref
    ret = np.minimum(ret, ucb / weight)
  return ret


def scalarise_ts(scal, weights, refs, samples):
  """ :36-39 / :61-65 from the objectives' draws """
  if scal == 'lin':
    s = 0.0
    for sample, weight in zip(samples, weights):
      s += sample * weight
    return s
  s = np.full((len(samples[0]), ), np.inf)
  for sample, weight, ref in zip(samples, weights, refs):
    s = np.minimum(s, (sample - ref) / weight)
  return s


def _means(k, m, mean_consts, mean_vals):
  if mean_vals is not None:
    return [np.asarray(mean_vals[i], dtype=np.float64) for i in range(k)]
  consts = np.zeros(k) if mean_consts is None else mean_consts
  return [np.array([consts[i]] * m) for i in range(k)]


class MooOracleEngine(oracle_engine.OracleEngine):
  """ OracleEngine + the multi-objective calls; `calls` records (method, candidates) of each """

  def __init__(self):
    self.calls = []

  def mo_ucb_argmax(self, gps, scal, beta, weights, refs, Xs, mean_consts=None, mean_vals=None, return_vals=False):
    Xs = np.asarray(Xs, dtype=np.float64)
    self.calls.append(('mo_ucb_argmax', len(Xs)))
    means = _means(len(gps), len(Xs), mean_consts, mean_vals)
    mus, sds = [], []
    for gp, mean in zip(gps, means):
      mu, sd = gp.predict(Xs, True)
      mus.append(mean + mu)                  # test_mean + K_tetr.dot(alpha), gp_core.py:173-175
      sds.append(sd)
    vals = scalarise_ucb(scal, beta, weights, refs, mus, sds)
    best_val, best_idx = O.argmax_first(vals)
    return (best_val, best_idx, vals) if return_vals else (best_val, best_idx)

  def mo_thompson(self, gps, scal, weights, refs, Xs, U, block=4096, X_halluc=None, mean_consts=None, mean_vals=None,
                  return_vals=False):
    Xs = np.asarray(Xs, dtype=np.float64)
    k, m = len(gps), len(Xs)
    self.calls.append(('mo_thompson', m))
    U = np.asarray(U, dtype=np.float64).reshape(k, m)
    means = _means(k, m, mean_consts, mean_vals)
    samples, powers = [], []
    for i, gp in enumerate(gps):
      draw, pw = np.empty(m), []
      for i0 in range(0, m, block):
        sl = slice(i0, min(m, i0 + block))
        if X_halluc is not None and len(X_halluc) > 0:      # gp_core.py:256-261
          mu, cov = gp.oracle.eval_with_hallucinated_observations(Xs[sl], np.asarray(X_halluc, dtype=np.float64), 'covar')
        else:
          mu, cov = gp.oracle.eval(Xs[sl], 'covar')
        draw[sl] = O.draw_gaussian_samples_with_normals(means[i][sl] + mu, cov, U[i, sl].reshape(-1, 1)).ravel()
        pw.append(O.stable_cholesky(cov, return_power=True)[1])
      samples.append(draw)
      powers.append(pw)
    vals = scalarise_ts(scal, weights, refs, samples)
    best_val, best_idx = O.argmax_first(vals)
    return (best_val, best_idx, vals, powers) if return_vals else (best_val, best_idx)


def patch_engine_moo(monkeypatch):
  """ oracle_engine.patch_engine with a MooOracleEngine: every FittedGP the mirrors build carries it as .engine """
  monkeypatch.setattr(oracle_engine, 'OracleEngine', MooOracleEngine)
  return oracle_engine.patch_engine(monkeypatch)
