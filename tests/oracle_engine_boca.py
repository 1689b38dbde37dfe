"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

tests/oracle_engine.py's CPU stand-in for the engine, extended with what BOCA's decision step uses of
dragonfly_amd.engine: Engine.join_fixed and FittedGP.mf_add_ucb_group / mf_add_ucb_all.  The arithmetic is the
reference's own (_add_ucb_for_boca, opt/gpb_acquisitions.py:353-374) over oracle/ref_numpy.py's kernels and solves.
oracle_engine.py itself is left as it is."""
import numpy as np

import oracle_engine
from oracle import ref_numpy as O


def mf_add_ucb_values(og, z_opt, group, beta, Xg):
  """ _mf_add_ucb_acq_j (:360-374) with beta given and a zero group mean, on a GPOracle whose kernel is the product
      [fidelity kernel, additive domain kernel] over joint points [z, x] """
  prod = og.kernel
  (fid_cols, dom_cols), (fid, add) = prod.groups, prod.subs
  Xg = np.asarray(Xg, dtype=np.float64)
  z = np.asarray(z_opt, dtype=np.float64).reshape(1, -1)
  K_fidel_Z_tr_to_f2o = fid(og.X[:, fid_cols], z)                                      # :353
  K_fidel_f2o_to_f2o = float(fid(z, z))                                                # :354
  kernel_j, group_j = add.subs[group], add.groups[group]
  X_train_j = og.X[:, dom_cols][:, group_j]
  K_tetr_domain_j = kernel_j(Xg, X_train_j)
  K_tetr_fidel_j = np.repeat(K_fidel_Z_tr_to_f2o.T, len(Xg), axis=0)
  K_tetr_j = prod.scale * K_tetr_fidel_j * K_tetr_domain_j
  pred_mean_j = K_tetr_j.dot(og.alpha) + np.array([0] * len(Xg))
  K_tete_j = prod.scale * K_fidel_f2o_to_f2o * kernel_j(Xg, Xg)
  V_j = O.solve_lower_triangular(og.L, K_tetr_j.T)
  post_covar_j = K_tete_j - V_j.T.dot(V_j)
  return pred_mean_j + beta * np.sqrt(np.diag(post_covar_j))


class BocaOracleFittedGP(oracle_engine.OracleFittedGP):
  """ OracleFittedGP + the multi-fidelity add-UCB calls """

  def mf_add_ucb_group(self, z_opt, group, beta, Xg, return_vals=False):
    self.engine.calls.append(('mf_add_ucb_group', len(Xg)))
    vals = mf_add_ucb_values(self.oracle, z_opt, group, beta, Xg)
    best_val, best_idx = O.argmax_first(vals)
    return (best_val, best_idx, vals) if return_vals else (best_val, best_idx)

  def mf_add_ucb_all(self, z_opt, betas, cands_per_group, return_vals=False, sizes=None):
    self.engine.calls.append(('mf_add_ucb_all', [len(c) for c in cands_per_group]))
    vals = [mf_add_ucb_values(self.oracle, z_opt, g, betas[g], c) for g, c in enumerate(cands_per_group)]
    best = [O.argmax_first(v) for v in vals]
    out = (np.array([b[0] for b in best]), np.array([b[1] for b in best]))
    return out + (vals,) if return_vals else out

  def acq_argmax(self, acq, Xs, params=(0.0, 0.0), mean_const=0.0, mean_vals=None, X_halluc=None, return_vals=False):
    self.engine.calls.append(('acq_argmax', acq, np.shape(Xs), 0 if X_halluc is None else len(X_halluc)))
    return super(BocaOracleFittedGP, self).acq_argmax(acq, Xs, params, mean_const, mean_vals, X_halluc, return_vals)

  def thompson(self, Xs, U, block=4096, mean_const=0.0, mean_vals=None, return_samples=False):
    self.engine.calls.append(('thompson', np.shape(Xs)))
    return super(BocaOracleFittedGP, self).thompson(Xs, U, block, mean_const, mean_vals, return_samples)


class BocaOracleEngine(oracle_engine.OracleEngine):
  """ OracleEngine + join_fixed; `calls` records the fused calls BOCA's decisions made """

  def __init__(self):
    self.calls = []

  def join_fixed(self, z, cands):
    cands = np.asarray(cands, dtype=np.float64)
    self.calls.append(('join_fixed', cands.shape))
    return np.hstack((np.tile(np.asarray(z, dtype=np.float64).reshape(1, -1), (len(cands), 1)), cands))


def patch_engine_boca(monkeypatch):
  """ oracle_engine.patch_engine with a BocaOracleEngine whose fits are BocaOracleFittedGPs """
  monkeypatch.setattr(oracle_engine, 'OracleEngine', BocaOracleEngine)
  monkeypatch.setattr(oracle_engine, 'OracleFittedGP', BocaOracleFittedGP)
  return oracle_engine.patch_engine(monkeypatch)
