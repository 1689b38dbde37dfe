"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

tests/oracle_engine_cp.py's CPU stand-in for the engine, extended to product descriptors whose factors are products
themselves (factor_sums == 2, DFH_FACTOR_PRODUCT: the joint kernel of a multi-fidelity GP on a Cartesian-product
domain).  nested_product_matrix is the NumPy restatement of the reference's order -- scale * ones, then *= per factor,
a factor being factor_scale * ones, then *= per part (kernel.py:525-533 inside itself) -- that the GPU tests hold the
device to as well."""
import numpy as np

import oracle_engine
import oracle_engine_cp
import oracle_engine_cp_acq


class NestedProductOracleKernel(object):
  """ scale * prod_f F_f, F_f = factor_scale_f * prod_{g in f} k_g for a product factor, the group's kernel for a plain one """

  def __init__(self, spec, plain):
    self.scale, self.groups, self.subs = spec.scale, [list(g) for g in spec.groups], []
    self.group_factors, self.factor_sums, self.factor_scales = list(spec.group_factors), list(spec.factor_sums), list(spec.factor_scales)
    if any(int(s) not in (0, 2) for s in self.factor_sums):
      raise ValueError('the stand-in knows plain and product factors beside each other, no additive ones')
    for kind, grp, sc, nu, bw in zip(spec.sub_kinds, spec.groups, spec.sub_scales, spec.sub_nus, spec.sub_bandwidths):
      if kind == 'hamming':
        self.subs.append(oracle_engine_cp.HammingOracleKernel(bw))
      else:
        self.subs.append(plain(type(spec)(kind, len(grp), sc, bw, nu=nu)))

  def __call__(self, X1, X2=None):
    X2 = X1 if X2 is None else X2
    X1, X2 = np.asarray(X1, dtype=float), np.asarray(X2, dtype=float)
    # a part's columns as the reference's np.array(list of points) holds them: row-major.  (X[:, columns] alone is
    # column-major, and a row sum over it adds the columns left to right instead of in NumPy's pairwise order -- what
    # the reference's Hamming kernel gets from eight columns on.)
    cols = lambda X, g: np.ascontiguousarray(X[:, self.groups[g]])
    K = self.scale * np.ones((len(X1), len(X2)))
    for f, mode in enumerate(self.factor_sums):
      members = [g for g, ff in enumerate(self.group_factors) if ff == f]
      if int(mode) == 0:
        g = members[0]
        K *= self.subs[g](cols(X1, g), cols(X2, g))
        continue
      F = self.factor_scales[f] * np.ones((len(X1), len(X2)))
      for g in members:
        F *= self.subs[g](cols(X1, g), cols(X2, g))
      K *= F
    return K


def nested_product_matrix(spec, X1, X2=None):
  """ the value of a nested product descriptor in the reference's order: every SE / Matern part by oracle/ref_numpy.py,
      every Hamming part by oracle_engine_cp.hamming_matrix """
  def part_kernel(sp):
    return oracle_engine_cp.HammingOracleKernel(sp.bandwidths) if sp.kind == 'hamming' else oracle_engine.to_oracle_spec(sp)
  return NestedProductOracleKernel(spec, part_kernel)(X1, X2)


def patch_engine_cpmf(monkeypatch):
  """ oracle_engine_cp_acq.patch_engine_cp_acq (fitted GPs with the fused calls of a product domain, every call counted
      in eng.calls), with product factors understood and Engine.join_fixed """
  eng = oracle_engine_cp_acq.patch_engine_cp_acq(monkeypatch)

  def join_fixed(z, cands):
    eng.calls['join_fixed'] = eng.calls.get('join_fixed', 0) + 1
    cands = np.asarray(cands, dtype=np.float64)
    return np.hstack((np.tile(np.asarray(z, dtype=np.float64).reshape(1, -1), (len(cands), 1)), cands))
  monkeypatch.setattr(eng, 'join_fixed', join_fixed, raising=False)
  cp_to_spec = oracle_engine.to_oracle_spec

  def to_spec(spec):
    sums = getattr(spec, 'factor_sums', None)
    if spec.kind == 'product' and sums is not None and any(int(s) == 2 for s in sums):
      return NestedProductOracleKernel(spec, cp_to_spec)
    return cp_to_spec(spec)
  monkeypatch.setattr(oracle_engine, 'to_oracle_spec', to_spec)
  return eng
