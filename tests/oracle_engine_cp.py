"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

tests/oracle_engine.py's CPU stand-in for the engine, extended to the Hamming kernel (DFH_KERNEL_HAMMING), to product
kernels with a Hamming factor (the reference's CartesianProductKernel over packed columns) and to fits with
handle_non_psd_kernels.  oracle_engine.py itself is left as it is: its module-level to_oracle_spec is wrapped for the
test's duration."""
import numpy as np

import oracle_engine


def hamming_matrix(w, A, B):
  """ (np.equal(x, y) * w).sum() for every pair of rows (general_utils.py:113-145), a row of B at a time as there """
  A, B = np.asarray(A, dtype=float), np.asarray(B, dtype=float)
  out = np.zeros((len(A), len(B)))
  for j, row in enumerate(B):
    out[:, j] = (np.equal(A, row) * w).sum(axis=1)
  return out


class HammingOracleKernel(object):
  def __init__(self, weights):
    self.w = np.asarray(weights, dtype=float)

  def __call__(self, X1, X2=None):
    return hamming_matrix(self.w, X1, X1 if X2 is None else X2)


class ProductOracleKernel(object):
  """ scale * prod_g k_g(X[:, group g]) in the reference's order (kernel.py:525-533), Hamming factors included """

  def __init__(self, spec, plain):
    self.scale, self.groups, self.subs = spec.scale, [list(g) for g in spec.groups], []
    for kind, grp, sc, nu, bw in zip(spec.sub_kinds, spec.groups, spec.sub_scales, spec.sub_nus, spec.sub_bandwidths):
      if kind == 'hamming':
        self.subs.append(HammingOracleKernel(bw))
      else:
        self.subs.append(plain(type(spec)(kind, len(grp), sc, bw, nu=nu)))

  def __call__(self, X1, X2=None):
    X2 = X1 if X2 is None else X2
    X1, X2 = np.asarray(X1, dtype=float), np.asarray(X2, dtype=float)
    K = self.scale * np.ones((len(X1), len(X2)))
    for kern, grp in zip(self.subs, self.groups):
      K *= kern(X1[:, grp], X2[:, grp])
    return K


def patch_engine_cp(monkeypatch):
  """ oracle_engine.patch_engine, with Hamming specs and projection fits understood """
  plain = oracle_engine.to_oracle_spec

  def to_spec(spec):
    if spec.kind == 'hamming':
      return HammingOracleKernel(spec.bandwidths)
    if spec.kind == 'product' and 'hamming' in spec.sub_kinds and getattr(spec, 'group_factors', None) is None:
      return ProductOracleKernel(spec, plain)
    return plain(spec)
  monkeypatch.setattr(oracle_engine, 'to_oracle_spec', to_spec)
  eng = oracle_engine.patch_engine(monkeypatch)
  from dragonfly_amd import cartesian_product_gp  # noqa: F401  pylint: disable=unused-import

  def gp_fit(spec, X, y_centred, noise_var, allow_jitter=True, handle_non_psd_kernels='guaranteed_psd'):
    return oracle_engine.OracleFittedGP(eng, spec, X, y_centred, noise_var, handle_non_psd_kernels=handle_non_psd_kernels)
  monkeypatch.setattr(eng, 'gp_fit', gp_fit, raising=False)
  def gp_lml_batch(specs, X, y, mean_consts, noise_vars, allow_jitter=True, return_powers=False,
                   handle_non_psd_kernels='guaranteed_psd'):
    if eng.lml_batch_sizes is not None:
      eng.lml_batch_sizes.append(len(specs))
    y = np.asarray(y, dtype=np.float64)
    return np.array([gp_fit(sp, X, y - c, nv, handle_non_psd_kernels=handle_non_psd_kernels).lml
                     for sp, c, nv in zip(specs, mean_consts, noise_vars)])
  monkeypatch.setattr(eng, 'gp_lml_batch', gp_lml_batch, raising=False)
  monkeypatch.setattr(eng, 'kernel_kinds', frozenset(['se', 'matern', 'poly', 'expdecay', 'hamming', 'additive', 'product', 'esp']),
                      raising=False)
  return eng
