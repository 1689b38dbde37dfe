"""TEST INFRASTRUCTURE ONLY -- never imported by the product.

tests/oracle_engine.py's CPU stand-in for the engine, extended to the ESP kernel (DFH_KERNEL_ESP): a KernelSpec of kind
'esp' is evaluated by the reference's formula (dragonfly/gp/kernel.py:693-726) over the oracle's 1-D SE / Matern
kernels.  oracle_engine.py itself is left as it is: its module-level to_oracle_spec is wrapped for the test's duration."""
import numpy as np

import oracle_engine
from oracle import ref_numpy as O


class ESPOracleKernel(object):
  """ scale * e_order of the columns' 1-D kernels, Newton-Girard from the power sums in the reference's order """

  def __init__(self, spec):
    self.scale, self.order = spec.scale, int(spec.nu)
    self.cols = [(kind, sc, nu, float(np.ravel(bw)[0]))
                 for kind, sc, nu, bw in zip(spec.sub_kinds, spec.sub_scales, spec.sub_nus, spec.sub_bandwidths)]

  def __call__(self, X1, X2=None):
    X2 = X1 if X2 is None else X2
    X1, X2 = np.asarray(X1, dtype=float), np.asarray(X2, dtype=float)
    mats = []
    for c, (kind, sc, nu, bw) in enumerate(self.cols):
      A, B = X1[:, c:c + 1], X2[:, c:c + 1]
      mats.append(O.se_kernel(A, B, sc, np.array([bw])) if kind == 'se' else O.matern_kernel(A, B, nu, sc, np.array([bw])))
    return newton_girard(mats, self.order, self.scale)


def newton_girard(mats, order, scale):
  """ kernel.py:709-726 on the columns' kernel matrices """
  n1, n2 = mats[0].shape
  ones = np.ones((n1, n2))
  power_sum = [ones] + [np.zeros((n1, n2)) for _ in range(order)]
  for i in range(1, order + 1):
    for matrix in mats:
      power_sum[i] += matrix ** i
  esp = [ones] + [np.zeros((n1, n2)) for _ in range(order)]
  for m in range(1, order + 1):
    for i in range(1, m + 1):
      esp[m] += ((-1) ** (i - 1)) * esp[m - i] * power_sum[i]
    esp[m] /= m
  return scale * esp[order]


def patch_engine_esp(monkeypatch):
  """ oracle_engine.patch_engine, with ESP specs understood """
  plain = oracle_engine.to_oracle_spec
  monkeypatch.setattr(oracle_engine, 'to_oracle_spec',
                      lambda spec: ESPOracleKernel(spec) if spec.kind == 'esp' else plain(spec))
  return oracle_engine.patch_engine(monkeypatch)
