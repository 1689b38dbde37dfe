"""Run in a subprocess by tests/test_gpu_chol_paths.py with the factorisation's schedule switches set
in the environment (they are read once per process): factors SPD matrices of assorted sizes -- single
and as lock-step batches through the tuning objective -- and compares with LAPACK / one-at-a-time
fits.  Then the factor bit for bit: a second set of matrices, built by + - * / only so that their bytes do not depend
on the host's libm or BLAS, is factored and the SHA-256 of np.tril(L) compared with tests/golden/chol_factor_digests.npz,
keyed by (variant name, n) -- every sum on this path runs in a fixed order, so a schedule returns the same bits on
every run and a library that returns other bits has changed what it computes.  Prints OK on success.

    chol_paths_check.py [VARIANT]                 all checks; the digests of VARIANT (a name of test_gpu_chol_paths.VARIANTS)
    chol_paths_check.py --record FILE [VARIANT]   only factors the second set and writes its digests into FILE (created
                                                  or updated).  Record every variant twice into the same file: a pair
                                                  whose second digest differs from its first is stored empty -- it did
                                                  not reproduce and is not checked; such pairs are findings to report.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dragonfly_amd import general_utils as G                  # noqa: E402
from dragonfly_amd.engine import KernelSpec, get_engine       # noqa: E402
from oracle import ref_numpy as O                              # noqa: E402


def relerr(a, b):
  return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


SIZES = (513, 1024, 1100, 1536, 1601, 2048, 2500, 3100)
DIGESTS = os.path.join(ROOT, 'tests', 'golden', 'chol_factor_digests.npz')


def arith_matrix(n):
  """ SPD (a Cauchy kernel on n points of [0, 1] plus 0.05 I) from RandomState(n).rand(n) by + - * / only. """
  x = np.random.RandomState(n).rand(n)
  D = x[:, None] - x[None, :]
  return 1 / (1 + 25 * D * D) + 0.05 * np.eye(n)


def sha(a):
  return hashlib.sha256(np.ascontiguousarray(a, dtype='<f8').tobytes()).hexdigest()


def load_digests(path):
  if not os.path.exists(path):
    return {}
  with np.load(path) as z:
    return dict(zip((str(k) for k in z['keys']), (str(d) for d in z['digests'])))


def factor_digests(variant, record_to=None):
  """ Digest of M itself under 'input|n' (a differing input is not to be taken for a differing library), of
      np.tril(L) under 'variant|n'. """
  known = load_digests(record_to or DIGESTS)
  for n in SIZES:
    M = arith_matrix(n)
    L = G.stable_cholesky(M)
    for key, got in (('input|%d' % n, sha(M)), ('%s|%d' % (variant, n), sha(np.tril(L)))):
      print('%s %s' % (key, got))
      if record_to:
        known[key] = got if known.get(key, got) == got else ''
      elif known.get(key):        # (an empty digest: the pair did not reproduce when the file was recorded)
        assert known[key] == got, 'the bits of %s differ from tests/golden/chol_factor_digests.npz: %s, recorded %s' % (key, got, known[key])
      else:
        assert key in known, '%s is not in tests/golden/chol_factor_digests.npz' % key
  if record_to:
    keys = sorted(known)
    np.savez_compressed(record_to, keys=np.array(keys), digests=np.array([known[k] for k in keys]))


def main():
  eng = get_engine()
  if len(sys.argv) > 1 and sys.argv[1] == '--record':
    factor_digests(sys.argv[3] if len(sys.argv) > 3 else 'defaults', record_to=sys.argv[2])
    print('OK')
    return
  for n in SIZES:
    rs = np.random.RandomState(n)
    X = rs.rand(n, 4)
    M = O.se_kernel(X, X, 1.0, np.full(4, 0.4)) + 0.05 * np.eye(n)
    L = G.stable_cholesky(M)
    Lr = np.linalg.cholesky(M)
    assert relerr(L, Lr) < 1e-11 and np.array_equal(np.triu(L, 1), np.zeros_like(L)), n
  # failures inside full 512-panels: a negative pivot in the second strip of the third panel, a NaN
  # further down; the jitter ladder on a rank-deficient 1300 x 1300 matrix picks NumPy's power
  rs = np.random.RandomState(5)
  n = 1700
  X = rs.rand(n, 3)
  M = O.se_kernel(X, X, 1.0, np.full(3, 0.4)) + 0.05 * np.eye(n)
  for bad_at, bad_val in ((1100, -1.0), (40, -1.0), (1300, np.nan)):
    Mb = M.copy(); Mb[bad_at, bad_at] = bad_val
    try:
      G.stable_cholesky(Mb, add_to_diag_till_psd=False)
      raise AssertionError('no error for a bad pivot at %d' % bad_at)
    except np.linalg.LinAlgError as e:
      # the first failing pivot, 1-based; a NaN entry makes the first pivot whose column it reaches fail
      if bad_val < 0:
        assert 'pivot %d' % (bad_at + 1) in str(e), str(e)
  A = rs.randn(1300, 40)
  Mr = A.dot(A.T)
  L, p = eng.stable_cholesky(Mr, return_power=True)
  _, pr = O.stable_cholesky(Mr, return_power=True)
  assert p == pr and relerr(L.dot(L.T), Mr) < 1e-7, (p, pr)
  # lock-step batches: 9 candidate kernels on n = 1300 / 2200 points against single fits
  for n in (1300, 2200):
    rs = np.random.RandomState(n)
    d = 3
    X = rs.rand(n, d)
    Y = np.sin(4 * X.sum(axis=1)) + 0.1 * rs.randn(n)
    specs = [KernelSpec('se', d, float(Y.var()) * (0.5 + rs.rand()), 0.2 + 0.6 * rs.rand(d)) for _ in range(9)]
    means = [float(0.1 * rs.randn()) for _ in specs]
    noises = [float(Y.var() * (0.01 + 0.1 * rs.rand())) for _ in specs]
    lml = eng.gp_lml_batch(specs, X, Y, means, noises)
    for c in (0, 4, 8):
      one = eng.gp_fit(specs[c], X, Y - means[c], noises[c])
      assert abs(lml[c] - one.lml) <= 1e-11 * abs(one.lml), (n, c, lml[c], one.lml)
      one.free()
  factor_digests(sys.argv[1] if len(sys.argv) > 1 else 'defaults')
  print('OK')


if __name__ == '__main__':
  main()
