"""What tests/test_gpu_lml_grad.py and tests/test_lml_grad_cpu.py share: the cases, the gradient of the log marginal
likelihood in extended precision (the truth), and the reference's formula (gp_core.py:229-240 with kernel.py's
gradient methods) evaluated in NumPy double precision -- whose distance from the truth sets the tolerance, as
tests/truth_bounds.py does for the posterior.  Everything is in the tuner's coordinates:
[d/d log scale, d/d log bw_0 .. d/d log bw_{d-1}, d/d log noise_var, d/d constant mean]."""
import numpy as np

LD = np.longdouble


def make_case(n, d, seed, noise, near_dup=0.0, dup=False):
  """ inputs in the unit cube, labels of a smooth function plus a little noise; bandwidths around 0.5.
      near_dup: row 1 = row 0 + near_dup in every column, with row 0's label; dup: row 3 = row 2 exactly """
  rs = np.random.RandomState(seed)
  X = rs.random_sample((n, d))
  if near_dup:
    X[1] = X[0] + near_dup
  if dup:
    X[3] = X[2]
  y = np.sin(3.0 * X[:, :3].sum(axis=1)) + X[:, -1] ** 2 + 0.05 * rs.standard_normal(n)
  if near_dup:
    # the same label on both rows (a repeated measurement): with different labels and no noise, alpha of the pair is
    # (y_0 - y_1) / (2 jitter) ~ 1e9 and the gradient hangs on K_00 + K_11 - 2 K_01 ~ 1e-18, below what ANY double
    # evaluation resolves -- the reference's formula in double would then measure chance, not a rounding scale
    y[1] = y[0]
  bw = 0.35 + 0.4 * rs.random_sample(d)
  if d > 8:
    bw = bw * np.sqrt(d / 3.0)      # keep the distances, and with them the condition number, those of d = 3
  return dict(X=X, y=y, bw=bw, scale=1.3, noise=noise, mean=float(np.mean(y)))


# ---- the truth: np.longdouble throughout, direct-difference distances, its own Cholesky and inverse -------------
def _chol_ld(A):
  n = len(A)
  L = np.zeros((n, n), dtype=LD)
  for j in range(n):
    v = A[j:, j] - L[j:, :j].dot(L[j, :j])
    L[j, j] = np.sqrt(v[0])
    L[j + 1:, j] = v[1:] / L[j, j]
  return L


def _tri_inv_ld(L):
  """ inverse of a lower-triangular matrix, row by row: M[i] = (e_i - L[i, :i] M[:i]) / L[i, i] """
  n = len(L)
  M = np.zeros((n, n), dtype=LD)
  for i in range(n):
    M[i, :i] = -L[i, :i].dot(M[:i, :i])
    M[i, i] = LD(1)
    M[i, :i + 1] /= L[i, i]
  return M


def _spd_inv_from_factor_ld(L, nb=128):
  """ (L L^T)^-1 = M^T M with M = L^-1, block by block: M is lower triangular, so block (bi, bj), bj <= bi, only sums
      over the rows from block bi on """
  M = _tri_inv_ld(L)
  n = len(L)
  Ainv = np.zeros((n, n), dtype=LD)
  for i0 in range(0, n, nb):
    Mi = M[i0:, i0:i0 + nb].T
    for j0 in range(0, i0 + 1, nb):
      blk = Mi.dot(M[i0:, j0:j0 + nb])
      Ainv[i0:i0 + nb, j0:j0 + nb] = blk
      Ainv[j0:j0 + nb, i0:i0 + nb] = blk.T
  return Ainv


def _kernel_parts_ld(kind, nu, scale, S):
  """ K and dK/d(dsq) (0 where dsq = 0: the limit of dK/d(dsq) * s_c) from S[c] = ((x_ic - x_jc) / bw_c)^2 """
  dsq = S.sum(axis=0)
  zero = dsq == 0
  if kind == 'se':
    K = scale * np.exp(-dsq / 2)
    dK = -K / 2
  else:
    p = int(nu)
    dist = np.sqrt(dsq)
    safe = np.where(zero, LD(1), dist)
    s2 = np.sqrt(LD(2) * LD(nu))
    e = np.exp(-s2 * dist)
    if p == 0:
      K, dKd = scale * e, -scale * s2 * e
    elif p == 1:
      K, dKd = scale * (1 + s2 * dist) * e, -scale * s2 * s2 * dist * e
    elif p == 2:
      K = scale * (1 + s2 * dist + s2 * s2 * dsq / 3) * e
      dKd = -scale * (s2 * s2 / 3) * dist * (1 + s2 * dist) * e
    else:
      raise ValueError('nu')
    dK = dKd / (2 * safe)
  return K, np.where(zero, LD(0), dK)


def truth(kind, nu, case, jitter=0.0):
  """ (gradient, lml) of K + (noise + jitter) I in extended precision """
  X, bw = case['X'].astype(LD), case['bw'].astype(LD)
  n, d = X.shape
  yc = case['y'].astype(LD) - LD(case['mean'])
  S = np.stack([((X[:, None, c] - X[None, :, c]) / bw[c]) ** 2 for c in range(d)])
  K, dK = _kernel_parts_ld(kind, nu, LD(case['scale']), S)
  A = K + (LD(case['noise']) + LD(jitter)) * np.eye(n, dtype=LD)
  L = _chol_ld(A)
  Ainv = _spd_inv_from_factor_ld(L)
  alpha = Ainv.dot(yc)
  W = np.outer(alpha, alpha) - Ainv
  g = np.zeros(d + 3, dtype=LD)
  g[0] = (W * K).sum() / 2
  WdK = W * dK
  for c in range(d):
    g[1 + c] = (WdK * (-2 * S[c])).sum() / 2
  g[d + 1] = LD(case['noise']) * np.trace(W) / 2
  g[d + 2] = alpha.sum()
  lml = -yc.dot(alpha) / 2 - np.log(np.diag(L)).sum() - LD(n) * np.log(2 * LD(np.pi)) / 2
  return g, lml


def truth_lml(kind, nu, case, jitter=0.0):
  X, bw = case['X'].astype(LD), case['bw'].astype(LD)
  n, d = X.shape
  yc = case['y'].astype(LD) - LD(case['mean'])
  S = np.stack([((X[:, None, c] - X[None, :, c]) / bw[c]) ** 2 for c in range(d)])
  K, _ = _kernel_parts_ld(kind, nu, LD(case['scale']), S)
  L = _chol_ld(K + (LD(case['noise']) + LD(jitter)) * np.eye(n, dtype=LD))
  M = _tri_inv_ld(L)
  z = M.dot(yc)
  return -z.dot(z) / 2 - np.log(np.diag(L)).sum() - LD(n) * np.log(2 * LD(np.pi)) / 2


def central_differences(kind, nu, case, h=1e-4):
  """ the gradient by central differences of the truth's own lml, in the same coordinates """
  d = case['X'].shape[1]
  g = np.zeros(d + 3, dtype=LD)
  def moved(idx, step):
    c = dict(case)
    if idx == 0:
      c['scale'] = case['scale'] * np.exp(step)
    elif idx <= d:
      c['bw'] = case['bw'].astype(LD).copy()
      c['bw'][idx - 1] = c['bw'][idx - 1] * np.exp(LD(step))
    elif idx == d + 1:
      c['noise'] = case['noise'] * np.exp(step)
    else:
      c['mean'] = case['mean'] + step
    return c
  for idx in range(d + 3):
    g[idx] = (truth_lml(kind, nu, moved(idx, h)) - truth_lml(kind, nu, moved(idx, -h))) / (2 * LD(h))
  return g


# ---- the reference's formula in NumPy double precision ------------------------------------------------------------
def _dist_squared(X1, X2):
  """ general_utils.py:62-70 """
  n1sq = (X1 ** 2).sum(axis=1)
  n2sq = (X2 ** 2).sum(axis=1)
  return np.clip(np.outer(n1sq, np.ones(len(X2))) + np.outer(np.ones(len(X1)), n2sq) - 2 * X1.dot(X2.T), 0.0, np.inf)


def reference_formula(kind, nu, case, jitter=0.0):
  """ gp_core.py:229-240: 1/2 tr(alpha alpha^T G - A^-1 G) per parameter with two triangular solves, G the kernel's
      derivative matrix in the parameter (kernel.py:202-217, 301-322, turned to log bandwidths); dsq = 0 entries of a
      bandwidth's G are 0, as the reference's fill_diagonal makes the diagonal's. """
  from scipy.linalg import solve_triangular
  X, bw = case['X'], case['bw']
  n, d = X.shape
  yc = case['y'] - case['mean']
  Xs = X / bw
  dsq = _dist_squared(Xs, Xs)
  scale = case['scale']
  if kind == 'se':
    K = scale * np.exp(-dsq / 2)
    dK = -K / 2
  else:
    p = int(nu)
    dist = np.sqrt(dsq)
    safe = np.where(dist == 0, 1.0, dist)
    s2 = np.sqrt(2 * nu)
    e = np.exp(-s2 * dist)
    if p == 0:
      K, dKd = scale * e, -scale * s2 * e
    elif p == 1:
      K, dKd = scale * (1 + s2 * dist) * e, -scale * s2 * s2 * dist * e
    else:
      K, dKd = scale * (1 + s2 * dist + s2 * s2 * dsq / 3) * e, -scale * (s2 * s2 / 3) * dist * (1 + s2 * dist) * e
    dK = np.where(dist == 0, 0.0, dKd / (2 * safe))
  L = np.linalg.cholesky(K + (case['noise'] + jitter) * np.eye(n))
  alpha = solve_triangular(L.T, solve_triangular(L, yc, lower=True), lower=False)

  def half_trace(G):
    return 0.5 * np.trace(np.outer(alpha, alpha.dot(G)) - solve_triangular(L.T, solve_triangular(L, G, lower=True), lower=False))
  g = np.zeros(d + 3)
  g[0] = half_trace(K)
  for c in range(d):
    sc = _dist_squared(Xs[:, c:c + 1], Xs[:, c:c + 1])
    g[1 + c] = half_trace(dK * (-2 * sc))
  g[d + 1] = half_trace(case['noise'] * np.eye(n))
  g[d + 2] = alpha.sum()
  return g


def gradient_bound(kind, nu, case, true_grad, jitter=0.0, floor=1e-10):
  """ max(1e-10, twice the norm-wise distance of the reference's formula in double precision from the truth) """
  ref = reference_formula(kind, nu, case, jitter)
  dist = float(np.max(np.abs(ref.astype(LD) - true_grad)) / np.max(np.abs(true_grad)))
  return max(floor, 2.0 * dist), dist


def condition_number(kind, nu, case, jitter=0.0):
  # (the double matrix is enough for a figure that is only printed)
  X, bw = case['X'], case['bw']
  dsq = _dist_squared(X / bw, X / bw)
  if kind == 'se':
    K = case['scale'] * np.exp(-dsq / 2)
  else:
    dist, s2 = np.sqrt(dsq), np.sqrt(2 * nu)
    poly = {0: 1.0, 1: 1 + s2 * dist, 2: 1 + s2 * dist + s2 * s2 * dsq / 3}[int(nu)]
    K = case['scale'] * poly * np.exp(-s2 * dist)
  return float(np.linalg.cond(K + (case['noise'] + jitter) * np.eye(len(X))))
