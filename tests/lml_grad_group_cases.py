"""What tests/test_gpu_lml_grad_groups.py and tests/test_lml_grad_groups_cpu.py share: additive and product kernels of
SE / Matern groups on the data of lml_grad_cases.make_case, the gradient of their log marginal likelihood in extended
precision (the truth), central differences of the truth's own lml, and the formula in NumPy double precision -- the
per-parameter derivative matrix and two triangular solves, distances as general_utils.py:62-70 -- whose distance from
the truth sets the bound exactly as lml_grad_cases.gradient_bound does.  Coordinates, as dfh_gp_lml_grad_groups:
[d/d log scale, d/d log bandwidth of every column of every group in the groups' order, d/d log noise_var, d/d mean].
A group's own scale (sub_scale) enters the value and is not differentiated."""
import numpy as np

import lml_grad_cases as base

LD = np.longdouble
SUB_SCALES = (1.25, 0.8, 1.1)            # group g's own scale: SUB_SCALES[g % 3]


class GroupCase(object):
  """ family 'additive' | 'product'; groups: columns per group; kinds: (kind, nu) per group; data: a make_case dict """

  def __init__(self, family, groups, kinds, data):
    assert len(groups) == len(kinds)
    self.family, self.groups, self.kinds, self.data = family, [list(g) for g in groups], list(kinds), data
    self.sub_scales = [SUB_SCALES[g % 3] for g in range(len(groups))]
    self.columns = [c for grp in self.groups for c in grp]           # flattened position -> input column
    self.bws = np.asarray(data['bw'], dtype=float)[self.columns]     # flattened position -> bandwidth

  def spec(self):
    from dragonfly_amd.engine import KernelSpec
    d = self.data['X'].shape[1]
    return KernelSpec(self.family, d, self.data['scale'], groups=self.groups, sub_kinds=[k for k, _ in self.kinds],
                      sub_scales=self.sub_scales, sub_nus=[nu for _, nu in self.kinds],
                      sub_bandwidths=[np.asarray(self.data['bw'], dtype=float)[grp] for grp in self.groups])

  def moved(self, **changes):
    data = dict(self.data)
    data.update(changes)
    return GroupCase(self.family, self.groups, self.kinds, data)


SE, M05, M15, M25 = ('se', 0.0), ('matern', 0.5), ('matern', 1.5), ('matern', 2.5)


def _three(n, **kwargs):
  return base.make_case(n, 5, 21, 1e-2, **kwargs)


def make(name):
  """ the named cases; the first nine are the ones the formula in double holds to the flat 1e-10 """
  if name == 'additive_n70':
    return GroupCase('additive', [[0, 1], [2], [3, 4]], [SE, M25, M15], _three(70))
  if name == 'product_n70':
    return GroupCase('product', [[0, 1], [2, 3, 4]], [SE, M25], _three(70))
  if name == 'product3_n70':
    return GroupCase('product', [[0], [1, 2], [3, 4]], [M05, SE, M25], _three(70))
  if name == 'additive_permuted_n70':
    return GroupCase('additive', [[4, 0], [5, 2], [1, 3]], [SE, SE, SE], base.make_case(70, 6, 21, 1e-2))
  if name == 'additive_20groups_n130':
    return GroupCase('additive', [[2 * g, 2 * g + 1] for g in range(20)], [SE if g % 2 == 0 else M25 for g in range(20)],
                     base.make_case(130, 40, 21, 1e-2))
  if name == 'additive_n513':
    return GroupCase('additive', [[0, 1], [2], [3, 4]], [SE, M25, M15], _three(513))
  if name == 'product_n513':
    return GroupCase('product', [[0, 1], [2, 3, 4]], [SE, M25], _three(513))
  if name == 'additive_n1030':
    return GroupCase('additive', [[0, 1], [2, 3]], [SE, M25], base.make_case(1030, 4, 21, 1e-2))
  if name == 'additive_dup_nu05':
    return GroupCase('additive', [[0, 1], [2], [3, 4]], [SE, M05, M15], _three(70, dup=True))
  # bounded by the rule alone
  if name == 'additive_wide_n70':          # a group past one 16-column chunk beside a padded one
    return GroupCase('additive', [list(range(17)), [17, 18, 19]], [SE, M25], base.make_case(70, 20, 21, 1e-2))
  if name == 'product_wide_n70':
    return GroupCase('product', [list(range(17)), [17, 18, 19]], [SE, M25], base.make_case(70, 20, 21, 1e-2))
  if name == 'product_jitter':             # noise 0, two rows 1e-9 apart: the fit takes jitter
    return GroupCase('product', [[0, 1], [2]], [SE, SE], base.make_case(70, 3, 13, 0.0, near_dup=1e-9))
  if name == 'product_dup_nu05':
    return GroupCase('product', [[0, 1], [2], [3, 4]], [SE, M05, M15], _three(70, dup=True))
  raise KeyError(name)


FLAT = ['additive_n70', 'product_n70', 'product3_n70', 'additive_permuted_n70', 'additive_20groups_n130', 'additive_n513',
        'product_n513', 'additive_n1030', 'additive_dup_nu05']


# ---- the truth ------------------------------------------------------------------------------------------------------
def _parts_ld(case):
  """ per group (K_g, dK_g / d(dsq_g)) with the group's own scale, and S[c] per input column """
  X, bw = case.data['X'].astype(LD), case.data['bw'].astype(LD)
  S = {c: ((X[:, None, c] - X[None, :, c]) / bw[c]) ** 2 for c in case.columns}
  parts = [base._kernel_parts_ld(kind, nu, LD(s), np.stack([S[c] for c in grp]))      # pylint: disable=protected-access
           for grp, (kind, nu), s in zip(case.groups, case.kinds, case.sub_scales)]
  return parts, S


def _combine(case, parts, one=None):
  """ K, and per group the factor in front of S_c: scale dK_g (additive), scale prod_{h != g} K_h dK_g (product) """
  one = LD(1) if one is None else one
  scale = one * case.data['scale']
  if case.family == 'additive':
    K = scale * sum(Kg for Kg, _ in parts)
    return K, [scale * dKg for _, dKg in parts]
  K = scale * np.prod([Kg for Kg, _ in parts], axis=0)
  front = []
  for g, (_, dKg) in enumerate(parts):
    others = one
    for h, (Kh, _) in enumerate(parts):
      if h != g:
        others = others * Kh
    front.append(scale * others * dKg)
  return K, front


def truth(case, jitter=0.0):
  """ (gradient, lml) of K + (noise + jitter) I in extended precision """
  parts, S = _parts_ld(case)
  K, front = _combine(case, parts)
  n = len(K)
  yc = case.data['y'].astype(LD) - LD(case.data['mean'])
  A = K + (LD(case.data['noise']) + LD(jitter)) * np.eye(n, dtype=LD)
  L = base._chol_ld(A)                                     # pylint: disable=protected-access
  Ainv = base._spd_inv_from_factor_ld(L)                   # pylint: disable=protected-access
  alpha = Ainv.dot(yc)
  W = np.outer(alpha, alpha) - Ainv
  Q = len(case.columns)
  g = np.zeros(Q + 3, dtype=LD)
  g[0] = (W * K).sum() / 2
  q = 0
  for grp, fr in zip(case.groups, front):
    Wf = W * fr
    for c in grp:
      g[1 + q] = (Wf * (-2 * S[c])).sum() / 2
      q += 1
  g[Q + 1] = LD(case.data['noise']) * np.trace(W) / 2
  g[Q + 2] = alpha.sum()
  lml = -yc.dot(alpha) / 2 - np.log(np.diag(L)).sum() - LD(n) * np.log(2 * LD(np.pi)) / 2
  return g, lml


def truth_lml(case):
  parts, _ = _parts_ld(case)
  K, _ = _combine(case, parts)
  n = len(K)
  yc = case.data['y'].astype(LD) - LD(case.data['mean'])
  L = base._chol_ld(K + LD(case.data['noise']) * np.eye(n, dtype=LD))        # pylint: disable=protected-access
  z = base._tri_inv_ld(L).dot(yc)                                            # pylint: disable=protected-access
  return -z.dot(z) / 2 - np.log(np.diag(L)).sum() - LD(n) * np.log(2 * LD(np.pi)) / 2


def central_differences(case, h=1e-4):
  """ the gradient by central differences of the truth's own lml, in the same coordinates """
  Q = len(case.columns)
  g = np.zeros(Q + 3, dtype=LD)

  def moved(idx, step):
    if idx == 0:
      return case.moved(scale=case.data['scale'] * np.exp(step))
    if idx <= Q:
      bw = case.data['bw'].astype(LD).copy()
      bw[case.columns[idx - 1]] *= np.exp(LD(step))
      return case.moved(bw=bw)
    if idx == Q + 1:
      return case.moved(noise=case.data['noise'] * np.exp(step))
    return case.moved(mean=case.data['mean'] + step)
  for idx in range(Q + 3):
    g[idx] = (truth_lml(moved(idx, h)) - truth_lml(moved(idx, -h))) / (2 * LD(h))
  return g


# ---- the formula in NumPy double precision ----------------------------------------------------------------------------
def _parts_double(case):
  """ per group (K_g, dK_g / d(dsq_g)) in double, distances by the expansion (general_utils.py:62-70); a bandwidth's
      derivative is 0 where the group's distance is, as lml_grad_cases.reference_formula has it """
  X, bw = case.data['X'], np.asarray(case.data['bw'], dtype=float)
  parts = []
  for grp, (kind, nu), s in zip(case.groups, case.kinds, case.sub_scales):
    Xs = X[:, grp] / bw[grp]
    dsq = base._dist_squared(Xs, Xs)                       # pylint: disable=protected-access
    if kind == 'se':
      K = s * np.exp(-dsq / 2)
      dK = -K / 2
    else:
      p = int(nu)
      dist = np.sqrt(dsq)
      safe = np.where(dist == 0, 1.0, dist)
      s2 = np.sqrt(2 * nu)
      e = np.exp(-s2 * dist)
      if p == 0:
        K, dKd = s * e, -s * s2 * e
      elif p == 1:
        K, dKd = s * (1 + s2 * dist) * e, -s * s2 * s2 * dist * e
      else:
        K, dKd = s * (1 + s2 * dist + s2 * s2 * dsq / 3) * e, -s * (s2 * s2 / 3) * dist * (1 + s2 * dist) * e
      dK = np.where(dist == 0, 0.0, dKd / (2 * safe))
    parts.append((K, dK))
  return parts


def double_formula(case, jitter=0.0):
  """ 1/2 tr(alpha alpha^T G - A^-1 G) per parameter, G the derivative matrix of K in it, two triangular solves each """
  from scipy.linalg import solve_triangular
  X, bw = case.data['X'], np.asarray(case.data['bw'], dtype=float)
  n = len(X)
  yc = case.data['y'] - case.data['mean']
  K, front = _combine(case, _parts_double(case), one=1.0)
  L = np.linalg.cholesky(K + (case.data['noise'] + jitter) * np.eye(n))
  alpha = solve_triangular(L.T, solve_triangular(L, yc, lower=True), lower=False)

  def half_trace(G):
    return 0.5 * np.trace(np.outer(alpha, alpha.dot(G)) - solve_triangular(L.T, solve_triangular(L, G, lower=True), lower=False))
  Q = len(case.columns)
  g = np.zeros(Q + 3)
  g[0] = half_trace(K)
  q = 0
  for grp, fr in zip(case.groups, front):
    for c in grp:
      xc = X[:, c:c + 1] / bw[c]
      g[1 + q] = half_trace(fr * (-2 * base._dist_squared(xc, xc)))       # pylint: disable=protected-access
      q += 1
  g[Q + 1] = half_trace(case.data['noise'] * np.eye(n))
  g[Q + 2] = alpha.sum()
  return g


def nwise(got, want):
  """ norm-wise distance against max|want|, in extended precision """
  want = np.asarray(want, dtype=LD)
  return float(np.max(np.abs(np.asarray(got, dtype=LD) - want)) / np.max(np.abs(want)))


def gradient_bound(case, true_grad, jitter=0.0, floor=1e-10):
  """ max(1e-10, twice the norm-wise distance of the formula in double precision from the truth) """
  dist = nwise(double_formula(case, jitter), true_grad)
  return max(floor, 2.0 * dist), dist


_TRUTHS = {}


def truth_and_bound(name, jitter=0.0):
  """ (case, true gradient, true lml, bound, distance of the double formula), computed once per case and jitter """
  key = (name, jitter)
  if key not in _TRUTHS:
    case = make(name)
    true_grad, lml = truth(case, jitter)
    bound, dist = gradient_bound(case, true_grad, jitter)
    true_grad.setflags(write=False)
    _TRUTHS[key] = (case, true_grad, lml, bound, dist)
  return _TRUTHS[key]


# ---- the mirror's GPs on a case ------------------------------------------------------------------------------------
def _sub_kernel(kind, nu, scale, bws):
  from dragonfly_amd import kernel as K
  return K.SEKernel(len(bws), scale, bws) if kind == 'se' else K.MaternKernel(len(bws), nu, scale, bws)


def _sub_kernels(case):
  bw = np.asarray(case.data['bw'], dtype=float)
  return [_sub_kernel(kind, nu, s, bw[grp]) for grp, (kind, nu), s in zip(case.groups, case.kinds, case.sub_scales)]


def additive_mirror_gp(case):
  from dragonfly_amd import kernel as K
  from dragonfly_amd.euclidean_gp import EuclideanGP
  from dragonfly_amd.gp_core import ConstantMean
  kern = K.AdditiveKernel(case.data['scale'], _sub_kernels(case), case.groups)
  return EuclideanGP(case.data['X'], case.data['y'], kern, ConstantMean(case.data['mean']), case.data['noise'])


def mf_mirror_gp(case, domain_kernel=None):
  """ the two-factor product case as a multi-fidelity GP: group 0 the fidelity space, group 1 the domain """
  from dragonfly_amd.gp_core import ConstantMean
  from dragonfly_amd.mf_gp import EuclideanMFGP
  fidel, domain = case.groups
  assert fidel + domain == list(range(len(fidel) + len(domain)))
  kf, kd = _sub_kernels(case)
  X = case.data['X']
  return EuclideanMFGP(list(X[:, fidel]), list(X[:, domain]), list(case.data['y']), None, case.data['scale'], kf,
                       kd if domain_kernel is None else domain_kernel, ConstantMean(case.data['mean']), case.data['noise'])


def named_components(gp, case, names):
  """ compute_grad_log_marginal_likelihood for scale, every bandwidth under its name, noise_var, noise_mean -- and what
      the truth says each is: its component, a bandwidth's divided by the bandwidth """
  got = [gp.compute_grad_log_marginal_likelihood('scale')]
  got += [gp.compute_grad_log_marginal_likelihood(name, c) for name, c in names]
  got += [gp.compute_grad_log_marginal_likelihood('noise_var'), gp.compute_grad_log_marginal_likelihood('noise_mean')]
  return np.array(got)


def wanted(case, true_grad):
  want = np.array(true_grad, dtype=np.longdouble)
  want[1:-2] /= case.bws
  return want
