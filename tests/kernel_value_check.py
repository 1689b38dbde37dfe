"""Case table, truth and checks of the device's kernel VALUES, element by element in ulps, on every route of the
kernel-matrix builder (tests/test_gpu_kernel_values.py on the device, tests/test_kernel_values_cpu.py for the
reference side), and the z sweep of the acquisition epilogue.

Exact-argument inputs.  Every coordinate is k 2^-q with an integer k and every bandwidth a power of two, so a scaled
coordinate is an integer s times 2^-E.  lattice_ints asserts, in integers, 4 max_row sum s^2 < 2^53: then every
partial sum of every row norm and dot product is an integer below 2^53 (times 2^-2E) and exact in fp64 in any order,
on the matrix cores included, and dsq = (|a|^2 + |b|^2) - 2 a.b is the same exact number on every route.  It is
computed here in int64.  What is left in K[i][j] is the error of the device's exp, sqrt and polynomial code.

Truth: scale k(dsq) in numpy.longdouble (x87: eps 1.1e-19) from the integer dsq, following kernel.py:171-177, 259-299;
additive / product kernels from the parts' truths; the ESP kernel by the all-positive recurrence e_m += k_c e_{m-1}.
Metric: |value - truth| / spacing(double(truth)) -- 2^-1074 where the truth is subnormal or rounds to 0 -- divided by
1 + max_part arg (arg = sqrt(2 nu) dist: the conditioning of exp(-arg) under a rounded arg) where a Matern part is in.
Bound: max(2, 2 x the figure of oracle/ref_numpy.py on the same inputs), never anything the device returned.  The
floor of 2 ulp is what the source claims for itself: 0.7 ulp polynomial + 0.5 ulp scale + 0.5 ulp ldexp into a
subnormal.  The bound is taken per region of a case, 'head' and 'tail': in the tail (a part's arg above 693, its
exponential below 2^-1000) the reference rounds gfac exp(-arg) into a subnormal BEFORE the Matern polynomial multiplies
it, which costs it up to 0.5 u(mult) units of 2^-1074 -- 1.4e3 (1 + arg) ulp at nu = 2.5, 2e6 at nu = 3.5 -- and one
bound for the whole case would allow the head that much too.  Each region's bound is at most the case's.

Each case names the route it was written for (Engine.counters()['km_route']) and fails when the dispatch books another.

    kernel_value_check.py --variant NAME [--json FILE]   the cases of one variant (the caller sets its switches: they are
                                                         read once per process); prints OK
    kernel_value_check.py --all --json FILE              every variant, each in a child process with a time limit, and
                                                         the acquisition sweep; FILE collects the measured figures
"""
import collections
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
  if _p not in sys.path:
    sys.path.insert(0, _p)
from dragonfly_amd.engine import KernelSpec      # noqa: E402
import oracle_engine                             # noqa: E402
import oracle_engine_esp                         # noqa: E402

LD = np.longdouble
FLOOR_ULP = 2.0
MIN_NORMAL = 2.0 ** -1022
TAIL_ARG = 693.0                      # a part's exp(-arg) below 2^-1000: the 'tail' region of a case
BAND_MIN = 50                         # entries the truth of an SE / Matern case has in each band
BANDS = ('arg_below_1', 'normal', 'subnormal', 'zero')
ROUTES = ('sym', 'cross_lds', 'strip', 'strip_mean', 'symmulti', 'generic', 'esp', 'colw')
VARIANTS = {'default': {}, 'cfg1': {'DFH_KM_CFG': '1'}, 'cfg2': {'DFH_KM_CFG': '2'}, 'strip0': {'DFH_KM_STRIP': '0'},
            'symmulti0': {'DFH_KM_SYMMULTI': '0'}}
CHILD_TIMEOUT = 120

# kind of spec: builder(bw_exp) -> KernelSpec with bandwidth 2^bw_exp(c) on column c.  Scales are no powers of two:
# the strip kernel folds the scale into its polynomial coefficients, which a power of two would not test.
Case = collections.namedtuple('Case', 'variant route tag kernel d n1 n2 q span')      # n1 == 0: symmetric, n2 rows


def case_id(c):
  shape = 'sym%d' % c.n2 if not c.n1 else 'cross%dx%d' % (c.n1, c.n2)
  return '%s-%s-%s-d%d-%s' % (c.variant, c.route, c.tag, c.d, shape)


def _bw_exp(c):
  return (c % 3) - 1               # bandwidths 0.5, 1, 2, 0.5, ...


def spec_of(kernel, d, bw_exp=_bw_exp):
  bw = lambda cols: np.array([2.0 ** bw_exp(c) for c in cols])
  if kernel == 'se':
    return KernelSpec('se', d, 0.7, bw(range(d)))
  if kernel.startswith('m'):                                    # 'm25': Matern nu = 2.5
    return KernelSpec('matern', d, 0.9, bw(range(d)), nu=int(kernel[1:]) / 10.0)
  if kernel in ('add', 'prod'):
    groups = [[0, 1, 2], [3, 4]]
    return KernelSpec('additive' if kernel == 'add' else 'product', d, 1.5, groups=groups, sub_kinds=['se', 'matern'],
                      sub_scales=[1.25, 0.8], sub_nus=[0.0, 2.5], sub_bandwidths=[bw(g) for g in groups])
  if kernel.startswith('esp'):                                  # 'esp3' / 'esp3m': order 3 / with a Matern-2.5 column 1
    order, with_matern = int(kernel[3:].rstrip('m')), kernel.endswith('m')
    kinds = ['matern' if (with_matern and c == 1) else 'se' for c in range(d)]
    return KernelSpec('esp', d, 1.5, nu=order, sub_kinds=kinds, sub_scales=[1.0] * d,      # (ESPKernelSE / Matern: 1-D scales 1)
                      sub_nus=[2.5 if k == 'matern' else 0.0 for k in kinds], sub_bandwidths=[bw([c]) for c in range(d)])
  raise ValueError(kernel)


def parts_of(spec):
  """ [(kind, scale, nu, columns, bandwidths)] of the stationary parts """
  if spec.kind in ('se', 'matern'):
    return [(spec.kind, spec.scale, spec.nu, list(range(spec.dim)), np.asarray(spec.bandwidths))]
  return [(k, s, nu, list(g), np.ravel(np.asarray(b, dtype=float)))
          for k, s, nu, g, b in zip(spec.sub_kinds, spec.sub_scales, spec.sub_nus, spec.groups, spec.sub_bandwidths)]


def has_matern(spec):
  return any(p[0] == 'matern' for p in parts_of(spec))


# ---- inputs -------------------------------------------------------------------------------------------------------
def lattice_points(seed, n, d, q, span):
  """ n points of the lattice 2^-q Z^d within [-span, span]^d: a third of them at log-uniform radii around the origin
      (pairs at every small distance: arg < 1 and the middle range), the rest uniform in the cube (the tails).
      Integer arithmetic and RandomState integers only: the same bytes on every host. """
  rs = np.random.RandomState(seed)
  top = int(span * 2 ** q)
  k = rs.randint(-top, top + 1, size=(n, d)).astype(np.int64)
  near = np.arange(n) % 3 == 0
  shift = rs.randint(0, max(1, int(math.log2(top)) + 1), size=n)           # radius ~ top / 2^shift
  k[near] = k[near] >> shift[near][:, None]
  return k.astype(np.float64) / 2.0 ** q


def far_points(n, d, first, spec):
  """ integer points: the first column of every part holds the row number (from `first`), so any two rows differ by
      at least 1 in every part; the other columns hold -1, 0, 1 """
  rows = first + np.arange(n, dtype=np.float64)
  X = (rows[:, None] + np.arange(d)[None, :]) % 3 - 1.0
  for part in parts_of(spec):
    X[:, part[3][0]] = rows
  return X


def inputs_of(case):
  seed = 7919 * case.d + 31 * case.q + int(4 * case.span)
  X2 = lattice_points(seed, case.n2, case.d, case.q, case.span)
  X1 = None if not case.n1 else lattice_points(seed + 1, case.n1, case.d, case.q, case.span)
  return X1, X2


def lattice_ints(part, X1, X2):
  """ the integer scaled coordinates of a part's columns and the exponent E: X / bw = s 2^-E, asserted exact and small
      enough for every sum of the distance expansion to be exact in fp64 """
  _, _, _, cols, bw = part
  A, B = X1[:, cols] / bw, X2[:, cols] / bw
  both = np.concatenate([A, B]).ravel()
  nz = both[both != 0]
  E = 0 if not nz.size else max(0, int(-np.min(np.frexp(nz)[1])) + 53)      # every nonzero is a multiple of 2^-E ...
  while E > 0 and np.all(np.ldexp(both, E - 1) == np.rint(np.ldexp(both, E - 1))):     # ... and E is the least such
    E -= 1
  sa, sb = np.ldexp(A, E), np.ldexp(B, E)
  assert np.all(sa == np.rint(sa)) and np.all(sb == np.rint(sb)), 'the scaled inputs are not on a lattice'
  assert max(np.abs(sa).max(), np.abs(sb).max()) < 2.0 ** 31
  sa, sb = sa.astype(np.int64), sb.astype(np.int64)
  worst = max(int((sa * sa).sum(axis=1).max()), int((sb * sb).sum(axis=1).max()))
  assert 4 * worst < 2 ** 53, 'the lattice is too wide for exact fp64 sums: 4 max sum s^2 = %d' % (4 * worst)
  return sa, sb, E


def dsq_exact(part, X1, X2):
  """ (integer squared distances, E): dsq = integer 2^-2E, exactly """
  sa, sb, E = lattice_ints(part, X1, X2)
  diff = sa[:, None, :] - sb[None, :, :]
  return (diff * diff).sum(axis=2), E


# ---- truth --------------------------------------------------------------------------------------------------------
def part_truth(part, dsq_int, E):
  """ (value, arg) of one part in long double from the exact squared distance """
  kind, scale, nu, _, _ = part
  dsq = dsq_int.astype(LD) * LD(2.0) ** (-2 * E)
  if kind == 'se':
    return LD(scale) * np.exp(-dsq / 2), dsq / 2                       # kernel.py:176
  nu_l, p = LD(nu), int(nu)
  dist = np.sqrt(dsq)
  mult = np.sqrt(8 * nu_l) * dist
  u = np.zeros_like(dist)
  for i in range(p + 1):                                                 # kernel.py:259-270
    u += LD(math.factorial(p + i)) / LD(math.factorial(i) * math.factorial(p - i)) * mult ** (p - i)
  arg = np.sqrt(2 * nu_l) * dist
  u0 = LD(math.factorial(2 * p)) / LD(math.factorial(p))                 # the unnormalised value at 0
  return LD(scale) * (u * np.exp(-arg) / u0), arg                       # kernel.py:253, 298


def truth_of(spec, X1, X2):
  """ (truth in long double, the largest Matern arg of any part per entry -- zeros without one, the first part's arg) """
  X1 = X2 if X1 is None else X1
  vals, arg_max, arg0, arg_any = [], np.zeros((len(X1), len(X2)), dtype=LD), None, np.zeros((len(X1), len(X2)), dtype=LD)
  for part in parts_of(spec):
    v, arg = part_truth(part, *dsq_exact(part, X1, X2))
    vals.append(v)
    arg0 = arg if arg0 is None else arg0
    arg_any = np.maximum(arg_any, arg)
    if part[0] == 'matern':
      arg_max = np.maximum(arg_max, arg)
  if spec.kind in ('se', 'matern'):
    return vals[0], arg_max, arg0, np.asarray(arg_any > TAIL_ARG)
  if spec.kind == 'additive':
    return LD(spec.scale) * sum(vals[1:], vals[0]), arg_max, arg0, np.asarray(arg_any > TAIL_ARG)
  if spec.kind == 'product':
    out = LD(spec.scale) * vals[0]
    for v in vals[1:]:
      out = out * v
    return out, arg_max, arg0, np.asarray(arg_any > TAIL_ARG)
  order = int(spec.nu)                                                   # esp: e_order, all terms positive
  e = [np.ones_like(vals[0])] + [np.zeros_like(vals[0]) for _ in range(order)]
  for kc in vals:
    for m in range(order, 0, -1):
      e[m] = e[m] + kc * e[m - 1]
  return LD(spec.scale) * e[order], arg_max, arg0, np.asarray(arg_any > TAIL_ARG)


def oracle_of(spec, X1, X2):
  kern = oracle_engine_esp.ESPOracleKernel(spec) if spec.kind == 'esp' else oracle_engine.to_oracle_spec(spec)
  return kern(X2 if X1 is None else X1, X2)


def ulps(got, truth, arg_max=None):
  """ |got - truth| in units of the spacing of the truth rounded to double (over 1 + arg where given) """
  t64 = truth.astype(np.float64)
  err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - truth) / np.spacing(np.abs(t64)).astype(LD)
  if arg_max is not None:
    err = err / (1 + arg_max)
  return err.astype(np.float64)


def bands(truth, arg):
  """ how many entries of the truth lie in each band; arg: dsq / 2 (SE), sqrt(2 nu) dist (Matern) of the first part """
  t64 = truth.astype(np.float64)
  small = np.asarray(arg < 1)
  return {'arg_below_1': int(small.sum()), 'normal': int(((t64 >= MIN_NORMAL) & ~small).sum()),
          'subnormal': int(((t64 > 0) & (t64 < MIN_NORMAL)).sum()), 'zero': int((t64 == 0).sum())}


Reference = collections.namedtuple('Reference', 'spec X1 X2 truth arg_max oracle regions oracle_ulp limit bands')
_REFERENCES = {}


def reference_of(case):
  """ everything of a case that does not need the device; computed once per input (the variants share it) """
  key = case[2:]
  if key not in _REFERENCES:
    spec = spec_of(case.kernel, case.d)
    X1, X2 = inputs_of(case)
    truth, arg_max, arg0, tail = truth_of(spec, X1, X2)
    scale_by = arg_max if has_matern(spec) else None
    oracle = oracle_of(spec, X1, X2)
    err = ulps(oracle, truth, scale_by)
    regions = {name: mask for name, mask in (('head', ~tail), ('tail', tail)) if mask.any()}
    oracle_ulp = {name: float(err[mask].max()) for name, mask in regions.items()}
    limit = {name: max(FLOOR_ULP, 2 * v) for name, v in oracle_ulp.items()}
    _REFERENCES[key] = Reference(spec, X1, X2, truth, scale_by, oracle, regions, oracle_ulp, limit, bands(truth, arg0))
  return _REFERENCES[key]


# ---- the case table: the shapes of kernmat_digest_check.py ---------------------------------------------------------
def _c(variant, route, tag, kernel, d, n1, n2, q, span):
  return Case(variant, route, tag, kernel, d, n1, n2, q, span)


# (q, span) per kernel and width so that the truth alone has BAND_MIN entries in every band (test_kernel_values_cpu.py)
LATTICE = {('se', 3): (6, 24), ('se', 20): (4, 10), ('se', 8): (5, 14), ('se', 16): (4, 10), ('se', 24): (4, 8),
           ('se', 32): (4, 8), ('m05', 8): (4, 400), ('m15', 8): (4, 220), ('m25', 8): (4, 180), ('m25', 3): (5, 260),
           ('m35', 3): (5, 220)}
MULTI_LATTICE = (5, 30)               # additive / product: the SE part's tail within the Matern part's middle range
# The ESP recurrence subtracts (Newton-Girard, as the reference's): it amplifies the rounding of the 1-D values by
# sum |e_{m-i} p_i| / (m e_m), which grows with the spread of the k_c -- on a lattice with scaled distances up to 8 the
# ORACLE is 3e3 ulp from the truth at order 3, and that amplification, not the device's exp, is what a case would measure.
# Order 17 of 18 columns: the recurrence's terms reach p_1^17 / 17! = 6e6 while e_17 >= 18 min(k_c)^17.  Scaled distances
# of at most 1 (bandwidths 0.5 .. 2, span 0.25: k_c >= exp(-1/2)) keep e_17 above 3e-3, nine orders above the rounding
# of those terms, and the amplification at orders 2 and 3 below 4; test_kernel_values_cpu.py holds the oracle to
# ESP_ORACLE_ULP there.  The tails of the ESP kernel's exp are reached by the huge-distance edge alone.
ESP_LATTICE = (8, 0.25)
ESP_ORACLE_ULP = {2: 8.0, 3: 16.0, 17: 1e6}


def _single(variant, route, kernels, d, n1, n2):
  return [_c(variant, route, k, k, d, n1, n2, *LATTICE[(k, d)]) for k in kernels]


def _multi(variant, route, n1, n2):
  return [_c(variant, route, k, k, 5, n1, n2, *MULTI_LATTICE) for k in ('add', 'prod')]


CASES = (
  _single('default', 'sym', ('se', 'm25', 'm35'), 3, 0, 130) + _single('default', 'sym', ('se',), 20, 0, 130)
  + _single('cfg1', 'sym', ('se', 'm25', 'm35'), 3, 0, 130) + _single('cfg2', 'sym', ('se', 'm25', 'm35'), 3, 0, 258)
  + _single('default', 'cross_lds', ('se', 'm35'), 3, 70, 130)
  + _single('default', 'generic', ('se',), 3, 70, 129)                         # odd leading dimension
  + [c for v, r in (('default', 'strip'), ('strip0', 'cross_lds'))
     for c in _single(v, r, ('se', 'm05', 'm15', 'm25'), 8, 200, 330) + [x for d in (16, 24, 32) for x in _single(v, r, ('se',), d, 200, 330)]]
  + _multi('default', 'symmulti', 0, 130) + _multi('default', 'generic', 70, 130) + _multi('symmulti0', 'generic', 0, 130)
  + [_c('default', 'esp', k, k, d, n1, 70, *ESP_LATTICE)
     for k, d in (('esp2', 5), ('esp3', 5), ('esp3m', 5), ('esp17', 18)) for n1 in (0, 40)]
)
# one small case per route for the edges (equal rows, huge distances, NaN containment); the variants run theirs too
def _family(c):
  k = c.kernel
  return (c.variant, c.route, not c.n1, 'matern' if k[0] == 'm' else ('esp-matern' if k.endswith('m') else k.rstrip('0123456789')))


EDGE_CASES = [c for i, c in enumerate(CASES) if _family(c) not in [_family(x) for x in CASES[:i]]]


def routes_in_table():
  return sorted(set(c.route for c in CASES), key=ROUTES.index)


# ---- checks on the device -------------------------------------------------------------------------------------------
MEASURED = []                       # one record per checked case (--json)


def km(engine, route, spec, X1, X2, diag_add=0.0):
  """ Engine.kernel_matrix as exactly one dispatch on the route the case names """
  before = engine.counters()
  K = engine.kernel_matrix(spec, X2 if X1 is None else X1, None if X1 is None else X2, diag_add=diag_add)
  after = engine.counters()
  assert after['km_dispatches'] == before['km_dispatches'] + 1, (before, after)
  assert after['km_route'] == route, 'written for the %s route, dispatched to %s' % (route, after['km_route'])
  return K


def assert_clean(K, what):
  assert np.all(np.isfinite(K)), '%s: NaN or Inf entries' % what
  assert not np.any(np.signbit(K)), '%s: negative entries (or -0.0)' % what


def check_values(engine, case):
  ref = reference_of(case)
  K = km(engine, case.route, ref.spec, ref.X1, ref.X2)
  err = ulps(K, ref.truth, ref.arg_max)
  device_ulp = {name: float(err[mask].max()) for name, mask in ref.regions.items()}
  rec = {'case': case_id(case), 'route': case.route, 'variant': case.variant, 'kernel': case.kernel, 'device_ulp': device_ulp,
         'oracle_ulp': ref.oracle_ulp, 'limit_ulp': ref.limit, 'per_one_plus_arg': ref.arg_max is not None,
         'band_fraction': {b: ref.bands[b] / float(K.size) for b in BANDS}}
  MEASURED.append(rec)
  print('%-46s %s' % (rec['case'], '; '.join('%s: device %.3g ulp, oracle %.3g, limit %.3g' % (r, device_ulp[r], ref.oracle_ulp[r], ref.limit[r])
                                             for r in ref.regions)))
  assert_clean(K, case_id(case))
  for name, mask in ref.regions.items():
    worst = tuple(np.argwhere(mask)[int(np.argmax(err[mask]))])
    assert err[worst] <= ref.limit[name], (
      '%s, %s: %.4g ulp at %s (device %r, truth %r, oracle %r); the oracle is within %.4g ulp, limit %.4g'
      % (case_id(case), name, err[worst], worst, K[worst], float(ref.truth[worst]), ref.oracle[worst], ref.oracle_ulp[name], ref.limit[name]))
  if not case.n1:
    assert np.array_equal(K, K.T), '%s: the symmetric matrix is not symmetric bit for bit' % case_id(case)


def check_edges(engine, case):
  ref = reference_of(case)
  spec, sym, what = ref.spec, not case.n1, case_id(case)
  n1, n2 = (case.n2, case.n2) if sym else (min(case.n1, 70), min(case.n2, 130))
  X2 = ref.X2[:n2].copy()
  X1 = None if sym else ref.X1[:n1].copy()
  # -- a row of X2 equal to a row of X1: dsq = 0 exactly, the reference's bits
  if not sym:
    X2[5] = X1[3]
  K = km(engine, case.route, spec, X1, X2)
  assert_clean(K, what)
  oracle = oracle_of(spec, X1, X2)
  at = (np.arange(n2), np.arange(n2)) if sym else (3, 5)
  assert np.array_equal(K[at], oracle[at]), '%s: equal rows give %r, the reference %r' % (what, K[at], oracle[at])
  # -- one NaN coordinate in one row of X1: that row (and column of a symmetric matrix), nothing else
  r = 7
  Xn = (X2 if sym else X1).copy()
  Xn[r, case.d - 1] = np.nan
  Kn = km(engine, case.route, spec, None if sym else Xn, Xn if sym else X2)
  hit = np.zeros(K.shape, dtype=bool)
  hit[r, :] = True
  if sym:
    hit[:, r] = True
  assert np.all(np.isnan(Kn[hit])), '%s: entries of the NaN row are not NaN' % what
  assert np.array_equal(Kn[~hit].view(np.int64), K[~hit].view(np.int64)), '%s: a NaN coordinate changed other rows' % what
  # -- bandwidth 2^-17 on integer points: every dsq between different rows is at least 2^34 > 1e10, so -dsq/2 times
  #    log2(e) is beyond the int range; off the diagonal exactly +0.0, on it the scale (+ diag_add)
  far = spec_of(case.kernel, case.d, bw_exp=lambda c: -17)
  F2 = far_points(n2, case.d, 0, far)
  F1 = None if sym else far_points(n1, case.d, n2 - 2, far)           # rows 0, 1 of F1 are rows n2 - 2, n2 - 1 of F2
  for part in parts_of(far):
    lattice_ints(part, F2 if sym else F1, F2)
  Kf = km(engine, case.route, far, F1, F2, diag_add=0.25 if sym else 0.0)
  same = np.eye(n2, dtype=bool) if sym else np.zeros((n1, n2), dtype=bool)
  if not sym:
    same[0, n2 - 2] = same[1, n2 - 1] = True
  assert np.all(Kf[~same] == 0.0) and not np.any(np.signbit(Kf[~same])), '%s: entries at dsq > 1e10 are not +0.0' % what
  at_zero = oracle_of(far, F2[:1], F2[:1])[0, 0]
  assert np.all(Kf[same] == (at_zero + 0.25 if sym else at_zero)), '%s: the entries of equal rows at bandwidth 2^-17' % what
  if sym:
    assert np.array_equal(Kn.view(np.int64), Kn.T.view(np.int64)) and np.array_equal(Kf, Kf.T), '%s: not symmetric' % what


def run_variant(variant, json_path=None):
  from dragonfly_amd.engine import get_engine
  for name, val in VARIANTS[variant].items():
    assert os.environ.get(name) == val, 'variant %s needs %s=%s in the environment' % (variant, name, val)
  engine = get_engine()
  failures = []
  for check, cases in ((check_values, CASES), (check_edges, EDGE_CASES)):
    for case in cases:
      if case.variant == variant:
        try:
          check(engine, case)
        except AssertionError as exc:
          failures.append('%s %s' % (check.__name__, exc))
  if json_path:
    with open(json_path, 'w') as f:
      json.dump(MEASURED, f, indent=1)
  assert not failures, '\n'.join(failures)
  print('OK')


def run_child(variant, json_path=None):
  """ one variant in a child process with its switches set and a time limit of its own """
  cmd = [sys.executable, os.path.abspath(__file__), '--variant', variant] + (['--json', json_path] if json_path else [])
  return subprocess.run(cmd, env=dict(os.environ, **VARIANTS[variant]), capture_output=True, text=True, timeout=CHILD_TIMEOUT)


def main():
  args = sys.argv[1:]
  json_path = args[args.index('--json') + 1] if '--json' in args else None
  if '--all' not in args:
    run_variant(args[args.index('--variant') + 1] if '--variant' in args else 'default', json_path)
    return
  import acq_tail_check
  records, failed = [], []
  for variant in VARIANTS:                       # one at a time
    part = '%s.%s' % (json_path, variant)
    res = run_child(variant, part)
    sys.stdout.write(res.stdout)
    if os.path.exists(part):
      with open(part) as f:
        records += json.load(f)
      os.remove(part)
    if res.returncode != 0 or not res.stdout.strip().endswith('OK'):
      failed.append(variant)
      sys.stdout.write(res.stderr[-4000:])
    if res.returncode not in (0, 1):             # not a failed assertion: nothing more is started on the device
      sys.exit('variant %s ended with exit status %d' % (variant, res.returncode))
  from dragonfly_amd.engine import get_engine
  acq = acq_tail_check.measure(get_engine())
  with open(json_path, 'w') as f:
    json.dump({'metric': 'max |value - truth| / spacing(double(truth)); per_one_plus_arg: divided by 1 + sqrt(2 nu) dist',
               'limit': 'max(2, 2 x oracle_ulp)', 'kernel_values': records, 'acquisitions': acq}, f, indent=1)
  if failed:
    sys.exit('variants that failed: %s' % failed)
  print('ALL OK')


if __name__ == '__main__':
  main()
