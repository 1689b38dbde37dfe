"""Case table and checks of the fp64 MFMA GEMM behind the public dfh_gemm (tests/test_gpu_gemm.py).

Every call goes through Engine.gemm, or through engine.lib.dfh_gemm where leading dimensions or null operands
are wanted, inside a gemm_profile bracket: a case states which kernel variant it was written for -- slot =
(NN ? 4 : 0) | (edge ? 2 : 0) | (64-tile ? 1 : 0) -- and how many launches it books there, and fails when the
dispatch sends it anywhere else.

Two references, neither with a measured tolerance:
  exact    integer entries in [-8, 8], alpha and beta from {+-1, 2, 0.5, 1.5, 0}: every intermediate is a
           multiple of 1/4 far below 2^53, so the device result equals the int64 product (scaled on the host)
           bit for bit whatever the summation order;
  rounded  randn entries against numpy.longdouble, componentwise
           |got - ref| <= gamma_{K+2} (|alpha| |A||B|^T + |beta| |C|),  gamma_n = n u / (1 - n u),  u = 2^-53:
           K fused multiply-adds in any order and the two roundings of the epilogue.

Run as a program with DFH_GEMM_FORCE_LA=1 in the environment (the switch is read once per process) it sends
the LOWER products of LA_CASES through the look-ahead tile order and prints OK; without the switch it runs the
whole in-process table."""
import collections
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

U = 2.0 ** -53
SENTINEL = 7777.25          # every result of the exact cases is a multiple of 1/2: none equals it
NAN = float('nan')

# slots: what a launch books in gemm_profile
NT128, NT64, NT128E, NT64E, NN128, NN64, NN128E, NN64E = range(8)
LA = 7                      # the look-ahead kernel shares the number of the NN edge 64-tile kernel: it is NT and
                            # LOWER only, so a case that is neither NN nor below 192 128-tiles can only mean it

Case = collections.namedtuple('Case', 'group M N K transb lower alpha beta pads slots')


def case_id(c):
  s = '%s-%s-%dx%dx%d-a%g-b%g' % (c.group, 'nn' if c.transb else 'nt', c.M, c.N, c.K, c.alpha, c.beta)
  if c.lower:
    s += '-lower'
  if any(c.pads):
    s += '-ld+%d+%d+%d' % c.pads
  return s + '-slot' + '+'.join('%dx%d' % (k, v) for k, v in sorted(c.slots.items()))


def _case(group, M, N, K, transb, alpha, beta, slots, lower=False, pads=(0, 0, 0)):
  if isinstance(slots, int):
    slots = {slots: 1}
  return Case(group, M, N, K, bool(transb), bool(lower), float(alpha), float(beta), tuple(pads), dict(slots))


# -- 64 x 64 tiles: fewer than 192 128-tiles.  (M, N, K, alpha, beta, NT slot, NN slot); both operand layouts run.
# Edge = ragged M or N, K no multiple of 16, or an odd leading dimension (NT: lda = ldb = K; NN: ldb = N).
_T64 = [
  (1, 1, 1, 1, 0, NT64E, NN64E),
  (1, 63, 15, -1, 1, NT64E, NN64E),
  (63, 1, 16, 2, -1, NT64E, NN64E),
  (64, 64, 16, 0.5, 0.5, NT64, NN64),
  (64, 64, 64, 1, 1, NT64, NN64),
  (64, 64, 1, -1, 0, NT64E, NN64E),        # full tiles, K alone picks the edge kernel: only the k predicate guards
  (64, 64, 17, 2, 1, NT64E, NN64E),
  (64, 64, 33, 0.5, -1, NT64E, NN64E),
  (65, 65, 17, 1, -1, NT64E, NN64E),
  (129, 129, 33, -1, 0.5, NT64E, NN64E),
  (63, 64, 1, 2, 0, NT64E, NN64E),
  (64, 65, 15, 0.5, 1, NT64E, NN64E),
  (65, 63, 17, 1, 0.5, NT64E, NN64E),
  (129, 64, 16, -1, -1, NT64E, NN64E),
  (64, 129, 64, 2, 0.5, NT64E, NN64E),
  (1, 129, 33, 0.5, 0, NT64E, NN64E),
  (129, 1, 17, -1, 1, NT64E, NN64E),
  (63, 63, 64, 1, 1, NT64E, NN64E),
  (129, 65, 1, 2, -1, NT64E, NN64E),
  (64, 63, 33, 0.5, 0.5, NT64E, NN64E),
  # 13 x 7 tiles = 91 workgroups: the XCD spans differ in length (91 = 8 * 11 + 3) and the last group of row
  # tiles holds 5; ragged through the edge kernel, whole through the fast one
  (12 * 64 + 5, 6 * 64 + 3, 17, -1, 1, NT64E, NN64E),
  (13 * 64, 7 * 64, 16, 2, 0.5, NT64, NN64),
]
TILE64 = [_case('t64', M, N, K, tb, a, b, (snn if tb else snt))
          for (M, N, K, a, b, snt, snn) in _T64 for tb in (False, True)]

# -- 128 x 128 tiles: at least 192 of them.  1792 = 14 tiles (196 workgroups = 8 * 24 + 4, last row group of 6),
# 1791 x 1793 = 14 x 15, 1800 x 1600 = 15 x 13 (195 = 8 * 24 + 3, last row group of 7).
TILE128 = [
  _case('t128', 1792, 1792, 16, False, 1, 1, NT128),
  _case('t128', 1792, 1792, 48, False, 0.5, -1, NT128),
  _case('t128', 1792, 1792, 17, False, -1, 0.5, NT128E),
  _case('t128', 1792, 1792, 48, True, 2, 0, NN128),
  _case('t128', 1792, 1792, 16, True, -1, 1, NN128),
  _case('t128', 1791, 1793, 48, False, 2, 1, NT128E),
  _case('t128', 1791, 1793, 17, True, 1, -1, NN128E),
  _case('t128', 1800, 1600, 16, False, -1, 1, NT128E),
  _case('t128', 1800, 1600, 17, False, 0.5, 0.5, NT128E),
  _case('t128', 1800, 1600, 48, True, 1, 0, NN128E),
]

# -- row split (gemm_f64: N a multiple of 128, M >= 1024 and not, nothing else ragged): the full row tiles and the
# leftover rows are products of their own, each dispatched by its own tile count.
#   1032 x 2816: 9 x 22 = 198 128-tiles, so the split is taken; 1024 x 2816 is 8 x 22 = 176 < 192 and runs as 64-tiles
#   through the fast kernel; the 8 leftover rows are a ragged 64-tile and must be bounds-checked.
#   1088 x 3072: 1024 x 3072 is 8 x 24 = 192 128-tiles, the 64 leftover rows are one whole row of 64-tiles.
ROWSPLIT = [
  _case('rowsplit', 1032, 2816, 32, False, 1, 1, {NT64: 1, NT64E: 1}),
  _case('rowsplit', 1088, 3072, 32, False, -1, 0.5, {NT128: 1, NT64: 1}),
]

# -- lower_only: tiles above the diagonal are not computed
LOWER = [
  _case('lower', 65, 65, 17, False, -1, 1, NT64E, lower=True),
  _case('lower', 65, 65, 17, False, 0.5, 0, NT64E, lower=True),
  _case('lower', 200, 200, 16, False, -1, 1, NT64E, lower=True),
  _case('lower', 200, 200, 16, False, 0.5, 0, NT64E, lower=True),
  _case('lower', 200, 200, 16, True, -1, 1, NN64E, lower=True),
  _case('lower', 1700, 1700, 16, False, -1, 1, NT128E, lower=True),
  _case('lower', 1700, 1700, 16, False, 0.5, 0, NT128E, lower=True),
  _case('lower', 1792, 1792, 16, False, -1, 1, NT128, lower=True),
  _case('lower', 1792, 1792, 16, False, 0.5, 0, NT128, lower=True),
  _case('lower', 1792, 1792, 16, True, -1, 1, NN128, lower=True),
]

# -- leading dimensions: pads = extra columns of (A, B, C); A's and B's hold NaN, C's the sentinel.
# An odd lda or ldb must pick the edge kernel (16-byte operand loads), an even one must not.
LEADING = [
  _case('ld', 128, 64, 16, False, 1, 1, NT64E, pads=(1, 1, 3)),
  _case('ld', 128, 64, 16, False, -1, 0.5, NT64, pads=(2, 2, 3)),
  _case('ld', 128, 64, 16, False, 2, 0, NT64E, pads=(1, 2, 3)),
  _case('ld', 128, 64, 16, False, 0.5, 1, NT64E, pads=(2, 1, 3)),
  _case('ld', 65, 63, 17, False, -1, 1, NT64E, pads=(1, 1, 3)),
  _case('ld', 128, 64, 16, True, 1, -1, NN64E, pads=(1, 1, 3)),
  _case('ld', 128, 64, 16, True, 2, 1, NN64, pads=(2, 2, 3)),
  _case('ld', 1792, 1792, 16, False, -1, 1, NT128E, pads=(1, 1, 3)),
  _case('ld', 1792, 1792, 16, False, 0.5, 0.5, NT128, pads=(2, 2, 3)),
  _case('ld', 1792, 1792, 16, True, 1, 0, NN128E, pads=(1, 1, 3)),
  _case('ld', 1792, 1792, 16, True, -1, 1, NN128, pads=(2, 2, 3)),
]

# -- the two epilogues: alpha = +-1 loads beta * C into the accumulators, any other alpha adds it at the end
_EPI = [(1, 1), (-1, 1), (-1, 0.5), (1.5, 0.5), (2, 0)]
EPILOGUE = ([_case('epi', 129, 65, 17, False, a, b, NT64E) for a, b in _EPI] +
            [_case('epi', 1792, 1792, 16, False, a, b, NT128) for a, b in _EPI])

EXACT_CASES = TILE64 + TILE128 + ROWSPLIT + LOWER + LEADING + EPILOGUE
ROUNDED_CASES = TILE64 + TILE128 + ROWSPLIT + [LOWER[2], LOWER[5], LEADING[1], LEADING[7]]

# -- K = 0 with null operands: out = beta * C.  (M, N, transb, slot); lda = 0, ldb = 0 (NT) or N (NN)
K0_SHAPES = [(64, 64, False, NT64), (64, 64, True, NN64), (65, 129, False, NT64E), (65, 129, True, NN64E)]
K0_SCALARS = [(1, 0), (2, 0), (2, 0.5), (1, 1), (-1, -1), (0.5, 1)]

# -- NaN containment: one edge and one fast shape per tile size.  (M, N, K, transb, slot)
NAN_SHAPES = [(65, 63, 17, False, NT64E), (128, 64, 16, False, NT64), (1800, 1600, 17, False, NT128E),
              (1792, 1792, 16, False, NT128), (65, 63, 17, True, NN64E), (128, 64, 16, True, NN64),
              (1800, 1600, 17, True, NN128E), (1792, 1792, 16, True, NN128)]

# -- look-ahead tile order (child process, DFH_GEMM_FORCE_LA=1): LOWER NT products of 5, 6, 8, 9 and 14 tile rows
# (one or two blocks of 32 look-ahead workgroups, of which 14, 18, 26, 30 and 50 are real tiles), K whole and ragged
LA_CASES = [_case('la', M, M, K, False, -1, 1, LA, lower=True) for M in (640, 641, 1024, 1152, 1700) for K in (16, 20)]
LA_TOO_SMALL = _case('la', 512, 512, 16, False, -1, 1, NT64, lower=True)      # four tile rows: not eligible


def slots_in_table():
  """ {slot: number of in-process cases written for it alone} """
  out = collections.Counter()
  for c in EXACT_CASES:
    if len(c.slots) == 1:
      out[next(iter(c.slots))] += 1
  return out


def one_case_per_slot():
  picked = {}
  for c in EXACT_CASES:
    if len(c.slots) == 1 and not any(c.pads) and not c.lower:
      picked.setdefault(next(iter(c.slots)), c)
  return [picked[s] for s in sorted(picked)]


# -- inputs and references (computed once per shape, handed out read-only) ------------------------------------------
def _ro(a):
  a.setflags(write=False)
  return a


@functools.lru_cache(maxsize=6)
def int_inputs(M, N, K, transb):
  rs = np.random.RandomState((M * 7919 + N * 104729 + K * 31 + int(transb)) % (2 ** 31))
  A = rs.randint(-8, 9, size=(M, K)).astype(np.float64)
  B = rs.randint(-8, 9, size=((K, N) if transb else (N, K))).astype(np.float64)
  C = rs.randint(-8, 9, size=(M, N)).astype(np.float64)
  Bi = B.astype(np.int64)
  P = A.astype(np.int64).dot(Bi if transb else Bi.T)
  return _ro(A), _ro(B), _ro(C), _ro(P.astype(np.float64))


@functools.lru_cache(maxsize=3)
def randn_inputs(M, N, K, transb):
  rs = np.random.RandomState((M * 15485863 + N * 32452843 + K * 17 + int(transb)) % (2 ** 31))
  A = rs.randn(M, K)
  B = rs.randn(*((K, N) if transb else (N, K)))
  C = rs.randn(M, N)
  Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
  P = Al.dot(Bl if transb else Bl.T)
  S = np.abs(Al).dot(np.abs(Bl) if transb else np.abs(Bl).T)
  return _ro(A), _ro(B), _ro(C), _ro(P), _ro(S)


def gamma(n):
  return n * U / (1.0 - n * U)


# -- the call -------------------------------------------------------------------------------------------------------
def profiled(eng, fn):
  """ fn() between gemm_profile brackets -> (result, {slot: launches}) """
  eng.gemm_profile(enable=True, fetch=False)
  try:
    out = fn()
  finally:
    prof = eng.gemm_profile(enable=False)
  return out, {v: p['launches'] for v, p in enumerate(prof) if p['launches']}


def raw_gemm(eng, transb, M, N, K, alpha, A, lda, B, ldb, beta, Cbuf, ldc, lower):
  from dragonfly_amd._lib import check
  ptr = lambda a: None if a is None else a.__array_interface__['data'][0]
  check(eng.lib.dfh_gemm(eng.ctx, 1 if transb else 0, M, N, K, float(alpha), ptr(A), lda, ptr(B), ldb, float(beta),
                         ptr(Cbuf), ldc, 1 if lower else 0))


def _padded(a, pad, fill):
  out = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=np.float64)
  out[:, :a.shape[1]] = a
  return out


def run(eng, c, A, B, Cin):
  """ One product of case c on the device -> out[M x N]; asserts the launches it books and, with padded leading
      dimensions, that C's padding columns come back bit-unchanged.  Cin is what the output buffer holds on entry. """
  pa, pb, pc = c.pads
  if not any(c.pads):
    out, booked = profiled(eng, lambda: eng.gemm(A, B, Cin, alpha=c.alpha, beta=c.beta, transb=c.transb,
                                                 lower_only=c.lower))
  else:
    Ap, Bp, Cp = _padded(A, pa, NAN), _padded(B, pb, NAN), _padded(Cin, pc, SENTINEL)
    _, booked = profiled(eng, lambda: raw_gemm(eng, c.transb, c.M, c.N, c.K, c.alpha, Ap, Ap.shape[1], Bp, Bp.shape[1],
                                               c.beta, Cp, Cp.shape[1], c.lower))
    assert np.array_equal(Cp[:, c.N:], np.full((c.M, pc), SENTINEL)), 'padding columns of C were written'
    out = np.ascontiguousarray(Cp[:, :c.N])
  assert booked == c.slots, 'launches booked %r, the case was written for %r' % (booked, c.slots)
  return out


def tile_edge(c):
  """ tile size of a single-launch case """
  (slot,) = c.slots
  return 64 if (slot & 1 and c.group != 'la') else 128


def entry_c(c, C):
  """ What the output buffer holds on entry: C where beta reads it, NaN where beta = 0 must not; for LOWER the
      tiles strictly above the diagonal hold the sentinel. """
  Cin = C.copy() if c.beta != 0.0 else np.full((c.M, c.N), NAN)
  if c.lower:
    Cin[upper_tiles(c)] = SENTINEL
  return Cin


def upper_tiles(c):
  t = tile_edge(c)
  i = np.arange(c.M) // t
  return i[:, None] < i[None, :]


def first_bad(mask):
  idx = np.argwhere(mask)
  return 'none' if not len(idx) else '%d entries, first (row %d, col %d), last (row %d, col %d)' % (
    len(idx), idx[0][0], idx[0][1], idx[-1][0], idx[-1][1])


def check_exact(eng, c):
  A, B, C, P = int_inputs(c.M, c.N, c.K, c.transb)
  Cin = entry_c(c, C)
  got = run(eng, c, A, B, Cin)
  ref = c.alpha * P + (c.beta * C if c.beta != 0.0 else 0.0)
  if c.lower:
    up = upper_tiles(c)
    assert np.array_equal(got[up], Cin[up]), 'tiles above the diagonal written: ' + first_bad(up & (got != Cin))
    low = np.tril(np.ones((c.M, c.M), dtype=bool))
    bad = low & (got != ref)
  else:
    bad = got != ref
  assert not bad.any(), 'not the exact product: ' + first_bad(bad)
  return got


def check_rounded(eng, c):
  A, B, C, P, S = randn_inputs(c.M, c.N, c.K, c.transb)
  Cin = entry_c(c, C)
  got = run(eng, c, A, B, Cin)
  ref = c.alpha * P + (c.beta * C.astype(np.longdouble) if c.beta != 0.0 else 0.0)
  bound = gamma(c.K + 2) * (abs(c.alpha) * S + abs(c.beta) * np.abs(C))
  err = np.abs(got.astype(np.longdouble) - ref)
  keep = np.tril(np.ones((c.M, c.M), dtype=bool)) if c.lower else np.ones((c.M, c.N), dtype=bool)
  if c.lower:
    up = upper_tiles(c)
    assert np.array_equal(got[up], Cin[up]), 'tiles above the diagonal written'
  ratio = float(np.max(np.where(keep & (bound > 0), err / np.where(bound > 0, bound, 1), 0)))
  print('%s: largest |got - ref| / bound = %.3f' % (case_id(c), ratio))
  bad = keep & ~(err <= bound)
  assert not bad.any(), 'beyond gamma_{K+2}: ' + first_bad(bad)
  return got


def check_k0(eng, M, N, transb, slot, alpha, beta):
  """ K = 0, A = B = NULL: out = beta * C exactly; with beta = 0 all zeros, over a NaN-filled C too. """
  rs = np.random.RandomState(M + N)
  C = rs.randn(M, N) if beta != 0.0 else np.full((M, N), NAN)
  buf = C.copy()
  _, booked = profiled(eng, lambda: raw_gemm(eng, transb, M, N, 0, alpha, None, 0, None, (N if transb else 0), beta,
                                             buf, N, False))
  assert booked == {slot: 1}, booked
  ref = beta * C if beta != 0.0 else np.zeros((M, N))
  assert np.array_equal(buf, ref), first_bad(buf != ref)


def check_nan(eng, M, N, K, transb, slot):
  """ beta = 0 over a NaN-filled C gives no NaN; a NaN in row i of A poisons row i and nothing else, a NaN in
      row j of op(B)^T column j and nothing else; every other entry is still the exact product. """
  A, B, _, P = int_inputs(M, N, K, transb)
  c = _case('nan', M, N, K, transb, 1.0, 0.0, slot)
  Cin = np.full((M, N), NAN)
  got = run(eng, c, A, B, Cin)
  assert np.array_equal(got, P), first_bad(got != P)
  i, j, k = (2 * M) // 3, N // 2, K - 1
  An = A.copy(); An[i, k] = NAN
  got = run(eng, c, An, B, Cin)
  rows = np.zeros((M, N), dtype=bool); rows[i, :] = True
  assert np.array_equal(np.isnan(got), rows), first_bad(np.isnan(got) != rows)
  assert np.array_equal(got[~rows], P[~rows])
  Bn = B.copy()
  if transb:
    Bn[k, j] = NAN
  else:
    Bn[j, k] = NAN
  got = run(eng, c, A, Bn, Cin)
  cols = np.zeros((M, N), dtype=bool); cols[:, j] = True
  assert np.array_equal(np.isnan(got), cols), first_bad(np.isnan(got) != cols)
  assert np.array_equal(got[~cols], P[~cols])


def check_deterministic(eng, c):
  A, B, C = randn_inputs(c.M, c.N, c.K, c.transb)[:3]
  first = run(eng, c, A, B, entry_c(c, C))
  again = run(eng, c, A, B, entry_c(c, C))
  assert np.array_equal(first, again), first_bad(first != again)


def check_row_split_bits(eng, c):
  """ The split product's rows are bit for bit those of the two products it is made of. """
  A, B = randn_inputs(c.M, c.N, c.K, c.transb)[:2]
  M1 = (c.M // 128) * 128
  whole, booked = profiled(eng, lambda: eng.gemm(A, B))
  assert booked == c.slots, booked
  top, booked_top = profiled(eng, lambda: eng.gemm(A[:M1], B))
  bottom, booked_bottom = profiled(eng, lambda: eng.gemm(A[M1:], B))
  assert sum(booked_top.values()) == 1 and sum(booked_bottom.values()) == 1
  assert collections.Counter(booked_top) + collections.Counter(booked_bottom) == collections.Counter(c.slots)
  assert np.array_equal(whole[:M1], top), first_bad(whole[:M1] != top)
  assert np.array_equal(whole[M1:], bottom), first_bad(whole[M1:] != bottom)


# sub-ranges of the rows of a 1792 x 1792 x 48 product (128-tiles, fast kernel) that run as 64-tiles on their own:
# (first row, rows, slot) -- a whole number of 64-tiles through the fast kernel, a ragged range off the tile grid
SUBRANGES = [(256, 128, NT64), (300, 129, NT64E)]


def check_subrange_bits(eng):
  """ gemm(A[r0:r1], B) == gemm(A, B)[r0:r1] bit for bit although the tile size differs: a row's sum runs over
      the same 16-column chunks in the same order in every instantiation. """
  M, N, K = 1792, 1792, 48
  A, B = randn_inputs(M, N, K, False)[:2]
  whole, booked = profiled(eng, lambda: eng.gemm(A, B))
  assert booked == {NT128: 1}, booked
  for r0, rows, slot in SUBRANGES:
    part, booked = profiled(eng, lambda: eng.gemm(A[r0:r0 + rows], B))
    assert booked == {slot: 1}, booked
    assert np.array_equal(part, whole[r0:r0 + rows]), (r0, rows, first_bad(part != whole[r0:r0 + rows]))


def check_lookahead(eng):
  assert os.environ.get('DFH_GEMM_FORCE_LA') == '1'
  for c in LA_CASES + [LA_TOO_SMALL]:
    check_exact(eng, c)
    print('ok', case_id(c))
  check_deterministic(eng, LA_CASES[-1])


def main():
  from dragonfly_amd.engine import get_engine
  eng = get_engine()
  if os.environ.get('DFH_GEMM_FORCE_LA') == '1':
    check_lookahead(eng)
  else:
    for c in EXACT_CASES:
      check_exact(eng, c)
    for c in ROUNDED_CASES:
      check_rounded(eng, c)
    for M, N, transb, slot in K0_SHAPES:
      for alpha, beta in K0_SCALARS:
        check_k0(eng, M, N, transb, slot, alpha, beta)
    for shape in NAN_SHAPES:
      check_nan(eng, *shape)
    for c in one_case_per_slot():
      check_deterministic(eng, c)
    for c in ROWSPLIT:
      check_row_split_bits(eng, c)
    check_subrange_bits(eng)
  print('OK')


if __name__ == '__main__':
  main()
