"""Run in a subprocess by tests/test_gpu_api_digests.py with DFH_CHUNK_GIB set so small that a posterior chunk is its
512-row floor (the switch is read once per process): every output of the GP entry points of gp_fit.hip, gp_posterior.hip,
gp_adducb.hip, gp_mf.hip and gp_draw.hip on small problems, bit for bit -- the SHA-256 of each is compared with tests/golden/api_output_digests.npz.
Every sum on these paths runs in a fixed order, so a library returns the same bits on every run, and one that returns
other bits has changed what it computes.  The inputs are built by + - * / only from RandomState(seed).random_sample
(labels: a polynomial of X; normals: twelve uniforms minus 6), so their bytes do not depend on the host's libm; each
input's digest is stored under 'input|...', so that a differing input fails as such.  Prints OK on success.

    api_digest_check.py                  compare every digest with the recorded file
    api_digest_check.py --record FILE    write the digests into FILE (created or updated).  Record twice into the same
                                         file: a key whose second digest differs from its first is stored empty -- it did
                                         not reproduce and is not checked; such keys are findings to report.

n = 150, d = 3; m = 300 candidates (one chunk), m = 1100 where chunks matter (512 / 512 / 76: both parities of the
Thompson pipeline, and the wait for a parity's buffers).  Kernels: SE, Matern-2.5, and an additive kernel of an SE group
and a polynomial group.  'dup' is an SE fit on duplicated training rows without noise: it needs the jitter ladder, so
its points in progress take the augmented-GP route instead of the block form; 'adddup' is the additive kernel fitted the
same way, where that route meets the per-candidate prior variance of the polynomial group.  Where an entry point returns
an error, the digest is of its status code.

Besides the digests, every call that returns values and a winner is held to np.argmax -- the first NaN, else the first
maximum, the winning value bit-equal to its element (winner) -- on the computed values and on planted ones: ties across a
workgroup edge and a chunk edge, the last index, NaNs, all -inf (check_planted, check_segment_ties).  numpy is the
reference there: no tolerance, nothing recorded.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from dragonfly_amd import _lib, engine as engine_mod                   # noqa: E402
from dragonfly_amd.engine import ACQ_IDS, KernelSpec, get_engine      # noqa: E402
from draw_cases import CASES                                            # noqa: E402

DIGESTS = os.path.join(ROOT, 'tests', 'golden', 'api_output_digests.npz')
N, DIM, M_ONE, M_CHUNKS, BLOCK = 150, 3, 300, 1100, 128
ADD_GROUPS = [[0, 1], [2]]
MF_GROUPS = [[0], [1, 2], [3, 4, 5]]                 # the additive domain factor of the multi-fidelity GP (behind 1 fidelity column)
LAST_RC = [_lib.DFH_OK]


def _recording_check(rc):
  LAST_RC[0] = rc
  _lib.check(rc)


engine_mod.check = _recording_check                  # the engine's calls leave their status code where Book.call finds it


def uniforms(seed, shape):
  return np.random.RandomState(seed).random_sample(shape)


def normals(seed, shape):
  """ the sum of twelve uniforms minus 6 """
  u = np.random.RandomState(seed).random_sample((12,) + tuple(shape))
  tot = u[0]
  for i in range(1, 12):
    tot = tot + u[i]
  return tot - 6.0


def poly_labels(X):
  return (X[:, 0] - 0.3) * (X[:, 1] + 0.5) * 2.0 - X[:, 2] * X[:, 2] + 0.25 * X[:, 0] * X[:, 2]


def specs():
  bw = 0.3 * (1 + 0.2 * np.arange(DIM))
  return {
    'se': KernelSpec('se', DIM, 0.5, bw),
    'm25': KernelSpec('matern', DIM, 0.5, bw * 0.5 / 0.3, nu=2.5),
    'add': KernelSpec('additive', DIM, 1.5, groups=ADD_GROUPS, sub_kinds=['se', 'poly'], sub_scales=[1.25, 0.75],
                      sub_nus=[0.0, 2.0], sub_bandwidths=[np.array([0.4, 0.6]), np.array([0.8])]),
    'dup': KernelSpec('se', DIM, 0.5, np.full(DIM, 1.5)),
  }


def mf_spec():
  """ 0.7 * SE(z) * 1.2 * (SE(x0) + Matern-2.5(x1, x2) + SE(x3, x4, x5)) over joint points [z, x] """
  groups = [[0]] + [[1 + c for c in g] for g in MF_GROUPS]
  return KernelSpec('product', 7, 0.7, groups=groups, sub_kinds=['se', 'se', 'matern', 'se'], sub_scales=[1.0] * 4,
                    sub_nus=[0.0, 0.0, 2.5, 0.0], sub_bandwidths=[np.array([0.6]), np.array([0.4]), np.array([0.5, 0.7]),
                                                                  np.array([0.6, 0.8, 1.0])],
                    group_factors=[0, 1, 1, 1], factor_sums=[False, True], factor_scales=[1.0, 1.2])


def winner(vals, bv, bi):
  """ the np.argmax rule: the first NaN, else the first maximum; the winning value has the bits of vals[bi] """
  vals = np.ascontiguousarray(vals, dtype=np.float64)
  want = int(np.argmax(vals))
  assert int(bi) == want, 'winner %d, np.argmax %d' % (int(bi), want)
  assert np.float64(bv).tobytes() == vals[want].tobytes(), 'winning value %r, vals[%d] = %r' % (bv, want, vals[want])


class Book(object):
  """ the digests of one run, in the order they were taken """

  def __init__(self):
    self.got = []

  def put(self, key, *arrays):
    h = hashlib.sha256()
    for a in arrays:
      a = np.asarray(a)
      h.update(np.ascontiguousarray(a, dtype='<i8' if a.dtype.kind in 'iub' else '<f8').tobytes())
    self.got.append((key, h.hexdigest()))

  def inp(self, key, a):
    self.put('input|' + key, a)
    return a

  def call(self, key, fn):
    """ fn()'s arrays under `key`, and fn()'s result; where the entry point returns an error, the digest is of its code
        (an error is an output too) and the result is None """
    LAST_RC[0] = _lib.DFH_OK
    try:
      out = fn()
    except (ValueError, np.linalg.LinAlgError, _lib.DfhipError):
      assert LAST_RC[0] != _lib.DFH_OK
      self.put(key, np.array([LAST_RC[0]], dtype=np.int64))
      print('%s returned error %d: %s' % (key, LAST_RC[0], _lib.last_error()))
      return None
    self.put(key, *out)
    return out


def powers(p):
  """ jitter powers as integers (None: no jitter) """
  return np.array([-(1 << 31) if v is None else int(v) for v in np.ravel(np.array(p, dtype=object))], dtype=np.int64)


def run(eng, book):
  X = book.inp('X', uniforms(1, (N, DIM)))
  Y = book.inp('Y', poly_labels(X))
  Xd = X.copy()
  Xd[N // 2:] = Xd[:N - N // 2]                       # every row twice: singular without noise
  book.inp('Xdup', Xd)
  Yd = poly_labels(Xd)
  Xs = book.inp('Xs300', uniforms(2, (M_ONE, DIM)))
  Xl = book.inp('Xs1100', uniforms(3, (M_CHUNKS, DIM)))
  Xh = book.inp('Xh', uniforms(4, (3, DIM)))
  Xn = book.inp('Xnew', uniforms(5, (4, DIM)))
  mv_s = book.inp('mean300', 0.1 * Xs[:, 0] - 0.2 * Xs[:, 1] * Xs[:, 2])
  mv_l = book.inp('mean1100', 0.1 * Xl[:, 0] - 0.2 * Xl[:, 1] * Xl[:, 2])
  U1 = book.inp('U1100x1', normals(6, (M_CHUNKS,)))
  U3 = book.inp('U1100x3', normals(7, (M_CHUNKS, 3)))
  mean_c = 0.125
  sp = specs()
  gps = {}
  for name in ('se', 'm25', 'add', 'dup'):
    noise = 0.0 if name == 'dup' else 0.01
    gp = eng.gp_fit(sp[name], Xd if name == 'dup' else X, (Yd if name == 'dup' else Y) - mean_c, noise)
    gps[name] = gp
    book.put('fit|%s' % name, [gp.lml], gp.get_alpha(), np.tril(gp.get_L()), powers([gp.jitter_power]))
  assert gps['dup'].jitter_power is not None, 'the fit on duplicated rows was meant to need the jitter ladder'
  assert gps['se'].jitter_power is None
  # dfh_gp_append: the block-row update, and (ladder fit) the refit from scratch
  for name in ('se', 'add', 'dup'):
    base_y = (Yd if name == 'dup' else Y) - mean_c
    g2 = gps[name].append(Xn, np.concatenate((base_y, poly_labels(Xn) - mean_c)))
    book.put('append|%s' % name, [g2.lml], g2.get_alpha(), np.tril(g2.get_L()), powers([g2.jitter_power]))
    g2.free()
  book.put('get_K|m25', gps['m25'].get_K())
  # q = 0 / q = 3 in block form ('se', 'm25', 'add') and by the augmented GP ('dup')
  for name in ('se', 'm25', 'add', 'dup'):
    gp = gps[name]
    for q in (0, 3):
      xh = Xh[:q] if q else None
      tag = '%s|q%d' % (name, q)
      book.put('predict|m300|' + tag, *gp.predict(Xs, X_halluc=xh))
      book.put('predict|m1100|' + tag, *gp.predict(Xl, X_halluc=xh))
      for acq in sorted(ACQ_IDS):
        bv, bi, vals = gp.acq_argmax(acq, Xl, params=(0.4, 0.3), mean_const=mean_c, mean_vals=mv_l, X_halluc=xh, return_vals=True)
        book.put('acq|%s|m1100|%s' % (acq, tag), vals, [bv], [bi])
        winner(vals, bv, bi)
      bv, bi, vals = gp.acq_argmax('ucb', Xs, params=(1.7, 0.0), mean_const=mean_c, X_halluc=xh, return_vals=True)
      book.put('acq|ucb|m300|const-mean|' + tag, vals, [bv], [bi])
      winner(vals, bv, bi)
    book.put('predict|mean-only|' + name, gp.predict(Xl, want_std=False)[0])
    for q in (0, 2):
      book.put('covar|%s|q%d' % (name, q), *gp.predict_covar(Xs, X_halluc=Xh[:q] if q else None))
  # add-UCB: one group at a time, all groups stacked (400 rows: one chunk) and the per-group fall-back (1300 rows)
  add = gps['add']
  for sizes in ((200, 200), (700, 600)):
    cands = [book.inp('Xg%d|%d' % (g, mg), uniforms(20 + g + mg, (mg, len(ADD_GROUPS[g])))) for g, mg in enumerate(sizes)]
    bvs, bis, vals = add.add_ucb_all([1.3, 0.7], cands, return_vals=True)
    book.put('add_ucb_all|%d+%d' % sizes, bvs, bis, *vals)
    for g in range(2):
      winner(vals[g], bvs[g], bis[g])
      bv, bi, v = add.add_ucb_group(g, 1.3 - 0.6 * g, cands[g], return_vals=True)
      book.put('add_ucb_group|%d|%d' % (g, sizes[g]), v, [bv], [bi])
      winner(v, bv, bi)
  check_segment_ties(add)
  run_mf(eng, book)
  # Thompson sampling and the joint draws over three chunks
  for name in ('se', 'm25', 'add'):
    bv, bi, samp, jp = gps[name].thompson(Xl, U1, block=BLOCK, mean_const=mean_c, mean_vals=mv_l, return_samples=True)
    book.put('ts|m1100|' + name, samp, [bv], [bi], powers(jp))
    winner(samp, bv, bi)
  bv, bi, samp, jp = gps['se'].thompson(Xs, U1[:M_ONE], block=BLOCK, mean_const=mean_c, return_samples=True)
  book.put('ts|m300|const-mean|se', samp, [bv], [bi], powers(jp))
  winner(samp, bv, bi)
  for name in ('se', 'm25', 'add', 'dup'):
    samp, bvs, bis, jp = gps[name].draw(Xl, U3, 3, BLOCK, Xh, mean_c, mv_l)
    book.put('draw|m1100|q3|S3|' + name, samp, bvs, bis, powers(jp))
    winner_rows(samp, bvs, bis)
  samp, bvs, bis, jp = gps['se'].draw(Xl, U1, 1, BLOCK, Xh, mean_c, mv_l)
  book.put('draw|m1100|q3|S1|se', samp, bvs, bis, powers(jp))
  winner_rows(samp, bvs, bis)
  # point-wise Thompson sampling: the fused first stage of the arg-max, block form and ('dup') the augmented GP
  for name in ('se', 'm25', 'add', 'dup'):
    for q in (0, 3):
      ts_pointwise(book, 'ts_pointwise|m1100|%s|q%d' % (name, q), gps[name], Xl, U1, Xh[:q] if q else None, mean_c, mv_l)
  ts_pointwise(book, 'ts_pointwise|m300|const-mean|se', gps['se'], Xs, U1[:M_ONE], None, mean_c, None)
  run_adddup(eng, book, sp['add'], Xd, Yd - mean_c, Xl, Xh, U1, U3, mean_c, mv_l)
  check_planted(gps['se'], Xl, U1, U3, mean_c)
  for ci, cname in enumerate(sorted(CASES)):
    kind, m, block, q, S, dup = CASES[cname]
    cx = uniforms(100 + ci, (m, DIM))
    for row in dup:
      cx[row] = cx[3]
    book.inp('case|%s|Xs' % cname, cx)
    cu = book.inp('case|%s|U' % cname, normals(200 + ci, (m, S)))
    samp, bvs, bis, jp = gps[kind].draw(cx, cu, S, block, Xh[:q] if q else None, mean_c)
    book.put('draw|case|' + cname, samp, bvs, bis, powers(jp))
    winner_rows(samp, bvs, bis)
  # multi-objective: k = 2, both scalarisations, block form / no points in progress; then with a ladder fit among the two
  Uk = book.inp('U2x1100', normals(8, (2, M_CHUNKS)))
  mvk = np.stack((mv_l, 0.5 * mv_l))
  for pair in (('se', 'm25'), ('add', 'dup')):
    two = [gps[pair[0]], gps[pair[1]]]
    for scal in ('lin', 'tch'):
      tag = '%s|%s+%s' % (scal, pair[0], pair[1])
      bv, bi, vals = eng.mo_ucb_argmax(two, scal, 1.1, [0.6, 0.4], [0.05, -0.1], Xl, mean_consts=[mean_c, 0.0], return_vals=True)
      book.put('mo_ucb|' + tag, vals, [bv], [bi])
      winner(vals, bv, bi)
      bv, bi, vals = eng.mo_ucb_argmax(two, scal, 1.1, [0.6, 0.4], [0.05, -0.1], Xl, mean_vals=mvk, return_vals=True)
      book.put('mo_ucb|mean-vals|' + tag, vals, [bv], [bi])
      winner(vals, bv, bi)
      for q in (0, 3):
        bv, bi, vals, jp = eng.mo_thompson(two, scal, [0.6, 0.4], [0.05, -0.1], Xl, Uk, block=BLOCK, X_halluc=Xh[:q] if q else None,
                                           mean_consts=[mean_c, 0.0], return_vals=True)
        book.put('mo_ts|q%d|%s' % (q, tag), vals, [bv], [bi], powers(jp))
        winner(vals, bv, bi)
  for gp in gps.values():
    gp.free()


def winner_rows(samp, bvs, bis):
  for s in range(len(samp)):
    winner(samp[s], bvs[s], bis[s])


def ts_pointwise(book, key, gp, Xs, U, xh, mean_c, mv):
  """ digest of (samples, best value, best index) of one point-wise Thompson call, or of its error code """
  def fn():
    bv, bi, samp = gp.thompson_pointwise(Xs, U, X_halluc=xh, mean_const=mean_c, mean_vals=mv, return_samples=True)
    return samp, [bv], [bi]
  out = book.call(key, fn)
  if out is not None:
    winner(out[0], out[1][0], out[2][0])


def run_adddup(eng, book, spec, Xd, yd, Xl, Xh, U1, U3, mean_c, mv_l):
  """ A ladder fit with a non-stationary part: the additive kernel (SE + polynomial group) on duplicated rows without
      noise -- the only route where the augmented GP of the points in progress and prior_diag (kss) meet. """
  gp = eng.gp_fit(spec, Xd, yd, 0.0)
  book.put('fit|adddup', [gp.lml], gp.get_alpha(), np.tril(gp.get_L()), powers([gp.jitter_power]))
  assert gp.jitter_power is not None, 'the additive fit on duplicated rows was meant to need the jitter ladder'
  for q in (0, 3):
    xh = Xh[:q] if q else None
    book.call('predict|m1100|adddup|q%d' % q, lambda: gp.predict(Xl, X_halluc=xh))
    for acq in ('ucb', 'ei'):
      def fn():
        bv, bi, vals = gp.acq_argmax(acq, Xl, params=(0.4, 0.3), mean_const=mean_c, mean_vals=mv_l, X_halluc=xh, return_vals=True)
        return vals, [bv], [bi]
      out = book.call('acq|%s|m1100|adddup|q%d' % (acq, q), fn)
      if out is not None:
        winner(out[0], out[1][0], out[2][0])
  ts_pointwise(book, 'ts_pointwise|m1100|adddup|q3', gp, Xl, U1, Xh, mean_c, mv_l)

  def draw():
    samp, bvs, bis, jp = gp.draw(Xl, U3, 3, BLOCK, Xh, mean_c, mv_l)
    return samp, bvs, bis, powers(jp)
  out = book.call('draw|m1100|q3|S3|adddup', draw)
  if out is not None:
    winner_rows(out[0], out[1], out[2])
  gp.free()


def run_mf(eng, book):
  """ the multi-fidelity add-UCB of gp_mf.hip: the stack in one chunk (450 rows), the per-group fall-back (1800 rows) and
      one group at a time """
  J = book.inp('mf|J', uniforms(30, (N, 7)))
  y = (J[:, 0] - 0.4) * (J[:, 1] + 0.3) + J[:, 2] * J[:, 3] - 0.5 * J[:, 4] * J[:, 4] + 0.25 * J[:, 5] * J[:, 6]
  book.inp('mf|y', y)
  gp = eng.gp_fit(mf_spec(), J, y - 0.125, 0.01)
  book.put('fit|mf', [gp.lml], gp.get_alpha(), np.tril(gp.get_L()), powers([gp.jitter_power]))
  z, betas = np.array([0.8]), [1.3, 0.7, 2.1]
  for sizes in ((150, 150, 150), (700, 600, 500)):
    cands = [book.inp('mf|Xg%d|%d' % (g, mg), uniforms(40 + g + mg, (mg, len(MF_GROUPS[g])))) for g, mg in enumerate(sizes)]
    bvs, bis, vals = gp.mf_add_ucb_all(z, betas, cands, return_vals=True)
    book.put('mf_add_ucb_all|%d+%d+%d' % sizes, bvs, bis, *vals)
    for g in range(3):
      winner(vals[g], bvs[g], bis[g])
      bv, bi, v = gp.mf_add_ucb_group(z, g, betas[g], cands[g], return_vals=True)
      book.put('mf_add_ucb_group|%d|%d' % (g, sizes[g]), v, [bv], [bi])
      winner(v, bv, bi)
  gp.free()


def check_segment_ties(add):
  """ The segment reducer takes no prior means: ties are planted by copying each group's winning row over that group's
      rows 199 and (winner + 1) % 200. """
  cands = [uniforms(20 + g + 200, (200, len(ADD_GROUPS[g]))) for g in range(2)]
  _, bis, _ = add.add_ucb_all([1.3, 0.7], cands, return_vals=True)
  copies = []
  for g in range(2):
    rows = (199, (int(bis[g]) + 1) % 200)
    for r in rows:
      cands[g][r] = cands[g][int(bis[g])]
    copies.append(rows)
  bvs, bi2, vals = add.add_ucb_all([1.3, 0.7], cands, return_vals=True)
  for g in range(2):
    winner(vals[g], bvs[g], bi2[g])
    for r in copies[g]:
      assert vals[g][r].tobytes() == vals[g][int(bis[g])].tobytes(), 'group %d: a copy of the winning row has other bits' % g


def check_planted(gp, Xl, U1, U3, mean_c):
  """ The arg-max rule on planted prior means, against np.argmax: ties across a workgroup edge and a chunk edge, the last
      index, NaNs, and all -inf (the winner is index 0).  Through acq_argmax (two stages and the merge across chunks),
      thompson_pointwise (the fused first stage) and draw with S = 3 (one workgroup per row). """
  inf, nan = np.inf, np.nan
  plans = [{255: inf, 256: inf}, {511: inf, 512: inf}, {1099: inf}, {1099: nan}, {512: nan, 1099: nan, 3: inf}, None]
  for plan in plans:
    mv = np.full(M_CHUNKS, -inf) if plan is None else 0.01 * np.arange(M_CHUNKS) / M_CHUNKS
    for i, v in (plan or {}).items():
      mv[i] = v
    bv, bi, vals = gp.acq_argmax('ucb', Xl, params=(0.4, 0.0), mean_const=mean_c, mean_vals=mv, return_vals=True)
    winner(vals, bv, bi)
    bv, bi, samp = gp.thompson_pointwise(Xl, U1, mean_const=mean_c, mean_vals=mv, return_samples=True)
    winner(samp, bv, bi)
    samp, bvs, bis, _ = gp.draw(Xl, U3, 3, BLOCK, None, mean_c, mv)
    winner_rows(samp, bvs, bis)
    if plan is None:
      assert bi == 0 and np.all(bis == 0)
  for m in (1, 257):
    mv = np.zeros(m)
    mv[m - 1] = inf
    bv, bi, vals = gp.acq_argmax('ucb', Xl[:m], params=(0.4, 0.0), mean_const=mean_c, mean_vals=mv, return_vals=True)
    winner(vals, bv, bi)
    assert bi == m - 1
    bv, bi, samp = gp.thompson_pointwise(Xl[:m], U1[:m], mean_const=mean_c, mean_vals=mv, return_samples=True)
    winner(samp, bv, bi)
    assert bi == m - 1


def load_digests(path):
  if not os.path.exists(path):
    return {}
  with np.load(path) as z:
    return dict(zip((str(k) for k in z['keys']), (str(d) for d in z['digests'])))


def main():
  record_to = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == '--record' else None
  book = Book()
  run(get_engine(), book)
  known = load_digests(record_to or DIGESTS)
  bad = []
  for key, got in book.got:
    print('%s %s' % (key, got))
    if record_to:
      known[key] = got if known.get(key, got) == got else ''
    elif key not in known:
      bad.append('%s is not in tests/golden/api_output_digests.npz' % key)
    elif not known[key]:
      bad.append('%s did not reproduce when the file was recorded (stored empty)' % key)
    elif known[key] != got:
      bad.append('the bits of %s differ from tests/golden/api_output_digests.npz: %s, recorded %s' % (key, got, known[key]))
  if record_to:
    keys = sorted(known)
    np.savez_compressed(record_to, keys=np.array(keys), digests=np.array([known[k] for k in keys]))
    print('empty: %s' % sorted(k for k in keys if not known[k]))
  else:
    missing = sorted(set(known) - set(k for k, _ in book.got))
    bad += ['%s is recorded but was not computed' % k for k in missing]
    assert not bad, '\n'.join(bad)
  print('OK')


if __name__ == '__main__':
  main()
