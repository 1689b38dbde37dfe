"""Run in a subprocess by tests/test_gpu_api_digests.py with DFH_CHUNK_GIB set so small that a posterior chunk is its
512-row floor (the switch is read once per process): every output of the GP entry points of gp_fit.hip, gp_posterior.hip
and gp_draw.hip on small problems, bit for bit -- the SHA-256 of each is compared with tests/golden/api_output_digests.npz.
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
its points in progress take the augmented-GP route instead of the block form.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from dragonfly_amd.engine import ACQ_IDS, KernelSpec, get_engine      # noqa: E402
from draw_cases import CASES                                            # noqa: E402

DIGESTS = os.path.join(ROOT, 'tests', 'golden', 'api_output_digests.npz')
N, DIM, M_ONE, M_CHUNKS, BLOCK = 150, 3, 300, 1100, 128
ADD_GROUPS = [[0, 1], [2]]


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
      bv, bi, vals = gp.acq_argmax('ucb', Xs, params=(1.7, 0.0), mean_const=mean_c, X_halluc=xh, return_vals=True)
      book.put('acq|ucb|m300|const-mean|' + tag, vals, [bv], [bi])
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
      bv, bi, v = add.add_ucb_group(g, 1.3 - 0.6 * g, cands[g], return_vals=True)
      book.put('add_ucb_group|%d|%d' % (g, sizes[g]), v, [bv], [bi])
  # Thompson sampling and the joint draws over three chunks
  for name in ('se', 'm25', 'add'):
    bv, bi, samp, jp = gps[name].thompson(Xl, U1, block=BLOCK, mean_const=mean_c, mean_vals=mv_l, return_samples=True)
    book.put('ts|m1100|' + name, samp, [bv], [bi], powers(jp))
  bv, bi, samp, jp = gps['se'].thompson(Xs, U1[:M_ONE], block=BLOCK, mean_const=mean_c, return_samples=True)
  book.put('ts|m300|const-mean|se', samp, [bv], [bi], powers(jp))
  for name in ('se', 'm25', 'add', 'dup'):
    samp, bvs, bis, jp = gps[name].draw(Xl, U3, 3, BLOCK, Xh, mean_c, mv_l)
    book.put('draw|m1100|q3|S3|' + name, samp, bvs, bis, powers(jp))
  samp, bvs, bis, jp = gps['se'].draw(Xl, U1, 1, BLOCK, Xh, mean_c, mv_l)
  book.put('draw|m1100|q3|S1|se', samp, bvs, bis, powers(jp))
  for ci, cname in enumerate(sorted(CASES)):
    kind, m, block, q, S, dup = CASES[cname]
    cx = uniforms(100 + ci, (m, DIM))
    for row in dup:
      cx[row] = cx[3]
    book.inp('case|%s|Xs' % cname, cx)
    cu = book.inp('case|%s|U' % cname, normals(200 + ci, (m, S)))
    samp, bvs, bis, jp = gps[kind].draw(cx, cu, S, block, Xh[:q] if q else None, mean_c)
    book.put('draw|case|' + cname, samp, bvs, bis, powers(jp))
  # multi-objective: k = 2, both scalarisations, block form / no points in progress; then with a ladder fit among the two
  Uk = book.inp('U2x1100', normals(8, (2, M_CHUNKS)))
  mvk = np.stack((mv_l, 0.5 * mv_l))
  for pair in (('se', 'm25'), ('add', 'dup')):
    two = [gps[pair[0]], gps[pair[1]]]
    for scal in ('lin', 'tch'):
      tag = '%s|%s+%s' % (scal, pair[0], pair[1])
      bv, bi, vals = eng.mo_ucb_argmax(two, scal, 1.1, [0.6, 0.4], [0.05, -0.1], Xl, mean_consts=[mean_c, 0.0], return_vals=True)
      book.put('mo_ucb|' + tag, vals, [bv], [bi])
      bv, bi, vals = eng.mo_ucb_argmax(two, scal, 1.1, [0.6, 0.4], [0.05, -0.1], Xl, mean_vals=mvk, return_vals=True)
      book.put('mo_ucb|mean-vals|' + tag, vals, [bv], [bi])
      for q in (0, 3):
        bv, bi, vals, jp = eng.mo_thompson(two, scal, [0.6, 0.4], [0.05, -0.1], Xl, Uk, block=BLOCK, X_halluc=Xh[:q] if q else None,
                                           mean_consts=[mean_c, 0.0], return_vals=True)
        book.put('mo_ts|q%d|%s' % (q, tag), vals, [bv], [bi], powers(jp))
  for gp in gps.values():
    gp.free()


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
