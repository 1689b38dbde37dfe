"""Run in a subprocess by tests/test_gpu_kernmat_digests.py, once per variant (the DFH_KM_* / DFH_PACK_FUSED switches are
read once per process): every route of the kernel-matrix builder -- the single-part symmetric and cross kernels, the
odd-leading-dimension fall-through, the strip kernel with and without the fused posterior mean, the symmetric multi-part
kernel, the seven generic instances, the ESP kernel, dist_squared, the prior diagonal, the two pack routes and the
lower-triangle build of a fit -- on the smallest shapes that reach each route's edges, bit for bit: the SHA-256 of each
output is compared with tests/golden/kernmat_digests.npz.  Every element is computed by one thread in a fixed order and
the fused mean adds its 512-column blocks in a fixed order, so a library returns the same bits on every run.  The inputs
are built by + - * / only from RandomState(seed).random_sample (labels: a polynomial of X; category codes: sums of
comparisons), so their bytes do not depend on the host's libm; each input's digest is stored under 'input|...'.
Prints OK on success.

    kernmat_digest_check.py [--variant NAME]                  compare with the recorded file (the caller sets NAME's switches)
    kernmat_digest_check.py --all [--record FILE]             every variant, each in a child process with its switches set;
                                                              --record writes the digests into FILE (created or updated).
                                                              Record twice into the same file: a key whose second digest
                                                              differs from its first is stored empty -- it did not
                                                              reproduce and is not checked; such keys are findings.

A variant's keys are 'NAME|...'; the default's have no prefix.  'packfused0' (the two-kernel pack) records nothing: the
source promises the bits of the fused pack, so it is held to the default's digests (recorded under its own keys only
where the library the file was recorded with did not keep that promise).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dragonfly_amd.engine import KernelSpec, get_engine      # noqa: E402

DIGESTS = os.path.join(ROOT, 'tests', 'golden', 'kernmat_digests.npz')
GROUPS = ('single_sym', 'odd_ld', 'cross_lds', 'strip', 'mean', 'multi', 'generic', 'esp', 'dist', 'prior', 'lower')
# name -> (the switches, the case groups they touch)
VARIANTS = {
  'default': ({}, GROUPS),
  'cfg1': ({'DFH_KM_CFG': '1'}, ('single_sym',)),
  'cfg2': ({'DFH_KM_CFG': '2'}, ('single_sym',)),
  'waves8': ({'DFH_KM_WAVES': '8'}, ('strip', 'mean')),
  'strip0': ({'DFH_KM_STRIP': '0'}, ('strip', 'mean')),
  'fusedmean0': ({'DFH_KM_FUSED_MEAN': '0'}, ('mean',)),
  'symmulti0': ({'DFH_KM_SYMMULTI': '0'}, ('multi',)),
  'nt1': ({'DFH_KM_NT': '1'}, ('single_sym', 'cross_lds')),
  'lower0': ({'DFH_KM_LOWER_ONLY': '0'}, ('lower',)),
  'packfused0': ({'DFH_PACK_FUSED': '0'}, GROUPS),
}
SAME_AS_DEFAULT = ('packfused0',)
MEAN_C, NOISE = 0.125, 0.01


def uniforms(seed, shape):
  return np.random.RandomState(seed).random_sample(shape)


def codes(u):
  """ category codes 0..3 """
  return (u > 0.25) * 1.0 + (u > 0.5) * 1.0 + (u > 0.75) * 1.0


def poly_labels(X):
  return (X[:, 0] - 0.3) * (X[:, 1] + 0.5) * 2.0 - X[:, 2] * X[:, 2] + 0.25 * X[:, 0] * X[:, 2]


def bws(d, base=0.3):
  return base * (1 + 0.2 * (np.arange(d) % 5))


def se(d):
  return KernelSpec('se', d, 0.5, bws(d))


def matern(d, nu):
  return KernelSpec('matern', d, 0.75, bws(d, 0.5), nu=nu)


def grouped(kind, d, scale, groups, kinds, nus, **kw):
  return KernelSpec(kind, d, scale, groups=groups, sub_kinds=kinds, sub_scales=[1.25 - 0.25 * g for g in range(len(groups))],
                    sub_nus=nus, sub_bandwidths=[0.4 + 0.2 * np.arange(len(g)) for g in groups], **kw)


def hamming_groups(kind, groups, kinds, nus, **kw):
  """ a product whose last group is a Hamming kernel (scale 1, nu 0, weights for bandwidths) """
  sp = grouped(kind, 5, 1.3, groups, kinds, nus, **kw)
  sp.sub_scales = list(sp.sub_scales[:-1]) + [1.0]
  sp.sub_bandwidths = list(sp.sub_bandwidths[:-1]) + [np.array([0.6, 0.4])]
  return sp


def esp(d, order, matern_col=None):
  kinds = ['matern' if c == matern_col else 'se' for c in range(d)]
  return KernelSpec('esp', d, 1.5, nu=order, sub_kinds=kinds, sub_scales=[1.0 - 0.05 * (c % 3) for c in range(d)],
                    sub_nus=[2.5 if k == 'matern' else 0.0 for k in kinds], sub_bandwidths=[[0.5 + 0.1 * (c % 5)] for c in range(d)])


ADD_SE_M25 = lambda: grouped('additive', 5, 1.5, [[0, 1, 2], [3, 4]], ['se', 'matern'], [0.0, 2.5])
ADD_SE_POLY = lambda: grouped('additive', 5, 1.5, [[0, 1, 2], [3, 4]], ['se', 'poly'], [0.0, 2.0])
SE_X_EXPDECAY = lambda: grouped('product', 5, 1.2, [[0], [1, 2, 3, 4]], ['expdecay', 'se'], [0.1, 0.0])


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


class Inputs(object):
  """ X|n|d: uniforms, seeded by the shape; with_codes: the last two columns hold category codes """

  def __init__(self, book):
    self.book, self.have = book, {}

  def __call__(self, n, d, with_codes=False):
    key = 'X|%d|%d%s' % (n, d, '|codes' if with_codes else '')
    if key not in self.have:
      X = uniforms(1000 * d + n, (n, d))
      if with_codes:
        X[:, d - 2:] = codes(X[:, d - 2:])
      self.have[key] = self.book.inp(key, X)
    return self.have[key]


def gram_and_cross(eng, book, X, tag, spec, n, m, d, with_codes=False, cross=True, sym=True):
  if sym:
    book.put('%s|sym%d' % (tag, n), eng.kernel_matrix(spec, X(n, d, with_codes), diag_add=0.01))
  if cross:
    book.put('%s|cross%dx%d' % (tag, m, n), eng.kernel_matrix(spec, X(m, d, with_codes), X(n, d, with_codes)))


def fit(eng, X, spec, n, d):
  Xt = X(n, d)
  return eng.gp_fit(spec, Xt, poly_labels(Xt) - MEAN_C, NOISE)


def run_single_sym(eng, book, X):
  for n in (130, 258):                     # 130: two full 64-tiles and a partial one; 258: the same of the 128-tile
    for tag, spec, d in (('se3', se(3), 3), ('m25d3', matern(3, 2.5), 3), ('se20', se(20), 20)):
      gram_and_cross(eng, book, X, 'single|' + tag, spec, n, 0, d, cross=False)


def run_odd_ld(eng, book, X):
  gram_and_cross(eng, book, X, 'oddld|se3', se(3), 129, 70, 3)


def run_cross_lds(eng, book, X):
  gram_and_cross(eng, book, X, 'crosslds|se3', se(3), 130, 70, 3, sym=False)
  gram_and_cross(eng, book, X, 'crosslds|m35d8', matern(8, 3.5), 130, 70, 8, sym=False)


def run_strip(eng, book, X):
  cases = [('se8', se(8), 8)] + [('m%dd8' % int(10 * nu), matern(8, nu), 8) for nu in (0.5, 1.5, 2.5)]
  cases += [('se%d' % d, se(d), d) for d in (16, 24, 32)]
  for tag, spec, d in cases:
    gram_and_cross(eng, book, X, 'strip|' + tag, spec, 330, 200, d, sym=False)


def run_mean(eng, book, X):
  for tag, spec in (('se8', se(8)), ('m15d8', matern(8, 1.5))):
    gp = fit(eng, X, spec, 600, 8)
    book.put('mean|%s|mean-only' % tag, gp.predict(X(200, 8), want_std=False)[0])
    book.put('mean|%s|with-std' % tag, *gp.predict(X(200, 8)))
    gp.free()


def run_multi(eng, book, X):
  gram_and_cross(eng, book, X, 'multi|add-se-m25', ADD_SE_M25(), 130, 70, 5)
  prod = grouped('product', 5, 1.5, [[0, 1, 2], [3, 4]], ['se', 'matern'], [0.0, 2.5])
  gram_and_cross(eng, book, X, 'multi|prod-se-m25', prod, 130, 70, 5)
  wide = grouped('additive', 20, 1.1, [list(range(17)), [17, 18, 19]], ['se', 'matern'], [0.0, 1.5])
  gram_and_cross(eng, book, X, 'multi|add-17col', wide, 130, 0, 20, cross=False)


def run_generic(eng, book, X):
  nested = grouped('product', 5, 1.4, [[0], [1, 2], [3, 4]], ['se', 'se', 'matern'], [0.0, 0.0, 2.5],
                   group_factors=[0, 1, 1], factor_sums=[False, True], factor_scales=[1.0, 1.7])
  for tag, spec in (('add-se-poly', ADD_SE_POLY()), ('se-x-expdecay', SE_X_EXPDECAY()), ('nested', nested)):
    gram_and_cross(eng, book, X, 'generic|' + tag, spec, 130, 70, 5)
  ham = KernelSpec('hamming', 5, 1.0, np.array([0.3, 0.25, 0.2, 0.15, 0.1]))
  book.put('generic|hamming|sym130', eng.kernel_matrix(ham, codes(X(130, 5)), diag_add=0.01))
  book.put('generic|hamming|cross70x130', eng.kernel_matrix(ham, codes(X(70, 5)), codes(X(130, 5))))
  ham_cases = (
    ('se-x-hamming', hamming_groups('product', [[0, 1, 2], [3, 4]], ['se', 'hamming'], [0.0, 0.0])),
    ('poly-x-hamming', hamming_groups('product', [[0, 1, 2], [3, 4]], ['poly', 'hamming'], [2.0, 0.0])),
    ('nested-hamming', hamming_groups('product', [[0, 1], [2], [3, 4]], ['se', 'matern', 'hamming'], [0.0, 1.5, 0.0],
                                      group_factors=[0, 0, 1], factor_sums=[True, False], factor_scales=[1.3, 1.0])),
  )
  for tag, spec in ham_cases:
    gram_and_cross(eng, book, X, 'generic|' + tag, spec, 130, 70, 5, with_codes=True)


def run_esp(eng, book, X):
  # the five register buckets (orders 2, 3, 7, 9, 17) and both ALL_SE values
  for tag, spec, d in (('d5o2', esp(5, 2), 5), ('d5o3-matern', esp(5, 3, matern_col=1), 5), ('d9o7', esp(9, 7), 9),
                       ('d12o9', esp(12, 9), 12), ('d18o17', esp(18, 17), 18)):
    gram_and_cross(eng, book, X, 'esp|' + tag, spec, 70, 40, d)
  gram_and_cross(eng, book, X, 'esp|d130o2', esp(130, 2), 40, 30, 130)      # more than 64 KiB of LDS


def run_dist(eng, book, X):
  for d in (3, 8):
    book.put('dist|d%d|70x130' % d, eng.dist_squared(X(70, d), X(130, d)))


def run_prior(eng, book, X):
  for tag, spec in (('add-se-poly', ADD_SE_POLY()), ('se-x-expdecay', SE_X_EXPDECAY()), ('esp-d5o2', esp(5, 2))):
    gp = fit(eng, X, spec, 130, 5)
    book.put('prior|%s|predict' % tag, *gp.predict(X(70, 5)))
    gp.free()


def run_lower(eng, book, X):
  for tag, spec, d in (('se3', se(3), 3), ('add-se-m25', ADD_SE_M25(), 5), ('esp-d5o2', esp(5, 2), 5)):
    gp = fit(eng, X, spec, 2050, d)
    book.put('lower|%s|fit2050' % tag, np.tril(gp.get_L()), gp.get_alpha(), [gp.lml])
    gp.free()


RUNNERS = {'single_sym': run_single_sym, 'odd_ld': run_odd_ld, 'cross_lds': run_cross_lds, 'strip': run_strip, 'mean': run_mean,
           'multi': run_multi, 'generic': run_generic, 'esp': run_esp, 'dist': run_dist, 'prior': run_prior, 'lower': run_lower}


def load_digests(path):
  if not os.path.exists(path):
    return {}
  with np.load(path) as z:
    return dict(zip((str(k) for k in z['keys']), (str(d) for d in z['digests'])))


def run_variant(variant, record_to):
  env, groups = VARIANTS[variant]
  for name, val in env.items():
    assert os.environ.get(name) == val, 'variant %s needs %s=%s in the environment' % (variant, name, val)
  book = Book()
  eng = get_engine()
  X = Inputs(book)
  for g in groups:
    RUNNERS[g](eng, book, X)
  known = load_digests(record_to or DIGESTS)
  own = '' if variant == 'default' else variant + '|'
  bad = []
  for key, got in book.got:
    print('%s%s %s' % (own, key, got))
    is_input = key.startswith('input|')
    shared = is_input or variant in SAME_AS_DEFAULT          # held to the default's digest
    name = key if shared and own + key not in known else own + key
    if record_to:
      if shared and variant != 'default':
        if is_input or known.get(key) == got:
          if known.get(key, got) != got:
            bad.append('%s differs from the default run\'s' % key)
          continue
        print('FINDING: %s does not reproduce the default\'s digest of %s; recorded as %s' % (variant, key, own + key))
        name = own + key
      known[name] = got if known.get(name, got) == got else ''
    elif name not in known:
      bad.append('%s is not in tests/golden/kernmat_digests.npz' % name)
    elif not known[name]:
      print('%s did not reproduce when the file was recorded (stored empty): not checked' % name)
    elif known[name] != got:
      bad.append('the bits of %s differ from tests/golden/kernmat_digests.npz: %s, recorded %s' % (name, got, known[name]))
  if record_to:
    keys = sorted(known)
    np.savez_compressed(record_to, keys=np.array(keys), digests=np.array([known[k] for k in keys]))
    print('empty: %s' % sorted(k for k in keys if not known[k]))
  elif variant not in SAME_AS_DEFAULT:
    computed = set(own + k for k, _ in book.got)
    mine = [k for k in known if (k.startswith(own) if own else (k.split('|')[0] not in VARIANTS and not k.startswith('input|')))]
    bad += ['%s is recorded but was not computed' % k for k in sorted(set(mine) - computed)]
  assert not bad, '\n'.join(bad)
  print('OK')


def main():
  args = sys.argv[1:]
  record_to = args[args.index('--record') + 1] if '--record' in args else None
  if '--all' in args:
    for variant in VARIANTS:
      cmd = [sys.executable, os.path.abspath(__file__), '--variant', variant] + (['--record', record_to] if record_to else [])
      res = subprocess.run(cmd, env=dict(os.environ, **VARIANTS[variant][0]), timeout=600)
      if res.returncode != 0:
        sys.exit('variant %s failed (exit status %d)' % (variant, res.returncode))
    print('ALL OK')
    return
  run_variant(args[args.index('--variant') + 1] if '--variant' in args else 'default', record_to)


if __name__ == '__main__':
  main()
