"""Run in a subprocess by tests/test_gpu_lml_route_bits.py, once per variant (the DFH_LML_* switches are read once per
process): what dfh_gp_lml_batch returns -- log marginal likelihoods as uint64, jitter powers, and for the calls that fail
the exception type and its full text -- on the smallest shapes that reach each branch of its route chooser and of its two
schedules, compared with tests/golden/lml_route_bits.npz.  That file was recorded twice with the library of the commit
before the tuning objective's host side was taken apart (DFH_LIB selects a library):

    lml_route_bits_check.py --variant V                  compare with the recorded file (the caller sets V's switches)
    lml_route_bits_check.py --variant V --record FILE    record V into FILE (created or updated)
    lml_route_bits_check.py --all [--record FILE]        every variant, each in a child process with its switches set

A second recording into the same file compares itself with the first: inputs, jitter powers and error texts must be equal;
log marginal likelihoods that differ in a bit get their relative spread stored (0 for a reproducible call), and a later
comparison allows twice that -- two runs bound the spread from below only.  tests/test_gpu_lml_route_bits.py holds the
file itself to: recorded twice, at most two calls with a spread, none above 1e-13.

Inputs come from RandomState(seed).rand and + - * / only (no libm call whose last bit might depend on the host); their
SHA-256 is stored beside the results.  D = 3; candidates are SE, every third one Matern 2.5 (tools/record_lml_bits.py).
A case is a list of calls on one engine; a key is VARIANT__CASE__CALL__{lml, powers, digest, error, spread}.  The lock-step
variant's "no jitter" case at n = 150 is err_wg_nojitter: err_tiny_nojitter's construction at that size is the same input.
Prints OK on success."""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'lml_route_bits.npz')
D = 3
NO_POWER = -2 ** 31

DEFAULT_CASES = ('tiny64_ladder', 'fused_redo', 'fused_device', 'tiny_device', 'fused_refused', 'wg_191', 'wg_192', 'wg_129',
                 'wg_2047', 'wg_host_y_twice', 'psd_try_device_y', 'tiny64_timed', 'err_tiny_nojitter', 'err_wg_nojitter',
                 'err_nan')
LOCKSTEP = {'DFH_LML_WG': '0', 'DFH_LML_TINY': '0'}
# name -> (the switches, the cases they run); plain_N_NB: nb candidates on n points
VARIANTS = {
  'defaults': ({}, DEFAULT_CASES),
  'lockstep': (LOCKSTEP, ('plain_40_3', 'plain_150_5', 'plain_600_5', 'ladder_150', 'err_wg_nojitter')),
  # 600 * 600 * 8 B = 2.88 MB per matrix, 0.006 GiB = 6.44 MB: G = 2, groups of 2, 2, 1
  'lockstep-groups': (dict(LOCKSTEP, DFH_LML_GROUP_GIB='0.006'), ('plain_600_5',)),
  'lockstep-solve-each': ({'DFH_LML_WG': '0', 'DFH_LML_BATCH_SOLVE': '0'}, ('plain_600_3',)),
  'wg-min-batch': ({'DFH_LML_WG_MIN_BATCH': '4'}, ('plain_150_3', 'plain_150_4')),
  'no-teams': ({'DFH_LML_TEAM': '0'}, ('plain_150_5', 'plain_300_3')),
  'teams-of-two': ({'DFH_LML_TEAM': '2'}, ('plain_150_5', 'plain_300_3')),
  'wg-groups-of-two': ({'DFH_LML_WG_GROUP': '2'}, ('plain_150_5',)),
  'no-tiny': ({'DFH_LML_TINY': '0'}, ('plain_40_6', 'plain_100_8')),
  'no-fused': ({'DFH_LML_FUSED': '0'}, ('plain_100_8',)),
  'by-copies': ({'DFH_LML_DIRECT': '0'}, ('plain_40_6', 'plain_100_70')),
  'old-tiny': ({'DFH_LML_TINY64': '0'}, ('plain_40_6',)),
  'fused-255': ({'DFH_LML_FUSED_MAX_N': '255'}, ('plain_200_4',)),
}


def make(seed, n, nb, duplicated=False):
  """ (specs, X, y, means, noises) as tools/record_lml_bits.py builds them; duplicated: the second half of X repeats the
      first, and candidate 1 is a wide SE kernel of scale 1 (singular without noise) """
  from dragonfly_amd.engine import KernelSpec
  rs = np.random.RandomState(seed)
  X = rs.rand(n, D)
  s = X[:, 0] + X[:, 1] + X[:, 2]
  y = (s - 1.5) * (s - 1.5) - X[:, 0] * X[:, 2] + 0.2 * (rs.rand(n) - 0.5)
  if duplicated:
    X[n // 2:2 * (n // 2)] = X[:n // 2]
  specs = []
  for c in range(nb):
    scale, bw = 0.2 + 0.4 * rs.rand(), 0.2 + 0.8 * rs.rand(D)
    specs.append(KernelSpec('matern', D, scale, bw, nu=2.5) if c % 3 == 2 else KernelSpec('se', D, scale, bw))
  means = 0.1 * (rs.rand(nb) - 0.5)
  noises = 0.002 + 0.02 * rs.rand(nb)
  if duplicated and nb > 1:
    specs[1] = KernelSpec('se', D, 1.0, np.full(D, 2.0))
  return specs, X, y, means, noises


def inputs_digest(specs, X, y, means, noises):
  h = hashlib.sha256()
  for a in [X, y, means, noises] + [sp.bandwidths for sp in specs]:
    h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
  h.update(np.array([sp.scale for sp in specs], dtype=np.float64).tobytes())
  return np.frombuffer(h.digest(), dtype=np.uint8).copy()


class Book(object):
  """ the calls of one run, in order: (key, {lml, powers, digest, error}) """

  def __init__(self, engine, prefix):
    self.engine, self.prefix, self.got = engine, prefix, []

  def call(self, tag, inputs, x_dev=False, y_dev=False, **kwargs):
    specs, X, y, means, noises = inputs
    eng = self.engine
    Xa = eng.to_device(X) if x_dev else X
    ya = eng.to_device(y) if y_dev else y
    lml, powers, error = np.zeros(0), np.zeros(0, dtype=np.int64), ''
    try:
      lml, powers = eng.gp_lml_batch(specs, Xa, ya, means, noises, return_powers=True, **kwargs)
      lml = np.array(lml, dtype=np.float64)
      powers = np.array([NO_POWER if p is None else p for p in powers], dtype=np.int64)
    except (np.linalg.LinAlgError, ValueError) as e:
      error = '%s: %s' % (type(e).__name__, e)
    for a in ([Xa] if x_dev else []) + ([ya] if y_dev else []):
      a.free()
    self.got.append((self.prefix + tag, dict(lml=lml, powers=powers, digest=inputs_digest(*inputs), error=np.array(error))))


def ladder_inputs(seed, n, noise1):
  specs, X, y, means, noises = make(seed, n, 3, duplicated=True)
  return specs, X, y, means, np.array([1e-3, noise1, 1e-2])


def run_case(book, name):
  if name.startswith('plain_'):
    n, nb = (int(v) for v in name.split('_')[1:])
    book.call('call', make(7 * n + nb, n, nb))
  elif name == 'tiny64_ladder':                     # the in-kernel ladder and its power
    book.call('call', ladder_inputs(201, 40, 1e-18))
  elif name == 'fused_redo':                        # a candidate of the one-launch small group handed on alone
    book.call('call', ladder_inputs(202, 100, 1e-18))
  elif name == 'ladder_150':
    book.call('call', ladder_inputs(203, 150, 1e-18))
  elif name == 'fused_device':                      # resident labels are downloaded for the staging blob
    book.call('call', make(204, 100, 4), x_dev=True, y_dev=True)
  elif name == 'tiny_device':
    book.call('call', make(205, 100, 70), x_dev=True, y_dev=True)
  elif name == 'fused_refused':                     # a kernel the one-launch forms do not take: the workgroup route at n <= 128
    from dragonfly_amd.engine import KernelSpec
    inputs = make(206, 100, 4)
    inputs[0][1] = KernelSpec('poly', D, 0.5, np.array([0.5, 0.75, 1.0]), nu=2)
    book.call('call', inputs)
  elif name in ('wg_191', 'wg_192'):                # n + 1 fills three tiles exactly; the augmented row alone in the last tile
    book.call('call', make(int(name[3:]), int(name[3:]), 3))
  elif name in ('wg_129', 'wg_2047'):               # first size past the one-launch forms; the workgroup route's last size
    book.call('call', make(int(name[3:]), int(name[3:]), 2))
  elif name == 'wg_host_y_twice':                   # the resident-label cache: miss, hit, miss
    inputs = make(207, 150, 2)
    book.call('first', inputs)
    book.call('same_y', inputs)
    other = make(208, 150, 2)
    book.call('other_y', (inputs[0], inputs[1], other[2], inputs[3], inputs[4]))
  elif name == 'psd_try_device_y':
    book.call('call', make(209, 60, 2), y_dev=True, handle_non_psd_kernels='try_before_project')
  elif name == 'tiny64_timed':                      # section timing switches the copy-free form off
    book.engine.timings(True)
    book.call('call', make(210, 40, 6))
    book.engine.timings(False)
  elif name in ('err_tiny_nojitter', 'err_wg_nojitter'):
    n = 40 if name == 'err_tiny_nojitter' else 150
    inputs = ladder_inputs(211 + n, n, 0.0)
    book.call('fails', inputs, allow_jitter=False)
    book.call('good_after', inputs[:4] + (np.array([1e-3, 1e-3, 1e-2]),))
  elif name == 'err_nan':
    specs, X, y, means, noises = make(212, 150, 1)
    Xnan = X.copy()
    Xnan[3, 1] = np.nan
    book.call('fails', (specs, Xnan, y, means, noises))
    book.call('good_after', (specs, X, y, means, noises))
  else:
    raise KeyError(name)


def rel_spread(a, b):
  return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def run_variant(variant, record_to):
  env, cases = VARIANTS[variant]
  for name, val in env.items():
    assert os.environ.get(name) == val, 'variant %s needs %s=%s in the environment' % (variant, name, val)
  sys.path.insert(0, ROOT)
  from dragonfly_amd.engine import get_engine
  engine = get_engine()
  got = []
  for case in cases:
    book = Book(engine, '%s__%s__' % (variant, case))
    run_case(book, case)
    got += book.got
  path = record_to or GOLDEN
  known = dict(np.load(path, allow_pickle=False)) if os.path.exists(path) else {}
  runs_key = variant + '__runs'
  again = runs_key in known
  bad = []
  for key, res in got:
    print('%s lml=%s powers=%s %s' % (key, res['lml'].tolist(), sorted(set(res['powers'].tolist()) - {NO_POWER}), res['error']),
          flush=True)
    if record_to and not again:
      known.update({key + '__' + f: v for f, v in res.items()})
      known[key + '__spread'] = np.float64(0.0)
      continue
    if key + '__lml' not in known:
      bad.append('%s is not in %s' % (key, path))
      continue
    want = {f: known[key + '__' + f] for f in res}
    if not np.array_equal(want['digest'], res['digest']):
      bad.append('%s: the inputs rebuilt from the seed are not the recorded ones' % key)
    elif str(want['error']) != str(res['error']):
      bad.append('%s: error %r, recorded %r' % (key, str(res['error']), str(want['error'])))
    elif not np.array_equal(want['powers'], res['powers']):
      bad.append('%s: jitter powers %s, recorded %s' % (key, res['powers'], want['powers']))
    elif want['lml'].shape != res['lml'].shape:
      bad.append('%s: %d values, recorded %d' % (key, res['lml'].size, want['lml'].size))
    elif record_to:
      same = np.array_equal(want['lml'].view(np.uint64), res['lml'].view(np.uint64))
      known[key + '__spread'] = np.float64(0.0 if same else rel_spread(want['lml'], res['lml']))
      known[key + '__lml'] = res['lml']
      print('  %s' % ('bit-reproducible' if same else 'run-to-run spread %.3e' % known[key + '__spread']))
    else:
      spread = float(known[key + '__spread'])
      if spread == 0.0 and not np.array_equal(want['lml'].view(np.uint64), res['lml'].view(np.uint64)):
        bad.append('%s: the bits differ: %s, recorded %s' % (key, res['lml'].tolist(), want['lml'].tolist()))
      elif spread > 0.0 and rel_spread(res['lml'], want['lml']) > 2.0 * spread:
        bad.append('%s: beyond twice the recorded spread %.3e: %s, recorded %s' % (key, spread, res['lml'].tolist(), want['lml'].tolist()))
  if not bad:
    mine = set(k[:-len('__lml')] for k in known if k.startswith(variant + '__') and k.endswith('__lml'))
    bad += ['%s is recorded but was not computed' % k for k in sorted(mine - set(k for k, _ in got))]
  assert not bad, '\n'.join(bad)
  if record_to:
    known[runs_key] = np.int64(int(known.get(runs_key, 0)) + 1)
    np.savez_compressed(record_to, **known)
  print('OK')


def main():
  args = sys.argv[1:]
  record_to = args[args.index('--record') + 1] if '--record' in args else None
  if '--all' in args:
    for variant in VARIANTS:
      cmd = [sys.executable, os.path.abspath(__file__), '--variant', variant] + (['--record', record_to] if record_to else [])
      res = subprocess.run(cmd, env=dict(os.environ, **VARIANTS[variant][0]), timeout=300)
      if res.returncode != 0:
        sys.exit('variant %s failed (exit status %d)' % (variant, res.returncode))
    print('ALL OK')
    return
  run_variant(args[args.index('--variant') + 1], record_to)


if __name__ == '__main__':
  main()
