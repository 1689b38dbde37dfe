"""Records what dfh_gp_lml_batch returns, bit for bit, for one small input per route of its dispatcher:
tests/golden/lml_batch_parent_bits.npz, which tests/test_gpu_lml_bits.py holds every later build to.  Run it on an MI355X
at the commit whose behaviour is to be kept (DFH_LIB selects that commit's library):

    python tools/record_lml_bits.py --out first.npz
    python tools/record_lml_bits.py --out tests/golden/lml_batch_parent_bits.npz --previous first.npz

The second run compares itself with the first.  A case that is not bit-reproducible from run to run cannot be held to
bit equality: its observed relative spread is stored (spread_<case>, 0 for a reproducible case) and the test allows
twice that -- two runs bound the spread from below only.

The inputs come from np.random.RandomState(seed).rand and plain arithmetic (no libm call whose last bit might depend
on the host), and their SHA-256 is stored with the results, so a mismatch of the inputs is not taken for one of the
library."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'lml_batch_parent_bits.npz')
D = 3

#        name                    seed   n   nb   route of dfh_gp_lml_batch the case reaches
CASES = [('tiny64',               101,   40,   6),    # one 64 x 64 tile per candidate
         ('fused',                102,  100,   8),    # one-launch small group
         ('tiny',                 103,  100,  70),    # too many candidates for the one-launch small group
         ('wg_team',              104,  150,   5),    # workgroup route, a team of workgroups per candidate
         ('wg_two_groups',        105,  150, 300),    # one workgroup per candidate, more candidates than CUs
         ('wg_ladder',            106,  150,   6),    # candidate 2 falls to the lock-step schedule alone, through the ladder
         ('wg_nonuniform_device', 107,  150,   4),    # additive kernels among plain ones; X and y resident on the device
         ('lockstep_2048',        108, 2048,   2),    # past the workgroup route: the lock-step schedule's batched solve
         ('psd_project_first',    109,   60,   2)]    # a PSD flag: every candidate is a fit of its own


def build_case(name):
  """ (specs, X, y, means, noises, keyword arguments of gp_lml_batch, X / y go to the device first?) """
  from dragonfly_amd.engine import KernelSpec
  _, seed, n, nb = [c for c in CASES if c[0] == name][0]
  rs = np.random.RandomState(seed)
  X = rs.rand(n, D)
  s = X[:, 0] + X[:, 1] + X[:, 2]
  y = (s - 1.5) * (s - 1.5) - X[:, 0] * X[:, 2] + 0.2 * (rs.rand(n) - 0.5)
  if name == 'wg_ladder':
    X[75:] = X[:75]                               # duplicated points: singular without noise
  specs = []
  for c in range(nb):
    scale, bw = 0.2 + 0.4 * rs.rand(), 0.2 + 0.8 * rs.rand(D)
    if name == 'wg_nonuniform_device' and c % 2 == 1:
      specs.append(KernelSpec('additive', D, scale, groups=[[0, 1], [2]], sub_kinds=['se', 'matern'], sub_scales=[1.0, 1.0],
                              sub_nus=[0.0, 2.5], sub_bandwidths=[bw[:2].copy(), bw[2:].copy()]))
    elif c % 3 == 2:
      specs.append(KernelSpec('matern', D, scale, bw, nu=2.5))
    else:
      specs.append(KernelSpec('se', D, scale, bw))
  means = 0.1 * (rs.rand(nb) - 0.5)
  noises = 0.002 + 0.02 * rs.rand(nb)
  if name == 'wg_ladder':
    specs[2] = KernelSpec('se', D, 1.0, np.full(D, 2.0))
    noises[2] = 0.0
  kwargs = {'handle_non_psd_kernels': 'project_first'} if name == 'psd_project_first' else {}
  return specs, X, y, means, noises, kwargs, name == 'wg_nonuniform_device'


def inputs_digest(specs, X, y, means, noises):
  h = hashlib.sha256()
  for a in [X, y, means, noises] + [sp.bandwidths for sp in specs if sp.bandwidths is not None] + \
           [b for sp in specs if sp.sub_bandwidths is not None for b in sp.sub_bandwidths]:
    h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
  h.update(np.array([sp.scale for sp in specs], dtype=np.float64).tobytes())
  return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def run_case(engine, name):
  """ (lml [nb] float64, powers [nb] int64 with INT32_MIN for none, digest of the inputs) """
  specs, X, y, means, noises, kwargs, on_device = build_case(name)
  digest = inputs_digest(specs, X, y, means, noises)
  Xa, ya = (engine.to_device(X), engine.to_device(y)) if on_device else (X, y)
  lml, powers = engine.gp_lml_batch(specs, Xa, ya, means, noises, return_powers=True, **kwargs)
  if on_device:
    Xa.free(); ya.free()
  return np.array(lml, dtype=np.float64), np.array([-2 ** 31 if p is None else p for p in powers], dtype=np.int64), digest


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
  ap.add_argument('--out', default=GOLDEN)
  ap.add_argument('--previous', default=None, help='the file an earlier run wrote: compare, and store the spread')
  args = ap.parse_args()
  sys.path.insert(0, ROOT)
  from dragonfly_amd.engine import get_engine
  engine = get_engine()
  prev = dict(np.load(args.previous, allow_pickle=False)) if args.previous else None
  out = {'names': np.array([c[0] for c in CASES]), 'seeds': np.array([c[1] for c in CASES], dtype=np.int64)}
  for name, _, n, nb in CASES:
    lml, powers, digest = run_case(engine, name)
    spread = 0.0
    if prev is not None:
      assert np.array_equal(prev['digest_' + name], digest), 'the two runs did not see the same inputs: %s' % name
      assert np.array_equal(prev['powers_' + name], powers), 'jitter powers differ between two runs: %s' % name
      if not np.array_equal(prev['lml_' + name].view(np.uint64), lml.view(np.uint64)):
        spread = float(np.max(np.abs(prev['lml_' + name] - lml) / np.abs(lml)))
    out['lml_' + name], out['powers_' + name], out['digest_' + name] = lml, powers, digest
    out['spread_' + name] = np.float64(spread)
    print('%-22s n=%4d nb=%3d lml[0]=%.17g powers=%s %s' % (
        name, n, nb, lml[0], sorted(set(powers.tolist()) - {-2 ** 31}),
        '' if prev is None else ('bit-reproducible' if spread == 0.0 else 'run-to-run spread %.3e' % spread)), flush=True)
  np.savez(args.out, **out)
  print('wrote %s' % args.out)


if __name__ == '__main__':
  main()
