"""Writes tests/golden/cp_acq_n70.npz: what the reference computes, ONE POINT PER CALL, when it maximises an
acquisition over random samples of a Cartesian-product domain (opt/gpb_acquisitions.py:35-37, exd/exd_utils.py:265) --
per candidate the posterior (gp.eval([x], 'std'), or eval_with_hallucinated_observations with two points in progress),
the UCB / EI / PI / TTEI values, and the one-point Thompson draw gp.draw_samples(1, [x]) -- for
tests/test_gpu_cp_acq.py.  Runs the real reference on the CPU; nothing under oracle/ is changed.

    python tools/record_cp_acq_golden.py [/path/to/dragonfly-checkout]   (default: oracle.make_golden.REF)

The GP: 70 points of a mixed domain -- a 2-D SE part, an integer Matern-2.5 part, a Hamming part of two columns --
fitted with 'project_first' as every CPGP is.  257 candidates, candidate DUP_CAND equal to training point DUP_TRAIN.
The file holds numbers only: the points packed into the dense layout of the kernel's descriptor (categories as integer
codes), hyper-parameters, normals, and the reference's values, winners and top-two gaps.  Every arg-max is checked here to
be decided by more than MIN_GAP of the largest value; a seed that fails the check is replaced, never tolerated.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')
N, M, Q = 70, 257, 2
DUP_CAND, DUP_TRAIN = 100, 17
SEED = 20240611
MIN_GAP = 1e-8
SCALE, SE_BW, MATERN_BW, HAMMING_W = 1.7, [0.45, 0.8], [2.5], [0.6, 0.4]
NOISE = 0.02


def points(rng, n):
  """ list-of-lists points and the same packed: [x0, x1 | k | c0, c1] """
  x = rng.random_sample((n, 2))
  k = rng.randint(1, 8, size=(n, 1))
  c = rng.randint(0, 3, size=(n, 2))
  packed = np.hstack([x, k.astype(float), c.astype(float)])
  return [[x[i].copy(), [int(k[i, 0])], [int(c[i, 0]), int(c[i, 1])]] for i in range(n)], packed


def objective(packed):
  return np.sin(3 * packed[:, 0]) + packed[:, 1] ** 2 - 0.05 * (packed[:, 2] - 4) ** 2 + 0.3 * (packed[:, 3] == packed[:, 4])


def top2(vals):
  """ (winner by np.argmax, gap between the two largest values relative to the largest magnitude) """
  vals = np.asarray(vals, dtype=float)
  order = np.sort(vals)
  return int(np.argmax(vals)), float((order[-1] - order[-2]) / np.max(np.abs(vals)))


def main():
  sys.path.insert(0, ROOT)
  from oracle.make_golden import import_reference
  if len(sys.argv) > 1:
    os.environ['DRAGONFLY_REFERENCE'] = sys.argv[1]
  import_reference()
  from scipy.stats import norm as normal_distro
  from dragonfly.gp import kernel as ref_kernel
  from dragonfly.gp.cartesian_product_gp import CPGP
  rng = np.random.RandomState(SEED)
  X, Xp = points(rng, N)
  Y = objective(Xp) + 0.05 * rng.standard_normal(N)
  C, Cp = points(rng, M)
  C[DUP_CAND], Cp[DUP_CAND] = X[DUP_TRAIN], Xp[DUP_TRAIN]
  H, Hp = points(rng, Q)
  mean_c = float(np.mean(Y))
  kern = ref_kernel.CartesianProductKernel(SCALE, [ref_kernel.SEKernel(2, 1.0, SE_BW), ref_kernel.MaternKernel(1, 2.5, 1.0, MATERN_BW),
                                                   ref_kernel.HammingKernel(HAMMING_W)])
  gp = CPGP(X, list(Y), kern, lambda x: np.array([mean_c] * len(x)), NOISE, handle_non_psd_kernels='project_first')
  assert kern.is_guaranteed_psd()
  t = N + 1
  beta = float(np.sqrt(0.5 * 3.0 * np.log(2 * 3.0 * t + 1)))       # _get_ucb_beta_th with the dimension of a kernel without `dim`
  best = float(np.max(Y))
  ei_norm = lambda z: z * normal_distro.cdf(z) + normal_distro.pdf(z)
  out = dict(Xp=Xp, Y=Y, Cp=Cp, Hp=Hp, mean_const=mean_c, noise=NOISE, scale=SCALE, se_bw=np.array(SE_BW), matern_bw=np.array(MATERN_BW),
             hamming_w=np.array(HAMMING_W), dup_cand=DUP_CAND, dup_train=DUP_TRAIN, min_gap=MIN_GAP)
  np.random.seed(SEED + 1)
  out['U'] = U = np.random.normal(size=M)
  for q in (0, Q):
    tag = 'q%d' % q
    if q:
      one = lambda x: gp.eval_with_hallucinated_observations([x], H, uncert_form='std')
      draw = lambda x: gp.draw_samples_with_hallucinated_observations(1, [x], H)
    else:
      one = lambda x: gp.eval([x], uncert_form='std')
      draw = lambda x: gp.draw_samples(1, [x])
    post = [one(x) for x in C]
    mu = np.array([float(p[0][0]) for p in post])
    sd = np.array([float(p[1][0]) for p in post])
    ref_mean, ref_std = mu[3], sd[3]                      # TTEI's reference point: candidate 3
    vals = {'ucb': mu + beta * sd,
            'ei': sd * ei_norm((mu - best) / sd),
            'pi': normal_distro.cdf((mu - best) / sd)}
    comb = np.sqrt(ref_std ** 2 + sd ** 2)
    vals['ttei'] = comb * ei_norm((mu - ref_mean) / comb)
    params = {'ucb': (beta, 0.0), 'ei': (best, 0.0), 'pi': (best, 0.0), 'ttei': (ref_mean, ref_std)}
    # the m one-point draws consume the global stream as one np.random.normal(size=m) does: U is what they drew
    np.random.seed(SEED + 1)
    vals['ts'] = np.array([float(np.ravel(draw(x))[0]) for x in C])
    assert np.array_equal(vals['ts'], sd * U + mu) or np.max(np.abs(vals['ts'] - (sd * U + mu))) < 1e-12
    out['mu_' + tag], out['sd_' + tag] = mu, sd
    for name, v in vals.items():
      win, gap = top2(v)
      assert np.all(np.isfinite(v)), (name, tag)
      assert gap > MIN_GAP, 'top-two gap %.2e of %s (%s): choose another seed' % (gap, name, tag)
      out['%s_%s' % (name, tag)], out['%s_win_%s' % (name, tag)], out['%s_gap_%s' % (name, tag)] = v, win, gap
      if name in params:
        out['%s_params_%s' % (name, tag)] = np.array(params[name])
      print('%-5s %s winner %3d gap %.3e' % (name, tag, win, gap))
  np.savez_compressed(os.path.join(OUT, 'cp_acq_n70.npz'), **out)
  print('wrote', os.path.join(OUT, 'cp_acq_n70.npz'), os.path.getsize(os.path.join(OUT, 'cp_acq_n70.npz')), 'bytes')


if __name__ == '__main__':
  main()
