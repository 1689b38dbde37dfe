"""Writes tests/golden/esp_*.npz: the reference's ESP kernels (dragonfly/gp/kernel.py:671-744) on small inputs,
for tests/test_gpu_esp.py.  Runs the real reference on the CPU (oracle.make_golden.import_reference: its NumPy-2
shim); nothing under oracle/ is changed.

    python tools/make_esp_golden.py [/path/to/dragonfly-checkout]   (default: oracle.make_golden.REF)

Kernel matrices (X2 = X1 and rectangular); two fitted GPs (K + noise I, L, alpha, lml, mu / sd / covariance at test
points, the hallucinated sd, the UCB / EI / PI / TTEI values, the points the reference's asynchronous acquisitions
recommend under a seed, a joint Thompson draw with its normals); and the reference's stand-alone EuclideanGPFitter
with kernel_type='esp' (se / matern members, tuned and fixed order, ML by 'rand' and 'pdoo', posterior sampling),
seeded: the chosen hyper-parameters, order, nu and lml.
"""
import os
import sys

from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')

# (name, member kind, dim, order, nu list or None, n1, n2)
KERNEL_CASES = [
  ('se_d6_o1', 'se', 6, 1, None, 40, 23),
  ('se_d6_o2', 'se', 6, 2, None, 40, 23),
  ('se_d6_o3', 'se', 6, 3, None, 40, 23),
  ('se_d6_o6', 'se', 6, 6, None, 40, 23),
  ('m05_d5_o2', 'matern', 5, 2, [0.5] * 5, 37, 19),
  ('m05_d5_o5', 'matern', 5, 5, [0.5] * 5, 37, 19),
  ('m15_d5_o2', 'matern', 5, 2, [1.5] * 5, 37, 19),
  ('m15_d5_o5', 'matern', 5, 5, [1.5] * 5, 37, 19),
  ('m25_d5_o2', 'matern', 5, 2, [2.5] * 5, 37, 19),
  ('m25_d5_o5', 'matern', 5, 5, [2.5] * 5, 37, 19),
  ('mix_d4_o3', 'matern', 4, 3, [0.5, 2.5, 1.5, 2.5], 33, 17),
  ('se_d20_o10', 'se', 20, 10, None, 30, 14),
  ('se_d20_o20', 'se', 20, 20, None, 30, 14),
]
# (name, member kind, dim, order, nu, n, m test points)
GP_CASES = [
  ('gp_se_d6_o2', 'se', 6, 2, None, 60, 25),
  ('gp_m25_d5_o3', 'matern', 5, 3, 2.5, 80, 25),
]


def _kernel(gk, kind, dim, order, nus, rng):
  bws = np.exp(rng.uniform(np.log(0.2), np.log(2.0), dim))
  scale = float(np.exp(rng.uniform(-1.0, 1.0)))
  if kind == 'se':
    return gk.ESPKernelSE(dim, scale, order, bws), scale, bws
  return gk.ESPKernelMatern(dim, nus, scale, order, bws), scale, bws


# (name, fitter options): d = 4, n = 30 (esp_order -1: tuned over 1..4)
FITTER_CASES = [
  ('se_tuned_rand', dict(esp_kernel_type='se', esp_order=-1, ml_hp_tune_opt='rand', hp_tune_max_evals=30)),
  ('se_o2_pdoo', dict(esp_kernel_type='se', esp_order=2, ml_hp_tune_opt='pdoo', hp_tune_max_evals=40)),
  ('matern_tuned_rand', dict(esp_kernel_type='matern', esp_order=-1, ml_hp_tune_opt='rand', hp_tune_max_evals=12)),
  ('matern_o3_nu25_pdoo', dict(esp_kernel_type='matern', esp_order=3, esp_matern_nu=2.5, ml_hp_tune_opt='pdoo',
                               hp_tune_max_evals=40)),
  ('se_tuned_post', dict(esp_kernel_type='se', esp_order=-1, hp_tune_criterion='post_sampling', post_hp_tune_burn=8)),
  ('matern_tuned_post', dict(esp_kernel_type='matern', esp_order=-1, hp_tune_criterion='post_sampling',
                             post_hp_tune_burn=8)),
]
FITTER_SEED = 31337
ASY_ACQS = ['ucb', 'ei', 'pi', 'ttei', 'ts']


def fitter_options(opts):
  """ the options of a fitter case, as both fitters take them """
  out = dict(kernel_type='esp', hp_tune_criterion='ml')
  out.update(opts)
  return out


def fitter_data():
  rs = np.random.RandomState(404)
  X = rs.random_sample((30, 4))
  return X, np.sin(3 * X.sum(axis=1)) + 0.05 * rs.randn(30)


def fitter_record(kind, gp, hps):
  """ what a fitter case keeps of fit_gp's result """
  kern = gp.kernel
  return dict(kind=kind, cts=np.array(np.ravel(hps[0]), dtype=float), dscr=np.array(np.ravel(hps[1]), dtype=float),
              lml=gp.compute_log_marginal_likelihood(), noise=gp.noise_var, scale=kern.hyperparams['scale'],
              order=int(kern.hyperparams['order']),
              nu=float(kern.kernel_list[0].hyperparams.get('nu', 0.0)),
              bws=np.array([float(np.ravel(k.hyperparams['dim_bandwidths'])[0]) for k in kern.kernel_list]))


def main(ref_path):
  sys.path.insert(0, ROOT)
  from oracle import make_golden
  make_golden.REF = ref_path
  make_golden.import_reference()
  from dragonfly.gp import kernel as gk
  from dragonfly.gp.euclidean_gp import EuclideanGP
  from dragonfly.opt import gpb_acquisitions as A
  from dragonfly.exd.domains import EuclideanDomain
  rng = np.random.RandomState(2016)
  for name, kind, dim, order, nus, n1, n2 in KERNEL_CASES:
    kern, scale, bws = _kernel(gk, kind, dim, order, nus, rng)
    X1, X2 = rng.random_sample((n1, dim)), rng.random_sample((n2, dim))
    np.savez_compressed(os.path.join(OUT, 'esp_kernel_%s.npz' % (name)), kind=kind, dim=dim, order=order, scale=scale,
                        bws=bws, nus=np.array(nus if nus else [0.0] * dim), X1=X1, X2=X2, K11=kern(X1, X1), K12=kern(X1, X2))
    print('wrote esp_kernel_%s' % (name))
  for name, kind, dim, order, nu, n, m in GP_CASES:
    kern, scale, bws = _kernel(gk, kind, dim, order, [nu] * dim if nu else None, rng)
    X = rng.random_sample((n, dim))
    Y = np.sin(3 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    Xt = rng.random_sample((m, dim))
    noise, mean = 0.05, float(np.median(Y))
    gp = EuclideanGP(list(X), list(Y), kern, lambda x, _c=mean: np.array([_c] * len(x)), noise)
    mu, cov = gp.eval(list(Xt), uncert_form='covar')
    _, sd = gp.eval(list(Xt), uncert_form='std')
    K = kern(X, X) + noise * np.eye(n)
    Xh = rng.random_sample((3, dim))
    _, sd_h = gp.eval_with_hallucinated_observations(list(Xt), list(Xh), 'std')
    out = dict(kind=kind, dim=dim, order=order, scale=scale, bws=bws, nu=nu if nu else 0.0, X=X, Y=Y, Xt=Xt,
               noise=noise, mean=mean, K=K, L=gp.L, alpha=gp.alpha, lml=gp.compute_log_marginal_likelihood(), mu=mu,
               sd=sd, cov=cov, Xh=Xh, sd_h=sd_h)
    # acquisition values from the reference's formulas, its asynchronous acquisitions ('rand' maximiser) under a seed
    best = float(Y.max())
    beta = A._get_ucb_beta_th(A._get_gp_ucb_dim(gp), n)            # pylint: disable=protected-access
    nd = (mu - best) / sd
    comb = np.sqrt(0.3 ** 2 + sd ** 2)
    out.update(beta_th=beta, val_ucb=mu + beta * sd, val_pi=A.normal_distro.cdf(nd),
               val_ei=sd * A._expected_improvement_for_norm_diff(nd),                              # pylint: disable=protected-access
               val_ttei=comb * A._expected_improvement_for_norm_diff((mu - best) / comb))          # pylint: disable=protected-access
    bounds = np.array([[0.0, 1.0]] * dim)
    def anc(max_evals, in_progress=()):
      return Namespace(max_evals=max_evals, t=n, domain=EuclideanDomain(bounds), curr_max_val=best,
                       eval_points_in_progress=list(in_progress), acq_opt_method='rand', handle_parallel='halluc',
                       is_mf=False, domain_bounds=bounds)
    ci = [c[0] for c in GP_CASES].index(name)
    for ai, acq in enumerate(ASY_ACQS):
      np.random.seed(5100 + 10 * ci + ai)
      out['asy_' + acq] = getattr(A.asy, acq)(gp, anc(64))
    np.random.seed(6100 + ci)
    out['asy_ucb_halluc'] = A.asy.ucb(gp, anc(64, in_progress=[Xh[0], Xh[1]]))
    # a joint Thompson draw: the normals it consumes from np.random, recorded
    np.random.seed(9100 + ci)
    out['ts_U'] = np.random.RandomState(9100 + ci).normal(size=(m, 1)).ravel()
    out['ts_sample'] = gp.draw_samples(1, list(Xt)).ravel()
    np.savez_compressed(os.path.join(OUT, 'esp_%s.npz' % (name)), **out)
    print('wrote esp_%s' % (name))
  from dragonfly.gp.euclidean_gp import EuclideanGPFitter
  from dragonfly.utils.option_handler import load_options
  from dragonfly.gp import euclidean_gp as ref_egp
  X, Y = fitter_data()
  res = dict(X=X, Y=Y)
  for name, opts in FITTER_CASES:
    np.random.seed(FITTER_SEED)
    options = load_options(ref_egp.euclidean_gp_args, partial_options=Namespace(**fitter_options(opts)))
    fitter = EuclideanGPFitter(list(X), list(Y), options=options)
    kind, gp, hps = fitter.fit_gp()
    for k, v in fitter_record(kind, gp, hps).items():
      res[name + '__' + k] = v
    print('fitted %s: %s order %d nu %g lml %.6f' % (name, kind, res[name + '__order'], res[name + '__nu'],
                                                     res[name + '__lml']))
  np.savez_compressed(os.path.join(OUT, 'esp_fitter_d4_n30.npz'), **res)
  print('wrote esp_fitter_d4_n30')


def make_golden_default_ref():
  sys.path.insert(0, ROOT)
  from oracle import make_golden
  return make_golden.REF


if __name__ == '__main__':
  main(sys.argv[1] if len(sys.argv) > 1 else make_golden_default_ref())
