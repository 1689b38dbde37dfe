"""Writes tests/golden/lml_grad_ref.npz: what the reference's GP.compute_grad_log_marginal_likelihood
(gp/gp_core.py:229-240) returns for SE and Matern (nu = 0.5, 1.5, 2.5) kernels at n = 70, d = 3 -- for 'scale',
'noise_var', 'noise_mean', every ('dim_bandwidths', c) and, on a second kernel with one bandwidth for all dimensions,
'same_dim_bandwidths' -- with its log marginal likelihood, for tests/test_gpu_lml_grad.py.  Runs the real reference on
the CPU; nothing under oracle/ is changed.

    python tools/record_lml_grad_golden.py [/path/to/dragonfly-checkout]   (default: oracle.make_golden.REF)

The reference's kernel gradient indexes the bandwidths as a 2-D array (kernel.py:216, 320) while its constructors keep
them 1-D, so the bandwidths are set on the kernel object as a (1, d) array after construction; nothing else is touched.
The file holds numbers only.  The bandwidth components are in the reference's convention: derivatives in the bandwidth
itself, not in its logarithm.  Each value is printed beside the extended-precision truth of tests/lml_grad_cases.py,
so that a deviation of the reference's own is seen when the file is made.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'lml_grad_ref.npz')
N, D, SEED, NOISE = 70, 3, 11, 1e-2
SAME_BW = 0.5
KERNELS = [('se', 'se', 0.0), ('matern05', 'matern', 0.5), ('matern15', 'matern', 1.5), ('matern25', 'matern', 2.5)]


def main():
  sys.path.insert(0, ROOT)
  sys.path.insert(0, os.path.join(ROOT, 'tests'))
  from oracle.make_golden import import_reference
  if len(sys.argv) > 1:
    os.environ['DRAGONFLY_REFERENCE'] = sys.argv[1]
  import_reference()
  from dragonfly.gp import kernel as ref_kernel
  from dragonfly.gp.gp_core import GP
  import lml_grad_cases as cases

  case = cases.make_case(N, D, SEED, NOISE)
  out = dict(X=case['X'], y=case['y'], bw=case['bw'], scale=case['scale'], noise=case['noise'], mean=case['mean'],
             same_bw=SAME_BW)

  def reference_gp(kind, nu, bw):
    kern = ref_kernel.SEKernel(D, case['scale'], bw) if kind == 'se' else ref_kernel.MaternKernel(D, nu, case['scale'], bw)
    kern.hyperparams['dim_bandwidths'] = np.asarray(bw, dtype=float).reshape(1, -1)
    mean = case['mean']
    return GP(case['X'], case['y'], kern, lambda x: np.array([mean] * len(x)), case['noise'])

  for name, kind, nu in KERNELS:
    gp = reference_gp(kind, nu, case['bw'])
    grad = [gp.compute_grad_log_marginal_likelihood('scale')]
    grad += [gp.compute_grad_log_marginal_likelihood('dim_bandwidths', c) for c in range(D)]
    grad += [gp.compute_grad_log_marginal_likelihood('noise_var'), gp.compute_grad_log_marginal_likelihood('noise_mean')]
    out[name + '_grad'] = np.array(grad, dtype=float)
    out[name + '_lml'] = float(gp.compute_log_marginal_likelihood())
    out[name + '_nu'] = nu
    true_grad, _ = cases.truth(kind, nu, case)
    true_ref = np.asarray(true_grad, dtype=float)
    true_ref[1:D + 1] /= case['bw']
    print(name, 'reference', out[name + '_grad'])
    print(name, 'truth    ', true_ref, 'norm-wise distance %.2e' % (np.max(np.abs(out[name + '_grad'] - true_ref)) / np.max(np.abs(true_ref))))
    same = dict(case, bw=np.full(D, SAME_BW))
    gp = reference_gp(kind, nu, same['bw'])
    out[name + '_same_grad'] = float(gp.compute_grad_log_marginal_likelihood('same_dim_bandwidths'))
    true_same = float(np.sum(cases.truth(kind, nu, same)[0][1:D + 1]) / SAME_BW)
    print(name, 'same_dim_bandwidths: reference', out[name + '_same_grad'], 'truth', true_same)
  np.savez(OUT, **out)
  print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
  main()
