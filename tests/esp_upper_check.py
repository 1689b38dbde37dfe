"""Run by tests/test_gpu_esp.py in a subprocess (the switches are read per process): an ESP fit at n >= 2048 -- the
lower-triangle-only Gram build -- and what reads its factor afterwards, dumped for comparison across switch settings
(as tests/upper_triangle_check.py for the SE / Matern kernels)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dragonfly_amd.engine import get_engine, KernelSpec   # noqa: E402

n, out = int(sys.argv[1]), sys.argv[2]
eng = get_engine()
rs = np.random.RandomState(n)
d = 7
X = rs.rand(n, d)
Y = np.sin(3 * X.sum(axis=1)) + 0.05 * rs.randn(n)
spec = KernelSpec('esp', d, float(Y.var()), nu=3, sub_kinds=['se', 'matern'] * 3 + ['se'], sub_scales=[1.0] * d,
                  sub_nus=[0.0, 2.5] * 3 + [0.0], sub_bandwidths=[[b] for b in rs.uniform(0.3, 1.0, d)])
gp = eng.gp_fit(spec, X, Y - 0.1, float(Y.var() / 30))
Xs = rs.rand(700, d)
mu, sd = gp.predict(Xs)
np.savez(out, L=np.tril(gp.get_L()), alpha=gp.get_alpha(), lml=gp.lml, mu=mu, sd=sd)
print('OK')
