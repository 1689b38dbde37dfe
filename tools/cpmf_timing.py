"""Times BOCA's decision step and a tuning batch of a multi-fidelity GP on a Cartesian-product domain, and writes
profiles/cpmf_boca_timing.json.

    python tools/cpmf_timing.py host [out.json] [/path/to/dragonfly-checkout]     the route before cp_multi_fidelity
    python tools/cpmf_timing.py device [out.json]                                 the device routes, on the MI355X

Two phases, because the two routes need different things.  `host`: before install(cp_multi_fidelity=True) existed, a
multi-fidelity run on a product domain was the reference's own CPMFGP whatever else was installed -- NumPy Gram
matrices, an eigh projection and a Cholesky per candidate, one eval_at_fidel per point -- and touched no GPU; it is timed
with the unmodified reference wherever that is importable.  `device`: the new routes on the GPU -- the fused step
(install(..., boca=True, cp_acquisitions=True, cp_multi_fidelity=True)), the per-point step on the device posterior
(cp_multi_fidelity alone), and one dfh_gp_lml_batch call of 64 nested candidates with the projection flag -- the two
device steps alternating in one process.  Each phase merges its figures into the file and names the host they were
taken on: when the phases ran on different hosts the host figure is an indication, not one side of a same-host
comparison.

The data: fixture A's spaces of tools/record_cpmf_golden.py (fidelity: SE + Hamming of 2 columns; domain: Matern 2.5 on
three columns, an integral SE column, Hamming of 9 columns), n = 200 and 1000 training pairs, 2000 candidates, 12
candidate fidelities.  Every figure: one warm-up, then the median of REPEATS runs that end in a device synchronise;
the spread (max - min) / min is kept beside it.  The host phase times each of the 64 candidates of the tuning batch on
its own (64 fits, their sum is the batch) after one warm-up fit.
"""
import importlib.util
import json
import os
import platform
import sys
import time
from argparse import Namespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_EVALS, REPEATS, BATCH, SIZES = 2000, 5, 64, (200, 1000)


def _recorder():
  spec = importlib.util.spec_from_file_location('record_cpmf_golden', os.path.join(ROOT, 'tools', 'record_cpmf_golden.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def data(n):
  """ fixture A's spaces: training pairs, labels, candidates, fidel_to_opt, candidate fidelities, as lists and packed """
  R = _recorder()
  fx = R.FIXTURES['A']
  rng = np.random.RandomState(1000 + n)
  ZZ, Zp = R.space_points(rng, fx['fidel'], n)
  XX, Xp = R.space_points(rng, fx['domain'], n)
  Y = R.objective(Zp, Xp) + 0.05 * rng.standard_normal(n)
  C, _ = R.space_points(rng, fx['domain'], MAX_EVALS)
  f2o, _ = R.space_points(rng, fx['fidel'], 1)
  FZ, _ = R.space_points(rng, fx['fidel'], R.F)
  cost_ratios = np.sort(0.05 + 0.9 * rng.random_sample(R.F))
  gaps = 0.1 + rng.random_sample(R.F)
  return R, fx, dict(ZZ=ZZ, XX=XX, Y=Y, C=C, f2o=f2o[0], FZ=FZ, cost_ratios=cost_ratios, gaps=gaps, noise=float(np.var(Y) / 20),
                     mean=float(np.mean(Y)), packed=np.hstack([Zp, Xp]))


def candidate_hyperparams(fx, rs):
  """ one tuning candidate: (kernel scale, per part the per-column parameters), drawn around the fixture's """
  jitter = lambda par: list(np.asarray(par, dtype=float) * np.exp(rs.uniform(-0.5, 0.5, size=len(par))))
  return float(fx['kernel_scale'] * np.exp(rs.uniform(-0.5, 0.5))), \
         [[part[:2] + (jitter(part[2]),) + part[3:] for part in fx[space]] for space in ('fidel', 'domain')]


class Caller(object):
  def __init__(self, d):
    self.fidel_to_opt, self.d = d['f2o'], d

  def get_candidate_fidels_and_cost_ratios(self, point, filter_by_cost=True):     # pylint: disable=unused-argument
    return list(self.d['FZ']), list(self.d['cost_ratios'])

  def get_information_gap(self, fidels):
    return list(self.d['gaps'])


class CPDomain(object):
  def get_type(self):
    return 'cartesian_product'


def anc_data(d, acq):
  return Namespace(domain=CPDomain(), acq_opt_method='rand', max_evals=MAX_EVALS, t=len(d['Y']) + 1, is_mf=True, curr_acq=acq,
                   handle_parallel='halluc', eval_points_in_progress=[], eval_fidel_points_in_progress=[],
                   curr_max_val=float(np.max(d['Y'])), boca_thresh_coeff=2.5, y_range=float(np.ptp(d['Y'])),
                   boca_max_low_fidel_cost_ratio=0.9)


def figure(samples_ms):
  s = [float(v) for v in samples_ms]
  return dict(median_ms=round(float(np.median(s)), 3), spread=round((max(s) - min(s)) / min(s), 4), repeats=len(s),
              samples_ms=[round(v, 3) for v in s] if len(s) <= 8 else None)


def repeat(fn, sync=lambda: None, repeats=REPEATS):
  fn()
  out = []
  for _ in range(repeats):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    out.append((time.perf_counter() - t0) * 1e3)
  return figure(out)


def merge(path, phase, host, rows):
  doc = {}
  if os.path.exists(path):
    with open(path) as f:
      doc = json.load(f)
  doc['what'] = ('one BOCA step (2000 candidates, 12 candidate fidelities) and one 64-candidate tuning batch of a multi-fidelity '
                 'GP on a Cartesian-product domain; wall-clock ms, median of the repeats after a warm-up, every run ended by a '
                 'device synchronise; spread = (max - min) / min')
  doc[phase] = dict(host=host, rows=rows)
  if 'host' in doc and 'device' in doc:         # (a host without a GPU cannot be the one the device phase ran on)
    doc['same_host'] = doc['host']['host']['gpu'] == doc['device']['host']['gpu']
  os.makedirs(os.path.dirname(path), exist_ok=True)
  with open(path, 'w') as f:
    json.dump(doc, f, indent=1)
  print('wrote', path)


def _gpu_name():
  """ the device of this host, or None: the host phase needs none """
  from dragonfly_amd import _lib
  try:
    if _lib.device_count() == 0:
      return None
    from dragonfly_amd.engine import get_engine
    return get_engine().name()
  except Exception:           # pylint: disable=broad-except
    return None


def host_phase(path):
  from oracle.make_golden import import_reference
  import_reference()
  from dragonfly.gp import kernel as ref_kernel
  from dragonfly.gp.cartesian_product_gp import CPMFGP
  import dragonfly.opt.gpb_acquisitions as ref_acq
  rows = []
  for n in SIZES:
    R, fx, d = data(n)
    mean_func = lambda x, _c=d['mean']: np.array([_c] * len(x))
    def build(scale, parts):
      return CPMFGP(d['ZZ'], d['XX'], list(d['Y']), None, mean_func, d['noise'], scale, R.build_kernel(ref_kernel, fx['fidel_scale'], parts[0]),
                    R.build_kernel(ref_kernel, fx['domain_scale'], parts[1]), [None] * len(parts[0]), [None] * len(parts[1]))
    gp = build(fx['kernel_scale'], [fx['fidel'], fx['domain']])
    def pinned(acq_fn, anc, *args, **kwargs):               # pylint: disable=unused-argument
      vals = [float(np.ravel(acq_fn([x]))[0]) for x in d['C'][:anc.max_evals]]
      return d['C'][int(np.argmax(vals))]
    saved, ref_acq.maximise_acquisition = ref_acq.maximise_acquisition, pinned
    try:
      for acq in ('ucb', 'ts'):
        def step(_acq=acq):
          np.random.seed(5)
          return ref_acq.boca(getattr(ref_acq.asy, _acq), gp, anc_data(d, _acq), Caller(d))
        rows.append(dict(row='boca step, %s' % acq, n=n, route='reference CPMFGP, one point per call (NumPy)', **repeat(step)))
        print(json.dumps(rows[-1]), flush=True)
    finally:
      ref_acq.maximise_acquisition = saved
    rs = np.random.RandomState(7)
    cands = [candidate_hyperparams(fx, rs) for _ in range(BATCH)]
    build(*cands[0]).compute_log_marginal_likelihood()
    per = []
    for scale, parts in cands:
      t0 = time.perf_counter()
      build(scale, parts).compute_log_marginal_likelihood()
      per.append((time.perf_counter() - t0) * 1e3)
    rows.append(dict(row='tuning batch, %d candidates' % BATCH, n=n, route='reference CPMFGP, one fit per candidate (NumPy Gram, eigh, Cholesky)',
                     batch_ms=round(float(np.sum(per)), 3), per_candidate=figure(per)))
    print(json.dumps(rows[-1]), flush=True)
  merge(path, 'host', dict(machine=platform.machine(), cpus=os.cpu_count(), gpu=_gpu_name()), rows)


def device_phase(path):
  from dragonfly_amd import gpb_acquisitions as A, cartesian_product_gp as cpgp, kernel as K
  from dragonfly_amd.engine import get_engine
  from dragonfly_amd.mf_gp import MFGP
  engine = get_engine()

  class PackedCPMFGP(MFGP):
    """ the hooks of the class device_cpmfgp_class makes (its body is the reference's, which is not needed here) """
    _generic = False

    def _points_array(self, pts):
      return self.kernel.pack(pts)
  cpgp._mf_classes['timing'] = PackedCPMFGP                    # pylint: disable=protected-access

  def mirror(factor_scale, parts):
    members = [K.SEKernel(p[1], 1.0, p[2]) if p[0] == 'se' else K.MaternKernel(p[1], p[3], 1.0, p[2]) if p[0] == 'matern'
               else K.HammingKernel(p[2]) for p in parts]
    return K.CartesianProductKernel(factor_scale, members)
  rows = []
  for n in SIZES:
    _, fx, d = data(n)
    fidel, domain = mirror(fx['fidel_scale'], fx['fidel']), mirror(fx['domain_scale'], fx['domain'])
    gp = PackedCPMFGP(d['ZZ'], d['XX'], list(d['Y']), K.CartesianProductKernel(fx['kernel_scale'], [fidel, domain]),
                      lambda x, _c=d['mean']: np.array([_c] * len(x)), d['noise'], handle_non_psd_kernels='project_first')
    gp.domain_kernel = domain
    A._cp_candidates = lambda anc, _c=d['C']: _c[:anc.max_evals]      # pylint: disable=protected-access
    view = A.FidelToOptGP(gp, d['f2o'])
    for acq in ('ucb', 'ts'):
      anc = anc_data(d, acq)
      assert A.cp_boca_applies(gp, anc) and A.cp_boca_view_applies(acq, view, anc)
      def fused(_acq=acq, _anc=anc):
        np.random.seed(5)
        return A.boca(getattr(A.asy, _acq), gp, _anc, Caller(d))
      def per_point(_acq=acq, _anc=anc):
        # what the reference's callable does with the view when the BOCA flags are off: one device call per point
        np.random.seed(5)
        if _acq == 'ucb':
          beta = A._get_ucb_beta_th(A._get_gp_ucb_dim(view), _anc.t)      # pylint: disable=protected-access
          select = lambda v, a: d['C'][int(np.argmax([float((lambda ms: ms[0][0] + beta * ms[1][0])(v.eval([x], uncert_form='std')))
                                                       for x in d['C']]))]
        else:
          select = lambda v, a: d['C'][int(np.argmax([float(np.ravel(v.draw_samples(1, [x]))[0]) for x in d['C']]))]
        return A.boca(select, gp, _anc, Caller(d))
      same = fused()[1] is per_point()[1] if acq == 'ucb' else None
      # alternating, as two versions compared in one call should be
      t_fused, t_point = [], []
      for _ in range(REPEATS):
        for fn, out in ((fused, t_fused), (per_point, t_point)):
          engine.sync()
          t0 = time.perf_counter()
          fn()
          engine.sync()
          out.append((time.perf_counter() - t0) * 1e3)
      rows.append(dict(row='boca step, %s' % acq, n=n, route='device posterior, one call per point', **figure(t_point)))
      rows.append(dict(row='boca step, %s' % acq, n=n, route='fused: one acq_argmax / thompson_pointwise + one predict',
                       same_point_as_per_point=same, **figure(t_fused)))
      print(json.dumps(rows[-2]), json.dumps(rows[-1]), flush=True)
    rs = np.random.RandomState(7)
    specs = []
    for scale, parts in [candidate_hyperparams(fx, rs) for _ in range(BATCH)]:
      specs.append(K.CartesianProductKernel(scale, [mirror(fx['fidel_scale'], parts[0]), mirror(fx['domain_scale'], parts[1])]).to_spec())
    Xd = engine.to_device(d['packed'])
    batch = lambda: engine.gp_lml_batch(specs, Xd, d['Y'], [d['mean']] * BATCH, [d['noise']] * BATCH, handle_non_psd_kernels='project_first')
    rows.append(dict(row='tuning batch, %d candidates' % BATCH, n=n, route='one dfh_gp_lml_batch call with the projection flag',
                     **repeat(batch, engine.sync)))
    print(json.dumps(rows[-1]), flush=True)
  merge(path, 'device', dict(machine=platform.machine(), cpus=os.cpu_count(), gpu=engine.name()), rows)


def main():
  phase = sys.argv[1] if len(sys.argv) > 1 else ''
  path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'cpmf_boca_timing.json')
  if phase == 'host':
    if len(sys.argv) > 3:
      os.environ['DRAGONFLY_REFERENCE'] = sys.argv[3]
    host_phase(path)
  elif phase == 'device':
    device_phase(path)
  else:
    sys.exit(__doc__)


if __name__ == '__main__':
  main()
