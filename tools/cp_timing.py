"""Times Cartesian-product kernels on the device and writes profiles/cp_timing.json:
 - the Gram matrix of SE(d=6) x Hamming(5) at n = 4096 and n = 16384 next to the SE(d=6) Gram matrix of the same n,
   each as a fraction of the HBM bound of 8 n^2 bytes written, and the same pair through the
   fit path (DFH_T_KERNMAT of dfh_gp_fit);
 - tuning: dfh_gp_lml_batch of 64 CP candidates at n = 1000 with project_first, the same 64 without the flag, and the
   same 64 by the host-kernel route -- kernel matrices composed in NumPy here, dfh_gp_fit_gram with the flag per
   candidate; the projection alone (dfh_project_psd at n = 1000).

    python tools/cp_timing.py [--reps R] [--host-route-only] [--out FILE]

--host-route-only measures only the host-kernel route (it needs nothing of the Hamming kind, so it also runs on a
build without it).  Device times: the library's HIP-event timer, after a warm-up, median of R (default 7); the
tuning routes include their host work and are wall-clock medians."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E


def _median_device(eng, fn, reps):
  fn()
  eng.sync()
  ms = []
  for _ in range(reps):
    eng.timer_begin()
    fn()
    ms.append(eng.timer_end())
  return float(np.median(ms))


def _median_wall(eng, fn, reps):
  fn()
  eng.sync()
  ms = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    eng.sync()
    ms.append((time.perf_counter() - t0) * 1e3)
  return float(np.median(ms))


def _candidates(rs, nb):
  """ (scale, 6 bandwidths, 5 weights, noise) of nb candidates """
  out = []
  for _ in range(nb):
    w = rs.uniform(0.1, 1.0, 5)
    out.append((float(np.exp(rs.uniform(-1, 1))), np.exp(rs.uniform(np.log(0.3), np.log(2.0), 6)), w / w.sum(),
                float(np.exp(rs.uniform(-6, -3)))))
  return out


def _host_gram(P, cand):
  """ scale * SE(d=6) * Hamming(5) in NumPy, as the reference composes it (a row of the smaller operand at a time) """
  scale, bws, w, _ = cand
  A = P[:, :6] / bws
  sq = (A ** 2).sum(axis=1)
  K = scale * np.exp(-np.clip(sq[:, None] + sq[None, :] - 2 * A.dot(A.T), 0, np.inf) / 2)
  ham = np.zeros((len(P), len(P)))
  C = P[:, 6:]
  for j in range(len(P)):
    ham[:, j] = (np.equal(C, C[j]) * w).sum(axis=1)
  return K * ham


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--host-route-only', action='store_true')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cp_timing.json'))
  args = ap.parse_args()
  from dragonfly_amd.engine import get_engine, KernelSpec
  eng = get_engine()
  rs = np.random.RandomState(0)
  out = {'reps': args.reps, 'hbm_peak_GBs': HBM_PEAK_GBS}
  n = 1000
  P = np.hstack([rs.rand(n, 6), rs.randint(0, 4, (n, 5)).astype(float)])
  Y = np.sin(3 * P[:, :6].sum(axis=1)) + 0.2 * (P[:, 6] == 0)
  cands = _candidates(rs, 64)
  yc = Y - Y.mean()

  def host_route():
    return [eng.gp_fit_gram(_host_gram(P, c), yc, c[3], handle_non_psd_kernels='project_first').lml for c in cands]
  t_host = _median_wall(eng, host_route, max(3, args.reps // 2))
  t_compose = _median_wall(eng, lambda: [_host_gram(P, c) for c in cands], 3)
  out['tuning_n1000_64'] = {'host_kernel_route_ms': t_host, 'of_which_numpy_composition_ms': t_compose}
  if not args.host_route_only:
    def cp_spec(c):
      return KernelSpec('product', 11, c[0], groups=[list(range(6)), list(range(6, 11))], sub_kinds=['se', 'hamming'],
                        sub_scales=[1.0, 1.0], sub_nus=[0.0, 0.0], sub_bandwidths=[c[1], c[2]])
    specs = [cp_spec(c) for c in cands]
    means, noises = [float(Y.mean())] * 64, [c[3] for c in cands]
    Pd = eng.to_device(P)
    lml_flag = eng.gp_lml_batch(specs, Pd, Y, means, noises, handle_non_psd_kernels='project_first')
    t = out['tuning_n1000_64']
    t['lml_rel_descriptor_vs_host_route'] = float(np.max(np.abs(lml_flag - np.array(host_route())) / np.abs(lml_flag)))
    t['lml_batch_project_first_ms'] = _median_wall(
        eng, lambda: eng.gp_lml_batch(specs, Pd, Y, means, noises, handle_non_psd_kernels='project_first'), args.reps)
    t['lml_batch_no_flag_ms'] = _median_wall(eng, lambda: eng.gp_lml_batch(specs, Pd, Y, means, noises), args.reps)
    t['host_route_over_descriptor_route'] = t_host / t['lml_batch_project_first_ms']
    Kh = _host_gram(P, cands[0])
    t['projection_alone_ms_per_matrix'] = _median_wall(eng, lambda: eng.project_psd(Kh), args.reps)
    out['gram'] = []
    for n in (4096, 16384):
      X = eng.to_device(np.hstack([rs.rand(n, 6), rs.randint(0, 4, (n, 5)).astype(float)]))
      X6 = eng.to_device(rs.rand(n, 6))
      K = eng.empty((n, n))
      bws, w = np.exp(rs.uniform(np.log(0.3), np.log(2.0), 6)), np.array([0.3, 0.2, 0.2, 0.2, 0.1])
      cp = KernelSpec('product', 11, 1.0, groups=[list(range(6)), list(range(6, 11))], sub_kinds=['se', 'hamming'],
                      sub_scales=[1.0, 1.0], sub_nus=[0.0, 0.0], sub_bandwidths=[bws, w])
      se = KernelSpec('se', 6, 1.0, bws)
      ms_cp = _median_device(eng, lambda: eng.kernel_matrix(cp, X, None, out=K), args.reps)
      ms_se = _median_device(eng, lambda: eng.kernel_matrix(se, X6, None, out=K), args.reps)
      bound_ms = 8.0 * n * n / (HBM_PEAK_GBS * 1e9) * 1e3
      out['gram'].append(dict(n=n, se6_x_hamming5_ms=ms_cp, se6_ms=ms_se, ratio=ms_cp / ms_se, hbm_bound_ms_8n2=bound_ms,
                              se6_x_hamming5_frac_of_hbm_bound=bound_ms / ms_cp, se6_frac_of_hbm_bound=bound_ms / ms_se))
      del K
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
  print(json.dumps(out))


if __name__ == '__main__':
  main()
