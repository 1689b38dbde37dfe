"""Multi-objective acquisitions on the MI355X -- host-side mirror of
dragonfly/opt/multiobjective_gpb_acquisitions.py (Thompson sampling :19-67, UCB :76-106; namespaces
asy / syn / seq :109-125).

Same callables, same `anc_data` fields (opt/multiobjective_gp_bandit.py): `asy.<scal>_<acq>(gps, anc_data)
-> point` with one GP per objective, `anc_data.obj_weights` and, for the Tchebychev scalarisation,
`anc_data.reference_point`.

With K device GPs on a Euclidean domain the K posteriors (or K joint draws), the scalarisation and the
arg-max are ONE device call (dfh_mo_ucb_argmax / dfh_mo_ts_argmax): the reference's closures call gp.eval
or gp.draw_samples once per objective and scalarise K vectors of m values in NumPy.  With 'rand' the
candidates, and for Thompson sampling the K m normals, continue the global np.random state exactly as
the reference consumes it -- candidates first, then objective 0's normals, objective 1's, ... -- and are
generated in HBM.  UCB under a tree search evaluates a frontier of boxes per call.  GPs without a device
kernel, other domains and multi-fidelity runs take the reference's closure route.
"""
from argparse import Namespace
from copy import copy

import numpy as np

from . import gpb_acquisitions as _single
from ._lib import MO_MAX_OBJECTIVES
from .gpb_acquisitions import get_gp_sampler_for_parallel_strategy
from .gpb_acquisitions import _draw_candidates, _host_rows, _mean_constant, _standard_normals      # pylint: disable=protected-access
from .gpb_acquisitions import maximise_acquisition as _maximise_acquisition
from .kernel import _as_2d_array


def maximise_acquisition(acq_fn, anc_data, *args, **kwargs):
  """ gpb_acquisitions.maximise_acquisition for the closures of this module, which take rows of Euclidean points: the
      multi-objective acquisitions of a Cartesian-product domain stay with the reference (install dispatches them). """
  if anc_data.domain.get_type() != 'euclidean':
    raise NotImplementedError('dragonfly_amd multi-objective acquisitions handle Euclidean domains.')
  return _maximise_acquisition(acq_fn, anc_data, *args, **kwargs)


def _get_ucb_beta_th(dim, time_step):
  """ multiobjective_gpb_acquisitions.py:71-73 """
  return np.sqrt(0.2 * dim * np.log(2 * dim * time_step + 1))


def _domain_dim(domain):
  dim = getattr(domain, 'dim', None)
  return domain.get_dim() if dim is None else dim


def _device_gps(gps, anc_data):
  """ The objectives' FittedGPs when all of them can go into one device call, else None: every GP a
      fitted mirror GP with a device kernel, on one engine, a Euclidean domain, no fidelities. """
  gps = list(gps)
  if not 1 <= len(gps) <= MO_MAX_OBJECTIVES or getattr(anc_data, 'is_mf', False) or \
     anc_data.domain.get_type() != 'euclidean' or not all(_single._is_device_gp(gp) for gp in gps):     # pylint: disable=protected-access
    return None
  fitted = [gp.device_gp for gp in gps]
  if any(f.engine is not fitted[0].engine for f in fitted):
    return None
  return fitted


def _prior_means(gps, cands):
  """ What the device call adds to K(x, X) alpha per objective, by the single-objective rule: the fitters' constant
      means, or the mean functions' values on the candidates (a host copy of them when they were generated in HBM). """
  consts = [_mean_constant(gp.mean_func) for gp in gps]
  if None not in consts:
    return dict(mean_consts=consts)
  host = _host_rows(cands)
  return dict(mean_vals=np.array([np.asarray(gp.mean_func(host), dtype=np.float64).ravel() for gp in gps]))


def _scal_args(scal, anc_data):
  return scal, anc_data.obj_weights, (anc_data.reference_point if scal == 'tch' else None)


# Thompson sampling ------------------------------------------------------------------------------
def _host_ts_acquisition(scal, gps, anc_data):
  """ The reference's closures (:32-39, :57-65) over the per-objective samplers. """
  gp_samples = [get_gp_sampler_for_parallel_strategy(gp, anc_data) for gp in gps]
  if scal == 'lin':
    def acquisition(x):
      s = 0.0
      for gp_sample, weight in zip(gp_samples, anc_data.obj_weights):
        s += gp_sample(x) * weight
      return s
  else:
    def acquisition(x):
      s = np.full((len(x), ), np.inf)
      for gp_sample, weight, ref in zip(gp_samples, anc_data.obj_weights, anc_data.reference_point):
        s = np.minimum(s, (gp_sample(x) - ref) / weight)
      return s
  return acquisition


def _mo_ts(scal, gps, anc_data):
  """ :19-67.  TS always works on random candidates with one vectorised joint sample per objective; a
      different configured method only multiplies the number of candidates by four. """
  anc_data = copy(anc_data)
  if anc_data.acq_opt_method != 'rand':
    anc_data.acq_opt_method = 'rand'
    anc_data.max_evals = 4 * anc_data.max_evals
  fitted = _device_gps(gps, anc_data)
  if fitted is None:
    return maximise_acquisition(_host_ts_acquisition(scal, gps, anc_data), anc_data, vectorised=True)
  engine = fitted[0].engine
  Xh = _single._halluc_points(anc_data)       # pylint: disable=protected-access
  cands, row = _draw_candidates(fitted[0], anc_data)
  m, k = cands.shape[0], len(fitted)
  # once per objective in the order the reference's loop asks: one stream of k m normals
  normals = _standard_normals(fitted[0], m, draws=k)
  _, idx = engine.mo_thompson(fitted, *_scal_args(scal, anc_data), Xs=cands, U=normals, block=m, X_halluc=Xh,
                              **_prior_means(gps, cands))
  if hasattr(normals, 'free'):
    normals.free()
  return row(idx)


def mo_lin_asy_ts(gps, anc_data):
  """ TS with linear scalarisation, asynchronous setting (:19-41) """
  return _mo_ts('lin', gps, anc_data)


def mo_tch_asy_ts(gps, anc_data):
  """ TS with Tchebychev scalarisation, asynchronous setting (:44-67) """
  return _mo_ts('tch', gps, anc_data)


# UCB ----------------------------------------------------------------------------------------------
def _host_ucb_acquisition(scal, gps, anc_data, beta_th):
  """ The reference's closures (:80-89, :97-105) over gp.eval. """
  if scal == 'lin':
    def acquisition(x):
      mu_tot = 0.0
      sigma2_tot = 0.0
      for gp, weight in zip(gps, anc_data.obj_weights):
        mu, sigma = gp.eval(x, uncert_form='std')
        mu_tot += mu * weight
        sigma2_tot += sigma * sigma * weight**2
      return mu_tot + beta_th * np.sqrt(sigma2_tot)
  else:
    def acquisition(x):
      ret = np.asarray([np.inf for _ in range(len(x))])
      for gp, weight, ref in zip(gps, anc_data.obj_weights, anc_data.reference_point):
        mu, sigma2 = gp.eval(x, uncert_form='std')
        ucb = mu + beta_th * np.sqrt(sigma2) - ref      # the square root of 'std', as the reference has it
        ret = np.minimum(ret, ucb / weight)
      return ret
  return acquisition


def _mo_ucb(scal, gps, anc_data):
  """ :76-106 """
  beta_th = _get_ucb_beta_th(_domain_dim(anc_data.domain), anc_data.t)
  fitted = _device_gps(gps, anc_data)
  if fitted is None:
    return maximise_acquisition(_host_ucb_acquisition(scal, gps, anc_data, beta_th), anc_data)
  engine = fitted[0].engine
  scal_args = _scal_args(scal, anc_data)
  if str(anc_data.acq_opt_method).lower().startswith('rand'):
    cands, row = _draw_candidates(fitted[0], anc_data)
    _, idx = engine.mo_ucb_argmax(fitted, scal_args[0], beta_th, scal_args[1], scal_args[2], cands,
                                  **_prior_means(gps, cands))
    return row(idx)
  # a tree search (or Dragonfly's own maximiser): the rows it asks for -- a frontier of boxes per call under
  # pdoo_maximise_batched -- cost one device call instead of one gp.eval per objective
  def acquisition(x):
    x = _as_2d_array(x)
    return engine.mo_ucb_argmax(fitted, scal_args[0], beta_th, scal_args[1], scal_args[2], x, return_vals=True,
                                **_prior_means(gps, x))[2]
  return maximise_acquisition(acquisition, anc_data)


def mo_lin_asy_ucb(gps, anc_data):
  """ UCB with linear scalarisation, asynchronous setting (:76-90) """
  return _mo_ucb('lin', gps, anc_data)


def mo_tch_asy_ucb(gps, anc_data):
  """ UCB with Tchebychev scalarisation, asynchronous setting (:93-106) """
  return _mo_ucb('tch', gps, anc_data)


asy = Namespace(lin_ts=mo_lin_asy_ts, tch_ts=mo_tch_asy_ts, lin_ucb=mo_lin_asy_ucb, tch_ucb=mo_tch_asy_ucb)
# (the reference has no synchronous versions: its namespace is empty, :116-118)
syn = Namespace()
seq = Namespace(lin_ts=mo_lin_asy_ts, tch_ts=mo_tch_asy_ts, lin_ucb=mo_lin_asy_ucb, tch_ucb=mo_tch_asy_ucb)
