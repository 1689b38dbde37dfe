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
generated in HBM.  UCB under a tree search evaluates a frontier of boxes per call.

On a Cartesian-product domain the reference calls these closures one point at a time.  Where mo_cp_acquisition_applies
holds -- K device CP GPs on the kernel's descriptor, install(multi_objective=True, cartesian_product=True,
cp_acquisitions=True) -- a Thompson step is the reference's own samples, packed in one pass, in ONE
mo_thompson_pointwise call (dfh_mo_ts_pointwise: a one-point draw per candidate and objective, the m K normals
POINT-major, the order in which the reference's loop over points, with its loop over objectives inside, draws them), and a
UCB step ONE mo_ucb_argmax on the packed samples, a frontier of the tree search per call, or one call per point of
Dragonfly's own maximiser.  GPs without a device kernel, other domains and multi-fidelity runs take the reference's closure
route.
"""
from argparse import Namespace
from copy import copy

import numpy as np

from . import gpb_acquisitions as _single
from ._lib import MO_MAX_OBJECTIVES
from .gpb_acquisitions import get_gp_sampler_for_parallel_strategy
from .gpb_acquisitions import _draw_candidates, _host_rows, _mean_constant, _standard_normals      # pylint: disable=protected-access
from .gpb_acquisitions import _cp_maximiser, _in_progress, _is_cp_device_step, _normals_in_hbm       # pylint: disable=protected-access
from .gpb_acquisitions import maximise_acquisition as _maximise_acquisition
from .kernel import _as_2d_array


def maximise_acquisition(acq_fn, anc_data, *args, **kwargs):
  """ gpb_acquisitions.maximise_acquisition for the closures of this module: over rows of Euclidean points, or over lists
      of the points of a Cartesian-product domain. """
  if anc_data.domain.get_type() not in ('euclidean', 'cartesian_product'):
    raise NotImplementedError('dragonfly_amd multi-objective acquisitions handle Euclidean and Cartesian-product domains.')
  return _maximise_acquisition(acq_fn, anc_data, *args, **kwargs)


def _get_ucb_beta_th(dim, time_step):
  """ multiobjective_gpb_acquisitions.py:71-73 """
  return np.sqrt(0.2 * dim * np.log(2 * dim * time_step + 1))


def _domain_dim(domain):
  dim = getattr(domain, 'dim', None)
  return domain.get_dim() if dim is None else dim


def _device_gps(gps, anc_data):
  """ The objectives' FittedGPs when all of them can go into one device call, else None: no fidelities, all on one
      engine, and every GP a fitted mirror GP with a device kernel on a Euclidean domain, or -- a Cartesian-product
      domain -- the device CP GP on the descriptor route with a kernel guaranteed PSD (_is_cp_device_step), all of one
      packed width. """
  gps = list(gps)
  if not 1 <= len(gps) <= MO_MAX_OBJECTIVES or getattr(anc_data, 'is_mf', False):
    return None
  domain_type = anc_data.domain.get_type()
  if domain_type == 'euclidean':
    usable = all(_single._is_device_gp(gp) for gp in gps)     # pylint: disable=protected-access
  elif domain_type == 'cartesian_product':
    usable = all(_is_cp_device_step(gp, anc_data) for gp in gps) and \
             len(set(gp.kernel.part_offsets()[1] for gp in gps)) == 1
  else:
    usable = False
  if not usable:
    return None
  fitted = [gp.device_gp for gp in gps]
  if any(f.engine is not fitted[0].engine for f in fitted):
    return None
  return fitted


def mo_cp_acquisition_applies(acq, gps, anc_data):
  """ Whether acquisition `acq` ('lin_ts' | 'tch_ts' | 'lin_ucb' | 'tch_ucb') of this module serves a step on a
      Cartesian-product domain: _device_gps holds there, and -- decided before any random number is drawn -- the engine
      draws point-wise (Thompson sampling, which always takes 'rand'), or the UCB's maximiser is one of _cp_maximiser's
      two or Dragonfly's own, reachable when installed under it.  install(multi_objective=True, cartesian_product=True,
      cp_acquisitions=True) asks before it calls ours. """
  if acq not in ('lin_ts', 'tch_ts', 'lin_ucb', 'tch_ucb') or anc_data.domain.get_type() != 'cartesian_product':
    return False
  fitted = _device_gps(gps, anc_data)
  if fitted is None:
    return False
  if acq.endswith('_ts'):
    return hasattr(fitted[0].engine, 'mo_thompson_pointwise')
  return _cp_maximiser(anc_data) is not None or _single.external_maximise_with_method is not None


def _is_cp(anc_data):
  return anc_data.domain.get_type() == 'cartesian_product'


def _closure_route(gps, anc_data):
  """ Checks that the closures of this module can serve the step.  On a Euclidean domain they serve anything with eval /
      draw_samples.  On a Cartesian-product domain they are called on lists of points, one point per call, which is what
      device CP GPs take (K above the limit, several engines or differing category codes only cost the fused call); any
      other GP there, and a multi-fidelity run, is the reference's business (install dispatches them). """
  if _is_cp(anc_data) and not all(_is_cp_device_step(gp, anc_data) for gp in gps):
    raise NotImplementedError('dragonfly_amd multi-objective acquisitions handle Cartesian-product domains for device CP GPs.')


def _pack_shared(gps, points):
  """ The points of a Cartesian-product domain packed by every objective's own kernel (each owns its category codes):
      the one matrix, if the K matrices are equal -- as they are when the GPs were built from the same training list --
      else None, and the caller takes the per-point closure route: no objective is handed rows coded by another's
      dictionary. """
  packed = [gp.kernel.pack_many(points) for gp in gps]
  return packed[0] if all(np.array_equal(packed[0], other) for other in packed[1:]) else None


def _cp_prior_means(gps, points):
  """ _prior_means on a Cartesian-product domain: mean functions that are not constant are evaluated on the point lists,
      not on packed rows. """
  consts = [_mean_constant(gp.mean_func) for gp in gps]
  if None not in consts:
    return dict(mean_consts=consts)
  return dict(mean_vals=np.array([np.asarray(gp.mean_func(points), dtype=np.float64).ravel() for gp in gps]))


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
  if fitted is not None and _is_cp(anc_data) and not hasattr(fitted[0].engine, 'mo_thompson_pointwise'):
    fitted = None
  if fitted is None:
    _closure_route(gps, anc_data)
    return maximise_acquisition(_host_ts_acquisition(scal, gps, anc_data), anc_data, vectorised=True)
  engine = fitted[0].engine
  if _is_cp(anc_data):
    return _cp_mo_ts(scal, gps, fitted, anc_data)
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


def _cp_mo_ts(scal, gps, fitted, anc_data):
  """ The Thompson step on a Cartesian-product domain: the reference's samples (its consumption of np.random, its
      constraint handling, its count), then per sample and objective a one-point draw -- the normals in the order of the
      reference's loops, point by point and inside that objective by objective, generated in HBM when handed None -- in
      ONE mo_thompson_pointwise; the point returned is the winning sample object itself. """
  cands = _single._cp_candidates(anc_data)       # pylint: disable=protected-access
  pts = _in_progress(anc_data)
  rows = _pack_shared(gps, cands)
  rows_in_progress = None if pts is None or rows is None else _pack_shared(gps, pts)
  if rows is None or (pts is not None and rows_in_progress is None):
    # (the samples are drawn: the reference's loop over them, one closure call per point)
    acquisition = _host_ts_acquisition(scal, gps, anc_data)
    return cands[int(np.argmax([acquisition([x]) for x in cands]))]
  m, k = len(cands), len(fitted)
  normals = None if _normals_in_hbm(fitted[0]) else \
            np.array([np.random.normal(size=(1, 1))[0, 0] for _ in range(m * k)])
  _, idx = fitted[0].engine.mo_thompson_pointwise(fitted, *_scal_args(scal, anc_data), Xs=rows, normals=normals,
                                                  X_halluc=rows_in_progress, **_cp_prior_means(gps, cands))
  return cands[idx]


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
    _closure_route(gps, anc_data)
    return maximise_acquisition(_host_ucb_acquisition(scal, gps, anc_data, beta_th), anc_data)
  engine = fitted[0].engine
  scal_args = _scal_args(scal, anc_data)
  if _is_cp(anc_data):
    return _cp_mo_ucb(scal, gps, fitted, anc_data, beta_th)
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


def _cp_mo_ucb(scal, gps, fitted, anc_data, beta_th):
  """ The UCB step on a Cartesian-product domain.  The acquisition takes a list of points, packs it with every
      objective's kernel and makes one mo_ucb_argmax (no points in progress: the reference's closures call gp.eval); lists
      whose packed forms differ between the objectives go to the reference's closure.  'rand': the reference's samples in
      one call; the tree search: a frontier per call; any other maximiser is Dragonfly's own, one call per point. """
  engine = fitted[0].engine
  scal_args = _scal_args(scal, anc_data)
  host_acquisition = _host_ucb_acquisition(scal, gps, anc_data, beta_th)
  def acquisition(points):
    rows = _pack_shared(gps, points)
    if rows is None:
      return np.concatenate([np.ravel(host_acquisition([x])) for x in points])
    return engine.mo_ucb_argmax(fitted, scal_args[0], beta_th, scal_args[1], scal_args[2], rows, return_vals=True,
                                **_cp_prior_means(gps, points))[2]
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
