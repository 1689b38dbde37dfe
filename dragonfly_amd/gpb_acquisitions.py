"""Acquisition functions for Bayesian optimisation on the MI355X -- host-side mirror of
dragonfly/opt/gpb_acquisitions.py (UCB :215, PI :230, EI :251, TTEI :282, TS :119, add-UCB :139;
hallucination wrappers :43-87; synchronous batches :90-115; BOCA's view of a multi-fidelity GP, its add-UCB and
its decision step :313-439; namespaces asy / syn / seq :443-471).

Same callables, same `anc_data` fields (gp_bandit.py:462-484): `asy.<acq>(gp, anc_data) -> point`,
`syn.<acq>(num_workers, gps, anc_datas) -> [points]`.

With acq_opt_method == 'rand' on a Euclidean domain -- the batched path, oper_utils.py:59-80 --
the whole evaluation is ONE fused device call: candidates are drawn from the global np.random
state exactly as the reference draws them, then posterior mean / std, the acquisition formula
and the arg-max (first NaN, else first maximum) run in libdfhip.so and only the winning index
comes back.  Other acq_opt_method values are per-point serial tree searches in the reference
(DIRECT / PDOO, out of scope): they are served through Dragonfly's own maximisers when this
package is installed under Dragonfly (dragonfly_amd.install), each callback hitting GP.eval on
the device.

On a Cartesian-product domain the reference evaluates every acquisition one point per call.  Where
cp_acquisition_applies holds -- the device CP GP on the kernel's descriptor, install(cp_acquisitions=True) -- a 'rand'
step is the reference's own samples, packed in one pass, in ONE acq_argmax or (Thompson sampling: a one-point draw per
candidate, not a joint draw) ONE thompson_pointwise call, and the tree search of an all-Euclidean product fetches its
values a frontier per call.

All four -- a Euclidean GP, BOCA's view of a multi-fidelity GP (FidelToOptGP), the device GP of a product domain, BOCA's
view of the multi-fidelity GP of a product domain -- take
the same fused step: _fused_source decides, before any random number is drawn, which of _euclidean_step / _boca_step /
_cp_step / _cp_boca_step describes it (a _FusedStep: handle, rows, prior mean, rows in progress, index -> point), and _fused_argmax or
_fused_thompson makes the one device call.  Add-UCB is one function (_add_ucb) over the handle's per-group and all-groups
calls, BOCA's with the fidelity bound.  With DFH_GAP_LOG set every fused single-objective step records its margin.
"""
import os
from argparse import Namespace
from copy import copy
from functools import partial

import numpy as np

from . import gaplog
from .general_utils import map_to_bounds
from .kernel import AdditiveKernel, _as_2d_array
from .doo import pdoo_maximise_batched
from .oper_utils import random_maximise

# Candidates of the fused 'rand' path are generated in HBM (bit-identical to the host draw, same
# generator state afterwards); DFH_HOST_CANDIDATES=1 keeps the draw on the host.
DEVICE_CANDIDATES = os.environ.get('DFH_HOST_CANDIDATES', '0') != '1'

# Open leaves whose halves are prefetched with every cache miss of the batched PDOO (0: one point
# per device call, the reference's access pattern).
PDOO_FRONTIER = int(os.environ.get('DFH_PDOO_FRONTIER', '32'))

# A maximiser for non-'rand' methods; dragonfly_amd.install points this at
# dragonfly.exd.exd_utils.maximise_with_method.
external_maximise_with_method = None


def _candidates(anc_data, max_evals=None):
  """ random_sample's draw (oper_utils.py:61-62): map_to_bounds(np.random.random((m, d)), b). """
  bounds = np.asarray(anc_data.domain.bounds, dtype=np.float64)
  m = int(anc_data.max_evals if max_evals is None else max_evals)
  return map_to_bounds(np.random.random((m, len(bounds))), bounds)


def _draw_candidates(fitted, anc_data):
  """ The candidates of a 'rand' step on a Euclidean domain, from the global np.random state: generated in HBM
      (Engine.random_candidates: the state is continued bit for bit and left where the host draw would have left it, so
      the candidates are the reference's -- without the host generation and the m x d copy), or _candidates on the host.
      Returns (candidates, index -> host point). """
  if DEVICE_CANDIDATES:
    bounds = np.asarray(anc_data.domain.bounds, dtype=np.float64)
    cands = fitted.engine.random_candidates(int(anc_data.max_evals), len(bounds), bounds=bounds)
    return cands, cands.row
  cands = _candidates(anc_data)
  return cands, cands.__getitem__


def _host_rows(cands):
  return cands if isinstance(cands, np.ndarray) else cands.download()


def _mean_constant(mean_func):
  """ The value of the fitter's constant mean (gp_core.ConstantMean), or None for any other mean function. """
  const = getattr(mean_func, 'constant_value', None)
  return None if const is None else float(const)


def _prior_mean(mean_func, points):
  """ What a fused call adds to K(x, X) alpha, as its keyword arguments: the constant of a constant mean, else the mean
      function's values on points() -- the host form of the candidates, fetched only when it is needed. """
  const = _mean_constant(mean_func)
  return dict(mean_vals=mean_func(points())) if const is None else dict(mean_const=const)


def _normals_in_hbm(fitted):
  return DEVICE_CANDIDATES and getattr(getattr(fitted, 'engine', None), 'random_normals', None) is not None


def _standard_normals(fitted, m, draws=1):
  """ np.random.normal(size=(m, 1)) of draw_gaussian_samples (general_utils.py:230), `draws` times in a row, as one
      stream -- generated in HBM where the candidates are (Engine.random_normals continues the global state bit for bit,
      the cached second gaussian included; free() the DeviceArray after the call), else drawn here. """
  if _normals_in_hbm(fitted):
    return fitted.engine.random_normals(draws * m)
  return np.concatenate([np.random.normal(size=(m, 1)).ravel() for _ in range(draws)])


def _is_rand_euclidean(anc_data):
  return anc_data.domain.get_type() == 'euclidean' and \
         str(anc_data.acq_opt_method).lower().startswith('rand')


def _is_device_gp(gp):
  """ A fitted mirror GP with a device kernel.  Anything else offering eval() -- e.g. the
      Namespace BOCA hands the acquisitions for the GP restricted to the target fidelity
      (gpb_acquisitions.py:384-395) -- is served through its eval. """
  from .gp_core import GP
  return isinstance(gp, GP) and gp.num_tr_data > 0 and not gp._generic    # pylint: disable=protected-access


class FidelToOptGP(object):
  """ The GP BOCA hands the acquisitions: the multi-fidelity GP seen at fidel_to_opt
      (_get_fidel_to_opt_gp, gpb_acquisitions.py:314-332) -- the reference Namespace's five attributes,
      plus the GP and the fidelity themselves, so that the acquisitions can take the fused route (_boca_step): the
      candidates drawn as ever, joined with the fidelity in HBM (Engine.join_fixed) and handed to the
      joint GP's fused calls with the joint (fidelity, point) pairs in progress. """

  def __init__(self, mfgp, fidel_to_opt):
    self.mfgp, self.fidel_to_opt = mfgp, fidel_to_opt
    self.kernel = mfgp.get_domain_kernel()

  def _joint(self, x):
    return self.mfgp.get_ZX_from_ZZ_XX([self.fidel_to_opt] * len(x), x)

  def eval(self, x, *args, **kwargs):
    return self.mfgp.eval_at_fidel([self.fidel_to_opt] * len(x), x, *args, **kwargs)

  def eval_with_hallucinated_observations(self, x, halluc_fidel_pts, *args, **kwargs):
    return self.mfgp.eval_with_hallucinated_observations(self._joint(x), halluc_fidel_pts, *args, **kwargs)

  def draw_samples(self, n, x, *args, **kwargs):
    return self.mfgp.draw_samples(n, self._joint(x), *args, **kwargs)

  def draw_samples_with_hallucinated_observations(self, n, x, halluc_fidel_pts, *args, **kwargs):
    return self.mfgp.draw_samples_with_hallucinated_observations(n, self._joint(x), halluc_fidel_pts, *args, **kwargs)

  def is_fusable(self):
    """ A Euclidean multi-fidelity mirror GP with a device kernel: its joint points are [z, x] rows.  Or the device
        CPMFGP of a Cartesian-product domain on the descriptor route with a kernel guaranteed PSD (on_product_domain):
        its joint points are (z, x) pairs, packed side by side. """
    from .mf_gp import EuclideanMFGP
    return (isinstance(self.mfgp, EuclideanMFGP) and _is_device_gp(self.mfgp)) or self.on_product_domain()

  def on_product_domain(self):
    return _is_cp_device_mfgp(self.mfgp)

def _fortran_direct_available():
  """ True when a Dragonfly with its compiled DIRECT is importable (oper_utils.py:21-25). """
  if external_maximise_with_method is None:      # not installed under a Dragonfly
    return False
  try:
    from dragonfly.utils import oper_utils as ref_oper_utils
    return ref_oper_utils.direct_ft_wrap is not None
  except Exception:     # pylint: disable=broad-except
    return False


def maximise_acquisition(acq_fn, anc_data, *args, **kwargs):
  """ gpb_acquisitions.py:23-40 for acquisition callables over rows of points ([m x d] -> [m]).
      'rand': one vectorised call on the random candidates.  'pdoo', and 'direct' where the
      reference itself falls back to PDOO because its Fortran DIRECT is not built
      (oper_utils.py:130-133): the tree search of dragonfly_amd.doo, which visits the boxes the
      reference visits but fetches the values a frontier per device call.  Anything else goes to
      Dragonfly's own maximiser when installed under it. """
  acq_opt_method = str(anc_data.acq_opt_method).lower()
  if anc_data.domain.get_type() == 'cartesian_product':
    return _maximise_acquisition_on_cp_domain(acq_fn, anc_data, *args, **kwargs)
  if anc_data.domain.get_type() != 'euclidean':
    raise NotImplementedError('dragonfly_amd acquisitions handle Euclidean and Cartesian-product domains.')
  if acq_opt_method.startswith('rand'):
    kwargs.pop('vectorised', None)
    _, opt_pt, _ = random_maximise(acq_fn, anc_data.domain.bounds, anc_data.max_evals)
    return opt_pt
  if acq_opt_method.startswith('pdoo') or \
     (acq_opt_method.startswith('direct') and not _fortran_direct_available()):
    frontier = int(getattr(anc_data, 'pdoo_frontier', PDOO_FRONTIER))
    _, opt_pt, _ = pdoo_maximise_batched(acq_fn, anc_data.domain.bounds, anc_data.max_evals,
                                         frontier=frontier, depth=2 if frontier > 0 else 0)
    return opt_pt
  if external_maximise_with_method is None:
    raise NotImplementedError(
        'acq_opt_method=%s is served by Dragonfly\'s own maximiser; install under Dragonfly '
        '(dragonfly_amd.install) to use it.' % (anc_data.acq_opt_method))
  acquisition = lambda x: acq_fn(x.reshape((1, -1)))
  _, opt_pt = external_maximise_with_method(anc_data.acq_opt_method, acquisition, anc_data.domain,
                                            anc_data.max_evals, *args, **kwargs)
  return opt_pt


# Cartesian-product domains ------------------------------------------------------------------------
def _cp_maximiser(anc_data):
  """ How an acquisition is maximised on a Cartesian-product domain, by the reference's own tests of the method's name
      (exd_utils.py:277-339): 'rand' -- its loop over random samples, here one vectorised call -- 'tree' -- PDOO, and
      DIRECT where the Fortran library is not built, over the flattened bounds of a domain whose parts are all
      Euclidean and that has no constraints (exd_utils.py:219-244), here a frontier per call -- or None: the GA, a
      compiled DIRECT and everything else stay with the reference's maximiser. """
  method = str(anc_data.acq_opt_method).lower()
  if method == 'rand':
    return 'rand'
  if method.startswith('pdoo') or (method.startswith('direct') and not _fortran_direct_available()):
    domain = anc_data.domain
    if all(dom.get_type() == 'euclidean' for dom in domain.list_of_domains) and \
       not getattr(domain, 'has_constraints', lambda: False)():
      return 'tree'
  return None


def _cp_candidates(anc_data):
  """ The random samples of _rand_maximise_vectorised_objective_in_cp_domain (exd_utils.py:252-263), by the
      reference's own sampler and loop: its consumption of the global np.random state, its handling of constraints,
      and its sample count, which may exceed max_evals. """
  from dragonfly.exd.exd_utils import sample_from_cp_domain
  domain, max_evals = anc_data.domain, anc_data.max_evals
  rand_samples = []
  num_sample_tries = 0
  while not (len(rand_samples) >= max_evals or (len(rand_samples) > 0 and num_sample_tries >= 5)):
    rand_samples.extend(sample_from_cp_domain(domain, int(max_evals), verbose_constraint_satisfaction=False))
    num_sample_tries += 1
    if len(rand_samples) == 0 and num_sample_tries % 10 == 0:
      from warnings import warn
      warn(('Sampling from domain failed despite %d attempts -- will continue trying but consider '
            'reparametrising your domain if this problem persists.') % (num_sample_tries))
  return rand_samples


def _cp_flat_bounds(domain):
  """ The flattened box of a product of Euclidean domains and the map from its rows back to points (lists of
      per-part slices), exd_utils.py:223-232. """
  dims = [dom.dim for dom in domain.list_of_domains]
  starts = [0] + list(np.cumsum(dims))[:-1]
  bounds = np.array([row for dom in domain.list_of_domains for row in dom.bounds], dtype=np.float64)
  return bounds, lambda pt: [pt[cd:cd + d] for (cd, d) in zip(starts, dims)]


def _maximise_acquisition_on_cp_domain(acq_fn, anc_data, *args, **kwargs):
  """ maximise_acquisition for an acquisition over lists of Cartesian-product points ([m points] -> [m]): the random
      samples in one call, the tree search a frontier per call; what the reference evaluates one point per callback
      (gpb_acquisitions.py:35-37, exd_utils.py:265).  vectorised=True marks a sampler (asy_ts): a call of it on many
      points is a joint draw, which the reference never makes on these domains, so it keeps one call per point.
      Other maximisers are Dragonfly's own, point by point. """
  route = _cp_maximiser(anc_data)
  per_point = kwargs.pop('vectorised', False)
  if route == 'rand':
    cands = _cp_candidates(anc_data)
    vals = [acq_fn([x]) for x in cands] if per_point else acq_fn(cands)
    return cands[int(np.argmax(vals))]
  if route == 'tree':
    bounds, regroup = _cp_flat_bounds(anc_data.domain)
    frontier = int(getattr(anc_data, 'pdoo_frontier', PDOO_FRONTIER))
    _, opt_pt, _ = pdoo_maximise_batched(lambda rows: acq_fn([regroup(row) for row in rows]), bounds, anc_data.max_evals,
                                         frontier=frontier, depth=2 if frontier > 0 else 0)
    return regroup(opt_pt)
  if external_maximise_with_method is None:
    raise NotImplementedError(
        'acq_opt_method=%s on a Cartesian-product domain is served by Dragonfly\'s own maximiser; install under '
        'Dragonfly (dragonfly_amd.install) to use it.' % (anc_data.acq_opt_method))
  _, opt_pt = external_maximise_with_method(anc_data.acq_opt_method, lambda x: acq_fn([x]), anc_data.domain,
                                            anc_data.max_evals, *args, **kwargs)
  return opt_pt


def _is_cp_device_step(gp, anc_data):
  """ A step on a Cartesian-product domain whose GP is the device GP running from the kernel's descriptor, with a
      kernel guaranteed positive semi-definite (so the reference does not project the per-point covariances,
      gp_core.py:849-857), in a run that is not multi-fidelity. """
  return anc_data.domain.get_type() == 'cartesian_product' and not getattr(anc_data, 'is_mf', False) and \
         _is_device_gp(gp) and hasattr(gp.kernel, 'pack_many') and gp.kernel.is_guaranteed_psd()


def cp_acquisition_applies(acq, gp, anc_data):
  """ Whether acquisition `acq` ('ucb' | 'ei' | 'pi' | 'ttei' | 'ts') of this module serves a step on a Cartesian-product
      domain: _is_cp_device_step, and the maximiser is one of _cp_maximiser's two (Thompson sampling always takes
      'rand', gpb_acquisitions.py:119-127).  install(cp_acquisitions=True) asks before it calls ours. """
  if acq not in ('ucb', 'ei', 'pi', 'ttei', 'ts') or not _is_cp_device_step(gp, anc_data):
    return False
  return acq == 'ts' or _cp_maximiser(anc_data) is not None


def _is_cp_device_mfgp(mfgp):
  """ The device CPMFGP (cartesian_product_gp.device_cpmfgp_class) running from the nested product descriptor, with a
      kernel guaranteed positive semi-definite -- as _is_cp_device_step asks of a CPGP. """
  from .cartesian_product_gp import is_device_cpmfgp
  return is_device_cpmfgp(mfgp) and _is_device_gp(mfgp) and hasattr(mfgp.kernel, 'pack_many') and \
         mfgp.kernel.is_guaranteed_psd()


def cp_boca_applies(mfgp, anc_data):
  """ Whether boca() of this module takes BOCA's decision step on a Cartesian-product domain: the device CPMFGP on the
      descriptor route with a kernel guaranteed PSD.  Add-UCB is Euclidean-only in the reference and stays with it.
      install(boca=True, cp_acquisitions=True, cp_multi_fidelity=True) asks before it calls ours. """
  return anc_data.domain.get_type() == 'cartesian_product' and getattr(anc_data, 'curr_acq', None) != 'add_ucb' and \
         _is_cp_device_mfgp(mfgp)


def cp_boca_view_applies(acq, gp, anc_data):
  """ Whether acquisition `acq` of this module serves BOCA's view of such a GP: the view boca() made (cp_boca_applies
      held), and a maximiser of _cp_maximiser's two -- the GA and a compiled DIRECT keep the reference's callable, which
      then evaluates point by point through the view. """
  if acq not in ('ucb', 'ei', 'pi', 'ttei', 'ts') or not isinstance(gp, FidelToOptGP) or not gp.on_product_domain():
    return False
  return anc_data.domain.get_type() == 'cartesian_product' and (acq == 'ts' or _cp_maximiser(anc_data) is not None)


class _BoxDomain(object):
  """ The Euclidean sub-domain of one additive group (EuclideanDomain(domain_bounds[group_j]),
      gpb_acquisitions.py:180). """

  def __init__(self, bounds):
    self.bounds = np.asarray(bounds, dtype=np.float64)

  def get_type(self):
    return 'euclidean'

  def get_dim(self):
    return len(self.bounds)


def _in_progress(anc_data):
  """ What the acquisitions hallucinate (gpb_acquisitions.py:56-64): the evaluations in progress
      when handle_parallel == 'halluc' -- (fidelity, point) pairs in multi-fidelity runs, where the
      GP handed in is BOCA's view at the target fidelity -- or None. """
  if getattr(anc_data, 'handle_parallel', None) != 'halluc' or \
     len(getattr(anc_data, 'eval_points_in_progress', [])) == 0:
    return None
  if getattr(anc_data, 'is_mf', False):
    return anc_data.eval_fidel_points_in_progress
  return anc_data.eval_points_in_progress


def _halluc_points(anc_data):
  """ The in-progress points as an array for the device calls (single-fidelity GPs only). """
  pts = _in_progress(anc_data)
  if pts is None or _points_stay_lists(anc_data):
    return None
  return _as_2d_array(pts)


def _points_stay_lists(anc_data):
  """ (fidelity, point) pairs and the points of a Cartesian-product domain are not rows of one matrix: the GP packs them """
  return getattr(anc_data, 'is_mf', False) or anc_data.domain.get_type() == 'cartesian_product'


def _get_gp_eval_for_parallel_strategy(gp, anc_data, uncert_form='std'):
  """ gpb_acquisitions.py:43-64 """
  pts = _in_progress(anc_data)
  if pts is not None:
    pts = pts if _points_stay_lists(anc_data) else _as_2d_array(pts)
    return lambda x: gp.eval_with_hallucinated_observations(x, pts, uncert_form=uncert_form)
  return lambda x: gp.eval(x, uncert_form=uncert_form)


def get_gp_sampler_for_parallel_strategy(gp, anc_data):
  """ gpb_acquisitions.py:67-87 """
  pts = _in_progress(anc_data)
  if pts is not None:
    pts = pts if _points_stay_lists(anc_data) else _as_2d_array(pts)
    return lambda x: gp.draw_samples_with_hallucinated_observations(1, x, pts).ravel()
  return lambda x: gp.draw_samples(1, x).ravel()


# The fused step ---------------------------------------------------------------------------------
class _FusedStep(object):
  """ One fused device call of a 'rand' step, described: the fitted handle; the candidates as rows the kernel reads; the
      prior-mean keyword arguments; the rows in progress, or None; index -> the point the step returns.  pointwise: Thompson
      sampling draws one point at a time, as the reference does on a Cartesian-product domain, not jointly. """

  def __init__(self, fitted, rows, mean, in_progress, point, pointwise=False):
    self.fitted, self.rows, self.mean, self.in_progress, self.point = fitted, rows, mean, in_progress, point
    self.pointwise = pointwise


def _euclidean_step(gp, anc_data):
  """ A Euclidean device GP: the rows are the candidates. """
  cands, point = _draw_candidates(gp.device_gp, anc_data)
  if isinstance(cands, np.ndarray):
    # host candidates have always gone with the mean function's values, constant or not
    mean = dict(mean_vals=gp.mean_func(cands))
  else:
    mean = _prior_mean(gp.mean_func, cands.download)
  return _FusedStep(gp.device_gp, cands, mean, _halluc_points(anc_data), point)


def _boca_step(view, anc_data):
  """ BOCA's view: the same candidates, joined in HBM with fidel_to_opt into rows of the joint GP; the prior mean is
      the joint GP's on the joint points, the points in progress are the joint pairs; the point is the un-joined
      candidate. """
  fitted = view.mfgp.device_gp
  cands, point = _draw_candidates(fitted, anc_data)
  joint = fitted.engine.join_fixed(view.fidel_to_opt, cands)
  mean = _prior_mean(view.mfgp.mean_func, lambda: view._joint(list(_host_rows(cands))))      # pylint: disable=protected-access
  pts = _in_progress(anc_data)
  return _FusedStep(fitted, joint, mean, None if pts is None else _as_2d_array(pts), point)


def _cp_step(gp, anc_data):
  """ The device GP of a Cartesian-product domain: the reference's samples, packed into the descriptor's dense layout in
      one pass, as are the points in progress; the point is the winning sample object itself. """
  cands = _cp_candidates(anc_data)
  pts = _in_progress(anc_data)
  return _FusedStep(gp.device_gp, gp.kernel.pack_many(cands), _prior_mean(gp.mean_func, lambda: cands),
                    None if pts is None else gp.kernel.pack_many(pts), cands.__getitem__, pointwise=True)


def _cp_boca_step(view, anc_data):
  """ BOCA's view of the device CPMFGP of a product domain: the reference's samples packed by the domain kernel in one
      pass and joined in HBM with the packed fidel_to_opt into rows of the joint descriptor; the prior mean is the joint
      GP's on the (fidelity, point) pairs, the pairs in progress are packed jointly; the point is the winning sample. """
  mfgp = view.mfgp
  fitted = mfgp.device_gp
  fidel_kernel, domain_kernel = mfgp.kernel.kernel_list
  cands = _cp_candidates(anc_data)
  joint = fitted.engine.join_fixed(fidel_kernel.pack([view.fidel_to_opt])[0], domain_kernel.pack_many(cands))
  mean = _prior_mean(mfgp.mean_func, lambda: view._joint(cands))      # pylint: disable=protected-access
  pts = _in_progress(anc_data)
  return _FusedStep(fitted, joint, mean, None if pts is None else mfgp.kernel.pack_many(pts), cands.__getitem__,
                    pointwise=True)


def _fused_source(gp, anc_data, thompson=False):
  """ Which of the four builds this step's _FusedStep, or None for the reference's closure route; decided before any
      random number is drawn.  The fused call needs a device kernel and the 'rand' maximiser.  In a multi-fidelity run
      only BOCA's own view of a device GP is fused -- though Thompson sampling (thompson=True) has never asked a plain
      Euclidean GP whether the run is multi-fidelity.  Thompson sampling also needs a handle that draws the way the step
      asks: with the points in progress in one call (FittedGP.fused_draws), or point-wise on a product domain. """
  if isinstance(gp, FidelToOptGP) and gp.on_product_domain():
    if not (anc_data.domain.get_type() == 'cartesian_product' and _cp_maximiser(anc_data) == 'rand'):
      return None
    return _cp_boca_step if not thompson or hasattr(gp.mfgp.device_gp, 'thompson_pointwise') else None
  if isinstance(gp, FidelToOptGP):
    if not (_is_rand_euclidean(anc_data) and gp.is_fusable()):
      return None
    source, fitted, waiting = _boca_step, gp.mfgp.device_gp, _in_progress(anc_data)
  elif _is_rand_euclidean(anc_data) and _is_device_gp(gp) and (thompson or not getattr(anc_data, 'is_mf', False)):
    source, fitted, waiting = _euclidean_step, gp.device_gp, _halluc_points(anc_data)
  elif _is_cp_device_step(gp, anc_data) and _cp_maximiser(anc_data) == 'rand':
    return _cp_step if not thompson or hasattr(gp.device_gp, 'thompson_pointwise') else None
  else:
    return None
  if thompson and waiting is not None and not getattr(fitted, 'fused_draws', False):
    return None
  return source


def _fused_argmax(step, acq, params):
  """ Posterior -> acquisition -> arg-max (first NaN, else first maximum) on the device; returns the point. """
  extra = dict(return_vals=True) if gaplog.ENABLED else {}
  out = step.fitted.acq_argmax(acq, step.rows, params=params, X_halluc=step.in_progress, **step.mean, **extra)
  if gaplog.ENABLED:
    gaplog.top2('acq_argmax', out[2])
  return step.point(out[1])


def _fused_thompson(step):
  """ Thompson sampling on the device.  Jointly: one draw over all m rows -- covariance, stable_cholesky, L u and the
      arg-max stay there, and with the normals generated in HBM nothing of size m crosses PCIe in either direction.
      Point-wise: per row a one-point posterior, its 1 x 1 stable_cholesky and one normal, the m normals in the order of m
      calls of np.random.normal(size=(1, 1)), in ONE thompson_pointwise -- which generates them itself when handed None. """
  m = step.rows.shape[0]
  extra = dict(return_samples=True) if gaplog.ENABLED else {}
  normals = None if step.pointwise and _normals_in_hbm(step.fitted) else _standard_normals(step.fitted, m)
  if step.pointwise:
    out = step.fitted.thompson_pointwise(step.rows, normals, X_halluc=step.in_progress, **step.mean, **extra)
  else:
    if step.in_progress is not None:      # (a handle without fused_draws takes no such argument)
      extra['X_halluc'] = step.in_progress
    out = step.fitted.thompson(step.rows, normals, block=m, **step.mean, **extra)
  if hasattr(normals, 'free'):
    normals.free()
  if gaplog.ENABLED:
    gaplog.top2('thompson', out[2])
  return step.point(out[1])


def _get_syn_recommendations_from_asy(asy_acq, num_workers, list_of_gps, anc_datas):
  """ A synchronous batch is the asynchronous rule applied num_workers times in a row, every
      earlier recommendation counting as an evaluation in progress for the later ones
      (gpb_acquisitions.py:90-115); a single gp / anc_data serves all workers, lists are used
      round-robin.  The objects are shallow-copied so that the caller's anc_data keeps its own
      eval_points_in_progress. """
  def _per_worker(obj):
    seq = list(obj) if hasattr(obj, '__iter__') else [obj]
    return [copy(seq[i % len(seq)]) for i in range(num_workers)]
  recommendations = []
  for worker, (worker_gp, worker_anc) in enumerate(zip(_per_worker(list_of_gps), _per_worker(anc_datas))):
    if worker > 0:
      worker_anc.eval_points_in_progress = recommendations
    recommendations.append(asy_acq(worker_gp, worker_anc))
  return recommendations


def _host_acquisition(gp, anc_data, formula):
  """ The reference's closure route: `formula(mu, sigma)` on the posterior of whatever points the
      maximiser asks for (hallucinated observations included), maximised by maximise_acquisition. """
  gp_eval = _get_gp_eval_for_parallel_strategy(gp, anc_data, 'std')
  return maximise_acquisition(lambda x: formula(*gp_eval(x)), anc_data)


def _acquire(gp, anc_data, acq, params, formula):
  """ One acquisition step: fused on the device when possible, the closure route otherwise. """
  source = _fused_source(gp, anc_data)
  if source is not None:
    return _fused_argmax(source(gp, anc_data), acq, params)
  return _host_acquisition(gp, anc_data, formula)


def _ndtr(x):
  from scipy.stats import norm as normal_distro
  return normal_distro.cdf(x)


def _expected_improvement_for_norm_diff(norm_diff):
  """ z Phi(z) + phi(z)  (gpb_acquisitions.py:247-249; host form, closure route only) """
  from scipy.stats import norm as normal_distro
  return norm_diff * normal_distro.cdf(norm_diff) + normal_distro.pdf(norm_diff)


# Thompson sampling ---------------------------------------------------------------------------
def asy_ts(gp, anc_data):
  """ gpb_acquisitions.py:119-127: TS always works on random candidates with one vectorised joint
      sample; a different configured method only multiplies the number of candidates by four. """
  anc_data = copy(anc_data)
  if anc_data.acq_opt_method != 'rand':
    anc_data.max_evals *= 4
    anc_data.acq_opt_method = 'rand'
  source = _fused_source(gp, anc_data, thompson=True)
  if source is None:
    return maximise_acquisition(get_gp_sampler_for_parallel_strategy(gp, anc_data), anc_data, vectorised=True)
  return _fused_thompson(source(gp, anc_data))


# Add-UCB -------------------------------------------------------------------------------------
def _get_add_ucb_beta_th(dim, time_step):
  """ gpb_acquisitions.py:135-137 """
  return np.sqrt(0.2 * dim * np.log(2 * dim * time_step + 1))


def _add_ucb(fitted, group_ucb, all_ucb, groupings, mean_funcs, anc_data):
  """ gpb_acquisitions.py:139-189, and :334-388 for BOCA: one UCB maximisation per additive group, each over its own
      candidate set (max_evals // number of groups points, drawn group by group from the global
      np.random state as the reference's loop draws them; the acquisition itself consumes no random
      numbers), the winners assembled coordinate-wise.  group_ucb and all_ucb are the fitted handle's calls for one group
      and for all of them (add_ucb_group / add_ucb_all; for a multi-fidelity GP with an additive domain model
      mf_add_ucb_group / mf_add_ucb_all with fidel_to_opt bound).  With 'rand' all groups go to the device in
      ONE call: the per-group posteriors share the factor L and alpha in HBM and one triangular
      solve.  Other maximisers, and per-group mean functions, take the reference's loop. """
  all_bounds = np.asarray(anc_data.domain_bounds, dtype=np.float64)
  per_group_evals = int(anc_data.max_evals // len(groupings))
  betas = [_get_add_ucb_beta_th(len(grp), anc_data.t) for grp in groupings]
  point = np.zeros((sum(len(grp) for grp in groupings),))
  if mean_funcs is not None or not _is_rand_euclidean(anc_data):
    # the reference's loop shape (gpb_acquisitions.py:159-183): one maximisation per group over
    # the group's own box, by whatever maximiser is configured (the tree search for 'pdoo' /
    # 'direct'), the group's posterior evaluated on the device for the rows the maximiser asks for
    if mean_funcs is None:
      mean_funcs = lambda x: np.array([0] * len(x))
    if not hasattr(mean_funcs, '__iter__'):
      mean_funcs = [mean_funcs] * len(groupings)
    for j, (grp, beta, mean_func_j) in enumerate(zip(groupings, betas, mean_funcs)):
      def _group_acq(X_j, _j=j, _beta=beta, _mean=mean_func_j):
        X_j = _as_2d_array(X_j)
        return group_ucb(_j, _beta, X_j, return_vals=True)[2] + _mean(X_j)
      anc_j = copy(anc_data)
      anc_j.max_evals = per_group_evals
      anc_j.domain = _BoxDomain(all_bounds[grp])
      point[grp] = maximise_acquisition(_group_acq, anc_j)
    return point
  if DEVICE_CANDIDATES:
    engine = fitted.engine
    widths = [len(grp) for grp in groupings]
    starts = np.concatenate([[0], np.cumsum([per_group_evals * w for w in widths])])
    flat = engine.empty((int(starts[-1]),))
    for grp, start in zip(groupings, starts):
      engine.random_candidates(per_group_evals, len(grp), bounds=all_bounds[grp], out=flat.offset(start))
    _, winners = all_ucb(betas, flat, sizes=[per_group_evals] * len(groupings))
    for grp, start, idx in zip(groupings, starts, winners):
      point[grp] = flat.slice(int(start) + int(idx) * len(grp), len(grp))
    return point
  cands = [map_to_bounds(np.random.random((per_group_evals, len(grp))), all_bounds[grp])
           for grp in groupings]
  _, winners = all_ucb(betas, cands)
  for grp, cands_g, idx in zip(groupings, cands, winners):
    point[grp] = cands_g[int(idx)]
  return point


def asy_add_ucb(gp, anc_data):
  if not isinstance(gp.kernel, AdditiveKernel):
    raise TypeError('add_ucb needs a GP with an AdditiveKernel.')
  fitted = gp.device_gp
  return _add_ucb(fitted, fitted.add_ucb_group, fitted.add_ucb_all, gp.kernel.groupings, None, anc_data)


# UCB ------------------------------------------------------------------------------------------
def _get_gp_ucb_dim(gp):
  """ The dimension that enters beta_t (gpb_acquisitions.py:202-209): an explicit gp.ucb_dim, the
      kernel's dimension, or 3. """
  explicit = getattr(gp, 'ucb_dim', None)
  if explicit is not None:
    return explicit
  return getattr(gp.kernel, 'dim', 3.0)


def _get_ucb_beta_th(dim, time_step):
  """ gpb_acquisitions.py:211-213 """
  return np.sqrt(0.5 * dim * np.log(2 * dim * time_step + 1))


def asy_ucb(gp, anc_data):
  """ mu + beta_t sigma  (gpb_acquisitions.py:215-223) """
  beta_th = _get_ucb_beta_th(_get_gp_ucb_dim(gp), anc_data.t)
  return _acquire(gp, anc_data, 'ucb', (beta_th, 0.0), lambda mu, sigma: mu + beta_th * sigma)


# PI -------------------------------------------------------------------------------------------
def asy_pi(gp, anc_data):
  """ Phi((mu - best) / sigma)  (gpb_acquisitions.py:230-239) """
  best = anc_data.curr_max_val
  return _acquire(gp, anc_data, 'pi', (best, 0.0), lambda mu, sigma: _ndtr((mu - best) / sigma))


# EI -------------------------------------------------------------------------------------------
def asy_ei(gp, anc_data):
  """ sigma (z Phi(z) + phi(z)), z = (mu - best) / sigma  (gpb_acquisitions.py:251-261) """
  best = anc_data.curr_max_val
  return _acquire(gp, anc_data, 'ei', (best, 0.0),
                  lambda mu, sigma: sigma * _expected_improvement_for_norm_diff((mu - best) / sigma))


# TTEI -----------------------------------------------------------------------------------------
def _ttei(gp_eval, anc_data, ref_point, gp=None):
  """ Expected improvement over a reference point, with the combined standard deviation
      (gpb_acquisitions.py:269-280). """
  ref_mean, ref_std = [float(np.ravel(v)[0]) for v in gp_eval([ref_point])]
  source = None if gp is None else _fused_source(gp, anc_data)
  if source is not None:
    return _fused_argmax(source(gp, anc_data), 'ttei', (ref_mean, ref_std))
  def _tt_ei_acq(x):
    mu, sigma = gp_eval(x)
    comb_std = np.sqrt(ref_std ** 2 + sigma ** 2)
    return comb_std * _expected_improvement_for_norm_diff((mu - ref_mean) / comb_std)
  return maximise_acquisition(_tt_ei_acq, anc_data)


def asy_ttei(gp, anc_data):
  """ Top-two EI (gpb_acquisitions.py:282-294): with probability 1/2 plain EI; otherwise EI with
      half the budget gives the reference point and the other half maximises the improvement over
      it.  The coin is the first np.random.random() call, as in the reference. """
  if np.random.random() < 0.5:
    return asy_ei(gp, anc_data)
  halved = copy(anc_data)
  halved.max_evals = anc_data.max_evals // 2
  ei_argmax = asy_ei(gp, halved)
  return _ttei(_get_gp_eval_for_parallel_strategy(gp, halved, 'std'), halved, ei_argmax, gp)


# Random ---------------------------------------------------------------------------------------
def asy_rand(_, anc_data):
  """ gpb_acquisitions.py:301-306: maximise a random acquisition.  The reference's objective
      returns ONE random number per call and is called point by point by its tree searches; the
      batched searches here hand over k points per call and get k numbers back (the 'rand'
      maximiser's single call with all candidates still draws one, as in the reference). """
  vectorised = anc_data.acq_opt_method == 'rand'
  return maximise_acquisition(lambda x: np.random.random((1,) if vectorised else (len(x),)), anc_data)


# Multi-fidelity strategies (gpb_acquisitions.py:313-439) ----------------------------------------
def _get_fidel_to_opt_gp(mfgp, fidel_to_opt):
  """ gpb_acquisitions.py:314-332 """
  return FidelToOptGP(mfgp, fidel_to_opt)


def asy_add_ucb_for_boca(mfgp, fidel_to_opt, anc_data):
  """ gpb_acquisitions.py:334-392: _add_ucb for a multi-fidelity GP with an additive domain model, at fidel_to_opt.
      Group j's cross matrix is kern_scale * k_fid(Z, fidel_to_opt) * k_j(x_j, X[:, group j]), its prior variance
      kern_scale * k_fid(f2o, f2o) * k_j(x, x); L and alpha are the joint GP's and stay in HBM
      (FittedGP.mf_add_ucb_group / _all). """
  fitted = mfgp.device_gp
  return _add_ucb(fitted, partial(fitted.mf_add_ucb_group, fidel_to_opt), partial(fitted.mf_add_ucb_all, fidel_to_opt),
                  mfgp.domain_kernel.groupings, None, anc_data)


def syn_add_ucb_for_boca(num_workers, list_of_mfgps, fidel_to_opt, anc_data):
  """ gpb_acquisitions.py:394-397 """
  # pylint: disable=unused-argument
  raise NotImplementedError('Not Implemented Yet!')


def boca(select_pt_func, mfgp, anc_data, func_caller):
  """ BOCA's decision (gpb_acquisitions.py:399-439; Kandasamy et al. 2017): the next point by the
      acquisition at fidel_to_opt -- fused on the device through FidelToOptGP, add-UCB through
      mf_add_ucb_* -- then the fidelity: among the caller's candidate fidelities those whose posterior
      standard deviation at the point (one eval_at_fidel call) exceeds the threshold, the cheapest of
      them unless it costs more than boca_max_low_fidel_cost_ratio of fidel_to_opt. """
  if anc_data.curr_acq == 'add_ucb':
    next_eval_point = asy_add_ucb_for_boca(mfgp, func_caller.fidel_to_opt, anc_data)
  else:
    fidel_to_opt_gp = _get_fidel_to_opt_gp(mfgp, func_caller.fidel_to_opt)
    next_eval_point = select_pt_func(fidel_to_opt_gp, anc_data)
  candidate_fidels, cost_ratios = func_caller.get_candidate_fidels_and_cost_ratios(next_eval_point, filter_by_cost=True)
  num_candidates = len(candidate_fidels)
  cost_ratios = np.array(cost_ratios)
  sqrt_cost_ratios = np.sqrt(cost_ratios)
  information_gaps = np.array(func_caller.get_information_gap(candidate_fidels))
  _, cand_fidel_stds = mfgp.eval_at_fidel(candidate_fidels, [next_eval_point] * num_candidates, uncert_form='std')
  cand_fidel_stds = cand_fidel_stds / np.sqrt(mfgp.kernel.hyperparams['scale'])
  std_thresholds = anc_data.boca_thresh_coeff * anc_data.y_range * sqrt_cost_ratios * information_gaps
  high_std_idxs = cand_fidel_stds > std_thresholds
  qualifying_idxs = np.where(high_std_idxs)[0]
  if len(qualifying_idxs) == 0:
    return func_caller.fidel_to_opt, next_eval_point
  qualifying_fidels = [candidate_fidels[idx] for idx in qualifying_idxs]
  qualifying_sqrt_cost_ratios = sqrt_cost_ratios[qualifying_idxs]
  qualifying_cost_ratios = cost_ratios[qualifying_idxs]
  next_eval_fidel_idx = qualifying_sqrt_cost_ratios.argmin()
  # a qualifying fidelity that costs nearly as much as fidel_to_opt is not worth the detour
  if qualifying_cost_ratios[next_eval_fidel_idx] > anc_data.boca_max_low_fidel_cost_ratio:
    return func_caller.fidel_to_opt, next_eval_point
  return qualifying_fidels[next_eval_fidel_idx], next_eval_point


# Synchronous versions (gpb_acquisitions.py:129, 191, 225, 241, 263, 296, 308) -------------------
def _synchronous(asy_acq):
  def syn_acq(num_workers, list_of_gps, anc_datas):
    return _get_syn_recommendations_from_asy(asy_acq, num_workers, list_of_gps, anc_datas)
  syn_acq.__name__ = asy_acq.__name__.replace('asy_', 'syn_')
  return syn_acq


syn_ts, syn_add_ucb, syn_ucb = _synchronous(asy_ts), _synchronous(asy_add_ucb), _synchronous(asy_ucb)
syn_pi, syn_ei, syn_ttei, syn_rand = _synchronous(asy_pi), _synchronous(asy_ei), _synchronous(asy_ttei), \
                                     _synchronous(asy_rand)

_ASY = dict(ucb=asy_ucb, add_ucb=asy_add_ucb, ei=asy_ei, pi=asy_pi, ttei=asy_ttei, ts=asy_ts, rand=asy_rand)
asy = Namespace(**_ASY)
seq = Namespace(**_ASY)
syn = Namespace(ucb=syn_ucb, add_ucb=syn_add_ucb, ei=syn_ei, pi=syn_pi, ttei=syn_ttei, ts=syn_ts,
                rand=syn_rand)
