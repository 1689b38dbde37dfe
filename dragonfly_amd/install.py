"""Install the MI355X engine under a real Dragonfly (the drop-in of SURVEY.md section 8b).

    import dragonfly_amd.install as dfi
    dfi.install()          # before building optimisers / calling maximise_function
    ...
    dfi.uninstall()

Every seam is a *name looked up at call time* in the reference, so no reference file is edited.  What each one
replaces, where the reference looks it up and when ours applies is the catalogue of INTEGRATION.md section 4; here
only which flag of install() enables it:
  S1     kernels (dragonfly.gp.kernel.SEKernel ...)                 always
  S2/S3  dragonfly.gp.euclidean_gp.EuclideanGP                      always
  S2'    EuclideanMFGP                                              multi_fidelity
  S2''   CPGP, HammingKernel, CartesianProductKernel                cartesian_product
  S2'''  CPMFGP                                                     cp_multi_fidelity
  S3     the bandits' EuclideanGPFitter (batched_fitter.py)         batched_tuning (default); tuning_gpus=N: over N GPUs
         ... their CPGPFitter / CPMFGPFitter                        with cartesian_product / cp_multi_fidelity
  S4     acquisition dispatchers in gpb_acquisitions.asy/syn/seq    always
  S4-CP  ... ours on Cartesian-product domains too                  cp_acquisitions
  S4'    multi-objective maximise_acquisition                       always
  S4''   multi-objective acquisition dispatchers                    multi_objective (with cp_acquisitions: product domains)
  S4'''  BOCA dispatcher                                            boca
  S4-CP-BOCA  ... ours on Cartesian-product domains too             boca, cp_acquisitions and cp_multi_fidelity
"""
from .batched_fitter import make_batched_fitter, make_batched_cp_fitter, _CPMFKernelMeanNoise


_saved = []     # (object, attribute name, original value)

# flag -> (the flags it needs, why): install() refuses the flag without them
_NEEDS = (
  ('boca', ('multi_fidelity',), 'BOCA runs on the device through the mirror MF GP.'),
  ('cp_acquisitions', ('cartesian_product',), 'the fused calls run on the device CP GP.'),
  ('cp_multi_fidelity', ('cartesian_product', 'multi_fidelity'),
   'the multi-fidelity GP of product domains runs on the device CP kernel mirrors.'),
)


def _check_flags(flags):
  for flag, needs, why in _NEEDS:
    if flags[flag] and not all(flags[need] for need in needs):
      raise ValueError('install(%s=True) needs %s: %s' % (flag, ' and '.join('%s=True' % need for need in needs), why))


def install(multi_fidelity=False, batched_tuning=True, cartesian_product=False, multi_objective=False, tuning_gpus=None,
            boca=False, cp_acquisitions=False, cp_multi_fidelity=False):
  """ Rebinds the names listed above; returns the list of patched attributes.  A flag without the flags it needs
      (_NEEDS) is a ValueError.  cp_acquisitions rebinds no name of its own: the dispatchers of S4, S4'' and S4'''
      call ours on Cartesian-product domains as well, where the predicates of gpb_acquisitions /
      multiobjective_gpb_acquisitions hold.
      tuning_gpus=N > 1 (with batched_tuning): a tuning batch large enough to fill more than one GPU
      (parallel.lml_shard_plan: more than 256 candidates up to n = 2047) is cut over N GPUs of this process
      (dfh_mgpu_lml_batch); every other batch, and everything with None or 1, goes exactly where it went before. """
  _check_flags(locals())
  import dragonfly.gp.kernel as ref_kernel
  import dragonfly.gp.euclidean_gp as ref_egp
  import dragonfly.opt.gpb_acquisitions as ref_acq
  from dragonfly.exd.exd_utils import maximise_with_method
  from . import kernel, euclidean_gp, gpb_acquisitions, mf_gp
  patched = []
  def _set(obj, name, new, label=None):
    """ obj: a module of the reference, or one of its acquisition namespaces (an object: `label` is its dotted name) """
    _saved.append((obj, name, getattr(obj, name)))
    setattr(obj, name, new)
    patched.append('%s.%s' % (label or obj.__name__, name))
  for name in ('SEKernel', 'MaternKernel', 'AdditiveKernel', 'ESPKernelSE', 'ESPKernelMatern'):
    _set(ref_kernel, name, getattr(kernel, name))
  _set(ref_egp, 'EuclideanGP', euclidean_gp.EuclideanGP)

  if multi_fidelity:
    # (opt-in: the reference's class cannot be reached once the name is rebound, its __init__ names itself in super())
    _set(ref_egp, 'EuclideanMFGP', mf_gp.EuclideanMFGP)
  if cartesian_product:
    import dragonfly.gp.cartesian_product_gp as ref_cpgp
    from . import cartesian_product_gp
    _set(ref_cpgp, 'CPGP', cartesian_product_gp.device_cpgp_class(ref_cpgp))
    # the CP kernel factory builds its Hamming parts and the product itself by these two names, looked up at call time
    # in both modules (cartesian_product_gp.py:19); the Euclidean parts already arrive as our mirrors
    for name in ('HammingKernel', 'CartesianProductKernel'):
      _set(ref_kernel, name, getattr(kernel, name))
      _set(ref_cpgp, name, getattr(kernel, name))
    if cp_multi_fidelity:
      _set(ref_cpgp, 'CPMFGP', cartesian_product_gp.device_cpmfgp_class(ref_cpgp))
  for ns_name in ('asy', 'syn', 'seq'):
    ref_ns, our_ns = getattr(ref_acq, ns_name), getattr(gpb_acquisitions, ns_name)
    for acq in ('ucb', 'ei', 'pi', 'ttei', 'ts', 'add_ucb'):
      _set(ref_ns, acq, _euclidean_dispatch(getattr(our_ns, acq), getattr(ref_ns, acq),
                                            _cp_predicate(acq) if cp_acquisitions else None),
           label='dragonfly.opt.gpb_acquisitions.' + ns_name)
  gpb_acquisitions.external_maximise_with_method = maximise_with_method
  if boca:
    _set(ref_acq, 'boca', _boca_dispatch(gpb_acquisitions.boca, ref_acq.boca,
                                         cp_boca=cp_acquisitions and cp_multi_fidelity))
  # the multi-objective acquisitions (opt/multiobjective_gpb_acquisitions.py:19-107) are closures
  # over rows of points handed to maximise_acquisition, a name they import at module level: with
  # ours they get the batched tree search / vectorised random search on Euclidean domains
  import dragonfly.opt.multiobjective_gpb_acquisitions as ref_moo_acq
  ref_maximise = ref_moo_acq.maximise_acquisition
  def _moo_maximise_acquisition(acq_fn, anc_data, *args, **kwargs):
    if anc_data.domain.get_type() == 'euclidean':
      return gpb_acquisitions.maximise_acquisition(acq_fn, anc_data, *args, **kwargs)
    return ref_maximise(acq_fn, anc_data, *args, **kwargs)
  _set(ref_moo_acq, 'maximise_acquisition', _moo_maximise_acquisition)
  if multi_objective:
    # the four acquisitions themselves, looked up with getattr in the namespaces asy / seq
    # (opt/multiobjective_gp_bandit.py): K posteriors or draws, scalarisation and arg-max in one device call
    from . import multiobjective_gpb_acquisitions as our_moo_acq
    for ns_name in ('asy', 'seq'):
      ref_ns, our_ns = getattr(ref_moo_acq, ns_name), getattr(our_moo_acq, ns_name)
      for acq in ('lin_ts', 'tch_ts', 'lin_ucb', 'tch_ucb'):
        _set(ref_ns, acq, _euclidean_dispatch(getattr(our_ns, acq), getattr(ref_ns, acq),
                                              _mo_cp_predicate(acq) if cp_acquisitions else None),
             label='dragonfly.opt.multiobjective_gpb_acquisitions.' + ns_name)
  if batched_tuning:
    import dragonfly.opt.gp_bandit as ref_gp_bandit
    import dragonfly.opt.multiobjective_gp_bandit as ref_moo_bandit
    batched = make_batched_fitter(ref_egp.EuclideanGPFitter, tuning_gpus=tuning_gpus)
    _set(ref_gp_bandit, 'EuclideanGPFitter', batched)
    _set(ref_moo_bandit, 'EuclideanGPFitter', batched)
    if cartesian_product:
      # the names the CP bandits construct their fitter by (gp_bandit.py, multiobjective_gp_bandit.py)
      batched_cp = make_batched_cp_fitter(ref_cpgp.CPGPFitter, tuning_gpus=tuning_gpus)
      _set(ref_gp_bandit, 'CPGPFitter', batched_cp)
      _set(ref_moo_bandit, 'CPGPFitter', batched_cp)
      if cp_multi_fidelity:
        _set(ref_gp_bandit, 'CPMFGPFitter', make_batched_cp_fitter(ref_cpgp.CPMFGPFitter, tuning_gpus=tuning_gpus,
                                                                   gp_name='CPMFGP', stand_in=_CPMFKernelMeanNoise))
  return patched


def _cp_predicate(acq):
  """ install(cp_acquisitions=True), the single-objective dispatchers: gpb_acquisitions.cp_acquisition_applies for every
      GP of the call -- the device CP GP on the descriptor route with a kernel guaranteed PSD, no multi-fidelity, 'rand'
      or the tree search; the GA, a compiled DIRECT, host-kernel GPs and add-UCB stay with the reference's callable. """
  from .gpb_acquisitions import cp_acquisition_applies, cp_boca_view_applies
  def applies(args, anc_data):
    gps = args[-2]
    gps = list(gps) if isinstance(gps, (list, tuple)) else [gps]
    # (BOCA's view of a product-domain GP exists only where _boca_dispatch let our boca() make it)
    return all(cp_acquisition_applies(acq, gp, anc_data) or cp_boca_view_applies(acq, gp, anc_data) for gp in gps)
  return applies


def _mo_cp_predicate(acq):
  """ install(multi_objective=True, cartesian_product=True, cp_acquisitions=True), the multi-objective dispatchers:
      multiobjective_gpb_acquisitions.mo_cp_acquisition_applies for the call's list of GPs. """
  from .multiobjective_gpb_acquisitions import mo_cp_acquisition_applies
  return lambda args, anc_data: mo_cp_acquisition_applies(acq, args[-2], anc_data)


def _euclidean_dispatch(ours, theirs, cp_applies=None):
  """ The acquisition entry installed in the reference's namespaces: ours on Euclidean domains,
      the reference's own callable on every other domain (Cartesian-product, neural-network, ...
      domains keep running exactly as before).  Works for asy (gp, anc_data) and syn
      (num_workers, gps, anc_datas) signatures: the ancillary data is the last argument.
      cp_applies(args, anc_data) -> bool, when given: ours on a Cartesian-product domain as well, where it holds
      (_cp_predicate, _mo_cp_predicate). """
  def acquisition(*args, **kwargs):
    anc_data = args[-1]
    if isinstance(anc_data, (list, tuple)):
      anc_data = anc_data[0]
    domain_type = anc_data.domain.get_type()
    if domain_type == 'euclidean' or \
       (cp_applies is not None and domain_type == 'cartesian_product' and cp_applies(args, anc_data)):
      return ours(*args, **kwargs)
    return theirs(*args, **kwargs)
  acquisition.__wrapped__ = ours
  acquisition.reference_callable = theirs
  return acquisition


def _boca_dispatch(ours, theirs, cp_boca=False):
  """ dragonfly.opt.gpb_acquisitions.boca under install(boca=True): ours for the mirror EuclideanMFGP with a device
      kernel on a Euclidean domain, the reference's own boca for everything else.
      cp_boca (install(boca=True, cp_acquisitions=True, cp_multi_fidelity=True)): ours on a Cartesian-product domain as
      well, where gpb_acquisitions.cp_boca_applies holds -- the device CPMFGP on the descriptor route, a kernel
      guaranteed PSD, not add-UCB. """
  from .gpb_acquisitions import cp_boca_applies, _is_device_gp
  from .mf_gp import EuclideanMFGP
  def boca(select_pt_func, mfgp, anc_data, func_caller):
    if (anc_data.domain.get_type() == 'euclidean' and isinstance(mfgp, EuclideanMFGP) and _is_device_gp(mfgp)) or \
       (cp_boca and cp_boca_applies(mfgp, anc_data)):
      return ours(select_pt_func, mfgp, anc_data, func_caller)
    return theirs(select_pt_func, mfgp, anc_data, func_caller)
  boca.__wrapped__ = ours
  boca.reference_callable = theirs
  return boca


def uninstall():
  """ Restores every name install() rebound. """
  from . import gpb_acquisitions, parallel
  for obj, name, old in reversed(_saved):
    setattr(obj, name, old)
  del _saved[:]
  parallel.close_tuning_engines()
  gpb_acquisitions.external_maximise_with_method = None
