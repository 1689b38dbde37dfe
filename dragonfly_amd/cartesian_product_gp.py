"""GPs on Cartesian-product domains on the MI355X: the reference's own CPGP
(dragonfly/gp/cartesian_product_gp.py:208-248) re-based onto the device GP at install() time.

A CPGP's kernel is a product over the parts of the domain (Euclidean, integral, discrete, neural-
network, ...), not guaranteed to be positive semi-definite, so the reference builds its posterior
through _get_cholesky_decomp's 'project_first' branch (gp_core.py:838-841: eigen-projection of the
Gram matrix onto the PSD cone) and projects every posterior covariance as well (gp_core.py:849-857).
When the kernel is our CartesianProductKernel mirror with SE / Matern / exponential-decay / Hamming parts
(kernel.py: has_device_spec) and no part comes with pre-computed distances, the GP runs from the
descriptor: the list-of-lists points are packed into one dense matrix (categories as codes), the Gram
matrix is built, projected (csrc/psdproj.hip) and factored on the device (dfh_gp_fit with
DFH_FIT_PROJECT_FIRST), and no n x n matrix crosses PCIe.  With any other kernel object (the
reference's CartesianProductKernel, a neural-network part, distance lists) the kernel is evaluated on
the host as the reference does, and the projection, the factorisation, the solves and the posterior
run on the device: the GP of gp_core.py in host-kernel mode.

Nothing of the reference class is restated here.  device_cpgp_class(ref_module) makes a class whose
base is dragonfly_amd.gp_core.GP and whose body IS the reference class's body -- its constructor, its
distance-list setter, its string form and its training-kernel-matrix hook, the function objects
themselves.  Overriding that documented hook is what puts the device GP into host-kernel mode
(dfh_gp_fit_gram with DFH_FIT_PROJECT_FIRST), so build_posterior / eval / the hallucinated posterior
are the device's and everything else is the reference's; the class adds only the test for the
descriptor route and the packing of the points.

dragonfly_amd.install(cartesian_product=True) rebinds dragonfly.gp.cartesian_product_gp.CPGP to that
class: the reference's CPGPFitter constructs its GPs through the module global
(cartesian_product_gp.py: `CPGP(X, Y, kernel, mean_func, noise_var, ...)`), so Cartesian-product
runs -- the reference's default for every non-Euclidean domain -- get the device posterior.
"""
import types

from .gp_core import GP
from .kernel import CartesianProductKernel
from .mf_gp import MFGP


def runs_from_descriptor(kernel, *lists_of_dists):
  """ The kernel is our mirror, every part has a device description, and no part -- of any of the spaces whose
      distance lists are given -- comes with pre-computed distances.  The one definition of "runs from the descriptor":
      the GP classes below ask it of themselves, the batched fitters' stand-ins (batched_fitter.py) of a candidate. """
  return isinstance(kernel, CartesianProductKernel) and kernel.has_device_spec() and \
         all(dists is None for lists in lists_of_dists for dists in lists or [])


def _generic(self):
  """ gp_core.GP._generic: host-kernel mode unless the GP runs from the descriptor. """
  return not runs_from_descriptor(self.kernel, getattr(self, 'domain_lists_of_dists', None))


def _points_array(self, X):
  """ gp_core.GP._points_array: the points packed as the kernel's descriptor expects them. """
  return self.kernel.pack(X)


def _uses_mf_descriptor(self):
  """ CPMFGP: the kernel is our mirror over exactly [fidel_space_kernel, domain_kernel] -- two product factors of
      one descriptor (kernel.py: a part that is itself a product) --, every member has a device description, and no
      member of either space is given by distances.  Then kernel_scale * KF * KD of the reference's training-matrix
      hook (cartesian_product_gp.py:310-319) is the descriptor's value, rounding for rounding. """
  kern = self.kernel
  fidel_kernel, domain_kernel = getattr(self, 'fidel_space_kernel', None), getattr(self, 'domain_kernel', None)
  if fidel_kernel is None or domain_kernel is None or not isinstance(kern, CartesianProductKernel):
    return False
  parts = kern.kernel_list
  if len(parts) != 2 or parts[0] is not fidel_kernel or parts[1] is not domain_kernel or \
     not all(isinstance(part, CartesianProductKernel) for part in parts) or \
     kern.hyperparams['scale'] != self.kernel_scale:
    return False
  return runs_from_descriptor(kern, getattr(self, 'fidel_space_lists_of_dists', None),
                              getattr(self, 'domain_lists_of_dists', None))


def _mf_generic(self):
  """ gp_core.GP._generic for CPMFGP: host-kernel mode unless the GP runs from the descriptor. """
  return not _uses_mf_descriptor(self)


def _rebased_functions(ref_cls, env):
  """ The functions (and class methods) of the reference class's body, re-made over the globals `env`. """
  def remake(fn):
    new = types.FunctionType(fn.__code__, env, fn.__name__, fn.__defaults__, fn.__closure__)
    new.__kwdefaults__ = fn.__kwdefaults__
    new.__doc__ = fn.__doc__
    return new
  body = {}
  for name, fn in vars(ref_cls).items():
    if isinstance(fn, types.FunctionType):
      body[name] = remake(fn)
    elif isinstance(fn, classmethod):
      body[name] = classmethod(remake(fn.__func__))
  return body


_classes = {}      # reference module name -> the class made for it
_mf_classes = {}   # the same for CPMFGP


def device_cpgp_class(ref_module):
  """ ref_module: dragonfly.gp.cartesian_product_gp (as imported by the caller).  Returns the class described above,
      one per reference module (a second call returns the same class), published as CPGP of this module: the class and
      its instances pickle by that name, in a process that has made the class (install() does) -- the one made last
      if several reference modules are in use.
      The reference's constructor names its own class in `super(CPGP, self)`, a module global: the functions are
      re-made over a copy of the module's globals in which that name is the new class, so the class works whether or
      not the module global has been rebound. """
  if ref_module.__name__ in _classes:
    return _classes[ref_module.__name__]
  ref_cls = ref_module.__dict__.get('_dfh_reference_CPGP', ref_module.CPGP)
  env = dict(ref_module.__dict__)
  body = {'__doc__': ref_cls.__doc__, '__module__': __name__,
          '_generic': property(_generic), '_points_array': _points_array}
  body.update(_rebased_functions(ref_cls, env))
  cls = type('CPGP', (GP,), body)
  env['CPGP'] = cls
  _classes[ref_module.__name__] = cls
  globals()['CPGP'] = cls
  return cls


def is_device_cpmfgp(gp):
  """ An instance of a class device_cpmfgp_class made. """
  return any(isinstance(gp, cls) for cls in _mf_classes.values())


def device_cpmfgp_class(ref_module):
  """ The same recipe for the reference's CPMFGP (cartesian_product_gp.py:251-319), the multi-fidelity GP on a
      Cartesian-product domain: its own function objects -- constructor, distance-list setters, string form, the
      training-kernel-matrix hook and the class method behind it -- over dragonfly_amd.mf_gp.MFGP, one class per
      reference module, published as CPMFGP of this module.  The constructor builds the joint kernel by the name
      CartesianProductKernel: in the functions' globals that name is our mirror, so a GP made from
      (kernel_scale, fidel_space_kernel, domain_kernel) mirrors gets the nested mirror and, when _uses_mf_descriptor
      holds, runs from ONE product descriptor with two product factors; the joint points are (z, x) pairs, packed side
      by side.  In every other case the hook puts the GP in host-kernel mode, as for CPGP. """
  if ref_module.__name__ in _mf_classes:
    return _mf_classes[ref_module.__name__]
  ref_cls = ref_module.__dict__.get('_dfh_reference_CPMFGP', ref_module.CPMFGP)
  env = dict(ref_module.__dict__)
  env['CartesianProductKernel'] = CartesianProductKernel
  body = {'__doc__': ref_cls.__doc__, '__module__': __name__,
          '_generic': property(_mf_generic), '_points_array': _points_array}
  body.update(_rebased_functions(ref_cls, env))
  cls = type('CPMFGP', (MFGP,), body)
  env['CPMFGP'] = cls
  _mf_classes[ref_module.__name__] = cls
  globals()['CPMFGP'] = cls
  return cls
