"""Kernels evaluated on the MI355X: SE, Matern, Polynomial, Exponential-decay, Additive, coordinate-wise
Product and ESP (elementary symmetric polynomial of 1-D kernels) on Euclidean inputs, the Hamming kernel on
categorical ones, and the Cartesian-product kernel over the parts of a mixed domain.

Host-side counterpart of dragonfly/gp/kernel.py: the class names, constructor arguments, the
`hyperparams` dictionary, the printed form and the error behaviour are the reference's (its lines
are quoted in the docstrings), so code written against the reference's kernels runs unchanged.
The Gram / cross matrices themselves are produced by libdfhip.so (csrc/kernmat.hip and the km_*.hip units) -- there is no
NumPy evaluation path here, except for grouped kernels with a factor the device does not know,
which are composed from their factors' own evaluations.
"""
import numpy as np

from .engine import KernelSpec, get_engine


def _as_2d_array(X):
  """ The reference passes lists of 1-D arrays (gp_core.py:129-130) or 2-D arrays. """
  X = np.asarray(X, dtype=np.float64)
  if X.ndim == 1:
    X = X.reshape((len(X), -1)) if X.size else X.reshape((0, 0))
  return np.ascontiguousarray(X)


def _scale_and_bandwidth_text(kern):
  """ The two fragments the reference prints for SE / Matern kernels (kernel.py:48-57): the mean
      bandwidth above six dimensions, the individual ones otherwise. """
  bws = kern.hyperparams['dim_bandwidths']
  if kern.dim <= 6:
    bw_text = 'bws:[%s]' % (' '.join('%0.2f' % (b) for b in bws))
  else:
    bw_text = 'avg-bw: %0.4f' % (bws.mean())
  return 'sc:%0.4f' % (kern.hyperparams['scale']), bw_text


def _bandwidth_vector(dim, bandwidths, allow_scalar):
  """ Per-dimension bandwidths as the reference stores them (kernel.py:151-160, 247-250): a
      vector of length dim (checked), or one value repeated; None stays None. """
  if bandwidths is None:
    return None
  if hasattr(bandwidths, '__len__'):
    if len(bandwidths) != dim:
      raise ValueError('Dimension of dim_bandwidths should be the same as dimension.')
    return np.array(bandwidths).T
  if not allow_scalar:
    raise ValueError('Dimension of dim_bandwidths should be the same as dimension.')
  return np.array([bandwidths] * dim).T


class Kernel(object):
  """ Base class (kernel.py:60-129): a callable returning the n1 x n2 kernel matrix, with its
      parameters in the dictionary `hyperparams`. """

  def __init__(self):
    self.hyperparams = dict()

  def is_guaranteed_psd(self):
    raise NotImplementedError('Implement in a child class.')

  def evaluate(self, X1, X2=None):
    """ kernel.py:76-83; empty inputs give an empty matrix without touching the device. """
    if X2 is None:
      X2 = X1
    n1, n2 = len(X1), len(X2)
    if n1 == 0 or n2 == 0:
      return np.zeros((n1, n2))
    return self._child_evaluate(X1, X2)

  __call__ = evaluate

  def _child_evaluate(self, X1, X2):
    raise NotImplementedError('Implement in a child class.')

  def set_hyperparams(self, **kwargs):
    """ Replaces the whole dictionary (kernel.py:110-112). """
    self.hyperparams = dict(kwargs)

  def add_hyperparams(self, **kwargs):
    """ Adds / overwrites entries (kernel.py:114-117). """
    self.hyperparams.update(kwargs)

  def to_spec(self, in_dim=None):
    """ Description handed to the C-ABI (struct dfh_kernel_desc). in_dim: number of columns of
        the inputs (only a grouped kernel cannot tell it from its own parameters). """
    raise NotImplementedError('Implement in a child class.')

  def __str__(self):
    return '%s:: %s'%(type(self), str(self.hyperparams))


class _EuclideanDeviceKernel(Kernel):
  """ Shared device evaluation of the Euclidean kernels. """

  def has_device_spec(self):
    """ False for a grouped kernel with a factor the device does not evaluate (e.g. the reference's
        PolyKernel inside a product): it is then composed on the host from its factors' own
        evaluations, and GPs using it run in host-kernel mode (gp_core.GP._generic). """
    return True

  def _child_evaluate(self, X1, X2):
    A = _as_2d_array(X1)
    B = None if X2 is X1 else _as_2d_array(X2)
    if B is not None and A.shape[1] != B.shape[1]:
      raise ValueError('Second dimension of X1 and X2 should be equal.')   # general_utils.py:64
    if not self.has_device_spec():
      return self._host_compose(A, A if B is None else B)
    return get_engine().kernel_matrix(self.to_spec(in_dim=A.shape[1]), A, B)

  # helpers of the reference's SE kernel that other parts of Dragonfly call (kernel.py:179-200)
  def get_scaled_repr(self, X):
    return X/self.hyperparams['dim_bandwidths']

  def get_effective_norm(self, X, order=None, is_single=True):
    scaled = self.get_scaled_repr(X)
    if is_single:
      return np.linalg.norm(scaled, ord=order)
    return np.array([np.linalg.norm(row, ord=order) for row in scaled])

  def compute_std_slack(self, X1, X2):
    pairwise = [float(self.evaluate(x1.reshape(1, -1), x2.reshape(1, -1))[0, 0]) for x1, x2 in zip(X1, X2)]
    return np.sqrt(self.hyperparams['scale'] - np.array(pairwise))

  def change_smoothness(self, factor):
    self.hyperparams['dim_bandwidths'] *= factor


class SEKernel(_EuclideanDeviceKernel):
  """ Squared exponential kernel scale * exp(-|x/bw - y/bw|^2 / 2) (kernel.py:132-222). """

  def __init__(self, dim, scale=None, dim_bandwidths=None):
    super(SEKernel, self).__init__()
    self.dim = dim
    self.set_se_hyperparams(scale, dim_bandwidths)

  def is_guaranteed_psd(self):
    return True

  def set_scale(self, scale):
    self.hyperparams['scale'] = scale

  def set_dim_bandwidths(self, dim_bandwidths):
    self.hyperparams['dim_bandwidths'] = _bandwidth_vector(self.dim, dim_bandwidths, allow_scalar=False)

  def set_single_bandwidth(self, bandwidth):
    self.hyperparams['dim_bandwidths'] = _bandwidth_vector(self.dim, bandwidth, allow_scalar=True)

  def set_se_hyperparams(self, scale, dim_bandwidths):
    """ kernel.py:167-173: a vector is taken per dimension, anything else as one common value. """
    self.set_scale(scale)
    self.hyperparams['dim_bandwidths'] = _bandwidth_vector(self.dim, dim_bandwidths, allow_scalar=True)

  def to_spec(self, in_dim=None):
    return KernelSpec('se', self.dim, self.hyperparams['scale'],
                      np.ravel(np.asarray(self.hyperparams['dim_bandwidths'], dtype=float)))

  def __str__(self):
    return 'SE: %s %s' % _scale_and_bandwidth_text(self)


class MaternKernel(_EuclideanDeviceKernel):
  """ The Matern class of kernels (kernel.py:225-328), nu = p + 1/2. """

  def __init__(self, dim, nu=None, scale=None, dim_bandwidths=None):
    super(MaternKernel, self).__init__()
    self.dim = dim
    self.p = None
    self.norm_constant = None
    self.set_matern_hyperparams(nu, scale, dim_bandwidths)

  def is_guaranteed_psd(self):
    return True

  def set_matern_hyperparams(self, nu, scale, dim_bandwidths):
    """ kernel.py:242-253; the half-integer check and its message are the reference's. """
    if nu%1 != 0.5:
      raise ValueError('Matern kernel: nu has to be p + 0.5 where p is an integer.')
    if hasattr(dim_bandwidths, '__len__'):
      bws = np.array(dim_bandwidths).T            # length is checked when the kernel is evaluated
    else:
      bws = np.array([dim_bandwidths] * self.dim).T
    self.hyperparams.update(nu=nu, scale=scale, dim_bandwidths=bws)
    self.p = int(nu)
    self.norm_constant = 1.0     # 1/value(0); the library evaluates it with the reference's formula

  def to_spec(self, in_dim=None):
    bws = np.ravel(np.asarray(self.hyperparams['dim_bandwidths'], dtype=float))
    if bws.size != self.dim:
      raise ValueError('Dimension of dim_bandwidths should be the same as dimension.')
    return KernelSpec('matern', self.dim, self.hyperparams['scale'], bws,
                      nu=self.hyperparams['nu'])

  def __str__(self):
    return 'Matern: nu=%0.1f %s %s' % ((self.hyperparams['nu'],) + _scale_and_bandwidth_text(self))


class PolyKernel(_EuclideanDeviceKernel):
  """ The polynomial kernel scale * ((x*s).(y*s) + 1)^order (kernel.py:331-395).  Not stationary:
      the prior variance k(x, x) depends on x (the library evaluates it per point). """

  def __init__(self, dim, order, scale, dim_scalings=None):
    super(PolyKernel, self).__init__()
    self.dim = dim
    self.set_poly_hyperparams(order, scale, dim_scalings)

  def is_guaranteed_psd(self):
    return True

  def set_order(self, order):
    self.add_hyperparams(order=order)

  def set_scale(self, scale):
    self.add_hyperparams(scale=scale)

  def set_dim_scalings(self, dim_scalings):
    """ kernel.py:356-364 """
    if dim_scalings is not None:
      if len(dim_scalings) != self.dim:
        raise ValueError('Dimension of dim_scalings should be dim.')
      dim_scalings = np.array(dim_scalings)
    self.add_hyperparams(dim_scalings=dim_scalings)

  def set_single_scaling(self, scaling):
    self.set_dim_scalings(None if scaling is None else [scaling] * self.dim)

  def set_poly_hyperparams(self, order, scale, dim_scalings):
    """ kernel.py:373-380 """
    self.set_order(order)
    self.set_scale(scale)
    if hasattr(dim_scalings, '__len__'):
      self.set_dim_scalings(dim_scalings)
    else:
      self.set_single_scaling(dim_scalings)

  def get_scaled_repr(self, X):
    return X * self.hyperparams['dim_scalings']

  def to_spec(self, in_dim=None):
    return _poly_spec(self)

  def __str__(self):
    return 'Poly: d=%d, scale=%0.2f, %s'%(self.hyperparams['order'], self.hyperparams['scale'],
                                          ','.join('%0.2f'%(elem) for elem in self.hyperparams['dim_scalings']))


class ExpDecayKernel(_EuclideanDeviceKernel):
  """ The kernel for exponentially decaying functions of Freeze-Thaw Bayesian optimisation,
      scale * prod_d (1 + x_d + y_d)^(-powers_d) + offset (kernel.py:398-437): the fidelity kernel of
      the reference's multi-fidelity GPs (euclidean_gp.py:881-887).  Not stationary. """

  def __init__(self, dim, scale=None, offset=None, powers=None):
    super(ExpDecayKernel, self).__init__()
    self.dim = dim
    if not hasattr(powers, '__iter__'):
      powers = [powers] * dim
    self.set_hyperparams(scale=scale, offset=offset, powers=powers)

  def is_guaranteed_psd(self):
    return True

  def get_scaled_repr(self, X):
    raise NotImplementedError('Not defined for the exponential-decay kernel.')

  def to_spec(self, in_dim=None):
    return _expdecay_spec(self)

  def __str__(self):
    return 'ExpDec: sc=%0.3f, offset=%0.3f, pow=%s'%(self.hyperparams['scale'], self.hyperparams['offset'],
        '[' + ', '.join('%0.3f'%(b) for b in np.ravel(self.hyperparams['powers'])) + ']')


def _factor_kind(kern):
  """ 'se' | 'matern' | 'poly' | 'expdecay' | None for a factor of a grouped kernel.  Decided by the
      class NAME and the hyper-parameters it carries, so that the reference's own PolyKernel /
      ExpDecayKernel objects (dragonfly/gp/kernel.py), which `install()` may leave in place inside a
      product kernel, reach the device as well. """
  hps = getattr(kern, 'hyperparams', None)
  if not isinstance(hps, dict):
    return None
  name = type(kern).__name__
  if isinstance(kern, SEKernel):
    return 'se'
  if isinstance(kern, MaternKernel):
    return 'matern'
  if name == 'PolyKernel' and all(k in hps for k in ('order', 'scale', 'dim_scalings')):
    order = hps['order']
    if hps['dim_scalings'] is not None and float(order) == int(order) and 0 <= int(order) <= 64:
      return 'poly'
  if name == 'ExpDecayKernel' and all(k in hps for k in ('scale', 'offset', 'powers')):
    if len(np.ravel(hps['powers'])) <= 8:
      return 'expdecay'
  if isinstance(kern, HammingKernel) and 1 <= len(np.ravel(hps['dim_weights'])) <= HAMMING_DEVICE_MAX_DIM and \
     _engine_knows_hamming():
    return 'hamming'
  return None


def _factor_fields(kern, kind):
  """ (scale, nu field, per-column field) of one factor, as struct dfh_kernel_desc carries them """
  hps = kern.hyperparams
  if kind == 'se':
    return hps['scale'], 0.0, np.ravel(np.asarray(hps['dim_bandwidths'], dtype=float))
  if kind == 'matern':
    return hps['scale'], hps['nu'], np.ravel(np.asarray(hps['dim_bandwidths'], dtype=float))
  if kind == 'poly':
    return hps['scale'], float(hps['order']), np.ravel(np.asarray(hps['dim_scalings'], dtype=float))
  if kind == 'hamming':
    return 1.0, 0.0, np.ravel(np.asarray(hps['dim_weights'], dtype=float))
  return hps['scale'], float(hps['offset']), np.ravel(np.asarray(hps['powers'], dtype=float))


def _poly_spec(kern):
  scale, order, scalings = _factor_fields(kern, 'poly')
  if scalings.size != kern.dim:
    raise ValueError('Dimension of dim_scalings should be dim.')
  return KernelSpec('poly', kern.dim, scale, scalings, nu=order)


def _expdecay_spec(kern):
  scale, offset, powers = _factor_fields(kern, 'expdecay')
  if powers.size != kern.dim:
    raise ValueError('Dimension of powers should be dim.')
  return KernelSpec('expdecay', kern.dim, scale, powers, nu=offset)


class _GroupedKernel(_EuclideanDeviceKernel):
  """ A kernel assembled from SE / Matern factors on groups of coordinates: the additive kernel
      (sum) and the coordinate-wise product kernel.  `_groups()` gives the coordinate lists. """
  _kind = None
  _label = None

  def _groups(self):
    raise NotImplementedError

  def is_guaranteed_psd(self):
    return all(kern.is_guaranteed_psd() for kern in self.kernel_list)

  def get_scaled_repr(self, X):
    raise NotImplementedError('Not defined for grouped kernels.')

  _factor_kinds = ('se', 'matern', 'poly')  # what the device evaluates inside this grouped kernel (poly: euclidean_gp.py:870-879)

  def has_device_spec(self):
    return all(_factor_kind(kern) in self._factor_kinds for kern in self.kernel_list)

  def to_spec(self, in_dim=None):
    groups = [[int(c) for c in grp] for grp in self._groups()]
    if len(groups) != len(self.kernel_list):
      raise ValueError("number of kernels do not correspond to number of groups.")
    kinds, scales, nus, bws = [], [], [], []
    for kern in self.kernel_list:
      kind = _factor_kind(kern)
      if kind not in self._factor_kinds:
        raise TypeError('%s on the device supports %s sub-kernels only, got %s.'
                        % (type(self).__name__, '/'.join(self._factor_kinds), type(kern)))
      scale, nu, per_col = _factor_fields(kern, kind)
      kinds.append(kind)
      nus.append(nu)
      scales.append(scale)
      bws.append(per_col)
    if in_dim is None:
      in_dim = max(1 + max(max(grp) for grp in groups), self.dim)
    return KernelSpec(self._kind, in_dim, self.hyperparams['scale'], groups=groups, sub_kinds=kinds,
                      sub_scales=scales, sub_nus=nus, sub_bandwidths=bws)

  def __str__(self):
    parts = ', '.join('%s(%s)' % (grp, kern) for grp, kern in zip(self._groups(), self.kernel_list))
    return '%s scale=%0.2f, %s' % (self._label, self.hyperparams['scale'], parts)


class AdditiveKernel(_GroupedKernel):
  """ Additive kernel scale * sum_g k_g(X[:, group g]) with non-overlapping groups
      (kernel.py:461-501). """
  _kind = 'additive'
  _label = 'ADD'

  def __init__(self, scale, kernel_list, groupings):
    if len(kernel_list) != len(groupings):
      raise ValueError("number of kernels do not correspond to number of groups.")
    super(AdditiveKernel, self).__init__()
    self.hyperparams['scale'] = scale
    self.kernel_list, self.groupings = kernel_list, groupings
    self.dim = sum(kern.dim for kern in kernel_list)

  def _groups(self):
    return self.groupings

  def _host_compose(self, X1, X2):
    """ kernel.py:484-494 with each factor evaluated by its own class """
    total = np.zeros((X1.shape[0], X2.shape[0]))
    for kern, grp in zip(self.kernel_list, self.groupings):
      total += kern(X1[:, grp], X2[:, grp])
    return self.hyperparams['scale'] * total


class CoordinateProductKernel(_GroupedKernel):
  """ Coordinate-wise product kernel scale * prod_i k_i(X[:, coordinate_list[i]])
      (kernel.py:541-591); the kernel of a Euclidean multi-fidelity GP (fidelity x domain). """
  _kind = 'product'
  _label = 'CoordProd'
  _factor_kinds = ('se', 'matern', 'poly', 'expdecay')

  def __init__(self, dim, scale, kernel_list=None, coordinate_list=None):
    super(CoordinateProductKernel, self).__init__()
    self.dim = dim
    self.hyperparams['scale'] = scale
    self.kernel_list, self.coordinate_list = kernel_list, coordinate_list

  def _groups(self):
    return self.coordinate_list

  def set_kernel_list(self, kernel_list):
    self.kernel_list = kernel_list

  def set_new_kernel(self, kernel_idx, new_kernel):
    self.kernel_list[kernel_idx] = new_kernel

  def set_kernel_hyperparams(self, kernel_idx, **kwargs):
    self.kernel_list[kernel_idx].set_hyperparams(**kwargs)

  @staticmethod
  def _additive_factor(kern):
    """ An AdditiveKernel among the product's kernels (ours or, left in place by `install()`, the
        reference's): the multi-fidelity GP with an additive domain model, euclidean_gp.py:696-707 """
    return type(kern).__name__ == 'AdditiveKernel' and hasattr(kern, 'kernel_list') and hasattr(kern, 'groupings') \
           and isinstance(getattr(kern, 'hyperparams', None), dict) and 'scale' in kern.hyperparams

  def has_device_spec(self):
    for kern in self.kernel_list:
      if self._additive_factor(kern):
        if not all(_factor_kind(k) in AdditiveKernel._factor_kinds for k in kern.kernel_list):
          return False
      elif _factor_kind(kern) not in self._factor_kinds:
        return False
    return True

  def to_spec(self, in_dim=None):
    in_dim = self.dim if in_dim is None else in_dim
    if not any(self._additive_factor(kern) for kern in self.kernel_list):
      return super(CoordinateProductKernel, self).to_spec(in_dim)
    # additive factors: their groups are listed with the product's own, in absolute coordinates
    if len(self.coordinate_list) != len(self.kernel_list):
      raise ValueError("number of kernels do not correspond to number of groups.")
    groups, kinds, scales, nus, bws, gfac, fsum, fscale = [], [], [], [], [], [], [], []
    for f, (kern, coords) in enumerate(zip(self.kernel_list, self.coordinate_list)):
      coords = [int(c) for c in coords]
      if self._additive_factor(kern):
        if len(kern.kernel_list) != len(kern.groupings):
          raise ValueError("number of kernels do not correspond to number of groups.")
        members = [(k, [coords[int(c)] for c in grp]) for k, grp in zip(kern.kernel_list, kern.groupings)]
        allowed = AdditiveKernel._factor_kinds
        fsum.append(True)
        fscale.append(kern.hyperparams['scale'])
      else:
        members = [(kern, coords)]
        allowed = self._factor_kinds
        fsum.append(False)
        fscale.append(1.0)
      for k, cols in members:
        kind = _factor_kind(k)
        if kind not in allowed:
          raise TypeError('%s on the device supports %s sub-kernels only, got %s.'
                          % (type(self).__name__, '/'.join(allowed), type(k)))
        scale, nu, per_col = _factor_fields(k, kind)
        groups.append(cols); kinds.append(kind); scales.append(scale); nus.append(nu); bws.append(per_col)
        gfac.append(f)
    return KernelSpec('product', in_dim, self.hyperparams['scale'], groups=groups, sub_kinds=kinds,
                      sub_scales=scales, sub_nus=nus, sub_bandwidths=bws, group_factors=gfac, factor_sums=fsum,
                      factor_scales=fscale)

  def _host_compose(self, X1, X2):
    """ kernel.py:578-589 with each factor evaluated by its own class """
    K = self.hyperparams['scale'] * np.ones((X1.shape[0], X2.shape[0]))
    for kern, coords in zip(self.kernel_list, self.coordinate_list):
      K *= kern(X1[:, coords], X2[:, coords])
    return K


# Orders above this stay in host-kernel mode: the device keeps the power sums in registers (csrc/km_esp.hip), and at
# such orders the reference's Newton-Girard recursion is dominated by cancellation in fp64 anyway.
ESP_DEVICE_MAX_ORDER = 32
ESP_DEVICE_MAX_DIM = 256


class ESPKernel(_EuclideanDeviceKernel):
  """ The ESP kernel of Kandasamy & Yu (2016), 'Additive Approximations in High Dimensional
      Nonparametric Regression' (kernel.py:671-726): scale * e_order(k_0(x_0, y_0), .., k_{d-1}(x_{d-1},
      y_{d-1})), kernel_list[i] a 1-D kernel of column i.  The bandwidths live in kernel_list, `hyperparams`
      holds scale and order only. """

  def __init__(self, scale, order, kernel_list):
    super(ESPKernel, self).__init__()
    self.dim = len(kernel_list)
    self.kernel_list = kernel_list
    self.add_hyperparams(scale=scale, order=order)
    if self.dim < 0:
      raise ValueError("dim cannot not be negative")
    if order > self.dim:
      raise ValueError("order must be less than or equal to dim")
    if order < 1:
      raise ValueError("order must be an integer between 1 and dim")

  def is_guaranteed_psd(self):
    return all([kern.is_guaranteed_psd() for kern in self.kernel_list])

  def get_scaled_repr(self, X):
    raise NotImplementedError('Not defined for the ESP kernel.')

  def _members(self):
    """ (kind, scale, nu, bandwidth) of every column's kernel, or None if one is not a 1-D SE / Matern """
    out = []
    for kern in self.kernel_list:
      kind = _factor_kind(kern)
      if kind not in ('se', 'matern') or getattr(kern, 'dim', None) != 1:
        return None
      scale, nu, bws = _factor_fields(kern, kind)
      if bws.size != 1:
        return None
      out.append((kind, scale, nu, float(bws[0])))
    return out

  def has_device_spec(self):
    order = self.hyperparams['order']
    return float(order) == int(order) and 1 <= int(order) <= min(ESP_DEVICE_MAX_ORDER, self.dim) and \
           self.dim <= ESP_DEVICE_MAX_DIM and self._members() is not None

  def to_spec(self, in_dim=None):
    if not self.has_device_spec():
      raise TypeError('This ESP kernel does not run on the device (1-D SE / Matern members, order <= %d, '
                      'dim <= %d).' % (ESP_DEVICE_MAX_ORDER, ESP_DEVICE_MAX_DIM))
    if in_dim is not None and in_dim != self.dim:
      raise ValueError('Second dimension of X1 and X2 should be %d (one column per kernel).' % (self.dim))
    members = self._members()
    return KernelSpec('esp', self.dim, self.hyperparams['scale'], nu=int(self.hyperparams['order']),
                      sub_kinds=[m[0] for m in members], sub_scales=[m[1] for m in members],
                      sub_nus=[m[2] for m in members], sub_bandwidths=[[m[3]] for m in members])

  def _host_compose(self, X1, X2):
    """ kernel.py:693-726, the reference's formula with each column's kernel evaluated by its own class """
    order = self.hyperparams["order"]
    n1, n2 = X1.shape[0], X2.shape[0]
    kernel_matrices = [kern(X1[:, i:i+1], X2[:, i:i+1]) for i, kern in enumerate(self.kernel_list)]
    ones = np.ones((n1, n2))
    power_sum = [np.zeros((n1, n2)) for _ in range(order + 1)]
    power_sum[0] = ones
    for i in range(1, order + 1):
      for matrix in kernel_matrices:
        power_sum[i] += matrix ** i
    esp = [np.zeros((n1, n2)) for _ in range(order + 1)]
    esp[0] = ones
    for m in range(1, order + 1):
      for i in range(1, m + 1):
        esp[m] += ((-1) ** (i - 1)) * esp[m - i] * power_sum[i]
      esp[m] /= m
    return self.hyperparams["scale"] * esp[order]

  def __str__(self):
    return 'ESP: order=%d, sc=%0.4f, [%s]' % (int(self.hyperparams['order']), self.hyperparams['scale'],
                                              ', '.join(str(kern) for kern in self.kernel_list))


def _esp_bandwidth(dim_bandwidths, i):
  """ np.asscalar(dim_bandwidths[i]) of kernel.py:733, 741 """
  return np.asarray(dim_bandwidths[i]).item()


class ESPKernelSE(ESPKernel):
  """ ESP kernel with an SE kernel for each dimension (kernel.py:729-734) """

  def __init__(self, dim, scale, order, dim_bandwidths):
    kernel_list = [SEKernel(1, 1.0, _esp_bandwidth(dim_bandwidths, i)) for i in range(dim)]
    super(ESPKernelSE, self).__init__(scale, order, kernel_list)


class ESPKernelMatern(ESPKernel):
  """ ESP kernel with a Matern kernel for each dimension (kernel.py:737-742); nu is a list, one per dimension """

  def __init__(self, dim, nu, scale, order, dim_bandwidths):
    kernel_list = [MaternKernel(1, nu[i], 1.0, _esp_bandwidth(dim_bandwidths, i)) for i in range(dim)]
    super(ESPKernelMatern, self).__init__(scale, order, kernel_list)


# ---- categorical inputs and Cartesian-product domains ---------------------------------------------------------------
HAMMING_DEVICE_MAX_DIM = 32        # csrc/common.h: HAMMING_MAX_DIM
FACTOR_PRODUCT = 2                 # include/dfhip.h: DFH_FACTOR_PRODUCT, a factor_sums value


def _engine_knows_hamming():
  """ The engine in use evaluates DFH_KERNEL_HAMMING and takes the projection flags in gp_fit (engine.Engine does; an
      engine object written against the earlier interface says nothing, and kernels with a Hamming part then stay in
      host-kernel mode with it, as they were before the kind existed). """
  return 'hamming' in getattr(get_engine(), 'kernel_kinds', ())


class CategoryCoder(object):
  """ Integer codes for the categories of each column of a discrete part, so that the device can compare them
      as doubles.  Two items share a code exactly when the reference calls them equal: pairwise_hamming_kernel
      (general_utils.py:113-145) compares the elements of np.array(X, dtype=object) with np.equal, i.e. with the
      items' own `==` -- 1 == 1.0 (one code), 1 != '1' (two codes), and an np.str_ out of a string-coerced array
      equals the same str.  The dictionary of a column grows by first appearance, so training points, test points
      and points added later share codes.  Items that cannot be dictionary keys (unhashable, or not equal to
      themselves such as nan) have no faithful code: ValueError, and the caller stays on the host. """

  def __init__(self):
    self.columns = []

  def encode(self, part_points):
    """ part_points: one list (or 1-D array) of items per point -> float64 [n x dim] of codes. """
    rows = np.array([list(pt) for pt in part_points], dtype=object)
    if rows.ndim != 2:
      raise ValueError('The points of a discrete part must all have the same number of items.')
    n, dim = rows.shape
    while len(self.columns) < dim:
      self.columns.append({})
    out = np.empty((n, dim), dtype=np.float64)
    for c in range(dim):
      codes = self.columns[c]
      for i in range(n):
        item = rows[i, c]
        try:
          if not item == item:
            raise ValueError('An item that is not equal to itself has no category code: %r.' % (item,))
          code = codes.get(item)
          if code is None:
            code = codes[item] = len(codes)
        except TypeError:
          raise ValueError('An unhashable item has no category code: %r.' % (item,))
        out[i, c] = code
    return out

  def encode_many(self, part_points):
    """ encode() for many points at once: per column the distinct items are coded in order of first appearance
        -- the codes encode() would give them going down the rows -- and the column is mapped through the
        dictionary in one pass, with no Python statement per item.  Same codes, same dictionaries afterwards,
        same errors. """
    rows = np.array([list(pt) for pt in part_points], dtype=object)
    if rows.ndim != 2:
      raise ValueError('The points of a discrete part must all have the same number of items.')
    n, dim = rows.shape
    while len(self.columns) < dim:
      self.columns.append({})
    out = np.empty((n, dim), dtype=np.float64)
    for c in range(dim):
      codes = self.columns[c]
      items = rows[:, c].tolist()
      try:
        for item in dict.fromkeys(items):
          if not item == item:
            raise ValueError('An item that is not equal to itself has no category code: %r.' % (item,))
          if item not in codes:
            codes[item] = len(codes)
      except TypeError:
        bad = next(it for it in items if getattr(it, '__hash__', None) is None)
        raise ValueError('An unhashable item has no category code: %r.' % (bad,))
      out[:, c] = np.fromiter(map(codes.__getitem__, items), dtype=np.float64, count=n)
    return out


class HammingKernel(Kernel):
  """ The Hamming kernel sum_c w_c [x_c == y_c] on lists of categories (kernel.py:436-457).  A call on lists of
      items codes them (CategoryCoder, owned by this object) and compares the codes on the device. """

  def __init__(self, dim_weights):
    super(HammingKernel, self).__init__()
    if isinstance(dim_weights, (int, float)):
      dim_weights = np.ones((dim_weights,))/float(dim_weights)
    dim_weights = np.array(dim_weights)
    self.set_hyperparams(dim_weights=dim_weights)
    self.coder = CategoryCoder()

  @property
  def dim(self):
    return len(self.hyperparams['dim_weights'])

  def is_guaranteed_psd(self):
    return True

  def has_device_spec(self):
    return _factor_kind(self) == 'hamming'

  def to_spec(self, in_dim=None):
    weights = np.ravel(np.asarray(self.hyperparams['dim_weights'], dtype=float))
    return KernelSpec('hamming', weights.size, 1.0, weights, nu=0.0)

  def pack(self, X):
    """ The points' category codes as the n x dim matrix the device compares. """
    return self.coder.encode(X)

  def pack_many(self, X):
    """ pack() of many points (the candidates of an acquisition step) in one pass. """
    return self.coder.encode_many(X)

  def _child_evaluate(self, X1, X2):
    A = self.pack(X1)
    B = A if X2 is X1 else self.pack(X2)
    if A.shape[1] != B.shape[1]:
      raise ValueError('Second dimension of X1 and X2 should be equal.')
    if not self.has_device_spec():
      return self._host_compose(A, B)
    return get_engine().kernel_matrix(self.to_spec(), A, None if X2 is X1 else B)

  def _host_compose(self, A, B):
    """ general_utils.py:113-145 on the codes, for host-kernel mode (more than 32 columns, or an engine object
        that does not know the kind): the weighted matches of every row of the smaller operand, a row at a time """
    weights = np.ravel(np.asarray(self.hyperparams['dim_weights'], dtype=float))
    small, large, flip = (A, B, True) if len(B) < len(A) else (B, A, False)
    ret = np.zeros((len(large), len(small)))
    for idx, vec in enumerate(small):
      ret[:, idx] = (np.equal(large, vec) * weights).sum(axis=1)
    return ret.T if flip else ret

  def __str__(self):
    return 'Hamming: wts=%s'%('[' + ' '.join('%0.3f'%(w) for w in np.ravel(self.hyperparams['dim_weights'])) + ']')


class CartesianProductKernel(Kernel):
  """ scale * prod_j k_j(part j of x, part j of y) over the parts of a Cartesian-product domain (kernel.py:504-538).
      Every point is a list of per-part lists.  When every part is an SE, Matern, exponential-decay or Hamming
      mirror (an additive kernel of SE / Matern / polynomial groups too), the parts are laid side by side as
      column groups of ONE product descriptor and the kernel is evaluated by the device in one launch per matrix;
      with any other part the product is composed on the host from the parts' own evaluations, as the reference
      does, and GPs using it run in host-kernel mode. """
  _factor_kinds = ('se', 'matern', 'expdecay', 'hamming')

  def __init__(self, scale, kernel_list):
    super(CartesianProductKernel, self).__init__()
    self.kernel_list = kernel_list
    self.num_kernels = len(kernel_list)
    self.add_hyperparams(scale=scale)

  def is_guaranteed_psd(self):
    return all(kern.is_guaranteed_psd() for kern in self.kernel_list)

  @staticmethod
  def _product_factor(kern):
    """ A CartesianProductKernel mirror among the parts: the fidelity-space and the domain kernel of a multi-fidelity
        GP on a Cartesian-product domain (cartesian_product_gp.py:262-263).  Its point is a list of parts. """
    return isinstance(kern, CartesianProductKernel)

  def _part_dim(self, kern):
    if self._product_factor(kern):
      return kern.part_offsets()[1]
    kind = _factor_kind(kern)
    if kind == 'hamming':
      return len(np.ravel(kern.hyperparams['dim_weights']))
    return int(kern.dim)

  def has_device_spec(self):
    for kern in self.kernel_list:
      if self._product_factor(kern):
        # one level: the members of a product factor are single kernels the device knows
        if len(kern.kernel_list) == 0 or not all(_factor_kind(k) in self._factor_kinds for k in kern.kernel_list):
          return False
      elif CoordinateProductKernel._additive_factor(kern):
        if not all(_factor_kind(k) in AdditiveKernel._factor_kinds for k in kern.kernel_list):
          return False
      elif _factor_kind(kern) not in self._factor_kinds:
        return False
    return len(self.kernel_list) > 0

  def part_offsets(self):
    """ First column of every part in the packed matrix, and the total width (a product factor's parts side by side). """
    offs, at = [], 0
    for kern in self.kernel_list:
      offs.append(at)
      at += self._part_dim(kern)
    return offs, at

  def _as_coordinate_product(self):
    offs, total = self.part_offsets()
    coords = [list(range(o, o + self._part_dim(k))) for o, k in zip(offs, self.kernel_list)]
    return CoordinateProductKernel(total, self.hyperparams['scale'], self.kernel_list, coords)

  def to_spec(self, in_dim=None):
    """ One DFH_KERNEL_PRODUCT over the packed columns: part j is the column group [offset_j, offset_j + dim_j).  A part
        that is itself a product lists its members as groups of one factor with factor_sums = 2 (DFH_FACTOR_PRODUCT)
        and factor_scales = its own scale; the device multiplies in the reference's order. """
    if not self.has_device_spec():
      raise TypeError('This Cartesian-product kernel has a part the device does not evaluate.')
    inner = self._as_coordinate_product()
    inner._factor_kinds = self._factor_kinds
    if not any(self._product_factor(kern) for kern in self.kernel_list):
      return inner.to_spec(in_dim=None)
    groups, kinds, scales, nus, bws, gfac, fsum, fscale = [], [], [], [], [], [], [], []
    offs, total = self.part_offsets()
    for f, (kern, off) in enumerate(zip(self.kernel_list, offs)):
      if self._product_factor(kern):
        sub_offs, _ = kern.part_offsets()
        members = [(k, list(range(off + so, off + so + kern._part_dim(k)))) for k, so in zip(kern.kernel_list, sub_offs)]
        allowed = self._factor_kinds
        fsum.append(FACTOR_PRODUCT)
        fscale.append(kern.hyperparams['scale'])
      elif CoordinateProductKernel._additive_factor(kern):
        cols = list(range(off, off + self._part_dim(kern)))
        members = [(k, [cols[int(c)] for c in grp]) for k, grp in zip(kern.kernel_list, kern.groupings)]
        allowed = AdditiveKernel._factor_kinds
        fsum.append(1)
        fscale.append(kern.hyperparams['scale'])
      else:
        members = [(kern, list(range(off, off + self._part_dim(kern))))]
        allowed = self._factor_kinds
        fsum.append(0)
        fscale.append(1.0)
      for k, cols in members:
        kind = _factor_kind(k)
        if kind not in allowed:
          raise TypeError('%s on the device supports %s sub-kernels only, got %s.'
                          % (type(self).__name__, '/'.join(allowed), type(k)))
        scale, nu, per_col = _factor_fields(k, kind)
        groups.append(cols); kinds.append(kind); scales.append(scale); nus.append(nu); bws.append(per_col)
        gfac.append(f)
    return KernelSpec('product', total, self.hyperparams['scale'], groups=groups, sub_kinds=kinds, sub_scales=scales,
                      sub_nus=nus, sub_bandwidths=bws, group_factors=gfac, factor_sums=fsum, factor_scales=fscale)

  def pack(self, X, many=False):
    """ The reference's list-of-lists points as the dense n x d matrix of to_spec: Euclidean, integral and
        discrete-numeric parts become floats, the items of a Hamming part that kernel's category codes.
        many: the categories are coded a column at a time (pack_many). """
    offs, total = self.part_offsets()
    out = np.empty((len(X), total), dtype=np.float64)
    for j, (kern, off) in enumerate(zip(self.kernel_list, offs)):
      part = [pt[j] for pt in X]
      width = self._part_dim(kern)
      if self._product_factor(kern):
        block = kern.pack(part, many=many)               # the part of a point is itself a list of parts
      elif _factor_kind(kern) == 'hamming':
        block = kern.pack_many(part) if many else kern.pack(part)
      else:
        block = np.asarray(part, dtype=np.float64).reshape((len(X), -1))
      if block.shape[1] != width:
        raise ValueError('Part %d of the points has %d columns, its kernel %d.' % (j, block.shape[1], width))
      out[:, off:off + width] = block
    return out

  def pack_many(self, X):
    """ pack() for the thousands of candidates of one acquisition step: row for row the matrix pack() gives, the
        categories of every Hamming part coded by column instead of item by item. """
    return self.pack(X, many=True)

  def _host_compose(self, X1, X2):
    """ kernel.py:525-533 with every part evaluated by its own class """
    result = self.hyperparams['scale'] * np.ones((len(X1), len(X2)))
    for idx, kern in enumerate(self.kernel_list):
      result *= kern([pt[idx] for pt in X1], [pt[idx] for pt in X2])
    return result

  def _child_evaluate(self, X1, X2):
    if not self.has_device_spec():
      return self._host_compose(X1, X2)
    A = self.pack(X1)
    B = None if X2 is X1 else self.pack(X2)
    return get_engine().kernel_matrix(self.to_spec(), A, B)

  def __str__(self):
    kernels_str = ', '.join([str(kern) for kern in self.kernel_list])
    return 'DomProd scale=%0.2f, '%(self.hyperparams['scale']) + kernels_str
