"""Thin Python layer over the C-ABI: one Engine per GPU (dfh_ctx) and the fitted-GP handle.

Everything numeric happens in libdfhip.so; this module only marshals NumPy arrays and maps
status codes to the exceptions the reference raises at the same point.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (ACQ_EI, ACQ_MEAN, ACQ_PI, ACQ_STD, ACQ_TTEI, ACQ_UCB, GET_ALPHA, GET_K, GET_L,
                   INT32_MIN, KERNEL_ADDITIVE, KERNEL_ESP, KERNEL_EXPDECAY, KERNEL_HAMMING, KERNEL_MATERN, KERNEL_POLY, KERNEL_PRODUCT, KERNEL_SE,
                   KernelDesc,
                   check)

MO_SCALARISATIONS = {'lin': _lib.MO_LIN, 'tch': _lib.MO_TCH}
# dfh_ctx_counters out[2]: the route of the most recent kernel-matrix build (csrc/kernmat.h: KmRoute)
KM_ROUTES = (None, 'sym', 'cross_lds', 'strip', 'strip_mean', 'symmulti', 'generic', 'esp', 'colw')
# dfh_ctx_solve_launches out[16] (csrc/common.h: SolveCounter)
SOLVE_COUNTERS = ('trsv_blk_fwd', 'trsv_upd_fwd8', 'trsv_upd_fwd2', 'trsv_blk_bwd', 'trsv_upd_bwd16', 'trsv_upd_bwd64',
                  'trsv_general_blocks', 'refine_steps', 'skinny_1', 'skinny_2', 'skinny_4', 'skinny_4_split', 'skinny_8',
                  'skinny_8_split', 'skinny_16', 'skinny_16_split')
ACQ_IDS = {'mean': ACQ_MEAN, 'ucb': ACQ_UCB, 'ei': ACQ_EI, 'pi': ACQ_PI, 'ttei': ACQ_TTEI,
           'std': ACQ_STD}


def _f64(a):
  return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
  """ void* of a NumPy array, a DeviceArray, or None. """
  if a is None:
    return None
  if isinstance(a, DeviceArray):
    return a.ptr
  if isinstance(a, C.c_void_p):
    return a
  # (the address as an integer: what a.ctypes.data_as(c_void_p) passes, without building the ctypes view -- 1.1 against
  #  2.5 us, five times per call of a tuning objective that a real run evaluates a hundred thousand times)
  return a.__array_interface__['data'][0]


class DeviceArray(object):
  """ A float64 buffer resident in HBM (dfh_malloc). Passed to the C-ABI by pointer. """

  def __init__(self, engine, shape):
    self.engine = engine
    self.shape = tuple(int(s) for s in np.atleast_1d(shape))
    self.size = int(np.prod(self.shape))
    p = C.c_void_p()
    check(engine.lib.dfh_malloc(engine.ctx, self.size * 8, C.byref(p)))
    self.ptr = p

  def upload(self, host):
    host = _f64(host)
    assert host.size == self.size
    check(self.engine.lib.dfh_memcpy_h2d(self.engine.ctx, self.ptr, _ptr(host), self.size * 8))
    return self

  def download(self):
    out = np.empty(self.shape, dtype=np.float64)
    check(self.engine.lib.dfh_memcpy_d2h(self.engine.ctx, _ptr(out), self.ptr, self.size * 8))
    return out

  def slice(self, start, count):
    """ `count` doubles from element `start`, as a host array. """
    out = np.empty(int(count), dtype=np.float64)
    check(self.engine.lib.dfh_memcpy_d2h(self.engine.ctx, _ptr(out), self.offset(start), int(count) * 8))
    return out

  def row(self, i):
    """ Row i of a 2-D buffer as a host array (the winning candidate of a device-side search). """
    return self.slice(int(i) * self.shape[-1], self.shape[-1])

  def offset(self, n_elems):
    """ A raw pointer n_elems doubles into the buffer (no ownership). """
    return C.c_void_p(self.ptr.value + 8 * int(n_elems))

  def view(self, start, shape):
    """ A DeviceArray over the elements [start, start + prod(shape)) of this buffer: no copy, no
        ownership (it keeps this buffer alive; free() on the view does nothing). """
    v = DeviceArray.__new__(DeviceArray)
    v.engine = self.engine
    v.shape = tuple(int(x) for x in np.atleast_1d(shape))
    v.size = int(np.prod(v.shape))
    assert 0 <= int(start) and int(start) + v.size <= self.size
    v.ptr = self.offset(start)
    v._owner = self
    return v

  def free(self):
    if getattr(self, '_owner', None) is not None:      # a view
      self.ptr = None
      self._owner = None
      return
    if self.ptr is not None and self.engine.ctx is not None:
      self.engine.lib.dfh_free(self.engine.ctx, self.ptr)
    self.ptr = None

  def __del__(self):
    try:
      self.free()
    except Exception:     # pylint: disable=broad-except
      pass


_SINGLE_KINDS = {'se': KERNEL_SE, 'matern': KERNEL_MATERN, 'poly': KERNEL_POLY, 'expdecay': KERNEL_EXPDECAY,
                 'hamming': KERNEL_HAMMING}
_PSD_FLAGS = {'guaranteed_psd': 0, 'project_first': _lib.FIT_PROJECT_FIRST, 'try_before_project': _lib.FIT_TRY_BEFORE_PROJECT}


def _rows(Xs):
  """ Points as the library takes them: a DeviceArray as it is, anything else as a contiguous fp64 matrix; and their number. """
  if not isinstance(Xs, DeviceArray):
    Xs = _f64(Xs)
  return Xs, Xs.shape[0]


def _halluc_rows(X_halluc):
  """ (rows, q) of the points in progress; (None, 0) without any. """
  return (None, 0) if X_halluc is None or len(X_halluc) == 0 else _rows(X_halluc)


def _mean_vals_arg(mean_vals):
  """ Per-candidate prior means as the library takes them (None: the constant alone). """
  return mean_vals if mean_vals is None or isinstance(mean_vals, DeviceArray) else _f64(mean_vals)


def _group_blocks(cands_per_group, sizes, betas, who):
  """ The groups' candidates of an add-UCB call as (one flat buffer, m_g per group, beta per group): cands_per_group[g] is
      [m_g x |group g|] -- or ONE DeviceArray holding the blocks back to back, with sizes[g] = m_g. """
  if isinstance(cands_per_group, DeviceArray):
    flat = cands_per_group
    ms = np.ascontiguousarray(sizes, dtype=np.int64)
  else:
    blocks = [_f64(c) for c in cands_per_group]
    ms = np.ascontiguousarray([b.shape[0] for b in blocks], dtype=np.int64)
    flat = np.ascontiguousarray(np.concatenate([b.ravel() for b in blocks]), dtype=np.float64)
  be = _f64(np.asarray(betas, dtype=float).reshape(-1))
  if len(be) != len(ms):
    raise ValueError('%s: need one beta per group.' % who)
  return flat, ms, be


def _psd_flags(handle_non_psd_kernels):
  """ The fit flag of one of _get_cholesky_decomp's branches (gp_core.py:827-847). """
  if handle_non_psd_kernels not in _PSD_FLAGS:
    raise ValueError('Unknown option for handle_non_psd_kernels: %s' % (handle_non_psd_kernels))
  return _PSD_FLAGS[handle_non_psd_kernels]


_DESC_DTYPE = np.dtype({'names': [f[0] for f in KernelDesc._fields_],
                        'formats': ['<i4' if f[1] is C.c_int32 else ('<f8' if f[1] is C.c_double else '<u8') for f in KernelDesc._fields_],
                        'offsets': [getattr(KernelDesc, f[0]).offset for f in KernelDesc._fields_],
                        'itemsize': C.sizeof(KernelDesc)})


def _single_kind_descs(specs, d, backing):
  """ struct dfh_kernel_desc[len(specs)] for a list of SE / Matern / polynomial / exponential-decay candidates of
      dimension d, filled column-wise (a tuning batch holds thousands: 6 us of ctypes per candidate otherwise);
      None if some candidate has groups or a bandwidth vector of another length (to_desc reports those). """
  nb = len(specs)
  if nb == 0:
    return None
  try:
    kinds = [_SINGLE_KINDS[sp.kind] for sp in specs]
  except KeyError:
    return None
  if any(sp.bandwidths is None or sp.bandwidths.size != d or sp.dim != d for sp in specs):
    return None
  bw = np.empty((nb, d), dtype=np.float64)
  for i, sp in enumerate(specs):
    bw[i] = sp.bandwidths
  arr = np.zeros(nb, dtype=_DESC_DTYPE)
  arr['kind'] = kinds
  arr['dim'] = d
  arr['scale'] = [sp.scale for sp in specs]
  arr['nu'] = [sp.nu for sp in specs]
  base = bw.__array_interface__['data'][0]
  arr['bw'] = range(base, base + 8 * d * nb, 8 * d) if nb < 64 else base + np.arange(nb, dtype=np.uint64) * np.uint64(8 * d)
  backing += [bw, arr]
  return arr.ctypes.data_as(C.POINTER(KernelDesc))


class KernelSpec(object):
  """ Host-side description of a Euclidean kernel, convertible to struct dfh_kernel_desc.
      kind: 'se' | 'matern' | 'poly' (nu = order, bandwidths = dim_scalings) | 'expdecay' (nu =
      offset, bandwidths = powers) | 'hamming' (HammingKernel, kernel.py:436-457: bandwidths = dim_weights,
      scale 1, nu 0; the columns hold category codes) | 'additive' | 'product' (coordinate-wise product,
      kernel.py:541; its factors may be any of the five single kinds, an additive kernel's se / matern /
      poly -- with a hamming factor it is the reference's CartesianProductKernel, kernel.py:504-538).
      A product may hold ADDITIVE FACTORS (an AdditiveKernel among its kernels): list the factor's
      groups like any others and give group_factors[g] = index of the factor group g belongs to
      (non-decreasing), factor_sums[f] = True for an additive factor, factor_scales[f] = its scale.
      factor_sums[f] = 2 (DFH_FACTOR_PRODUCT): the factor is itself a product, factor_scales[f] * k_g * k_g' ...
      over its se / matern / expdecay / hamming groups (a CartesianProductKernel among the parts of one: CPMFGP).
      'esp' (ESPKernel, kernel.py:671-744): nu = order, one 1-D se / matern kernel per column in
      column order (sub_kinds / sub_scales / sub_nus / sub_bandwidths, one entry each; groups
      default to [[0], [1], ..]). """

  def __init__(self, kind, dim, scale, bandwidths=None, nu=0.0, groups=None, sub_kinds=None,
               sub_scales=None, sub_nus=None, sub_bandwidths=None, group_factors=None, factor_sums=None,
               factor_scales=None):
    self.kind = kind
    self.dim = int(dim)
    self.scale = float(scale)
    self.nu = float(nu) if nu is not None else 0.0
    self.bandwidths = None if bandwidths is None else _f64(np.ravel(bandwidths))
    self.groups = groups
    self.sub_kinds = sub_kinds
    self.sub_scales = sub_scales
    self.sub_nus = sub_nus
    self.sub_bandwidths = sub_bandwidths
    self.group_factors, self.factor_sums, self.factor_scales = group_factors, factor_sums, factor_scales
    if kind == 'esp' and groups is None:
      self.groups = [[c] for c in range(self.dim)]
    self._keep = []

  def signature(self):
    """ Hashable value identifying the kernel exactly (used to decide whether a cached posterior
        was built with the same kernel). """
    def _t(a):
      return None if a is None else tuple(np.ravel(np.asarray(a, dtype=float)).tolist())
    groups = None if self.groups is None else tuple(tuple(int(c) for c in g) for g in self.groups)
    subs = None if self.sub_bandwidths is None else tuple(_t(b) for b in self.sub_bandwidths)
    kinds = None if self.sub_kinds is None else tuple(self.sub_kinds)
    return (self.kind, self.dim, self.scale, self.nu, _t(self.bandwidths), groups, kinds,
            _t(self.sub_scales), _t(self.sub_nus), subs, _t(self.group_factors), _t(self.factor_sums),
            _t(self.factor_scales))

  def to_desc(self):
    """ Builds the ctypes struct.  The arrays it points at are kept alive both on the struct
        (d.backing) and on self -- appended, never dropped, so an earlier descriptor of the same
        spec stays valid (a list of specs may hold one object several times). """
    d = KernelDesc()
    first = len(self._keep)
    if self.kind in _SINGLE_KINDS:
      d.kind = _SINGLE_KINDS[self.kind]
      d.dim = self.dim
      d.scale = self.scale
      d.nu = self.nu
      if self.bandwidths is None or self.bandwidths.size != self.dim:
        raise ValueError('Dimension of dim_bandwidths should be the same as dimension.')
      bw = _f64(self.bandwidths)
      self._keep.append(bw)
      d.bw = bw.ctypes.data_as(_lib.c_double_p)
      d.n_groups = 0
    elif self.kind in ('additive', 'product', 'esp'):
      d.kind = {'additive': KERNEL_ADDITIVE, 'product': KERNEL_PRODUCT, 'esp': KERNEL_ESP}[self.kind]
      d.dim = self.dim
      d.scale = self.scale
      d.nu = self.nu if self.kind == 'esp' else 0.0     # ESP: the order
      ng = len(self.groups)
      off = np.zeros(ng + 1, dtype=np.int32)
      off[1:] = np.cumsum([len(g) for g in self.groups])
      dims = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.int32).ravel()
                                                  for g in self.groups]), dtype=np.int32)
      kinds = np.ascontiguousarray([_SINGLE_KINDS[k] for k in self.sub_kinds], dtype=np.int32)
      scales = _f64(self.sub_scales)
      nus = _f64(self.sub_nus if self.sub_nus is not None else np.zeros(ng))
      bws = _f64(np.concatenate([_f64(np.ravel(b)) for b in self.sub_bandwidths]))
      if bws.size != dims.size:
        raise ValueError('Group bandwidths do not match the group dimensions.')
      self._keep += [off, dims, kinds, scales, nus, bws]
      d.n_groups = ng
      d.group_off = off.ctypes.data_as(_lib.c_int32_p)
      d.group_dims = dims.ctypes.data_as(_lib.c_int32_p)
      d.sub_kind = kinds.ctypes.data_as(_lib.c_int32_p)
      d.sub_scale = scales.ctypes.data_as(_lib.c_double_p)
      d.sub_nu = nus.ctypes.data_as(_lib.c_double_p)
      d.sub_bw = bws.ctypes.data_as(_lib.c_double_p)
      if self.group_factors is not None:
        if self.kind != 'product':
          raise ValueError('Additive factors exist in product kernels only.')
        gf = np.ascontiguousarray(self.group_factors, dtype=np.int32)
        fs = np.ascontiguousarray([int(s) for s in self.factor_sums], dtype=np.int32)     # 0 | 1 (True) | 2: a product factor
        fsc = _f64(self.factor_scales)
        if gf.size != ng or fs.size != fsc.size or (ng and int(gf.max()) >= fs.size):
          raise ValueError('group_factors / factor_sums / factor_scales do not fit the groups.')
        self._keep += [gf, fs, fsc]
        d.group_factor = gf.ctypes.data_as(_lib.c_int32_p)
        d.factor_is_sum = fs.ctypes.data_as(_lib.c_int32_p)
        d.factor_scale = fsc.ctypes.data_as(_lib.c_double_p)
    else:
      raise ValueError('Unidentified kernel type %s.' % (self.kind))
    d.backing = self._keep[first:]
    if first > 0:
      self._keep = self._keep[first:]       # older arrays live on with the descriptors that use them
    return d


class Engine(object):
  """ One MI355X: a dfh_ctx (stream + workspaces). """
  kernel_kinds = frozenset(_SINGLE_KINDS) | frozenset(['additive', 'product', 'esp'])     # what kernel_matrix / gp_fit describe

  def __init__(self, device=None):
    self.lib = _lib.load()
    self.ctx = None
    if device is None:
      device = int(os.environ.get('DFH_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    if _lib.device_count() == 0:
      raise _lib.DfhipError('No HIP device visible: dragonfly_amd needs an MI355X (gfx950); '
                            'there is no CPU fallback.')
    ctx = C.c_void_p()
    check(self.lib.dfh_ctx_create(int(device), C.byref(ctx)))
    self.ctx = ctx
    self.device = int(device)
    self._owns_ctx = True

  @classmethod
  def from_ctx(cls, ctx, device):
    """ A view of a context somebody else owns (parallel.MultiEngine's per-device contexts). """
    new = cls.__new__(cls)
    new.lib, new.ctx, new.device, new._owns_ctx = _lib.load(), ctx, int(device), False
    return new

  def close(self):
    if self.ctx is not None and getattr(self, '_owns_ctx', True):
      self.lib.dfh_ctx_destroy(self.ctx)
    self.ctx = None

  def __del__(self):
    try:
      self.close()
    except Exception:     # pylint: disable=broad-except
      pass

  # -- plumbing --------------------------------------------------------------------------
  def name(self):
    buf = C.create_string_buffer(256)
    check(self.lib.dfh_device_name(self.ctx, buf, 256))
    return buf.value.decode()

  def sync(self):
    check(self.lib.dfh_sync(self.ctx))

  def to_device(self, host):
    host = _f64(host)
    return DeviceArray(self, host.shape).upload(host)

  def empty(self, shape):
    return DeviceArray(self, shape)

  def join_fixed(self, z, cands):
    """ The joint candidates of a fixed fidelity (dfh_join_fixed_columns): row a of the result is [z, cands[a]], what
        mfgp.get_ZX_from_ZZ_XX([z] * m, cands) builds on the host (opt/gpb_acquisitions.py:314-332), written in HBM.
        cands: a DeviceArray [m x d] (a host array is uploaded first).  Returns a DeviceArray [m x (p + d)]. """
    z = _f64(np.ravel(z))
    if not isinstance(cands, DeviceArray):
      cands = self.to_device(np.atleast_2d(_f64(cands)))
    m, d = cands.shape
    out = DeviceArray(self, (max(m, 1), len(z) + d))
    out.shape, out.size = (m, len(z) + d), m * (len(z) + d)
    check(self.lib.dfh_join_fixed_columns(self.ctx, _ptr(z), len(z), _ptr(cands), m, d, _ptr(out)))
    return out

  def random_candidates(self, num, dim, bounds=None, rng=None, out=None, rows=None):
    """ `num` uniform points of the box `bounds` ([dim][2]; None = unit cube) generated in HBM:
        the draw np.random.random((num, dim)) mapped to the bounds (oper_utils.py:62,
        general_utils.py:25-27), bit for bit, from the state of `rng` -- None / the np.random module
        (the global legacy state the reference uses), a np.random.RandomState, or a
        np.random.Generator over a Philox bit generator.  The generator is advanced exactly as
        the host draw would have advanced it.  Returns a DeviceArray [num x dim] (or fills `out`,
        a DeviceArray or a host array).  rows=(begin, count) keeps only that slice of the rows (the
        result is [count x dim]) while the generator still advances over all `num` rows: the shard
        of one rank in a multi-GPU run. """
    num, dim = int(num), int(dim)
    if num < 0 or dim < 1:
      raise ValueError('random_candidates needs num >= 0 and dim >= 1.')
    if bounds is not None:
      bounds = _f64(bounds)
      if bounds.shape != (dim, 2):
        raise ValueError('bounds must have shape (dim, 2).')
    row_begin, row_count = (0, num) if rows is None else (int(rows[0]), int(rows[1]))
    if row_begin < 0 or row_count < 0 or row_begin + row_count > num:
      raise ValueError('rows must lie inside [0, num).')
    if out is None:
      out = DeviceArray(self, (max(row_count, 1), dim))
      out.shape, out.size = (row_count, dim), row_count * dim
    if rng is None or rng is np.random or isinstance(rng, np.random.RandomState):
      legacy = np.random if (rng is None or rng is np.random) else rng
      state = legacy.get_state()
      if state[0] != 'MT19937':
        raise ValueError('The legacy NumPy state is not MT19937.')
      key = np.ascontiguousarray(state[1], dtype=np.uint32).copy()
      pos = C.c_int32(int(state[2]))
      check(self.lib.dfh_rand_mt19937_uniform(self.ctx, _ptr(key), C.byref(pos), num, dim, row_begin,
                                              row_count, _ptr(bounds), _ptr(out)))
      legacy.set_state((state[0], key, int(pos.value)) + tuple(state[3:]))
      return out
    bit_gen = getattr(rng, 'bit_generator', rng)
    if not isinstance(bit_gen, np.random.Philox):
      raise ValueError('Device candidate generation follows MT19937 (np.random / RandomState) or '
                       'Philox (Generator(Philox(...))) streams; got %s.' % (type(bit_gen).__name__))
    state = bit_gen.state
    if state['has_uint32']:
      raise ValueError('The Philox generator holds half a word from a 32-bit draw.')
    key = np.ascontiguousarray(state['state']['key'], dtype=np.uint64).copy()
    counter = np.ascontiguousarray(state['state']['counter'], dtype=np.uint64).copy()
    held = np.ascontiguousarray(state['buffer'], dtype=np.uint64).copy()
    held_pos = C.c_int32(int(state['buffer_pos']))
    check(self.lib.dfh_rand_philox_uniform(self.ctx, _ptr(key), _ptr(counter), _ptr(held),
                                           C.byref(held_pos), num, dim, row_begin, row_count,
                                           _ptr(bounds), _ptr(out)))
    state['state']['counter'] = counter
    state['buffer'] = held
    state['buffer_pos'] = int(held_pos.value)
    bit_gen.state = state
    return out

  def random_normals(self, num, rng=None, out=None):
    """ np.random.normal(size=num) -- the standard normals of draw_gaussian_samples
        (general_utils.py:230) -- generated in HBM from the legacy MT19937 state of `rng` (None / the
        np.random module: the global state the reference uses; or a RandomState), bit for bit, the
        cached second gaussian included; the generator is advanced exactly as the host draw would
        have advanced it.  Returns a DeviceArray [num] (or fills `out`). """
    num = int(num)
    if num < 0:
      raise ValueError('random_normals needs num >= 0.')
    legacy = np.random if (rng is None or rng is np.random) else rng
    if not (legacy is np.random or isinstance(legacy, np.random.RandomState)):
      raise ValueError('Device normals follow the legacy MT19937 stream (np.random / RandomState).')
    if out is None:
      out = DeviceArray(self, (max(num, 1),))
      out.shape, out.size = (num,), num
    state = legacy.get_state()
    if state[0] != 'MT19937':
      raise ValueError('The legacy NumPy state is not MT19937.')
    key = np.ascontiguousarray(state[1], dtype=np.uint32).copy()
    pos, has_gauss, gauss = C.c_int32(int(state[2])), C.c_int32(int(state[3])), C.c_double(float(state[4]))
    check(self.lib.dfh_rand_mt19937_normal(self.ctx, _ptr(key), C.byref(pos), C.byref(has_gauss), C.byref(gauss),
                                           num, _ptr(out)))
    legacy.set_state((state[0], key, int(pos.value), int(has_gauss.value), float(gauss.value)))
    return out

  def mem_info(self):
    """ (free, total) HBM bytes of this engine's device. """
    f, t = C.c_uint64(0), C.c_uint64(0)
    check(self.lib.dfh_mem_info(self.ctx, C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)

  def timer_begin(self):
    check(self.lib.dfh_timer_begin(self.ctx))

  def timer_end(self):
    ms = C.c_double(0)
    check(self.lib.dfh_timer_end(self.ctx, C.byref(ms)))
    return ms.value

  def timings(self, enable=True):
    """ Returns the section timings (ms) accumulated since the last call and resets them. """
    arr = (C.c_double * 8)()
    check(self.lib.dfh_ctx_timings(self.ctx, 1 if enable else 0, arr))
    return dict(zip(_lib.T_NAMES, list(arr)))

  def counters(self):
    """ {'chol_fallbacks': factorisations repeated on the hand-off-free schedule, 'chol_cooldown': how many
        of the next ones skip the hand-off schedules, 'km_route': the route of the most recent kernel-matrix build
        (KM_ROUTES; None before the first), 'km_dispatches': how many such builds there were} (dfh_ctx_counters) """
    arr = (C.c_int64 * 4)()
    check(self.lib.dfh_ctx_counters(self.ctx, arr))
    return {'chol_fallbacks': int(arr[0]), 'chol_cooldown': int(arr[1]), 'km_route': KM_ROUTES[int(arr[2])],
            'km_dispatches': int(arr[3])}

  def gemm_profile(self, enable=True, fetch=True):
    """ Per-variant {launches, ms (sum of launch durations), flop, busy_ms (union of the launch
        intervals), bytes (algorithmic)} of the GEMM kernel since the last call (HIP events). """
    arr = (C.c_double * 40)()
    check(self.lib.dfh_ctx_gemm_profile(self.ctx, 1 if enable else 0, arr if fetch else None))
    return [dict(launches=int(arr[5 * v]), ms=arr[5 * v + 1], flop=arr[5 * v + 2], busy_ms=arr[5 * v + 3],
                 bytes=arr[5 * v + 4]) for v in range(8)]

  def gemm_solo_launches(self):
    """ Launches of the one-workgroup-per-CU form of the 128-tile NT GEMM kernel since the context was created. """
    out = C.c_int64(0)
    check(self.lib.dfh_ctx_gemm_solo_launches(self.ctx, C.byref(out)))
    return int(out.value)

  def solve_launches(self):
    """ What the triangular solves launched since the context was created (dfh_ctx_solve_launches), by SOLVE_COUNTERS'
        names: the four single-vector kernels with their update variants, the 512-blocks solved by the general
        single-vector route, the refinement steps run, and each instantiation of the few-row GEMM. """
    arr = (C.c_int64 * len(SOLVE_COUNTERS))()
    check(self.lib.dfh_ctx_solve_launches(self.ctx, arr))
    return {name: int(arr[i]) for i, name in enumerate(SOLVE_COUNTERS)}

  # -- building blocks ---------------------------------------------------------------------
  def kernel_matrix(self, spec, X1, X2=None, diag_add=0.0, out=None):
    X1h = X1 if isinstance(X1, DeviceArray) else _f64(X1)
    n1 = X1h.shape[0]
    if X2 is None:
      X2h, n2 = None, n1
    else:
      X2h = X2 if isinstance(X2, DeviceArray) else _f64(X2)
      n2 = X2h.shape[0]
    if out is None:
      out = np.zeros((n1, n2), dtype=np.float64)
    if n1 == 0 or n2 == 0:
      return out
    desc = spec.to_desc()
    check(self.lib.dfh_kernel_matrix(self.ctx, C.byref(desc), _ptr(X1h), n1, _ptr(X2h), n2,
                                     float(diag_add), _ptr(out)))
    return out

  def dist_squared(self, X1, X2):
    X1 = _f64(X1)
    X2 = _f64(X2)
    n1, d1 = X1.shape
    n2, d2 = X2.shape
    if d1 != d2:
      raise ValueError('Second dimension of X1 and X2 should be equal.')
    out = np.zeros((n1, n2), dtype=np.float64)
    if n1 == 0 or n2 == 0:
      return out
    check(self.lib.dfh_dist_squared(self.ctx, _ptr(X1), n1, _ptr(X2), n2, d1, _ptr(out)))
    return out

  def gemm(self, A, B, C_in=None, alpha=1.0, beta=0.0, transb=False, lower_only=False,
           shape=None, out=None):
    """ out = beta*C + alpha*A*op(B). Host arrays or (with shape=(M,N,K)) DeviceArrays. """
    if shape is None:
      A = _f64(A)
      B = _f64(B)
      M, K = A.shape
      N = B.shape[1] if transb else B.shape[0]
      if out is None:
        out = np.zeros((M, N)) if C_in is None else _f64(C_in).copy()
      lda, ldb, ldc = K, (N if transb else K), N
    else:
      M, N, K = shape
      lda, ldb, ldc = K, (N if transb else K), N
      assert out is not None
    check(self.lib.dfh_gemm(self.ctx, 1 if transb else 0, M, N, K, float(alpha), _ptr(A), lda,
                            _ptr(B), ldb, float(beta), _ptr(out), ldc, 1 if lower_only else 0))
    return out

  def cholesky(self, M):
    """ numpy.linalg.cholesky semantics (raises LinAlgError when not positive definite). """
    if isinstance(M, DeviceArray):
      n = M.shape[0]
      piv = C.c_int64(0)
      check(self.lib.dfh_cholesky(self.ctx, M.ptr, n, C.byref(piv)))
      return M
    L = _f64(M).copy()
    n = L.shape[0]
    piv = C.c_int64(0)
    check(self.lib.dfh_cholesky(self.ctx, _ptr(L), n, C.byref(piv)))
    return L

  def stable_cholesky(self, M, return_power=False):
    M = _f64(M)
    n = M.shape[0]
    L = np.empty_like(M)
    jp = C.c_int32(INT32_MIN)
    check(self.lib.dfh_stable_cholesky(self.ctx, _ptr(M), n, _ptr(L), C.byref(jp)))
    if return_power:
      return L, (None if jp.value == INT32_MIN else jp.value)
    return L

  def solve_triangular(self, L_lower, b, upper=False):
    """ Solves L x = b (upper=False) or L^T x = b (upper=True) for lower-triangular L. """
    L_lower = _f64(L_lower)
    b = _f64(b)
    n = L_lower.shape[0]
    nrhs = 1 if b.ndim == 1 else b.shape[1]
    x = np.empty_like(b)
    check(self.lib.dfh_solve_triangular(self.ctx, _ptr(L_lower), n, 1 if upper else 0, _ptr(b),
                                        nrhs, _ptr(x)))
    return x

  # -- multi-objective acquisitions --------------------------------------------------------
  @staticmethod
  def _mo_args(gps, scal, weights, refs, Xs, mean_consts, mean_vals):
    """ What dfh_mo_ucb_argmax and dfh_mo_ts_argmax share: the handle array, the scalarisation and its
        parameters, the candidates and the prior means (constants, or [k x m] values). """
    k = len(gps)
    handles = (C.c_void_p * max(k, 1))(*[gp.handle for gp in gps])
    if scal not in MO_SCALARISATIONS:
      raise ValueError('Unknown scalarisation %s (lin | tch).' % (scal))
    w = _f64(np.ravel(weights))
    r = None if refs is None else _f64(np.ravel(refs))
    if len(w) != k or (r is not None and len(r) != k):
      raise ValueError('Need one weight (and one reference value) per objective.')
    Xs, m = _rows(Xs)
    mv = _mean_vals_arg(mean_vals)
    if mv is not None and tuple(mv.shape) != (k, m):
      raise ValueError('mean_vals must have shape (objectives, candidates).')
    mc = _f64(np.zeros(k) if mean_consts is None else np.ravel(mean_consts))
    if len(mc) != k:
      raise ValueError('Need one mean constant per objective.')
    return handles, k, MO_SCALARISATIONS[scal], w, r, Xs, m, mc, mv

  def mo_ucb_argmax(self, gps, scal, beta, weights, refs, Xs, mean_consts=None, mean_vals=None, return_vals=False):
    """ The multi-objective UCB of K FittedGPs (opt/multiobjective_gpb_acquisitions.py:76-106) over the
        candidates Xs (host array or DeviceArray) and its arg-max in one device call.  scal 'lin' | 'tch';
        refs may be None for 'lin'.  Returns (best_val, best_idx[, vals]). """
    handles, k, scal_id, w, r, Xs, m, mc, mv = self._mo_args(gps, scal, weights, refs, Xs, mean_consts, mean_vals)
    vals = np.empty(m) if return_vals else None
    bv, bi = C.c_double(0), C.c_int64(-1)
    check(self.lib.dfh_mo_ucb_argmax(handles, k, scal_id, float(beta), _ptr(w), _ptr(r), _ptr(Xs), m, _ptr(mc), _ptr(mv),
                                     _ptr(vals), C.byref(bv), C.byref(bi)))
    return (bv.value, bi.value, vals) if return_vals else (bv.value, bi.value)

  def mo_thompson(self, gps, scal, weights, refs, Xs, U, block=4096, X_halluc=None, mean_consts=None, mean_vals=None,
                  return_vals=False):
    """ Multi-objective Thompson sampling (:19-67): objective i's blocked-joint draw from row i of the
        standard normals U [k x m] (host array or DeviceArray), with the points in progress X_halluc
        hallucinated into every objective's GP, scalarised, and the arg-max.  Returns (best_val, best_idx[,
        vals, jitter_powers [k][blocks]]). """
    handles, k, scal_id, w, r, Xs, m, mc, mv = self._mo_args(gps, scal, weights, refs, Xs, mean_consts, mean_vals)
    Uh = U if isinstance(U, DeviceArray) else _f64(np.ravel(U))
    if Uh.size != k * m:
      raise ValueError('U must hold one standard normal per objective and candidate.')
    block = int(min(block, m))
    nblk = (m + block - 1) // block
    Xh, q = _halluc_rows(X_halluc)
    vals = np.empty(m) if return_vals else None
    jps = (C.c_int32 * (k * nblk))()
    bv, bi = C.c_double(0), C.c_int64(-1)
    check(self.lib.dfh_mo_ts_argmax(handles, k, scal_id, _ptr(w), _ptr(r), _ptr(Xs), m, block, _ptr(Xh), q, _ptr(Uh),
                                    _ptr(mc), _ptr(mv), _ptr(vals), C.byref(bv), C.byref(bi), jps))
    if return_vals:
      powers = [[None if jps[i * nblk + b] == INT32_MIN else jps[i * nblk + b] for b in range(nblk)] for i in range(k)]
      return bv.value, bi.value, vals, powers
    return bv.value, bi.value

  def mo_thompson_pointwise(self, gps, scal, weights, refs, Xs, normals=None, X_halluc=None, mean_consts=None,
                            mean_vals=None, return_vals=False, return_samples=False):
    """ Point-wise multi-objective Thompson sampling (dfh_mo_ts_pointwise): per candidate and objective the one-point
        draw of FittedGP.thompson_pointwise, the K draws of a candidate scalarised, and the arg-max, in one device call
        -- what the reference's maximisers on Cartesian-product domains make of mo_lin_asy_ts / mo_tch_asy_ts.
        normals: the m * K standard normals [m x K], POINT-major (host array or DeviceArray; mo_thompson's U is
        objective-major); None: Engine.random_normals(m * K), which continues the global np.random stream exactly as
        m * K calls of np.random.normal(size=(1, 1)) do.  A variance that is not positive raises the ValueError of an
        exhausted jitter ladder.  Returns (best_val, best_idx[, vals][, samples [K x m]]). """
    handles, k, scal_id, w, r, Xs, m, mc, mv = self._mo_args(gps, scal, weights, refs, Xs, mean_consts, mean_vals)
    own = normals is None
    Uh = self.random_normals(m * k) if own else (normals if isinstance(normals, DeviceArray) else _f64(np.ravel(normals)))
    try:
      if Uh.size != m * k:
        raise ValueError('normals must hold one standard normal per candidate and objective.')
      Xh, q = _halluc_rows(X_halluc)
      vals = np.empty(m) if return_vals else None
      samples = np.empty((k, m)) if return_samples else None
      bv, bi = C.c_double(0), C.c_int64(-1)
      check(self.lib.dfh_mo_ts_pointwise(handles, k, scal_id, _ptr(w), _ptr(r), _ptr(Xs), m, _ptr(Xh), q, _ptr(Uh), _ptr(mc),
                                         _ptr(mv), _ptr(samples), _ptr(vals), C.byref(bv), C.byref(bi)))
    finally:
      if own:
        Uh.free()
    return (bv.value, bi.value) + ((vals,) if return_vals else ()) + ((samples,) if return_samples else ())

  # -- GP ----------------------------------------------------------------------------------
  def gp_lml_batch(self, specs, X, y, mean_consts, noise_vars, allow_jitter=True, return_powers=False,
                   handle_non_psd_kernels='guaranteed_psd'):
    """ Log marginal likelihoods of len(specs) hyper-parameter candidates on the same (X, y): the
        tuning objective of GPFitter (gp_core.py:551-564) for a list of candidates, fitted in
        lock-step groups on the device.  y holds raw labels; mean_consts[c] is subtracted.
        handle_non_psd_kernels other than 'guaranteed_psd': every candidate's Gram matrix takes that
        branch of _get_cholesky_decomp (gp_core.py:827-841), one candidate at a time. """
    nb = len(specs)
    Xh = X if isinstance(X, DeviceArray) else _f64(X)
    yh = y if isinstance(y, DeviceArray) else _f64(y)
    n, d = Xh.shape
    backing = []
    descs = _single_kind_descs(specs, d, backing)      # one vectorised fill when every candidate is a plain kernel
    if descs is None:
      descs = (_lib.KernelDesc * max(nb, 1))()
      for i, sp in enumerate(specs):
        one = sp.to_desc()
        backing.append(one.backing)       # the arrays the copied struct points at
        descs[i] = one
    mc = _f64(np.zeros(nb) if mean_consts is None else mean_consts).reshape(-1)
    nv = _f64(noise_vars).reshape(-1)
    if len(mc) != nb or len(nv) != nb:
      raise ValueError('gp_lml_batch: need one mean constant and one noise variance per candidate.')
    lml = np.empty(nb, dtype=np.float64)
    jps = np.empty(nb, dtype=np.int32)
    flags = (0 if allow_jitter else _lib.FIT_NO_JITTER) | _psd_flags(handle_non_psd_kernels)
    if isinstance(Xh, DeviceArray):
      flags |= _lib.LML_X_IS_DEVICE
    if not isinstance(yh, DeviceArray):
      flags |= _lib.LML_Y_IS_HOST
    check(self.lib.dfh_gp_lml_batch(self.ctx, descs, nb, _ptr(Xh), n, d, _ptr(yh), _ptr(mc), _ptr(nv),
                                    flags, _ptr(lml), _ptr(jps)))
    if return_powers:
      return lml, [None if p == INT32_MIN else int(p) for p in jps]
    return lml

  def gp_fit_gram(self, K, y_centred, noise_var, allow_jitter=True, handle_non_psd_kernels='guaranteed_psd'):
    """ Posterior from a Gram matrix the caller evaluated: a FittedGP without a kernel -- use
        predict_gram / predict_covar_gram with it.  handle_non_psd_kernels as in the reference's
        _get_cholesky_decomp (gp_core.py:827-847): 'guaranteed_psd' | 'project_first' |
        'try_before_project'. """
    return FittedGP.from_gram(self, K, y_centred, noise_var, allow_jitter, handle_non_psd_kernels)

  def project_psd(self, M, epsilon=0.0):
    """ project_symmetric_to_psd_cone (general_utils.py:150-163) on the device. """
    M = _f64(M)
    n = M.shape[0]
    if M.shape != (n, n):
      raise ValueError('project_psd: the matrix must be square.')
    out = np.empty_like(M)
    check(self.lib.dfh_project_psd(self.ctx, _ptr(M), n, float(epsilon), _ptr(out)))
    return out

  def gp_fit(self, spec, X, y_centred, noise_var, allow_jitter=True, handle_non_psd_kernels='guaranteed_psd'):
    """ Returns a FittedGP (posterior resident in HBM).  handle_non_psd_kernels as in gp_fit_gram: the Gram
        matrix is built on the device from the descriptor and projected there. """
    return FittedGP(self, spec, X, y_centred, noise_var, allow_jitter, handle_non_psd_kernels)


class FittedGP(object):
  """ Handle of a dfh_gp: K, L, alpha live on the device. """

  # Capability: joint draws with points in progress and several samples run as one device call (draw, and
  # thompson's X_halluc).  Callers choose the fused route by this attribute, never by the handle's type.
  fused_draws = True

  def __init__(self, engine, spec, X, y_centred, noise_var, allow_jitter=True, handle_non_psd_kernels='guaranteed_psd'):
    self.engine = engine
    self.handle = None
    self.spec = spec
    Xh = X if isinstance(X, DeviceArray) else _f64(X)
    yh = y_centred if isinstance(y_centred, DeviceArray) else _f64(y_centred)
    n, d = Xh.shape
    self.n, self.d = int(n), int(d)
    desc = spec.to_desc()
    h = C.c_void_p()
    lml = C.c_double(0)
    jp = C.c_int32(INT32_MIN)
    check(engine.lib.dfh_gp_fit(engine.ctx, C.byref(desc), _ptr(Xh), n, d, _ptr(yh),
                                float(noise_var),
                                (0 if allow_jitter else _lib.FIT_NO_JITTER) | _psd_flags(handle_non_psd_kernels),
                                C.byref(h), C.byref(lml), C.byref(jp)))
    self.handle = h
    self.lml = lml.value
    self.jitter_power = None if jp.value == INT32_MIN else jp.value

  @classmethod
  def from_gram(cls, engine, K, y_centred, noise_var, allow_jitter=True, handle_non_psd_kernels='guaranteed_psd'):
    Kh = K if isinstance(K, DeviceArray) else _f64(K)
    n = Kh.shape[0]
    if Kh.shape != (n, n):
      raise ValueError('from_gram: the Gram matrix must be square.')
    yh = _f64(y_centred).reshape(-1)
    if yh.shape[0] != n:
      raise ValueError('from_gram: need %d centred labels, got %d.' % (n, yh.shape[0]))
    h = C.c_void_p()
    lml = C.c_double(0)
    jp = C.c_int32(INT32_MIN)
    flags = (0 if allow_jitter else _lib.FIT_NO_JITTER) | _psd_flags(handle_non_psd_kernels)
    check(engine.lib.dfh_gp_fit_gram(engine.ctx, _ptr(Kh), n, _ptr(yh), float(noise_var), flags, C.byref(h),
                                     C.byref(lml), C.byref(jp)))
    new = cls.__new__(cls)
    new.engine, new.spec, new.handle = engine, None, h
    new.n, new.d = int(n), 0
    new.lml = lml.value
    new.jitter_power = None if jp.value == INT32_MIN else jp.value
    return new

  def predict_gram(self, K_cross, k_ss=None, mean_const=0.0, mean_vals=None):
    """ (mu, sd) from the caller's cross matrix K(X*, X) [m x n] and prior variances k(x*, x*) [m]
        (k_ss None: mean only). """
    Kc = _f64(K_cross)
    m = Kc.shape[0]
    if Kc.ndim != 2 or Kc.shape[1] != self.n:
      raise ValueError('predict_gram: the cross matrix must be m x %d.' % (self.n))
    mu = np.empty(m, dtype=np.float64)
    sd = np.empty(m, dtype=np.float64) if k_ss is not None else None
    ks = None if k_ss is None else _f64(k_ss).reshape(-1)
    mv = None if mean_vals is None else _f64(mean_vals).reshape(-1)
    check(self.engine.lib.dfh_gp_predict_gram(self.handle, _ptr(Kc), m, _ptr(ks), float(mean_const),
                                              _ptr(mv), _ptr(mu), _ptr(sd)))
    return mu, sd

  def predict_covar_gram(self, K_cross, K_tete):
    """ (K_cross alpha, K_tete - V^T V) for the caller's kernel matrices. """
    Kc, Kt = _f64(K_cross), _f64(K_tete)
    m = Kc.shape[0]
    if Kc.shape != (m, self.n) or Kt.shape != (m, m):
      raise ValueError('predict_covar_gram: need an m x %d cross matrix and an m x m test matrix.' % (self.n))
    mu = np.empty(m, dtype=np.float64)
    cov = np.empty((m, m), dtype=np.float64)
    check(self.engine.lib.dfh_gp_predict_covar_gram(self.handle, _ptr(Kc), m, _ptr(Kt), _ptr(mu), _ptr(cov)))
    return mu, cov

  def append(self, X_new, y_centred_all, allow_jitter=True):
    """ Posterior extended by the rows of X_new (dfh_gp_append): a NEW FittedGP, this one stays
        valid.  y_centred_all: all n+q centred labels, old observations first. """
    Xn = _f64(X_new)
    if Xn.ndim == 1:
      Xn = Xn.reshape(1, -1)
    q = Xn.shape[0]
    if Xn.shape[1] != self.d:
      raise ValueError('append: new points have %d columns, the GP has %d.' % (Xn.shape[1], self.d))
    yh = _f64(y_centred_all).reshape(-1)
    if yh.shape[0] != self.n + q:
      raise ValueError('append: need %d centred labels, got %d.' % (self.n + q, yh.shape[0]))
    h = C.c_void_p()
    lml = C.c_double(0)
    jp = C.c_int32(INT32_MIN)
    check(self.engine.lib.dfh_gp_append(self.handle, _ptr(Xn), q, _ptr(yh),
                                        0 if allow_jitter else _lib.FIT_NO_JITTER,
                                        C.byref(h), C.byref(lml), C.byref(jp)))
    new = FittedGP.__new__(FittedGP)
    new.engine, new.spec, new.handle = self.engine, self.spec, h
    new.n, new.d = self.n + q, self.d
    new.lml = lml.value
    new.jitter_power = None if jp.value == INT32_MIN else jp.value
    return new

  def free(self):
    if self.handle is not None:
      self.engine.lib.dfh_gp_free(self.handle)
      self.handle = None

  def __del__(self):
    try:
      self.free()
    except Exception:     # pylint: disable=broad-except
      pass

  def _get(self, what, shape):
    out = np.empty(shape, dtype=np.float64)
    check(self.engine.lib.dfh_gp_get(self.handle, what, _ptr(out)))
    return out

  def refine_steps(self):
    """ Iterative-refinement steps the triangular solves take per 512-block of the factor
        (all zero unless a diagonal block is ill-conditioned; dfh_gp_refine_steps). """
    nblk = (self.n + 511) // 512
    out = (C.c_int32 * nblk)()
    check(self.engine.lib.dfh_gp_refine_steps(self.handle, out))
    return list(out)

  def lml_grad(self):
    """ (grad, lml): the gradient of the log marginal likelihood in the tuner's coordinates -- [log scale,
        log bw_0 .. log bw_{d-1}, log noise_var, constant mean] -- and the value itself (dfh_gp_lml_grad).
        A single SE / Matern kernel (nu <= 2.5) fitted from its descriptor; anything else raises ValueError. """
    grad = np.empty(self.d + 3, dtype=np.float64)
    lml = C.c_double(0)
    check(self.engine.lib.dfh_gp_lml_grad(self.handle, _ptr(grad), C.byref(lml)))
    return grad, lml.value

  def lml_grad_layout(self):
    """ [(group, column)] of the bandwidth entries of lml_grad_groups, in order: the groups' columns as the
        descriptor lists them; group 0 and every column for a single kernel. """
    spec = self.spec
    if spec is None:
      raise ValueError('lml_grad_layout: a Gram-mode fit keeps no kernel.')
    if spec.groups is None:
      return [(0, c) for c in range(spec.dim)]
    return [(g, int(c)) for g, cols in enumerate(spec.groups) for c in cols]

  def lml_grad_groups(self):
    """ (grad, lml) as lml_grad, with one entry per bandwidth of every group (dfh_gp_lml_grad_groups):
        [log scale, the log bandwidths in lml_grad_layout's order, log noise_var, constant mean].  A single SE /
        Matern kernel, or an additive / product kernel of plain SE / Matern groups (nu <= 2.5); anything else
        raises ValueError. """
    nbw = self.d if self.spec is None else len(self.lml_grad_layout())
    grad = np.empty(nbw + 3, dtype=np.float64)
    lml = C.c_double(0)
    check(self.engine.lib.dfh_gp_lml_grad_groups(self.handle, _ptr(grad), grad.size, C.byref(lml)))
    return grad, lml.value

  def get_L(self):
    return self._get(GET_L, (self.n, self.n))

  def get_alpha(self):
    return self._get(GET_ALPHA, (self.n,))

  def get_K(self):
    return self._get(GET_K, (self.n, self.n))

  def predict(self, Xs, want_std=True, X_halluc=None):
    """ (K(Xs,X) alpha, posterior std) -- the caller adds the mean function. """
    Xs, m = _rows(Xs)
    mu = np.empty(m)
    sd = np.empty(m) if want_std else None
    Xh, q = _halluc_rows(X_halluc)
    check(self.engine.lib.dfh_gp_predict(self.handle, _ptr(Xs), m, _ptr(Xh), q, _ptr(mu), _ptr(sd)))
    return mu, sd

  def predict_covar(self, Xs, X_halluc=None):
    Xs, m = _rows(Xs)
    mu = np.empty(m)
    cov = np.empty((m, m))
    Xh, q = _halluc_rows(X_halluc)
    check(self.engine.lib.dfh_gp_predict_covar(self.handle, _ptr(Xs), m, _ptr(Xh), q, _ptr(mu),
                                               _ptr(cov)))
    return mu, cov

  def acq_argmax(self, acq, Xs, params=(0.0, 0.0), mean_const=0.0, mean_vals=None, X_halluc=None,
                 return_vals=False):
    """ Fused posterior + acquisition + arg-max. Returns (best_val, best_idx[, vals]). """
    Xs, m = _rows(Xs)
    p = (C.c_double * 2)(float(params[0]), float(params[1]) if len(params) > 1 else 0.0)
    vals = np.empty(m) if return_vals else None
    mv = _mean_vals_arg(mean_vals)
    Xh, q = _halluc_rows(X_halluc)
    bv = C.c_double(0)
    bi = C.c_int64(-1)
    check(self.engine.lib.dfh_gp_acq_argmax(self.handle, ACQ_IDS[acq], p, _ptr(Xs), m, _ptr(Xh), q,
                                            float(mean_const), _ptr(mv), _ptr(vals), C.byref(bv),
                                            C.byref(bi)))
    if return_vals:
      return bv.value, bi.value, vals
    return bv.value, bi.value

  def draw(self, Xs, U, num_samples=1, block=None, X_halluc=None, mean_const=0.0, mean_vals=None,
           return_samples=True):
    """ num_samples joint draws over the candidates Xs in one device call (dfh_gp_draw): with block None (one
        block) gp.draw_samples(num_samples, Xs), and with X_halluc
        gp.draw_samples_with_hallucinated_observations(num_samples, Xs, X_halluc).  U: the standard normals
        np.random.normal(size=(m, num_samples)), host array or DeviceArray.  Returns (samples [S x m] or
        None, best_vals [S], best_idx [S], jitter_powers [blocks]). """
    Xs, m = _rows(Xs)
    S = int(num_samples)
    Uh = U if isinstance(U, DeviceArray) else _f64(np.ravel(U))
    if Uh.size != m * S:
      raise ValueError('U must hold one standard normal per candidate and sample.')
    block = m if block is None else int(min(block, m))
    nblk = (m + block - 1) // block
    Xh, q = _halluc_rows(X_halluc)
    samples = np.empty((S, m)) if return_samples else None
    bvs = np.empty(max(S, 1), dtype=np.float64)
    bis = np.empty(max(S, 1), dtype=np.int64)
    jps = (C.c_int32 * nblk)()
    mv = _mean_vals_arg(mean_vals)
    check(self.engine.lib.dfh_gp_draw(self.handle, _ptr(Xs), m, block, _ptr(Xh), q, _ptr(Uh), S, float(mean_const),
                                      _ptr(mv), _ptr(samples), _ptr(bvs), _ptr(bis), jps))
    return samples, bvs, bis, [None if j == INT32_MIN else j for j in jps]

  def thompson(self, Xs, U, block=4096, mean_const=0.0, mean_vals=None, return_samples=False, X_halluc=None):
    """ Blocked-joint Thompson sample over the candidates. Returns (best_val, best_idx[, samples,
        jitter_powers]).  X_halluc: the points in progress, hallucinated into the covariance (dfh_gp_draw). """
    if X_halluc is not None and len(X_halluc) > 0:
      samples, bvs, bis, powers = self.draw(Xs, U, 1, block, X_halluc, mean_const, mean_vals, return_samples)
      if return_samples:
        return float(bvs[0]), int(bis[0]), samples[0], powers
      return float(bvs[0]), int(bis[0])
    Xs, m = _rows(Xs)
    Uh = U if isinstance(U, DeviceArray) else _f64(np.ravel(U))
    block = int(min(block, m))
    nblk = (m + block - 1) // block
    samples = np.empty(m) if return_samples else None
    jps = (C.c_int32 * nblk)()
    mv = _mean_vals_arg(mean_vals)
    bv = C.c_double(0)
    bi = C.c_int64(-1)
    check(self.engine.lib.dfh_gp_ts(self.handle, _ptr(Xs), m, block, _ptr(Uh), float(mean_const),
                                    _ptr(mv), _ptr(samples), C.byref(bv), C.byref(bi), jps))
    if return_samples:
      return bv.value, bi.value, samples, [None if j == INT32_MIN else j for j in jps]
    return bv.value, bi.value

  def thompson_pointwise(self, Xs, normals=None, X_halluc=None, mean_const=0.0, mean_vals=None, return_samples=False):
    """ Point-wise Thompson sampling (dfh_gp_ts_pointwise): per candidate the one-point draw gp.draw_samples(1, [x]) --
        with X_halluc gp.draw_samples_with_hallucinated_observations(1, [x], X_halluc) -- what the reference's
        maximisers on Cartesian-product domains make of a sampler, in one device call.  normals: the m standard
        normals (host array or DeviceArray); None: Engine.random_normals(m), which continues the global np.random
        stream exactly as m calls of np.random.normal(size=(1, 1)) do.  A candidate whose variance is not positive
        raises the ValueError of an exhausted jitter ladder.  Returns (best_val, best_idx[, samples]). """
    Xs, m = _rows(Xs)
    own = normals is None
    Uh = self.engine.random_normals(m) if own else (normals if isinstance(normals, DeviceArray) else _f64(np.ravel(normals)))
    if Uh.size != m:
      raise ValueError('normals must hold one standard normal per candidate.')
    samples = np.empty(m) if return_samples else None
    mv = _mean_vals_arg(mean_vals)
    Xh, q = _halluc_rows(X_halluc)
    bv = C.c_double(0)
    bi = C.c_int64(-1)
    try:
      check(self.engine.lib.dfh_gp_ts_pointwise(self.handle, _ptr(Xs), m, _ptr(Xh), q, _ptr(Uh), float(mean_const),
                                                _ptr(mv), _ptr(samples), C.byref(bv), C.byref(bi)))
    finally:
      if own:
        Uh.free()
    if return_samples:
      return bv.value, bi.value, samples
    return bv.value, bi.value

  def add_ucb_group(self, group, beta, Xg, return_vals=False):
    Xg, m = _rows(Xg)
    vals = np.empty(m) if return_vals else None
    bv = C.c_double(0)
    bi = C.c_int64(-1)
    check(self.engine.lib.dfh_gp_add_ucb_group(self.handle, int(group), float(beta), _ptr(Xg), m,
                                               _ptr(vals), C.byref(bv), C.byref(bi)))
    if return_vals:
      return bv.value, bi.value, vals
    return bv.value, bi.value

  def add_ucb_all(self, betas, cands_per_group, return_vals=False, sizes=None):
    """ add-UCB for every group of the additive kernel in one device call (one posterior solve for
        all groups).  cands_per_group[g]: [m_g x |group g|] -- or ONE DeviceArray holding the groups'
        candidate blocks back to back, with sizes[g] = m_g.  Returns (best_vals, best_idx[, vals]). """
    flat, ms, be = _group_blocks(cands_per_group, sizes, betas, 'add_ucb_all')
    G = len(ms)
    bv = np.empty(G, dtype=np.float64)
    bi = np.empty(G, dtype=np.int64)
    vals = np.empty(int(ms.sum()), dtype=np.float64) if return_vals else None
    check(self.engine.lib.dfh_gp_add_ucb_all(self.handle, _ptr(be), _ptr(flat), _ptr(ms), _ptr(vals),
                                             _ptr(bv), _ptr(bi)))
    if return_vals:
      return bv, bi, np.split(vals, np.cumsum(ms)[:-1])
    return bv, bi

  def mf_add_ucb_group(self, z_opt, group, beta, Xg, return_vals=False):
    """ add_ucb_group for a multi-fidelity GP with an additive domain model at the fidelity z_opt
        (dfh_mf_add_ucb_group; _mf_add_ucb_acq_j, opt/gpb_acquisitions.py:360-374).  `group` counts the groups of
        the domain kernel, Xg holds that group's columns. """
    z = _f64(np.ravel(z_opt))
    Xg, m = _rows(Xg)
    vals = np.empty(m) if return_vals else None
    bv = C.c_double(0)
    bi = C.c_int64(-1)
    check(self.engine.lib.dfh_mf_add_ucb_group(self.handle, _ptr(z), int(group), float(beta), _ptr(Xg), m,
                                               _ptr(vals), C.byref(bv), C.byref(bi)))
    if return_vals:
      return bv.value, bi.value, vals
    return bv.value, bi.value

  def mf_add_ucb_all(self, z_opt, betas, cands_per_group, return_vals=False, sizes=None):
    """ add_ucb_all for a multi-fidelity GP with an additive domain model at the fidelity z_opt
        (dfh_mf_add_ucb_all): every group of the domain kernel in one device call, one posterior solve.
        Arguments and results as add_ucb_all. """
    z = _f64(np.ravel(z_opt))
    flat, ms, be = _group_blocks(cands_per_group, sizes, betas, 'mf_add_ucb_all')
    G = len(ms)
    bv = np.empty(G, dtype=np.float64)
    bi = np.empty(G, dtype=np.int64)
    vals = np.empty(int(ms.sum()), dtype=np.float64) if return_vals else None
    check(self.engine.lib.dfh_mf_add_ucb_all(self.handle, _ptr(z), _ptr(be), _ptr(flat), _ptr(ms), _ptr(vals),
                                             _ptr(bv), _ptr(bi)))
    if return_vals:
      return bv, bi, np.split(vals, np.cumsum(ms)[:-1])
    return bv, bi


_default_engine = None


def get_engine():
  """ The process-wide engine (one process per GPU; device = LOCAL_RANK / DFH_DEVICE). """
  global _default_engine
  if _default_engine is None:
    _default_engine = Engine()
  return _default_engine
