"""CPU: dfh_mgpu_lml_batch and dfh_lml_shard_plan in the C-ABI -- exported, bound with the documented argument types,
and the two outcomes that need no device: nb == 0 is DFH_OK whatever else is passed, a NULL engine is a bad argument."""
import ctypes as C
import re

import numpy as np

from dragonfly_amd import _lib
from test_abi import HEADER


def test_symbols_are_bound_with_the_documented_argument_types():
  lib = _lib.load()
  restype, argtypes = _lib.SIGNATURES['dfh_mgpu_lml_batch']
  assert restype is C.c_int and lib.dfh_mgpu_lml_batch.argtypes == argtypes
  # mg, descs, nb, X[], n, d, y[], mean_consts, noise_vars, flags, lml_out, jitter_powers, shard_lo
  assert argtypes == [C.c_void_p, C.POINTER(_lib.KernelDesc), C.c_int32, C.POINTER(C.c_void_p), C.c_int64, C.c_int64,
                      C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, _lib.c_int64_p]
  assert _lib.SIGNATURES['dfh_lml_shard_plan'] == (C.c_int, [C.c_int32, C.c_int64, C.c_int, C.c_int, _lib.c_int64_p])
  # the parameter list of the header's declaration, type by type
  text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
  decl = re.search(r'int\s+dfh_mgpu_lml_batch\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
  params = [' '.join(p.split()) for p in decl.split(',')]
  assert [p.rsplit(' ', 1)[0].replace(' *', '*') for p in params] == [
    'dfh_mgpu*', 'const dfh_kernel_desc*', 'int32_t', 'const double* const*', 'int64_t', 'int64_t', 'const double* const*',
    'const double*', 'const double*', 'int', 'double*', 'int32_t*', 'int64_t*']


def test_flag_and_fill_constants_are_the_headers():
  text = open(HEADER).read()
  defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r'^#define\s+(DFH_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|\d+)\b', text, flags=re.M)}
  assert defs['DFH_MGPU_LML_SPREAD'] == _lib.MGPU_LML_SPREAD and defs['DFH_MGPU_LML_FILL'] == _lib.MGPU_LML_FILL == 256
  others = (_lib.FIT_NO_JITTER | _lib.FIT_PROJECT_FIRST | _lib.FIT_TRY_BEFORE_PROJECT | _lib.LML_X_IS_DEVICE | _lib.LML_Y_IS_HOST)
  assert _lib.MGPU_LML_SPREAD & others == 0
  assert defs['DFH_ABI_VERSION'] == 2 and _lib.load().dfh_abi_version() == 2          # no struct changed


def test_empty_batch_and_null_engine_need_no_device():
  lib = _lib.load()
  lml = np.full(3, 7.0)
  cut = np.full(4, -5, dtype=np.int64)
  # nb == 0: DFH_OK, nothing is looked at and nothing written
  assert lib.dfh_mgpu_lml_batch(None, None, 0, None, 10, 2, None, None, None, 0, lml.ctypes.data, None,
                                cut.ctypes.data_as(_lib.c_int64_p)) == _lib.DFH_OK
  assert np.all(lml == 7.0) and np.all(cut == -5)
  # a NULL engine, a negative count: rejected before anything starts
  descs = (_lib.KernelDesc * 1)()
  ptrs = (C.c_void_p * 1)(lml.ctypes.data)
  nv = np.ones(1)
  assert lib.dfh_mgpu_lml_batch(None, descs, 1, ptrs, 3, 1, ptrs, None, nv.ctypes.data, 0, lml.ctypes.data, None,
                                None) == _lib.DFH_ERR_BAD_ARG
  assert 'bad argument' in _lib.last_error()
  assert lib.dfh_mgpu_lml_batch(None, descs, -1, ptrs, 3, 1, ptrs, None, nv.ctypes.data, 0, lml.ctypes.data, None,
                                None) == _lib.DFH_ERR_BAD_ARG
  assert np.all(lml == 7.0)
