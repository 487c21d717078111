"""ctypes binding of libhgx.so (include/hgx.h) -- the only way the package
reaches the GPU. There is no CPU fallback: if the library or a HIP device is
missing, every entry point raises.
"""

import ctypes
import os
import re
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libhgx.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "hgx.h")

HGX_OK, HGX_EINVAL, HGX_EHIP, HGX_ENOMEM = 0, -1, -2, -3
HGX_EZERODIV, HGX_ESTATE, HGX_EUNSUP, HGX_EVALUE = -4, -5, -6, -7
HGX_ENUMERIC = -8
LOSS_KLD, LOSS_MSE = 0, 1
ACT_SIGMOID, ACT_RELU = 0, 1
HOBE_NN, HOBE_EE, HOBE_NE = 0, 1, 2
WEIGHT_UNIFORM, WEIGHT_NEIGHBORHOOD, WEIGHT_DISTANCE = 0, 1, 2
NORM_L2, NORM_INF = 0, 1
MLP_LP_CLASSIFIER, MLP_NE_SUPERVISED, MLP_NE_SEMI_SUPERVISED = 0, 1, 2
STORE_FOBE, STORE_HOBE = 0, 1
STORE_BINS = 16384

_lib = None

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64
_int = ctypes.c_int
_f32 = ctypes.c_float
_pi64 = ctypes.POINTER(ctypes.c_int64)
_pint = ctypes.POINTER(ctypes.c_int)
_pdbl = ctypes.POINTER(ctypes.c_double)

# name -> (restype, argtypes); mirrors include/hgx.h one to one.
SIGNATURES = {
    "hgx_create": (_int, [_int, ctypes.POINTER(_vp)]),
    "hgx_destroy": (_int, [_vp]),
    "hgx_last_error": (ctypes.c_char_p, [_vp]),
    "hgx_version": (_int, []),
    "hgx_set_stream": (_int, [_vp, _vp]),
    "hgx_synchronize": (_int, [_vp]),
    "hgx_device_count": (_int, [_pint]),
    "hgx_mem_info": (_int, [_vp, _pi64, _pi64]),
    "hgx_set_tuning": (_int, [_vp, ctypes.c_char_p, _i64]),
    "hgx_upload_incidence": (_int, [_vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp]),
    "hgx_alg_dist": (_int, [_vp, _int, _int, _vp, _vp]),
    "hgx_alg_set": (_int, [_vp, _int, _vp, _vp]),
    "hgx_alg_run": (_int, [_vp, _int]),
    "hgx_alg_get": (_int, [_vp, _vp, _vp]),
    "hgx_alg_last_stats": (_int, [_vp, _pdbl, _pdbl]),
    "hgx_alg_shard_begin": (_int, [_vp, _i32, _i32, _vp, _vp, _int, _pint]),
    "hgx_alg_shard_node": (_int, [_vp, _int]),
    "hgx_alg_shard_edge_partial": (_int, [_vp, _int]),
    "hgx_alg_shard_edge_final": (_int, [_vp, _int]),
    "hgx_alg_shard_end": (_int, [_vp]),
    "hgx_alg_shard_wire": (_int, [_vp, _vp, _i64, _vp]),
    "hgx_alg_shard_ranges": (_int, [_vp, _int, _vp]),
    "hgx_alg_shard_edge_partial_range": (_int, [_vp, _int, _int]),
    "hgx_hobe_probs": (_int, [_vp, _int, _i64, _vp, _vp, _vp]),
    "hgx_incidence_weights": (_int, [_vp, _int, ctypes.c_double, _vp, _vp]),
    "hgx_weight_distance": (_int, [_vp, _int, ctypes.c_double, _vp, _vp]),
    "hgx_weight_same_type": (_int, [_vp, _int, _int, ctypes.c_double, _pi64,
                                    _vp, _vp, _vp]),
    "hgx_weight_span": (_int, [_vp, ctypes.c_double, _vp, _vp, _vp, _vp]),
    "hgx_sample_fobe": (_int, [_vp, _u64, _int, _vp, _vp, _vp, _vp, _pi64]),
    "hgx_sample_hobe": (_int, [_vp, _u64, _int, _int, _pi64]),
    "hgx_sample_hobe_rows": (_int, [_vp, _u64, _int, _vp, _vp, _int, _pi64]),
    "hgx_sample_fobe_mt": (_int, [_vp, _vp, _pint, _int, _vp, _vp, _vp, _vp,
                                  _pi64]),
    "hgx_sample_hobe_mt": (_int, [_vp, _vp, _pint, _int, _int, _pi64]),
    "hgx_sample_jaccard_mt": (_int, [_vp, _vp, _pint, _int, _vp, _vp, _pi64]),
    "hgx_sample_last_stats": (_int, [_vp, _pi64, _pi64]),
    "hgx_sample_uniform_rows": (_int, [_vp, _pi64]),
    "hgx_features_set": (_int, [_vp, _vp, _vp]),
    "hgx_sample_jaccard": (_int, [_vp, _u64, _int, _vp, _vp, _pi64]),
    "hgx_jaccard_probs": (_int, [_vp, _int, _i64, _vp, _vp, _vp]),
    "hgx_jaccard_centroids": (_int, [_vp, _int, _pi64, _vp, _vp, _vp]),
    "hgx_records_set": (_int, [_vp, _i64, _int, _vp, _vp]),
    "hgx_records_info": (_int, [_vp, _pi64, _pint]),
    "hgx_records_copy": (_int, [_vp, _vp]),
    "hgx_records_get": (_int, [_vp, _vp, _vp]),
    "hgx_records_blocks": (_int, [_vp, _pint, _vp]),
    "hgx_records_export": (_int, [_vp, _vp, _vp]),
    "hgx_records_import": (_int, [_vp, _i64, _int, _vp, _vp, _int, _vp]),
    "hgx_store_reset": (_int, [_vp, _i64]),
    "hgx_store_append": (_int, [_vp]),
    "hgx_store_info": (_int, [_vp, _pi64, _pint, _pint,
                              ctypes.POINTER(ctypes.c_uint64)]),
    "hgx_store_read": (_int, [_vp, _i64, _i64, _vp, _int]),
    "hgx_store_write": (_int, [_vp, _i64, _vp, _int, _int, _int, _u64]),
    "hgx_store_plan": (_int, [_vp, _u64, _i64, _pint, _vp, _vp]),
    "hgx_store_load": (_int, [_vp, _u64, _i32, _i32, _int, _int, _pi64]),
    "hgx_store_release": (_int, [_vp]),
    "hgx_model_init": (_int, [_vp, _int, _i64, _i64, _u64, _vp, _vp]),
    "hgx_model_get": (_int, [_vp, _vp, _vp]),
    "hgx_model_get_rows": (_int, [_vp, _int, _i64, _vp, _vp]),
    "hgx_probe_gather": (_int, [_vp, _i64, _int, _int, _int, _pdbl]),
    "hgx_train": (_int, [_vp, _int, _int, _f32, _f32, _int, _int, _f32, _u64,
                         _vp, _vp, _pint]),
    "hgx_train_last_stats": (_int, [_vp, _pdbl, _pi64, _pi64]),
    "hgx_train_path_stats": (_int, [_vp, _pi64, _pi64]),
    "hgx_train_multi_pending": (_int, [_vp, _pi64]),
    "hgx_train_step_geometry": (_int, [_vp, _pint, _pint]),
    "hgx_train_last_loss": (_int, [_vp, _pdbl]),
    "hgx_synth_powerlaw": (_int, [_i32, _i32, ctypes.c_double, ctypes.c_double,
                                  _u64, _vp, _vp, _pi64,
                                  ctypes.POINTER(ctypes.c_int32)]),
    "hgx_csr_transpose": (_int, [_i32, _i32, _vp, _vp, _vp, _vp]),
    "hgx_proto_parse_hypergraph": (_int, [_vp, _i64, ctypes.POINTER(_vp),
                                          ctypes.POINTER(_i32),
                                          ctypes.POINTER(_i32), _pi64]),
    "hgx_proto_hypergraph_fill": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hgx_proto_hypergraph_free": (None, [_vp]),
    "hgx_proto_write_embedding": (_int, [_i64, _vp, _vp, _i64, _vp, _vp, _int,
                                         ctypes.c_char_p, _vp, _i64, _pi64]),
    "hgx_host_last_error": (ctypes.c_char_p, []),
    "hgx_proto_parse_embedding": (_int, [_vp, _i64, ctypes.POINTER(_vp), _pi64,
                                         _pi64, _pi64,
                                         ctypes.POINTER(_i32)]),
    "hgx_proto_embedding_fill": (_int, [_vp, _vp, _vp, _vp, _vp,
                                        ctypes.c_char_p, _i64]),
    "hgx_proto_embedding_method_len": (_i64, [_vp]),
    "hgx_proto_embedding_free": (None, [_vp]),
    "hgx_proto_write_hypergraph": (_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _i64, _pi64]),
    "hgx_mlp_create": (_int, [_vp, _int, _int, _int, ctypes.POINTER(_vp)]),
    "hgx_mlp_destroy": (_int, [_vp]),
    "hgx_mlp_layers": (_int, [_vp, _pint, _vp]),
    "hgx_mlp_set_weights": (_int, [_vp, _vp]),
    "hgx_mlp_get_weights": (_int, [_vp, _vp]),
    "hgx_mlp_set_tables": (_int, [_vp, _i64, _vp, _i64, _vp]),
    "hgx_mlp_set_samples": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "hgx_mlp_fit": (_int, [_vp, _int, _int, _f32, _f32, _f32, _u64, _vp, _vp,
                           _pint]),
    "hgx_mlp_predict": (_int, [_vp, _int, _i64, _vp, _vp, _vp]),
    "hgx_mlp_last_stats": (_int, [_vp, _pdbl, _pi64, _pi64, _pdbl]),
    "hgx_svc_create": (_int, [_vp, _int, _i64, _vp, ctypes.POINTER(_vp)]),
    "hgx_svc_destroy": (_int, [_vp]),
    "hgx_svc_fit": (_int, [_vp, _i64, _vp, _vp, _vp, _f32, _f32, _f32, _int,
                           _vp, _vp]),
    "hgx_svc_decision": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "hgx_svc_decision_vec": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "hgx_svc_get": (_int, [_vp, _vp, _vp]),
    "hgx_svc_last_stats": (_int, [_vp, _pdbl, _pdbl]),
    "hgx_svd_create": (_int, [_vp, _int, ctypes.POINTER(_vp)]),
    "hgx_svd_destroy": (_int, [_vp]),
    "hgx_svd_panel": (_int, [_vp, _int, _int, _int]),
    "hgx_svd_set": (_int, [_vp, _int, _int, _int, _vp]),
    "hgx_svd_get": (_int, [_vp, _int, _int, _int, _vp]),
    "hgx_svd_copy": (_int, [_vp, _int, _int, _int, _int, _int]),
    "hgx_svd_spmm": (_int, [_vp, _int, _int, _int, _int, _int]),
    "hgx_svd_gram": (_int, [_vp, _int, _int, _int, _int, _int, _int, _vp]),
    "hgx_svd_apply": (_int, [_vp, _int, _int, _int, _int, _int, _int, _vp,
                             ctypes.c_double]),
    "hgx_svd_scale": (_int, [_vp, _int, _int, _int, _vp]),
    "hgx_svd_last_stats": (_int, [_vp, _pdbl, _pdbl, _pi64, _pi64, _pi64]),
    "hgx_svd_cd_sweep": (_int, [_vp, _int, _int, _int, _int, _int, _vp, _pdbl]),
    "hgx_svd_cd_sweep_fused": (_int, [_vp, _int, _int, _int, _int, _int, _vp,
                                      _pdbl]),
    "hgx_svd_cd_last_stats": (_int, [_vp, _pdbl, _pi64]),
    "hgx_ae_create": (_int, [_vp, _int, _int, ctypes.POINTER(_vp)]),
    "hgx_ae_destroy": (_int, [_vp]),
    "hgx_ae_set_weights": (_int, [_vp, _vp]),
    "hgx_ae_get_weights": (_int, [_vp, _vp]),
    "hgx_ae_draw": (_int, [_vp, _i64, _vp, _int, _u64, _int, _pi64, _vp, _vp]),
    "hgx_ae_step": (_int, [_vp, _i64, _vp, _vp, _f32, _f32,
                           ctypes.POINTER(_f32)]),
    "hgx_ae_fit": (_int, [_vp, _int, _int, _int, _f32, _f32, _u64, _vp, _vp,
                          _pint]),
    "hgx_ae_encode": (_int, [_vp, _i64, _vp, _vp]),
    "hgx_ae_last_stats": (_int, [_vp, _pdbl, _pi64, _pi64, _pdbl]),
    "hgx_n2v_create": (_int, [_vp, _int, _int, ctypes.POINTER(_vp)]),
    "hgx_n2v_destroy": (_int, [_vp]),
    "hgx_n2v_walks": (_int, [_vp, _i64, _vp, _vp, _int, ctypes.c_double, _u64,
                             _vp]),
    "hgx_n2v_counts": (_int, [_vp, _vp]),
    "hgx_n2v_set_vocab": (_int, [_vp, _vp, _vp]),
    "hgx_n2v_set_vectors": (_int, [_vp, _vp, _vp]),
    "hgx_n2v_get_vectors": (_int, [_vp, _vp, _vp]),
    "hgx_n2v_train": (_int, [_vp, _i64, _int, _vp, _int, _int, _int, _f32,
                             _f32, _u64, _int]),
    "hgx_n2v_last_stats": (_int, [_vp, _pdbl, _pdbl, _pi64, _pi64, _pi64,
                                  _pi64, _pi64]),
    "hgx_n2v_set_tree": (_int, [_vp, _vp, _vp, _vp]),
    "hgx_n2v_train_hs": (_int, [_vp, _i64, _int, _vp, _int, _int, _f32, _f32,
                                _u64, _int]),
    "hgx_n2v_last_hs_stats": (_int, [_vp, _pi64]),
    "hgx_n2v_set_arcs": (_int, [_vp, _vp, _vp, _vp]),
    "hgx_n2v_line_samples": (_int, [_vp, _i64, _i64, _int, _u64, _vp]),
    "hgx_n2v_train_line": (_int, [_vp, _int, _int, _i64, _f32, _u64, _int]),
    "hgx_n2v_last_line_stats": (_int, [_vp, _pi64, _pi64, _pi64]),
    "hgx_n2v_mp_walks": (_int, [_vp, _i64, _vp, _int, _int, _u64, _i64, _i64,
                                _vp]),
    "hgx_n2v_mp_counts": (_int, [_vp, _i64, _vp, _int, _int, _u64, _vp]),
    "hgx_n2v_set_vocab_typed": (_int, [_vp, _vp, _vp, _int]),
    "hgx_n2v_train_mp": (_int, [_vp, _i64, _vp, _int, _int, _int, _int, _int,
                                _f32, _f32, _u64, _u64, _int]),
    "hgx_n2v_last_mp_stats": (_int, [_vp, _pi64, _pi64, _pi64, _pi64, _pi64]),
    "hgx_pyrandom_sample_missing": (_int, [_vp, _i32, _i32, _vp, _vp, _i64,
                                           _vp, _vp, _pi64]),
    "hgx_pyrandom_remove_connections": (_int, [_vp, _i64, _vp, _vp, _vp, _vp,
                                               ctypes.c_double, _vp, _pi64]),
    "hgx_lp_last_error": (ctypes.c_char_p, []),
}


def header_symbols():
  """Function names declared in include/hgx.h."""
  with open(HEADER) as f:
    text = f.read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  return sorted(set(re.findall(r"\b(hgx_[a-z0-9_]+)\s*\(", text)))


def lib():
  """Load libhgx.so (raises if it was not built)."""
  global _lib
  if _lib is None:
    # HGX_LIB_PATH: load another build of the same ABI (A/B timing)
    path = os.environ.get("HGX_LIB_PATH") or LIB_PATH
    if not os.path.exists(path):
      raise ImportError(
          f"{path} missing: run hypergraphembedding_amd.build.build() "
          "(there is no CPU fallback)")
    L = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
      fn = getattr(L, name)
      fn.restype = res
      fn.argtypes = args
    _lib = L
  return _lib


class HgxError(RuntimeError):
  pass


def _raise(rc, msg):
  if rc == HGX_EINVAL:
    raise AssertionError(msg)
  if rc == HGX_EZERODIV:
    raise ZeroDivisionError(msg)
  if rc == HGX_EVALUE:
    raise ValueError(msg)
  if rc == HGX_ENUMERIC:
    raise FloatingPointError(msg)
  raise HgxError(f"libhgx error {rc}: {msg}")


def _ptr(a):
  return None if a is None else a.ctypes.data


def _c(a, dtype):
  return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def device_count():
  """HIP devices visible to libhgx (hipGetDeviceCount)."""
  n = ctypes.c_int()
  lib().hgx_device_count(ctypes.byref(n))
  return n.value


class Context:
  """One device context (owns device memory and one HIP stream)."""

  def __init__(self, device=0):
    h = _vp()
    rc = lib().hgx_create(device, ctypes.byref(h))
    if rc != HGX_OK:
      _raise(rc, f"hgx_create(device={device}) failed: no usable HIP device")
    self.h = h
    self.device = device
    self._engines = weakref.WeakSet()  # Mlp engines living on this context

  def close(self):
    if getattr(self, "h", None):
      for e in list(getattr(self, "_engines", ())):
        e.close()
      lib().hgx_destroy(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def _chk(self, rc):
    if rc != HGX_OK:
      _raise(rc, lib().hgx_last_error(self.h).decode(errors="replace"))

  # ---- plumbing ----
  def set_stream(self, stream_ptr):
    self._chk(lib().hgx_set_stream(self.h, stream_ptr))

  def synchronize(self):
    self._chk(lib().hgx_synchronize(self.h))

  def mem_info(self):
    """(free, total) bytes of the context's device (hipMemGetInfo)."""
    f, t = ctypes.c_int64(), ctypes.c_int64()
    self._chk(lib().hgx_mem_info(self.h, ctypes.byref(f), ctypes.byref(t)))
    return f.value, t.value

  def set_tuning(self, key, value):
    """Pick between exact implementations (hgx_set_tuning): sample_reject_w,
    sample_mode3, sample_mode3_shift, sample_mode3_shift_e, train_fused,
    train_lanes, train_tb, train_wave_pair (1 one record on two waves, 3 on
    four waves with 2 records per workgroup where padded d = 128, 4 on four
    waves with 1 record per workgroup there, 0 off, -1 per geometry),
    train_prep_overlap, train_prep_cus, alg_long, alg_ks,
    alg_push, mlp_fuse_head, mlp_prefetch, mlp_wgrad_split, svc_lds_m,
    ae_chunk_rows, n2v_expand_w, n2v_chunk_walks, dw_hot_levels,
    line_chunk_samples, mp_chunk_walks, stream_cus."""
    self._chk(lib().hgx_set_tuning(self.h, key.encode(), int(value)))

  # ---- incidence ----
  def upload(self, inc):
    self.inc = inc
    self._keep = (_c(inc.rp_n, np.int32), _c(inc.col_n, np.int32),
                  _c(inc.rp_e, np.int32), _c(inc.col_e, np.int32))
    a, b, c, d = self._keep
    self._chk(lib().hgx_upload_incidence(self.h, inc.N, inc.E, inc.nnz,
                                         _ptr(a), _ptr(b), _ptr(c), _ptr(d)))

  # ---- algebraic distance ----
  def alg_set(self, x, y):
    x = _c(x, np.float32)
    y = _c(y, np.float32)
    assert x.ndim == 2 and y.ndim == 2 and x.shape[1] == y.shape[1]
    self.k = x.shape[1]
    self._chk(lib().hgx_alg_set(self.h, self.k, _ptr(x), _ptr(y)))

  def alg_run(self, iters):
    self._chk(lib().hgx_alg_run(self.h, iters))

  def alg_get(self):
    x = np.empty((self.inc.N, self.k), np.float32)
    y = np.empty((self.inc.E, self.k), np.float32)
    self._chk(lib().hgx_alg_get(self.h, _ptr(x), _ptr(y)))
    return x, y

  def alg_dist(self, x, y, iters):
    self.alg_set(x, y)
    self.alg_run(iters)
    return self.alg_get()

  def alg_stats(self):
    ms, by = ctypes.c_double(), ctypes.c_double()
    self._chk(lib().hgx_alg_last_stats(self.h, ctypes.byref(ms),
                                       ctypes.byref(by)))
    return ms.value, by.value

  # sharded relaxation (exchange buffers are caller-owned device pointers)
  def alg_shard_begin(self, row0, row1, d_partial, d_mm, iters):
    ks = ctypes.c_int()
    self._chk(lib().hgx_alg_shard_begin(self.h, row0, row1, d_partial, d_mm,
                                        iters, ctypes.byref(ks)))
    return ks.value

  def alg_shard_node(self, it):
    self._chk(lib().hgx_alg_shard_node(self.h, it))

  def alg_shard_edge_partial(self, it):
    self._chk(lib().hgx_alg_shard_edge_partial(self.h, it))

  def alg_shard_ranges(self, n):
    """Split the local edge rows into n ranges; returns the n + 1 bounds."""
    b = np.zeros(n + 1, np.int32)
    self._chk(lib().hgx_alg_shard_ranges(self.h, n, _ptr(b)))
    return b

  def alg_shard_edge_partial_range(self, it, r):
    self._chk(lib().hgx_alg_shard_edge_partial_range(self.h, it, r))

  def alg_shard_edge_final(self, it):
    self._chk(lib().hgx_alg_shard_edge_final(self.h, it))

  def alg_shard_end(self):
    self._chk(lib().hgx_alg_shard_end(self.h))

  def alg_shard_wire(self, d_wire, n_shared, edge_slot):
    es = _c(edge_slot, np.int32)
    self._keep_slot = es
    self._chk(lib().hgx_alg_shard_wire(self.h, d_wire, n_shared, _ptr(es)))

  # ---- HOBE probabilities / incidence weights ----
  def hobe_probs(self, kind, a, b):
    a = _c(a, np.int32)
    b = _c(b, np.int32)
    out = np.empty(a.size, np.float32)
    self._chk(lib().hgx_hobe_probs(self.h, kind, a.size, _ptr(a), _ptr(b),
                                   _ptr(out)))
    return out

  def incidence_weights(self, which, alpha=0.0):
    n = np.empty(self.inc.nnz, np.float32)
    e = np.empty(self.inc.nnz, np.float32)
    self._chk(lib().hgx_incidence_weights(self.h, which, alpha, _ptr(n),
                                          _ptr(e)))
    return n, e

  # hg2v_weighting distance / span weights (vectors = the alg coordinates)
  def weight_distance(self, norm=NORM_L2, alpha=0.0):
    """WeightByDistance values per incidence, A and A^T CSR order."""
    n = np.empty(self.inc.nnz, np.float32)
    e = np.empty(self.inc.nnz, np.float32)
    self._chk(lib().hgx_weight_distance(self.h, norm, float(alpha), _ptr(n),
                                        _ptr(e)))
    return n, e

  def weight_same_type(self, side, norm=NORM_L2, alpha=0.0):
    """WeightBySameTypeDistance CSR (rowptr int64, col int32, val float32)
    of the node (side 0) or edge (side 1) pattern, compressed ids."""
    R = self.inc.N if side == 0 else self.inc.E
    nnz = ctypes.c_int64()
    rp = np.empty(R + 1, np.int64)
    self._chk(lib().hgx_weight_same_type(self.h, side, norm, float(alpha),
                                         ctypes.byref(nnz), _ptr(rp), None, None))
    col = np.empty(nnz.value, np.int32)
    val = np.empty(nnz.value, np.float32)
    self._chk(lib().hgx_weight_same_type(self.h, side, norm, float(alpha),
                                         ctypes.byref(nnz), _ptr(rp), _ptr(col),
                                         _ptr(val)))
    return rp, col, val

  def weight_span(self, alpha=0.0):
    """(node spans, edge spans) float32 and the span weights per incidence
    (A and A^T CSR order)."""
    sn = np.empty(self.inc.N, np.float32)
    se = np.empty(self.inc.E, np.float32)
    n = np.empty(self.inc.nnz, np.float32)
    e = np.empty(self.inc.nnz, np.float32)
    self._chk(lib().hgx_weight_span(self.h, float(alpha), _ptr(sn), _ptr(se),
                                    _ptr(n), _ptr(e)))
    return sn, se, n, e

  def probe_gather(self, table_bytes, row_floats=16, in_flight=8, reps=3):
    """Random-row gather rate (rows/s) of the device (hgx_probe_gather)."""
    v = ctypes.c_double()
    self._chk(lib().hgx_probe_gather(self.h, int(table_bytes), row_floats,
                                     in_flight, reps, ctypes.byref(v)))
    return v.value

  # ---- samplers / records ----
  def sample_fobe(self, seed, K, node_q, edge_q, neg_node_q=None,
                  neg_edge_q=None):
    nq, eq = _c(node_q, np.int32), _c(edge_q, np.int32)
    nnq, neq = _c(neg_node_q, np.int32), _c(neg_edge_q, np.int32)
    n = ctypes.c_int64()
    self._chk(lib().hgx_sample_fobe(self.h, seed & (2**64 - 1), K, _ptr(nq),
                                    _ptr(eq), _ptr(nnq), _ptr(neq),
                                    ctypes.byref(n)))
    return n.value

  def sample_hobe(self, seed, K, S, node_q=None, edge_q=None):
    """AlgebraicDistanceSamples on the device; with node_q / edge_q only
    those rows (quota per row instead of S)."""
    n = ctypes.c_int64()
    if node_q is None and edge_q is None:
      self._chk(lib().hgx_sample_hobe(self.h, seed & (2**64 - 1), K, S,
                                      ctypes.byref(n)))
    else:
      nq, eq = _c(node_q, np.int32), _c(edge_q, np.int32)
      assert nq.size == self.inc.N and eq.size == self.inc.E
      self._chk(lib().hgx_sample_hobe_rows(self.h, seed & (2**64 - 1), K,
                                           _ptr(nq), _ptr(eq), S,
                                           ctypes.byref(n)))
    return n.value

  def _mt_call(self, fn, *args):
    """Run a numpy-seeded sampler on numpy's global RandomState: its MT19937
    state goes in, the state the reference leaves behind comes back."""
    st = np.random.get_state()
    if st[0] != "MT19937":
      raise ValueError("numpy's global RandomState is not MT19937")
    key = np.array(st[1], dtype=np.uint32, copy=True)
    pos = ctypes.c_int(int(st[2]))
    n = ctypes.c_int64()
    self._chk(fn(self.h, _ptr(key), ctypes.byref(pos), *args, ctypes.byref(n)))
    np.random.set_state((st[0], key, pos.value, st[3], st[4]))
    return n.value

  def sample_fobe_mt(self, K, node_q, edge_q, neg_node_q=None, neg_edge_q=None):
    """BooleanSamples drawing from numpy's global RandomState (the
    reference's stream bit for bit; hgx_sample_fobe_mt)."""
    nq, eq = _c(node_q, np.int32), _c(edge_q, np.int32)
    nnq, neq = _c(neg_node_q, np.int32), _c(neg_edge_q, np.int32)
    for q, n in ((nq, self.inc.N), (eq, self.inc.E), (nnq, self.inc.N),
                 (neq, self.inc.E)):
      assert q is None or q.size == n, "one quota per row"
    return self._mt_call(lib().hgx_sample_fobe_mt, K, _ptr(nq), _ptr(eq),
                         _ptr(nnq), _ptr(neq))

  def sample_hobe_mt(self, K, S):
    """AlgebraicDistanceSamples(run_in_parallel=False) drawing from numpy's
    global RandomState (hgx_sample_hobe_mt)."""
    return self._mt_call(lib().hgx_sample_hobe_mt, K, S)

  def sample_jaccard_mt(self, K, node_q, edge_q):
    """WeightedJaccardSamples(run_in_parallel=False) drawing from numpy's
    global RandomState (hgx_sample_jaccard_mt; features_set first)."""
    nq, eq = _c(node_q, np.int32), _c(edge_q, np.int32)
    assert nq.size == self.inc.N and eq.size == self.inc.E
    return self._mt_call(lib().hgx_sample_jaccard_mt, K, _ptr(nq), _ptr(eq))

  # weighted-Jaccard samplers
  def features_set(self, node_major, edge_major):
    fn, fe = _c(node_major, np.float32), _c(edge_major, np.float32)
    assert fn.size == self.inc.nnz and fe.size == self.inc.nnz
    self._chk(lib().hgx_features_set(self.h, _ptr(fn), _ptr(fe)))

  def sample_jaccard(self, seed, K, node_q, edge_q):
    nq, eq = _c(node_q, np.int32), _c(edge_q, np.int32)
    n = ctypes.c_int64()
    self._chk(lib().hgx_sample_jaccard(self.h, seed & (2**64 - 1), K, _ptr(nq),
                                       _ptr(eq), ctypes.byref(n)))
    return n.value

  def jaccard_probs(self, kind, a, b):
    a, b = _c(a, np.int32), _c(b, np.int32)
    out = np.empty(a.size, np.float32)
    self._chk(lib().hgx_jaccard_probs(self.h, kind, a.size, _ptr(a), _ptr(b),
                                      _ptr(out)))
    return out

  def jaccard_centroids(self, which):
    """(p int64, j int32, v float32) of the node (0) / edge (1) centroids."""
    R = self.inc.N if which == 0 else self.inc.E
    nnz = ctypes.c_int64()
    self._chk(lib().hgx_jaccard_centroids(self.h, which, ctypes.byref(nnz),
                                          None, None, None))
    p = np.empty(R + 1, np.int64)
    j = np.empty(nnz.value, np.int32)
    v = np.empty(nnz.value, np.float32)
    self._chk(lib().hgx_jaccard_centroids(self.h, which, ctypes.byref(nnz),
                                          _ptr(p), _ptr(j), _ptr(v)))
    return p, j, v

  def sample_stats(self):
    """(rows sampled by rejection, fallbacks to expansion) of the last call."""
    u, f = ctypes.c_int64(), ctypes.c_int64()
    self._chk(lib().hgx_sample_last_stats(self.h, ctypes.byref(u),
                                          ctypes.byref(f)))
    return u.value, f.value

  def sample_uniform_rows(self):
    """3-hop rows of the last call sampled by uniform-column rejection."""
    u = ctypes.c_int64()
    self._chk(lib().hgx_sample_uniform_rows(self.h, ctypes.byref(u)))
    return u.value

  def records_set(self, idx, tgt):
    idx = _c(idx, np.int32)
    tgt = _c(tgt, np.float32)
    n, R = idx.shape
    assert R % 2 == 0 and R >= 4 and tgt.shape == (n, 3)
    self._chk(lib().hgx_records_set(self.h, n, (R - 4) // 2, _ptr(idx),
                                    _ptr(tgt)))

  def records_copy_from(self, other):
    """This context's records := `other`'s (device to device, same GPU)."""
    self._chk(lib().hgx_records_copy(self.h, other.h))

  def records_info(self):
    n, K = ctypes.c_int64(), ctypes.c_int()
    self._chk(lib().hgx_records_info(self.h, ctypes.byref(n), ctypes.byref(K)))
    return n.value, K.value

  def records_blocks(self):
    """Kind-block bounds of the record stream (nblocks + 1 int64)."""
    nb = ctypes.c_int()
    b = np.zeros(17, np.int64)
    self._chk(lib().hgx_records_blocks(self.h, ctypes.byref(nb), _ptr(b)))
    return b[:nb.value + 1].copy()

  def records_export(self, d_idx, d_tgt):
    """Copy the records into caller device buffers (data pointers)."""
    self._chk(lib().hgx_records_export(self.h, d_idx, d_tgt))

  def records_import(self, n, K, d_idx, d_tgt, bounds=None):
    """Set the records from caller device buffers (data pointers)."""
    b = None if bounds is None else _c(bounds, np.int64)
    nb = 0 if b is None else b.size - 1
    self._chk(lib().hgx_records_import(self.h, n, K, d_idx, d_tgt, nb, _ptr(b)))

  def records_get(self):
    n, K = self.records_info()
    idx = np.empty((n, 4 + 2 * K), np.int32)
    tgt = np.empty((n, 3), np.float32)
    self._chk(lib().hgx_records_get(self.h, _ptr(idx), _ptr(tgt)))
    return idx, tgt

  # ---- compact record store (streams larger than HBM, hgx_store_*) ----
  def store_reset(self, capacity=0):
    self._chk(lib().hgx_store_reset(self.h, int(capacity)))

  def store_release(self):
    """Free the store, its load scratch and the loaded records."""
    self._chk(lib().hgx_store_release(self.h))

  def store_append(self):
    """Pack the records of the last sample_fobe / sample_hobe call."""
    self._chk(lib().hgx_store_append(self.h))

  def store_info(self):
    """(records, family, K, seed) of the store."""
    n, fam, K = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    seed = ctypes.c_uint64()
    self._chk(lib().hgx_store_info(self.h, ctypes.byref(n), ctypes.byref(fam),
                                   ctypes.byref(K), ctypes.byref(seed)))
    return n.value, fam.value, K.value, seed.value

  def store_read(self, start=0, n=None, dst_ptr=None):
    """Entries [start, start + n) as an (n, 3) uint32 host array, or into
    the device buffer at dst_ptr."""
    if n is None:
      n = self.store_info()[0] - start
    if dst_ptr is not None:
      self._chk(lib().hgx_store_read(self.h, start, n, dst_ptr, 1))
      return None
    out = np.empty((n, 3), np.uint32)
    self._chk(lib().hgx_store_read(self.h, start, n, _ptr(out), 0))
    return out

  def store_write(self, entries, family, K, seed, n=None, src_ptr=None):
    """Append raw entries ((n, 3) uint32 host array, or n at device src_ptr)
    packed by a sampler of `family` / K / seed (another rank's store)."""
    if src_ptr is None:
      e = _c(entries, np.uint32).reshape(-1, 3)
      self._chk(lib().hgx_store_write(self.h, e.shape[0], _ptr(e), 0, family, K,
                                      seed & (2**64 - 1)))
    else:
      self._chk(lib().hgx_store_write(self.h, int(n), src_ptr, 1, family, K,
                                      seed & (2**64 - 1)))

  def store_plan(self, epoch_seed, budget):
    """The epoch's chunks: (bin bounds, record counts)."""
    nc = ctypes.c_int()
    b = np.zeros(STORE_BINS + 1, np.int32)
    c = np.zeros(STORE_BINS + 1, np.int64)
    self._chk(lib().hgx_store_plan(self.h, epoch_seed & (2**64 - 1), int(budget),
                                   ctypes.byref(nc), _ptr(b), _ptr(c)))
    return b[:nc.value + 1].copy(), c[:nc.value].copy()

  def store_load(self, epoch_seed, bin_lo, bin_hi, batch, last):
    """One chunk of the epoch as the record stream (trained in order);
    returns the records to train."""
    n = ctypes.c_int64()
    self._chk(lib().hgx_store_load(self.h, epoch_seed & (2**64 - 1), int(bin_lo),
                                   int(bin_hi), int(batch), 1 if last else 0,
                                   ctypes.byref(n)))
    return n.value

  # ---- model / trainer ----
  def model_init(self, d, node_rows, edge_rows, seed=0, node_tab=None,
                 edge_tab=None):
    nt, et = _c(node_tab, np.float32), _c(edge_tab, np.float32)
    if nt is not None:
      assert nt.shape == (node_rows, d) and et.shape == (edge_rows, d)
    self.d, self.node_rows, self.edge_rows = d, node_rows, edge_rows
    self._chk(lib().hgx_model_init(self.h, d, node_rows, edge_rows,
                                   seed & (2**64 - 1), _ptr(nt), _ptr(et)))

  def model_get(self):
    nt = np.empty((self.node_rows, self.d), np.float32)
    et = np.empty((self.edge_rows, self.d), np.float32)
    self._chk(lib().hgx_model_get(self.h, _ptr(nt), _ptr(et)))
    return nt, et

  def model_get_rows(self, table, rows):
    """Rows of the node (0) or edge (1) table, (len(rows), d) float32."""
    r = _c(rows, np.int64).ravel()
    out = np.empty((r.size, self.d), np.float32)
    self._chk(lib().hgx_model_get_rows(self.h, table, r.size, _ptr(r), _ptr(out)))
    return out

  def train(self, batch=256, max_epochs=10, lr=0.01, eps=1e-7, loss=LOSS_MSE,
            act=ACT_RELU, min_delta=1e-3, shuffle_seed=0, perms=None):
    pp = None
    if perms is not None:
      pp = _c(perms, np.int64)
      max_epochs = min(max_epochs, pp.shape[0])
    losses = np.zeros(max(max_epochs, 1), np.float32)
    ran = ctypes.c_int()
    self._chk(lib().hgx_train(self.h, batch, max_epochs, lr, eps, loss, act,
                              min_delta, shuffle_seed & (2**64 - 1), _ptr(pp),
                              _ptr(losses), ctypes.byref(ran)))
    return losses[:ran.value].copy()

  def train_stats(self):
    ms, rec, bat = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
    self._chk(lib().hgx_train_last_stats(self.h, ctypes.byref(ms),
                                         ctypes.byref(rec), ctypes.byref(bat)))
    return ms.value, rec.value, bat.value

  def train_loss_sum(self):
    """Sum of the per-record losses of the last trained epoch (double)."""
    v = ctypes.c_double()
    self._chk(lib().hgx_train_last_loss(self.h, ctypes.byref(v)))
    return v.value

  def train_path_stats(self):
    """(fused, split) batch counts of the last train() call."""
    f, sp = ctypes.c_int64(), ctypes.c_int64()
    self._chk(lib().hgx_train_path_stats(self.h, ctypes.byref(f),
                                         ctypes.byref(sp)))
    return f.value, sp.value

  def train_multi_pending(self):
    """Step batches of the last train() in the MULTI pending-slot form."""
    v = ctypes.c_int64()
    self._chk(lib().hgx_train_multi_pending(self.h, ctypes.byref(v)))
    return v.value

  def train_step_geometry(self):
    """(threads, records) per workgroup of the last train()'s deferred-row
    step, (0, 0) without it; the paired-wave form is (512, 4)."""
    t, r = ctypes.c_int(), ctypes.c_int()
    self._chk(lib().hgx_train_step_geometry(self.h, ctypes.byref(t),
                                            ctypes.byref(r)))
    return t.value, r.value


class Mlp:
  """One hgx_mlp engine (include/hgx.h, dense MLP section) on a Context."""

  def __init__(self, ctx, kind, in_dim, out_dim=0):
    self.ctx, self.kind, self.in_dim, self.out_dim = ctx, kind, in_dim, out_dim
    h = _vp()
    ctx._chk(lib().hgx_mlp_create(ctx.h, kind, in_dim, out_dim, ctypes.byref(h)))
    self.h = h
    ctx._engines.add(self)
    n = ctypes.c_int()
    ctx._chk(lib().hgx_mlp_layers(self.h, ctypes.byref(n), None))
    sh = np.empty((n.value, 2), np.int32)
    ctx._chk(lib().hgx_mlp_layers(self.h, ctypes.byref(n), _ptr(sh)))
    self.shapes = [tuple(int(v) for v in r) for r in sh]

  def close(self):
    if getattr(self, "h", None):
      lib().hgx_mlp_destroy(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def num_weights(self):
    return sum(k * n + n for k, n in self.shapes)

  def set_weights(self, flat):
    flat = _c(flat, np.float32)
    assert flat.size == self.num_weights()
    self.ctx._chk(lib().hgx_mlp_set_weights(self.h, _ptr(flat)))

  def get_weights(self):
    flat = np.empty(self.num_weights(), np.float32)
    self.ctx._chk(lib().hgx_mlp_get_weights(self.h, _ptr(flat)))
    return flat

  def set_tables(self, node_tab, edge_tab):
    nt, et = _c(node_tab, np.float32), _c(edge_tab, np.float32)
    assert nt.ndim == 2 and et.ndim == 2
    assert nt.shape[1] == self.in_dim and et.shape[1] == self.in_dim
    self.ctx._chk(lib().hgx_mlp_set_tables(self.h, nt.shape[0], _ptr(nt),
                                           et.shape[0], _ptr(et)))

  def set_samples(self, node_row, edge_row, label):
    nr, er = _c(node_row, np.int32), _c(edge_row, np.int32)
    lab = _c(label, np.float32)
    assert nr.shape == er.shape == lab.shape
    self.ctx._chk(lib().hgx_mlp_set_samples(self.h, nr.size, _ptr(nr), _ptr(er),
                                            _ptr(lab)))

  def fit(self, batch=256, max_epochs=1, lr=0.01, eps=1e-7, min_delta=0.0,
          seed=0, perms=None):
    pp = None
    if perms is not None:
      pp = _c(perms, np.int64)
      max_epochs = min(max_epochs, pp.shape[0])
    losses = np.zeros(max(max_epochs, 1), np.float32)
    ran = ctypes.c_int()
    self.ctx._chk(lib().hgx_mlp_fit(self.h, batch, max_epochs, lr, eps,
                                    min_delta, seed & (2**64 - 1), _ptr(pp),
                                    _ptr(losses), ctypes.byref(ran)))
    return losses[:ran.value].copy()

  def predict(self, output, node_row=None, edge_row=None):
    nr, er = _c(node_row, np.int32), _c(edge_row, np.int32)
    n = (nr if nr is not None else er).size
    shape = (n,) if output == 0 else (n, self.out_dim)
    out = np.empty(shape, np.float32)
    self.ctx._chk(lib().hgx_mlp_predict(self.h, output, n, _ptr(nr), _ptr(er),
                                        _ptr(out)))
    return out

  def stats(self):
    ms, fl = ctypes.c_double(), ctypes.c_double()
    sm, bt = ctypes.c_int64(), ctypes.c_int64()
    self.ctx._chk(lib().hgx_mlp_last_stats(self.h, ctypes.byref(ms),
                                           ctypes.byref(sm), ctypes.byref(bt),
                                           ctypes.byref(fl)))
    return {"ms": ms.value, "samples": sm.value, "batches": bt.value,
            "flops": fl.value}


class Svc:
  """One hgx_svc engine (include/hgx.h, batched RBF C-SVC section): a float32
  table on a Context, the problems of the last ``fit`` and their dual
  coefficients on the device."""

  def __init__(self, ctx, table):
    tab = _c(table, np.float32)
    assert tab.ndim == 2
    self.ctx, self.dim, self.n_rows = ctx, tab.shape[1], tab.shape[0]
    h = _vp()
    ctx._chk(lib().hgx_svc_create(ctx.h, self.dim, self.n_rows, _ptr(tab),
                                  ctypes.byref(h)))
    self.h = h
    self.n_prob = self.n_samp = 0
    ctx._engines.add(self)

  def close(self):
    if getattr(self, "h", None):
      lib().hgx_svc_destroy(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def fit(self, off, row, label, C=1.0, gamma=0.1, eps=1e-3, max_iter=0):
    """Solve the problems [off[p], off[p + 1]) of (row, 0/1 label) samples;
    returns (iterations, status) per problem, status 1 = iteration cap."""
    off, row = _c(off, np.int64), _c(row, np.int32)
    label = _c(label, np.uint8)
    n_prob = off.size - 1
    assert n_prob >= 1 and row.size == label.size == off[-1]
    iters = np.zeros(n_prob, np.int32)
    status = np.zeros(n_prob, np.int32)
    self.ctx._chk(lib().hgx_svc_fit(self.h, n_prob, _ptr(off), _ptr(row),
                                    _ptr(label), C, gamma, eps, int(max_iter),
                                    _ptr(iters), _ptr(status)))
    self.n_prob, self.n_samp = n_prob, int(off[-1])
    return iters, status

  def decision(self, prob, row):
    """f of table row ``row[q]`` under problem ``prob[q]``'s classifier."""
    prob, row = _c(prob, np.int32), _c(row, np.int32)
    assert prob.shape == row.shape
    out = np.empty(prob.size, np.float32)
    self.ctx._chk(lib().hgx_svc_decision(self.h, prob.size, _ptr(prob),
                                         _ptr(row), _ptr(out)))
    return out

  def decision_vec(self, prob, vecs):
    """f of the free vector ``vecs[q]`` under problem ``prob[q]``."""
    prob = _c(prob, np.int32)
    vecs = _c(vecs, np.float32).reshape(-1, self.dim)
    assert prob.size == vecs.shape[0]
    out = np.empty(prob.size, np.float32)
    self.ctx._chk(lib().hgx_svc_decision_vec(self.h, prob.size, _ptr(prob),
                                             _ptr(vecs), _ptr(out)))
    return out

  def get(self):
    """(coef = s * alpha per sample, rho per problem) of the last fit."""
    coef = np.empty(self.n_samp, np.float32)
    rho = np.empty(self.n_prob, np.float32)
    self.ctx._chk(lib().hgx_svc_get(self.h, _ptr(coef), _ptr(rho)))
    return coef, rho

  def stats(self):
    f, d = ctypes.c_double(), ctypes.c_double()
    self.ctx._chk(lib().hgx_svc_last_stats(self.h, ctypes.byref(f),
                                           ctypes.byref(d)))
    return {"fit_ms": f.value, "decision_ms": d.value}


class Svd:
  """One hgx_svd engine (include/hgx.h, truncated-SVD block primitives) on a
  Context whose incidence is uploaded: fp32 panels with one row per edge
  (side 0) or per node (side 1) in slots 0..7, and the block products on
  column ranges of them. This is the device backend of svd.svd_incidence."""

  EDGE, NODE = 0, 1

  def __init__(self, ctx, long_row=0):
    self.ctx = ctx
    h = _vp()
    ctx._chk(lib().hgx_svd_create(ctx.h, int(long_row), ctypes.byref(h)))
    self.h = h
    self.rows = (ctx.inc.E, ctx.inc.N)
    self._side = {}
    ctx._engines.add(self)

  def close(self):
    if getattr(self, "h", None):
      lib().hgx_svd_destroy(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def panel(self, slot, side, width):
    self.ctx._chk(lib().hgx_svd_panel(self.h, slot, side, width))
    self._side[slot] = side

  def set(self, slot, col0, host):
    host = _c(host, np.float32)
    assert host.ndim == 2 and host.shape[0] == self.rows[self._side[slot]]
    self.ctx._chk(lib().hgx_svd_set(self.h, slot, col0, host.shape[1],
                                    _ptr(host)))

  def get(self, slot, col0, ncols):
    out = np.empty((self.rows[self._side[slot]], ncols), np.float32)
    self.ctx._chk(lib().hgx_svd_get(self.h, slot, col0, ncols, _ptr(out)))
    return out

  def copy(self, dst, dcol0, src, scol0, ncols):
    self.ctx._chk(lib().hgx_svd_copy(self.h, dst, dcol0, src, scol0, ncols))

  def spmm(self, dst, dcol0, src, scol0, ncols):
    self.ctx._chk(lib().hgx_svd_spmm(self.h, dst, dcol0, src, scol0, ncols))

  def gram(self, pslot, pcol0, p, qslot, qcol0, q):
    out = np.empty((p, q), np.float64)
    self.ctx._chk(lib().hgx_svd_gram(self.h, pslot, pcol0, p, qslot, qcol0, q,
                                     _ptr(out)))
    return out

  def apply(self, dst, dcol0, src, scol0, M, beta=0.0):
    M = _c(M, np.float64)
    assert M.ndim == 2
    q, p = M.shape
    self.ctx._chk(lib().hgx_svd_apply(self.h, dst, dcol0, p, src, scol0, q,
                                      _ptr(M), float(beta)))

  def scale(self, slot, col0, scale):
    scale = _c(scale, np.float64).ravel()
    self.ctx._chk(lib().hgx_svd_scale(self.h, slot, col0, scale.size,
                                      _ptr(scale)))

  def stats(self):
    ms, by = ctypes.c_double(), ctypes.c_double()
    n, c, d = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    self.ctx._chk(lib().hgx_svd_last_stats(self.h, ctypes.byref(ms),
                                           ctypes.byref(by), ctypes.byref(n),
                                           ctypes.byref(c), ctypes.byref(d)))
    return {"spmm_ms": ms.value, "spmm_bytes": by.value, "spmm_calls": n.value,
            "spmm_cols": c.value, "dense_calls": d.value}

  def cd_sweep(self, pslot, pcol0, bslot, bcol0, Q):
    """One coordinate-descent sweep (hgx_svd_cd_sweep) of the k columns from
    pcol0 of pslot against the k columns from bcol0 of bslot, Q the k x k
    float64 Gram of the other factor; returns the summed violation."""
    Q = _c(Q, np.float64)
    assert Q.ndim == 2 and Q.shape[0] == Q.shape[1]
    v = ctypes.c_double()
    self.ctx._chk(lib().hgx_svd_cd_sweep(self.h, pslot, pcol0, bslot, bcol0,
                                         Q.shape[0], _ptr(Q), ctypes.byref(v)))
    return v.value

  def cd_sweep_fused(self, pslot, pcol0, xslot, xcol0, Q):
    """cd_sweep with the product formed inside the kernel in float64 from the
    k columns from xcol0 of xslot, a panel of the other side
    (hgx_svd_cd_sweep_fused)."""
    Q = _c(Q, np.float64)
    assert Q.ndim == 2 and Q.shape[0] == Q.shape[1]
    v = ctypes.c_double()
    self.ctx._chk(lib().hgx_svd_cd_sweep_fused(
        self.h, pslot, pcol0, xslot, xcol0, Q.shape[0], _ptr(Q),
        ctypes.byref(v)))
    return v.value

  def cd_stats(self):
    ms, n = ctypes.c_double(), ctypes.c_int64()
    self.ctx._chk(lib().hgx_svd_cd_last_stats(self.h, ctypes.byref(ms),
                                              ctypes.byref(n)))
    return {"sweep_ms": ms.value, "sweeps": n.value}


class Ae:
  """One hgx_ae engine (include/hgx.h, auto-encoder baseline) on a Context
  whose incidence is uploaded: the model of one side (0: a row per node, 1: a
  row per edge) with its Adagrad state on the device. This is the device
  backend of auto_encoder.auto_encoder_incidence."""

  NODE, EDGE = 0, 1

  def __init__(self, ctx, side, dim):
    self.ctx, self.side, self.dim = ctx, int(side), int(dim)
    h = _vp()
    ctx._chk(lib().hgx_ae_create(ctx.h, self.side, self.dim, ctypes.byref(h)))
    self.h = h
    self.R, self.C = ((ctx.inc.E, ctx.inc.N) if self.side
                      else (ctx.inc.N, ctx.inc.E))
    ctx._engines.add(self)

  def close(self):
    if getattr(self, "h", None):
      lib().hgx_ae_destroy(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  def num_weights(self):
    return 2 * self.C * self.dim + self.dim + self.C

  def set_weights(self, W1, b1, W2, b2):
    flat = np.concatenate([
        _c(W1, np.float32).reshape(self.C * self.dim),
        _c(b1, np.float32).reshape(self.dim),
        _c(W2, np.float32).reshape(self.dim * self.C),
        _c(b2, np.float32).reshape(self.C)])
    self.ctx._chk(lib().hgx_ae_set_weights(self.h, _ptr(flat)))

  def get_weights(self):
    flat = np.empty(self.num_weights(), np.float32)
    self.ctx._chk(lib().hgx_ae_get_weights(self.h, _ptr(flat)))
    C, d = self.C, self.dim
    o = np.cumsum([0, C * d, d, d * C, C])
    return (flat[o[0]:o[1]].reshape(C, d).copy(), flat[o[1]:o[2]].copy(),
            flat[o[2]:o[3]].reshape(d, C).copy(), flat[o[3]:o[4]].copy())

  def draw(self, rows, samples_per_idx, seed, epoch):
    """(row, drop) int32 lists of the listed rows' samples (hgx_ae_draw)."""
    rows = _c(rows, np.int32).ravel()
    n = ctypes.c_int64()
    args = (self.h, rows.size, _ptr(rows), int(samples_per_idx),
            int(seed) & (2**64 - 1), int(epoch), ctypes.byref(n))
    self.ctx._chk(lib().hgx_ae_draw(*args, None, None))
    row = np.empty(n.value, np.int32)
    drop = np.empty(n.value, np.int32)
    if n.value:
      self.ctx._chk(lib().hgx_ae_draw(*args, _ptr(row), _ptr(drop)))
    return row, drop

  def step(self, row, drop, lr=0.01, eps=1e-7):
    """One train_on_batch on the explicit sample list; returns the loss."""
    row, drop = _c(row, np.int32).ravel(), _c(drop, np.int32).ravel()
    assert row.size == drop.size
    loss = _f32()
    self.ctx._chk(lib().hgx_ae_step(self.h, row.size, _ptr(row), _ptr(drop), lr,
                                    eps, ctypes.byref(loss)))
    return loss.value

  def fit(self, epochs=5, idx_per_batch=200, samples_per_idx=100, lr=0.01,
          eps=1e-7, seed=0, perms=None):
    """hgx_ae_fit; returns the per-batch losses, epochs x sections."""
    pp = None
    if perms is not None:
      pp = _c(perms, np.int64)
      assert pp.shape == (epochs, self.R)
    s = max(1, self.R // int(idx_per_batch))
    losses = np.zeros(max(epochs * s, 1), np.float32)
    nb = ctypes.c_int()
    self.ctx._chk(lib().hgx_ae_fit(self.h, int(epochs), int(idx_per_batch),
                                   int(samples_per_idx), lr, eps,
                                   int(seed) & (2**64 - 1), _ptr(pp),
                                   _ptr(losses), ctypes.byref(nb)))
    return losses[:nb.value].reshape(epochs, s).copy()

  def encode(self, rows):
    rows = _c(rows, np.int32).ravel()
    out = np.empty((rows.size, self.dim), np.float32)
    self.ctx._chk(lib().hgx_ae_encode(self.h, rows.size, _ptr(rows), _ptr(out)))
    return out

  def stats(self):
    ms, fl = ctypes.c_double(), ctypes.c_double()
    sm, bt = ctypes.c_int64(), ctypes.c_int64()
    self.ctx._chk(lib().hgx_ae_last_stats(self.h, ctypes.byref(ms),
                                          ctypes.byref(sm), ctypes.byref(bt),
                                          ctypes.byref(fl)))
    return {"ms": ms.value, "samples": sm.value, "batches": bt.value,
            "flops": fl.value}


class N2v:
  """One hgx_n2v engine (include/hgx.h, node2vec baselines) on a Context
  whose incidence is uploaded: the walks, the vocabulary tables and the two
  V x dim tables of the skip-gram trainer on the device, for the bipartite
  (0) or the clique (1) graph. This is the device backend of
  node2vec.node2vec_incidence."""

  BIPARTITE, CLIQUE = 0, 1

  def __init__(self, ctx, graph, dim):
    self.ctx, self.graph, self.dim = ctx, int(graph), int(dim)
    h = _vp()
    ctx._chk(lib().hgx_n2v_create(ctx.h, self.graph, self.dim, ctypes.byref(h)))
    self.h = h
    self.V = ctx.inc.N if self.graph else ctx.inc.N + ctx.inc.E
    ctx._engines.add(self)

  def close(self):
    if getattr(self, "h", None):
      lib().hgx_n2v_destroy(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  def walks(self, passes, sources, walk_length, p, seed, copy=True):
    """One walk per (pass, source), kept on the device; the (n, walk_length)
    int32 host copy unless ``copy`` is False (hgx_n2v_walks)."""
    ps, sr = _c(passes, np.int32).ravel(), _c(sources, np.int32).ravel()
    assert ps.size == sr.size
    out = np.empty((sr.size, int(walk_length)), np.int32) if copy else None
    self.ctx._chk(lib().hgx_n2v_walks(self.h, sr.size, _ptr(ps), _ptr(sr),
                                      int(walk_length), float(p),
                                      int(seed) & (2**64 - 1), _ptr(out)))
    return out

  def counts(self):
    """Occurrences of every vertex in the resident walks (int64)."""
    out = np.empty(self.V, np.int32)
    self.ctx._chk(lib().hgx_n2v_counts(self.h, _ptr(out)))
    return out.astype(np.int64)

  def set_vocab(self, keep, cum):
    keep, cum = _c(keep, np.uint32).ravel(), _c(cum, np.int32).ravel()
    assert keep.size == cum.size == self.V
    self.ctx._chk(lib().hgx_n2v_set_vocab(self.h, _ptr(keep), _ptr(cum)))

  def set_vectors(self, syn0, syn1=None):
    s0 = _c(syn0, np.float32).reshape(self.V, self.dim)
    s1 = None if syn1 is None else _c(syn1, np.float32).reshape(self.V, self.dim)
    self.ctx._chk(lib().hgx_n2v_set_vectors(self.h, _ptr(s0), _ptr(s1)))

  def get_vectors(self):
    s0 = np.empty((self.V, self.dim), np.float32)
    s1 = np.empty((self.V, self.dim), np.float32)
    self.ctx._chk(lib().hgx_n2v_get_vectors(self.h, _ptr(s0), _ptr(s1)))
    return s0, s1

  def train(self, walks=None, *, window=3, negative=5, epochs=5, alpha=0.025,
            min_alpha=1e-4, seed=0, concurrent=True):
    """Skip-gram with negative sampling over the resident walks, or over the
    explicit (n, walk_length) ``walks`` (hgx_n2v_train)."""
    w = None if walks is None else _c(walks, np.int32)
    n, L = (0, 0) if w is None else w.shape
    self.ctx._chk(lib().hgx_n2v_train(self.h, n, L, _ptr(w), int(window),
                                      int(negative), int(epochs), alpha,
                                      min_alpha, int(seed) & (2**64 - 1),
                                      1 if concurrent else 0))

  def set_tree(self, ptr, point, code):
    """The Huffman paths of deepwalk.huffman_tree (hgx_n2v_set_tree)."""
    ptr, point = _c(ptr, np.int32).ravel(), _c(point, np.int32).ravel()
    code = _c(code, np.uint8).ravel()
    assert ptr.size == self.V + 1
    assert point.size == code.size and (ptr[-1] < 0 or point.size >= ptr[-1])
    self.ctx._chk(lib().hgx_n2v_set_tree(self.h, _ptr(ptr), _ptr(point),
                                         _ptr(code)))

  def train_hs(self, walks=None, *, window=5, epochs=5, alpha=0.025,
               min_alpha=1e-4, seed=0, concurrent=True):
    """Skip-gram with hierarchical softmax over the resident walks, or over
    the explicit (n, walk_length) ``walks`` (hgx_n2v_train_hs)."""
    w = None if walks is None else _c(walks, np.int32)
    n, L = (0, 0) if w is None else w.shape
    self.ctx._chk(lib().hgx_n2v_train_hs(self.h, n, L, _ptr(w), int(window),
                                         int(epochs), alpha, min_alpha,
                                         int(seed) & (2**64 - 1),
                                         1 if concurrent else 0))

  def set_arcs(self, thr, alias, cum):
    """LINE's tables (line.alias_table over the incidences, both None for
    equal weights, and the negatives' cumulative table; hgx_n2v_set_arcs)."""
    thr = None if thr is None else _c(thr, np.uint32).ravel()
    alias = None if alias is None else _c(alias, np.int32).ravel()
    cum = _c(cum, np.int32).ravel()
    assert cum.size == self.V
    assert all(t is None or t.size == self.ctx.inc.nnz for t in (thr, alias))
    self.ctx._chk(lib().hgx_n2v_set_arcs(self.h, _ptr(thr), _ptr(alias),
                                         _ptr(cum)))

  def line_samples(self, s0, count, negative, seed):
    """(count, 2 + negative) int32: (u, v, negatives) of the samples s0,
    s0 + 1, ... (hgx_n2v_line_samples)."""
    out = np.empty((int(count), 2 + max(int(negative), 0)), np.int32)
    self.ctx._chk(lib().hgx_n2v_line_samples(self.h, int(s0), int(count),
                                             int(negative),
                                             int(seed) & (2**64 - 1),
                                             _ptr(out)))
    return out

  def train_line(self, order, negative, n_samples, rho=0.025, seed=0,
                 concurrent=True):
    """LINE of ``order`` 1 or 2 over ``n_samples`` edge samples
    (hgx_n2v_train_line)."""
    self.ctx._chk(lib().hgx_n2v_train_line(self.h, int(order), int(negative),
                                           int(n_samples), rho,
                                           int(seed) & (2**64 - 1),
                                           1 if concurrent else 0))

  def mp_walks(self, sources, num_walks, L, walk_seed, g0, count):
    """(count, L) int32: the walks g0 .. g0 + count - 1 of the metapath2vec
    corpus (hgx_n2v_mp_walks)."""
    sr = _c(sources, np.int32).ravel()
    out = np.empty((max(int(count), 0), max(int(L), 0)), np.int32)
    self.ctx._chk(lib().hgx_n2v_mp_walks(self.h, sr.size, _ptr(sr),
                                         int(num_walks), int(L),
                                         int(walk_seed) & (2**64 - 1), int(g0),
                                         int(count), _ptr(out)))
    return out

  def mp_counts(self, sources, num_walks, L, walk_seed):
    """Occurrences of every vertex over the streamed corpus, int64
    (hgx_n2v_mp_counts)."""
    sr = _c(sources, np.int32).ravel()
    out = np.empty(self.V, np.int64)
    self.ctx._chk(lib().hgx_n2v_mp_counts(self.h, sr.size, _ptr(sr),
                                          int(num_walks), int(L),
                                          int(walk_seed) & (2**64 - 1),
                                          _ptr(out)))
    return out

  def set_vocab_typed(self, keep, cum, typed):
    """The metapath2vec trainer's vocabulary: ``typed`` true for one segment
    of ``cum`` per vertex type (hgx_n2v_set_vocab_typed)."""
    keep, cum = _c(keep, np.uint32).ravel(), _c(cum, np.int32).ravel()
    assert keep.size == cum.size == self.V
    self.ctx._chk(lib().hgx_n2v_set_vocab_typed(self.h, _ptr(keep), _ptr(cum),
                                                1 if typed else 0))

  def train_mp(self, sources, num_walks, L, *, window=7, negative=5, epochs=5,
               alpha=0.025, min_alpha=2.5e-6, walk_seed=0, train_seed=0,
               concurrent=True):
    """metapath2vec(++) over the streamed corpus (hgx_n2v_train_mp)."""
    sr = _c(sources, np.int32).ravel()
    self.ctx._chk(lib().hgx_n2v_train_mp(
        self.h, sr.size, _ptr(sr), int(num_walks), int(L), int(window),
        int(negative), int(epochs), alpha, min_alpha,
        int(walk_seed) & (2**64 - 1), int(train_seed) & (2**64 - 1),
        1 if concurrent else 0))

  def mp_stats(self):
    """walks, words, pairs, targets and clamped of the last train_mp
    (hgx_n2v_last_mp_stats)."""
    v = [ctypes.c_int64() for _ in range(5)]
    self.ctx._chk(lib().hgx_n2v_last_mp_stats(
        self.h, *[ctypes.byref(x) for x in v]))
    return dict(zip(("walks", "words", "pairs", "targets", "clamped"),
                    (x.value for x in v)))

  def stats(self):
    wm, tm = ctypes.c_double(), ctypes.c_double()
    v = [ctypes.c_int64() for _ in range(9)]
    self.ctx._chk(lib().hgx_n2v_last_stats(self.h, ctypes.byref(wm),
                                           ctypes.byref(tm),
                                           *[ctypes.byref(x) for x in v[:5]]))
    self.ctx._chk(lib().hgx_n2v_last_hs_stats(self.h, ctypes.byref(v[5])))
    self.ctx._chk(lib().hgx_n2v_last_line_stats(
        self.h, *[ctypes.byref(x) for x in v[6:]]))
    return {"walk_ms": wm.value, "train_ms": tm.value, "walks": v[0].value,
            "words": v[1].value, "pairs": v[2].value,
            "expand_steps": v[3].value, "reject_steps": v[4].value,
            "path_nodes": v[5].value, "samples": v[6].value,
            "targets": v[7].value, "clamped": v[8].value,
            "mp": self.mp_stats()}


# ---- host utilities (no context, no device) --------------------------------
def synth_powerlaw(N, E, mean_degree=20.0, exponent=0.8, seed=0):
  """(rp_n, col_n, E_kept) of hgx_synth_powerlaw."""
  rp = np.zeros(N + 1, np.int32)
  nnz = ctypes.c_int64()
  rc = lib().hgx_synth_powerlaw(N, E, mean_degree, exponent, seed, _ptr(rp),
                                None, ctypes.byref(nnz), None)
  if rc != HGX_OK:
    _raise(rc, "hgx_synth_powerlaw failed")
  col = np.empty(nnz.value, np.int32)
  e_out = ctypes.c_int32()
  rc = lib().hgx_synth_powerlaw(N, E, mean_degree, exponent, seed, _ptr(rp),
                                _ptr(col), ctypes.byref(nnz),
                                ctypes.byref(e_out))
  if rc != HGX_OK:
    _raise(rc, "hgx_synth_powerlaw failed")
  return rp, col, int(e_out.value)


def csr_transpose(nrow, ncol, rp, col):
  rp = _c(rp, np.int32)
  col = _c(col, np.int32)
  rpt = np.empty(ncol + 1, np.int32)
  colt = np.empty(col.size, np.int32)
  rc = lib().hgx_csr_transpose(nrow, ncol, _ptr(rp), _ptr(col), _ptr(rpt),
                               _ptr(colt))
  if rc != HGX_OK:
    _raise(rc, "hgx_csr_transpose: column index out of range")
  return rpt, colt


def _host_raise(rc):
  _raise(rc, lib().hgx_host_last_error().decode(errors="replace"))


def parse_hypergraph(buf):
  """Serialized Hypergraph bytes (bytes / memoryview / uint8 array) ->
  dict of compressed-incidence arrays (hgx_proto_parse_hypergraph)."""
  a = np.frombuffer(buf, dtype=np.uint8)
  h = _vp()
  n, e, nnz = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
  rc = lib().hgx_proto_parse_hypergraph(_ptr(a) if a.size else None, a.size,
                                        ctypes.byref(h), ctypes.byref(n),
                                        ctypes.byref(e), ctypes.byref(nnz))
  if rc != HGX_OK:
    _host_raise(rc)
  try:
    out = {"N": n.value, "E": e.value,
           "rp_n": np.empty(n.value + 1, np.int32),
           "col_n": np.empty(nnz.value, np.int32),
           "node_ids": np.empty(n.value, np.int64),
           "edge_ids": np.empty(e.value, np.int64),
           "node_weight": np.empty(n.value, np.float32),
           "edge_weight": np.empty(e.value, np.float32)}
    rc = lib().hgx_proto_hypergraph_fill(
        h, _ptr(out["rp_n"]), _ptr(out["col_n"]), _ptr(out["node_ids"]),
        _ptr(out["edge_ids"]), _ptr(out["node_weight"]),
        _ptr(out["edge_weight"]))
    if rc != HGX_OK:
      _host_raise(rc)
  finally:
    lib().hgx_proto_hypergraph_free(h)
  return out


def write_embedding_bytes(node_ids, node_tab, edge_ids, edge_tab, method_name):
  """HypergraphEmbedding wire bytes (hgx_proto_write_embedding)."""
  node_ids = _c(node_ids, np.int64)
  edge_ids = _c(edge_ids, np.int64)
  node_tab = _c(node_tab, np.float32)
  edge_tab = _c(edge_tab, np.float32)
  d = int(node_tab.shape[1]) if node_tab.ndim == 2 else int(edge_tab.shape[1])
  assert node_tab.shape == (node_ids.size, d) and edge_tab.shape == (edge_ids.size, d)
  name = None if method_name is None else method_name.encode()
  ln = ctypes.c_int64()
  args = (node_ids.size, _ptr(node_ids), _ptr(node_tab), edge_ids.size,
          _ptr(edge_ids), _ptr(edge_tab), d, name)
  rc = lib().hgx_proto_write_embedding(*args, None, 0, ctypes.byref(ln))
  if rc != HGX_OK:
    _host_raise(rc)
  out = np.empty(ln.value, np.uint8)
  rc = lib().hgx_proto_write_embedding(*args, _ptr(out), out.size,
                                       ctypes.byref(ln))
  if rc != HGX_OK:
    _host_raise(rc)
  return out


def parse_embedding(buf):
  """Serialized HypergraphEmbedding bytes (one message or concatenated
  shards; bytes / memoryview / uint8 array / mmap) -> dict(node_ids,
  node_tab, edge_ids, edge_tab, dim, width, method_name)
  (hgx_proto_parse_embedding)."""
  a = np.frombuffer(buf, dtype=np.uint8)
  h = _vp()
  nn, ne, w = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
  dim = ctypes.c_int32()
  rc = lib().hgx_proto_parse_embedding(_ptr(a) if a.size else None, a.size,
                                       ctypes.byref(h), ctypes.byref(nn),
                                       ctypes.byref(ne), ctypes.byref(w),
                                       ctypes.byref(dim))
  if rc != HGX_OK:
    _host_raise(rc)
  try:
    W = w.value
    out = {"node_ids": np.empty(nn.value, np.int64),
           "node_tab": np.empty((nn.value, W), np.float32),
           "edge_ids": np.empty(ne.value, np.int64),
           "edge_tab": np.empty((ne.value, W), np.float32),
           "dim": dim.value, "width": W}
    mlen = lib().hgx_proto_embedding_method_len(h)
    name = ctypes.create_string_buffer(mlen + 1)
    rc = lib().hgx_proto_embedding_fill(
        h, _ptr(out["node_ids"]), _ptr(out["node_tab"]), _ptr(out["edge_ids"]),
        _ptr(out["edge_tab"]), name, mlen + 1)
    if rc != HGX_OK:
      _host_raise(rc)
    out["method_name"] = name.value.decode()
  finally:
    lib().hgx_proto_embedding_free(h)
  return out


def write_hypergraph_bytes(inc):
  """Hypergraph wire bytes of an Incidence (hgx_proto_write_hypergraph)."""
  ids = (_c(inc.node_ids, np.int64), _c(inc.edge_ids, np.int64))
  args = (inc.N, inc.E, _ptr(inc.rp_n), _ptr(inc.col_n), _ptr(inc.rp_e),
          _ptr(inc.col_e), _ptr(ids[0]), _ptr(ids[1]))
  ln = ctypes.c_int64()
  rc = lib().hgx_proto_write_hypergraph(*args, None, 0, ctypes.byref(ln))
  if rc != HGX_OK:
    _host_raise(rc)
  out = np.empty(ln.value, np.uint8)
  rc = lib().hgx_proto_write_hypergraph(*args, _ptr(out), out.size,
                                        ctypes.byref(ln))
  if rc != HGX_OK:
    _host_raise(rc)
  return out


# ---- Python-`random`-compatible link-prediction loops (host) ---------------
def _mt_state(rnd):
  ver, st, gauss = rnd.getstate()
  return np.array(st, np.uint32), (ver, gauss)


def _mt_restore(rnd, arr, meta):
  rnd.setstate((meta[0], tuple(int(v) for v in arr), meta[1]))


def _lp_chk(rc):
  if rc != HGX_OK:
    _raise(rc, lib().hgx_lp_last_error().decode())


def pyrandom_sample_missing(rnd, n_nodes, n_edges, rowptr, col, num_samples):
  """(node positions, edge positions) drawn as SampleMissingConnections
  draws them with the `random.Random` instance `rnd` (advanced)."""
  st, meta = _mt_state(rnd)
  rp = _c(rowptr, np.int64)
  cl = _c(col, np.int32)
  npos = np.empty(max(num_samples, 1), np.int32)
  epos = np.empty(max(num_samples, 1), np.int32)
  got = ctypes.c_int64()
  _lp_chk(lib().hgx_pyrandom_sample_missing(
      _ptr(st), n_nodes, n_edges, _ptr(rp), _ptr(cl), num_samples, _ptr(npos),
      _ptr(epos), ctypes.byref(got)))
  _mt_restore(rnd, st, meta)
  return npos[:got.value].copy(), epos[:got.value].copy()


def pyrandom_remove_connections(rnd, pair_node, pair_edge, node_deg,
                                edge_size, probability):
  """Indices of the pairs RemoveRandomConnections removes, in order."""
  st, meta = _mt_state(rnd)
  pn, pe = _c(pair_node, np.int32), _c(pair_edge, np.int32)
  nd = np.array(node_deg, np.int32)
  es = np.array(edge_size, np.int32)
  out = np.empty(max(pn.size, 1), np.int64)
  got = ctypes.c_int64()
  _lp_chk(lib().hgx_pyrandom_remove_connections(
      _ptr(st), pn.size, _ptr(pn), _ptr(pe), _ptr(nd), _ptr(es),
      float(probability), _ptr(out), ctypes.byref(got)))
  _mt_restore(rnd, st, meta)
  return out[:got.value].copy()
