"""The loaders' host preparation without an engine (fb_debug_prepare_* of include/fakebob_hip_test.h): what fb_load_gmm,
fb_load_ivector and fb_set_frontend would upload for the same arrays and the same environment, on a machine with or
without a GPU."""
import ctypes as C

import numpy as np

from . import _native as N

GMM_BUFFERS = {"fx": np.uint16, "bx": np.uint16, "fd": np.uint16, "anchor": np.float32, "item_model": np.int32}
IVECTOR_BUFFERS = {"dg_gc": np.float32, "dg_miv": np.float32, "dg_iv": np.float32, "fg_gc": np.float32, "tri": np.uint8,
                   "fg64": np.float64, "fgL": np.float64, "backend": np.float64, "backend_offsets": np.int64}
FRONTEND_BUFFERS = {"blob": np.uint8, "offsets": np.int64, "f32": np.float32}


def _fetch(call, dtype):
    """size-then-fill: call(out, cap, size_ref) -> the named buffer as an array of dtype"""
    size = C.c_int64()
    N.check(call(None, C.c_int64(0), C.byref(size)))
    out = np.empty(size.value // np.dtype(dtype).itemsize, dtype)
    N.check(call(N.ptr(out), C.c_int64(out.nbytes), C.byref(size)))
    return out


def gmm_plan(gc, miv, iv):
    """gconsts (M, C), means_invvars and inv_vars (M, C, D) -> (plan as a dict, the component permutation [C])"""
    gc, miv, iv = (np.ascontiguousarray(a, np.float32) for a in (gc, miv, iv))
    M, Cn, D = miv.shape
    plan = N.GmmPlan()
    perm = np.empty(Cn, np.int32)
    N.check(N.lib().fb_debug_prepare_gmm(C.c_int(M), C.c_int(Cn), C.c_int(D), N.ptr(gc), N.ptr(miv), N.ptr(iv), C.byref(plan),
                                         N.ptr(perm), None, C.c_int(0), None, C.c_int64(0), None))
    d = {name: getattr(plan, name) for name, _ in N.GmmPlan._fields_}
    d["pass_lo"] = list(plan.pass_lo)
    return d, perm


def gmm_buffer(gc, miv, iv, name, pass_=0):
    """one of GMM_BUFFERS ("fd": of pass pass_) as fb_load_gmm would upload it; empty when it is not built"""
    gc, miv, iv = (np.ascontiguousarray(a, np.float32) for a in (gc, miv, iv))
    M, Cn, D = miv.shape
    L = N.lib()
    return _fetch(lambda out, cap, size: L.fb_debug_prepare_gmm(
        C.c_int(M), C.c_int(Cn), C.c_int(D), N.ptr(gc), N.ptr(miv), N.ptr(iv), None, None, name.encode(), C.c_int(pass_),
        out, cap, size), GMM_BUFFERS[name])


def ivector_buffer(system, name):
    """one of IVECTOR_BUFFERS of a models.IvectorSystem"""
    sy, keep = N.ivector_struct(system)
    L = N.lib()
    return _fetch(lambda out, cap, size: L.fb_debug_prepare_ivector(C.byref(sy), name.encode(), out, cap, size),
                  IVECTOR_BUFFERS[name])


def xvector_buffer(system, name):
    """of a models.XvectorSystem: "w<l>" (uint16: layer l's f16 fragment image), "kw" (int32), "segT", "backend" (float64),
    "backend_offsets" (int64); "wt<l>" (uint16: layer l's transposed image, the white-box backward's) and "kwt" (int32)"""
    sy, keep = N.xvector_struct(system)
    L = N.lib()
    dtype = np.uint16 if name.startswith("w") else {"kw": np.int32, "kwt": np.int32, "backend_offsets": np.int64}.get(name, np.float64)
    return _fetch(lambda out, cap, size: L.fb_debug_prepare_xvector(C.byref(sy), name.encode(), out, cap, size), dtype)


def frontend_buffer(name, **over):
    """one of FRONTEND_BUFFERS of the stock front-end configuration with the fields of `over` replaced"""
    L = N.lib()
    cfg = N.FrontendCfg()
    L.fb_default_frontend(C.byref(cfg))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise KeyError(k)
        setattr(cfg, k, v)
    return _fetch(lambda out, cap, size: L.fb_debug_prepare_frontend(C.byref(cfg), name.encode(), out, cap, size),
                  FRONTEND_BUFFERS[name])
