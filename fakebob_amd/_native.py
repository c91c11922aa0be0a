"""ctypes binding of libfakebob_hip.so (include/fakebob_hip.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded,
importing the native layer raises.  (oracle/ is test infrastructure and is
never imported from here.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FAKEBOB_HIP_LIB: a library built elsewhere (an install prefix, a profiling build); default: the in-tree build
LIB_PATH = os.environ.get("FAKEBOB_HIP_LIB") or os.path.join(_HERE, "lib", "libfakebob_hip.so")

FB_OK = 0
FB_E_ARG, FB_E_HIP, FB_E_STATE, FB_E_NO_VOICED, FB_E_NOMEM, FB_E_LIMIT, FB_E_CALLBACK = -1, -2, -3, -4, -5, -6, -7
TASK = {"OSI": 0, "CSI": 1, "SV": 2}
ATTACK = {"untargeted": 0, "targeted": 1}


class FrontendCfg(C.Structure):
    """fb_frontend_cfg"""
    _fields_ = [
        ("sample_freq", C.c_double), ("frame_length", C.c_int), ("frame_shift", C.c_int),
        ("padded_length", C.c_int), ("num_mel_bins", C.c_int), ("num_ceps", C.c_int),
        ("low_freq", C.c_double), ("high_freq", C.c_double), ("preemph", C.c_double),
        ("cepstral_lifter", C.c_double), ("snip_edges", C.c_int), ("remove_dc", C.c_int),
        ("use_energy", C.c_int), ("raw_energy", C.c_int), ("energy_floor", C.c_double),
        ("vad_energy_threshold", C.c_double), ("vad_energy_mean_scale", C.c_double),
        ("vad_proportion_threshold", C.c_double), ("vad_frames_context", C.c_int),
        ("delta_window", C.c_int), ("delta_order", C.c_int), ("cmn_window", C.c_int), ("text_scores", C.c_int), ("compress_feats", C.c_int),
        ("mfcc_f32", C.c_int), ("dither", C.c_double),
    ]


class NesParams(C.Structure):
    """fb_nes_params"""
    _fields_ = [
        ("task", C.c_int), ("attack_type", C.c_int), ("adver_thresh", C.c_double),
        ("epsilon", C.c_double), ("max_iter", C.c_int), ("max_lr", C.c_double),
        ("min_lr", C.c_double), ("samples_per_draw", C.c_int), ("sigma", C.c_double),
        ("momentum", C.c_double), ("plateau_length", C.c_int), ("plateau_drop", C.c_double),
        ("threshold", C.c_double), ("target", C.c_int), ("true_label", C.c_int),
        ("seed", C.c_uint64), ("stream", C.c_uint32), ("bits_per_sample", C.c_int),
    ]


class PsoParams(C.Structure):
    """fb_pso_params"""
    _fields_ = [("particles", C.c_int), ("w_init", C.c_double), ("w_end", C.c_double), ("c1", C.c_double),
                ("c2", C.c_double), ("v_max", C.c_double)]


class Cw2Params(C.Structure):
    """fb_cw2_params"""
    _fields_ = [("initial_const", C.c_double), ("search_steps", C.c_int), ("lr", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("adam_eps", C.c_double), ("abort_every", C.c_int)]


class PsyParams(C.Structure):
    """fb_psy_params"""
    _fields_ = [("theta", C.c_void_p), ("n_frames", C.c_int), ("window", C.c_int), ("psd_max", C.c_double), ("l2_weight", C.c_double)]


class KvParams(C.Structure):
    """fb_kv_params"""
    _fields_ = [("window", C.c_int), ("grid", C.c_int), ("q_max", C.c_int), ("max_rounds", C.c_int)]


class HsjParams(C.Structure):
    """fb_hsj_params"""
    _fields_ = [("grid", C.c_int), ("max_rounds", C.c_int), ("num_evals_init", C.c_int), ("num_evals_max", C.c_int),
                ("max_queries", C.c_int), ("sigma_min", C.c_double), ("probe_scale", C.c_double)]


class IvectorSystem(C.Structure):
    """fb_ivector_system"""
    _fields_ = [
        ("C", C.c_int), ("D", C.c_int), ("R", C.c_int), ("L", C.c_int), ("S", C.c_int),
        ("lda_cols", C.c_int), ("num_gselect", C.c_int), ("min_post", C.c_double),
        ("prior_offset", C.c_double), ("fg_weights", C.c_void_p), ("fg_means_invcovars", C.c_void_p),
        ("fg_inv_covars", C.c_void_p), ("ie_M", C.c_void_p), ("ie_sigma_inv", C.c_void_p),
        ("mean_vec", C.c_void_p), ("lda", C.c_void_p), ("plda_mean", C.c_void_p),
        ("plda_transform", C.c_void_p), ("plda_psi", C.c_void_p), ("enrolled", C.c_void_p),
        ("z_mean", C.c_void_p), ("z_std", C.c_void_p),
    ]


def ivector_struct(system):
    """models.IvectorSystem -> (fb_ivector_system, the arrays it points into: keep them alive for the call)"""
    sy = IvectorSystem()
    sy.C, sy.D, sy.R, sy.L, sy.S = system.C, system.D, system.R, system.L, system.S
    sy.lda_cols = system.lda.shape[1]
    sy.num_gselect = system.num_gselect
    sy.min_post = system.min_post
    sy.prior_offset = system.prior_offset
    keep = []
    for name in ("fg_weights", "fg_means_invcovars", "fg_inv_covars", "ie_M", "ie_sigma_inv", "mean_vec",
                 "lda", "plda_mean", "plda_transform", "plda_psi", "enrolled", "z_mean", "z_std"):
        a = getattr(system, name)
        keep.append(a)
        setattr(sy, name, a.ctypes.data)
    return sy, keep


FB_XV_MAX_LAYERS, FB_XV_MAX_CTX = 8, 5


class XvectorLayer(C.Structure):
    """fb_xvector_layer"""
    _fields_ = [("dout", C.c_int), ("n_ctx", C.c_int), ("ctx", C.c_int * FB_XV_MAX_CTX), ("W", C.c_void_p),
                ("bias", C.c_void_p), ("bn_scale", C.c_void_p), ("bn_offset", C.c_void_p)]


class XvectorSystem(C.Structure):
    """fb_xvector_system"""
    _fields_ = [
        ("D", C.c_int), ("n_layers", C.c_int), ("layers", XvectorLayer * FB_XV_MAX_LAYERS),
        ("seg_W", C.c_void_p), ("seg_bias", C.c_void_p), ("R", C.c_int), ("L", C.c_int), ("S", C.c_int),
        ("lda_cols", C.c_int), ("mean_vec", C.c_void_p), ("lda", C.c_void_p), ("plda_mean", C.c_void_p),
        ("plda_transform", C.c_void_p), ("plda_psi", C.c_void_p), ("enrolled", C.c_void_p),
        ("z_mean", C.c_void_p), ("z_std", C.c_void_p),
    ]


def xvector_struct(system):
    """models.XvectorSystem -> (fb_xvector_system, the arrays it points into: keep them alive for the call).  More layers
    or context offsets than the struct holds are a ValueError here; every other limit is the library's to refuse."""
    if len(system.layers) > FB_XV_MAX_LAYERS:
        raise ValueError("an x-vector system has at most %d frame layers (got %d)" % (FB_XV_MAX_LAYERS, len(system.layers)))
    sy = XvectorSystem()
    sy.D, sy.n_layers = system.D, len(system.layers)
    keep = []
    for l, ly in enumerate(system.layers):
        d = sy.layers[l]
        d.dout, d.n_ctx = ly["W"].shape[0], len(ly["ctx"])
        if d.n_ctx <= FB_XV_MAX_CTX:     # (more: the library refuses n_ctx by name, it reads no offset then)
            for j, c in enumerate(ly["ctx"]):
                d.ctx[j] = c
        for name in ("W", "bias", "bn_scale", "bn_offset"):
            keep.append(ly[name])
            setattr(d, name, ly[name].ctypes.data)
    sy.R, sy.L, sy.S = system.R, system.L, system.S
    sy.lda_cols = system.lda.shape[1]
    for name in ("seg_W", "seg_bias", "mean_vec", "lda", "plda_mean", "plda_transform", "plda_psi", "enrolled", "z_mean", "z_std"):
        a = getattr(system, name)
        keep.append(a)
        setattr(sy, name, a.ctypes.data)
    return sy, keep


class GmmPlan(C.Structure):
    """fb_gmm_plan (include/fakebob_hip_test.h)"""
    _fields_ = [("mode", C.c_int), ("NK", C.c_int), ("NKF", C.c_int), ("kx", C.c_int), ("kx2", C.c_int), ("kacc", C.c_int),
                ("n_tiles", C.c_int), ("n_items", C.c_int), ("n_groups", C.c_int),
                ("delta_p", C.c_int), ("t3", C.c_int), ("t6", C.c_int), ("t2", C.c_int), ("n_pass", C.c_int),
                ("pass_lo", C.c_int * 4), ("delta_rms", C.c_double)]


# fb_score_cb: int (*)(void *ctx, const double *audios, int64_t N, int B, double *scores)
SCORE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int, C.POINTER(C.c_double))

# fb_score_dev_cb: int (*)(void *ctx, void *stream, int64_t N, int B, int S) -- a device-resident foreign model
SCORE_DEV_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int)
FB_DT_F32, FB_DT_F64 = 0, 1


class DevModel(C.Structure):
    """fb_dev_model"""
    _fields_ = [("x_dtype", C.c_int), ("x", C.c_void_p), ("score_dtype", C.c_int), ("scores", C.c_void_p),
                ("look_every", C.c_int)]


# fb_decide_cb: int (*)(void *ctx, const double *audios, int64_t N, int B, int *decisions, double *scores)
DECIDE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double))
FB_VICTIM_HOST_SCORES, FB_VICTIM_HOST_DECISIONS, FB_VICTIM_DEVICE_SCORES = 1, 2, 3


class Victim(C.Structure):
    """fb_victim"""
    _fields_ = [("mode", C.c_int), ("S", C.c_int), ("score", SCORE_CB), ("decide", DECIDE_CB), ("dev", C.POINTER(DevModel)),
                ("score_dev", SCORE_DEV_CB), ("ctx", C.c_void_p)]


class TfStage(C.Structure):
    """fb_tf_stage"""
    _fields_ = [("kind", C.c_int), ("k", C.c_int), ("taps", C.POINTER(C.c_double))]


FB_TF_QUANT, FB_TF_MEDIAN, FB_TF_FIR, FB_TF_DECIMATE, FB_TF_NOISE = 0, 1, 2, 3, 4


class AirParams(C.Structure):
    """fb_air_params"""
    _fields_ = [("taps", C.c_int), ("predelay", C.c_int), ("amp", C.c_double), ("rho_lo", C.c_double), ("rho_hi", C.c_double)]


class ForeignPathInfo(C.Structure):
    """fb_foreign_path_info (include/fakebob_hip_test.h)"""
    _fields_ = [("path", C.c_int), ("x_dtype", C.c_int), ("score_dtype", C.c_int), ("launches_per_iter", C.c_int),
                ("model_calls", C.c_int64), ("batch_bytes_d2h", C.c_int64), ("score_bytes_h2d", C.c_int64)]


EXPORTS = [
    "fb_last_error", "fb_version", "fb_device_count", "fb_engine_create", "fb_engine_destroy",
    "fb_default_frontend", "fb_set_frontend", "fb_set_dither_seed", "fb_set_input_transform", "fb_set_air_channel", "fb_set_codec", "fb_set_eot", "fb_set_companions", "fb_set_play_offset", "fb_debug_play_offsets", "fb_debug_play_route", "fb_bench_play_compose", "fb_debug_wb_play_compose_t", "fb_debug_wb_play_route", "fb_set_query_eot", "fb_set_feature_compression", "fb_load_gmm", "fb_load_ivector", "fb_set_system", "fb_num_speakers",
    "fb_score_i16", "fb_score_f64", "fb_system_scores", "fb_get_grad", "fb_attack", "fb_get_grad_wb", "fb_get_grad_wb_iter", "fb_set_wb_bpda", "fb_set_wb_ivector", "fb_set_wb_air", "fb_set_wb_frontend", "fb_set_wb_universal", "fb_get_grad_wb_from", "fb_attack_wb", "fb_attack_cw2", "fb_debug_cw2_step", "fb_attack_psy", "fb_debug_psy_loss", "fb_debug_psy_step", "fb_attack_pso", "fb_attack_kenansville", "fb_attack_hsj", "fb_hsj_max_rows", "fb_attack_pso_foreign", "fb_attack_kenansville_foreign", "fb_attack_hsj_foreign", "fb_debug_rows_to_model", "fb_debug_decide_foreign", "fb_attack_iter_seconds", "fb_get_grad_ext", "fb_attack_ext",
    "fb_get_grad_dev", "fb_attack_dev", "fb_debug_foreign_path", "fb_debug_nes_route", "fb_debug_nes_batch", "fb_debug_shared_chain_engines",
    "fb_estimate_threshold", "fb_debug_noise", "fb_debug_quantize", "fb_debug_mfcc", "fb_debug_feats", "fb_debug_dither_noise", "fb_debug_mfcc_dither", "fb_debug_feats_dither", "fb_debug_input_transform", "fb_debug_tf_noise", "fb_debug_input_transform_eot", "fb_debug_compose", "fb_debug_air_taps", "fb_debug_air_convolve", "fb_debug_codec", "fb_debug_feature_compress", "fb_debug_feco_keys", "fb_debug_pso_init", "fb_debug_pso_step", "fb_debug_kv_analyse", "fb_debug_kv_candidates", "fb_debug_hsj_line", "fb_debug_hsj_probes", "fb_debug_hsj_dir", "fb_debug_hsj_step", "fb_debug_vote", "fb_debug_gmm_frames", "fb_debug_gmm_acc_rows", "fb_debug_gmm_feat_grad", "fb_debug_frontend_vjp", "fb_debug_defence_vjp", "fb_debug_wb_route", "fb_debug_air_conv_t", "fb_debug_air_conv_t_chunk", "fb_debug_wb_air_route", "fb_debug_feature_compress_vjp", "fb_debug_wb_feco_route", "fb_debug_wb_feco_state", "fb_debug_wb_compose_t", "fb_debug_wb_universal_route", "fb_debug_iv_backend_grad", "fb_debug_iv_feat_grad", "fb_debug_iv_active", "fb_debug_iv_gselect", "fb_debug_frontend_route", "fb_debug_launch_shape", "fb_stats", "fb_gmm_acc_stats", "fb_last_ivectors", "fb_gmm_kernel_mode", "fb_gmm_kernel_variant", "fb_gmm_delta_tiles", "fb_gmm_delta_tiles_f6", "fb_set_fused_chain",
    "fb_debug_prepare_gmm", "fb_debug_prepare_ivector", "fb_debug_prepare_frontend",
    "fb_load_xvector", "fb_debug_prepare_xvector", "fb_debug_xv_embed", "fb_bench_xvector",
    "fb_set_wb_xvector", "fb_debug_xv_backward", "fb_debug_xv_masks", "fb_debug_wb_xv_route", "fb_bench_xv_backward",
    "fb_bench_gmm_kernel", "fb_bench_kv_kernels", "fb_bench_hsj_kernels", "fb_bench_vote", "fb_bench_foreign_rows", "fb_bench_nes", "fb_bench_nes_state",
]

ABI_VERSION = 101  # fb_version() of the library these bindings were written for (101: fb_set_wb_bpda, fb_get_grad_wb_iter)
# (the library is at 102 with fb_set_wb_ivector and at 103 with fb_set_wb_air and fb_set_wb_frontend; a library without them
#  fails the EXPORTS check above all the same; fb_set_wb_universal and fb_get_grad_wb_from came at 103 as well)

_lib = None


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libfakebob_hip: %s (code %d)" % (msg, code))
        self.code = code


def lib():
    """Load libfakebob_hip.so; raise loudly when it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libfakebob_hip.so not built: run `python -m fakebob_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback for the hot path")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    L.fb_last_error.restype = C.c_char_p
    L.fb_hsj_max_rows.restype = C.c_longlong
    for name in EXPORTS:
        getattr(L, name)  # AttributeError if the ABI is incomplete
    if L.fb_version() < ABI_VERSION:
        raise ImportError("libfakebob_hip.so is version %d, this package needs %d: rebuild it (`python -m fakebob_amd.build`)"
                          % (L.fb_version(), ABI_VERSION))
    _lib = L
    return L


def hip_runtimes():
    """The distinct libamdhip64 files this process has mapped (/proc/self/maps)."""
    paths = set()
    try:
        with open("/proc/self/maps") as r:
            for line in r:
                f = line.split(None, 5)
                if len(f) == 6 and os.path.basename(f[5].strip()).startswith("libamdhip64"):
                    paths.add(f[5].strip())
    except OSError:
        pass
    return sorted(paths)


def torch_first():
    """Import torch ahead of this library: the device path hands torch's device pointers and streams to the library, so
    both must run on ONE HIP runtime.  torch's wheel ships its own libamdhip64 under the soname the library links
    against, and whichever of the two loads first serves both.  Imported here, lazily: nothing else needs torch."""
    import torch
    return torch


def check_one_hip_runtime():
    """Raise when the process maps more than one libamdhip64: pointers and streams must not cross runtimes."""
    rt = hip_runtimes()
    if len(rt) > 1:
        raise RuntimeError("this process maps %d HIP runtimes (%s): torch and libfakebob_hip.so must share one.  Import "
                           "torch before the library is first loaded (fakebob_amd._native.torch_first())" %
                           (len(rt), ", ".join(rt)))


def check(rc):
    if rc != FB_OK:
        raise NativeError(rc, lib().fb_last_error().decode("utf-8", "replace"))


def ptr(a, t=C.c_void_p):
    return a.ctypes.data_as(t)
