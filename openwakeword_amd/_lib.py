"""ctypes binding of libowwhip.so (C ABI in include/owwhip.h).  Fails loudly when the library is
missing -- there is no CPU fallback in the product path."""
from __future__ import annotations

import ctypes as C
import os

from . import _build

_lib = None
ABI_VERSION = 6          # OWW_ABI_VERSION of include/owwhip.h this binding was written against
ERANGE = -5


class OwwError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_streams", C.c_int32), ("max_chunks", C.c_int32),
                ("feature_ring", C.c_int32), ("use_mfma", C.c_int32), ("debug_layers", C.c_int32),
                ("stream", C.c_void_p)]


class FitResult(C.Structure):
    """oww_fit_result (include/owwhip.h)"""
    _fields_ = [("status", C.c_int32), ("id", C.c_int32), ("n_pos", C.c_int32), ("n_neg", C.c_int32), ("iterations", C.c_int32),
                ("residual", C.c_float)]


FIT_MAX_N = 1024         # OWW_FIT_MAX_N
FIT_STATUS = ("OK", "ONE_CLASS", "BAD_N", "NONFINITE", "NOT_CONVERGED")      # OWW_FIT_*


class TrainRecord(C.Structure):
    """oww_train_record (include/owwhip.h)"""
    _fields_ = [("loss", C.c_float), ("m", C.c_int32)]


TRAIN_MAX_BATCH = 4096   # OWW_TRAIN_MAX_BATCH
TRAIN_MAX_STEPS = 4096   # OWW_TRAIN_MAX_STEPS
TRAIN_EVAL_MAX_ROWS = 1 << 20   # OWW_TRAIN_EVAL_MAX_ROWS


class IngestClass(C.Structure):
    """oww_ingest_class (include/owwhip.h)"""
    _fields_ = [("encoding", C.c_int32), ("p", C.c_int32), ("q", C.c_int32), ("n_taps", C.c_int32), ("taps", C.c_void_p)]


INGEST_MAX_CLASSES = 16  # OWW_INGEST_MAX_CLASSES

# every symbol include/owwhip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "oww_abi_version": (C.c_int, []),
    "oww_build_info": (C.c_char_p, []),
    "oww_last_error": (C.c_char_p, []),
    "oww_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "oww_destroy": (C.c_int, [_P]),
    "oww_load_mel": (C.c_int, [_P, _P, C.c_size_t]),
    "oww_load_embedding": (C.c_int, [_P, _P, C.c_size_t]),
    "oww_add_head": (C.c_int, [_P, _P, C.c_size_t]),
    "oww_commit": (C.c_int, [_P]),
    "oww_set_calibration": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "oww_calibration_info": (C.c_int, [_P, _P, _P, _P, _P]),
    "oww_n_labels": (C.c_int, [_P]),
    "oww_reset": (C.c_int, [_P, _P, C.c_int32, _P]),
    "oww_set_postproc": (C.c_int, [_P, _P, _P, C.c_int32]),
    "oww_step": (C.c_int, [_P, _P, C.c_int, C.c_int32, _P, C.c_int]),
    "oww_step_masked": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_int]),
    "oww_sync": (C.c_int, [_P]),
    "oww_range_status": (C.c_int, [_P, C.c_int]),
    "oww_range_where": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "oww_submit": (C.c_int, [_P, _P, C.c_int32]),
    "oww_submit_masked": (C.c_int, [_P, _P, _P]),
    "oww_collect": (C.c_int, [_P, _P]),
    "oww_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "oww_host_free": (C.c_int, [_P]),
    "oww_set_verifier": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.c_float, C.c_float]),
    "oww_set_vad_threshold": (C.c_int, [_P, C.c_float]),
    "oww_push_vad": (C.c_int, [_P, _P, C.c_int]),
    "oww_load_vad": (C.c_int, [_P, _P, C.c_size_t]),
    "oww_get_vad": (C.c_int, [_P, _P]),
    "oww_reset_vad": (C.c_int, [_P, _P, C.c_int32]),
    "oww_scores_dev": (_P, [_P]),
    "oww_get_raw": (C.c_int, [_P, _P]),
    "oww_resample": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int, C.c_int32]),
    "oww_ingest_configure": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    "oww_ingest": (C.c_int, [_P, _P, C.c_int, C.c_int32, _P, C.c_int, _P, C.c_int]),
    "oww_ingest_dev": (_P, [_P]),
    "oww_step_ingest": (C.c_int, [_P, _P, C.c_int, C.c_int32, _P, C.c_int, _P, C.c_int]),
    "oww_ingest_configure_classes": (C.c_int, [_P, C.c_int32, C.POINTER(IngestClass)]),
    "oww_ingest_assign": (C.c_int, [_P, _P, C.c_int32, _P]),
    "oww_ingest_mixed": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int32, _P, C.c_int, _P, C.c_int]),
    "oww_step_ingest_mixed": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int32, _P, C.c_int, _P, C.c_int]),
    "oww_submit_ingest_mixed": (C.c_int, [_P, _P, C.c_int64, _P]),
    "oww_mel": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "oww_mel_clips": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "oww_embed": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "oww_embed_clips": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    "oww_head": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P]),
    "oww_score_shape": (C.c_int, [_P, C.c_int32, _P, _P]),
    "oww_score_features": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int32, _P, C.c_int]),
    "oww_score_clips": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int32, _P, C.c_int, _P, C.c_int]),
    "oww_bank_score_shape": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "oww_bank_score_features": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int]),
    "oww_bank_score_stats": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P]),
    "oww_score_hits_layout": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "oww_score_hits": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, C.c_int]),
    "oww_score_clip_hits": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, C.c_int]),
    "oww_bank_score_hits": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, C.c_int]),
    "oww_get_features": (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    "oww_get_mel": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "oww_debug_read": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "oww_debug_profile": (C.c_int, [_P, _P, C.c_int32]),
    "oww_enable_timing": (C.c_int, [_P, C.c_int]),
    "oww_kernel_times": (C.c_int, [_P, _P, _P]),
    "oww_use_graph": (C.c_int, [_P, C.c_int]),
    "oww_bank_configure": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "oww_bank_add": (C.c_int, [_P, _P, C.c_size_t]),
    "oww_bank_remove": (C.c_int, [_P, C.c_int32]),
    "oww_bank_set_postproc": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_float]),
    "oww_subscribe": (C.c_int, [_P, _P, C.c_int32, _P]),
    "oww_bank_scores": (C.c_int, [_P, _P]),
    "oww_bank_scores_dev": (_P, [_P]),
    "oww_bank_routing": (C.c_int, [_P, _P, _P]),
    "oww_verifier_configure": (C.c_int, [_P, C.c_int32]),
    "oww_verifier_add": (C.c_int, [_P, _P, C.c_int32, C.c_float]),
    "oww_verifier_remove": (C.c_int, [_P, C.c_int32]),
    "oww_assign_verifiers": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P]),
    "oww_bank_assign_verifiers": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P]),
    "oww_verifier_stats": (C.c_int, [_P, _P]),
    "oww_verifier_fit": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int32, C.c_int32, C.c_float, C.POINTER(FitResult)]),
    "oww_verifier_get": (C.c_int, [_P, C.c_int32, _P, C.c_int32, C.POINTER(C.c_float)]),
    "oww_train_param_count": (C.c_int64, [C.c_int32, C.c_int32]),
    "oww_train_begin": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "oww_train_set_pool": (C.c_int, [_P, _P, C.c_int, C.c_int64]),
    "oww_train_steps": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int, C.c_int, _P, _P, _P]),
    "oww_train_get": (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    "oww_train_end": (C.c_int, [_P]),
    "oww_train_new_sequence": (C.c_int, [_P]),
    "oww_train_set_eval_pool": (C.c_int, [_P, _P, C.c_int, C.c_int64]),
    "oww_train_eval": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int, C.c_int, _P, _P]),
    "oww_train_checkpoints": (C.c_int, [_P, C.c_int32]),
    "oww_train_snapshot": (C.c_int, [_P, _P]),
    "oww_train_average": (C.c_int, [_P, _P, C.c_int32]),
    "oww_train_get_slot": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int64]),
    "oww_state_info": (C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "oww_state_export": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int]),
    "oww_state_import": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int]),
    "oww_move_streams": (C.c_int, [_P, _P, _P, C.c_int32]),
    "oww_events_configure": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "oww_events_set_thresholds": (C.c_int, [_P, _P, C.c_float]),
    "oww_get_events": (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "oww_get_event_features": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int]),
    "oww_events_dev": (_P, [_P, C.POINTER(_P)]),
    "oww_event_features_dev": (_P, [_P]),
    "oww_audio_configure": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "oww_get_audio": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int, _P]),
    "oww_get_event_audio": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int]),
    "oww_event_audio_dev": (_P, [_P]),
    "oww_comm_id": (C.c_int, [_P]),
    "oww_comm_init": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "oww_gather_scores": (C.c_int, [_P, _P, _P]),
    "oww_comm_count": (C.c_int, [_P, _P]),
    "oww_comm_destroy": (C.c_int, [_P]),
}


def load():
    """dlopen libowwhip.so once.  torch is imported first when available so that the HIP runtime
    torch bundles (soname libamdhip64.so.7) is the one and only runtime in the process."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.lib_path()
    if not os.path.exists(path):
        raise OwwError(f"{path} is missing: build it with `python -m openwakeword_amd._build` "
                       "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    if lib.oww_abi_version() != ABI_VERSION:
        raise OwwError("libowwhip.so ABI version mismatch")
    _lib = lib
    return lib


class OwwRangeError(OwwError):
    """OWW_ERANGE: an activation left the f16 range of the fp16-split kernels (sticky per handle)."""


def check(rc: int) -> int:
    if rc == ERANGE:
        raise OwwRangeError(f"libowwhip error {rc}: {load().oww_last_error().decode(errors='replace')}")
    if rc < 0:
        raise OwwError(f"libowwhip error {rc}: {load().oww_last_error().decode(errors='replace')}")
    return rc
