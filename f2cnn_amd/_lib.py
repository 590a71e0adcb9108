"""ctypes binding of libf2cnn_hip.so (C ABI: include/f2cnn_hip.h).

There is no CPU fallback: if the library is missing it is built with hipcc; if that fails, or no
gfx950 device is present when a context is requested, an exception is raised.
"""
import ctypes as C
import importlib.util
import os
import sys
import threading

import numpy as np

from . import build as _build

F2_OK, F2_ERR_INVALID, F2_ERR_HIP, F2_ERR_UNSUPPORTED, F2_ERR_NOMEM, F2_ERR_NONPOSITIVE = 0, -1, -2, -3, -4, -5
CNN_ROUTES = {"call": 0, "f32": 1, "tile": 2, "ws": 3, "ws_dense": 4, "recorded": 5}   # F2_CNN_ROUTE_* of f2_cnn_layers
MEM_HOST, MEM_DEVICE, MEM_HOST_ASYNC = 0, 1, 2
WAVE_I16, WAVE_F64 = 0, 1
FFT_F32, FFT_F64 = 0, 1
PCM_U8, PCM_I16, PCM_I32, PCM_F32, PCM_F64 = 0, 1, 2, 3, 4
K_COUNT = 7
# tile constants of k_reverb_levels (csrc/f2_internal.h: F2_REVERB_BLOCK outputs per workgroup, F2_REVERB_TAP_CHUNK taps per staged
# span) and the longest impulse response f2_reverb_levels takes (F2_REVERB_MAX_TAPS)
REVERB_BLOCK, REVERB_TAP_CHUNK, REVERB_MAX_TAPS = 1024, 1024, 32768
# tile constants of k_channel_mix_levels (csrc/f2_internal.h: F2_SMEAR_TILE_SAMPLES samples by F2_SMEAR_TILE_CHANNELS output channels
# per workgroup) and the most channels and levels f2_channel_mix_levels takes (F2_SMEAR_MAX_CHANNELS, F2_SMEAR_MAX_LEVELS)
SMEAR_TILE_SAMPLES, SMEAR_TILE_CHANNELS, SMEAR_MAX_CHANNELS, SMEAR_MAX_LEVELS = 512, 16, 512, 64
# tile constant of k_shaped_noise_levels (csrc/f2_internal.h: F2_SHAPED_BLOCK outputs per workgroup) and the longest filter and the most
# levels f2_shaped_noise_levels takes (F2_SHAPED_MAX_TAPS, F2_SHAPED_MAX_LEVELS)
SHAPED_BLOCK, SHAPED_MAX_TAPS, SHAPED_MAX_LEVELS = 1024, 2048, 64
# the most recordings and levels the masker calls take and the longest recording (csrc/f2_internal.h: F2_MASKER_MAX_RECORDINGS,
# F2_MASKER_MAX_LEVELS, F2_MASKER_MAX_SAMPLES), the threads of their fixed-order sum, and the second counter word of the segment draw
MASKER_MAX_RECORDINGS, MASKER_MAX_LEVELS, MASKER_MAX_SAMPLES, MASKER_SUM_THREADS, MASKER_STREAM = 64, 64, 1 << 26, 1024, 0x4D41534B
# the decoding kernels of f2_decision_path (include/f2cnn_hip.h): F2_PATH_TILE rows per workgroup, F2_PATH_SCAN_CHUNK tile products per
# step of the per-utterance scans; the largest logit_scale and penalty the call takes
PATH_TILE, PATH_SCAN_CHUNK, PATH_MAX_SCALE, PATH_MAX_PENALTY = 1024, 256, float(1 << 20), 1 << 40

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_P = C.POINTER

# name -> (restype, argtypes); mirrors include/f2cnn_hip.h one to one
SIGNATURES = {
    "f2_version": (_i, []),
    "f2_device_count": (_i, [_P(_i)]),
    "f2_ctx_create": (_i, [_i, _P(_vp)]),
    "f2_ctx_destroy": (_i, [_vp]),
    "f2_ctx_synchronize": (_i, [_vp]),
    "f2_ctx_set_stream": (_i, [_vp, _vp]),
    "f2_ctx_get_stream": (_vp, [_vp]),
    "f2_last_error": (C.c_char_p, [_vp]),
    "f2_ctx_set_option": (_i, [_vp, C.c_char_p, _d]),
    "f2_ctx_get_option": (_i, [_vp, C.c_char_p, _P(_d)]),
    "f2_spectral_guard_read": (_i, [_vp, _vp, _i64, _P(_i64)]),
    "f2_dev_malloc": (_i, [_vp, C.c_size_t, _P(_vp)]),
    "f2_dev_free": (_i, [_vp, _vp]),
    "f2_dev_memset": (_i, [_vp, _vp, _i, C.c_size_t]),
    "f2_host_alloc": (_i, [_vp, C.c_size_t, _P(_vp)]),
    "f2_host_free": (_i, [_vp, _vp]),
    "f2_memcpy_h2d": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "f2_memcpy_d2h": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "f2_event_create": (_i, [_vp, _P(_vp)]),
    "f2_event_destroy": (_i, [_vp, _vp]),
    "f2_event_record": (_i, [_vp, _vp]),
    "f2_event_elapsed_ms": (_i, [_vp, _vp, _vp, _P(C.c_float)]),
    "f2_event_query": (_i, [_vp, _vp, _P(C.c_int)]),
    "f2_prof_enable": (_i, [_vp, _i]),
    "f2_prof_reset": (_i, [_vp]),
    "f2_prof_get": (_i, [_vp, _i, _P(_i), _P(C.c_float)]),
    "f2_prof_kernel_name": (C.c_char_p, [_i]),
    "f2_erb_filterbank_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i]),
    "f2_envelope_batch": (_i, [_vp, _vp, _vp, _i, _i, _i, _d, _i, _vp, _i]),
    "f2_filterbank_envelope_fused": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i]),
    "f2_gather_windows": (_i, [_vp, _vp, _i, _i64, _vp, _i64, _i, _i, _i, _vp, _i]),
    "f2_input_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i, _i, _i, _vp, _i]),
    "f2_cnn_create": (_i, [_vp, _P(_vp), _i, _i, _P(_vp)]),
    "f2_cnn_destroy": (_i, [_vp, _vp]),
    "f2_cnn_get_info": (_i, [_vp, _vp, C.c_char_p, _P(_d)]),
    "f2_cnn_forward": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _i]),
    "f2_eval_utterance": (_i, [_vp, _vp, _vp, _i, _i64, _vp, _i, _i, _d, _i, _i, _i, _vp, _vp, _vp, _P(_i64), _i]),
    "f2_eval_batch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _vp, _vp, _i]),
    "f2_eval_batch_strided": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _vp, _vp, _i]),
    "f2_eval_noise_sweep": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _i, C.c_uint64, _vp, _vp, _vp,
                                 _vp, _vp, _vp, _i]),
    "f2_label_accuracy": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i64, _i, _i, _vp, _i]),
    "f2_cnn_score_windows": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i]),
    "f2_envelope_picture": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _i]),
    "f2_gammatonegram_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _i, _i, _vp, _vp, _vp, _i]),
    "f2_resample_batch": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i64, _i64, _vp, _i64, _vp, _vp, _i]),
    "f2_score_track": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i64, _i, _i, _vp, _i]),
    "f2_eval_figure_batch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _i]),
    "f2_occlude_windows": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i, C.c_float, _vp, _i]),
    "f2_occlusion_map": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i64, _i, _i, _vp, _i]),
    "f2_eval_occlusion_batch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _i, C.c_float, _vp, _i, _i, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "f2_cnn_input_gradient": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i]),
    "f2_cnn_layers": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _vp, _i]),
    "f2_saliency_map": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i64, _i, _i, _vp, _i]),
    "f2_eval_saliency_batch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _i]),
    "f2_lowpass_levels": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i]),
    "f2_eval_cutoff_sweep": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "f2_reverb_levels": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i]),
    "f2_eval_reverb_sweep": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                  _i]),
    "f2_channel_mix_levels": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i]),
    "f2_eval_smear_sweep": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i]),
    "f2_cnn_loss_gradient": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _i]),
    "f2_trainer_create": (_i, [_vp, _P(_vp), _i, _i, _d, _d, _d, _d, _vp, C.c_uint64, _P(_vp)]),
    "f2_trainer_destroy": (_i, [_vp, _vp]),
    "f2_trainer_set_data": (_i, [_vp, _vp, _vp, _vp, _i64]),
    "f2_trainer_steps": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp]),
    "f2_trainer_get": (_i, [_vp, _vp, _i, _P(_vp)]),
    "f2_trainer_get_info": (_i, [_vp, _vp, C.c_char_p, _P(_d)]),
    "f2_noise_pick": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, C.c_uint32, C.c_uint64, _vp, _vp, _i]),
    "f2_input_batch_noisy": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, C.c_uint32, C.c_uint64,
                                  _vp, _i]),
    "f2_trainer_set_waves": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _vp, _i, _i, _i]),
    "f2_trainer_render": (_i, [_vp, _vp, _vp, _i, _vp, C.c_uint64]),
    "f2_trainer_get_windows": (_i, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "f2_reverb_pick": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i]),
    "f2_input_batch_wet": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp,
                                C.c_uint32, C.c_uint64, _vp, _i]),
    "f2_trainer_render_wet": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, C.c_uint64]),
    "f2_shaped_noise_levels": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, C.c_uint64, _vp, _vp, _i]),
    "f2_eval_shaped_noise_sweep": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _vp, _vp, _i, C.c_uint64, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _i]),
    "f2_shaped_noise_pick": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, C.c_uint32, C.c_uint64, _vp, _vp, _i]),
    "f2_input_batch_coloured": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                     _i, _vp, C.c_uint32, C.c_uint64, _vp, _i]),
    "f2_trainer_render_coloured": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, C.c_uint64]),
    "f2_gather_windows_mixed": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i]),
    "f2_input_batch_smeared": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                    _i, _vp, C.c_uint32, C.c_uint64, _vp, _i, _vp, _vp, _i]),
    "f2_trainer_render_smeared": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, C.c_uint64, _vp, _i, _vp]),
    "f2_masker_levels": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, C.c_uint64, _vp, _vp, _vp, _vp, _i]),
    "f2_eval_masker_sweep": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, C.c_uint64, _vp,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "f2_masker_pick": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, C.c_uint32, C.c_uint64, _vp, _vp, _vp, _vp, _i]),
    "f2_input_batch_masked": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                   _i, _vp, C.c_uint32, C.c_uint64, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i]),
    "f2_trainer_render_masked": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, C.c_uint64, _vp, _i, _vp, _vp, _vp, _vp, _i,
                                      _vp, _i, _vp]),
    "f2_lowpass_pick": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i]),
    "f2_input_batch_filtered": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp,
                                     _i, _vp, C.c_uint32, C.c_uint64, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp,
                                     _i]),
    "f2_trainer_render_filtered": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, C.c_uint64, _vp, _i, _vp, _vp, _vp, _vp, _i,
                                        _vp, _i, _vp, _vp, _i, _vp]),
    "f2_decision_path": (_i, [_vp, _vp, _vp, _i, _d, _i64, _vp, _vp, _vp, _i]),
    "f2_decision_runs": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i64, _i]),
    "f2_interval_tally": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i64, _i, _vp, _i]),
    "f2_eval_segments_batch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _i, _i, _d, _i64, _vp, _vp, _i, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _i]),
}
TRAINER_WHAT = {"weights": 0, "accumulators": 1, "gradient": 2}   # F2_TRAINER_* of f2_trainer_get

_lib = None
_lock = threading.Lock()


class F2Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libf2cnn_hip error {code}: {msg}")
        self.code = code


def library_path():
    return _build.LIB_PATH


def _share_hip_runtime_with_torch():
    """A process can hold one HIP runtime. PyTorch-ROCm ships its own libamdhip64.so.7 (same SONAME as the system
    one this library is linked against), and whichever loads first serves both: with the system runtime loaded first,
    a later `import torch` (bench.py's process group, `cnn train`) finds no usable device. So when torch is installed
    its runtime is mapped first, whatever the import order. F2CNN_HIP_RUNTIME=system skips this."""
    if os.environ.get("F2CNN_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        cand = os.path.join(libdir, name)
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def load(build_if_missing=True):
    """dlopen the library (building it first if it is absent) and declare every signature."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.exists(path):
            if not build_if_missing:
                raise FileNotFoundError(f"{path} is missing: run `python -m f2cnn_amd.build` (needs hipcc)")
            _build.build_library()
        _share_hip_runtime_with_torch()
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                if os.environ.get("F2CNN_PROBE_OLD_LIB") == "1":   # tools/ab_old_new.sh: an older build beside the tree's
                    continue
                raise
            fn.restype, fn.argtypes = res, args
        _lib = lib
        return lib


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a  # int device pointer


def _want_array(a, dtype, size, name):
    """A numpy output (device pointers and None pass): contiguous, of this dtype, with room for `size` elements."""
    if isinstance(a, np.ndarray) and (a.dtype != dtype or a.size < size or not a.flags["C_CONTIGUOUS"]):
        raise ValueError(f"{name} must be contiguous {np.dtype(dtype).name} with room for {size} elements")


class _PinnedOwner:
    def __init__(self, ctx, ptr):
        self.ctx, self.ptr = ctx, ptr

    def __del__(self):
        try:
            if self.ctx.handle and self.ptr:
                self.ctx.lib.f2_host_free(self.ctx.handle, self.ptr)
        except Exception:
            pass


class Context:
    """One f2_ctx: a device, a stream and its scratch memory. Not thread-safe (one host thread per context)."""

    def __init__(self, device=0):
        self.lib = load()
        h = _vp()
        rc = self.lib.f2_ctx_create(int(device), C.byref(h))
        if rc != F2_OK:
            raise F2Error(rc, self.lib.f2_last_error(None).decode())
        self.handle = h
        self.device = int(device)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.f2_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != F2_OK:
            raise F2Error(rc, self.lib.f2_last_error(self.handle).decode())

    # ---- plumbing ----
    def synchronize(self):
        self.check(self.lib.f2_ctx_synchronize(self.handle))

    def set_stream(self, stream_ptr):
        self.check(self.lib.f2_ctx_set_stream(self.handle, stream_ptr))

    def set_option(self, key, value):
        """Per-context tuning switch (include/f2cnn_hip.h: f2_ctx_set_option); returns the previous value."""
        old = self.get_option(key)
        self.check(self.lib.f2_ctx_set_option(self.handle, key.encode(), float(value)))
        return old

    def get_option(self, key):
        v = _d()
        self.check(self.lib.f2_ctx_get_option(self.handle, key.encode(), C.byref(v)))
        return v.value

    def spectral_guard_values(self):
        """(rows, 4) float32 {row max, padding residual, low-passed row max, flagged} of the last fused call made with option
        spectral_guard_dump = 1, rows in (utterance, channel) batch order; NaN rows were not served by the spectral kernel."""
        avail = _i64()
        self.check(self.lib.f2_spectral_guard_read(self.handle, None, 0, C.byref(avail)))
        out = np.empty((avail.value, 4), np.float32)
        if avail.value:
            self.check(self.lib.f2_spectral_guard_read(self.handle, out.ctypes.data, avail.value, None))
        return out

    def options(self, **kv):
        """Context manager: set the given options, restore the previous values on exit."""
        ctx = self

        class _Scope:
            def __enter__(self_inner):
                self_inner.old = {k: ctx.set_option(k, v) for k, v in kv.items()}
                return ctx

            def __exit__(self_inner, *exc):
                for k, v in self_inner.old.items():
                    ctx.set_option(k, v)
                return False

        return _Scope()

    def malloc(self, nbytes):
        p = _vp()
        self.check(self.lib.f2_dev_malloc(self.handle, int(nbytes), C.byref(p)))
        return p.value or 0

    def free(self, dptr):
        self.check(self.lib.f2_dev_free(self.handle, dptr))

    def host_alloc(self, nbytes):
        """Page-locked host buffer of nbytes: a ctypes byte array (buffer protocol) that frees itself when collected."""
        p = _vp()
        self.check(self.lib.f2_host_alloc(self.handle, int(nbytes), C.byref(p)))
        buf = (C.c_ubyte * int(nbytes)).from_address(p.value)
        buf._f2_owner = _PinnedOwner(self, p.value)
        return buf

    def memset(self, dptr, value, nbytes):
        self.check(self.lib.f2_dev_memset(self.handle, dptr, value, int(nbytes)))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.check(self.lib.f2_memcpy_h2d(self.handle, dptr, arr.ctypes.data, arr.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        self.check(self.lib.f2_memcpy_d2h(self.handle, arr.ctypes.data, dptr, arr.nbytes))

    def event(self):
        e = _vp()
        self.check(self.lib.f2_event_create(self.handle, C.byref(e)))
        return e

    def record(self, ev):
        self.check(self.lib.f2_event_record(self.handle, ev))

    def elapsed_ms(self, e0, e1):
        ms = C.c_float()
        self.check(self.lib.f2_event_elapsed_ms(self.handle, e0, e1, C.byref(ms)))
        return ms.value

    def event_done(self, ev):
        """True once the stream has passed the event (does not wait)."""
        done = C.c_int()
        self.check(self.lib.f2_event_query(self.handle, ev, C.byref(done)))
        return bool(done.value)

    def destroy_event(self, ev):
        self.check(self.lib.f2_event_destroy(self.handle, ev))

    def prof_enable(self, on=True):
        self.check(self.lib.f2_prof_enable(self.handle, int(on)))

    def prof_get(self):
        """{kernel name: (launches, total_ms)} since profiling was enabled/reset; waits for the stream."""
        out = {}
        for k in range(K_COUNT):
            n, ms = _i(), C.c_float()
            self.check(self.lib.f2_prof_get(self.handle, k, C.byref(n), C.byref(ms)))
            if n.value:
                out[self.lib.f2_prof_kernel_name(k).decode()] = (n.value, ms.value)
        return out

    def prof_reset(self):
        self.check(self.lib.f2_prof_reset(self.handle))

    # ---- ops (data pointers: numpy arrays with mem_space HOST, or int device pointers) ----
    def erb_filterbank_batch(self, wave, wave_dtype, offsets, coefs, B, Cn, gfb, mem_space):
        self.check(self.lib.f2_erb_filterbank_batch(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs),
                                                    B, Cn, _ptr(gfb), mem_space))

    def envelope_batch(self, gfb, offsets, B, Cn, lpf, cutoff, precision, env, mem_space):
        self.check(self.lib.f2_envelope_batch(self.handle, _ptr(gfb), _ptr(offsets), B, Cn, int(bool(lpf)),
                                              float(cutoff), precision, _ptr(env), mem_space))

    def filterbank_envelope_fused(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, env, gfb,
                                  mem_space):
        self.check(self.lib.f2_filterbank_envelope_fused(self.handle, _ptr(wave), wave_dtype, _ptr(offsets),
                                                         _ptr(coefs), B, Cn, int(bool(lpf)), float(cutoff), precision,
                                                         _ptr(env), _ptr(gfb), mem_space))

    def gather_windows(self, env, Cn, N, centers, n_windows, radius, step, normalize, out, mem_space):
        self.check(self.lib.f2_gather_windows(self.handle, _ptr(env), Cn, N, _ptr(centers), n_windows, radius, step,
                                              int(bool(normalize)), _ptr(out), mem_space))

    def input_batch(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, center_offsets, centers, radius,
                    step, normalize, windows, mem_space):
        """Ragged batch of waves -> (center_offsets[B], 2*radius+1, Cn) float32 windows at the given centres (each relative
        to its own utterance), the envelopes never leaving the device; see f2_input_batch."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        center_offsets = np.ascontiguousarray(center_offsets, dtype=np.int64)
        centers = np.ascontiguousarray(centers, dtype=np.int64)
        self.check(self.lib.f2_input_batch(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn,
                                           int(bool(lpf)), float(cutoff), precision, _ptr(center_offsets), _ptr(centers),
                                           radius, step, int(bool(normalize)), _ptr(windows), mem_space))

    def noise_pick(self, wave, wave_dtype, offsets, B, snr_db, level_of, first_utterance, seed, noisy, mem_space, sigma=None):
        """The batch with one noise level per utterance (see f2_noise_pick): utterance b at snr_db[level_of[b]], or clean where
        level_of[b] == len(snr_db); level_of None: all clean. wave / noisy are numpy arrays or device pointers, by mem_space.
        sigma: True for a new (B) float64 array, an array to fill, or None. Returns sigma (or None)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        snr, lev = _noise_levels(snr_db, level_of)
        if sigma is True:
            sigma = np.zeros(int(B), np.float64)
        self.check(self.lib.f2_noise_pick(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), int(B), _ptr(snr) if len(snr) else None,
                                          len(snr), _ptr(lev), int(first_utterance), int(seed) & (2 ** 64 - 1), _ptr(noisy), _ptr(sigma),
                                          mem_space))
        return sigma

    def _input_batch_staged(self, name, v):
        """f2_input_batch_<name> from the arguments `v` of its method: input_batch's, with that symbol's stage arguments before `windows`"""
        offsets, center_offsets, centers = (np.ascontiguousarray(v[k], dtype=np.int64) for k in ("offsets", "center_offsets", "centers"))
        args, alive = _stage_args(_STAGE_KEYS[name], v)
        self.check(getattr(self.lib, "f2_input_batch_" + name)(
            self.handle, _ptr(v["wave"]), v["wave_dtype"], _ptr(offsets), _ptr(v["coefs"]), int(v["B"]), v["Cn"], int(bool(v["lpf"])),
            float(v["cutoff"]), v["precision"], _ptr(center_offsets), _ptr(centers), v["radius"], v["step"], int(bool(v["normalize"])),
            *args, _ptr(v["windows"]), v["mem_space"]))

    def input_batch_noisy(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, center_offsets, centers, radius,
                          step, normalize, snr_db, level_of, first_utterance, seed, windows, mem_space):
        """input_batch on the batch as noise_pick leaves it, the noisy waveform never leaving the device; see
        f2_input_batch_noisy."""
        self._input_batch_staged("noisy", locals())

    def reverb_pick(self, wave, wave_dtype, offsets, B, rirs, room_of, wet, mem_space):
        """The batch with one room per utterance (see f2_reverb_pick): utterance b convolved with rirs[room_of[b]] (a sequence of
        1-D float64 arrays), or dry where room_of[b] == len(rirs); room_of None: all dry. wet receives offsets[B] float64 in the
        layout of wave (numpy arrays or device pointers, by mem_space)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        taps, rir_offsets, room = _rooms(rirs, room_of)
        self.check(self.lib.f2_reverb_pick(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), int(B), _ptr(taps) if len(taps) else None,
                                           _ptr(rir_offsets), len(rir_offsets) - 1, _ptr(room), _ptr(wet), mem_space))

    def input_batch_wet(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, center_offsets, centers, radius, step,
                        normalize, rirs, room_of, snr_db, level_of, first_utterance, seed, windows, mem_space):
        """input_batch on the batch as reverb_pick, then noise_pick leave it, neither waveform leaving the device; see
        f2_input_batch_wet."""
        self._input_batch_staged("wet", locals())

    def shaped_noise_pick(self, wave, wave_dtype, offsets, B, snr_db, firs, level_of, first_utterance, seed, noisy, mem_space,
                          sigma=None):
        """The batch with one coloured-noise level per utterance (see f2_shaped_noise_pick): utterance b at snr_db[level_of[b]]
        under the filter firs[level_of[b]] (a sequence of 1-D float64 arrays, one per level, always host arrays; None: no taps are
        handed over), or clean where level_of[b] == len(snr_db); level_of None: all clean. wave / noisy are numpy arrays or device
        pointers, by mem_space. sigma: True for a new (B) float64 array, an array to fill, or None. Returns sigma (or None)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        snr, lev = _noise_levels(snr_db, level_of)
        taps, fir_offsets = _colours(firs, len(snr))
        if sigma is True:
            sigma = np.zeros(int(B), np.float64)
        self.check(self.lib.f2_shaped_noise_pick(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), int(B),
                                                 _ptr(snr) if len(snr) else None, _ptr(taps), _ptr(fir_offsets), len(snr), _ptr(lev),
                                                 int(first_utterance), int(seed) & (2 ** 64 - 1), _ptr(noisy), _ptr(sigma), mem_space))
        return sigma

    def input_batch_coloured(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, center_offsets, centers, radius,
                             step, normalize, rirs, room_of, snr_db, firs, level_of, first_utterance, seed, windows, mem_space):
        """input_batch on the batch as reverb_pick, then shaped_noise_pick leave it, neither waveform leaving the device; firs None:
        input_batch_wet. See f2_input_batch_coloured."""
        self._input_batch_staged("coloured", locals())

    def gather_windows_mixed(self, env, offsets, B, Cn, center_offsets, centers, radius, step, normalize, mixes, mix_of, windows,
                             mem_space):
        """The ragged gather of input_batch on envelopes that are already in memory, the channels of utterance b's windows mixed
        by mixes[mix_of[b]] ((K, Cn, Cn) float64, always a host array) before the normaliser, or sharp where mix_of[b] == K;
        mixes None or mix_of None: all sharp. env holds the ragged (Cn, n_b) float64 blocks, windows receives
        (center_offsets[B], 2 * radius + 1, Cn) float32 (numpy arrays or device pointers, by mem_space). See
        f2_gather_windows_mixed."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        center_offsets = np.ascontiguousarray(center_offsets, dtype=np.int64)
        centers = np.ascontiguousarray(centers, dtype=np.int64)
        mix, mlev = _smears(mixes, mix_of, Cn)
        self.check(self.lib.f2_gather_windows_mixed(self.handle, _ptr(env), _ptr(offsets), int(B), int(Cn), _ptr(center_offsets),
                                                    _ptr(centers), radius, step, int(bool(normalize)),
                                                    _ptr(mix) if len(mix) else None, len(mix), _ptr(mlev), _ptr(windows), mem_space))

    def input_batch_smeared(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, center_offsets, centers, radius,
                            step, normalize, rirs, room_of, snr_db, firs, level_of, first_utterance, seed, mixes, mix_of, windows,
                            mem_space):
        """input_batch_coloured whose gather is gather_windows_mixed: room, noise, envelopes, then the windows of utterance b
        through mixes[mix_of[b]], nothing leaving the device; mixes None: input_batch_coloured. See f2_input_batch_smeared."""
        self._input_batch_staged("smeared", locals())

    def input_batch_masked(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, center_offsets, centers, radius,
                           step, normalize, rirs, room_of, snr_db, firs, level_of, first_utterance, seed, mixes, mix_of, maskers,
                           masker_of, masker_snrs, masker_level_of, windows, mem_space):
        """input_batch_smeared with a recorded masker per utterance between the room and the noise: utterance b under the recording
        maskers[masker_of[l]] at masker_snrs[l], l = masker_level_of[b], or none where l == len(masker_snrs); maskers None:
        input_batch_smeared. See f2_input_batch_masked."""
        self._input_batch_staged("masked", locals())

    def input_batch_filtered(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, center_offsets, centers, radius,
                             step, normalize, rirs, room_of, snr_db, firs, level_of, first_utterance, seed, mixes, mix_of, maskers,
                             masker_of, masker_snrs, masker_level_of, cutoffs, cutoff_of, windows, mem_space):
        """input_batch_masked with an envelope cutoff per utterance between the envelopes and the gather: the unfiltered envelopes
        of utterance b low-passed at cutoffs[cutoff_of[b]] Hz, or left as they are where cutoff_of[b] == len(cutoffs); cutoffs
        empty or cutoff_of None: input_batch_masked. The stage excludes lpf. See f2_input_batch_filtered."""
        self._input_batch_staged("filtered", locals())

    def lowpass_pick(self, env, offsets, B, Cn, cutoffs, cutoff_of, filtered, mem_space):
        """Envelopes that are already in memory with one cutoff per utterance (see f2_lowpass_pick): utterance b low-passed at
        cutoffs[cutoff_of[b]] Hz, or copied where cutoff_of[b] == len(cutoffs); cutoff_of None: all copied. filtered receives
        Cn * offsets[B] float64 in the layout of env (numpy arrays or device pointers, by mem_space); in device memory it may be
        env itself."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        cut, lev = _cutoff_levels(cutoffs, cutoff_of)
        self.check(self.lib.f2_lowpass_pick(self.handle, _ptr(env), _ptr(offsets), int(B), int(Cn), _ptr(cut) if len(cut) else None,
                                            len(cut), _ptr(lev), _ptr(filtered), mem_space))

    def masker_pick(self, wave, wave_dtype, offsets, B, snr_db, maskers, masker_of, level_of, first_utterance, seed, noisy, mem_space,
                    small=False):
        """The batch with one masker level per utterance (see f2_masker_pick): utterance b under the recording maskers[masker_of[l]]
        (a sequence of 1-D float64 arrays, always host arrays) at snr_db[l], l = level_of[b], or clean where l == len(snr_db);
        level_of None: all clean. wave / noisy are numpy arrays or device pointers, by mem_space. small: also return (sigma, gain,
        start), B values each."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        snr, lev = _noise_levels(snr_db, level_of)
        samples, moff, mof = _maskers(maskers, masker_of, len(snr))
        out = (np.zeros(int(B), np.float64), np.zeros(int(B), np.float64), np.zeros(int(B), np.int64)) if small else (None, None, None)
        self.check(self.lib.f2_masker_pick(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), int(B), _ptr(snr) if len(snr) else None,
                                           _ptr(samples), _ptr(moff), len(moff) - 1 if moff is not None else 0, _ptr(mof), len(snr),
                                           _ptr(lev), int(first_utterance), int(seed) & (2 ** 64 - 1), _ptr(noisy), _ptr(out[0]),
                                           _ptr(out[1]), _ptr(out[2]), mem_space))
        return out if small else None

    def masker_levels(self, wave, wave_dtype, offsets, B, snr_db, maskers, masker_of, seed, noisy, mem_space):
        """The batch under recorded maskers at every level and clean, in one device pass (see f2_masker_levels): level l is the
        recording maskers[masker_of[l]] at snr_db[l]. noisy receives (K+1) * offsets[B] float64, level-major, the clean level last.
        Returns (sigma, gain, start), (K+1)*B values each, level-major."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        snr = np.ascontiguousarray(snr_db, dtype=np.float64).reshape(-1)
        samples, moff, mof = _maskers(maskers, masker_of, len(snr))
        U = (len(snr) + 1) * int(B)
        sigma, gain, start = np.zeros(U, np.float64), np.zeros(U, np.float64), np.zeros(U, np.int64)
        self.check(self.lib.f2_masker_levels(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), int(B), _ptr(snr) if len(snr) else None,
                                             _ptr(samples), _ptr(moff), len(moff) - 1, _ptr(mof), len(snr), int(seed) & (2 ** 64 - 1),
                                             _ptr(noisy), _ptr(sigma), _ptr(gain), _ptr(start), mem_space))
        return sigma, gain, start

    def eval_masker_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, snr_db,
                          maskers, masker_of, seed, noisy, scores, labels, mem_space, window_offsets=None, sigma=None, stats=None):
        """eval_noise_sweep with a recorded masker per level (see f2_eval_masker_sweep): level l is the batch under the recording
        maskers[masker_of[l]] at snr_db[l], the clean level last. Returns (window_offsets, sigma, stats, gain, start): the first
        three as eval_noise_sweep does, gain (float64) and start (int64) of (K+1)*B, level-major."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        snr = np.ascontiguousarray(snr_db, dtype=np.float64).reshape(-1)
        samples, moff, mof = _maskers(maskers, masker_of, len(snr))
        U = (len(snr) + 1) * int(B)
        window_offsets, stats, sigma = _sweep_outputs(U, window_offsets, stats, sigma, True)
        gain, start = np.zeros(U, np.float64), np.zeros(U, np.int64)
        self.check(self.lib.f2_eval_masker_sweep(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn,
                                                 int(bool(lpf)), float(cutoff), precision, radius, step, int(hop),
                                                 _ptr(snr) if len(snr) else None, _ptr(samples), _ptr(moff), len(moff) - 1, _ptr(mof),
                                                 len(snr), int(seed) & (2 ** 64 - 1), _ptr(noisy), _ptr(scores), _ptr(labels),
                                                 _ptr(window_offsets), _ptr(sigma), _ptr(gain), _ptr(start), _ptr(stats), mem_space))
        return window_offsets, sigma, stats, gain, start

    def cnn_create(self, tensors, rows, channels):
        """tensors: 12 contiguous float32 arrays in Keras layouts (see include/f2cnn_hip.h). Returns a handle."""
        arrs = [np.ascontiguousarray(t, dtype=np.float32) for t in tensors]
        if len(arrs) != 12:
            raise ValueError("the network has 12 weight tensors")
        ptrs = (_vp * 12)(*[a.ctypes.data for a in arrs])
        h = _vp()
        self.check(self.lib.f2_cnn_create(self.handle, ptrs, int(rows), int(channels), C.byref(h)))
        return h

    def cnn_info(self, handle, key):
        """f2_cnn_get_info: 'ws_ok', 'ws_dense_ok', 'ws_check_diff', 'ws_dense_check_diff', 'flat', 'f16x3_ok',
        'f16x3_check_diff', 'last_input_bound'"""
        v = _d()
        self.check(self.lib.f2_cnn_get_info(self.handle, handle, key.encode(), C.byref(v)))
        return v.value

    def cnn_destroy(self, handle):
        self.check(self.lib.f2_cnn_destroy(self.handle, handle))

    def cnn_forward(self, handle, x, n, scores, labels, mem_space):
        self.check(self.lib.f2_cnn_forward(self.handle, handle, _ptr(x), int(n), _ptr(scores), _ptr(labels), mem_space))

    def cnn_layers(self, handle, x, n, route, pooled, dense1, scores, mem_space):
        """Inspection entry (f2_cnn_layers): conv4's pooled output (n, flat) in (row, column, channel) order, dense1's output
        (n, 516) and the scores (n, 2), all float32, of n windows on `route` - a CNN_ROUTES value: "call" is what cnn_forward
        does, the others force their kernels and raise F2Error (F2_ERR_UNSUPPORTED) where the network or the input cannot take
        them. numpy arrays or device pointers, by mem_space; any output may be None."""
        self.check(self.lib.f2_cnn_layers(self.handle, handle, _ptr(x), int(n), int(route), _ptr(pooled), _ptr(dense1), _ptr(scores),
                                          mem_space))

    def eval_utterance(self, handle, wave, wave_dtype, N, coefs, Cn, lpf, cutoff, precision, radius, step, env, scores,
                       labels, mem_space):
        nb = _i64()
        self.check(self.lib.f2_eval_utterance(self.handle, handle, _ptr(wave), wave_dtype, int(N), _ptr(coefs), Cn,
                                              int(bool(lpf)), float(cutoff), precision, radius, step, _ptr(env),
                                              _ptr(scores), _ptr(labels), C.byref(nb), mem_space))
        return nb.value


    def eval_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, scores,
                   labels, mem_space):
        """Ragged batch through filterbank, envelope, every-sample windows and the CNN; see f2_eval_batch."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.check(self.lib.f2_eval_batch(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B),
                                          Cn, int(bool(lpf)), float(cutoff), precision, radius, step, _ptr(scores),
                                          _ptr(labels), mem_space))

    def eval_batch_strided(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop,
                           scores, labels, mem_space):
        """f2_eval_batch with a decision every `hop` samples (see f2_eval_batch_strided): row window_offsets[b] + j is
        every-sample window j * hop of utterance b. Returns window_offsets (B + 1, int64)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        window_offsets = np.zeros(int(B) + 1, np.int64)
        self.check(self.lib.f2_eval_batch_strided(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs),
                                                  int(B), Cn, int(bool(lpf)), float(cutoff), precision, radius, step, int(hop),
                                                  _ptr(scores), _ptr(labels), _ptr(window_offsets), mem_space))
        return window_offsets

    def eval_noise_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop,
                         snr_db, seed, noisy, scores, labels, mem_space, window_offsets=None, sigma=None, stats=None):
        """The batch at every noise level of snr_db and clean, in one device pass (see f2_eval_noise_sweep): utterance
        l * B + b of the evaluated batch is utterance b at level l, the clean level last. noisy / scores / labels (numpy
        arrays or device pointers, by mem_space) may be None. Returns (window_offsets ((K+1)*B + 1, int64), sigma ((K+1)*B,
        float64), stats ((K+1)*B, 2) int64: rising windows, windows labelled as the clean level labels them), allocating
        those it is not given."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        snr = np.ascontiguousarray(snr_db, dtype=np.float64).reshape(-1)
        window_offsets, stats, sigma = _sweep_outputs((len(snr) + 1) * int(B), window_offsets, stats, sigma, True)
        self.check(self.lib.f2_eval_noise_sweep(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B),
                                                Cn, int(bool(lpf)), float(cutoff), precision, radius, step, int(hop),
                                                _ptr(snr) if len(snr) else None, len(snr), int(seed) & (2 ** 64 - 1), _ptr(noisy),
                                                _ptr(scores), _ptr(labels), _ptr(window_offsets), _ptr(sigma), _ptr(stats),
                                                mem_space))
        return window_offsets, sigma, stats

    def shaped_noise_levels(self, wave, wave_dtype, offsets, B, snr_db, firs, seed, noisy, mem_space, sigma=None):
        """The batch under coloured noise at every level and clean, in one device pass (see f2_shaped_noise_levels): level l has the
        SNR snr_db[l] and the filter firs[l] (a sequence of 1-D float64 arrays, always host arrays; the library does not normalise
        them). noisy receives (K+1) * offsets[B] float64, level-major, the clean level last (wave and noisy numpy arrays or device
        pointers, by mem_space). Returns sigma ((K+1)*B, float64), allocating it if it is not given."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        snr = np.ascontiguousarray(snr_db, dtype=np.float64).reshape(-1)
        taps, fir_offsets = _pack_firs(firs, len(snr))
        if sigma is None:
            sigma = np.zeros((len(snr) + 1) * int(B), np.float64)
        self.check(self.lib.f2_shaped_noise_levels(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), int(B),
                                                   _ptr(snr) if len(snr) else None, _ptr(taps) if len(taps) else None, _ptr(fir_offsets),
                                                   len(snr), int(seed) & (2 ** 64 - 1), _ptr(noisy), _ptr(sigma), mem_space))
        return sigma

    def eval_shaped_noise_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop,
                                snr_db, firs, seed, noisy, scores, labels, mem_space, window_offsets=None, sigma=None, stats=None):
        """eval_noise_sweep with a filter per level (see f2_eval_shaped_noise_sweep): level l is the batch under noise of the colour
        firs[l] at snr_db[l], the clean level last. Returns (window_offsets, sigma, stats) as eval_noise_sweep does."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        snr = np.ascontiguousarray(snr_db, dtype=np.float64).reshape(-1)
        taps, fir_offsets = _pack_firs(firs, len(snr))
        window_offsets, stats, sigma = _sweep_outputs((len(snr) + 1) * int(B), window_offsets, stats, sigma, True)
        self.check(self.lib.f2_eval_shaped_noise_sweep(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B),
                                                       Cn, int(bool(lpf)), float(cutoff), precision, radius, step, int(hop),
                                                       _ptr(snr) if len(snr) else None, _ptr(taps) if len(taps) else None,
                                                       _ptr(fir_offsets), len(snr), int(seed) & (2 ** 64 - 1), _ptr(noisy), _ptr(scores),
                                                       _ptr(labels), _ptr(window_offsets), _ptr(sigma), _ptr(stats), mem_space))
        return window_offsets, sigma, stats

    def lowpass_levels(self, env, offsets, B, Cn, cutoffs, levels, mem_space):
        """Envelopes that are already in memory at every cutoff of `cutoffs` and unfiltered, in one device pass (see
        f2_lowpass_levels): env holds the ragged (Cn, n_b) float64 blocks of the batch, levels receives (K+1) * Cn *
        offsets[B] float64, level-major, the copy last (numpy arrays or device pointers, by mem_space)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        cut = np.ascontiguousarray(cutoffs, dtype=np.float64).reshape(-1)
        self.check(self.lib.f2_lowpass_levels(self.handle, _ptr(env), _ptr(offsets), int(B), int(Cn), _ptr(cut) if len(cut) else None,
                                              len(cut), _ptr(levels), mem_space))

    def eval_cutoff_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, precision, radius, step, hop, cutoffs, env_levels,
                          scores, labels, mem_space, window_offsets=None, stats=None):
        """The batch at every envelope cutoff of `cutoffs` and unfiltered, in one device pass (see f2_eval_cutoff_sweep):
        utterance l * B + b of the evaluated batch is utterance b at level l, the unfiltered level last. env_levels / scores /
        labels (numpy arrays or device pointers, by mem_space) may be None. Returns (window_offsets ((K+1)*B + 1, int64), stats
        ((K+1)*B, 2) int64: rising windows, windows labelled as the unfiltered level labels them), allocating those it is not
        given."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        cut = np.ascontiguousarray(cutoffs, dtype=np.float64).reshape(-1)
        window_offsets, stats, _ = _sweep_outputs((len(cut) + 1) * int(B), window_offsets, stats)
        self.check(self.lib.f2_eval_cutoff_sweep(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn,
                                                 precision, radius, step, int(hop), _ptr(cut) if len(cut) else None, len(cut),
                                                 _ptr(env_levels), _ptr(scores), _ptr(labels), _ptr(window_offsets), _ptr(stats),
                                                 mem_space))
        return window_offsets, stats

    def reverb_levels(self, wave, wave_dtype, offsets, B, rirs, levels, mem_space):
        """The batch convolved with every impulse response of `rirs` (a sequence of 1-D float64 arrays) and dry, in one device
        pass (see f2_reverb_levels): levels receives (K+1) * offsets[B] float64, level-major, the dry level last (wave and levels
        numpy arrays or device pointers, by mem_space; the responses always host arrays)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        taps, rir_offsets = _pack_rirs(rirs)
        self.check(self.lib.f2_reverb_levels(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), int(B), _ptr(taps) if len(taps) else None,
                                             _ptr(rir_offsets), len(rir_offsets) - 1, _ptr(levels), mem_space))

    def eval_reverb_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, rirs,
                          wet, scores, labels, mem_space, window_offsets=None, stats=None):
        """The batch at every impulse response of `rirs` and dry, in one device pass (see f2_eval_reverb_sweep): utterance
        l * B + b of the evaluated batch is utterance b at level l, the dry level last. wet / scores / labels (numpy arrays or
        device pointers, by mem_space) may be None. Returns (window_offsets ((K+1)*B + 1, int64), stats ((K+1)*B, 2) int64: rising
        windows, windows labelled as the dry level labels them), allocating those it is not given."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        taps, rir_offsets = _pack_rirs(rirs)
        K = len(rir_offsets) - 1
        window_offsets, stats, _ = _sweep_outputs((K + 1) * int(B), window_offsets, stats)
        self.check(self.lib.f2_eval_reverb_sweep(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn,
                                                 int(bool(lpf)), float(cutoff), precision, radius, step, int(hop),
                                                 _ptr(taps) if len(taps) else None, _ptr(rir_offsets), K, _ptr(wet), _ptr(scores),
                                                 _ptr(labels), _ptr(window_offsets), _ptr(stats), mem_space))
        return window_offsets, stats

    def channel_mix_levels(self, env, offsets, B, Cn, mix, levels, mem_space):
        """Envelopes that are already in memory through every mixing matrix of `mix` ((K, Cn, Cn) float64, mix[l][c][c'] the
        weight of input channel c' in output channel c; always a host array) and unchanged, in one device pass (see
        f2_channel_mix_levels): env holds the ragged (Cn, n_b) float64 blocks of the batch, levels receives (K+1) * Cn *
        offsets[B] float64, level-major, the copy last (numpy arrays or device pointers, by mem_space)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        mix = _pack_mix(mix, Cn)
        self.check(self.lib.f2_channel_mix_levels(self.handle, _ptr(env), _ptr(offsets), int(B), int(Cn), _ptr(mix) if len(mix) else None,
                                                  len(mix), _ptr(levels), mem_space))

    def eval_smear_sweep(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, mix,
                         env_levels, scores, labels, mem_space, window_offsets=None, stats=None):
        """The batch at every mixing matrix of `mix` ((K, Cn, Cn) float64, host) and sharp, in one device pass (see
        f2_eval_smear_sweep): utterance l * B + b of the evaluated batch is utterance b at level l, the sharp level last.
        env_levels / scores / labels (numpy arrays or device pointers, by mem_space) may be None. Returns (window_offsets
        ((K+1)*B + 1, int64), stats ((K+1)*B, 2) int64: rising windows, windows labelled as the sharp level labels them),
        allocating those it is not given."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        mix = _pack_mix(mix, Cn)
        window_offsets, stats, _ = _sweep_outputs((len(mix) + 1) * int(B), window_offsets, stats)
        self.check(self.lib.f2_eval_smear_sweep(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn,
                                                int(bool(lpf)), float(cutoff), precision, radius, step, int(hop),
                                                _ptr(mix) if len(mix) else None, len(mix), _ptr(env_levels), _ptr(scores),
                                                _ptr(labels), _ptr(window_offsets), _ptr(stats), mem_space))
        return window_offsets, stats

    def label_accuracy(self, labels, window_offsets, ref_offsets, ref_timepoints, ref_signs, origin, hop, step, mem_space,
                       counts=None):
        """The labels of a strided evaluation against reference labels (see f2_label_accuracy): utterance u owns rows
        window_offsets[u] .. window_offsets[u + 1] of `labels` (uint8 numpy array or device pointer, by mem_space), row j at
        sample origin + j * hop, and is scored against reference set u % R - timepoints (int64, strictly increasing) and signs
        (uint8, 0 / 1) between ref_offsets[r] and ref_offsets[r + 1]. Returns the (U, 2, 2) int64 confusion matrices
        [utterance][reference sign][label] of the counted rows (written into `counts` when given)."""
        window_offsets = np.ascontiguousarray(window_offsets, dtype=np.int64)
        ref_offsets = np.ascontiguousarray(ref_offsets, dtype=np.int64)
        ref_timepoints = np.ascontiguousarray(ref_timepoints, dtype=np.int64)
        ref_signs = np.ascontiguousarray(ref_signs, dtype=np.uint8)
        if isinstance(labels, np.ndarray):
            labels = np.ascontiguousarray(labels, dtype=np.uint8)
        U, R = len(window_offsets) - 1, len(ref_offsets) - 1
        if counts is None:
            counts = np.zeros((U, 2, 2), np.int64)
        if counts.dtype != np.int64 or counts.size != 4 * U or not counts.flags["C_CONTIGUOUS"]:
            raise ValueError("counts must be contiguous int64 (U, 2, 2)")
        self.check(self.lib.f2_label_accuracy(self.handle, _ptr(labels), _ptr(window_offsets), U, _ptr(ref_offsets),
                                              _ptr(ref_timepoints), _ptr(ref_signs), R, int(origin), int(hop), int(step),
                                              _ptr(counts), mem_space))
        return counts.reshape(U, 2, 2)


    def decision_path(self, scores, window_offsets, logit_scale, penalty, path, mem_space, emissions=None, value=None):
        """The smoothed decision per row (see f2_decision_path): the most probable two-state sequence of every utterance under a
        switching penalty, on the integer emissions q = rint(logit_scale * log-odds). scores (n, 2) float32, path (n) uint8 and
        emissions (n) int32 or None: numpy arrays or device pointers, by mem_space. Returns value (U,) int64, the optimum of every
        utterance (written into `value` when given)."""
        window_offsets = np.ascontiguousarray(window_offsets, dtype=np.int64)
        U = len(window_offsets) - 1
        if isinstance(scores, np.ndarray):
            scores = np.ascontiguousarray(scores, dtype=np.float32)
        _want_array(path, np.uint8, int(window_offsets[-1]), "path")
        _want_array(emissions, np.int32, int(window_offsets[-1]), "emissions")
        if value is None:
            value = np.zeros(U, np.int64)
        _want_array(value, np.int64, U, "value")
        self.check(self.lib.f2_decision_path(self.handle, _ptr(scores), _ptr(window_offsets), U, float(logit_scale), int(penalty),
                                             _ptr(path), _ptr(emissions), _ptr(value), mem_space))
        return value

    def decision_runs(self, labels, emissions, window_offsets, runs, capacity, mem_space, run_offsets=None):
        """Maximal runs of equal decisions (see f2_decision_runs). labels (n) uint8 - a path or raw labels - and emissions (n)
        int32 or None: numpy arrays or device pointers, by mem_space; runs (capacity, 4) int64 likewise, or None to count only:
        {first row within the utterance, rows, label, sum of the emissions}. Returns run_offsets (U + 1,) int64."""
        window_offsets = np.ascontiguousarray(window_offsets, dtype=np.int64)
        U = len(window_offsets) - 1
        if isinstance(labels, np.ndarray):
            labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if isinstance(emissions, np.ndarray):
            emissions = np.ascontiguousarray(emissions, dtype=np.int32)
        _want_array(runs, np.int64, 4 * max(int(capacity), 0), "runs")
        if run_offsets is None:
            run_offsets = np.zeros(U + 1, np.int64)
        _want_array(run_offsets, np.int64, U + 1, "run_offsets")
        self.check(self.lib.f2_decision_runs(self.handle, _ptr(labels), _ptr(emissions), _ptr(window_offsets), U, _ptr(run_offsets),
                                             _ptr(runs), int(capacity), mem_space))
        return run_offsets

    def interval_tally(self, labels, path, emissions, window_offsets, iv_offsets, iv_bounds, origin, hop, tally, mem_space):
        """Decisions per labelled interval (see f2_interval_tally): utterance u is tallied against interval set u % R, sample
        intervals [a, b) between iv_offsets[r] and iv_offsets[r + 1] of iv_bounds (total, 2). labels / path (uint8, path may be
        None) / emissions (int32 or None) / tally ((U / R) * total, 4) int64 - {rows, rising labels, rising path, sum of the
        emissions} -: numpy arrays or device pointers, by mem_space. Returns `tally`."""
        window_offsets = np.ascontiguousarray(window_offsets, dtype=np.int64)
        iv_offsets = np.ascontiguousarray(iv_offsets, dtype=np.int64)
        iv_bounds = np.ascontiguousarray(iv_bounds, dtype=np.int64)
        U, R = len(window_offsets) - 1, len(iv_offsets) - 1
        if isinstance(labels, np.ndarray):
            labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if isinstance(path, np.ndarray):
            path = np.ascontiguousarray(path, dtype=np.uint8)
        if isinstance(emissions, np.ndarray):
            emissions = np.ascontiguousarray(emissions, dtype=np.int32)
        if R >= 1 and U % R == 0:
            _want_array(tally, np.int64, 4 * (U // R) * int(iv_offsets[-1]), "tally")
        self.check(self.lib.f2_interval_tally(self.handle, _ptr(labels), _ptr(path), _ptr(emissions), _ptr(window_offsets), U,
                                              _ptr(iv_offsets), _ptr(iv_bounds), R, int(origin), int(hop), _ptr(tally), mem_space))
        return tally

    def eval_segments_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop,
                            logit_scale, penalty, iv_offsets, iv_bounds, scores, labels, path, emissions, runs, tally, mem_space,
                            want_value=True, want_runs=True):
        """f2_eval_batch_strided, then the path, its runs and the interval tally on the device's scores (see
        f2_eval_segments_batch). iv_offsets / iv_bounds: the interval sets or None (no tally). scores / labels / path / emissions /
        runs ((rows, 4) int64, room for every row) / tally: numpy arrays or device pointers, by mem_space, each may be None.
        Returns (window_offsets (B + 1), value (B) or None, run_offsets (B + 1) or None)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        R = 0
        if iv_offsets is not None:
            iv_offsets = np.ascontiguousarray(iv_offsets, dtype=np.int64)
            iv_bounds = np.ascontiguousarray(iv_bounds, dtype=np.int64)
            R = len(iv_offsets) - 1
        window_offsets = np.zeros(max(int(B), 0) + 1, np.int64)
        value = np.zeros(max(int(B), 0), np.int64) if want_value else None
        run_offsets = np.zeros(max(int(B), 0) + 1, np.int64) if want_runs else None
        self.check(self.lib.f2_eval_segments_batch(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn,
                                                   int(bool(lpf)), float(cutoff), precision, radius, step, int(hop), float(logit_scale),
                                                   int(penalty), _ptr(iv_offsets), _ptr(iv_bounds), R, _ptr(scores), _ptr(labels),
                                                   _ptr(window_offsets), _ptr(path), _ptr(emissions), _ptr(value), _ptr(run_offsets),
                                                   _ptr(runs), _ptr(tally), mem_space))
        return window_offsets, value, run_offsets

    def cnn_score_windows(self, handle, windows, n, normalize, signs, groups, n_groups, scores, labels, mem_space, counts=None,
                          loss_sum=None):
        """A model scored on n stored, labelled windows in one device pass (see f2_cnn_score_windows): `windows` (n, rows, C)
        float32, `signs` (n) uint8 0 / 1, `groups` (n) int32 in [0, n_groups) or None (then n_groups must be 1), `scores` (n, 2)
        float32 / `labels` (n) uint8 or None - numpy arrays or device pointers, by mem_space. normalize=True: the windows are raw
        envelope windows, normalised on the device as normalizeInputBatch does. Returns (counts (n_groups, 2, 2) int64
        [group][sign][label], loss_sum (n_groups,) float64), written into `counts` / `loss_sum` when given."""
        G = int(n_groups)
        if isinstance(windows, np.ndarray):
            windows = np.ascontiguousarray(windows, dtype=np.float32)
        if isinstance(signs, np.ndarray):
            signs = np.ascontiguousarray(signs, dtype=np.uint8)
        if isinstance(groups, np.ndarray):
            groups = np.ascontiguousarray(groups, dtype=np.int32)
        if counts is None:
            counts = np.zeros((max(G, 0), 2, 2), np.int64)
        if loss_sum is None:
            loss_sum = np.zeros(max(G, 0), np.float64)
        if G >= 1 and (counts.dtype != np.int64 or counts.size != 4 * G or not counts.flags["C_CONTIGUOUS"]
                       or loss_sum.dtype != np.float64 or loss_sum.size != G or not loss_sum.flags["C_CONTIGUOUS"]):
            raise ValueError("counts / loss_sum must be contiguous int64 (n_groups, 2, 2) / float64 (n_groups,)")
        self.check(self.lib.f2_cnn_score_windows(self.handle, handle, _ptr(windows), int(n), int(normalize), _ptr(signs),
                                                 _ptr(groups), G, _ptr(scores), _ptr(labels), _ptr(counts), _ptr(loss_sum),
                                                 mem_space))
        return counts.reshape(G, 2, 2), loss_sum

    def _picture_args(self, offsets, B, spans, range_out):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if spans is not None:
            spans = np.ascontiguousarray(spans, dtype=np.int64)
            if spans.size != 2 * int(B):
                raise ValueError("spans must hold (s_b, e_b) for each of the B utterances")
        if range_out is None:
            range_out = np.zeros((max(int(B), 0), 2), np.float64)
        if range_out.dtype != np.float64 or range_out.size != 2 * max(int(B), 0) or not range_out.flags["C_CONTIGUOUS"]:
            raise ValueError("range_out must be contiguous float64 (B, 2)")
        return offsets, spans, range_out

    def envelope_picture(self, env, offsets, B, Cn, spans, width, pool, pooled, levels, mem_space, range_out=None):
        """Pictures of `width` columns of the ragged (Cn, n_b) float64 envelopes (see f2_envelope_picture): `pooled` (B, Cn, width)
        float64 mean (pool=0) or maximum (pool=1) per column, `levels` (B, Cn, width) uint8 LogNorm levels - numpy arrays or device
        pointers, by mem_space, either may be None. spans: (B, 2) sample spans [s_b, e_b) or None for whole utterances. Returns
        the (B, 2) float64 range (smallest, largest pixel > 0) of every picture, written into `range_out` when given."""
        offsets, spans, range_out = self._picture_args(offsets, B, spans, range_out)
        self.check(self.lib.f2_envelope_picture(self.handle, _ptr(env), _ptr(offsets), int(B), Cn, _ptr(spans), int(width), int(pool),
                                                _ptr(pooled), _ptr(levels), _ptr(range_out), mem_space))
        return range_out.reshape(-1, 2)

    def gammatonegram_batch(self, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, spans, width, pool, pooled, levels,
                            mem_space, range_out=None):
        """Ragged batch of waves -> the pictures f2_envelope_picture gives for its envelopes, which never leave the device (see
        f2_gammatonegram_batch). Arguments and return value as in envelope_picture."""
        offsets, spans, range_out = self._picture_args(offsets, B, spans, range_out)
        self.check(self.lib.f2_gammatonegram_batch(self.handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn,
                                                   int(bool(lpf)), float(cutoff), precision, _ptr(spans), int(width), int(pool),
                                                   _ptr(pooled), _ptr(levels), _ptr(range_out), mem_space))
        return range_out.reshape(-1, 2)

    def score_track(self, scores, labels, window_offsets, spans, origin, hop, width, track, mem_space):
        """The decisions of a strided evaluation reduced to `width` time columns per utterance (see f2_score_track): utterance u
        owns rows window_offsets[u] .. window_offsets[u + 1] of `scores` (n, 2) float32 / `labels` (n) uint8, row j at sample
        origin + j * hop; spans (U, 2): the sample span [s_u, e_u) its columns divide. `track` (U, width, 5) float64 - rows,
        rising rows, mean / min / max of scores[:, 1] per column. scores / labels / track: numpy arrays or device pointers, by
        mem_space. Returns `track`."""
        window_offsets, spans, U = _track_args(window_offsets, spans)
        if isinstance(scores, np.ndarray):
            scores = np.ascontiguousarray(scores, dtype=np.float32)
        if isinstance(labels, np.ndarray):
            labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if isinstance(track, np.ndarray) and (track.dtype != np.float64 or track.size != 5 * U * int(width)
                                              or not track.flags["C_CONTIGUOUS"]):
            raise ValueError("track must be contiguous float64 (U, width, 5)")
        self.check(self.lib.f2_score_track(self.handle, _ptr(scores), _ptr(labels), _ptr(window_offsets), U, _ptr(spans), int(origin),
                                           int(hop), int(width), _ptr(track), mem_space))
        return track

    def _figure_call(self, fn, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, own, spans,
                     width, pool, levels, range_out, reduced, scores, labels, mem_space):
        """The three fused figure calls: `own` - the call's arguments between hop and spans, as they go down; `reduced` - its
        outputs between the range and the scores. Returns (window_offsets (B + 1, int64), range (B, 2) float64)."""
        offsets, spans, range_out = self._picture_args(offsets, B, spans, range_out)
        window_offsets = np.zeros(max(int(B), 0) + 1, np.int64)
        self.check(fn(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn, int(bool(lpf)), float(cutoff),
                      precision, radius, step, int(hop), *own, _ptr(spans), int(width), int(pool), _ptr(levels), _ptr(range_out),
                      *[_ptr(a) for a in reduced], _ptr(scores), _ptr(labels), _ptr(window_offsets), mem_space))
        return window_offsets, range_out.reshape(-1, 2)

    def eval_figure_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, spans,
                          width, pool, levels, track, scores, labels, mem_space, range_out=None):
        """eval_batch_strided, the picture of the envelopes it uses and the track of its decisions in one device pass (see
        f2_eval_figure_batch). levels (B, Cn, width) uint8, track (B, width, 5) float64, scores, labels: numpy arrays or device
        pointers, by mem_space, any may be None; spans as in envelope_picture. Returns (window_offsets (B + 1, int64), range
        (B, 2) float64)."""
        return self._figure_call(self.lib.f2_eval_figure_batch, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision,
                                 radius, step, hop, (), spans, width, pool, levels, range_out, (track,), scores, labels, mem_space)

    @staticmethod
    def _patch_args(patches, fill):
        patches = np.ascontiguousarray(patches, dtype=np.int32).reshape(-1, 4)
        # (a c_float made from the float32's bytes: a NaN payload reaches the library as it is)
        return patches, len(patches), C.c_float.from_buffer_copy(np.float32(fill).tobytes())

    def occlude_windows(self, x, n, R, Cn, patches, fill, out, mem_space):
        """n windows (R, Cn) float32 -> (n, K + 1, R, Cn): level 0 the window, level k + 1 the window with the rectangle
        patches[k] = (r0, r1, c0, c1), half-open, replaced by `fill` (see f2_occlude_windows). x / out: numpy arrays or device
        pointers, by mem_space. Returns `out`."""
        patches, K, fill = self._patch_args(patches, fill)
        self.check(self.lib.f2_occlude_windows(self.handle, _ptr(x), int(n), int(R), int(Cn), _ptr(patches) if K else None, K, fill,
                                               _ptr(out), mem_space))
        return out

    def occlusion_map(self, scores, labels, window_offsets, K, spans, origin, hop, width, map_out, mem_space):
        """The scores (n, K + 1, 2) float32 and labels (n, K + 1) uint8 of an occluded evaluation reduced to `width` time columns per
        utterance and patch (see f2_occlusion_map; rows, spans and columns as in score_track). `map_out` (U, K, width, 4) float64 -
        rows, flipped rows, mean and mean absolute change of scores[:, k + 1, 1] against scores[:, 0, 1]. scores / labels /
        map_out: numpy arrays or device pointers, by mem_space. Returns `map_out`."""
        window_offsets, spans, U = _track_args(window_offsets, spans)
        if isinstance(scores, np.ndarray):
            scores = np.ascontiguousarray(scores, dtype=np.float32)
        if isinstance(labels, np.ndarray):
            labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if isinstance(map_out, np.ndarray) and (map_out.dtype != np.float64 or map_out.size != 4 * U * max(int(K), 0) * int(width)
                                                or not map_out.flags["C_CONTIGUOUS"]):
            raise ValueError("map_out must be contiguous float64 (U, K, width, 4)")
        self.check(self.lib.f2_occlusion_map(self.handle, _ptr(scores), _ptr(labels), _ptr(window_offsets), U, int(K), _ptr(spans),
                                             int(origin), int(hop), int(width), _ptr(map_out), mem_space))
        return map_out

    def eval_occlusion_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, patches,
                             fill, spans, width, pool, levels, map_out, summary, scores, labels, mem_space, range_out=None):
        """eval_figure_batch with every window evaluated at K + 1 occlusion levels and the occlusion map in the track's place (see
        f2_eval_occlusion_batch). levels (B, Cn, width) uint8, map_out (B, K, width, 4) and summary (B, K, 4) float64, scores
        (n, K + 1, 2) float32, labels (n, K + 1) uint8: numpy arrays or device pointers, by mem_space, any may be None; n counts
        the windows of eval_batch_strided. Returns (window_offsets (B + 1, int64), range (B, 2) float64)."""
        patches, K, fill = self._patch_args(patches, fill)
        return self._figure_call(self.lib.f2_eval_occlusion_batch, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision,
                                 radius, step, hop, (_ptr(patches) if K else None, K, fill), spans, width, pool, levels, range_out,
                                 (map_out, summary), scores, labels, mem_space)

    def cnn_input_gradient(self, handle, x, n, grad, profile, scores, mem_space):
        """G = dP(rising)/dx of n windows (rows, channels) float32 by one backward-data pass on the device (see
        f2_cnn_input_gradient). grad (n, rows, channels) float32, profile (n, channels, 2) float64 - sum over the rows of G x and
        of |G| - and scores (n, 2) float32 of the recorded forward: numpy arrays or device pointers, by mem_space, any may be
        None."""
        self.check(self.lib.f2_cnn_input_gradient(self.handle, handle, _ptr(x), int(n), _ptr(grad), _ptr(profile), _ptr(scores),
                                                  mem_space))

    def cnn_loss_gradient(self, handle, x, y, index, m, drop, seed, step, grads, mem_space, want_loss=True):
        """The gradient of the summed cross-entropy of m labelled windows for the 12 weight tensors, training mode (see
        f2_cnn_loss_gradient): x (n_all, rows, channels) float32, y (n_all) uint8, index (m) int64 or None (the first m) - numpy
        arrays or device pointers, by mem_space. drop: the three dropout rates; seed, step: of the masks. grads: None, or 12 numpy
        arrays / device pointers in the Keras layouts, filled. Returns (loss sum, windows decided as labelled), or None with
        want_loss=False (a device-memory call then only enqueues)."""
        rates = (_d * 3)(*[float(r) for r in drop])
        ptrs = None
        if grads is not None:
            if len(grads) != 12:
                raise ValueError("the network has 12 weight tensors")
            ptrs = (_vp * 12)(*[_ptr(g) for g in grads])
        loss, hits = _d(), _i64()
        self.check(self.lib.f2_cnn_loss_gradient(self.handle, handle, _ptr(x), _ptr(y), _ptr(index), int(m), rates, int(seed), int(step), ptrs,
                                                 C.byref(loss) if want_loss else None, C.byref(hits) if want_loss else None, mem_space))
        return (loss.value, hits.value) if want_loss else None

    def trainer_create(self, tensors, rows, channels, lr, rho, eps, decay, drop, seed):
        """A training state on the device (see f2_trainer_create): 12 float32 tensors in Keras layouts, RMSprop's constants, the
        three dropout rates and the seed of the masks. Returns a handle."""
        arrs = [np.ascontiguousarray(t, dtype=np.float32) for t in tensors]
        if len(arrs) != 12:
            raise ValueError("the network has 12 weight tensors")
        ptrs = (_vp * 12)(*[a.ctypes.data for a in arrs])
        rates = (_d * 3)(*[float(r) for r in drop])
        h = _vp()
        self.check(self.lib.f2_trainer_create(self.handle, ptrs, int(rows), int(channels), float(lr), float(rho), float(eps), float(decay),
                                              rates, int(seed), C.byref(h)))
        return h

    def trainer_destroy(self, handle):
        self.check(self.lib.f2_trainer_destroy(self.handle, handle))

    def trainer_set_data(self, handle, x, y):
        """x (n, rows, channels) float32 normalised windows and y (n) 0 / 1 labels, copied to the device once"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.uint8)
        if x.ndim != 3 or len(y) != len(x):
            raise ValueError("expected (n, rows, channels) windows and n labels")
        self.check(self.lib.f2_trainer_set_data(self.handle, handle, x.ctypes.data, y.ctypes.data, len(x)))

    def trainer_set_waves(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, center_offsets, centers, signs,
                          radius, step, group):
        """The corpus the trainer renders its windows from (see f2_trainer_set_waves): host arrays, copied to the device once"""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        center_offsets = np.ascontiguousarray(center_offsets, dtype=np.int64)
        centers = np.ascontiguousarray(centers, dtype=np.int64)
        signs = np.ascontiguousarray(signs, dtype=np.uint8)
        self.check(self.lib.f2_trainer_set_waves(self.handle, handle, _ptr(wave), wave_dtype, _ptr(offsets), _ptr(coefs), int(B), Cn,
                                                 int(bool(lpf)), float(cutoff), precision, _ptr(center_offsets), _ptr(centers),
                                                 _ptr(signs), radius, step, int(group)))

    def _trainer_render_staged(self, name, v):
        """f2_trainer_render (name "noisy") / f2_trainer_render_<name> from the arguments `v` of its method; no first_utterance: a render counts"""
        args, alive = _stage_args([k for k in _STAGE_KEYS[name] if k != "first_utterance"], v)
        self.check(getattr(self.lib, "f2_trainer_render" + ("" if name == "noisy" else "_" + name))(self.handle, v["handle"], *args))

    def trainer_render(self, handle, snr_db=(), level_of=None, seed=0):
        """The training windows from the stored waves, utterance b at snr_db[level_of[b]] (see f2_trainer_render)"""
        self._trainer_render_staged("noisy", locals())

    def trainer_render_wet(self, handle, rirs=(), room_of=None, snr_db=(), level_of=None, seed=0):
        """The training windows from the stored waves, utterance b in room rirs[room_of[b]] and at snr_db[level_of[b]] (see
        f2_trainer_render_wet)"""
        self._trainer_render_staged("wet", locals())

    def trainer_render_coloured(self, handle, rirs=(), room_of=None, snr_db=(), firs=None, level_of=None, seed=0):
        """The training windows from the stored waves, utterance b in room rirs[room_of[b]] and under noise of the colour
        firs[level_of[b]] at snr_db[level_of[b]]; firs None: trainer_render_wet (see f2_trainer_render_coloured)"""
        self._trainer_render_staged("coloured", locals())

    def trainer_render_smeared(self, handle, rirs=(), room_of=None, snr_db=(), firs=None, level_of=None, seed=0, mixes=None,
                               mix_of=None, channels=None):
        """trainer_render_coloured with the windows of utterance b mixed across their channels by mixes[mix_of[b]] ((K, C, C)
        float64), sharp where mix_of[b] == K; mixes None: trainer_render_coloured (see f2_trainer_render_smeared)"""
        self._trainer_render_staged("smeared", locals())

    def trainer_render_masked(self, handle, rirs=(), room_of=None, snr_db=(), firs=None, level_of=None, seed=0, mixes=None,
                              mix_of=None, channels=None, maskers=None, masker_of=None, masker_snrs=(), masker_level_of=None):
        """trainer_render_smeared with utterance b under the recording maskers[masker_of[l]] at masker_snrs[l], l =
        masker_level_of[b], between its room and its noise; maskers None: trainer_render_smeared (see f2_trainer_render_masked)"""
        self._trainer_render_staged("masked", locals())

    def trainer_render_filtered(self, handle, rirs=(), room_of=None, snr_db=(), firs=None, level_of=None, seed=0, mixes=None,
                                mix_of=None, channels=None, maskers=None, masker_of=None, masker_snrs=(), masker_level_of=None,
                                cutoffs=(), cutoff_of=None):
        """trainer_render_masked with the unfiltered envelopes of utterance b low-passed at cutoffs[cutoff_of[b]] Hz before the
        gather, left as they are where cutoff_of[b] == len(cutoffs); cutoff_of None: trainer_render_masked (see
        f2_trainer_render_filtered)"""
        self._trainer_render_staged("filtered", locals())

    def trainer_get_windows(self, handle, first, count, shape):
        """Rows first .. first + count - 1 of the training set: (count, *shape) float32 windows and (count) uint8 labels"""
        x = np.empty((int(count),) + tuple(shape), np.float32)
        y = np.empty(int(count), np.uint8)
        self.check(self.lib.f2_trainer_get_windows(self.handle, handle, int(first), int(count), _ptr(x), _ptr(y)))
        return x, y

    def trainer_steps(self, handle, order, batch):
        """ceil(len(order) / batch) RMSprop steps over the windows order[...] of the training set, enqueued back to back (see
        f2_trainer_steps). Returns (sum of the steps' loss sums, windows decided as labelled)."""
        order = np.ascontiguousarray(order, dtype=np.int64)
        loss, hits = _d(), _i64()
        self.check(self.lib.f2_trainer_steps(self.handle, handle, order.ctypes.data, len(order), int(batch), C.byref(loss), C.byref(hits)))
        return loss.value, hits.value

    def trainer_get(self, handle, what, shapes):
        """The trainer's 'weights', 'accumulators' or last 'gradient' as 12 float32 arrays of `shapes` (Keras layouts)"""
        out = [np.empty(shp, np.float32) for shp in shapes]
        ptrs = (_vp * 12)(*[a.ctypes.data for a in out])
        self.check(self.lib.f2_trainer_get(self.handle, handle, TRAINER_WHAT[what], ptrs))
        return out

    def trainer_info(self, handle, key):
        """f2_trainer_get_info: 'iterations', 'windows', 'utterances'"""
        v = _d()
        self.check(self.lib.f2_trainer_get_info(self.handle, handle, key.encode(), C.byref(v)))
        return v.value

    def saliency_map(self, profile, window_offsets, Cn, spans, origin, hop, width, map_out, mem_space):
        """The profile rows (n, Cn, 2) float64 of cnn_input_gradient reduced to `width` time columns per utterance and channel (see
        f2_saliency_map; rows, spans and columns as in score_track). `map_out` (U, Cn, width, 3) float64 - rows, mean of
        profile[:, c, 0], mean of profile[:, c, 1]. profile / map_out: numpy arrays or device pointers, by mem_space. Returns
        `map_out`."""
        window_offsets, spans, U = _track_args(window_offsets, spans)
        if isinstance(profile, np.ndarray):
            profile = np.ascontiguousarray(profile, dtype=np.float64)
        if isinstance(map_out, np.ndarray) and (map_out.dtype != np.float64 or map_out.size != 3 * U * max(int(Cn), 0) * int(width)
                                                or not map_out.flags["C_CONTIGUOUS"]):
            raise ValueError("map_out must be contiguous float64 (U, Cn, width, 3)")
        self.check(self.lib.f2_saliency_map(self.handle, _ptr(profile), _ptr(window_offsets), U, int(Cn), _ptr(spans), int(origin),
                                            int(hop), int(width), _ptr(map_out), mem_space))
        return map_out

    def eval_saliency_batch(self, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision, radius, step, hop, spans,
                            width, pool, levels, map_out, summary, scores, labels, mem_space, range_out=None):
        """eval_figure_batch with every window differentiated while it is in device scratch and the saliency map in the track's
        place (see f2_eval_saliency_batch). levels (B, Cn, width) uint8, map_out (B, Cn, width, 3) and summary (B, Cn, 3) float64,
        scores (n, 2) float32, labels (n) uint8: numpy arrays or device pointers, by mem_space, any may be None. Returns
        (window_offsets (B + 1, int64), range (B, 2) float64)."""
        return self._figure_call(self.lib.f2_eval_saliency_batch, handle, wave, wave_dtype, offsets, coefs, B, Cn, lpf, cutoff, precision,
                                 radius, step, hop, (), spans, width, pool, levels, range_out, (map_out, summary), scores, labels, mem_space)

    def resample_batch(self, audio, pcm_format, channels, channel, offsets, B, up, down, taps, half_len, out, mem_space):
        """Ragged batch of interleaved PCM frames (offsets in frames) -> mono float64 samples in int16 units at up / down times
        the rate, scipy.signal.resample_poly's arithmetic (see f2_resample_batch). audio / out: numpy arrays or device pointers,
        by mem_space; out holds sum(resampled_length(n_b, up, down)) samples. taps (2 * half_len + 1 float64) may be None when
        up == down == 1. channel -1: the mean of the channels. Returns out_offsets (B + 1, int64)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if taps is not None:
            taps = np.ascontiguousarray(taps, dtype=np.float64)
            if taps.size != 2 * int(half_len) + 1:
                raise ValueError("taps must hold 2 * half_len + 1 values")
        out_offsets = np.zeros(max(int(B), 0) + 1, np.int64)
        self.check(self.lib.f2_resample_batch(self.handle, _ptr(audio), int(pcm_format), int(channels), int(channel), _ptr(offsets),
                                              int(B), int(up), int(down), _ptr(taps), int(half_len), _ptr(out), _ptr(out_offsets),
                                              mem_space))
        return out_offsets


def _track_args(window_offsets, spans):
    """window offsets and spans of score_track, occlusion_map and saliency_map as they go down, and U"""
    window_offsets = np.ascontiguousarray(window_offsets, dtype=np.int64)
    U = len(window_offsets) - 1
    spans = np.ascontiguousarray(spans, dtype=np.int64)
    if spans.size != 2 * U:
        raise ValueError("spans must hold (s_u, e_u) for each of the U utterances")
    return window_offsets, spans, U


def _sweep_outputs(U, window_offsets, stats, sigma=None, with_sigma=False):
    """The small outputs of a sweep over U = (K+1)*B utterances, allocated where they are None and checked where they are given:
    (window_offsets, stats, sigma); sigma stays None without with_sigma"""
    want = [(np.int64, U + 1, (U + 1,)), (np.int64, 2 * U, (U, 2))] + ([(np.float64, U, (U,))] if with_sigma else [])
    got = [np.zeros(shape, dt) if a is None else a for a, (dt, _, shape) in zip((window_offsets, stats, sigma), want)]
    if any(a.dtype != dt or a.size != n or not a.flags["C_CONTIGUOUS"] for a, (dt, n, _) in zip(got, want)):
        raise ValueError("window_offsets / sigma / stats must be contiguous int64 (K+1)*B + 1, float64 (K+1)*B, int64 ((K+1)*B, 2)"
                         if with_sigma else "window_offsets / stats must be contiguous int64 (K+1)*B + 1 / ((K+1)*B, 2)")
    return got + [None] * (3 - len(got))


def _noise_levels(snr_db, level_of):
    """(snr_db as float64 (K), level_of as int32 or None) for the calls that give every utterance a noise level of its own"""
    snr = np.ascontiguousarray(snr_db if snr_db is not None else (), dtype=np.float64).reshape(-1)
    lev = None if level_of is None else np.ascontiguousarray(level_of, dtype=np.int32).reshape(-1)
    return snr, lev


def _pack_rirs(rirs):
    """(taps, rir_offsets) of f2_reverb_levels: the responses one after the other as float64, and their K + 1 offsets"""
    rirs = [np.ascontiguousarray(h, dtype=np.float64).reshape(-1) for h in rirs]
    rir_offsets = np.zeros(len(rirs) + 1, np.int64)
    rir_offsets[1:] = np.cumsum([len(h) for h in rirs])
    taps = np.concatenate(rirs) if rirs else np.zeros(0, np.float64)
    return np.ascontiguousarray(taps), rir_offsets


def _pack_firs(firs, K):
    """(taps, fir_offsets) of f2_shaped_noise_levels: one filter per level of snr_db, packed as _pack_rirs packs responses"""
    firs = list(firs)
    if len(firs) != K:
        raise ValueError("{} filters for {} noise levels (one per level is needed)".format(len(firs), K))
    return _pack_rirs(firs)


def _colours(firs, K):
    """(taps, fir_offsets) for the calls that give every utterance a coloured level of its own, (None, None) without filters"""
    if firs is None:
        return None, None
    taps, fir_offsets = _pack_firs(firs, K)
    return (taps if len(taps) else None), fir_offsets


def _maskers(maskers, masker_of, K):
    """(samples, masker_offsets, masker_of as int32) of the masker calls: the recordings one after the other as float64 with their
    R + 1 offsets, and the recording of each of the K levels; (None, None, None) without recordings"""
    if maskers is None:
        return None, None, None
    samples, masker_offsets = _pack_rirs(maskers)
    mof = np.ascontiguousarray(masker_of if masker_of is not None else (), dtype=np.int32).reshape(-1)
    if len(mof) != K:
        raise ValueError("{} recordings named for {} masker levels (one per level is needed)".format(len(mof), K))
    return (samples if len(samples) else None), masker_offsets, mof


def _cutoff_levels(cutoffs, cutoff_of):
    """(cutoffs as float64, cutoff_of as int32 or None) for the calls that give every utterance an envelope cutoff of its own"""
    cut = np.ascontiguousarray(cutoffs if cutoffs is not None else (), dtype=np.float64).reshape(-1)
    lev = None if cutoff_of is None else np.ascontiguousarray(cutoff_of, dtype=np.int32).reshape(-1)
    return cut, lev


def _rooms(rirs, room_of):
    """(taps, rir_offsets, room_of as int32 or None) for the calls that give every utterance a room of its own"""
    taps, rir_offsets = _pack_rirs(rirs if rirs is not None else ())
    room = None if room_of is None else np.ascontiguousarray(room_of, dtype=np.int32).reshape(-1)
    return taps, rir_offsets, room


def _pack_mix(mix, Cn):
    """the (K, Cn, Cn) float64 matrices of f2_channel_mix_levels as one contiguous array (K = 0 for an empty sequence)"""
    mix = np.ascontiguousarray(mix, dtype=np.float64)
    if mix.size == 0:
        return np.zeros((0, int(Cn), int(Cn)), np.float64)
    if mix.ndim == 2:
        mix = mix[None]
    if mix.ndim != 3 or mix.shape[1:] != (int(Cn), int(Cn)):
        raise ValueError("mixing matrices must have the shape (K, {0}, {0}), not {1}".format(int(Cn), mix.shape))
    return np.ascontiguousarray(mix)


def _smears(mixes, mix_of, Cn):
    """(mix as (K, Cn, Cn) float64, mix_of as int32 or None) for the calls that give every utterance a spectral resolution of its
    own; mixes None: no matrices. Cn None: the matrices say how many channels they have."""
    if mixes is None:
        mixes = ()
    if Cn is None:
        mixes = np.asarray(mixes, dtype=np.float64)
        Cn = mixes.shape[-1] if mixes.size else 1
    mix = _pack_mix(mixes, Cn)
    lev = None if mix_of is None else np.ascontiguousarray(mix_of, dtype=np.int32).reshape(-1)
    return mix, lev


# the stage arguments of f2_input_batch_<name>, in the order of the C declaration (f2_trainer_render<_name>: without first_utterance)
_STAGE_KEYS = {"noisy": "snr_db K level_of first_utterance seed".split()}
_STAGE_KEYS["wet"] = "rir rir_offsets Kr room_of".split() + _STAGE_KEYS["noisy"]
_STAGE_KEYS["coloured"] = "rir rir_offsets Kr room_of snr_db fir fir_offsets K level_of first_utterance seed".split()
_STAGE_KEYS["smeared"] = _STAGE_KEYS["coloured"] + "mix Km mix_of".split()
_STAGE_KEYS["masked"] = _STAGE_KEYS["smeared"] + "masker_snr_db masker masker_offsets R masker_of Kk masker_level_of".split()
_STAGE_KEYS["filtered"] = _STAGE_KEYS["masked"] + "cutoff_levels_hz Kc cutoff_of".split()


def _stage_args(keys, v):
    """([the C arguments named by `keys`], what holds their arrays until the call returns) from the Python arguments `v` of a call with
    augmentation stages: noise levels, colours, rooms, spectral resolutions, maskers, cutoffs, marshalled in that order and only where the symbol has
    them. Arrays become their addresses; counts, first_utterance and seed are plain ints, which _ptr hands through as they are"""
    snr, lev = _noise_levels(v["snr_db"], v["level_of"])
    a = dict(snr_db=snr if len(snr) else None, K=len(snr), level_of=lev, first_utterance=int(v.get("first_utterance", 0)),
             seed=int(v["seed"]) & (2 ** 64 - 1))
    if "fir" in keys:
        a["fir"], a["fir_offsets"] = _colours(v["firs"], len(snr))
    if "rir" in keys:
        taps, a["rir_offsets"], a["room_of"] = _rooms(v["rirs"], v["room_of"])
        a.update(rir=taps if len(taps) else None, Kr=len(a["rir_offsets"]) - 1)
    if "mix" in keys:
        mix, a["mix_of"] = _smears(v["mixes"], v["mix_of"], v.get("Cn", v.get("channels")))
        a.update(mix=mix if len(mix) else None, Km=len(mix))
    if "masker" in keys:
        msnr, a["masker_level_of"] = _noise_levels(v["masker_snrs"], v["masker_level_of"])
        a["masker"], a["masker_offsets"], a["masker_of"] = _maskers(v["maskers"], v["masker_of"], len(msnr))
        a.update(masker_snr_db=msnr if len(msnr) else None, Kk=len(msnr), R=len(a["masker_offsets"]) - 1 if a["masker_offsets"] is not None else 0)
    if "cutoff_of" in keys:
        cut, a["cutoff_of"] = _cutoff_levels(v["cutoffs"], v["cutoff_of"])
        a.update(cutoff_levels_hz=cut if len(cut) else None, Kc=len(cut))
    return [_ptr(a[k]) for k in keys], a


def resampled_length(n, up, down):
    """Samples f2_resample_batch gives for n frames: ceil(n up / down), as scipy.signal.resample_poly."""
    return -(-int(n) * int(up) // int(down))


def strided_window_count(n, radius, step, hop):
    """Windows f2_eval_batch_strided evaluates in an utterance of n samples: ceil(max(0, n - (2 radius + 1) step) / hop)."""
    if hop < 1:
        raise ValueError("hop must be at least 1 sample")
    return -(-max(int(n) - (2 * radius + 1) * step, 0) // int(hop))


def strided_timepoints(n, radius, step, hop):
    """Centre sample of each of those windows: radius step + j hop (int64)."""
    return radius * step + int(hop) * np.arange(strided_window_count(n, radius, step, hop), dtype=np.int64)


_default_ctx = {}
_extra_ctx = {}


def default_context(device=None):
    """Process-wide context per device (default: $F2CNN_DEVICE, else torchrun's $LOCAL_RANK, else 0)."""
    if device is None:
        device = int(os.environ.get("F2CNN_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    ctx = _default_ctx.get(device)
    if ctx is None or ctx.handle is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx


def pipeline_contexts(n=2, device=None):
    """n contexts (= n streams with their own staging memory) on one device, the first being the default context:
    the file drivers alternate batches between them so that one batch's copies run beside the next one's kernels."""
    first = default_context(device)
    out = [first]
    for i in range(1, n):
        key = (first.device, i)
        ctx = _extra_ctx.get(key)
        if ctx is None or ctx.handle is None:
            ctx = _extra_ctx[key] = Context(first.device)
        out.append(ctx)
    return out
