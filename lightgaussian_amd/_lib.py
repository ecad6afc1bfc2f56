"""ctypes binding of the C ABI declared in include/lightgaussian.h.

PyTorch is used only for device memory and streams; every compute call goes through
liblightgaussian_hip.so.  There is NO fallback: if the library is missing or a GPU call
fails, this module raises -- it never routes to a CPU/PyTorch implementation.
"""
import ctypes as C
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# LIGHTGAUSSIAN_HIP_LIB: A/B builds of the same library on one GPU box (tools/gpu_ab.sh); always an in-tree HIP build
LIB_PATH = os.environ.get("LIGHTGAUSSIAN_HIP_LIB") or os.path.join(_HERE, "liblightgaussian_hip.so")

LG_OK = 0
LG_ERR_INVALID_ARGUMENT = -1
LG_ERR_DEVICE = -2
LG_ERR_ALLOC = -3
LG_ERR_PREFILTERED = -4

WEIGHT_ONE, WEIGHT_OPACITY, WEIGHT_ALPHA, WEIGHT_ALPHA_T = 0, 1, 2, 3
FLAG_DEBUG, FLAG_FAST_EXP, FLAG_PROFILE, FLAG_RAW_PARAMS, FLAG_SKIP_COLOR, FLAG_L1_ONLY = 1, 2, 4, 8, 16, 32
FLAG_NARROW_KEY, FLAG_SORT_ALL_BITS, FLAG_K1_LDS = 64, 128, 256
FLAG_LONG_SERIAL, FLAG_LONG_PARALLEL = 512, 1024
FLAG_SAVE_SH_JACOBIAN = 2048
FLAG_COUNT_WIDE_BAND = 8192
FLAG_ANTIALIAS = 16384
FLAG_ABSGRAD = 32768       # lg_backward_abs (absolute screen-space mean gradients); ignored by everything else
ADAM_DECOUPLED_WD = 1       # lg_adam_step flags: LG_ADAM_DECOUPLED_WD (AdamW), FLAG_PROFILE
ADAM_MAX_TENSORS = 8        # LG_ADAM_MAX_TENSORS: tensors per launch of lg_adam_step
ADAM_SPAN = 4096            # LG_ADAM_SPAN: elements per workgroup of lg_adam_step
DENSIFY_COPY, DENSIFY_MOMENT, DENSIFY_XYZ, DENSIFY_SCALING, DENSIFY_ZERO = 0, 1, 2, 3, 4     # lg_densify_tensor.role (LG_DENSIFY_*)
DENSIFY_MAX_TENSORS = 32    # LG_DENSIFY_MAX_TENSORS: tensors per lg_densify_rows call
FEATURES_MAX = 64           # LG_FEATURES_MAX: channels per lg_blend_features call
FILTER3D_RAW = 1            # LG_FILTER3D_RAW: lg_filter3d_apply / _bwd on log-scales and opacity logits
ABI_VERSION = 7     # include/lightgaussian.h LG_ABI_VERSION this binding was written against (load() refuses another)


class lg_view(C.Structure):
    _fields_ = [("image_height", C.c_int32), ("image_width", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float),
                ("bg", C.c_void_p), ("scale_modifier", C.c_float), ("viewmatrix", C.c_void_p),
                ("projmatrix", C.c_void_p), ("sh_degree", C.c_int32), ("campos", C.c_void_p),
                ("prefiltered", C.c_int32), ("flags", C.c_uint32), ("segment_length", C.c_int32), ("count_sum", C.c_void_p)]


class lg_gaussians(C.Structure):
    _fields_ = [("N", C.c_int32), ("M", C.c_int32), ("means3D", C.c_void_p), ("shs", C.c_void_p),
                ("colors_precomp", C.c_void_p), ("opacities", C.c_void_p), ("scales", C.c_void_p),
                ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("shs_rest", C.c_void_p)]


class lg_kernel_time(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("total_ms", C.c_double), ("launches", C.c_int64)]


class lg_stats(C.Structure):
    _fields_ = [("num_rendered", C.c_int64), ("num_visible", C.c_int64)]


class lg_adam_tensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("numel", C.c_int64), ("lr", C.c_double), ("weight_decay", C.c_double), ("step", C.c_int64)]


class lg_adam_rows_tensor(C.Structure):
    _fields_ = [("t", lg_adam_tensor), ("row_mask", C.c_void_p), ("rows", C.c_int64)]


class lg_densify_tensor(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_words", C.c_int32), ("role", C.c_int32)]


class lg_filter_camera(C.Structure):
    _fields_ = [("viewmatrix", C.c_float * 16), ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("width", C.c_int32), ("height", C.c_int32)]


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
CHUNK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32)


def build(force=False, verbose=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", src_dir] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL, stderr=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


# The C ABI of include/lightgaussian.h and include/lightgaussian_debug.h, in header order: name -> (restype, argtypes).
# tests/test_abi.py holds every entry against the headers.
i32, i64, u32, f32, f64, sz, vp, P = C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_double, C.c_size_t, C.c_void_p, C.POINTER
_VIEW, _GAUSSIANS = P(lg_view), P(lg_gaussians)
_BACKWARD = (_VIEW, _GAUSSIANS, vp, vp, vp, vp, i64) + (vp,) * 12      # ... dL_dcolor, the nine gradients, scratch, stream
_CHUNKED = _BACKWARD + (i32, CHUNK_FN, vp)
PROTOTYPES = {
    "lg_geom_bytes": (sz, (i32,)),
    "lg_img_bytes": (sz, (i32, i32)),
    "lg_binning_bytes": (sz, (i64, i32, i32, i32)),
    "lg_backward_scratch_bytes": (sz, (i32, i64)),
    "lg_forward": (C.c_int, (_VIEW, _GAUSSIANS, vp, vp, ALLOC_FN, vp, vp, vp, P(vp), P(i64), vp)),
    "lg_forward_count": (C.c_int, (_VIEW, _GAUSSIANS, vp, vp, ALLOC_FN, vp, i32, vp, vp, vp, vp, P(vp), P(i64), vp)),
    "lg_forward_bounded": (C.c_int, (_VIEW, _GAUSSIANS, vp, vp, vp, i64, f32, i32, vp, vp, vp, vp, vp, P(u32 * 4), vp)),
    "lg_backward": (C.c_int, _BACKWARD),
    "lg_sh_grad_from_rgb": (C.c_int, (i32, i32, i32, i32, vp, vp, vp, i64, f32, i32, vp, vp, vp)),
    "lg_backward_chunked": (C.c_int, _CHUNKED),
    "lg_backward_abs": (C.c_int, _CHUNKED + (vp,)),
    "lg_score_from_count": (C.c_int, (i32, vp, vp, vp, vp)),
    "lg_prune_scratch_bytes": (sz, (i32,)),
    "lg_prune_epilogue": (C.c_int, (i32, vp, vp, f32, f64, vp, vp, vp, vp, u32, vp)),
    "lg_select_mask": (C.c_int, (i32, vp, i64, vp, vp, vp, vp)),
    "lg_compact_scratch_bytes": (sz, (i32,)),
    "lg_compact_plan": (C.c_int, (i32, vp, vp, vp, vp, vp)),
    "lg_compact_rows": (C.c_int, (i32, vp, i32, P(vp), P(vp), P(i32), vp)),
    "lg_vq_scratch_bytes": (sz, (i32, i32)),
    "lg_vq_nearest": (C.c_int, (i32, i32, i32, vp, vp, vp, vp, u32, vp)),
    "lg_vq_ema_scratch_bytes": (sz, (i32, i32, i32)),
    "lg_vq_ema_step": (C.c_int, (i32, i32, i32, vp, vp, vp, vp, f64, f64, vp, vp, u32, vp)),
    "lg_vq_colors": (C.c_int, (i32, i32, i32, vp, vp, vp, vp, i32, vp, u32, vp)),
    "lg_vq_code_index_bytes": (sz, (i32, i32)),
    "lg_vq_code_index_scratch_bytes": (sz, (i32, i32)),
    "lg_vq_code_index": (C.c_int, (i32, i32, vp, vp, vp, vp)),
    "lg_vq_colors_bwd_scratch_bytes": (sz, (i32, i32, i32)),
    "lg_vq_colors_bwd": (C.c_int, (i32, i32, i32, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, u32, vp)),
    "lg_adam_step": (C.c_int, (i32, P(lg_adam_tensor), f64, f64, f64, u32, vp)),
    "lg_adam_step_rows": (C.c_int, (i32, P(lg_adam_rows_tensor), f64, f64, f64, u32, vp)),
    "lg_densify_scratch_bytes": (sz, (i32,)),
    "lg_densify_stats": (C.c_int, (i32, vp, vp, vp, vp, vp, vp, u32, vp)),
    "lg_densify_plan": (C.c_int, (i32, vp, vp, vp, vp, f32, f32, f32, f32, i32, vp, vp, vp, u32, vp)),
    "lg_densify_rows": (C.c_int, (i32, i64, vp, vp, i32, P(lg_densify_tensor), vp, vp, vp, i64, u32, vp)),
    "lg_features_scratch_bytes": (sz, (i32, i64, i32)),
    "lg_blend_features": (C.c_int, (_VIEW, i32, vp, vp, i64, vp, i32, vp, vp, vp, vp)),
    "lg_blend_features_backward": (C.c_int, (_VIEW, i32, vp, vp, i64, vp, i32, vp, vp, vp)),
    "lg_backward_features_scratch_bytes": (sz, (i32, i64, i32)),
    "lg_backward_features": (C.c_int, (_VIEW, _GAUSSIANS, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp) + (vp,) * 12),
    "lg_camera_scratch_bytes": (sz, (i32,)),
    "lg_backward_camera": (C.c_int, (_VIEW, _GAUSSIANS, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp)),
    "lg_filter3d_scratch_bytes": (sz, (i32,)),
    "lg_filter3d_update": (C.c_int, (i32, vp, i32, vp, vp, vp, vp, u32, vp)),
    "lg_filter3d_apply": (C.c_int, (i32, vp, vp, vp, vp, vp, u32, vp)),
    "lg_filter3d_apply_bwd": (C.c_int, (i32, vp, vp, vp, vp, vp, vp, vp, u32, vp)),
    "lg_ordered_sum": (C.c_int, (i32, i64, vp, i64, vp, vp)),
    "lg_knn_scratch_bytes": (sz, (i32,)),
    "lg_knn3_mean_dist2": (C.c_int, (i32, vp, vp, vp, u32, vp)),
    "lg_loss_state_bytes": (sz, (i32, i32, i32)),
    "lg_loss_forward": (C.c_int, (i32, i32, i32, vp, vp, vp, vp, u32, vp)),
    "lg_loss_backward": (C.c_int, (i32, i32, i32, vp, vp, vp, vp, f32, vp, f32, vp, u32, vp)),
    "lg_view_status": (C.c_int, (vp, i32, P(u32 * 4), vp)),
    "lg_geom_visible_offset": (sz, (i32,)),
    "lg_abi_version": (C.c_int, ()),
    "lg_last_error": (C.c_char_p, ()),
    "lg_build_id": (C.c_char_p, ()),
    "lg_profile_read": (C.c_int, (P(lg_kernel_time), C.c_int)),
    "lg_profile_reset": (None, ()),
    "lg_last_stats": (C.c_int, (P(lg_stats),)),
    "lg_debug_activations": (C.c_int, (i32, vp, vp, vp, vp, vp, vp, vp)),
    "lg_debug_sort_temp_bytes": (sz, (i64,)),
    "lg_debug_sort_keys": (C.c_int, (i64, vp, vp, i32, i32, vp, vp)),
    "lg_debug_last_contributor": (C.c_int, (_VIEW, i32, vp, vp, vp, i64, vp, vp)),
    "lg_debug_tile_lists": (C.c_int, (_VIEW, vp, i64, vp, vp, vp)),
    "lg_debug_view_meta": (C.c_int, (_VIEW, vp, i64, vp, vp)),
    "lg_debug_sort_orphan": (C.c_int, (i64, vp, vp, vp, vp)),
    "lg_debug_reduce9": (C.c_int, (vp, vp, vp)),
}
EXPORTS = list(PROTOTYPES)

_lib = None
_BOUND = []     # the prototype tables bind() has set


def bind(lib, prototypes):
    """`lib` with the restype / argtypes of a prototype table (name -> (restype, argtypes)) set on it, once per table: the table of
    this module by load(), the table of an extension header by the load() of its module."""
    if not any(t is prototypes for t in _BOUND):
        for name, (restype, argtypes) in prototypes.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        _BOUND.append(prototypes)
    return lib


def load():
    """Load the native library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MI355X rasterizer has no CPU/PyTorch fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950).")
    lib = C.CDLL(LIB_PATH)
    if lib.lg_abi_version() != ABI_VERSION:         # (ctypes' default prototype, int f(void), is this function's)
        raise RuntimeError(f"{LIB_PATH} reports ABI {lib.lg_abi_version()}, this binding needs {ABI_VERSION}: rebuild the library "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
    _lib = bind(lib, PROTOTYPES)
    return lib


def check(rc):
    """Map C error codes onto the reference's Python-side behaviour: invalid argument combos ->
    Exception, device errors -> RuntimeError."""
    if rc == LG_OK:
        return
    msg = load().lg_last_error().decode("utf-8", "replace")
    if rc == LG_ERR_INVALID_ARGUMENT:
        raise Exception(msg)
    raise RuntimeError(f"lightgaussian_hip error {rc}: {msg}")


def ptr(t):
    """The device address of a tensor as a pointer argument; None (NULL) for None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(dev=None):
    """The current stream of `dev` (None: of the current device) as the `stream` argument of a library call."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def scratch(nbytes, dev):
    """A uint8 device buffer for a lg_*_bytes() answer (at least one byte, so that its address is never NULL)."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def profile_flag(on):
    return FLAG_PROFILE if on else 0


def build_id():
    """Identity of the kernel sources the loaded library was built from (see include/lightgaussian.h lg_build_id)."""
    return load().lg_build_id().decode()


def profile_read():
    """Per-kernel hipEvent totals recorded under FLAG_PROFILE: {name: (total_ms, launches)}."""
    lib = load()
    arr = (lg_kernel_time * 32)()
    n = lib.lg_profile_read(arr, 32)
    return {arr[i].name.decode(): (arr[i].total_ms, arr[i].launches) for i in range(min(n, 32))}


def profile_reset():
    load().lg_profile_reset()


def last_stats():
    s = lg_stats()
    load().lg_last_stats(C.byref(s))
    return {"num_rendered": s.num_rendered, "num_visible": s.num_visible}
