"""ctypes binding of libnerf_amd.so (C ABI: include/nerf_amd.h).

There is deliberately NO fallback: if the shared library is missing or a call
fails, a RuntimeError is raised.  The library is built in-tree by
``make -C nerf-simple_amd/csrc`` (or ``__graft_entry__.build()``).
"""
import ctypes
import os
import threading

# torch must be imported BEFORE the library is dlopen'ed: torch ships its own
# HIP runtime (torch/lib/libamdhip64.so) and device pointers only mean something
# inside the runtime that allocated them.  Loaded first, that runtime also
# satisfies libnerf_amd.so's libamdhip64 dependency; loaded second, the process
# would hold two runtimes and every launch would fail with hipErrorNoDevice.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnerf_amd.so")

F32, BF16, FP16, BF16_BWD = 0, 1, 2, 3
FLAG_TS_GIVEN, FLAG_DEVICE_RNG, FLAG_SEED_IN_MEMORY = 1, 2, 4
FLAG_STORE_E4M3 = 8          # nerf_amd_mlp_forward_train: the 8-bit storage form of the saved activations
FLAG_OUTSIDE_EMPTY = 16      # nerf_amd_occupancy_mark: a sample outside the occupancy grid is dead
STATUS_NONFINITE, STATUS_WEIGHT_RANGE = 1, 2
_PRECISIONS = {"fp32": F32, "f32": F32, "float32": F32, F32: F32,
               "bf16": BF16, "bfloat16": BF16, BF16: BF16,
               "fp16": FP16, "f16": FP16, "float16": FP16, "half": FP16, FP16: FP16,
               "bf16_bwd": BF16_BWD, BF16_BWD: BF16_BWD}     # the backward kernel's transposed image

_lib = None
_lock = threading.Lock()

_vp, _i64, _i32, _u32, _u64 = (ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                               ctypes.c_uint32, ctypes.c_uint64)
_SIGNATURES = {
    # name: (restype, argtypes)
    "nerf_amd_abi_version": (_i32, []),
    "nerf_amd_param_count": (_i64, []),
    "nerf_amd_packed_bytes": (_i64, [_i32]),
    "nerf_amd_render_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "nerf_amd_packed_status_offset": (_i64, [_i32]),
    "nerf_amd_query_points": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_grad_bucket_range": (_i32, [_i32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "nerf_amd_param_gradients_finish_bucket": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_layout_selfcheck": (_i32, []),
    "nerf_amd_layout_src_col": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "nerf_amd_pack_weights": (_i32, [_vp, _vp, _i32, _vp]),
    "nerf_amd_gamma": (_i32, [_vp, _i64, _vp, _i64, _i32, _vp]),
    "nerf_amd_positional_encoder": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "nerf_amd_mlp_forward": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render_pixels": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render_backward": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render_rays": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render_rays_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render_mse_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_param_gradients_begin": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_param_gradients_finish": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_pack_weights_train": (_i32, [_vp, _vp, _vp, _vp]),
    "nerf_amd_mse_loss": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_mlp_forward_train_points": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_encode_points_bf16": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_sample_encode": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_generate_rays": (_i32, [_vp, _i32, _i32, ctypes.c_float, _i64, _i64, _vp, _vp]),
    "nerf_amd_render_image_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "nerf_amd_render_image_forward": (_i32, [_vp, _i32, _i32, ctypes.c_float, _i64, _i64, _vp, _vp, _vp, _i32,
                                             _u32, _u64, _vp, _vp, _i32, _vp]),
    "nerf_amd_sample_pdf": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _i64, _i32, _i32, _vp]),
    "nerf_amd_sample_pdf_volume": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _i64, _i32, _i32, _vp]),
    "nerf_amd_sample_pdf_volume_masked": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _i64, _i64, _i64, _vp, _vp,
                                                 _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                 _i64, _i32, _i32, _vp]),
    "nerf_amd_volume_render_mse_backward_pdf": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _i64,
                                                       _i32, _i32, _vp]),
    "nerf_amd_sigma_noise": (_i32, [_vp, _vp, ctypes.c_float, _u32, _u64, _vp, _i64, _i64, _i32, _vp]),
    "nerf_amd_background_blend": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "nerf_amd_background_blend_backward": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "nerf_amd_volume_render_mse_backward_bg": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_float, _u32, _u64, _vp, _i64,
                                                      _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_distortion_loss": (_i32, [_vp, _vp, ctypes.c_float, ctypes.c_float, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_sum_f32": (_i32, [_vp, _vp, _i64, _vp]),
    "nerf_amd_volume_render_mse_backward_dist": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_float, _u32, _u64, _vp, _i64,
                                                        ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_render_hierarchical_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "nerf_amd_render_hierarchical_forward": (_i32, [_vp, _i32, _i32, ctypes.c_float, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                                                    _i32, _u32, _u64, _vp, _vp, _i32, _i32, _vp]),
    "nerf_amd_train_activation_bytes": (_i64, [_i64]),
    "nerf_amd_mlp_forward_train": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_mlp_backward": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_train_activation_bytes_e4m3": (_i64, [_i64]),
    "nerf_amd_train_gradient_bytes_e4m3": (_i64, [_i64]),
    "nerf_amd_param_gradients_scratch_e4m3_bytes": (_i64, [_i64]),
    "nerf_amd_mlp_backward_e4m3": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_param_gradients_convert_e4m3": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_param_gradients_finish_e4m3": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_sample_encode_bf16": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_param_gradients_scratch_bytes": (_i64, [_i64]),
    "nerf_amd_param_gradients": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_adam_step": (_i32, [_vp, _vp, _vp, _vp, _i64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                  ctypes.c_float, _i64, _vp]),
    "nerf_amd_mt19937_uniform": (_i32, [_vp, _i32, _vp, _i64, _vp, _vp]),
    "nerf_amd_mt19937_segments": (_i64, [_i32, _i64, _i64]),
    "nerf_amd_mt19937_uniform_par": (_i32, [_vp, _i32, _vp, _i64, _vp, _vp, _i32, _i64, _vp, _vp]),
    "nerf_amd_adam_step_hyper": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "nerf_amd_hyper_fetch": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "nerf_amd_pinned_device_address": (_i64, [_vp]),
    "nerf_amd_range_check": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _i64, _i32, _vp]),
    "nerf_amd_mt19937_raw": (_i32, [_vp, _i32, _vp, _i64, _vp, _vp]),
    "nerf_amd_mt19937_jump_poly": (_i32, [_i64, _vp, _vp]),
    "nerf_amd_mt19937_advance": (_i32, [_vp, _vp, _vp, _vp]),
    "nerf_amd_mt19937_uniform_after": (_i32, [_vp, _vp, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp]),
    "nerf_amd_select_workspace_bytes": (_i64, [_i64]),
    "nerf_amd_select_rays": (_i32, [_vp, _u64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nerf_amd_linear_f32": (_i32, [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _u32, _vp]),
    "nerf_amd_render_forward": (_i32, [_vp, _vp, _vp, _vp, _i32, _u32, _u64, _i64,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_render_pixels_forward": (_i32, [_vp, _vp, _vp, _vp, _i32, _u32, _u64, _i64,
                                              _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_mlp_forward_rays": (_i32, [_vp, _vp, _vp, _vp, _i32, _u32, _u64, _i64,
                                         _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_input_gradients": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_query_points_backward": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_gamma_backward": (_i32, [_vp, _i64, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_positional_encoder_backward": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "nerf_amd_camera_rays": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, ctypes.c_float, _vp, _i64, _i64, _vp]),
    "nerf_amd_camera_workspace_bytes": (_i64, [_i64, _i64]),
    "nerf_amd_camera_rays_backward": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, ctypes.c_float, _vp, _vp, _i64, _i64, _vp]),
    "nerf_amd_camera_poses": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "nerf_amd_image_metrics_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "nerf_amd_image_metrics": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "nerf_amd_density_forward": (_i32, [_vp, _i64, _vp, _i32, _vp, _i64, _vp]),
    "nerf_amd_density_grid": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp]),
    "nerf_amd_grid_points": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "nerf_amd_marching_cubes_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "nerf_amd_marching_cubes_count": (_i32, [_vp, _i64, _i64, _i64, ctypes.c_float, _vp, _vp, _vp]),
    "nerf_amd_marching_cubes_emit": (_i32, [_vp, _i64, _i64, _i64, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _i64, _i64, _vp]),
    "nerf_amd_occupancy_grid_words": (_i64, [_i64, _i64, _i64]),
    "nerf_amd_occupancy_from_density": (_i32, [_vp, _i64, _i64, _i64, ctypes.c_float, _i32, _vp, _vp]),
    "nerf_amd_occupancy_from_mask": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp]),
    "nerf_amd_occupancy_mask_words": (_i64, [_i64, _i32]),
    "nerf_amd_occupancy_workspace_bytes": (_i64, [_i64]),
    "nerf_amd_occupancy_mark": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _i64, _i32, _vp]),
    "nerf_amd_occupancy_points": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    "nerf_amd_volume_render_masked": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                             _i32, _vp]),
    "nerf_amd_volume_render_masked_pixels": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_termination_workspace_bytes": (_i64, [_i64]),
    "nerf_amd_termination_advance": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _i64,
                                            ctypes.c_float, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render_masked_backward": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                      _vp, _i64, _i32, _vp]),
    "nerf_amd_occupancy_decay_max": (_i32, [_vp, _vp, ctypes.c_float, _i64, _vp]),
    "nerf_amd_occupancy_points_capped": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    "nerf_amd_volume_render_masked_mse_backward": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _vp, _vp, _i64,
                                                          _i64, _i32, _vp]),
    "nerf_amd_appearance_gather": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp]),
    "nerf_amd_appearance_apply": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp]),
    "nerf_amd_appearance_apply_backward": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "nerf_amd_appearance_reduce": (_i32, [_vp, _vp, _i64, _vp, ctypes.c_float, _vp, _vp, _i64, _i64, _vp]),
    "nerf_amd_volume_render_mse_backward_affine": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_sigma_noise_masked": (_i32, [_vp, _vp, ctypes.c_float, _u32, _u64, _vp, _i64, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render_masked_mse_backward_dist": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _vp, _i64,
                                                               ctypes.c_float, _u32, _u64, _vp, ctypes.c_float, ctypes.c_float,
                                                               _vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    "nerf_amd_box_positions": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp,
                                      _i64, _i32, _vp]),
    "nerf_amd_span_positions": (_i32, [_vp, _vp, _vp, _u32, _u64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _i32,
                                       ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _i64, _i32, _vp]),
    "nerf_amd_volume_render_mse_backward_pdf_bg": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_float, _u32, _u64, _vp, _vp,
                                                          _u32, _u64, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "nerf_amd_volume_render_masked_mse_backward_pdf_bg": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _vp, _i64,
                                                                 ctypes.c_float, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                                                 _i32, _i32, _vp]),
    "nerf_amd_grad_guard_workspace_bytes": (_i64, [_i64]),
    "nerf_amd_grad_guard": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "nerf_amd_adam_step_guarded": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "nerf_amd_volume_render_masked_mse_backward_pdf": (_i32, [_vp, _vp, _vp, _vp, _u32, _u64, _i64, _vp, _vp, _vp, _vp, _vp,
                                                              _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
}
EXPORTS = tuple(_SIGNATURES)


def precision_code(p):
    try:
        return _PRECISIONS[p]
    except KeyError:
        raise ValueError(f"precision must be 'fp32', 'bf16' or 'fp16', got {p!r}") from None


def lib():
    """The loaded library (loads on first use; raises if it is not built)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} is missing: build the HIP library with "
                        "`make -C nerf-simple_amd/csrc` (there is no CPU fallback)")
                h = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in _SIGNATURES.items():
                    fn = getattr(h, name)          # AttributeError if an export is missing
                    fn.restype, fn.argtypes = res, args
                if h.nerf_amd_abi_version() != 5:
                    raise RuntimeError("libnerf_amd.so ABI version mismatch")
                _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        kind = {-1: "invalid argument", -2: "unsupported configuration"}.get(rc, f"hipError_t {rc}")
        raise RuntimeError(f"{what} failed: {kind}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def launch(name, *args, dev=None, stream=None):
    """Enqueue the C entry point ``name``: the one way the package calls into the library.  ``args``
    are the ABI's arguments in the ABI's order without the trailing stream: a tensor goes as its device pointer, None as
    NULL, everything else (ints, floats, raw addresses, host float triples) as it is, for the declared argtypes to convert.
    ``stream`` (a stream pointer): the caller has fixed device and stream, as a captured sequence has.  Without one the
    launch goes on the current stream of ``dev``, under its device guard.  A non-zero status raises under ``name``."""
    argv = [a.data_ptr() if torch.is_tensor(a) else a for a in args]
    if stream is not None:
        return check(getattr(lib(), name)(*argv, stream), name)
    with torch.cuda.device(dev):
        check(getattr(lib(), name)(*argv, torch.cuda.current_stream(dev).cuda_stream), name)


def host_f32x3(v):
    """Three host floats as a launcher's ``const float*`` argument (read before the call returns)."""
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def grad_bucket_range(bucket):
    """(first, count) of exchange bucket ``bucket`` inside the flat gradient vector (nerf_amd_grad_bucket_range)."""
    first, count = ctypes.c_int64(), ctypes.c_int64()
    check(lib().nerf_amd_grad_bucket_range(bucket, ctypes.byref(first), ctypes.byref(count)), "nerf_amd_grad_bucket_range")
    return first.value, count.value


def require_cuda_f32(t, name):
    """The kernels take fp32, contiguous, device-resident tensors; anything
    else is an error (the reference's callers do .cuda() themselves,
    utils/rendering.py:102, train.py:51)."""
    if not torch.is_tensor(t):
        raise AssertionError(f"{name} needs to be a torch tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got a {t.device} tensor); "
                           "this package has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    return t


# ---- the entry points' argument rules, each stated once ---------------------------------------------
def require_rays(rays):
    """rays [B, 6], float32 on the GPU -> B."""
    require_cuda_f32(rays, "rays")
    if rays.dim() != 2 or rays.shape[1] != 6:
        raise RuntimeError("rays must be [B, 6]")
    return rays.size(0)


def require_shape(t, name, shape):
    """An optional per-ray argument (None passes): float32 on the GPU and exactly ``shape`` = (B, n)."""
    if t is not None and tuple(require_cuda_f32(t, name).shape) != tuple(shape):
        raise RuntimeError(f"{name} must be [B, {shape[1]}]")
    return t


def require_same_device(what, tensor, dev):
    """``tensor`` (of the occupancy grid, the proposal volume) sits where the rays do."""
    if tensor.device != dev:
        raise RuntimeError(f"the {what} lives on {tensor.device}, the rays on {dev}")


def require_pair_sizes(Nc, Nf):
    """nerf_amd_sample_pdf's sample counts for a coarse / fine pair."""
    if Nc < 3 or Nc > 256 or Nf < 0 or Nc + Nf > 512:
        raise ValueError(f"hierarchical sampling needs 3 <= Nc <= 256 and Nc + Nf <= 512 (got Nc={Nc}, Nf={Nf})")


def precision_of(net, precision):
    """The precision code of a call: the module's own unless the call names one."""
    return precision_code(net.precision if precision is None else precision)


def workspace(nbytes, dev, floor=256):
    """A scratch buffer of ``nbytes`` (at least ``floor``) on ``dev``; ``floor=0``: None for an entry point that needs none
    (nerf_amd_render_workspace_bytes is 0 for the one-launch render, which takes NULL)."""
    n = max(int(nbytes), floor) if floor else int(nbytes)
    return torch.empty(n, dtype=torch.uint8, device=dev) if n else None
