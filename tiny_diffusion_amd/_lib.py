"""ctypes binding of libtdx.so (include/tdx.h).

There is no CPU fallback: if the library is missing or fails to load, importing
this module raises.  The library is linked against ``libamdhip64.so.7``; torch is
imported first so that the HIP runtime torch already mapped (same SONAME) is
the one libtdx binds to - streams and device pointers are then shared.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import torch  # noqa: F401  (must precede the dlopen below)

from . import _build

_c_float_p = C.c_void_p
_c_i64_p = C.c_void_p
_ptr = C.c_void_p


class TdxError(RuntimeError):
    pass


def _load():
    path = _build.LIB
    if not os.path.exists(path):
        if os.environ.get("TDX_NO_AUTOBUILD"):
            raise TdxError(
                f"{path} not found: build it with `python -m tiny_diffusion_amd._build` "
                "(there is no CPU fallback for the HIP path)"
            )
        _build.build()
    elif _build.stamp_mismatch() and not os.environ.get("TDX_NO_AUTOBUILD"):
        _build.build(force=False)  # the sources changed since the library was linked
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    # one HIP runtime per process, or streams/pointers would not be shared
    hips = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    hips.add(os.path.realpath(line.split()[-1]))
    except OSError:
        pass
    if len(hips) > 1:
        raise TdxError(f"two HIP runtimes mapped in one process: {sorted(hips)}")
    return lib


lib = _load()

_SIGS = {
    "tdx_version": (C.c_int, []),
    "tdx_error_string": (C.c_char_p, [C.c_int]),
    "tdx_q_sample": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_q_sample_philox": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int,
                                      C.c_uint64, C.c_uint64, _ptr]),
    "tdx_q_sample_target": (C.c_int, [_ptr] * 7 + [C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_q_sample_target_philox": (C.c_int, [_ptr] * 6 + [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _ptr]),
    "tdx_p_sample_step": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int64, _ptr]),
    "tdx_p_sample_step_philox": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, C.c_int64, C.c_uint64, _ptr]),
    "tdx_u8_gather_normalize": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_float, C.c_float, _ptr]),
    "tdx_mse_loss": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_float, C.c_int64, _ptr]),
    "tdx_mse_scratch_bytes": (C.c_size_t, []),
    "tdx_mse_loss_grad": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_float, C.c_int64, _ptr, _ptr]),
    "tdx_mse_loss_grad_weighted": (C.c_int, [_ptr] * 6 + [C.c_float, C.c_int, C.c_int, _ptr, _ptr]),
    "tdx_timestep_cdf": (C.c_int, [_ptr, _ptr, C.c_int, _ptr, _ptr, C.c_int, _ptr]),
    "tdx_timestep_draw": (C.c_int, [_ptr, C.c_int, _ptr, _ptr, C.c_int, C.c_uint64, C.c_uint64, _ptr, _ptr]),
    "tdx_mse_per_sample": (C.c_int, [_ptr] * 5 + [C.c_int, C.c_int, _ptr]),
    "tdx_timestep_history_update": (C.c_int, [_ptr, _ptr, C.c_int, _ptr, _ptr, C.c_int, C.c_float, _ptr, _ptr, _ptr,
                                              C.c_int, _ptr]),
    "tdx_distill_teacher_step": (C.c_int, [_ptr] * 8 + [C.c_int, C.c_int, C.c_float, C.c_float, _ptr]),
    "tdx_distill_target": (C.c_int, [_ptr] * 8 + [C.c_int, C.c_int, C.c_float, C.c_float, _ptr]),
    "tdx_distill_teacher_step_guided": (C.c_int, [_ptr] * 8 + [C.c_int, C.c_int] + [C.c_float] * 3 + [_ptr]),
    "tdx_distill_target_guided": (C.c_int, [_ptr] * 8 + [C.c_int, C.c_int] + [C.c_float] * 3 + [_ptr]),
    "tdx_distill_guidance_target": (C.c_int, [_ptr] * 6 + [C.c_int, C.c_int, C.c_int] + [C.c_float] * 3 + [_ptr]),
    "tdx_adam_step": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int64, C.c_float, C.c_float, C.c_float,
                                C.c_float, C.c_int, C.c_float, _ptr]),
    "tdx_adam_clip_scratch_bytes": (C.c_size_t, []),
    "tdx_adam_step_clip": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_int, C.c_float, C.c_float, _ptr, _ptr, _ptr]),
    "tdx_adam_ema_step": (C.c_int, [_ptr] * 5 + [C.c_int64] + [C.c_float] * 4 + [C.c_int, C.c_float, C.c_float, _ptr]),
    "tdx_adam_ema_step_dev": (C.c_int, [_ptr] * 5 + [C.c_int64, _ptr, C.c_float, C.c_float, C.c_float, _ptr]),
    "tdx_adam_ema_step_clip": (C.c_int, [_ptr] * 5 + [C.c_int64] + [C.c_float] * 4 + [C.c_int] + [C.c_float] * 3
                               + [_ptr, _ptr, _ptr]),
    "tdx_swap_f32": (C.c_int, [_ptr, _ptr, C.c_int64, _ptr]),
    "tdx_edge_conv_wgrad_scratch_floats": (C.c_size_t, [C.c_int] * 3),
    "tdx_initial_conv_forward": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_initial_conv_backward": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            _ptr]),
    "tdx_final_conv_forward": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_final_conv_backward": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                          _ptr]),
    "tdx_pack_conv3x3": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_conv3x3_wino_ok": (C.c_int, [C.c_int] * 5),
    "tdx_pack_conv3x3_wino": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_conv3x3_fwd_wino": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ptr,
                                       _ptr, _ptr, _ptr]),
    "tdx_conv3x3_fwd_wino_infer": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ptr, _ptr,
                                             _ptr, C.c_size_t, _ptr]),
    "tdx_conv3x3_train_algo": (C.c_int, [C.c_int] * 6),
    "tdx_conv3x3_infer_algo": (C.c_int, [C.c_int] * 5),
    "tdx_conv3x3_wgrad_wino_splits": (C.c_int, [C.c_int] * 5),
    "tdx_conv3x3_wgrad_wino": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_conv3x3_wino_stat_tiles": (C.c_int, [C.c_int] * 3),
    "tdx_conv3x3_wino_stat_tile_rows": (C.c_int, [C.c_int] * 3),
    "tdx_pack_conv3x3_tiled": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_conv3x3_fwd_infer": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ptr, _ptr,
                                        _ptr, C.c_size_t, _ptr]),
    "tdx_conv3x3_infer_scratch_floats": (C.c_size_t, [C.c_int] * 5),
    "tdx_conv3x3_fwd": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "tdx_conv3x3_fwd_splitk": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_size_t, _ptr]),
    "tdx_conv3x3_splitk_scratch_floats": (C.c_size_t, [C.c_int] * 5),
    "tdx_conv3x3_fwd_train": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        _ptr, _ptr, C.c_size_t, _ptr]),
    "tdx_conv3x3_train_scratch_floats": (C.c_size_t, [C.c_int] * 5),
    "tdx_conv3x3_stat_tiles": (C.c_int, [C.c_int] * 5),
    "tdx_conv3x3_stat_tile_rows": (C.c_int, [C.c_int] * 5),
    "tdx_conv3x3_wgrad_splits": (C.c_int, [C.c_int] * 5),
    "tdx_diag_conv_occupancy": (C.c_int, [C.c_int]),
    "tdx_conv3x3_wgrad_splits_bf16": (C.c_int, [C.c_int] * 5),
    "tdx_conv3x3_fwd_bf16_io": (C.c_int, [_ptr] * 4 + [C.c_int] * 6 + [_ptr] * 5 + [C.c_int, _ptr]),
    "tdx_conv3x3_wgrad_bf16_io": (C.c_int, [_ptr] * 3 + [C.c_int] * 6 + [_ptr] * 2 + [C.c_int, _ptr]),
    "tdx_conv3x3_shape_ok": (C.c_int, [C.c_int] * 5),
    "tdx_conv3x3_tile_shape": (C.c_int, [C.c_int] * 6),
    "tdx_conv3x3_wgrad": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, _ptr, _ptr, _ptr]),
    "tdx_conv3x3_wgrad_reduce": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_bn_finalize": (C.c_int, [_ptr, C.c_int, C.c_int, C.c_int64, C.c_int, _ptr, _ptr, _ptr, _ptr, _ptr,
                                  _ptr, _ptr, _ptr, _ptr, C.c_int, _ptr]),
    "tdx_bn_relu_bwd": (C.c_int, [_ptr, _ptr, C.c_int64, C.c_int, _ptr, _ptr, _ptr, _ptr, _ptr,
                                  _ptr, _ptr, _ptr, _ptr, C.c_int, _ptr]),
    "tdx_bn_relu_bwd_scratch_floats": (C.c_size_t, [C.c_int64, C.c_int]),
    "tdx_maxpool2_ceil_fwd": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_maxpool2_ceil_bwd": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int,
                                        C.c_int, _ptr]),
    "tdx_bilinear_ac_fwd": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_bilinear_ac_bwd": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, _ptr]),
    # the storage-flag (_io) forms and the sum-emitting producers (io16 last before the stream)
    "tdx_bn_apply_relu_fwd_io": (C.c_int, [_ptr, _ptr, C.c_int64, C.c_int, _ptr, _ptr, C.c_int, _ptr]),
    "tdx_bn_relu_bwd_io": (C.c_int, [_ptr, _ptr, C.c_int64, C.c_int] + [_ptr] * 9 + [C.c_int, C.c_int, _ptr]),
    "tdx_bn_relu_bwd_from_partials": (C.c_int, [_ptr, _ptr, C.c_int64, C.c_int] + [_ptr] * 9
                                      + [C.c_int, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_maxpool2_ceil_fwd_io": (C.c_int, [_ptr] * 4 + [C.c_int] * 5 + [_ptr]),
    "tdx_maxpool2_ceil_bwd_io": (C.c_int, [_ptr] * 6 + [C.c_int] * 4 + [_ptr, _ptr, _ptr, C.POINTER(C.c_int), C.c_int,
                                                                        _ptr]),
    "tdx_bilinear_ac_fwd_io": (C.c_int, [_ptr] * 5 + [C.c_int] * 9 + [_ptr]),
    "tdx_bilinear_ac_bwd_io": (C.c_int, [_ptr, _ptr] + [C.c_int] * 8 + [_ptr] * 6 + [C.POINTER(C.c_int), C.c_int, _ptr]),
    "tdx_bilinear_pair_fwd_io": (C.c_int, [_ptr, _ptr, C.c_int, C.c_size_t, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int,
                                           _ptr, _ptr, C.c_int, C.c_int, C.c_int, _ptr, C.c_int, C.c_int, C.c_int,
                                           C.c_int, _ptr]),
    "tdx_pixel_sum_io": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_initial_conv_forward_io": (C.c_int, [_ptr] * 4 + [C.c_int] * 6 + [_ptr]),
    "tdx_initial_conv_backward_io": (C.c_int, [_ptr] * 5 + [C.c_int] * 6 + [_ptr]),
    "tdx_initial_conv_input_grad_io": (C.c_int, [_ptr] * 3 + [C.c_int] * 6 + [_ptr]),
    "tdx_final_conv_forward_io": (C.c_int, [_ptr] * 4 + [C.c_int] * 5 + [_ptr]),
    "tdx_final_conv_backward_io": (C.c_int, [_ptr] * 7 + [C.c_int] * 5 + [_ptr]),
    "tdx_adam_step_dev": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int64, _ptr, C.c_float, C.c_float, C.c_float, _ptr]),
    "tdx_step_begin": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, _ptr]),
    "tdx_step_begin_sched": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, _ptr]),
    "tdx_p_sample_step_sched": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int64, _ptr]),
    "tdx_p_sample_step_sched_philox": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int64, C.c_uint64, _ptr]),
    "tdx_linear_fwd": (C.c_int, [_ptr, C.c_int, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_linear_bwd": (C.c_int, [_ptr, C.c_int, _ptr, C.c_int, _ptr, _ptr, C.c_int, _ptr, _ptr, C.c_int, C.c_int,
                                 C.c_int, _ptr]),
    "tdx_linear_fwd_prec": (C.c_int, [_ptr, C.c_int, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      _ptr]),
    "tdx_linear_bwd_prec": (C.c_int, [_ptr, C.c_int, _ptr, C.c_int, _ptr, _ptr, C.c_int, _ptr, _ptr, C.c_int, C.c_int,
                                      C.c_int, C.c_int, _ptr]),
    "tdx_vae_workspace_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "tdx_vae_encode": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_vae_reparameterize": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int64, _ptr]),
    "tdx_vae_decode": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_vae_loss_scratch_bytes": (C.c_size_t, []),
    "tdx_vae_bce_logits_grad": (C.c_int, [_ptr] * 5 + [C.c_float, C.c_int64, _ptr, _ptr]),
    "tdx_vae_kld_reparam_bwd": (C.c_int, [_ptr] * 7 + [C.c_float, C.c_int64, _ptr, _ptr]),
    "tdx_vae_reparameterize_philox": (C.c_int, [_ptr] * 4 + [C.c_int64, C.c_uint64, C.c_uint64, _ptr]),
    "tdx_vae_train_workspace_floats": (C.c_size_t, [C.c_int] * 4),
    "tdx_vae_loss_grads": (C.c_int, [_ptr] * 4 + [C.c_uint64, C.c_uint64, C.c_float, C.c_float, _ptr, _ptr]
                           + [C.c_int] * 4 + [_ptr]),
    "tdx_layernorm_fwd": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_float, _ptr]),
    "tdx_layernorm_bwd": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_act_fwd": (C.c_int, [_ptr, _ptr, C.c_int64, C.c_int, _ptr]),
    "tdx_act_bwd": (C.c_int, [_ptr, _ptr, _ptr, C.c_int64, C.c_int, _ptr]),
    "tdx_dropout": (C.c_int, [_ptr, _ptr, C.c_int64, C.c_int, C.c_float, C.c_uint64, C.c_uint64, _ptr]),
    "tdx_add": (C.c_int, [_ptr, _ptr, _ptr, C.c_int64, C.c_int64, _ptr]),
    "tdx_embedding_fwd": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_embedding_bwd": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_transformer_train_workspace_floats": (C.c_size_t, [_ptr]),
    "tdx_transformer_loss_grads": (C.c_int, [_ptr] * 8 + [C.c_int, C.c_uint64, C.c_uint64, _ptr, C.c_float] + [_ptr] * 4),
    "tdx_unet_create": (C.c_int, [C.POINTER(_ptr), C.c_int, C.c_int]),
    "tdx_unet_create_ex": (C.c_int, [C.POINTER(_ptr), C.c_int, C.c_int, C.c_int]),
    "tdx_unet_create_hw": (C.c_int, [C.POINTER(_ptr), C.c_int, C.c_int, C.c_int, C.c_int]),
    "tdx_unet_create_full": (C.c_int, [C.POINTER(_ptr), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tdx_unet_set_bn_sync": (C.c_int, [_ptr, _ptr, _ptr, _ptr]),
    "tdx_unet_set_streams": (C.c_int, [_ptr, C.c_int]),
    "tdx_unet_set_precision": (C.c_int, [_ptr, C.c_int]),
    "tdx_pack_conv3x3_bf16": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_conv3x3_bf16_stat_tile_rows": (C.c_int, []),
    "tdx_conv3x3_fwd_bf16": (C.c_int, [_ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "tdx_conv3x3_wgrad_bf16": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, _ptr, _ptr, _ptr]),
    "tdx_unet_destroy": (C.c_int, [_ptr]),
    "tdx_unet_workspace_bytes": (C.c_size_t, [_ptr, C.c_int, C.c_int]),
    "tdx_unet_forward": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_size_t, C.c_int,
                                   C.c_int, _ptr]),
    "tdx_unet_backward_stages": (C.c_int, []),
    "tdx_unet_backward": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                    _ptr]),
    "tdx_unet_backward_join": (C.c_int, [_ptr, _ptr]),
    "tdx_unet_backward_mark": (C.c_int, [_ptr, C.c_int]),
    "tdx_unet_backward_wait_mark": (C.c_int, [_ptr, C.c_int, _ptr]),
    "tdx_unet_backward_sync_mark": (C.c_int, [_ptr, C.c_int]),
    "tdx_unet_request_input_grad": (C.c_int, [_ptr, _ptr]),
    "tdx_unet_prepare_sampling": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_unet_drop_sampling_tables": (C.c_int, [_ptr]),
    "tdx_unet_prepare_sampling_sched": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, _ptr, C.c_int, _ptr]),
    "tdx_initial_conv_input_grad": (C.c_int, [_ptr, _ptr, _ptr] + [C.c_int] * 5 + [_ptr]),
    "tdx_unet_eval_step": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int64,
                                     _ptr, C.c_size_t, C.c_int, C.c_uint64, _ptr]),
    "tdx_unet_eval_step_update": (C.c_int, [_ptr] * 8 + [C.c_int, _ptr, _ptr, _ptr, _ptr, C.c_int64, _ptr, C.c_size_t,
                                            C.c_int, C.c_uint64, C.c_int, C.c_int] + [C.c_float] * 3 + [_ptr] * 4),
    "tdx_p_sample_update": (C.c_int, [_ptr, _ptr, _ptr, C.c_int64, C.c_int, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_uint64,
                                      C.c_int, C.c_float, C.c_float, C.c_float, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "tdx_x0_dyn_threshold": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, _ptr, _ptr, C.c_int, C.c_float, C.c_float, C.c_float,
                                       C.c_int, C.c_float, _ptr, _ptr]),
    "tdx_p_sample_update_dyn": (C.c_int, [_ptr, _ptr, _ptr, C.c_int64, C.c_int, _ptr, _ptr, _ptr, _ptr, C.c_int,
                                          C.c_uint64, C.c_int, C.c_float, C.c_float, C.c_float, _ptr, _ptr, _ptr, _ptr,
                                          _ptr, C.c_int, _ptr]),
    "tdx_unet_eval_step_update_dyn": (C.c_int, [_ptr] * 8 + [C.c_int, _ptr, _ptr, _ptr, _ptr, C.c_int64, _ptr, C.c_size_t,
                                                C.c_int, C.c_uint64, C.c_int, C.c_int] + [C.c_float] * 3 + [_ptr] * 3
                                      + [C.c_int, C.c_float, _ptr, _ptr]),
    "tdx_vlb_terms": (C.c_int, [_ptr] * 6 + [C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_int, _ptr, C.c_int64, _ptr]),
    "tdx_eps_sqnorm": (C.c_int, [_ptr] * 4 + [C.c_int, C.c_int, _ptr, C.c_int64, _ptr]),
    "tdx_p_sample_step_guided": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int64, C.c_float, C.c_int,
                                           C.c_uint64, _ptr, _ptr]),
    "tdx_p_sample_step_x0": (C.c_int, [_ptr] * 7 + [C.c_int64, C.c_float, C.c_float, C.c_int, C.c_uint64, _ptr, _ptr]),
    "tdx_p_sample_step_x0_guided": (C.c_int, [_ptr] * 6 + [C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int,
                                                           C.c_uint64, _ptr, _ptr]),
    "tdx_p_sample_step_ms": (C.c_int, [_ptr] * 6 + [C.c_int64, C.c_float, C.c_float, _ptr, _ptr]),
    "tdx_p_sample_step_ms_guided": (C.c_int, [_ptr] * 5 + [C.c_int64, C.c_float, C.c_float, C.c_float, _ptr, _ptr]),
    "tdx_p_sample_step_x0_masked": (C.c_int, [_ptr] * 9 + [C.c_int64, C.c_float, C.c_float, C.c_int, C.c_uint64, _ptr,
                                                           _ptr]),
    "tdx_p_sample_step_x0_guided_masked": (C.c_int, [_ptr] * 8 + [C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int,
                                                                  C.c_uint64, _ptr, _ptr]),
    "tdx_p_sample_step_ms_masked": (C.c_int, [_ptr] * 8 + [C.c_int64, C.c_float, C.c_float, _ptr, _ptr]),
    "tdx_p_sample_step_ms_guided_masked": (C.c_int, [_ptr] * 7 + [C.c_int64, C.c_float, C.c_float, C.c_float, _ptr,
                                                                  _ptr]),
    "tdx_cond_drop_labels": (C.c_int, [_ptr, _ptr, C.c_int, C.c_float, C.c_uint64, C.c_uint64, _ptr]),
    "tdx_cond_drop_rows": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, _ptr]),
    "tdx_timestep_embedding": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_timestep_embedding_f32": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, _ptr]),
    "tdx_time_mlp_fwd": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, _ptr]),
    "tdx_time_mlp_bwd": (C.c_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, C.c_int, C.c_int,
                                   _ptr]),
    "tdx_time_path_fwd": (C.c_int, [C.c_int, C.c_int] + [_ptr] * 9 + [C.c_int, _ptr]),
    "tdx_time_path_bwd": (C.c_int, [C.c_int, C.c_int, C.c_int] + [_ptr] * 10 + [C.c_int, C.c_int, _ptr]),
    "tdx_time_path_proj_bwd": (C.c_int, [C.c_int, C.c_int, C.c_int] + [_ptr] * 5 + [C.c_int, _ptr]),
    "tdx_conv3x3_dgrad": (C.c_int, [_ptr, _ptr, _ptr, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ptr]),
    "tdx_bn_apply_relu_fwd": (C.c_int, [_ptr, _ptr, C.c_int64, C.c_int, _ptr, _ptr, _ptr]),
    "tdx_unet_pack": (C.c_int, [_ptr, _ptr, _ptr, _ptr]),
    "tdx_unet_tensor": (C.c_int, [_ptr, C.c_int, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "tdx_tune_set": (C.c_int, [C.c_char_p, C.c_int]),
    "tdx_tune_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "tdx_tune_name": (C.c_char_p, [C.c_int]),
    "tdx_diag_set_buffer": (C.c_int, [_ptr, C.c_size_t]),
    "tdx_probe_mfma_f32": (C.c_int, [_ptr, C.c_int, C.c_int, _ptr]),
    "tdx_probe_stream_copy": (C.c_int, [_ptr, _ptr, C.c_int64, _ptr]),
    # the pairwise kernels of the sample-quality metrics (metrics.hip)
    "tdx_pair_scratch_bytes": (C.c_size_t, [C.c_int] * 4),
    "tdx_pair_gram": (C.c_int, [_ptr, _ptr, C.c_int, C.c_int, C.c_int, _ptr, _ptr]),
    "tdx_pair_kth_dist2": (C.c_int, [_ptr, _ptr] + [C.c_int] * 6 + [_ptr, _ptr, C.c_size_t, _ptr]),
    "tdx_pair_member": (C.c_int, [_ptr, _ptr, _ptr] + [C.c_int] * 4 + [_ptr, _ptr, C.c_size_t, _ptr]),
    "tdx_pair_poly_rowsum": (C.c_int, [_ptr, _ptr] + [C.c_int] * 3 + [C.c_float, C.c_float, C.c_int, C.c_int,
                                                                    _ptr, _ptr, C.c_size_t, _ptr]),
}

EXPORTS = tuple(_SIGS)
STEP_EPS, STEP_X0, STEP_MS = 0, 1, 2   # TDX_STEP_*: the forms of tdx_p_sample_update / tdx_unet_eval_step_update


def _bind():
    missing = []
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing:
        raise TdxError(f"libtdx.so lacks symbols declared in include/tdx.h: {missing}")


_bind()


def _apply_env_tuning():
    """TDX_TUNE="conv_tile=3,splitk=0": process-wide tuning knobs (tdx_tune_set)."""
    spec = os.environ.get("TDX_TUNE", "")
    for item in filter(None, (x.strip() for x in spec.split(","))):
        key, _, val = item.partition("=")
        if lib.tdx_tune_set(key.encode(), int(val)) != 0:
            raise TdxError(f"unknown TDX_TUNE knob {key!r}")


_apply_env_tuning()


def check(code: int, what: str = "tdx"):
    if code != 0:
        msg = lib.tdx_error_string(code)
        raise TdxError(f"{what} failed: {msg.decode() if msg else code} ({code})")


def tune_get(key: str) -> int:
    value = C.c_int()
    if lib.tdx_tune_get(key.encode(), C.byref(value)) != 0:
        raise TdxError(f"unknown tuning knob {key!r}")
    return value.value


@contextlib.contextmanager
def tuned(**knobs):
    """Run the body under these tuning knobs, then put back the values they held, last set first.
    An unknown key raises TdxError before any knob is set."""
    old = [(key, tune_get(key)) for key in knobs]
    try:
        for key, value in knobs.items():
            check(lib.tdx_tune_set(key.encode(), int(value)), f"tdx_tune_set({key})")
        yield
    finally:
        for key, value in reversed(old):
            check(lib.tdx_tune_set(key.encode(), value), f"tdx_tune_set({key})")


def ptr(t):
    """Device (or host) address of a torch tensor, None -> NULL."""
    return None if t is None else t.data_ptr()


def stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream
