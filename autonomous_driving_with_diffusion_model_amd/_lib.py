"""ctypes binding of libadx.so (C ABI declared in include/adx.h).

There is NO fallback: if the shared library is missing every op raises, so a GPU box can
never silently run an eager/PyTorch path instead of the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADX_LIB") or os.path.join(_HERE, "libadx.so")   # ADX_LIB: A/B builds in one run

c_f32p = C.POINTER(C.c_float)
i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class TConvDesc(C.Structure):
    _fields_ = [("kind", i32), ("taps", i32), ("stride", i32), ("pad", i32), ("c0", i32), ("c1", i32),
                ("cout", i32), ("lin", i32), ("lout", i32), ("groups", i32), ("eps", f32), ("w_layout", i32),
                ("w_flip", i32), ("exact", i32), ("lin_valid", i32), ("lout_valid", i32)]


class TConvIO(C.Structure):
    _fields_ = [("x0", vp), ("x0_sb", i64), ("x0_sc", i64), ("x0_sl", i64),
                ("x1", vp), ("x1_sb", i64), ("x1_sc", i64), ("x1_sl", i64),
                ("packed_w", vp), ("bias", vp), ("gamma", vp), ("beta", vp),
                ("tbias", vp), ("tbias_stride", i64),
                ("res", vp), ("res_sb", i64), ("res_sc", i64), ("res_sl", i64),
                ("y", vp), ("y_sb", i64), ("y_sc", i64), ("y_sl", i64), ("batch", i32), ("pre", vp), ("stats", vp),
                ("scratch", vp), ("scratch_floats", i64), ("tickets", vp)]


class EmbedWeights(C.Structure):
    _fields_ = [(n, vp) for n in ("freqs", "w1", "b1", "w3", "b3", "cw0", "cb0", "cw2", "cb2")]


class UnetConfig(C.Structure):
    _fields_ = [("horizon", i32), ("transition_dim", i32), ("dim", i32), ("n_mults", i32),
                ("dim_mults", i32 * 8), ("guidance", i32)]


class UnetIO(C.Structure):
    _fields_ = [("x", vp), ("img_feature", vp), ("feat_rows", i32), ("t", vp), ("t_rows", i32), ("cond", vp),
                ("rows", i32), ("out", vp), ("time_embed", vp), ("x_rows", i32), ("time_bias", vp)]


UNET_ATTENTION = 1          # adx_unet_create_ex flag (ADX_UNET_ATTENTION)


class Conv2dDesc(C.Structure):
    _fields_ = [("cin", i32), ("cout", i32), ("k", i32), ("stride", i32), ("pad", i32)]


class StepCoef(C.Structure):
    _fields_ = [("prediction_type", i32), ("clip", i32), ("clip_range", f32), ("sqrt_alpha_t", f32),
                ("sqrt_beta_t", f32), ("c_x0", f32), ("c_dir", f32), ("c_x", f32), ("c_noise", f32),
                ("add_noise", i32), ("use_clipped_model_output", i32), ("inpaint", i32), ("c_const", f32),
                ("c_known", f32), ("c_known_noise", f32), ("known_noise", i32), ("cfg_combine", i32),
                ("free_scale", f32), ("zero_first", i32)]


class DpmCoef(C.Structure):
    _fields_ = [("prediction_type", i32), ("clip", i32), ("clip_range", f32), ("alpha_s", f32), ("sigma_s", f32),
                ("r", f32), ("k", f32), ("second_order", i32), ("inv_r0", f32), ("half_k", f32), ("cfg_combine", i32),
                ("free_scale", f32), ("zero_first", i32)]


class PinDesc(C.Structure):
    """adx_pin ("pinned waypoints v1", include/adx.h)."""
    _fields_ = [("known", vp), ("mask", vp), ("known_rows", i32), ("c_known", f32), ("c_known_noise", f32), ("known_noise", i32)]


class GuideDesc(C.Structure):
    """adx_guide ("cost guidance v1", include/adx.h)."""
    _fields_ = [("discs", vp), ("planes", vp), ("scene_rows", i32), ("n_discs", i32), ("n_planes", i32), ("iters", i32),
                ("lambda_", f32), ("cap", f32)]


class FieldDesc(C.Structure):
    """adx_guide_field ("cost guidance v2", include/adx.h)."""
    _fields_ = [("cells", vp), ("scene_rows", i32), ("gx", i32), ("gy", i32), ("x_min", f32), ("y_min", f32), ("inv_dx", f32),
                ("inv_dy", f32), ("weight", f32)]


class MotionDesc(C.Structure):
    """adx_guide_motion ("cost guidance v3", include/adx.h)."""
    _fields_ = [("limits", vp), ("scene_rows", i32), ("w_speed", f32), ("w_accel", f32)]


class RouteDesc(C.Structure):
    """adx_guide_route ("cost guidance v4", include/adx.h)."""
    _fields_ = [("points", vp), ("half_width", vp), ("scene_rows", i32), ("n_points", i32), ("weight", f32)]


class CapsuleDesc(C.Structure):
    """adx_guide_capsules ("cost guidance v5", include/adx.h)."""
    _fields_ = [("capsules", vp), ("scene_rows", i32), ("n_capsules", i32), ("weight", f32)]


class SelectCfg(C.Structure):
    _fields_ = [("scenes", i32), ("candidates", i32), ("horizon", i32), ("dim", i32), ("w_goal", f32), ("w_smooth", f32),
                ("w_consensus", f32)]


class SelectGuideCfg(C.Structure):
    """adx_select_guide_cfg ("selection cost v2", include/adx.h)."""
    _fields_ = [("scenes", i32), ("candidates", i32), ("horizon", i32), ("dim", i32), ("w_goal", f32), ("w_smooth", f32),
                ("w_consensus", f32), ("w_guide", f32), ("hard", i32)]


class ModesCfg(C.Structure):
    """adx_modes_cfg ("trajectory modes v1", include/adx.h)."""
    _fields_ = [("scenes", i32), ("candidates", i32), ("horizon", i32), ("dim", i32), ("max_modes", i32), ("h0", i32),
                ("radius", f32)]


class CommitCfg(C.Structure):
    """adx_commit_cfg ("manoeuvre commitment v1", include/adx.h)."""
    _fields_ = [("scenes", i32), ("candidates", i32), ("horizon", i32), ("dim", i32), ("h0", i32), ("shift", i32), ("max_hold", i32),
                ("radius", f32), ("margin", f32), ("ratio", f32)]


class NavCfg(C.Structure):
    """adx_nav_cfg ("route planner v1", include/adx.h)."""
    _fields_ = [("scenes", i32), ("max_points", i32), ("window", i32), ("first", i32), ("min_distance", C.c_double),
                ("max_distance", C.c_double), ("xy_scale", C.c_double)]


class VehicleCfg(C.Structure):
    """adx_vehicle_cfg ("vehicle v1", include/adx.h)."""
    _fields_ = [("scenes", i32), ("substeps", i32), ("steer_sign", i32), ("reserved", i32)] + \
               [(n, C.c_double) for n in ("dt", "wheelbase", "accel_max", "brake_max", "drag", "roll", "v_max", "steer_max")]


class DriveCfg(C.Structure):
    """adx_drive_cfg ("drive metrics v1", include/adx.h)."""
    _fields_ = [(n, i32) for n in ("scenes", "max_points", "window", "n_world_discs", "n_boxes", "n_discs", "stop_on_collision",
                                   "max_ticks")] + \
               [("dt", C.c_double), ("r_ego", C.c_double), ("offset", C.c_double * 4)] + \
               [(n, C.c_double) for n in ("offroad_min", "offroad_max", "max_route_percentage", "speed_threshold", "max_time",
                                          "completion_tol")]


class SignalsCfg(C.Structure):
    """adx_signals_cfg ("signals v1", include/adx.h)."""
    _fields_ = [(n, i32) for n in ("scenes", "n_signals", "n_planes", "stop_on_yellow")] + \
               [(n, C.c_double) for n in ("dt", "xy_scale", "margin", "probe", "min_cos", "speed_threshold")]


class TrafficCfg(C.Structure):
    """adx_traffic_cfg ("traffic v1", include/adx.h)."""
    _fields_ = [(n, i32) for n in ("scenes", "n_agents", "n_paths", "n_points", "n_stops", "n_signals")] + \
               [(n, C.c_double) for n in ("dt", "lane_half_width", "ego_length", "jam", "gap_min", "brake_max")]


class CameraCfg(C.Structure):
    """adx_camera_cfg ("camera v1", include/adx.h)."""
    _fields_ = [(n, i32) for n in ("scenes", "width", "height", "n_boxes", "n_discs", "n_signals", "n_paths", "n_points")] + \
               [(n, C.c_double) for n in ("fov", "mount_back", "cam_height", "near", "far", "half_width", "mark", "line_half",
                                          "box_height", "disc_height", "lamp_radius", "lamp_height", "lamp_setback", "pole_radius")] + \
               [("mean", f32 * 3), ("stdv", f32 * 3), ("palette", C.c_uint8 * 60), ("shade", C.c_uint8 * 5), ("reserved", C.c_uint8 * 7)]


class ExpertCfg(C.Structure):
    """adx_expert_cfg ("expert v1", include/adx.h)."""
    _fields_ = [(n, i32) for n in ("scenes", "window", "n_boxes", "n_discs", "n_planes", "horizon", "dim", "reserved")] + \
               [(n, C.c_double) for n in ("xy_scale", "waypoint_dt", "desired_v", "accel", "brake", "brake_max", "headway", "jam", "gap_min",
                                          "corridor_half", "lat_accel", "look_time", "ego_front", "end_margin", "look_min")]


class ControlCfg(C.Structure):
    _fields_ = ([(n, i32) for n in ("scenes", "horizon", "dim", "waypoints", "n_turn", "n_speed", "source", "post")] +
                [(n, f32) for n in ("sign_x", "xy_scale", "target_scale", "turn_kp", "turn_ki", "turn_kd", "speed_kp", "speed_ki",
                                    "speed_kd", "aim_dist", "angle_thresh", "dist_thresh", "brake_speed", "brake_ratio", "clip_delta",
                                    "max_throttle")])


class MetricsCfg(C.Structure):
    """adx_metrics_cfg ("open-loop metrics v1", include/adx.h)."""
    _fields_ = [("scenes", i32), ("candidates", i32), ("horizon", i32), ("dim", i32), ("h0", i32), ("miss_radius", f32),
                ("xy_scale", f32)]


_SIGS = {
    "adx_version": (i32, []),
    "adx_last_error": (C.c_char_p, []),
    "adx_source_hash": (C.c_char_p, []),
    "adx_tconv_packed_bytes": (C.c_size_t, [C.POINTER(TConvDesc)]),
    "adx_tconv_pack": (i32, [C.POINTER(TConvDesc), vp, vp, vp]),
    "adx_tconv_forward": (i32, [C.POINTER(TConvDesc), C.POINTER(TConvIO), vp]),
    "adx_embed_forward": (i32, [C.POINTER(EmbedWeights), i32, vp, i32, vp, vp, i32, i32, vp, vp, vp]),
    "adx_unet_create": (i32, [C.POINTER(UnetConfig), C.POINTER(vp)]),
    "adx_unet_create_ex": (i32, [C.POINTER(UnetConfig), i32, C.POINTER(vp)]),
    "adx_unet_destroy": (None, [vp]),
    "adx_unet_num_params": (i32, [vp]),
    "adx_unet_packed_bytes": (C.c_size_t, [vp]),
    "adx_unet_pack": (i32, [vp, C.POINTER(vp), i32, vp, vp, vp]),
    "adx_unet_workspace_bytes": (C.c_size_t, [vp, i32]),
    "adx_unet_forward": (i32, [vp, vp, vp, C.POINTER(UnetIO), vp]),
    "adx_unet_time_bias_width": (i32, [vp]),
    "adx_unet_time_conditioning_workspace_bytes": (C.c_size_t, [vp, i32]),
    "adx_unet_time_conditioning": (i32, [vp, vp, vp, C.POINTER(UnetIO), vp, vp, vp]),
    "adx_unet_pipe_describe": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i64)]),
    "adx_unet_plan_describe": (i32, [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), i32]),
    "adx_tconv_plan_describe": (i32, [C.POINTER(TConvDesc), i32, i64, i32, C.POINTER(i32), C.POINTER(i32), i32]),
    "adx_unet_tape_create": (i32, [C.POINTER(vp)]),
    "adx_unet_tape_destroy": (None, [vp]),
    "adx_unet_train_workspace_bytes": (C.c_size_t, [vp, i32]),
    "adx_unet_forward_train": (i32, [vp, vp, vp, C.c_size_t, C.POINTER(UnetIO), vp, vp]),
    "adx_unet_backward": (i32, [vp, vp, vp, C.c_size_t, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), i32, vp]),
    "adx_gn_mish_backward": (i32, [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp]),
    "adx_tconv_wgrad": (i32, [C.POINTER(TConvDesc), C.POINTER(TConvIO), vp, vp, vp]),
    "adx_bias_grad": (i32, [vp, vp, i32, i32, i32, vp]),
    "adx_gn_mish_backward_ex": (i32, [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp]),
    "adx_bias_grad_ex": (i32, [vp, i64, i64, i64, vp, i32, i32, i32, i32, vp]),
    "adx_tconv_wgrad_plan_describe": (i32, [C.POINTER(TConvDesc), i32, C.POINTER(i32)]),
    "adx_chan_layernorm_forward": (i32, [vp, i64, i64, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "adx_chan_layernorm_backward": (i32, [vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "adx_linattn_forward": (i32, [vp, vp, i32, i32, i32, vp]),
    "adx_linattn_backward": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "adx_resnet_create": (i32, [i32, C.POINTER(vp)]),
    "adx_resnet_destroy": (None, [vp]),
    "adx_resnet_num_tensors": (i32, [vp]),
    "adx_resnet_packed_bytes": (C.c_size_t, [vp]),
    "adx_resnet_pack": (i32, [vp, C.POINTER(vp), i32, vp, vp]),
    "adx_resnet_workspace_bytes": (C.c_size_t, [vp, i32, i32, i32]),
    "adx_resnet_plan_describe": (i32, [vp, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), i32]),
    "adx_resnet_forward": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "adx_resnet_forward_u8": (i32, [vp, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), i32, i32, i32, vp, vp]),
    "adx_unet_status_words": (i32, [vp]),
    "adx_unet_set_status": (i32, [vp, vp]),
    "adx_unet_status_name": (C.c_char_p, [vp, i32]),
    "adx_resnet_status_words": (i32, [vp]),
    "adx_resnet_set_status": (i32, [vp, vp]),
    "adx_resnet_status_name": (C.c_char_p, [vp, i32]),
    "adx_resnet_tape_create": (i32, [C.POINTER(vp)]),
    "adx_resnet_tape_destroy": (None, [vp]),
    "adx_resnet_train_workspace_bytes": (C.c_size_t, [vp, i32, i32, i32]),
    "adx_resnet_forward_train": (i32, [vp, C.POINTER(vp), i32, vp, vp, C.c_size_t, vp, i32, i32, i32, vp, vp, i32, vp]),
    "adx_resnet_backward": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, vp, C.c_size_t, vp, vp, vp]),
    "adx_resnet_backward_groups": (i32, [vp]),
    "adx_resnet_tensor_group": (i32, [vp, i32]),
    "adx_resnet_backward_events": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, vp, C.c_size_t, vp, vp, C.POINTER(vp), i32, vp]),
    "adx_resnet_tape_describe": (i32, [vp, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]),
    "adx_resnet_bn_layers": (i32, [vp]),
    "adx_resnet_bn_tensor": (i32, [vp, i32]),
    "adx_resnet_forward_train_ex": (i32, [vp, C.POINTER(vp), i32, vp, vp, C.c_size_t, vp, i32, i32, i32, vp, vp, i32, C.c_uint64,
                                          vp]),
    "adx_resnet_backward_ex": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, vp, C.c_size_t, vp, vp, C.c_uint64, C.POINTER(vp), i32,
                                     vp]),
    "adx_conv2d_packed_bytes": (C.c_size_t, [C.POINTER(Conv2dDesc)]),
    "adx_conv2d_pack": (i32, [C.POINTER(Conv2dDesc), vp, vp, vp]),
    "adx_conv2d_forward": (i32, [C.POINTER(Conv2dDesc), vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "adx_conv2d_cells_supported": (i32, [C.POINTER(Conv2dDesc), i32, i32, i32]),
    "adx_conv2d_forward_cells": (i32, [C.POINTER(Conv2dDesc), vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "adx_conv2d_stem_pool": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "adx_conv2d_wgrad_scratch_bytes": (C.c_size_t, []),
    "adx_conv2d_wgrad": (i32, [C.POINTER(Conv2dDesc), vp, vp, vp, i32, i32, i32, vp, vp]),
    "adx_conv2d_wgrad_ex": (i32, [C.POINTER(Conv2dDesc), vp, vp, vp, i32, i32, i32, vp, i32, vp]),
    "adx_conv2d_wgrad_cells": (i32, [C.POINTER(Conv2dDesc), vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "adx_trajpred_create": (i32, [i32, C.POINTER(vp)]),
    "adx_trajpred_destroy": (None, [vp]),
    "adx_trajpred_num_params": (i32, [vp]),
    "adx_trajpred_packed_bytes": (C.c_size_t, [vp]),
    "adx_trajpred_scratch_bytes": (C.c_size_t, [vp, i32, i32]),
    "adx_trajpred_set_scratch": (i32, [vp, vp, C.c_size_t]),
    "adx_trajpred_pack": (i32, [vp, C.POINTER(vp), i32, vp, vp, vp]),
    "adx_trajpred_forward": (i32, [vp, vp, vp, i64, i64, vp, vp, i32, i32, vp]),
    "adx_trajpred_backward": (i32, [vp, vp, vp, i64, i64, vp, vp, vp, i32, i32, vp]),
    "adx_trajpred_backward_params": (i32, [vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_uint64, vp]),
    "adx_trajpred_forward_train": (i32, [vp, vp, vp, i64, i64, vp, vp, i32, i32, C.c_float, C.c_uint64, vp]),
    "adx_trajpred_param_offsets": (i32, [vp, C.POINTER(i64), i32]),
    "adx_guided_output": (i32, [vp, vp, vp, vp, vp, f32, f32, vp, vp, i32, i32, vp]),
    "adx_optim_chunk": (i32, []),
    "adx_adamw_ema_step": (i32, [vp, vp, vp, i32, f32, f32, f32, f32, f32, i32, f32, i32, i32, vp]),
    "adx_adamw_ema_step_scaled": (i32, [vp, vp, vp, i32, f32, f32, f32, f32, f32, i32, f32, i32, i32, f32, vp]),
    "adx_image_normalize": (i32, [vp, vp, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), vp]),
    "adx_probe_mfma_fp16": (i32, [vp, vp, i32, i32, C.POINTER(C.c_double), vp]),
    "adx_probe_mfma_fp16_16x16x32": (i32, [vp, vp, i32, i32, C.POINTER(C.c_double), vp]),
    "adx_image_augment": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp]),
    "adx_ddim_step": (i32, [C.POINTER(StepCoef), vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "adx_ddpm_step": (i32, [C.POINTER(StepCoef), vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "adx_ddim_step_rng": (i32, [C.POINTER(StepCoef), vp, vp, vp, i32, i64, vp, vp, vp, vp, i32, i32, i32, vp]),
    "adx_ddpm_step_rng": (i32, [C.POINTER(StepCoef), vp, vp, vp, i32, i64, vp, vp, vp, vp, i32, i32, i32, vp]),
    "adx_dpm_step": (i32, [C.POINTER(DpmCoef), vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "adx_traj_select": (i32, [C.POINTER(SelectCfg), vp, vp, vp, vp, vp, vp]),
    "adx_control_state_bytes": (C.c_size_t, [i32, i32, i32]),
    "adx_control_step": (i32, [C.POINTER(ControlCfg), vp, vp, vp, vp, vp, vp]),
    "adx_control_reset": (i32, [vp, i32, i32, i32, vp, vp]),
    "adx_traj_metrics": (i32, [C.POINTER(MetricsCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_metrics_state_bytes": (C.c_size_t, []),
    "adx_metrics_reset": (i32, [vp, vp]),
    "adx_metrics_accumulate": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    "adx_noise_normal": (i32, [vp, i32, i64, vp, i64, vp]),
    "adx_noise_words": (i32, [vp, i32, i64, vp, i64, vp]),
    "adx_noise_advance": (i32, [vp, vp]),
    "adx_warm_init": (i32, [vp, i32, vp, vp, i32, i32, i32, i32, f32, f32, vp, i64, i32, vp]),
    "adx_add_noise": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, vp]),
}

# resolved on first use (lazy()), not at load: ADX_LIB may point at a library built before these entry points existed (A/B runs)
_LAZY_SIGS = {
    "adx_resnet_plan_grids": (i32, [vp, i32, i32, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), i32]),
    "adx_conv2d_hs3x3q_walk": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
    "adx_conv2d_hs3x3_pair_walk": (i32, [i32, C.POINTER(i32), C.POINTER(i32), i32]),
    "adx_conv2d_hs3x3_plan_query": (i32, [C.POINTER(Conv2dDesc), i32, i32, i32, i32, i32, C.POINTER(i32)]),
    "adx_conv2d_pack_ds": (i32, [i32, i32, vp, vp, vp]),
    "adx_conv2d_block_s2_cells": (i32, [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "adx_ddim_step_pin": (i32, [C.POINTER(StepCoef), vp, vp, vp, vp, i32, i64, C.POINTER(PinDesc), vp, vp, i32, i32, i32, vp]),
    "adx_ddpm_step_pin": (i32, [C.POINTER(StepCoef), vp, vp, vp, vp, i32, i64, C.POINTER(PinDesc), vp, vp, i32, i32, i32, vp]),
    "adx_dpm_step_pin": (i32, [C.POINTER(DpmCoef), vp, vp, vp, vp, i32, i64, C.POINTER(PinDesc), vp, vp, i32, i32, i32, vp]),
    "adx_pin_apply": (i32, [vp, C.POINTER(PinDesc), vp, i64, i32, i32, i32, vp]),
    "adx_cost_field_from_occupancy": (i32, [vp, vp, i32, i32, i32, f32, f32, f32, i32, i32, vp]),
    "adx_capsules_from_boxes": (i32, [vp, vp, i32, i32, f32, vp]),
    "adx_stop_short": (i32, [vp, C.POINTER(GuideDesc), C.POINTER(FieldDesc), C.POINTER(RouteDesc), C.POINTER(CapsuleDesc), vp, i32, vp, vp,
                             vp, vp, vp, i32, i32, i32, vp]),
    "adx_traj_modes": (i32, [C.POINTER(ModesCfg), vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_commit_state_bytes": (C.c_size_t, [i32, i32]),
    "adx_commit_reset": (i32, [vp, i32, i32, vp, vp]),
    "adx_traj_commit": (i32, [C.POINTER(CommitCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_nav_state_bytes": (C.c_size_t, [i32]),
    "adx_nav_reset": (i32, [vp, i32, vp, vp]),
    "adx_nav_step": (i32, [C.POINTER(NavCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_vehicle_state_bytes": (C.c_size_t, [i32]),
    "adx_vehicle_reset": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "adx_vehicle_step": (i32, [C.POINTER(VehicleCfg), vp, vp, vp, vp, vp, vp, vp]),
    "adx_drive_state_bytes": (C.c_size_t, [i32]),
    "adx_drive_reset": (i32, [vp, i32, vp, vp, vp]),
    "adx_drive_step": (i32, [C.POINTER(DriveCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_signals_state_bytes": (C.c_size_t, [i32]),
    "adx_signals_reset": (i32, [vp, i32, vp, vp, i32, vp]),
    "adx_signals_step": (i32, [C.POINTER(SignalsCfg), vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_traffic_state_bytes": (C.c_size_t, [i32, i32]),
    "adx_traffic_reset": (i32, [C.POINTER(TrafficCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_traffic_step": (i32, [C.POINTER(TrafficCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_camera_prims_bytes": (C.c_size_t, [C.POINTER(CameraCfg)]),
    "adx_camera_default_palette": (None, [vp, vp]),
    "adx_camera_render": (i32, [C.POINTER(CameraCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_expert_plan": (i32, [C.POINTER(ExpertCfg), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "adx_world_to_ego": (i32, [i32, vp, vp, vp, i32, i32, C.c_double, C.c_double, vp]),
    "adx_ego_to_world": (i32, [vp, vp, vp, i32, i32, i32, i32, C.c_double, vp]),
}

# the guided exports: five families (the three steps, the cost, the guided selection) times five suffixes, each suffix taking the
# record of the one before it and one more -- the order of guide.py's RECORDS, which names the suffixes
_records = ()
for _suffix, _desc in (("guide", GuideDesc), ("field", FieldDesc), ("motion", MotionDesc), ("route", RouteDesc), ("capsule", CapsuleDesc)):
    _records += (C.POINTER(_desc),)
    for _step, _coef in (("ddim", StepCoef), ("ddpm", StepCoef), ("dpm", DpmCoef)):
        _LAZY_SIGS[f"adx_{_step}_step_{_suffix}"] = (i32, [C.POINTER(_coef), vp, vp, vp, vp, i32, i64, C.POINTER(PinDesc), *_records,
                                                          vp, vp, i32, i32, i32, vp])
    _tail = "" if _suffix == "guide" else "_" + _suffix
    _LAZY_SIGS["adx_guide_cost" + _tail] = (i32, [vp, *_records, vp, vp, i32, i32, i32, vp])
    _LAZY_SIGS["adx_traj_select_guide" + _tail] = (i32, [C.POINTER(SelectGuideCfg), vp, vp, *_records, vp, vp, vp, vp, vp, vp])

EXPORTED_SYMBOLS = tuple(_SIGS) + tuple(_LAZY_SIGS)

_lib: Optional[C.CDLL] = None


class AdxError(RuntimeError):
    pass


class AdxRangeError(AdxError):
    """A forward under `range_guard = "raise"` split a value outside fp16's range (|x| >= 65504 or NaN) into the
    hi / lo operands of the split-fp16 kernels; `groups` names the layer groups whose status words are set."""

    def __init__(self, groups):
        self.groups = list(groups)
        super().__init__(f"values outside the fp16 range of the split kernels (|x| >= 65504 or NaN) in {', '.join(self.groups)}; "
                         "ADX_CHECK_RANGE=1 names the first tensor, ADX_CONV_EXACT=1 runs the perception pass on the exact-fp32 kernels")


def lib() -> C.CDLL:
    """Load libadx.so once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AdxError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
                f"g.build()'` (or autonomous_driving_with_diffusion_model_amd/csrc/build.sh). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(handle, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def lazy(name: str):
    """An entry point of _LAZY_SIGS; raises AdxError when the loaded library does not export it."""
    handle = lib()
    res, args = _LAZY_SIGS[name]
    try:
        fn = getattr(handle, name)
    except AttributeError:
        raise AdxError(f"{LIB_PATH} does not export {name} (a library built from older sources?)") from None
    fn.restype = res
    fn.argtypes = args
    return fn


class NativeTape:
    """Owner of one native training tape (adx_*_tape_create / _destroy).  The handle is destroyed exactly once: by
    `release()` after the backward pass, or by the finalizer when the autograd node that holds it is dropped without a
    backward (a train-mode forward under no_grad, a loss that is never back-propagated)."""

    def __init__(self, create, destroy, what: str):
        import weakref
        h = vp()
        check(create(C.byref(h)), what)
        self.handle = h
        self._fin = weakref.finalize(self, destroy, h)

    @property
    def alive(self) -> bool:
        return self._fin.alive

    def release(self) -> None:
        self._fin()          # idempotent


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().adx_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}" if what else msg)
        raise AdxError(f"{what} failed (status {rc}): {msg}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu_f32(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not t.is_cuda:
        raise AdxError(f"{name} lives on {t.device}; the adx kernels only run on an MI355X (no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def write_stamp(t: torch.Tensor) -> int:
    """A number that moves when `t` is written in place: autograd's version counter.  Inference tensors -- everything
    created under `torch.inference_mode()`, which is how the reference's `train.evaluate` runs (train.py:53) -- carry no
    counter (`._version` raises on them); they answer 0, so a memo keyed on (identity, stamp) then rests on identity alone:
    an in-place write to an inference tensor between two forwards is NOT seen.  The image-feature memo therefore skips
    inference tensors unless the caller opts in (`model.cache_perception = "identity"`, modeling/temporal.py:image_feature);
    the weight-image memos key on parameters, which optimizers and loaders replace or write outside inference mode."""
    return 0 if t.is_inference() else t._version


def grad_buffer(p: torch.Tensor) -> torch.Tensor:
    """Where a backward node writes d(loss)/d(p).  Under `parallel.GradientAverager` every parameter owns a view into a
    flat communication bucket (`p._adx_grad_view`); when the parameter has no gradient yet, a fresh alias of that view is
    handed out -- autograd adopts a gradient tensor nobody else holds as `.grad` without copying, so the gradient is born
    inside the bucket the collective runs on.  With a gradient already present (accumulation over several backwards)
    autograd ADDS what the node returns to `.grad`, which may be this very storage: then, and without an averager, the
    node gets a buffer of its own.

    The view is LENT at most once per backward (`p._adx_grad_leased`): a parameter that feeds two nodes of one graph (the
    model called twice before one `loss.backward()`, shared weights) reaches both nodes with `.grad is None` -- AccumulateGrad
    has not run yet -- and two nodes writing the same storage would leave autograd summing two aliases of the second
    gradient.  The averager clears the lease when the gradient has been accumulated (its post-accumulate hook) or reduced."""
    v = getattr(p, "_adx_grad_view", None)
    if (v is not None and p.grad is None and not getattr(p, "_adx_grad_leased", False)
            and v.device == p.device and v.shape == p.shape):
        p._adx_grad_leased = True
        return v.detach()
    return torch.empty_like(p)


def ptr_array(tensors: Sequence[torch.Tensor]):
    arr = (vp * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr
