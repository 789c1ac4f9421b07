"""ctypes binding of libmarl_hip.so (the C ABI declared in include/marl_hip.h).

The library is the product: there is no CPU or PyTorch fallback.  If it has not
been built (``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C marlclassification_amd/csrc``) loading fails loudly.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

MARL_MAX_CNN_LAYERS = 5
MARL_MAX_ACTIONS = 16
MARL_ABI_VERSION = 5
MARL_COUNTERS_BYTES = 32
MARL_GRAD_CLIP_SCRATCH_BYTES = 1024 * 8

_HERE = os.path.dirname(os.path.abspath(__file__))
# MARL_LIB_PATH: another build of the SAME library (tools/build_variant.sh: timing / ablation builds, the previous
# round's library for same-box A/Bs) - never a different implementation: load() checks the ABI and every export
LIB_PATH = os.environ.get("MARL_LIB_PATH") or os.path.join(_HERE, "csrc", "libmarl_hip.so")


class MarlConfig(C.Structure):
    """Mirror of ``marl_config`` (include/marl_hip.h)."""

    _fields_ = [
        ("nb_agents", C.c_int32),
        ("batch", C.c_int32),
        ("nb_steps", C.c_int32),
        ("img_c", C.c_int32),
        ("img_h", C.c_int32),
        ("img_w", C.c_int32),
        ("window", C.c_int32),
        ("cnn_layers", C.c_int32),
        ("cnn_ch", C.c_int32 * (MARL_MAX_CNN_LAYERS + 1)),
        ("cnn_groups", C.c_int32 * MARL_MAX_CNN_LAYERS),
        ("n_b", C.c_int32),
        ("n_a", C.c_int32),
        ("n_m", C.c_int32),
        ("n_m_o", C.c_int32),
        ("n_d", C.c_int32),
        ("nb_action", C.c_int32),
        ("nb_class", C.c_int32),
        ("nlb", C.c_int32),
        ("nla", C.c_int32),
        ("actions", (C.c_int32 * 2) * MARL_MAX_ACTIONS),
        ("img_u8", C.c_int32),
    ]


# parameter table indices (enum in include/marl_hip.h)
_NAMES = (
    "POS_W POS_B POS_LNW POS_LNB "
    "ENC_W0 ENC_B0 ENC_LN0W ENC_LN0B ENC_W1 ENC_B1 ENC_LN1W ENC_LN1B "
    "DEC_W0 DEC_B0 DEC_LN0W DEC_LN0B DEC_W1 DEC_B1 DEC_LN1W DEC_LN1B "
    "LB_WIH LB_WHH LB_BIH LB_BHH LA_WIH LA_WHH LA_BIH LA_BHH "
    "POL_W0 POL_B0 POL_LNW POL_LNB POL_W1 POL_B1 "
    "CRI_W0 CRI_B0 CRI_LNW CRI_LNB CRI_W1 CRI_B1 "
    "PRE_W0 PRE_B0 PRE_LNW PRE_LNB PRE_W1 PRE_B1"
).split()
P = {name: 20 + i for i, name in enumerate(_NAMES)}
MARL_NPARAMS = 20 + len(_NAMES)

# every symbol include/marl_hip.h declares
EXPORTS = (
    "marl_abi_version marl_last_error marl_param_numel marl_workspace_sizes marl_pack_weights "
    "marl_patch_gather marl_transition marl_episode_forward marl_episode_backward "
    "marl_a2c_loss_fwd_bwd marl_adam_step marl_step_forward marl_gemm_nt marl_gemm_tn "
    "marl_gemm_tn_scratch marl_gemm_nt_weights marl_gemm_weight_image_bytes marl_ln_silu_fwd marl_debug_buffer "
    "marl_profile_begin marl_profile_end marl_normalize_positions "
    "marl_cnn_wgrad marl_cnn_wgrad_scratch marl_tune marl_tune_get marl_draw_episode "
    "marl_counters_set marl_counters_tick marl_graph_begin marl_graph_end marl_graph_launch "
    "marl_graph_destroy marl_image_bytes marl_image_build marl_gemm_nt_images marl_gemm_nt_images_batch "
    "marl_lstm_images marl_gemm_tn_images marl_gemm_tn_images_scratch marl_plan_query "
    "marl_gemm_tn_images_cell marl_gemm_tn_images_cell_scratch marl_backward_heads_event "
    "marl_step_forward_train marl_step_backward marl_episode_backward_img "
    "marl_episode_forward_probs marl_episode_backward_probs marl_a2c_loss_entropy_fwd_bwd "
    "marl_advantages marl_ppo_loss_fwd_bwd marl_grad_clip marl_comm_matrix "
    "marl_comm_grad marl_comm_grad_scratch_bytes marl_comm_range"
).split()

# kernel-level test hooks that include/marl_hip_rowops.h declares (outside the versioned ABI above)
ROWOP_HOOKS = ("marl_ln_silu_bwd", "marl_gn_silu_bwd", "marl_gn_silu_fwd", "marl_ln_silu_dot_fwd", "marl_pos_embed_fwd",
               "marl_lstm_cell_bwd", "marl_policy_dlogits", "marl_rowdot", "marl_agg_msg")
# ... and those of the conv kernels that include/marl_hip_cnnops.h declares
CNNOP_HOOKS = ("marl_cnn_dgrad", "marl_cnn_dgrad_scratch", "marl_cnn_bwd_plan", "marl_cnn_fwd", "marl_cnn_fwd_plan")
# ... and the exploration controls that include/marl_hip_explore.h declares (beside the versioned ABI, not in it)
EXPLORE_ENTRIES = ("marl_policy_explore",)
# ... and the augmenting batch gather that include/marl_hip_augment.h declares (likewise; augment.py binds it)
AUGMENT_ENTRIES = ("marl_batch_augment", "marl_batch_augment_plan")
# ... and the options of the vote error and the rewards that include/marl_hip_classloss.h declares (likewise)
CLASSLOSS_ENTRIES = ("marl_class_loss",)
# ... and the target distributions of the same two kernels that include/marl_hip_softtargets.h declares (likewise)
SOFTTARGET_ENTRIES = ("marl_soft_targets",)
# ... and the mixing batch gather that include/marl_hip_mix.h declares (likewise; mix.py binds it)
MIX_ENTRIES = ("marl_batch_mix", "marl_batch_mix_plan")
# ... and the flat optimiser step that include/marl_hip_optim.h declares (likewise; optim.py holds its structures)
OPTIM_ENTRIES = ("marl_optim_step",)
# ... and the kernel-level hooks of the row-panel kernels that include/marl_hip_panelops.h declares (tests only)
PANELOP_HOOKS = ("marl_panel_fwd", "marl_panel_bwd", "marl_panel_scratch_bytes", "marl_panel_plan")
# ... and the host-only witness of the matrix-product launchers that include/marl_hip_gemmops.h declares (tests only)
GEMMOP_HOOKS = ("marl_gemm_plan",)
# ... and the episode report that include/marl_hip_report.h declares (beside the versioned ABI; report.py binds it)
REPORT_ENTRIES = ("marl_report_layout", "marl_report_scratch_bytes", "marl_episode_report")
# ... and the resampling batch gather that include/marl_hip_warp.h declares (likewise; warp.py binds it)
WARP_ENTRIES = ("marl_batch_warp", "marl_batch_warp_plan")
# ... and the per-image input normalisation that include/marl_hip_normalize.h declares (likewise; transforms.py binds it)
NORMALIZE_ENTRIES = ("marl_batch_stats", "marl_batch_stats_scratch_bytes", "marl_batch_normalize",
                     "marl_batch_normalize_plan")
# ... and the colour jitter that include/marl_hip_color.h declares (likewise; color.py binds it)
COLOR_ENTRIES = ("marl_batch_color", "marl_batch_color_plan")
_HOOKS = (ROWOP_HOOKS + CNNOP_HOOKS + EXPLORE_ENTRIES + AUGMENT_ENTRIES + CLASSLOSS_ENTRIES + OPTIM_ENTRIES +
          PANELOP_HOOKS + SOFTTARGET_ENTRIES + MIX_ENTRIES + GEMMOP_HOOKS + REPORT_ENTRIES + WARP_ENTRIES +
          NORMALIZE_ENTRIES + COLOR_ENTRIES)
# the launchers marl_gemm_plan answers for (its `kind`)
GEMM_KINDS = ("nt", "lstm", "tn", "nt_images", "lstm_images", "tn_images", "tn_images_cell")
MARL_PANEL_MAX_LAYERS = 4


class PanelLayer(C.Structure):
    """Mirror of ``marl_panel_layer`` (include/marl_hip_panelops.h)."""

    _fields_ = [("w", C.c_void_p), ("ldw", C.c_int), ("bias", C.c_void_p), ("gamma", C.c_void_p),
                ("beta", C.c_void_p), ("n", C.c_int), ("z", C.c_void_p), ("ldz", C.c_int), ("stats", C.c_void_p),
                ("a", C.c_void_p), ("lda", C.c_int), ("a3", C.c_void_p), ("a3_row0", C.c_int), ("a3_steps", C.c_int),
                ("a3_col0", C.c_int)]


class PanelFwdProb(C.Structure):
    """Mirror of ``marl_panel_fwd_prob``."""

    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int), ("k0", C.c_int), ("m", C.c_int), ("nlayers", C.c_int),
                ("layer", PanelLayer * MARL_PANEL_MAX_LAYERS), ("agg_na", C.c_int), ("agg_nb", C.c_int),
                ("xbar", C.c_void_p), ("by_batch", C.c_int), ("g_na", C.c_int), ("g_nb", C.c_int),
                ("agg_at", C.c_int), ("ld_xbar", C.c_int), ("mix", C.c_void_p), ("sample", C.c_int),
                ("explore", C.c_int), ("gate_pos", C.c_void_p)]


class PanelCell(C.Structure):
    """Mirror of ``marl_panel_cell``."""

    _fields_ = [("dh", C.c_void_p), ("dc", C.c_void_p), ("gates", C.c_void_p), ("c_prev", C.c_void_p),
                ("c_new", C.c_void_p), ("lddh", C.c_int), ("lddc", C.c_int), ("ldg", C.c_int), ("ldc", C.c_int),
                ("n", C.c_int), ("g3", C.c_void_p), ("g3_row0", C.c_int), ("g3_steps", C.c_int),
                ("skip_f32", C.c_int)]


class PanelBwdLayer(C.Structure):
    """Mirror of ``marl_panel_bwd_layer``."""

    _fields_ = [("z", C.c_void_p), ("ldz", C.c_int), ("stats", C.c_void_p), ("gamma", C.c_void_p),
                ("beta", C.c_void_p), ("n", C.c_int), ("k_in", C.c_int), ("w", C.c_void_p), ("ldw", C.c_int),
                ("dz", C.c_void_p), ("lddz", C.c_int), ("part", C.c_void_p)]


class PanelBwdProb(C.Structure):
    """Mirror of ``marl_panel_bwd_prob``."""

    _fields_ = [("da", C.c_void_p), ("ldda", C.c_int), ("da2", C.c_void_p), ("ldda2", C.c_int),
                ("agg_na", C.c_int), ("agg_nb", C.c_int), ("m", C.c_int), ("nlayers", C.c_int),
                ("layer", PanelBwdLayer * MARL_PANEL_MAX_LAYERS), ("dx", C.c_void_p), ("lddx", C.c_int),
                ("accumulate", C.c_int), ("by_batch", C.c_int), ("g_na", C.c_int), ("g_nb", C.c_int),
                ("agg_at", C.c_int), ("mix", C.c_void_p), ("has_cellb", C.c_int), ("cellb", PanelCell),
                ("has_cell", C.c_int), ("cell", PanelCell), ("cell_rows", C.c_int64), ("gate_pos", C.c_void_p),
                ("cellb_img_done", C.c_int), ("cell_img_done", C.c_int)]


class PanelPlan(C.Structure):
    """Mirror of ``marl_panel_plan_info``."""

    _PER_LAYER = ("layer_waves", "nt", "ks", "kper", "empty", "rounds", "ln_slots")
    _fields_ = ([("waves", C.c_int), ("lds_bytes", C.c_int), ("blocks", C.c_int), ("cell_blocks", C.c_int),
                 ("by_batch", C.c_int * 2), ("nlayers", C.c_int)] +
                [(name, C.c_int * (2 * MARL_PANEL_MAX_LAYERS)) for name in _PER_LAYER] +
                [(name, C.c_int) for name in ("maxc", "tail_lds", "retried", "cell_vec4", "cellb_img_done",
                                              "cell_img_done")])

    def as_dict(self) -> dict:
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v)[: self.nlayers] if name in self._PER_LAYER else (list(v) if name == "by_batch" else v)
        return out


class GemmPlan(C.Structure):
    """Mirror of ``marl_gemm_plan_info`` (include/marl_hip_gemmops.h)."""

    _fields_ = ([(name, C.c_int32) for name in (
        "kind family variant row_id bm bn wm wn nst pipelined threads gx gy gz blocks xcd_map single_buf pre safe "
        "splits").split()] + [("rows_per_split", C.c_int64)] +
        [(name, C.c_int32) for name in "ok teams ih256 ih128 hh256 hh128".split()] +
        [("lds_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64)])

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class CnnBwdPlan(C.Structure):
    """Mirror of ``marl_cnn_bwd_plan_info`` (include/marl_hip_cnnops.h)."""

    _fields_ = [(name, C.c_int32) for name in (
        "wg_form wg_rb wg_chunks wg_blocks wg_sct wg_skt wg_tgc wg_tgk wg_ms wg_slabs wg_pd wg_pi "
        "dg_supported dg_rb dg_mt dg_nt dg_blocks").split()]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class CnnFwdIo(C.Structure):
    """Mirror of ``marl_cnn_fwd_io`` (include/marl_hip_cnnops.h)."""

    _fields_ = [("img", C.c_void_p), ("pos", C.c_void_p), ("obs", C.c_void_p), ("rows", C.c_int64),
                ("u", C.c_void_p), ("ldu", C.c_int32),
                ("z", C.c_void_p * MARL_MAX_CNN_LAYERS), ("gst", C.c_void_p * MARL_MAX_CNN_LAYERS),
                ("cols", C.c_void_p * MARL_MAX_CNN_LAYERS),
                ("u3", C.c_void_p), ("u3_row0", C.c_int32), ("u3_steps", C.c_int32)]


class CnnFwdPlan(C.Structure):
    """Mirror of ``marl_cnn_fwd_plan_info`` (include/marl_hip_cnnops.h)."""

    _fields_ = [("fused", C.c_int32), ("which", C.c_int32), ("rb", C.c_int32), ("blocks", C.c_int32),
                ("keeps_cols", C.c_int32 * MARL_MAX_CNN_LAYERS), ("writes_image", C.c_int32)]

    def as_dict(self) -> dict:
        out = {name: getattr(self, name) for name, _ in self._fields_}
        out["keeps_cols"] = list(self.keeps_cols)
        return out


_lib: Optional[C.CDLL] = None

_vp, _i, _i64, _f, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_u64 = C.c_uint64
_cfgp = C.POINTER(MarlConfig)


def _declare(lib: C.CDLL) -> None:
    lib.marl_abi_version.restype = _i
    lib.marl_last_error.restype = C.c_char_p
    lib.marl_param_numel.restype = _i64
    lib.marl_param_numel.argtypes = [_cfgp, _i]
    lib.marl_workspace_sizes.argtypes = [_cfgp, _i, C.POINTER(_sz), C.POINTER(_sz)]
    lib.marl_pack_weights.argtypes = [_cfgp, C.POINTER(_vp), _vp, _sz, _vp]
    lib.marl_patch_gather.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]
    lib.marl_transition.argtypes = [_vp, _vp, _vp, C.POINTER(C.c_int32), _i, _i, _i, _i, _i, _vp]
    lib.marl_episode_forward.argtypes = ([_cfgp, _vp, _sz, _vp, _sz] + [_vp] * 8 + [_u64, _u64, _vp] + [_vp] * 5 +
                                         [_i, _vp])
    lib.marl_episode_forward_probs.argtypes = ([_cfgp, _vp, _sz, _vp, _sz] + [_vp] * 8 + [_u64, _u64, _vp] +
                                               [_vp] * 6 + [_i, _vp])
    lib.marl_draw_episode.argtypes = [_cfgp, _u64, _u64, _vp] + [_vp] * 7
    lib.marl_counters_set.argtypes = [_vp, _u64, _i64, _f, _f, _f, _vp]
    lib.marl_counters_tick.argtypes = [_vp, _f, _f, _f, _vp]
    lib.marl_graph_begin.argtypes = [_vp]
    lib.marl_graph_end.argtypes = [_vp, C.POINTER(_vp)]
    lib.marl_graph_launch.argtypes = [_vp, _vp]
    lib.marl_graph_destroy.argtypes = [_vp]
    lib.marl_episode_backward.argtypes = [_cfgp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, C.POINTER(_vp), _vp]
    lib.marl_episode_backward_img.argtypes = ([_cfgp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, C.POINTER(_vp), _vp,
                                               _vp])
    lib.marl_episode_backward_probs.argtypes = ([_cfgp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, C.POINTER(_vp), _vp,
                                                 _vp, _vp])
    lib.marl_a2c_loss_entropy_fwd_bwd.argtypes = (
        [_cfgp, _vp, _sz, _vp, _vp, _vp, _vp, _f, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]
    )
    lib.marl_a2c_loss_fwd_bwd.argtypes = (
        [_cfgp, _vp, _sz, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp]
    )
    lib.marl_advantages.argtypes = [_cfgp, _vp, _sz, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _i, _vp]
    lib.marl_ppo_loss_fwd_bwd.argtypes = ([_cfgp, _vp, _sz] + [_vp] * 7 + [_f, _vp, _f] + [_vp] * 6)
    lib.marl_grad_clip.argtypes = [_vp, _i64, _f, _f, _vp, _vp, _sz, _vp]
    lib.marl_adam_step.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _f, _f, _f, _f, _f, _vp, _vp]
    lib.marl_step_forward.argtypes = ([_cfgp, _vp, _sz, _vp, _sz] + [_vp] * 15 + [_vp, _u64, _u64, _vp, _vp] +
                                      [_vp])
    lib.marl_step_forward_train.argtypes = lib.marl_step_forward.argtypes
    lib.marl_step_backward.argtypes = [_cfgp, _vp, _sz, _vp, _sz] + [_vp] * 10 + [C.POINTER(_vp)] + [_vp] * 6
    lib.marl_normalize_positions.argtypes = [_vp, _vp, _i, _i, _i, _vp]
    lib.marl_gemm_nt.argtypes = [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]
    lib.marl_gemm_nt_weights.argtypes = [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]
    lib.marl_gemm_weight_image_bytes.restype = _sz
    lib.marl_gemm_weight_image_bytes.argtypes = [_i, _i]
    lib.marl_gemm_tn.argtypes = [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i64, _vp, _sz, _vp]
    lib.marl_gemm_tn_scratch.restype = _sz
    lib.marl_gemm_tn_scratch.argtypes = [_i, _i, _i64]
    lib.marl_ln_silu_fwd.argtypes = [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _vp]
    lib.marl_image_bytes.restype = _sz
    lib.marl_image_bytes.argtypes = [_i64, _i]
    lib.marl_image_build.argtypes = [_vp, _i, _i64, _i, _vp, _vp]
    lib.marl_gemm_nt_images.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]
    lib.marl_gemm_nt_images_batch.argtypes = [_i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i),
                                              C.POINTER(_i), _i, _i, _i, _i, _vp]
    lib.marl_gemm_tn_images_scratch.restype = _sz
    lib.marl_gemm_tn_images_scratch.argtypes = [_i, _i, _i64]
    lib.marl_gemm_tn_images.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i64, _vp, _vp, _sz, _vp]
    lib.marl_lstm_images.argtypes = [_vp, _i] + [_vp] * 9 + [_i] * 6 + [_vp]
    lib.marl_cnn_wgrad.argtypes = ([_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64] + [_i] * 8 +
                                   [_vp, _vp, _vp, _sz, _vp])
    lib.marl_cnn_wgrad_scratch.restype = _sz
    lib.marl_cnn_wgrad_scratch.argtypes = [_i64, _i, _i, _i, _i, _i]
    lib.marl_tune.argtypes = [C.c_char_p, _i]
    lib.marl_tune_get.argtypes = [C.c_char_p, _i]
    lib.marl_profile_begin.argtypes = [_i, _i]
    lib.marl_profile_end.argtypes = [C.POINTER(C.c_double), C.POINTER(_i)]
    lib.marl_debug_buffer.argtypes = [_cfgp, _i, C.c_char_p, _i, C.POINTER(_i64), C.POINTER(_i)]
    lib.marl_gemm_tn_images_cell_scratch.restype = _sz
    lib.marl_gemm_tn_images_cell_scratch.argtypes = [_i, _i, _i, _i64]
    lib.marl_gemm_tn_images_cell.argtypes = [_vp, _i, _vp, _i, _vp, _i, _i64, _vp, _i, _vp, _i, _vp, _vp, _sz, _vp]
    lib.marl_plan_query.argtypes = [_cfgp, _i, C.c_char_p, C.POINTER(_i)]
    lib.marl_backward_heads_event.argtypes = [_vp]
    lib.marl_comm_matrix.argtypes = [_vp, _i]
    lib.marl_comm_grad_scratch_bytes.restype = _sz
    lib.marl_comm_grad_scratch_bytes.argtypes = [_cfgp]
    lib.marl_comm_grad.argtypes = [_cfgp, _vp, _sz, _vp, _sz, _i, _vp, _vp, _sz, _vp]
    lib.marl_comm_range.argtypes = [_i, _i, _i]
    lib.marl_policy_explore.argtypes = [_f, _f, _i]
    lib.marl_class_loss.argtypes = [_vp, _i, _f, _vp, _i, _i]
    _d = C.c_double
    lib.marl_optim_step.argtypes = [_vp, _vp, _vp, _vp, _vp, _i64, _f, _vp, _i, _d, _d, _d, _vp, _i64, _vp, _d, _vp,
                                    _vp]
    lib.marl_batch_augment.argtypes = [_vp, _i64, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, C.c_uint32, _vp]
    lib.marl_batch_augment_plan.argtypes = [_i, _i, _i, _i, _vp, _vp, _vp]
    lib.marl_batch_warp.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, C.c_uint32, _vp]
    lib.marl_batch_warp_plan.argtypes = [_i, _i, _i, _i, _vp, _vp, _vp]
    lib.marl_soft_targets.argtypes = [_vp, _i, _i]
    lib.marl_batch_mix.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, C.c_uint32, _vp]
    lib.marl_batch_mix_plan.argtypes = [_i, _i, _i, _i, _vp, _vp, _vp]
    lib.marl_batch_stats.argtypes = [_vp, _i64, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]
    lib.marl_batch_stats_scratch_bytes.restype = _sz
    lib.marl_batch_stats_scratch_bytes.argtypes = [_i] * 5
    lib.marl_batch_normalize.argtypes = [_vp, _i64, _vp, _vp, _i, C.POINTER(_d), _i, _i, _i, _i, _i, _vp, _vp, _vp]
    lib.marl_batch_normalize_plan.argtypes = [_i, _i, _i, _i, _vp, _vp, _vp]
    lib.marl_batch_color.argtypes = [_vp, _i64, _vp, _vp, _vp, _i, _i, C.POINTER(_d), _i, _i, _i, _i, _i, _vp, _vp, _vp]
    lib.marl_batch_color_plan.argtypes = [_i, _i, _i, _i, _i, _vp, _vp, _vp]
    lib.marl_report_layout.argtypes = [_i] * 6 + [C.POINTER(_i64)]
    lib.marl_report_scratch_bytes.restype = _sz
    lib.marl_report_scratch_bytes.argtypes = [_i] * 7
    lib.marl_episode_report.argtypes = [_vp, _vp] + [_i] * 6 + [C.POINTER(_f), _i, _i, _vp, _sz, _vp, _sz, _vp]
    lib.marl_ln_silu_bwd.argtypes = [_vp, _i, _vp, _i, _i, _vp, _i, _vp, _i] + [_vp] * 4 + [_i, _vp, _vp, _vp, _sz, _i, _i, _vp]
    lib.marl_gn_silu_bwd.argtypes = [_vp, _i64, _i] + [_vp] * 8 + [_sz, _i64, _i, _i, _i, _vp]
    lib.marl_gn_silu_fwd.argtypes = [_vp, _vp, _vp, _vp, _i64, _i, _vp, _i64, _i, _i, _i, _vp, _i, _i, _vp]
    lib.marl_ln_silu_dot_fwd.argtypes = [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]
    lib.marl_pos_embed_fwd.argtypes = [_vp, _vp, _i, _i] + [_vp] * 6 + [_i, _vp, _vp, _i, _i64, _i, _vp]
    lib.marl_lstm_cell_bwd.argtypes = ([_i] + [C.POINTER(_vp)] * 5 + [C.POINTER(_i)] * 5 +
                                       [C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i64, _vp])
    lib.marl_policy_dlogits.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _f, _f, _f, _vp]
    lib.marl_rowdot.argtypes = [_vp, _i, _vp, _vp, _vp, _i64, _i, _vp]
    lib.marl_agg_msg.argtypes = [_vp, _vp, _i, _i, _i, _i, _vp]
    lib.marl_cnn_dgrad.argtypes = [_vp, _vp, _i] + [_vp] * 8 + [_sz, _i64, _i, _i, _i, _i, _vp]
    lib.marl_cnn_dgrad_scratch.restype = _sz
    lib.marl_cnn_dgrad_scratch.argtypes = [_i64, _i, _i, _i, _i]
    lib.marl_cnn_bwd_plan.argtypes = [_i64, _i, _i, _i, _i, _i, C.POINTER(CnnBwdPlan)]
    lib.marl_cnn_fwd.argtypes = [_cfgp, _vp, _sz, C.POINTER(CnnFwdIo), _vp]
    lib.marl_cnn_fwd_plan.argtypes = [_cfgp, _i, _i64, C.POINTER(CnnFwdPlan)]
    lib.marl_panel_scratch_bytes.restype = _sz
    lib.marl_panel_scratch_bytes.argtypes = [_i, _i, C.POINTER(_i), C.POINTER(_i)]
    lib.marl_panel_fwd.argtypes = [C.POINTER(PanelFwdProb), _i, _vp, _sz, _vp]
    lib.marl_panel_bwd.argtypes = [C.POINTER(PanelBwdProb), _vp, _sz, _vp]
    lib.marl_gemm_plan.argtypes = [_i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _i64, _i, _i, C.POINTER(GemmPlan)]
    lib.marl_panel_plan.argtypes = [C.POINTER(PanelFwdProb), _i, C.POINTER(PanelBwdProb), C.POINTER(PanelPlan)]
    for name in EXPORTS + list(_HOOKS):
        fn = getattr(lib, name)
        if fn.restype is C.c_int and name not in ("marl_abi_version", "marl_tune_get"):
            fn.restype = _i


def load() -> C.CDLL:
    """Loads libmarl_hip.so; raises if it is missing or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP library is the only implementation of this "
            "package (no CPU fallback). Build it with `make -C marlclassification_amd/csrc` "
            "or `python -c 'import __graft_entry__ as g; g.build()'`."
        )
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in EXPORTS + list(_HOOKS) if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"{LIB_PATH} lacks symbols {missing}")
    _declare(lib)
    if lib.marl_abi_version() != MARL_ABI_VERSION:
        raise RuntimeError("libmarl_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().marl_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libmarl_hip error {rc}: {msg}")
