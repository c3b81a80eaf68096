"""ctypes binding of libseg2eye_hip.so (include/seg2eye_hip.h).

The library is the product path: if it is missing this module raises on import
of any op -- there is NO CPU or stock-torch fallback for the ops it exports.
"""
import ctypes as C
import os

import torch  # noqa: F401  -- MUST load before the library: both link libamdhip64 and the process must
#                       end up with torch's HIP runtime, or launches from the .so see "no ROCm-capable device"

_HERE = os.path.dirname(os.path.abspath(__file__))
# S2E_LIB_PATH: an alternative build of the SAME library (same-box A/B runs of experiment builds); never a fallback
LIB_PATH = os.environ.get('S2E_LIB_PATH') or os.path.join(_HERE, 'lib', 'libseg2eye_hip.so')

S2E_F32, S2E_BF16 = 0, 1
UNI_REPLICAS = 16           # S2E_UNI_REPLICAS of include/seg2eye_hip.h
SPADE_ANY_TILES, SPADE_DENSE, SPADE_ANY_RECTS, SPADE_X_HALF = 1, 2, 4, 8     # S2E_SPADE_* of include/seg2eye_hip.h: the fused launch's flags
ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
AUX_NONE, AUX_RELU_MASK, AUX_LRELU_GRAD = 0, 1, 2
NORM_SPADE_STYLE, NORM_PLAIN_IN, NORM_SPADE_STYLE_BATCH = 0, 1, 2
NORM_ACCUMULATE_DX = 0x100
LOSS_NEG_MEAN, LOSS_HINGE_REAL, LOSS_HINGE_FAKE, LOSS_L1, LOSS_L1_NANGRAD = 0, 1, 2, 3, 4
REGION_L1, REGION_L2 = 0, 1
RANK_L2, RANK_MISMATCH = 0, 1
MASK_ALL, MASK_LARGEST, MASK_BORDER = 0, 1, 2          # the mode bytes of s2e_mask_clean


class ConvDesc(C.Structure):
    """s2e_conv_desc"""
    _fields_ = [(n, C.c_int) for n in (
        'N', 'Hi', 'Wi', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride', 'pad',
        'transposed', 'in_act', 'out_act', 'aux_mode')]


class WgradC8Job(C.Structure):
    _fields_ = [('x', C.c_void_p), ('gy', C.c_void_p), ('dw_oihw', C.c_void_p), ('dbias', C.c_void_p),
                ('H', C.c_int), ('W', C.c_int), ('ncls', C.c_int), ('rect_list', C.c_void_p), ('rect_count', C.c_void_p)]


class WgradBatchJob(C.Structure):
    """s2e_wgrad_batch_job"""
    _fields_ = [('x', C.c_void_p), ('gy', C.c_void_p), ('dw', C.c_void_p), ('dbias', C.c_void_p),
                ('rect_list', C.c_void_p), ('rect_count', C.c_void_p),
                ('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('Cin', C.c_int), ('Cout', C.c_int), ('flags', C.c_int)]


class WgradMultiJob(C.Structure):
    """s2e_wgrad_multi_job"""
    _fields_ = [('x', C.c_void_p), ('gy', C.c_void_p), ('dw', C.c_void_p), ('dbias', C.c_void_p), ('d', ConvDesc)]


class LabelConvJob(C.Structure):
    _fields_ = [('weight', C.c_void_p), ('bias', C.c_void_p), ('out_off', C.c_long), ('h', C.c_int), ('w', C.c_int),
                ('cout', C.c_int), ('relu', C.c_int)]


class ClassTableJob(C.Structure):
    _fields_ = [('w_sh', C.c_void_p), ('b_sh', C.c_void_p), ('w_packed', C.c_void_p), ('bias', C.c_void_p), ('table_off', C.c_long),
                ('nh', C.c_int), ('C', C.c_int)]


class SnLayer(C.Structure):
    """s2e_sn_layer"""
    _fields_ = [('w', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p), ('t', C.c_void_p), ('s', C.c_void_p),
                ('rows', C.c_int), ('cols', C.c_int), ('tq', C.c_void_p), ('y', C.c_void_p), ('cin', C.c_int), ('taps', C.c_int)]


class PackJob(C.Structure):
    """s2e_pack_job"""
    _fields_ = [('w', C.c_void_p), ('out', C.c_void_p), ('sigma_index', C.c_int), ('cout', C.c_int), ('cin', C.c_int),
                ('taps', C.c_int), ('cin_pad', C.c_int), ('transposed', C.c_int), ('out_fwd', C.c_void_p)]


class GradJob(C.Structure):
    """s2e_grad_job"""
    _fields_ = [('gw_packed', C.c_void_p), ('out', C.c_void_p), ('w_orig', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p),
                ('sigma', C.c_void_p), ('cout', C.c_int), ('cin', C.c_int), ('taps', C.c_int), ('cin_pad', C.c_int),
                ('dot_index', C.c_int), ('reserved', C.c_int)]


class SpadeUniJob(C.Structure):
    """s2e_spade_uni_job"""
    _fields_ = [('R', C.c_void_p), ('A', C.c_void_p), ('w_gb', C.c_void_p), ('w_sc', C.c_long), ('w_sk', C.c_long), ('w_st', C.c_long),
                ('w_sh', C.c_void_p), ('b_sh', C.c_void_p), ('dw_sh', C.c_void_p), ('db_sh', C.c_void_p), ('dw_gb', C.c_void_p),
                ('db_gb', C.c_void_p), ('C2', C.c_int), ('nh', C.c_int), ('ncls', C.c_int), ('act_bf16', C.c_int)]


class SnGradJob(C.Structure):
    """s2e_sngrad_job"""
    _fields_ = [('g', C.c_void_p), ('w', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p), ('sigma', C.c_void_p),
                ('rows', C.c_int), ('cin', C.c_int), ('taps', C.c_int), ('part0', C.c_int), ('nparts', C.c_int), ('vmem0', C.c_int)]


_vp, _i, _l, _f = C.c_void_p, C.c_int, C.c_long, C.c_float
# What a function returns, by the kind its table entry names (read from its definition, not from its name):
#   STATUS  int: 0, or a negative S2E_ERR_* with s2e_last_error() set      COUNT  long: >= 0, or a negative S2E_ERR_* (no error text)
#   SIZE    size_t                    VALUE  a plain int answer (*_supported, *_kind, *_slots, *_pad, ...)                  TEXT  const char*
STATUS, COUNT, SIZE, VALUE, TEXT = 'status', 'count', 'size', 'value', 'text'
_RESTYPE = {STATUS: C.c_int, COUNT: C.c_long, SIZE: C.c_size_t, VALUE: C.c_int, TEXT: C.c_char_p}
# name -> (kind, argtypes).  Must list EVERY symbol declared in include/seg2eye_hip.h, as the header declares it
# (tests/test_abi_and_host.py compares names, arguments, return types and the job structures: header <-> table <-> .so).
SIGNATURES = {
    's2e_version': (VALUE, []),
    's2e_last_error': (TEXT, []),
    's2e_conv_cout_pad': (VALUE, [_i]),
    's2e_conv_k_pad': (VALUE, [_i, _i]),
    's2e_pack_conv_weight': (STATUS, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_sn_block_shape': (STATUS, [_i, _vp, _vp]),
    's2e_sn_power_iteration': (STATUS, [_vp, _i, _vp, _i, _vp, _i, _vp, C.c_size_t, _vp, _i, _i, _f, _vp]),
    's2e_sn_weight_grad': (STATUS, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_grad_block_map': (COUNT, [_vp, _i, _vp]),
    's2e_sngrad_block_map': (COUNT, [_vp, _i, _vp]),
    's2e_sngrad_scratch_floats': (COUNT, [_vp, _i]),
    's2e_sn_grads_inplace': (STATUS, [_vp, _vp, _i, _vp, _vp]),
    's2e_weight_grads_batched': (STATUS, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    's2e_unpack_weight_grad': (STATUS, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_pack_block_map': (COUNT, [_i, _vp, _i, _vp]),
    's2e_pack_conv_weights': (STATUS, [_i, _vp, _vp, _i, _i, _vp, _vp]),
    's2e_conv2d_workspace_bytes': (SIZE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d_kernel_kind': (VALUE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d_wgrad_kernel_kind': (VALUE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp, C.c_size_t, _vp]),
    's2e_conv2d_plane_supported': (VALUE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv_plane_weight_elems': (SIZE, [C.POINTER(ConvDesc)]),
    's2e_conv2d_plane': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp]),
    's2e_conv2d_stats_slots': (VALUE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d_stats': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp, _vp]),
    's2e_in_stats_from_partials': (STATUS, [_vp, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    's2e_label_rect_lists_bwd': (STATUS, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    's2e_conv2d_rects_supported': (VALUE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d_rects': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp, _vp, _vp]),
    's2e_conv2d_wgrad_rects_workspace_bytes': (SIZE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d_wgrad_rects': (STATUS, [_i, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_spade_uniform_sums': (STATUS, [_i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    's2e_spade_uniform_grads': (STATUS, [_vp, _i, _vp]),
    's2e_conv2d_wgrad_workspace_bytes': (SIZE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d_wgrad': (STATUS, [_i, _vp, _vp, _vp, _vp, C.POINTER(ConvDesc), _vp, C.c_size_t, _vp]),
    's2e_conv2d_wgrad_multi_supported': (VALUE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d_wgrad_multi_kind': (VALUE, [_i, C.POINTER(ConvDesc)]),
    's2e_conv2d_wgrad_multi_workspace_bytes': (SIZE, [_i, _vp, _i]),
    's2e_conv2d_wgrad_multi': (STATUS, [_i, _vp, _i, _vp, C.c_size_t, _vp]),
    's2e_in_stats_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_modulate_bwd_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_instance_norm_fwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    's2e_instance_norm_bwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    's2e_in_stats': (STATUS, [_i, _vp, _i, _i, _i, _f, _vp, _vp, _vp]),
    's2e_modulate_fwd': (STATUS, [_i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    's2e_modulate_bwd': (STATUS, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, C.c_double, _i, _i, _vp]),
    's2e_spade_conv_modulate_rect': (VALUE, [_i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    's2e_label_rect_classify': (STATUS, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    's2e_spade_conv_modulate_sparse': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    's2e_spade_class_table': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    's2e_spade_modulate_uniform': (STATUS, [_i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_spade_conv_modulate_supported': (VALUE, [_i, _i, _i, _i, _i, _i, _i]),
    's2e_spade_conv_modulate': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_colsum': (STATUS, [_i, _vp, _l, _i, _vp, _vp]),
    's2e_wgrad_c8_batch_supported': (VALUE, [_i, _i, _i, _i]),
    's2e_wgrad_c8_batch_workspace_bytes': (SIZE, [_i, _vp, _i]),
    's2e_wgrad_c8_batch': (STATUS, [_i, _i, _vp, _i, _vp, C.c_size_t, _vp]),
    's2e_wgrad_batch_supported': (VALUE, [_i, _i, _i, _i, _i, _i]),
    's2e_wgrad_batch_workspace_bytes': (SIZE, []),
    's2e_wgrad_batch': (STATUS, [_i, _vp, _i, _vp, C.c_size_t, _vp]),
    's2e_label_conv_block_map': (COUNT, [_i, _vp, _i, _i, _vp]),
    's2e_label_conv3x3_batch': (STATUS, [_i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    's2e_class_table_block_map': (COUNT, [_vp, _i, _vp]),
    's2e_spade_class_table_batch': (STATUS, [_i, _vp, _vp, _i, _vp, _i, _vp]),
    's2e_label_conv3x3': (STATUS, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_onehot_nhwc': (STATUS, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_d_input_aug_workspace_bytes': (SIZE, [_i, _i, _i]),
    's2e_d_input_aug': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_d_input_aug_bwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    's2e_openeds_error': (STATUS, [_i, _vp, _vp, _i, _i, _i, _vp, _vp]),
    's2e_openeds_error_u8': (STATUS, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    's2e_resize_to255': (STATUS, [_i, _vp, _i, _i, _i, _vp, _i, _i, _vp]),
    's2e_ssim_workspace_bytes': (SIZE, [_i, _i, _i]),
    's2e_ssim_fwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_ssim_u8': (STATUS, [_vp, _vp, _i, _i, _i, _vp, _vp, C.c_size_t, _vp]),
    's2e_ssim_bwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    's2e_msssim_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_msssim_pyramid_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_msssim_maps_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_msssim_fwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    's2e_msssim_u8': (STATUS, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    's2e_msssim_bwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, C.c_size_t, _vp, _vp]),
    's2e_ffl_tables_bytes': (SIZE, [_i, _i]),
    's2e_ffl_workspace_bytes': (SIZE, [_i, _i, _i]),
    's2e_ffl_spectrum_bytes': (SIZE, [_i, _i, _i]),
    's2e_ffl_tables': (STATUS, [_i, _i, _vp, C.c_size_t, _vp]),
    's2e_ffl_fwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _f, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    's2e_ffl_u8': (STATUS, [_vp, _vp, _i, _i, _i, _f, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    's2e_ffl_bwd': (STATUS, [_i, _vp, _vp, _vp, _i, _i, _i, _f, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp]),
    's2e_region_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_region_loss_fwd': (STATUS, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_region_stats_u8': (STATUS, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, C.c_size_t, _vp]),
    's2e_region_loss_bwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    's2e_mask_dist': (STATUS, [_vp, _vp, _i, _i, _l, _l, _i, _i, _vp, _vp]),
    's2e_rank_topk_max_candidates': (VALUE, []),
    's2e_rank_topk': (STATUS, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    's2e_seg_ce_workspace_bytes': (SIZE, [_i, _i, _i]),
    's2e_seg_ce_fwd': (STATUS, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_seg_ce_bwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    's2e_seg_argmax_u8': (STATUS, [_i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    's2e_seg_confusion_u8': (STATUS, [_vp, _vp, _l, _i, _vp, _vp]),
    's2e_seg_dist_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_seg_dist_maps': (STATUS, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_seg_loss_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_seg_loss_fwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_seg_loss_bwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp, _vp]),
    's2e_mask_clean_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_mask_components': (STATUS, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    's2e_mask_clean': (STATUS, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_rim_moments_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_rim_moments': (STATUS, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_ellipse_paint': (STATUS, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    's2e_refine_input': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    's2e_refine_head_workspace_bytes': (SIZE, [_i, _i, _i]),
    's2e_refine_head_fwd': (STATUS, [_i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_refine_head_bwd': (STATUS, [_i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _f, _f, _vp, _vp]),
    's2e_refine_predict_u8': (STATUS, [_i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp]),
    's2e_bilinear_resize_fwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    's2e_bilinear_resize_bwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    's2e_upsample2x_fwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    's2e_upsample2x_bwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    's2e_avgpool3x3s2_fwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    's2e_avgpool3x3s2_bwd': (STATUS, [_i, _vp, _vp, _i, _i, _i, _i, _vp]),
    's2e_tanh_bwd': (STATUS, [_i, _vp, _vp, _vp, _l, _vp]),
    's2e_lrelu_bwd': (STATUS, [_i, _vp, _vp, _vp, _l, _vp]),
    's2e_loss_reduce': (STATUS, [_i, _i, _vp, _vp, _l, _f, _vp, _vp]),
    's2e_loss_grad': (STATUS, [_i, _i, _vp, _vp, _l, _f, _vp, _vp, _i, _vp]),
    's2e_style_fc_supported': (VALUE, [_i, _i]),
    's2e_style_fc_bwd_workspace_bytes': (SIZE, [_i, _i, _i]),
    's2e_style_fc_fwd': (STATUS, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    's2e_style_fc_bwd': (STATUS, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _i, _i, _i, _f, _vp]),
    's2e_fc_head_supported': (VALUE, [_i, _i]),
    's2e_fc_head_fwd_workspace_bytes': (SIZE, [_i, _i, _i, _i]),
    's2e_fc_head_fwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, C.c_size_t, _vp]),
    's2e_fc_head_bwd': (STATUS, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    's2e_adam_flat': (STATUS, [_vp, _vp, _vp, _vp, _l, _vp, _vp]),
    's2e_adam_flat_ema': (STATUS, [_vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp]),
    's2e_grad_guard_workspace_bytes': (SIZE, [_l]),
    's2e_grad_guard': (STATUS, [_vp, _l, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    's2e_adam_flat_guarded': (STATUS, [_vp, _vp, _vp, _vp, _l, _vp, _vp, _vp]),
    's2e_adam_flat_ema_guarded': (STATUS, [_vp, _vp, _vp, _vp, _vp, _l, _vp, _vp, _vp, _vp]),
    's2e_shard_sum': (STATUS, [_i, _vp, _vp, _i, _l, _vp]),
    's2e_resize_bicubic_u8': (STATUS, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    's2e_resize_nearest_u8': (STATUS, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    's2e_augment_pairs': (STATUS, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    's2e_sidebyside_ws_bytes': (COUNT, [_i, _i, _i]),
    's2e_sidebyside_u8': (STATUS, [_i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _l, _vp, _vp, _vp, _vp]),
}

_lib = None


class Seg2EyeHipError(RuntimeError):
    pass


def _bind(errcheck):
    """A CDLL of the library with every table entry's argtypes / restype set (handles of one library share the dlopen handle
    and have their own function objects).  errcheck: kind -> ctypes errcheck hook, for the kinds that get one."""
    if not os.path.exists(LIB_PATH):
        raise Seg2EyeHipError(
            'libseg2eye_hip.so not found at %s -- build it with `python -m seg2eye_amd.build` '
            '(or __graft_entry__.build()).  There is no fallback path.' % LIB_PATH)
    dll = C.CDLL(LIB_PATH)
    for name, (kind, argtypes) in SIGNATURES.items():
        fn = getattr(dll, name)
        fn.argtypes, fn.restype = argtypes, _RESTYPE[kind]
        if kind in errcheck:
            fn.errcheck = errcheck[kind]
    return dll


def lib():
    """Load (once) and return the raw CDLL: integers come back as integers.  Raises if the extension has not been built."""
    global _lib
    if _lib is None:
        _lib = _bind({})
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().s2e_last_error()
        raise Seg2EyeHipError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else '?'))


def _status(rc, func, args):
    if rc:
        check(rc, func.__name__)
    return rc


def _count(n, func, args):
    if n < 0:                                                # (the planners return the code without setting the error text)
        raise Seg2EyeHipError('%s failed (%d)' % (func.__name__, n))
    return n


class _Checked:
    """L.call.s2e_x(...): the same symbols with the error handling installed as ctypes' errcheck -- a STATUS entry raises
    Seg2EyeHipError with the library's message on a non-zero result, a COUNT entry on a negative one; the others are plain.
    Bound on the first attribute access; after that every function is an entry of the instance dictionary."""

    def __getattr__(self, name):
        dll = _bind({STATUS: _status, COUNT: _count})
        self.__dict__.update((n, getattr(dll, n)) for n in SIGNATURES)
        return getattr(dll, name)


call = _Checked()
