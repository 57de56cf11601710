"""ctypes binding of libmvae_hip.so (the C ABI declared in include/mvae_hip.h).

The library is the product: there is no CPU / eager-PyTorch fallback.  ``lib()`` raises
``RuntimeError`` when the shared object has not been built (``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C multimodal-vae-public_amd/csrc``), and every
wrapper in ``ops.py`` raises when it is handed a non-GPU tensor.
"""
import ctypes
import os
from ctypes import c_double, c_float, c_int, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmvae_hip.so')

MVAE_OK = 0
ERRORS = {-1: 'MVAE_ERR_ARG (bad shape / null pointer / unsupported stride)',
          -2: 'MVAE_ERR_LAUNCH (hip kernel launch failed)',
          -3: 'MVAE_ERR_WS (workspace too small)',
          -4: 'MVAE_ERR_COMM (RCCL not loadable, or an RCCL / HIP runtime call of mvae_comm_* failed)'}
COMM_ID_BYTES = 128   # MVAE_COMM_ID_BYTES
ACT_SWISH = 1
ACCUMULATE = 2
POE_NO_PRIOR = 4     # MVAE_POE_NO_PRIOR
POE_VARIANT = {'A': 0, 'B': 1, 'A-noprior': 0 | POE_NO_PRIOR, 'B-noprior': 1 | POE_NO_PRIOR}
MAX_EXPERTS = 32
STATS_TILE_ELEMS = 512   # MVAE_STATS_TILE_ELEMS
MAX_TERMS = 40
# mvae_conv_k4_route: the launches (MVAE_OP_*) and the kernels they take (MVAE_ROUTE_*)
CONV_OPS = {'conv_fwd': 0, 'conv_dgrad': 1, 'conv_wgrad': 2, 'convT_fwd': 3, 'convT_fwd_stats': 4, 'convT_dgrad': 5,
            'convT_wgrad': 6}
CONV_ROUTES = {1: 'igemm', 2: 'igemm_pair', 3: 'gemm2', 4: 'conv_patch', 5: 'small_fwd16', 6: 'small_fwd32',
               7: 'dgrad_small3d', 8: 'dgrad_small3', 9: 'dgrad_small2', 10: 'dgrad_small', 11: 's1', 12: 's1_wide',
               13: 'patch8', 14: 'patch7', 15: 'patch16', 16: 'patch_stats', 17: 'wgrad_smallcin',
               18: 'wgrad_smallcin2', 19: 'wgrad_patch'}

# mvae_linear_route / mvae_linear_wgrad_batched_route: the launches (MVAE_LOP_*), the forward's output forms
# (MVAE_LFORM_*), the kernels (MVAE_LROUTE_*) and the launches that sum split partials (MVAE_LFINISH_*)
LINEAR_OPS = {'fwd': 0, 'bce_fwd': 1, 'ce_fwd': 2, 'dgrad': 3, 'wgrad': 4}
LINEAR_FORMS = {'other': 0, 'pre+act': 1, 'act': 2}
LINEAR_FINISH = {0: None, 1: 'finish', 2: 'finish_few', 3: 'finish_few_vec', 4: 'g2_finish'}
LINEAR_ROUTES = {1: 'gemm2', 2: 'g2s_32x64_k4', 3: 'g2s_64x32_k4', 4: 'g2s_32x64_k2', 5: 'g2s_64x32_k2',
                 6: 'g2s_32x32_k8', 7: 'g2s_32x32_k4', 8: 'igs_64x32_k4', 9: 'igs_64x32_k2', 10: 'igs_32x64_k4',
                 11: 'igs_32x64_k2', 12: 'igs_32x32_k8', 13: 'igs_32x32_k4', 14: 'ig_32x128', 15: 'ig_128x128',
                 16: 'ig_128x64', 17: 'ig_64x128',
                 18: 'ig_64x64_k4', 19: 'ig_64x64_k2', 20: 'ig_64x64', 30: 'ig_32x128_s', 31: 'ig_128x128_s',
                 32: 'ig_128x64_s', 33: 'ig_64x128_s',
                 34: 'ig_64x64_k4_s', 35: 'ig_64x64_k2_s', 36: 'ig_64x64_s', 40: 'dgrad_smalln', 41: 'wgrad_direct_4',
                 42: 'wgrad_direct_8', 43: 'wgrad_direct_16', 50: 'wgrad_batched2', 51: 'wgrad_batched',
                 52: 'wgrad_batched_adam'}

# mvae_bn_route: the kernels the training-mode BatchNorm launches choose between (MVAE_BNROUTE_*)
BN_ROUTES = {1: 'two_vec_rows', 2: 'two_vec_cols', 3: 'two_scalar', 4: 'fused_vec_g1', 5: 'fused_vec_g2',
             6: 'fused_vec_g3', 7: 'fused_scalar_g1', 8: 'fused_scalar_gn', 9: 'bn1d_g1', 10: 'bn1d_gn', 11: 'slice'}

# mvae_bce_route: the kernels the BCE row-sum launches choose between (MVAE_BCEROUTE_*) and the two thresholds of loss.hip
BCE_ROUTES = {1: 'wave', 2: 'block_scalar', 3: 'block_vec', 4: 'block_vec_batched'}
BCE_BLOCK_MIN_P = 512    # MVAE_BCE_BLOCK_MIN_P
ELBO_LONG_GROUP = 2048   # MVAE_ELBO_LONG_GROUP


class Experts(ctypes.Structure):
    _fields_ = [('mu', c_void_p * MAX_EXPERTS), ('logvar', c_void_p * MAX_EXPERTS)]


class ElboPart(ctypes.Structure):
    _fields_ = [('rows', c_void_p), ('coef', c_void_p), ('term_of', c_void_p), ('first_term', c_int),
                ('groups', c_int), ('rows_per_group', c_int)]


ELBO_MAX_PARTS = 4


class WgradItem(ctypes.Structure):          # mvae_wgrad_item
    _fields_ = [('dy', c_void_p), ('lddy', c_int), ('x', c_void_p), ('ldx', c_int), ('dw', c_void_p),
                ('db', c_void_p), ('M', c_int), ('N', c_int), ('K', c_int), ('flags', c_int)]


WGRAD_BATCH_MAX = 16


class AdamFuse(ctypes.Structure):           # mvae_adam_fuse
    _fields_ = [('grad_base', c_void_p), ('param_base', c_void_p), ('exp_avg_base', c_void_p),
                ('exp_avg_sq_base', c_void_p), ('coef2', c_void_p), ('beta1', ctypes.c_double),
                ('beta2', ctypes.c_double), ('eps', ctypes.c_double), ('grad_scale', ctypes.c_float)]


class RepackItem(ctypes.Structure):         # mvae_repack_item
    _fields_ = [('w', c_void_p), ('wr', c_void_p), ('transposed', c_int), ('Cin', c_int), ('Cout', c_int),
                ('stride', c_int), ('pad', c_int)]


REPACK_MAX = 16


class BceSeg(ctypes.Structure):             # mvae_bce_seg
    _fields_ = [('logits', c_void_p), ('target', c_void_p), ('dlogits', c_void_p), ('P', c_int), ('weight', c_float)]


BCE_MULTI_MAX = 8
IW_FOLD_MAX = 64      # MVAE_IW_FOLD_MAX
POE_TABLE_MAX_A = 32  # MVAE_POE_TABLE_MAX_A
PREDICT_MAX_C = 64    # MVAE_PREDICT_MAX_C
PREDICT_CATEGORICAL, PREDICT_BERNOULLI = 0, 1      # MVAE_PREDICT_*


class ExpertGrads(ctypes.Structure):
    _fields_ = [('dmu', c_void_p * MAX_EXPERTS), ('dlogvar', c_void_p * MAX_EXPERTS)]


P = c_void_p
_SIGNATURES = {
    'mvae_abi_version': (c_int, []),
    'mvae_gemm_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'mvae_linear_fwd': (c_int, [P, c_int, P, P, P, P, c_int, P, c_float, c_int, c_int, c_int, P, c_size_t, P]),
    'mvae_linear_bce_fwd': (c_int, [P, c_int, P, P, P, c_int, c_int, P, c_int, P, c_int, P, P, c_int, c_int, c_int, P]),
    'mvae_linear_ce_fwd': (c_int, [P, c_int, P, P, P, c_int, P, c_int, P, c_int, P, P, c_int, c_int, c_int, P]),
    'mvae_linear_dgrad': (c_int, [P, c_int, P, P, c_int, P, P, c_float, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    'mvae_linear_wgrad': (c_int, [P, c_int, P, c_int, P, P, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    'mvae_linear_fwd_grouped': (c_int, [P, c_int, c_size_t, P, c_size_t, P, c_size_t, P, P, c_int, c_size_t,
                                        c_int, c_int, c_int, c_int, P, c_size_t, P]),
    'mvae_linear_dgrad_grouped': (c_int, [P, c_int, c_size_t, P, c_size_t, P, c_int, c_size_t, P, c_size_t,
                                          c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    'mvae_linear_wgrad_grouped': (c_int, [P, c_int, c_size_t, P, c_int, c_size_t, P, c_size_t, P, c_size_t,
                                          c_int, c_int, c_int, c_int, c_int, P, c_size_t, P]),
    'mvae_conv2d_k4_fwd': (c_int, [P, P, P, P] + [c_int] * 7 + [P]),
    'mvae_conv2d_k4_dgrad': (c_int, [P, P, P, P] + [c_int] * 7 + [P, c_size_t, P]),
    'mvae_conv2d_k4_wgrad': (c_int, [P, P, P] + [c_int] * 8 + [P, c_size_t, P]),
    'mvae_convT2d_k4_fwd': (c_int, [P, P, P, P] + [c_int] * 7 + [P, c_size_t, P]),
    'mvae_convT2d_k4_dgrad': (c_int, [P, P, P, P] + [c_int] * 7 + [P]),
    'mvae_convT2d_k4_wgrad': (c_int, [P, P, P] + [c_int] * 8 + [P, c_size_t, P]),
    'mvae_bn_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'mvae_bn_train_fwd': (c_int, [P] * 8 + [c_int] * 4 + [c_float, c_float, c_int, P, c_int, P, c_size_t, P]),
    'mvae_bn_train_bwd': (c_int, [P] * 9 + [c_int] * 5 + [P, c_size_t, P]),
    'mvae_bn_eval_fwd': (c_int, [P] * 6 + [c_int] * 3 + [c_float, c_int, P]),
    'mvae_bn_route': (c_int, [c_int] * 6 + [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'mvae_swish_fwd': (c_int, [P, P, c_size_t, P]),
    'mvae_swish_bwd': (c_int, [P, P, P, c_size_t, P]),
    'mvae_sigmoid_fwd': (c_int, [P, P, c_size_t, P]),
    'mvae_affine_fwd': (c_int, [P, P, P, P, c_size_t, c_size_t, P]),
    'mvae_embedding_swish_fwd': (c_int, [P, c_int, P, P, c_int, c_int, c_int, P]),
    'mvae_embedding_swish_bwd': (c_int, [P, c_int, P, P, P, c_int, c_int, c_int, c_int, P]),
    'mvae_embedding_swish_fwd_grouped': (c_int, [P, c_int, c_size_t, P, c_size_t, P, c_size_t, c_int, c_int, c_int,
                                                 c_int, P]),
    'mvae_embedding_swish_bwd_grouped': (c_int, [P, c_int, c_size_t, P, c_size_t, P, c_size_t, P, c_int, c_int,
                                                 c_int, c_int, c_int, P]),
    'mvae_resample_ksize': (c_int, [c_int, c_int]),
    'mvae_resample_coeffs': (c_int, [c_int, c_int, P, P]),
    'mvae_resize_crop_u8_to_f32': (c_int, [P, P] + [c_int] * 8 + [P, P, c_int, P, P, c_int, c_int, c_int, P]),
    'mvae_u8_to_f32': (c_int, [P, P, c_size_t, P]),
    'mvae_poe_fwd': (c_int, [ctypes.POINTER(Experts), c_int, c_int, P, c_int, P, P, P, P, P,
                             c_int, c_int, c_int, P]),
    'mvae_poe_fwd_draw': (c_int, [ctypes.POINTER(Experts), c_int, c_int, P, c_int, P, c_uint64, P, c_uint64, P, P, P, P,
                                  c_int, c_int, c_int, P]),
    'mvae_poe_bwd': (c_int, [ctypes.POINTER(Experts), c_int, c_int, P, c_int, P, P, P, P, P, P, P, c_int,
                             ctypes.POINTER(ExpertGrads), c_int, c_int, c_int, c_int, P]),
    'mvae_poe_bwd_split': (c_int, [ctypes.POINTER(Experts), c_int, c_int, P, c_int, P, P, P, P,
                                   ctypes.POINTER(c_int), P, ctypes.POINTER(c_int), P, c_int,
                                   ctypes.POINTER(ExpertGrads), c_int, c_int, c_int, c_int, P]),
    'mvae_kl_rows_fwd': (c_int, [P, P, P, c_int, c_int, P]),
    'mvae_kl_rows_bwd': (c_int, [P, P, P, P, P, c_int, c_int, P]),
    'mvae_bce_rowsum_fwd': (c_int, [P, P, P, P, P, P] + [c_int] * 7 + [P]),
    'mvae_bce_rowsum_bwd': (c_int, [P, P, P, P, P] + [c_int] * 7 + [P]),
    'mvae_bce_route': (c_int, [c_int] * 4 + [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'mvae_ce_fwd': (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    'mvae_ce_bwd': (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P]),
    'mvae_group_sums': (c_int, [P, P, P, P, c_int, c_int, c_int, P]),
    'mvae_conv_k4_repack_floats': (c_size_t, [c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'mvae_conv_k4_repack_batched': (c_int, [ctypes.POINTER(RepackItem), c_int, P]),
    'mvae_convT2d_k4_stats_tiles': (c_size_t, [c_int] * 7),
    'mvae_convT2d_k4_fwd_stats': (c_int, [P, P, P, c_size_t] + [c_int] * 7 + [P, c_size_t, P]),
    'mvae_conv_k4_route': (c_int, [c_int] * 8 + [c_size_t, ctypes.POINTER(c_int)]),
    'mvae_linear_route': (c_int, [c_int] * 7 + [c_size_t, c_size_t, c_int, c_int, c_int, c_size_t, ctypes.POINTER(c_int),
                                  ctypes.POINTER(c_int)]),
    'mvae_linear_wgrad_batched_route': (c_int, [ctypes.POINTER(WgradItem), c_int, c_int, ctypes.POINTER(c_int),
                                                ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    # K17: the general stride-2 conv family (ks in {4, 5}, pad in {0, 1}, any map size)
    'mvae_conv2d_gen_fwd': (c_int, [P, P, P, P] + [c_int] * 8 + [P]),
    'mvae_conv2d_gen_dgrad': (c_int, [P, P, P, P] + [c_int] * 8 + [P, c_size_t, P]),
    'mvae_conv2d_gen_wgrad': (c_int, [P, P, P] + [c_int] * 9 + [P, c_size_t, P]),
    'mvae_convT2d_gen_fwd': (c_int, [P, P, P, P] + [c_int] * 8 + [P, c_size_t, P]),
    'mvae_convT2d_gen_dgrad': (c_int, [P, P, P, P] + [c_int] * 8 + [P]),
    'mvae_convT2d_gen_wgrad': (c_int, [P, P, P] + [c_int] * 9 + [P, c_size_t, P]),
    'mvae_conv_gen_ws_bytes': (c_size_t, [c_int] * 9),
    'mvae_conv_gen_supported': (c_int, [c_int] * 9),
    'mvae_bn_stats_merge': (c_int, [P, c_int, c_int, c_int, c_int, P, P, P, P, c_float, c_float, c_int, P, P]),
    'mvae_linear_wgrad_batched': (c_int, [ctypes.POINTER(WgradItem), c_int, P]),
    'mvae_linear_wgrad_batched_adam': (c_int, [ctypes.POINTER(WgradItem), c_int, ctypes.POINTER(AdamFuse), P]),
    'mvae_adam_prepare': (c_int, [P, ctypes.c_int64, c_double, c_double, c_double, P, P]),
    'mvae_elbo_reduce': (c_int, [ctypes.POINTER(ElboPart), c_int, P, c_int, P, c_size_t, P, c_uint64, P]),
    'mvae_elbo_reduce_prepare': (c_int, [ctypes.POINTER(ElboPart), c_int, P, c_int, P, c_size_t, P, c_uint64, P,
                                         ctypes.c_int64, c_double, c_double, c_double, P, P]),
    'mvae_philox_fill': (c_int, [P, c_size_t, c_int, c_float, c_uint64, P, c_uint64, P]),
    'mvae_randn': (c_int, [P, c_size_t, c_uint64, P, P]),
    'mvae_bernoulli': (c_int, [P, c_size_t, c_float, c_uint64, P, P]),
    'mvae_adam_step': (c_int, [P, P, P, P, c_size_t, c_double, c_double, c_double, c_double, c_float, P, P]),
    'mvae_adam_apply': (c_int, [P, P, P, P, c_size_t, c_double, c_double, c_double, c_double, c_float, P, P]),
    'mvae_adam_apply_at': (c_int, [P, P, P, P, c_size_t, c_double, c_double, c_double, c_double, c_float, P,
                                   ctypes.c_int64, P]),
    'mvae_adam_apply_coef': (c_int, [P, P, P, P, c_size_t, P, c_double, c_double, c_double, c_float, P]),
    'mvae_counter_add': (c_int, [P, ctypes.c_int64, P]),
    'mvae_trace_marker': (c_int, [c_int, P]),
    'mvae_fill': (c_int, [P, c_size_t, c_float, P]),
    'mvae_ingest': (c_int, [P, P, c_size_t, P, P, c_size_t, P, P, c_size_t, P]),
    'mvae_reparam_fwd': (c_int, [P, P, P, P, c_size_t, P]),
    'mvae_reparam_bwd': (c_int, [P, P, P, P, P, c_size_t, P]),
    'mvae_dropout_fanout_fwd': (c_int, [P, P, P, c_float, c_int, c_int, c_int, P]),
    'mvae_dropout_fanin_bwd': (c_int, [P, P, P, c_float, c_int, c_int, c_int, P]),
    'mvae_block_gather': (c_int, [P, P, P, c_int, c_size_t, P]),
    'mvae_block_scatter_add': (c_int, [P, P, P, c_int, c_int, c_size_t, P]),
    'mvae_scatter_sums': (c_int, [P, P, P, P, P, c_int, c_int, P]),
    'mvae_bce_elem_fwd': (c_int, [P, P, P, c_size_t, P]),
    'mvae_bce_elem_bwd': (c_int, [P, P, P, P, P, c_size_t, P]),
    # K16: the recurrent text stacks of MultiMNIST
    'mvae_gru_cell_fwd': (c_int, [P, c_int, P, c_int, P, c_int, P, c_int, P, c_int, c_int, P]),
    'mvae_gru_cell_bwd': (c_int, [P, c_int, P, c_int, P, P, c_int, P, P, P, c_int, c_int, P]),
    'mvae_embedding_fwd': (c_int, [P, c_int, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    'mvae_embedding_bwd': (c_int, [P, c_int, P, P, c_int, P, c_int, c_int, c_int, c_int, P]),
    'mvae_copy2d': (c_int, [P, c_int, P, c_int, P, c_int, c_float, c_int, c_int, c_int, P]),
    'mvae_argmax_rows': (c_int, [P, c_int, P, c_int, c_int, P]),
    # K18: the whole greedy TextDecoder in one launch per direction
    'mvae_gru_dec_seq_supported': (c_int, [c_int] * 5),
    'mvae_gru_dec_seq_fwd': (c_int, [P] * 14 + [c_float] + [P] * 9 + [c_int] * 6 + [P]),
    'mvae_gru_dec_seq_bwd': (c_int, [P] * 7 + [c_float] + [P] * 12 + [c_int] * 5 + [P]),
    # K19: the whole TextEncoder in one launch per direction
    'mvae_gru_enc_seq_supported': (c_int, [c_int] * 6),
    'mvae_gru_enc_seq_fwd': (c_int, [P] * 19 + [c_int] * 5 + [P]),
    'mvae_gru_enc_seq_bwd': (c_int, [P] * 13 + [c_int] * 5 + [P]),
    # K20: the importance-weighted log-likelihood (draw + density ratio, streaming log-mean-exp)
    'mvae_iw_draw': (c_int, [P, P, c_int, P, c_uint64, P, c_uint64, P, P, P, c_int, c_int, c_int, P]),
    'mvae_iw_accumulate': (c_int, [P, P, c_int, P, c_int, P, P, c_int, c_int, c_int, P]),
    # K21: the MultiMNIST dataset builder's compose step
    'mvae_multimnist_compose': (c_int, [P, c_int, P, c_int, P, P, P, P, P]),
    # K22: the BCE row sums of several image modalities in one launch
    'mvae_bce_multi_ws_bytes': (c_size_t, [ctypes.POINTER(BceSeg), c_int, c_int]),
    'mvae_bce_multi_fwd': (c_int, [ctypes.POINTER(BceSeg), c_int, P, P, c_int, c_int, c_int, P, c_size_t, P]),
    'mvae_bce_multi_bwd': (c_int, [ctypes.POINTER(BceSeg), c_int, P, c_int, c_int, c_int, P]),
    # K23: the six modalities of the vision step from raw uint8 sources in one launch
    'mvae_vision_compose': (c_int, [P] * 11 + [c_int] * 8 + [P, P, c_int, P, P, c_int, c_int, c_int, P]),
    # K24: the per-modality and joint importance-weighted estimates from one decoder pass
    'mvae_iw_score_multi_ws_bytes': (c_size_t, [ctypes.POINTER(BceSeg), c_int, c_int]),
    'mvae_iw_score_multi': (c_int, [ctypes.POINTER(BceSeg), c_int, P, P, P, c_int, c_int, c_int, P, c_size_t, P]),
    # K25: G one-logit heads fused with their Bernoulli term, and the fold of up to IW_FOLD_MAX existing row sums
    'mvae_heads_bce_rows': (c_int, [P, c_int, c_size_t, P, c_size_t, P, c_size_t, P, c_int, c_int, P, c_size_t, P,
                                    c_size_t, c_int, c_int, c_int, P]),
    'mvae_iw_fold_rows': (c_int, [P, c_size_t, ctypes.POINTER(c_int), c_int, P, P, P, c_int, c_int, c_int, P]),
    # K26: Canny edges of a uint8 batch (float stage + hysteresis), the edge step of vision/setup.py
    'mvae_canny_supported': (c_int, [c_int, c_int, c_float]),
    'mvae_canny_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'mvae_canny': (c_int, [P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, P, P, P, P, c_size_t, P]),
    'mvae_canny_hysteresis': (c_int, [P, P, c_int, c_int, c_int, P]),
    # K27: the PoE of condition rows that each select their experts from a table, with n draws per row
    'mvae_poe_table_draw': (c_int, [P, c_int, P, P, c_int, c_int, P, P, c_uint64, P, c_uint64, P, P, P, P, c_int, c_int,
                                    c_int, P]),
    # K28: label prediction (the fold of one state per (datum, class), and the scoring against labels)
    'mvae_predict_fold': (c_int, [P, ctypes.c_longlong, ctypes.c_longlong, c_int, c_int, c_int, c_int, P, P, c_int, P]),
    'mvae_predict_score': (c_int, [P, c_int, P, c_int, c_int, c_int, P, P, P, P, P]),
    # K29: the PoE of a batch whose rows observe different modalities (compact experts and outputs behind index tables)
    'mvae_poe_ragged_fwd': (c_int, [ctypes.POINTER(Experts), c_int, c_int, ctypes.POINTER(c_int), P, P, c_int, P, c_int,
                                    P, c_int, c_uint64, P, c_uint64, P, P, P, P, c_int, c_int, c_int, P]),
    'mvae_poe_ragged_bwd': (c_int, [ctypes.POINTER(Experts), c_int, c_int, ctypes.POINTER(c_int), P, P, c_int, P, c_int,
                                    P, P, P, P, P, P, P, ctypes.POINTER(ExpertGrads), c_int, c_int, c_int, c_int, P]),
    # K30: BCE / CE row sums of compact logits rows that find their target through a row map
    'mvae_bce_rows_indexed_fwd': (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, P]),
    'mvae_bce_rows_indexed_bwd': (c_int, [P, P, P, P, P, c_int, c_int, c_int, P]),
    'mvae_ce_rows_indexed_fwd': (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, P]),
    'mvae_ce_rows_indexed_bwd': (c_int, [P, P, P, P, P, c_int, c_int, c_int, P]),
    # C1: the gradient exchange (RCCL bound at run time)
    'mvae_comm_use_library': (c_int, [ctypes.c_char_p]),
    'mvae_comm_rccl_version': (c_int, []),
    'mvae_comm_unique_id': (c_int, [P, c_size_t]),
    'mvae_comm_init': (c_int, [ctypes.POINTER(P), P, c_size_t, c_int, c_int, c_int]),
    'mvae_comm_rank': (c_int, [P]),
    'mvae_comm_world': (c_int, [P]),
    'mvae_comm_last_error': (ctypes.c_char_p, [P]),
    'mvae_comm_broadcast': (c_int, [P, P, c_size_t, c_int, P]),
    'mvae_comm_allreduce_async': (c_int, [P, P, c_size_t, P, ctypes.POINTER(c_int)]),
    'mvae_comm_wait': (c_int, [P, c_int, P]),
    'mvae_comm_async_error': (c_int, [P]),
    'mvae_comm_synchronize': (c_int, [P, P, c_int]),
    'mvae_comm_destroy': (c_int, [P]),
}

# tuning overrides: only exported by libmvae_hip_tuning.so (csrc built with -DMVAE_TUNING); bound when
# MVAE_HIP_LIB points the loader at that build (tools/gemm_bench.py, bench.py --force-tiling)
_TUNING_SIGNATURES = {
    'mvae_debug_set_tiling': (None, [c_int, c_int, c_int]),
    'mvae_debug_set_kwaves': (None, [c_int]),
    'mvae_debug_set_small': (None, [c_int, c_int]),
    'mvae_debug_set_split_target': (None, [ctypes.c_long]),
    'mvae_debug_set_knockout': (None, [c_int]),
}
TUNING_LIB_PATH = os.path.join(_HERE, 'libmvae_hip_tuning.so')

_lib = None


def exported_symbols():
    """Names include/mvae_hip.h declares (the not-gpu tests check the .so exports each)."""
    return sorted(_SIGNATURES)


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get('MVAE_HIP_LIB') or LIB_PATH     # an alternative BUILD of the same library
        if not os.path.exists(path):
            raise RuntimeError(
                'libmvae_hip.so is not built (%s missing): run `make -C %s/csrc`; there is no '
                'CPU fallback for the MVAE HIP path.' % (path, _HERE))
        handle = ctypes.CDLL(path)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)   # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in _TUNING_SIGNATURES.items():
            fn = getattr(handle, name, None)
            if fn is not None:
                fn.restype = res
                fn.argtypes = args
        if handle.mvae_abi_version() != 6:
            raise RuntimeError('libmvae_hip.so ABI version mismatch')
        _lib = handle
    return _lib


def check(rc, what):
    if rc != MVAE_OK:
        raise RuntimeError('%s failed: %s' % (what, ERRORS.get(rc, 'error %d' % rc)))
