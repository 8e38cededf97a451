"""ctypes binding of libbnerv_hip.so (include/bnerv.h).  The HIP extension is the ONLY compute path of this package:
if the shared object is missing or a call fails, we raise -- there is no CPU / eager fallback."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BNERV_LIB") or os.path.join(_HERE, "libbnerv_hip.so")     # BNERV_LIB: another build of the same ABI (debug / trace variants)

MAX_DENSE_GROUPS = 40
ADAN_MAX_TENSORS = 48
SFT_CHUNKS = 32
LOSS_STATS = 5
DENSE_DX_CHUNK = 64

ACT_NONE, ACT_RELU, ACT_SIN = 0, 1, 2
IN_PLAIN, IN_AFFINE, IN_GELU_AFFINE, IN_UNSHUFFLE, IN_TANHGRAD = 0, 1, 2, 3, 4
EP_BIAS, EP_BIAS_SIN, EP_BIAS_RES, EP_BIAS_TANH, EP_PLAIN, EP_DGELU, EP_DSIN, EP_BIAS_GELU, EP_DGELU_SAVED = 0, 1, 2, 3, 4, 5, 6, 7, 8
# kernel families / pair forms reported by bnerv_conv_family, bnerv_conv_wgrad_family, bnerv_conv_wgrad_pair_form (BNERV_CONV_FAM_* ...)
CONV_FAM = ("head1_fwd", "head1_dgrad", "head3", "stem_dgrad", "small", "small96", "wide_bf16", "q4", "generic")
WGRAD_FAM = ("stem", "gemm1x1", "lean", "wide_bf16", "wide_f32", "generic")
PAIR_FORM = ("stem", "q4_lean", "small_wide", "bf16_wide", "head")      # -1: none

_fp = C.c_void_p     # device pointers travel as void* (data_ptr())


class DenseFwdDesc(C.Structure):
    _fields_ = [("x", _fp), ("w", _fp), ("b", _fp), ("y", _fp), ("aux", _fp),
                ("I", C.c_int), ("O", C.c_int), ("act", C.c_int), ("_pad", C.c_int)]


class DenseBwdDesc(C.Structure):
    _fields_ = [("x", _fp), ("w", _fp), ("y", _fp), ("aux", _fp), ("dy", _fp), ("dpre", _fp), ("dw", _fp), ("db", _fp),
                ("dx_part", _fp), ("I", C.c_int), ("O", C.c_int), ("act", C.c_int), ("_pad", C.c_int)]


class ConvDesc(C.Structure):
    _fields_ = [("x", _fp), ("w", _fp), ("bias", _fp), ("out", _fp), ("out2", _fp), ("aux0", _fp), ("aux1", _fp),
                ("aux2", _fp), ("scale", _fp), ("shift", _fp), ("partial", _fp),
                ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("H", C.c_int), ("W", C.c_int), ("k", C.c_int),
                ("in_mode", C.c_int), ("ep_mode", C.c_int), ("in_s", C.c_int), ("out_s", C.c_int),
                ("transposed", C.c_int), ("wCo", C.c_int), ("wCi", C.c_int), ("ctx", _fp)]


class TimeBranchMlp(C.Structure):
    _fields_ = [("w1", _fp), ("b1", _fp), ("w2", _fp), ("b2", _fp), ("hs", _fp), ("out", _fp), ("C", C.c_int), ("_pad", C.c_int)]


class TimeBranchDesc(C.Structure):
    _fields_ = [("pos", _fp), ("bases", _fp), ("pe", _fp), ("sw0", _fp), ("sb0", _fp), ("sy0", _fp), ("saux0", _fp),
                ("tw0", _fp), ("tb0", _fp), ("tw1", _fp), ("tb1", _fp), ("ty0", _fp), ("taux0", _fp), ("ty1", _fp), ("taux1", _fp),
                ("B", C.c_int), ("L", C.c_int), ("SH", C.c_int), ("TH", C.c_int), ("TO", C.c_int), ("n_mlp", C.c_int)]


class TimeBranchBwdMlp(C.Structure):
    _fields_ = [("w1", _fp), ("w2", _fp), ("hs", _fp), ("d_out", _fp), ("dw1", _fp), ("db1", _fp), ("dw2", _fp), ("db2", _fp),
                ("C", C.c_int), ("_pad", C.c_int)]


class TimeBranchBwdDesc(C.Structure):
    _fields_ = [("pe", _fp), ("sw1", _fp), ("sy0", _fp), ("saux0", _fp), ("saux1", _fp), ("d_sy1", _fp),
                ("tw1", _fp), ("ty0", _fp), ("taux0", _fp), ("ty1", _fp), ("taux1", _fp), ("d_ty1", _fp),
                ("d_sw0", _fp), ("d_sb0", _fp), ("d_sw1", _fp), ("d_sb1", _fp), ("d_tw0", _fp), ("d_tb0", _fp), ("d_tw1", _fp), ("d_tb1", _fp),
                ("sx_part", _fp), ("zt_part", _fp), ("s_dpre", _fp),
                ("B", C.c_int), ("L", C.c_int), ("SH", C.c_int), ("SO", C.c_int), ("TH", C.c_int), ("TO", C.c_int), ("n_mlp", C.c_int), ("_pad", C.c_int)]


TIME_BRANCH_BWD_MLP_BYTES, TIME_BRANCH_BWD_DESC_BYTES = 72, 216      # include/bnerv.h: BNERV_TIME_BRANCH_BWD_*_BYTES


class WgradDesc(C.Structure):
    _fields_ = [("x", _fp), ("g", _fp), ("gaux", _fp), ("scale", _fp), ("shift", _fp), ("dw", _fp), ("db", _fp),
                ("ws", _fp), ("ws_bytes", C.c_size_t),
                ("B", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("H", C.c_int), ("W", C.c_int), ("k", C.c_int),
                ("in_mode", C.c_int), ("g_mode", C.c_int), ("g_s", C.c_int), ("defer_finish", C.c_int), ("ctx", _fp)]


class LossDesc(C.Structure):
    _fields_ = [("pred", _fp), ("target", _fp), ("grad", _fp), ("loss_out", _fp), ("stats_out", _fp), ("ws", _fp),
                ("ws_bytes", C.c_size_t), ("B", C.c_int), ("C", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("c_l1", C.c_float), ("c_l2", C.c_float), ("c_ms", C.c_float), ("c_fft", C.c_float)]


class AdanChunk(C.Structure):
    _fields_ = [("p", _fp * ADAN_MAX_TENSORS), ("g", _fp * ADAN_MAX_TENSORS), ("exp_avg", _fp * ADAN_MAX_TENSORS),
                ("exp_avg_sq", _fp * ADAN_MAX_TENSORS), ("exp_avg_diff", _fp * ADAN_MAX_TENSORS),
                ("neg_pre_grad", _fp * ADAN_MAX_TENSORS), ("n", C.c_int * ADAN_MAX_TENSORS), ("n_tensors", C.c_int)]


class AdanHyper(C.Structure):
    _fields_ = [("beta1", C.c_float), ("beta2", C.c_float), ("beta3", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("clip_global_grad_norm", C.c_float), ("no_prox", C.c_int),
                ("sched_dev", _fp)]


class AdanEntry(C.Structure):
    _fields_ = [("p", _fp), ("g", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp), ("exp_avg_diff", _fp), ("neg_pre_grad", _fp),
                ("n", C.c_int), ("bstart", C.c_int)]


class BucketChunk(C.Structure):
    _fields_ = [("t", _fp * (ADAN_MAX_TENSORS * 2)), ("n", C.c_int * (ADAN_MAX_TENSORS * 2)),
                ("off", C.c_int * (ADAN_MAX_TENSORS * 2)), ("n_tensors", C.c_int)]


CEM_MAX_TENSORS = 48


class CemItem(C.Structure):
    _fields_ = [("w", _fp), ("scale", _fp), ("noise", _fp), ("dequant", _fp), ("n", C.c_int), ("_pad", C.c_int)]


class CemChunk(C.Structure):
    _fields_ = [("it", CemItem * CEM_MAX_TENSORS), ("n_items", C.c_int), ("training", C.c_int), ("first", C.c_int), ("_pad", C.c_int)]


class CemItemBwd(C.Structure):
    _fields_ = [("w", _fp), ("scale", _fp), ("noise", _fp), ("d_dequant", _fp), ("dw", _fp), ("n", C.c_int), ("_pad", C.c_int)]


class CemChunkBwd(C.Structure):
    _fields_ = [("it", CemItemBwd * CEM_MAX_TENSORS), ("n_items", C.c_int), ("training", C.c_int), ("first", C.c_int), ("_pad", C.c_int)]


DEQUANT_CHUNK = 8192      # BNERV_DEQUANT_CHUNK


class DequantItem(C.Structure):
    _fields_ = [("q", _fp), ("out", _fp), ("scale", _fp), ("beta", _fp), ("n", C.c_int), ("_pad", C.c_int)]


class DequantChunk(C.Structure):
    _fields_ = [("it", DequantItem * CEM_MAX_TENSORS), ("n_items", C.c_int), ("_pad", C.c_int)]


HUFF_RUN, HUFF_LEAVES, HUFF_LUT_BITS = 256, 257, 12      # BNERV_HUFF_RUN, BNERV_HUFF_LEAVES, BNERV_HUFF_LUT_BITS
HUFF_F32, HUFF_F16 = 0, 1
HUFFZ_LEAVES, HUFFZ_ZERO, HUFFZ_ZERO_LEAVES = 266, 256, 9      # BNERV_HUFFZ_LEAVES, BNERV_HUFFZ_ZERO, BNERV_HUFFZ_ZERO_LEAVES
HUFFZ_SINGLE, HUFFZ_RUNS = 0, 1                                # BNERV_HUFFZ_SINGLE, BNERV_HUFFZ_RUNS


class HuffRun(C.Structure):        # bnerv_huff_run
    _fields_ = [("start_bit", C.c_uint64), ("item", C.c_uint32), ("first", C.c_uint32)]


class HuffItem(C.Structure):       # bnerv_huff_item
    _fields_ = [("out", _fp), ("min", _fp), ("scale", _fp), ("dtype", C.c_int), ("n", C.c_uint32), ("red", C.c_uint32), ("inner", C.c_uint32)]


class HuffItemU8(C.Structure):     # bnerv_huff_item_u8
    _fields_ = [("out", C.c_void_p), ("n", C.c_uint32)]


RANS_MAX_ALPHABET, RANS_MIN_RUN, RANS_MAX_RUN = 4096, 64, 4096     # BNERV_RANS_MAX_ALPHABET, BNERV_RANS_MIN_RUN, BNERV_RANS_MAX_RUN


class RansBlock(C.Structure):      # bnerv_rans_block
    _fields_ = [("item", C.c_uint32), ("run", C.c_uint32), ("first", C.c_uint32), ("_pad", C.c_uint32)]


class RansItem(C.Structure):       # bnerv_rans_item
    _fields_ = [("out", _fp), ("scale", C.c_float), ("beta", C.c_float), ("lo", C.c_int), ("n", C.c_uint32), ("table", C.c_uint32), ("alphabet", C.c_uint32),
                ("has_beta", C.c_int), ("_pad", C.c_int)]


HIST_SLICE = 16384      # BNERV_HIST_SLICE


class HistItem(C.Structure):       # bnerv_hist_item
    _fields_ = [("sym", _fp), ("n", C.c_uint32), ("lo", C.c_int), ("alphabet", C.c_uint32), ("out", C.c_uint32)]


class RencItem(C.Structure):       # bnerv_renc_item
    _fields_ = [("sym", _fp), ("n", C.c_uint32), ("lo", C.c_int), ("alphabet", C.c_uint32), ("table", C.c_uint32)]


class RansCopy(C.Structure):       # bnerv_rans_copy
    _fields_ = [("slot", C.c_uint32), ("dst", C.c_uint32), ("count", C.c_uint32), ("_pad", C.c_uint32)]


RANSW_MAX_SHIFT = 16    # BNERV_RANSW_MAX_SHIFT


class WsymItem(C.Structure):       # bnerv_wsym_item
    _fields_ = [("sym", _fp), ("n", C.c_uint32), ("lo", C.c_int), ("alphabet", C.c_uint32), ("at", C.c_uint32), ("shift", C.c_uint32), ("span_m1", C.c_uint32)]


class RanswItem(C.Structure):      # bnerv_ransw_item
    _fields_ = [("out", _fp), ("scale", C.c_float), ("beta", C.c_float), ("lo", C.c_int), ("n", C.c_uint32), ("table", C.c_uint32), ("alphabet", C.c_uint32),
                ("has_beta", C.c_int), ("shift", C.c_uint32), ("span_m1", C.c_uint32), ("_pad", C.c_uint32)]


CHAIN_UNROLL, CHAIN_SEG = 8, 64    # BNERV_CHAIN_UNROLL, BNERV_CHAIN_SEG


class DeltaStats(C.Structure):     # bnerv_delta_stats
    _fields_ = [("max_key", C.c_uint32), ("min_key_inv", C.c_uint32), ("s1", C.c_int64), ("s2", C.c_uint64)]


PRUNE_SLICE = 16384     # BNERV_PRUNE_SLICE


class PruneItem(C.Structure):      # bnerv_prune_item
    _fields_ = [("x", _fp), ("mask", _fp), ("n", C.c_uint32), ("_pad", C.c_uint32)]


class YuvCoeffs(C.Structure):      # bnerv_yuv_coeffs: what yuvio.coefficients() computed in float64, rounded to fp32
    _fields_ = [("m", C.c_float * 9), ("off", C.c_float * 3), ("scale", C.c_float * 3), ("maxcode", C.c_float)]


# every symbol include/bnerv.h declares: name -> (restype, argtypes)
_I, _Z, _V, _F = C.c_int, C.c_size_t, C.c_void_p, C.c_float
SYMBOLS = {
    "bnerv_abi_version": (_I, []),
    "bnerv_last_error": (C.c_char_p, []),
    "bnerv_build_arch": (C.c_char_p, []),
    "bnerv_pe_fwd_f32": (_I, [_V, _V, _V, _V, _I, _I]),
    "bnerv_pe_fwd_f64": (_I, [_V, _V, _V, _V, _I, _I]),
    "bnerv_pe_fwd_f32_from_f64": (_I, [_V, _V, _V, _V, _I, _I]),
    "bnerv_dense_grouped_fwd": (_I, [_V, C.POINTER(DenseFwdDesc), _I, _I]),
    "bnerv_time_branch_fwd": (_I, [_V, C.POINTER(TimeBranchDesc), C.POINTER(TimeBranchMlp)]),
    "bnerv_time_branch_bwd": (_I, [_V, C.POINTER(TimeBranchBwdDesc), C.POINTER(TimeBranchBwdMlp)]),
    "bnerv_dense_grouped_bwd": (_I, [_V, C.POINTER(DenseBwdDesc), _I, _I]),
    "bnerv_sft_affine_fwd": (_I, [_V, _V, _V, _V, _V, _I, _I, _I]),
    "bnerv_sft_affine_bwd": (_I, [_V, _V, _V, _V, _V, _V, _I, _I, _I]),
    "bnerv_reduce_slabs": (_I, [_V, _V, _I, _I, _V]),
    "bnerv_ctx_create": (_I, [C.POINTER(C.c_void_p)]),
    "bnerv_ctx_destroy": (None, [_V]),
    "bnerv_ctx_scratch_bytes": (_Z, [_V]),
    "bnerv_ctx_reserve": (_I, [_V, _Z]),
    "bnerv_ctx_wplan_record": (_I, [_V]),
    "bnerv_ctx_wplan_freeze": (_I, [_V]),
    "bnerv_ctx_wplan_run": (_I, [_V, _V]),
    "bnerv_ctx_wplan_run_fetch": (_I, [_V, _V, _V, _V, _V, _I, _Z, _V, _V]),
    "bnerv_ctx_wplan_end": (_I, [_V]),
    "bnerv_ctx_wplan_entries": (_I, [_V]),
    "bnerv_reduce_slabs_deferred": (_I, [_V, _V, _V, _I, _I, _V]),
    "bnerv_flush_deferred": (_I, [_V, _V]),
    "bnerv_deferred_pending": (_I, [_V]),
    "bnerv_conv_tiles": (_I, [_I, _I]),
    "bnerv_conv_igemm": (_I, [_V, C.POINTER(ConvDesc)]),
    "bnerv_conv_splitk_ws_bytes": (_Z, [C.POINTER(ConvDesc)]),
    "bnerv_conv_partial_rows": (_I, [C.POINTER(ConvDesc)]),
    "bnerv_conv_family": (_I, [C.POINTER(ConvDesc), C.POINTER(C.c_int)]),
    "bnerv_conv_wgrad_ws_bytes": (_Z, [_I, _I, _I, _I, _I, _I]),
    "bnerv_conv_wgrad_pair": (_I, [_V, C.POINTER(ConvDesc), C.POINTER(WgradDesc)]),
    "bnerv_conv_wgrad_pair_form": (_I, [C.POINTER(ConvDesc), C.POINTER(WgradDesc), C.POINTER(C.c_int)]),
    "bnerv_conv_wgrad": (_I, [_V, C.POINTER(WgradDesc)]),
    "bnerv_conv_wgrad_family": (_I, [C.POINTER(WgradDesc), C.POINTER(C.c_int)]),
    "bnerv_conv5_ws_bytes": (_Z, [_I, _I]),
    "bnerv_conv5_igemm": (_I, [_V, C.POINTER(ConvDesc), _V, _Z]),
    "bnerv_conv5_wgrad_ws_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "bnerv_conv5_wgrad": (_I, [_V, C.POINTER(WgradDesc)]),
    "bnerv_gelu_fwd": (_I, [_V, _V, _V, _V, _Z]),
    "bnerv_mul": (_I, [_V, _V, _V, _V, _Z]),
    "bnerv_cem_ws_bytes": (_Z, [_I, _I]),
    "bnerv_cem_scale_fwd": (_I, [_V, C.POINTER(CemChunk), _V, _V, _Z]),
    "bnerv_cem_scale_bwd": (_I, [_V, C.POINTER(CemChunkBwd), _V, _V, _V, _V, _Z]),
    "bnerv_dequant_table": (_I, [_V, C.POINTER(DequantChunk)]),
    "bnerv_frame_to_u8": (_I, [_V, _V, _V, _I, _I, _I]),
    "bnerv_yuv420_to_rgb": (_I, [_V, _V, _I, _I, _Z, _I, _I, _I, _I, _V, _I, _I, C.POINTER(YuvCoeffs)]),
    "bnerv_rgb_to_yuv420": (_I, [_V, _V, _I, _I, _I, _V, _I, _Z, C.POINTER(YuvCoeffs)]),
    "bnerv_yuv420_sse": (_I, [_V, _V, _Z, _V, _Z, _I, _I, _I, _I, _I, _I, _I, _I, _V]),
    "bnerv_yuv_luma_f32": (_I, [_V, _V, _I, _I, _Z, _I, _I, _I, _I, _V, _I, _I, _F]),
    "bnerv_yuv420_loss_ws_bytes": (_Z, [_I, _I, _I]),
    "bnerv_yuv420_loss": (_I, [_V, _V, _I, _I, _I, _V, _I, _Z, _I, _I, _I, _I, _I, _V, C.POINTER(YuvCoeffs), C.POINTER(C.c_float), _F, _V, _I, _V,
                               _V, _V, _Z]),
    "bnerv_yuv_luma_pair": (_I, [_V, _V, _I, _I, _I, _V, _I, _Z, _I, _I, _I, _I, _I, _V, C.POINTER(YuvCoeffs), _V, _V]),
    "bnerv_luma_grad_rgb": (_I, [_V, _V, _I, _I, _I, C.POINTER(C.c_double), _F, _V, _I, _V, _V]),
    "bnerv_dense_gemm_fwd": (_I, [_V, _V, _V, _V, _V, _V, _I, _I, _I, _I]),
    "bnerv_dense_gemm_bwd_ws_bytes": (_Z, [_I, _I, _I]),
    "bnerv_dense_gemm_bwd": (_I, [_V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _Z, _I, _I, _I, _I]),
    "bnerv_cnx_mlp_fwd": (_I, [_V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _I, _I, _I]),
    "bnerv_cnx_mlp_bwd": (_I, [_V, _V, _V, _V, _V, _V, _V, _V, _V, _I, _I, _I]),
    "bnerv_cnx_mlp_plan": (_I, [_I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "bnerv_cnx_param_grads": (_I, [_V, _V, _V, _V, _V, _V, _V, _V, _V, _I]),
    "bnerv_ans_encode_gaussian": (C.c_long, [_V, _Z, _I, _I, C.c_double, C.c_double, _V, _Z]),
    "bnerv_ans_decode_gaussian": (_I, [_V, _Z, _Z, _I, _I, C.c_double, C.c_double, _V]),
    "bnerv_ans_encode_categorical": (C.c_long, [_V, _Z, _V, _I, _V, _Z]),
    "bnerv_ans_decode_categorical": (_I, [_V, _Z, _Z, _V, _I, _V]),
    "bnerv_ans_gaussian_cdf": (C.c_long, [_I, _I, C.c_double, C.c_double, _V, _Z]),
    "bnerv_ans_encode_gaussian_runs": (C.c_long, [_V, _Z, _I, _I, C.c_double, C.c_double, _I, _V, _Z, _V]),
    "bnerv_ans_decode_gaussian_runs": (_I, [_V, _Z, _V, _Z, _Z, _I, _I, C.c_double, C.c_double, _I, _V]),
    "bnerv_rans_dequant": (_I, [_V, _V, _Z, _V, _Z, _V, _Z, _V, _I, _V, _Z, _I, _V]),
    "bnerv_ans_counts_cdf": (C.c_long, [_V, _I, _V, _Z]),
    "bnerv_ans_encode_table_runs": (C.c_long, [_V, _Z, _I, _V, _I, _I, _V, _Z, _V]),
    "bnerv_ans_decode_table_runs": (_I, [_V, _Z, _V, _Z, _Z, _I, _V, _I, _I, _V]),
    "bnerv_sym_hist": (_I, [_V, _V, _I, _V, _Z, _V, _Z, _V]),
    "bnerv_rans_encode": (_I, [_V, _V, _Z, _V, _I, _V, _Z, _I, _V, _Z, _V, _V]),
    "bnerv_rans_compact": (_I, [_V, _V, _Z, _I, _V, _Z, _V, _Z, _V]),
    "bnerv_ans_gaussian_bucket_cdf": (C.c_long, [_I, _I, _I, C.c_double, C.c_double, _V, _Z]),
    "bnerv_ans_encode_wide_runs": (C.c_long, [_V, _Z, _I, _I, _V, _I, _I, _I, _V, _Z, _V]),
    "bnerv_ans_decode_wide_runs": (_I, [_V, _Z, _V, _Z, _Z, _I, _I, _V, _I, _I, _I, _V]),
    "bnerv_sym_hist_wide": (_I, [_V, _V, _I, _V, _Z, _V, _Z, _V]),
    "bnerv_rans_encode_wide": (_I, [_V, _V, _Z, _V, _I, _V, _Z, _I, _V, _Z, _I, _V, _V]),
    "bnerv_rans_dequant_wide": (_I, [_V, _V, _Z, _V, _Z, _V, _Z, _V, _I, _V, _Z, _I, _V]),
    "bnerv_embed_delta": (_I, [_V, _V, _Z, _I, _Z, _V, _Z, _V]),
    "bnerv_rans_decode_wide": (_I, [_V, _V, _Z, _V, _Z, _V, _Z, _V, _I, _V, _Z, _I, _V]),
    "bnerv_embed_chain_dequant": (_I, [_V, _V, _Z, _V, _V, _V, _I, _Z, _V, _Z, _V]),
    "bnerv_embed_delta_u8": (_I, [_V, _V, _Z, _I, _Z, _V, _Z, _V]),
    "bnerv_huff_decode_u8": (_I, [_V, _V, _Z, _V, _Z, _V, _I, _V, _I, _V]),
    "bnerv_embed_chain_dequant_u8": (_I, [_V, _V, _Z, _V, _V, _V, _I, C.c_uint32, C.c_uint32, _I, _Z, _V, _Z]),
    "bnerv_huff_encode": (C.c_long, [_V, _V, _I, _V, _I, _V, _Z, _V, _Z]),
    "bnerv_huff_decode": (_I, [_V, _Z, _V, _Z, _V, _I, _V, _I, _V]),
    "bnerv_huff_dequant": (_I, [_V, _V, _Z, _V, _Z, _V, _I, _V, _I, _V]),
    "bnerv_huffz_encode": (C.c_long, [_V, _V, _V, _I, _V, _I, _I, _V, _Z, _V, _Z]),
    "bnerv_huffz_decode": (_I, [_V, _Z, _V, _Z, _V, _I, _V, _I, _V, _V]),
    "bnerv_huffz_dequant": (_I, [_V, _V, _Z, _V, _Z, _V, _I, _V, _I, _V]),
    "bnerv_dwconv_fwd": (_I, [_V, _V, _V, _V, _V, _I, _I, _I, _I, _I, _I]),
    "bnerv_dwconv_wgrad_ws_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "bnerv_dwconv_wgrad": (_I, [_V, _V, _V, _V, _V, _Z, _I, _I, _I, _I, _I, _V]),
    "bnerv_dwconv_wgrad_plan": (_I, [_I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "bnerv_lncf_fwd": (_I, [_V, _V, _V, _V, _V, _I, _I, _I, _F]),
    "bnerv_lncf_bwd_ws_bytes": (_Z, [_I, _I, _I]),
    "bnerv_lncf_bwd": (_I, [_V, _V, _V, _V, _V, _V, _V, _Z, _I, _I, _I, _F]),
    "bnerv_loss_ws_bytes": (_Z, [_I, _I, _I, _I, _I, _I]),
    "bnerv_fft_prepare": (_I, [_I, _I]),
    "bnerv_loss_fwd_bwd": (_I, [_V, C.POINTER(LossDesc)]),
    "bnerv_msssim": (_I, [_V, _V, _V, _V, _V, _Z, _I, _I, _I, _I]),
    "bnerv_loss_ssim_ws_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "bnerv_loss_ssim_prepare": (_I, [_I, _I]),
    "bnerv_loss_ssim_fwd_bwd": (_I, [_V, C.POINTER(LossDesc), _F]),
    "bnerv_ssim": (_I, [_V, _V, _V, _V, _V, _Z, _I, _I, _I, _I]),
    "bnerv_tanh_grad_blocks": (_I, [_I]),
    "bnerv_tanh_grad": (_I, [_V, _V, _V, _V, _V, _I, _I, _I]),
    "bnerv_inpaint_head": (_I, [_V, _V, _V, _V, _V, _I, _I, _I]),
    "bnerv_inpaint_ws_bytes": (_Z, [_I, _I, _I]),
    "bnerv_inpaint_pred": (_I, [_V, _V, _V, _V, _V, _V, _Z, _I, _I, _I]),
    "bnerv_inpaint_psnr": (_I, [_V, _V, _Z, _V, _I, _I, _I, _I]),
    "bnerv_inpaint_grad": (_I, [_V, _V, _V, _I, _I, _I]),
    "bnerv_psnr_ws_bytes": (_Z, [_I, _I, _I, _I]),
    "bnerv_psnr": (_I, [_V, _V, _V, _V, _V, _Z, _I, _I, _I, _I]),
    "bnerv_adan_multi_tensor": (_I, [_V, C.POINTER(AdanChunk), C.POINTER(AdanHyper)]),
    "bnerv_adan_table_blocks": (_I, [_I]),
    "bnerv_adan_table": (_I, [_V, _V, _I, _I, C.POINTER(AdanHyper)]),
    "bnerv_adam_table_blocks": (_I, [_I]),
    "bnerv_adam_table": (_I, [_V, _V, _I, _I, C.POINTER(AdanHyper)]),
    "bnerv_grad_sqsum_table": (_I, [_V, _V, _I, _I, _V]),
    "bnerv_grad_scale_table": (_I, [_V, _V, _I, _I, _V, _I, _F, _V]),
    "bnerv_fetch_frame": (_I, [_V, _V, _V, _V, _I, _Z, _V, _V]),
    "bnerv_bucket_gather": (_I, [_V, C.POINTER(BucketChunk), _V, _F]),
    "bnerv_bucket_scatter": (_I, [_V, C.POINTER(BucketChunk), _V, _F]),
    "bnerv_kth_abs": (_I, [_V, _V, _V, _I, _V, _Z, C.c_ulonglong, _V]),
    "bnerv_prune_masks": (_I, [_V, _V, _I, _V, _Z, _V]),
    "bnerv_mask_mul": (_I, [_V, _V, _I, _V, _Z]),
    "bnerv_grad_mask_table": (_I, [_V, _V, _I, _I, _V]),
    "bnerv_embed_expand": (_I, [_V, _V, _V, _V, _I, _I, _I]),
    "bnerv_resize_rows": (_I, [_V, _V, _V, _V, C.c_longlong, _I, _I, _I, _I]),
    "bnerv_resize_cols": (_I, [_V, _V, _V, _V, _I, _I, _I, _I, _I, _I]),
    "bnerv_resize_cols_yuv420": (_I, [_V, _V, _V, _I, _I, _I, _I, _I, _V, _I, _Z, C.POINTER(YuvCoeffs)]),
    "bnerv_yuv420_up_loss_ws_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "bnerv_yuv420_up_loss_fwd": (_I, [_V, _V, _I, _I, _I, _I, _I, _V, _I, _I, _V, _I, _V, _I, _Z, _I, _I, _I, _I, _I, _V, C.POINTER(YuvCoeffs),
                                      C.POINTER(C.c_float), _F, _I, _I, _V, _V, _V, _Z]),
    "bnerv_yuv420_up_loss_bwd": (_I, [_V, _I, _I, _I, _I, _I, _V, _I, _V, _I, _I, C.POINTER(YuvCoeffs), _F, _V, _I, _V, _Z]),
}

_lib = None
ABI_VERSION = 9


class BnervError(RuntimeError):
    pass


def load(optional=()):
    """Load the shared object (once) and bind every symbol.  Raises if the library is missing: the HIP path is the
    product, there is nothing to fall back to.  `optional`: names that an OLDER build of the same ABI may lack (additive entry
    points); they are left unbound there instead of failing the load -- for tools that compare two builds, first call only."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise BnervError(f"{LIB_PATH} not found -- build it with boosting_nerv_amd/csrc/build.sh "
                         f"(or `python -c 'import __graft_entry__ as g; g.build()'`)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        if name in optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)          # AttributeError here = header and library out of sync
        fn.restype = res
        fn.argtypes = args
    if lib.bnerv_abi_version() != ABI_VERSION:
        raise BnervError(f"ABI version mismatch: {lib.bnerv_abi_version()}")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().bnerv_last_error().decode("utf-8", "replace")
        raise BnervError(f"{what} failed (rc={rc}): {msg}")


def require_device(t, name="tensor"):
    """The decoder path runs only on a ROCm device; fail loudly rather than silently computing elsewhere."""
    if not t.is_cuda:
        raise BnervError(f"{name} is on {t.device}: the bnerv HIP path needs a ROCm GPU tensor (no CPU fallback exists)")
    return t


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def graph_capture(graph, **kw):
    """torch.cuda.graph(graph, ...) with the capture in THREAD-LOCAL error mode, after quiesce_collectives().

    torch.distributed's ProcessGroupNCCL keeps a watchdog thread that polls the end event of every EAGER collective with
    hipEventQuery until it has seen it complete (every 100 ms; torch.cuda.synchronize() does not retire the work item, the next poll
    does).  Two HIP rules turn that poll into a process abort (the watchdog rethrows on its own thread -> std::terminate -> SIGABRT;
    this was the round-4 abort of the GPU suite, DESIGN section 12.1, reproduced at will by tools/repro_watchdog_capture.py):
      (1) while ANY thread captures in torch's default GLOBAL mode, hipEventQuery from another thread on an event recorded on a
          non-default stream fails with hipErrorStreamCaptureUnsupported; in thread-local mode only the capturing thread is policed.
          This package's captures issue kernel launches, event record / wait edges and async copies on streams of their own -- the
          cross-thread policing protects nothing here, so every capture of the package goes through this helper;
      (2) in ANY mode, querying an event whose last record was on a stream that is capturing NOW fails (hipErrorCapturedEvent): a stream
          that hosted an eager collective must never be captured while that collective's work item may be alive -- dp.GradBucket keeps
          separate side streams for its eager and its captured exchange for this reason."""
    kw.setdefault("capture_error_mode", "thread_local")
    quiesce_collectives()
    return torch.cuda.graph(graph, **kw)


_WATCHDOG_POLL_S = 0.1      # ProcessGroupNCCL's kWatchdogThreadSleepMillis


def quiesce_collectives():
    """Before a stream capture in a process that has an NCCL(=RCCL) process group: let the watchdog retire every eager work item.
    There is no API that waits for the watchdog; after a device synchronisation every work item is complete, and two and a half poll
    periods later the watchdog has seen that.  Belt to graph_capture's braces (either alone survives the reproducer); costs 0.25 s per
    capture, nothing per step, nothing at all without a process group."""
    import time
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    try:
        if "nccl" not in str(dist.get_backend()):
            return
    except Exception:       # noqa: BLE001
        return
    if torch.cuda.is_current_stream_capturing():
        return
    torch.cuda.synchronize()
    time.sleep(2.5 * _WATCHDOG_POLL_S)


def f32c(t):
    """contiguous fp32 view/copy (plumbing: kernels require dense NCHW fp32)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


class StreamContext:
    """The deferred-reduction context (include/bnerv.h, bnerv_ctx) of one HIP stream, plus what the host knows about its queue:
    `keep`, the workspaces its queued jobs still read, and `dx_queued`, whether a DATA gradient that ops has already handed to
    autograd is among those jobs (set by ops._end_block, cleared with `keep` by every flush: ops._flush_deferred).  The library
    keeps no global queue: whoever launches on a stream passes that stream's context."""

    def __init__(self):
        h = C.c_void_p()
        check(load().bnerv_ctx_create(C.byref(h)), "bnerv_ctx_create")
        self.handle = h
        self.keep = []
        self.dx_queued = False

    def __del__(self):
        try:
            if _lib is not None and self.handle:
                _lib.bnerv_ctx_destroy(self.handle)
        except Exception:
            pass


_contexts = {}
_ctx_override = []      # innermost last.  A module-level stack on purpose (not thread-local): autograd runs backward on its own thread


def _device_scratch_bytes(dev):
    return max([load().bnerv_ctx_scratch_bytes(o.handle) for (d, _), o in _contexts.items() if d == dev] or [0])


def new_ctx():
    """A private context for whoever captures a graph (engine.TrainStep / DecodeGraph): its scratch is reserved to what the
    device's stream contexts have grown to (a capture cannot allocate), and its weight-fragment plan -- whose arena the captured
    kernels read -- lives and dies with its owner, whatever torch's stream pool hands out to other users later."""
    c = StreamContext()
    reserve_ctx(c)
    return c


def reserve_ctx(c):
    want = _device_scratch_bytes(torch.cuda.current_device())
    if want:
        check(load().bnerv_ctx_reserve(c.handle, want), "bnerv_ctx_reserve")


class use_ctx:
    """with use_ctx(c): every library call made meanwhile (forward, backward) names context c instead of the current stream's.
    The caller keeps all of that work on ONE stream."""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        _ctx_override.append(self.c)
        return self.c

    def __exit__(self, *exc):
        _ctx_override.pop()


def ctx(create=True):
    """Context of torch's current stream (created on first use; one per (device, stream)) unless a use_ctx block is open.  A new
    context reserves the scratch the other contexts of its device have grown to: a stream that is about to be captured into a
    graph cannot allocate.  create=False: None for a stream that has no context yet (nothing can be queued on it)."""
    if _ctx_override:
        return _ctx_override[-1]
    st = torch.cuda.current_stream()
    key = (st.device_index, st.cuda_stream)
    c = _contexts.get(key)
    if c is None and create:
        want = _device_scratch_bytes(st.device_index)
        c = _contexts[key] = StreamContext()
        if want:
            check(load().bnerv_ctx_reserve(c.handle, want), "bnerv_ctx_reserve")
    return c
