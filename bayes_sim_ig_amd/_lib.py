"""ctypes binding of libbsig_hip.so: every public header include/bsig*.h, one table of prototypes per header
(``HEADERS``), merged into the one table (``PROTOS``) the loader and the precision seam read.

Whether a call computes in fp32 or fp64 is decided in ONE place, the two ``Precision`` objects ``F32`` and
``F64`` below: they carry the dtype, the sizes and the entry points that exist in both modes under one
signature, and ``as_rows`` converts a caller's rows to either.  What exists in fp32 only (data parallel, block
launches, debug entry points) is called on the library directly.

The product path has NO fallback: if the library is missing or there is no
GPU, every compute entry point raises.  torch is used only for device memory,
streams and torch.distributed.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from .protocol import eval_updates, split_rows

_HERE = os.path.dirname(os.path.abspath(__file__))
# (BSIG_LIB_PATH: another build of the same library, for A/B measurements of kernel variants)
LIB_PATH = os.environ.get('BSIG_LIB_PATH') or os.path.join(_HERE, 'lib', 'libbsig_hip.so')

BSIG_OK, BSIG_EINVAL, BSIG_ELAUNCH, BSIG_EUNSUPPORTED, BSIG_ENONFINITE = 0, -1, -2, -3, -4
EPI_NONE, EPI_BIAS, EPI_BIAS_ACT, EPI_COS_SIN, EPI_COS_OFF, EPI_MUL_DACT = range(6)
ACT_TANH, ACT_RELU, ACT_LEAKY_RELU, ACT_SIGMOID, ACT_IDENTITY = range(5)
MAX_HIDDEN = 8
FIT_GRAPH, FIT_SPLIT_ADAM = 1, 2
PLAN_NO_PERSISTENT = 1
PLAN_SPLIT_BF16 = 2        # include/bsig_matmul.h
MATMUL_FP32, MATMUL_SPLIT_BF16 = 0, 1
MATMUL_PRECISIONS = {'float32': MATMUL_FP32, 'split_bf16': MATMUL_SPLIT_BF16}
GEMM_PATH_SPLIT_BF16 = 10
X_ROWS, X_CROSSCORR_FACTORS = 0, 1
FLAG_NONFINITE, FLAG_TIMEOUT = 1, 2      # the state block's flag word (csrc/fit_protocol.h)

i64, i32, u64, f32, vp, sz = (C.c_int64, C.c_int32, C.c_uint64, C.c_float,
                              C.c_void_p, C.c_size_t)
f64 = C.c_double


class HeadDims(C.Structure):
    _fields_ = [('out_dim', i32), ('n_comp', i32), ('full_cov', i32),
                ('eps_noise', f32), ('min_weight', f32), ('ll_limit', f32)]


class MdnCfg(C.Structure):
    _fields_ = [('input_dim', i32), ('n_hidden', i32),
                ('hidden', i32 * MAX_HIDDEN), ('activation', i32),
                ('rff_feats', i32), ('rff_cos_only', i32),
                ('rff_scale', f32), ('head', HeadDims),
                ('lr', f32), ('beta1', f32), ('beta2', f32), ('adam_eps', f32)]


class FitBuffers(C.Structure):
    _fields_ = [('params', vp), ('grads', vp), ('exp_avg', vp),
                ('exp_avg_sq', vp),
                ('rff_coeff', vp), ('ld_coeff', i64), ('rff_offset', vp),
                ('x_train', vp), ('ldx_train', i64), ('n_train', i64),
                ('y_train', vp), ('ldy_train', i64),
                ('x_test', vp), ('ldx_test', i64), ('n_test', i64),
                ('y_test', vp), ('ldy_test', i64),
                ('ids_table', vp), ('train_loss', vp), ('test_loss', vp),
                ('state', vp), ('workspace', vp), ('workspace_bytes', sz),
                ('x_kind', i32), ('x_s', i32), ('x_a', i32),
                ('x_test_factors', vp), ('ldx_test_factors', i64)]


class F64Hyper(C.Structure):
    """bsig_f64_hyper (include/bsig_f64.h): the hyper-parameters as doubles"""
    _fields_ = [('lr', f64), ('beta1', f64), ('beta2', f64), ('adam_eps', f64),
                ('eps_noise', f64), ('min_weight', f64), ('ll_limit', f64), ('rff_scale', f64)]


class Fit64Buffers(C.Structure):
    """bsig_fit64_buffers (include/bsig_f64.h)"""
    _fields_ = [('params', vp), ('grads', vp), ('exp_avg', vp), ('exp_avg_sq', vp),
                ('rff_coeff', vp), ('ld_coeff', i64), ('rff_offset', vp),
                ('x_train', vp), ('ldx_train', i64), ('n_train', i64),
                ('y_train', vp), ('ldy_train', i64),
                ('x_test', vp), ('ldx_test', i64), ('n_test', i64),
                ('y_test', vp), ('ldy_test', i64),
                ('ids_table', vp), ('train_loss', vp), ('test_loss', vp),
                ('state', vp), ('workspace', vp), ('workspace_bytes', sz),
                ('x_kind', i32)]


# bsig_fit_chunk (include/bsig.h): one entry per chunk of a block launch, 64 bytes
FIT_CHUNK = np.dtype([('row0', '<i8'), ('n_train', '<i4'), ('n_test', '<i4'), ('ids_off', '<i8'),
                      ('seed', '<u8'), ('rng_ctr0', '<u8'), ('n_updates', '<i4'), ('eval_every', '<i4'),
                      ('train_slot', '<i4'), ('test_slot', '<i4'), ('upd_base', '<i4'), ('eval_base', '<i4')])


def fit_chunk_table(sizes, seeds, n_updates, batch_size, test_frac):
    """The chunk table of a block launch (bsig_fit_run_block) for consecutive chunks of ``sizes`` pairs:
    rows and ids of the chunks follow each other, every chunk holds out its last rows (mdnn.py:206-211),
    evaluates at protocol.eval_updates (mdnn.py:235), starts its jitter
    streams at 1 with its own seed (what bsig_fit_begin does per call) and logs behind the chunk before."""
    every, eval_its = eval_updates(n_updates)
    n_evals = len(eval_its)
    table = np.zeros(len(sizes), dtype=FIT_CHUNK)
    row0 = 0
    for c, (n_tot, seed) in enumerate(zip(sizes, seeds)):
        n_train, n_test = split_rows(n_tot, test_frac)
        table[c] = (row0, n_train, n_test, c * n_updates * batch_size, seed, 1, n_updates, every,
                    c * n_updates, c * n_evals, c * n_updates, c * n_evals)
        row0 += n_tot
    return table


_HD, _HY, _CFG = C.POINTER(HeadDims), C.POINTER(F64Hyper), C.POINTER(MdnCfg)
SIGNATURE_MAX_DEPTH = 6        # include/bsig_signature.h
INPUT_NORM_SLAB_ROWS = 64      # include/bsig_input_norm.h
RFF_BANDWIDTH_MAX_ROWS = 1024                   # include/bsig_rff_bandwidth.h
RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES = 8448     # include/bsig_rff_bandwidth.h
# public header -> the prototypes of its declarations: name -> (restype, argtypes).  A new header adds its
# table here and nothing else; tests/test_headers_host.py holds every table against its header.  (The tables of
# the two base headers also go by a name: an entry point Precision routes fp32 to must not be one of the fp64
# header and the other way round.)
HEADERS = {}
HEADERS['bsig.h'] = _PROTOS = {
    'bsig_last_error': (C.c_char_p, []),
    'bsig_version': (C.c_int, []),
    'bsig_abi_info': (u64, [C.c_int]),
    'bsig_device_count': (C.c_int, []),
    'bsig_summary_dim': (i64, [C.c_int] * 5),
    'bsig_summary_start': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 5 + [i64, vp]),
    'bsig_crosscorr': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 5 + [i64, vp, vp]),
    'bsig_crosscorr_factor_dims': (C.c_int, [C.c_int] * 3 + [C.POINTER(i32)] * 2),
    'bsig_crosscorr_factors': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 5 + [i64, vp, vp]),
    'bsig_crosscorr_expand': (C.c_int, [vp, i64, i64, C.c_int, C.c_int, vp, i64, vp]),
    'bsig_signature': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 4 + [i64, vp]),
    'bsig_gemm_workspace_bytes': (sz, [i64, i64, i64]),
    'bsig_gemm_f32': (C.c_int, [vp, i64, C.c_int, vp, vp, i64, C.c_int, vp, vp,
                                i64, i64, i64, i64, C.c_int, C.c_int, vp, vp,
                                i64, f32, vp, sz, vp]),
    'bsig_rff_coeff': (C.c_int, [vp, vp, vp, i64, i64, i64, vp]),
    'bsig_rff_project': (C.c_int, [vp, i64, vp, vp, i64, vp, vp, i64, i64, i64,
                                   i64, f32, C.c_int, vp, sz, vp]),
    'bsig_head_width': (i64, [C.POINTER(HeadDims)]),
    'bsig_head_workspace_bytes': (sz, [C.POINTER(HeadDims), i64]),
    'bsig_mdn_head_outputs': (C.c_int, [C.POINTER(HeadDims), vp, i64, i64, vp,
                                        u64, u64, vp, vp, vp, vp, vp, vp, sz, vp]),
    'bsig_mdn_nll_from_tuple': (C.c_int, [C.POINTER(HeadDims), vp, vp, vp, vp,
                                          vp, i64, i64, vp, vp, vp, sz, vp]),
    'bsig_mdn_head_nll': (C.c_int, [C.POINTER(HeadDims), vp, i64, vp, i64, vp,
                                    i64, i64, vp, u64, u64, vp, vp, vp, vp, sz,
                                    vp]),
    'bsig_adam_flat': (C.c_int, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, vp]),
    'bsig_colsum': (C.c_int, [vp, i64, i64, i64, vp, vp, sz, vp]),
    'bsig_normalize_rows': (C.c_int, [vp, i64, vp, vp, vp, i64, i64, i64, vp]),
    'bsig_copy_rows': (C.c_int, [vp, i64, vp, vp, i64, i64, i64, vp]),
    'bsig_mdn_param_count': (i64, [C.POINTER(MdnCfg)]),
    'bsig_mdn_param_offsets': (C.c_int, [C.POINTER(MdnCfg), C.POINTER(i64), C.c_int]),
    'bsig_mdn_workspace_bytes': (sz, [C.POINTER(MdnCfg), i64]),
    'bsig_mdn_head_forward': (C.c_int, [C.POINTER(MdnCfg), vp, vp, i64, vp, vp,
                                        i64, vp, i64, vp, i64, vp, sz, vp]),
    'bsig_mdn_loss_grad': (C.c_int, [C.POINTER(MdnCfg), vp, vp, i64, vp, vp, i64,
                                     vp, i64, vp, i64, i64, vp, u64, u64, vp, vp,
                                     vp, vp, sz, vp]),
    'bsig_fit_create': (C.c_int, [C.POINTER(MdnCfg), i64, i64, i64, C.POINTER(vp)]),
    'bsig_fit_create_sized': (C.c_int, [C.POINTER(MdnCfg), i64, i64, i64, i64, C.POINTER(vp)]),
    'bsig_fit_create_ex': (C.c_int, [C.POINTER(MdnCfg), i64, i64, i64, i64, C.c_int, C.POINTER(vp)]),
    'bsig_fit_destroy': (None, [vp]),
    'bsig_fit_workspace_bytes': (sz, [vp]),
    'bsig_fit_bind': (C.c_int, [vp, C.POINTER(FitBuffers), C.c_int]),
    'bsig_fit_begin': (C.c_int, [vp, u64, i64, vp]),
    'bsig_fit_set_features': (C.c_int, [vp, vp, i64, i64, vp]),
    'bsig_fit_run': (C.c_int, [vp, i64, vp]),
    'bsig_fit_grad': (C.c_int, [vp, vp]),
    'bsig_fit_apply': (C.c_int, [vp, vp]),
    'bsig_fit_flush': (C.c_int, [vp, vp]),
    'bsig_fit_is_persistent': (C.c_int, [vp]),
    'bsig_fit_accepts_factors': (C.c_int, [vp]),
    'bsig_fit_accepts_factor_rows': (C.c_int, [vp, C.c_int, C.c_int]),
    'bsig_fit_evaluates_from_factors': (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
    'bsig_fit_takes_features': (C.c_int, [vp, i64]),
    'bsig_fit_eval': (C.c_int, [vp, vp]),
    'bsig_fit_updates': (C.c_int, [vp, i64, vp]),
    'bsig_debug_persist_profile': (None, [vp]),
    'bsig_debug_spin': (C.c_int, [C.c_int, sz, C.c_int, vp]),
    'bsig_debug_persist_geometry': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    'bsig_debug_head_geometry': (C.c_int, [C.POINTER(HeadDims), i64, C.POINTER(C.c_int32)]),
    'bsig_debug_summary_path': (C.c_int, [C.c_int, i64] + [C.c_int] * 6 + [i64, C.c_int, C.c_int,
                                                                         C.POINTER(C.c_int32)]),
    'bsig_debug_mfma_vs_fma': (C.c_int, [vp, vp, C.c_int, vp, vp]),
    'bsig_debug_persist_mdnn_geometry': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    'bsig_comm_unique_id': (C.c_int, [vp]),
    'bsig_comm_init': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    'bsig_comm_init_external': (C.c_int, [C.c_int, C.c_int, vp, vp, C.POINTER(vp)]),
    'bsig_comm_transport': (C.c_int, [vp]),
    'bsig_comm_world': (C.c_int, [vp]),
    'bsig_fit_dp_graph_status': (C.c_int, [vp, C.c_char_p, sz]),
    'bsig_comm_rank': (C.c_int, [vp]),
    'bsig_comm_resident_calls': (i64, [vp]),
    'bsig_comm_set_resident': (None, [vp, C.c_int]),
    'bsig_comm_resident_mode': (C.c_int, [vp]),
    'bsig_comm_allreduce': (C.c_int, [vp, vp, i64, vp]),
    'bsig_comm_broadcast': (C.c_int, [vp, vp, i64, C.c_int, vp]),
    'bsig_comm_destroy': (None, [vp]),
    'bsig_fit_pack_logs': (C.c_int, [vp, i64, vp, vp]),
    'bsig_fit_block_chunks': (C.c_int, [vp, i64]),
    'bsig_fit_run_block': (C.c_int, [vp, vp, i64, i64, vp, i64, vp, i64, vp, vp, C.c_int, vp, vp, vp, i64, vp]),
    'bsig_debug_block_launch': (C.c_int, [C.c_int, C.c_int, C.c_int]),
    'bsig_debug_fit_deferred': (C.c_int, [vp, vp]),
    'bsig_debug_fit_schedule': (C.c_int, [C.c_int, C.c_int, C.c_int, vp, C.c_int]),
    'bsig_fit_run_dp': (C.c_int, [vp, vp, i64, vp, vp]),
}
# the fp64 mode
HEADERS['bsig_f64.h'] = _PROTOS_F64 = {
    'bsig_summary_start_f64': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 5 + [i64, vp]),
    'bsig_crosscorr_f64': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 5 + [i64, vp, vp]),
    'bsig_signature_f64': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 4 + [i64, vp]),
    'bsig_gemm_f64': (C.c_int, [vp, i64, C.c_int, vp, vp, i64, C.c_int, vp, vp, i64, i64, i64, i64,
                                C.c_int, C.c_int, vp, vp, i64, f64, vp]),
    'bsig_rff_project_f64': (C.c_int, [vp, i64, vp, vp, i64, vp, vp, i64, i64, i64, i64, f64, C.c_int, vp]),
    'bsig_head_workspace_bytes_f64': (sz, [_HD, i64]),
    'bsig_mdn_head_outputs_f64': (C.c_int, [_HD, _HY, vp, i64, i64, vp, u64, u64, vp, vp, vp, vp, vp,
                                            vp, sz, vp]),
    'bsig_mdn_nll_from_tuple_f64': (C.c_int, [_HD, _HY, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, sz, vp]),
    'bsig_mdn_head_nll_f64': (C.c_int, [_HD, _HY, vp, i64, vp, i64, vp, i64, i64, vp, u64, u64, vp, vp,
                                        vp, vp, sz, vp]),
    'bsig_adam_flat_f64': (C.c_int, [vp, vp, vp, vp, i64, f64, f64, f64, f64, i64, vp]),
    'bsig_normalize_rows_f64': (C.c_int, [vp, i64, vp, vp, vp, i64, i64, i64, vp]),
    'bsig_copy_rows_f64': (C.c_int, [vp, i64, vp, vp, i64, i64, i64, vp]),
    'bsig_mdn_workspace_bytes_f64': (sz, [_CFG, i64]),
    'bsig_mdn_head_forward_f64': (C.c_int, [_CFG, _HY, vp, vp, i64, vp, vp, i64, vp, i64, vp, i64, vp,
                                            sz, vp]),
    'bsig_mdn_loss_grad_f64': (C.c_int, [_CFG, _HY, vp, vp, i64, vp, vp, i64, vp, i64, vp, i64, i64, vp,
                                         u64, u64, vp, vp, vp, vp, sz, vp]),
    'bsig_fit64_create': (C.c_int, [_CFG, _HY, i64, i64, i64, i64, C.POINTER(vp)]),
    'bsig_fit64_destroy': (None, [vp]),
    'bsig_fit64_workspace_bytes': (sz, [vp]),
    'bsig_fit64_bind': (C.c_int, [vp, C.POINTER(Fit64Buffers), C.c_int]),
    'bsig_fit64_begin': (C.c_int, [vp, u64, i64, vp]),
    'bsig_fit64_run': (C.c_int, [vp, i64, vp]),
    'bsig_fit64_pack_logs': (C.c_int, [vp, i64, i64, vp, vp]),
}
# the matmul precision of the fp32 products
HEADERS['bsig_matmul.h'] = {
    'bsig_gemm_f32_ex': (C.c_int, HEADERS['bsig.h']['bsig_gemm_f32'][1] + [C.c_int]),
    'bsig_rff_project_ex': (C.c_int, HEADERS['bsig.h']['bsig_rff_project'][1] + [C.c_int]),
    'bsig_debug_gemm_path': (C.c_int, [i64, i64, i64, C.c_int, C.c_int, C.c_int, C.c_int, sz, C.c_int,
                                       C.POINTER(C.c_int32)]),
}
# signatures beyond depth 3 and on a chosen subset of channels
HEADERS['bsig_signature.h'] = {
    'bsig_signature_ex_dim': (i64, [C.c_int, C.c_int]),
    'bsig_signature_ex_fits': (C.c_int, [C.c_int] * 4),
    'bsig_signature_ex': (C.c_int, [vp, vp, vp, C.c_int, vp, i64] + [C.c_int] * 4 + [i64, vp]),
    'bsig_signature_ex_f64': (C.c_int, [vp, vp, vp, C.c_int, vp, i64] + [C.c_int] * 4 + [i64, vp]),
}
# the log-signature at the Lyndon words, on the general signature kernel
HEADERS['bsig_logsignature.h'] = {
    'bsig_logsignature_dim': (i64, [C.c_int, C.c_int]),
    'bsig_logsignature_words': (C.c_int, [C.c_int, C.c_int, C.POINTER(i32), i64]),
    'bsig_logsignature': (C.c_int, [vp, vp, vp, C.c_int, vp, vp, i64] + [C.c_int] * 4 + [i64, vp]),
    'bsig_logsignature_f64': (C.c_int, [vp, vp, vp, C.c_int, vp, vp, i64] + [C.c_int] * 4 + [i64, vp]),
}
# column statistics of the estimator's input rows and their standardisation
HEADERS['bsig_input_norm.h'] = {
    'bsig_input_norm_workspace_bytes': (i64, [i64, i64]),
    'bsig_input_norm_stats': (C.c_int, [vp, i64, i64, i64, vp, vp, vp, sz, vp]),
    'bsig_input_norm_stats_f64': (C.c_int, [vp, i64, i64, i64, vp, vp, vp, sz, vp]),
    'bsig_input_norm_apply': (C.c_int, [vp, i64, vp, vp, vp, i64, i64, i64, vp]),
    'bsig_input_norm_apply_f64': (C.c_int, [vp, i64, vp, vp, vp, i64, i64, i64, vp]),
}
# the kernel bandwidth of an RFF map by the median heuristic, and the coefficient from that device scalar
HEADERS['bsig_rff_bandwidth.h'] = {
    'bsig_rff_bandwidth_workspace_bytes': (i64, [i64, i64]),
    'bsig_rff_bandwidth_median': (C.c_int, [vp, i64, i64, i64, f64, vp, vp, sz, vp]),
    'bsig_rff_bandwidth_median_f64': (C.c_int, [vp, i64, i64, i64, f64, vp, vp, sz, vp]),
    'bsig_rff_bandwidth_select': (C.c_int, [vp, i64, vp, vp, sz, vp]),
    'bsig_rff_coeff_dev': (C.c_int, [vp, vp, vp, i64, i64, i64, vp]),
    'bsig_rff_coeff_dev_f64': (C.c_int, [vp, vp, vp, i64, i64, i64, vp]),
}
# the paper's time-lagged cross-correlation summary
HEADERS['bsig_xcorr.h'] = {
    'bsig_xcorr_dim': (i64, [C.c_int] * 3),
    'bsig_xcorr_fits': (C.c_int, [C.c_int] * 7),
    'bsig_xcorr_group': (C.c_int, [C.c_int] * 7),
    'bsig_xcorr': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 6 + [i64, vp, vp]),
    'bsig_xcorr_f64': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 6 + [i64, vp, vp]),
}
# the random-feature kernel mean embedding summary
KME_BLOCK_ROWS = 32            # include/bsig_kme.h
HEADERS['bsig_kme.h'] = {
    'bsig_kme_row_dim': (i64, [C.c_int] * 4),
    'bsig_kme_fits': (C.c_int, [C.c_int] * 8),
    'bsig_kme_group': (C.c_int, [C.c_int] * 8),
    'bsig_kme_rows': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 6 + [i64, vp]),
    'bsig_kme_rows_f64': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 6 + [i64, vp]),
    'bsig_kme_coeff': (C.c_int, [vp, i64, vp, f64, vp, i64, i64, i64, vp]),
    'bsig_kme_coeff_f64': (C.c_int, [vp, i64, vp, f64, vp, i64, i64, i64, vp]),
    'bsig_kme': (C.c_int, [vp, vp, vp, i64, vp, i64] + [C.c_int] * 7 + [i64, vp, vp]),
    'bsig_kme_f64': (C.c_int, [vp, vp, vp, i64, vp, i64] + [C.c_int] * 7 + [i64, vp, vp]),
}
# per-trajectory lengths for the two summaries above: the lengths (and the rows' offsets) follow the trajectories
HEADERS['bsig_ragged.h'] = {
    'bsig_xcorr_ragged': (C.c_int, [vp, vp, vp, vp, i64] + [C.c_int] * 6 + [i64, vp, vp]),
    'bsig_xcorr_ragged_f64': (C.c_int, [vp, vp, vp, vp, i64] + [C.c_int] * 6 + [i64, vp, vp]),
    'bsig_kme_ragged': (C.c_int, [vp, vp, vp, vp, i64, vp, i64] + [C.c_int] * 7 + [i64, vp, vp]),
    'bsig_kme_ragged_f64': (C.c_int, [vp, vp, vp, vp, i64, vp, i64] + [C.c_int] * 7 + [i64, vp, vp]),
    'bsig_kme_rows_ragged': (C.c_int, [vp, vp, vp, vp, vp, i64] + [C.c_int] * 6 + [i64, vp]),
    'bsig_kme_rows_ragged_f64': (C.c_int, [vp, vp, vp, vp, vp, i64] + [C.c_int] * 6 + [i64, vp]),
}
# the least-squares dynamics summary
HEADERS['bsig_sysid.h'] = {
    'bsig_sysid_dim': (i64, [C.c_int] * 2),
    'bsig_sysid_fits': (C.c_int, [C.c_int] * 5),
    'bsig_sysid_group': (C.c_int, [C.c_int] * 5),
    'bsig_sysid': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 4 + [f64, i64, vp, vp]),
    'bsig_sysid_f64': (C.c_int, [vp, vp, vp, i64] + [C.c_int] * 4 + [f64, i64, vp, vp]),
}
# open-loop rollouts of the two analytic tasks, with episode ends
SIM_PENDULUM, SIM_CARTPOLE = 0, 1                              # include/bsig_sim.h
SIM_TASKS = {'pendulum': SIM_PENDULUM, 'cartpole': SIM_CARTPOLE}
SIM_EPISODES, SIM_STEP_BLOCK, SIM_GRID_CAP = 64, 8, 2048       # include/bsig_sim.h
HEADERS['bsig_sim.h'] = {
    'bsig_sim_dims': (C.c_int, [C.c_int] + [C.POINTER(C.c_int)] * 3),
    'bsig_sim_rollout': (C.c_int, [C.c_int] + [vp] * 6 + [i64] + [C.c_int] * 3 + [vp, vp]),
    'bsig_sim_rollout_f64': (C.c_int, [C.c_int] + [vp] * 6 + [i64] + [C.c_int] * 3 + [vp, vp]),
}
# closed-loop rollouts: an MLP policy inside the rollout kernel
SIM_ACTIVATIONS = {'identity': 0, 'relu': 1, 'tanh': 2}         # include/bsig_sim_policy.h
SIM_POLICY_MAX_HIDDEN, SIM_POLICY_MAX_WIDTH, SIM_POLICY_UNITS = 2, 64, 4
HEADERS['bsig_sim_policy.h'] = {
    'bsig_sim_policy_size': (i64, [C.c_int] * 4),
    'bsig_sim_rollout_policy': (C.c_int, [C.c_int] + [vp] * 5 + [C.c_int] * 4 + [vp] * 3 + [i64] + [C.c_int] * 3
                                + [vp, vp]),
    'bsig_sim_rollout_policy_f64': (C.c_int, [C.c_int] + [vp] * 5 + [C.c_int] * 4 + [vp] * 3 + [i64]
                                    + [C.c_int] * 3 + [vp, vp]),
}
# rollouts whose numbers are drawn inside the kernel by a counter-based generator
SIM_DRAW_STEP, SIM_DRAW_THETA, SIM_DRAW_INIT = 0, 1, 2         # include/bsig_sim_draws.h: the counter's purpose word
_DRAWN = [C.c_int, vp, vp] + [vp] * 4 + [f64] * 4 + [u64, u64] + [vp] + [C.c_int] * 4 + [vp] * 7 \
    + [i64, C.c_int, C.c_int, vp, vp]
HEADERS['bsig_sim_draws.h'] = {
    'bsig_philox4x32_10': (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, i64, vp]),
    'bsig_sim_rollout_drawn': (C.c_int, _DRAWN),
    'bsig_sim_rollout_drawn_f64': (C.c_int, list(_DRAWN)),
}
COMM_ID_BYTES = 128
EXCHANGE_SUM, EXCHANGE_BROADCAST = 0, 1
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, vp, C.c_int, vp, i64, C.c_int, vp)



def _merged(headers):
    """Every header's prototypes in one table.  A name belongs to one header: ImportError otherwise."""
    protos = {}
    for header, table in headers.items():
        twice = sorted(set(table) & set(protos))
        if twice:
            raise ImportError('include/%s declares %s, which another header declares too' % (header, twice))
        protos.update(table)
    return protos


PROTOS = _merged(HEADERS)

_lib = None


def exported_symbols(header='bsig.h'):
    """Names every declaration of include/<header> must resolve to; ``header=None``: those of every header."""
    return sorted(PROTOS if header is None else HEADERS[header])


def matmul_precision(name):
    """'float32' | 'split_bf16' -> BSIG_MATMUL_* (include/bsig_matmul.h); ValueError on anything else."""
    if name not in MATMUL_PRECISIONS:
        raise ValueError("matmul precision must be 'float32' or 'split_bf16', not %r" % (name,))
    return MATMUL_PRECISIONS[name]


def default_matmul_precision():
    """The process default: the environment variable BSIG_MATMUL_PRECISION, else 'float32'."""
    name = os.environ.get('BSIG_MATMUL_PRECISION') or 'float32'
    matmul_precision(name)
    return name


def load():
    """Load the shared library (no GPU needed for loading)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'libbsig_hip.so not built (%s): run ./build.sh or '
                '__graft_entry__.build(); there is no CPU fallback' % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _check_abi(lib)
        _lib = lib
    return _lib


HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'bsig.h')


def header_hash(path=HEADER_PATH):
    """64-bit FNV-1a of include/bsig.h (what build.sh hands the compiler as BSIG_HEADER_HASH)."""
    h = 0xcbf29ce484222325
    with open(path, 'rb') as f:
        for b in f.read():
            h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _check_abi(lib):
    """The library's view of include/bsig.h against this binding's: struct sizes always, the
    header text when the header is next to the package (a library or an object file built against
    another revision of the header must not be driven through these ctypes mirrors)."""
    want = {1: C.sizeof(HeadDims), 2: C.sizeof(MdnCfg), 3: C.sizeof(FitBuffers),
            4: FitBuffers.x_kind.offset}
    for which, size in want.items():
        got = int(lib.bsig_abi_info(which))
        if got != size:
            raise RuntimeError('libbsig_hip.so was built against another include/bsig.h (layout %d: '
                               'library %d, binding %d): rebuild with ./build.sh' % (which, got, size))
    built = int(lib.bsig_abi_info(0))
    if built and os.path.exists(HEADER_PATH) and built != header_hash():
        raise RuntimeError('libbsig_hip.so was built from another revision of include/bsig.h '
                           '(hash %016x, header %016x): rebuild with ./build.sh'
                           % (built, header_hash()))


def require_gpu():
    """The product path runs on MI355X only — fail loudly otherwise."""
    lib = load()
    if not torch.cuda.is_available():
        raise RuntimeError('bayes_sim_ig_amd needs a ROCm GPU (MI355X): '
                           'torch.cuda.is_available() is False and there is '
                           'no CPU fallback')
    return lib


def check(rc):
    if rc == BSIG_OK:
        return
    msg = load().bsig_last_error().decode('utf-8', 'replace')
    if rc == BSIG_EINVAL:
        raise AssertionError(msg)        # the reference asserts on bad shapes
    if rc == BSIG_EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError('libbsig_hip: %s (code %d)' % (msg, rc))


class Precision:
    """The one place where "fp32 or fp64" is decided: the dtype and its sizes, the buffers struct of a fit
    plan and every entry point that exists in both precisions, under ONE signature per operation -- the
    fp64 one, with the bsig_f64_hyper* behind the dims / cfg argument (include/bsig_f64.h); F32 drops it
    and calls the unsuffixed symbol.  Calls that return a code are checked.  The entry points are resolved
    together, on the first use of any, and then are plain attributes of the instance.

    What an fp64 plan cannot do (persistent kernels, factor rows, handed-over features, block launches) it
    answers here, WITHOUT calling the library: no bsig_fit_* function ever sees a plan that
    bsig_fit64_create made."""
    # operation -> (fp32 symbol, fp64 symbol), whichever header declares them
    OPS = {
        'summary_start': ('bsig_summary_start', 'bsig_summary_start_f64'),
        'crosscorr': ('bsig_crosscorr', 'bsig_crosscorr_f64'),
        'signature': ('bsig_signature', 'bsig_signature_f64'),
        'head_workspace_bytes': ('bsig_head_workspace_bytes', 'bsig_head_workspace_bytes_f64'),
        'mdn_workspace_bytes': ('bsig_mdn_workspace_bytes', 'bsig_mdn_workspace_bytes_f64'),
        'head_forward': ('bsig_mdn_head_forward', 'bsig_mdn_head_forward_f64'),
        'head_outputs': ('bsig_mdn_head_outputs', 'bsig_mdn_head_outputs_f64'),
        'nll_from_tuple': ('bsig_mdn_nll_from_tuple', 'bsig_mdn_nll_from_tuple_f64'),
        'loss_grad': ('bsig_mdn_loss_grad', 'bsig_mdn_loss_grad_f64'),
        'adam_flat': ('bsig_adam_flat', 'bsig_adam_flat_f64'),
        'normalize_rows': ('bsig_normalize_rows', 'bsig_normalize_rows_f64'),
        'copy_rows': ('bsig_copy_rows', 'bsig_copy_rows_f64'),
        'signature_ex': ('bsig_signature_ex', 'bsig_signature_ex_f64'),
        'logsignature': ('bsig_logsignature', 'bsig_logsignature_f64'),
        'xcorr': ('bsig_xcorr', 'bsig_xcorr_f64'),
        # the kernel mean embedding, its rows written out and its coefficients in the output precision
        'kme': ('bsig_kme', 'bsig_kme_f64'),
        'kme_rows': ('bsig_kme_rows', 'bsig_kme_rows_f64'),
        'kme_coeff': ('bsig_kme_coeff', 'bsig_kme_coeff_f64'),
        # both summaries, and the embedding's rows, with a length per trajectory (include/bsig_ragged.h)
        'xcorr_ragged': ('bsig_xcorr_ragged', 'bsig_xcorr_ragged_f64'),
        'kme_ragged': ('bsig_kme_ragged', 'bsig_kme_ragged_f64'),
        'kme_rows_ragged': ('bsig_kme_rows_ragged', 'bsig_kme_rows_ragged_f64'),
        'sysid': ('bsig_sysid', 'bsig_sysid_f64'),
        # the rollouts of the analytic tasks (include/bsig_sim.h): fp32 data or double data, double arithmetic
        'sim_rollout': ('bsig_sim_rollout', 'bsig_sim_rollout_f64'),
        # the same under an MLP policy evaluated in the kernel (include/bsig_sim_policy.h)
        'sim_rollout_policy': ('bsig_sim_rollout_policy', 'bsig_sim_rollout_policy_f64'),
        # the same with every number drawn inside the kernel (include/bsig_sim_draws.h)
        'sim_rollout_drawn': ('bsig_sim_rollout_drawn', 'bsig_sim_rollout_drawn_f64'),
        # the input-side companions of normalize_rows / copy_rows (the statistics of rows, and the copy that
        # standardises)
        'input_norm_stats': ('bsig_input_norm_stats', 'bsig_input_norm_stats_f64'),
        'input_norm_apply': ('bsig_input_norm_apply', 'bsig_input_norm_apply_f64'),
        # the median bandwidth of rows of either type, and freqs / sigma in the model's precision
        'rff_bandwidth_median': ('bsig_rff_bandwidth_median', 'bsig_rff_bandwidth_median_f64'),
        'rff_coeff_dev': ('bsig_rff_coeff_dev', 'bsig_rff_coeff_dev_f64'),
    }
    HYPER_OPS = ('head_forward', 'head_outputs', 'nll_from_tuple', 'loss_grad')    # take the hyper in fp64
    # the plan lifecycle
    FIT_OPS = {
        'fit_create': ('bsig_fit_create_ex', 'bsig_fit64_create'),
        'fit_destroy': ('bsig_fit_destroy', 'bsig_fit64_destroy'),
        'fit_workspace_bytes': ('bsig_fit_workspace_bytes', 'bsig_fit64_workspace_bytes'),
        'fit_bind': ('bsig_fit_bind', 'bsig_fit64_bind'),
        'fit_begin': ('bsig_fit_begin', 'bsig_fit64_begin'),
        'fit_run': ('bsig_fit_run', 'bsig_fit64_run'),
        'fit_pack_logs': ('bsig_fit_pack_logs', 'bsig_fit64_pack_logs'),
    }
    # what a plan can do -> (the fp32 symbol, what an fp64 plan answers); fit_set_features: an fp64 plan
    # declines, as an fp32 plan without a feature cache does
    QUERIES = {
        'is_persistent': ('bsig_fit_is_persistent', 0),
        'accepts_factor_rows': ('bsig_fit_accepts_factor_rows', 0),
        'evaluates_from_factors': ('bsig_fit_evaluates_from_factors', 0),
        'takes_features': ('bsig_fit_takes_features', 0),
        'block_chunks': ('bsig_fit_block_chunks', 0),
        'fit_set_features': ('bsig_fit_set_features', BSIG_EUNSUPPORTED),
    }

    # every operation's pair: (fp32 symbol, fp64 symbol, or what an fp64 plan answers in its place)
    _SYMBOLS = {**OPS, **FIT_OPS, **QUERIES}
    assert len(_SYMBOLS) == len(OPS) + len(FIT_OPS) + len(QUERIES)

    def __init__(self, dtype):
        self.dtype = dtype
        self.itemsize = 8 if dtype == torch.float64 else 4
        self.np_dtype = np.float64 if self.itemsize == 8 else np.float32
        self.Buffers, self.state_words = (Fit64Buffers, 32) if self.itemsize == 8 else (FitBuffers, 16)
        # fp32 replays an update from a HIP graph, so a call's rows are staged at fixed addresses; fp64
        # has no graphs: it binds the rows where they lie and is never asked for one (FIT_GRAPH)
        self.replays_graphs = self.itemsize == 4
        other = _PROTOS if self.itemsize == 8 else _PROTOS_F64      # the other precision's own header
        for op in self._SYMBOLS:                                                 # (a typo fails the import)
            name = self.symbol(op)
            assert name is None or (name in PROTOS and name not in other), op

    def __repr__(self):
        return 'Precision(%s)' % (self.dtype,)

    def symbol(self, op):
        """The library symbol behind ``op``; None where this precision answers without the library."""
        if op in self.QUERIES and self.itemsize == 8:
            return None
        return self._SYMBOLS[op][self.itemsize == 8]

    def __getattr__(self, op):       # the first use of an entry point
        if op not in self._SYMBOLS:
            raise AttributeError(op)
        self._resolve()
        return vars(self)[op]

    def _resolve(self):
        lib, is64 = load(), self.itemsize == 8

        def checked(fn, drop_hyper=False):
            if drop_hyper:
                return lambda first, hyper, *rest: check(fn(first, *rest))
            return lambda *args: check(fn(*args))

        for op in self._SYMBOLS:
            name = self.symbol(op)
            if name is None:                          # what an fp64 plan answers without the library
                fn = (lambda *args, answer=self.QUERIES[op][1]: answer)
            else:
                fn = getattr(lib, name)
                # a return code is checked (the others: a size, nothing; a query's answer is the caller's)
                if op not in self.QUERIES and PROTOS[name][0] is C.c_int:
                    fn = checked(fn, drop_hyper=op in self.HYPER_OPS and not is64)
            setattr(self, op, fn)
        create, pack = self.fit_create, self.fit_pack_logs

        def fit_create(cfg, hyper, batch, max_train, max_test, n_updates, flags):
            handle = C.c_void_p()
            if is64:
                # (an fp64 plan IS per-phase launches: that option holds by itself; there is no other)
                if flags & ~PLAN_NO_PERSISTENT:
                    raise NotImplementedError('bsig_fit64_create takes no plan flags (%d)' % flags)
                create(cfg, hyper, batch, max_train, max_test, n_updates, C.byref(handle))
            else:
                create(cfg, batch, max_train, max_test, n_updates, flags, C.byref(handle))
            return handle
        self.fit_create = fit_create
        if not is64:
            self.fit_pack_logs = lambda plan, n_updates, n_evals, out, st: pack(plan, n_updates, out, st)


F32, F64 = Precision(torch.float32), Precision(torch.float64)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device=None):
    """torch's current stream of ``device`` (default: the current device) as a hipStream_t."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device(device):
    """Context: make ``device`` the current HIP device (kernels launch on the current
    device; a model built on cuda:1 must not launch on cuda:0's stream)."""
    return torch.cuda.device(device)


@contextlib.contextmanager
def device_stream(device):
    """Context: ``on_device(device)``, yielding ``stream(device)`` -- the ONE rule for where a call of the
    summarizers, the embedding and the RFF map launches: on the device its rows live on, on that device's
    current torch stream, whichever device was current before (and is again afterwards)."""
    with on_device(device):
        yield stream(device)


def as_rows(t, device=None, dtype=torch.float32):
    """``dtype`` (fp32 or fp64), last dim contiguous, on the GPU.  Returns (tensor, ld).  The smaller form
    crosses the bus: an input is narrowed to fp32 before the move to the device, widened to fp64 after it."""
    if hasattr(t, 'materialize'):      # a lazy summary handle (summarizers.CrossCorrFactors)
        t = t.materialize()
    if dtype != torch.float64 and t.dtype != dtype:
        t = t.to(dtype)
    if device is not None and t.device != torch.device(device):
        t = t.to(device)
    if not t.is_cuda:
        raise RuntimeError('expected a GPU tensor (no CPU fallback)')
    if t.dtype != dtype:
        t = t.to(dtype)
    if t.dim() != 2:
        raise AssertionError('expected a 2-D tensor')
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    return t, ld


as_f32_rows = as_rows      # (the fp32-only callers: rff.py, the block launch, factor rows)


def round_up(x, m):
    return (x + m - 1) // m * m
