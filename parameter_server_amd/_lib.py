"""ctypes binding of the native C ABI (include/psg.h) in libpsg.so.

The library is built in-tree by ``__graft_entry__.build()`` (or
``make -C parameter_server_amd/csrc``).  There is no fallback: if the
shared object is missing, :func:`lib` raises, so nothing silently runs a CPU
path in its place.

``torch`` is imported before the library is loaded whenever it is
available, so that the process holds ONE HIP runtime (torch's bundled
``libamdhip64.so.7``, which then also satisfies libpsg's dependency by
soname) and device pointers / streams from torch are valid here.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PSG_LIB_PATH: benchmarking aid (an A/B build of the same sources)
LIB_PATH = os.environ.get("PSG_LIB_PATH") or os.path.join(_HERE, "libpsg.so")

PSG_OK = 0
PSG_ERR_ARG = -1
PSG_ERR_UNMATCHED = -2
PSG_ERR_RANGE = -3
PSG_ERR_NO_TIME = -4
PSG_ERR_OOM = -5
PSG_ERR_DEVICE = -6
PSG_ERR_UNSORTED = -7
PSG_ERR_SIZE = -8
PSG_ERR_CHANNEL = -9
PSG_ERR_EMPTY_KEYS = -10
PSG_ERR_SIGNATURE = -11
PSG_KC_SIG = 1
PSG_KC_KEYS = 2
PSG_KC_ERASE = 4
PSG_MAX_SIG_LEN = 2048
PSG_NO_SLICE = (1 << 64) - 1  # (size_t)-1: psg_push_dev without a slice claim

PSG_F32 = 0
PSG_F64 = 1
PSG_SERIAL_MATCH = 0
PSG_PARALLEL_MATCH = 1
PSG_HOLD_BUFFERS = 0x100
# kernel-form overrides (include/psg.h): tests and A/B measurements only
PSG_FORM_PACKED = 0x1000
PSG_FORM_UNIFORM = 0x2000
PSG_PART_SEARCH = 0x4000
PSG_PART_STREAM = 0x8000
PSG_GROUP32 = 0x10000
PSG_GROUP64 = 0x20000
PSG_NO_DENSE = 0x40000
PSG_NO_ZERO_COPY = 0x80000
PSG_NO_INDEX = 0x100000
# plan option: push keys fixed for the plan's lifetime (enables the dense kernel)
PSG_STATIC_KEYS = 0x200000
PSG_FORM_CURSOR = 0x400000
PSG_NO_CURSOR = 0x800000
PSG_NO_HINTS = 0x1000000
# psg_plan_form: the aggregate kernel a plan runs
(PSG_KERNEL_TILE, PSG_KERNEL_TILE64, PSG_KERNEL_PACKED, PSG_KERNEL_DENSE, PSG_KERNEL_CURSOR,
 PSG_KERNEL_PACKED_CURSOR) = range(6)
MAX_VALUE_ARRAYS = 4
# psg_mb_stage_ms's stages, in order
MB_STAGES = ("sort", "run_length", "localize", "count_keys", "times", "logit", "trans_times")
# psg_mb_gradient's loss and psg_mb_read's arrays
PSG_LOSS_LOGIT = 0
(PSG_MB_SORTED_KEY, PSG_MB_SORTED_POS, PSG_MB_UNIQ_KEY, PSG_MB_KEY_CNT, PSG_MB_NEW_OFFSET,
 PSG_MB_NEW_INDEX, PSG_MB_NEW_VALUE, PSG_MB_POS, PSG_MB_NEG, PSG_MB_XW, PSG_MB_TAU, PSG_MB_LOSS,
 PSG_MB_GRAD, PSG_MB_RUN_START, PSG_MB_REMAPPED, PSG_MB_ROW_OF, PSG_MB_SCRATCH) = range(17)
# psg_auc_evaluate's modes
PSG_AUC_BY_KEY, PSG_AUC_AS_WRITTEN = 0, 1
# ... and the Darling worker's state (psg_mb_darling_*)
(PSG_MB_DARLING_DUAL, PSG_MB_DARLING_CUR_W, PSG_MB_DARLING_DELTA, PSG_MB_DARLING_ACTIVE,
 PSG_MB_DARLING_DELTA_W) = range(32, 37)
# ... and the loaded CSR
PSG_MB_OFFSET, PSG_MB_INDEX, PSG_MB_VALUE, PSG_MB_Y = range(24, 28)
# psg_mb_load_text's formats (DataConfig's values)
PSG_TEXT_ADFEA, PSG_TEXT_LIBSVM = 4, 5
# ... the entries' slot ids, and psg_slot_info's formats (SlotInfo)
PSG_MB_SLOT = 28
PSG_SLOT_DENSE, PSG_SLOT_SPARSE, PSG_SLOT_SPARSE_BINARY = 1, 2, 3
# psg_mb_cache_pack's arrays
PSG_CACHE_COLIDX, PSG_CACHE_ROWSIZ, PSG_CACHE_VALUE, PSG_CACHE_LABEL = range(4)

# Every symbol include/psg.h declares, with its ctypes signature.
_u64 = C.c_uint64
_sz = C.c_size_t
_p = C.c_void_p
_pu64 = C.POINTER(C.c_uint64)
_psz = C.POINTER(C.c_size_t)


class MergeJob(C.Structure):
    """psg_merge_job (include/psg.h)."""

    _fields_ = [
        ("keys", _p),
        ("nslots", _u64),
        ("npush", C.c_int),
        ("push_keys", C.POINTER(_p)),
        ("push_vals", C.POINTER(_p)),
        ("push_n", _pu64),
        ("out", C.POINTER(_p)),
    ]


class FtrlParam(C.Structure):
    """psg_ftrl_param (include/psg.h)."""

    _fields_ = [("alpha", C.c_double), ("beta", C.c_double),
                ("lambda1", C.c_double), ("lambda2", C.c_double)]


class DarlingParam(C.Structure):
    """psg_darling_param (include/psg.h)."""

    _fields_ = [("eta", C.c_double), ("lambda_", C.c_double),
                ("kkt_filter_threshold", C.c_double), ("delta_max", C.c_double)]


class TextResult(C.Structure):
    """psg_text_result (include/psg.h)."""

    _fields_ = [("rows", _u64), ("nnz", _u64), ("consumed", _u64), ("bad_line", C.c_int64),
                ("slow_tokens", _u64), ("parse_ms", C.c_double)]


class SlotInfo(C.Structure):
    """psg_slot_info (include/psg.h)."""

    _fields_ = [("id", C.c_int32), ("format", C.c_int32), ("min_key", _u64), ("max_key", _u64),
                ("nnz_ele", _u64), ("nnz_ex", _u64)]


class CacheArray(C.Structure):
    """psg_cache_array (include/psg.h)."""

    _fields_ = [("data", _p), ("nbytes", _sz), ("parts", _pu64), ("nparts", _sz)]


class CacheFile(C.Structure):
    """psg_cache_file (include/psg.h)."""

    _fields_ = [("colidx", CacheArray), ("rowsiz", CacheArray), ("value", CacheArray),
                ("label", CacheArray), ("num_ex", _u64)]


class CacheResult(C.Structure):
    """psg_cache_result (include/psg.h)."""

    _fields_ = [("rows", _u64), ("nnz", _u64), ("bad_file", C.c_int64), ("bad_what", C.c_int32),
                ("bad_part", C.c_int32)]


SIGNATURES = {
    "psg_abi_version": (C.c_int, []),
    "psg_status_string": (C.c_char_p, [C.c_int]),
    "psg_last_error": (C.c_char_p, []),
    "psg_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "psg_create": (C.c_int, [C.c_int, C.c_int, C.c_uint, C.POINTER(_p)]),
    "psg_destroy": (C.c_int, [_p]),
    "psg_set_flush_pushes": (C.c_int, [_p, C.c_int]),
    "psg_set_match_flags": (C.c_int, [_p, C.c_uint]),
    "psg_key_union": (C.c_int, [_p, C.c_int, _p, _sz]),
    "psg_key_size": (C.c_int, [_p, C.c_int, _psz]),
    "psg_key_copy": (C.c_int, [_p, C.c_int, _sz, _sz, _p]),
    "psg_find_range": (C.c_int, [_p, C.c_int, _u64, _u64, _psz, _psz]),
    "psg_value_assign": (C.c_int, [_p, C.c_int, _p, _sz]),
    "psg_value_size": (C.c_int, [_p, C.c_int, _psz]),
    "psg_value_copy": (C.c_int, [_p, C.c_int, _sz, _sz, _p]),
    "psg_push": (C.c_int, [_p, C.c_int, C.c_int, _u64, _u64, _p, _sz, C.c_int,
                           C.POINTER(_p)]),
    "psg_push_cached": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _u64, _u64, C.c_uint,
                                  C.c_uint32, _p, _sz, C.c_int, _p, _sz]),
    "psg_key_cache_clear": (C.c_int, [_p, C.c_int]),
    "psg_push_compressed": (C.c_int, [_p, C.c_int, C.c_int, _u64, _u64, _p, _sz, C.c_int,
                                      _p, _p]),
    "psg_key_cache_bytes": (C.c_int, [_p, C.c_int, _psz]),
    "psg_received_shape": (C.c_int, [_p, C.c_int, C.POINTER(C.c_int), _psz, _psz]),
    "psg_received": (C.c_int, [_p, C.c_int, C.c_int, C.POINTER(_p)]),
    "psg_gather": (C.c_int, [_p, C.c_int, _p, _sz, _p, _psz]),
    "psg_gather_compressed": (C.c_int, [_p, C.c_int, _p, _sz, _p, _sz, _psz, _psz]),
    "psg_push_dev": (C.c_int, [_p, C.c_int, C.c_int, _u64, _u64, _p, _sz, C.c_int,
                               C.POINTER(_p), _sz, _p]),
    "psg_pull_dev": (C.c_int, [_p, C.c_int, _p, _sz, _p, _p, _p]),
    "psg_dev_status": (C.c_int, [_p]),
    "psg_plan_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint,
                                  C.POINTER(MergeJob), C.c_int, C.POINTER(_p)]),
    "psg_plan_max_push": (C.c_int, []),
    "psg_plan_run": (C.c_int, [_p, _p]),
    "psg_plan_run_stage": (C.c_int, [_p, C.c_int, _p]),
    "psg_plan_matched": (C.c_int, [_p, _pu64]),
    "psg_plan_bytes": (C.c_int, [_p, _pu64, _pu64]),
    "psg_plan_form": (C.c_int, [_p, C.POINTER(C.c_int)]),
    "psg_plan_index_info": (C.c_int, [_p, _pu64, _pu64]),
    "psg_plan_hint_state": (C.c_int, [_p, _pu64]),
    "psg_plan_destroy": (C.c_int, [_p]),
    "psg_gather_dev": (C.c_int, [C.c_int, _p, _u64, _p, _p, _u64, _p, _p, _p]),
    "psg_key_union_dev": (C.c_int, [_p, _u64, _p, _u64, _p, _pu64, _p]),
    "psg_shard_bounds": (C.c_int, [_sz, _pu64]),
    "psg_slice_dev": (C.c_int, [_p, _u64, _u64, _u64, _p, C.c_int, _p, _p]),
    "psg_crc32c_dev": (C.c_int, [_p, _p, _u64, _u64, _p, _p, _p]),
    "psg_snappy_uncompress_dev": (C.c_int, [_p, _p, _u64, _p, _p, _p, _p]),
    "psg_snappy_uncompressed_length": (C.c_int, [_p, _sz, _psz]),
    "psg_snappy_max_compressed_length": (_sz, [_sz]),
    "psg_snappy_compress_scratch_bytes": (_sz, [_sz, _u64]),
    "psg_snappy_compress_dev": (C.c_int, [_p, _p, _u64, _p, _p, _p, _p, _p]),
    "psg_snappy_compress_host": (C.c_int, [_p, _sz, _p, _sz, _psz]),
    "psg_freq_resize": (C.c_int, [_p, C.c_int, C.c_int, C.c_int]),
    "psg_freq_clear": (C.c_int, [_p, C.c_int]),
    "psg_freq_empty": (C.c_int, [_p, C.c_int, C.POINTER(C.c_int)]),
    "psg_freq_insert": (C.c_int, [_p, C.c_int, _p, _p, _sz]),
    "psg_freq_query": (C.c_int, [_p, C.c_int, _p, _sz, C.c_int, _p, _psz]),
    "psg_freq_insert_dev": (C.c_int, [_p, C.c_int, _p, _p, _sz, _p]),
    "psg_freq_query_scratch_bytes": (_sz, [_sz]),
    "psg_freq_query_dev": (C.c_int, [_p, C.c_int, _p, _sz, C.c_int, _p, _p, _p, _p]),
    "psg_freq_table": (C.c_int, [_p, C.c_int, _p, _sz]),
    "psg_freq_table_assign": (C.c_int, [_p, C.c_int, _p, _sz]),
    "psg_comm_unique_id": (C.c_int, [_p]),
    "psg_comm_init": (C.c_int, [C.c_int, C.c_int, _p, C.c_int, C.POINTER(_p)]),
    "psg_comm_destroy": (C.c_int, [_p]),
    "psg_comm_init_loopback": (C.c_int, [C.c_int, C.c_int, C.POINTER(_p)]),
    "psg_exchange_create": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _p, _p, _p,
                                      C.POINTER(_p)]),
    "psg_exchange_run": (C.c_int, [_p, _p]),
    "psg_exchange_recv": (C.c_int, [_p, C.POINTER(_p), _p, _pu64, _p, _pu64]),
    "psg_exchange_destroy": (C.c_int, [_p]),
    "psg_exchange_status": (C.c_int, [_p, _pu64]),
    "psg_exchange_create_local": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p,
                                            _p, _p, C.POINTER(_p)]),
    "psg_exchange_set_direct": (C.c_int, [_p, C.c_int]),
    "psg_exchange_send_layout": (C.c_int, [_p, C.POINTER(_p), _p, _p]),
    "psg_key_union_batch": (C.c_int, [_p, C.c_int, _p, _p, C.c_int]),
    "psg_nway_max_push": (C.c_int, []),
    "psg_nway_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, _p, _p, _p, _p,
                                  _p, C.POINTER(_p)]),
    "psg_nway_create_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, _p, _p, _p,
                                         _p, _p, _p, C.POINTER(_p)]),
    "psg_nway_run": (C.c_int, [_p, _p]),
    "psg_nway_count_dev": (C.c_int, [_p, C.POINTER(_p)]),
    "psg_nway_result": (C.c_int, [_p, _pu64]),
    "psg_nway_bytes": (C.c_int, [_p, _pu64, _pu64]),
    "psg_nway_destroy": (C.c_int, [_p]),
    "psg_nway_shape": (C.c_int, [C.c_int, _p, _pu64, _p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "psg_nway_splitters": (C.c_int, [_p, C.c_int, _pu64]),
    "psg_darling_init": (C.c_int, [_p, C.c_int, C.c_double]),
    "psg_darling_reset_active": (C.c_int, [_p, C.c_int]),
    "psg_darling_update": (C.c_int, [_p, C.c_int, C.c_int, _p, C.POINTER(C.c_double)]),
    "psg_darling_update_dev": (C.c_int, [_p, C.c_int, C.c_int, _p]),
    "psg_darling_progress": (C.c_int, [_p, C.c_int, C.c_double, C.c_int, _psz,
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), _psz]),
    "psg_darling_state": (C.c_int, [_p, C.c_int, _sz, _sz, _p, _p, _psz]),
    "psg_ftrl_init": (C.c_int, [_p, _p, _sz]),
    "psg_ftrl_reserve": (C.c_int, [_p, _sz]),
    "psg_ftrl_push": (C.c_int, [_p, _p, _sz, _p, _p, _p]),
    "psg_ftrl_push_dev": (C.c_int, [_p, _p, _sz, _p, _p, _p, _p]),
    "psg_ftrl_pull": (C.c_int, [_p, _p, _sz, _p]),
    "psg_ftrl_pull_dev": (C.c_int, [_p, _p, _sz, _p, _p]),
    "psg_ftrl_status": (C.c_int, [_p, _psz, _psz, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "psg_ftrl_export": (C.c_int, [_p, _p, _p, _sz, _psz]),
    "psg_ftrl_lookup": (C.c_int, [_p, _p, _sz, _p, _p, _p, _p, _p]),
    "psg_ftrl_import": (C.c_int, [_p, _p, _sz, _p, _p, _p, _p]),
    "psg_ftrl_import_dev": (C.c_int, [_p, _p, _sz, _p, _p, _p, _p, _p]),
    "psg_ftrl_export_state": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _sz, _psz]),
    "psg_ftrl_export_state_dev": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _sz, _p, _p]),
    "psg_ftrl_frozen": (C.c_int, [_p, C.POINTER(C.c_int)]),
    "psg_mb_create": (C.c_int, [_p, C.POINTER(_p)]),
    "psg_mb_destroy": (None, [_p]),
    "psg_mb_load": (C.c_int, [_p, _p, _sz, _p, _p, _p]),
    "psg_mb_uniq": (C.c_int, [_p, C.POINTER(_p), C.POINTER(_p), _psz]),
    "psg_mb_localize": (C.c_int, [_p, _p, _sz, C.POINTER(_p), C.POINTER(_p), _p]),
    "psg_mb_times": (C.c_int, [_p, _p, _p, _p]),
    "psg_mb_trans_times": (C.c_int, [_p, _p, _p, _p]),
    "psg_mb_gradient": (C.c_int, [_p, C.c_int, _p, C.POINTER(_p), C.POINTER(C.c_double), _p]),
    "psg_mb_read": (C.c_int, [_p, C.c_int, _p, _sz, _psz]),
    "psg_mb_scratch": (C.c_int, [_p, C.c_int, _sz, C.POINTER(_p)]),
    "psg_mb_profile": (C.c_int, [_p, C.c_int]),
    "psg_mb_stage_ms": (C.c_int, [_p, C.POINTER(C.c_double)]),
    "psg_mb_stream": (C.c_int, [_p, C.POINTER(_p)]),
    "psg_mb_sort_tile": (_sz, []),
    "psg_mb_darling_init": (C.c_int, [_p, C.c_double, _p, _p]),
    "psg_mb_darling_reset_active": (C.c_int, [_p, _p]),
    "psg_mb_darling_gradients": (C.c_int, [_p, _sz, _sz, _p, _p, _p]),
    "psg_mb_darling_update_dual": (C.c_int, [_p, _sz, _sz, _p, C.c_double, _p]),
    "psg_mb_darling_objv": (C.c_int, [_p, C.POINTER(C.c_double), _p]),
    "psg_mb_darling_set_state": (C.c_int, [_p, _p, _p, _p, _p]),
    "psg_mb_labels": (C.c_int, [_p, C.POINTER(_p), C.POINTER(_p)]),
    "psg_mb_load_text": (C.c_int, [_p, _p, _sz, C.c_int, _sz, C.c_int, C.POINTER(TextResult)]),
    "psg_text_parse_host": (C.c_int, [_p, _sz, C.c_int, _sz, C.c_int, _p, _p, _p, _p, _sz, _sz,
                                      C.POINTER(TextResult)]),
    "psg_text_chunk": (_sz, []),
    "psg_mb_load_text_groups": (C.c_int, [_p, _p, _sz, C.c_int, _sz, C.c_int,
                                          C.POINTER(TextResult)]),
    "psg_text_parse_groups_host": (C.c_int, [_p, _sz, C.c_int, _sz, C.c_int, _p, _p, _p, _p, _p,
                                             _sz, _sz, C.POINTER(TextResult)]),
    "psg_mb_set_slots": (C.c_int, [_p, _p, _sz]),
    "psg_mb_groups": (C.c_int, [_p, C.POINTER(SlotInfo), _sz, _psz, C.POINTER(C.c_int64)]),
    "psg_mb_group_extract": (C.c_int, [_p, C.c_int, _p]),
    "psg_even_divide": (C.c_int, [_u64, _u64, _sz, _pu64]),
    "psg_cache_pack_bound": (C.c_int, [_sz, _sz, _psz, _psz]),
    "psg_mb_cache_pack": (C.c_int, [_p, C.c_int, _sz, _p, _sz, _psz, _p, _sz, _psz,
                                    C.POINTER(C.c_int64)]),
    "psg_mb_load_cache": (C.c_int, [_p, C.POINTER(CacheFile), _sz, C.c_int,
                                    C.POINTER(CacheResult)]),
    "psg_cache_scan_tile": (_sz, []),
    "psg_mb_darling_share_dual": (C.c_int, [_p, _p]),
    "psg_auc_create": (C.c_int, [_p, C.c_int64, C.POINTER(_p)]),
    "psg_auc_destroy": (None, [_p]),
    "psg_auc_clear": (C.c_int, [_p]),
    "psg_auc_set_goodness": (C.c_int, [_p, C.c_int64]),
    "psg_auc_add_dev": (C.c_int, [_p, _p, _p, _sz, _p]),
    "psg_auc_add": (C.c_int, [_p, _p, _p, _sz]),
    "psg_auc_merge": (C.c_int, [_p, _p, _p, _sz, _p, _p, _sz]),
    "psg_auc_data": (C.c_int, [_p, _p, _p, _sz, _psz, _p, _p, _sz, _psz]),
    "psg_auc_accuracy_data": (C.c_int, [C.c_int64, _p, _p, _sz, _p, _p, _sz, C.c_double,
                                        C.POINTER(C.c_double)]),
    "psg_auc_evaluate_data": (C.c_int, [_p, _p, _sz, _p, _p, _sz, C.c_int,
                                        C.POINTER(C.c_double)]),
    "psg_auc_accuracy": (C.c_int, [_p, C.c_double, C.POINTER(C.c_double)]),
    "psg_auc_evaluate": (C.c_int, [_p, C.c_int, C.POINTER(C.c_double)]),
    "psg_auc_exact_dev": (C.c_int, [_p, _p, _p, _sz, C.POINTER(C.c_double), _p]),
    "psg_auc_exact": (C.c_int, [_p, _p, _p, _sz, C.POINTER(C.c_double)]),
}

_LIB = None


class PSGError(RuntimeError):
    """A negative psg_status from the native library."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"psg status {status}: {msg}")
        self.status = status


def lib() -> C.CDLL:
    """Load libpsg.so (raises if it has not been built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` "
            "(no CPU fallback exists for this path)")
    try:  # one HIP runtime per process: let torch load it first
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the ABI
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.psg_abi_version() != 1:
        raise ImportError("libpsg ABI version mismatch")
    _LIB = L
    return L


def check(rc: int) -> None:
    if rc != PSG_OK:
        L = lib()
        raise PSGError(rc, L.psg_last_error().decode(errors="replace"))


def ptr_array(ptrs) -> "C.Array":
    arr = (_p * max(1, len(ptrs)))()
    for i, v in enumerate(ptrs):
        arr[i] = v
    return arr
