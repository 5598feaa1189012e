"""ctypes binding of ``libdiffattn.so`` (C ABI declared in ``include/diffattn.h``).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C
differential_transformer_replication_amd/csrc``) for gfx950 only.  There is no
fallback: if the library is missing or cannot load, every op raises.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DTA_LIB", os.path.join(_HERE, "lib", "libdiffattn.so"))

DTA_BF16, DTA_F16, DTA_F32 = 0, 1, 2
_DTYPES = {torch.bfloat16: DTA_BF16, torch.float16: DTA_F16, torch.float32: DTA_F32}

ABI_VERSION = 9

class DtaTensor(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("sb", ctypes.c_int64), ("st", ctypes.c_int64),
                ("sh", ctypes.c_int64), ("si", ctypes.c_int64)]


class SwigluArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("rows", ctypes.c_int64), ("n", ctypes.c_int64),
                ("a", ctypes.c_void_p), ("a_stride", ctypes.c_int64),
                ("b", ctypes.c_void_p), ("b_stride", ctypes.c_int64),
                ("out", ctypes.c_void_p), ("out_stride", ctypes.c_int64),
                ("dout", ctypes.c_void_p), ("dout_stride", ctypes.c_int64),
                ("da", ctypes.c_void_p), ("da_stride", ctypes.c_int64),
                ("db", ctypes.c_void_p), ("db_stride", ctypes.c_int64),
                ("dbias", ctypes.c_void_p), ("dbias_work", ctypes.c_void_p)]


class AttnFwdArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("T", ctypes.c_int32),
                ("H", ctypes.c_int32), ("n_terms", ctypes.c_int32), ("head_size", ctypes.c_int32),
                ("dv", ctypes.c_int32), ("scale", ctypes.c_float), ("dropout_p", ctypes.c_float),
                ("q", DtaTensor), ("k", DtaTensor), ("v", DtaTensor), ("o", DtaTensor),
                ("obr", DtaTensor), ("lse", ctypes.c_void_p), ("coef", ctypes.c_void_p),
                ("dropout_seed", ctypes.c_uint64), ("rope_freqs", ctypes.c_void_p), ("q_rot", DtaTensor),
                ("obr_dtype", ctypes.c_int32)]


class AttnBwdArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("T", ctypes.c_int32),
                ("H", ctypes.c_int32), ("n_terms", ctypes.c_int32), ("head_size", ctypes.c_int32),
                ("dv", ctypes.c_int32), ("scale", ctypes.c_float), ("dropout_p", ctypes.c_float),
                ("q", DtaTensor), ("k", DtaTensor), ("v", DtaTensor), ("obr", DtaTensor),
                ("lse", ctypes.c_void_p), ("coef", ctypes.c_void_p), ("dout", DtaTensor),
                ("dq", DtaTensor), ("dk", DtaTensor), ("dv_out", DtaTensor),
                ("dcoef", ctypes.c_void_p), ("delta", ctypes.c_void_p), ("dq_f32", ctypes.c_void_p),
                ("stages", ctypes.c_int32), ("rope_freqs", ctypes.c_void_p), ("dcoef_partial", ctypes.c_void_p),
                ("dropout_seed", ctypes.c_uint64), ("obr_dtype", ctypes.c_int32),
                ("group_max_dq", ctypes.c_int32), ("group_max_dkdv", ctypes.c_int32),
                ("dv_f32", ctypes.c_void_p), ("lse_c", ctypes.c_void_p)]


BWD_PRE, BWD_DQ, BWD_DKDV = 1, 2, 4


class LnArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("rows", ctypes.c_int64), ("C", ctypes.c_int64),
                ("eps", ctypes.c_float), ("out_scale", ctypes.c_float),
                ("x", ctypes.c_void_p), ("x_stride", ctypes.c_int64),
                ("y", ctypes.c_void_p), ("y_stride", ctypes.c_int64),
                ("w", ctypes.c_void_p), ("b", ctypes.c_void_p),
                ("mean", ctypes.c_void_p), ("rstd", ctypes.c_void_p),
                ("dy", ctypes.c_void_p), ("dy_stride", ctypes.c_int64),
                ("dx", ctypes.c_void_p), ("dx_stride", ctypes.c_int64),
                ("dw", ctypes.c_void_p), ("db", ctypes.c_void_p), ("partial", ctypes.c_void_p), ("io_dtype", ctypes.c_int32),
                ("res", ctypes.c_void_p), ("res_stride", ctypes.c_int64), ("xo", ctypes.c_void_p),
                ("xo_stride", ctypes.c_int64), ("dres", ctypes.c_void_p), ("dres_stride", ctypes.c_int64),
                ("dx16", ctypes.c_void_p), ("dx16_stride", ctypes.c_int64)]


class RopeArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("T", ctypes.c_int32),
                ("H", ctypes.c_int32), ("n_terms", ctypes.c_int32), ("head_size", ctypes.c_int32),
                ("inverse", ctypes.c_int32), ("src_f32", ctypes.c_int32),
                ("src", DtaTensor), ("dst", DtaTensor), ("freqs", ctypes.c_void_p)]


def _cache_op_fields(sizes, k: str, v: str, pointers):
    """The field list the decode and extend structs share: dtype .. dv, the op's own int32
    ``sizes``, scale, the four views (the cache's named ``k`` / ``v``), coef, the op's ``pointers``."""
    i32 = ("dtype", "B", "H", "n_terms", "head_size", "dv") + sizes
    return ([(n, ctypes.c_int32) for n in i32] + [("scale", ctypes.c_float)]
            + [(n, DtaTensor) for n in ("q", k, v, "o")]
            + [(n, ctypes.c_void_p) for n in ("coef",) + pointers])


_PAGED_FIELDS = [("page_size", ctypes.c_int32), ("max_pages", ctypes.c_int32), ("n_pages", ctypes.c_int32),
                 ("block_table_dev", ctypes.c_void_p)]
_DECODE_SIZES = ("length", "t_cap")


class DecodeArgs(ctypes.Structure):
    _fields_ = _cache_op_fields(_DECODE_SIZES, "k_cache", "v_cache", ("workspace", "length_dev"))


class ExtendArgs(ctypes.Structure):
    _fields_ = _cache_op_fields(("Tq", "pos", "t_cap"), "k_cache", "v_cache", ())


class DecodeRaggedArgs(ctypes.Structure):
    _fields_ = _cache_op_fields(_DECODE_SIZES, "k_cache", "v_cache", ("workspace", "lengths_dev"))


class ExtendRaggedArgs(ctypes.Structure):
    _fields_ = _cache_op_fields(("Tq", "t_cap"), "k_cache", "v_cache", ("pos_dev", "count_dev"))


class DecodePagedArgs(ctypes.Structure):
    _fields_ = _cache_op_fields(_DECODE_SIZES, "k_pool", "v_pool", ("workspace", "lengths_dev")) + _PAGED_FIELDS


class ExtendPagedArgs(ctypes.Structure):
    _fields_ = _cache_op_fields(("Tq", "t_cap"), "k_pool", "v_pool", ("pos_dev", "count_dev")) + _PAGED_FIELDS


class DecodePagedFp8Args(ctypes.Structure):
    _fields_ = DecodePagedArgs._fields_ + [("scale_pool_dev", ctypes.c_void_p), ("scale_page_stride", ctypes.c_int64)]


class ExtendPagedFp8Args(ctypes.Structure):
    _fields_ = ExtendPagedArgs._fields_ + [("scale_pool_dev", ctypes.c_void_p), ("scale_page_stride", ctypes.c_int64)]


class DecodeRowsArgs(ctypes.Structure):
    _fields_ = _cache_op_fields(("Tq", "t_cap"), "k_cache", "v_cache", ("workspace", "pos_dev", "count_dev"))


class DecodeRowsPagedArgs(ctypes.Structure):
    _fields_ = (_cache_op_fields(("Tq", "t_cap"), "k_pool", "v_pool", ("workspace", "pos_dev", "count_dev"))
                + _PAGED_FIELDS)


class DecodeRowsPagedFp8Args(ctypes.Structure):
    _fields_ = DecodeRowsPagedArgs._fields_ + [("scale_pool_dev", ctypes.c_void_p),
                                               ("scale_page_stride", ctypes.c_int64)]


# the shared-prefix plan, appended to the paged and the fp8 paged decode structs
_SHARED_FIELDS = [("n_groups", ctypes.c_int32), ("group_members_dev", ctypes.c_void_p),
                  ("group_rows_dev", ctypes.c_void_p)]


class DecodePagedSharedArgs(ctypes.Structure):
    _fields_ = DecodePagedArgs._fields_ + _SHARED_FIELDS


class DecodePagedSharedFp8Args(ctypes.Structure):
    _fields_ = DecodePagedFp8Args._fields_ + _SHARED_FIELDS


class KvQuantRowsArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("Tn", ctypes.c_int32), ("H", ctypes.c_int32),
                ("n_terms", ctypes.c_int32), ("head_size", ctypes.c_int32), ("dv", ctypes.c_int32),
                ("page_size", ctypes.c_int32), ("n_pages", ctypes.c_int32),
                ("k_new", DtaTensor), ("v_new", DtaTensor), ("k_pool", DtaTensor), ("v_pool", DtaTensor),
                ("scale_pool_dev", ctypes.c_void_p), ("scale_page_stride", ctypes.c_int64),
                ("slot_dev", ctypes.c_void_p)]


# dta_kv_step_dest
KV_STEP_CONTIGUOUS, KV_STEP_PAGED, KV_STEP_SLOTS = 0, 1, 2


class KvStepRowsArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("dtype", "B", "Tn", "H", "n_terms", "head_size", "dv", "t_cap", "dest",
                                               "page_size", "max_pages", "n_pages")]
                + [(n, DtaTensor) for n in ("q", "k", "v", "q_out", "k_dst", "v_dst")]
                + [(n, ctypes.c_void_p) for n in ("rope_freqs", "pos_dev", "count_dev", "block_table_dev",
                                                  "slots_out_dev")])


class SampleRowsArgs(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("R", ctypes.c_int32), ("V", ctypes.c_int32),
                ("logits", ctypes.c_void_p), ("row_stride", ctypes.c_int64),
                ("temperature", ctypes.c_float), ("top_k", ctypes.c_int32), ("top_p", ctypes.c_float),
                ("temperature_dev", ctypes.c_void_p), ("top_k_dev", ctypes.c_void_p), ("top_p_dev", ctypes.c_void_p),
                ("seed", ctypes.c_uint64), ("stream_dev", ctypes.c_void_p), ("offset_dev", ctypes.c_void_p),
                ("token_out", ctypes.c_void_p), ("logprob_out", ctypes.c_void_p)]


class PenalizeRowsArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("dtype", "B", "Tn", "V", "cap", "K")]
                + [("logits", ctypes.c_void_p), ("row_stride", ctypes.c_int64),
                   ("out", ctypes.c_void_p), ("out_stride", ctypes.c_int64),
                   ("hist", ctypes.c_void_p), ("hist_stride", ctypes.c_int64),
                   ("hlen_dev", ctypes.c_void_p), ("gen_start_dev", ctypes.c_void_p),
                   ("draft", ctypes.c_void_p), ("draft_stride", ctypes.c_int64), ("dcnt_dev", ctypes.c_void_p)]
                + [(n, ctypes.c_float) for n in ("repetition", "frequency", "presence", "floor_gap")]
                + [(n, ctypes.c_void_p) for n in ("repetition_dev", "frequency_dev", "presence_dev", "floor_gap_dev",
                                                  "bias")]
                + [("bias_stride", ctypes.c_int64), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)])


class SpecAcceptDraftArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("B", "Tn", "K", "cap", "t_cap", "ngram_min", "ngram_max", "eos_id")]
                + [(n, ctypes.c_int64) for n in ("hist_stride", "draft_stride", "tok_stride")]
                + [(n, ctypes.c_void_p) for n in ("hist", "hlen_dev", "remaining_dev", "draft", "dcnt_dev", "tok",
                                                  "result_out")])


class SpecFeedRowsArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("B", "K", "cap", "vocab", "total")]
                + [(n, ctypes.c_int64) for n in ("hist_stride", "draft_stride", "idx_stride", "offset_stride")]
                + [(n, ctypes.c_void_p) for n in ("hist", "hlen_dev", "remaining_dev", "draft", "dcnt_dev", "idx_out",
                                                  "counts_out", "offset_out")])


class SpecCommitLengthsArgs(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("B", "K", "t_cap", "n_slots")]
                + [(n, ctypes.c_void_p) for n in ("lengths", "result", "slots")])


_I32, _I64, _VP = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
_INT, _SIZE = ctypes.c_int, ctypes.c_size_t

# Every symbol include/diffattn.h declares, once: symbol -> (the argument struct of an
# ``(args*, stream)`` entry point, or the argtypes list; restype; feature group).  A group names
# entry points that arrived within ABI 9, each set "added the same way": an older library of the
# same ABI may lack them without being unusable, and their presence is the capability check.
_SYMBOLS = {
    "dta_attn_fwd": (AttnFwdArgs, _INT, None),
    "dta_attn_bwd": (AttnBwdArgs, _INT, None),
    "dta_attn_bwd_workspace_bytes": ([_I32] * 5, _SIZE, None),
    "dta_attn_bwd_dcoef_partial_bytes": ([_I32] * 4, _SIZE, None),
    "dta_ln_fwd": (LnArgs, _INT, None),
    "dta_ln_bwd": (LnArgs, _INT, None),
    "dta_ln_bwd_workspace_bytes": ([_I64] * 2, _SIZE, None),
    "dta_rope": (RopeArgs, _INT, None),
    "dta_cast_f32": ([_I32] * 6 + [_VP, DtaTensor, _VP], _INT, None),
    "dta_error_string": ([_INT], ctypes.c_char_p, None),
    "dta_abi_version": ([], _INT, None),
    "dta_supported": ([_I32] * 4, _INT, None),
    "dta_attn_decode": (DecodeArgs, _INT, None),
    "dta_attn_decode_workspace_bytes": ([_I32] * 6, _SIZE, None),
    "dta_swiglu_fwd": (SwigluArgs, _INT, None),
    "dta_swiglu_bwd": (SwigluArgs, _INT, None),
    "dta_accumulate_f32": ([_I32, _I64, _VP, _VP, _VP], _INT, None),
    "dta_swiglu_bwd_workspace_bytes": ([_I64, _I64], _SIZE, None),
    "dta_attn_bwd_dkdv_groups": ([_I32] * 5, _INT, None),
    "dta_attn_extend": (ExtendArgs, _INT, None),
    "dta_extend_supported": ([_I32] * 4, _INT, None),
    # ragged batches, then paged caches (block table over a pool of pages): no group, their tests need them
    "dta_attn_decode_ragged": (DecodeRaggedArgs, _INT, None),
    "dta_attn_extend_ragged": (ExtendRaggedArgs, _INT, None),
    "dta_attn_decode_paged": (DecodePagedArgs, _INT, None),
    "dta_attn_extend_paged": (ExtendPagedArgs, _INT, None),
    # fp8 (e4m3fn) pages with per-(row, head) scales (``ops.fp8_cache_supported``)
    "dta_attn_decode_paged_fp8": (DecodePagedFp8Args, _INT, "fp8"),
    "dta_kv_quant_rows": (KvQuantRowsArgs, _INT, "fp8"),
    # the multi-row step on fp8 pages (``ops.extend_fp8_supported``)
    "dta_attn_extend_paged_fp8": (ExtendPagedFp8Args, _INT, "fp8_extend"),
    "dta_extend_fp8_supported": ([_I32] * 4, _INT, "fp8_extend"),
    # the split-key decode for a step of 2 .. 8 rows (``ops.decode_rows_supported``)
    "dta_attn_decode_rows": (DecodeRowsArgs, _INT, "rows"),
    "dta_attn_decode_rows_paged": (DecodeRowsPagedArgs, _INT, "rows"),
    "dta_attn_decode_rows_paged_fp8": (DecodeRowsPagedFp8Args, _INT, "rows"),
    "dta_attn_decode_rows_workspace_bytes": ([_I32] * 7, _SIZE, "rows"),
    "dta_decode_rows_supported": ([_I32] * 6, _INT, "rows"),
    # the shared-prefix decode on the paged cache (``ops.decode_shared_supported``)
    "dta_attn_decode_paged_shared": (DecodePagedSharedArgs, _INT, "shared"),
    "dta_attn_decode_paged_shared_fp8": (DecodePagedSharedFp8Args, _INT, "shared"),
    "dta_decode_shared_supported": ([_I32] * 5, _INT, "shared"),
    # the fused row write of a ragged / paged step (``ops.kv_step_supported``)
    "dta_kv_step_rows": (KvStepRowsArgs, _INT, "step"),
    # seeded temperature / top-k / top-p sampling of logits rows (``ops.sample_supported``)
    "dta_sample_rows": (SampleRowsArgs, _INT, "sample"),
    # penalties, logit bias and the min-p floor of logits rows (``ops.penalize_rows_supported``)
    "dta_penalize_rows": (PenalizeRowsArgs, _INT, "penalty"),
    "dta_penalize_rows_workspace_bytes": ([_I64, _I32], _SIZE, "penalty"),
    # a speculative round's acceptance and next prompt-lookup draft (``ops.spec_supported``)
    "dta_spec_accept_draft": (SpecAcceptDraftArgs, _INT, "spec"),
    # the feed and the length commit of a fixed-shape (graph-replayed) round (``ops.spec_round_supported``)
    "dta_spec_feed_rows": (SpecFeedRowsArgs, _INT, "spec_round"),
    "dta_spec_commit_lengths": (SpecCommitLengthsArgs, _INT, "spec_round"),
}


EXPORTS = tuple(_SYMBOLS)
_GROUPS = {group: tuple(name for name, row in _SYMBOLS.items() if row[2] == group)
           for group in dict.fromkeys(row[2] for row in _SYMBOLS.values())}
FP8_EXPORTS = _GROUPS["fp8"]
FP8_EXTEND_EXPORTS = _GROUPS["fp8_extend"]
ROWS_EXPORTS = _GROUPS["rows"]
SHARED_EXPORTS = _GROUPS["shared"]
STEP_EXPORTS = _GROUPS["step"]
SAMPLE_EXPORTS = _GROUPS["sample"]
PENALTY_EXPORTS = _GROUPS["penalty"]
SPEC_EXPORTS = _GROUPS["spec"]
SPEC_ROUND_EXPORTS = _GROUPS["spec_round"]

_lock = threading.Lock()
_lib: Optional[ctypes.CDLL] = None


def _has(lib, names) -> bool:
    return all(hasattr(lib, name) for name in names)


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load (once) and type the library.  Raises if it is missing."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise RuntimeError(f"libdiffattn.so not found at {path}: run __graft_entry__.build() "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        lib = ctypes.CDLL(path)
        for group, names in _GROUPS.items():
            if group is not None and not _has(lib, names):
                continue                            # a feature group is typed only if the library has all of it
            for name in names:
                args, restype, _ = _SYMBOLS[name]
                fn = getattr(lib, name)
                fn.argtypes = args if isinstance(args, list) else [ctypes.POINTER(args), _VP]
                fn.restype = restype
        if lib.dta_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libdiffattn ABI {lib.dta_abi_version()} != expected {ABI_VERSION}")
        _lib = lib
        return lib


def fp8_symbols(lib) -> bool:
    """Whether ``lib`` exports the fp8-cache entry points (they arrived inside ABI 9)."""
    return _has(lib, FP8_EXPORTS)


def fp8_extend_symbols(lib) -> bool:
    """Whether ``lib`` exports the fp8 extend entry points (they arrived inside ABI 9, after the
    fp8-cache ones)."""
    return _has(lib, FP8_EXTEND_EXPORTS)


def rows_symbols(lib) -> bool:
    """Whether ``lib`` exports the multi-row split-key decode entry points (they arrived inside
    ABI 9, after the fp8 extend ones)."""
    return _has(lib, ROWS_EXPORTS)


def shared_symbols(lib) -> bool:
    """Whether ``lib`` exports the shared-prefix decode entry points (they arrived inside ABI 9,
    after the multi-row decode ones)."""
    return _has(lib, SHARED_EXPORTS)


def step_symbols(lib) -> bool:
    """Whether ``lib`` exports the fused row write of a ragged / paged step (it arrived inside ABI 9,
    after the shared-prefix decode)."""
    return _has(lib, STEP_EXPORTS)


def sample_symbols(lib) -> bool:
    """Whether ``lib`` exports the row sampler (it arrived inside ABI 9, after the fused row write)."""
    return _has(lib, SAMPLE_EXPORTS)


def penalty_symbols(lib) -> bool:
    """Whether ``lib`` exports the penalty row kernel (it arrived inside ABI 9, after the fixed-shape
    speculative round)."""
    return _has(lib, PENALTY_EXPORTS)


def spec_symbols(lib) -> bool:
    """Whether ``lib`` exports the speculative round's accept + draft kernel (it arrived inside ABI 9, after
    the row sampler)."""
    return _has(lib, SPEC_EXPORTS)


def spec_round_symbols(lib) -> bool:
    """Whether ``lib`` exports the feed and the length commit of the fixed-shape speculative round (they
    arrived inside ABI 9, after the accept + draft kernel)."""
    return _has(lib, SPEC_ROUND_EXPORTS)


def check(rc: int) -> None:
    if rc != 0:
        msg = load().dta_error_string(rc).decode()
        raise RuntimeError(f"libdiffattn: {msg} (code {rc})")


def dtype_code(t: torch.dtype) -> int:
    try:
        return _DTYPES[t]
    except KeyError:
        raise RuntimeError(f"libdiffattn supports bf16, fp16 and fp32 activations, got {t}") from None


def stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def tensor5(t: torch.Tensor) -> DtaTensor:
    """[b][t][h][i][d] (5-d) or [b][t][h][e] (4-d) view -> strides struct."""
    if t.dim() == 5:
        sb, st, sh, si, sd = t.stride()
    elif t.dim() == 4:
        sb, st, sh, sd = t.stride()
        si = 0
    else:
        raise ValueError("expected a 4-d or 5-d view")
    if sd != 1:
        raise RuntimeError("innermost dimension must be contiguous")
    return DtaTensor(t.data_ptr(), sb, st, sh, si)


def supported(dtype: torch.dtype, head_size: int, n_terms: int, dv: int) -> bool:
    return bool(load().dta_supported(dtype_code(dtype), head_size, n_terms, dv))
