"""Workspace sizes of the C ABI, pinned (host-only queries).

Callers and the poison tests size buffers from ``dta_ln_bwd_workspace_bytes`` and
``dta_attn_decode_workspace_bytes``, so the figures are ABI: a cleanup inside the kernels must not
move them.  The LayerNorm figure is (blocks + 32) * 2 * C floats with blocks = min(ceil(rows / 8),
512); the 32 further rows served the two-launch reduce that the one-launch reduce replaced, and
stay in the figure although no kernel touches them.  The constants were read from the library
built before that reduce was deleted."""
import pytest

from differential_transformer_replication_amd import _lib

LN_BWD = {(1, 8): 2112, (9, 2048): 557056, (4096, 2048): 8912896, (5000, 8192): 35651584}
# (B, H, n_terms, head_size, dv, t_cap): a split plan, and the single-pass plan at a long cache
DECODE = {(2, 4, 2, 64, 128, 769): 49216, (8, 16, 3, 16, 32, 32768): 50331648}


@pytest.mark.parametrize("rows,C", list(LN_BWD))
def test_ln_bwd_workspace_bytes(rows, C):
    assert _lib.load().dta_ln_bwd_workspace_bytes(rows, C) == LN_BWD[(rows, C)]


@pytest.mark.parametrize("shape", list(DECODE))
def test_attn_decode_workspace_bytes(shape):
    assert _lib.load().dta_attn_decode_workspace_bytes(*shape) == DECODE[shape]
