"""Which N-branch attention plans the built library runs natively, pinned (host-only queries).

``dta_supported`` answers 1 for every branch count that can run at all: natively, or as branch
groups over smaller plans -- different kernels, and slower.  If ``Plan<E, HS, N, DV>::ok``
(csrc/attn_kernels.h) turns false for a built configuration, through an LDS or register limit
say, nothing else notices.  ``dta_attn_bwd_dkdv_groups(dtype, hs, N, dv, N) == 1`` holds exactly
when the N-branch plan is native, so the inventory is pinned here; ``test_gpu_plan_matrix.py``
runs every entry.  A new ``X(...)`` entry of ``DTA_FOR_CONFIGS`` has to be added to the list."""
import pytest

from differential_transformer_replication_amd import _lib

# DTA_FOR_CONFIGS of csrc/attn_kernels.h, restated: (head size, branches, value width)
CONFIGS = [
    (16, 1, 32), (16, 2, 32), (16, 3, 32), (16, 4, 32), (32, 1, 64), (32, 2, 64), (32, 3, 64), (32, 4, 64),
    (64, 1, 128), (64, 2, 128), (64, 3, 128), (64, 4, 128), (128, 1, 256), (128, 2, 256), (128, 3, 256),
    (128, 4, 256), (64, 1, 64), (128, 1, 128), (32, 1, 32),
    (96, 1, 192), (96, 2, 192), (96, 3, 192), (96, 4, 192), (96, 1, 96),
    (256, 1, 512), (256, 2, 512), (256, 1, 256),
]
# fp32 lacks N = 3 / 4 at head sizes 96 / 128 (attn_kernels.h: "Any branch count N >= 2 whose
# N-branch plan is not built (N >= 5, fp32 N = 3 / 4 at head sizes 96 / 128)" runs branch-split
# with a grouped backward) and the differential plans at head size 256 ("Head size 256 (16-bit
# diff plans; fp32 only the control's dv = hs one fits)").
F32_ABSENT = [(96, 3, 192), (96, 4, 192), (128, 3, 256), (128, 4, 256), (256, 1, 512), (256, 2, 512)]
NATIVE = {
    _lib.DTA_BF16: CONFIGS,
    _lib.DTA_F16: CONFIGS,
    _lib.DTA_F32: [c for c in CONFIGS if c not in F32_ABSENT],
}


def _native(lib, dt, hs, n, dv):
    return lib.dta_attn_bwd_dkdv_groups(dt, hs, n, dv, n) == 1


def test_config_list_is_the_headers():
    assert len(CONFIGS) == 27 and len(set(CONFIGS)) == 27 and len(NATIVE[_lib.DTA_F32]) == 21


@pytest.mark.parametrize("dt", [_lib.DTA_BF16, _lib.DTA_F16, _lib.DTA_F32], ids=["bf16", "fp16", "fp32"])
def test_native_plan_inventory(dt):
    lib = _lib.load()
    missing = [c for c in NATIVE[dt] if not _native(lib, dt, *c)]
    assert not missing, f"plans that dropped to branch groups (Plan::ok false): {missing}"
    # nothing else is native: every head size up to 512 in steps of 8, N = 1..8, dv = hs or 2 hs
    found = [(hs, n, dv) for hs in range(8, 513, 8) for n in range(1, 9) for dv in (hs, 2 * hs)
             if _native(lib, dt, hs, n, dv)]
    extra = sorted(set(found) - set(NATIVE[dt]))
    assert not extra, f"native plans missing from this test's list: {extra}"
    # a native plan answers dta_supported, and so does every branch count above the built ones
    for hs, n, dv in NATIVE[dt]:
        assert lib.dta_supported(dt, hs, n, dv) == 1
