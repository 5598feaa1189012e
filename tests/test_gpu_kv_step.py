"""The fused row write of a ragged / paged step (``ops.kv_step_rows``, ``dta_kv_step_rows``).

The reference is the path it replaces: ``kv_cache._rope_rows_at`` (two ``ops.rope_rows``) and the
``index_put_`` of ``RaggedKVCache.write_rows`` / ``PagedKVCache.write_rows``, run on identical
inputs.  Everything is compared bit for bit (byte views, so NaN poison compares too): there is no
tolerance.  B 3, H 2, page size 32, t_cap 64, ``pos = [30, 0, 61]``, ``counts = [5, 0, 3]``: at
Tn = 5 sequence 0's rows straddle the page boundary at 32, sequence 1 writes nothing, and
sequence 2's padding rows lie past t_cap (positions 64, 65).  ``qkv`` is a slice of a wider
buffer.  Every destination starts as 0xFF bytes between guard bands (``_poison``): whatever the
call does not own -- the rows of no real row, the spare row, the spare page, the padding rows of
the K temporary -- must still be 0xFF afterwards."""
import pytest
import torch

from _poison import FILL, poisoned_allocations

from differential_transformer_replication_amd import kv_cache, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, P, CAP, NPG = 3, 2, 32, 64, 7
POS, COUNTS = (30, 0, 61), (5, 0, 3)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SIZES = [(16, 32), (40, 80), (64, 64)]
LAYER = 1


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _poison(shape, dtype):
    """A tensor of 0xFF bytes (not yet guarded: ``Session.guarded`` copies it between guard bands)."""
    n = torch.Size(shape).numel() * dtype.itemsize
    return torch.full((n,), FILL, dtype=torch.uint8, device=DEV).view(dtype).view(shape)


def _freqs(hs):
    ang = torch.outer(torch.arange(CAP, dtype=torch.float64),
                      10000.0 ** (-torch.arange(0, hs, 2, dtype=torch.float64) / hs))
    return torch.stack([ang.cos(), ang.sin()], dim=-1).to(torch.float32).to(DEV).contiguous()


def _case(dtype, N, hs, dv, Tn, rope):
    """(qkv, a strided slice of a wider buffer; the RoPE table or None; pos; counts; the block table)."""
    g = torch.Generator().manual_seed(1000 * N + 10 * hs + Tn)
    W = H * (2 * N * hs + dv)
    wide = torch.randn(B, Tn, W + 24, generator=g).to(dtype).to(DEV)
    qkv = wide[..., 8:8 + W]
    assert not qkv.is_contiguous()
    # sequence 1 caches nothing: its table row names no page
    tbl = torch.tensor([[5, 2], [-1, -1], [0, 6]], dtype=torch.int32, device=DEV)
    return qkv, (_freqs(hs) if rope else None), _i32(POS), _i32(COUNTS), tbl


def _today(qkv, freqs, pos, dims):
    """q and K_i as the eager step rotates them: (q the decode reads, k_rot or None)."""
    Hh, N, hs, dv = dims
    q, k_new, _ = ops.split_packed(qkv, Hh, N, hs, dv)
    if freqs is None:
        return q, None
    r = torch.arange(qkv.shape[1], device=DEV)
    rows = (pos[:, None].long() + r[None, :]).clamp_(max=CAP - 1)
    return kv_cache._rope_rows_at(q, k_new, freqs, rows)


def _real(Tn):
    return [(b, r) for b in range(B) for r in range(Tn) if r < COUNTS[b] and POS[b] + r < CAP]


CASES = [(Tn, N, rope) for Tn in (1, 5) for N in (1, 2, 3) for rope in (True, False)]


@pytest.mark.parametrize("hs,dv", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_contiguous_destination_bitwise(dtype, hs, dv):
    for Tn, N, rope in CASES:
        tag = (Tn, N, rope)
        dims = (H, N, hs, dv)
        nq = H * N * hs
        qkv, freqs, pos, counts, _ = _case(dtype, N, hs, dv, Tn, rope)
        q_ref, k_rot = _today(qkv, freqs, pos, dims)
        ref = kv_cache.RaggedKVCache()
        ref.store[LAYER] = _poison((B, CAP + 1, nq + H * dv), dtype)
        ref.rows[LAYER] = ref.store[LAYER][:, :CAP]
        ref.write_rows(LAYER, qkv, k_rot, dims, CAP, None, pos, counts)
        with poisoned_allocations() as s:
            store = s.guarded(_poison((B, CAP + 1, nq + H * dv), dtype), "store")
            buf = store[:, :CAP]
            dest = buf[..., :nq].unflatten(-1, (H, N, hs)), buf[..., nq:].unflatten(-1, (H, dv))
            q_rot, k_out, slots = ops.kv_step_rows(*ops.split_packed(qkv, *dims), pos, counts, CAP, freqs, dest=dest)
            s.check()                                   # the guard bands of the store and of q_rot
        assert k_out is None and slots is None
        if rope:
            assert torch.equal(_bytes(q_rot), _bytes(q_ref)), tag      # every row, padding rows included
        else:
            assert q_rot is None
        assert torch.equal(_bytes(store[:, :CAP]), _bytes(ref.store[LAYER][:, :CAP])), tag
        assert bool((_bytes(store[:, CAP]) == FILL).all()), tag         # the spare row: never touched
        # and only the real rows' destinations changed at all
        mask = torch.zeros(B, CAP + 1, dtype=torch.bool, device=DEV)
        for b, r in _real(Tn):
            mask[b, POS[b] + r] = True
        assert bool((_bytes(store)[~mask] == FILL).all()), tag
        assert not bool((_bytes(store)[mask] == FILL).all(dim=-1).any()), tag


@pytest.mark.parametrize("hs,dv", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_paged_destination_bitwise(dtype, hs, dv):
    for Tn, N, rope in CASES:
        tag = (Tn, N, rope)
        dims = (H, N, hs, dv)
        nq = H * N * hs
        qkv, freqs, pos, counts, tbl = _case(dtype, N, hs, dv, Tn, rope)
        q_ref, k_rot = _today(qkv, freqs, pos, dims)
        ref = kv_cache.PagedKVCache(NPG, P)
        ref.pool[LAYER] = _poison((NPG + 1, P, nq + H * dv), dtype)
        ref.write_rows(LAYER, qkv, k_rot, dims, CAP, tbl, pos, counts)
        with poisoned_allocations() as s:
            pool = s.guarded(_poison((NPG + 1, P, nq + H * dv), dtype), "pool")
            dest = pool[:NPG, :, :nq].unflatten(-1, (H, N, hs)), pool[:NPG, :, nq:].unflatten(-1, (H, dv))
            q_rot, k_out, slots = ops.kv_step_rows(*ops.split_packed(qkv, *dims), pos, counts, CAP, freqs, dest=dest,
                                                   block_table=tbl)
            s.check()
        assert k_out is None and slots is None
        if rope:
            assert torch.equal(_bytes(q_rot), _bytes(q_ref)), tag
        else:
            assert q_rot is None
        assert torch.equal(_bytes(pool[:NPG]), _bytes(ref.pool[LAYER][:NPG])), tag
        assert bool((_bytes(pool[NPG]) == FILL).all()), tag             # the spare page: never touched
        mask = torch.zeros(NPG + 1, P, dtype=torch.bool, device=DEV)
        for b, r in _real(Tn):
            at = POS[b] + r
            mask[int(tbl[b, at // P]), at % P] = True
        assert int(mask.sum()) == len(_real(Tn))
        assert bool((_bytes(pool)[~mask] == FILL).all()), tag
        assert not bool((_bytes(pool)[mask] == FILL).all(dim=-1).any()), tag


@pytest.mark.parametrize("hs,dv", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_form_bitwise(dtype, hs, dv, monkeypatch):
    """The fp8 form: the K temporary and the slots are what ``write_rows`` hands ``kv_quant_rows`` today,
    and the quantiser then leaves the same bytes and scales in every page of the pool (the spare page
    aside: it takes the padding rows, whose K the fused write leaves unwritten)."""
    quant = ops.kv_quant_rows
    seen = {}

    def recorder(k, v, k_all, v_all, s_all, slots):
        seen["k"], seen["slots"] = k, slots.clone()
        if hs % 16 == 0:                     # the quantiser's own shapes; head size 40 ends at the slots
            quant(k, v, k_all, v_all, s_all, slots)

    for Tn, N, rope in CASES:
        tag = (Tn, N, rope)
        dims = (H, N, hs, dv)
        nq = H * N * hs
        qkv, freqs, pos, counts, tbl = _case(dtype, N, hs, dv, Tn, rope)
        q_ref, k_rot = _today(qkv, freqs, pos, dims)
        _, k_new, v_new = ops.split_packed(qkv, *dims)
        ref = kv_cache.PagedKVCache(NPG, P, kv_dtype="fp8_e4m3")
        ref.pool[LAYER] = _poison((NPG + 1, P, nq + H * dv), torch.uint8)
        ref.scale_pool[LAYER] = _poison((NPG + 1, P, H * (N + 1)), torch.float32)
        monkeypatch.setattr(ops, "kv_quant_rows", recorder)
        ref.write_rows(LAYER, qkv, k_rot, dims, CAP, tbl, pos, counts)
        monkeypatch.setattr(ops, "kv_quant_rows", quant)
        with poisoned_allocations() as s:
            q_rot, k_out, slots = ops.kv_step_rows(*ops.split_packed(qkv, *dims), pos, counts, CAP, freqs, None, tbl,
                                                   P, NPG)
            s.check()                                   # the guard bands of q_rot, k_out and slots
        assert torch.equal(slots, seen["slots"]), tag
        assert bool((slots.view(B, Tn)[1] >= NPG * P).all())            # count 0: every slot in the spare page
        if rope:
            assert torch.equal(_bytes(q_rot), _bytes(q_ref)), tag
            real = torch.zeros(B, Tn, dtype=torch.bool, device=DEV)
            for b, r in _real(Tn):
                real[b, r] = True
            assert torch.equal(_bytes(k_out)[real], _bytes(k_rot)[real]), tag
            assert bool((_bytes(k_out)[~real] == FILL).all()), tag      # a padding row stores no K
        else:
            assert q_rot is None and k_out is None
        if hs % 16:
            continue
        pool = _poison((NPG + 1, P, nq + H * dv), torch.uint8)
        scales = _poison((NPG + 1, P, H * (N + 1)), torch.float32)
        ops.kv_quant_rows(k_new if k_out is None else k_out, v_new, pool[..., :nq].unflatten(-1, (H, N, hs)),
                          pool[..., nq:].unflatten(-1, (H, dv)), scales.unflatten(-1, (H, N + 1)), slots)
        assert torch.equal(pool[:NPG], ref.pool[LAYER][:NPG]), tag
        assert torch.equal(_bytes(scales[:NPG]), _bytes(ref.scale_pool[LAYER][:NPG])), tag


def test_device_values_are_clamped():
    """A position past the window and a page id outside the pool write nothing out of range: the
    first makes every row a padding row, the second lands in the last page of the pool."""
    dtype, N, hs, dv, Tn = torch.bfloat16, 2, 16, 32, 5
    dims = (H, N, hs, dv)
    nq = H * N * hs
    qkv, freqs, _, _, _ = _case(dtype, N, hs, dv, Tn, True)
    pos, counts = _i32([2 ** 31 - 1, -7, 3]), _i32([5, 5, 99])
    tbl = torch.tensor([[1, 1], [10 ** 6, 0], [-5, 0]], dtype=torch.int32, device=DEV)
    with poisoned_allocations() as s:
        pool = s.guarded(_poison((NPG + 1, P, nq + H * dv), dtype), "pool")
        dest = pool[:NPG, :, :nq].unflatten(-1, (H, N, hs)), pool[:NPG, :, nq:].unflatten(-1, (H, dv))
        ops.kv_step_rows(*ops.split_packed(qkv, *dims), pos, counts, CAP, freqs, dest=dest, block_table=tbl)
        s.check()
    written = ~(_bytes(pool) == FILL).all(dim=-1)
    want = torch.zeros(NPG + 1, P, dtype=torch.bool, device=DEV)
    want[NPG - 1, 0:5] = True                 # sequence 1: pos -7 -> 0, page id 10^6 -> the pool's last page
    want[0, 3:8] = True                       # sequence 2: page id -5 -> page 0; counts 99 is at most Tn rows
    assert torch.equal(written, want)


def test_contract():
    dtype = torch.bfloat16
    qkv, freqs, pos, counts, tbl = _case(dtype, 2, 16, 32, 1, True)
    q, k, v = ops.split_packed(qkv, H, 2, 16, 32)
    assert ops.kv_step_supported() is True
    cache = torch.zeros(B, CAP, H * (2 * 16 + 32), device=DEV, dtype=dtype)
    dest = cache[..., :64].unflatten(-1, (H, 2, 16)), cache[..., 64:].unflatten(-1, (H, 32))
    with pytest.raises(RuntimeError):                       # the whole table, not a slice of it
        ops.kv_step_rows(q, k, v, pos, counts, CAP, freqs[:8], dest=dest)
    with pytest.raises(RuntimeError):
        ops.kv_step_rows(q, k, v, pos.long(), counts, CAP, freqs, dest=dest)
    with pytest.raises(RuntimeError):                       # cache views of another capacity
        ops.kv_step_rows(q, k, v, pos, counts, CAP - 1, None, dest=dest)
    with pytest.raises(RuntimeError):                       # the fp8 form needs the pool's geometry
        ops.kv_step_rows(q, k, v, pos, counts, CAP, freqs, None, tbl)
    with pytest.raises(RuntimeError):                       # a table that does not reach t_cap
        ops.kv_step_rows(q, k, v, pos, counts, CAP, freqs, None, tbl[:, :1].contiguous(), P, NPG)
    # head size 12: not a multiple of 8 -- the library refuses, nothing falls back
    q12 = torch.zeros(B, 1, H, 2, 12, device=DEV, dtype=dtype)
    v12 = torch.zeros(B, 1, H, 24, device=DEV, dtype=dtype)
    d12 = torch.zeros(B, CAP, H, 2, 12, device=DEV, dtype=dtype), torch.zeros(B, CAP, H, 24, device=DEV, dtype=dtype)
    with pytest.raises(RuntimeError):
        ops.kv_step_rows(q12, q12, v12, pos, counts, CAP, None, dest=d12)
