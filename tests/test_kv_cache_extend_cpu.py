"""CPU checks of the multi-row KV-cache host logic: which model steps a chunked
prefill (``prefill_chunk``) and ``kv_cache.append_logits`` issue, their bounds, and
the length bookkeeping.  The model step is stubbed, so no kernel runs."""
import pytest
import torch

from differential_transformer_replication_amd import kv_cache


class _Model:
    block_size = 16


@pytest.fixture
def calls(monkeypatch):
    monkeypatch.setenv("DTA_DECODE_GRAPH", "0")
    out = []

    def step(model, idx, cache, pos, all_rows=False):
        out.append((idx.shape[1], pos))
        return torch.zeros(idx.shape[0], idx.shape[1], 3) if all_rows else torch.zeros(idx.shape[0], 3)

    monkeypatch.setattr(kv_cache, "_model_step", step)
    return out


def test_chunked_prefill_trace(calls):
    idx = torch.zeros(1, 7, dtype=torch.long)
    out = kv_cache.cached_generate(_Model(), idx, 4, prefill_chunk=3)
    assert out.shape == (1, 11)
    assert calls == [(3, 0), (3, 3), (1, 6), (1, 7), (1, 8), (1, 9)]


def test_default_trace_is_unchanged(calls):
    idx = torch.zeros(1, 7, dtype=torch.long)
    kv_cache.cached_generate(_Model(), idx, 4)
    assert calls == [(7, 0), (1, 7), (1, 8), (1, 9)]
    del calls[:]
    kv_cache.cached_generate(_Model(), idx, 4, prefill_chunk=None)
    assert calls == [(7, 0), (1, 7), (1, 8), (1, 9)]


def test_chunk_larger_than_prompt_is_one_prefill(calls):
    kv_cache.cached_generate(_Model(), torch.zeros(1, 7, dtype=torch.long), 2, prefill_chunk=64)
    assert calls == [(7, 0), (1, 7)]


def test_chunked_prefill_of_a_full_window_slides(calls):
    cache = kv_cache.KVCache()
    kv_cache.prefill_logits(_Model(), torch.zeros(1, 20, dtype=torch.long), cache, prefill_chunk=6)
    assert calls == [(6, 0), (6, 6), (4, 12)]            # the last block_size tokens
    assert cache.length == 0                             # a full window slides next step


def test_append_bookkeeping_then_decode(calls):
    cache = kv_cache.KVCache()
    model = _Model()
    idx = torch.zeros(2, 4, dtype=torch.long)
    kv_cache.last_logits(model, idx, cache)
    assert cache.length == 4
    last = kv_cache.append_logits(model, torch.zeros(2, 3, dtype=torch.long), cache)
    assert last.shape == (2, 3) and cache.length == 7
    kv_cache.last_logits(model, torch.zeros(2, 8, dtype=torch.long), cache)
    assert calls == [(4, 0), (3, 4), (1, 7)]
    rows = kv_cache.append_logits(model, torch.zeros(2, 2, dtype=torch.long), cache, all_rows=True)
    assert rows.shape == (2, 2, 3) and cache.length == 10
    kv_cache.append_logits(model, torch.zeros(2, 6, dtype=torch.long), cache)     # reaches block_size
    assert cache.length == 0


def test_append_bounds(calls):
    model = _Model()
    cache = kv_cache.KVCache()
    with pytest.raises(ValueError):
        kv_cache.append_logits(model, torch.zeros(1, 2, dtype=torch.long), cache)          # empty cache
    kv_cache.last_logits(model, torch.zeros(1, 10, dtype=torch.long), cache)
    with pytest.raises(ValueError):
        kv_cache.append_logits(model, torch.zeros(1, 7, dtype=torch.long), cache)          # 10 + 7 > 16
    cache.rows[1] = torch.zeros(1, 16, 8)
    with pytest.raises(ValueError):
        kv_cache.append_logits(model, torch.zeros(2, 2, dtype=torch.long), cache)          # batch 2 != 1
    assert cache.length == 10 and calls == [(10, 0)]
    with pytest.raises(ValueError):
        kv_cache.cached_generate(model, torch.zeros(1, 3, dtype=torch.long), 1, prefill_chunk=0)
    assert "append_logits" in kv_cache.__all__
