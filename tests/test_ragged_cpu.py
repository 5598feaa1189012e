"""CPU checks of the ragged-batch path: ``_lib.DecodeRaggedArgs`` / ``ExtendRaggedArgs``
lay out ``dta_attn_decode_ragged_args`` / ``dta_attn_extend_ragged_args`` exactly as
include/diffattn.h does (the gcc sizeof / offsetof probe of test_abi_layout.py), the
built library exports both entry points and still reports ABI 9, and the host
bookkeeping of ``kv_cache``'s ragged functions (lengths, bounds, truncate, the frozen
length of a finished sequence) with the model step stubbed, so no kernel runs."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

from differential_transformer_replication_amd import _lib, kv_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "dta_attn_decode_ragged_args": _lib.DecodeRaggedArgs,
    "dta_attn_extend_ragged_args": _lib.ExtendRaggedArgs,
}


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_ragged_args_match_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "diffattn.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'  printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines += ['  printf("abi version %d\\n", DTA_ABI_VERSION);', "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        exe = os.path.join(d, "probe")
        with open(src, "w") as fh:
            fh.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    assert got[("abi", "version")] == _lib.ABI_VERSION == 9         # the feature arrives without an ABI bump
    bad = []
    for cname, py in STRUCTS.items():
        if got[(cname, "sizeof")] != ctypes.sizeof(py):
            bad.append((cname, "sizeof", got[(cname, "sizeof")], ctypes.sizeof(py)))
        for f in py._fields_:
            off = getattr(py, f[0]).offset
            if got[(cname, f[0])] != off:
                bad.append((cname, f[0], got[(cname, f[0])], off))
    assert not bad, bad
    # the one-length structs keep their layout: the ragged decode args differ from them by the
    # meaning of the last pointer only
    assert [f[0] for f in _lib.DecodeRaggedArgs._fields_][:-1] == [f[0] for f in _lib.DecodeArgs._fields_][:-1]
    assert ctypes.sizeof(_lib.DecodeRaggedArgs) == ctypes.sizeof(_lib.DecodeArgs)


def test_built_library_exports_the_ragged_entry_points():
    lib = _lib.load()
    assert lib.dta_abi_version() == 9
    for name in ("dta_attn_decode_ragged", "dta_attn_extend_ragged"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # argument validation needs no device: a null struct or a null lengths / pos array is invalid
    assert lib.dta_attn_decode_ragged(None, None) == -1
    assert lib.dta_attn_extend_ragged(None, None) == -1
    assert lib.dta_attn_decode_ragged(ctypes.byref(_lib.DecodeRaggedArgs()), None) == -1
    assert lib.dta_attn_extend_ragged(ctypes.byref(_lib.ExtendRaggedArgs()), None) == -1


# ------------------------------------------------------------- bookkeeping ---
class _Model:
    block_size = 16


@pytest.fixture
def calls(monkeypatch):
    out = []

    def step(model, idx, cache, pos, counts, gather=None, one_row=False):
        out.append((tuple(idx.shape), None if pos is None else pos.tolist(),
                    None if counts is None else counts.tolist(), None if gather is None else gather.tolist(),
                    one_row))
        if gather is None:
            return torch.zeros(idx.shape[0], idx.shape[1], 3)
        return torch.zeros(idx.shape[0], 3)

    monkeypatch.setattr(kv_cache, "_ragged_model_step", step)
    return out


def _prompts(*lens):
    return [torch.arange(n, dtype=torch.long) % 5 for n in lens]


def test_lengths_after_prefill_decode_and_append(calls):
    model, cache = _Model(), kv_cache.RaggedKVCache()
    logits = kv_cache.prefill_ragged(model, _prompts(3, 7, 5), cache)
    assert logits.shape == (3, 3)
    assert calls == [((3, 7), None, None, [2, 6, 4], False)]          # right-padded, gathered at len - 1
    assert cache.host_lengths == [3, 7, 5] and cache.lengths.tolist() == [3, 7, 5]
    assert cache.lengths.dtype == torch.int32

    logits = kv_cache.decode_ragged(model, torch.zeros(3, 1, dtype=torch.long), cache)
    assert logits.shape == (3, 3)
    assert calls[-1] == ((3, 1), [3, 7, 5], [1, 1, 1], None, True)
    assert cache.host_lengths == [4, 8, 6] and cache.lengths.tolist() == [4, 8, 6] and cache.host_exact

    rows = kv_cache.append_ragged(model, torch.zeros(3, 4, dtype=torch.long), [4, 0, 2], cache, all_rows=True)
    assert rows.shape == (3, 4, 3)
    assert calls[-1] == ((3, 4), [4, 8, 6], [4, 0, 2], None, False)
    assert cache.host_lengths == [8, 8, 8] and cache.lengths.tolist() == [8, 8, 8]

    last = kv_cache.append_ragged(model, torch.zeros(3, 2, dtype=torch.long), torch.tensor([1, 2, 0]), cache)
    assert last.shape == (3, 3)
    assert calls[-1] == ((3, 2), [8, 8, 8], [1, 2, 0], [0, 1, 0], False)     # each sequence's last real row
    assert cache.host_lengths == [9, 10, 8] and cache.lengths.tolist() == [9, 10, 8]
    assert len(calls) == 4


def test_append_near_block_size_runs_narrower_steps(calls):
    """pos[b] + Tq must fit the window for every sequence that still has real rows."""
    model, cache = _Model(), kv_cache.RaggedKVCache()
    kv_cache.prefill_ragged(model, _prompts(14, 2), cache)
    del calls[:]
    rows = kv_cache.append_ragged(model, torch.zeros(2, 5, dtype=torch.long), [2, 5], cache, all_rows=True)
    assert rows.shape == (2, 5, 3)
    assert calls == [((2, 2), [14, 2], [2, 2], None, False), ((2, 3), [16, 4], [0, 3], None, False)]
    assert cache.host_lengths == [16, 7] and cache.lengths.tolist() == [16, 7]


def test_block_size_errors(calls):
    model, cache = _Model(), kv_cache.RaggedKVCache()
    with pytest.raises(ValueError):
        kv_cache.prefill_ragged(model, _prompts(3, 17), cache)               # longer than block_size
    with pytest.raises(ValueError):
        kv_cache.prefill_ragged(model, [torch.zeros(0, dtype=torch.long)], cache)
    with pytest.raises(ValueError):
        kv_cache.prefill_ragged(model, [torch.zeros(2, 2, dtype=torch.long)], cache)
    with pytest.raises(ValueError):
        kv_cache.decode_ragged(model, torch.zeros(2, 1, dtype=torch.long), cache)    # not prefilled
    with pytest.raises(ValueError):
        kv_cache.append_ragged(model, torch.zeros(2, 1, dtype=torch.long), [1, 1], kv_cache.KVCache())
    kv_cache.prefill_ragged(model, _prompts(15, 4), cache)
    n = len(calls)
    with pytest.raises(ValueError):
        kv_cache.append_ragged(model, torch.zeros(2, 3, dtype=torch.long), [2, 3], cache)    # 15 + 2 > 16
    with pytest.raises(ValueError):
        kv_cache.append_ragged(model, torch.zeros(2, 3, dtype=torch.long), [0, 4], cache)    # count > Tn
    with pytest.raises(ValueError):
        kv_cache.append_ragged(model, torch.zeros(2, 3, dtype=torch.long), [0, -1], cache)
    with pytest.raises(ValueError):
        kv_cache.append_ragged(model, torch.zeros(3, 3, dtype=torch.long), [0, 1, 1], cache)  # batch 3 != 2
    kv_cache.append_ragged(model, torch.zeros(2, 3, dtype=torch.long), [1, 3], cache)        # 16 and 7: fits (two steps)
    assert cache.host_lengths == [16, 7]
    with pytest.raises(ValueError):
        kv_cache.decode_ragged(model, torch.zeros(2, 1, dtype=torch.long), cache)            # 16 + 1 > 16
    assert cache.host_lengths == [16, 7] and len(calls) == n + 2
    with pytest.raises(ValueError):
        kv_cache.generate_ragged(model, _prompts(3, 10), 7)                                   # 10 + 7 > 16
    assert len(calls) == n + 2
    for name in ("RaggedKVCache", "prefill_ragged", "decode_ragged", "append_ragged", "generate_ragged"):
        assert name in kv_cache.__all__


def test_truncate_validation(calls):
    model, cache = _Model(), kv_cache.RaggedKVCache()
    with pytest.raises(ValueError):
        cache.truncate([1])                                   # nothing cached
    kv_cache.prefill_ragged(model, _prompts(3, 7, 5), cache)
    kv_cache.append_ragged(model, torch.zeros(3, 4, dtype=torch.long), [4, 4, 4], cache)
    assert cache.host_lengths == [7, 11, 9]
    for bad in ([8, 11, 9], [7, -1, 9], [7, 11], [7, 11, 9, 1]):
        with pytest.raises(ValueError):
            cache.truncate(bad)
        assert cache.host_lengths == [7, 11, 9] and cache.lengths.tolist() == [7, 11, 9]
    cache.truncate([7, 8, 5])                                 # accepted 4, 1 and 0 of the 4 rows
    assert cache.host_lengths == [7, 8, 5] and cache.lengths.tolist() == [7, 8, 5]
    cache.truncate(torch.tensor([0, 8, 5]))
    assert cache.lengths.tolist() == [0, 8, 5] and cache.lengths.dtype == torch.int32
    kv_cache.decode_ragged(model, torch.zeros(3, 1, dtype=torch.long), cache)
    assert calls[-1][1] == [0, 8, 5] and cache.host_lengths == [1, 9, 6]


def test_finished_sequence_keeps_its_length(calls, monkeypatch):
    model, cache = _Model(), kv_cache.RaggedKVCache()
    kv_cache.prefill_ragged(model, _prompts(3, 7), cache)
    kv_cache.decode_ragged(model, torch.zeros(2, 1, dtype=torch.long), cache, active=torch.tensor([True, False]))
    assert calls[-1] == ((2, 1), [3, 7], [1, 0], None, True)
    assert cache.lengths.tolist() == [4, 7]
    assert not cache.host_exact and cache.host_lengths == [4, 8]          # an upper bound until sync()
    assert cache.sync() == [4, 7] and cache.host_exact

    # generate_ragged: sequence 0 samples eos_id = 2 at its second token and stops there
    samples = iter([[1, 1], [2, 3], [4, 3], [2, 2]])
    monkeypatch.setattr(torch, "multinomial", lambda probs, num_samples: torch.tensor(next(samples))[:, None])
    del calls[:]
    out = kv_cache.generate_ragged(model, _prompts(3, 7), 4, eos_id=2)
    assert [o.tolist() for o in out] == [[0, 1, 2, 1, 2], [0, 1, 2, 3, 4, 0, 1, 1, 3, 3, 2]]
    # prefill, then three decode steps; from the second on sequence 0 is inactive and its length frozen
    assert [c[1] for c in calls] == [None, [3, 7], [4, 8], [4, 9]]
    assert [c[2] for c in calls] == [None, [1, 1], [0, 1], [0, 1]]
    out = kv_cache.generate_ragged(model, _prompts(3, 7), 0)
    assert [o.tolist() for o in out] == [[0, 1, 2], [0, 1, 2, 3, 4, 0, 1]]
