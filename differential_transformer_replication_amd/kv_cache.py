"""Incremental decoding for ``generate``.

The reference's ``generate`` (diff_transformer.py:177-185; the same loop in
Ndiff_transformer.py and control.py:163-171) runs a full forward over
``idx[:, -block_size:]`` for every new token and keeps only the last row of
logits.  Here the first call runs the
prompt once through the fused training kernels (prefill) and keeps every
layer's K_i / V rows in a KV cache; each further token costs one projection row
per layer and one ``dta_attn_decode`` launch (``ops.diff_attention_decode``)
instead of a T x T recompute.

Positions are absolute within the window (learned position table in
DiffTransformer, RoPE rows in AlternatingDiffTransformer and the control
StandardTransformer, which runs as N = 1 with dv = hs), so once the sequence
outgrows ``block_size`` the window slides, every cached row changes position,
and the step falls back to the reference's own full recompute of the cropped
window.  Sampling (softmax of the last logits, ``torch.multinomial``) is the
reference's, so with the same generator state the tokens match the
full-recompute path whenever the logits agree to sampling precision.
``DTA_KV_CACHE=0`` selects the full-recompute loop.  Decode steps replay one
captured HIP graph of the whole model step (the position lives on the device,
``dta_attn_decode`` reads its length there); ``DTA_DECODE_GRAPH=0`` launches
them eagerly instead.

Between the prefill and the one-token step sits the multi-row step: several new
positions at once against the live cache (``append_logits``: a second chat turn,
a tool result, the scoring of candidate tokens with ``all_rows=True``), through
``ops.diff_attention_extend``, which writes nothing but its output.  The same step
prefills a long prompt in bounded memory (``prefill_chunk``): the first chunk runs
the fused training forward, every further chunk appends.

Everything above keeps the whole batch at one position (``KVCache.length``).  Two further
caches keep one length per sequence on the device; they run eagerly unless made with ``graph=True``
(``SeqDecodeGraph``: the one-token step as one replayed HIP graph), stay within one
window, and no existing path enters them.  ``RaggedKVCache`` (``prefill_ragged``,
``decode_ragged``, ``append_ragged``, ``generate_ragged``) has the same contiguous rows:
prompts of different lengths generate as one batch, a verification step accepts a different
number of tokens per sequence (``truncate`` rolls the rest back).  ``PagedKVCache``
(``prefill_paged``, ``decode_paged``, ``append_paged``, ``generate_paged``) keeps the rows in a
shared pool of fixed-size pages behind a per-sequence block table, with a host allocator:
``release`` hands a finished sequence's pages to the next prompt, ``fork`` shares a prompt's
pages among its continuations (copy on write); ``kv_dtype="fp8_e4m3"`` stores e4m3fn bytes
with one fp32 scale per (row, head, K_i | V), and with ``fp8_extend=True`` a multi-row step on
those pages is one ``ops.diff_attention_extend_paged_fp8`` launch per layer; with ``shared_decode=True`` the
one-token step reads the pages forked sequences still share once per group (``shared_groups``).  Both run one step (``_seq_model_step``,
``_seq_attention_step``); the cache says where the new rows go (``write_rows``) and which op
reads them back (``decode_rows``, ``extend_rows``); with ``fused_step=True`` the RoPE and the scatter of a step's
rows are one ``ops.kv_step_rows`` launch (``step_rows``).

Every generate loop takes ``sampler=None``: a ``Sampler`` (temperature, top-k, top-p, seed) replaces the
reference's two sampling lines by one ``ops.sample_rows`` launch per step whose draw for a sequence depends
on (seed, the sequence's stream, its position) only; None keeps the reference's lines, token for token.

``generate_ragged`` / ``generate_paged`` also take ``speculate=None``: a ``Speculation`` makes every model step
a round that scores the pending token and up to k drafted ones (``append_*(all_rows=True)``), samples every
row with the offsets the plain loop would use, and lets ``ops.spec_accept_draft`` accept, append and draft
again on the device (``_speculative_tokens``).  The tokens are the ``sampler`` loop's, token for token.
``Speculation(graph=True)`` makes every round the same K + 1 rows per sequence and replays it as one captured
HIP graph (``SpecRound``): ``ops.spec_feed_rows`` builds its inputs and ``ops.spec_commit_lengths`` rolls the
lengths back on the device, so the host only grows pages before the replay and reads the round's result after.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence

import torch
from torch.nn import functional as F

from . import ops
from ._compat import mha_out_scale

__all__ = ["KVCache", "DecodeGraph", "DevicePosition", "cached_generate", "enabled", "append_logits",
           "prefill_logits", "check_prefill_chunk", "RaggedKVCache", "prefill_ragged", "decode_ragged",
           "append_ragged", "generate_ragged", "PagedKVCache", "OutOfPages", "prefill_paged", "decode_paged",
           "append_paged", "generate_paged", "SeqDecodeGraph", "Sampler", "Speculation", "SpecRound", "Penalties"]


class Sampler:
    """Opt-in sampling controls of the generate loops: ``temperature`` (``<= 0``: greedy), ``top_k``
    (``<= 0``: off), ``top_p`` (``>= 1``: off) and ``seed``.  One ``ops.sample_rows`` launch per step
    draws sequence s's t-th token from Philox(seed, stream=s, offset=t) alone, so its samples do not
    depend on what else is in the batch.  Immutable; ``sampler=None`` everywhere keeps the
    reference's softmax + ``torch.multinomial``."""
    __slots__ = ("temperature", "top_k", "top_p", "seed")

    def __init__(self, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0):
        if temperature != temperature or top_p != top_p:
            raise ValueError("temperature and top_p must not be NaN")
        for name, v in (("temperature", float(temperature)), ("top_k", int(top_k)), ("top_p", float(top_p)),
                        ("seed", int(seed))):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a Sampler is immutable")

    def __repr__(self):
        return f"Sampler(temperature={self.temperature}, top_k={self.top_k}, top_p={self.top_p}, seed={self.seed})"

    def sample(self, logits: torch.Tensor, step: int, streams: Optional[torch.Tensor] = None,
               return_logprobs: bool = False):
        """The ``step``-th token of every row of ``logits`` (B, V): (B, 1) int64 (and the (B,) logprobs).
        ``streams``: int64 (B,) stream ids, default the row index.  The offsets are filled on the
        device: no host sync, and the same values under a graph-replayed step."""
        offset = torch.full((logits.shape[0],), step, dtype=torch.int64, device=logits.device)
        out = ops.sample_rows(logits, self.temperature, self.top_k, self.top_p, self.seed, streams, offset,
                              return_logprobs)
        return (out[0][:, None], out[1]) if return_logprobs else out[:, None]


class Penalties:
    """Opt-in logit processing of the generate loops, applied before the ``Sampler`` in one
    ``ops.penalize_rows`` launch per step (include/diffattn.h, "Sampling penalties"): ``repetition`` (> 0;
    1: off) divides the positive and multiplies the other logits of every token the sequence holds, prompt
    included; ``frequency`` times a token's count among the generated tokens and ``presence`` once are
    subtracted; ``logit_bias`` -- a ``{token: float}`` dict or a (V,) tensor -- is added and ``banned`` tokens
    get ``-inf``; ``min_p`` in [0, 1) removes what is less probable than ``min_p`` times the most probable token
    (after the temperature; off at temperature <= 0).  The history a row is penalised with is its own
    sequence's, so a sequence's tokens still do not depend on the batch, and a speculative round penalises
    row j with the j drafted tokens before it: ``speculate`` emits the same tokens.  Immutable."""
    __slots__ = ("repetition", "presence", "frequency", "min_p", "logit_bias", "banned")

    def __init__(self, repetition: float = 1.0, presence: float = 0.0, frequency: float = 0.0, min_p: float = 0.0,
                 logit_bias=None, banned=()):
        repetition, presence, frequency, min_p = float(repetition), float(presence), float(frequency), float(min_p)
        inf = float("inf")
        if not 0 < repetition < inf:
            raise ValueError(f"repetition {repetition} must be positive and finite")
        if not (-inf < presence < inf and -inf < frequency < inf):
            raise ValueError("presence and frequency must be finite")
        if not 0 <= min_p < 1:
            raise ValueError(f"min_p {min_p} outside [0, 1)")
        if isinstance(logit_bias, dict):
            logit_bias = {int(t): float(v) for t, v in logit_bias.items()}
            if any(t < 0 or v != v or v == inf for t, v in logit_bias.items()):
                raise ValueError("logit_bias maps token ids >= 0 to values that are neither NaN nor +inf")
        elif isinstance(logit_bias, torch.Tensor):
            if logit_bias.dim() != 1 or not logit_bias.is_floating_point() or bool(torch.isnan(logit_bias).any()) \
                    or bool((logit_bias == inf).any()):
                raise ValueError("a logit_bias tensor is (V,), floating point, without NaN or +inf")
            logit_bias = logit_bias.detach().clone()
        elif logit_bias is not None:
            raise ValueError("logit_bias must be a {token: float} dict or a (V,) tensor")
        banned = tuple(sorted({int(t) for t in banned}))
        if any(t < 0 for t in banned):
            raise ValueError("banned token ids must be >= 0")
        for name, v in (("repetition", repetition), ("presence", presence), ("frequency", frequency), ("min_p", min_p),
                        ("logit_bias", logit_bias), ("banned", banned)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a Penalties is immutable")

    def __repr__(self):
        return (f"Penalties(repetition={self.repetition}, presence={self.presence}, frequency={self.frequency}, "
                f"min_p={self.min_p}, logit_bias={'None' if self.logit_bias is None else '...'}, banned={self.banned})")

    def bias_row(self, V: int, device) -> Optional[torch.Tensor]:
        """The fp32 (V,) bias row of a call -- ``logit_bias`` with ``-inf`` at the banned tokens -- or None."""
        if self.logit_bias is None and not self.banned:
            return None
        row = torch.zeros(V, dtype=torch.float32)
        if isinstance(self.logit_bias, torch.Tensor):
            if self.logit_bias.shape[0] != V:
                raise ValueError(f"the logit_bias tensor has {self.logit_bias.shape[0]} entries, the vocabulary {V}")
            row = self.logit_bias.to("cpu", torch.float32).clone()
        ids = list(self.logit_bias) if isinstance(self.logit_bias, dict) else []
        if any(t >= V for t in ids + list(self.banned)):
            raise ValueError(f"a logit_bias or banned token id is outside the vocabulary of {V}")
        for t in ids:
            row[t] = self.logit_bias[t]
        if self.banned:
            row[list(self.banned)] = float("-inf")
        if bool((row == float("-inf")).all()):
            raise ValueError("logit_bias and banned leave no token")
        return row.to(device)

    def floor_gap(self, temperature: float) -> Optional[float]:
        """``T * ln(min_p)`` in double, rounded to fp32; None where min-p is off."""
        if self.min_p <= 0 or not temperature > 0:
            return None
        return torch.tensor(temperature * math.log(self.min_p), dtype=torch.float64).to(torch.float32).item()


class _PenaltyState:
    """What a generate loop holds on the device to penalise its rows: the int32 token histories (B, cap),
    their lengths, the prompt lengths and the call's bias row.  ``apply`` is the loop's one
    ``ops.penalize_rows`` launch; ``append`` adds a step's tokens with no host sync."""

    def __init__(self, penalties: Penalties, sampler: "Sampler", V: int, device, hist, hlen, gen_start):
        self.pen, self.hist, self.hlen, self.gen_start = penalties, hist, hlen, gen_start
        self.bias = penalties.bias_row(V, device)
        self.gap = penalties.floor_gap(sampler.temperature)

    @classmethod
    def from_prompts(cls, penalties, sampler, V: int, device, prompts, max_new_tokens: int):
        lens = [int(p.shape[0]) for p in prompts]
        hist = torch.zeros(len(prompts), max(lens) + max_new_tokens, dtype=torch.int32, device=device)
        hist[:, :max(lens)] = torch.nn.utils.rnn.pad_sequence(list(prompts), batch_first=True).to(device, torch.int32)
        lens = torch.tensor(lens, dtype=torch.int32, device=device)
        return cls(penalties, sampler, V, device, hist, lens.clone(), lens)

    def apply(self, logits, draft=None, dcnt=None, rows_per_seq: int = 1):
        p = self.pen
        return ops.penalize_rows(logits, self.hist, self.hlen, self.gen_start, draft, dcnt, p.repetition, p.presence,
                                 p.frequency, self.gap, self.bias, rows_per_seq)

    def append(self, tok) -> None:
        self.hist.scatter_(1, self.hlen.long()[:, None], tok.to(torch.int32))
        self.hlen += 1


def _check_penalties(penalties, sampler) -> None:
    if not isinstance(penalties, Penalties):
        raise ValueError("penalties must be a Penalties")
    if sampler is None:
        raise ValueError("penalties need a sampler: they are applied in front of ops.sample_rows, not of the "
                         "reference's softmax + torch.multinomial")


class Speculation:
    """Opt-in speculative decoding of ``generate_ragged`` / ``generate_paged`` by prompt lookup: each round
    verifies up to ``k`` (1 .. 7) drafted tokens in one multi-row step.  The draft is the continuation of the
    longest (``ngram_max`` .. ``ngram_min`` tokens, at most 8), then latest, earlier occurrence of the
    sequence's last tokens in its own history; it is deterministic, so accepting a draft iff it equals the
    token sampled at its position -- with the uniform the plain loop would draw there -- emits exactly the
    plain ``sampler`` loop's tokens, whatever is drafted.  ``drafter``: an object whose
    ``propose(hist, hlen, remaining, k) -> (draft, dcnt)`` replaces the lookup (device tensors: int32
    (B, cap) histories, their lengths, the tokens still owed; returns an integer (B, k) draft and its (B,)
    lengths, which the loop clips to what the window and ``remaining`` allow).  Immutable; ``stats`` holds
    the counts of the last call: ``rounds`` (model steps), ``drafted`` and ``accepted`` draft tokens,
    ``emitted`` tokens.  ``graph=True`` (default False: the eager round, as it was): every round runs k + 1
    rows per sequence and is one replay of a HIP graph captured once per call (``SpecRound``); same tokens,
    same ``stats``.  It needs ``ops.spec_round_supported()`` on the GPU -- ``RuntimeError`` otherwise, there
    is no fallback -- and a round whose padded rows would pass ``block_size`` runs eagerly."""
    __slots__ = ("k", "ngram_max", "ngram_min", "drafter", "stats", "graph")

    def __init__(self, k: int = 4, ngram_max: int = 3, ngram_min: int = 1, drafter=None, graph: bool = False):
        k, ngram_max, ngram_min = int(k), int(ngram_max), int(ngram_min)
        if not 1 <= k <= ops.SPEC_MAX_K:
            raise ValueError(f"k {k} outside 1 .. {ops.SPEC_MAX_K}")
        if not 1 <= ngram_min <= ngram_max <= ops.SPEC_MAX_NGRAM:
            raise ValueError(f"need 1 <= ngram_min {ngram_min} <= ngram_max {ngram_max} <= {ops.SPEC_MAX_NGRAM}")
        if drafter is not None and not callable(getattr(drafter, "propose", None)):
            raise ValueError("drafter must have propose(hist, hlen, remaining, k) -> (draft, dcnt)")
        for name, v in (("k", k), ("ngram_max", ngram_max), ("ngram_min", ngram_min), ("drafter", drafter),
                        ("stats", dict(rounds=0, drafted=0, accepted=0, emitted=0)), ("graph", bool(graph))):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a Speculation is immutable")

    def __repr__(self):
        return (f"Speculation(k={self.k}, ngram_max={self.ngram_max}, ngram_min={self.ngram_min}, "
                f"drafter={self.drafter!r}" + (", graph=True)" if self.graph else ")"))


def _stream_ids(streams, B: int, n_samples: int, device) -> Optional[torch.Tensor]:
    """int64 (B * n_samples,) stream ids: ``streams[b] * n_samples + sample`` (None: the row index)."""
    if streams is None:
        return None
    if len(streams) != B:
        raise ValueError(f"streams must give one id per prompt ({B}), got {len(streams)}")
    return torch.tensor([int(s) * n_samples + j for s in streams for j in range(n_samples)], dtype=torch.int64,
                        device=device)


def enabled(idx: torch.Tensor, model=None) -> bool:
    if not idx.is_cuda or os.environ.get("DTA_KV_CACHE", "1") == "0":
        return False
    if model is not None:
        # the prefill runs on the fused kernels (ops.diff_attention: any built or padded head
        # size, any branch count); the decode kernel takes head sizes % 8 up to 128, N <= 4
        _, _, N, hs, dv, _ = _spec(model.blocks[0])
        return (ops.attention_supported(model.lm_head.weight.dtype, hs, N, dv) and N <= 4 and hs % 8 == 0
                and hs <= 128)
    return True


class KVCache:
    """Per-layer packed rows ``[K (H, N, hs) | V (H, dv)]`` of every cached position:
    (B, block_size, H*N*hs + H*dv) in the projection's dtype, allocated once."""

    def __init__(self):
        self.rows: Dict[int, torch.Tensor] = {}
        self.length = 0
        # parameters do not change inside generate(): the packed projection weight,
        # the branch coefficients and the RoPE table are built once per layer
        self.consts: Dict[int, tuple] = {}
        self.graph = None
        self.use_graph = os.environ.get("DTA_DECODE_GRAPH", "1") != "0"
        self.kv_dtype = None                       # rows in the projection's dtype (PagedKVCache may differ)
        self.fp8_extend = False                    # PagedKVCache: the multi-row step of an fp8 pool is one extend launch
        self.rows_decode = False                   # ragged / paged: a step of 2 .. 8 rows is one split-key decode launch
        self.shared_decode = False                 # PagedKVCache: the one-token step reads forked pages once per group
        self.shared_plan = None                    # the running decode_paged step's ops.SharedDecodePlan, else None
        self.fused_step = False                    # ragged / paged: a step's RoPE and row scatter are one ops.kv_step_rows
        self.graphs: Dict[tuple, "SeqDecodeGraph"] = {}    # ragged / paged with graph=True: one per (B, mask given)

    def layer(self, layer: int, B: int, cap: int, width: int, like: torch.Tensor) -> torch.Tensor:
        buf = self.rows.get(layer)
        if buf is None or buf.shape != (B, cap, width) or buf.dtype != like.dtype:
            buf = torch.empty(B, cap, width, device=like.device, dtype=like.dtype)
            self.rows[layer] = buf
        return buf


def _spec(block):
    """(attention module, H, N, hs, dv, block_size) of a Block: the differential
    MHAs (dv = 2hs), or control.py's standard MHA as N = 1, dv = hs."""
    if hasattr(block, "diff_attn"):
        a = block.diff_attn
        return a, a.num_heads, getattr(a, "n_terms", 2), a.head_size, 2 * a.head_size, a.block_size
    a = block.attn
    return a, a.num_heads, 1, a.head_size, a.head_size, a.heads[0].block_size


def _constants(cache: KVCache, attn, layer: int, H: int, hs: int, bs: int, x: torch.Tensor):
    """(packed projection weight, branch coefficients, RoPE table or None) of a layer,
    built on ``x``'s device on first use and kept in ``cache.consts``."""
    consts = cache.consts.get(layer)
    if consts is None:
        device = x.device
        freqs = None
        if hasattr(attn.heads[0], "freqs_cis"):
            from .Ndiff_transformer import rope_table
            freqs = rope_table(attn.heads[0].freqs_cis, bs, hs).to(device=device, dtype=torch.float32).contiguous()
        weight = attn.packed_weight()
        if hasattr(attn, "coefficients"):
            coef = attn.coefficients(layer)
        else:   # control.py MultiHeadAttention: packed [Q | K | V], one branch of weight 1
            coef = torch.ones(H, 1, device=device, dtype=torch.float32)
        consts = cache.consts[layer] = (weight, coef, freqs)
    return consts


def _attention_step(block, x: torch.Tensor, layer: int, cache: KVCache, pos: int) -> torch.Tensor:
    """The block's attention forward (MultiHead(Alternating)DiffAttention, or
    control.py's MultiHeadAttention) for the rows at positions pos .. pos+Tn-1,
    reading and extending the layer's cache."""
    attn, H, N, hs, dv, bs = _spec(block)
    weight, coef, freqs = _constants(cache, attn, layer, H, hs, bs, x)
    rope = freqs is not None
    qkv = F.linear(x, weight)
    B, Tn, W = qkv.shape
    nq = H * N * hs
    buf = cache.layer(layer, B, bs, W - nq, qkv)
    k_rows = buf[..., :nq].unflatten(-1, (H, N, hs))
    if pos == 0:
        # prefill: the prompt through the training kernels, then cache its K_i / V rows
        out = ops.diff_attention(qkv, coef, H, N, hs, None if freqs is None else freqs[:Tn], dv)
        src = qkv[..., nq:2 * nq].unflatten(-1, (H, N, hs))
        if rope:
            ops.rope_rows(src, k_rows[:, :Tn], freqs[:Tn])
        else:
            k_rows[:, :Tn].copy_(src)
        buf[:, :Tn, nq:].copy_(qkv[..., 2 * nq:])
    elif not isinstance(pos, DevicePosition) and Tn != 1:
        out = _extend_rows(qkv, buf, coef, freqs, H, N, hs, dv, pos)
    else:
        if Tn != 1:
            raise RuntimeError("graph decode steps take one new position at a time")
        dev = isinstance(pos, DevicePosition)
        q = qkv[:, :, :nq].unflatten(-1, (H, N, hs))               # (B, 1, H, N, hs)
        k_new = qkv[:, :, nq:2 * nq].unflatten(-1, (H, N, hs))
        v_new = qkv[:, :, 2 * nq:].unflatten(-1, (H, dv))
        v_rows = buf[..., nq:].unflatten(-1, (H, dv))
        if rope:
            tab = freqs.index_select(0, pos.idx) if dev else freqs[pos:pos + 1]
            q_rot, k_rot = torch.empty_like(q), torch.empty_like(k_new)
            ops.rope_rows(q, q_rot, tab)
            ops.rope_rows(k_new, k_rot, tab)
            q, k_new = q_rot, k_rot
        if dev:                                   # graph-replayable: position read on the device
            k_rows.index_copy_(1, pos.idx, k_new)
            v_rows.index_copy_(1, pos.idx, v_new)
            out = ops.diff_attention_decode(q[:, 0], k_rows, v_rows, coef, bs, pos.length)
        else:
            k_rows[:, pos:pos + 1].copy_(k_new)
            v_rows[:, pos:pos + 1].copy_(v_new)
            out = ops.diff_attention_decode(q[:, 0], k_rows, v_rows, coef, pos + 1)
        out = out.view(B, 1, H * dv)
    return _attention_tail(attn, out)


def _attention_tail(attn, out: torch.Tensor) -> torch.Tensor:
    """What follows the heads' concatenated output: the differential MHAs' GroupLayerNorm
    with its constant scale, the output projection, dropout."""
    if hasattr(attn, "group_norm"):
        gn = attn.group_norm
        out = ops.group_ln_scale(out, gn.weight, gn.bias, gn.eps, mha_out_scale(attn.lambda_init))
    return attn.dropout(attn.proj(out))


def _decode_per_row(decode, Tn: int, pos, counts=None) -> torch.Tensor:
    """The multi-row step of a head size without an extend plan (40, 72: not a multiple of
    16), or of an fp8 pool: ``decode(i, lengths)`` once per row i -- correct, but the cache
    is read once per row.  ``pos``: a host integer, every row real; or with ``counts`` device
    int32 (B,), a padding row decoding at length 0 (zeros)."""
    if counts is None:
        return torch.stack([decode(i, pos + i + 1) for i in range(Tn)], dim=1)
    zero = torch.zeros_like(pos)
    return torch.stack([decode(i, torch.where(counts > i, pos + (i + 1), zero)) for i in range(Tn)], dim=1)


def _rope_rows_at(q, k_new, freqs, rows):
    """``q`` and ``k_new`` (B, Tn, H, N, hs) rotated to the positions ``rows`` (B, Tn), into
    temporaries: one table row per (b, r), so the views collapse to (1, B*Tn, ...)."""
    B, Tn, H, N, hs = q.shape
    tab = freqs[rows.flatten()]
    q_rot = torch.empty(B, Tn, H, N, hs, device=q.device, dtype=q.dtype)
    k_rot = torch.empty_like(q_rot)
    ops.rope_rows(q.reshape(1, B * Tn, H, N, hs), q_rot.view(1, B * Tn, H, N, hs), tab)
    ops.rope_rows(k_new.reshape(1, B * Tn, H, N, hs), k_rot.view(1, B * Tn, H, N, hs), tab)
    return q_rot, k_rot


def _extend_rows(qkv, buf, coef, freqs, H: int, N: int, hs: int, dv: int, pos: int) -> torch.Tensor:
    """Attention of the Tn new rows at positions pos .. pos+Tn-1 (pos > 0, host
    integer): their K_i / V rows go into the cache first, then one
    ``diff_attention_extend`` launch, or ``_decode_per_row`` where it has no plan."""
    B, Tn, _ = qkv.shape
    nq = H * N * hs
    q = qkv[:, :, :nq].unflatten(-1, (H, N, hs))
    k_new = qkv[:, :, nq:2 * nq].unflatten(-1, (H, N, hs))
    k_rows = buf[..., :nq].unflatten(-1, (H, N, hs))
    v_rows = buf[..., nq:].unflatten(-1, (H, dv))
    if freqs is not None:
        tab = freqs[pos:pos + Tn]
        q_rot = torch.empty_like(q)
        ops.rope_rows(q, q_rot, tab)
        ops.rope_rows(k_new, k_rows[:, pos:pos + Tn], tab)
        q = q_rot
    else:
        k_rows[:, pos:pos + Tn].copy_(k_new)
    buf[:, pos:pos + Tn, nq:].copy_(qkv[..., 2 * nq:])
    if ops.extend_supported(qkv.dtype, hs, N, dv):
        return ops.diff_attention_extend(q, k_rows, v_rows, coef, pos)
    return _decode_per_row(lambda i, n: ops.diff_attention_decode(q[:, i], k_rows, v_rows, coef, n), Tn, pos)


class DevicePosition:
    """The decode position held on the device (index and index + 1), so one
    captured graph replays for every position."""

    def __init__(self, device):
        self.idx = torch.zeros(1, dtype=torch.long, device=device)
        self.length = torch.ones(1, dtype=torch.int32, device=device)

    def set(self, p: int) -> None:
        self.idx.fill_(p)
        self.length.fill_(p + 1)


class DecodeGraph:
    """One decode step (every layer, Tn = 1) captured as a HIP graph: per token the
    host issues two fills and one graph launch instead of ~15 launches per layer."""

    def __init__(self, model, cache: "KVCache", B: int, device):
        self.tok = torch.zeros(B, 1, dtype=torch.long, device=device)
        self.pos = DevicePosition(device)
        # warm-up (allocator, cached constants) writes cache row block_size-1 only,
        # which is rewritten before it is ever read
        self.pos.set(model.block_size - 1)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            _model_step(model, self.tok, cache, self.pos)
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.logits = _model_step(model, self.tok, cache, self.pos)

    def step(self, tok: torch.Tensor, p: int) -> torch.Tensor:
        self.tok.copy_(tok)
        self.pos.set(p)
        self.graph.replay()
        return self.logits.clone()


class SeqDecodeGraph:
    """``DecodeGraph`` for the caches with per-sequence lengths: the one-token step of ``decode_ragged``
    or ``decode_paged`` for a batch of B, captured once and replayed for every token.  The static
    inputs are ``tok`` (B, 1) long, ``counts`` (B,) int32 (1, or the step's ``active`` mask) and, paged,
    ``slots`` (B,) long: which rows of ``cache.block_table`` / ``cache.lengths`` the step's sequences
    are, so any subset or order of B live sequences replays the same graph.  Captured: the paged
    gather of the table rows and lengths, ``_seq_model_step(..., one_row=True)`` and the length update
    (ragged: ``lengths.add_(counts)`` in place).  The decode launch sizes its grid from the capacity,
    and every length, position and page id is read on the device, so one graph serves every length.
    Page growth and copy on write stay on the host, before the replay (``decode_paged``).

    The graph holds the cache's pools (or rows), ``block_table``, ``lengths`` and the per-layer
    constants of ``cache.consts`` by address: they exist before the capture (any prefill makes them)
    and are only ever updated in place.  As for ``DecodeGraph`` the model's parameters are assumed
    fixed while the graph lives.  Warm-up and capture run with ``counts = 0``: an all-inactive step
    caches nothing and moves no length, so neither changes the cache's content.  One stream only:
    the graph has no parallel branches."""

    def __init__(self, model, cache: "KVCache", B: int, device, slots: Optional[torch.Tensor] = None):
        self.paged = slots is not None
        if not (cache.pool if self.paged else cache.rows) or cache.lengths is None:
            raise ValueError("a decode graph needs a prefilled cache: its pools are made by the first prefill")
        self.model, self.cache = model, cache
        self.tok = torch.zeros(B, 1, dtype=torch.long, device=device)
        self.counts = torch.zeros(B, dtype=torch.int32, device=device)
        self.slots = slots.clone() if self.paged else None
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            self._step()
        torch.cuda.current_stream(device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.logits = self._step()

    def _step(self) -> torch.Tensor:
        cache = self.cache
        if self.paged:
            tbl = cache.block_table.index_select(0, self.slots)
            pos = cache.lengths.index_select(0, self.slots)
            logits = _paged_model_step(self.model, self.tok, cache, tbl, pos, self.counts, one_row=True)[:, 0]
            cache.lengths.index_copy_(0, self.slots, pos + self.counts)
        else:
            logits = _ragged_model_step(self.model, self.tok, cache, cache.lengths, self.counts, one_row=True)[:, 0]
            cache.lengths.add_(self.counts)
        return logits

    def step(self, tok: torch.Tensor, counts: torch.Tensor, slots: Optional[torch.Tensor] = None) -> torch.Tensor:
        self.tok.copy_(tok)
        self.counts.copy_(counts)
        if self.paged:
            self.slots.copy_(slots)
        self.graph.replay()
        return self.logits.clone()


def _seq_graph(model, cache, B: int, masked: bool, device, slots: Optional[torch.Tensor] = None) -> SeqDecodeGraph:
    """The cache's graph for a batch of B (one per (B, mask given or not)), captured on first use."""
    g = cache.graphs.get((B, masked))
    if g is None:
        g = cache.graphs[(B, masked)] = SeqDecodeGraph(model, cache, B, device, slots)
    return g


class SpecRound:
    """``SeqDecodeGraph`` for a speculative round (``Speculation(graph=True)``): the round of
    ``_speculative_tokens`` at a fixed shape, K + 1 rows per sequence, captured once per call of
    ``generate_ragged`` / ``generate_paged`` and replayed for every round.  It holds by address the loop's
    state (``hist``, ``hlen``, ``remaining``, ``draft``, ``dcnt``, ``result``), its static buffers (``idx``
    (B, K + 1) long, ``counts`` (B,) int32, ``offset`` (B, K + 1) long, ``stream`` the (B * (K + 1),) stream
    ids, ``tok`` the round's samples) and, paged, ``slots`` (B,) long: the rows of ``cache.block_table`` /
    ``cache.lengths`` of the call's sequences.  The body, in order: ``ops.spec_feed_rows``; paged, the gather
    of the table rows and lengths; ``_ragged_model_step`` / ``_paged_model_step`` over the (B, K + 1) tokens
    (reached by their module names at call time; the lengths are not advanced); ``ops.sample_rows`` of all
    B * (K + 1) rows with the sampler's scalars and the device ``stream`` / ``offset``; ``ops.spec_accept_draft``
    with ``Tn = K + 1``; ``ops.spec_commit_lengths``, the only writer of the lengths.  No host value shapes
    it.  Page growth and copy on write stay on the host, before the replay; a ``drafter`` proposes after it.

    A fixed ``Tn = K + 1`` gives the (m, dcnt), history and drafts of the eager round's ``Tn = max(dcnt) + 1``:
    in the header's accept rule ``a <= dcnt <= Tn - 1`` either way, so ``min(a + 1, remaining, Tn, cap - hlen)``
    never takes its ``Tn`` term, and the rows past ``dcnt`` -- padding here -- are never looked at.

    On a CUDA device the body is warmed up on a side stream and captured on one stream (no parallel
    branches).  The warm-up runs for real, so it is made inert: ``remaining`` is saved and zeroed for warm-up
    and capture, every sequence is then not live (``counts = 0``, ``m = 0``: nothing is cached, accepted or
    moved), and it is restored after.  The graph holds the cache's pools (or rows), ``block_table``,
    ``lengths`` and ``cache.consts`` by address, as ``SeqDecodeGraph`` does.  On CPU tensors the same body
    runs uncaptured, through the ops' references."""

    def __init__(self, model, cache: "KVCache", sampler: Sampler, spec: Speculation, state, total: int, vocab: int,
                 eos: int, stream: torch.Tensor, slots: Optional[torch.Tensor] = None):
        self.hist, self.hlen, self.remaining, self.draft, self.dcnt, self.result = state
        dev = self.hist.device
        if dev.type == "cuda" and not (ops.spec_round_supported() and ops.spec_supported()):
            raise RuntimeError("Speculation(graph=True) needs dta_spec_feed_rows, dta_spec_commit_lengths and "
                               "dta_spec_accept_draft, which this libdiffattn.so does not export "
                               "(ops.spec_round_supported); there is no fallback")
        if cache.lengths is None:
            raise ValueError("a speculative round needs a prefilled cache")
        self.model, self.cache, self.sampler, self.spec = model, cache, sampler, spec
        self.total, self.vocab, self.eos, self.bs = int(total), int(vocab), int(eos), model.block_size
        B, K = self.hist.shape[0], spec.k
        self.paged = slots is not None
        self.slots = slots.clone() if self.paged else None
        self.idx = torch.zeros(B, K + 1, dtype=torch.long, device=dev)
        self.counts = torch.zeros(B, dtype=torch.int32, device=dev)
        self.offset = torch.zeros(B, K + 1, dtype=torch.long, device=dev)
        self.stream = stream[:, None].expand(B, K + 1).reshape(-1).contiguous()
        self.tok = None
        self.graph = None
        if dev.type != "cuda":
            return
        owed = self.remaining.clone()
        self.remaining.zero_()                     # inert: no sequence is live
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body()
        self.remaining.copy_(owed)

    def _body(self) -> None:
        cache, spec, smp, K = self.cache, self.spec, self.sampler, self.spec.k
        B = self.hist.shape[0]
        ops.spec_feed_rows(self.hist, self.hlen, self.remaining, self.draft, self.dcnt, K, self.vocab, self.total,
                           self.idx, self.counts, self.offset)
        if self.paged:
            tbl = cache.block_table.index_select(0, self.slots)
            pos = cache.lengths.index_select(0, self.slots)
            rows = _paged_model_step(self.model, self.idx, cache, tbl, pos, self.counts)
        else:
            rows = _ragged_model_step(self.model, self.idx, cache, cache.lengths, self.counts)
        self.tok = ops.sample_rows(rows, smp.temperature, smp.top_k, smp.top_p, smp.seed, self.stream,
                                   self.offset.reshape(-1)).reshape(B, K + 1)
        ops.spec_accept_draft(self.hist, self.hlen, self.remaining, self.draft, self.dcnt, self.tok, self.eos, K,
                              spec.ngram_min if spec.drafter is None else 0, spec.ngram_max, self.bs, self.result)
        ops.spec_commit_lengths(cache.lengths, self.result, K, self.bs, self.slots)

    def run(self) -> None:
        """One round on the state as it stands: a replay, or on CPU tensors the body itself."""
        if self.graph is None:
            self._body()
        else:
            self.graph.replay()


def _model_step(model, idx: torch.Tensor, cache: KVCache, pos: int, all_rows: bool = False) -> torch.Tensor:
    """The model's forward (diff_transformer.py:154-175 / Ndiff_transformer.py) over
    positions pos .. pos+T-1 of the window; returns the last row of logits (B, vocab),
    or with ``all_rows`` every row's (B, T, vocab)."""
    T = idx.shape[1]
    x = model.token_embedding_table(idx)
    if hasattr(model, "position_embedding_table"):
        rows = pos.idx if isinstance(pos, DevicePosition) else torch.arange(pos, pos + T, device=idx.device)
        x = x + model.position_embedding_table(rows)
    for layer, block in enumerate(model.blocks, 1):
        x = x + _attention_step(block, block.ln1(x), layer, cache, pos)
        x = x + block.ffwd(block.ln2(x))
    if all_rows:
        return model.lm_head(model.ln_f(x))
    return model.lm_head(model.ln_f(x[:, -1:]))[:, -1]


def last_logits(model, idx: torch.Tensor, cache: KVCache) -> torch.Tensor:
    """Logits of the newest position of ``idx``, reusing ``cache`` when the window
    has not slid (exposed for the parity tests)."""
    bs = model.block_size
    if cache.length == 0 or idx.shape[1] > bs or idx.shape[1] != cache.length + 1:
        cond = idx[:, -bs:]
        cache.length = 0
        logits = _model_step(model, cond, cache, 0)
        cache.length = cond.shape[1] if idx.shape[1] < bs else 0    # a full window slides next step
        return logits
    if cache.use_graph:
        if cache.graph is None:
            cache.graph = DecodeGraph(model, cache, idx.shape[0], idx.device)
        logits = cache.graph.step(idx[:, -1:], cache.length)
    else:
        logits = _model_step(model, idx[:, -1:], cache, cache.length)
    cache.length += 1
    if cache.length >= bs:
        cache.length = 0
    return logits


def append_logits(model, new_idx: torch.Tensor, cache: KVCache, all_rows: bool = False) -> torch.Tensor:
    """Feed ``new_idx`` (B, Tn >= 1) as the tokens at positions ``cache.length ..
    cache.length+Tn-1`` of a live cache (one multi-row step per layer instead of a
    re-prefill of the whole window) and advance ``cache.length``.  Returns the last
    row's logits (B, vocab), or with ``all_rows`` the logits of all Tn rows
    (B, Tn, vocab): row r is the distribution of the token after ``new_idx[:, r]``,
    which scores a continuation or verifies speculated tokens in one step.

    Positions are absolute within the window, so an append cannot cross
    ``block_size``: the slide would move every cached row, and the caller re-prefills
    through ``last_logits``.  ``last_logits`` continues single-token decode afterwards
    (same cache buffers, so a captured decode graph stays valid)."""
    if new_idx.dim() != 2 or new_idx.shape[1] < 1:
        raise ValueError("new_idx must be (B, Tn) with Tn >= 1")
    Tn, bs = new_idx.shape[1], model.block_size
    if cache.length == 0:
        raise ValueError("append_logits needs a prefilled cache: run last_logits on the prompt first")
    if cache.length + Tn > bs:
        raise ValueError(f"appending {Tn} tokens at length {cache.length} crosses block_size {bs}: "
                         "re-prefill the slid window through last_logits")
    for buf in cache.rows.values():
        if buf.shape[0] != new_idx.shape[0]:
            raise ValueError(f"batch size {new_idx.shape[0]} differs from the cache's {buf.shape[0]}")
    logits = _model_step(model, new_idx, cache, cache.length, all_rows=all_rows)
    cache.length += Tn
    if cache.length >= bs:
        cache.length = 0                      # a full window slides next step
    return logits


def check_prefill_chunk(prefill_chunk) -> None:
    if prefill_chunk is not None and prefill_chunk < 1:
        raise ValueError(f"prefill_chunk must be >= 1, got {prefill_chunk}")


def prefill_logits(model, idx: torch.Tensor, cache: KVCache, prefill_chunk=None) -> torch.Tensor:
    """Prefill ``cache`` with the window of ``idx`` and return its newest position's
    logits.  ``prefill_chunk = C``: the first min(C, T) tokens run the fused training
    forward (which saves its backward tensors), the rest go in chunks of at most C
    through ``append_logits``, so no step holds more than C rows of activations.
    ``None``: ``last_logits``'s one-shot prefill."""
    check_prefill_chunk(prefill_chunk)
    cache.length = 0
    if prefill_chunk is None:
        return last_logits(model, idx, cache)
    cond = idx[:, -model.block_size:]
    T = cond.shape[1]
    first = min(prefill_chunk, T)
    logits = _model_step(model, cond[:, :first], cache, 0)
    cache.length = first if first < model.block_size else 0
    for s in range(first, T, prefill_chunk):
        logits = append_logits(model, cond[:, s:s + prefill_chunk], cache)
    return logits


@torch.no_grad()
def cached_generate(model, idx: torch.Tensor, max_new_tokens: int, prefill_chunk=None,
                    sampler: Optional[Sampler] = None, penalties: Optional[Penalties] = None) -> torch.Tensor:
    check_prefill_chunk(prefill_chunk)
    if penalties is not None:
        _check_penalties(penalties, sampler)
    cache = KVCache()
    state = None
    for step in range(max_new_tokens):
        if prefill_chunk is not None and (cache.length == 0 or idx.shape[1] != cache.length + 1):
            logits = prefill_logits(model, idx, cache, prefill_chunk)
        else:
            logits = last_logits(model, idx, cache)
        if penalties is not None:
            if state is None:
                state = _PenaltyState.from_prompts(penalties, sampler, logits.shape[-1], logits.device, list(idx),
                                                   max_new_tokens)
            tok = sampler.sample(state.apply(logits), step)
            state.append(tok)
            idx = torch.cat((idx, tok), dim=1)
            continue
        if sampler is not None:
            idx = torch.cat((idx, sampler.sample(logits, step)), dim=1)
            continue
        probs = F.softmax(logits, dim=-1)
        idx = torch.cat((idx, torch.multinomial(probs, num_samples=1)), dim=1)
    return idx


@torch.no_grad()
def naive_generate(model, idx: torch.Tensor, max_new_tokens: int, sampler: Sampler,
                   penalties: Optional[Penalties] = None) -> torch.Tensor:
    """The models' full-recompute ``generate`` loop with a ``Sampler`` in place of softmax + multinomial
    (and, with ``penalties``, one ``ops.penalize_rows`` launch in front of it)."""
    state = None
    if penalties is not None:
        _check_penalties(penalties, sampler)
    for step in range(max_new_tokens):
        logits, _ = model(idx[:, -model.block_size:])
        logits = logits[:, -1, :]
        if penalties is not None:
            if state is None:
                state = _PenaltyState.from_prompts(penalties, sampler, logits.shape[-1], logits.device, list(idx),
                                                   max_new_tokens)
            logits = state.apply(logits)
        tok = sampler.sample(logits, step)
        if state is not None:
            state.append(tok)
        idx = torch.cat((idx, tok), dim=1)
    return idx


# ---------------------------------------------------------------------- ragged ---
class RaggedKVCache(KVCache):
    """A ``KVCache`` whose sequences each sit at their own length.

    The per-layer packed rows are the same ``(B, block_size, H*N*hs + H*dv)`` views
    (``rows``); each is cut from a ``(B, block_size + 1, ...)`` allocation (``store``)
    whose last row no kernel reads: the padding rows of a ragged step are written
    there.  ``lengths`` is a device int32 ``(B,)`` the kernels read; ``host_lengths``
    is the host's copy, kept in step by every function here.  Only ``decode_ragged``
    with a device-side ``active`` mask (``generate_ragged`` with ``eos_id``) cannot keep
    it exact without a sync: ``host_lengths`` is then an upper bound (``host_exact`` is
    False) until ``sync()``."""

    def __init__(self, rows_decode: bool = False, graph: bool = False, fused_step: bool = False):
        super().__init__()
        # rows_decode: a step of 2 .. 8 rows is one ops.diff_attention_decode_rows launch where it has
        # a plan (every row bitwise the one-row decode's); False (the default) keeps the extend kernel
        self.rows_decode = bool(rows_decode)
        # graph: decode_ragged replays one captured HIP graph per token (SeqDecodeGraph); ``lengths`` then
        # keeps its storage for the life of the cache.  fused_step: a step's RoPE and row scatter are one
        # ops.kv_step_rows launch.  Both False (the default): the eager step as it was
        self.use_graph = bool(graph)
        self.fused_step = _want_fused_step(fused_step)
        self.store: Dict[int, torch.Tensor] = {}
        self.lengths: Optional[torch.Tensor] = None
        self.host_lengths: List[int] = []
        self.host_exact = True

    def layer(self, layer: int, B: int, cap: int, width: int, like: torch.Tensor) -> torch.Tensor:
        buf = self.store.get(layer)
        if buf is None or buf.shape != (B, cap + 1, width) or buf.dtype != like.dtype:
            buf = torch.empty(B, cap + 1, width, device=like.device, dtype=like.dtype)
            self.store[layer] = buf
            self.rows[layer] = buf[:, :cap]
        return self.rows[layer]

    def _views(self, layer: int, qkv, dims, bs: int):
        """The layer's (k_rows, v_rows) views the kernels read, made on first use."""
        H, N, hs, dv = dims
        nq = H * N * hs
        buf = self.layer(layer, qkv.shape[0], bs, qkv.shape[-1] - nq, qkv)
        return buf[..., :nq].unflatten(-1, (H, N, hs)), buf[..., nq:].unflatten(-1, (H, dv))

    def write_rows(self, layer: int, qkv, k_rot, dims, bs: int, tbl, pos, counts):
        """Scatter a step's new rows: the real ones to cache rows pos[b] + r, the padding to
        the spare row.  Returns the (k_rows, v_rows) views the kernels read."""
        H, N, hs, _ = dims
        B, Tn, _ = qkv.shape
        kv = self._views(layer, qkv, dims, bs)
        r = torch.arange(Tn, device=qkv.device)
        real = r[None, :] < counts[:, None]
        dst = torch.where(real, pos[:, None].long() + r[None, :], bs).clamp_(max=bs)
        self.store[layer].index_put_((torch.arange(B, device=qkv.device)[:, None].expand(B, Tn), dst),
                                     _packed_new_rows(qkv, k_rot, H * N * hs))
        return kv

    def step_rows(self, layer: int, qkv, dims, bs: int, tbl, pos, counts, freqs):
        """``fused_step``: what ``_rope_rows_at`` + ``write_rows`` do, as one ``ops.kv_step_rows`` (the
        padding rows write nothing; the spare row stays untouched).  Returns (the rotated q, or None
        without RoPE; the (k_rows, v_rows) views ``write_rows`` returns)."""
        kv = self._views(layer, qkv, dims, bs)
        q_rot, _, _ = ops.kv_step_rows(*ops.split_packed(qkv, *dims), pos, counts, bs, freqs, dest=kv)
        return q_rot, kv

    def decode_rows(self, kv, q, coef, tbl, lengths):
        return ops.diff_attention_decode_ragged(q, *kv, coef, lengths)

    def extend_rows(self, kv, q, coef, tbl, pos, counts):
        return ops.diff_attention_extend_ragged(q, *kv, coef, pos, counts)

    def rows_rows(self, kv, q, coef, tbl, pos, counts):
        return ops.diff_attention_decode_rows(q, *kv, coef, pos, counts)

    def set_lengths(self, lengths: Sequence[int], device) -> None:
        self.host_lengths = [int(n) for n in lengths]
        new = torch.tensor(self.host_lengths, dtype=torch.int32, device=device)
        if self.use_graph and self.lengths is not None and self.lengths.shape == new.shape \
                and self.lengths.device == new.device:
            self.lengths.copy_(new)                # a captured graph reads and advances this storage
        else:
            self.graphs.clear()                    # another batch: the rows are reallocated with it
            self.lengths = new
        self.host_exact = True

    def advance(self, counts: torch.Tensor) -> None:
        """``lengths += counts`` on the device: in place where a graph may hold the storage."""
        if self.use_graph:
            self.lengths.add_(counts)
        else:
            self.lengths = self.lengths + counts

    def sync(self) -> List[int]:
        """Refresh ``host_lengths`` from the device (one host sync)."""
        if self.lengths is not None:
            self.host_lengths = self.lengths.tolist()
        self.host_exact = True
        return self.host_lengths

    def truncate(self, new_lengths) -> None:
        """Roll every sequence back to ``new_lengths[b] <= lengths[b]`` (the tokens a
        verification step did not accept).  Nothing is erased: the kernels ignore rows
        past a sequence's length, and the next step overwrites them."""
        if self.lengths is None:
            raise ValueError("truncate needs a prefilled cache")
        new = [int(n) for n in (new_lengths.tolist() if isinstance(new_lengths, torch.Tensor) else new_lengths)]
        if not self.host_exact:
            self.sync()
        if len(new) != len(self.host_lengths):
            raise ValueError(f"{len(new)} lengths for a batch of {len(self.host_lengths)}")
        for b, (n, have) in enumerate(zip(new, self.host_lengths)):
            if not 0 <= n <= have:
                raise ValueError(f"sequence {b}: cannot truncate length {have} to {n}")
        self.set_lengths(new, self.lengths.device)


def _want_fused_step(fused_step) -> bool:
    """The caches' ``fused_step`` flag; a library without ``dta_kv_step_rows`` cannot honour it."""
    if fused_step and not ops.kv_step_supported():
        raise RuntimeError("fused_step=True needs dta_kv_step_rows, which this libdiffattn.so does not export "
                           "(ops.kv_step_supported); there is no fallback")
    return bool(fused_step)


def _packed_new_rows(qkv, k_rot, nq: int):
    """A step's new cache rows ``[K | V]`` (B, Tn, W - nq): the slice of ``qkv``, or with
    RoPE the rotated K_i next to its V."""
    if k_rot is None:
        return qkv[..., nq:]
    return torch.cat([k_rot.flatten(2), qkv[..., 2 * nq:]], dim=-1)


def _seq_attention_step(block, x, layer: int, cache, tbl, pos, counts, rows, one_row: bool):
    """``_attention_step`` for rows at per-sequence positions, on a ``RaggedKVCache``
    (``tbl=None``) or a ``PagedKVCache`` (``tbl``: the step's contiguous (B, max_pages) table):
    sequence b's Tn rows sit at pos[b] .. pos[b]+Tn-1, the first counts[b] of them real (pos,
    counts: device int32 (B,); rows: their (B, Tn) long positions, clamped to the window).
    The cache writes the new rows (``write_rows``: the padding rows land in its spare row or
    page) and names the op that reads them back (``decode_rows``, ``extend_rows``, and with
    ``cache.rows_decode`` ``rows_rows`` for a step of 2 .. 8 rows that has a plan).  With
    ``cache.fused_step`` the rotation of q and K_i and the write are one launch (``step_rows``:
    the same views back, the padding rows written nowhere).
    ``pos=None``: the paged cache's right-padded prefill from position 0 (fused training
    forward on the unquantised activations; counts = the prompt lengths)."""
    attn, H, N, hs, dv, bs = _spec(block)
    weight, coef, freqs = _constants(cache, attn, layer, H, hs, bs, x)
    qkv = F.linear(x, weight)
    B, Tn, _ = qkv.shape
    q, k_new, _ = ops.split_packed(qkv, H, N, hs, dv)
    k_rot = None
    fused = pos is not None and getattr(cache, "fused_step", False)     # a cache class of its own may not know the flag
    if pos is None:
        out = ops.diff_attention(qkv, coef, H, N, hs, None if freqs is None else freqs[:Tn], dv)
        if freqs is not None:
            k_rot = torch.empty(B, Tn, H, N, hs, device=qkv.device, dtype=qkv.dtype)
            ops.rope_rows(k_new, k_rot, freqs[:Tn])
    elif fused:                                   # RoPE and scatter in one launch; padding rows write nothing
        q_rot, kv = cache.step_rows(layer, qkv, (H, N, hs, dv), bs, tbl, pos, counts, freqs)
        q = q if q_rot is None else q_rot
    elif freqs is not None:
        q, k_rot = _rope_rows_at(q, k_new, freqs, rows)
    if not fused:
        kv = cache.write_rows(layer, qkv, k_rot, (H, N, hs, dv), bs, tbl, pos, counts)
    if pos is None:
        pass
    elif one_row:
        out = cache.decode_rows(kv, q[:, 0], coef, tbl, pos + counts).view(B, 1, H * dv)
    elif (cache.rows_decode and 2 <= Tn <= ops.DECODE_ROWS_MAX
          and ops.decode_rows_supported(qkv.dtype, hs, N, dv, Tn, fp8=cache.kv_dtype is not None)):
        out = cache.rows_rows(kv, q, coef, tbl, pos, counts)      # a short step: the cache is read once
    elif (ops.extend_supported(qkv.dtype, hs, N, dv) if cache.kv_dtype is None
          else cache.fp8_extend and ops.extend_fp8_supported(qkv.dtype, hs, N, dv)):
        out = cache.extend_rows(kv, q, coef, tbl, pos, counts)
    else:       # no extend plan for this shape, or an fp8 pool without ``fp8_extend``
        out = _decode_per_row(lambda i, n: cache.decode_rows(kv, q[:, i], coef, tbl, n), Tn, pos, counts)
    return _attention_tail(attn, out)


def _seq_model_step(model, idx, cache, tbl, pos, counts, gather=None, one_row: bool = False):
    """The model's forward over (B, T) tokens, sequence b's at positions pos[b] .., on a
    ``RaggedKVCache`` (``tbl=None``) or a ``PagedKVCache``.  ``pos=None``: a right-padded
    prefill from position 0 through the fused training forward.  Returns every row's logits
    (B, T, vocab), or with ``gather`` (long (B,)) row gather[b] of each sequence (B, vocab)."""
    B, T = idx.shape
    r = torch.arange(T, device=idx.device)
    rows = r if pos is None else (pos[:, None].long() + r[None, :]).clamp_(max=model.block_size - 1)
    x = model.token_embedding_table(idx)
    if hasattr(model, "position_embedding_table"):
        x = x + model.position_embedding_table(rows)
    for layer, block in enumerate(model.blocks, 1):
        h = block.ln1(x)
        if pos is None and tbl is None:       # the ragged prefill is the one-length prefill
            x = x + _attention_step(block, h, layer, cache, 0)
        else:
            x = x + _seq_attention_step(block, h, layer, cache, tbl, pos, counts, rows, one_row)
        x = x + block.ffwd(block.ln2(x))
    if gather is None:
        return model.lm_head(model.ln_f(x))
    x = x[torch.arange(B, device=idx.device), gather].unsqueeze(1)
    return model.lm_head(model.ln_f(x))[:, 0]


# the names the ragged and the paged functions reach the step by (the CPU bookkeeping tests stub each)
def _ragged_model_step(model, idx, cache: RaggedKVCache, pos, counts, gather=None, one_row: bool = False):
    return _seq_model_step(model, idx, cache, None, pos, counts, gather, one_row)


_paged_model_step = _seq_model_step


def _check_prompts(prompts, bs: int) -> List[int]:
    """The lengths of a prefill's prompts (one-dimensional LongTensors of 1 .. block_size tokens)."""
    lens = []
    for p in prompts:
        if not isinstance(p, torch.Tensor) or p.dim() != 1 or p.dtype != torch.long:
            raise ValueError("prompts must be one-dimensional LongTensors")
        if not 1 <= p.shape[0] <= bs:
            raise ValueError(f"a prompt of {p.shape[0]} tokens is outside 1 .. block_size {bs}")
        lens.append(p.shape[0])
    if not lens:
        raise ValueError("no prompts")
    return lens


def _check_counts(counts, names, have: Sequence[int], Tn: int, bs: int) -> List[int]:
    """An append's ``counts`` as host integers (a tensor: one sync), each within 0 .. Tn and
    within the window of its sequence (``names[b]`` at length ``have[b]``)."""
    cnt = [int(c) for c in (counts.tolist() if isinstance(counts, torch.Tensor) else counts)]
    if len(cnt) != len(have):
        raise ValueError(f"{len(cnt)} counts for a batch of {len(have)}")
    for name, c, n in zip(names, cnt, have):
        if not 0 <= c <= Tn:
            raise ValueError(f"sequence {name}: count {c} outside 0 .. {Tn}")
        if n + c > bs:
            raise ValueError(f"sequence {name}: appending {c} tokens at length {n} crosses block_size {bs}")
    return cnt


def _append_parts(step, lens, have: Sequence[int], cnt: Sequence[int], new_idx, bs: int, all_rows: bool):
    """An append as one step, or as several narrower ones where a sequence sits so close to
    block_size that its padded rows would not fit.  ``step(idx, pos, counts, gather)`` is the
    cache's model step, ``lens`` / ``have`` the device and host lengths before the append.
    Returns (the logits ``append_ragged`` documents, ``cnt`` on the device)."""
    Tn = new_idx.shape[1]
    cnt_dev = torch.tensor(cnt, dtype=torch.int32, device=new_idx.device)
    out = None
    done = 0
    while done < Tn:
        # the kernel needs pos[b] + width <= block_size of every sequence that still has real rows
        live = [n + done for c, n in zip(cnt, have) if c > done]
        w = min(Tn - done, bs - max(live)) if live else min(Tn - done, bs)
        pos = lens + cnt_dev.clamp(max=done)
        part_cnt = (cnt_dev - done).clamp_(0, w)
        part_idx = new_idx[:, done:done + w]
        if all_rows:
            part = step(part_idx, pos, part_cnt, None)
            out = part if out is None else torch.cat([out, part], dim=1)
        else:
            last = (cnt_dev.long() - 1 - done).clamp_(0, w - 1)
            part = step(part_idx, pos, part_cnt, last)
            here = ((cnt_dev > done) | (done == 0))[:, None]
            out = part if out is None else torch.where(here, part, out)
        done += w
    return out, cnt_dev


def _sample_tokens(logits, max_new_tokens: int, eos_id: Optional[int], decode, sampler: Optional[Sampler] = None,
                   streams: Optional[torch.Tensor] = None, penalties: Optional["_PenaltyState"] = None):
    """The reference's sampling loop (softmax of the last logits, one ``torch.multinomial``
    over the whole batch; with a ``sampler``, one ``ops.sample_rows`` launch that draws row b's
    ``step``-th token from (seed, ``streams[b]`` or b, step)) for ``max_new_tokens >= 1`` tokens; ``decode(tok, active)`` is the
    cache's one-token step, ``active`` the device mask of the sequences that have not
    sampled ``eos_id`` (None without one).  Returns (toks (B, max_new_tokens), keep): sequence
    b keeps its first keep[b] tokens, up to its first ``eos_id`` -- the loop's one host sync.
    ``penalties``: the loop's ``_PenaltyState`` (one history row per row of ``logits``); every step then runs
    ``ops.penalize_rows`` in front of the sampler and appends its tokens to the histories on the device."""
    B = logits.shape[0]
    active = None if eos_id is None else torch.ones(B, dtype=torch.bool, device=logits.device)
    new = []
    for step in range(max_new_tokens):
        if penalties is not None:
            tok = sampler.sample(penalties.apply(logits), step, streams)
            penalties.append(tok)
        elif sampler is not None:
            tok = sampler.sample(logits, step, streams)
        else:
            probs = F.softmax(logits, dim=-1)
            tok = torch.multinomial(probs, num_samples=1)
        new.append(tok)
        if step + 1 == max_new_tokens:
            break
        if active is not None:
            active = active & (tok[:, 0] != eos_id)
        logits = decode(tok, active)
    toks = torch.cat(new, dim=1)
    keep = [max_new_tokens] * B
    if eos_id is not None:
        hit = toks == eos_id
        first = torch.where(hit.any(dim=1), hit.int().argmax(dim=1) + 1, max_new_tokens)
        keep = first.tolist()
    return toks, keep


def _check_speculate(speculate, sampler, n_samples: int = 1, shared_decode: bool = False, penalties=None) -> None:
    if not isinstance(speculate, Speculation):
        raise ValueError("speculate must be a Speculation")
    if penalties is not None and speculate.graph:
        raise ValueError("Speculation(graph=True) with penalties is not supported: the captured round does not "
                         "hold the ops.penalize_rows launch")
    if sampler is None:
        raise ValueError("speculate needs a sampler: the reference's batch-wide torch.multinomial has no "
                         "per-sequence stream to couple the verification to")
    if n_samples > 1:
        raise ValueError("speculate with n_samples > 1 is not supported")
    if shared_decode:
        raise ValueError("speculate with shared_decode=True is not supported")


def _speculative_tokens(logits, prompts, max_new_tokens: int, eos_id: Optional[int], sampler: Sampler,
                        streams: Optional[torch.Tensor], spec: Speculation, bs: int, append, truncate,
                        fixed=None, penalties: Optional[Penalties] = None):
    """``_sample_tokens`` by speculative rounds, for ``max_new_tokens >= 1``.  ``logits`` (B, vocab) are the
    prefill's; ``append(new_idx, counts)`` is the cache's multi-row step with ``all_rows=True`` and
    ``truncate(lengths)`` its roll-back.  Per sequence the device holds the token history (prompt and
    emitted tokens; the last one is pending: emitted, not yet through the model), the tokens still owed
    and the draft.  A round feeds [pending, draft...] (counts ``dcnt + 1``, 0 for a finished sequence),
    samples every row in one ``ops.sample_rows`` launch -- sequence b's row j with (stream b, offset =
    tokens emitted so far + j), the plain loop's -- runs one ``ops.spec_accept_draft`` and reads one
    small tensor back ((m, next dcnt) and the tokens still owed), then truncates each cache to its old
    length + m.  The first token comes from the prefill's logits through the same kernel, with no draft
    to accept.  Returns the histories: a list of B int64 tensors, prompt included.

    ``fixed``: with ``spec.graph``, the (model, cache, the paged call's sequence ids or None) a ``SpecRound``
    is made from.  A round then does the host's work first -- paged: ``_check_live``, the pages of its
    ``dcnt + 1`` rows (exact: ``dcnt`` came back with the last read), ``_flush`` -- then replays, reads the
    same small tensor back and settles the host's copy of the lengths (``PagedKVCache._rolled_back``; the
    device lengths are already right).  A round in which a live sequence has ``length + K + 1 > block_size``
    -- its padded rows would not fit the window -- takes the eager path above on the same state; the two
    give the same tokens, so they may interleave.

    ``penalties``: the first token's logits and every round's rows pass through ``ops.penalize_rows`` with the
    loop's own ``hist`` / ``hlen`` / ``draft`` / ``dcnt`` and the prompt lengths as ``gen_start``: row j is
    penalised with the history plus the j drafts before it, what the plain loop sees there if they are accepted
    (eager rounds only)."""
    dev = logits.device
    B, K = len(prompts), spec.k
    lens = [int(p.shape[0]) for p in prompts]
    cap = max(lens) + max_new_tokens
    hist = torch.zeros(B, cap, dtype=torch.int32, device=dev)
    hist[:, :max(lens)] = torch.nn.utils.rnn.pad_sequence(list(prompts), batch_first=True).to(dev, torch.int32)
    hlen = torch.tensor(lens, dtype=torch.int32, device=dev)
    draft = torch.zeros(B, K, dtype=torch.int32, device=dev)
    dcnt = torch.zeros(B, dtype=torch.int32, device=dev)
    back = torch.zeros(3 * B, dtype=torch.int32, device=dev)     # (m, next dcnt) next to the tokens still owed:
    result, remaining = back[:2 * B].view(B, 2), back[2 * B:]    # one read a round
    remaining.fill_(max_new_tokens)
    strm = torch.arange(B, dtype=torch.int64, device=dev) if streams is None else streams
    eos = -1 if eos_id is None else int(eos_id)
    lookup = spec.drafter is None
    stats = spec.stats
    stats.update(rounds=0, drafted=0, accepted=0, emitted=0)

    def tally(counts, m):
        stats["rounds"] += 1
        stats["drafted"] += sum(c - 1 for c in counts if c)
        stats["accepted"] += sum(k - 1 for k in m if k)
        stats["emitted"] += sum(m)

    def accept(tok):
        ops.spec_accept_draft(hist, hlen, remaining, draft, dcnt, tok, eos, K, spec.ngram_min if lookup else 0,
                              spec.ngram_max, bs, result)
        return read_back()

    def read_back():
        if not lookup:
            d, n = spec.drafter.propose(hist, hlen, remaining, K)
            room = torch.minimum(remaining - 1, bs - hlen).clamp(0, K)
            dcnt.copy_(torch.minimum(n.to(dev, torch.int32), room))
            draft.copy_(d.to(dev, torch.int32))
            result[:, 1] = dcnt
        host = back.tolist()
        return host[0:2 * B:2], host[1:2 * B:2], host[2 * B:]

    have = list(lens)                                            # rows in the cache
    pen = None
    if penalties is not None:
        pen = _PenaltyState(penalties, sampler, logits.shape[-1], dev, hist, hlen,
                            torch.tensor(lens, dtype=torch.int32, device=dev))
        logits = pen.apply(logits)
    tok = sampler.sample(logits, 0, strm)                        # (B, 1): offset 0 of every stream
    m, dc, rem = accept(tok)
    stats["emitted"] += sum(m)
    cols = torch.arange(K, device=dev)
    fixed_round = None
    if spec.graph and any(r > 0 for r in rem):
        model, cache, seqs = fixed
        slots = None if seqs is None else torch.tensor([cache.slot[q] for q in seqs], device=dev)
        fixed_round = SpecRound(model, cache, sampler, spec, (hist, hlen, remaining, draft, dcnt, result),
                                max_new_tokens, logits.shape[-1], eos, strm, slots)
    while any(r > 0 for r in rem):
        counts = [d + 1 if r > 0 else 0 for d, r in zip(dc, rem)]
        if fixed_round is not None and all(n + K + 1 <= bs for n, r in zip(have, rem) if r > 0):
            if seqs is not None:                                 # page growth and copy on write: the host's, first
                cache._check_live(seqs)
                writers = [b for b in range(B) if counts[b] > 0]
                cache._prepare_writes([seqs[b] for b in writers], [have[b] + counts[b] for b in writers])
                cache._flush()
            fixed_round.run()
            m, dc_next, rem = read_back()
            have = [n + k for n, k in zip(have, m)]
            if seqs is None:
                cache.host_lengths = list(have)
            else:
                for q, n in zip(seqs, have):
                    cache._rolled_back(q, n)
            tally(counts, m)
            dc = dc_next
            continue
        Tn = max(counts)
        pending = hist.gather(1, (hlen.long() - 1).clamp_(min=0)[:, None])
        drafted = torch.where(cols[None, :Tn - 1] < dcnt[:, None], draft[:, :Tn - 1], 0)
        new_idx = torch.cat([pending, drafted], dim=1).long().clamp_(min=0)
        rows = append(new_idx, counts)                           # (B, Tn, vocab)
        if pen is not None:
            rows = pen.apply(rows.reshape(B * Tn, -1), draft, dcnt, Tn).view(B, Tn, -1)
        offset = (max_new_tokens - remaining.long())[:, None] + torch.arange(Tn, device=dev)[None, :]
        tok = ops.sample_rows(rows, sampler.temperature, sampler.top_k, sampler.top_p, sampler.seed,
                              strm[:, None].expand(B, Tn).reshape(-1), offset.reshape(-1))
        m, dc_next, rem = accept(tok)
        have = [n + k for n, k in zip(have, m)]
        if any(k < c for k, c in zip(m, counts)):
            truncate(have)
        tally(counts, m)
        dc = dc_next
    ends = hlen.tolist()
    out = hist.cpu()
    return [out[b, :ends[b]].long() for b in range(B)]


def _check_ragged(cache, B: int) -> None:
    if not isinstance(cache, RaggedKVCache) or cache.lengths is None:
        raise ValueError("a prefilled RaggedKVCache is needed: run prefill_ragged first")
    if len(cache.host_lengths) != B:
        raise ValueError(f"batch size {B} differs from the cache's {len(cache.host_lengths)}")


@torch.no_grad()
def prefill_ragged(model, prompts: Sequence[torch.Tensor], cache: RaggedKVCache) -> torch.Tensor:
    """Prefill ``cache`` with B prompts of different lengths (one-dimensional
    LongTensors, 1 .. block_size tokens each) in one fused forward: the prompts are
    right-padded to the longest (the forward is causal, so the padding cannot reach a
    real row), every row's K_i / V is cached and ``lengths[b] = len(prompts[b])`` hides
    the padding.  Returns (B, vocab): each sequence's logits at its own last token."""
    lens = _check_prompts(prompts, model.block_size)
    if not isinstance(cache, RaggedKVCache):
        raise ValueError("prefill_ragged needs a RaggedKVCache")
    idx = torch.nn.utils.rnn.pad_sequence(list(prompts), batch_first=True)
    last = torch.tensor(lens, device=idx.device) - 1
    logits = _ragged_model_step(model, idx, cache, None, None, gather=last)
    cache.set_lengths(lens, idx.device)
    return logits


@torch.no_grad()
def decode_ragged(model, tok: torch.Tensor, cache: RaggedKVCache, active: Optional[torch.Tensor] = None):
    """One new token per sequence: ``tok`` (B, 1) is sequence b's token at position
    ``lengths[b]``.  Its K_i / V row is scattered there, the position-table or RoPE row
    is gathered per sequence, and each layer runs one ``diff_attention_decode_ragged``
    over ``lengths + 1``.  Returns (B, vocab) and advances every length by one.

    ``active``: optional device bool (B,).  A sequence with ``active[b]`` False is
    finished: its length stays, nothing of it is cached and its logits are unspecified.
    The mask is applied on the device (no host sync), so ``host_lengths`` becomes an
    upper bound (``RaggedKVCache.sync``)."""
    if tok.dim() != 2 or tok.shape[1] != 1:
        raise ValueError("tok must be (B, 1)")
    B, bs = tok.shape[0], model.block_size
    _check_ragged(cache, B)
    if active is None:
        if max(cache.host_lengths) + 1 > bs:
            raise ValueError(f"a sequence is at block_size {bs}: positions are absolute within the window, "
                             "the sliding window is the one-length path's job (last_logits)")
        counts = torch.ones_like(cache.lengths)
    else:
        counts = active.to(torch.int32)
    if cache.use_graph:
        logits = _seq_graph(model, cache, B, active is not None, tok.device).step(tok, counts)
    else:
        logits = _ragged_model_step(model, tok, cache, cache.lengths, counts, one_row=True)[:, 0]
        cache.advance(counts)
    cache.host_lengths = [min(n + 1, bs) for n in cache.host_lengths]
    if active is not None:
        cache.host_exact = False
    return logits


@torch.no_grad()
def append_ragged(model, new_idx: torch.Tensor, counts, cache: RaggedKVCache, all_rows: bool = False):
    """Feed sequence b the first ``counts[b]`` tokens of ``new_idx[b]`` ((B, Tn), padded;
    ``0 <= counts[b] <= Tn``) at positions ``lengths[b] ..``: one
    ``diff_attention_extend_ragged`` per layer (head sizes without an extend plan: one
    ragged decode per row).  Returns each sequence's logits at its last real row
    (B, vocab), or with ``all_rows`` every row's (B, Tn, vocab), where row r < counts[b]
    is the distribution after ``new_idx[b, r]`` -- the verification of speculated tokens;
    ``cache.truncate`` then rolls back what was not accepted.  Padding rows, and the
    returned row of a sequence with count 0 (whose length stays), are unspecified.

    Raises ``ValueError`` if any ``lengths[b] + counts[b] > block_size``.  ``counts`` is
    read on the host (a list, or a tensor: one sync).  A sequence so close to
    block_size that its padded rows would not fit (``lengths[b] + Tn > block_size``) makes
    the step run as several narrower ones."""
    if new_idx.dim() != 2 or new_idx.shape[1] < 1:
        raise ValueError("new_idx must be (B, Tn) with Tn >= 1")
    B, Tn = new_idx.shape
    bs = model.block_size
    _check_ragged(cache, B)
    if not cache.host_exact:
        cache.sync()
    cnt = _check_counts(counts, range(B), cache.host_lengths, Tn, bs)
    out, cnt_dev = _append_parts(lambda idx, pos, c, last: _ragged_model_step(model, idx, cache, pos, c, last),
                                 cache.lengths, cache.host_lengths, cnt, new_idx, bs, all_rows)
    cache.advance(cnt_dev)
    cache.host_lengths = [n + c for n, c in zip(cache.host_lengths, cnt)]
    return out


@torch.no_grad()
def generate_ragged(model, prompts: Sequence[torch.Tensor], max_new_tokens: int, eos_id: Optional[int] = None,
                    graph: bool = False, fused_step: bool = False, sampler: Optional[Sampler] = None,
                    streams: Optional[Sequence[int]] = None, speculate: Optional[Speculation] = None,
                    penalties: Optional[Penalties] = None):
    """``generate`` for B prompts of different lengths as one batch (any of the three
    models): one ``prefill_ragged``, then one ``decode_ragged`` step per token.  Sampling
    is the reference's (softmax of the last logits, ``torch.multinomial`` over the whole
    batch, diff_transformer.py:177-185).  Returns a list of B one-dimensional tensors,
    prompt b followed by its ``max_new_tokens`` samples; with ``eos_id`` a sequence ends
    at its first sampled ``eos_id`` (kept): from then on its length is frozen and its
    further samples are discarded.

    Positions are absolute within the window, and a slide re-bases every cached
    position: that stays the one-length path's job (``model.generate``).  So this
    raises ``ValueError`` if any ``len(prompts[b]) + max_new_tokens > block_size``.  The
    loop never reads a length back to the host; the one sync is at the end, where
    ``eos_id`` cuts the outputs.  ``graph`` / ``fused_step``: ``RaggedKVCache``'s (each token's step
    replays one captured HIP graph; its RoPE and row scatter are one launch): same logits, bit for bit.
    ``sampler``: a ``Sampler`` replaces softmax + multinomial by one ``ops.sample_rows`` launch per step,
    run eagerly after the step or its graph replay; sequence b's t-th token is drawn from (seed,
    stream b, offset t) -- ``streams`` gives the prompts other stream ids -- so it does not depend on
    the rest of the batch.  None (the default): the reference's sampling, token for token.
    ``speculate``: a ``Speculation`` (needs a ``sampler``) runs the loop as speculative rounds
    (``_speculative_tokens``): the same tokens as without it, token for token, in fewer model steps where the
    drafts are accepted.  The cache is then made with ``rows_decode=True``, so a round of 2 .. 8 rows that
    has a plan reads the cache once and every row is the one-row decode's; ``graph`` / ``fused_step`` keep
    their meaning for one-token steps and rounds do not use the graph; a round reads three small integers
    per sequence back.  ``Speculation(graph=True)`` replays each round as one captured HIP graph of K + 1 rows
    per sequence (``SpecRound``); the cache then keeps the storage of ``lengths`` as with ``graph=True``.
    ``penalties``: a ``Penalties`` (needs a ``sampler``) puts one ``ops.penalize_rows`` launch in front of every
    ``ops.sample_rows`` one, eagerly after the step or its replay; the loop keeps the token histories on the
    device and appends to them without a host sync.  With ``speculate`` the tokens stay the plain loop's (not
    with ``Speculation(graph=True)``: ``ValueError``).  None (the default): the loops as they were."""
    bs = model.block_size
    if penalties is not None:
        _check_penalties(penalties, sampler)
    if speculate is not None:
        _check_speculate(speculate, sampler, penalties=penalties)
    for p in prompts:
        if p.shape[0] + max_new_tokens > bs:
            raise ValueError(f"a prompt of {p.shape[0]} tokens plus {max_new_tokens} new ones crosses "
                             f"block_size {bs}: the sliding window is the one-length path's job")
    cache = RaggedKVCache(rows_decode=speculate is not None,
                          graph=graph or (speculate is not None and speculate.graph), fused_step=fused_step)
    logits = prefill_ragged(model, prompts, cache)
    if max_new_tokens < 1:
        return [p.clone() for p in prompts]
    if speculate is not None:
        outs = _speculative_tokens(logits, prompts, max_new_tokens, eos_id, sampler,
                                   _stream_ids(streams, len(prompts), 1, logits.device), speculate, bs,
                                   lambda idx, counts: append_ragged(model, idx, counts, cache, all_rows=True),
                                   cache.truncate, (model, cache, None), penalties)
        return [o.to(p.device) for o, p in zip(outs, prompts)]
    state = None if penalties is None else _PenaltyState.from_prompts(penalties, sampler, logits.shape[-1],
                                                                      logits.device, prompts, max_new_tokens)
    toks, keep = _sample_tokens(logits, max_new_tokens, eos_id,
                                lambda tok, active: decode_ragged(model, tok, cache, active), sampler,
                                _stream_ids(streams, len(prompts), 1, logits.device), state)
    return [torch.cat([p, toks[b, :keep[b]].to(p.device)]) for b, p in enumerate(prompts)]


# ----------------------------------------------------------------------- paged ---
SHARED_MIN_ROWS = 256      # one decode chunk (DTA_DECODE_CHUNK): a group pass covers whole chunks only


class OutOfPages(RuntimeError):
    """The pool has fewer free pages than a step needs.  Raised before anything is
    written: the allocator, the tables and the lengths are as they were."""


class PagedKVCache(KVCache):
    """K_i / V rows of many sequences in one pool of ``num_pages`` pages of ``page_size``
    rows (32, 64, 128 or 256), reached through a block table.

    Per layer one ``(num_pages + 1, page_size, H*N*hs + H*dv)`` allocation (``pool``), made
    on first use; the last page is a spare no table points to, where the padding rows of
    a step are scattered (the ragged cache's spare row).  A sequence is named by the id
    ``prefill_paged`` or ``fork`` returned; ids are never reused.  The host keeps the free
    list, one refcount per page, each sequence's page list (``pages``) and length
    (``host_lengths``); the device keeps ``block_table`` int32 ``(max_seqs, max_pages)``
    (``max_pages = ceil(block_size / page_size)``, unused entries -1) and ``lengths`` int32
    ``(max_seqs,)``, one row per live sequence (``slot``).  A step gathers the rows of its
    sequences with ``index_select`` into the contiguous table the kernels take and
    scatters the new lengths back.  Host changes of a table row or a length (prefill,
    fork, copy on write, truncate, release) reach the device in one copy at the start of
    the next step.

    As for ``RaggedKVCache``, a ``decode_paged`` with a device-side ``active`` mask leaves
    ``host_lengths`` an upper bound (``host_exact`` False) until ``sync()``; pages are then
    taken for the bound and ``sync()`` / ``release`` return the surplus."""

    KV_DTYPES = (None, "fp8_e4m3")

    def __init__(self, num_pages: int, page_size: int = 64, max_seqs: Optional[int] = None, kv_dtype=None,
                 fp8_extend: bool = False, rows_decode: bool = False, shared_decode: bool = False,
                 graph: bool = False, fused_step: bool = False):
        super().__init__()
        if page_size not in ops.PAGE_SIZES:
            raise ValueError(f"page_size {page_size} is not one of {ops.PAGE_SIZES}")
        if kv_dtype not in self.KV_DTYPES:
            raise ValueError(f"kv_dtype {kv_dtype!r} is not one of {self.KV_DTYPES}")
        if fp8_extend and kv_dtype is None:
            raise ValueError("fp8_extend=True needs an fp8 pool (kv_dtype='fp8_e4m3')")
        # "fp8_e4m3": the per-layer pool is uint8 (num_pages + 1, P, W), OCP e4m3fn bytes in the same
        # row layout, next to scale_pool fp32 (num_pages + 1, P, H * (N + 1)): one scale per (row,
        # head, K_i | V).  A step quantises its new rows (ops.kv_quant_rows) and decodes on the bytes
        # (ops.diff_attention_decode_paged_fp8).  None: the pool in the projection's dtype.
        # fp8_extend: a multi-row step on those bytes is one ops.diff_attention_extend_paged_fp8 launch
        # where it has a plan; False (the default) keeps one decode launch per row.
        self.kv_dtype = kv_dtype
        self.fp8_extend = bool(fp8_extend)
        # rows_decode: a step of 2 .. 8 rows is one ops.diff_attention_decode_rows_paged(_fp8) launch where
        # it has a plan, on either kind of pool (it comes before fp8_extend); False (the default) changes nothing
        self.rows_decode = bool(rows_decode)
        # shared_decode: decode_paged plans, on the host, which of its sequences still share their first
        # pages (forks of one prompt) and each layer's one-row decode reads those pages once per group
        # (ops.diff_attention_decode_paged_shared(_fp8), bitwise the paged op); False (the default) changes nothing
        self.shared_decode = bool(shared_decode)
        self._shared_key = None                    # (sequences, their page lists) the kept plan was made from
        self._shared_kept = None
        self.scale_pool: Dict[int, torch.Tensor] = {}
        if num_pages < 1:
            raise ValueError("num_pages must be >= 1")
        # graph: decode_paged replays one captured HIP graph per token (SeqDecodeGraph; page growth and copy
        # on write stay on the host, before the replay).  Not with shared_decode: the plan's group count is a
        # host launch argument that changes between steps.  fused_step: a step's RoPE and row scatter are one
        # ops.kv_step_rows launch (fp8: followed by ops.kv_quant_rows).  Both False (the default) change nothing
        if graph and shared_decode:
            raise ValueError("graph=True cannot be combined with shared_decode=True: the shared plan's group "
                             "count is a host launch argument that changes between steps")
        self.use_graph = bool(graph)
        self.fused_step = _want_fused_step(fused_step)
        self.num_pages, self.page_size = int(num_pages), int(page_size)
        self.max_seqs = int(num_pages if max_seqs is None else max_seqs)
        if self.max_seqs < 1:
            raise ValueError("max_seqs must be >= 1")
        self.pool: Dict[int, torch.Tensor] = {}
        self.free: List[int] = list(range(self.num_pages - 1, -1, -1))    # a stack: pop() takes page 0 first
        self.refcount: List[int] = [0] * self.num_pages
        self.pages: Dict[int, List[int]] = {}
        self.host_lengths: Dict[int, int] = {}
        self.host_low: Dict[int, int] = {}         # the exact length at the last sync (<= the true length)
        self.host_exact = True
        self.slot: Dict[int, int] = {}
        self.free_slots: List[int] = list(range(self.max_seqs - 1, -1, -1))
        self.next_id = 0
        self.max_pages = 0
        self.block_table: Optional[torch.Tensor] = None
        self.lengths: Optional[torch.Tensor] = None
        self._dirty_rows: set = set()              # sequences whose table row / length the device has not seen
        self._dirty_lens: set = set()

    # ---- storage
    def layer_pool(self, layer: int, width: int, like: torch.Tensor) -> torch.Tensor:
        buf = self.pool.get(layer)
        shape = (self.num_pages + 1, self.page_size, width)
        if buf is None or buf.shape != shape or buf.dtype != like.dtype:
            buf = torch.empty(shape, device=like.device, dtype=like.dtype)
            self.pool[layer] = buf
        return buf

    def layer_pool_fp8(self, layer: int, width: int, H: int, N: int, device):
        """The layer's byte pool and scale pool (``kv_dtype="fp8_e4m3"``), made on first use."""
        buf, sc = self.pool.get(layer), self.scale_pool.get(layer)
        shape, sshape = (self.num_pages + 1, self.page_size, width), (self.num_pages + 1, self.page_size, H * (N + 1))
        if buf is None or buf.shape != shape or buf.dtype != torch.uint8 or sc is None or sc.shape != sshape:
            buf = torch.empty(shape, device=device, dtype=torch.uint8)
            sc = torch.empty(sshape, device=device, dtype=torch.float32)
            self.pool[layer], self.scale_pool[layer] = buf, sc
        return buf, sc

    def _views(self, layer: int, qkv, dims):
        """The layer's pool, made on first use, as (what a row write takes, what the kernels read): the
        pool itself and the (k, v) views of its own pages; fp8: the (k, v, scales) views of every page, the
        spare one included, and of its own pages."""
        H, N, hs, dv = dims
        nq, npg = H * N * hs, self.num_pages
        if self.kv_dtype is None:
            pool = self.layer_pool(layer, qkv.shape[-1] - nq, qkv)
            return pool, (pool[:npg, :, :nq].unflatten(-1, (H, N, hs)), pool[:npg, :, nq:].unflatten(-1, (H, dv)))
        pool, scales = self.layer_pool_fp8(layer, qkv.shape[-1] - nq, H, N, qkv.device)
        every = (pool[..., :nq].unflatten(-1, (H, N, hs)), pool[..., nq:].unflatten(-1, (H, dv)),
                 scales.unflatten(-1, (H, N + 1)))
        return every, (every[0][:npg], every[1][:npg], every[2][:npg])

    def write_rows(self, layer: int, qkv, k_rot, dims, bs: int, tbl, pos, counts):
        """Scatter a step's new rows: the real ones to row (pos[b] + r) % P of page
        tbl[b, (pos[b] + r) // P] (``pos=None``: the prefill's, from row 0), the padding to
        the spare page -- one ``index_put_``, or on an fp8 pool one ``ops.kv_quant_rows``
        (straight from the RoPE temporary and the V slice of ``qkv``: no concatenated copy).
        Returns the pool views the kernels read: (k_pool, v_pool), fp8 (k, v, scales)."""
        H, N, hs, _ = dims
        B, Tn, _ = qkv.shape
        nq = H * N * hs
        P, npg = self.page_size, self.num_pages
        r = torch.arange(Tn, device=qkv.device)
        at = r[None, :].expand(B, Tn) if pos is None else pos[:, None].long() + r[None, :]
        real = (r[None, :] < counts[:, None]) & (at < bs)
        page = torch.where(real, tbl.gather(1, (at // P).clamp(max=tbl.shape[1] - 1)).long(), npg)
        store, kv = self._views(layer, qkv, dims)
        if self.kv_dtype is None:
            store.index_put_((page, at % P), _packed_new_rows(qkv, k_rot, nq))
            return kv
        _, k_new, v_new = ops.split_packed(qkv, *dims)
        ops.kv_quant_rows(k_new if k_rot is None else k_rot, v_new, *store,
                          (page * P + at % P).to(torch.int32).flatten())
        return kv

    def step_rows(self, layer: int, qkv, dims, bs: int, tbl, pos, counts, freqs):
        """``fused_step``: what ``_rope_rows_at`` + ``write_rows`` do, as one ``ops.kv_step_rows`` -- on an
        fp8 pool that launch makes the rotated K_i and the slots, and ``ops.kv_quant_rows`` runs on them
        unchanged.  The spare page is never written (fp8: only by the quantiser, with the padding rows).
        Returns (the rotated q, or None without RoPE; the pool views ``write_rows`` returns)."""
        q, k_new, v_new = ops.split_packed(qkv, *dims)
        store, kv = self._views(layer, qkv, dims)
        if self.kv_dtype is None:
            q_rot, _, _ = ops.kv_step_rows(q, k_new, v_new, pos, counts, bs, freqs, dest=kv, block_table=tbl)
            return q_rot, kv
        q_rot, k_out, slots = ops.kv_step_rows(q, k_new, v_new, pos, counts, bs, freqs, None, tbl, self.page_size,
                                               self.num_pages)
        ops.kv_quant_rows(k_new if k_out is None else k_out, v_new, *store, slots)
        return q_rot, kv

    def decode_rows(self, kv, q, coef, tbl, lengths):
        plan = self.shared_plan                   # set by decode_paged for its one-row step only
        if (plan is not None and plan.n_groups and plan.B == q.shape[0] and ops.decode_shared_supported(
                q.dtype, q.shape[-1], q.shape[-2], kv[1].shape[-1], fp8=self.kv_dtype is not None)):
            if self.kv_dtype is None:
                return ops.diff_attention_decode_paged_shared(q, *kv, coef, tbl, lengths, plan)
            return ops.diff_attention_decode_paged_shared_fp8(q, *kv, coef, tbl, lengths, plan)
        if self.kv_dtype is None:
            return ops.diff_attention_decode_paged(q, *kv, coef, tbl, lengths)
        return ops.diff_attention_decode_paged_fp8(q, *kv, coef, tbl, lengths)

    def extend_rows(self, kv, q, coef, tbl, pos, counts):
        if self.kv_dtype is None:
            return ops.diff_attention_extend_paged(q, *kv, coef, tbl, pos, counts)
        return ops.diff_attention_extend_paged_fp8(q, *kv, coef, tbl, pos, counts)

    def rows_rows(self, kv, q, coef, tbl, pos, counts):
        if self.kv_dtype is None:
            return ops.diff_attention_decode_rows_paged(q, *kv, coef, tbl, pos, counts)
        return ops.diff_attention_decode_rows_paged_fp8(q, *kv, coef, tbl, pos, counts)

    # ---- shared-prefix plan (host only: no device read, no sync)
    def shared_groups(self, seqs: Sequence[int]):
        """Which of ``seqs`` (a step's sequences, in batch order) reach their first rows through
        the same pool pages.  Sequences are gathered by their first page; a set of more than 8 is
        cut into sets of at most 8; a set shares the pages its lists have in common from the start,
        and its shared rows are those pages' rows cut to the smallest ``host_low`` of the set (the
        exact lower bound of a length, so a device-side ``active`` mask cannot make it too large).
        Sets of one and sets that share less than one decode chunk are dropped.  Returns
        (groups of batch indices, shared rows), from ``pages``, ``host_low`` and ``page_size`` alone."""
        first: Dict[int, List[int]] = {}
        for b, q in enumerate(seqs):
            if self.pages[q]:
                first.setdefault(self.pages[q][0], []).append(b)
        groups, rows = [], []
        for members in first.values():
            for at in range(0, len(members), ops.SHARED_GROUP_MAX):
                part = members[at:at + ops.SHARED_GROUP_MAX]
                if len(part) < 2:
                    continue
                lists = [self.pages[seqs[b]] for b in part]
                common = 0
                while all(len(pl) > common and pl[common] == lists[0][common] for pl in lists):
                    common += 1
                n = min(common * self.page_size, min(self.host_low[seqs[b]] for b in part))
                if n >= SHARED_MIN_ROWS:
                    groups.append(tuple(part))
                    rows.append(n)
        return groups, rows

    def _step_plan(self, seqs: Sequence[int], device):
        """The step's ``ops.SharedDecodePlan``: the kept one while the step's sequences and their
        page lists stand as they stood when it was made, else a new one (one upload)."""
        key = (tuple(seqs), tuple(tuple(self.pages[q]) for q in seqs))
        if key != self._shared_key:
            groups, rows = self.shared_groups(seqs)
            self._shared_kept = ops.shared_decode_plan(groups, rows, len(seqs), device)
            self._shared_key = key
        return self._shared_kept

    def cache_bytes(self) -> int:
        """Bytes the pools of every layer hold (spare pages included)."""
        return sum(t.numel() * t.element_size() for d in (self.pool, self.scale_pool) for t in d.values())

    def _ensure(self, block_size: int, device) -> None:
        if self.block_table is None:
            self.max_pages = -(-block_size // self.page_size)
            self.block_table = torch.full((self.max_seqs, self.max_pages), -1, dtype=torch.int32, device=device)
            self.lengths = torch.zeros(self.max_seqs, dtype=torch.int32, device=device)

    def pages_in_use(self) -> int:
        return self.num_pages - len(self.free)

    # ---- host allocator
    def _need(self, n: int) -> int:
        return -(-n // self.page_size)

    def _drop(self, page: int) -> None:
        self.refcount[page] -= 1
        if self.refcount[page] == 0:
            self.free.append(page)

    def _check_live(self, seqs: Sequence[int]) -> List[int]:
        seqs = [int(q) for q in seqs]
        if self.block_table is None:
            raise ValueError("a prefilled PagedKVCache is needed: run prefill_paged first")
        for q in seqs:
            if q not in self.slot:
                raise ValueError(f"sequence {q} is not live in this cache (never made, or released)")
        if len(set(seqs)) != len(seqs):
            raise ValueError("a sequence is named twice")
        return seqs

    def _plan_writes(self, seqs: Sequence[int], upto: Sequence[int]):
        """What sequence q needs before it writes rows below ``upto[q]``: fresh pages past
        its list and a copy of every page it shares (refcount > 1) from the page of its
        lowest possible write position on.  Returns (copies [(seq, index)], grow [(seq, n)],
        pages needed); changes nothing."""
        rc: Dict[int, int] = {}
        copies, grow, need = [], [], 0
        for q, end in zip(seqs, upto):
            have = self.pages[q]
            for i in range(self.host_low[q] // self.page_size, min(self._need(end), len(have))):
                pg = have[i]
                if rc.get(pg, self.refcount[pg]) > 1:
                    rc[pg] = rc.get(pg, self.refcount[pg]) - 1
                    copies.append((q, i))
                    need += 1
            more = self._need(end) - len(have)
            if more > 0:
                grow.append((q, more))
                need += more
        return copies, grow, need

    def _prepare_writes(self, seqs: Sequence[int], upto: Sequence[int]) -> None:
        """Take the pages ``_plan_writes`` asks for (``OutOfPages`` first, if they are not
        there), copy the shared ones on the device in every layer and repoint the tables."""
        copies, grow, need = self._plan_writes(seqs, upto)
        if need > len(self.free):
            raise OutOfPages(f"{need} pages needed, {len(self.free)} of {self.num_pages} free")
        src, dst = [], []
        for q, i in copies:
            old, new = self.pages[q][i], self.free.pop()
            self.refcount[new] = 1
            self._drop(old)
            self.pages[q][i] = new
            src.append(old)
            dst.append(new)
            self._dirty_rows.add(q)
        for q, more in grow:
            for _ in range(more):
                new = self.free.pop()
                self.refcount[new] = 1
                self.pages[q].append(new)
            self._dirty_rows.add(q)
        if src:
            for buf in list(self.pool.values()) + list(self.scale_pool.values()):    # fp8: bytes and their scales
                buf.index_copy_(0, torch.tensor(dst, device=buf.device),
                                buf.index_select(0, torch.tensor(src, device=buf.device)))

    def _flush(self) -> None:
        dev = self.block_table.device
        rows = [q for q in self._dirty_rows if q in self.slot]
        if rows:
            tab = [self.pages[q] + [-1] * (self.max_pages - len(self.pages[q])) for q in rows]
            self.block_table.index_copy_(0, torch.tensor([self.slot[q] for q in rows], device=dev),
                                         torch.tensor(tab, dtype=torch.int32, device=dev).view(-1, self.max_pages))
        lens = [q for q in self._dirty_lens if q in self.slot]
        if lens:
            self.lengths.index_copy_(0, torch.tensor([self.slot[q] for q in lens], device=dev),
                                     torch.tensor([self.host_lengths[q] for q in lens], dtype=torch.int32, device=dev))
        self._dirty_rows.clear()
        self._dirty_lens.clear()

    def _trim(self, q: int) -> None:
        """Return the whole pages past sequence q's (exact) length."""
        keep = self._need(self.host_lengths[q])
        if len(self.pages[q]) > keep:
            for pg in reversed(self.pages[q][keep:]):
                self._drop(pg)
            del self.pages[q][keep:]
            self._dirty_rows.add(q)

    def _new_seq(self, pages: List[int], length: int) -> int:
        q = self.next_id
        self.next_id += 1
        self.slot[q] = self.free_slots.pop()
        self.pages[q] = pages
        self.host_lengths[q] = self.host_low[q] = length
        self._dirty_rows.add(q)
        self._dirty_lens.add(q)
        return q

    # ---- public
    def sync(self) -> Dict[int, int]:
        """Refresh ``host_lengths`` from the device (one host sync) and return the pages
        that were taken for the upper bound only."""
        if self.block_table is not None and not self.host_exact:
            self._flush()
            dev = self.lengths.tolist()
            for q, sl in self.slot.items():
                self.host_lengths[q] = self.host_low[q] = dev[sl]
                self._trim(q)
        self.host_exact = True
        return self.host_lengths

    def release(self, seq: int) -> None:
        """Forget sequence ``seq``: every page of its list loses one reference, and the
        pages nobody else holds go back to the free list."""
        seq = int(seq)
        if seq not in self.slot:
            raise ValueError(f"sequence {seq} is not live in this cache (never made, or released twice)")
        for pg in reversed(self.pages.pop(seq)):
            self._drop(pg)
        self.free_slots.append(self.slot.pop(seq))
        del self.host_lengths[seq], self.host_low[seq]

    def truncate(self, seq: int, new_length: int) -> None:
        """Roll ``seq`` back to ``new_length <= its length`` and return the whole pages
        past it.  Nothing is erased: the kernels ignore rows past a length."""
        (seq,) = self._check_live([seq])
        self.sync()
        new_length = int(new_length)
        if not 0 <= new_length <= self.host_lengths[seq]:
            raise ValueError(f"sequence {seq}: cannot truncate length {self.host_lengths[seq]} to {new_length}")
        self.host_lengths[seq] = self.host_low[seq] = new_length
        self._dirty_lens.add(seq)
        self._trim(seq)
        self._shared_key = None                    # a kept plan's rows were cut to the lengths before

    def _rolled_back(self, seq: int, new_length: int) -> None:
        """The host half of ``truncate`` after a round whose lengths the device has already settled
        (``SpecRound``: ``ops.spec_commit_lengths``): ``seq`` holds ``new_length`` rows, the whole pages past
        them are returned.  No length is marked for upload."""
        self.host_lengths[seq] = self.host_low[seq] = int(new_length)
        self._trim(seq)
        self._shared_key = None                    # a kept plan's rows were cut to the lengths before

    def fork(self, seq: int) -> int:
        """A new sequence with the same content as ``seq``, sharing every one of its
        pages, a partial last page included (each refcount goes up by one; no device
        work).  Whichever of them first writes into a shared page takes a fresh page and
        copies the shared one there (copy on write, done by the next step)."""
        (seq,) = self._check_live([seq])
        self.sync()
        if not self.free_slots:
            raise RuntimeError(f"all {self.max_seqs} sequence slots are live (max_seqs)")
        for pg in self.pages[seq]:
            self.refcount[pg] += 1
        return self._new_seq(list(self.pages[seq]), self.host_lengths[seq])


def _paged_gather(cache: PagedKVCache, seqs: Sequence[int]):
    """The step's view of the device state: (slots, contiguous (B, max_pages) table, (B,) lengths)."""
    cache._flush()
    sl = torch.tensor([cache.slot[q] for q in seqs], device=cache.block_table.device)
    return sl, cache.block_table.index_select(0, sl), cache.lengths.index_select(0, sl)


@torch.no_grad()
def prefill_paged(model, prompts: Sequence[torch.Tensor], cache: PagedKVCache):
    """Add B prompts of different lengths (one-dimensional LongTensors, 1 .. block_size
    tokens each) to ``cache`` -- an empty one or a live one, so new sequences join a
    running batch -- in one fused right-padded causal forward, as ``prefill_ragged``:
    pages are taken for every prompt (``OutOfPages``, before anything changes, if the
    pool does not hold them), and each layer scatters its K_i / V rows
    into them.  Returns (sequence ids, (B, vocab) logits at each prompt's last token)."""
    bs = model.block_size
    lens = _check_prompts(prompts, bs)
    if not isinstance(cache, PagedKVCache):
        raise ValueError("prefill_paged needs a PagedKVCache")
    need = sum(cache._need(n) for n in lens)
    if need > len(cache.free):
        raise OutOfPages(f"{need} pages needed for {len(lens)} prompts, {len(cache.free)} of {cache.num_pages} free")
    if len(lens) > len(cache.free_slots):
        raise RuntimeError(f"{len(lens)} prompts, {len(cache.free_slots)} of {cache.max_seqs} sequence slots free "
                           "(max_seqs)")
    idx = torch.nn.utils.rnn.pad_sequence(list(prompts), batch_first=True)
    cache._ensure(bs, idx.device)
    seqs = []
    for n in lens:
        pages = [cache.free.pop() for _ in range(cache._need(n))]
        for pg in pages:
            cache.refcount[pg] = 1
        seqs.append(cache._new_seq(pages, n))
    _, tbl, counts = _paged_gather(cache, seqs)
    last = torch.tensor(lens, device=idx.device) - 1
    logits = _paged_model_step(model, idx, cache, tbl, None, counts, gather=last)
    return seqs, logits


@torch.no_grad()
def decode_paged(model, seqs: Sequence[int], tok: torch.Tensor, cache: PagedKVCache,
                 active: Optional[torch.Tensor] = None):
    """``decode_ragged`` over any subset ``seqs`` (B ids) of the live sequences: ``tok``
    (B, 1) is sequence seqs[b]'s token at its own length.  A sequence that crosses a page
    boundary takes one page first, one about to write into a shared page copies it
    (``OutOfPages`` before anything is written).  Returns (B, vocab) and advances the
    lengths by one.

    ``active``: optional device bool (B,), as for ``decode_ragged``: applied on the
    device, so ``host_lengths`` becomes an upper bound, pages are taken for the bound and
    ``sync()`` / ``release`` return the surplus."""
    if tok.dim() != 2 or tok.shape[1] != 1:
        raise ValueError("tok must be (B, 1)")
    bs = model.block_size
    if not isinstance(cache, PagedKVCache):
        raise ValueError("decode_paged needs a PagedKVCache")
    seqs = cache._check_live(seqs)
    if len(seqs) != tok.shape[0]:
        raise ValueError(f"batch size {tok.shape[0]} differs from the {len(seqs)} sequences named")
    have = [cache.host_lengths[q] for q in seqs]
    if active is None and max(have) + 1 > bs:
        raise ValueError(f"a sequence is at block_size {bs}: positions are absolute within the window, "
                         "the sliding window is the one-length path's job (last_logits)")
    cache._prepare_writes(seqs, [min(n + 1, bs) for n in have])
    if cache.use_graph:                           # the gather, the step and the length update are the graph's
        cache._flush()
        sl = torch.tensor([cache.slot[q] for q in seqs], device=tok.device)
        counts = (torch.ones(len(seqs), dtype=torch.int32, device=tok.device) if active is None
                  else active.to(torch.int32))
        logits = _seq_graph(model, cache, len(seqs), active is not None, tok.device, sl).step(tok, counts, sl)
    else:
        sl, tbl, pos = _paged_gather(cache, seqs)
        counts = torch.ones_like(pos) if active is None else active.to(torch.int32)
        if cache.shared_decode:                   # copy on write and growth have settled the tables
            cache.shared_plan = cache._step_plan(seqs, tok.device)
        try:
            logits = _paged_model_step(model, tok, cache, tbl, pos, counts, one_row=True)[:, 0]
        finally:
            cache.shared_plan = None
        cache.lengths.index_copy_(0, sl, pos + counts)
    for q, n in zip(seqs, have):
        cache.host_lengths[q] = min(n + 1, bs)
        if active is None and cache.host_low[q] == n:
            cache.host_low[q] = n + 1
    if active is not None:
        cache.host_exact = False
    return logits


@torch.no_grad()
def append_paged(model, seqs: Sequence[int], new_idx: torch.Tensor, counts, cache: PagedKVCache,
                 all_rows: bool = False):
    """``append_ragged`` over any subset ``seqs`` of the live sequences: seqs[b] is fed the
    first ``counts[b]`` tokens of ``new_idx[b]`` ((B, Tn), padded) at its own length, one
    ``diff_attention_extend_paged`` per layer (head sizes without an extend plan: one
    paged decode per row).  Pages are taken, and shared pages copied, for all of a
    sequence's new rows first (``OutOfPages`` before anything is written).  Returns, raises
    and splits the step near ``block_size`` as ``append_ragged`` does."""
    if new_idx.dim() != 2 or new_idx.shape[1] < 1:
        raise ValueError("new_idx must be (B, Tn) with Tn >= 1")
    B, Tn = new_idx.shape
    bs = model.block_size
    if not isinstance(cache, PagedKVCache):
        raise ValueError("append_paged needs a PagedKVCache")
    seqs = cache._check_live(seqs)
    if len(seqs) != B:
        raise ValueError(f"batch size {B} differs from the {len(seqs)} sequences named")
    cache.sync()
    have = [cache.host_lengths[q] for q in seqs]
    cnt = _check_counts(counts, seqs, have, Tn, bs)
    writers = [b for b in range(B) if cnt[b] > 0]
    cache._prepare_writes([seqs[b] for b in writers], [have[b] + cnt[b] for b in writers])
    sl, tbl, lens = _paged_gather(cache, seqs)
    out, cnt_dev = _append_parts(lambda idx, pos, c, last: _paged_model_step(model, idx, cache, tbl, pos, c, last),
                                 lens, have, cnt, new_idx, bs, all_rows)
    cache.lengths.index_copy_(0, sl, lens + cnt_dev)
    for q, n, c in zip(seqs, have, cnt):
        cache.host_lengths[q] = cache.host_low[q] = n + c
    return out


@torch.no_grad()
def generate_paged(model, prompts: Sequence[torch.Tensor], max_new_tokens: int, eos_id: Optional[int] = None,
                   n_samples: int = 1, num_pages: Optional[int] = None, page_size: int = 64, kv_dtype=None,
                   rows_decode: bool = False, shared_decode: bool = False, graph: bool = False,
                   fused_step: bool = False, sampler: Optional[Sampler] = None,
                   streams: Optional[Sequence[int]] = None, speculate: Optional[Speculation] = None,
                   penalties: Optional[Penalties] = None):
    """``generate_ragged`` on a ``PagedKVCache``: same prefill, same reference sampling
    (softmax of the last logits, one ``torch.multinomial`` over the whole batch), one
    window (``ValueError`` if a prompt plus ``max_new_tokens`` crosses ``block_size``), the
    same ``eos_id`` handling.  Returns a list of B one-dimensional tensors.

    ``n_samples > 1``: every prompt is prefilled once and forked ``n_samples - 1`` times,
    so its samples share the prompt's full pages (a partial last page is copied when a
    sample first writes into it); the batch is sample-major within a prompt, and the
    result is a list of B lists of ``n_samples`` tensors.  ``num_pages``: the pool size;
    default the exact need of the call (``OutOfPages`` if a given one is too small).
    ``kv_dtype``: ``PagedKVCache``'s (``"fp8_e4m3"``: the pages hold e4m3fn bytes and scales);
    ``rows_decode``: ``PagedKVCache``'s, for the multi-row steps made on the cache;
    ``shared_decode``: ``PagedKVCache``'s: each token's step reads the pages the samples of a
    prompt still share once per group of up to 8 samples (same logits, bit for bit);
    ``graph`` / ``fused_step``: ``PagedKVCache``'s (each token's step replays one captured HIP graph; its
    RoPE and row scatter are one launch; not with ``shared_decode``): same logits, bit for bit.
    ``sampler`` / ``streams``: ``generate_ragged``'s; sample j of prompt b draws from stream
    ``b * n_samples + j`` (``streams[b] * n_samples + j``), so the forks of one prompt differ.
    ``speculate``: ``generate_ragged``'s (not with ``n_samples > 1`` or ``shared_decode``); the pool is made
    with ``rows_decode=True``, a round takes pages for its drafted rows and ``truncate`` returns those of
    the rejected ones, so the default ``num_pages`` still holds the call; with ``Speculation(graph=True)`` the
    pages are taken before the round's replay and returned after the read of its result.
    ``penalties``: ``generate_ragged``'s; with ``n_samples > 1`` every sample has its own history row and its
    prompt's length as ``gen_start``, so each equals its own one-sample run."""
    bs = model.block_size
    if n_samples < 1:
        raise ValueError("n_samples must be >= 1")
    if penalties is not None:
        _check_penalties(penalties, sampler)
    if speculate is not None:
        _check_speculate(speculate, sampler, n_samples, shared_decode, penalties)
    for p in prompts:
        if p.shape[0] + max_new_tokens > bs:
            raise ValueError(f"a prompt of {p.shape[0]} tokens plus {max_new_tokens} new ones crosses "
                             f"block_size {bs}: the sliding window is the one-length path's job")
    if num_pages is None:
        num_pages = 0
        for p in prompts:
            n, end = p.shape[0], p.shape[0] + max(max_new_tokens - 1, 0)       # the last sample is never cached
            shared = n // page_size if end > n else -(-n // page_size)         # nothing written: all pages shared
            num_pages += shared + n_samples * (-(-end // page_size) - shared)
        num_pages = max(num_pages, 1)
    cache = PagedKVCache(num_pages, page_size, max_seqs=max(len(prompts) * n_samples, 1), kv_dtype=kv_dtype,
                          rows_decode=rows_decode or speculate is not None, shared_decode=shared_decode, graph=graph,
                          fused_step=fused_step)
    roots, logits = prefill_paged(model, prompts, cache)
    if speculate is not None and max_new_tokens >= 1:
        def roll_back(lengths):
            for q, n in zip(roots, lengths):
                if n < cache.host_lengths[q]:
                    cache.truncate(q, n)

        outs = _speculative_tokens(logits, prompts, max_new_tokens, eos_id, sampler,
                                   _stream_ids(streams, len(prompts), 1, logits.device), speculate, bs,
                                   lambda idx, counts: append_paged(model, roots, idx, counts, cache, all_rows=True),
                                   roll_back, (model, cache, roots), penalties)
        return [o.to(p.device) for o, p in zip(outs, prompts)]
    seqs = [q for root in roots for q in [root] + [cache.fork(root) for _ in range(n_samples - 1)]]
    outs = [p for p in prompts for _ in range(n_samples)]
    if max_new_tokens >= 1:
        if n_samples > 1:
            logits = logits.repeat_interleave(n_samples, dim=0)
        state = None if penalties is None else _PenaltyState.from_prompts(penalties, sampler, logits.shape[-1],
                                                                          logits.device, outs, max_new_tokens)
        toks, keep = _sample_tokens(logits, max_new_tokens, eos_id,
                                    lambda tok, active: decode_paged(model, seqs, tok, cache, active), sampler,
                                    _stream_ids(streams, len(prompts), n_samples, logits.device), state)
        outs = [torch.cat([p, toks[b, :keep[b]].to(p.device)]) for b, p in enumerate(outs)]
    else:
        outs = [p.clone() for p in outs]
    if n_samples == 1:
        return outs
    return [outs[b * n_samples:(b + 1) * n_samples] for b in range(len(prompts))]
