"""The probes of tests/_kvprobe.py through every KV-cache attention op.

Inputs: planted keys (gap 8 and gap 40 nats, one branch at a time, another key, branch and gap in
every (b, h) block of B = 2, H = 2), score ramps of 30 nats that run opposite ways in even and odd
branches, coef summing to zero over nearly equal maps, and for the fp8 pools the same cases with
stored scales spread over four decades.  Each result is judged against ``diff_core`` in fp64 on the
values as stored with ``probe_err`` (max_c |got - want| / max_c D per (b, row, h), D the
un-cancelled magnitude) at ``TOL[dtype]`` on every block, and the bitwise relations the ops
document are asserted on the same inputs.  tests/test_kvprobe_cpu.py shows which defect each probe
is for.  Every check prints one ``kv_probe`` line; profiles/kv_probe_errors.json keeps their worst.

Shapes (N, hs, dv): the split-key plan, the single-pass decode, and two the extend alone takes."""
import functools

import pytest
import torch

import _kvprobe as KP
import test_gpu_decode_shared as SH
import test_gpu_fp8_cache as F8
import test_gpu_paged as PG

from differential_transformer_replication_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = KP.TOL
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
B, H = 2, 2
SPLIT = [(2, 64, 128), (1, 64, 64), (3, 32, 64), (4, 32, 64)]
SINGLE = [(2, 16, 32), (2, 48, 96)]
EXTEND_ONLY = [(8, 16, 32), (2, 128, 256)]
P = 32
DEC_CAP = 600                                    # three 256-key chunks, the last one partial
DEC_LENGTHS = (1, 256, 257, 512, 513, 600)
EXT_CASES = [(31, 2, 64), (63, 70, 160), (200, 57, 300)]       # (pos, Tq, cap); the last does not fill four waves
ROWS_CAP = 320
ROWS_TQS = [2, 5, 8]
_i32 = PG._i32


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _round_up(n, p):
    return -(-n // p) * p


def _slots(probes, N, salt=0):
    """Deal (where, gap) probes to the four (b, h) blocks, four to a case, the branch cycling; the
    last case is filled up from the front with the other gap's branch order."""
    cases = []
    for c in range(0, len(probes), B * H):
        group = list(probes[c:c + B * H])
        fill = 0
        while len(group) < B * H:
            group.append(probes[fill])
            fill += 1
        cases.append({(s // H, s % H): [(where, (c + s + salt + (s >= len(probes) - c)) % N, gap)]
                      for s, (where, gap) in enumerate(group)})
    return cases


def _judge(family, kind, dtype, got, want, D, tag):
    got = got.view(want.shape).float().cpu()
    assert torch.isfinite(got).all(), (family, kind, tag, "not finite")
    err = KP.probe_err(got, want, D)
    print(f"kv_probe {family} {_name(dtype)} {kind}: worst probe_err {err.max().item():.3e} (bar {TOL[dtype]:.0e}) {tag}")
    bad = (~(err <= TOL[dtype])).nonzero().tolist()
    assert not bad, (family, kind, tag, "blocks (b, row, h) over the bar", bad[:8], err.max().item())


def _plain(case, dtype):
    q, k, v = KP.stored(case, dtype)
    return q.to(DEV), k.to(DEV), v.to(DEV), case.coef.to(DEV)


def _plain_oracle(case, dtype, counts=None):
    q, k, v = (t.float() for t in KP.stored(case, dtype))
    return KP.oracle(q, k, v, case.coef, case.pos, counts)


def _fp8(case, dtype, seed, counts=None):
    """The case re-scaled for the fp8 pool (planted keys on small rows between large ones when the
    seed is even, the other way round when odd): q on the device, the host bytes and scales, the
    oracle on the dequantised rows."""
    c8 = KP.scaled_rows(case, seed=seed, flip=seed % 2 == 1)
    q, kb, vb, sc, k, v = KP.stored_fp8(c8, dtype, ops.kv_quant_reference)
    want, D = KP.oracle(q.float(), k, v, c8.coef, c8.pos, counts)
    return c8, q.to(DEV), kb, vb, sc, want, D


# ------------------------------------------------------------------ decode ---
@functools.lru_cache(maxsize=None)
def _decode_cases(N, hs, dv, L):
    dims, pos = (B, 1, H, N, hs, dv), (L - 1,) * B
    keys = sorted({j for j in (0, 255, 256, 511, 512, L - 1) if j < L})
    if L < DEC_CAP:
        keys.append(L)                           # the first invisible key: finite, so no NaN check sees a read of it
    probes = [(j, gap) for j in keys for gap in KP.GAPS]
    cases = [("planted", KP.planted(dims, DEC_CAP, pos, spots, seed=1000 * L + 10 * n + N + hs))
             for n, spots in enumerate(_slots(probes, N))]
    if L == DEC_CAP:
        cases.append(("ramp", KP.ramp(dims, DEC_CAP, pos, seed=L + N + hs)))
        if N >= 2:
            cases.append(("cancelling", KP.cancelling(dims, DEC_CAP, pos, seed=L + N + hs + 1)))
    return cases


@functools.lru_cache(maxsize=None)
def _decode_oracle(N, hs, dv, L, n, dtype):
    return _plain_oracle(_decode_cases(N, hs, dv, L)[n][1], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("N,hs,dv", SPLIT + SINGLE)
def test_decode_probes(dtype, N, hs, dv):
    cap = _round_up(DEC_CAP, P)
    for L in DEC_LENGTHS:
        for n, (kind, case) in enumerate(_decode_cases(N, hs, dv, L)):
            tag = (N, hs, dv, L, n, case.hot)
            qd, kd, vd, cd = _plain(case, dtype)
            qd, ln = qd[:, 0], _i32([L] * B)
            want, D = _decode_oracle(N, hs, dv, L, n, dtype)
            host = ops.diff_attention_decode(qd, kd, vd, cd, L)
            dev = ops.diff_attention_decode(qd, kd, vd, cd, DEC_CAP, length_dev=_i32([L]))
            assert torch.equal(host, dev), (tag, "host length != device length")
            ragged = ops.diff_attention_decode_ragged(qd, kd, vd, cd, ln)
            k_pool, v_pool, table, k_cap, v_cap = PG._paginate(kd, vd, [DEC_CAP] * B, P, cap, seed=L + n)
            paged = ops.diff_attention_decode_paged(qd, k_pool, v_pool, cd, table, ln)
            same = ops.diff_attention_decode_ragged(qd, k_cap, v_cap, cd, ln)
            assert torch.equal(paged, same), (tag, "paged != ragged on the gathered cache")
            for family, got in (("decode", host), ("decode_ragged", ragged), ("decode_paged", paged)):
                _judge(family, kind, dtype, got, want, D, tag)
            c8, q8, kb, vb, sc, want8, D8 = _fp8(case, dtype, seed=L + n)
            kq, vq, scales, table8 = F8._paginate(kb, vb, sc, [DEC_CAP] * B, P, cap, seed=L + n + 1)
            got8 = ops.diff_attention_decode_paged_fp8(q8[:, 0], kq, vq, scales, c8.coef.to(DEV), table8, ln)
            _judge("decode_paged_fp8", kind, dtype, got8, want8, D8, tag)


# ------------------------------------------------------------------ extend ---
@functools.lru_cache(maxsize=None)
def _extend_cases(N, hs, dv, pos, Tq, cap):
    dims, p = (B, Tq, H, N, hs, dv), (pos,) * B
    diag = pos // 32 * 32                        # the first key of row 0's diagonal tile
    probes = [(w, gap) for w in ("own", "next", 0, 31, diag) for gap in KP.GAPS]
    cases = [("planted", KP.planted(dims, cap, p, spots, seed=100 * pos + 10 * n + N + hs))
             for n, spots in enumerate(_slots(probes, N))]
    cases.append(("ramp", KP.ramp(dims, cap, p, seed=pos + N + hs)))
    if N >= 2:
        cases.append(("cancelling", KP.cancelling(dims, cap, p, seed=pos + N + hs + 1)))
    return cases


@functools.lru_cache(maxsize=None)
def _extend_oracle(N, hs, dv, pos, Tq, cap, n, dtype):
    return _plain_oracle(_extend_cases(N, hs, dv, pos, Tq, cap)[n][1], dtype)


def _short(want, D, counts):
    """The oracle of a ragged step: rows >= counts[b] are zeros (the rows below are unchanged: causal)."""
    want, D = want.clone(), D.clone()
    for b, n in enumerate(counts):
        want[b, n:] = 0
        D[b, n:] = 0
    return want, D


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("N,hs,dv", SPLIT + SINGLE + EXTEND_ONLY)
def test_extend_probes(dtype, N, hs, dv):
    assert ops.extend_supported(dtype, hs, N, dv)
    assert ops.extend_fp8_supported(dtype, hs, N, dv) == (N <= 4)          # a missing plan cannot hide
    for pos, Tq, cap0 in EXT_CASES:
        cap = _round_up(cap0, P)
        for n, (kind, case) in enumerate(_extend_cases(N, hs, dv, pos, Tq, cap0)):
            tag = (N, hs, dv, pos, Tq, n)
            qd, kd, vd, cd = _plain(case, dtype)
            pd, counts = _i32([pos] * B), (Tq, 1)
            want, D = _extend_oracle(N, hs, dv, pos, Tq, cap0, n, dtype)
            _judge("extend", kind, dtype, ops.diff_attention_extend(qd, kd, vd, cd, pos), want, D, tag)
            short = ops.diff_attention_extend_ragged(qd, kd, vd, cd, pd, _i32(counts))
            _judge("extend_ragged", kind, dtype, short, *_short(want, D, counts), tag)
            k_pool, v_pool, table, k_cap, v_cap = PG._paginate(kd, vd, [cap0] * B, P, cap, seed=pos + n)
            paged = ops.diff_attention_extend_paged(qd, k_pool, v_pool, cd, table, pd)
            same = ops.diff_attention_extend_ragged(qd, k_cap, v_cap, cd, pd)
            assert torch.equal(paged, same), (tag, "paged != ragged on the gathered cache")
            _judge("extend_paged", kind, dtype, paged, want, D, tag)
            if N <= 4:
                c8, q8, kb, vb, sc, want8, D8 = _fp8(case, dtype, seed=pos + n)
                kq, vq, scales, table8 = F8._paginate(kb, vb, sc, [cap0] * B, P, cap, seed=pos + n + 1)
                got8 = ops.diff_attention_extend_paged_fp8(q8, kq, vq, scales, c8.coef.to(DEV), table8, pd)
                _judge("extend_paged_fp8", kind, dtype, got8, want8, D8, tag)


# -------------------------------------------------------------------- rows ---
def _rows_pos(Tq):
    """Both steps straddle key 256: sequence 0's early rows see nothing of chunk 1 and one row's own
    key is its first key; sequence 1's last row is that row."""
    return (256 - Tq // 2, 257 - Tq)


@functools.lru_cache(maxsize=None)
def _rows_cases(N, hs, dv, Tq):
    dims, pos = (B, Tq, H, N, hs, dv), _rows_pos(Tq)
    probes = [(w, gap) for w in ("own", "next", 256, 255, 0) for gap in KP.GAPS][:8]
    cases = [("planted", KP.planted(dims, ROWS_CAP, pos, spots, seed=100 * Tq + 10 * n + N + hs))
             for n, spots in enumerate(_slots(probes, N, salt=1))]
    cases.append(("ramp", KP.ramp(dims, ROWS_CAP, pos, seed=Tq + N + hs)))
    if N >= 2:
        cases.append(("cancelling", KP.cancelling(dims, ROWS_CAP, pos, seed=Tq + N + hs + 1)))
    return cases


@functools.lru_cache(maxsize=None)
def _rows_oracle(N, hs, dv, Tq, n, dtype):
    return _plain_oracle(_rows_cases(N, hs, dv, Tq)[n][1], dtype)


@pytest.mark.parametrize("Tq", ROWS_TQS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("N,hs,dv", SPLIT)
def test_rows_probes(dtype, N, hs, dv, Tq):
    assert ops.decode_rows_supported(dtype, hs, N, dv, Tq) and ops.decode_rows_supported(dtype, hs, N, dv, Tq, fp8=True)
    pos = _rows_pos(Tq)
    pd = _i32(pos)
    for n, (kind, case) in enumerate(_rows_cases(N, hs, dv, Tq)):
        tag = (N, hs, dv, Tq, n)
        qd, kd, vd, cd = _plain(case, dtype)
        want, D = _rows_oracle(N, hs, dv, Tq, n, dtype)
        k_pool, v_pool, table, _, _ = PG._paginate(kd, vd, [ROWS_CAP] * B, P, ROWS_CAP, seed=Tq + n)
        c8, q8, kb, vb, sc, want8, D8 = _fp8(case, dtype, seed=Tq + n)
        kq, vq, scales, table8 = F8._paginate(kb, vb, sc, [ROWS_CAP] * B, P, ROWS_CAP, seed=Tq + n + 1)
        cd8 = c8.coef.to(DEV)
        rows = ops.diff_attention_decode_rows(qd, kd, vd, cd, pd)
        paged = ops.diff_attention_decode_rows_paged(qd, k_pool, v_pool, cd, table, pd)
        rows8 = ops.diff_attention_decode_rows_paged_fp8(q8, kq, vq, scales, cd8, table8, pd)
        for r in range(Tq):
            ln = _i32([p + r + 1 for p in pos])
            assert torch.equal(rows[:, r], ops.diff_attention_decode_ragged(qd[:, r], kd, vd, cd, ln)), (tag, r)
            assert torch.equal(paged[:, r], ops.diff_attention_decode_paged(qd[:, r], k_pool, v_pool, cd, table, ln)), (tag, r)
            assert torch.equal(rows8[:, r], ops.diff_attention_decode_paged_fp8(q8[:, r], kq, vq, scales, cd8, table8, ln)), (tag, r)
        _judge("decode_rows", kind, dtype, rows, want, D, tag)
        _judge("decode_rows_paged", kind, dtype, paged, want, D, tag)
        _judge("decode_rows_paged_fp8", kind, dtype, rows8, want8, D8, tag)


# ------------------------------------------------------------------ shared ---
SH_LENGTHS = (290, 300, 320, 270)                # three forks of one 256-row prompt, and a sequence of its own
SH_GROUPS, SH_ROWS = ((0, 1, 2),), (256,)


def _share(case):
    """The members hold the first member's first 256 rows."""
    for b in SH_GROUPS[0][1:]:
        case.k[b, :SH_ROWS[0]] = case.k[0, :SH_ROWS[0]]
        case.v[b, :SH_ROWS[0]] = case.v[0, :SH_ROWS[0]]
    return case


@functools.lru_cache(maxsize=None)
def _shared_cases(N, hs, dv):
    Bs = len(SH_LENGTHS)
    dims, pos = (Bs, 1, H, N, hs, dv), tuple(L - 1 for L in SH_LENGTHS)
    cases = []
    for n, (gs, gt) in enumerate(((8.0, 8.0), (40.0, 40.0), (40.0, 8.0))):
        # one key in the shared chunk (the same one for every fork: one direction u for the batch)
        # and another in each sequence's own tail, in another branch where there is one
        spots = {(b, h): [(100 + 20 * h, h % N, gs), (257 + 3 * b + h, (h + 1) % N, gt)] for b in range(Bs) for h in range(H)}
        cases.append(("planted", _share(KP.planted(dims, ROWS_CAP, pos, spots, seed=10 * n + N + hs, shared_u=True))))
    cases.append(("ramp", _share(KP.ramp(dims, ROWS_CAP, pos, seed=N + hs + 50, shared_u=True))))
    if N >= 2:
        cases.append(("cancelling", _share(KP.cancelling(dims, ROWS_CAP, pos, seed=N + hs + 51, shared_u=True))))
    return cases


@functools.lru_cache(maxsize=None)
def _shared_oracle(N, hs, dv, n, dtype):
    return _plain_oracle(_shared_cases(N, hs, dv)[n][1], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("N,hs,dv", SPLIT)
def test_shared_probes(dtype, N, hs, dv):
    assert ops.decode_shared_supported(dtype, hs, N, dv) and ops.decode_shared_supported(dtype, hs, N, dv, fp8=True)
    Bs = len(SH_LENGTHS)
    plan = ops.shared_decode_plan(SH_GROUPS, SH_ROWS, Bs, DEV)
    ln = _i32(SH_LENGTHS)
    for n, (kind, case) in enumerate(_shared_cases(N, hs, dv)):
        tag = (N, hs, dv, n)
        q, k, v = KP.stored(case, dtype)
        qd, cd = q[:, 0].to(DEV), case.coef.to(DEV)
        pools = SH._pools(k.float(), v.float(), P, ROWS_CAP, SH_LENGTHS, SH_GROUPS, SH_ROWS, dtype, seed=n)
        got = ops.diff_attention_decode_paged_shared(qd, *pools[:2], cd, pools[2], ln, plan)
        assert torch.equal(got, ops.diff_attention_decode_paged(qd, *pools[:2], cd, pools[2], ln)), (tag, "shared != paged")
        _judge("decode_paged_shared", kind, dtype, got, *_shared_oracle(N, hs, dv, n, dtype), tag)
        c8 = _share(KP.scaled_rows(case, seed=n, flip=n % 2 == 1))
        q8, kb, vb, sc, k8, v8 = KP.stored_fp8(c8, dtype, ops.kv_quant_reference)
        want8, D8 = KP.oracle(q8.float(), k8, v8, c8.coef, c8.pos)
        pools8 = SH._pools(c8.k, c8.v, P, ROWS_CAP, SH_LENGTHS, SH_GROUPS, SH_ROWS, seed=n + 1)
        q8d, cd8 = q8[:, 0].to(DEV), c8.coef.to(DEV)
        got8 = ops.diff_attention_decode_paged_shared_fp8(q8d, *pools8[:3], cd8, pools8[3], ln, plan)
        assert torch.equal(got8, ops.diff_attention_decode_paged_fp8(q8d, *pools8[:3], cd8, pools8[3], ln)), (tag, "fp8 shared != paged")
        _judge("decode_paged_shared_fp8", kind, dtype, got8, want8, D8, tag)


# -------------------------------------------------------------- wide chunks ---
def test_wide_chunk_probes():
    """ceil(t_cap / 256) * H * B >= 8192: the 512-key chunk plan, built as
    test_decode_paged_wide_chunk_plan_bitwise builds it (a table 16384 rows wide over a pool of a
    few pages).  Keys planted on both sides of the 512-key boundary and at the edges, and a ramp."""
    Bw, Hw, N, hs, dv, Pw, cap, rows, dtype = 8, 16, 2, 32, 64, 64, 16384, 576, torch.bfloat16
    assert -(-cap // 256) * Hw * Bw >= 8192
    lengths = (513, 511, 1, 40, 520, 512, 100, 515)
    dims, pos = (Bw, 1, Hw, N, hs, dv), tuple(L - 1 for L in lengths)
    spots = {}
    for b, L in enumerate(lengths):
        for h in range(Hw):
            j = (0, 255, 256, 511, 512, L - 1, L)[(b + h) % 7]
            spots[(b, h)] = [(j if j <= L else L - 1, h % N, KP.GAPS[(b + h // 2) % 2])]
    wide = lambda t: torch.cat([t, torch.full((Bw, cap // Pw - t.shape[1]), -1, dtype=torch.int32, device=DEV)], dim=1).contiguous()
    ln = _i32(lengths)
    for kind, case in (("planted", KP.planted(dims, rows, pos, spots, seed=77)), ("ramp", KP.ramp(dims, rows, pos, seed=78))):
        qd, kd, vd, cd = _plain(case, dtype)
        k_pool, v_pool, table, _, _ = PG._paginate(kd, vd, [rows] * Bw, Pw, rows, seed=5)
        got = ops.diff_attention_decode_paged(qd[:, 0], k_pool, v_pool, cd, wide(table), ln)
        _judge("decode_paged_wide", kind, dtype, got, *_plain_oracle(case, dtype), (kind,))
        c8, q8, kb, vb, sc, want8, D8 = _fp8(case, dtype, seed=6)
        kq, vq, scales, table8 = F8._paginate(kb, vb, sc, [rows] * Bw, Pw, rows, seed=7)
        got8 = ops.diff_attention_decode_paged_fp8(q8[:, 0], kq, vq, scales, c8.coef.to(DEV), wide(table8), ln)
        _judge("decode_paged_fp8_wide", kind, dtype, got8, want8, D8, (kind,))
