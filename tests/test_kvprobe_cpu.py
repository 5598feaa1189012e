"""The probes of tests/_kvprobe.py work, and they bite -- without a GPU.

A small torch model of the two cache algorithms stands in for the kernels: the split-key decode
(256-key chunks, a partial (m, l, acc) per chunk and branch, P rounded to the dtype, fp32
accumulation, a combine with exp(m_s - M) weights) and the two-pass extend (32-key tiles dealt to
``nw`` interleaved waves, a pass of per-wave online (m, l) and their merge, then P = sum_i coef_i /
l_i exp(s_i - m_i) rounded once to the dtype and one PV product per wave, summed).  Scores are fp32
from the stored inputs; the output is rounded once.  One keyword injects one fault:

    edge+1 / edge-1   the causal edge off by one key, either way
    drop_last         the last chunk / tile dropped
    drop_wave         wave 1's partials dropped in the merge (extend)
    no_rescale        the combine / merge without the exp(m_s - M) weights
    l_from_0          branch i >= 1 normalised with branch 0's l
    m_from_0          branch i >= 1 shifted with branch 0's maximum
    double_first      the first key of every chunk / tile counted twice
    k_scale_next / v_scale_next   an fp8 row's K / V scale taken from row j + 1 (fp8 storage)

The faultless model passes every probe at TOL[dtype] per (b, row, h) block in every dtype and on
both storages; every fault fails at least one named probe in every dtype (the table is printed: run
with -s); the last test records what the suite's randn case made of the same faults."""
import functools

import pytest
import torch

import _kvprobe as KP
from conftest import rel_err
from differential_transformer_replication_amd import ops

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
B, H, N, HS, DV = 2, 2, 2, 64, 128
CAP = 600
CHUNK, TILE, NW = 256, 32, 4
FAULTS = ["edge+1", "edge-1", "drop_last", "drop_wave", "no_rescale", "l_from_0", "m_from_0", "double_first"]
FP8_FAULTS = ["k_scale_next", "v_scale_next"]


# ------------------------------------------------------------------ the model ---
def _visible(n, fault):
    return n + 1 if fault == "edge+1" else max(n - 1, 1) if fault == "edge-1" else n


def model_decode(q, k, v, coef, L, dtype, fault=None):
    """One (b, h) block: q (N, hs), k (cap, N, hs), v (cap, dv), coef (N,), all fp32 holding stored values."""
    rd = lambda x: x.to(dtype).float()
    n = min(_visible(L, fault), k.shape[0])
    s = torch.einsum("jid,id->ij", k[:n], q) / q.shape[-1] ** 0.5            # (N, n) fp32
    bounds = [(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)]
    if fault == "drop_last" and len(bounds) > 1:
        bounds = bounds[:-1]
    Nn = q.shape[0]
    m = torch.empty(len(bounds), Nn)
    l = torch.empty(len(bounds), Nn)
    acc = torch.empty(len(bounds), Nn, v.shape[-1])
    for c, (lo, hi) in enumerate(bounds):
        idx = list(range(lo, hi))
        if fault == "double_first":
            idx = [lo] + idx
        sc, vc = s[:, idx], v[idx]
        m[c] = sc.amax(1)
        shift = m[c].clone()
        if fault == "m_from_0":
            shift[1:] = m[c, 0]
        p = torch.exp(sc - shift[:, None])
        l[c] = p.sum(1)
        acc[c] = rd(p) @ vc
    M = m.amax(0)
    w = torch.ones_like(m) if fault == "no_rescale" else torch.exp(m - M)
    Ls = (w * l).sum(0)
    if fault == "l_from_0":
        Ls[1:] = Ls[0]
    o = torch.einsum("i,ci,cie->e", coef / Ls, w, acc)
    return rd(o)


def model_extend(q, k, v, coef, pos, dtype, fault=None, nw=NW):
    """One (b, h) block: q (Tq, N, hs); rows in blocks of 32, each over the tiles up to its last row."""
    rd = lambda x: x.to(dtype).float()
    Tq, Nn, hs = q.shape
    out = torch.zeros(Tq, v.shape[-1])
    for r0 in range(0, Tq, 32):
        rows = range(r0, min(r0 + 32, Tq))
        reach = min(_visible(pos + rows[-1] + 1, fault), k.shape[0])
        ntiles = -(-reach // TILE)
        tiles = list(range(ntiles))
        if fault == "drop_last" and ntiles > 1:
            tiles = tiles[:-1]
        kk = k[:ntiles * TILE] if k.shape[0] >= ntiles * TILE else torch.cat([k, torch.zeros(ntiles * TILE - k.shape[0], Nn, hs)])
        vv = v[:ntiles * TILE] if v.shape[0] >= ntiles * TILE else torch.cat([v, torch.zeros(ntiles * TILE - v.shape[0], v.shape[-1])])
        R = len(rows)
        s = torch.einsum("jid,rid->rij", kk, q[r0:r0 + R]) / hs ** 0.5       # (R, N, keys)
        j = torch.arange(ntiles * TILE)
        vis = torch.tensor([min(_visible(pos + r + 1, fault), k.shape[0]) for r in rows])
        s = s.masked_fill(j[None, None, :] >= vis[:, None, None], float("-inf"))
        mult = torch.ones(ntiles * TILE)
        if fault == "double_first":
            mult[::TILE] = 2.0
        # pass 1: per-wave online statistics, then the merge
        mw = torch.full((nw, R, Nn), float("-inf"))
        lw = torch.zeros(nw, R, Nn)
        for kt in tiles:
            w = kt % nw
            st = s[..., kt * TILE:(kt + 1) * TILE]
            mn = torch.maximum(mw[w], st.amax(-1))
            ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
            e = torch.exp(st - ms[..., None]) * mult[kt * TILE:(kt + 1) * TILE]
            lw[w] = lw[w] * torch.exp(mw[w] - ms) + e.sum(-1)                # exp(-inf - ms) = 0: nothing carried yet
            mw[w] = mn
        waves = [w for w in range(nw) if not (fault == "drop_wave" and w == 1)]
        M = mw[waves].amax(0)
        wt = torch.exp(mw[waves] - M)
        wt = torch.where(torch.isnan(wt), torch.zeros_like(wt), wt)
        if fault == "no_rescale":
            wt = torch.ones_like(wt) * (~torch.isinf(mw[waves]))
        lsum = (wt * lw[waves]).sum(0)
        if fault == "l_from_0":
            lsum[:, 1:] = lsum[:, :1]
        shift = M.clone()
        if fault == "m_from_0":
            shift[:, 1:] = M[:, :1]
        # pass 2: the combined P, rounded once, one PV product per wave
        o = torch.zeros(R, v.shape[-1])
        for kt in tiles:
            if fault == "drop_wave" and kt % nw == 1:
                continue
            st = s[..., kt * TILE:(kt + 1) * TILE]
            p = (torch.exp(st - shift[..., None]) * (coef / lsum)[..., None]).sum(1) * mult[kt * TILE:(kt + 1) * TILE]
            o += rd(p) @ vv[kt * TILE:(kt + 1) * TILE]
        out[r0:r0 + R] = rd(o)
    return out


# ------------------------------------------------------------------ the probes ---
def _dims(Tq):
    return (B, Tq, H, N, HS, DV)


def _dec(L):
    return (L - 1,) * B


@functools.lru_cache(maxsize=None)
def probes():
    """name -> (op, case).  Each (b, h) block of a planted case carries its own key, branch and gap."""
    ext = (63,) * B
    return {
        "decode planted L=5 (keys 4, 0; invisible 5)": ("decode", KP.planted(_dims(1), CAP, _dec(5), {
            (0, 0): [(4, 0, 8.0)], (0, 1): [(5, 1, 8.0)], (1, 0): [(0, 1, 40.0)], (1, 1): [(5, 0, 40.0)]}, 1)),
        "decode planted L=257 (key 256; invisible 257)": ("decode", KP.planted(_dims(1), CAP, _dec(257), {
            (0, 0): [(256, 0, 8.0)], (0, 1): [(256, 1, 40.0)], (1, 0): [(257, 0, 8.0)], (1, 1): [(257, 1, 40.0)]}, 2)),
        "decode planted L=600 (keys 0, 255, 512, 599)": ("decode", KP.planted(_dims(1), CAP, _dec(600), {
            (0, 0): [(0, 1, 40.0)], (0, 1): [(255, 0, 8.0)], (1, 0): [(512, 1, 8.0)], (1, 1): [(599, 0, 40.0)]}, 3)),
        "decode ramp L=600": ("decode", KP.ramp(_dims(1), CAP, _dec(600), 4)),
        "decode ramp L=257": ("decode", KP.ramp(_dims(1), CAP, _dec(257), 5)),
        "decode cancelling L=600": ("decode", KP.cancelling(_dims(1), CAP, _dec(600), 6)),
        "extend planted own / next keys (63, 70)": ("extend", KP.planted(_dims(70), 160, ext, {
            (0, 0): [("own", 0, 8.0)], (0, 1): [("next", 1, 40.0)], (1, 0): [("next", 0, 8.0)], (1, 1): [("own", 1, 40.0)]}, 7)),
        "extend planted keys 0, 31, 32, 64 (63, 70)": ("extend", KP.planted(_dims(70), 160, ext, {
            (0, 0): [(0, 0, 40.0)], (0, 1): [(31, 1, 8.0)], (1, 0): [(32, 0, 8.0)], (1, 1): [(64, 1, 40.0)]}, 8)),
        "extend ramp (63, 70)": ("extend", KP.ramp(_dims(70), 160, ext, 9)),
        "extend cancelling (63, 70)": ("extend", KP.cancelling(_dims(70), 160, ext, 10)),
    }


@functools.lru_cache(maxsize=None)
def _stored(name, dtype, fp8):
    """The stored values of a probe and their oracle: (q, k, v, coef, pos, want, D, extras)."""
    _, case = probes()[name]
    if not fp8:
        q, k, v = (t.float() for t in KP.stored(case, dtype))
        extras = None
    else:
        case = KP.scaled_rows(case, seed=len(name), flip=len(name) % 2 == 1)
        q, kb, vb, sc, k, v = KP.stored_fp8(case, dtype, ops.kv_quant_reference)
        q = q.float()
        extras = (kb.view(torch.float8_e4m3fn).float(), vb.view(torch.float8_e4m3fn).float(), sc)
    want, D = KP.oracle(q, k, v, case.coef, case.pos)
    return q, k, v, case.coef, case.pos, want, D, extras


def _model(name, dtype, fp8, fault):
    op, _ = probes()[name]
    q, k, v, coef, pos, want, D, extras = _stored(name, dtype, fp8)
    if fault in FP8_FAULTS:
        kq, vq, sc = extras
        nxt = torch.roll(sc, -1, dims=1)
        if fault == "k_scale_next":
            k = kq * nxt[..., :N, None]
        else:
            v = vq * nxt[..., N, None]
    got = torch.zeros_like(want, dtype=torch.float32)
    for b in range(B):
        for h in range(H):
            if op == "decode":
                got[b, 0, h] = model_decode(q[b, 0, h], k[b, :, h], v[b, :, h], coef[h], pos[b] + 1, dtype, fault)
            else:
                got[b, :, h] = model_extend(q[b, :, h], k[b, :, h], v[b, :, h], coef[h], pos[b], dtype, fault)
    return KP.probe_err(got, want, D)


# ------------------------------------------------------------------- the tests ---
def test_builders_are_deterministic_and_planted_rows_are_well_conditioned():
    probes.cache_clear()
    first = {n: c for n, (_, c) in probes().items()}
    probes.cache_clear()
    for name, (_, c) in probes().items():
        for f in ("q", "k", "v", "coef"):
            assert torch.equal(getattr(c, f), getattr(first[name], f)), (name, f)
        assert c.hot == first[name].hot
    for name, (op, c) in probes().items():
        if c.kind != "planted":
            continue
        want, D = KP.oracle(c.q, c.k, c.v, c.coef, c.pos)
        for b, j, h, i, gap, p in KP.p_top(c):
            r = min(max(j - c.pos[b], 0), c.Tq - 1)
            ratio = (D[b, r, h].amax() / want[b, r, h].abs().amax()).item()
            if op == "decode":
                print(f"{name}: b={b} h={h} key {j} branch {i} gap {gap:.0f}: p_top {p:.15f}, D / |want| {ratio:.2f}")
            assert ratio <= 16.0, (name, b, h, ratio)
            if gap == 40.0 and op == "decode":
                assert p > 1 - 1e-12, (name, b, h, p)
            if gap == 8.0 and op == "decode":
                assert 0.5 < p < 0.999, (name, b, h, p)


def test_a_key_planted_in_both_branches_of_1_minus_1_cancels():
    dims, pos = _dims(1), _dec(257)
    both = KP.planted(dims, CAP, pos, {(b, h): [(100, 0, 40.0), (100, 1, 40.0)] for b in range(B) for h in range(H)}, 11)
    one = KP.planted(dims, CAP, pos, {(b, h): [(100, 0, 40.0)] for b in range(B) for h in range(H)}, 11)
    for c in (both, one):
        c.coef = torch.tensor([[1.0, -1.0]] * H)
    wb, Db = KP.oracle(both.q, both.k, both.v, both.coef, pos)
    wo, _ = KP.oracle(one.q, one.k, one.v, one.coef, pos)
    assert wb.abs().max() <= 1e-9 * Db.max()                 # one-hot on the same key in both maps: V[j*] - V[j*]
    assert wo.abs().amax(-1).min() >= 0.99 * KP.V_HOT        # in one branch it is the whole row
    assert Db.amax(-1).min() >= 1.9 * KP.V_HOT


def test_an_invisible_key_does_not_move_the_oracle_and_a_visible_one_does():
    dims, pos = _dims(1), _dec(257)
    spots = lambda j: {(b, h): [(j, h, 8.0)] for b in range(B) for h in range(H)}
    past, last = KP.planted(dims, CAP, pos, spots(257), 12), KP.planted(dims, CAP, pos, spots(256), 12)
    plain = KP.planted(dims, CAP, pos, {}, 12)
    assert torch.equal(past.q, plain.q) and not torch.equal(past.k, plain.k)
    wp, _ = KP.oracle(past.q, past.k, past.v, past.coef, pos)
    w0, D0 = KP.oracle(plain.q, plain.k, plain.v, plain.coef, pos)
    wl, _ = KP.oracle(last.q, last.k, last.v, last.coef, pos)
    assert torch.equal(wp, w0)
    assert ((wl - w0).abs().amax(-1) >= 50.0).all() and (w0.abs().amax(-1) <= 1.0).all()


@pytest.mark.parametrize("fp8", [False, True], ids=["plain", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_faultless_model_passes_every_probe(dtype, fp8):
    for name in probes():
        err = _model(name, dtype, fp8, None)
        print(f"{'fp8' if fp8 else 'plain'} {dtype} {name}: worst probe_err {err.max().item():.3e} (bar {KP.TOL[dtype]:.0e})")
        assert (err <= KP.TOL[dtype]).all(), (name, dtype, fp8, err.max().item())


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_fault_fails_a_named_probe(dtype):
    table = {}
    for fault in FAULTS + FP8_FAULTS:
        fp8 = fault in FP8_FAULTS
        for name, (op, _) in probes().items():
            if fault == "drop_wave" and op != "extend":
                continue
            worst = _model(name, dtype, fp8, fault).max().item()
            if not worst <= KP.TOL[dtype]:
                table.setdefault(fault, []).append((name, worst))
    for fault in FAULTS + FP8_FAULTS:
        for name, worst in table.get(fault, []):
            print(f"{dtype} {fault:>13}: fails {name} at {worst:.2e}")
    for fault in FAULTS + FP8_FAULTS:
        caught = {n.split()[0] for n, _ in table.get(fault, [])}
        want = {"extend"} if fault == "drop_wave" else {"decode", "extend"}
        assert caught >= want, (dtype, fault, "no probe of", want - caught, "notices this fault")


def test_the_randn_case_under_the_tensor_wide_norm_for_the_record():
    """The suite's own case (test_gpu_ragged._dec_inputs, bf16, lengths 257 and 600) judged by
    conftest.rel_err at the suite's bar of 2e-2, with the faults above.  The issue behind this file
    expected a causal edge off by one and a neighbour's scale to pass there.  Measured, they do not
    quite: an edge off by one scores 2.1e-2 .. 2.6e-2 (L = 257 / 600; the faultless model 2.6e-3), so
    the old tests stand 1.05 .. 1.3 x above their bar on it, where the planted probes stand 20 .. 50 x
    above the same bar; a dropped chunk, a missing rescale and the per-branch statistics score 3.7e-2 ..
    0.5; the neighbour's-scale faults on test_gpu_fp8_cache._inputs' rows (scales 0.25 .. 2.25) score
    0.6 .. 1.1.  So nothing is asserted to pass here: the figures are printed, the faultless model is
    held to the bar, and an edge fault is held to at least 10 x the bar on the planted probes."""
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(11 * N + HS + DV)
    q = torch.randn(B, H, N, HS, generator=g)
    k = torch.randn(B, CAP, H, N, HS, generator=g)
    v = torch.randn(B, CAP, H, DV, generator=g)
    coef = torch.randn(H, N, generator=g) * 0.5
    coef[:, 0] = 1.0
    qs, ks, vs = (t.to(dtype).float() for t in (q, k, v))
    for L in (257, 600):
        want, _ = KP.oracle(qs[:, None], ks, vs, coef, _dec(L))
        for fault in [None] + [f for f in FAULTS if f != "drop_wave"]:
            got = torch.stack([torch.stack([model_decode(qs[b, h], ks[b, :, h], vs[b, :, h], coef[h], L, dtype, fault)
                                            for h in range(H)]) for b in range(B)])
            worst = max(rel_err(got[b], want[b, 0]) for b in range(B))
            print(f"randn bf16 L={L} fault {fault}: rel_err {worst:.3e}")
            if fault is None:
                assert worst <= 2e-2
    name = "decode planted L=257 (key 256; invisible 257)"
    for fault in ("edge+1", "edge-1"):
        assert _model(name, dtype, False, fault).max().item() >= 10 * KP.TOL[dtype], fault
