"""Helpers of the penalty tests: a pure-Python reading of include/diffattn.h's "Sampling penalties" on
``numpy.float32`` scalars, one operation at a time, and random cases (logits, histories, drafts, parameters)
that exercise every clamp of the definition."""
import numpy as np
import torch

F32 = np.float32
NINF = F32("-inf")


def _bits(x):
    return int(np.array(x, dtype=np.float32).view(np.uint32))


def _is_nan(x):
    return (_bits(x) & 0x7FFFFFFF) > 0x7F800000


def brute_force(logits, hist, hlen, gen_start, draft, dcnt, theta, pres, freq, gap, bias, Tn):
    """The definition over rows and columns.  ``logits``: (R, V) float32 array (already converted); ``hist`` /
    ``draft``: lists of lists; ``theta`` .. ``gap``: lists of B Python floats; ``bias``: None or a (B or 1, V)
    float32 array.  Returns the (R, V) float32 array."""
    R, V = logits.shape
    cap = len(hist[0])
    K = len(draft[0]) if draft is not None else 0
    out = np.empty((R, V), dtype=np.float32)
    with np.errstate(all="ignore"):
        for r in range(R):
            b, j = divmod(r, Tn)
            L = min(max(hlen[b], 0), cap)
            g = min(max(gen_start[b] if gen_start is not None else 0, 0), L)
            d = min(max(dcnt[b], 0), K) if draft is not None else 0
            e = min(j, d)
            seen, cnt = [False] * V, [0] * V
            for t in range(L):
                tok = hist[b][t]
                if 0 <= tok < V:
                    seen[tok] = True
                    cnt[tok] += t >= g
            for t in range(e):
                tok = draft[b][t]
                if 0 <= tok < V:
                    seen[tok] = True
                    cnt[tok] += 1
            th, f, p, gp = F32(theta[b]), F32(freq[b]), F32(pres[b]), F32(gap[b])
            row = []
            for i in range(V):
                x = F32(logits[r, i])
                if _is_nan(x):
                    row.append(x)
                    continue
                if not _is_nan(th) and th != F32(1) and seen[i]:
                    positive = _bits(x) != 0 and _bits(x) >> 31 == 0
                    x = F32(x / th) if positive else F32(x * th)
                if cnt[i] > 0 and not _is_nan(f) and not _is_nan(p):
                    x = F32(F32(x - F32(f * F32(cnt[i]))) - p)
                if bias is not None:
                    x = F32(x + bias[b if bias.shape[0] > 1 else 0, i])
                row.append(x)
            if np.isfinite(gp) and gp < 0:
                vals = [x for x in row if not _is_nan(x)]
                m = max(vals) if vals else NINF
                if np.isfinite(m):
                    thr = F32(m + gp)
                    row = [x if _is_nan(x) or x >= thr else NINF for x in row]
            for i in range(V):
                out[r, i] = row[i]
    return out


def same_bits(a, b):
    """fp32 tensors equal bit for bit (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def made_nans(want, logits):
    """Where the reference holds a NaN that the input did not: one the arithmetic made (inf - inf), whose
    payload include/diffattn.h leaves open."""
    return torch.isnan(want.cpu()) & ~torch.isnan(logits.float().cpu()).reshape(want.shape)


def same_but_made_nans(got, want, logits):
    """``same_bits`` everywhere but at the NaNs the arithmetic made, where ``got`` must hold a NaN too."""
    made = made_nans(want, logits)
    got, want = got.cpu(), want.cpu()
    zero = torch.zeros_like(want)
    return bool(torch.isnan(got[made]).all()) and same_bits(torch.where(made, zero, got), torch.where(made, zero, want))


def first_diff(a, b):
    """Where and how two fp32 tensors first differ in their bits, for an assertion's message."""
    ia, ib = a.contiguous().view(torch.int32).cpu().reshape(-1), b.contiguous().view(torch.int32).cpu().reshape(-1)
    bad = (ia != ib).nonzero().reshape(-1)
    if not bad.numel():
        return "equal"
    at = int(bad[0])
    return (f"{bad.numel()} of {ia.numel()} elements differ, first at flat index {at}: "
            f"{int(ia[at]) & 0xFFFFFFFF:#010x} != {int(ib[at]) & 0xFFFFFFFF:#010x}")


def i32(x):
    return torch.tensor(x, dtype=torch.int32)


class Case:
    """One call's CPU tensors.  Histories hold out-of-range and negative tokens; ``hlen`` cycles through
    0, 1, cap, mid values, one past cap and a negative; ``gen_start`` through 0, mid values, above ``hlen`` and a
    negative; ``dcnt`` through 0 .. K, above K and a negative (B = 8 reaches all of them).  With ``specials`` the
    logits hold -0, +0, -inf, a NaN and -- in column 2 of row 0, where both bias tensors are -inf -- a +inf: with a
    bias the sum there is a NaN that the arithmetic makes."""

    def __init__(self, B, Tn, V, dtype, cap=24, K=3, seed=0, draft=True, specials=True):
        g = torch.Generator().manual_seed(seed)
        R = B * Tn
        self.B, self.Tn, self.V, self.K, self.cap = B, Tn, V, K, cap
        x = (torch.randn(R, V, generator=g) * 4).to(dtype)
        if specials:
            x[0, 0] = -0.0
            x[R - 1, V // 2] = float("-inf")
            if V > 2:
                x[0, V - 1] = 0.0
                x[R // 2, 1] = float("nan")
                x[0, 2] = float("inf")
        self.logits = x
        self.hist = torch.randint(-2, V + 2, (B, cap), generator=g).to(torch.int32)
        if V > 4:                                                      # repeats, so counts above 1 occur
            self.hist[:, ::3] = torch.randint(0, min(V, 5), (B, len(range(0, cap, 3))), generator=g).to(torch.int32)
        hl = [cap // 2, cap, 0, 1, cap + 5, cap - 1, -3, 7]
        gs = [2, 0, 0, 5, 3, cap + 9, 1, -4]
        dc = [K, 1, K + 4, 0, 2, -1, K, 1]
        self.hlen = i32([hl[b % 8] for b in range(B)])
        self.gen_start = i32([gs[b % 8] for b in range(B)])
        self.draft = self.dcnt = None
        if draft:
            self.draft = torch.randint(-1, V + 1, (B, K), generator=g).to(torch.int32)
            self.dcnt = i32([dc[b % 8] for b in range(B)])
        self.bias = torch.randn(V, generator=g)
        self.bias[torch.rand(V, generator=g) < 0.2] = float("-inf")
        self.bias_rows = torch.randn(B, V, generator=g)
        self.bias_rows[torch.rand(B, V, generator=g) < 0.1] = float("-inf")
        if V > 2:
            self.bias[2] = self.bias_rows[:, 2] = float("-inf")
        self.per_seq = dict(repetition=torch.tensor([(1.3, 1.0, 0.8, 2.0)[b % 4] for b in range(B)]),
                            presence=torch.tensor([(0.4, 0.0, -0.3, 1.5)[b % 4] for b in range(B)]),
                            frequency=torch.tensor([(0.7, 0.25, 0.0, -0.1)[b % 4] for b in range(B)]),
                            floor_gap=torch.tensor([(-1.5, 0.0, -6.0, float("-inf"))[b % 4] for b in range(B)]))

    def features(self):
        """name -> keyword arguments: every feature alone, all together, all per sequence."""
        alone = dict(rep=dict(repetition=1.3), rep_up=dict(repetition=0.75), freq=dict(frequency=0.7),
                     pres=dict(presence=0.4), bias=dict(bias=self.bias), floor=dict(floor_gap=-1.5),
                     none=dict())
        alone["all"] = dict(repetition=1.3, frequency=0.7, presence=0.4, bias=self.bias, floor_gap=-1.5)
        alone["per_seq"] = dict(self.per_seq, bias=self.bias_rows)
        return alone

    def args(self, device="cpu", **kw):
        to = lambda t: None if t is None else t.to(device)              # noqa: E731
        kw = {k: to(v) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
        return dict(logits=to(self.logits), hist=to(self.hist), hlen=to(self.hlen), gen_start=to(self.gen_start),
                    draft=to(self.draft), dcnt=to(self.dcnt), rows_per_seq=self.Tn, **kw)

    def brute(self, **kw):
        per = lambda v, d: (v.tolist() if isinstance(v, torch.Tensor) else [d if v is None else v] * self.B)   # noqa: E731
        bias = kw.get("bias")
        return torch.from_numpy(brute_force(
            self.logits.float().numpy(), self.hist.tolist(), self.hlen.tolist(), self.gen_start.tolist(),
            None if self.draft is None else self.draft.tolist(), None if self.dcnt is None else self.dcnt.tolist(),
            per(kw.get("repetition"), 1.0), per(kw.get("presence"), 0.0), per(kw.get("frequency"), 0.0),
            per(kw.get("floor_gap"), 0.0), None if bias is None else bias.reshape(-1, self.V).numpy(), self.Tn))
