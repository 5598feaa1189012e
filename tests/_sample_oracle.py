"""The fp64 oracle of the row sampler (include/diffattn.h "Sampling"), in numpy, for test_sample_cpu.py and
test_gpu_sample.py.  It takes the fp32-converted logits of one row and follows the definition literally
(counts and masses of the strictly greater logits through a sort and ``searchsorted``); nothing here
comes from the kernel or from ``ops.sample_rows_reference``.

``D(V)`` is the longest fp32 add chain the kernel's documented shape has (csrc/sample.hip, DESIGN.md
"Sampling"), derived from that shape:

* the masked sum: a thread adds its chunks' sums in round order, ``ceil(V / 2048)`` adds (a chunk is 8
  elements, a round is 256 chunks), each chunk sum is a 3-level tree, the 64 lanes combine in 6
  butterfly levels and the 4 waves in 3 adds: ``ceil(V / 2048) + 12``;
* the scan of the draw: 8 chunk-local adds, 6 levels of the lane scan, up to 3 wave totals, the carry
  of ``ceil(V / 2048) - 1`` earlier tiles (each a 6 + 3 level total of its own, not on the chain of
  the carry's adds), and 2 adds that join carry, wave offset and lane prefix: ``ceil(V / 2048) + 18``.

``D(V) = ceil(V / 2048) + 20`` covers both.  Each add rounds by at most 2^-24 of its result (at most Z),
the sum and the scan each contribute one chain, hence the ``2^-23 * D(V) * Z`` term of ``E``; the other
term, ``2^-23 * sum w_i (|z_i| + 8)``, covers the two roundings of ``z_i`` and the fp32 ``exp``.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Plain-integer Philox4x32-10: counter (4 words), key (2 words) -> 4 words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, stream, offset):
    seed, stream, offset = (int(v) & 0xFFFFFFFFFFFFFFFF for v in (seed, stream, offset))
    out = philox4x32_10((offset & MASK, offset >> 32, stream & MASK, stream >> 32), (seed & MASK, seed >> 32))
    return (out[0] >> 8) * 2.0 ** -24


def D(V):
    return -(-V // 2048) + 20


class Row:
    """What the definition says about one row: ``degenerate``, ``greedy`` (with ``token`` and
    ``logprob``), or the kept set, ``z``, ``w``, the prefix sums ``C`` over the kept indices, ``Z``, the
    error bound ``E`` and ``margin``: the least distance of ``p * Z_k`` from a mass it is compared with
    (inf with top-p off)."""

    def __init__(self, x32, T=1.0, k=0, p=1.0):
        x = np.asarray(x32, dtype=np.float32).astype(np.float64)
        V = x.shape[0]
        T, p, k = float(np.float32(T)), float(np.float32(p)), int(k)
        self.V = V
        self.degenerate = bool(np.isnan(x).any() or (x == np.inf).any() or (x == -np.inf).all())
        self.greedy = not self.degenerate and not T > 0
        self.margin = np.inf
        if self.degenerate:
            return
        m = x.max()
        if self.greedy:
            self.token = int(np.flatnonzero(x == m)[0])
            w = np.exp(x - m)                                      # temperature 1, unfiltered
            self.Z = float(w.sum())
            self.logprob = -np.log(self.Z)
            self.E = 2.0 ** -23 * (float((w * (np.abs(np.where(w > 0, x - m, 0.0)) + 8.0)).sum()) + D(V) * self.Z)
            return
        self.z = z = (x - m) / T
        self.w = w = np.exp(z)
        order = np.argsort(x, kind="stable")
        xs = x[order]
        right = np.searchsorted(xs, x, side="right")               # elements <= x_i
        kept = np.ones(V, dtype=bool)
        if 0 < k < V:
            kept = (V - right) < k
        if 0 < p < 1:
            mass = np.concatenate([[0.0], np.cumsum(np.where(kept, w, 0.0)[order])])
            Zk = mass[-1]
            above = Zk - mass[right]                               # kept weight strictly above x_i
            self.margin = float(np.abs(above[kept] - p * Zk).min())
            kept = kept & (above < p * Zk)
        self.kept = kept
        self.C = np.cumsum(np.where(kept, w, 0.0))
        self.Z = float(self.C[-1])
        self.E = 2.0 ** -23 * (float((w * (np.abs(np.where(w > 0, z, 0.0)) + 8.0))[kept].sum()) + D(V) * self.Z)

    def accepts(self, token, u):
        """The acceptance rule of the draw: ``token`` is kept and ``u * Z`` lies within E of its CDF step."""
        t = int(token)
        if not (0 <= t < self.V) or not self.kept[t]:
            return False
        return self.C[t] - self.w[t] - self.E <= u * self.Z <= self.C[t] + self.E

    def logprob_of(self, token):
        return self.z[int(token)] - np.log(self.Z)


def midpoint_p(x32, T=1.0, k=0, classes=3):
    """A top-p (fp32) that keeps exactly the ``classes`` largest distinct values of the row among what
    top-k keeps: the midpoint of the two cumulative masses around that boundary, over Z_k."""
    row = Row(x32, T, k, 1.0)
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    vals = np.unique(x[row.kept])[::-1]
    assert len(vals) > classes, "the row keeps too few distinct values for this boundary"
    mass = np.array([row.w[row.kept & (x == v)].sum() for v in vals[:classes + 1]])
    lo, hi = mass[:classes - 1].sum() if classes > 1 else 0.0, mass[:classes].sum()
    return float(np.float32((lo + hi) / 2.0 / row.Z))


def check_row(x32, T, k, p, seed, stream, offset, token, logprob=None):
    """Assert the kernel's (or the reference's) result for one row against the oracle."""
    row = Row(x32, T, k, p)
    token = int(token)
    if row.degenerate:
        assert token == -1, f"degenerate row: token {token}"
        assert logprob is None or np.isnan(logprob)
        return row
    assert 0 <= token < row.V, f"token {token} outside [0, {row.V})"
    if row.greedy:
        assert token == row.token, f"greedy: {token} != {row.token}"
        if logprob is not None:
            assert abs(float(logprob) - row.logprob) <= row.E / row.Z + 2.0 ** -20
        return row
    assert row.margin >= 16 * row.E, f"test input: top-p margin {row.margin} < 16 E = {16 * row.E}"
    u = uniform(seed, stream, offset)
    assert row.accepts(token, u), (f"token {token} (kept: {bool(row.kept[token])}) is not the draw of u = {u}: "
                                   f"u Z = {u * row.Z}, C- = {row.C[token] - row.w[token]}, C = {row.C[token]}, E = {row.E}")
    if logprob is not None:
        err = abs(float(logprob) - row.logprob_of(token))
        assert err <= row.E / row.Z + 2.0 ** -20, f"logprob off by {err} (bound {row.E / row.Z + 2.0 ** -20})"
    return row
