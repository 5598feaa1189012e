"""csrc/layout_checks.h -- the host predicates that decide, per launch, whether a dta_tensor's
strides may be served by the LDS-DMA descriptors (else the tiles are staged by address) --
compiled into a stand-alone program and compared with the conditions in exact integer
arithmetic: each side of (n - 1) si + width <= st, each side of T st es < 2^31, and strides
large enough to overflow a 64-bit product (the program is built with the undefined-behaviour
sanitizer where the toolchain has it).  CPU only."""
import itertools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differential_transformer_replication_amd", "csrc")


def _rows_ok(T, st, si, n, width, es):
    return T <= 0 or (st > 0 and si >= 0 and (n - 1) * si + width <= st and T * st * es < 2 ** 31)


def _rowvecs_ok(n, B, H, T):
    return min(n, B, H, T) <= 0 or n * B * H * T * 4 < 2 ** 31


def _rows_table():
    rows = []
    for n, width, es in ((2, 64, 2), (3, 64, 2), (1, 64, 2), (4, 32, 2), (2, 128, 2), (2, 64, 4)):
        eq = (n - 1) * width + width                    # st at equality with si = width
        v = 16 // es
        for T in (70, 200):
            rows += [(T, eq, width, n, width, es), (T, eq, width + v, n, width, es), (T, eq + v, width + v, n, width, es),
                     (T, eq - v, width, n, width, es), (T, eq + 8, width, n, width, es),
                     (T, 2 * eq, T * 2 * eq, n, width, es),                 # branch-outer
                     (T, eq, 0, n, width, es), (T, 0, width, n, width, es), (T, eq, -v, n, width, es),
                     (T, width - v, 0, 1, width, es)]
        # the 32-bit edge: the largest row stride with T st es < 2^31, and one vector more
        for T in (70, 4096, 2 ** 20):
            edge = (2 ** 31 - 1) // (T * es) // v * v
            rows += [(T, edge, width, n, width, es), (T, edge + v, width, n, width, es)]
        rows += [(70, 2 ** 25, 64, n, width, es), (0, 0, 0, n, width, es)]
        # products past 64 bits
        rows += [(2 ** 31 - 1, 2 ** 62, 2 ** 62, n, width, es), (70, 2 ** 62, 2 ** 62, 5, width, es),
                 (70, 2 ** 63 - 8, 2 ** 61, n, width, es), (70, 256, 2 ** 63 - 8, n, width, es)]
    return rows


def _rowvecs_table():
    big = (1, 2, 64, 2 ** 20, 2 ** 29 - 1, 2 ** 29, 2 ** 31 - 1)
    rows = [t for t in itertools.product(big, repeat=4) if t[0] <= 64][::7]
    return rows + [(2, 2, 64, 2 ** 21 - 1), (2, 2, 64, 2 ** 21), (1, 1, 1, 2 ** 29 - 1), (1, 1, 1, 2 ** 29), (0, 1, 1, 1)]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_layout_predicates_match_exact_arithmetic():
    rows, vecs = _rows_table(), _rowvecs_table()
    fmt = lambda t: ", ".join(f"{x}ll" for x in t)
    src = ['#include <stdio.h>', '#include "layout_checks.h"',
           "static const long long R[][6] = {" + ", ".join("{" + fmt(t) + "}" for t in rows) + "};",
           "static const long long V[][4] = {" + ", ".join("{" + fmt(t) + "}" for t in vecs) + "};",
           "int main() {",
           "  for (auto& r : R) printf(\"%d\\n\", (int)dta::dma_rows_ok(r[0], r[1], r[2], (int)r[3], (int)r[4], (int)r[5]));",
           "  for (auto& v : V) printf(\"%d\\n\", (int)dta::dma_rowvecs_ok(v[0], v[1], v[2], v[3]));",
           "  return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        cpp, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "probe")
        with open(cpp, "w") as fh:
            fh.write("\n".join(src))
        base = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, cpp, "-o", exe]
        ubsan = ["-fsanitize=undefined", "-fno-sanitize-recover=all"]
        if subprocess.run(base + ubsan, capture_output=True).returncode != 0:     # a toolchain without libubsan
            subprocess.run(base, check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = [bool(int(x)) for x in out]
    want = [_rows_ok(*t) for t in rows] + [_rowvecs_ok(*t) for t in vecs]
    assert len(got) == len(want)
    bad = [(t, g, w) for t, g, w in zip(rows + vecs, got, want) if g != w]
    assert not bad, bad
    assert 0.2 < sum(want) / len(want) < 0.8               # both outcomes are well represented
