"""The batch ladder of tests/single_pass_ladder.py against the planner and the kernel source, on the CPU (tests/emu, the LDS budget
of gfx950): the ladder must reach every tile the planner gives the single-pass kernel -- each C = 4 ... Cmax with a partly filled
tile and a full one, Cmax also with several tiles -- and for fp32 n = 128 ... 4096 that Cmax is the shape baked into the
ROWS_FIX / ROWS_FIX8 instantiations.  If a planner change picks a tile the ladder misses, this fails, and the GPU test
(tests/test_gpu_single_pass.py) that imports the ladder has to follow.  Every emulated transform passes accuracy.check_rows;
n = 1 returns its input bit for bit.  The GPU test runs many(n) too; the emulation stops at 2 Cmax + 1."""
import numpy as np
import pytest

import accuracy as A
import emu_lib as E
import single_pass_ladder as L

ALGO = {"auto": 0, "radix2": 1, "radix4": 2, "split_radix": 3}


def _emulate(algo, log2n, dtype, batch, direction):
    n = 1 << log2n
    x = A.block_normal_rows(n, 0, batch, dtype, seed=500 + log2n)
    y, info = E.emu_fft(x, direction, ALGO[algo], L.LDS_BUDGET)
    label = "emulated %s %s n=%d batch=%d" % (algo, np.dtype(dtype).name, n, batch)
    if log2n == 0:
        assert info[0] == 0 and np.array_equal(y.view(np.uint8), x.view(np.uint8)), label
        return None
    assert info[0] == 1 and info[1] == log2n, (label, info)  # one pass over rows of the whole transform
    A.check_rows(y, x, direction, "multipass", label=label)
    return 1 << info[2]


def _ladder_tiles(algo, log2n, dtype, batches):
    """{C: the kinds of tile the batches gave the kernel of tile C: 'partial' (a partly filled tile), 'full', 'multi' (more than
    one tile)}, over batches of at most 2 Cmax + 1; directions alternate."""
    seen = {}
    for i, batch in enumerate(batches):
        c = _emulate(algo, log2n, dtype, batch, -1 if i % 2 == 0 else 1)
        if c is None:
            continue
        assert c == min(L.cmax(log2n, dtype), max(2 if np.dtype(dtype) == np.complex64 else 1, 1 << (batch - 1).bit_length())), \
            ("tile", algo, log2n, dtype, batch, c)
        kinds = seen.setdefault(c, set())
        if batch % c:
            kinds.add("partial")  # a partly filled tile (n_cols = batch)
        if batch >= c:
            kinds.add("full")
        if batch > c:
            kinds.add("multi")
    return seen


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("log2n", L.LOG2N)
def test_ladder_reaches_every_tile_auto(log2n, dtype):
    if log2n == 0:
        for i, batch in enumerate(b for b in L.LADDER[(0, dtype)] if b <= 3):
            _emulate("auto", 0, dtype, batch, -1 if i % 2 == 0 else 1)
        return
    cm = L.cmax(log2n, dtype)
    if dtype == np.complex64 and log2n >= 7:
        assert cm == 1 << (13 - log2n)  # the fixed shapes: ROWS_FIX (n = 128, 256), ROWS_FIX8 (n = 512 ... 4096)
    batches = [b for b in L.LADDER[(log2n, dtype)] if b <= 2 * cm + 1]
    assert L.many(log2n, dtype) in L.LADDER[(log2n, dtype)] and L.many(log2n, dtype) >= 3 * 2048 * cm
    seen = _ladder_tiles("auto", log2n, dtype, batches)
    assert "multi" in seen.get(cm, ()) and "full" in seen[cm] and (cm == 1 or "partial" in seen[cm]), (cm, seen)
    c = 4
    while c <= cm:
        assert {"partial", "full"} <= seen.get(c, set()), (c, seen)
        c *= 2


@pytest.mark.parametrize("dtype", L.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("log2n", L.LOG2N[1:])
@pytest.mark.parametrize("algo", ["radix2", "radix4", "split_radix"])
def test_ladder_explicit_families(algo, log2n, dtype):
    """The explicit families plan the same tiles; their GPU batches (single_pass_ladder.explicit_batches) up to 2 Cmax + 1."""
    cm = L.cmax(log2n, dtype)
    batches = sorted({b for b in L.explicit_batches(log2n, dtype) if b <= 2 * cm + 1} | {2 * cm + 1})
    seen = _ladder_tiles(algo, log2n, dtype, batches)
    assert "multi" in seen.get(cm, ()), (cm, seen)
