"""Negative tests of the guarded arena (tests/_arena.py), in the manner of tests/test_judges_reject.py: a NumPy array
stands in for the device, a fake "kernel" computes out = 2 * x + y on it, and each deliberate defect -- a store one
element past the output, one in front of it, a flipped input word, the last element or one interior tile left
unwritten -- must make check() raise with the buffer, the index and the pattern; the correct fake must pass, at every
placement of the buffers the GPU tests use."""
import numpy as np
import pytest

from _arena import GUARD_BYTES, GUARD_WORD, UNWRITTEN, Arena, ArenaError, HostMemory

N = 2 * 1024 + 3  # two fp32 tiles of 256 lanes x 4 elements and a ragged tail
TILE = 1024


def _setup(dtype, offset):
    rng = np.random.default_rng(7)
    x, y = rng.uniform(1.0, 2.0, N).astype(dtype), rng.uniform(1.0, 2.0, N).astype(dtype)
    a = Arena(HostMemory())
    a.input("x", x, offset)
    a.input("y", y, offset)
    a.output("out", N, dtype, offset)
    a.commit()
    return a, x, y


def _kernel(a, dtype, lo=0, hi=N, skip=None):
    """out[lo:hi] = 2 x + y through the arena's "pointers"; `skip` = (first, last) elements left alone."""
    m = a.mem
    x, y = (m.view(a.ptr(k), dtype, N) for k in ("x", "y"))
    # (the view is taken wider than the buffer on purpose: a stray store needs somewhere to go)
    wide = m.view(a.ptr("out") - 16 * np.dtype(dtype).itemsize, dtype, N + 32)
    for i in range(lo, hi):
        if skip and skip[0] <= i < skip[1]:
            continue
        wide[16 + i] = 2 * x[i] + y[i] if 0 <= i < N else dtype(3.0)
    return wide[16:16 + N]


PLACEMENTS = [(np.float32, 0), (np.float32, 1), (np.float32, 3), (np.float64, 0), (np.float64, 1)]


@pytest.mark.parametrize("dtype,offset", PLACEMENTS)
def test_correct_kernel_passes(dtype, offset):
    a, x, y = _setup(dtype, offset)
    assert a.ptr("out") % 16 == offset * np.dtype(dtype).itemsize and a.ptr("x") >= GUARD_BYTES
    assert a.ptr("y") - (a.ptr("x") + x.nbytes) >= GUARD_BYTES and a.size - (a.ptr("out") + x.nbytes) >= GUARD_BYTES
    _kernel(a, dtype)
    a.check()
    assert np.array_equal(a.result("out"), 2 * x + y)


@pytest.mark.parametrize("dtype,offset", PLACEMENTS)
def test_one_element_past_the_end(dtype, offset):
    a, _, _ = _setup(dtype, offset)
    _kernel(a, dtype, 0, N + 1)
    with pytest.raises(ArenaError, match=rf"guard word changed past the end of output 'out' .*element index {N}, found 0x"):
        a.check()


@pytest.mark.parametrize("dtype,offset", PLACEMENTS)
def test_one_element_before_the_start(dtype, offset):
    a, _, _ = _setup(dtype, offset)
    _kernel(a, dtype, -1, N)
    with pytest.raises(ArenaError, match=r"guard word changed before the start of output 'out' .*element index -1, found 0x"):
        a.check()


@pytest.mark.parametrize("dtype,offset", PLACEMENTS)
def test_flipped_input_word(dtype, offset):
    a, _, _ = _setup(dtype, offset)
    _kernel(a, dtype)
    a.mem.view(a.ptr("y"), np.uint32, N)[77] ^= 1  # (fp64: the low word of element 38)
    idx = 77 if dtype is np.float32 else 38
    with pytest.raises(ArenaError, match=rf"input 'y' was modified: element index {idx} holds 0x"):
        a.check()


@pytest.mark.parametrize("dtype,offset", PLACEMENTS)
def test_last_element_unwritten(dtype, offset):
    a, _, _ = _setup(dtype, offset)
    _kernel(a, dtype, 0, N - 1)
    with pytest.raises(ArenaError, match=rf"output 'out' .*element index {N - 1} was never written .*0x{UNWRITTEN:08x}\); 1 elements"):
        a.check()


@pytest.mark.parametrize("dtype,offset", PLACEMENTS)
def test_interior_tile_unwritten(dtype, offset):
    a, _, _ = _setup(dtype, offset)
    _kernel(a, dtype, skip=(TILE, 2 * TILE))
    with pytest.raises(ArenaError, match=rf"element index {TILE} was never written .*; {TILE} elements unwritten, the last at index {2 * TILE - 1}"):
        a.check()


def test_a_computed_nan_is_not_unwritten():
    """The default NaN of the arithmetic, and a NaN that carries another payload, count as written."""
    a, _, _ = _setup(np.float32, 0)
    out = _kernel(a, np.float32)
    out[5] = np.float32(np.nan)
    out.view(np.uint32)[6] = 0x7FC00001
    a.check()
    a, _, _ = _setup(np.float64, 0)
    out = _kernel(a, np.float64)
    out[5] = np.nan
    a.check()
    assert np.isnan(np.array([UNWRITTEN], np.uint32).view(np.float32)[0])
    assert np.isnan(np.array([UNWRITTEN, UNWRITTEN], np.uint32).view(np.float64)[0])
    assert not np.isnan(np.array([GUARD_WORD], np.uint32).view(np.float32)[0])


def test_inout_word_is_guarded_but_not_judged():
    a = Arena(HostMemory())
    a.input("sp", np.ones(5, np.float32))
    a.inout("flag", np.zeros(1, np.int32))
    a.commit()
    a.mem.view(a.ptr("flag"), np.int32, 1)[0] |= 1
    a.check()
    assert a.result("flag")[0] == 1
    a.mem.view(a.ptr("flag"), np.int32, 2)[1] = 1
    with pytest.raises(ArenaError, match="past the end of in-out buffer 'flag'"):
        a.check()
