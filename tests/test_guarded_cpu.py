"""The guard-zone net of tests/guarded.py catches what it is for: on numpy-backed arenas (no GPU), `check` passes
after a call that kept to its footprint and fails, naming the argument, the side and the offset, for one word
flipped in the front guard, the back guard, the shift slot or a row's padding, and for one output element left
unwritten."""
import numpy as np
import pytest

import guarded as G

B, N, LD = 3, 5, 8


def make(dtype, shifts):
    """One forward-like call's arenas: padded row input, a threshold input, one output; the "kernel" writes the
    output completely."""
    s = G.GuardedSide(None, N, shifts)
    s.rows(B, N, LD, dtype, name="x")
    s.inp(np.full(B, 0.25, dtype), name="thr")
    s.out((B, N), dtype, name="y")
    x, thr, y = s.arenas
    y.store[y.begin * y.wpe:(y.begin + y.count) * y.wpe] = np.arange(B * N, dtype=dtype).view(y.word)
    return s, x, thr, y


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shifts", ["none", "all", {0}, {2}], ids=["none", "all", "x", "y"])
def test_a_call_inside_its_footprint_passes(dtype, shifts):
    s, x, thr, y = make(dtype, shifts)
    G.check(s)
    want = {"none": (0, 0, 0), "all": (1, 1, 1)}.get(shifts if isinstance(shifts, str) else "", None)
    got = (x.shift, thr.shift, y.shift)
    assert got == (want if want else tuple(int(k in shifts) for k in range(3)))
    for a in (x, thr, y):
        assert a.ptr % 16 == a.shift * a.dtype.itemsize and a.guard >= max(N, 16384) + 64
    assert x.count == (B - 1) * LD + N
    out, = s.results()
    assert out.shape == (B, N) and np.array_equal(out.reshape(-1), np.arange(B * N, dtype=dtype))
    # the pads are the sentinel, the data is what the plain side's rows hold
    flat = x.payload()
    assert G.holds_sentinel(flat) and not G.holds_sentinel(s.matrices[0])
    assert np.array_equal(G.row_matrix(flat, B, N, LD), s.matrices[0])


def flip(a, word):
    a.store[word] ^= a.word.type(1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shift", [0, 1])
def test_one_flipped_word_fails_with_its_place(dtype, shift):
    shifts = "all" if shift else "none"
    # front guard of the output, 3 elements before the payload
    s, x, thr, y = make(dtype, shifts)
    flip(y, (y.begin - 3 - shift) * y.wpe)
    with pytest.raises(AssertionError, match=rf"y: front guard / shift slot changed, front: 1 words, offsets -{3 + shift} "):
        G.check(s)
    # back guard of the output: the element right after the payload
    s, x, thr, y = make(dtype, shifts)
    flip(y, (y.begin + y.count) * y.wpe)
    with pytest.raises(AssertionError, match=rf"y: back guard changed, back: 1 words, offsets {B * N} \.\. {B * N} "):
        G.check(s)
    # back guard of an input (a stray write into a const array's slack)
    s, x, thr, y = make(dtype, shifts)
    flip(thr, (thr.begin + thr.count + 7) * thr.wpe)
    with pytest.raises(AssertionError, match=rf"thr: back guard changed, back: 1 words, offsets {B + 7} "):
        G.check(s)
    # a pad element of row 1 of the input
    s, x, thr, y = make(dtype, shifts)
    flip(x, (x.begin + LD + N + 1) * x.wpe)
    with pytest.raises(AssertionError, match=rf"x: const input changed, inside: 1 words, offsets {LD + N + 1} "):
        G.check(s)
    # a data element of the input: inputs are const
    s, x, thr, y = make(dtype, shifts)
    flip(x, (x.begin + 2) * x.wpe)
    with pytest.raises(AssertionError, match=r"x: const input changed, inside: 1 words, offsets 2 \.\. 2 "):
        G.check(s)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_shift_slot_is_guarded(dtype):
    s, x, thr, y = make(dtype, "all")
    flip(y, (y.begin - 1) * y.wpe)  # the one element between the 16-byte boundary and the payload
    with pytest.raises(AssertionError, match=r"y: front guard / shift slot changed, front: 1 words, offsets -1 \.\. -1 "):
        G.check(s)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_unwritten_output_element_fails(dtype):
    s, x, thr, y = make(dtype, "none")
    y.store[(y.begin + 11) * y.wpe] = G.sentinel(dtype)
    with pytest.raises(AssertionError, match=r"y: output not written, inside: 1 words, offsets 11 \.\. 11 of 15"):
        G.check(s)


def test_in_place_arrays_guard_their_surroundings_only():
    s = G.GuardedSide(None, N, {0})
    s.inout(np.arange(6.0), name="c")
    c, = s.arenas
    c.store[c.begin:c.begin + 6] = np.arange(6.0)[::-1].copy().view(np.uint64)  # the call rewrites the payload
    G.check(s)
    assert np.array_equal(s.results()[0], np.arange(6.0)[::-1])
    flip(c, c.begin + 6)
    with pytest.raises(AssertionError, match=r"c: back guard changed"):
        G.check(s)


def test_the_sentinels_are_quiet_nans_with_the_stated_payload():
    assert int(G.sentinel(np.float64)) == 0x7FF8C0DEC0DEC0DE and int(G.sentinel(np.float32)) == 0x7FC0C0DE
    assert np.isnan(np.array([G.sentinel(np.float64)]).view(np.float64)[0])
    assert np.isnan(np.array([G.sentinel(np.float32)]).view(np.float32)[0])
    # arithmetic NaNs carry another payload
    with np.errstate(all="ignore"):
        made = np.array([np.inf - np.inf, 0.0 * np.inf, np.nan, np.sqrt(-1.0)])
    assert not G.holds_sentinel(made) and not G.holds_sentinel(made.astype(np.float32))


def test_host_tables_are_guarded_and_never_shifted():
    s = G.GuardedSide(None, N, "all")
    p = s.table([1.0, 2.0, 3.0], name="lo")
    t, = s.arenas
    assert t.shift == 0 and [p[i] for i in range(3)] == [1.0, 2.0, 3.0] and np.isnan(p[3]) and np.isnan(p[-1])
    G.check(s)
    assert s.n_args() == 0
