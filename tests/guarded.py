"""Arenas with guard zones: every array of a C-ABI call lives alone inside a buffer the test owns,

    [front guard][shift][payload][back guard]

so the test can say WHERE a call read and wrote, not only what it computed.  `shift` is 0 or 1 element: the payload
pointer is 16-byte aligned or exactly one element off.  Each guard is at least max(N, 16384) + 64 elements (a row,
or the largest tile a step writes in one go, past either end stays inside the arena), rounded up to whole 16-byte
vectors.  Guards, the shift slot, the pad elements of padded rows and the payload of outputs hold one NaN bit
pattern no arithmetic produces; arenas are compared as integers, so the comparison sees bits, not values.

`GuardedSide` is a `Side` of tests/host_calls.py (inp / inout / out / rows / table / results): device memory,
VW_FLAG_SYNC.  `check(side)` after the call asserts that every guard, shift, pad and input word still holds its bits
and that no output element still holds the sentinel.  tests/test_guarded_cpu.py runs the same check on numpy-backed
arenas with words flipped on purpose."""
import ctypes
from ctypes import POINTER, c_double, c_void_p

import numpy as np

from oracle import oracle as O
from vectorwave_amd import _native as nat

SENTINEL64 = 0x7FF8C0DEC0DEC0DE
SENTINEL32 = 0x7FC0C0DE
MIN_GUARD = 16384


def word_type(dtype):
    """The unsigned integer arenas of `dtype` are compared as: 8-byte words where the element is made of them."""
    return np.dtype(np.uint64 if np.dtype(dtype).itemsize % 8 == 0 else np.uint32)


def sentinel(dtype):
    w = word_type(dtype)
    return w.type(SENTINEL64 if w.itemsize == 8 else SENTINEL32)


def guard_elems(n, itemsize):
    """Guard length in elements for rows of n: >= max(n, 16384) + 64, a whole number of 16-byte vectors."""
    g = max(int(n), MIN_GUARD) + 64
    per = max(1, 16 // itemsize) if 16 % itemsize == 0 else 2
    return (g + per - 1) // per * per


def row_matrix(flat, B, N, ld):
    """The [B, N] data of a padded row buffer of exactly (B - 1) * ld + N elements."""
    return np.stack([flat[b * ld:b * ld + N] for b in range(B)])


def holds_sentinel(a) -> bool:
    a = np.ascontiguousarray(a)
    return bool((a.view(word_type(a.dtype)) == sentinel(a.dtype)).any())


class Arena:
    """One array.  kind: "in" (const: every word must survive), "out" (payload pre-filled with the sentinel, every
    element must be overwritten) or "inout" (values in, any values out).  `pad`: a boolean mask over the payload's
    elements that are row padding (held at the sentinel; they must survive whatever the kind).  Backing store:
    a torch device tensor when `torch` is given, else numpy (host tables, and the CPU self-test)."""

    def __init__(self, name, kind, values, shift, n_guard, torch=None, pad=None):
        values = np.ascontiguousarray(values).reshape(-1)
        self.name, self.kind, self.shift, self.torch, self.table = name, kind, int(shift), torch, False
        self.dtype, self.count = values.dtype, values.size
        self.word = word_type(self.dtype)
        self.wpe = self.dtype.itemsize // self.word.itemsize  # words per element
        self.guard = guard_elems(n_guard, self.dtype.itemsize)
        self.begin = self.guard + self.shift                   # payload start, in elements
        total = self.begin + self.count + self.guard
        s = sentinel(self.dtype)
        words = np.full(total * self.wpe, s, self.word)
        lo, hi = self.begin * self.wpe, (self.begin + self.count) * self.wpe
        if kind != "out":
            words[lo:hi] = values.view(self.word)
        self.const = np.ones(total * self.wpe, bool)           # words the call must not change
        if kind != "in":
            self.const[lo:hi] = False
        if pad is not None:
            pw = np.repeat(np.ascontiguousarray(pad).reshape(-1), self.wpe)
            words[lo:hi][pw] = s
            self.const[lo:hi] |= pw
        self.orig = words
        if torch is not None:
            signed = np.int64 if self.word.itemsize == 8 else np.int32
            self.store = torch.from_numpy(words.view(signed).copy()).cuda()
            base = self.store.data_ptr()
        else:
            self.store = words.copy()
            base = self.store.ctypes.data
        assert base % 16 == 0 and (self.guard * self.dtype.itemsize) % 16 == 0
        self.ptr = base + self.begin * self.dtype.itemsize
        assert self.ptr % 16 == (self.shift * self.dtype.itemsize) % 16

    def words(self):
        """The arena's current words (numpy; a device arena is copied back)."""
        if self.torch is not None:
            return self.store.cpu().numpy().view(self.word)
        return self.store

    def payload(self):
        w = self.words()
        return w[self.begin * self.wpe:(self.begin + self.count) * self.wpe].copy().view(self.dtype)

    def problems(self):
        """Findings as text ([] when the call kept to its footprint)."""
        now, found = self.words(), []
        lo, hi = self.begin * self.wpe, (self.begin + self.count) * self.wpe
        bad = np.flatnonzero((now != self.orig) & self.const)
        regions = (("front", bad[bad < lo]), ("inside", bad[(bad >= lo) & (bad < hi)]), ("back", bad[bad >= hi]))
        for side, idx in regions:
            if idx.size:
                off = (idx - lo) // self.wpe  # element offsets relative to the payload: front < 0, back >= count
                what = {"front": "front guard / shift slot", "back": "back guard",
                        "inside": "row padding" if self.kind != "in" else "const input"}[side]
                found.append(f"{self.name}: {what} changed, {side}: {idx.size} words, offsets {int(off[0])} .. "
                             f"{int(off[-1])} relative to the payload of {self.count} elements")
        if self.kind == "out":
            left = np.flatnonzero((now[lo:hi] == sentinel(self.dtype)) & ~self.const[lo:hi])
            if left.size:
                off = left // self.wpe
                found.append(f"{self.name}: output not written, inside: {left.size} words, offsets {int(off[0])} .. "
                             f"{int(off[-1])} of {self.count} elements")
        return found


class GuardedSide:
    """tests/host_calls.py's Side on guarded device arenas.  `shifts`: which arenas, by order of creation, have
    their payload one element off a 16-byte boundary: "none", "all" or a set of indices.  `n_guard`: the row length
    N of the call (guards are sized from it).  Host tables (filter taps, CWT tables) go through `table`: a numpy
    arena with the same guards, never shifted (the C side reads them on the host)."""

    def __init__(self, torch, n_guard, shifts="none"):
        self.torch, self.n_guard, self.shifts = torch, int(n_guard), shifts
        self.flags = nat.FLAG_SYNC if torch is not None else 0
        self.arenas, self.outs, self.handles, self.matrices = [], [], [], []

    def _shift(self, k):
        return 1 if self.shifts == "all" or (self.shifts != "none" and k in self.shifts) else 0

    def _new(self, name, kind, values, pad=None):
        k = sum(1 for a in self.arenas if not a.table)
        a = Arena(name or f"arg{k}", kind, values, self._shift(k), self.n_guard, self.torch, pad)
        self.arenas.append(a)
        return a

    def inp(self, a, name=None):
        return c_void_p(self._new(name, "in", a).ptr)

    def inout(self, a, name=None):
        ar = self._new(name, "inout", a)
        self.outs.append((ar, np.shape(a)))
        return c_void_p(ar.ptr)

    def out(self, shape, dtype=np.float64, name=None):
        ar = self._new(name, "out", np.zeros(int(np.prod(shape)), dtype))
        self.outs.append((ar, tuple(shape)))
        return c_void_p(ar.ptr)

    def rows(self, B, N, ld, dtype=np.float64, add=0.0, name=None):
        """Row input [B, N] at leading dimension ld >= N: exactly (B - 1) * ld + N elements, the values of the
        plain Side's `rows`, the ld - N pad elements of every row but the last at the sentinel.  The [B, N] matrix
        of the data alone is appended to `matrices` (what a reference may see)."""
        n = (B - 1) * ld + N
        flat = (O.fill_uniform(n, 42) + add).astype(dtype)
        pad = (np.arange(n) % ld) >= N
        self.matrices.append(row_matrix(flat, B, N, ld))
        return c_void_p(self._new(name, "in", flat, pad).ptr)

    def table(self, values, name=None):
        v = np.ascontiguousarray(values, np.float64)
        a = Arena(name or "table", "in", v, 0, self.n_guard, None)
        a.table = True
        self.arenas.append(a)
        return ctypes.cast(c_void_p(a.ptr), POINTER(c_double))

    def structs(self, ctypes_array, name=None):
        """A host array of C structs made of 8-byte words (vw_cwt_scale), guarded: -> its address."""
        raw = np.frombuffer(bytes(ctypes_array), np.uint64)
        a = Arena(name or "structs", "in", raw, 0, self.n_guard, None)
        a.table = True
        self.arenas.append(a)
        return a.ptr

    def n_args(self):
        return sum(1 for a in self.arenas if not a.table)

    def close(self, lib):
        for h in self.handles:
            assert lib.vw_stream_destroy(h) == 0

    def results(self):
        if self.torch is not None:
            self.torch.cuda.synchronize()
        return [ar.payload().reshape(shape) for ar, shape in self.outs]


def check(side):
    """After the call and a synchronize: (a) every guard, shift, pad and input word holds its original bits, (b) no
    output payload element still holds the sentinel.  The message names the argument, the side, the first and last
    touched offsets relative to the payload and the count."""
    if side.torch is not None:
        side.torch.cuda.synchronize()
    found = [p for a in side.arenas for p in a.problems()]
    assert not found, "footprint: " + "; ".join(found)
