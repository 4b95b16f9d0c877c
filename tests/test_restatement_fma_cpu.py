"""The FMA option of the numpy restatements (``fma=True``), without a GPU.

Three things entitle the FMA restatement to stand as the bit-level reference of the engine's FMA kernels:

1. its primitive -- ``oracle.fma_f64`` / ``oracle.fma_f32``, libm's fma / fmaf -- is correctly rounded: compared
   with exact rational arithmetic (``fractions.Fraction``) on random triples and on triples built so that the exact
   ``x * f + acc`` lies one unit in the product's last place above or below the midpoint of two representable
   results.  For float32 the twice-rounded emulation ``float32(float64(x) * f + acc)`` is shown to get built
   triples wrong: the cases bite, and the emulation is not a substitute;
2. its indexing and step order equal a scalar restatement's that shares none of its code: plain Python loops over
   outputs and taps, its own modulo / mirror / zero index maps, every step rounded from an exact Fraction;
3. the comparison has teeth: at db4, N = 512, J = 3 the FMA restatement differs in bits from the EXACT one in
   at least 40 % of the outputs while staying far inside the tolerance bars the GPU tests keep.  The test prints
   max |FMA - EXACT| per plane (DESIGN.md 2 quotes them): run with ``-s``.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from vectorwave_amd.wavelets import WID_OTHER, Coiflet, Daubechies

import mra_restatement as M
import restatement_bi as RB
import restatement_generic as G

BOUNDARIES = [O.PERIODIC, O.SYMMETRIC, O.ZERO_PADDING]
BIDS = ["P", "S", "Z"]
PREC = {np.float64: (53, -1022), np.float32: (24, -126)}   # significand bits, minimum normal exponent
FMA_OF = {np.float64: O.fma_f64, np.float32: O.fma_f32}
DTYPES = [np.float64, np.float32]
DIDS = ["f64", "f32"]


# ---- exact rational arithmetic ----------------------------------------------------------------------------------
def rnd(q: Fraction, dtype) -> Fraction:
    """q rounded to the nearest value of ``dtype`` (ties to even), as an exact Fraction.  Gradual underflow;
    nothing here comes near overflow."""
    if q == 0:
        return Fraction(0)
    p, emin = PREC[dtype]
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()   # 2**(e-1) <= a < 2**(e+1)
    if a < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, emin) - p + 1)
    m, rem = divmod(a, ulp)
    if rem > ulp / 2 or (rem == ulp / 2 and m % 2 == 1):
        m += 1
    r = m * ulp
    return -r if q < 0 else r


def as_float(q: Fraction, dtype):
    v = dtype(float(q))          # q is a value of dtype: both conversions are exact
    assert Fraction(float(v)) == q
    return v


def test_rnd_is_pythons_own_rounding_at_binary64():
    """Fraction -> float is correctly rounded in CPython (integer true division): the helper agrees with it."""
    rng = np.random.default_rng(1)
    for _ in range(500):
        q = Fraction(int(rng.integers(-2**62, 2**62)), int(rng.integers(1, 2**62))) * Fraction(2) ** int(rng.integers(-40, 40))
        assert float(rnd(q, np.float64)) == float(q)
    assert rnd(Fraction(1) + Fraction(1, 2**24), np.float32) == 1                          # tie to even, down
    assert rnd(Fraction(1) + Fraction(3, 2**24), np.float32) == 1 + Fraction(4, 2**24)     # tie to even, up
    assert rnd(Fraction(3, 2**150), np.float32) == Fraction(4, 2**150)                     # subnormal tie


# ---- 1. the primitive ------------------------------------------------------------------------------------------
def _check_triples(dtype, xs, fs, accs):
    """fma per distinct f (the entry point takes one tap) against rnd(x * f + acc); returns the results."""
    out = np.empty(len(xs), dtype=dtype)
    for i in range(len(xs)):
        out[i] = FMA_OF[dtype](xs[i:i + 1], fs[i], accs[i:i + 1])[0]
        want = rnd(Fraction(float(xs[i])) * Fraction(float(fs[i])) + Fraction(float(accs[i])), dtype)
        assert Fraction(float(out[i])) == want, (i, float(xs[i]), float(fs[i]), float(accs[i]), float(out[i]))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_fma_random_triples_against_fractions(dtype):
    rng = np.random.default_rng(11)
    n = 3000
    scale = 2.0 ** rng.integers(-12, 4, n)           # accumulators from well below to well above the product
    xs = rng.uniform(-1, 1, n).astype(dtype)
    fs = rng.uniform(-1, 1, n).astype(dtype)
    accs = (rng.uniform(-1, 1, n) * scale).astype(dtype)
    got = _check_triples(dtype, xs, fs, accs)
    if dtype is np.float32:   # the record of why random triples are not enough: the twice-rounded form rarely differs
        twice = (xs.astype(np.float64) * fs.astype(np.float64) + accs.astype(np.float64)).astype(np.float32)
        print(f"random float32 triples where float32(float64(x)*f+acc) differs from fmaf: "
              f"{int(np.count_nonzero(twice != got))} of {n}")
    # one vectorised call is the element-wise call
    f0 = fs[0]
    exact_rows = FMA_OF[dtype](xs.reshape(30, 100), f0, accs.reshape(30, 100))
    assert exact_rows.shape == (30, 100) and exact_rows.dtype == dtype
    for i in (0, 1, 1234, n - 1):
        want = rnd(Fraction(float(xs[i])) * Fraction(float(f0)) + Fraction(float(accs[i])), dtype)
        assert Fraction(float(exact_rows.reshape(-1)[i])) == want


def built_triples(dtype, count, seed):
    """(x, f, acc, side) with x * f + acc = (R + 1/2) ulp +- one unit in the product's last place, R a full
    significand.  X, F, A integers of at most p bits, everything in units u = 2**-2p of the product's last place:
    X odd, F = X^-1 * (2**(p-1) +- 1) mod 2**p, so X * F = q * 2**p + 2**(p-1) +- 1, and A = R - q (|A| < 2**p)
    gives A * 2**p + X * F = R * 2**p + 2**(p-1) +- 1."""
    p = PREC[dtype][0]
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        X = int(rng.integers(2**(p - 1), 2**p)) | 1
        side = 1 if len(out) % 2 else -1
        F = (pow(X, -1, 2**p) * (2**(p - 1) + side)) % 2**p
        q = (X * F) >> p
        R = int(rng.integers(2**(p - 1), 2**p - 1))
        A = R - q
        sign = -1 if (len(out) // 2) % 2 else 1
        x, f, acc = math.ldexp(sign * X, -p), math.ldexp(F, -p), math.ldexp(sign * A, -p)
        assert Fraction(x) * Fraction(f) + Fraction(acc) == sign * Fraction(R * 2**p + 2**(p - 1) + side, 2**(2 * p))
        out.append((dtype(x), dtype(f), dtype(acc), side, sign * Fraction(R + (1 if side > 0 else 0), 2**p)))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_fma_next_to_a_midpoint(dtype):
    tr = built_triples(dtype, 400, 5)
    xs, fs, accs = (np.array([t[k] for t in tr], dtype=dtype) for k in range(3))
    got = _check_triples(dtype, xs, fs, accs)
    for g, t in zip(got, tr):    # ... and the result the construction predicts: just above rounds up, just below down
        assert Fraction(float(g)) == t[4]


def test_the_twice_rounded_emulation_of_fmaf_is_wrong():
    """10610063 * 13264529 = 2**47 - 1 (2351 * 4513 * 13264529), both factors below 2**24: with acc = A * 2**48 the
    exact sum is A * 2**48 +- (2**47 - 1), a float32 midpoint -+ one unit, 72 bits wide.  binary64 rounds it ONTO
    the midpoint and the second rounding breaks the tie to even: wrong for every odd A on one side, every even A
    on the other."""
    X, F = 10610063, 13264529
    assert X * F == 2**47 - 1 and X < 2**24 and F < 2**24
    rng = np.random.default_rng(3)
    n = 200
    A = rng.integers(2**23 + 1, 2**24 - 1, n)
    sgn = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    xs = (sgn * math.ldexp(X, -24)).astype(np.float32)     # product +-(1/2 - 2**-48)
    fs = np.full(n, math.ldexp(F, -24), dtype=np.float32)
    accs = A.astype(np.float32)
    assert np.array_equal(accs.astype(np.int64), A)
    got = _check_triples(np.float32, xs, fs, accs)
    # below the midpoint A + 1/2: A; above the midpoint A - 1/2: A
    assert np.array_equal(got, accs)
    twice = (xs.astype(np.float64) * fs.astype(np.float64) + accs.astype(np.float64)).astype(np.float32)
    wrong = int(np.count_nonzero(twice != got))
    print(f"built float32 triples the twice-rounded binary64 emulation gets wrong: {wrong} of {n}")
    assert wrong >= 1
    assert wrong == int(np.count_nonzero(A % 2 == 1))   # exactly the odd accumulators


def test_fma_f32_refuses_a_binary64_tap():
    with pytest.raises(ValueError):
        O.fma_f32(np.zeros(2, np.float32), 0.1, np.zeros(2, np.float32))


# ---- 2. a scalar restatement that shares no indexing ----------------------------------------------------------
class Scalar:
    """Plain loops over outputs and taps on exact Fractions; every arithmetic step is one ``rnd``."""

    def __init__(self, dtype, fma):
        self.dtype, self.fma = dtype, fma

    def r(self, q):
        return rnd(q, self.dtype)

    def step(self, acc, x, f):
        return self.r(x * f + acc) if self.fma else self.r(acc + self.r(x * f))

    def pair(self, acc, lo, a, hi, d):
        if self.fma:
            return self.r(acc + self.r(lo * a + self.r(hi * d)))
        return self.r(acc + self.r(self.r(lo * a) + self.r(hi * d)))

    def taps(self, h):
        return [Fraction(float(self.dtype(float(v) * (1.0 / math.sqrt(2.0))))) for v in h]

    @staticmethod
    def mirror(i, n):
        """half-sample symmetric extension, written as a walk: ... 1 0 | 0 1 .. n-1 | n-1 n-2 ..."""
        while i < 0 or i >= n:
            i = -i - 1 if i < 0 else 2 * n - 1 - i
        return i

    def forward(self, x, lo, hi, boundary, J):
        n = len(x)
        flo, fhi = self.taps(lo), self.taps(hi)
        cur = [Fraction(float(v)) for v in x]
        det = []
        for j in range(1, J + 1):
            s = 2 ** (j - 1)
            a, d = [], []
            for t in range(n):
                sa, sd = Fraction(0), Fraction(0)
                for l in range(len(lo)):
                    i = t - l * s
                    if boundary == O.PERIODIC:
                        while i < 0:
                            i += n
                    elif boundary == O.ZERO_PADDING:
                        if i < 0:
                            continue
                    else:
                        i = self.mirror(i, n)
                    sa = self.step(sa, cur[i], flo[l])
                    sd = self.step(sd, cur[i], fhi[l])
                a.append(sa)
                d.append(sd)
            det.append(d)
            cur = a
        return det, cur

    def inverse(self, det, app, lo, hi, boundary, wid):
        n, J, L = len(app), len(det), len(lo)
        flo, fhi = self.taps(lo), self.taps(hi)
        cur = list(app)
        for j in range(J, 0, -1):
            s = 2 ** (j - 1)
            d = det[j - 1]
            if boundary == O.SYMMETRIC:   # integer bookkeeping of the alignment: the oracle's
                ap, dh, dp, dg = O.sym_decide(wid, L, j)
                tau = O.lib().vwo_compute_tau(L, j)
            out = []
            for t in range(n):
                acc = Fraction(0)
                if boundary == O.ZERO_PADDING:
                    for l in range(L):
                        if t + l * s < n:
                            acc = self.pair(acc, flo[l], cur[t + l * s], fhi[l], d[t + l * s])
                elif boundary == O.PERIODIC:
                    for l in range(L):
                        acc = self.step(acc, cur[(t + l * s) % n], flo[l])
                    for l in range(L):
                        acc = self.step(acc, d[(t + l * s) % n], fhi[l])
                else:
                    for l in range(L):
                        i = t + l * s - (tau + dh) if ap else t - l * s + (tau + dh)
                        acc = self.step(acc, cur[self.mirror(i, n)], flo[l])
                    for l in range(L):
                        i = t + l * s - (tau + dg) if dp else t - l * s + (tau + dg)
                        acc = self.step(acc, d[self.mirror(i, n)], fhi[l])
                out.append(acc)
            cur = out
        return cur

    def arr(self, rows):
        return np.array([[as_float(v, self.dtype) for v in row] for row in rows], dtype=self.dtype)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert a.tobytes() == b.tobytes(), f"{int(np.count_nonzero(a != b))} of {a.size} differ"


SMALL = {"N16-L4-J2": (16, Daubechies.DB2.lowPassDecomposition(), Daubechies.DB2.highPassDecomposition(),
                       Daubechies.DB2.wavelet_id, 2),
         "N19-L9-J1": (19,) + G.synthetic_filter(9) + (WID_OTHER, 1)}


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "exact"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
@pytest.mark.parametrize("case", list(SMALL))
def test_vectorised_equals_scalar(case, boundary, dtype, fma):
    """Forward, and the inverse fed the forward's planes, bit for bit.  The EXACT run checks the scalar form itself
    (the vectorised EXACT restatement equals the C oracle: tests/test_restatement_generic_cpu.py)."""
    n, lo, hi, wid, J = SMALL[case]
    assert len(lo) == int(case.split("-")[1][1:])
    x = O.java_random_signal(n, 23 + n).astype(dtype)
    sc = Scalar(dtype, fma)
    det_s, app_s = sc.forward(x, lo, hi, boundary, J)
    det, app = G.decompose(x, lo, hi, boundary, J, dtype=dtype, fma=fma)
    same_bytes(det, sc.arr(det_s))
    same_bytes(app, sc.arr([app_s])[0])
    y_s = sc.inverse(det_s, app_s, lo, hi, boundary, wid)
    y = G.reconstruct(det, app, lo, hi, boundary, wid, dtype=dtype, fma=fma)
    same_bytes(y, sc.arr([y_s])[0])
    assert float(np.max(np.abs(y.astype(np.float64)))) > 0.01   # not a degenerate comparison
    # the two-length restatement on a bank of equal lengths is the same arithmetic
    det_b, app_b = RB.decompose(x, lo, hi, boundary, J, dtype=dtype, fma=fma)
    same_bytes(det_b, det)
    same_bytes(app_b, app)
    same_bytes(RB.reconstruct(det, app, lo, hi, boundary, wid, dtype=dtype, fma=fma), y)


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_single_level_pairwise_equals_scalar(boundary, dtype):
    """restatement_bi.forward1 / inverse1 (pairwise in all three boundaries, SYMMETRIC t - l and the batch t + l) in
    FMA mode against scalar loops."""
    n, lo, hi, _, _ = SMALL["N19-L9-J1"]
    x = O.java_random_signal(n, 61).astype(dtype)
    sc = Scalar(dtype, True)
    (d_s,), a_s = sc.forward(x, lo, hi, boundary, 1)
    a, d = RB.forward1(x, lo, hi, boundary, dtype=dtype, fma=True)
    same_bytes(a, sc.arr([a_s])[0])
    same_bytes(d, sc.arr([d_s])[0])
    flo, fhi = sc.taps(lo), sc.taps(hi)
    for batch_sym in (False, True):
        want = []
        for t in range(n):
            acc = Fraction(0)
            for l in range(len(lo)):
                if boundary == O.PERIODIC:
                    i = (t + l) % n
                elif boundary == O.ZERO_PADDING:
                    i = t + l
                    if i >= n:
                        continue
                else:
                    i = sc.mirror(t + l if batch_sym else t - l, n)
                acc = sc.pair(acc, flo[l], a_s[i], fhi[l], d_s[i])
            want.append(acc)
        same_bytes(RB.inverse1(a, d, lo, hi, boundary, batch_sym=batch_sym, dtype=dtype, fma=True), sc.arr([want])[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=BIDS)
def test_mra_components_in_fma(boundary, dtype):
    """mra_restatement in FMA mode: each branch pass is the scalar chain; and for PERIODIC / SYMMETRIC the skipped
    zero-plane steps could not change a bit under FMA either (fma(+-0, f, acc) = acc), so the J+1 masked FMA
    reconstructions give the same bytes.  ZERO_PADDING's pairwise term does not fuse the same way
    (acc + fma(lo, a, 0) rounds the product): there the branch-pass form is the kernel's, not the masked one."""
    n, lo, hi, wid, J = SMALL["N16-L4-J2"]
    rng = np.random.default_rng(9)
    det = rng.uniform(-1, 1, (J, n)).astype(dtype)
    app = rng.uniform(-1, 1, n).astype(dtype)
    got = M.mra(det, app, lo, hi, boundary, wid, dtype=dtype, fma=True)
    sc = Scalar(dtype, True)
    if boundary != O.ZERO_PADDING:
        fr = lambda a: [Fraction(float(v)) for v in a]
        zero = [Fraction(0)] * n
        for c in range(J + 1):
            planes = [fr(det[j]) if c == j + 1 else zero for j in range(J)]
            want = sc.inverse(planes, fr(app) if c == 0 else zero, lo, hi, boundary, wid)
            same_bytes(got[c], sc.arr([want])[0])
        masked = np.stack([G.reconstruct(det, app, lo, hi, boundary, wid, (1 << (c - 1)) if c else 0, c != 0, dtype,
                                         fma=True) for c in range(J + 1)])
        same_bytes(got, masked)
    else:
        flo, fhi = sc.taps(lo), sc.taps(hi)

        def zpass(src, f, s):
            out = []
            for t in range(n):
                acc = Fraction(0)
                for l in range(len(f)):
                    if t + l * s < n:
                        acc = sc.step(acc, src[t + l * s], f[l])
                out.append(acc)
            return out
        for c in range(J + 1):
            if c == 0:
                cur, top = [Fraction(float(v)) for v in app], J
            else:
                cur, top = zpass([Fraction(float(v)) for v in det[c - 1]], fhi, 2 ** (c - 1)), c - 1
            for j in range(top, 0, -1):
                cur = zpass(cur, flo, 2 ** (j - 1))
            same_bytes(got[c], sc.arr([cur])[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_zero_padding_in_fma_mode_is_the_zero_extended_row(dtype):
    """ZERO_PADDING under FMA visits every tap with +0 outside the row (the kernels' zero halo): one level of it is
    the PERIODIC level of the row extended by (L-1) zeros, signs of zeros included.  The row ends in values so small
    that a lone product underflows completely: the fused chain then holds -0, and the +0 samples of the later taps
    decide the sign it leaves -- skipping them, as EXACT may, would keep -0."""
    lo, hi = Daubechies.DB2.lowPassDecomposition(), Daubechies.DB2.highPassDecomposition()
    L, n = len(lo), 24
    tiny = np.finfo(dtype).smallest_subnormal
    x = O.java_random_signal(n, 77).astype(dtype)
    x[:3] = [tiny, -tiny, tiny]          # forward: output t < L-1 sums taps 0..t only
    x[-3:] = [-tiny, tiny, -tiny]        # inverse: output t > n-L sums taps 0..n-1-t only
    xz = np.concatenate([np.zeros(L - 1, dtype), x])
    det, app = G.decompose(x, lo, hi, O.ZERO_PADDING, 1, dtype=dtype, fma=True)
    det_p, app_p = G.decompose(xz, lo, hi, O.PERIODIC, 1, dtype=dtype, fma=True)
    same_bytes(det[0], det_p[0][L - 1:])
    same_bytes(app, app_p[L - 1:])
    zx = np.concatenate([x, np.zeros(L - 1, dtype)])
    comp = M.mra(np.stack([x]), x, lo, hi, O.ZERO_PADDING, dtype=dtype, fma=True)
    comp_p = M.mra(np.stack([zx]), zx, lo, hi, O.PERIODIC, dtype=dtype, fma=True)
    same_bytes(comp, comp_p[:, :n])
    # output 0 of the forward by hand: tap 0 on x[0] (its product underflows to +-0), then taps 1 .. L-1 on +0
    fma1 = lambda a, f, c: FMA_OF[dtype](np.array([a], dtype), f, np.array([c], dtype))[0]   # noqa: E731
    bites = 0
    for taps, out in ((G.scaled_taps(lo, dtype), app[0]), (G.scaled_taps(hi, dtype), det[0][0])):
        assert abs(float(taps[0])) < 0.5                      # |x[0] * f[0]| < tiny / 2: rounds to a zero
        skipped = full = fma1(x[0], taps[0], dtype(0))
        for f in taps[1:]:
            full = fma1(dtype(0), f, full)
        assert skipped == 0 and full == 0 and out == 0 and np.signbit(out) == np.signbit(full)
        bites += int(np.signbit(skipped) != np.signbit(full))
    assert bites > 0, "visiting the +0 samples changed no sign: the case does not bite"
    # EXACT never leaves -0, visited or skipped
    d_e, a_e = G.decompose(x, lo, hi, O.ZERO_PADDING, 1, dtype=dtype)
    assert not np.any((d_e == 0) & np.signbit(d_e)) and not np.any((a_e == 0) & np.signbit(a_e))


# ---- 3. teeth -----------------------------------------------------------------------------------------------------
def _modes(w, n, J, dtype, boundary=O.PERIODIC):
    lo, hi = w.lowPassDecomposition(), w.highPassDecomposition()
    x = O.fill_uniform(n, 42).astype(dtype)
    out = []
    for fma in (False, True):
        d, a = G.decompose(x, lo, hi, boundary, J, dtype=dtype, fma=fma)
        y = G.reconstruct(d, a, lo, hi, boundary, w.wavelet_id, dtype=dtype, fma=fma)
        out.append((d, a, y))
    return x, out


@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_fma_differs_from_exact_in_bits_but_not_in_size(dtype):
    w, n, J = Daubechies.DB4, 512, 3
    x, (ex, fm) = _modes(w, n, J, dtype)
    bar = 1e-12 if dtype is np.float64 else 1e-5 * float(np.max(np.abs(x))) * J
    for name, e, f in zip(("details", "approx", "y"), ex, fm):
        frac = float(np.count_nonzero(e != f)) / e.size
        err = float(np.max(np.abs(e.astype(np.float64) - f.astype(np.float64))))
        print(f"db4 N={n} J={J} {np.dtype(dtype).name} {name}: max|FMA-EXACT| = {err:.2e}, "
              f"{100 * frac:.0f} % of outputs differ in bits (bar {bar:.0e})")
        assert frac >= 0.40, (name, frac)
        assert err <= bar, (name, err, bar)
        assert err <= bar / 50, (name, err)   # the bars are orders of magnitude wider than the effect they bound


@pytest.mark.parametrize("wname,n,J,dtype", [("db4", 4096, 6, np.float64), ("coif5", 8192, 6, np.float32)],
                         ids=["db4-4096-J6-f64", "coif5-8192-J6-f32"])
def test_size_of_the_effect_at_the_benchmark_shapes(wname, n, J, dtype):
    """The figures DESIGN.md 2 quotes (printed), and the hole a tolerance leaves: the smallest low-pass tap of coif5
    zeroed at the deepest level only moves the approximation by a small fraction of the bar and most of its bits."""
    w = {"db4": Daubechies.DB4, "coif5": Coiflet.COIF5}[wname]
    x, (ex, fm) = _modes(w, n, J, dtype)
    bar = 1e-12 if dtype is np.float64 else 1e-5 * float(np.max(np.abs(x))) * J
    for name, e, f in zip(("details", "approx", "y"), ex, fm):
        err = float(np.max(np.abs(e.astype(np.float64) - f.astype(np.float64))))
        frac = float(np.count_nonzero(e != f)) / e.size
        print(f"{wname} N={n} J={J} {np.dtype(dtype).name} {name}: max|FMA-EXACT| = {err:.2e}, "
              f"{100 * frac:.0f} % differ in bits (bar {bar:.0e})")
        assert err <= bar / 50 and frac >= 0.40
    if wname == "coif5":
        lo, hi = list(w.lowPassDecomposition()), w.highPassDecomposition()
        k = int(np.argmin(np.abs(lo)))
        d5, a5 = G.decompose(x, lo, hi, O.PERIODIC, J - 1, dtype=dtype, fma=True)
        cut = list(lo)
        cut[k] = 0.0
        a6_cut, _ = G._forward_level(a5, G.scaled_taps(cut, dtype), G.scaled_taps(hi, dtype), 1 << (J - 1), O.PERIODIC,
                                     fma=True)
        moved = float(np.max(np.abs(a6_cut.astype(np.float64) - fm[1].astype(np.float64))))
        frac = float(np.count_nonzero(a6_cut != fm[1])) / a6_cut.size
        print(f"coif5 tap {k} ({lo[k]:.1e}) zeroed at level {J}: approx moves {moved:.1e} = bar/{bar / moved:.0f}, "
              f"{100 * frac:.0f} % of its bits change")
        assert moved < bar / 100 and frac >= 0.40
