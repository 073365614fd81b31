"""Edge-value inputs for the fold kernels: signed zeros, subnormals, overflow,
inf, NaN, zero weights, bf16 rounding ties.  Deterministic: seed and shape
give the same bits every time.

A matrix starts from the synthetic generator (fedlesscan_amd.synth) and has
its columns overwritten by class, class = column % K (CLASSES names them);
class 0 stays the untouched control.  The same classes exist as float32,
bf16 bit patterns and float64.  factor_sets() gives the client factors to
fold them with, left_fold() the literal numpy fold the tests answer to.

leading_neg_zero has -0.0 in row 0 and +0.0 below it, and in every other of
its columns the mirror (+0.0 first, -0.0 below): with a zero weight on row 0
that column is +0.0, but -0.0 if the zero-weight client is skipped.
subnormal_inputs keeps every 16th of its columns all +0.0.  one_neg_inf is
one_pos_inf's counterpart, so that -inf results exist for a single client too.

The near-max class is written against the `ordinary` cardinalities of the same
seed (x_i = c * MAX / n_i), so that under those factors its terms are known
fractions of the largest finite value: two of +0.9 and one of -0.9 overflow
in one order and stay finite in the other.
"""
from __future__ import annotations

import numpy as np

from fedlesscan_amd import synth

CLASSES = ("control", "all_neg_zero", "leading_neg_zero", "subnormal_inputs", "smallest_normals", "near_max",
           "one_pos_inf", "one_neg_inf", "both_infs", "one_nan", "cancellation", "random_bits", "bf16_tie")
K = len(CLASSES)
CLS = {name: i for i, name in enumerate(CLASSES)}

_F32_MAX = float(np.finfo(np.float32).max)
_F64_MAX = float(np.finfo(np.float64).max)


def _rng(seed, N, P, tag):
    return np.random.default_rng([int(seed), int(N), int(P), int(tag)])


def class_columns(P: int, name: str) -> np.ndarray:
    return np.arange(CLS[name], P, K)


def _rows_for(rng, N, n):
    """n random row indices in [0, N)."""
    return rng.integers(0, N, size=n)


# the terms of a near-max column under the ordinary factors, as fractions of the
# largest finite value, by column sub-pattern (column // K) % 4:
#   0  +.9 +.9 -.9 first: inf in client order, finite in reverse
#   1  -.9 +.9 +.9 last:  finite in client order, inf in reverse
#   2  as 0 without the 1/n_i scale: overflows in order under the identity factors
#   3  the mirror of 0: -inf in client order
_BIG = 0.9
_SMALL = 0.0003  # 297 of them stay below 0.1: they never decide an overflow


def _near_max_fractions(rng, N, ncols):
    F = rng.uniform(-_SMALL, _SMALL, size=(N, ncols))
    sub = np.arange(ncols) % 4
    lead = np.array([_BIG, _BIG, -_BIG])
    for k in range(min(N, 3)):
        F[k, (sub == 0) | (sub == 2)] = lead[k]
        F[k, sub == 3] = -lead[k]
        F[N - 1 - k, sub == 1] = lead[k]
    return F, sub


def _near_max(rng, seed, N, ncols, fmax):
    F, sub = _near_max_fractions(rng, N, ncols)
    w = np.array(synth.cardinalities(seed, N), np.float64)[:, None]
    V = F * fmax
    V[:, sub != 2] /= np.broadcast_to(w, V.shape)[:, sub != 2]
    return V


def _one_per_column(N, ncols, rows, value, dtype, base=0.0):
    M = np.full((N, ncols), base, dtype=dtype)
    M[rows, np.arange(ncols)] = value
    return M


def _second_rows(rng, N, rows):
    """A row different from rows[j] for every column (N >= 2)."""
    return (rows + 1 + rng.integers(0, N - 1, size=rows.size)) % N


def _cancel(M):
    """rows 2k+1 = -rows 2k; an unpaired last row is -0.0."""
    N = M.shape[0]
    M[1::2] = -M[0:N - (N % 2):2]
    if N % 2:
        M[N - 1] = -0.0
    return M


def _bf16_tie_f32(rng, N, ncols):
    """float32 values on and beside the bf16 rounding ties, one per column in a
    random row, +0.0 elsewhere: under the identity factors they reach the
    output unchanged."""
    sub = np.arange(ncols) % 12
    hi = rng.integers(0x0080, 0x7F00, size=ncols).astype(np.uint32)  # a normal, finite upper half
    even, odd = hi & ~np.uint32(1), hi | np.uint32(1)
    lo = np.zeros(ncols, np.uint32)
    up = hi.copy()
    tab = [(even, 0x8000), (odd, 0x8000), (even, 0x7FFF), (odd, 0x7FFF), (even, 0x8001), (odd, 0x8001),
           (None, 0x7FFF), (None, 0x8000), (None, 0xFFFF),  # within half a bf16 ulp of the bf16 maximum
           ("sub", 0x8000), ("sub", 0x7FFF), ("sub", 0x8001)]  # the bf16 subnormal range
    for k, (u, l) in enumerate(tab):
        m = sub == k
        if u is None:
            up[m] = 0x7F7F
        elif isinstance(u, str):
            up[m] = rng.integers(0, 0x0080, size=int(m.sum()))
        else:
            up[m] = u[m]
        lo[m] = l
    bits = (up << np.uint32(16)) | lo
    bits |= (rng.integers(0, 2, size=ncols).astype(np.uint32) << np.uint32(31))
    return _one_per_column(N, ncols, _rows_for(rng, N, ncols), bits.view(np.float32), np.float32)


def matrix_f32(seed: int, N: int, P: int) -> np.ndarray:
    X = synth.clients_f32(seed, N, 0, P)

    def cols(name):
        c = class_columns(P, name)
        return c, _rng(seed, N, P, CLS[name])

    c, _ = cols("all_neg_zero")
    X[:, c] = -0.0
    c, _ = cols("leading_neg_zero")
    X[:, c] = 0.0
    X[0, c] = -0.0
    X[:, c[1::2]] = -X[:, c[1::2]]  # every other column mirrored: +0.0 first, -0.0 in the rest
    c, r = cols("subnormal_inputs")
    k = r.integers(-40, 41, size=(N, c.size))
    k[:, ::16] = 0  # every 16th column of the class is all +0.0
    X[:, c] = (k.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    c, r = cols("smallest_normals")
    b = r.integers(0x00800000, 0x01000000, size=(N, c.size)).astype(np.uint32)
    b |= r.integers(0, 2, size=b.shape).astype(np.uint32) << np.uint32(31)
    X[:, c] = b.view(np.float32)
    c, r = cols("near_max")
    X[:, c] = _near_max(r, seed, N, c.size, _F32_MAX).astype(np.float32)
    c, r = cols("one_pos_inf")
    X[_rows_for(r, N, c.size), c] = np.inf
    c, r = cols("one_neg_inf")
    X[_rows_for(r, N, c.size), c] = -np.inf
    c, r = cols("both_infs")
    rows = _rows_for(r, N, c.size)
    X[rows, c] = np.inf
    if N > 1:
        X[_second_rows(r, N, rows), c] = -np.inf
    c, r = cols("one_nan")
    X[_rows_for(r, N, c.size), c] = np.nan
    c, _ = cols("cancellation")
    X[:, c] = _cancel(X[:, c])
    c, r = cols("random_bits")
    b = r.integers(0, 1 << 32, size=(N, c.size), dtype=np.uint64).astype(np.uint32)
    b = np.where((b >> np.uint32(23)) & np.uint32(0xFF) == 0xFF, b & ~np.uint32(1 << 23), b)  # exponent 254: finite
    X[:, c] = b.view(np.float32)
    c, r = cols("bf16_tie")
    X[:, c] = _bf16_tie_f32(r, N, c.size)
    return X


def _bf16_exp2(e: np.ndarray) -> np.ndarray:
    """bf16 bits of 2**e, normal range."""
    return ((e + 127).astype(np.uint16) << np.uint16(7)).astype(np.uint16)


def _bf16_tie_bits(rng, N, ncols):
    """bf16 rows whose exact float32 sum (identity factors) sits on or beside a
    bf16 rounding tie: row 0 the upper half h, row 1 half a bf16 ulp of it,
    row 2 one float32 ulp up or down; every add is exact.  Sub-patterns:
    tie with an even and an odd h, the 0x7FFF / 0x8001 neighbours, the bf16
    maximum plus half an ulp (a finite float32 that rounds to inf) and just
    below it, a bf16 subnormal alone, a negative tie.  One row: h alone; two
    rows: the ties without their neighbours."""
    M = np.zeros((N, ncols), np.uint16)
    sub = np.arange(ncols) % 8
    e = rng.integers(-60, 61, size=ncols)
    mant = rng.integers(0, 128, size=ncols).astype(np.uint16)
    mant = np.where(np.isin(sub, (0, 2, 7)), mant & ~np.uint16(1), mant)
    mant = np.where(np.isin(sub, (1, 3)), mant | np.uint16(1), mant)
    h = _bf16_exp2(e) | mant
    top = np.isin(sub, (4, 5))
    h = np.where(top, np.uint16(0x7F7F), h)
    e = np.where(top, 127, e)
    half, ulp = _bf16_exp2(e - 8), _bf16_exp2(e - 23)
    neg = np.uint16(0x8000)
    sgn = np.where(sub == 7, neg, np.uint16(0))
    M[0] = h | sgn
    if N > 1:
        M[1] = half | sgn
    if N > 2:
        M[2] = np.where(np.isin(sub, (2, 5)), ulp | neg, np.where(sub == 3, ulp, np.uint16(0)))
    s6 = sub == 6
    M[:, s6] = 0
    M[rng.integers(0, N, size=int(s6.sum())), np.flatnonzero(s6)] = (
        rng.integers(1, 0x0080, size=int(s6.sum())).astype(np.uint16)
        | (rng.integers(0, 2, size=int(s6.sum())).astype(np.uint16) << np.uint16(15)))
    return M


def bf16_rne_independent(x_f32: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bits by PyTorch's CPU conversion (round to nearest even):
    an implementation that does not share the kernel's or the oracle's expression."""
    import torch
    x = np.ascontiguousarray(x_f32, dtype=np.float32)
    return torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def matrix_bf16(seed: int, N: int, P: int) -> np.ndarray:
    """[N, P] bf16 bit patterns (uint16), the classes of matrix_f32."""
    X = synth.clients_bf16(seed, N, 0, P)
    NEG0, PINF, NINF, NAN = 0x8000, 0x7F80, 0xFF80, 0x7FC0

    def cols(name):
        c = class_columns(P, name)
        return c, _rng(seed, N, P, 100 + CLS[name])

    def sign(r, shape):
        return r.integers(0, 2, size=shape).astype(np.uint16) << np.uint16(15)

    c, _ = cols("all_neg_zero")
    X[:, c] = NEG0
    c, _ = cols("leading_neg_zero")
    X[:, c] = 0
    X[0, c] = NEG0
    X[:, c[1::2]] ^= np.uint16(NEG0)  # every other column mirrored: +0.0 first, -0.0 in the rest
    c, r = cols("subnormal_inputs")
    k = r.integers(0, 41, size=(N, c.size)).astype(np.uint16) | sign(r, (N, c.size))
    k[:, ::16] = 0  # every 16th column of the class is all +0.0
    X[:, c] = k
    c, r = cols("smallest_normals")
    X[:, c] = r.integers(0x0080, 0x0100, size=(N, c.size)).astype(np.uint16) | sign(r, (N, c.size))
    c, r = cols("near_max")
    X[:, c] = bf16_rne_independent(_near_max(r, seed, N, c.size, _F32_MAX).astype(np.float32)).reshape(N, c.size)
    c, r = cols("one_pos_inf")
    X[_rows_for(r, N, c.size), c] = PINF
    c, r = cols("one_neg_inf")
    X[_rows_for(r, N, c.size), c] = NINF
    c, r = cols("both_infs")
    rows = _rows_for(r, N, c.size)
    X[rows, c] = PINF
    if N > 1:
        X[_second_rows(r, N, rows), c] = NINF
    c, r = cols("one_nan")
    X[_rows_for(r, N, c.size), c] = NAN
    c, _ = cols("cancellation")
    sub = X[:, c]
    sub[1::2] = sub[0:N - (N % 2):2] ^ np.uint16(NEG0)
    if N % 2:
        sub[N - 1] = NEG0
    X[:, c] = sub
    c, r = cols("random_bits")
    b = r.integers(0, 1 << 16, size=(N, c.size)).astype(np.uint16)
    X[:, c] = np.where((b >> np.uint16(7)) & np.uint16(0xFF) == 0xFF, b & ~np.uint16(1 << 7), b)
    c, r = cols("bf16_tie")
    X[:, c] = _bf16_tie_bits(r, N, c.size)
    return X


def matrix_f64(seed: int, N: int, P: int) -> np.ndarray:
    """The classes at double's ranges (bf16_tie: values on the float32 rounding ties)."""
    X = synth.clients_f32(seed, N, 0, P).astype(np.float64) * (1.0 + 1.0 / 3.0)

    def cols(name):
        c = class_columns(P, name)
        return c, _rng(seed, N, P, 200 + CLS[name])

    def sign(r, shape):
        return r.integers(0, 2, size=shape).astype(np.uint64) << np.uint64(63)

    c, _ = cols("all_neg_zero")
    X[:, c] = -0.0
    c, _ = cols("leading_neg_zero")
    X[:, c] = 0.0
    X[0, c] = -0.0
    X[:, c[1::2]] = -X[:, c[1::2]]  # every other column mirrored: +0.0 first, -0.0 in the rest
    c, r = cols("subnormal_inputs")
    k = r.integers(0, 41, size=(N, c.size)).astype(np.uint64) | sign(r, (N, c.size))
    k[:, ::16] = 0  # every 16th column of the class is all +0.0
    X[:, c] = k.view(np.float64)
    c, r = cols("smallest_normals")
    b = r.integers(1 << 52, 1 << 53, size=(N, c.size)).astype(np.uint64) | sign(r, (N, c.size))
    X[:, c] = b.view(np.float64)
    c, r = cols("near_max")
    X[:, c] = _near_max(r, seed, N, c.size, _F64_MAX)
    c, r = cols("one_pos_inf")
    X[_rows_for(r, N, c.size), c] = np.inf
    c, r = cols("one_neg_inf")
    X[_rows_for(r, N, c.size), c] = -np.inf
    c, r = cols("both_infs")
    rows = _rows_for(r, N, c.size)
    X[rows, c] = np.inf
    if N > 1:
        X[_second_rows(r, N, rows), c] = -np.inf
    c, r = cols("one_nan")
    X[_rows_for(r, N, c.size), c] = np.nan
    c, _ = cols("cancellation")
    X[:, c] = _cancel(X[:, c])
    c, r = cols("random_bits")
    b = r.integers(0, 1 << 63, size=(N, c.size)).astype(np.uint64) | sign(r, (N, c.size))
    b = np.where((b >> np.uint64(52)) & np.uint64(0x7FF) == 0x7FF, b & ~np.uint64(1 << 52), b)
    X[:, c] = b.view(np.float64)
    c, r = cols("bf16_tie")
    b = r.integers(1 << 52, 0x7FE << 52, size=c.size).astype(np.uint64)
    b = (b & ~np.uint64((1 << 29) - 1)) | np.uint64(1 << 28)
    X[:, c] = _one_per_column(N, c.size, _rows_for(r, N, c.size), b.view(np.float64), np.float64)
    return X


FACTOR_SETS = ("ordinary", "identity", "zero_weights", "zero_total", "fractional", "huge_divisor")


def factor_sets(seed: int, N: int, dtype=np.float32):
    """Yields (name, a, s_or_None, divisor): every set of FACTOR_SETS twice,
    first without scores, then with its scores.  a, s: arrays of `dtype`,
    divisor: a scalar of it.  The C-ABI and the oracle take the three as
    independent arguments, so the divisor need not be the weights' sum."""
    dt = np.dtype(dtype).type
    r = _rng(seed, N, 0, 300)
    card = synth.cardinalities(seed, N)
    sc = np.array([(k + 1) / 11 for k in synth.round_ids(seed, N, 10, 2)], dtype=dt)
    ones = np.ones(N, dt)
    zw = r.integers(0, 4, size=N)
    zw[0] = zw[-1] = 0
    menu = np.array([0.1, 2.5, 1 / 3, 7.75, 1e-3], np.float64)
    frac = np.where(np.arange(N) % 3 == 2, 2.0 ** -20 * (1 + np.arange(N)), menu[r.integers(0, menu.size, size=N)])
    fsc = r.choice(np.array([1 / 3, 0.7, 1.0, 1e-2]), size=N).astype(dt)
    sets = [
        ("ordinary", np.array(card, dt), sc, dt(sum(card))),
        ("identity", ones, ones, dt(1)),
        # the divisor of an all-zero draw (N <= 2) is 1, so that the set differs from zero_total
        ("zero_weights", zw.astype(dt), sc, dt(int(zw.sum()) or 1)),
        ("zero_total", np.zeros(N, dt), sc, dt(0)),
        ("fractional", frac.astype(dt), fsc, dt(frac.astype(dt).astype(np.float64).sum())),
        # smallest normals (2**-126, at double 2**-1022) times a weight of a few hundred, summed,
        # over 2**18.45: quotients around 2**-136 (2**-1032), subnormal and nonzero
        ("huge_divisor", np.array(card, dt), sc, dt(2.0 ** 18 * 1.37)),
    ]
    assert tuple(n for n, *_ in sets) == FACTOR_SETS
    for name, a, s, d in sets:
        yield name, a, None, d
        yield name, a, s.copy(), d


def set_id(name, s) -> str:
    return f"{name}-{'plain' if s is None else 'scored'}"


def upcast_bf16(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def left_fold(X: np.ndarray, a: np.ndarray, divisor, s: np.ndarray | None = None) -> np.ndarray:
    """The literal fold in the matrix's own dtype: one np.multiply (two with
    scores) and one np.add per client, in order, then a true divide.  bf16 bit
    patterns (uint16) are upcast exactly and folded in float32."""
    if X.dtype == np.uint16:
        X = upcast_bf16(X)
    dt = X.dtype.type
    assert X.dtype in (np.float32, np.float64)
    with np.errstate(all="ignore"):
        acc = None
        for i in range(X.shape[0]):
            t = np.multiply(X[i], dt(a[i]))
            if s is not None:
                t = np.multiply(t, dt(s[i]))
            acc = t if acc is None else np.add(acc, t)
        out = np.true_divide(acc, dt(divisor))
    assert out.dtype == X.dtype
    return out


def is_nan_bf16(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, np.uint16) & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def same_bf16_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal bf16 bit patterns, except where both are NaN patterns (sign and payload unspecified)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint16 or b.dtype != np.uint16 or a.shape != b.shape:
        return False
    both = is_nan_bf16(a) & is_nan_bf16(b)
    return bool(np.array_equal(a[~both], b[~both]))


def bf16_matches_independent(bits: np.ndarray, f32: np.ndarray) -> bool:
    """bits == the independent rounding of f32 wherever f32 is not NaN."""
    ok = ~np.isnan(f32)
    return bool(np.array_equal(np.asarray(bits, np.uint16)[ok], bf16_rne_independent(f32)[ok]))
