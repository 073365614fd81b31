"""Case builders shared by the MX / fp8 matrix, tie and model tests (GPU and
host): byte rows with dead blocks, a second reference of the MX quantiser
written from the formats' definitions, deliberately wrong quantisers, and the
tie input -- rows whose float32 quotients sit on, just below and just above
every rounding boundary of a result format.  numpy only; no GPU, no torch.
"""
import functools

import numpy as np

# exponent bits, mantissa bits, bias, codes that are not finite, emax of the MX contract
_FIELDS = {"e4m3": (4, 3, 7, (0x7F,), 8), "e5m2": (5, 2, 15, (0x7C, 0x7D, 0x7E, 0x7F), 15), "e2m1": (2, 1, 1, (), 2)}
TIE_E = (121, 134)  # the two block exponents of the tie input, neither 127


@functools.lru_cache(maxsize=None)
def magnitudes(fmt: str) -> np.ndarray:
    """The values of the finite non-negative codes 0, 1, 2, ... of fmt, in float64, decoded from the bit fields."""
    eb, mb, bias, special, _ = _FIELDS[fmt]
    vals = []
    for code in range(1 << (eb + mb)):
        if code in special:
            break
        e, m = code >> mb, code & ((1 << mb) - 1)
        vals.append(m / (1 << mb) * 2.0 ** (1 - bias) if e == 0 else (1 + m / (1 << mb)) * 2.0 ** (e - bias))
    v = np.array(vals, dtype=np.float64)
    assert (np.diff(v) > 0).all()
    return v


def midpoints(fmt: str) -> np.ndarray:
    """The midpoint of every pair of adjacent finite non-negative codes (exact in float64)."""
    m = magnitudes(fmt)
    return (m[:-1] + m[1:]) / 2


def _bf16_rne(y: np.ndarray) -> np.ndarray:
    b = y.astype(np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def quantise(v: np.ndarray, fmt: str, *, rounding="even", bf16_first=False, e_rounds_up=False, clamp=True,
             sign_from_rounded=False):
    """(element bytes, scale bytes) of the float32 quotients v, from the formats' definitions.

    The defaults are the contract: per block of 32, a non-finite quotient kills
    the block (E = 255, zero codes); else E = max(floor(log2(amax)) + 127 -
    emax, 0), y = v / 2^(E - 127) clamped to +-maxnorm, the nearest magnitude of
    fmt (a tie: the even code), the sign v's own.  Every keyword switches ONE
    deliberate mistake on: ties away from zero / truncation, a rounding to bf16
    first, E from amax rounded up to a power of two, no clamp (the next code up
    exists and is what an unclamped convert returns: NaN or inf), the sign of
    the rounded value (a negative quotient that rounds to zero loses it)."""
    mags, emax = magnitudes(fmt), _FIELDS[fmt][4]
    if not clamp:
        assert fmt != "e2m1", "a four-bit convert has no code past maxnorm to overflow into"
        mags = np.append(mags, 2 * mags[-1] - mags[-2])
    nb = (v.size + 31) // 32
    B = np.zeros(nb * 32, dtype=np.float64)
    B[:v.size] = v.astype(np.float64)
    B = B.reshape(nb, 32)
    dead = ~np.isfinite(B).all(axis=1)
    amax = np.abs(np.where(np.isfinite(B), B, 0.0)).max(axis=1)
    mant, ex = np.frexp(amax)  # amax = mant * 2^ex, mant in [.5, 1)
    if e_rounds_up:
        ex = np.where(mant > 0.5, ex + 1, ex)
    E = np.where(amax > 0, np.maximum(np.maximum(ex - 1 + 127, 0) - emax, 0), 0)
    y = np.abs(B) / np.exp2((E - 127).astype(np.float64))[:, None]
    if clamp:
        y = np.minimum(y, mags[-1])
    if bf16_first:
        y = _bf16_rne(y)
    y[dead] = 0.0
    hi = np.clip(np.searchsorted(mags, y, side="left"), 1, mags.size - 1)  # mags[hi - 1] <= y <= mags[hi] (or past the end)
    lo = hi - 1
    dl, dh = y - mags[lo], mags[hi] - y
    if rounding == "trunc":
        c = np.where(dh <= 0, hi, lo)
    elif rounding == "away":
        c = np.where(dh <= dl, hi, lo)
    else:
        c = np.where(dh < dl, hi, np.where(dl < dh, lo, np.where(lo % 2 == 0, lo, hi)))
    neg = (np.signbit(B) & (c > 0)) if sign_from_rounded else np.signbit(B)
    c = c | (neg & ~dead[:, None]).astype(np.int64) << (7 if fmt != "e2m1" else 3)
    E = np.where(dead, 255, E).astype(np.uint8)
    c = c.reshape(-1)
    if fmt == "e2m1":
        return (c[0::2] | c[1::2] << 4).astype(np.uint8)[:v.size // 2], E
    return c.astype(np.uint8)[:v.size], E


# the wrong quantisers of the discrimination test: name -> (keywords, formats it applies to)
WRONG = {
    "ties away from zero": (dict(rounding="away"), ("e4m3", "e5m2", "e2m1")),
    "truncation": (dict(rounding="trunc"), ("e4m3", "e5m2", "e2m1")),
    "bf16 first": (dict(bf16_first=True), ("e4m3", "e5m2", "e2m1")),
    "E from amax rounded up": (dict(e_rounds_up=True), ("e4m3", "e5m2", "e2m1")),
    "no clamp": (dict(clamp=False), ("e4m3", "e5m2")),
    "sign of the rounded value": (dict(sign_from_rounded=True), ("e4m3", "e5m2", "e2m1")),
}


# ---------------------------------------------------------------------------
# source rows: exact encodings
# ---------------------------------------------------------------------------
def _encode_e5m2(x: np.ndarray) -> np.ndarray:
    """The e5m2 codes of values that ARE e5m2 values (asserted); zero is +0."""
    mags = magnitudes("e5m2")
    c = np.searchsorted(mags, np.abs(x))
    assert (c < mags.size).all() and (mags[np.minimum(c, mags.size - 1)] == np.abs(x)).all(), "not an e5m2 value"
    return (c | ((x < 0) << 7)).astype(np.uint8)


def _lg(x):
    return np.frexp(x)[1] - 1  # floor(log2 x), x > 0


# ---------------------------------------------------------------------------
# the tie input
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_pieces(fmt: str):
    """([4, P] float64 pieces, [P] float32 quotients): column j's quotient is
    the sum of its four pieces, each a value of at most three significant bits
    (an e5m2 element times a power of two) -- the leading bits, the next bits,
    the +- one float32 step, and the anchor that fixes its block's amax -- and
    every partial sum is a float32.  Per block exponent E of TIE_E: every
    midpoint of fmt times 2^(E - 127) with its float32 neighbours in both signs,
    31 to a block beside an anchor of maxnorm; then two blocks with the same 31
    neighbours whose amax is the last float32 below 2^(emax + 1 + E - 127) and
    that power itself."""
    mags, emax = magnitudes(fmt), _FIELDS[fmt][4]
    cols = []  # (p0, p1, p2, anchor)

    def split(m):  # the leading three significant bits and the rest
        p0 = np.floor(np.ldexp(m, 2 - _lg(m))) * 2.0 ** (_lg(m) - 2) if m else 0.0
        return float(p0), float(m - p0)

    for E in TIE_E:
        s = 2.0 ** (E - 127)
        targets = []
        for m in midpoints(fmt) * s:
            f = np.float32(m)
            assert float(f) == m
            for t in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(np.inf))):
                for sign in (1.0, -1.0):
                    targets.append(tuple(sign * p for p in (*split(m), float(t) - m, 0.0)))
        near = targets[-31:]  # the 31 largest neighbours
        targets += [(0.0, 0.0, 0.0, 0.0)] * (-len(targets) % 31)
        for b in range(len(targets) // 31):
            blk = targets[31 * b:31 * b + 31]
            blk.insert((5 * b) % 32, (0.0, 0.0, 0.0, (-1.0) ** b * mags[-1] * s))
            cols += blk
        top = 2.0 ** (emax + 1) * s
        for anchor in ((0.0, 0.0, -top * 2.0 ** -24, top), (0.0, 0.0, 0.0, top)):
            cols += near[:7] + [anchor] + near[7:]
    pieces = np.array(cols, dtype=np.float64).T.copy()
    v = pieces.sum(axis=0)
    assert (v.astype(np.float32).astype(np.float64) == v).all()
    pieces.setflags(write=False)
    return pieces, v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def tie_mx_rows(fmt: str):
    """(q [4, P] e5m2 codes, E [4, P / 32] scale bytes, weights): MX e5m2 rows whose FedAvg quotients are
    tie_pieces(fmt)[1].  Row r carries piece r times 4 (the divisor), at a scale byte of its own per block."""
    pieces, _ = tie_pieces(fmt)
    P = pieces.shape[1]
    q, E = np.zeros((4, P), dtype=np.uint8), np.full((4, P // 32), 127, dtype=np.uint8)
    for r in range(4):
        for b in range(P // 32):
            x = 4 * pieces[r, 32 * b:32 * b + 32]
            if np.any(x):
                k = int(_lg(np.abs(x).max())) - 8  # the largest element in binade 8 of e5m2's -14 .. 15
                assert 0 < k + 127 < 255
                E[r, b] = k + 127
                q[r, 32 * b:32 * b + 32] = _encode_e5m2(x / 2.0 ** k)
    q.setflags(write=False), E.setflags(write=False)
    return q, E, [1, 1, 1, 1]


@functools.lru_cache(maxsize=None)
def tie_fp8_rows(fmt: str):
    """(b [N, P] e5m2 codes, scales, weights): plain fp8 rows with per-client scales= (powers of two) whose
    FedAvg quotients are tie_pieces(fmt)[1].  A row holds the pieces of one kind within 24 binades; N is
    padded to a power of two with zero rows, so the division is exact."""
    pieces, _ = tie_pieces(fmt)
    rows = []  # (base exponent, [P] values)
    for r in range(4):
        x = pieces[r]
        if not x.any():  # e2m1's midpoints have three significant bits: no second piece
            continue
        lg =np.where(x != 0, _lg(np.where(x != 0, np.abs(x), 1.0)), 0)
        lo = int(lg[x != 0].min())
        for k in range(lo, int(lg[x != 0].max()) + 1, 24):
            rows.append((k, np.where((x != 0) & (lg >= k) & (lg < k + 24), x, 0.0)))
    N = 1 << (len(rows) - 1).bit_length()
    b, scales = np.zeros((N, pieces.shape[1]), dtype=np.uint8), [1.0] * N
    for i, (k, x) in enumerate(rows):
        b[i] = _encode_e5m2(x / 2.0 ** (k + 12))  # elements in binades -12 .. 11
        scales[i] = float(N * 2.0 ** (k + 12))
    b.setflags(write=False)
    return b, scales, [1] * N


def tie_coverage(v: np.ndarray, fmt: str):
    """Assert on the float32 quotients v alone that they are a tie input of fmt; returns the block exponents
    at which the whole coverage holds (two or more, none 127)."""
    mags, emax = magnitudes(fmt), _FIELDS[fmt][4]
    assert v.dtype == np.float32 and v.size % 32 == 0 and np.isfinite(v).all()
    assert (np.abs(v[v != 0]) >= np.finfo(np.float32).tiny).all(), "every quotient a normal float32"
    B = v.reshape(-1, 32)
    bits = B.view(np.uint32)
    amax = np.abs(B).max(axis=1)
    E = (amax.view(np.uint32) >> 23).astype(np.int64) - emax
    assert (E > 0).all()
    covered = []
    for e in np.unique(E):
        s = np.float32(2.0 ** (int(e) - 127))
        have = set(bits[E == e].reshape(-1).tolist())
        mids = (midpoints(fmt) * float(s)).astype(np.float32)
        assert mids.size == mags.size - 1 == {"e2m1": 7, "e4m3": 126, "e5m2": 123}[fmt]
        want = np.concatenate([mids, np.nextafter(mids, np.float32(0)), np.nextafter(mids, np.float32(np.inf))])
        want = np.concatenate([want, -want])
        if not set(want.view(np.uint32).tolist()) <= have:
            continue
        # the clamp: an amax that is the largest float32 of maxnorm's binade, at this E
        if not ((E == e) & ((amax.view(np.uint32) & 0x7FFFFF) == 0x7FFFFF)).any():
            continue
        # the block-exponent boundary: amax the float32 below a power of two at this E, amax that power at E + 1,
        # the other 31 quotients the same bits
        pairs = 0
        for a in np.flatnonzero((E == e) & ((amax.view(np.uint32) & 0x7FFFFF) == 0x7FFFFF)):
            for c in np.flatnonzero((E == e + 1) & (amax == np.nextafter(amax[a], np.float32(np.inf)))):
                ia, ic = np.abs(B[a]).argmax(), np.abs(B[c]).argmax()
                same = np.delete(bits[a], ia).tolist() == np.delete(bits[c], ic).tolist()
                pairs += int(ia == ic and same and np.count_nonzero(np.delete(B[a], ia)) >= 16)
        if pairs:
            covered.append(int(e))
    assert len(covered) >= 2 and 127 not in covered, f"{fmt}: full coverage at block exponents {covered} only"
    return covered


# ---------------------------------------------------------------------------
# rows with dead blocks (the instantiation matrix)
# ---------------------------------------------------------------------------
def with_dead_blocks(kind: str, q: np.ndarray, E, nan_col: int, inf_col: int):
    """Copies of the element bytes q [N, row bytes] (and scale bytes E [N, blocks], None for plain fp8 rows)
    in which column nan_col's block holds a NaN in row 1 and column inf_col's block an infinity (where the
    format has none: an overflow under scale byte 254, or for plain e4m3fn rows a second NaN) in the last
    row; returns (q, E, the sorted dead blocks).  kind: "e4m3fn" / "e5m2" (plain fp8), "mx_e4m3", "mx_e5m2",
    "mx_e2m1"."""
    q, E = np.array(q), (None if E is None else np.array(E))
    N = q.shape[0]
    if kind == "mx_e2m1":  # no NaN and no infinity among the codes: the scale byte's NaN; 6 * 2^127 overflows
        E[1, nan_col // 32] = 255
        q[N - 1, inf_col // 2] = 0x77
        E[N - 1, inf_col // 32] = 254
    elif kind == "mx_e4m3":  # 448 * 2^127 overflows
        q[1, nan_col], q[N - 1, inf_col], E[N - 1, inf_col // 32] = 0x7F, 0x7E, 254
    elif kind == "e4m3fn":
        q[1, nan_col], q[N - 1, inf_col] = 0x7F, 0xFF
    else:
        q[1, nan_col], q[N - 1, inf_col] = 0x7F, 0x7C
    return q, E, sorted({nan_col // 32, inf_col // 32})
