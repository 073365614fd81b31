"""GPU parity of the float64 pair folds (raw ABI): the chunked fold fa_fold_f64
and the row-table fold fa_fedavg_f64_ptrs.

Every result is compared bit for bit (view(np.uint64)), NaN by position, with
numpy's literal float64 left fold `reduce(np.add, [x_i * n_i (* s_i)]) / sum(n)`,
with oracle_lib.fedavg_f64 and with fa_fedavg_f64 over the same rows.

Ordinary inputs are synth.clients_f32(...).astype(float64) * (1 + 1/3), which
fills the low mantissa bits, with synth.cardinalities weights;
tests/test_f64_host.py keeps on record that these inputs tell the left fold
from a reversed, fused, reciprocal-divided, float32-rounded or once-rounded one.

Shapes.  The form is fixed by width: a lane owns 4, 2 or 1 pairs of columns,
the most whose balanced grid still covers 7/8 of the CUs, so every narrow shape
takes 1 pair per lane: T = 512 columns per full tile.  Rows ahead U: 4 for the
chunked fold, 8 for the row table.  P runs over 1, 2, 3, T-1, T, T+1,
2T + T/2 + 1 and (CUs + 44) T + 7 (more than one pass over the CUs; N = 3), and
over the two narrowest widths at which the 2-pair and the 4-pair form take
over (a partial last tile and an odd column; N = 3, and N = 2U + 3 so that the
U-rows-ahead loop of those forms runs: 11 rows for the chunked fold, 19 for the
row table, 20-70 MB of input, the least these forms can be given on 256 CUs);
N over 1, 2, U-1, U, U+1, 2U+3 and 33."""
from functools import reduce

import numpy as np
import pytest

from fedlesscan_amd import synth
from oracle import oracle_lib as OL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64 = np.float64
SENTINEL = 0x5A5A5A5A5A5A5A5A  # an element the kernel never writes keeps this pattern
PAD = 16
T = 512
U_FOLD, U_ROWS = 4, 8
PS_SMALL = [1, 2, 3, T - 1, T, T + 1, 2 * T + T // 2 + 1]
SEED = 11


def _ns(U):
    return sorted({1, 2, U - 1, U, U + 1, 2 * U + 3, 33})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from fedlesscan_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _grid(P, C, cus):
    units = (P >> 1) + (P & 1)
    tiles = -(-units // (256 * C))
    g = min(cus, tiles)
    passes = -(-tiles // g)
    return -(-tiles // passes)


def pick_pairs(P, cus):
    """The library's policy (fold_kernels.hpp pick_pairs), restated."""
    for c in (4, 2):
        if _grid(P, c, cus) * 8 >= cus * 7:
            return c
    return 1


def wide_ps(cus):
    """(P, pairs per lane): more than one pass of the 1-pair form; the narrowest
    widths of the 2-pair and 4-pair forms, each with a partial last tile and an
    odd last column."""
    need = -(-7 * cus // 8)
    out = [((cus + 44) * T + 7, 1), (2 * 512 * need - 512 + 3, 2), (2 * 1024 * need - 1024 + 3, 4)]
    for P, c in out:
        assert pick_pairs(P, cus) == c, (P, c)
    return out


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F64 or b.dtype != F64 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~na]))


def _describe(got, exp):
    na, nb = np.isnan(got), np.isnan(exp)
    bad = np.flatnonzero((na != nb) | ((got.view(np.uint64) != exp.view(np.uint64)) & ~(na & nb)))
    i = int(bad[0]) if bad.size else -1
    return f"{bad.size} differ; first col {i}: got {got.view(np.uint64)[i]:#018x} exp {exp.view(np.uint64)[i]:#018x}"


def _numpy_fold(X, a, s, d):
    """(running, final): numpy's float64 left fold of the terms of rows 0..i,
    and running[-1] / d.  a, s, d are float64 values."""
    with np.errstate(all="ignore"):
        terms = [np.multiply(X[i], F64(a[i])) if s is None else np.multiply(np.multiply(X[i], F64(a[i])), F64(s[i]))
                 for i in range(X.shape[0])]
        running = [terms[0]]
        for t in terms[1:]:
            running.append(np.add(running[-1], t))
        final = np.true_divide(running[-1], F64(d))
        assert same_bits(reduce(np.add, terms) / F64(d), final)  # the literal form itself
        assert same_bits(OL.fedavg_f64(np.ascontiguousarray(X), np.asarray(a, F64), float(d),
                                       s=None if s is None else np.asarray(s, F64)), final)
    return running, final


_cache = {}


def _case(N, P, scored):
    key = (N, P, scored)
    if key not in _cache:
        X = synth.clients_f32(SEED + N, N, 0, P).astype(F64) * (1.0 + 1.0 / 3.0)
        w = synth.cardinalities(SEED + N, N)
        sc = [float(k + 1) / 11 for k in synth.round_ids(SEED + N, N, 10, 2)] if scored else None
        a = np.array(w, F64)
        s = None if sc is None else np.array(sc, F64)
        running, final = _numpy_fold(X, a, s, float(sum(w)))
        assert np.isfinite(final).all() and final.any()
        _cache[key] = (X, a, s, float(sum(w)), running, final)
    return _cache[key]


class Fold:
    """The rows on the device at pitch ldx (16-B aligned base, or 8 bytes past
    it with x_off), the factors as doubles, and two sentinel-filled output
    buffers (16-B aligned, or 8 bytes past that with acc_off)."""

    def __init__(self, dev, L, X, a, s, d, ldx=None, x_off=0, acc_off=0):
        self.dev, self.L = dev, L
        self.N, self.P = X.shape
        self.ldx = ldx or (self.P + 63) // 64 * 64
        Xp = np.zeros(self.N * self.ldx + 2, F64)
        self.x_off = x_off
        Xp[x_off:x_off + self.N * self.ldx].reshape(self.N, self.ldx)[:, :self.P] = X
        self.X = torch.from_numpy(Xp).to(dev)
        self.a = torch.from_numpy(np.ascontiguousarray(a, F64)).to(dev)
        self.s = None if s is None else torch.from_numpy(np.ascontiguousarray(s, F64)).to(dev)
        self.d = float(d)
        self.off = acc_off
        self.bufs = [torch.full((self.P + PAD,), SENTINEL, dtype=torch.int64, device=dev) for _ in range(2)]
        self.st = torch.cuda.current_stream(dev).cuda_stream
        assert self.X.data_ptr() % 16 == 0 and all(b.data_ptr() % 16 == 0 for b in self.bufs)

    def xptr(self, i0=0):
        return self.X.data_ptr() + 8 * (self.x_off + i0 * self.ldx)

    def ptr(self, k):
        return self.bufs[k].data_ptr() + 8 * self.off

    def read(self, k):
        h = self.bufs[k].cpu().numpy().view(np.uint64)
        assert (h[:self.off] == SENTINEL).all() and (h[self.off + self.P:] == SENTINEL).all(), "wrote out of range"
        return h[self.off:self.off + self.P].copy().view(F64)

    def call(self, i0, n, acc_in, fin, out, d=None):
        """Rows [i0, i0 + n) into buffer `out`, continuing from buffer acc_in (None: a fresh fold)."""
        return self.L.fa_fold_f64(self.xptr(i0) if n else None, n, self.P, self.ldx,
                                  self.a.data_ptr() + 8 * i0 if n else None,
                                  self.s.data_ptr() + 8 * i0 if (n and self.s is not None) else None,
                                  None if acc_in is None else self.ptr(acc_in),
                                  (self.d if d is None else d) if fin else 0.0, int(fin), self.ptr(out), self.st)

    def fedavg(self):
        """fa_fedavg_f64 over the same rows (fresh, 16-B aligned output)."""
        out = torch.full((self.P + PAD,), SENTINEL, dtype=torch.int64, device=self.dev)
        rc = self.L.fa_fedavg_f64(self.xptr(), self.N, self.P, self.ldx, self.a.data_ptr(),
                                  None if self.s is None else self.s.data_ptr(), self.d, out.data_ptr(), self.st)
        assert rc == 0
        h = out.cpu().numpy().view(np.uint64)
        assert (h[self.P:] == SENTINEL).all()
        return h[:self.P].copy().view(F64)


def _cuts(N):
    """Three uneven cuts of N rows (fewer when N < 3), none empty."""
    c1, c2 = (N + 2) // 4, (N + 1) // 2 + (N > 4)
    segs = [(0, c1), (c1, c2), (c2, N)]
    return [(i0, i1 - i0) for i0, i1 in segs if i1 > i0]


def _check_fold(f, running, final, what):
    # one fold, against fa_fedavg_f64 and numpy
    assert f.call(0, f.N, None, True, 0) == 0, what
    got = f.read(0)
    assert same_bits(got, final), (what, "one fold", _describe(got, final))
    ref = f.fedavg()
    assert same_bits(got, ref), (what, "fa_fedavg_f64", _describe(got, ref))
    # the same rows in uneven cuts, the accumulator in place (acc_in == out), never finalised:
    # numpy's running sum; then a finalize-only call (N == 0) in place
    cuts = _cuts(f.N)
    assert sum(n for _, n in cuts) == f.N
    for k, (i0, n) in enumerate(cuts):
        assert f.call(i0, n, None if k == 0 else 1, False, 1) == 0, what
        got = f.read(1)
        assert same_bits(got, running[i0 + n - 1]), (what, "running sum after cut", k, _describe(got, running[i0 + n - 1]))
    assert f.call(0, 0, 1, True, 1) == 0, what
    got = f.read(1)
    assert same_bits(got, final), (what, "cuts + finalize only", _describe(got, final))
    # the last cut finalises itself; the accumulator comes from the other buffer
    if len(cuts) > 1:
        for k, (i0, n) in enumerate(cuts[:-1]):
            assert f.call(i0, n, None if k == 0 else 0, False, 0) == 0, what
        i0, n = cuts[-1]
        assert f.call(i0, n, 0, True, 1) == 0, what
        got = f.read(1)
        assert same_bits(got, final), (what, "last cut finalises", _describe(got, final))


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("P", PS_SMALL)
def test_fold_f64_grid(dev, L, P, scored):
    for N in _ns(U_FOLD):
        X, a, s, d, running, final = _case(N, P, scored)
        _check_fold(Fold(dev, L, X, a, s, d), running, final, (N, P, scored))


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["two_passes", "two_pairs", "four_pairs"])
def test_fold_f64_wide(dev, L, cus, which, scored):
    P, _ = wide_ps(cus)[which]
    X, a, s, d, running, final = _case(3, P, scored)
    _check_fold(Fold(dev, L, X, a, s, d), running, final, (3, P, scored))


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("which", [1, 2], ids=["two_pairs", "four_pairs"])
def test_fold_f64_wide_rows_ahead(dev, L, cus, which, scored):
    """2 and 4 pairs per lane with 2U + 3 rows: the one fold runs the U rows x C
    pairs loop twice after the first row and then a leftover row; the cuts (3, 4
    and 4 rows) enter it from a carried accumulator."""
    P, _ = wide_ps(cus)[which]
    N = 2 * U_FOLD + 3
    assert [n for _, n in _cuts(N)] == [3, 4, 4]
    X, a, s, d, running, final = _case(N, P, scored)
    _check_fold(Fold(dev, L, X, a, s, d), running, final, (N, P, scored))
    _cache.pop((N, P, scored))  # tens of MB: not kept for the rest of the module


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("layout", ["x_off", "odd_ldx", "out_off"])
def test_fold_f64_unaligned_takes_the_column_kernel(dev, L, layout, scored):
    """Rows at an 8-byte offset, an odd pitch, an output (and accumulator) at an
    8-byte offset: one column per lane, the same bits."""
    for N, P in [(1, 1), (5, 3), (9, T + 1), (13, 2 * T + T // 2 + 1)]:
        X, a, s, d, running, final = _case(N, P, scored)
        kw = {"x_off": dict(x_off=1), "odd_ldx": dict(ldx=P + 1 + (P & 1)), "out_off": dict(acc_off=1)}[layout]
        f = Fold(dev, L, X, a, s, d, **kw)
        assert (f.xptr() % 16 != 0) or (f.ldx % 2 == 1) or (f.ptr(0) % 16 != 0)
        _check_fold(f, running, final, (layout, N, P, scored))


def test_fold_f64_status_codes(dev, L):
    from fedlesscan_amd import _lib
    X, a, s, d, running, final = _case(5, 3, False)
    f = Fold(dev, L, X, a, s, d)
    assert f.call(0, 0, None, True, 0) == _lib.FA_ERR_NO_CLIENTS  # N == 0 without acc_in
    assert "N == 0" in _lib.last_error()
    rc = L.fa_fold_f64(f.xptr(), 5, 3, 2, f.a.data_ptr(), None, None, d, 1, f.ptr(0), f.st)
    assert rc == _lib.FA_ERR_SHAPE  # ldx < P
    assert L.fa_fold_f64(f.xptr(), -1, 3, 64, f.a.data_ptr(), None, None, d, 1, f.ptr(0), f.st) == _lib.FA_ERR_ARG
    assert L.fa_fold_f64(None, 5, 3, 64, f.a.data_ptr(), None, None, d, 1, f.ptr(0), f.st) == _lib.FA_ERR_ARG
    assert L.fa_fold_f64(None, 0, 3, 64, None, None, f.ptr(0), d, 1, None, f.st) == _lib.FA_ERR_ARG  # null out
    assert L.fa_fold_f64(f.xptr(), 5, 0, 64, f.a.data_ptr(), None, None, d, 1, f.ptr(0), f.st) == 0  # P == 0
    torch.cuda.synchronize()
    assert (f.bufs[0].cpu().numpy().view(np.uint64) == SENTINEL).all()  # none of them wrote


# ---------------------------------------------------------------------------
# the row table
# ---------------------------------------------------------------------------
class Rows:
    """N separately allocated rows (16-B aligned, or views 8 bytes into their
    allocation with off=1), their pointer table and the factors on the device."""

    def __init__(self, dev, L, X, a, s, d, off=0):
        self.dev, self.L = dev, L
        self.N, self.P = X.shape
        self.keep = []
        ptrs = []
        for i in range(self.N):
            h = np.zeros(self.P + 2, F64)
            h[off:off + self.P] = X[i]
            t = torch.from_numpy(h).to(dev)
            assert t.data_ptr() % 16 == 0
            self.keep.append(t)
            ptrs.append(t.data_ptr() + 8 * off)
        self.table = torch.from_numpy(np.array(ptrs, np.int64)).to(dev)
        self.a = torch.from_numpy(np.ascontiguousarray(a, F64)).to(dev)
        self.s = None if s is None else torch.from_numpy(np.ascontiguousarray(s, F64)).to(dev)
        self.d = float(d)
        self.st = torch.cuda.current_stream(dev).cuda_stream

    def fold(self, aligned, out_off=0):
        out = torch.full((self.P + PAD,), SENTINEL, dtype=torch.int64, device=self.dev)
        rc = self.L.fa_fedavg_f64_ptrs(self.table.data_ptr(), self.N, self.P, self.a.data_ptr(),
                                       None if self.s is None else self.s.data_ptr(), self.d, int(aligned),
                                       out.data_ptr() + 8 * out_off, self.st)
        assert rc == 0
        h = out.cpu().numpy().view(np.uint64)
        assert (h[:out_off] == SENTINEL).all() and (h[out_off + self.P:] == SENTINEL).all(), "wrote out of range"
        return h[out_off:out_off + self.P].copy().view(F64)


def _check_rows(dev, L, X, a, s, d, final, what, offsets=True):
    stacked = Fold(dev, L, X, a, s, d).fedavg()  # fa_fedavg_f64 on the stacked rows
    assert same_bits(stacked, final), (what, "fa_fedavg_f64", _describe(stacked, final))
    r = Rows(dev, L, X, a, s, d)
    for aligned in (1, 0):
        got = r.fold(aligned)
        assert same_bits(got, final), (what, "aligned rows, rows_aligned", aligned, _describe(got, final))
        assert same_bits(got, stacked), (what, "against the stacked fold", aligned)
    if not offsets:
        return
    r = Rows(dev, L, X, a, s, d, off=1)  # views at an 8-byte offset
    for out_off in (0, 1):
        got = r.fold(0, out_off)
        assert same_bits(got, final), (what, "rows at an 8-byte offset, out offset", out_off, _describe(got, final))


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("P", PS_SMALL)
def test_rows_f64_grid(dev, L, P, scored):
    for N in _ns(U_ROWS):
        X, a, s, d, _, final = _case(N, P, scored)
        _check_rows(dev, L, X, a, s, d, final, (N, P, scored))


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["two_passes", "two_pairs", "four_pairs"])
def test_rows_f64_wide(dev, L, cus, which, scored):
    P, _ = wide_ps(cus)[which]
    X, a, s, d, _, final = _case(3, P, scored)
    _check_rows(dev, L, X, a, s, d, final, (3, P, scored))


@pytest.mark.parametrize("which", [1, 2], ids=["two_pairs", "four_pairs"])
def test_rows_f64_wide_rows_ahead(dev, L, cus, which):
    """2 and 4 pairs per lane with 2U + 3 = 19 rows: the 8 rows x C pairs loop
    runs twice after the first row, then two leftover rows.  Scored (both
    multiplies); the rows at an 8-byte offset take the column kernel whatever
    the width and are left to the narrower cases."""
    P, _ = wide_ps(cus)[which]
    N = 2 * U_ROWS + 3
    X, a, s, d, _, final = _case(N, P, True)
    _check_rows(dev, L, X, a, s, d, final, (N, P, "scored"), offsets=False)
    _cache.pop((N, P, True))  # tens of MB: not kept for the rest of the module


def test_rows_f64_status_codes(dev, L):
    from fedlesscan_amd import _lib
    X, a, s, d, _, final = _case(5, 3, False)
    r = Rows(dev, L, X, a, s, d)
    out = torch.full((8,), SENTINEL, dtype=torch.int64, device=dev)
    call = lambda N, P, al, o: L.fa_fedavg_f64_ptrs(r.table.data_ptr(), N, P, r.a.data_ptr(), None, d, al, o, r.st)
    assert call(0, 3, 1, out.data_ptr()) == _lib.FA_ERR_NO_CLIENTS
    assert call(-1, 3, 1, out.data_ptr()) == _lib.FA_ERR_ARG
    assert call(5, 3, 1, None) == _lib.FA_ERR_ARG
    assert call(5, 3, 1, out.data_ptr() + 8) == _lib.FA_ERR_ARG  # rows_aligned with out off 16-B alignment
    assert call(5, 0, 1, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint64) == SENTINEL).all()


# ---------------------------------------------------------------------------
# edge columns, in binary64: the class list of tests/edge_values.py
# ---------------------------------------------------------------------------
CLASSES = ("control", "all_neg_zero", "leading_neg_zero", "subnormal_inputs", "smallest_normals", "near_max_in_order",
           "near_max_reversed", "one_pos_inf", "one_neg_inf", "both_infs", "one_nan", "cancellation", "random_bits")
K = len(CLASSES)
MAX = float(np.finfo(F64).max)
EDGE_P = 2 * T + T // 2 + 1  # two full tiles, a partial one, the odd column
EDGE_NS = [1, 2, 3, 9, 33]


def edge_matrix(seed, N, P):
    """Column c holds class c % K; class 0 stays the ordinary control.  The
    near-max classes are written against the ordinary cardinalities of the same
    seed (x_i = f * MAX / n_i), so their terms are known fractions of MAX."""
    rng = np.random.default_rng([seed, N, P])
    X = synth.clients_f32(seed, N, 0, P).astype(F64) * (1.0 + 1.0 / 3.0)
    card = np.array(synth.cardinalities(seed, N), F64)
    cols = lambda name: np.arange(CLASSES.index(name), P, K)
    sign = lambda shape: rng.integers(0, 2, size=shape).astype(np.uint64) << np.uint64(63)
    row = lambda n: rng.integers(0, N, size=n)
    c = cols("all_neg_zero")
    X[:, c] = -0.0
    c = cols("leading_neg_zero")
    X[:, c] = 0.0
    X[0, c] = -0.0
    X[:, c[1::2]] = -X[:, c[1::2]]  # every other column mirrored: +0.0 first, -0.0 below
    c = cols("subnormal_inputs")  # 5e-324 ... 40 * 5e-324, either sign; every 8th column all +0.0
    k = rng.integers(0, 41, size=(N, c.size)).astype(np.uint64) | sign((N, c.size))
    k[:, ::8] = 0
    X[:, c] = k.view(F64)
    c = cols("smallest_normals")  # products and quotients under fractional or large factors are subnormal
    X[:, c] = (rng.integers(1 << 52, 1 << 53, size=(N, c.size)).astype(np.uint64) | sign((N, c.size))).view(F64)
    lead = [0.9, 0.9, -0.9]
    for name, rows in (("near_max_in_order", range(min(N, 3))), ("near_max_reversed", range(N - 1, max(N - 4, -1), -1))):
        c = cols(name)  # +.9 +.9 -.9 of MAX from one end: inf when folded from that end, finite from the other
        V = rng.uniform(-3e-4, 3e-4, size=(N, c.size)) * MAX
        for j, i in enumerate(rows):
            V[i] = lead[j] * MAX
        V[:, 1::2] = -V[:, 1::2]  # every other column mirrored: -inf
        X[:, c] = V / card[:, None]
    c = cols("one_pos_inf")
    X[row(c.size), c] = np.inf
    c = cols("one_neg_inf")
    X[row(c.size), c] = -np.inf
    c = cols("both_infs")
    r = row(c.size)
    X[r, c] = np.inf
    if N > 1:
        X[(r + 1 + rng.integers(0, N - 1, size=c.size)) % N, c] = -np.inf
    c = cols("one_nan")
    X[row(c.size), c] = np.nan
    c = cols("cancellation")  # rows 2k+1 = -rows 2k; an unpaired last row is -0.0
    M = X[:, c]
    M[1::2] = -M[0:N - (N % 2):2]
    if N % 2:
        M[N - 1] = -0.0
    X[:, c] = M
    c = cols("random_bits")  # random finite bit patterns
    b = rng.integers(0, 1 << 63, size=(N, c.size)).astype(np.uint64) | sign((N, c.size))
    b = np.where((b >> np.uint64(52)) & np.uint64(0x7FF) == 0x7FF, b & ~np.uint64(1 << 52), b)
    X[:, c] = b.view(F64)
    return X


def edge_factor_sets(seed, N):
    """(name, a, s or None, divisor): ordinary, identity, weights {0..3} with the
    first and last 0, all-zero over divisor 0; each plain and scored."""
    rng = np.random.default_rng([seed, N, 300])
    card = synth.cardinalities(seed, N)
    sc = np.array([(k + 1) / 11 for k in synth.round_ids(seed, N, 10, 2)], F64)
    zw = rng.integers(0, 4, size=N)
    zw[0] = zw[-1] = 0
    sets = [("ordinary", np.array(card, F64), sc, float(sum(card))),
            ("identity", np.ones(N), np.ones(N), 1.0),
            ("zero_weights", zw.astype(F64), sc, float(int(zw.sum()) or 1)),
            ("zero_total", np.zeros(N), sc, 0.0)]
    for name, a, s, d in sets:
        yield name + "-plain", a, None, d
        yield name + "-scored", a, s.copy(), d


_edge = {}


def _edge_cases(N):
    if N not in _edge:
        X = edge_matrix(2024, N, EDGE_P)
        _edge[N] = (X, [(name, a, s, d, *_numpy_fold(X, a, s, d)) for name, a, s, d in edge_factor_sets(2024, N)])
    return _edge[N]


def test_edge_inputs_hold_what_they_claim():
    """The classes produce the values they are there for (numpy, no GPU work)."""
    X, cases = _edge_cases(9)
    name, a, s, d, running, final = cases[0]
    assert name == "ordinary-plain"
    col = lambda n: final[CLASSES.index(n)::K]
    assert np.isfinite(col("control")).all()
    assert (np.signbit(col("all_neg_zero")) & (col("all_neg_zero") == 0)).all()
    assert np.isinf(col("near_max_in_order")).all() and {1.0, -1.0} == set(np.sign(col("near_max_in_order")))
    assert np.isfinite(col("near_max_reversed")).all()
    rev = _numpy_fold(X[::-1], a[::-1], None, d)[1]
    assert np.isfinite(rev[CLASSES.index("near_max_in_order")::K]).all()
    assert np.isinf(rev[CLASSES.index("near_max_reversed")::K]).all()
    assert np.isinf(col("one_pos_inf")).all() and np.isnan(col("both_infs")).all() and np.isnan(col("one_nan")).all()
    sub = col("subnormal_inputs")
    assert (np.abs(sub[sub != 0]) < np.finfo(F64).tiny).any()
    ident = cases[2][5]
    assert cases[2][0] == "identity-plain"
    c = ident[CLASSES.index("cancellation")::K]
    assert (c == 0).all()
    zt = cases[6][5]
    assert cases[6][0] == "zero_total-plain" and np.isnan(zt[CLASSES.index("control")::K]).all()


@pytest.mark.parametrize("N", EDGE_NS)
def test_fold_f64_edge_values(dev, L, N):
    X, cases = _edge_cases(N)
    for name, a, s, d, running, final in cases:
        _check_fold(Fold(dev, L, X, a, s, d), running, final, (name, N))
        _check_fold(Fold(dev, L, X, a, s, d, acc_off=1), running, final, (name, N, "column kernel"))


@pytest.mark.parametrize("N", EDGE_NS)
def test_rows_f64_edge_values(dev, L, N):
    X, cases = _edge_cases(N)
    for name, a, s, d, running, final in cases:
        _check_rows(dev, L, X, a, s, d, final, (name, N))
