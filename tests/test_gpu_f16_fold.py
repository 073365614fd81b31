"""GPU parity of the chunked binary16 fold (fa_fold_f16, raw ABI).

Folding the rows in any cuts, with the accumulator carried between the calls
as halves, must give the bits of numpy's own literal float16 left fold
`reduce(np.add, [x_i * n_i (* s_i)]) / sum(n)` with Python-number factors, and
of one fa_fedavg_f16 call over all rows.  Compared bit for bit, NaN by position
(NaN sign and payload are free, as for fa_fedavg_f16).

Ordinary inputs: rows uniform in [-1, 1), weights Python ints 1..40, scores in
(0, 1], N <= 33, so |acc| <= 1320 and the total <= 1320: every expected value is
finite, which the tests assert; nothing is masked."""
from functools import reduce

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F16 = np.float16
SENTINEL = 0x5A5A  # an element the kernel never writes keeps this pattern
# the policy folds 2 octets per lane (256 lanes): a full tile is 4096 columns;
# 4899 = one full tile, a partial tile of 100 octets, a 3-column tail
P_TILES = 2 * 256 * 8 + 100 * 8 + 3
# 4107 = one full tile, a last tile with exactly one octet, a 3-column tail
PS = [1, 7, 8, 9, 2048, 2059, 2 * 256 * 8 + 8 + 3, P_TILES]
NS = [1, 2, 6, 9, 33]  # 6: the first row, one group of the 4 rows ahead, a leftover row


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from fedlesscan_amd import _lib
    return _lib.load()


def same_bits16(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F16 or b.dtype != F16 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~na]))


def _describe(got, exp):
    na, nb = np.isnan(got), np.isnan(exp)
    bad = np.flatnonzero((na != nb) | ((got.view(np.uint16) != exp.view(np.uint16)) & ~(na & nb)))
    i = int(bad[0]) if bad.size else -1
    return f"{bad.size} differ; first col {i}: got {got.view(np.uint16)[i]:#06x} exp {exp.view(np.uint16)[i]:#06x}"


def _bits(x) -> int:
    with np.errstate(all="ignore"):
        return int(np.asarray(F16(x)).view(np.uint16))


# ---------------------------------------------------------------------------
# numpy's literal fold, and its running sums
# ---------------------------------------------------------------------------
def _numpy_fold(X, w, sc=None):
    """(running, final): running[i] = the float16 left fold of the terms of rows
    0..i, final = running[-1] / sum(w); weights and scores are Python numbers,
    so numpy keeps every operation in float16."""
    assert all(type(v) is int for v in w) and (sc is None or all(type(v) is float for v in sc))
    with np.errstate(all="ignore"):
        terms = [X[i] * w[i] if sc is None else X[i] * w[i] * sc[i] for i in range(len(w))]
        running = [terms[0]]
        for t in terms[1:]:
            running.append(np.add(running[-1], t))
        final = running[-1] / sum(w)
        assert final.dtype == F16 and all(r.dtype == F16 for r in running)
        lit = reduce(np.add, terms) / sum(w)  # the literal form itself
        assert same_bits16(lit, final)
    return running, final


_cache = {}


def _case(seed, N, P, scored):
    """Rows, weights, scores and numpy's fold of them, computed once per shape."""
    key = (seed, N, P, scored)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        X = (rng.random((N, P), dtype=np.float32) * 2 - 1).astype(F16)
        w = [int(v) for v in rng.integers(1, 41, N)]
        sc = [float(v) for v in 1.0 - rng.random(N)] if scored else None  # (0, 1]
        running, final = _numpy_fold(X, w, sc)
        assert np.isfinite(final).all() and all(np.isfinite(r).all() for r in running)
        _cache[key] = (X, w, sc, running, final)
    return _cache[key]


# ---------------------------------------------------------------------------
# the raw entry
# ---------------------------------------------------------------------------
class Fold:
    """The rows on the device at pitch ldx (16-B aligned base unless x_off),
    the factors as halves in arrays padded to a whole 4-byte word, and two
    accumulator buffers (16-B aligned, or 2 bytes past that with acc_off)."""

    def __init__(self, dev, L, X, w, sc, ldx=None, acc_off=0):
        self.dev, self.L = dev, L
        self.N, self.P = X.shape
        self.ldx = ldx or (self.P + 63) // 64 * 64
        Xp = np.zeros((self.N, self.ldx), np.uint16)
        Xp[:, :self.P] = X.view(np.uint16)
        self.X = torch.from_numpy(Xp.view(np.int16)).to(dev)

        def factors(vals):
            h = np.zeros(self.N + 2 + (self.N & 1), np.uint16)  # ends on a 4-byte word inside the allocation
            with np.errstate(all="ignore"):
                h[:self.N] = np.array([F16(v) for v in vals], F16).view(np.uint16)
            return torch.from_numpy(h.view(np.int16)).to(dev)

        self.a = factors(w)
        self.s = None if sc is None else factors(sc)
        self.dbits = _bits(sum(w))
        self.off = acc_off
        self.bufs = [torch.full((self.P + 16,), SENTINEL, dtype=torch.int16, device=dev) for _ in range(2)]
        self.st = torch.cuda.current_stream(dev).cuda_stream

    def ptr(self, k):
        return self.bufs[k].data_ptr() + 2 * self.off

    def read(self, k):
        h = self.bufs[k].cpu().numpy().view(np.uint16)
        assert (h[:self.off] == SENTINEL).all() and (h[self.off + self.P:] == SENTINEL).all(), "wrote out of range"
        return h[self.off:self.off + self.P].copy().view(F16)

    def call(self, i0, n, acc_in, fin, out, dbits=None):
        """Rows [i0, i0 + n) into buffer `out`, continuing from buffer acc_in (None: a fresh fold)."""
        rc = self.L.fa_fold_f16(self.X.data_ptr() + 2 * i0 * self.ldx if n else None, n, self.P, self.ldx,
                                self.a.data_ptr() + 2 * i0 if n else None,
                                None if (self.s is None or not n) else self.s.data_ptr() + 2 * i0,
                                None if acc_in is None else self.ptr(acc_in),
                                self.dbits if dbits is None else dbits, int(fin), self.ptr(out), self.st)
        from fedlesscan_amd import _lib
        _lib.check(rc, "fa_fold_f16")

    def one_shot(self):
        out = torch.full((self.P,), SENTINEL, dtype=torch.int16, device=self.dev)
        rc = self.L.fa_fedavg_f16(self.X.data_ptr(), self.N, self.P, self.ldx, self.a.data_ptr(),
                                  None if self.s is None else self.s.data_ptr(), self.dbits, out.data_ptr(), self.st)
        from fedlesscan_amd import _lib
        _lib.check(rc, "fa_fedavg_f16")
        return out.cpu().numpy().view(F16)


def _cuts(N):
    """name -> (row counts per call, a final N == 0 divide-only call?)"""
    ramp, left, k = [], N, 1
    while left > 0 and k <= 8:
        ramp.append(min(k, left))
        left -= ramp[-1]
        k *= 2
    if left:
        ramp.append(left)
    return {"all": ([N], False), "rows": ([1] * N, False), "ramp": (ramp, False), "divide_only": (ramp, True)}


def _run_cuts(f, running, final, what, cuts=None):
    """Every cut, in place and through a separate buffer; the unfinalised
    partial after each call against numpy's running sum."""
    for name, (counts, tail) in (cuts or _cuts(f.N)).items():
        for in_place in (True, False):
            i0, cur = 0, None
            for k, n in enumerate(counts):
                last = k == len(counts) - 1
                fin = last and not tail
                out = 0 if (in_place or cur is None) else 1 - cur
                f.call(i0, n, cur, fin, out)
                i0 += n
                cur = out
                if not fin:
                    got = f.read(cur)
                    assert same_bits16(got, running[i0 - 1]), (what, name, in_place, "partial after row", i0 - 1,
                                                               _describe(got, running[i0 - 1]))
            if tail:
                out = cur if in_place else 1 - cur
                f.call(i0, 0, cur, True, out)
                cur = out
            got = f.read(cur)
            assert same_bits16(got, final), (what, name, in_place, _describe(got, final))


# ---------------------------------------------------------------------------
# 1. ordinary inputs: every width, row count and cut
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("P", PS)
def test_cuts_match_numpy_and_one_call(dev, L, P, N, scored):
    X, w, sc, running, final = _case(100 + N, N, P, scored)
    f = Fold(dev, L, X, w, sc)
    one = f.one_shot()
    assert same_bits16(one, final), ("fa_fedavg_f16", _describe(one, final))
    _run_cuts(f, running, final, (P, N, scored))


# ---------------------------------------------------------------------------
# 2. the one-column-per-lane path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("how", ["pitch", "acc_offset"])
def test_scalar_path(dev, L, how, scored):
    """A row pitch with ldx % 8 != 0, and the accumulator and output 2 bytes
    off 16-B alignment (rows aligned, pitch a multiple of 8)."""
    N, P = 9, 2059
    X, w, sc, running, final = _case(100 + N, N, P, scored)
    f = Fold(dev, L, X, w, sc, ldx=P + 3) if how == "pitch" else Fold(dev, L, X, w, sc, acc_off=1)
    assert (f.ldx % 8 != 0) if how == "pitch" else (f.ldx % 8 == 0 and f.ptr(0) % 16 == 2 and f.X.data_ptr() % 16 == 0)
    _run_cuts(f, running, final, (how, scored))


# ---------------------------------------------------------------------------
# 3. edge columns: each class lies across the chunk boundary after row 3
# ---------------------------------------------------------------------------
EDGE_N, EDGE_P = 9, P_TILES
EDGE_CUTS = {"4+5": ([4, 5], False), "rows": ([1] * EDGE_N, False), "ramp": ([1, 2, 4, 2], False),
             "divide_only": ([4, 5], True)}


def _edge_cases():
    rng = np.random.default_rng(77)
    N, P = EDGE_N, EDGE_P
    base = (rng.random((N, P), dtype=np.float32) * 2 - 1).astype(F16)
    w = [int(v) for v in rng.integers(1, 41, N)]
    ones = [1] * N
    sc = [float(v) for v in 1.0 - rng.random(N)]
    out = {}

    def full(v):
        return np.full((N, P), v, F16)

    out["all_neg_zero"] = (full(-0.0), w, None)
    x = base.copy()
    x[:5] = F16(-0.0)  # -0.0 through the boundary, then ordinary rows
    out["leading_neg_zero"] = (x, w, None)
    x = full(-0.0)
    x[5] = F16(0.0)  # the first +0.0 arrives in the second chunk
    out["neg_zero_then_pos_zero"] = (x, w, None)
    # subnormal inputs (every subnormal pattern, both signs) under small weights
    sub = (rng.integers(1, 0x400, (N, P)).astype(np.uint16) | (rng.integers(0, 2, (N, P)).astype(np.uint16) << 15))
    out["subnormal_inputs"] = (sub.view(F16), [1, 2, 1, 3, 1, 2, 1, 1, 2], None)
    # products that fall into the subnormal range: |x| < 2^-10 times a score <= 1/16
    x = (base.astype(np.float32) * 2.0 ** -10).astype(F16)
    out["subnormal_products"] = (x, ones, [float(v) / 16 for v in 1.0 - rng.random(N)])
    # terms that overflow in client order (60000 + 60000 = inf) but not in reverse
    x = (base.astype(np.float32) * 4).astype(F16)
    x[3], x[4], x[5] = F16(60000), F16(60000), F16(-60000)
    out["overflow_in_order"] = (x, ones, None)
    x = base.copy()
    x[4, ::2] = F16(np.inf)
    x[4, 1::2] = F16(-np.inf)
    out["one_inf"] = (x, w, None)
    x = base.copy()
    x[3], x[4] = F16(np.inf), F16(-np.inf)  # inf in the first chunk, -inf in the second: NaN
    out["both_infs"] = (x, w, sc)
    x = base.copy()
    x[4, ::3] = F16(np.nan)
    out["one_nan"] = (x, w, None)
    x = full(-0.0)
    x[3] = base[3]
    x[4] = -base[3]  # v in the first chunk, -v in the second: +0.0, and it stays +0.0 under the -0.0 rows after it
    out["exact_cancellation"] = (x, ones, None)
    out["random_bits"] = (rng.integers(0, 1 << 16, (N, P)).astype(np.uint16).view(F16), w, sc)
    out["zero_weights_first_last"] = (base, [0] + w[1:-1] + [0], None)
    x = base.copy()
    x[4, ::5] = F16(np.inf)
    out["divisor_zero"] = (x, [0] * N, None)
    return out


@pytest.fixture(scope="module")
def edge_cases():
    return _edge_cases()


EDGE_NAMES = ["all_neg_zero", "leading_neg_zero", "neg_zero_then_pos_zero", "subnormal_inputs", "subnormal_products",
              "overflow_in_order", "one_inf", "both_infs", "one_nan", "exact_cancellation", "random_bits",
              "zero_weights_first_last", "divisor_zero"]


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_columns(dev, L, edge_cases, name):
    X, w, sc = edge_cases[name]
    running, final = _numpy_fold(X, w, sc)
    fb = final.view(np.uint16)
    # the class is really there
    if name == "all_neg_zero":
        assert (fb == 0x8000).all()
    elif name in ("neg_zero_then_pos_zero", "exact_cancellation"):
        assert (fb == 0x0000).all() and (running[3].view(np.uint16) != 0).any()
    elif name == "subnormal_inputs":
        assert ((running[0].view(np.uint16) & 0x7C00) == 0).any()
    elif name == "subnormal_products":
        t0 = (X[0] * 1 * sc[0]).view(np.uint16)
        assert (((t0 & 0x7C00) == 0) & ((t0 & 0x3FF) != 0)).any()
    elif name == "overflow_in_order":
        assert np.isinf(final).all() and np.isfinite(_numpy_fold(X[::-1], w[::-1])[1]).all()
        assert np.isfinite(running[3]).all() and np.isinf(running[4]).all()  # overflows in the second chunk
    elif name == "one_inf":
        assert np.isinf(final).all() and (final > 0).any() and (final < 0).any()
    elif name == "both_infs":
        assert np.isnan(final).all() and np.isinf(running[3]).all()
    elif name == "one_nan":
        assert np.isnan(final[::3]).all() and np.isfinite(np.delete(final, np.s_[::3])).all()
    elif name == "random_bits":
        assert np.isnan(final).any() and np.isfinite(final).any()
    elif name == "zero_weights_first_last":
        assert np.isfinite(final).all() and (running[0] == 0).all()
    elif name == "divisor_zero":
        assert np.isnan(final).all()  # 0 / 0, and 0 * inf on the way
    f = Fold(dev, L, X, w, sc)
    assert same_bits16(f.one_shot(), final), name
    _run_cuts(f, running, final, name, EDGE_CUTS)
    # the scalar kernel gives the same bits
    g = Fold(dev, L, X[:, :523], w, sc, ldx=523 + 3)
    _run_cuts(g, [r[:523] for r in running], final[:523], (name, "scalar"), {"4+5": EDGE_CUTS["4+5"]})


# ---------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------
def test_argument_errors(dev, L):
    from fedlesscan_amd import _lib
    X, w, sc, running, final = _case(102, 2, 2059, False)
    f = Fold(dev, L, X, w, None)
    x, a, o, st, d = f.X.data_ptr(), f.a.data_ptr(), f.ptr(0), f.st, f.dbits
    assert L.fa_fold_f16(None, 2, f.P, f.ldx, a, None, None, d, 1, o, st) == _lib.FA_ERR_ARG
    assert L.fa_fold_f16(x, 2, f.P, f.ldx, None, None, None, d, 1, o, st) == _lib.FA_ERR_ARG
    assert L.fa_fold_f16(x, 2, f.P, f.ldx, a, None, None, d, 1, None, st) == _lib.FA_ERR_ARG
    assert L.fa_fold_f16(None, 0, f.P, f.ldx, None, None, o, d, 1, None, st) == _lib.FA_ERR_ARG
    assert L.fa_fold_f16(x, 0, f.P, f.ldx, a, None, None, d, 1, o, st) == _lib.FA_ERR_NO_CLIENTS  # N == 0, no acc_in
    assert L.fa_fold_f16(x, 2, f.P, f.P - 1, a, None, None, d, 1, o, st) == _lib.FA_ERR_SHAPE
    torch.cuda.synchronize()
    assert (f.bufs[0].cpu().numpy().view(np.uint16) == SENTINEL).all()  # nothing was launched
    # a capturing stream is refused, and the device is fine afterwards
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="capture"):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.fa_fold_f16(x, 2, f.P, f.ldx, a, None, None, d, 1, o, side.cuda_stream), "fa_fold_f16")
    torch.cuda.synchronize()
    f.call(0, 2, None, True, 0)
    assert same_bits16(f.read(0), final)
