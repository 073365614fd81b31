"""GPU parity of the float16 one-launch step (fa_fedavg_f16_rounds and every
float16 step form of the bench library).

The expected value is numpy's literal float16 fold with Python-number factors,
`reduce(np.add, [x_i * n_i (* s_i)]) / sum(n)`, compared bit for bit with NaN
by position; each round must also hold the bits of fa_fedavg_f16 over the
round's columns.  Weights are Python ints 1..5 and N <= 33, so the binary16
divisor is finite and the quotients are non-trivial (asserted: _meaningful)."""
import ctypes
from functools import reduce

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F16 = np.float16
SENTINEL = 0x5A5A  # an element the kernels never write keeps this pattern
P_EDGE = 20507
OFFS_EDGE = [0, 8200, 12304, P_EDGE]  # per round: a full tile and a last tile of one octet; the last a 3-column tail


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def libs(dev):
    """(_lib, product library, bench library, product rounds state, bench rounds state)"""
    from fedlesscan_amd import _lib
    L, B = _lib.load(), _lib.load_bench()
    r, rb = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.fa_rounds_create(ctypes.byref(r), dev.index), "fa_rounds_create")
    _lib.check(B.fa_bench_rounds_create(ctypes.byref(rb), dev.index), "rounds state", bench=True)
    yield _lib, L, B, r, rb
    torch.cuda.synchronize()
    _lib.check(B.fa_bench_rounds_destroy(rb), "destroy", bench=True)
    _lib.check(L.fa_rounds_destroy(r), "destroy")


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


def _meaningful(exp) -> None:
    """Parity is never satisfied by inf == inf or 0 == 0: the expected output
    is finite everywhere and holds a normal nonzero value."""
    e = np.asarray(exp, F16).ravel()
    assert np.isfinite(e).all()
    assert (np.abs(e.astype(np.float32)) >= 2.0 ** -14).any()


def _numpy_fold(X, w, sc=None):
    assert all(type(v) is int for v in w) and (sc is None or all(type(v) is float for v in sc))
    with np.errstate(all="ignore"):
        out = reduce(np.add, [X[i] * w[i] if sc is None else X[i] * w[i] * sc[i] for i in range(len(w))]) / sum(w)
    assert out.dtype == F16
    return out


def _bits(x) -> int:
    with np.errstate(all="ignore"):
        return int(np.asarray(F16(x)).view(np.uint16))


_cache = {}


def _case(seed, N, P, scored):
    """Rows, weights (1..5), scores and numpy's fold of them, once per shape."""
    key = (seed, N, P, scored)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        X = (rng.random((N, P), dtype=np.float32) * 2 - 1).astype(F16)
        w = [int(v) for v in rng.integers(1, 6, N)]
        sc = [float(v) for v in 1.0 - rng.random(N)] if scored else None  # (0, 1]
        exp = _numpy_fold(X, w, sc)
        _meaningful(exp)
        _cache[key] = (X, w, sc, exp)
    return _cache[key]


class Step:
    """The rows on the device at a pitch of P rounded up to 64, the factors as
    halves in arrays that end on a whole 4-byte word, and the entries."""

    def __init__(self, dev, libs, X, w, sc, offs, out_offs=None, out_len=None):
        self._lib, self.L, self.B, self.r, self.rb = libs
        self.dev = dev
        self.N, self.P = X.shape
        self.ldx = (self.P + 63) // 64 * 64
        Xp = np.zeros((self.N, self.ldx), np.uint16)
        Xp[:, :self.P] = X.view(np.uint16)
        self.X = torch.from_numpy(Xp.view(np.int16)).to(dev)

        def factors(vals):
            h = np.zeros(self.N + 2 + (self.N & 1), np.uint16)
            with np.errstate(all="ignore"):
                h[:self.N] = np.array([F16(v) for v in vals], F16).view(np.uint16)
            return torch.from_numpy(h.view(np.int16)).to(dev)

        self.a = factors(w)
        self.s = None if sc is None else factors(sc)
        self.dbits = _bits(sum(w))
        self.rounds = len(offs) - 1
        self.offs = list(offs)
        self.coffs = (ctypes.c_int64 * len(offs))(*offs)
        self.out_offs = None if out_offs is None else list(out_offs)
        self.coo = None if out_offs is None else (ctypes.c_int64 * self.rounds)(*out_offs)
        self.out = torch.full((out_len or self.ldx,), SENTINEL, dtype=torch.int16, device=dev)
        self.st = torch.cuda.current_stream(dev).cuda_stream

    def sp(self):
        return None if self.s is None else self.s.data_ptr()

    def launch(self, form, x=None, offs=None, rounds=None, stream=None):
        """Product entry (form None) or bench form `form`; returns the status."""
        args = (self.X.data_ptr() if x is None else x, self.N, self.ldx, self.a.data_ptr(), self.sp(), self.dbits,
                self.out.data_ptr(), self.rounds if rounds is None else rounds,
                self.coffs if offs is None else offs, self.coo, self.st if stream is None else stream)
        if form is None:
            return self.L.fa_fedavg_f16_rounds(self.r, *args)
        return self.B.fa_fedavg_f16_rounds_form(self.rb, form, *args)

    def run(self, form):
        self.out.fill_(SENTINEL)
        rc = self.launch(form)
        self._lib.check(rc, "f16 rounds", bench=form is not None)
        torch.cuda.synchronize()
        return self.out.cpu().numpy().view(np.uint16)

    def per_round(self):
        """fa_fedavg_f16 over each round's columns, at the rounds' input columns."""
        ref = torch.full((self.ldx,), SENTINEL, dtype=torch.int16, device=self.dev)
        for k in range(self.rounds):
            c0, c1 = self.offs[k], self.offs[k + 1]
            self._lib.check(self.L.fa_fedavg_f16(self.X.data_ptr() + 2 * c0, self.N, c1 - c0, self.ldx,
                                                 self.a.data_ptr(), self.sp(), self.dbits, ref.data_ptr() + 2 * c0,
                                                 self.st), "fa_fedavg_f16")
        torch.cuda.synchronize()
        return ref.cpu().numpy().view(np.uint16)[:self.P].copy().view(F16)

    def forms(self):
        return [None] + list(range(self.B.fa_num_step_forms_f16()))

    def name(self, form):
        return "fa_fedavg_f16_rounds" if form is None else self.B.fa_step_form_name_f16(form).decode()


def _offsets(P):
    if P == P_EDGE:
        return OFFS_EDGE
    q = P // 4 // 8 * 8
    return [0, q, 3 * q, P]


def _check_all(step, exp, what):
    ref = step.per_round()
    assert same_bits16(ref, exp), (what, "fa_fedavg_f16 per round", _describe(ref, exp))
    assert len(step.forms()) == 3
    for form in step.forms():
        h = step.run(form)
        assert (h[step.P:] == SENTINEL).all(), (what, step.name(form), "wrote past P")
        got = h[:step.P].copy().view(F16)
        assert same_bits16(got, exp), (what, step.name(form), _describe(got, exp))
        assert same_bits16(got, ref), (what, step.name(form), "fa_fedavg_f16", _describe(got, ref))


# ---------------------------------------------------------------------------
# 1. every form: row counts around the 8 rows ahead, tiles, one-octet tiles, tails
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("N,P", [(9, 1027), (33, 4099), (1, P_EDGE), (2, P_EDGE), (10, P_EDGE)])
def test_every_form_matches_numpy(dev, libs, N, P, scored):
    X, w, sc, exp = _case(300 + N, N, P, scored)
    _check_all(Step(dev, libs, X, w, sc, _offsets(P)), exp, (N, P, scored))


def test_out_offsets_permute_the_rounds(dev, libs):
    """The rounds land at permuted 8-aligned output columns; the gaps between
    them keep the sentinel."""
    N, P = 9, P_EDGE
    X, w, sc, exp = _case(300 + N, N, P, True)
    offs = OFFS_EDGE
    wd = [offs[k + 1] - offs[k] for k in range(3)]
    up8 = lambda v: (v + 7) // 8 * 8  # noqa: E731
    oo = [0] * 3
    oo[2] = 16                        # the last round first, behind a 16-column gap
    oo[0] = up8(oo[2] + wd[2]) + 8    # then round 0, a gap of at least 8
    oo[1] = up8(oo[0] + wd[0]) + 24   # then round 1
    total = up8(oo[1] + wd[1]) + 64
    step = Step(dev, libs, X, w, sc, offs, out_offs=oo, out_len=total)
    for form in step.forms():
        h = step.run(form)
        written = np.zeros(total, bool)
        for k in range(3):
            got = h[oo[k]:oo[k] + wd[k]].copy().view(F16)
            assert same_bits16(got, exp[offs[k]:offs[k + 1]]), (step.name(form), k)
            written[oo[k]:oo[k] + wd[k]] = True
        assert (h[~written] == SENTINEL).all(), (step.name(form), "wrote into a gap")


def test_divisor_that_rounds_to_inf(dev, libs):
    """The reference's overflow is kept: sum(n) = 80000 rounds to inf in
    binary16, so finite sums give 0 and overflowed ones NaN."""
    N, P = 2, P_EDGE
    rng = np.random.default_rng(7)
    X = (rng.random((N, P), dtype=np.float32) * 4 - 2).astype(F16)
    w = [40000, 40000]
    exp = _numpy_fold(X, w)
    assert np.isnan(exp).any() and (exp[~np.isnan(exp)] == 0).all() and (~np.isnan(exp)).any()
    step = Step(dev, libs, X, w, None, OFFS_EDGE)
    assert step.dbits == 0x7C00
    for form in step.forms():
        got = step.run(form)[:P].copy().view(F16)
        assert same_bits16(got, exp), (step.name(form), _describe(got, exp))


# ---------------------------------------------------------------------------
# 2. a round wider than one pass of the grid; the waits
# ---------------------------------------------------------------------------
def test_wide_round_and_the_waits(dev, libs):
    """Round 0 is wider than one pass (CU count x 8192 columns), so its
    balanced stride is below the grid size; the product launch three times,
    each round copied on a side stream behind fa_rounds_wait."""
    _lib, L, B, r, rb = libs
    N = 12
    widths = [2_200_064, 300_032, 70_003]
    assert widths[0] > torch.cuda.get_device_properties(dev).multi_processor_count * 8192
    offs = [0, widths[0], widths[0] + widths[1], sum(widths)]
    P = offs[-1]
    X, w, sc, exp = _case(512, N, P, True)
    step = Step(dev, libs, X, w, sc, offs)
    _check_all(step, exp, "wide")
    side = torch.cuda.Stream(device=dev)
    got = torch.empty((step.ldx,), dtype=torch.int16, device=dev)
    for rep in range(3):
        step.out.fill_(SENTINEL)
        got.fill_(-1)
        _lib.check(step.launch(None), "fa_fedavg_f16_rounds")
        for k in range(3):
            _lib.check(L.fa_rounds_wait(r, k, side.cuda_stream), "fa_rounds_wait")
            with torch.cuda.stream(side):
                got[offs[k]:offs[k + 1]].copy_(step.out[offs[k]:offs[k + 1]])
        torch.cuda.synchronize()
        for name, t in (("out", step.out), ("copied behind the waits", got)):
            h = t.cpu().numpy().view(np.uint16)[:P].copy().view(F16)
            assert same_bits16(h, exp), (rep, name, _describe(h, exp))
    assert L.fa_rounds_timeouts(r) == 0 and L.fa_rounds_check(r) == 0


# ---------------------------------------------------------------------------
# 3. edge columns (the classes of tests/test_gpu_f16_fold.py at this shape)
# ---------------------------------------------------------------------------
EDGE_N = 9


def _edge_cases():
    rng = np.random.default_rng(78)
    N, P = EDGE_N, P_EDGE
    base = (rng.random((N, P), dtype=np.float32) * 2 - 1).astype(F16)
    w = [int(v) for v in rng.integers(1, 6, N)]
    ones = [1] * N
    sc = [float(v) for v in 1.0 - rng.random(N)]
    out = {}
    out["all_neg_zero"] = (np.full((N, P), -0.0, F16), w, None)
    x = base.copy()
    x[:5] = F16(-0.0)
    out["leading_neg_zero"] = (x, w, None)
    sub = (rng.integers(1, 0x400, (N, P)).astype(np.uint16) | (rng.integers(0, 2, (N, P)).astype(np.uint16) << 15))
    out["subnormal_inputs"] = (sub.view(F16), [1, 2, 1, 3, 1, 2, 1, 1, 2], None)
    x = (base.astype(np.float32) * 2.0 ** -10).astype(F16)
    out["subnormal_products"] = (x, ones, [float(v) / 16 for v in 1.0 - rng.random(N)])
    x = (base.astype(np.float32) * 4).astype(F16)
    x[3], x[4], x[5] = F16(60000), F16(60000), F16(-60000)
    out["overflow_in_order"] = (x, ones, None)
    x = base.copy()
    x[4, ::2] = F16(np.inf)
    x[4, 1::2] = F16(-np.inf)
    out["one_inf"] = (x, w, None)
    x = base.copy()
    x[3], x[4] = F16(np.inf), F16(-np.inf)
    out["both_infs"] = (x, w, sc)
    x = base.copy()
    x[4, ::3] = F16(np.nan)
    out["one_nan"] = (x, w, None)
    out["zero_weights_first_last"] = (base, [0] + w[1:-1] + [0], None)
    return out


@pytest.fixture(scope="module")
def edge_cases():
    return _edge_cases()


EDGE_NAMES = ["all_neg_zero", "leading_neg_zero", "subnormal_inputs", "subnormal_products", "overflow_in_order",
              "one_inf", "both_infs", "one_nan", "zero_weights_first_last"]


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_columns(dev, libs, edge_cases, name):
    X, w, sc = edge_cases[name]
    final = _numpy_fold(X, w, sc)
    fb = final.view(np.uint16)
    # the class is really there
    if name == "all_neg_zero":
        assert (fb == 0x8000).all()
    elif name == "leading_neg_zero":
        assert np.isfinite(final).all() and (fb != 0x8000).any()
    elif name == "subnormal_inputs":
        assert ((X[0].view(np.uint16) & 0x7C00) == 0).all() and (final != 0).any()
    elif name == "subnormal_products":
        with np.errstate(all="ignore"):
            t0 = (X[0] * 1 * sc[0]).view(np.uint16)
        assert (((t0 & 0x7C00) == 0) & ((t0 & 0x3FF) != 0)).any()
    elif name == "overflow_in_order":
        assert np.isinf(final).all() and np.isfinite(_numpy_fold(X[::-1], w[::-1])).all()
    elif name == "one_inf":
        assert np.isinf(final).all() and (final > 0).any() and (final < 0).any()
    elif name == "both_infs":
        assert np.isnan(final).all()
    elif name == "one_nan":
        assert np.isnan(final[::3]).all() and np.isfinite(np.delete(final, np.s_[::3])).all()
    elif name == "zero_weights_first_last":
        _meaningful(final)
    _check_all(Step(dev, libs, X, w, sc, OFFS_EDGE), final, name)


# ---------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------
def test_argument_errors(dev, libs):
    _lib, L, B, r, rb = libs
    X, w, sc, exp = _case(302, 2, P_EDGE, False)
    step = Step(dev, libs, X, w, None, OFFS_EDGE)
    off_grid = (ctypes.c_int64 * 4)(0, 8204, 12304, P_EDGE)
    nine = (ctypes.c_int64 * 10)(*range(0, 80, 8))
    for form in step.forms():
        assert step.launch(form, x=step.X.data_ptr() + 2) == _lib.FA_ERR_ARG, step.name(form)
        assert step.launch(form, offs=off_grid) == _lib.FA_ERR_ARG, step.name(form)
        assert step.launch(form, offs=nine, rounds=9) == _lib.FA_ERR_ARG, step.name(form)
    assert B.fa_fedavg_f16_rounds_form(rb, 2, step.X.data_ptr(), 2, step.ldx, step.a.data_ptr(), None, step.dbits,
                                       step.out.data_ptr(), 3, step.coffs, None, step.st) == _lib.FA_ERR_ARG
    torch.cuda.synchronize()
    assert (step.out.cpu().numpy().view(np.uint16) == SENTINEL).all()  # nothing was launched
    # a capturing stream is refused, and a normal call afterwards gives the right bits
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="capture"):
        with torch.cuda.graph(g, stream=side):
            _lib.check(step.launch(None, stream=side.cuda_stream), "fa_fedavg_f16_rounds")
    torch.cuda.synchronize()
    assert (step.out.cpu().numpy().view(np.uint16) == SENTINEL).all()
    got = step.run(None)[:step.P].copy().view(F16)
    assert same_bits16(got, exp), _describe(got, exp)
