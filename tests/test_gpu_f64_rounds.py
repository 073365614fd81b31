"""GPU parity of the float64 one-launch step (fa_fedavg_f64_rounds and every
float64 step form of the bench library).

The expected value is numpy's literal float64 left fold,
`reduce(np.add, [x_i * n_i (* s_i)]) / sum(n)`, which test_gpu_f64_fold's
_numpy_fold also checks against oracle_lib.fedavg_f64; results are compared bit
for bit (view(np.uint64)) with NaN by position, and each round must also hold
the bits of fa_fedavg_f64 over the round's columns.

Shapes come from the tile sizes: a wide tile is 4 pairs x 256 lanes x 2 = 2048
columns, a one-pair tile 512.  P_EDGE = 5127 with offsets [0, 2050, 3076, 5127]:
a round of a full wide tile plus one pair, a round of two one-pair tiles plus
one pair, and a round that ends in the P % 2 column."""
import ctypes

import numpy as np
import pytest

import test_gpu_f64_fold as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64 = np.float64
SENTINEL = F.SENTINEL  # an element the kernels never write keeps this pattern
P_EDGE = 5127
OFFS_EDGE = [0, 2050, 3076, P_EDGE]
same_bits, _describe = F.same_bits, F._describe


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


_cache = {}


def _case(seed, N, P, scored):
    """Rows with full mantissas, weights 1..5, scores in (0, 1] and numpy's fold
    of them (checked against the oracle library inside _numpy_fold), once per
    shape."""
    key = (seed, N, P, scored)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        X = (rng.random((N, P)) * 2 - 1) * (1.0 + 1.0 / 3.0)
        a = rng.integers(1, 6, N).astype(F64)
        s = (1.0 - rng.random(N)) if scored else None
        d = float(a.sum())
        _, exp = F._numpy_fold(X, a, s, d)
        assert np.isfinite(exp).all() and exp.any()
        _cache[key] = (X, a, s, d, exp)
    return _cache[key]


class Step:
    """The rows on the device at a pitch of P rounded up to 64, the factors as
    doubles, a sentinel-filled output, and the entries."""

    def __init__(self, dev, libs, X, a, s, d, offs, out_offs=None, out_len=None):
        self._lib, self.L, self.B, self.r, self.rb = libs
        self.dev = dev
        self.N, self.P = X.shape
        self.ldx = (self.P + 63) // 64 * 64
        Xp = np.zeros((self.N, self.ldx), F64)
        Xp[:, :self.P] = X
        self.X = torch.from_numpy(Xp).to(dev)
        self.a = torch.from_numpy(np.ascontiguousarray(a, F64)).to(dev)
        self.s = None if s is None else torch.from_numpy(np.ascontiguousarray(s, F64)).to(dev)
        self.d = float(d)
        self.rounds = len(offs) - 1
        self.offs = list(offs)
        self.coffs = (ctypes.c_int64 * len(offs))(*offs)
        self.coo = None if out_offs is None else (ctypes.c_int64 * self.rounds)(*out_offs)
        self.out = torch.full((out_len or self.ldx,), SENTINEL, dtype=torch.int64, device=dev)
        self.st = torch.cuda.current_stream(dev).cuda_stream
        assert self.X.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def sp(self):
        return None if self.s is None else self.s.data_ptr()

    def launch(self, form, x=None, ldx=None, offs=None, rounds=None, stream=None):
        """Product entry (form None) or bench form `form`; returns the status."""
        args = (self.X.data_ptr() if x is None else x, self.N, self.ldx if ldx is None else ldx, self.a.data_ptr(),
                self.sp(), self.d, self.out.data_ptr(), self.rounds if rounds is None else rounds,
                self.coffs if offs is None else offs, self.coo, self.st if stream is None else stream)
        if form is None:
            return self.L.fa_fedavg_f64_rounds(self.r, *args)
        return self.B.fa_fedavg_f64_rounds_form(self.rb, form, *args)

    def run(self, form):
        self.out.fill_(SENTINEL)
        self._lib.check(self.launch(form), "f64 rounds", bench=form is not None)
        torch.cuda.synchronize()
        return self.out.cpu().numpy().view(np.uint64)

    def per_round(self):
        """fa_fedavg_f64 over each round's columns, at the rounds' input columns."""
        ref = torch.full((self.ldx,), SENTINEL, dtype=torch.int64, device=self.dev)
        for k in range(self.rounds):
            c0, c1 = self.offs[k], self.offs[k + 1]
            self._lib.check(self.L.fa_fedavg_f64(self.X.data_ptr() + 8 * c0, self.N, c1 - c0, self.ldx,
                                                 self.a.data_ptr(), self.sp(), self.d, ref.data_ptr() + 8 * c0,
                                                 self.st), "fa_fedavg_f64")
        torch.cuda.synchronize()
        return ref.cpu().numpy().view(np.uint64)[:self.P].copy().view(F64)

    def forms(self):
        return [None] + list(range(self.B.fa_num_step_forms_f64()))

    def name(self, form):
        return "fa_fedavg_f64_rounds" if form is None else self.B.fa_step_form_name_f64(form).decode()


def _offsets(P):
    if P == P_EDGE:
        return OFFS_EDGE
    q = P // 4 // 2 * 2
    return [0, q, 3 * q, P]


def _check_all(step, exp, what):
    ref = step.per_round()
    assert same_bits(ref, exp), (what, "fa_fedavg_f64 per round", _describe(ref, exp))
    assert len(step.forms()) == 4
    for form in step.forms():
        h = step.run(form)
        assert (h[step.P:] == SENTINEL).all(), (what, step.name(form), "wrote past P")
        got = h[:step.P].copy().view(F64)
        assert same_bits(got, exp), (what, step.name(form), _describe(got, exp))
        assert same_bits(got, ref), (what, step.name(form), "fa_fedavg_f64", _describe(got, ref))


# ---------------------------------------------------------------------------
# 1. every form: row counts around the 8 rows ahead, tiles, one-pair tiles, the odd column
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("N,P", [(9, 1027), (33, 4099), (1, P_EDGE), (2, P_EDGE), (10, P_EDGE)])
def test_every_form_matches_numpy(dev, libs, N, P, scored):
    X, a, s, d, exp = _case(300 + N, N, P, scored)
    _check_all(Step(dev, libs, X, a, s, d, _offsets(P)), exp, (N, P, scored))


def test_out_offsets_permute_the_rounds(dev, libs):
    """The rounds land at permuted 2-aligned output columns; the gaps between
    them keep the sentinel."""
    N, P = 9, P_EDGE
    X, a, s, d, exp = _case(300 + N, N, P, True)
    offs = OFFS_EDGE
    wd = [offs[k + 1] - offs[k] for k in range(3)]
    up2 = lambda v: (v + 1) // 2 * 2  # noqa: E731
    oo = [0] * 3
    oo[2] = 4                         # the last round first, behind a 4-column gap
    oo[0] = up2(oo[2] + wd[2]) + 2    # then round 0, a gap of at least 2
    oo[1] = up2(oo[0] + wd[0]) + 6    # then round 1
    total = up2(oo[1] + wd[1]) + 64
    step = Step(dev, libs, X, a, s, d, offs, out_offs=oo, out_len=total)
    for form in step.forms():
        h = step.run(form)
        written = np.zeros(total, bool)
        for k in range(3):
            got = h[oo[k]:oo[k] + wd[k]].copy().view(F64)
            assert same_bits(got, exp[offs[k]:offs[k + 1]]), (step.name(form), k)
            written[oo[k]:oo[k] + wd[k]] = True
        assert (h[~written] == SENTINEL).all(), (step.name(form), "wrote into a gap")


# ---------------------------------------------------------------------------
# 2. a round wider than one pass of the grid; the waits
# ---------------------------------------------------------------------------
def test_wide_round_and_the_waits(dev, libs):
    """Round 0 is one wide tile wider than a pass of the grid (CU count x 2048
    columns), so its balanced stride is below the grid size; every form, then
    the product launch three times, each round copied on a side stream behind
    fa_rounds_wait."""
    _lib, L, B, r, rb = libs
    N = 3
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    widths = [cus * 2048 + 2048, 30_002, 7_003]
    offs = [0, widths[0], widths[0] + widths[1], sum(widths)]
    P = offs[-1]
    X, a, s, d, exp = _case(512, N, P, True)
    step = Step(dev, libs, X, a, s, d, offs)
    _check_all(step, exp, "wide")
    side = torch.cuda.Stream(device=dev)
    got = torch.empty((step.ldx,), dtype=torch.int64, device=dev)
    for rep in range(3):
        step.out.fill_(SENTINEL)
        got.fill_(-1)
        _lib.check(step.launch(None), "fa_fedavg_f64_rounds")
        for k in range(3):
            _lib.check(L.fa_rounds_wait(r, k, side.cuda_stream), "fa_rounds_wait")
            with torch.cuda.stream(side):
                got[offs[k]:offs[k + 1]].copy_(step.out[offs[k]:offs[k + 1]])
        torch.cuda.synchronize()
        for name, t in (("out", step.out), ("copied behind the waits", got)):
            h = t.cpu().numpy().view(np.uint64)[:P].copy().view(F64)
            assert same_bits(h, exp), (rep, name, _describe(h, exp))
    assert L.fa_rounds_timeouts(r) == 0 and L.fa_rounds_check(r) == 0


# ---------------------------------------------------------------------------
# 3. edge columns in binary64 (the classes and factor sets test_gpu_f64_fold
#    builds for fa_fold_f64, at this file's edge shape): -0.0, subnormal inputs,
#    products and quotients, overflow in client order but not in reverse, infs
#    of either sign, NaN, exact cancellation
# ---------------------------------------------------------------------------
EDGE_N = 9


@pytest.fixture(scope="module")
def edge_cases():
    X = F.edge_matrix(2024, EDGE_N, P_EDGE)
    return X, [(name, a, s, d, F._numpy_fold(X, a, s, d)[1]) for name, a, s, d in F.edge_factor_sets(2024, EDGE_N)]


EDGE_SETS = [n + k for n in ("ordinary", "identity", "zero_weights", "zero_total") for k in ("-plain", "-scored")]


def test_edge_inputs_hold_what_they_claim(edge_cases):
    """The classes are really there at this shape (numpy only)."""
    X, cases = edge_cases
    assert [c[0] for c in cases] == EDGE_SETS
    name, a, s, d, final = cases[0]
    col = lambda n: final[F.CLASSES.index(n)::F.K]  # noqa: E731
    assert np.isfinite(col("control")).all()
    assert (np.signbit(col("all_neg_zero")) & (col("all_neg_zero") == 0)).all()
    assert np.isinf(col("near_max_in_order")).all() and {1.0, -1.0} == set(np.sign(col("near_max_in_order")))
    rev = F._numpy_fold(X[::-1], a[::-1], None, d)[1]
    assert np.isfinite(rev[F.CLASSES.index("near_max_in_order")::F.K]).all()
    assert np.isinf(col("one_pos_inf")).all() and np.isinf(col("one_neg_inf")).all()
    assert np.isnan(col("both_infs")).all() and np.isnan(col("one_nan")).all()
    sub = col("subnormal_inputs")
    assert (np.abs(sub[sub != 0]) < np.finfo(F64).tiny).any()  # subnormal quotients
    with np.errstate(all="ignore"):
        t = X[:, F.CLASSES.index("subnormal_inputs")::F.K] * a[:, None]
    assert ((t != 0) & (np.abs(t) < np.finfo(F64).tiny)).any()  # subnormal products
    assert (cases[2][4][F.CLASSES.index("cancellation")::F.K] == 0).all()


@pytest.mark.parametrize("which", range(len(EDGE_SETS)), ids=EDGE_SETS)
def test_edge_columns(dev, libs, edge_cases, which):
    X, cases = edge_cases
    name, a, s, d, final = cases[which]
    _check_all(Step(dev, libs, X, a, s, d, OFFS_EDGE), final, name)


# ---------------------------------------------------------------------------
# 4. argument errors
# ---------------------------------------------------------------------------
def test_argument_errors(dev, libs):
    _lib, L, B, r, rb = libs
    X, a, s, d, exp = _case(302, 2, P_EDGE, False)
    step = Step(dev, libs, X, a, None, d, OFFS_EDGE)
    off_grid = (ctypes.c_int64 * 4)(0, 2051, 3076, P_EDGE)
    nine = (ctypes.c_int64 * 10)(*range(0, 20, 2))
    for form in step.forms():
        assert step.launch(form, ldx=step.ldx + 1) == _lib.FA_ERR_ARG, step.name(form)             # an odd ldx
        assert step.launch(form, x=step.X.data_ptr() + 8) == _lib.FA_ERR_ARG, step.name(form)      # X off 16 B
        assert step.launch(form, offs=off_grid) == _lib.FA_ERR_ARG, step.name(form)
        assert step.launch(form, offs=nine, rounds=9) == _lib.FA_ERR_ARG, step.name(form)
    for bad in (-1, B.fa_num_step_forms_f64()):  # a form index out of range
        assert step.launch(bad) == _lib.FA_ERR_ARG
    torch.cuda.synchronize()
    assert (step.out.cpu().numpy().view(np.uint64) == SENTINEL).all()  # nothing was launched
    # a capturing stream is refused, and a normal call afterwards gives the right bits
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="capture"):
        with torch.cuda.graph(g, stream=side):
            _lib.check(step.launch(None, stream=side.cuda_stream), "fa_fedavg_f64_rounds")
    torch.cuda.synchronize()
    assert (step.out.cpu().numpy().view(np.uint64) == SENTINEL).all()
    got = step.run(None)[:step.P].copy().view(F64)
    assert same_bits(got, exp), _describe(got, exp)
