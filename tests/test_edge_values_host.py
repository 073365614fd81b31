"""Edge-value recipes (tests/edge_values.py) on the host: the C oracle agrees
bit for bit with the literal numpy left fold on them, the recipes contain the
values they promise, and each of eight deliberately wrong folds / roundings is
told apart from the reference by them -- three of which plain synthetic data
cannot tell apart.  These results are what lets tests/test_gpu_edge_values.py
answer to the fast C oracle."""
import numpy as np
import pytest

import edge_values as E
import golden_cases as G
from fedlesscan_amd import synth
from oracle import oracle_lib as OL

SEED = 2024
NS = [1, 2, 9, 33, 70, 300]  # 300: the GPU file's client count for the 8-wave forms
PS = [7, 1027, 4099]


def _ordinary(seed, N, dtype=np.float32):
    return next(iter(E.factor_sets(seed, N, dtype)))


# ---------------------------------------------------------------------------
# the oracle against the literal fold
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("N", NS)
def test_oracle_equals_left_fold(N, P):
    X32, Xb, X64 = E.matrix_f32(SEED, N, P), E.matrix_bf16(SEED, N, P), E.matrix_f64(SEED, N, P)
    seen = set()
    for name, a, s, d in E.factor_sets(SEED, N):
        what = (E.set_id(name, s), N, P)
        seen.add(what[0])
        assert G.same_bits(OL.fedavg_f32(X32, a, d, s=s), E.left_fold(X32, a, d, s)), what
        ef, eb = OL.fedavg_bf16(Xb, a, d, s=s)
        assert G.same_bits(ef, E.left_fold(Xb, a, d, s)), what
        # the oracle's bf16 rounding against an implementation that does not share its expression
        assert E.bf16_matches_independent(eb, ef), what
        assert np.array_equal(E.is_nan_bf16(eb), np.isnan(ef)), what
    for name, a, s, d in E.factor_sets(SEED, N, np.float64):
        assert a.dtype == np.float64
        assert G.same_bits(OL.fedavg_f64(X64, a, d, s=s), E.left_fold(X64, a, d, s)), (E.set_id(name, s), N, P)
    assert len(seen) == 2 * len(E.FACTOR_SETS)


def test_recipes_are_deterministic():
    for fn in (E.matrix_f32, E.matrix_bf16, E.matrix_f64):
        a, b = fn(SEED, 9, 1027), fn(SEED, 9, 1027)
        assert a.tobytes() == b.tobytes()
        assert fn(SEED + 1, 9, 1027).tobytes() != a.tobytes()
    f1 = [(n, a.tobytes(), None if s is None else s.tobytes(), float(d)) for n, a, s, d in E.factor_sets(SEED, 9)]
    f2 = [(n, a.tobytes(), None if s is None else s.tobytes(), float(d)) for n, a, s, d in E.factor_sets(SEED, 9)]
    assert f1 == f2
    # class 0 is the untouched control
    c = E.class_columns(1027, "control")
    assert np.array_equal(E.matrix_f32(SEED, 9, 1027)[:, c], synth.clients_f32(SEED, 9, 0, 1027)[:, c])


def test_same_bf16_bits():
    a = np.array([0x7FC0, 0x0000, 0x3F80, 0xFFC1], np.uint16)
    assert E.same_bf16_bits(a, np.array([0xFFC0, 0x0000, 0x3F80, 0x7F81], np.uint16))
    assert not E.same_bf16_bits(a, np.array([0x7FC0, 0x8000, 0x3F80, 0xFFC1], np.uint16))  # -0 is not +0
    assert not E.same_bf16_bits(a, np.array([0x7F80, 0x0000, 0x3F80, 0xFFC1], np.uint16))  # inf is not NaN


# ---------------------------------------------------------------------------
# the inputs contain what they promise (conditions, not measurements)
# ---------------------------------------------------------------------------
def _reverse_fold(X, a, d, s):
    return E.left_fold(X[::-1], a[::-1], d, None if s is None else s[::-1])


@pytest.mark.parametrize("P", [p for p in PS if p >= 4 * E.K])
@pytest.mark.parametrize("N", NS)
def test_expected_outputs_hold_every_value_kind(N, P):
    """Over the ordinary factors the expected fp32 output has at most a third
    of its columns NaN (a NaN column is compared by position only) and holds
    every kind of value the recipes are there for."""
    X = E.matrix_f32(SEED, N, P)
    name, a, s, d = _ordinary(SEED, N)
    assert name == "ordinary" and s is None
    e = E.left_fold(X, a, d)
    bits = e.view(np.uint32)
    nan = np.isnan(e)
    assert nan.sum() * 3 <= P, nan.mean()
    assert (bits == 0x80000000).any(), "-0.0"
    assert (bits == 0).any(), "+0.0"
    assert ((e != 0) & (np.abs(e) < np.finfo(np.float32).tiny)).any(), "a nonzero subnormal"
    assert (e == np.inf).any() and (e == -np.inf).any() and nan.any()
    assert (np.isfinite(e) & (np.abs(e) > 1e30)).any(), "a finite value above 1e30"
    if N >= 3:  # two terms commute: no order of one or two clients changes a sum
        c = E.class_columns(P, "near_max")
        fwd, rev = e[c], _reverse_fold(X[:, c], a, d, None)
        assert (np.isinf(fwd) & np.isfinite(rev)).any(), "inf in client order, finite in reverse"
        assert (np.isfinite(fwd) & np.isinf(rev)).any(), "finite in client order, inf in reverse"
    # the same kinds in double
    X64 = E.matrix_f64(SEED, N, P)
    _, a64, _, d64 = _ordinary(SEED, N, np.float64)
    e64 = E.left_fold(X64, a64, d64)
    assert np.isnan(e64).sum() * 3 <= P
    assert (e64.view(np.uint64) == 1 << 63).any() and (e64.view(np.uint64) == 0).any()
    assert ((e64 != 0) & (np.abs(e64) < np.finfo(np.float64).tiny)).any()
    assert (e64 == np.inf).any() and (e64 == -np.inf).any() and np.isnan(e64).any()
    # a subnormal, nonzero quotient under the huge divisor, in a visible share of a class
    for nm, ah, sh, dh in E.factor_sets(SEED, N):
        if nm == "huge_divisor":
            q = E.left_fold(X, ah, dh, sh)[E.class_columns(P, "smallest_normals")]
            sub = (q != 0) & (np.abs(q) < np.finfo(np.float32).tiny)
            assert sub.mean() >= 0.25, (sub.mean(), sh is not None)


@pytest.mark.parametrize("P", [p for p in PS if p >= 4 * E.K])
@pytest.mark.parametrize("N", NS)
def test_bf16_outputs_hold_every_rounding_case(N, P):
    """The bf16 output over the identity factors: both tie directions, a finite
    fp32 value that rounds to bf16 inf, a bf16 subnormal and -0."""
    Xb = E.matrix_bf16(SEED, N, P)
    ones = np.ones(N, np.float32)
    ef, eb = OL.fedavg_bf16(Xb, ones, np.float32(1))
    u = ef.view(np.uint32)
    ok = ~np.isnan(ef)
    mag = eb & 0x7FFF
    assert ((mag > 0) & (mag < 0x0080)).any(), "a bf16 subnormal"
    assert (eb == 0x8000).any(), "-0"
    if N >= 2:  # one client under the identity factors is a bf16 value already: nothing is rounded
        tie = ok & ((u & 0xFFFF) == 0x8000)
        assert (tie & (eb == (u >> 16) + 1)).any(), "a tie rounded up"
        assert (tie & (eb == (u >> 16))).any(), "a tie rounded down"
        assert (np.isfinite(ef) & (mag == 0x7F80)).any(), "a finite fp32 value that rounds to bf16 inf"
    if N >= 3:
        low = u[ok] & 0xFFFF
        assert (low == 0x7FFF).any() and (low == 0x8001).any(), "the ties' neighbours"
    # the float32 matrix carries the same cases as values (its bf16_tie class)
    t = E.matrix_f32(SEED, N, P)[:, E.class_columns(P, "bf16_tie")]
    low = t.view(np.uint32) & 0xFFFF
    for pat in (0x8000, 0x7FFF, 0x8001):
        assert (low == pat).any()
    r = E.bf16_rne_independent(t)
    assert (np.isfinite(t) & ((r & 0x7FFF) == 0x7F80)).any()
    assert np.array_equal(synth.f32_to_bf16_bits(t), r)  # the package's host rounding, same independent check


# ---------------------------------------------------------------------------
# sensitivity: wrong folds the recipes must tell from the reference
# ---------------------------------------------------------------------------
def _terms(X, a, s):
    for i in range(X.shape[0]):
        t = np.multiply(X[i], a[i])
        yield t if s is None else np.multiply(t, s[i])


def fold_zero_init(X, a, d, s):
    acc = np.zeros(X.shape[1], X.dtype)
    for t in _terms(X, a, s):
        acc = acc + t
    return acc / d


def fold_skip_zero_weights(X, a, d, s):
    acc = None
    for i, t in enumerate(_terms(X, a, s)):
        if a[i] == 0:
            continue
        acc = t if acc is None else acc + t
    if acc is None:
        acc = np.zeros(X.shape[1], X.dtype)
    return acc / d


def fold_pairwise(X, a, d, s):
    ts = list(_terms(X, a, s))
    while len(ts) > 1:
        ts = [ts[k] + ts[k + 1] if k + 1 < len(ts) else ts[k] for k in range(0, len(ts), 2)]
    return ts[0] / d


def fold_fma(X, a, d, s):
    """acc = fma(x, a, acc) (scored: fma(fl(x * a), s, acc)), the product kept exact in float64."""
    acc = None
    for i in range(X.shape[0]):
        if s is None:
            u, v = X[i].astype(np.float64), np.float64(a[i])
        else:
            u, v = np.multiply(X[i], a[i]).astype(np.float64), np.float64(s[i])
        acc = (u * v).astype(np.float32) if acc is None else (u * v + acc.astype(np.float64)).astype(np.float32)
    return acc / d


def _ftz(x):
    x = np.asarray(x, np.float32)
    return np.where(np.abs(x) < np.finfo(np.float32).tiny, np.copysign(np.float32(0), x), x).astype(np.float32)


def fold_flush_to_zero(X, a, d, s):
    acc = None
    for i in range(X.shape[0]):
        t = _ftz(_ftz(X[i]) * _ftz(a[i]))
        if s is not None:
            t = _ftz(t * _ftz(s[i]))
        acc = t if acc is None else _ftz(acc + t)
    return _ftz(acc / _ftz(d))


def fold_reciprocal(X, a, d, s):
    acc = None
    for t in _terms(X, a, s):
        acc = t if acc is None else acc + t
    return acc * (np.float32(1) / np.float32(d))


MUTANTS = {"zero_init": fold_zero_init, "skip_zero_weights": fold_skip_zero_weights, "pairwise": fold_pairwise,
           "fma": fold_fma, "flush_to_zero": fold_flush_to_zero, "reciprocal": fold_reciprocal}


def _differences_in_non_nan_columns(got, ref) -> int:
    """Columns where the reference is not NaN and got is another value (or NaN).
    A column that is NaN in the reference is compared by position only, so it
    cannot show a wrong value; it is not counted."""
    nr = np.isnan(ref)
    return int((~nr & (np.isnan(got) | (got.view(np.uint32) != ref.view(np.uint32)))).sum())


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_wrong_folds_are_detected(mutant):
    N, P = 9, 1027
    X = E.matrix_f32(SEED, N, P)
    found = {}
    with np.errstate(all="ignore"):
        for name, a, s, d in E.factor_sets(SEED, N):
            ref = E.left_fold(X, a, d, s)
            got = MUTANTS[mutant](X, a, d, s).astype(np.float32)
            found[E.set_id(name, s)] = _differences_in_non_nan_columns(got, ref)
            assert found[E.set_id(name, s)] == 0 or not G.same_bits(got, ref)  # what the GPU tests assert sees it
    assert max(found.values()) >= 1, found


def bf16_truncate(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_round_half_up(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) >> 16).astype(np.uint16)


@pytest.mark.parametrize("rounding", [bf16_truncate, bf16_round_half_up])
def test_wrong_bf16_roundings_are_detected(rounding):
    N, P = 9, 1027
    Xb = E.matrix_bf16(SEED, N, P)
    found = {}
    for name, a, s, d in E.factor_sets(SEED, N):
        ef, eb = OL.fedavg_bf16(Xb, a, d, s=s)
        ok = ~np.isnan(ef)
        found[E.set_id(name, s)] = int((rounding(ef)[ok] != eb[ok]).sum())
    assert found["identity-plain"] >= 1, found  # the tie class alone must do it
    assert max(found.values()) >= 1


@pytest.mark.parametrize("mutant", ["zero_init", "skip_zero_weights", "flush_to_zero"])
def test_synthetic_data_cannot_detect(mutant):
    """The gap the edge values close: plain synthetic data under the ordinary
    factors has no -0.0, no subnormal and no zero weight, so these three wrong
    folds give the reference's bits on it."""
    N, P = 9, 1027
    X = synth.clients_f32(SEED, N, 0, P)
    for name, a, s, d in E.factor_sets(SEED, N):
        if name == "ordinary":
            with np.errstate(all="ignore"):
                got = MUTANTS[mutant](X, a, d, s).astype(np.float32)
            assert G.same_bits(got, E.left_fold(X, a, d, s)), (mutant, s is not None)
