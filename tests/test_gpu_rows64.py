"""GPU: separately allocated CUDA float64 rows fold through the device row
table (fa_fedavg_f64_ptrs), with no stacked copy.

engine.fold_rows, engine.RowSet, engine.aggregate_layers and both strategy
classes on CUDA float64 layers: numpy's literal float64 left fold, bit for bit
(view(np.uint64)); the fold is counted under engine.stats["rows64_folds"] and
no layer group is stacked.  Inputs: synth.clients_f32(...).astype(float64) *
(1 + 1/3) with synth.cardinalities weights (tests/test_f64_host.py)."""
import numpy as np
import pytest

from fedlesscan_amd import synth
from oracle import fedavg_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64 = np.float64
R = 10
LAYERS = [2 * 512 + 256 + 1, 5]  # two full pair tiles, a partial one and an odd column; a tiny layer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F64 or b.dtype != F64 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~na]))


def _rows(seed, n, p):
    return synth.clients_f32(seed, n, 0, p).astype(F64) * (1.0 + 1.0 / 3.0)


def _scores(seed, n):
    return [float(k + 1) / (R + 1) for k in synth.round_ids(seed, n, R, 2)]


_cache = {}


def _case(seed, n, p):
    if (seed, n, p) not in _cache:
        X, w, sc = _rows(seed, n, p), synth.cardinalities(seed, n), _scores(seed, n)
        plain, scored = O.fedavg_stacked(X, w), O.fedavg_stacked(X, w, sc)
        assert plain.dtype == F64 and np.isfinite(plain).all() and plain.any() and not same_bits(plain, scored)
        _cache[(seed, n, p)] = (X, w, sc, plain, scored)
    return _cache[(seed, n, p)]


def _separate(X, dev, off=0):
    """One allocation per row; off=1: views 8 bytes into their allocation."""
    rows = []
    for x in X:
        t = torch.zeros(x.size + 2, dtype=torch.float64, device=dev)
        t[off:off + x.size].copy_(torch.from_numpy(x))
        rows.append(t[off:off + x.size])
    return rows


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("place", ["aligned", "offset8", "rowset_reused", "np_float64_weights", "out_given",
                                   "out_over_a_row"])
def test_fold_rows_takes_the_table(dev, place, scored):
    from fedlesscan_amd import engine
    n, p = 19, LAYERS[0]
    X, w, sc, plain, scored_exp = _case(31, n, p)
    exp = scored_exp if scored else plain
    sc = sc if scored else None
    rows = _separate(X, dev, off=1 if place == "offset8" else 0)
    before = dict(engine.stats)
    folds = 1
    if place == "rowset_reused":
        rs = engine.RowSet(rows)
        assert rs.view is None and rs.ptrs is not None and rs.aligned
        got = engine.fold_rows(rs, w, sc)
        rows[3].mul_(2.0)  # the contents may change between folds
        got2 = engine.fold_rows(rs, w, sc)
        X2 = X.copy()
        X2[3] *= 2.0
        assert same_bits(got2.cpu().numpy(), O.fedavg_stacked(X2, w, sc))
        folds = 2
    elif place == "np_float64_weights":
        got = engine.fold_rows(rows, [np.float64(v) for v in w], sc)  # float64 stays float64: still the table
    elif place == "out_given":
        out = torch.full((p + 3,), 7.0, dtype=torch.float64, device=dev)
        got = engine.fold_rows(rows, w, sc, out=out)
        assert got is out and (out[p:] == 7.0).all()
        got = out[:p]
    elif place == "out_over_a_row":
        got = engine.fold_rows(rows, w, sc, out=rows[2])  # folded into a fresh buffer, then copied
        assert got is rows[2]
    else:
        rs = engine.RowSet(rows)
        assert rs.view is None and rs.aligned == (place == "aligned")
        got = engine.fold_rows(rs, w, sc)
    assert engine.stats["rows64_folds"] - before["rows64_folds"] == folds
    assert engine.stats["rows16_folds"] == before["rows16_folds"]
    assert engine.stats["stacked_groups"] == before["stacked_groups"]
    assert got.dtype == torch.float64 and same_bits(got.cpu().numpy(), exp)
    # the same bits as the stacked fold over the same rows
    ref = engine.fold_stacked(torch.from_numpy(X).to(dev), w, sc)
    assert same_bits(got.cpu().numpy(), ref.cpu().numpy())


def test_equal_stride_views_keep_the_strided_stacked_fold(dev):
    from fedlesscan_amd import engine
    n, p = 19, LAYERS[0]
    X, w, sc, plain, scored = _case(31, n, p)
    S = torch.zeros((n, p + 3), dtype=torch.float64, device=dev)
    S[:, :p].copy_(torch.from_numpy(X))
    rs = engine.RowSet([S[i, :p] for i in range(n)])
    assert rs.view is not None and rs.ptrs is None
    before = dict(engine.stats)
    got = engine.fold_rows(rs, w, sc)
    assert engine.stats["rows64_folds"] == before["rows64_folds"]
    assert engine.stats["stacked_groups"] == before["stacked_groups"]
    assert same_bits(got.cpu().numpy(), scored)


def test_promoting_factors_keep_the_stacked_route(dev):
    """np.longdouble weights promote a float64 fold where long double is wider:
    no row-table fold does that arithmetic, so fold_rows does not take the table."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    if np.dtype(np.longdouble) == np.dtype(F64):
        pytest.skip("long double is double on this platform")
    n, p = 5, 33
    X, w, sc, plain, scored = _case(33, n, p)
    rows = _separate(X, dev)
    before = dict(engine.stats)
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_rows(rows, [np.longdouble(v) for v in w])
    assert engine.stats["rows64_folds"] == before["rows64_folds"]


@pytest.mark.parametrize("strategy", ["fedavg", "stall_aware", "aggregate_layers"])
def test_strategy_classes_fold_through_the_row_table(dev, strategy):
    from fedlesscan_amd import FedAvgAggregator, StallAwareAggregator, engine
    from fedlesscan_amd.common.models import AggregationHyperParams
    n, seed = 9, 41
    host = [[_rows(seed + 10 * li, n, sz)[i] for li, sz in enumerate(LAYERS)] for i in range(n)]
    params = [[torch.from_numpy(x.copy()).to(dev) for x in cl] for cl in host]
    w = synth.cardinalities(seed, n)
    feats = [{"round_id": r} for r in synth.round_ids(seed, n, R, 2)]
    before = dict(engine.stats)
    if strategy == "fedavg":
        got = FedAvgAggregator()._aggregate(params, w)
        exp = O.fedavg_literal(host, w)
    elif strategy == "aggregate_layers":
        got = engine.aggregate_layers(params, w)
        exp = O.fedavg_literal(host, w)
    else:
        got = StallAwareAggregator(R, AggregationHyperParams(tolerance=2))._aggregate(feats, params, w)
        exp = O.stall_aware_literal(feats, R, host, w)
    assert engine.stats["rows64_folds"] - before["rows64_folds"] == len(LAYERS)
    assert engine.stats["stacked_groups"] == before["stacked_groups"]
    assert len(got) == len(LAYERS)
    for li, (g, e) in enumerate(zip(got, exp)):
        assert g.is_cuda and g.dtype == torch.float64 and tuple(g.shape) == (LAYERS[li],)
        assert np.isfinite(e).all() and e.any()
        assert same_bits(g.cpu().numpy(), e), (strategy, li)


def test_no_stacking_copy_in_memory(dev):
    """16 rows of 64K doubles (8 MB): one fold_rows raises the peak of allocated
    memory by less than half the input's size -- a stacked copy alone needs all
    of it.  The result equals the stacked fold over the same rows."""
    from fedlesscan_amd import engine
    n, p = 16, 1 << 16
    X = _rows(51, n, p)
    w = synth.cardinalities(51, n)
    rows = [torch.from_numpy(x.copy()).to(dev) for x in X]
    rs = engine.RowSet(rows)
    assert rs.view is None and rs.aligned
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = engine.fold_rows(rs, w)
    torch.cuda.synchronize(dev)
    rise = torch.cuda.max_memory_allocated(dev) - base
    print(f"peak rise {rise} bytes for {8 * n * p} input bytes")
    assert rise < 4 * n * p, rise
    ref = engine.fold_stacked(torch.stack(rows), w)
    assert out.dtype == torch.float64 and torch.equal(out.view(torch.int64), ref.view(torch.int64))
    assert same_bits(out.cpu().numpy(), O.fedavg_stacked(X, w))
