"""GPU: float64 models from host blobs through the native ingest pipe.

ingest.NativeStreamingFold(dtype=float64) and every public route that folds
host float64 rows -- aggregate() on NPZ results, aggregate_decoded and
aggregate_layers on numpy float64 layers -- must give numpy's own literal
float64 left fold (oracle.fedavg_oracle: reduce(np.add, [x_i * n_i (* s_i)]) /
sum(n)), bit for bit (view(np.uint64)), NaN by position; the same bits as the
same call under FEDAVG_F64_STREAM=0 (the materialised route: stack, one H2D,
one fa_fedavg_f64); and the route counters must show which route ran.

Inputs: synth.clients_f32(...).astype(float64) * (1 + 1/3) with
synth.cardinalities weights (tests/test_f64_host.py keeps on record what these
inputs tell apart)."""
import ctypes

import numpy as np
import pytest

from fedlesscan_amd import synth
from oracle import fedavg_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64 = np.float64
N, P, R = 37, 70001, 10
LDX = (P + 63) // 64 * 64
PIECES = (5, 40001, 29995)  # a row handed over as three pieces; the second crosses the 256 KiB tasks of the ramp
SHAPES = [(10, 10), (7,), (), (1951,)]  # a 0-d layer among them
FIXTURE_SHAPES = [(1, 2, 3), (1, 2, 3)]  # the reference's own aggregation fixture: 3 clients, weights 1.0, 2.0, 0.0


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


def _feats(seed, n):
    return [{"round_id": int(r)} for r in synth.round_ids(seed, n, R, 2)]


def _model(seed, n, shapes):
    sizes = [int(np.prod(s)) if len(s) else 1 for s in shapes]
    X = _rows(seed, n, sum(sizes))
    offs = np.cumsum([0, *sizes])
    # np.asarray: the 0-d layer is an array too, as a decoded NPZ member is
    return [[np.asarray(X[i, offs[k]:offs[k + 1]].reshape(s)) for k, s in enumerate(shapes)] for i in range(n)]


def _layers_equal(got, exp, what=""):
    assert len(got) == len(exp), what
    for g, e in zip(got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.dtype == e.dtype == F64 and g.shape == e.shape, (what, g.dtype, e.dtype, g.shape, e.shape)
        assert same_bits(g, e), what


@pytest.fixture(scope="module")
def flat_case():
    X = _rows(5, N, P)
    w, sc = synth.cardinalities(5, N), _scores(5, N)
    plain, scored = O.fedavg_stacked(X, w), O.fedavg_stacked(X, w, sc)
    assert plain.dtype == F64 and np.isfinite(plain).all() and np.isfinite(scored).all() and plain.any()
    assert not same_bits(plain, scored)
    return X, w, sc, plain, scored


# ---------------------------------------------------------------------------
# 1. NativeStreamingFold(dtype=float64)
# ---------------------------------------------------------------------------
def _pieces(row):
    out, off = [], 0
    for n in PIECES:
        out.append(row[off:off + n])
        off += n
    assert off == row.size
    return out


def _stream(dev, X, w, sc, chunk_rows, slots, expected, total=None, pieces=_pieces):
    from fedlesscan_amd.ingest import NativeStreamingFold
    ldx = (X.shape[1] + 63) // 64 * 64
    sf = NativeStreamingFold(X.shape[1], dev, chunk_bytes=chunk_rows * ldx * 8, slots=slots, expected_rows=expected,
                             dtype=F64)
    assert sf.acc.dtype == torch.float64 and sf.key[-1] == "float64"
    assert sf.L.fa_ingest_rows_per_chunk(sf.pipe) == chunk_rows
    for i in range(len(w)):
        sf.add(pieces(X[i]), w[i], None if sc is None else sc[i])
    got = sf.finish(total=total)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("chunk_rows", [1, 2, 5, 64])
def test_native_streaming_fold_float64(dev, flat_case, chunk_rows, slots, scored):
    """1-64 rows per chunk: the ramp, full chunks and (row count announced) the
    halving tail all occur; 64 rows per chunk never fills one."""
    from fedlesscan_amd.ingest import NativeStreamingFold
    X, w, sc, plain, scored_exp = flat_case
    before = NativeStreamingFold.stats["rows"]
    got = _stream(dev, X, w, sc if scored else None, chunk_rows, slots, N if chunk_rows != 2 else 0)
    assert same_bits(got, scored_exp if scored else plain)
    assert NativeStreamingFold.stats["rows"] - before == N


def test_pieces_across_the_copy_task_boundary(dev):
    """Rows of 1.07 MiB handed over as two layers: the first crosses the 1 MiB
    copy-task boundary, the second starts inside the second task."""
    n, p = 7, 140001
    X = _rows(9, n, p)
    w = synth.cardinalities(9, n)
    exp = O.fedavg_stacked(X, w)
    cut = 135007  # 1080056 bytes: past 1 MiB
    assert cut * 8 > (1 << 20)
    got = _stream(dev, X, w, None, 2, 3, n, pieces=lambda r: [r[:cut].reshape(-1, 1), r[cut:]])
    assert same_bits(got, exp)


def test_pipe_reuse_over_three_rounds_and_total_override(dev, flat_case):
    from fedlesscan_amd.ingest import NativeStreamingFold, _pipes, make_streaming_fold
    X, w, sc, plain, scored = flat_case
    for k in range(3):  # the same key: the pipe of round k - 1 serves round k
        got = _stream(dev, X, w, sc if k == 1 else None, 5, 3, N)
        assert same_bits(got, scored if k == 1 else plain), k
        assert any(key[-1] == "float64" for key in _pipes.idle)
    total = sum(w) + 1000
    exp = O.fedavg_stacked(X, w, None, total=total)
    got = _stream(dev, X, w, None, 5, 3, N, total=total)
    assert same_bits(got, exp) and not same_bits(got, plain)
    sf = make_streaming_fold(P, dev, 1 << 22, direct=True, dtype=F64)  # float64: always the native pipe
    assert isinstance(sf, NativeStreamingFold) and sf.dtype == F64
    sf.abandon()


def test_float32_row_on_a_float64_pipe_raises(dev, flat_case):
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    from fedlesscan_amd.ingest import NativeStreamingFold
    X, w, sc, plain, scored = flat_case
    sf = NativeStreamingFold(P, dev, chunk_bytes=2 * LDX * 8, slots=2, dtype=F64)
    sf.add(X[0], w[0])
    with pytest.raises(InvalidParameterShapeError):
        sf.add(X[1].astype(np.float32), w[1])
    with pytest.raises(InvalidParameterShapeError):  # the failed fold stays failed
        sf.add(X[1], w[1])
    got = _stream(dev, X, w, None, 2, 2, N)  # and the next fold is clean
    assert same_bits(got, plain)


def test_raw_pipe_wrong_kind_calls_refused(dev, flat_case):
    from fedlesscan_amd import _lib
    X, w, sc, plain, scored = flat_case
    L = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    h = ctypes.c_void_p()
    _lib.check(L.fa_ingest_create_f64(ctypes.byref(h), P, 3 * LDX * 8, 3, dev.index), "fa_ingest_create_f64")
    try:
        assert L.fa_ingest_rows_per_chunk(h) == 3
        row = X[0].copy()
        ptrs, sizes = (ctypes.c_void_p * 1)(row.ctypes.data), (ctypes.c_int64 * 1)(row.nbytes)
        acc64 = torch.zeros(P, dtype=torch.float64, device=dev)
        acc32 = torch.zeros(P, dtype=torch.float32, device=dev)
        assert L.fa_ingest_begin(h, acc32.data_ptr(), st, 0) == _lib.FA_ERR_ARG
        assert "kind" in _lib.last_error()
        assert L.fa_ingest_begin_f16(h, acc32.data_ptr(), st, 0) == _lib.FA_ERR_ARG
        assert L.fa_ingest_begin_f64(h, acc64.data_ptr(), st, 0) == _lib.FA_OK
        assert L.fa_ingest_add(h, ptrs, sizes, 1, 1.0, 1.0, 0) == _lib.FA_ERR_ARG
        assert L.fa_ingest_add_f16(h, ptrs, sizes, 1, 0x3C00, 0x3C00, 0) == _lib.FA_ERR_ARG
        assert L.fa_ingest_finish(h, 1.0) == _lib.FA_ERR_ARG
        short = (ctypes.c_int64 * 1)(row.nbytes - 8)
        assert L.fa_ingest_add_f64(h, ptrs, short, 1, 1.0, 1.0, 0) == _lib.FA_ERR_SHAPE
        assert L.fa_ingest_add_f64(h, ptrs, sizes, 1, 3.0, 1.0, 0) == _lib.FA_OK
        assert L.fa_ingest_finish_f64(h, 3.0) == _lib.FA_OK
        torch.cuda.synchronize()
        assert same_bits(acc64.cpu().numpy(), row * 3.0 / 3.0)
    finally:
        L.fa_ingest_destroy(h)


# ---------------------------------------------------------------------------
# 2. the public routes
# ---------------------------------------------------------------------------
def _npz_results(params, cards):
    from fedlesscan_amd.common.models import (ClientResult, NpzWeightsSerializerConfig, SerializedParameters,
                                              WeightsSerializerConfig)
    from fedlesscan_amd.common.serialization import NpzWeightsSerializer
    cfg = WeightsSerializerConfig(type="npz", params=NpzWeightsSerializerConfig())
    return [ClientResult(parameters=SerializedParameters(blob=NpzWeightsSerializer().serialize(p), serializer=cfg),
                         cardinality=c) for p, c in zip(params, cards)]


def _dict_results(params, cards):
    from fedlesscan_amd.common.serialization import NpzWeightsSerializer
    return [{"blob": NpzWeightsSerializer().serialize(p), "cardinality": c} for p, c in zip(params, cards)]


def _both_routes(monkeypatch, run, exp, rows, what):
    """run() on the streamed route and under FEDAVG_F64_STREAM=0: numpy's bits
    from both, `rows` more rows through the pipe and no stacked group on the
    first, the reverse on the second."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    assert all(np.asarray(x).dtype == F64 and np.isfinite(x).all() for x in exp) and any(np.asarray(x).any() for x in exp)
    monkeypatch.delenv("FEDAVG_F64_STREAM", raising=False)
    r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
    got = run()
    assert NativeStreamingFold.stats["rows"] - r0 == rows, what
    assert engine.stats["stacked_groups"] == g0, what
    monkeypatch.setenv("FEDAVG_F64_STREAM", "0")
    r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
    mat = run()
    assert NativeStreamingFold.stats["rows"] == r0 and engine.stats["stacked_groups"] > g0, what
    monkeypatch.delenv("FEDAVG_F64_STREAM")
    _layers_equal(got, exp, (what, "numpy"))
    _layers_equal(got, mat, (what, "materialised route"))
    return got


CASES = {"model": (33, SHAPES, None), "reference_fixture": (3, FIXTURE_SHAPES, [1.0, 2.0, 0.0])}


@pytest.fixture(scope="module", params=list(CASES))
def model_case(request):
    n, shapes, w = CASES[request.param]
    params = _model(21, n, shapes)
    return params, (w or synth.cardinalities(21, n)), _feats(21, n)


def test_fedavg_aggregate_from_npz(dev, model_case, monkeypatch):
    from fedlesscan_amd import FedAvgAggregator
    params, w, _ = model_case
    n = len(w)
    exp, _ = O.aggregate_fedavg(_dict_results(params, w))
    got = _both_routes(monkeypatch, lambda: FedAvgAggregator().aggregate(_npz_results(params, w))[0], exp, n, "fedavg")
    assert all(isinstance(g, np.ndarray) for g in got)
    # an iterator (row count unknown) streams the same way
    _both_routes(monkeypatch, lambda: FedAvgAggregator().aggregate(iter(_npz_results(params, w)))[0], exp, n,
                 "fedavg, iterator")


def test_stall_aware_aggregate_from_npz(dev, model_case, monkeypatch):
    from fedlesscan_amd import StallAwareAggregator
    from fedlesscan_amd.common.models import AggregationHyperParams
    params, w, feats = model_case
    exp, _ = O.aggregate_stall_aware(_dict_results(params, w), feats, R)
    _both_routes(monkeypatch,
                 lambda: StallAwareAggregator(R, AggregationHyperParams(tolerance=2)).aggregate(
                     _npz_results(params, w), feats)[0], exp, len(w), "stall-aware")


def test_aggregate_decoded_and_layers_on_numpy_float64(dev, model_case, monkeypatch):
    from fedlesscan_amd import FedAvgAggregator, StallAwareAggregator, engine
    from fedlesscan_amd.common.models import AggregationHyperParams
    params, w, feats = model_case
    n = len(w)
    exp = O.fedavg_literal(params, w)
    _both_routes(monkeypatch, lambda: engine.aggregate_decoded(iter(zip(params, w)), expected_rows=n), exp, n,
                 "aggregate_decoded")
    _both_routes(monkeypatch, lambda: engine.aggregate_layers(params, w), exp, n, "aggregate_layers")
    _both_routes(monkeypatch, lambda: FedAvgAggregator()._aggregate(params, w), exp, n, "_aggregate")
    exp = O.stall_aware_literal(feats, R, params, w)
    _both_routes(monkeypatch,
                 lambda: StallAwareAggregator(R, AggregationHyperParams(tolerance=2))._aggregate(feats, params, w),
                 exp, n, "_aggregate, scored")


# ---------------------------------------------------------------------------
# 3. fallbacks: the pipe is abandoned, the next round streams again
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_case():
    return _model(21, 33, SHAPES), synth.cardinalities(21, 33)


def _clean_round_streams(params, w):
    """A fresh round right after a fallback: through the pipe, numpy's bits."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
    got = engine.aggregate_decoded(iter(zip(params, w)))
    assert NativeStreamingFold.stats["rows"] - r0 == len(w) and engine.stats["stacked_groups"] == g0
    _layers_equal(got, O.fedavg_literal(params, w), "clean round after a fallback")


def test_fallback_numpy_scalar_weight_mid_stream(dev, big_case, monkeypatch):
    """A numpy-scalar weight in the middle of the stream: the rows ahead of it
    have entered the pipe, the round is abandoned there and aggregate_layers
    folds every row.  np.float64 weights keep a float64 fold float64, so numpy's
    bits come back from both routes."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    params, w = big_case
    n = len(w)
    wm = list(w)
    wm[n // 2] = np.float64(wm[n // 2])
    exp = O.fedavg_literal(params, wm)
    monkeypatch.delenv("FEDAVG_F64_STREAM", raising=False)
    r0 = NativeStreamingFold.stats["rows"]
    got = engine.aggregate_decoded(iter(zip(params, wm)))
    assert NativeStreamingFold.stats["rows"] - r0 >= n // 2  # the rows ahead of it were streamed, then dropped
    monkeypatch.setenv("FEDAVG_F64_STREAM", "0")
    g0 = engine.stats["stacked_groups"]
    mat = engine.aggregate_decoded(iter(zip(params, wm)))
    assert engine.stats["stacked_groups"] == g0 + 1
    monkeypatch.delenv("FEDAVG_F64_STREAM")
    _layers_equal(got, exp, "numpy-scalar weight")
    _layers_equal(mat, exp, "numpy-scalar weight, materialised")
    _clean_round_streams(params, w)


def test_fallback_float32_row_mid_stream(dev, big_case, monkeypatch):
    """A float32 row among float64 rows: the pipe is abandoned at that row and
    the rows fold as numpy types them (the float32 row widens in its product)."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    params, w = big_case
    n = len(w)
    bad = [list(p) for p in params]
    bad[n // 2] = [x.astype(np.float32) for x in bad[n // 2]]
    exp = O.fedavg_literal(bad, w)
    assert {e.dtype for e in exp} == {np.dtype(F64)}
    monkeypatch.delenv("FEDAVG_F64_STREAM", raising=False)
    r0 = NativeStreamingFold.stats["rows"]
    got = engine.aggregate_decoded(iter(zip(bad, w)))
    assert NativeStreamingFold.stats["rows"] - r0 == n // 2
    _layers_equal(got, exp, "float32 row mid-stream")
    _clean_round_streams(params, w)


def test_fallback_several_devices(dev, big_case, monkeypatch):
    """devices=[...] naming more than one bucket: float64 rows do not stream row
    by row (one GPU only, as float16) and never reach the float32-only
    MultiStreamingFold; aggregate_layers folds the float64 group on the first
    GPU of the list, through that GPU's own float64 pipe.  A GPU may repeat in
    the list (buckets sharing one GPU), so one GPU is enough to run this."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    from fedlesscan_amd.multigpu import MultiStreamingFold
    params, w = big_case
    n = len(w)
    exp = O.fedavg_literal(params, w)
    monkeypatch.delenv("FEDAVG_F64_STREAM", raising=False)
    made = []
    real = MultiStreamingFold.__init__

    def spy(self, *a, **k):
        made.append(1)
        real(self, *a, **k)

    monkeypatch.setattr(MultiStreamingFold, "__init__", spy)
    drained = []  # the row counts aggregate_decoded handed to aggregate_layers (its fallback)
    real_layers = engine.aggregate_layers

    def layers_spy(parameters, *a, **k):
        drained.append(len(parameters))
        return real_layers(parameters, *a, **k)

    monkeypatch.setattr(engine, "aggregate_layers", layers_spy)
    lists = [[0, 0]] + ([[0, 1]] if torch.cuda.device_count() > 1 else [])
    for devices in lists:
        assert engine._multi(devices) is not None  # a multi-GPU call
        r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
        got = engine.aggregate_decoded(iter(zip(params, w)), devices=devices)
        assert not made, devices  # no multi-GPU pipe for float64 rows
        _layers_equal(got, exp, ("aggregate_decoded", devices))
        # the rows did not stream while they were decoded: the iterator was drained and
        # aggregate_layers folded them, its float64 group through the first GPU's pipe
        assert drained == [n], devices
        drained.clear()
        assert NativeStreamingFold.stats["rows"] - r0 == n and engine.stats["stacked_groups"] == g0, devices
        got = real_layers(params, w, devices=devices)
        assert not made, devices
        _layers_equal(got, exp, ("aggregate_layers", devices))
        # the float32 model of the same call does take the multi-GPU pipe: the spy sees it
        p32 = [[x.astype(np.float32) for x in p] for p in params]
        engine.aggregate_decoded(iter(zip(p32, w)), devices=devices)
        assert made and not drained, devices
        made.clear()
        _clean_round_streams(params, w)
        assert not drained  # the clean round streamed row by row
    # one GPU listed is a one-GPU call: it streams row by row
    r0 = NativeStreamingFold.stats["rows"]
    got = engine.aggregate_decoded(iter(zip(params, w)), devices=[0])
    assert engine._multi([0]) is None and NativeStreamingFold.stats["rows"] - r0 == n and not made and not drained
    _layers_equal(got, exp, "devices=[0]")
