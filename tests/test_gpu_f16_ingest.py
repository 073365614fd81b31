"""GPU: float16 models from host blobs through the native ingest pipe.

The raw float16 pipe (fa_ingest_*_f16) and every public route that folds host
float16 rows -- aggregate() on NPZ results, the stream variants, _aggregate on
numpy layers, the handler -- must give numpy's own literal float16 left fold
(oracle.fedavg_oracle: reduce(np.add, [x_i * n_i (* s_i)]) / sum(n) with
Python-number factors), bit for bit, NaN by position; the same bits as the
same call under FEDAVG_F16_STREAM=0 (the materialised route: stack, one H2D,
one fa_fedavg_f16); and the route counters must show which route ran.

Ordinary inputs: rows uniform in [-1, 1), weights Python ints 1..40, scores in
(0, 1], N = 33, so |acc| <= 1320 and the total <= 1320: every expected value is
finite, which the tests assert."""
import ctypes

import numpy as np
import pytest

from oracle import fedavg_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F16 = np.float16
SENTINEL = 0x5A5A
N, P, R = 33, 2059, 10
SHAPES = [(10, 10), (7,), (), (1951,)]  # 100 + 7 + 1 + 1951 = 2059 columns, a 0-d layer among them
PIECES = (5, 1001, 1053)  # a row handed over as three pieces with odd element counts


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def same_bits16(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F16 or b.dtype != F16 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~na]))


def _bits(v) -> int:
    return int(np.asarray(F16(v)).view(np.uint16))


def _weights(seed, n=N):
    return [int(v) for v in np.random.default_rng(seed + 1000).integers(1, 41, n)]


def _scores(seed, n=N):
    return [float(v) for v in 1.0 - np.random.default_rng(seed + 2000).random(n)]  # (0, 1]


def _feats(seed, n=N):
    return [{"round_id": int(r)} for r in np.random.default_rng(seed + 3000).integers(R - 2, R + 1, n)]


def _model(seed, n=N, shapes=SHAPES):
    rng = np.random.default_rng(seed)
    # np.asarray: the 0-d layer is an array too, as a decoded NPZ member is
    return [[np.asarray((rng.random(s, dtype=np.float32) * 2 - 1).astype(F16)) for s in shapes] for _ in range(n)]


def _finite(layers):
    assert all(np.asarray(x).dtype == F16 and np.isfinite(x).all() for x in layers)
    assert any(np.asarray(x).any() for x in layers)


def _layers_equal(got, exp, what=""):
    assert len(got) == len(exp), what
    for g, e in zip(got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.dtype == e.dtype and g.shape == e.shape, (what, g.dtype, e.dtype, g.shape, e.shape)
        assert same_bits16(g, e), what


# ---------------------------------------------------------------------------
# 1. the raw pipe
# ---------------------------------------------------------------------------
class Pipe:
    def __init__(self, dev, rows_per_chunk=3, slots=3, f16=True):
        from fedlesscan_amd import _lib
        self.L, self.dev, self.f16 = _lib.load(), dev, f16
        self.h = ctypes.c_void_p()
        ldx = (P + 63) // 64 * 64
        create = self.L.fa_ingest_create_f16 if f16 else self.L.fa_ingest_create
        _lib.check(create(ctypes.byref(self.h), P, rows_per_chunk * ldx * (2 if f16 else 4), slots, dev.index),
                   "fa_ingest_create")
        assert self.L.fa_ingest_rows_per_chunk(self.h) == rows_per_chunk
        self.st = torch.cuda.current_stream(dev).cuda_stream

    def close(self):
        self.L.fa_ingest_destroy(self.h)

    def begin(self, expected):
        from fedlesscan_amd import _lib
        acc = torch.full((P,), SENTINEL, dtype=torch.int16, device=self.dev)
        _lib.check(self.L.fa_ingest_begin_f16(self.h, acc.data_ptr(), self.st, expected), "fa_ingest_begin_f16")
        return acc

    def add(self, row, w, s, keep):
        from fedlesscan_amd import _lib
        parts, off = [], 0
        for n in PIECES:
            parts.append(row[off:off + n].copy())
            off += n
        assert off == P and all(n % 2 == 1 for n in PIECES)
        keep.append(parts)
        ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in parts])
        sizes = (ctypes.c_int64 * 3)(*[a.nbytes for a in parts])
        _lib.check(self.L.fa_ingest_add_f16(self.h, ptrs, sizes, 3, _bits(w), 0x3C00 if s is None else _bits(s),
                                            0 if s is None else 1), "fa_ingest_add_f16")

    def round(self, X, w, sc, expected):
        from fedlesscan_amd import _lib
        acc, keep = self.begin(expected), []
        for i in range(len(w)):
            self.add(X[i], w[i], None if sc is None else sc[i], keep)
        _lib.check(self.L.fa_ingest_finish_f16(self.h, _bits(sum(w))), "fa_ingest_finish_f16")
        torch.cuda.synchronize()
        return acc.cpu().numpy().view(F16)


@pytest.fixture(scope="module")
def flat_case():
    rng = np.random.default_rng(5)
    X = (rng.random((N, P), dtype=np.float32) * 2 - 1).astype(F16)
    w, sc = _weights(5), _scores(5)
    plain, scored = O.fedavg_stacked(X, w), O.fedavg_stacked(X, w, sc)
    assert plain.dtype == F16 and np.isfinite(plain).all() and np.isfinite(scored).all()
    return X, w, sc, plain, scored


@pytest.mark.parametrize("rows_per_chunk", [1, 2, 3])
@pytest.mark.parametrize("known", [False, True], ids=["rows_unknown", "rows_known"])
def test_raw_pipe_rounds(dev, flat_case, rows_per_chunk, known):
    """1-3 rows per chunk, so the ramp, full chunks and (with the row count
    announced) the halving tail all occur; plain then scored on one pipe."""
    X, w, sc, plain, scored = flat_case
    p = Pipe(dev, rows_per_chunk)
    try:
        assert same_bits16(p.round(X, w, None, N if known else 0), plain)
        assert same_bits16(p.round(X, w, sc, N if known else 0), scored)
    finally:
        p.close()


def test_raw_pipe_abandoned_round_then_a_clean_one(dev, flat_case):
    X, w, sc, plain, scored = flat_case
    p = Pipe(dev, 3)
    try:
        keep = []
        abandoned = p.begin(N)  # stays alive: the chunks already sent fold into it
        for i in range(5):  # chunks of 1, 2 rows sent, 2 rows in a half-filled chunk; no finish
            p.add(X[N - 1 - i], 40, None, keep)
        assert same_bits16(p.round(X, w, sc, N), scored)
        assert same_bits16(p.round(X, w, None, 0), plain)
        del abandoned
    finally:
        p.close()


def test_raw_pipe_wrong_kind_calls_refused(dev, flat_case):
    from fedlesscan_amd import _lib
    X, w, sc, plain, scored = flat_case
    L = _lib.load()
    row = X[0].copy()
    ptrs, sizes = (ctypes.c_void_p * 1)(row.ctypes.data), (ctypes.c_int64 * 1)(row.nbytes)
    acc16 = torch.zeros(P, dtype=torch.int16, device=dev)
    acc32 = torch.zeros(P, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    p = Pipe(dev, 3)
    q = Pipe(dev, 3, f16=False)
    try:
        assert L.fa_ingest_begin(p.h, acc32.data_ptr(), st, 0) == _lib.FA_ERR_ARG
        assert "kind" in _lib.last_error()
        acc = p.begin(0)
        assert L.fa_ingest_add(p.h, ptrs, sizes, 1, 1.0, 1.0, 0) == _lib.FA_ERR_ARG
        assert L.fa_ingest_finish(p.h, 1.0) == _lib.FA_ERR_ARG
        del acc
        assert same_bits16(p.round(X, w, None, N), plain)  # the refused calls left the pipe usable
        assert L.fa_ingest_begin_f16(q.h, acc16.data_ptr(), st, 0) == _lib.FA_ERR_ARG
        assert L.fa_ingest_begin(q.h, acc32.data_ptr(), st, 0) == _lib.FA_OK
        assert L.fa_ingest_add_f16(q.h, ptrs, sizes, 1, 0x3C00, 0x3C00, 0) == _lib.FA_ERR_ARG
        assert L.fa_ingest_finish_f16(q.h, 0x3C00) == _lib.FA_ERR_ARG
        assert L.fa_ingest_finish(q.h, 1.0) == _lib.FA_ERR_NO_CLIENTS  # no row was taken
    finally:
        p.close()
        q.close()


def test_native_streaming_fold_float16(dev, flat_case):
    """ingest.NativeStreamingFold(dtype=float16): float16 accumulator, factors
    rounded as fold_stacked rounds them, pipes cached by dtype, float32 rows refused."""
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    from fedlesscan_amd.ingest import NativeStreamingFold, make_streaming_fold
    X, w, sc, plain, scored = flat_case
    ldx = (P + 63) // 64 * 64
    before = NativeStreamingFold.stats["rows"]
    sf = NativeStreamingFold(P, dev, chunk_bytes=3 * ldx * 2, slots=2, expected_rows=N, dtype=np.float16)
    assert sf.acc.dtype == torch.float16 and sf.key[-1] == "float16"
    for i in range(N):
        sf.add([X[i, :100].reshape(10, 10), X[i, 100:]], w[i], sc[i])
    got = sf.finish()
    torch.cuda.synchronize()
    assert same_bits16(got.cpu().numpy(), scored)
    assert NativeStreamingFold.stats["rows"] - before == N
    f32 = NativeStreamingFold(P, dev, chunk_bytes=3 * ldx * 2, slots=2)  # same shape, its own (float32) pipe
    assert f32.acc.dtype == torch.float32 and f32.key != sf.key and f32.key[:-1] == sf.key[:-1]
    f32.abandon()
    sf = make_streaming_fold(P, dev, 1 << 20, direct=True, dtype=np.float16)  # float16: always the native pipe
    assert isinstance(sf, NativeStreamingFold)
    with pytest.raises(InvalidParameterShapeError):
        sf.add(X[0].astype(np.float32), 1)
    # a factor that overflows stays inf, as fold_stacked forms it: x * inf, then inf / inf
    sf = NativeStreamingFold(P, dev, chunk_bytes=1 << 20, dtype=np.float16)
    with np.errstate(all="ignore"):
        sf.add(X[0], 70000)
        sf.add(X[1], 1)
        got = sf.finish().cpu().numpy()
        exp = O.fedavg_stacked(X[:2], [70000, 1])
    assert np.isnan(exp).all() and same_bits16(got, exp)


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
    """run() on the streamed route and under FEDAVG_F16_STREAM=0: numpy's bits
    from both, `rows` more rows through the pipe and no stacked group on the
    first, the reverse on the second."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    _finite(exp)
    monkeypatch.delenv("FEDAVG_F16_STREAM", raising=False)
    r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
    got = run()
    assert NativeStreamingFold.stats["rows"] - r0 == rows, what
    assert engine.stats["stacked_groups"] == g0, what
    monkeypatch.setenv("FEDAVG_F16_STREAM", "0")
    r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
    mat = run()
    assert NativeStreamingFold.stats["rows"] == r0 and engine.stats["stacked_groups"] > g0, what
    monkeypatch.delenv("FEDAVG_F16_STREAM")
    _layers_equal(got, exp, (what, "numpy"))
    _layers_equal(got, mat, (what, "materialised route"))
    return got


@pytest.fixture(scope="module")
def model_case():
    params, w, feats = _model(21), _weights(21), _feats(21)
    return params, w, feats


def test_fedavg_aggregate_from_npz(dev, model_case, monkeypatch):
    from fedlesscan_amd import FedAvgAggregator
    params, w, _ = model_case
    exp, _ = O.aggregate_fedavg(_dict_results(params, w))
    got = _both_routes(monkeypatch, lambda: FedAvgAggregator().aggregate(_npz_results(params, w))[0], exp, N, "fedavg")
    assert all(isinstance(g, np.ndarray) for g in got)
    # an iterator (row count unknown) streams the same way
    _both_routes(monkeypatch, lambda: FedAvgAggregator().aggregate(iter(_npz_results(params, w)))[0], exp, N,
                 "fedavg, iterator")


def test_stall_aware_aggregate_from_npz(dev, model_case, monkeypatch):
    from fedlesscan_amd import StallAwareAggregator
    from fedlesscan_amd.common.models import AggregationHyperParams
    params, w, feats = model_case
    exp, _ = O.aggregate_stall_aware(_dict_results(params, w), feats, R)
    _both_routes(monkeypatch,
                 lambda: StallAwareAggregator(R, AggregationHyperParams(tolerance=2)).aggregate(
                     _npz_results(params, w), feats)[0], exp, N, "stall-aware")


@pytest.mark.parametrize("chunk", [1, 2, 10])
def test_stream_variants_from_npz(dev, model_case, monkeypatch, chunk):
    """The running aggregate (float16, on the host) is fed back as row 0 of
    every chunk after the first, so N + chunks - 1 rows go through the pipe."""
    from fedlesscan_amd import StreamFedAvgAggregator, StreamStallAwareAggregator
    from fedlesscan_amd.common.models import AggregationHyperParams
    params, w, feats = model_case
    rows = N + (N + chunk - 1) // chunk - 1
    exp, _ = O.aggregate_stream_fedavg(_dict_results(params, w), chunk_size=chunk)
    _both_routes(monkeypatch,
                 lambda: StreamFedAvgAggregator(chunk_size=chunk).aggregate(iter(_npz_results(params, w)), feats)[0],
                 exp, rows, ("stream fedavg", chunk))
    exp, _ = O.aggregate_stream_stall_aware(_dict_results(params, w), feats, R, chunk_size=chunk)
    _both_routes(monkeypatch,
                 lambda: StreamStallAwareAggregator(R, AggregationHyperParams(tolerance=2), chunk_size=chunk).aggregate(
                     iter(_npz_results(params, w)), feats)[0], exp, rows, ("stream stall-aware", chunk))


def test_aggregate_numpy_float16_layers(dev, model_case, monkeypatch):
    from fedlesscan_amd import FedAvgAggregator, StallAwareAggregator
    from fedlesscan_amd.common.models import AggregationHyperParams
    params, w, feats = model_case
    exp = O.fedavg_literal(params, w)
    _both_routes(monkeypatch, lambda: FedAvgAggregator()._aggregate(params, w), exp, N, "_aggregate")
    exp = O.stall_aware_literal(feats, R, params, w)
    _both_routes(monkeypatch,
                 lambda: StallAwareAggregator(R, AggregationHyperParams(tolerance=2))._aggregate(feats, params, w),
                 exp, N, "_aggregate, scored")


def test_handler_saves_float16_npz(dev, model_case, monkeypatch):
    from fedlesscan_amd.common.models import NpzWeightsSerializerConfig, WeightsSerializerConfig
    from fedlesscan_amd.common.serialization import NpzWeightsSerializer
    from fedlesscan_amd.handler import default_aggregation_handler
    from fedlesscan_amd.store import InMemoryClientResultStore, InMemoryParameterStore
    params, w, _ = model_case
    exp, _ = O.aggregate_fedavg(_dict_results(params, w))

    def run():
        st, ps = InMemoryClientResultStore(), InMemoryParameterStore()
        for i, r in enumerate(_npz_results(params, w)):
            st.save("s", 3, f"c{i}", r)
        cfg = WeightsSerializerConfig(type="npz", params=NpzWeightsSerializerConfig())
        res = default_aggregation_handler("s", 3, st, ps, cfg)
        assert res.new_round_id == 4 and res.num_clients == N
        return NpzWeightsSerializer().deserialize(ps.load("s", 4).blob)

    _both_routes(monkeypatch, run, exp, N, "handler")


# ---------------------------------------------------------------------------
# 3. fallbacks: the materialised route takes over, the next round streams again
# ---------------------------------------------------------------------------
def _clean_round_streams(params, w):
    """A fresh round right after a fallback: through the pipe, numpy's bits."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
    got = engine.aggregate_decoded(iter(zip(params, w)))
    assert NativeStreamingFold.stats["rows"] - r0 == len(w) and engine.stats["stacked_groups"] == g0
    _layers_equal(got, O.fedavg_literal(params, w), "clean round after a fallback")


def _mixed_weights(w):
    w = list(w)
    w[N // 2] = np.float32(w[N // 2])  # a numpy scalar in the middle of the stream: numpy promotes the fold
    return w


def test_fallback_numpy_scalar_weight_mid_stream(dev, model_case, monkeypatch):
    """The rows before the numpy-scalar weight have entered the pipe; the round
    is abandoned and every row takes the materialised route: a float32 result,
    the bits of the same call under FEDAVG_F16_STREAM=0, and a pipe that the
    next round uses."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    params, w, _ = model_case
    wm = _mixed_weights(w)
    monkeypatch.delenv("FEDAVG_F16_STREAM", raising=False)
    r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
    got = engine.aggregate_decoded(iter(zip(params, wm)))
    assert NativeStreamingFold.stats["rows"] - r0 == N // 2  # the rows ahead of it were streamed, then dropped
    assert engine.stats["stacked_groups"] == g0 + 1
    monkeypatch.setenv("FEDAVG_F16_STREAM", "0")
    mat = engine.aggregate_decoded(iter(zip(params, wm)))
    monkeypatch.delenv("FEDAVG_F16_STREAM")
    assert [g.dtype for g in got] == [np.float32] * len(SHAPES) == [m.dtype for m in mat]
    assert all(g.shape == m.shape and np.array_equal(g.view(np.uint32), m.view(np.uint32)) for g, m in zip(got, mat))
    _clean_round_streams(params, w)


def _flat32(layers):
    assert [np.asarray(x).dtype for x in layers] == [np.float32] * len(SHAPES)
    return np.concatenate([np.asarray(x).ravel() for x in layers]).view(np.uint32)


def test_fallback_numpy_scalar_weight_matches_numpy(dev, model_case):
    """The same fallback against numpy's literal fold of the same weights
    (float32, as numpy promotes), bit for bit.  With ONE numpy-scalar weight
    among Python numbers numpy still rounds every other product, and every sum
    ahead of that row, to float16 and only then widens; a fold that widened
    every row first gave other bits in 2058 of these 2059 columns (by up to
    5.7e-4 of the largest value), so the materialised route folds such mixes
    the way numpy does (engine._fold_general)."""
    from fedlesscan_amd import engine
    params, w, _ = model_case
    wm = _mixed_weights(w)
    exp = O.fedavg_literal(params, wm)
    got = engine.aggregate_decoded(iter(zip(params, wm)))
    ge, gg = _flat32(exp), _flat32(got)
    print(f"numpy-scalar weight mid-stream: {int((ge != gg).sum())} of {ge.size} columns differ from numpy")
    assert np.array_equal(ge, gg)


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("where", ["first", "two_runs", "last", "int16"])
def test_mixed_weights_fold_as_numpy(dev, model_case, where, scored):
    """Other places for the numpy scalars: the first row (the fold starts in
    float32, float16 terms follow), two separate runs, the last row (a float16
    running sum widened at the very end), and an np.int16 weight (a float32
    term by numpy's promotion, and the total an np.int16)."""
    from fedlesscan_amd import engine
    params, w, feats = model_case
    n = 9
    params, w = params[:n], list(w[:n])
    sc = O.score_clients(feats[:n], R) if scored else None
    for i in {"first": [0], "two_runs": [2, 3, 6], "last": [n - 1], "int16": [4]}[where]:
        w[i] = np.int16(w[i]) if where == "int16" else np.float32(w[i])
    total = sum(w)
    terms = [[np.multiply(x, k) if sc is None else np.multiply(np.multiply(x, k), s) for x in layers]
             for layers, k, s in zip(params, w, sc or [None] * n)]
    from functools import reduce
    exp = [np.true_divide(reduce(np.add, per_layer), total) for per_layer in zip(*terms)]
    got = engine.aggregate_decoded(iter(zip(params, w)), sc)
    assert np.array_equal(_flat32(got), _flat32(exp))


def test_fallback_float32_row_mid_stream(dev, model_case, monkeypatch):
    """A float32 row among float16 rows: the pipe is abandoned at that row and
    the materialised route folds the rows as numpy does -- float16 up to the
    float32 row, float32 from there on, every later float16 term still rounded
    to float16 first -- the same on both routes, and the next round streams
    again."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    params, w, _ = model_case
    bad = [list(p) for p in params]
    bad[N // 2] = [x.astype(np.float32) for x in bad[N // 2]]
    exp = O.fedavg_literal(bad, w)
    assert {e.dtype for e in exp} == {np.dtype(np.float32)}
    monkeypatch.delenv("FEDAVG_F16_STREAM", raising=False)
    r0 = NativeStreamingFold.stats["rows"]
    streamed = engine.aggregate_decoded(iter(zip(bad, w)))
    assert NativeStreamingFold.stats["rows"] - r0 == N // 2
    monkeypatch.setenv("FEDAVG_F16_STREAM", "0")
    materialised = engine.aggregate_decoded(iter(zip(bad, w)))
    monkeypatch.delenv("FEDAVG_F16_STREAM")
    for got in (streamed, materialised):
        assert len(got) == len(exp)
        for g, e in zip(got, exp):
            assert g.dtype == e.dtype and g.shape == e.shape
            assert np.array_equal(np.asarray(g).reshape(-1).view(np.uint32), e.reshape(-1).view(np.uint32))
    _clean_round_streams(params, w)
    # mixed-dtype rows never enter the pipe: the first row already is not fast
    mixed = [[p[0].astype(np.float32), *p[1:]] for p in params]
    r0 = NativeStreamingFold.stats["rows"]
    got = engine.aggregate_decoded(iter(zip(mixed, w)))
    # inside aggregate_layers its float32 group streams as before, and its float16 group through a float16 pipe
    assert NativeStreamingFold.stats["rows"] - r0 == 2 * N
    assert [g.dtype for g in got] == [np.float32] + [F16] * (len(SHAPES) - 1)
    exp = O.fedavg_literal(mixed, w)
    assert np.array_equal(got[0].view(np.uint32), exp[0].view(np.uint32))
    _layers_equal(got[1:], exp[1:], "mixed rows")
