"""float16 models through ShardedAggregator on the GPU: the one-launch step
(fa_fedavg_f16_rounds), per-round launches (fa_fedavg_f16 with staged factors),
the probe and its record, the per-layer entry, the refusals, and two ranks on
one GPU over gloo.  The expected model is numpy's literal float16 fold with
Python-number factors, bit for bit (NaN by position); weights 1..5."""
import os
import socket
from functools import reduce

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F16 = np.float16


def _numpy_fold(X, w, sc=None, total=None):
    with np.errstate(all="ignore"):
        terms = [X[i] * w[i] if sc is None else X[i] * w[i] * sc[i] for i in range(len(X))]
        out = reduce(np.add, terms) / (sum(w) if total is None else total)
    assert out.dtype == F16
    return out


def same_bits16(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F16 or b.dtype != F16 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~na]))


def _meaningful(exp) -> None:
    e = np.asarray(exp, F16).ravel()
    assert np.isfinite(e).all() and (np.abs(e.astype(np.float32)) >= 2.0 ** -14).any()


def _rows(seed, N, lo, n):
    """Columns [lo, lo + n) of the seed's [N, *] float16 clients (a column's
    values depend on the seed and the column only, so ranks agree)."""
    cols = np.arange(lo, lo + n, dtype=np.uint64)[None, :]
    rows = np.arange(N, dtype=np.uint64)[:, None]
    h = (cols * np.uint64(0x9E3779B97F4A7C15) + rows * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(seed)) >> np.uint64(40)
    return ((h.astype(np.float32) / np.float32(1 << 24)) * 2 - 1).astype(F16)


def _weights(seed, N):
    return [int(v) for v in np.random.default_rng(seed + 1000).integers(1, 6, N)]


def _scores(seed, N):
    return [float(v) for v in 1.0 - np.random.default_rng(seed + 2000).random(N)]


_cache = {}


def _expected(seed, N, P, scored):
    key = (seed, N, P, scored)
    if key not in _cache:
        exp = _numpy_fold(_rows(seed, N, 0, P), _weights(seed, N), _scores(seed, N) if scored else None)
        _meaningful(exp)
        _cache[key] = exp
    return _cache[key]


def _slots_input(N, P, seed, lay, dev, rank=0):
    X = torch.zeros((N, lay.local_width), dtype=torch.float16, device=dev)
    for k, (lo, hi) in enumerate(lay.slots(rank)):
        if hi > lo:
            X[:, lay.offset(k):lay.offset(k) + hi - lo] = torch.from_numpy(_rows(seed, N, lo, hi - lo)).to(dev)
    return X


def _host(full) -> np.ndarray:
    return full.view(torch.int16).cpu().numpy().view(F16)


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("one_launch", [True, False, "auto"])
@pytest.mark.parametrize("P,rounds", [(8003, 2), (65536, 4), (300001, 8)])
def test_slots_world1_f16(P, rounds, one_launch, scored):
    from fedlesscan_amd import engine
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout
    dev = torch.device("cuda", 0)
    N, seed = 13, 61
    lay = SlotLayout(P, 1, rounds)
    X = _slots_input(N, P, seed, lay, dev)
    w, sc = _weights(seed, N), (_scores(seed, N) if scored else None)
    agg = ShardedAggregator(one_launch=one_launch)
    calls = []
    real = engine.fold_rounds
    engine.fold_rounds = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        full = agg.aggregate_slots(X, w, sc, lay)
    finally:
        engine.fold_rounds = real
    assert len(calls) == (1 if one_launch is True else 0)  # "auto" with nothing recorded: per-round launches
    assert full.dtype == torch.float16 and full.numel() == P
    exp = _expected(seed, N, P, scored)
    assert same_bits16(_host(full), exp)
    out = torch.zeros(lay.padded_total, dtype=torch.float16, device=dev)
    again = agg.aggregate_slots(X, w, sc, lay, out=out)
    assert again.data_ptr() == out.data_ptr() and same_bits16(_host(again), exp)
    for dt in (torch.float32, torch.bfloat16):
        with pytest.raises(ValueError):
            agg.aggregate_slots(X, w, sc, lay, out=torch.zeros(lay.padded_total, dtype=dt, device=dev))


def test_engine_fold_rounds_and_fold_staged_f16():
    """engine.fold_rounds on float16 rows: a tensor out, a raw address with
    its capacity, factors given or rounded here; fold_staged with the staged
    halves; out_bf16 and outputs of another dtype are refused."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    from fedlesscan_amd.sharding import SlotLayout
    dev = torch.device("cuda", 0)
    N, P, seed = 13, 8003, 61
    lay = SlotLayout(P, 1, 2)
    X = _slots_input(N, P, seed, lay, dev)
    W = lay.local_width
    w, sc = _weights(seed, N), _scores(seed, N)
    exp = _expected(seed, N, P, True)
    offs = [lay.offset(k) for k in range(lay.rounds + 1)]
    out = torch.zeros(W, dtype=torch.float16, device=dev)
    engine.fold_rounds(X, w, sc, offs, out=out)
    assert same_bits16(_host(out)[:P], exp)
    f = engine.f16_factors(w, sc)
    raw = torch.zeros(W, dtype=torch.float16, device=dev)
    engine.fold_rounds(X, w, sc, offs, out=raw.data_ptr(), capacity=W, factors=f)
    assert same_bits16(_host(raw)[:P], exp)
    with pytest.raises(ValueError):
        engine.fold_rounds(X, w, sc, offs, out=raw.data_ptr(), capacity=W - 1)
    with pytest.raises(InvalidParameterShapeError, match="out_bf16"):
        engine.fold_rounds(X, w, sc, offs, out_bf16=torch.zeros(W, dtype=torch.bfloat16, device=dev))
    with pytest.raises(ValueError):
        engine.fold_rounds(X, w, sc, offs, out=torch.zeros(W, dtype=torch.float32, device=dev))
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_rounds(X, w, sc, offs, out=out, factors=engine.f32_factors(w, sc))
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_rounds(X, [np.float32(w[0])] + w[1:], sc, offs, out=out)
    sf = engine.StagedFactors(f, dev)
    assert sf.dtype == F16 and engine.StagedFactors(engine.f32_factors(w, sc), dev).dtype == np.float32
    staged = torch.zeros(W, dtype=torch.float16, device=dev)
    assert engine.fold_staged(X, sf, out=staged) is staged
    assert same_bits16(_host(staged)[:P], exp)
    with pytest.raises(ValueError):
        engine.fold_staged(X, sf, out=torch.zeros(W, dtype=torch.float32, device=dev))
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_staged(X.view(torch.bfloat16), sf, out_bf16=torch.zeros(W, dtype=torch.bfloat16, device=dev))


def test_odd_pitch_warns_and_folds_an_aligned_copy():
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout
    dev = torch.device("cuda", 0)
    N, P, seed = 13, 65536, 61
    lay = SlotLayout(P, 1, 4)
    X = _slots_input(N, P, seed, lay, dev)
    W = X.shape[1]
    base = torch.empty(N * (W + 1) + 1, dtype=X.dtype, device=dev)
    V = base[1:].view(N, W + 1)[:, :W]
    V.copy_(X)
    assert V.data_ptr() % 16 != 0 and V.stride(0) % 8 != 0
    w, sc = _weights(seed, N), _scores(seed, N)
    with pytest.warns(RuntimeWarning, match="aligned copy"):
        full = ShardedAggregator(one_launch=True).aggregate_slots(V, w, sc, lay)
    assert same_bits16(_host(full), _expected(seed, N, P, True))


def test_refusals():
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout
    dev = torch.device("cuda", 0)
    N, P, seed = 13, 8003, 61
    lay = SlotLayout(P, 1, 2)
    X = _slots_input(N, P, seed, lay, dev)
    w, sc = _weights(seed, N), _scores(seed, N)
    for one_launch in (True, False, "auto"):
        agg = ShardedAggregator(one_launch=one_launch)
        with pytest.raises(InvalidParameterShapeError, match="promote"):
            agg.aggregate_slots(X, [np.float32(w[0])] + w[1:], sc, lay)
        with pytest.raises(InvalidParameterShapeError, match="promote"):
            agg.aggregate(X[:, :lay.P], [np.float32(w[0])] + w[1:], sc, P=lay.P)
        with pytest.raises(InvalidParameterShapeError, match="RCCL"):
            ShardedAggregator(one_launch=one_launch, exchange="peer_copy").aggregate_slots(X, w, sc, lay)
    # graph capture: the per-round path reaches the fold's own refusal; the device folds correctly afterwards
    agg = ShardedAggregator(one_launch=True)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with pytest.raises(InvalidParameterShapeError, match="capture"):
        with torch.cuda.graph(g, stream=side):
            agg.aggregate_slots(X, w, sc, lay)
    torch.cuda.synchronize()
    assert same_bits16(_host(agg.aggregate_slots(X, w, sc, lay)), _expected(seed, N, P, True))


def test_probe_settles_and_records_under_the_f16_key(monkeypatch, tmp_path):
    """one_launch="probe" on float16 rows: every call exact, the decision
    recorded under the float16 key in the cache file; a bf16 record for the
    same layout is not picked up."""
    from fedlesscan_amd import _lib, engine
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout, step_key
    dev = torch.device("cuda", 0)
    session_cache = os.environ["FEDAVG_TUNE_CACHE"]
    path = str(tmp_path / "tuner.txt")
    monkeypatch.setenv("FEDAVG_TUNE_CACHE", path)
    _lib.call("fa_tune_cache_path", path.encode())
    try:
        N, P, rounds, seed = 13, 300_009, 4, 67
        lay = SlotLayout(P, 1, rounds)
        X = _slots_input(N, P, seed, lay, dev)
        w, sc = _weights(seed, N), _scores(seed, N)
        exp = _expected(seed, N, P, True)
        agg = ShardedAggregator(one_launch="probe")
        key = agg.step_key(X, lay)
        kb = agg.step_key(X.view(torch.bfloat16), lay)
        assert key != kb and key == step_key(agg.ident, "f16", N, lay) and kb == step_key(agg.ident, True, N, lay)
        # a bf16 decision for the same layout: the float16 step does not read it
        _lib.call("fa_step_record", kb.encode(), 1)
        assert agg.step_form(X.view(torch.bfloat16), lay) == "one launch" and agg.step_form(X, lay) is None
        for call in range(ShardedAggregator.PROBE_STEPS + 2):
            settled = agg.step_form(X, lay)
            assert (settled is None) == (call < ShardedAggregator.PROBE_STEPS), (call, settled)
            assert same_bits16(_host(agg.aggregate_slots(X, w, sc, lay)), exp), call
        form = agg.step_form(X, lay)
        assert form in ("one launch", "per round")
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("fedavg-step") and f" {key} " in ln + " "]
        assert lines and " float16 " in lines[-1] and lines[-1].endswith(" one" if form == "one launch" else " per")
        # a fresh aggregator (a later process's) restores it and times nothing
        fresh = ShardedAggregator()
        assert fresh.step_form(X, lay) == form
        calls = []
        real = engine.fold_rounds
        monkeypatch.setattr(engine, "fold_rounds", lambda *a, **k: calls.append(1) or real(*a, **k))
        monkeypatch.setattr(torch.cuda.Event, "elapsed_time", lambda *a: pytest.fail("a probe timed a call"))
        assert same_bits16(_host(fresh.aggregate_slots(X, w, sc, lay)), exp)
        assert len(calls) == (1 if form == "one launch" else 0)
    finally:
        _lib.call("fa_tune_cache_path", session_cache.encode())


def test_aggregate_layers_world1_f16():
    """float16 layers through the sharded per-layer entry: the reference's
    `_aggregate` expression in numpy, layer by layer."""
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    from fedlesscan_amd.sharding import ShardedAggregator
    shapes = [(5, 5, 3), (64,), (), (33, 7)]
    N, seed = 6, 71
    rng = np.random.default_rng(seed)
    params = [[np.asarray(rng.random(s, dtype=np.float32) * 2 - 1).astype(F16) for s in shapes] for _ in range(N)]
    assert all(isinstance(x, np.ndarray) and x.dtype == F16 for row in params for x in row)
    w, sc = _weights(seed, N), _scores(seed, N)
    agg = ShardedAggregator()
    for scores in (None, sc):
        outs = agg.aggregate_layers(params, w, scores)
        with np.errstate(all="ignore"):
            exp = [reduce(np.add, [params[i][li] * w[i] if scores is None else params[i][li] * w[i] * scores[i]
                                   for i in range(N)]) / sum(w) for li in range(len(shapes))]
        _meaningful(np.concatenate([e.reshape(-1) for e in exp]))
        assert len(outs) == len(exp)
        for o, e in zip(outs, exp):
            assert o.dtype == F16 and o.shape == e.shape and same_bits16(o, e)
    mixed = [[x.astype(np.float32) if li == 2 else x for li, x in enumerate(row)] for row in params]
    with pytest.raises(InvalidParameterShapeError):
        agg.aggregate_layers(mixed, w)
    with pytest.raises(InvalidParameterShapeError):
        agg.aggregate_layers(params, [np.float64(w[0])] + w[1:])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, N, P, rounds, seed, q):
    import torch as T
    import torch.distributed as dist
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    T.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = T.device("cuda", 0)
        lay = SlotLayout(P, world, rounds)
        X = _slots_input(N, P, seed, lay, dev, rank)
        agg = ShardedAggregator(one_launch=True)
        fulls = [agg.aggregate_slots(X, _weights(seed, N), _scores(seed, N), lay) for _ in range(3)]
        assert all(f.dtype == T.float16 and f.numel() == P for f in fulls)
        outs = [f.view(T.int16).cpu().numpy().tobytes() for f in fulls]
        assert all(o == outs[0] for o in outs)
        q.put((rank, outs[0]))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_f16():
    """Two freshly spawned ranks share the GPU over gloo (the default exchange,
    host-staged here), each folding its slots with the one-launch float16
    step: both models have numpy's bits."""
    import torch.multiprocessing as mp
    N, P, rounds, seed, world = 17, 20011, 3, 73, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, N, P, rounds, seed, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=100) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    exp = _expected(seed, N, P, True)
    for r in range(world):
        assert same_bits16(np.frombuffer(got[r], dtype=F16), exp), r
