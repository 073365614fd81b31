"""float64 models through ShardedAggregator on the GPU: the one-launch step
(fa_fedavg_f64_rounds), per-round launches (fa_fedavg_f64 with staged factors),
the probe and its record, the refusals, and two ranks on one GPU over gloo.
The expected model is numpy's literal float64 fold,
`reduce(np.add, [x_i * n_i (* s_i)]) / sum(n)`, bit for bit (NaN by position);
weights 1..5 unless a test says otherwise."""
import os
import socket
import time
from functools import reduce

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F64 = np.float64


def _numpy_fold(X, w, sc=None, total=None):
    with np.errstate(all="ignore"):
        terms = [X[i] * w[i] if sc is None else X[i] * w[i] * sc[i] for i in range(len(X))]
        out = reduce(np.add, terms) / (sum(w) if total is None else total)
    assert out.dtype == F64
    return out


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F64 or b.dtype != F64 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~na]))


def _meaningful(exp) -> None:
    e = np.asarray(exp, F64).ravel()
    assert np.isfinite(e).all() and (np.abs(e) >= 2.0 ** -20).any()
    assert (e.view(np.uint64) & np.uint64(0xFFFFFFF)).any()  # the low mantissa bits are in play


def _rows(seed, N, lo, n):
    """Columns [lo, lo + n) of the seed's [N, *] float64 clients (a column's
    values depend on the seed and the column only, so ranks agree); 53 random
    bits in (-4/3, 4/3), so every mantissa bit is filled."""
    cols = np.arange(lo, lo + n, dtype=np.uint64)[None, :]
    rows = np.arange(N, dtype=np.uint64)[:, None]
    h = cols * np.uint64(0x9E3779B97F4A7C15) + rows * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(seed)
    h = (h ^ (h >> np.uint64(29))) * np.uint64(0xBF58476D1CE4E5B9)
    u = (h >> np.uint64(11)).astype(F64) / F64(1 << 53)
    return (u * 2 - 1) * (1.0 + 1.0 / 3.0)


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
    X = torch.zeros((N, lay.local_width), dtype=torch.float64, device=dev)
    for k, (lo, hi) in enumerate(lay.slots(rank)):
        if hi > lo:
            X[:, lay.offset(k):lay.offset(k) + hi - lo] = torch.from_numpy(_rows(seed, N, lo, hi - lo)).to(dev)
    return X


def _misaligned(X):
    """The same rows 8 bytes off 16-B alignment, at an odd pitch."""
    N, W = X.shape
    base = torch.empty(N * (W + 1) + 1, dtype=X.dtype, device=X.device)
    V = base[1:].view(N, W + 1)[:, :W]
    V.copy_(X)
    assert V.data_ptr() % 16 != 0 and V.stride(0) % 2 != 0
    return V


def _host(full) -> np.ndarray:
    return full.cpu().numpy()


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("one_launch", [True, False, "auto"])
@pytest.mark.parametrize("P,rounds", [(8003, 2), (65536, 4), (300001, 8)])
def test_slots_world1_f64(P, rounds, one_launch, scored):
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
    assert full.dtype == torch.float64 and full.numel() == P
    exp = _expected(seed, N, P, scored)
    assert same_bits(_host(full), exp)
    out = torch.zeros(lay.padded_total, dtype=torch.float64, device=dev)
    again = agg.aggregate_slots(X, w, sc, lay, out=out)
    assert again.data_ptr() == out.data_ptr() and same_bits(_host(again), exp)
    for dt in (torch.float32, torch.float16):
        with pytest.raises(ValueError):
            agg.aggregate_slots(X, w, sc, lay, out=torch.zeros(lay.padded_total, dtype=dt, device=dev))
    # the unsloted entry: one fold, one gather
    if rounds == 2:
        whole = torch.from_numpy(_rows(seed, N, 0, P)).to(dev)
        got = agg.aggregate(whole, w, sc, P=P)
        assert got.dtype == torch.float64 and same_bits(_host(got), exp)


def test_engine_fold_rounds_and_fold_staged_f64():
    """engine.fold_rounds on float64 rows: a tensor out, a raw address with its
    capacity, factors given or rounded here, np.float64 weights; fold_staged
    with the staged doubles; out_bf16, outputs of another dtype and factors of
    another dtype are refused."""
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
    out = torch.zeros(W, dtype=torch.float64, device=dev)
    engine.fold_rounds(X, w, sc, offs, out=out)
    assert same_bits(_host(out)[:P], exp)
    f = engine.f64_factors(w, sc)
    raw = torch.zeros(W, dtype=torch.float64, device=dev)
    engine.fold_rounds(X, w, sc, offs, out=raw.data_ptr(), capacity=W, factors=f)
    assert same_bits(_host(raw)[:P], exp)
    with pytest.raises(ValueError):
        engine.fold_rounds(X, w, sc, offs, out=raw.data_ptr(), capacity=W - 1)
    with pytest.raises(InvalidParameterShapeError, match="out_bf16"):
        engine.fold_rounds(X, w, sc, offs, out_bf16=torch.zeros(W, dtype=torch.bfloat16, device=dev))
    with pytest.raises(ValueError):
        engine.fold_rounds(X, w, sc, offs, out=torch.zeros(W, dtype=torch.float32, device=dev))
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_rounds(X, w, sc, offs, out=out, factors=engine.f32_factors(w, sc))
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_rounds(X, [np.complex128(w[0])] + w[1:], sc, offs, out=out)
    sf = engine.StagedFactors(f, dev)
    assert sf.dtype == F64 and type(sf.div) is float and sf.div == float(sum(w))
    assert engine.StagedFactors(engine.f32_factors(w, sc), dev).dtype == np.float32
    staged = torch.zeros(W, dtype=torch.float64, device=dev)
    assert engine.fold_staged(X, sf, out=staged) is staged
    assert same_bits(_host(staged)[:P], exp)
    with pytest.raises(ValueError):
        engine.fold_staged(X, sf, out=torch.zeros(W, dtype=torch.float32, device=dev))
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_staged(X, engine.StagedFactors(engine.f32_factors(w, sc), dev), out=staged)
    with pytest.raises(InvalidParameterShapeError):
        engine.fold_staged(X.to(torch.float32), sf, out=torch.zeros(W, dtype=torch.float32, device=dev))
    # numpy-scalar weights that keep the fold float64: fractional np.float64, np.float32 and np.int64
    wn = [np.float64(v) + np.float64(0.1) for v in w[:5]] + [np.float32(v) / np.float32(3) for v in w[5:9]] + \
        [np.int64(v) for v in w[9:]]
    expn = _numpy_fold(_rows(seed, N, 0, P), wn, sc)
    _meaningful(expn)
    assert not same_bits(expn, exp)
    out.zero_()
    engine.fold_rounds(X, wn, sc, offs, out=out)
    assert same_bits(_host(out)[:P], expn)
    staged.zero_()
    engine.fold_staged(X, engine.StagedFactors(engine.f64_factors(wn, sc), dev), out=staged)
    assert same_bits(_host(staged)[:P], expn)


def test_odd_pitch_warns_and_folds_an_aligned_copy():
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout
    dev = torch.device("cuda", 0)
    N, P, seed = 13, 65536, 61
    lay = SlotLayout(P, 1, 4)
    V = _misaligned(_slots_input(N, P, seed, lay, dev))
    w, sc = _weights(seed, N), _scores(seed, N)
    with pytest.warns(RuntimeWarning, match="aligned copy"):
        full = ShardedAggregator(one_launch=True).aggregate_slots(V, w, sc, lay)
    exp = _expected(seed, N, P, True)
    assert same_bits(_host(full), exp)
    # per-round launches take the rows as they are
    assert same_bits(_host(ShardedAggregator(one_launch=False).aggregate_slots(V, w, sc, lay)), exp)


def test_refusals():
    """Each an InvalidParameterShapeError before any fold or collective:
    factors that leave float64, the peer-copy exchange, a stream capture."""
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout
    dev = torch.device("cuda", 0)
    N, P, seed = 13, 8003, 61
    lay = SlotLayout(P, 1, 2)
    X = _slots_input(N, P, seed, lay, dev)
    w, sc = _weights(seed, N), _scores(seed, N)
    foreign = [[np.complex128(w[0])] + w[1:]]
    if np.finfo(np.longdouble).nmant > np.finfo(F64).nmant:
        foreign.append([np.longdouble(w[0])] + w[1:])
    for one_launch in (True, False, "auto"):
        agg = ShardedAggregator(one_launch=one_launch)
        for bad in foreign:
            with pytest.raises(InvalidParameterShapeError, match="promote"):
                agg.aggregate_slots(X, bad, sc, lay)
            with pytest.raises(InvalidParameterShapeError, match="promote"):
                agg.aggregate(X[:, :lay.P], bad, sc, P=lay.P)
        with pytest.raises(InvalidParameterShapeError, match="RCCL"):
            ShardedAggregator(one_launch=one_launch, exchange="peer_copy").aggregate_slots(X, w, sc, lay)
        # graph capture: refused up front, whatever the step form
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with pytest.raises(InvalidParameterShapeError, match="capture"):
            with torch.cuda.graph(g, stream=side):
                agg.aggregate_slots(X, w, sc, lay)
        torch.cuda.synchronize()
        # the device folds correctly afterwards
        assert same_bits(_host(agg.aggregate_slots(X, w, sc, lay)), _expected(seed, N, P, True))


def test_probe_settles_and_records_under_the_f64_key(monkeypatch, tmp_path):
    """one_launch="probe" on float64 rows: every call exact, the decision
    recorded under the float64 key in the cache file; bf16 and f32 records for
    the same layout are neither picked up nor changed."""
    from fedlesscan_amd import _lib, engine
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout, step_key
    dev = torch.device("cuda", 0)
    session_cache = os.environ["FEDAVG_TUNE_CACHE"]
    path = str(tmp_path / "tuner.txt")
    monkeypatch.setenv("FEDAVG_TUNE_CACHE", path)
    _lib.call("fa_tune_cache_path", path.encode())
    try:
        N, P, rounds, seed = 13, 100_003, 4, 67
        lay = SlotLayout(P, 1, rounds)
        X = _slots_input(N, P, seed, lay, dev)
        w, sc = _weights(seed, N), _scores(seed, N)
        exp = _expected(seed, N, P, True)
        agg = ShardedAggregator(one_launch="probe")
        key = agg.step_key(X, lay)
        others = {dt: torch.empty((N, 0), dtype=dt, device=dev) for dt in (torch.bfloat16, torch.float32)}
        kb, kf = (agg.step_key(others[dt], lay) for dt in (torch.bfloat16, torch.float32))
        assert len({key, kb, kf}) == 3 and key == step_key(agg.ident, "f64", N, lay)
        assert kb == step_key(agg.ident, True, N, lay) and kf == step_key(agg.ident, False, N, lay)
        # decisions of the other dtypes for the same layout: the float64 step does not read them
        _lib.call("fa_step_record", kb.encode(), 1)
        _lib.call("fa_step_record", kf.encode(), 0)
        assert agg.step_form(others[torch.bfloat16], lay) == "one launch"
        assert agg.step_form(others[torch.float32], lay) == "per round" and agg.step_form(X, lay) is None
        for call in range(ShardedAggregator.PROBE_STEPS + 2):
            settled = agg.step_form(X, lay)
            assert (settled is None) == (call < ShardedAggregator.PROBE_STEPS), (call, settled)
            assert same_bits(_host(agg.aggregate_slots(X, w, sc, lay)), exp), call
        form = agg.step_form(X, lay)
        assert form in ("one launch", "per round")
        with open(path) as f:
            steps = [ln for ln in f.read().splitlines() if ln.startswith("fedavg-step")]
        lines = [ln for ln in steps if f" {key} " in ln + " "]
        assert lines and " float64 " in lines[-1] and lines[-1].endswith(" one" if form == "one launch" else " per")
        # a fresh aggregator (a later process's) restores all three, each its own
        fresh = ShardedAggregator()
        assert fresh.step_form(X, lay) == form
        assert fresh.step_form(others[torch.bfloat16], lay) == "one launch"
        assert fresh.step_form(others[torch.float32], lay) == "per round"
        calls = []
        real = engine.fold_rounds
        monkeypatch.setattr(engine, "fold_rounds", lambda *a, **k: calls.append(1) or real(*a, **k))
        monkeypatch.setattr(torch.cuda.Event, "elapsed_time", lambda *a: pytest.fail("a probe timed a call"))
        assert same_bits(_host(fresh.aggregate_slots(X, w, sc, lay)), exp)
        assert len(calls) == (1 if form == "one launch" else 0)
    finally:
        _lib.call("fa_tune_cache_path", session_cache.encode())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, N, P, rounds, seed, q):
    import warnings

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
        if rank == 1:  # this rank hands over a misaligned view; the others' rows are aligned
            X = _misaligned(X)
        outs = []
        for one_launch in (True, False):  # both step forms
            agg = ShardedAggregator(one_launch=one_launch)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # rank 1's aligned copy
                fulls = [agg.aggregate_slots(X, _weights(seed, N), _scores(seed, N), lay) for _ in range(2)]
            assert all(f.dtype == T.float64 and f.numel() == P for f in fulls)
            outs += [f.cpu().numpy().tobytes() for f in fulls]
        assert all(o == outs[0] for o in outs)
        q.put((rank, outs[0]))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_f64():
    """Two freshly spawned ranks share the GPU over gloo (the default exchange,
    host-staged here), each folding its slots with the one-launch float64 step
    and then with per-round launches, rank 1 from a misaligned view: every
    model on every rank has numpy's bits.  Each child has its own deadline and
    is ended at it."""
    import queue

    import torch.multiprocessing as mp
    N, P, rounds, seed, world = 17, 20011, 3, 73, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, N, P, rounds, seed, q)) for r in range(world)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + 100
    got = {}
    try:
        while (len(got) < world and time.monotonic() < deadline and any(p.is_alive() for p in procs)
               and all(p.exitcode in (None, 0) for p in procs)):
            try:
                r, b = q.get(timeout=0.25)
                got[r] = b
            except queue.Empty:
                pass
        while len(got) < world:  # results put just before the last child left
            try:
                r, b = q.get(timeout=0.25)
                got[r] = b
            except queue.Empty:
                break
        for p in procs:
            p.join(timeout=max(0.0, deadline + 20 - time.monotonic()))
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join()
    assert [p.exitcode for p in procs] == [0] * world and sorted(got) == list(range(world))
    exp = _expected(seed, N, P, True)
    for r in range(world):
        assert same_bits(np.frombuffer(got[r], dtype=F64), exp), r
