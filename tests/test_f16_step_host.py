"""The float16 sharded step without a GPU: the new symbols, the step forms'
names, the layout / key helpers, and ShardedAggregator over gloo on CPU ranks
with a literal numpy float16 fold (the slots, the model and every exchange
stay float16)."""
import os
import socket
from functools import reduce

import numpy as np
import pytest

from fedlesscan_amd import _lib

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from fedlesscan_amd.sharding import (ShardedAggregator, SlotLayout, overlap_layout, pass_quantum,  # noqa: E402
                                     step_key)

F16 = np.float16


def _numpy_fold(X, w, sc=None, total=None):
    """reduce(np.add, [x_i * n_i (* s_i)]) / total on float16 rows with
    Python-number factors: numpy keeps every operation float16."""
    with np.errstate(all="ignore"):
        terms = [X[i] * w[i] if sc is None else X[i] * w[i] * sc[i] for i in range(len(X))]
        out = reduce(np.add, terms) / (sum(w) if total is None else total)
    assert out.dtype == F16
    return out


def _same_bits16(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F16 or b.dtype != F16 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~na]))


def _meaningful(exp) -> None:
    e = np.asarray(exp, F16).ravel()
    assert np.isfinite(e).all() and (np.abs(e.astype(np.float32)) >= 2.0 ** -14).any()


def _rows(seed, N, P):
    rng = np.random.default_rng(seed)
    return (rng.random((N, P), dtype=np.float32) * 2 - 1).astype(F16)


def _weights(seed, N):
    return [int(v) for v in np.random.default_rng(seed + 1000).integers(1, 6, N)]


def _scores(seed, N):
    return [float(v) for v in 1.0 - np.random.default_rng(seed + 2000).random(N)]


def _f16_fold(X, w, s=None, out=None, total=None, want_bf16=False, out_bf16=None):
    """engine.fold_stacked's contract for float16 rows, by numpy (CPU ranks)."""
    assert X.dtype == torch.float16 and out_bf16 is None and not want_bf16
    res = torch.from_numpy(_numpy_fold(np.ascontiguousarray(X.numpy()), w, s, total))
    if out is not None:
        assert out.dtype == torch.float16
        out.copy_(res)
        return out
    return res


# ---------------------------------------------------------------------------
# symbols and names
# ---------------------------------------------------------------------------
def test_abi_and_new_symbols():
    assert _lib.ABI_VERSION == 7 and _lib.load().fa_abi_version() == 7
    L, B = _lib.load(), _lib.load_bench()
    for name in ("fa_fedavg_f16_rounds", "fa_rounds_form_f16"):
        assert name in _lib.header_functions() and name in _lib._PROTOS and hasattr(L, name), name
    for name in ("fa_num_step_forms_f16", "fa_step_form_name_f16", "fa_fedavg_f16_rounds_form"):
        assert name in _lib._BENCH_PROTOS and hasattr(B, name), name
    with open(os.path.join(os.path.dirname(_lib.PKG), "include", "fedavg_hip_bench.h")) as f:
        text = f.read()
    assert all(n + "(" in text for n in ("fa_num_step_forms_f16", "fa_step_form_name_f16",
                                         "fa_fedavg_f16_rounds_form"))


def test_step_form_names():
    L, B = _lib.load(), _lib.load_bench()
    names = [B.fa_step_form_name_f16(f).decode() for f in range(B.fa_num_step_forms_f16())]
    assert names == ["f16_step_bal_u8c4", "f16_step_static_u8c4"]
    assert L.fa_rounds_form_f16().decode() in names
    assert B.fa_step_form_name_f16(-1) == b"" and B.fa_step_form_name_f16(len(names)) == b""
    old = [B.fa_step_form_name(f).decode() for f in range(B.fa_num_step_forms())]
    assert old and all(n.startswith(("bf16", "f32")) for n in old)
    assert L.fa_rounds_form(1).decode().startswith("bf16") and L.fa_rounds_form(0).decode().startswith("f32")


def test_null_state_is_an_argument_error():
    L, B = _lib.load(), _lib.load_bench()
    assert L.fa_fedavg_f16_rounds(None, None, 1, 8, None, None, 0x3C00, None, 1, None, None, None) == _lib.FA_ERR_ARG
    assert B.fa_fedavg_f16_rounds_form(None, 0, None, 1, 8, None, None, 0x3C00, None, 1, None, None, None) == \
        _lib.FA_ERR_ARG


# ---------------------------------------------------------------------------
# layout and keys
# ---------------------------------------------------------------------------
def test_layout_quantum_and_keys():
    assert overlap_layout(100_000_000, 8, "f16").widths == overlap_layout(100_000_000, 8, "bf16").widths
    assert pass_quantum(256, "f16") == 2_097_152
    lay = SlotLayout(100_000_000, 8, 4)
    w = ",".join(map(str, lay.widths))
    kb, kf = step_key("gfx950:256", True, 200, lay), step_key("gfx950:256", False, 200, lay)
    assert kb == f"gfx950:256 bf16 8 256 100000000 {w}"
    assert kf == f"gfx950:256 f32 8 256 100000000 {w}"
    assert step_key("gfx950:256", True, 200, lay, "peer_copy") == f"gfx950:256 bf16.peer 8 256 100000000 {w}"
    kh = step_key("gfx950:256", "f16", 200, lay)
    assert kh not in (kb, kf) and kh == step_key("gfx950:256", False, 200, lay, dtype="f16")
    assert step_key("gfx950:256", "bf16", 200, lay) == kb and step_key("gfx950:256", "f32", 200, lay) == kf
    # the library takes the float16 key, and keeps the three dtypes' decisions apart
    L = _lib.load()
    assert L.fa_step_lookup(kh.encode()) in (-1, 0, 1)
    agg = ShardedAggregator(fold=_f16_fold, device_ident="gfx950:256")
    for dt, k in ((torch.float16, kh), (torch.bfloat16, kb), (torch.float32, kf)):
        assert agg.step_key(torch.zeros((200, lay.local_width), dtype=dt), lay) == k


def test_f16_factors():
    from fedlesscan_amd import engine
    f = engine.f16_factors([1, 2, 3], [0.5, 1.0, 0.25])
    assert f.a.dtype == F16 and f.s.dtype == F16 and type(f.div) is F16 and float(f.div) == 6.0
    assert engine.f16_factors([1, np.float32(2)]) is None and engine.f16_factors([1, 2], [np.float64(1), 1.0]) is None
    big = engine.f16_factors([40000, 40000])  # the divisor rounds to inf, as numpy's
    assert np.isinf(big.div)


# ---------------------------------------------------------------------------
# gloo ranks
# ---------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _slot_worker(rank, world, port, N, P, rounds, seed, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        agg = ShardedAggregator(fold=_f16_fold)
        lay = SlotLayout(P, world, rounds)
        Xh = _rows(seed, N, P)
        X = torch.zeros((N, lay.local_width), dtype=torch.float16)
        for k, (lo, hi) in enumerate(lay.slots(rank)):
            if hi > lo:
                X[:, lay.offset(k):lay.offset(k) + hi - lo] = torch.from_numpy(Xh[:, lo:hi])
        full = agg.aggregate_slots(X, _weights(seed, N), _scores(seed, N), lay)
        assert full.dtype == torch.float16 and full.numel() == P
        q.put((rank, full.numpy().tobytes()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,P,rounds", [(2, 10007, 3), (3, 5000, 2)])
def test_f16_slot_gather_gloo_matches_numpy(world, P, rounds):
    N, seed = 7, 41
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_slot_worker, args=(r, world, port, N, P, rounds, seed, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    exp = _numpy_fold(_rows(seed, N, P), _weights(seed, N), _scores(seed, N))
    _meaningful(exp)
    for r in range(world):
        assert _same_bits16(np.frombuffer(got[r], dtype=F16), exp), r


SHAPES = [(5, 5, 3), (64,), (), (33, 7)]


def _layers(seed, N):
    P = sum(int(np.prod(s)) for s in SHAPES)
    X = _rows(seed, N, P)
    params = []
    for i in range(N):
        row, off = [], 0
        for shp in SHAPES:
            n = int(np.prod(shp))
            row.append(X[i, off:off + n].reshape(shp).copy())
            off += n
        params.append(row)
    return X, params


def test_aggregate_layers_f16_on_the_cpu_device():
    from fedlesscan_amd.aggregator.exceptions import InvalidParameterShapeError
    N, seed = 6, 43
    X, params = _layers(seed, N)
    w, sc = _weights(seed, N), _scores(seed, N)
    agg = ShardedAggregator(fold=_f16_fold)
    outs = agg.aggregate_layers(params, w, sc, device=torch.device("cpu"))
    assert [o.shape for o in outs] == SHAPES and all(o.dtype == F16 for o in outs)
    exp = _numpy_fold(X, w, sc)
    _meaningful(exp)
    assert _same_bits16(np.concatenate([o.reshape(-1) for o in outs]), exp)
    mixed = [[x.astype(np.float32) if li == 1 else x for li, x in enumerate(row)] for row in params]
    with pytest.raises(InvalidParameterShapeError):
        agg.aggregate_layers(mixed, w, sc, device=torch.device("cpu"))
    mixed = [[x.astype(np.float32) if li != 1 else x for li, x in enumerate(row)] for row in params]
    with pytest.raises(InvalidParameterShapeError):
        agg.aggregate_layers(mixed, w, sc, device=torch.device("cpu"))
    with pytest.raises(InvalidParameterShapeError):  # a numpy-scalar weight promotes the float16 layers
        agg.aggregate_layers(params, [np.float32(1)] + w[1:], sc, device=torch.device("cpu"))
