"""The float64 sharded step without a GPU: the new symbols, the step forms'
names, the layout / key helpers, f64_factors, and ShardedAggregator over gloo
on CPU ranks with a literal numpy float64 fold (the slots, the model and every
exchange stay float64)."""
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

F64 = np.float64
FORMS = ["f64_step_bal_u8c4", "f64_step_sd_u8c4_p75", "f64_step_static_u8c4"]


def _numpy_fold(X, w, sc=None, total=None):
    """reduce(np.add, [x_i * n_i (* s_i)]) / total on float64 rows."""
    with np.errstate(all="ignore"):
        terms = [X[i] * w[i] if sc is None else X[i] * w[i] * sc[i] for i in range(len(X))]
        out = reduce(np.add, terms) / (sum(w) if total is None else total)
    assert out.dtype == F64
    return out


def _same_bits64(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != F64 or b.dtype != F64 or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~na]))


def _meaningful(exp) -> None:
    e = np.asarray(exp, F64).ravel()
    assert np.isfinite(e).all() and (np.abs(e) >= 2.0 ** -20).any()


def _rows(seed, N, P):
    return np.random.default_rng(seed).random((N, P)) * 2 - 1


def _weights(seed, N):
    return [int(v) for v in np.random.default_rng(seed + 1000).integers(1, 6, N)]


def _scores(seed, N):
    return [float(v) for v in 1.0 - np.random.default_rng(seed + 2000).random(N)]


def _f64_fold(X, w, s=None, out=None, total=None, want_bf16=False, out_bf16=None):
    """engine.fold_stacked's contract for float64 rows, by numpy (CPU ranks)."""
    assert X.dtype == torch.float64 and out_bf16 is None and not want_bf16
    res = torch.from_numpy(_numpy_fold(np.ascontiguousarray(X.numpy()), w, s, total))
    if out is not None:
        assert out.dtype == torch.float64
        out.copy_(res)
        return out
    return res


# ---------------------------------------------------------------------------
# symbols and names
# ---------------------------------------------------------------------------
def test_abi_and_new_symbols():
    assert _lib.ABI_VERSION == 7 and _lib.load().fa_abi_version() == 7
    L, B = _lib.load(), _lib.load_bench()
    for name in ("fa_fedavg_f64_rounds", "fa_rounds_form_f64"):
        assert name in _lib.header_functions() and name in _lib._PROTOS and hasattr(L, name), name
    for name in ("fa_num_step_forms_f64", "fa_step_form_name_f64", "fa_fedavg_f64_rounds_form"):
        assert name in _lib._BENCH_PROTOS and hasattr(B, name), name
    with open(os.path.join(os.path.dirname(_lib.PKG), "include", "fedavg_hip_bench.h")) as f:
        text = f.read()
    assert all(n + "(" in text for n in ("fa_num_step_forms_f64", "fa_step_form_name_f64",
                                         "fa_fedavg_f64_rounds_form"))


def test_step_form_names():
    L, B = _lib.load(), _lib.load_bench()
    names = [B.fa_step_form_name_f64(f).decode() for f in range(B.fa_num_step_forms_f64())]
    assert names == FORMS
    assert L.fa_rounds_form_f64().decode() in names[:2]  # the policy: the balanced or the pooled form
    assert B.fa_step_form_name_f64(-1) == b"" and B.fa_step_form_name_f64(len(names)) == b""
    # the other dtypes' tables are what they were
    old = [B.fa_step_form_name(f).decode() for f in range(B.fa_num_step_forms())]
    assert old and all(n.startswith(("bf16", "f32")) for n in old)
    assert [B.fa_step_form_name_f16(f).decode() for f in range(B.fa_num_step_forms_f16())] == \
        ["f16_step_bal_u8c4", "f16_step_static_u8c4"]


def test_null_state_is_an_argument_error():
    L, B = _lib.load(), _lib.load_bench()
    assert L.fa_fedavg_f64_rounds(None, None, 1, 2, None, None, 1.0, None, 1, None, None, None) == _lib.FA_ERR_ARG
    assert B.fa_fedavg_f64_rounds_form(None, 0, None, 1, 2, None, None, 1.0, None, 1, None, None, None) == \
        _lib.FA_ERR_ARG


# ---------------------------------------------------------------------------
# layout and keys
# ---------------------------------------------------------------------------
def test_layout_quantum_and_keys():
    for P in (25_000_000, 100_000_000, 10007):
        assert overlap_layout(P, 8, "f64").widths == overlap_layout(P, 8, "f32").widths
    assert pass_quantum(256, "f64") == 524288
    assert pass_quantum(256, "f32") == 1_048_576 and pass_quantum(256, "f16") == 2_097_152
    lay = SlotLayout(100_000_000, 8, 4)
    w = ",".join(map(str, lay.widths))
    kb, kf = step_key("gfx950:256", True, 200, lay), step_key("gfx950:256", False, 200, lay)
    kh = step_key("gfx950:256", "f16", 200, lay)
    kd = step_key("gfx950:256", "f64", 200, lay)
    assert kd == f"gfx950:256 float64 8 256 100000000 {w}"
    assert kd not in (kb, kf, kh) and kd == step_key("gfx950:256", False, 200, lay, dtype="f64")
    with pytest.raises(ValueError):
        step_key("gfx950:256", "f64", 200, lay, "peer_copy")
    # the library takes the float64 key; the short token stays malformed
    L = _lib.load()
    assert L.fa_step_lookup(kd.encode()) in (-1, 0, 1)
    assert L.fa_step_lookup(kd.replace("float64", "f64").encode()) == -2
    assert L.fa_step_lookup(kd.replace("float64", "float64.peer").encode()) == -2
    agg = ShardedAggregator(fold=_f64_fold, device_ident="gfx950:256")
    for dt, k in ((torch.float64, kd), (torch.float16, kh), (torch.bfloat16, kb), (torch.float32, kf)):
        assert agg.step_key(torch.zeros((200, lay.local_width), dtype=dt), lay) == k


def test_f64_factors():
    from fedlesscan_amd import engine
    f = engine.f64_factors([1, 2, 3], [0.5, 1.0, 0.25])
    assert f.a.dtype == F64 and f.s.dtype == F64 and type(f.div) is F64 and float(f.div) == 6.0
    assert f.a.tolist() == [1.0, 2.0, 3.0] and f.s.tolist() == [0.5, 1.0, 0.25]
    for w in ([np.float64(1.5), 2, 3], [np.float32(0.1), 2, 3], [np.int64(4), np.int64(2), 3]):
        g = engine.f64_factors(w)
        assert g is not None and g.a.dtype == F64 and g.s is None, w
        assert g.a.tolist() == [float(v) for v in w] and float(g.div) == float(sum(w))
    g = engine.f64_factors([1, 2], [np.float32(0.1), 1.0], total=np.float64(3))
    assert g is not None and g.s[0] == float(np.float32(0.1))
    if np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant:  # wider than double on this host
        assert engine.f64_factors([np.longdouble(1), 2]) is None
        assert engine.f64_factors([1, 2], [np.longdouble(1), 1.0]) is None
    assert engine.f64_factors([np.complex128(1), 2]) is None


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
        agg = ShardedAggregator(fold=_f64_fold)
        lay = SlotLayout(P, world, rounds)
        Xh = _rows(seed, N, P)
        X = torch.zeros((N, lay.local_width), dtype=torch.float64)
        for k, (lo, hi) in enumerate(lay.slots(rank)):
            if hi > lo:
                X[:, lay.offset(k):lay.offset(k) + hi - lo] = torch.from_numpy(Xh[:, lo:hi])
        full = agg.aggregate_slots(X, _weights(seed, N), _scores(seed, N), lay)
        assert full.dtype == torch.float64 and full.numel() == P
        q.put((rank, full.numpy().tobytes()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,P,rounds", [(2, 10007, 3), (3, 5000, 2)])
def test_f64_slot_gather_gloo_matches_numpy(world, P, rounds):
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
        assert _same_bits64(np.frombuffer(got[r], dtype=F64), exp), r
