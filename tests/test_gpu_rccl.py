"""The RCCL (torch.distributed "nccl") exchange on the MI355X.

The 8-GPU run belongs to the driver; a one-GPU box cannot hold two RCCL ranks
(RCCL refuses two ranks on one device), so this runs the nccl backend at world
size 1 on cuda:0, in ONE spawned process (RCCL state stays out of the pytest
process): the per-round async all_gather_into_tensor on RCCL's streams, its
overlap with the next round's fold, the bf16-as-uint8 exchange, and the
reference-shaped per-layer entry, all bit-exact against the oracle.
"""
import os
import socket

import numpy as np
import pytest

import golden_cases as G
from fedlesscan_amd import synth

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, SEED = 41, 21
# (dtype, P, rounds, tail): tail < 1 is the short-last-round layout (tail_shares)
CASES = [("f32", 10007, 4, 1.0), ("f32", 262144 + 5, 4, 1.0), ("bf16", 8 * 1000 + 3, 4, 1.0), ("bf16", 65536, 3, 1.0),
         ("f32", 262144 + 5, 4, 0.25), ("bf16", 100003, 4, 0.1)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scores(seed, n):
    return [(r + 1) / 11 for r in synth.round_ids(seed, n, 10, 2)]


def _rccl_worker(port, q):
    import torch as T
    import torch.distributed as dist
    from fedlesscan_amd.sharding import ShardedAggregator, SlotLayout, tail_shares
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    T.cuda.set_device(0)
    dev = T.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        out = {"backend": dist.get_backend()}
        w = synth.cardinalities(SEED, N)
        sc = _scores(SEED, N)
        for dt, P, rounds, tail in CASES:
            lay = SlotLayout(P, 1, rounds, shares=tail_shares(rounds, tail))
            bf16 = dt == "bf16"
            X = T.zeros((N, lay.local_width), dtype=T.int16 if bf16 else T.float32, device=dev)
            for k, (lo, hi) in enumerate(lay.slots(0)):
                if hi > lo:
                    part = (synth.clients_bf16(SEED, N, lo, hi - lo).view(np.int16) if bf16
                            else synth.clients_f32(SEED, N, lo, hi - lo))
                    X[:, lay.offset(k):lay.offset(k) + hi - lo] = T.from_numpy(part).to(dev)
            for scored in (False, True):
                # one launch per step (each round's all-gather behind its wait) and one launch per round
                for one in (True, False):
                    agg = ShardedAggregator(one_launch=one)
                    full = agg.aggregate_slots(X.view(T.bfloat16) if bf16 else X, w, sc if scored else None, lay)
                    out[(dt, P, tail, scored, one)] = full.view(T.int16 if bf16 else T.int32).cpu().numpy().tobytes()
                # "probe": both forms timed over the first calls, then the faster kept and recorded
                agg = ShardedAggregator(one_launch="probe")
                runs = set()
                for _ in range(ShardedAggregator.PROBE_STEPS + 1):
                    full = agg.aggregate_slots(X.view(T.bfloat16) if bf16 else X, w, sc if scored else None, lay)
                    runs.add(full.view(T.int16 if bf16 else T.int32).cpu().numpy().tobytes())
                assert len(runs) == 1 and agg.step_form(X.view(T.bfloat16) if bf16 else X, lay) is not None
                out[(dt, P, tail, scored, "probe")] = runs.pop()
                # "auto" (the default) in a fresh aggregator: the recorded form, no probe
                agg = ShardedAggregator()
                assert agg.step_form(X.view(T.bfloat16) if bf16 else X, lay) is not None
                full = agg.aggregate_slots(X.view(T.bfloat16) if bf16 else X, w, sc if scored else None, lay)
                out[(dt, P, tail, scored, "auto")] = full.view(T.int16 if bf16 else T.int32).cpu().numpy().tobytes()
        m = G.manifest()["f32_small"]
        layers = ShardedAggregator().aggregate_layers(G.parameters("f32_small"), m["weights"])
        out["layers"] = [np.array(a) for a in layers]
        q.put(out)
    finally:
        dist.destroy_process_group()


def test_rccl_world1_slots_and_layers_bit_exact():
    import torch.multiprocessing as mp
    from oracle import fedavg_oracle as O
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    got = q.get(timeout=100)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert got["backend"] == "nccl"
    w = synth.cardinalities(SEED, N)
    sc = _scores(SEED, N)
    for dt, P, _, tail in CASES:
        for scored in (False, True):
            s = sc if scored else None
            for one in (True, False, "probe", "auto"):
                key = (dt, P, tail, scored, one)
                if dt == "bf16":
                    _, exp = O.fedavg_stacked_bf16(synth.clients_bf16(SEED, N, 0, P), w, s)
                    assert np.array_equal(np.frombuffer(got[key], dtype=np.uint16), exp), key
                else:
                    exp = O.fedavg_stacked(synth.clients_f32(SEED, N, 0, P), w, s)
                    assert np.array_equal(np.frombuffer(got[key], dtype=np.uint32), exp.view(np.uint32)), key
    exp_layers = G.expected("f32_small", "fedavg")
    assert len(got["layers"]) == len(exp_layers)
    assert all(a.shape == b.shape and G.same_bits(a, b) for a, b in zip(got["layers"], exp_layers))


@pytest.mark.parametrize("impl,extra", [("product", []), ("product", ["--check", "deferred"]),
                                        ("product", ["--exchange", "peer_copy", "--step-mode", "one"]),
                                        ("loop", [])])
@pytest.mark.parametrize("config", ["c4", "c3"])
def test_bench_times_the_shipped_class(config, impl, extra):
    """bench.py under a one-rank nccl group (--rccl-world1): the default
    --step-impl product times ShardedAggregator.aggregate_slots itself (VERDICT
    r5 next #1), --step-impl loop bench.py's own step; both reassemble the
    model the per-round folds give (gather_check), with no round-wait timeout,
    and a bf16 step stores only the bf16 copy (ABI 5)."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    params = "2000000" if config == "c4" else "500000"
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--rccl-world1", "--config", config, "--params", params,
           "--clients", "64", "--steps", "3", "--warmup", "5", "--full", "--no-cpu-baseline", "--step-impl", impl,
           *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["gather_check"] is True and line["round_wait_timeouts"] == 0
    cfg = line["config"]
    assert cfg["step_impl"].startswith("product: ShardedAggregator") == (impl == "product")
    if impl == "product":
        assert ("check='deferred'" in cfg["step_impl"]) == ("deferred" in extra)
    if config == "c4":
        assert cfg["outputs"].startswith("RNE bf16 only")
        assert line["roofline"]["bytes_per_launch"] == 64 * line["config"]["params_per_gpu"] * 2 + \
            line["config"]["params_per_gpu"] * 2
    if "peer_copy" in extra:
        assert cfg["exchange"] == "peer_copy"
