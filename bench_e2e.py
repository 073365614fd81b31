#!/usr/bin/env python3
"""End-to-end aggregation rate from host-resident serialized client blobs.

    python bench_e2e.py [--clients N] [--params P] [--reps R] [--bson [--pinned-store]]

What the reference's aggregator function actually does per round
(aggregation.py:87-97, fed_avg_aggregator.py:57-92): N ClientResult objects
holding NPZ blobs -> decode -> weighted fold -> parameters.  Timed here:

  gpu_e2e   FedAvgAggregator.aggregate(ClientResults) of this package: zero-copy
            NPZ views -> pinned chunks -> H2D (copy stream) -> in-order chunked
            HIP fold -> D2H of the result, returned as numpy layers
  cpu_ref   the oracle's restatement of the same call (np.load decode + numpy
            fold on one core), i.e. the reference's own cost on this host
  h2d       pinned host->device copy bandwidth of the same bytes (PCIe bound)

With --bson the results start where the reference keeps them: one BSON
document per client in the (in-memory) result store, as GridFS holds them
(client_daos.py:73).  gpu_e2e then includes the store read and the native BSON
walk (blob stays a view); cpu_ref includes pymongo's bson.decode (the
reference's own codec, client_daos.py:142) before the np.load + numpy fold.
--pinned-store keeps those documents in page-locked memory and turns on the
direct route: the ingest DMAs every layer straight from its document, with no
packing copy (engine.DIRECT_DMA).

--dtype float16 times the same call on float16 NPZ blobs, two routes
interleaved in one process: the streamed route (the native pipe with 2-byte
rows and the chunked binary16 fold) and FEDAVG_F16_STREAM=0 (every row stacked
into one pinned matrix, one H2D, one fold).  It reports each route's median and
min-max, the pinned H2D rate of the same run, whether the two routes agree bit
for bit, and a column sample against numpy's own float16 fold.  --dtype float64
does the same on float64 NPZ blobs: the float64 pipe (8-byte rows, the chunked
float64 fold) against FEDAVG_F64_STREAM=0, with the sample against numpy's
float64 fold.

Rates are input bytes (N * P * 4, * 2 for float16, * 8 for float64) per second.  Results are
compared bit for bit.
Writes one JSON line (rank 0, one GPU).  Not the headline metric: DESIGN.md.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from fedlesscan_amd import FedAvgAggregator, synth  # noqa: E402
from fedlesscan_amd.common.models import (ClientResult, NpzWeightsSerializerConfig,  # noqa: E402
                                          SerializedParameters, WeightsSerializerConfig)

MNIST_LIKE = [(5, 5, 1, 32), (32,), (5, 5, 32, 64), (64,), (1024, 512), (512,), (512, 10), (10,)]


def make_blobs(N, P, seed):
    from oracle import oracle_lib as OL  # fast host generator (test/bench infrastructure)
    from fedlesscan_amd.npz import write_npz  # byte-identical to np.savez, threaded CRC
    blobs = []
    for i in range(N):
        row = OL.synth_f32(seed, 1, P, row0=i)[0]
        # split the row into a few layers like a Keras get_weights() list
        cuts = [0, P // 64, P // 8, P // 2, P]
        layers = [row[cuts[k]:cuts[k + 1]].reshape(-1, 1) if k % 2 else row[cuts[k]:cuts[k + 1]]
                  for k in range(4)]
        blob = write_npz(layers)
        if blob is None:
            f = io.BytesIO()
            np.savez(f, *layers)
            blob = f.getvalue()
        blobs.append(blob)
    return blobs


def check_columns(out, N, P, seed, cards, ncols):
    """GPU result vs the C oracle (the reference op order, fed_avg_aggregator.py:31-41)
    on the first and the last `ncols` columns, regenerated on the host."""
    from oracle import oracle_lib as OL
    flat = np.concatenate([np.asarray(x).reshape(-1) for x in out])
    a = np.array(cards, np.float32)
    div = np.float32(sum(cards))
    ok = True
    for c0 in sorted({0, max(0, P - ncols)}):
        nc = min(ncols, P - c0)
        exp = OL.fedavg_f32(OL.synth_f32(seed, N, nc, col0=c0), a, div)
        ok &= bool(np.array_equal(flat[c0:c0 + nc].view(np.uint32), exp.view(np.uint32)))
    return ok


def results(blobs, cards):
    cfg = WeightsSerializerConfig(type="npz", params=NpzWeightsSerializerConfig())
    return [ClientResult(parameters=SerializedParameters(blob=b, serializer=cfg), cardinality=c)
            for b, c in zip(blobs, cards)]


def make_blobs_f16(N, P, seed):
    """float16 NPZ blobs: rows uniform in [-1, 1), split into layers as make_blobs does."""
    from fedlesscan_amd.common.serialization import NpzWeightsSerializer
    ser, blobs = NpzWeightsSerializer(), []
    cuts = [0, P // 64, P // 8, P // 2, P]
    for i in range(N):
        row = (np.random.default_rng((seed, i)).random(P, dtype=np.float32) * 2 - 1).astype(np.float16)
        blobs.append(ser.serialize([row[cuts[k]:cuts[k + 1]].reshape(-1, 1) if k % 2 else row[cuts[k]:cuts[k + 1]]
                                    for k in range(4)]))
    return blobs


def make_blobs_f64(N, P, seed):
    """float64 NPZ blobs: the synthetic rows widened and scaled by 1 + 1/3, which fills
    the low mantissa bits; split into layers as make_blobs does."""
    from oracle import oracle_lib as OL
    from fedlesscan_amd.common.serialization import NpzWeightsSerializer
    ser, blobs = NpzWeightsSerializer(), []
    cuts = [0, P // 64, P // 8, P // 2, P]
    for i in range(N):
        row = OL.synth_f32(seed, 1, P, row0=i)[0].astype(np.float64) * (1.0 + 1.0 / 3.0)
        blobs.append(ser.serialize([row[cuts[k]:cuts[k + 1]].reshape(-1, 1) if k % 2 else row[cuts[k]:cuts[k + 1]]
                                    for k in range(4)]))
    return blobs


def same_bits(a, b, bits=np.uint16) -> bool:
    """Equal NaN positions, equal bit patterns elsewhere (the float16 / float64 folds' contract)."""
    na, nb = np.isnan(a), np.isnan(b)
    return bool(a.shape == b.shape and np.array_equal(na, nb) and
                np.array_equal(a.view(bits)[~na], b.view(bits)[~na]))


def main_streamed_vs_materialised(a):
    """The float16 / float64 comparison: streamed route against FEDAVG_F16_STREAM=0 /
    FEDAVG_F64_STREAM=0, interleaved."""
    from fedlesscan_amd import engine
    from fedlesscan_amd.ingest import NativeStreamingFold
    from fedlesscan_amd.npz import read_layers
    from oracle import fedavg_oracle as O  # checker only
    N, P = a.clients, a.params
    f64 = a.dtype == "float64"
    np_dt, tdt, esz = (np.float64, torch.float64, 8) if f64 else (np.float16, torch.float16, 2)
    ubits = np.uint64 if f64 else np.uint16
    switch = "FEDAVG_F64_STREAM" if f64 else "FEDAVG_F16_STREAM"
    t0 = time.time()
    if f64:
        blobs, cards = make_blobs_f64(N, P, a.seed), synth.cardinalities(a.seed, N)
    else:
        blobs = make_blobs_f16(N, P, a.seed)
        cards = [int(v) for v in np.random.default_rng(a.seed + 1000).integers(1, 41, N)]  # total < 65504: finite
    gen_s = time.time() - t0
    in_bytes = N * P * esz
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    routes = {"streamed": "1", "materialised": "0"}

    def one_round(flag):
        os.environ[switch] = flag
        crs = results(blobs, cards)
        t0 = time.perf_counter()
        out, _ = FedAvgAggregator().aggregate(crs, None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for flag in routes.values():  # warm up both routes (pinned allocations, library load, the pipe)
        one_round(flag)
    ts = {k: [] for k in routes}
    outs = {}
    counted = {}
    for _ in range(a.reps):
        for k, flag in routes.items():
            r0, g0 = NativeStreamingFold.stats["rows"], engine.stats["stacked_groups"]
            dt, outs[k] = one_round(flag)
            counted[k] = {"pipe_rows": NativeStreamingFold.stats["rows"] - r0,
                          "stacked_groups": engine.stats["stacked_groups"] - g0}
            ts[k].append(dt)
    os.environ.pop(switch, None)
    flat = {k: np.concatenate([np.asarray(x).reshape(-1) for x in v]) for k, v in outs.items()}
    t0 = time.perf_counter()
    for b in blobs:
        read_layers(b)
    t_decode = time.perf_counter() - t0
    host = torch.empty(min(in_bytes // esz, (1 << 30) // esz), dtype=tdt, pin_memory=True)
    dbuf = torch.empty_like(host, device=dev)
    dbuf.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        dbuf.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    h2d_gbs = 3 * host.numel() * esz / (time.perf_counter() - t0) / 1e9
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    spread = max(ts["materialised"]) - min(ts["materialised"])
    res = {
        "metric": f"end-to-end aggregation of {a.dtype} NPZ blobs, streamed route vs {switch}=0",
        "dtype": a.dtype, "clients": N, "params": P, "input_bytes": in_bytes, "reps": a.reps,
        "gen_s": round(gen_s, 1),
    }
    for k in routes:
        res[k] = {"median_s": round(med[k], 4), "min_s": round(min(ts[k]), 4), "max_s": round(max(ts[k]), 4),
                  "median_gbs": round(in_bytes / med[k] / 1e9, 2), **counted[k]}
    res["speedup_streamed_vs_materialised"] = round(med["materialised"] / med["streamed"], 2)
    res["materialised_spread_s"] = round(spread, 4)
    res["bar_streamed_no_slower_than_spread"] = bool(med["streamed"] - med["materialised"] <= spread)
    res["h2d_pinned_gbs"] = round(h2d_gbs, 1)
    res["streamed_fraction_of_h2d"] = round(in_bytes / med["streamed"] / 1e9 / h2d_gbs, 3)
    res["decode_views_s"] = round(t_decode, 4)
    res["stream_chunk_mb"] = int(os.environ.get("FEDAVG_STREAM_CHUNK_MB", "32"))
    res["routes_bit_equal"] = same_bits(flat["streamed"], flat["materialised"], ubits)
    # numpy's own fold in the rows' dtype on the first and the last K columns
    K = min(a.check_cols or 4096, P)
    ok = True
    for c0 in sorted({0, P - K}):
        X = np.stack([np.concatenate([np.asarray(x).reshape(-1) for x in read_layers(b)])[c0:c0 + K] for b in blobs])
        with np.errstate(all="ignore"):
            exp = O.fedavg_stacked(X, cards)
        ok &= exp.dtype == np_dt and same_bits(flat["streamed"][c0:c0 + K], exp, ubits)
    res["bit_exact_column_sample"] = bool(ok)
    res["column_sample"] = f"first and last {K} columns vs numpy's {a.dtype} fold"
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["float32", "float16", "float64"], default="float32",
                    help="float16 / float64: the streamed route against FEDAVG_F16_STREAM=0 / FEDAVG_F64_STREAM=0, "
                         "interleaved (NPZ blobs, one GPU)")
    ap.add_argument("--clients", type=int, default=100)
    ap.add_argument("--params", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--check-cols", type=int, default=0,
                    help="with --no-cpu: check the first and last K output columns against the C oracle")
    ap.add_argument("--bson", action="store_true", help="start from BSON documents in the result store")
    ap.add_argument("--pinned-store", action="store_true", help="with --bson: documents in page-locked memory")
    ap.add_argument("--devices", default="",
                    help="comma-separated GPU ordinals for the multi-GPU drop-in (FedAvgAggregator(devices=...)); "
                         "'all' = every visible GPU; a GPU may repeat (buckets sharing one GPU)")
    a = ap.parse_args()
    if a.dtype in ("float16", "float64"):
        if a.bson or a.pinned_store or a.devices:
            ap.error(f"--dtype {a.dtype} measures NPZ blobs on one GPU")
        return main_streamed_vs_materialised(a)
    from oracle import fedavg_oracle as O  # checker + CPU reference timing only
    N, P = a.clients, a.params
    t0 = time.time()
    blobs = make_blobs(N, P, a.seed)
    cards = synth.cardinalities(a.seed, N)
    gen_s = time.time() - t0
    in_bytes = N * P * 4
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    store = None
    if a.pinned_store:
        from fedlesscan_amd import engine
        engine.DIRECT_DMA = True
    if a.bson or a.pinned_store:
        from fedlesscan_amd.store import InMemoryClientResultStore
        store = InMemoryClientResultStore(pinned=a.pinned_store)
        for i, cr in enumerate(results(blobs, cards)):
            store.save("bench", 1, f"client-{i}", cr)

    devices = None
    if a.devices:
        devices = "all" if a.devices == "all" else [int(x) for x in a.devices.split(",")]

    def one_round(crs):
        if store is not None:
            agg = FedAvgAggregator(devices=devices)
            feats, it = agg.select_aggregation_candidates(store, "bench", 1)
            return agg.aggregate(list(it), feats)
        return FedAvgAggregator(devices=devices).aggregate(crs, None)

    # warm up the pipeline (pinned allocations, library load)
    FedAvgAggregator(devices=devices).aggregate(results(blobs[: min(N, 4)], cards[: min(N, 4)]), None)
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(a.reps):
        crs = None if store is not None else results(blobs, cards)
        t0 = time.perf_counter()
        out, _ = one_round(crs)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t_gpu = sorted(ts)[len(ts) // 2]
    from fedlesscan_amd.ingest import NATIVE_INGEST, NativeStreamingFold, StreamingFold
    routes = dict(StreamingFold.stats)
    routes["native_pipe_rows"] = NativeStreamingFold.stats["rows"]

    # decode-only (zero-copy views) and pinned H2D of the same bytes
    from fedlesscan_amd.npz import read_layers
    t0 = time.perf_counter()
    for b in blobs:
        read_layers(b)
    t_decode = time.perf_counter() - t0
    host = torch.empty(min(in_bytes // 4, 1 << 28), dtype=torch.float32, pin_memory=True)
    dbuf = torch.empty_like(host, device=dev)
    dbuf.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        dbuf.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    h2d_gbs = 3 * host.numel() * 4 / (time.perf_counter() - t0) / 1e9

    res = {
        "metric": "end-to-end aggregation GB/s from host NPZ blobs (not the headline)",
        "source": ("BSON documents in a page-locked result store" if a.pinned_store else
                   "BSON documents in the result store" if a.bson else "ClientResult objects holding NPZ blobs"),
        "clients": N, "params": P, "input_bytes": in_bytes, "gen_s": round(gen_s, 1),
        "gpu_e2e_s": round(t_gpu, 4), "gpu_e2e_gbs": round(in_bytes / t_gpu / 1e9, 2),
        "gpu_e2e_min_s": round(min(ts), 4), "gpu_e2e_max_s": round(max(ts), 4),
        "stream_chunk_mb": int(os.environ.get("FEDAVG_STREAM_CHUNK_MB", "32")),
        "stream_slots": int(os.environ.get("FEDAVG_STREAM_SLOTS", "0")) or None,
        "ingest": "native pipe (fa_ingest_*)" if NATIVE_INGEST and not a.pinned_store else "python StreamingFold",
        "decode_views_s": round(t_decode, 4), "h2d_pinned_gbs": round(h2d_gbs, 1),
        "ingest_rows": routes,
        "devices": a.devices or "current GPU",
    }
    if a.no_cpu and a.check_cols > 0:
        t0 = time.perf_counter()
        res["bit_exact_column_sample"] = check_columns(out, N, P, a.seed, cards, a.check_cols)
        res["column_sample"] = f"first and last {min(a.check_cols, P)} columns vs the C oracle"
        res["check_s"] = round(time.perf_counter() - t0, 1)
    if not a.no_cpu:
        if store is not None:
            import bson  # pymongo's codec: the reference's own decode (CPU leg only)
            files = [store._files[d["file_id"]] for d in store._docs]
            files = [f if isinstance(f, bytes) else bytes(f) for f in files]  # untimed: GridFS hands bytes
        t0 = time.perf_counter()
        if store is not None:
            docs = [bson.decode(f) for f in files]
            dicts = [{"blob": d["parameters"]["blob"], "cardinality": d["cardinality"]} for d in docs]
        else:
            dicts = [{"blob": b, "cardinality": c} for b, c in zip(blobs, cards)]
        ref, _ = O.aggregate_fedavg(dicts)
        t_cpu = time.perf_counter() - t0
        res["cpu_ref_s"] = round(t_cpu, 3)
        res["cpu_ref_gbs"] = round(in_bytes / t_cpu / 1e9, 3)
        res["cpu_ref_cores"] = 1
        res["speedup_vs_cpu_ref"] = round(t_cpu / t_gpu, 1)
        res["bit_exact"] = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) and x.shape == y.shape
                               for x, y in zip(out, ref))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
