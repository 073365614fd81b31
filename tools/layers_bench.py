#!/usr/bin/env python3
"""The one-launch layer-table fold (fa_fedavg_*_layers) against the per-layer
row-table route it replaces, on multi-layer models whose every client layer is
a separately allocated device tensor.

Models: the four layer lists of SURVEY.md App. D (Keras get_weights() order).
Per model, dtype (fp32 and bf16; --dtypes also takes f16, f64) and client
count it times, as GPU-event spans around the Python call on the current stream (host work included whenever the
GPU waits for it):
  a_per_layer_ms   aggregate_layers, FEDAVG_LAYER_TABLE=0   one fold_rows per layer (the route before)
  b_table_ms       aggregate_layers, FEDAVG_LAYER_TABLE=1   table and plan built in the call, one launch
  c_prepared_ms    fold_model_rows(ModelRowSet)             table built beforehand: factors + one launch
  d_stacked_ms     fold_stacked(X)                          the model flattened and stacked beforehand: the floor
Everything is warmed up, then the candidates run interleaved for --reps rounds;
each figure is the median with the spread (min, max) next to it.  (a), (b) and
(c) must give the same bits.  The bar, fixed before any run: (b) is no slower
than (a) by more than (a)'s own min-max spread.

    python tools/layers_bench.py [--models m,...] [--dtypes f32,bf16] [--clients 100,1024] [--reps R] [--out FILE]
prints one JSON line per case, and writes them to FILE when given.  (GPU box)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedlesscan_amd import engine, synth  # noqa: E402

MODELS = {
    "mnist_cnn": [(5, 5, 1, 32), (32,), (5, 5, 32, 64), (64,), (1024, 512), (512,), (512, 10), (10,)],
    "femnist_cnn": [(5, 5, 1, 32), (32,), (5, 5, 32, 64), (64,), (3136, 2048), (2048,), (2048, 62), (62,)],
    "shakespeare_lstm": [(82, 8), (8, 1024), (256, 1024), (1024,), (256, 1024), (256, 1024), (1024,), (256, 82),
                         (82,)],
    "speech_cnn": [(3, 3, 1, 32), (32,), (3, 3, 32, 32), (32,), (3, 3, 32, 64), (64,), (3, 3, 64, 64), (64,),
                   (64, 35), (35,)],
}
PARAMS = {"mnist_cnn": 582026, "femnist_cnn": 6603710, "shakespeare_lstm": 818402, "speech_cnn": 67267}

ap = argparse.ArgumentParser()
ap.add_argument("--models", default=",".join(MODELS))
ap.add_argument("--dtypes", default="f32,bf16")
ap.add_argument("--clients", default="100,1024")
ap.add_argument("--skip", default="femnist_cnn:1024", help="model:clients pairs left out (27 GB of fp32 rows)")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("layers_bench needs a GPU")
dev = torch.device("cuda", 0)
SEED = 9
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}


def numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


for name, shapes in MODELS.items():
    assert sum(numel(s) for s in shapes) == PARAMS[name], name


def span(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fns: dict, reps: int) -> dict:
    for _ in range(3):
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(span(fn))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def switched(value, params, w):
    os.environ["FEDAVG_LAYER_TABLE"] = value
    return engine.aggregate_layers(params, w)


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


skip = {tuple(x.split(":")) for x in args.skip.split(",") if x}
lines = []
for model in args.models.split(","):
    shapes = MODELS[model]
    for dname in args.dtypes.split(","):
        for N in (int(x) for x in args.clients.split(",")):
            if (model, str(N)) in skip:
                continue
            gen = torch.Generator(device=dev).manual_seed(SEED)
            params = [[(torch.randn(s, device=dev, generator=gen) * 0.05).to(DT[dname]) for s in shapes]
                      for _ in range(N)]
            w = synth.cardinalities(SEED, N)
            ms = engine.ModelRowSet(params)
            X = torch.stack([torch.cat([t.reshape(-1) for t in cl]) for cl in params])
            before = dict(engine.stats)
            t = measure({"a": lambda: switched("0", params, w),
                         "b": lambda: switched("1", params, w),
                         "c": lambda: engine.fold_model_rows(ms, w),
                         "d": lambda: engine.fold_stacked(X, w)}, args.reps)
            assert engine.stats["layer_table_folds"] - before["layer_table_folds"] == 2 * (3 + args.reps)
            assert engine.stats["stacked_groups"] == before["stacked_groups"]
            ra, rb, rc = switched("0", params, w), switched("1", params, w), engine.fold_model_rows(ms, w)
            rd = engine.fold_stacked(X, w)
            same = all(torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(z)) for x, y, z in zip(ra, rb, rc))
            same_d = torch.equal(bits(torch.cat([x.reshape(-1) for x in ra])), bits(rd))
            a_spread = t["a"][2] - t["a"][1]
            P = PARAMS[model]
            rec = {"model": model, "dtype": dname, "clients": N, "layers": len(shapes), "params": P,
                   "reps": args.reps, "units_per_lane": ms.units, "tiles": ms.tiles}
            for k, nm in (("a", "a_per_layer"), ("b", "b_table"), ("c", "c_prepared"), ("d", "d_stacked")):
                rec[nm + "_ms"] = round(t[k][0], 4)
                rec[nm + "_spread_ms"] = [round(x, 4) for x in t[k][1:]]
            rec.update({"b_over_a": round(t["b"][0] / t["a"][0], 3), "c_over_a": round(t["c"][0] / t["a"][0], 3),
                        "c_over_d": round(t["c"][0] / t["d"][0], 3),
                        "bar_b_no_slower_than_a_by_more_than_its_spread": bool(t["b"][0] - t["a"][0] <= a_spread),
                        "bit_identical_abc": bool(same), "bit_identical_stacked": bool(same_d)})
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del params, ms, X, ra, rb, rc, rd
            torch.cuda.empty_cache()
os.environ.pop("FEDAVG_LAYER_TABLE", None)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
