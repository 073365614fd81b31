#!/usr/bin/env python3
"""Promoted folds over separately allocated client tensors: the widening row
tables (fa_fedavg_widen_ptrs / fa_fedavg_widen_layers: fold_rows,
fold_model_rows) against the route they replace, which stacks the rows into
one matrix first and folds that with fa_fedavg_widen.  Per kind and shape:
time per fold, source bytes per second and the rise of peak allocated memory,
for both routes.

Kinds: F32_F64 (float32 rows, np.int64 weights), F16_F32 (float16, np.float32),
I64_F64 (int64, float weights).  Shapes: NxP rows apart (100x1000000,
256x12500000; fewer rows where the sets would not fit), and `model`: 100
clients x 10 tensors (8 of 1M, 2 of 1000 elements) through fold_model_rows
against aggregate_layers' stacked [N, sum] matrix.

Each shape runs in a child process of its own under `timeout`, one after the
other, and the first that fails ends the run.  In a child, per kind: several
sets of rows that together exceed the 256 MB Infinity Cache, warm-up folds of
both routes, then --reps rounds in which a window of the stacked route and a
window of the table route alternate, each window several folds between two
device events rotating over the sets; the figure is the median window over
its folds, with (min, max) as the spread.  The peak rise of one fold is taken
separately.

    python tools/widen_rows_bench.py [--reps 7] [--shapes 100x1000000,256x12500000,model] [--out FILE]
prints one JSON line per kind, shape and route.  (GPU box)
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shapes", default="100x1000000,256x12500000,model")
ap.add_argument("--kinds", default="F32_F64,F16_F32,I64_F64")
ap.add_argument("--timeout", type=int, default=240, help="seconds per shape")
ap.add_argument("--out", default="")
ap.add_argument("--shape", default="", help="(child) the one shape to measure")
args = ap.parse_args()

KINDS = {"F32_F64": ("float32", "np_int64", 8), "F16_F32": ("float16", "np_float32", 4), "I64_F64": ("int64", "py_float", 8)}
MODEL = [1000000] * 4 + [1000] + [1000000] * 4 + [1000]

if not args.shape:
    for shape in args.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--shape", shape,
               "--reps", str(args.reps), "--kinds", args.kinds] + (["--out", args.out] if args.out else [])
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit(f"widen_rows_bench: shape {shape} ended with status {rc}; nothing further is started")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
from fedlesscan_amd import engine  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("widen_rows_bench needs a GPU")
dev = torch.device("cuda", 0)
CACHE_BYTES = 256 << 20
model = args.shape == "model"
N0, sizes = (100, MODEL) if model else (int(args.shape.split("x")[0]), [int(args.shape.split("x")[1])])
P = sum(sizes)


def weights(kind: str, n: int):
    base = [3 + (7 * i) % 600 for i in range(n)]
    return {"py_float": [v + 0.25 for v in base], "np_int64": [np.int64(v) for v in base],
            "np_float32": [np.float32(v + 1 / 3) for v in base]}[kind]


def tensor(dtype, n, gen):
    if dtype.is_floating_point:
        return (torch.randn(n, device=dev, generator=gen) * 0.05).to(dtype)
    return torch.randint(-2 ** 62, 2 ** 62, (n,), dtype=dtype, device=dev, generator=gen)


def window(fn, sets, k0: int, folds: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(folds):
        fn(sets[(k0 + k) % len(sets)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / folds


def peak_rise(fn, arg) -> int:
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn(arg)
    torch.cuda.synchronize(dev)
    del out
    return int(torch.cuda.max_memory_allocated(dev) - base)


lines = []
for cell in args.kinds.split(","):
    tname, wkind, wide = KINDS[cell]
    dtype = getattr(torch, tname)
    esize = torch.empty(0, dtype=dtype).element_size()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    nset = min(4, max(2, -(-2 * CACHE_BYTES // (N0 * P * esize))))
    n = N0
    while n > 1 and (nset + 1) * esize * n * P > 0.8 * free:  # the sets and one stacked copy must fit
        n //= 2
    gen = torch.Generator(device=dev).manual_seed(11)
    # a set: n clients x len(sizes) tensors, every tensor an allocation of its own
    clients = [[[tensor(dtype, m, gen) for m in sizes] for _ in range(n)] for _ in range(nset)]
    w = weights(wkind, n)
    if model:
        prepared = [engine.ModelRowSet(c) for c in clients]
        table = lambda k: engine.fold_model_rows(prepared[k], w)  # noqa: E731
        # aggregate_layers' own stacking of a promoted group: one copy per client and tensor into [N, sum]
        stacked = lambda k: engine.fold_stacked(  # noqa: E731
            engine._stack_group(clients[k], n, list(range(len(sizes))), sizes, P, dev, True), w)
    else:
        prepared = [engine.RowSet([cl[0] for cl in c]) for c in clients]
        table = lambda k: engine.fold_rows(prepared[k], w)  # noqa: E731
        stacked = lambda k: engine.fold_stacked(prepared[k].stacked(), w)  # noqa: E731
    ks = list(range(nset))
    before = dict(engine.stats)
    for fn in (stacked, table, stacked, table):
        fn(0)
    took = {k: v - before[k] for k, v in engine.stats.items() if v != before[k]}
    assert took.get("widened_folds") == 2 and took.get("widened_table_folds" if model else "widened_row_folds"), took
    torch.cuda.synchronize(dev)
    routes = {"stack_then_widen": stacked, "row_table": table}
    folds = {r: int(min(50, max(2, 50.0 / max(window(fn, ks, 0, 2), 1e-3)))) for r, fn in routes.items()}
    ts = {r: [] for r in routes}
    for rep in range(args.reps):  # the two routes alternate, window by window
        for r, fn in routes.items():
            ts[r].append(window(fn, ks, rep * folds[r], folds[r]))
    src = n * P * esize
    for r, fn in routes.items():
        t = sorted(ts[r])
        med = t[len(t) // 2]
        rec = {"cell": cell, "shape": args.shape, "route": r, "clients": n, "cols": P, "tensors": len(sizes),
               "row_dtype": tname, "weights": wkind, "sets": nset, "folds_per_window": folds[r], "reps": args.reps,
               "ms_per_fold": round(med, 4), "spread_ms": [round(t[0], 4), round(t[-1], 4)],
               "source_gb_per_s": round(src / med / 1e6, 1), "peak_rise_bytes": peak_rise(fn, 0), "source_bytes": src,
               "output_bytes": P * wide}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    del clients, prepared
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
