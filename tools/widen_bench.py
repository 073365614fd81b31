#!/usr/bin/env python3
"""Promoted stacked folds: time per fold, source bytes per second and the rise
of peak allocated memory, per (row dtype -> fold dtype) kind and shape.

The tool is written against engine.fold_stacked only, so the same file times a
checkout from before the widening fold (fa_fedavg_widen): --repo names the
tree to import.  There a promoted fold widens the whole matrix first (X.to)
and folds the copy; here it reads the narrow rows once.

Cells, X device-resident, weights of a type that makes numpy promote:
  F16_F32  float16 rows, np.float32 weights      F16_F64  float16 rows, np.float64 weights
  F32_F64  float32 rows, np.int64 weights        I32_F64  int32 rows, float weights
  I64_F64  int64 rows, float weights             I32_I64  int32 rows, np.int64 weights
and next to them the same rows under Python-int weights, which do not promote
(f32, f16, i32: fa_fedavg_f32, fa_fedavg_f16, fa_fedavg_i32): what a read-once
fold of those bytes reaches here.
Shapes: 100 x 1M, 1024 x 1M, 256 x 12.5M; fewer rows where the source and a
widened copy of it would not fit in the free device memory.

Each shape runs in a child process of its own under `timeout`, one after the
other, and the first that fails ends the run (as steps chained with &&).  In a
child, per cell: warm-up folds, then --reps windows of several folds between
two device events (enough folds for a window of about 50 ms), rotating over
copies of X that together exceed the 256 MB Infinity Cache; the figure is the
median window over its folds, with (min, max) as the run-to-run spread.  The
rise of torch.cuda.max_memory_allocated over one fold is taken separately.

    python tools/widen_bench.py [--repo DIR] [--tag NAME] [--reps 7] [--shapes 100x1000000,...] [--out FILE]
prints one JSON line per cell and appends them to FILE when given.  (GPU box)
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=os.path.dirname(HERE))
ap.add_argument("--tag", default="")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shapes", default="100x1000000,1024x1000000,256x12500000")
ap.add_argument("--cells", default="")
ap.add_argument("--timeout", type=int, default=240, help="seconds per shape")
ap.add_argument("--out", default="")
ap.add_argument("--shape", default="", help="(child) the one shape to measure")
args = ap.parse_args()

# cell -> (torch row dtype name, weights' type name, wide element bytes or 0, scored allowed)
CELLS = {"F16_F32": ("float16", "np_float32", 4), "F16_F64": ("float16", "np_float64", 8),
         "F32_F64": ("float32", "np_int64", 8), "I32_F64": ("int32", "py_float", 8),
         "I64_F64": ("int64", "py_float", 8), "I32_I64": ("int32", "np_int64", 8),
         "f32": ("float32", "py_int", 0), "f16": ("float16", "py_int", 0), "i32": ("int32", "py_int", 0)}
cells = [c for c in args.cells.split(",") if c] or list(CELLS)
unknown = [c for c in cells if c not in CELLS]
if unknown:
    sys.exit(f"unknown cells {unknown}")

if not args.shape:
    # the driver: one child per shape, each under its own time limit; the first failure ends the run
    for shape in args.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--shape", shape,
               "--repo", args.repo, "--tag", args.tag, "--reps", str(args.reps), "--cells", ",".join(cells)]
        if args.out:
            cmd += ["--out", args.out]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit(f"widen_bench: shape {shape} ended with status {rc}; nothing further is started")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.abspath(args.repo))
from fedlesscan_amd import engine  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("widen_bench needs a GPU")
dev = torch.device("cuda", 0)
SEED = 11
CACHE_BYTES = 256 << 20
N0, P = (int(v) for v in args.shape.split("x"))


def weights(kind: str, n: int):
    base = [3 + (7 * i) % 600 for i in range(n)]
    return {"py_int": base, "py_float": [v + 0.25 for v in base], "np_int64": [np.int64(v) for v in base],
            "np_float32": [np.float32(v + 1 / 3) for v in base],
            "np_float64": [np.float64(v + 1 / 3) for v in base]}[kind]


def rows(dtype: torch.dtype, n: int, gen) -> torch.Tensor:
    if dtype.is_floating_point:
        X = torch.empty((n, P), dtype=dtype, device=dev)
        for i in range(n):  # row by row: no float32 temporary of the whole matrix
            X[i] = torch.randn(P, device=dev, generator=gen) * 0.05
        return X
    lim = 2 ** 30 if dtype == torch.int32 else 2 ** 62
    return torch.randint(-lim, lim, (n, P), dtype=dtype, device=dev, generator=gen)


def window(fn, bufs, k0: int, folds: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(folds):
        fn(bufs[(k0 + k) % len(bufs)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / folds


lines = []
for cell in cells:
    tname, wkind, wide = CELLS[cell]
    dtype = getattr(torch, tname)
    esize = torch.empty(0, dtype=dtype).element_size()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    # copies of X so that consecutive folds do not read one another's rows from the Infinity Cache
    nbuf = min(4, max(1, -(-2 * CACHE_BYTES // (N0 * P * esize))))
    n = N0
    while n > 1 and (nbuf * esize + wide) * n * P > 0.8 * free:  # the source and one widened copy must fit
        n //= 2
    gen = torch.Generator(device=dev).manual_seed(SEED)
    bufs = [rows(dtype, n, gen) for _ in range(nbuf)]
    w = weights(wkind, n)

    def fold(X):
        return engine.fold_stacked(X, w)

    for X in bufs[:2] * 2:
        fold(X)
    torch.cuda.synchronize(dev)
    est = window(fold, bufs, 0, 2)
    folds = int(min(50, max(2, 50.0 / max(est, 1e-3))))
    ts = sorted(window(fold, bufs, r * folds, folds) for r in range(args.reps))
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fold(bufs[0])
    torch.cuda.synchronize(dev)
    rise = torch.cuda.max_memory_allocated(dev) - base
    med = ts[len(ts) // 2]
    src = n * P * esize
    rec = {"tag": args.tag, "cell": cell, "rows": n, "cols": P, "row_dtype": tname, "weights": wkind,
           "out_dtype": str(out.dtype).replace("torch.", ""), "buffers": nbuf, "folds_per_window": folds,
           "reps": args.reps, "ms_per_fold": round(med, 4), "spread_ms": [round(ts[0], 4), round(ts[-1], 4)],
           "source_gb_per_s": round(src / med / 1e6, 1),
           "source_gb_per_s_spread": [round(src / ts[-1] / 1e6, 1), round(src / ts[0] / 1e6, 1)],
           "peak_rise_bytes": int(rise), "source_bytes": src,
           "widened_folds": engine.stats.get("widened_folds")}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    del bufs, out
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
