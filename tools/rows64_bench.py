#!/usr/bin/env python3
"""The float64 row-table fold (fa_fedavg_f64_ptrs) against the stacking route it
replaces, on separately allocated client rows.

Per shape (default: 256 x 3.125M, the bytes of the C4 rank bucket; 1024 x 67K;
100 x 582K) it times, as GPU-event spans around the Python call on the current
stream (host work included whenever the GPU waits for it):
  a_rows_ms      engine.fold_rows(RowSet)            the row-table fold
  b_stack_ms     fold_stacked(RowSet.stacked())      copy the rows into a fresh [N, P], then fold
  c_stacked_ms   engine.fold_stacked(X)              fa_fedavg_f64 alone, X stacked beforehand
  sweep_ms       fa_read_sweep_f32 over the same bytes (the read-only calibration kernel)
Everything is warmed up, then the candidates run interleaved for --reps rounds;
each figure is the median with the spread (min, max) next to it.  (a), (b) and
(c) must give the same bits.

    python tools/rows64_bench.py [--shapes NxP,...] [--reps R] [--out FILE]   (GPU box)
prints one JSON line per shape, and writes them to FILE when given.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedlesscan_amd import _lib, engine, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="256x3125000,1024x67000,100x582026")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rows64_bench needs a GPU")
dev = torch.device("cuda", 0)
L, B = _lib.load(), _lib.load_bench()
st = torch.cuda.current_stream(dev).cuda_stream
SEED = 9


def make_rows(N, P):
    """N separately allocated float64 rows: the library's generator (bit-identical
    to synth) widened and scaled by 1 + 1/3, which fills the low mantissa bits."""
    rows = []
    tmp = torch.empty(P, dtype=torch.float32, device=dev)
    for i in range(N):
        _lib.check(B.fa_synth_f32(tmp.data_ptr(), 1, P, P, SEED, i, 0, st), "fa_synth_f32", bench=True)
        rows.append(tmp.to(torch.float64) * (1.0 + 1.0 / 3.0))
    return rows


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


lines = []
for shape in args.shapes.split(","):
    N, P = (int(x) for x in shape.lower().split("x"))
    w = synth.cardinalities(SEED, N)
    rows = make_rows(N, P)
    rs, X = engine.RowSet(rows), torch.stack(rows)
    assert rs.view is None and rs.aligned
    sink = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    nfloats = X.numel() * 2 - (X.numel() * 2) % 4

    def sweep():
        _lib.check(B.fa_read_sweep_f32(X.data_ptr(), nfloats, sink.data_ptr(), sink.numel(), st), "fa_read_sweep_f32",
                   bench=True)

    before = engine.stats["rows64_folds"]
    t = measure({"a": lambda: engine.fold_rows(rs, w),
                 "b": lambda: engine.fold_stacked(rs.stacked(), w),
                 "c": lambda: engine.fold_stacked(X, w),
                 "sweep": sweep}, args.reps)
    assert engine.stats["rows64_folds"] > before, "fold_rows did not take the row table"
    ra, rb, rc = engine.fold_rows(rs, w), engine.fold_stacked(rs.stacked(), w), engine.fold_stacked(X, w)
    same = torch.equal(ra.view(torch.int64), rb.view(torch.int64)) and torch.equal(ra.view(torch.int64),
                                                                                   rc.view(torch.int64))
    gb = (N * P * 8 + P * 8) / 1e9
    b_spread = t["b"][2] - t["b"][1]
    rec = {"dtype": "float64", "clients": N, "params": P, "reps": args.reps,
           "a_rows_ms": round(t["a"][0], 4), "a_spread_ms": [round(x, 4) for x in t["a"][1:]],
           "b_stack_ms": round(t["b"][0], 4), "b_spread_ms": [round(x, 4) for x in t["b"][1:]],
           "c_stacked_ms": round(t["c"][0], 4), "c_spread_ms": [round(x, 4) for x in t["c"][1:]],
           "sweep_ms": round(t["sweep"][0], 4), "sweep_spread_ms": [round(x, 4) for x in t["sweep"][1:]],
           "a_GBps": round(gb / t["a"][0] * 1e3, 1), "c_GBps": round(gb / t["c"][0] * 1e3, 1),
           "sweep_GBps": round(N * P * 8 / 1e9 / t["sweep"][0] * 1e3, 1),
           "a_over_b": round(t["a"][0] / t["b"][0], 3), "a_over_c": round(t["a"][0] / t["c"][0], 3),
           "a_fraction_of_sweep": round(t["sweep"][0] / t["a"][0], 3),
           "bar_a_no_slower_than_b_by_more_than_its_spread": bool(t["a"][0] - t["b"][0] <= b_spread),
           "bit_identical": bool(same)}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    del rows, rs, X
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
