#!/usr/bin/env python3
"""The 16-bit row-table folds (fa_fedavg_bf16_ptrs / fa_fedavg_f16_ptrs) against
the stacking route they replace, on separately allocated client rows.

Per dtype (bf16, float16) and shape (default: 256 x 12.5M, the C4 rank bucket;
1024 x 67K; 100 x 582K) it times, as GPU-event spans around the Python call on
the current stream (host work included whenever the GPU waits for it):
  a_rows_ms      engine.fold_rows(RowSet)            the row-table fold
  b_stack_ms     fold_stacked(RowSet.stacked())      copy the rows into a fresh [N, P], then fold
  c_stacked_ms   engine.fold_stacked(X)              the fold alone, X stacked beforehand
and, for the ratio the fp32 pointer fold itself reaches at the shape,
  f32_rows_ms / f32_stacked_ms  the same pair for float32 rows.
Every shape is warmed up until the tuner has no measurement pending, then the
candidates run interleaved for --reps rounds; each figure is the median with
the spread (min, max) next to it.  (a) and (c) must give the same bits.

    python tools/rows16_bench.py [--shapes NxP,...] [--reps R] [--out FILE]   (GPU box)
prints one JSON line per dtype and shape, and writes them to FILE when given.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedlesscan_amd import _lib, engine, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="256x12500000,1024x67000,100x582026")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--no-f32", action="store_true", help="skip the float32 pair")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rows16_bench needs a GPU")
dev = torch.device("cuda", 0)
L, B = _lib.load(), _lib.load_bench()
st = torch.cuda.current_stream(dev).cuda_stream
SEED = 9


def make_rows(dtype, N, P):
    """N separately allocated rows of the library's generator (bit-identical to synth)."""
    rows = []
    tmp = torch.empty(P, dtype=torch.float32, device=dev) if dtype != torch.bfloat16 else None
    for i in range(N):
        if dtype == torch.bfloat16:
            r = torch.empty(P, dtype=dtype, device=dev)
            _lib.check(B.fa_synth_bf16(r.data_ptr(), 1, P, P, SEED, i, 0, st), "fa_synth_bf16", bench=True)
        else:
            _lib.check(B.fa_synth_f32(tmp.data_ptr(), 1, P, P, SEED, i, 0, st), "fa_synth_f32", bench=True)
            r = tmp.to(dtype) if dtype != torch.float32 else tmp.clone()
        rows.append(r)
    return rows


def span(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fns: dict, reps: int) -> dict:
    """Warm every candidate up (until no tuner measurement is pending), then
    time them interleaved; {name: (median, min, max)} in ms."""
    for _ in range(4):
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        if L.fa_autotune_pending() == 0:
            break
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(span(fn))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


lines = []
for shape in args.shapes.split(","):
    N, P = (int(x) for x in shape.lower().split("x"))
    w = synth.cardinalities(SEED, N, 1, 40)  # sums below 65504: the binary16 divisor stays finite
    f32 = None
    if not args.no_f32:
        rows = make_rows(torch.float32, N, P)
        rs, X = engine.RowSet(rows), torch.stack(rows)
        assert rs.view is None
        f32 = measure({"rows": lambda: engine.fold_rows(rs, w), "stacked": lambda: engine.fold_stacked(X, w)},
                      args.reps)
        assert torch.equal(bits(engine.fold_rows(rs, w)), bits(engine.fold_stacked(X, w)))
        del rows, rs, X
        torch.cuda.empty_cache()
    for name, dtype in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        rows = make_rows(dtype, N, P)
        rs, X = engine.RowSet(rows), torch.stack(rows)
        assert rs.view is None and rs.aligned
        before = engine.stats["rows16_folds"]
        t = measure({"a": lambda: engine.fold_rows(rs, w),
                     "b": lambda: engine.fold_stacked(rs.stacked(), w),
                     "c": lambda: engine.fold_stacked(X, w)}, args.reps)
        assert engine.stats["rows16_folds"] > before, "fold_rows did not take the row table"
        same = torch.equal(bits(engine.fold_rows(rs, w)), bits(engine.fold_stacked(X, w)))
        kind = 2 if name == "bf16" else 4
        gb = (N * P * 2 + P * (4 if name == "bf16" else 2)) / 1e9
        rec = {"dtype": name, "clients": N, "params": P, "reps": args.reps,
               "a_rows_ms": round(t["a"][0], 4), "a_spread_ms": [round(x, 4) for x in t["a"][1:]],
               "b_stack_ms": round(t["b"][0], 4), "b_spread_ms": [round(x, 4) for x in t["b"][1:]],
               "c_stacked_ms": round(t["c"][0], 4), "c_spread_ms": [round(x, 4) for x in t["c"][1:]],
               "a_GBps": round(gb / t["a"][0] * 1e3, 1), "c_GBps": round(gb / t["c"][0] * 1e3, 1),
               "a_over_b": round(t["a"][0] / t["b"][0], 3), "a_over_c": round(t["a"][0] / t["c"][0], 3),
               "stacked_form": L.fa_fold_form(kind, N, P, P, 0, st).decode(),
               "bit_identical": bool(same)}
        if f32 is not None:
            rec.update({"f32_rows_ms": round(f32["rows"][0], 4), "f32_stacked_ms": round(f32["stacked"][0], 4),
                        "f32_rows_over_stacked": round(f32["rows"][0] / f32["stacked"][0], 3)})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del rows, rs, X
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
