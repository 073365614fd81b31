#!/usr/bin/env python3
"""The MX folds with an MX result (fa_fedavg_mx_q) against the same folds with
their float32 result (fa_fedavg_mx, the route without out_format), inputs in
HBM, one process.

Per shape (default: 10 x 100M; 256 x 100M) and format (e2m1, e4m3: the source
and the result alike) it times, as GPU-event spans around the Python call:
  f32      engine.fold_stacked(X, w, block_scales=E)
  mx       engine.fold_stacked(X, w, block_scales=E, out_format=dtype)
  both     ... with out= too: the float32 result and the MX result of one launch
and records the peak of torch.cuda.max_memory_allocated over one call above
what was allocated before it.  Every candidate is warmed up, then the candidates
run interleaved for --reps rounds; each figure is the median with the spread
(min, max).  The float32 result of `both` must have the bits of `f32` (checked).

--forms adds the bench library's fa_fedavg_mx_q_form, forms 0..4 (bit 0 = fp8
codes exchanged through LDS, bit 1 = the hardware's scaled convert divides,
4 = form 0 with the sign bits patched), and says which give the product's bytes.

    python tools/mx_out_bench.py [--shapes NxP,...] [--fmts e2m1,...] [--reps R] [--forms] [--out FILE]
prints one JSON line per shape and format, and writes them to FILE when given.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedlesscan_amd import _lib, engine, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="10x100000000,256x100000000")
ap.add_argument("--fmts", default="e2m1,e4m3")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--forms", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mx_out_bench needs a GPU")
dev = torch.device("cuda", 0)
B = _lib.load_bench()
st = torch.cuda.current_stream(dev).cuda_stream
SEED = 9
FMTS = {"e4m3": (torch.float8_e4m3fn, _lib.FA_MX_E4M3), "e5m2": (torch.float8_e5m2, _lib.FA_MX_E5M2),
        "e2m1": (torch.float4_e2m1fn_x2, _lib.FA_MX_E2M1)}


def span(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def peak_over(fn) -> int:
    """Bytes allocated at the peak of one call above what was allocated before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    r = fn()
    torch.cuda.synchronize()
    del r
    return torch.cuda.max_memory_allocated(dev) - base


def measure(fns: dict, reps: int) -> dict:
    """{name: (median, min, max) ms, peak bytes}: two warm-up rounds, then interleaved."""
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    peaks = {k: peak_over(fn) for k, fn in fns.items()}
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(span(fn))
    return {k: ((sorted(v)[len(v) // 2], min(v), max(v)), peaks[k]) for k, v in ts.items()}


lines = []
for shape in args.shapes.split(","):
    N, P = (int(x) for x in shape.lower().split("x"))
    w = synth.cardinalities(SEED, N)
    for name in args.fmts.split(","):
        dt, fmt = FMTS[name]
        nb, pb = (P + 31) // 32, (P // 2 if name == "e2m1" else P)
        # finite codes (bit 3 of an e4m3 byte cleared, bit 2 of e5m2), scale bytes in 117..137
        X = torch.randint(0, 256, (N, pb), dtype=torch.uint8, device=dev)
        if name != "e2m1":
            X.bitwise_and_(0xF7 if name == "e4m3" else 0xFB)
        E = torch.randint(117, 138, (N, nb), dtype=torch.uint8, device=dev)
        X = X.view(dt)
        fout = torch.empty(P, dtype=torch.float32, device=dev)
        fns = {"f32": lambda: engine.fold_stacked(X, w, block_scales=E),
               "mx": lambda: engine.fold_stacked(X, w, block_scales=E, out_format=dt),
               "both": lambda: engine.fold_stacked(X, w, block_scales=E, out_format=dt, out=fout)}
        fa = torch.tensor(np.asarray(w, dtype=np.float32), device=dev)
        fq, fe = torch.empty(pb, dtype=torch.uint8, device=dev), torch.empty(nb, dtype=torch.uint8, device=dev)
        for form in range(5) if args.forms else ():
            def run_form(form=form):
                _lib.check(B.fa_fedavg_mx_q_form(fmt, X.data_ptr(), E.data_ptr(), N, P, pb, nb, fa.data_ptr(),
                                                 float(np.float32(sum(w))), None, fmt, fq.data_ptr(), fe.data_ptr(), st,
                                                 form), "fa_fedavg_mx_q_form", bench=True)
                return fq, fe

            fns[f"form{form}"] = run_form
        t = measure(fns, args.reps)
        ref = engine.fold_stacked(X, w, block_scales=E, out_format=dt, out=fout)
        assert torch.equal(fout.view(torch.int32), fns["f32"]().view(torch.int32)), "out= differs from the float32 fold"
        rq, re = ref.q.view(torch.uint8).clone(), ref.e.view(torch.uint8).clone()
        forms_same = {}
        for k in [k for k in fns if k.startswith("form")]:
            q, e = fns[k]()
            forms_same[k] = bool(torch.equal(q, rq) and torch.equal(e, re))
        rec = {"fmt": name, "clients": N, "params": P, "reps": args.reps, "src_bytes": N * (pb + nb),
               "f32_out_bytes": 4 * P, "mx_out_bytes": pb + nb}
        for k, ((med, lo, hi), peak) in t.items():
            rec[k + "_ms"] = round(med, 4)
            rec[k + "_spread_ms"] = [round(lo, 4), round(hi, 4)]
            rec[k + "_peak_bytes"] = int(peak)
        rec["f32_over_mx"] = round(t["f32"][0][0] / t["mx"][0][0], 3)
        rec["forms_bytes_identical_to_product"] = forms_same
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del X, E, fout, fq, fe, ref, rq, re
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
