#!/usr/bin/env python3
"""The fp8 folds (fa_fedavg_fp8 / fa_fedavg_fp8_ptrs) against the yardsticks
that are not the code under test, inputs in HBM, one process.

Per shape (default: 100 x 1M; 256 x 12.5M, the C4 rank bucket; 256 x 100M, the
whole C4 model) and e4m3fn rows it times, as GPU-event spans around the Python
call on the current stream:
  fp8_ms[variant]  engine.fold_stacked(X8, w, scores?, scales=?)  plain, scaled, scored, scaled+scored
  rows_ms          engine.fold_rows(RowSet of separately allocated rows, scaled + scored)
  upcast_ms        (a) the route without the kernels: X8.to(float32) * scale[:, None], then fold_stacked
  bf16_ms          (b) the bf16 fold of the same N x P, float32 output
  sweep_ms         (c) fa_read_sweep_f32 over the fp8 bytes: the streaming-read ceiling
and records, per candidate, the peak of torch.cuda.max_memory_allocated over
one call above what was allocated before it.  The fp8 folds must add the
outputs alone (checked: at most P * 4 bytes plus the factor staging).  Every
candidate is warmed up, then the candidates run interleaved for --reps rounds;
each figure is the median with the spread (min, max).  The plain fold and the
upcast route must give the same bits (checked at every shape).

--forms F:B,... adds, per listed pair, the bench library's fa_fedavg_fp8_form
(form F of the unit fold: bit 0 = loads of the next row group ahead of the
adds, bit 1 = stores exchanged through LDS; B blocks per CU) plain and with
scales and scores, checked for the product's bits: the rows of DESIGN.md 5
that fix the product's form and grid.

    python tools/fp8_bench.py [--shapes NxP,...] [--reps R] [--forms F:B,...] [--out FILE]   (GPU box)
prints one JSON line per shape, and writes them to FILE when given.
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
ap.add_argument("--shapes", default="100x1000000,256x12500000,256x100000000")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--no-upcast", action="store_true", help="skip (a), whose float32 copy is 4 x the rows")
ap.add_argument("--forms", default="", help="form:blocks_per_cu pairs of fa_fedavg_fp8_form, e.g. 0:1,3:1,3:2")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("fp8_bench needs a GPU")
dev = torch.device("cuda", 0)
B = _lib.load_bench()
st = torch.cuda.current_stream(dev).cuda_stream
SEED = 9


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


def bits(t):
    return t.view(torch.int32)


lines = []
for shape in args.shapes.split(","):
    N, P = (int(x) for x in shape.lower().split("x"))
    w = synth.cardinalities(SEED, N)
    sc = [(r + 1) / 11 for r in synth.round_ids(SEED, N, 10, 2)]
    scales = [float(x) for x in np.random.default_rng(SEED).uniform(0.01, 2.0, N)]
    # finite e4m3fn bytes: bit 3 cleared, so never the NaN encodings 0x7f / 0xff
    X8 = torch.randint(0, 256, (N, P), dtype=torch.uint8, device=dev).bitwise_and_(0xF7).view(torch.float8_e4m3fn)
    cdev = torch.tensor(np.asarray(scales, dtype=np.float32), device=dev)[:, None]
    sink = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    nfloats = (N * P) // 4

    def sweep():
        _lib.check(B.fa_read_sweep_f32(X8.data_ptr(), nfloats, sink.data_ptr(), sink.numel(), st), "fa_read_sweep_f32",
                   bench=True)

    def upcast():
        return engine.fold_stacked(X8.to(torch.float32).mul_(cdev), w)

    fns = {"plain": lambda: engine.fold_stacked(X8, w),
           "scaled": lambda: engine.fold_stacked(X8, w, scales=scales),
           "scored": lambda: engine.fold_stacked(X8, w, sc),
           "scaled_scored": lambda: engine.fold_stacked(X8, w, sc, scales=scales),
           "sweep": sweep}
    if not args.no_upcast:
        fns["upcast"] = upcast
    fa, fs, fc = (torch.tensor(np.asarray(v, dtype=np.float32), device=dev) for v in (w, sc, scales))
    fout = torch.empty(P, dtype=torch.float32, device=dev)
    form_keys = []
    for pair in filter(None, args.forms.split(",")):
        form, bpc = (int(x) for x in pair.split(":"))

        def run_form(both, form=form, bpc=bpc):
            _lib.check(B.fa_fedavg_fp8_form(X8.data_ptr(), N, P, P, fa.data_ptr(), fs.data_ptr() if both else None,
                                            fc.data_ptr() if both else None, float(np.float32(sum(w))),
                                            fout.data_ptr(), None, st, form, bpc), "fa_fedavg_fp8_form", bench=True)
            return fout

        for both in (False, True):
            key = f"form{form}_bpc{bpc}" + ("_scaled_scored" if both else "_plain")
            fns[key] = lambda both=both, run_form=run_form: run_form(both)
            form_keys.append((key, both))
    t = measure(fns, args.reps)
    for key, both in form_keys:
        ref = engine.fold_stacked(X8, w, sc, scales=scales) if both else engine.fold_stacked(X8, w)
        assert torch.equal(bits(fns[key]()), bits(ref)), f"{key} differs from the product fold"
    same = None
    if not args.no_upcast:
        same = bool(torch.equal(bits(engine.fold_stacked(X8, w, scales=scales)), bits(upcast())))
    # separately allocated rows through the table
    rows = [X8[i].clone() for i in range(N)]
    rs = engine.RowSet(rows)
    assert rs.view is None and rs.aligned
    t.update(measure({"rows": lambda: engine.fold_rows(rs, w, sc, scales=scales)}, args.reps))
    same_rows = bool(torch.equal(bits(engine.fold_rows(rs, w, sc, scales=scales)),
                                 bits(engine.fold_stacked(X8, w, sc, scales=scales))))
    del rows, rs
    # (b) the bf16 fold of the same N x P
    Xb = torch.empty((N, P), dtype=torch.bfloat16, device=dev)
    _lib.check(B.fa_synth_bf16(Xb.data_ptr(), N, P, P, SEED, 0, 0, st), "fa_synth_bf16", bench=True)
    t.update(measure({"bf16": lambda: engine.fold_stacked(Xb, w)}, args.reps))
    del Xb
    torch.cuda.empty_cache()

    src = N * P
    rec = {"fmt": "e4m3fn", "clients": N, "params": P, "reps": args.reps, "src_bytes": src, "out_bytes": 4 * P}
    for k, ((med, lo, hi), peak) in t.items():
        rec[k + "_ms"] = round(med, 4)
        rec[k + "_spread_ms"] = [round(lo, 4), round(hi, 4)]
        rec[k + "_peak_bytes"] = int(peak)
        if k != "sweep":
            rec[k + "_Gelem_s"] = round(N * P / med / 1e6, 1)
    for k in ("plain", "scaled", "scored", "scaled_scored", "rows", "sweep") + tuple(k for k, _ in form_keys):
        rec[k + "_src_GBps"] = round(src / t[k][0][0] / 1e6, 1)
    rec["plain_over_sweep"] = round(t["plain"][0][0] / t["sweep"][0][0], 3)
    rec["bit_identical_to_upcast"] = same
    rec["rows_bit_identical_to_stacked"] = same_rows
    # the condition: an fp8 fold allocates its output and the staged factors (each rounded up to the
    # caching allocator's granule: 2 MiB for a large block, 512 B for a small one), nothing that grows with N * P
    slack = -(-4 * P // (2 << 20)) * (2 << 20) + -(-12 * N // 512) * 512 + 512
    rec["fp8_peak_is_outputs_only"] = all(t[k][1] <= slack for k in ("plain", "scaled", "scored", "scaled_scored", "rows"))
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    assert rec["fp8_peak_is_outputs_only"], "an fp8 fold allocated more than its outputs"
    assert same is not False and same_rows, "fp8 fold differs from the upcast route / the row table from the stacked fold"
    del X8
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
