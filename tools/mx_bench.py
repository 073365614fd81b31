#!/usr/bin/env python3
"""The MX folds (fa_fedavg_mx / fa_fedavg_mx_ptrs) against the yardsticks that
are not the code under test, inputs in HBM, one process.

Per shape (default: 100 x 1M; 256 x 12.5M; 256 x 100M) and format (e4m3, e5m2,
e2m1) it times, as GPU-event spans around the Python call on the current stream:
  plain / scored   engine.fold_stacked(X, w, scores?, block_scales=E)
  rows             engine.fold_rows(RowSet of separately allocated rows and scale rows, scored)
  sweep            fa_read_sweep_f32 over the same bytes (elements + scales): the streaming-read ceiling
  fp8_scaled       the fp8 fold with per-client scales over N x P bytes   (once per shape)
  bf16             the bf16 fold of the same N x P, float32 output        (once per shape)
  upcast           the route without the kernels: dequantise with torch, then fold_stacked (where it fits)
and records the peak of torch.cuda.max_memory_allocated over one call above
what was allocated before it.  Every candidate is warmed up, then the candidates
run interleaved for --reps rounds; each figure is the median with the spread
(min, max).  The MX fold must give the bits of the upcast route and the row
table those of the stacked fold (checked).

--forms F:B,... adds, per listed pair, the bench library's fa_fedavg_mx_form
(bit 0 = loads ahead, bit 1 = LDS exchange, bit 2 = the hardware's scaled
convert; B blocks per CU), plain; forms without bit 2 are checked for the
product's bits, forms with it report whether they have them.

    python tools/mx_bench.py [--shapes NxP,...] [--fmts e4m3,...] [--reps R] [--forms F:B,...] [--out FILE]
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
ap.add_argument("--shapes", default="100x1000000,256x12500000,256x100000000")
ap.add_argument("--fmts", default="e4m3,e5m2,e2m1")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--forms", default="", help="form:blocks_per_cu pairs of fa_fedavg_mx_form, e.g. 1:2,3:1,7:2")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mx_bench needs a GPU")
dev = torch.device("cuda", 0)
B = _lib.load_bench()
st = torch.cuda.current_stream(dev).cuda_stream
SEED = 9
FMTS = {"e4m3": (torch.float8_e4m3fn, _lib.FA_MX_E4M3), "e5m2": (torch.float8_e5m2, _lib.FA_MX_E5M2),
        "e2m1": (torch.float4_e2m1fn_x2, _lib.FA_MX_E2M1)}
E2M1 = [0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6]


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


def dequantise(name, X, E, P):
    """The float32 rows a user forms with torch today."""
    if name == "e2m1":
        b = X.view(torch.uint8)
        tab = torch.tensor(E2M1, dtype=torch.float32, device=dev)
        x = torch.stack([tab[(b & 15).long()], tab[(b >> 4).long()]], dim=-1).reshape(b.shape[0], -1)
    else:
        x = X.to(torch.float32)
    # 2^(e - 127) from the byte as an exponent field: this tool's scale bytes are 117..137, never 0 or 255
    return x.mul_((E.to(torch.int32) << 23).view(torch.float32).repeat_interleave(32, dim=1)[:, :P])


lines = []
for shape in args.shapes.split(","):
    N, P = (int(x) for x in shape.lower().split("x"))
    w = synth.cardinalities(SEED, N)
    sc = [(r + 1) / 11 for r in synth.round_ids(SEED, N, 10, 2)]
    scales = [float(x) for x in np.random.default_rng(SEED).uniform(0.01, 2.0, N)]
    sink = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    # the yardsticks of the same N x P: the fp8 fold with per-client scales, the bf16 fold
    X8 = torch.randint(0, 256, (N, P), dtype=torch.uint8, device=dev).bitwise_and_(0xF7).view(torch.float8_e4m3fn)
    base = measure({"fp8_scaled": lambda: engine.fold_stacked(X8, w, scales=scales)}, args.reps)
    del X8
    Xb = torch.empty((N, P), dtype=torch.bfloat16, device=dev)
    _lib.check(B.fa_synth_bf16(Xb.data_ptr(), N, P, P, SEED, 0, 0, st), "fa_synth_bf16", bench=True)
    base.update(measure({"bf16": lambda: engine.fold_stacked(Xb, w)}, args.reps))
    del Xb
    torch.cuda.empty_cache()
    for name in args.fmts.split(","):
        dt, fmt = FMTS[name]
        nb, pb = (P + 31) // 32, (P // 2 if name == "e2m1" else P)
        # one allocation holds the element bytes and then the scale bytes, so one sweep reads both;
        # finite codes (bit 3 of an e4m3 byte cleared, bits 2 of e5m2), scale bytes in 117..137
        buf = torch.randint(0, 256, (N * pb + N * nb + 16,), dtype=torch.uint8, device=dev)
        X = buf[:N * pb].view(N, pb)
        if name != "e2m1":
            X.bitwise_and_(0xF7 if name == "e4m3" else 0xFB)
        E = buf[N * pb:N * pb + N * nb].view(N, nb)
        E.remainder_(21).add_(117)
        X = X.view(dt)
        nfloats = (N * pb + N * nb) // 16 * 4  # whole 16-byte units

        def sweep():
            _lib.check(B.fa_read_sweep_f32(buf.data_ptr(), nfloats, sink.data_ptr(), sink.numel(), st),
                       "fa_read_sweep_f32", bench=True)

        fns = {"plain": lambda: engine.fold_stacked(X, w, block_scales=E),
               "scored": lambda: engine.fold_stacked(X, w, sc, block_scales=E), "sweep": sweep}
        fits = N * P <= (4e9 if name != "e2m1" else 2e8)
        if fits:
            fns["upcast"] = lambda: engine.fold_stacked(dequantise(name, X, E, P), w)
        fa = torch.tensor(np.asarray(w, dtype=np.float32), device=dev)
        fout = torch.empty(P, dtype=torch.float32, device=dev)
        form_keys = []
        for pair in filter(None, args.forms.split(",")):
            form, bpc = (int(x) for x in pair.split(":"))

            def run_form(form=form, bpc=bpc):
                _lib.check(B.fa_fedavg_mx_form(fmt, X.data_ptr(), E.data_ptr(), N, P, pb, nb, fa.data_ptr(), None, None,
                                               float(np.float32(sum(w))), fout.data_ptr(), None, st, form, bpc),
                           "fa_fedavg_mx_form", bench=True)
                return fout

            fns[f"form{form}_bpc{bpc}"] = run_form
            form_keys.append((f"form{form}_bpc{bpc}", form))
        t = measure(fns, args.reps)
        ref = engine.fold_stacked(X, w, block_scales=E)
        forms_same = {k: bool(torch.equal(bits(fns[k]()), bits(ref))) for k, _ in form_keys}
        assert all(same for (k, form), same in zip(form_keys, forms_same.values()) if not form & 4)
        same = bool(torch.equal(bits(ref), bits(fns["upcast"]()))) if fits else None
        rows, es = [X[i].clone() for i in range(N)], [E[i].clone() for i in range(N)]
        rs = engine.RowSet(rows, block_scales=es)
        assert rs.aligned
        t.update(measure({"rows": lambda: engine.fold_rows(rs, w, sc)}, args.reps))
        same_rows = bool(torch.equal(bits(engine.fold_rows(rs, w, sc)),
                                     bits(engine.fold_stacked(X, w, sc, block_scales=E))))
        del rows, es, rs
        t.update(base)
        src = N * pb + N * nb
        rec = {"fmt": name, "clients": N, "params": P, "reps": args.reps, "src_bytes": src, "out_bytes": 4 * P}
        for k, ((med, lo, hi), peak) in t.items():
            rec[k + "_ms"] = round(med, 4)
            rec[k + "_spread_ms"] = [round(lo, 4), round(hi, 4)]
            rec[k + "_peak_bytes"] = int(peak)
            if k != "sweep":
                rec[k + "_Gelem_s"] = round(N * P / med / 1e6, 1)
        rec["plain_over_sweep"] = round(t["plain"][0][0] / t["sweep"][0][0], 3)
        rec["plain_over_fp8_scaled"] = round(t["plain"][0][0] / t["fp8_scaled"][0][0], 3)
        rec["bit_identical_to_upcast"] = same
        rec["rows_bit_identical_to_stacked"] = same_rows
        rec["forms_bit_identical_to_product"] = forms_same
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        assert same is not False and same_rows, "MX fold differs from the upcast route / the row table from the stacked"
        del X, E, buf
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
