#!/usr/bin/env python3
"""The NVFP4 folds (fa_fedavg_nvfp4 / fa_fedavg_nvfp4_ptrs) against the
yardsticks that are not the code under test, inputs in HBM, one process.

Per shape (default: 100 x 1M; 256 x 12.5M; 256 x 100M) it times, as GPU-event
spans around the Python call on the current stream, for the plain, the scaled
(per-tensor scales) and the scaled + scored fold:
  stacked   engine.fold_stacked(X, w, scores?, block_scales=E, scales=?)
  rows      engine.fold_rows(RowSet of separately allocated rows and scale rows, ...)
  upcast    the route without the kernel: dequantise with torch to float32, then
            fold_stacked (where N x P float32 and its temporaries fit)
and once per shape
  mxfp4         the MXFP4 fold of the same N x P (E8M0 scales), the product's form
  mxfp4_form3   its multiply form (fa_fedavg_mx_form 3:2): plain NVFP4's instruction count
  sweep         fa_read_sweep_f32 over the same bytes, P / 2 + P / 16 per row
with the peak of torch.cuda.max_memory_allocated over one call above what was
allocated before it.  Every candidate is warmed up, then the candidates run
interleaved for --reps rounds; each figure is the median with the spread (min,
max).  stacked, rows and upcast must give the same bits (asserted).

--forms F:B,... adds, per listed pair, the bench library's fa_fedavg_nvfp4_form
(bit 0 = loads ahead, bit 1 = LDS exchange; B blocks per CU), plain, checked
for the product's bits.

    python tools/nvfp4_bench.py [--shapes NxP,...] [--reps R] [--forms F:B,...] [--out FILE]
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
ap.add_argument("--forms", default="", help="form:blocks_per_cu pairs of fa_fedavg_nvfp4_form, e.g. 1:2,3:1")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("nvfp4_bench needs a GPU")
dev = torch.device("cuda", 0)
B = _lib.load_bench()
st = torch.cuda.current_stream(dev).cuda_stream
SEED = 9
FP4, E4M3 = torch.float4_e2m1fn_x2, torch.float8_e4m3fn
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


def dequantise(X, E, P, scales):
    """The float32 rows a user forms with torch today: codes, times the block scales, times the tensor's scale."""
    b = X.view(torch.uint8)
    tab = torch.tensor(E2M1, dtype=torch.float32, device=dev)
    x = torch.stack([tab[(b & 15).int()], tab[(b >> 4).int()]], dim=-1).reshape(b.shape[0], -1)
    x.mul_(E.view(E4M3).to(torch.float32).repeat_interleave(16, dim=1)[:, :P])
    if scales is not None:
        x.mul_(torch.tensor(np.asarray(scales, dtype=np.float32), device=dev)[:, None])
    return x


lines = []
for shape in args.shapes.split(","):
    N, P = (int(x) for x in shape.lower().split("x"))
    w = synth.cardinalities(SEED, N)
    sc = [(r + 1) / 11 for r in synth.round_ids(SEED, N, 10, 2)]
    scales = [float(x) for x in np.random.default_rng(SEED).uniform(0.01, 2.0, N)]
    cases = {"plain": (None, None), "scaled": (None, scales), "scaled_scored": (sc, scales)}
    sink = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    pb, nb, nmx = P // 2, (P + 15) // 16, (P + 31) // 32
    # one allocation holds the codes and then the scale bytes, so one sweep reads both; the scale bytes are
    # positive normal e4m3 values in [0.25, 4]; the MXFP4 fold reads the same codes with E8M0 bytes 117..137
    buf = torch.randint(0, 256, (N * pb + N * nb + 16,), dtype=torch.uint8, device=dev)
    X = buf[:N * pb].view(N, pb).view(FP4)
    E = buf[N * pb:N * pb + N * nb].view(N, nb)
    E.remainder_(33).add_(0x28)
    E = E.view(E4M3)
    Emx = torch.randint(117, 138, (N, nmx), dtype=torch.uint8, device=dev)
    nfloats = (N * pb + N * nb) // 16 * 4  # whole 16-byte units
    fa = torch.tensor(np.asarray(w, dtype=np.float32), device=dev)
    fout = torch.empty(P, dtype=torch.float32, device=dev)
    div = float(np.float32(sum(w)))

    def sweep():
        _lib.check(B.fa_read_sweep_f32(buf.data_ptr(), nfloats, sink.data_ptr(), sink.numel(), st),
                   "fa_read_sweep_f32", bench=True)

    def mx_form3():
        _lib.check(B.fa_fedavg_mx_form(_lib.FA_MX_E2M1, X.data_ptr(), Emx.data_ptr(), N, P, pb, nmx, fa.data_ptr(), None,
                                       None, div, fout.data_ptr(), None, st, 3, 2), "fa_fedavg_mx_form", bench=True)

    fns = {"sweep": sweep, "mxfp4": lambda: engine.fold_stacked(X, w, block_scales=Emx), "mxfp4_form3": mx_form3}
    fits = N * P <= 4e9
    for k, (s_, c_) in cases.items():
        fns["stacked_" + k] = lambda s_=s_, c_=c_: engine.fold_stacked(X, w, s_, block_scales=E, scales=c_)
        if fits:
            fns["upcast_" + k] = lambda s_=s_, c_=c_: engine.fold_stacked(dequantise(X, E, P, c_), w, s_)
    form_keys = []
    for pair in filter(None, args.forms.split(",")):
        form, bpc = (int(x) for x in pair.split(":"))

        def run_form(form=form, bpc=bpc):
            _lib.check(B.fa_fedavg_nvfp4_form(X.data_ptr(), E.data_ptr(), N, P, pb, nb, fa.data_ptr(), None, None, div,
                                              fout.data_ptr(), None, st, form, bpc), "fa_fedavg_nvfp4_form", bench=True)
            return fout

        fns[f"form{form}_bpc{bpc}"] = run_form
        form_keys.append(f"form{form}_bpc{bpc}")
    t = measure(fns, args.reps)
    ref = {k: engine.fold_stacked(X, w, s_, block_scales=E, scales=c_) for k, (s_, c_) in cases.items()}
    forms_same = {k: bool(torch.equal(bits(fns[k]()), bits(ref["plain"]))) for k in form_keys}
    same = {k: bool(torch.equal(bits(ref[k]), bits(fns["upcast_" + k]()))) for k in cases} if fits else None
    rows, es = [X[i].clone() for i in range(N)], [E[i].clone() for i in range(N)]
    rs = engine.RowSet(rows, block_scales=es)
    assert rs.aligned
    rfns = {"rows_" + k: lambda s_=s_, c_=c_: engine.fold_rows(rs, w, s_, scales=c_) for k, (s_, c_) in cases.items()}
    t.update(measure(rfns, args.reps))
    same_rows = {k: bool(torch.equal(bits(rfns["rows_" + k]()), bits(ref[k]))) for k in cases}
    del rows, es, rs
    rec = {"clients": N, "params": P, "reps": args.reps, "src_bytes": N * pb + N * nb, "out_bytes": 4 * P}
    for k, ((med, lo, hi), peak) in t.items():
        rec[k + "_ms"] = round(med, 4)
        rec[k + "_spread_ms"] = [round(lo, 4), round(hi, 4)]
        rec[k + "_peak_bytes"] = int(peak)
        if k != "sweep":
            rec[k + "_Gelem_s"] = round(N * P / med / 1e6, 1)
    rec["plain_over_sweep"] = round(t["stacked_plain"][0][0] / t["sweep"][0][0], 3)
    rec["plain_over_mxfp4_form3"] = round(t["stacked_plain"][0][0] / t["mxfp4_form3"][0][0], 3)
    rec["bit_identical_to_upcast"] = same
    rec["rows_bit_identical_to_stacked"] = same_rows
    rec["forms_bit_identical_to_product"] = forms_same
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    assert (same is None or all(same.values())) and all(same_rows.values()) and all(forms_same.values()), \
        "the NVFP4 fold differs from the upcast route, the row table from the stacked fold, or a form from the product"
    del X, E, Emx, buf
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
