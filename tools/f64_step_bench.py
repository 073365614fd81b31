#!/usr/bin/env python3
"""The float64 one-launch step, form by form, next to its per-round launches,
the tiled pair body and the fp32 one-launch step of equal bytes, in one process
at world 1, inputs in HBM.

A rank's share of a 25M-parameter float64 model at 8 GPUs:
overlap_layout(25_000_000, 8, "f64"), 256 clients, its slots side by side
(3.125M columns, 6.4 GB read per step -- the C4 rank's bytes).  Variants over
the same bytes:
  <form>      every kStepSpecsF64 form as one launch (fa_fedavg_f64_rounds_form)
  per_round   the same rounds as fa_fedavg_f64 launches with staged factors
              (what one_launch=False runs)
  pair_fold   the same rounds as finalising fa_fold_f64 launches (acc_in NULL):
              the pair body, tiled
  f32_one     fa_fedavg_f32_rounds over 256 x twice the columns of fp32
              (equal bytes in and out), for scale
Everything is warmed first (timing starts once fa_autotune_pending() == 0),
then `--repeats` windows of `--batch` back-to-back steps between two events,
the variants interleaved within a repeat; median and min-max per variant.  The
policy form is the faster of the balanced and the pooled form when the gap
exceeds the other's min-max spread, else the balanced one.

    python tools/f64_step_bench.py [--clients 256] [--params 25000000] [--repeats 7] [--batch 31] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedlesscan_amd import _lib, synth  # noqa: E402
from fedlesscan_amd.sharding import overlap_layout  # noqa: E402


def fill_rows(X: torch.Tensor, seed: int) -> None:
    """x = (U(0, 1) - 0.5) * 4/3 in X's dtype, generated on the device a few rows at a time."""
    g = torch.Generator(device=X.device)
    g.manual_seed(seed)
    N, ldx = X.shape
    step = max(1, (1 << 26) // max(ldx, 1))
    for i in range(0, N, step):
        n = min(step, N - i)
        r = torch.rand((n, ldx), generator=g, device=X.device, dtype=X.dtype)
        X[i:i + n].copy_((r - 0.5) * (4.0 / 3.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=256)
    ap.add_argument("--params", type=int, default=25_000_000)
    ap.add_argument("--world", type=int, default=8, help="the layout's world size (the run itself is one process)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=31, help="steps per timed window")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L, B = _lib.load(), _lib.load_bench()
    st = torch.cuda.current_stream(dev)
    sp = st.cuda_stream
    N = args.clients
    lay = overlap_layout(args.params, args.world, "f64")
    W, R = lay.local_width, lay.rounds
    offs = [lay.offset(k) for k in range(R + 1)]
    coffs = (ctypes.c_int64 * (R + 1))(*offs)
    coffs32 = (ctypes.c_int64 * (R + 1))(*[2 * o for o in offs])  # the fp32 step: twice the columns, equal bytes
    X = torch.empty((N, W), dtype=torch.float64, device=dev)
    fill_rows(X, 5)
    X32 = torch.empty((N, 2 * W), dtype=torch.float32, device=dev)
    fill_rows(X32, 6)
    w = synth.cardinalities(5, N)
    a64 = torch.tensor(np.array(w, np.float64), device=dev)
    d64 = float(sum(w))
    a32 = torch.tensor(np.array(w, np.float32), device=dev)
    d32 = float(np.float32(sum(w)))
    out64 = torch.empty(W, dtype=torch.float64, device=dev)
    out32 = torch.empty(2 * W, dtype=torch.float32, device=dev)
    rb, r32 = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(B.fa_bench_rounds_create(ctypes.byref(rb), dev.index), "rounds state", bench=True)
    _lib.check(L.fa_rounds_create(ctypes.byref(r32), dev.index), "fa_rounds_create")
    forms = [B.fa_step_form_name_f64(f).decode() for f in range(B.fa_num_step_forms_f64())]

    def one_launch(f):
        def run():
            _lib.check(B.fa_fedavg_f64_rounds_form(rb, f, X.data_ptr(), N, W, a64.data_ptr(), None, d64,
                                                   out64.data_ptr(), R, coffs, None, sp), "f64 rounds", bench=True)
        return run

    def per_round():
        for k in range(R):
            _lib.check(L.fa_fedavg_f64(X.data_ptr() + 8 * offs[k], N, offs[k + 1] - offs[k], W, a64.data_ptr(), None,
                                       d64, out64.data_ptr() + 8 * offs[k], sp), "fa_fedavg_f64")

    def pair_fold():
        for k in range(R):
            _lib.check(L.fa_fold_f64(X.data_ptr() + 8 * offs[k], N, offs[k + 1] - offs[k], W, a64.data_ptr(), None,
                                     None, d64, 1, out64.data_ptr() + 8 * offs[k], sp), "fa_fold_f64")

    def f32_one():
        _lib.check(L.fa_fedavg_f32_rounds(r32, X32.data_ptr(), N, 2 * W, a32.data_ptr(), None, d32, out32.data_ptr(),
                                          R, coffs32, None, sp), "fa_fedavg_f32_rounds")

    runs = {name: one_launch(f) for f, name in enumerate(forms)}
    runs.update(per_round=per_round, pair_fold=pair_fold, f32_one=f32_one)
    for _ in range(20):  # warm-up; the tuner's measurement of each round's shape completes here
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        if L.fa_autotune_pending() == 0:
            break
    pending = L.fa_autotune_pending()
    # every float64 variant computed the same bits
    per_round()
    torch.cuda.synchronize()
    ref = out64.clone()
    same = {}
    for k, fn in runs.items():
        if k in ("per_round", "f32_one"):
            continue
        out64.zero_()
        fn()
        torch.cuda.synchronize()
        same[k] = bool(torch.equal(ref.view(torch.int64), out64.view(torch.int64)))
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    step_bytes = N * W * 8 + W * 8
    batch = args.batch
    ms = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _b in range(batch):
                fn()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / batch)
    assert L.fa_rounds_timeouts(r32) == 0
    rec = {"clients": N, "params": args.params, "world": args.world, "widths": lay.widths, "local_width": W,
           "step_bytes": step_bytes, "batch": batch, "repeats": args.repeats, "autotune_pending": pending,
           "same_bits_as_per_round": same, "policy_now": L.fa_rounds_form_f64().decode(),
           "f32_form": L.fa_rounds_form(0).decode(), "device": torch.cuda.get_device_properties(dev).name}
    for k, v in ms.items():
        s = sorted(v)
        rec[k] = {"ms": [round(x, 5) for x in v], "median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1],
                  "spread_ms": s[-1] - s[0], "median_TBps": step_bytes / (s[len(s) // 2] * 1e-3) / 1e12}
    bal, sd = forms[0], forms[1]
    gap = rec[sd]["median_ms"] - rec[bal]["median_ms"]  # > 0: the balanced form is faster
    if gap < 0 and -gap > rec[bal]["spread_ms"]:
        pick = sd
    else:
        pick = bal  # faster by more than the pooled form's spread, or inside a spread: no dynamic pool
    rec["pooled_minus_balanced_median_ms"] = gap
    rec["policy_by_this_run"] = pick
    for a, b in ((pick, "per_round"), ("per_round", "pair_fold"), (pick, "f32_one")):
        rec[f"{a}_minus_{b}_median_ms"] = rec[a]["median_ms"] - rec[b]["median_ms"]
    for k in runs:
        print(f"{k:22s} median {rec[k]['median_ms']:.4f} ms  min-max {rec[k]['min_ms']:.4f}-{rec[k]['max_ms']:.4f} "
              f"({rec[k]['median_TBps']:.2f} TB/s)", flush=True)
    print(f"pooled - balanced: {gap:+.4f} ms (spreads {rec[bal]['spread_ms']:.4f} / {rec[sd]['spread_ms']:.4f}) -> "
          f"policy {pick};  same bits: {same}", flush=True)
    _lib.check(B.fa_bench_rounds_destroy(rb), "destroy", bench=True)
    _lib.check(L.fa_rounds_destroy(r32), "destroy")
    text = json.dumps(rec, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
