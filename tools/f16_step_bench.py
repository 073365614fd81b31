#!/usr/bin/env python3
"""The float16 one-launch step next to its per-round launches and the bf16
one-launch step of equal bytes, in one process at world 1, inputs in HBM.

A C4 rank's shape: overlap_layout(100_000_000, 8, "f16"), 256 clients, its four
slots side by side.  Three variants over the same bytes:
  one_launch  fa_fedavg_f16_rounds (every round in one launch)
  per_round   the same rounds as four fa_fedavg_f16 launches with staged factors
  bf16_one    fa_fedavg_bf16_rounds with out_bf16 only (equal bytes in and out)
Everything is warmed first (the tuner measures each round's shape on its first
calls; timing starts once fa_autotune_pending() == 0), then `--repeats` windows
of `--batch` back-to-back steps between two events, the variants interleaved
within a repeat; median and min-max per variant, each difference stated against
the other variant's own spread.

    python tools/f16_step_bench.py [--clients 256] [--params 100000000] [--repeats 7] [--out FILE]
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
    """x = +-2^-3 * U(0, 1) as float16, generated on the device a few rows at a time."""
    g = torch.Generator(device=X.device)
    g.manual_seed(seed)
    N, ldx = X.shape
    step = max(1, (1 << 27) // max(ldx, 1))
    for i in range(0, N, step):
        n = min(step, N - i)
        r = torch.rand((n, ldx), generator=g, device=X.device, dtype=torch.float32)
        X[i:i + n].copy_(((r - 0.5) * 0.25).to(torch.float16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=256)
    ap.add_argument("--params", type=int, default=100_000_000)
    ap.add_argument("--world", type=int, default=8, help="the layout's world size (the run itself is one process)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=0, help="steps per timed window (0: ~50 ms of work, 3..200)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.load()
    st = torch.cuda.current_stream(dev)
    sp = st.cuda_stream
    N = args.clients
    lay = overlap_layout(args.params, args.world, "f16")
    W, R = lay.local_width, lay.rounds
    offs = [lay.offset(k) for k in range(R + 1)]
    coffs = (ctypes.c_int64 * (R + 1))(*offs)
    X = torch.empty((N, W), dtype=torch.float16, device=dev)
    fill_rows(X, 5)  # +-2^-3 * U(0, 1): finite halves, and finite values read as bf16 too
    w = [1 + c % 5 for c in synth.cardinalities(5, N)]  # 1..5: the binary16 divisor stays finite
    with np.errstate(over="ignore"):
        a16 = torch.from_numpy(np.array(w, np.float64).astype(np.float16).view(np.int16)).to(dev)
        d16 = int(np.float16(sum(w)).view(np.uint16))
    a32 = torch.tensor(np.array(w, np.float32), device=dev)
    d32 = float(np.float32(sum(w)))
    out16 = torch.empty(W, dtype=torch.float16, device=dev)
    outb = torch.empty(W, dtype=torch.bfloat16, device=dev)
    r16, rb = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(L.fa_rounds_create(ctypes.byref(r16), dev.index), "fa_rounds_create")
    _lib.check(L.fa_rounds_create(ctypes.byref(rb), dev.index), "fa_rounds_create")

    def one_launch():
        _lib.check(L.fa_fedavg_f16_rounds(r16, X.data_ptr(), N, W, a16.data_ptr(), None, d16, out16.data_ptr(), R,
                                          coffs, None, sp), "fa_fedavg_f16_rounds")

    def per_round():
        for k in range(R):
            _lib.check(L.fa_fedavg_f16(X.data_ptr() + 2 * offs[k], N, offs[k + 1] - offs[k], W, a16.data_ptr(), None,
                                       d16, out16.data_ptr() + 2 * offs[k], sp), "fa_fedavg_f16")

    def bf16_one():
        _lib.check(L.fa_fedavg_bf16_rounds(rb, X.data_ptr(), N, W, a32.data_ptr(), None, d32, None, outb.data_ptr(),
                                           R, coffs, None, sp), "fa_fedavg_bf16_rounds")

    runs = {"one_launch": one_launch, "per_round": per_round, "bf16_one": bf16_one}
    for _ in range(20):  # warm-up; the tuner's measurement of each round's shape completes here
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        if L.fa_autotune_pending() == 0:
            break
    pending = L.fa_autotune_pending()
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the one launch and the per-round launches computed the same bits
    ref = out16.clone()
    per_round()
    torch.cuda.synchronize()
    same = bool(torch.equal(ref.view(torch.int16), out16.view(torch.int16)))
    step_bytes = N * W * 2 + W * 2
    batch = args.batch or int(min(200, max(3, 0.05 / (step_bytes / 4.0e12))))
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
    assert L.fa_rounds_timeouts(r16) == 0 and L.fa_rounds_timeouts(rb) == 0
    rec = {"clients": N, "params": args.params, "world": args.world, "widths": lay.widths, "local_width": W,
           "batch": batch, "repeats": args.repeats, "autotune_pending": pending, "same_bits_one_vs_per_round": same,
           "forms": {"one_launch": L.fa_rounds_form_f16().decode(), "bf16_one": L.fa_rounds_form(1).decode()},
           "device": torch.cuda.get_device_properties(dev).name}
    for k, v in ms.items():
        s = sorted(v)
        rec[k] = {"ms": [round(x, 5) for x in v], "median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1],
                  "spread_ms": s[-1] - s[0], "median_TBps": step_bytes / (s[len(s) // 2] * 1e-3) / 1e12}
    for a, b in (("one_launch", "per_round"), ("one_launch", "bf16_one")):
        d = rec[a]["median_ms"] - rec[b]["median_ms"]
        rec[f"{a}_minus_{b}_median_ms"] = d
        rec[f"{a}_within_{b}_spread"] = abs(d) <= rec[b]["spread_ms"]
    for k in runs:
        print(f"{k:11s} median {rec[k]['median_ms']:.4f} ms  min-max {rec[k]['min_ms']:.4f}-{rec[k]['max_ms']:.4f} "
              f"({rec[k]['median_TBps']:.2f} TB/s)", flush=True)
    print(f"one launch - per round: {rec['one_launch_minus_per_round_median_ms']:+.4f} ms (per-round spread "
          f"{rec['per_round']['spread_ms']:.4f});  one launch - bf16 one launch: "
          f"{rec['one_launch_minus_bf16_one_median_ms']:+.4f} ms (bf16 spread {rec['bf16_one']['spread_ms']:.4f});  "
          f"same bits: {same}", flush=True)
    _lib.check(L.fa_rounds_destroy(r16), "destroy")
    _lib.check(L.fa_rounds_destroy(rb), "destroy")
    text = json.dumps(rec, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
