#!/usr/bin/env python3
"""The float16 fold next to the bf16 fold of equal HBM traffic and the read
sweep, in one process, inputs in HBM.

Per shape (256 x 12.5M, 256 x 100M, 1024 x 67K by default): fa_fedavg_f16,
fa_fedavg_bf16 with out_bf16 only (both read N*P*2 bytes and write P*2) and
fa_read_sweep_f32 over the same buffer.  Each is warmed up (the tuner measures
the shape on the first call; timing starts once fa_autotune_pending() == 0),
then `--repeats` windows of `--batch` back-to-back launches between two events,
the three interleaved within a repeat.  The two folds run on the same bytes:
the rows are random halves in +-2^-3 (finite, no subnormal flood), which read
as bf16 are finite values too.

    python tools/f16_fold_bench.py [--shapes 256x12500000,1024x67000] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedlesscan_amd import _lib, synth  # noqa: E402

FA_FOLD_BF16, FA_FOLD_F16 = 2, 4


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
    ap.add_argument("--shapes", default="256x12500000,256x100000000,1024x67000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=0, help="launches per timed window (0: ~50 ms of work, 3..200)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L, B = _lib.load(), _lib.load_bench()
    st = torch.cuda.current_stream(dev)
    sp = st.cuda_stream
    results = []
    for shape in args.shapes.split(","):
        N, P = (int(v) for v in shape.lower().split("x"))
        ldx = (P + 63) // 64 * 64
        X = torch.empty((N, ldx), dtype=torch.float16, device=dev)
        fill_rows(X, 5)
        w = synth.cardinalities(5, N)
        with np.errstate(over="ignore"):
            a16 = torch.from_numpy(np.array(w, np.float64).astype(np.float16).view(np.int16)).to(dev)
            d16 = int(np.float16(sum(w)).view(np.uint16))
        a32 = torch.tensor(np.array(w, np.float32), device=dev)
        d32 = float(np.float32(sum(w)))
        out16 = torch.empty(P, dtype=torch.float16, device=dev)
        outb = torch.empty(P, dtype=torch.bfloat16, device=dev)
        sink = torch.empty(4096, dtype=torch.float32, device=dev)
        nsweep = N * ldx // 2  # the buffer as floats

        def f16():
            _lib.check(L.fa_fedavg_f16(X.data_ptr(), N, P, ldx, a16.data_ptr(), None, d16, out16.data_ptr(), sp),
                       "fa_fedavg_f16")

        def bf16():
            _lib.check(L.fa_fedavg_bf16(X.data_ptr(), N, P, ldx, a32.data_ptr(), None, d32, None, outb.data_ptr(),
                                        sp), "fa_fedavg_bf16")

        def sweep():
            _lib.check(B.fa_read_sweep_f32(X.data_ptr(), nsweep, sink.data_ptr(), sink.numel(), sp), "read sweep",
                       bench=True)

        runs = {"f16": f16, "bf16": bf16, "read_sweep": sweep}
        for _ in range(20):  # warm-up; the tuner's measurement of the shape completes here
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
        fold_bytes = N * P * 2 + P * 2
        sweep_bytes = nsweep * 4
        batch = args.batch or int(min(200, max(3, 0.05 / (fold_bytes / 4.0e12))))
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
        rec = {"N": N, "P": P, "ldx": ldx, "batch": batch, "repeats": args.repeats, "autotune_pending": pending,
               "forms": {"f16": L.fa_fold_form(FA_FOLD_F16, N, P, ldx, 0, sp).decode(),
                         "bf16": L.fa_fold_form(FA_FOLD_BF16, N, P, ldx, 0, sp).decode()}}
        for k, v in ms.items():
            nbytes = sweep_bytes if k == "read_sweep" else fold_bytes
            s = sorted(v)
            rec[k] = {"ms": [round(x, 5) for x in v], "median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1],
                      "median_TBps": nbytes / (s[len(s) // 2] * 1e-3) / 1e12}
        spread = rec["bf16"]["max_ms"] - rec["bf16"]["min_ms"]
        rec["bf16_spread_ms"] = spread
        rec["f16_minus_bf16_median_ms"] = rec["f16"]["median_ms"] - rec["bf16"]["median_ms"]
        rec["f16_within_bf16_spread"] = rec["f16_minus_bf16_median_ms"] <= spread
        results.append(rec)
        print(f"{N} x {P}: f16 {rec['f16']['median_ms']:.4f} ms ({rec['f16']['median_TBps']:.2f} TB/s, "
              f"{rec['forms']['f16']})  bf16 {rec['bf16']['median_ms']:.4f} ms ({rec['bf16']['median_TBps']:.2f} TB/s, "
              f"{rec['forms']['bf16']}, spread {spread:.4f} ms)  read sweep {rec['read_sweep']['median_ms']:.4f} ms "
              f"({rec['read_sweep']['median_TBps']:.2f} TB/s)  f16 within the bf16 spread: "
              f"{rec['f16_within_bf16_spread']}", flush=True)
        del X, out16, outb
        torch.cuda.empty_cache()
    text = json.dumps(results, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
