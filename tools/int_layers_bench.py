#!/usr/bin/env python3
"""Integer layers of a device-resident model: the row-table route
(fa_fedavg_i64_ptrs / fa_fedavg_i64_layers) against the stacking route it
replaces.  The tool uses only entries both routes have (aggregate_layers,
ModelRowSet, fold_model_rows, RowSet, fold_rows), so the same file times a
checkout from before the row-table route: --repo names the tree to import.

Shapes, N = 100 clients, every client tensor its own device allocation:
  resnet18_bn   torchvision's ResNet-18 state_dict: 102 float32 tensors (21
                weight matrices and biases, 20 BatchNorm layers' weight, bias,
                running_mean, running_var) and 20 int64 num_batches_tracked
                scalars
  wide_i64      one int64 layer of 1M elements
Per shape, for FedAvg (no scores) and for stall-aware scores:
  full_ms       aggregate_layers over the whole model
  ints_ms       aggregate_layers over the integer layers alone
  prepared_ms   fold_model_rows over a ModelRowSet of the integer layers
GPU-event spans around the Python call on the current stream (host work
included whenever the GPU waits for it); warmed up, candidates interleaved
for --reps rounds; each figure the median with (min, max).

    python tools/int_layers_bench.py [--repo DIR] [--clients 100] [--reps 15] [--tag NAME] [--out FILE]
prints one JSON line per case and appends them to FILE when given.  (GPU box)
"""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--clients", type=int, default=100)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--tag", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.repo))
from fedlesscan_amd import engine, synth  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("int_layers_bench needs a GPU")
dev = torch.device("cuda", 0)
SEED = 9
INT = "i64"  # marks a BatchNorm layer's num_batches_tracked


def resnet18_state_dict():
    """Shapes in state_dict order; INT where the entry is the int64 counter."""
    def bn(c):
        return [(c,), (c,), (c,), (c,), INT]
    out = [(64, 3, 7, 7)] + bn(64)
    cin = 64
    for c in (64, 128, 256, 512):
        for block in range(2):
            out += [(c, cin if block == 0 else c, 3, 3)] + bn(c) + [(c, c, 3, 3)] + bn(c)
            if block == 0 and c != cin:
                out += [(c, cin, 1, 1)] + bn(c)  # the downsample branch
        cin = c
    return out + [(1000, 512), (1000,)]


def numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


RESNET18 = resnet18_state_dict()
assert len(RESNET18) == 122 and RESNET18.count(INT) == 20
assert sum(numel(s) for s in RESNET18 if s != INT) == 11689512 + 2 * 4800  # parameters and running statistics


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


def model(shapes, N, gen):
    def layer(s, i):
        if s == INT:  # the counter of a client that trained for 1000 + i batches
            return torch.tensor(1000 + i, dtype=torch.int64, device=dev)
        if isinstance(s, tuple) and s and s[0] == "wide":
            return torch.randint(-2 ** 62, 2 ** 62, (s[1],), dtype=torch.int64, device=dev, generator=gen)
        return torch.randn(s, device=dev, generator=gen) * 0.05
    return [[layer(s, i) for s in shapes] for i in range(N)]


CASES = {"resnet18_bn": RESNET18, "wide_i64": [("wide", 1 << 20)]}
N = args.clients
w = synth.cardinalities(SEED, N)
scores = [(r + 1) / 11 for r in synth.round_ids(SEED, N, 10, 2)]
lines = []
for name, shapes in CASES.items():
    gen = torch.Generator(device=dev).manual_seed(SEED)
    params = model(shapes, N, gen)
    ints = [k for k, s in enumerate(shapes) if s == INT or (isinstance(s, tuple) and s and s[0] == "wide")]
    only = [[cl[k] for k in ints] for cl in params]
    ms = engine.ModelRowSet(only)
    for form, sc in (("fedavg", None), ("stall_aware", scores)):
        before = dict(engine.stats)
        t = measure({"full": lambda: engine.aggregate_layers(params, w, sc),
                     "ints": lambda: engine.aggregate_layers(only, w, sc),
                     "prepared": lambda: engine.fold_model_rows(ms, w, sc)}, args.reps)
        rf, ri, rp = engine.aggregate_layers(params, w, sc), engine.aggregate_layers(only, w, sc), \
            engine.fold_model_rows(ms, w, sc)
        same = all(torch.equal(rf[k].view(torch.int64), a.view(torch.int64)) and
                   torch.equal(a.view(torch.int64), b.view(torch.int64)) for k, a, b in zip(ints, ri, rp))
        rec = {"tag": args.tag, "case": name, "form": form, "clients": N, "layers": len(shapes),
               "int_layers": len(ints), "reps": args.reps,
               "stacked_groups": engine.stats["stacked_groups"] - before["stacked_groups"]}
        for k in ("full", "ints", "prepared"):
            rec[k + "_ms"] = round(t[k][0], 4)
            rec[k + "_spread_ms"] = [round(x, 4) for x in t[k][1:]]
        rec["bit_identical_routes"] = bool(same)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    del params, only, ms
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
