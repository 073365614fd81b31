#!/usr/bin/env python3
"""Compare two builds of the device code kernel by kernel.

    hipcc <native_build.HIPCC_FLAGS without -shared/-fPIC> --cuda-device-only -S \
          -I include -o old.s fedlesscan_amd/csrc/fedavg.hip      (at the old commit)
    ... the same at the new commit -> new.s
    tools/kernel_isa_diff.py old.s new.s [--show KERNEL_SUBSTRING]

Both files are split at the kernel labels; comments are stripped and local
label names renumbered in order of appearance.  Per kernel one verdict:

    identical   the same instruction text
    same-shape  the same opcode histogram and the same register budget
                (.amdhsa_next_free_vgpr / _sgpr), private-segment and
                group-segment size: operand order, register numbers, label
                order or the sense of a compare-and-branch pair may differ
                (the histogram counts an inverted compare (eq/ne, lt/ge,
                gt/le and no other change of predicate), its branch and the
                and/or-not mask operation between them as the ones they
                invert, ignores the _e32/_e64 encoding suffix and s_nop
                padding)
    different   anything else

A generic text diff of two builds: it looks for no particular instruction.
Exit status 0 when the kernel sets are equal and no kernel is "different".
"""
import argparse
import collections
import difflib
import re
import sys

META = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(path):
    """{name: (normalised instruction lines, {meta: value})} of one .s file."""
    text, meta = {}, {}
    name = desc = body = None  # the function announced by .type, the open descriptor, the open body
    with open(path) as f:
        lines = f.read().splitlines()
    for raw in lines:
        s = raw.split(";", 1)[0].strip()
        if not s:
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            desc = meta[m.group(1)] = {}
        elif s == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", s)
            if m and m.group(1) in META:
                desc[m.group(1)] = m.group(2)
        elif body is not None:
            if s.startswith(".Lfunc_end"):
                name = body = None
            elif not s.startswith(".") or LABEL.match(s):
                body.append(s)
        elif re.match(r"\.type\s+(\S+),@function", s):
            name = re.match(r"\.type\s+(\S+),@function", s).group(1)
        elif name is not None and s == name + ":":
            body = text[name] = []
    out = {}
    for k, v in text.items():
        if k not in meta:
            continue  # a device function, not a kernel
        names = {}
        norm = [LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln) for ln in v]
        out[k] = (norm, meta[k])
    return out


SENSE = [  # an inverted compare-and-branch pair counts as the pair it inverts
    (re.compile(r"^([sv]_cmpx?)_(?:ne|lg)_"), r"\1_eq_"),  # only a predicate and its inverse fold: eq = ne,
    (re.compile(r"^([sv]_cmpx?)_ge_"), r"\1_lt_"),        # lt = ge,
    (re.compile(r"^([sv]_cmpx?)_le_"), r"\1_gt_"),        # gt = le
    (re.compile(r"^s_cbranch_(scc|vcc|exec)n?[01z]$"), r"s_cbranch_\1"),
    (re.compile(r"^s_(and|or)n2_"), r"s_\1_"),  # the mask operation that consumes the inverted compare
    (re.compile(r"_e(?:32|64)$"), ""),  # the encoding follows the registers the result lands in
]


def histogram(lines):
    ops = collections.Counter()
    for ln in lines:
        op = ln.split()[0]
        if ln.endswith(":") or op == "s_nop":  # labels; padding the scheduler inserts
            continue
        for pat, to in SENSE:
            op = pat.sub(to, op)
        ops[op] += 1
    return ops


def verdict(a, b):
    if a[0] == b[0] and a[1] == b[1]:
        return "identical"
    if a[1] == b[1] and histogram(a[0]) == histogram(b[0]):
        return "same-shape"
    return "different"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", metavar="SUBSTRING", help="print the diff of the non-identical kernels whose name has it")
    ap.add_argument("--quiet", action="store_true", help="do not list identical kernels")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    for k in sorted(set(old) - set(new)):
        print("missing    ", k)
    for k in sorted(set(new) - set(old)):
        print("added      ", k)
    count = collections.Counter()
    for k in sorted(set(old) & set(new)):
        v = verdict(old[k], new[k])
        count[v] += 1
        if v != "identical" or not args.quiet:
            print("%-11s %s" % (v, k))
        if v != "identical" and args.show is not None and args.show in k:
            for m in META:
                if old[k][1].get(m) != new[k][1].get(m):
                    print("    %s: %s -> %s" % (m, old[k][1].get(m), new[k][1].get(m)))
            print("\n".join("    " + d for d in difflib.unified_diff(old[k][0], new[k][0], "old", "new", lineterm="", n=1)))
    print("%d kernels old, %d new: %d identical, %d same-shape, %d different" %
          (len(old), len(new), count["identical"], count["same-shape"], count["different"]))
    return 0 if set(old) == set(new) and not count["different"] else 1


if __name__ == "__main__":
    sys.exit(main())
