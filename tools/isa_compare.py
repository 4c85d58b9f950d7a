#!/usr/bin/env python3
"""Two device listings of the same source (`hipcc ... -S --cuda-device-only`, before and after a change), kernel by kernel: one line
per kernel with its register counts and scratch in both, whether the instruction streams are the same once labels and comments are
stripped, and, where they are not, whether at least the per-mnemonic instruction counts are.

    python tools/isa_compare.py before.s after.s            exit status 1 if any kernel is `DIFFERENT` or exists on one side only

  identical    the same instructions in the same order with the same operands
  rescheduled  another order or other registers, but the same register counts, scratch and number of every mnemonic
  DIFFERENT    a count differs"""
import collections
import re
import sys

META = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size")
LABEL = re.compile(r"^[.\w$]+:")


def kernels(path):
    """{name: (instruction lines, {metadata field: value})}"""
    out, meta, name, body = {}, {}, None, []
    record = None                                    # the metadata record being read (amdhsa.kernels: one `  - ` item per kernel)
    for raw in open(path):
        if record is not None:
            if raw.startswith("  - "):
                record = {}
            m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)$", raw)
            if m and m.group(1) in META:
                record[m.group(1)] = int(m.group(2))
            elif m and m.group(1) == "name" and m.group(2) in out:
                meta[m.group(2)] = record
            continue
        if raw.startswith("amdhsa.kernels:"):
            record = {}
            continue
        line = raw.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            out[m.group(1)] = body
            name = None
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None or not line or LABEL.match(line) or line.startswith("."):
            continue
        body.append(re.sub(r"\.LBB\d+_\d+", "L", " ".join(line.split())))
    return {k: (v, meta.get(k, {})) for k, v in out.items()}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    tally = collections.Counter()
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{'ONLY IN ' + sys.argv[1 if k in a else 2]:11s} {k}")
            bad += 1
            continue
        (ia, ma), (ib, mb) = a[k], b[k]
        same_meta = ma == mb and len(ma) == len(META)
        if ia == ib and same_meta:
            verdict = "identical"
        elif same_meta and collections.Counter(i.split()[0] for i in ia) == collections.Counter(i.split()[0] for i in ib):
            verdict = "rescheduled"
        else:
            verdict = "DIFFERENT"
            bad += 1
        tally[verdict] += 1
        counts = " ".join(f"{f.split('_')[0][:7]} {ma.get(f)}" + ("" if ma.get(f) == mb.get(f) else f"->{mb.get(f)}") for f in META)
        print(f"{verdict:11s} {counts}  insns {len(ia)}" + ("" if len(ia) == len(ib) else f"->{len(ib)}") + f"  {k}")
    print(f"{len(set(a) | set(b))} kernels: " + ", ".join(f"{n} {v}" for v, n in sorted(tally.items())))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
