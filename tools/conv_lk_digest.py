#!/usr/bin/env python3
"""One SHA-256 per case over everything the large-kernel convolutions of csrc/conv_lk.hip compute: two builds of the library
(`SRK_LIB_PATH=... python tools/conv_lk_digest.py`, each in a fresh process) compute the same thing iff every line matches.  Every kernel
of that file is deterministic (slabs and a finalize launch, no atomics), so the lines of two builds that sum in the same order are equal.

The cases are those of tests/test_gpu_conv_lk_elements.py in both dtypes: the direct convolutions through autograd (digest over the output,
the data gradient, the weight gradient and the bias gradient) and the collapsed HR stage's forward kernel (over the image).  A line also
names the kernels that ran (srk_last_kernel()).  An A/B knob of tools/README.md is read once per process: run the tool once more per
`SRK_DEBUG=1 SRK_NO_LK...=1` for the other side of each dispatch decision."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

LK_CASES = [(9, 3, 2, 40, 33), (9, 1, 1, 35, 20), (5, 6, 1, 33, 33), (7, 4, 2, 16, 47), (7, 16, 2, 17, 30), (5, 8, 1, 21, 19), (5, 12, 3, 48, 48),
            (5, 3, 1, 17, 18), (9, 16, 1, 17, 18)]
COLLAPSED_CASES = [(3, 2, 96, 96), (3, 3, 37, 61), (3, 1, 5, 29), (2, 2, 16, 28), (1, 1, 9, 57), (3, 17, 48, 48), (4, 2, 20, 33)]


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("conv_lk_digest.py runs the GPU kernels: no GPU here")
    import sr_amd
    import dispatch_cases as D
    knobs = " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("SRK_NO_LK")) if os.environ.get("SRK_DEBUG") == "1" else ""
    print("library", os.path.basename(sr_amd._lib.LIB_PATH), "knobs", knobs or "-", flush=True)
    seen = set()
    with D.Recorder() as rec:
        for dt in (torch.bfloat16, torch.float16):
            for (k, cout, n, h, w) in LK_CASES:
                outs, _, kern = D.lk_run(rec, dt, k, cout, n, h, w)
                seen.update(kern.values())
                print(f"lk {str(dt)[6:]:9s} k{k} cout{cout:<2d} {n}x{h}x{w:<3d} {digest(*outs)}  {kern['fwd']} {kern['dgrad']} {kern['wgrad']}", flush=True)
            for (O, n, h, w) in COLLAPSED_CASES:
                rec.take()
                got, _ = D.collapsed_fwd_one(dt, O, n, h, w)
                name = D._names(rec.take(), "srk_conv2d")[-1]
                seen.add(name)
                print(f"collapsed {str(dt)[6:]:9s} O{O} {n}x{h}x{w:<3d} {digest(got)}  {name}", flush=True)
    print("kernels", " ".join(sorted(seen)), flush=True)


if __name__ == "__main__":
    main()
