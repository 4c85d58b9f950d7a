#!/usr/bin/env python3
"""Diagnostic: the slab-mode 3x3 weight gradient alone, single launch (n x 48 x 48, 64 -> 64, bf16; n >= 114 runs the 8-row form with helper waves).
Prints the launch time (HIP events, median of 20) and, with the stamp build (make -C .../csrc stamp), two s_memtime stamps per tile of compute
wave 0 and of helper wave 4 of workgroup 0: at the top of the tile and in front of the tile's barrier (tile period and barrier wait of the two roles).  --dump FILE saves the slabs and bias
slabs the launch wrote, to compare two builds bit for bit.
usage: tools/stamp_wg.py [n] [--dump FILE]     (SRK_LIB_PATH picks the library; default: the stamp build)"""
import os, sys
os.environ.setdefault("SRK_LIB_PATH", os.path.join(os.path.dirname(os.path.abspath(__file__)), "ubench", "libsrk_stamp.so"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, sr_amd as A
argv = sys.argv[1:]
dump = argv[argv.index("--dump") + 1] if "--dump" in argv else None
pos = [v for i, v in enumerate(argv) if v != "--dump" and (i == 0 or argv[i - 1] != "--dump")]
n = int(pos[0]) if pos else 256
L = A._lib
dev, dt = torch.device("cuda"), torch.bfloat16
gen = torch.Generator().manual_seed(0)
x = (torch.rand(n, 48, 48, 64, generator=gen) - 0.5).to(dt).to(dev)
dy = (torch.rand(n, 48, 48, 64, generator=gen) - 0.5).to(dt).to(dev)
a = L.WgradArgs(x=x.data_ptr(), x_pitch=64, x_coff=0, x_ps=0, dy=dy.data_ptr(), dy_pitch=64, dy_coff=0, dy_ps=0,
                N=n, H=48, W=48, Cin=64, Cout=64, KH=3, KW=3, dwp=0, dbp=0, nslabs=0, dtype=L.SRK_BF16, cout_real=64)
ns = L.load().srk_wgrad_slabs(a)
per = 9 * 64 * 64
NST = 32
scratch = torch.zeros(ns * (per + 64) + 2 * 2 * 2 * NST, dtype=torch.float32, device=dev)      # slabs, bias slabs, 2 roles x 32 tiles x 2 64-bit stamps
a.dwp, a.dbp, a.nslabs = scratch.data_ptr(), scratch[ns * per:].data_ptr(), ns
st = torch.cuda.current_stream().cuda_stream
for _ in range(3):
    L.call("srk_conv2d_wgrad", a, st)
torch.cuda.synchronize()
times = []
for _ in range(20):
    scratch[ns * (per + 64):].zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); L.call("srk_conv2d_wgrad", a, st); e1.record(); torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3)
print(f"{os.path.basename(L.LIB_PATH)}: launch {np.median(times):.1f} us (min {min(times):.1f}, max {max(times):.1f}), {ns} slabs, "
      f"{n * 6 * 3 // ns} tiles of 8 rows per workgroup")
if dump:
    np.save(dump, scratch[:ns * (per + 64)].cpu().numpy())
stamps = scratch[ns * (per + 64):].cpu().view(torch.int64).numpy().reshape(2, NST, 2)
if stamps[0, 0, 0]:
    print("s_memtime ticks relative to compute wave 0's first tile; work = top of the tile to its barrier, wait = barrier to the top of the next tile")
    print("tile | compute: top  period   work   wait | helper: top  period   work   wait")
    t0 = stamps[0, 0, 0]
    for s in range(NST):
        if stamps[0, s, 0] == 0: break
        row = f"{s:4d} |"
        for r in (0, 1):
            top, bar = stamps[r, s]
            nxt = stamps[r, s + 1, 0] if s + 1 < NST and stamps[r, s + 1, 0] else 0
            row += f" {top - t0:12d} {nxt - top if nxt else 0:7d} {bar - top:6d} {nxt - bar if nxt else 0:6d} |"
        print(row)
else:
    print("(no stamps: not the stamp build)")
