#!/usr/bin/env python3
"""Diagnostic: lk5_wgrad_kernel alone at the collapsed HR stage's shape (n x 96 x 96, 64 input x 16 stored gradient channels, bf16).
Prints the launch time (HIP events, median of 20) and, with the stamp build (make -C .../csrc stamp), the s_memtime stamps of wave 0 of
workgroup 0 per tile.  --dump FILE saves the slabs ([slab][tap][ci][16] and the bias slabs) the launch wrote, to compare two builds
bit for bit.  usage: tools/stamp_lk5w.py [n] [--dump FILE]     (SRK_LIB_PATH picks the library; default: the stamp build)"""
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
x = (torch.rand(n, 96, 96, 64, generator=gen) - 0.5).to(dt).to(dev)
g12 = (torch.rand(n, 96, 96, 16, generator=gen) - 0.5).to(dt).to(dev)
g12[..., 12:] = 0
a = L.WgradArgs(x=x.data_ptr(), x_pitch=64, x_coff=0, x_ps=0, dy=g12.data_ptr(), dy_pitch=16, dy_coff=0, dy_ps=0,
                N=n, H=96, W=96, Cin=64, Cout=16, KH=5, KW=5, dwp=0, dbp=0, nslabs=0, dtype=L.SRK_BF16, cout_real=12)
ns = L.load().srk_wgrad_slabs(a)
per = 25 * 64 * 16
scratch = torch.zeros(ns * (per + 16) + 2 * 24 * 8, dtype=torch.float32, device=dev)      # slabs, bias slabs, 24 x 8 64-bit stamps
a.dwp, a.dbp, a.nslabs = scratch.data_ptr(), scratch[ns * per:].data_ptr(), ns
st = torch.cuda.current_stream().cuda_stream
for _ in range(3):
    L.call("srk_conv2d_wgrad", a, st)
torch.cuda.synchronize()
times = []
for _ in range(20):
    scratch[ns * (per + 16):].zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); L.call("srk_conv2d_wgrad", a, st); e1.record(); torch.cuda.synchronize()
    times.append(e0.elapsed_time(e1) * 1e3)
print(f"{os.path.basename(L.LIB_PATH)}: launch {np.median(times):.1f} us (min {min(times):.1f}, max {max(times):.1f}), {ns} slabs")
if dump:
    np.save(dump, scratch[:ns * (per + 16)].cpu().numpy())
stamps = scratch[ns * (per + 16):].cpu().view(torch.int64).numpy().reshape(24, 8)
if stamps[0, 0]:
    print("s_memtime ticks relative to tile 0's first stamp")
    print("tile   start  waited barrier rows-begin mfma-done | tile length")
    t0 = stamps[0, 0]
    for s in range(24):
        if stamps[s, 0] == 0: break
        r = stamps[s] - t0
        nxt = (stamps[s + 1, 0] - stamps[s, 0]) if s + 1 < 24 and stamps[s + 1, 0] else 0
        print(f"{s:4d} {r[0]:7d} {r[1]:7d} {r[2]:7d} {r[3]:10d} {r[4]:9d} | {nxt}")
else:
    print("(no stamps: not the stamp build)")
