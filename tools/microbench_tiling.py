#!/usr/bin/env python3
"""Tiled inference (sr_amd.tiling, csrc/tile.hip) on the device: the measurements of INTEGRATION.md "Large images and self-ensemble".

  microbench_tiling.py --kernels   srk_tile_gather + srk_tile_place over the whole plan of one 339x510 LR image, x4, tile 48, pad 8, against
                                   the same work as a loop of torch slice copies (one copy per tile in, one per owned rectangle out); the
                                   two are timed alternately, median of --reps device-event timings after warm-up; outputs compared
  microbench_tiling.py --predict   predict_step of EDSR-baseline x4 on that image: whole against tiled for tile_batch in {1, 4, 16, 64}
  microbench_tiling.py --profile   only tiled predict_steps (for a `rocprofv3 --kernel-trace --stats` run)
  microbench_tiling.py --stats F   share of the two kernels in that run's kernel_stats.csv
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

H, W, SCALE, TILE, PAD = 339, 510, 4, 48, 8


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def alternate(fns, reps, warm=3):
    """{name: median us}: the candidates run in turn, `reps` rounds after `warm` untimed ones."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in times.items()}


def kernels(reps):
    from sr_amd import tiling as T
    p = T.plan(H, W, SCALE, TILE, PAD)
    n, s = len(p.tiles), SCALE
    g = torch.Generator().manual_seed(0)
    x = torch.rand(1, 3, H, W, generator=g).cuda()
    sr = torch.rand(n, 3, p.th * s, p.tw * s, generator=g).cuda()
    host, _ = T.device_table([(0, p)], H, W)
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    moh, mow = max(e.oh for e in host), max(e.ow for e in host)
    out_h = torch.empty(1, 3, H * s, W * s, device="cuda")
    out_t = torch.empty_like(out_h)
    tiles_t = torch.empty(n, 3, p.th, p.tw, device="cuda")
    res = {}

    def hip():
        res["tiles"] = T.gather(x, table, 0, n, p.th, p.tw)
        T.place(sr, out_h, table, 0, n, (H, W), p.th, p.tw, s, moh, mow)

    def torch_loop():
        for i, t in enumerate(p.tiles):
            tiles_t[i].copy_(x[0, :, t.y0:t.y0 + p.th, t.x0:t.x0 + p.tw])
        for i, t in enumerate(p.tiles):
            r0, r1, c0, c1 = p.owned_hr(t)
            out_t[0, :, r0:r1, c0:c1].copy_(sr[i, :, r0 - t.y0 * s:r1 - t.y0 * s, c0 - t.x0 * s:c1 - t.x0 * s])

    t = alternate({"hip_gather_place": hip, "torch_slice_copies": torch_loop}, reps)
    assert torch.equal(res["tiles"], tiles_t) and torch.equal(out_h, out_t)
    moved = 4 * (2 * tiles_t.numel() + 2 * out_h.numel())
    return {"case": f"{H}x{W} x{SCALE} tile {TILE} pad {PAD}", "tiles": n, "bytes_moved_MB": round(moved / 1e6, 1), **t,
            "hip_GB_per_s": round(moved / (t["hip_gather_place"]["median_us"] * 1e-6) / 1e9, 1),
            "torch_over_hip": round(t["torch_slice_copies"]["median_us"] / t["hip_gather_place"]["median_us"], 1)}


def _edsr(precision, **opts):
    import sr_amd
    torch.manual_seed(0)
    return sr_amd.EDSR(n_feats=64, n_resblocks=16, res_scale=0.1, scale_factor=SCALE, precision=precision, **opts).cuda().eval()


def predict(reps, precision):
    x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    whole = _edsr(precision)
    models = {"whole": whole}
    for tb in (1, 4, 16, 64):
        m = _edsr(precision, tile=TILE, tile_pad=PAD, tile_batch=tb)
        m.load_state_dict(whole.state_dict())
        models[f"tile_batch_{tb}"] = m

    def step(m):
        def run():
            with torch.no_grad():
                m.predict_step({"lr": x}, 0)
        return run
    t = alternate({k: step(m) for k, m in models.items()}, reps, warm=2)
    base = t["whole"]["median_us"]
    for k, v in t.items():
        v["over_whole"] = round(v["median_us"] / base, 2)
    return {"case": f"EDSR-baseline x{SCALE} {H}x{W} precision {precision} tile {TILE} pad {PAD}", **t}


def profile(iters, precision, tile_batch):
    x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    m = _edsr(precision, tile=TILE, tile_pad=PAD, tile_batch=tile_batch)
    with torch.no_grad():
        for _ in range(iters):
            m.predict_step({"lr": x}, 0)
    torch.cuda.synchronize()
    return {"profiled_predict_steps": iters, "tile_batch": tile_batch}


def stats(path):
    total, ours = 0.0, {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            total += ns
            for key in ("tile_gather_kernel", "tile_place_kernel"):
                if key in name:
                    ours[key] = {"calls": int(r["Calls"]), "total_us": round(ns / 1e3, 1), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
    mine = sum(v["total_us"] for v in ours.values()) * 1e3
    return {"all_kernels_us": round(total / 1e3, 1), "tile_kernels": ours, "share_of_kernel_time": round(mine / total, 5) if total else None}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kernels", action="store_true")
    p.add_argument("--predict", action="store_true")
    p.add_argument("--profile", action="store_true")
    p.add_argument("--stats", default=None)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--precision", default="bf16")
    p.add_argument("--tile_batch", type=int, default=16)
    a = p.parse_args()
    if a.stats:
        print(json.dumps(stats(a.stats)))
        return
    assert torch.cuda.is_available(), "needs the GPU"
    if a.kernels:
        print(json.dumps({"kernels": kernels(a.reps)}), flush=True)
    if a.predict:
        print(json.dumps({"predict": predict(a.reps, a.precision)}), flush=True)
    if a.profile:
        print(json.dumps({"profile": profile(5, a.precision, a.tile_batch)}), flush=True)


if __name__ == "__main__":
    main()
