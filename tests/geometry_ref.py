"""Shared helpers of the launch-geometry tests (test_gpu_step_geometry.py, test_gpu_step_geometry_models.py) -- TEST
INFRASTRUCTURE, never imported by the product: exact 16-bit operands, the per-element / reduction bounds, the batch geometries
and the choice of images a float64 CPU reference is computed for."""
import torch


def _geom(cus, which, hr=False):
    """(N, H, W): 'bench' = the bench step's shape; 'ragged' = every workgroup walks >= 2 units with a nonzero remainder."""
    if which == "bench":
        return (cus, 96, 96) if hr else (cus, 48, 48)
    return (cus + 37, 94, 100) if hr else (cus + 37, 47, 50)


def _ex(shape, gen, p, lo=-127, hi=127):
    """Seeded values k * 2**-p, lo <= k <= hi, |k| < 128: exact in bf16 and in fp16."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen).double() * 2.0 ** -p


def _eps(dt):
    return 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11         # half an ulp of the storage type, relative


def _check16(got, ref, dt, what):
    """The per-element bound of test_gpu_ws_epilogue.py: 1.5 half-ulps of the storage type, relative, plus a small absolute term."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite elements (a tile never written?)"
    eps = _eps(dt)
    m = float(ref.abs().max())
    tol = eps * ref.abs() * 1.5 + 4e-3 * eps + 1e-3 * m * (1 if dt == torch.bfloat16 else 0.1)
    err = (got - ref).abs()
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements out of bound, max err {float(err.max()):.3e} (max |ref| {m:.3f}), first at {bad.nonzero()[0].tolist()}"


def _relerr(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _check32(got, ref, what, rel=5e-5, elem=1e-4):
    """fp32 reduction: relative norm error and a per-element bound against the largest element."""
    got = got.double().cpu()
    ref = ref.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite"
    e = _relerr(got, ref)
    m = float(ref.abs().max())
    emax = float((got - ref).abs().max())
    assert e <= rel, f"{what}: relative error {e:.3e} > {rel:.1e}"
    assert emax <= elem * m + 1e-9, f"{what}: max element error {emax:.3e} > {elem:.1e} * {m:.3e}"


def _pick(n, tiles_per_img, ntiles, slots, k=16, seed=0):
    """Images to compare: first, last, the images holding the first tile of slots trem - 1 and trem, seeded others."""
    tq, trem = divmod(ntiles, slots)
    s = {0, n - 1}
    if trem:
        for slot in (trem - 1, trem):
            s.add((slot * tq + min(slot, trem)) // tiles_per_img)
    g = torch.Generator().manual_seed(seed)
    for i in torch.randperm(n, generator=g).tolist():
        if len(s) >= min(k, n):
            break
        s.add(i)
    return sorted(s)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _ws_premise(cus, n, h, w, coutp):
    """launch_ws (conv_igemm.hip): slots = cus / ctiles workgroups per 64-channel tile, each walks tq (+1) of the 16x16 tiles."""
    tiles_img = -(-h // 16) * -(-w // 16)
    ntiles = n * tiles_img
    slots = min(max(cus // (coutp // 64), 1), ntiles)
    assert ntiles // slots >= 2, f"premise: {ntiles} tiles over {slots} slots is not the multi-tile walk"
    return tiles_img, ntiles, slots
