#!/usr/bin/env python3
"""Generate the FLIP golden vectors (tests/golden/flip_*.npz) from the REFERENCE's own losses/flip.py.

Runs only in the build container (needs the reference checkout); nothing here is imported by the tests, the bench or
the product.  The reference's FLIP is written for a CUDA device (`.cuda()` on every filter, `device='cuda'` on its
scratch tensors); on the CPU it runs unchanged with two shims:
  * `torch.Tensor.cuda` is the identity while the reference runs;
  * the module's `torch` is a proxy whose `zeros` drops `device=`.
Every FLOP is the reference's own code on torch's CPU ops, in fp32 (its filters are always fp32, so float64 inputs
make its conv2d raise).  Written per case: the inputs, the error map (`compute_flip` before the mean), the loss, the
gradient of the loss w.r.t. `sr` (NaN entries included: the reference's gradient is NaN where the filtered colours of
the two images coincide), the fp32 filters the reference convolves with and `cmax`.

    python tests/golden/generate_flip_golden.py
"""
import importlib.util
import os
import types

import numpy as np
import torch

REF = os.environ.get("SR_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_flip", os.path.join(REF, "losses", "flip.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    proxy = types.ModuleType("torch_cpu_proxy")
    proxy.__dict__.update({k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")})

    def zeros(*a, **k):
        k.pop("device", None)
        return torch.zeros(*a, **k)
    proxy.zeros = zeros
    mod.torch = proxy
    return mod


def cases():
    g = torch.Generator().manual_seed(20201)
    out = {}
    out["random_2x48x48"] = (torch.rand(2, 3, 48, 48, generator=g), torch.rand(2, 3, 48, 48, generator=g))
    hr = torch.rand(2, 3, 48, 48, generator=g)
    hr[:, :, 2:30, 4:34] = 1.0                                   # saturated plateaus (white and black)
    hr[:, 1:, 32:46, 20:44] = 0.0
    sr = hr + 0.05 * torch.randn(hr.shape, generator=g)
    sr[:, :, 2:30, 4:34] = 1.0 + 0.05 * torch.rand(2, 3, 28, 30, generator=g)    # clipped to hr's white: NaN gradients in the reference
    out["plateau_2x48x48"] = (sr, hr)
    hr = torch.rand(2, 3, 48, 48, generator=g)
    out["outofrange_2x48x48"] = (1.3 * hr - 0.1, hr)
    hr = torch.rand(2, 3, 48, 48, generator=g)
    sr = torch.rand(2, 3, 48, 48, generator=g)
    sr[:, :, :, 24:] = hr[:, :, :, 24:]
    out["halfequal_2x48x48"] = (sr, hr)
    hr = torch.rand(1, 3, 7, 5, generator=g)
    out["tiny_1x7x5"] = ((hr + 0.1 * torch.randn(hr.shape, generator=g)).clamp(0, 1), hr)
    hr = torch.rand(1, 3, 85, 123, generator=g)
    out["odd_1x85x123"] = ((hr + 0.1 * torch.randn(hr.shape, generator=g)), hr)
    return out


def main():
    torch.set_num_threads(8)                 # the thread count every fixture here is generated with
    ref = load_reference()
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        m = ref.FLIP()
        ppd = m.pixels_per_degree
        s_a, r_c = ref.generate_spatial_filter(ppd, "A")
        s_rg, _ = ref.generate_spatial_filter(ppd, "RG")
        s_by, _ = ref.generate_spatial_filter(ppd, "BY")
        # the feature filters as feature_detection builds them (it does not return them): recorded through F.conv2d
        seen = []
        real_conv = ref.F.conv2d
        ref.F = types.SimpleNamespace(**{k: getattr(torch.nn.functional, k) for k in ("pad",)},
                                      conv2d=lambda x, w, **k: (seen.append(w.clone()), real_conv(x, w, **k))[1])
        y = torch.rand(1, 1, 24, 24)
        ref.feature_detection(y, ppd, "edge")
        ref.feature_detection(y, ppd, "point")
        ref.F = torch.nn.functional
        edge, point = seen[0], seen[2]
        for name, (sr, hr) in cases().items():
            sr = sr.float().contiguous().requires_grad_(True)
            hr = hr.float().contiguous()
            err = m.compute_flip(hr, sr, ppd)
            loss = err.mean()
            loss.backward()
            cmax_t = torch.pow(ref.hyab(ref.hunt_adjustment(ref.color_space_transform(torch.tensor([[[0.0]], [[1.0]], [[0.0]]]).unsqueeze(0), "linrgb2lab")),
                                        ref.hunt_adjustment(ref.color_space_transform(torch.tensor([[[0.0]], [[0.0]], [[1.0]]]).unsqueeze(0), "linrgb2lab"))), m.qc)
            path = os.path.join(OUT, f"flip_{name}.npz")
            np.savez_compressed(path, sr=sr.detach().numpy(), hr=hr.numpy(), err=err.detach().numpy()[:, 0],
                                loss=np.float32(loss.item()), grad=sr.grad.numpy(),
                                csf_a=s_a[0, 0].numpy(), csf_rg=s_rg[0, 0].numpy(), csf_by=s_by[0, 0].numpy(),
                                edge=edge[0, 0].numpy(), point=point[0, 0].numpy(), cmax=np.float64(cmax_t.item()),
                                csf_radius=np.int32(r_c), ppd=np.float64(ppd))
            print(f"{path}: loss {loss.item():.7f}, NaN gradient entries {int(torch.isnan(sr.grad).sum())} of {sr.grad.numel()}")
    finally:
        torch.Tensor.cuda = real_cuda


if __name__ == "__main__":
    main()
