"""FLIP (Andersson, Nilsson, Akenine-Moller, Oskarsson, Astrom, Fairchild: "FLIP: A Difference Evaluator for Alternating
Images", HPG 2020) as a training loss and a validation metric (reference: losses/flip.py, srmodel.py:35,49).  Part of
`ops` (re-exported there).

The error of a pixel, for a reference image R (the HR target) and a test image T (the model's output), both sRGB:
  1. both images -> linear RGB (inputs clamped to [0,1]) -> CIE XYZ (D65) -> YCxCz (opponent space);
  2. each opponent channel is filtered with its contrast sensitivity function (CSF): A and RG one Gaussian each, BY the
     sum of two; the filters have radius 10 at 67.02 pixels per degree, `replicate` borders;
  3. the filtered colours -> linear RGB, clamped to [0,1] -> L*a*b* -> Hunt adjustment (a, b scaled by 0.01 L);
     colour error  C = redistribute(HyAB(R~, T~) ** qc), HyAB = |dL| + ||(da, db)||, redistribute maps [0, pc cmax) linearly
     onto [0, pt) and [pc cmax, cmax] onto [pt, 1];
  4. feature error on the unfiltered luminance y = (Y + 16) / 116: edges (first derivative of a Gaussian) and points
     (second derivative), radius 9, in x and y;  Fe = max(| |edges R| - |edges T| |, | |points R| - |points T| |),
     F = clamp((Fe / sqrt 2) ** qf, 0, 1);
  5. error = C ** (1 - F);  the loss / metric is the mean error over N x H x W.

Every filter is separable (CSF A and RG exactly g x g, BY a sum of two such products, the feature filters (normalised
1-D derivative in x) x (normalised Gaussian in y) and the transpose): the HIP kernels (csrc/flip.hip) and `flip_torch`
filter with 1-D passes.  The 2-D fp32 filters the reference convolves with are built by `flip_tables()` too, for the
tests.

Gradient convention.  Where the gradient is finite it is the gradient of the expression above with torch's choices at the
kinks (abs and norm at 0: 0; elementwise max on a tie: half to each side; clamp: passes on the closed interval; the
branch of every threshold as in the forward).  Where it is not -- a pixel whose colour error C is 0 (the filtered,
clamped colours of the two images coincide: C ** (1 - F) has an infinite slope there and the reference's autograd gives
NaN), or whose feature difference Fe is 0 (sqrt at 0) -- that pixel's error (resp. its feature term) contributes a zero
gradient.  Both are minima of the error, so 0 is a valid subgradient, and the gradient is finite everywhere.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from .ops import _f32c, _need_gpu, _ptr, _stream      # (ops.py imports this module at its END: these exist by then)

__all__ = ["flip_tables", "flip_torch", "flip_error_map_torch", "FlipLossFn", "flip_loss", "flip_error_map", "flip"]

# viewing conditions of the reference (0.7 m from a 0.7 m wide 3840-pixel monitor) and the paper's parameters
PIXELS_PER_DEGREE = 0.7 * (3840 / 0.7) * (math.pi / 180)
QC, QF, PC, PT = 0.7, 0.5, 0.4, 0.95
# CSF of each opponent channel: a1 sqrt(pi/b1) exp(-pi^2 r^2 / b1) + a2 sqrt(pi/b2) exp(-pi^2 r^2 / b2), r in degrees
_CSF = {"A": (1.0, 0.0047, 0.0, 1e-5), "RG": (1.0, 0.0053, 0.0, 1e-5), "BY": (34.1, 0.04, 13.5, 0.025)}
_FEATURE_WIDTH = 0.082          # peak-to-trough width of the human edge detector, degrees (2 standard deviations)

# linear sRGB -> CIE XYZ, D65 (exact rational form of the sRGB primaries)
_RGB2XYZ = np.array([[10135552 / 24577794, 8788810 / 24577794, 4435075 / 24577794],
                     [2613072 / 12288897, 8788810 / 12288897, 887015 / 12288897],
                     [1425312 / 73733382, 8788810 / 73733382, 70074185 / 73733382]], dtype=np.float64)

# the device table (include/srk.h SRK_FLIP_*): fp32, in this order
_TAB_CSF_A, _TAB_CSF_RG, _TAB_CSF_BY1, _TAB_CSF_BY2 = 0, 21, 42, 63
_TAB_EDGE, _TAB_POINT, _TAB_GAUSS = 84, 103, 122
_TAB_BY_W, _TAB_REDIST, _TAB_M, _TAB_MINV, _TAB_WHITE = 141, 143, 147, 156, 165
TABLE_FLOATS = L.SRK_FLIP_TABLE_FLOATS
ADJ_CHANNELS = L.SRK_FLIP_ADJ_CHANNELS      # d err / d(filtered test Y, Cx, Cz), d err / d(test edge x, edge y, point x, point y)


def _csf_radius(ppd):
    bmax = max(b for a1, b1, a2, b2 in _CSF.values() for b in (b1, b2))
    return int(np.ceil(3 * np.sqrt(bmax / (2 * np.pi ** 2)) * ppd))


def _feature_sd(ppd):
    return 0.5 * _FEATURE_WIDTH * ppd


def _split_normalise(v):
    """Positive entries scaled to sum 1, negative entries to sum -1 (float64)."""
    pos, neg = v[v > 0].sum(), -v[v < 0].sum()
    return np.where(v < 0, v / neg, v / pos)


@functools.lru_cache(maxsize=None)
def flip_tables():
    """Host-side FLIP constants, built once in float64 from the definitions and rounded to fp32 where the kernels use them.

    Keys: `ppd`; `csf_radius` (10) and `feature_radius` (9); the 1-D taps `csf_a`, `csf_rg`, `csf_by1`, `csf_by2` and the BY
    weights `by_w` (CSF_BY = by_w[0] by1 x by1 + by_w[1] by2 x by2), `edge` / `point` (1-D derivative taps along the
    detector's direction) and `gauss` (across it); `cmax` (the colour error of green vs blue, fp32, as a Python float);
    `rgb2xyz`, `xyz2rgb`, `white` (float64); `table` (the device table, float32 numpy); and the 2-D fp32 filters the
    reference convolves with: `csf_a_2d`, `csf_rg_2d`, `csf_by_2d`, `edge_2d`, `point_2d` (x-direction forms)."""
    ppd = PIXELS_PER_DEGREE
    r = _csf_radius(ppd)
    dx = 1.0 / ppd
    t = np.arange(-r, r + 1, dtype=np.float64) * dx
    out = {"ppd": ppd, "csf_radius": r}
    # 2-D CSFs (the reference's filters: float64, normalised, then fp32)
    yy, xx = np.meshgrid(t, t, indexing="ij")
    rr = xx ** 2 + yy ** 2
    for name, (a1, b1, a2, b2) in _CSF.items():
        g2 = a1 * np.sqrt(np.pi / b1) * np.exp(-np.pi ** 2 * rr / b1) + a2 * np.sqrt(np.pi / b2) * np.exp(-np.pi ** 2 * rr / b2)
        out[f"csf_{name.lower()}_2d"] = (g2 / np.sum(g2)).astype(np.float32)
    # separable forms: exp(-pi^2 (x^2 + y^2) / b) = e(x) e(y)
    def gauss_1d(b):
        e = np.exp(-np.pi ** 2 * t ** 2 / b)
        return e / e.sum(), e.sum()
    out["csf_a"] = gauss_1d(_CSF["A"][1])[0]
    out["csf_rg"] = gauss_1d(_CSF["RG"][1])[0]
    a1, b1, a2, b2 = _CSF["BY"]
    u1, s1 = gauss_1d(b1)
    u2, s2 = gauss_1d(b2)
    m1, m2 = a1 * np.sqrt(np.pi / b1) * s1 * s1, a2 * np.sqrt(np.pi / b2) * s2 * s2
    out["csf_by1"], out["csf_by2"], out["by_w"] = u1, u2, np.array([m1 / (m1 + m2), m2 / (m1 + m2)])
    # feature detectors
    sd = _feature_sd(ppd)
    fr = int(np.ceil(3 * sd))
    out["feature_radius"] = fr
    k = np.arange(-fr, fr + 1, dtype=np.float64)
    e = np.exp(-k ** 2 / (2 * sd * sd))
    out["gauss"] = e / e.sum()
    out["edge"] = _split_normalise((0.0 - k) * e)           # (0 - k: a +0 centre tap, as the reference has)
    out["point"] = _split_normalise((k ** 2 / (sd * sd) - 1) * e)
    ky, kx = np.meshgrid(k, k, indexing="ij")
    e2 = np.exp(-(kx ** 2 + ky ** 2) / (2 * sd * sd))
    for name, d in (("edge", (0.0 - kx) * e2), ("point", (kx ** 2 / (sd * sd) - 1) * e2)):
        # the reference normalises the fp32-rounded filter by the float64 sums, in fp32
        pos, neg = float(d[d > 0].sum()), float(-d[d < 0].sum())
        d32 = torch.from_numpy(d.astype(np.float32))
        out[f"{name}_2d"] = torch.where(d32 < 0, d32 / neg, d32 / pos).numpy()
    # colour spaces
    out["rgb2xyz"] = _RGB2XYZ
    out["xyz2rgb"] = np.linalg.inv(_RGB2XYZ)
    out["white"] = _RGB2XYZ.sum(axis=1)
    out["cmax"] = _cmax()
    out["table"] = _device_table(out)
    return out


def _cmax():
    """Largest colour error the pipeline can produce (green vs blue, HyAB ** qc), computed in fp32 as the reference does."""
    px = torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32).view(2, 3, 1, 1)
    lab = _hunt(_linrgb_to_lab(px, _mats(torch.float32, "cpu")))
    return float(torch.pow(_hyab(lab[0:1], lab[1:2]), QC))


def _device_table(t):
    tab = np.zeros(TABLE_FLOATS, dtype=np.float32)
    tab[_TAB_CSF_A:_TAB_CSF_A + 21] = t["csf_a"]
    tab[_TAB_CSF_RG:_TAB_CSF_RG + 21] = t["csf_rg"]
    tab[_TAB_CSF_BY1:_TAB_CSF_BY1 + 21] = t["csf_by1"]
    tab[_TAB_CSF_BY2:_TAB_CSF_BY2 + 21] = t["csf_by2"]
    tab[_TAB_EDGE:_TAB_EDGE + 19] = t["edge"]
    tab[_TAB_POINT:_TAB_POINT + 19] = t["point"]
    tab[_TAB_GAUSS:_TAB_GAUSS + 19] = t["gauss"]
    tab[_TAB_BY_W:_TAB_BY_W + 2] = t["by_w"]
    cmax = t["cmax"]
    pcc = PC * cmax
    tab[_TAB_REDIST:_TAB_REDIST + 4] = [pcc, PT / pcc, (1.0 - PT) / (cmax - pcc), PT]
    tab[_TAB_M:_TAB_M + 9] = t["rgb2xyz"].ravel()
    tab[_TAB_MINV:_TAB_MINV + 9] = t["xyz2rgb"].ravel()
    tab[_TAB_WHITE:_TAB_WHITE + 3] = t["white"]
    assert t["csf_radius"] == 10 and t["feature_radius"] == 9       # the kernels' compile-time radii
    return tab


# --------------------------------------------------------------------------------------------
# plain torch (CPU path, float64 ground truth, eager baseline)
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mats_cached(dtype, device):
    t = flip_tables()
    f = lambda a: torch.tensor(np.asarray(a), dtype=dtype, device=device)   # noqa: E731
    return {"m": f(t["rgb2xyz"]), "minv": f(t["xyz2rgb"]), "white": f(t["white"]).view(1, 3, 1, 1)}


def _mats(dtype, device):
    if dtype == torch.float32 and str(device) == "cpu":
        # (flip_tables -> _cmax needs these before flip_tables has returned)
        return {"m": torch.tensor(_RGB2XYZ, dtype=dtype), "minv": torch.tensor(np.linalg.inv(_RGB2XYZ), dtype=dtype),
                "white": torch.tensor(_RGB2XYZ.sum(axis=1), dtype=dtype).view(1, 3, 1, 1)}
    return _mats_cached(dtype, torch.device(device))


@functools.lru_cache(maxsize=None)
def _taps(dtype, device):
    t = flip_tables()
    f = lambda a: torch.tensor(np.asarray(a, dtype=np.float32 if dtype == torch.float32 else np.float64), dtype=dtype, device=device)  # noqa: E731
    return {k: f(t[k]) for k in ("csf_a", "csf_rg", "csf_by1", "csf_by2", "edge", "point", "gauss", "by_w")}


def _mix(m, x):
    """3x3 colour matrix applied per pixel to an N x 3 x H x W image."""
    return torch.einsum("ij,njhw->nihw", m, x)


def _safe_where(cond, fn, x, other):
    """where(cond, fn(x), other) whose gradient is finite where fn's is not on the unselected side."""
    xs = torch.where(cond, x, torch.ones_like(x))
    return torch.where(cond, fn(xs), other)


def _srgb_to_ycxcz(x, mats):
    c = x.clamp(0.0, 1.0)
    lin = torch.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92)
    xyz = _mix(mats["m"], lin) / mats["white"]
    return torch.cat((116 * xyz[:, 1:2] - 16, 500 * (xyz[:, 0:1] - xyz[:, 1:2]), 200 * (xyz[:, 1:2] - xyz[:, 2:3])), 1)


def _ycxcz_to_linrgb(o, mats):
    y = (o[:, 0:1] + 16) / 116
    xyz = torch.cat((y + o[:, 1:2] / 500, y, y - o[:, 2:3] / 200), 1) * mats["white"]
    return _mix(mats["minv"], xyz)


def _linrgb_to_lab(lin, mats):
    t = _mix(mats["m"], lin) / mats["white"]
    d = 6.0 / 29.0
    f = _safe_where(t > 0.00885, lambda v: v ** (1.0 / 3.0), t, t / (3 * d * d) + 4.0 / 29.0)
    return torch.cat((116 * f[:, 1:2] - 16, 500 * (f[:, 0:1] - f[:, 1:2]), 200 * (f[:, 1:2] - f[:, 2:3])), 1)


def _hunt(lab):
    l = lab[:, 0:1]
    return torch.cat((l, 0.01 * l * lab[:, 1:2], 0.01 * l * lab[:, 2:3]), 1)


def _hyab(p, q):
    d = p - q
    return d[:, 0:1].abs() + torch.linalg.vector_norm(d[:, 1:3], dim=1, keepdim=True)


def _sep(x, th, tv):
    """Separable filter, replicate borders: th along x (width), then tv along y."""
    r = (th.numel() - 1) // 2
    c = x.shape[1]
    x = F.pad(x, (r, r, r, r), mode="replicate")
    x = F.conv2d(x, th.view(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)
    return F.conv2d(x, tv.view(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)


def flip_error_map_torch(sr, hr):
    """Per-pixel FLIP error (N x 1 x H x W) of test image `sr` against reference image `hr`, in plain torch (fp32 or
    float64, any device); autograd gives the gradient with the convention of the module docstring."""
    if sr.shape[1] != 3:
        raise ValueError(f"FLIP needs 3-channel (RGB) images, got {sr.shape[1]} channels")
    dt, dev = sr.dtype, sr.device
    mats, tp = _mats(dt, dev), _taps(dt, dev)
    cmax = flip_tables()["cmax"]
    pcc = PC * cmax
    n = sr.shape[0]
    o = _srgb_to_ycxcz(torch.cat((hr.to(dt), sr), 0), mats)                 # reference images first, then the test images
    filt = torch.cat((_sep(o[:, 0:1], tp["csf_a"], tp["csf_a"]), _sep(o[:, 1:2], tp["csf_rg"], tp["csf_rg"]),
                      tp["by_w"][0] * _sep(o[:, 2:3], tp["csf_by1"], tp["csf_by1"])
                      + tp["by_w"][1] * _sep(o[:, 2:3], tp["csf_by2"], tp["csf_by2"])), 1)
    lab = _hunt(_linrgb_to_lab(_ycxcz_to_linrgb(filt, mats).clamp(0.0, 1.0), mats))
    h = _hyab(lab[:n], lab[n:])
    p = _safe_where(h > 0, lambda v: v ** QC, h, torch.zeros_like(h))
    cerr = torch.where(p < pcc, (PT / pcc) * p, PT + ((p - pcc) / (cmax - pcc)) * (1.0 - PT))
    y = (o[:, 0:1] + 16) / 116
    ex, ey = _sep(y, tp["edge"], tp["gauss"]), _sep(y, tp["gauss"], tp["edge"])
    px, py = _sep(y, tp["point"], tp["gauss"]), _sep(y, tp["gauss"], tp["point"])
    en = torch.linalg.vector_norm(torch.cat((ex, ey), 1), dim=1, keepdim=True)
    pn = torch.linalg.vector_norm(torch.cat((px, py), 1), dim=1, keepdim=True)
    fe = torch.max((en[:n] - en[n:]).abs(), (pn[n:] - pn[:n]).abs())
    fe = _safe_where(fe > 0, lambda v: (v / math.sqrt(2.0)) ** QF, fe, torch.zeros_like(fe)).clamp(0.0, 1.0)
    return _safe_where(cerr > 0, lambda v: v ** (1.0 - fe), cerr, torch.zeros_like(cerr))


def flip_torch(sr, hr):
    """FLIP loss / metric in plain torch: mean of `flip_error_map_torch` over N x H x W."""
    return flip_error_map_torch(sr, hr).mean()


# --------------------------------------------------------------------------------------------
# HIP path (csrc/flip.hip)
# --------------------------------------------------------------------------------------------
_dev_tables = {}


def _device_table_for(device):
    """The fp32 constant table on `device`, uploaded once and cached (a replayed graph reads the same allocation)."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    tab = _dev_tables.get(key)
    if tab is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the FLIP constant table is built on the first eager call; call flip once before capturing a graph")
        tab = _dev_tables[key] = torch.from_numpy(flip_tables()["table"]).to(torch.device("cuda", key[1]))
    return tab


def _args(s, h, tab, *, partial=None, err=None, adj=None, gout=None, scale=0.0, grad=None):
    n, _, hh, ww = s.shape
    return L.FlipArgs(sr=s.data_ptr(), hr=_ptr(h), N=n, H=hh, W=ww, table=tab.data_ptr(), partial=_ptr(partial), err=_ptr(err),
                      adj=_ptr(adj), gout=_ptr(gout), scale=float(scale), grad=_ptr(grad))


def _forward(sr, hr, want_map, want_adj):
    _need_gpu(sr)
    s, h = _f32c(sr), _f32c(hr)
    n, c, hh, ww = s.shape
    if c != 3 or h.shape != s.shape:
        raise ValueError(f"FLIP needs two N x 3 x H x W images of one shape, got {tuple(sr.shape)} and {tuple(hr.shape)}")
    tab = _device_table_for(s.device)
    nb = L.load().srk_flip_blocks(n, hh, ww)
    partial = torch.empty(nb, dtype=torch.float64, device=s.device)
    err = torch.empty(n, 1, hh, ww, dtype=torch.float32, device=s.device) if want_map else None
    adj = torch.empty(n, ADJ_CHANNELS, hh, ww, dtype=torch.float32, device=s.device) if want_adj else None
    L.call("srk_flip_fwd", _args(s, h, tab, partial=partial, err=err, adj=adj), _stream())
    out = torch.empty((), dtype=torch.float32, device=s.device)
    L.check(L.load().srk_flip_mean(partial.data_ptr(), nb, n * hh * ww, out.data_ptr(), _stream()), "srk_flip_mean")
    return out, err, adj, s, tab


class FlipLossFn(torch.autograd.Function):
    """mean FLIP error as two launches forward (srk_flip_fwd: both images, every filter and the per-pixel error in one pass,
    plus the fixed-order mean) and one backward (srk_flip_bwd: the transposed filters and the colour-space Jacobians).  The
    forward leaves the 7 per-pixel adjoints of the error for a unit upstream gradient; the backward scales by the upstream
    gradient read on the device (no host sync: capturable)."""

    @staticmethod
    def forward(ctx, sr, hr):
        out, _, adj, s, tab = _forward(sr, hr, False, ctx.needs_input_grad[0])
        ctx.save_for_backward(s, adj, tab)
        return out

    @staticmethod
    def backward(ctx, g):
        s, adj, tab = ctx.saved_tensors
        gout = g.detach().float().contiguous()
        grad = torch.empty_like(s)
        n, _, hh, ww = s.shape
        L.call("srk_flip_bwd", _args(s, None, tab, adj=adj, gout=gout, scale=1.0 / (n * hh * ww), grad=grad), _stream())
        return grad, None


def _hip_ok(sr, hr):
    return (sr.is_cuda and sr.dtype == torch.float32 and hr.dtype == torch.float32 and sr.dim() == 4 and sr.shape[1] == 3
            and sr.shape == hr.shape and sr.numel() > 0)


def flip_loss(sr, hr):
    """Mean FLIP error of `sr` (test) against `hr` (reference): HIP for CUDA fp32 RGB tensors when `hr` needs no gradient,
    `flip_torch` otherwise."""
    if hr.requires_grad or not _hip_ok(sr, hr):
        return flip_torch(sr, hr)
    return FlipLossFn.apply(sr, hr)


def flip_error_map(sr, hr):
    """Per-pixel FLIP error (N x 1 x H x W), no gradient."""
    with torch.no_grad():
        if not _hip_ok(sr, hr):
            return flip_error_map_torch(sr, hr)
        return _forward(sr, hr, True, False)[1]


def flip(sr, hr):
    """FLIP metric: mean error over N x H x W as a 0-d tensor, no gradient (no host sync on the GPU)."""
    with torch.no_grad():
        if not _hip_ok(sr, hr):
            return flip_torch(sr, hr)
        return _forward(sr, hr, False, False)[0]
