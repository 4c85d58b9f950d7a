"""CPU tests of the product's host side: the C-ABI library loads and exports what include/srk.h declares,
the ctypes binding derived from the header has the C compiler's struct layouts, the prototypes and the constants,
the model classes keep the reference's constructor / state_dict / init contract, the HIP path refuses to run
without a GPU, and config 0 (SRCNN x2 on CPU) works."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import sr_amd
from oracle import fill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
HEADER = open(os.path.join(ROOT, "include", "srk.h")).read()


def _declared_functions():
    return sorted(set(re.findall(r"^(?:int|long long|const char\*)\s+(srk_\w+)\s*\(", HEADER, flags=re.M)))


def test_library_exports_every_declared_symbol():
    lib = sr_amd._lib.load()
    names = _declared_functions()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/srk.h but not exported"
    assert set(names) == set(sr_amd._lib.LAUNCHERS) | set(sr_amd._lib.OTHER_SYMBOLS)
    assert lib.srk_version() >= 100
    assert [lib.srk_conv_tile(c) for c in (3, 48, 64, 102, 128, 192, 256, 768)] == [32, 64, 64, 128, 128, 64, 128, 128]


# ---- the binding derived from include/srk.h (sr_amd._lib) -----------------------------------------------------------------------------
L = sr_amd._lib
HEADER_CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)          # comments out first: some contain braces and calls


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """What the C compiler lays out for every struct of the header: {C name: (sizeof, [offsetof of each field], [sizeof of each field])},
    printed by one generated program that includes srk.h."""
    cc = os.environ.get("CC") or shutil.which("cc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    if not (shutil.which(cc) or os.path.exists(cc)):
        pytest.fail(f"no C compiler to check the struct layouts with ($CC, cc, {cc})")
    d = tmp_path_factory.mktemp("layout")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "srk.h"', "int main(void) {"]
    for cname, cls in L.STRUCTS.items():
        names = [n for n, _ in cls._fields_]
        lines.append('  printf("%s offsets %%zu%s\\n", sizeof(%s)%s);' % (
            cname, " %zu" * len(names), cname, "".join(", offsetof(%s, %s)" % (cname, n) for n in names)))
        lines.append('  printf("%s sizes%s\\n"%s);' % (
            cname, " %zu" * len(names), "".join(", sizeof(((%s*)0)->%s)" % (cname, n) for n in names)))
    (d / "layout.c").write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(d / "layout"), str(d / "layout.c")], check=True)
    out = {}
    for line in subprocess.run([str(d / "layout")], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, what, *nums = line.split()
        out.setdefault(cname, {})[what] = [int(v) for v in nums]
    return {c: (v["offsets"][0], v["offsets"][1:], v["sizes"]) for c, v in out.items()}


@pytest.mark.parametrize("cname,cls", [(c, k.__name__) for c, k in L.STRUCTS.items()])
def test_ctypes_structs_mirror_header(c_layout, cname, cls):
    """Every struct of the binding against the C compiler's layout of include/srk.h: size, each field's offset, and each field's size
    (a float taken for an int sits at the same offset)."""
    st = getattr(L, cls)
    assert st is L.STRUCTS[cname]
    size, offsets, sizes = c_layout[cname]
    assert ctypes.sizeof(st) == size
    assert [getattr(st, n).offset for n, _ in st._fields_] == offsets
    assert [getattr(st, n).size for n, _ in st._fields_] == sizes


def test_every_struct_of_the_header_is_bound(c_layout):
    assert len(L.STRUCTS) == len(re.findall(r"\btypedef struct\b", HEADER_CODE)) == len(c_layout) > 0
    assert all(getattr(L, cls.__name__) is cls for cls in L.STRUCTS.values())


# feature -> (argument struct, launchers that take it, helpers that must be bound as plain functions)
ABI = {
    "gmsd": ("GmsdArgs", ["srk_gmsd_fwd", "srk_gmsd_finalize", "srk_gmsd_bwd"], ["srk_gmsd_tiles"]),
    "ssim_loss": ("SsimLossArgs", ["srk_ssim_loss_fwd", "srk_ssim_loss_finalize", "srk_ssim_loss_bwd"], ["srk_ssim_loss_tiles"]),
    "ms_ssim_loss": ("MsSsimLossArgs", ["srk_ms_ssim_loss_fwd", "srk_ms_ssim_loss_finalize", "srk_ms_ssim_loss_bwd"],
                     ["srk_ms_ssim_loss_workspace_bytes", "srk_ms_ssim_loss_tiles"]),
    "ms_ssim": ("MsSsimArgs", ["srk_ms_ssim"], ["srk_ms_ssim_workspace_bytes", "srk_ms_ssim_tiles"]),
    "haarpsi": ("HaarpsiArgs", ["srk_haarpsi_fwd", "srk_haarpsi_finalize", "srk_haarpsi_bwd"], ["srk_haarpsi_tiles"]),
    "flip": ("FlipArgs", ["srk_flip_fwd", "srk_flip_bwd"], ["srk_flip_blocks", "srk_flip_mean"]),
    "l1": ("L1Args", ["srk_l1_loss_fwd", "srk_l1_loss_bwd"], ["srk_l1_blocks", "srk_l1_loss_mean"]),
    "adam": ("AdamArgs", ["srk_adam_step"], ["srk_adam_step_scaled", "srk_adam_check_scaled", "srk_adam_update_scaled"]),
    "ranger": ("RangerArgs", ["srk_ranger_step"], ["srk_ranger_step_scaled", "srk_ranger_check_scaled", "srk_ranger_update_scaled"]),
    "sgd": ("SgdArgs", ["srk_sgd_step"], ["srk_sgd_step_scaled", "srk_sgd_check_scaled", "srk_sgd_update_scaled"]),
    "rmsprop": ("RmspropArgs", ["srk_rmsprop_step"], ["srk_rmsprop_step_scaled", "srk_rmsprop_check_scaled", "srk_rmsprop_update_scaled"]),
    "ema": ("EmaArgs", ["srk_ema_step"], []),
    "tile": ("TileArgs", ["srk_tile_gather", "srk_tile_place"], []),
    "hrtail": ("HrtailArgs", ["srk_hrtail_collapse", "srk_hrtail_edge_fwd", "srk_hrtail_edge_bwd_x", "srk_hrtail_edge_bwd_w",
                              "srk_hrtail_expand"], ["srk_hrtail_scratch_floats"]),
}


@pytest.mark.parametrize("feature", sorted(ABI))
def test_feature_entry_points_are_bound(feature):
    cls, launchers, helpers = ABI[feature]
    for name in launchers:
        assert L.LAUNCHERS[name] is getattr(L, cls), name
        assert L.PROTOTYPES[name] == (ctypes.c_int, [ctypes.POINTER(getattr(L, cls)), ctypes.c_void_p]), name
    for name in helpers:
        assert name in L.OTHER_SYMBOLS and name not in L.LAUNCHERS, name


def test_every_declared_function_has_a_prototype():
    names = set(L.LAUNCHERS) | set(L.OTHER_SYMBOLS)
    assert len(names) == len(L.LAUNCHERS) + len(L.OTHER_SYMBOLS) == len(re.findall(r"\bsrk_\w+\s*\(", HEADER_CODE)) > 0
    assert names == set(L.PROTOTYPES) == set(_declared_functions())


def test_irregular_prototypes():
    """Pinned by hand: the prototypes that are not `int f(const srk_x_args* a, srk_stream_t stream)`."""
    P, i, p, q = ctypes.POINTER, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong
    want = {
        "srk_wgrad_group_plan": (i, [P(L.WgradArgs), i, p, p, p, p, p]),
        "srk_pw_pack_bytes": (q, [i, i, i, i]),
        "srk_proj_pack_bytes": (q, []),
        "srk_last_error": (ctypes.c_char_p, []),
        "srk_pack_group_tiles": (i, [p, i, p]),                      # `host_table`: an address, not a struct instance
        "srk_pack_conv_weights_group": (i, [p, i, p]),               # `table`
        "srk_weight_norm_group": (i, [p, i, i, i, p]),               # `table_dev`
        "srk_chan_stats_finalize": (i, [P(L.ChanStatsArgs), P(L.ChanFinalizeArgs), p, p]),
        "srk_conv_trunk": (i, [P(L.ConvArgs), p, i, p]),
        "srk_conv_bits_ok": (i, [P(L.ConvArgs)]),
        "srk_l1_blocks": (i, [q]),
        "srk_upload_small": (i, [p, p, q, p]),
    }
    for name, proto in want.items():
        assert L.PROTOTYPES[name] == proto, name
        assert name in L.OTHER_SYMBOLS


def _stub_library(without=()):
    return types.SimpleNamespace(**{n: types.SimpleNamespace() for n in L.PROTOTYPES if n not in without})


def test_bind_sets_every_prototype_on_any_object():
    lib = L.bind(_stub_library(), False)
    for name, (restype, argtypes) in L.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_bind_of_a_library_that_lacks_a_symbol():
    with pytest.raises(RuntimeError, match="srk_gmsd_tiles"):
        L.bind(_stub_library(without=["srk_gmsd_tiles"]), False)
    lib = L.bind(_stub_library(without=["srk_gmsd_tiles"]), True)            # an older build, loaded through SRK_LIB_PATH
    assert lib.srk_gmsd_fwd.restype is ctypes.c_int
    with pytest.raises(RuntimeError, match="srk_gmsd_tiles is not exported by .*SRK_LIB_PATH"):
        lib.srk_gmsd_tiles(1, 3, 8, 8)


def test_parser_on_a_small_header():
    h = L.parse_header("""
        /* a comment with { braces } and srk_call( */
        #define SRK_N 12
        enum { SRK_A = 0, SRK_B = -3 };
        typedef void* srk_stream_t;
        typedef struct srk_two_part_args { const float *a, *b; int n, m; long long P; double lr; unsigned int* t; } srk_two_part_args;
        int srk_go(const srk_two_part_args* a, srk_stream_t stream);
        int srk_go_group(const srk_two_part_args* table_dev, int n, srk_stream_t stream);
        long long srk_bytes(void);
        const char* srk_name(const srk_two_part_args* a,
                             float* out);
    """)
    p, cls = ctypes.c_void_p, h.structs["srk_two_part_args"]
    assert cls.__name__ == "TwoPartArgs" and issubclass(cls, ctypes.Structure)
    assert cls._fields_ == [("a", p), ("b", p), ("n", ctypes.c_int), ("m", ctypes.c_int), ("P", ctypes.c_longlong),
                            ("lr", ctypes.c_double), ("t", p)]
    assert h.consts == {"SRK_N": 12, "SRK_A": 0, "SRK_B": -3}
    assert h.launchers == {"srk_go": cls}
    assert h.protos == {"srk_go": (ctypes.c_int, [ctypes.POINTER(cls), p]), "srk_go_group": (ctypes.c_int, [p, ctypes.c_int, p]),
                        "srk_bytes": (ctypes.c_longlong, []), "srk_name": (ctypes.c_char_p, [ctypes.POINTER(cls), p])}


@pytest.mark.parametrize("text,quoted", [
    ("typedef struct { const float* x; short n; } srk_bad_args;", "short n"),                        # an unknown field type
    ("typedef struct { int a; struct { int b; } inner; } srk_bad_args;", "struct { int b"),          # a nested struct
    ("typedef struct { int a; float w[5]; } srk_bad_args;", "float w[5]"),                           # an array field
    ("typedef struct { int a; float** w; } srk_bad_args;", "float** w"),
    ("typedef struct { int a; } srk_ok_args; typedef struct { srk_ok_args inner; } srk_bad_args;", "srk_ok_args inner"),
    ("typedef struct { int a } srk_bad_args;", "int a"),
    ("void srk_f(int n);", "void srk_f(int n)"),                                                     # an unknown return type
    ("int srk_f(const srk_later_args* a, srk_stream_t stream);", "srk_later_args* a"),               # a struct not declared yet
    ("int srk_f(unsigned n);", "unsigned n"),
    ("enum { SRK_A = 0, SRK_B };", "SRK_B"),
    ("#define SRK_F(x) (x)", "#define SRK_F(x) (x)"),
    ("#pragma pack(1)", "#pragma pack(1)"),
    ("int srk_f(int n)", "int srk_f(int n)"),                                                        # no `;`
])
def test_parser_refuses_and_quotes_what_it_does_not_understand(text, quoted):
    with pytest.raises(ValueError, match=re.escape(quoted)):
        L.parse_header(text)


def test_constants_come_from_the_header():
    assert (L.SRK_BF16, L.SRK_F16, L.SRK_F32) == (0, 1, 2)
    assert (L.OUT_NHWC, L.OUT_NHWC_PS, L.OUT_PLANAR) == (L.SRK_OUT_NHWC, L.SRK_OUT_NHWC_PS, L.SRK_OUT_PLANAR) == (0, 1, 2)
    assert (L.EMA_UPDATE, L.EMA_SWAP, L.EMA_STORE, L.EMA_LOAD) == (L.SRK_EMA_UPDATE, L.SRK_EMA_SWAP, L.SRK_EMA_STORE, L.SRK_EMA_LOAD) == (0, 1, 2, 3)
    assert (L.SRK_E_BADARG, L.SRK_E_NODEV) == (-1, -2)
    assert sr_amd.flip.TABLE_FLOATS == L.SRK_FLIP_TABLE_FLOATS == 176
    assert sr_amd.flip.ADJ_CHANNELS == L.SRK_FLIP_ADJ_CHANNELS == 7


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_state_dict_layout_and_init_match_reference(name):
    ent = MANIFEST[name]
    torch.manual_seed(0)
    m = getattr(sr_amd, ent["class"])(**ent["kwargs"])
    sd = m.state_dict()
    assert list(sd.keys()) == [k for k, _ in ent["state_dict"]]
    for k, shp in ent["state_dict"]:
        assert list(sd[k].shape) == shp
    assert sorted(n for n, p in m.named_parameters() if p.requires_grad) == sorted(ent["trainable"])
    for k, ref in ent["init_seed0"].items():
        t = sd[k].double()
        got = [float(t.sum()), float(t.abs().sum())] + [float(v) for v in sd[k].flatten()[:3]]
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-7, err_msg=k)
    if ent["class"] != "SRResNet":              # BatchNorm running statistics are the only buffers in the zoo
        assert not list(m.named_buffers())      # like the reference


def test_ctor_defaults_and_registry():
    assert sr_amd.models.__all__ == ['DDBPN', 'EDSR', 'RCAN', 'RDN', 'SRCNN', 'SRModel', 'SRResNet', 'WDSR']
    m = sr_amd.EDSR()
    assert (m._batch_size, m._channels, m._scale_factor) == (16, 3, 4)
    assert tuple(m.example_input_array.shape) == (16, 3, 32, 32)     # patch_size 128 // scale 4
    assert m.compute_dtype == torch.float32
    assert sr_amd.EDSR(precision="bf16").compute_dtype == torch.bfloat16
    assert sr_amd.EDSR(precision=16).compute_dtype == torch.float16
    with pytest.raises(ValueError):
        sr_amd.RDN(scale_factor=8)
    with pytest.raises(AttributeError):
        sr_amd.EDSR(losses="l1 + nope")
    with pytest.raises(NotImplementedError):
        sr_amd.EDSR(losses="lpips")
    with pytest.raises(ValueError):
        sr_amd.EDSR(optimizer="LION")
    with pytest.raises(ValueError):
        sr_amd.EDSR(losses="x*l1")


def test_hip_models_refuse_cpu():
    for cls, kw in (("EDSR", dict(n_feats=16, n_resblocks=1)), ("RCAN", dict(n_feats=16, n_resblocks=1, n_resgroups=1, reduction=4)),
                    ("WDSR", dict(n_feats=16, n_resblocks=1)), ("RDN", dict(rdn_config="A", G0=16))):
        m = getattr(sr_amd, cls)(**kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.rand(1, 3, 8, 8))


def test_product_does_not_import_oracle():
    import sys
    pkg = os.path.join(ROOT, "sr-pytorch-lightning_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f"{f} imports the oracle"


def test_reference_state_dict_loads_strict():
    m = sr_amd.RCAN(n_feats=16, n_resblocks=2, n_resgroups=2, reduction=4)
    from oracle import init as OI
    sd, _ = OI.build_state_dict("RCAN", n_feats=16, n_resblocks=2, n_resgroups=2, reduction=4)
    m.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("name", ["srcnn_x2", "srcnn_x4"])
def test_srcnn_cpu_plumbing_matches_reference(name):
    """BASELINE config 0: SRCNN on CPU, against the reference's golden output and gradients."""
    ent = MANIFEST[name]
    g = np.load(os.path.join(GOLDEN, f"model_{name}.npz"))
    m = sr_amd.SRCNN(**ent["kwargs"])
    fill.formula_fill_module(m)
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    y = m(x)
    np.testing.assert_allclose(y.detach().numpy(), g["y"], atol=2e-6)
    (y * fill.formula_tensor(tuple(y.shape), 77, 1.0)).sum().backward()
    np.testing.assert_allclose(x.grad.numpy(), g["dx"], atol=2e-5)
    res = m.training_step({"lr": torch.rand(4, 3, 32, 32), "hr": torch.rand(4, 3, 32 * ent["kwargs"]["scale_factor"], 32 * ent["kwargs"]["scale_factor"])}, 0)
    assert set(res) == {"loss", "loss/l1"}
    opt = m.configure_optimizers()[0]
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["lr"] == 1e-3


def test_adam_on_cpu_parameters_is_torch_adam():
    """sr_amd.optim.Adam subclasses torch.optim.Adam: CPU-resident models (SRCNN, the reference's CPU-runnable case) step
    through torch's implementation; the HIP launch is for GPU parameters only."""
    import sr_amd
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.rand(5, 3, generator=g)), torch.nn.Parameter(torch.rand(7, generator=g))]
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt, ropt = sr_amd.optim.Adam(ps, lr=1e-2), torch.optim.Adam(rs, lr=1e-2)
    for _ in range(3):
        for p, r in zip(ps, rs):
            p.grad = torch.rand(p.shape, generator=g)
            r.grad = p.grad.clone()
        opt.step()
        ropt.step()
    for p, r in zip(ps, rs):
        assert torch.equal(p, r)
    with pytest.raises(NotImplementedError):
        sr_amd.optim.Adam(ps, amsgrad=True)


def test_device_table_keeps_its_address_grows_and_rewrites_only_changed_bytes():
    """packing.DeviceTable, the persistent table behind every grouped pack launch (a captured step names its address)."""
    from sr_amd.packing import DeviceTable
    cpu = torch.device("cpu")
    t = DeviceTable()
    host = (ctypes.c_int * 8)(*range(8))
    buf = t.put(host, cpu)
    addr, cap = buf.data_ptr(), buf.numel()
    assert bytes(buf[:32].numpy()) == bytes(host) and cap >= 4096
    buf[:4].fill_(0xAB)                                   # unchanged bytes are not written again
    assert t.put(host, cpu).data_ptr() == addr and int(buf[0]) == 0xAB
    host[1] = 99                                          # changed bytes are, in place
    buf = t.put(host, cpu)
    assert buf.data_ptr() == addr and bytes(buf[:32].numpy()) == bytes(host)
    big = (ctypes.c_int * (cap // 4 + 1))(*range(cap // 4 + 1))      # content that does not fit: a larger buffer, with head room
    buf = t.put(big, cpu)
    assert buf.numel() >= 2 * ctypes.sizeof(big) and bytes(buf[:ctypes.sizeof(big)].numpy()) == bytes(big)
    addr = buf.data_ptr()
    assert t.put(host, cpu).data_ptr() == addr and bytes(buf[:32].numpy()) == bytes(host)
