"""Every A/B knob the HIP sources read (srk_dbg_getenv("SRK_...") in csrc/*.hip) selects a kernel somebody has to have run against
float64: it is either a setting of tests/dispatch_cases.py (test_gpu_dispatch_sides.py runs the side it selects, and asserts that it
ran) or on the list below with the reason it needs no such run.  A knob added later cannot arrive untested, and a setting whose knob
the sources no longer read is caught here as well as by that test's premise."""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dispatch_cases as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXCEPTIONS = {
    "SRK_STATS_PPB": "a tuning value (pixels per block of the channel statistics), not a choice between kernels",
    "SRK_PROJ_WGS_PER_CU": "a tuning value (workgroups per CU of the projection kernels)",
    "SRK_PROJ_WG_SLICES": "a tuning value (slices per workgroup of the projection weight gradient)",
    "SRK_WGRAD_TH": "a tuning value; both tile heights: test_gpu_wgrad_group.py::test_both_tile_geometries_of_the_slab_weight_gradient_against_float64",
    "SRK_NO_WGRAD1X1_SMALL": "test_gpu_head_conv.py::test_small_1x1_weight_gradient_kernel_matches_the_general_one_bit_for_bit",
    "SRK_NO_TRUNK": "the same switch as ops._TRUNK_OFF, which test_gpu_trunk.py and test_gpu_trainer_graph.py set in-process for both sides",
}


def _knobs_read_by_the_sources():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "sr-pytorch-lightning_amd", "csrc", "*.hip"))):
        for name in re.findall(r'srk_dbg_getenv\("(SRK_\w+)"\)', open(path).read()):
            found.setdefault(name, os.path.basename(path))
    return found


def test_every_knob_of_the_hip_sources_is_covered_or_excepted():
    found = _knobs_read_by_the_sources()
    assert len(found) >= 18, found
    covered = set(D.KNOBS)
    assert not covered & set(EXCEPTIONS), "a knob is either covered or excepted"
    missing = {k: f for k, f in found.items() if k not in covered and k not in EXCEPTIONS}
    assert not missing, f"knobs without a case in tests/dispatch_cases.py and without a reason here: {missing}"
    retired = sorted((covered | set(EXCEPTIONS)) - set(found))
    assert not retired, f"the sources no longer read {retired}: drop the setting / the exception"
    assert all(len(reason) > 10 for reason in EXCEPTIONS.values())


def test_every_setting_sets_one_knob_and_has_cases():
    for name, (env, groups, limit) in D.SETTINGS.items():
        assert list(env) == [name] and env[name] == "1" and groups and 0 < limit <= 300, name
        env_child = D.child_env(name)
        assert env_child["SRK_DEBUG"] == "1" and env_child[name] == "1"
    assert "SRK_DEBUG" not in D.child_env("none")
