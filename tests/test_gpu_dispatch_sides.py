"""The other side of every dispatch decision of srk_conv2d / srk_conv2d_wgrad / srk_unfold_nchw: the kernel the launcher falls back to
when a `*_ok()` predicate refuses a shape or an A/B knob is set (SRK_DEBUG=1, tools/ab_knob.sh), against float64 of the same
16-bit-rounded operands.  The knobs are read once per process: each setting is one child `python tests/dispatch_cases.py <setting>`,
which runs all cases of that setting, compares them itself and prints one "RESULT {json}" line (tests/dispatch_cases.py holds the case
bodies, the criteria -- those of the existing test of the same operation -- and the two derived bounds).

Every case is checked in this order:
1. premise: srk_last_kernel() named the fallback, and the same call with no knob (the child "none") named another kernel -- a misspelt
   or retired knob cannot pass by running the preferred side twice; under SRK_NO_WS the weight gradient also ran with the generic
   kernel's own slab count (one slab per workgroup of its grid, worked out in dispatch_cases.generic_slabs) where the no-knob run used
   the slab kernels' count, and its two runs are equal bit for bit;
2. coverage: no NaN of the prefilled outputs survived;
3. numbers: the worst error is within its bound.

Children run one at a time, each under a time limit of its own.  A child that ends by a signal, a time limit or a HIP error poisons
the module: every later test fails at once with that reason and starts no process.  Nothing is retried.

With SRK_PROFILE_DIR set, the result lines are saved there as one JSON document, dispatch_sides.json: tools/collect_profiles.sh
regenerates profiles/dispatch_sides.json this way."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dispatch_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = D.ROOT
_POISON = []          # the reason the module stopped starting processes
_DONE = {}            # setting -> parsed RESULT
_FAILED = {}          # setting -> why its child gave no result (a child runs once: nothing is retried)
_HIP_TROUBLE = ("HIP error", "hipError", "illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "GPU Hang")


def _child(setting):
    if setting in _DONE:
        return _DONE[setting]
    if _POISON:
        pytest.fail(f"not started: {_POISON[0]}")
    if setting in _FAILED:
        pytest.fail(_FAILED[setting])
    limit = D.NONE_TIMEOUT if setting == "none" else D.SETTINGS[setting][2]
    cmd = [sys.executable, os.path.join(ROOT, "tests", "dispatch_cases.py"), setting]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, env=D.child_env(setting), timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _POISON.append(f"the child of setting {setting!r} ran into its time limit of {limit} s")
        pytest.fail(_POISON[0])
    if p.returncode < 0 or any(t in p.stderr for t in _HIP_TROUBLE):
        _POISON.append(f"the child of setting {setting!r} ended with status {p.returncode}: {p.stderr[-1500:]}")
        pytest.fail(_POISON[0])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        _FAILED[setting] = f"the child of setting {setting!r} ended with status {p.returncode}: {p.stderr[-3000:]}"
        pytest.fail(_FAILED[setting])
    line = lines[-1]
    _DONE[setting] = json.loads(line[7:])
    _save()
    return _DONE[setting]


def _save():
    out = os.environ.get("SRK_PROFILE_DIR")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "dispatch_sides.json"), "w") as f:
            json.dump({k: _DONE[k] for k in sorted(_DONE)}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass          # a read-only directory: the assertions below do not depend on the file


@pytest.mark.parametrize("setting", list(D.SETTINGS))
def test_fallback_side_against_float64(setting):
    base = _child("none")["cases"]
    got = _child(setting)
    assert got["setting"] == setting and got["cases"], "the child ran no case"
    moved, bad = 0, []          # every case is judged; the message lists all that failed
    for cid, c in got["cases"].items():
        # 1. premise
        if not c["expect"]:
            bad.append((cid, "no expectation for this setting"))
        for role, want in c["expect"].items():
            if c["kernels"][role] != want:
                bad.append((cid, role, "ran", c["kernels"][role], "expected", want))
            elif c.get("same_side_because"):
                if base[cid]["kernels"][role] != want:
                    bad.append((cid, role, "expected on the same side", base[cid]["kernels"][role]))
            elif base[cid]["kernels"][role] == want:
                bad.append((cid, role, "the no-knob run took the same kernel", want))
            else:
                moved += 1
        if "nslabs" in c and not (c["nslabs"] == c["nslabs_generic"] and all(s > 0 for s in c["nslabs"] + base[cid]["nslabs"])):
            bad.append((cid, "srk_wgrad_slabs()", c["nslabs"], "generic grid", c["nslabs_generic"], "no knob", base[cid]["nslabs"]))
        if "nslabs" in c and not c["bitwise_repeat"]:
            bad.append((cid, "two runs of the generic weight gradient differ", c["run_to_run"]))
        # 2. coverage
        if c["nan"]:
            bad.append((cid, "a NaN of the prefilled output survived (or the kernel made one)"))
        # 3. numbers
        if c["ratio"] is None or not c["ratio"] <= 1.0:
            bad.append((cid, "error / bound", c["ratio"], {k: v for k, v in c.items() if k not in ("kernels", "expect", "nan", "ratio")}))
    assert not bad, (setting, len(bad), "of", len(got["cases"]), bad[:40])
    assert moved > 0
