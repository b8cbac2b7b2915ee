"""
The planners of the three header-shift sweeps (csrc/sweep_plan.hpp: Carrington, CAR to CAR, TAN) on the host, plain and
under AddressSanitizer + UndefinedBehaviorSanitizer.  tests/native/sweep_plan_rules.cpp states the rules on its own: slot
coverage over mid-row slices, combination ranges and lag lists in any order; the Carrington origins and cull boxes; the
identity lag-point, the skip bytes and the pole-less lags of the CAR sweep; the homographies, BorderFix items, skip bytes
and sweep mode of the TAN sweep; byte-equal plans on 1 and 8 threads.  The header compiles with a host compiler alone.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    # (geometry.hpp pins wcslib's roundings with `#pragma clang fp`, which g++ does not know and does not need: it never
    # contracts across statements without -ffast-math / -march flags)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-pthread",
                         os.path.join(HERE, "native", "sweep_plan_rules.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok: sweep plan rules" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sweep_plan_rules(tmp_path):
    """The plain build: runs wherever there is a host compiler."""
    exe, cc = _build(tmp_path, "sweep_plan_rules", [])
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sweep_plan_rules_under_asan_ubsan(tmp_path):
    exe, cc = _build(tmp_path, "sweep_plan_rules_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)
