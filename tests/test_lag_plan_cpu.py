"""
The lag planner and the slot layout of a sweep (csrc/lag_plan.hpp) on the host, under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/native/lag_plan_rules.cpp): on fourteen lag planes -- the headline's 60 x 60, a slice of
it cut in mid-row, 1 x 300, 300 x 1, 1 x 1 among them -- every requested lag occurs exactly once, padding is the tail of a
batch, the live lag-waves do not exceed the single-rectangle plan's (restated there), 60 x 60 takes 57 of them, the
headline's patches fit the compiled pitch 121, `patch_w` brings the single rectangle back batch for batch, a patch of more
than 256 lags loses no lag, and the planes of tests/test_gpu_lag_packing.py have batches of one to four live lag-waves.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-Wall", "-Wextra",
                         os.path.join(HERE, "native", "lag_plan_rules.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: 14 lag planes" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_lag_plan_rules(tmp_path):
    """The plain build: runs wherever there is a host compiler."""
    exe, cc = _build(tmp_path, "lag_plan_rules", [])
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_lag_plan_rules_under_asan_ubsan(tmp_path):
    exe, cc = _build(tmp_path, "lag_plan_rules_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)
