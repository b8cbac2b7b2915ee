"""
The planner of the pixel-lag sweep (csrc/pixels_plan.hpp) on the host, under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/native/pixels_plan_rules.cpp): the dx groups of nine lag lists, the window count against
a brute-force count for every axis up to 40 pixels, the band of thirty image and tile shapes against the four bounds
that keep it within the kernels' LDS, the section offsets of the plan blob and what its writer leaves in it (plain,
mutual information, apodized), and every refusal -- code, message and order -- with the requests either side of each
limit.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-Wall", "-Wextra",
                         os.path.join(HERE, "native", "pixels_plan_rules.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: pixels plan rules" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pixels_plan_rules(tmp_path):
    """The plain build: runs wherever there is a host compiler."""
    exe, cc = _build(tmp_path, "pixels_plan_rules", [])
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_pixels_plan_rules_under_asan_ubsan(tmp_path):
    exe, cc = _build(tmp_path, "pixels_plan_rules_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)
