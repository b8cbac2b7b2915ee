"""
The plan of the median/MAD despiking (csrc/despike_plan.hpp) on the host, plain and under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/native/despike_rules.cpp, a program with its own main, run directly): every parameter
refusal either side of each limit, the launch geometry -- every pixel owned exactly once, nothing outside the image or the
LDS a work item has -- for the shapes 1x1, 1x300, 300x1, 5x5 and one pixel past and one short of a tile in each axis with
R = 1, 2, 3, and the decision function the kernel calls against a brute-force sort for every k from 0 to 48.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-Wall", "-Wextra",
                         os.path.join(HERE, "native", "despike_rules.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: despike rules" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_despike_rules(tmp_path):
    """The plain build: runs wherever there is a host compiler."""
    exe, cc = _build(tmp_path, "despike_rules", [])
    assert cc.returncode == 0, cc.stderr[-2000:]
    assert "warning" not in cc.stderr, cc.stderr[-2000:]
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_despike_rules_under_asan_ubsan(tmp_path):
    exe, cc = _build(tmp_path, "despike_rules_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)
