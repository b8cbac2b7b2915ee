"""
The planner of the mutual-information launches of the Carrington sweep (csrc/sweep_mi_plan.hpp) on the host, under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/native/sweep_mi_rules.cpp): every slot of a launch in exactly one
group of 16 whatever the padding, the chunk walks partitioning tile lists of 1..40 entries for 1..7 chunks, the LDS and
histogram bytes against a brute-force count for all 31 x 31 pairs of edge counts, the chunk heuristic's range, and every
refusal -- code, message and order -- with the requests either side of each limit.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-Wall", "-Wextra",
                         os.path.join(HERE, "native", "sweep_mi_rules.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: sweep mi rules" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sweep_mi_rules(tmp_path):
    """The plain build: runs wherever there is a host compiler."""
    exe, cc = _build(tmp_path, "sweep_mi_rules", [])
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sweep_mi_rules_under_asan_ubsan(tmp_path):
    exe, cc = _build(tmp_path, "sweep_mi_rules_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)
