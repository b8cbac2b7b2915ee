"""
The library's four owning types (csrc/host_owned.hpp: device buffer, page-locked buffer, event, stream) on the host, against
a stub of the HIP calls they make that journals every allocation and free (tests/native/owned_rules.cpp), plain and under
AddressSanitizer + UndefinedBehaviorSanitizer: a move leaves its source empty and frees nothing, destruction frees exactly
once, reserve keeps its growth sizes and frees the old block before it makes the new one, a std::vector of buffers that
is resized and cleared frees each block once, and a borrowed stream is never destroyed.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, "-Wall", "-Wextra",
                         os.path.join(HERE, "native", "owned_rules.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok: owned rules" in r.stdout, (r.stdout + r.stderr)[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_owned_rules(tmp_path):
    """The plain build: runs wherever there is a host compiler."""
    exe, cc = _build(tmp_path, "owned_rules", [])
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_owned_rules_under_asan_ubsan(tmp_path):
    exe, cc = _build(tmp_path, "owned_rules_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)
