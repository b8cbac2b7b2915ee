"""
The last axis of a spline sample as a polynomial in its fraction (csrc/spline_last.hpp), compiled for the host, plain and
under AddressSanitizer + UndefinedBehaviorSanitizer (tests/native/poly_stage_rules.cpp): orders 1, 2 and 3 against a long
double evaluation of scipy's weights over the fractions 0, 2^-53, 1/2, 1 - 2^-53 and a seeded random set and row sums of
mixed sign and scale; the polynomial's maximum error may be twice that of the weight form it replaces, measured on the same
inputs against the same reference (both maxima are printed); a NaN or an infinity in any row sum gives a non-finite sample
at every fraction.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *extra, "-Wall", "-Wextra",
                         os.path.join(HERE, "native", "poly_stage_rules.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, cc


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ok: 3 orders" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.count("none finite") == 3 and r.stdout.count("allowed 2") == 3, r.stdout[-3000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_poly_stage_rules(tmp_path):
    """The plain build: runs wherever there is a host compiler."""
    exe, cc = _build(tmp_path, "poly_stage_rules", [])
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_poly_stage_rules_under_asan_ubsan(tmp_path):
    exe, cc = _build(tmp_path, "poly_stage_rules_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    _run(exe)
