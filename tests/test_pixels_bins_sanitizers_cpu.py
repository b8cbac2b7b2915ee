"""
The mutual-information rule of the library (csrc/pixels_bins.hpp: the text k_pixels_mi runs per thread) under
AddressSanitizer + UndefinedBehaviorSanitizer on the host (tests/native/fuzz_pixels_bins.cpp): edge lists of 1 and of 31
entries, edges an ulp apart, NaN and +-inf pixels, pixels on an edge and an ulp beside it, histograms with empty rows, one
row, one column, no pair at all -- no sanitizer report, every bin inside its histogram and equal to a count of the edges
one by one, the score equal to a straightforward second evaluation and to itself at any stride.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_bin_rule_and_score_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "fuzz_pixels_bins")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-Wno-unknown-pragmas", os.path.join(HERE, "native", "fuzz_pixels_bins.cpp"), "-o", exe],
                        capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    r = subprocess.run([exe, "3000", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: 3000 iterations" in r.stdout, (r.stdout + r.stderr)[-3000:]
