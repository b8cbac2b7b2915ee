"""
The destretch rule of the library (csrc/pixels_field.hpp: the text k_pixels_destretch runs per thread) under
AddressSanitizer + UndefinedBehaviorSanitizer on the host (tests/native/fuzz_pixels_field.cpp): fields of one node,
ragged centres, centres a hair apart, pixels far outside the field, huge offsets and node values, planes of one row or
column -- no sanitizer report, cell and tap indices always inside their arrays, bit-reproducible.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_field_rule_stays_inside_its_arrays_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "fuzz_pixels_field")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-Wno-unknown-pragmas", os.path.join(HERE, "native", "fuzz_pixels_field.cpp"), "-o", exe],
                        capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        pytest.skip("no sanitizer runtime for g++ here")
    assert cc.returncode == 0, cc.stderr[-2000:]
    r = subprocess.run([exe, "4000", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: 4000 iterations" in r.stdout, (r.stdout + r.stderr)[-3000:]
