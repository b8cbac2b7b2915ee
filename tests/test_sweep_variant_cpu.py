"""
The rule that picks one of the 71 k_sweep instantiations (csrc/sweep_variant.hpp: pure C++, no HIP) against the rules
restated independently in tests/native/sweep_variant_rules.cpp, over the full cross-product of 672 inputs: every pick is
the expected variant and an entry of the instantiation list, every entry is reached, and the list has 71 entries --
built with AddressSanitizer + UndefinedBehaviorSanitizer where the host compiler has them.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sweep_variant_pick_restates_the_dispatch_rules(tmp_path):
    exe = str(tmp_path / "sweep_variant_rules")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    src = [os.path.join(HERE, "native", "sweep_variant_rules.cpp"), "-o", exe]
    cc = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + src,
                        capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "cannot find" in cc.stderr:
        cc = subprocess.run(base + src, capture_output=True, text=True)  # (no sanitizer runtime: a plain build)
    assert cc.returncode == 0, cc.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok: 672 inputs, 71 variants (15 pitched), all reached" in r.stdout, \
        (r.stdout + r.stderr)[-3000:]
