"""The index rule of k_ssc's compact stopper array (gtsam-vslam_amd/csrc/ssc_stoppers.hpp), built without a device under
AddressSanitizer + UBSan as a stand-alone program (tests/native/ssc_stoppers.cpp)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ssc_stopper_rule_asan():
    """Every 0/1 array of 17..20 elements, seeded random arrays up to 2 100 elements over alphabets of 1, 2, 3, 17 and 256 values,
    sorted, reversed and organ-pipe inputs, each partitioned down to 16-element blocks: the capped one-array form and libstdc++'s
    sequential partition loop agree on the cut, the exchanges and the array of every segment; no slot of a segment's slice is
    written twice or read unwritten; the even-m, K = m / 2 case occurs."""
    src = os.path.join(ROOT, "tests", "native", "ssc_stoppers.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ssc_stoppers")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "gtsam-vslam_amd", "csrc"), src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("ok"), r.stdout + r.stderr
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
