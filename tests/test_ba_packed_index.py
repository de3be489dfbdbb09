"""The index map of k_ba_schur2's packed accumulator (gtsam-vslam_amd/csrc/ba_packed.hpp), built without a device under
AddressSanitizer + UBSan as a stand-alone program (tests/native/ba_packed_index.cpp)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_packed_index_map_asan():
    """F = 1..10: the packed offsets of all (a <= b, i, j) and of the right-hand side are distinct and inside the stated size, the
    row-major <-> packed maps agree with them in both directions, entries below the block diagonal map to "absent"."""
    src = os.path.join(ROOT, "tests", "native", "ba_packed_index.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ba_packed_index")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "gtsam-vslam_amd", "csrc"), src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("ok"), r.stdout + r.stderr
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
