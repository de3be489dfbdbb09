"""The grow-only buffer of the local-BA workspaces (gtsam-vslam_amd/csrc/grow_buf.hpp), built without a device under AddressSanitizer +
UBSan as a stand-alone program (tests/native/grow_buf.cpp) over a counting allocator that can be told to fail."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grow_buf_asan():
    """Each of the six growth rules at requests of 0, 1, exactly the capacity and capacity + 1 (capacity after growth, no allocation
    when the request fits, the site's synchronisation ahead of the free); an allocator that fails on its k-th call leaves p == nullptr
    and capacity 0, frees nothing twice, and the following request allocates afresh; release() frees exactly once and is idempotent;
    allocations equal frees at exit."""
    src = os.path.join(ROOT, "tests", "native", "grow_buf.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grow_buf")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "gtsam-vslam_amd", "csrc"), src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.splitlines()[-1].startswith("ok"), r.stdout + r.stderr
        assert "FAIL" not in r.stdout, r.stdout
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
