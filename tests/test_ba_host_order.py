"""The host side of local BA (gtsam-vslam_amd/csrc/ba_order_host.hpp, ba_plan.hpp: factor ordering, slot tables, membership, second-pass
statistics, window work lists, launch plans), built without a device under AddressSanitizer + UBSan as a stand-alone program
(tests/native/ba_host_order.cpp)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_host_order_asan():
    """Fixed-seed problems (K 1..12, L 0..300, every pair_flags value, random chi2 flags, fixed keyframes, unsorted ids, landmark shards,
    with and without a worker pool): everything BaPassHost writes equals a brute-force stable sort, pooled = serial bytewise, the arena
    formula bounds the layout, second_pass equals a recount, the window lists hold every (landmark, row pair) once and their cuts tile
    them, and every LDS size of ba_single_plan fits or the plan refuses."""
    src = os.path.join(ROOT, "tests", "native", "ba_host_order.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ba_host_order")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                        "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "gtsam-vslam_amd", "csrc"),
                        src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("ok"), r.stdout + r.stderr
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
