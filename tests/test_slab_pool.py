"""Host code behind vslam_batch_restart_lane, built without a device: the key-slab free list (gtsam-vslam_amd/csrc/slab_pool.hpp)
under AddressSanitizer + UBSan with malloc / free as its allocator, and the queue removal of the mapping engine (job_engine.hpp,
JobEngine::cancel) under ThreadSanitizer."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_native(name, sanitize):
    src = os.path.join(ROOT, "tests", "native", name + ".cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, name)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "gtsam-vslam_amd", "csrc"), src, "-o", exe, "-lpthread"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("ok"), r.stdout + r.stderr
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_slab_pool_accounting_asan():
    """take / give / stats / destroy: reuse before allocation, best fit, refusals, every slab freed exactly once; lanes restarting on
    their own threads never share a slab and never hold more slabs than they use at once (bounded memory)."""
    _run_native("slab_pool_asan", "address,undefined")


def test_job_engine_cancel_tsan():
    """a job taken back from the engine's queues is never served; one that a thread has taken is served exactly once"""
    _run_native("engine_cancel_tsan", "thread")
