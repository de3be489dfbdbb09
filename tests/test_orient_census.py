"""Exhaustive census of the descriptor's cos / sin (tests/native/orient_census.cpp, a stand-alone host program; CPU only).

The hard claim: over EVERY float angle the kernel can see - 0 and [4e-5, 360] degrees, 193 739 350 values -
sincos_deg_range of gtsam-vslam_amd/csrc/orient_math.hpp (the code k_orient_desc runs) rotates the 512 pattern offsets
exactly as float(cos(double)), float(sin(double)) does.  Where the float route of the host libm (cosf / sinf) parts from that
is a property of the libm, so those counts are recorded (profiles/orient_census.json), not asserted; each listed angle is
checked to be one where the trig pair really differs.  tests/golden/orient_flip_cases.json holds, for the angles at which the
two routes sample different pixels, integer disc moments that produce the angle (recorded on glibc 2.35; regenerate with
`python tests/test_orient_census.py write-fixture`); here its entries are checked against the program and the oracle."""
import ctypes
import json
import math
import os
import platform
import struct
import subprocess
import sys
import tempfile
import time
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "orient_flip_cases.json")
PROFILE = os.path.join(ROOT, "profiles", "orient_census.json")
N_ANGLES = 193739349 + 1          # every float in [4e-5, 360], and 0.0


def run_census():
    src = os.path.join(ROOT, "tests", "native", "orient_census.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "orient_census")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-pthread", "-std=c++17", "-I", os.path.join(ROOT, "gtsam-vslam_amd", "csrc"),
                        src, "-o", exe], check=True)
        t0 = time.time()
        r = subprocess.run([exe, str(max(1, min(16, os.cpu_count() or 1))), "search"], capture_output=True, text=True, timeout=1200)
        secs = time.time() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(seconds=round(secs, 1), flip_kernel_vs_double=[], flip_double_vs_float=[], moments={}, unreachable=[])
    for line in r.stdout.splitlines():
        name, *v = line.split()
        if name.startswith("flip_") or name == "unreachable":
            out[name].append(int(v[0], 16))
        elif name == "moments":
            out["moments"][int(v[0], 16)] = (int(v[1]), int(v[2]))
        else:
            out[name] = int(v[0])
    return out


@pytest.fixture(scope="module")
def census():
    return run_census()


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_kernel_trig_rotates_every_offset_like_the_double_route(census):
    print("census: %d angles in %.1f s, kernel vs double: %d trig pairs, %d offset sets differ" %
          (census["angles"], census["seconds"], census["trig_kernel_vs_double"], census["offsets_kernel_vs_double"]))
    assert census["angles"] == N_ANGLES                      # the whole range, not a sample
    assert census["offsets_kernel_vs_double"] == 0, ["0x%08x" % b for b in census["flip_kernel_vs_double"]]
    assert census["flip_kernel_vs_double"] == []


def test_float_route_counts_are_recorded_and_each_flip_angle_differs(census):
    libm = ctypes.CDLL("libm.so.6")
    libm.cosf.restype = libm.sinf.restype = ctypes.c_float
    libm.cosf.argtypes = libm.sinf.argtypes = [ctypes.c_float]
    factor = _f32(_bits(math.pi / 180.0))
    flips = census["flip_double_vs_float"]
    assert len(flips) == census["offsets_double_vs_float"] <= census["trig_double_vs_float"]
    for b in flips:
        ang = _f32(_bits(_f32(b) * factor))                  # the float product the kernel and the oracle form
        dbl = (_bits(math.cos(ang)), _bits(math.sin(ang)))
        flt = (_bits(libm.cosf(ang)), _bits(libm.sinf(ang)))
        assert dbl != flt, "0x%08x" % b
    rec = dict(angles=census["angles"], trig_kernel_vs_double=census["trig_kernel_vs_double"],
               offsets_kernel_vs_double=census["offsets_kernel_vs_double"], trig_double_vs_float=census["trig_double_vs_float"],
               offsets_double_vs_float=census["offsets_double_vs_float"], flip_angles_reachable=len(census["moments"]),
               flip_angles_unreachable=len(census["unreachable"]), libc=" ".join(platform.libc_ver()),
               flip_double_vs_float=["0x%08x" % b for b in flips],
               route="double: float(cos(double(angle))); the reference's unqualified cos(float) could not be resolved without its "
                     "Eigen / OpenCV headers (DESIGN.md section 6 item 5)")
    print("float route of this libm: %d trig pairs and %d offset sets differ, %d of them reachable from integer moments" %
          (rec["trig_double_vs_float"], rec["offsets_double_vs_float"], rec["flip_angles_reachable"]))
    with open(PROFILE, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


def test_flip_fixture_is_what_the_program_finds(census, oracle):
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert len(fx["cases"]) >= 20
    for c in fx["cases"]:
        b = int(c["angle_bits"], 16)
        assert abs(c["m10"]) + abs(c["m01"]) <= 1248480
        assert _bits(oracle.fast_atan2(float(c["m01"]), float(c["m10"]))) == b, c
        if b in census["moments"]:                           # (the flip set belongs to the libm; the moments of an angle do not)
            assert census["moments"][b] == (c["m10"], c["m01"]), c
    if platform.libc_ver() == tuple(fx["libc"].split()):
        assert sorted(census["moments"]) == sorted(int(c["angle_bits"], 16) for c in fx["cases"])
        assert sorted(census["unreachable"]) == sorted(int(b, 16) for b in fx["unreachable"])


if __name__ == "__main__" and sys.argv[1:] == ["write-fixture"]:
    cs = run_census()
    with open(FIXTURE, "w") as f:
        json.dump(dict(libc=" ".join(platform.libc_ver()),
                       cases=[dict(angle_bits="0x%08x" % b, m10=m[0], m01=m[1]) for b, m in sorted(cs["moments"].items())],
                       unreachable=["0x%08x" % b for b in sorted(cs["unreachable"])]), f, indent=1)
        f.write("\n")
    print("%d cases, %d unreachable" % (len(cs["moments"]), len(cs["unreachable"])))
