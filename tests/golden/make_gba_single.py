#!/usr/bin/env python3
"""Record tests/golden/gba_single.npz: what vslam_global_ba RETURNS, byte for byte, on four cases of tests/gba_ref.py.

The file in the tree was recorded on an MI355X (gfx950) from commit 360e8fd, the last one whose kernels held their bodies
themselves.  Since then the bodies live in csrc/gba_dev.hpp, where the kernels of vslam_global_ba_batch call them too, and
tests/test_gpu_gba_golden.py holds the single call to these bytes.  Nothing here comes from the reference project: the inputs are
the seeded problems of tests/gba_ref.py, the outputs are this library's.

The bytes depend on the compiler's code for the fp64 kernels.  After a compiler upgrade that moves them, re-record from a commit
whose single call is already trusted (one that passed the test under the old compiler), never from the commit under test.

usage: python tests/golden/make_gba_single.py [out.npz]        (needs a GPU and the built library)"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("gtsam-vslam_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import gba_ref as gr            # noqa: E402
import vslam_capi as vc         # noqa: E402

NAMES = ("mixed", "dense12", "outliers", "rejected")
N_INT = 10                      # the report's leading int32 fields (the last is reserved)


def run(name):
    """(result dict of the single call, report as (int32 [10], float64 [3]))"""
    prob, edges = gr.CASES[name]()
    got = vc.global_ba(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob, edges, **gr.PARAMS.get(name, {}))
    rep = got["report"]
    fields = [f[0] for f in vc.GbaReport._fields_]
    ri = np.array([rep.get(f, 0) for f in fields[:N_INT]], np.int32)
    rf = np.array([rep[f] for f in fields[N_INT:]], np.float64)
    return got, ri, rf


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "gba_single.npz")
    d = {}
    for name in NAMES:
        got, ri, rf = run(name)
        d[name + "/kf_pose"] = got["kf_pose"]; d[name + "/lm"] = got["lm"]; d[name + "/pair_wrong"] = got["pair_wrong"]
        d[name + "/report_int"] = ri; d[name + "/report_f64"] = rf
        print(name, got["report"])
    d["names"] = np.array(NAMES)
    d["report_fields"] = np.array([f[0] for f in vc.GbaReport._fields_])
    np.savez_compressed(out_path, **d)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
