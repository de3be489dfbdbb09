#!/usr/bin/env python3
"""Record tests/golden/pgo_single.npz: what vslam_pose_graph_optimize and vslam_pose_graph_move_points RETURN, byte for byte.

The file in the tree was recorded on an MI355X (gfx950, ROCm 7.2.0) from commit cb6998a, the last one whose single call had its
own kernels and its own Levenberg-Marquardt loop on the host.  Since then the single call is the one-lane case of the batched
solve, and tests/test_gpu_pgo.py::test_single_call_returns_recorded_bytes holds it to these bytes.  Nothing here comes from the
reference project: the inputs are the seeded graphs of tests/pgo_ref.py, the outputs are this library's.

The bytes depend on the compiler's code for the fp64 kernels.  After a compiler upgrade that moves them, re-record from a commit
whose single call is already trusted (one that passed this test under the old compiler), never from the commit under test.

usage: python tests/golden/make_pgo_single.py [out.npz]        (needs a GPU and the built library)"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("gtsam-vslam_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import pgo_ref as pr            # noqa: E402
import vslam_capi as vc         # noqa: E402
import test_gpu_pgo as tg       # noqa: E402

MOVE_SIZES = (1, 255, 257)


def optimize_cases():
    """name -> (poses, fixed, edges, keyword arguments)"""
    cases = {name: make() + ({},) for name, make in tg.GRAPHS.items()}
    poses, fixed, edges = tg.GRAPHS["ring8"]()
    cases["ring8_singular"] = (poses, fixed, [(i, j, Z, 0.0, 0.0) if 3 in (i, j) else (i, j, Z, a, b) for (i, j, Z, a, b) in edges], {})
    cases["exact"] = pr.exact_graph() + ({},)
    cases["ring8_all_fixed"] = (poses, np.ones(8, np.uint8), edges, {})
    cases["ring8_two_iterations"] = (poses, fixed, edges, dict(max_iterations=2, lambda0=10.0))
    return cases


def move_inputs(n):
    """the inputs of test_gpu_pgo.test_move_points"""
    rng = np.random.default_rng(n)
    A = np.array([pr.random_pose(rng, 1.0, 3.0) for _ in range(7)])
    B = np.array([pr.random_pose(rng, 1.0, 3.0) for _ in range(7)])
    B[2] = A[2]
    X = rng.uniform(-5, 5, (n, 3))
    ref = rng.integers(0, 7, n).astype(np.int32)
    if n > 1:
        ref[0] = 2; ref[-1] = -1
    return X, ref, A, B


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "pgo_single.npz")
    d = {}
    names = []
    for name, (poses, fixed, edges, kw) in optimize_cases().items():
        poses = np.ascontiguousarray(poses, np.float64)
        fixed = np.ascontiguousarray(fixed, np.uint8)
        ea = vc.pgo_edges(edges)[:len(edges)]
        out, rep = vc.pose_graph_optimize(poses, fixed, ea, **kw)
        names.append(name)
        d[name + "/poses"] = poses; d[name + "/fixed"] = fixed; d[name + "/edges"] = ea
        d[name + "/params"] = np.array([kw.get("max_iterations", 0), kw.get("lambda0", 0.0)])
        d[name + "/out"] = out
        d[name + "/report_int"] = np.array([rep[f[0]] for f in vc.PgoReport._fields_[:6]], np.int32)
        d[name + "/report_f64"] = np.array([rep[f[0]] for f in vc.PgoReport._fields_[6:]], np.float64)
        print(name, rep)
    for n in MOVE_SIZES:
        X, ref, A, B = move_inputs(n)
        d["move%d/X" % n] = X; d["move%d/ref" % n] = ref; d["move%d/A" % n] = A; d["move%d/B" % n] = B
        d["move%d/out" % n] = vc.pose_graph_move_points(X, ref, A, B)
    d["names"] = np.array(names)
    d["report_fields"] = np.array([f[0] for f in vc.PgoReport._fields_])
    np.savez_compressed(out_path, **d)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
