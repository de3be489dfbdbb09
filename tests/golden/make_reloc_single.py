#!/usr/bin/env python3
"""Record tests/golden/reloc_single.npz: what vslam_relocalize and vslam_relocalize_debug RETURN on the crafted frames of
tests/test_gpu_reloc.py (RECORDED: hypothesis_case in mode 0, reloc_p3p_cases.find_case in mode 1, matching_scene shapes).

The file in the tree was recorded on an MI355X (gfx950, ROCm 7.2.0) from commit 85824ca, the last one whose single call had its
own by-value kernels, its own host loop and a refinement problem built on the host.  Since then the single call is the one-lane
case of the batched driver, and tests/test_gpu_reloc.py::test_single_call_returns_recorded_results holds it to these results.
Nothing here comes from the reference project: the inputs are the seeded generators of the tests, the outputs are this library's.
The inputs are not stored: a checksum of them is, so that a generator that drifts fails loudly instead of comparing other frames.

The pose and the LM doubles depend on the compiler's code for the fp64 kernels.  After a compiler upgrade that moves them, re-record
from a commit whose single call is already trusted (one that passed this test under the old compiler), never from the commit under
test.

usage: python tests/golden/make_reloc_single.py [out.npz]        (needs a GPU and the built library)"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("gtsam-vslam_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import pyoracle                 # noqa: E402
import vslam_capi as vc         # noqa: E402
import test_gpu_reloc as tg     # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "reloc_single.npz")
    pyoracle.lib()
    ge = vc.Extractor(tg.RIG["w"], tg.RIG["h"], 1500, batch=2)
    m = vc.Matcher(tg.RIG, ge, 0, ge, 1)
    inv_sigma = pyoracle.Extractor(1500).InvSigmaFactor
    d = {}
    for name in tg.RECORDED:
        got = tg.recorded_case(name, m, pyoracle, inv_sigma)
        for k, v in got.items():
            d[name + "/" + k] = v
        print(name, got["ints"].tolist(), got["f64"][16:].tolist())
    d["names"] = np.array(list(tg.RECORDED))
    np.savez_compressed(out_path, **d)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
