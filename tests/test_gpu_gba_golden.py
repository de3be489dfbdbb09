"""vslam_global_ba returns the recorded bytes.  tests/golden/gba_single.npz holds what the call returned on four cases of
tests/gba_ref.py while its kernels still held their bodies themselves (tests/golden/make_gba_single.py says from which commit and
how to re-record).  The bodies now live in csrc/gba_dev.hpp, shared with the kernels of vslam_global_ba_batch: this test shows
that the move changed no byte, and it is the pin for making the single call the one-lane case of the batched one."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_gba_single as mk           # noqa: E402

pytestmark = pytest.mark.gpu


def test_single_call_returns_recorded_bytes(capi):
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gba_single.npz")) as z:
        gold = {k: z[k] for k in z.files}
    assert [str(f) for f in gold["report_fields"]] == [f[0] for f in capi.GbaReport._fields_]
    names = [str(n) for n in gold["names"]]
    assert names == ["mixed", "dense12", "outliers", "rejected"]
    for name in names:
        got, ri, rf = mk.run(name)
        print(name, got["report"])
        assert ri.tobytes() == gold[name + "/report_int"].tobytes(), name
        assert rf.tobytes() == gold[name + "/report_f64"].tobytes(), name
        for k in ("kf_pose", "lm", "pair_wrong"):
            assert got[k].tobytes() == gold[name + "/" + k].tobytes(), (name, k)
    assert gold["rejected/report_int"][2] >= 1          # the case with a rejected trial
