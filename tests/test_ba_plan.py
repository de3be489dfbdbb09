"""CPU tests of the batched local BA's launch plan: vslam_local_ba_batch_plan is the pure host function whose plan
vslam_local_ba_batch launches (no GPU needed).  Swept over the cohort shapes the batch can meet, every launch of every plan
must fit the 160 KB of LDS a workgroup gets, static LDS included (read from the gfx950 code objects' metadata with
tools/kernel_resources.py), the kernel forms must stay within their structural limits, and the production tracker shape
keeps its plan."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BYTES = 160 * 1024
BA2_MAX_F = 10          # k_ba_schur2 / k_ba_back2: tracker windows
BA_LDS_MAX_F = 20       # beyond: the one-problem path (windowed accumulation)
BA_WAVE_N = 60          # largest system the wave solve takes
KERNELS = ("k_ba_schur", "k_ba_schur2", "k_ba_back", "k_ba_back2", "k_ba_reduce", "k_ba_solve_mfma64", "k_ba_solve_wave", "k_ba_solve_mfma")
SOLVE_KERNEL = {1: "k_ba_solve_mfma64", 2: "k_ba_solve_wave", 4: "k_ba_solve_mfma"}
KIND = {1: "k_ba_schur", 2: "k_ba_schur2", 3: "k_ba_back", 4: "k_ba_back2"}
MAX_WAVES = {"k_ba_schur": 16, "k_ba_schur2": 16, "k_ba_back": 16, "k_ba_back2": 8}      # __launch_bounds__ / 64


@pytest.fixture(scope="module")
def static_lds():
    """static LDS bytes of the batch's kernels, from the built library's code objects"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernel_rows()
    out = {}
    for k in KERNELS:
        hit = [int(r[5]) for r in rows if re.search(k + r"(E|$)", r[0])]      # (mangled: ...k_ba_back2EPK..., demangled: ...::k_ba_back2)
        assert len(hit) == 1, (k, hit)
        out[k] = hit[0]
    return out


def _lane(F, slots, fac, lp, pairs=None):
    return dict(n_free_kf=F, n_points=lp, n_factors=max(1, 2 * lp) if F else 0, n_edges=max(F - 1, 0), n_pairs=pairs if pairs is not None else 2 * lp,
                max_slots=slots, max_factors=fac)


class _Planner:
    """vslam_local_ba_batch_plan through ctypes with the argument structs reused (the sweep makes ~10^6 calls)"""

    def __init__(self, capi, n_max=64):
        import ctypes as C
        self.C, self.capi, self.fn = C, capi, capi.lib().vslam_local_ba_batch_plan
        self.arr = (capi.BaLaneShape * n_max)()
        self.S = capi.BaBatchShape(0, self.arr, 4, 0)
        self.P = capi.BaBatchPlan()
        self.sp, self.pp = C.byref(self.S), C.byref(self.P)

    def set_lane(self, i, **kw):
        for k, v in kw.items():
            setattr(self.arr[i], k, int(v))

    def __call__(self):
        assert self.fn(self.sp, self.pp) == 0
        return self.P


def _check_launches(P, static, where):
    """every launch of the plan fits the LDS (dynamic + static) and its kernel's limits"""
    assert P.status == 0, where
    if P.n_batch == 0:
        assert (P.schur_kernel, P.back_kernel, P.solve_kinds) == (0, 0, 0), where
        return
    sk, bk = KIND[P.schur_kernel], KIND[P.back_kernel]
    assert sk in ("k_ba_schur", "k_ba_schur2") and bk in ("k_ba_back", "k_ba_back2"), where
    assert P.schur_lds + static[sk] <= LDS_BYTES, (where, sk, P.schur_lds, static[sk])
    assert P.back_lds + static[bk] <= LDS_BYTES, (where, bk, P.back_lds, static[bk])
    assert P.schur_lds > 0 and P.back_lds > 0, where
    for bit, k in SOLVE_KERNEL.items():
        if P.solve_kinds & bit:
            assert (P.solve_lds if bit == 4 else 0) + static[k] <= LDS_BYTES, (where, k)
    assert (P.solve_lds > 0) == bool(P.solve_kinds & 4), where
    assert static["k_ba_reduce"] <= LDS_BYTES
    # structure: the tracker-window forms only for tracker windows; waves from each kernel's menu; a block at least
    if sk == "k_ba_schur2":
        assert P.f_max <= BA2_MAX_F and P.max_slots <= BA2_MAX_F and P.schur_shared_w == 0, where
        assert P.schur_waves in (2, 4, 8, 16), where
    else:
        assert P.schur_waves in ((2, 4, 6, 8, 12, 16) if P.schur_shared_w else (2, 4, 8, 16)), where
        assert P.schur_shared_w == 0 or P.lookahead > 1, where
    if bk == "k_ba_back2":
        assert sk == "k_ba_schur2" and P.back_waves in (2, 4), where
    else:
        assert P.back_waves in (2, 4, 8) and P.back_shared == (1 if P.lookahead > 1 else 0), where
    assert P.schur_waves <= MAX_WAVES[sk] and P.back_waves <= MAX_WAVES[bk], where
    assert P.schur_blocks >= 1 and P.back_blocks >= 1, where
    assert 1 <= P.f_max <= BA_LDS_MAX_F and 1 <= P.max_slots <= P.f_max, where


def test_ba_batch_plan_sweep_fits_lds(capi, static_lds):
    """F 0..21 x max_slots 1..F x max_factors 1..2000 x lookahead 1..4 x lanes 1 / 2 / 16 / 64 x small / large landmark counts.
    Every value of max_factors for the tracker windows (F <= 10: the k_ba_schur2 / k_ba_back2 staging grows with it), a stride
    elsewhere and for the other lane counts.  Lane 0 carries the maxima; the other lanes are small tracker windows."""
    pl = _Planner(capi)
    full = list(range(1, 2001))
    coarse = sorted(set(range(1, 2001, 37)) | {2, 24, 100, 200, 232, 300, 379, 380, 450, 1000, 2000})
    n = 0
    for lanes in (1, 2, 16, 64):
        for lp in (5, 100000):
            pl.S.n_lanes = lanes
            for i in range(1, lanes):
                pl.set_lane(i, **_lane(1 + i % 10, 1 + i % 10, 2 + 2 * (i % 10), 5))
            dense = lanes == 2 and lp == 100000
            for F in range(0, 22):
                for slots in (range(1, F + 1) if F else [1]):
                    for NB in (1, 2, 4, 3):
                        pl.S.lookahead = NB
                        for fac in (full if (dense and F <= BA2_MAX_F) else coarse):
                            if fac < slots:
                                continue
                            pl.set_lane(0, **_lane(F, slots, fac, lp))
                            P = pl()
                            n += 1
                            where = (lanes, lp, F, slots, fac, NB)
                            _check_launches(P, static_lds, where)
                            single0 = F == 0 or F > BA_LDS_MAX_F
                            assert P.n_single == (1 if single0 else 0) and P.n_batch == lanes - P.n_single, where
                            if not single0:
                                assert P.f_max == max([F] + [1 + i % 10 for i in range(1, lanes)]) and P.max_factors >= fac and P.lp_max == lp, where
    assert n > 400000


def test_ba_batch_plan_back2_fits_with_many_view_landmarks(capi, static_lds):
    """k_ba_back2 stages 4 landmark-waves of the same front part k_ba_schur2 stages; with the system copy gone its staging is not
    bounded by k_ba_schur2's fit.  F = 10 windows whose landmarks carry ~230-400 factors (stereo views of ~120-200 keyframes):
    k_ba_schur2 fits with 2 waves; k_ba_back2 must halve to 2 waves too instead of asking for more than 160 KB."""
    for F, fac in ((10, 232), (10, 300), (10, 379), (6, 300), (3, 379)):
        P = capi.local_ba_batch_plan([_lane(F, F, fac, 3000)] * 4)
        assert P["status"] == 0 and P["schur_kernel"] == "schur2" and P["schur_waves"] == 2, (F, fac, P)
        assert P["back_kernel"] == "back2" and P["back_waves"] == 2, (F, fac, P)
        assert P["back_lds"] + static_lds["k_ba_back2"] <= LDS_BYTES, (F, fac, P)


def test_ba_batch_plan_production_shape(capi):
    """The default tracker cohort (windows of <= 10 free keyframes, <= 12 stereo views per landmark, 4 lambda candidates, MFMA
    solves) keeps its plan: k_ba_schur2 with 8 waves, k_ba_back2 with 4, the one-wave MFMA solve."""
    lanes = [_lane(4 + i % 7, 4 + i % 7, 24, 500 + 300 * i) for i in range(8)]
    P = capi.local_ba_batch_plan(lanes, lookahead=4, solver=0)
    assert P["status"] == 0 and P["n_batch"] == 8 and P["n_single"] == 0
    assert (P["schur_kernel"], P["schur_waves"], P["back_kernel"], P["back_waves"]) == ("schur2", 8, "back2", 4), P
    assert P["solves"] == {"mfma64"} and P["solve_lds"] == 0


def test_ba_batch_plan_routing(capi):
    """Problems outside the batched class go to the one-problem path: more than 20 free keyframes, empty graphs (no free keyframe,
    no factor, no pair), another rig, and - with the wave / LDS solves selected - systems beyond the wave solve's 60 unknowns."""
    win = _lane(10, 10, 24, 800)
    cases = [(dict(win, n_free_kf=21, max_slots=21), 1), (dict(win, n_free_kf=20, max_slots=20), 0), (dict(win, n_free_kf=0), 1),
             (dict(win, n_factors=0), 1), (dict(win, n_pairs=0), 1), (dict(win, own_rig=1), 1)]
    for ln, single in cases:
        P = capi.local_ba_batch_plan([win, ln])
        assert (P["n_single"], P["n_batch"]) == (single, 2 - single), (ln, P)
    for F, single in ((10, 0), (11, 1), (20, 1)):
        P = capi.local_ba_batch_plan([dict(win, n_free_kf=F, max_slots=F)], solver=1)
        assert P["n_single"] == single, (F, P)
        if not single:
            assert P["solves"] == {"wave"}
    P = capi.local_ba_batch_plan([dict(win, n_free_kf=4), dict(win, n_free_kf=14, max_slots=14), dict(win, n_free_kf=9)])
    assert P["solves"] == {"mfma64", "mfma"} and P["schur_kernel"] == "schur" and P["f_max"] == 14
    P = capi.local_ba_batch_plan([dict(win, n_free_kf=22)] * 3)
    assert (P["n_batch"], P["n_single"], P["schur_kernel"], P["back_kernel"], P["solves"]) == (0, 3, None, None, set())
    import vslam_capi
    with pytest.raises(vslam_capi.VslamError):
        capi.local_ba_batch_plan([win], lookahead=5)
    with pytest.raises(vslam_capi.VslamError):
        capi.local_ba_batch_plan([win], solver=2)
