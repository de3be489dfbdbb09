"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every
symbol include/vslam_hip.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "vslam_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(vslam_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(capi):
    lib = ctypes.CDLL(capi.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 10
    assert "vslam_extractor_describe" in syms and "vslam_extractor_ssc_level" in syms      # the extractor's test taps
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing


def test_no_cpu_fallback_without_gpu(capi):
    """Without a device the product must fail loudly, never compute on the CPU."""
    if capi.device_count() > 0:
        return
    try:
        capi.Extractor(752, 480, 1500)
    except capi.VslamError as e:
        assert e.status == capi.ERR_NO_DEVICE
    else:
        raise AssertionError("extractor creation must fail without a GPU")


def test_product_does_not_reference_oracle():
    """Nothing under gtsam-vslam_amd/ may import, link or include the oracle."""
    pkg = os.path.join(ROOT, "gtsam-vslam_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h", "Makefile")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle" not in txt.lower().replace("no oracle", ""), os.path.join(dp, f)


def test_hot_path_kernels_have_no_scratch():
    """Register spills / stack objects of the built gfx950 code objects, read from their metadata (no GPU needed; tools/kernel_resources.py).
    Every kernel of the per-frame path must run without scratch memory; the two large-window solve kernels that still spill are pinned to
    what they use today, so that a regression (a dynamically indexed local array, a pointer phi the optimiser makes of two member stores,
    a register budget blown by an unroll) shows up in the CPU suite."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.kernel_rows()
    assert len(rows) >= 80
    allowed = {"k_ba_solveEPK": 352, "k_ba_solve_mfmaEPK": 64}      # (A/B solve for > 144 unknowns without MFMA; 61..256-unknown MFMA solve)
    bad = []
    for name, vgpr, agpr, sgpr, scratch, lds, wg in rows:
        limit = 0
        for key, v in allowed.items():
            if key in name:
                limit = v
        if int(scratch) > limit:
            bad.append((name, int(scratch)))
    assert not bad, bad
