"""CPU-side checks of the raw-frame entry points: declared in include/vslam_hip.h, exported by the library, reachable from the
ctypes layer.  What they compute is pinned on the GPU (tests/test_gpu_raw.py)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vslam_extractor_set_image_raw", "vslam_system_set_rectifiers", "vslam_system_track_stereo_raw",
               "vslam_batch_set_rectifiers", "vslam_batch_track_stereo_raw", "vslam_batch_track_stereo_prefetch_raw"]


def test_raw_entry_points_declared_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "vslam_hip.h")).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s


def test_python_layer_has_the_raw_forms(capi):
    assert callable(capi.Extractor.set_image_raw) and callable(capi.System.set_rectifiers) and callable(capi.Batch.set_rectifiers)
    for fn in (capi.System.track, capi.Batch.track, capi.Batch.track_prefetch):
        assert inspect.signature(fn).parameters["raw"].default is False, fn


def test_fused_kernels_are_in_the_library():
    """k_load_images_rect<1 / 3 / 4> exist as gfx950 kernels and use no scratch (tools/kernel_resources.py)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [r for r in kr.kernel_rows() if "k_load_images_rect" in r[0]]
    assert len(rows) == 3, [r[0] for r in rows]
    assert all(int(r[4]) == 0 for r in rows), rows
