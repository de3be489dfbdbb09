"""Raw (unrectified) frames end to end: rectification - and the gray conversion of BGR / BGRA sources - fused into the launch
that fills pyramid level 0 (k_load_images_rect), for the extractor, the session and the lockstep batch.  The reference for
every comparison is the EXISTING two-step path: Rectifier.remap on the host form (pinned to the CPU restatement of cv::remap
by test_gpu_rectify.py) fed to the existing gray entry point.  Level 0 must be equal byte for byte, keys and descriptors
field for field, the closed loop by the rule below.

Poses: two runs of the same kernels on the same gray input agree bit for bit until a local BA has run; after that the BA's LDS
atomics may sum in another order, so poses are compared to 1e-9 from the first local BA on (as in test_gpu_color.py /
test_gpu_batch.py); every integer report field, keyframe index and match table must still be equal."""
import ctypes as C
import numpy as np
import pytest
import synth
import vslam_capi
from test_color_host import colorize, assert_channels_differ

pytestmark = pytest.mark.gpu

G = (0.0, 9.81, 0.0)
NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)
INT_KEYS = [f[0] for f in vslam_capi.FrameReport._fields_ if f[0] != "ba_report"]

# EuRoC cam0 / cam1 (as tests/test_gpu_rectify.py), the rectified projection, and one with a wider field of view than the
# source so that taps leave the image (as tests/test_gpu_color.py)
K0 = [[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]]; D0 = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]
K1 = [[457.587, 0, 379.999], [0, 456.134, 255.238], [0, 0, 1]]; D1 = [-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05]
R0 = [[0.999966347530033, -0.001422739138722922, 0.008079580483432283], [0.001365741834644127, 0.9999741760894847, 0.007055629199258132],
      [-0.008089410156878961, -0.007044357138835809, 0.9999424675829176]]
R1 = [[0.9999633526194376, -0.003625811871560086, 0.007755443660172947], [0.003680398547259526, 0.9999684752771629, -0.007035845251224894],
      [-0.007729688520722713, 0.007064130529506649, 0.999945173484644]]
P0 = [[435.2046959714599, 0, 367.4517211914062], [0, 435.2046959714599, 252.2008514404297], [0, 0, 1]]
P_WIDE = [[300.0, 0, 367.0], [0, 300.0, 250.0], [0, 0, 1]]


def _device(capi, a):
    return capi.DeviceImage(np.ascontiguousarray(a))


def _padded(img, stride):
    """img (h, w[, cn]) in rows of `stride` bytes (padding filled with a pattern that must not leak into the result)"""
    h = img.shape[0]
    buf = np.full((h, stride), 0xA5, np.uint8)
    row = img.reshape(h, -1)
    buf[:, :row.shape[1]] = row
    return buf


def _centred(M, cx, cy):
    M = [list(r) for r in M]
    M[0][2], M[1][2] = cx, cy
    return M


def _source(sw, sh, seed, cn):
    g = synth.random_image(sw, sh, seed)
    if cn == 1:
        return g
    c = colorize(g, seed + 50, cn)
    assert_channels_differ(c)
    return c


# ---- 1. extractor: level 0 and keys ------------------------------------------------------------------------------------------
# (333 x 257 from 401 x 275: source != output size, widths that are a multiple of neither 4 nor 16 - three rows in four take the
#  scalar map loads, every row the byte tail; 752 x 480: the vector path)
@pytest.mark.parametrize("w,h,sw,sh,nfeat", [(333, 257, 401, 275, 300), (752, 480, 752, 480, 1500)])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_extractor_level0_and_keys(capi, w, h, sw, sh, nfeat, cn):
    L = capi.lib()
    small = (sw, sh) != (752, 480)
    srcs = [_source(sw, sh, 300 + 10 * cn + i, cn) for i in range(2)]
    eg = capi.Extractor(w, h, nfeat, batch=2)
    ex = capi.Extractor(w, h, nfeat, batch=2)
    for P in (P0, P_WIDE):
        Ka, Kb, Pn = (_centred(K0, sw / 2, sh / 2), _centred(K1, sw / 2 + 3, sh / 2 - 2), _centred(P, w / 2, h / 2)) if small else (K0, K1, P)
        rects = [capi.Rectifier(Ka, D0, R0, Pn, (sw, sh), (w, h)), capi.Rectifier(Kb, D1, R1, Pn, (sw, sh), (w, h))]
        ref = [rects[i].remap([srcs[i]])[0] for i in range(2)]
        # the two cameras' maps give different images of the same source: a swapped or shared map table cannot pass
        assert not np.array_equal(ref[0], rects[1].remap([srcs[0]])[0])
        assert not np.array_equal(ref[1], rects[0].remap([srcs[1]])[0])
        if P is P_WIDE:         # taps leave the source: whole regions are BORDER_CONSTANT 0
            assert (ref[0][0, :8] == 0).all() and (ref[0][-1, -8:] == 0).all()
        rkeys = eg.extract(ref)

        def check(tag):
            ex.run()
            for i in range(2):
                assert np.array_equal(ex.level(i, 0), ref[i]), (tag, i)
                k, d = ex.fetch(i)
                rk, rd = rkeys[i]
                assert len(k) == len(rk) and len(k) > 20, (tag, i, len(k), len(rk))
                for f in k.dtype.names:
                    assert np.array_equal(k[f], rk[f]), (tag, i, f)
                assert np.array_equal(d, rd), (tag, i)
                ex.set_image(i, np.zeros((h, w), np.uint8))         # (the next source must overwrite everything)

        for i in range(2):
            ex.set_image_raw(i, rects[i], srcs[i])
        check("host")
        dv = [_device(capi, s) for s in srcs]
        for i in range(2):
            ex.set_image_raw(i, rects[i], dv[i].ptr, channels=cn, on_device=True)
        check("device")
        stride = sw * cn + 13                                    # padded, not a multiple of 4
        pads = [_padded(s, stride) for s in srcs]
        for i in range(2):
            capi._chk(L.vslam_extractor_set_image_raw(ex.h, i, rects[i].h_r, capi._p(pads[i]), stride, cn, 0))
        check("host padded")
        dp = [_device(capi, p) for p in pads]
        for i in range(2):
            capi._chk(L.vslam_extractor_set_image_raw(ex.h, i, rects[i].h_r, C.c_void_p(dp[i].ptr), stride, cn, 1))
        check("device padded")
        for a in dv + dp:
            a.free()
        for r in rects:
            r.close()


def test_extractor_raw_image_keeps_the_others(capi):
    """a raw set_image on one image of a batch leaves the other image's level 0 as it was (one launch, nullptr = keep)"""
    g0 = synth.random_image(752, 480, 5)
    s1 = _source(752, 480, 6, 3)
    r = capi.Rectifier(K1, D1, R1, P0, (752, 480), (752, 480))
    ex = capi.Extractor(752, 480, 1500, batch=2)
    ex.set_image(0, g0)
    ex.set_image_raw(1, r, s1)
    ex.run()
    assert np.array_equal(ex.level(0, 0), g0) and np.array_equal(ex.level(1, 0), r.remap([s1])[0])
    r.close()


# ---- 3. the closed loop ------------------------------------------------------------------------------------------------------
D_LEFT = [-0.02, 0.004, 0, 0]
D_RIGHT = [-0.021, 0.0045, 1e-4, -5e-5]


def _rig_rectifiers(capi, dl=D_LEFT, dr=D_RIGHT):
    """K = P = the EuRoC rig's intrinsics, no rotation, a mild distortion per camera: the maps differ by fractions of a pixel
    and shift pixels by a few pixels, no tap leaves the image"""
    rig = synth.RIGS["euroc"]
    K = [[rig["fx"], 0, rig["cx"]], [0, rig["fy"], rig["cy"]], [0, 0, 1]]
    size = (rig["w"], rig["h"])
    return capi.Rectifier(K, dl, None, K, size, size), capi.Rectifier(K, dr, None, K, size, size)


def _velocity(f, fps):
    h = 1e-4
    return (synth.pose_at(f + h * fps, fps)[:3, 3] - synth.pose_at(f - h * fps, fps)[:3, 3]) / (2 * h)


def _bucket(f0, f1, fps):
    S, dts, _ = synth.imu_samples(f0, f1, fps, noise_seed=0x1A00 + f1)
    return (S[:, :3], S[:, 3:], np.arange(len(dts)) * 5e6)


def _compare_runs(a, b):
    """a, b: per frame (T, report, last_frame) + (counts, keyframes); returns the number of local BAs covered"""
    (oa, ca, ka), (ob, cb, kb) = a, b
    assert len(oa) == len(ob)
    ba = 0
    for n, ((P1, r1, l1), (P2, r2, l2)) in enumerate(zip(oa, ob)):
        for k in INT_KEYS:
            assert r1[k] == r2[k], (n, k, r1[k], r2[k])
        ba += r1["mapping_ran"] and r1["ba_keyframes"] > 0     # (timed mode: the BA's write-back landed before this frame's pose)
        if ba == 0:
            assert np.array_equal(P1, P2), n
        else:
            assert np.abs(P1 - P2).max() <= 1e-9, (n, np.abs(P1 - P2).max())
        if l1 is not None:
            assert np.array_equal(l1[0], l2[0]) and np.array_equal(l1[1], l2[1]), n
    assert ca == cb
    assert list(ka[0]) == list(kb[0])
    assert np.abs(ka[1] - kb[1]).max() <= (1e-9 if ba else 0.0)
    return ba


def _raw_frames(frames, cn, seed):
    """raw[n] = (left, right): the synthetic renders taken as the cameras' unrectified frames, gray or colourised"""
    synth.prerender(frames, "euroc")
    raw = []
    for n, f in enumerate(frames):
        L, R, _ = synth.stereo_frame(f, "euroc")
        if cn != 1:
            L, R = colorize(L, seed + 2 * n, cn), colorize(R, seed + 2 * n + 1, cn)
            if n == 0:
                assert_channels_differ(L)
        raw.append((L, R))
    return raw


def _system_run(capi, frames, images, rects=None, imu=False, on_device=False, **kw):
    """rects None: images are rectified gray frames for the gray entry point; else raw frames through track(raw=True)"""
    rig = synth.RIGS["euroc"]
    im = dict(gravity=G, noise=NOISE, T_bs=synth.T_BC1, hz=200, velocity=_velocity(frames[0], rig["fps"])) if imu else None
    s = capi.System(rig, 1500, T0=synth.pose_at(frames[0], rig["fps"]), imu=im, **kw)
    if rects:
        s.set_rectifiers(*rects)
    out = []
    for n, f in enumerate(frames):
        L, R = images[n]
        b = _bucket(frames[n - 1], f, rig["fps"]) if (imu and n > 0) else None
        if on_device:
            cn = 1 if L.ndim == 2 else L.shape[2]
            dl, dr = _device(capi, L), _device(capi, R)
            P, rep = s.track(dl.ptr, dr.ptr, n, imu_bucket=b, on_device=True, stride=rig["w"] * cn, channels=cn, raw=bool(rects))
            dl.free(); dr.free()
        else:
            P, rep = s.track(L, R, n, imu_bucket=b, raw=bool(rects))
        out.append((P, rep, s.last_frame() if n > 0 else None))
    s.wait_mapping()
    res = (out, s.counts(), s.keyframes())
    s.close()
    return res


def _two_step(rects, raw):
    return [(rects[0].remap([L])[0], rects[1].remap([R])[0]) for L, R in raw]


def _assert_reference_is_a_real_run(a):
    out, counts, _ = a
    assert counts["keyframes"] >= 4, counts
    assert min(r["n_inliers"] for _, r, _ in out[1:]) >= 100


@pytest.mark.parametrize("cn", [1, 3])
def test_system_euroc_host_raw(capi, cn):
    frames = list(range(0, 56, 2))
    rects = _rig_rectifiers(capi)
    raw = _raw_frames(frames, cn, 6000)
    gray = _two_step(rects, raw)
    if cn == 1:
        assert not np.array_equal(gray[0][0], raw[0][0])         # (the maps move pixels)
    a = _system_run(capi, frames, gray, local_mapping=1)
    _assert_reference_is_a_real_run(a)
    b = _system_run(capi, frames, raw, rects=rects, local_mapping=1)
    assert _compare_runs(a, b) >= 1
    for r in rects:
        r.close()


def test_system_timed_mode_device_bgra_imu_raw(capi):
    frames = list(range(0, 56, 2))
    rects = _rig_rectifiers(capi)
    raw = _raw_frames(frames, 4, 7000)
    kw = dict(imu=True, local_mapping=2, mapping_delay=4)
    a = _system_run(capi, frames, _two_step(rects, raw), **kw)
    _assert_reference_is_a_real_run(a)
    b = _system_run(capi, frames, raw, rects=rects, on_device=True, **kw)
    assert _compare_runs(a, b) >= 1
    for r in rects:
        r.close()


# ---- 4. the lockstep batch ---------------------------------------------------------------------------------------------------
def _batch_run(capi, schedules, images, masks, mode, lane_rects=None):
    """mode: 'host' (Batch.track), 'prefetch' (device images, track_prefetch with the next step's); lane_rects: per-lane
    rectifier pairs -> raw frames (lanes 0 .. B-2 bound by one call for every lane, the last lane rebound on its own)"""
    rig = synth.RIGS["euroc"]
    B = len(schedules)
    raw = lane_rects is not None
    bt = capi.Batch(rig, 1500, B, T0s=[synth.pose_at(sc[0], rig["fps"]) for sc in schedules], local_mapping=1, host_threads=2)
    if raw:
        bt.set_rectifiers(-1, *lane_rects[0])
        bt.set_rectifiers(B - 1, *lane_rects[B - 1])
    nSteps = len(masks)
    count = [0] * B
    fnums = []
    for step in range(nSteps):
        fn = []
        for b in range(B):
            fn.append(count[b])
            count[b] += masks[step][b]
        fnums.append(fn)
    out = [[] for _ in range(B)]
    dev = {}
    if mode == "prefetch":
        for step in range(nSteps):
            for b in range(B):
                if masks[step][b]:
                    L, R = images[b][fnums[step][b]]
                    dev[(step, b)] = (_device(capi, L), _device(capi, R))
    for step in range(nSteps):
        mask = masks[step]
        if mode == "host":
            Ls = [images[b][fnums[step][b]][0] if mask[b] else None for b in range(B)]
            Rs = [images[b][fnums[step][b]][1] if mask[b] else None for b in range(B)]
            T, reps = bt.track(Ls, Rs, fnums[step], mask=mask, raw=raw)
        else:
            im = images[0][0][0]
            cn = 1 if im.ndim == 2 else im.shape[2]
            Ls = [dev[(step, b)][0].ptr if mask[b] else None for b in range(B)]
            Rs = [dev[(step, b)][1].ptr if mask[b] else None for b in range(B)]
            nL = nR = nmask = None
            if step + 1 < nSteps:
                nmask = masks[step + 1]
                nL = [dev[(step + 1, b)][0].ptr if nmask[b] else None for b in range(B)]
                nR = [dev[(step + 1, b)][1].ptr if nmask[b] else None for b in range(B)]
            T, reps = bt.track_prefetch(Ls, Rs, fnums[step], nL, nR, mask=mask, next_mask=nmask, stride=rig["w"] * cn, channels=cn, raw=raw)
        for b in range(B):
            if mask[b]:
                out[b].append((T[b].copy(), reps[b], bt.system(b).last_frame() if fnums[step][b] > 0 else None))
    res = [(out[b], bt.system(b).counts(), bt.system(b).keyframes()) for b in range(B)]
    bt.close()
    for d in dev.values():
        d[0].free(); d[1].free()
    return res


def test_batch_host_raw_masked_and_device_prefetch(capi):
    B, nSteps = 4, 28
    schedules = [list(range(2 * b, 2 * b + 2 * nSteps, 2)) for b in range(B)]
    masks = [[1] * B for _ in range(nSteps)]
    masks[5][2] = 0                                  # lane 2 idles for one step
    shared = _rig_rectifiers(capi)
    other = _rig_rectifiers(capi, D_RIGHT, D_LEFT)   # lane 3: the two cameras exchanged - its own table entries
    lane_rects = [shared] * (B - 1) + [other]
    raw = [_raw_frames(schedules[b], 3, 8000 + 100 * b) for b in range(B)]
    gray = [_two_step(lane_rects[b], raw[b]) for b in range(B)]
    assert not np.array_equal(_two_step(shared, raw[B - 1][:1])[0][0], gray[B - 1][0][0])      # (lane 3's maps matter)
    ref = _batch_run(capi, schedules, gray, masks, "host")
    got = _batch_run(capi, schedules, raw, masks, "host", lane_rects)
    ba = sum(_compare_runs(ref[b], got[b]) for b in range(B))
    got = _batch_run(capi, schedules, raw, masks, "prefetch", lane_rects)
    ba += sum(_compare_runs(ref[b], got[b]) for b in range(B))
    assert ba >= 1
    for r in shared + other:
        r.close()


# ---- 5. invalid arguments ----------------------------------------------------------------------------------------------------
def test_invalid_raw_arguments(capi):
    L = capi.lib()
    rig = synth.RIGS["euroc"]
    w, h = rig["w"], rig["h"]
    K = [[rig["fx"], 0, rig["cx"]], [0, rig["fy"], rig["cy"]], [0, 0, 1]]
    g, _, _ = synth.stereo_frame(0, "euroc")
    col = colorize(g, 1, 4)                                     # (large enough for every channel count tried below)
    rl, rr = _rig_rectifiers(capi)
    small = capi.Rectifier(K, D_LEFT, None, K, (w, h), (w - 16, h))          # another output size
    wide = capi.Rectifier(K, D_LEFT, None, K, (w - 8, h), (w, h))            # another source size
    T = np.zeros(16); rep = capi.FrameReport()
    bad = [(2, w * 3), (3, w * 3 - 1), (4, w * 4 - 1), (1, w - 1), (0, w * 3)]

    def expect_invalid(st, what):
        assert st == capi.ERR_INVALID, (what, st)
        assert L.vslam_last_error().decode(), what

    # extractor
    ex = capi.Extractor(w, h, 1500)
    for cn, stride in bad:
        expect_invalid(L.vslam_extractor_set_image_raw(ex.h, 0, rl.h_r, capi._p(col), stride, cn, 0), ("extractor", cn, stride))
    expect_invalid(L.vslam_extractor_set_image_raw(ex.h, 0, None, capi._p(col), w, 1, 0), "extractor: no rectifier")
    expect_invalid(L.vslam_extractor_set_image_raw(ex.h, 0, small.h_r, capi._p(col), w, 1, 0), "extractor: output size")
    expect_invalid(L.vslam_extractor_set_image_raw(ex.h, 1, rl.h_r, capi._p(col), w, 1, 0), "extractor: image index")
    if capi.device_count() > 1:
        far = capi.Rectifier(K, D_LEFT, None, K, (w, h), (w, h), device=1)
        expect_invalid(L.vslam_extractor_set_image_raw(ex.h, 0, far.h_r, capi._p(col), w, 1, 0), "extractor: other device")
        far.close()
    (k, _), = ex.extract([g])
    assert len(k) > 100

    # session
    s = capi.System(rig, 1500, local_mapping=1)

    def sys_raw(cn, stride):
        return L.vslam_system_track_stereo_raw(s.h_sys, capi._p(col), capi._p(col), stride, cn, 0, 0, None, capi._p(T), C.byref(rep))

    expect_invalid(sys_raw(1, w), "system: nothing bound")
    expect_invalid(L.vslam_system_set_rectifiers(s.h_sys, rl.h_r, None), "system: one rectifier")
    expect_invalid(L.vslam_system_set_rectifiers(s.h_sys, small.h_r, small.h_r), "system: output size")
    expect_invalid(L.vslam_system_set_rectifiers(s.h_sys, rl.h_r, wide.h_r), "system: source sizes differ")
    expect_invalid(sys_raw(1, w), "system: still nothing bound")
    s.set_rectifiers(rl, rr)
    for cn, stride in bad:
        expect_invalid(sys_raw(cn, stride), ("system", cn, stride))
    s.set_rectifiers(None, None)
    expect_invalid(sys_raw(1, w), "system: unbound again")
    P, r0 = s.track(g, g, 0)                         # the handle still tracks gray frames
    assert np.isfinite(P).all() and r0["frame"] == 0
    s.close()

    # batch and prefetch
    bt = capi.Batch(rig, 1500, 2, local_mapping=1)
    lp = (C.c_void_p * 2)(col.ctypes.data, col.ctypes.data); fr = np.zeros(2, np.int32); TT = np.zeros((2, 16))
    reps = (capi.FrameReport * 2)()

    def batch_raw(cn, stride):
        return L.vslam_batch_track_stereo_raw(bt.h_b, lp, lp, stride, cn, 0, capi._p(fr), None, None, capi._p(TT), reps)

    def prefetch_raw(cn, stride):
        return L.vslam_batch_track_stereo_prefetch_raw(bt.h_b, lp, lp, stride, cn, capi._p(fr), None, None, capi._p(TT), reps, None, None, None)

    expect_invalid(batch_raw(1, w), "batch: nothing bound")
    expect_invalid(prefetch_raw(1, w), "prefetch: nothing bound")
    expect_invalid(L.vslam_batch_set_rectifiers(bt.h_b, 2, rl.h_r, rr.h_r), "batch: lane out of range")
    expect_invalid(L.vslam_batch_set_rectifiers(bt.h_b, -1, rl.h_r, None), "batch: one rectifier")
    expect_invalid(L.vslam_batch_set_rectifiers(bt.h_b, -1, small.h_r, small.h_r), "batch: output size")
    expect_invalid(L.vslam_batch_set_rectifiers(bt.h_b, 0, rl.h_r, wide.h_r), "batch: source sizes differ")
    bt.set_rectifiers(0, rl, rr)
    expect_invalid(batch_raw(1, w), "batch: lane 1 not bound")
    bt.set_rectifiers(-1, rl, rr)
    for cn, stride in bad:
        expect_invalid(batch_raw(cn, stride), ("batch", cn, stride))
        expect_invalid(prefetch_raw(cn, stride), ("prefetch", cn, stride))
    bt.set_rectifiers(-1, None, None)
    expect_invalid(batch_raw(1, w), "batch: unbound again")
    expect_invalid(prefetch_raw(1, w), "prefetch: unbound again")
    T2, reps2 = bt.track([g, g], [g, g], [0, 0])
    assert np.isfinite(T2).all()
    bt.close()
    for r in (rl, rr, small, wide):
        r.close()
