"""Colour frames end to end (BGR / BGRA converted to gray on the device, as the reference's TrackImage does with cvtColor,
src/FeatureTracker.cpp:1130-1144).  The reference for every comparison is the numpy conversion (test_color_host.bgr_to_gray)
fed to the EXISTING gray entry point: extractor level 0 and keys, the closed loop (host / device, stereo / stereo + IMU,
EuRoC / KITTI), the lockstep batch (host, masked lane, device with prefetch), the rectifier (remap per channel, then convert),
the C++ shim's cv::Mat dispatch, and the argument checks of every new entry point.

Poses: two runs of the same kernels on the same gray input agree bit for bit until a local BA has run; after that the BA's LDS
atomics may sum in another order, so poses are compared to 1e-9 from the first local BA on (as in test_gpu_batch.py /
test_cpp_link.py); every integer report field, keyframe index and match table must still be equal."""
import ctypes as C
import numpy as np
import pytest
import synth
import vslam_capi
from test_color_host import bgr_to_gray, colorize, assert_channels_differ, build_adapter_color

pytestmark = pytest.mark.gpu

G = (0.0, 9.81, 0.0)
NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)
INT_KEYS = [f[0] for f in vslam_capi.FrameReport._fields_ if f[0] != "ba_report"]


def _device(capi, a):
    return capi.DeviceImage(np.ascontiguousarray(a))


def _padded(img, stride):
    """img (h, w, cn) in rows of `stride` bytes (padding filled with a pattern that must not leak into the result)"""
    h = img.shape[0]
    buf = np.full((h, stride), 0xA5, np.uint8)
    buf[:, :img.shape[1] * img.shape[2]] = img.reshape(h, -1)
    return buf


# ---- 1. extractor level 0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(752, 480), (1241, 376)])
@pytest.mark.parametrize("cn", [3, 4])
def test_extractor_level0_and_keys(capi, w, h, cn):
    g = synth.random_image(w, h, 40 + cn)
    col = colorize(g, 100 + w + cn, cn)
    assert_channels_differ(col)
    ref = bgr_to_gray(col)
    eg = capi.Extractor(w, h, 1500)
    (rk, rd), = eg.extract([ref])
    ex = capi.Extractor(w, h, 1500)
    L = capi.lib()

    def check(tag):
        ex.run()
        assert np.array_equal(ex.level(0, 0), ref), tag
        k, d = ex.fetch(0)
        assert len(k) == len(rk) and len(k) > 100, tag
        for f in k.dtype.names:
            assert np.array_equal(k[f], rk[f]), (tag, f)
        assert np.array_equal(d, rd), tag
        ex.set_image(0, np.zeros((h, w), np.uint8))         # (the next source must overwrite everything)

    ex.set_image(0, col)
    check("host")
    di = _device(capi, col)
    ex.set_image_device(0, di.ptr, w * cn, channels=cn)
    check("device")
    stride = w * cn + 13                                     # padded, not a multiple of 16
    pad = _padded(col, stride)
    capi._chk(L.vslam_extractor_set_image_color(ex.h, 0, capi._p(pad), stride, cn, 0))
    check("host padded")
    dp = _device(capi, pad)
    capi._chk(L.vslam_extractor_set_image_color(ex.h, 0, C.c_void_p(dp.ptr), stride, cn, 1))
    check("device padded")
    di.free(); dp.free()


def test_extractor_colour_image_keeps_the_others(capi):
    """a colour set_image on one image of a batch leaves the other images' level 0 as it was (one launch, nullptr = keep)"""
    g0 = synth.random_image(752, 480, 5)
    c1 = colorize(synth.random_image(752, 480, 6), 9, 3)
    ex = capi.Extractor(752, 480, 1500, batch=2)
    ex.set_image(0, g0)
    ex.set_image(1, c1)
    ex.run()
    assert np.array_equal(ex.level(0, 0), g0) and np.array_equal(ex.level(1, 0), bgr_to_gray(c1))


# ---- 2. the closed loop ------------------------------------------------------------------------------------------------------
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


def _system_run(capi, rig_name, nfeat, frames, images, imu=False, on_device=False, **kw):
    """images[n] = (left, right, channels); device: uploaded here"""
    rig = synth.RIGS[rig_name]
    im = dict(gravity=G, noise=NOISE, T_bs=synth.T_BC1, hz=200, velocity=_velocity(frames[0], rig["fps"])) if imu else None
    s = capi.System(rig, nfeat, T0=synth.pose_at(frames[0], rig["fps"]), imu=im, **kw)
    out = []
    for n, f in enumerate(frames):
        L, R, cn = images[n]
        b = _bucket(frames[n - 1], f, rig["fps"]) if (imu and n > 0) else None
        if on_device:
            dl, dr = _device(capi, L), _device(capi, R)
            P, rep = s.track(dl.ptr, dr.ptr, n, imu_bucket=b, on_device=True, stride=rig["w"] * cn, channels=cn)
            dl.free(); dr.free()
        else:
            P, rep = s.track(L, R, n, imu_bucket=b)
        out.append((P, rep, s.last_frame() if n > 0 else None))
    s.wait_mapping()
    res = (out, s.counts(), s.keyframes())
    s.close()
    return res


def _colour_frames(rig_name, frames, cn, seed):
    synth.prerender(frames, rig_name)
    col, gray = [], []
    for n, f in enumerate(frames):
        L, R, _ = synth.stereo_frame(f, rig_name)
        cl, cr = colorize(L, seed + 2 * n, cn), colorize(R, seed + 2 * n + 1, cn)
        if n == 0:
            assert_channels_differ(cl)
        col.append((cl, cr, cn))
        gray.append((bgr_to_gray(cl), bgr_to_gray(cr), 1))
    return col, gray


def test_system_euroc_host_bgr(capi):
    frames = list(range(0, 80, 2))
    col, gray = _colour_frames("euroc", frames, 3, 1000)
    a = _system_run(capi, "euroc", 1500, frames, gray, local_mapping=1)
    b = _system_run(capi, "euroc", 1500, frames, col, local_mapping=1)
    assert _compare_runs(a, b) >= 1


def test_system_timed_mode_device_bgra_imu(capi):
    frames = list(range(0, 60, 2))
    col, gray = _colour_frames("euroc", frames, 4, 2000)
    kw = dict(imu=True, local_mapping=2, mapping_delay=4)
    a = _system_run(capi, "euroc", 1500, frames, gray, **kw)
    b = _system_run(capi, "euroc", 1500, frames, col, on_device=True, **kw)
    assert _compare_runs(a, b) >= 1


def test_system_kitti_host_bgr(capi):
    frames = list(range(0, 90, 3))
    col, gray = _colour_frames("kitti", frames, 3, 3000)
    a = _system_run(capi, "kitti", 2000, frames, gray, local_mapping=1)
    b = _system_run(capi, "kitti", 2000, frames, col, local_mapping=1)
    _compare_runs(a, b)
    assert a[1]["keyframes"] >= 2


# ---- 3. the lockstep batch ---------------------------------------------------------------------------------------------------
def _batch_run(capi, schedules, images, masks, mode):
    """mode: 'host' (Batch.track), 'prefetch' (device images, vslam_batch_track_stereo_prefetch_color with the next step's)"""
    rig = synth.RIGS["euroc"]
    B = len(schedules)
    bt = capi.Batch(rig, 1500, B, T0s=[synth.pose_at(sc[0], rig["fps"]) for sc in schedules], local_mapping=1, host_threads=2)
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
                    L, R, cn = images[b][fnums[step][b]]
                    dev[(step, b)] = (_device(capi, L), _device(capi, R))
    for step in range(nSteps):
        mask = masks[step]
        if mode == "host":
            Ls = [images[b][fnums[step][b]][0] if mask[b] else None for b in range(B)]
            Rs = [images[b][fnums[step][b]][1] if mask[b] else None for b in range(B)]
            T, reps = bt.track(Ls, Rs, fnums[step], mask=mask)
        else:
            cn = images[0][0][2]
            Ls = [dev[(step, b)][0].ptr if mask[b] else None for b in range(B)]
            Rs = [dev[(step, b)][1].ptr if mask[b] else None for b in range(B)]
            nL = nR = nmask = None
            if step + 1 < nSteps:
                nmask = masks[step + 1]
                nL = [dev[(step + 1, b)][0].ptr if nmask[b] else None for b in range(B)]
                nR = [dev[(step + 1, b)][1].ptr if nmask[b] else None for b in range(B)]
            T, reps = bt.track_prefetch(Ls, Rs, fnums[step], nL, nR, mask=mask, next_mask=nmask, stride=rig["w"] * cn, channels=cn)
        for b in range(B):
            if mask[b]:
                out[b].append((T[b].copy(), reps[b], bt.system(b).last_frame() if fnums[step][b] > 0 else None))
    res = [(out[b], bt.system(b).counts(), bt.system(b).keyframes()) for b in range(B)]
    bt.close()
    for d in dev.values():
        d[0].free(); d[1].free()
    return res


def test_batch_host_bgr_masked_and_device_prefetch(capi):
    B, nSteps = 4, 28
    schedules = [list(range(2 * b, 2 * b + 2 * nSteps, 2)) for b in range(B)]
    masks = [[1] * B for _ in range(nSteps)]
    masks[5][2] = 0                                  # lane 2 idles for one step
    col, gray = [], []
    for b in range(B):
        c, g = _colour_frames("euroc", schedules[b], 3, 4000 + 100 * b)
        col.append(c); gray.append(g)
    ref = _batch_run(capi, schedules, gray, masks, "host")
    got = _batch_run(capi, schedules, col, masks, "host")
    ba = sum(_compare_runs(ref[b], got[b]) for b in range(B))
    got = _batch_run(capi, schedules, col, masks, "prefetch")
    ba += sum(_compare_runs(ref[b], got[b]) for b in range(B))
    assert ba >= 1


# ---- 4. rectifier --------------------------------------------------------------------------------------------------------------
K0 = [[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]]; D0 = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]
R0 = [[0.999966347530033, -0.001422739138722922, 0.008079580483432283], [0.001365741834644127, 0.9999741760894847, 0.007055629199258132],
      [-0.008089410156878961, -0.007044357138835809, 0.9999424675829176]]
P0 = [[435.2046959714599, 0, 367.4517211914062], [0, 435.2046959714599, 252.2008514404297], [0, 0, 1]]
P_WIDE = [[300.0, 0, 367.0], [0, 300.0, 250.0], [0, 0, 1]]        # wider field of view than the source: taps leave the image


@pytest.mark.parametrize("P", [P0, P_WIDE])
def test_rectifier_remap_gray(capi, P):
    import rectify as orc
    sw, sh = 752, 480
    mx, my = orc.init_undistort_rectify_map(K0, D0, R0, P, sw, sh)
    r = capi.Rectifier(K0, D0, R0, P, (sw, sh), (sw, sh))
    L = capi.lib()
    for cn in (3, 4):
        imgs = [colorize(synth.random_image(sw, sh, 70 + k), 80 + k + cn, cn) for k in range(2)]
        assert_channels_differ(imgs[0])
        ref = [bgr_to_gray(np.stack([orc.remap_linear(np.ascontiguousarray(im[..., c]), mx, my) for c in range(cn)], -1)) for im in imgs]
        out = r.remap(imgs)                                           # host form
        for k in range(2):
            assert np.array_equal(out[k], ref[k]), (cn, k)
        src = [_device(capi, im) for im in imgs]                      # device form
        dst = [_device(capi, np.zeros((sh, sw), np.uint8)) for _ in imgs]
        r.remap_device([s.ptr for s in src], sw * cn, [d.ptr for d in dst], sw, channels=cn)
        for k in range(2):
            got = np.zeros((sh, sw), np.uint8)
            capi._chk(L.vslam_device_download(0, capi._p(got), C.c_void_p(dst[k].ptr), C.c_size_t(got.nbytes)))
            assert np.array_equal(got, ref[k]), (cn, k, "device")
        for a in src + dst:
            a.free()
    # channels = 1 is the gray remap
    g = [synth.random_image(sw, sh, 99)]
    want = r.remap(g)[0]
    got = np.zeros((sh, sw), np.uint8)
    sp = (C.c_void_p * 1)(g[0].ctypes.data); dp = (C.c_void_p * 1)(got.ctypes.data)
    capi._chk(L.vslam_rectifier_remap_gray_host(r.h_r, sp, sw, 1, dp, sw, 1))
    assert np.array_equal(got, want) and np.array_equal(want, orc.remap_linear(g[0], mx, my))
    r.close()


# ---- 5. the C++ shim's cv::Mat dispatch ------------------------------------------------------------------------------------------
def test_adapter_trackimage_bgr_matches_gray_path(capi, tmp_path):
    so = build_adapter_color(tmp_path, True)
    A = C.CDLL(so)
    A.adapter_color_run.restype = C.c_int
    rig = synth.RIGS["euroc"]
    w, h = rig["w"], rig["h"]
    frames = list(range(0, 40, 2))
    col, gray = _colour_frames("euroc", frames, 3, 5000)
    buf = np.ascontiguousarray(np.stack([np.stack([c[0], c[1]]) for c in col]))         # n x 2 x h x w x 3
    T0 = np.ascontiguousarray(synth.pose_at(frames[0], rig["fps"]))
    crig = capi.make_rig(rig)

    def run(data, cn):
        out = np.zeros((len(frames), 20)); keys = np.zeros(4096, capi.KP_DTYPE); desc = np.zeros((4096, 32), np.uint8)
        nk = C.c_int(); err = C.create_string_buffer(512)
        kf = A.adapter_color_run(capi._p(data), len(frames), w, h, cn, w * cn, C.byref(crig), 1500, capi._p(T0), capi._p(out),
                                 capi._p(keys), capi._p(desc), 4096, C.byref(nk), err, 512)
        return kf, out, keys[:nk.value], desc[:nk.value], err.value.decode()

    kf, out, keys, desc, err = run(buf, 3)
    assert kf >= 2, err
    s = capi.System(rig, 1500, T0=T0, local_mapping=1)
    ba = 0
    for n in range(len(frames)):
        Pg, rep = s.track(gray[n][0], gray[n][1], n)
        ba += rep["mapping_ran"]
        d = np.abs(Pg.reshape(16) - out[n, :16]).max()
        assert (d == 0.0) if ba == 0 else (d <= 1e-9), (n, d)
        assert (rep["n_inliers"], rep["keyframe_inserted"], rep["mapping_ran"], rep["n_map_points"]) == tuple(int(v) for v in out[n, 16:20]), n
    assert s.counts()["keyframes"] == kf
    (rk, rd), = capi.Extractor(w, h, 1500).extract([gray[0][0]])
    assert len(keys) == len(rk) and all(np.array_equal(keys[f], rk[f]) for f in rk.dtype.names) and np.array_equal(desc, rd)
    # a 2-channel image: TrackImage throws, the entry point returns an error code
    two = np.ascontiguousarray(buf[..., :2])
    kf2, _, _, _, err2 = run(two, 2)
    assert kf2 == -1 and "channels" in err2, err2


# ---- 6. invalid arguments ----------------------------------------------------------------------------------------------------
def test_invalid_channels_and_strides(capi):
    L = capi.lib()
    rig = synth.RIGS["euroc"]
    w, h = rig["w"], rig["h"]
    g, _, _ = synth.stereo_frame(0, "euroc")
    col = colorize(g, 1, 3)
    T = np.zeros(16); rep = capi.FrameReport()
    bad = [(2, w * 3), (3, w * 3 - 1), (4, w * 4 - 1), (0, w * 3)]

    def expect_invalid(st, what):
        assert st == capi.ERR_INVALID, (what, st)
        assert L.vslam_last_error().decode(), what

    ex = capi.Extractor(w, h, 1500)
    for cn, stride in bad:
        expect_invalid(L.vslam_extractor_set_image_color(ex.h, 0, capi._p(col), stride, cn, 0), ("extractor", cn, stride))
    (k, _), = ex.extract([g])
    assert len(k) > 100

    s = capi.System(rig, 1500, local_mapping=1)
    for cn, stride in bad:
        expect_invalid(L.vslam_system_track_stereo_color(s.h_sys, capi._p(col), capi._p(col), stride, cn, 0, 0, None, capi._p(T), C.byref(rep)),
                       ("system", cn, stride))
    P, r0 = s.track(g, g, 0)                         # the handle still tracks gray frames
    assert np.isfinite(P).all() and r0["frame"] == 0
    s.close()

    bt = capi.Batch(rig, 1500, 2, local_mapping=1)
    lp = (C.c_void_p * 2)(col.ctypes.data, col.ctypes.data); fr = np.zeros(2, np.int32); TT = np.zeros((2, 16))
    reps = (capi.FrameReport * 2)()
    for cn, stride in bad:
        expect_invalid(L.vslam_batch_track_stereo_color(bt.h_b, lp, lp, stride, cn, 0, capi._p(fr), None, None, capi._p(TT), reps),
                       ("batch", cn, stride))
        expect_invalid(L.vslam_batch_track_stereo_prefetch_color(bt.h_b, lp, lp, stride, cn, capi._p(fr), None, None, capi._p(TT), reps,
                                                                 None, None, None), ("prefetch", cn, stride))
    T2, reps2 = bt.track([g, g], [g, g], [0, 0])
    assert np.isfinite(T2).all()
    bt.close()

    r = capi.Rectifier(K0, D0, R0, P0, (w, h), (w, h))
    out = np.zeros((h, w), np.uint8)
    dp = (C.c_void_p * 1)(out.ctypes.data); sp = (C.c_void_p * 1)(col.ctypes.data)
    for cn, stride in bad:
        expect_invalid(L.vslam_rectifier_remap_gray_host(r.h_r, sp, stride, cn, dp, w, 1), ("remap host", cn, stride))
    dcol = _device(capi, col); dout = _device(capi, out)
    dsp = (C.c_void_p * 1)(dcol.ptr); ddp = (C.c_void_p * 1)(dout.ptr)
    for cn, stride in bad:
        expect_invalid(L.vslam_rectifier_remap_gray(r.h_r, dsp, stride, cn, ddp, w, 1), ("remap device", cn, stride))
    dcol.free(); dout.free()
    assert r.remap([g])[0].shape == (h, w)
    r.close()
