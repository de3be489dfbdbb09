// The shim's OpenCV branch (include/vslam_adapter.hpp under -DVSLAM_WITH_OPENCV) compiled by g++ against the stand-in headers
// in tests/native/cv_stub/ and linked against libvslam_hip.so (tests/test_color_host.py: it compiles and links; tests/
// test_gpu_color.py: its results on colour frames equal the ctypes gray path on the converted frames).
//
// adapter_color_run: caller buffers wrapped in cv::Mat of 1, 3 (BGR) or 4 (BGRA) channels, the closed loop through
// FeatureTracker::TrackImage(cv::Mat, cv::Mat, ...) (local mapping inline), then FeatureExtractor::extractKeysNew(cv::Mat&, ...)
// on the first left image.  Exceptions (e.g. a 2-channel image) are caught here and returned as -1 with their message: nothing
// unwinds through the C boundary.
#include "../../include/vslam_adapter.hpp"
#include <cstdio>
#include <cstdlib>

using namespace GTSAM_VIOSLAM_HIP;

extern "C" int adapter_color_run(const uint8_t* frames /* n x 2 x h rows of `stride` bytes */, int n, int w, int h, int channels,
                                 int stride, const vslam_rig* rig, int nfeat, const double* T0, double* out /* per frame 20 doubles */,
                                 vslam_keypoint* keys, uint8_t* desc, int cap, int* nKeys, char* err, int errCap) {
    try {
        const size_t img = (size_t)stride * h;
        vslam_system_config cfg{};
        cfg.fe.n_features = nfeat; cfg.fe.n_levels = 8; cfg.fe.scale = 1.2f; cfg.fe.edge_threshold = 19; cfg.fe.patch_size = 31;
        cfg.fe.max_fast_threshold = 20; cfg.fe.min_fast_threshold = 7;
        cfg.rig = *rig; cfg.device = 0; cfg.use_imu = 0; cfg.local_mapping = 1; cfg.window = 10;
        memcpy(cfg.T_wc_init, T0, sizeof(cfg.T_wc_init));
        auto map = std::make_shared<Map>(cfg);
        FeatureTracker tracker(map);
        for (int f = 0; f < n; f++) {
            const cv::Mat L(h, w, CV_8UC(channels), (void*)(frames + (size_t)(2 * f) * img), (size_t)stride);
            const cv::Mat R(h, w, CV_8UC(channels), (void*)(frames + (size_t)(2 * f + 1) * img), (size_t)stride);
            tracker.TrackImage(L, R, f);
            double* o = out + (size_t)f * 20;
            memcpy(o, tracker.lastPose, 16 * sizeof(double));
            o[16] = tracker.lastReport.n_inliers; o[17] = tracker.lastReport.keyframe_inserted; o[18] = tracker.lastReport.mapping_ran;
            o[19] = tracker.lastReport.n_map_points;
        }
        int kf = 0, mp = 0, act = 0, fr = 0;
        map->counts(kf, mp, act, fr);
        // extractKeysNew(cv::Mat&, ...) on the first left image
        FeatureExtractor fe(w, h, nfeat);
        cv::Mat im(h, w, CV_8UC(channels), (void*)frames, (size_t)stride);
        std::vector<cv::KeyPoint> kps;
        cv::Mat d;
        fe.extractKeysNew(im, kps, d);
        *nKeys = (int)kps.size();
        for (int i = 0; i < (int)kps.size() && i < cap; i++) {
            keys[i] = vslam_keypoint{kps[i].pt.x, kps[i].pt.y, kps[i].size, kps[i].angle, kps[i].response, kps[i].octave, kps[i].class_id};
            memcpy(desc + (size_t)i * 32, d.ptr<uint8_t>(i), 32);
        }
        return kf;
    } catch (const std::exception& e) {
        if (err && errCap > 0) snprintf(err, (size_t)errCap, "%s", e.what());
        return -1;
    }
}

#ifdef VSLAM_LINK_MAIN
// usage: adapter_color frames.raw n w h channels fx fy cx cy baseline nfeat   (frames.raw: n x (left, right) images of w x channels bytes per row)
int main(int argc, char** argv) {
    if (argc < 12) { fprintf(stderr, "usage: %s frames.raw n w h channels fx fy cx cy baseline nfeat\n", argv[0]); return 2; }
    const int n = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]), cn = atoi(argv[5]);
    vslam_rig rig{};
    rig.width = w; rig.height = h; rig.fx = atof(argv[6]); rig.fy = atof(argv[7]); rig.cx = atof(argv[8]); rig.cy = atof(argv[9]);
    rig.baseline = (float)atof(argv[10]);
    std::vector<uint8_t> buf((size_t)n * 2 * w * cn * h);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(buf.data(), 1, buf.size(), f) != buf.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    const double T0[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<double> out((size_t)n * 20);
    std::vector<vslam_keypoint> keys(4096);
    std::vector<uint8_t> desc((size_t)4096 * 32);
    int nk = 0;
    char err[256] = "";
    const int kf = adapter_color_run(buf.data(), n, w, h, cn, w * cn, &rig, atoi(argv[11]), T0, out.data(), keys.data(), desc.data(), 4096, &nk,
                                     err, sizeof(err));
    if (kf < 0) { fprintf(stderr, "%s\n", err); return 1; }
    printf("%d keyframes; %d keypoints in the first left image\n", kf, nk);
    for (int i = 0; i < n; i++) printf("frame %d: t = (%.6f %.6f %.6f) inliers %.0f\n", i, out[20 * i + 3], out[20 * i + 7], out[20 * i + 11], out[20 * i + 16]);
    return 0;
}
#endif
