// A C++ caller of the mono + IMU mode through include/vslam_adapter.hpp: VSlamSystem::InitializeMonocular's construction
// sequence (src/System.cpp:27-34) and VSlamSystem::TrackMonoIMU (:82-85) on the shim's classes, with the namespace as the only
// change, compiled by g++ and LINKED against libvslam_hip.so (tests/test_cpp_link_mono.py: the CPU test builds and links it as
// a shared wrapper and as a program; the GPU test loads adapter_mono_run() and compares it call by call with the ctypes path).
#include "../../include/vslam_adapter.hpp"
#include <cstdio>
#include <cstdlib>

using namespace GTSAM_VIOSLAM_HIP;

struct MonoConfig {            // what the reference reads from its yaml ConfigFile
    vslam_rig rig; double fps; const double* T0; const double* gravity; const double* noise /* gyro density, gyro walk, acc density, acc walk */;
    const double* TBodyToCam; int hz;
};

struct VSlamSystem {
    std::shared_ptr<Map> mMap;
    std::shared_ptr<Camera> mMonoCamera;
    std::shared_ptr<StereoCamera> mStereoCamera;
    std::shared_ptr<FeatureExtractor> mFeatureExtractorLeft, mFeatureExtractorRight;
    std::shared_ptr<FeatureMatcher> mFeatureMatcher;
    std::shared_ptr<FeatureTracker> mFeatureTracker;
    explicit VSlamSystem(const MonoConfig& c) {
        mMap = std::make_shared<Map>();
        InitializeMonocular(c);
    }
    void InitializeMonocular(const MonoConfig& c) {
        mMonoCamera = std::make_shared<Camera>();                                       // Camera(mConfigFile, "Camera_l")
        mMonoCamera->fx = c.rig.fx; mMonoCamera->fy = c.rig.fy; mMonoCamera->cx = c.rig.cx; mMonoCamera->cy = c.rig.cy;
        memcpy(mMonoCamera->TBodyToCam, c.TBodyToCam, sizeof(mMonoCamera->TBodyToCam));
        for (int k = 0; k < 3; k++) mMonoCamera->mIMUGravity[k] = c.gravity[k];
        mMonoCamera->mIMUData = std::make_shared<IMUData>(c.noise[0], c.noise[1], c.noise[2], c.noise[3], c.hz);
        mStereoCamera = std::make_shared<StereoCamera>(mMonoCamera, nullptr);
        mStereoCamera->mWidth = c.rig.width; mStereoCamera->mHeight = c.rig.height; mStereoCamera->mFps = (float)c.fps;
        memcpy(mStereoCamera->mCameraPose.pose, c.T0, sizeof(mStereoCamera->mCameraPose.pose));
        mFeatureExtractorLeft = std::make_shared<FeatureExtractor>();
        mFeatureMatcher = std::make_shared<FeatureMatcher>(mStereoCamera, mFeatureExtractorLeft, mFeatureExtractorLeft);
        mFeatureTracker = std::make_shared<FeatureTracker>(mStereoCamera, mFeatureExtractorLeft, mFeatureExtractorRight, mMap);
    }
    void TrackMonoIMU(const uint8_t* imLRect, int stride, const int frameNumb, const IMUData& IMUDataVal) {
        mFeatureTracker->TrackImageMonoIMU(imLRect, stride, frameNumb, std::make_shared<IMUData>(IMUDataVal));
    }
};

// frames: n x h x w gray; call f has frame number frameNumb[f] and the IMU samples [bucketStart[f], bucketStart[f + 1]) of
// acc / gyro (x 3) / ts; out: 20 doubles per call (pose, state, inliers, map points, keyframe inserted)
extern "C" int adapter_mono_run(const uint8_t* frames, int n, int w, int h, const vslam_rig* rig, double fps, const double* T0,
                                const double* gravity, const double* noise, const double* TBodyToCam, int hz, const int* frameNumb,
                                const int* bucketStart, const double* acc, const double* gyro, const double* ts, double* out) {
    try {
        MonoConfig c{*rig, fps, T0, gravity, noise, TBodyToCam, hz};
        c.rig.width = w; c.rig.height = h;
        VSlamSystem sys(c);
        if (!sys.mFeatureTracker->mono || sys.mFeatureExtractorLeft->nFeatures != 2000 || sys.mFeatureExtractorRight) return -2;
        for (int f = 0; f < n; f++) {
            IMUData d(noise[0], noise[1], noise[2], noise[3], hz);
            const int b0 = bucketStart[f], b1 = bucketStart[f + 1];
            d.mvAccelBuffer.assign(acc + 3 * (size_t)b0, acc + 3 * (size_t)b1); d.mvGyroBuffer.assign(gyro + 3 * (size_t)b0, gyro + 3 * (size_t)b1);
            d.mvTimestamps.assign(ts + b0, ts + b1);
            sys.TrackMonoIMU(frames + (size_t)f * w * h, w, frameNumb[f], d);
            double* o = out + (size_t)f * 20;
            memcpy(o, sys.mStereoCamera->mCameraPose.pose, 16 * sizeof(double));
            const vslam_mono_frame_report& r = sys.mFeatureTracker->lastMonoReport;
            o[16] = r.state; o[17] = r.n_inliers; o[18] = r.n_map_points; o[19] = r.keyframe_inserted;
        }
        int kf, mp, act, fr;
        sys.mMap->counts(kf, mp, act, fr);
        return kf;
    } catch (const std::exception& e) {
        fprintf(stderr, "adapter_mono_run: %s\n", e.what());
        return -1;
    }
}

#ifdef VSLAM_LINK_MAIN
// usage: adapter_mono_link frames.raw n w h fx fy cx cy fps imu.txt   (frames.raw: n gray u8 images; imu.txt: per call one line
// "frame_number samples", then `samples` lines "ax ay az gx gy gz t_ns")
int main(int argc, char** argv) {
    if (argc < 11) { fprintf(stderr, "usage: %s frames.raw n w h fx fy cx cy fps imu.txt\n", argv[0]); return 2; }
    const int n = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]);
    vslam_rig rig{};
    rig.width = w; rig.height = h; rig.fx = atof(argv[5]); rig.fy = atof(argv[6]); rig.cx = atof(argv[7]); rig.cy = atof(argv[8]);
    std::vector<uint8_t> buf((size_t)n * w * h);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(buf.data(), 1, buf.size(), f) != buf.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    std::vector<int> numb(n), start(n + 1, 0);
    std::vector<double> acc, gyro, ts;
    f = fopen(argv[10], "r");
    for (int i = 0; f && i < n; i++) {
        int m = 0;
        if (fscanf(f, "%d %d", &numb[i], &m) != 2) { fclose(f); f = nullptr; break; }
        for (int k = 0; k < m; k++) {
            double v[7];
            if (fscanf(f, "%lf %lf %lf %lf %lf %lf %lf", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6) != 7) { fclose(f); f = nullptr; break; }
            acc.insert(acc.end(), v, v + 3); gyro.insert(gyro.end(), v + 3, v + 6); ts.push_back(v[6]);
        }
        start[i + 1] = (int)ts.size();
    }
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[10]); return 2; }
    fclose(f);
    const double T0[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, g[3] = {0, 9.81, 0}, noise[4] = {1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3};
    std::vector<double> out((size_t)n * 20);
    const int kf = adapter_mono_run(buf.data(), n, w, h, &rig, atof(argv[9]), T0, g, noise, T0, 200, numb.data(), start.data(), acc.data(),
                                    gyro.data(), ts.data(), out.data());
    if (kf < 0) return 1;
    for (int i = 0; i < n; i++)
        printf("call %d: state %.0f t = (%.6f %.6f %.6f) inliers %.0f map points %.0f\n", i, out[20 * i + 16], out[20 * i + 3], out[20 * i + 7],
               out[20 * i + 11], out[20 * i + 17], out[20 * i + 18]);
    printf("%d keyframes\n", kf);
    return 0;
}
#endif
