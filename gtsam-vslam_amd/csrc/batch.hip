// vslam_batch: B independent sequences ("lanes") tracked in lockstep, one kernel launch per stage for ALL lanes.
//
// Why: a frame of one sequence is a chain of ~25 small kernels, most of them one workgroup wide (SSC per level, the
// ordered claim resolution of the projection match, the pose LM, the pre-integration) - it cannot fill 256 CUs, and the
// part runs at most ~4 kernels of different streams concurrently (tools/launchrate.hip), so independent sessions on
// their own streams stop scaling at about two sessions' worth.  Here every stage kernel is launched once with the
// lane as a grid dimension and a per-lane argument table (common.hpp lane_entry): the one-workgroup stages become
// B-workgroup launches of the same duration.
//
// Each lane is a complete vslam_system (system.hpp: the reference's Map / KeyFrame / MapPoint bookkeeping, keyframe rule,
// local mapping) bound to images 2b / 2b+1 of ONE shared extractor and to the batch's stream.  A step is
//   host  (thread pool, per lane)  frame_begin, candidate list                      [FeatureTracker::TrackImage :1115-1122]
//   device                         images -> pyramid, extraction of 2B images, stereo match of B pairs
//   host  (thread pool, per lane)  upload block: active map points, IMU bucket      (overlaps the extraction)
//   device                         one H2D, then predict / pre-integrate / project / solve / re-chain / re-predict /
//                                  project / solve / pack for all lanes, one D2H, one synchronisation
//   host  (per lane)               retry rule on lanes whose first round failed (their own launches, rare), then
//   host  (thread pool, per lane)  frame_post: bookkeeping, keyframe insertion, hand-off to the mapping threads
// Local mapping (find new points + local BA) of a lane runs on one of the batch's few mapping threads, so the number
// of streams competing for the hardware queues stays small.
//
// A lane's results are bit-identical to the same sequence run through a single vslam_system (tests/test_gpu_batch.py):
// the batched kernels are the one-session kernels' bodies, fed per-lane argument blocks built by the same host code.
//
// A lane is one robot: its own camera (rig intrinsics and baseline are per lane - every lane's matcher, TrackGeom and mapping
// problems are built from its own config; only image size, extractor parameters, device, IMU and mapping mode are the group's),
// its own start (frame number 0 initialises its map) and its own end (restart_lane: a new session in the lane's place, the key
// slabs of the old one back on the group's free list).
#include "system.hpp"
#include "pose_dev.hpp"
#include "imu_dev.hpp"
#include "track_dev.hpp"
#include "ba_pool.hpp"
#include "job_engine.hpp"
#include <chrono>
#include <malloc.h>

namespace vslam {
void launch_pose_batch(hipStream_t s, const PoseLane* dLanes, int B);
void launch_pose_imu_batch(hipStream_t s, const PoseLane* dLanes, int B, int ldsFactors);
void launch_imu_batch(hipStream_t s, const ImuLane* dLanes, int B);
}

namespace vslam { void ba_host_profile_print(); }
using namespace vslam;
using namespace vslam_sys;

namespace {
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
}


// ---- the mapping engine (local_mapping = 2) ------------------------------------------------------------------------------------
// The device work of the lanes' local-mapping passes, COHORT by cohort: the jobs the lanes of a group hand over during a host
// phase of a step are collected (vslam_batch::submit_mapping) and released together when that phase ends (kick).  An engine
// thread takes EVERYTHING that has been released when it becomes free - the new-point searches of the lanes that inserted a
// keyframe, the local BAs of the lanes that did a frames earlier - and runs it as ONE batched call (vslam_find_new_points_batch /
// vslam_local_ba_batch: one launch per stage for all of them).  One engine per device, shared by the lockstep groups of that
// device: a cohort then holds the jobs of every group (twice the lanes per launch with two groups, half the launches), and
// the cohort size adapts to the load - the longer a cohort takes, the more jobs the next one finds.
// VSLAM_MAP_ENGINE_PRIVATE=1: one engine per group (round-3 first form).
struct MapEngine {
    int device = 0;
    vslam::JobEngine<vslam_system*> eng;           // queues + threads (job_engine.hpp: host-only, ThreadSanitizer-tested)
    // local-BA stage timing of the cohorts (HIP events on the engine's stream), summed since the last read
    std::atomic<int> baTimingOn{0};
    std::atomic<long long> baCohortSeq{0};
    std::mutex btMu;
    std::vector<std::pair<const char*, float>> baTimes;
    long long baTimedCohorts = 0, baTimedLanes = 0;

    void release_jobs(std::deque<vslam_system*>& np, std::deque<vslam_system*>& ba) { eng.release_jobs(np, ba); }
    // the cohort's new-point searches: one upload, one launch per kernel, one download (vslam_find_new_points_batch)
    void serve_np(std::vector<vslam_system*>& jobs) {
        std::vector<const vslam_new_points_problem*> Ps; std::vector<vslam_new_points_result*> Rs;
        for (vslam_system* s : jobs) { Ps.push_back(&s->pass.np.P); Rs.push_back(&s->pass.np.R); }
        vslam_status st;
        { SysProfScope pn(sys_prof().npNs, sys_prof().npN); st = vslam_find_new_points_batch(Ps.data(), Rs.data(), (int)jobs.size(), device); }
        char err[200];
        snprintf(err, sizeof(err), "%s", st == VSLAM_OK ? "" : vslam_last_error());
        for (vslam_system* s : jobs) s->finish_job(st, err);
    }
    // the cohort's local BAs: ONE batched call (vslam_local_ba_batch: one launch per stage for all of them)
    void serve_ba(std::vector<vslam_system*>& jobs) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<const vslam_ba_problem*> Ps; std::vector<vslam_ba_result*> Rs;
        for (vslam_system* s : jobs) { Ps.push_back(&s->pass.ba.P); Rs.push_back(&s->pass.ba.R); }
        // stage timing (HIP events around every launch) on every 4th cohort while it is switched on: the events are launches of
        // their own on a launch-bound path (measured: all cohorts timed costs 8 % frames/s)
        const int timing = baTimingOn.load() && (baCohortSeq.fetch_add(1) % 4) == 0;
        vslam_local_ba_set_timing(timing);
        vslam_status st;
        { SysProfScope pb(sys_prof().baNs, sys_prof().baN); st = vslam_local_ba_batch(Ps.data(), Rs.data(), (int)jobs.size(), device); }
        if (st == VSLAM_OK && timing) {
            const char* nm[32]; float ms[32]; int n = 0;
            if (vslam_local_ba_timings(nm, ms, 32, &n) == VSLAM_OK) {
                std::lock_guard<std::mutex> lk(btMu);
                baTimedCohorts++; baTimedLanes += (long long)jobs.size();
                for (int i = 0; i < n; i++) {
                    size_t j = 0;
                    for (; j < baTimes.size(); j++) if (!strcmp(baTimes[j].first, nm[i])) break;
                    if (j == baTimes.size()) baTimes.push_back({nm[i], 0.f});
                    baTimes[j].second += ms[i];
                }
            }
        }
        char err[200];
        snprintf(err, sizeof(err), "%s", st == VSLAM_OK ? "" : vslam_last_error());
        for (vslam_system* s : jobs) s->finish_job(st, err);
        const long long d = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        SysProf& p = sys_prof();
        p.mqNs += d; p.mqN++; p.mqLate += (long long)jobs.size();
        if (d > 15000000) p.mapLate++;
        long long m = p.mapMaxNs.load(); while (d > m && !p.mapMaxNs.compare_exchange_weak(m, d)) {}
    }
    void start(int nNp, int nBa) {
        eng.lanes[0].serve = [this](std::vector<vslam_system*>& j) { serve_np(j); };
        eng.lanes[1].serve = [this](std::vector<vslam_system*>& j) { serve_ba(j); };
        eng.onThreadStart = [this]() { hipSetDevice(device); };
        eng.onThreadExit = []() { vslam::thread_release(); };
        eng.start(nNp, nBa);
    }
    ~MapEngine() { eng.shutdown(); }
    // one engine per device, alive while a group of that device holds it
    static std::shared_ptr<MapEngine> acquire(int device, int nBaThreads) {
        static std::mutex gMu;
        static std::weak_ptr<MapEngine> shared[64];
        static const bool priv = getenv("VSLAM_MAP_ENGINE_PRIVATE") && atoi(getenv("VSLAM_MAP_ENGINE_PRIVATE")) != 0;
        std::lock_guard<std::mutex> lk(gMu);
        std::shared_ptr<MapEngine> e = (priv || device < 0 || device >= 64) ? nullptr : shared[device].lock();
        if (!e) {
            e = std::make_shared<MapEngine>();
            e->device = device;
            const int nNp = getenv("VSLAM_MAP_NP_THREADS") ? std::max(1, atoi(getenv("VSLAM_MAP_NP_THREADS"))) : (priv ? 2 : 1);
            e->start(nNp, nBaThreads);
            if (!priv && device >= 0 && device < 64) shared[device] = e;
        }
        return e;
    }
};

struct vslam_batch {
    int B = 0, device = 0;
    bool useImu = false;
    vslam_extractor* fe = nullptr;
    hipStream_t stream = nullptr;
    // the two pre-integrations of a step run beside the matching passes that do not depend on them (one-workgroup-per-lane
    // kernels of ~90 us each): side stream + events, as the one-session path does
    hipStream_t imuStream = nullptr; hipEvent_t evTab = nullptr, evImu0 = nullptr, evSolve0 = nullptr, evImu1 = nullptr;
    std::vector<vslam_system*> sys;
    // per-lane argument tables of one step: pinned host block + device mirror (one H2D per step)
    struct Tables {
        StereoLane* stereo; PredictLane* predict; ImuLane* imu0; ProjLane* proj0; PoseLane* pose0; ImuLane* imu1;
        RepredictLane* repredict; ProjLane* proj1; PoseLane* pose1; PackLane* pack;
    } ht{}, dt{};
    uint8_t* h_tab = nullptr; uint8_t* d_tab = nullptr; size_t tabBytes = 0;
    uint8_t* h_up = nullptr; uint8_t* d_up = nullptr; size_t upCap = 0;      // upload block (map points, IMU buckets)
    uint8_t* h_dn = nullptr; uint8_t* d_dn = nullptr; size_t dnCap = 0;      // download block (per-lane tracking state)
    double* d_res = nullptr; double* h_res = nullptr;                        // [B][64] result blocks
    uint8_t* d_zero = nullptr; size_t zeroCap = 0;                           // MapPoint::GetIsOutlier of uploaded points: all 0
    BaPool pool;                                                             // host phases
    vslam_system_config shared{};                                            // lane 0's config at creation: the fields every lane shares
    vslam::SlabPool slabs;                                                   // the lanes' keyframe key slabs (HBM) + those handed back by restarts
    std::vector<uint8_t> needFirst;                                          // lane restarted: its next frame must carry frame number 0
    // mapping engine (shared by the groups of this device); the jobs of the current host phase wait here for kick()
    std::shared_ptr<MapEngine> eng;
    std::deque<vslam_system*> npPend, baPend;
    std::mutex pendMu;
    // per-step scratch
    struct LaneStep { bool on = false, first = false, failed = false; vslam_status st = VSLAM_OK; char err[200] = ""; size_t upOff = 0, dnOff = 0, keyOff = 0; int N = 0, nL = 0, nR = 0; bool wantKeys = false; void* keySlot = nullptr; };
    std::vector<LaneStep> ls;
    std::vector<const uint8_t*> imgPtrs;
    StageTimer timer;
    // host-side phase times of the last step (seconds): pre, extract enqueue, fill, tables + enqueue, wait, finish, post
    double phase[8] = {0}, phaseSum[8] = {0}, subSum[6] = {0};      // subSum: begin a / serve / b, post a / serve / b
    long long nSteps = 0;

    vslam_status init(const vslam_system_config* cfgs, int n, int hostThreads, int mapThreads);
    bool shares(const vslam_system_config& c) const;
    vslam_status make_lane(int b, const vslam_system_config& c, vslam_system** out);
    vslam_status restart_lane(int lane, const vslam_system_config* c);
    void release();
    vslam_status ensure_up(size_t bytes);
    vslam_status ensure_dn(size_t bytes);
    vslam_status serve_requests();
    vslam_status first_error();
    vslam_status host_begin(const int* frames, const vslam_imu_bucket* imu, bool candidates, bool needImu = true);
    // imuCall: vslam_batch_relocalize_imu (imu: the phase-2 lanes' buckets, ireps: [B]); else vslam_batch_relocalize (both null)
    vslam_status relocalize(const uint8_t* const* L, const uint8_t* const* R, int stride, bool onDevice, const int* frames, const uint8_t* mask,
                            const vslam_reloc_params* prm, double* T_wc_out, vslam_reloc_report* reps, bool imuCall = false,
                            const vslam_imu_bucket* imu = nullptr, vslam_reloc_imu_report* ireps = nullptr);
    // correct: vslam_batch_correct_loop (kfLoop [B], T_wc_corrected [B][16]); else vslam_batch_close_loop (both null)
    // ireps != null: the _imu forms for an IMU batch (the yaw-only correction of every masked lane about its own gravity)
    vslam_status loop(bool correct, const uint8_t* mask, const int32_t* kfLoop, const double* T_wc_corrected, const vslam_loop_params* prm,
                      vslam_loop_report* reps, vslam_loop_imu_report* ireps = nullptr);
    // what fuse_loop and global_ba refuse, in the order of loop(): the arguments and an IMU batch, (the parameters,) then any masked
    // lane's loop_check with the lane in the message; nothing has changed when one fails.  *nOn: masked lanes
    vslam_status followup_check_args(const char* fn, const uint8_t* mask, const void* reps) const;
    vslam_status followup_check_lanes(const char* fn, const uint8_t* mask, int* nOn) const;
    vslam_status fuse_loop(const uint8_t* mask, const vslam_fuse_loop_params* prm, vslam_fuse_loop_report* reps);
    vslam_status global_ba(const uint8_t* mask, const vslam_system_gba_params* prm, vslam_system_gba_report* reps);
    std::vector<uint8_t> rqDescs; std::vector<int> rqStart, rqBest;
    vslam_status step(const uint8_t* const* L, const uint8_t* const* R, int stride, int channels, bool onDevice, const int* frames,
                      const vslam_imu_bucket* imu, const uint8_t* mask, double* T_wc_out, vslam_frame_report* reps,
                      const uint8_t* const* nextL = nullptr, const uint8_t* const* nextR = nullptr, const uint8_t* nextMask = nullptr,
                      bool raw = false);
    // images of the NEXT step whose extraction was enqueued at the end of the previous one (prefetch)
    std::vector<const uint8_t*> prefetched; int prefetchedChannels = 1; bool prefetchedRaw = false;
    // raw: unrectified frames through each lane's rectifiers (sys[b]->rectL / rectR)
    vslam_status enqueue_extraction(const uint8_t* const* L, const uint8_t* const* R, const uint8_t* mask, int stride, int channels, bool onDevice,
                                    bool raw);
    std::vector<const vslam_rectifier*> rectPtrs;
    static void submit_mapping(void* self, vslam_system* s) {
        vslam_batch* b = (vslam_batch*)self;
        bool now = false;
        {
            std::lock_guard<std::mutex> lk(b->pendMu);
            (s->pass.stage == MapPass::NEW_POINTS ? b->npPend : b->baPend).push_back(s);
            // mapping_delay == mapping_np_delay: the lane waits for this local BA inside the same host phase - no cohort to wait for
            now = s->pass.stage == MapPass::LOCAL_BA && s->pass.commitFrame <= s->pass.npFrame;
        }
        if (now) b->kick();
    }
    void kick() {                                  // a host phase has ended: its jobs are released to the engine
        if (!eng) return;
        std::lock_guard<std::mutex> lk(pendMu);
        if (!npPend.empty() || !baPend.empty()) eng->release_jobs(npPend, baPend);
    }
};

// what the lanes of a group share: the extractor (image size, parameters), the device and its streams, the schedule.  The camera
// behind the images - fx, fy, cx, cy, baseline - is the lane's own.
bool vslam_batch::shares(const vslam_system_config& c) const {
    return c.device == shared.device && (c.use_imu != 0) == (shared.use_imu != 0) && c.rig.width == shared.rig.width &&
           c.rig.height == shared.rig.height && !memcmp(&c.fe, &shared.fe, sizeof(c.fe)) && c.local_mapping == shared.local_mapping &&
           c.mapping_delay == shared.mapping_delay && c.mapping_np_delay == shared.mapping_np_delay;
}
static const char* const kSharedRule = "lanes must share device, image size (rig width x height), extractor parameters, IMU mode and mapping mode / "
                                       "delays; rig intrinsics and baseline are per lane";

// a lane's session on the group's shared objects: extractor images 2b / 2b + 1, stream, result-block slices, mapping engine, slabs
vslam_status vslam_batch::make_lane(int b, const vslam_system_config& c, vslam_system** out) {
    vslam_system* s = new (std::nothrow) vslam_system();
    if (!s) return VSLAM_ERR_INVALID;
    *out = s;
    VS_CHECK(s->init(&c, fe, 2 * b, stream));
    vslam_matcher* m = s->fm;
    m->resExternal = true;
    m->d_res = d_res + (size_t)b * 64; m->h_res = h_res + (size_t)b * 64;
    m->d_poseIO = m->d_res; m->imuIo = m->d_res + 32; m->d_poseOut = (int*)(m->d_res + 48); m->d_trCount = (int*)(m->d_res + 52);
    m->trExternal = true;
    s->mapExec = &vslam_batch::submit_mapping; s->mapExecArg = this;
    s->slabPool = &slabs;
    return VSLAM_OK;
}

vslam_status vslam_batch::init(const vslam_system_config* cfgs, int n, int hostThreads, int nMapThreads) {
    if (!cfgs || n <= 0 || n > 256) { set_error("vslam_batch: 1..256 lanes"); return VSLAM_ERR_INVALID; }
    B = n; device = cfgs[0].device; useImu = cfgs[0].use_imu != 0;
    shared = cfgs[0];
    for (int b = 1; b < B; b++)
        if (!shares(cfgs[b])) { set_error("vslam_batch: %s", kSharedRule); return VSLAM_ERR_INVALID; }
    slabs.alloc = [](size_t bytes) -> void* { void* p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; };
    slabs.dealloc = [](void* p) { hipFree(p); };
    VS_HIP(hipSetDevice(device));
    {
        // Every keyframe keeps ~200 KB of key arrays on the host; by default glibc serves blocks of that size with one mmap each,
        // and a dozen host-phase threads doing that at every step queue on the process's mm lock (the copy of a key block took
        // 170 - 600 us instead of ~15).  Serve them from the (per-thread) heaps instead.  VSLAM_MALLOC_TUNE=0 leaves malloc alone.
        static std::once_flag once;
        std::call_once(once, [] {
            const char* e = getenv("VSLAM_MALLOC_TUNE");
            if (e && atoi(e) == 0) return;
            mallopt(M_MMAP_THRESHOLD, 64 << 20);
            mallopt(M_TRIM_THRESHOLD, 512 << 20);
            mallopt(M_TOP_PAD, 64 << 20);
        });
    }
    VS_HIP(vslam::create_main_stream(&stream));
    timer.stream = stream; timer.multi = true;
    VS_HIP(vslam::create_main_stream(&imuStream));
    for (hipEvent_t* e : {&evTab, &evImu0, &evSolve0, &evImu1}) VS_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    VS_CHECK(vslam_extractor_create(&shared.fe, shared.rig.width, shared.rig.height, 2 * B, device, &fe));
    VS_CHECK(fe->enable_double_output());
    VS_HIP(hipMalloc(&d_res, (size_t)B * 64 * sizeof(double)));
    VS_HIP(vslam::memset_sync(d_res, 0, (size_t)B * 64 * sizeof(double)));
    VS_HIP(hipHostMalloc(&h_res, (size_t)B * 64 * sizeof(double), hipHostMallocDefault));
    sys.assign(B, nullptr);
    ls.assign(B, LaneStep{});
    needFirst.assign(B, 0);
    for (int b = 0; b < B; b++) VS_CHECK(make_lane(b, cfgs[b], &sys[b]));
    // argument tables
    size_t off = 0;
    auto place = [&](size_t elem) { const size_t o = off; off = up256(off + elem * (size_t)B); return o; };
    const size_t oStereo = place(sizeof(StereoLane)), oPredict = place(sizeof(PredictLane)), oImu0 = place(sizeof(ImuLane)),
                 oProj0 = place(sizeof(ProjLane)), oPose0 = place(sizeof(PoseLane)), oImu1 = place(sizeof(ImuLane)),
                 oRep = place(sizeof(RepredictLane)), oProj1 = place(sizeof(ProjLane)), oPose1 = place(sizeof(PoseLane)), oPack = place(sizeof(PackLane));
    tabBytes = off;
    VS_HIP(hipHostMalloc((void**)&h_tab, tabBytes, hipHostMallocDefault));
    VS_HIP(hipMalloc((void**)&d_tab, tabBytes));
    memset(h_tab, 0, tabBytes);
    auto bindT = [&](Tables& t, uint8_t* base) {
        t.stereo = (StereoLane*)(base + oStereo); t.predict = (PredictLane*)(base + oPredict); t.imu0 = (ImuLane*)(base + oImu0);
        t.proj0 = (ProjLane*)(base + oProj0); t.pose0 = (PoseLane*)(base + oPose0); t.imu1 = (ImuLane*)(base + oImu1);
        t.repredict = (RepredictLane*)(base + oRep); t.proj1 = (ProjLane*)(base + oProj1); t.pose1 = (PoseLane*)(base + oPose1);
        t.pack = (PackLane*)(base + oPack);
    };
    bindT(ht, h_tab); bindT(dt, d_tab);
    if (hostThreads < 0) hostThreads = std::min(B, 8);
    pool.onExit = []() { vslam::thread_release(); };
    if (hostThreads > 1) pool.start(hostThreads - 1);
    if (shared.local_mapping == 2) {
        // mapping_threads = the engine's threads for the cohorts' batched local BAs (a second cohort may start while one is in its
        // last rounds), + its thread(s) for the cohorts' batched new-point searches
        if (nMapThreads <= 0) nMapThreads = getenv("VSLAM_BATCH_MAP_THREADS") ? std::max(1, atoi(getenv("VSLAM_BATCH_MAP_THREADS"))) : 3;
        eng = MapEngine::acquire(device, nMapThreads);
    }
    return VSLAM_OK;
}

void vslam_batch::release() {
    if (getenv("VSLAM_BATCH_PHASES") && nSteps)
        fprintf(stderr, "vslam_batch %d lanes, %lld steps, host phases (us / step): begin %.1f | images + extract enqueue %.1f | upload block %.1f | "
                        "tables + enqueue %.1f (of which waiting for the extraction %.1f) | wait %.1f | retry %.1f | post %.1f\n", B, nSteps, 1e6 * phaseSum[0] / nSteps, 1e6 * phaseSum[1] / nSteps,
                1e6 * phaseSum[2] / nSteps, 1e6 * phaseSum[3] / nSteps, 1e6 * phaseSum[7] / nSteps, 1e6 * phaseSum[4] / nSteps, 1e6 * phaseSum[5] / nSteps, 1e6 * phaseSum[6] / nSteps);
    if (getenv("VSLAM_BATCH_PHASES") && nSteps)
        fprintf(stderr, "  begin = first half (waits for the jobs that are due + commits) %.1f + requests %.1f + second half (BA collection, changePosesLCA, candidates) %.1f | "
                        "post = first half %.1f + requests %.1f + second half (new-point collection, reports) %.1f\n", 1e6 * subSum[0] / nSteps, 1e6 * subSum[1] / nSteps,
                1e6 * subSum[2] / nSteps, 1e6 * subSum[3] / nSteps, 1e6 * subSum[4] / nSteps, 1e6 * subSum[5] / nSteps);
    if (getenv("VSLAM_BATCH_PHASES")) {
        SysProf& p = sys_prof();
        auto avg = [](std::atomic<long long>& ns, std::atomic<long long>& n) { return n.load() ? 1e-3 * (double)ns.load() / (double)n.load() : 0.0; };
        fprintf(stderr, "  per-lane host work so far (us per call x calls): changePosesLCA %.1f x %lld | keyframe insertion %.1f x %lld | calcDescriptor round trip "
                        "%.1f x %lld | frame_post %.1f x %lld\n", avg(p.lcaNs, p.lcaN), p.lcaN.load(), avg(p.kfNs, p.kfN), p.kfN.load(), avg(p.descNs, p.descN),
                p.descN.load(), avg(p.postNs, p.postN), p.postN.load());
        fprintf(stderr, "  mapping passes: %.1f us x %lld (find new points %.1f, vslam_local_ba %.1f) | frames that waited for their mapper: %.1f us x %lld\n",
                avg(p.mapNs, p.mapN), p.mapN.load(), avg(p.npNs, p.npN), avg(p.baNs, p.baN), avg(p.waitNs, p.waitN), p.waitN.load());
        fprintf(stderr, "  sections (total ms): KF new_keyframe %.1f | observations %.1f | stereo refill %.1f | descriptor request %.1f | key slot %.1f | connections %.1f | "
                        "keys from block %.1f (%lld by fetch_keys) || ba_collect %.1f | np_commit_a %.1f | ba_commit_a %.1f | np_collect %.1f\n", 1e-6 * p.sec[0], 1e-6 * p.sec[1], 1e-6 * p.sec[2],
                1e-6 * p.sec[3], 1e-6 * p.sec[4], 1e-6 * p.sec[5], 1e-6 * p.sec[6], (long long)p.sec[14].load(), 1e-6 * p.sec[7], 1e-6 * p.sec[8], 1e-6 * p.sec[9], 1e-6 * p.sec[10]);
        fprintf(stderr, "  ba_collect parts (total ms): window / landmark sweep %.1f | pairs %.1f | copies %.1f\n", 1e-6 * p.sec[11], 1e-6 * p.sec[12], 1e-6 * p.sec[13]);
        vslam::ba_host_profile_print();
        vslam_sys::keys_from_block_profile_print();
        fprintf(stderr, "  local-BA cohorts: %.1f us per cohort x %lld cohorts of %.1f lanes (above 15 ms: %lld, longest %.1f ms)\n",
                avg(p.mqNs, p.mqN), p.mqN.load(), p.mqN.load() ? (double)p.mqLate.load() / (double)p.mqN.load() : 0.0, p.mapLate.load(), 1e-6 * (double)p.mapMaxNs.load());
    }
    // sessions first (each waits for its mapping job), then the mapping threads, then the shared objects
    kick();
    for (vslam_system* s : sys) if (s) { s->release(); delete s; }
    sys.clear();
    eng.reset();                                   // (the last group of the device stops the engine's threads)
    slabs.destroy();                               // (the sessions handed their key slabs back: everything the group allocated)
    if (stream) hipStreamSynchronize(stream);
    if (imuStream) { hipStreamSynchronize(imuStream); hipStreamDestroy(imuStream); imuStream = nullptr; }
    for (hipEvent_t e : {evTab, evImu0, evSolve0, evImu1}) if (e) hipEventDestroy(e);
    evTab = evImu0 = evSolve0 = evImu1 = nullptr;
    timer.destroy();
    if (fe) vslam_extractor_destroy(fe);
    fe = nullptr;
    hipFree(d_res); hipFree(d_tab); hipFree(d_up); hipFree(d_dn); hipFree(d_zero);
    if (h_res) hipHostFree(h_res);
    if (h_tab) hipHostFree(h_tab);
    if (h_up) hipHostFree(h_up);
    if (h_dn) hipHostFree(h_dn);
    if (stream) hipStreamDestroy(stream);
    stream = nullptr;
}

// The lanes' pending device requests of a host phase (descriptor selection after a keyframe insertion / new points / a local BA's
// write-back; the write-back's depth refresh), served together: ONE launch + one synchronisation per kind instead of one round
// trip per lane on the pool threads.
vslam_status vslam_batch::serve_requests() {
    // ---- gather: MapPoint::calcDescriptor ------------------------------------------------------------------------------------
    size_t nMp = 0, nDesc = 0;
    for (vslam_system* s : sys) if (s->descReq.pending) { nMp += s->descReq.mps.size(); nDesc += s->descReq.descs.size() / 32; }
    if (nMp) {
        rqDescs.resize(nDesc * 32); rqStart.assign(1, 0); rqBest.assign(nMp, -1);
        size_t at = 0;
        for (vslam_system* s : sys) {
            DescReq& q = s->descReq;
            if (!q.pending) continue;
            if (!q.descs.empty()) memcpy(rqDescs.data() + at * 32, q.descs.data(), q.descs.size());
            for (size_t i = 0; i < q.mps.size(); i++) rqStart.push_back((int)at + q.start[i + 1]);
            at += q.descs.size() / 32;
        }
    }
    // ---- gather: MapPoint::updatePos depth / close refresh ----------------------------------------------------------------------
    size_t nPair = 0; int nKf = 0, nLm = 0;
    for (vslam_system* s : sys) if (s->refReq.pending) { nPair += s->refReq.rk.size(); nKf += s->refReq.nKf; nLm += s->refReq.nLm; }
    std::vector<int> rk, rl; std::vector<float> cur, dep, kfTh; std::vector<double> pose, lm;
    std::vector<uint8_t> zeroW, zeroO, clo, up;
    if (nPair) {
        cur.resize(nPair); dep.resize(nPair); pose.resize((size_t)nKf * 16); lm.resize((size_t)nLm * 3);
        zeroW.assign(nPair, 0); zeroO.assign(std::max(nLm, 1), 0); clo.resize(nPair); up.resize(nPair);
        rk.reserve(nPair); rl.reserve(nPair);
        size_t ap = 0; int ak = 0, al = 0;
        for (vslam_system* s : sys) {
            RefreshReq& r = s->refReq;
            if (!r.pending) continue;
            for (size_t i = 0; i < r.rk.size(); i++) { rk.push_back(r.rk[i] + ak); rl.push_back(r.rl[i] + al); cur[ap + i] = r.cur[i]; }
            memcpy(pose.data() + (size_t)ak * 16, r.rpose.data(), (size_t)r.nKf * 16 * sizeof(double));
            kfTh.insert(kfTh.end(), (size_t)r.nKf, vslam::refresh_close_th(s->cfg.rig));      // (the lane's own camera: close = depth <= 40 x ITS baseline)
            memcpy(lm.data() + (size_t)al * 3, r.rlm.data(), (size_t)r.nLm * 3 * sizeof(double));
            ap += r.rk.size(); ak += r.nKf; al += r.nLm;
        }
    }
    // ---- device: both kinds enqueued on this thread's (high-priority) pool stream, ONE wait - each used to be a round trip of its
    //      own that queued behind the groups' wide kernels.  No staging room yet (the arena grows at the sync): the synchronous calls.
    const bool wantDesc = nMp && nDesc, wantRef = nPair > 0;
    if (wantDesc || wantRef) {
        SysProfScope ps(sys_prof().descNs, sys_prof().descN);
        const int* bestP = nullptr;
        vslam::RefreshTicket tk{};
        vslam_status sd = wantDesc ? vslam::calc_descriptors_enqueue(rqDescs.data(), rqStart.data(), (int)nMp, device, &bestP) : VSLAM_OK;
        vslam_status sr = VSLAM_OK;
        if (wantRef && (sd == VSLAM_OK || sd == VSLAM_ERR_CAPACITY))
            sr = vslam::refresh_depth_enqueue(kfTh.data(), nKf, pose.data(), nLm, lm.data(), zeroO.data(), (int)nPair, rk.data(), rl.data(), zeroW.data(),
                                              cur.data(), device, &tk);
        if (sd != VSLAM_OK && sd != VSLAM_ERR_CAPACITY) return sd;
        if (sr != VSLAM_OK && sr != VSLAM_ERR_CAPACITY) return sr;
        vslam::DevPool* pool = vslam::thread_pool(device);
        if (!pool) return VSLAM_ERR_HIP;
        VS_HIP(hipStreamSynchronize(pool->stream));
        if (wantDesc && sd == VSLAM_OK) memcpy(rqBest.data(), bestP, nMp * sizeof(int));
        if (wantRef && sr == VSLAM_OK) { memcpy(dep.data(), tk.dep, nPair * sizeof(float)); memcpy(clo.data(), tk.clo, nPair); memcpy(up.data(), tk.up, nPair); }
        VS_HIP(pool->sync());          // (recycles the arena; may re-allocate it - after the copies)
        if (wantDesc && sd == VSLAM_ERR_CAPACITY) VS_CHECK(vslam_calc_descriptors(rqDescs.data(), rqStart.data(), (int)nMp, device, rqBest.data()));
        if (wantRef && sr == VSLAM_ERR_CAPACITY)
            VS_CHECK(vslam::refresh_depth_sync(kfTh.data(), 0.f, nKf, pose.data(), nLm, lm.data(), zeroO.data(), (int)nPair, rk.data(), rl.data(), zeroW.data(),
                                               cur.data(), device, dep.data(), clo.data(), up.data()));
    }
    // ---- scatter ----------------------------------------------------------------------------------------------------------------
    if (nMp) {
        size_t m = 0;
        for (vslam_system* s : sys) {
            DescReq& q = s->descReq;
            if (!q.pending) continue;
            q.best.assign(rqBest.begin() + m, rqBest.begin() + m + q.mps.size());
            m += q.mps.size();
        }
    }
    if (nPair) {
        size_t ap = 0;
        for (vslam_system* s : sys) {
            RefreshReq& r = s->refReq;
            if (!r.pending) continue;
            const size_t n = r.rk.size();
            r.dep.assign(dep.begin() + ap, dep.begin() + ap + n); r.clo.assign(clo.begin() + ap, clo.begin() + ap + n); r.up.assign(up.begin() + ap, up.begin() + ap + n);
            ap += n;
        }
    }
    return VSLAM_OK;
}

vslam_status vslam_batch::ensure_up(size_t bytes) {
    if (bytes <= upCap) return VSLAM_OK;
    VS_HIP(hipStreamSynchronize(stream));
    if (h_up) hipHostFree(h_up);
    hipFree(d_up);
    upCap = bytes + bytes / 2;
    VS_HIP(hipHostMalloc((void**)&h_up, upCap, hipHostMallocDefault));
    VS_HIP(hipMalloc((void**)&d_up, upCap));
    return VSLAM_OK;
}
vslam_status vslam_batch::ensure_dn(size_t bytes) {
    if (bytes <= dnCap) return VSLAM_OK;
    VS_HIP(hipStreamSynchronize(stream));
    if (h_dn) hipHostFree(h_dn);
    hipFree(d_dn);
    dnCap = bytes + bytes / 2;
    // (download block: written by the copy engine, READ by the host phases - keyframe key blocks of 200 KB each: cacheable host memory;
    //  the default coherent kind read at < 0.5 GB/s here)
    VS_HIP(hipHostMalloc((void**)&h_dn, dnCap, hipHostMallocNonCoherent));
    VS_HIP(hipMalloc((void**)&d_dn, dnCap));
    return VSLAM_OK;
}

#define LANE_TRY(expr)                                                                                  \
    do {                                                                                                \
        vslam_status s_ = (expr);                                                                       \
        if (s_ != VSLAM_OK) { q.st = s_; q.failed = true; snprintf(q.err, sizeof(q.err), "%s", vslam_last_error()); return; } \
    } while (0)

// level 0 of every active lane's pair + the whole extraction, on the extractor's stream
vslam_status vslam_batch::enqueue_extraction(const uint8_t* const* L, const uint8_t* const* R, const uint8_t* mask, int stride, int channels,
                                             bool onDevice, bool raw) {
    if (raw) {                  // unrectified frames: every active lane's pair through its own cameras' maps, one launch
        imgPtrs.assign((size_t)2 * B, nullptr); rectPtrs.assign((size_t)2 * B, nullptr);
        for (int b = 0; b < B; b++) if (!mask || mask[b]) {
            imgPtrs[2 * b] = L[b]; imgPtrs[2 * b + 1] = R[b];
            rectPtrs[2 * b] = sys[b]->rectL; rectPtrs[2 * b + 1] = sys[b]->rectR;
        }
        VS_CHECK(fe->set_images_raw(imgPtrs.data(), rectPtrs.data(), stride, channels, onDevice, true));
    } else if (channels != 1) {        // colour frames: every active lane's pair converted by one launch (host: uploads, one wait, one launch)
        imgPtrs.assign((size_t)2 * B, nullptr);
        for (int b = 0; b < B; b++) if (!mask || mask[b]) { imgPtrs[2 * b] = L[b]; imgPtrs[2 * b + 1] = R[b]; }
        VS_CHECK(fe->set_images_color(imgPtrs.data(), stride, channels, onDevice, true));
    } else if (onDevice) {
        imgPtrs.assign((size_t)2 * B, nullptr);
        for (int b = 0; b < B; b++) if (!mask || mask[b]) { imgPtrs[2 * b] = L[b]; imgPtrs[2 * b + 1] = R[b]; }
        VS_CHECK(fe->set_images_device(imgPtrs.data(), stride));
    } else {
        for (int b = 0; b < B; b++) {
            if (mask && !mask[b]) continue;
            VS_CHECK(fe->set_image_async(2 * b, L[b], stride, false));
            VS_CHECK(fe->set_image_async(2 * b + 1, R[b], stride, false));
        }
        VS_HIP(hipStreamSynchronize(fe->stream));      // callers may reuse their buffers
    }
    return fe->run();
}

vslam_status vslam_batch::first_error() {
    for (int b = 0; b < B; b++) if (ls[b].failed) { set_error("lane %d: %s", b, ls[b].err); return ls[b].st; }
    return VSLAM_OK;
}

// The host begin phase of the lanes that are on in ls[]: mapping results due at the lanes' frame numbers land (frame_begin_a, the
// group's request service, frame_begin_b1, the merged changePosesLCA pass, frame_begin_b2).  candidates: the tracker's candidate
// lists as well (a tracked step; a relocalisation gathers its own).
vslam_status vslam_batch::host_begin(const int* frames, const vslam_imu_bucket* imu, bool candidates, bool needImu) {
    using clk = std::chrono::steady_clock;
    auto sub = [&](int k, clk::time_point& ts) { const auto t1 = clk::now(); subSum[k] += std::chrono::duration<double>(t1 - ts).count(); ts = t1; };

    auto ts = clk::now();
    pool.run(B, [&](int b) {
        LaneStep& q = ls[b];
        if (!q.on) return;
        hipSetDevice(device);
        vslam_system* s = sys[b];
        s->deferDevice = true;
        const vslam_status bs = s->frame_begin_a(s->ctx, frames[b], imu ? &imu[b] : nullptr, needImu);
        s->deferDevice = false;
        LANE_TRY(bs);
    });
    VS_CHECK(first_error());
    sub(0, ts);
    VS_CHECK(serve_requests());                    // descriptor selection / depth refresh of every lane that committed a job
    sub(1, ts);
    pool.run(B, [&](int b) {
        LaneStep& q = ls[b];
        if (!q.on) return;
        hipSetDevice(device);
        vslam_system* s = sys[b];
        s->deferLca = true;
        const vslam_status bs = s->frame_begin_b1(s->ctx);
        s->deferLca = false;
        LANE_TRY(bs);
        if (candidates && !s->lcaReq.pending && !q.first) q.N = s->frame_candidates(s->ctx);
    });
    VS_CHECK(first_error());
    // changePosesLCA of the lanes whose local BA landed at this step: their KeyFrame::updatePose kernels enqueued back to back on this
    // thread's stream, ONE wait (each used to be a synchronous round trip of its own on a pool thread)
    {
        std::vector<int> lanesL;
        for (int b = 0; b < B; b++) if (ls[b].on && sys[b]->lcaReq.pending) lanesL.push_back(b);
        if (!lanesL.empty()) {
            std::vector<vslam::KfUpdTicket> tk(lanesL.size());
            std::vector<vslam_status> st(lanesL.size(), VSLAM_OK);
            for (size_t i = 0; i < lanesL.size(); i++) st[i] = vslam::kf_update_pose_enqueue(&sys[lanesL[i]]->lcaReq.P, device, &tk[i]);
            vslam::DevPool* dp = vslam::thread_pool(device);
            if (!dp) return VSLAM_ERR_HIP;
            VS_HIP(hipStreamSynchronize(dp->stream));
            for (size_t i = 0; i < lanesL.size(); i++) {
                if (st[i] != VSLAM_OK) continue;
                vslam_system::LcaReq& r = sys[lanesL[i]]->lcaReq;
                if (tk[i].drop_l && r.P.n_left) memcpy(r.dl.data(), tk[i].drop_l, r.P.n_left);
                if (tk[i].drop_r && r.P.n_right) memcpy(r.dr.data(), tk[i].drop_r, r.P.n_right);
                if (tk[i].lm_xyz && r.P.n_lm) memcpy(r.xyz.data(), tk[i].lm_xyz, (size_t)3 * r.P.n_lm * sizeof(double));
            }
            VS_HIP(dp->sync());          // (recycles the arena - after the copies)
            for (size_t i = 0; i < lanesL.size(); i++) {
                if (st[i] == VSLAM_OK) continue;
                if (st[i] != VSLAM_ERR_CAPACITY) return st[i];
                vslam_system::LcaReq& r = sys[lanesL[i]]->lcaReq;      // no staging room yet: the synchronous entry point
                double poseOut[16];
                VS_CHECK(vslam_keyframe_update_pose(&r.P, device, r.dl.data(), r.dr.data(), poseOut));
            }
            pool.run((int)lanesL.size(), [&](int i) {
                const int b = lanesL[i];
                LaneStep& q = ls[b];
                vslam_system* s = sys[b];
                LANE_TRY(s->frame_begin_b2(s->ctx));
                if (candidates && !q.first) q.N = s->frame_candidates(s->ctx);
            });
            VS_CHECK(first_error());
        }
    }
    sub(2, ts);
    return VSLAM_OK;
}

vslam_status vslam_batch::step(const uint8_t* const* L, const uint8_t* const* R, int stride, int channels, bool onDevice, const int* frames,
                               const vslam_imu_bucket* imu, const uint8_t* mask, double* T_wc_out, vslam_frame_report* reps,
                               const uint8_t* const* nextL, const uint8_t* const* nextR, const uint8_t* nextMask, bool raw) {
    if (!L || !R || !frames || !T_wc_out) return VSLAM_ERR_INVALID;
    VS_HIP(hipSetDevice(device));
    vslam::thread_pool_wants_priority() = true;      // this thread's pool serves the group's requests (serve_requests)
    using clk = std::chrono::steady_clock;
    auto t0 = clk::now();
    auto lap = [&](int k) { const auto t1 = clk::now(); phase[k] = std::chrono::duration<double>(t1 - t0).count(); phaseSum[k] += phase[k]; t0 = t1; };
    auto sub = [&](int k, clk::time_point& ts) { const auto t1 = clk::now(); subSum[k] += std::chrono::duration<double>(t1 - ts).count(); ts = t1; };
    nSteps++;
    int nOn = 0;
    for (int b = 0; b < B; b++) {
        LaneStep& q = ls[b];
        q = LaneStep{};
        q.on = !mask || mask[b];
        if (!q.on) continue;
        if (!L[b] || !R[b]) { set_error("vslam_batch: lane %d has no images", b); return VSLAM_ERR_INVALID; }
        q.first = frames[b] == 0;
        if (sys[b]->relocPending) { set_error("vslam_batch: lane %d: %s", b, kRelocPendingMsg); return VSLAM_ERR_INVALID; }
        if (needFirst[b] && !q.first) { set_error("vslam_batch: lane %d was restarted, its next frame must carry frame number 0 (got %d)", b, frames[b]); return VSLAM_ERR_INVALID; }
        nOn++;
    }
    if (!nOn) return VSLAM_OK;
    VS_CHECK(host_begin(frames, imu, true));
    lap(0);

    // ---- device: images, extraction (already in flight when the previous step prefetched exactly these images) -----------
    {
        bool hit = onDevice && prefetched.size() == (size_t)2 * B && prefetchedChannels == channels && prefetchedRaw == raw;
        for (int b = 0; b < B && hit; b++) {
            const bool on = ls[b].on;
            hit = prefetched[2 * b] == (on ? L[b] : nullptr) && prefetched[2 * b + 1] == (on ? R[b] : nullptr);
        }
        prefetched.clear();
        if (!hit) {
            if (fe->countsPending) VS_CHECK(fe->wait_counts());      // (a prefetch for other images: let it finish first)
            VS_CHECK(enqueue_extraction(L, R, mask, stride, channels, onDevice, raw));
        }
    }
    lap(1);

    // ---- host, under the extraction: the upload block -----------------------------------------------------------------------
    size_t upBytes = 0;
    for (int b = 0; b < B; b++) {
        LaneStep& q = ls[b];
        if (!q.on || q.first) continue;
        q.upOff = upBytes;
        const int n = std::max(q.N, 1);
        upBytes += up256((size_t)n * 24) + up256((size_t)n * 32) + up256((size_t)n * 4);
        if (useImu) upBytes += up256((size_t)(7 * std::max(imu ? imu[b].n : 0, 0) + 6) * sizeof(double));
    }
    VS_CHECK(ensure_up(std::max<size_t>(upBytes, 256)));
    {
        size_t zneed = 0;
        for (int b = 0; b < B; b++) zneed = std::max(zneed, (size_t)ls[b].N);
        if (zneed > zeroCap) {
            VS_HIP(hipStreamSynchronize(stream));
            hipFree(d_zero);
            zeroCap = up256(zneed + zneed / 2 + 1024);
            VS_HIP(hipMalloc((void**)&d_zero, zeroCap));
            VS_HIP(vslam::memset_sync(d_zero, 0, zeroCap));
        }
    }
    pool.run(B, [&](int b) {
        LaneStep& q = ls[b];
        if (!q.on || q.first) return;
        vslam_system* s = sys[b];
        vslam_matcher* m = s->fm;
        const int n = std::max(q.N, 1);
        uint8_t* h = h_up + q.upOff;
        uint8_t* d = d_up + q.upOff;
        const size_t oDesc = up256((size_t)n * 24), oMsd = oDesc + up256((size_t)n * 32), oImu = oMsd + up256((size_t)n * 4);
        s->frame_fill_upload(s->ctx, (double*)h, h + oDesc, (float*)(h + oMsd));
        m->track_bind_map((double*)d, d + oDesc, (float*)(d + oMsd), d_zero, q.N);
        if (useImu) {
            s->frame_imu_input(s->ctx);
            LANE_TRY(m->imu_stage(&s->ctx.in, 0.0, (double*)(h + oImu), (double*)(d + oImu), ht.imu0[b]));
        }
    });
    VS_CHECK(first_error());
    if (upBytes) VS_HIP(hipMemcpyAsync(d_up, h_up, upBytes, hipMemcpyHostToDevice, stream));
    lap(2);

    // ---- keys of the new frames (waits for the extraction's totals) -----------------------------------------------------------
    VS_HIP(hipStreamWaitEvent(stream, fe->evDone, 0));
    {
        const auto w0 = clk::now();
        VS_CHECK(fe->wait_counts());
        phaseSum[7] += std::chrono::duration<double>(clk::now() - w0).count();      // (part of phase 3: the extraction still running)
    }
    int maxL = 0, maxR = 0, maxN = 0, nTrack = 0, ldsFactors = 0;
    size_t dnBytes = 0;
    for (int b = 0; b < B; b++) {
        LaneStep& q = ls[b];
        if (!q.on) continue;
        vslam_matcher* m = sys[b]->fm;
        VS_CHECK(m->refresh_keys(false));
        q.nL = m->nKeys[0]; q.nR = m->nKeys[1];
        maxL = std::max(maxL, q.nL); maxR = std::max(maxR, q.nR);
        if (q.first) continue;
        nTrack++;
        maxN = std::max(maxN, std::max(q.N, 1));
        q.dnOff = dnBytes;
        dnBytes += up256((size_t)std::max(q.N, 1) * 15 + (size_t)q.nL * 4 + 16);
        // a lane whose keyframe counter allows an insertion this frame (src/FeatureTracker.cpp:1262: count >= 5) gets its
        // TrackedKeys in the same download; the rarer nStereo < 80 branch falls back to fetch_keys()
        // (its nStereo < 80 branch can insert at any frame: a lane whose previous frame was near that bound gets them too;
        //  a keyframe that still arrives without its block falls back to fetch_keys())
        q.wantKeys = sys[b]->insertKeyFrameCount + 1 >= 5 || sys[b]->lastNStereo < 110;
        if (q.wantKeys) { q.keyOff = dnBytes; dnBytes += up256(key_block_layout(q.nL, q.nR).total); }
    }
    VS_CHECK(ensure_dn(std::max<size_t>(dnBytes, 256)));

    // ---- per-lane argument tables (each lane fills its own entries: on the host-phase pool) ---------------------------------
    std::vector<int> laneLds((size_t)B, 0);
    pool.run(B, [&](int b) {
        LaneStep& q = ls[b];
        StereoLane& S = ht.stereo[b];
        if (!q.on) { S.A.nL = 0; S.A.nR = 0; }
        else LANE_TRY(sys[b]->fm->stereo_lane(S));
        if (q.on) sys[b]->fm->stereoDone = true;
        const bool tr = q.on && !q.first;
        vslam_matcher* m = sys[b]->fm;
        if (!tr) {
            // idle lanes: every kernel's lane test fails on these entries (count 0 / gate closed)
            ht.predict[b] = PredictLane{};
            ht.predict[b].count = m->d_trCount; ht.predict[b].poseIO = m->d_poseIO + 24;      // (scratch slot of the result block)
            ht.predict[b].setCount = 1;
            ht.imu0[b].n = 0; ht.imu1[b].n = 0;
            ht.proj0[b].A = ProjArgs{}; ht.proj1[b].A = ProjArgs{};
            ht.proj0[b].A.gate = ht.proj1[b].A.gate = m->d_trCount + 2; ht.proj0[b].A.gateMin = ht.proj1[b].A.gateMin = 1;     // (an int that stays 0)
            ht.pose0[b].A = PoseArgs{}; ht.pose1[b].A = PoseArgs{};
            ht.pose0[b].A.gate = ht.pose1[b].A.gate = m->d_trCount + 2; ht.pose0[b].A.gateMin = ht.pose1[b].A.gateMin = 1;
            ht.repredict[b] = RepredictLane{};
            ht.pack[b] = PackLane{};
            ht.pack[b].count = m->d_trCount;
            return;
        }
        vslam_system* s = sys[b];
        hipSetDevice(device);
        LANE_TRY(m->track_begin(s->predNPose.data(), frames[b], useImu));
        const int Nub = std::max(m->trNub, 1);
        const int* Mdev = m->d_trCount + 1;
        const int* gate = m->d_poseOut;          // inlier count of the first round
        const int minIn = vslam_matcher::TRACK_MIN_INLIERS;
        m->predict_lane(ht.predict[b], 0);
        ht.predict[b].setCount = 1;
        m->proj_lane(ht.proj0[b], Nub, m->trRad, Mdev, nullptr, 0, PROJ_STEREO);
        m->proj_lane(ht.proj1[b], Nub, 4.f, Mdev, gate, minIn, PROJ_STEREO);
        m->repredict_lane(ht.repredict[b], gate, minIn);
        if (useImu) {
            m->pose_imu_lane(ht.pose0[b], Nub, Mdev, nullptr, minIn, 0, 0);
            m->pose_imu_lane(ht.pose1[b], Nub, Mdev, gate, minIn, 1, 0);
            m->imu_lane(ht.imu1[b], true);
            laneLds[b] = std::max(ht.pose0[b].I.ldsFactors, ht.pose1[b].I.ldsFactors);
        } else {
            m->pose_lane(ht.pose0[b].A, Nub, Mdev, nullptr, minIn, 0, 0);
            m->pose_lane(ht.pose1[b].A, Nub, Mdev, gate, minIn, 1, 0);
        }
        PackLane& K = ht.pack[b];
        K.N = q.N; K.nL = q.nL; K.count = m->d_trCount; K.matches = m->d_matches; K.act = m->d_trAct; K.matchedL = m->d_matchedL;
        K.flags = m->d_flags; K.flagStride = (size_t)m->poseCap; K.visLeft = m->d_trVisL; K.out = d_dn + q.dnOff;
        K.keyOut = q.wantKeys ? d_dn + q.keyOff : nullptr; K.nR = q.nR;
        q.keySlot = (q.wantKeys && s->cfg.local_mapping) ? s->reserve_key_slot(q.nL, q.nR) : nullptr;
        K.keyOut2 = (uint8_t*)q.keySlot;
        K.kps[0] = m->d_kps[0]; K.kps[1] = m->d_kps[1]; K.desc[0] = m->d_desc[0]; K.desc[1] = m->d_desc[1];
        K.rightIdxs = m->d_rightIdxs; K.leftIdxs = m->d_leftIdxs; K.depth = m->d_depth; K.closef = m->d_close;
    });
    VS_CHECK(first_error());
    for (int b = 0; b < B; b++) ldsFactors = std::max(ldsFactors, laneLds[b]);
    VS_HIP(hipMemcpyAsync(d_tab, h_tab, tabBytes, hipMemcpyHostToDevice, stream));

    // ---- device: every stage once for all lanes --------------------------------------------------------------------------------
    int t;
    launch_stereo_batch(stream, dt.stereo, B, maxL, maxR, shared.rig.height, &timer);      // (image height: shared; the lanes' fx / baseline are in their StereoLane)
    // (stage timing brackets launches with events on the main stream: keep the pre-integrations there when it is on)
    static const bool sideEnv = getenv("VSLAM_BATCH_IMU_SIDE") ? atoi(getenv("VSLAM_BATCH_IMU_SIDE")) != 0 : true;
    const bool side = useImu && !timer.enabled && sideEnv;
    if (nTrack) {
        if (side) {
            VS_HIP(hipEventRecord(evTab, stream));                 // tables + upload block are on the device
            VS_HIP(hipStreamWaitEvent(imuStream, evTab, 0));
            launch_imu_batch(imuStream, dt.imu0, B);
            VS_HIP(hipEventRecord(evImu0, imuStream));
        }
        t = timer.begin("track_predict"); launch_track_predict_batch(stream, dt.predict, B); timer.end(t);
        if (useImu && !side) { t = timer.begin("imu_preintegrate"); launch_imu_batch(stream, dt.imu0, B); timer.end(t); }
        launch_proj_batch(stream, dt.proj0, B, maxN, maxL, maxR, &timer);
        if (side) VS_HIP(hipStreamWaitEvent(stream, evImu0, 0));
        t = timer.begin(useImu ? "pose_imu_lm" : "pose_lm");
        if (useImu) launch_pose_imu_batch(stream, dt.pose0, B, ldsFactors); else launch_pose_batch(stream, dt.pose0, B);
        timer.end(t);
        if (side) {
            VS_HIP(hipEventRecord(evSolve0, stream));
            VS_HIP(hipStreamWaitEvent(imuStream, evSolve0, 0));
            launch_imu_batch(imuStream, dt.imu1, B);
            VS_HIP(hipEventRecord(evImu1, imuStream));
        } else if (useImu) { t = timer.begin("imu_preintegrate"); launch_imu_batch(stream, dt.imu1, B); timer.end(t); }
        t = timer.begin("track_repredict"); launch_track_repredict_batch(stream, dt.repredict, B, maxN); timer.end(t);
        launch_proj_batch(stream, dt.proj1, B, maxN, maxL, maxR, &timer, false);
        if (side) VS_HIP(hipStreamWaitEvent(stream, evImu1, 0));
        t = timer.begin(useImu ? "pose_imu_lm" : "pose_lm");
        if (useImu) launch_pose_imu_batch(stream, dt.pose1, B, ldsFactors); else launch_pose_batch(stream, dt.pose1, B);
        timer.end(t);
        t = timer.begin("pack"); launch_track_pack_batch(stream, dt.pack, B, maxN); timer.end(t);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(h_res, d_res, (size_t)B * 64 * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (dnBytes) VS_HIP(hipMemcpyAsync(h_dn, d_dn, dnBytes, hipMemcpyDeviceToHost, stream));
    }
    VS_HIP(hipGetLastError());
    lap(3);
    // ---- host, under the step's kernels: the local BAs' window collection + hand-over (reads the map as frame_begin left it) ----
    pool.run(B, [&](int b) {
        LaneStep& q = ls[b];
        if (!q.on || !sys[b]->pass.collectDue) return;
        hipSetDevice(device);
        LANE_TRY(sys[b]->frame_mid());
    });
    kick();                                        // the local BAs handed over: one cohort
    VS_CHECK(first_error());
    VS_HIP(hipStreamSynchronize(stream));
    lap(4);
    // ---- prefetch: the next frames' extraction runs under this step's host phases and the next step's begin ----------------
    // (the extractor alternates between two output sets, so this frame's keys stay readable for keyframe insertion)
    if (nextL && nextR && onDevice) {
        VS_CHECK(enqueue_extraction(nextL, nextR, nextMask, stride, channels, true, raw));
        prefetched.assign((size_t)2 * B, nullptr); prefetchedChannels = channels; prefetchedRaw = raw;
        for (int b = 0; b < B; b++) if (!nextMask || nextMask[b]) { prefetched[2 * b] = nextL[b]; prefetched[2 * b + 1] = nextR[b]; }
    }

    // ---- host: the reference's retry rule per lane (launches only for lanes whose first round failed) ------------------------
    std::vector<SysTrackState> st(B);
    for (int b = 0; b < B; b++) {
        LaneStep& q = ls[b];
        if (!q.on || q.first) continue;
        vslam_system* s = sys[b];
        vslam_matcher* m = s->fm;
        SysFrameCtx& c = s->ctx;
        VS_CHECK(m->track_finish(c.T_cw, &c.tr, useImu ? &c.imuOut : nullptr));
        const int M = c.tr.n_active, N = q.N, nL = q.nL;
        uint8_t* p = h_dn + q.dnOff;
        SysTrackState& v = st[b];
        if (!m->trRetried) {
            v.matches = (const int*)p; v.actIdx = v.matches + 2 * (size_t)N; v.matchedL = v.actIdx + N;
            v.outl = (const uint8_t*)(v.matchedL + nL); v.inF = v.outl + N; v.visL = v.inF + N;
        } else {
            // the slice is large enough for the one-session layout (M <= N)
            VS_CHECK(m->track_fetch_state(p, M, nL, N));
            v.matches = (const int*)p; p += (size_t)M * 8;
            v.actIdx = (const int*)p; p += (size_t)M * 4;
            v.matchedL = (const int*)p; p += (size_t)nL * 4;
            v.outl = p; p += M;
            v.inF = p; p += M;
            v.visL = p;
        }
        v.nL = nL;
        v.keys = (q.wantKeys && !m->trRetried) ? h_dn + q.keyOff : nullptr; v.nR = q.nR;      // (retry rounds ran after the pack)
        v.keySlot = v.keys ? q.keySlot : nullptr;
    }
    lap(5);

    // ---- host: frame_post (first frames: the one-session path on their own stereo result) ------------------------------------
    auto ts = clk::now();
    pool.run(B, [&](int b) {
        LaneStep& q = ls[b];
        if (!q.on) return;
        hipSetDevice(device);
        vslam_system* s = sys[b];
        if (q.first) LANE_TRY(s->frame_first(s->ctx, T_wc_out + 16 * (size_t)b, reps ? &reps[b] : nullptr));
        else {
            s->deferDevice = true;
            const vslam_status ps = s->frame_post_a(s->ctx, st[b]);
            s->deferDevice = false;
            LANE_TRY(ps);
        }
    });
    VS_CHECK(first_error());
    sub(3, ts);
    VS_CHECK(serve_requests());                    // descriptor selection of the lanes that inserted a keyframe
    sub(4, ts);
    pool.run(B, [&](int b) {
        LaneStep& q = ls[b];
        if (!q.on || q.first) return;
        hipSetDevice(device);
        LANE_TRY(sys[b]->frame_post_b(sys[b]->ctx, T_wc_out + 16 * (size_t)b, reps ? &reps[b] : nullptr));
    });
    kick();                                        // the new-point searches of the lanes that inserted a keyframe
    VS_CHECK(first_error());
    for (int b = 0; b < B; b++) if (ls[b].on) needFirst[b] = 0;      // (a restarted lane's frame 0 has been tracked)
    sub(5, ts);
    lap(6);
    return VSLAM_OK;
}

// Relocalisation of the masked lanes from their own maps, in lockstep: per lane what vslam_system::relocalize does, with one extraction
// enqueue, one stereo launch set and one launch per relocalisation stage for all of them (reloc.hip: reloc_batch_run), the map points
// gathered straight into the group's upload block.  One wait for the extraction's counts (as a step has), one at the end.
vslam_status vslam_batch::relocalize(const uint8_t* const* L, const uint8_t* const* R, int stride, bool onDevice, const int* frames,
                                     const uint8_t* mask, const vslam_reloc_params* prm, double* T_wc_out, vslam_reloc_report* reps, bool imuCall,
                                     const vslam_imu_bucket* imu, vslam_reloc_imu_report* ireps) {
    const char* const fn = imuCall ? "vslam_batch_relocalize_imu" : "vslam_batch_relocalize";
    if (!L || !R || !frames || !T_wc_out || !reps || (imuCall && !ireps)) { set_error("%s: invalid arguments", fn); return VSLAM_ERR_INVALID; }
    // ---- refusals: nothing has changed when one of these returns ----------------------------------------------------------------
    int nOn = 0;
    for (int b = 0; b < B; b++) {
        if (mask && !mask[b]) continue;
        nOn++;
        if (useImu && !imuCall) { set_error("vslam_batch_relocalize: lane %d: an IMU batch cannot relocalise yet (its velocity would need re-initialising)", b); return VSLAM_ERR_INVALID; }
        if (!useImu && imuCall) { set_error("vslam_batch_relocalize_imu: lane %d: a batch without IMU relocalises through vslam_batch_relocalize", b); return VSLAM_ERR_INVALID; }
        if (!L[b] || !R[b]) { set_error("%s: lane %d has no images", fn, b); return VSLAM_ERR_INVALID; }
        if (needFirst[b] || sys[b]->keyFrames.empty()) { set_error("%s: lane %d has no map (track its frame 0 first)", fn, b); return VSLAM_ERR_INVALID; }
        if (imuCall) VS_CHECK(sys[b]->reloc_imu_check(imu ? &imu[b] : nullptr, fn, b));      // (a lane between its two poses needs its bucket)
    }
    vslam_reloc_params P;
    VS_CHECK(reloc_resolve_params(prm, P));
    if (!nOn) return VSLAM_OK;
    VS_HIP(hipSetDevice(device));
    vslam::thread_pool_wants_priority() = true;
    for (int b = 0; b < B; b++) { ls[b] = LaneStep{}; ls[b].on = !mask || mask[b]; }
    // ---- host: mapping results due at these frame numbers land as in a tracked step ------------------------------------------------
    VS_CHECK(host_begin(frames, nullptr, false, false));
    // ---- device: the frames' extraction; a prefetched one (for a tracked step's images) finishes first and is discarded ---------
    prefetched.clear();
    if (fe->countsPending) VS_CHECK(fe->wait_counts());
    VS_CHECK(enqueue_extraction(L, R, mask, stride, 1, onDevice, false));
    // ---- host, under the extraction: the local BAs' window collection, the candidate lists, the upload block --------------------
    std::vector<RelocBatchLane> rl((size_t)B);
    pool.run(B, [&](int b) {
        LaneStep& q = ls[b];
        if (!q.on) return;
        hipSetDevice(device);
        if (sys[b]->pass.collectDue) LANE_TRY(sys[b]->frame_mid());
        rl[b].m = sys[b]->fm; rl[b].n = sys[b]->reloc_candidates(); rl[b].wantInFrame = true;
        if (imuCall && sys[b]->relocPending) {               // second pose: the bucket since the first, x0 = the camera pose, b0 = biasGood
            sys[b]->reloc_imu_input(sys[b]->ctx, &imu[b]);
            rl[b].imu = &sys[b]->ctx.in;
        }
    });
    kick();
    VS_CHECK(first_error());
    RelocBatchPlan plan;
    reloc_batch_plan(rl.data(), B, plan);
    VS_CHECK(ensure_up(plan.upBytes));
    VS_CHECK(ensure_dn(plan.dnBytes));
    pool.run(B, [&](int b) {
        if (!ls[b].on) return;
        sys[b]->reloc_fill_upload((double*)(h_up + rl[b].oXyz), h_up + rl[b].oDesc, (float*)(h_up + rl[b].oMsd));
    });
    // ---- keys of the new frames (waits for the extraction's totals), stereo match of the masked pairs -----------------------------
    VS_HIP(hipStreamWaitEvent(stream, fe->evDone, 0));
    VS_CHECK(fe->wait_counts());
    int maxL = 0, maxR = 0;
    for (int b = 0; b < B; b++) {
        StereoLane& S = ht.stereo[b];
        if (!ls[b].on) { S.A.nL = 0; S.A.nR = 0; continue; }
        vslam_matcher* m = sys[b]->fm;
        VS_CHECK(m->refresh_keys(false));
        VS_CHECK(m->stereo_lane(S));
        m->stereoDone = true;
        maxL = std::max(maxL, m->nKeys[0]); maxR = std::max(maxR, m->nKeys[1]);
    }
    VS_HIP(hipMemcpyAsync(dt.stereo, ht.stereo, (size_t)B * sizeof(StereoLane), hipMemcpyHostToDevice, stream));
    launch_stereo_batch(stream, dt.stereo, B, maxL, maxR, shared.rig.height, &timer);
    VS_CHECK(reloc_batch_check(rl.data(), B, device));
    // ---- device: every relocalisation stage once for all lanes; one wait ----------------------------------------------------------
    std::vector<double> Tcw((size_t)B * 16, 0.0);
    const RelocBlocks blk{h_up, d_up, h_dn, d_dn};
    if (imuCall) for (int b = 0; b < B; b++) if (ls[b].on) ireps[b] = vslam_reloc_imu_report{};
    VS_CHECK(reloc_batch_run(rl.data(), B, plan, blk, stream, P, (double)(float)std::log((double)shared.fe.scale), &timer, Tcw.data(), reps,
                                 imuCall ? ireps : nullptr));
    // ---- host: commit per lane (a failure changes nothing in its session) ----------------------------------------------------------
    pool.run(B, [&](int b) {
        if (!ls[b].on) return;
        vslam_system* s = sys[b];
        double* out = T_wc_out + 16 * (size_t)b;
        if (imuCall) s->reloc_imu_finish(reps[b], ireps[b], Tcw.data() + 16 * (size_t)b, h_dn + rl[b].oInF, out);
        else if (reps[b].success) s->reloc_commit(Tcw.data() + 16 * (size_t)b, h_dn + rl[b].oInF, out);
        else memcpy(out, s->camPose.data(), sizeof(double) * 16);
    });
    return VSLAM_OK;
}

// Loop closing of the masked lanes, between two steps: per lane what vslam_system::close_loop / correct_loop does to a session, with the
// detection through the batched relocalisation stage (one launch per stage for all lanes that have candidates), ONE batched pose-graph
// solve and ONE move-points launch for all lanes that reach the solve.  A lane's outcome does not depend on the other lanes: a busy lane
// reports busy, a lane that finds nothing reports success = 0, both untouched.  Refusals come first and change nothing in any lane.
// ireps != null: the _imu calls for an IMU batch - the same stages with every lane's claim projected
// about its own gravity (loop_build_imu), ONE vslam_pose_graph_optimize_yaw_batch with each lane's axis, loop_hold_unmoved before
// the move of the points and loop_commit_imu after it.
vslam_status vslam_batch::loop(bool correct, const uint8_t* mask, const int32_t* kfLoop, const double* T_wc_corrected, const vslam_loop_params* prm,
                               vslam_loop_report* reps, vslam_loop_imu_report* ireps) {
    const bool imuCall = ireps != nullptr;
    const char* const fn = imuCall ? (correct ? "vslam_batch_correct_loop_imu" : "vslam_batch_close_loop_imu")
                                   : (correct ? "vslam_batch_correct_loop" : "vslam_batch_close_loop");
    if (!mask || !reps || (correct && (!kfLoop || !T_wc_corrected))) { set_error("%s: invalid arguments", fn); return VSLAM_ERR_INVALID; }
    if (useImu && !imuCall) { set_error("%s: an IMU batch cannot close loops yet (its velocity and gravity frame would have to follow)", fn); return VSLAM_ERR_INVALID; }
    if (!useImu && imuCall) { set_error("%s: the batch has no IMU (vslam_batch_close_loop / _correct_loop serve it)", fn); return VSLAM_ERR_INVALID; }
    vslam_loop_params P;
    vslam_reloc_params RP{};
    if (!resolve_loop_params(prm, P)) { set_error("%s: negative or non-finite parameter", fn); return VSLAM_ERR_INVALID; }
    if (!correct) VS_CHECK(reloc_resolve_params(&P.reloc, RP));
    char who[96];
    int nOn = 0;
    for (int b = 0; b < B; b++) {
        if (!mask[b]) continue;
        nOn++;
        snprintf(who, sizeof who, "%s: lane %d", fn, b);
        VS_CHECK(imuCall ? sys[b]->loop_check_imu(who) : sys[b]->loop_check(who));
        if (correct) VS_CHECK(sys[b]->loop_check_correct(who, kfLoop[b], T_wc_corrected + 16 * (size_t)b));
        else VS_CHECK(sys[b]->loop_check_close(who));
    }
    if (!correct && nOn && !prefetched.empty()) {
        set_error("%s: a prefetched extraction is in flight: the matchers no longer hold the tracked frames", fn);
        return VSLAM_ERR_INVALID;
    }
    if (!nOn) return VSLAM_OK;
    VS_HIP(hipSetDevice(device));
    struct Solve { int lane, kf; M4 T_corr; };
    std::vector<Solve> solve;
    std::vector<int> detect;
    std::vector<RelocBatchLane> rl((size_t)B);
    for (int b = 0; b < B; b++) {
        if (!mask[b]) continue;
        vslam_loop_report& r = reps[b];
        r = vslam_loop_report{};
        r.kf_loop = correct ? kfLoop[b] : -1;
        if (imuCall) sys[b]->loop_imu_report_init(&ireps[b]);
        if (sys[b]->loop_busy()) { r.busy = 1; continue; }
        if (correct) {
            r.success = 1;
            const M4 T_corr = m4_from(T_wc_corrected + 16 * (size_t)b);
            loop_drift(T_corr, sys[b]->camPoseInv, &r);
            solve.push_back({b, kfLoop[b], T_corr});
            continue;
        }
        const int n = sys[b]->loop_candidates(P.min_kf_gap);
        r.n_candidates = n;
        r.reloc.n_points = n;
        if (n < RP.min_inliers) continue;
        rl[b].m = sys[b]->fm; rl[b].n = n; rl[b].wantInFrame = true;      // (the in-frame bytes are not used: the upload carries maxScaleDist anyway)
        detect.push_back(b);
    }
    // ---- detection: the batched relocalisation stage over the candidates; nothing of it reaches the sessions ------------------------
    if (!detect.empty()) {
        RelocBatchPlan plan;
        reloc_batch_plan(rl.data(), B, plan);
        VS_CHECK(ensure_up(plan.upBytes));
        VS_CHECK(ensure_dn(plan.dnBytes));
        for (int b : detect) sys[b]->reloc_fill_upload((double*)(h_up + rl[b].oXyz), h_up + rl[b].oDesc, (float*)(h_up + rl[b].oMsd));
        VS_CHECK(reloc_batch_check(rl.data(), B, device));
        std::vector<double> Tcw((size_t)B * 16, 0.0);
        std::vector<vslam_reloc_report> rr((size_t)B);
        {
            // step D may clear stereo matches of the frames the matchers hold: each lane's four stereo arrays are saved here and restored
            // below, as close_loop does for one session
            DevPool* tp = thread_pool(device);
            if (!tp) { set_error("no device pool"); return VSLAM_ERR_HIP; }
            std::vector<size_t> off(detect.size() + 1, 0);
            for (size_t i = 0; i < detect.size(); i++) off[i + 1] = off[i] + up256((size_t)sys[detect[i]]->fm->cap * 16);
            PoolBuf<uint8_t> save(tp);
            VS_HIP(save.alloc(off.back()));
            for (size_t i = 0; i < detect.size(); i++) {
                vslam_matcher* m = sys[detect[i]]->fm;
                const size_t c = (size_t)m->cap;
                uint8_t* s = save.p + off[i];
                VS_HIP(hipMemcpyAsync(s, m->d_rightIdxs, c * 4, hipMemcpyDeviceToDevice, stream));
                VS_HIP(hipMemcpyAsync(s + c * 4, m->d_leftIdxs, c * 4, hipMemcpyDeviceToDevice, stream));
                VS_HIP(hipMemcpyAsync(s + c * 8, m->d_depth, c * 4, hipMemcpyDeviceToDevice, stream));
                VS_HIP(hipMemcpyAsync(s + c * 12, m->d_close, c, hipMemcpyDeviceToDevice, stream));
            }
            const RelocBlocks blk{h_up, d_up, h_dn, d_dn};
            const vslam_status st = reloc_batch_run(rl.data(), B, plan, blk, stream, RP, (double)(float)std::log((double)shared.fe.scale), &timer,
                                                    Tcw.data(), rr.data());
            for (size_t i = 0; i < detect.size(); i++) {
                vslam_matcher* m = sys[detect[i]]->fm;
                const size_t c = (size_t)m->cap;
                const uint8_t* s = save.p + off[i];
                VS_HIP(hipMemcpyAsync(m->d_rightIdxs, s, c * 4, hipMemcpyDeviceToDevice, stream));
                VS_HIP(hipMemcpyAsync(m->d_leftIdxs, s + c * 4, c * 4, hipMemcpyDeviceToDevice, stream));
                VS_HIP(hipMemcpyAsync(m->d_depth, s + c * 8, c * 4, hipMemcpyDeviceToDevice, stream));
                VS_HIP(hipMemcpyAsync(m->d_close, s + c * 12, c, hipMemcpyDeviceToDevice, stream));
            }
            VS_HIP(hipStreamSynchronize(stream));
            VS_CHECK(st);
        }
        for (int b : detect) {
            vslam_loop_report& r = reps[b];
            r.reloc = rr[b];
            if (!r.reloc.success) continue;
            vslam_matcher* m = sys[b]->fm;
            const int C = m->rlLast[3];
            std::vector<uint8_t> flags(std::max(C, 1), 0);
            VS_CHECK(m->relocalize_debug(nullptr, 0, nullptr, 0, nullptr, 0, flags.data(), C, nullptr));
            snprintf(who, sizeof who, "%s: lane %d", fn, b);
            int best = -1;
            VS_CHECK(sys[b]->loop_vote((const int*)(h_dn + rl[b].oPairs), (size_t)rl[b].n, flags.data(), C, who, &best));
            if (best < 0) continue;
            r.kf_loop = best;
            r.success = 1;
            const M4 T_corr = m4_rigid_inv(m4_from(Tcw.data() + 16 * (size_t)b));
            loop_drift(T_corr, sys[b]->camPoseInv, &r);
            if (!P.detect_only) solve.push_back({b, best, T_corr});
            else if (imuCall) loop_project_yaw(T_corr, sys[b]->camPose, sys[b]->camPoseInv, sys[b]->cfg.gravity, &ireps[b]);
        }
    }
    // ---- correction: every lane's graph, one solve, one move-points launch, the commits ---------------------------------------------
    if (!solve.empty()) {
        const int ns = (int)solve.size();
        std::vector<vslam_system::LoopGraph> G((size_t)ns);
        std::vector<vslam_pgo_graph> graphs((size_t)ns);
        std::vector<vslam_pgo_yaw_graph> ygraphs((size_t)(imuCall ? ns : 0));
        std::vector<vslam_pgo_report> pr((size_t)ns);
        std::vector<PgoMoveGraph> mv((size_t)ns);
        {
            std::vector<std::unique_lock<std::mutex>> locks;       // every lane's map stays as its graph saw it until its commit
            for (int i = 0; i < ns; i++) {
                vslam_system* s = sys[solve[i].lane];
                locks.emplace_back(s->mapMutex);
                if (imuCall) VS_CHECK(s->loop_build_imu(solve[i].kf, solve[i].T_corr, P, &reps[solve[i].lane], &ireps[solve[i].lane], G[i]));
                else VS_CHECK(s->loop_build(solve[i].kf, solve[i].T_corr, P, &reps[solve[i].lane], G[i]));
                graphs[i] = vslam_pgo_graph{G[i].poses.data(), G[i].fixed.data(), G[i].K, G[i].edges.data(), (int32_t)G[i].edges.size(), G[i].fresh.data()};
                mv[i] = PgoMoveGraph{G[i].xyz.data(), G[i].ref.data(), G[i].nMp, G[i].poses.data(), G[i].fresh.data(), G[i].K, G[i].moved.data()};
                if (imuCall) { ygraphs[i].graph = graphs[i]; for (int k = 0; k < 3; k++) ygraphs[i].axis[k] = s->cfg.gravity[k]; }
            }
            if (imuCall) {
                VS_CHECK(vslam_pose_graph_optimize_yaw_batch(ygraphs.data(), ns, &P.pgo, device, pr.data()));
                for (int i = 0; i < ns; i++) loop_hold_unmoved(G[i]);
            } else {
                VS_CHECK(vslam_pose_graph_optimize_batch(graphs.data(), ns, &P.pgo, device, pr.data()));
            }
            VS_CHECK(pgo_move_points_batch(mv.data(), ns, device));
            for (int i = 0; i < ns; i++) {
                reps[solve[i].lane].pgo = pr[i];
                if (imuCall) sys[solve[i].lane]->loop_commit_imu(G[i], &reps[solve[i].lane], &ireps[solve[i].lane]);
                else sys[solve[i].lane]->loop_commit(G[i], &reps[solve[i].lane]);
            }
        }
        for (int i = 0; i < ns; i++) VS_CHECK(sys[solve[i].lane]->loop_activate(&reps[solve[i].lane]));
    }
    for (int b = 0; b < B; b++) if (mask[b]) memcpy(reps[b].T_wc, sys[b]->camPose.data(), 16 * sizeof(double));
    return VSLAM_OK;
}

vslam_status vslam_batch::followup_check_args(const char* fn, const uint8_t* mask, const void* reps) const {
    if (!mask || !reps) { set_error("%s: invalid arguments", fn); return VSLAM_ERR_INVALID; }
    if (useImu) { set_error("%s: an IMU batch cannot close loops yet (its velocity and gravity frame would have to follow)", fn); return VSLAM_ERR_INVALID; }
    return VSLAM_OK;
}

vslam_status vslam_batch::followup_check_lanes(const char* fn, const uint8_t* mask, int* nOn) const {
    char who[96];
    *nOn = 0;
    for (int b = 0; b < B; b++) {
        if (!mask[b]) continue;
        (*nOn)++;
        snprintf(who, sizeof who, "%s: lane %d", fn, b);
        VS_CHECK(sys[b]->loop_check(who));
    }
    return VSLAM_OK;
}

// The duplicate map points of the masked lanes, between two steps: per lane what vslam_system::fuse_loop does to a session, with ONE
// vslam_fuse_search_batch call for all lanes that reach the search.  Every lane's map is locked from its sets to its commit.  Refusals
// come first and change nothing in any lane; a busy lane reports busy and is untouched.
vslam_status vslam_batch::fuse_loop(const uint8_t* mask, const vslam_fuse_loop_params* prm, vslam_fuse_loop_report* reps) {
    static const char* const fn = "vslam_batch_fuse_loop";
    int nOn = 0;
    VS_CHECK(followup_check_args(fn, mask, reps));
    vslam_fuse_loop_params P;
    if (!resolve_fuse_loop_params(fn, prm, P)) return VSLAM_ERR_INVALID;
    VS_CHECK(followup_check_lanes(fn, mask, &nOn));
    if (!nOn) return VSLAM_OK;
    VS_HIP(hipSetDevice(device));
    std::vector<int> run;
    for (int b = 0; b < B; b++) {
        if (!mask[b]) continue;
        reps[b] = vslam_fuse_loop_report{};
        if (sys[b]->loop_busy()) { reps[b].busy = 1; continue; }
        run.push_back(b);
    }
    const int nr = (int)run.size();
    if (!nr) return VSLAM_OK;
    std::vector<vslam_system::FuseSets> F((size_t)nr);
    std::vector<vslam_fuse_lane> lanes((size_t)nr);
    std::vector<vslam_fuse_report> sr((size_t)nr);
    std::vector<std::unique_lock<std::mutex>> locks;           // every lane's map stays as its sets saw it until its commit
    for (int i = 0; i < nr; i++) {
        vslam_system* s = sys[run[i]];
        locks.emplace_back(s->mapMutex);
        VS_CHECK(s->fuse_sets(P, &reps[run[i]], F[i]));
        lanes[i] = F[i].lane;
    }
    VS_CHECK(vslam_fuse_search_batch(lanes.data(), nr, &P.search, device, sr.data()));
    for (int i = 0; i < nr; i++) {
        reps[run[i]].search = sr[i];
        sys[run[i]]->fuse_commit(F[i], &reps[run[i]]);
    }
    return VSLAM_OK;
}

// One global bundle adjustment per masked lane, between two steps: per lane what vslam_system::global_ba does to a session, with ONE
// vslam_global_ba_batch call for all lanes that reach the solve (their factorisations' dependency chains run side by side).  Every
// lane's map is locked from its flattening to its commit.  Refusals come first and change nothing in any lane - a refusal of the
// batched solve for any lane (a free gauge, a point behind its keyframe) included: it is returned as it is.
vslam_status vslam_batch::global_ba(const uint8_t* mask, const vslam_system_gba_params* prm, vslam_system_gba_report* reps) {
    static const char* const fn = "vslam_batch_global_ba";
    int nOn = 0;
    VS_CHECK(followup_check_args(fn, mask, reps));
    vslam_system_gba_params P;
    if (!resolve_system_gba_params(fn, prm, P)) return VSLAM_ERR_INVALID;
    VS_CHECK(followup_check_lanes(fn, mask, &nOn));
    if (!nOn) return VSLAM_OK;
    VS_HIP(hipSetDevice(device));
    std::vector<int> run;
    for (int b = 0; b < B; b++) {
        if (!mask[b]) continue;
        reps[b] = vslam_system_gba_report{};
        if (sys[b]->loop_busy()) { reps[b].busy = 1; continue; }
        if (sys[b]->keyFrames.size() < 2) continue;
        run.push_back(b);
    }
    const int nr = (int)run.size();
    if (!nr) return VSLAM_OK;
    std::vector<vslam_system::GbaFlat> F((size_t)nr);
    std::vector<vslam_gba_result> R((size_t)nr);
    std::vector<vslam_gba_lane> lanes((size_t)nr);
    {
        std::vector<std::unique_lock<std::mutex>> locks;       // every lane's map stays as its problem saw it until its commit
        for (int i = 0; i < nr; i++) {
            vslam_system* s = sys[run[i]];
            vslam_system_gba_report& r = reps[run[i]];
            locks.emplace_back(s->mapMutex);
            VS_CHECK(s->gba_flatten(P.edge_weight, F[i]));
            r.n_keyframes = F[i].P.n_kf; r.n_landmarks = F[i].P.n_lm; r.n_pairs = F[i].P.n_pairs; r.n_edges = (int)F[i].edges.size();
            R[i] = vslam_gba_result{};
            R[i].kf_pose_wc = F[i].kfOut.data(); R[i].lm_xyz = F[i].lmOut.data(); R[i].pair_wrong = F[i].wrong.data();
            lanes[i] = vslam_gba_lane{&F[i].P, F[i].edges.empty() ? nullptr : F[i].edges.data(), (int32_t)F[i].edges.size(), &R[i]};
        }
        VS_CHECK(vslam_global_ba_batch(lanes.data(), nr, &P.gba, device));
        for (int i = 0; i < nr; i++) {
            reps[run[i]].gba = R[i].report;
            VS_CHECK(sys[run[i]]->gba_finish(F[i], &reps[run[i]]));
        }
    }
    for (int i = 0; i < nr; i++) VS_CHECK(sys[run[i]]->gba_activate(&reps[run[i]]));
    return VSLAM_OK;
}

// Ends a lane's session and starts a new one in its place, between two steps, on the thread that drives the group.  Nothing on the
// device is allocated or freed (a device free waits for every group's kernels, and a service whose lanes restart for ever is the steady
// state): the new session takes over the old one's matcher - same extractor images, stream and result-block slices; its rig and
// host-side frame state are reset (vslam_matcher::reset_session) - and the old session's key slabs go to the group's free list.  Order:
//   1. validate: nothing has changed when this fails;
//   2. the old session's mapping job: taken back from the group's pending lists or the engine's queues if no thread has picked it
//      up, else waited for (finish_job notifies under the session's mutex, so the session can go once the flag is seen);
//   3. the old session hands over its matcher and is released (slabs -> free list); the new one is initialised on that matcher;
//   4. the lane's per-step state, result-block slices and the prefetch are reset.
vslam_status vslam_batch::restart_lane(int lane, const vslam_system_config* config) {
    if (lane < 0 || lane >= B) { set_error("vslam_batch_restart_lane: lane %d of %d", lane, B); return VSLAM_ERR_INVALID; }
    const vslam_system_config c = config ? *config : sys[lane]->cfg;
    if (!shares(c)) { set_error("vslam_batch_restart_lane: %s", kSharedRule); return VSLAM_ERR_INVALID; }
    if (c.window > 16) { set_error("vslam_system: window > 16 keyframes is not supported by the new-point pipeline"); return VSLAM_ERR_INVALID; }
    VS_HIP(hipSetDevice(device));
    VS_HIP(hipStreamSynchronize(stream));          // (between steps the stream is idle; the slabs are written by the step's pack kernel)
    vslam_system* s = new (std::nothrow) vslam_system();
    if (!s) return VSLAM_ERR_INVALID;
    vslam_system* old = sys[lane];
    bool queued = false;
    {
        std::lock_guard<std::mutex> lk(pendMu);
        for (std::deque<vslam_system*>* q : {&npPend, &baPend})
            for (auto it = q->begin(); it != q->end();) { if (*it == old) { it = q->erase(it); queued = true; } else ++it; }
    }
    if (!queued && eng) queued = eng->eng.cancel(old);
    if (queued) old->finish_job(VSLAM_OK, "");     // (never ran: nobody else knows the job any more)
    old->wait_idle();                              // a job that an engine thread has taken: finished, its result dropped with the session
    vslam_matcher* fm = old->fm;
    old->fm = nullptr;                             // (kept: release() below frees nothing on the device)
    old->release();                                // slabs -> free list
    delete old;
    sys[lane] = s;
    ls[lane] = LaneStep{};
    needFirst[lane] = 1;
    prefetched.clear();                            // a prefetched extraction may hold the old session's next frame
    const vslam_status is = s->init(&c, fe, 2 * lane, stream, fm);
    if (is != VSLAM_OK) {                          // (cannot happen after the checks above; the lane then has no tracker until it is restarted)
        if (!s->fm) vslam_matcher_destroy(fm);
        return is;
    }
    s->mapExec = &vslam_batch::submit_mapping; s->mapExecArg = this;
    s->slabPool = &slabs;
    VS_HIP(hipMemsetAsync(d_res + (size_t)lane * 64, 0, 64 * sizeof(double), stream));
    VS_HIP(hipStreamSynchronize(stream));
    memset(h_res + (size_t)lane * 64, 0, 64 * sizeof(double));
    return VSLAM_OK;
}

extern "C" {

vslam_status vslam_batch_restart_lane(vslam_batch* b, int32_t lane, const vslam_system_config* config) {
    if (!b) return VSLAM_ERR_INVALID;
    return b->restart_lane(lane, config);
}

vslam_status vslam_batch_relocalize(vslam_batch* b, const uint8_t* const* left, const uint8_t* const* right, int32_t stride, int32_t on_device,
                                    const int32_t* frame_numbers, const uint8_t* lane_mask, const vslam_reloc_params* params, double* T_wc_out,
                                    vslam_reloc_report* reports) {
    if (!b) return VSLAM_ERR_INVALID;
    return b->relocalize(left, right, stride, on_device != 0, frame_numbers, lane_mask, params, T_wc_out, reports);
}

vslam_status vslam_batch_correct_loop(vslam_batch* b, const uint8_t* lane_mask, const int32_t* kf_loop, const double* T_wc_corrected,
                                      const vslam_loop_params* params, vslam_loop_report* reports) {
    if (!b) return VSLAM_ERR_INVALID;
    if (!kf_loop || !T_wc_corrected) { set_error("vslam_batch_correct_loop: invalid arguments"); return VSLAM_ERR_INVALID; }
    return b->loop(true, lane_mask, kf_loop, T_wc_corrected, params, reports);
}

vslam_status vslam_batch_correct_loop_imu(vslam_batch* b, const uint8_t* lane_mask, const int32_t* kf_loop, const double* T_wc_corrected,
                                          const vslam_loop_params* params, vslam_loop_report* reports, vslam_loop_imu_report* imu_reports) {
    if (!b) return VSLAM_ERR_INVALID;
    if (!kf_loop || !T_wc_corrected || !imu_reports) { set_error("vslam_batch_correct_loop_imu: invalid arguments"); return VSLAM_ERR_INVALID; }
    return b->loop(true, lane_mask, kf_loop, T_wc_corrected, params, reports, imu_reports);
}

vslam_status vslam_batch_close_loop_imu(vslam_batch* b, const uint8_t* lane_mask, const vslam_loop_params* params, vslam_loop_report* reports,
                                        vslam_loop_imu_report* imu_reports) {
    if (!b) return VSLAM_ERR_INVALID;
    if (!imu_reports) { set_error("vslam_batch_close_loop_imu: invalid arguments"); return VSLAM_ERR_INVALID; }
    return b->loop(false, lane_mask, nullptr, nullptr, params, reports, imu_reports);
}

vslam_status vslam_batch_close_loop(vslam_batch* b, const uint8_t* lane_mask, const vslam_loop_params* params, vslam_loop_report* reports) {
    if (!b) return VSLAM_ERR_INVALID;
    return b->loop(false, lane_mask, nullptr, nullptr, params, reports);
}

vslam_status vslam_batch_fuse_loop(vslam_batch* b, const uint8_t* lane_mask, const vslam_fuse_loop_params* params, vslam_fuse_loop_report* reports) {
    if (!b) return VSLAM_ERR_INVALID;
    return b->fuse_loop(lane_mask, params, reports);
}

vslam_status vslam_batch_global_ba(vslam_batch* b, const uint8_t* lane_mask, const vslam_system_gba_params* params, vslam_system_gba_report* reports) {
    if (!b) return VSLAM_ERR_INVALID;
    return b->global_ba(lane_mask, params, reports);
}

vslam_status vslam_batch_relocalize_imu(vslam_batch* b, const uint8_t* const* left, const uint8_t* const* right, int32_t stride, int32_t on_device,
                                        const int32_t* frame_numbers, const vslam_imu_bucket* imu, const uint8_t* lane_mask,
                                        const vslam_reloc_params* params, double* T_wc_out, vslam_reloc_report* reports,
                                        vslam_reloc_imu_report* imu_reports) {
    if (!b) return VSLAM_ERR_INVALID;
    return b->relocalize(left, right, stride, on_device != 0, frame_numbers, lane_mask, params, T_wc_out, reports, true, imu, imu_reports);
}

vslam_status vslam_batch_relocalize_debug(vslam_batch* b, int32_t lane, int32_t* d1_i1_d2, int32_t cap_points, int32_t* key_winner,
                                          int32_t cap_keys, int32_t* hyp_counts, int32_t cap_hypotheses, uint8_t* inlier_flags,
                                          int32_t cap_pairs, int32_t* sizes4) {
    if (!b) return VSLAM_ERR_INVALID;
    if (lane < 0 || lane >= b->B) { set_error("vslam_batch_relocalize_debug: lane %d of %d", lane, b->B); return VSLAM_ERR_INVALID; }
    return b->sys[lane]->fm->relocalize_debug(d1_i1_d2, cap_points, key_winner, cap_keys, hyp_counts, cap_hypotheses, inlier_flags, cap_pairs, sizes4);
}

vslam_status vslam_batch_memory(vslam_batch* b, int64_t* key_slab_bytes, int32_t* slabs_in_use, int32_t* slabs_free) {
    if (!b) return VSLAM_ERR_INVALID;
    b->slabs.stats(key_slab_bytes, slabs_in_use, slabs_free);
    return VSLAM_OK;
}

vslam_status vslam_batch_create(const vslam_system_config* configs, int32_t lanes, int32_t host_threads, int32_t mapping_threads,
                                vslam_batch** out) {
    if (!out) return VSLAM_ERR_INVALID;
    *out = nullptr;
    vslam_batch* b = new (std::nothrow) vslam_batch();
    if (!b) return VSLAM_ERR_INVALID;
    vslam_status s = b->init(configs, lanes, host_threads, mapping_threads);
    if (s != VSLAM_OK) { b->release(); delete b; return s; }
    *out = b;
    return VSLAM_OK;
}

void vslam_batch_destroy(vslam_batch* b) {
    if (!b) return;
    b->release();
    delete b;
}

vslam_status vslam_batch_track_stereo(vslam_batch* b, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                      int32_t on_device, const int32_t* frame_numbers, const vslam_imu_bucket* imu,
                                      const uint8_t* lane_mask, double* T_wc_out, vslam_frame_report* reports) {
    if (!b) return VSLAM_ERR_INVALID;
    return b->step(left, right, stride, 1, on_device != 0, frame_numbers, imu, lane_mask, T_wc_out, reports);
}

vslam_status vslam_batch_track_stereo_prefetch(vslam_batch* b, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                               const int32_t* frame_numbers, const vslam_imu_bucket* imu, const uint8_t* lane_mask,
                                               double* T_wc_out, vslam_frame_report* reports, const uint8_t* const* next_left,
                                               const uint8_t* const* next_right, const uint8_t* next_mask) {
    if (!b) return VSLAM_ERR_INVALID;
    return b->step(left, right, stride, 1, true, frame_numbers, imu, lane_mask, T_wc_out, reports, next_left, next_right, next_mask);
}

static vslam_status batch_color_args(const vslam_batch* b, int32_t stride, int32_t channels, const char* fn) {
    if ((channels != 1 && channels != 3 && channels != 4) || stride < b->fe->width * channels) {
        set_error("%s: channels %d (1, 3 or 4), stride %d (at least width x channels)", fn, channels, stride);
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}

vslam_status vslam_batch_track_stereo_color(vslam_batch* b, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                            int32_t channels, int32_t on_device, const int32_t* frame_numbers, const vslam_imu_bucket* imu,
                                            const uint8_t* lane_mask, double* T_wc_out, vslam_frame_report* reports) {
    if (!b) return VSLAM_ERR_INVALID;
    VS_CHECK(batch_color_args(b, stride, channels, "vslam_batch_track_stereo_color"));
    return b->step(left, right, stride, channels, on_device != 0, frame_numbers, imu, lane_mask, T_wc_out, reports);
}

vslam_status vslam_batch_track_stereo_prefetch_color(vslam_batch* b, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                                     int32_t channels, const int32_t* frame_numbers, const vslam_imu_bucket* imu,
                                                     const uint8_t* lane_mask, double* T_wc_out, vslam_frame_report* reports,
                                                     const uint8_t* const* next_left, const uint8_t* const* next_right,
                                                     const uint8_t* next_mask) {
    if (!b) return VSLAM_ERR_INVALID;
    VS_CHECK(batch_color_args(b, stride, channels, "vslam_batch_track_stereo_prefetch_color"));
    return b->step(left, right, stride, channels, true, frame_numbers, imu, lane_mask, T_wc_out, reports, next_left, next_right, next_mask);
}

vslam_status vslam_batch_set_rectifiers(vslam_batch* b, int32_t lane, const vslam_rectifier* left, const vslam_rectifier* right) {
    if (!b) return VSLAM_ERR_INVALID;
    if (lane < -1 || lane >= b->B) { set_error("vslam_batch_set_rectifiers: lane %d of %d (-1 = every lane)", lane, b->B); return VSLAM_ERR_INVALID; }
    // (all lanes share image size and device: what one lane accepts, every lane accepts)
    for (int k = 0; k < b->B; k++) if (lane < 0 || k == lane) VS_CHECK(b->sys[k]->set_rectifiers(left, right, "vslam_batch_set_rectifiers"));
    b->prefetched.clear();      // a prefetched extraction went through the rectifiers bound before
    return VSLAM_OK;
}

// a raw call's arguments against the rectifiers of every lane that is active in this step (or the prefetched one)
static vslam_status batch_raw_args(const vslam_batch* b, int32_t stride, int32_t channels, const uint8_t* mask, const uint8_t* nextMask,
                                   bool next, const char* fn) {
    for (int k = 0; k < b->B; k++) {
        if (!((!mask || mask[k]) || (next && (!nextMask || nextMask[k])))) continue;
        VS_CHECK(b->sys[k]->raw_args(stride, channels, fn));
    }
    return VSLAM_OK;
}

vslam_status vslam_batch_track_stereo_raw(vslam_batch* b, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                          int32_t channels, int32_t on_device, const int32_t* frame_numbers, const vslam_imu_bucket* imu,
                                          const uint8_t* lane_mask, double* T_wc_out, vslam_frame_report* reports) {
    if (!b) return VSLAM_ERR_INVALID;
    VS_CHECK(batch_raw_args(b, stride, channels, lane_mask, nullptr, false, "vslam_batch_track_stereo_raw"));
    return b->step(left, right, stride, channels, on_device != 0, frame_numbers, imu, lane_mask, T_wc_out, reports, nullptr, nullptr, nullptr, true);
}

vslam_status vslam_batch_track_stereo_prefetch_raw(vslam_batch* b, const uint8_t* const* left, const uint8_t* const* right, int32_t stride,
                                                   int32_t channels, const int32_t* frame_numbers, const vslam_imu_bucket* imu,
                                                   const uint8_t* lane_mask, double* T_wc_out, vslam_frame_report* reports,
                                                   const uint8_t* const* next_left, const uint8_t* const* next_right,
                                                   const uint8_t* next_mask) {
    if (!b) return VSLAM_ERR_INVALID;
    VS_CHECK(batch_raw_args(b, stride, channels, lane_mask, next_mask, next_left && next_right, "vslam_batch_track_stereo_prefetch_raw"));
    return b->step(left, right, stride, channels, true, frame_numbers, imu, lane_mask, T_wc_out, reports, next_left, next_right, next_mask, true);
}

vslam_system* vslam_batch_system(vslam_batch* b, int32_t lane) {
    if (!b || lane < 0 || lane >= b->B) return nullptr;
    return b->sys[lane];
}

int32_t vslam_batch_lanes(const vslam_batch* b) { return b ? b->B : 0; }

vslam_status vslam_batch_wait_mapping(vslam_batch* b) {
    if (!b) return VSLAM_ERR_INVALID;
    b->kick();
    for (vslam_system* s : b->sys) VS_CHECK(vslam_system_wait_mapping(s));
    return VSLAM_OK;
}

vslam_status vslam_batch_set_timing(vslam_batch* b, int32_t on) {
    if (!b) return VSLAM_ERR_INVALID;
    b->timer.enabled = on != 0;
    b->fe->timer.enabled = on != 0;
    return VSLAM_OK;
}

// local-BA stage timing of the mapping engine's cohorts (HIP events on its stream): switch, and read-and-reset of the sums
vslam_status vslam_batch_set_ba_timing(vslam_batch* b, int32_t on) {
    if (!b) return VSLAM_ERR_INVALID;
    if (b->eng) b->eng->baTimingOn = on ? 1 : 0;
    return VSLAM_OK;
}
vslam_status vslam_batch_ba_timings(vslam_batch* b, const char** names, float* ms, int32_t cap, int32_t* n_out, int64_t* cohorts_out, int64_t* lanes_out) {
    if (!b || !n_out || !names || !ms) return VSLAM_ERR_INVALID;
    int n = 0;
    if (cohorts_out) *cohorts_out = 0;
    if (lanes_out) *lanes_out = 0;
    if (b->eng) {
        MapEngine& e = *b->eng;
        std::lock_guard<std::mutex> lk(e.btMu);
        for (auto& t : e.baTimes) if (n < cap) { names[n] = t.first; ms[n] = t.second; n++; }
        if (cohorts_out) *cohorts_out = e.baTimedCohorts;
        if (lanes_out) *lanes_out = e.baTimedLanes;
        e.baTimes.clear(); e.baTimedCohorts = 0; e.baTimedLanes = 0;
    }
    *n_out = n;
    return VSLAM_OK;
}

// device time per stage (batched launches: all lanes) since the last read, then the host phases of the last step
vslam_status vslam_batch_timings(vslam_batch* b, const char** names, float* ms, int32_t cap, int32_t* n_out, double* host_phases7) {
    if (!b || !n_out) return VSLAM_ERR_INVALID;
    VS_HIP(hipSetDevice(b->device));
    VS_HIP(hipStreamSynchronize(b->stream));
    VS_HIP(hipStreamSynchronize(b->fe->stream));
    const char* nm[64];
    float tv[64];
    int n = 0;
    {
        const int k = b->fe->timer.read(nm, tv, 64);
        b->fe->timer.reset();
        for (int i = 0; i < k && n < cap; i++, n++) { if (names) names[n] = nm[i]; if (ms) ms[n] = tv[i]; }
    }
    {
        const int k = b->timer.read(nm, tv, 64);
        b->timer.reset();
        for (int i = 0; i < k && n < cap; i++, n++) { if (names) names[n] = nm[i]; if (ms) ms[n] = tv[i]; }
    }
    *n_out = n;
    if (host_phases7) for (int i = 0; i < 7; i++) host_phases7[i] = b->phase[i];
    return VSLAM_OK;
}

}  // extern "C"
