// ThreadSanitizer check of JobEngine::cancel (gtsam-vslam_amd/csrc/job_engine.hpp), the queue removal behind vslam_batch_restart_lane:
// a producer releases jobs and takes some of them back while the engine threads take cohorts.  Every job is either served exactly once
// (cancel returned false: a thread had it already) or never (cancel returned true) - a job that was taken back must not run afterwards,
// because its owner's memory is gone by then.
#include "job_engine.hpp"
#include <atomic>
#include <cstdio>

int main() {
    constexpr int N = 20000;
    static std::atomic<int> served[N], cancelled[N];
    for (int i = 0; i < N; i++) { served[i] = 0; cancelled[i] = 0; }
    {
        vslam::JobEngine<int> E;
        for (int kind = 0; kind < 2; kind++)
            E.lanes[kind].serve = [&](std::vector<int>& c) { for (int j : c) served[j]++; };
        E.start(1, 2);
        std::deque<int> a, b;
        for (int i = 0; i < N; i++) {
            (i & 1 ? a : b).push_back(i);
            if ((i & 3) == 3) {
                E.release_jobs(a, b);
                if (E.cancel(i)) cancelled[i] = 1;             // the newest job ...
                if (E.cancel(i - 1)) cancelled[i - 1] = 1;     // ... and one of the other kind
                if (E.cancel(N + 5)) { printf("FAILED: cancelled a job that was never queued\n"); return 1; }
            }
        }
        E.shutdown();
    }
    int nc = 0;
    for (int i = 0; i < N; i++) {
        if (served[i] + cancelled[i] != 1) { printf("FAILED: job %d served %d times, cancelled %d\n", i, served[i].load(), cancelled[i].load()); return 1; }
        nc += cancelled[i];
    }
    printf("ok: %d of %d jobs taken back\n", nc, N);
    return 0;
}
