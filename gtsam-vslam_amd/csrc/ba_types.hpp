// Local BA: what the host code and the kernels of ba.hip agree on - argument blocks, the LM control block, the constants the host
// sizes launches with.  Plain structs and constexpr only (no HIP calls): also compiled by g++ for the CPU tests of the host code
// (tests/native/ba_host_order.cpp).  Field order and types of the structs are kernel ABI.
#pragma once
#include "dmath.hpp"
#include "ba_packed.hpp"
#include <cstddef>
#include <cstdint>

namespace vslam {

constexpr int BA_MAX_LEVELS = 12;         // = MAX_LEVELS (common.hpp; asserted in ba.hip)

struct BaEdge {
    int a, b, fa, fb;
    DPose measured;
    double r[6], Ja[36], Jb[36];
    double Haa[36], Hab[36], Hbb[36], ga[6], gb[6];   // Ja^T Ja, Ja^T Jb, Jb^T Jb, Ja^T r, Jb^T r (filled at linearisation)
};

struct BaDev {
    int NF, Lp, F, K, NE, n;
    const int* facKf; const int* facFi; const int* facLp; const int* facLm;
    const double* facZ; const double* facIs; const uint8_t* facRight;
    double* facJ;
    const int* lpStart; const int* lpSlotStart; const int* slotStart; const int* slotFi; const int* lpOrig;
    DPose* poseCur; DPose* poseTrial; const int* fidx;
    double* lmCur; double* lmTrial;
    BaEdge* edges;
    double* S; double* rhs; double* Spart; double* Sedge; double* dP; double* dL;
    double* sums; double* partial;
    int* flags;
    double fx, fy, cx, cy, b;
    double* ctl;      // device-side LM state (below)
    // ---- lambda look-ahead + speculative linearisation (single GPU) --------------------------------------
    // One "trial" launch evaluates NB candidates lambda, 10 lambda, 100 lambda ... at once (grid dimension y / z /
    // x of the per-trial kernels); the control step then walks them in order exactly as the sequential policy
    // would (the outcome of a rejected trial only changes lambda), so the result is bit-identical to NB = 1
    // while a chain of rejections costs one round instead of NB.
    // Values live in NB + 1 slots; slot `sel` is current, candidate c writes slot (sel + 1 + c) mod (NB + 1).
    // With specLin every candidate also linearises at its trial values into its slot's facJ / edge buffers, so
    // an accepted step needs no linearisation launch of its own.
    int NB, specLin, cand;
    // Large problems: the look-ahead is ADAPTIVE - a round evaluates only nAct candidates (control block, CI_NACT): one
    // while steps are being accepted, all NB after a round that ended in rejections (a rejection chain is then walked in
    // one round as before).  The sequential policy is replayed unchanged; candidates that are not evaluated cost nothing.
    int adaptive, nAct;                  // nAct: set by ba_enter
    double lambda;                       // set by ba_enter: damping of this workgroup's candidate
    DPose* poseBase; double* lmBase; size_t lmStride;
    double* facJBase; size_t facJStride; double* SedgeBase; BaEdge* edgesBase;
    double* facJ2; double* Sedge2; BaEdge* edges2;            // set by ba_enter (slot of the candidate)
    size_t sysStride, spartStride, partialStride, dLStride;
    int solveKind;                       // which reduced-camera solve serves this lane (a batch may mix kinds: each kernel skips foreign lanes)
    double* Lg;                          // k_ba_solve_mfma: the lane's factor storage (null: the launch's argument)
    double* ctlHost;                     // != null: pinned host mirror of the control block, written by the control step (the host's poll is then a wait, not a copy)
};
enum { BA_SOLVE_MFMA64 = 0, BA_SOLVE_WAVE = 1, BA_SOLVE_MFMA = 2, BA_SOLVE_LARGE = 3 };

// The LM policy (GTSAM 4.2) runs on the DEVICE: the control step after each linearisation / trial updates this
// block, every other kernel starts by checking that it is its turn (state) and picks the current / trial
// buffers by `sel`.  The host enqueues a few speculative steps at a time and only reads the
// block back to learn whether the pass has finished - no host round trip per lambda trial.
enum { CTL_LAMBDA = 0, CTL_ERROR = 1, CTL_CUR = 2, CTL_INIT_ERR = 3, CTL_INTS = 8, CTL_DOUBLES = 16 };
enum { CI_STATE = 0, CI_SEL = 1, CI_ITER = 2, CI_INNER = 3, CI_MAXIT = 4, CI_FIRST = 5, CI_NACT = 6, CI_ROUNDS = 7 };
enum { BA_LINEARIZE = 0, BA_TRY = 1, BA_DONE = 2 };
enum { BA_MAX_NB = 4, SUMS_CAND = 16, FLAG_COUNT = 1, FLAG_FAIL = 4 };   // sums[16 + 2c | 17 + 2c], flags[4 + c] per candidate

constexpr int BA_SCHUR_WAVES = 16;         // max landmarks in flight per workgroup (one per wave): the LDS copy of S is
                                           // zeroed / written out once per group; the host picks 16, 8 or 4 to fit the LDS
constexpr int BA_LDS_MAX_F = 20;          // (6F)^2 doubles must fit next to the W staging in 160 KB
// A workgroup gets 160 KB of LDS, static and dynamic together.  The batch's kernels with dynamic LDS have (almost) no static LDS:
// its plan keeps BA_STATIC_LDS_RESERVE bytes for it, and ba_kernel_attributes checks the code objects against the reserve.
constexpr int BA_LDS_BYTES = 160 * 1024, BA_STATIC_LDS_RESERVE = 1024, BA_DYN_LDS_MAX = BA_LDS_BYTES - BA_STATIC_LDS_RESERVE;
constexpr int BA_MAX_FREE_KF = 170;       // 6 F <= 1024 unknowns: the largest reduced camera system the solves take

// lanes that serve one landmark in k_ba_schur / k_ba_back (ba_lm_blocks)
constexpr int BA_LPL_SCHUR = 64, BA_LPL_BACK = 32;

// k_ba_schur2 / k_ba_back2 (tracker windows): free keyframes at most, and the doubles of one landmark-wave's staging region
constexpr int BA2_MAX_F = 10;
BA_PACKED_HD int ba2_stage_doubles(int maxFac, int maxSlots) {
    const int ints = maxFac + 2 * (maxSlots + 1);
    return ((maxFac * 20 + 2 * maxSlots * 18 + 10 + (ints + 1) / 2) + 1) & ~1;        // even: rows are copied as double2
}
// Layout of the workgroup's LDS copy of the system (and of the partial it writes out):
//   BA2_PACKED     upper 6x6 blocks only, block pitch BA_PACKED_PITCH (ba_packed.hpp) - the production form: 2 095 instead of 3 660
//                  doubles to zero, flush, write and sum at F = 10, and block bases spread over the LDS banks;
//   BA2_ROWMAJOR   n x n row-major with pitch n (the form of D.S; k_ba_schur's);  BA2_ROWMAJOR1  the same with LDS pitch n + 1 (the
//                  bank effect alone; written out with pitch n).  Developer overrides: VSLAM_BA_SCHUR2_LAYOUT = 0 / 1.
enum { BA2_ROWMAJOR = 0, BA2_ROWMAJOR1 = 1, BA2_PACKED = 2 };
BA_PACKED_HD int ba2_sys_doubles(int n, int layout) {       // LDS doubles of the system copy (even: the staging regions follow)
    return layout == BA2_PACKED ? (ba_packed_doubles(n / 6) + 1) & ~1 : layout == BA2_ROWMAJOR1 ? n * (n + 1) + n : n * n + n;
}
BA_PACKED_HD int ba2_part_doubles(int n, int layout) {      // doubles of one partial in Spart
    return layout == BA2_PACKED ? ba_packed_doubles(n / 6) : n * n + n;
}

// Windowed Schur accumulation (k_ba_lm_prep / k_ba_schur_win / k_ba_reduce_win; see there)
struct BaWin {
    int TB, T, TP, tileDoubles, nWin;      // T = 6 TB; tile = T rows of pitch TP = T + 1 (rows 6 apart must not share an
                                           // LDS bank pair) followed by T right-hand-side entries (diagonal windows)
    const int* winA; const int* winB;      // [nWin] block row / block column of a window
    const int* winFirstWg;                 // [nWin + 1] first workgroup (= partial) of each window
    const int* wgWin; const int* wgBegin; const int* wgEnd;   // [nWg] window and range of winLm of a workgroup
    const int* winLm;                      // concatenated landmark lists (local landmark index lp)
    double* part;                          // [nWg][NB][tileDoubles]
    double* Wg; double* Hg;                // per slot entry: Hpl block (18), per landmark: Hll (6) | bl (3) - k_ba_lm_prep
};
constexpr int BA_WIN_HG = 9 + 6 * BA_MAX_NB;      // doubles per landmark: Hll (6) | bl (3) | per candidate the 6 unique entries of (Hll + lambda I)^-1
constexpr int BA_WIN_META = 5 * 64 + 65;       // ints of LDS per wave: lp, seR, nR, seC, nC per entry + prefix

// sizes of the reduced-camera solves: k_ba_solve_wave, k_ba_solve_mfma, k_ba_chol_col / k_ba_chol_back (see the kernels)
constexpr int BA_WAVE_N = 60;
constexpr int BA_MFMA_N = 256, BA_MFMA_NB = BA_MFMA_N / 16, BA_MFMA_NW = 8, BA_MFMA_SLOTS = 17, BA_MFMA_LD = 17;
constexpr int CH_B = 64, CH_LD = 65, CH_PLD = 17;

// chi2 re-check (src/OptimizationBA.cpp:787-871): pair-parallel
struct BaChi {
    int NP; const int* pairKf; const int* pairLm; const uint8_t* pairFlags; const float* pairUv; const int* pairOct;
    const uint8_t* kfLocal; const uint8_t* kfPresent; const uint8_t* lmPresent; const DPose* pose; const double* lm;
    float thr[BA_MAX_LEVELS]; double fx, fy, cx, cy, b; uint8_t* wrong;
};
// batch only: the steps the one-problem path drives from the host, per lane
struct BaLaneAux {
    BaChi C;                                        // chi2 re-check (C.pose / C.lm: taken from the lane's current value slot)
    int NF; const int* facPair; double* facIs;      // k_ba_mask
    int nPose, nLm; const double* pose0; const double* lm0;     // k_ba_init_slots over the lane's NB + 1 slots
    double* outPose; double* outLm;                 // final values, gathered for one download
};

}  // namespace vslam
