// Factor ordering of local BA on the device (large problems: the 100 k-landmark window): the k_ord_* / k_win_* kernels and the host
// unit that drives them (BaDeviceOrder).  Part of the ba.hip translation unit: included there, and only there, after the argument
// blocks (ba_types.hpp), the host ordering (ba_order_host.hpp) and the workspace buffer types (DevBuf, PinBuf, PinnedArena).
#pragma once

namespace vslam {

// ---- factor ordering on the device (large problems: the 100 k-landmark window) --------------------------------------------------
// BaPassHost::count / fill as kernels over the raw pair arrays, which are on the device anyway (the chi2 kernel reads them).  The
// factor order is (landmark, free index, pair, side): a TOTAL order - the bucket of a landmark is filled in arrival order (atomics)
// and every factor then finds its place by counting the entries of its bucket that precede it, so the result does not depend on the
// arrival order and equals the host's stable counting sort + insertion sort entry for entry.
struct BaOrd {
    int NP, L, K, world, rank;
    const int* pairKf; const int* pairLm; const uint8_t* pairFlags; const uint8_t* wrong; const float* pairUv; const int* pairOct;
    int* cnt; int* lpOf; int* tLpOrig; int* tLpStart; int* kfPres; uint8_t* lmPres; long long* scal;      // phase 1 (sized by L, K)
    const int* fidx; int* fillc; int* ns; int* key; int* src; int* key2; int* src2;                        // phase 2 (sized by NF, Lp)
    int* facKf; int* facFi; int* facLp; int* facLm; int* facPair; double* facZ; double* facIs; uint8_t* facRight;
    int* lpStart; int* lpSlotStart; int* lpOrig; int* slotStart; int* slotFi;
    float invSigma[MAX_LEVELS];
};
enum { ORD_LP = 0, ORD_NF = 1, ORD_NSLOT = 2, ORD_MAXSLOTS = 3, ORD_MAXFAC = 4, ORD_SUMK2 = 5, ORD_K2_MASKED = 6, ORD_SCAL = 8 };

__global__ __launch_bounds__(256) void k_ord_count(BaOrd O) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < O.NP; p += gridDim.x * 256) {
        if (O.wrong[p]) continue;
        const int fl = O.pairFlags[p] & 3;
        if (!fl) continue;
        const int l = O.pairLm[p];
        O.kfPres[O.pairKf[p]] = 1; O.lmPres[l] = 1;             // graph membership is global
        if (l % O.world != O.rank) continue;                      // landmark shard of this rank
        atomicAdd(&O.cnt[l], (fl & 1) + (fl >> 1));
    }
}
// One workgroup walks an array in tiles of 1024 consecutive elements (coalesced): exclusive prefix of two ints per element = carry of the
// tiles before + prefix of the waves before (LDS) + the wave's own inclusive scan (shuffles).  Two barriers per tile.
struct OrdScan {
    int carryA = 0, carryB = 0;
    __device__ __forceinline__ void tile(int a, int b, int* sA, int* sB, int& exA, int& exB) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        int ia = a, ib = b;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int ta = __shfl_up(ia, d), tb = __shfl_up(ib, d);
            if (lane >= d) { ia += ta; ib += tb; }
        }
        if (lane == 63) { sA[wave] = ia; sB[wave] = ib; }
        __syncthreads();
        int pa = 0, pb = 0, ta = 0, tb = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) { const int va = sA[w], vb = sB[w]; if (w < wave) { pa += va; pb += vb; } ta += va; tb += vb; }
        exA = carryA + pa + ia - a; exB = carryB + pb + ib - b;
        carryA += ta; carryB += tb;
        __syncthreads();
    }
};
// landmarks of this rank's shard that are in the graph, in index order: lpOf / lpOrig, and the start of every bucket
__global__ __launch_bounds__(1024) void k_ord_scan_lm(BaOrd O) {
    __shared__ int sA[16], sB[16];
    OrdScan sc;
    constexpr int E = 4;             // consecutive elements per thread and tile
    for (int base = 0; base < O.L; base += 1024 * E) {
        const int l0 = base + threadIdx.x * E;
        bool in[E]; int cn[E];
        int a = 0, b = 0;
#pragma unroll
        for (int j = 0; j < E; j++) {
            const int l = l0 + j;
            in[j] = l < O.L && O.lmPres[l] && l % O.world == O.rank;
            cn[j] = in[j] ? O.cnt[l] : 0;
            a += in[j] ? 1 : 0; b += cn[j];
        }
        int ea, eb;
        sc.tile(a, b, sA, sB, ea, eb);
#pragma unroll
        for (int j = 0; j < E; j++) {
            const int l = l0 + j;
            if (l >= O.L) break;
            if (in[j]) { O.lpOf[l] = ea; O.tLpOrig[ea] = l; O.tLpStart[ea] = eb; ea++; eb += cn[j]; }
            else O.lpOf[l] = -1;
        }
    }
    if (threadIdx.x == 0) { O.tLpStart[sc.carryA] = sc.carryB; O.scal[ORD_LP] = sc.carryA; O.scal[ORD_NF] = sc.carryB; O.scal[ORD_K2_MASKED] = 0; }
}
__global__ __launch_bounds__(256) void k_ord_scatter(BaOrd O) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < O.NP; p += gridDim.x * 256) {
        if (O.wrong[p]) continue;
        const int l = O.pairLm[p];
        if (l % O.world != O.rank) continue;
        const int fl = O.pairFlags[p] & 3;
        if (!fl) continue;
        const int lp = O.lpOf[l], fi = O.fidx[O.pairKf[p]];
        const int c = (fl & 1) + (fl >> 1);
        int pos = O.tLpStart[lp] + atomicAdd(&O.fillc[lp], c);
        for (int side = 0; side < 2; side++) {
            if (!((fl >> side) & 1)) continue;
            O.key[pos] = fi; O.src[pos] = 2 * p + side; O.facLp[pos] = lp;
            pos++;
        }
    }
}
// every factor finds its place inside its landmark's bucket: the number of entries (fi, 2 pair + side) that precede it
__global__ __launch_bounds__(256) void k_ord_rank(BaOrd O, int NF) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const int lp = O.facLp[f], f0 = O.tLpStart[lp], f1 = O.tLpStart[lp + 1];
    const int k = O.key[f], v = O.src[f];
    int r = 0;
    for (int g = f0; g < f1; g++) { const int kg = O.key[g], vg = O.src[g]; r += (kg < k || (kg == k && vg < v)) ? 1 : 0; }
    O.key2[f0 + r] = k; O.src2[f0 + r] = v;
}
__global__ __launch_bounds__(256) void k_ord_ns(BaOrd O, int Lp) {
    const int lp = blockIdx.x * 256 + threadIdx.x;
    if (lp >= Lp) return;
    int last = -2, ns = 0;
    for (int f = O.tLpStart[lp]; f < O.tLpStart[lp + 1]; f++) { const int fi = O.key2[f]; if (fi >= 0 && fi != last) { last = fi; ns++; } }
    O.ns[lp] = ns;
}
// slot-table prefix (per landmark its slots + an end sentinel), the statistics of the pass, and the landmark arrays into their final place
__global__ __launch_bounds__(1024) void k_ord_scan_slots(BaOrd O, int Lp) {
    __shared__ int sA[16], sB[16];
    __shared__ int rA[1024], rB[1024];
    __shared__ long long rK[1024];
    const int tid = threadIdx.x;
    OrdScan sc;
    int mx = 0, mf = 0;
    long long k2 = 0;
    constexpr int E = 4;
    for (int base = 0; base < Lp; base += 1024 * E) {
        const int lp0 = base + tid * E;
        int nsv[E];
        int a = 0;
#pragma unroll
        for (int j = 0; j < E; j++) {
            const int lp = lp0 + j;
            nsv[j] = 0;
            if (lp < Lp) {
                const int ns = O.ns[lp], f0 = O.tLpStart[lp], nf = O.tLpStart[lp + 1] - f0;
                nsv[j] = ns + 1; a += ns + 1; mx = max(mx, ns); mf = max(mf, nf); k2 += (long long)ns * ns;
                O.lpStart[lp] = f0; O.lpOrig[lp] = O.tLpOrig[lp];
            }
        }
        int ea, eb;
        sc.tile(a, 0, sA, sB, ea, eb);
#pragma unroll
        for (int j = 0; j < E; j++) { const int lp = lp0 + j; if (lp < Lp) { O.lpSlotStart[lp] = ea; ea += nsv[j]; } }
    }
    rA[tid] = mx; rB[tid] = mf; rK[tid] = k2;
    __syncthreads();
    for (int d = 512; d >= 1; d >>= 1) {
        if (tid < d) { rA[tid] = max(rA[tid], rA[tid + d]); rB[tid] = max(rB[tid], rB[tid + d]); rK[tid] += rK[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) {
        O.lpSlotStart[Lp] = sc.carryA; O.lpStart[Lp] = O.tLpStart[Lp]; O.scal[ORD_NSLOT] = sc.carryA;
        O.scal[ORD_MAXSLOTS] = max(rA[0], 1); O.scal[ORD_MAXFAC] = max(rB[0], 1); O.scal[ORD_SUMK2] = rK[0];
    }
}
// statistics of the masked second pass: sum over the landmarks of (free keyframes still observing it)^2 with the rejected pairs left out
__global__ __launch_bounds__(256) void k_ord_k2_masked(BaOrd O, int Lp) {
    __shared__ long long sK[4];
    const int lp = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long k2 = 0;
    if (lp < Lp) {
        int last = -2, ns = 0;
        for (int f = O.lpStart[lp]; f < O.lpStart[lp + 1]; f++) {
            if (O.wrong[O.facPair[f]]) continue;
            const int fi = O.facFi[f];
            if (fi >= 0 && fi != last) { last = fi; ns++; }
        }
        k2 = (long long)ns * ns;
    }
    for (int d = 32; d >= 1; d >>= 1) k2 += __shfl_xor(k2, d);
    if (lane == 0) sK[wave] = k2;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd((unsigned long long*)&O.scal[ORD_K2_MASKED], (unsigned long long)(sK[0] + sK[1] + sK[2] + sK[3]));
}
__global__ __launch_bounds__(256) void k_ord_emit_fac(BaOrd O, int NF) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const int fi = O.key2[f], sv = O.src2[f], p = sv >> 1, side = sv & 1;
    O.facKf[f] = O.pairKf[p]; O.facFi[f] = fi; O.facLm[f] = O.pairLm[p];
    O.facZ[2 * (size_t)f] = (double)O.pairUv[4 * (size_t)p + 2 * side]; O.facZ[2 * (size_t)f + 1] = (double)O.pairUv[4 * (size_t)p + 2 * side + 1];
    O.facIs[f] = 1.0 / (1.0 / (double)O.invSigma[O.pairOct[2 * p + side]]);
    O.facRight[f] = (uint8_t)side;
    O.facPair[f] = p;
}
__global__ __launch_bounds__(256) void k_ord_emit_slots(BaOrd O, int Lp) {
    const int lp = blockIdx.x * 256 + threadIdx.x;
    if (lp >= Lp) return;
    const int f0 = O.tLpStart[lp], f1 = O.tLpStart[lp + 1];
    int se = O.lpSlotStart[lp], last = -2;
    for (int f = f0; f < f1; f++) {
        const int fi = O.key2[f];
        if (fi >= 0 && fi != last) { O.slotStart[se] = f; O.slotFi[se] = fi; se++; last = fi; }
    }
    O.slotStart[se] = f1; O.slotFi[se] = -1;     // end sentinel
}


// ---- work lists of the windowed Schur accumulation on the device (same lists as the host sweep in ba_run: per window the landmarks
// with slots in both of its block rows, ascending) : per 256-landmark block and window a count, a prefix over (window, block), the fill
struct BaWinOrd {
    int Lp, TB, nBR, nWin, nBlk;
    const int* lpSlotStart; const int* slotFi;
    int* blkCnt; int* blkOff;       // [nWin][nBlk]
    int* winCnt;                    // [nWin + 1]
    int* winLm;
};
template <int FILL>
__global__ __launch_bounds__(256) void k_win_lists(BaWinOrd Q) {
    __shared__ int sWave[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lp = blockIdx.x * 256 + tid;
    unsigned long long rows = 0;        // block rows (free index / TB) this landmark has slots in: <= 43 for 170 free keyframes
    if (lp < Q.Lp)
        for (int se = Q.lpSlotStart[lp]; se < Q.lpSlotStart[lp + 1] - 1; se++) rows |= 1ull << (Q.slotFi[se] / Q.TB);
    const unsigned long long lt = (1ull << lane) - 1ull;
    int w = 0;
    for (int a = 0; a < Q.nBR; a++)
        for (int b = a; b < Q.nBR; b++, w++) {
            const bool has = ((rows >> a) & 1ull) && ((rows >> b) & 1ull);
            const unsigned long long bal = __ballot(has);
            int* sw = sWave[w & 1];                      // (double-buffered: one barrier per window)
            if (lane == 0) sw[wave] = __popcll(bal);
            __syncthreads();
            int before = 0, total = 0;
            for (int k = 0; k < 4; k++) { const int c = sw[k]; if (k < wave) before += c; total += c; }
            if (FILL) { if (has) Q.winLm[Q.blkOff[(size_t)w * Q.nBlk + blockIdx.x] + before + __popcll(bal & lt)] = lp; }
            else if (tid == 0) Q.blkCnt[(size_t)w * Q.nBlk + blockIdx.x] = total;
        }
}
__global__ __launch_bounds__(1024) void k_win_prefix(BaWinOrd Q) {
    extern __shared__ int sTot[];       // [nWin] totals, then bases
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int w = wave; w < Q.nWin; w += 16) {
        int run = 0;
        for (int base = 0; base < Q.nBlk; base += 64) {
            const int c = base + lane;
            const int v = c < Q.nBlk ? Q.blkCnt[(size_t)w * Q.nBlk + c] : 0;
            int inc = v;
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
            if (c < Q.nBlk) Q.blkOff[(size_t)w * Q.nBlk + c] = run + inc - v;
            run += __shfl(inc, 63);
        }
        if (lane == 0) sTot[w] = run;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int w = 0; w < Q.nWin; w++) { const int t = sTot[w]; sTot[w] = run; Q.winCnt[w] = run; run += t; }
        Q.winCnt[Q.nWin] = run;
    }
    __syncthreads();
    for (int w = wave; w < Q.nWin; w += 16)
        for (int c = lane; c < Q.nBlk; c += 64) Q.blkOff[(size_t)w * Q.nBlk + c] += sTot[w];
}

}  // namespace vslam

namespace {

// ---- the host side: what only the device ordering needs, and the places where ba_run hands a pass to it --------------------------
// The host keeps the free set, the BetweenFactor chain and the launch plan; nothing of the factor list comes back to it - the window
// lists and the second pass's statistics are device work too.  Every method enqueues on the call's stream, in the order written.
struct BaDeviceOrder {
    DevBuf<int> d_ord1, d_ord2, d_winTmp;
    PinBuf h_ordScal;         // read-backs: the scalars of a pass | kfPres[K]; the starts of the window lists
    BaOrd O{};
    BaWinOrd Q{};
    const long long* scal() const { return (const long long*)h_ordScal.p; }
    const uint8_t* lm_present() const { return O.lmPres; }      // (device) membership of the landmarks, as the last count left it
    void release() { d_ord1.release(); d_ord2.release(); d_winTmp.release(); h_ordScal.release(); }

    // membership, the shard's landmarks and their bucket sizes -> H.Lp, H.NF, T.kfPresent, the free set and the edge chain
    vslam_status count(const vslam_ba_problem* P, const BaPairArrays& a, uint8_t* d_wrong, int pass, int rank, int world, hipStream_t stream,
                       BaPassHost& H, BaHostTmp& T) {
        const int K = P->n_kf, L = P->n_lm, NP = P->n_pairs;
        O = BaOrd{};
        O.NP = NP; O.L = L; O.K = K; O.world = world; O.rank = rank;
        O.pairKf = a.kf; O.pairLm = a.lm; O.pairFlags = a.flags; O.wrong = d_wrong; O.pairUv = a.uv; O.pairOct = a.oct;
        for (int l = 0; l < P->n_levels; l++) O.invSigma[l] = P->inv_sigma_factor[l];
        // phase 1 buffers: cnt[L] | kfPres[K] | lmPres bytes[L] (zeroed) | lpOf[L] | tLpOrig[L] | tLpStart[L + 1] | scal
        const size_t zInts = zeroed_ints(K, L), nInts1 = zInts + (size_t)3 * L + 1 + 2 * ORD_SCAL + 2;
        VS_HIP(d_ord1.alloc(nInts1));
        int* w = d_ord1.p;
        O.cnt = w; O.kfPres = w + L; O.lmPres = (uint8_t*)(w + L + K);
        O.lpOf = w + zInts; O.tLpOrig = O.lpOf + L; O.tLpStart = O.tLpOrig + L;
        O.scal = (long long*)(w + ((zInts + (size_t)3 * L + 1 + 1) & ~(size_t)1));
        VS_HIP(h_ordScal.ensure(ORD_SCAL * sizeof(long long) + (size_t)K * sizeof(int), grow_ord_scal()));
        VS_HIP(hipMemsetAsync(w, 0, zInts * sizeof(int), stream));
        if (pass == 0) VS_HIP(hipMemsetAsync(d_wrong, 0, NP, stream));      // (later passes: the chi2 kernel's flags)
        hipLaunchKernelGGL(k_ord_count, dim3(pair_blocks(NP)), dim3(256), 0, stream, O);
        hipLaunchKernelGGL(k_ord_scan_lm, dim3(1), dim3(1024), 0, stream, O);
        VS_HIP(hipGetLastError());
        VS_CHECK(read_back(K, stream));
        H.Lp = (int)scal()[ORD_LP]; H.NF = (int)scal()[ORD_NF];
        T.kfPresent.assign(K, 0);
        for (int k = 0; k < K; k++) T.kfPresent[k] = kf_pres()[k] ? 1 : 0;
        H.free_set_and_edges(P, rank, T);
        return VSLAM_OK;
    }
    // the factor arrays and the slot table, written in place into the arena's device half -> the statistics of the pass
    vslam_status emit(const vslam_ba_problem* P, const DPose* pose0, int edgeSlots, const PinnedArena& A, hipStream_t stream, BaPassHost& H, BaHostTmp& T) {
        const int K = P->n_kf, L = P->n_lm, NP = P->n_pairs, NF = H.NF, Lp = H.Lp;
        H.fill_small(P, T, pose0, edgeSlots);
        VS_HIP(hipMemcpyAsync(A.dev(H.h_fidx), H.h_fidx, (size_t)K * sizeof(int), hipMemcpyHostToDevice, stream));
        // phase 2 buffers: fillc[Lp] (zeroed) | ns[Lp] | key | src | key2 | src2 [NF each]
        VS_HIP(d_ord2.alloc((size_t)2 * std::max(Lp, 1) + (size_t)4 * std::max(NF, 1)));
        int* w = d_ord2.p;
        O.fillc = w; O.ns = w + std::max(Lp, 1); O.key = O.ns + std::max(Lp, 1); O.src = O.key + std::max(NF, 1); O.key2 = O.src + std::max(NF, 1); O.src2 = O.key2 + std::max(NF, 1);
        O.fidx = A.dev(H.h_fidx);
        O.facKf = A.dev(H.h_facKf); O.facFi = A.dev(H.h_facFi); O.facLp = A.dev(H.h_facLp); O.facLm = A.dev(H.h_facLm); O.facPair = A.dev(H.h_facPair);
        O.facZ = A.dev(H.h_facZ); O.facIs = A.dev(H.h_facIs); O.facRight = A.dev(H.h_facRight);
        O.lpStart = A.dev(H.h_lpStart); O.lpSlotStart = A.dev(H.h_lpSlotStart); O.lpOrig = A.dev(H.h_lpOrig);
        O.slotStart = A.dev(H.h_slotStart); O.slotFi = A.dev(H.h_slotFi);
        VS_HIP(hipMemsetAsync(O.fillc, 0, (size_t)std::max(Lp, 1) * sizeof(int), stream));
        if (NF > 0) {
            hipLaunchKernelGGL(k_ord_scatter, dim3(pair_blocks(NP)), dim3(256), 0, stream, O);
            hipLaunchKernelGGL(k_ord_rank, dim3((NF + 255) / 256), dim3(256), 0, stream, O, NF);
        }
        if (Lp > 0) hipLaunchKernelGGL(k_ord_ns, dim3((Lp + 255) / 256), dim3(256), 0, stream, O, Lp);
        hipLaunchKernelGGL(k_ord_scan_slots, dim3(1), dim3(1024), 0, stream, O, Lp);
        if (NF > 0) hipLaunchKernelGGL(k_ord_emit_fac, dim3((NF + 255) / 256), dim3(256), 0, stream, O, NF);
        if (Lp > 0) hipLaunchKernelGGL(k_ord_emit_slots, dim3((Lp + 255) / 256), dim3(256), 0, stream, O, Lp);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(A.dev(H.h_lmPresent), O.lmPres, (size_t)L, hipMemcpyDeviceToDevice, stream));
        VS_HIP(hipMemcpyAsync(h_ordScal.p, O.scal, ORD_SCAL * sizeof(long long), hipMemcpyDeviceToHost, stream));
        VS_HIP(vslam::stream_wait_blocking(stream));
        H.nSlotEntries = (int)scal()[ORD_NSLOT]; H.maxSlots = (int)scal()[ORD_MAXSLOTS]; H.maxFac = (int)scal()[ORD_MAXFAC];
        H.sumK2 = scal()[ORD_SUMK2];
        return VSLAM_OK;
    }
    // windowed accumulation: the slot table is on the device - count per (window, 256-landmark block), prefix; only the nWin + 1 list
    // starts come back (*winCnt, valid until the next read-back).  The fill follows once the list buffer has its size.
    vslam_status window_counts(const BaPassHost& H, const PinnedArena& A, int TB, int nBR, int nWin, hipStream_t stream, const int** winCnt) {
        Q = BaWinOrd{};
        Q.Lp = H.Lp; Q.TB = TB; Q.nBR = nBR; Q.nWin = nWin; Q.nBlk = (H.Lp + 255) / 256;
        Q.lpSlotStart = A.dev(H.h_lpSlotStart); Q.slotFi = A.dev(H.h_slotFi);
        VS_HIP(d_winTmp.alloc((size_t)2 * nWin * std::max(Q.nBlk, 1) + nWin + 1));
        Q.blkCnt = d_winTmp.p; Q.blkOff = Q.blkCnt + (size_t)nWin * std::max(Q.nBlk, 1); Q.winCnt = Q.blkOff + (size_t)nWin * std::max(Q.nBlk, 1);
        const size_t need = ((size_t)nWin + 1) * sizeof(int);
        VS_HIP(h_ordScal.ensure(need, grow_ord_scal(), [&] { return hipStreamSynchronize(stream); }));
        if (Q.nBlk > 0) hipLaunchKernelGGL(k_win_lists<0>, dim3(Q.nBlk), dim3(256), 0, stream, Q);
        hipLaunchKernelGGL(k_win_prefix, dim3(1), dim3(1024), (size_t)nWin * sizeof(int), stream, Q);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(h_ordScal.p, Q.winCnt, need, hipMemcpyDeviceToHost, stream));
        VS_HIP(vslam::stream_wait_blocking(stream));
        *winCnt = (const int*)h_ordScal.p;
        return VSLAM_OK;
    }
    vslam_status window_fill(int* winLm, int total, hipStream_t stream) {
        if (Q.nBlk <= 0 || total <= 0) return VSLAM_OK;
        Q.winLm = winLm;
        hipLaunchKernelGGL(k_win_lists<1>, dim3(Q.nBlk), dim3(256), 0, stream, Q);
        VS_HIP(hipGetLastError());
        return VSLAM_OK;
    }
    // membership / statistics of the second graph: the count kernels again, now with the chi2 flags, and the masked slot statistics
    vslam_status second_pass(int Lp, const BaHostTmp& T, hipStream_t stream, BaSecondPass& S2) {
        const int K = O.K;
        VS_HIP(hipMemsetAsync(d_ord1.p, 0, zeroed_ints(K, O.L) * sizeof(int), stream));
        hipLaunchKernelGGL(k_ord_count, dim3(pair_blocks(O.NP)), dim3(256), 0, stream, O);
        hipLaunchKernelGGL(k_ord_scan_lm, dim3(1), dim3(1024), 0, stream, O);
        if (Lp > 0) hipLaunchKernelGGL(k_ord_k2_masked, dim3((Lp + 255) / 256), dim3(256), 0, stream, O, Lp);
        VS_HIP(hipGetLastError());
        VS_CHECK(read_back(K, stream));
        S2.kfP2.resize(K);
        for (int k = 0; k < K; k++) S2.kfP2[k] = kf_pres()[k] ? 1 : 0;
        S2.NF2 = scal()[ORD_NF]; S2.Lp2 = scal()[ORD_LP]; S2.k2 = scal()[ORD_K2_MASKED];
        S2.same = S2.kfP2 == T.kfPresent;
        return VSLAM_OK;
    }

private:
    static int pair_blocks(int NP) { return std::max(1, std::min((NP + 255) / 256, 8 * BA_NCU)); }
    static size_t zeroed_ints(int K, int L) { return (size_t)L + K + ((size_t)L + 3) / 4; }
    const int* kf_pres() const { return (const int*)(scal() + ORD_SCAL); }
    vslam_status read_back(int K, hipStream_t stream) {      // the scalars and the keyframe membership of a count
        VS_HIP(hipMemcpyAsync(h_ordScal.p, O.scal, ORD_SCAL * sizeof(long long), hipMemcpyDeviceToHost, stream));
        VS_HIP(hipMemcpyAsync(h_ordScal.p + ORD_SCAL * sizeof(long long), O.kfPres, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, stream));
        VS_HIP(vslam::stream_wait_blocking(stream));
        return VSLAM_OK;
    }
};

}  // namespace
