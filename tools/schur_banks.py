"""CPU model of the LDS bank conflicts of k_ba_schur2's two accumulation phases, for a synth.make_ba_problem shape and a layout of
the workgroup's LDS copy of the reduced system (numpy only, no GPU): what a layout costs can be priced before it is built.

usage: schur_banks.py [--max-views V] [--n-local F] [--n-fixed K] [--n-lm L] [--seed S] [--pitch P ...]

For every landmark (one wave) the lanes' addresses are enumerated from the problem's real slot tables, as the kernel forms them:
  blocks  lane 2 b + half owns rows 3 half .. 3 half + 2 of block b of the landmark's (slot, slot) pairs s1 <= s2, 32 blocks per
          pass; its 18 atomics are constant offsets from one base, so one instruction's pattern is every instruction's;
  Hpp     lane 6 f + i owns row i of factor f's Jp^T Jp (entries j >= i) and its right-hand-side entry, ten factors per pass;
          the left and the right factor of one keyframe add to the same addresses.
An LDS cycle serves one lane per bank position in each lane group; lanes on the same position serialise - identical addresses
too, since these are atomics.  The hardware guide has no row for the fp64 LDS atomic, so both candidate groupings are reported:
  w64  4 groups of 16 contiguous lanes, 16 positions of 8 bytes (as the 8-byte store),
  r64  2 groups of 32 lanes, 32 positions of 8 bytes (as the 8-byte load).
Printed: LDS cycles as a multiple of the conflict-free count (one cycle per group with an active lane).  A model, not a
measurement: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of the kernel (tools/pmc_cohort.sh) is the check."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gtsam-vslam_amd"))
import synth  # noqa: E402

GROUPINGS = {"w64": (16, 16), "r64": (32, 32)}      # lanes per group, 8-byte bank positions


def landmark_tables(prob):
    """per landmark: the free index of every factor (-1: fixed keyframe), sorted as the host sorts them"""
    fl = prob["pair_flags"].astype(np.int64) & 3
    on = fl != 0
    kf, lm, nfac = prob["pair_kf"][on], prob["pair_lm"][on], ((fl & 1) + (fl >> 1))[on]
    free = np.flatnonzero(prob["kf_fixed"] == 0)
    fidx = -np.ones(len(prob["kf_fixed"]), np.int64)
    fidx[free] = np.arange(len(free))
    out = {}
    for k, l, c in zip(kf, lm, nfac):
        out.setdefault(int(l), []).extend([int(fidx[k])] * int(c))
    return [np.sort(np.array(v)) for v in out.values()], len(free)


def block_ordinal(F, a, b):
    return a * (2 * F - a + 1) // 2 + (b - a)


class Layout:
    def __init__(self, kind, F, pitch=37):
        self.kind, self.F, self.n, self.pitch = kind, F, 6 * F, pitch
        self.ld = self.n + 1 if kind == "rowmajor+1" else self.n

    def block_base(self, a, b, half):
        if self.kind == "packed":
            return block_ordinal(self.F, a, b) * self.pitch + 18 * half
        return (6 * a + 3 * half) * self.ld + 6 * b

    def hpp(self, a, i, j):
        if self.kind == "packed":
            return block_ordinal(self.F, a, a) * self.pitch + 6 * i + j
        return (6 * a + i) * self.ld + 6 * a + j

    def rhs(self, a, i):
        base = block_ordinal(self.F, self.F - 1, self.F - 1) * self.pitch + self.pitch if self.kind == "packed" else self.ld * self.n
        return base + 6 * a + i

    def doubles(self):
        return self.rhs(self.F - 1, 5) + 1


def cycles(lanes, addrs, grouping):
    """LDS cycles of one wave-instruction and its conflict-free count; lanes / addrs: the active lanes and their 8-byte addresses"""
    per, pos = GROUPINGS[grouping]
    cyc = free = 0
    for g in np.unique(lanes // per):
        a = addrs[lanes // per == g]
        cyc += np.bincount(a % pos, minlength=pos).max()
        free += 1
    return cyc, free


def model(tables, lay, grouping):
    bc = bf = hc = hf = 0
    for ffi in tables:
        slots = np.unique(ffi[ffi >= 0])
        ns = len(slots)
        pairs = [(slots[s1], slots[s2]) for s1 in range(ns) for s2 in range(s1, ns)]
        for b0 in range(0, len(pairs), 32):
            chunk = pairs[b0:b0 + 32]
            lanes = np.arange(2 * len(chunk))
            addrs = np.array([lay.block_base(a, b, h) for (a, b) in chunk for h in (0, 1)])
            c, f = cycles(lanes, addrs, grouping)
            bc += 18 * c
            bf += 18 * f
        for f0 in range(0, len(ffi), 10):
            part = ffi[f0:f0 + 10]
            act = [(q, a) for q, a in enumerate(part) if a >= 0]
            if not act:
                continue
            for j in range(6):
                lanes = np.array([6 * q + i for q, a in act for i in range(j + 1)])
                addrs = np.array([lay.hpp(a, i, j) for q, a in act for i in range(j + 1)])
                c, f = cycles(lanes, addrs, grouping)
                hc += c
                hf += f
            lanes = np.array([6 * q + i for q, a in act for i in range(6)])
            addrs = np.array([lay.rhs(a, i) for q, a in act for i in range(6)])
            c, f = cycles(lanes, addrs, grouping)
            hc += c
            hf += f
    return bc / max(bf, 1), hc / max(hf, 1)


def main(argv):
    opt = {"--max-views": 12, "--n-local": 10, "--n-fixed": 4, "--n-lm": 1000, "--seed": 100}
    pitches = []
    k = 0
    while k < len(argv):
        if argv[k] == "--pitch":
            k += 1
            while k < len(argv) and not argv[k].startswith("--"):
                pitches.append(int(argv[k]))
                k += 1
            continue
        if argv[k] not in opt:
            sys.exit(__doc__)
        opt[argv[k]] = int(argv[k + 1])
        k += 2
    prob = synth.make_ba_problem(n_local=opt["--n-local"], n_fixed=opt["--n-fixed"], n_lm=opt["--n-lm"], seed=opt["--seed"],
                                 max_views=opt["--max-views"])
    tables, F = landmark_tables(prob)
    nfac = np.array([len(t) for t in tables])
    nsl = np.array([len(np.unique(t[t >= 0])) for t in tables])
    print("max_views %d: %d landmarks, F = %d | per landmark: %.1f factors, %.1f slots, sum k^2 = %.1f"
          % (opt["--max-views"], len(tables), F, nfac.mean(), nsl.mean(), (nsl * (nsl + 1) / 2).mean()))
    lays = [Layout("rowmajor", F), Layout("rowmajor+1", F)] + [Layout("packed", F, p) for p in (pitches or [37])]
    print("%-22s %8s | %-13s | %-13s" % ("layout", "doubles", "blocks w64/r64", "Hpp w64/r64"))
    for lay in lays:
        r = {g: model(tables, lay, g) for g in GROUPINGS}
        name = lay.kind + (" pitch %d" % lay.pitch if lay.kind == "packed" else "")
        print("%-22s %8d | x%.2f / x%.2f | x%.2f / x%.2f" % (name, lay.doubles(), r["w64"][0], r["r64"][0], r["w64"][1], r["r64"][1]))


if __name__ == "__main__":
    main(sys.argv[1:])
