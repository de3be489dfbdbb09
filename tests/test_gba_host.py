"""The host plan of vslam_global_ba (gtsam-vslam_amd/csrc/gba_host.hpp: presence, free set, block graph, reordering, gather lists),
built without a device as a stand-alone program under AddressSanitizer + UBSan (tests/native/gba_host.cpp) and compared with a
brute-force builder on the problems of tests/test_gpu_gba.py, and its refusals."""
import os
import subprocess
import tempfile
import numpy as np
import pytest
import gba_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, CAPACITY = 0, 1, 4


@pytest.fixture(scope="module")
def program():
    src = os.path.join(ROOT, "tests", "native", "gba_host.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gba_host")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "gtsam-vslam_amd", "csrc"), src, "-o", exe], check=True)
        yield exe


def run_native(exe, fixed, n_lm, pk, pl, pf, edges):
    words = [len(fixed)] + [int(v) for v in fixed] + [n_lm, len(pk)]
    for p in range(len(pk)):
        words += [int(pk[p]), int(pl[p]), int(pf[p])]
    words += [len(edges)] + [int(x) for e in edges for x in e[:2]]
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        f.write(" ".join(str(w) for w in words))
        f.flush()
        r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    head = lines[0].split(" ", 2)
    assert head[0] == "status"
    out = dict(status=int(head[1]), message=head[2] if len(head) > 2 else "", blocks={})
    for line in lines[1:]:
        name, *v = line.split()
        v = [int(x) for x in v]
        if name == "block":
            out["blocks"][(v[0], v[1])] = [(v[2 + 2 * q], v[3 + 2 * q]) for q in range((len(v) - 2) // 2)]
        else:
            out[name] = v
    return out


def brute(fixed, n_lm, pk, pl, pf, edges, pos):
    """everything the plan holds, from the definitions, given the plan's own numbering `pos` (checked to be a permutation)"""
    K, P = len(fixed), len(pk)
    nfac = [(pf[p] & 1) + ((pf[p] >> 1) & 1) for p in range(P)]
    fac = [sum(nfac[p] for p in range(P) if pl[p] == l) for l in range(n_lm)]
    present = [int(c >= 2) for c in fac]
    lm_pairs = [[p for p in range(P) if pl[p] == l and nfac[p] and present[l]] for l in range(n_lm)]
    tied = set(pk[p] for lst in lm_pairs for p in lst) | set(x for e in edges for x in e[:2])
    free = [k for k in range(K) if not fixed[k] and k in tied]
    iso = sum(1 for k in range(K) if not fixed[k] and k not in tied)
    assert sorted(pos[k] for k in free) == list(range(len(free))) and all(pos[k] == -1 for k in range(K) if k not in free)
    blocks = {}
    for l in range(n_lm):
        for p1 in lm_pairs[l]:
            for p2 in lm_pairs[l]:
                r, c = pos[pk[p1]], pos[pk[p2]]
                if r >= 0 and c >= 0 and c <= r:
                    blocks.setdefault((c, r - c), []).append((p1, p2))
    b = max([d for _, d in blocks] + [abs(pos[e[0]] - pos[e[1]]) for e in edges if pos[e[0]] >= 0 and pos[e[1]] >= 0] + [0])
    inc = [[] for _ in free]
    for n, e in enumerate(edges):
        for side in (0, 1):
            if pos[e[side]] >= 0:
                inc[pos[e[side]]].append(2 * n + side)
    return dict(present=present, lm_pairs=lm_pairs, nf=len(free), iso=iso, blocks=blocks, b=b, inc=inc,
                factors=sum(fac[l] for l in range(n_lm) if present[l]))


def compare(exe, prob, edges):
    fixed = [int(v) for v in prob["kf_fixed"]]
    pk, pl, pf = ([int(v) for v in prob[k]] for k in ("pair_kf", "pair_lm", "pair_flags"))
    n_lm = len(prob["lm"])
    got = run_native(exe, fixed, n_lm, pk, pl, pf, edges)
    assert got["status"] == OK, got["message"]
    want = brute(fixed, n_lm, pk, pl, pf, edges, got.get("pos", []))
    nf, iso, n_present, n_thin, n_fac, b, n_blk = got["counts"]
    assert (nf, iso, n_present, n_thin, n_fac, b) == (want["nf"], want["iso"], sum(want["present"]), n_lm - sum(want["present"]), want["factors"], want["b"])
    assert got.get("present", []) == want["present"]
    starts = got["lmStart"]
    assert [got.get("lmPairs", [])[starts[l]:starts[l + 1]] for l in range(n_lm)] == want["lm_pairs"]
    rows = got["rowStart"]
    assert [got.get("inc", [])[rows[c]:rows[c + 1]] for c in range(nf)] == want["inc"]
    assert got["blocks"] == want["blocks"] and n_blk == len(want["blocks"])
    assert list(got["blocks"]) == sorted(got["blocks"])              # numbered by (column, offset)
    S = gr.Structure(prob, edges, gr.INV_SIGMA)                       # the restatement's presence and free set are the plan's
    assert [int(v) for v in S.present] == want["present"] and len(S.free) == nf and S.n_isolated == iso
    return got


@pytest.mark.parametrize("name", list(gr.CASES))
def test_lists_of_the_cases(program, name):
    prob, edges = gr.CASES[name]()
    got = compare(program, prob, edges)
    if name == "dense12":
        assert got["counts"][5] == 11 and all(len(v) == 40 for v in got["blocks"].values()) and len(got["blocks"]) == 78
    if name == "long_list":
        assert len(got["blocks"][(0, 1)]) == 300
    if name == "no_shared":
        assert got["counts"][5] == 0
    if name == "chain172":
        assert got["counts"][0] == 172 and got["counts"][5] == 2
    if name == "chain260_loop":
        assert got["counts"][0] == 260 and got["counts"][5] <= 8


def test_duplicate_pairs_and_random_problems(program):
    """a (keyframe, landmark) pair listed twice fills the diagonal block with every ordered combination; random small problems"""
    prob = dict(kf_fixed=[1, 0, 0], lm=np.zeros((2, 3)), pair_kf=[0, 1, 1, 2, 1, 2], pair_lm=[0, 0, 0, 0, 1, 1], pair_flags=[3, 1, 2, 3, 3, 0],
                kf_pose=np.zeros((3, 4, 4)), pair_uv=np.zeros((6, 4), np.float32), pair_oct=np.zeros((6, 2), np.int32))
    got = compare(program, prob, [])
    c = got["pos"][1]
    assert sorted(got["blocks"][(c, 0)]) == [(1, 1), (1, 2), (2, 1), (2, 2), (4, 4)]
    rng = np.random.default_rng(5)
    for _ in range(25):
        K, L, P = int(rng.integers(2, 9)), int(rng.integers(1, 7)), int(rng.integers(0, 30))
        fixed = (rng.random(K) < 0.3).astype(int)
        fixed[0] = 1
        prob = dict(kf_fixed=fixed, lm=np.zeros((L, 3)), pair_kf=rng.integers(0, K, P), pair_lm=rng.integers(0, L, P), pair_flags=rng.integers(0, 4, P),
                    kf_pose=np.zeros((K, 4, 4)), pair_uv=np.zeros((P, 4), np.float32), pair_oct=np.zeros((P, 2), np.int32))
        edges = [(int(a), int(b)) for a, b in rng.integers(0, K, (int(rng.integers(0, 5)), 2)) if a != b]
        edges += [(0, k) for k in range(1, K)]                       # (every keyframe tied to the fixed keyframe 0: no free gauge)
        compare(program, prob, [(i, j, np.eye(4), 1.0, 1.0) for i, j in edges])


def test_refusals(program):
    run = lambda *a: run_native(program, *a)
    r = run([0, 0], 1, [0, 1], [0, 0], [3, 3], [])
    assert r["status"] == INVALID and "free gauge" in r["message"]
    r = run([1, 0, 0], 1, [0, 1], [0, 0], [3, 3], [])                # keyframe 2 is isolated, not a gauge problem
    assert r["status"] == OK and r["counts"][:2] == [1, 1]
    r = run([1, 0, 0, 0], 1, [0, 1], [0, 0], [3, 3], [(2, 3)])
    assert r["status"] == INVALID and "keyframe 2" in r["message"]
    r = run([1, 0], 1, [0, 1], [0, 0], [1, 0], [])                   # one factor: thin, nothing free
    assert r["status"] == OK and r["counts"][:4] == [0, 1, 0, 1]
    assert run([1, 0], 1, [0, 2], [0, 0], [3, 3], [])["status"] == INVALID
    assert run([1, 0], 1, [0, 1], [0, 1], [3, 3], [])["status"] == INVALID
    assert run([1, 0], 1, [0, 1], [0, 0], [3, 3], [(1, 1)])["status"] == INVALID
    assert run([1, 0], 1, [0, 1], [0, 0], [3, 3], [(0, 2)])["status"] == INVALID
    assert run([], 0, [], [], [], [])["status"] == INVALID
    r = run([1] + [0] * 16384, 0, [], [], [], [])
    assert r["status"] == CAPACITY and "keyframes" in r["message"]
    n = 4098
    r = run([1] + [0] * (n - 1), 1, list(range(n)), [0] * n, [3] * n, [])
    assert r["status"] == CAPACITY and "block lists" in r["message"]
    n = 601
    r = run([1] + [0] * (n - 1), 1, list(range(n)), [0] * n, [3] * n, [])
    assert r["status"] == CAPACITY and "band" in r["message"]
