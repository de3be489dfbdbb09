"""vslam_pose_graph_optimize / vslam_pose_graph_move_points against the numpy restatement (tests/pgo_ref.py) on the shapes where
the kernels can go wrong: one free pose, no free-free edge (b = 0), block columns / edges / incidence rows across 64 and 256,
a band as wide as the matrix, a chord that the reordering has to absorb, a long incidence row, the legal special cases and
every refusal.  Tolerances: 1e-7 absolute per pose entry (the closed-loop tests' pose tolerance; the graphs are a few metres
across), 1e-9 relative on the final cost, and the solver-independent stationarity |J^T W r|_inf <= 1e-6 of its initial value,
evaluated by the restatement on the device's result."""
import functools
import os
import numpy as np
import pytest
import pgo_ref as pr

pytestmark = pytest.mark.gpu


def hub_graph():
    return pr.star_graph(51, seed=13, hub_fixed=False)           # pose 0 free with 100 edges (two per neighbour), pose 1 fixed


def special_graph():
    poses, fixed, edges = pr.chain_graph(12, (2, 9), fixed_ids=(0, 5))
    poses = np.concatenate([poses, poses[-1:] @ pr.make_pose(np.eye(3), [1.0, 0, 0])])      # pose 12: free, no edge
    fixed = np.concatenate([fixed, [0]]).astype(np.uint8)
    edges = edges + [(0, 5, np.eye(4), 2.0, 3.0)] + edges[3:6] + [(8, 7, pr.rigid_inv(np.asarray(edges[7][2])), 0.5, 0.0)]
    return poses, fixed, edges


GRAPHS = {
    "one_free": lambda: pr.ring_graph(2, 2),
    "star": lambda: pr.star_graph(9),
    "ring8": lambda: pr.ring_graph(8, 8),
    "ring64": lambda: pr.ring_graph(64, 64),
    "ring65": lambda: pr.ring_graph(65, 65),
    "ring257": lambda: pr.ring_graph(257, 257),
    "complete12": pr.complete_graph,
    "chain300": lambda: pr.chain_graph(300, (3, 290)),
    "hub100": hub_graph,
    "special": special_graph,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(poses, fixed, edges, reference poses, reference report, initial gradient): computed once, never modified"""
    poses, fixed, edges = GRAPHS[name]()
    ref, rep = pr.optimize(poses, fixed, edges)
    for a in (poses, fixed, ref):
        a.setflags(write=False)
    return poses, fixed, edges, ref, rep, pr.gradient_inf(poses, fixed, edges)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_against_restatement(capi, name):
    poses, fixed, edges, ref, rrep, g0 = case(name)
    out, rep = capi.pose_graph_optimize(poses, fixed, edges)
    print(name, rep, "ref", rrep, "max pose diff", np.abs(out - ref).max(), "gradient", pr.gradient_inf(out, fixed, edges), "of", g0)
    assert rep["n_free"] == rrep["n_free"] and rep["n_isolated"] == rrep["n_isolated"]
    assert rep["iterations"] == rep["accepted"] + rep["rejected"] and 1 <= rep["accepted"] <= 20
    assert (rep["accepted"], rep["rejected"]) == (rrep["accepted"], rrep["rejected"])        # the same trials as the restatement
    assert abs(rep["initial_cost"] - rrep["initial_cost"]) <= 1e-9 * rrep["initial_cost"]
    assert np.abs(out - ref).max() <= 1e-7
    assert abs(rep["final_cost"] - rrep["final_cost"]) <= 1e-9 * rrep["final_cost"]
    assert pr.gradient_inf(out, fixed, edges) <= 1e-6 * g0
    free, _ = pr.free_poses(len(poses), fixed, edges)
    for k in range(len(poses)):
        if k not in free:
            assert out[k].tobytes() == poses[k].tobytes(), k         # fixed and isolated poses: not a bit
    # two calls on the same input return the same bytes
    out2, rep2 = capi.pose_graph_optimize(poses, fixed, edges)
    assert out2.tobytes() == out.tobytes() and rep2 == rep


def test_single_call_returns_recorded_bytes(capi):
    """The single call is the one-lane case of the batched solve; tests/golden/pgo_single.npz holds what the last single call
    with kernels and a host loop of its own returned (tests/golden/make_pgo_single.py says from which commit and how to
    re-record): every graph above, the singular ring, the exact graph, all poses fixed, max_iterations = 2 with lambda0 = 10,
    and the moved points of test_move_points.  Pose bytes and every report field are equal."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pgo_single.npz")) as z:
        gold = {k: z[k] for k in z.files}
    fields = [str(f) for f in gold["report_fields"]]
    assert fields == [f[0] for f in capi.PgoReport._fields_]
    names = [str(n) for n in gold["names"]]
    assert set(GRAPHS) < set(names) and len(names) == len(GRAPHS) + 4
    for name in names:
        g = lambda k: gold[name + "/" + k]
        out, rep = capi.pose_graph_optimize(g("poses"), g("fixed"), g("edges"), max_iterations=int(g("params")[0]), lambda0=float(g("params")[1]))
        want = dict(zip(fields[:6], (int(v) for v in g("report_int"))), **dict(zip(fields[6:], (float(v) for v in g("report_f64")))))
        print(name, rep)
        assert rep == want, name
        assert out.tobytes() == g("out").tobytes(), name
    for n in (1, 255, 257):
        g = lambda k: gold["move%d/%s" % (n, k)]
        assert capi.pose_graph_move_points(g("X"), g("ref"), g("A"), g("B")).tobytes() == g("out").tobytes(), n


def test_bandwidths(capi):
    # no free-free edge
    poses, fixed, edges, *_ = case("star")
    assert capi.pose_graph_optimize(poses, fixed, edges)[1]["half_bandwidth"] == 0
    assert capi.pose_graph_optimize(*case("one_free")[:3])[1]["half_bandwidth"] == 0
    # every pair of the 11 free poses shares an edge: the band is the whole matrix
    assert capi.pose_graph_optimize(*case("complete12")[:3])[1]["half_bandwidth"] == 10
    # the chain with the edge (3, 290): in pose order the band would be 287 blocks wide.  A breadth-first numbering from the
    # chain's end has at most 3 poses per level (the chain ahead, and both directions from pose 290 once pose 3 is reached);
    # an edge joins the same or neighbouring levels, so its ends are at most 3 + 3 - 1 = 5 positions apart
    rep = capi.pose_graph_optimize(*case("chain300")[:3])[1]
    assert rep["n_free"] == 299 and rep["half_bandwidth"] <= 5
    # the hub is a neighbour of each of the other 49 free poses: one of them is at least 25 positions away
    rep = capi.pose_graph_optimize(*case("hub100")[:3])[1]
    assert rep["n_free"] == 50 and rep["half_bandwidth"] >= 25


def test_special_cases(capi):
    poses, fixed, edges, ref, rrep, _ = case("special")
    out, rep = capi.pose_graph_optimize(poses, fixed, edges)
    assert rep["n_isolated"] == 1 and rep["n_free"] == 10
    fixed_cost = pr.cost(poses, [edges[12]])               # the edge between the fixed poses 0 and 5
    assert fixed_cost > 0.1 and rep["final_cost"] >= fixed_cost
    # duplicate edges add up: the list twice = the weights doubled
    e2 = [(i, j, Z, 2 * a, 2 * b) for (i, j, Z, a, b) in edges]
    o1, r1 = capi.pose_graph_optimize(poses, fixed, edges + edges)
    o2, r2 = capi.pose_graph_optimize(poses, fixed, e2)
    assert np.abs(o1 - o2).max() <= 1e-7 and abs(r1["final_cost"] - r2["final_cost"]) <= 1e-9 * r2["final_cost"]
    assert abs(r1["initial_cost"] - 2 * rep["initial_cost"]) <= 1e-9 * r1["initial_cost"]


def test_singular_system_is_rejected_until_lambda_runs_out(capi):
    """every edge of free pose 3 has zero weights: its diagonal block is exactly zero, the factorisation meets a pivot that is
    not positive (the dense solve: an exactly singular matrix) at every lambda - every trial is rejected, whatever its delta,
    until lambda passes 1e8: 1e-4 * 4^20 = 1.1e8 > 1e8 >= 1e-4 * 4^19, so 20 trials; nothing moves"""
    poses, fixed, edges, *_ = case("ring8")
    ez = [(i, j, Z, 0.0, 0.0) if 3 in (i, j) else (i, j, Z, a, b) for (i, j, Z, a, b) in edges]
    want, wrep = pr.optimize(poses, fixed, ez)
    out, rep = capi.pose_graph_optimize(poses, fixed, ez)
    assert (wrep["accepted"], wrep["rejected"]) == (0, 20) and (rep["accepted"], rep["rejected"], rep["iterations"]) == (0, 20, 20)
    assert out.tobytes() == poses.tobytes() and want.tobytes() == poses.tobytes()
    assert rep["final_cost"] == rep["initial_cost"] and abs(rep["final_lambda"] - wrep["final_lambda"]) <= 1e-12 * wrep["final_lambda"]


def test_exact_graph_and_all_fixed(capi):
    poses, fixed, edges = pr.exact_graph()
    out, rep = capi.pose_graph_optimize(poses, fixed, edges)
    assert rep["initial_cost"] <= 1e-20 and rep["iterations"] == 0 and out.tobytes() == poses.tobytes()
    poses, fixed, edges, *_ = case("ring8")
    out, rep = capi.pose_graph_optimize(poses, np.ones(8, np.uint8), edges)
    assert rep["n_free"] == 0 and rep["iterations"] == 0 and out.tobytes() == poses.tobytes()
    assert abs(rep["final_cost"] - pr.cost(poses, edges)) <= 1e-9 * rep["final_cost"]


def test_parameters(capi):
    poses, fixed, edges, ref, rrep, _ = case("ring8")
    out, rep = capi.pose_graph_optimize(poses, fixed, edges, max_iterations=2, lambda0=10.0)
    r2, rr2 = pr.optimize(poses, fixed, edges, max_iterations=2, lambda0=10.0)
    assert rep["accepted"] == 2 and rr2["accepted"] == 2 and rep["rejected"] == rr2["rejected"]
    assert np.abs(out - r2).max() <= 1e-7 and abs(rep["final_lambda"] - rr2["final_lambda"]) <= 1e-12 * rr2["final_lambda"]
    assert rep["final_cost"] > rrep["final_cost"]


def test_refusals(capi):
    poses, fixed, edges, *_ = case("ring8")
    I = np.eye(4)

    def status(p=poses, f=fixed, e=edges, **kw):
        with pytest.raises(capi.VslamError) as ex:
            capi.pose_graph_optimize(p, f, e, **kw)
        return ex.value.status

    assert status(e=edges + [(3, 3, I, 1.0, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(3, 8, I, 1.0, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(-1, 2, I, 1.0, 1.0)]) == capi.ERR_INVALID
    bad = poses.copy(); bad[4, 1, 3] = np.nan
    assert status(p=bad) == capi.ERR_INVALID
    Zi = I.copy(); Zi[0, 0] = np.inf
    assert status(e=edges + [(1, 2, Zi, 1.0, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(1, 2, I, np.nan, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(1, 2, I, -1.0, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(1, 2, I, 1.0, -1e-3)]) == capi.ERR_INVALID
    assert status(lambda0=-1.0) == capi.ERR_INVALID
    assert status(max_iterations=-1) == capi.ERR_INVALID
    # a free gauge: nothing fixed; and a second component that no edge ties to a fixed pose
    assert status(f=np.zeros(8, np.uint8)) == capi.ERR_INVALID
    p2 = np.concatenate([poses, poses[:2]]); f2 = np.concatenate([fixed, [0, 0]]).astype(np.uint8)
    assert status(p=p2, f=f2, e=edges + [(8, 9, I, 1.0, 1.0)]) == capi.ERR_INVALID
    # capacities: poses, edges, band blocks (a free hub tied to 1098 free poses: the band is as wide as the matrix)
    big = np.tile(I, (16385, 1, 1)); fb = np.zeros(16385, np.uint8); fb[0] = 1
    assert status(p=big, f=fb, e=[(0, 1, I, 1.0, 1.0)]) == capi.ERR_CAPACITY
    many = capi.pgo_edges([(0, 1, I, 1.0, 1.0)] * 2)
    many = np.tile(many, 131073)
    assert len(many) == 262146 and status(p=poses[:2], f=fixed[:2], e=many) == capi.ERR_CAPACITY
    hub = np.tile(I, (1100, 1, 1)); fh = np.zeros(1100, np.uint8); fh[1] = 1
    assert status(p=hub, f=fh, e=[(0, k, I, 1.0, 1.0) for k in range(1, 1100)]) == capi.ERR_CAPACITY


@pytest.mark.parametrize("n", [0, 1, 255, 257, 70000])
def test_move_points(capi, n):
    rng = np.random.default_rng(n)
    A = np.array([pr.random_pose(rng, 1.0, 3.0) for _ in range(7)])
    B = np.array([pr.random_pose(rng, 1.0, 3.0) for _ in range(7)])
    B[2] = A[2]                                              # a reference pose that did not move
    X = rng.uniform(-5, 5, (n, 3))
    ref = rng.integers(0, 7, n).astype(np.int32)
    if n > 1:
        ref[0] = 2; ref[-1] = -1
    Y = capi.pose_graph_move_points(X, ref, A, B)
    R = pr.move_points(X, ref, A, B) if n <= 257 else \
        np.where(ref[:, None] >= 0, np.einsum("kab,kb->ka", B[ref, :3, :3], np.einsum("kba,kb->ka", A[ref, :3, :3], X - A[ref, :3, 3])) + B[ref, :3, 3], X)
    assert Y.shape == (n, 3)
    if n:
        scale = np.abs(X).max() + np.abs(A[:, :3, 3]).max() + np.abs(B[:, :3, 3]).max()
        assert np.abs(Y - R).max() <= 1e-12 * scale
    if n > 1:
        assert np.abs(Y[0] - X[0]).max() <= 1e-12 * scale and Y[-1].tobytes() == X[-1].tobytes()
        with pytest.raises(capi.VslamError) as ex:
            capi.pose_graph_move_points(X, np.full(n, 7, np.int32), A, B)
        assert ex.value.status == capi.ERR_INVALID
