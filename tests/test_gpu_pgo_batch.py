"""vslam_pose_graph_optimize_batch against the rule that defines it: a lane's poses and report are, byte for byte, what
vslam_pose_graph_optimize returns for that graph alone with the same parameters - whatever the other lanes are, in whatever
order, however many.  The lanes of the main case differ in n, m, band width (0 to >= 25) and trial counts (0 to 20), so that
most rounds run with lanes that have already stopped; m = 257 and n = 257 cross the 256-thread boundaries.  The C entry point is
called directly (ctypes), because the tests put sentinel bytes into every output and report to see what a call did NOT write."""
import ctypes as C
import functools
import numpy as np
import pytest
import pgo_ref as pr

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def hub_graph():
    return pr.star_graph(51, seed=13, hub_fixed=False)           # pose 0 free with 100 edges (two per neighbour), pose 1 fixed


def special_graph():
    poses, fixed, edges = pr.chain_graph(12, (2, 9), fixed_ids=(0, 5))
    poses = np.concatenate([poses, poses[-1:] @ pr.make_pose(np.eye(3), [1.0, 0, 0])])      # pose 12: free, no edge
    fixed = np.concatenate([fixed, [0]]).astype(np.uint8)
    edges = edges + [(0, 5, np.eye(4), 2.0, 3.0)] + edges[3:6] + [(8, 7, pr.rigid_inv(np.asarray(edges[7][2])), 0.5, 0.0)]
    return poses, fixed, edges


def ring8_all_fixed():
    poses, fixed, edges = pr.ring_graph(8, 8)
    return poses, np.ones(8, np.uint8), edges


def ring8_singular():
    poses, fixed, edges = pr.ring_graph(8, 8)
    return poses, fixed, [(i, j, Z, 0.0, 0.0) if 3 in (i, j) else (i, j, Z, a, b) for (i, j, Z, a, b) in edges]


GRAPHS = {
    "one_free": lambda: pr.ring_graph(2, 2),
    "ring257": lambda: pr.ring_graph(257, 257),
    "star": lambda: pr.star_graph(9),
    "hub100": hub_graph,
    "exact": pr.exact_graph,
    "ring8_all_fixed": ring8_all_fixed,
    "ring8_singular": ring8_singular,
    "complete12": pr.complete_graph,
    "chain300": lambda: pr.chain_graph(300, (3, 290)),
    "special": special_graph,
    "ring65": lambda: pr.ring_graph(65, 65),
    "ring64": lambda: pr.ring_graph(64, 64),
    "ring8": lambda: pr.ring_graph(8, 8),
}
MIX = ["one_free", "ring257", None, "star", "hub100", "exact", "ring8_all_fixed", "ring8_singular", "complete12", "chain300",
       "special", "ring65", "ring64"]


def _arrays(capi, graph):
    poses, fixed, edges = graph
    return (np.ascontiguousarray(poses, np.float64).reshape(-1, 4, 4), np.ascontiguousarray(fixed, np.uint8),
            edges if isinstance(edges, np.ndarray) else capi.pgo_edges(edges), len(edges))


@functools.lru_cache(maxsize=None)
def graph(name):
    import vslam_capi
    g = _arrays(vslam_capi, GRAPHS[name]())
    for a in g[:3]:
        a.setflags(write=False)
    return g


_SINGLE = {}


def single(capi, g, key, **params):
    """(bytes of the poses, report dict) of the single call: computed once per graph and parameter set"""
    key = (key, tuple(sorted(params.items())))
    if key not in _SINGLE:
        out, rep = capi.pose_graph_optimize(g[0], g[1], g[2] if g[3] else [], **params)
        _SINGLE[key] = (out.tobytes(), rep)
    return _SINGLE[key]


def call_batch(capi, lanes, n_lanes=None, inplace=(), **params):
    """lanes: (poses, fixed, edge array, m) or None per lane.  Every output and report starts as sentinel bytes.
    Returns (status, [output bytes], [report dict or None where the report still holds the sentinel])."""
    B = len(lanes)
    tab = (capi.PgoGraph * max(B, 1))()
    reps = (capi.PgoReport * max(B, 1))()
    C.memset(reps, SENTINEL, C.sizeof(reps))
    outs = []
    for k, g in enumerate(lanes):
        if g is None:
            outs.append(np.full(16 * 8, SENTINEL, np.uint8))
            tab[k] = capi.PgoGraph(None, None, 0, None, 0, outs[k].ctypes.data)
            continue
        if k in inplace:
            outs.append(g[0].copy())
            tab[k] = capi.PgoGraph(outs[k].ctypes.data, g[1].ctypes.data, len(g[0]), g[2].ctypes.data, g[3], outs[k].ctypes.data)
        else:
            outs.append(np.full(g[0].nbytes, SENTINEL, np.uint8))
            tab[k] = capi.PgoGraph(g[0].ctypes.data, g[1].ctypes.data, len(g[0]), g[2].ctypes.data, g[3], outs[k].ctypes.data)
    prm = capi.PgoParams(int(params.get("max_iterations", 0)), float(params.get("lambda0", 0.0)))
    st = capi.lib().vslam_pose_graph_optimize_batch(tab, B if n_lanes is None else n_lanes, C.byref(prm), 0, reps)
    sentinel_rep = bytes([SENTINEL]) * C.sizeof(capi.PgoReport)
    rd = [None if bytes(reps[k]) == sentinel_rep else capi._pgo_report_dict(reps[k]) for k in range(B)]
    return st, [o.tobytes() for o in outs], rd


def untouched(out_bytes):
    return out_bytes == bytes([SENTINEL]) * len(out_bytes)


@functools.lru_cache(maxsize=None)
def mix_result():
    import vslam_capi
    return call_batch(vslam_capi, [None if nm is None else graph(nm) for nm in MIX])


def test_lane_equals_single_call_bitwise(capi):
    st, outs, reps = mix_result()
    assert st == capi.OK, capi.lib().vslam_last_error()
    its = []
    for k, nm in enumerate(MIX):
        if nm is None:
            assert untouched(outs[k]) and reps[k] is None          # the idle lane: neither output nor report written
            continue
        want, wrep = single(capi, graph(nm), nm)
        print(nm, reps[k])
        assert reps[k] == wrep, nm
        assert outs[k] == want, nm
        its.append(reps[k]["iterations"])
    bands = [r["half_bandwidth"] for r in reps if r]
    assert min(bands) == 0 and max(bands) >= 25
    # the mix really runs rounds in which some lanes have stopped: one lane needs 20 rounds, another stops before round 5
    assert max(its) >= 20 and min(its) < 5 and any(1 <= i < 5 for i in its), its
    assert reps[MIX.index("ring8_singular")]["rejected"] == 20 and reps[MIX.index("exact")]["iterations"] == 0
    assert reps[MIX.index("ring8_all_fixed")]["n_free"] == 0
    # the same call twice returns the same bytes
    st2, outs2, reps2 = call_batch(capi, [None if nm is None else graph(nm) for nm in MIX])
    assert st2 == capi.OK and outs2 == outs and reps2 == reps


def test_order_and_company_do_not_matter(capi):
    st0, outs0, reps0 = mix_result()
    st, outs, reps = call_batch(capi, [None if nm is None else graph(nm) for nm in MIX[::-1]])
    assert st == capi.OK and outs == outs0[::-1] and reps == reps0[::-1]
    st, outs, reps = call_batch(capi, [graph("ring64")])
    k = MIX.index("ring64")
    assert st == capi.OK and outs[0] == outs0[k] and reps[0] == reps0[k]


def test_more_lanes_than_a_wave(capi):
    makers = [lambda s: pr.ring_graph(8, s), lambda s: pr.star_graph(9, seed=s), lambda s: pr.ring_graph(2, s)]
    lanes = [_arrays(capi, makers[s % 3](s)) for s in range(70)]
    st, outs, reps = call_batch(capi, lanes)
    assert st == capi.OK, capi.lib().vslam_last_error()
    for s, g in enumerate(lanes):
        want, wrep = single(capi, g, ("seeded", s))
        assert reps[s] == wrep and outs[s] == want, s
    assert len({r["iterations"] for r in reps}) > 1


def test_in_place_output_and_parameters(capi):
    names = ["ring8", "star", "ring65"]
    st, outs, reps = call_batch(capi, [graph(nm) for nm in names], inplace=(0, 2), max_iterations=2, lambda0=10.0)
    assert st == capi.OK, capi.lib().vslam_last_error()
    for k, nm in enumerate(names):
        want, wrep = single(capi, graph(nm), nm, max_iterations=2, lambda0=10.0)
        assert reps[k] == wrep and outs[k] == want, nm
    assert reps[0]["accepted"] == 2
    assert outs[0] != single(capi, graph("ring8"), "ring8")[0]        # (the parameters did apply)


def test_refusals(capi):
    I = np.eye(4)
    ring = graph("ring8")
    poses, fixed, edges = pr.ring_graph(8, 8)

    def refused(lanes, want, names_lane=None, **kw):
        st, outs, reps = call_batch(capi, lanes, **kw)
        msg = capi.lib().vslam_last_error().decode()
        assert st == want, (st, msg)
        assert all(untouched(o) for o in outs) and all(r is None for r in reps)        # nothing written in any lane
        if names_lane is not None:
            assert "lane %d" % names_lane in msg, msg

    def lanes_with(bad):
        return [ring, graph("star"), _arrays(capi, bad), graph("one_free")]

    refused(lanes_with((poses, fixed, edges + [(3, 8, I, 1.0, 1.0)])), capi.ERR_INVALID, 2)          # a bad edge index
    refused(lanes_with((poses, np.zeros(8, np.uint8), edges)), capi.ERR_INVALID, 2)                  # a free gauge
    bad = poses.copy(); bad[4, 1, 3] = np.nan
    refused(lanes_with((bad, fixed, edges)), capi.ERR_INVALID, 2)                                    # a non-finite pose
    refused(lanes_with((poses, fixed, edges + [(1, 2, I, -1.0, 1.0)])), capi.ERR_INVALID, 2)         # a negative weight
    refused([ring, ring], capi.ERR_INVALID, n_lanes=0)
    refused([ring], capi.ERR_INVALID, lambda0=-1.0)
    refused([ring] + [None] * 1024, capi.ERR_CAPACITY)                                               # 1025 lanes
    big = np.tile(I, (16385, 1, 1)); fb = np.ones(16385, np.uint8)
    refused([ring, (big, fb, capi.pgo_edges([]), 0)], capi.ERR_CAPACITY, 1)                          # a lane beyond the single call's limit
    # the call-wide pose count: 17 lanes of 16384 fixed poses without edges (16 of them are exactly the limit and pass)
    full = (np.tile(I, (16384, 1, 1)), np.ones(16384, np.uint8), capi.pgo_edges([]), 0)
    B = 17
    tab = (capi.PgoGraph * B)()
    reps = (capi.PgoReport * B)()
    C.memset(reps, SENTINEL, C.sizeof(reps))
    out = np.full(full[0].nbytes, SENTINEL, np.uint8)              # (one output shared by all lanes: it must not be written)
    for k in range(B):
        tab[k] = capi.PgoGraph(full[0].ctypes.data, full[1].ctypes.data, 16384, None, 0, out.ctypes.data)
    assert capi.lib().vslam_pose_graph_optimize_batch(tab, B, None, 0, reps) == capi.ERR_CAPACITY
    assert untouched(out.tobytes()) and bytes(reps) == bytes([SENTINEL]) * C.sizeof(reps)
    assert capi.lib().vslam_pose_graph_optimize_batch(tab, 16, None, 0, reps) == capi.OK
    assert out.tobytes() == full[0].tobytes() and reps[15].n_free == 0 and reps[15].iterations == 0
    assert bytes(reps[16]) == bytes([SENTINEL]) * C.sizeof(capi.PgoReport)


def test_python_binding(capi):
    res = capi.pose_graph_optimize_batch([GRAPHS["ring8"](), None, GRAPHS["star"]()])
    assert res[1] is None
    for r, nm in ((res[0], "ring8"), (res[2], "star")):
        want, wrep = single(capi, graph(nm), nm)
        assert r[0].tobytes() == want and r[1] == wrep
