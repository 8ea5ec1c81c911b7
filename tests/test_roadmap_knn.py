"""Nearest-neighbour search over a roadmap's nodes (include/armour_hip.h armour_roadmap_knn / armour_roadmap_knn_host, Roadmap.knn,
device_roadmap).

The rule is restated below in numpy: the wrapped distance accumulated joint by joint (test_roadmap_field.wrapped_len), the candidates by
mask, exclusion and radius, and the order by lexsort on (index, distance).  The order is total, so the result is unique and everything is
held to bit equality: the host entry against numpy on the CPU, the device against the host entry on the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_roadmap import _limits, _reference_obstacles, _robot
from test_roadmap_field import wrapped_len

I32, DP = C.POINTER(C.c_int32), C.POINTER(C.c_double)


# ----------------------------------------------------------------------------------------------------------- restatement
def knn_np(nodes, queries, cont, k, radius=np.inf, exclude=None, free=None):
    """(index [Q,k], dist [Q,k], count [Q]) by the header's rule; free [Q,N] bool (None: every node), exclude [Q] (None or -1: none)."""
    Q, N = queries.shape[0], nodes.shape[0]
    index, dist, count = np.full((Q, k), -1, dtype=np.int32), np.full((Q, k), np.inf), np.zeros(Q, dtype=np.int32)
    for i in range(Q):
        d = wrapped_len(queries[i][None], nodes, cont)
        cand = d <= radius
        if exclude is not None and 0 <= exclude[i] < N:
            cand[exclude[i]] = False
        if free is not None:
            cand &= free[i]
        idx = np.flatnonzero(cand)
        first = idx[np.lexsort((idx, d[idx]))[:k]]
        index[i, :first.size], dist[i, :first.size], count[i] = first, d[first], first.size
    return index, dist, count


def same(got, want):
    """index and count equal, dist bitwise (infinities in the padding included)"""
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64)) and np.array_equal(got[2], want[2])


def _nodes(robot, N, seed):
    lb, ub, cont = _limits(robot)
    return lb + (ub - lb) * np.random.default_rng(seed).random((N, robot.num_factors)), cont


def _bare(robot, nodes, cont, host):
    from armour_amd.roadmap import Roadmap
    return Roadmap(robot, nodes, np.zeros((0, 2), dtype=np.int32), continuous=cont.astype(np.uint8), host=host)


# ----------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_host_entry_equals_the_numpy_restatement(name):
    robot = _robot(name)
    nodes, cont = _nodes(robot, 500, 3)
    queries, _ = _nodes(robot, 40, 4)
    queries[:5] = nodes[10:15]                                       # queries that are nodes: distance 0 to themselves
    rm = _bare(robot, nodes, cont, host=True)
    excl = np.where(np.arange(40) < 5, np.arange(10, 50), -1).astype(np.int32)
    for k in (1, 8, 64):
        for radius in (np.inf, 2.5):
            for ex in (None, excl):
                got = rm.knn(queries, k, radius=radius, exclude=ex, host=True)
                assert same(got, knn_np(nodes, queries, cont, k, radius, ex)), (name, k, radius, ex is not None)
    got = rm.knn(queries, 8, radius=2.5, host=True)
    assert got[2].min() < 8 and got[2].max() == 8                    # the radius cuts some lists short and not others
    assert np.array_equal(rm.knn(queries, 1, host=True)[0][:5, 0], np.arange(10, 15))
    assert not np.array_equal(rm.knn(queries, 1, exclude=excl, host=True)[0][:5, 0], np.arange(10, 15))
    rm.close()


def test_host_entry_at_the_edges_of_its_shapes():
    robot = _robot("kinova")
    nodes, cont = _nodes(robot, 90, 7)
    assert cont.any() and not cont.all()
    queries, _ = _nodes(robot, 6, 8)
    # one node; k above N; k = 64; one query
    one = _bare(robot, nodes[:1], cont, host=True)
    for k in (1, 64):
        got = one.knn(queries, k, host=True)
        assert same(got, knn_np(nodes[:1], queries, cont, k)) and (got[2] == 1).all() and (got[0][:, 1:] == -1).all() and np.isinf(got[1][:, 1:]).all()
    assert (one.knn(queries[:1], 3, exclude=[0], host=True)[2] == 0).all()
    one.close()
    rm = _bare(robot, nodes[:40], cont, host=True)
    got = rm.knn(queries[:1], 64, host=True)
    assert same(got, knn_np(nodes[:40], queries[:1], cont, 64)) and got[2][0] == 40
    rm.close()
    # every node twice: equal distances, the smaller index first
    twice = np.repeat(nodes, 2, axis=0)
    rm = _bare(robot, twice, cont, host=True)
    got = rm.knn(queries, 8, host=True)
    assert same(got, knn_np(twice, queries, cont, 8))
    assert (got[0][:, 0::2] % 2 == 0).all() and np.array_equal(got[0][:, 1::2], got[0][:, 0::2] + 1) and np.array_equal(got[1][:, 0::2], got[1][:, 1::2])
    rm.close()
    # +-pi on the continuous joints: -pi and pi are one angle (distance 0), and the wrap of a difference of exactly pi
    edge = np.zeros((4, 7))
    edge[0, cont], edge[1, cont], edge[3, cont] = np.pi, -np.pi, np.pi
    edge[3, ~cont] = 0.25
    rm = _bare(robot, edge, cont, host=True)
    q = edge.copy()
    got = rm.knn(q, 4, host=True)
    assert same(got, knn_np(edge, q, cont, 4))
    assert np.array_equal(got[0][0][:2], [0, 1]) and np.array_equal(got[1][0][:2], [0.0, 0.0]) and np.array_equal(got[0][1][:2], [0, 1])
    # a radius that equals a distance exactly takes the node (<=), the next double below does not
    d = got[1][2]
    assert 0 < d[1] < d[3]
    assert rm.knn(q[2:3], 4, radius=d[1], host=True)[2][0] == int((d <= d[1]).sum())
    assert rm.knn(q[2:3], 4, radius=np.nextafter(d[1], 0), host=True)[2][0] == int((d < d[1]).sum())
    assert same(rm.knn(q[2:3], 4, radius=0.0, host=True), knn_np(edge, q[2:3], cont, 4, 0.0))
    rm.close()


def test_argument_and_state_rules_of_the_host_entry():
    from armour_amd import _lib
    L = _lib.load()
    robot = _robot("kinova")
    nodes, cont = _nodes(robot, 20, 1)
    rm = _bare(robot, nodes, cont, host=True)
    q = np.ascontiguousarray(nodes[:3])

    def call(fn, h, Q, queries, mask, k, radius):
        index, dist, count = np.full((3, 64), 77, dtype=np.int32), np.full((3, 64), 77.0), np.full(3, 77, dtype=np.int32)
        m = None if mask is None else np.asarray(mask, dtype=np.int32)
        rc = fn(h, Q, queries.ctypes.data_as(DP), None if m is None else m.ctypes.data_as(I32), None, k, radius, index.ctypes.data_as(I32),
                dist.ctypes.data_as(DP), count.ctypes.data_as(I32), None)
        untouched = (index == 77).all() and (dist == 77.0).all() and (count == 77).all()
        return rc, untouched

    host = L.armour_roadmap_knn_host
    assert call(host, rm.h, 3, q, None, 8, np.inf) == (_lib.OK, False)
    for k in (0, -1, 65):
        assert call(host, rm.h, 3, q, None, k, np.inf) == (_lib.EINVAL, True), k
    assert call(host, rm.h, 3, q, None, 64, np.inf)[0] == _lib.OK
    assert call(host, rm.h, 0, q, None, 8, np.inf) == (_lib.OK, True)              # Q = 0: nothing written
    assert call(host, rm.h, -1, q, None, 8, np.inf) == (_lib.EINVAL, True)
    for radius in (-1e-300, -np.inf, np.nan):
        assert call(host, rm.h, 3, q, None, 8, radius) == (_lib.EINVAL, True), radius
    assert call(host, rm.h, 3, q, None, 8, 0.0)[0] == _lib.OK
    for bad in (np.nan, np.inf):
        qq = q.copy()
        qq[2, 6] = bad
        assert call(host, rm.h, 3, qq, None, 8, np.inf) == (_lib.EINVAL, True)
    assert call(host, rm.h, 3, q, [-1, -1, -5], 8, np.inf)[0] == _lib.OK           # negative rows: no mask
    assert call(host, rm.h, 3, q, [-1, 0, -1], 8, np.inf) == (_lib.ESTATE, True)   # a world before any check
    assert call(host, None, 3, q, None, 8, np.inf) == (_lib.EINVAL, True)
    # a host handle serves the host entry alone
    assert call(L.armour_roadmap_knn, rm.h, 3, q, None, 8, np.inf) == (_lib.EDEVICE, True)
    assert call(L.armour_roadmap_knn, rm.h, 3, q, None, 0, np.inf) == (_lib.EINVAL, True)
    with pytest.raises(_lib.ArmourError) as ei:
        rm.check(np.zeros((1, 1, 12)))
    assert ei.value.code == _lib.EDEVICE
    rm.close()
    empty = _bare(robot, np.zeros((0, 7)), cont, host=True)                        # N = 0: nothing written
    assert call(host, empty.h, 3, q, None, 8, np.inf) == (_lib.OK, True)
    empty.close()


def test_the_search_constants_and_names_match_the_header():
    from armour_amd import _lib, roadmap
    text = open(os.path.join(ROOT, "include", "armour_hip.h")).read()
    assert int(re.search(r"#define ARMOUR_ROADMAP_KNN_MAX (\d+)", text).group(1)) == _lib.ROADMAP_KNN_MAX == 64
    assert int(re.search(r"#define ARMOUR_ROADMAP_KNN_MANY (\d+)", text).group(1)) == _lib.ROADMAP_KNN_MANY
    L = _lib.load()
    for name in ("armour_roadmap_knn", "armour_roadmap_knn_host", "armour_roadmap_create_host", "armour_roadmap_connect_batch", "armour_roadmap_descend_batch"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("knn", "connect_many", "descend_many"):
        assert hasattr(roadmap.Roadmap, name)
    assert hasattr(roadmap, "device_roadmap")


# ----------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def kinova():
    return _robot("kinova")


def _queries(robot, nodes, Q, seed):
    """Q queries: the nodes themselves (each excluding itself) when Q is their number, else random configurations"""
    if Q == nodes.shape[0] and Q > 1:
        return nodes, np.arange(Q, dtype=np.int32)
    return _nodes(robot, Q, seed)[0], None


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1023, 1025, 5000])
def test_device_equals_host_bit_for_bit(kinova, N):
    """Both launch shapes (a block per (query, 256 nodes) below ROADMAP_KNN_MANY queries, a lane per query with up to 16 slices of the nodes
    from there on) and every merge: one tile and several, a last tile of 1, 255 and 256 nodes, slices of unequal length."""
    nodes, cont = _nodes(kinova, N, 100 + N)
    rm = _bare(kinova, nodes, cont, host=False)
    for Q in sorted({1, 3, 64, 65, N}):
        queries, excl = _queries(kinova, nodes, Q, 200 + Q)
        for k in (1, 8, 64):
            radius = np.inf if k != 8 else 3.0
            got = rm.knn(queries, k, radius=radius, exclude=excl)
            want = rm.knn(queries, k, radius=radius, exclude=excl, host=True)
            assert same(got, want), (N, Q, k)
            assert want[2].max() == min(k, N - (excl is not None)) or radius < np.inf
    rm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N, Q", [(65, 2047), (65, 2048), (300, 2048), (700, 2100), (65, 131072)])
def test_device_equals_host_where_the_launch_shape_changes(kinova, N, Q):
    """One query short of the lane-per-query shape and the first with it (2 slices of 33 and 32 nodes; 5 slices of 60; 11 of 64 with a last
    block of 52 lanes), and queries enough for a single slice, whose merge has one list."""
    from armour_amd import _lib
    assert _lib.ROADMAP_KNN_MANY == 2048
    nodes, cont = _nodes(kinova, N, 300 + N)
    queries, _ = _nodes(kinova, Q, 400 + Q)
    rm = _bare(kinova, nodes, cont, host=False)
    for k, radius in ((8, np.inf), (64, 3.5)):
        assert same(rm.knn(queries, k, radius=radius), rm.knn(queries, k, radius=radius, host=True)), (N, Q, k)
    rm.close()


@pytest.fixture(scope="module")
def masked(kinova):
    """An edge-less roadmap of 700 nodes, each twice, checked against a world that leaves no node free and four reference worlds, with its
    self masks computed; queries for both launch shapes with rows that mix the worlds and -1."""
    nodes, cont = _nodes(kinova, 700, 21)
    nodes = np.repeat(nodes, 2, axis=0)
    rm = _bare(kinova, nodes, cont, host=False)
    obs = _reference_obstacles()["obstacles"][:4]
    wall = np.tile(np.array([0, 0, 0, 5.0, 0, 0, 0, 5.0, 0, 0, 0, 5.0]), (obs.shape[1], 1))     # the arm is inside it everywhere
    v = rm.check(np.concatenate([wall[None], obs]))
    s = rm.check_self()
    assert not v["node_free"][0].any() and all(0 < v["node_free"][w].sum() < 1400 for w in range(1, 5)) and 0 < s["node_free"].sum() < 1400
    yield dict(rm=rm, nodes=nodes, cont=cont, world=v["node_free"], self_=s["node_free"])
    rm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("Q", [70, 2100])
def test_masks_duplicates_and_an_empty_world(kinova, masked, Q):
    rm, nodes, cont = masked["rm"], masked["nodes"], masked["cont"]
    queries, _ = _nodes(kinova, Q, 30 + Q)
    rows = (np.arange(Q) % 6 - 1).astype(np.int32)                   # -1, 0 (nothing free), 1 .. 4
    for self_on in (False, True):
        rm.use_self(self_on)
        free = np.ones((Q, nodes.shape[0]), dtype=bool)
        for i in range(Q):
            if rows[i] >= 0:
                free[i] = masked["world"][rows[i]] & (masked["self_"] if self_on else True)
        got = rm.knn(queries, 8, worlds=rows, radius=4.0)
        assert same(got, rm.knn(queries, 8, worlds=rows, radius=4.0, host=True)), (Q, self_on)
        if Q == 70:
            assert same(got, knn_np(nodes, queries, cont, 8, 4.0, None, free)), self_on
        empty = rows == 0
        assert (got[2][empty] == 0).all() and (got[0][empty] == -1).all() and np.isinf(got[1][empty]).all()      # count 0, the padding intact
        assert (got[2][~empty] > 0).all() and all(free[i, got[0][i, :got[2][i]]].all() for i in range(Q))
        plain = np.flatnonzero(rows == -1)
        assert np.array_equal(got[0][plain, 1], got[0][plain, 0] + 1) and (got[0][plain, 0] % 2 == 0).all()      # a node, then its twin
        keep = got
    rm.use_self(False)
    assert not same(keep, rm.knn(queries, 8, worlds=rows, radius=4.0))                                           # the self mask took nodes away


@pytest.mark.gpu
def test_a_batch_of_queries_equals_one_query_at_a_time(kinova, masked):
    """A query's result does not depend on what shares its call -- nor on the launch shape: a one-query call takes a block per tile, the
    2100-query call a lane per query."""
    from armour_amd import _lib
    L = _lib.load()
    rm, nodes = masked["rm"], masked["nodes"]
    queries, _ = _nodes(kinova, 2100, 77)
    rows = (np.arange(2100) % 6 - 1).astype(np.int32)
    many = rm.knn(queries, 8, worlds=rows)
    few = rm.knn(queries[:9], 8, worlds=rows[:9])
    for i in range(9):
        one = rm.knn(queries[i], 8, worlds=rows[i:i + 1])
        for got in (many, few):
            assert same(one, tuple(a[i:i + 1] for a in got)), i
    # the state rules that need a check: a world past the last check's is EINVAL for both entries
    for host in (False, True):
        with pytest.raises(_lib.ArmourError) as ei:
            rm.knn(queries[:2], 8, worlds=[0, 5], host=host)
        assert ei.value.code == _lib.EINVAL
    fresh = _bare(kinova, nodes[:10], masked["cont"], host=False)
    with pytest.raises(_lib.ArmourError) as ei:
        fresh.knn(queries[:2], 8, worlds=[-1, 0])
    assert ei.value.code == _lib.ESTATE
    assert fresh.knn(queries[:2], 8, worlds=[-1, -1])[2].tolist() == [8, 8]
    fresh.close()


@pytest.mark.gpu
def test_device_roadmap_equals_uniform_roadmap(kinova):
    """Same nodes, exactly the same edges (at 7 joints numpy's sum over the joints is sequential, so the host builder's distances are the
    library's)."""
    from armour_amd.roadmap import device_roadmap, uniform_roadmap
    lb, ub, cont = _limits(kinova)
    n0, e0 = uniform_roadmap(3000, 1.5, 16, 6, lb, ub, cont)
    n1, e1 = device_roadmap(kinova, 3000, 1.5, 16, 6, lb, ub, cont)
    assert np.array_equal(n0, n1) and e1.dtype == np.int32 and np.array_equal(e0, e1)
    assert e0.shape[0] > 100                                        # (the bar of test_roadmap.py for its 600-node roadmap)
