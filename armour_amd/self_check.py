"""Self-collision checks: the arm's link boxes against each other on the MI355X (include/armour_hip.h, armour_self_*).

    res = check(robot, q)                                  # q [N,n] -> SelfResult: free [N] bool, worst_pair [N] (a*J + b, -1: free)
    res = check(robot, q, clearance=True)                  # + clearance [N]; worst_pair = the pair of the minimum
    shrink = calibrate_shrink(robot, known_good_configs)   # [J,J]: the smallest per-pair shrink that clears them
    check(robot, q, shrink=shrink)

The link boxes are the roadmap node rule's; they are bounding boxes and coarser than the arm, so adjacent links are never paired
(`default_pairs`: b - a >= 2) and a pair that overlaps at configurations known to be fine is discounted with `shrink`.  `host=True` runs
the library's host twin of the same rule (no GPU needed; for tests).  Roadmaps: Roadmap.check_self / use_self; executed pieces:
path_audit.audit_self.  The rule and its motion bound are stated in include/armour_hip.h and DESIGN.md.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import _dp, check as _check

_u8 = C.POINTER(C.c_uint8)


def table_args(robot, pairs, shrink):
    """(pairs [J,J] uint8 or None, shrink [J,J] float64 or None) as contiguous arrays, and their ctypes pointers."""
    J = robot.num_joints
    pairs = None if pairs is None else np.ascontiguousarray(np.asarray(pairs).astype(np.uint8).reshape(J, J))
    shrink = None if shrink is None else np.ascontiguousarray(np.asarray(shrink, dtype=np.float64).reshape(J, J))
    return pairs, shrink, (None if pairs is None else pairs.ctypes.data_as(_u8)), _dp(shrink)


def default_pairs(robot):
    """[J,J] uint8: 1 where b - a >= 2 (armour_self_pairs_default)."""
    J = robot.num_joints
    out = np.zeros((J, J), dtype=np.uint8)
    _check(_lib.load().armour_self_pairs_default(C.byref(robot), out.ctypes.data_as(_u8)))
    return out


@dataclass
class SelfResult:
    free: np.ndarray         # [N] bool
    worst_pair: np.ndarray   # [N] int32: a*J + b; verdict mode: the first colliding pair, -1 when free
    clearance: np.ndarray    # [N], None unless requested
    ms: float                # device time of the launch (0 on the host)


def check(robot, q, pairs=None, shrink=None, clearance=False, host=False):
    """q [N,n] (or [n]) -> SelfResult.  pairs [J,J] (None: default_pairs), shrink [J,J] (None: zeros); only a < b is read."""
    L = _lib.load()
    n = robot.num_factors
    q = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1, n))
    N = q.shape[0]
    pairs, shrink, pp, sp = table_args(robot, pairs, shrink)
    free = np.zeros(N, dtype=np.uint8)
    wp = np.zeros(N, dtype=np.int32)
    cl = np.zeros(N) if clearance else None
    args = [C.byref(robot), pp, sp, N, _dp(q), free.ctypes.data_as(_u8), _dp(cl), wp.ctypes.data_as(C.POINTER(C.c_int32))]
    ms = C.c_double(0.0)
    if host:
        _check(L.armour_self_check_host(*args))
    else:
        _check(L.armour_self_check(*args, C.byref(ms)))
    return SelfResult(free=free.astype(bool), worst_pair=wp, clearance=cl, ms=ms.value)


def edges_free_host(robot, qa, qb, edge_step=0.05, continuous=None, pairs=None, shrink=None):
    """The self edge rule for the joint-space segments qa[e] -> qb[e] in a host loop (armour_self_edges_host) -> [E] bool."""
    n = robot.num_factors
    qa = np.ascontiguousarray(np.asarray(qa, dtype=np.float64).reshape(-1, n))
    qb = np.ascontiguousarray(np.asarray(qb, dtype=np.float64).reshape(-1, n))
    cont = None if continuous is None else np.ascontiguousarray(continuous, dtype=np.uint8).reshape(n)
    pairs, shrink, pp, sp = table_args(robot, pairs, shrink)
    out = np.zeros(qa.shape[0], dtype=np.uint8)
    _check(_lib.load().armour_self_edges_host(C.byref(robot), None if cont is None else cont.ctypes.data_as(_u8), float(edge_step), pp, sp, qa.shape[0],
                                              _dp(qa), _dp(qb), out.ctypes.data_as(_u8)))
    return out.astype(bool)


def calibrate_shrink(robot, configs, pairs=None, margin=1e-3, host=False):
    """[J,J]: the smallest per-pair shrink that clears every configuration of `configs` [N,n] -- for pair (a, b), its deepest penetration
    over the configurations + margin, 0 where the pair never penetrates.  Shrinking box b by d raises every axis value of the pair by at
    least d, so a pair that penetrates by p is cleared by p + margin.  One clearance-mode check per listed pair."""
    J = robot.num_joints
    listed = default_pairs(robot) if pairs is None else np.asarray(pairs).astype(np.uint8).reshape(J, J)
    out = np.zeros((J, J))
    for a in range(J):
        for b in range(a + 1, J):
            if not listed[a, b]:
                continue
            one = np.zeros((J, J), dtype=np.uint8)
            one[a, b] = 1
            cl = check(robot, configs, pairs=one, clearance=True, host=host).clearance
            worst = float(np.min(cl)) if cl.size else np.inf
            if worst <= 0.0:
                out[a, b] = -worst + margin
    return out
