"""Path audit: executed pieces of Bezier plans checked against worlds' obstacles on the MI355X (include/armour_hip.h, armour_path_audit).

    res = audit(robot, obstacles, world_of_piece, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube=None, step=0.02)
    res.verdict        # [P]: 0 proved free, 1 proved hit, 2 undecided (NOT a finding: the audit at this step could not prove the piece free)
    res.t_hit          # [P]: the first colliding sample time of a verdict-1 piece, NaN otherwise
    res.clearance      # [P]: the minimum sample clearance (with clearance=True)

audit_moving(robot, obstacles, velocity, world_of_piece, t_world, ...) is the same audit against obstacles in linear motion.

`host=True` runs the library's host restatement of the same rule (no GPU needed; for tests).  The rule, its bound and the proof sketch are
stated in include/armour_hip.h and DESIGN.md.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import _dp, check

FREE, HIT, UNDECIDED = 0, 1, 2


@dataclass
class AuditResult:
    verdict: np.ndarray
    t_hit: np.ndarray
    clearance: np.ndarray   # None unless requested
    ms: float               # device time of the launch (0 on the host)


def _pieces(robot, q0, qd0, qdd0, k, k_range, ta, tb):
    n = robot.num_factors
    q0, qd0, qdd0, k = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, n)) for a in (q0, qd0, qdd0, k)]
    P = q0.shape[0]
    for a in (qd0, qdd0, k):
        if a.shape != (P, n):
            raise ValueError(f"expected shape ({P},{n}), got {a.shape}")
    k_range = np.ascontiguousarray(np.broadcast_to(np.asarray(k_range, dtype=np.float64), (n,)))
    ta = np.ascontiguousarray(np.broadcast_to(np.asarray(ta, dtype=np.float64), (P,)))
    tb = np.ascontiguousarray(np.broadcast_to(np.asarray(tb, dtype=np.float64), (P,)))
    return P, n, q0, qd0, qdd0, k, k_range, ta, tb


def _audit(entries, lead, robot, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step, clearance, host):
    """What audit and audit_self share.  entries: the (device, host) entries' names; lead(P): the arguments between the robot and q0."""
    L = _lib.load()
    P, n, q0, qd0, qdd0, k, k_range, ta, tb = _pieces(robot, q0, qd0, qdd0, k, k_range, ta, tb)
    tube = None if tube is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tube, dtype=np.float64), (P, n)))
    verdict = np.zeros(P, dtype=np.int32)
    t_hit = np.zeros(P)
    cl = np.zeros(P) if clearance else None
    args = [C.byref(robot), *lead(P), _dp(q0), _dp(qd0), _dp(qdd0), _dp(k), _dp(k_range), float(duration), _dp(ta), _dp(tb), _dp(tube), float(step),
            verdict.ctypes.data_as(C.POINTER(C.c_int32)), _dp(t_hit), _dp(cl)]
    ms = C.c_double(0.0)
    if host:
        check(getattr(L, entries[1])(*args))
    else:
        check(getattr(L, entries[0])(*args, C.byref(ms)))
    return AuditResult(verdict=verdict, t_hit=t_hit, clearance=cl, ms=ms.value)


def audit(robot, obstacles, world_of_piece, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube=None, step=0.02, clearance=False, host=False):
    """P pieces in one call.  obstacles [W,O,12] (or [O,12]: W = 1); world_of_piece [P]; q0 / qd0 / qdd0 / k [P,n]; k_range [n]; ta / tb [P] or
    scalars; tube [P,n], [n] or None (zeros): the per-joint radius about the plan that is audited with it."""
    obs, W, O = _lib.as_worlds(obstacles)

    def lead(P):
        wp = np.ascontiguousarray(np.broadcast_to(np.asarray(world_of_piece, dtype=np.int32), (P,)))
        return [W, O, _dp(obs) if obs.size else None, P, wp.ctypes.data_as(C.POINTER(C.c_int32))]
    return _audit(("armour_path_audit", "armour_path_audit_host"), lead, robot, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step, clearance, host)


def audit_moving(robot, obstacles, velocity, world_of_piece, t_world, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube=None, step=0.02, clearance=False,
                 host=False):
    """audit against obstacles in linear motion (armour_path_audit_moving): obstacles [W,O,12] (or [O,12]) are the poses at world time 0, velocity
    [W,O,3] (or [O,3]) the constant velocities, t_world [P] (or a scalar) the world time of every piece's plan time 0.  t_hit is a plan time."""
    obs, W, O = _lib.as_worlds(obstacles)
    vel = np.ascontiguousarray(np.asarray(velocity, dtype=np.float64).reshape(W, O, 3))

    def lead(P):
        wp = np.ascontiguousarray(np.broadcast_to(np.asarray(world_of_piece, dtype=np.int32), (P,)))
        tw = np.ascontiguousarray(np.broadcast_to(np.asarray(t_world, dtype=np.float64), (P,)))
        return [W, O, _dp(obs) if obs.size else None, _dp(vel) if vel.size else None, P, wp.ctypes.data_as(C.POINTER(C.c_int32)), _dp(tw)]
    return _audit(("armour_path_audit_moving", "armour_path_audit_moving_host"), lead, robot, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube, step, clearance,
                  host)


def audit_self(robot, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube=None, step=0.02, pairs=None, shrink=None, clearance=False, host=False):
    """The same pieces against the arm itself (armour_path_audit_self): verdict 0 proved self-free, 1 proved self-hit (t_hit), 2 undecided.
    pairs / shrink [J,J] as armour_amd.self_check.check takes them (None: every pair b - a >= 2, no shrink)."""
    from .self_check import table_args
    pairs, shrink, pp, sp = table_args(robot, pairs, shrink)
    return _audit(("armour_path_audit_self", "armour_path_audit_self_host"), lambda P: [pp, sp, P], robot, q0, qd0, qdd0, k, k_range, duration, ta, tb, tube,
                  step, clearance, host)


def audit_items(robot, q0, qd0, qdd0, k, k_range, duration, ta, tb, step=0.02):
    """[P] int64: the sub-intervals (work items) an audit of every piece takes at `step`."""
    P, n, q0, qd0, qdd0, k, k_range, ta, tb = _pieces(robot, q0, qd0, qdd0, k, k_range, ta, tb)
    out = np.zeros(P, dtype=np.int64)
    check(_lib.load().armour_path_audit_items(C.byref(robot), P, _dp(q0), _dp(qd0), _dp(qdd0), _dp(k), _dp(k_range), float(duration), _dp(ta), _dp(tb),
                                              float(step), out.ctypes.data_as(C.POINTER(C.c_int64))))
    return out
