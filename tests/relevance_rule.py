"""The row rule of relevance.hip (include/armour_hip.h: armour_get_row_relevance, armour_get_solver_rows), restated once in numpy.

A function of ONE problem's tables alone, in np.longdouble, the planes and the monomials in plain loops (only the rows are vectorised).  There is
no hull pass: the kernel's hull pass is an early exit of the same rule (hull >= tight sum).  The constants are the doubles the kernel compiles.

Layouts (one problem; J links, T time steps, O obstacles, n factors):
  link_cen [J*T, 3], link_keys [J*T, cap], link_coef [J*T, cap, 3], link_cnt [J*T]     index l * T + t; keys: 2 bits per factor
  A [Q, 36, 3], d [Q, 36], delta [Q, 36]                                             row q = (l * T + t) * O + o;  live [36] bool
  tq_cen [n*T], tq_keys [n*T, cap], tq_coef [n*T, cap], tq_cnt [n*T]                   row r = t * n + j
  gl, gu [m]                                                                         m = n*T + Q + 4n (the limit rows' entries are not read)
"""
import numpy as np

LD = np.longdouble
REL_MARGIN = LD(1e-9)
TIGHT = LD(1.0 + 1e-12)          # the factor on the relevance mask's sums
BOX_SLACK = LD(3e-5)             # the solver evaluates its lists up to 1e-6 outside the box: (1 + 1e-6)^21 < 1 + 3e-5
UNDECIDED = LD(1e-11)            # relative width of the band in which a row counts as undecided


def key_degrees(keys):
    """total degree of each monomial: the sum of the key's 2-bit fields"""
    k = np.asarray(keys, dtype=np.uint64)
    deg = np.zeros(k.shape, dtype=np.int64)
    for j in range(32):
        deg += ((k >> np.uint64(2 * j)) & np.uint64(3)).astype(np.int64)
    return deg


def collision_rule(link_cen, link_keys, link_coef, link_cnt, A, d, delta, live, gl_c, gu_c, O, unit_normals):
    """Collision rows.  gl_c, gu_c: the bounds of the Q collision rows.  Returns the dict of row_rule() for these rows."""
    A, d, delta = LD(np.asarray(A)), LD(np.asarray(d)), LD(np.asarray(delta))
    Q = A.shape[0]
    lt = np.arange(Q) // max(O, 1)
    c = LD(np.asarray(link_cen))[lt]
    co = LD(np.asarray(link_coef))[lt]
    cnt = np.asarray(link_cnt)[lt]
    deg = key_degrees(link_keys)[lt]
    cap = int(cnt.max()) if Q else 0          # (no monomial behind the largest count is read)
    u = LD(np.asarray(gu_c))
    rd = np.zeros((Q, 3), dtype=LD)
    for i in range(cap):
        on = (i < cnt)[:, None]
        rd += np.where(on, LD(deg[:, i])[:, None] * np.abs(co[:, i, :]), LD(0))
    rdn = np.sqrt((rd * rd).sum(1))
    amax = np.ones(Q, dtype=LD)
    if not unit_normals:
        for p in range(36):
            if live[p]:
                amax = np.maximum(amax, np.sqrt((A[:, p, :] * A[:, p, :]).sum(1)) * TIGHT)
    need2 = REL_MARGIN + LD(2) * rdn * amax * (LD(1) + BOX_SLACK) - u
    ninf = LD(-np.inf)
    best1, best2 = np.full(Q, ninf), np.full(Q, ninf)
    sure1, near1 = np.zeros(Q, bool), np.zeros(Q, bool)      # some plane surely separates | some plane is inside its band
    sure2, near2 = np.zeros(Q, bool), np.zeros(Q, bool)
    for p in range(36):
        if not live[p]:
            continue
        a = A[:, p, :]
        nz = (a != 0).any(1)
        s = np.abs(a[:, 0] * c[:, 0] + a[:, 1] * c[:, 1] + a[:, 2] * c[:, 2] - d[:, p])
        h = np.zeros(Q, dtype=LD)
        for i in range(cap):
            h += np.where(i < cnt, np.abs(a[:, 0] * co[:, i, 0] + a[:, 1] * co[:, i, 1] + a[:, 2] * co[:, i, 2]), LD(0))
        L = s - h * TIGHT - delta[:, p]
        scale = s + h + np.abs(delta[:, p])
        e1 = L - REL_MARGIN                      # >= 0: plane p separates the family
        e2 = L - h * BOX_SLACK - need2           # >= 0: ... by enough that the row is never a QP candidate
        band1 = UNDECIDED * scale
        band2 = UNDECIDED * (scale + LD(2) * rdn * amax + np.abs(u))   # (need2's own terms round too)
        best1 = np.where(nz, np.maximum(best1, e1), best1)
        best2 = np.where(nz, np.maximum(best2, e2), best2)
        sure1 |= nz & (e1 > band1); near1 |= nz & (np.abs(e1) <= band1)
        sure2 |= nz & (e2 > band2); near2 |= nz & (np.abs(e2) <= band2)
    dropped = best1 >= 0
    lower_bounded = np.asarray(gl_c) > -1e18     # (no collision row has a lower bound; one that had would stay a solver row)
    dropped2 = dropped & (best2 >= 0) & ~lower_bounded
    und1 = ~sure1 & near1
    # the solver's verdict is an AND of two ORs: surely dropped = both surely hold; surely kept = one of them surely fails
    und2 = ~lower_bounded & ~(sure1 & sure2) & ~((~sure1 & ~near1) | (~sure2 & ~near2))
    return dict(rel=~dropped, solver=~dropped2, dist_rel=best1, dist_solver=np.minimum(best1, best2), undecided_rel=und1, undecided_solver=und2)


def torque_rule(tq_cen, tq_keys, tq_coef, tq_cnt, gl_t, gu_t):
    cen, co, cnt = LD(np.asarray(tq_cen)), LD(np.asarray(tq_coef)), np.asarray(tq_cnt)
    deg = key_degrees(tq_keys)
    l, u = LD(np.asarray(gl_t)), LD(np.asarray(gu_t))
    R = cen.shape[0]
    rad, radd = np.zeros(R, dtype=LD), np.zeros(R, dtype=LD)
    for i in range(int(cnt.max()) if R else 0):
        f = np.where(i < cnt, np.abs(co[:, i]), LD(0))
        rad += f
        radd += LD(deg[:, i]) * f
    reach = (rad + LD(2) * radd) * (LD(1) + BOX_SLACK)
    out = {}
    for name, r in (("rel", rad), ("solver", reach)):
        eu = cen + r - (u - REL_MARGIN)          # >= 0: the interval reaches the upper bound
        el = (l + REL_MARGIN) - (cen - r)        # >= 0: ... the lower bound
        bu, bl = UNDECIDED * (np.abs(cen) + r + np.abs(u)), UNDECIDED * (np.abs(cen) + r + np.abs(l))
        out[name] = (eu >= 0) | (el >= 0)
        out["dist_" + name] = np.maximum(eu, el)
        out["sure_" + name] = (eu > bu) | (el > bl)
        out["near_" + name] = (np.abs(eu) <= bu) | (np.abs(el) <= bl)
    rel, solver = out["rel"], out["rel"] | out["solver"]
    und1 = ~out["sure_rel"] & out["near_rel"]
    und2 = ~(out["sure_rel"] | out["sure_solver"]) & (out["near_rel"] | out["near_solver"])
    return dict(rel=rel, solver=solver, dist_rel=out["dist_rel"], dist_solver=np.maximum(out["dist_rel"], out["dist_solver"]),
                undecided_rel=und1, undecided_solver=und2)


def row_rule(link_cen, link_keys, link_coef, link_cnt, A, d, delta, live, tq_cen, tq_keys, tq_coef, tq_cnt, gl, gu, O, unit_normals):
    """Both verdicts of every row of one problem.  Returns dict of [m] arrays:
      rel, solver                         bool: the row is in the relevance mask / the solver's mask
      dist_rel, dist_solver               longdouble: the signed distance of the deciding inequality to its threshold -- collision rows: >= 0 = dropped
                                          (the largest over the planes; the solver's: the smaller of its two conditions); torque rows: >= 0 = kept;
                                          limit rows: +inf
      undecided_rel, undecided_solver     bool: the verdict hangs on a distance within 1e-11 x (|A.c - d| + sum |A.coef| + |delta|) of zero (torque
                                          rows: 1e-11 x (|cen| + rad + |bound|); the solver's second condition adds 2 |rd| amax + |u| to the scale)"""
    nT, Q = np.asarray(tq_cen).shape[0], np.asarray(A).shape[0]
    m = len(gl)
    tq = torque_rule(tq_cen, tq_keys, tq_coef, tq_cnt, gl[:nT], gu[:nT])
    if Q:
        col = collision_rule(link_cen, link_keys, link_coef, link_cnt, A, d, delta, live, gl[nT:nT + Q], gu[nT:nT + Q], O, unit_normals)
    out = {}
    for key in tq:
        limit = np.full(m - nT - Q, LD(np.inf)) if key.startswith("dist") else np.full(m - nT - Q, not key.startswith("undecided"))
        out[key] = np.concatenate([tq[key], col[key] if Q else tq[key][:0], limit])
    return out
