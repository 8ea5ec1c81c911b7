"""The device form's QP (solve_qp_wave of armour_amd/csrc/solver_device.hip) tested directly, against the host form's (solve_qp of solver.hip).

Both forms of armour_solve must produce the same iterates bit for bit, and the device QP is hand-written wave-level code with three ways of
holding the rows (registers, LDS staging, global memory), two of holding the flags (LDS, global bytes), a Cholesky factor that is extended and
rolled back, and four elastic attempts side by side.  Whole solves of random worlds (tests/test_solve.py) reach it without anybody knowing
which of these a QP met.  Here hand-built QPs go through two test hooks that pose them as armour_solve does:

  armour_debug_qp_elastic  the host form's attempt loop and solve_qp, with counters of what the active-set method did;
  armour_debug_qp_device   solve_qp_wave in a one-block launch of its own, for either kernel build (wps = 1 | 2) and any LDS room.

CPU: every feasible case passes the KKT certificate of tests/test_qp_solver.py (the literal floor cases its primal part: check_certificates), the attempt taken is the lowest feasible one of separate
solves at the four sigmas, and the case list is shown to reach every path (per storage regime: a row dropped from the middle of the active
set, each attempt 0..3 and none; somewhere: an excluded row, a full active set, an attempt of more than 18 steps) -- so the GPU parity
cannot be vacuous.  GPU: the device hook equals the host hook bit for bit, in both builds and in both ABIs (the 8-factor library in a child
process with ARMOUR_KEY128=1, as tests/test_key128.py runs its bodies)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = (0.0, 0.5, 0.9, 0.99)
K_FLAGS_IN_LDS = 1024   # solver_device.hip kFlagsInLds


def _reg_rows(wps):
    return 64 * (4 if wps == 1 else 2)   # solve_qp_wave: 64 * kRegRows


def _lds_rows(wps, maxf):
    return ((96 if wps == 1 else 40) * 1024) // (8 * (maxf + 1))   # what a solve of that build stages (armour_solve_device_capacity)


# ---------------------------------------------------------------------------------------------------------------- the case generator
def _pose(rng, n, hd_floor=None, far_out=False):
    """Hd, gradf, x and the scale of every variable's column in the candidate rows.

    hd_floor: the floor of hess_diag (1e-12) against ordinary entries -- one variable at the floor, the others of the chosen ones between 10^-11.5 and 1e-3.

    "literal": nothing else changes -- rows and a gradient of ordinary size on those variables.  M = N'G^-1 N then spans twelve decades, and this is where
    the two forms' sums, factors and final verifications would part first.  The host form's answer is itself inexact there (see check_certificates).

    "posed": as armour_solve can pose it.  Hd_j = 2 cost_scale dk_j^2 with dk_j proportional to the joint's k_range_j, and k_j enters the trajectory -- so
    every constraint row and the cost's gradient -- through the product k_range_j k_j only: column j of the Jacobian and gradf_j carry the factor
    k_range_j, i.e. sqrt(Hd_j).  So a variable AT the floor (k_range_j = 0: dk_j = 0) has a zero column and a zero gradient entry and meets only its own
    box rows, and one NEAR it has a column and a gradient entry scaled by sqrt(Hd_j).  In scaled variables these QPs are as well conditioned as (a)."""
    assert hd_floor in (None, "literal", "posed")
    Hd = rng.uniform(0.05, 30.0, n)
    col = np.ones(n)
    gradf = rng.normal(size=n) * (8.0 if far_out else 0.5)
    if hd_floor:
        idx = rng.choice(n, size=max(2, n // 3), replace=False)
        Hd[idx[0]] = 1e-12                                                # at the floor
        for j in idx[1:]:                                                 # between the floor and the ordinary entries
            Hd[j] = 10.0 ** rng.uniform(-11.5, -3.0)
        if hd_floor == "posed":
            col[idx] = np.sqrt(Hd[idx])
            col[idx[0]] = 0.0
            gradf[idx] *= col[idx]
            gradf[idx[0]] = 0.0
    x = rng.uniform(-0.6, 0.6, n)
    return Hd, gradf, x, col


def _far_rows(rng, n, count, x, around, col=None):
    """rows a'd >= v that hold with room at `around` (a point of the step's box); col: the scale of every variable's column"""
    a = -rng.normal(size=(count, n)) * (1.0 if col is None else col)
    v = a @ around - rng.uniform(0.05, 2.0, count)
    return a, v


def _case_random(rng, n, ncand, hd_floor, far_out, ncut):
    """(a) / (b): random rows of which some cut the box-clipped point off.  A variant of the seed % 4 == 3 recipe of tests/test_qp_solver.py, not that
    recipe: there every row's slack at the box-clipped point is uniform(-0.3, 1.0), so about a quarter of the rows cut it; here exactly `ncut` rows cut
    it, by 0 .. 0.3, and the others have room 0.05 .. 2, so that the number of cutting rows does not grow with ncand (check_coverage shows what the
    cases reach)."""
    Hd, gradf, x, col = _pose(rng, n, hd_floor, far_out)
    d_box = np.clip(-gradf / Hd, -1.0 - x, 1.0 - x)
    a, v = _far_rows(rng, n, ncand, x, d_box, col)
    cut = rng.choice(ncand, size=min(ncut, ncand), replace=False) if ncand else np.zeros(0, dtype=int)
    v[cut] = a[cut] @ d_box + rng.uniform(0.0, 0.3, len(cut))
    return Hd, gradf, x, a, v, cut


def _case_parallel(rng, n, ncand, noise):
    """(c): near-parallel rows, as the collision rows of adjacent time steps (test_nearly_parallel_rows_like_adjacent_time_steps)"""
    base = rng.normal(size=n)
    A = np.vstack([base + noise * rng.normal(size=n) for _ in range(ncand)])
    hi = np.full(ncand, -0.3) + 0.1 * noise * rng.normal(size=ncand)
    return np.ones(n), np.zeros(n), np.zeros(n), -A, -hi


def _case_dependent(rng, n, ncand, ncut):
    """(d): exact duplicates and exact multiples of the cutting rows (ties in the arg-min, a dependent active set), and rows one rounding away from
    dependent (the factor's spd test)"""
    Hd, gradf, x, a, v, cut = _case_random(rng, n, ncand, None, True, ncut)
    free = [i for i in range(ncand) if i not in set(cut.tolist())]
    rng.shuffle(free)
    for c in cut:
        for scale in (1.0, 2.0, 0.5, 1.0 + 2.0 ** -50):
            if not free:
                break
            i = free.pop()
            a[i], v[i] = a[c] * scale, v[c] * scale
    return Hd, gradf, x, a, v


def _case_apex(rng, n, ncand, extra):
    """(e): n + extra rows that meet at one point, which is the solution: more rows want to be active than the active set can hold"""
    Hd, _, x, _ = _pose(rng, n)
    apex = rng.uniform(-0.3, 0.3, n) - 0.3 * x
    c = rng.normal(size=n)
    c /= np.linalg.norm(c)
    k = min(ncand, n + extra)
    a, v = _far_rows(rng, n, ncand, x, apex)
    at = rng.choice(ncand, size=k, replace=False)
    a[at] = c + 0.6 * rng.normal(size=(k, n))
    v[at] = a[at] @ apex
    d0 = apex - 1.5 * c
    return Hd, -Hd * d0, x, a, v


def _case_elastic(rng, n, ncand, which):
    """(f): on one unit normal a, at x = 0: a'd >= 0.6 against a second row -- 0.6 (1 - sigma) against the second bound decides the attempt (0.6 a lies
    inside the box); the other rows hold with room everywhere near"""
    a0 = rng.normal(size=n)
    a0 /= np.linalg.norm(a0)
    second = {1: (-a0, -0.4), 2: (-a0, -0.1), 3: (-a0, -0.01), 4: (-a0, 0.1)}[which]   # a'd <= 0.4 | 0.1 | 0.01; -a'd >= 0.1: infeasible at every sigma
    x = np.zeros(n)
    a, v = _far_rows(rng, n, ncand, x, 0.3 * a0)
    v -= 0.3 * np.abs(a @ a0)   # room along the whole segment [0, 0.6 a0], where every attempt's iterates lie
    at = np.sort(rng.choice(ncand, size=2, replace=False))
    a[at[0]], v[at[0]] = a0, 0.6
    a[at[1]], v[at[1]] = second
    return np.ones(n), np.zeros(n), x, a, v


def _sizes(n, maxf):
    """(tag, ncand, lds_rows): the smallest shapes that reach each way of holding rows and flags; mrows = ncand + 2 n"""
    out = [("edge0", 0, 0), ("edge1", 1, 0)]
    for wps in (2, 1):
        out += [("reg%d" % _reg_rows(wps), _reg_rows(wps) - 2 * n, 0), ("reg%d" % (_reg_rows(wps) + 1), _reg_rows(wps) + 1 - 2 * n, 0)]
    out += [("lds300", 300, 300), ("lds301", 301, 300)]
    for wps in (2, 1):
        out += [("own%d" % _lds_rows(wps, maxf), _lds_rows(wps, maxf), 0), ("own%d" % (_lds_rows(wps, maxf) + 1), _lds_rows(wps, maxf) + 1, 0)]
    out += [("flags1024", K_FLAGS_IN_LDS - 2 * n, 0), ("flags1025", K_FLAGS_IN_LDS + 1 - 2 * n, 0)]
    return out


# A case's generator is seeded with SEED0 + its position in the list.  The seeds have to meet the conditions of check_coverage for both ABIs' lists:
# change the generators or the list's order and check that again -- on the CPU, before any GPU run.
SEED0 = 20240


def make_cases(maxf):
    """the named QPs of one ABI: n = maxf (every lane and entry in use) and n = 3 (the lanes and entries past n are padding)"""
    cases = []

    def add(name, n, content, lds_rows, Hd, gradf, x, a, v, tol=1e-7):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, n))
        cases.append(dict(name=name, n=n, content=content, lds_rows=lds_rows, Hd=np.asarray(Hd, dtype=np.float64), gradf=np.asarray(gradf, dtype=np.float64),
                          x=np.asarray(x, dtype=np.float64), a=a, v=np.ascontiguousarray(v, dtype=np.float64), tol=tol))

    def rng_for():
        return np.random.default_rng(SEED0 + len(cases))

    for n in (maxf, 3):
        # (g) no candidate rows: the minimiser inside and outside the box
        add("n%d-g-inside" % n, n, "g", 0, np.full(n, 2.0), np.linspace(-0.4, 0.4, n), np.full(n, 0.1), np.zeros((0, n)), np.zeros(0))
        add("n%d-g-outside" % n, n, "g", 0, np.linspace(0.5, 3.0, n), np.linspace(-9.0, 9.0, n), np.linspace(-0.5, 0.5, n), np.zeros((0, n)), np.zeros(0))
        for tag, ncand, lds in _sizes(n, maxf):
            if ncand == 0:
                continue
            for content, floor, far_out in (("a", None, False), ("a2", None, True), ("b", "posed", False), ("b2", "posed", True)):
                name = "n%d-%s-%s" % (n, tag, content)
                Hd, gradf, x, a, v, _ = _case_random(rng_for(), n, ncand, floor, far_out, ncut=3 * n)
                add(name, n, content[0], lds, Hd, gradf, x, a, v)
            if ncand >= 8 * n:
                name = "n%d-%s-d" % (n, tag)
                add(name, n, "d", lds, *_case_dependent(rng_for(), n, ncand, ncut=2 * n))
                name = "n%d-%s-e" % (n, tag)
                add(name, n, "e", lds, *_case_apex(rng_for(), n, ncand, extra=5))
            if tag in ("edge1",):
                continue
            if tag in ("reg128", "reg257", "lds300", "lds301", "flags1025") or tag.startswith("own"):
                for which in (1, 2, 3, 4):
                    name = "n%d-%s-f%d" % (n, tag, which)
                    add(name, n, "f%d" % which, lds, *_case_elastic(rng_for(), n, ncand, which))
        # (c) 200 near-parallel rows, at the noise of test_qp_solver.py and closer
        for noise in (1e-6, 1e-9):
            name = "n%d-c-%g" % (n, noise)
            add(name, n, "c", 0, *_case_parallel(rng_for(), n, 200, noise), tol=1e-6)
        # (f) the four elastic cases alone: two rows
        for which in (1, 2, 3, 4):
            name = "n%d-two-f%d" % (n, which)
            add(name, n, "f%d" % which, 0, *_case_elastic(rng_for(), n, 2, which))
    # (b) as it reads: rows and a gradient of ordinary size on variables whose Hd goes down to the floor, in every storage regime.  (Behind all other
    # cases, whose seeds are their positions.)
    for n in (maxf, 3):
        for tag, ncand, lds in _sizes(n, maxf):
            if ncand == 0:
                continue
            for content, far_out in (("bl", False), ("bl2", True)):
                Hd, gradf, x, a, v, _ = _case_random(rng_for(), n, ncand, "literal", far_out, ncut=3 * n)
                add("n%d-%s-%s" % (n, tag, content), n, "bl", lds, Hd, gradf, x, a, v)
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def storage(case, wps, maxf):
    """where solve_qp_wave of the `wps` build holds this case's rows and flags"""
    n, ncand = case["n"], len(case["v"])
    mrows = ncand + 2 * n
    lds = case["lds_rows"] or _lds_rows(wps, maxf)
    rows = "registers" if mrows <= _reg_rows(wps) else "lds" if ncand <= lds else "global"
    return rows, "lds" if mrows <= K_FLAGS_IN_LDS else "global"


# ---------------------------------------------------------------------------------------------------------------- the hooks
def _ptrs(case):
    dp = C.POINTER(C.c_double)
    a = case["a"] if len(case["v"]) else np.zeros(1)
    v = case["v"] if len(case["v"]) else np.zeros(1)
    return [arr.ctypes.data_as(dp) for arr in (case["Hd"], case["gradf"], case["x"])], a.ctypes.data_as(dp), v.ctypes.data_as(dp)


def host_qp(case):
    from armour_amd import _lib
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    n = case["n"]
    d = np.zeros(n)
    feas, att, mult = C.c_int32(-1), C.c_int32(-1), C.c_double(0)
    per = [np.full(4, -7, dtype=np.int32) for _ in range(5)]
    (hd, gf, x), a, v = _ptrs(case)
    _lib.check(L.armour_debug_qp_elastic(n, hd, gf, x, len(case["v"]), a, v, d.ctypes.data_as(dp), C.byref(feas), C.byref(att), C.byref(mult),
                                         *[p.ctypes.data_as(ip) for p in per]))
    return dict(d=d, feasible=bool(feas.value), attempt=att.value, max_mult=mult.value, steps=per[0], dropped=per[1], dropped_mid=per[2],
                excluded=per[3], active=per[4])


def device_qp(case, wps):
    from armour_amd import _lib
    L = _lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    n = case["n"]
    d = np.zeros(n)
    feas, att, mult = C.c_int32(-1), C.c_int32(-1), C.c_double(0)
    it = np.full(4, -7, dtype=np.int32)
    (hd, gf, x), a, v = _ptrs(case)
    _lib.check(L.armour_debug_qp_device(n, hd, gf, x, len(case["v"]), a, v, wps, case["lds_rows"], d.ctypes.data_as(dp), C.byref(feas), C.byref(att),
                                        C.byref(mult), it.ctypes.data_as(ip)))
    return dict(d=d, feasible=bool(feas.value), attempt=att.value, max_mult=mult.value, qp_iter=it)


def _elastic_rows(case, sigma):
    """the QP of one attempt as lo <= A d <= hi: the candidate rows with their elastic right-hand sides, then the step's box"""
    n, v, x = case["n"], case["v"], case["x"]
    b = v - np.where(v > 0, sigma * v, 0.0)
    A = np.vstack([case["a"], np.eye(n)])
    return A, np.concatenate([b, -1.0 - x]), np.concatenate([np.full(len(v), 1e19), 1.0 - x])


# ---------------------------------------------------------------------------------------------------------------- CPU: the host hook
_HOST = {}


def host_results(maxf):
    """[(case, host result)] of one ABI's list, solved once per process and left unchanged"""
    if maxf not in _HOST:
        from armour_amd import _lib
        assert _lib.MAXF == maxf
        _HOST[maxf] = [(case, host_qp(case)) for case in make_cases(maxf)]
    return _HOST[maxf]


def check_attempts(maxf):
    """the attempt taken is the lowest feasible one of four separate solves at the four sigmas, with the same step, multiplier and steps; the (f)
    cases take exactly the stated attempts"""
    from test_qp_solver import _qp_box
    for case, h in host_results(maxf):
        k, m = h["attempt"], len(case["v"])
        assert 0 <= k <= 3 and (h["feasible"] or k == 3), (case["name"], h)
        assert all(h["steps"][e] >= 0 for e in range(k + 1)) and all(h["steps"][e] == -1 for e in range(k + 1, 4)), (case["name"], h)
        lowest = None
        for e, sigma in enumerate(SIGMAS):
            A, lo, hi = _elastic_rows(case, sigma)
            xb, ok, steps, mult = _qp_box(case["Hd"], case["gradf"], A[:m], lo[:m], hi[:m], lo[m:], hi[m:], True)
            if e <= k:
                assert steps == h["steps"][e], (case["name"], e, steps, h)
            if ok and lowest is None:
                lowest = e
                assert h["feasible"] and k == e and np.array_equal(xb, h["d"]) and mult == h["max_mult"], (case["name"], e, xb, mult, h)
        assert (lowest is None) == (not h["feasible"]), (case["name"], lowest, h)
        if case["content"].startswith("f"):   # 0.6 (1 - sigma) against the second row's bound
            which = int(case["content"][1])
            assert (h["feasible"], k) == ((True, which) if which < 4 else (False, 3)), (case["name"], h)


def check_certificates(maxf):
    """every feasible case passes the KKT certificate of tests/test_qp_solver.py, with its tolerances, on the rows of the attempt taken.

    The literal floor cases ("bl") are held to the certificate's primal part only, with its tolerance.  Their stationarity is not asserted because the
    host form -- the reference of the bit parity, not the code under test here -- does not reach it: with Hd_j = 1e-12 under rows of ordinary size
    N'G^-1 N loses twelve digits, and solve_qp returns feasible = 1 with its active rows up to 4e-4 inside their bounds (its final verification looks
    at violations only), which the certificate's 1e-6 active-row window and residual cannot pass.  That is a limitation of solve_qp on input a problem
    set is not expected to pose; what the two forms owe each other there -- the same bits -- is asserted in full on the GPU."""
    from test_qp_solver import _kkt_certificate
    failed = []
    for case, h in host_results(maxf):
        if not h["feasible"]:
            continue
        A, lo, hi = _elastic_rows(case, SIGMAS[h["attempt"]])
        if case["content"] == "bl":
            Ad = A @ h["d"]
            if not (np.all(Ad <= hi + case["tol"]) and np.all(Ad >= lo - case["tol"])):
                failed.append("%s (attempt %d): primal infeasible by %.3g" % (case["name"], h["attempt"], max((Ad - hi).max(), (lo - Ad).max())))
            continue
        try:
            _kkt_certificate(case["Hd"], case["gradf"], A, lo, hi, h["d"], tol=case["tol"])
        except AssertionError as e:
            slack = np.sort(A @ h["d"] - lo)[:case["n"]]
            failed.append("%s (attempt %d, %d active rows): %s; smallest row slacks %s" % (case["name"], h["attempt"], h["active"][h["attempt"]], str(e).split("\n")[0],
                                                                                         np.array2string(slack, precision=2)))
    assert not failed, "\n".join(failed)


def check_coverage(maxf, done, verbose=True):
    """the case list reaches every path of the QP, by the host's counters (conditions, not measurements); prints what every case did and, per
    regime, the first case that meets each condition"""
    regimes = {}   # (wps, rows held in) -> {what some case of that regime did: the first such case}
    anywhere = {}
    for case, h in done:
        k = h["attempt"]
        did = ["attempt%d" % k if h["feasible"] else "none"]
        ran = range(k + 1)
        if any(h["dropped_mid"][e] > 0 for e in ran):
            did.append("dropped_mid")
        if any(h["excluded"][e] > 0 for e in ran):
            anywhere.setdefault("excluded", case["name"])
        if h["feasible"] and h["active"][k] == case["n"]:
            anywhere.setdefault("full_active_set", case["name"])
        if max(h["steps"][e] for e in ran) > 18:
            anywhere.setdefault("more_than_18_steps", case["name"])
        for wps in (1, 2):
            rows, flags = storage(case, wps, maxf)
            for key in [(wps, rows)] + ([(wps, "global flags")] if flags == "global" else []):
                for what in did:
                    regimes.setdefault(key, {}).setdefault(what, case["name"])
                regimes[key].setdefault("content " + (case["content"] if case["content"] == "bl" else case["content"][0]), case["name"])
        if verbose:
            ints = lambda q: " ".join("%d" % e for e in h[q])
            print("%-22s ncand %4d lds_rows %3d wps1 %-14s wps2 %-14s | feasible %d attempt %d | steps %s | dropped %s | mid %s | excluded %s | active %s" % (
                case["name"], len(case["v"]), case["lds_rows"], "+".join(storage(case, 1, maxf)), "+".join(storage(case, 2, maxf)), h["feasible"], k,
                ints("steps"), ints("dropped"), ints("dropped_mid"), ints("excluded"), ints("active")))
    if verbose:
        for key in sorted(regimes):
            print("wps %d, %s: %s" % (key[0], key[1], ", ".join("%s: %s" % kv for kv in sorted(regimes[key].items()))))
        print("anywhere: %s" % ", ".join("%s: %s" % kv for kv in sorted(anywhere.items())))
    want = {"dropped_mid", "attempt0", "attempt1", "attempt2", "attempt3", "none", "content bl"}
    for wps in (1, 2):
        for rows in ("registers", "lds", "global", "global flags"):
            missing = want - set(regimes.get((wps, rows), {}))
            assert not missing, "no case of the %d-wave build with %s does: %s" % (wps, rows, sorted(missing))
    missing = {"excluded", "full_active_set", "more_than_18_steps"} - set(anywhere)
    assert not missing, "no case does: %s" % sorted(missing)


def _cpu_body(maxf, what):
    {"attempts": check_attempts, "certificates": check_certificates, "coverage": lambda f: check_coverage(f, host_results(f))}[what](maxf)
    print("qp host ok", flush=True)


def _run_k128(code):
    env = dict(os.environ, ARMOUR_KEY128="1")
    env.pop("ARMOUR_HIP_LIB", None)
    return subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_qp_device as t; %s" % (
        ROOT, os.path.join(ROOT, "tests"), code)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("what", ["attempts", "certificates", "coverage"])
def test_host_qp(what):
    _cpu_body(7, what)


@pytest.mark.parametrize("what", ["attempts", "certificates", "coverage"])
def test_host_qp_8_factor_abi(what):
    r = _run_k128("t._cpu_body(8, %r)" % what)
    assert r.returncode == 0 and "qp host ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------- GPU: device == host, bit for bit
def _gpu_body(maxf):
    from armour_amd import _lib
    assert _lib.MAXF == maxf and _lib.load().armour_abi_max_factors() == maxf
    cases = host_results(maxf)
    bad = []
    for wps in (1, 2):
        for case, h in cases:
            g = device_qp(case, wps)
            k = h["attempt"]
            same = (np.array_equal(g["d"], h["d"]) and g["feasible"] == h["feasible"] and g["attempt"] == k and g["max_mult"] == h["max_mult"]
                    and all(g["qp_iter"][e] == h["steps"][e] for e in range(k + 1)))
            if not same:
                bad.append("%s wps=%d (%s): device %s | host %s" % (case["name"], wps, "+".join(storage(case, wps, maxf)), g, {q: h[q] for q in ("d", "feasible", "attempt", "max_mult", "steps")}))
    print("%d cases x 2 builds, %d differ" % (len(cases), len(bad)), flush=True)
    assert not bad, "\n".join(bad[:12])
    print("qp device ok", flush=True)


@pytest.mark.gpu
def test_a_joint_without_range_has_a_zero_jacobian_column():
    """what _pose assumes about the floor of hess_diag: with k_range_j = 0 the plan does not move with k_j -- Hd_j is at its floor -- and then neither
    does any constraint row or the cost: column j of the Jacobian and entry j of the cost's gradient are exactly zero, at any k"""
    from armour_amd.planner import ArmourNLP, default_params
    from armour_amd.worlds import random_k, random_problem
    j = 2
    params = default_params(20)
    params.k_range[j] = 0.0
    p = random_problem(7, 4)
    nlp = ArmourNLP(params=params).set_parameters(p["q0"], p["qd0"], p["qdd0"], p["q_des"], p["obstacles"])
    k = random_k(3, 1)
    _, jac = nlp.eval_g_jac(k)
    assert np.all(jac[0][:, j] == 0.0) and np.abs(jac[0]).max() > 0.0
    assert nlp.eval_grad_f(k)[0][j] == 0.0
    nlp.close()


@pytest.mark.gpu
def test_device_qp_equals_the_host_qp_bit_for_bit():
    _gpu_body(7)


@pytest.mark.gpu
def test_device_qp_equals_the_host_qp_bit_for_bit_8_factor_abi():
    r = _run_k128("t._gpu_body(8)")
    assert r.returncode == 0 and "qp device ok" in r.stdout, r.stdout[-4000:] + r.stderr[-3000:]
