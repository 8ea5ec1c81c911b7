"""The plane-table addressing armour_p2_plan hands the exact-layout (EX) kernels, against a restatement of common.h's layout (no GPU).

armour_debug_p2_plan_shape runs the plan for a table shape and a set of live-plane masks without a handle or a device and returns its verdict
and the scalars the collision block adds to its 64-bit base per problem.  Here every one of them is recomputed from the layout's definition
(armour_row_stride, the section offsets and armour_plane_index, restated in numpy below) and compared exactly; the shapes cover the row-stride
rounding (Q = 1, 63, 64, 65), the suite's O = 20 shape, the largest Q the kernel takes, a mask that is no EX layout, two problems with different
masks (the kernel must then walk each problem's mask, as before) and tables past the 32-bit range (no EX launch).
"""
import ctypes as C

import numpy as np
import pytest

NPLANES, FIRST_LL, LL_RECORD = 36, 21, 48
# axis-aligned boxes: the planes pairing two obstacle generators among themselves (12..20) and the last three link x link planes are skipped
BOX_LIVE = list(range(0, 12)) + list(range(21, 33))


def skip_mask(live):
    return np.uint64(sum(1 << p for p in range(NPLANES) if p not in live))


# ---- common.h, restated
def row_stride(Q):
    return (Q + 15) & ~15


def section_offsets(Q):
    """Doubles from the start of one problem's table: CD, DLL, D, the whole table."""
    Qs = row_stride(Q)
    return 2 * NPLANES * Qs, 4 * NPLANES * Qs, (4 * NPLANES + 16) * Qs, (5 * NPLANES + 16) * Qs


def plane_index(Q, q, p, c):
    Qs = row_stride(Q)
    cd, dll, d, _ = section_offsets(Q)
    if c < 2:
        return (p * Qs + q) * 2 + c
    if c == 2:
        return cd + (p * Qs + q) * 2
    if c == 3:
        return d + p * Qs + q
    if p < FIRST_LL:
        return cd + (p * Qs + q) * 2 + 1
    return dll + (((p - FIRST_LL) >> 1) * Qs + q) * 2 + ((p - FIRST_LL) & 1)


def plan(B, T, J, n, O, capL, max_link, masks, recompute_d=0):
    from armour_amd import _lib
    L = _lib.load()
    v = np.zeros(6, dtype=np.int32); f = np.zeros(20, dtype=np.uint32)
    m = np.ascontiguousarray(masks, dtype=np.uint64)
    assert m.shape == (B,)
    _lib.check(L.armour_debug_p2_plan_shape(B, T, J, n, O, capL, max_link, recompute_d, m.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            v.ctypes.data_as(C.POINTER(C.c_int32)), f.ctypes.data_as(C.POINTER(C.c_uint32))))
    return dict(zip(("dfc", "six", "exact", "arg_bytes", "shared", "by_value"), (int(x) for x in v))), [int(x) for x in f]


def expected_fields(Q, JT, live, shared=True):
    """The 20 fields of an EX launch, from the layout: every offset is the byte address of row 0 of the named plane and component."""
    cd, dll, d, whole = section_offsets(Q)
    plane_bytes = (plane_index(Q, 0, 1, 0) - plane_index(Q, 0, 0, 0)) * 8
    f = [plane_bytes, cd * 8, dll * 8, d * 8, whole * 8, LL_RECORD * JT * 8]
    order = sorted(live)
    if not shared:
        return f + [0] * 14
    f += [plane_index(Q, 0, p, 0) * 8 for p in order[:12]]
    f += [order[12] - FIRST_LL, order[18] - FIRST_LL]
    return f


# Q = J * T * O; an EX launch slices a block's (link, time step) pairs in one pass, 63 / O + 2 <= 10 of them, so O >= 8 -- except at Q = 1
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 1120, (1 << 20) - 1])
def test_offsets_are_the_layouts(Q):
    shapes = {1: (1, 1, 1), 63: (3, 1, 21), 64: (1, 1, 64), 65: (5, 1, 13), 1120: (7, 8, 20), (1 << 20) - 1: (1, 1, (1 << 20) - 1)}
    J, T, O = shapes[Q]
    assert J * T * O == Q
    v, f = plan(1, T, J, 7, O, 8, 8, [skip_mask(BOX_LIVE)])
    if Q == 1:   # O = 1: 65 pairs per block, no one-pass slicing, hence no EX launch and no fields
        assert v["exact"] == 0 and v["six"] == 1 and f == [0] * 20
        return
    assert v == dict(dfc=0, six=1, exact=1, arg_bytes=v["arg_bytes"], shared=1, by_value=1), v
    assert f == expected_fields(Q, J * T, BOX_LIVE)
    # what the kernel builds from them is armour_plane_index of the plane table, row q: checked for the first and the last row
    pb, cd, dll, d = f[0], f[1], f[2], f[3]
    for q in (0, Q - 1):
        for w in range(2):
            for i in range(6):
                p = BOX_LIVE[6 * w + i]
                po = f[6 + 6 * w + i]
                assert po + q * 16 == plane_index(Q, q, p, 0) * 8 and po + q * 16 + 8 == plane_index(Q, q, p, 1) * 8
                assert cd + po + q * 16 == plane_index(Q, q, p, 2) * 8 and cd + po + q * 16 + 8 == plane_index(Q, q, p, 4) * 8
                assert d + po // 2 + q * 8 == plane_index(Q, q, p, 3) * 8
        for w in range(2):
            pll0 = f[18 + w]
            for i in range(6):
                p = FIRST_LL + pll0 + i
                assert p == BOX_LIVE[12 + 6 * w + i]
                assert dll + ((pll0 >> 1) + (i >> 1)) * pb + q * 16 + 8 * (i & 1) == plane_index(Q, q, p, 4) * 8
                assert d + p * (pb // 2) + q * 8 == plane_index(Q, q, p, 3) * 8
    assert f[4] < (1 << 32) and f[5] < (1 << 32)


def test_the_smallest_ex_table():
    """Q = 1 is no EX launch (above); the smallest table that is one: one link, one step, 8 obstacles (Q = 8, row stride 16)."""
    v, f = plan(1, 1, 1, 7, 8, 4, 4, [skip_mask(BOX_LIVE)])
    assert v["exact"] == 1 and f == expected_fields(8, 1, BOX_LIVE) and f[0] == 16 * 16


def test_the_arguments_grew_by_the_plan_scalars_only():
    """29 words of plan scalars: the issue's 60-100 B for the plane table plus four byte counts of the link-PZ tables."""
    v, _ = plan(1, 8, 7, 7, 20, 8, 8, [skip_mask(BOX_LIVE)])
    assert 500 < v["arg_bytes"] <= 640


def test_recomputed_d_is_reported():
    v, f = plan(8, 2, 7, 7, 20, 8, 8, [skip_mask(BOX_LIVE)] * 8, recompute_d=1)
    assert v["dfc"] == 1 and v["exact"] == 1 and v["shared"] == 1 and v["by_value"] == 1
    assert f == expected_fields(280, 14, BOX_LIVE)


def test_a_mask_that_is_no_ex_layout_takes_the_six_slot_kernel():
    live = list(range(0, 12)) + list(range(22, 34))   # the link x link planes start at an odd p - 21
    v, f = plan(1, 8, 7, 7, 20, 8, 8, [skip_mask(live)])
    assert v["six"] == 1 and v["exact"] == 0 and v["shared"] == 0 and f == [0] * 20
    v, f = plan(1, 8, 7, 7, 20, 8, 8, [np.uint64(0)])   # every plane live: the 9-slot kernel
    assert v["six"] == 0 and v["exact"] == 0 and f == [0] * 20


def test_two_problems_with_different_masks_walk_their_masks():
    other = [p for p in range(1, 13)] + list(range(21, 33))   # another EX layout: obstacle planes 1..12
    v, f = plan(2, 8, 7, 7, 20, 8, 8, [skip_mask(BOX_LIVE), skip_mask(other)])
    assert v["exact"] == 1 and v["shared"] == 0 and v["by_value"] == 0
    assert f == expected_fields(1120, 56, BOX_LIVE, shared=False)
    v, f = plan(2, 8, 7, 7, 20, 8, 8, [skip_mask(other), skip_mask(other)])
    assert v["exact"] == 1 and v["shared"] == 1 and v["by_value"] == 1 and f == expected_fields(1120, 56, other)


def test_tables_past_the_32_bit_range_are_no_ex_launch():
    """The largest table an EX block indexes is link_coeff, JT * capL * 24 B per problem: the last capL below 2^32 B is an EX launch, the next is not."""
    J, O = 7, 20
    T = ((1 << 20) - 1) // (J * O)          # the longest horizon with Q < 2^20
    JT = J * T
    cap_ok = ((1 << 32) - 1) // (JT * 24)
    assert JT * cap_ok * 24 < (1 << 32) <= JT * (cap_ok + 1) * 24
    v, f = plan(1, T, J, 7, O, cap_ok, 8, [skip_mask(BOX_LIVE)])
    assert v["exact"] == 1 and f == expected_fields(J * T * O, JT, BOX_LIVE)
    v, f = plan(1, T, J, 7, O, cap_ok + 1, 8, [skip_mask(BOX_LIVE)])
    assert v["six"] == 1 and v["exact"] == 0 and v["shared"] == 0 and f == [0] * 20
    # and Q itself past 2^20 is refused with the capacity error, as before
    from armour_amd import _lib
    with pytest.raises(_lib.ArmourError):
        plan(1, T + 1, J, 7, O, 8, 8, [skip_mask(BOX_LIVE)])
