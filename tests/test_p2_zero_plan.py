"""When may an exact-layout (EX) launch of the fused evaluation drop its scan's zero-normal test?  The rule of armour_p2_plan, without a device.

The reach-set build hands the plan two masks per problem: skip (bit p: plane p is never needed by a row of the problem) and zero (bit p: plane p
has the zero normal in at least one row).  The launch takes the kernel without the test only if it is an EX launch and zero & ~skip is empty over
the 36 planes for EVERY problem; bits of skipped planes carry no meaning.  armour_debug_p2_zero_plan_shape runs the plan for a table shape and
given masks and returns {EX launch, test dropped}.
"""
import ctypes as C

import numpy as np
import pytest

NPLANES = 36
BOX_LIVE = list(range(0, 12)) + list(range(21, 33))   # the live planes of a world of axis-aligned boxes (tests/test_p2_plan_addressing.py)
T, J, N, O, CAPL, MAX_LINK = 2, 7, 7, 20, 8, 8         # the shape of tests/golden/make_p2_ex_rows.py at O = 20


def bits(planes):
    return sum(1 << p for p in planes)


def skip_mask(live):
    return bits(p for p in range(NPLANES) if p not in live)


def zero_plan(skip, zero, O=O, recompute_d=0):
    from armour_amd import _lib
    L = _lib.load()
    s, z = np.array(skip, dtype=np.uint64), np.array(zero, dtype=np.uint64)
    assert s.shape == z.shape and s.ndim == 1
    v = np.full(2, -1, dtype=np.int32)
    u64 = C.POINTER(C.c_uint64)
    _lib.check(L.armour_debug_p2_zero_plan_shape(len(s), T, J, N, O, CAPL, MAX_LINK, recompute_d, s.ctypes.data_as(u64), z.ctypes.data_as(u64),
                                                 v.ctypes.data_as(C.POINTER(C.c_int32))))
    return int(v[0]), int(v[1])


BOX = skip_mask(BOX_LIVE)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_no_zero_bit_anywhere_drops_the_test(B):
    assert zero_plan([BOX] * B, [0] * B, recompute_d=int(B >= 8)) == (1, 1)


def test_zero_bits_on_skipped_planes_carry_no_meaning():
    assert zero_plan([BOX] * 3, [BOX, 0, bits([12, 35])]) == (1, 1)
    # ... whatever lies above the 36 planes included
    assert zero_plan([BOX], [BOX | (0xfffffff << NPLANES)]) == (1, 1)


@pytest.mark.parametrize("b", [0, 1, 2])
@pytest.mark.parametrize("p", [BOX_LIVE[0], BOX_LIVE[11], BOX_LIVE[12], BOX_LIVE[23]])
def test_one_zero_bit_on_a_live_plane_of_one_problem_keeps_the_test(b, p):
    zero = [BOX, 0, BOX]
    zero[b] |= 1 << p
    assert zero_plan([BOX] * 3, zero) == (1, 0)


def test_a_launch_that_is_not_ex_keeps_the_test():
    # 25 live planes: the nine-slot kernel;  24 in no EX layout: the six-slot kernel;  O = 1: no one-pass slicing
    assert zero_plan([skip_mask(BOX_LIVE + [12])], [0]) == (0, 0)
    assert zero_plan([skip_mask(list(range(0, 12)) + list(range(22, 34)))], [0]) == (0, 0)
    assert zero_plan([BOX], [0], O=1) == (0, 0)


def test_all_ones_masks_keep_the_test():
    """What a handle reports whose masks do not come from the build (loaded tables: skip 0, zero all ones) -- and all ones in both."""
    ones = (1 << 64) - 1
    assert zero_plan([0], [ones]) == (0, 0)
    assert zero_plan([BOX] * 3, [ones] * 3) == (1, 0)
    assert zero_plan([ones], [ones])[1] == 0
