"""The block steps under the four per-world planner kernels (armour_amd/csrc/tree_block.h), tested directly.

The kernels' twin tests reach ties between waves, lone lanes and empty flags only by luck of their random inputs; here each is a case.
armour_debug_block_steps runs every cooperative step once in one block of 256 lanes and is compared with numpy exactly (integers, and a
minimum that is one of the inputs).  The obstacle split and the owner search are host-callable functions and are compared with brute force
on the CPU."""
import ctypes as C

import numpy as np
import pytest

BLOCK, NONE = 256, 2**31 - 1


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def run_steps(d, v, flag, n):
    from armour_amd import _lib
    L = _lib.load()
    d = np.ascontiguousarray(d, dtype=np.float64).reshape(BLOCK)
    v, flag, n = (np.ascontiguousarray(a, dtype=np.int32).reshape(BLOCK) for a in (v, flag, n))
    min_d = C.c_double()
    min_v, first, any_, total = (C.c_int32() for _ in range(4))
    sums = np.zeros(BLOCK, dtype=np.int32)
    _lib.check(L.armour_debug_block_steps(_lib._dp(d), _ip(v), _ip(flag), _ip(n), C.byref(min_d), C.byref(min_v), C.byref(first), C.byref(any_), _ip(sums),
                                          C.byref(total)))
    return dict(min_d=min_d.value, min_v=min_v.value, first=first.value, any=any_.value, sums=sums, total=total.value)


def expect_steps(d, v, flag, n):
    d, v, flag, n = np.asarray(d, dtype=np.float64), np.asarray(v, dtype=np.int64), np.asarray(flag), np.asarray(n, dtype=np.int64)
    k = np.lexsort((v, d))[0]                                   # the order key_less: d, then v
    set_ = np.nonzero(flag)[0]
    return dict(min_d=float(d[k]), min_v=int(v[k]), first=int(set_[0]) if set_.size else NONE, any=int(set_.size > 0), sums=np.cumsum(n), total=int(n.sum()))


def no_keys():
    return np.full(BLOCK, np.inf), np.full(BLOCK, NONE)


def keys_tie_across_waves():
    """equal d in lanes of waves 1 and 2, the smaller v in the later wave; every other key is larger"""
    d, v = np.arange(BLOCK, dtype=np.float64) + 10.0, np.arange(BLOCK) + 1000
    d[70], v[70] = 3.0, 500
    d[130], v[130] = 3.0, 7
    return d, v


def keys_lane_255():
    d, v = no_keys()
    d[255], v[255] = 2.5, 41
    return d, v


def keys_random():
    rng = np.random.default_rng(5)
    return rng.integers(0, 8, BLOCK).astype(np.float64), rng.permutation(BLOCK)   # many equal d, distinct v


def flag_in(*lanes):
    f = np.zeros(BLOCK, dtype=np.int32)
    f[list(lanes)] = 1
    return f


def terms_wave_sums():
    """wave sums 0, 64, 1, 63"""
    n = np.zeros(BLOCK, dtype=np.int32)
    n[64:128] = 1
    n[128 + 17] = 1
    n[192:256] = 1
    n[192 + 30] = 0
    return n


def terms_wave_3():
    n = np.zeros(BLOCK, dtype=np.int32)
    n[192:] = 1
    return n


KEYS = {"tie_across_waves": keys_tie_across_waves, "no_keys": no_keys, "lane_255": keys_lane_255, "random": keys_random}
FLAGS = {"lane_0": flag_in(0), "lane_64": flag_in(64), "lane_255": flag_in(255), "none": flag_in(), "lanes_70_200": flag_in(70, 200)}
TERMS = {"ones": np.ones(BLOCK, dtype=np.int32), "wave_3": terms_wave_3(), "zero": np.zeros(BLOCK, dtype=np.int32), "wave_sums_0_64_1_63": terms_wave_sums(),
         "mixed": (np.arange(BLOCK) * 7 % 5).astype(np.int32)}
# every case of each step once; the three steps of a launch do not see each other's inputs
CASES = [("tie_across_waves", "lane_0", "ones"), ("no_keys", "lane_64", "wave_3"), ("lane_255", "lane_255", "zero"), ("random", "none", "wave_sums_0_64_1_63"),
         ("tie_across_waves", "lanes_70_200", "mixed")]


@pytest.mark.gpu
@pytest.mark.parametrize("keys,flags,terms", CASES)
def test_block_steps_against_numpy(keys, flags, terms):
    d, v = KEYS[keys]()
    got, want = run_steps(d, v, FLAGS[flags], TERMS[terms]), expect_steps(d, v, FLAGS[flags], TERMS[terms])
    print(keys, flags, terms, {k: x for k, x in got.items() if k != "sums"})
    if keys == "tie_across_waves":
        assert (want["min_d"], want["min_v"]) == (3.0, 7)
    if terms == "wave_sums_0_64_1_63":
        assert [int(TERMS[terms][64 * w:64 * w + 64].sum()) for w in range(4)] == [0, 64, 1, 63]
    for k in ("min_d", "min_v", "first", "any", "total"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["sums"], want["sums"])


def test_obstacle_split_against_brute_force():
    """items 1..256 x O in {0, 1, 2, 13, 14, 50} x allowed: G as the rule states it, and the G lanes of every item cover [0, O) once, in order"""
    from armour_amd import _lib
    L = _lib.load()
    split = np.zeros((BLOCK, 4), dtype=np.int32)
    t = np.arange(BLOCK)
    for items in range(1, BLOCK + 1):
        for O in (0, 1, 2, 13, 14, 50):
            for allowed in (0, 1):
                _lib.check(L.armour_debug_block_split(items, O, allowed, _ip(split)))
                G = min(O, BLOCK // items) if allowed and 2 * items <= BLOCK and O > 1 else 1
                assert G >= 1 and (split[:, 0] == G).all() and (split[:, 1] == BLOCK // G).all(), (items, O, allowed)
                g = t % G
                assert np.array_equal(split[:, 2], g * O // G) and np.array_equal(split[:, 3], (g + 1) * O // G), (items, O, allowed)
                assert G * min(items, BLOCK // G) <= BLOCK
                for item in {0, min(items, BLOCK // G) - 1}:    # the lanes item * G .. item * G + G - 1 partition the obstacles
                    rows = split[item * G:(item + 1) * G]
                    covered = np.concatenate([np.arange(a, b) for a, b in rows[:, 2:]]) if O else np.zeros(0, dtype=int)
                    assert np.array_equal(covered, np.arange(O)), (items, O, allowed, item)


def test_item_owner_against_brute_force():
    """ascending end[] with equal neighbours (candidates without items), n = 1 .. 256: the owner of every item is the first end above it"""
    from armour_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 63, 64, 65, 255, 256):
        for trial in range(4):
            widths = rng.integers(0, 4, n) if trial else np.ones(n, dtype=np.int64)   # width 0: end[k] == end[k - 1]
            if trial == 3:
                widths[:] = 0
                widths[n // 2] = 5
            end = np.ascontiguousarray(np.cumsum(widths), dtype=np.int32)
            item = np.arange(-1, int(end[-1]) + 2, dtype=np.int32)                   # one below and two past the items
            owner = np.zeros(item.size, dtype=np.int32)
            _lib.check(L.armour_debug_block_owner(_ip(end), n, item.size, _ip(item), _ip(owner)))
            want = np.array([next((k for k in range(n) if end[k] > i), n) for i in item])
            assert np.array_equal(owner, want), (n, trial)
            assert np.array_equal(owner, np.searchsorted(end, item, side="right"))
