"""The two kernels that order a trace's hand-over list between its passes (k_order_count,
k_order_place), on their own, through the library's launcher for them: the front [0, F) comes out
in non-decreasing order of its one-byte keys, the back [n - K, n) as it was, the places between
untouched.  Sizes around a wave, a word of keys, a block's chunk and the grid; fronts and backs that
are empty, whole, adjoining and apart; keys all equal, every value, descending, random."""
import ctypes as C

import numpy as np
import pytest
import torch

import turtle_amd as TA

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 100_003)
KEYS = ("equal", "every", "descending", "random")
HOLE = -7


def splits(n):
    """(F, K): nothing, all front, all back, adjoining, holes between"""
    some = [(0, 0), (n, 0), (0, n), (n - n // 3, n // 3)]
    if n >= 3:
        some.append((n // 2, n // 4))
    else:
        some.append((n - 1, 0))          # (two places at the most: a hole behind the front)
    return sorted(set(some))


def front_keys(kind, count, rng):
    if kind == "equal":
        return np.full(count, 17, dtype=np.uint8)
    if kind == "every":
        return rng.permutation(np.arange(count) % 254).astype(np.uint8)
    if kind == "descending":
        return (253 - (np.arange(count) * 254 // max(count, 1))).astype(np.uint8)
    return rng.integers(0, 254, count).astype(np.uint8)


def order(ids, keys, n_front, n_back):
    """one run of the two kernels over device copies; -> the list they wrote (host)"""
    n = ids.shape[0]
    d_ids = torch.as_tensor(ids, device="cuda")
    d_keys = torch.as_tensor(keys, device="cuda")
    d_front = torch.tensor([n_front], dtype=torch.int64, device="cuda")
    d_back = torch.tensor([n_back], dtype=torch.int64, device="cuda")
    words = torch.zeros(512, dtype=torch.int32, device="cuda")
    out = torch.full((n,), HOLE, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = TA.lib().tamd_k_hand_over_order(
        C.c_long(n), C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_keys.data_ptr()), C.c_void_p(d_front.data_ptr()),
        C.c_void_p(d_back.data_ptr()), C.c_void_p(words.data_ptr()), C.c_void_p(out.data_ptr()))
    assert rc == 0
    TA.synchronize()
    counts = words[:256].cpu().numpy()
    assert np.array_equal(counts, np.bincount(keys[:n_front], minlength=256)), "the counts"
    assert np.array_equal(words[256:].cpu().numpy(), counts), "every bin's cursor ends at its count"
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", KEYS)
@pytest.mark.parametrize("n", SIZES)
def test_front_in_key_order_back_as_it_was(n, kind):
    rng = np.random.default_rng(n)
    for n_front, n_back in splits(n):
        ids = rng.permutation(n).astype(np.int32)           # a ray is listed once
        # (the keys of the holes are whatever the memory held: nothing may read them)
        keys = rng.integers(0, 256, n).astype(np.uint8)
        keys[:n_front] = front_keys(kind, n_front, rng)
        keys[n - n_back:] = 255
        key_of = np.zeros(n, dtype=np.uint8)
        key_of[ids] = keys
        out = order(ids, keys, n_front, n_back)
        where = (n, kind, n_front, n_back)
        front = out[:n_front]
        assert np.all(np.diff(key_of[front].astype(np.int32)) >= 0), where
        assert np.array_equal(np.sort(front), np.sort(ids[:n_front])), where
        assert np.array_equal(out[n - n_back:], ids[n - n_back:]), where
        assert np.all(out[n_front:n - n_back] == HOLE), where
        # ties come out in any order: a second run gives the same ids under every key
        again = order(ids, keys, n_front, n_back)
        for run in (out, again):
            assert np.array_equal(key_of[run[:n_front]], np.sort(keys[:n_front])), where
        same = np.lexsort((front, key_of[front])), np.lexsort((again[:n_front], key_of[again[:n_front]]))
        assert np.array_equal(front[same[0]], again[:n_front][same[1]]), where


def test_counters_beyond_the_list_write_nothing_outside_it():
    """the lengths are read on the device and held to the list's n places"""
    n = 257
    rng = np.random.default_rng(5)
    ids = rng.permutation(n).astype(np.int32)
    keys = rng.integers(0, 254, n).astype(np.uint8)
    d_ids, d_keys = torch.as_tensor(ids, device="cuda"), torch.as_tensor(keys, device="cuda")
    d_front = torch.tensor([n + 1000], dtype=torch.int64, device="cuda")
    d_back = torch.tensor([5], dtype=torch.int64, device="cuda")
    words = torch.zeros(512, dtype=torch.int32, device="cuda")
    out = torch.full((n + 64,), HOLE, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert TA.lib().tamd_k_hand_over_order(
        C.c_long(n), C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_keys.data_ptr()), C.c_void_p(d_front.data_ptr()),
        C.c_void_p(d_back.data_ptr()), C.c_void_p(words.data_ptr()), C.c_void_p(out.data_ptr())) == 0
    TA.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:] == HOLE)
    assert np.array_equal(np.sort(got[:n]), np.arange(n))
