"""Argument errors of the Poseidon and Merkle entry points (ronk_poseidon_*, ronk_merkle_*): all of them are refused before any
device work, so this runs without a GPU.  Also the tree-layout helpers and the host-side opening, which are integer logic."""
import ctypes as C

import numpy as np
import pytest

P = 0xFFFFFFFF00000001
NAMES = ("ronk_poseidon_create", "ronk_poseidon_destroy", "ronk_poseidon_permute_dev", "ronk_poseidon_hash", "ronk_poseidon_sponge_dev",
         "ronk_merkle_tree_words", "ronk_merkle_level_offset", "ronk_merkle_commit_dev", "ronk_merkle_open_dev",
         "ronk_merkle_verify_dev", "ronk_merkle_commit", "ronk_merkle_open", "ronk_merkle_verify")


@pytest.fixture(scope="module")
def L():
    from ronkathon_amd import _lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_exported(L):
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(L.lib, name)


def test_create_arguments(L):
    f = L.lib.ronk_poseidon_create
    h = C.c_void_p()
    rc, mds = np.zeros(17 * 17 * 4, np.uint64), np.ones(17 * 17, np.uint64)
    assert f(None, P, 3, 5, 2, 2, 2, _p(rc), _p(mds)) == L.ERR_INVALID
    assert f(C.byref(h), P, 3, 5, 2, 2, 2, None, _p(mds)) == L.ERR_INVALID
    assert f(C.byref(h), P, 3, 5, 2, 2, 2, _p(rc), None) == L.ERR_INVALID
    assert f(C.byref(h), P, 1, 5, 2, 2, 1, _p(rc), _p(mds)) == L.ERR_INVALID         # width < 2
    assert f(C.byref(h), P, 0, 5, 2, 2, 1, _p(rc), _p(mds)) == L.ERR_INVALID
    assert f(C.byref(h), P, 17, 5, 2, 2, 1, _p(rc), _p(mds)) == L.ERR_UNSUPPORTED    # width > 16
    assert f(C.byref(h), P, 3, 5, 2, 2, 0, _p(rc), _p(mds)) == L.ERR_INVALID         # rate < 1
    assert f(C.byref(h), P, 3, 5, 2, 2, 3, _p(rc), _p(mds)) == L.ERR_INVALID         # rate == width
    assert f(C.byref(h), P, 3, 0, 2, 2, 2, _p(rc), _p(mds)) == L.ERR_INVALID         # alpha < 1
    assert f(C.byref(h), 91, 3, 5, 2, 2, 2, _p(rc), _p(mds)) == L.ERR_NOT_PRIME      # 7 * 13
    assert f(C.byref(h), 100, 3, 5, 2, 2, 2, _p(rc), _p(mds)) == L.ERR_NOT_PRIME
    assert f(C.byref(h), P - 2, 3, 5, 2, 2, 2, _p(rc), _p(mds)) == L.ERR_NOT_PRIME
    assert f(C.byref(h), 2, 3, 5, 2, 2, 2, _p(rc), _p(mds)) == L.ERR_UNSUPPORTED
    assert not h.value
    if L.device_count() == 0:
        # valid arguments, odd num_f included: only the device is missing
        assert f(C.byref(h), P, 3, 5, 2, 3, 2, _p(rc), _p(mds)) == L.ERR_NO_DEVICE
        assert f(C.byref(h), 101, 16, 3, 11, 8, 15, _p(rc), _p(mds)) == L.ERR_NO_DEVICE
    assert L.lib.ronk_poseidon_destroy(None) == L.ERR_INVALID


def test_null_handles_and_pointers(L):
    d = C.c_void_p(16)   # never dereferenced: refused first
    assert L.lib.ronk_poseidon_permute_dev(None, d, 4, None) == L.ERR_INVALID
    assert L.lib.ronk_poseidon_hash(None, d, 1, d) == L.ERR_INVALID
    assert L.lib.ronk_poseidon_sponge_dev(None, d, 4, 3, 3, 1, d, 1, None) == L.ERR_INVALID
    assert L.lib.ronk_merkle_commit_dev(None, d, 4, 3, 3, 1, 1, d, None) == L.ERR_INVALID
    assert L.lib.ronk_merkle_verify_dev(None, d, 1, 3, 3, 1, d, d, 4, 1, d, d, None) == L.ERR_INVALID
    assert L.lib.ronk_merkle_commit(None, d, 4, 3, 1, d) == L.ERR_INVALID
    assert L.lib.ronk_merkle_verify(None, d, 1, 3, d, d, 4, 1, d, d) == L.ERR_INVALID
    g = L.lib.ronk_merkle_open_dev
    assert g(None, 4, 1, d, 1, d, d, None) == L.ERR_INVALID          # d_tree
    assert g(d, 0, 1, d, 1, d, d, None) == L.ERR_INVALID             # n_leaves == 0
    assert g(d, 4, 0, d, 1, d, d, None) == L.ERR_INVALID             # digest_len == 0
    assert g(d, 4, 1, None, 1, d, d, None) == L.ERR_INVALID          # d_indices
    assert g(d, 4, 1, d, 1, None, d, None) == L.ERR_INVALID          # d_paths with a non-empty path
    assert g(d, 4, 1, d, 1, d, None, None) == L.ERR_INVALID          # d_status
    assert g(d, 4, 1, None, 0, None, None, None) == L.OK             # nothing asked


def test_tree_layout(L):
    words, off = L.lib.ronk_merkle_tree_words, L.lib.ronk_merkle_level_offset
    assert words(0, 4) == 0
    assert words(1, 4) == 4 and off(1, 4, 0) == 0 and off(1, 4, 1) == 4
    assert words(2, 3) == 9 and off(2, 3, 1) == 6
    # 5 -> 3 -> 2 -> 1
    assert words(5, 2) == 22 and [off(5, 2, l) for l in range(5)] == [0, 10, 16, 20, 22]
    assert words(1 << 20, 4) == 4 * ((1 << 21) - 1)
    # 5000, 2500, 1250, 625, 313, 157, 79, 40, 20, 10, 5, 3, 2, 1
    sizes = [5000, 2500, 1250, 625, 313, 157, 79, 40, 20, 10, 5, 3, 2, 1]
    assert words(5000, 1) == sum(sizes) and off(5000, 1, 4) == sum(sizes[:4]) and off(5000, 1, 99) == sum(sizes)


def test_host_open(L):
    """ronk_merkle_open walks a host tree: sibling digests from the bottom up, RONK_ERR_INDEX where the reference panics"""
    n, d = 5, 2
    tree = np.arange(100, 122, dtype=np.uint64)          # 22 words: levels of 5, 3, 2, 1 nodes
    idx = np.array([0, 1, 3, 4, 5], dtype=np.uint64)
    paths = np.full(idx.size * 3 * d, 7, dtype=np.uint64)
    st = (C.c_int * idx.size)()
    f = L.lib.ronk_merkle_open
    assert f(_p(tree), n, d, _p(idx), idx.size, _p(paths), st) == L.OK
    assert list(st) == [0, 0, 0, L.ERR_INDEX, L.ERR_INDEX]       # 4: the unpaired last leaf; 5: out of range
    pa = paths.reshape(idx.size, 3, d)
    assert pa[0].tolist() == [[102, 103], [112, 113], [118, 119]]   # leaf 1, level-1 node 1, level-2 node 1
    assert pa[1].tolist() == [[100, 101], [112, 113], [118, 119]]
    assert pa[2].tolist() == [[104, 105], [110, 111], [118, 119]]   # leaf 2, level-1 node 0, level-2 node 1
    assert not pa[3].any() and not pa[4].any()
    assert f(None, n, d, _p(idx), 1, _p(paths), st) == L.ERR_INVALID
    assert f(_p(tree), 0, d, _p(idx), 1, _p(paths), st) == L.ERR_INVALID
    assert f(_p(tree), n, d, _p(idx), 1, None, st) == L.ERR_INVALID
    one = np.array([0], dtype=np.uint64)
    assert f(_p(tree), 1, d, _p(one), 1, None, st) == L.OK and st[0] == 0    # one leaf: an empty path
