"""CPU: the dirty rule of incremental meshing — the oracle's key-shift form against its brute-force geometric form,
the Morton parent identity the shift relies on, and the host logic that decides when update_octree_mesh's cache is rebuilt."""
import types

import numpy as np
import pytest

import mesh_cache_oracle as mo


def _random_change(rng, keys, ids, rows):
    """a previous state: some nodes of every slot are new, a few rows changed"""
    prev = [int(rng.integers(max(1, len(k) // 2), len(k) + 1)) for k in keys]
    flags = [rng.random(r) < 0.02 for r in rows]
    return prev, flags


@pytest.mark.parametrize("sq", [0, 1, 2])
@pytest.mark.parametrize("seed", range(6))
def test_shift_form_equals_the_brute_force_form_on_random_octrees(sq, seed):
    rng = np.random.default_rng(100 * sq + seed)
    keys, ids, rows = mo.random_octree(rng, int(rng.integers(50, 301)), L=3, span=int(rng.choice([6, 8, 16])))
    assert 30 <= len(keys[2]) <= 300
    prev, flags = _random_change(rng, keys, ids, rows)
    if seed == 0:  # only new nodes, no changed row
        flags = [np.zeros(r, bool) for r in rows]
    if seed == 1:  # only changed rows, no new node
        prev = [len(k) for k in keys]
    a = mo.dirty_query_nodes(keys, ids, prev, flags, sq)
    b = mo.dirty_query_nodes_brute(keys, ids, prev, flags, sq)
    print("sq %d seed %d: %d / %d query nodes dirty" % (sq, seed, a.sum(), len(a)))
    assert np.array_equal(a, b)
    assert a.sum() > 0


def test_nothing_changed_marks_nothing():
    rng = np.random.default_rng(7)
    keys, ids, rows = mo.random_octree(rng, 200)
    for sq in range(3):
        d = mo.dirty_query_nodes(keys, ids, [len(k) for k in keys], [np.zeros(r, bool) for r in rows], sq)
        assert not d.any()
        assert not mo.dirty_query_nodes_brute(keys, ids, [len(k) for k in keys], [np.zeros(r, bool) for r in rows], sq).any()


def test_the_parent_of_a_morton_key_is_the_key_shifted_by_three():
    from shine_mapping_amd.feature_octree import morton_decode, morton_encode

    rng = np.random.default_rng(3)
    xyz = rng.integers(0, 1 << 15, (5000, 3))
    key = morton_encode(xyz)
    assert np.array_equal(morton_decode(key >> 3), xyz >> 1)
    assert np.array_equal(morton_decode(key >> 9), xyz >> 3)
    assert np.array_equal(morton_encode(xyz >> 1), key >> 3)
    # the oracle's own bit-by-bit code agrees with the package's
    assert np.array_equal(mo.decode(key), xyz) and np.array_equal(mo.encode(xyz), key)


def test_changed_rows_is_bitwise_and_skips_the_trash_row():
    t = np.zeros((5, 8), np.float32)
    t[1, 7] = np.nan
    snap = t[:-1].copy()
    assert not mo.changed_rows(t, snap).any()  # an identical NaN is unchanged
    u = t.copy()
    u[4] = 9.0  # the trash row only
    assert not mo.changed_rows(u, snap).any()
    u[2, 3] = -0.0
    assert mo.changed_rows(u, snap).tolist() == [False, False, True, False]
    assert mo.changed_rows(t, snap[:2]).tolist() == [False, False, True, True]  # beyond the snapshot


def _ids(n, first=0):
    return (np.arange(first, first + 8 * n, dtype=np.int32).reshape(n, 8))


def _cached(key, node_keys, snap_rows, node_ids=None):
    node_keys = [np.asarray(k, np.int64) for k in node_keys]
    return types.SimpleNamespace(key=key, node_keys=node_keys, snap_rows=snap_rows,
                                 node_ids=node_ids if node_ids is not None else [_ids(len(k)) for k in node_keys])


def test_prefix_and_shrink_detection():
    from shine_mapping_amd.mesher import keys_are_prefix, mesh_cache_rebuild_reason

    assert keys_are_prefix(np.array([5, 3, 9]), np.array([5, 3, 9]))
    assert keys_are_prefix(np.array([5, 3, 9]), np.array([5, 3, 9, 1, 2]))
    assert keys_are_prefix(np.zeros(0, np.int64), np.array([1]))
    assert not keys_are_prefix(np.array([5, 3, 9]), np.array([5, 3]))  # shrank
    assert not keys_are_prefix(np.array([5, 3, 9]), np.array([3, 5, 9, 1]))  # the same set in another order
    assert not keys_are_prefix(np.array([5, 3, 9]), np.array([5, 3, 8, 9]))
    assert keys_are_prefix(_ids(2), _ids(3)) and not keys_are_prefix(_ids(2), _ids(3, 1))  # [n, 8] corner ids alike

    key = ("k",)
    c = _cached(key, [[7, 8], [5, 3, 9]], [10, 20])  # two levels; the query level may be either
    same = lambda: True
    A = np.array
    assert mesh_cache_rebuild_reason(c, key, same, [A([7, 8]), A([5, 3, 9, 4])], [_ids(2), _ids(4)], [10, 25]) is None
    assert mesh_cache_rebuild_reason(c, key, same, [A([7, 8]), A([5, 3, 9])], [_ids(2), _ids(3)], [10, 20]) is None
    assert mesh_cache_rebuild_reason(c, key, same, [A([7, 8]), A([5, 9, 3])], [_ids(2), _ids(3)], [10, 20]) == "octree"
    assert mesh_cache_rebuild_reason(c, key, same, [A([8, 7]), A([5, 3, 9])], [_ids(2), _ids(3)], [10, 20]) == "octree"  # ANOTHER level reordered
    assert mesh_cache_rebuild_reason(c, key, same, [A([7, 8]), A([5, 3, 9])], [_ids(2), _ids(3, 1)], [10, 20]) == "octree"  # corner ids replaced
    assert mesh_cache_rebuild_reason(c, key, same, [A([7, 8]), A([5, 3, 9])], [_ids(2), _ids(3)], [10, 19]) == "octree"  # a level's rows shrank
    assert mesh_cache_rebuild_reason(c, key, same, [A([7]), A([5, 3, 9])], [_ids(1), _ids(3)], [10, 20]) == "octree"  # a level's nodes shrank


def test_rebuild_reasons_and_their_order():
    from shine_mapping_amd.mesher import mesh_cache_key, mesh_cache_rebuild_reason

    def never():
        raise AssertionError("the decoder is compared only under a matching key")

    key = mesh_cache_key(9, 4, 2.0 ** -8 / 4, True, 2, 0.02)
    assert mesh_cache_rebuild_reason(None, key, never, [np.zeros(0)], [_ids(0)], [0]) == "first"
    c = _cached(key, [[1, 2]], [4])
    cur = ([np.array([1, 2])], [_ids(2)], [4])
    swapped = ([np.array([2, 1])], [_ids(2)], [4])
    for other in (mesh_cache_key(10, 4, 2.0 ** -8 / 4, True, 2, 0.02), mesh_cache_key(9, 5, 2.0 ** -8 / 4, True, 2, 0.02),
                  mesh_cache_key(9, 4, 2.0 ** -8 / 5, True, 2, 0.02), mesh_cache_key(9, 4, 2.0 ** -8 / 4, False, 2, 0.02),
                  mesh_cache_key(9, 4, 2.0 ** -8 / 4, True, 1, 0.02), mesh_cache_key(9, 4, 2.0 ** -8 / 4, True, 2, 0.04)):
        assert other != key
        assert mesh_cache_rebuild_reason(c, other, never, *cur) == "key"
    assert mesh_cache_key(np.int64(9), 4.0, np.float64(2.0 ** -8 / 4), 1, np.int32(2), 0.02) == key  # (number types do not matter)
    assert mesh_cache_rebuild_reason(c, key, lambda: False, *cur) == "decoder"
    assert mesh_cache_rebuild_reason(c, key, lambda: False, *swapped) == "decoder"  # (before "octree")
    assert mesh_cache_rebuild_reason(c, key, lambda: True, *swapped) == "octree"
    assert mesh_cache_rebuild_reason(c, key, lambda: True, [np.array([1, 2, 3])], [_ids(3)], [6]) is None


def test_capacity_grows_geometrically():
    from shine_mapping_amd.mesher import grown_capacity

    assert grown_capacity(100, 100) == 100 and grown_capacity(100, 60) == 100
    assert grown_capacity(100, 101) == 200 and grown_capacity(100, 500) == 500 and grown_capacity(0, 3) == 16
    cap, copies = 0, 0
    for need in range(1, 5000):
        new = grown_capacity(cap, need)
        copies += new != cap
        cap = new
    assert copies <= 10
