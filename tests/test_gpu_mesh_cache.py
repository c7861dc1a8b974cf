"""GPU: incremental meshing.  The three kernels of csrc/shine_mesh_cache.hip against numpy / the dirty-rule oracle
(tests/mesh_cache_oracle.py), and Mesher.update_octree_mesh against a fresh Mesher's recon_octree_mesh(sparse=True) on the same
state — vertices, faces, normals, colours and the PLY bytes — along a small synthetic incremental drive, with the number of
re-queried blocks held to the oracle's count."""
import copy
import functools
import pickle

import numpy as np
import pytest
import torch

import mesh_cache_oracle as mo
from test_gpu_mesh import _T

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ shine_rows_diff
def _rows_diff(tables, snaps, snap_rows):
    """tables: numpy [rows, 8] with the trash row last; snaps: numpy buffers with room for rows - 1 -> (flags, changed, snaps after)"""
    from shine_mapping_amd.mesher import rows_diff_device

    feats = [torch.as_tensor(t).cuda() for t in tables]
    dsnaps = [torch.as_tensor(s).cuda() for s in snaps]
    flags = [torch.full((len(t) - 1,), 7, dtype=torch.uint8, device="cuda") for t in tables]
    changed = torch.zeros(len(tables), dtype=torch.int64, device="cuda")
    rows_diff_device(feats, dsnaps, snap_rows, flags, changed)
    torch.cuda.synchronize()
    return [f.cpu().numpy() for f in flags], changed.cpu().numpy(), [s.cpu().numpy() for s in dsnaps], (feats, dsnaps, flags, changed)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("rows", [(1, 2, 64), (65, 257, 1), (257, 64, 65), (2, 65, 257), (258, 1, 600)])
def test_rows_diff_against_numpy(rows):
    from shine_mapping_amd.mesher import rows_diff_device

    rng = np.random.default_rng(sum(rows))
    tables = [rng.standard_normal((r, 8)).astype(np.float32) for r in rows]
    snaps, snap_rows = [], []
    for lvl, t in enumerate(tables):
        real = len(t) - 1
        s = np.full((real + 3, 8), 123.0, np.float32)  # (room beyond the table: must stay untouched)
        s[:real] = t[:-1]
        keep = real
        if real >= 1:
            last = _bits(t)[real - 1]  # one bit in the last float of the last real row
            last[7] ^= 1
        if real >= 4:
            t[0, 3], s[0, 3] = 0.0, -0.0  # -0.0 against 0.0: changed
            t[1, 5] = s[1, 5] = np.nan  # an identical NaN: unchanged
            t[2, 0] = 5.0  # an ordinary change, first float
        if real >= 60 and lvl != 1:
            keep = real // 2  # a snapshot shorter than the table: the rows beyond it are new
            s[keep:] = 123.0
        t[-1] += 1.0  # the trash row only: never flagged
        snaps.append(s)
        snap_rows.append(keep)
    want = [mo.changed_rows(t, s[:k]) for t, s, k in zip(tables, snaps, snap_rows)]
    flags, changed, after, dev = _rows_diff(tables, snaps, snap_rows)
    for lvl, (t, f, w, a) in enumerate(zip(tables, flags, want, after)):
        real = len(t) - 1
        print("level %d: %d real rows, snapshot %d, %d changed" % (lvl, real, snap_rows[lvl], w.sum()))
        assert np.array_equal(f.astype(bool), w) and set(np.unique(f)) <= {0, 1}
        assert changed[lvl] == w.sum()
        assert np.array_equal(_bits(a[:real]), _bits(t[:-1]))  # the snapshot is the table now
        assert (a[real:] == 123.0).all()
        if real >= 1:
            assert f[real - 1] == 1
        if real >= 4:
            assert f[0] == 1 and f[1] == 0 and f[2] == 1
            assert real < 60 or f[3] == 0 or snap_rows[lvl] <= 3
    # a second call with nothing changed: no flag, the counts stay, the snapshots are bit-equal
    feats, dsnaps, dflags, dchanged = dev
    rows_diff_device(feats, dsnaps, [len(t) - 1 for t in tables], dflags, dchanged)
    torch.cuda.synchronize()
    for f, s, a in zip(dflags, dsnaps, after):
        assert int(f.sum()) == 0
        assert np.array_equal(_bits(s.cpu().numpy()), _bits(a))
    assert np.array_equal(dchanged.cpu().numpy(), changed)


# ------------------------------------------------------------------------------------------------------ shine_mesh_mark_dirty
BOX = (12, 8, 4)  # finest cells of the hand-built octree: slot 0 has 3 x 2 x 1 nodes, slot 1 6 x 4 x 2, slot 2 all 384


@functools.lru_cache(None)
def _hand_octree():
    """every finest cell of BOX, three slots; every slot in a shuffled insertion order, but cell (5, 5, 1) — all of whose
    corners belong to neighbours too — is the LAST node of the finest slot"""
    rng = np.random.default_rng(11)
    ax = [np.arange(n) for n in BOX]
    cells = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    keys, ids, rows, corner_id = [], [], [], []
    off = np.array([[(j >> 2) & 1, (j >> 1) & 1, j & 1] for j in range(8)], np.int64)
    for s in range(3):
        k = np.unique(mo.encode(cells >> (2 - s)))
        rng.shuffle(k)
        if s == 2:
            last = mo.encode(np.array([[5, 5, 1]]))[0]
            k = np.concatenate((k[k != last], [last]))
        corners = (mo.decode(k)[:, None, :] + off[None]).reshape(-1, 3)
        uniq, inv = np.unique(corners, axis=0, return_inverse=True)
        order = rng.permutation(len(uniq))  # (row ids in no particular order)
        keys.append(k)
        ids.append(order[inv.reshape(-1)].reshape(-1, 8).astype(np.int32))
        rows.append(len(uniq))
        corner_id.append({tuple(c): int(order[i]) for i, c in enumerate(uniq)})
    return keys, ids, rows, corner_id


def _mark(keys, ids, prev, flags, sq):
    from shine_mapping_amd.mesher import mark_dirty_device

    dk = [torch.as_tensor(k).cuda() for k in keys]
    di = [torch.as_tensor(np.ascontiguousarray(i)).cuda() for i in ids]
    df = [torch.as_tensor(f.astype(np.uint8)).cuda() for f in flags]
    srt = [torch.sort(k) if s <= sq else None for s, k in enumerate(dk)]
    dirty = torch.full((len(keys[sq]),), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    mark_dirty_device(sq, dk, di, [len(k) for k in keys], prev, df, [e[0] if e else None for e in srt],
                      [e[1] if e else None for e in srt], dirty, counts)
    torch.cuda.synchronize()
    d = dirty.cpu().numpy()
    assert set(np.unique(d)) <= {0, 1}
    d = d.astype(bool)
    c = counts.cpu().numpy()
    assert c[1] == d.sum() and c[0] == d[:prev[sq]].sum()
    want = mo.dirty_query_nodes(keys, ids, prev, flags, sq)
    assert np.array_equal(want, mo.dirty_query_nodes_brute(keys, ids, prev, flags, sq))
    assert np.array_equal(d, want)
    return d


def _query_coords(keys, sq):
    return [tuple(c) for c in mo.decode(keys[sq]).tolist()]


@pytest.mark.parametrize("sq", [0, 1, 2])
def test_mark_dirty_on_a_hand_built_octree(sq):
    keys, ids, rows, corner_id = _hand_octree()
    full = [len(k) for k in keys]
    none = [np.zeros(r, bool) for r in rows]
    qc = _query_coords(keys, sq)
    size = 1 << (2 - sq)

    # nothing changed
    assert not _mark(keys, ids, full, none, sq).any()

    # one changed row of the FINEST slot, the corner shared by the cells (size - 1, 0, 0) and (size, 0, 0): two query nodes
    flags = [f.copy() for f in none]
    flags[2][corner_id[2][(size, 0, 0)]] = True
    d = _mark(keys, ids, full, flags, sq)
    assert {qc[i] for i in np.nonzero(d)[0]} == {(0, 0, 0), (1, 0, 0)}
    # ... and the same with a row of the query slot itself (the corner (1, 0, 0) of its nodes)
    flags = [f.copy() for f in none]
    flags[sq][corner_id[sq][(1, 0, 0)]] = True
    d = _mark(keys, ids, full, flags, sq)
    assert {qc[i] for i in np.nonzero(d)[0]} == {(0, 0, 0), (1, 0, 0)}

    # a new fine node whose corners all existed and did not change: its ancestor, and nothing else
    prev = [full[0], full[1], full[2] - 1]
    assert all((ids[2][:-1] == r).any() for r in ids[2][-1])  # (every corner row of the new cell is a neighbour's too)
    d = _mark(keys, ids, prev, none, sq)
    assert {qc[i] for i in np.nonzero(d)[0]} == {tuple(np.array([5, 5, 1]) >> (2 - sq))}

    # a dirty coarse node (the slot-0 row of corner (3, 2, 1) belongs to node (2, 1, 0) alone): all its descendants
    flags = [f.copy() for f in none]
    flags[0][corner_id[0][(3, 2, 1)]] = True
    d = _mark(keys, ids, full, flags, sq)
    got = {qc[i] for i in np.nonzero(d)[0]}
    want = {c for c in qc if (c[0] >> sq, c[1] >> sq, c[2] >> sq) == (2, 1, 0)}
    assert got == want and len(want) == 8 ** sq

    # everything at once, new nodes in every slot
    rng = np.random.default_rng(sq)
    flags = [rng.random(r) < 0.01 for r in rows]
    prev = [full[0] - 1, full[1] - 3, full[2] - 10]
    d = _mark(keys, ids, prev, flags, sq)
    assert 0 < d.sum() and (sq == 0 or d.sum() < len(d))


@pytest.mark.parametrize("sq", [0, 1, 2])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mark_dirty_on_random_octrees(sq, seed):
    rng = np.random.default_rng(10 * sq + seed)
    keys, ids, rows = mo.random_octree(rng, 2000, L=3, span=24)
    prev = [int(len(k) * 0.9) for k in keys]
    flags = [rng.random(r) < 0.003 for r in rows]
    d = _mark(keys, ids, prev, flags, sq)
    print("sq %d: %d of %d query nodes dirty" % (sq, d.sum(), len(d)))
    assert 0 < d.sum() and (sq < 2 or d.sum() < len(d))  # (a coarse query node has a new descendant almost surely)


def test_blocks_scatter():
    from shine_mapping_amd.mesher import blocks_scatter_device

    rng = np.random.default_rng(0)
    k3, cap, n = 27, 40, 17  # 459 points: two workgroups, blocks that straddle them
    values = torch.full((cap, 3, 3, 3), -1.0, device="cuda")
    masks = torch.full((cap, 3, 3, 3), 5, dtype=torch.uint8, device="cuda")
    index = torch.as_tensor(rng.permutation(cap)[:n].astype(np.int64)).cuda()
    sdf = torch.as_tensor(rng.standard_normal(n * k3).astype(np.float32)).cuda()
    m = torch.as_tensor(rng.random(n * k3) < 0.5).cuda()
    blocks_scatter_device(sdf, m, index, values, masks)
    want_v = torch.full((cap, k3), -1.0, device="cuda")
    want_m = torch.full((cap, k3), 5, dtype=torch.uint8, device="cuda")
    want_v[index] = sdf.view(n, k3)
    want_m[index] = m.view(n, k3).to(torch.uint8)
    assert torch.equal(values.view(cap, k3), want_v) and torch.equal(masks.view(cap, k3), want_m)
    blocks_scatter_device(sdf, None, index, values, masks)  # without the mask the blocks' masks are zero
    want_m[index] = 0
    assert torch.equal(values.view(cap, k3), want_v) and torch.equal(masks.view(cap, k3), want_m)


# ------------------------------------------------------------------------------------------------------ update_octree_mesh
@functools.lru_cache(None)
def _frames(radius):
    """frames 0, 1, 2 (12.5 m apart: they overlap) and frame 7 (62 m further on: far from all of them) of a 100 m street"""
    from shine_mapping_amd import synth

    cfg = _config(radius)
    frames = list(synth.make_frames(cfg, frames=8, beams=32, azimuths=180, seed=42, device="cuda"))
    return [frames[i] for i in (0, 1, 2, 7)]


def _config(radius, **over):
    from shine_mapping_amd import synth

    cfg = synth.make_config("ncd", device="cuda", lr=0.01, opt_adam=True, adam_eps=1e-15, lr_level_reduce_ratio=1.0,
                            street_len=100.0, pc_radius_m=radius, **over)
    cfg.mc_mask_on = True
    cfg.sem_color_map = synth.DRIVE_COLOR_MAP
    return cfg


class _Drive:
    """shine_incre.py's loop on the synthetic frames: update, a new optimiser, `iters` fused iterations; the decoder is frozen
    after the first frame."""

    def __init__(self, radius=8.0, iters=30, seed=0, **over):
        from shine_mapping_amd import Decoder, FeatureOctree, StepOptions

        self.cfg = _config(radius, **over)
        self.frames = _frames(radius)
        torch.manual_seed(seed)
        self.octree, self.dec = FeatureOctree(self.cfg), Decoder(self.cfg).cuda()
        self.opts = StepOptions(sigma=self.cfg.sigma_sigmoid, loss_reduction="sum")
        self.iters, self.done = iters, 0

    def train_frame(self):
        from shine_mapping_amd import fused_train_step
        from shine_mapping_amd.ops import fused_regularization, touched_flags
        from shine_mapping_amd.optim import setup_optimizer
        from shine_mapping_amd.sampler import SortedPool

        coord, label, weight = self.frames[self.done]
        octree, dec, cfg = self.octree, self.dec, self.cfg
        octree.update(coord[weight > 0], incremental_on=True)
        octree._require_tables(with_ranks=True)
        if self.done == 1:  # freeze_after_frame
            for p in dec.parameters():
                p.requires_grad_(False)
            self.opts.decoder_grad_on = False
        opt = setup_optimizer(cfg, list(octree.parameters()), dec.fused_params())
        pool = SortedPool(octree, coord, label, weight, seed=self.done)
        touched = touched_flags(octree)
        for _ in range(self.iters):
            idx = pool.draw(cfg.bs)
            fused_train_step(octree, dec, None, None, None, self.opts, pool=pool, idx=idx, touched=touched)
            fused_regularization(octree, cfg.lambda_forget, touched)
            opt.step(zero_grad=True)
        torch.cuda.synchronize()
        self.done += 1

    def mesher(self, sem=None):
        from shine_mapping_amd.mesher import Mesher

        m = Mesher(self.cfg, self.octree, self.dec, sem)
        m.global_transform = _T()
        return m


class _Oracle:
    """the dirty set the rule gives, from the octree's HOST tables and copies of its features at the previous call"""

    def __init__(self):
        self.feats = self.counts = None

    def expect(self, octree, sq):
        octree._sync_host()
        keys, ids = octree._node_keys, octree._node_ids
        tables = [p.detach().cpu().numpy() for p in octree.hier_features]
        if self.feats is None:
            prev, flags = [0] * len(keys), [np.ones(len(t) - 1, bool) for t in tables]
        else:
            prev, flags = self.counts, [mo.changed_rows(t, s) for t, s in zip(tables, self.feats)]
        d = mo.dirty_query_nodes(keys, ids, prev, flags, sq)
        new = len(keys[sq]) - prev[sq]
        self.feats, self.counts = [t[:-1].copy() for t in tables], [len(k) for k in keys]
        return d, new

    def forget(self):
        self.feats = self.counts = None


def _files_equal(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


def _update_equals_fresh(m, level, res, tmp_path, tag, **kw):
    """update_octree_mesh on `m` against recon_octree_mesh(sparse=True) of a fresh Mesher on the same state"""
    from shine_mapping_amd.mesher import Mesher

    pu, pf = str(tmp_path / (tag + "_update.ply")), str(tmp_path / (tag + "_fresh.ply"))
    mu = m.update_octree_mesh(level, res, pu, **kw)
    vu, fu = m.last_mesh_device
    fresh = Mesher(m.config, m.octree, m.geo_decoder, m.sem_decoder)
    fresh.global_transform = m.global_transform
    mf = fresh.recon_octree_mesh(level, res, pf, None, sparse=True, **kw)
    vf, ff = fresh.last_mesh_device
    st = m.last_update_stats
    print("%s: %d vertices, %d faces; %d nodes, %d new, %d dirty, %d re-queried (%d points), full %s (%s)"
          % (tag, len(vf), len(ff), st["nodes"], st["new_nodes"], st["dirty_nodes"], st["requeried_nodes"], st["requeried_points"],
             st["full"], st["reason"]))
    assert vu.dtype == vf.dtype and fu.dtype == ff.dtype
    assert torch.equal(fu, ff) and torch.equal(vu, vf)
    for name in ("vertices", "triangles", "vertex_normals", "vertex_colors"):
        a, b = np.asarray(getattr(mu, name)), np.asarray(getattr(mf, name))
        assert a.shape == b.shape and np.array_equal(a, b), name
    assert _files_equal(pu, pf)
    # the cache itself: every block, re-queried or kept, holds what a fresh query of all blocks gives (also where the mask is off
    # and the mesh therefore empty)
    c, M = m._mesh_cache, st["nodes"]
    lay = m.octree_grid_layout(level, res)
    mine = m._blocks_as_bricks(c.values[:M], c.masks[:M], lay[4], lay[5])
    theirs = fresh.octree_bricks_device(level, res)
    assert torch.equal(mine[0], theirs[0]) and torch.equal(mine[1], theirs[1])
    assert np.array_equal(mine[2], theirs[2]) and tuple(mine[3]) == tuple(theirs[3])
    assert bool(theirs[1].any()) == bool(m.config.mc_mask_on)
    assert st["requeried_nodes"] == (st["nodes"] if st["full"] else st["new_nodes"] + st["dirty_nodes"])
    assert st["requeried_points"] == st["requeried_nodes"] * m._mesh_cache.key[1] ** 3
    return pu, len(ff)


def _top(octree):
    return octree.max_level - octree.featured_level_num + 1


# (k = 4 at the coarsest featured level with and without the mask, k = 4 at the middle level, and k = 33 -> bricks of 11 on a
# smaller drive)
@pytest.mark.parametrize("radius,dlevel,res,k,mask_on", [(8.0, 0, 0.2, 4, True), (8.0, 0, 0.2, 4, False), (8.0, 1, 0.1, 4, True),
                                                         (5.5, 0, 0.0243, 33, True)])
def test_update_equals_a_fresh_mesh_after_every_frame(radius, dlevel, res, k, mask_on, tmp_path):
    from shine_mapping_amd.mesher import brick_edge

    d = _Drive(radius)
    d.cfg.mc_mask_on = mask_on
    m, oracle = d.mesher(), _Oracle()
    level = _top(d.octree) + dlevel
    faces = 0
    for f in range(4):
        d.train_frame()
        want, new = oracle.expect(d.octree, dlevel)
        path, nf = _update_equals_fresh(m, level, res, tmp_path, "f%d" % f, filter_isolated_mesh=f % 2 == 1)
        faces += nf
        st = m.last_update_stats
        assert m._mesh_cache.key[1] == k and (k <= 32 or brick_edge(k) == 11)
        assert st["nodes"] == len(want) and st["new_nodes"] == new
        assert st["full"] == (f == 0) and st["reason"] == ("first" if f == 0 else None)
        assert st["requeried_nodes"] == int(want.sum())  # exactly the oracle's new + dirty nodes
        assert f == 0 or 0 < st["requeried_nodes"]
    assert faces > 100 if mask_on else faces == 0  # (without the mask the blocks' masks are zero: no cube is processed)
    # the last frame lies far from the others: the rule itself (the CPU oracle on the host tables) asks for at most half the blocks
    assert int(want.sum()) <= len(want) // 2 and st["requeried_nodes"] <= st["nodes"] // 2
    # no training in between: nothing is queried, the mesh is the same
    before = open(path, "rb").read()
    v0, f0 = m.last_mesh_device
    m.update_octree_mesh(level, res, path, filter_isolated_mesh=True)
    st = m.last_update_stats
    assert (st["requeried_nodes"], st["requeried_points"], st["new_nodes"], st["dirty_nodes"], st["full"]) == (0, 0, 0, 0, False)
    assert open(path, "rb").read() == before
    assert torch.equal(m.last_mesh_device[0], v0) and torch.equal(m.last_mesh_device[1], f0)
    # mesh_path None: no file, the mesh on the device all the same
    m.last_mesh_device = None
    mesh = m.update_octree_mesh(level, res, None)
    assert torch.equal(m.last_mesh_device[0], v0) and len(np.asarray(mesh.vertices)) == len(v0)


def test_update_with_semantics(tmp_path):
    from shine_mapping_amd import Decoder

    d = _Drive(8.0, sem_class_count=5)
    torch.manual_seed(4)
    sem = copy.deepcopy(Decoder(d.cfg, is_geo_encoder=False)).cuda()
    with torch.no_grad():  # (spread the logits of the untrained head, as tests/test_gpu_mesh.py does)
        sem.layers[0].weight.mul_(100.0)
        sem.nclass_out.weight.mul_(10.0)
    m = d.mesher(sem)
    level = _top(d.octree)
    for f in range(2):
        d.train_frame()
        _update_equals_fresh(m, level, 0.2, tmp_path, "sem%d" % f, estimate_sem=True, filter_isolated_mesh=False)
    colors = np.asarray(m.update_octree_mesh(level, 0.2, None, estimate_sem=True).vertex_colors)
    assert len(colors) > 0 and len(np.unique(colors, axis=0)) > 1
    assert m.last_update_stats["requeried_nodes"] == 0


@pytest.mark.parametrize("slot", [0, 1, 2])
@pytest.mark.parametrize("dlevel", [0, 2])
def test_one_feature_row_edited_by_hand(slot, dlevel, tmp_path):
    d = _Drive(8.0)
    m, oracle = d.mesher(), _Oracle()
    level, res = _top(d.octree) + dlevel, (0.2 if dlevel == 0 else 0.05)
    for f in range(2):
        d.train_frame()
    oracle.expect(d.octree, dlevel)
    _update_equals_fresh(m, level, res, tmp_path, "before")
    r = int(d.octree.hier_features[slot].shape[0] // 3)
    with torch.no_grad():
        d.octree.hier_features[slot].data[r] += 1
    want, new = oracle.expect(d.octree, dlevel)
    _update_equals_fresh(m, level, res, tmp_path, "after")
    st = m.last_update_stats
    assert new == 0 and st["new_nodes"] == 0 and not st["full"]
    assert st["changed_rows"] == [int(s == slot) for s in range(3)]
    assert st["requeried_nodes"] == st["dirty_nodes"] == int(want.sum())
    assert 0 < st["requeried_nodes"] <= 8 * 8 ** max(dlevel - slot, 0)  # (the row's <= 8 nodes, and their descendants)


def test_rebuild_paths(tmp_path):
    d = _Drive(8.0)
    m = d.mesher()
    level = _top(d.octree)
    d.train_frame()
    d.train_frame()
    _update_equals_fresh(m, level, 0.2, tmp_path, "a")
    assert m.last_update_stats["reason"] == "first"

    with torch.no_grad():  # a decoder weight changed
        d.dec.fused_params()[2][3, 4] += 0.01
    _update_equals_fresh(m, level, 0.2, tmp_path, "dec")
    st = m.last_update_stats
    assert st["full"] and st["reason"] == "decoder" and st["requeried_nodes"] == st["nodes"]

    _update_equals_fresh(m, level, 0.1, tmp_path, "key")  # another resolution
    assert m.last_update_stats["full"] and m.last_update_stats["reason"] == "key"
    _update_equals_fresh(m, level, 0.1, tmp_path, "key2")
    assert not m.last_update_stats["full"] and m.last_update_stats["requeried_nodes"] == 0
    d.cfg.mc_mask_on = False
    _update_equals_fresh(m, level, 0.1, tmp_path, "mask")
    assert m.last_update_stats["reason"] == "key"
    d.cfg.mc_mask_on = True
    _update_equals_fresh(m, level, 0.1, tmp_path, "mask2")
    assert m.last_update_stats["reason"] == "key"

    # rebuilt device tables keep the host order: a valid prefix, nothing to query — and never a stale mesh
    d.octree.rebuild_device_tables()
    _update_equals_fresh(m, level, 0.1, tmp_path, "rebuilt")
    st = m.last_update_stats
    assert (st["full"], st["requeried_nodes"]) == (False, 0) or st["reason"] == "octree"

    # an unpickled octree with one row changed: a valid prefix (one row's blocks) or "octree"
    other = pickle.loads(pickle.dumps(d.octree))
    with torch.no_grad():
        other.hier_features[2].data[7] += 1
    m.octree = other
    _update_equals_fresh(m, level, 0.1, tmp_path, "pickled")
    st = m.last_update_stats
    assert (not st["full"] and 0 < st["requeried_nodes"] < st["nodes"]) or st["reason"] == "octree"

    # the FINEST level's tables in another order, the query level's as they were: the cache holds device copies of every level
    other._sync_host()
    tables = [(torch.as_tensor(k[::-1].copy() if s == 2 else k), torch.as_tensor(i[::-1].copy() if s == 2 else i))
              for s, (k, i) in enumerate(zip(other._node_keys, other._node_ids))]
    other.load_tables(tables)
    _update_equals_fresh(m, level, 0.1, tmp_path, "finest_reordered")
    assert m.last_update_stats["full"] and m.last_update_stats["reason"] == "octree"

    # tables in another order (load_tables): the cached keys are no prefix
    other._sync_host()
    tables = [(torch.as_tensor(k[::-1].copy()), torch.as_tensor(i[::-1].copy())) for k, i in zip(other._node_keys, other._node_ids)]
    other.load_tables(tables)
    _update_equals_fresh(m, level, 0.1, tmp_path, "reordered")
    assert m.last_update_stats["full"] and m.last_update_stats["reason"] == "octree"

    m.reset_mesh_cache()
    _update_equals_fresh(m, level, 0.1, tmp_path, "reset")
    assert m.last_update_stats["full"] and m.last_update_stats["reason"] == "first"

    d.cfg.time_conditioned = True
    with pytest.raises(NotImplementedError):
        m.update_octree_mesh(level, 0.1, None)
