"""FeatureOctree — host-side mirror of the reference class, backed by libshine_hip.so.

Same constructor, attributes and methods as model/feature_octree.py:29-298 (the surface the drivers,
the mesher and cal_feature_importance touch — SURVEY.md §8b), but:

  * the per-level python dicts ``nodes_lookup_tables`` are replaced by device hash tables owned by the
    library (node Morton -> 8 corner ids); dict *views* are still available for code that reads them
    (utils/mesher.py, checkpoints) and are rebuilt lazily;
  * ``update`` (:114-166) is vectorised on the host (unique/searchsorted instead of per-node Python
    loops) and reproduces the reference's corner-id assignment exactly: ids are appended per call in
    lexicographic (x,y,z) order of the new nodes' unique corners (:132-137,148-151);
  * ``get_indices`` / ``query_feature`` run on the GPU with no host round trip (the reference crosses
    the device boundary twice per level, :204,215).

There is no CPU fallback: every query goes through the HIP library and raises if it is missing.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List

import numpy as np
import torch
import torch.nn as nn

from . import _ext, _lib, autograd_ops

_OPS = None


def _ops():
    """ops, imported on first use (ops imports this module's types) — not per call: a function-level import costs ~1 us"""
    global _OPS
    if _OPS is None:
        from . import ops

        _OPS = ops
    return _OPS

_CORNER_OFFSETS = np.array([[(j >> 2) & 1, (j >> 1) & 1, j & 1] for j in range(8)], dtype=np.int64)


# --------------------------------------------------------------------------- integer helpers (host, numpy int64)


def _spread3(v: np.ndarray) -> np.ndarray:
    x = v.astype(np.uint64) & np.uint64(0xFFFF)
    x = (x | (x << np.uint64(32))) & np.uint64(0x001F00000000FFFF)
    x = (x | (x << np.uint64(16))) & np.uint64(0x001F0000FF0000FF)
    x = (x | (x << np.uint64(8))) & np.uint64(0x100F00F00F00F00F)
    x = (x | (x << np.uint64(4))) & np.uint64(0x10C30C30C30C30C3)
    x = (x | (x << np.uint64(2))) & np.uint64(0x1249249249249249)
    return x


def _compact3(m: np.ndarray) -> np.ndarray:
    x = m.astype(np.uint64) & np.uint64(0x1249249249249249)
    x = (x | (x >> np.uint64(2))) & np.uint64(0x10C30C30C30C30C3)
    x = (x | (x >> np.uint64(4))) & np.uint64(0x100F00F00F00F00F)
    x = (x | (x >> np.uint64(8))) & np.uint64(0x001F0000FF0000FF)
    x = (x | (x >> np.uint64(16))) & np.uint64(0x001F00000000FFFF)
    x = (x | (x >> np.uint64(32))) & np.uint64(0xFFFF)
    return x


def morton_encode(xyz: np.ndarray) -> np.ndarray:
    """kaolin.ops.spc.points_to_morton convention: per bit triplet x is the MSB, z the LSB. -> int64"""
    m = (_spread3(xyz[..., 0]) << np.uint64(2)) | (_spread3(xyz[..., 1]) << np.uint64(1)) | _spread3(xyz[..., 2])
    return m.astype(np.int64)


def morton_decode(m: np.ndarray) -> np.ndarray:
    mu = m.astype(np.uint64)
    return np.stack(
        (_compact3(mu >> np.uint64(2)), _compact3(mu >> np.uint64(1)), _compact3(mu)), axis=-1
    ).astype(np.int64)


def _pack_lex(xyz: np.ndarray) -> np.ndarray:
    """(x,y,z) -> one int64 whose ascending order is the lexicographic order torch.unique(dim=0) uses (:132)."""
    return (xyz[..., 0] << 42) | (xyz[..., 1] << 21) | xyz[..., 2]


def _unpack_lex(k: np.ndarray) -> np.ndarray:
    return np.stack((k >> 42, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF), axis=-1)


import os as _os
from operator import is_ as _is

RIDER_ENABLED = _os.environ.get("SHINE_RIDER", "1") != "0"  # tests / tools: False = cal_regularization always runs its own launches


class _DeviceTables:
    """Owner of the library's shine_tables handle."""

    def __init__(self, n_levels: int):
        self.n_levels = n_levels
        self.handle = C.c_void_p()
        _lib.check(_lib.lib().shine_tables_create(n_levels, C.byref(self.handle)), "shine_tables_create")

    def insert(self, slot: int, keys: torch.Tensor, ids: torch.Tensor):
        assert keys.is_cuda and ids.is_cuda and keys.dtype == torch.int64 and ids.dtype == torch.int32
        keys = keys.contiguous()
        ids = ids.contiguous()
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(
            _lib.lib().shine_tables_insert(self.handle, slot, keys.data_ptr(), ids.data_ptr(), keys.numel(), stream),
            "shine_tables_insert",
        )
        torch.cuda.current_stream().synchronize()  # keys/ids staging tensors may be freed by the caller

    def stats(self, slot: int):
        cap, cnt = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().shine_tables_stats(self.handle, slot, C.byref(cap), C.byref(cnt)), "shine_tables_stats")
        return cap.value, cnt.value

    def __del__(self):
        try:
            if self.handle:
                _lib.lib().shine_tables_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass


class FeatureOctree(nn.Module):
    def __init__(self, config):
        super().__init__()
        # model/feature_octree.py:35-44
        self.max_level = config.tree_level_world
        self.leaf_vox_size = config.leaf_vox_size
        self.featured_level_num = config.tree_level_feat
        self.free_level_num = self.max_level - self.featured_level_num + 1
        self.feature_dim = config.feature_dim
        self.feature_std = config.feature_std
        self.polynomial_interpolation = config.poly_int_on
        self.device = config.device
        if self.featured_level_num < 1:
            raise ValueError("No level with grid features!")  # :57-58
        if self.feature_dim != _lib.FEATURE_DIM:
            raise NotImplementedError("libshine_hip is built for feature_dim == 8 (every shipped config)")
        if self.featured_level_num > _lib.MAX_LEVELS or self.max_level > 15:
            raise NotImplementedError("at most 8 featured levels and tree_level_world <= 15")

        L = self.featured_level_num
        # host copies of the tables, per featured slot (top-down): everything the dict views need
        self._node_keys = [np.zeros(0, np.int64) for _ in range(L)]       # insertion order
        self._node_ids = [np.zeros((0, 8), np.int32) for _ in range(L)]   # insertion order
        self._node_sorted = [np.zeros(0, np.int64) for _ in range(L)]     # sorted, for membership tests
        self._corner_lex = [np.zeros(0, np.int64) for _ in range(L)]      # sorted lexicographic keys
        self._corner_id_of_lex = [np.zeros(0, np.int64) for _ in range(L)]
        self._corner_count = [0] * L
        self._dict_cache = None
        self._sort_box_cache = None
        self._ranks_uploaded = False
        self._n_buckets = 0
        self._tables_epoch = 0  # bumped whenever nodes are added (hash slots may move): invalidates planned pools
        self._tables = None  # created at the first query (needs the GPU); update() itself is host-only
        self._pending = [[] for _ in range(L)]  # (node keys, corner ids) not yet inserted on the device
        # device growth (shine_tables_grow): per level the (node keys, corner ids, new corner keys) device tensors of
        # every frame, not yet merged into the host copies above (_sync_host does that when a host view is needed)
        self._dev_log = [[] for _ in range(L)]
        self._dev_frames = []  # (flat copy, fresh counts, added counts) per frame, not yet split into _dev_log
        self._growth_stream = None  # enable_async_growth(): update() grows the tree on this stream
        self._probe_pending = False
        self._ev_read = self._ev_grown = None
        self._ev_read_valid = False
        self._corners_on_device = False  # the handle's corner tables hold every corner of every level
        self._box = None  # running (lo, hi) of the coarsest featured level's node coords, for _sort_box
        self._box_pending = []  # device tensors of coarse node keys not yet folded into _box
        # a level's regulariser contributes gradient only while its features_last_frame copy is detached
        # (first-frame branch :146); the later branch :160 stores an attached clone -> zero net gradient.
        self._reg_grad_on = [True] * L

        self.hier_features = nn.ParameterList([])  # top-down  :63
        self.hierarchical_indices = []  # bottom-up :67
        self.importance_weight = []  # :71
        self.features_last_frame = []  # :72
        self.to(config.device)

    # ------------------------------------------------------------------ dict views (compat)
    def _build_dicts(self):
        self._sync_host()
        nodes = [dict() for _ in range(self.max_level + 1)]
        corners = [dict() for _ in range(self.max_level + 1)]
        for s in range(self.featured_level_num):
            lvl = self.free_level_num + s
            nodes[lvl] = dict(zip(self._node_keys[s].tolist(), self._node_ids[s].tolist()))
            cm = morton_encode(_unpack_lex(self._corner_lex[s]))
            corners[lvl] = dict(zip(cm.tolist(), self._corner_id_of_lex[s].tolist()))
        self._dict_cache = (nodes, corners)

    @property
    def nodes_lookup_tables(self):
        """list over absolute levels of {node morton: [8 corner ids]} (model/feature_octree.py:47-52)."""
        if self._dict_cache is None:
            self._build_dicts()
        return self._dict_cache[0]

    @property
    def corners_lookup_tables(self):
        if self._dict_cache is None:
            self._build_dicts()
        return self._dict_cache[1]

    # ------------------------------------------------------------------ :67, :199-218
    @property
    def hierarchical_indices(self):
        """list of L [N, 8] int64 tensors, bottom-up (:67).  query_feature in a training loop does not materialise them
        (192 B per point and level that nothing on that path reads): they are computed here, on first access, from the
        coordinates of the last query — cal_regularization (:246-255) and the mesher (utils/mesher.py:82,102) read them."""
        d = self.__dict__
        if d.get("_hidx") is None and d.get("_hidx_coord") is not None:
            if d.get("_hidx_epoch") != self._tables_epoch:
                # the reference's list is computed AT query time and holds -1 for nodes that did not exist then (:199-218);
                # a lazy evaluation against the grown tables would silently differ
                raise RuntimeError("hierarchical_indices of a query made before update() grew the octree: they are computed on "
                                   "first access — read them before update(), or call get_indices(coord) again")
            coord, d["_hidx_coord"] = d["_hidx_coord"], None
            self.get_indices(coord)
        return d.get("_hidx") if d.get("_hidx") is not None else []

    @hierarchical_indices.setter
    def hierarchical_indices(self, value):
        self.__dict__["_hidx"] = value
        self.__dict__["_hidx_coord"] = None

    def _reg_rider(self, st):
        """Incremental mapping from its second frame on (shine_incre.py:152-158 with features_last_frame an attached clone, :160: the
        regulariser enters the loss by VALUE only): that value rides on query_feature's own launch (csrc/shine_forward.hip,
        cfg->reg_rider) instead of costing cal_regularization four launches of its own.  Decided once per set of tensors (they
        change once per frame): on iff every level's features_last_frame is an attached clone and all tables are float32 CUDA of
        the features' shapes; the extension's state then holds the tensors (st.set_reg)."""
        d = self.__dict__
        last, imp, feats = self.features_last_frame, self.importance_weight, self.hier_features
        k = d.get("_rider_keep")  # (the tensors the decision was taken on: identity checks, ~1 us per query)
        if (k is not None and k[3] is st and k[4] == RIDER_ENABLED and len(last) == len(k[0]) and len(imp) == len(k[1])
                and len(feats) == len(k[2]) and all(map(_is, last, k[0])) and all(map(_is, imp, k[1]))
                and all(map(_is, feats, k[2]))):
            return d["_rider_on"]
        L = self.featured_level_num
        on = (RIDER_ENABLED and 0 < L <= 4 and len(last) == L and len(imp) == L and len(feats) == L
              and all(a.shape == p.shape and b.shape == p.shape and a.is_cuda and b.is_cuda and a.dtype == torch.float32
                      and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and p.is_contiguous()
                      for a, b, p in zip(last, imp, feats)))
        if on:
            live = self._reg_live_levels()
            on = live is not None and not any(live)
        if on:
            stamps = d.get("_rider_stamps")
            if stamps is None or any(s.numel() < p.shape[0] or s.device != p.device for s, p in zip(stamps, feats)):
                stamps = d["_rider_stamps"] = [torch.zeros(p.shape[0] + 1024, dtype=torch.int32, device=p.device) for p in feats]
                d["_rider_acc"] = torch.zeros(8, dtype=torch.float32, device=feats[0].device)
            st.set_reg([t.detach() for t in last], [t.detach() for t in imp], stamps, d["_rider_acc"])
        else:
            st.set_reg([], [], [], torch.empty(0))
        d["_rider_on"] = on
        d["_rider_keep"] = (tuple(last), tuple(imp), tuple(feats), st, RIDER_ENABLED)
        return on

    def _defer_indices(self, coord):
        self.__dict__["_reg_riding"] = None  # (whoever ran the query sets it afterwards if the regulariser rode on it)
        self.__dict__["_hidx"] = None
        self.__dict__["_hidx_coord"] = coord.detach()
        self.__dict__["_hidx_epoch"] = self._tables_epoch

    # ------------------------------------------------------------------ :78-81
    def set_zero(self):
        with torch.no_grad():
            for n in range(len(self.hier_features)):
                self.hier_features[n][-1] = 0.0

    def forward(self, x):
        return self.query_feature(x)

    def is_empty(self):
        return len(self.hier_features) == 0

    def clear_temp(self):
        self.hierarchical_indices = []
        self.importance_weight = []
        self.features_last_frame = []

    # ------------------------------------------------------------------ :94-101
    def get_octree_nodes(self, level):
        self._sync_host()
        s = level - self.free_level_num
        xyz = morton_decode(self._node_keys[s]).astype(np.float64) if 0 <= s < self.featured_level_num else \
            np.zeros((0, 3))
        node_size = 2 ** (1 - level)
        return (xyz * node_size) - 1.0 + 0.5 * node_size

    # ------------------------------------------------------------------ :114-166
    def update(self, surface_points: torch.Tensor, incremental_on: bool = False, ready=None):
        """CUDA points grow the tree on the device (shine_tables_grow); host points take the
        vectorised numpy path below.  Both produce the reference's tables bit for bit.
        `ready` matters only after enable_async_growth(), where the growth runs on a stream of its own and must not start before
        `surface_points` exist: None (default) — the growth waits for everything queued on the caller's stream so far (always
        safe; the host then waits for that too); a torch.cuda.Event or Stream — it waits for that only; False — the caller
        states that the points were produced ON octree.growth_stream (or are long finished): no wait at all."""
        if surface_points.is_cuda:
            return self._update_device(surface_points, incremental_on, ready)
        self._sync_host()
        if self._corners_on_device:  # the handle's corner tables would go stale: rebuild it from the host copies
            self.rebuild_device_tables()
        dev = self.hier_features[0].device if len(self.hier_features) else torch.device(self.device)
        res = 2 ** self.max_level
        # kaolin quantize_points, fp32, on whatever device the points live on
        q = torch.floor(torch.clamp(res * (surface_points.float() + 1.0) / 2.0, 0, res - 1.0)).to(torch.int64)
        leaf = np.unique(morton_encode(q.cpu().numpy()))
        self._dict_cache = None
        self._sort_box_cache = None
        for s in range(self.featured_level_num):
            lvl = self.free_level_num + s
            nodes = np.unique(leaf >> (3 * (self.max_level - lvl)))  # Morton order, like point_hierarchies
            known = self._node_sorted[s]
            if known.size:
                pos = np.searchsorted(known, nodes)
                pos[pos == known.size] = 0
                fresh = nodes[known[pos] != nodes]
            else:
                fresh = nodes
            if fresh.size == 0:
                continue  # :129-130
            corners = morton_decode(fresh)[:, None, :] + _CORNER_OFFSETS[None, :, :]  # [M,8,3]
            lex = _pack_lex(corners.reshape(-1, 3))
            uniq = np.unique(lex)  # lexicographic (x,y,z)
            first = self._corner_count[s] == 0
            if first:
                new_lex = uniq
            else:
                cpos = np.searchsorted(self._corner_lex[s], uniq)
                cpos[cpos == self._corner_lex[s].size] = 0
                new_lex = uniq[self._corner_lex[s][cpos] != uniq]
            base = self._corner_count[s]
            new_ids = np.arange(base, base + new_lex.size, dtype=np.int64)
            merged = np.concatenate((self._corner_lex[s], new_lex))
            merged_ids = np.concatenate((self._corner_id_of_lex[s], new_ids))
            order = np.argsort(merged, kind="stable")
            self._corner_lex[s] = merged[order]
            self._corner_id_of_lex[s] = merged_ids[order]
            self._corner_count[s] = base + new_lex.size
            added = int(new_lex.size)
            if s == 0:
                self._grow_box(fresh)
            self._append_rows(s, first, added, incremental_on, dev)
            ids = self._corner_id_of_lex[s][np.searchsorted(self._corner_lex[s], lex)].reshape(-1, 8).astype(np.int32)
            self._node_keys[s] = np.concatenate((self._node_keys[s], fresh))
            self._node_ids[s] = np.concatenate((self._node_ids[s], ids))
            self._node_sorted[s] = np.sort(np.concatenate((known, fresh)))
            self._pending[s].append((fresh, ids))  # uploaded to the device hash table at the next query
            self._bump_epoch()

    def _append_rows(self, s, first, added, incremental_on, dev):
        """The feature-side half of update() for one level that received new nodes (:135-160)."""
        if first:  # :135-146
            fts = self.feature_std * torch.randn(added + 1, self.feature_dim, device=dev)
            fts[-1] = 0.0
            self.hier_features.append(nn.Parameter(fts))
            if incremental_on:
                self.importance_weight.append(torch.zeros(added + 1, self.feature_dim, device=dev))
                self.features_last_frame.append(fts.clone())
                self._reg_grad_on[s] = True
        else:  # :147-160
            new_fts = self.feature_std * torch.randn(added + 1, self.feature_dim, device=dev)
            new_fts[-1] = 0.0
            self.hier_features[s] = nn.Parameter(torch.cat((self.hier_features[s].detach()[:-1], new_fts), 0))
            if incremental_on:
                new_w = torch.zeros(added + 1, self.feature_dim, device=dev)
                self.importance_weight[s] = torch.cat((self.importance_weight[s][:-1], new_w), 0)
                # the reference clones the Parameter itself (attached to the graph, :160): the regulariser
                # then adds to the loss value but its gradient cancels.  Kept.
                self.features_last_frame[s] = self.hier_features[s].clone()
                self._reg_grad_on[s] = False

    def _grow_box(self, coarse_keys: np.ndarray):
        if coarse_keys.size == 0:
            return
        xyz = morton_decode(coarse_keys)
        lo, hi = xyz.min(0), xyz.max(0)
        if self._box is not None:
            lo, hi = np.minimum(lo, self._box[0]), np.maximum(hi, self._box[1])
        self._box = (lo, hi)
        self._sort_box_cache = None

    # ------------------------------------------------------------------ :114-166 on the device
    def _update_device(self, surface_points: torch.Tensor, incremental_on: bool, ready=None):
        pts = surface_points.detach()
        if pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("surface_points must be a float32 tensor of shape [M,3]")
        pts = pts.contiguous()
        dev = pts.device
        L = self.featured_level_num
        t = self._ensure_handle(dev)
        if not self._corners_on_device:
            self._upload_corners(dev)
        fresh, added = (C.c_int64 * L)(), (C.c_int64 * L)()
        cfg = _lib.StepConfig()
        cfg.n_levels, cfg.max_level = L, self.max_level
        lib = _lib.lib()
        main = torch.cuda.current_stream(dev)
        side = self._growth_stream if self._growth_stream is not None else main
        if side is not main:
            # asynchronous growth (enable_async_growth): the growth's kernels and its two host reads use a stream of their own, so
            # this call does not wait for what the caller has queued (the previous frame's iterations).  Growth writes the hash
            # tables — which the queued steps read only through slots they memoised, never by probing — so the one thing it has
            # to wait for is the last PROBE of the tables (a pool plan, a query): _tables_read_done() recorded it; a probe nobody
            # recorded (self._probe_pending) falls back to waiting for everything queued so far.
            if self._probe_pending:
                self._ev_read.record(main)
                self._ev_read_valid = True
                self._probe_pending = False
            if self._ev_read_valid:
                side.wait_event(self._ev_read)
            # ... and for the points themselves (ADVICE / VERDICT r04: an enforced contract instead of a sentence in DESIGN.md)
            if ready is None:
                side.wait_stream(main)
            elif ready is not False:
                (side.wait_event if isinstance(ready, torch.cuda.Event) else side.wait_stream)(ready)
        with torch.cuda.stream(side):
            stream = side.cuda_stream
            _lib.check(lib.shine_tables_grow(t.handle, C.byref(cfg), pts.data_ptr(), pts.shape[0], fresh, added, stream),
                       "shine_tables_grow")
            nf, na = [int(v) for v in fresh], [int(v) for v in added]
            grown = [s for s in range(L) if nf[s]]  # (a level without new nodes has no new corners: :129-130)
            if not grown:
                return
            # what the device added — node keys, corner ids, new corner keys of every level — in ONE copy; it is split per
            # level only when a host view is asked for (_drain_dev_frames)
            words = sum(5 * nf[s] + na[s] for s in range(L))
            flat = torch.empty(words, dtype=torch.int64, device=dev)
            _lib.check(lib.shine_tables_grow_fetch_all(t.handle, flat.data_ptr(), words, stream), "shine_tables_grow_fetch_all")
            if side is not main:
                # the node ranks (what the next pool plan sorts by) on the growth's stream too: they share the handle's scratch
                self._ranks_uploaded = False
                self._upload_ranks(dev)
        if side is not main:
            self._ev_grown.record(side)
            main.wait_event(self._ev_grown)  # the appends, plans and steps queued from here on see the grown tables
            flat.record_stream(main)  # (allocated in the side stream's pool, read on the caller's: _drain_dev_frames / _sync_host)
        stream = main.cuda_stream
        self._dev_frames.append((flat, nf, na))
        self._sort_box_cache = None
        first = [self._corner_count[s] == 0 for s in range(L)]
        for s in grown:
            self._corner_count[s] += na[s]
        if any(first[s] for s in grown):  # (the first frame: torch, level by level — the order of the random draws is the loop's)
            for s in grown:
                self._append_rows(s, first[s], na[s], incremental_on, dev)
        else:
            self._append_rows_fused(grown, [na[s] for s in grown], incremental_on, dev, stream)
        self._dict_cache = None
        if side is main:
            self._ranks_uploaded = False
        self._bump_epoch()
        if self.retired_table_bytes() > self.trim_retired_above:
            self.trim_tables()

    # Device arrays a growth replaced are retired inside the handle, not freed (launches bound to them may be queued, and hipFree
    # waits for the whole device).  They never exceed the live tables (capacities double), but on a 10^7-row map that is still
    # hundreds of MB: above this many bytes update() synchronises the device once and frees them.
    trim_retired_above = 1 << 30

    def retired_table_bytes(self) -> int:
        if self._tables is None:
            return 0
        b = C.c_int64()
        _lib.check(_lib.lib().shine_tables_retired_bytes(self._tables.handle, C.byref(b)), "shine_tables_retired_bytes")
        return int(b.value)

    def trim_tables(self) -> int:
        """Free the arrays earlier growths replaced.  Synchronises the device first: every launch that was handed the old arrays
        — also those of an iteration graph bound before the growth — has then finished (graphs are re-bound to the handle's
        live arrays when the next frame's iterations are set up)."""
        if self._tables is None:
            return 0
        torch.cuda.synchronize(self.hier_features[0].device if len(self.hier_features) else None)
        b = C.c_int64()
        _lib.check(_lib.lib().shine_tables_trim(self._tables.handle, C.byref(b)), "shine_tables_trim")
        return int(b.value)

    def enable_async_growth(self, stream=None):
        """Let update() grow the tree on a stream of its own (`growth_stream`), so that a loop which keeps the host ahead of the
        device — no synchronisation between frames — does not stall in update()'s two host reads behind the previous frame's
        iterations.  Contract: the surface points handed to update() must not depend on work still queued on another stream
        (produce them under `with torch.cuda.stream(octree.growth_stream)`, or synchronise first).  Everything else stays ordered
        by events: growth waits for the last probe of the tables, and the caller's stream waits for the growth."""
        dev = self.hier_features[0].device if len(self.hier_features) else torch.device(self.device)
        # (high priority: the growth is a few dozen tiny kernels the host WAITS for — twice — while the main stream is busy with
        # the previous frame's iterations)
        self._growth_stream = stream if stream is not None else torch.cuda.Stream(device=dev, priority=-1)
        self._ev_read, self._ev_grown = torch.cuda.Event(), torch.cuda.Event()
        self._ev_read_valid = False
        self._probe_pending = True  # (whatever was queued before this call counts as a probe nobody recorded)
        return self._growth_stream

    @property
    def growth_stream(self):
        return self._growth_stream

    def _tables_read_done(self):
        """Called by the entry points that PROBE the hash tables, right after their launch (asynchronous growth waits for it)."""
        if self._growth_stream is not None:
            self._ev_read.record(torch.cuda.current_stream())
            self._ev_read_valid = True
            self._probe_pending = False

    def _append_rows_fused(self, levels, added, incremental_on, dev, stream):
        """_append_rows' second branch (:147-160) for all levels that grew, ONE launch (shine_append_rows): the random rows come
        from torch.randn, level by level in the order the loop above would draw them — the generator's stream is the
        reference's."""
        lib = _lib.lib()
        n = len(levels)
        old = [self.hier_features[s].detach() for s in levels]
        noise = [torch.randn(a + 1, self.feature_dim, device=dev) for a in added]
        new = [torch.empty(o.shape[0] + a, self.feature_dim, device=dev) for o, a in zip(old, added)]
        if incremental_on:
            old_imp = [self.importance_weight[s] for s in levels]
            imp = [torch.empty_like(f) for f in new]
        _lib.check(lib.shine_append_rows(
            n, _lib.ptr_array([o.data_ptr() for o in old]),
            _lib.ptr_array([o.data_ptr() for o in old_imp]) if incremental_on else None,
            _lib.ptr_array([r.data_ptr() for r in noise]), _lib.i64_array([o.shape[0] - 1 for o in old]),
            _lib.i64_array(added), float(self.feature_std), _lib.ptr_array([f.data_ptr() for f in new]),
            _lib.ptr_array([w.data_ptr() for w in imp]) if incremental_on else None, None, stream), "shine_append_rows")
        for k, s in enumerate(levels):
            self.hier_features[s] = nn.Parameter(new[k])
            if incremental_on:
                self.importance_weight[s] = imp[k]
                # the reference clones the Parameter itself (attached to the graph, :160): the regulariser then adds to the
                # loss value but its gradient cancels.  Kept, as a torch clone — cal_regularization below differentiates
                # through it
                self.features_last_frame[s] = self.hier_features[s].clone()
                self._reg_grad_on[s] = False

    def _drain_dev_frames(self):
        """Split the frames' flat copies (shine_tables_grow_fetch_all) into the per-level logs _sync_host / _sort_box read."""
        frames, self._dev_frames = getattr(self, "_dev_frames", None) or [], []
        for flat, nf, na in frames:
            off = 0
            for s in range(self.featured_level_num):
                keys = flat[off:off + nf[s]]
                off += nf[s]
                ids = flat[off:off + 4 * nf[s]].view(torch.int32).view(nf[s], 8)
                off += 4 * nf[s]
                newc = flat[off:off + na[s]]
                off += na[s]
                if nf[s]:
                    self._dev_log[s].append((keys, ids, newc))
                    if s == 0:
                        self._box_pending.append(keys)  # (the sort box is derived lazily: no host read per frame)

    def _sync_host(self):
        """Merge what the device added (shine_tables_grow) into the host copies the dict views / pickles read."""
        self._drain_dev_frames()
        if not any(self._dev_log):
            return
        for s in range(self.featured_level_num):
            if not self._dev_log[s]:
                continue
            keys = torch.cat([e[0] for e in self._dev_log[s]]).cpu().numpy()
            ids = torch.cat([e[1] for e in self._dev_log[s]]).cpu().numpy()
            newc = torch.cat([e[2] for e in self._dev_log[s]]).cpu().numpy()
            base = self._corner_lex[s].size
            self._node_keys[s] = np.concatenate((self._node_keys[s], keys))
            self._node_ids[s] = np.concatenate((self._node_ids[s], ids))
            self._node_sorted[s] = np.sort(self._node_keys[s])
            merged = np.concatenate((self._corner_lex[s], newc))
            merged_ids = np.concatenate((self._corner_id_of_lex[s], np.arange(base, base + newc.size, dtype=np.int64)))
            order = np.argsort(merged, kind="stable")
            self._corner_lex[s], self._corner_id_of_lex[s] = merged[order], merged_ids[order]
            assert self._corner_lex[s].size == self._corner_count[s]
            self._dev_log[s] = []
        self._dict_cache = None

    def _ensure_handle(self, dev):
        """The library handle with every host-side node inserted (works on an empty tree too)."""
        if self._tables is None:
            self._tables = _DeviceTables(self.featured_level_num)
            self._ranks_uploaded = False
            self._corners_on_device = False
        for s in range(self.featured_level_num):
            for keys, ids in self._pending[s]:
                self._tables.insert(s, torch.from_numpy(keys).to(dev), torch.from_numpy(ids).to(dev))
                self._ranks_uploaded = False
            self._pending[s] = []
        return self._tables

    def _upload_corners(self, dev):
        """Seed the handle's corner tables from the host copies (after host-side updates / load_tables / unpickling)."""
        lib = _lib.lib()
        stream = torch.cuda.current_stream(dev).cuda_stream
        for s in range(self.featured_level_num):
            cnt = C.c_int64()
            _lib.check(lib.shine_tables_corner_count(self._tables.handle, s, C.byref(cnt)), "shine_tables_corner_count")
            if cnt.value:
                raise RuntimeError("corner tables partially present: rebuild_device_tables() first")
            if self._corner_lex[s].size == 0:
                continue
            keys_d = torch.from_numpy(self._corner_lex[s]).to(dev)
            ids_d = torch.from_numpy(self._corner_id_of_lex[s].astype(np.int32)).to(dev)
            _lib.check(lib.shine_tables_insert_corners(self._tables.handle, s, keys_d.data_ptr(), ids_d.data_ptr(),
                                                       keys_d.numel(), stream), "shine_tables_insert_corners")
            torch.cuda.current_stream(dev).synchronize()
        self._corners_on_device = True

    # ------------------------------------------------------------------ hot path plumbing
    def _require_tables(self, with_ranks=False, probe=True):
        """`probe=False`: the caller reads the tables only through hash slots it memoised (the fused step on a planned batch or a
        pool, the importance sweep) — asynchronous growth need not wait for it."""
        if len(self.hier_features) != self.featured_level_num:
            raise RuntimeError("FeatureOctree is empty: call update() before querying")
        if probe and self._growth_stream is not None:
            self._probe_pending = True
        dev = self.hier_features[0].device
        t = self._ensure_handle(dev)
        if with_ranks and not self._ranks_uploaded:
            self._upload_ranks(dev)
        return t

    def _upload_ranks(self, dev):
        """Rank every node of every featured level in ONE Z-order (a parent's own bucket right after its
        children's) for shine_plan_batch / shine_sample_sorted: sorted on the device, once per tree growth."""
        n_buckets = C.c_int64()
        _lib.check(_lib.lib().shine_tables_rank_nodes(self._tables.handle, C.byref(n_buckets),
                                                      torch.cuda.current_stream(dev).cuda_stream),
                   "shine_tables_rank_nodes")
        self._n_buckets = int(n_buckets.value)
        self._ranks_uploaded = True

    def _host_node_ranks(self):
        """The same ranking on the host (numpy): per featured slot an int32 array aligned with _node_keys.
        Test oracle for shine_tables_rank_nodes and feeder of shine_tables_set_ranks."""
        self._sync_host()
        L = self.featured_level_num
        ext = []
        for s in range(L):
            sh = 3 * (L - 1 - s)
            k = self._node_keys[s].astype(np.int64)
            ext.append(((k << sh) | ((1 << sh) - 1)) * 8 + (L - 1 - s))  # end of the subtree range; deeper first
        ext_all = np.concatenate(ext)
        order = np.argsort(ext_all, kind="stable")
        rank_all = np.empty(order.size, np.int32)
        rank_all[order] = np.arange(order.size, dtype=np.int32)
        out, off = [], 0
        for s in range(L):
            n = self._node_keys[s].size
            out.append(rank_all[off:off + n].copy())
            off += n
        return out

    DEBUG_VARIANT_BITS = 0  # measurement only (tools/): OR-ed into every launch's kernel_variant, e.g. 0x800 = plan with the counting sort

    def _bump_epoch(self):
        """the tables changed (nodes added, handle rebuilt): planned pools are stale, and so is every pending C++ autograd node of
        this octree — the extension's state learns the new epoch at once (csrc/shine_torch_ext.cpp TierAState::check_epoch)"""
        self._tables_epoch = getattr(self, "_tables_epoch", 0) + 1
        st = self.__dict__.get("_ext_st")
        if st is not None:
            st.set_epoch(int(self._tables_epoch))

    def _ext_state(self, ext):
        """The C++ extension's view of this octree (csrc/shine_torch_ext.cpp TierAState): table handle, scalar configuration,
        row counts — refreshed when the tables grew or were rebuilt (both bump _tables_epoch)."""
        d = self.__dict__
        key = (self._tables_epoch, self._tables.handle.value if self._tables is not None else 0, len(self.hier_features),
               FeatureOctree.DEBUG_VARIANT_BITS)
        st = d.get("_ext_st")
        if st is None or d.get("_ext_key") != key:
            if st is None:
                st = d["_ext_st"] = ext.TierAState()
            st.set(int(self._tables.handle.value), bytes(self.step_config()), [int(r) for r in self.row_counts()],
                   _ext.register(self), self._growth_stream is not None, int(self._tables_epoch),
                   (weakref.ref(self), weakref.ref(self._tables)))  # (weak: this state lives in the octree's own __dict__)
            d["_ext_key"] = key
        return st

    def step_config(self, with_sort_box=False, **kw) -> _lib.StepConfig:
        cfg = _lib.StepConfig()
        cfg.n_levels = self.featured_level_num
        cfg.max_level = self.max_level
        cfg.poly_int_on = 1 if self.polynomial_interpolation else 0
        cfg.sigma = 1.0
        cfg.inv_n = 1.0
        if with_sort_box:  # only shine_morton_sort reads it (dp.morton_order); it costs a host read after a device-side update
            origin, bits = self._sort_box()
            cfg.sort_origin[0], cfg.sort_origin[1], cfg.sort_origin[2] = origin
            cfg.sort_bits[0], cfg.sort_bits[1], cfg.sort_bits[2] = bits
        for k, v in kw.items():
            setattr(cfg, k, v)
        cfg.kernel_variant |= FeatureOctree.DEBUG_VARIANT_BITS
        return cfg

    def _sort_box(self):
        """Leaf-level voxel bounding box of the map (from the coarsest featured level's nodes, tracked as the tree
        grows): lets shine_morton_sort use bx+by+bz-bit keys instead of 3*tree_level_world."""
        self._drain_dev_frames()
        if self._box_pending:  # coarse node keys the device added since the box was last read: one host read, on demand
            pend, self._box_pending = self._box_pending, []
            for keys in pend:
                self._grow_box(keys.cpu().numpy())
        if self._sort_box_cache is None:
            if self._box is None:
                self._sort_box_cache = ((0, 0, 0), (0, 0, 0))
            else:
                shift = self.featured_level_num - 1  # coarsest featured level -> leaf voxel units
                lo = (self._box[0] << shift) - (1 << shift)  # one coarse cell of margin for free-space samples
                hi = ((self._box[1] + 2) << shift)
                lo = np.maximum(lo, 0)
                bits = tuple(min(self.max_level, max(1, int(int(e) - 1).bit_length())) for e in (hi - lo))
                self._sort_box_cache = (tuple(int(v) for v in lo), bits)
        return self._sort_box_cache

    def feature_list(self):
        """hier_features as a plain list (top-down).  nn.ParameterList.__getitem__ costs ~2 us per access; the small-batch
        loop touches the levels a dozen times per iteration.  Re-read whenever an entry was replaced."""
        cache = self.__dict__.get("_feat_list")
        hf = self.hier_features
        if cache is None or len(cache) != len(hf) or any(a is not b for a, b in zip(cache, hf._parameters.values())):
            cache = list(hf._parameters.values())
            self.__dict__["_feat_list"] = cache
        return cache

    def feature_ptrs(self):
        return _lib.ptr_array([p.data_ptr() for p in self.feature_list()])

    def row_counts(self):
        return _lib.i64_array([p.shape[0] - 1 for p in self.feature_list()])

    @staticmethod
    def _check_coord(coord):
        if not (coord.is_cuda and coord.dtype == torch.float32 and coord.dim() == 2 and coord.shape[1] == 3):
            raise ValueError("coord must be a CUDA float32 tensor of shape [N,3]")
        return coord.contiguous()

    # ------------------------------------------------------------------ :199-218
    def get_indices(self, coord):
        t = self._require_tables()
        coord = self._check_coord(coord.detach())
        n = coord.shape[0]
        out = [torch.empty((n, 8), dtype=torch.int64, device=coord.device) for _ in range(self.featured_level_num)]
        cfg = self.step_config()
        _lib.check(
            _lib.lib().shine_query_indices(
                t.handle, C.byref(cfg), coord.data_ptr(), n, _lib.ptr_array([o.data_ptr() for o in out]),
                torch.cuda.current_stream().cuda_stream,
            ),
            "shine_query_indices",
        )
        self.hierarchical_indices = out
        return out

    # ------------------------------------------------------------------ :237-244
    def query_feature(self, coord, faster=False):
        """`faster` (get_indices_fast, :267-286) is a CPU-side dedup trick; on the GPU both paths are the same."""
        # set_zero (:238) happens inside the forward kernel (shine_forward re-zeroes the trash rows): L python index ops and L
        # fill launches less per query
        feat = _ops().octree_interp(self, coord)
        if feat.requires_grad:  # lets Decoder.sdf fuse the two calls into one autograd node (autograd_ops.FusedInterpSdf)
            feat._shine_src = autograd_ops.FeatureSource(self, coord, feat)
        return feat

    # ------------------------------------------------------------------ :246-255
    def cal_regularization(self):
        """shine_incre.py:152-158 calls this right after `feature = octree.query_feature(coord)`: the rows of THAT query are what
        the reference's unique(hierarchical_indices) selects.  When the indices have not been materialised (a training loop:
        nothing read them) the regulariser is one autograd node over two HIP launches (autograd_ops.OctreeRegularizer);
        otherwise — indices set from outside, CPU tensors, more than 4 levels — the reference's composite below."""
        d = self.__dict__
        coord = d.get("_hidx_coord")
        riding = d.get("_reg_riding")
        if (riding is not None and coord is not None and d.get("_hidx") is None and d.get("_hidx_epoch") == self._tables_epoch
                and d.get("_reg_riding_versions") == self._reg_versions()):
            # the query's own launch evaluated it (_reg_rider: value only, its gradient cancels): no launch but the copy that
            # takes the number out of the rider's ring — unless a feature, features_last_frame or importance_weight was written
            # since the query (an optimiser step, an in-place update): then the regulariser's own launches below
            return riding.clone()
        if (coord is not None and d.get("_hidx") is None and d.get("_hidx_epoch") == self._tables_epoch and coord.is_cuda
                and self.featured_level_num <= 4 and len(self.importance_weight) == self.featured_level_num
                and len(self.features_last_frame) == self.featured_level_num
                and all(a.shape == p.shape and b.shape == p.shape and a.is_cuda and b.is_cuda
                        for a, b, p in zip(self.importance_weight, self.features_last_frame, self.hier_features))):
            live = self._reg_live_levels()
            if live is not None:
                ext = _ext.module()
                if ext is not None:  # the C++ node (csrc/shine_torch_ext.cpp) — a node at all only while a gradient is live
                    self._require_tables()
                    return ext.cal_regularization(self._ext_state(ext), coord, self.feature_list(), list(self.features_last_frame),
                                                  list(self.importance_weight), self._reg_row_flags(coord.device), live)
                return autograd_ops.OctreeRegularizer.apply(self, coord, *self.feature_list())
        return self._cal_regularization_composite()

    def _reg_versions(self):
        """the in-place write counters of the tensors the regulariser reads"""
        return tuple(t._version for ts in (self.hier_features, self.features_last_frame, self.importance_weight) for t in ts)

    def _reg_live_levels(self):
        """OctreeRegularizer.levels_with_gradient, remembered for as long as the tensors it looked at are the same objects (they
        change once per frame, the loop asks once per iteration)"""
        d = self.__dict__
        hit = d.get("_reg_live")
        last, feats = self.features_last_frame, self.hier_features
        if (hit is not None and len(hit[0]) == len(last) and len(hit[1]) == len(feats)
                and all(a is b and a.requires_grad == r for a, b, r in zip(hit[0], last, hit[2]))
                and all(a is b for a, b in zip(hit[1], feats))):
            return hit[3]
        live = autograd_ops.OctreeRegularizer.levels_with_gradient(self)
        d["_reg_live"] = (tuple(last), tuple(feats), tuple(x.requires_grad for x in last), live)
        return live

    def _reg_row_flags(self, dev):
        """the regulariser's per-row byte flags (all zero between its launches)"""
        d = self.__dict__
        flags = d.get("_reg_flags")
        if flags is None or any(f.shape[0] != p.shape[0] or f.device != dev for f, p in zip(flags, self.hier_features)):
            flags = d["_reg_flags"] = _ops().touched_flags(self)
            d["_reg_flags_dirty"] = False
        if d.get("_reg_flags_dirty"):  # a forward of the Python node whose backward never came left its rows flagged
            for f in flags:
                f.zero_()
            d["_reg_flags_dirty"] = False
        return flags

    def _cal_regularization_composite(self):
        regularization = 0.0
        for i in range(self.featured_level_num):
            feature_level = self.featured_level_num - i - 1
            unique_indices = self.hierarchical_indices[i].flatten().unique()
            difference = self.hier_features[feature_level][unique_indices] - \
                self.features_last_frame[feature_level][unique_indices]
            regularization = regularization + (self.importance_weight[feature_level][unique_indices] *
                                               (difference ** 2)).sum()
        return regularization

    # ------------------------------------------------------------------ :288-298
    def print_detail(self):
        print("Current Octomap:")
        total = 0
        for level in range(self.featured_level_num):
            size = self.leaf_vox_size * (2 ** (self.featured_level_num - 1 - level))
            count = self.hier_features[level].shape[0]
            print("%.2f m: %d voxel corners" % (size, count))
            total += count
        print("memory: %d x %d x 4 = %.3f MB" % (total, self.feature_dim, total * self.feature_dim * 4 / 1024 / 1024))
        print("--------------------------------")

    # ------------------------------------------------------------------ checkpoints (utils/tools.py:200-213 pickles the module)
    def __getstate__(self):
        self._sync_host()
        self._sort_box()  # folds the coarse node keys the device added into the host-side box (device tensors do not pickle)
        state = self.__dict__.copy()
        state["_tables"] = None
        state["_hidx_coord"] = None
        state.pop("_spec_decoder", None)
        state.pop("_spec_result", None)
        state.pop("_ext_st", None)
        state.pop("_ext_key", None)
        state.pop("_reg_flags", None)
        for k in ("_rider_key", "_rider_on", "_rider_keep", "_rider_stamps", "_rider_acc", "_reg_riding", "_reg_riding_versions"):
            state.pop(k, None)
        state["_dict_cache"] = None
        state["_pending"] = None
        state["_dev_log"] = None
        state["_dev_frames"] = None
        for k in ("_growth_stream", "_ev_read", "_ev_grown"):
            state[k] = None
        state["_probe_pending"] = state["_ev_read_valid"] = False
        state.pop("_feat_list", None)
        return state

    def __setstate__(self, state):
        if "_node_keys" not in state and "nodes_lookup_tables" in state:
            return self._adopt_reference_state(state)
        self.__dict__.update(state)
        self.rebuild_device_tables()

    def _adopt_reference_state(self, state):
        """Unpickling a checkpoint the REFERENCE wrote (utils/tools.py:200-213 pickles its whole FeatureOctree module;
        with shine_mapping_amd.dropin installed the class path resolves here).  Its __dict__ carries the plain python
        dict tables (model/feature_octree.py:47-52); they go through load_tables().  One-way: a pickle written by this
        class names shine_mapping_amd.feature_octree.FeatureOctree and needs this package to load."""
        state = dict(state)
        nodes = state.pop("nodes_lookup_tables")
        state.pop("corners_lookup_tables", None)  # re-derived from the node tables (same ids)
        self.__dict__.update(state)
        L = self.featured_level_num
        if self.feature_dim != _lib.FEATURE_DIM:
            raise NotImplementedError("libshine_hip is built for feature_dim == 8 (every shipped config)")
        self._node_keys = [np.zeros(0, np.int64) for _ in range(L)]
        self._node_ids = [np.zeros((0, 8), np.int32) for _ in range(L)]
        self._node_sorted = [np.zeros(0, np.int64) for _ in range(L)]
        self._corner_lex = [np.zeros(0, np.int64) for _ in range(L)]
        self._corner_id_of_lex = [np.zeros(0, np.int64) for _ in range(L)]
        self._corner_count = [0] * L
        self._dict_cache = self._sort_box_cache = self._tables = self._box = None
        self._box_pending = []
        self._ranks_uploaded = False
        self._n_buckets = 0
        self._tables_epoch = 0
        self._pending = [[] for _ in range(L)]
        self._dev_log = [[] for _ in range(L)]
        self._dev_frames = []
        self._corners_on_device = False
        # features_last_frame as pickled are plain tensors: the attached-clone quirk (:160) does not survive a pickle
        self._reg_grad_on = [True] * L
        tables = []
        for s in range(L):
            tab = nodes[self.free_level_num + s]
            keys = torch.tensor(list(tab.keys()), dtype=torch.int64)
            ids = torch.tensor(list(tab.values()), dtype=torch.int32).reshape(-1, 8)
            tables.append((keys, ids))
        self.load_tables(tables)

    def rebuild_device_tables(self):
        """Drop the library handle; it is re-created from the host copies at the next query / device update
        (after unpickling, a device move, or a host-side update that follows device-side ones)."""
        if getattr(self, "_dev_log", None) or getattr(self, "_dev_frames", None):
            self._sync_host()
        self._dev_log = [[] for _ in range(self.featured_level_num)]
        self._dev_frames = []
        self._corners_on_device = False
        if getattr(self, "_box_pending", None) is None:  # (pickles written before the box became lazy)
            self._box_pending = []
        if getattr(self, "_box", None) is None and not self._box_pending:
            self._box = None
            self._grow_box(self._node_keys[0])
        self._tables = None
        self._ranks_uploaded = False
        self._bump_epoch()
        self._pending = [[(self._node_keys[s], self._node_ids[s])] if self._node_keys[s].size else []
                         for s in range(self.featured_level_num)]

    def load_tables(self, tables):
        """Adopt externally built tables: per featured slot (top-down) a (node_morton[int64 n], corner_ids[int32 n,8])
        pair, e.g. from a reference checkpoint's nodes_lookup_tables.  Feature rows must be set by the caller."""
        self._tables = None
        self._dict_cache = None
        self._sort_box_cache = None
        self._dev_log = [[] for _ in range(self.featured_level_num)]
        self._dev_frames = []
        self._box = None
        self._box_pending = []
        for s, (keys, ids) in enumerate(tables):
            keys_np = keys.cpu().numpy().astype(np.int64)
            ids_np = ids.cpu().numpy().astype(np.int32).reshape(-1, 8)
            self._node_keys[s], self._node_ids[s] = keys_np, ids_np
            self._node_sorted[s] = np.sort(keys_np)
            corners = morton_decode(keys_np)[:, None, :] + _CORNER_OFFSETS[None, :, :]
            lex = _pack_lex(corners.reshape(-1, 3))
            uniq, first_idx = np.unique(lex, return_index=True)
            self._corner_lex[s] = uniq
            self._corner_id_of_lex[s] = ids_np.reshape(-1)[first_idx].astype(np.int64)
            self._corner_count[s] = int(ids_np.max()) + 1 if ids_np.size else 0
        self._grow_box(self._node_keys[0])
        self.rebuild_device_tables()
