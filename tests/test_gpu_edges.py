"""GPU suite (-m gpu), part 3: inputs where per-point and per-run decisions change.

(1) The edge fixtures (oracle/make_golden.py edge_batch, recorded from the reference): coordinates on voxel vertices / edges / faces
of every level (F1), one ulp either side (F2), on the cube's boundary (F3), outside it (F4), misses (F5), duplicates (F6) — through
every entry point, against the recorded reference AND the oracle's wide mode (fp32 voxel ids and d, fp64 downstream).
(2) Degenerate batch structures (one node, one point, all misses, hit/miss alternating, two nodes interleaved, runs ending on
tile and wave-share boundaries, ragged sizes) at both launch geometries and with the FAR build, against the oracle.
(3) The regulariser rider's lifecycle on one octree (off -> on again; tensors changed between the query and cal_regularization).

Tolerances are the suite's: indices / masks / slots / orders exact; values TOL against the reference; against fp64 no farther
than max(TOL x scale, the fp32 oracle's own distance from it) (test_gpu_scale_parity.py's policy); g by the ReLU-kink rule.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, oracle_from_golden, oracle_from_product, product_from_golden
from test_gpu_parity import TOL, abs_err, decoder_grad_errs, rel_err, step_options
from test_gpu_scale_parity import _workload, node_name

pytestmark = pytest.mark.gpu

EDGES = ["edges_L3", "edges_L2_nopoly_eik"]
V3_TP = 16  # points per tile of the fused step (csrc/shine_tile16.hpp)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return load_golden(name)


@functools.lru_cache(maxsize=None)
def _wide(name):
    """The oracle's wide mode on a fixture's batch (fp32 voxel ids and d, fp64 everything downstream)."""
    from oracle import shine_oracle as so

    fx = _fixture(name)
    ocfg, oct_, mlp = oracle_from_golden(fx)
    so.to_wide(oct_, mlp)
    return so.train_step(oct_, mlp, fx["coord"], fx["sdf_label"], fx["weight"], ocfg), mlp


def _assert_g(g, ref, mlp, what):
    """g against a reference g: TOL of max |g|, except points at a ReLU kink of the reference decoder (|z| < 1e-5 for some hidden
    unit), of which there may be a handful (test_gpu_scale_parity.py's rule)."""
    gr = ref["g"].double()
    err = (g.detach().double().cpu() - gr).abs().max(dim=1).values / max(float(gr.abs().max()), 1e-30)
    bad = torch.nonzero(err > TOL).flatten()
    assert bad.numel() <= max(2, g.shape[0] // 20000), "%s: %d points of g off" % (what, bad.numel())
    if bad.numel():
        f = ref["feat"][bad].double()
        W1, b1, W2, b2 = (t.detach().double() for t in mlp.params()[:4])
        z1 = f @ W1.T + b1
        z2 = torch.relu(z1) @ W2.T + b2
        zmin = torch.minimum(z1.abs().min(dim=1).values, z2.abs().min(dim=1).values)
        assert float(zmin.max()) < 1e-5, "%s: a point of g off by more than TOL is not at a ReLU kink" % what


def _check(what, ref, wide, loss, pred, g, feat_grads, mlp_grads, mlp64, order=None, pred_scale=1.0):
    """One entry point's results against the fp32 reference `ref` (TOL) and the wide oracle `wide` (no farther than
    max(TOL x scale, ref's own distance)).  `order`: the batch's order relative to ref / wide (pool batches).  `pred_scale`: pred
    is held to TOL x pred_scale (tests/step_value_cases.py: max(1, max |reference pred|) on maps whose logits reach 80)."""
    sel = (lambda t: t) if order is None else (lambda t: t[order])
    if pred is not None:
        assert abs_err(pred, sel(ref["pred"])) <= TOL * pred_scale, what + ": pred"
        assert abs_err(pred, sel(wide["pred"])) <= max(TOL * pred_scale, abs_err(sel(ref["pred"]), sel(wide["pred"]))), \
            what + ": pred (wide)"
    if loss is not None:
        r, w = float(ref["loss"]), float(wide["loss"])
        assert abs(float(loss) - r) <= TOL * max(1.0, abs(r)), what + ": loss"
        assert abs(float(loss) - w) <= max(TOL * max(1.0, abs(w)), abs(r - w)), what + ": loss (wide)"
    if g is not None and ref["g"] is not None:
        sref = dict(g=sel(ref["g"]), feat=sel(ref["feat"]))
        _assert_g(g, sref, mlp64, what + ": g")
        _assert_g(g, dict(g=sel(wide["g"]), feat=sel(wide["feat"])), mlp64, what + ": g (wide)")
    for k, (ours, r, r64) in enumerate(zip(feat_grads, ref["feat_grads"], wide["feat_grads"])):
        assert rel_err(ours, r) <= TOL, "%s: feature grad level %d" % (what, k)
        scale = float(r64.abs().max())
        own = float((r.double() - r64).abs().max())
        assert float((ours.detach().double().cpu() - r64).abs().max()) <= max(TOL * scale, own), \
            "%s: feature grad level %d (wide)" % (what, k)
        assert float((ours[-1].detach().double().cpu() - r64[-1]).abs().max()) <= max(TOL * scale, own), \
            "%s: trash row level %d (wide)" % (what, k)
    if mlp_grads is not None:
        errs = decoder_grad_errs(mlp_grads, ref["mlp_grads"])
        assert max(errs) <= TOL, (what + ": decoder grads", errs)
        own = decoder_grad_errs([t.double() for t in ref["mlp_grads"]], wide["mlp_grads"])
        errs64 = decoder_grad_errs(mlp_grads, wide["mlp_grads"])
        assert all(e <= max(TOL, o) for e, o in zip(errs64, own)), (what + ": decoder grads (wide)", errs64, own)


# ----------------------------------------------------------------------------------------------------------- (1) edge fixtures


@pytest.mark.parametrize("name", EDGES)
def test_edge_indices_masks_and_forward(name):
    """hierarchical_indices (forward_sdf, get_indices) and the mesher's mc_mask exact; pred / feat / g of the forward kernel and
    the mesher's SDF against the reference and the wide oracle."""
    from shine_mapping_amd import forward_sdf
    from shine_mapping_amd.mesher import Mesher

    fx = _fixture(name)
    ref, (wide, mlp64) = fx["out"], _wide(name)
    cfg, octree, dec = product_from_golden(fx)
    coord = fx["coord"].cuda()
    eik = ref["g"] is not None
    out = forward_sdf(octree, dec, coord, want_feat=True, want_indices=True, want_grad_x=eik, sigma=fx["sigma"])
    torch.cuda.synchronize()
    for k, r in enumerate(ref["indices"]):
        assert torch.equal(out["indices"][k].cpu(), r), "forward_sdf indices[%d]" % k
    idx = octree.get_indices(coord)
    for k, r in enumerate(ref["indices"]):
        assert torch.equal(idx[k].cpu(), r), "get_indices[%d]" % k
    assert abs_err(out["feat"], ref["feat"]) <= TOL
    assert abs_err(out["feat"], wide["feat"]) <= max(TOL, abs_err(ref["feat"], wide["feat"]))
    _check("forward_sdf", ref, wide, None, out["pred"], out["grad_x"] if eik else None, [], None, mlp64)
    L = cfg.tree_level_feat
    for vis in range(1, L + 1):  # utils/mesher.py:47,78-86: all 8 corners present at level min(L, mc_vis_level) - 1
        cfg.mc_vis_level = vis
        mesher = Mesher(cfg, octree, dec.cuda(), None)
        sdf, sem, mask = mesher.query_points(coord, 10 ** 9, True, False, True)
        want = (ref["indices"][min(L, vis) - 1] >= 0).all(1).numpy()
        assert np.array_equal(mask.astype(bool), want), "mc_mask, mc_vis_level %d" % vis
        assert np.abs(sdf.astype("float64") + ref["pred"].double().numpy()).max() <= TOL
        _, _, m2 = mesher.query_points(coord, 257, False, False, True)  # chunked: chunk ends fall anywhere in the families
        assert np.array_equal(m2.astype(bool), want)


@pytest.mark.parametrize("name", EDGES)
def test_edge_fused_step_every_form(name):
    """fused_train_step on the edge batch: product kernel (variant 0) and the check library's lane-per-point kernel (variant 1),
    unplanned and planned; pool-record mode on the same samples (slots memoised in the records == a fresh probe); the planner's
    node order."""
    from shine_mapping_amd import dp, fused_train_step
    from shine_mapping_amd.sampler import SortedPool

    fx = _fixture(name)
    ref, (wide, mlp64) = fx["out"], _wide(name)
    coord, label, weight = fx["coord"].cuda(), fx["sdf_label"].cuda(), fx["weight"].cuda()
    n, L = coord.shape[0], len(ref["indices"])
    for variant in (0, 1):
        for planned in (False, True):
            cfg, octree, dec = product_from_golden(fx)
            opts = step_options(fx)
            opts.kernel_variant = variant
            kw = {}
            if planned:
                perm, slots = dp.plan_batch(octree, coord)
                kw = dict(perm=perm, slots=slots)
            loss, pred, g = fused_train_step(octree, dec, coord, label, weight, opts, want_grad_x=True, **kw)
            torch.cuda.synchronize()
            _check("step v%d %s" % (variant, "planned" if planned else "unplanned"), ref, wide, loss, pred, g,
                   [p.grad for p in octree.hier_features], [p.grad for p in dec.fused_params()], mlp64)
            assert all(float(p[-1].abs().max()) == 0.0 for p in octree.hier_features)  # set_zero

    # the planner: a permutation in node order, slots == the hits of the reference's indices
    cfg, octree, dec = product_from_golden(fx)
    perm, slots = dp.plan_batch(octree, coord, _debug_variant=0x800, sort=False)
    p = perm.cpu().long()
    assert torch.equal(torch.sort(p).values, torch.arange(n))
    sl = slots.cpu()
    for s in range(L):
        assert torch.equal(sl[:, s] >= 0, (ref["indices"][L - 1 - s][:, 0] >= 0)[p]), "plan slots level %d" % s
    deepest = torch.full((n,), -1, dtype=torch.int64)
    for s in range(L):
        deepest = torch.where(sl[:, s] >= 0, sl[:, s].long() + (s << 40), deepest)
    assert int((deepest[1:] != deepest[:-1]).sum()) + 1 == len(torch.unique(deepest)), "a node's points split into runs"
    _, fresh = dp.plan_batch(octree, coord, sort=False)  # n <= 16384: identity order, slots of a fresh probe
    fresh = fresh.cpu()
    assert torch.equal(sl, fresh[p]), "planner slots != a fresh probe"

    # pool-record mode: the pool is the edge batch itself, drawn whole
    octree._require_tables(with_ranks=True)
    sp = SortedPool(octree, coord, label, weight, seed=5)
    order = sp.perm.cpu().long()
    assert torch.equal(torch.sort(order).values, torch.arange(n))
    if sp.rec is not None:
        slot0 = 4 if L == 4 else 5  # csrc/shine_step_body.hpp RecLayout
        rec_slots = sp.rec.view(torch.int32)[:, slot0:slot0 + L].cpu()
        assert torch.equal(rec_slots, fresh[order]), "slots memoised in the records != a fresh probe"
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    c, l, w = sp.get_batch(idx)
    assert torch.equal(c.cpu(), fx["coord"][order]) and torch.equal(w.cpu(), fx["weight"][order])
    loss, pred, g = fused_train_step(octree, dec, None, None, None, step_options(fx), want_grad_x=True, pool=sp, idx=idx)
    torch.cuda.synchronize()
    _check("pool-record step", ref, wide, loss, pred, g, [p.grad for p in octree.hier_features],
           [p.grad for p in dec.fused_params()], mlp64, order=order)


@pytest.mark.parametrize("name", EDGES)
def test_edge_autograd_entry_points(name):
    """query_feature through the C++ node and the Python OctreeInterp, the Tier A fused node (backward: the EXT build via
    shine_interp_sdf_backward) and the split nodes with the eikonal double backward — each with the reference's loss."""
    from shine_mapping_amd import autograd_ops, get_gradient, sdf_bce_loss

    fx = _fixture(name)
    ref, (wide, mlp64) = fx["out"], _wide(name)
    sigma, c = fx["sigma"], fx["cfg"]
    eik = c.get("ekional_loss_on", False)
    label, weight = fx["sdf_label"].cuda(), fx["weight"].cuda()
    red = c.get("loss_reduction", "mean")

    def loop(mode):
        autograd_ops.FUSE_WITH_COORD_GRAD = mode == "fused"
        try:
            cfg, octree, dec = product_from_golden(fx)
            coord = fx["coord"].cuda().requires_grad_(eik)
            if mode == "python node":
                feature = autograd_ops.OctreeInterp.apply(coord, octree, *octree.feature_list())
            else:
                feature = octree.query_feature(coord)
            if mode == "split":
                feature = feature * 1.0  # (a driver that touches the feature tensor: the split nodes)
            pred = dec.sdf(feature)
            assert ("FusedInterpSdf" in node_name(pred.grad_fn)) == (mode == "fused"), (mode, node_name(pred.grad_fn))
            loss = sdf_bce_loss(pred, label, sigma, torch.abs(weight), False, red)
            g = None
            if eik:
                g = get_gradient(coord, pred) * sigma
                loss = loss + c["weight_e"] * ((1.0 - g[weight > 0].norm(2, dim=-1)) ** 2).mean()
            loss.backward()
            torch.cuda.synchronize()
            assert all(float(p[-1].abs().max()) == 0.0 for p in octree.hier_features)
            _check("autograd " + mode, ref, wide, loss.detach(), pred, None if g is None else g.detach(),
                   [p.grad for p in octree.hier_features], [p.grad for p in dec.fused_params()], mlp64)
            assert abs_err(feature, ref["feat"]) <= TOL
        finally:
            autograd_ops.FUSE_WITH_COORD_GRAD = False

    for mode in ("fused", "split", "python node"):
        loop(mode)


# --------------------------------------------------------------------------------------------- (2) degenerate batch structures


def _wave_share_starts(n, eik):
    """First point of every wave's share of tiles (csrc/shine_step_v3.hip v3_geometry + shine_step_body.hpp's split)."""
    tiles = max(1, (n + V3_TP - 1) // V3_TP)
    wg = 4 if tiles < 2048 else 8
    waves = min(tiles, 256 * 8)
    blocks = (waves + wg - 1) // wg
    starts = set()
    old = 140 if eik else 128
    for b in range(blocks):
        t0, t1 = b * tiles // blocks, (b + 1) * tiles // blocks
        nt, hw = t1 - t0, wg // 2
        cut = (nt * old) >> 8 if (wg >= 8 and nt >= 4 * wg) else nt // 2
        for wv in range(wg):
            lo = (wv * cut) // hw if wv < hw else cut + ((wv - hw) * (nt - cut)) // hw
            starts.add(V3_TP * (t0 + lo))
    return sorted(s for s in starts if 0 < s < n)


@functools.lru_cache(maxsize=None)
def _degenerate_map(levels):
    wl = _workload("maicity", levels, frames=4)
    octree = wl.octree
    c = wl.pool.coord
    idx = octree.get_indices(c)
    hits = torch.stack([(t >= 0).all(1) for t in idx], 1)  # bottom-up
    return wl, c, hits


def _voxel_points(center, level, n, g):
    """n points strictly inside the level-`level` voxel that holds `center` (fp32, exact voxel)."""
    res = 2 ** level
    v = torch.floor(torch.clamp(res * (center + 1.0) / 2.0, 0, res - 1.0))
    u = v + 0.05 + 0.9 * torch.rand((n, 3), generator=g, device=center.device)
    return (u * (2.0 / res) - 1.0).float()


def _structure(kind, n, wl, pool, hits, eik, g):
    """(coord [n, 3] in visiting order, keep_order) for the structures D1..D7 of the issue."""
    octree = wl.octree
    top = octree.max_level
    full = torch.nonzero(hits.all(1)).flatten()
    anchor = pool[full[0]]
    if kind == "one_leaf":  # D1
        return _voxel_points(anchor, top, n, g), False
    if kind == "identical":  # D2: all identical, on a vertex of the COARSEST featured level (so of every level) that hits
        res = 2 ** octree.free_level_num
        v = (torch.round((pool[full[:4096]] + 1.0) * (res / 2.0)) * (2.0 / res) - 1.0).float()
        ok = torch.stack([(t >= 0).all(1) for t in octree.get_indices(v)], 1).all(1)
        assert bool(ok.any()), "no coarse vertex with a node at every level"
        return v[torch.nonzero(ok).flatten()[0]].expand(n, 3).contiguous(), False
    if kind == "all_miss":  # D3
        cand = torch.rand((1 << 16, 3), generator=g, device="cuda") * 2 - 1
        miss = ~torch.stack([(t >= 0).any(1) for t in octree.get_indices(cand)], 1).any(1)
        cand = cand[miss]
        assert cand.shape[0] > 100
        return cand[torch.arange(n, device="cuda") % cand.shape[0]], False
    if kind == "alternate":  # D4: hit / miss alternating at the finest level under ONE coarse node
        for j in full[:200].tolist():
            base = _voxel_points(pool[j], top - 1, 4096, g)
            h = (octree.get_indices(base)[0] >= 0).all(1)
            if bool(h.any()) and bool((~h).any()):
                hit_pts, miss_pts = base[h], base[~h]
                break
        else:
            pytest.fail("no coarse node with a missing child in the map")
        k = torch.arange(n, device="cuda")
        out = torch.where((k % 2 == 0)[:, None], hit_pts[(k // 2) % hit_pts.shape[0]], miss_pts[(k // 2) % miss_pts.shape[0]])
        return out, True
    leaves = [pool[j] for j in full[torch.randperm(full.numel(), generator=torch.Generator().manual_seed(1))[:64]].tolist()]
    ids = [tuple(torch.floor(torch.clamp(2 ** top * (c + 1.0) / 2.0, 0, 2 ** top - 1.0)).tolist()) for c in leaves]
    uniq = [c for i, c in enumerate(leaves) if ids[i] not in ids[:i]]
    if kind == "interleaved":  # D5: two nodes, a run breaks at every point
        a, b = _voxel_points(uniq[0], top, n, g), _voxel_points(uniq[1], top, n, g)
        k = torch.arange(n, device="cuda")
        return torch.where((k % 2 == 0)[:, None], a, b), True
    if kind == "runs":  # D6: runs of 15 / 16 / 17 and runs ending exactly on (and one off) the wave-share boundaries
        cuts = set()
        pos, cyc = 0, [15, 16, 17, 16, 1, 33]
        while pos < n:
            pos += cyc[len(cuts) % len(cyc)]
            cuts.add(pos)
        ws = _wave_share_starts(n, eik)
        cuts |= set(ws) | {s + 1 for s in ws[::3]} | {s - 1 for s in ws[1::3]}
        cuts = torch.tensor(sorted(c for c in cuts if 0 < c < n), dtype=torch.int64)
        run = torch.searchsorted(cuts, torch.arange(n), right=True)
        K = len(uniq)
        assert K >= 3
        jitter = torch.stack([_voxel_points(c, top, 8, g) for c in uniq])  # [K, 8, 3]
        node = (run % K).cuda()
        return jitter[node, torch.arange(n, device="cuda") % 8], True
    raise ValueError(kind)


def _labels(n, sigma, g):
    lab = sigma * 3.0 * torch.randn(n, generator=g, device="cuda")
    w = torch.tensor([1.0, -1.0, 0.5], device="cuda")[torch.randint(0, 3, (n,), generator=g, device="cuda")]
    w[0] = 1.0
    return lab, w


def _run_structure(wl, coord, lab, w, keep_order, eik, variant):
    from shine_mapping_amd import StepOptions, dp, fused_train_step

    octree, dec, cfg = wl.octree, wl.decoder, wl.cfg
    params = list(octree.hier_features) + dec.fused_params()
    for p in params:
        p.grad = None
    opts = StepOptions(sigma=cfg.sigma_sigmoid, ekional_loss_on=eik, weight_e=cfg.weight_e, kernel_variant=variant)
    kw = {}
    if keep_order:  # the batch reaches the kernel in THIS order (a plan would sort it by node at n > 16384)
        perm, slots = dp.plan_batch(octree, coord)
        mine = torch.empty_like(slots)
        mine[perm.long()] = slots
        kw = dict(perm=torch.arange(coord.shape[0], dtype=torch.int32, device="cuda"), slots=mine)
    loss, pred, g = fused_train_step(octree, dec, coord, lab, w, opts, want_grad_x=True, **kw)
    torch.cuda.synchronize()
    return loss, pred, g, [p.grad.clone() for p in octree.hier_features], [p.grad.clone() for p in dec.fused_params()]


def _oracles(wl, coord, lab, w, eik):
    from oracle import shine_oracle as so

    octree, dec, cfg = wl.octree, wl.decoder, wl.cfg
    cfg.ekional_loss_on = eik
    ocfg, oct_, mlp = oracle_from_product(octree, dec, cfg)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    c, l, ww = coord.cpu(), lab.cpu(), w.cpu()
    ref = so.train_step(oct_, mlp, c, l, ww, ocfg)
    _, oct64, mlp64 = oracle_from_product(octree, dec, cfg)
    so.to_wide(oct64, mlp64)
    wide = so.train_step(oct64, mlp64, c, l, ww, ocfg)
    return ref, wide, mlp64


STRUCTURES = ["one_leaf", "identical", "all_miss", "alternate", "interleaved", "runs"]


@pytest.mark.parametrize("n", [(1 << 17) + 1, 20000])  # full-chip launch / 4-wave workgroups
@pytest.mark.parametrize("kind", STRUCTURES)
def test_degenerate_batch_structures(kind, n):
    """D1..D6 at both launch geometries, BCE and eikonal, the near build and (full-chip, L = 3) the FAR build forced."""
    wl, pool, hits = _degenerate_map(3)
    g = torch.Generator(device="cuda").manual_seed(STRUCTURES.index(kind) * 7 + n % 5)
    cfg = wl.cfg
    for eik in (False, True):
        coord, keep = _structure(kind, n, wl, pool, hits, eik, g)
        lab, w = _labels(n, cfg.sigma_sigmoid, g)
        ref, wide, mlp64 = _oracles(wl, coord, lab, w, eik)
        hit0 = (ref["indices"][0] >= 0).all(1)
        if kind in ("one_leaf", "identical"):
            assert bool(hit0.all())
        if kind == "all_miss":
            assert not any(bool((t >= 0).any()) for t in ref["indices"])
        if kind == "alternate":
            assert torch.equal(hit0, torch.arange(n) % 2 == 0)
        if kind == "identical" and cfg.poly_int_on and eik:
            assert float(ref["g"].abs().max()) == 0.0  # on a vertex every d = 0: dt = 6 (d - d^2) = 0
        for variant in ((0, 5) if n >= 32768 else (0,)):
            loss, pred, gg, fg, mg = _run_structure(wl, coord, lab, w, keep, eik, variant)
            what = "%s n=%d eik=%d v%d" % (kind, n, eik, variant)
            _check(what, ref, wide, loss, pred, gg if eik else None, fg, mg, mlp64)
            if kind == "identical" and cfg.poly_int_on and eik:
                assert float(gg.abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 15, 16, 17, 32767, 32768])
def test_ragged_batch_sizes_against_the_oracle(n):
    """D7: a partial first tile, exact tiles, one point over; the last size below and the first size of the full-chip launch."""
    wl, pool, hits = _degenerate_map(3)
    g = torch.Generator(device="cuda").manual_seed(n)
    sel = torch.randint(0, pool.shape[0], (n,), generator=g, device="cuda")
    coord = pool[sel].contiguous()
    lab, w = _labels(n, wl.cfg.sigma_sigmoid, g)
    for eik in (False, True):
        ref, wide, mlp64 = _oracles(wl, coord, lab, w, eik)
        loss, pred, gg, fg, mg = _run_structure(wl, coord, lab, w, False, eik, 0)
        _check("n=%d eik=%d" % (n, eik), ref, wide, loss, pred, gg if eik else None, fg, mg, mlp64)


@pytest.mark.parametrize("kind", ["one_leaf", "identical"])
@pytest.mark.parametrize("attached", [False, True])
def test_regulariser_on_batches_that_address_eight_rows(kind, attached, monkeypatch):
    """2^17 + 1 points that address only 8 rows per level: cal_regularization (its own launches, and riding on the query with
    features_last_frame an attached clone) against the reference's composite evaluated in fp64."""
    from shine_mapping_amd import feature_octree

    monkeypatch.setattr(feature_octree, "RIDER_ENABLED", True)
    wl, pool, hits = _degenerate_map(3)
    n = (1 << 17) + 1
    g = torch.Generator(device="cuda").manual_seed(11)
    coord, _ = _structure(kind, n, wl, pool, hits, False, g)
    octree = wl.octree
    feats = octree.hier_features
    saved = (octree.importance_weight, octree.features_last_frame)
    try:
        octree.importance_weight = [torch.rand(p.shape, generator=g, device="cuda") for p in feats]
        drift = [0.05 * torch.randn(p.shape, generator=g, device="cuda") for p in feats]
        if attached:
            octree.features_last_frame = [p.clone() for p in feats]
            with torch.no_grad():
                for t, d in zip(octree.features_last_frame, drift):
                    t.sub_(d)
        else:
            octree.features_last_frame = [(p.detach() - d) for p, d in zip(feats, drift)]
        octree.query_feature(coord)
        assert (octree.__dict__.get("_reg_riding") is not None) == attached
        got = float(octree.cal_regularization())
        exact = _composite64(octree, coord)
        assert abs(got - exact) <= TOL * abs(exact), (got, exact)
    finally:
        octree.importance_weight, octree.features_last_frame = saved


def _composite64(octree, coord):
    """FeatureOctree._cal_regularization_composite (model/feature_octree.py:246-255) on the current tensors, in fp64."""
    idx = octree.get_indices(coord.detach())
    L = octree.featured_level_num
    reg = 0.0
    for i in range(L):
        fl = L - i - 1
        u = idx[i].flatten().unique()  # (-1 included, as in the reference: the trash row)
        d = octree.hier_features[fl].detach().double()[u] - octree.features_last_frame[fl].detach().double()[u]
        reg += float((octree.importance_weight[fl].double()[u] * d * d).sum())
    return reg


# -------------------------------------------------------------------------------------------------- (3) the rider's lifecycle


def _rider_octree():
    fx = _fixture("ncd_reg_L3")
    cfg, octree, dec = product_from_golden(fx)
    vals = [v.detach().clone() for v in octree.features_last_frame]
    octree.features_last_frame = [p.clone() for p in octree.hier_features]  # attached clones: the rider rides
    with torch.no_grad():
        for t, v in zip(octree.features_last_frame, vals):
            t.copy_(v)
    return fx, octree


def _query_and_check(octree, q, rides, what):
    octree.query_feature(q)
    assert (octree.__dict__.get("_reg_riding") is not None) == rides, what
    got = float(octree.cal_regularization())
    exact = _composite64(octree, q)
    assert abs(got - exact) <= 1e-5 * max(abs(exact), 1e-30), (what, got, exact)


def test_regulariser_rider_off_and_on_again_on_one_octree(monkeypatch):
    """switching the rider off (RIDER_ENABLED, or features_last_frame detached) and on again on ONE octree must not
    restart its epoch under the stamps / accumulator ring of the earlier queries.  After every query cal_regularization() equals
    the composite on the current tensors — at least 9 queries after each re-enable, so the 8-slot ring wraps."""
    from shine_mapping_amd import feature_octree

    fx, octree = _rider_octree()
    base = fx["coord"].cuda()
    g = torch.Generator(device="cuda").manual_seed(7)

    def q(n):
        return base[torch.randint(0, base.shape[0], (n,), device="cuda", generator=g)]

    sizes = (1024, 17, 300, 1024, 999, 64, 1024, 512, 1024, 200, 1024)
    monkeypatch.setattr(feature_octree, "RIDER_ENABLED", True)
    for k, n in enumerate(sizes):
        _query_and_check(octree, q(n), True, "on #%d" % k)
    monkeypatch.setattr(feature_octree, "RIDER_ENABLED", False)  # off by the switch
    for k in range(3):
        _query_and_check(octree, q(700), False, "off #%d" % k)
    monkeypatch.setattr(feature_octree, "RIDER_ENABLED", True)
    for k, n in enumerate(sizes):
        _query_and_check(octree, q(n), True, "on again #%d" % k)
    attached = octree.features_last_frame  # off by a detached features_last_frame, then attached again
    octree.features_last_frame = [t.detach().clone() for t in attached]
    for k in range(3):
        _query_and_check(octree, q(700), False, "detached #%d" % k)
    octree.features_last_frame = attached
    for k, n in enumerate(sizes):
        _query_and_check(octree, q(n), True, "attached again #%d" % k)


@pytest.mark.parametrize("change", ["importance", "last_frame", "feature"])
def test_regulariser_value_follows_tensors_changed_after_the_query(change, monkeypatch):
    """a query, then importance_weight / features_last_frame / a feature changed in place, then cal_regularization():
    the value is the one of the CURRENT tensors (the reference evaluates at call time), not the one that rode on the query."""
    from shine_mapping_amd import feature_octree

    monkeypatch.setattr(feature_octree, "RIDER_ENABLED", True)
    fx, octree = _rider_octree()
    q = fx["coord"].cuda()
    octree.query_feature(q)
    riding = octree.__dict__.get("_reg_riding")
    assert riding is not None
    before = float(riding)
    with torch.no_grad():
        if change == "importance":
            for t in octree.importance_weight:
                t.mul_(3.0)
        elif change == "last_frame":
            for t in octree.features_last_frame:
                t.add_(0.01)
        else:
            for p in octree.hier_features:
                p.sub_(0.02)
    got = float(octree.cal_regularization())
    exact = _composite64(octree, q)  # (after: it materialises the indices, which takes cal_regularization off the rider)
    assert abs(exact - before) > 1e-3 * abs(before)
    assert abs(got - exact) <= 1e-5 * abs(exact), (change, got, exact, before)
