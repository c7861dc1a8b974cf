"""The time-conditioned training step on the device (csrc/shine_time_step.hip, ops.fused_time_step, SortedPool(ts=),
GraphedIteration's time route) against the fp64 oracle of tests/time_step_oracle.py and the torch composite.

The tolerance is the project's contract, TOL of tests/test_gpu_parity.py through normal_step_oracle.rel_errors: the loss
absolute-or-relative, each gradient tensor <= TOL of its max-abs against the oracle, an all-zero oracle tensor <= TOL of the
largest gradient tensor's max-abs; pred <= TOL of max(1, max |pred|).  tests/test_time_step.py shows on the CPU that the
reference's own fp32 evaluation sits within TOL / 4 on every case.
"""
import contextlib
import copy
import functools

import pytest
import torch

import step_value_cases as sv
import time_step_oracle as to
from conftest import oracle_from_golden, product_from_golden
from test_gpu_parity import TOL
from test_gpu_sem_step import LOOP_TOL, counted_launches, rel_err

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def time_calls():
    """the arguments of every shine_time_step call made inside the block"""
    from shine_mapping_amd import _lib

    lib, seen = _lib.lib(), []
    fn = lib.shine_time_step
    lib.shine_time_step = lambda *a: (seen.append(a), fn(*a))[1]
    try:
        yield seen
    finally:
        lib.shine_time_step = fn


def _clear(octree, dec):
    for p in list(octree.hier_features) + list(dec.parameters()):
        p.grad = None


def _opts(sigma, eik, weight_e=0.1, **kw):
    from shine_mapping_amd import StepOptions

    return StepOptions(sigma=float(sigma), ekional_loss_on=bool(eik), weight_e=float(weight_e), **kw)


def _fused(octree, dec, coord, label, weight, ts, opts, **kw):
    """-> (loss, feature grads, decoder grads | None, pred)"""
    from shine_mapping_amd import ops

    _clear(octree, dec)
    n = kw["idx"].numel() if kw.get("idx") is not None else coord.shape[0]
    pred = torch.full((n,), float("nan"), device="cuda")
    loss = ops.fused_time_step(octree, dec, coord, label, weight, ts, opts, pred_out=pred, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.grad_fn is None
    mlp = dec.time_params()
    out = (loss.clone(), [p.grad.clone() for p in octree.hier_features],
           None if mlp[0].grad is None else [p.grad.clone() for p in mlp], pred)
    _clear(octree, dec)
    return out


def _check(what, got, ref, tol=TOL):
    loss_err, errs = to.rel_errors(got[0], got[1], got[2], ref)
    pr = ref["pred"].double()
    pred_err = float((got[3].double().cpu() - pr).abs().max()) / max(1.0, float(pr.abs().max())) if pr.numel() else 0.0
    print(what, "loss %.1e pred %.1e" % (loss_err, pred_err), " ".join("%.1e" % e for e in errs))
    assert all(bool(torch.isfinite(t).all()) for t in [got[0], got[3]] + got[1] + got[2]), what
    assert loss_err <= tol and pred_err <= tol and max(errs) <= tol, (what, loss_err, pred_err, errs)


def _time_decoder(cfg, state, w_t):
    """Decoder(cfg, is_time_conditioned=True) holding a plain decoder's state dict widened by the column w_t"""
    from shine_mapping_amd import Decoder

    dec = Decoder(cfg, is_time_conditioned=True)
    sd = {k: v.clone().float() for k, v in state.items() if k in sv.NAMES}
    sd["layers.0.weight"] = torch.cat((sd["layers.0.weight"], w_t.reshape(-1, 1).float()), 1)
    dec.load_state_dict(sd, strict=False)
    assert dec.time_fusable
    return dec


@functools.lru_cache(maxsize=None)
def _product(name, kind):
    fx, ts, w_t = to.inputs(name, kind)
    cfg, octree, _ = product_from_golden(fx)
    return cfg, octree, _time_decoder(cfg, fx["decoder"], w_t)


def _dev(c):
    return c.coord.cuda(), c.label.cuda(), c.weight.cuda(), c.ts.cuda()


# ---- 1. one step on every case against the wide oracle
@pytest.mark.parametrize("name,kind,eik", to.CASES, ids=[to.case_id(*c) for c in to.CASES])
def test_one_step_matches_the_fp64_oracle(name, kind, eik):
    c = to.case(name, kind, eik)
    _, octree, dec = _product(name, kind)
    got = _fused(octree, dec, *_dev(c), _opts(c.sigma, eik, c.weight_e))
    _check(to.case_id(name, kind, eik), got, c.wide)
    if kind != "wt_zero":
        assert float(got[2][0][:, 8].abs().max()) > 0.0


# ---- 2. tile edges, and the same through a reversed gather
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2048])
def test_tile_edges_and_the_reversed_gather(n):
    name, kind = "kitti_eik_L3", "frames"
    c = to.case(name, kind, True)
    _, octree, dec = _product(name, kind)
    coord, label, weight, ts = _dev(c)
    assert coord.shape[0] >= 2048
    oct_, mlp = to.oracle_for(c.fx, c.w_t, wide=True)
    ref = to.time_step(oct_, mlp, c.coord[:n], c.label[:n], c.weight[:n], c.ts[:n], c.sigma, eik=True, weight_e=c.weight_e)
    opts = _opts(c.sigma, True, c.weight_e)
    plain = _fused(octree, dec, coord[:n].contiguous(), label[:n].contiguous(), weight[:n].contiguous(), ts[:n].contiguous(), opts)
    _check("n=%d" % n, plain, ref)
    idx = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")
    got = _fused(octree, dec, coord, label, weight, ts, opts, idx=idx)
    _check("n=%d gathered" % n, got[:3] + (got[3].flip(0),), ref)  # (pred is written at the batch position)


# ---- 2b. the grid sum's boundaries (a tile is 64 rows, a workgroup 4 tiles, a first-level run 16 workgroups): exactly one full
#      run, a run of one workgroup behind it, and every workgroup plus a grid-stride pass.  The fixture's 2048 rows repeated.  The
#      loss, the weight grads and pred are the same bits from call to call at each size.  The fp64 oracle takes half a minute at
#      65537 rows and its two terms have two divisors, so that size checks the deterministic outputs call to call only.
@pytest.mark.parametrize("n", [4096, 4113, 65537])
def test_grid_sum_boundary_sizes(n):
    name, kind = "kitti_eik_L3", "frames"
    c = to.case(name, kind, True)
    _, octree, dec = _product(name, kind)
    rows = torch.arange(n) % c.coord.shape[0]
    dev = [t[rows].contiguous().cuda() for t in (c.coord, c.label, c.weight, c.ts)]
    opts = _opts(c.sigma, True, c.weight_e)
    a, b = _fused(octree, dec, *dev, opts), _fused(octree, dec, *dev, opts)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and torch.equal(a[3], b[3]), n
    assert all(bool(torch.isfinite(t).all()) for t in [a[0], a[3]] + a[1] + a[2]) and float(a[0]) > 0.0
    if n > 8192:
        return
    oct_, mlp = to.oracle_for(c.fx, c.w_t, wide=True)
    ref = to.time_step(oct_, mlp, c.coord[rows], c.label[rows], c.weight[rows], c.ts[rows], c.sigma, eik=True, weight_e=c.weight_e)
    _check("n=%d" % n, a, ref)


def test_an_empty_batch_writes_a_zero_loss_and_nothing_else():
    from shine_mapping_amd import ops

    c = to.case("kitti_eik_L3", "frames", True)
    _, octree, dec = _product("kitti_eik_L3", "frames")
    coord, label, weight, ts = _dev(c)
    _clear(octree, dec)
    out = torch.full((1,), 7.0, device="cuda")
    loss = ops.fused_time_step(octree, dec, coord[:0], label[:0], weight[:0], ts[:0], _opts(c.sigma, True), out=out)
    assert float(loss) == 0.0 and float(out[0]) == 0.0
    assert all(float(p.grad.abs().max()) == 0.0 for p in list(octree.hier_features) + dec.time_params())
    _clear(octree, dec)


# ---- 3. every instantiation against the torch composite on the device
def _composite(octree, dec, coord, label, weight, ts, opts):
    """query_feature -> Decoder._time_composite -> sdf_bce_loss [+ eikonal] -> backward, the parent's route with torch's decoder"""
    from shine_mapping_amd import get_gradient, sdf_bce_loss

    _clear(octree, dec)
    eik = bool(opts.ekional_loss_on)
    x = coord.detach().clone().requires_grad_(eik)
    pred = dec._time_composite(octree.query_feature(x), ts)
    loss = sdf_bce_loss(pred, label, opts.sigma, None, False, opts.loss_reduction)
    if eik:
        g = get_gradient(x, pred) * opts.sigma
        surf = weight > 0
        if bool(surf.any()):
            loss = loss + opts.weight_e * ((1.0 - g[surf].norm(2, dim=-1)) ** 2).mean()
    loss.backward()
    out = dict(loss=loss.detach().cpu(), pred=pred.detach().cpu(),
               feat_grads=[p.grad.detach().cpu().clone() for p in octree.hier_features],
               mlp_grads=[(torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().clone() for p in dec.time_params()])
    _clear(octree, dec)
    return out


def _synth_time_decoder(cfg, seed=3, wt_scale=0.03):
    from shine_mapping_amd import Decoder

    torch.manual_seed(seed)
    dec = Decoder(cfg, is_time_conditioned=True)
    with torch.no_grad():
        dec.layers[0].weight[:, 8] *= wt_scale  # (frame ids reach 1100: the shift of the first bias stays of the bias's order)
    return dec


def _synth_batch(wl, n, seed):
    """n pool samples with frame ids; rows 3..6 are moved outside the mapped box (they miss every level) as surface rows"""
    from shine_mapping_amd import synth

    gen = torch.Generator(device="cuda").manual_seed(seed)
    coord, label, weight = synth.draw_batch(wl.pool, n, gen)
    coord, weight = coord.clone(), weight.clone()
    cell = wl.cfg.leaf_vox_size * wl.cfg.scale
    coord[3:7] = (wl.pool.coord.max(0).values + 3.0 * cell).clamp(max=0.999)
    weight[3:7] = 1.0
    ts = torch.randint(0, to.FRAMES, (n,), device="cuda", generator=gen).float()
    return coord.contiguous(), label.contiguous(), weight.contiguous(), ts


@pytest.mark.parametrize("eik", [False, True])
@pytest.mark.parametrize("poly", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_every_instantiation_matches_the_composite(L, poly, eik):
    from shine_mapping_amd import synth

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L,
                              poly_int_on=poly)
    assert wl.octree.featured_level_num == L and bool(wl.octree.step_config().poly_int_on) == poly
    dec = _synth_time_decoder(wl.cfg)
    batch = _synth_batch(wl, 1000, 5)
    opts = _opts(wl.cfg.sigma_sigmoid, eik, 0.1)
    ref = _composite(wl.octree, dec, *batch, opts)
    assert bool(torch.isfinite(ref["loss"])) and float(ref["feat_grads"][-1].abs().max()) > 0
    _check("L=%d poly=%d eik=%d" % (L, poly, eik), _fused(wl.octree, dec, *batch, opts), ref)


# ---- 4. the surface count's forms, and rows whose g is exactly zero
def test_no_surface_all_surface_and_surface_count_forms():
    name, kind = "maicity_bce_L3", "unit"
    c = to.case(name, kind, True)
    _, octree, dec = _product(name, kind)
    coord, label, weight, ts = _dev(c)
    opts = _opts(c.sigma, True, c.weight_e)
    oct_, mlp = to.oracle_for(c.fx, c.w_t, wide=True)
    # no surface row: the eikonal part is 0 and sends nothing — the BCE step's numbers
    free = -c.weight.abs() - 1.0
    got = _fused(octree, dec, coord, label, free.cuda(), ts, opts)
    ref = to.time_step(oct_, mlp, c.coord, c.label, free, c.ts, c.sigma, eik=True, weight_e=c.weight_e)
    bce = to.case(name, kind, False).wide
    assert float(ref["loss"]) == float(bce["loss"])
    _check("no surface", got, ref)
    # every row a surface row
    ones = torch.ones_like(c.weight)
    ref = to.time_step(oct_, mlp, c.coord, c.label, ones, c.ts, c.sigma, eik=True, weight_e=c.weight_e)
    _check("all surface", _fused(octree, dec, coord, label, ones.cuda(), ts, opts), ref)
    # the surface count as the draw's partial counts, and as one count: the same bits
    ns = int((c.weight > 0).sum())
    parts = torch.zeros(64, dtype=torch.int64, device="cuda")
    parts[0], parts[5], parts[63] = ns - 7, 4, 3
    one = torch.tensor([ns], dtype=torch.int64, device="cuda")
    a = _fused(octree, dec, coord, label, weight, ts, opts, n_surf=parts)
    b = _fused(octree, dec, coord, label, weight, ts, opts, n_surf=one)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    _check("n_surf parts", a, c.wide)
    # a caller-supplied (global) count is the divisor of the eikonal part
    twice = _fused(octree, dec, coord, label, weight, ts, opts, n_surf=2 * one)
    bce_loss, full = float(bce["loss"]), float(c.wide["loss"])
    assert abs(float(twice[0]) - (bce_loss + 0.5 * (full - bce_loss))) <= TOL * max(1.0, full)


def test_rows_with_a_zero_gradient_contribute_one_and_get_no_second_order_gradient():
    """step_value_cases' "dead_points": the features the first quarter of the batch addresses are zero, so A = 0 and g == 0 there
    exactly, whatever the time column does to the masks"""
    from oracle import shine_oracle as so

    name, kind = "kitti_eik_L3", "unit"
    fx, ts, w_t = to.inputs(name, kind)
    vc = sv.value_case(fx, "dead_points")
    pair = oracle_from_golden(fx)
    sv.apply_to_oracle(vc, pair)
    _, oct_, mlp = pair
    to.widen(mlp, w_t)
    so.to_wide(oct_, mlp)
    weight = fx["weight"].clone()
    weight[: fx["coord"].shape[0] // 4] = 1.0  # (every zero-g row a surface row)
    ref = to.time_step(oct_, mlp, fx["coord"], fx["sdf_label"], weight, ts, fx["sigma"], eik=True, weight_e=to.weight_e_of(fx))
    zero_rows = ref["g"][vc.zero_points]
    assert zero_rows.shape[0] >= 500 and float(zero_rows.abs().max()) == 0.0
    cfg, octree, _ = product_from_golden(fx)
    with torch.no_grad():
        for p, f in zip(octree.hier_features, vc.features):
            p.copy_(f.to(p.device))
    dec = _time_decoder(cfg, vc.decoder, w_t)
    got = _fused(octree, dec, fx["coord"].cuda(), fx["sdf_label"].cuda(), weight.cuda(), ts.cuda(),
                 _opts(fx["sigma"], True, to.weight_e_of(fx)))
    _check("dead_points", got, ref)


# ---- 5. with w_t = 0: the check library's lane-per-point step on the same batch
@pytest.mark.parametrize("eik", [False, True])
def test_a_zero_time_column_agrees_with_the_lane_per_point_step(eik):
    from shine_mapping_amd import ops

    name = "kitti_eik_L3"
    c = to.case(name, "wt_zero", eik)
    cfg, octree, dec = _product(name, "wt_zero")
    coord, label, weight, ts = _dev(c)
    got = _fused(octree, dec, coord, label, weight, ts, _opts(c.sigma, eik, c.weight_e))
    _, octree0, plain = product_from_golden(c.fx)
    loss, pred, _ = ops.fused_train_step(octree0, plain, coord, label, weight, _opts(c.sigma, eik, c.weight_e, kernel_variant=1))
    torch.cuda.synchronize()
    ref = dict(loss=loss.cpu(), pred=pred.cpu(), feat_grads=[p.grad.cpu() for p in octree0.hier_features],
               mlp_grads=[p.grad.cpu() for p in plain.fused_params()])
    narrow = (got[0], got[1], [got[2][0][:, :8].contiguous()] + got[2][1:], got[3])
    _check("w_t = 0 vs kernel_variant 1, eik=%d" % eik, narrow, ref)
    assert float(got[2][0][:, 8].abs().max()) > 0.0


# ---- 6. pool mode, both record layouts
@pytest.mark.parametrize("L", [3, 4])
def test_pool_mode_reads_the_records(L):
    from shine_mapping_amd import ops, synth
    from shine_mapping_amd.sampler import SortedPool

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L)
    pl = wl.pool
    dec = _synth_time_decoder(wl.cfg)
    gen = torch.Generator(device="cuda").manual_seed(9)
    ts_all = torch.randint(0, to.FRAMES, (pl.coord.shape[0],), device="cuda", generator=gen)  # int64, as time_pool may hold them
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=3, ts=ts_all)
    assert pool.rec is not None and (pool._weight_sep is None) == (L < 4)
    assert pool.ts.dtype == torch.float32 and pool.ts.is_contiguous() and torch.equal(pool.ts, ts_all[pool.perm.long()].float())
    parts = pool.surf_parts_buffer(1000)
    idx = pool.draw(1000, surf_parts=parts)
    coord, label, weight = pool.get_batch(idx)
    ts = pool.ts[idx.long()].contiguous()
    opts = _opts(wl.cfg.sigma_sigmoid, True, 0.1)
    got = _fused(wl.octree, dec, None, None, None, None, opts, pool=pool, idx=idx)
    with_parts = _fused(wl.octree, dec, None, None, None, None, opts, pool=pool, idx=idx, n_surf=parts)
    plain = _fused(wl.octree, dec, coord, label, weight, ts, opts)
    assert torch.equal(got[0], plain[0]) and torch.equal(with_parts[0], plain[0]), L  # (the same row order: the same bits)
    assert all(torch.equal(a, b) for a, b in zip(got[2], plain[2])) and torch.equal(got[3], plain[3])
    for a, b in zip(got[1], plain[1]):
        assert rel_err(a, b) <= TOL, (L, rel_err(a, b))
    _check("pool L=%d" % L, got, _composite(wl.octree, dec, coord, label, weight, ts, opts))
    bce = _opts(wl.cfg.sigma_sigmoid, False)
    _check("pool L=%d bce" % L, _fused(wl.octree, dec, None, None, None, None, bce, pool=pool, idx=idx),
           _composite(wl.octree, dec, coord, label, weight, ts, bce))
    plain_pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=3)
    assert not hasattr(plain_pool, "ts")
    with pytest.raises(ValueError, match="ts="):
        ops.fused_time_step(wl.octree, dec, None, None, None, None, opts, pool=plain_pool, idx=idx)
    pool.rebuild(pl.coord, pl.sdf_label, pl.weight)  # (a rebuild without ts drops it)
    assert not hasattr(pool, "ts")


# ---- 7. determinism, accumulation, grad_buffers, the frozen decoder, the workspace, the reductions
def test_determinism_accumulation_buffers_frozen_decoder_and_workspace():
    from shine_mapping_amd import _lib, autograd_ops, ops

    name, kind = "maicity_bce_L4", "frames"
    c = to.case(name, kind, True)
    fx, _, w_t = to.inputs(name, kind)
    cfg, octree, _ = product_from_golden(fx)
    dec = _time_decoder(cfg, fx["decoder"], w_t)
    batch = _dev(c)
    opts = _opts(c.sigma, True, c.weight_e)
    a, b = _fused(octree, dec, *batch, opts), _fused(octree, dec, *batch, opts)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and torch.equal(a[3], b[3])
    # a second call doubles the grads; the caller's workspace is all zero afterwards
    _clear(octree, dec)
    ws = _lib.zeroed_workspace(autograd_ops.time_step_workspace_bytes(), "cuda")
    ops.fused_time_step(octree, dec, *batch, opts, workspace=ws)
    ops.fused_time_step(octree, dec, *batch, opts, workspace=ws)
    params = list(octree.hier_features) + list(dec.time_params())
    for k, (p, r) in enumerate(zip(params, a[1] + a[2])):
        assert float((p.grad - 2 * r).abs().max()) <= TOL * float(r.abs().max()) or float(r.abs().max()) == 0.0, k
    assert not bool(ws.any()), "the workspace is all zero after a call"
    with pytest.raises(_lib.ShineHipError, match="shine_time_step: workspace too small"):
        ops.fused_time_step(octree, dec, *batch, opts, workspace=ws[:64])
    # grad_buffers: the same numbers land in the buffers, .grad stays as it is
    kept = [p.grad.clone() for p in params]
    bufs = ([torch.zeros_like(p) for p in octree.hier_features], [torch.zeros_like(p) for p in dec.time_params()])
    ops.fused_time_step(octree, dec, *batch, opts, grad_buffers=bufs)
    assert all(torch.equal(p.grad, k) for p, k in zip(params, kept))
    assert all(torch.equal(x, y) for x, y in zip(bufs[1], a[2]))
    for x, y in zip(bufs[0], a[1]):
        assert rel_err(x, y) <= TOL
    _clear(octree, dec)
    # 'sum' against the oracle; 'mean' over a global count
    oct_, mlp = to.oracle_for(fx, w_t, wide=True)
    ref = to.time_step(oct_, mlp, c.coord, c.label, c.weight, c.ts, c.sigma, eik=True, weight_e=c.weight_e, reduction="sum")
    _check("sum", _fused(octree, dec, *batch, _opts(c.sigma, True, c.weight_e, loss_reduction="sum")), ref)
    n = c.coord.shape[0]
    half = _fused(octree, dec, *batch, _opts(c.sigma, False, n_global=2 * n))
    full = _fused(octree, dec, *batch, _opts(c.sigma, False))
    assert abs(float(half[0]) - 0.5 * float(full[0])) <= 1e-6 * float(full[0])
    # a decoder that is neither trained nor frozen is refused; a frozen one gets no gradient and the same feature grads
    dec.time_params()[2].requires_grad_(False)
    with pytest.raises(ValueError, match="all require grad or all be frozen"):
        ops.fused_time_step(octree, dec, *batch, opts)
    for p in dec.parameters():
        p.requires_grad_(False)
    guard = [p.detach().clone() for p in dec.parameters()]
    frozen = _fused(octree, dec, *batch, opts)
    assert frozen[2] is None and all(p.grad is None for p in dec.parameters())
    assert all(torch.equal(p, g) for p, g in zip(dec.parameters(), guard))
    assert torch.equal(frozen[0], a[0]) and torch.equal(frozen[3], a[3])
    for x, y in zip(frozen[1], a[1]):
        assert rel_err(x, y) <= TOL
    for bad in (dict(out=torch.zeros(2, device="cuda")), dict(n_surf=torch.zeros(1, device="cuda")),
                dict(idx=torch.zeros(4, dtype=torch.int64, device="cuda")), dict(pred_out=torch.zeros(3, device="cuda"))):
        with pytest.raises(ValueError):
            ops.fused_time_step(octree, dec, *batch, opts, **bad)
    with pytest.raises(ValueError, match="ts"):
        ops.fused_time_step(octree, dec, batch[0], batch[1], batch[2], batch[3].double(), opts)
    with pytest.raises(NotImplementedError, match="loss_weight_on"):
        ops.fused_time_step(octree, dec, *batch, _opts(c.sigma, True, loss_weight_on=True))
    _, _, plain = product_from_golden(fx)
    with pytest.raises(NotImplementedError, match="time_fusable"):
        ops.fused_time_step(octree, plain, *batch, opts)


# ---- 8. the loop
ITERS = 12
N = 4096
FRAMES_LOOP = 12


@pytest.fixture(scope="module")
def workload():
    from shine_mapping_amd import synth

    wl = synth.build_workload("maicity", frames=FRAMES_LOOP, beams=32, azimuths=180, device="cuda", seed=7)
    wl.time_decoder = _synth_time_decoder(wl.cfg, seed=5, wt_scale=1.0)  # (frame ids below 12: the column at its init scale)
    gen = torch.Generator(device="cuda").manual_seed(13)
    wl.ts = torch.randint(0, FRAMES_LOOP, (wl.pool.coord.shape[0],), device="cuda", generator=gen).float()
    wl.start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.time_decoder.parameters())]
    return wl


def _loop_parts(wl, seed=11):
    from shine_mapping_amd import autograd_ops
    from shine_mapping_amd.sampler import SortedPool

    params = list(wl.octree.hier_features) + list(wl.time_decoder.parameters())
    with torch.no_grad():
        for p, s in zip(params, wl.start):
            p.copy_(s)
            p.grad = None
            p.requires_grad_(True)
    autograd_ops.bump_param_epoch()
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.ray_loss, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, False, 1.0
    pl = wl.pool
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=seed, canonical=True, ts=wl.ts)
    return cfg, params, pool


def _make_opt(cfg, wl, hip):
    from shine_mapping_amd import optim

    feats = list(wl.octree.parameters())
    if hip:
        return optim.setup_optimizer(cfg, feats, wl.time_decoder.time_params())
    groups = [{"params": wl.time_decoder.time_params(), "lr": cfg.lr, "weight_decay": cfg.weight_decay}]
    groups += [{"params": feats[cfg.tree_level_feat - i - 1], "lr": cfg.lr} for i in range(cfg.tree_level_feat)]
    return torch.optim.Adam(groups, betas=(0.9, 0.99), eps=cfg.adam_eps)


def _graphed(cfg, wl, pool, opt, eik, **kw):
    from shine_mapping_amd.loop import GraphedIteration

    return GraphedIteration(wl.octree, wl.time_decoder, pool, opt, _opts(cfg.sigma_sigmoid, eik, 0.1), N, **kw)


def _replay(cfg, wl, pool, batches, eik, composite):
    """{fused_time_step | the torch composite, torch.optim.Adam} on the recorded draws"""
    from shine_mapping_amd import ops

    opt = _make_opt(cfg, wl, False)
    opts = _opts(cfg.sigma_sigmoid, eik, 0.1)
    losses = []
    for idx in batches:
        coord, label, weight = pool.get_batch(idx)
        ts = pool.ts[idx.long()].contiguous()
        opt.zero_grad(set_to_none=True)
        if composite:
            losses.append(float(_composite_keep(wl.octree, wl.time_decoder, coord, label, weight, ts, opts)))
        else:
            losses.append(float(ops.fused_time_step(wl.octree, wl.time_decoder, coord, label, weight, ts, opts)))
        opt.step()
    torch.cuda.synchronize()
    return losses


def _composite_keep(octree, dec, coord, label, weight, ts, opts):
    """_composite's forward and backward, leaving the grads in place for the optimiser"""
    from shine_mapping_amd import get_gradient, sdf_bce_loss

    eik = bool(opts.ekional_loss_on)
    x = coord.detach().clone().requires_grad_(eik)
    pred = dec._time_composite(octree.query_feature(x), ts)
    loss = sdf_bce_loss(pred, label, opts.sigma, None, False, opts.loss_reduction)
    if eik:
        g = get_gradient(x, pred) * opts.sigma
        loss = loss + opts.weight_e * ((1.0 - g[weight > 0].norm(2, dim=-1)) ** 2).mean()
    loss.backward()
    return loss.detach()


@pytest.mark.parametrize("eik", [False, True])
def test_graphed_time_loop_matches_an_eager_replay_and_the_composite(workload, eik):
    wl = workload
    cfg, params, pool = _loop_parts(wl)
    g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True), eik)
    # the constructor ran iteration 1 eagerly: {draw, the one-launch step, the optimiser's graph-safe step}
    assert g.time and g.ran_eager and not g.native and not g.fold and g.touched is None
    batches, hip_loss = [g._idx.clone()], [g.loss.clone()]
    for it in range(ITERS - 1):
        with counted_launches() as calls, time_calls() as steps:
            loss = g()
        names = [c[0] for c in calls]
        if it == 0:  # this object's first call captures the iteration
            assert names == ["shine_sample_sorted_dev", "shine_adam_step_dev"] and len(steps) == 1, (names, len(steps))
            assert steps[0][3] == 8 and steps[0][10] == (64 if eik else 0)  # (pool records; the draw's partial surface counts)
        else:
            assert names == [] and steps == []  # (a replay goes through no entry point)
        batches.append(g._idx.clone())  # (the time route draws inside the iteration: _idx is the batch that just ran)
        hip_loss.append(loss.clone())
    torch.cuda.synchronize()
    hip_loss = [float(x) for x in hip_loss]
    hip_params = [p.detach().clone() for p in params]
    assert all(x == x and abs(x) != float("inf") for x in hip_loss), hip_loss
    for composite in (False, True):
        cfg, params, _ = _loop_parts(wl)
        ref_loss = _replay(cfg, wl, pool, batches, eik, composite)
        worst = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(hip_loss, ref_loss))
        errs = [rel_err(a, b) for a, b in zip(hip_params, params)]
        print("losses", hip_loss[0], hip_loss[-1], ref_loss[0], ref_loss[-1])
        print("eik=%d vs %s: worst loss %.2e" % (eik, "composite + Adam" if composite else "eager replay", worst),
              "params", " ".join("%.1e" % e for e in errs))
        assert worst <= LOOP_TOL["loss"], worst
        assert max(errs) <= LOOP_TOL["params"], errs
    _loop_parts(wl)


def test_unrolled_run_equals_single_calls(workload):
    wl = workload
    K = 5
    out = []
    for unroll in (1, 2):
        cfg, params, pool = _loop_parts(wl)
        g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True), True, unroll=unroll)
        if unroll == 1:
            for _ in range(K):
                g()
        else:
            assert float(g.run(K)) == float(g.loss)  # 2 x 2 + 1
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for p in params], g._idx.clone(), float(g.loss)))
    assert torch.equal(out[0][1], out[1][1])  # (the same batches were drawn)
    errs = [rel_err(a, b) for a, b in zip(out[1][0], out[0][0])]
    print("unrolled vs single:", " ".join("%.1e" % e for e in errs), out[0][2], out[1][2])
    assert max(errs) <= TOL, errs
    assert abs(out[0][2] - out[1][2]) <= TOL * abs(out[0][2])
    _loop_parts(wl)


def test_with_a_plain_decoder_the_iteration_is_still_the_two_launch_native_graph(workload):
    from shine_mapping_amd import optim
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.sampler import SortedPool

    wl = workload
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters())]
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, 1.0
    opt = optim.setup_optimizer(cfg, list(wl.octree.parameters()), wl.decoder.fused_params())
    pool = SortedPool(wl.octree, wl.pool.coord, wl.pool.sdf_label, wl.pool.weight, seed=5, ts=wl.ts)  # (ts changes nothing)
    g = GraphedIteration(wl.octree, wl.decoder, pool, opt, _opts(cfg.sigma_sigmoid, False), N)
    assert not g.time and g.native and not g.ran_eager
    with counted_launches() as calls, time_calls() as steps:
        g()
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["shine_iter_graph_set_step", "shine_iter_graph_set_finish"] and steps == []
    assert g.graph is None and g.graph_k is None
    with torch.no_grad():
        for p, s in zip(list(wl.octree.hier_features) + list(wl.decoder.parameters()), start):
            p.copy_(s)
            p.grad = None


# ---- 9. the dataset's pool
def test_dataset_pool_carries_the_time_stamps_and_trains(tmp_path):
    from shine_mapping_amd import Decoder, FeatureOctree, optim, synth
    from shine_mapping_amd.dataset import LiDARDataset
    from shine_mapping_amd.loop import GraphedIteration

    base = synth.make_config("ncd", device="cuda")
    drive = synth.write_kitti_drive(str(tmp_path), base, frames=3, beams=16, azimuths=90, device="cpu")
    cfg = synth.dataset_config("ncd", drive, pc_radius=20.0, min_range=2.5, bs=N, time_conditioned=True)
    torch.manual_seed(1)
    octree = FeatureOctree(cfg)
    ds = LiDARDataset(cfg, octree)
    for f in range(3):
        ds.process_frame(f)
    sp = ds.sorted_pool()
    assert sp.ts.dtype == torch.float32 and sp.ts.shape == (sp.size,)
    assert torch.equal(sp.ts, ds.time_pool[sp.perm.long()].float().reshape(-1))
    assert sorted(set(sp.ts.tolist())) == [0.0, 1.0, 2.0]
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, 1.0
    torch.manual_seed(3)
    geo = Decoder(cfg, is_time_conditioned=True)
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), geo.time_params())
    g = GraphedIteration(octree, geo, sp, opt, _opts(cfg.sigma_sigmoid, True, 0.1), N)
    seen = [g.loss.clone()]
    for _ in range(19):
        g()
        seen.append(g.loss.clone())
    seen = [float(x) for x in seen]
    print("loss over 20 iterations: %.4f -> %.4f" % (seen[0], seen[-1]))
    assert all(x == x and abs(x) != float("inf") for x in seen) and seen[-1] < seen[0]
