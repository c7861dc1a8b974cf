"""The ray-rendering training step on the device (csrc/shine_ray_step.hip, ops.fused_ray_step, sampler.RayPool,
GraphedIteration's ray route) against the fp64 oracle of tests/ray_step_oracle.py and the torch composite.

The tolerance is the project's contract, TOL of tests/test_gpu_parity.py through normal_step_oracle.rel_errors, with d loss /
d sigma_size as one more one-element tensor in the decoder list; pred <= TOL of max(1, max |pred|), dpred <= TOL of its max-abs.
tests/test_ray_step.py shows on the CPU that the fp32 torch evaluation sits within TOL / 4 on every case.
"""
import copy
import functools

import pytest
import torch

import ray_step_oracle as ro
from conftest import product_from_golden
from test_gpu_parity import TOL
from test_gpu_sem_step import LOOP_TOL, counted_launches, rel_err

pytestmark = pytest.mark.gpu


def _clear(octree, dec, ss=None):
    for p in list(octree.hier_features) + list(dec.parameters()) + ([ss] if ss is not None else []):
        p.grad = None


def _opts(sigma, eik, weight_e=0.1):
    from shine_mapping_amd import StepOptions

    return StepOptions(sigma=float(sigma), ekional_loss_on=bool(eik), weight_e=float(weight_e))


def _sigma(v, train=True):
    return torch.full((1,), float(v), device="cuda").requires_grad_(train)


def _fused(octree, dec, coord, weight, depth, ray_depth, ss, opts, S, neus, **kw):
    """-> (loss, feature grads, decoder grads + [sigma grad] | None, pred, dpred)"""
    from shine_mapping_amd import ops

    _clear(octree, dec, ss)
    n = kw["idx"].numel() if kw.get("idx") is not None else ray_depth.numel()
    rows = n * (kw["pool"].samples if kw.get("pool") is not None else S)
    pred = torch.full((rows,), float("nan"), device="cuda")
    dpred = torch.full((rows,), float("nan"), device="cuda")
    loss = ops.fused_ray_step(octree, dec, coord, weight, depth, ray_depth, ss, opts, S, neus_on=neus, pred_out=pred,
                              dpred_out=dpred, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.grad_fn is None
    mlp = dec.fused_params()
    sg = [ss.grad.clone() if ss.grad is not None else torch.zeros(1, device="cuda")]
    out = (loss.clone(), [p.grad.clone() for p in octree.hier_features],
           None if mlp[0].grad is None else [p.grad.clone() for p in mlp] + sg, pred, dpred)
    if out[2] is None:
        out = out[:2] + (None,) + out[3:] + (sg[0],)
    _clear(octree, dec, ss)
    return out


def _check(what, got, ref, tol=TOL):
    loss_err, errs = ro.rel_errors(got[0], got[1], got[2], ref)
    pr, dp = ref["pred"].double().cpu(), ref["dpred"].double().cpu()
    pred_err = float((got[3].double().cpu() - pr).abs().max()) / max(1.0, float(pr.abs().max())) if pr.numel() else 0.0
    top = float(dp.abs().max()) if dp.numel() else 0.0
    dpred_err = float((got[4].double().cpu() - dp).abs().max()) / (top if top > 0 else 1.0) if dp.numel() else 0.0
    print(what, "loss %.1e pred %.1e dpred %.1e" % (loss_err, pred_err, dpred_err), " ".join("%.1e" % e for e in errs))
    assert all(bool(torch.isfinite(t).all()) for t in [got[0], got[3], got[4]] + got[1] + got[2]), what
    assert loss_err <= tol and pred_err <= tol and dpred_err <= tol and max(errs) <= tol, (what, loss_err, pred_err, dpred_err, errs)


@functools.lru_cache(maxsize=None)
def _product(name, scale=1.0):
    fx = ro.load_golden(name)
    cfg, octree, dec = product_from_golden(fx)
    if scale != 1.0:
        with torch.no_grad():
            dec.fused_params()[4].mul_(scale)
            dec.fused_params()[5].mul_(scale)
    return cfg, octree, dec


def _dev(c):
    return c.coord.cuda(), c.weight.cuda(), c.depth.cuda(), c.ray_depth.cuda()


# ---- 1. one step on every case against the wide oracle
@pytest.mark.parametrize("name,neus,eik,S", ro.CASES, ids=[ro.case_id(*c) for c in ro.CASES])
def test_one_step_matches_the_fp64_oracle(name, neus, eik, S):
    c = ro.case(name, neus, eik, S)
    _, octree, dec = _product(name, c.out_scale)
    got = _fused(octree, dec, *_dev(c), _sigma(c.sigma_size), _opts(c.sigma, eik, c.weight_e), S, neus)
    _check(ro.case_id(name, neus, eik, S), got, c.wide)
    assert float(got[2][6].abs().max()) > 0.0


# ---- 2. tile edges: plain, through a reversed index, through an index with repeated rays
def _sub_ref(c, rays, S, neus, eik):
    """the wide oracle on the rays `rays` (a list of ray numbers, repeats allowed) of a case's fixture"""
    rows = (torch.tensor(rays).view(-1, 1) * S + torch.arange(S).view(1, -1)).reshape(-1)
    oct_, mlp = ro.oracle_for(c.fx, wide=True, scale=c.out_scale)
    return ro.ray_step(oct_, mlp, c.coord[rows], c.weight[rows], c.depth[rows], c.ray_depth[torch.tensor(rays)], c.sigma_size,
                       c.sigma, S, neus=neus, eik=eik, weight_e=c.weight_e)


def _rays_of(name, S, neus, stride=None):
    """a case-like view of a fixture at any S (the oracle's depths are drawn per (fixture, S)).  `stride`: ray i takes the fixture's
    rows i * stride .. i * stride + S - 1 — overlapping rays, for more rays than the fixture has rows / S"""
    from types import SimpleNamespace

    fx, coord, weight, depth, ray_depth = ro.inputs(name, S)
    if stride is not None:
        m = (fx["coord"].shape[0] - S) // stride + 1
        rows = (torch.arange(m).view(-1, 1) * stride + torch.arange(S).view(1, -1)).reshape(-1)
        coord, weight = fx["coord"][rows].contiguous(), fx["weight"][rows].contiguous()
        depth, ray_depth = ro.draw_depths(m, S, ro.to._seed("ray", name, S, stride))
    return SimpleNamespace(fx=fx, coord=coord, weight=weight, depth=depth, ray_depth=ray_depth, out_scale=ro.out_scale(name, neus),
                           sigma_size=1.0, sigma=fx["sigma"], weight_e=ro.weight_e_of(fx))


def _edge(name, S, n, neus, eik=True, stride=None):
    c = _rays_of(name, S, neus, stride)
    assert c.ray_depth.numel() >= n
    _, octree, dec = _product(name, c.out_scale)
    coord, weight, depth, ray_depth = _dev(c)
    opts = _opts(c.sigma, eik, c.weight_e)
    ss = _sigma(c.sigma_size)
    ref = _sub_ref(c, list(range(n)), S, neus, eik)
    plain = _fused(octree, dec, coord[:n * S].contiguous(), weight[:n * S].contiguous(), depth[:n * S].contiguous(),
                   ray_depth[:n].contiguous(), ss, opts, S, neus)
    _check("S=%d n=%d" % (S, n), plain, ref)
    idx = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")
    got = _fused(octree, dec, coord, weight, depth, ray_depth, ss, opts, S, neus, idx=idx)
    flip = lambda t: t.view(n, S).flip(0).reshape(-1)  # (pred is written at the batch position)
    _check("S=%d n=%d reversed" % (S, n), got[:3] + (flip(got[3]), flip(got[4])), ref)
    rep = [(3 * i) % max(n // 2, 1) for i in range(n)]
    got = _fused(octree, dec, coord, weight, depth, ray_depth, ss, opts, S, neus,
                 idx=torch.tensor(rep, dtype=torch.int32, device="cuda"))
    _check("S=%d n=%d repeated" % (S, n), got, _sub_ref(c, rep, S, neus, eik))
    return plain


@pytest.mark.parametrize("n", [1, 9, 10, 11, 40, 41, 641])
def test_tile_edges_at_six_samples(n):
    # (a fixture holds 341 rays of 6: the 641 rays are overlapping windows of its rows: 65 tiles, 17 workgroups, both ticket levels)
    _edge("kitti_eik_L3", 6, n, neus=(n % 2 == 0), stride=3 if n > 341 else None)


# the grid sum's boundaries at six samples (10 rays per tile, 40 per workgroup): 641 rays are 17 workgroups — a full first-level run
# and a run of one behind it, checked against the oracle above — and 10241 rays are 257, every workgroup plus a grid-stride pass.
# The loss, the weight grads, the sigma_size grad, pred and dpred are the same bits from call to call at both sizes.  The fp64
# oracle takes most of a minute on the 61446 rows of the larger one, so that size checks the deterministic outputs call to call only.
@pytest.mark.parametrize("n", [641, 10241])
def test_grid_sum_boundary_ray_counts_repeat_bit_identically(n):
    c = _rays_of("kitti_eik_L3", 6, False)
    _, octree, dec = _product("kitti_eik_L3", c.out_scale)
    coord, weight, depth, ray_depth = _dev(c)
    idx = (torch.arange(n) % c.ray_depth.numel()).to(torch.int32).cuda()
    opts, ss = _opts(c.sigma, True, c.weight_e), _sigma(c.sigma_size)
    a = _fused(octree, dec, coord, weight, depth, ray_depth, ss, opts, 6, False, idx=idx)
    b = _fused(octree, dec, coord, weight, depth, ray_depth, ss, opts, 6, False, idx=idx)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2])), n
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]), n
    assert all(bool(torch.isfinite(t).all()) for t in [a[0], a[3], a[4]] + a[1] + a[2]) and float(a[0]) > 0.0
    assert float(a[2][6].abs().max()) > 0.0


@pytest.mark.parametrize("S", [1, 2, 7, 8, 9, 16, 17, 32])
def test_tile_edges_at_every_sample_count(S):
    for n in (1, 64 // S, 64 // S + 1):
        _edge("kitti_eik_L3", S, n, neus=False)
        got = _edge("maicity_bce_L3", S, n, neus=True)
        if S == 1:  # dr_neus without an alpha column: the loss is mean |ray_depth|, nothing receives a gradient (no eikonal part here)
            c = _rays_of("maicity_bce_L3", 1, True)
            _, octree, dec = _product("maicity_bce_L3", c.out_scale)
            coord, weight, depth, ray_depth = _dev(c)
            g = _fused(octree, dec, coord[:n].contiguous(), weight[:n].contiguous(), depth[:n].contiguous(),
                       ray_depth[:n].contiguous(), _sigma(1.0), _opts(c.sigma, False), 1, True)
            assert abs(float(g[0]) - float(c.ray_depth[:n].abs().mean())) <= 1e-6
            assert all(float(t.abs().max()) == 0.0 for t in g[1] + g[2] + [g[4]])


def test_more_than_32_samples_is_refused_and_an_empty_batch_writes_zero():
    from shine_mapping_amd import ops

    c = _rays_of("kitti_eik_L3", 6, False)
    _, octree, dec = _product("kitti_eik_L3", 1.0)
    coord, weight, depth, ray_depth = _dev(c)
    ss = _sigma(1.0)
    with pytest.raises(ValueError, match="SHINE_RAY_MAX_SAMPLES"):
        ops.fused_ray_step(octree, dec, coord[:33], weight[:33], depth[:33], ray_depth[:1], ss, _opts(c.sigma, True), 33)
    _clear(octree, dec, ss)
    out = torch.full((1,), 7.0, device="cuda")
    loss = ops.fused_ray_step(octree, dec, coord[:0], weight[:0], depth[:0], ray_depth[:0], ss, _opts(c.sigma, True), 6, out=out)
    assert float(loss) == 0.0 and float(out[0]) == 0.0
    assert all(float(p.grad.abs().max()) == 0.0 for p in list(octree.hier_features) + dec.fused_params() + [ss])
    _clear(octree, dec, ss)


# ---- 3. every instantiation against the torch composite on the device
def _composite(octree, dec, coord, weight, depth, ray_depth, ss, opts, S, neus, keep=False):
    from shine_mapping_amd import get_gradient
    from shine_mapping_amd.losses import batch_ray_rendering_loss_composite

    if not keep:
        _clear(octree, dec, ss)
    eik = bool(opts.ekional_loss_on)
    x = coord.detach().clone().requires_grad_(eik)
    pred = dec.sdf(octree.query_feature(x))
    m = ray_depth.numel()
    render = batch_ray_rendering_loss_composite(depth.view(m, S), torch.sigmoid(pred / ss).view(m, S), ray_depth, neus)
    dpred = torch.autograd.grad(render, pred, retain_graph=True, allow_unused=True)[0]
    loss = render
    if eik:
        g = get_gradient(x, pred) * opts.sigma
        surf = weight > 0
        if bool(surf.any()):
            loss = loss + opts.weight_e * ((1.0 - g[surf].norm(2, dim=-1)) ** 2).mean()
    loss.backward()
    if keep:
        return loss.detach()
    out = dict(loss=loss.detach().cpu(), pred=pred.detach().cpu(), dpred=(torch.zeros_like(pred) if dpred is None else dpred).cpu(),
               feat_grads=[p.grad.detach().cpu().clone() for p in octree.hier_features],
               mlp_grads=[(torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().clone()
                          for p in dec.fused_params() + [ss]])
    _clear(octree, dec, ss)
    return out


def _synth_rays(wl, m, S, seed, span=0.3):
    """m rays of S pool samples (a ray's samples are consecutive pool rows) with seeded depths; rows 3..6 are moved outside the
    mapped box (they miss every level) as surface rows"""
    from shine_mapping_amd import synth

    gen = torch.Generator(device="cuda").manual_seed(seed)
    coord, _, weight = synth.draw_batch(wl.pool, m * S, gen)
    coord, weight = coord.clone(), weight.clone()
    cell = wl.cfg.leaf_vox_size * wl.cfg.scale
    coord[3:7] = (wl.pool.coord.max(0).values + 3.0 * cell).clamp(max=0.999)
    weight[3:7] = 1.0
    depth = torch.rand(m * S, device="cuda", generator=gen) * 2.0 + 0.1
    ray_depth = torch.rand(m, device="cuda", generator=gen) * 2.0 + 0.1
    return coord.contiguous(), weight.contiguous(), depth, ray_depth


@pytest.mark.parametrize("eik", [False, True])
@pytest.mark.parametrize("poly", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_every_instantiation_matches_the_composite(L, poly, eik):
    from shine_mapping_amd import Decoder, synth

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L,
                              poly_int_on=poly)
    assert wl.octree.featured_level_num == L and bool(wl.octree.step_config().poly_int_on) == poly
    torch.manual_seed(3)
    dec = Decoder(wl.cfg)
    batch = _synth_rays(wl, 11, 6, 5)
    opts = _opts(wl.cfg.sigma_sigmoid, eik, 0.1)
    for neus in (False, True):
        ss = _sigma(1.0)
        ref = _composite(wl.octree, dec, *batch, ss, opts, 6, neus)
        assert bool(torch.isfinite(ref["loss"])) and float(ref["feat_grads"][-1].abs().max()) > 0
        _check("L=%d poly=%d eik=%d neus=%d" % (L, poly, eik, neus), _fused(wl.octree, dec, *batch, ss, opts, 6, neus), ref)


# ---- 4. saturated rays: every output finite, dpred is the Tier A kernel's dy on the step's own pred
@pytest.mark.parametrize("neus", [False, True])
def test_saturated_rays_are_finite_and_dpred_is_the_tier_a_gradient(neus):
    from shine_mapping_amd import _lib
    from shine_mapping_amd.losses import loss_workspace

    c = _rays_of("kitti_eik_L3", 6, False)
    _, octree, dec = _product("kitti_eik_L3", 1.0)
    coord, weight, depth, ray_depth = _dev(c)
    ssv = 0.05
    got = _fused(octree, dec, coord, weight, depth, ray_depth, _sigma(ssv), _opts(c.sigma, True, c.weight_e), 6, neus)
    assert all(bool(torch.isfinite(t).all()) for t in [got[0], got[3], got[4]] + got[1] + got[2])
    m = ray_depth.numel()
    y = torch.sigmoid(got[3] / ssv)
    assert int(((y == 0) | (y == 1)).sum()) > 0, "the case holds saturated samples"
    # the kernel's own y = 1 / (1 + exp(-pred / sigma_size)), the step's arithmetic, for a bit-level comparison
    z = got[3] / torch.full((1,), ssv, device="cuda")
    yk = 1.0 / (1.0 + torch.exp(-z))
    dy = torch.empty_like(yk)
    loss = torch.empty(1, device="cuda")
    ws = loss_workspace(yk.device)
    _lib.check(_lib.lib().shine_ray_render_loss(depth.data_ptr(), yk.data_ptr(), ray_depth.data_ptr(), m, 6, 1 if neus else 0,
                                                loss.data_ptr(), dy.data_ptr(), ws.data_ptr(), _lib.current_stream_handle()),
               "shine_ray_render_loss")
    want = dy * ((1.0 - yk) * yk) / ssv
    top = float(want.abs().max())
    err = float((got[4] - want).abs().max())
    print("saturated neus=%d: max |dpred| %.3e, max difference %.3e" % (neus, top, err))
    # one rounding of exp / the quotient apart at most: fp32 epsilon times the handful of operations between y and dpred
    assert top > 0 and err <= 16 * 1.2e-7 * top, (err, top)


# ---- 5. the eikonal term's edge cases
def test_eikonal_edge_cases_and_surface_count_forms():
    name = "maicity_bce_L3"
    c = _rays_of(name, 6, False)
    _, octree, dec = _product(name, 1.0)
    coord, weight, depth, ray_depth = _dev(c)
    opts = _opts(c.sigma, True, c.weight_e)
    ss = _sigma(1.0)
    m = ray_depth.numel()
    rays = list(range(m))

    def ref_with(w):
        cc = copy.copy(c)
        cc.weight = w
        return _sub_ref(cc, rays, 6, False, True)

    # no surface sample: the eikonal part is 0 and sends nothing — the plain step's numbers
    free = -c.weight.abs() - 1.0
    ref = ref_with(free)
    assert float(ref["loss"]) == float(_sub_ref(c, rays, 6, False, False)["loss"])
    _check("no surface", _fused(octree, dec, coord, free.cuda(), depth, ray_depth, ss, opts, 6, False), ref)
    # rays whose weights are all <= 0 beside rays with mixed signs
    mixed = c.weight.clone().view(m, 6)
    mixed[::3] = -1.0
    mixed[1::3, ::2] = 1.0
    mixed = mixed.reshape(-1)
    _check("mixed", _fused(octree, dec, coord, mixed.cuda(), depth, ray_depth, ss, opts, 6, False), ref_with(mixed))
    # the surface count as one count and as partial counts: the same bits
    ns = int((c.weight > 0).sum())
    parts = torch.zeros(64, dtype=torch.int64, device="cuda")
    parts[0], parts[5], parts[63] = ns - 7, 4, 3
    one = torch.tensor([ns], dtype=torch.int64, device="cuda")
    a = _fused(octree, dec, coord, weight, depth, ray_depth, ss, opts, 6, False, n_surf=parts)
    b = _fused(octree, dec, coord, weight, depth, ray_depth, ss, opts, 6, False, n_surf=one)
    d = _fused(octree, dec, coord, weight, depth, ray_depth, ss, opts, 6, False)
    assert torch.equal(a[0], b[0]) and torch.equal(b[0], d[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    # rows with g exactly zero: surface rows outside the mapped box miss every level — they contribute 1 and get no gradient
    out = coord.clone()
    out[6:12] = 0.9990
    wz = c.weight.clone()
    wz[6:12] = 1.0
    cc = copy.copy(c)
    cc.coord, cc.weight = out.cpu(), wz
    ref = _sub_ref(cc, rays, 6, False, True)
    _check("zero g", _fused(octree, dec, out, wz.cuda(), depth, ray_depth, ss, opts, 6, False), ref)


# ---- 6. determinism, accumulation, decoder states, the workspace
def test_determinism_decoder_states_buffers_and_workspace():
    from shine_mapping_amd import _lib, autograd_ops, ops

    name = "maicity_bce_L4"
    c = ro.case(name, False, True, 6)
    fx = c.fx
    cfg, octree, dec = product_from_golden(fx)
    batch = _dev(c)
    opts = _opts(c.sigma, True, c.weight_e)
    ss = _sigma(1.0)
    a, b = _fused(octree, dec, *batch, ss, opts, 6, False), _fused(octree, dec, *batch, ss, opts, 6, False)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    # a second call doubles the grads; the caller's workspace is all zero afterwards
    _clear(octree, dec, ss)
    ws = _lib.zeroed_workspace(autograd_ops.ray_step_workspace_bytes(), "cuda")
    ops.fused_ray_step(octree, dec, *batch, ss, opts, 6, workspace=ws)
    ops.fused_ray_step(octree, dec, *batch, ss, opts, 6, workspace=ws)
    params = list(octree.hier_features) + list(dec.fused_params()) + [ss]
    for k, (p, r) in enumerate(zip(params, a[1] + a[2])):
        assert float((p.grad - 2 * r).abs().max()) <= TOL * float(r.abs().max()) or float(r.abs().max()) == 0.0, k
    assert not bool(ws.any()), "the workspace is all zero after a call"
    with pytest.raises(_lib.ShineHipError, match="shine_ray_step: workspace too small"):
        ops.fused_ray_step(octree, dec, *batch, ss, opts, 6, workspace=ws[:64])
    with pytest.raises(_lib.ShineHipError, match="shine_ray_step: workspace"):
        ops.fused_ray_step(octree, dec, *batch, ss, opts, 6, workspace=ws.view(torch.uint8)[16:])
    # grad_buffers / sigma_grad: the same numbers land in the buffers, .grad stays as it is
    kept = [p.grad.clone() for p in params]
    bufs = ([torch.zeros_like(p) for p in octree.hier_features], [torch.zeros_like(p) for p in dec.fused_params()])
    sgrad = torch.zeros(1, device="cuda")
    ops.fused_ray_step(octree, dec, *batch, ss, opts, 6, grad_buffers=bufs, sigma_grad=sgrad)
    assert all(torch.equal(p.grad, k) for p, k in zip(params, kept))
    assert all(torch.equal(x, y) for x, y in zip(bufs[1] + [sgrad], a[2]))
    for x, y in zip(bufs[0], a[1]):
        assert rel_err(x, y) <= TOL
    _clear(octree, dec, ss)
    # a frozen sigma_size gets no gradient, everything else keeps its bits
    fs = _sigma(1.0, train=False)
    f = _fused(octree, dec, *batch, fs, opts, 6, False)
    assert fs.grad is None and torch.equal(f[0], a[0]) and all(torch.equal(x, y) for x, y in zip(f[2][:6], a[2][:6]))
    # a decoder that is neither trained nor frozen is refused; a frozen one gets no gradient and the same feature grads
    dec.fused_params()[2].requires_grad_(False)
    with pytest.raises(ValueError, match="all require grad or all be frozen"):
        ops.fused_ray_step(octree, dec, *batch, ss, opts, 6)
    for p in dec.parameters():
        p.requires_grad_(False)
    frozen = _fused(octree, dec, *batch, ss, opts, 6, False)
    assert frozen[2] is None and all(p.grad is None for p in dec.parameters())
    assert torch.equal(frozen[0], a[0]) and torch.equal(frozen[3], a[3]) and torch.equal(frozen[5], a[2][6])
    for x, y in zip(frozen[1], a[1]):
        assert rel_err(x, y) <= TOL
    for bad in (dict(out=torch.zeros(2, device="cuda")), dict(n_surf=torch.zeros(1, device="cuda")),
                dict(idx=torch.zeros(4, dtype=torch.int64, device="cuda")), dict(pred_out=torch.zeros(3, device="cuda")),
                dict(dpred_out=torch.zeros(3, device="cuda")), dict(sigma_grad=torch.zeros(2, device="cuda"))):
        with pytest.raises(ValueError):
            ops.fused_ray_step(octree, dec, *batch, ss, opts, 6, **bad)


def test_refusals_leave_the_outputs_untouched():
    from shine_mapping_amd import _lib, ops

    c = ro.case("kitti_eik_L3", False, True, 6)
    _, octree, dec = _product("kitti_eik_L3", 1.0)
    batch = _dev(c)
    ss = _sigma(1.0)
    _clear(octree, dec, ss)
    m = c.ray_depth.numel()
    out = torch.full((1,), 7.0, device="cuda")
    pred = torch.full((m * 6,), 3.0, device="cuda")
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.ShineHipError, match="shine_ray_step: workspace too small"):
        ops.fused_ray_step(octree, dec, *batch, ss, _opts(c.sigma, True), 6, out=out, pred_out=pred, dpred_out=pred.clone(),
                           workspace=small)
    torch.cuda.synchronize()
    assert float(out[0]) == 7.0 and bool((pred == 3.0).all()) and not bool(small.any())
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in list(octree.hier_features) + dec.fused_params() + [ss])
    _clear(octree, dec, ss)


# ---- 7. RayPool
def _ray_pool(wl, m, S, seed=11, signs=False):
    from shine_mapping_amd.sampler import RayPool

    coord, weight, depth, ray_depth = _synth_rays(wl, m, S, 21)
    if signs:
        gen = torch.Generator(device="cuda").manual_seed(2)
        weight = torch.where(torch.rand(m * S, device="cuda", generator=gen) < 0.4, weight.abs() + 0.1, -weight.abs() - 0.1)
        weight.view(m, S)[::5] = -1.0
    return RayPool(wl.octree, coord, weight, depth, ray_depth, samples=S, seed=seed), (coord, weight, depth, ray_depth)


@pytest.fixture(scope="module")
def workload():
    from shine_mapping_amd import Decoder, synth

    wl = synth.build_workload("maicity", frames=12, beams=32, azimuths=180, device="cuda", seed=7)
    torch.manual_seed(5)
    wl.ray_decoder = Decoder(wl.cfg)
    wl.start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.ray_decoder.parameters())]
    return wl


def test_ray_pool_keeps_the_rays_and_draws_sorted_uniform_reproducible(workload):
    wl = workload
    m, S = 3008, 6  # (47 x 64: the histogram's bins hold the same number of rays)
    pool, (coord, weight, depth, ray_depth) = _ray_pool(wl, m, S, signs=True)
    p = pool.perm.long()
    assert sorted(p.tolist()) == list(range(m))
    assert torch.equal(pool.coord.view(m, S, 3), coord.view(m, S, 3)[p]) and torch.equal(pool.ray_depth, ray_depth[p])
    assert torch.equal(pool.sample_depth.view(m, S), depth.view(m, S)[p]) and torch.equal(pool.weight.view(m, S), weight.view(m, S)[p])
    assert torch.equal(pool.surf_per_ray.long(), (pool.weight.view(m, S) > 0).sum(1))
    n = 4096
    surf = pool.surf_buffer()
    idx = pool.draw(n, surf_out=surf)
    i = idx.long()
    assert idx.dtype == torch.int32 and bool((i[1:] >= i[:-1]).all()) and int(i.min()) >= 0 and int(i.max()) < m
    assert int(surf[0]) == int((pool.weight.view(m, S)[i] > 0).sum())
    c, sd, rd, w = pool.get_batch(idx)
    assert torch.equal(rd, pool.ray_depth[i]) and torch.equal(c.view(n, S, 3), pool.coord.view(m, S, 3)[i]) and w.shape == (n * S,)
    # uniform: tests/test_gpu_parity.py::test_sorted_sampler_is_sorted_uniform_and_reproducible's 64-bin chi-square
    draws = [idx] + [pool.draw(n) for _ in range(2)]
    for d in draws:
        hist = torch.bincount((d.long() * 64) // m, minlength=64).double()
        chi2 = float(((hist - n / 64) ** 2 / (n / 64)).sum())
        assert chi2 < 130.0, chi2  # 63 dof: mean 63, sd ~11
    assert not torch.equal(draws[1], draws[2])
    again, _ = _ray_pool(wl, m, S, signs=True)
    assert torch.equal(again.perm, pool.perm) and torch.equal(again.draw(n), idx)  # reproducible per seed, the rays' order too
    other, _ = _ray_pool(wl, m, S, seed=12, signs=True)
    assert not torch.equal(other.draw(n), idx)
    # a captured draw yields fresh indices on each replay
    out, s2 = torch.empty(256, dtype=torch.int32, device="cuda"), pool.surf_buffer()
    pool.draw(256, out=out, graph_safe=True, surf_out=s2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pool.draw(256, out=out, graph_safe=True, surf_out=s2)
    seen = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        seen.append(out.clone())
        assert int(s2[0]) == int(pool.surf_per_ray[out.long()].sum())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_pool_mode_equals_array_mode(workload):
    wl = workload
    pool, _ = _ray_pool(wl, 500, 9)
    dec = wl.ray_decoder
    surf = pool.surf_buffer()
    idx = pool.draw(100, surf_out=surf)
    coord, sd, rd, w = pool.get_batch(idx)
    opts = _opts(wl.cfg.sigma_sigmoid, True, 0.1)
    ss = _sigma(1.0)
    a = _fused(wl.octree, dec, None, None, None, None, ss, opts, None, True, pool=pool, idx=idx, n_surf=surf)
    b = _fused(wl.octree, dec, coord.contiguous(), w.contiguous(), sd.contiguous(), rd.contiguous(), ss, opts, 9, True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2])) and torch.equal(a[4], b[4])
    _check("pool", a, _composite(wl.octree, dec, coord.contiguous(), w.contiguous(), sd.contiguous(), rd.contiguous(), ss, opts, 9,
                                 True))


# ---- 8. the loop
ITERS = 12
N = 64
S_LOOP = 6


def _loop_parts(wl, seed=11):
    from shine_mapping_amd import autograd_ops

    params = list(wl.octree.hier_features) + list(wl.ray_decoder.parameters())
    with torch.no_grad():
        for p, s in zip(params, wl.start):
            p.copy_(s)
            p.grad = None
            p.requires_grad_(True)
    autograd_ops.bump_param_epoch()
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.ray_loss, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, True, 1.0
    pool, _ = _ray_pool(wl, 2000, S_LOOP, seed=seed)
    ss = torch.nn.Parameter(torch.ones(1, device="cuda"))
    return cfg, params + [ss], pool, ss


def _make_opt(cfg, wl, ss, hip):
    from shine_mapping_amd import optim

    feats = list(wl.octree.parameters())
    if hip:
        return optim.setup_optimizer(cfg, feats, wl.ray_decoder.fused_params(), None, ss)
    groups = [{"params": wl.ray_decoder.fused_params(), "lr": cfg.lr, "weight_decay": cfg.weight_decay}]
    groups += [{"params": feats[cfg.tree_level_feat - i - 1], "lr": cfg.lr} for i in range(cfg.tree_level_feat)]
    groups += [{"params": [ss], "lr": cfg.lr}]
    return torch.optim.Adam(groups, betas=(0.9, 0.99), eps=cfg.adam_eps)


def _graphed(cfg, wl, pool, opt, ss, eik, neus, **kw):
    from shine_mapping_amd.loop import GraphedIteration, RayTerm

    return GraphedIteration(wl.octree, wl.ray_decoder, pool, opt, _opts(cfg.sigma_sigmoid, eik, 0.1), N,
                            ray=RayTerm(ss, neus_on=neus), **kw)


def _replay(cfg, wl, pool, ss, batches, eik, neus, composite):
    """{fused_ray_step | the torch composite, torch.optim.Adam} on the recorded draws"""
    from shine_mapping_amd import ops

    opt = _make_opt(cfg, wl, ss, False)
    opts = _opts(cfg.sigma_sigmoid, eik, 0.1)
    losses = []
    for idx in batches:
        coord, sd, rd, w = [t.contiguous() for t in pool.get_batch(idx)]
        opt.zero_grad(set_to_none=True)
        if composite:
            losses.append(float(_composite(wl.octree, wl.ray_decoder, coord, w, sd, rd, ss, opts, S_LOOP, neus, keep=True)))
        else:
            losses.append(float(ops.fused_ray_step(wl.octree, wl.ray_decoder, coord, w, sd, rd, ss, opts, S_LOOP, neus_on=neus)))
        opt.step()
    torch.cuda.synchronize()
    return losses


@pytest.mark.parametrize("eik", [False, True])
@pytest.mark.parametrize("neus", [False, True])
def test_graphed_ray_loop_matches_an_eager_replay_and_the_composite(workload, neus, eik):
    wl = workload
    cfg, params, pool, ss = _loop_parts(wl)
    g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, ss, True), ss, eik, neus)
    assert g.ray is not None and g.ran_eager and not g.native and not g.fold and not g.time and g.touched is None
    batches, hip_loss = [g._idx.clone()], [g.loss.clone()]
    for it in range(ITERS - 1):
        with counted_launches() as calls:
            loss = g()
        names = [c[0] for c in calls]
        assert names == (["shine_sample_sorted_dev", "shine_adam_step_dev"] if it == 0 else []), names
        batches.append(g._idx.clone())  # (the ray route draws inside the iteration: _idx is the batch that just ran)
        hip_loss.append(loss.clone())
    torch.cuda.synchronize()
    hip_loss = [float(x) for x in hip_loss]
    hip_params = [p.detach().clone() for p in params]
    assert all(x == x and abs(x) != float("inf") for x in hip_loss), hip_loss
    assert float(hip_params[-1][0]) != 1.0, "sigma_size moved"
    for composite in (False, True):
        cfg, params, _, ss2 = _loop_parts(wl)
        ref_loss = _replay(cfg, wl, pool, ss2, batches, eik, neus, composite)
        worst = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(hip_loss, ref_loss))
        errs = [rel_err(a, b) for a, b in zip(hip_params, params)]
        print("neus=%d eik=%d vs %s: worst loss %.2e" % (neus, eik, "composite + Adam" if composite else "eager replay", worst),
              "params", " ".join("%.1e" % e for e in errs), "sigma_size %.6f / %.6f" % (float(hip_params[-1]), float(params[-1])))
        assert worst <= LOOP_TOL["loss"], worst
        assert max(errs) <= LOOP_TOL["params"], errs
    _loop_parts(wl)


def test_unrolled_run_equals_single_calls_and_a_grown_octree_is_refused(workload):
    wl = workload
    K = 11
    out = []
    for unroll in (1, 5):
        cfg, params, pool, ss = _loop_parts(wl)
        g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, ss, True), ss, True, True, unroll=unroll)
        if unroll == 1:
            for _ in range(K):
                g()
        else:
            assert float(g.run(K)) == float(g.loss)  # 2 x 5 + 1
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for p in params], g._idx.clone(), float(g.loss)))
    assert torch.equal(out[0][1], out[1][1])  # (the same batches were drawn)
    errs = [rel_err(a, b) for a, b in zip(out[1][0], out[0][0])]
    print("unrolled vs single:", " ".join("%.1e" % e for e in errs), out[0][2], out[1][2])
    assert max(errs) <= TOL, errs
    assert abs(out[0][2] - out[1][2]) <= TOL * abs(out[0][2])
    wl.octree._tables_epoch += 1  # (what a growing octree does)
    try:
        with pytest.raises(RuntimeError, match="the octree grew"):
            g()
        with pytest.raises(RuntimeError, match="the octree grew"):
            g.run(2)
    finally:
        wl.octree._tables_epoch -= 1
    _loop_parts(wl)


# ---- 9. the dataset's pool
def test_dataset_ray_pool_equals_the_pools_and_is_replanned(tmp_path):
    from shine_mapping_amd import FeatureOctree, synth
    from shine_mapping_amd.dataset import LiDARDataset

    base = synth.make_config("ncd", device="cuda")
    drive = synth.write_kitti_drive(str(tmp_path), base, frames=3, beams=16, azimuths=90, device="cpu")
    cfg = synth.dataset_config("ncd", drive, pc_radius=20.0, min_range=2.5, bs=64, ray_loss=True)
    torch.manual_seed(1)
    octree = FeatureOctree(cfg)
    ds = LiDARDataset(cfg, octree)
    ds.process_frame(0)
    with pytest.raises(ValueError, match="not ray_loss"):
        ds.sorted_pool()
    rp = ds.ray_pool()
    assert rp is ds.ray_pool()
    S, m = ds.ray_sample_count, ds.ray_depth_pool.shape[0]
    p = rp.perm.long()
    assert rp.samples == S and rp.size == m
    assert torch.equal(rp.ray_depth, ds.ray_depth_pool[p]) and torch.equal(rp.coord.view(m, S, 3), ds.coord_pool.view(m, S, 3)[p])
    assert torch.equal(rp.sample_depth.view(m, S), ds.sample_depth_pool.view(m, S)[p])
    assert torch.equal(rp.weight.view(m, S), ds.weight_pool.view(m, S)[p])
    ds.process_frame(1)
    rp2 = ds.ray_pool()
    assert rp2 is rp and rp2.size == ds.ray_depth_pool.shape[0] > m and rp2.tables_epoch == octree._tables_epoch
    assert torch.equal(rp2.ray_depth, ds.ray_depth_pool[rp2.perm.long()])
