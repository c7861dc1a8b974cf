"""GPU: the surface-normal training step (csrc/shine_normal_step.hip) — ops.fused_normal_step against the fp64 CPU oracle
(tests/normal_step_oracle.py) on the five step fixtures and the value cases, against the GPU composite (drop-in query_feature ->
sdf -> get_gradient -> losses.normal_loss, backward) on every L x interpolation instantiation, over tile tails and gathers, the
pool's two record layouts, reproducibility, accumulation, the frozen decoder; then loop.GraphedIteration(normal=...) against an
eager replay of its own batches, and the dataset's pool.

Tolerance: the project's contract, TOL = 1e-4 of tests/test_gpu_parity.py — the loss absolute-or-relative, every gradient tensor
<= TOL of its max-abs against the fp64 oracle, a tensor whose oracle value is all zero <= TOL of the largest gradient tensor's
max-abs (tests/test_normal_step.py shows the fp32 reference itself at <= 2e-5)."""
import contextlib
import copy
import functools

import pytest
import torch

import normal_step_oracle as no
import step_value_cases as sv
from conftest import oracle_from_golden, product_from_golden
from test_gpu_parity import TOL
from test_gpu_sem_step import LOOP_TOL, counted_launches, rel_err

pytestmark = pytest.mark.gpu

WN = no.WEIGHT_N


@contextlib.contextmanager
def normal_calls():
    """the arguments of every shine_normal_train_step call made inside the block"""
    from shine_mapping_amd import _lib

    lib, seen = _lib.lib(), []
    fn = lib.shine_normal_train_step
    lib.shine_normal_train_step = lambda *a: (seen.append(a), fn(*a))[1]
    try:
        yield seen
    finally:
        lib.shine_normal_train_step = fn


def _conditioned(lab, g):
    """`lab` [n,3] float32 with the helper's condition enforced on EVERY row against the fp64 g: NaN -> 0, then a label closer
    than MIN_ELL to gh is replaced by its negative"""
    lab = torch.where(torch.isnan(lab), torch.zeros_like(lab), lab)
    gn = g.norm(dim=-1, keepdim=True)
    gh = torch.where(gn > 0, g / gn.clamp_min(1e-300), torch.zeros_like(g)).float()
    bad = ((gh - lab).norm(dim=-1) < no.MIN_ELL) & (gn.squeeze(1) > 0)
    lab[bad] = -lab[bad]
    assert bool(((gh - lab).norm(dim=-1)[gn.squeeze(1) > 0] >= no.MIN_ELL).all())
    return lab


def _clear(octree, dec):
    for p in list(octree.hier_features) + list(dec.parameters()):
        p.grad = None


def _fused(octree, dec, coord, weight, normal, weight_n=WN, **kw):
    from shine_mapping_amd import ops

    _clear(octree, dec)
    loss = ops.fused_normal_step(octree, dec, coord, weight, normal, weight_n, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.grad_fn is None
    mlp = dec.fused_params()
    out = (loss.clone(), [p.grad.clone() for p in octree.hier_features],
           None if mlp[0].grad is None else [p.grad.clone() for p in mlp])
    _clear(octree, dec)
    return out


def _check(what, got, ref):
    """got = _fused(...) against an oracle dict: the module's tolerance; everything finite; the biases untouched"""
    loss_err, errs = no.rel_errors(got[0], got[1], got[2], ref)
    print(what, "loss %.1e" % loss_err, " ".join("%.1e" % e for e in errs))
    assert all(bool(torch.isfinite(t).all()) for t in [got[0]] + got[1] + got[2]), what
    assert loss_err <= TOL and max(errs) <= TOL, (what, loss_err, errs)
    for k in (1, 3, 5):
        assert float(got[2][k].abs().max()) == 0.0, (what, "bias grad", k)


@functools.lru_cache(maxsize=None)
def _product(name):
    return product_from_golden(no.case(name).fx)


def _dev(c):
    return c.coord.cuda(), c.weight.cuda(), c.normal.cuda()


# ---- 1. one step against the oracle
@pytest.mark.parametrize("name", no.FIXTURES)
def test_one_step_matches_the_fp64_oracle(name):
    c = no.case(name)
    _, octree, dec = _product(name)
    assert c.zero_g > 0 and "nan" in c.hand
    _check(name, _fused(octree, dec, *_dev(c)), c.wide)


# ---- 2. sizes, and the same through a reversed gather
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2048])
def test_sizes_and_the_reversed_gather(n):
    c = no.case("kitti_eik_L3")
    _, octree, dec = _product("kitti_eik_L3")
    coord, weight, normal = _dev(c)
    assert coord.shape[0] >= 2048 and float(c.weight[0]) > 0 and float(c.weight[2]) < 0
    oct_, mlp = no.wide_oracle(c.fx)
    ref = no.normal_term(oct_, mlp, c.coord[:n], c.weight[:n], c.normal[:n], WN)
    plain = _fused(octree, dec, coord[:n].contiguous(), weight[:n].contiguous(), normal[:n].contiguous())
    _check("n=%d" % n, plain, ref)
    idx = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")
    _check("n=%d gathered" % n, _fused(octree, dec, coord, weight, normal, idx=idx), ref)
    if n == 1:  # ... and one free-space row: the loss is 0, nothing is written, nothing is NaN (its label is)
        idx = torch.tensor([2], dtype=torch.int32, device="cuda")
        assert bool(torch.isnan(normal[2]).all())
        got = _fused(octree, dec, coord, weight, normal, idx=idx)
        assert float(got[0]) == 0.0 and all(float(t.abs().max()) == 0.0 for t in got[1] + got[2])
    from shine_mapping_amd import ops

    assert float(ops.fused_normal_step(octree, dec, coord[:0], weight[:0], normal[:0], WN)) == 0.0
    _clear(octree, dec)


# ---- 2b. the grid sum's boundaries (a tile is 64 rows, a workgroup 4 tiles, a first-level run 16 workgroups): exactly one full
#      run, a run of one workgroup behind it, and every workgroup plus a grid-stride pass.  The fixture's 2048 rows repeated.  The
#      loss and the weight grads are the same bits from call to call at each size.  The fp64 oracle takes half a minute at 65537
#      rows, so there it is put together from its values on the 2048 rows and on the one row behind the 32 repeats: the term is a
#      sum over surface rows divided by their count.
@pytest.mark.parametrize("n", [4096, 4113, 65537])
def test_grid_sum_boundary_sizes(n):
    c = no.case("kitti_eik_L3")
    _, octree, dec = _product("kitti_eik_L3")
    n0 = c.coord.shape[0]
    rows = torch.arange(n) % n0
    coord, weight, normal = (t[rows].contiguous().cuda() for t in (c.coord, c.weight, c.normal))
    a, b = _fused(octree, dec, coord, weight, normal), _fused(octree, dec, coord, weight, normal)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2])), n
    oct_, mlp = no.wide_oracle(c.fx)
    if n <= 2 * n0 + 64:
        ref = no.normal_term(oct_, mlp, c.coord[rows], c.weight[rows], c.normal[rows], WN)
    else:
        q, r = divmod(n, n0)
        whole = no.normal_term(oct_, mlp, c.coord, c.weight, c.normal, WN)
        rest = no.normal_term(oct_, mlp, c.coord[:r], c.weight[:r], c.normal[:r], WN)
        w0, wr = q * int((c.weight > 0).sum()), int((c.weight[:r] > 0).sum())
        assert r > 0 and wr > 0

        def mix(x, y):
            return (w0 * x.double() + wr * y.double()) / (w0 + wr)

        ref = dict(loss=mix(whole["loss"], rest["loss"]),
                   feat_grads=[mix(x, y) for x, y in zip(whole["feat_grads"], rest["feat_grads"])],
                   mlp_grads=[mix(x, y) for x, y in zip(whole["mlp_grads"], rest["mlp_grads"])])
    _check("n=%d" % n, a, ref)


# ---- 3. every instantiation against the GPU composite
def _composite(octree, dec, coord, weight, normal, weight_n=WN):
    from shine_mapping_amd import get_gradient, losses

    _clear(octree, dec)
    x = coord.detach().clone().requires_grad_(True)
    pred = dec.sdf(octree.query_feature(x))
    g = get_gradient(x, pred)
    loss = losses.normal_loss(g, normal, weight)
    (weight_n * loss).backward()
    mlp = dec.fused_params()
    out = dict(loss=loss.detach().cpu(), feat_grads=[p.grad.detach().cpu().clone() for p in octree.hier_features],
               mlp_grads=[(torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().clone() for p in mlp])
    _clear(octree, dec)
    return out, g.detach()


def _safe_labels(g, weight, seed):
    """seeded random unit labels under the helper's condition (l >= 0.05 on live surface rows: a violating label is negated)"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lab = torch.randn(g.shape, device="cuda", generator=gen)
    lab = lab / lab.norm(dim=-1, keepdim=True)
    gn = g.norm(dim=-1, keepdim=True)
    gh = torch.where(gn > 0, g / gn.clamp_min(1e-30), torch.zeros_like(g))
    bad = ((gh - lab).norm(dim=-1) < no.MIN_ELL) & (gn.squeeze(1) > 0)
    lab[bad] = -lab[bad]
    live = (weight > 0) & (gn.squeeze(1) > 0)
    assert bool(((gh - lab).norm(dim=-1)[live] >= no.MIN_ELL).all())
    return lab.contiguous()


def _synth_batch(wl, n, seed):
    """n pool samples; rows 3..6 are moved outside the mapped box (they miss every node: g == 0) and made surface rows"""
    from shine_mapping_amd import synth

    gen = torch.Generator(device="cuda").manual_seed(seed)
    coord, _, weight = synth.draw_batch(wl.pool, n, gen)
    coord, weight = coord.clone(), weight.clone()
    cell = wl.cfg.leaf_vox_size * wl.cfg.scale
    coord[3:7] = (wl.pool.coord.max(0).values + 3.0 * cell).clamp(max=0.999)
    weight[3:7] = 1.0
    coord, weight = coord.contiguous(), weight.contiguous()
    _, g = _composite(wl.octree, wl.decoder, coord, weight, torch.zeros_like(coord))
    assert float(g[3:7].abs().max()) == 0.0, "rows meant to miss every level"
    return coord, weight, _safe_labels(g, weight, seed + 1)


@pytest.mark.parametrize("poly", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_every_instantiation_matches_the_composite(L, poly):
    from shine_mapping_amd import synth

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L,
                              poly_int_on=poly)
    assert wl.octree.featured_level_num == L and bool(wl.octree.step_config().poly_int_on) == poly
    coord, weight, normal = _synth_batch(wl, 200, 5)
    ref, _ = _composite(wl.octree, wl.decoder, coord, weight, normal)
    assert bool(torch.isfinite(ref["loss"])) and float(ref["feat_grads"][-1].abs().max()) > 0
    _check("L=%d poly=%d" % (L, poly), _fused(wl.octree, wl.decoder, coord, weight, normal), ref)


# ---- 4. no surface row; all rows surface; n_surf as parts
def test_no_surface_all_surface_and_surface_count_forms():
    c = no.case("maicity_bce_L3")
    _, octree, dec = _product("maicity_bce_L3")
    coord, weight, normal = _dev(c)
    n = coord.shape[0]
    got = _fused(octree, dec, coord, -weight.abs() - 1.0, normal)
    assert float(got[0]) == 0.0 and all(float(t.abs().max()) == 0.0 for t in got[1] + got[2])
    ones = torch.ones(n)
    lab = _conditioned(c.normal.clone(), c.wide["g"])
    oct_, mlp = no.wide_oracle(c.fx)
    ref = no.normal_term(oct_, mlp, c.coord, ones, lab, WN)
    _check("all surface", _fused(octree, dec, coord, ones.cuda(), lab.cuda()), ref)
    # the surface count as the draw's partial counts, and as one count: the same bits
    ns = int((c.weight > 0).sum())
    parts = torch.zeros(64, dtype=torch.int64, device="cuda")
    parts[0], parts[5], parts[63] = ns - 7, 4, 3
    one = torch.tensor([ns], dtype=torch.int64, device="cuda")
    a = _fused(octree, dec, coord, weight, normal, n_surf=parts)
    b = _fused(octree, dec, coord, weight, normal, n_surf=one)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    _check("n_surf parts", a, c.wide)
    # a caller-supplied (global) count is the divisor
    twice = _fused(octree, dec, coord, weight, normal, n_surf=2 * one)
    assert abs(float(twice[0]) - 0.5 * float(b[0])) <= 1e-6 * float(b[0])


# ---- 5. value cases
# CONDITION ON THE INPUTS, beside the helper's l >= 0.05 and as little a tolerance: no live surface row of the batch has an fp64
# |g| below FAINT_G times the median |g| of the live surface rows.  The term's condition number is 1 / |g|: q carries 1 / |g|, so
# a row whose |g| is orders below the batch's typical one owns the gradient tensors' largest entries, and its g is what cancellation
# leaves of a sum whose terms are of the typical size — ONE fp32 rounding of such a sum is 2^-24 of the median, i.e. 6e-8 / rho of a
# |g| that is rho times the median: 6e-5 at rho = 1e-3, the contract's own size.  Such a row is handed to the step as a free-space
# row (weight = -|weight|), and the condition is asserted.  Two rows of (kitti_eik_L3, on_kink) — one at |g| = 1.1e-2 beside a
# median of 2.2e3, where the REFERENCE's fp32 evaluation is 2.2e-2 of max-abs from the fp64 one — and two of (maicity_bce_L4,
# on_kink) go that way, none elsewhere; under the condition the reference's fp32 evaluation is within 5.5e-5 on every case
# (measured on the CPU oracle).
FAINT_G = 1e-3
VALUE_CASES = [(name, kind) for name in sv.FIXTURES for kind in ("dead", "dead_points", "on_kink")]


def _without_faint_rows(weight, g):
    """`weight` with every live surface row whose |g| < FAINT_G x the live surface rows' median turned into a free-space row"""
    gn = g.norm(dim=-1)
    live = (weight > 0) & (gn > 0)
    if not bool(live.any()):
        return weight.clone(), 0
    floor = FAINT_G * float(gn[live].median())
    faint = live & (gn < floor)
    out = torch.where(faint, -weight.abs(), weight)
    assert bool((gn[(out > 0) & (gn > 0)] >= floor).all()), "the condition on the inputs: no faint-gradient surface row"
    return out, int(faint.sum())


@pytest.mark.parametrize("name,kind", VALUE_CASES)
def test_value_cases(name, kind):
    c = no.case(name)
    case = sv.value_case(sv.fixture(name), kind)
    _, octree, dec = sv.apply_to_product(case, product_from_golden(c.fx))
    _, oct_, mlp = sv.apply_to_oracle(case, oracle_from_golden(c.fx))
    from oracle import shine_oracle as so

    so.to_wide(oct_, mlp)
    # labels under the helper's condition for THIS map's g (the fixture's labels were made for another map)
    g = no.normal_term(oct_, mlp, c.coord, torch.ones(c.coord.shape[0]), torch.zeros(c.coord.shape[0], 3), 1.0)["g"]
    lab = _conditioned(c.normal.clone(), g)
    weight, faint = _without_faint_rows(c.weight, g)
    print(name, kind, "faint-gradient surface rows handed over as free space:", faint)
    assert faint <= 2 and int((weight > 0).sum()) >= int((c.weight > 0).sum()) - 2  # (the case keeps its batch)
    ref = no.normal_term(oct_, mlp, c.coord, weight, lab, WN)
    got = _fused(octree, dec, c.coord.cuda(), weight.cuda(), lab.cuda())
    surf = weight > 0
    if kind == "dead":  # every g == 0: the mean of |n| over the surface rows, every gradient exactly zero
        want = float(lab[surf].double().norm(dim=-1).mean())
        assert abs(float(got[0]) - want) <= TOL * want
        assert all(float(t.abs().max()) == 0.0 for t in got[1] + got[2])
        return
    _check(kind, got, ref)
    # the zero-feature quarter gets no gradient: the rows only its points address stay exactly zero
    zp = case.zero_points
    assert float(ref["g"][zp].abs().max()) == 0.0
    idx_zero = oct_.get_indices(c.coord[zp & surf])
    idx_rest = oct_.get_indices(c.coord[~zp & surf])
    L = len(idx_zero)
    for i in range(L):
        only = set(idx_zero[i].flatten().tolist()) - set(idx_rest[i].flatten().tolist()) - {-1}
        if only:
            rows = torch.tensor(sorted(only))
            assert float(got[1][L - 1 - i].cpu()[rows].abs().max()) == 0.0, (kind, i)


# ---- 6. sigma invariance
def test_sigma_does_not_enter():
    c = no.case("maicity_bce_L4")
    oct_, mlp = no.wide_oracle(c.fx)
    scaled = no.normal_term(oct_, mlp, c.coord, c.weight, c.normal, WN, sigma=0.07)
    loss_err, errs = no.rel_errors(scaled["loss"], scaled["feat_grads"], scaled["mlp_grads"], c.wide)
    assert loss_err <= 1e-12 and max(errs) <= 1e-10, (loss_err, errs)
    _, octree, dec = _product("maicity_bce_L4")
    got = _fused(octree, dec, *_dev(c))
    _check("sigma 1.0", got, c.wide)
    _check("sigma 0.07", got, scaled)


# ---- 7. pool mode, both record layouts
@pytest.mark.parametrize("L", [3, 4])
def test_pool_mode_reads_the_records(L):
    from shine_mapping_amd import synth
    from shine_mapping_amd.sampler import SortedPool

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L)
    pl = wl.pool
    _, g = _composite(wl.octree, wl.decoder, pl.coord.contiguous(), pl.weight.contiguous(), torch.zeros_like(pl.coord))
    lab = _safe_labels(g, pl.weight, 21)
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=3, normal_label=lab)
    assert pool.rec is not None and (pool._weight_sep is None) == (L < 4)
    assert torch.equal(pool.normal_label, lab[pool.perm.long()])
    parts = pool.surf_parts_buffer(1000)
    idx = pool.draw(1000, surf_parts=parts)
    coord, _, weight = pool.get_batch(idx)
    normal = pool.normal_label[idx.long()].contiguous()
    assert int(parts.sum()) == int((weight > 0).sum())
    got = _fused(wl.octree, wl.decoder, None, None, None, pool=pool, idx=idx)
    with_parts = _fused(wl.octree, wl.decoder, None, None, None, pool=pool, idx=idx, n_surf=parts)
    plain = _fused(wl.octree, wl.decoder, coord, weight, normal)
    assert torch.equal(got[0], plain[0]) and torch.equal(with_parts[0], plain[0]), L  # (the same row order: the same bits)
    assert all(torch.equal(a, b) for a, b in zip(got[2], plain[2]))
    for a, b in zip(got[1], plain[1]):
        assert rel_err(a, b) <= TOL, (L, rel_err(a, b))
    ref, _ = _composite(wl.octree, wl.decoder, coord, weight, normal)
    _check("pool L=%d" % L, got, ref)
    plain_pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=3)
    assert not hasattr(plain_pool, "normal_label")
    from shine_mapping_amd import ops

    with pytest.raises(ValueError, match="normal_label="):
        ops.fused_normal_step(wl.octree, wl.decoder, None, None, None, WN, pool=plain_pool, idx=idx)


# ---- 8. determinism, accumulation, grad_buffers, the frozen decoder, the workspace
def test_determinism_accumulation_buffers_frozen_decoder_and_workspace():
    from shine_mapping_amd import _lib, autograd_ops, ops

    c = no.case("maicity_bce_L4")
    _, octree, dec = product_from_golden(c.fx)
    coord, weight, normal = _dev(c)
    a, b = _fused(octree, dec, coord, weight, normal), _fused(octree, dec, coord, weight, normal)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    # a second call doubles the grads
    _clear(octree, dec)
    ws = _lib.zeroed_workspace(autograd_ops.NORMAL_WORKSPACE_BYTES, coord.device)
    ops.fused_normal_step(octree, dec, coord, weight, normal, WN, workspace=ws)
    ops.fused_normal_step(octree, dec, coord, weight, normal, WN, workspace=ws)
    params = list(octree.hier_features) + list(dec.fused_params())
    for k, (p, r) in enumerate(zip(params, a[1] + a[2])):
        assert float((p.grad - 2 * r).abs().max()) <= TOL * float(r.abs().max()) or float(r.abs().max()) == 0.0, k
    assert not bool(ws.any()), "the workspace is all zero after a call"
    # grad_buffers: the same numbers land in the buffers, .grad stays as it is
    kept = [p.grad.clone() for p in params]
    bufs = ([torch.zeros_like(p) for p in octree.hier_features], [torch.zeros_like(p) for p in dec.fused_params()])
    ops.fused_normal_step(octree, dec, coord, weight, normal, WN, grad_buffers=bufs)
    assert all(torch.equal(p.grad, k) for p, k in zip(params, kept))
    assert all(torch.equal(x, y) for x, y in zip(bufs[1], a[2]))
    for x, y in zip(bufs[0], a[1]):
        assert rel_err(x, y) <= TOL
    _clear(octree, dec)
    # a decoder that is neither trained nor frozen is refused; a frozen one gets no gradient and the same feature grads
    dec.fused_params()[2].requires_grad_(False)
    with pytest.raises(ValueError, match="all require grad or all be frozen"):
        ops.fused_normal_step(octree, dec, coord, weight, normal, WN)
    for p in dec.parameters():
        p.requires_grad_(False)
    guard = [p.detach().clone() for p in dec.parameters()]
    _clear(octree, dec)
    loss = ops.fused_normal_step(octree, dec, coord, weight, normal, WN)
    assert all(p.grad is None for p in dec.parameters())
    assert all(torch.equal(p, g) for p, g in zip(dec.parameters(), guard))
    assert torch.equal(loss, a[0])
    for p, r in zip(octree.hier_features, a[1]):
        assert rel_err(p.grad, r) <= TOL
    for bad in (dict(out=torch.zeros(2, device="cuda")), dict(n_surf=torch.zeros(1, device="cuda")),
                dict(idx=torch.zeros(4, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            ops.fused_normal_step(octree, dec, coord, weight, normal, WN, **bad)
    with pytest.raises(ValueError, match="normal_label"):
        ops.fused_normal_step(octree, dec, coord, weight, normal[:, :2].contiguous(), WN)
    with pytest.raises(ValueError, match="weight"):
        ops.fused_normal_step(octree, dec, coord, weight.double(), normal, WN)


# ---- 9. the loop
ITERS = 12
N = 4096
W_LOOP = 0.05


@pytest.fixture(scope="module")
def workload():
    from shine_mapping_amd import synth

    return synth.build_workload("maicity", frames=12, beams=32, azimuths=180, device="cuda", seed=7)


@pytest.fixture(scope="module")
def loop_start(workload):
    """every parameter's start and the pool's labels (unit vectors that lean to the map's own gradient direction, so the term has
    something to learn); one eager iteration has run on the device afterwards"""
    wl = workload
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters())]
    pl = wl.pool
    _, g = _composite(wl.octree, wl.decoder, pl.coord.contiguous(), pl.weight.contiguous(), torch.zeros_like(pl.coord))
    lab = _safe_labels(g, pl.weight, 31)
    cfg, _, pool = _loop_parts(wl, start, lab)
    it = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True))
    assert it.ran_eager and not it.native and float(it.normal_loss) > 0
    return start, lab


def _loop_parts(wl, start, lab, seed=11, sem=None):
    from shine_mapping_amd import autograd_ops
    from shine_mapping_amd.sampler import SortedPool

    params = list(wl.octree.hier_features) + list(wl.decoder.parameters())
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
            p.grad = None
            p.requires_grad_(True)
    autograd_ops.bump_param_epoch()
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.ray_loss, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, False, 1.0
    pl = wl.pool
    kw = {}
    if sem is not None:
        from test_gpu_sem_step import C_LOOP, _labels

        kw = dict(sem_label=_labels(pl.coord, pl.weight, C_LOOP), n_class=C_LOOP)
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=seed, canonical=True, normal_label=lab, **kw)
    return cfg, params, pool


def _make_opt(cfg, wl, hip, sem=None):
    from shine_mapping_amd import optim

    feats, geo = list(wl.octree.parameters()), list(wl.decoder.parameters())
    semp = list(sem.parameters()) if sem is not None else None
    if hip:
        if sem is not None:
            return optim.setup_optimizer(cfg, feats, geo, semp, None)
        return optim.setup_optimizer(cfg, feats, wl.decoder.fused_params())
    groups = [{"params": wl.decoder.fused_params() if sem is None else geo, "lr": cfg.lr, "weight_decay": cfg.weight_decay}]
    if sem is not None:
        groups.append({"params": semp, "lr": cfg.lr, "weight_decay": cfg.weight_decay})
    groups += [{"params": feats[cfg.tree_level_feat - i - 1], "lr": cfg.lr} for i in range(cfg.tree_level_feat)]
    return torch.optim.Adam(groups, betas=(0.9, 0.99), eps=cfg.adam_eps)


def _graphed(cfg, wl, pool, opt, sem=None, **kw):
    from shine_mapping_amd import StepOptions
    from shine_mapping_amd.loop import GraphedIteration, NormalTerm, SemTerm

    if sem is not None:
        kw["sem"] = SemTerm(sem, 0.7, 3)
    return GraphedIteration(wl.octree, wl.decoder, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid), N,
                            normal=NormalTerm(W_LOOP), **kw)


def _eager_replay(cfg, wl, pool, params, batches, sem=None):
    """{fused_train_step, [the semantic composite,] fused_normal_step, torch.optim.Adam} on the recorded draws"""
    from shine_mapping_amd import StepOptions, ops

    opt = _make_opt(cfg, wl, False, sem)
    opts = StepOptions(sigma=cfg.sigma_sigmoid)
    losses, normals, sems = [], [], []
    for idx in batches:
        coord, sdf_label, weight = pool.get_batch(idx)
        normal = pool.normal_label[idx.long()].contiguous()
        opt.zero_grad(set_to_none=True)
        if sem is not None:
            labels = pool.sem_label[idx.long()].long()
            sem_loss = torch.nn.NLLLoss(reduction="mean")(sem._sem_composite(wl.octree.query_feature(coord))[::3, :], labels[::3])
            (0.7 * sem_loss).backward()
            sems.append(float(sem_loss.detach()))
        loss, _, _ = ops.fused_train_step(wl.octree, wl.decoder, coord, sdf_label, weight, opts)
        normals.append(float(ops.fused_normal_step(wl.octree, wl.decoder, coord, weight, normal, W_LOOP)))
        opt.step()
        losses.append(float(loss))
    torch.cuda.synchronize()
    return losses, normals, sems


def test_graphed_normal_loop_matches_an_eager_replay(workload, loop_start):
    wl = workload
    start, lab = loop_start
    cfg, params, pool = _loop_parts(wl, start, lab)
    g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True), eager_first=False)
    assert not g.ran_eager and not g.native and g.sem is None
    batches, hip_loss, hip_normal = [], [], []
    for it in range(ITERS):
        batches.append(g._idx.clone())
        with counted_launches() as calls, normal_calls() as normal:
            loss = g()
        names = [c[0] for c in calls]
        if it == 0:  # this object's first call records the iteration: fused kernel, normal kernel, tail
            assert names == ["shine_train_step", "shine_finish_iteration"] and len(normal) == 1, (names, len(normal))
            assert calls[0][1][1]._obj.defer_reduce == 1 and normal[0][9] == 64  # (the draw's partial surface counts)
        else:
            assert names == [] and normal == []  # (a replay goes through no entry point)
        hip_loss.append(loss.clone())
        hip_normal.append(g.normal_loss.clone())
    torch.cuda.synchronize()
    hip_loss, hip_normal = [float(x) for x in hip_loss], [float(x) for x in hip_normal]
    hip_params = [p.detach().clone() for p in params]
    cfg, params, _ = _loop_parts(wl, start, lab)
    ref_loss, ref_normal, _ = _eager_replay(cfg, wl, pool, params, batches)
    worst = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(hip_loss + hip_normal, ref_loss + ref_normal))
    errs = [rel_err(a, b) for a, b in zip(hip_params, params)]
    print("worst loss %.2e" % worst, "params", " ".join("%.1e" % e for e in errs))
    print("normal_loss %.4f -> %.4f" % (hip_normal[0], hip_normal[-1]))
    assert all(x == x for x in hip_normal) and worst <= LOOP_TOL["loss"], worst
    assert max(errs) <= LOOP_TOL["params"], errs
    _loop_parts(wl, start, lab)


def test_unrolled_run_equals_single_calls(workload, loop_start):
    wl = workload
    start, lab = loop_start
    K = 5
    out = []
    for unroll in (1, 2):
        cfg, params, pool = _loop_parts(wl, start, lab)
        g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True), eager_first=False, unroll=unroll)
        if unroll == 1:
            for _ in range(K):
                g()
        else:
            g.run(K)  # 2 x 2 + 1
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for p in params], g._idx.clone(), float(g.normal_loss), float(g.loss)))
    assert torch.equal(out[0][1], out[1][1])  # (the same batches were drawn)
    errs = [rel_err(a, b) for a, b in zip(out[1][0], out[0][0])]
    print("unrolled vs single:", " ".join("%.1e" % e for e in errs), out[0][2:], out[1][2:])
    assert max(errs) <= TOL, errs
    assert abs(out[0][2] - out[1][2]) <= TOL * abs(out[0][2])
    _loop_parts(wl, start, lab)


def test_semantic_and_normal_terms_together(workload, loop_start):
    from test_gpu_sem_step import C_LOOP, _head

    wl = workload
    start, lab = loop_start
    sem = _head(C_LOOP, seed=4)
    sem_start = [p.detach().clone() for p in sem.parameters()]

    def reset_head():
        with torch.no_grad():
            for p, s0 in zip(sem.parameters(), sem_start):
                p.copy_(s0)
                p.grad = None

    cfg, params, pool = _loop_parts(wl, start, lab, sem=sem)
    cfg.semantic_on = True
    g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True, sem), sem=sem, eager_first=False)
    assert not g.ran_eager and not g.native
    batches, seen = [], []
    for it in range(6):
        batches.append(g._idx.clone())
        with counted_launches() as calls, normal_calls() as normal:
            g()
        if it == 0:  # {fused, semantic, normal, tail, head Adam}
            assert [c[0] for c in calls] == ["shine_train_step", "shine_sem_train_step", "shine_finish_iteration",
                                             "shine_adam_step_dev"] and len(normal) == 1, [c[0] for c in calls]
        seen.append((g.loss.clone(), g.normal_loss.clone(), g.sem_loss.clone()))
    torch.cuda.synchronize()
    seen = [tuple(float(v) for v in row) for row in seen]
    assert all(all(v == v and abs(v) != float("inf") for v in row) for row in seen), seen
    hip_params = [p.detach().clone() for p in params + list(sem.sem_params())]
    reset_head()
    cfg, params, _ = _loop_parts(wl, start, lab, sem=sem)
    cfg.semantic_on = True
    ref_loss, ref_normal, ref_sem = _eager_replay(cfg, wl, pool, params, batches, sem=sem)
    worst = max(abs(a - b) / max(abs(b), 1e-12)
                for row, ref in zip(seen, zip(ref_loss, ref_normal, ref_sem)) for a, b in zip(row, ref))
    errs = [rel_err(a, b) for a, b in zip(hip_params, params + list(sem.sem_params()))]
    print("sem + normal: worst loss %.2e" % worst, "params", " ".join("%.1e" % e for e in errs))
    # (the parameters are printed, not held to LOOP_TOL["params"]: six iterations in, one element whose three-term gradient sum
    # is rounding noise of either sign has moved by +-lr in the two runs — Adam's first steps are sign(g) * lr — and nothing
    # reads it: the losses are the check, as for every later iteration they are a function of all parameters that matter)
    assert worst <= LOOP_TOL["loss"], (worst, errs)
    assert seen[-1][1] == seen[-1][1] and seen[-1][2] < seen[0][2]
    _loop_parts(wl, start, lab)


def test_without_normal_the_iteration_is_the_two_launch_native_graph(workload):
    from shine_mapping_amd import StepOptions, optim
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.sampler import SortedPool

    wl = workload
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters())]
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, 1.0
    opt = optim.setup_optimizer(cfg, list(wl.octree.parameters()), wl.decoder.fused_params())
    pool = SortedPool(wl.octree, wl.pool.coord, wl.pool.sdf_label, wl.pool.weight, seed=5)
    g = GraphedIteration(wl.octree, wl.decoder, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid), N, normal=None)
    assert g.native and not g.ran_eager and g.normal is None and g.normal_loss is None and g._surf is None
    with counted_launches() as calls, normal_calls() as seen:
        g()
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["shine_iter_graph_set_step", "shine_iter_graph_set_finish"] and seen == []
    assert g.graph is None and g.graph_k is None
    with torch.no_grad():
        for p, s in zip(list(wl.octree.hier_features) + list(wl.decoder.parameters()), start):
            p.copy_(s)
            p.grad = None


# ---- 10. the dataset's pool
def test_dataset_pool_carries_the_normals_and_trains(tmp_path):
    from shine_mapping_amd import Decoder, FeatureOctree, StepOptions, forward_sdf, optim, synth
    from shine_mapping_amd.dataset import LiDARDataset
    from shine_mapping_amd.loop import GraphedIteration, NormalTerm

    base = synth.make_config("ncd", device="cuda")
    drive = synth.write_kitti_drive(str(tmp_path), base, frames=3, beams=16, azimuths=90, device="cpu")
    cfg = synth.dataset_config("ncd", drive, pc_radius=20.0, min_range=2.5, estimate_normal=True, normal_radius_m=1.0, normal_max_nn=20,
                               bs=N)
    torch.manual_seed(1)
    octree = FeatureOctree(cfg)
    ds = LiDARDataset(cfg, octree)
    for f in range(3):
        ds.process_frame(f)
    sp = ds.sorted_pool()
    assert sp.normal_label.dtype == torch.float32 and sp.normal_label.shape == (sp.size, 3)
    assert torch.equal(sp.normal_label, ds.normal_label_pool[sp.perm.long()].float())
    assert float(sp.normal_label.abs().max()) > 0
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, 1.0
    torch.manual_seed(3)
    geo = Decoder(cfg).cuda()
    surf = sp.weight > 0
    coord, normal = sp.coord[surf].contiguous(), sp.normal_label[surf]

    def alignment():
        g = forward_sdf(octree, geo, coord, want_grad_x=True)["grad_x"]
        gn = g.norm(dim=-1, keepdim=True)
        live = gn.squeeze(1) > 0
        return float(((g / gn.clamp_min(1e-30)) * normal).sum(-1)[live].mean())

    before = alignment()
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), geo.fused_params())
    g = GraphedIteration(octree, geo, sp, opt, StepOptions(sigma=cfg.sigma_sigmoid), N, normal=NormalTerm(1.0))
    seen = [g.normal_loss.clone()]
    for _ in range(19):
        g()
        seen.append(g.normal_loss.clone())
    seen = [float(x) for x in seen]
    after = alignment()
    print("normal_loss over 20 iterations: %.4f -> %.4f; mean gh.n %.4f -> %.4f" % (seen[0], seen[-1], before, after))
    assert all(x == x and abs(x) != float("inf") for x in seen) and seen[-1] < seen[0]
    assert after > before
