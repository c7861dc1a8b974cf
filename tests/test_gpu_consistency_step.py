"""GPU: the gradient-consistency training step (csrc/shine_consistency_step.hip) — ops.fused_consistency_step against the fp64 CPU
oracle (tests/consistency_step_oracle.py) on the five step fixtures and the value cases, over pair counts around the tile (32
pairs) and workgroup (128 pairs) sizes and past the grid stride, against the GPU composite (drop-in query_feature -> sdf ->
get_gradient on both point sets -> losses.consistency_loss, backward) on every L x interpolation instantiation, the pairs drawn
on the device, the touched-row flags, the pool's two record layouts, reproducibility, accumulation, the frozen decoder; then
loop.GraphedIteration(consistency=...) against an eager replay of its own batches and draws.

Tolerance: the project's contract, TOL = 1e-4 of tests/test_gpu_parity.py, through normal_step_oracle.rel_errors — the loss
absolute-or-relative, every gradient tensor <= TOL of its max-abs against the fp64 oracle, a tensor whose oracle value is all zero
<= TOL of the largest gradient tensor's max-abs — under the helper's condition on the inputs (no pair with a faint gradient on
either side; tests/test_consistency_step.py shows the fp32 reference itself at <= 1e-5 there).  Measured on an MI355X: the
kernel's largest error is 3.8e-5 ((kitti_eik_L3, on_kink)), at most 7.0e-6 on the five step fixtures."""
import contextlib
import copy
import functools

import pytest
import torch

import consistency_step_oracle as co
import normal_step_oracle as no
import step_value_cases as sv
from conftest import oracle_from_golden, product_from_golden
from test_gpu_parity import TOL
from test_gpu_sem_step import LOOP_TOL, counted_launches, rel_err

pytestmark = pytest.mark.gpu

WC = co.WEIGHT_C


@contextlib.contextmanager
def consistency_calls():
    """the arguments of every shine_consistency_train_step call made inside the block"""
    from shine_mapping_amd import _lib

    lib, seen = _lib.lib(), []
    fn = lib.shine_consistency_train_step
    lib.shine_consistency_train_step = lambda *a: (seen.append(a), fn(*a))[1]
    try:
        yield seen
    finally:
        lib.shine_consistency_train_step = fn


def _clear(octree, dec):
    for p in list(octree.hier_features) + list(dec.parameters()):
        p.grad = None


def _fused(octree, dec, coord, near, shift, weight_c=WC, **kw):
    from shine_mapping_amd import ops

    _clear(octree, dec)
    loss = ops.fused_consistency_step(octree, dec, coord, weight_c, near, shift, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.grad_fn is None
    mlp = dec.fused_params()
    out = (loss.clone(), [p.grad.clone() for p in octree.hier_features],
           None if mlp[0].grad is None else [p.grad.clone() for p in mlp])
    _clear(octree, dec)
    return out


def _check(what, got, ref):
    """got = _fused(...) against an oracle dict: the module's tolerance; everything finite; the biases untouched"""
    loss_err, errs = co.rel_errors(got[0], got[1], got[2], ref)
    print(what, "loss %.1e" % loss_err, " ".join("%.1e" % e for e in errs))
    assert all(bool(torch.isfinite(t).all()) for t in [got[0]] + got[1] + got[2]), what
    assert loss_err <= TOL and max(errs) <= TOL, (what, loss_err, errs)
    for k in (1, 3, 5):
        assert float(got[2][k].abs().max()) == 0.0, (what, "bias grad", k)
    return max([loss_err] + errs)


@functools.lru_cache(maxsize=None)
def _product(name):
    return product_from_golden(co.case(name).fx)


def _dev(c):
    return c.coord.cuda(), c.pairs.near_index.cuda(), c.pairs.shift.cuda()


# ---- 1. one step against the oracle
@pytest.mark.parametrize("name", co.FIXTURES)
def test_one_step_matches_the_fp64_oracle(name):
    c = co.case(name)
    _, octree, dec = _product(name)
    assert c.pairs.zero_g > 0 and c.pairs.near_index.numel() >= co.K_PAIRS - co.MAX_LEFT_OUT
    _check(name, _fused(octree, dec, *_dev(c)), c.wide)


# ---- 2. pair counts around a tile (32 pairs) and a workgroup (128 pairs), and the same through a reversed gather
@pytest.mark.parametrize("k", [1, 31, 32, 33, 127, 128, 129, 1000])
def test_pair_counts_and_the_reversed_gather(k):
    c = co.case("kitti_eik_L3")
    _, octree, dec = _product("kitti_eik_L3")
    coord, near, shift = _dev(c)
    n = coord.shape[0]
    oct_, mlp = no.wide_oracle(c.fx)
    ref = co.consistency_term(oct_, mlp, c.pairs.coord_a[:k], c.pairs.coord_b[:k], WC)
    near_k, shift_k = near[:k].contiguous(), shift[:k].contiguous()
    if k > 1:
        assert int(near_k[0]) == int(near_k[1])  # (a repeated base row)
    _check("k=%d" % k, _fused(octree, dec, coord, near_k, shift_k), ref)
    # batch row i = coord row n - 1 - i: the same points through the gather
    idx = torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda")
    _check("k=%d gathered" % k, _fused(octree, dec, coord, (n - 1 - near_k).contiguous(), shift_k, idx=idx), ref)


# ---- 2b. the grid sum's boundaries (a tile is 32 pairs, a workgroup 4 tiles, a first-level run 16 workgroups): exactly one full
#      run, a run of one workgroup behind it, and every workgroup plus a grid-stride pass.  The case's pairs repeated.  The loss
#      and the weight grads are the same bits from call to call at each size.  The fp64 oracle takes half a minute at 32769
#      pairs, so there it is put together from its values on the case's pairs and on the pairs behind the whole repeats: the term
#      is a sum over pairs divided by their count.
@pytest.mark.parametrize("k", [2048, 2049, 32769])
def test_grid_sum_boundary_pair_counts(k):
    c = co.case("kitti_eik_L3")
    _, octree, dec = _product("kitti_eik_L3")
    coord, near, shift = _dev(c)
    k0 = near.numel()
    sel = torch.arange(k) % k0
    near_k, shift_k = near[sel.cuda()].contiguous(), shift[sel.cuda()].contiguous()
    a, b = _fused(octree, dec, coord, near_k, shift_k), _fused(octree, dec, coord, near_k, shift_k)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2])), k
    oct_, mlp = no.wide_oracle(c.fx)
    if k <= 2 * k0 + 64:
        ref = co.consistency_term(oct_, mlp, c.pairs.coord_a[sel], c.pairs.coord_b[sel], WC)
    else:
        q, r = divmod(k, k0)
        whole = co.consistency_term(oct_, mlp, c.pairs.coord_a, c.pairs.coord_b, WC)
        rest = co.consistency_term(oct_, mlp, c.pairs.coord_a[:r], c.pairs.coord_b[:r], WC)
        assert r > 0

        def mix(x, y):
            return (q * k0 * x.double() + r * y.double()) / k

        ref = dict(loss=mix(whole["loss"], rest["loss"]),
                   feat_grads=[mix(x, y) for x, y in zip(whole["feat_grads"], rest["feat_grads"])],
                   mlp_grads=[mix(x, y) for x, y in zip(whole["mlp_grads"], rest["mlp_grads"])])
    _check("k=%d" % k, a, ref)


def test_no_pair_one_row_repeated_and_a_zero_shift():
    from shine_mapping_amd import ops

    c = co.case("kitti_eik_L3")
    _, octree, dec = _product("kitti_eik_L3")
    coord, near, shift = _dev(c)
    # K = 0: a loss of 0, nothing written
    got = _fused(octree, dec, coord, near[:0].contiguous(), shift[:0].contiguous())
    assert float(got[0]) == 0.0 and all(float(t.abs().max()) == 0.0 for t in got[1] + got[2])
    state = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert float(ops.fused_consistency_step(octree, dec, coord, WC, n_pairs=0, shift_scale=0.01, draw_state=state)) == 0.0
    assert int(state) == 0
    _clear(octree, dec)
    # every pair on ONE live base row (33 pairs: two tiles)
    live = torch.nonzero(c.wide["live"]).flatten()
    row = int(c.pairs.near_index[live[0]])
    k = 33
    near1 = torch.full((k,), row, dtype=torch.int32)
    shift1 = c.pairs.shift[live[:k]].contiguous()
    a = c.coord[near1.long()]
    oct_, mlp = no.wide_oracle(c.fx)
    ref = co.consistency_term(oct_, mlp, a, (a + shift1).float(), WC)
    assert int(ref["live"].sum()) > 0
    _check("one row, %d pairs" % k, _fused(octree, dec, coord, near1.cuda(), shift1.cuda()), ref)
    # a zero shift: both points are the same, c_k = 1 on the live pairs up to rounding — on live base rows only
    rows = torch.nonzero(c.wide["ga"].norm(dim=-1) > 0).flatten()[:500]
    near0 = c.pairs.near_index[rows].contiguous().cuda()
    got = _fused(octree, dec, coord, near0, torch.zeros(near0.numel(), 3, device="cuda"))
    print("zero shift: loss %.3g" % float(got[0]))
    assert 0.0 <= abs(float(got[0])) <= 1e-6


# ---- 3. past the grid stride: 256 workgroups x 128 pairs = 32768 in one sweep
def test_past_the_grid_stride_equals_the_sum_of_two_launches():
    c = co.case("maicity_bce_L3")
    _, octree, dec = _product("maicity_bce_L3")
    coord = c.coord.cuda()
    n = coord.shape[0]
    k = 32768 + 33
    gen = torch.Generator(device="cuda").manual_seed(9)
    near = torch.randint(0, n, (k,), generator=gen, device="cuda").to(torch.int32)
    s = 2.0 ** -12
    shift = ((torch.rand(k, 3, generator=gen, device="cuda") * 2 - 1) * s).contiguous()
    full = _fused(octree, dec, coord, near, shift)
    ka = 16384
    parts = []
    for lo, hi in ((0, ka), (ka, k)):
        parts.append(_fused(octree, dec, coord, near[lo:hi].contiguous(), shift[lo:hi].contiguous(), weight_c=WC * (hi - lo) / k))
    loss = (float(parts[0][0]) * ka + float(parts[1][0]) * (k - ka)) / k
    errs = [rel_err(f, a + b) for f, a, b in zip(full[1] + full[2], parts[0][1] + parts[0][2], parts[1][1] + parts[1][2])
            if float((a + b).abs().max()) > 0]
    print("grid stride: loss %.6f vs %.6f" % (float(full[0]), loss), " ".join("%.1e" % e for e in errs))
    assert abs(float(full[0]) - loss) <= TOL * max(1.0, abs(loss)) and len(errs) >= 5 and max(errs) <= TOL, errs
    assert all(float(full[2][i].abs().max()) == 0.0 for i in (1, 3, 5))


# ---- 4. every instantiation against the GPU composite
def _composite(octree, dec, coord_a, coord_b, weight_c=WC):
    from shine_mapping_amd import get_gradient, losses

    _clear(octree, dec)
    gs = []
    for x in (coord_a, coord_b):
        x = x.detach().clone().requires_grad_(True)
        gs.append(get_gradient(x, dec.sdf(octree.query_feature(x))))
    loss = losses.consistency_loss(gs[0], gs[1])
    (weight_c * loss).backward()
    mlp = dec.fused_params()
    out = dict(loss=loss.detach().cpu(), feat_grads=[p.grad.detach().cpu().clone() for p in octree.hier_features],
               mlp_grads=[(torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().clone() for p in mlp])
    _clear(octree, dec)
    return out, gs[0].detach(), gs[1].detach()


def _well_conditioned(ga, gb):
    """the helper's condition on the inputs from the GPU's own g: keep = not (live with a |g| below FAINT_G x the median)"""
    na, nb = ga.norm(dim=-1), gb.norm(dim=-1)
    live = (na > 0) & (nb > 0)
    if not bool(live.any()):
        return torch.ones_like(live)
    med = torch.cat([na[na > 0], nb[nb > 0]]).median()
    return ~(live & ((na < co.FAINT_G * med) | (nb < co.FAINT_G * med)))


def _synth_pairs(wl, n, k, seed):
    """n pool samples and k pairs on them, half a finest cell apart at most; rows 3..6 are moved outside the mapped box (they miss
    every level: g == 0) and are the first base rows.  The helper's condition is applied (at most 1 % of the pairs may go)."""
    from shine_mapping_amd import synth

    gen = torch.Generator(device="cuda").manual_seed(seed)
    coord, _, _ = synth.draw_batch(wl.pool, n, gen)
    coord = coord.clone()
    cell = wl.cfg.leaf_vox_size * wl.cfg.scale
    coord[3:7] = (wl.pool.coord.max(0).values + 3.0 * cell).clamp(max=0.999)
    coord = coord.contiguous()
    near = torch.randint(0, n, (k,), generator=gen, device="cuda")
    near[:4] = torch.arange(3, 7, device="cuda")
    shift = (torch.rand(k, 3, generator=gen, device="cuda") * 2 - 1) * (0.5 * cell)
    a = coord[near]
    _, ga, gb = _composite(wl.octree, wl.decoder, a, (a + shift).contiguous())
    assert float(ga[:4].abs().max()) == 0.0, "rows meant to miss every level"
    keep = _well_conditioned(ga, gb)
    assert int((~keep).sum()) <= k // 100
    return coord, near[keep].to(torch.int32).contiguous(), shift[keep].contiguous()


@pytest.mark.parametrize("poly", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_every_instantiation_matches_the_composite(L, poly):
    from shine_mapping_amd import synth

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L,
                              poly_int_on=poly)
    assert wl.octree.featured_level_num == L and bool(wl.octree.step_config().poly_int_on) == poly
    coord, near, shift = _synth_pairs(wl, 200, 200, 5)
    a = coord[near.long()]
    ref, ga, gb = _composite(wl.octree, wl.decoder, a, (a + shift).contiguous())
    assert bool(torch.isfinite(ref["loss"])) and float(ref["feat_grads"][-1].abs().max()) > 0
    _check("L=%d poly=%d" % (L, poly), _fused(wl.octree, wl.decoder, coord, near, shift), ref)


# ---- 5. value cases
VALUE_CASES = [(name, kind) for name in sv.FIXTURES for kind in ("dead", "dead_points", "on_kink")]


@pytest.mark.parametrize("name,kind", VALUE_CASES)
def test_value_cases(name, kind):
    from oracle import shine_oracle as so

    c = co.case(name)
    case = sv.value_case(sv.fixture(name), kind)
    _, octree, dec = sv.apply_to_product(case, product_from_golden(c.fx))
    _, oct_, mlp = sv.apply_to_oracle(case, oracle_from_golden(c.fx))
    so.to_wide(oct_, mlp)
    pairs = co.pairs_for(c.fx, oracle=(oct_, mlp))  # the condition for THIS map's g (asserts at most 16 pairs left out)
    print(name, kind, "pairs", pairs.near_index.numel(), "left out", pairs.left_out, "zero-g", pairs.zero_g)
    got = _fused(octree, dec, c.coord.cuda(), pairs.near_index.cuda(), pairs.shift.cuda())
    if kind == "dead":  # every g == 0: every pair is behind the guard — a loss of exactly 1, every gradient exactly zero
        assert float(got[0]) == 1.0
        assert all(float(t.abs().max()) == 0.0 for t in got[1] + got[2])
        return
    ref = co.consistency_term(oct_, mlp, pairs.coord_a, pairs.coord_b, WC)
    _check(kind, got, ref)
    # the zero-feature quarter gets no gradient: the rows only its points (base or shifted) address stay exactly zero
    za, zb = ref["ga"].norm(dim=-1) == 0, ref["gb"].norm(dim=-1) == 0
    dead_pts = torch.cat([pairs.coord_a[za], pairs.coord_b[zb]])
    rest_pts = torch.cat([pairs.coord_a[~za], pairs.coord_b[~zb]])
    assert dead_pts.shape[0] > 0
    idx_zero, idx_rest = oct_.get_indices(dead_pts), oct_.get_indices(rest_pts)
    L = len(idx_zero)
    for i in range(L):
        only = set(idx_zero[i].flatten().tolist()) - set(idx_rest[i].flatten().tolist()) - {-1}
        if only:
            rows = torch.tensor(sorted(only))
            assert float(got[1][L - 1 - i].cpu()[rows].abs().max()) == 0.0, (kind, i)


# ---- 6. pairs drawn on the device
def test_drawn_pairs():
    from shine_mapping_amd import ops

    c = co.case("maicity_bce_L4")
    _, octree, dec = _product("maicity_bce_L4")
    coord = c.coord.cuda()
    n, k, s = coord.shape[0], 1000, 2.0 ** -12

    def drawn(state, seed=3):
        _clear(octree, dec)
        draws = (torch.full((k,), -1, dtype=torch.int32, device="cuda"), torch.full((k, 3), 9.0, device="cuda"))
        loss = ops.fused_consistency_step(octree, dec, coord, WC, n_pairs=k, shift_scale=s, seed=seed, draw_state=state,
                                          draws_out=draws)
        out = (loss.clone(), [p.grad.clone() for p in octree.hier_features], [p.grad.clone() for p in dec.fused_params()])
        _clear(octree, dec)
        return out, draws

    state = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    first, d1 = drawn(state)
    assert int(state) == 6  # the launch advanced it by one
    near, shift = d1
    assert int(near.min()) >= 0 and int(near.max()) < n and near.unique().numel() > k // 2
    assert float(shift.min()) >= -s and float(shift.max()) < s and float(shift.abs().max()) > 0.9 * s
    assert abs(float(shift.mean())) < 0.1 * s  # (3000 uniform variates: the mean's sigma is 0.01 s)
    second, d2 = drawn(state)
    assert int(state) == 7 and not torch.equal(d1[0], d2[0]) and not torch.equal(d1[1], d2[1])
    again, d3 = drawn(torch.full((1,), 5, dtype=torch.int64, device="cuda"))  # the same (seed, state): the same draws
    assert torch.equal(d3[0], d1[0]) and torch.equal(d3[1], d1[1]) and torch.equal(again[0], first[0])
    _, d4 = drawn(torch.full((1,), 5, dtype=torch.int64, device="cuda"), seed=4)
    assert not torch.equal(d4[0], d1[0])
    # an explicit call fed the written draws: the same loss and decoder grads to the bit, feature grads within TOL
    explicit = _fused(octree, dec, coord, near, shift)
    assert torch.equal(explicit[0], first[0]) and all(torch.equal(a, b) for a, b in zip(explicit[2], first[2]))
    for a, b in zip(explicit[1], first[1]):
        assert rel_err(a, b) <= TOL
    assert float(first[0]) > 0 and float(first[1][-1].abs().max()) > 0


# ---- 7. the touched-row flags
def test_every_row_with_a_gradient_is_flagged():
    from shine_mapping_amd import ops

    c = co.case("maicity_bce_L4")
    _, octree, dec = _product("maicity_bce_L4")
    coord, near, shift = _dev(c)
    touched = ops.touched_flags(octree)
    got = _fused(octree, dec, coord, near, shift, touched=touched)
    plain = _fused(octree, dec, coord, near, shift)
    assert torch.equal(got[0], plain[0]) and all(torch.equal(a, b) for a, b in zip(got[2], plain[2]))
    _, oct_, _ = oracle_from_golden(c.fx)
    base_rows = oct_.get_indices(c.pairs.coord_a)  # bottom-up: entry i belongs to hier_features[L - 1 - i]
    L = len(touched)
    outside = 0
    for lvl in range(L):
        g, flag = got[1][lvl], touched[lvl].bool()
        rows = g.shape[0] - 1  # (the trash row carries no flag: the tail steps it with the decoder units)
        has = g[:rows].ne(0).any(dim=1)
        assert bool(flag[:rows][has].all()), "a row holds gradient and is not flagged (level %d)" % lvl
        assert set(touched[lvl].unique().tolist()) <= {0, 1}
        own = torch.zeros(rows + 1, dtype=torch.bool)
        ids = base_rows[L - 1 - lvl].flatten()
        own[ids[ids >= 0]] = True
        outside += int((flag[:rows].cpu() & ~own[:rows]).sum())
    print("flagged rows outside the base points' own corners:", outside)
    assert outside > 0  # the shifted points reach rows the batch's own points do not


# ---- 8. pool mode, both record layouts
@pytest.mark.parametrize("L", [3, 4])
def test_pool_mode_reads_the_records(L):
    from shine_mapping_amd import synth
    from shine_mapping_amd.sampler import SortedPool

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L)
    pl = wl.pool
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=3)
    assert pool.rec is not None and (pool._weight_sep is None) == (L < 4)
    n, k = 1000, 500
    idx = pool.draw(n)
    coord, _, _ = pool.get_batch(idx)
    coord = coord.contiguous()
    gen = torch.Generator(device="cuda").manual_seed(13)
    near = torch.randint(0, n, (k,), generator=gen, device="cuda")
    cell = wl.cfg.leaf_vox_size * wl.cfg.scale
    shift = (torch.rand(k, 3, generator=gen, device="cuda") * 2 - 1) * (0.5 * cell)
    a = coord[near]
    _, ga, gb = _composite(wl.octree, wl.decoder, a, (a + shift).contiguous())
    keep = _well_conditioned(ga, gb)
    assert int((~keep).sum()) <= k // 100
    near, shift = near[keep].to(torch.int32).contiguous(), shift[keep].contiguous()
    got = _fused(wl.octree, wl.decoder, None, near, shift, pool=pool, idx=idx)
    plain = _fused(wl.octree, wl.decoder, coord, near, shift)
    assert torch.equal(got[0], plain[0]) and all(torch.equal(x, y) for x, y in zip(got[2], plain[2])), L
    for x, y in zip(got[1], plain[1]):
        assert rel_err(x, y) <= TOL, (L, rel_err(x, y))
    a = coord[near.long()]
    ref, _, _ = _composite(wl.octree, wl.decoder, a, (a + shift).contiguous())
    _check("pool L=%d" % L, got, ref)


# ---- 9. determinism, accumulation, grad_buffers, the frozen decoder, the workspace
def test_determinism_accumulation_buffers_frozen_decoder_and_workspace():
    from shine_mapping_amd import _lib, autograd_ops, ops

    c = co.case("maicity_bce_L4")
    _, octree, dec = product_from_golden(c.fx)
    coord, near, shift = _dev(c)
    runs = [_fused(octree, dec, coord, near, shift) for _ in range(3)]
    a = runs[0]
    for b in runs[1:]:
        assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    # a second call doubles the grads
    _clear(octree, dec)
    ws = _lib.zeroed_workspace(autograd_ops.CONSISTENCY_WORKSPACE_BYTES, coord.device)
    ops.fused_consistency_step(octree, dec, coord, WC, near, shift, workspace=ws)
    ops.fused_consistency_step(octree, dec, coord, WC, near, shift, workspace=ws)
    params = list(octree.hier_features) + list(dec.fused_params())
    for k, (p, r) in enumerate(zip(params, a[1] + a[2])):
        assert float((p.grad - 2 * r).abs().max()) <= TOL * float(r.abs().max()) or float(r.abs().max()) == 0.0, k
    assert not bool(ws.any()), "the workspace is all zero after a call"
    # grad_buffers: the same numbers land in the buffers, .grad stays as it is
    kept = [p.grad.clone() for p in params]
    bufs = ([torch.zeros_like(p) for p in octree.hier_features], [torch.zeros_like(p) for p in dec.fused_params()])
    ops.fused_consistency_step(octree, dec, coord, WC, near, shift, grad_buffers=bufs)
    assert all(torch.equal(p.grad, k) for p, k in zip(params, kept))
    assert all(torch.equal(x, y) for x, y in zip(bufs[1], a[2]))
    for x, y in zip(bufs[0], a[1]):
        assert rel_err(x, y) <= TOL
    _clear(octree, dec)
    # a decoder that is neither trained nor frozen is refused; a frozen one gets no gradient and the same feature grads
    dec.fused_params()[2].requires_grad_(False)
    with pytest.raises(ValueError, match="all require grad or all be frozen"):
        ops.fused_consistency_step(octree, dec, coord, WC, near, shift)
    for p in dec.parameters():
        p.requires_grad_(False)
    guard = [p.detach().clone() for p in dec.parameters()]
    _clear(octree, dec)
    loss = ops.fused_consistency_step(octree, dec, coord, WC, near, shift)
    assert all(p.grad is None for p in dec.parameters())
    assert all(torch.equal(p, g) for p, g in zip(dec.parameters(), guard))
    assert torch.equal(loss, a[0])
    for p, r in zip(octree.hier_features, a[1]):
        assert rel_err(p.grad, r) <= TOL
    _clear(octree, dec)
    for bad in (dict(out=torch.zeros(2, device="cuda")), dict(idx=torch.zeros(4, dtype=torch.int64, device="cuda")),
                dict(n_pairs=3), dict(draws_out=(near[:5], shift[:5])), dict(touched=[torch.zeros(4, device="cuda")])):
        with pytest.raises(ValueError):
            ops.fused_consistency_step(octree, dec, coord, WC, near, shift, **bad)
    with pytest.raises(ValueError, match="shift"):
        ops.fused_consistency_step(octree, dec, coord, WC, near, shift[:, :2].contiguous())
    with pytest.raises(ValueError, match="near_index"):
        ops.fused_consistency_step(octree, dec, coord, WC, near.long(), shift)
    with pytest.raises(ValueError, match="no batch row"):
        ops.fused_consistency_step(octree, dec, coord[:0], WC, near, shift)
    assert all(p.grad is None or not bool(p.grad.any()) for p in octree.hier_features)  # (refused before any launch)


# ---- 10. the loop
ITERS = 12
N = 4096
K_LOOP = 1000
W_LOOP = 0.2


@pytest.fixture(scope="module")
def workload():
    from shine_mapping_amd import synth

    return synth.build_workload("maicity", frames=12, beams=32, azimuths=180, device="cuda", seed=7)


@pytest.fixture(scope="module")
def loop_start(workload):
    """every parameter's start; one eager iteration has run on the device afterwards"""
    wl = workload
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters())]
    cfg, _, pool = _loop_parts(wl, start)
    it = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True))
    assert it.ran_eager and not it.native and float(it.consistency_loss) > 0
    return start


def _term(wl):
    from shine_mapping_amd.loop import ConsistencyTerm

    return ConsistencyTerm(W_LOOP, K_LOOP, 0.5 * wl.cfg.leaf_vox_size * wl.cfg.scale, seed=17)


def _loop_parts(wl, start, seed=11, normal=None):
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
    kw = dict(normal_label=normal) if normal is not None else {}
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=seed, canonical=True, **kw)
    return cfg, params, pool


def _make_opt(cfg, wl, hip):
    from shine_mapping_amd import optim

    feats = list(wl.octree.parameters())
    if hip:
        return optim.setup_optimizer(cfg, feats, wl.decoder.fused_params())
    groups = [{"params": wl.decoder.fused_params(), "lr": cfg.lr, "weight_decay": cfg.weight_decay}]
    groups += [{"params": feats[cfg.tree_level_feat - i - 1], "lr": cfg.lr} for i in range(cfg.tree_level_feat)]
    return torch.optim.Adam(groups, betas=(0.9, 0.99), eps=cfg.adam_eps)


def _graphed(cfg, wl, pool, opt, normal=False, **kw):
    from shine_mapping_amd import StepOptions
    from shine_mapping_amd.loop import GraphedIteration, NormalTerm

    if normal:
        kw["normal"] = NormalTerm(0.05)
    return GraphedIteration(wl.octree, wl.decoder, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid), N, consistency=_term(wl), **kw)


def _eager_replay(cfg, wl, pool, params, batches, draws, normal=False):
    """{fused_train_step, [fused_normal_step,] fused_consistency_step on the recorded pairs, torch.optim.Adam} on the recorded draws"""
    from shine_mapping_amd import StepOptions, ops

    opt = _make_opt(cfg, wl, False)
    opts = StepOptions(sigma=cfg.sigma_sigmoid)
    losses, cons, normals = [], [], []
    for idx, (near, shift) in zip(batches, draws):
        coord, sdf_label, weight = pool.get_batch(idx)
        opt.zero_grad(set_to_none=True)
        loss, _, _ = ops.fused_train_step(wl.octree, wl.decoder, coord, sdf_label, weight, opts)
        if normal:
            lab = pool.normal_label[idx.long()].contiguous()
            normals.append(float(ops.fused_normal_step(wl.octree, wl.decoder, coord, weight, lab, 0.05)))
        cons.append(float(ops.fused_consistency_step(wl.octree, wl.decoder, coord.contiguous(), W_LOOP, near, shift)))
        opt.step()
        losses.append(float(loss))
    torch.cuda.synchronize()
    return losses, cons, normals


def _run_graphed(g, iters, feats):
    """`iters` single iterations -> batches, draws, losses; after EVERY iteration every feature .grad must be all zero (a row the
    term added gradient to and did not flag would keep it: the active-row tail neither steps nor clears an unflagged row)"""
    batches, draws, loss, cons = [], [], [], []
    leftover = torch.zeros((), dtype=torch.int64, device="cuda")
    for it in range(iters):
        batches.append(g._idx.clone())
        with counted_launches() as calls, consistency_calls() as seen:
            out = g()
        names = [c[0] for c in calls]
        if it == 0:  # this object's first call records the iteration
            assert names[0] == "shine_train_step" and names[-1] == "shine_finish_iteration" and len(seen) == 1, (names, len(seen))
            assert seen[0][6] is None and seen[0][7] is None and seen[0][8] == K_LOOP and seen[0][5] == N  # drawn pairs
        else:
            assert names == [] and seen == []  # (a replay goes through no entry point)
        draws.append((g.consistency_draws[0].clone(), g.consistency_draws[1].clone()))
        loss.append(out.clone())
        cons.append(g.consistency_loss.clone())
        for p in feats:
            leftover += p.grad.ne(0).sum()
    torch.cuda.synchronize()
    return batches, draws, [float(x) for x in loss], [float(x) for x in cons], int(leftover)


@pytest.mark.parametrize("active_rows", [True, False])
def test_graphed_consistency_loop_matches_an_eager_replay(workload, loop_start, active_rows):
    wl = workload
    start = loop_start
    cfg, params, pool = _loop_parts(wl, start)
    g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True), eager_first=False, active_rows=active_rows)
    assert not g.ran_eager and not g.native and g.active_rows == active_rows and (g.touched is not None) == active_rows
    assert g.consistency_draws[0].shape == (K_LOOP,) and g.consistency_draws[1].shape == (K_LOOP, 3)
    feats = list(wl.octree.hier_features)
    batches, draws, hip_loss, hip_cons, leftover = _run_graphed(g, ITERS, feats)
    assert leftover == 0, "a feature gradient survived the tail: %d elements" % leftover
    assert int(g._consistency_state) == ITERS
    assert all(not torch.equal(draws[i][0], draws[i + 1][0]) for i in range(ITERS - 1))  # fresh pairs every iteration
    hip_params = [p.detach().clone() for p in params]
    cfg, params, _ = _loop_parts(wl, start)
    ref_loss, ref_cons, _ = _eager_replay(cfg, wl, pool, params, batches, draws)
    worst = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(hip_loss + hip_cons, ref_loss + ref_cons))
    errs = [rel_err(a, b) for a, b in zip(hip_params, params)]
    print("active_rows=%s worst loss %.2e" % (active_rows, worst), "params", " ".join("%.1e" % e for e in errs))
    print("consistency_loss %.4f -> %.4f" % (hip_cons[0], hip_cons[-1]))
    assert all(x == x for x in hip_cons) and worst <= LOOP_TOL["loss"], worst
    assert max(errs) <= LOOP_TOL["params"], errs
    _loop_parts(wl, start)


def test_unrolled_run_equals_single_calls(workload, loop_start):
    wl = workload
    start = loop_start
    K = 5
    out = []
    for unroll in (1, 2):
        cfg, params, pool = _loop_parts(wl, start)
        g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True), eager_first=False, unroll=unroll)
        if unroll == 1:
            for _ in range(K):
                g()
        else:
            g.run(K)  # 2 x 2 + 1
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for p in params], g._idx.clone(), float(g.consistency_loss), float(g.loss),
                    g.consistency_draws[0].clone(), int(g._consistency_state)))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][4], out[1][4])  # (the same batches and pairs were drawn)
    assert out[0][5] == out[1][5] == K
    errs = [rel_err(a, b) for a, b in zip(out[1][0], out[0][0])]
    print("unrolled vs single:", " ".join("%.1e" % e for e in errs), out[0][2:4], out[1][2:4])
    assert max(errs) <= TOL, errs
    assert abs(out[0][2] - out[1][2]) <= TOL * abs(out[0][2])
    _loop_parts(wl, start)


def test_normal_and_consistency_terms_together(workload, loop_start):
    from test_gpu_normal_step import _composite as normal_composite, _safe_labels, normal_calls

    wl = workload
    start = loop_start
    _loop_parts(wl, start)
    pl = wl.pool
    _, gpool = normal_composite(wl.octree, wl.decoder, pl.coord.contiguous(), pl.weight.contiguous(), torch.zeros_like(pl.coord))
    lab = _safe_labels(gpool, pl.weight, 31)
    cfg, params, pool = _loop_parts(wl, start, normal=lab)
    g = _graphed(cfg, wl, pool, _make_opt(cfg, wl, True), normal=True, eager_first=False)
    assert not g.ran_eager and not g.native
    feats = list(wl.octree.hier_features)
    with normal_calls() as normal_seen:
        batches, draws, hip_loss, hip_cons, leftover = _run_graphed(g, 6, feats)
    assert len(normal_seen) == 1 and leftover == 0  # {fused, normal, consistency, tail}, recorded once
    hip_normal = float(g.normal_loss)
    cfg, params, _ = _loop_parts(wl, start, normal=lab)
    ref_loss, ref_cons, ref_normal = _eager_replay(cfg, wl, pool, params, batches, draws, normal=True)
    worst = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(hip_loss + hip_cons + [hip_normal], ref_loss + ref_cons + ref_normal[-1:]))
    print("normal + consistency: worst loss %.2e" % worst)
    assert worst <= LOOP_TOL["loss"], worst
    _loop_parts(wl, start)


def test_all_three_terms_in_one_iteration(workload, loop_start):
    """{fused, sem, normal, consistency, tail, the head's Adam}: the recorded launches in that order, then losses and parameters
    against the eager replay of the loop's own batches and pairs"""
    from shine_mapping_amd import StepOptions, _lib, autograd_ops, ops
    from shine_mapping_amd.loop import GraphedIteration, NormalTerm, SemTerm
    from shine_mapping_amd.sampler import SortedPool
    from test_gpu_normal_step import _composite as normal_composite, _safe_labels
    from test_gpu_sem_step import C_LOOP, WEIGHT_S, _head, _labels, _make_opt as sem_opt

    wl, d, iters = workload, 3, 6
    _loop_parts(wl, loop_start)
    sem = _head(C_LOOP, seed=4)
    params = list(wl.octree.hier_features) + list(wl.decoder.parameters()) + list(sem.parameters())
    start = [p.detach().clone() for p in params]
    pl = wl.pool
    _, gpool = normal_composite(wl.octree, wl.decoder, pl.coord.contiguous(), pl.weight.contiguous(), torch.zeros_like(pl.coord))
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.semantic_on, cfg.ray_loss, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, True, False, 1.0
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=11, canonical=True, normal_label=_safe_labels(gpool, pl.weight, 31),
                      sem_label=_labels(pl.coord, pl.weight, C_LOOP), n_class=C_LOOP)
    opts = StepOptions(sigma=cfg.sigma_sigmoid)
    g = GraphedIteration(wl.octree, wl.decoder, pool, sem_opt(cfg, wl, sem, True), opts, N, eager_first=False,
                         sem=SemTerm(sem, WEIGHT_S, d), normal=NormalTerm(0.05), consistency=_term(wl))
    assert not g.ran_eager and not g.native and g.active_rows
    lib, extra = _lib.lib(), ("shine_normal_train_step", "shine_consistency_train_step")  # (beside counted_launches()' own)
    saved = {name: getattr(lib, name) for name in extra}
    batches, draws, hip = [], [], []
    leftover = torch.zeros((), dtype=torch.int64, device="cuda")
    for it in range(iters):
        batches.append(g._idx.clone())
        with counted_launches() as calls:
            try:
                for name, fn in saved.items():
                    setattr(lib, name, lambda *a, _fn=fn, _name=name: (calls.append((_name, a)), _fn(*a))[1])
                out = g()
            finally:
                for name, fn in saved.items():
                    setattr(lib, name, fn)
        names = [c[0] for c in calls]  # this object's first call records the iteration; a replay goes through no entry point
        assert names == (["shine_train_step", "shine_sem_train_step", "shine_normal_train_step", "shine_consistency_train_step",
                          "shine_finish_iteration", "shine_adam_step_dev"] if it == 0 else []), names
        draws.append((g.consistency_draws[0].clone(), g.consistency_draws[1].clone()))
        hip.append([x.clone() for x in (out, g.sem_loss, g.normal_loss, g.consistency_loss)])
        for p in wl.octree.hier_features:
            leftover += p.grad.ne(0).sum()
    torch.cuda.synchronize()
    assert int(leftover) == 0 and int(g._consistency_state) == iters
    hip = [[float(x) for x in row] for row in hip]
    hip_params = [p.detach().clone() for p in params]

    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
            p.grad = None
    autograd_ops.bump_param_epoch()
    opt = sem_opt(cfg, wl, sem, False)
    ref = []
    for idx, (near, shift) in zip(batches, draws):
        coord, sdf_label, weight = pool.get_batch(idx)
        coord, i = coord.contiguous(), idx.long()
        opt.zero_grad(set_to_none=True)
        loss, _, _ = ops.fused_train_step(wl.octree, wl.decoder, coord, sdf_label, weight, opts)
        sem_loss = ops.fused_sem_step(wl.octree, sem, coord, pool.sem_label[i].contiguous(), WEIGHT_S, d)
        normal_loss = ops.fused_normal_step(wl.octree, wl.decoder, coord, weight, pool.normal_label[i].contiguous(), 0.05)
        cons = ops.fused_consistency_step(wl.octree, wl.decoder, coord, W_LOOP, near, shift)
        ref.append([float(x) for x in (loss, sem_loss, normal_loss, cons)])
        opt.step()
    torch.cuda.synchronize()
    worst = max(abs(a - b) / max(abs(b), 1e-12) for ra, rb in zip(hip, ref) for a, b in zip(ra, rb))
    errs = [rel_err(a, b) for a, b in zip(hip_params, params)]
    print("sem + normal + consistency: worst loss %.2e" % worst, "params", " ".join("%.1e" % e for e in errs))
    print("fused / sem / normal / consistency losses, first and last:", hip[0], hip[-1])
    assert all(x > 0 for x in hip[0]) and worst <= LOOP_TOL["loss"], worst
    assert max(errs) <= LOOP_TOL["params"], errs
    _loop_parts(wl, loop_start)


def test_without_consistency_the_iteration_is_the_two_launch_native_graph(workload):
    from shine_mapping_amd import StepOptions, optim
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.sampler import SortedPool

    wl = workload
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters())]
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, 1.0
    opt = optim.setup_optimizer(cfg, list(wl.octree.parameters()), wl.decoder.fused_params())
    pool = SortedPool(wl.octree, wl.pool.coord, wl.pool.sdf_label, wl.pool.weight, seed=5)
    g = GraphedIteration(wl.octree, wl.decoder, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid), N, consistency=None)
    assert g.native and not g.ran_eager and g.consistency is None and g.consistency_loss is None and g.consistency_draws is None
    with counted_launches() as calls, consistency_calls() as seen:
        g()
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["shine_iter_graph_set_step", "shine_iter_graph_set_finish"] and seen == []
    assert g.graph is None and g.graph_k is None
    with torch.no_grad():
        for p, s in zip(list(wl.octree.hier_features) + list(wl.decoder.parameters()), start):
            p.copy_(s)
            p.grad = None
