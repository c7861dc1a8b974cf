"""GPU: the sdf_l1 / sdf_l2 and ray-rendering (dr, dr_neus) objectives on HIP (csrc/shine_loss_modes.hip) against the reference's
recorded values (tests/golden/loss_modes.pt), against torch composites at scale, and in the drivers' Tier A loop together with
the fused optimiser's learnable sigma_size group; then the sweeps on the CPU-generated inputs of tests/test_loss_modes.py: every
sample count 1..32 in both modes with tied depths and saturated rows, every launch shape of the two kernels, and the workspace
and ticket counter they share."""
import pytest
import torch

from test_loss_modes import (DIFF_SCALES, DIFF_SIZES, FIXTURE, LAUNCH_RAYS, LAUNCH_SAMPLES, SWEEP_RAYS, composite_diff,
                             composite_ray, diff_inputs, fp64_rows, grad_close, load_fixture, ray_distance, ray_inputs,
                             ray_reference, ray_sweep_case, saturated_rows)

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _paths():
    """the public entry point (the C++ node when the extension is loaded) and the Python autograd.Function"""
    from shine_mapping_amd import losses

    def ray_py(x, y, d, neus):
        return losses._RayRender.apply(x, y, d, neus, losses.loss_workspace(y.device))

    def diff_py(p, l, w, scale, l2):
        return losses._SdfDiff.apply(p, l, w, scale, l2, losses.loss_workspace(p.device))

    return [("public", losses.batch_ray_rendering_loss, losses.sdf_diff_loss), ("python", ray_py, diff_py)]


@pytest.mark.parametrize("path", [0, 1])
def test_ray_loss_matches_the_reference_fixture(path):
    name, ray, _ = _paths()[path]
    for case in load_fixture()["ray"]:
        x, d = case["x"].cuda(), case["d_meas"].cuda()
        y = case["y"].cuda().requires_grad_(True)
        loss = ray(x, y, d, case["neus"])
        if name == "public":
            assert "RayRender" in loss.grad_fn.name(), loss.grad_fn.name()
        loss.backward()
        ref = float(case["loss"])
        assert abs(float(loss.detach()) - ref) <= 1e-5 * abs(ref), (case["neus"], case["S"], float(loss.detach()), ref)
        assert torch.isfinite(y.grad).all()
        ok, worst = grad_close(y.grad.cpu(), case["grad_y"], 1e-4)
        assert ok, (name, case["neus"], case["S"], worst)


@pytest.mark.parametrize("path", [0, 1])
def test_diff_loss_matches_the_reference_fixture(path):
    name, _, diff = _paths()[path]
    for case in load_fixture()["sdf"]:
        p = case["pred"].cuda().requires_grad_(True)
        loss = diff(p, case["label"].cuda(), case["weight"].cuda(), case["scale"], case["l2"])
        if name == "public":
            assert "SdfDiff" in loss.grad_fn.name(), loss.grad_fn.name()
        loss.backward()
        ref = float(case["loss"])
        assert abs(float(loss.detach()) - ref) <= 1e-5 * abs(ref), (case["l2"], case["scale"], float(loss.detach()), ref)
        scale = max(1.0, float(case["grad_pred"].abs().max()))
        assert float((p.grad.cpu() - case["grad_pred"]).abs().max()) <= 1e-4 * scale


def _big_ray_batch(R, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(R, S, device="cuda", generator=g) * 20.0 + 0.5
    y = torch.sigmoid(torch.randn(R, S, device="cuda", generator=g) * 1.5)
    d = torch.rand(R, device="cuda", generator=g) * 20.0 + 0.5
    return x, y, d


@pytest.mark.parametrize("neus", [False, True])
def test_ray_loss_at_65k_rays_matches_the_composite(neus):
    from shine_mapping_amd.losses import batch_ray_rendering_loss

    x, y, d = _big_ray_batch(1 << 16, 9, 5 + int(neus))
    ya = y.clone().requires_grad_(True)
    yb = y.clone().requires_grad_(True)
    la = batch_ray_rendering_loss(x, ya, d, neus)
    lb = composite_ray(x, yb, d, neus)
    la.backward()
    lb.backward()
    assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(lb))
    R = y.shape[0]  # (per-ray units: the mean's 1 / R would put every gradient under the absolute floor of grad_close)
    ok, worst = grad_close(ya.grad.cpu() * R, yb.grad.cpu() * R, 1e-4)
    assert ok, worst


@pytest.mark.parametrize("l2", [False, True])
def test_diff_loss_at_1m_points_matches_the_composite(l2):
    from shine_mapping_amd.losses import sdf_diff_loss

    n = 1 << 20
    g = torch.Generator(device="cuda").manual_seed(9)
    pred = torch.randn(n, device="cuda", generator=g)
    label = torch.randn(n, device="cuda", generator=g)
    weight = torch.rand(n, device="cuda", generator=g)
    label[::5] = pred[::5]
    scale = 0.0390625
    pa, pb = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    la = sdf_diff_loss(pa, label, weight, scale, l2)
    lb = composite_diff(pb, label, weight, scale, l2)
    la.backward()
    lb.backward()
    assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(lb))
    assert rel_err(pa.grad, pb.grad) <= 1e-5


def test_repeated_calls_are_bit_identical():
    from shine_mapping_amd.losses import batch_ray_rendering_loss, sdf_diff_loss

    for R in (100, 4096, (1 << 20) + 3):
        x, y, d = _big_ray_batch(R, 6, R)
        outs = []
        for _ in range(3):
            yy = y.clone().requires_grad_(True)
            loss = batch_ray_rendering_loss(x, yy, d, True)
            loss.backward()
            outs.append((loss.detach().clone(), yy.grad.clone()))
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), R
    for n in (1, 4096, (1 << 20) + 17):
        p = torch.randn(n, device="cuda")
        l, w = torch.randn(n, device="cuda"), torch.rand(n, device="cuda")
        outs = []
        for _ in range(3):
            pp = p.clone().requires_grad_(True)
            loss = sdf_diff_loss(pp, l, w, 0.1, n % 2 == 0)
            loss.backward()
            outs.append((loss.detach().clone(), pp.grad.clone()))
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), n


def test_upstream_gradient_other_than_one():
    from shine_mapping_amd.losses import batch_ray_rendering_loss, sdf_diff_loss

    x, y, d = _big_ray_batch(4096, 9, 1)
    ya, yb = y.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (batch_ray_rendering_loss(x, ya, d, False) * 3.5).backward()
    batch_ray_rendering_loss(x, yb, d, False).backward()
    assert torch.equal(ya.grad, yb.grad * 3.5)
    p = torch.randn(4096, device="cuda")
    l, w = torch.randn(4096, device="cuda"), torch.rand(4096, device="cuda")
    pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
    (sdf_diff_loss(pa, l, w, 0.2, True) * -0.25).backward()
    sdf_diff_loss(pb, l, w, 0.2, True).backward()
    assert torch.equal(pa.grad, pb.grad * -0.25)


def test_fallbacks_run_the_composite():
    """S = 33 (beyond the kernel's register rows), CPU tensors and float64 run the composite: the same results as it"""
    from shine_mapping_amd.losses import batch_ray_rendering_loss, sdf_diff_loss

    for dev, dt, S in (("cuda", torch.float32, 33), ("cpu", torch.float32, 9), ("cuda", torch.float64, 9)):
        x, y, d = _big_ray_batch(256, S, 3)
        x, y, d = x.to(dev, dt), y.to(dev, dt), d.to(dev, dt)
        for neus in (False, True):
            ya, yb = y.clone().requires_grad_(True), y.clone().requires_grad_(True)
            la, lb = batch_ray_rendering_loss(x, ya, d, neus), composite_ray(x, yb, d, neus)
            assert "RayRender" not in la.grad_fn.name()
            la.backward()
            lb.backward()
            assert torch.equal(la, lb) and torch.equal(ya.grad, yb.grad), (dev, dt, S, neus)
        if dev == "cuda" and dt == torch.float32:
            continue  # (the point loss has no sample-count limit)
        p = torch.randn(300, device=dev, dtype=dt)
        l, w = torch.randn(300, device=dev, dtype=dt), torch.rand(300, device=dev, dtype=dt)
        pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
        la, lb = sdf_diff_loss(pa, l, w, 0.1, False), composite_diff(pb, l, w, 0.1, False)
        assert "SdfDiff" not in la.grad_fn.name()
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(pa.grad, pb.grad), (dev, dt)
    # a label that needs a gradient is the composite too
    p = torch.randn(64, device="cuda", requires_grad=True)
    l = torch.randn(64, device="cuda", requires_grad=True)
    loss = sdf_diff_loss(p, l, torch.rand(64, device="cuda"), 0.1, True)
    assert "SdfDiff" not in loss.grad_fn.name()


def _sigma_groups(t, lr):
    """utils/tools.py:57-83's layout with ray_loss: decoder (L2), feature levels leaf first, then sigma_size"""
    return [{"params": t[:6], "lr": lr, "weight_decay": 1e-7}, {"params": [t[8]], "lr": lr}, {"params": [t[7]], "lr": lr},
            {"params": [t[6]], "lr": lr}, {"params": t[9], "lr": lr}]


def test_fused_adam_with_the_sigma_group_matches_torch_adam():
    from types import SimpleNamespace

    from shine_mapping_amd.optim import FusedAdam, setup_optimizer

    g = torch.Generator().manual_seed(21)
    shapes = [(32, 8), (32,), (32, 32), (32,), (1, 32), (1,), (1001, 8), (4003, 8), (16385, 8), (1,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in shapes]
    ps[9].data.fill_(1.0)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    cfg = SimpleNamespace(lr=0.01, weight_decay=1e-7, tree_level_feat=3, lr_level_reduce_ratio=1.0, adam_eps=1e-15,
                          opt_adam=True, semantic_on=False, ray_loss=True)
    opt = setup_optimizer(cfg, ps[6:9], ps[:6], None, ps[9])
    assert isinstance(opt, FusedAdam) and len(opt.param_groups) == 5
    assert opt.param_groups[-1]["params"][0] is ps[9] and opt.param_groups[-1]["weight_decay"] == 0.0
    ref = torch.optim.Adam(_sigma_groups(qs, 0.01), betas=(0.9, 0.99), eps=1e-15)
    worst = 0.0
    for it in range(10):
        if it == 5:  # step_lr_decay (utils/tools.py:135-155) on every group, then the device copy
            for o in (opt, ref):
                for grp in o.param_groups:
                    grp["lr"] *= 0.5
            opt.sync_lr()
        for p, q in zip(ps, qs):
            gr = torch.randn(p.shape, generator=g).cuda()
            p.grad, q.grad = gr.clone(), gr.clone()
        opt.step()
        ref.step()
        for p, q in zip(ps, qs):
            worst = max(worst, rel_err(p, q))
    # the decoder / feature groups are held to torch.optim.Adam as in the fused optimiser's own parity test; the sigma group is
    # one more group of the same launch
    assert worst <= 2e-6, worst
    # the extra group round-trips through torch.optim.Adam's state_dict layout
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 5 and sd["param_groups"][-1]["params"] == [9] and float(sd["state"][9]["step"]) == 10.0
    other = torch.optim.Adam(_sigma_groups([torch.nn.Parameter(p.detach().clone()) for p in ps], 0.01), betas=(0.9, 0.99),
                             eps=1e-15)
    other.load_state_dict(sd)
    back = setup_optimizer(cfg, ps[6:9], ps[:6], None, ps[9])
    back.load_state_dict(ref.state_dict())
    assert back.param_groups[-1]["lr"] == 0.005 and back.step_count == 10
    assert torch.equal(back.state[ps[9]][0].cpu(), ref.state[qs[9]]["exp_avg"].cpu())


# ---- the drivers' Tier A loop (shine_batch.py:115-209, ray and point branches) on the drop-in's classes

ITERS = 30
LOOP_TOL = dict(loss=2e-3, sigma=2e-3, params=2e-2)  # HIP losses + FusedAdam vs composites + torch.optim.Adam after 30 steps


@pytest.fixture(scope="module")
def workload():
    from shine_mapping_amd import synth

    wl = synth.build_workload("maicity", frames=12, beams=32, azimuths=180, device="cuda", seed=7)
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters())]
    return wl, start


def _loop(wl, start, mode, eik, hip):
    import copy

    from shine_mapping_amd import autograd_ops, get_gradient, losses, optim, synth

    cfg = copy.copy(wl.cfg)
    cfg.ray_loss = mode in ("dr", "dr_neus")
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.semantic_on, cfg.weight_e = 0.01, 1e-15, True, False, 0.1
    cfg.lr_level_reduce_ratio = 1.0
    octree, dec = wl.octree, wl.decoder
    params = list(octree.hier_features) + list(dec.parameters())
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
            p.grad = None
    autograd_ops.bump_param_epoch()
    sigma_size = torch.nn.Parameter(torch.ones(1, device="cuda"))
    sigma_sigmoid = cfg.sigma_sigmoid
    feats, geo = list(octree.parameters()), list(dec.parameters())
    if hip:
        opt = optim.setup_optimizer(cfg, feats, geo, None, sigma_size)
    else:
        groups = [{"params": geo, "lr": cfg.lr, "weight_decay": cfg.weight_decay}]
        groups += [{"params": feats[cfg.tree_level_feat - i - 1], "lr": cfg.lr} for i in range(cfg.tree_level_feat)]
        if cfg.ray_loss:
            groups.append({"params": sigma_size, "lr": cfg.lr})
        opt = torch.optim.Adam(groups, betas=(0.9, 0.99), eps=cfg.adam_eps)
    S = cfg.surface_sample_n + cfg.free_sample_n
    pts = wl.pool.coord[wl.pool.weight > 0]
    origin = pts.mean(0) + torch.tensor([0.0, 0.0, 1.8 * cfg.scale], device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(11)
    bs = 512
    losses_seen = []
    for it in range(ITERS):
        if it == ITERS // 2:
            for grp in opt.param_groups:
                grp["lr"] *= 0.5
            if hip:
                opt.sync_lr()
        if cfg.ray_loss:
            hit = pts[torch.randint(0, pts.shape[0], (bs,), device="cuda", generator=gen)]
            coord, _, _ = synth.sample_rays(hit, origin, cfg, gen)
            sample_depth = (coord - origin).norm(dim=1)
            ray_depth = (hit - origin).norm(dim=1)
            weight = torch.ones(coord.shape[0], device="cuda")
            weight.view(bs, S)[:, cfg.surface_sample_n:] = -1.0
        else:
            coord, sdf_label, weight = synth.draw_batch(wl.pool, bs * S, gen)
        if eik:
            coord.requires_grad_(True)
        pred = dec.sdf(octree.query_feature(coord))
        surface_mask = weight > 0
        if eik:
            g = get_gradient(coord, pred) * sigma_sigmoid
        cur_loss = 0.0
        if cfg.ray_loss:
            pred_ray = torch.sigmoid(pred / sigma_size).reshape(bs, -1)
            fn = losses.batch_ray_rendering_loss if hip else composite_ray
            cur_loss = cur_loss + fn(sample_depth.reshape(bs, -1), pred_ray, ray_depth, mode == "dr_neus")
        else:
            fn = losses.sdf_diff_loss if hip else composite_diff
            cur_loss = cur_loss + fn(pred, sdf_label, torch.abs(weight), cfg.scale, mode == "sdf_l2")
        if eik:
            cur_loss = cur_loss + cfg.weight_e * ((1.0 - g[surface_mask].norm(2, dim=-1)) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        cur_loss.backward()
        opt.step()
        losses_seen.append(float(cur_loss))
    torch.cuda.synchronize()
    return losses_seen, float(sigma_size), [p.detach().clone() for p in params]


@pytest.mark.parametrize("eik", [False, True])
@pytest.mark.parametrize("mode", ["dr", "dr_neus", "sdf_l1", "sdf_l2"])
def test_tier_a_loop_with_hip_losses_matches_the_composites(workload, mode, eik):
    from shine_mapping_amd import autograd_ops

    wl, start = workload
    autograd_ops.FUSE_WITH_COORD_GRAD = True  # (what the drop-in installs with get_gradient)
    try:
        hip = _loop(wl, start, mode, eik, True)
        ref = _loop(wl, start, mode, eik, False)
    finally:
        autograd_ops.FUSE_WITH_COORD_GRAD = False
    worst_loss = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(hip[0], ref[0]))
    assert worst_loss <= LOOP_TOL["loss"], (mode, eik, worst_loss)
    if mode in ("dr", "dr_neus"):
        assert hip[1] != 1.0  # sigma_size is learned
        assert abs(hip[1] - ref[1]) <= LOOP_TOL["sigma"] * abs(ref[1]), (hip[1], ref[1])
    else:
        assert hip[1] == ref[1] == 1.0
    for a, b in zip(hip[2], ref[2]):
        assert rel_err(a, b) <= LOOP_TOL["params"], (mode, eik, rel_err(a, b))


def test_fixture_is_present():
    import os

    assert os.path.isfile(FIXTURE)


# ---- sweeps: the inputs come from tests/test_loss_modes.py's CPU generators (their conditions are asserted there)

BOUND_FACTOR = 4.0  # x e_ref (test_gpu_dataset.py): two correct fp32 evaluations in different operation orders each sit within
# ~e_ref of exact; e_ref = the float32 composite's own distance to its float64 evaluation over the same rows


def _ray(fn, x, y, d, neus):
    """(loss, d loss / d y) of one call, on the host"""
    yy = y.detach().clone().cuda().requires_grad_(True)
    loss = fn(x.cuda(), yy, d.cuda(), neus)
    loss.backward()
    return loss.detach().cpu(), yy.grad.cpu()


def _assert_ray_matches_a(what, loss, g, loss_a, ga):
    """the fixture tests' bounds against the float32 composite: loss 1e-5 relative, grad_close(. R, . R, 1e-4), finite"""
    R = g.shape[0]
    ok, worst = grad_close(g * R, ga * R, 1e-4)
    rel = abs(float(loss) - float(loss_a)) / abs(float(loss_a))
    print("%s  vs float32 composite: loss rel %.2e  grad distance %.2e" % (what, rel, worst))
    assert torch.isfinite(g).all(), what
    assert rel <= 1e-5, (what, float(loss), float(loss_a))
    assert ok, (what, worst)


@pytest.mark.parametrize("neus", [False, True])
@pytest.mark.parametrize("S", range(1, 33))
def test_every_sample_count_matches_the_float32_and_float64_composites(S, neus):
    x, y, d = ray_sweep_case(S, neus)
    loss_a, ga = ray_reference(x, y, d, neus, torch.float32)  # A: what the fixture pins to the reference; every row
    _, gb = ray_reference(x, y, d, neus, torch.float64)  # B: the rows an fp64 evaluation can judge
    rows = fp64_rows(y, S >= 2)
    e_ref = ray_distance(ga, gb, rows)
    if S >= 2:  # another order of row 0's probabilities: its depths are all equal, so the column order alone decides
        yp = y.clone()
        yp[0] = y[0].flip(0)
        loss_ap, gap = ray_reference(x, yp, d, neus, torch.float32)
    # (row 5, all zeros, is what pins the backward loop's `k < A` guard with dr_neus at every S below the network's width: the
    # last sample's quotient against the padding column behind it is 0 / 1, inside the clamp, and would put -gd x into its column)
    for name, ray, _ in _paths():
        what = "S=%d neus=%d R=%d %s" % (S, neus, SWEEP_RAYS, name)
        loss, g = _ray(ray, x, y, d, neus)
        assert g.shape == (SWEEP_RAYS, S)
        dist = ray_distance(g, gb, rows)
        print("%s  vs float64 composite over %d unsaturated rows: kernel %.3e  e_ref %.3e  bound %.3e"
              % (what, int(rows.sum()), dist, e_ref, BOUND_FACTOR * e_ref))
        _assert_ray_matches_a(what, loss, g, loss_a, ga)
        assert dist <= BOUND_FACTOR * e_ref, (what, dist, e_ref)
        if S == 1 and neus:  # no alpha at all
            assert float(g.abs().max()) == 0.0, what
        if S >= 2:
            loss_p, gp = _ray(ray, x, yp, d, neus)
            _assert_ray_matches_a(what + " row 0 flipped", loss_p, gp, loss_ap, gap)
            assert torch.equal(gp[1:], g[1:]), what  # (nothing else moves)


@pytest.mark.parametrize("S", LAUNCH_SAMPLES)
@pytest.mark.parametrize("R", LAUNCH_RAYS)
def test_ray_loss_at_every_launch_shape(R, S):
    x, y, d = ray_inputs(R, S, 2000 + S)
    assert not saturated_rows(y).any()
    for neus in (False, True):
        loss_a, ga = ray_reference(x, y, d, neus, torch.float32)
        for name, ray, _ in _paths():
            loss, g = _ray(ray, x, y, d, neus)
            _assert_ray_matches_a("R=%d S=%d neus=%d %s" % (R, S, neus, name), loss, g, loss_a, ga)


def _raw_diff_loss(p, l, w, scale, l2):
    """shine_sdf_diff_loss through ctypes without the gradient output: the loss alone"""
    from shine_mapping_amd import _lib, losses

    out = torch.empty(1, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().shine_sdf_diff_loss(p.data_ptr(), l.data_ptr(), w.data_ptr(), p.shape[0], float(scale), 1 if l2 else 0,
                                              out.data_ptr(), None, losses.loss_workspace(p.device).data_ptr(),
                                              _lib.current_stream_handle()), "shine_sdf_diff_loss")
    return out[0]


@pytest.mark.parametrize("n", DIFF_SIZES)
def test_diff_loss_at_every_launch_shape(n):
    pred, label, weight = diff_inputs(n, 3000 + n)
    pc, lc, wc = pred.cuda(), label.cuda(), weight.cuda()
    for l2 in (False, True):
        for scale in DIFF_SCALES:
            pb = pred.double().requires_grad_(True)
            lb = composite_diff(pb, label.double(), weight.double(), scale, l2)
            lb.backward()
            for name, _, diff in _paths():
                what = "n=%d l2=%d scale=%g %s" % (n, l2, scale, name)
                pa = pc.clone().requires_grad_(True)
                la = diff(pa, lc, wc, scale, l2)
                la.backward()
                rel = abs(float(la) - float(lb)) / abs(float(lb))
                err = rel_err(pa.grad, pb.grad)
                print("%s  loss rel %.2e  grad rel_err %.2e" % (what, rel, err))
                assert rel <= 1e-5, (what, float(la), float(lb))
                assert err <= 1e-5, (what, err)
                # a label equal to the prediction: sgn(0) = 0 (l1), 2 * 0 (l2); a zero weight: no gradient either
                assert not bool(pa.grad[1::5].any()) and not bool(pa.grad[1::7].any()), what
                assert bool((pa.grad[::35] != 0).all()), what  # (a difference and a weight: a gradient, at n = 1 too)
                assert torch.equal(_raw_diff_loss(pc, lc, wc, scale, l2), la.detach()), what


def test_ray_and_point_losses_share_one_workspace():
    """the two kernels share loss_workspace(device) and its ticket counter: a sequence of launches of both, with one and with
    1024 workgroups, gives on the shared workspace what each call gives on a freshly zeroed one"""
    from shine_mapping_amd import losses

    big_r, big_n = LAUNCH_RAYS[6], DIFF_SIZES[8]
    rays = {R: tuple(t.cuda() for t in ray_inputs(R, S, 2000 + S)) for R, S in ((big_r, 17), (1, 8))}
    pts = {n: tuple(t.cuda() for t in diff_inputs(n, 3000 + n)) for n in (1, big_n)}
    sequence = [("ray", big_r, True), ("diff", 1, False), ("ray", 1, False), ("diff", big_n, True), ("ray", big_r, True)]

    def call(kind, size, flag, ray, diff):
        if kind == "ray":
            x, y, d = rays[size]
            yy = y.clone().requires_grad_(True)
            loss = ray(x, yy, d, flag)
            loss.backward()
            return loss.detach().clone(), yy.grad.clone()
        p, l, w = pts[size]
        pp = p.clone().requires_grad_(True)
        loss = diff(pp, l, w, DIFF_SCALES[0], flag)
        loss.backward()
        return loss.detach().clone(), pp.grad.clone()

    def fresh_ray(x, y, d, neus):
        return losses._RayRender.apply(x, y, d, neus, torch.zeros(losses.LOSS_WORKSPACE_BYTES // 8, dtype=torch.float64, device="cuda"))

    def fresh_diff(p, l, w, scale, l2):
        return losses._SdfDiff.apply(p, l, w, scale, l2, torch.zeros(losses.LOSS_WORKSPACE_BYTES // 8, dtype=torch.float64,
                                                                   device="cuda"))

    want = [call(kind, size, flag, fresh_ray, fresh_diff) for kind, size, flag in sequence]
    for name, ray, diff in _paths():
        got = [call(kind, size, flag, ray, diff) for kind, size, flag in sequence]
        for step, (a, b) in enumerate(zip(got, want)):
            assert torch.isfinite(a[0]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (name, step, sequence[step])
    assert not bool(losses.loss_workspace(torch.device("cuda"))[1024:].view(torch.int64).any())  # (the counter is back at zero)
