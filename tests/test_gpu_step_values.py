"""GPU suite (-m gpu), part 4: the SDF step on trained-map VALUES (tests/step_value_cases.py): dead units, dead points next to
live ones, pre-activations exactly on ReLU's kink, saturated logits with and without sample weights — through every form
tests/test_gpu_edges.py runs its edge batches through, on the fixtures' own batches (n <= 2048).

(1) Every run: everything returned is finite; the cases' exact claims (tests/test_step_values.py asserts them on the oracles)
hold on the device; values against the fp32 oracle and the wide oracle under the suite's standing policy (test_gpu_edges._check,
TOL), pred held to TOL x max(1, max |reference pred|).
(2) delta per point.  Every gradient comparison of (1) divides by the tensor's largest entry, and a saturated sample's delta
vanishes next to a near-surface sample's.  With a ONE-point batch d loss / d b3 IS that point's delta: b3 is written in place so
that the logit lands on each of step_value_cases.Y_TARGETS, for each label of LABEL_OVER_SIGMA, and d b3 and the loss are held to
bounds from the formats (step_value_cases.delta_ratios) against fp64 at the device's own prediction.  The worst ratio to the
bound is printed per form before it is asserted (profiles/step_value_cases_gpu.txt keeps the measured ones).
"""
import numpy as np
import pytest
import torch

import step_value_cases as sv
from conftest import product_from_golden
from test_gpu_edges import _fixture
from test_gpu_parity import step_options
from test_gpu_scale_parity import node_name

pytestmark = pytest.mark.gpu

CASES = [(n, k) for n in sv.FIXTURES for k in sv.KINDS]


def _product(name, case):
    return sv.apply_to_product(case, product_from_golden(_fixture(name)))


def _options(fx, case, variant=0):
    opts = step_options(fx)
    opts.kernel_variant = variant
    opts.loss_weight_on = case.loss_weight_on
    return opts


def _step_run(octree, dec, loss, pred, g, eik):
    parts = loss._base  # the step's four doubles: BCE, eikonal, count, total (ops._fused_launch)
    return dict(loss=loss, pred=pred, g=g, feat_grads=[p.grad for p in octree.hier_features],
                mlp_grads=[p.grad for p in dec.fused_params()], eikonal=parts[1] if eik else None)


@pytest.mark.parametrize("name,kind", CASES)
def test_value_case_fused_step_every_form(name, kind):
    """fused_train_step: the product kernel unplanned and planned, the check library's lane-per-point kernel (variant 1), the far
    (5) and near (6) builds planned, and the pool-record step with the whole batch drawn.  (The far build exists for full-chip
    launches only: at these sizes 5 and 6 check that forcing either reaches a kernel that computes the same.)"""
    from shine_mapping_amd import dp, fused_train_step
    from shine_mapping_amd.sampler import SortedPool

    fx = _fixture(name)
    case, ref, wide, mlp64 = sv.oracles(name, kind)
    eik = sv.is_eikonal(fx)
    coord, label, weight = fx["coord"].cuda(), case.sdf_label.cuda(), case.weight.cuda()
    n = coord.shape[0]
    for variant, planned in ((0, False), (0, True), (1, False), (1, True), (5, True), (6, True)):
        cfg, octree, dec = _product(name, case)
        kw = {}
        if planned:
            perm, slots = dp.plan_batch(octree, coord)
            kw = dict(perm=perm, slots=slots)
        loss, pred, g = fused_train_step(octree, dec, coord, label, weight, _options(fx, case, variant), want_grad_x=True, **kw)
        torch.cuda.synchronize()
        sv.check_run("%s %s: step v%d %s" % (name, kind, variant, "planned" if planned else "unplanned"), case, ref, wide, mlp64,
                     _step_run(octree, dec, loss, pred, g, eik))
        assert all(float(p[-1].abs().max()) == 0.0 for p in octree.hier_features)  # set_zero

    cfg, octree, dec = _product(name, case)
    octree._require_tables(with_ranks=True)
    sp = SortedPool(octree, coord, label, weight, seed=5)
    order = sp.perm.cpu().long()
    assert torch.equal(torch.sort(order).values, torch.arange(n))
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    loss, pred, g = fused_train_step(octree, dec, None, None, None, _options(fx, case), want_grad_x=True, pool=sp, idx=idx)
    torch.cuda.synchronize()
    sv.check_run("%s %s: pool-record step" % (name, kind), case, ref, wide, mlp64, _step_run(octree, dec, loss, pred, g, eik),
                 order=order)


@pytest.mark.parametrize("name,kind", CASES)
def test_value_case_autograd_entry_points(name, kind):
    """The three Tier A loops of test_gpu_edges.test_edge_autograd_entry_points (the fused node, the split nodes, the Python
    OctreeInterp), the eikonal term through get_gradient, each with the reference's loss."""
    from shine_mapping_amd import autograd_ops, get_gradient, sdf_bce_loss

    fx = _fixture(name)
    case, ref, wide, mlp64 = sv.oracles(name, kind)
    sigma, c = fx["sigma"], fx["cfg"]
    eik = sv.is_eikonal(fx)
    label, weight = case.sdf_label.cuda(), case.weight.cuda()
    red = c.get("loss_reduction", "mean")
    for mode in ("fused", "split", "python node"):
        autograd_ops.FUSE_WITH_COORD_GRAD = mode == "fused"
        try:
            cfg, octree, dec = _product(name, case)
            coord = fx["coord"].cuda().requires_grad_(eik)
            if mode == "python node":
                feature = autograd_ops.OctreeInterp.apply(coord, octree, *octree.feature_list())
            else:
                feature = octree.query_feature(coord)
            if mode == "split":
                feature = feature * 1.0
            pred = dec.sdf(feature)
            assert ("FusedInterpSdf" in node_name(pred.grad_fn)) == (mode == "fused"), (mode, node_name(pred.grad_fn))
            loss = sdf_bce_loss(pred, label, sigma, torch.abs(weight), case.loss_weight_on, red)
            g = None
            if eik:
                g = get_gradient(coord, pred) * sigma
                loss = loss + c["weight_e"] * ((1.0 - g[weight > 0].norm(2, dim=-1)) ** 2).mean()
            loss.backward()
            torch.cuda.synchronize()
            assert all(float(p[-1].abs().max()) == 0.0 for p in octree.hier_features)
            run = dict(loss=loss.detach(), pred=pred.detach(), g=None if g is None else g.detach(),
                       feat_grads=[p.grad for p in octree.hier_features], mlp_grads=[p.grad for p in dec.fused_params()])
            # (the eikonal mean here is torch's own launch, sum x (1 / n): only the step's loss_parts are held to exactly 1)
            sv.check_run("%s %s: autograd %s" % (name, kind, mode), case, ref, wide, mlp64, run)
        finally:
            autograd_ops.FUSE_WITH_COORD_GRAD = False


@pytest.mark.parametrize("name,kind", CASES)
def test_value_case_forward_and_mesher(name, kind):
    """forward_sdf with d pred / d coord, and the mesher's query kernel (it returns -pred)"""
    from shine_mapping_amd import forward_sdf
    from shine_mapping_amd.mesher import query_points_device

    fx = _fixture(name)
    case, ref, wide, mlp64 = sv.oracles(name, kind)
    eik = sv.is_eikonal(fx)
    cfg, octree, dec = _product(name, case)
    coord = fx["coord"].cuda()
    out = forward_sdf(octree, dec, coord, want_feat=True, want_grad_x=True, sigma=fx["sigma"])
    sdf, _ = query_points_device(octree, dec, coord)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["feat"]).all()) and bool(torch.isfinite(out["grad_x"]).all())
    if case.zero_points is not None:
        assert float(out["feat"][case.zero_points.cuda()].abs().max()) == 0.0
        if kind == "dead_points":
            assert float(out["grad_x"][case.zero_points.cuda()].abs().max()) == 0.0
    sv.check_run("%s %s: forward_sdf" % (name, kind), case, ref, wide, mlp64,
                 dict(pred=out["pred"], g=out["grad_x"] if eik else None))
    if kind in ("dead", "on_kink") and not eik:  # (no reference g on the BCE fixture; the exact claims still hold)
        gx = out["grad_x"] if kind == "dead" else out["grad_x"][case.zero_points.cuda()]
        assert float(gx.abs().max()) == 0.0
    sv.check_run("%s %s: mesher" % (name, kind), case, ref, wide, mlp64, dict(pred=-sdf))


# ------------------------------------------------------------------------------------------------------- (2) delta per point


def _mapped_surface_point(fx):
    """the first surface sample of the batch with a node on every level"""
    hit = torch.stack([(t >= 0).all(1) for t in fx["out"]["indices"]], 1).all(1) & (fx["weight"] > 0)
    return int(torch.nonzero(hit).flatten()[0])


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", ["maicity_bce_L4", "kitti_eik_L3"])
def test_delta_of_one_point_over_the_logit_range(name, variant, weighted, reduction):
    """n = 1: d loss / d b3 is the point's delta and the BCE part of the loss its loss (mean and sum coincide at n = 1, and the
    eikonal term of the surface point does not depend on b3)."""
    from shine_mapping_amd import fused_train_step

    fx = _fixture(name)
    cfg, octree, dec = product_from_golden(fx)
    i = _mapped_surface_point(fx)
    coord = fx["coord"][i:i + 1].cuda()
    w = 3.0 if weighted else float(fx["weight"][i])
    weight = torch.tensor([w], device="cuda")
    sigma = fx["sigma"]
    opts = step_options(fx)
    opts.kernel_variant, opts.loss_weight_on, opts.loss_reduction = variant, weighted, reduction
    b3 = dec.fused_params()[5]

    def step(label):
        loss, pred, _ = fused_train_step(octree, dec, coord, label, weight, opts)
        out = pred.clone(), b3.grad.clone().reshape(()), loss._base[0].clone()
        b3.grad.zero_()
        return out

    with torch.no_grad():
        b3.zero_()  # in place: the kernels read the tensor where it is
    base = float(step(torch.zeros(1, device="cuda"))[0])
    ys, xs = sv.sweep_grid()
    labels = (xs * sigma).float()
    runs = []
    for y, lab in zip(ys.tolist(), labels):
        with torch.no_grad():
            b3.fill_(float(np.float32(y - base)))
        runs.append(step(lab.reshape(1).cuda()))
    torch.cuda.synchronize()
    pred = torch.cat([r[0] for r in runs]).cpu()
    db3 = torch.stack([r[1] for r in runs]).cpu()
    loss = torch.stack([r[2] for r in runs]).cpu()
    assert float((pred.double() - ys).abs().max()) <= 1e-4  # the logits landed on their targets
    sv.check_delta("%s v%d %s %s" % (name, variant, "|w| = 3" if weighted else "unweighted", reduction), pred, db3, loss, labels,
                   sigma, w if weighted else 1.0)


@pytest.mark.parametrize("weighted", [False, True])
def test_delta_per_point_of_the_one_launch_bce_loss(weighted):
    """losses.sdf_bce_loss (shine_bce_loss) on the same sweep: its per-point d loss / d pred in ONE call (sum reduction: no 1 / n),
    the loss per point from calls of one element each, mean and sum."""
    from shine_mapping_amd import losses

    sigma = _fixture("maicity_bce_L4")["sigma"]
    ys, xs = sv.sweep_grid()
    labels = (xs * sigma).float().cuda()
    w = 3.0 if weighted else 1.0
    wt = torch.full_like(labels, w)
    pred = ys.float().cuda().requires_grad_(True)
    total = losses.sdf_bce_loss(pred, labels, sigma, wt, weighted, "sum")
    total.backward()
    per_point = []
    for k in range(pred.shape[0]):
        red = "mean" if k % 2 else "sum"
        per_point.append(losses.sdf_bce_loss(pred.detach()[k:k + 1], labels[k:k + 1], sigma, wt[k:k + 1], weighted, red).detach())
    torch.cuda.synchronize()
    loss = torch.stack(per_point).cpu()
    sv.check_delta("sdf_bce_loss %s" % ("|w| = 3" if weighted else "unweighted"), pred.detach(), pred.grad, loss, labels, sigma, w)
    l64 = sv.delta_reference(pred, labels, sigma, w)[1]
    bound = float((8 * sv.U24 * w * ys.abs().clamp_min(1.0)).sum())  # the per-point bounds added up
    assert abs(float(total) - float(l64.sum())) <= bound
