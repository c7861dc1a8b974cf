"""GPU: the semantic head (csrc/shine_semantic.hip) — sem_label_prob, its backward and sem_label against the reference's recorded
values (tests/golden/semantic.pt), against an fp64 composite at 2^20 points, repeat determinism, the frozen decoder, the feature
gradient it shares with the fused query_feature -> sdf node, the drivers' Tier A loop with the fused optimiser's semantic group,
and the mesher's label query."""
import copy

import numpy as np
import pytest
import torch

from test_semantic import SEM_NAMES, decoder_from_case, load_fixture, sem_config

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _paths():
    from shine_mapping_amd import autograd_ops

    def public(dec, f):
        return dec.sem_label_prob(f)

    def python(dec, f):
        return autograd_ops.SemLabelProb.apply(f, *dec.sem_params())

    return [("public", public), ("python", python)]


@pytest.mark.parametrize("path", [0, 1])
def test_semantic_head_matches_the_reference_fixture(path):
    name, fn = _paths()[path]
    for case in load_fixture()["cases"]:
        dec = decoder_from_case(case, "cuda")
        lab = dec.sem_label(case["feat"].cuda())
        assert lab.dtype == torch.int64 and torch.equal(lab.cpu(), case["sem_label"]), case["name"]
        for d, rec in case["by_decimation"].items():
            f = case["feat"].cuda().requires_grad_(True)
            dec.zero_grad(set_to_none=True)
            logp = fn(dec, f)
            if name == "public":
                assert "SemLabelProb" in logp.grad_fn.name(), logp.grad_fn.name()
            scale = max(1.0, float(case["logp"].abs().max()))
            assert float((logp.detach().cpu() - case["logp"]).abs().max()) <= 1e-5 * scale, (case["name"], name)
            assert torch.equal(torch.argmax(logp.detach(), dim=1).cpu(), case["sem_label"]), case["name"]
            loss = torch.nn.NLLLoss()(logp[::d], case["label"].cuda()[::d])
            loss.backward()
            ref = float(rec["loss"])
            assert abs(float(loss.detach()) - ref) <= 1e-5 * max(1.0, abs(ref)), (case["name"], d, float(loss.detach()), ref)
            assert rel_err(f.grad, rec["grad_feat"]) <= 1e-5, (case["name"], d, rel_err(f.grad, rec["grad_feat"]))
            for k, p in dec.named_parameters():
                if k.startswith("lout"):
                    assert p.grad is None, k
                    continue
                assert rel_err(p.grad, rec["grads"][k]) <= 1e-5, (case["name"], d, k, rel_err(p.grad, rec["grads"][k]))


def _big(n, seed, classes=21):
    from shine_mapping_amd import Decoder

    torch.manual_seed(seed)
    dec = Decoder(sem_config("cuda", classes - 1), is_geo_encoder=False)
    g = torch.Generator(device="cuda").manual_seed(seed)
    f = torch.randn(n, 8, device="cuda", generator=g) * 0.3
    dlogp = torch.randn(n, classes, device="cuda", generator=g) / n
    return dec, f, dlogp


def _fp64_reference(dec, f, dlogp):
    ps = [p.detach().double().requires_grad_(True) for p in dec.sem_params()]
    fd = f.detach().double().requires_grad_(True)
    h = torch.relu(fd @ ps[0].T + ps[1])
    h = torch.relu(h @ ps[2].T + ps[3])
    logp = torch.log_softmax(h @ ps[4].T + ps[5], dim=1)
    grads = torch.autograd.grad(logp, [fd] + ps, dlogp.double())
    return logp.detach(), grads[0], grads[1:]


def _kink_rows(dec, f, eps=1e-5):
    """rows with a hidden pre-activation within eps of 0 (in fp64): float32 rounding may put them on either side of ReLU's kink,
    and the gradient jumps there"""
    ps = [p.detach().double() for p in dec.sem_params()]
    z1 = f.double() @ ps[0].T + ps[1]
    z2 = torch.relu(z1) @ ps[2].T + ps[3]
    return (z1.abs() < eps).any(dim=1) | (z2.abs() < eps).any(dim=1)


def test_semantic_head_at_a_million_points_matches_an_fp64_composite():
    n = 1 << 20
    dec, f, dlogp = _big(n, 3)
    kink = _kink_rows(dec, f)
    assert int(kink.sum()) <= n // 100, int(kink.sum())
    dlogp[kink] = 0.0  # (no gradient flows from the rows at a kink: both sides then agree on every other row)
    fr = f.clone().requires_grad_(True)
    logp = dec.sem_label_prob(fr)
    logp.backward(dlogp)
    ref_logp, ref_df, ref_w = _fp64_reference(dec, f, dlogp)
    assert rel_err(logp, ref_logp) <= 1e-5
    assert rel_err(fr.grad, ref_df) <= 1e-5, rel_err(fr.grad, ref_df)
    for p, r, nm in zip(dec.sem_params(), ref_w, SEM_NAMES):
        assert rel_err(p.grad, r) <= 1e-5, (nm, rel_err(p.grad, r))
    # labels: exact except where the fp64 top two are within 4 float32 ulp (rounding may order them either way)
    lab = dec.sem_label(f)
    ref_lab = torch.argmax(ref_logp, dim=1)
    top = ref_logp.topk(2, dim=1).values
    near = (top[:, 0] - top[:, 1]) <= 4 * torch.finfo(torch.float32).eps * top[:, 0].abs().clamp_min(1e-30)
    diff = lab != ref_lab
    assert not bool((diff & ~near).any()), int((diff & ~near).sum())
    assert int(diff.sum()) <= max(16, n // 10000), int(diff.sum())
    assert torch.equal(lab, torch.argmax(logp.detach(), dim=1))  # (the labels-only launch is the argmax of the same logp)


def test_weight_grads_are_bit_identical_over_repeated_calls():
    dec, f, dlogp = _big(200_003, 5)
    runs = []
    for _ in range(3):
        dec.zero_grad(set_to_none=True)
        fr = f.clone().requires_grad_(True)
        dec.sem_label_prob(fr).backward(dlogp)
        runs.append([p.grad.clone() for p in dec.sem_params()] + [fr.grad.clone()])
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


def test_frozen_decoder_gets_no_weight_grads_and_the_same_feature_grad():
    dec, f, dlogp = _big(70_001, 9)
    fr = f.clone().requires_grad_(True)
    dec.sem_label_prob(fr).backward(dlogp)
    df_full = fr.grad.clone()
    dec.zero_grad(set_to_none=True)
    for p in dec.parameters():  # freeze_model (utils/tools.py), shine_incre.py:94-97
        p.requires_grad_(False)
    fr2 = f.clone().requires_grad_(True)
    dec.sem_label_prob(fr2).backward(dlogp)
    assert all(p.grad is None for p in dec.parameters())
    assert torch.equal(fr2.grad, df_full)


def test_double_backward_raises():
    dec, f, dlogp = _big(1000, 2)
    for _, fn in _paths():  # (the C++ node refuses create_graph at once, the Python node when its result is differentiated)
        fr = f.clone().requires_grad_(True)
        with pytest.raises(RuntimeError):
            (g,) = torch.autograd.grad(fn(dec, fr), fr, dlogp, create_graph=True)
            torch.autograd.grad(g.sum(), fr)


# ---- the feature gradient: the sem head's d loss / d feat reaches the tables through the interpolation node and sums with the
# fused query_feature -> sdf node's contribution

@pytest.fixture(scope="module")
def workload():
    from shine_mapping_amd import Decoder, synth

    wl = synth.build_workload("maicity", frames=12, beams=32, azimuths=180, device="cuda", seed=7)
    torch.manual_seed(1)
    sem = Decoder(wl.cfg, is_geo_encoder=False)
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters()) + list(sem.parameters())]
    return wl, sem, start


def _reset(wl, sem, start):
    from shine_mapping_amd import autograd_ops

    params = list(wl.octree.hier_features) + list(wl.decoder.parameters()) + list(sem.parameters())
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
            p.grad = None
            p.requires_grad_(True)
    autograd_ops.bump_param_epoch()
    return params


def _iteration(wl, sem, coord, sdf_label, weight, eik, dec_s, hip, hip_sdf=None):
    """shine_batch.py:119-209's body with semantic_on: BCE [+ eikonal] + weight_s * NLL(sem_pred[::d], label[::d]).  hip: the
    semantic head on HIP (else its composite); hip_sdf: the fused query_feature -> sdf node (else the decoder's composite),
    default as `hip`"""
    from shine_mapping_amd import get_gradient, sdf_bce_loss, synth

    cfg = wl.cfg
    sem_label = synth.semantic_labels(coord, weight, 21)
    if eik:
        coord = coord.clone().requires_grad_(True)
    feature = wl.octree.query_feature(coord)
    pred = wl.decoder.sdf(feature) if (hip if hip_sdf is None else hip_sdf) else wl.decoder._sdf_composite(feature)
    sem_pred = sem.sem_label_prob(feature) if hip else sem._sem_composite(feature)
    loss = sdf_bce_loss(pred, sdf_label, cfg.sigma_sigmoid, torch.abs(weight), False, "mean")
    if eik:
        g = get_gradient(coord, pred) * cfg.sigma_sigmoid
        loss = loss + 0.1 * ((1.0 - g[weight > 0].norm(2, dim=-1)) ** 2).mean()
    sem_loss = torch.nn.NLLLoss(reduction="mean")(sem_pred[::dec_s, :], sem_label[::dec_s])
    return loss, sem_loss


@pytest.mark.parametrize("eik", [False, True])
@pytest.mark.parametrize("dec_s", [1, 3])
def test_tables_grad_sums_the_sdf_node_and_the_semantic_head(workload, eik, dec_s):
    from shine_mapping_amd import autograd_ops, synth

    wl, sem, start = workload
    gen = torch.Generator(device="cuda").manual_seed(4)
    batches = [synth.draw_batch(wl.pool, 8192, gen) for _ in range(2)]
    autograd_ops.FUSE_WITH_COORD_GRAD = True
    try:
        got = {}
        for mode in ("hip", "hip_reversed", "composite"):
            params = _reset(wl, sem, start)
            per_iter = []
            for coord, sdf_label, weight in batches:  # two iterations with zero_grad(set_to_none=True) between
                for p in params:
                    p.grad = None
                loss, sem_loss = _iteration(wl, sem, coord, sdf_label, weight, eik, dec_s, mode != "composite")
                if mode == "hip":
                    (loss + sem_loss).backward()
                else:  # the other order of the two contributions (autograd accumulates either way)
                    sem_loss.backward(retain_graph=True)
                    loss.backward()
                per_iter.append([p.grad.clone() for p in wl.octree.hier_features])
            got[mode] = per_iter
        for it in range(2):
            for a, b, c in zip(got["hip"][it], got["hip_reversed"][it], got["composite"][it]):
                assert rel_err(a, c) <= 1e-4, (eik, dec_s, it, rel_err(a, c))
                assert rel_err(b, c) <= 1e-4, (eik, dec_s, it, rel_err(b, c))
    finally:
        autograd_ops.FUSE_WITH_COORD_GRAD = False
        _reset(wl, sem, start)


ITERS = 30
LOOP_TOL = dict(loss=2e-3, params=2e-2)  # HIP + FusedAdam vs composites + torch.optim.Adam after 30 steps (test_gpu_loss_modes)


def _loop(wl, sem, start, hip, freeze_after=None):
    from shine_mapping_amd import optim, synth

    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.semantic_on, cfg.ray_loss = 0.01, 1e-15, True, True, False
    cfg.lr_level_reduce_ratio = 1.0
    octree, dec = wl.octree, wl.decoder
    params = _reset(wl, sem, start)
    feats, geo, semp = list(octree.parameters()), list(dec.parameters()), list(sem.parameters())

    def make_opt():
        if hip:
            return optim.setup_optimizer(cfg, feats, geo, semp, None)
        groups = [{"params": geo, "lr": cfg.lr, "weight_decay": cfg.weight_decay},
                  {"params": semp, "lr": cfg.lr, "weight_decay": cfg.weight_decay}]
        groups += [{"params": feats[cfg.tree_level_feat - i - 1], "lr": cfg.lr} for i in range(cfg.tree_level_feat)]
        return torch.optim.Adam(groups, betas=(0.9, 0.99), eps=cfg.adam_eps)

    opt = make_opt()
    gen = torch.Generator(device="cuda").manual_seed(11)
    seen = []
    for it in range(ITERS):
        if freeze_after is not None and it == freeze_after:  # shine_incre.py:94-97: freeze both decoders after frame 1, new optimiser
            for p in geo + semp:
                p.requires_grad_(False)
                p.grad = None
            opt = make_opt()
        coord, sdf_label, weight = synth.draw_batch(wl.pool, 4096, gen)
        # (the geometry path is the fused node in both runs, as in test_gpu_loss_modes: what differs is the semantic head and
        # the optimiser)
        loss, sem_loss = _iteration(wl, sem, coord, sdf_label, weight, False, 1, hip, hip_sdf=True)
        cur = loss + 1.0 * sem_loss
        opt.zero_grad(set_to_none=True)
        cur.backward()
        opt.step()
        seen.append(float(cur.detach()))
    torch.cuda.synchronize()
    out = [p.detach().clone() for p in params]
    _reset(wl, sem, start)
    return seen, out


@pytest.mark.parametrize("freeze_after", [None, 10])
def test_tier_a_semantic_loop_matches_the_composites(workload, freeze_after):
    wl, sem, start = workload
    hip = _loop(wl, sem, start, True, freeze_after)
    ref = _loop(wl, sem, start, False, freeze_after)
    worst = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(hip[0], ref[0]))
    assert worst <= LOOP_TOL["loss"], (freeze_after, worst)
    assert hip[0][-1] < hip[0][0]  # (it trains)
    n_feat = len(wl.octree.hier_features)
    for k, (a, b) in enumerate(zip(hip[1], ref[1])):
        if k >= n_feat + 8 and (k - n_feat - 8) in (4, 5):
            assert torch.equal(a, b), "the semantic decoder's lout never moves"
        assert rel_err(a, b) <= LOOP_TOL["params"], (freeze_after, k, rel_err(a, b))


def test_mesher_labels_match_query_feature_and_the_composite(workload):
    from shine_mapping_amd.mesher import Mesher

    wl, sem, start = workload
    _reset(wl, sem, start)
    octree = wl.octree
    sem = copy.deepcopy(sem)
    with torch.no_grad():  # (an untrained head on feature_std-sized features labels every point alike: spread the logits)
        sem.layers[0].weight.mul_(100.0)
        sem.nclass_out.weight.mul_(10.0)
    m = Mesher(wl.cfg, octree, wl.decoder, sem)
    lo, hi = wl.pool.coord.min(0).values, wl.pool.coord.max(0).values
    side = 102  # 102^3 ~ 2^20 grid points
    axes = [torch.linspace(float(lo[k]), float(hi[k]), side, device="cuda") for k in range(3)]
    coord = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    with torch.no_grad():
        ref_logp = torch.cat([sem._sem_composite(octree.query_feature(c, True)) for c in coord.split(1 << 18)])
    ref = torch.argmax(ref_logp, dim=1).cpu().numpy()
    top = ref_logp.topk(2, dim=1).values
    near = ((top[:, 0] - top[:, 1]) <= 1e-5 * top[:, 0].abs().clamp_min(1e-6)).cpu().numpy()  # (rounding may order a near tie)
    _, sem_un, _ = m.query_points(coord, coord.shape[0] + 1, False, True, False)
    assert sem_un.dtype == np.int64 and sem_un.shape == ref.shape
    diff = sem_un != ref
    assert not (diff & ~near).any() and diff.sum() <= max(16, ref.size // 10000), (int(diff.sum()), int((diff & ~near).sum()))
    sdf_c, sem_c, mask_c = m.query_points(coord, 1 << 17, True, True, True)
    assert sem_c.dtype == np.float64 and np.array_equal(sem_c, sem_un.astype(np.float64))
    sdf_r, _, mask_r = m.query_points(coord, 1 << 17, True, False, True)
    assert np.array_equal(sdf_c, sdf_r) and np.array_equal(mask_c, mask_r)
    assert len(np.unique(ref)) > 1
