"""GPU: the semantic head (csrc/shine_semantic.hip) — sem_label_prob, its backward and sem_label against the reference's recorded
values (tests/golden/semantic.pt), against an fp64 composite at 2^20 points, repeat determinism, the frozen decoder, the feature
gradient it shares with the fused query_feature -> sdf node, the drivers' Tier A loop with the fused optimiser's semantic group,
and the mesher's label query; then the sweeps on the CPU-generated inputs of tests/test_semantic.py: every class count 1..32, the
entry points' optional outputs with guard floats behind the padded Wc / bc gradients, ties / large logits / dead rows, every
shape of the backward's ticket reduction with interleaved calls on one workspace, and all eight label-query instantiations."""
import copy

import numpy as np
import pytest
import torch

from test_semantic import (FWD_STRIDE_N, SEM_NAMES, SWEEP_N, TICKET_CLASSES, TICKET_SIZES, decoder_from_case, decoder_from_params,
                           fp64_logits, kink_rows, load_fixture, sem_config, sweep_inputs, sweep_params, tie_pairs, value_case)

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
    return kink_rows(dec.sem_params(), f, eps)


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


# ---- sweeps: the inputs come from tests/test_semantic.py's CPU generators (their conditions are asserted there)

def _sweep(C, n=SWEEP_N, seed=None, params=None):
    """decoder, features and d loss / d logp on the device; no gradient flows from the rows at a ReLU kink"""
    dec = decoder_from_params(sweep_params(C) if params is None else params, "cuda")
    f, dlogp = (t.cuda() for t in sweep_inputs(C, n, seed))
    kink = _kink_rows(dec, f)
    assert int(kink.sum()) <= max(2, n // 100), (C, n, int(kink.sum()))
    dlogp[kink] = 0.0
    return dec, f, dlogp


def _run(fn, dec, f, dlogp):
    """(logp, d feat, the six weight grads) of one forward and backward"""
    dec.zero_grad(set_to_none=True)
    fr = f.clone().requires_grad_(True)
    logp = fn(dec, fr)
    logp.backward(dlogp)
    return logp.detach(), fr.grad, [p.grad for p in dec.sem_params()]


def _flat(run):
    return [run[0], run[1]] + list(run[2])


def _assert_matches_fp64(what, got, ref):
    """the file's rel_err <= 1e-5 on logp, d feat and the six weight grads"""
    names = ("logp", "d feat") + SEM_NAMES
    errs = [rel_err(a, b) for a, b in zip(_flat(got), _flat(ref))]
    print("%s  " % (what,) + "  ".join("%s %.2e" % (k.replace("layers.", "l").replace("nclass_out", "c"), e)
                                       for k, e in zip(names, errs)))
    for k, e in zip(names, errs):
        assert e <= 1e-5, (what, k, e)


@pytest.mark.parametrize("C", range(1, 33))
def test_every_class_count_matches_an_fp64_composite(C):
    dec, f, dlogp = _sweep(C)
    ref = _fp64_reference(dec, f, dlogp)
    lab = dec.sem_label(f)
    assert lab.dtype == torch.int64 and lab.shape == (SWEEP_N,)
    for name, fn in _paths():
        got = _run(fn, dec, f, dlogp)
        assert got[0].shape == (SWEEP_N, C) and all(g is not None for g in got[2]), (C, name)
        _assert_matches_fp64("C=%d n=%d %s" % (C, SWEEP_N, name), got, ref)
        assert torch.equal(lab, torch.argmax(got[0], dim=1)), (C, name)  # (the labels-only launch: the argmax of the same logp)
        if C == 1:  # log_softmax of one class is 0, and dz = dlogp - exp(0) dlogp: exact zeros, no tolerance
            assert torch.equal(got[0], torch.zeros_like(got[0])) and torch.equal(lab, torch.zeros_like(lab)), name
            for k, g in zip(("d feat",) + SEM_NAMES, _flat(got)[1:]):
                assert torch.equal(g, torch.zeros_like(g)), (name, k)


SENTINEL = -12345.0
GUARD = 64


def _guarded(numel):
    return torch.full((numel + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")


def _raw_backward(f, logp, dlogp, params, want_f, want_w):
    """shine_sem_backward through ctypes with each output followed by 64 guard floats; (d feat | None, six grads | None)"""
    from shine_mapping_amd import _lib, autograd_ops

    n, C = logp.shape
    sizes = [32 * 8, 32, 32 * 32, 32, C * 32, C]
    df = _guarded(n * 8) if want_f else None
    gw = [_guarded(k) for k in sizes] if want_w else None
    _lib.check(_lib.lib().shine_sem_backward(
        f.data_ptr(), logp.data_ptr(), dlogp.data_ptr(), n, _lib.ptr_array([p.data_ptr() for p in params]), C,
        df.data_ptr() if want_f else None, _lib.ptr_array([t.data_ptr() for t in gw]) if want_w else None,
        autograd_ops.sem_workspace(f.device).data_ptr(), _lib.current_stream_handle()), "shine_sem_backward")
    torch.cuda.synchronize()
    for t, k in zip(([df] if want_f else []) + (gw if want_w else []), ([n * 8] if want_f else []) + (sizes if want_w else [])):
        assert torch.equal(t[k:], torch.full((GUARD,), SENTINEL, device="cuda")), ("guard floats written", C, k)
        assert not bool((t[:k] == SENTINEL).any()), ("output not written", C, k)
    return (df[:n * 8].view(n, 8) if want_f else None), ([t[:k].view(p.shape) for t, k, p in zip(gw, sizes, params)] if want_w else None)


@pytest.mark.parametrize("C", [1, 5, 32])
def test_entry_points_with_optional_outputs_and_guarded_gradients(C):
    from shine_mapping_amd import autograd_ops

    dec, f, dlogp = _sweep(C)
    params = [p.detach() for p in dec.sem_params()]
    logp, lab = autograd_ops.sem_forward(f, params, want_logp=True, want_label=True)
    only_logp, none = autograd_ops.sem_forward(f, params, want_logp=True, want_label=False)
    assert none is None and torch.equal(only_logp, logp), C
    none, only_lab = autograd_ops.sem_forward(f, params, want_logp=False, want_label=True)
    assert none is None and only_lab.dtype == torch.int64 and torch.equal(only_lab, lab), C
    assert torch.equal(lab, torch.argmax(logp, dim=1)), C
    # backward: the Wc / bc partials are padded to 32 classes, the outputs are [C, 32] / [C] with guard floats behind them
    df, gw = _raw_backward(f, logp, dlogp, params, True, True)
    ref = _fp64_reference(dec, f, dlogp)
    _assert_matches_fp64("C=%d n=%d ctypes" % (C, SWEEP_N), (logp, df, gw), ref)
    df_only, none = _raw_backward(f, logp, dlogp, params, True, False)
    assert none is None and torch.equal(df_only, df), C
    none, gw_only = _raw_backward(f, logp, dlogp, params, False, True)
    assert none is None and all(torch.equal(a, b) for a, b in zip(gw_only, gw)), C
    pub = _run(_paths()[0][1], dec, f, dlogp)  # (the autograd node makes the same call)
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(_flat(pub), [logp, df] + gw)), C


# ---- values where a one-pass softmax or argmax goes wrong

@pytest.mark.parametrize("C", [2, 7, 32])
def test_exact_ties_go_to_the_first_class(C):
    dec = decoder_from_params(value_case("ties", C), "cuda")
    f = sweep_inputs(C)[0].cuda()
    lab = dec.sem_label(f)
    for name, fn in _paths():
        logp = fn(dec, f).detach()
        mx = logp.max(dim=1, keepdim=True).values
        first = torch.where(logp == mx, torch.arange(C, device="cuda").expand_as(logp), C).min(dim=1).values
        assert torch.equal(lab, first) and torch.equal(lab, torch.argmax(logp, dim=1)), (C, name)
        for i, j in tie_pairs(C):
            assert torch.equal(logp[:, i], logp[:, j]), (C, name, i, j)
            rows = (logp[:, i] == mx[:, 0]) & (first >= min(i, j))  # either is the argmax
            assert int(rows.sum()) > 0 and bool((lab[rows] == min(i, j)).all()), (C, name, i, j, int(rows.sum()))
            assert not bool((lab == max(i, j)).any()), (C, name, i, j)


@pytest.mark.parametrize("C", [2, 7, 32])
def test_large_logits_neither_overflow_nor_lose_the_normalisation(C):
    dec = decoder_from_params(value_case("large", C), "cuda")
    f = sweep_inputs(C)[0].cuda()
    _, z = fp64_logits(dec.sem_params(), f)
    assert float(z.abs().max()) > 200.0
    ref = torch.log_softmax(z, dim=1)
    for name, fn in _paths():
        logp = fn(dec, f).detach()
        assert torch.isfinite(logp).all(), (C, name)
        err, norm = rel_err(logp, ref), float((torch.exp(logp.double()).sum(dim=1) - 1.0).abs().max())
        print("C=%d %s  max|z| %.1f  min logp %.1f  rel_err %.2e  |sum exp(logp) - 1| %.2e"
              % (C, name, float(z.abs().max()), float(ref.min()), err, norm))
        assert err <= 1e-5, (C, name, err)
        assert norm <= 1e-5, (C, name, norm)
        assert torch.equal(dec.sem_label(f), torch.argmax(logp, dim=1)), (C, name)


@pytest.mark.parametrize("C", [2, 7, 32])
def test_dead_rows_zero_gradients_and_zero_features(C):
    dec, f, dlogp = _sweep(C, params=value_case("dead", C))
    ref = _fp64_reference(dec, f, dlogp)
    bc = dec.sem_params()[5].detach().double()
    assert rel_err(ref[0], torch.log_softmax(bc, dim=0).expand(SWEEP_N, C)) <= 1e-12  # (the same row everywhere)
    for name, fn in _paths():
        got = _run(fn, dec, f, dlogp)
        _assert_matches_fp64("dead C=%d %s" % (C, name), got, ref)  # (logp = log_softmax(bc) on every row, dbc, dWc = 0)
        for k, g in zip(("d feat",) + SEM_NAMES[:4], _flat(got)[1:6]):
            assert torch.equal(g, torch.zeros_like(g)), (C, name, k)
    # zero d loss / d logp: every gradient exactly 0; zero features: finite outputs that match the composite
    dec, f, dlogp = _sweep(C)
    assert not bool(_kink_rows(dec, torch.zeros_like(f)).any()), C  # (zero features: the same pre-activations on every row)
    zref = _fp64_reference(dec, torch.zeros_like(f), dlogp)
    for name, fn in _paths():
        got = _run(fn, dec, f, torch.zeros_like(dlogp))
        for k, g in zip(("d feat",) + SEM_NAMES, _flat(got)[1:]):
            assert torch.equal(g, torch.zeros_like(g)), (C, name, k)
        got = _run(fn, dec, torch.zeros_like(f), dlogp)
        assert all(bool(torch.isfinite(g).all()) for g in _flat(got)), (C, name)
        _assert_matches_fp64("zero features C=%d %s" % (C, name), got, zref)


# ---- every shape of the backward's two-level ticket reduction, and the forward's grid-stride pass

@pytest.mark.parametrize("n", TICKET_SIZES)
@pytest.mark.parametrize("C", TICKET_CLASSES)
def test_backward_ticket_reduction_at_every_launch_shape(C, n):
    """against the fp64 composite, and bit-identical when repeated on the same workspace with a launch of another shape in
    between: every ticket counter is back at zero after every launch shape"""
    dec, f, dlogp = _sweep(C, n, 1000 + n)
    other = 257 if n != 257 else 65537
    _, fo, do = _sweep(C, other, 1000 + other)
    ref = _fp64_reference(dec, f, dlogp)
    for name, fn in _paths():
        first = [t.clone() for t in _flat(_run(fn, dec, f, dlogp))]
        _run(fn, dec, fo, do)
        again = _flat(_run(fn, dec, f, dlogp))
        _assert_matches_fp64("C=%d n=%d %s" % (C, n, name), (first[0], first[1], first[2:]), ref)
        for k, a, b in zip(("logp", "d feat") + SEM_NAMES, first, again):
            assert torch.equal(a, b), (C, n, other, name, k)


@pytest.mark.parametrize("C", [3, 32])
def test_forward_grid_stride_pass(C):
    n = FWD_STRIDE_N
    dec = decoder_from_params(sweep_params(C), "cuda")
    f = sweep_inputs(C, n, 1000 + n)[0].cuda()
    with torch.no_grad():
        logp = dec.sem_label_prob(f)
    lab = dec.sem_label(f)
    ref_logp = torch.log_softmax(fp64_logits(dec.sem_params(), f)[1], dim=1)
    err = rel_err(logp, ref_logp)
    # labels: exact except where the fp64 top two are within 4 float32 ulp (rounding may order them either way)
    ref_lab = torch.argmax(ref_logp, dim=1)
    top = ref_logp.topk(2, dim=1).values
    near = (top[:, 0] - top[:, 1]) <= 4 * torch.finfo(torch.float32).eps * top[:, 0].abs().clamp_min(1e-30)
    diff = lab != ref_lab
    print("C=%d n=%d  logp rel_err %.2e  near ties %d  labels that differ %d" % (C, n, err, int(near.sum()), int(diff.sum())))
    assert err <= 1e-5, (C, n, err)
    assert not bool((diff & ~near).any()), (C, n, int((diff & ~near).sum()))
    assert int(diff.sum()) <= max(16, n // 10000), (C, n, int(diff.sum()))
    assert torch.equal(lab, torch.argmax(logp, dim=1)), (C, n)


# ---- mesh labels: k_sem_query<L, POLY> for L = 1..4, both interpolations

@pytest.mark.parametrize("poly", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_mesh_labels_in_every_instantiation(L, poly):
    from shine_mapping_amd import synth
    from shine_mapping_amd.mesher import Mesher

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L,
                              poly_int_on=poly)
    octree = wl.octree
    assert octree.featured_level_num == L and bool(octree.step_config().poly_int_on) == poly
    params = sweep_params(21)
    params[0] *= 100.0  # (an untrained head on feature_std-sized features labels every point alike: spread the logits)
    params[4] *= 10.0
    sem = decoder_from_params(params, "cuda")
    m = Mesher(wl.cfg, octree, wl.decoder, sem)
    cell = wl.cfg.leaf_vox_size * wl.cfg.scale  # one leaf cell of margin: points that miss some or all levels
    lo, hi = wl.pool.coord.min(0).values - cell, wl.pool.coord.max(0).values + cell
    side = 40
    axes = [torch.linspace(float(lo[k]), float(hi[k]), side, device="cuda") for k in range(3)]
    coord = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    with torch.no_grad():
        feat = octree.query_feature(coord, True)
        ref_logp = sem._sem_composite(feat)
    missed = int((feat.abs().sum(dim=1) == 0).sum())
    assert coord.shape[0] - missed >= 256, (L, poly, missed)  # (enough points that interpolate at all)
    ref = torch.argmax(ref_logp, dim=1).cpu().numpy()
    top = ref_logp.topk(2, dim=1).values
    near = ((top[:, 0] - top[:, 1]) <= 1e-5 * top[:, 0].abs().clamp_min(1e-6)).cpu().numpy()  # (rounding may order a near tie)
    _, sem_un, _ = m.query_points(coord, coord.shape[0] + 1, False, True, False)
    assert sem_un.dtype == np.int64 and sem_un.shape == ref.shape
    diff = sem_un != ref
    print("L=%d poly=%d  N=%d  points off every level %d  classes %d  near ties %d  labels that differ %d"
          % (L, poly, ref.size, missed, len(np.unique(ref)), int(near.sum()), int(diff.sum())))
    assert not (diff & ~near).any() and diff.sum() <= max(16, ref.size // 10000), (L, poly, int(diff.sum()),
                                                                                   int((diff & ~near).sum()))
    assert len(np.unique(ref)) > 1
    _, sem_c, _ = m.query_points(coord, 257, False, True, False)  # (250 launches, the last one ragged)
    assert sem_c.dtype == np.float64 and np.array_equal(sem_c, sem_un.astype(np.float64)), (L, poly)
