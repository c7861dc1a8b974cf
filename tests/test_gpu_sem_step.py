"""GPU: the semantic training step (csrc/shine_sem_step.hip) — ops.fused_sem_step against the composite the repository uses
(query_feature -> Decoder._sem_composite -> NLLLoss('mean') on [::d], times weight_s, backward()) over tile tails, decimations
and class counts, every L x interpolation instantiation, the pool's two record layouts, reproducibility, accumulation, the
frozen head; then loop.GraphedIteration(sem=...) against an eager replay of its own batches, and the labelled dataset's pool."""
import contextlib
import copy

import pytest
import torch

from test_semantic import sem_config

pytestmark = pytest.mark.gpu

WEIGHT_S = 0.7
STEP_TOL = 1e-4                          # tests/test_gpu_semantic.py: one step's gradients and loss against the composite
LOOP_TOL = dict(loss=2e-3, params=2e-2)  # tests/test_gpu_semantic.py: HIP + FusedAdam vs composites + torch.optim.Adam, 30 steps


# every entry point of the library through which an iteration can put a kernel on the stream (or a node into the library-built
# graph): the launch counts below are COUNTED calls of these during one recorded iteration, not declared numbers
LAUNCHERS = ("shine_train_step", "shine_sem_train_step", "shine_finish_iteration", "shine_adam_step_dev", "shine_adam_step",
             "shine_regularize", "shine_sample_sorted", "shine_sample_sorted_dev", "shine_sample_sorted_finish",
             "shine_sample_sorted_slice", "shine_sem_forward", "shine_sem_backward", "shine_forward", "shine_interp_backward",
             "shine_interp_sdf_backward", "shine_mark_touched", "shine_iter_graph_set_step", "shine_iter_graph_set_finish")


@contextlib.contextmanager
def counted_launches():
    """[(entry point, its arguments)] of every launching library call made inside the block"""
    from shine_mapping_amd import _lib

    lib, calls, saved = _lib.lib(), [], {}
    for name in LAUNCHERS:
        saved[name] = fn = getattr(lib, name)
        setattr(lib, name, lambda *a, _fn=fn, _name=name: (calls.append((_name, a)), _fn(*a))[1])
    try:
        yield calls
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


SEM_ITERATION = ["shine_train_step", "shine_sem_train_step", "shine_finish_iteration"]


def _assert_recorded(calls, head_trains):
    """one recorded semantic iteration: fused step, semantic step, tail, and while the head trains ONE Adam launch on its six
    tensors whose flags (1 | 2: clear the grads, the step was counted already) rule out a preparation launch"""
    names = [c[0] for c in calls]
    assert names == SEM_ITERATION + (["shine_adam_step_dev"] if head_trains else []), names
    assert calls[0][1][1]._obj.defer_reduce == 1  # (the fused kernel alone: its reduction is the tail's)
    if head_trains:
        args = calls[3][1]
        assert args[0] == 6 and args[12] == 3, (args[0], args[12])


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def workload():
    from shine_mapping_amd import synth

    return synth.build_workload("maicity", frames=12, beams=32, azimuths=180, device="cuda", seed=7)


def _head(C, seed=1):
    from shine_mapping_amd import Decoder

    torch.manual_seed(seed)
    return Decoder(sem_config("cuda", C - 1), is_geo_encoder=False)


def _labels(coord, weight, C):
    from shine_mapping_amd import synth

    if C == 1:
        return torch.zeros(coord.shape[0], dtype=torch.int32, device=coord.device)
    return synth.semantic_labels(coord, weight, C).to(torch.int32)


def _batch(wl, n, C, seed):
    """n pool samples; from 8 rows on, rows 3..6 are moved a few leaf cells outside the mapped box: they miss every node"""
    from shine_mapping_amd import synth

    gen = torch.Generator(device="cuda").manual_seed(seed)
    coord, _, weight = synth.draw_batch(wl.pool, n, gen)
    coord = coord.clone()
    if n >= 8:
        cell = wl.cfg.leaf_vox_size * wl.cfg.scale
        coord[3:7] = (wl.pool.coord.max(0).values + 3.0 * cell).clamp(max=0.999)
        with torch.no_grad():
            assert bool((wl.octree.query_feature(coord[3:7], True) == 0).all()), "rows meant to miss every level"
    return coord.contiguous(), _labels(coord, weight, C)


def _clear(octree, sem):
    for p in list(octree.hier_features) + list(sem.parameters()):
        p.grad = None


def _composite(octree, sem, coord, labels, d, weight_s=WEIGHT_S):
    _clear(octree, sem)
    logp = sem._sem_composite(octree.query_feature(coord))
    loss = torch.nn.NLLLoss(reduction="mean")(logp[::d, :], labels.long()[::d])
    (weight_s * loss).backward()
    out = (loss.detach(), [p.grad.clone() for p in octree.hier_features], [p.grad.clone() for p in sem.sem_params()])
    assert all(p.grad is None for p in sem.lout.parameters())
    _clear(octree, sem)
    return out


def _fused(octree, sem, coord, labels, d, weight_s=WEIGHT_S, **kw):
    from shine_mapping_amd import ops

    _clear(octree, sem)
    loss = ops.fused_sem_step(octree, sem, coord, labels, weight_s, d, **kw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.grad_fn is None
    frozen = not sem.sem_params()[0].requires_grad
    out = (loss.clone(), [p.grad.clone() for p in octree.hier_features],
           None if frozen else [p.grad.clone() for p in sem.sem_params()])
    assert all(p.grad is None for p in sem.lout.parameters())
    _clear(octree, sem)
    return out


def _assert_close(what, got, ref, tol=STEP_TOL):
    errs = [rel_err(got[0], ref[0])] + [rel_err(a, b) for a, b in zip(got[1] + got[2], ref[1] + ref[2])]
    print(what, " ".join("%.1e" % e for e in errs))
    assert max(errs) <= tol, (what, errs)


# ---- 1. one step against the composite
@pytest.mark.parametrize("C", [1, 21, 32])
# (a workgroup is 256 rows, a first-level run of the ticket sums 16 workgroups, the grid 256 workgroups at most: 257 = two
# workgroups, 4096 = exactly one full run, 4096 + 17 = a run of one behind it, 65537 = every workgroup and a grid-stride pass)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096, 4096 + 17, 65537])
def test_one_step_matches_the_composite(workload, n, C):
    wl = workload
    sem = _head(C)
    coord, labels = _batch(wl, n, C, 100 + n)
    for d in (1, 3, n + 5):
        ref = _composite(wl.octree, sem, coord, labels, d)
        got = _fused(wl.octree, sem, coord, labels, d)
        _assert_close("n=%d C=%d d=%d" % (n, C, d), got, ref)
        if n >= 8 and d in (1, 3):  # the rows outside every node were computed: their gradient is in the trash rows
            assert all(bool(g[-1].any()) for g in ref[1]) or C == 1
            for lv, (a, b) in enumerate(zip(got[1], ref[1])):  # ... compared on their own, not under the table's largest entry
                assert rel_err(a[-1], b[-1]) <= STEP_TOL, (n, C, d, lv, rel_err(a[-1], b[-1]))
    from shine_mapping_amd import ops

    empty = ops.fused_sem_step(wl.octree, sem, coord[:0], labels[:0], WEIGHT_S, 1)
    assert float(empty) == 0.0
    _clear(wl.octree, sem)


# ---- 2. every instantiation
@pytest.mark.parametrize("poly", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_every_instantiation_matches_the_composite(L, poly):
    from shine_mapping_amd import synth

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L,
                              poly_int_on=poly)
    assert wl.octree.featured_level_num == L and bool(wl.octree.step_config().poly_int_on) == poly
    sem = _head(21)
    coord, labels = _batch(wl, 200, 21, 5)
    for d in (1, 2):
        _assert_close("L=%d poly=%d d=%d" % (L, poly, d), _fused(wl.octree, sem, coord, labels, d),
                      _composite(wl.octree, sem, coord, labels, d))


# ---- 3. pool mode, both record layouts; a bad label is refused at rebuild
@pytest.mark.parametrize("L", [3, 4])
def test_pool_mode_reads_the_records(L):
    from shine_mapping_amd import synth
    from shine_mapping_amd.sampler import SortedPool

    wl = synth.build_workload("maicity", frames=4, beams=16, azimuths=90, device="cuda", seed=7, tree_level_feat=L)
    C = 21
    sem = _head(C)
    pl = wl.pool
    lab = _labels(pl.coord, pl.weight, C)
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=3, sem_label=lab.long(), n_class=C)
    assert pool.rec is not None and (pool._weight_sep is None) == (L < 4)
    assert pool.sem_label.dtype == torch.int32 and pool.sem_label.is_contiguous()
    assert torch.equal(pool.sem_label, lab[pool.perm.long()])
    idx = pool.draw(1000)
    coord = pool.get_batch(idx)[0]
    labels = pool.sem_label[idx.long()].contiguous()
    for d in (1, 3):
        got = _fused(wl.octree, sem, None, None, d, pool=pool, idx=idx)
        plain = _fused(wl.octree, sem, coord, labels, d)
        assert torch.equal(got[0], plain[0]), (L, d)
        assert all(torch.equal(a, b) for a, b in zip(got[2], plain[2])), (L, d)
        for a, b in zip(got[1], plain[1]):
            assert rel_err(a, b) <= STEP_TOL, (L, d, rel_err(a, b))
        _assert_close("pool L=%d d=%d" % (L, d), got, _composite(wl.octree, sem, coord, labels, d))
    for bad in (C, -1):
        wrong = lab.clone()
        wrong[7] = bad
        with pytest.raises(ValueError, match="out of range"):
            pool.rebuild(pl.coord, pl.sdf_label, pl.weight, sem_label=wrong)
        with pytest.raises(ValueError, match="out of range"):
            SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, sem_label=wrong, n_class=C)
    plain_pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=3)
    assert not hasattr(plain_pool, "sem_label")  # (defaults: today's attributes)


# ---- 4. reproducibility, 5. accumulation, 6. the frozen head
def test_two_calls_give_bit_identical_loss_and_head_grads(workload):
    wl = workload
    sem = _head(21)
    coord, labels = _batch(wl, 4096 + 17, 21, 9)
    a, b = _fused(wl.octree, sem, coord, labels, 1), _fused(wl.octree, sem, coord, labels, 1)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_gradients_accumulate_and_grad_buffers_leave_grad_alone(workload):
    from shine_mapping_amd import ops

    wl, octree = workload, workload.octree
    sem = _head(21)
    coord, labels = _batch(wl, 1000, 21, 13)
    ref = _composite(octree, sem, coord, labels, 3)
    params = list(octree.hier_features) + list(sem.sem_params())
    g = torch.Generator(device="cuda").manual_seed(2)
    start = [torch.randn(p.shape, device="cuda", generator=g) * float(r.abs().max())
             for p, r in zip(params, ref[1] + ref[2])]
    for p, s in zip(params, start):
        p.grad = s.clone()
    ops.fused_sem_step(octree, sem, coord, labels, WEIGHT_S, 3)
    for k, (p, s, r) in enumerate(zip(params, start, ref[1] + ref[2])):
        # (the sum was rounded at the magnitude of start + increment, about twice the increment's: 2^-23 relative, far below)
        assert rel_err(p.grad - s, r) <= STEP_TOL, (k, rel_err(p.grad - s, r))
    # grad_buffers: the same numbers land in the buffers, .grad stays as it is
    kept = [p.grad.clone() for p in params]
    bufs = ([torch.zeros_like(p) for p in octree.hier_features], [torch.zeros_like(p) for p in sem.sem_params()])
    ops.fused_sem_step(octree, sem, coord, labels, WEIGHT_S, 3, grad_buffers=bufs)
    assert all(torch.equal(p.grad, k) for p, k in zip(params, kept))
    for b, r in zip(bufs[0] + bufs[1], ref[1] + ref[2]):
        assert rel_err(b, r) <= STEP_TOL
    _clear(octree, sem)
    bufs = ([torch.zeros_like(p) for p in octree.hier_features], [torch.zeros_like(p) for p in sem.sem_params()])
    ops.fused_sem_step(octree, sem, coord, labels, WEIGHT_S, 3, grad_buffers=bufs)
    assert all(p.grad is None for p in params)
    _clear(octree, sem)


def test_frozen_head_gets_no_gradient_and_the_same_feature_grads(workload):
    wl = workload
    sem = _head(21)
    coord, labels = _batch(wl, 1000, 21, 17)
    full = _fused(wl.octree, sem, coord, labels, 1)
    from shine_mapping_amd import ops

    sem.sem_params()[2].requires_grad_(False)  # a head that is neither trained nor frozen is refused, not treated as frozen
    with pytest.raises(ValueError, match="all require grad or all be frozen"):
        ops.fused_sem_step(wl.octree, sem, coord, labels, WEIGHT_S, 1)
    for p in sem.parameters():  # freeze_model (utils/tools.py), shine_incre.py:94-97
        p.requires_grad_(False)
    guard = [p.detach().clone() for p in sem.parameters()]
    from shine_mapping_amd import ops

    _clear(wl.octree, sem)
    loss = ops.fused_sem_step(wl.octree, sem, coord, labels, WEIGHT_S, 1)
    assert all(p.grad is None for p in sem.parameters())
    assert all(torch.equal(p, g) for p, g in zip(sem.parameters(), guard))
    assert torch.equal(loss, full[0])
    for p, r in zip(wl.octree.hier_features, full[1]):
        assert rel_err(p.grad, r) <= STEP_TOL
    _clear(wl.octree, sem)


# ---- 7. the loop
ITERS = 30
N = 4096
C_LOOP = 21


def _loop_parts(wl, sem, start, seed=11):
    """parameters back at their start, a labelled node-ordered pool and the loop's config"""
    from shine_mapping_amd import autograd_ops
    from shine_mapping_amd.sampler import SortedPool

    params = list(wl.octree.hier_features) + list(wl.decoder.parameters()) + list(sem.parameters())
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
            p.grad = None
            p.requires_grad_(True)
    autograd_ops.bump_param_epoch()
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.semantic_on, cfg.ray_loss, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, True, False, 1.0
    pl = wl.pool
    pool = SortedPool(wl.octree, pl.coord, pl.sdf_label, pl.weight, seed=seed, canonical=True,
                      sem_label=_labels(pl.coord, pl.weight, C_LOOP), n_class=C_LOOP)
    return cfg, params, pool


def _make_opt(cfg, wl, sem, hip):
    from shine_mapping_amd import optim

    feats, geo, semp = list(wl.octree.parameters()), list(wl.decoder.parameters()), list(sem.parameters())
    if hip:
        return optim.setup_optimizer(cfg, feats, geo, semp, None)
    groups = [{"params": geo, "lr": cfg.lr, "weight_decay": cfg.weight_decay},
              {"params": semp, "lr": cfg.lr, "weight_decay": cfg.weight_decay}]
    groups += [{"params": feats[cfg.tree_level_feat - i - 1], "lr": cfg.lr} for i in range(cfg.tree_level_feat)]
    return torch.optim.Adam(groups, betas=(0.9, 0.99), eps=cfg.adam_eps)


def _graphed(cfg, wl, sem, pool, opt, d, **kw):
    from shine_mapping_amd import StepOptions
    from shine_mapping_amd.loop import GraphedIteration, SemTerm

    return GraphedIteration(wl.octree, wl.decoder, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid), N,
                            sem=SemTerm(sem, WEIGHT_S, d), **kw)


@pytest.fixture(scope="module")
def loop_start(workload):
    """the loop's semantic head and every parameter's start; one eager iteration has run on the device afterwards, so the
    iterations under test can be built with eager_first=False and replay nothing but their graph"""
    wl = workload
    sem = _head(C_LOOP, seed=4)
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters()) + list(sem.parameters())]
    cfg, _, pool = _loop_parts(wl, sem, start)
    g = _graphed(cfg, wl, sem, pool, _make_opt(cfg, wl, sem, True), 1)
    assert g.ran_eager and not g.native and float(g.sem_loss) > 0
    return sem, start


def _freeze(wl, sem):
    for p in list(wl.decoder.parameters()) + list(sem.parameters()):
        p.requires_grad_(False)
        p.grad = None


@pytest.mark.parametrize("freeze_after", [None, 10])
def test_graphed_semantic_loop_matches_an_eager_replay(workload, loop_start, freeze_after):
    from shine_mapping_amd import sdf_bce_loss

    wl = workload
    sem, start = loop_start
    d = 3
    cfg, params, pool = _loop_parts(wl, sem, start)
    g = _graphed(cfg, wl, sem, pool, _make_opt(cfg, wl, sem, True), d, eager_first=False)
    assert not g.ran_eager and not g.native
    batches, hip_loss, hip_sem = [], [], []
    recorded = None
    for it in range(ITERS):
        if freeze_after is not None and it == freeze_after:  # shine_incre.py:94-109: both decoders frozen, a new optimiser
            _freeze(wl, sem)
            g = _graphed(cfg, wl, sem, pool, _make_opt(cfg, wl, sem, True), d, eager_first=False)
            recorded = None
        batches.append(g._idx.clone())
        if recorded is None:  # this object's first call records the iteration into its graph: count what it launches
            with counted_launches() as recorded:
                loss = g()
            _assert_recorded(recorded, head_trains=freeze_after is None or it < freeze_after)
        else:
            with counted_launches() as replay:
                loss = g()
            assert replay == []  # (a replay goes through no entry point: the graph holds exactly what was counted)
        hip_loss.append(loss.clone())
        hip_sem.append(g.sem_loss.clone())
    torch.cuda.synchronize()
    hip_loss, hip_sem = [float(x) for x in hip_loss], [float(x) for x in hip_sem]
    hip_params = [p.detach().clone() for p in params]
    lout = [p for k, p in sem.named_parameters() if k.startswith("lout")]
    assert all(torch.equal(p, s) for p, s in zip(lout, start[-4:-2])), "the semantic decoder's lout never moves"

    # the same batches, eagerly: the fused query_feature -> sdf node, the head's composite, torch.optim.Adam
    cfg, params, _ = _loop_parts(wl, sem, start)
    opt = _make_opt(cfg, wl, sem, False)
    ref_loss, ref_sem = [], []
    for it, idx in enumerate(batches):
        if freeze_after is not None and it == freeze_after:
            _freeze(wl, sem)
            opt = _make_opt(cfg, wl, sem, False)
        coord, sdf_label, weight = pool.get_batch(idx)
        labels = pool.sem_label[idx.long()].long()
        feature = wl.octree.query_feature(coord)
        loss = sdf_bce_loss(wl.decoder.sdf(feature), sdf_label, cfg.sigma_sigmoid, torch.abs(weight), False, "mean")
        sem_loss = torch.nn.NLLLoss(reduction="mean")(sem._sem_composite(feature)[::d, :], labels[::d])
        opt.zero_grad(set_to_none=True)
        (loss + WEIGHT_S * sem_loss).backward()
        opt.step()
        ref_loss.append(float(loss.detach()))
        ref_sem.append(float(sem_loss.detach()))
    torch.cuda.synchronize()
    worst = max(abs(a - b) / max(abs(b), 1e-12) for a, b in zip(hip_loss + hip_sem, ref_loss + ref_sem))
    errs = [rel_err(a, b) for a, b in zip(hip_params, params)]
    print("freeze_after", freeze_after, "worst loss %.2e" % worst, "params", " ".join("%.1e" % e for e in errs))
    print("sem_loss %.4f -> %.4f" % (hip_sem[0], hip_sem[-1]))
    assert worst <= LOOP_TOL["loss"], (freeze_after, worst)
    assert max(errs) <= LOOP_TOL["params"], (freeze_after, errs)
    assert hip_sem[-1] < hip_sem[0]
    _loop_parts(wl, sem, start)


def test_unrolled_run_equals_single_calls(workload, loop_start):
    wl = workload
    sem, start = loop_start
    K = 5
    out = []
    for unroll in (1, 2):
        cfg, params, pool = _loop_parts(wl, sem, start)
        g = _graphed(cfg, wl, sem, pool, _make_opt(cfg, wl, sem, True), 1, eager_first=False, unroll=unroll)
        if unroll == 1:
            for _ in range(K):
                g()
        else:
            g.run(K)  # 2 x 2 + 1
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for p in params], g._idx.clone(), float(g.sem_loss), float(g.loss)))
    assert torch.equal(out[0][1], out[1][1])  # (the same batches were drawn)
    errs = [rel_err(a, b) for a, b in zip(out[1][0], out[0][0])]
    print("unrolled vs single:", " ".join("%.1e" % e for e in errs), out[0][2:], out[1][2:])
    assert max(errs) <= STEP_TOL, errs
    assert abs(out[0][2] - out[1][2]) <= STEP_TOL * abs(out[0][2])
    _loop_parts(wl, sem, start)


def test_without_sem_the_iteration_is_the_two_launch_native_graph(workload):
    from shine_mapping_amd import StepOptions, optim
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.sampler import SortedPool

    wl = workload
    start = [p.detach().clone() for p in list(wl.octree.hier_features) + list(wl.decoder.parameters())]
    cfg = copy.copy(wl.cfg)
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, 1.0
    opt = optim.setup_optimizer(cfg, list(wl.octree.parameters()), wl.decoder.fused_params())
    pool = SortedPool(wl.octree, wl.pool.coord, wl.pool.sdf_label, wl.pool.weight, seed=5)
    g = GraphedIteration(wl.octree, wl.decoder, pool, opt, StepOptions(sigma=cfg.sigma_sigmoid), N)
    assert g.native and not g.ran_eager and g.sem is None and g.sem_loss is None
    with counted_launches() as calls:
        g()
    torch.cuda.synchronize()
    # the two nodes of the library-built graph and nothing launched beside it
    assert [c[0] for c in calls] == ["shine_iter_graph_set_step", "shine_iter_graph_set_finish"], [c[0] for c in calls]
    assert g.graph is None and g.graph_k is None
    assert all(p.grad is None for p in wl.decoder.nclass_out.parameters())
    with torch.no_grad():
        for p, s in zip(list(wl.octree.hier_features) + list(wl.decoder.parameters()), start):
            p.copy_(s)
            p.grad = None


# ---- 8. the labelled dataset's pool
def test_dataset_pool_carries_the_labels_and_trains(tmp_path):
    from shine_mapping_amd import Decoder, FeatureOctree, StepOptions, optim, synth
    from shine_mapping_amd.dataset import LiDARDataset
    from shine_mapping_amd.loop import GraphedIteration, SemTerm

    base = synth.make_config("ncd", device="cuda")
    drive = synth.write_kitti_drive(str(tmp_path), base, frames=3, beams=16, azimuths=90, device="cpu", labels=True)
    cfg = synth.dataset_config("ncd", drive, pc_radius=20.0, min_range=2.5, semantic_on=True, bs=N)
    torch.manual_seed(1)
    octree = FeatureOctree(cfg)
    ds = LiDARDataset(cfg, octree)
    for f in range(3):
        ds.process_frame(f)
    sp = ds.sorted_pool()
    assert sp.sem_label.dtype == torch.int32 and sp.n_class == cfg.sem_class_count + 1
    assert torch.equal(sp.sem_label.long(), ds.sem_label_pool[sp.perm.long()].long())
    assert int(sp.sem_label.max()) > 0
    cfg.lr, cfg.adam_eps, cfg.opt_adam, cfg.lr_level_reduce_ratio = 0.01, 1e-15, True, 1.0
    torch.manual_seed(3)
    geo, sem = Decoder(cfg).cuda(), Decoder(cfg, is_geo_encoder=False).cuda()
    opt = optim.setup_optimizer(cfg, list(octree.parameters()), list(geo.parameters()), list(sem.parameters()), None)
    g = GraphedIteration(octree, geo, sp, opt, StepOptions(sigma=cfg.sigma_sigmoid), N, sem=SemTerm(sem, 1.0, 1))
    seen = [g.sem_loss.clone()]
    for _ in range(19):
        g()
        seen.append(g.sem_loss.clone())
    seen = [float(x) for x in seen]
    print("sem_loss over 20 iterations: %.4f -> %.4f" % (seen[0], seen[-1]))
    assert all(x == x and abs(x) != float("inf") for x in seen) and seen[-1] < seen[0]
