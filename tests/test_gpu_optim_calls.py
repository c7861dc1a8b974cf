"""GPU: what FusedAdam (shine_mapping_amd/optim.py) hands each entry point — shine_adam_step, the extension's adam_step,
shine_adam_step_dev, shine_finish_iteration.  The entry points are intercepted the way tests/test_gpu_sem_step.py counts
launches and the real call still runs; the library's arithmetic behind these arguments is tests/test_gpu_finish.py's subject."""
import ctypes as C

import pytest
import torch

from conftest import load_golden, product_from_golden
from test_gpu_sem_step import counted_launches

pytestmark = pytest.mark.gpu

LR, WD, TABLE_LRS, BETAS, EPS = 0.01, 1e-3, (0.02, 0.005), (0.9, 0.99), 1e-15
DECODER_SHAPES = [(32, 8), (32,), (32, 32), (32,), (1, 32), (1,)]
TABLE_SHAPES = [(5, 8), (9, 8)]


def f32(x):
    return C.c_float(x).value


def _optimizer():
    """six decoder-shaped tensors in one group with weight decay, two tables in a group each; seeded random grads"""
    from shine_mapping_amd.optim import FusedAdam

    gen = torch.Generator(device="cuda").manual_seed(3)
    rand = lambda shape: torch.randn(shape, device="cuda", generator=gen)
    tensors = [torch.nn.Parameter(rand(s)) for s in DECODER_SHAPES + TABLE_SHAPES]
    for p in tensors:
        p.grad = rand(p.shape)
    groups = [{"params": tensors[:6], "lr": LR, "weight_decay": WD}]
    groups += [{"params": [t], "lr": lr} for t, lr in zip(tensors[6:], TABLE_LRS)]
    return FusedAdam(groups, betas=BETAS, eps=EPS), tensors


def _assert_arrays(args, opt, sel):
    """args[0:6] of the three Adam entry points: n, then p / grad / exp_avg / exp_avg_sq pointers and the element counts"""
    n = len(sel)
    assert args[0] == n
    assert [args[1][i] for i in range(n)] == [p.data_ptr() for p in sel]
    assert [args[2][i] for i in range(n)] == [p.grad.data_ptr() for p in sel]
    assert [args[3][i] for i in range(n)] == [opt.state[p][0].data_ptr() for p in sel]
    assert [args[4][i] for i in range(n)] == [opt.state[p][1].data_ptr() for p in sel]
    assert [args[5][i] for i in range(n)] == [p.numel() for p in sel]


def _assert_eager(call, opt, sel, lrs, wds, step, zero, flags=None):
    name, a = call
    assert name == "shine_adam_step"
    _assert_arrays(a, opt, sel)
    n = len(sel)
    assert [a[6][i] for i in range(n)] == [f32(x) for x in lrs] and [a[7][i] for i in range(n)] == [f32(x) for x in wds]
    assert (a[8], a[9], a[10], a[11], a[12]) == (BETAS[0], BETAS[1], EPS, step, zero)
    if flags is None:
        assert a[13] is None
    else:
        assert [a[13][i] for i in range(n)] == flags


# ------------------------------------------------------------------------------------------------- (a) eager, ctypes path
def test_eager_steps_through_the_c_abi(monkeypatch):
    monkeypatch.setenv("SHINE_TIER_A_EXT", "0")
    opt, ts = _optimizer()
    lrs, wds = [LR] * 6 + list(TABLE_LRS), [WD] * 6 + [0.0, 0.0]
    with counted_launches() as calls:
        opt.step()
        opt.step(zero_grad=True)
    assert len(calls) == 2
    _assert_eager(calls[0], opt, ts, lrs, wds, 1, 0)
    _assert_eager(calls[1], opt, ts, lrs, wds, 2, 1)
    # row_flags: the tables' flag pointers, NULL for the decoder tensors
    flags = {t: torch.ones(t.shape[0], dtype=torch.uint8, device="cuda") for t in ts[6:]}
    with counted_launches() as calls:
        opt.step(row_flags=flags)
    assert len(calls) == 1
    _assert_eager(calls[0], opt, ts, lrs, wds, 3, 0, flags=[None] * 6 + [flags[t].data_ptr() for t in ts[6:]])
    # a tensor without grad for one step is one step younger afterwards: one launch per age, in age order, each with age + 1
    held, ts[1].grad = ts[1].grad, None
    rest = ts[:1] + ts[2:]
    with counted_launches() as calls:
        opt.step()
        ts[1].grad = held
        opt.step()
    torch.cuda.synchronize()
    assert len(calls) == 3
    _assert_eager(calls[0], opt, rest, lrs[:1] + lrs[2:], wds[:1] + wds[2:], 4, 0)
    _assert_eager(calls[1], opt, [ts[1]], [LR], [WD], 4, 0)
    _assert_eager(calls[2], opt, rest, lrs[:1] + lrs[2:], wds[:1] + wds[2:], 5, 0)
    assert opt.step_count == 5 and opt._age[ts[1]] == 4 and opt._age[ts[0]] == 5


# ---------------------------------------------------------------------------------------------- (b) eager, extension path
def test_eager_steady_state_goes_through_the_extension(monkeypatch):
    from shine_mapping_amd import _ext

    monkeypatch.setenv("SHINE_TIER_A_EXT", "1")
    ext = _ext.module()
    if ext is None:
        pytest.skip("lib/_shine_ext.so not built")
    opt, ts = _optimizer()
    real, seen, general = ext.adam_step, [], []
    monkeypatch.setattr(ext, "adam_step", lambda *a: (seen.append(a), real(*a))[1])
    launch = opt._launch
    monkeypatch.setattr(opt, "_launch", lambda *a, **k: (general.append(a), launch(*a, **k))[1])
    with counted_launches() as calls:
        opt.step()
        opt.step(zero_grad=True)
        opt.step()
    torch.cuda.synchronize()
    assert calls == [] and len(seen) == 3 and len(general) == 1  # (the first step alone takes the general path)
    for k, zero in ((1, True), (2, False)):
        params, grads, m, v, lrs, wds, b1, b2, eps, step, zero_grad, flags = seen[k]
        assert len(params) == 8 and all(a is b for a, b in zip(params, ts))
        assert all(g is p.grad for g, p in zip(grads, ts))
        assert all(a is opt.state[p][0] and b is opt.state[p][1] for a, b, p in zip(m, v, ts))
        assert list(lrs) == [LR] * 6 + list(TABLE_LRS) and list(wds) == [WD] * 6 + [0.0, 0.0]
        assert (b1, b2, eps, step, zero_grad, flags) == (BETAS[0], BETAS[1], EPS, k + 1, zero, [])
    assert opt.step_count == 3 and all(opt._age[p] == 3 for p in ts)


# ------------------------------------------------------------------------------------------------ (c) graph-replayable steps
def test_graph_safe_steps_read_the_device_state():
    opt, ts = _optimizer()
    with counted_launches() as calls:
        opt.step(graph_safe=True, zero_grad=True)
        opt.step(graph_safe=True, zero_grad=True, advanced=True)
        opt.step_tensors_dev(ts[2:4])
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["shine_adam_step_dev"] * 3
    state, lr = opt.device_state(), opt._dev[1]
    assert lr.cpu().tolist() == [f32(x) for x in [LR] * 6 + list(TABLE_LRS)]
    for (_, a), sel, lr_ptr, bits in ((calls[0], ts, lr.data_ptr(), 1), (calls[1], ts, lr.data_ptr(), 3),
                                      (calls[2], ts[2:4], lr.data_ptr() + 4 * 2, 3)):
        _assert_arrays(a, opt, sel)
        assert a[6] == lr_ptr and a[11] == state.data_ptr() and a[12] == bits and a[13] is None
        assert [a[7][i] for i in range(len(sel))] == [f32(WD if any(p is q for q in ts[:6]) else 0.0) for p in sel]
        assert (a[8], a[9], a[10]) == (BETAS[0], BETAS[1], EPS)
    assert int(state[0]) == 1  # (the first launch counted its step; `advanced` and step_tensors_dev leave the counter alone)


# --------------------------------------------------------------------------------------------------- (d) the iteration tail
def test_finish_iteration_selects_tables_then_decoder():
    from shine_mapping_amd import StepOptions, dp, fused_train_step, ops
    from shine_mapping_amd.optim import FusedAdam

    fx = load_golden("linear_L2_nopoly")
    cfg, octree, dec = product_from_golden(fx)
    dec = dec.cuda()
    tables, six = list(octree.hier_features), dec.fused_params()
    L = len(tables)
    extra = [torch.nn.Parameter(torch.zeros(4, device="cuda")), torch.nn.Parameter(torch.zeros(3, device="cuda"))]
    # setup_optimizer's order with a second decoder-like group in between: decoder, extra, then the levels leaf first
    groups = [{"params": six, "lr": LR, "weight_decay": WD}, {"params": extra, "lr": LR, "weight_decay": 2 * WD}]
    groups += [{"params": [tables[L - 1 - i]], "lr": LR * 0.5 ** i} for i in range(L)]
    opt = FusedAdam(groups, betas=BETAS, eps=EPS)
    opt.prepare_graph_safe()
    stepped = [p for g in opt.param_groups for p in g["params"]]
    position = lambda p: next(i for i, q in enumerate(stepped) if q is p)
    coord, label, weight = fx["coord"][:64].cuda(), fx["sdf_label"][:64].cuda(), fx["weight"][:64].cuda()
    perm, slots = dp.plan_batch(octree, coord)
    c = fx["cfg"]
    opts = StepOptions(sigma=fx["sigma"], loss_reduction=c.get("loss_reduction", "mean"),
                       ekional_loss_on=c.get("ekional_loss_on", False), weight_e=c.get("weight_e", 0.1),
                       adam_state=opt.device_state(), adam_betas=BETAS)
    touched = ops.touched_flags(octree)
    order = tables + six
    for it, active in enumerate((None, touched)):
        pending = {}
        fused_train_step(octree, dec, coord, label, weight, opts, perm=perm, slots=slots, touched=touched, pending=pending)
        with counted_launches() as calls:
            opt.finish_iteration(pending, active_flags=active, others=extra)
        torch.cuda.synchronize()
        assert [name for name, _ in calls] == ["shine_finish_iteration"]
        a = calls[0][1]
        n = L + 6
        assert a[11] == n
        _assert_arrays(a[11:17], opt, order)
        assert a[17] == opt._dev[1].data_ptr() and a[23] == opt.device_state().data_ptr()
        assert [a[18][i] for i in range(n)] == [position(p) for p in order]
        assert [a[19][i] for i in range(n)] == [0.0] * L + [f32(WD)] * 6
        assert (a[20], a[21], a[22]) == (BETAS[0], BETAS[1], EPS)
        assert a[25] == (0 if active is None else 1)
        if active is None:
            assert a[7] is None
        else:
            assert [a[7][i] for i in range(L)] == [f.data_ptr() for f in touched]
        assert int(opt.device_state()[0]) == it + 1  # (the fused step counted it)
        assert all(not p.grad.any() for p in order)  # (the tail cleared the grads it stepped)
