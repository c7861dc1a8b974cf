"""CPU suite: the oracle, pins, checkers and mutants of tests/finish_cases.py (the GPU runs are tests/test_gpu_finish.py), and the
host's refusals of shine_finish_iteration / shine_adam_step / shine_adam_step_dev.

(1) the oracle is right: its Adam equals torch.optim.Adam run in fp64 on the same inputs, its regulariser (value and gradient) the
    oracle's cal_regularization composite (oracle/shine_oracle.py) under autograd in fp64;
(2) the pins are honest: on every small case the fp32 CPU oracle's ratio is at most K / 4 in its family (the two large cases,
    10^6 and 4 x 10^6 rows, were measured once: the figures stand next to the pins);
(3) the checkers reject what they are for: each mutant of the oracle, with exactly one defect, breaks the rule on a named case;
(4) prepare_finish and adam_impl refuse bad arguments on the host, each in its own words, before any launch.
"""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

import finish_cases as fc

INVALID = -1  # SHINE_E_INVALID


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------------ (1) the oracle is right
def _close(what, a, b, scale):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    worst = float(((a - b).abs() - 1e-14 * scale.reshape(-1)).max()) if a.numel() else 0.0
    assert worst <= 0.0, "%s: the oracle and torch differ by more than 1e-14 of the element's scale" % what


def _unrounded(t):
    return 1.0 - fc.B1 ** t, math.sqrt(1.0 - fc.B2 ** t)


def _torch_adam64(c, ps, gs, ms, vs, lr):
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    for q, g in zip(params, gs):
        q.grad = g.clone()
    opt = torch.optim.Adam([{"params": [q], "lr": lr[s], "weight_decay": c.wd[s]} for s, q in enumerate(params)],
                           betas=(fc.B1, fc.B2), eps=c.eps, foreach=False)
    for q, m, v in zip(params, ms, vs):
        opt.state[q] = {"step": torch.tensor(float(c.t - 1), dtype=torch.float64), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    with torch.no_grad():
        opt.step()
    return [q.detach() for q in params], [opt.state[q]["exp_avg"] for q in params], [opt.state[q]["exp_avg_sq"] for q in params]


@pytest.mark.parametrize("name", ["mixed-sizes", "sixteen-segments"])
def test_the_oracles_adam_is_torchs_adam_in_fp64(name):
    c = fc.ADAM_CASES[name]
    T = fc.adam_build(c)
    lr = list(fc.LR_DEV[:c.n_tensors])
    ref = fc.adam_oracle(c, T, lr, bc=_unrounded(c.t))
    p, m, v = _torch_adam64(c, [x.double() for x in T.p], [x.double() for x in T.g], [x.double() for x in T.m],
                            [x.double() for x in T.v], lr)
    for s in range(c.n_tensors):
        _close("p[%d]" % s, ref.p[s], p[s], ref.sp[s] + ref.p[s].abs())
        _close("m[%d]" % s, ref.m[s], m[s], ref.sm[s])
        _close("v[%d]" % s, ref.v[s], v[s], ref.sv[s])


@pytest.mark.parametrize("name", [fc.MUTANT_CASE, fc.MUTANT_WD, "rows255x1-active"])
def test_the_oracles_tail_is_the_composite_and_torchs_adam_in_fp64(name):
    """g = S.g + the partial sums (+ d / dF of lambda x cal_regularization over the rows flagged with bit 0, by autograd), the trash
    rows zeroed, then torch.optim.Adam in fp64; the skipped rows of an active case are left out of the comparison's torch side"""
    from oracle import shine_oracle as so

    c, T, _ = fc.reference(name)
    ref = fc.oracle(c, T, bc=_unrounded(c.t))
    part = T.partials.double()
    ps, gs, value = [], [], torch.zeros((), dtype=torch.float64)
    feats = [T.p[s].double().view(-1, fc.F).clone().requires_grad_(True) for s in range(c.L)]
    if c.lam != 0.0:
        rows = [torch.nonzero(((T.flags[s] & 1) == 1)[:-1]).flatten() for s in range(c.L)]
        oct_ = SimpleNamespace(featured_level_num=c.L, hier_features=feats, hierarchical_indices=rows[::-1],  # (bottom-up)
                               features_last_frame=[x.double().view(-1, fc.F) for x in T.last],
                               importance_weight=[x.double().view(-1, fc.F) for x in T.imp])
        value = so.OracleOctree.cal_regularization(oct_)
        on = [f for s, f in enumerate(feats) if c.grad_on[s]]
        grads = dict(zip(map(id, on), torch.autograd.grad(c.lam * value, on, allow_unused=True)))
    for s in range(c.n_tensors):
        p, g = T.p[s].double().clone(), T.g[s].double().clone()
        if s < c.L:
            if c.lam != 0.0 and grads.get(id(feats[s])) is not None:
                g += grads[id(feats[s])].reshape(-1)
            g[-fc.F:] += part[:, fc.PART_TRASH + s * fc.F:fc.PART_TRASH + (s + 1) * fc.F].sum(0)
            p[-fc.F:] = 0.0
        else:
            g += part[:, fc.DEC_OFF[s - c.L]:fc.DEC_OFF[s - c.L] + p.numel()].sum(0)
        ps.append(p)
        gs.append(g)
    lr = [fc.LR_DEV[i] for i in fc.lr_index(c.n_tensors)]
    p, m, v = _torch_adam64(c, ps, gs, [x.double() for x in T.m], [x.double() for x in T.v], lr)
    assert abs(float(ref.reg) - T.reg_out0 - float(value.detach())) <= 1e-14 * float(ref.reg_scale)
    assert (c.lam != 0.0) == (float(ref.reg_scale) > 0.0)
    assert (c.mode == "active") == any(sk is not None and bool(sk.any()) for sk in T.skipped)
    for s in range(c.n_tensors):
        keep = torch.ones(ps[s].numel(), dtype=torch.bool)
        if s < c.L and T.skipped[s] is not None:
            keep = ~T.skipped[s][:, None].expand(-1, fc.F).reshape(-1)
        _close("p[%d]" % s, ref.p[s][keep], p[s][keep], (ref.sp[s] + ref.p[s].abs())[keep])
        _close("m[%d]" % s, ref.m[s][keep], m[s][keep], ref.sm[s][keep])
        _close("v[%d]" % s, ref.v[s][keep], v[s][keep], ref.sv[s][keep])


def test_the_inputs_are_what_the_rule_assumes():
    """gradients and partials from {0} u +-[2^-10, 2^4), a warm v >= 2^-20, half of the rows fresh, flags 0 / 1 / 2, poison on the
    skipped rows of an active case; the restated layout constants are consistent"""
    assert fc.DEC_OFF[-1] + fc.DEC_N[-1] == fc.MLP_PARAMS == fc.PART_TRASH and sum(fc.DEC_N) == fc.MLP_PARAMS
    assert fc.PART_TRASH + fc.MAX_LEVELS * fc.F <= fc.PART_LOSS and fc.PART_LOSS % 2 == 0 and fc.PART_LOSS + 8 <= fc.PART_STRIDE
    for name in (fc.MUTANT_CASE, "rows1x63x64x1000-active", "nblocks7"):
        c, T, _ = fc.reference(name)
        used = fc.MLP_PARAMS + c.L * fc.F
        for x in [T.partials[:, :used]] + T.g:
            a = x[(x != 0) & (x != fc.POISON)].abs()
            assert a.numel() == 0 or (float(a.min()) >= 2.0 ** -10 and float(a.max()) < 2.0 ** 4)
        for s in range(c.L):
            v = T.v[s][T.v[s] != fc.POISON]
            assert not bool(((v > 0) & (v < 2.0 ** -20)).any())
        if c.mode != "none":
            assert set(T.flags[c.L - 1].tolist()) == {0, 1, 2} and int(T.flags[c.L - 1][-1]) == 0
        fresh = (T.v[c.L - 1].view(-1, fc.F) == 0).all(1).float().mean()
        assert 0.3 < float(fresh) < 0.7
    c, T, _ = fc.reference("rows1x63x64x1000-active")
    sk = T.skipped[c.L - 1]
    assert int(sk.sum()) > 100 and bool((T.p[c.L - 1].view(-1, fc.F)[sk] == fc.POISON).all())
    assert {c.family for c in fc.CASES.values()} == {"same", "mixed", "exact"}
    assert {c.t for c in fc.CASES.values()} == set(fc.TS) and {c.eps for c in fc.CASES.values()} == {fc.f32(1e-15), fc.f32(1e-8)}


# ----------------------------------------------------------------------------------------------------------------- (2) the pins
def test_pins_follow_the_rule():
    assert fc.K == {fam: 4.0 * max(rho, 1.0) for fam, rho in fc.RHO_REF.items()}
    assert all(rho * 2 == int(rho * 2) for rho in fc.RHO_REF.values())  # halves


@pytest.mark.parametrize("name", fc.SMALL)
def test_tail_pins_are_honest(name, one_thread):
    c, T, ref = fc.reference(name)
    rho = fc.check_case("fp32 oracle, " + name, c, fc.oracle32(c, T), ref)
    fc.record("finish/" + name, "cpu32", rho)
    for fam, v in rho.items():
        assert v <= fc.K[fam] / 4.0, "%s: the fp32 oracle's ratio %.3f exceeds K / 4 of %s" % (name, v, fam)


@pytest.mark.parametrize("name", fc.ADAM_SMALL)
def test_adam_pins_are_honest(name, one_thread):
    c = fc.ADAM_CASES[name]
    T = fc.adam_build(c)
    lr = list(fc.LR_DEV[:c.n_tensors])
    rho = fc.check_case("fp32 oracle, " + name, c, fc.adam_oracle32(c, T, lr), fc.adam_oracle(c, T, lr), adam_only=True)
    fc.record("adam/" + name, "cpu32", rho)
    for fam, v in rho.items():
        assert v <= fc.K[fam] / 4.0, "%s: the fp32 oracle's ratio %.3f exceeds K / 4 of %s" % (name, v, fam)


# ------------------------------------------------------------------------------------------------------------- (3) the mutants
MUTANT_ON = {
    "last block dropped": fc.MUTANT_BLOCKS,
    "blocks below 8 floor(nblocks / 8) only": fc.MUTANT_BLOCKS,
    "trash row not zeroed": fc.MUTANT_CASE,
    "trash row regularised": fc.MUTANT_CASE,
    "bias corrections of step t - 1": fc.MUTANT_CASE,
    "gradient factor lambda": fc.MUTANT_CASE,
    "regulariser on flag-2 rows": fc.MUTANT_CASE,
    "decoupled weight decay": fc.MUTANT_WD,
    "lr_index ignored": fc.MUTANT_CASE,
    "eikonal over n": fc.MUTANT_BLOCKS,
    "row off by one at a level boundary": fc.MUTANT_CASE,
}


def test_every_mutant_is_named():
    assert set(MUTANT_ON) == set(fc.MUTANTS)


@pytest.mark.parametrize("mutant", fc.MUTANTS)
def test_a_mutant_of_the_oracle_breaks_the_rule(mutant):
    c, T, ref = fc.reference(MUTANT_ON[mutant])
    fc.check_case("unmutated", c, fc.round32(ref), ref)  # the oracle itself, rounded to fp32, passes
    bad = fc.round32(fc.oracle(c, T, mutant=mutant))
    bad.g, bad.flags = [None] * c.n_tensors, None  # (the rule alone has to reject it: p, m, v, reg_out, loss_parts)
    with pytest.raises(AssertionError, match="2\\^-24 scale off"):
        fc.check_case(mutant, c, bad, ref)


def test_the_checker_wants_poison_grads_and_flags_back():
    c, T, ref = fc.reference("rows1x63x64x1000-active")
    good = fc.round32(ref)
    fc.check_case("unmutated", c, good, ref)
    s = c.L - 1
    row = int(torch.nonzero(T.skipped[s])[0])
    for field in ("p", "m", "v"):
        bad = fc.round32(ref)
        getattr(bad, field)[s] = getattr(bad, field)[s].clone()
        getattr(bad, field)[s][row * fc.F + 3] = 0.0  # a skipped row written
        with pytest.raises(AssertionError):
            fc.check_case("skipped row", c, bad, ref)
    bad = fc.round32(ref)
    bad.g = [g.clone() for g in ref.g]
    bad.g[s][row * fc.F] = 0.0
    with pytest.raises(AssertionError, match="grads"):
        fc.check_case("skipped grad", c, bad, ref)
    bad = fc.round32(ref)
    bad.flags = [f.clone() for f in ref.flags]
    bad.flags[s][int(torch.nonzero(ref.flags[s] == 2)[0])] = 1
    with pytest.raises(AssertionError, match="flags"):
        fc.check_case("flag left at 1", c, bad, ref)


# --------------------------------------------------------------------------------------------------------- (4) the host's refusals
FAKE = 0x10000  # a 16-byte aligned non-null address; nothing is dereferenced before the refusals


def _finish(L=3, n_tensors=None, numel=None, variant=0, eik=0, lam=0.0, active=0, n=64, **over):
    """shine_finish_iteration on fake non-null pointers -> (rc, message)"""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    nt = L + 6 if n_tensors is None else n_tensors
    if callable(numel):
        over["numel"], numel = numel, None
    numel = list(numel) if numel is not None else [16, 24, 32, 40][:max(0, min(L, 4))] + list(fc.DEC_N)
    numel = (numel + [8] * 16)[:max(nt, 1)]
    cfg = _lib.StepConfig(n_levels=L, max_level=12, kernel_variant=variant, eikonal_on=eik, inv_n=1.0 / 64,
                          n_surf_parts=over.pop("n_surf_parts", 0))
    ptrs = lambda: _lib.ptr_array([FAKE] * max(nt, 1))
    lv = lambda: _lib.ptr_array([FAKE] * 8)
    a = dict(cfg=C.byref(cfg), n=n, workspace=C.c_void_p(FAKE), n_surf=None, loss_parts=C.c_void_p(FAKE), feats_last=None,
             importance=None, touched=None, grad_on=None, lam=lam, reg_out=None, n_tensors=nt, params=ptrs(), grads=ptrs(),
             exp_avg=ptrs(), exp_avg_sq=ptrs(), numel=_lib.i64_array(numel), lr_dev=C.c_void_p(FAKE),
             lr_index=(C.c_int32 * max(nt, 1))(*range(max(nt, 1))), weight_decay=(C.c_float * max(nt, 1))(), b1=0.9, b2=0.99,
             eps=1e-15, step_state=C.c_void_p(FAKE), next_draw=None, active=active, stream=None)
    if lam != 0.0:
        a.update(feats_last=lv(), importance=lv(), touched=lv(), reg_out=C.c_void_p(FAKE))
    if active:
        a.update(touched=lv())
    for k, v in over.items():
        a[k] = v(a, _lib) if callable(v) else v
    rc = lib.shine_finish_iteration(*a.values())
    return rc, (lib.shine_error_string(rc) or b"").decode()


def _set(key, index, value):
    """an override that changes one entry of an array argument"""
    def f(a, _lib):
        arr = a[key]
        arr[index] = value
        return arr
    return f


def _draw(n):
    def f(a, _lib):
        f.keep = _lib.NextDraw(pool_size=1000, n=n, seed=1, stream_state=FAKE, idx_out=FAKE)
        return C.pointer(f.keep)
    return f


FINISH_REFUSALS = [
    (dict(cfg=None), "null argument"),
    (dict(n=0), "null argument"),
    (dict(workspace=None), "null argument"),
    (dict(params=None), "null argument"),
    (dict(lr_index=None), "null argument"),
    (dict(step_state=None), "null argument"),
    (dict(L=0), "1..4 featured levels"),
    (dict(L=5), "1..4 featured levels"),
    (dict(n_tensors=4), "tensors = the L feature tables"),
    (dict(n_tensors=8), "tensors = the L feature tables"),
    (dict(variant=1), "follows the product kernel"),
    (dict(eik=1), "eikonal needs n_surf"),
    (dict(lam=1.0, feats_last=None), "the regulariser needs feats_last, importance, touched, reg_out"),
    (dict(lam=1.0, importance=None), "the regulariser needs feats_last, importance, touched, reg_out"),
    (dict(lam=1.0, touched=None), "the regulariser needs feats_last, importance, touched, reg_out"),
    (dict(lam=1.0, reg_out=None), "the regulariser needs feats_last, importance, touched, reg_out"),
    (dict(active=1, touched=None), "active_rows needs the touched-row flags"),
    (dict(grads=_set("grads", 4, None)), "null tensor"),
    (dict(numel=_set("numel", 2, -8)), "null tensor"),
    (dict(lr_index=_set("lr_index", 1, 16)), "bad lr_index"),
    (dict(lr_index=_set("lr_index", 8, -1)), "bad lr_index"),
    (dict(numel=[16, 20, 32]), "feature tables are [rows + 1][8] floats"),
    (dict(numel=[16, 0, 32]), "feature tables are [rows + 1][8] floats"),
    (dict(exp_avg=_set("exp_avg", 0, FAKE + 4)), "feature tables are [rows + 1][8] floats, 16-byte aligned"),
    (dict(active=1, touched=_set("touched", 1, None)), "active_rows needs flags for every level"),
    (dict(active=1, weight_decay=_set("weight_decay", 2, 1e-4)), "exact only without weight decay"),
    (dict(lam=1.0, importance=_set("importance", 2, None)), "null or unaligned regulariser tensor"),
    (dict(lam=1.0, feats_last=_set("feats_last", 0, FAKE + 8)), "null or unaligned regulariser tensor"),
    (dict(lam=1.0, touched=_set("touched", 1, None)), "null or unaligned regulariser tensor"),
    (dict(numel=[16, 24, 32, 256, 32, 1024, 32, 32, 2]), "decoder tensors are W1, b1, W2, b2, w3, b3"),
    (dict(numel=[16, 24, 32, 256, 33, 1024, 32, 32, 1]), "decoder tensors are W1, b1, W2, b2, w3, b3"),
    (dict(n_surf_parts=65), "at most 64 n_surf parts"),
    (dict(next_draw=_draw(16384)), "next_draw wants 1 <= n < 16 K draws"),
    (dict(next_draw=_draw(0)), "next_draw wants 1 <= n < 16 K draws"),
]


@pytest.mark.parametrize("over,text", FINISH_REFUSALS, ids=["%02d-%s" % (i, t[:28]) for i, (_, t) in enumerate(FINISH_REFUSALS)])
def test_shine_finish_iteration_refuses_on_the_host(over, text):
    rc, msg = _finish(**over)
    assert rc == INVALID and msg.startswith("shine_finish_iteration: ") and text in msg, (rc, msg)


def _adam(dev=False, n_tensors=3, numel=(0, 0, 0), wd=(0.0, 0.0, 0.0), flags=None, **over):
    """shine_adam_step / _dev on fake non-null pointers -> (rc, message); the tensors are empty wherever the refusal under test
    does not need a size"""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    ptrs = lambda: _lib.ptr_array([FAKE] * max(n_tensors, 1))
    if callable(numel):
        over["numel"], numel = numel, (0, 0, 0)
    numel = (list(numel) + [0] * 32)[:max(n_tensors, 1)]
    wd = (list(wd) + [0.0] * 32)[:max(n_tensors, 1)]
    a = dict(n_tensors=n_tensors, params=ptrs(), grads=ptrs(), exp_avg=ptrs(), exp_avg_sq=ptrs(), numel=_lib.i64_array(numel),
             lr=C.c_void_p(FAKE) if dev else (C.c_float * max(n_tensors, 1))(), weight_decay=(C.c_float * max(n_tensors, 1))(*wd),
             b1=0.9, b2=0.99, eps=1e-15, step=C.c_void_p(FAKE) if dev else 1, zero_grad=1,
             row_flags=None if flags is None else _lib.ptr_array(flags), stream=None)
    for k, v in over.items():
        a[k] = v(a, _lib) if callable(v) else v
    rc = (lib.shine_adam_step_dev if dev else lib.shine_adam_step)(*a.values())
    return rc, (lib.shine_error_string(rc) or b"").decode()


ADAM_REFUSALS = [
    (dict(n_tensors=17), "shine_adam_step: bad argument"),
    (dict(n_tensors=0), "shine_adam_step: bad argument"),
    (dict(step=0), "shine_adam_step: bad argument"),
    (dict(step=-3), "shine_adam_step: bad argument"),
    (dict(lr=None), "shine_adam_step: bad argument"),
    (dict(weight_decay=None), "shine_adam_step: bad argument"),
    (dict(exp_avg_sq=_set("exp_avg_sq", 1, None)), "shine_adam_step: null tensor"),
    (dict(numel=_set("numel", 0, -1)), "shine_adam_step: null tensor"),
    (dict(numel=(8, 16, 5), flags=[None, None, FAKE]), "row_flags are for [rows, 8] feature tables without weight decay"),
    (dict(numel=(8, 16, 5), flags=[FAKE, None, None], wd=(1e-7, 0.0, 0.0)), "row_flags are for [rows, 8] feature tables without weight decay"),
    (dict(dev=True, n_tensors=17), "shine_adam_step: bad argument"),
    (dict(dev=True, lr=None), "shine_adam_step_dev: null lr_dev/step_state"),
    (dict(dev=True, step=None), "shine_adam_step_dev: null lr_dev/step_state"),
    (dict(dev=True, numel=(8, 16, 5), flags=[None, None, FAKE]), "row_flags are for [rows, 8] feature tables without weight decay"),
]


@pytest.mark.parametrize("over,text", ADAM_REFUSALS, ids=["%02d-%s" % (i, t[-30:]) for i, (_, t) in enumerate(ADAM_REFUSALS)])
def test_shine_adam_step_refuses_on_the_host(over, text):
    rc, msg = _adam(**over)
    assert rc == INVALID and text in msg, (rc, msg)


def test_an_empty_adam_call_launches_nothing():
    rc, _ = _adam()  # (three empty tensors)
    assert rc == 0


def test_the_workspace_holds_the_wanted_number_of_partial_vectors():
    """nblocks is not restated: it is what shine_train_step_workspace_bytes answers for the case's n"""
    from shine_mapping_amd import _lib

    seen = set()
    for c in fc.CASES.values():
        if c.variant:  # (the deterministic bit: one workgroup at any n, decided in the launch)
            assert c.variant == 0x4000 and c.nblocks == 1
            continue
        cfg = _lib.StepConfig(n_levels=c.L, kernel_variant=c.variant)
        got = int(_lib.lib().shine_train_step_workspace_bytes(C.byref(cfg), c.n)) // (fc.PART_STRIDE * 4)
        assert got == c.nblocks, (c.name, got)
        seen.add(c.nblocks)
    assert seen >= set(fc.NBLOCKS)
