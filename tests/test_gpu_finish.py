"""GPU suite (-m gpu): the iteration tail (shine_finish_iteration, k_finish) and the fused Adam (shine_adam_step / _dev, k_adam)
element by element against fp64 (tests/finish_cases.py has the cases, the oracle, the scales, the K of every family and the
checkers; tests/test_finish.py shows on the CPU that they reject wrong results).

(a) shine_finish_iteration through the C ABI on inputs the test writes — partial vectors, step state, learning rates, flags: no
    octree, no fused step.  Every tensor sits between two 256-float guards whose pattern must survive the launch.
(b) the same launch with next_draw: the draw is shine_sample_sorted_dev's, everything else is bit-identical.
(c) shine_adam_step / shine_adam_step_dev on the Adam cases; the device step state's bias corrections over consecutive launches.
(d) the decoder's operand image the tail keeps current equals the one k_operand_image rebuilds.
(e) the layout the cases restate is the layout the fused step writes with defer_reduce.
"""
import ctypes as C
import math

import pytest
import torch

import finish_cases as fc
from conftest import load_golden, product_from_golden

pytestmark = pytest.mark.gpu

GUARD = 256
PATTERN = 7.0e22  # what the guards hold; nothing here produces it


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    yield
    fc.forget()
    torch.cuda.empty_cache()


class Buf:
    """a device copy of `x` with GUARD elements of PATTERN either side; offset: extra floats in front (a misaligned tensor)"""

    def __init__(self, x, offset=0):
        n = x.numel()
        pat = PATTERN if x.dtype.is_floating_point else 0x5A
        self.flat = torch.full((n + 2 * GUARD + offset,), pat, dtype=x.dtype, device="cuda")
        self.lo = GUARD + offset
        self.t = self.flat[self.lo:self.lo + n]
        self.t.copy_(x.reshape(-1))
        self.pat = pat

    def ptr(self):
        return self.t.data_ptr() if self.t.numel() else self.flat.data_ptr() + self.lo * self.flat.element_size()

    def result(self):
        n = self.t.numel()
        assert bool((self.flat[:self.lo] == self.pat).all()) and bool((self.flat[self.lo + n:] == self.pat).all()), \
            "a write outside a tensor"
        return self.t.clone()


def _stream():
    from shine_mapping_amd import _lib

    return _lib.current_stream_handle()


def _step_state(t, bc=None):
    """device int64[8]: [0] = t, the two bias-correction floats at [1] (bc = None: zero, with zero running products)"""
    st = torch.zeros(8, dtype=torch.int64)
    st[0] = t
    if bc is not None:
        st[1:2].view(torch.float32).copy_(torch.tensor(bc, dtype=torch.float32))
    return st.cuda()


# ------------------------------------------------------------------------------------------- (a) shine_finish_iteration, C ABI
def run_finish(c, T, next_draw=None, loss_null=False):
    """one launch of case `c` on copies of its inputs -> what fc.check_case judges (tensors on the device)"""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    cfg = _lib.StepConfig(n_levels=c.L, max_level=12, reduction_sum=c.reduction_sum, eikonal_on=c.eik, kernel_variant=c.variant,
                          inv_n=1.0 / c.n, weight_e=c.weight_e, n_global=c.n)
    assert c.variant or int(lib.shine_train_step_workspace_bytes(C.byref(cfg), c.n)) // (fc.PART_STRIDE * 4) == c.nblocks
    assert tuple(T.partials.shape) == (c.nblocks, fc.PART_STRIDE)
    B = {k: [Buf(x) for x in getattr(T, k)] for k in "pgmv"}
    flags = [None if f is None else Buf(f) for f in T.flags]
    state = _step_state(c.t, fc.bias_corrections(c.t))
    lr_dev = torch.tensor(fc.LR_DEV, dtype=torch.float32).cuda()
    n_surf = torch.full((64,), 123456, dtype=torch.int64, device="cuda") if c.eik else None  # (the count comes from workgroup 0)
    loss = None if loss_null else torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    reg_out = torch.full((1,), T.reg_out0, dtype=torch.float64, device="cuda")
    reg = c.lam != 0.0
    ptrs = lambda xs: _lib.ptr_array([None if x is None else x.ptr() if isinstance(x, Buf) else x.data_ptr() for x in xs])
    _lib.check(lib.shine_finish_iteration(
        C.byref(cfg), c.n, T.partials.data_ptr(), n_surf.data_ptr() if c.eik else None, None if loss_null else loss.data_ptr(),
        ptrs(T.last) if reg else None, ptrs(T.imp) if reg else None, ptrs(flags) if c.mode != "none" else None,
        (C.c_int32 * c.L)(*c.grad_on) if reg else None, c.lam, reg_out.data_ptr() if reg else None, c.n_tensors,
        ptrs(B["p"]), ptrs(B["g"]), ptrs(B["m"]), ptrs(B["v"]), _lib.i64_array(c.numel), lr_dev.data_ptr(),
        (C.c_int32 * c.n_tensors)(*fc.lr_index(c.n_tensors)), (C.c_float * c.n_tensors)(*c.wd), fc.B1, fc.B2, c.eps,
        state.data_ptr(), C.byref(next_draw) if next_draw is not None else None, 1 if c.mode == "active" else 0, _stream()),
        "shine_finish_iteration")
    torch.cuda.synchronize()
    from types import SimpleNamespace

    return SimpleNamespace(p=[b.result() for b in B["p"]], m=[b.result() for b in B["m"]], v=[b.result() for b in B["v"]],
                           g=[b.result() for b in B["g"]], flags=[None if f is None else f.result() for f in flags]
                           if c.mode != "none" else None, reg=float(reg_out), loss=loss)


def _ids(names):
    return [n.replace(" ", "_") for n in names]


@pytest.mark.parametrize("name", list(fc.CASES), ids=_ids(fc.CASES))
def test_the_tail_matches_fp64_on_every_element(name):
    """every case of fc.CASES: levels and rows, lane slots 1..3 and the second pass of the row loop, every nblocks, flags and modes
    (dense, dense with flags, active with poisoned skipped rows), the Adam scalars, the loss block"""
    c, T, ref = fc.reference(name, "cuda")
    got = run_finish(c, T)
    rho = fc.check_case(name, c, got, ref)
    fc.record("finish/" + name, "hip", rho)
    if not c.eik or c.n_surf == 0:
        assert float(got.loss[1]) == 0.0  # no eikonal term without surface samples
    if c.mode == "dense":
        assert all(int(f.sum()) == 0 for f in got.flags)
    if c.mode == "active":
        assert all(set(f.unique().tolist()) <= {0, 2} for f in got.flags)


def test_loss_parts_may_be_null():
    c, T, ref = fc.reference(fc.MUTANT_CASE, "cuda")
    got = run_finish(c, T, loss_null=True)
    assert got.loss is None
    fc.check_case("loss_parts = NULL", c, got, ref)


# -------------------------------------------------------------------------------------------------------- (b) with next_draw
POOL = 100003
DRAW_SEED = 20240611


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 16383])
def test_the_tails_next_draw_is_the_samplers_and_changes_nothing_else(n):
    """idx_out, the advanced stream state and surf_parts equal shine_sample_sorted_dev's with the same seed and stream id, bit for
    bit; every Adam and loss output and every flag is bit-identical to the launch without next_draw (the block index remap).
    reg_out is the sum of the row blocks' fp64 atomics, in the order they arrive: bit-identical where one row block adds to it
    ("one-row-block"), held to the rule where five do."""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    bits = (fc.choice(77, (POOL + 31) // 32, "cuda", 1 << 24) * 251 + 13).to(torch.int32)

    def fresh():
        return (torch.tensor([5, 0, 5, 0], dtype=torch.int64).cuda(), torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                torch.zeros(64, dtype=torch.int64, device="cuda"))

    state1, idx1, parts1 = fresh()
    need = C.c_size_t(0)
    _lib.check(lib.shine_sample_sorted_dev(POOL, n, DRAW_SEED, state1.data_ptr(), idx1.data_ptr(), None, 0, bits.data_ptr(),
                                           parts1.data_ptr(), None, C.byref(need), _stream()), "size query")
    ws = _lib.workspace(need.value, "cuda")
    _lib.check(lib.shine_sample_sorted_dev(POOL, n, DRAW_SEED, state1.data_ptr(), idx1.data_ptr(), None, 0, bits.data_ptr(),
                                           parts1.data_ptr(), ws.data_ptr(), C.byref(need), _stream()), "shine_sample_sorted_dev")
    torch.cuda.synchronize()
    assert int(idx1.min()) >= 0 and int(idx1.max()) < POOL and bool((idx1[1:] >= idx1[:-1]).all()) and int(state1[0]) != 5
    for name in ("rows1x63x64x1000-active", "one-row-block"):
        c, T, ref = fc.reference(name, "cuda")
        state2, idx2, parts2 = fresh()
        nd = _lib.NextDraw(pool_size=POOL, n=n, seed=DRAW_SEED, stream_state=state2.data_ptr(), idx_out=idx2.data_ptr(),
                           surf_bits=bits.data_ptr(), surf_parts=parts2.data_ptr())
        with_draw = run_finish(c, T, next_draw=nd)
        plain = run_finish(c, T)
        assert torch.equal(idx1, idx2) and torch.equal(parts1, parts2)
        assert int(state1[0]) == int(state2[0]) and int(state1[2]) == int(state2[2])
        for k in "pmvg":
            for a, b in zip(getattr(with_draw, k), getattr(plain, k)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert all(torch.equal(a, b) for a, b in zip(with_draw.flags, plain.flags))
        assert torch.equal(with_draw.loss.view(torch.int64), plain.loss.view(torch.int64))
        if sum(c.rows) + c.L <= 256:
            assert with_draw.reg == plain.reg != T.reg_out0
        fc.check_case(name + " with next_draw", c, with_draw, ref)


# ---------------------------------------------------------------------------------------- (c) shine_adam_step / shine_adam_step_dev
MISALIGNED = {"mixed-sizes": (2, 6)}  # tensors whose four pointers are offset by one float: the scalar path of k_adam


def run_adam(c, T, dev, zero_grad):
    """one launch -> (results as fc.check_case judges them, the bias corrections the launch used)"""
    from types import SimpleNamespace

    from shine_mapping_amd import _lib

    lib = _lib.lib()
    off = MISALIGNED.get(c.name, ())
    B = {k: [Buf(x, 1 if s in off else 0) for s, x in enumerate(getattr(T, k))] for k in "pgmv"}
    flags = [None if f is None else Buf(f) for f in T.flags]
    lr = list(fc.LR_DEV[:c.n_tensors])
    ptrs = lambda xs: _lib.ptr_array([None if x is None else x.ptr() for x in xs])
    args = (c.n_tensors, ptrs(B["p"]), ptrs(B["g"]), ptrs(B["m"]), ptrs(B["v"]), _lib.i64_array(c.numel))
    tail = ((C.c_float * c.n_tensors)(*c.wd), fc.B1, fc.B2, c.eps)
    rf = ptrs(flags) if c.flagged else None
    bc = fc.bias_corrections(c.t)
    if dev:
        state = _step_state(c.t - 1)  # zero products: the launch derives them with pow
        lr_dev = torch.tensor(lr, dtype=torch.float32).cuda()
        _lib.check(lib.shine_adam_step_dev(*args, lr_dev.data_ptr(), *tail, state.data_ptr(), zero_grad, rf, _stream()),
                   "shine_adam_step_dev")
        torch.cuda.synchronize()
        assert int(state[0]) == c.t
        used = state[1:2].view(torch.float32).cpu().tolist()
        _one_ulp(used, c.t)
        bc = tuple(used)
    else:
        _lib.check(lib.shine_adam_step(*args, (C.c_float * c.n_tensors)(*lr), *tail, c.t, zero_grad, rf, _stream()),
                   "shine_adam_step")
        torch.cuda.synchronize()
    got = SimpleNamespace(p=[b.result() for b in B["p"]], m=[b.result() for b in B["m"]], v=[b.result() for b in B["v"]],
                          g=[b.result() for b in B["g"]], flags=[None if f is None else f.result() for f in flags])
    return got, bc, lr


def _one_ulp(bc, t):
    """the two bias-correction floats are within one fp32 ulp of the fp64 values of step t"""
    for got, want in zip(bc, (1.0 - fc.B1 ** t, math.sqrt(1.0 - fc.B2 ** t))):
        ulp = 2.0 ** (math.frexp(want)[1] - 24)
        assert abs(got - want) <= ulp, (t, got, want)


@pytest.mark.parametrize("zero_grad", [1, 0])
@pytest.mark.parametrize("dev", [False, True], ids=["host-step", "device-step"])
@pytest.mark.parametrize("name", list(fc.ADAM_CASES))
def test_fused_adam_matches_fp64_on_every_element(name, dev, zero_grad):
    c = fc.ADAM_CASES[name]
    T = fc.adam_build(c, "cuda")
    got, bc, lr = run_adam(c, T, dev, zero_grad)
    ref = fc.adam_oracle(c, T, lr, zero_grad=zero_grad, bc=bc)
    rho = fc.check_case(name, c, got, ref, adam_only=True)
    fc.record("adam/%s/%s/zero_grad=%d" % (name, "dev" if dev else "host", zero_grad), "hip", rho)


def test_the_device_step_state_counts_and_keeps_its_bias_corrections():
    """seeded with [0] = t - 1 and zero products the first launch derives the powers with pow; ten more launches take the running
    products: after each, the two floats are within one fp32 ulp of the fp64 value and [0] counts the steps"""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    for t in fc.TS:
        c = fc.adam_case("state", (5, 8), t=t, seed=46)
        T = fc.adam_build(c, "cuda")
        B = {k: [Buf(x) for x in getattr(T, k)] for k in "pgmv"}
        ptrs = lambda xs: _lib.ptr_array([x.ptr() for x in xs])
        state = _step_state(t - 1)
        lr_dev = torch.tensor(fc.LR_DEV[:2], dtype=torch.float32).cuda()
        for k in range(11):
            _lib.check(lib.shine_adam_step_dev(2, ptrs(B["p"]), ptrs(B["g"]), ptrs(B["m"]), ptrs(B["v"]), _lib.i64_array(c.numel),
                                               lr_dev.data_ptr(), (C.c_float * 2)(), fc.B1, fc.B2, c.eps, state.data_ptr(), 0, None,
                                               _stream()), "shine_adam_step_dev")
            torch.cuda.synchronize()
            assert int(state[0]) == t + k
            _one_ulp(state[1:2].view(torch.float32).cpu().tolist(), t + k)
            pr = state[2:4].view(torch.float64).cpu().tolist()
            assert abs(pr[0] - fc.B1 ** (t + k)) <= 1e-13 * fc.B1 ** (t + k) and abs(pr[1] - fc.B2 ** (t + k)) <= 1e-13 * fc.B2 ** (t + k)
        # zero_grad bit 1: the state was advanced by another launch — this one leaves it alone
        _lib.check(lib.shine_adam_step_dev(2, ptrs(B["p"]), ptrs(B["g"]), ptrs(B["m"]), ptrs(B["v"]), _lib.i64_array(c.numel),
                                           lr_dev.data_ptr(), (C.c_float * 2)(), fc.B1, fc.B2, c.eps, state.data_ptr(), 1 | 2, None,
                                           _stream()), "shine_adam_step_dev")
        torch.cuda.synchronize()
        assert int(state[0]) == t + 10
        for b in B["p"] + B["m"] + B["v"] + B["g"]:
            b.result()


# ----------------------------------------------------------------------------------------------------- (d) the operand image
def _iteration(fx, frozen, n, unroll, dec=None, octree=None):
    from shine_mapping_amd import StepOptions
    from shine_mapping_amd.loop import GraphedIteration
    from shine_mapping_amd.optim import setup_optimizer
    from shine_mapping_amd.sampler import SortedPool

    cfg, octree2, dec2 = product_from_golden(fx)
    octree = octree if octree is not None else octree2
    dec = dec if dec is not None else dec2.cuda()
    cfg.lr, cfg.opt_adam, cfg.adam_eps, cfg.lr_level_reduce_ratio, cfg.weight_decay = 0.01, True, 1e-15, 0.5, 1e-7
    for p in dec.parameters():
        p.requires_grad_(not frozen)
    opt = setup_optimizer(cfg, list(octree.parameters()), None if frozen else dec.fused_params())
    octree._require_tables(with_ranks=True)
    pool = SortedPool(octree, fx["coord"].cuda(), fx["sdf_label"].cuda(), fx["weight"].cuda(), seed=5, canonical=True)
    opts = StepOptions(sigma=fx["sigma"], loss_reduction="mean", deterministic=True, decoder_grad_on=False if frozen else None)
    it = GraphedIteration(octree, dec, pool, opt, opts, n, unroll=unroll)
    assert it.native
    return it, octree, dec


def _image_after(it, unroll, iters):
    """the graph's operand image after `iters` iterations; what the launches do not write keeps a pattern"""
    from shine_mapping_amd.loop import IterationGraph

    g = IterationGraph.shared(it.pool.coord.device, unroll, it.graph_slot)
    g.ensure_image(it.pool.coord.device)
    g.image.fill_(PATTERN)
    it.run(iters)
    torch.cuda.synchronize()
    assert it._bound(unroll)[0] is g
    return g.image.clone()


def test_the_operand_image_the_tail_keeps_is_the_one_the_head_rebuilds():
    """operand_image_slots (csrc/shine_tile16.hpp) is the inverse of k_operand_image: after two iterations with a trainable decoder
    — the head built the image, the tail kept it current twice — it equals, float for float, what a frozen-decoder iteration
    (no decoder units in its tail: the image is only rebuilt) holds for the same decoder tensors"""
    from shine_mapping_amd import _lib

    fx = load_golden("maicity_bce_L3")
    floats = int(_lib.lib().shine_iter_graph_operand_image_floats())
    it0, _, _ = _iteration(fx, True, 512, 1)
    initial = _image_after(it0, 1, 1)
    it, octree, dec = _iteration(fx, False, 512, 2)
    before = [p.detach().clone() for p in dec.fused_params()]
    kept = _image_after(it, 2, 2)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, dec.fused_params()))
    it2, _, _ = _iteration(fx, True, 512, 1, dec=dec, octree=octree)
    rebuilt = _image_after(it2, 1, 1)
    assert kept.numel() == rebuilt.numel() == floats
    assert torch.equal(kept.view(torch.int32), rebuilt.view(torch.int32))
    assert not torch.equal(kept.view(torch.int32), initial.view(torch.int32))
    assert int((kept != PATTERN).sum()) >= fc.MLP_PARAMS  # the launches did write it


# ------------------------------------------------------------------------------- (e) the layout the step writes with defer_reduce
def test_the_layout_the_cases_restate_is_the_layout_the_step_writes():
    """kitti_eik_L3 at N = 4096 + 24 (65 workgroups): the sums over the partial vectors a deferred step leaves — decoder entries,
    trash rows, the four doubles, read with fc's constants — against the grads and loss_parts of the non-deferred call from the same
    start (k_reduce_partials), by the tail_sum rule: |x - sum64| <= K 2^-24 sum_b |partial_b| (K of tail_sum_m: exp_avg of a fresh
    element is (1 - b1) g, so g's ratio is its ratio)"""
    from shine_mapping_amd import StepOptions, _lib, fused_train_step
    from shine_mapping_amd.sampler import SortedPool

    fx = load_golden("kitti_eik_L3")
    N = 4096 + 24

    def start():
        cfg, octree, dec = product_from_golden(fx)
        dec = dec.cuda()
        octree._require_tables(with_ranks=True)
        pool = SortedPool(octree, fx["coord"].cuda().repeat(8, 1), fx["sdf_label"].cuda().repeat(8), fx["weight"].cuda().repeat(8),
                          seed=5, canonical=True)
        for p in list(octree.hier_features) + dec.fused_params():
            p.grad = torch.zeros_like(p)
        surf = pool.surf_parts_buffer(N)
        idx = pool.draw(N, surf_parts=surf)
        return octree, dec, pool, idx, surf, StepOptions(sigma=fx["sigma"], ekional_loss_on=True, weight_e=0.1)

    octree, dec, pool, idx, surf, opts = start()
    loss, _, _ = fused_train_step(octree, dec, None, None, None, opts, n_surf=surf, pool=pool, idx=idx)
    torch.cuda.synchronize()
    want_dec = [p.grad.detach().reshape(-1).clone() for p in dec.fused_params()]
    want_trash = [p.grad.detach()[-1].clone() for p in octree.hier_features]
    octree2, dec2, pool2, idx2, surf2, opts2 = start()
    assert torch.equal(idx, idx2)
    pending = {}
    fused_train_step(octree2, dec2, None, None, None, opts2, n_surf=surf2, pool=pool2, idx=idx2, pending=pending)
    torch.cuda.synchronize()
    L = len(octree.hier_features)
    nb = int(_lib.lib().shine_train_step_workspace_bytes(C.byref(pending["cfg"]), N)) // (fc.PART_STRIDE * 4)
    assert nb == 65 and pending["cfg"].defer_reduce == 1
    part = pending["workspace"].view(torch.float32)[:nb * fc.PART_STRIDE].view(nb, fc.PART_STRIDE)
    p64 = part.double()
    worst = 0.0
    for i, (off, n) in enumerate(zip(fc.DEC_OFF, fc.DEC_N)):
        assert want_dec[i].numel() == n
        worst = max(worst, fc.check("decoder grad %d" % i, "tail_sum_m", want_dec[i], p64[:, off:off + n].sum(0),
                                    p64[:, off:off + n].abs().sum(0)))
    for s in range(L):
        cols = slice(fc.PART_TRASH + s * fc.F, fc.PART_TRASH + (s + 1) * fc.F)
        worst = max(worst, fc.check("trash row %d" % s, "tail_sum_m", want_trash[s], p64[:, cols].sum(0), p64[:, cols].abs().sum(0)))
    assert float(sum(w.abs().sum() for w in want_dec)) > 0.0 and float(sum(w.abs().sum() for w in want_trash)) > 0.0
    d = part.view(torch.float64).view(nb, fc.PART_STRIDE // 2)[:, fc.PART_LOSS // 2:fc.PART_LOSS // 2 + 4]
    ns = int(surf.sum())
    assert ns > 0 and float(d[0, 3]) == float(ns)
    bce, eik = d[:, 0].sum() / N, d[:, 2].sum() / ns
    sb, se = d[:, 0].abs().sum() / N, d[:, 2].abs().sum() / ns
    fc.check("loss", "loss", loss.detach().reshape(1).cpu(), (bce + fc.f32(0.1) * eik).reshape(1).cpu(),
             (sb + fc.f32(0.1) * se).reshape(1).cpu())
    fc.record("layout/kitti_eik_L3", "hip", {"tail_sum_m": worst})
