"""CPU suite of the gradient-consistency training term (csrc/shine_consistency_step.hip, ops.fused_consistency_step,
losses.consistency_loss, loop.GraphedIteration(consistency=...)): losses.consistency_loss against the fp64 autograd oracle on
pairs that include exactly-zero gradients, the reference's line on the same pairs (equal value, a 1e8-scaled gradient on the zero
side), sigma's cancellation, the fp32 oracle's own distance from the fp64 one, the entry point's header / binding / host-side
argument errors and the Python argument errors that need no launch.  The kernel itself is checked in
tests/test_gpu_consistency_step.py."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import consistency_step_oracle as co
from conftest import ROOT, oracle_from_golden


# ---- 1. losses.consistency_loss is the oracle's definition, guard included
def test_consistency_loss_is_the_definition_with_the_guard():
    from shine_mapping_amd import losses

    c = co.case("kitti_eik_L3")
    w = c.wide
    ga, gb = w["ga"], w["gb"]
    zero = (ga.norm(dim=-1) == 0) | (gb.norm(dim=-1) == 0)
    one_sided = (ga.norm(dim=-1) == 0) != (gb.norm(dim=-1) == 0)
    assert int(zero.sum()) > 100 and int(one_sided.sum()) > 0 and int((~zero).sum()) > 1000
    a, b = ga.clone().requires_grad_(True), gb.clone().requires_grad_(True)
    loss = losses.consistency_loss(a, b)
    assert loss.dim() == 0 and abs(float(loss.detach()) - float(w["loss"])) <= 1e-12
    (co.WEIGHT_C * loss).backward()
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all())
    # the closed form of the issue: dL/dga = -(gbh - c gah) / |ga| * weight_c / K, symmetrically for gb; nothing behind the guard
    k = ga.shape[0]
    live = ~zero
    na, nb = ga[live].norm(dim=-1, keepdim=True), gb[live].norm(dim=-1, keepdim=True)
    ah, bh = ga[live] / na, gb[live] / nb
    cc = (ah * bh).sum(-1, keepdim=True)
    assert float((a.grad[live] - (-(bh - cc * ah) / na * co.WEIGHT_C / k)).abs().max()) <= 1e-12 * float(a.grad.abs().max())
    assert float((b.grad[live] - (-(ah - cc * bh) / nb * co.WEIGHT_C / k)).abs().max()) <= 1e-12 * float(b.grad.abs().max())
    assert float(a.grad[zero].abs().max()) == 0.0 and float(b.grad[zero].abs().max()) == 0.0
    # a guarded pair contributes exactly 1
    assert abs(float(loss.detach()) - (float((1 - cc).sum()) + int(zero.sum())) / k) <= 1e-12
    # K = 0
    e = losses.consistency_loss(ga[:0], gb[:0])
    assert e.dim() == 0 and float(e) == 0.0
    # fp32 inputs stay fp32
    assert losses.consistency_loss(ga.float(), gb.float()).dtype == torch.float32


# ---- 2. the reference's line: the same value, and a gradient of gbh / eps on the zero side
def test_reference_line_has_the_same_value_and_a_1e8_scaled_gradient_on_the_zero_side():
    from shine_mapping_amd import losses

    c = co.case("kitti_eik_L3")
    ga, gb = c.wide["ga"].float(), c.wide["gb"].float()
    a, b = ga.clone().requires_grad_(True), gb.clone().requires_grad_(True)
    ref = (1.0 - F.cosine_similarity(a, b)).mean()  # shine_batch.py:189
    ours = losses.consistency_loss(ga, gb)
    assert abs(float(ref.detach()) - float(ours)) <= 1e-6
    ref.backward()
    k = ga.shape[0]
    za = (ga.norm(dim=-1) == 0) & (gb.norm(dim=-1) > 0)
    assert int(za.sum()) > 0
    push = a.grad[za].norm(dim=-1) * k  # per-pair gradient of (1 - cos): |gbh| / eps = 1e8
    print("reference gradient on a zero side: %.3g .. %.3g" % (float(push.min()), float(push.max())))
    assert float(push.min()) > 1e6
    a2 = ga.clone().requires_grad_(True)
    losses.consistency_loss(a2, gb).backward()
    assert float(a2.grad[za].abs().max()) == 0.0
    # away from the guard the two gradients agree
    live = (ga.norm(dim=-1) > 0) & (gb.norm(dim=-1) > 0)
    assert float((a2.grad[live] - a.grad[live]).abs().max()) <= 1e-5 * float(a2.grad[live].abs().max())


# ---- 3. sigma cancels
def test_sigma_cancels():
    from shine_mapping_amd import losses
    import normal_step_oracle as no

    c = co.case("maicity_bce_L4")
    oct_, mlp = no.wide_oracle(c.fx)
    scaled = co.consistency_term(oct_, mlp, c.pairs.coord_a, c.pairs.coord_b, co.WEIGHT_C, sigma=0.07)
    loss_err, errs = co.rel_errors(scaled["loss"], scaled["feat_grads"], scaled["mlp_grads"], c.wide)
    assert loss_err <= 1e-12 and max(errs) <= 1e-10, (loss_err, errs)
    ga, gb = c.wide["ga"], c.wide["gb"]
    assert abs(float(losses.consistency_loss(0.07 * ga, 0.07 * gb)) - float(losses.consistency_loss(ga, gb))) <= 1e-12
    assert "sigma" not in inspect.signature(__import__("shine_mapping_amd").fused_consistency_step).parameters


# ---- 4. the fixtures hold the guard's cases, nothing is left out, and the fp32 oracle alone is well inside the GPU tests' line
@pytest.mark.parametrize("name", co.FIXTURES)
def test_fp32_oracle_is_within_tolerance_of_the_fp64_one(name):
    c = co.case(name)
    assert c.pairs.left_out <= co.MAX_LEFT_OUT and c.pairs.zero_g > 100
    assert int(c.pairs.near_index[0]) == int(c.pairs.near_index[1])  # (a repeated base row)
    _, oct_, mlp = oracle_from_golden(c.fx)
    ref = co.consistency_term(oct_, mlp, c.pairs.coord_a, c.pairs.coord_b, co.WEIGHT_C)
    loss_err, errs = co.rel_errors(ref["loss"], ref["feat_grads"], ref["mlp_grads"], c.wide)
    print(name, "pairs", c.pairs.near_index.numel(), "zero-g", c.pairs.zero_g, "loss %.1e" % loss_err, " ".join("%.1e" % e for e in errs))
    assert loss_err <= 1e-4 and max(errs) <= 1e-4, (name, loss_err, errs)
    w = c.wide
    assert float(w["mlp_grads"][1].abs().max()) == 0.0 and float(w["mlp_grads"][3].abs().max()) == 0.0  # b1, b2: exactly 0
    assert w["has_grad"][5] is False  # b3 has no path


# ---- 5. header, binding, host-side argument errors
def _call(lib, table, cfg, stride=3, n=16, k=8, coord=True, near=True, shift=True, state=True, mlp=True, loss=True, ws=256):
    """shine_consistency_train_step with stand-in (never dereferenced) pointers wherever the argument checks only look for NULL"""
    from shine_mapping_amd import _lib

    fake = 4096
    ptrs = _lib.ptr_array([fake] * 6)
    feats = _lib.ptr_array([fake] * 3)
    rows = _lib.i64_array([10, 10, 10])
    return lib.shine_consistency_train_step(table, cfg, fake if coord else None, stride, None, n, fake if near else None,
                                            fake if shift else None, k, 0.01, 7, fake if state else None, None, None, 0.5, feats,
                                            rows, None, ptrs if mlp else None, None, None, fake if loss else None, ws, None)


def test_argument_errors_come_back_without_touching_the_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    table = C.c_void_p()
    assert lib.shine_tables_create(3, C.byref(table)) == 0
    cfg = _lib.StepConfig()
    cfg.n_levels, cfg.max_level = 3, 12
    try:
        for kw, word in ((dict(stride=4), b"coord_stride"), (dict(stride=0), b"coord_stride"), (dict(n=-1), b"n < 0"),
                         (dict(k=-1), b"n_pairs < 0"), (dict(near=False), b"near_index and shift come together"),
                         (dict(shift=False), b"near_index and shift come together"),
                         (dict(near=False, shift=False, state=False), b"drawn pairs need draw_state"),
                         (dict(n=0), b"n_pairs > 0 with n == 0"), (dict(coord=False), b"null argument"),
                         (dict(mlp=False), b"null argument"), (dict(loss=False), b"null argument"), (dict(ws=0), b"workspace"),
                         (dict(ws=8), b"workspace")):
            rc = _call(lib, table, C.byref(cfg), **kw)
            assert rc == -1 and word in lib.shine_error_string(rc), (kw, lib.shine_error_string(rc))
            assert b"shine_consistency_train_step" in lib.shine_error_string(rc)
        rc = _call(lib, None, C.byref(cfg))
        assert rc == -1 and b"null table handle" in lib.shine_error_string(rc)
        rc = _call(lib, table, None)
        assert rc == -1 and b"null config" in lib.shine_error_string(rc)
        # every argument in order (explicit and drawn), but the handle's levels were never inserted: a state error, still on the host
        for kw in (dict(), dict(near=False, shift=False)):
            rc = _call(lib, table, C.byref(cfg), **kw)
            assert rc == -4 and b"no table yet" in lib.shine_error_string(rc), lib.shine_error_string(rc)
        cfg.n_levels = 5
        rc = _call(lib, table, C.byref(cfg))
        assert rc == -1 and b"more than 4 featured levels" in lib.shine_error_string(rc)
    finally:
        assert lib.shine_tables_destroy(table) == 0


def test_header_declares_the_entry_point_with_its_contract():
    from shine_mapping_amd import _lib, autograd_ops, build

    text = open(os.path.join(ROOT, "include", "shine_hip.h")).read()
    assert re.search(r"\bint shine_consistency_train_step\(", text)
    m = re.search(r"#define SHINE_CONSISTENCY_WORKSPACE_BYTES (\d+)", text)
    assert m and int(m.group(1)) == autograd_ops.CONSISTENCY_WORKSPACE_BYTES and int(m.group(1)) % 8 == 0
    assert callable(autograd_ops.consistency_workspace)
    doc = text[:text.index("int shine_consistency_train_step(")]
    doc = doc[doc.rindex("/* ----"):]
    for word in ("coord_stride", "near_index", "shift_scale", "draw_state", "THE GUARD", "eps = 1e-8", "EXPLICIT", "DRAWN", "touched",
                 "grad_mlp: NULL", "ACCUMULATED", "ADDED", "bit-identical", "fp64", "n_pairs == 0",
                 "SHINE_CONSISTENCY_WORKSPACE_BYTES", "SHINE_E_INVALID", "UNWEIGHTED"):
        assert word in doc, word
    res, args = _lib._SIGNATURES["shine_consistency_train_step"]
    assert res is C.c_int and len(args) == 24 and args[3] is C.c_int32 and args[5] is C.c_int64 and args[8] is C.c_int64
    assert args[9] is C.c_float and args[10] is C.c_uint64 and args[14] is C.c_float
    decl = text[text.index("int shine_consistency_train_step("):]
    decl = decl[:decl.index(");")]
    assert decl.count(",") + 1 == len(args)  # (the binding covers the header's parameter list)
    assert hasattr(C.CDLL(build.build(verbose=False)), "shine_consistency_train_step")
    assert "shine_consistency_step.hip" in build.sources() and "shine_normal_step.hip" in build.sources()
    # one chain in the source: both kernels instantiate the shared body
    for f in ("shine_consistency_step.hip", "shine_normal_step.hip"):
        src = open(os.path.join(ROOT, "shine_mapping_amd", "csrc", f)).read()
        assert '#include "shine_gterm_body.hpp"' in src and "gterm_step<L, POLY," in src, f


# ---- 6. the public surface and the argument errors that need no launch
def test_public_surface_and_the_loop_s_argument_errors():
    import shine_mapping_amd as s
    from shine_mapping_amd import loop, losses, ops

    assert s.fused_consistency_step is ops.fused_consistency_step and s.consistency_loss is losses.consistency_loss
    assert s.ConsistencyTerm is loop.ConsistencyTerm
    assert all(name in s.__all__ for name in ("fused_consistency_step", "consistency_loss", "ConsistencyTerm"))
    sig = inspect.signature(ops.fused_consistency_step)
    assert list(sig.parameters) == ["octree", "decoder", "coord", "weight_c", "near_index", "shift", "n_pairs", "shift_scale", "seed",
                                    "draw_state", "pool", "idx", "touched", "grad_buffers", "out", "workspace", "draws_out"]
    assert sig.parameters["seed"].default == 0
    assert all(sig.parameters[k].default is None for k in list(sig.parameters)[4:] if k != "seed")
    assert list(inspect.signature(losses.consistency_loss).parameters) == ["g_base", "g_near"]
    term = loop.ConsistencyTerm()
    assert (term.weight_c, term.count, term.seed) == (1.0, 1000, 0) and term.shift_scale > 0
    assert loop.ConsistencyTerm(0.5, 10, 0.01, 3) == loop.ConsistencyTerm(weight_c=0.5, count=10, shift_scale=0.01, seed=3)
    assert not hasattr(loop, "_IterationTerms")
    p = inspect.signature(loop.GraphedIteration).parameters["consistency"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None

    class Opt:  # has the folded iteration's hooks; nothing is called before the argument checks
        param_groups = []

        def finish_iteration(self):
            pass

        def prepare_graph_safe(self, skip=()):
            raise AssertionError("argument errors come first")

    class Pool:
        coord = torch.zeros(4, 3)

        def surf_parts_buffer(self, n=None):
            return torch.zeros(64, dtype=torch.int64)

    octree = type("O", (), {"hier_features": [], "_tables_epoch": 0})()
    opts = s.StepOptions(sigma=0.1)
    with pytest.raises(ValueError, match=r"consistency=\.\.\.\) needs the folded iteration"):
        loop.GraphedIteration(octree, None, Pool(), Opt(), opts, 16, fold=False, consistency=loop.ConsistencyTerm())
    with pytest.raises(ValueError, match=r"consistency=\.\.\.\) needs the folded iteration"):
        loop.GraphedIteration(octree, None, Pool(), object(), opts, 16, consistency=loop.ConsistencyTerm())
    with pytest.raises(ValueError, match="lambda_forget"):
        loop.GraphedIteration(octree, None, Pool(), Opt(), opts, 16, 0.1, consistency=loop.ConsistencyTerm())
    with pytest.raises(ValueError, match="count >= 0 and shift_scale >= 0"):
        loop.GraphedIteration(octree, None, Pool(), Opt(), opts, 16, consistency=loop.ConsistencyTerm(shift_scale=-1.0))
    with pytest.raises(TypeError):
        loop.GraphedIteration(octree, None, Pool(), Opt(), opts, 16, consistencies=loop.ConsistencyTerm())


def test_fused_consistency_step_refuses_bad_arguments_before_any_launch():
    from shine_mapping_amd import ops

    class Octree:
        _tables_epoch = 3

        def _require_tables(self, probe=False):
            return None

        def _check_coord(self, coord):
            return coord

    class Dec:
        def fused_params(self):
            return []

    pool = type("P", (), {"tables_epoch": 3, "rec": None})()
    near, shift = torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="array mode needs coord"):
        ops.fused_consistency_step(Octree(), Dec(), None, 0.1, n_pairs=8, shift_scale=0.01)
    with pytest.raises(ValueError, match="pool mode needs idx"):
        ops.fused_consistency_step(Octree(), Dec(), None, 0.1, n_pairs=8, shift_scale=0.01, pool=pool)
    with pytest.raises(ValueError, match="pool mode needs idx"):
        ops.fused_consistency_step(Octree(), Dec(), None, 0.1, pool=pool, idx=torch.zeros(4, dtype=torch.int32))
    coord = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="near_index and shift come together"):
        ops.fused_consistency_step(Octree(), Dec(), coord, 0.1, near_index=near)
    with pytest.raises(ValueError, match="near_index and shift come together"):
        ops.fused_consistency_step(Octree(), Dec(), coord, 0.1, shift=shift)
    with pytest.raises(ValueError, match="near_index must be a contiguous CUDA int32"):  # (host tensors)
        ops.fused_consistency_step(Octree(), Dec(), coord, 0.1, near_index=near, shift=shift)
    with pytest.raises(ValueError, match="drawn pairs need n_pairs"):
        ops.fused_consistency_step(Octree(), Dec(), coord, 0.1)
    with pytest.raises(ValueError, match="drawn pairs need n_pairs"):
        ops.fused_consistency_step(Octree(), Dec(), coord, 0.1, n_pairs=-1)
    with pytest.raises(ValueError, match="drawn pairs need shift_scale"):
        ops.fused_consistency_step(Octree(), Dec(), coord, 0.1, n_pairs=8)
    with pytest.raises(ValueError, match="drawn pairs need draw_state"):
        ops.fused_consistency_step(Octree(), Dec(), coord, 0.1, n_pairs=8, shift_scale=0.01)
    with pytest.raises(ValueError, match="drawn pairs need draw_state"):  # (a Python int: the natural mistake)
        ops.fused_consistency_step(Octree(), Dec(), coord, 0.1, n_pairs=8, shift_scale=0.01, draw_state=0)
