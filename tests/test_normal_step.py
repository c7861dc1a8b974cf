"""CPU suite of the surface-normal training term (csrc/shine_normal_step.hip, ops.fused_normal_step, losses.normal_loss,
loop.GraphedIteration(normal=...)): the closed form of the issue against the fp64 autograd oracle, losses.normal_loss against
the reference's expression, the fp32 oracle's own distance from the fp64 one, the entry point's header / binding / host-side
argument errors, SortedPool's normals, and the Python argument errors that need no launch.  The kernel itself is checked in
tests/test_gpu_normal_step.py."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import normal_step_oracle as no
from conftest import ROOT, oracle_from_golden


# ---- 1. the closed form is the oracle
@pytest.mark.parametrize("name", no.FIXTURES)
def test_closed_form_equals_the_fp64_autograd_oracle(name):
    c = no.case(name)
    oct_, mlp = no.wide_oracle(c.fx)
    cf = no.closed_form(oct_, mlp, c.coord, c.weight, c.normal, no.WEIGHT_N)
    wide = c.wide
    assert abs(float(cf["loss"]) - float(wide["loss"])) <= 1e-10 * max(1.0, abs(float(wide["loss"])))
    assert torch.equal(cf["live"], wide["live"])
    for k, (a, b) in enumerate(zip(cf["feat_grads"] + cf["mlp_grads"], wide["feat_grads"] + wide["mlp_grads"])):
        err = float((a - b.reshape(a.shape)).abs().max())
        assert err <= 1e-10 * float(b.abs().max()) or float(b.abs().max()) == 0.0 == err, (name, k, err, float(b.abs().max()))
    L = len(wide["feat_grads"])
    assert float(wide["mlp_grads"][1].abs().max()) == 0.0 and float(wide["mlp_grads"][3].abs().max()) == 0.0  # b1, b2: exactly 0
    assert wide["has_grad"][5] is False  # b3 has no path
    assert all(float(t.abs().max()) > 0 for t in wide["feat_grads"][:L]) or c.zero_g > 0
    assert all(bool(torch.isfinite(t).all()) for t in wide["feat_grads"] + wide["mlp_grads"])  # (the NaN label was never read)


def test_fixtures_hold_the_rows_the_guard_is_for():
    counts = {name: (no.case(name).zero_g, int((no.case(name).weight > 0).sum())) for name in no.FIXTURES}
    print(counts)
    assert all(z > 0 for z, _ in counts.values()), counts  # every fixture has surface rows with g == 0 exactly
    assert counts["edges_L2_nopoly_eik"][0] > 100


# ---- 2. losses.normal_loss
def test_normal_loss_is_the_reference_expression_with_keepdim_and_the_guard():
    from shine_mapping_amd import losses

    c = no.case("kitti_eik_L3")
    g32 = c.wide["g"].float()
    n = g32.shape[0]
    surf = c.weight > 0
    # the reference's lines as written do not broadcast
    with pytest.raises(RuntimeError):
        _ = g32[surf] / g32[surf].norm(2, dim=-1)
    # with keepdim, on the rows where |g| > 0, it is the reference's expression
    live = surf & (g32.norm(2, dim=-1) > 0)
    gs = g32[live]
    ref = ((gs / gs.norm(2, dim=-1, keepdim=True) - c.normal[live]).abs()).norm(2, dim=-1).mean()
    w_live = torch.where(live, torch.ones(n), -torch.ones(n))
    got = losses.normal_loss(g32, c.normal, w_live)
    assert abs(float(got) - float(ref)) <= 1e-6 * float(ref)
    # with the zero-g rows in: the reference is NaN, the guarded form finite — those rows add |n| and stay in the denominator
    gz = g32[surf]
    raw = ((gz / gz.norm(2, dim=-1, keepdim=True) - c.normal[surf]).abs()).norm(2, dim=-1).mean()
    assert c.zero_g > 0 and bool(torch.isnan(raw))
    full = losses.normal_loss(g32, c.normal, c.weight)
    dead = surf & ~live
    want = (float(ref) * int(live.sum()) + float(c.normal[dead].norm(2, dim=-1).sum())) / int(surf.sum())
    assert bool(torch.isfinite(full)) and abs(float(full) - want) <= 1e-5 * want
    # no surface row: 0
    assert float(losses.normal_loss(g32, c.normal, -torch.ones(n))) == 0.0
    # its autograd gradient is the helper's q (fp64, at the oracle's g)
    oct_, mlp = no.wide_oracle(c.fx)
    cf = no.closed_form(oct_, mlp, c.coord, c.weight, c.normal, no.WEIGHT_N)
    g = cf["g"].clone().requires_grad_(True)
    (no.WEIGHT_N * losses.normal_loss(g, c.normal.double(), c.weight)).backward()
    assert bool(torch.isfinite(g.grad).all())
    assert float((g.grad - cf["q"]).abs().max()) <= 1e-12 * float(cf["q"].abs().max())
    assert float(g.grad[~surf].abs().max()) == 0.0 and float(g.grad[dead].abs().max()) == 0.0


# ---- 3. the fp32 oracle alone stays well inside the GPU tests' tolerance (measured with these labels: <= 1.6e-5 on every tensor
#         of every fixture — the worst on maicity_bce_L3's feature levels —, the loss to 8.3e-8)
@pytest.mark.parametrize("name", no.FIXTURES)
def test_fp32_oracle_is_within_tolerance_of_the_fp64_one(name):
    c = no.case(name)
    _, oct_, mlp = oracle_from_golden(c.fx)
    ref = no.normal_term(oct_, mlp, c.coord, c.weight, c.normal, no.WEIGHT_N)
    loss_err, errs = no.rel_errors(ref["loss"], ref["feat_grads"], ref["mlp_grads"], c.wide)
    print(name, "loss %.1e" % loss_err, " ".join("%.1e" % e for e in errs))
    assert loss_err <= 1e-4 and max(errs) <= 1e-4, (name, loss_err, errs)


# ---- 4. header, binding, host-side argument errors
def _call(lib, table, cfg, stride=3, wstride=1, n=16, coord=True, weight=True, normal=True, nsurf=True, mlp=True, loss=True,
          ws=256):
    """shine_normal_train_step with stand-in (never dereferenced) pointers wherever the argument checks only look for NULL"""
    from shine_mapping_amd import _lib

    fake = 4096
    ptrs = _lib.ptr_array([fake] * 6)
    feats = _lib.ptr_array([fake] * 3)
    rows = _lib.i64_array([10, 10, 10])
    return lib.shine_normal_train_step(table, cfg, fake if coord else None, stride, None, fake if weight else None, wstride,
                                       fake if normal else None, fake if nsurf else None, 1, n, 0.5, feats, rows, None,
                                       ptrs if mlp else None, None, fake if loss else None, ws, None)


def test_argument_errors_come_back_without_touching_the_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    table = C.c_void_p()
    assert lib.shine_tables_create(3, C.byref(table)) == 0
    cfg = _lib.StepConfig()
    cfg.n_levels, cfg.max_level = 3, 12
    try:
        for kw, word in ((dict(stride=4), b"coord_stride"), (dict(stride=0), b"coord_stride"), (dict(wstride=3), b"weight_stride"),
                         (dict(wstride=0), b"weight_stride"), (dict(n=-1), b"n < 0"), (dict(coord=False), b"null argument"),
                         (dict(weight=False), b"null argument"), (dict(normal=False), b"null argument"),
                         (dict(nsurf=False), b"null argument"), (dict(mlp=False), b"null argument"),
                         (dict(loss=False), b"null argument"), (dict(ws=0), b"workspace"), (dict(ws=8), b"workspace")):
            rc = _call(lib, table, C.byref(cfg), **kw)
            assert rc == -1 and word in lib.shine_error_string(rc), (kw, lib.shine_error_string(rc))
            assert b"shine_normal_train_step" in lib.shine_error_string(rc)
        rc = _call(lib, None, C.byref(cfg))
        assert rc == -1 and b"null table handle" in lib.shine_error_string(rc)
        rc = _call(lib, table, None)
        assert rc == -1 and b"null config" in lib.shine_error_string(rc)
        # every argument in order, but the handle's levels were never inserted: a state error, still on the host
        rc = _call(lib, table, C.byref(cfg))
        assert rc == -4 and b"no table yet" in lib.shine_error_string(rc), lib.shine_error_string(rc)
        cfg.n_levels = 5
        rc = _call(lib, table, C.byref(cfg))
        assert rc == -1 and b"more than 4 featured levels" in lib.shine_error_string(rc)
    finally:
        assert lib.shine_tables_destroy(table) == 0


def test_header_declares_the_entry_point_with_its_contract():
    from shine_mapping_amd import _lib, autograd_ops, build

    text = open(os.path.join(ROOT, "include", "shine_hip.h")).read()
    assert re.search(r"\bint shine_normal_train_step\(", text)
    m = re.search(r"#define SHINE_NORMAL_WORKSPACE_BYTES (\d+)", text)
    assert m and int(m.group(1)) == autograd_ops.NORMAL_WORKSPACE_BYTES and int(m.group(1)) % 8 == 0
    doc = text[:text.index("int shine_normal_train_step(")]
    doc = doc[doc.rindex("/* ----"):]
    for word in ("coord_stride", "weight_stride", "n_surf_parts", "THE GUARD", "keepdim", "grad_mlp: NULL", "ACCUMULATED", "ADDED",
                 "bit-identical", "fp64", "n == 0", "SHINE_NORMAL_WORKSPACE_BYTES", "SHINE_E_INVALID", "UNWEIGHTED"):
        assert word in doc, word
    res, args = _lib._SIGNATURES["shine_normal_train_step"]
    assert res is C.c_int and len(args) == 20 and args[3] is C.c_int32 and args[6] is C.c_int32 and args[11] is C.c_float
    assert hasattr(C.CDLL(build.build(verbose=False)), "shine_normal_train_step")
    assert "shine_normal_step.hip" in build.sources()


# ---- 5. the pool keeps the normals in pool order
def test_sorted_pool_keeps_normals_in_pool_order_on_host_tensors(monkeypatch):
    from shine_mapping_amd import sampler

    n, L = 50, 3
    g = torch.Generator().manual_seed(0)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    slots = torch.zeros((n, L), dtype=torch.int32)
    monkeypatch.setattr(sampler, "plan_batch", lambda octree, coord, sort=True: (perm, slots))
    octree = type("O", (), {"_tables_epoch": 0})()
    coord, label, weight = torch.rand(n, 3, generator=g), torch.rand(n, generator=g), torch.rand(n, generator=g) - 0.5
    normal = torch.randn(n, 3, generator=g, dtype=torch.float64)
    pool = sampler.SortedPool(octree, coord, label, weight, normal_label=normal)
    assert pool.normal_label.dtype == torch.float32 and pool.normal_label.is_contiguous() and pool.normal_label.shape == (n, 3)
    assert torch.equal(pool.normal_label, normal[pool.perm.long()].float())
    assert not hasattr(pool, "sem_label")
    pool.rebuild(coord, label, weight)  # a rebuild without: nothing stale is kept
    assert not hasattr(pool, "normal_label")
    pool.rebuild(coord, label, weight, normal_label=normal.float(), sem_label=torch.zeros(n, dtype=torch.long))
    assert torch.equal(pool.normal_label, normal.float()[perm.long()]) and hasattr(pool, "sem_label")
    for wrong in (normal[:-1], normal[:, :2], normal.flatten()):
        with pytest.raises(ValueError, match="normal_label"):
            pool.rebuild(coord, label, weight, normal_label=wrong)
        with pytest.raises(ValueError, match="normal_label"):
            sampler.SortedPool(octree, coord, label, weight, normal_label=wrong)
    for fn in (sampler.SortedPool.__init__, sampler.SortedPool.rebuild):
        assert inspect.signature(fn).parameters["normal_label"].default is None
    assert "12 B per sample" in sampler.SortedPool.__init__.__doc__


# ---- 6. argument errors that need no launch
def test_public_surface_and_the_loop_s_argument_errors():
    import shine_mapping_amd as s
    from shine_mapping_amd import loop, losses, ops

    assert s.fused_normal_step is ops.fused_normal_step and s.normal_loss is losses.normal_loss
    sig = inspect.signature(ops.fused_normal_step)
    assert list(sig.parameters) == ["octree", "decoder", "coord", "weight", "normal_label", "weight_n", "n_surf", "pool", "idx",
                                    "grad_buffers", "out", "workspace"]
    assert all(sig.parameters[k].default is None for k in ("n_surf", "pool", "idx", "grad_buffers", "out", "workspace"))
    assert loop.NormalTerm().weight_n == 0.01 and loop.NormalTerm(0.05).weight_n == 0.05

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
    with pytest.raises(ValueError, match="SortedPool built with normal_label="):
        loop.GraphedIteration(octree, None, Pool(), Opt(), opts, 16, normal=loop.NormalTerm(0.05))
    with pytest.raises(ValueError, match=r"normal=\.\.\.\) needs the folded iteration"):
        loop.GraphedIteration(octree, None, Pool(), Opt(), opts, 16, fold=False, normal=loop.NormalTerm(0.05))
    with pytest.raises(ValueError, match=r"normal=\.\.\.\) needs the folded iteration"):
        loop.GraphedIteration(octree, None, Pool(), object(), opts, 16, normal=loop.NormalTerm(0.05))
    with pytest.raises(TypeError):
        loop.GraphedIteration(octree, None, Pool(), Opt(), opts, 16, normals=loop.NormalTerm(0.05))


def test_fused_normal_step_refuses_bad_arguments_before_any_launch():
    from shine_mapping_amd import ops

    class Octree:
        _tables_epoch = 3

        def _require_tables(self, probe=False):
            return None

    class Dec:
        def fused_params(self):
            return []

    pool = type("P", (), {"tables_epoch": 3, "rec": None})()
    with pytest.raises(ValueError, match="n_surf must be a contiguous CUDA int64 tensor"):  # (a Python int: the natural mistake)
        ops.fused_normal_step(Octree(), Dec(), None, None, None, 0.1, n_surf=512, pool=pool)
    with pytest.raises(ValueError, match="array mode needs coord"):
        ops.fused_normal_step(Octree(), Dec(), None, None, None, 0.1)
    with pytest.raises(ValueError, match="array mode needs coord"):
        ops.fused_normal_step(Octree(), Dec(), torch.zeros(4, 3), torch.zeros(4), None, 0.1)
    with pytest.raises(ValueError, match="pool mode needs idx"):
        ops.fused_normal_step(Octree(), Dec(), None, None, None, 0.1, pool=pool)
    with pytest.raises(ValueError, match="pool mode needs idx"):
        ops.fused_normal_step(Octree(), Dec(), None, None, None, 0.1, pool=pool, idx=torch.zeros(4, dtype=torch.int32))
