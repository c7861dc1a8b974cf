"""CPU: the sdf_l1 / sdf_l2 and ray-rendering (dr, dr_neus) objectives — the stored reference values (tests/golden/loss_modes.pt,
tools/make_loss_golden.py), the torch composites the GPU tests hold the HIP kernels to at scale, the drop-in's re-binding of
utils.loss.sdf_diff_loss / batch_ray_rendering_loss, the C ABI's declarations and host-side argument checks, and the fused
optimiser's learnable sigma_size group (utils/tools.py:74-76)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

FIXTURE = os.path.join(GOLDEN_DIR, "loss_modes.pt")


def load_fixture():
    return torch.load(FIXTURE, map_location="cpu", weights_only=False)


# ---- composites written from the formulas (the fixture pins them to the reference): the at-scale GPU checks use them

def composite_diff(pred, label, weight, scale, l2_loss):
    """mean over the N points of weight * ((pred - label) / scale)^2 (l2) or weight * |(pred - label) / scale| (l1)"""
    r = (pred - label) / scale
    per = r ** 2 if l2_loss else r.abs()
    return (weight * per).sum() / pred.shape[0]


def rendered_depth(x, y, neus_on, stable=False):
    """per ray: samples in depth order; alphas = the probabilities (dr) or clamp((y[i+1] - y[i]) / (1 - y[i] + 1e-10), 0, 1)
    (dr_neus); o = (1 - a) + 1e-10; w = cumprod(o) / o * a; sum w x.  stable: the order the kernel documents and no torch
    version or machine changes — equal depths keep their column order (torch.sort promises nothing about them without it) and
    the samples are added front to back (torch.sum's order over a short row depends on the vector width: the last bit of the
    depth, and with it sgn(d - d_meas) of a ray rendered exactly onto its measurement)"""
    depth, order = x.sort(dim=1, stable=True) if stable else x.sort(dim=1)
    prob = y.gather(1, order)
    if neus_on:
        lo, hi = prob[:, :-1], prob[:, 1:]
        a = ((hi - lo) / (1.0 - lo + 1e-10)).clamp(0.0, 1.0)
    else:
        a = prob
    o = torch.ones_like(a) - a + 1e-10
    w = o.cumprod(dim=1) / o * a
    t = w * depth[:, :a.shape[1]]
    if not stable:
        return t.sum(dim=1)
    d = t[:, :0].sum(dim=1)
    for k in range(t.shape[1]):
        d = d + t[:, k]
    return d


def composite_ray(x, y, d_meas, neus_on, stable=False):
    """the mean over rays of |rendered_depth - d_meas|"""
    return (rendered_depth(x, y, neus_on, stable) - d_meas).abs().mean()


def grad_close(got, ref, tol):
    """per ray: |got - ref| <= tol * max(1, max |ref of that ray|) (saturated rows carry very large, finite gradients)"""
    got, ref = got.double(), ref.double()
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1.0)
    worst = float(((got - ref).abs() / scale).max())
    return worst <= tol, worst


# ---- the sweep over every sample count and launch shape: CPU generators, so the conditions on the inputs can be checked here and
# are the same on every machine; tests/test_gpu_loss_modes.py runs the kernels on exactly these inputs

SWEEP_RAYS = 300  # three 128-ray chunks, the last ragged
ZERO_GRAD_ROW = 6  # d_meas is the row's own rendered depth


def ray_inputs(R, S, seed):
    """x = 20 rand + 0.5, y = sigmoid(1.5 randn), d_meas = 20 rand + 0.5"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(R, S, generator=g) * 20.0 + 0.5
    y = torch.sigmoid(torch.randn(R, S, generator=g) * 1.5)
    d = torch.rand(R, generator=g) * 20.0 + 0.5
    return x, y, d


def ray_sweep_case(S, neus):
    """ray_inputs with the edge rows (S >= 2): 0 all depths equal, 1 one pair of equal depths, 2 a leading 0, 3 a trailing 1,
    4 all ones, 5 all zeros (with dr_neus the last sample's quotient against the padding column behind it is 0 / 1, inside the
    clamp: the row that pins the backward loop's `k < A` guard at every S below its network's width), 6 the measurement equal
    to the rendered depth of the float32 composite (sgn(0) = 0)"""
    x, y, d = ray_inputs(SWEEP_RAYS, S, 1000 + 2 * S + int(neus))
    if S >= 2:
        x[0, :] = x[0, 0]
        x[1, 1] = x[1, 0]
        y[2, 0] = 0.0
        y[3, S - 1] = 1.0
        y[4, :] = 1.0
        y[5, :] = 0.0
        d[ZERO_GRAD_ROW] = rendered_depth(x, y, neus, stable=True)[ZERO_GRAD_ROW]
    return x, y, d


def saturated_rows(y):
    """rays with a probability of exactly 0 or 1: the gradient's autograd form is a difference of ~1e10-sized terms there, and
    only the float32 composite's own roundings specify it"""
    return ((y == 0) | (y == 1)).any(dim=1)


def fp64_rows(y, with_edges):
    """the rays an fp64 evaluation can judge: unsaturated ones, without the row whose measurement IS the float32 rendered
    depth — its gradient is sgn(d - d_meas) at the jump: 0 in float32, +-1 times the weights as soon as d is rounded otherwise"""
    rows = ~saturated_rows(y)
    if with_edges:
        rows[ZERO_GRAD_ROW] = False
    return rows


def ray_reference(x, y, d_meas, neus, dtype):
    """(loss, d loss / d y) of the stable composite evaluated in `dtype` on the inputs' device"""
    yy = y.detach().clone().to(dtype).requires_grad_(True)
    loss = composite_ray(x.to(dtype), yy, d_meas.to(dtype), neus, stable=True)
    (g,) = torch.autograd.grad(loss, yy)
    return loss.detach(), g


def ray_distance(got, ref, rows):
    """grad_close's unit over `rows`: the per-ray error of the per-ray gradient (x R) over max(1, largest |ref| in the ray)"""
    R = got.shape[0]
    return grad_close(got[rows].cpu() * R, ref[rows].cpu() * R, 0.0)[1]


@pytest.mark.parametrize("neus", [False, True])
def test_ray_sweep_recipe_holds_its_conditions(neus):
    for S in range(1, 33):
        x, y, d = ray_sweep_case(S, neus)
        loss_a, ga = ray_reference(x, y, d, neus, torch.float32)
        loss_b, gb = ray_reference(x, y, d, neus, torch.float64)
        assert ga.dtype == torch.float32 and gb.dtype == torch.float64 and ga.shape == gb.shape == (SWEEP_RAYS, S)
        assert torch.isfinite(ga).all() and torch.isfinite(loss_a), (S, neus)
        sat = saturated_rows(y)
        rows = fp64_rows(y, S >= 2)
        e_ref = ray_distance(ga, gb, rows)
        print("S=%2d neus=%d  e_ref = %.3e over %d rows, |loss A - loss B| / loss B = %.3e"
              % (S, neus, e_ref, int(rows.sum()), abs(float(loss_a) - float(loss_b)) / float(loss_b)))
        assert e_ref < 1e-4, (S, neus, e_ref)
        if S == 1:
            assert not sat.any()
            if neus:  # no alpha at all: every ray renders 0
                assert torch.equal(loss_a, d.abs().mean()) and float(ga.abs().max()) == 0.0
            continue
        assert bool((x[0] == x[0, 0]).all()) and float(x[1, 1]) == float(x[1, 0])
        assert sat[2:6].all() and not sat[:2].any() and not sat[ZERO_GRAD_ROW] and int(sat.sum()) == 4, (S, neus)
        assert float(y[2, 0]) == 0.0 and float(y[3, S - 1]) == 1.0 and bool((y[4] == 1).all()) and bool((y[5] == 0).all())
        assert float(ga[ZERO_GRAD_ROW].abs().max()) == 0.0, (S, neus)  # d == d_meas: sgn(0) = 0
        assert int(rows.sum()) == SWEEP_RAYS - 5
        # a permutation of row 0's probabilities is another ray (the stable order of equal depths is the column order)
        if S >= 3 or float(y[0, 0]) != float(y[0, 1]):
            yp = y.clone()
            yp[0] = y[0].flip(0)
            assert not torch.equal(ray_reference(x, yp, d, neus, torch.float32)[1][0], ga[0].flip(0)), (S, neus)


LAUNCH_RAYS = (1, 127, 128, 129, 256, 131072, 131073, 131072 + 128 * 5 + 3)  # one workgroup (the gridDim == 1 branch), two,
# exactly 1024 chunks, the chunk-stride pass (one more chunk, five more and a ragged one)
LAUNCH_SAMPLES = (1, 8, 17, 32)
DIFF_SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 1 << 20, (1 << 20) + 1, (1 << 20) + 1025)  # 1024 points per workgroup, 1024
# workgroups at most
DIFF_SCALES = (0.0390625, -0.1)


def diff_inputs(n, seed):
    """pred, label, weight: every fifth label equal to the prediction, every seventh weight zero, both from index 1 on (the
    point of n = 1 carries a difference and a weight)"""
    g = torch.Generator().manual_seed(seed)
    pred, label, weight = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.rand(n, generator=g)
    label[1::5] = pred[1::5]
    weight[1::7] = 0.0
    return pred, label, weight


def test_launch_shape_recipes_hold_their_conditions():
    for S in LAUNCH_SAMPLES:
        for R in LAUNCH_RAYS[:5]:
            x, y, d = ray_inputs(R, S, 2000 + S)
            assert not saturated_rows(y).any() and x.shape == y.shape == (R, S) and d.shape == (R,)
    chunks = [(R + 127) // 128 for R in LAUNCH_RAYS]
    assert chunks == [1, 1, 1, 2, 2, 1024, 1025, 1030]
    for n in DIFF_SIZES:
        pred, label, weight = diff_inputs(n, 3000 + n)
        assert torch.equal(pred[1::5], label[1::5]) and bool((weight[1::7] == 0).all())
        assert bool((pred[::5] != label[::5]).all()) and bool((weight[::7] > 0).all())  # (index 0 among them: n = 1 is no zero)
    assert [(n + 1023) // 1024 for n in DIFF_SIZES] == [1, 1, 1, 1, 1, 1, 2, 1024, 1025, 1026]


def test_composites_reproduce_the_reference_fixture():
    torch.set_num_threads(1)
    fx = load_fixture()
    assert len(fx["ray"]) == 8 and len(fx["sdf"]) == 4
    for case in fx["ray"]:
        y = case["y"].clone().requires_grad_(True)
        loss = composite_ray(case["x"], y, case["d_meas"], case["neus"])
        loss.backward()
        assert abs(float(loss.detach()) - float(case["loss"])) <= 1e-6 * abs(float(case["loss"]))
        ok, worst = grad_close(y.grad, case["grad_y"], 1e-6)
        assert ok, (case["neus"], case["S"], worst)
        assert torch.isfinite(case["grad_y"]).all()
    for case in fx["sdf"]:
        p = case["pred"].clone().requires_grad_(True)
        loss = composite_diff(p, case["label"], case["weight"], case["scale"], case["l2"])
        loss.backward()
        assert abs(float(loss.detach()) - float(case["loss"])) <= 1e-6 * abs(float(case["loss"]))
        assert float((p.grad - case["grad_pred"]).abs().max()) <= 1e-6 * max(1.0, float(case["grad_pred"].abs().max()))


def test_fixture_covers_the_edge_rows():
    """saturated probabilities, rows whose rendered depth equals the measurement (zero gradient), zero differences / weights"""
    fx = load_fixture()
    assert sorted({c["S"] for c in fx["ray"]}) == [2, 6, 9, 32] and {c["neus"] for c in fx["ray"]} == {False, True}
    for case in fx["ray"]:
        y = case["y"]
        assert bool(((y == 0) | (y == 1)).any())
        assert float(case["grad_y"][6].abs().max()) == 0.0  # d == d_meas: sgn(0) = 0
        assert all(len(set(r.tolist())) == r.numel() for r in case["x"])  # distinct, unsorted depths
        assert not bool((case["x"][:, 1:] >= case["x"][:, :-1]).all())
    for case in fx["sdf"]:
        assert bool((case["pred"] == case["label"]).any()) and bool((case["weight"] == 0).any())
    assert {(c["l2"]) for c in fx["sdf"]} == {False, True}


def test_library_composites_are_the_test_composites():
    """losses.py's fallback (CPU tensors here) is the same composite"""
    from shine_mapping_amd import losses

    fx = load_fixture()
    for case in fx["ray"]:
        ya, yb = case["y"].clone().requires_grad_(True), case["y"].clone().requires_grad_(True)
        la = losses.batch_ray_rendering_loss(case["x"], ya, case["d_meas"], case["neus"])
        lb = composite_ray(case["x"], yb, case["d_meas"], case["neus"])
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(ya.grad, yb.grad)
    for case in fx["sdf"]:
        la = losses.sdf_diff_loss(case["pred"], case["label"], case["weight"], case["scale"], case["l2"])
        assert torch.equal(la, composite_diff(case["pred"], case["label"], case["weight"], case["scale"], case["l2"]))


@pytest.mark.reference
def test_fixture_regenerates_bit_identically_from_the_live_reference():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_loss_golden.py"), "--check"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "identical" in out.stdout, out.stdout + out.stderr[-2000:]


def test_header_declares_the_loss_mode_entry_points():
    text = open(os.path.join(ROOT, "include", "shine_hip.h")).read()
    for sym in ("shine_sdf_diff_loss", "shine_ray_render_loss"):
        assert "int %s(" % sym in text
    assert "SHINE_LOSS_WORKSPACE_BYTES" in text and "SHINE_RAY_MAX_SAMPLES 32" in text
    from shine_mapping_amd import _lib, losses

    assert "shine_sdf_diff_loss" in _lib.exported_symbols() and "shine_ray_render_loss" in _lib.exported_symbols()
    assert losses.LOSS_WORKSPACE_BYTES == 16384 and losses.RAY_MAX_SAMPLES == 32


def test_loss_mode_argument_checks_do_not_need_a_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(64)  # (never dereferenced: every call below is refused on the host)
    assert lib.shine_ray_render_loss(p, p, p, 16, 33, 0, p, p, p, None) == -1
    assert b"32" in lib.shine_error_string(-1)
    assert lib.shine_ray_render_loss(p, p, p, 0, 6, 0, p, p, p, None) == -1
    assert lib.shine_ray_render_loss(p, p, p, 16, 0, 0, p, p, p, None) == -1
    assert lib.shine_ray_render_loss(p, p, p, 16, 6, 1, p, p, None, None) == -1
    assert lib.shine_ray_render_loss(None, p, p, 16, 6, 1, p, p, p, None) == -1
    assert lib.shine_sdf_diff_loss(p, p, p, 0, 0.1, 1, p, p, p, None) == -1
    assert lib.shine_sdf_diff_loss(p, p, None, 8, 0.1, 1, p, p, p, None) == -1
    assert lib.shine_sdf_diff_loss(p, p, p, 8, 0.0, 1, p, p, p, None) == -1
    assert lib.shine_sdf_diff_loss(p, p, p, 8, 0.1, 1, p, p, None, None) == -1


def test_setup_optimizer_appends_the_sigma_group():
    """utils/tools.py:74-76: with ray_loss the learnable sigma_size is the last group, at lr, without weight decay; the fused
    optimiser's state_dict numbers it after the feature levels (CPU tensors: no step is taken)"""
    from types import SimpleNamespace

    from shine_mapping_amd.optim import FusedAdam, setup_optimizer

    cfg = SimpleNamespace(lr=0.01, weight_decay=1e-7, tree_level_feat=3, lr_level_reduce_ratio=0.5, adam_eps=1e-15,
                          opt_adam=True, semantic_on=False, ray_loss=True)
    feats = [torch.nn.Parameter(torch.zeros(5, 8)) for _ in range(3)]
    dec = [torch.nn.Parameter(torch.zeros(4, 4)), torch.nn.Parameter(torch.zeros(4))]
    sigma = torch.nn.Parameter(torch.ones(1))
    opt = setup_optimizer(cfg, feats, dec, None, sigma)
    assert isinstance(opt, FusedAdam) and len(opt.param_groups) == 5
    last = opt.param_groups[-1]
    assert last["params"] == [sigma] and last["params"][0] is sigma and last["lr"] == 0.01 and last["weight_decay"] == 0.0
    assert [g["lr"] for g in opt.param_groups] == [0.01, 0.01, 0.005, 0.0025, 0.01]
    sd = opt.state_dict()
    assert sd["param_groups"][-1]["params"] == [5] and sd["state"] == {}
    # a bare tensor as a group's params is one parameter, as torch.optim takes it (the reference passes sigma_size so)
    assert FusedAdam([{"params": sigma, "lr": 0.1}]).param_groups[0]["params"][0] is sigma
    cfg.ray_loss = False
    assert len(setup_optimizer(cfg, feats, dec, None, sigma).param_groups) == 4
    cfg.ray_loss = True
    with pytest.raises(ValueError):
        setup_optimizer(cfg, feats, dec, None, None)
    cfg.semantic_on = True
    with pytest.raises(NotImplementedError):
        setup_optimizer(cfg, feats, dec, None, sigma)


_LOSS_STAND_IN = (
    "import torch\n"
    "def sdf_bce_loss(pred, label, sigma, weight, weighted=False, bce_reduction='mean'):\n"
    "    f = torch.nn.BCEWithLogitsLoss(reduction=bce_reduction, weight=weight if weighted else None)\n"
    "    return f(pred, torch.sigmoid(label / sigma))\n"
    "def sdf_diff_loss(pred, label, weight, scale, l2_loss=True):\n"
    "    from test_loss_modes import composite_diff\n"
    "    return composite_diff(pred, label, weight, scale, l2_loss)\n"
    "def batch_ray_rendering_loss(x, y, d_meas, neus_on=True):\n"
    "    from test_loss_modes import composite_ray\n"
    "    return composite_ray(x, y, d_meas, neus_on)\n"
)

_TOOLS_STAND_IN = (
    "import torch\n"
    "def get_gradient(inputs, outputs):\n"
    "    return torch.autograd.grad(outputs, inputs, torch.ones_like(outputs), create_graph=True)[0]\n"
    "def setup_optimizer(config, octree_feat, mlp_geo_param, mlp_sem_param, sigma_size):\n"
    "    groups = [{'params': mlp_geo_param, 'lr': config.lr, 'weight_decay': config.weight_decay}]\n"
    "    groups += [{'params': octree_feat[config.tree_level_feat - i - 1], 'lr': config.lr}\n"
    "               for i in range(config.tree_level_feat)]\n"
    "    if config.ray_loss:\n"
    "        groups.append({'params': sigma_size, 'lr': config.lr})\n"
    "    return torch.optim.Adam(groups, betas=(0.9, 0.99), eps=config.adam_eps)\n"
)


def test_dropin_rebinds_the_loss_mode_functions(tmp_path):
    """`import shine_mapping_amd.dropin` re-binds utils.loss.sdf_diff_loss / batch_ray_rendering_loss (the drivers take them
    with `from utils.loss import *`, shine_batch.py:15) next to sdf_bce_loss: status() says so, `_shine_reference` keeps the
    originals, names a driver imported before the drop-in are re-bound, CPU tensors through the wrappers give the originals'
    results, the SHINE_DROPIN_FUSED_LOSS opt-out and uninstall() put the originals back; the optimiser wrapper takes the fused
    path for ray_loss only with a CUDA float32 sigma_size (CPU here: the reference's own)."""
    (tmp_path / "utils").mkdir()
    (tmp_path / "utils" / "__init__.py").write_text("")
    (tmp_path / "utils" / "loss.py").write_text(_LOSS_STAND_IN)
    (tmp_path / "utils" / "tools.py").write_text(_TOOLS_STAND_IN)
    code = (
        "import os, sys, types, torch\n"
        "sys.path.insert(0, %r)\n"
        "sys.path.insert(0, %r)\n"
    ) % (str(tmp_path), os.path.join(ROOT, "tests")) + (
        "import utils.loss as ul, utils.tools as ut\n"
        "orig = (ul.sdf_bce_loss, ul.sdf_diff_loss, ul.batch_ray_rendering_loss)\n"
        "drv = types.ModuleType('shine_batch'); sys.modules['shine_batch'] = drv\n"
        "exec('from utils.loss import *', drv.__dict__)  # a driver that imported before the drop-in\n"
        "import shine_mapping_amd.dropin as d\n"
        "from shine_mapping_amd import losses\n"
        "st = d.status()\n"
        "assert st['sdf_diff_loss'] is True and st['batch_ray_rendering_loss'] is True and st['sdf_bce_loss'] is True, st\n"
        "assert ul.sdf_diff_loss is losses.sdf_diff_loss and ul.batch_ray_rendering_loss is losses.batch_ray_rendering_loss\n"
        "assert ul._shine_reference == {'sdf_bce_loss': orig[0], 'sdf_diff_loss': orig[1], 'batch_ray_rendering_loss': orig[2]}\n"
        "assert drv.sdf_diff_loss is losses.sdf_diff_loss and drv.batch_ray_rendering_loss is losses.batch_ray_rendering_loss\n"
        "assert st['names_rebound_in_loaded_drivers'] == 3, st\n"
        "ns = {}\n"
        "exec('from utils.loss import *', ns)\n"
        "assert ns['sdf_diff_loss'] is losses.sdf_diff_loss and ns['batch_ray_rendering_loss'] is losses.batch_ray_rendering_loss\n"
        "g = torch.Generator().manual_seed(0)\n"
        "x = torch.rand(64, 9, generator=g) * 10; y = torch.rand(64, 9, generator=g); dm = torch.rand(64, generator=g) * 10\n"
        "for neus in (False, True):\n"
        "    ya, yb = y.clone().requires_grad_(True), y.clone().requires_grad_(True)\n"
        "    a, b = ns['batch_ray_rendering_loss'](x, ya, dm, neus), orig[2](x, yb, dm, neus)\n"
        "    a.backward(); b.backward()\n"
        "    assert torch.equal(a, b) and torch.equal(ya.grad, yb.grad)\n"
        "p = torch.randn(100, generator=g, requires_grad=True); lab = torch.randn(100, generator=g); w = torch.rand(100, generator=g)\n"
        "for l2 in (False, True):\n"
        "    assert torch.equal(ns['sdf_diff_loss'](p, lab, w, 0.1, l2), orig[1](p, lab, w, 0.1, l2))\n"
        "# ray_loss with a CPU sigma_size: the reference's own setup_optimizer\n"
        "cfg = types.SimpleNamespace(lr=0.01, weight_decay=1e-7, tree_level_feat=2, lr_level_reduce_ratio=1.0, adam_eps=1e-15,\n"
        "                            opt_adam=True, semantic_on=False, ray_loss=True)\n"
        "feats = [torch.nn.Parameter(torch.zeros(5, 8)) for _ in range(2)]\n"
        "opt = ut.setup_optimizer(cfg, feats, [torch.nn.Parameter(torch.zeros(3))], None, torch.nn.Parameter(torch.ones(1)))\n"
        "assert isinstance(opt, torch.optim.Adam) and len(opt.param_groups) == 4\n"
        "d.uninstall()\n"
        "assert (ul.sdf_bce_loss, ul.sdf_diff_loss, ul.batch_ray_rendering_loss) == orig\n"
        "assert drv.sdf_diff_loss is orig[1] and drv.batch_ray_rendering_loss is orig[2]\n"
        "os.environ['SHINE_DROPIN_FUSED_LOSS'] = '0'\n"
        "d.install()\n"
        "st = d.status()\n"
        "assert (ul.sdf_bce_loss, ul.sdf_diff_loss, ul.batch_ray_rendering_loss) == orig, st\n"
        "assert st['sdf_diff_loss'].startswith('off') and st['batch_ray_rendering_loss'].startswith('off'), st\n"
        "print('ok')\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]


def test_dropin_leaves_a_loss_module_without_the_new_names_alone(tmp_path):
    (tmp_path / "utils").mkdir()
    (tmp_path / "utils" / "__init__.py").write_text("")
    (tmp_path / "utils" / "loss.py").write_text(_LOSS_STAND_IN.split("def sdf_diff_loss")[0])
    code = (
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "import utils.loss as ul\n"
        "import shine_mapping_amd.dropin as d\n"
        "st = d.status()\n"
        "assert st['sdf_bce_loss'] is True and 'sdf_diff_loss' not in st and 'batch_ray_rendering_loss' not in st, st\n"
        "assert not hasattr(ul, 'sdf_diff_loss') and not hasattr(ul, 'batch_ray_rendering_loss')\n"
        "assert list(ul._shine_reference) == ['sdf_bce_loss']\n"
        "d.uninstall()\n"
        "assert not hasattr(ul, 'sdf_diff_loss')\n"
        "print('ok')\n"
    ) % str(tmp_path)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]
