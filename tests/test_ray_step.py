"""The ray-rendering training step on the CPU: the oracle behind tests/test_gpu_ray_step.py (tests/ray_step_oracle.py), its pin,
and the host logic of shine_ray_step / sampler.RayPool / LiDARDataset.ray_pool / GraphedIteration's ray route.

(1) the oracle equals the reference's own batch_ray_rendering_loss + the drivers' lines under torch.autograd in fp64 — in a child
    process, as tests/test_time_step.py does it;
(2) the pin is honest: on every case the fp32 torch evaluation is within TOL / 4 of the wide one (loss, pred, dpred, every gradient
    tensor, d loss / d sigma_size among them);
(3) shine_ray_step refuses bad arguments on the host, each in its own words, and answers the size query;
(4) RayPool / ray_pool() / GraphedIteration argument errors that need no device, and the public surface.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import ray_step_oracle as ro
from conftest import ROOT

TOL = 1e-4  # tests/test_gpu_parity.py's (imported there; spelled here so that this file needs nothing of the GPU suite)

REF_CASES = [("kitti_eik_L3", 6), ("edges_L2_nopoly_eik", 9), ("maicity_bce_L4", 6)]


# ------------------------------------------------------------------------------------------------ (1) the oracle is the reference's
def reference_check():
    """(the child process of the test below)"""
    from oracle import ref_import

    R = ref_import.install()
    from utils.loss import batch_ray_rendering_loss  # (the reference's)

    seen = 0
    for name, S in REF_CASES:
        fx, coord, weight, depth, ray_depth = ro.inputs(name, S)
        m = ray_depth.numel()
        for neus in (False, True):
            for eik in (False, True):
                ssv = ro.sigma_size_of(neus, S)
                oct_, mlp = ro.oracle_for(fx, wide=True, scale=ro.out_scale(name, neus))
                mine = ro.ray_step(oct_, mlp, coord, weight, depth, ray_depth, ssv, fx["sigma"], S, neus=neus, eik=eik,
                                   weight_e=ro.weight_e_of(fx))
                oct_.zero_grad()
                mlp.zero_grad()
                ss = torch.tensor([ssv], dtype=torch.float64, requires_grad=True)
                delta = torch.zeros(coord.shape, dtype=torch.float64, requires_grad=True)
                pred = mlp.sdf(ro.to.wide_features(oct_, coord, delta))
                pred_occ = torch.sigmoid(pred / ss)  # shine_batch.py:160-170
                pred_ray = pred_occ.reshape(m, -1)
                loss = batch_ray_rendering_loss(depth.double().reshape(m, -1), pred_ray, ray_depth.double(), neus_on=neus)
                if eik:
                    g = R.get_gradient(delta, pred) * fx["sigma"]
                    surface_mask = weight > 0
                    loss = loss + ro.weight_e_of(fx) * ((1.0 - g[surface_mask].norm(2, dim=-1)) ** 2).mean()  # shine_batch.py:182-185
                loss.backward()
                ref = dict(loss=loss.detach(), feat_grads=[t.grad.clone() for t in oct_.hier_features],
                           mlp_grads=[torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in mlp.params()]
                           + [ss.grad.clone()])
                loss_err, errs = ro.rel_errors(mine["loss"], mine["feat_grads"], mine["mlp_grads"], ref)
                assert loss_err <= 1e-12 and max(errs) <= 1e-10, (name, S, neus, eik, loss_err, errs)
                seen += 1
    print("reference agrees on %d cases" % seen)


def test_the_oracle_equals_the_references_lines_under_autograd_in_fp64():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_ray_step as t; t.reference_check()"], capture_output=True, text=True,
                         timeout=600, cwd=os.path.join(ROOT, "tests"), env=env)
    assert out.returncode == 0 and "reference agrees on" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ (2) the pin
@pytest.mark.parametrize("name,neus,eik,S", ro.CASES, ids=[ro.case_id(*c) for c in ro.CASES])
def test_the_pin_is_honest(name, neus, eik, S):
    """TOL is the GPU tests' bound against the wide oracle; the fp32 torch evaluation has to sit well inside it"""
    c = ro.case(name, neus, eik, S)
    oct_, mlp = ro.oracle_for(c.fx, wide=False, scale=c.out_scale)
    fp32 = ro.ray_step(oct_, mlp, c.coord, c.weight, c.depth, c.ray_depth, c.sigma_size, c.sigma, S, neus=neus, eik=eik,
                       weight_e=c.weight_e)
    loss_err, errs = ro.rel_errors(fp32["loss"], fp32["feat_grads"], fp32["mlp_grads"], c.wide)
    pred_err = float((fp32["pred"].double() - c.wide["pred"]).abs().max()) / max(1.0, float(c.wide["pred"].abs().max()))
    dp = c.wide["dpred"]
    dpred_err = float((fp32["dpred"].double() - dp).abs().max()) / float(dp.abs().max())
    print(ro.case_id(name, neus, eik, S), "loss %.1e pred %.1e dpred %.1e" % (loss_err, pred_err, dpred_err),
          " ".join("%.1e" % e for e in errs))
    assert len(errs) == len(c.wide["feat_grads"]) + 7
    assert loss_err <= TOL / 4 and pred_err <= TOL / 4 and dpred_err <= TOL / 4 and max(errs) <= TOL / 4, \
        (loss_err, pred_err, dpred_err, errs)
    assert float(c.wide["mlp_grads"][6].abs().max()) > 0.0  # sigma_size receives a gradient
    assert float(c.depth.view(-1, S)[1, 0]) == float(c.depth.view(-1, S)[1, S - 1])  # the tie


@pytest.mark.parametrize("neus", [False, True])
def test_the_oracles_render_is_the_projects_composite(neus):
    from shine_mapping_amd.losses import batch_ray_rendering_loss_composite

    for S in ro.SAMPLES:
        _, _, _, depth, ray_depth = ro.inputs("kitti_eik_L3", S)
        m = ray_depth.numel()
        gen = torch.Generator().manual_seed(S)
        y = torch.rand(m, S, generator=gen, dtype=torch.float64).requires_grad_(True)
        x, dm = depth.double().view(m, S), ray_depth.double()
        mine, theirs = ro.composite(x, y, dm, neus), batch_ray_rendering_loss_composite(x, y, dm, neus)
        gm, gt = torch.autograd.grad(mine, y)[0], torch.autograd.grad(theirs, y)[0]
        assert float(mine) == float(theirs) and torch.equal(gm, gt)


# ------------------------------------------------------------------------------------------------ (3) the host's refusals
def _call(**over):
    """shine_ray_step on fake non-null pointers (nothing is dereferenced before the refusals) -> (rc, message)"""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    cfg = _lib.StepConfig(n_levels=3, max_level=12, poly_int_on=1, sigma=0.1, inv_n=1.0, eikonal_on=1)
    fake = C.c_void_p(0x10000)
    six = _lib.ptr_array([0x10000] * 6)
    three = _lib.ptr_array([0x10000] * 3)
    rows = _lib.i64_array([4, 4, 4])
    need = C.c_size_t(1 << 24)
    a = dict(t=fake, cfg=C.byref(cfg), coord=fake, idx=None, weight=fake, sample_depth=fake, ray_depth=fake, sigma_size=fake,
             samples=6, neus_on=0, n_surf=fake, n_surf_parts=1, n_rays=64, feats=three, rows=rows, grad_feats=three, mlp=six,
             grad_mlp=six, sigma_grad=fake, pred_out=None, dpred_out=None, loss_out=fake, workspace=fake,
             workspace_bytes=C.byref(need), stream=None)
    a.update(over)
    rc = lib.shine_ray_step(*a.values())
    return rc, (lib.shine_error_string(rc) or b"").decode()


REFUSALS = [
    (dict(t=None), "null table handle"),
    (dict(cfg=None), "null config"),
    (dict(n_rays=-1), "n < 0"),
    (dict(feats=None), "null argument"),
    (dict(rows=None), "null argument"),
    (dict(loss_out=None), "null argument"),
    (dict(mlp=None), "null argument"),
    (dict(workspace=C.c_void_p(0x10010)), "workspace"),
    (dict(workspace_bytes=C.byref(C.c_size_t(4096))), "workspace too small"),
    (dict(workspace_bytes=None), "null workspace_bytes"),
    (dict(samples=0), "samples < 1"),
    (dict(samples=33), "more than SHINE_RAY_MAX_SAMPLES (32) samples per ray"),
    (dict(n_rays=(1 << 31) // 6), "n * samples exceeds 2^31 - 1 rows"),
    (dict(n_surf_parts=65), "n_surf_parts is 0 .. 64"),
    (dict(coord=None), "null argument"),
    (dict(sample_depth=None), "null argument"),
    (dict(ray_depth=None), "null argument"),
    (dict(sigma_size=None), "null argument"),
    (dict(weight=None), "null argument"),
    (dict(n_surf=None), "null argument"),
]


@pytest.mark.parametrize("over,text", REFUSALS)
def test_shine_ray_step_refuses_on_the_host(over, text):
    rc, msg = _call(**over)
    assert rc != 0 and msg.startswith("shine_ray_step: ") and text in msg, (rc, msg)


def test_the_size_query_answers():
    from shine_mapping_amd import autograd_ops

    need = C.c_size_t(0)
    rc, _ = _call(workspace=None, workspace_bytes=C.byref(need), t=None, cfg=None)  # (the query reads nothing else)
    assert rc == 0 and need.value == autograd_ops.ray_step_workspace_bytes() and need.value % 256 == 0
    # counters + (256 + 16) partial vectors of 1412 floats + (256 + 16) x 3 loss sums, each array at a 256-byte boundary
    assert need.value == 256 + 256 * 1412 * 4 + (16 * 1412 * 4 + 255) // 256 * 256 + 256 * 24 + 512
    rc, msg = _call(workspace_bytes=C.byref(C.c_size_t(need.value - 1)))
    assert rc != 0 and msg == "shine_ray_step: workspace too small"


# ------------------------------------------------------------------------------------------------ (4) Python argument errors
def test_ray_pool_validation():
    from shine_mapping_amd import sampler

    def build(m=4, S=6, **over):
        a = dict(coord=torch.zeros(m * S, 3), weight=torch.zeros(m * S), sample_depth=torch.zeros(m * S), ray_depth=torch.zeros(m))
        a.update(over)
        pool = sampler.RayPool.__new__(sampler.RayPool)
        pool.rebuild(a["coord"], a["weight"], a["sample_depth"], a["ray_depth"], samples=S)

    with pytest.raises(ValueError, match="samples must be 1 .. 32"):
        build(S=0)
    with pytest.raises(ValueError, match="samples must be 1 .. 32"):
        build(S=33)
    with pytest.raises(ValueError, match="rows per entry of ray_depth"):
        build(coord=torch.zeros(23, 3))
    with pytest.raises(ValueError, match="rows per entry of ray_depth"):
        build(sample_depth=torch.zeros(25))
    with pytest.raises(ValueError, match="rows per entry of ray_depth"):
        build(ray_depth=torch.zeros(5))
    with pytest.raises(ValueError, match="weight must be a float32 tensor"):
        build(weight=torch.zeros(24, dtype=torch.float64))
    with pytest.raises(ValueError, match="ray_depth must be a float32 tensor"):
        build(ray_depth=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="one CUDA device"):
        build()  # (CPU tensors: everything else holds)


def test_ray_pool_of_a_dataset_without_ray_loss_raises():
    from shine_mapping_amd.dataset import LiDARDataset

    ds = LiDARDataset.__new__(LiDARDataset)
    ds.config = type("Cfg", (), {"ray_loss": False})()
    with pytest.raises(ValueError, match="ray_loss"):
        ds.ray_pool()
    from shine_mapping_amd.rgbd import RGBDDataset

    assert RGBDDataset.ray_pool is LiDARDataset.ray_pool


def test_public_surface_and_the_loops_refusals_without_a_device():
    import inspect

    import shine_mapping_amd as s
    from shine_mapping_amd import Decoder, loop, ops, sampler, synth

    assert s.fused_ray_step is ops.fused_ray_step and "fused_ray_step" in s.__all__
    assert s.RayTerm is loop.RayTerm and s.RayPool is sampler.RayPool and {"RayTerm", "RayPool"} <= set(s.__all__)
    sig = inspect.signature(ops.fused_ray_step)
    assert list(sig.parameters) == ["octree", "decoder", "coord", "weight", "sample_depth", "ray_depth", "sigma_size", "opts",
                                    "samples", "neus_on", "n_surf", "pool", "idx", "grad_buffers", "sigma_grad", "out", "workspace",
                                    "pred_out", "dpred_out"]
    assert sig.parameters["neus_on"].default is False
    assert all(sig.parameters[k].default is None for k in list(sig.parameters)[10:])
    assert list(inspect.signature(sampler.RayPool.__init__).parameters) == ["self", "octree", "coord", "weight", "sample_depth",
                                                                             "ray_depth", "samples", "seed"]
    assert list(inspect.signature(sampler.RayPool.draw).parameters) == ["self", "n", "out", "graph_safe", "surf_out"]
    term = loop.RayTerm(sigma_size=torch.ones(1))
    assert term.neus_on is False

    cfg = synth.make_config("maicity", device="cpu")
    plain, timed = Decoder(cfg), Decoder(cfg, is_time_conditioned=True)

    class Opt:  # nothing is called before the argument checks
        param_groups = []

        def step(self, **kw):
            raise AssertionError("argument errors come first")

        def finish_iteration(self):
            pass

        def prepare_graph_safe(self, skip=()):
            raise AssertionError("argument errors come first")

    class Pool:
        coord = torch.zeros(4, 3)

        def surf_parts_buffer(self, n=None):
            raise AssertionError("argument errors come first")

    class Rays(Pool):
        surf_per_ray = torch.zeros(4, dtype=torch.int32)

        def surf_buffer(self):
            raise AssertionError("argument errors come first")

    octree = type("O", (), {"hier_features": [], "_tables_epoch": 0})()
    opts = s.StepOptions(sigma=0.1, ekional_loss_on=True)
    with pytest.raises(ValueError, match="needs a sampler.RayPool"):
        loop.GraphedIteration(octree, plain, Pool(), Opt(), opts, 16, ray=term)
    with pytest.raises(ValueError, match="needs ray=RayTerm"):
        loop.GraphedIteration(octree, plain, Rays(), Opt(), opts, 16)
    with pytest.raises(ValueError, match="time-conditioned decoder"):
        loop.GraphedIteration(octree, timed, Rays(), Opt(), opts, 16, ray=term)
    with pytest.raises(ValueError, match="lambda_forget"):
        loop.GraphedIteration(octree, plain, Rays(), Opt(), opts, 16, lambda_forget=1e5, ray=term)
    with pytest.raises(ValueError, match="sem="):
        loop.GraphedIteration(octree, plain, Rays(), Opt(), opts, 16, sem=loop.SemTerm(decoder=object()), ray=term)
    with pytest.raises(ValueError, match="normal="):
        loop.GraphedIteration(octree, plain, Rays(), Opt(), opts, 16, normal=loop.NormalTerm(0.05), ray=term)
    with pytest.raises(ValueError, match="consistency="):
        loop.GraphedIteration(octree, plain, Rays(), Opt(), opts, 16, consistency=loop.ConsistencyTerm(), ray=term)
