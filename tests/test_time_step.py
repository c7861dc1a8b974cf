"""The time-conditioned training step on the CPU: the oracle behind tests/test_gpu_time_step.py (tests/time_step_oracle.py), its
pin, and the host logic of shine_time_step / SortedPool(ts=) / GraphedIteration's time route.

(1) the oracle equals the reference's own Decoder.time_conditionded_sdf + sdf_bce_loss + the drivers' eikonal lines under
    torch.autograd in fp64 — in a child process, as tests/test_time_decoder.py does it;
(2) with w_t = 0 every output but dW1[:, 8] is oracle.shine_oracle.train_step's;
(3) the pin is honest: on every case the fp32 oracle is within TOL / 4 of the wide one;
(4) shine_time_step refuses bad arguments on the host, each in its own words, and answers the size query;
(5) SortedPool and GraphedIteration argument errors that need no device.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import time_step_oracle as to
from conftest import ROOT, oracle_from_golden

TOL = 1e-4  # tests/test_gpu_parity.py's (imported there; spelled here so that this file needs nothing of the GPU suite)

REF_CASES = [("kitti_eik_L3", "frames"), ("edges_L2_nopoly_eik", "unit"), ("maicity_bce_L4", "frames")]


# ------------------------------------------------------------------------------------------------ (1) the oracle is the reference's
def reference_check():
    """(the child process of the test below)"""
    from oracle import ref_import
    from oracle import shine_oracle as so

    R = ref_import.install()
    cfg = R.SHINEConfig()
    cfg.device = "cpu"
    seen = 0
    for name, kind in REF_CASES:
        fx, ts, w_t = to.inputs(name, kind)
        for eik in (False, True):
            oct_, mlp = to.oracle_for(fx, w_t, wide=True)
            mine = to.time_step(oct_, mlp, fx["coord"], fx["sdf_label"], fx["weight"], ts, fx["sigma"], eik=eik,
                                weight_e=to.weight_e_of(fx))
            dec = R.Decoder(cfg, is_geo_encoder=True, is_time_conditioned=True).double()
            dec.load_state_dict(dict(zip(so.OracleDecoder.NAMES, [p.detach().clone() for p in mlp.params()])), strict=False)
            leaves = [dec.layers[0].weight, dec.layers[0].bias, dec.layers[1].weight, dec.layers[1].bias, dec.lout.weight,
                      dec.lout.bias]
            oct_.zero_grad()
            delta = torch.zeros(fx["coord"].shape, dtype=torch.float64, requires_grad=True)
            pred = dec.time_conditionded_sdf(to.wide_features(oct_, fx["coord"], delta), ts.double())
            # (the label's sigmoid in fp32, as the oracle and the kernel take it: label_op = sigmoid(label / sigma))
            target = torch.sigmoid(fx["sdf_label"] / fx["sigma"]).double()
            loss = torch.nn.BCEWithLogitsLoss(reduction="mean")(pred, target)
            same = R.sdf_bce_loss(pred, fx["sdf_label"].double(), fx["sigma"], None, False, "mean")
            assert abs(float(same) - float(loss)) <= 1e-6 * abs(float(loss))
            if eik:
                g = R.get_gradient(delta, pred) * fx["sigma"]
                surface_mask = fx["weight"] > 0
                loss = loss + to.weight_e_of(fx) * ((1.0 - g[surface_mask].norm(2, dim=-1)) ** 2).mean()  # shine_batch.py:182-185
            loss.backward()
            ref = dict(loss=loss.detach(), feat_grads=[t.grad.clone() for t in oct_.hier_features],
                       mlp_grads=[torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in leaves])
            loss_err, errs = to.rel_errors(mine["loss"], mine["feat_grads"], mine["mlp_grads"], ref)
            assert loss_err <= 1e-12 and max(errs) <= 1e-10, (name, kind, eik, loss_err, errs)
            assert float((mine["pred"] - pred.detach()).abs().max()) <= 1e-12 * max(1.0, float(pred.abs().max()))
            seen += 1
    print("reference agrees on %d cases" % seen)


def test_the_oracle_equals_the_references_lines_under_autograd_in_fp64():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_time_step as t; t.reference_check()"], capture_output=True, text=True,
                         timeout=600, cwd=os.path.join(ROOT, "tests"), env=env)
    assert out.returncode == 0 and "reference agrees on" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ (2) w_t = 0 is the plain step
@pytest.mark.parametrize("eik", [False, True])
@pytest.mark.parametrize("name", to.FIXTURES)
def test_with_a_zero_time_column_the_step_is_the_plain_oracle_step(name, eik):
    from oracle import shine_oracle as so

    fx, ts, w_t = to.inputs(name, "wt_zero")
    assert float(w_t.abs().max()) == 0.0 and float(ts.max()) > 1.0
    oct_, mlp = to.oracle_for(fx, w_t, wide=False)
    mine = to.time_step(oct_, mlp, fx["coord"], fx["sdf_label"], fx["weight"], ts, fx["sigma"], eik=eik, weight_e=to.weight_e_of(fx))
    cfg, oct0, mlp0 = oracle_from_golden(fx)
    cfg.ekional_loss_on, cfg.weight_e = eik, to.weight_e_of(fx)
    assert abs(so.sigma_sigmoid(cfg) - fx["sigma"]) <= 1e-12
    ref = so.train_step(oct0, mlp0, fx["coord"], fx["sdf_label"], fx["weight"], cfg)
    got_mlp = [mine["mlp_grads"][0][:, :8].contiguous()] + mine["mlp_grads"][1:]
    loss_err, errs = to.rel_errors(mine["loss"], mine["feat_grads"], got_mlp, ref)
    # (the 9-wide first layer is another GEMM shape: its sums come in another order, nothing more)
    assert loss_err <= 1e-6 and max(errs) <= 2e-5, (loss_err, errs)
    assert float((mine["pred"] - ref["pred"]).abs().max()) <= 1e-5 * max(1.0, float(ref["pred"].abs().max()))
    assert float(mine["mlp_grads"][0][:, 8].abs().max()) > 0.0  # d1 . ts: the one output w_t = 0 does not silence


# ------------------------------------------------------------------------------------------------ (3) the pin
@pytest.mark.parametrize("name,kind,eik", to.CASES, ids=[to.case_id(*c) for c in to.CASES])
def test_the_pin_is_honest(name, kind, eik):
    """TOL is the GPU tests' bound against the wide oracle; the reference's own fp32 evaluation has to sit well inside it"""
    c = to.case(name, kind, eik)
    oct_, mlp = to.oracle_for(c.fx, c.w_t, wide=False)
    fp32 = to.time_step(oct_, mlp, c.coord, c.label, c.weight, c.ts, c.sigma, eik=eik, weight_e=c.weight_e)
    loss_err, errs = to.rel_errors(fp32["loss"], fp32["feat_grads"], fp32["mlp_grads"], c.wide)
    pred_err = float((fp32["pred"].double() - c.wide["pred"]).abs().max()) / max(1.0, float(c.wide["pred"].abs().max()))
    print(to.case_id(name, kind, eik), "loss %.1e pred %.1e" % (loss_err, pred_err), " ".join("%.1e" % e for e in errs))
    assert loss_err <= TOL / 4 and pred_err <= TOL / 4 and max(errs) <= TOL / 4, (loss_err, pred_err, errs)
    if kind != "wt_zero":
        assert float(c.wide["mlp_grads"][0][:, 8].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ (4) the host's refusals
def _call(**over):
    """shine_time_step on fake non-null pointers (nothing is dereferenced before the refusals) -> (rc, message)"""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    cfg = _lib.StepConfig(n_levels=3, max_level=12, poly_int_on=1, sigma=0.1, inv_n=1.0)
    fake = C.c_void_p(0x10000)
    six = _lib.ptr_array([0x10000] * 6)
    three = _lib.ptr_array([0x10000] * 3)
    rows = _lib.i64_array([4, 4, 4])
    need = C.c_size_t(1 << 24)
    a = dict(t=fake, cfg=C.byref(cfg), coord=fake, coord_stride=3, idx=None, label=fake, weight=fake, weight_stride=1, ts=fake,
             n_surf=fake, n_surf_parts=1, n=64, feats=three, rows=rows, grad_feats=three, mlp=six, grad_mlp=six, pred_out=None,
             loss_out=fake, workspace=fake, workspace_bytes=C.byref(need), stream=None)
    a.update(over)
    rc = lib.shine_time_step(*a.values())
    return rc, (lib.shine_error_string(rc) or b"").decode()


@pytest.mark.parametrize("over,text", [
    (dict(t=None), "null table handle"),
    (dict(cfg=None), "null config"),
    (dict(coord_stride=5), "coord_stride is 3"),
    (dict(n=-1), "n < 0"),
    (dict(ts=None), "null argument"),
    (dict(feats=None), "null argument"),
    (dict(loss_out=None), "null argument"),
    (dict(workspace=C.c_void_p(0x10010)), "workspace"),
    (dict(workspace_bytes=C.byref(C.c_size_t(4096))), "workspace too small"),
    (dict(workspace_bytes=None), "null workspace_bytes"),
    (dict(n=1 << 31), "n exceeds 2^31 - 1 rows"),
    (dict(mlp=None), "null argument"),
])
def test_shine_time_step_refuses_on_the_host(over, text):
    rc, msg = _call(**over)
    assert rc != 0 and msg.startswith("shine_time_step: ") and text in msg, (rc, msg)


def test_loss_weight_on_is_refused_and_the_size_query_answers():
    from shine_mapping_amd import _lib, autograd_ops

    cfg = _lib.StepConfig(n_levels=3, max_level=12, poly_int_on=1, sigma=0.1, inv_n=1.0, loss_weight_on=1)
    rc, msg = _call(cfg=C.byref(cfg))
    assert rc != 0 and msg.startswith("shine_time_step: loss_weight_on"), msg
    need = C.c_size_t(0)
    rc, _ = _call(workspace=None, workspace_bytes=C.byref(need), t=None, cfg=None)  # (the query reads nothing else)
    assert rc == 0 and need.value == autograd_ops.time_step_workspace_bytes() and need.value % 256 == 0
    # counters + (256 + 16) partial vectors of 1412 floats + (256 + 16) x 2 loss sums, each array at a 256-byte boundary
    assert need.value == 256 + 256 * 1412 * 4 + (16 * 1412 * 4 + 255) // 256 * 256 + 256 * 16 + 256
    rc, msg = _call(workspace_bytes=C.byref(C.c_size_t(need.value - 1)))
    assert rc != 0 and msg == "shine_time_step: workspace too small"


# ------------------------------------------------------------------------------------------------ (5) Python argument errors
def test_public_surface_and_argument_errors_without_a_device():
    import inspect

    import shine_mapping_amd as s
    from shine_mapping_amd import Decoder, loop, ops, sampler, synth

    assert s.fused_time_step is ops.fused_time_step and "fused_time_step" in s.__all__
    sig = inspect.signature(ops.fused_time_step)
    assert list(sig.parameters) == ["octree", "decoder", "coord", "sdf_label", "weight", "ts", "opts", "n_surf", "pool", "idx",
                                    "grad_buffers", "out", "workspace", "pred_out"]
    assert all(sig.parameters[k].default is None for k in list(sig.parameters)[7:])
    for fn in (sampler.SortedPool.__init__, sampler.SortedPool.rebuild):
        assert inspect.signature(fn).parameters["ts"].default is None
    # a pool's ts holds one stamp per sample (checked before anything is planned)
    pool = sampler.SortedPool.__new__(sampler.SortedPool)
    pool.n_class = None
    with pytest.raises(ValueError, match="one time stamp per pool sample"):
        pool.rebuild(torch.zeros(5, 3), torch.zeros(5), torch.zeros(5), ts=torch.zeros(4))
    # the accessor of the six tensors
    cfg = synth.make_config("maicity", device="cpu")
    plain, timed = Decoder(cfg), Decoder(cfg, is_time_conditioned=True)
    assert timed.time_fusable and not plain.time_fusable
    assert [tuple(p.shape) for p in timed.time_params()] == [(32, 9), (32,), (32, 32), (32,), (1, 32), (1,)]
    assert timed.time_params()[0] is timed.layers[0].weight
    with pytest.raises(NotImplementedError):
        plain.time_params()
    with pytest.raises(NotImplementedError):
        timed.fused_params()

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

    class TimedPool(Pool):
        ts = torch.zeros(4)

    octree = type("O", (), {"hier_features": [], "_tables_epoch": 0})()
    opts = s.StepOptions(sigma=0.1, ekional_loss_on=True)
    with pytest.raises(ValueError, match="SortedPool built with ts="):
        loop.GraphedIteration(octree, timed, Pool(), Opt(), opts, 16)
    with pytest.raises(ValueError, match="lambda_forget"):
        loop.GraphedIteration(octree, timed, TimedPool(), Opt(), opts, 16, lambda_forget=1e5)
    with pytest.raises(ValueError, match="sem="):
        loop.GraphedIteration(octree, timed, TimedPool(), Opt(), opts, 16, sem=loop.SemTerm(decoder=object()))
    with pytest.raises(ValueError, match="normal="):
        loop.GraphedIteration(octree, timed, TimedPool(), Opt(), opts, 16, normal=loop.NormalTerm(0.05))
    with pytest.raises(ValueError, match="consistency="):
        loop.GraphedIteration(octree, timed, TimedPool(), Opt(), opts, 16, consistency=loop.ConsistencyTerm())
