"""The time-conditioned decoder on the CPU: the references, pins and host logic behind tests/test_gpu_time_decoder.py
(tests/time_decoder_cases.py has the cases).

(1) the closed forms equal the reference's own Decoder.time_conditionded_sdf (model/decoder.py:65-81) differentiated by
torch.autograd in fp64 — in a child process: oracle.ref_import puts the reference's `model` / `utils` packages and inert stubs of
open3d and skimage into sys.modules, which the rest of the suite must not see;
(2) the pins are honest: on every case the fp32 composite's ratio is at most K / 4 in its family;
(3) Decoder.fused_params_at(ts) fed to the plain 8-wide closed form equals the time form at constant ts, in fp64;
(4) time_fusable is false for every other shape, and those run the composite;
(5) the three entry points refuse bad arguments on the host.
The FusedAdam test at the end needs a GPU.
"""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import tier_a_kernel_cases as tc
import time_decoder_cases as td
from conftest import ROOT
from test_tier_a_kernels import _within, one_thread  # noqa: F401  (one_thread is a fixture)

REF_N = 257


def _assert_same(what, got, ref, scale, tol=1e-12):
    for k in tc.MLP_POINT:
        _within(got[k], ref[k], scale[k], tol, "%s %s" % (what, k))
    for k in ("gw", "bb"):
        for i in range(6):
            _within(got[k][i], ref[k][i], scale[k][i], tol, "%s %s[%d]" % (what, k, i))


# ------------------------------------------------------------------------------------------------ (1) the references are right


def reference_check():
    """(the child process of the test below)"""
    from oracle import ref_import

    R = ref_import.install()
    cfg = R.SHINEConfig()
    cfg.device = "cpu"
    seen = 0
    for decoder in td.DECODERS:
        for kind, wt in td.variants(decoder):
            if kind == "zero":
                continue
            case, ref, scale = td.time_reference(decoder, kind, wt, REF_N)
            dec = R.Decoder(cfg, is_geo_encoder=True, is_time_conditioned=True).double()
            dec.load_state_dict(dict(zip(tc.svc.NAMES, [p.double() for p in case.params])), strict=False)

            leaves = [dec.layers[0].weight, dec.layers[0].bias, dec.layers[1].weight, dec.layers[1].bias, dec.lout.weight,
                      dec.lout.bias]
            f = case.feat.double().requires_grad_(True)
            g = case.g.double().requires_grad_(True)
            pred = dec.time_conditionded_sdf(f, case.ts.double())
            first = torch.autograd.grad(pred, [f] + leaves, g, create_graph=True)
            second = torch.autograd.grad((first[0] * case.r.double()).sum(), [g] + leaves, allow_unused=True)
            bb = [torch.zeros_like(p) if t is None else t for t, p in zip(second[1:], leaves)]
            got = dict(pred=pred.detach(), grad_feat=first[0].detach(), dg=second[0].detach(), gw=[t.detach() for t in first[1:]],
                       bb=[t.detach() for t in bb])
            _assert_same(td.case_id(decoder, kind, wt, REF_N), got, ref, scale)
            assert float(got["bb"][0][:, 8].abs().max()) == 0.0 and all(float(got["bb"][i].abs().max()) == 0.0 for i in (1, 3, 5))
            seen += 1
    print("reference agrees on %d cases" % seen)


def test_closed_forms_equal_the_references_decoder_under_autograd_in_fp64():
    from oracle import ref_import

    if not ref_import.available():
        pytest.skip("the reference checkout is not here")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, "-c", "import test_time_decoder as t; t.reference_check()"], capture_output=True,
                         text=True, timeout=600, cwd=os.path.join(ROOT, "tests"), env=env)
    assert out.returncode == 0 and "reference agrees on" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_the_composite_of_the_cases_file_is_the_closed_form_too():
    """td.composite — what the pins are measured on and what Decoder falls back to — against the closed forms, in fp64 (this one
    runs wherever the suite runs, the reference is not needed)"""
    for decoder in td.DECODERS:
        kind, wt = td.variants(decoder)[0]
        case, ref, scale = td.time_reference(decoder, kind, wt, REF_N)
        _assert_same(decoder, td.time_autograd(case, torch.float64), ref, scale)
        assert float(ref["bb"][0][:, 8].abs().max()) == 0.0  # the double backward sends nothing to the time column


# --------------------------------------------------------------------------------------------- (2) the pins, and the kink rule


def test_pins_follow_the_rule():
    assert td.K == {fam: 4.0 * max(rho, 1.0) for fam, rho in td.RHO_REF.items()}
    assert all(rho * 2 == int(rho * 2) for rho in td.RHO_REF.values())


@pytest.mark.parametrize("decoder", td.DECODERS)
def test_time_pins_are_honest_and_no_point_sits_near_a_kink(decoder, one_thread):
    for kind, wt in td.variants(decoder):
        for n in td.sizes(decoder, False):
            case, ref, scale = td.time_reference(decoder, kind, wt, n)
            assert int(tc.near_kink(case.params, td.widened(case).feat).sum()) == 0
            assert case.redrawn <= max(5, n // 25), "the kink rule redrew %d of %d points" % (case.redrawn, n)
            got = td.time_autograd(case, torch.float32)
            if n not in td.sizes(decoder, True):
                got["gw"] = got["bb"] = None
            rho = td.check_time("fp32 composite, " + td.case_id(decoder, kind, wt, n), got, ref, scale)
            for fam, v in rho.items():
                assert v <= td.K[fam] / 4.0, "%s: the fp32 composite's ratio %.3f exceeds K / 4 of %s" % (
                    td.case_id(decoder, kind, wt, n), v, fam)
    if decoder == "b1_third":
        dead = scale["gw"][0].abs().sum(1) == 0
        assert bool(dead[::3].all()) and not bool(dead.all())
    if decoder in ("on_kink", "dead_points"):
        assert bool(case.zero_points.any()) and float(case.ts[case.zero_points].abs().max()) == 0.0
        assert float(ref["grad_feat"][case.zero_points].abs().max()) == 0.0
    if decoder == "wt_zero":
        # (w_t = 0 takes nothing from the time column's own gradient: with ts != 0 it is as large as any other)
        assert float(case.params[0][:, 8].abs().max()) == 0.0
        assert float(td.time_reference(decoder, "frames", 0.0, td.SMALL)[2]["gw"][0][:, 8].max()) > 0.0
    else:
        assert bool((case.params[0][::5, 8] == 0).all()) and float(case.params[0][:, 8].abs().max()) > 0.0


def test_the_query_pin_is_honest_and_no_point_sits_near_a_kink(one_thread):
    for ts in td.QUERY_TS:
        coord, ref, scale = td.query_reference(ts)
        src = td.tc.svc.fixture(td.QUERY_FIXTURE)["source"]
        assert int(td._query_forms(td.query_weights(), coord, ts, src)[2].sum()) == 0 and float(scale.min()) > 0.0
        rho = float(tc.ratios(td.query_oracle32(ts), ref, scale).max())
        assert rho <= td.K["time_query"] / 4.0, "ts = %g: the fp32 oracle's ratio %.3f exceeds K / 4" % (ts, rho)


# ------------------------------------------------------------------------------------------------ (3) the fold, (4) the gates


def _cpu_decoder(time_conditioned=True, **over):
    from shine_mapping_amd import Decoder, synth

    cfg = synth.make_config("maicity", device="cpu", **over)
    return Decoder(cfg, is_time_conditioned=time_conditioned)


@pytest.mark.parametrize("ts", [0, 3, 250.5])
def test_fused_params_at_makes_the_plain_decoder_of_one_time_stamp(ts):
    case, _, _ = td.time_reference("fixture", "frames", 0.3, REF_N)
    dec = _cpu_decoder().double()
    with torch.no_grad():
        for p, w in zip(dec._layer_params(), case.params):
            p.copy_(w.double())
    for stamp in (ts, torch.tensor(ts, dtype=torch.float64)):
        folded = dec.fused_params_at(stamp)
        assert [tuple(p.shape) for p in folded] == [(32, 8), (32,), (32, 32), (32,), (1, 32), (1,)]
        assert all(not p.requires_grad and p.dtype == torch.float64 for p in folded) and folded[0].is_contiguous()
        plain = SimpleNamespace(params=folded, n=case.n, feat=case.feat, g=case.g, r=case.r)
        const = SimpleNamespace(**{**vars(case), "ts": torch.full((case.n,), float(ts), dtype=torch.float64)})
        want, scale = td.time_closed(const, False), td.time_closed(const, True)
        got = tc.mlp_closed(plain, False)
        for k in tc.MLP_POINT:
            _within(got[k], want[k], scale[k], 1e-12, k)
        for k in ("gw", "bb"):
            for i in range(6):
                w, s = (want[k][i][:, :8], scale[k][i][:, :8]) if i == 0 else (want[k][i], scale[k][i])
                _within(got[k][i], w, s, 1e-12, "%s[%d]" % (k, i))
    with pytest.raises(NotImplementedError):
        _cpu_decoder(False).fused_params_at(0)


def test_time_fusable_is_false_for_other_shapes_and_those_run_the_composite():
    good = _cpu_decoder()
    assert good.time_fusable and not good.fusable
    plain = _cpu_decoder(False)
    assert plain.fusable and not plain.time_fusable and len(plain.fused_params()) == 6
    with pytest.raises(NotImplementedError):
        good.fused_params()
    others = [_cpu_decoder(geo_mlp_hidden_dim=64), _cpu_decoder(geo_mlp_level=3), _cpu_decoder(geo_mlp_bias_on=False),
              _cpu_decoder(feature_dim=4)]
    gen = torch.Generator().manual_seed(5)
    for dec in [good] + others:
        assert dec.time_fusable == (dec is good) and not dec.fusable
        f = torch.randn(33, dec.layers[0].in_features - 1, generator=gen)
        ts = torch.randint(0, 10, (33, 1), generator=gen).float()
        h = torch.cat((f, ts.view(-1, 1)), dim=1)
        for l in dec.layers:
            h = torch.relu(l(h))
        assert torch.equal(dec.time_conditionded_sdf(f, ts), dec.lout(h).squeeze(1))  # (CPU input: the composite, also for `good`)


# -------------------------------------------------------------------------------------------------- (5) host-side argument checks


def test_time_entry_points_refuse_bad_arguments_without_a_device():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(64)  # (never dereferenced: every call below returns on the host)
    six = _lib.ptr_array([64] * 6)
    holed = _lib.ptr_array([64, 64, None, 64, 64, 64])
    INVALID = -1
    assert lib.shine_time_mlp_forward(p, p, -1, six, p, None) == INVALID
    assert lib.shine_time_mlp_forward(None, p, 8, six, p, None) == INVALID
    assert lib.shine_time_mlp_forward(p, None, 8, six, p, None) == INVALID
    assert b"shine_time_mlp_forward" in lib.shine_error_string(-1)
    assert lib.shine_time_mlp_forward(p, p, 8, None, p, None) == INVALID
    assert lib.shine_time_mlp_forward(p, p, 8, holed, p, None) == INVALID
    assert lib.shine_time_mlp_forward(p, p, 8, six, None, None) == INVALID
    assert lib.shine_time_mlp_backward(p, p, p, -1, six, p, six, None) == INVALID
    assert lib.shine_time_mlp_backward(p, None, p, 8, six, p, six, None) == INVALID
    assert lib.shine_time_mlp_backward(p, p, None, 8, six, p, six, None) == INVALID
    assert b"shine_time_mlp_backward" in lib.shine_error_string(-1)
    assert lib.shine_time_mlp_backward(p, p, p, 8, holed, p, six, None) == INVALID
    assert lib.shine_time_mlp_backward(p, p, p, 8, six, p, holed, None) == INVALID
    assert lib.shine_time_mlp_backward_backward(p, p, p, p, -1, six, p, six, None) == INVALID
    assert lib.shine_time_mlp_backward_backward(p, None, p, p, 8, six, p, six, None) == INVALID
    assert lib.shine_time_mlp_backward_backward(p, p, None, p, 8, six, p, six, None) == INVALID
    assert lib.shine_time_mlp_backward_backward(p, p, p, None, 8, six, p, six, None) == INVALID
    assert b"shine_time_mlp_backward_backward" in lib.shine_error_string(-1)
    assert lib.shine_time_mlp_backward_backward(p, p, p, p, 8, holed, p, six, None) == INVALID
    # nothing to do: n == 0, or no output asked for — SHINE_OK without a launch
    assert lib.shine_time_mlp_forward(None, None, 0, six, None, None) == 0
    assert lib.shine_time_mlp_backward(None, None, None, 0, six, None, None, None) == 0
    assert lib.shine_time_mlp_backward_backward(None, None, None, None, 0, six, None, None, None) == 0
    assert lib.shine_time_mlp_backward(p, p, p, 8, six, None, None, None) == 0
    assert lib.shine_time_mlp_backward_backward(p, p, p, p, 8, six, None, None, None) == 0


# ---------------------------------------------------------------------------------------------------------------- the optimiser


@pytest.mark.gpu
def test_fused_adam_steps_the_288_element_first_layer_like_torch_adam():
    """setup_optimizer on a time-conditioned decoder (W1 [32,9]: 288 elements, rows that are no multiple of 16 bytes) and one feature
    level: three steps against torch.optim.Adam with the reference's groups, at the bound of test_fused_adam_matches_torch_adam"""
    from shine_mapping_amd import Decoder, synth
    from shine_mapping_amd.optim import FusedAdam, setup_optimizer
    from test_gpu_parity import rel_err

    cfg = synth.make_config("maicity", device="cuda", tree_level_feat=1)
    dec = Decoder(cfg, is_time_conditioned=True)
    assert dec.time_fusable and tuple(dec.layers[0].weight.shape) == (32, 9)
    gen = torch.Generator().manual_seed(9)
    feat = torch.nn.Parameter(torch.randn(1001, 8, generator=gen).cuda())
    opt = setup_optimizer(cfg, [feat], list(dec.parameters()))
    assert isinstance(opt, FusedAdam)
    ps = dec._layer_params() + [feat]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ref = torch.optim.Adam([{"params": qs[:6], "lr": cfg.lr, "weight_decay": cfg.weight_decay}, {"params": [qs[6]], "lr": cfg.lr}],
                           betas=(0.9, 0.99), eps=getattr(cfg, "adam_eps", 1e-15))
    for it in range(3):
        for p, q in zip(ps, qs):
            gr = torch.randn(p.shape, generator=gen).cuda() * (10.0 ** (it - 1))
            p.grad, q.grad = gr.clone(), gr.clone()
        ref.step()
        opt.step(zero_grad=True)
        for p, q in zip(ps, qs):
            assert rel_err(p, q) <= 2e-6
            assert float(p.grad.abs().max()) == 0.0
