"""CPU: the semantic head (semantic_on) — the stored reference values (tests/golden/semantic.pt, tools/make_semantic_golden.py)
against Decoder._sem_composite, the C ABI's declarations and host-side argument checks of csrc/shine_semantic.hip, and the fused
optimiser's semantic group (utils/tools.py:64-66) with and without the drop-in."""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

FIXTURE = os.path.join(GOLDEN_DIR, "semantic.pt")
SEM_NAMES = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias", "nclass_out.weight", "nclass_out.bias")


def load_fixture():
    return torch.load(FIXTURE, map_location="cpu", weights_only=False)


def sem_config(device="cpu", classes=20):
    return SimpleNamespace(feature_dim=8, geo_mlp_hidden_dim=32, geo_mlp_bias_on=True, geo_mlp_level=2, sem_mlp_hidden_dim=32,
                           sem_mlp_bias_on=True, sem_mlp_level=2, sem_class_count=classes, device=device)


def decoder_from_case(case, device="cpu"):
    """the project's Decoder(is_geo_encoder=False) holding the case's parameters"""
    from shine_mapping_amd import Decoder

    dec = Decoder(sem_config(device, case["params"]["nclass_out.bias"].numel() - 1), is_geo_encoder=False)
    with torch.no_grad():
        for k, p in dec.named_parameters():
            p.copy_(case["params"][k])
    return dec


def ulp_close(a, b, ulps=8):
    """|a - b| within a few float32 ulp of the larger magnitude (another CPU's BLAS rounds the products differently)"""
    a, b = a.detach().double(), b.detach().double()
    tol = ulps * torch.finfo(torch.float32).eps * torch.maximum(a.abs(), b.abs()).clamp_min(1e-30)
    return bool(((a - b).abs() <= tol + 1e-12).all()), float((a - b).abs().max())


# ---- the sweeps over every class count and launch shape: CPU generators, so the conditions on the inputs can be checked here and
# are the same on every machine; tests/test_gpu_semantic.py runs the kernels on exactly these inputs

SWEEP_N = 321  # five 64-point tiles and one ragged lane, in two backward workgroups
TICKET_CLASSES = (1, 20, 32)
# backward workgroups (256 points each, 256 at most, ticket runs of 16): 1 .. 256 one; 257 two; 4096 a full run; 4097 a second run
# of one; 65281 / 65536 all 256 with a ragged / full last tile; 65537 / 69700 the grid-stride pass on one wave / on 17 workgroups
TICKET_SIZES = (1, 63, 64, 65, 256, 257, 4096, 4097, 65281, 65536, 65537, 69700)
FWD_STRIDE_N = 2048 * 256 + 257  # the forward's 2048 workgroups and a second pass on two of them


def sweep_params(C, seed=None):
    """W1, b1, W2, b2, Wc [C, 32], bc [C] drawn as nn.Linear draws them (uniform in +-1 / sqrt(fan_in))"""
    g = torch.Generator().manual_seed(100 + C if seed is None else seed)
    out = []
    for rows, cols in ((32, 8), (32, 32), (C, 32)):
        bound = cols ** -0.5
        out.append((torch.rand(rows, cols, generator=g) * 2 - 1) * bound)
        out.append((torch.rand(rows, generator=g) * 2 - 1) * bound)
    return out


def sweep_inputs(C, n=SWEEP_N, seed=None):
    """feat = 0.3 randn [n, 8], d loss / d logp = randn / n [n, C]"""
    g = torch.Generator().manual_seed(C if seed is None else seed)
    return torch.randn(n, 8, generator=g) * 0.3, torch.randn(n, C, generator=g) / n


def decoder_from_params(params, device="cpu"):
    """the project's Decoder(is_geo_encoder=False) holding the six tensors"""
    from shine_mapping_amd import Decoder

    dec = Decoder(sem_config(device, params[5].numel() - 1), is_geo_encoder=False)
    named = dict(dec.named_parameters())
    with torch.no_grad():
        for k, p in zip(SEM_NAMES, params):
            named[k].copy_(p)
    return dec


def kink_rows(params, f, eps=1e-5):
    """rows with a hidden pre-activation within eps of 0 (in fp64): float32 rounding may put them on either side of ReLU's kink,
    and the gradient jumps there"""
    ps = [p.detach().double() for p in params]
    z1 = f.double() @ ps[0].T + ps[1]
    z2 = torch.relu(z1) @ ps[2].T + ps[3]
    return (z1.abs() < eps).any(dim=1) | (z2.abs() < eps).any(dim=1)


def fp64_logits(params, f):
    ps = [p.detach().double() for p in params]
    h = torch.relu(torch.relu(f.double() @ ps[0].T + ps[1]) @ ps[2].T + ps[3])
    return h, h @ ps[4].T + ps[5]


def tie_pairs(C):
    """(i, j): row j of Wc and bc copied onto row i"""
    return [(0, C - 1)] + ([(2, 3)] if C >= 4 else [])


def value_case(kind, C):
    """the six tensors for the value tests: "ties" one pair (C >= 4: two pairs) of classes with bit-identical logits on every
    row, "large" logits of several hundred, "dead" no second-layer unit alive on any row"""
    p = [t.clone() for t in sweep_params(C, 300 + C)]
    if kind == "ties":
        p[0] *= 10.0  # (spread the logits: an untrained head labels every row alike)
        for i, j in tie_pairs(C):
            p[4][i], p[5][i] = p[4][j], p[5][j]
    elif kind == "large":
        p[0] *= 30.0
        p[4] *= 300.0
    elif kind == "dead":
        p[3].fill_(-10.0)
    else:
        raise ValueError(kind)
    return p


def test_sweep_inputs_stay_off_the_relu_kinks():
    """the fp64 composite is a reference only off the kinks: at most max(2, n // 100) rows within 1e-5 of one"""
    for C in range(1, 33):
        f, dlogp = sweep_inputs(C)
        assert f.shape == (SWEEP_N, 8) and dlogp.shape == (SWEEP_N, C)
        k = int(kink_rows(sweep_params(C), f).sum())
        assert k <= max(2, SWEEP_N // 100), (C, k)
    for C in TICKET_CLASSES:
        p = sweep_params(C)
        for n in TICKET_SIZES + (FWD_STRIDE_N,):
            k = int(kink_rows(p, sweep_inputs(C, n, 1000 + n)[0]).sum())
            assert k <= max(2, n // 100), (C, n, k)
    assert [min(256, (n + 255) // 256) for n in TICKET_SIZES] == [1, 1, 1, 1, 1, 2, 16, 17, 256, 256, 256, 256]


def test_value_cases_hold_their_conditions():
    for C in (2, 7, 32):
        f, _ = sweep_inputs(C)
        h, z = fp64_logits(value_case("ties", C), f)
        for i, j in tie_pairs(C):
            assert torch.equal(z[:, i], z[:, j])
            assert int((z.argmax(dim=1) == min(i, j)).sum()) > 0, (C, i, j)  # (the pair is the argmax on some rows)
        h, z = fp64_logits(value_case("large", C), f)
        assert float(z.abs().max()) > 200.0, (C, float(z.abs().max()))
        if C > 1:
            assert float((z.max(dim=1).values - z.min(dim=1).values).max()) > 88.0  # exp() of a raw difference underflows
        h, z = fp64_logits(value_case("dead", C), f)
        assert float(h.max()) == 0.0, C
        assert int(kink_rows(value_case("ties", C), f).sum()) <= max(2, SWEEP_N // 100)
        assert not bool(kink_rows(sweep_params(C), torch.zeros(1, 8)).any()), C  # (zero features are off the kinks too)


def test_fixture_is_consistent_with_the_composite():
    torch.set_num_threads(1)
    fx = load_fixture()
    assert fx["classes"] == 21 and [c["name"] for c in fx["cases"]] == ["std", "large", "kinks", "ties"]
    for case in fx["cases"]:
        dec = decoder_from_case(case)
        logp = dec._sem_composite(case["feat"])
        ok, worst = ulp_close(logp, case["logp"], 64)
        assert ok, (case["name"], worst)
        assert torch.equal(torch.argmax(case["logp"], dim=1), case["sem_label"])
        assert torch.equal(dec.sem_label(case["feat"]), case["sem_label"]), case["name"]  # (CPU: the composite path)
        for d, rec in case["by_decimation"].items():
            f = case["feat"].clone().requires_grad_(True)
            dec.zero_grad(set_to_none=True)
            loss = torch.nn.NLLLoss()(dec._sem_composite(f)[::d], case["label"][::d])
            loss.backward()
            assert abs(float(loss) - float(rec["loss"])) <= 1e-5 * max(1.0, abs(float(rec["loss"])))
            scale = float(rec["grad_feat"].abs().max())
            assert float((f.grad - rec["grad_feat"]).abs().max()) <= 1e-5 * scale, (case["name"], d)
            assert rec["grads"]["lout.weight"] is None and rec["grads"]["lout.bias"] is None
            for k, p in dec.named_parameters():
                if k.startswith("lout"):
                    assert p.grad is None
                    continue
                ref = rec["grads"][k]
                assert float((p.grad - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1e-12), (case["name"], d, k)


def test_fixture_covers_the_edge_cases():
    fx = {c["name"]: c for c in load_fixture()["cases"]}
    assert float(fx["large"]["logp"].min()) < -88.0  # exp() of the raw logits would overflow without the max subtraction
    top = fx["ties"]["logp"].topk(2, dim=1).values
    assert int((top[:, 0] == top[:, 1]).sum()) > 0 and (fx["ties"]["sem_label"] == 3).any()
    p = fx["kinks"]["params"]
    h1 = fx["kinks"]["feat"] @ p["layers.0.weight"].T + p["layers.0.bias"]
    assert int((h1 == 0).sum()) > 0
    for c in fx.values():
        assert (c["label"] == 0).any() and (c["label"] == 20).any()


def test_fixture_regenerates_bit_identically_from_the_live_reference():
    if not os.path.isfile("/root/reference/model/decoder.py") and not os.environ.get("SHINE_REFERENCE_ROOT"):
        return  # (the recipe needs the reference checkout; the stored values are what the other tests use)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_semantic_golden.py"), "--check"], capture_output=True,
                       text=True, cwd=ROOT)
    assert r.returncode == 0 and "identical" in r.stdout, r.stdout + r.stderr


def test_header_declares_and_the_library_binds_the_semantic_entry_points():
    from shine_mapping_amd import _lib

    text = open(os.path.join(ROOT, "include", "shine_hip.h")).read()
    for sym in ("shine_sem_forward", "shine_sem_backward", "shine_sem_query_labels"):
        assert sym + "(" in text
        assert sym in _lib.exported_symbols()
        assert getattr(_lib.lib(), sym) is not None
    assert "#define SHINE_SEM_MAX_CLASSES 32" in text and "#define SHINE_SEM_WORKSPACE_BYTES 2621440" in text


def test_semantic_argument_checks_do_not_need_a_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    P = ctypes.c_void_p
    fake = [P(0x1000 * (k + 1)) for k in range(6)]
    mlp = _lib.ptr_array([p.value for p in fake])
    lab = P(0x9000)
    # null feature / outputs / decoder, class count out of range
    assert lib.shine_sem_forward(None, 10, mlp, 21, None, lab, None) == -1
    assert lib.shine_sem_forward(P(0x8000), 10, mlp, 21, None, None, None) == -1
    assert lib.shine_sem_forward(P(0x8000), 10, None, 21, None, lab, None) == -1
    assert lib.shine_sem_forward(P(0x8000), 10, mlp, 0, None, lab, None) == -1
    assert lib.shine_sem_forward(P(0x8000), 10, mlp, 33, None, lab, None) == -1
    assert lib.shine_sem_forward(P(0x8000), 10, _lib.ptr_array([None] + [p.value for p in fake[1:]]), 21, None, lab, None) == -1
    assert lib.shine_sem_forward(P(0x8000), 0, mlp, 21, None, lab, None) == 0  # (empty: nothing to launch)
    # backward: null inputs, weight grads without a workspace / with a misaligned one
    assert lib.shine_sem_backward(None, P(0x8000), P(0x8000), 10, mlp, 21, P(0x8000), None, None, None) == -1
    assert lib.shine_sem_backward(P(0x8000), None, P(0x8000), 10, mlp, 21, P(0x8000), None, None, None) == -1
    assert lib.shine_sem_backward(P(0x8000), P(0x8000), None, 10, mlp, 21, P(0x8000), None, None, None) == -1
    assert lib.shine_sem_backward(P(0x8000), P(0x8000), P(0x8000), 10, mlp, 21, None, mlp, None, None) == -1
    assert lib.shine_sem_backward(P(0x8000), P(0x8000), P(0x8000), 10, mlp, 21, None, mlp, P(0x8004), None) == -1
    assert lib.shine_sem_backward(P(0x8000), P(0x8000), P(0x8000), 10, mlp, 40, P(0x8000), None, None, None) == -1
    # label query: null tables / coord / output
    cfg = _lib.StepConfig()
    rows = (ctypes.c_int64 * 1)(10)
    feats = _lib.ptr_array([0x8000])
    assert lib.shine_sem_query_labels(None, ctypes.byref(cfg), P(0x8000), 10, feats, rows, mlp, 21, lab, None) == -1
    assert lib.shine_sem_query_labels(None, ctypes.byref(cfg), None, 10, feats, rows, mlp, 21, lab, None) == -1
    assert lib.shine_sem_query_labels(None, ctypes.byref(cfg), P(0x8000), 10, feats, rows, mlp, 21, None, None) == -1
    assert b"shine_sem" in lib.shine_error_string(-1)


def _params(shapes, device="cpu"):
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(device)) for s in shapes]


GEO = [(32, 8), (32,), (32, 32), (32,), (1, 32), (1,), (21, 32), (21,)]  # Decoder.parameters(): layers, lout, nclass_out


def _sem_cfg(**over):
    base = dict(lr=0.01, weight_decay=1e-7, tree_level_feat=3, lr_level_reduce_ratio=0.5, adam_eps=1e-15, opt_adam=True,
                semantic_on=True, ray_loss=False)
    base.update(over)
    return SimpleNamespace(**base)


def test_setup_optimizer_builds_the_reference_groups_with_the_semantic_head():
    from shine_mapping_amd.optim import FusedAdam, setup_optimizer

    geo, sem = _params(GEO), _params(GEO)
    feats = _params([(101, 8), (203, 8), (307, 8)])
    cfg = _sem_cfg()
    opt = setup_optimizer(cfg, feats, geo, sem, None)
    assert isinstance(opt, FusedAdam)
    gs = opt.param_groups
    assert len(gs) == 2 + 3
    assert gs[0]["params"] == geo and gs[0]["lr"] == 0.01 and gs[0]["weight_decay"] == 1e-7
    assert gs[1]["params"] == sem and gs[1]["lr"] == 0.01 and gs[1]["weight_decay"] == 1e-7
    assert [g["params"][0] is f for g, f in zip(gs[2:], feats[::-1])] == [True] * 3
    assert [g["lr"] for g in gs[2:]] == [0.01, 0.005, 0.0025] and all(g["weight_decay"] == 0.0 for g in gs[2:])
    # without the semantic head the group is not there, as in the reference (:64: `config.semantic_on and ...`)
    assert len(setup_optimizer(_sem_cfg(semantic_on=False), feats, geo, sem, None).param_groups) == 4
    assert len(setup_optimizer(cfg, feats, geo, None, None).param_groups) == 4
    with pytest.raises(NotImplementedError):
        setup_optimizer(_sem_cfg(opt_adam=False), feats, geo, sem, None)
    with pytest.raises(NotImplementedError):
        setup_optimizer(_sem_cfg(ray_loss=True), feats, geo, sem, torch.nn.Parameter(torch.ones(1)))


def test_fused_adam_skips_parameters_without_grad_in_the_state_dict():
    """lout of the semantic decoder never receives a grad: like torch.optim.Adam no state for it (the state_dict layout)"""
    from shine_mapping_amd.optim import setup_optimizer

    geo, sem = _params(GEO), _params(GEO)
    feats = _params([(11, 8), (13, 8), (17, 8)])
    opt = setup_optimizer(_sem_cfg(), feats, geo, sem, None)
    sd = opt.state_dict()
    assert sd["state"] == {} and [len(g["params"]) for g in sd["param_groups"]] == [8, 8, 1, 1, 1]
    ref = torch.optim.Adam([{"params": g["params"], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in opt.param_groups],
                           betas=(0.9, 0.99), eps=1e-15)
    ref.load_state_dict(sd)


def test_dropin_keeps_the_fused_optimizer_with_the_semantic_head(tmp_path):
    """the re-bound utils.tools.setup_optimizer returns the fused Adam with semantic_on (CUDA tensors), and still hands SGD and
    semantic_on + ray_loss to the reference's own function"""
    pkg = tmp_path / "utils"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "tools.py").write_text(
        "def setup_optimizer(config, octree_feat, mlp_geo_param, mlp_sem_param, sigma_size):\n    return 'reference'\n"
        "def get_gradient(inputs, outputs):\n    return 'reference'\n")
    (pkg / "loss.py").write_text("def sdf_bce_loss(*a, **k):\n    return 'reference'\n")
    code = (
        "import sys, types, torch\n"
        "sys.path.insert(0, %r)\n"
        "sys.path.insert(0, %r)\n"
        "import shine_mapping_amd.dropin as d\n"
        "import utils.tools as ut\n"
        "from shine_mapping_amd.optim import FusedAdam\n"
        "mk = lambda *s: torch.nn.Parameter(torch.zeros(*s))\n"
        "geo = [mk(32, 8), mk(32), mk(32, 32), mk(32), mk(1, 32), mk(1), mk(21, 32), mk(21)]\n"
        "sem = [mk(32, 8), mk(32), mk(32, 32), mk(32), mk(1, 32), mk(1), mk(21, 32), mk(21)]\n"
        "feats = [mk(5, 8), mk(6, 8)]\n"
        "cfg = types.SimpleNamespace(lr=0.01, weight_decay=0.0, tree_level_feat=2, lr_level_reduce_ratio=1.0, adam_eps=1e-15,\n"
        "                            opt_adam=True, semantic_on=True, ray_loss=False)\n"
        "import shine_mapping_amd.dropin as dd\n"
        "orig_is_cuda = torch.Tensor.is_cuda\n"
        "torch.Tensor.is_cuda = property(lambda self: True)  # (the check is all that looks at the device here)\n"
        "try:\n"
        "    opt = ut.setup_optimizer(cfg, feats, geo, sem, None)\n"
        "    cfg.ray_loss = True\n"
        "    other = ut.setup_optimizer(cfg, feats, geo, sem, mk(1))\n"
        "    cfg.ray_loss, cfg.opt_adam = False, False\n"
        "    sgd = ut.setup_optimizer(cfg, feats, geo, sem, None)\n"
        "finally:\n"
        "    torch.Tensor.is_cuda = orig_is_cuda\n"
        "assert isinstance(opt, FusedAdam) and len(opt.param_groups) == 4 and opt.param_groups[1]['params'] == sem\n"
        "assert other == 'reference' and sgd == 'reference', (other, sgd)\n"
        "st = d.status()\n"
        "assert st['setup_optimizer'] is True and 'HIP' in st['sem_label_prob'], st\n"
        "print('ok')\n" % (str(tmp_path), ROOT)
    )
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_synthetic_semantic_labels_follow_the_sampler_convention():
    from shine_mapping_amd import synth

    g = torch.Generator().manual_seed(5)
    coord = torch.rand(4000, 3, generator=g) * 2 - 1
    weight = torch.where(torch.rand(4000, generator=g) < 0.5, torch.ones(4000), -torch.ones(4000))
    lab = synth.semantic_labels(coord, weight, 21)
    assert lab.dtype == torch.int64 and bool((lab[weight <= 0] == 0).all())
    assert bool(((lab[weight > 0] >= 1) & (lab[weight > 0] <= 20)).all()) and int(lab[weight > 0].unique().numel()) == 20
    assert torch.equal(lab, synth.semantic_labels(coord.clone(), weight, 21))
