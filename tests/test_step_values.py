"""CPU: the value cases of the SDF step (tests/step_value_cases.py) are what they say — on the fp32 oracle and on the wide one —
and the checkers the GPU tests hold the kernels to (tests/test_gpu_step_values.py) reject wrong results: a checker that accepts
everything fails here, without a GPU."""
import pytest
import torch

import step_value_cases as sv

EIK_FIXTURES = [n for n in sv.FIXTURES if sv.is_eikonal(sv.fixture(n))]
BOTH = ("fp32", "wide")


def _outs(name, kind):
    case, ref, wide, _ = sv.oracles(name, kind)
    return case, dict(fp32=ref, wide=wide)


def _tensors(out):
    yield "loss", out["loss"]
    yield "pred", out["pred"]
    if out["g"] is not None:
        yield "g", out["g"]
    for k, t in enumerate(out["feat_grads"]):
        yield "feature grad %d" % k, t
    for k, t in enumerate(out["mlp_grads"]):
        yield "decoder grad %d" % k, t


@pytest.mark.parametrize("kind", sv.KINDS)
@pytest.mark.parametrize("name", sv.FIXTURES)
def test_every_case_is_finite_on_both_oracles(name, kind):
    case, outs = _outs(name, kind)
    for which in BOTH:
        for what, t in _tensors(outs[which]):
            assert bool(torch.isfinite(t).all()), (which, what)
    assert (outs["fp32"]["g"] is not None) == sv.is_eikonal(sv.fixture(name))


@pytest.mark.parametrize("name", sv.FIXTURES)
def test_dead_map_has_no_gradient_but_b3s(name):
    """b2 = -1000: g and every gradient but d b3 exactly zero, pred == b3, the eikonal term exactly 1"""
    case, outs = _outs(name, "dead")
    for which in BOTH:
        out = outs[which]
        b3 = case.decoder["lout.bias"].reshape(()).to(out["pred"].dtype)
        assert bool((out["pred"] == b3).all()), which
        if out["g"] is not None:
            assert float(out["g"].abs().max()) == 0.0, which
            assert float(out["parts"]["eikonal"]) == 1.0, which
        for t in out["feat_grads"] + out["mlp_grads"][:5]:
            assert float(t.abs().max()) == 0.0, which
        assert float(out["mlp_grads"][5].abs().max()) > 0.0, which


@pytest.mark.parametrize("name", EIK_FIXTURES)
def test_dead_points_mix_zero_and_live_gradients_among_the_surface_points(name):
    """the eikonal term's guard (gn > 0.f ? ... : 0.f) needs surface points with g == 0 and, in the same batch, live ones"""
    case, outs = _outs(name, "dead_points")
    surface = case.weight > 0
    for which in BOTH:
        g = outs[which]["g"]
        zero = (g == 0).all(1)
        assert bool(zero[case.zero_points].all()), which
        assert int((zero & surface).sum()) >= 16 and int((~zero & surface).sum()) >= 16, \
            (which, int((zero & surface).sum()), int((~zero & surface).sum()))


@pytest.mark.parametrize("name", sv.FIXTURES)
def test_on_kink_points_sit_exactly_on_the_kink(name):
    """b1 = b2 = 0 over zero features: every pre-activation exactly 0, so pred == b3 and (relu'(0) = 0) g == 0"""
    case, outs = _outs(name, "on_kink")
    zp = case.zero_points
    assert int(zp.sum()) == zp.numel() // 4
    for which in BOTH:
        out = outs[which]
        assert float(out["feat"][zp].abs().max()) == 0.0, which
        assert bool((out["pred"][zp] == case.decoder["lout.bias"].reshape(()).to(out["pred"].dtype)).all()), which
        if out["g"] is not None:
            assert float(out["g"][zp].abs().max()) == 0.0, which
        assert float(out["feat"][~zp].abs().max()) > 0.0, which


@pytest.mark.parametrize("kind", ["saturated", "saturated_weighted"])
@pytest.mark.parametrize("name", sv.FIXTURES)
def test_saturated_maps_reach_past_17_and_stay_below_the_exp2_range_limit(name, kind):
    case, outs = _outs(name, kind)
    for which in BOTH:
        y = outs[which]["pred"].abs()
        assert 60.0 <= float(y.max()) <= 100.0, (which, float(y.max()))
        assert int((y > 17.0).sum()) >= 32, (which, int((y > 17.0).sum()))
    if kind == "saturated_weighted":
        w = case.weight
        assert case.loss_weight_on and int((w == 0).sum()) >= w.numel() // 10 and float(w.abs().max()) == 50.0
        assert torch.equal((w > 0) | (w == 0), (sv.fixture(name)["weight"] > 0) | (w == 0))  # the sign stays


# ------------------------------------------------------------------------------------ the checkers reject what they should


def _checked(name, kind, corrupt=None):
    case, ref, wide, mlp64 = sv.oracles(name, kind)
    run = sv.run_of(ref)
    if corrupt is not None:
        corrupt(run)
    sv.check_run("oracle", case, ref, wide, mlp64, run)


@pytest.mark.parametrize("kind", sv.KINDS)
@pytest.mark.parametrize("name", sv.FIXTURES)
def test_checker_accepts_the_oracles_own_output(name, kind):
    _checked(name, kind)


def test_checker_rejects_a_nan_in_one_decoder_gradient():
    """(max() over a list that holds a NaN returns whatever stood first: the relative-error policy alone lets this one through)"""
    def corrupt(run):
        run["mlp_grads"][2][7, 3] = float("nan")

    with pytest.raises(AssertionError, match="not finite"):
        _checked("kitti_eik_L3", "dead_points", corrupt)


def test_checker_rejects_a_tiny_entry_in_a_dead_feature_gradient():
    def corrupt(run):
        run["feat_grads"][1][5, 2] = 1e-9

    with pytest.raises(AssertionError, match="feature grad level 1 != 0"):
        _checked("kitti_eik_L3", "dead", corrupt)


def test_checker_rejects_pred_one_ulp_off_on_a_dead_point():
    def corrupt(run):
        p = run["pred"]
        p[100] = torch.nextafter(p[100], torch.tensor(float("inf")))

    with pytest.raises(AssertionError, match="pred != b3"):
        _checked("maicity_bce_L4", "dead", corrupt)


def _fp32_sweep(sigma, clamp=None, w=1.0):
    """the per-point sweep on torch's fp32 expression of the head (utils/loss.py:17-24): (y, d b3, loss, label)"""
    y64, x64 = sv.sweep_grid()
    y = y64.float()
    label = (x64 * sigma).float()
    z = torch.sigmoid(label / torch.tensor(sigma, dtype=torch.float32))
    ys = y if clamp is None else y.clamp_max(clamp)
    db3 = abs(w) * (torch.sigmoid(ys) - z)
    loss = abs(w) * torch.nn.functional.binary_cross_entropy_with_logits(y, z, reduction="none")
    return y, db3, loss, label


@pytest.mark.parametrize("w", [1.0, -3.0])
def test_delta_checker_accepts_the_fp32_expression(w):
    sigma = sv.fixture("maicity_bce_L4")["sigma"]
    y, db3, loss, label = _fp32_sweep(sigma, w=w)
    worst = sv.check_delta("torch fp32", y, db3, loss, label, sigma, w)
    assert max(worst) <= 0.5  # (the reference's own expression: 2.72 of the bound's 8 x 2^-24)


def test_delta_checker_rejects_a_sigmoid_that_saturates_early():
    """A delta from sigmoid(min(y, 14)): 1 - sigmoid(14) = 13.9 x 2^-24, past the bound's 8 x 2^-24.
    (A clamp at 17 cannot be told from the correct head by ANY fp32 bound: 1 - sigmoid(17) = 0.69 x 2^-24 is less than the spacing of
    fp32 below 1, and the kernel's own expression — like torch's — returns exactly 1.0 from y = 16.64 up, where 1 + e rounds to
    1.  test_a_clamp_at_17_is_below_fp32_resolution pins that arithmetic.)"""
    sigma = sv.fixture("maicity_bce_L4")["sigma"]
    y, db3, loss, label = _fp32_sweep(sigma, clamp=14.0)
    with pytest.raises(AssertionError, match="d b3 is"):
        sv.check_delta("clamped", y, db3, loss, label, sigma)
    y, db3, loss, label = _fp32_sweep(sigma)
    nan = db3.clone()
    nan[3] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        sv.check_delta("nan", y, nan, loss, label, sigma)
    off = loss.clone()
    off[-5] *= 1.0 + 2e-6  # y = 120 against a target of 0: 16 ulp of a loss of 120
    with pytest.raises(AssertionError, match="loss is"):
        sv.check_delta("loss", y, db3, off, label, sigma)


def test_a_clamp_at_17_is_below_fp32_resolution():
    y = torch.tensor([17.0, 30.0, 120.0], dtype=torch.float64)
    assert float((torch.sigmoid(y) - torch.sigmoid(y.clamp_max(17.0))).abs().max()) < 0.7 * sv.U24
    assert bool((torch.sigmoid(y.float()) >= 1.0 - 2.0 ** -24).all())  # fp32: 1.0 or its neighbour below
