"""CPU suite: the references, pins and checkers of tests/tier_a_kernel_cases.py (the GPU runs are tests/test_gpu_tier_a_kernels.py).

(1) the references are right: the closed forms equal torch.autograd over the oracle in fp64, the restated corner weights equal the
oracle's bit for bit, and the same code in fp32 reproduces what the fixtures recorded from the reference;
(2) the pins are honest: on every case the fp32 oracle's ratio is at most K / 4 in its family;
(3) no point near a ReLU kink survives the redraw in any decoder case;
(4) the checkers reject what they are for — each mutation of the fp32 oracle's results fails its checker, and REL_ERR_PASSES
records which of them the suite's `rel_err <= TOL` would have let through.
"""
import pytest
import torch

import step_value_cases as svc
import tier_a_kernel_cases as tc
from test_gpu_parity import TOL, rel_err


@pytest.fixture
def one_thread():
    """the pins were measured with one thread: torch's GEMM blocks its sums by thread count"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _within(a, b, scale, tol, what):
    worst = float(((a.reshape(b.shape) - b).abs() - tol * scale.reshape(b.shape)).max())
    assert worst <= 0.0, "%s: closed form and autograd differ by more than %g of the element's scale" % (what, tol)


# ------------------------------------------------------------------------------------------------ (1) the references are right


def test_closed_forms_equal_autograd_over_the_oracle_in_fp64():
    case, ref, scale = tc.mlp_reference("on_kink", 257)
    closed = tc.mlp_closed(case, False)
    for k in tc.MLP_POINT:
        _within(closed[k], ref[k], scale[k], 1e-12, "decoder " + k)
    for k in ("gw", "bb"):
        for i in range(6):
            _within(closed[k][i], ref[k][i], scale[k][i], 1e-12, "decoder %s[%d]" % (k, i))
    assert all(float(ref["bb"][i].abs().max()) == 0.0 for i in (1, 3, 5))  # autograd sends nothing to the biases either
    case, ref, scale = tc.interp_reference("edges_L3", "whole")
    closed = tc.interp_closed(case, False)
    for k in ("grad_coord", "dg"):
        _within(closed[k], ref[k], scale[k], 1e-12, "interp " + k)
    for k in ("rows1", "rows2"):
        for i, (a, b, s) in enumerate(zip(closed[k], ref[k], scale[k])):
            _within(a, b, s, 1e-12, "interp %s[%d]" % (k, i))


@pytest.mark.parametrize("name", tc.INTERP_FIXTURES)
def test_restated_weights_and_feature_sum_equal_the_oracles_bit_for_bit(name):
    case = tc.interp_batch(name, "whole")
    for wide in (False, True):
        oct_ = tc._oracle_pair(name, wide)
        for i, (fl, ids, d, _) in enumerate(tc._levels(oct_, case.coord)):
            assert torch.equal(tc.corner_weights(d, oct_.poly).unsqueeze(2), oct_.interp_weights(case.coord, oct_.max_level - i))
        with torch.no_grad():
            want = oct_.query_feature_with_indices(case.coord, oct_.get_indices(case.coord))
        assert torch.equal(tc.interp_autograd(case, wide)["feat"], want)


@pytest.mark.parametrize("name", tc.INTERP_FIXTURES)
def test_fp32_mode_reproduces_what_the_fixture_recorded(name, one_thread):
    """feat; g = sigma d pred / d coord where the fixture has it (the first pass fed with d pred / d feat of the oracle decoder);
    feat_grads where the loss has no eikonal term (the first pass fed with d loss / d feat).  Tolerances: tests/test_oracle.py's."""
    from conftest import oracle_from_golden
    from oracle import shine_oracle as so

    fx = svc.fixture(name)
    out = fx["out"]
    case = tc.interp_batch(name, "whole")
    feat = tc.interp_autograd(case, wide=False)["feat"]
    assert float((feat - out["feat"]).abs().max()) <= 2e-6 * float(out["feat"].abs().max())
    ocfg, _, mlp = oracle_from_golden(fx)
    f = feat.clone().requires_grad_(True)
    pred = mlp.sdf(f)
    if out["g"] is not None:
        (up,) = torch.autograd.grad(pred, f, torch.ones_like(pred))
        g = tc.interp_autograd(case, wide=False, g=up)["grad_coord"] * fx["sigma"]
        assert float((g - out["g"]).abs().max()) <= 2e-6 * float(out["g"].abs().max())
    else:
        loss = so.sdf_bce_loss(pred, fx["sdf_label"], so.sigma_sigmoid(ocfg), ocfg.loss_reduction)
        (up,) = torch.autograd.grad(loss, f)
        rows = tc.interp_autograd(case, wide=False, g=up)["rows1"]
        for k, (a, b) in enumerate(zip(rows, out["feat_grads"])):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), "feat_grads[%d]" % k


# --------------------------------------------------------------------------------------------- (2) the pins, (3) the kink rule


def test_pins_follow_the_rule():
    assert tc.K == {fam: 4.0 * max(rho, 1.0) for fam, rho in tc.RHO_REF.items()}


@pytest.mark.parametrize("decoder", tc.DECODERS)
def test_decoder_pins_are_honest_and_no_point_sits_near_a_kink(decoder, one_thread):
    for n in tc.mlp_sizes(decoder, False):
        case, ref, scale = tc.mlp_reference(decoder, n)
        assert int(tc.near_kink(case.params, case.feat).sum()) == 0
        assert case.redrawn <= max(5, n // 25), "the kink rule redrew %d of %d points" % (case.redrawn, n)
        got = tc.mlp_autograd(case, torch.float32)
        if n not in tc.mlp_sizes(decoder, True):
            got["gw"] = got["bb"] = None
        rho = tc.check_mlp("fp32 oracle, %s n=%d" % (decoder, n), got, ref, scale)
        for fam, v in rho.items():
            assert v <= tc.K[fam] / 4.0, "%s n=%d: the fp32 oracle's ratio %.3f exceeds K / 4 of %s" % (decoder, n, v, fam)
    if decoder == "b1_third":  # the case is what it says: some weight-grad rows have scale zero, others do not
        dead = scale["gw"][0].abs().sum(1) == 0
        assert bool(dead[::3].all()) and not bool(dead.all())
    if decoder in ("on_kink", "dead_points"):
        assert bool(case.zero_points.any()) and float(ref["grad_feat"][case.zero_points].abs().max()) == 0.0


@pytest.mark.parametrize("name", tc.INTERP_FIXTURES)
def test_interpolation_pins_are_honest(name, one_thread):
    for batch in tc.BATCHES:
        case, ref, scale = tc.interp_reference(name, batch)
        suffix = "_repeat" if batch == "repeat" else ""
        rho = tc.check_interp("fp32 oracle, %s %s" % (name, batch), tc.interp_oracle32(name, batch), ref, scale, suffix=suffix)
        for fam, v in rho.items():
            assert v <= tc.K[fam] / 4.0, "%s %s: the fp32 oracle's ratio %.3f exceeds K / 4 of %s" % (name, batch, v, fam)
        trash = float(sum(s[-1].sum() for s in scale["rows1"]))
        if batch in ("misses", "alternate"):
            assert trash > 0.0
        if batch == "misses":  # nothing but the trash rows is touched
            assert all(float(s[:-1].abs().max()) == 0.0 for s in scale["rows1"] + scale["rows2"])
        if batch == "one_leaf":
            assert trash == 0.0 and all(int((s[:-1].sum(1) > 0).sum()) == 8 for s in scale["rows1"])
    assert case.n == 4096 * 256 + 1


# ----------------------------------------------------------------------------------------- (4) the checkers reject wrong results

# which mutations the suite's metric — rel_err(tensor, reference) <= TOL, a maximum over the tensor divided by the tensor's largest
# entry — would have passed (True) while the per-element checker rejects every one of them
REL_ERR_PASSES = {
    "rows: last point missing": True,
    "weights: last point missing": False,
    "one corner of one point dropped": True,
    "two features of one row swapped": True,
    "single small-g row zeroed": True,
    "relu'(0) = 1 at the exact kinks": False,
    "one wave's partial missing": False,
    "a bias moved by the double backward": False,
    "trash row given sum |coef|": False,
    "dW2 transposed": False,
}


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def _sub(case, sl):
    from types import SimpleNamespace

    return SimpleNamespace(**{**vars(case), "feat": case.feat[sl], "g": case.g[sl], "r": case.r[sl],
                              "n": case.feat[sl].shape[0]})


def _verdict(name, passes):
    assert name in REL_ERR_PASSES
    assert REL_ERR_PASSES[name] == passes, \
        "%s: rel_err <= TOL %s it, REL_ERR_PASSES says otherwise" % (name, "passes" if passes else "rejects")


MUT_INTERP = ("edges_L3", "prefix257")
MUT_MLP = ("b1_third", 257)  # its last point carries 4 % of sum |g| (the fixture decoder's case: 2e-9, below any rounding)


@pytest.fixture(scope="module")
def interp32():
    case, ref, scale = tc.interp_reference(*MUT_INTERP)
    got = tc.interp_oracle32(*MUT_INTERP)
    tc.check_interp("unmutated", got, ref, scale)
    return case, ref, scale, got


@pytest.fixture(scope="module")
def mlp32():
    case, ref, scale = tc.mlp_reference(*MUT_MLP)
    got = tc.mlp_autograd(case, torch.float32)
    tc.check_mlp("unmutated", got, ref, scale)
    return case, ref, scale, got


def _rows_rel_ok(rows, ref):
    return all(rel_err(a, b) <= TOL for a, b in zip(rows, ref))


def test_rows_without_the_last_point_are_rejected(interp32):
    case, ref, scale, got = interp32
    last = tc.interp_autograd(case, wide=False, coord=case.coord[-1:], g=case.g[-1:], gg=case.gg[-1:])
    for key in ("rows1", "rows2"):
        bad = [a - b for a, b in zip(got[key], last[key])]
        _rejected(lambda: tc.check_rows(key, bad, ref[key], scale[key]))
    _verdict("rows: last point missing", _rows_rel_ok([a - b for a, b in zip(got["rows1"], last["rows1"])], ref["rows1"]))


def test_weight_sums_without_the_last_point_or_one_wave_are_rejected(mlp32):
    case, ref, scale, got = mlp32
    assert abs(float(case.g[-1])) >= 0.01 * float(case.g.abs().sum())
    for name, sl in (("weights: last point missing", slice(case.n - 1, case.n)), ("one wave's partial missing", slice(64, 128))):
        part = tc.mlp_autograd(_sub(case, sl), torch.float32)
        ok = True
        for key in ("gw", "bb"):
            bad = [a - b for a, b in zip(got[key], part[key])]
            _rejected(lambda: tc.check_mlp(name, {key: bad}, ref, scale))
            ok = ok and all(rel_err(a, b) <= TOL for a, b in zip(bad, ref[key]) if float(b.abs().max()) > 0)
        _verdict(name, ok)


def _first_hit(case, oct_):
    """(level entry, point) of the first point that hits at the finest level with a g that is not zero"""
    fl, ids, d, dudx = tc._levels(oct_, case.coord)[0]
    p = int(torch.nonzero((ids >= 0).all(1) & (case.g.abs().sum(1) > 0))[0])
    return fl, ids, d, p


def test_a_dropped_corner_and_swapped_features_are_rejected(interp32):
    case, ref, scale, got = interp32
    oct_ = tc._oracle_pair(case.name, False)
    fl, ids, d, p = _first_hit(case, oct_)
    w = tc.corner_weights(d, oct_.poly)[p]
    c = int(w.argmax())
    bad = [t.clone() for t in got["rows1"]]
    bad[fl][ids[p, c]] -= w[c] * case.g[p]
    _rejected(lambda: tc.check_rows("corner", bad, ref["rows1"], scale["rows1"]))
    _verdict("one corner of one point dropped", _rows_rel_ok(bad, ref["rows1"]))
    bad = [t.clone() for t in got["rows1"]]
    row = bad[fl][ids[p, c]].clone()
    bad[fl][ids[p, c], 0], bad[fl][ids[p, c], 1] = row[1], row[0]
    _rejected(lambda: tc.check_rows("swap", bad, ref["rows1"], scale["rows1"]))
    _verdict("two features of one row swapped", _rows_rel_ok(bad, ref["rows1"]))


def test_a_zeroed_row_of_one_small_g_point_is_rejected(interp32):
    case, ref, scale, got = interp32
    oct_ = tc._oracle_pair(case.name, False)
    fl, ids, d, _ = tc._levels(oct_, case.coord)[0]
    count = torch.bincount(ids[ids >= 0].flatten(), minlength=got["rows1"][fl].shape[0])
    size = case.g.abs().sum(1)
    best = None
    for p in torch.nonzero((ids >= 0).all(1) & (size > 0)).flatten().tolist():
        for c in range(8):
            if int(count[ids[p, c]]) == 1 and (best is None or float(size[p]) < best[0]):
                best = (float(size[p]), int(ids[p, c]))
    assert best is not None and best[0] < 1e-3 * float(size.max()), "no row that a single small-g point touches"
    bad = [t.clone() for t in got["rows1"]]
    bad[fl][best[1]] = 0.0
    _rejected(lambda: tc.check_rows("zeroed", bad, ref["rows1"], scale["rows1"]))
    _verdict("single small-g row zeroed", _rows_rel_ok(bad, ref["rows1"]))


def test_the_trash_row_with_absolute_coefficients_is_rejected():
    case, ref, scale = tc.interp_reference("edges_L3", "alternate")
    got = tc.interp_oracle32("edges_L3", "alternate")
    oct_ = tc._oracle_pair(case.name, False)
    bad = [t.clone() for t in got["rows2"]]
    for fl, ids, d, dudx in tc._levels(oct_, case.coord):
        miss = (ids < 0).all(1)
        coef = torch.einsum("pca,pa->pc", tc._weight_grads(d, oct_.poly, dudx), case.gg)
        bad[fl][-1] = (coef.abs().sum(1)[miss, None] * case.g[miss]).sum(0)
    _rejected(lambda: tc.check_rows("trash", bad, ref["rows2"], scale["rows2"]))
    _verdict("trash row given sum |coef|", _rows_rel_ok(bad, ref["rows2"]))


def test_relu_derivative_one_at_the_exact_kinks_is_rejected():
    case, ref, scale = tc.mlp_reference("on_kink", 257)
    P = [p.detach().float() for p in tc._wide_params(case.params)]
    z1 = case.feat @ P[0].T + P[1]
    m1 = (z1 >= 0).float()  # relu'(0) = 1
    m2 = ((torch.relu(z1)) @ P[2].T + P[3] >= 0).float()
    bad = tc._mlp_forms(P, case.feat, case.g, case.r, m1, m2)
    assert bool((z1[case.zero_points] == 0).all())
    tc.check("pred", "mlp_point", bad["pred"], ref["pred"], scale["pred"])  # the forward does not see the convention
    for k in ("grad_feat", "dg"):
        _rejected(lambda: tc.check(k, "mlp_point", bad[k], ref[k], scale[k]))
    _rejected(lambda: tc.check_mlp("gw", {"gw": bad["gw"]}, ref, scale))
    _verdict("relu'(0) = 1 at the exact kinks", rel_err(bad["grad_feat"], ref["grad_feat"]) <= TOL)


def test_a_moved_bias_and_a_transposed_dW2_are_rejected(mlp32):
    case, ref, scale, got = mlp32
    bad = [t.clone() for t in got["bb"]]
    bad[1][3] += 1e-6
    _rejected(lambda: tc.check_mlp("bias", {"bb": bad}, ref, scale))
    _verdict("a bias moved by the double backward", rel_err(bad[1], ref["bb"][1]) <= TOL)
    bad = [t.clone() for t in got["gw"]]
    bad[2] = bad[2].T.contiguous()
    _rejected(lambda: tc.check_mlp("dW2", {"gw": bad}, ref, scale))
    _verdict("dW2 transposed", rel_err(bad[2], ref["gw"][2]) <= TOL)


def test_prefilled_buffers_keep_untouched_elements_to_the_bit():
    """the accumulate form of the checker: v0 where the scale is zero must come back exactly, elsewhere the bound gains 2^-24 |v0|"""
    case, ref, scale = tc.interp_reference("edges_L3", "one_leaf")
    v0 = [tc.prefill(s, 7 + k) for k, s in enumerate(scale["rows1"])]
    good = [(v.double() + r).float() for v, r in zip(v0, ref["rows1"])]
    tc.check_rows("prefilled", good, ref["rows1"], scale["rows1"], v0=v0)
    untouched = int(torch.nonzero(scale["rows1"][0][:-1].sum(1) == 0)[0])
    good[0][untouched, 2] += 1e-7
    _rejected(lambda: tc.check_rows("prefilled", good, ref["rows1"], scale["rows1"], v0=v0))
