"""Value cases of the SDF step: maps as training leaves them, derived in memory from the step fixtures (no file of their own).

Every step fixture holds a map at its start: predictions of a few hundredths, every hidden unit alive somewhere, no two points
with the same pre-activation.  The cases below edit a fixture's features and decoder so that the step meets

  "dead"                b2 = -1000: no second-layer unit alive on any point (pred == b3, g == 0, only d b3 is not zero),
  "dead_points"         b1 = -|b1| - 0.05 and every feature row the first quarter of the batch addresses set to zero: those
                        points have g == 0 exactly — the zero-gradient guard of the eikonal term — next to live ones,
  "on_kink"             the same rows zeroed with b1 = b2 = 0: pre-activations exactly 0 (relu'(0) = 0 in torch, h > 0.f in the
                        kernels),
  "saturated"           w3 and b3 times one factor so that max |pred| is about 80: the BCE head past |y| = 16.6, where 1 + e
                        rounds to 1, and short of 87.3, where e leaves the normal range,
  "saturated_weighted"  the same with loss_weight_on and weights that hold exact zeros and values up to 50.

The same edit goes to the oracle (apply_to_oracle) and to the product (apply_to_product); tests/test_step_values.py checks on the
CPU that the cases are what they say, tests/test_gpu_step_values.py runs them through every form of the step.  The checkers the
GPU tests use (check_run, delta_ratios) are here so that the CPU tests can show that they reject wrong results.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from conftest import load_golden, oracle_from_golden

FIXTURES = ["kitti_eik_L3", "maicity_bce_L4", "edges_L2_nopoly_eik"]
KINDS = ["dead", "dead_points", "on_kink", "saturated", "saturated_weighted"]
NAMES = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias", "lout.weight", "lout.bias")
SATURATED_TARGET = 80.0  # max |pred| of the saturated cases (the issue's window: [60, 100])
U24 = 2.0 ** -24

# the per-point sweep: logits either side of every point where the BCE head's fp32 expression changes character
Y_TARGETS = (-120.0, -104.0, -89.0, -88.0, -87.0, -30.0, -17.0, -16.6, -1.0, 0.0, 1.0, 16.6, 17.0, 30.0, 87.0, 88.0, 89.0, 104.0,
             120.0)
LABEL_OVER_SIGMA = (-60.0, -3.0, 0.0, 3.0, 60.0)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_golden(name)


def is_eikonal(fx):
    return bool(fx["cfg"].get("ekional_loss_on", False))


def _zeroed_features(fx, points):
    """the fixture's features with every row zeroed that `points` (a slice of the batch) address on any level"""
    _, oct_, _ = oracle_from_golden(fx)
    idx = oct_.get_indices(fx["coord"][points])  # bottom-up
    L = len(idx)
    feats = [f.clone() for f in fx["features"]]  # top-down
    for i, t in enumerate(idx):
        rows = t.flatten()
        feats[L - 1 - i][rows[rows >= 0].unique()] = 0.0
    return feats


def value_case(fx, kind):
    """The edit of one case: features (top-down, as fx["features"]), decoder (a state dict), sdf_label, weight, loss_weight_on,
    zero_points (bool [n]: the points whose features are exactly zero, or None) and the saturated cases' factor."""
    n = fx["coord"].shape[0]
    dec = {k: fx["decoder"][k].clone().float() for k in NAMES}
    feats = [f.clone() for f in fx["features"]]
    label, weight = fx["sdf_label"].clone(), fx["weight"].clone()
    zero_points, factor, weighted = None, None, False
    if kind == "dead":
        dec["layers.1.bias"].fill_(-1000.0)
    elif kind in ("dead_points", "on_kink"):
        quarter = slice(0, n // 4)
        feats = _zeroed_features(fx, quarter)
        zero_points = torch.zeros(n, dtype=torch.bool)
        zero_points[quarter] = True
        if kind == "dead_points":
            dec["layers.0.bias"] = -dec["layers.0.bias"].abs() - 0.05
        else:
            dec["layers.0.bias"].zero_()
            dec["layers.1.bias"].zero_()
    elif kind in ("saturated", "saturated_weighted"):
        _, oct_, mlp = oracle_from_golden(fx)
        with torch.no_grad():
            base = mlp.sdf(oct_.query_feature(fx["coord"]))  # the fp32 oracle on the fixture as it is
        factor = float(np.float32(SATURATED_TARGET / float(base.abs().max())))
        dec["lout.weight"] *= factor
        dec["lout.bias"] *= factor
        if kind == "saturated_weighted":
            weighted = True
            g = torch.Generator().manual_seed(50)
            mag = 0.5 + 49.5 * torch.rand(n, generator=g)
            mag[1] = 50.0
            weight = torch.where(fx["weight"] > 0, mag, -mag)  # the sign stays: surface / free space
            weight[::10] = 0.0
    else:
        raise ValueError(kind)
    return SimpleNamespace(kind=kind, features=feats, decoder=dec, sdf_label=label, weight=weight, loss_weight_on=weighted,
                           zero_points=zero_points, factor=factor)


def apply_to_oracle(case, pair):
    """the edit on (ocfg, octree, decoder) of conftest.oracle_from_golden"""
    ocfg, oct_, mlp = pair
    oct_.hier_features = [f.clone().requires_grad_(True) for f in case.features]
    mlp.load_state_dict(case.decoder)
    ocfg.loss_weight_on = case.loss_weight_on
    return pair


def apply_to_product(case, pair):
    """the edit on (cfg, octree, decoder) of conftest.product_from_golden, in place: the kernels read these tensors where they are"""
    cfg, octree, dec = pair
    with torch.no_grad():
        for p, f in zip(octree.hier_features, case.features):
            p.copy_(f.to(p.device))
        for p, k in zip(dec.fused_params(), NAMES):
            p.copy_(case.decoder[k].to(p.device))
    cfg.loss_weight_on = case.loss_weight_on
    return pair


@functools.lru_cache(maxsize=None)
def oracles(name, kind):
    """(case, fp32 oracle's step, wide oracle's step, wide decoder) of one case: computed once, shared, never written to"""
    from oracle import shine_oracle as so

    fx = fixture(name)
    case = value_case(fx, kind)
    ocfg, oct_, mlp = apply_to_oracle(case, oracle_from_golden(fx))
    ref = so.train_step(oct_, mlp, fx["coord"], case.sdf_label, case.weight, ocfg)
    ocfg, oct64, mlp64 = apply_to_oracle(case, oracle_from_golden(fx))
    so.to_wide(oct64, mlp64)
    wide = so.train_step(oct64, mlp64, fx["coord"], case.sdf_label, case.weight, ocfg)
    return case, ref, wide, mlp64


def run_of(out):
    """an oracle's step in the shape check_run takes a device run in (copies: the tests corrupt them)"""
    return dict(loss=out["loss"].clone(), pred=out["pred"].clone(), g=None if out["g"] is None else out["g"].clone(),
                feat_grads=[t.clone() for t in out["feat_grads"]], mlp_grads=[t.clone() for t in out["mlp_grads"]],
                eikonal=out["parts"].get("eikonal"))


# --------------------------------------------------------------------------------------------------------------- the checkers


def _finite(what, t):
    assert t is None or bool(torch.isfinite(torch.as_tensor(t).detach()).all()), what + " is not finite"


def check_run(what, case, ref, wide, mlp64, run, order=None):
    """One run of a value case.  run: dict(loss, pred, g, feat_grads, mlp_grads, eikonal), None / [] for what the form does not
    return; `order`: the run's batch order relative to ref / wide (pool batches).
    (1) everything finite; (2) the case's exact claims; (3) the suite's standing policy (test_gpu_edges._check with TOL), pred
    held to TOL x max(1, max |reference pred|): at |y| = 80 one fp32 ulp is 7.6e-6."""
    from test_gpu_edges import _check

    pred, g = run.get("pred"), run.get("g")
    feat_grads, mlp_grads = run.get("feat_grads") or [], run.get("mlp_grads")
    for k, t in (("loss", run.get("loss")), ("pred", pred), ("g", g), ("eikonal", run.get("eikonal"))):
        _finite("%s: %s" % (what, k), t)
    for k, t in enumerate(feat_grads):
        _finite("%s: feature grad level %d" % (what, k), t)
    for k, t in enumerate(mlp_grads or []):
        _finite("%s: decoder grad %d" % (what, k), t)
    b3 = case.decoder["lout.bias"].reshape(())
    if case.kind == "dead":
        if pred is not None:
            assert bool((pred.detach().cpu() == b3).all()), what + ": pred != b3 on a dead map"
        if g is not None:
            assert float(g.detach().abs().max()) == 0.0, what + ": g != 0 on a dead map"
        for k, t in enumerate(feat_grads):
            assert float(t.detach().abs().max()) == 0.0, "%s: feature grad level %d != 0 on a dead map" % (what, k)
        for k, t in enumerate((mlp_grads or [])[:5]):
            assert float(t.detach().abs().max()) == 0.0, "%s: decoder grad %d != 0 on a dead map" % (what, k)
        if run.get("eikonal") is not None:
            assert float(run["eikonal"]) == 1.0, what + ": eikonal term of g == 0 everywhere is not 1"
    if case.kind == "on_kink":
        zp = case.zero_points if order is None else case.zero_points[order]
        if pred is not None:
            assert bool((pred.detach().cpu()[zp] == b3).all()), what + ": pred != b3 on a zero-feature point"
        if g is not None:
            assert float(g.detach().cpu()[zp].abs().max()) == 0.0, what + ": g != 0 on a zero-feature point"
    scale = max(1.0, float(ref["pred"].abs().max()))
    _check(what, ref, wide, run.get("loss"), pred, g if ref["g"] is not None else None, feat_grads, mlp_grads, mlp64,
           order=order, pred_scale=scale)


def delta_reference(y_dev, label, sigma, w):
    """fp64: (|w| delta, |w| loss) of one sample per entry — delta = sigmoid(y) - sigmoid(label / sigma), loss = max(y, 0) - y z +
    log1p(exp(-|y|)) — at the device's own fp32 prediction, with label and sigma as the fp32 values the kernel receives."""
    y = y_dev.detach().cpu().float().double()
    x = label.detach().cpu().float().double() / float(np.float32(sigma))
    z = torch.sigmoid(x)
    aw = torch.as_tensor(w, dtype=torch.float64).abs()
    return aw * (torch.sigmoid(y) - z), aw * (y.clamp_min(0.0) - y * z + torch.log1p(torch.exp(-y.abs()))), aw, y


def delta_ratios(y_dev, db3, loss, label, sigma, w=1.0):
    """(|db3 - |w| delta64| / (8 x 2^-24 |w|), |loss - |w| l64| / (8 x 2^-24 |w| max(1, |y|))) per entry.  The bounds are from the
    formats: each sigmoid is one exp2, one add and one reciprocal on a value <= 1; the kernel's expression modelled in fp32 with
    exp2 and the reciprocal each moved by +-1 ulp over 4 x 10^5 logits in [-130, 130] errs by at most 3.72 x 2^-24 in delta and
    3.60 x 2^-24 max(1, |y|) in the loss (torch's own fp32 expression: 2.72 x 2^-24); 8 leaves a margin of about 2."""
    d64, l64, aw, y = delta_reference(y_dev, label, sigma, w)
    rd = (db3.detach().cpu().double() - d64).abs() / (8 * U24 * aw)
    rl = (loss.detach().cpu().double() - l64).abs() / (8 * U24 * aw * y.abs().clamp_min(1.0))
    return rd, rl


def check_delta(what, y_dev, db3, loss, label, sigma, w=1.0):
    """asserts both bounds of delta_ratios on every entry; returns the worst ratios (delta, loss)"""
    for k, t in (("pred", y_dev), ("d b3", db3), ("loss", loss)):
        _finite("%s: %s" % (what, k), t)
    rd, rl = delta_ratios(y_dev, db3, loss, label, sigma, w)
    worst = float(rd.max()), float(rl.max())
    print("%s: worst |d b3 - |w| delta64| / bound = %.3f, worst |loss - |w| l64| / bound = %.3f" % (what, worst[0], worst[1]))
    assert worst[0] <= 1.0, "%s: d b3 is %.2f x its bound at y = %g" % (what, worst[0], float(y_dev.flatten()[int(rd.argmax())]))
    assert worst[1] <= 1.0, "%s: loss is %.2f x its bound at y = %g" % (what, worst[1], float(y_dev.flatten()[int(rl.argmax())]))
    return worst


def sweep_grid():
    """(y targets, label / sigma) of the per-point sweep as two flat fp64 tensors, every pair once"""
    y = torch.tensor(Y_TARGETS, dtype=torch.float64)
    x = torch.tensor(LABEL_OVER_SIGMA, dtype=torch.float64)
    return y.repeat_interleave(x.numel()), x.repeat(y.numel())
