"""Oracle of the time-conditioned training step (csrc/shine_time_step.hip, ops.fused_time_step) — helper, no tests.

    widen(mlp, w_t)                                          the oracle decoder's W1 -> [W1 | w_t] ([32,9])
    time_sdf(mlp, feat, ts)                                  Decoder.time_conditionded_sdf's op sequence on the widened head
    time_step(oct_, mlp, coord, label, weight, ts, ...)      the step on oracle.shine_oracle's OracleOctree through torch autograd
    case(name, kind, eik)                                    one step fixture with its ts, its w_t and its fp64 oracle

The step (the definition everywhere): f = query_feature(x); pred = head([f | ts]); bce = BCEWithLogits(pred, sigmoid(label / sigma))
('mean' or 'sum'); with the eikonal term g = sigma d pred / d x and eik = the mean over the rows with weight > 0 of (1 - |g|)^2 (0
without such a row; torch's norm has a zero subgradient at g = 0, the fused step's guard); loss = bce + weight_e eik; backward.

FP32 FORM: the reference's op sequence with so.coord_gradient.  WIDE FORM (after so.to_wide): fp64 behind the fp32 coordinate
arithmetic, differentiated with respect to an fp64 `delta` added behind the cast — normal_step_oracle explains why.

CASES: normal_step_oracle.FIXTURES, each with and without the eikonal term, in the ts / w_t kinds of time_decoder_cases: "frames"
(frame ids in [0, 1100) with w_t at scale 0.01), "unit" (uniform [0,1) with w_t at scale 0.3) and "wt_zero" (frame ids, w_t = 0).
"""
import functools
from types import SimpleNamespace

import torch

import normal_step_oracle as nso
from conftest import load_golden, oracle_from_golden

FIXTURES = nso.FIXTURES
KINDS = ("frames", "unit", "wt_zero")
FRAMES = 1100
WT_SCALE = {"frames": 0.01, "unit": 0.3, "wt_zero": 0.0}
# every (fixture, kind, eik); test_time_step.py::test_the_pin_is_honest holds each to TOL / 4 between the fp32 and the wide oracle,
# and a case that failed it would be taken out HERE, with a comment, never loosened
CASES = [(name, kind, eik) for name in FIXTURES for kind in KINDS for eik in (False, True)]


def _seed(*parts):
    h = 1469598103934665603
    for ch in "/".join(str(p) for p in parts).encode():
        h = ((h ^ ch) * 1099511628211) % (1 << 61)
    return h


def draw_ts(kind, n, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "unit":
        return torch.rand(n, generator=gen)
    return torch.randint(0, FRAMES, (n,), generator=gen).float()


def draw_wt(kind, seed):
    gen = torch.Generator().manual_seed(seed)
    wt = torch.randn(32, generator=gen) * WT_SCALE[kind]
    wt[::5] = 0.0
    return wt


def widen(mlp, w_t):
    """the oracle decoder's first layer with the time column: W1 [32,8] -> [W1 | w_t] [32,9] (a fresh leaf)"""
    mlp.W1 = torch.cat((mlp.W1.detach(), w_t.to(mlp.W1.dtype).reshape(-1, 1)), 1).contiguous().requires_grad_(True)
    return mlp


def time_sdf(mlp, feat, ts):
    """model/decoder.py:65-81 on the widened oracle decoder"""
    h = torch.cat((feat, ts.to(feat.dtype).view(-1, 1)), dim=1)
    h = torch.relu(torch.nn.functional.linear(h, mlp.W1, mlp.b1))
    h = torch.relu(torch.nn.functional.linear(h, mlp.W2, mlp.b2))
    return torch.nn.functional.linear(h, mlp.w3, mlp.b3).squeeze(1)


def wide_features(oct_, coord, delta):
    """query_feature in the oracle's wide mode with the fp64 offset `delta` behind the fp32 coordinate arithmetic"""
    oct_.set_zero()
    hidx = oct_.get_indices(coord)
    dtype = oct_.acc_dtype
    L = oct_.featured_level_num
    acc = torch.zeros(coord.shape[0], oct_.feature_dim, dtype=dtype)
    for i in range(L):
        t, _ = nso._axis(oct_, coord, oct_.max_level - i, dtype, delta)
        acc = acc + (oct_.hier_features[L - i - 1][hidx[i]] * nso._corner_weights(t).unsqueeze(2)).sum(1)
    return acc


def time_step(oct_, mlp, coord, label, weight, ts, sigma, eik=False, weight_e=0.1, reduction="mean"):
    """One iteration minus the optimiser on the CPU oracle (fp32, or wide after so.to_wide) -> dict(loss, pred, g | None,
    feat_grads [as oct_.hier_features], mlp_grads [6, W1's is [32,9]])"""
    from oracle import shine_oracle as so

    oct_.zero_grad()
    mlp.zero_grad()
    wide = getattr(oct_, "acc_dtype", torch.float32) != torch.float32
    coord = coord.detach().clone()
    g = None
    if wide:
        delta = torch.zeros(coord.shape, dtype=oct_.acc_dtype, requires_grad=True)
        pred = time_sdf(mlp, wide_features(oct_, coord, delta), ts)
        if eik:
            g = so.coord_gradient(delta, pred) * sigma
    else:
        coord.requires_grad_(eik)
        pred = time_sdf(mlp, oct_.query_feature(coord), ts)
        if eik:
            g = so.coord_gradient(coord, pred) * sigma
    loss = so.sdf_bce_loss(pred, label, sigma, reduction)
    if eik:
        surf = weight > 0
        if bool(surf.any()):
            loss = loss + weight_e * ((1.0 - g[surf].norm(2, dim=-1)) ** 2).mean()
    loss.backward()
    return dict(loss=loss.detach(), pred=pred.detach(), g=None if g is None else g.detach(),
                feat_grads=[torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in oct_.hier_features],
                mlp_grads=[torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in mlp.params()])


def oracle_for(fx, w_t, wide):
    from oracle import shine_oracle as so

    _, oct_, mlp = oracle_from_golden(fx)
    widen(mlp, w_t)
    if wide:
        so.to_wide(oct_, mlp)
    return oct_, mlp


def weight_e_of(fx):
    return float(fx["cfg"].get("weight_e", 0.1))


@functools.lru_cache(maxsize=None)
def inputs(name, kind):
    """(fixture, ts [n], w_t [32]) of a case: computed once, shared, never written to"""
    fx = load_golden(name)
    return fx, draw_ts(kind, fx["coord"].shape[0], _seed("ts", name, kind)), draw_wt(kind, _seed("w_t", name, kind))


@functools.lru_cache(maxsize=None)
def case(name, kind, eik):
    """One case with its fp64 oracle: computed once, shared, never written to"""
    fx, ts, w_t = inputs(name, kind)
    oct_, mlp = oracle_for(fx, w_t, wide=True)
    wide = time_step(oct_, mlp, fx["coord"], fx["sdf_label"], fx["weight"], ts, fx["sigma"], eik=eik, weight_e=weight_e_of(fx))
    return SimpleNamespace(name=name, kind=kind, eik=eik, fx=fx, coord=fx["coord"], label=fx["sdf_label"], weight=fx["weight"],
                           ts=ts, w_t=w_t, sigma=fx["sigma"], weight_e=weight_e_of(fx), wide=wide)


def case_id(name, kind, eik):
    return "%s/%s/%s" % (name, kind, "eik" if eik else "bce")


rel_errors = nso.rel_errors
