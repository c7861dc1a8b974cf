"""Oracle of the ray-rendering training step (csrc/shine_ray_step.hip, ops.fused_ray_step) — helper, no tests.

    ray_step(oct_, mlp, coord, weight, depth, ray_depth, sigma_size, ...)   the step on oracle.shine_oracle's OracleOctree through
                                                                            torch autograd
    case(name, neus, eik, S)                                                one step fixture as rays with its fp64 oracle

The step (the definition everywhere): f = query_feature(x); pred = Decoder.sdf(f); y = sigmoid(pred / sigma_size);
render = the project's composite losses.batch_ray_rendering_loss_composite(depth [m,S], y [m,S], ray_depth [m], neus_on); with the
eikonal term g = sigma d pred / d x and eik = the mean over the rows with weight > 0 of (1 - |g|)^2 (0 without such a row; torch's
norm has a zero subgradient at g = 0, the fused step's guard); loss = render + weight_e eik; backward into the tables, the six
decoder tensors and sigma_size.  d loss / d sigma_size rides as a seventh one-element tensor at the end of `mlp_grads`.

FP32 FORM: the reference's op sequence with so.coord_gradient.  WIDE FORM (after so.to_wide): fp64 behind the fp32 coordinate
arithmetic, differentiated with respect to an fp64 `delta` added behind the cast — normal_step_oracle explains why.

CASES: normal_step_oracle.FIXTURES as rays — consecutive rows grouped into rays of S, the remainder dropped — x {dr, dr_neus} x
{plain, + eikonal} x S in {6, 9}.  Sample depths and measured depths are seeded; ray 1 of every case has two equal depths (the
sort's tie, broken by column).  sigma_size: dr uses 1.0 at S = 6 and 0.2 at S = 9; dr_neus uses 1.0 and the builder asserts
max |pred| / sigma_size <= 3 — beyond about 5 the quotient's 1 - y + 1e-10 cancels in fp32 and no fp32 evaluation holds TOL.
The fixtures' decoders reach |pred| = 10, so a dr_neus case scales its head's OUTPUT layer (w3, b3) by out_scale(name): the
power of two that brings the fixture's max |pred| to at most 2.5 (1 where it already is).  The dr cases keep the decoder as it is.

CASE TABLE: all 40 cases are in; none was dropped and no seed had to be changed.
"""
import functools
from types import SimpleNamespace

import torch

import normal_step_oracle as nso
import time_step_oracle as to
from conftest import load_golden, oracle_from_golden

FIXTURES = nso.FIXTURES
SAMPLES = (6, 9)
NEUS_MAX_ARG = 3.0
# every (fixture, neus, eik, S); test_ray_step.py::test_the_pin_is_honest holds each to TOL / 4 between the fp32 and the wide oracle.
# No case may be removed: a case that missed would get another seed, said in the table above.
CASES = [(name, neus, eik, S) for name in FIXTURES for neus in (False, True) for eik in (False, True) for S in SAMPLES]


def sigma_size_of(neus, S):
    return 1.0 if (neus or S == 6) else 0.2


def draw_depths(m, S, seed):
    """(sample_depth [m*S], ray_depth [m]): seeded; ray 1 (ray 0 of a single ray) has two equal depths"""
    gen = torch.Generator().manual_seed(seed)
    depth = torch.rand(m, S, generator=gen) * 2.0 + 0.1
    ray_depth = torch.rand(m, generator=gen) * 2.0 + 0.1
    if S >= 2:
        r = 1 if m > 1 else 0
        depth[r, S - 1] = depth[r, 0]
    return depth.reshape(-1).contiguous(), ray_depth


def composite(depth, y, ray_depth, neus):
    """losses.batch_ray_rendering_loss_composite, line for line, with the sort asked to be STABLE: ties go by column, which is the
    step's definition.  torch.sort without the flag keeps that order only for short rows (the S = 17 and 32 edge cases have a
    tie in a row of more than 16).  test_ray_step.py holds this to the project's composite and to the reference's function."""
    x, order = depth.sort(dim=1, stable=True)
    prob = y.gather(1, order)
    if neus:
        lo, hi = prob[:, :-1], prob[:, 1:]
        a = ((hi - lo) / (1.0 - lo + 1e-10)).clamp(0.0, 1.0)
    else:
        a = prob
    o = torch.ones_like(a) - a + 1e-10
    w = o.cumprod(dim=1) / o * a
    d = (w * x[:, :a.shape[1]]).sum(dim=1)
    return (d - ray_depth).abs().mean()


def ray_step(oct_, mlp, coord, weight, depth, ray_depth, sigma_size, sigma, S, neus=False, eik=False, weight_e=0.1):
    """One iteration minus the optimiser on the CPU oracle (fp32, or wide after so.to_wide) -> dict(loss, pred, dpred = d render / d
    pred, feat_grads [as oct_.hier_features], mlp_grads [6 decoder tensors + d loss / d sigma_size as one element])"""
    from oracle import shine_oracle as so

    oct_.zero_grad()
    mlp.zero_grad()
    wide = getattr(oct_, "acc_dtype", torch.float32) != torch.float32
    dtype = oct_.acc_dtype if wide else torch.float32
    coord = coord.detach().clone()
    m = ray_depth.numel()
    ss = torch.tensor([float(sigma_size)], dtype=dtype, requires_grad=True)
    g = None
    if wide:
        delta = torch.zeros(coord.shape, dtype=dtype, requires_grad=True)
        pred = mlp.sdf(to.wide_features(oct_, coord, delta))
        if eik:
            g = so.coord_gradient(delta, pred) * sigma
    else:
        coord.requires_grad_(eik)
        pred = mlp.sdf(oct_.query_feature(coord))
        if eik:
            g = so.coord_gradient(coord, pred) * sigma
    y = torch.sigmoid(pred / ss)
    render = composite(depth.to(dtype).view(m, S), y.view(m, S), ray_depth.to(dtype), neus)
    dpred = torch.autograd.grad(render, pred, retain_graph=True, allow_unused=True)[0]
    loss = render
    if eik:
        surf = weight > 0
        if bool(surf.any()):
            loss = loss + weight_e * ((1.0 - g[surf].norm(2, dim=-1)) ** 2).mean()
    if loss.requires_grad:
        loss.backward()
    return dict(loss=loss.detach(), pred=pred.detach(), dpred=torch.zeros_like(pred).detach() if dpred is None else dpred.detach(),
                feat_grads=[torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in oct_.hier_features],
                mlp_grads=[torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in mlp.params()]
                + [torch.zeros_like(ss) if ss.grad is None else ss.grad.clone()])


@functools.lru_cache(maxsize=None)
def out_scale(name, neus):
    """the factor on the head's output layer of a case: 1 for dr; for dr_neus the power of two that brings max |pred| <= 2.5"""
    if not neus:
        return 1.0
    fx = load_golden(name)
    _, oct_, mlp = oracle_from_golden(fx)
    with torch.no_grad():
        top = float(mlp.sdf(oct_.query_feature(fx["coord"])).abs().max())
    k = 1.0
    while top * k > 2.5:
        k *= 0.5
    return k


def oracle_for(fx, wide, scale=1.0):
    from oracle import shine_oracle as so

    _, oct_, mlp = oracle_from_golden(fx)
    if scale != 1.0:
        mlp.w3 = (mlp.w3.detach() * scale).requires_grad_(True)
        mlp.b3 = (mlp.b3.detach() * scale).requires_grad_(True)
    if wide:
        so.to_wide(oct_, mlp)
    return oct_, mlp


weight_e_of = to.weight_e_of


@functools.lru_cache(maxsize=None)
def inputs(name, S):
    """(fixture, coord [m*S,3], weight [m*S], sample_depth [m*S], ray_depth [m]) of a case: computed once, shared, never written to"""
    fx = load_golden(name)
    m = fx["coord"].shape[0] // S
    depth, ray_depth = draw_depths(m, S, to._seed("ray", name, S))
    return fx, fx["coord"][:m * S].contiguous(), fx["weight"][:m * S].contiguous(), depth, ray_depth


@functools.lru_cache(maxsize=None)
def case(name, neus, eik, S):
    """One case with its fp64 oracle: computed once, shared, never written to"""
    fx, coord, weight, depth, ray_depth = inputs(name, S)
    ss = sigma_size_of(neus, S)
    oct_, mlp = oracle_for(fx, wide=True, scale=out_scale(name, neus))
    wide = ray_step(oct_, mlp, coord, weight, depth, ray_depth, ss, fx["sigma"], S, neus=neus, eik=eik, weight_e=weight_e_of(fx))
    if neus:
        arg = float(wide["pred"].abs().max()) / ss
        assert arg <= NEUS_MAX_ARG, "dr_neus case %s: max |pred| / sigma_size = %.2f > %g" % (name, arg, NEUS_MAX_ARG)
    return SimpleNamespace(name=name, neus=neus, eik=eik, S=S, fx=fx, coord=coord, weight=weight, depth=depth, ray_depth=ray_depth,
                           out_scale=out_scale(name, neus), sigma_size=ss, sigma=fx["sigma"], weight_e=weight_e_of(fx), wide=wide)


def case_id(name, neus, eik, S):
    return "%s/%s/%s/S%d" % (name, "dr_neus" if neus else "dr", "eik" if eik else "plain", S)


rel_errors = nso.rel_errors
