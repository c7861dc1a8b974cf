"""Cases, fp64 references, per-element scales and pins for the time-conditioned decoder kernels (csrc/shine_time_mlp.hip
k_time_mlp_fwd, csrc/shine_mlp_body.hpp k_mlp_bwd<MODE, true>).

A time case is a decoder case of tests/tier_a_kernel_cases.py (mlp_case) widened by one column: W1 -> [W1 | w_t] (w_t seeded normal
times a scale, every fifth entry exactly 0), f9 = [feat | ts], r9 = [r | 0] (ts gets no gradient, so nothing is asked of the ninth
column of d / d f9).  tier_a_kernel_cases._mlp_forms is dimension-agnostic: on the widened arrays it gives the fp64 closed forms of
the header of csrc/shine_time_mlp.hip and, with absolute values, the per-element scales — the scale of a pre-activation now
includes |w_t| |ts|; column 8 of grad_feat is dropped.  tests/test_time_decoder.py pins the closed forms to the reference's own
Decoder.time_conditionded_sdf differentiated by torch.autograd in fp64.

The rule is that file's rule: |x - ref64| <= K 2^-24 scale, scale 0 -> exactly 0.0.  Near-kink points are judged on the 9-wide input
(tier_a_kernel_cases.near_kink) and redrawn, so no check skips a point.  on_kink and dead_points keep zero features AND ts == 0 on
their first quarter: z1 == b1 exactly there and relu'(0) = 0.  wt_zero is the fixture decoder with w_t all zeros.

The pins of the two families (time_point: pred, grad_feat, d/dg; time_weight: the weight sums of both backward passes), measured as
that file prescribes: the largest ratio of the fp32 CPU composite — the reference's op sequence cat -> Linear -> relu -> Linear ->
relu -> Linear, one thread, differentiated by torch.autograd — over every case of CASES, rounded up to the next half;
K = 4 max(pin, 1).  tests/test_time_decoder.py measures them again.
"""
import functools
from types import SimpleNamespace

import torch

import tier_a_kernel_cases as tc

TS_KINDS = ("frames", "unit", "zero")  # frames: integers in [0, 1100) as floats, what time_pool holds; unit: uniform in [0, 1)
WT_SCALES = (0.3, 0.01)
DECODERS = ("fixture", "b1_third", "on_kink", "dead_points", "wt_zero")
SIZES_WGRAD = (1, 63, 64, 65, 255, 256, 257, 24576, 24577)  # 24576 = 96 * 4 * 64: the last size with one tile per wave
SIZES_POINT = SIZES_WGRAD + (524289,)  # one past 2048 workgroups
SMALL = 257  # the other decoders run the sizes up to here
FRAMES = 1100

# family -> the fp32 composite's largest ratio over CASES (the figure in the comment), rounded up to the next half
RHO_REF = {
    "time_point": 4.5,   # 4.32  pred, grad_feat, d/dg                                      (fixture, unit, w_t 0.3, n = 524289)
    "time_weight": 9.0,  # 8.69  the weight sums of the backward and of the double backward   (dead_points, frames, w_t 0.3, n = 255)
}
K = {fam: 4.0 * max(rho, 1.0) for fam, rho in RHO_REF.items()}


def sizes(decoder, wgrad):
    s = SIZES_WGRAD if wgrad else SIZES_POINT
    return s if decoder == "fixture" else tuple(n for n in s if n <= SMALL)


def variants(decoder):
    """(ts kind, w_t scale) of a decoder's cases; w_t == 0 has no scale to vary"""
    return [(kind, 0.0 if decoder == "wt_zero" else wt) for kind in TS_KINDS for wt in (WT_SCALES[:1] if decoder == "wt_zero" else WT_SCALES)]


CASES = [(d, kind, wt, n) for d in DECODERS for kind, wt in variants(d) for n in sizes(d, False)]


@functools.lru_cache(maxsize=None)
def time_weights(decoder, wt_scale):
    """the six fp32 tensors of one time decoder: W1 [32,9] = [W1 of the 8-wide case | w_t], the other five as they are"""
    base = tc.decoder_weights("fixture" if decoder == "wt_zero" else decoder)
    gen = torch.Generator().manual_seed(tc._seed("w_t", decoder, wt_scale))
    wt = torch.randn(32, generator=gen) * wt_scale
    wt[::5] = 0.0
    if decoder == "wt_zero":
        wt.zero_()
    return [torch.cat((base[0], wt[:, None]), 1).contiguous()] + [p.clone() for p in base[1:]]


def _draw_ts(kind, n, gen):
    if kind == "frames":
        return torch.randint(0, FRAMES, (n,), generator=gen).float()
    if kind == "unit":
        return torch.rand(n, generator=gen)
    if kind == "zero":
        return torch.zeros(n)
    raise ValueError(kind)


@functools.lru_cache(maxsize=64)
def time_case(decoder, kind, wt_scale, n):
    """inputs of one case: params (6 fp32, W1 [32,9]), feat [n,8], ts [n], g [n], r [n,8], zero_points and how many points the kink
    rule, judged on [feat | ts], redrew on top of the 8-wide case's own"""
    base = tc.mlp_case("fixture" if decoder == "wt_zero" else decoder, n)
    params = time_weights(decoder, wt_scale)
    gen = torch.Generator().manual_seed(tc._seed("time", decoder, kind, wt_scale, n))
    ts = _draw_ts(kind, n, gen)
    ts[base.zero_points] = 0.0
    feat = base.feat.clone()
    redrawn = 0
    for _ in range(64):
        bad = tc.near_kink(params, torch.cat((feat, ts[:, None]), 1))
        assert not bool((bad & base.zero_points).any()), "a zero-feature point sits near a kink: the decoder case itself is off"
        k = int(bad.sum())
        if k == 0:
            break
        redrawn += k
        feat[bad] = torch.randn(k, 8, generator=gen) * 0.5
    else:
        raise AssertionError("the kink rule did not settle")
    return SimpleNamespace(decoder=decoder, kind=kind, wt_scale=wt_scale, n=n, params=params, feat=feat.contiguous(),
                           ts=ts.contiguous(), g=base.g, r=base.r, zero_points=base.zero_points, redrawn=redrawn)


def widened(case):
    """the case as tier_a_kernel_cases' closed forms take it: feat = [feat | ts], r = [r | 0]"""
    return SimpleNamespace(params=case.params, n=case.n, g=case.g, feat=torch.cat((case.feat, case.ts[:, None]), 1),
                           r=torch.cat((case.r, torch.zeros(case.n, 1)), 1))


def time_closed(case, absolute):
    """tier_a_kernel_cases.mlp_closed on the widened case, column 8 of grad_feat dropped: pred, grad_feat [n,8], dg, gw (gw[0]
    [32,9]: its last column is sum_i ts_i d1_i) and bb (bb[0][:,8] and the biases: zeros, scale zero)"""
    out = tc.mlp_closed(widened(case), absolute)
    out["grad_feat"] = out["grad_feat"][:, :8].contiguous()
    return out


@functools.lru_cache(maxsize=16)
def time_reference(decoder, kind, wt_scale, n):
    """(case, fp64 reference, scales) of one case: computed once, shared, never written to"""
    case = time_case(decoder, kind, wt_scale, n)
    return case, time_closed(case, False), time_closed(case, True)


def composite(params, feat, ts):
    """the reference's op sequence (model/decoder.py:65-81) on explicit tensors"""
    W1, b1, W2, b2, w3, b3 = params
    h = torch.cat((feat, ts.view(-1, 1)), dim=1)
    h = torch.relu(torch.nn.functional.linear(h, W1, b1))
    h = torch.relu(torch.nn.functional.linear(h, W2, b2))
    return torch.nn.functional.linear(h, w3, b3).squeeze(1)


def time_autograd(case, dtype=torch.float32, fn=None, chunk=32768):
    """`fn(params, feat, ts)` (default: composite) differentiated by torch.autograd in `dtype`, in the shape of time_closed's
    results.  fp32 — what the pins are measured on — runs in one piece, fp64 in chunks of points."""
    fn = fn or composite
    P = [p.detach().to(dtype).clone().requires_grad_(True) for p in case.params]
    parts = []
    for a, b in tc._chunks(case.n, chunk if dtype != torch.float32 else 0):
        f = case.feat[a:b].to(dtype).clone().requires_grad_(True)
        g = case.g[a:b].to(dtype).clone().requires_grad_(True)
        pred = fn(P, f, case.ts[a:b].to(dtype))
        first = torch.autograd.grad(pred, [f] + P, g, create_graph=True)
        s = (first[0] * case.r[a:b].to(dtype)).sum()
        second = torch.autograd.grad(s, [g] + P, allow_unused=True)
        bb = [torch.zeros_like(p) if t is None else t for t, p in zip(second[1:], P)]
        parts.append(dict(pred=pred.detach(), grad_feat=first[0].detach(), dg=second[0].detach(),
                          gw=[t.detach() for t in first[1:]], bb=[t.detach() for t in bb]))
    return tc._merge(parts)


def flushes(n):
    """how many workgroups of a backward launch over n points add their sums to a weight-grad element (the grid cap of
    csrc/shine_mlp_body.hpp's mlp_bwd_grid): each is one fp32 atomic add"""
    return min(96, -(-n // 256))


def ratios_into(x, ref, scale, v0, adds):
    """tier_a_kernel_cases.ratios for a buffer that held the CONSTANT v0 and received `adds` atomic adds: every add rounds a value of
    magnitude at most |v0| + scale with a relative error of at most 2^-24 (fp32's unit roundoff: half an ulp is 2^-24 of a value
    whose mantissa is 1.0), so next to the K 2^-24 scale of the sum itself the element may be off by adds * 2^-24 |v0|
    (tier_a_kernel_cases.ratios allows the 2^-24 |v0| of a single add; tier_a_kernel_cases.prefill avoids the term by filling with an eighth of each element's own scale; here the buffers hold one
    constant, as large as it likes against a small element).  Scale 0: nothing but exact zeros is added, v0 comes back to the bit."""
    x = torch.as_tensor(x).detach().double().cpu().reshape(ref.shape)
    err = ((x - (ref.double() + v0)).abs() - adds * tc.U24 * abs(v0)).clamp_min(0.0)
    inf = torch.full_like(err, float("inf"))
    return torch.where(scale > 0, err / (tc.U24 * scale.double()).clamp_min(1e-300), torch.where(x == v0, torch.zeros_like(err), inf))


def check_time(what, got, ref, scale, v0=None, adds=1):
    """every output present in `got` (pred / grad_feat / dg: "time_point"; gw / bb: "time_weight"; v0: the constant the weight
    buffers held before the call, `adds` = flushes(n)) -> {family: rho}; asserts rho <= K[family] on every element, exact zeros (v0
    to the bit) where the scale is zero"""
    rho = {"time_point": 0.0, "time_weight": 0.0}

    def one(name, fam, x, r, s, v=None):
        t = torch.as_tensor(x).detach()
        assert bool(torch.isfinite(t).all()), name + " is not finite"
        ratios = tc.ratios(t, r, s) if v is None else ratios_into(t, r, s, v, adds)
        worst = float(ratios.max()) if ratios.numel() else 0.0
        if worst > K[fam]:
            at = int(ratios.flatten().argmax())
            raise AssertionError("%s: element %d is %.3g x 2^-24 scale off (K = %g): got %r, fp64 %r, scale %r"
                                 % (name, at, worst, K[fam], float(t.double().flatten()[at]), float(r.flatten()[at]),
                                    float(s.flatten()[at])))
        rho[fam] = max(rho[fam], worst)

    for k in tc.MLP_POINT:
        if got.get(k) is not None:
            one("%s: %s" % (what, k), "time_point", got[k], ref[k], scale[k])
    for k in ("gw", "bb"):
        if got.get(k) is not None:
            for i, x in enumerate(got[k]):
                one("%s: %s[%d]" % (what, k, i), "time_weight", x, ref[k][i], scale[k][i], v0)
    return rho


def case_id(decoder, kind, wt_scale, n):
    return "time/%s/%s/wt=%g/n=%d" % (decoder, kind, wt_scale, n)


# ---- the Mesher's query at one time stamp: interpolation + decoder in one launch (csrc/shine_query.hip fed with
# Decoder.fused_params_at(ts)), on the octree of the mesh_query_L3 fixture
QUERY_FIXTURE = "mesh_query_L3"
QUERY_TS = (0, 3, 250)
QUERY_N = 4097
QUERY_WT = 0.01
# the family of its SDF values, pinned by the same rule: the fp32 CPU oracle (oracle.shine_oracle's query_feature, then the
# composite at constant ts) against fp64 over the three time stamps
RHO_REF["time_query"] = 1.0  # 0.79  (ts = 250; the scale's ceiling of 1 per corner weight is eight times the weights' sum)
K["time_query"] = 4.0 * max(RHO_REF["time_query"], 1.0)


@functools.lru_cache(maxsize=None)
def query_weights(wt_scale=QUERY_WT):
    """the decoder of the query fixture's source, widened: W1 [32,9] = [W1 | w_t] (every fifth entry of w_t exactly 0)"""
    from conftest import load_golden

    sd = load_golden(load_golden(QUERY_FIXTURE)["source"])["decoder"]
    base = [sd[k].clone().float().contiguous() for k in tc.svc.NAMES]
    gen = torch.Generator().manual_seed(tc._seed("w_t", QUERY_FIXTURE, wt_scale))
    wt = torch.randn(32, generator=gen) * wt_scale
    wt[::5] = 0.0
    return [torch.cat((base[0], wt[:, None]), 1).contiguous()] + base[1:]


def _query_forms(params, coord, ts, source):
    """(fp64 features, their scale, the points near a kink) of `coord` at time stamp `ts`: the features are sum_l interp(F_l) and
    their scale the same with |F| and every corner weight replaced by 1 (tier_a_kernel_cases.interp_tables); a point is near a
    kink when 0 < |z| < KINK_EPS scale(z) for a hidden unit, the feature's scale standing in for |f| — what the kernel's fp32
    interpolation can move z by is a multiple of 2^-24 of THAT"""
    case = SimpleNamespace(name=source, coord=coord)
    tables = tc._oracle_pair(source, True).hier_features
    f, fs = tc.interp_tables(case, tables), tc.interp_tables(case, tables, absolute=True)
    W1, b1, W2, b2, _, _ = tc._wide_params(params)
    col = torch.full((coord.shape[0], 1), float(ts), dtype=torch.float64)
    z1 = torch.cat((f, col), 1) @ W1.T + b1
    s1 = torch.cat((fs, col.abs()), 1) @ W1.abs().T + b1.abs()
    m1 = (z1 > 0).double()
    z2 = (m1 * z1) @ W2.T + b2
    s2 = (m1 * s1) @ W2.abs().T + b2.abs()
    bad = ((z1 != 0) & (z1.abs() < tc.KINK_EPS * s1)).any(1) | ((z2 != 0) & (z2.abs() < tc.KINK_EPS * s2)).any(1)
    return f, fs, bad, (m1, (z2 > 0).double())


@functools.lru_cache(maxsize=None)
def query_reference(ts):
    """(coord [QUERY_N,3] fp32 scaled, fp64 pred, scale) of the query case at time stamp `ts`: points drawn in the fixture's box,
    the ones near a kink redrawn; pred is the decoder's output (Mesher.query_points returns its negative)"""
    from conftest import load_golden

    fx = load_golden(QUERY_FIXTURE)
    src = load_golden(fx["source"])
    params = query_weights()
    lo, hi = torch.tensor(fx["lo"], dtype=torch.float32), torch.tensor(fx["hi"], dtype=torch.float32)
    gen = torch.Generator().manual_seed(tc._seed("query", ts))
    draw = lambda k: ((lo + (hi - lo) * torch.rand(k, 3, generator=gen)) * float(src["scale"])).float()
    coord = draw(QUERY_N)
    for _ in range(64):
        f, fs, bad, masks = _query_forms(params, coord, ts, fx["source"])
        k = int(bad.sum())
        if k == 0:
            break
        coord[bad] = draw(k)
    else:
        raise AssertionError("the kink rule did not settle")
    P = tc._wide_params(params)
    col = torch.full((QUERY_N, 1), float(ts), dtype=torch.float64)
    zero = torch.zeros(QUERY_N, dtype=torch.float64)
    zeros9 = torch.zeros(QUERY_N, 9, dtype=torch.float64)
    ref = tc._mlp_forms(P, torch.cat((f, col), 1), zero, zeros9, *masks)["pred"]
    scale = tc._mlp_forms([p.abs() for p in P], torch.cat((fs, col.abs()), 1), zero, zeros9, *masks)["pred"]
    return coord.contiguous(), ref, scale


def query_oracle32(ts):
    """the fp32 CPU oracle on the query case: query_feature in fp32 (the reference's op sequence), then the composite"""
    from conftest import load_golden

    coord, _, _ = query_reference(ts)
    oct_ = tc._oracle_pair(load_golden(QUERY_FIXTURE)["source"], False)
    with torch.no_grad():
        feat = oct_.query_feature(coord)
        return composite(query_weights(), feat, torch.full((QUERY_N,), float(ts)))


def check_query(what, x, ref, scale):
    """a [QUERY_N] decoder output against fp64 within K["time_query"] 2^-24 of each element's scale -> rho"""
    rho = tc.ratios(torch.as_tensor(x), ref, scale)
    worst = float(rho.max())
    assert worst <= K["time_query"], "%s: element %d is %.3g x 2^-24 scale off (K = %g)" % (what, int(rho.argmax()), worst,
                                                                                           K["time_query"])
    return worst
