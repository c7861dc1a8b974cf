"""Cases, fp64 references, per-element scales and checkers for the Tier A autograd kernels (csrc/shine_mlp.hip k_mlp_fwd /
k_mlp_bwd<MODE>, csrc/shine_interp.hip k_interp_bwd<POLY, SECOND>).

The rule.  Every element x of every output is held to

    |x - ref64| <= K * 2^-24 * scale        scale == 0  ->  x == 0.0 exactly,

where ref64 is the fp64 value of the reference's function on the fp32 inputs (the oracle in its wide mode, differentiated by
torch.autograd) and `scale` is the SAME expression with every factor replaced by its absolute value (|W|, |b|, |f|, |g|, |r|,
|F|; the ReLU masks stay as they are).  An interpolation coefficient enters a scale by a ceiling, not by itself — 1 for a
corner weight, sup |d w_c / d x_a| = 2^(l-1) max |t'| (t' = 6 d (1 - d) <= 1.5 for the smooth step, 1 for linear weights) for a
weight derivative — because a weight 1 - t near zero carries an absolute, not a relative, rounding error, and so does t' as the
reference's autograd evaluates it (6 d - 6 d^2: at d one ulp below a voxel face, where the edge fixtures put points on purpose, its
fp32 value is off by more than t' itself; with max_c |d w_c / d x_a| of the point as the ceiling the fp32 oracle's own ratio is
10^6 and no K derived from it would reject anything).  A scale depends only on the points that touch its element, never on a
maximum over the tensor: a feature-grad row that one small-g point touches is held to that point's size, and a dead unit's
weight-grad row (scale 0) to exactly zero.

K, one per output family (RHO_REF lists them), is not chosen: RHO_REF below is the largest ratio |x - ref64| / (2^-24 scale)
that the fp32 CPU oracle (the reference's op sequence: index_put_(accumulate) and GEMM in index order) shows on any case of the
family, and
K = 4 max(RHO_REF, 1) — the kernels add in another order (fp32 atomics, 64-point LDS contractions, lane-strided accumulators) and
contract to FMA, which moves the realised error without changing its worst case.  tests/test_tier_a_kernels.py re-measures the
oracle's ratios on the CPU and fails when one exceeds K / 4; profiles/tier_a_kernel_parity.txt records them next to the
kernels' own.

ReLU kinks.  A point whose fp64 pre-activation is nearly 0 can take the other branch in fp32; that is a property of the input.
Such points (0 < |z| < 1e-4 (|W||f| + |b|) for any hidden unit, judged in fp64) are redrawn before a case is used, so no check
skips a point.  Exact kinks (z == 0 in both precisions) are placed on purpose: relu'(0) = 0.

The interpolation reference computes voxel ids and d = frac(2^l (x/2 + 1/2)) in fp32 exactly as the reference does
(oracle.shine_oracle.to_wide, OracleOctree.get_indices) and differentiates with respect to d as an fp64 leaf: the oracle's own
query_feature_with_indices casts d to fp64 inside, and autograd would round d loss / d coord to fp32 on the way back through
that cast.  `corner_weights` restates interp_weights on a given d; the CPU tests pin it to interp_weights and the resulting feature
sum to query_feature_with_indices bit for bit.
"""
import functools
import zlib
from types import SimpleNamespace

import torch

import step_value_cases as svc
from conftest import oracle_from_golden

U24 = 2.0 ** -24

# ---- the pins: family -> the fp32 oracle's largest ratio over every case of the family, measured on the CPU with one thread (the
# figure in the comment) and rounded up to the next half (torch's GEMM blocks its sums by CPU and thread count: 5.79 with eight
# threads where one gives 7.10); tests/test_tier_a_kernels.py measures them again.  K = 4 max(rho_ref, 1).
RHO_REF = {
    "mlp_point": 4.5,     # 4.32  pred, grad_feat, d/dg                                            (fixture decoder, n = 524289)
    "mlp_weight": 7.5,    # 7.10  the six weight sums of the backward, dW1 / dW2 / dw3 of the double backward
    "interp_point": 3.5,  # 3.06  grad_coord, d/dg
    "interp_row": 7.0,    # 6.78  feature-grad rows of both passes, every batch but "repeat"
    "interp_trash": 2.0,  # 1.52  their trash rows
    # the rows of the "repeat" batch (2^20 + 1 points: 512 times the summands per row, which the reference adds one after the other
    # in fp32) are families of their own: one K for all rows would loosen the 33 small cases forty-fold
    "interp_row_repeat": 300.0,    # 290.5
    "interp_trash_repeat": 170.0,  # 162.5
}
K = {fam: 4.0 * max(rho, 1.0) for fam, rho in RHO_REF.items()}


def record(case_id, rho):
    """append the ratios of one case to the file TIER_A_PARITY_LOG names, if any (profiles/tier_a_kernel_parity.txt is made of these)"""
    import os

    path = os.environ.get("TIER_A_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            for fam in sorted(rho):
                fh.write("%s %s %.3f\n" % (case_id, fam, rho[fam]))


# ---- decoder cases
DECODER_FIXTURE = "kitti_eik_L3"
DECODERS = ("fixture", "dead", "dead_points", "on_kink", "b1_third", "big_out")
SIZES_WGRAD = (1, 63, 64, 65, 255, 256, 257, 24576, 24577, 49345)  # 24576 = 96 * 4 * 64: the last size with one tile per wave
SIZES_POINT = SIZES_WGRAD + (524289,)  # one past 2048 workgroups
SMALL = 257  # the other decoders run the sizes up to here
KINK_EPS = 1e-4


def mlp_sizes(decoder, wgrad):
    sizes = SIZES_WGRAD if wgrad else SIZES_POINT
    return sizes if decoder == "fixture" else tuple(n for n in sizes if n <= SMALL)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def decoder_weights(decoder):
    """the six fp32 tensors W1 [32,8], b1, W2 [32,32], b2, w3 [1,32], b3 [1] of one decoder case"""
    fx = svc.fixture(DECODER_FIXTURE)
    if decoder in ("dead", "dead_points", "on_kink"):
        sd = svc.value_case(fx, decoder).decoder
    else:
        sd = {k: fx["decoder"][k].clone().float() for k in svc.NAMES}
        if decoder == "b1_third":
            sd["layers.0.bias"][::3] = -100.0  # those units are dead on every point: their weight-grad rows are exactly zero
        elif decoder == "big_out":
            sd["lout.weight"] *= 1024.0
            sd["lout.bias"] *= 1024.0
        elif decoder != "fixture":
            raise ValueError(decoder)
    return [sd[k].contiguous() for k in svc.NAMES]


def _wide_params(params):
    W1, b1, W2, b2, w3, b3 = [p.detach().double() for p in params]
    return [W1, b1, W2, b2, w3.reshape(-1), b3.reshape(())]


def near_kink(params, feat):
    """bool [n]: the points with 0 < |z| < KINK_EPS (|W||f| + |b|) for some hidden unit of either layer, judged in fp64"""
    W1, b1, W2, b2, _, _ = _wide_params(params)
    f = feat.double()
    z1 = f @ W1.T + b1
    s1 = f.abs() @ W1.abs().T + b1.abs()
    m1 = (z1 > 0).double()
    z2 = (m1 * z1) @ W2.T + b2
    s2 = (m1 * s1) @ W2.abs().T + b2.abs()
    bad = ((z1 != 0) & (z1.abs() < KINK_EPS * s1)).any(1) | ((z2 != 0) & (z2.abs() < KINK_EPS * s2)).any(1)
    return bad


@functools.lru_cache(maxsize=64)
def mlp_case(decoder, n):
    """inputs of one decoder case: params (6 fp32), feat [n,8], g [n], r [n,8], zero_points (bool [n]) and how many points the
    kink rule redrew"""
    params = decoder_weights(decoder)
    gen = torch.Generator().manual_seed(_seed("mlp", decoder, n))
    feat = torch.randn(n, 8, generator=gen) * 0.5
    zero_points = torch.zeros(n, dtype=torch.bool)
    if decoder in ("on_kink", "dead_points"):
        zero_points[:(n + 3) // 4] = True  # the first quarter: all-zero features (z1 == b1 exactly)
    feat[zero_points] = 0.0
    redrawn = 0
    for _ in range(64):
        bad = near_kink(params, feat)
        assert not bool((bad & zero_points).any()), "a zero-feature point sits near a kink: the decoder case itself is off"
        k = int(bad.sum())
        if k == 0:
            break
        redrawn += k
        feat[bad] = torch.randn(k, 8, generator=gen) * 0.5
    else:
        raise AssertionError("the kink rule did not settle")
    mag = 10.0 ** (torch.rand(n, generator=gen) * 9.0 - 6.0)  # 1e-6 .. 1e3
    g = mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g[9::10] = 0.0
    r = torch.randn(n, 8, generator=gen)
    return SimpleNamespace(decoder=decoder, n=n, params=params, feat=feat.contiguous(), g=g.contiguous(), r=r.contiguous(),
                           zero_points=zero_points, redrawn=redrawn)


MLP_POINT = ("pred", "grad_feat", "dg")


def _oracle_decoder(params, dtype):
    from oracle import shine_oracle as so

    mlp = so.OracleDecoder(so.make_config())
    mlp.load_state_dict(dict(zip(svc.NAMES, params)))
    if dtype != torch.float32:
        for k in ("W1", "b1", "W2", "b2", "w3", "b3"):
            setattr(mlp, k, getattr(mlp, k).detach().to(dtype).requires_grad_(True))
    return mlp


def _chunks(n, chunk):
    step = n if not chunk else chunk
    return [(a, min(a + step, n)) for a in range(0, max(n, 1), max(step, 1))]


def _merge(parts):
    out = {k: torch.cat([p[k] for p in parts]) for k in MLP_POINT}
    for k in ("gw", "bb"):
        out[k] = [sum(p[k][i] for p in parts) for i in range(6)]
    return out


def mlp_autograd(case, dtype=torch.float64, chunk=32768):
    """OracleDecoder.sdf differentiated by torch.autograd in `dtype`: pred, grad_feat = g d pred / d feat, gw = the six weight
    grads of sum g pred, and of s = sum grad_feat . r: dg = ds / dg, bb = ds / d(W1, b1, W2, b2, w3, b3) (the biases: exact zeros).
    fp64 runs in chunks of points (the sums add in fp64); fp32 — the oracle that the pins are measured on — in one piece."""
    mlp = _oracle_decoder(case.params, dtype)
    P = mlp.params()
    parts = []
    for a, b in _chunks(case.n, chunk if dtype != torch.float32 else 0):
        f = case.feat[a:b].to(dtype).clone().requires_grad_(True)
        g = case.g[a:b].to(dtype).clone().requires_grad_(True)
        pred = mlp.sdf(f)
        first = torch.autograd.grad(pred, [f] + P, g, create_graph=True)
        s = (first[0] * case.r[a:b].to(dtype)).sum()
        second = torch.autograd.grad(s, [g] + P, allow_unused=True)
        bb = [torch.zeros_like(p) if t is None else t for t, p in zip(second[1:], P)]
        parts.append(dict(pred=pred.detach(), grad_feat=first[0].detach(), dg=second[0].detach(),
                          gw=[t.detach() for t in first[1:]], bb=[t.detach() for t in bb]))
    return _merge(parts)


def _mlp_forms(P, f, g, r, m1, m2):
    W1, b1, W2, b2, w3, b3 = P
    h1 = m1 * (f @ W1.T + b1)
    h2 = m2 * (h1 @ W2.T + b2)
    v2 = m2 * w3
    v1 = m1 * (v2 @ W2)
    d2, d1 = g[:, None] * v2, g[:, None] * v1
    a1 = m1 * (r @ W1.T)
    a2 = m2 * (a1 @ W2.T)
    zero = torch.zeros_like
    return dict(pred=h2 @ w3 + b3, grad_feat=d1 @ W1, dg=(v1 * a1).sum(1),
                gw=[d1.T @ f, d1.sum(0), d2.T @ h1, d2.sum(0), (g[:, None] * h2).sum(0)[None], g.sum()[None]],
                bb=[d1.T @ r, zero(b1), d2.T @ a1, zero(b2), (g[:, None] * a2).sum(0)[None], zero(b3)[None]])


def mlp_closed(case, absolute, chunk=32768):
    """The closed forms of shine_mlp.hip's header in fp64 (absolute=False: the values mlp_autograd returns) or with every factor
    replaced by its absolute value and the masks kept (absolute=True: the scale of every element)."""
    P = _wide_params(case.params)
    parts = []
    for a, b in _chunks(case.n, chunk):
        f, g, r = case.feat[a:b].double(), case.g[a:b].double(), case.r[a:b].double()
        z1 = f @ P[0].T + P[1]
        m1 = (z1 > 0).double()
        m2 = ((m1 * z1) @ P[2].T + P[3] > 0).double()
        if absolute:
            parts.append(_mlp_forms([p.abs() for p in P], f.abs(), g.abs(), r.abs(), m1, m2))
        else:
            parts.append(_mlp_forms(P, f, g, r, m1, m2))
    return _merge(parts)


# ---- interpolation cases
INTERP_FIXTURES = ("edges_L3", "edges_L2_nopoly_eik", "maicity_bce_L4")  # smooth-step L3, linear L2, L4: both POLY builds
PREFIXES = (1, 63, 64, 65, 255, 256, 257)
BATCHES = tuple("prefix%d" % k for k in PREFIXES) + ("whole", "misses", "alternate", "one_leaf", "repeat")
REPEAT_N = 4096 * 256 + 1  # one past the 4096-workgroup cap


def repeat_factor(k):
    """g and gg of repeat k of the "repeat" batch are the base vectors times this (a power of two: exact in fp32)"""
    return 2.0 ** (k % 5 - 2)


@functools.lru_cache(maxsize=None)
def _oracle_pair(name, wide):
    from oracle import shine_oracle as so

    _, oct_, mlp = oracle_from_golden(svc.fixture(name))
    oct_.set_zero()
    if wide:
        so.to_wide(oct_, mlp)
    return oct_


@functools.lru_cache(maxsize=None)
def _hit_miss(name):
    """(points of the fixture batch that hit at every level, points that miss at every level)"""
    fx = svc.fixture(name)
    idx = fx["out"]["indices"]
    hit = torch.stack([(t >= 0).all(1) for t in idx], 1).all(1)
    miss = torch.stack([(t < 0).all(1) for t in idx], 1).all(1)
    misses = fx["coord"][miss]
    if misses.shape[0] < 150:  # (the recorded batches of the shipped configurations: samples outside the mapped shell)
        gen = torch.Generator().manual_seed(_seed("miss", name))
        cand = torch.rand(4096, 3, generator=gen) * 2 - 1
        cidx = _oracle_pair(name, False).get_indices(cand)
        misses = cand[torch.stack([(t < 0).all(1) for t in cidx], 1).all(1)]
    return fx["coord"][hit], misses


@functools.lru_cache(maxsize=None)
def interp_batch(name, batch):
    """coord [n,3], g [n,8], gg [n,3] of one interpolation case, fp32 on the CPU.  "repeat" returns its BASE batch (the fixture's)
    and n = REPEAT_N; expand_repeat builds the tensors the kernel receives."""
    fx = svc.fixture(name)
    gen = torch.Generator().manual_seed(_seed("interp", name, batch))
    base = fx["coord"]
    hits, misses = _hit_miss(name)
    if batch.startswith("prefix"):
        coord = base[:int(batch[6:])]
    elif batch in ("whole", "repeat"):
        coord = base
    elif batch == "misses":
        coord = misses[:300]
    elif batch == "alternate":  # hit and miss lane by lane
        k = min(150, hits.shape[0], misses.shape[0])
        coord = torch.stack((hits[:k], misses[:k]), 1).reshape(-1, 3)
    elif batch == "one_leaf":  # the heaviest same-row atomics: 300 points in one leaf voxel
        from test_gpu_edges import _voxel_points

        coord = _voxel_points(hits[0], _oracle_pair(name, False).max_level, 300, gen)
    else:
        raise ValueError(batch)
    coord = coord.clone().contiguous()
    n = coord.shape[0]
    assert n > 0
    mag = 10.0 ** (torch.rand(n, generator=gen) * 9.0 - 6.0)
    g = torch.randn(n, 8, generator=gen) * mag[:, None]
    g[9::10] = 0.0
    gg = torch.randn(n, 3, generator=gen)
    return SimpleNamespace(name=name, batch=batch, coord=coord, g=g.contiguous(), gg=gg.contiguous(), n_base=n,
                           n=REPEAT_N if batch == "repeat" else n)


def expand_repeat(case, device="cpu"):
    """(coord, g, gg) of the "repeat" batch at its full size: the base batch tiled, g and gg of repeat k times repeat_factor(k)"""
    nb, n = case.n_base, case.n
    reps = (n + nb - 1) // nb
    s = torch.tensor([repeat_factor(k) for k in range(reps)], dtype=torch.float32, device=device).repeat_interleave(nb)[:n, None]
    tile = lambda t: t.to(device).repeat(reps, 1)[:n]
    return tile(case.coord).contiguous(), (tile(case.g) * s).contiguous(), (tile(case.gg) * s).contiguous()


def corner_weights(d, poly):
    """OracleOctree.interp_weights (model/feature_octree.py:172-196) on a given d [n,3] -> [n,8]"""
    if poly:
        tx, ty, tz = (3 * (d[:, a] ** 2) - 2 * (d[:, a] ** 3) for a in range(3))
    else:
        tx, ty, tz = d[:, 0], d[:, 1], d[:, 2]
    ux, uy, uz = 1 - tx, 1 - ty, 1 - tz
    return torch.stack((ux * uy * uz, ux * uy * tz, ux * ty * uz, ux * ty * tz, tx * uy * uz, tx * uy * tz, tx * ty * uz,
                        tx * ty * tz), 0).T


def _levels(oct_, coord):
    """per level, bottom-up as the oracle loops: (table index fl, ids [n,8] with -1 for the trash row, fp32 d [n,3] in the
    oracle's accumulation dtype, d u / d x)"""
    idx = oct_.get_indices(coord)
    dtype = getattr(oct_, "acc_dtype", torch.float32)
    out = []
    for i in range(oct_.featured_level_num):
        lvl = oct_.max_level - i
        d = torch.frac((2 ** lvl) * (coord * 0.5 + 0.5)).to(dtype)  # fp32 arithmetic, as interp_weights
        out.append((oct_.featured_level_num - i - 1, idx[i], d, float(2 ** lvl) * 0.5))
    return out


def interp_autograd(case, wide=True, coord=None, g=None, gg=None):
    """The oracle's interpolation differentiated by torch.autograd with respect to d (leaves in the accumulation dtype):
    feat, grad_coord [n,3], rows1 = the dense d / d F_l of sum feat . g (top-down, trash row last), and of s = sum grad_coord . gg:
    dg [n,8] and rows2 = d s / d F_l."""
    oct_ = _oracle_pair(case.name, wide)
    coord = case.coord if coord is None else coord
    dtype = getattr(oct_, "acc_dtype", torch.float32)
    g = (case.g if g is None else g).detach().to(dtype).clone().requires_grad_(True)  # (a copy: the case is shared)
    gg = (case.gg if gg is None else gg).to(dtype)
    F = [t.detach().clone().requires_grad_(True) for t in oct_.hier_features]
    lv = _levels(oct_, coord)
    ds = [d.clone().requires_grad_(True) for _, _, d, _ in lv]
    feat = 0
    for (fl, ids, _, _), d in zip(lv, ds):
        feat = feat + (F[fl][ids] * corner_weights(d, oct_.poly).unsqueeze(2)).sum(1)
    first = torch.autograd.grad(feat, ds + F, g, create_graph=True)
    grad_coord = sum(t * dudx for t, (_, _, _, dudx) in zip(first[:len(ds)], lv))
    second = torch.autograd.grad((grad_coord * gg).sum(), [g] + F, allow_unused=True)
    rows2 = [torch.zeros_like(f) if t is None else t for t, f in zip(second[1:], F)]
    return dict(feat=feat.detach(), grad_coord=grad_coord.detach(), dg=second[0].detach(),
                rows1=[t.detach() for t in first[len(ds):]], rows2=[t.detach() for t in rows2])


_BITS = torch.tensor([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)], dtype=torch.bool)  # corner c -> (x, y, z) bit


def _weight_grads(d, poly, dudx):
    """d w_c / d x_a [n,8,3] in closed form"""
    t = 3 * d ** 2 - 2 * d ** 3 if poly else d
    dt = (6 * d * (1 - d) if poly else torch.ones_like(d)) * dudx
    side = torch.where(_BITS[None], t[:, None, :], 1 - t[:, None, :])  # [n,8,3]: the factor of axis a in corner c
    sign = torch.where(_BITS, 1.0, -1.0).to(d.dtype)
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        out.append(sign[None, :, a] * dt[:, None, a] * side[:, :, b] * side[:, :, c])
    return torch.stack(out, 2)


def interp_closed(case, absolute, coord=None, g=None, gg=None):
    """The closed forms of shine_interp.hip's header in fp64 (absolute=False: the values interp_autograd returns) or the scale of
    every element (absolute=True): |F|, |g|, |gg|, a corner weight replaced by 1 and d w_c / d x_a by max_c |d w_c / d x_a|."""
    oct_ = _oracle_pair(case.name, True)
    coord = case.coord if coord is None else coord
    g = (case.g if g is None else g).double()
    gg = (case.gg if gg is None else gg).double()
    n = coord.shape[0]
    if absolute:
        g, gg = g.abs(), gg.abs()
    F = [t.detach().abs() if absolute else t.detach() for t in oct_.hier_features]
    grad_coord, dg = torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, 8, dtype=torch.float64)
    rows1, rows2 = [torch.zeros_like(f) for f in F], [torch.zeros_like(f) for f in F]
    for fl, ids, d, dudx in _levels(oct_, coord):
        w = corner_weights(d, oct_.poly)
        dw = _weight_grads(d, oct_.poly, dudx)
        if absolute:
            w = torch.ones_like(w)
            dw = torch.full_like(dw, dudx * (1.5 if oct_.poly else 1.0))
        rows = torch.where(ids < 0, F[fl].shape[0] - 1, ids).reshape(-1)
        Fc = F[fl][rows].reshape(n, 8, 8)  # [point, corner, feature]
        grad_coord += torch.einsum("pca,pcf,pf->pa", dw, Fc, g)
        rows1[fl].index_add_(0, rows, (w[:, :, None] * g[:, None, :]).reshape(-1, 8))
        coef = torch.einsum("pca,pa->pc", dw, gg)
        dg += torch.einsum("pc,pcf->pf", coef, Fc)
        rows2[fl].index_add_(0, rows, (coef[:, :, None] * g[:, None, :]).reshape(-1, 8))
    return dict(grad_coord=grad_coord, dg=dg, rows1=rows1, rows2=rows2)


def _repeat_sums(case, power):
    """(sum of repeat_factor(k)^power over the full repeats, the last repeat's factor^power, its number of points)"""
    full, rem = divmod(case.n, case.n_base)
    return sum(repeat_factor(k) ** power for k in range(full)), repeat_factor(full) ** power, rem


def _expand(case, fn):
    """the results of `fn` (interp_autograd / interp_closed with coord, g, gg keywords) for a case at its full size.  g and gg of
    the "repeat" batch are exact multiples of the base vectors, so its fp64 results are the base batch's — per point times the
    repeat's factor, the rows of the first pass times sum_k factor_k, of the second pass (linear in g AND gg) times sum_k
    factor_k^2 — plus the same of the prefix the last, partial repeat covers: the reference costs what 2048 points cost."""
    base = fn(case)
    if case.batch != "repeat":
        return base
    nb, n = case.n_base, case.n
    reps = (n + nb - 1) // nb
    s = torch.tensor([repeat_factor(k) for k in range(reps)], dtype=torch.float64).repeat_interleave(nb)[:n, None]
    out = {k: base[k].repeat(reps, 1)[:n] * s for k in ("grad_coord", "dg")}
    for key, power in (("rows1", 1), ("rows2", 2)):
        full, last, rem = _repeat_sums(case, power)
        tail = fn(case, coord=case.coord[:rem], g=case.g[:rem], gg=case.gg[:rem])[key] if rem else None
        out[key] = [r * full + (t * last if tail is not None else 0) for r, t in zip(base[key], tail or [None] * len(base[key]))]
    return out


@functools.lru_cache(maxsize=8)
def interp_reference(name, batch):
    """(case, fp64 reference, scales) of one interpolation case at its full size: computed once, shared, never written to"""
    case = interp_batch(name, batch)
    ref = _expand(case, lambda c, **kw: interp_autograd(c, True, **kw))
    scale = _expand(case, lambda c, **kw: interp_closed(c, True, **kw))
    return case, ref, scale


def interp_oracle32(name, batch):
    """The fp32 oracle on one case, in the shape of interp_reference's results.  The "repeat" batch: the per-point results are the
    base batch's times the repeat's factor (exact), the rows are the reference's index_put_(accumulate) — fp32, in index order —
    over all of its points, one repeat after the other into the same rows."""
    case = interp_batch(name, batch)
    base = interp_autograd(case, wide=False)
    if batch != "repeat":
        return base
    nb, n = case.n_base, case.n
    reps = (n + nb - 1) // nb
    s = torch.tensor([repeat_factor(k) for k in range(reps)], dtype=torch.float32).repeat_interleave(nb)[:n, None]
    out = {k: base[k].repeat(reps, 1)[:n] * s for k in ("grad_coord", "dg")}
    oct_ = _oracle_pair(name, False)
    lv = _levels(oct_, case.coord)
    rows1 = [torch.zeros_like(f.detach()) for f in oct_.hier_features]
    rows2 = [torch.zeros_like(f.detach()) for f in oct_.hier_features]
    terms = []
    for fl, ids, d, dudx in lv:
        coef = torch.einsum("pca,pa->pc", _weight_grads(d, oct_.poly, dudx), case.gg)
        terms.append((fl, ids.reshape(-1), (corner_weights(d, oct_.poly)[:, :, None] * case.g[:, None, :]).reshape(-1, 8),
                      (coef[:, :, None] * case.g[:, None, :]).reshape(-1, 8)))
    for k in range(reps):
        m = min(nb, n - k * nb) * 8
        f = repeat_factor(k)
        for fl, ids, c1, c2 in terms:
            rows1[fl].index_put_((ids[:m],), c1[:m] * f, accumulate=True)
            rows2[fl].index_put_((ids[:m],), c2[:m] * (f * f), accumulate=True)
    out["rows1"], out["rows2"] = rows1, rows2
    return out


# --------------------------------------------------------------------------------------------------------------- the checkers


def ratios(x, ref, scale, v0=None):
    """|x - (v0 + ref)| / (2^-24 scale) per element, after the allowance 2^-24 |v0| for a buffer that held v0; an element whose
    scale is 0 gives 0 if it is exactly v0 (0.0 without v0), infinity otherwise"""
    x = torch.as_tensor(x).detach().double().cpu().reshape(ref.shape)
    want = ref.double() if v0 is None else ref.double() + v0.double()
    err = (x - want).abs()
    if v0 is not None:
        err = (err - U24 * v0.double().abs()).clamp_min(0.0)
    scale = scale.double()
    exact = x == (torch.zeros_like(x) if v0 is None else v0.double())
    inf = torch.full_like(err, float("inf"))
    return torch.where(scale > 0, err / (U24 * scale).clamp_min(1e-300), torch.where(exact, torch.zeros_like(err), inf))


def check(what, family, x, ref, scale, v0=None):
    """asserts |x - ref64| <= K[family] 2^-24 scale on every element (exact zeros where the scale is zero) and returns the largest
    ratio rho = |x - ref64| / (2^-24 scale)"""
    t = torch.as_tensor(x).detach()
    assert bool(torch.isfinite(t).all()), what + " is not finite"
    rho = ratios(t, ref, scale, v0)
    worst = float(rho.max()) if rho.numel() else 0.0
    if worst > K[family]:
        at = int(rho.flatten().argmax())
        raise AssertionError("%s: element %d is %.3g x 2^-24 scale off (K = %g): got %r, fp64 %r, scale %r"
                             % (what, at, worst, K[family], float(t.double().flatten()[at]), float(ref.flatten()[at]),
                                float(scale.flatten()[at])))
    return worst


def check_rows(what, rows, ref, scale, v0=None, suffix=""):
    """the feature-grad tables of one pass, top-down: every row but the last as "interp_row", the trash row as "interp_trash"
    (`suffix` "_repeat": the large batch's families) -> (rho of the rows, rho of the trash rows)"""
    rr, rt = 0.0, 0.0
    for k, (x, r, s) in enumerate(zip(rows, ref, scale)):
        v = [None, None] if v0 is None else [v0[k][:-1], v0[k][-1]]
        rr = max(rr, check("%s level %d" % (what, k), "interp_row" + suffix, x[:-1], r[:-1], s[:-1], v[0]))
        rt = max(rt, check("%s level %d trash row" % (what, k), "interp_trash" + suffix, x[-1], r[-1], s[-1], v[1]))
    return rr, rt


def check_mlp(what, got, ref, scale, v0=None):
    """every output present in `got` (pred / grad_feat / dg: "mlp_point"; gw / bb: "mlp_weight", v0 = what the buffers held)
    -> {family: rho}"""
    rho = {"mlp_point": 0.0, "mlp_weight": 0.0}
    for k in MLP_POINT:
        if got.get(k) is not None:
            rho["mlp_point"] = max(rho["mlp_point"], check("%s: %s" % (what, k), "mlp_point", got[k], ref[k], scale[k]))
    for k in ("gw", "bb"):
        if got.get(k) is not None:
            for i, x in enumerate(got[k]):
                v = None if v0 is None else v0[i]
                rho["mlp_weight"] = max(rho["mlp_weight"], check("%s: %s[%d]" % (what, k, i), "mlp_weight", x, ref[k][i],
                                                                 scale[k][i], v))
    return rho


def check_interp(what, got, ref, scale, suffix=""):
    """every output present in `got` (grad_coord, dg, rows1, rows2) -> {family: rho}; `suffix` as for check_rows"""
    rho = {"interp_point": 0.0, "interp_row" + suffix: 0.0, "interp_trash" + suffix: 0.0}
    for k in ("grad_coord", "dg"):
        if got.get(k) is not None:
            rho["interp_point"] = max(rho["interp_point"], check("%s: %s" % (what, k), "interp_point", got[k], ref[k], scale[k]))
    for k in ("rows1", "rows2"):
        if got.get(k) is not None:
            rr, rt = check_rows("%s: %s" % (what, k), got[k], ref[k], scale[k], suffix=suffix)
            rho["interp_row" + suffix] = max(rho["interp_row" + suffix], rr)
            rho["interp_trash" + suffix] = max(rho["interp_trash" + suffix], rt)
    return rho


@functools.lru_cache(maxsize=16)
def mlp_reference(decoder, n):
    """(case, fp64 reference, scales) of one decoder case: computed once, shared, never written to"""
    case = mlp_case(decoder, n)
    return case, mlp_autograd(case), mlp_closed(case, True)


def prefill(scale, seed):
    """What an ACCUMULATED INTO buffer holds before the call, fp32: +- an eighth of the element's own scale (so that the additions
    round at the sums' own magnitude, which K covers) and 0.375 where the scale is zero — those must come back to the bit."""
    gen = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(scale.shape, generator=gen) < 0.5, -1.0, 1.0)
    v = (0.125 * scale.double() * sign).float()
    return torch.where(scale > 0, v, torch.full_like(v, 0.375))


def interp_tables(case, tables, absolute=False):
    """sum_l interp(T_l) [n,8] in fp64 for tables T_l shaped like the feature tables (top-down; a miss addresses the last row with
    all eight corners): d / d g of sum_l sum grad_F_l . T_l.  absolute=True: its scale (|T|, every corner weight replaced by 1)."""
    oct_ = _oracle_pair(case.name, True)
    out = torch.zeros(case.coord.shape[0], 8, dtype=torch.float64)
    for fl, ids, d, _ in _levels(oct_, case.coord):
        w = corner_weights(d, oct_.poly)
        T = tables[fl].detach().double().cpu()
        if absolute:
            w, T = torch.ones_like(w), T.abs()
        out += (T[ids] * w[:, :, None]).sum(1)
    return out
