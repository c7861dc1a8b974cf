"""Oracle of the surface-normal training term (csrc/shine_normal_step.hip, ops.fused_normal_step, losses.normal_loss) — helper,
no tests.

    normal_term(oct_, mlp, coord, weight, normal, weight_n, sigma=1.0)   the CPU oracle through torch autograd
    closed_form(oct_, mlp, coord, weight, normal, weight_n)              the issue's formulas in fp64 torch, no autograd through g
    case(name)                                                           one step fixture with its labels and its fp64 oracle

The term (the definition everywhere): g = d pred / d coord; gh = g / |g| where |g| > 0, else 0 (THE GUARD — the reference's lines
give NaN there, and fail to broadcast without keepdim); l = |gh - n|_2; normal_loss = the mean of l over the rows with weight > 0
(0 without one); the gradients are those of weight_n * normal_loss.  Rows with weight <= 0 never read their label.

WIDE MODE.  so.to_wide is used as it is meant: the coordinates stay fp32 — voxel ids and the fractions d = frac(2^l (x/2 + 1/2))
are the reference's fp32 arithmetic — and everything downstream is fp64.  Casting the coordinates themselves to fp64 moves the
voxel fractions and changes the answer by up to 90 % of max-abs on edges_L2_nopoly_eik.  torch's autograd rounds d pred / d coord
to the coordinates' fp32 on its way back through that cast, so the wide oracle differentiates with respect to an fp64 offset
`delta` (zero) added to the coordinate behind the cast, d -> d + 2^l / 2 * delta: the same derivative, kept in fp64.

LABELS (labels_for): seeded random unit vectors with hand-made rows mixed in — on live surface rows a zero vector, a vector of
length 0.3 and -gh of the fp64 oracle; on one free-space row NaN (it must never be read).  CONDITION ON THE INPUTS (not a
tolerance): on every live surface row (|g| > 0) the fp64 oracle's l >= 0.05 — below it u = d / l is rounding noise in any fp32
evaluation, the reference's included.  Random unit labels violate it on about 1 row in 1600, so a label that does is replaced by
its negative, and the condition is asserted: no test depends on the seed.
"""
import functools
from types import SimpleNamespace

import torch

from conftest import load_golden, oracle_from_golden

FIXTURES = ["kitti_eik_L3", "maicity_bce_L4", "edges_L2_nopoly_eik", "maicity_bce_L3", "linear_L2_nopoly"]
WEIGHT_N = 0.7
MIN_ELL = 0.05


def _corner_weights(t):
    """[N,3] axis weights -> [N,8] corner weights, corner c = 4 cx + 2 cy + cz (FeatureOctree.interpolat's order)"""
    u = 1 - t
    ax = (u, t)
    return torch.stack([ax[(c >> 2) & 1][:, 0] * ax[(c >> 1) & 1][:, 1] * ax[c & 1][:, 2] for c in range(8)], 1)


def _axis(oct_, coord, lvl, dtype, delta=None):
    """d (fp32 arithmetic, then `dtype`), the axis weights t(d) and dt / dx of one level"""
    d = torch.frac((2 ** lvl) * (coord * 0.5 + 0.5)).to(dtype)
    half = (2 ** lvl) * 0.5
    if delta is not None:
        d = d + half * delta
    if oct_.poly:
        return 3 * d ** 2 - 2 * d ** 3, 6 * (d - d ** 2) * half
    return d, torch.full_like(d, half)


def _wide_pred(oct_, mlp, coord, delta):
    oct_.set_zero()
    hidx = oct_.get_indices(coord)
    dtype = oct_.acc_dtype
    L = oct_.featured_level_num
    acc = torch.zeros(coord.shape[0], oct_.feature_dim, dtype=dtype)
    for i in range(L):
        t, _ = _axis(oct_, coord, oct_.max_level - i, dtype, delta)
        acc = acc + (oct_.hier_features[L - i - 1][hidx[i]] * _corner_weights(t).unsqueeze(2)).sum(1)
    return mlp.sdf(acc)


def _term(g, weight, normal):
    """(normal_loss, l per surface row, live per surface row) of the definition, differentiable in g"""
    surf = weight > 0
    gs, ns = g[surf], normal[surf].to(g.dtype)
    if gs.shape[0] == 0:
        return g.sum() * 0.0, gs.new_zeros(0), torch.zeros(0, dtype=torch.bool)
    gn = gs.norm(2, dim=-1, keepdim=True)
    live = gn > 0
    gh = torch.where(live, gs / torch.where(live, gn, torch.ones_like(gn)), torch.zeros_like(gs))
    ell = (gh - ns).norm(2, dim=-1)
    return ell.sum() / gs.shape[0], ell.detach(), live.squeeze(1)


def normal_term(oct_, mlp, coord, weight, normal, weight_n, sigma=1.0):
    """The term on the CPU oracle by autograd (fp32: the reference's op sequence with get_gradient; after so.to_wide: fp64 behind
    the fp32 coordinate arithmetic).  `sigma` multiplies g as the reference's sigma_sigmoid does.  -> dict(loss, g, ell, live,
    feat_grads [as oct_.hier_features], mlp_grads [6, zeros where no gradient arrives])"""
    from oracle import shine_oracle as so

    oct_.zero_grad()
    mlp.zero_grad()
    wide = getattr(oct_, "acc_dtype", torch.float32) != torch.float32
    coord = coord.detach().clone()
    if wide:
        delta = torch.zeros(coord.shape, dtype=oct_.acc_dtype, requires_grad=True)
        pred = _wide_pred(oct_, mlp, coord, delta)
        g = so.coord_gradient(delta, pred) * sigma
    else:
        coord.requires_grad_(True)
        pred = mlp.sdf(oct_.query_feature(coord))
        g = so.coord_gradient(coord, pred) * sigma
    loss, ell, live = _term(g, weight, normal)
    if loss.requires_grad:
        (weight_n * loss).backward()
    return dict(loss=loss.detach(), g=g.detach(), ell=ell, live=live,
                feat_grads=[torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in oct_.hier_features],
                mlp_grads=[torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in mlp.params()],
                has_grad=[p.grad is not None for p in mlp.params()])


def closed_form(oct_, mlp, coord, weight, normal, weight_n):
    """The issue's formulas in fp64 torch, no autograd through g: A, the masks, v2 / v1 / J / g, q, r / a1 / a2, the three
    outer-product sums and the feature scatter (a miss: the level's trash row).  -> dict as normal_term, plus q [N,3]."""
    dt = torch.float64
    oct_.set_zero()
    hidx = oct_.get_indices(coord)
    L, n = oct_.featured_level_num, coord.shape[0]
    feats = [t.detach().to(dt) for t in oct_.hier_features]
    W1, b1, W2, b2, w3, _ = [p.detach().to(dt) for p in mlp.params()]
    f = torch.zeros(n, oct_.feature_dim, dtype=dt)
    A = torch.zeros(n, oct_.feature_dim, 3, dtype=dt)
    dws = []
    for i in range(L):
        t, dtdx = _axis(oct_, coord, oct_.max_level - i, dt)
        rows = feats[L - i - 1][hidx[i]]  # [n,8,F]; a miss reads the zero trash row
        f = f + (rows * _corner_weights(t).unsqueeze(2)).sum(1)
        u = 1 - t
        val, der = (u, t), (-dtdx, dtdx)
        dw = torch.zeros(n, 8, 3, dtype=dt)
        for c in range(8):
            cx, cy, cz = (c >> 2) & 1, (c >> 1) & 1, c & 1
            dw[:, c, 0] = der[cx][:, 0] * val[cy][:, 1] * val[cz][:, 2]
            dw[:, c, 1] = val[cx][:, 0] * der[cy][:, 1] * val[cz][:, 2]
            dw[:, c, 2] = val[cx][:, 0] * val[cy][:, 1] * der[cz][:, 2]
        dws.append(dw)
        A = A + torch.einsum("nca,ncq->nqa", dw, rows)
    z1 = f @ W1.T + b1
    m1 = (z1 > 0).to(dt)
    z2 = torch.relu(z1) @ W2.T + b2
    m2 = (z2 > 0).to(dt)
    v2 = m2 * w3.reshape(1, -1)
    v1 = m1 * (v2 @ W2)
    J = v1 @ W1
    g = torch.einsum("nq,nqa->na", J, A)
    surf = weight > 0
    n_surf = int(surf.sum())
    gn = g.norm(2, dim=-1, keepdim=True)
    live = (gn > 0) & surf.unsqueeze(1)
    gh = torch.where(gn > 0, g / torch.where(gn > 0, gn, torch.ones_like(gn)), torch.zeros_like(g))
    lab = torch.where(surf.unsqueeze(1), normal.to(dt), torch.zeros_like(g))
    d = gh - lab
    ell = d.norm(2, dim=-1, keepdim=True)
    u = torch.where(ell > 0, d / torch.where(ell > 0, ell, torch.ones_like(ell)), torch.zeros_like(d))
    q = (weight_n / max(n_surf, 1)) * (u - (u * gh).sum(1, keepdim=True) * gh) / torch.where(gn > 0, gn, torch.ones_like(gn))
    q = torch.where(live, q, torch.zeros_like(q))
    loss = ell[surf].sum() / n_surf if n_surf else torch.zeros((), dtype=dt)
    r = torch.einsum("nqa,na->nq", A, q)
    a1 = m1 * (r @ W1.T)
    a2 = m2 * (a1 @ W2.T)
    grads = [v1.T @ r, torch.zeros_like(b1), v2.T @ a1, torch.zeros_like(b2), a2.sum(0, keepdim=True), torch.zeros(1, dtype=dt)]
    feat_grads = [torch.zeros_like(t) for t in feats]
    for i in range(L):
        cq = torch.einsum("nca,na->nc", dws[i], q)  # [n,8]
        gl = feat_grads[L - i - 1]
        idx = hidx[i].clone()
        idx[idx < 0] = gl.shape[0] - 1  # the trash row
        gl.index_put_((idx.reshape(-1),), (cq.unsqueeze(2) * J.unsqueeze(1)).reshape(-1, J.shape[1]), accumulate=True)
    return dict(loss=loss, g=g, q=q, ell=ell[surf].squeeze(1), live=live[surf].squeeze(1), feat_grads=feat_grads,
                mlp_grads=grads)


def wide_oracle(fx):
    from oracle import shine_oracle as so

    ocfg, oct_, mlp = oracle_from_golden(fx)
    so.to_wide(oct_, mlp)
    return oct_, mlp


def labels_for(fx, seed=11):
    """[n,3] float32 labels of a fixture's batch as the module docstring describes; the condition is asserted"""
    coord, weight = fx["coord"], fx["weight"]
    n = coord.shape[0]
    oct_, mlp = wide_oracle(fx)
    zero = torch.zeros(n, 3)
    g = normal_term(oct_, mlp, coord, torch.ones(n), zero, 1.0)["g"]  # fp64 g of every row
    gn = g.norm(2, dim=-1, keepdim=True)
    gh = torch.where(gn > 0, g / gn.clamp_min(1e-300), torch.zeros_like(g))
    gen = torch.Generator().manual_seed(seed)
    lab = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    lab = lab / lab.norm(dim=-1, keepdim=True)
    surf = weight > 0
    live = surf & (gn.squeeze(1) > 0)
    rows = torch.nonzero(live).flatten()
    hand = {}
    if rows.numel() >= 4:
        hand = dict(zero=int(rows[1]), short=int(rows[2]), opposite=int(rows[3]))
        lab[hand["zero"]] = 0.0
        lab[hand["short"]] = 0.3 * lab[hand["short"]]
        lab[hand["opposite"]] = -gh[hand["opposite"]]
    lab = lab.float()
    ell = (gh - lab.double()).norm(2, dim=-1)
    bad = live & (ell < MIN_ELL)
    lab[bad] = -lab[bad]
    ell = (gh - lab.double()).norm(2, dim=-1)
    assert bool((ell[live] >= MIN_ELL).all()), "the condition on the inputs: l >= %g on every live surface row" % MIN_ELL
    free = torch.nonzero(~surf).flatten()
    if free.numel():
        hand["nan"] = int(free[0])
        lab[hand["nan"]] = float("nan")
    return lab, hand


@functools.lru_cache(maxsize=None)
def case(name):
    """One step fixture with the helper's labels and its fp64 oracle at WEIGHT_N: computed once, shared, never written to.
    zero_g: the number of surface rows whose g is exactly zero (the rows the guard is for)."""
    fx = load_golden(name)
    normal, hand = labels_for(fx)
    oct_, mlp = wide_oracle(fx)
    wide = normal_term(oct_, mlp, fx["coord"], fx["weight"], normal, WEIGHT_N)
    zero_g = int((~wide["live"]).sum())
    return SimpleNamespace(name=name, fx=fx, coord=fx["coord"], weight=fx["weight"], normal=normal, hand=hand, wide=wide,
                           zero_g=zero_g)


def rel_errors(got_loss, got_feat, got_mlp, ref):
    """(loss error absolute-or-relative, per-tensor max-abs errors relative to the tensor's max-abs; a tensor whose oracle value
    is all zero: relative to the largest gradient tensor's max-abs) against an oracle dict"""
    refs = [t.double() for t in ref["feat_grads"] + ref["mlp_grads"]]
    gots = [t.detach().double().cpu() for t in list(got_feat) + list(got_mlp)]
    top = max(float(t.abs().max()) for t in refs)
    errs = []
    for a, b in zip(gots, refs):
        scale = float(b.abs().max())
        errs.append(float((a.reshape(b.shape) - b).abs().max()) / (scale if scale > 0 else max(top, 1e-300)))
    lg, lr = float(got_loss), float(ref["loss"])
    return abs(lg - lr) / max(1.0, abs(lr)), errs
