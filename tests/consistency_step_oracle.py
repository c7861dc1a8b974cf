"""Oracle of the gradient-consistency training term (csrc/shine_consistency_step.hip, ops.fused_consistency_step,
losses.consistency_loss) — helper, no tests.

    consistency_term(oct_, mlp, coord_a, coord_b, weight_c, sigma=1.0)   the CPU oracle through torch autograd
    pairs_for(fx, seed, oracle=None)                                     the pairs of a fixture, with the condition applied
    case(name)                                                           one step fixture with its pairs and its fp64 oracle

The term (the definition everywhere): K pairs, a_k = coord[near_index[k]], b_k = fl32(a_k + shift[k]); ga, gb = d pred / d coord
at the two points; c_k = (ga . gb) / (|ga| |gb|) where both norms are positive, else 0 (THE GUARD: such a pair contributes 1 and
gets no gradient on either side — the reference's F.cosine_similarity gives the same value and a gradient of gbh / 1e-8 on the
zero side); consistency_loss = the mean of 1 - c_k (0 for K = 0); the gradients are those of weight_c * consistency_loss, through
both points.  No weight, no label and no sigma enter.

WIDE MODE is normal_step_oracle's: the coordinates (b_k included: the sum is rounded to fp32 first) stay fp32, everything
downstream is fp64, and the derivative is taken with respect to an fp64 `delta` behind the cast.

PAIRS (pairs_for): near_index seeded uniform over ALL rows of the fixture's batch — free-space rows, the rows outside the mapped
box, repeats (entry 1 repeats entry 0) — and shifts uniform in [-s, s) per component with s = 2^-max_level, one finest-level cell
of the [-1,1] space.  CONDITION ON THE INPUTS (not a tolerance): q carries 1 / |g|, so a pair is left out when either fp64 |g| is
positive but below FAINT_G of the median over the live |g| of both sides; pairs with an exactly zero g stay in (the guard's
cases).  At most MAX_LEFT_OUT of a case's K_PAIRS pairs may go this way (asserted).  Also asserted: the shifted partner of every
base point inside (-1, 1) stays inside (-1, 1) — a shift component that would carry such a point across a face is negated first;
the fixtures' deliberate rows on and outside the box's faces are base points too: they miss every level and are guard cases
with their partners.
"""
import functools
from types import SimpleNamespace

import torch

import normal_step_oracle as no
from conftest import load_golden

FIXTURES = no.FIXTURES
WEIGHT_C = 0.7
K_PAIRS = 2048
FAINT_G = 1e-3
MAX_LEFT_OUT = 16
SEED = 5


def _g(oct_, mlp, coord, sigma):
    from oracle import shine_oracle as so

    wide = getattr(oct_, "acc_dtype", torch.float32) != torch.float32
    c = coord.detach().clone()
    if wide:
        delta = torch.zeros(c.shape, dtype=oct_.acc_dtype, requires_grad=True)
        return so.coord_gradient(delta, no._wide_pred(oct_, mlp, c, delta)) * sigma
    c.requires_grad_(True)
    return so.coord_gradient(c, mlp.sdf(oct_.query_feature(c))) * sigma


def term_of(ga, gb):
    """(consistency_loss, c per pair, live per pair) of the definition, differentiable in ga and gb"""
    if ga.shape[0] == 0:
        return (ga.sum() + gb.sum()) * 0.0, ga.new_zeros(0), torch.zeros(0, dtype=torch.bool)
    na, nb = ga.norm(2, dim=-1, keepdim=True), gb.norm(2, dim=-1, keepdim=True)
    live = ((na > 0) & (nb > 0)).squeeze(1)
    one = torch.ones_like(na)
    ah, bh = ga / torch.where(na > 0, na, one), gb / torch.where(nb > 0, nb, one)
    c = torch.where(live, (ah * bh).sum(-1), torch.zeros_like(na.squeeze(1)))
    return (1 - c).sum() / ga.shape[0], c.detach(), live


def consistency_term(oct_, mlp, coord_a, coord_b, weight_c, sigma=1.0):
    """The term on the CPU oracle by autograd over the pairs (coord_a[k], coord_b[k]) (fp32: the reference's op sequence with
    get_gradient on both point sets; after so.to_wide: fp64 behind the fp32 coordinate arithmetic).  `sigma` multiplies both
    gradients as the reference's sigma_sigmoid does.  -> dict(loss, ga, gb, c, live, feat_grads [as oct_.hier_features],
    mlp_grads [6, zeros where no gradient arrives])"""
    oct_.zero_grad()
    mlp.zero_grad()
    ga, gb = _g(oct_, mlp, coord_a, sigma), _g(oct_, mlp, coord_b, sigma)
    loss, c, live = term_of(ga, gb)
    if loss.requires_grad:
        (weight_c * loss).backward()
    return dict(loss=loss.detach(), ga=ga.detach(), gb=gb.detach(), c=c, live=live,
                feat_grads=[torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in oct_.hier_features],
                mlp_grads=[torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in mlp.params()],
                has_grad=[p.grad is not None for p in mlp.params()])


def pairs_for(fx, seed=SEED, oracle=None, k=K_PAIRS):
    """The pairs of a fixture's batch as the module docstring describes, for the map `oracle` = (oct_, mlp) in wide mode (default:
    the fixture's own).  -> near_index int32 [K'], shift float32 [K',3], coord_a, coord_b (fp32), left_out, zero_g — the K' <= k
    pairs that satisfy the condition; both assertions are made here, so no test depends on the seed."""
    oct_, mlp = oracle if oracle is not None else no.wide_oracle(fx)
    coord = fx["coord"]
    n = coord.shape[0]
    gen = torch.Generator().manual_seed(seed)
    near = torch.randint(0, n, (k,), generator=gen)
    near[1] = near[0]
    s = 2.0 ** (-oct_.max_level)
    shift = ((torch.rand(k, 3, generator=gen) * 2 - 1) * s).float()
    a = coord[near]
    inside = a.abs().max(1).values < 1
    crosses = inside.unsqueeze(1) & ((a + shift).float().abs() >= 1)
    shift = torch.where(crosses, -shift, shift)  # (a component that would carry an inside point across a face is negated)
    b = (a + shift).float()
    assert bool((b[inside].abs().max(1).values < 1).all()), "a shifted point left (-1, 1)"
    ga, gb = _g(oct_, mlp, a, 1.0).detach(), _g(oct_, mlp, b, 1.0).detach()
    na, nb = ga.norm(dim=-1), gb.norm(dim=-1)
    live = (na > 0) & (nb > 0)
    faint = torch.zeros_like(live)
    if bool(live.any()):
        med = torch.cat([na[na > 0], nb[nb > 0]]).median()
        faint = live & ((na < FAINT_G * med) | (nb < FAINT_G * med))
    left_out = int(faint.sum())
    assert left_out <= MAX_LEFT_OUT, "the condition on the inputs leaves out %d of %d pairs" % (left_out, k)
    keep = ~faint
    return SimpleNamespace(near_index=near[keep].to(torch.int32).contiguous(), shift=shift[keep].contiguous(),
                           coord_a=a[keep].contiguous(), coord_b=b[keep].contiguous(), left_out=left_out,
                           zero_g=int((~live).sum()), n=n)


@functools.lru_cache(maxsize=None)
def case(name):
    """One step fixture with the helper's pairs and its fp64 oracle at WEIGHT_C: computed once, shared, never written to."""
    fx = load_golden(name)
    pairs = pairs_for(fx)
    oct_, mlp = no.wide_oracle(fx)
    wide = consistency_term(oct_, mlp, pairs.coord_a, pairs.coord_b, WEIGHT_C)
    return SimpleNamespace(name=name, fx=fx, coord=fx["coord"], pairs=pairs, wide=wide)


rel_errors = no.rel_errors
