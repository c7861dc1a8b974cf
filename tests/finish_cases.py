"""Cases, fp64 oracle, per-element scales, checkers and mutants for the iteration tail (csrc/shine_finish.hip k_finish) and the
fused Adam (csrc/shine_adam.hip k_adam, which shares adam1 with it).  tests/test_finish.py is the CPU suite, tests/test_gpu_finish.py
the GPU one; the house rule is tests/tier_a_kernel_cases.py's.

The rule.  Every element x of every output (p, exp_avg m, exp_avg_sq v of every tensor, reg_out, loss_parts) is held to

    |x - ref64| <= K * 2^-24 * scale        scale == 0  ->  x == ref64 to the bit,

where ref64 is the fp64 value of what include/shine_hip.h documents for shine_finish_iteration on the fp32 inputs:
g = S.g + sum_b partial_b for the decoder's elements and the trash rows (whose p is taken as 0 before the update, set_zero,
model/feature_octree.py:78-81, and which get no regulariser); on rows flagged with bit 0 and lambda != 0 the value gains
sum w (p - l)^2 and g += 2 lambda w (p - l) unless grad_on[s] == 0; then torch's Adam with L2 weight decay (shine_adam.hip:6-7);
loss_parts as shine_finish.hip's last block writes them.  `scale` is the same expression with every leaf replaced by its
absolute value, to first order:

    scale_g = |S.g| + sum_b |partial_b| + 2 lambda w (|p| + |l|)      scale_gg = scale_g + wd |p|
    scale_m = b1 |m| + (1 - b1) scale_gg                              scale_v = b2 v + (1 - b2) scale_gg^2
    scale_denom = scale_v / (2 sqrt(v_new) bc2)   (0 when v_new == 0)
    scale_step = (lr / bc1) (scale_m / denom + |m_new| scale_denom / denom^2)
    scale_p = |p_old| + scale_step, and scale_step == 0 means p is bit-unchanged
    reg_out: sum w (|p| + |l|)^2                                      loss_parts: sum_b |term|

A scale depends only on its own element.  No element is excluded: gradients and partials are drawn from {0} u +-[2^-10, 2^4), a
warm v is >= 2^-20, half the rows are fresh (m = v = 0), and the oracle asserts that no denormal occurs anywhere in it.

K, one per family (RHO_REF), is not chosen: RHO_REF is the largest ratio the fp32 CPU oracle — torch.optim.Adam(foreach=False) in
fp32 on g = the partials added in block order in fp32, the regulariser composite in fp32 — shows on any case of the family, rounded
up to the next half, and K = 4 max(RHO_REF, 1).  tests/test_finish.py measures them again.

Inputs are a counter-based hash of (seed, element index): the same bits on the CPU and on the device, so the large cases are built
and judged where they run.
"""
import functools
import math
import os
from types import SimpleNamespace

import torch

U24 = 2.0 ** -24
TINY = 2.0 ** -126  # the smallest normal fp32

# the partial vector a workgroup of the fused step leaves (csrc/shine_step_common.hpp:11-14; decoder entries at
# csrc/shine_device.hpp:17-22's MLP_W1 .. MLP_B3)
MLP_PARAMS = 1377
PART_TRASH = MLP_PARAMS  # + s*8 + q
PART_LOSS = 1444         # float index of the doubles {bce sum, count, eikonal sum, n_surf}
PART_STRIDE = 1456
DEC_N = (256, 32, 1024, 32, 32, 1)              # W1, b1, W2, b2, w3, b3
DEC_OFF = (0, 256, 288, 1312, 1344, 1376)       # MLP_W1, MLP_B1, MLP_W2, MLP_B2, MLP_W3, MLP_B3
F = 8
MAX_LEVELS = 8
POISON = -6.0e23  # what must not be read or written


def f32(x):
    """the fp32 neighbour of a Python float, as a Python float"""
    return float(torch.tensor(x, dtype=torch.float32))


B1, B2 = f32(0.9), f32(0.99)
LR_DEV = tuple(f32(0.01 * 0.83 ** k) for k in range(16))  # lr_dev: distinct learning rates


def lr_index(n_tensors):
    """a non-identity map tensor -> entry of lr_dev, injective for n_tensors <= 10"""
    return [(3 * s + 5) % 16 for s in range(n_tensors)]


def bias_corrections(t):
    """(1 - b1^t, sqrt(1 - b2^t)) in fp64 on the host, rounded to fp32 (returned as Python floats)"""
    return f32(1.0 - B1 ** t), f32(math.sqrt(1.0 - B2 ** t))


# ---- the pins: family -> the fp32 CPU oracle's largest ratio over every case of the family (the figure in the comment, one thread),
# rounded up to the next half.  adam_*: elements whose gradient is their own; tail_sum_*: the decoder's elements and the trash rows,
# whose gradient is a sum over the workgroups' partial vectors.
RHO_REF = {
    "adam_m": 4.5,       # 4.005  slots (3.283 on the small cases: rows1x63x64x1000-dense)
    "adam_v": 7.5,       # 7.127  slots (5.832 on the small cases)
    "adam_p": 4.0,       # 3.512  second-pass (3.0002 slots; 2.813 on the small cases: shine_adam_step's sixteen-segments)
    "tail_sum_m": 22.5,  # 22.226 nblocks512: 512 same-sign summands, which the oracle adds one after the other
    "tail_sum_v": 45.5,  # 45.467 nblocks512
    "tail_sum_p": 6.0,   # 5.907  nblocks512
    "reg_value": 2.0,    # 1.745  rows255x1-active
    "loss": 0.5,         # 1.7e-8 nblocks256 (the loss block is fp64 on both sides)
}
K = {fam: 4.0 * max(rho, 1.0) for fam, rho in RHO_REF.items()}


def record(case_id, who, rho):
    """append the ratios of one case to the file FINISH_PARITY_LOG names, if any (profiles/finish_tail_parity.txt is made of these);
    who: "cpu32" (the fp32 CPU oracle) or "hip" (the kernels)"""
    path = os.environ.get("FINISH_PARITY_LOG")
    if path:
        with open(path, "a") as fh:
            for fam in sorted(rho):
                fh.write("%s %s %s %.3f\n" % (case_id, who, fam, rho[fam]))


# -------------------------------------------------------------------------------------------------------------- the inputs
def _s64(x):
    return x - (1 << 64) if x >= (1 << 63) else x


def _mix(idx, seed):
    """splitmix64 of idx + seed in wrapping int64 arithmetic (logical shifts by masking): the same on every device"""
    z = idx * _s64(0x9E3779B97F4A7C15) + _s64((seed * 0xD1B54A32D192ED03) & ((1 << 64) - 1))
    z = (z ^ ((z >> 30) & ((1 << 34) - 1))) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ ((z >> 27) & ((1 << 37) - 1))) * _s64(0x94D049BB133111EB)
    return z ^ ((z >> 31) & ((1 << 33) - 1))


def _bits(seed, n, device):
    return _mix(torch.arange(n, dtype=torch.int64, device=device), seed)


def draw(seed, n, device, zeros=0.25, signed=True, lo=-10, hi=4):
    """fp32 [n]: +-[2^lo, 2^hi) with a uniform exponent and mantissa, a fraction `zeros` of exact zeros"""
    h = _bits(seed, n, device)
    mant = (h & 0x7FFFFF).double() * 2.0 ** -23
    e = ((h >> 23) & 0xFFFF) % (hi - lo) + lo
    x = torch.ldexp(1.0 + mant, e)
    if signed:
        x = torch.where(((h >> 40) & 1) == 1, -x, x)
    if zeros:
        x = torch.where(((h >> 41) & 0xFF) < int(zeros * 256), torch.zeros_like(x), x)
    return x.float()


def uniform(seed, n, device):
    """fp64 [n] in [0, 1)"""
    return ((_bits(seed, n, device) >> 11) & ((1 << 53) - 1)).double() * 2.0 ** -53


def choice(seed, n, device, k):
    """int64 [n] in [0, k)"""
    return ((_bits(seed, n, device) >> 17) & 0xFFFFFF) % k


# ---------------------------------------------------------------------------------------------------------------- the cases
def blocks_n(nblocks, eight_wave=False):
    """(n, kernel_variant high bits) of a step whose fused launch leaves `nblocks` partial vectors: n = 64 B gives B four-wave
    workgroups up to 511, 32752 gives 512, 32768 gives 256 eight-wave ones"""
    if eight_wave:
        assert nblocks == 256
        return 32768
    if nblocks == 512:
        return 32752
    assert 1 <= nblocks <= 511
    return 64 * nblocks


def case(name, rows, dec=True, nblocks=7, eight_wave=False, deterministic=False, mode="none", lam=0.0, grad_off=None, eps=1e-15,
         wd_feat=0.0, wd_dec=1e-7, t=1, reduction_sum=0, eik=0, n_surf=0, family="mixed", seed=1, large=False):
    """mode: "none" (dense, touched = NULL), "dense" (flags, cleared by the launch), "active" (sticky flags, flag 0 = skipped);
    grad_off: a level whose grad_on is 0; family: how the partial vectors' summands relate ("same" sign, "mixed", "exact")"""
    L = len(rows)
    n = 777 if deterministic else blocks_n(nblocks, eight_wave)
    return SimpleNamespace(name=name, rows=tuple(rows), L=L, dec=dec, n_tensors=L + (6 if dec else 0),
                           nblocks=1 if deterministic else nblocks, n=n, variant=0x4000 if deterministic else 0, mode=mode,
                           lam=f32(lam), grad_on=[0 if s == grad_off else 1 for s in range(L)], eps=f32(eps),
                           wd=[f32(wd_feat if s == L - 1 else 0.0) for s in range(L)] + ([f32(wd_dec)] * 6 if dec else []),
                           t=t, reduction_sum=reduction_sum, eik=eik, n_surf=n_surf, family=family, seed=seed, large=large,
                           numel=[(r + 1) * F for r in rows] + (list(DEC_N) if dec else []), weight_e=f32(0.1),
                           inv_n=f32(1.0 / n))


ROWS = ((0,), (1,), (255, 1), (256, 0, 257), (1, 63, 64, 1000))
NBLOCKS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 256, 511, 512)
TS = (1, 2, 10, 1000)


def _cases():
    out = []
    k = 0
    for rows in ROWS:  # levels and rows x flags and modes, the Adam scalars and the loss block spread over them
        for mode in ("none", "dense", "active"):
            k += 1
            out.append(case("rows%s-%s" % ("x".join(map(str, rows)), mode), rows, dec=(k % 4 != 0), nblocks=(7, 9, 2)[k % 3],
                            mode=mode, lam=(0.0, 1000.0, 0.75)[("none", "dense", "active").index(mode)],
                            grad_off=(len(rows) - 1) if k % 2 else None, eps=(1e-15, 1e-8)[k % 2],
                            wd_feat=0.0 if mode == "active" else (0.0, 3e-4)[k % 2], t=TS[k % 4], reduction_sum=k % 2,
                            eik=(1, 1, 0)[k % 3], n_surf=(37, 0, 5)[k % 3], family=("mixed", "same", "exact")[k % 3], seed=k))
    for nb in NBLOCKS:  # the split of the partial sums over the lanes: all four trash units and the decoder's last unit (b3)
        k += 1
        out.append(case("nblocks%d" % nb, ROWS[4], nblocks=nb, family=("exact", "mixed", "same")[k % 3], t=TS[k % 4], eik=1,
                        n_surf=nb, reduction_sum=k % 2, seed=k))
    out.append(case("nblocks256-eight-wave", ROWS[4], nblocks=256, eight_wave=True, family="exact", t=2, eik=1, n_surf=3, seed=k + 1))
    out.append(case("deterministic", ROWS[4], deterministic=True, family="mixed", t=10, seed=k + 2))
    # one row block (213 units): reg_out, which the row blocks add to with fp64 atomics, is then the same bits in every launch
    out.append(case("one-row-block", (100, 50, 60), nblocks=3, mode="active", lam=0.75, t=2, eik=1, n_surf=11, seed=k + 5))
    # lane slots k = 1..3 of the row loop: 1 049 282 units, so the launch has 4096 row blocks and slot 0 ends at unit 1 048 575; a
    # level boundary and a trash row fall in slot 1
    out.append(case("slots", (1_048_570, 9, 700), nblocks=3, mode="active", lam=0.75, grad_off=1, t=10, seed=k + 3, large=True))
    # the second pass of u0 += 4 * stride: the level boundary falls inside slot 3 of pass one, the last ~300 rows and the second
    # trash row in pass two (no regulariser: four tables)
    out.append(case("second-pass", (4_194_299, 300), nblocks=2, mode="none", wd_feat=3e-4, t=2, seed=k + 4, large=True))
    return out


CASES = {c.name: c for c in _cases()}
SMALL = [c.name for c in CASES.values() if not c.large]
# the named small cases of the mutants (tests/test_finish.py)
MUTANT_CASE = "rows1x63x64x1000-dense"    # lambda 1000, every grad_on set, t = 10, flags 0 / 1 / 2
MUTANT_WD = "rows1x63x64x1000-none"       # weight decay 3e-4 on the finest level, t = 2
MUTANT_BLOCKS = "nblocks9"                # nine same-sign partial vectors, eikonal with n_surf = 9 != n


def build(c, device="cpu"):
    """every buffer the launch reads, fp32 / uint8 / fp64 on `device`: p, g, m, v per tensor, last / imp / flags per level (None
    without flags), partials [nblocks, PART_STRIDE] with the loss doubles in place, reg_out0"""
    dev = torch.device(device)
    T = SimpleNamespace(p=[], g=[], m=[], v=[], last=[], imp=[], flags=[], skipped=[])
    exact = c.family == "exact"
    for s, numel in enumerate(c.numel):
        sd = c.seed * 1000 + s * 16
        p = draw(sd + 1, numel, dev, zeros=0.1)
        g = draw(sd + 2, numel, dev)
        m = draw(sd + 3, numel, dev)
        v = draw(sd + 4, numel, dev, zeros=0.0, signed=False, lo=-10, hi=2) ** 2  # >= 2^-20
        if s < c.L:
            rows1 = numel // F
            kind = choice(sd + 5, rows1, dev, 8)  # per row: fresh (m = v = 0) for half of them, a zero gradient row for a quarter
            fresh = (kind < 4)[:, None].expand(rows1, F).reshape(-1)
            zero_g = (kind % 4 == 0)[:, None].expand(rows1, F).reshape(-1)
            m = torch.where(fresh, torch.zeros_like(m), m)
            v = torch.where(fresh, torch.zeros_like(v), v)
            g = torch.where(zero_g, torch.zeros_like(g), g)
            if exact:  # (the trash row's own gradient joins an exactly-summable sum)
                g[-F:] = (choice(sd + 6, F, dev, 1001) - 500).float() / 64.0
            flags = skipped = None
            if c.mode != "none":
                flags = choice(sd + 7, rows1, dev, 3).to(torch.uint8)
                flags[-1] = 0  # (the step's misses go to the partial vectors: it never flags the trash row)
                if c.mode == "active":
                    skipped = flags == 0
                    skipped[-1] = False  # (the trash row is updated whatever its flag says)
                    sk = skipped[:, None].expand(rows1, F).reshape(-1)
                    poison = torch.full_like(p, POISON)
                    p, g, m, v = (torch.where(sk, poison, x) for x in (p, g, m, v))
            T.flags.append(flags)
            T.skipped.append(skipped)
            T.last.append(draw(sd + 8, numel, dev, zeros=0.1) if c.lam != 0.0 else None)
            T.imp.append(draw(sd + 9, numel, dev, zeros=0.2, signed=False) if c.lam != 0.0 else None)
        elif exact:
            g = (choice(sd + 6, numel, dev, 1001) - 500).float() / 64.0
        for k, x in zip("pgmv", (p, g, m, v)):
            getattr(T, k).append(x.contiguous())
    nb = c.nblocks
    part = torch.full((nb, PART_STRIDE), POISON, dtype=torch.float32, device=dev)
    used = MLP_PARAMS + c.L * F
    sd = c.seed * 1000 + 900
    if c.family == "same":
        base = draw(sd, used, dev, zeros=0.1).double()
        part[:, :used] = (base[None, :] * (1.0 + 0.5 * uniform(sd + 1, nb * used, dev).view(nb, used))).float()
    elif c.family == "mixed":
        part[:, :used] = draw(sd, nb * used, dev).view(nb, used)
    else:  # integers / 64, below 2^12 in any partial sum (513 x 500 / 64): exact in every association
        part[:, :used] = ((choice(sd, nb * used, dev, 1001) - 500).float() / 64.0).view(nb, used)
    loss = torch.empty((nb, 4), dtype=torch.float64, device=dev)
    loss[:, 0] = draw(sd + 2, nb, dev, zeros=0.0).double() * (1.0 + uniform(sd + 3, nb, dev) * 2.0 ** -24)
    loss[:, 1] = choice(sd + 4, nb, dev, 4096).double()
    loss[:, 2] = draw(sd + 5, nb, dev, zeros=0.0, signed=False).double() * (1.0 + uniform(sd + 6, nb, dev) * 2.0 ** -24)
    loss[:, 3] = 1e300  # (only workgroup 0 leaves the surface count)
    loss[0, 3] = float(c.n_surf)
    part.view(torch.float64).view(nb, PART_STRIDE // 2)[:, PART_LOSS // 2:PART_LOSS // 2 + 4] = loss
    T.partials = part.contiguous()
    T.reg_out0 = 0.375 if c.lam != 0.0 else 0.0
    return T


# ---------------------------------------------------------------------------------------------------------------- the oracle
MUTANTS = ("last block dropped", "blocks below 8 floor(nblocks / 8) only", "trash row not zeroed", "trash row regularised",
           "bias corrections of step t - 1", "gradient factor lambda", "regulariser on flag-2 rows", "decoupled weight decay",
           "lr_index ignored", "eikonal over n", "row off by one at a level boundary")


def _normal(what, *xs):
    for x in xs:
        a = x.abs()
        assert not bool(((a > 0) & (a < TINY)).any()), "a denormal in the oracle: " + what


def adam64(p, g, m, v, sg, lr, wd, eps, bc1, bc2, decoupled=False):
    """torch's Adam (shine_adam.hip:6-7) on fp64 tensors and the scales of its three outputs; sg: the scale of g"""
    gg = g if decoupled else g + wd * p
    m2 = B1 * m + (1.0 - B1) * gg
    v2 = B2 * v + (1.0 - B2) * gg * gg
    denom = v2.sqrt() / bc2 + eps
    step = (lr / bc1) * (m2 / denom)
    p2 = (p * (1.0 - lr * wd) if decoupled else p) - step
    _normal("adam", gg, (1.0 - B2) * gg * gg, m2, v2, step, p2)
    s_gg = sg + wd * p.abs()
    s_m = B1 * m.abs() + (1.0 - B1) * s_gg
    s_v = B2 * v + (1.0 - B2) * s_gg ** 2
    s_den = torch.where(v2 > 0, s_v / (2.0 * v2.sqrt().clamp_min(1e-300) * bc2), torch.zeros_like(v2))
    s_step = (lr / bc1) * (s_m / denom + m2.abs() * s_den / denom ** 2)
    s_p = torch.where(s_step > 0, p.abs() + s_step, torch.zeros_like(p))
    return dict(p=p2, m=m2, v=v2, sp=s_p, sm=s_m, sv=s_v)


def oracle(c, T, mutant=None, bc=None):
    """bc: the two bias corrections, if not the fp32 ones of step t that the launch reads (tests/test_finish.py compares with
    torch's Adam, which keeps them in fp64).  fp64: per tensor p, m, v (what the launch leaves), their scales sp, sm, sv, `sum` (bool: the element's gradient is a sum of
    partials), g (the grads afterwards, fp32), flags (afterwards); reg, reg_scale; loss [4], loss_scale [4]"""
    assert mutant is None or mutant in MUTANTS
    t = c.t - 1 if mutant == "bias corrections of step t - 1" else c.t
    bc1, bc2 = bias_corrections(t) if bc is None else bc
    lri = list(range(c.n_tensors)) if mutant == "lr_index ignored" else lr_index(c.n_tensors)
    nb = c.nblocks
    if mutant == "last block dropped":
        nb -= 1
    elif mutant == "blocks below 8 floor(nblocks / 8) only":
        nb = 8 * (nb // 8)
    part = T.partials[:nb].double()
    kl = c.lam if mutant == "gradient factor lambda" else 2.0 * c.lam
    out = SimpleNamespace(p=[], m=[], v=[], sp=[], sm=[], sv=[], sum=[], g=[], flags=[])
    reg = torch.zeros((), dtype=torch.float64, device=part.device)
    reg_scale = torch.zeros_like(reg)
    for s in range(c.n_tensors):
        p, g, m, v = (x[s].double() for x in (T.p, T.g, T.m, T.v))
        sg = g.abs()
        is_sum = torch.zeros(p.shape, dtype=torch.bool, device=p.device)
        skipped = None
        if s < c.L:
            trash = slice(p.numel() - F, p.numel())
            if mutant == "row off by one at a level boundary" and p.numel() >= 2 * F:
                trash = slice(p.numel() - 2 * F, p.numel() - F)
            cols = slice(PART_TRASH + s * F, PART_TRASH + s * F + F)
            flags = T.flags[s]
            if c.lam != 0.0:
                on = (flags & 1) == 1
                if mutant == "regulariser on flag-2 rows":
                    on = on | (flags == 2)
                on = on[:, None].expand(-1, F).reshape(-1).clone()
                on[trash] = mutant == "trash row regularised"
                l, w = T.last[s].double(), T.imp[s].double()
                d = torch.where(on, p - l, torch.zeros_like(p))
                _normal("regulariser", w * d * d, kl * w * d)
                reg = reg + (w * d * d).sum()
                reg_scale = reg_scale + torch.where(on, w * (p.abs() + l.abs()) ** 2, torch.zeros_like(p)).sum()
                if c.grad_on[s]:
                    g = g + kl * w * d
                    sg = sg + torch.where(on, kl * w * (p.abs() + l.abs()), torch.zeros_like(p))
            g = g.clone()
            g[trash] += part[:, cols].sum(0)
            sg = sg.clone()
            sg[trash] += part[:, cols].abs().sum(0)
            is_sum[trash] = True
            if mutant != "trash row not zeroed":
                p = p.clone()
                p[trash] = 0.0
            if T.skipped[s] is not None:
                skipped = T.skipped[s][:, None].expand(-1, F).reshape(-1)
            out.flags.append(None if flags is None else
                             torch.where(flags == 0, flags, torch.full_like(flags, 2)) if c.mode == "active" else torch.zeros_like(flags))
        else:
            off = DEC_OFF[s - c.L]
            g = g + part[:, off:off + p.numel()].sum(0)
            sg = sg + part[:, off:off + p.numel()].abs().sum(0)
            is_sum[:] = True
        r = adam64(p, g, m, v, sg, LR_DEV[lri[s]], c.wd[s], c.eps, bc1, bc2, decoupled=mutant == "decoupled weight decay")
        g_after = torch.zeros_like(T.g[s])
        if skipped is not None:  # not read, not written: the poison comes back to the bit
            zero = torch.zeros_like(p)
            for k, src in (("p", T.p), ("m", T.m), ("v", T.v)):
                r[k] = torch.where(skipped, src[s].double(), r[k])
                r["s" + k] = torch.where(skipped, zero, r["s" + k])
            g_after = torch.where(skipped, T.g[s], g_after)
        for k in ("p", "m", "v", "sp", "sm", "sv"):
            getattr(out, k).append(r[k])
        out.sum.append(is_sum)
        out.g.append(g_after)
    out.reg, out.reg_scale = T.reg_out0 + reg, reg_scale
    d = T.partials.view(torch.float64).view(c.nblocks, PART_STRIDE // 2)[:nb, PART_LOSS // 2:PART_LOSS // 2 + 4]
    ls, cs, es = d[:, 0].sum(), d[:, 1].sum(), d[:, 2].sum()
    als, aes = d[:, 0].abs().sum(), d[:, 2].abs().sum()
    ns = int(T.partials.view(torch.float64)[0, PART_LOSS // 2 + 3]) if c.eik else 0
    if mutant == "eikonal over n" and ns > 0:
        ns = c.n
    f = 1.0 if c.reduction_sum else c.inv_n
    bce, eik = ls * f, (es / ns if ns > 0 else torch.zeros_like(es))
    sb, se = als * f, (aes / ns if ns > 0 else torch.zeros_like(es))
    out.loss = torch.stack([bce, eik, cs, bce + c.weight_e * eik])
    out.loss_scale = torch.stack([sb, se, d[:, 1].abs().sum(), sb + c.weight_e * se])
    return out


def oracle32(c, T):
    """The fp32 CPU oracle, in the shape of a launch's results (see check_case): torch.optim.Adam(foreach=False) in fp32 on
    g = S.g + the partials added in block order in fp32, the regulariser composite (oracle/shine_oracle.py cal_regularization:
    sum w (F - F_last)^2 over the rows, differentiated by autograd) in fp32; skipped rows are put back afterwards."""
    lri = lr_index(c.n_tensors)
    params, groups = [], []
    reg = torch.zeros((), dtype=torch.float32)
    for s in range(c.n_tensors):
        p, g = T.p[s].clone(), T.g[s].clone()
        if s < c.L:
            if c.lam != 0.0:
                on = ((T.flags[s] & 1) == 1).clone()
                on[-1] = False
                rows = torch.nonzero(on).flatten()
                q = p.view(-1, F).clone().requires_grad_(True)
                val = (T.imp[s].view(-1, F)[rows] * (q[rows] - T.last[s].view(-1, F)[rows]) ** 2).sum()
                (gr,) = torch.autograd.grad(c.lam * val, q)
                reg = reg + val.detach()
                if c.grad_on[s]:
                    g = g + gr.reshape(-1)
            for b in range(c.nblocks):
                g[-F:] += T.partials[b, PART_TRASH + s * F:PART_TRASH + s * F + F]
            p[-F:] = 0.0
        else:
            off = DEC_OFF[s - c.L]
            for b in range(c.nblocks):
                g += T.partials[b, off:off + p.numel()]
        q = torch.nn.Parameter(p)
        q.grad = g
        params.append(q)
        groups.append({"params": [q], "lr": LR_DEV[lri[s]], "weight_decay": c.wd[s]})
    opt = torch.optim.Adam(groups, betas=(B1, B2), eps=c.eps, foreach=False)
    for s, q in enumerate(params):
        opt.state[q] = {"step": torch.tensor(float(c.t - 1)), "exp_avg": T.m[s].clone(), "exp_avg_sq": T.v[s].clone()}
    with torch.no_grad():
        opt.step()
    got = SimpleNamespace(p=[], m=[], v=[], g=[], flags=None)
    for s, q in enumerate(params):
        st = opt.state[q]
        sk = None if s >= c.L or T.skipped[s] is None else T.skipped[s][:, None].expand(-1, F).reshape(-1)
        for k, new, old in (("p", q.detach(), T.p[s]), ("m", st["exp_avg"], T.m[s]), ("v", st["exp_avg_sq"], T.v[s])):
            getattr(got, k).append(new if sk is None else torch.where(sk, old, new))
        got.g.append(None)
    got.reg = T.reg_out0 + float(reg)
    d = T.partials.view(torch.float64).view(c.nblocks, PART_STRIDE // 2)[:, PART_LOSS // 2:PART_LOSS // 2 + 4]
    ls = cs = es = 0.0
    for b in range(c.nblocks):  # in block order
        ls, cs, es = ls + float(d[b, 0]), cs + float(d[b, 1]), es + float(d[b, 2])
    ns = int(d[0, 3]) if c.eik else 0
    bce = ls if c.reduction_sum else ls * c.inv_n
    eik = es / ns if ns > 0 else 0.0
    got.loss = torch.tensor([bce, eik, cs, bce + c.weight_e * eik], dtype=torch.float64)
    return got


def round32(ref):
    """an oracle's results as a launch would leave them: fp32 tensors (for the mutants)"""
    return SimpleNamespace(p=[x.float() for x in ref.p], m=[x.float() for x in ref.m], v=[x.float() for x in ref.v], g=ref.g,
                           flags=ref.flags, reg=float(ref.reg), loss=ref.loss)


# --------------------------------------------------------------------------------------------------------------- the checkers
def ratios(x, ref, scale):
    """|x - ref64| / (2^-24 scale) per element; where the scale is 0: 0 if x equals ref64 to the bit, infinity otherwise"""
    x = x.detach().double().reshape(ref.shape)
    err = (x - ref).abs()
    inf = torch.full_like(err, float("inf"))
    return torch.where(scale > 0, err / (U24 * scale).clamp_min(1e-300), torch.where(x == ref, torch.zeros_like(err), inf))


def check(what, family, x, ref, scale, mask=None):
    """asserts the rule on every element (of `mask`, if given: the elements of this family) and returns the largest ratio"""
    ref, scale = ref.to(x.device), scale.to(x.device)
    rho = ratios(x, ref, scale)
    bad = ~torch.isfinite(x.detach().double().reshape(ref.shape)) & torch.isfinite(ref)
    rho = torch.where(bad, torch.full_like(rho, float("inf")), rho)
    if mask is not None:
        rho = torch.where(mask.to(x.device), rho, torch.zeros_like(rho))
    worst = float(rho.max()) if rho.numel() else 0.0
    if not worst <= K[family]:
        at = int(rho.flatten().argmax())
        raise AssertionError("%s: element %d is %.3g x 2^-24 scale off (K = %g): got %r, fp64 %r, scale %r"
                             % (what, at, worst, K[family], float(x.detach().double().flatten()[at]), float(ref.flatten()[at]),
                                float(scale.flatten()[at])))
    return worst


def check_case(what, c, got, ref, adam_only=False):
    """Every output of one launch against the oracle `ref` -> {family: rho}.  got: p, m, v (per tensor), g (the grads afterwards,
    or None entries: not judged), flags (per level, or None), reg, loss (fp64 [4], or None: loss_parts was NULL)."""
    rho = {}
    for s in range(len(ref.p)):
        for k in "pmv":
            x = getattr(got, k)[s]
            r, sc = getattr(ref, k)[s], getattr(ref, "s" + k)[s]
            for fam, mask in (("adam_" + k, ~ref.sum[s]), ("tail_sum_" + k, ref.sum[s])):
                if adam_only and fam.startswith("tail"):
                    continue
                w = check("%s: %s of tensor %d" % (what, k, s), fam, x, r, sc, mask)
                rho[fam] = max(rho.get(fam, 0.0), w)
        if got.g[s] is not None:
            assert torch.equal(got.g[s].reshape(-1), ref.g[s].to(got.g[s].device)), \
                "%s: the grads of tensor %d afterwards (0 where processed, untouched where skipped)" % (what, s)
        if got.flags is not None and s < len(ref.flags) and ref.flags[s] is not None:
            assert torch.equal(got.flags[s], ref.flags[s].to(got.flags[s].device)), "%s: the flags of level %d afterwards" % (what, s)
    if adam_only:
        return rho
    one = lambda v: torch.as_tensor(v, dtype=torch.float64).reshape(1).cpu()
    rho["reg_value"] = check(what + ": reg_out", "reg_value", one(got.reg), one(ref.reg), one(ref.reg_scale))
    if got.loss is not None:
        rho["loss"] = check(what + ": loss_parts", "loss", got.loss.cpu(), ref.loss.cpu(), ref.loss_scale.cpu())
    return rho


def _reference(name, device):
    c = CASES[name]
    T = build(c, device)
    return c, T, oracle(c, T)


_small_reference = functools.lru_cache(maxsize=8)(_reference)


def reference(name, device="cpu"):
    """(case, inputs, oracle) of one case on `device`: computed once, shared, never written to.  The large cases (gigabytes) are
    not kept; forget() drops the rest, so that a suite's later tests find the device's memory as they expect it."""
    return (_reference if CASES[name].large else _small_reference)(name, device)


def forget():
    _small_reference.cache_clear()


# ------------------------------------------------------------------------------------------------- shine_adam_step(_dev) cases
ADAM_NUMEL = (5, 0, 1023, 1, 3, 4, 1025)  # mixed in one call, a zero-size tensor between two others
ADAM_BIG = 4 * (1 << 20) + 4 * 100 + 3    # more float4 units than 4096 blocks x 256 lanes: a second grid-stride pass


def adam_case(name, numel, t=1, eps=1e-15, wd=None, flags=(), seed=1):
    """a plain Adam call as a case of the same oracle: no levels, no partial sums.  flags: tensors that are [rows, 8] tables with
    row flags (active rows: flag 0 = skipped)"""
    n = len(numel)
    c = SimpleNamespace(name=name, numel=list(numel), n_tensors=n, t=t, eps=f32(eps), seed=seed, flagged=tuple(flags),
                        wd=[f32(w) for w in (wd if wd is not None else [0.0] * n)])
    return c


def adam_build(c, device="cpu"):
    dev = torch.device(device)
    T = SimpleNamespace(p=[], g=[], m=[], v=[], flags=[], skipped=[])
    for s, numel in enumerate(c.numel):
        sd = c.seed * 1000 + s * 16 + 500
        p, g, m = draw(sd + 1, numel, dev, zeros=0.1), draw(sd + 2, numel, dev), draw(sd + 3, numel, dev)
        v = draw(sd + 4, numel, dev, zeros=0.0, signed=False, lo=-10, hi=2) ** 2
        fresh = choice(sd + 5, (numel + F - 1) // F, dev, 2)[:, None].expand(-1, F).reshape(-1)[:numel] == 0
        m, v = torch.where(fresh, torch.zeros_like(m), m), torch.where(fresh, torch.zeros_like(v), v)
        flags = skipped = None
        if s in c.flagged:
            flags = choice(sd + 7, numel // F, dev, 3).to(torch.uint8)
            skipped = (flags == 0)[:, None].expand(-1, F).reshape(-1)
            p, g, m, v = (torch.where(skipped, torch.full_like(x, POISON), x) for x in (p, g, m, v))
        T.flags.append(flags)
        T.skipped.append(skipped)
        for k, x in zip("pgmv", (p, g, m, v)):
            getattr(T, k).append(x.contiguous())
    return T


def adam_oracle(c, T, lr, zero_grad=1, bc=None):
    """the oracle of one shine_adam_step call with learning rates `lr` (per tensor); bc as for oracle()"""
    bc1, bc2 = bias_corrections(c.t) if bc is None else bc
    out = SimpleNamespace(p=[], m=[], v=[], sp=[], sm=[], sv=[], sum=[], g=[], flags=[])
    for s in range(c.n_tensors):
        p, g, m, v = (x[s].double() for x in (T.p, T.g, T.m, T.v))
        r = adam64(p, g, m, v, g.abs(), lr[s], c.wd[s], c.eps, bc1, bc2)
        g_after = torch.zeros_like(T.g[s]) if zero_grad else T.g[s]
        if T.skipped[s] is not None:
            sk = T.skipped[s]
            for k, src in (("p", T.p), ("m", T.m), ("v", T.v)):
                r[k] = torch.where(sk, src[s].double(), r[k])
                r["s" + k] = torch.where(sk, torch.zeros_like(p), r["s" + k])
            g_after = torch.where(sk, T.g[s], g_after)
        for k in ("p", "m", "v", "sp", "sm", "sv"):
            getattr(out, k).append(r[k])
        out.sum.append(torch.zeros(p.shape, dtype=torch.bool, device=p.device))
        out.g.append(g_after)
        f = T.flags[s]
        out.flags.append(None if f is None else torch.where(f == 0, f, torch.full_like(f, 2)))
    return out


def adam_oracle32(c, T, lr):
    """torch.optim.Adam(foreach=False) in fp32 on the same call"""
    params = []
    groups = []
    for s in range(c.n_tensors):
        q = torch.nn.Parameter(T.p[s].clone())
        q.grad = T.g[s].clone()
        params.append(q)
        groups.append({"params": [q], "lr": lr[s], "weight_decay": c.wd[s]})
    opt = torch.optim.Adam(groups, betas=(B1, B2), eps=c.eps, foreach=False)
    for s, q in enumerate(params):
        opt.state[q] = {"step": torch.tensor(float(c.t - 1)), "exp_avg": T.m[s].clone(), "exp_avg_sq": T.v[s].clone()}
    with torch.no_grad():
        opt.step()
    got = SimpleNamespace(p=[], m=[], v=[], g=[None] * c.n_tensors, flags=None)
    for s, q in enumerate(params):
        st, sk = opt.state[q], T.skipped[s]
        for k, new, old in (("p", q.detach(), T.p[s]), ("m", st["exp_avg"], T.m[s]), ("v", st["exp_avg_sq"], T.v[s])):
            getattr(got, k).append(new if sk is None else torch.where(sk, old, new))
    return got


ADAM_CASES = {c.name: c for c in (
    adam_case("mixed-sizes", ADAM_NUMEL, t=1, wd=[1e-7, 0, 0, 3e-4, 0, 0, 1e-7], seed=41),
    adam_case("one-segment", (1023,), t=2, eps=1e-8, seed=42),
    adam_case("sixteen-segments", tuple(ADAM_NUMEL) * 2 + (8, 16), t=10, eps=1e-8, wd=[0, 1e-7] * 8, seed=43),
    adam_case("row-flags", (8 * 300, 33, 8 * 1, 8 * 129), t=1000, wd=[0, 1e-7, 0, 0], flags=(0, 2, 3), seed=44),
    adam_case("second-pass", (5, ADAM_BIG), t=2, wd=[0, 1e-7], seed=45),
)}
ADAM_SMALL = [n for n in ADAM_CASES if n != "second-pass"]
