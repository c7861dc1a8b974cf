"""GPU suite (-m gpu): cfg->draw_rider in the TRAILING WORKGROUPS OF THE FUSED LAUNCH (include/shine_hip.h shine_draw_rider with
idx_next; csrc/shine_draw_rider.hpp, k_step_v3's entry branch).  The rider — pass 2 of the next draw, pass 1 of the one after,
the zero-fill of the other gradient bucket — runs BESIDE the step it rides on, so everything that step reads must stay what it
was until the step is done: its sample indices (the rider draws into a shadow buffer, the reduction launch copies), its own
bucket, its surface count.  Every shape runs twice: the product's launch geometry (several step workgroups, the trailing ones
placed as those retire or, on a part-filled chip, at once beside them) and the single-wave deterministic launch
(kernel_variant | 0x4000: ONE step workgroup runs long while every trailing workgroup runs beside it from the start), where the
step's results are compared bit for bit with a plain step on the same batch.

Nothing here is a tolerance: every comparison is an equality (the draws are the stand-alone sampler's arithmetic and summation
order; the deterministic launch fixes the order of the feature-grad atomics)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SID0 = 40
STEPS = 4  # chained steps per pass: both parities twice
_CACHE = {}


def _setup(levels):
    """the small synthetic map + its sorted pool, built once per level count and left unchanged"""
    if levels not in _CACHE:
        from shine_mapping_amd import synth
        from shine_mapping_amd.sampler import SortedPool

        wl = synth.build_workload("maicity", frames=8, device="cuda", seed=21, tree_level_feat=levels, azimuths=300)
        with torch.no_grad():  # features x5: gradients through the ReLUs that are far from the 0.05-randn noise floor
            for p in wl.octree.hier_features:
                p.mul_(5.0)
        wl.octree._require_tables(with_ranks=True)
        sp = SortedPool(wl.octree, wl.pool.coord, wl.pool.sdf_label, wl.pool.weight, seed=11)
        _CACHE[levels] = (wl, sp)
    return _CACHE[levels]


def _buckets(params, n_levels_feat, pad16):
    """three flat gradient buckets (two alternate under the chain, one for the plain reference step) of total size + pad16 x 16 bytes,
    and the per-parameter views of each"""
    total = sum(p.numel() for p in params)
    size = (total + 3) // 4 * 4 + 4 * pad16
    flats = [torch.zeros(size, dtype=torch.float32, device="cuda") for _ in range(3)]

    def views(flat):
        out, off = [], 0
        for p in params:
            out.append(flat[off: off + p.numel()].view_as(p))
            off += p.numel()
        return out[:n_levels_feat], out[n_levels_feat:]

    return flats, [views(f) for f in flats]


def _rider_stride_bytes(n, det):
    """bytes one sweep of the trailing workgroups' zero-fill covers: 2 * ceil(sampler blocks / Q) workgroups of Q * 256 threads,
    16 bytes per thread (Q = 2 for the 8-wave step workgroups, 1 for the 4-wave ones — below 2048 tiles and the deterministic launch)"""
    nb = (n + 1 + 1023) // 1024
    q = 2 if (not det and (n + 15) // 16 >= 2048) else 1
    return 2 * ((nb + q - 1) // q) * q * 256 * 16


# n = 16 385: just above the size at which benchlib chains draws; 4-wave workgroups on a part of the chip.  32 769: the first 8-wave
# geometry (2049 tiles).  3 071 / 3 072: n + 1 spacings land on / just past a sampler-block boundary (3 blocks / 4).
# odd: a bucket whose byte size is no multiple of the rider's zero-fill stride (asserted below).  tail = False: the record built by
# hand WITHOUT idx_next — the rider on the reduction launch, as before the field existed.
CASES = [(n, levels, levels == 3, True, False) for levels in (3, 4) for n in (16385, 32768 + 1, 3 * 1024 - 1, 3 * 1024)]
CASES += [(3 * 1024 - 1, 3, False, True, True)]
CASES += [(16385, 4, False, False, False), (3 * 1024, 3, True, False, False)]


@pytest.mark.parametrize("n,levels,eik,tail,odd", CASES)
def test_next_draw_in_the_fused_launchs_trailing_workgroups(n, levels, eik, tail, odd):
    from shine_mapping_amd import StepOptions, fused_train_step

    wl, sp = _setup(levels)
    octree, dec, cfg = wl.octree, wl.decoder, wl.cfg
    params = list(octree.hier_features) + dec.fused_params()
    nf = len(octree.hier_features)
    flats, views = _buckets(params, nf, 1 if odd else 0)
    if odd:
        for det in (False, True):
            assert (flats[0].numel() * 4) % _rider_stride_bytes(n, det) != 0
    # the stand-alone sampler's draws of the same seed and stream ids (and their surface counts), once for both passes
    want_idx, want_surf = [], []
    for k in range(2 * 3 + 1):  # (the graph pass below runs 6 steps)
        sp.draws = SID0 + k
        idx = sp.draw(n).clone()
        want_idx.append(idx)
        want_surf.append(int((sp.weight[idx.long()] > 0).sum()))
    idx_buf = torch.empty(n, dtype=torch.int32, device="cuda")
    chain = sp.draw_chain(n, idx_buf, buckets=(flats[0], flats[1]), surf=eik)
    if not tail:
        for r in chain.rider:
            r.idx_next = None

    def run_pass(det, steps, record):
        """`steps` chained steps from a primed chain: -> per step what it read, what it returned and what it left"""
        opts = StepOptions(sigma=cfg.sigma_sigmoid, ekional_loss_on=eik, weight_e=cfg.weight_e, deterministic=det)
        for k in range(steps):
            p = k & 1
            o = copy.copy(opts)
            o.draw_rider = chain.rider[p]
            used = idx_buf.clone()
            surf_before = chain.surf_parts[p].sum().clone() if eik else None
            loss, pred, _ = fused_train_step(octree, dec, None, None, None, o, n_surf=chain.surf_parts[p] if eik else None, pool=sp,
                                             idx=idx_buf, grad_buffers=views[p])
            record.append(dict(used=used, surf_before=surf_before, loss=loss.clone(), pred=pred, own=flats[p].clone(),
                               other=flats[1 - p].abs().max().clone(), idx_after=idx_buf.clone(),
                               shadow=chain.idx_next.clone(),
                               parts_this=chain.surf_parts[p].clone() if eik else None,
                               parts_next=chain.surf_parts[1 - p].sum().clone() if eik else None))

    def prime():
        flats[0].zero_()
        flats[1].fill_(3.0)  # (dirty: step 0 must clear it before step 1 accumulates)
        chain.idx_next.fill_(-1)
        chain.prime(SID0)

    def check_draws(record, first=0):
        for j, r in enumerate(record):
            k = first + j
            # 1. bit-identical draws: what the step read, what it left for the next one, and the surface counts
            assert torch.equal(r["used"], want_idx[k]), "batch of step %d" % k
            assert torch.equal(r["idx_after"], want_idx[k + 1]), "batch left by step %d" % k
            if eik:
                assert int(r["surf_before"]) == want_surf[k], "surface count of step %d" % k
                assert int(r["parts_next"]) == want_surf[k + 1], "surface count left by step %d" % k
                assert int(r["parts_this"].abs().max()) == 0, "step %d's own count is cleared behind it" % k
            # 3. the other bucket is clean
            assert float(r["other"]) == 0.0, "the next step's bucket is not clean after step %d" % k
            # which launch ran the rider: the trailing workgroups draw into the shadow, the reduction launch's rider never touches it
            if tail:
                assert torch.equal(r["shadow"], want_idx[k + 1]), "step %d did not draw into idx_next" % k
            else:
                assert int((r["shadow"] != -1).sum()) == 0, "step %d wrote idx_next of a record that has none" % k

    for det in (False, True):
        rec = []
        prime()
        run_pass(det, STEPS, rec)
        torch.cuda.synchronize()
        check_draws(rec)
        # 2. unchanged results: the same step without a rider, on the same batch and a zeroed bucket
        plain = StepOptions(sigma=cfg.sigma_sigmoid, ekional_loss_on=eik, weight_e=cfg.weight_e, deterministic=det)
        for k, r in enumerate(rec):
            flats[2].zero_()
            loss, pred, _ = fused_train_step(octree, dec, None, None, None, plain, pool=sp, idx=want_idx[k], grad_buffers=views[2])
            torch.cuda.synchronize()
            assert torch.equal(pred, r["pred"]), "pred of step %d (deterministic=%s)" % (k, det)
            if det:  # (the product geometry's feature-grad atomics arrive in no fixed order: bit-equality is the single wave's)
                assert float(loss) == float(r["loss"]), "loss of step %d" % k
                assert torch.equal(flats[2], r["own"]), "gradients of step %d" % k

    # 4. graph replay: 2 steps per graph, 3 replays -> the same sequence of batches as eagerly
    prime()
    torch.cuda.synchronize()
    rec_g = []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run_pass(False, 2, rec_g)
    for rep in range(3):
        g.replay()
        torch.cuda.synchronize()
        check_draws(rec_g, first=2 * rep)
