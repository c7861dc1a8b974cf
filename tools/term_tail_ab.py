#!/usr/bin/env python
"""Same bits from two builds of the library: the five term steps (ops.fused_sem_step / _normal_step / _consistency_step / _time_step
/ _ray_step) plus the Tier A shine_sem_backward and shine_interp_backward[_backward], on fixed-seed synthetic inputs at L in
{3, 4}, interpolation polynomial on and off, the decoder training and frozen, the eikonal term on and off where a step has one, at
257 rows and at the 17-workgroup size (4113 rows; 2049 pairs; 43 and 641 rays of 6 samples).  Run under tools/run_with_lib.py
with either library, a process per library:

    python tools/run_with_lib.py tools/ab/lib_parent.so tools/term_tail_ab.py --dump parent_1.pt
    python tools/run_with_lib.py tools/ab/lib_parent.so tools/term_tail_ab.py --dump parent_2.pt
    python tools/run_with_lib.py shine_mapping_amd/lib/libshine_check.so tools/term_tail_ab.py --dump new.pt
    python tools/term_tail_ab.py --compare parent_1.pt new.pt --spread parent_1.pt parent_2.pt

--compare: every deterministic output (losses, decoder / head / sigma_size grads, pred, dpred, grad_feat of shine_sem_backward,
out_x / out_g of the interpolation's backwards) must be torch.equal; the feature-table grads come from fp32 atomics and have no
defined bits: max |new - parent| is printed next to max |parent - parent| of the --spread pair and must not exceed twice that.
Exit status 1 if either fails.

The product builds use hipcc's default -ffp-contract=fast, under which the back end picks per build which multiply-add pairs
become one fma; to compare two commits' ARITHMETIC, build both libraries' sources with the choice taken out
(`python tools/mk_variant.py NAME -ffp-contract=on FILE.hip ...` in each checkout) and compare those."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMIC = "feat_grad/"  # keys of outputs summed by fp32 atomics
S = 6                  # samples per ray


def run_all():
    import torch

    from shine_mapping_amd import Decoder, StepOptions, ops, synth

    out = {}

    def table(grad):  # (a feature table's grad: the touched rows alone)
        return grad.detach().to_sparse().cpu()

    def clear(params):
        for p in params:
            p.grad = None

    def record(key, octree, loss, params, extra=()):
        out[key + "/loss"] = loss.detach().cpu().clone()
        for s, p in enumerate(octree.hier_features):
            out[ATOMIC + key + "/level%d" % s] = table(p.grad)
        for k, p in enumerate(params):
            if p.grad is not None:
                out[key + "/wgrad%d" % k] = p.grad.detach().cpu().clone()
        for name, t in extra:
            out[key + "/" + name] = t.detach().cpu().clone()

    for L in (3, 4):
        for poly in (True, False):
            wl = synth.build_workload("kitti", frames=6, device="cuda", seed=42, tree_level_feat=L, poly_int_on=poly)
            cfg, octree, pl = wl.cfg, wl.octree, wl.pool
            torch.manual_seed(7)
            geo = Decoder(cfg).cuda()
            timed = Decoder(cfg, is_time_conditioned=True).cuda()
            sem = Decoder(cfg, is_geo_encoder=False).cuda()
            gen = torch.Generator(device="cuda").manual_seed(11)
            total = pl.coord.shape[0]
            labels = synth.semantic_labels(pl.coord, pl.weight, cfg.sem_class_count).to(torch.int32).contiguous()
            normal = torch.nn.functional.normalize(torch.randn(total, 3, device="cuda", generator=gen), dim=1)
            ts = torch.randint(0, 6, (total,), device="cuda", generator=gen).float()
            depth = torch.rand(total, device="cuda", generator=gen) * 0.2 + 0.05
            sigma_size = torch.nn.Parameter(torch.ones(1, device="cuda"))
            for n in (257, 4113):
                coord, label, weight = pl.coord[:n].contiguous(), pl.sdf_label[:n].contiguous(), pl.weight[:n].contiguous()
                k_pairs = 257 if n == 257 else 2049
                near = torch.randint(0, n, (k_pairs,), device="cuda", generator=gen).to(torch.int32)
                shift = ((torch.rand(k_pairs, 3, device="cuda", generator=gen) * 2 - 1) * 2.0 ** -12).contiguous()
                rays = 43 if n == 257 else 641
                rcoord, rweight = pl.coord[:rays * S].contiguous(), pl.weight[:rays * S].contiguous()
                rdepth, ray_depth = depth[:rays * S].contiguous(), (depth[:rays] + 0.1).contiguous()
                for frozen in (False, True):
                    for dec in (geo, timed, sem):
                        for p in dec.parameters():
                            p.requires_grad_(not frozen)
                    tag = "L%d/%s/n%d/%s" % (L, "poly" if poly else "linear", n, "frozen" if frozen else "train")
                    every = list(octree.hier_features) + list(geo.parameters()) + list(timed.parameters()) + list(sem.parameters())
                    every.append(sigma_size)

                    clear(every)
                    loss = ops.fused_sem_step(octree, sem, coord, labels[:n].contiguous(), 1.0)
                    record(tag + "/sem", octree, loss, sem.sem_params())
                    clear(every)
                    loss = ops.fused_normal_step(octree, geo, coord, weight, normal[:n].contiguous(), 0.05)
                    record(tag + "/normal", octree, loss, geo.fused_params())
                    clear(every)
                    loss = ops.fused_consistency_step(octree, geo, coord, 0.05, near_index=near, shift=shift)
                    record(tag + "/consistency", octree, loss, geo.fused_params())
                    for eik in (False, True):
                        opts = StepOptions(sigma=cfg.sigma_sigmoid, ekional_loss_on=eik, weight_e=0.1)
                        clear(every)
                        pred = torch.zeros(n, device="cuda")
                        loss = ops.fused_time_step(octree, timed, coord, label, weight, ts[:n].contiguous(), opts, pred_out=pred)
                        record(tag + "/time/eik%d" % eik, octree, loss, timed.time_params(), [("pred", pred)])
                        for neus in (False, True):
                            clear(every)
                            pred, dpred = torch.zeros(rays * S, device="cuda"), torch.zeros(rays * S, device="cuda")
                            loss = ops.fused_ray_step(octree, geo, rcoord, rweight, rdepth, ray_depth, sigma_size, opts, S,
                                                      neus_on=neus, pred_out=pred, dpred_out=dpred)
                            record(tag + "/ray/eik%d/neus%d" % (eik, neus), octree, loss, geo.fused_params() + [sigma_size],
                                   [("pred", pred), ("dpred", dpred)])
                    if frozen:
                        continue
                    # Tier A: shine_sem_backward (grad_feat_out and the head's grads)
                    clear(every)
                    feat = octree.query_feature(coord).detach().requires_grad_(True)
                    logp = sem.sem_label_prob(feat)
                    torch.nn.functional.nll_loss(logp, labels[:n].long()).backward()
                    out[tag + "/sem_backward/grad_feat"] = feat.grad.detach().cpu().clone()
                    for k, p in enumerate(sem.sem_params()):
                        out[tag + "/sem_backward/wgrad%d" % k] = p.grad.detach().cpu().clone()
                    # Tier A: shine_interp_backward (out_x) and shine_interp_backward_backward (out_g)
                    clear(every)
                    x = coord.clone().requires_grad_(True)
                    g = torch.randn(n, 8, device="cuda", generator=gen).requires_grad_(True)
                    gg = torch.randn(n, 3, device="cuda", generator=gen)
                    feat = octree.query_feature(x)
                    (gx,) = torch.autograd.grad(feat, x, g, create_graph=True)
                    out[tag + "/interp_backward/out_x"] = gx.detach().cpu().clone()
                    for s, p in enumerate(octree.hier_features):
                        p.grad = None
                    (gx * gg).sum().backward()
                    out[tag + "/interp_backward_backward/out_g"] = g.grad.detach().cpu().clone()
                    for s, p in enumerate(octree.hier_features):
                        out[ATOMIC + tag + "/interp_backward_backward/level%d" % s] = table(p.grad)
                    clear(every)
                    x = coord.clone().requires_grad_(True)
                    (octree.query_feature(x) * g.detach()).sum().backward()
                    for s, p in enumerate(octree.hier_features):
                        out[ATOMIC + tag + "/interp_backward/level%d" % s] = table(p.grad)
    torch.cuda.synchronize()
    return out


def compare(a_path, b_path, spread):
    import torch

    def load(path):
        d = torch.load(path, weights_only=False)
        return {k: (v.to_dense() if k.startswith(ATOMIC) else v) for k, v in d.items()}

    a, b = load(a_path), load(b_path)
    assert sorted(a) == sorted(b), "the two dumps hold different outputs"
    exact = [k for k in sorted(a) if not k.startswith(ATOMIC)]
    unequal = [k for k in exact if not torch.equal(a[k], b[k])]
    print("deterministic outputs: %d compared, %d not torch.equal" % (len(exact), len(unequal)))
    groups = {}  # (step, output) -> [count, largest difference relative to the tensor's max-abs]
    for k in unequal:
        part = k.split("/")
        step = next(p for p in part if p in ("sem", "normal", "consistency", "time", "ray", "sem_backward", "interp_backward",
                                             "interp_backward_backward"))
        g = groups.setdefault((step, part[-1]), [0, 0.0])
        g[0] += 1
        g[1] = max(g[1], float((a[k].double() - b[k].double()).abs().max()) / max(float(a[k].abs().max()), 1e-300))
    for (step, name), (count, rel) in sorted(groups.items()):
        print("  NOT EQUAL %-12s %-8s in %3d cases, max |a - b| / max |a| = %.3g" % (step, name, count, rel))
    atomic = [k for k in sorted(a) if k.startswith(ATOMIC)]
    diff = max(float((a[k] - b[k]).abs().max()) for k in atomic)
    print("feature-table grads (fp32 atomics): %d tensors, max |new - parent| = %.3g" % (len(atomic), diff))
    ok = not unequal
    if spread:
        p, q = load(spread[0]), load(spread[1])
        own = max(float((p[k] - q[k]).abs().max()) for k in atomic)
        worst = max(atomic, key=lambda k: float((a[k] - b[k]).abs().max()) - 2 * float((p[k] - q[k]).abs().max()))
        print("                                     max |parent - parent| = %.3g (two runs); bound: twice that" % own)
        det = [k for k in exact if not torch.equal(p[k], q[k])]
        print("parent against itself: %d deterministic outputs not torch.equal" % len(det))
        print("largest excess over a tensor's own spread: %s" % worst)
        ok = ok and diff <= 2 * own and not det
    print("RESULT:", "PASS" if ok else "FAIL")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", help="run everything and write the outputs to this .pt")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT.pt", "NEW.pt"))
    ap.add_argument("--spread", nargs=2, metavar=("PARENT_1.pt", "PARENT_2.pt"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.spread))
    import torch

    out = run_all()
    os.makedirs(os.path.dirname(os.path.abspath(a.dump)), exist_ok=True)
    torch.save(out, a.dump)
    print("%d outputs -> %s" % (len(out), a.dump))


if __name__ == "__main__":
    main()
