"""Record the reference's own answers for the CPU tests that hold the oracle and the product to the reference's functions
(tests/test_oracle.py), so that those tests run from the repository alone.

TEST INFRASTRUCTURE ONLY.  Run in the authoring container (needs the reference checkout, oracle/ref_import.py):

    python -m oracle.make_reference_checks     # writes tests/golden/{live_check,reference_checks,reference_importance}.pt.xz

Every value below is computed by the reference's unmodified code on fixed inputs; the inputs are stored next to it.
live_check is one more make_golden case (make_golden.run_case asserts the oracle bit-identical to the reference while
writing it), stored with the feature rows its batch does not read set to zero.  The files are torch.save streams,
lzma-compressed (save_xz / load_xz): most of what they hold is zeros and small integers.
"""
import io
import lzma
import os
import sys
import tempfile

import torch

from . import make_golden as mg
from . import ref_import
from . import shine_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE_SPEC = dict(cfg=dict(tree_level_world=11, tree_level_feat=3, leaf_vox_size=0.25, sigma_sigmoid_m=0.07,
                          ekional_loss_on=True, weight_e=0.2), n=512, decoder="pretrained", gain=5.0)
BCE_SIGMA = 0.0123
SWEEP_CASES = [("mean", 100, 3, 1001), ("sum", 4096, 1, 700), ("mean", 64, 2, 1024)]
OPT_RATIOS = [1.0, 0.5]
CKPT_POINTS = 1000  # surface points per frame of the pickled reference octree (the first ones of maicity_bce_L3's scans)


def save_xz(obj, name):
    buf = io.BytesIO()
    torch.save(obj, buf)
    path = os.path.join(mg.GOLDEN_DIR, name + ".pt.xz")
    with open(path, "wb") as f:
        f.write(lzma.compress(buf.getvalue(), preset=9 | lzma.PRESET_EXTREME))
    print("-> %s (%.0f kB)" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))


def load_xz(name):
    with open(os.path.join(mg.GOLDEN_DIR, name + ".pt.xz"), "rb") as f:
        return torch.load(io.BytesIO(lzma.decompress(f.read())), map_location="cpu", weights_only=False)


def _live_case(R, oracle_from_golden):
    """make_golden.run_case on LIVE_SPEC; then every feature row the batch does not read (its corners' ids, plus the trash
    row) is set to zero — the case's outputs do not depend on them, which is checked here to the bit"""
    old = mg.GOLDEN_DIR
    with tempfile.TemporaryDirectory() as d:
        mg.GOLDEN_DIR = d
        try:
            mg.run_case(R, "live_check", LIVE_SPEC)
            fx = torch.load(os.path.join(d, "live_check.pt"), weights_only=False)
        finally:
            mg.GOLDEN_DIR = old
    L = len(fx["features"])
    for s, f in enumerate(fx["features"]):
        keep = torch.zeros(f.shape[0], dtype=torch.bool)
        ids = fx["out"]["indices"][L - 1 - s].reshape(-1)  # (hierarchical_indices: finest level first)
        keep[ids[ids >= 0]] = True
        keep[-1] = True
        f[~keep] = 0.0
    cfg, oct_, mlp = oracle_from_golden(fx)
    out = so.train_step(oct_, mlp, fx["coord"], fx["sdf_label"], fx["weight"], cfg)
    ref = fx["out"]
    for key in ("pred", "feat", "loss", "g"):
        assert torch.equal(out[key], ref[key]), key
    for a, b in zip(out["feat_grads"] + out["mlp_grads"] + out["indices"], ref["feat_grads"] + ref["mlp_grads"] + ref["indices"]):
        assert torch.equal(a, b)
    return fx


def _weighted_bce(R):
    torch.manual_seed(3)
    pred = 3.0 * torch.randn(777)
    label = 0.05 * torch.randn(777)
    w = torch.rand(777) + 0.1
    out = dict(pred=pred, label=label, weight=w, sigma=BCE_SIGMA)
    for red in ("mean", "sum"):
        p = pred.clone().requires_grad_(True)
        loss = R.sdf_bce_loss(p, label, BCE_SIGMA, w, True, red)
        (g,) = torch.autograd.grad(loss, p)
        out[red] = dict(loss=loss.detach().clone(), grad=g)
    return out


def _importance_sweeps(R, load_golden, oracle_from_golden):
    import copy

    torch.set_num_threads(1)
    fx = load_golden("ncd_reg_L3")
    out = {}
    for reduction, bs, down_rate, take in SWEEP_CASES:
        ocfg, oct_, mlp = oracle_from_golden(fx)
        ocfg = copy.copy(ocfg)
        ocfg.loss_reduction = reduction
        coord, label = fx["coord"][:take].contiguous(), fx["sdf_label"][:take].contiguous()
        for t in oct_.importance_weight:
            t.zero_()
        data = type("Pool", (), {"coord_pool": coord, "sdf_label_pool": label})()
        decoder = type("Callable", (), {"__call__": lambda self, f: mlp.sdf(f)})()
        R.cal_feature_importance(data, oct_, decoder, so.sigma_sigmoid(ocfg), bs, down_rate, reduction)
        out[(reduction, bs, down_rate, take)] = [t.clone() for t in oct_.importance_weight]
    return out


def _optimizer_groups(R, load_golden, oracle_from_golden):
    """the reference's setup_optimizer groups, parameters named by their position in features + decoder params"""
    fx = load_golden("ncd_reg_L3")
    out = {}
    for ratio in OPT_RATIOS:
        ocfg, oct_, mlp = oracle_from_golden(fx)
        cfg = type("Cfg", (), dict(lr=0.01, weight_decay=1e-7, semantic_on=False, ray_loss=False, opt_adam=True,
                                   adam_eps=1e-15, lr_level_reduce_ratio=ratio, tree_level_feat=ocfg.tree_level_feat))()
        feats = list(oct_.hier_features)
        params = feats + list(mlp.params())
        pos = {id(p): i for i, p in enumerate(params)}
        opt = R.setup_optimizer(cfg, feats, mlp.params(), None, None)
        out[ratio] = dict(groups=[dict(params=[pos[id(p)] for p in g["params"]], lr=g["lr"],
                                       weight_decay=g.get("weight_decay", 0)) for g in opt.param_groups],
                          betas=tuple(opt.param_groups[0]["betas"]), eps=opt.param_groups[0]["eps"])
    return out


def _decoder_and_losses(R):
    from model.decoder import Decoder as RefDecoder  # (ref_import put the reference on sys.path)

    from shine_mapping_amd import synth

    cfg = synth.make_config("maicity", device="cpu")
    torch.manual_seed(0)
    ref = RefDecoder(cfg)
    shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    sd = torch.load(os.path.join(ref_import.REFERENCE_ROOT, "pretrained", "geo_decoder_8dim.pth"), map_location="cpu")
    sd = sd.get("geo_decoder", sd) if isinstance(sd, dict) else sd
    sd = {k: v.clone() for k, v in sd.items()}
    ref.load_state_dict(sd)
    f = torch.randn(257, 8)
    label, w = 0.05 * torch.randn(257), torch.rand(257) + 0.1
    fr = f.clone().requires_grad_(True)
    b = ref.sdf(fr)
    losses = {(weighted, red): R.sdf_bce_loss(b, label, BCE_SIGMA, w, weighted, red).detach().clone()
              for weighted in (False, True) for red in ("mean", "sum")}
    g = R.get_gradient(fr, b)
    return dict(state_shapes=shapes, state_dict=sd, feat=f, label=label, weight=w, sigma=BCE_SIGMA,
                sdf=b.detach().clone(), losses=losses, get_gradient=g.detach().clone())


def _pickled_octree(R, load_golden):
    """utils/tools.py:200-213's checkpoint of the reference's FeatureOctree (torch.save bytes) and the tables it holds"""
    fx = load_golden("maicity_bce_L3")
    cfg = R.SHINEConfig()
    for k, v in fx["cfg"].items():
        setattr(cfg, k, v)
    cfg.device = "cpu"
    cfg.calculate_world_scale() if hasattr(cfg, "calculate_world_scale") else None
    ref_oct = R.FeatureOctree(cfg)
    for sp in fx["surface_points"]:
        ref_oct.update(sp[:CKPT_POINTS].contiguous(), True)
    buf = io.BytesIO()
    torch.save({"feature_octree": ref_oct}, buf)
    return dict(checkpoint=buf.getvalue(), free_level_num=int(ref_oct.free_level_num), tables=mg.tables_of(ref_oct),
                rows=[int(p.shape[0]) for p in ref_oct.hier_features])


def main():
    R = ref_import.install()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_golden, oracle_from_golden

    torch.set_num_threads(1)
    prov = "reference executed on CPU by oracle/make_reference_checks.py, torch %s" % torch.__version__
    save_xz(_live_case(R, oracle_from_golden), "live_check")
    save_xz(dict(
        weighted_bce=_weighted_bce(R),
        optimizer_groups=_optimizer_groups(R, load_golden, oracle_from_golden),
        decoder=_decoder_and_losses(R),
        pickled_octree=_pickled_octree(R, load_golden),
        provenance=prov,
    ), "reference_checks")
    save_xz(dict(importance_sweep=_importance_sweeps(R, load_golden, oracle_from_golden), provenance=prov),
            "reference_importance")


if __name__ == "__main__":
    main()
