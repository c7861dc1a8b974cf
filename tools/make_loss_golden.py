"""Write tests/golden/loss_modes.pt: the reference's own sdf_diff_loss and batch_ray_rendering_loss (utils/loss.py:6-14,82-118)
on CPU, with their autograd gradients, on stored inputs.

    python tools/make_loss_golden.py            # (re)write the fixture
    python tools/make_loss_golden.py --check    # regenerate in memory, exit 1 unless it is bit-identical to the stored one

Needs the reference checkout (oracle/ref_import.py, read-only).  Cases:
  ray:  dr and dr_neus at S in {2, 6, 9, 32} — unsorted, distinct depths; rows with saturated probabilities (exact 0 / 1);
        rows whose rendered depth equals the measured one exactly (all-zero alphas, d = 0; one saturated sample, d = its depth)
  sdf:  sdf_l1 and sdf_l2 at two scales — zero differences and zero weights among the points
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "loss_modes.pt")
RAY_S = (2, 6, 9, 32)
RAYS = 48


def _ray_inputs(S, neus, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(RAYS, S)
    for r in range(RAYS):  # distinct depths in a shuffled order
        x[r] = (torch.rand(S, generator=g) * 0.3 + torch.arange(S, dtype=torch.float32) * 0.35 + 0.5)[torch.randperm(S, generator=g)]
    y = torch.sigmoid(torch.randn(RAYS, S, generator=g) * 3.0)
    d_meas = torch.rand(RAYS, generator=g) * S * 0.4 + 0.2
    # saturated probabilities
    y[1, 0] = 1.0
    y[2, S // 2] = 0.0
    y[3, :] = 1.0
    y[4, :] = 0.0
    y[5, S - 1] = 1.0
    y[5, 0] = 0.0
    # d == d_meas exactly: no alpha at all (d = 0) ...
    y[6, :] = 0.0 if not neus else 0.25
    d_meas[6] = 0.0
    # ... and (dr) one certain sample in front of unlikely ones: weight exactly 1 there
    if not neus:
        k = int(torch.argmin(x[7]))
        y[7, :] = 0.0
        y[7, k] = 1.0
        d_meas[7] = x[7, k]
    return x, y, d_meas


def _sdf_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, generator=g) * 0.5
    label = torch.randn(n, generator=g) * 0.5
    weight = torch.rand(n, generator=g) * 2.0
    label[::7] = pred[::7]  # zero differences
    weight[3::11] = 0.0  # zero weights
    return pred, label, weight


def generate(ref_loss):
    torch.set_num_threads(1)
    out = {"ray": [], "sdf": []}
    for neus in (False, True):
        for S in RAY_S:
            x, y, d = _ray_inputs(S, neus, 1000 + 10 * S + int(neus))
            yv = y.clone().requires_grad_(True)
            loss = ref_loss.batch_ray_rendering_loss(x, yv, d, neus_on=neus)
            (gy,) = torch.autograd.grad(loss, yv)
            out["ray"].append(dict(neus=neus, S=S, x=x, y=y, d_meas=d, loss=loss.detach(), grad_y=gy))
    for l2 in (False, True):
        for scale in (0.05, 1.0):
            pred, label, weight = _sdf_inputs(1000, 7 + int(l2) + int(10 * scale))
            pv = pred.clone().requires_grad_(True)
            loss = ref_loss.sdf_diff_loss(pv, label, weight, scale, l2_loss=l2)
            (gp,) = torch.autograd.grad(loss, pv)
            out["sdf"].append(dict(l2=l2, scale=scale, pred=pred, label=label, weight=weight, loss=loss.detach(), grad_pred=gp))
    return out


def reference_loss_module():
    from oracle import ref_import

    ref_import.install()
    import utils.loss as ref_loss

    return ref_loss


def identical(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(identical(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(identical(u, v) for u, v in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


def main():
    fx = generate(reference_loss_module())
    if "--check" in sys.argv:
        stored = torch.load(PATH, map_location="cpu", weights_only=False)
        ok = identical(fx, stored)
        print("identical" if ok else "DIFFERENT")
        sys.exit(0 if ok else 1)
    torch.save(fx, PATH)
    print("wrote", PATH)


if __name__ == "__main__":
    main()
