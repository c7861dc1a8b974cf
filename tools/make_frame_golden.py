"""Write tests/golden/frame_sampler.pt: the reference's own dataSampler.sample (utils/data_sampler.py:18-139) on CPU, on stored
points, origins and UNIFORMS, in fp64 and in fp32.

    python tools/make_frame_golden.py            # (re)write the fixture
    python tools/make_frame_golden.py --check    # regenerate in memory, exit 1 unless it is bit-identical to the stored one

Needs the reference checkout (oracle/ref_import.py, read-only).  torch.rand is replaced, for the duration of a call, by a function
that hands out the recorded uniforms in call order (surface, clearance, free space), so the fp64 run, the fp32 run and the device
kernel (shine_ray_sample with injected uniforms) all sample the same points.

The fixture holds recorded inputs and outputs only:
  cases[i]: ns, nc, nf, the sampler constants, scale, points [m,3] f32, origin [3] f32, labels [m] int32 or None,
            uniforms [m * S] f32 in draw order, and the fp64 outputs coord, sdf_label, sample_depth, ray_depth (ray-major),
            weight (int8) and sem_label (int32) — exact values
  e_ref:    per output tensor, the largest distance of the reference's fp32 outputs from its fp64 ones over ALL cases (a one-ray
            case alone can round exactly): the unit of the GPU test's bound (4 x e_ref)
Cases: (ns, nc, nf) = (3, 0, 3), (5, 0, 2) (the class defaults), (3, 2, 3) with labels, (1, 0, 0), and (3, 0, 3) with one ray;
ranges 3-50 m at scale 0.02, origin off zero.  800 rays per multi-sample case: five fp64 words per sample keep the file under the
1 MiB limit of a committed file at that size, not at 2000.
"""
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "frame_sampler.pt")
SCALE = 0.02
CASES = (  # ns, nc, nf, rays, labels, seed
    (3, 0, 3, 800, False, 11),
    (5, 0, 2, 800, False, 12),
    (3, 2, 3, 800, True, 13),
    (1, 0, 0, 2000, False, 14),
    (3, 0, 3, 1, False, 15),
)
CONST = dict(surface_sample_range_m=0.3, free_sample_begin_ratio=0.3, free_sample_end_dist_m=0.8, clearance_dist_m=0.25,
             sigma_sigmoid_m=0.1)
TENSORS = ("coord", "sdf_label", "sample_depth", "ray_depth", "weight")


def _inputs(ns, nc, nf, m, with_labels, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(m, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    rng = 3.0 + 47.0 * torch.rand(m, generator=g, dtype=torch.float64)
    origin = torch.tensor([0.113, -0.071, 0.0191], dtype=torch.float64) + 0.01 * torch.randn(3, generator=g, dtype=torch.float64)
    points = (origin + d * (rng * SCALE)[:, None]).float()
    labels = torch.randint(1, 20, (m,), generator=g, dtype=torch.int32) if with_labels else None
    uniforms = torch.rand(m * (ns + nc + nf), generator=g, dtype=torch.float32)
    return points, origin.float(), labels, uniforms


class _RecordedRand:
    """stands in for torch.rand: hands out the recorded uniforms in call order, in the dtype of the run"""

    def __init__(self, uniforms, dtype):
        self.u, self.dtype, self.at = uniforms, dtype, 0

    def __call__(self, *size, **kw):
        n = 1
        for s in size:
            n *= int(s)
        out = self.u[self.at:self.at + n].to(self.dtype).reshape(*size)
        self.at += n
        return out


def _run(ref, case, dtype):
    ns, nc, nf, m, with_labels, seed = case
    points, origin, labels, uniforms = _inputs(*case)
    cfg = SimpleNamespace(device="cpu", scale=SCALE, surface_sample_n=ns, clearance_sample_n=nc, free_sample_n=nf,
                          behind_dropoff_on=False, **CONST)
    sampler = ref.dataSampler(cfg)
    fake = _RecordedRand(uniforms, dtype)
    real, old_default = torch.rand, torch.get_default_dtype()
    torch.rand = fake
    torch.set_default_dtype(dtype)
    try:
        coord, sdf, _, sem, weight, depth, ray_depth = sampler.sample(
            points.to(dtype), origin.to(dtype), None, labels.to(dtype) if labels is not None else None)
    finally:
        torch.rand = real
        torch.set_default_dtype(old_default)
    assert fake.at == uniforms.numel()
    return dict(coord=coord, sdf_label=sdf, sample_depth=depth, ray_depth=ray_depth, weight=weight, sem_label=sem)


def generate(ref):
    cases, e_ref = [], {k: 0.0 for k in TENSORS}
    for case in CASES:
        ns, nc, nf, m, with_labels, seed = case
        points, origin, labels, uniforms = _inputs(*case)
        r64, r32 = _run(ref, case, torch.float64), _run(ref, case, torch.float32)
        for k in TENSORS:
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64
            e_ref[k] = max(e_ref[k], float((r32[k].double() - r64[k]).abs().max()))
        assert torch.equal(r32["weight"].double(), r64["weight"])
        cases.append(dict(ns=ns, nc=nc, nf=nf, scale=SCALE, points=points, origin=origin, labels=labels, uniforms=uniforms,
                          coord=r64["coord"].contiguous(), sdf_label=r64["sdf_label"].contiguous(),
                          sample_depth=r64["sample_depth"].contiguous(), ray_depth=r64["ray_depth"].contiguous(),
                          weight=r64["weight"].to(torch.int8).contiguous(),
                          sem_label=r64["sem_label"].to(torch.int32).contiguous() if with_labels else None, **CONST))
    return dict(cases=cases, e_ref=e_ref)


def identical(a, b):
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(identical(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(identical(u, v) for u, v in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


def main():
    from oracle import ref_import

    fx = generate(ref_import.install())
    if "--check" in sys.argv:
        stored = torch.load(PATH, map_location="cpu", weights_only=False)
        ok = identical(fx, stored)
        print("identical" if ok else "DIFFERENT")
        sys.exit(0 if ok else 1)
    torch.save(fx, PATH)
    print("wrote", PATH, os.path.getsize(PATH), "bytes;  e_ref", fx["e_ref"])


if __name__ == "__main__":
    main()
