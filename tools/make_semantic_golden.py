"""Write tests/golden/semantic.pt: the reference's own semantic decoder (model/decoder.py, Decoder(is_geo_encoder=False):
sem_label_prob / sem_label, :89-101) and torch.nn.NLLLoss (shine_batch.py:202-204) on CPU, with autograd gradients, on stored
inputs.

    python tools/make_semantic_golden.py            # (re)write the fixture
    python tools/make_semantic_golden.py --check    # regenerate in memory, exit 1 unless it is bit-identical to the stored one

Needs the reference checkout (oracle/ref_import.py, read-only).  SemanticKITTI's shape: 8 -> 32 -> 32 -> 21 classes.  Cases:
  std    features at the scale feature_std (0.05) gives, the decoder's own initialisation
  large  features scaled until max |z| is about 100 (log_softmax's max subtraction matters)
  kinks  pre-activations exactly 0 in both hidden layers (a zero row + zero bias; zero feature rows) — ReLU's kink
  ties   two identical nclass_out rows (3 and 7) with a larger bias: exact ties in logp, the first index wins
Labels include 0 (clearance and free space, utils/data_sampler.py:59,70) and 20.  Recorded per case: the inputs, the decoder's
parameters, logp, sem_label, and for sem_label_decimation 1 and 3 the NLL loss and the gradients of the features and of every
parameter (lout's is None: the head never uses it).
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "semantic.pt")
N = 320
CLASSES = 20  # sem_class_count (SemanticKITTI); the head has CLASSES + 1 outputs
PARAM_NAMES = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias", "lout.weight", "lout.bias",
               "nclass_out.weight", "nclass_out.bias")


def _config(ref):
    cfg = ref.SHINEConfig()
    cfg.device = "cpu"
    cfg.sem_class_count = CLASSES
    return cfg


def _case(ref, name, seed):
    torch.manual_seed(seed)
    dec = ref.Decoder(_config(ref), is_geo_encoder=False)
    g = torch.Generator().manual_seed(seed + 1)
    f = torch.randn(N, 8, generator=g) * 0.05
    label = torch.randint(0, CLASSES + 1, (N,), generator=g)
    label[::5] = 0
    label[1::7] = CLASSES
    with torch.no_grad():
        if name == "large":
            f = torch.randn(N, 8, generator=g)
            z = dec.nclass_out(torch.relu(dec.layers[1](torch.relu(dec.layers[0](f)))))
            f = f * (100.0 / float(z.abs().max()))
        elif name == "kinks":
            dec.layers[0].weight[5].zero_()
            dec.layers[0].bias[5] = 0.0
            dec.layers[0].bias[9] = 0.0
            dec.layers[1].weight[12].zero_()
            dec.layers[1].bias[12] = 0.0
            f[::4] = 0.0  # (with b1[9] = 0: pre-activation 9 is exactly 0 on these rows)
        elif name == "ties":
            dec.nclass_out.weight[7] = dec.nclass_out.weight[3]
            dec.nclass_out.bias[3] = 2.0
            dec.nclass_out.bias[7] = 2.0
    params = {k: v.detach().clone() for k, v in dec.named_parameters()}
    with torch.no_grad():
        logp = dec.sem_label_prob(f)
        sem_label = dec.sem_label(f)
    rec = dict(name=name, feat=f.clone(), label=label, params=params, logp=logp, sem_label=sem_label, by_decimation={})
    for d in (1, 3):
        fv = f.clone().requires_grad_(True)
        dec.zero_grad(set_to_none=True)
        pred = dec.sem_label_prob(fv)
        loss = torch.nn.NLLLoss(reduction="mean")(pred[::d, :], label[::d])
        loss.backward()
        grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in dec.named_parameters()}
        rec["by_decimation"][d] = dict(loss=loss.detach(), grad_feat=fv.grad.detach().clone(), grads=grads)
    return rec


def generate(ref):
    torch.set_num_threads(1)
    return {"classes": CLASSES + 1,
            "cases": [_case(ref, name, 100 + 10 * k) for k, name in enumerate(("std", "large", "kinks", "ties"))]}


def reference():
    from oracle import ref_import

    return ref_import.install()


def identical(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(identical(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(identical(u, v) for u, v in zip(a, b))
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return a == b


def main():
    fx = generate(reference())
    if "--check" in sys.argv:
        stored = torch.load(PATH, map_location="cpu", weights_only=False)
        ok = identical(fx, stored)
        print("identical" if ok else "DIFFERENT")
        sys.exit(0 if ok else 1)
    torch.save(fx, PATH)
    print("wrote", PATH)


if __name__ == "__main__":
    main()
