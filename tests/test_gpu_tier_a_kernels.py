"""GPU suite (-m gpu): the Tier A autograd kernels element by element against fp64 (tests/tier_a_kernel_cases.py has the cases, the
references, the scales, the K of every output family and the checkers; tests/test_tier_a_kernels.py shows on the CPU that they
reject wrong results).

(a) through the C ABI, as OctreeInterpBackward and FusedMLPBackward call it: shine_mlp_forward / _backward / _backward_backward
on every decoder case and size, shine_interp_backward / _backward_backward on every interpolation case, every output of a pass,
and the contracts of include/shine_hip.h (ACCUMULATED INTO, overwritten, untouched biases, NULL outputs, n == 0, refused arguments).
Every output buffer sits between two 256-float guards whose pattern must survive the call.
(b) through the autograd nodes (FusedMLP, OctreeInterp, query_feature, Decoder.sdf): frozen and partly frozen parameters, gradients
that accumulate, strided and fp64 inputs, the double backward with parts of it not wanted, gg_feats, the NotImplementedError.
"""
import ctypes as C
import functools

import pytest
import torch

import step_value_cases as svc
import tier_a_kernel_cases as tc
from conftest import product_from_golden
from test_gpu_scale_parity import node_name

pytestmark = pytest.mark.gpu

GUARD = 256
PATTERN = -6.0e23  # what the guards hold; no kernel here produces it
INVALID = -1       # SHINE_E_INVALID


class Buf:
    """an output buffer of `shape` with GUARD floats of PATTERN either side.  fill: a number, or a CPU tensor (what an ACCUMULATED
    INTO buffer holds before the call); the default NaN is the sentinel of an output that must be overwritten."""

    def __init__(self, shape, fill=float("nan")):
        n = 1
        for s in shape:
            n *= int(s)
        self.flat = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.float32, device="cuda")
        self.t = self.flat[GUARD:GUARD + n].view(*shape)
        if torch.is_tensor(fill):
            self.t.copy_(fill.reshape(self.t.shape))
        else:
            self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def result(self):
        """the buffer's content on the CPU, after checking the guards"""
        flat = self.flat.cpu()
        assert bool((flat[:GUARD] == PATTERN).all()) and bool((flat[-GUARD:] == PATTERN).all()), "a write outside an output buffer"
        return flat[GUARD:-GUARD].view(self.t.shape).clone()


def _stream():
    from shine_mapping_amd import _lib

    return _lib.current_stream_handle()


def _ptrs(items):
    from shine_mapping_amd import _lib

    return _lib.ptr_array([x if (x is None or isinstance(x, int)) else x.ptr() if isinstance(x, Buf) else x.data_ptr()
                           for x in items])


# ------------------------------------------------------------------------------------------------------- (a) the decoder, C ABI


@functools.lru_cache(maxsize=None)
def _dev_params(decoder):
    return [p.cuda().contiguous() for p in tc.decoder_weights(decoder)]


@functools.lru_cache(maxsize=4)
def _dev_inputs(decoder, n):
    case = tc.mlp_case(decoder, n)
    return case.feat.cuda(), case.g.cuda(), case.r.cuda()


def run_mlp(decoder, n, mode, point=True, wgrad=True, v0=None):
    """One call of shine_mlp_forward ("fwd") / _backward ("bwd") / _backward_backward ("bb") on a decoder case.  point / wgrad:
    whether the per-point output / the six weight buffers are passed (else NULL); v0: what the weight buffers hold before.
    -> dict in the shape of tc.mlp_autograd's, None for what was not asked."""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    params = _dev_params(decoder)
    feat, g, r = _dev_inputs(decoder, n)
    mlp = _ptrs(params)
    out = {k: None for k in tc.MLP_POINT + ("gw", "bb")}
    if mode == "fwd":
        pred = Buf((n,))
        _lib.check(lib.shine_mlp_forward(feat.data_ptr(), n, mlp, pred.ptr(), _stream()), "shine_mlp_forward")
        torch.cuda.synchronize()
        out["pred"] = pred.result()
        return out
    key, shape = ("grad_feat", (n, 8)) if mode == "bwd" else ("dg", (n,))
    pt = Buf(shape) if point else None
    gw = [Buf(p.shape, 0.0 if v0 is None else v0[i]) for i, p in enumerate(params)] if wgrad else None
    if mode == "bwd":
        rc = lib.shine_mlp_backward(feat.data_ptr(), g.data_ptr(), n, mlp, pt.ptr() if point else None,
                                    _ptrs(gw) if wgrad else None, _stream())
    else:
        rc = lib.shine_mlp_backward_backward(feat.data_ptr(), g.data_ptr(), r.data_ptr(), n, mlp, pt.ptr() if point else None,
                                             _ptrs(gw) if wgrad else None, _stream())
    _lib.check(rc, "shine_mlp_" + mode)
    torch.cuda.synchronize()
    if point:
        out[key] = pt.result()
        assert not bool(torch.isnan(out[key]).any()), key + ": the sentinel is left in an output that is overwritten"
    if wgrad:
        out["gw" if mode == "bwd" else "bb"] = [b.result() for b in gw]
    return out


MLP_CASES = [(d, n) for d in tc.DECODERS for n in tc.mlp_sizes(d, False)]


@pytest.mark.parametrize("decoder,n", MLP_CASES)
def test_decoder_kernels_hold_every_element_to_its_own_scale(decoder, n):
    """forward, backward and double backward of one decoder case: pred, grad_feat, the six weight sums, d/dg, dW1 / dW2 / dw3 and
    the untouched biases, each element against fp64 within K 2^-24 of its own scale, exact zeros where the scale is zero"""
    case, ref, scale = tc.mlp_reference(decoder, n)
    wgrad = n in tc.mlp_sizes(decoder, True)
    rho = {"mlp_point": 0.0, "mlp_weight": 0.0}
    for mode in ("fwd", "bwd", "bb"):
        got = run_mlp(decoder, n, mode, wgrad=wgrad)
        for fam, v in tc.check_mlp("%s n=%d %s" % (decoder, n, mode), got, ref, scale).items():
            rho[fam] = max(rho[fam], v)
    if decoder == "dead":
        assert bool((got["dg"] == 0).all())
    if case.zero_points.any() and decoder == "on_kink":  # relu'(0) = 0: an exact kink passes nothing
        assert float(run_mlp(decoder, n, "bwd", wgrad=False)["grad_feat"][case.zero_points].abs().max()) == 0.0
    print("rho", decoder, n, rho)
    tc.record("mlp/%s/n=%d" % (decoder, n), rho)


@pytest.mark.parametrize("decoder,n", [("fixture", 65), ("b1_third", 257), ("fixture", 24577)])
def test_decoder_contracts_null_outputs_accumulation_and_biases(decoder, n):
    case, ref, scale = tc.mlp_reference(decoder, n)
    for mode, key, sums in (("bwd", "grad_feat", "gw"), ("bb", "dg", "bb")):
        both = run_mlp(decoder, n, mode)
        # (ptr, NULL): the per-point output is deterministic — the same bits with and without the weight sums
        alone = run_mlp(decoder, n, mode, wgrad=False)
        assert torch.equal(alone[key], both[key]), "%s: %s changes when grad_mlp is NULL" % (mode, key)
        # (NULL, ptr): the sums within their bound
        only = run_mlp(decoder, n, mode, point=False)
        tc.check_mlp("%s with the per-point output NULL" % mode, only, ref, scale)
        # ACCUMULATED INTO: the buffers hold v0 before the call; where nothing is added (dead rows, and in the double backward the
        # three biases) v0 comes back to the bit
        v0 = [tc.prefill(s, 11 * i + n) for i, s in enumerate(scale[sums])]
        acc = run_mlp(decoder, n, mode, v0=v0)
        tc.check_mlp("%s into prefilled buffers" % mode, {sums: acc[sums]}, ref, scale, v0=v0)
        assert torch.equal(acc[key], both[key])
        if mode == "bb":
            for i in (1, 3, 5):
                assert torch.equal(acc["bb"][i], v0[i]), "the double backward moved bias %d" % i
    if decoder == "b1_third":
        assert torch.equal(acc["bb"][0][::3], v0[0][::3])  # the dead units' rows of dW1


def test_decoder_entry_points_accept_empty_calls_and_refuse_bad_arguments():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    n = 65
    params = _dev_params("fixture")
    feat, g, r = _dev_inputs("fixture", n)
    mlp = _ptrs(params)
    gw = [Buf(p.shape, 0.375) for p in params]
    pt = Buf((n, 8), 0.375)
    f, gp, rp, st = feat.data_ptr(), g.data_ptr(), r.data_ptr(), _stream()
    # both outputs NULL, and n == 0 with every buffer given: SHINE_OK, nothing written
    assert lib.shine_mlp_backward(f, gp, n, mlp, None, None, st) == 0
    assert lib.shine_mlp_backward_backward(f, gp, rp, n, mlp, None, None, st) == 0
    assert lib.shine_mlp_forward(f, 0, mlp, pt.ptr(), st) == 0
    assert lib.shine_mlp_backward(f, gp, 0, mlp, pt.ptr(), _ptrs(gw), st) == 0
    assert lib.shine_mlp_backward_backward(f, gp, rp, 0, mlp, pt.ptr(), _ptrs(gw), st) == 0
    # refused on the host, before anything is launched
    assert lib.shine_mlp_forward(f, -1, mlp, pt.ptr(), st) == INVALID
    assert lib.shine_mlp_backward(f, gp, -1, mlp, pt.ptr(), _ptrs(gw), st) == INVALID
    assert lib.shine_mlp_backward_backward(f, gp, rp, -1, mlp, pt.ptr(), _ptrs(gw), st) == INVALID
    holed = _ptrs(params[:2] + [None] + params[3:])
    assert lib.shine_mlp_forward(f, n, holed, pt.ptr(), st) == INVALID
    assert lib.shine_mlp_backward(f, gp, n, holed, pt.ptr(), _ptrs(gw), st) == INVALID
    assert lib.shine_mlp_backward_backward(f, gp, rp, n, holed, pt.ptr(), _ptrs(gw), st) == INVALID
    assert lib.shine_mlp_backward(f, None, n, mlp, pt.ptr(), _ptrs(gw), st) == INVALID
    assert lib.shine_mlp_backward_backward(f, None, rp, n, mlp, pt.ptr(), _ptrs(gw), st) == INVALID
    assert lib.shine_mlp_forward(f, n, mlp, None, st) == INVALID
    torch.cuda.synchronize()
    assert bool((pt.result() == 0.375).all()) and all(bool((b.result() == 0.375).all()) for b in gw)


# ------------------------------------------------------------------------------------------------- (a) the interpolation, C ABI


@functools.lru_cache(maxsize=None)
def _product(name):
    """(cfg, octree, decoder) of a fixture on the device; the tests read its tables and features and never write them"""
    return product_from_golden(svc.fixture(name))


@functools.lru_cache(maxsize=4)
def _interp_inputs(name, batch):
    case = tc.interp_batch(name, batch)
    if batch == "repeat":
        return tc.expand_repeat(case, "cuda")
    return case.coord.cuda(), case.g.cuda(), case.gg.cuda()


def run_interp(name, batch, second, point=True, rows=True, v0=None):
    """One call of shine_interp_backward (second=False) / _backward_backward on an interpolation case.  point: whether
    grad_coord_out / grad_gfeat_out is passed; rows: True (every level), None (a NULL array) or a list of bools (NULL entries);
    v0: what the feature-grad buffers hold before.  -> (per-point output or None, the buffers' contents top-down, None for a
    level that was not passed)"""
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    _, octree, _ = _product(name)
    coord, g, gg = _interp_inputs(name, batch)
    n = coord.shape[0]
    feats = octree.feature_list()
    want = [True] * len(feats) if rows is True else [False] * len(feats) if rows is None else list(rows)
    bufs = [Buf(f.shape, 0.0 if v0 is None else v0[k]) if w else None for k, (f, w) in enumerate(zip(feats, want))]
    pt = Buf((n, 8) if second else (n, 3)) if point else None
    t = octree._require_tables()
    cfg = octree.step_config()
    common = (t.handle, C.byref(cfg), coord.data_ptr(), n, _ptrs(feats), octree.row_counts(), g.data_ptr())
    grads = _ptrs(bufs) if rows is not None else None
    if second:
        rc = lib.shine_interp_backward_backward(*common, gg.data_ptr(), pt.ptr() if point else None, grads, _stream())
    else:
        rc = lib.shine_interp_backward(*common, pt.ptr() if point else None, grads, _stream())
    _lib.check(rc, "shine_interp_backward" + ("_backward" if second else ""))
    torch.cuda.synchronize()
    res = pt.result() if point else None
    if point:
        assert not bool(torch.isnan(res).any()), "the sentinel is left in an output that is overwritten"
    return res, [b.result() if b is not None else None for b in bufs]


INTERP_CASES = [(name, batch) for name in tc.INTERP_FIXTURES for batch in tc.BATCHES]


@pytest.mark.parametrize("name,batch", INTERP_CASES)
def test_interp_kernels_hold_every_element_to_its_own_scale(name, batch):
    """both passes of one interpolation case: grad_coord, d/dg, every feature-grad row and the trash rows, each element against
    fp64 within K 2^-24 of its own scale; rows that no point touches are exactly zero"""
    case, ref, scale = tc.interp_reference(name, batch)
    suffix = "_repeat" if batch == "repeat" else ""
    gc, rows1 = run_interp(name, batch, False)
    dg, rows2 = run_interp(name, batch, True)
    rho = tc.check_interp("%s %s" % (name, batch), dict(grad_coord=gc, dg=dg, rows1=rows1, rows2=rows2), ref, scale, suffix=suffix)
    print("rho", name, batch, rho)
    tc.record("interp/%s/%s" % (name, batch), rho)


@pytest.mark.parametrize("name", tc.INTERP_FIXTURES)
def test_interp_contracts_null_outputs_and_accumulation(name):
    batch = "alternate"  # rows and the trash row both receive something
    case, ref, scale = tc.interp_reference(name, batch)
    L = len(ref["rows1"])
    for second, key, rk in ((False, "grad_coord", "rows1"), (True, "dg", "rows2")):
        both, _ = run_interp(name, batch, second)
        # the per-point output is deterministic: the same bits with a NULL grad_feats array
        alone, none = run_interp(name, batch, second, rows=None)
        assert torch.equal(alone, both) and all(x is None for x in none)
        # the per-point output NULL: the rows within their bound
        _, rows = run_interp(name, batch, second, point=False)
        tc.check_rows("%s with the per-point output NULL" % rk, rows, ref[rk], scale[rk])
        # one NULL entry: that level is skipped, the others are right
        for hole in range(L):
            pt, rows = run_interp(name, batch, second, rows=[k != hole for k in range(L)])
            assert rows[hole] is None and torch.equal(pt, both)
            keep = [k for k in range(L) if k != hole]
            tc.check_rows("%s with level %d NULL" % (rk, hole), [rows[k] for k in keep], [ref[rk][k] for k in keep],
                          [scale[rk][k] for k in keep])
        # ACCUMULATED INTO, the trash row included: rows no point touches keep what they held to the bit
        v0 = [tc.prefill(s, 5 * k + 1) for k, s in enumerate(scale[rk])]
        _, rows = run_interp(name, batch, second, v0=v0)
        tc.check_rows("%s into prefilled buffers" % rk, rows, ref[rk], scale[rk], v0=v0)
        # both outputs NULL: SHINE_OK, nothing to write
        run_interp(name, batch, second, point=False, rows=None)


def test_interp_entry_points_accept_empty_calls_and_refuse_bad_arguments():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    name = "edges_L3"
    _, octree, _ = _product(name)
    coord, g, gg = _interp_inputs(name, "prefix65")
    n = coord.shape[0]
    feats = octree.feature_list()
    bufs = [Buf(f.shape, 0.375) for f in feats]
    pt3, pt8 = Buf((n, 3), 0.375), Buf((n, 8), 0.375)
    t, cfg, st = octree._require_tables(), octree.step_config(), _stream()
    head = (t.handle, C.byref(cfg))
    c, gp, qp, rows, fp, bp = coord.data_ptr(), g.data_ptr(), gg.data_ptr(), octree.row_counts(), _ptrs(feats), _ptrs(bufs)
    assert lib.shine_interp_backward(*head, c, 0, fp, rows, gp, pt3.ptr(), bp, st) == 0
    assert lib.shine_interp_backward_backward(*head, c, 0, fp, rows, gp, qp, pt8.ptr(), bp, st) == 0
    assert lib.shine_interp_backward(*head, c, -1, fp, rows, gp, pt3.ptr(), bp, st) == INVALID
    assert lib.shine_interp_backward_backward(*head, c, -1, fp, rows, gp, qp, pt8.ptr(), bp, st) == INVALID
    holed = _ptrs([None] + list(feats[1:]))
    assert lib.shine_interp_backward(*head, c, n, holed, rows, gp, pt3.ptr(), bp, st) == INVALID
    assert lib.shine_interp_backward_backward(*head, c, n, holed, rows, gp, qp, pt8.ptr(), bp, st) == INVALID
    assert lib.shine_interp_backward(*head, c, n, fp, rows, None, pt3.ptr(), bp, st) == INVALID
    assert lib.shine_interp_backward_backward(*head, c, n, fp, rows, gp, None, pt8.ptr(), bp, st) == INVALID
    assert lib.shine_interp_backward(None, C.byref(cfg), c, n, fp, rows, gp, pt3.ptr(), bp, st) == INVALID
    torch.cuda.synchronize()
    assert all(bool((b.result() == 0.375).all()) for b in bufs + [pt3, pt8])


# ---------------------------------------------------------------------------------------------------------- (b) the autograd nodes

NODE_SIZES = (257, 2048)  # 2048: the fixture's batch


def _decoder(weights="fixture"):
    _, _, dec = product_from_golden(svc.fixture(tc.DECODER_FIXTURE))
    with torch.no_grad():
        for p, w in zip(dec.fused_params(), tc.decoder_weights(weights)):
            p.copy_(w.to(p.device))
    return dec


def _cpu(t):
    return None if t is None else t.detach().cpu()


@pytest.mark.parametrize("n", NODE_SIZES)
def test_fused_mlp_node_first_and_second_backward(n):
    """Decoder.sdf on a leaf: FusedMLP, its backward (FusedMLPBackward) with every gradient, the double backward with d/dg and
    the weight sums — and the NotImplementedError for a function of a weight-grad output"""
    case, ref, scale = tc.mlp_reference("fixture", n)
    dec = _decoder()
    P = dec.fused_params()
    feat = case.feat.cuda().requires_grad_(True)
    g = case.g.cuda().requires_grad_(True)
    pred = dec.sdf(feat)
    assert "FusedMLP" in node_name(pred.grad_fn)
    first = torch.autograd.grad(pred, [feat] + P, g, create_graph=True)
    assert "FusedMLPBackward" in node_name(first[0].grad_fn)
    s = (first[0] * case.r.cuda()).sum()
    second = torch.autograd.grad(s, [g, P[0], P[2], P[4]], retain_graph=True)
    zero = [torch.zeros_like(p) for p in P]
    got = dict(pred=_cpu(pred), grad_feat=_cpu(first[0]), gw=[_cpu(t) for t in first[1:]], dg=_cpu(second[0]),
               bb=[_cpu(second[1]), _cpu(zero[1]), _cpu(second[2]), _cpu(zero[3]), _cpu(second[3]), _cpu(zero[5])])
    tc.check_mlp("FusedMLP n=%d" % n, got, ref, scale)
    for b in (P[1], P[3], P[5]):  # the biases are not in the double backward's graph at all, or get exact zeros
        (gb,) = torch.autograd.grad(s, [b], retain_graph=True, allow_unused=True)
        assert gb is None or float(gb.abs().max()) == 0.0
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(first[1].sum(), [g])


@pytest.mark.parametrize("n", NODE_SIZES)
def test_fused_mlp_node_with_parts_frozen_or_not_wanted(n):
    case, ref, scale = tc.mlp_reference("fixture", n)
    r = case.r.cuda()
    # a frozen decoder: grad_feat and d/dg only, no weight sums wanted in either pass
    dec = _decoder()
    for p in dec.parameters():
        p.requires_grad_(False)
    feat, g = case.feat.cuda().requires_grad_(True), case.g.cuda().requires_grad_(True)
    pred = dec.sdf(feat)
    assert "FusedMLP" in node_name(pred.grad_fn)
    (gf,) = torch.autograd.grad(pred, [feat], g, create_graph=True)
    (dg,) = torch.autograd.grad((gf * r).sum(), [g])
    tc.check_mlp("frozen decoder", dict(pred=_cpu(pred), grad_feat=_cpu(gf), dg=_cpu(dg)), ref, scale)
    # g constant: the double backward is asked for the weight sums alone
    dec = _decoder()
    P = dec.fused_params()
    feat = case.feat.cuda().requires_grad_(True)
    (gf,) = torch.autograd.grad(dec.sdf(feat), [feat], case.g.cuda(), create_graph=True)
    bb = torch.autograd.grad((gf * r).sum(), [P[0], P[2], P[4]])
    z = [torch.zeros_like(p) for p in P]
    tc.check_mlp("g constant", dict(bb=[_cpu(bb[0]), _cpu(z[1]), _cpu(bb[1]), _cpu(z[3]), _cpu(bb[2]), _cpu(z[5])]), ref, scale)
    # only lout trainable, features that do not require grad: .backward() fills lout's grads and nothing else
    dec = _decoder()
    for p in dec.fused_params()[:4]:
        p.requires_grad_(False)
    pred = dec.sdf(case.feat.cuda())
    assert "FusedMLP" in node_name(pred.grad_fn)
    pred.backward(case.g.cuda())
    P = dec.fused_params()
    assert all(p.grad is None for p in P[:4])
    for i in (4, 5):
        tc.check("lout only: gw[%d]" % i, "mlp_weight", P[i].grad, ref["gw"][i], scale["gw"][i])


@pytest.mark.parametrize("n", NODE_SIZES)
def test_fused_mlp_node_accumulates_and_takes_strided_and_fp64_features(n):
    from shine_mapping_amd.autograd_ops import FusedMLP

    case, ref, scale = tc.mlp_reference("fixture", n)
    # gradients add to what .grad holds
    dec = _decoder()
    P = dec.fused_params()
    v0 = [tc.prefill(s, 3 * i + n) for i, s in enumerate(scale["gw"])]
    for p, v in zip(P, v0):
        p.grad = v.reshape(p.shape).cuda()
    dec.sdf(case.feat.cuda()).backward(case.g.cuda())
    tc.check_mlp("into .grad", dict(gw=[_cpu(p.grad) for p in P]), ref, scale, v0=v0)
    # feat as a strided view of a wider tensor: the gradient lands in its columns, the others get zeros
    dec = _decoder()
    big = torch.zeros(n, 16, device="cuda")
    big[:, :8] = case.feat.cuda()
    big[:, 8:] = 7.0
    big.requires_grad_(True)
    pred = dec.sdf(big[:, :8])
    assert "FusedMLP" in node_name(pred.grad_fn)
    pred.backward(case.g.cuda())
    tc.check_mlp("strided", dict(pred=_cpu(pred), grad_feat=_cpu(big.grad[:, :8]), gw=[_cpu(p.grad) for p in dec.fused_params()]),
                 ref, scale)
    assert float(big.grad[:, 8:].abs().max()) == 0.0
    # feat as fp64 (the same values): the node converts, autograd hands back an fp64 gradient
    dec = _decoder()
    f64 = case.feat.double().cuda().requires_grad_(True)
    pred = FusedMLP.apply(f64, *dec.fused_params())
    pred.backward(case.g.cuda())
    assert f64.grad.dtype == torch.float64
    tc.check_mlp("fp64", dict(pred=_cpu(pred), grad_feat=_cpu(f64.grad), gw=[_cpu(p.grad) for p in dec.fused_params()]), ref, scale)


def _interp_setup(name, batch):
    cfg, octree, dec = product_from_golden(svc.fixture(name))
    case, ref, scale = tc.interp_reference(name, batch)
    return octree, dec, case, ref, scale


def _query(octree, coord, python_node):
    from shine_mapping_amd.autograd_ops import OctreeInterp

    if python_node:
        return OctreeInterp.apply(coord, octree, *octree.feature_list())
    return octree.query_feature(coord)


@pytest.mark.parametrize("python_node", [False, True])
@pytest.mark.parametrize("batch", ["prefix257", "whole"])
@pytest.mark.parametrize("name", ["edges_L3", "edges_L2_nopoly_eik"])
def test_interp_node_first_and_second_backward(name, batch, python_node):
    """query_feature (the extension's node where it is built) and OctreeInterp on leaves: backward with every gradient, then the
    double backward with d/dg and the feature rows"""
    octree, dec, case, ref, scale = _interp_setup(name, batch)
    coord = case.coord.cuda().requires_grad_(True)
    g = case.g.cuda().requires_grad_(True)
    F = octree.feature_list()
    feat = _query(octree, coord, python_node)
    assert "Interp" in node_name(feat.grad_fn)
    first = torch.autograd.grad(feat, [coord] + F, g, create_graph=True)
    assert "OctreeInterpBackward" in node_name(first[0].grad_fn)
    second = torch.autograd.grad((first[0] * case.gg.cuda()).sum(), [g] + F)
    got = dict(grad_coord=_cpu(first[0]), rows1=[_cpu(t) for t in first[1:]], dg=_cpu(second[0]), rows2=[_cpu(t) for t in second[1:]])
    tc.check_interp("%s %s node" % (name, batch), got, ref, scale)
    # a driver that touches the feature tensor reaches the split decoder node
    pred = dec.sdf(_query(octree, coord, python_node) * 1.0)
    assert "FusedMLP" in node_name(pred.grad_fn) and "FusedInterpSdf" not in node_name(pred.grad_fn)


@pytest.mark.parametrize("name", ["edges_L3", "edges_L2_nopoly_eik"])
def test_interp_node_with_parts_frozen_and_gradients_that_accumulate(name):
    batch = "prefix257"
    octree, dec, case, ref, scale = _interp_setup(name, batch)
    F = octree.feature_list()
    L = len(F)
    g, gg = case.g.cuda(), case.gg.cuda()
    # features that do not require grad: grad_coord and d/dg alone
    for p in F:
        p.requires_grad_(False)
    coord = case.coord.cuda().requires_grad_(True)
    gl = g.clone().requires_grad_(True)
    (gc,) = torch.autograd.grad(octree.query_feature(coord), [coord], gl, create_graph=True)
    (dg,) = torch.autograd.grad((gc * gg).sum(), [gl])
    tc.check_interp("frozen features", dict(grad_coord=_cpu(gc), dg=_cpu(dg)), ref, scale)
    # one level frozen: it gets nothing, the others their rows, in both passes
    for k, p in enumerate(F):
        p.requires_grad_(k != 0)
    gl = g.clone().requires_grad_(True)
    first = torch.autograd.grad(octree.query_feature(coord), [coord] + F[1:], gl, create_graph=True)
    second = torch.autograd.grad((first[0] * gg).sum(), F[1:])
    tc.check_rows("level 0 frozen: rows1", [_cpu(t) for t in first[1:]], ref["rows1"][1:], scale["rows1"][1:])
    tc.check_rows("level 0 frozen: rows2", [_cpu(t) for t in second], ref["rows2"][1:], scale["rows2"][1:])
    # coord not requiring grad, gradients that add to what .grad holds
    for p in F:
        p.requires_grad_(True)
    v0 = [tc.prefill(s, 13 * k + 2) for k, s in enumerate(scale["rows1"])]
    for p, v in zip(F, v0):
        p.grad = v.cuda()
    octree.query_feature(case.coord.cuda()).backward(g)
    tc.check_rows("into .grad", [_cpu(p.grad) for p in F], ref["rows1"], scale["rows1"], v0=v0)
    assert L == len(ref["rows1"])


@pytest.mark.parametrize("python_node", [False, True])
@pytest.mark.parametrize("name", ["edges_L3", "edges_L2_nopoly_eik"])
def test_interp_backward_differentiates_through_the_feature_grads(name, python_node):
    """OctreeInterpBackward.backward's gg_feats branch: d / d g of sum_l sum grad_F_l . T_l for random tables T_l is
    sum_l interp(T_l), the trash row of T_l included for the points that miss; the tables themselves are not written to"""
    octree, dec, case, ref, scale = _interp_setup(name, "whole")
    F = octree.feature_list()
    gen = torch.Generator().manual_seed(3)
    T = [torch.randn(f.shape, generator=gen) for f in F]
    Td = [t.cuda() for t in T]
    g = case.g.cuda().requires_grad_(True)
    rows = torch.autograd.grad(_query(octree, case.coord.cuda(), python_node), F, g, create_graph=True)
    assert "OctreeInterpBackward" in node_name(rows[0].grad_fn)
    (dg,) = torch.autograd.grad(sum((r * t).sum() for r, t in zip(rows, Td)), [g])
    tc.check("gg_feats", "interp_point", dg, tc.interp_tables(case, T), tc.interp_tables(case, T, absolute=True))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(Td, T)), "the double backward wrote into the incoming gradient tables"
