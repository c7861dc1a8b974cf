"""utils/loss.py:6-24,82-118 and utils/tools.py:175-185 under their reference names (Tier A, the strict drop-in).

`sdf_bce_loss` is ONE HIP launch that returns the loss and keeps d loss / d pred for its backward (the torch composite is a
sigmoid, a BCEWithLogits and their two backward launches); `get_gradient` on the output of the fused query_feature -> sdf node
is ONE launch of the forward kernel's closed-form d pred / d coord build, linked to that node so that the eikonal term's
backward joins the node's one fused launch (autograd_ops.InterpSdfGradCoord).  Anything else — CPU tensors, other dtypes,
other reductions, a pred that did not come from the fused node — runs the reference's torch composite, same results.

`sdf_diff_loss` (main_loss_type sdf_l1 / sdf_l2) and `batch_ray_rendering_loss` (ray_loss with dr / dr_neus) are ONE launch
each as well (csrc/shine_loss_modes.hip): the loss and d loss / d pred (d loss / d y for the rays) — where the composite runs a
sort, a gather, a cumprod and a dozen elementwise launches forward and more backward.  They take the HIP path for CUDA float32
inputs of the reference's shapes whose targets (label, weight, depths) need no gradient, with at most 32 samples per ray.
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd import grad

from . import _ext, _lib
from .autograd_ops import InterpSdfGradCoord


class _SdfBce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, weight, sigma, reduction_sum):
        p = pred.detach()
        l = label.detach()
        l = l if (l.dtype == torch.float32 and l.is_contiguous()) else l.contiguous().float()
        p = p if p.is_contiguous() else p.contiguous()
        w = None
        if weight is not None:
            w = weight.detach()
            w = w if (w.dtype == torch.float32 and w.is_contiguous()) else w.contiguous().float()
        n = p.shape[0]
        out = torch.empty(n + 1, dtype=torch.float32, device=p.device)  # [d loss / d pred (n) | loss]
        _lib.check(_lib.lib().shine_bce_loss(p.data_ptr(), l.data_ptr(), w.data_ptr() if w is not None else None, n, float(sigma),
                                             1 if reduction_sum else 0, out[n:].data_ptr(), out.data_ptr(),
                                             _lib.current_stream_handle()), "shine_bce_loss")
        ctx.dpred = out[:n]
        return out[n]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return ctx.dpred * g, None, None, None, None


def _bce_composite(pred, label, sigma, weight, weighted, bce_reduction):
    loss_bce = nn.BCEWithLogitsLoss(reduction=bce_reduction, weight=weight if weighted else None)
    return loss_bce(pred, torch.sigmoid(label / sigma))


def sdf_bce_loss(pred, label, sigma, weight, weighted=False, bce_reduction="mean"):
    """utils/loss.py:17-24"""
    w = weight if weighted else None
    if (pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 1 and pred.shape[0] > 0 and label.shape == pred.shape
            and label.device == pred.device and bce_reduction in ("mean", "sum") and not isinstance(sigma, torch.Tensor)
            and (w is None or (w.shape == pred.shape and w.device == pred.device)) and not label.requires_grad):
        ext = _ext.module()
        if ext is not None:  # the C++ node (csrc/shine_torch_ext.cpp)
            return ext.bce_loss(pred, label, w, float(sigma), bce_reduction == "sum")
        return _SdfBce.apply(pred, label, w, float(sigma), bce_reduction == "sum")
    return _bce_composite(pred, label, sigma, weight, weighted, bce_reduction)


def loss_workspace(device):
    """the workspace of shine_sdf_diff_loss / shine_ray_render_loss for the current stream of `device`"""
    return _lib.ticket_workspace(device, LOSS_WORKSPACE_BYTES)


LOSS_WORKSPACE_BYTES = 16384  # include/shine_hip.h SHINE_LOSS_WORKSPACE_BYTES
RAY_MAX_SAMPLES = 32  # SHINE_RAY_MAX_SAMPLES


class _SdfDiff(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, weight, scale, l2_loss, ws):
        p, l, w = pred.detach().contiguous(), label.detach().contiguous(), weight.detach().contiguous()
        n = p.shape[0]
        out = torch.empty(n + 1, dtype=torch.float32, device=p.device)  # [d loss / d pred (n) | loss]
        _lib.check(_lib.lib().shine_sdf_diff_loss(p.data_ptr(), l.data_ptr(), w.data_ptr(), n, float(scale), 1 if l2_loss else 0,
                                                  out[n:].data_ptr(), out.data_ptr(), ws.data_ptr(), _lib.current_stream_handle()),
                   "shine_sdf_diff_loss")
        ctx.dpred = out[:n]
        return out[n]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return ctx.dpred * g, None, None, None, None, None


class _RayRender(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, d_meas, neus_on, ws):
        xc, yc, dc = x.detach().contiguous(), y.detach().contiguous(), d_meas.detach().contiguous()
        r, s = yc.shape
        out = torch.empty(r * s + 1, dtype=torch.float32, device=yc.device)  # [d loss / d y (r * s) | loss]
        _lib.check(_lib.lib().shine_ray_render_loss(xc.data_ptr(), yc.data_ptr(), dc.data_ptr(), r, s, 1 if neus_on else 0,
                                                    out[r * s:].data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                    _lib.current_stream_handle()),
                   "shine_ray_render_loss")
        ctx.dy = out[:r * s].view(r, s)
        return out[r * s]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return None, ctx.dy * g, None, None, None


def _f32_cuda_like(t, ref):
    return isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == ref.device and not t.requires_grad


def sdf_diff_loss_composite(pred, label, weight, scale, l2_loss=True):
    """sdf_diff_loss's torch composite: the batch mean of weight * r^2 (l2) or weight * |r| (l1), r = (pred - label) / scale"""
    r = (pred - label) / scale
    per = r ** 2 if l2_loss else r.abs()
    return (weight * per).sum() / pred.shape[0]


def sdf_diff_loss(pred, label, weight, scale, l2_loss=True):
    """utils/loss.py:6-14 (main_loss_type sdf_l1: l2_loss=False, sdf_l2: True)"""
    if (isinstance(pred, torch.Tensor) and pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 1 and pred.shape[0] > 0
            and _f32_cuda_like(label, pred) and label.shape == pred.shape and _f32_cuda_like(weight, pred)
            and weight.shape == pred.shape and isinstance(scale, (int, float)) and not isinstance(scale, bool) and scale != 0):
        ws = loss_workspace(pred.device)
        ext = _ext.module()
        if ext is not None:  # the C++ node (csrc/shine_torch_ext.cpp)
            return ext.diff_loss(pred, label, weight, float(scale), bool(l2_loss), ws)
        return _SdfDiff.apply(pred, label, weight, float(scale), bool(l2_loss), ws)
    return sdf_diff_loss_composite(pred, label, weight, scale, l2_loss)


def batch_ray_rendering_loss_composite(x, y, d_meas, neus_on=True):
    """batch_ray_rendering_loss's torch composite: per ray the samples in depth order, alphas a (the probabilities, or the
    clamped neus quotient of neighbours), o = (1 - a) + 1e-10, weights cumprod(o) / o * a; the mean |sum w x - d_meas|"""
    depth, order = x.sort(dim=1)
    prob = y.gather(1, order)
    if neus_on:
        lo, hi = prob[:, :-1], prob[:, 1:]
        a = ((hi - lo) / (1.0 - lo + 1e-10)).clamp(0.0, 1.0)
    else:
        a = prob
    o = torch.ones_like(a) - a + 1e-10
    w = o.cumprod(dim=1) / o * a
    d = (w * depth[:, :a.shape[1]]).sum(dim=1)
    return (d - d_meas).abs().mean()


def batch_ray_rendering_loss(x, y, d_meas, neus_on=True):
    """utils/loss.py:82-118: x sample depths [rays, samples], y occupancy probabilities [rays, samples] (the alphas of dr, the
    neus quotient's inputs of dr_neus), d_meas measured depths [rays]"""
    if (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.shape[0] > 0
            and 0 < y.shape[1] <= RAY_MAX_SAMPLES and _f32_cuda_like(x, y) and x.shape == y.shape
            and _f32_cuda_like(d_meas, y) and d_meas.shape == (y.shape[0],)):
        ws = loss_workspace(y.device)
        ext = _ext.module()
        if ext is not None:
            return ext.ray_render_loss(x, y, d_meas, bool(neus_on), ws)
        return _RayRender.apply(x, y, d_meas, bool(neus_on), ws)
    return batch_ray_rendering_loss_composite(x, y, d_meas, neus_on)


def normal_loss(g, normal_label, weight):
    """The surface-normal term of the drivers' normal_loss_on branch (shine_batch.py:192-197) in a form that can be evaluated:

        surf = weight > 0;  gh = g / |g| where |g| > 0, else 0;  loss = mean over surf of |gh - normal_label|_2  (0 without a surface row)

    g [N,3] = get_gradient(coord, pred) (times sigma_sigmoid or not: gh does not change), normal_label [N,3], weight [N].
    The reference's lines differ in two ways, both defects: `g / g.norm(2, dim=-1)` divides [N,3] by [N] and fails to broadcast
    for N other than 1 or 3 (keepdim=True is meant), and with that repaired a surface row whose g is exactly zero — a point that
    misses every level, a dead unit — is 0/0 and turns the mean into NaN.  The guard is the eikonal term's: such a row stays in
    the denominator, contributes |normal_label| and gets no gradient.  Rows with weight <= 0 do not read their label (it may be
    NaN).  Plain differentiable torch with no host sync: the composite ops.fused_normal_step (Tier B, one HIP launch) is checked
    against, and what a Tier A driver calls in place of the reference's three lines."""
    surf = weight > 0
    gn = g.norm(2, dim=-1, keepdim=True)
    live = gn > 0
    gh = torch.where(live, g / torch.where(live, gn, torch.ones_like(gn)), torch.zeros_like(g))
    label = torch.where(surf.unsqueeze(-1), normal_label.to(g.dtype), torch.zeros_like(g))
    per = (gh - label).norm(2, dim=-1)  # (the reference's .abs() in front of a 2-norm changes nothing)
    return torch.where(surf, per, torch.zeros_like(per)).sum() / surf.sum().clamp_min(1).to(g.dtype)


def consistency_loss(g_base, g_near):
    """The gradient-consistency term of the drivers' consistency_loss_on branch (shine_batch.py:149-158,187-190):

        c_k = (ga . gb) / (|ga| |gb|) where |ga| > 0 and |gb| > 0, else 0;  loss = mean over the K pairs of (1 - c_k)  (0 for K = 0)

    g_base [K,3] = get_gradient at the base points coord[near_index], g_near [K,3] = get_gradient at the shifted points (times
    sigma_sigmoid or not: the factor cancels).  The value is the reference's (1 - F.cosine_similarity(g_near, g_base)).mean(); THE
    GUARD differs: a pair with either gradient exactly zero — a point that misses every level, dead units — contributes 1 and gets
    NO gradient on either side, where the reference's line hands the zero side gbh / eps with eps = 1e-8, a finite but 1e8-scaled
    push into every weight the row's second-order path reaches.  Plain differentiable torch with no host sync: the composite
    ops.fused_consistency_step (Tier B, one HIP launch) is checked against, and what a Tier A driver calls in place of the
    reference's F.cosine_similarity line."""
    if g_base.shape[0] == 0:
        return (g_base.sum() + g_near.sum()) * 0.0
    na, nb = g_base.norm(2, dim=-1, keepdim=True), g_near.norm(2, dim=-1, keepdim=True)
    live = (na > 0) & (nb > 0)
    one = torch.ones_like(na)
    ah = g_base / torch.where(live, na, one)
    bh = g_near / torch.where(live, nb, one)
    c = torch.where(live.squeeze(-1), (ah * bh).sum(-1), torch.zeros_like(na.squeeze(-1)))
    return (1.0 - c).sum() / g_base.shape[0]


def get_gradient(inputs, outputs):
    """utils/tools.py:175-185: d outputs / d inputs with create_graph=True.  For the pred of the fused query_feature -> sdf
    node and its own coord: one launch (autograd_ops.InterpSdfGradCoord); otherwise the reference's autograd call."""
    link = getattr(outputs, "_shine_link", None)
    if link is not None and link[0].coord is inputs and inputs.requires_grad and torch.is_grad_enabled():
        src, params, ext_link = link
        if ext_link is not None:  # the fused node is the C++ one: so is this (csrc/shine_torch_ext.cpp)
            ext = _ext.module()
            L = src.octree.featured_level_num
            return ext.grad_coord(src.octree._ext_state(ext), outputs, inputs, ext_link, list(params[:L]), list(params[L:]))
        return InterpSdfGradCoord.apply(outputs, inputs, src.octree, src, *params)
    d_points = torch.ones_like(outputs, requires_grad=False, device=outputs.device)
    return grad(outputs=outputs, inputs=inputs, grad_outputs=d_points, create_graph=True, retain_graph=True,
                only_inputs=True)[0]
