"""Operators of the SHINE hot path on top of libshine_hip.so.

Tier B (fused, benchmarked):  ``fused_train_step`` = query + decode + sdf_bce_loss (+ eikonal) + the
whole backward in one HIP pass, writing dense ``.grad`` tensors exactly where autograd would
(shine_batch.py:115-209 minus the optimiser).

Tier A (strict drop-in):      ``octree_interp`` = FeatureOctree.query_feature as an autograd op
(model/feature_octree.py:237-244) so the reference drivers run unchanged.

Every function here calls the HIP library; none has a CPU / eager fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import _ext, _lib, autograd_ops


@dataclass
class StepOptions:
    """Scalars of one training iteration (names follow utils/config.py)."""

    sigma: float                      # sigma_sigmoid = logistic_gaussian_ratio*sigma_sigmoid_m*scale (shine_batch.py:87)
    loss_reduction: str = "mean"      # "mean" | "sum" (shine_incre.py:77-78)
    ekional_loss_on: bool = False     # (sic) config key of the reference
    weight_e: float = 0.1
    loss_weight_on: bool = False      # BCEWithLogitsLoss(weight=|weight|), utils/loss.py:18-19 (False in all shipped yamls)
    n_global: Optional[int] = None    # global batch size under data parallelism (defaults to local N)
    decoder_grad_on: Optional[bool] = None  # default: any decoder parameter requires grad (freeze_model, tools.py:188)
    deterministic: bool = False       # tests: ONE wave walks the whole batch, so the fp32 atomics of the feature-grad scatter are
                                      # applied in stream order and two runs agree to the bit (hundreds of times slower)
    # iteration hooks (loop.GraphedIteration): housekeeping of the calls that follow the step rides on its reduction launch
    adam_state: Optional[torch.Tensor] = None   # FusedAdam's device step state: the step counts the optimiser step
    adam_betas: tuple = (0.9, 0.99)
    zero_f64: Optional[torch.Tensor] = None     # one float64 element cleared by the step (the regulariser's accumulator)
    next_draw: Optional[object] = None          # SortedPool.next_draw(...): the first pass of the NEXT large sorted draw rides on
                                                # the step's reduction launch; complete it with pool.draw(..., pass1_done=True)
    draw_rider: Optional[object] = None         # sampler.DrawChain.rider[parity]: the WHOLE next sorted draw and the next step's
                                                # zero-fill ride in this step's two launches (cfg.draw_rider)
    kernel_variant: int = 0           # 0 the fused step (5 / 6: its far / near build whatever the table size); tests / tools: 1 the
                                      # lane-per-point reference kernel
                                      # (libshine_check.so)


def eik_needs_count(opts) -> bool:
    return bool(opts.ekional_loss_on)


def _stream():
    return _lib.current_stream_handle()


def _f32(t, name):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise ValueError("%s must be a CUDA float32 tensor" % name)
    return t.contiguous()


def _dense_grad(p: torch.Tensor) -> torch.Tensor:
    """autograd hands the optimiser a dense zero-initialised grad of the parameter's shape; so do we."""
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


def forward_sdf(octree, decoder, coord, want_feat=False, want_indices=False, want_grad_x=False, sigma=1.0):
    """query_feature + Decoder.sdf, forward only (utils/mesher.py:69-72 style inference).

    Returns dict(pred[N], feat[N,8]|None, indices (bottom-up list)|None, grad_x[N,3]|None = d pred/d coord * sigma).
    """
    t = octree._require_tables()
    coord = octree._check_coord(coord.detach())
    n = coord.shape[0]
    dev = coord.device
    pred = torch.empty(n, dtype=torch.float32, device=dev)
    feat = torch.empty((n, 8), dtype=torch.float32, device=dev) if want_feat else None
    gx = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_grad_x else None
    idx = None
    if want_indices:
        idx = [torch.empty((n, 8), dtype=torch.int64, device=dev) for _ in range(octree.featured_level_num)]
    cfg = octree.step_config(sigma=float(sigma))  # (set_zero: the forward kernel re-zeroes the trash rows)
    mlp = [p.detach() for p in decoder.fused_params()]
    _lib.check(
        _lib.lib().shine_forward(
            t.handle, C.byref(cfg), coord.data_ptr(), n, octree.feature_ptrs(), octree.row_counts(),
            _lib.ptr_array([p.data_ptr() for p in mlp]),
            feat.data_ptr() if feat is not None else None, pred.data_ptr(),
            _lib.ptr_array([o.data_ptr() for o in idx]) if idx is not None else None,
            gx.data_ptr() if gx is not None else None, _stream(),
        ),
        "shine_forward",
    )
    octree._tables_read_done()
    if idx is not None:
        octree.hierarchical_indices = idx
    return dict(pred=pred, feat=feat, indices=idx, grad_x=gx)


def fused_train_step(octree, decoder, coord, sdf_label, weight, opts: StepOptions, want_grad_x=False, perm=None,
                     n_surf: Optional[torch.Tensor] = None, slots: Optional[torch.Tensor] = None, touched=None,
                     pool=None, idx: Optional[torch.Tensor] = None, pending: Optional[dict] = None, graph=None,
                     grad_buffers=None):
    """One training iteration's forward+backward (no optimiser): the fused Tier-B step, raw form.

    coord [N,3], sdf_label [N], weight [N] (sign: + surface / - free space, utils/data_sampler.py:102-103).
    Accumulates into ``.grad`` of octree.hier_features[*] and the six decoder tensors (dense, trash row
    included — what ``cur_loss.backward()`` produces, shine_batch.py:209).  Returns (loss, pred, g) where
    loss is a 0-dim float64 device tensor (no host sync, NO grad_fn — the gradients are already in place) and
    g = get_gradient(coord,pred)*sigma or None.  `train_step` is the same launch as an autograd node.

    `pending` (a dict): the step launches its fused kernel only (cfg->defer_reduce) and leaves the per-workgroup partial sums
    — decoder grads, trash-row grads, loss terms — in the workspace for the optimiser's launch; the dict is filled with what
    FusedAdam.finish_iteration(pending, ...) needs, and `loss` is valid after that call.
    `graph` (loop.IterationGraph, with `pending`): nothing is launched — the launch this call would make becomes the step node
    of the library-built iteration graph (shine_iter_graph_set_step); outputs are valid after the graph ran.
    `grad_buffers` = (L feature-grad tensors, 6 decoder-grad tensors): accumulate into THESE (zero-filled by the caller) instead of
    the parameters' `.grad`.
    """
    gfeat, gmlp = grad_buffers if grad_buffers is not None else (None, None)
    return _fused_launch(octree, decoder, coord, sdf_label, weight, opts, want_grad_x=want_grad_x, perm=perm,
                         n_surf=n_surf, slots=slots, touched=touched, pool=pool, idx=idx, pending=pending, graph=graph,
                         gfeat=gfeat, gmlp=gmlp)


def train_step(octree, decoder, coord, sdf_label, weight, opts: StepOptions, want_grad_x=False, perm=None,
               n_surf: Optional[torch.Tensor] = None, slots: Optional[torch.Tensor] = None, touched=None,
               pool=None, idx: Optional[torch.Tensor] = None):
    """The fused step as ONE node of the autograd graph (autograd_ops.ShineTrainStep; SURVEY.md §8b Tier B):

        loss, pred, g = train_step(octree, geo_mlp, coord, sdf_label, weight, opts)
        opt.zero_grad(set_to_none=True); loss.backward(); opt.step()          # shine_batch.py:208-210, unchanged

    `loss` (0-dim float32, requires grad) = sdf_bce_loss [+ weight_e * eikonal]; other terms (e.g. lambda *
    cal_regularization, shine_incre.py:156-158) can be added to it before backward().  Same keyword arguments as
    fused_train_step.  When nothing requires grad (or under torch.no_grad) it degenerates to a forward pass."""
    from .autograd_ops import ShineTrainStep

    params = list(octree.feature_list()) + list(decoder.fused_params())
    extras = dict(want_grad_x=want_grad_x, perm=perm, n_surf=n_surf, slots=slots, touched=touched, pool=pool, idx=idx)
    loss, pred, g = ShineTrainStep.apply(octree, decoder, opts, coord, sdf_label, weight, extras, *params)
    return loss, pred, (g if g.numel() else None)


def _fused_launch(octree, decoder, coord, sdf_label, weight, opts: StepOptions, want_grad_x=False, perm=None,
                  n_surf: Optional[torch.Tensor] = None, slots: Optional[torch.Tensor] = None, touched=None,
                  pool=None, idx: Optional[torch.Tensor] = None, gfeat=None, gmlp=None, dec_grad=None, pending=None,
                  graph=None):
    """shine_train_step on explicit gradient buffers (gfeat: L tensors or None entries, gmlp: 6 tensors; default: the
    parameters' own dense `.grad`)."""
    # (the fused kernel reads the tables through the batch's memoised hash slots; only the check library's v0 probes in-kernel)
    t = octree._require_tables(probe=(int(opts.kernel_variant) & 0xff) == 1)
    pool_mode = pool is not None
    if pool_mode:  # batch = pool[idx] with idx sorted (sampler.SortedPool.draw): read straight out of the pool
        _check_pool_idx(octree, pool, idx)
        if eik_needs_count(opts) and n_surf is None:
            n_surf = (pool.weight[idx.long()] > 0).sum()
    variant = int(opts.kernel_variant) & 0xff
    # a pool of 32-byte records (sampler.SortedPool.rec; cfg.sorted_input 3): the record base goes in as `coord` — and, unread, as
    # `slots`: the records carry them —, the weight array only for 4-level trees; the check library's kernel takes the arrays
    rec_mode = pool_mode and getattr(pool, "rec", None) is not None and variant != 1
    if rec_mode:
        coord, sdf_label, weight, perm, slots = pool.rec, None, pool._weight_sep, idx, pool.rec
    elif pool_mode:
        coord, sdf_label, weight, slots = pool.soa()
        perm = idx
    if not rec_mode:
        coord = octree._check_coord(coord.detach())
    n = idx.numel() if pool_mode else coord.shape[0]
    dev = coord.device
    if not pool_mode and slots is None and variant != 1:
        # a batch without a plan (what the reference's get_batch hands over): neighbouring lanes would hit unrelated nodes and
        # the fused kernel takes the hash slots from the plan — order it by octree node and look the slots up first
        # (shine_plan_batch: 3 small launches; measured at 2^18 points x 4 levels 320 -> 143 us for the whole call against
        # in-kernel probing of the unordered batch, tools/unordered_bench.py).  A caller's own `perm` without slots (e.g.
        # dp.morton_order) is replaced by the plan's node order: the step does not depend on the visiting order.
        from .dp import plan_batch

        perm, slots = plan_batch(octree, coord, sort=False)  # (the step does not see the order of a small batch: one launch)
    if not rec_mode:
        sdf_label = _f32(sdf_label, "sdf_label")
    eik = bool(opts.ekional_loss_on)
    if bool(opts.loss_weight_on) and weight is None and not rec_mode:
        raise ValueError("loss_weight_on needs the sample weights")
    if (eik and not rec_mode) or weight is not None:
        weight = _f32(weight, "weight")
    if opts.loss_reduction not in ("mean", "sum"):
        raise ValueError("loss_reduction must be 'mean' or 'sum'")
    params = decoder.fused_params()
    if dec_grad is None:
        dec_grad = opts.decoder_grad_on
    if dec_grad is None:
        dec_grad = any(p.requires_grad for p in params)
    cfg = octree.step_config(
        decoder_grad_on=1 if dec_grad else 0, sorted_input=(3 if rec_mode else 2) if pool_mode else (0 if perm is None else 1),
        kernel_variant=int(opts.kernel_variant) | (0x4000 if getattr(opts, "deterministic", False) else 0),
        loss_weight_on=1 if opts.loss_weight_on else 0, **_loss_scalars(opts, n),
    )
    if opts.adam_state is not None:
        cfg.adam_state = opts.adam_state.data_ptr()
        cfg.adam_beta1, cfg.adam_beta2 = float(opts.adam_betas[0]), float(opts.adam_betas[1])
    if opts.zero_f64 is not None:
        cfg.zero_f64 = opts.zero_f64.data_ptr()
    if opts.next_draw is not None:
        cfg.next_draw = C.pointer(opts.next_draw)
    if opts.draw_rider is not None:
        if pending is not None or graph is not None or opts.next_draw is not None:
            raise ValueError("draw_rider is a hook of the plain fused step (not with next_draw / the deferred-reduction forms)")
        cfg.draw_rider = C.pointer(opts.draw_rider)
    if eik and n_surf is None:
        n_surf = (weight > 0).sum()  # stays on the device; under DP the caller all-reduces it first
    if eik and n_surf.numel() > 1:  # the sampler's per-block partial counts (SortedPool.draw(surf_parts=...))
        if n_surf.dtype != torch.int64 or not n_surf.is_contiguous():
            raise ValueError("n_surf parts must be a contiguous int64 tensor")
        if (int(opts.kernel_variant) & 0xff) == 1 or slots is None:
            n_surf = n_surf.sum()  # the check library's kernels take one count
        else:
            cfg.n_surf_parts = int(n_surf.numel())
    pred = torch.empty(n, dtype=torch.float32, device=dev)
    gx = torch.empty((n, 3), dtype=torch.float32, device=dev) if (want_grad_x and eik) else None
    loss_parts = torch.empty(4, dtype=torch.float64, device=dev)  # overwritten by the step; set_zero is in-kernel
    if gfeat is None:
        gfeat = [_dense_grad(p) if p.requires_grad else None for p in octree.feature_list()]
    if gmlp is None:
        gmlp = [_dense_grad(p) for p in params] if dec_grad else [None] * 6
    if perm is not None and not (perm.is_cuda and perm.dtype == torch.int32 and perm.numel() == n):
        raise ValueError("perm must be a CUDA int32 tensor of N entries")
    # (slots without perm: a batch that already IS in visiting order — e.g. gathered from a node-ordered pool — with its hash slots)
    if slots is not None and not pool_mode and not (slots.is_cuda and slots.dtype == torch.int32
                                                    and slots.numel() == n * octree.featured_level_num):
        raise ValueError("slots (from dp.plan_batch, or of a batch in visiting order): CUDA int32 [N, L]")
    ws = _workspace(dev, cfg)
    if pending is not None:
        if variant not in (0, 4, 5, 6) or slots is None:
            raise ValueError("pending= (deferred reduction) needs the product kernel on a planned / pool batch")
        cfg.defer_reduce = 1
        pending.clear()
        pending.update(cfg=cfg, n=n, workspace=ws, n_surf=n_surf, loss_parts=loss_parts, dec_grad=bool(dec_grad),
                       octree=octree, decoder=decoder, pred=pred, gx=gx)
    if graph is not None and pending is None:
        raise ValueError("graph= records the deferred-reduction step: pass pending= too")
    # the product library trains on <= 4 featured levels (every shipped yaml: 3 or 4) with kernel_variant 0 / 4; the
    # lane-per-point reference kernel (1: any batch, <= 8 levels) is the check library's — tests / tools ask for it by name
    if variant != 1 and octree.featured_level_num > 4:
        raise NotImplementedError("the fused step handles tree_level_feat <= 4 (every shipped config); deeper trees only run "
                                  "on the check library's reference kernel (StepOptions.kernel_variant = 1, tests / tools)")
    library = _lib.check_lib() if variant == 1 else _lib.lib()
    entry = library.shine_train_step if graph is None else \
        (lambda *a: library.shine_iter_graph_set_step(graph.handle, *a[:-1]))  # (the same arguments minus the stream)
    _lib.check(
        entry(
            t.handle, C.byref(cfg), coord.data_ptr(), sdf_label.data_ptr() if sdf_label is not None else None,
            weight.data_ptr() if weight is not None else None,
            perm.data_ptr() if perm is not None else None,
            slots.data_ptr() if slots is not None else None,
            n_surf.data_ptr() if n_surf is not None else None, n,
            octree.feature_ptrs(), octree.row_counts(),
            _lib.ptr_array([p.data_ptr() for p in params]),
            pred.data_ptr(), gx.data_ptr() if gx is not None else None,
            _lib.ptr_array([g.data_ptr() if g is not None else None for g in gfeat]),
            _lib.ptr_array([g.data_ptr() if g is not None else None for g in gmlp]),
            loss_parts.data_ptr(),
            _lib.ptr_array([x.data_ptr() for x in touched]) if touched is not None else None,
            ws.data_ptr(), ws.numel(), _stream(),
        ),
        "shine_train_step", library,
    )
    if opts.next_draw is not None and pending is None and getattr(opts.next_draw, "_pool", None) is not None:
        opts.next_draw._pool._rider_for = int(opts.next_draw.n)  # its reduction launch carried that draw's first pass
    return loss_parts[3], pred, gx  # 0-dim float64 view: BCE (+ weight_e * eikonal), no extra launch


# ---- the five steps beside the fused one (fused_sem_step, fused_normal_step, fused_consistency_step, fused_time_step,
# fused_ray_step) share their host side: where the batch and its weights are read from, the surface count, the
# loss's scalars, where the gradients go, the loss's tensor, and the call.  A step keeps its own checks and its argument list.
def _i32c(x):
    return isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32 and x.is_contiguous()


def _loss_scalars(opts, n=None):
    """the loss's scalars of step_config; with `n`, the batch's rows, also those of a loss that is a mean over rows or a sum"""
    kw = dict(sigma=float(opts.sigma), weight_e=float(opts.weight_e), eikonal_on=1 if opts.ekional_loss_on else 0)
    if n is not None:
        n_global = int(opts.n_global) if opts.n_global else n
        total = opts.loss_reduction == "sum"
        kw.update(reduction_sum=1 if total else 0, n_global=n_global, inv_n=1.0 if total else 1.0 / max(n_global, 1))
    return kw


def _term_weights(pool, stride, weight, rows_n):
    """(ptr, stride in floats, the tensor to keep alive) of the batch's sample weights: the pool's SoA array, word 4 of its 32-byte
    records or its separate array (4-level trees); array mode: weight [rows_n] float32"""
    if pool is None:
        keep = _f32(weight, "weight")
        if keep.dim() != 1 or keep.numel() != rows_n:
            raise ValueError("weight must hold one value per coordinate")
    elif stride == 3:
        keep = pool.soa()[2]
    elif pool._weight_sep is None:
        return pool.rec.data_ptr() + 16, 8, pool.rec
    else:
        keep = pool._weight_sep
    return keep.data_ptr(), 1, keep


def _n_surf(n_surf, w=None, idx=None, max_parts=None, parts="the draw's partial counts"):
    """the surface count a step divides by, checked: one count or up to `max_parts` partial counts.  Without `w` only its type (the
    check that comes ahead of the batch's own); with `w`, the weights the batch reads through idx, everything, and the default:
    the rows with weight > 0, counted on the device"""
    ok = n_surf is None or isinstance(n_surf, torch.Tensor)
    if ok and w is not None:
        if n_surf is None:
            n_surf = ((w[idx.long()] if idx is not None else w) > 0).sum()
        ok = (n_surf.is_cuda and n_surf.dtype == torch.int64 and n_surf.is_contiguous()
              and 1 <= n_surf.numel() <= (max_parts or n_surf.numel()))
    if not ok:
        raise ValueError("n_surf must be a contiguous CUDA int64 tensor (one count, or %s)" % parts)
    return n_surf


def _check_pool_idx(octree, pool, idx):
    """pool mode: the batch is pool[idx], and the pool was planned on the octree's tables as they are now"""
    if not _i32c(idx):
        raise ValueError("pool mode needs idx = SortedPool.draw(n) (CUDA int32)")
    if pool.tables_epoch != octree._tables_epoch:
        raise RuntimeError("the octree grew since the pool was planned: call SortedPool.rebuild()")


def _term_batch(octree, coord, pool, idx, pool_needs=None):
    """(src, floats per row, n, device) of a term step's batch.  Array mode: coord [N,3], read through idx when given.  Pool
    mode: pool[idx] straight out of the pool's 32-byte records, or of its SoA coordinates; `pool_needs` names the pool attribute
    the term reads beside them."""
    if pool is not None:
        _check_pool_idx(octree, pool, idx)
        if pool_needs is not None and getattr(pool, pool_needs, None) is None:
            raise ValueError("pool mode needs a SortedPool built with %s=" % pool_needs)
        rec = getattr(pool, "rec", None)
        src, stride = (rec, 8) if rec is not None else (pool.soa()[0], 3)
    else:
        if not isinstance(coord, torch.Tensor):
            raise ValueError("array mode needs coord [N,3] (or pool= and idx=)")
        src, stride = octree._check_coord(coord.detach()), 3
        if idx is not None and not _i32c(idx):
            raise ValueError("idx must be a contiguous CUDA int32 tensor")
    n = int(idx.numel()) if idx is not None else int(src.shape[0])
    return src, stride, n, src.device


def _term_targets(octree, mlp, grad_buffers, who):
    """(L feature-grad tensors | None entries, 6 weight-grad tensors | None): `grad_buffers`, or the parameters' dense `.grad`"""
    gfeat, gmlp = grad_buffers if grad_buffers is not None else (None, None)
    if gfeat is None:
        gfeat = [_dense_grad(p) if p.requires_grad else None for p in octree.feature_list()]
    if grad_buffers is None:
        train = [p.requires_grad for p in mlp]
        if any(train) != all(train):
            raise ValueError("%s six tensors must all require grad or all be frozen" % who)
        gmlp = [_dense_grad(p) for p in mlp] if all(train) else None
    return gfeat, gmlp


def _term_out(out, dev):
    if out is None:
        return torch.empty(1, dtype=torch.float32, device=dev)
    if not (out.is_cuda and out.dtype == torch.float32 and out.numel() == 1):
        raise ValueError("out must be a CUDA float32 tensor of one element")
    return out


def _term_ptrs(octree, mlp, gfeat, gmlp):
    """(feats, rows, grad_feats, mlp, grad_mlp | None) as the entry points take them"""
    return (octree.feature_ptrs(), octree.row_counts(), _lib.ptr_array([g.data_ptr() if g is not None else None for g in gfeat]),
            _lib.ptr_array([p.data_ptr() for p in mlp]),
            _lib.ptr_array([g.data_ptr() for g in gmlp]) if gmlp is not None else None)


def _term_call(name, octree, *args):
    """the entry point `name` on the current stream (looked up at call time); the launch probed the hash tables"""
    rc = getattr(_lib.lib(), name)(*args, _lib.current_stream_handle())
    if rc != 0:
        _lib.check(rc, name)
    if not torch.cuda.is_current_stream_capturing():
        octree._tables_read_done()


def fused_sem_step(octree, sem_decoder, coord, sem_label, weight_s, decimation=1, pool=None, idx=None, grad_buffers=None,
                   out=None, workspace=None):
    """The semantic term of one training iteration (shine_batch.py:132-133,200-204) in ONE launch (shine_sem_train_step):

        sem_loss = NLLLoss('mean')(sem_decoder.sem_label_prob(octree.query_feature(coord))[::decimation], sem_label[::decimation])
        (weight_s * sem_loss).backward()

    coord [N,3] float32, sem_label [N] int32 with 0 <= label < the head's class count (the caller's precondition: SortedPool checks
    its labels at rebuild), or pool = a SortedPool built with sem_label= and idx = pool.draw(n): the batch is read straight out of
    the pool's records (coord / sem_label are ignored).  Returns the UNWEIGHTED sem_loss as a 0-dim float32 device tensor (no host
    sync, no grad_fn — the gradients are already in place; `out`: a float32 tensor of one element to write it to).
    Accumulates into ``.grad`` of octree.hier_features[*] and of the head's six tensors exactly as fused_train_step does (dense,
    trash row included), or into `grad_buffers` = (L feature-grad tensors, 6 head-grad tensors | None) instead.  A head whose
    parameters do not require grad (freeze_model) gets no gradient: only the feature grads are written.
    `workspace`: SHINE_SEM_WORKSPACE_BYTES of zeroed device memory the caller owns (default: the current stream's,
    autograd_ops.sem_workspace)."""
    t = octree._require_tables()  # (the kernel probes the hash tables from the coordinates)
    mlp = sem_decoder.sem_params()
    n_class = int(mlp[4].shape[0])
    decimation = int(decimation)
    if decimation < 1:
        raise ValueError("decimation must be >= 1")
    src, stride, n, dev = _term_batch(octree, coord, pool, idx, pool_needs="sem_label")
    labels = pool.sem_label if pool is not None else sem_label
    if pool is None and idx is None and labels.numel() != n:
        raise ValueError("sem_label must hold one label per coordinate")
    if not _i32c(labels):
        raise ValueError("sem_label must be a contiguous CUDA int32 tensor")
    if not sem_decoder._params_on(dev, mlp):
        raise ValueError("the semantic decoder's parameters must be CUDA float32 contiguous on the batch's device")
    gfeat, gmlp = _term_targets(octree, mlp, grad_buffers, "the semantic head's")
    out = _term_out(out, dev)
    ws = workspace if workspace is not None else autograd_ops.sem_workspace(dev)
    cfg = octree.step_config()
    feats, rows, grad_feats, mlp_ptrs, grad_mlp = _term_ptrs(octree, mlp, gfeat, gmlp)
    _term_call("shine_sem_train_step", octree, t.handle, C.byref(cfg), src.data_ptr(), stride,
               idx.data_ptr() if idx is not None else None, labels.data_ptr(), n, decimation, float(weight_s), feats, rows,
               grad_feats, mlp_ptrs, n_class, grad_mlp, out.data_ptr(), ws.data_ptr())
    return out.view(())


def fused_normal_step(octree, decoder, coord, weight, normal_label, weight_n, n_surf=None, pool=None, idx=None,
                      grad_buffers=None, out=None, workspace=None):
    """The surface-normal term of one training iteration (shine_batch.py:192-197) in ONE launch (shine_normal_train_step):

        g = get_gradient(coord, decoder.sdf(octree.query_feature(coord)))
        normal_loss = losses.normal_loss(g, normal_label, weight);  (weight_n * normal_loss).backward()

    — the definition of losses.normal_loss: the reference's lines with keepdim repaired and a zero-gradient guard (a surface row
    whose g is exactly zero stays in the mean's denominator, contributes |normal_label| and gets no gradient).  No sigma: a
    positive factor on g changes nothing.
    Array mode: coord [N,3] float32, weight [N] float32 (> 0: a surface sample), normal_label [N,3] float32 (need not be unit
    vectors; rows with weight <= 0 are not read), optionally idx (CUDA int32: batch position i reads row idx[i] of all three).
    Pool mode: pool = a SortedPool built with normal_label= and idx = pool.draw(n): the batch is read straight out of the pool's
    records (coord / weight / normal_label are ignored).  `n_surf`: the number of surface rows as an int64 device tensor of one
    element, or the draw's partial counts (pool.surf_parts_buffer(), summed in the kernel); default (weight > 0).sum() on the
    device; under data parallelism the caller passes the global count.
    Returns the UNWEIGHTED normal_loss as a 0-dim float32 device tensor (no host sync, no grad_fn — the gradients are already in
    place; `out`: a float32 tensor of one element to write it to).  Accumulates into ``.grad`` of octree.hier_features[*] and of
    the decoder's W1, W2, w3 exactly as fused_train_step does (dense, trash row included; the biases receive nothing), or into
    `grad_buffers` = (L feature-grad tensors, 6 decoder-grad tensors | None) instead.  A decoder whose parameters do not
    require grad (freeze_model) gets no gradient: only the feature grads are written.
    `workspace`: SHINE_NORMAL_WORKSPACE_BYTES of zeroed device memory the caller owns (default: the current stream's,
    autograd_ops.normal_workspace)."""
    t = octree._require_tables()  # (the kernel probes the hash tables from the coordinates)
    mlp = decoder.fused_params()
    _n_surf(n_surf)
    if pool is None and not all(isinstance(x, torch.Tensor) for x in (coord, weight, normal_label)):
        raise ValueError("array mode needs coord [N,3], weight [N] and normal_label [N,3] (or pool= and idx=)")
    src, stride, n, dev = _term_batch(octree, coord, pool, idx, pool_needs="normal_label")
    normal = pool.normal_label if pool is not None else normal_label
    w_ptr, w_stride, w_keep = _term_weights(pool, stride, weight, src.shape[0])
    if not (isinstance(normal, torch.Tensor) and normal.is_cuda and normal.dtype == torch.float32 and normal.is_contiguous()
            and normal.dim() == 2 and normal.shape[1] == 3):
        raise ValueError("normal_label must be a contiguous CUDA float32 [N,3] tensor")
    if pool is None and normal.shape[0] != src.shape[0]:
        raise ValueError("normal_label must hold one normal per coordinate")
    n_surf = _n_surf(n_surf, pool.weight if pool is not None else w_keep, idx)
    if not decoder._params_on(dev, mlp):
        raise ValueError("the decoder's parameters must be CUDA float32 contiguous on the batch's device")
    gfeat, gmlp = _term_targets(octree, mlp, grad_buffers, "the decoder's")
    out = _term_out(out, dev)
    ws = workspace if workspace is not None else autograd_ops.normal_workspace(dev)
    cfg = octree.step_config()
    _term_call("shine_normal_train_step", octree, t.handle, C.byref(cfg), src.data_ptr(), stride,
               idx.data_ptr() if idx is not None else None, w_ptr, w_stride, normal.data_ptr(), n_surf.data_ptr(),
               int(n_surf.numel()), n, float(weight_n), *_term_ptrs(octree, mlp, gfeat, gmlp), out.data_ptr(), ws.data_ptr())
    del w_keep  # (the weights outlive the call)
    return out.view(())


def fused_consistency_step(octree, decoder, coord, weight_c, near_index=None, shift=None, n_pairs=None, shift_scale=None, seed=0,
                           draw_state=None, pool=None, idx=None, touched=None, grad_buffers=None, out=None, workspace=None,
                           draws_out=None):
    """The gradient-consistency term of one training iteration (shine_batch.py:149-158,187-190) in ONE launch
    (shine_consistency_train_step):

        a = coord[near_index];  b = a + shift;  ga, gb = get_gradient at a, b (through the decoder's sdf of the queried features)
        consistency_loss = losses.consistency_loss(ga, gb);  (weight_c * consistency_loss).backward()

    — the definition of losses.consistency_loss: the mean over the K pairs of 1 - cos(ga, gb), a pair with either gradient exactly
    zero contributing 1 and getting no gradient (the reference's line pushes gbh / 1e-8 into the zero side).  Every batch row can
    be a base point, free-space rows included; no weight, no label and no sigma enter.
    Array mode: coord [N,3] float32, optionally idx (CUDA int32: batch row i is coord[idx[i]]).  Pool mode: pool = a SortedPool
    and idx = pool.draw(n): the base rows are read straight out of the pool's records (coord is ignored).
    Explicit pairs: near_index (CUDA int32 [K], values in [0, n) — batch rows, repeats allowed) and shift (CUDA float32 [K,3]).
    Drawn pairs: both None — the kernel draws K = n_pairs pairs itself from (seed, draw_state[0]) with each shift component in
    [-shift_scale, shift_scale) (the reference's consistency_range * scale) and advances draw_state (a CUDA int64 tensor of one
    element the caller owns) by one, so a replayed graph draws fresh pairs every time.  `draws_out` = (int32 [K], float32 [K,3])
    receives the pairs the launch used.
    `touched`: the per-level uint8 row flags of ops.touched_flags(octree); every row the term adds gradient to is flagged (the
    shifted points reach rows the batch's own points do not, and the active-row Adam skips an unflagged row).
    Returns the UNWEIGHTED consistency_loss as a 0-dim float32 device tensor (no host sync, no grad_fn — the gradients are
    already in place; `out`: a float32 tensor of one element to write it to).  Accumulates into ``.grad`` of
    octree.hier_features[*] and of the decoder's W1, W2, w3 exactly as fused_normal_step does, or into `grad_buffers` = (L
    feature-grad tensors, 6 decoder-grad tensors | None) instead.  A decoder whose parameters do not require grad gets no
    gradient: only the feature grads are written.
    `workspace`: SHINE_CONSISTENCY_WORKSPACE_BYTES of zeroed device memory the caller owns (default: the current stream's,
    autograd_ops.consistency_workspace)."""
    t = octree._require_tables()  # (the kernel probes the hash tables from the coordinates)
    mlp = decoder.fused_params()

    def _f32k3(x):
        return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2
                and x.shape[1] == 3)

    src, stride, n, dev = _term_batch(octree, coord, pool, idx)
    if (near_index is None) != (shift is None):
        raise ValueError("near_index and shift come together (both: explicit pairs; neither: drawn pairs)")
    explicit = near_index is not None
    if explicit:
        if not (_i32c(near_index) and near_index.dim() == 1):
            raise ValueError("near_index must be a contiguous CUDA int32 [K] tensor")
        k = int(near_index.numel())
        if not (_f32k3(shift) and shift.shape[0] == k):
            raise ValueError("shift must be a contiguous CUDA float32 [K,3] tensor, one row per near_index entry")
        if n_pairs is not None and int(n_pairs) != k:
            raise ValueError("n_pairs must equal the number of explicit pairs")
    else:
        if n_pairs is None or int(n_pairs) < 0:
            raise ValueError("drawn pairs need n_pairs >= 0")
        k = int(n_pairs)
        if shift_scale is None or not float(shift_scale) >= 0.0:
            raise ValueError("drawn pairs need shift_scale >= 0 (consistency_range * scale)")
        if not (isinstance(draw_state, torch.Tensor) and draw_state.is_cuda and draw_state.dtype == torch.int64
                and draw_state.numel() == 1):
            raise ValueError("drawn pairs need draw_state: a CUDA int64 tensor of one element")
    if k > 0 and n == 0:
        raise ValueError("pairs need a batch: n_pairs > 0 with no batch row")
    ni_out = sh_out = None
    if draws_out is not None:
        ni_out, sh_out = draws_out
        if not (_i32c(ni_out) and ni_out.numel() >= k and _f32k3(sh_out) and sh_out.shape[0] >= k):
            raise ValueError("draws_out = (CUDA int32 [K], CUDA float32 [K,3])")
    if touched is not None and not (len(touched) == octree.featured_level_num
                                    and all(x.is_cuda and x.dtype == torch.uint8 for x in touched)):
        raise ValueError("touched = ops.touched_flags(octree): one CUDA uint8 tensor per featured level")
    if not decoder._params_on(dev, mlp):
        raise ValueError("the decoder's parameters must be CUDA float32 contiguous on the batch's device")
    gfeat, gmlp = _term_targets(octree, mlp, grad_buffers, "the decoder's")
    out = _term_out(out, dev)
    if k == 0:  # (what the entry point does for n_pairs == 0; empty explicit tensors have no address to hand it)
        out.zero_()
        return out.view(())
    ws = workspace if workspace is not None else autograd_ops.consistency_workspace(dev)
    cfg = octree.step_config()
    _term_call("shine_consistency_train_step", octree, t.handle, C.byref(cfg), src.data_ptr(), stride,
               idx.data_ptr() if idx is not None else None, n,
               near_index.data_ptr() if explicit else None, shift.data_ptr() if explicit else None, k,
               float(shift_scale) if shift_scale is not None else 0.0, int(seed) & 0xFFFFFFFFFFFFFFFF,
               draw_state.data_ptr() if (draw_state is not None and not explicit) else None,
               ni_out.data_ptr() if ni_out is not None else None, sh_out.data_ptr() if sh_out is not None else None,
               float(weight_c), *_term_ptrs(octree, mlp, gfeat, gmlp),
               _lib.ptr_array([x.data_ptr() for x in touched]) if touched is not None else None,
               out.data_ptr(), ws.data_ptr())
    return out.view(())


def fused_time_step(octree, decoder, coord, sdf_label, weight, ts, opts: StepOptions, n_surf=None, pool=None, idx=None,
                    grad_buffers=None, out=None, workspace=None, pred_out=None):
    """One training iteration's forward + backward of a TIME-CONDITIONED map (config.time_conditioned; shine_batch.py:119-130,
    141-142,172-185,208-209) in ONE launch (shine_time_step), no optimiser:

        pred = decoder.time_conditionded_sdf(octree.query_feature(coord), ts)
        loss = sdf_bce_loss(pred, sdf_label, opts.sigma, None, False, opts.loss_reduction)
        [+ opts.weight_e * ((1 - (get_gradient(coord, pred) * opts.sigma)[weight > 0].norm(2, dim=-1)) ** 2).mean()]
        loss.backward()

    with fused_train_step's conventions: the eikonal mean is 0 without a surface row, a row with |g| == 0 contributes 1 and gets no
    gradient through g, 'mean' divides by opts.n_global or N.  `decoder`: Decoder(config, is_time_conditioned=True) in the fusable
    shape (decoder.time_fusable).  `opts.loss_weight_on` is not served.
    Array mode: coord [N,3], sdf_label [N], ts [N] float32, weight [N] float32 (read with the eikonal term only; may be None
    without it), optionally idx (CUDA int32: batch position i reads row idx[i] of all four).  Pool mode: pool = a SortedPool built
    with ts= and idx = pool.draw(n): the batch is read straight out of the pool's records (the four arrays are ignored).
    `n_surf` (eikonal): the number of surface rows as an int64 device tensor of one element, or the draw's partial counts
    (pool.surf_parts_buffer()); default (weight > 0).sum() on the device.
    Returns the loss as a 0-dim float32 device tensor (no host sync, no grad_fn — the gradients are already in place; `out`: a
    float32 tensor of one element to write it to).  Accumulates into ``.grad`` of octree.hier_features[*] (dense, trash row
    included) and of the head's six tensors — W1 [32,9] with its time column —, or into `grad_buffers` = (L feature-grad tensors, 6
    decoder-grad tensors | None) instead.  A decoder whose parameters do not require grad gets no gradient.  ts gets none.
    `pred_out`: a CUDA float32 [N] tensor that receives pred at the batch position.
    `workspace`: zeroed device memory of autograd_ops.time_step_workspace_bytes() bytes the caller owns (default: the current
    stream's, autograd_ops.time_step_workspace)."""
    t = octree._require_tables()  # (the kernel probes the hash tables from the coordinates)
    if not getattr(decoder, "time_fusable", False):
        raise NotImplementedError("fused_time_step needs the time-conditioned head 9 -> 32 -> 32 -> 1 with bias (decoder.time_fusable)")
    mlp = decoder.time_params()
    if bool(opts.loss_weight_on):
        raise NotImplementedError("fused_time_step does not serve loss_weight_on (False in every shipped config)")
    if opts.loss_reduction not in ("mean", "sum"):
        raise ValueError("loss_reduction must be 'mean' or 'sum'")
    eik = bool(opts.ekional_loss_on)
    _n_surf(n_surf)
    if pool is None and not all(isinstance(x, torch.Tensor) for x in (coord, sdf_label, ts) + ((weight,) if eik else ())):
        raise ValueError("array mode needs coord [N,3], sdf_label [N], ts [N] and, with the eikonal term, weight [N] (or pool= and "
                         "idx=)")
    src, stride, n, dev = _term_batch(octree, coord, pool, idx, pool_needs="ts")
    if pool is not None:
        ts_arr, label = pool.ts, (pool.soa()[1] if stride == 3 else None)  # (the records carry their labels)
    else:
        ts_arr, label = ts, _f32(sdf_label, "sdf_label")
        if label.dim() != 1 or label.numel() != int(src.shape[0]):
            raise ValueError("sdf_label must hold one value per coordinate")
    # (array mode reads the weights with the eikonal term only: they may be None without it)
    w_ptr, w_stride, w_keep = None, 1, None
    if pool is not None or eik:
        w_ptr, w_stride, w_keep = _term_weights(pool, stride, weight, int(src.shape[0]))
    if not (isinstance(ts_arr, torch.Tensor) and ts_arr.is_cuda and ts_arr.dtype == torch.float32 and ts_arr.is_contiguous()
            and ts_arr.numel() == (pool.size if pool is not None else int(src.shape[0]))):
        raise ValueError("ts must be a contiguous CUDA float32 tensor, one time stamp per coordinate")
    if eik:
        n_surf = _n_surf(n_surf, pool.weight if pool is not None else w_keep, idx, max_parts=64)
    if pred_out is not None and not (isinstance(pred_out, torch.Tensor) and pred_out.is_cuda and pred_out.dtype == torch.float32
                                     and pred_out.is_contiguous() and pred_out.numel() == n):
        raise ValueError("pred_out must be a contiguous CUDA float32 tensor of N elements")
    if not decoder._params_on(dev, mlp):
        raise ValueError("the decoder's parameters must be CUDA float32 contiguous on the batch's device")
    gfeat, gmlp = _term_targets(octree, mlp, grad_buffers, "the decoder's")
    out = _term_out(out, dev)
    ws = workspace if workspace is not None else autograd_ops.time_step_workspace(dev)
    cfg = octree.step_config(**_loss_scalars(opts, n))
    ws_bytes = C.c_size_t(int(ws.numel()) * int(ws.element_size()))
    _term_call("shine_time_step", octree, t.handle, C.byref(cfg), src.data_ptr(), stride,
               idx.data_ptr() if idx is not None else None, label.data_ptr() if label is not None else None,
               w_ptr if eik else None, w_stride, ts_arr.data_ptr(), n_surf.data_ptr() if eik else None,
               int(n_surf.numel()) if eik else 0, n, *_term_ptrs(octree, mlp, gfeat, gmlp),
               pred_out.data_ptr() if pred_out is not None else None, out.data_ptr(), ws.data_ptr(), C.byref(ws_bytes))
    del w_keep  # (the weights outlive the call)
    return out.view(())


RAY_MAX_SAMPLES = 32  # include/shine_hip.h SHINE_RAY_MAX_SAMPLES


def _f32_n(x, numel, what):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == numel):
        raise ValueError("%s must be a contiguous CUDA float32 tensor of %d elements" % (what, numel))
    return x


def fused_ray_step(octree, decoder, coord, weight, sample_depth, ray_depth, sigma_size, opts: StepOptions, samples, neus_on=False,
                   n_surf=None, pool=None, idx=None, grad_buffers=None, sigma_grad=None, out=None, workspace=None, pred_out=None,
                   dpred_out=None):
    """One training iteration's forward + backward of a map trained by RAY RENDERING (config.ray_loss with main_loss_type dr /
    dr_neus; shine_batch.py:119-130,160-170,172-185,208-209) in ONE launch (shine_ray_step), no optimiser:

        pred = decoder.sdf(octree.query_feature(coord))
        loss = losses.batch_ray_rendering_loss(sample_depth.view(-1, S), torch.sigmoid(pred / sigma_size).view(-1, S), ray_depth,
                                               neus_on)
        [+ opts.weight_e * ((1 - (get_gradient(coord, pred) * opts.sigma)[weight > 0].norm(2, dim=-1)) ** 2).mean()]
        loss.backward()

    with fused_train_step's conventions for the eikonal term: 0 without a surface row, a row with |g| == 0 contributes 1 and gets
    no gradient through g.  `decoder`: the plain 8 -> 32 -> 32 -> 1 geometry head.  `samples` = S = surface_sample_n +
    free_sample_n (1 .. 32).  `sigma_size`: the learnable CUDA float32 tensor of one element; the launch reads it on the device.
    Array mode: ray-major coord [m*S,3], weight [m*S] (read with the eikonal term only; may be None without it), sample_depth
    [m*S], ray_depth [m]; optionally idx (CUDA int32: batch ray i is ray idx[i]).  Pool mode: pool = a sampler.RayPool and idx =
    pool.draw(n) (the four arrays and `samples` are the pool's).
    `n_surf` (eikonal): the batch's rows with weight > 0 as an int64 device tensor (one count, e.g. RayPool.draw(surf_out=...), or
    up to 64 partial counts); default: counted here on the device.
    Returns the loss as a 0-dim float32 device tensor (no host sync, no grad_fn — the gradients are already in place; `out`: a
    float32 tensor of one element to write it to).  Accumulates into ``.grad`` of octree.hier_features[*] (dense, trash row
    included), of the head's six tensors and of sigma_size — or into `grad_buffers` = (L feature-grad tensors, 6 decoder-grad
    tensors | None) and `sigma_grad` (a CUDA float32 tensor of one element) instead.  A decoder whose parameters do not require
    grad gets no gradient (a half-frozen one is refused); a sigma_size that does not require grad gets none either.
    `pred_out` / `dpred_out`: CUDA float32 [n*S] tensors that receive pred and d (render term) / d pred at the batch position.
    `workspace`: zeroed device memory of autograd_ops.ray_step_workspace_bytes() bytes the caller owns (default: the current
    stream's, autograd_ops.ray_step_workspace)."""
    t = octree._require_tables()  # (the kernel probes the hash tables from the coordinates)
    if getattr(decoder, "time_fusable", False) or not hasattr(decoder, "fused_params"):
        raise NotImplementedError("fused_ray_step needs the plain geometry head 8 -> 32 -> 32 -> 1 (not a time-conditioned decoder)")
    mlp = decoder.fused_params()
    eik = bool(opts.ekional_loss_on)
    _n_surf(n_surf, parts="partial counts")
    if pool is not None:
        _check_pool_idx(octree, pool, idx)
        if not hasattr(pool, "surf_per_ray"):
            raise ValueError("pool mode needs a sampler.RayPool")
        coord, weight, sample_depth, ray_depth, S = pool.coord, pool.weight, pool.sample_depth, pool.ray_depth, int(pool.samples)
    else:
        S = int(samples)
        if not all(isinstance(x, torch.Tensor) for x in (coord, sample_depth, ray_depth) + ((weight,) if eik else ())):
            raise ValueError("array mode needs coord [m*S,3], sample_depth [m*S], ray_depth [m] and, with the eikonal term, weight "
                             "[m*S] (or pool= and idx=)")
        if idx is not None and not _i32c(idx):
            raise ValueError("idx must be a contiguous CUDA int32 tensor")
    if not 1 <= S <= RAY_MAX_SAMPLES:
        raise ValueError("samples must be 1 .. %d (SHINE_RAY_MAX_SAMPLES)" % RAY_MAX_SAMPLES)
    src = octree._check_coord(coord.detach())
    dev = src.device
    m = int(ray_depth.numel()) if isinstance(ray_depth, torch.Tensor) else -1
    if int(src.shape[0]) != m * S:
        raise ValueError("coord must hold samples rows per entry of ray_depth (ray-major)")
    _f32_n(sample_depth, m * S, "sample_depth")
    _f32_n(ray_depth, m, "ray_depth")
    if eik:
        _f32_n(weight, m * S, "weight")
    _f32_n(sigma_size, 1, "sigma_size")
    n = int(idx.numel()) if idx is not None else m
    if eik:
        n_surf = _n_surf(n_surf, weight.view(m, S), idx, max_parts=64, parts="partial counts")
    for name, o in (("pred_out", pred_out), ("dpred_out", dpred_out)):
        if o is not None:
            _f32_n(o, n * S, name)
    if not decoder._params_on(dev, mlp):
        raise ValueError("the decoder's parameters must be CUDA float32 contiguous on the batch's device")
    gfeat, gmlp = _term_targets(octree, mlp, grad_buffers, "the decoder's")
    if sigma_grad is not None:
        _f32_n(sigma_grad, 1, "sigma_grad")
    elif sigma_size.requires_grad:
        sigma_grad = _dense_grad(sigma_size)
    out = _term_out(out, dev)
    ws = workspace if workspace is not None else autograd_ops.ray_step_workspace(dev)
    cfg = octree.step_config(**_loss_scalars(opts))
    ws_bytes = C.c_size_t(int(ws.numel()) * int(ws.element_size()))
    _term_call("shine_ray_step", octree, t.handle, C.byref(cfg), src.data_ptr(), idx.data_ptr() if idx is not None else None,
               weight.data_ptr() if eik else None, sample_depth.data_ptr(), ray_depth.data_ptr(), sigma_size.data_ptr(), S,
               1 if neus_on else 0, n_surf.data_ptr() if eik else None, int(n_surf.numel()) if eik else 0, n,
               *_term_ptrs(octree, mlp, gfeat, gmlp), sigma_grad.data_ptr() if sigma_grad is not None else None,
               pred_out.data_ptr() if pred_out is not None else None, dpred_out.data_ptr() if dpred_out is not None else None,
               out.data_ptr(), ws.data_ptr(), C.byref(ws_bytes))
    return out.view(())


def octree_interp(octree, coord):
    """FeatureOctree.query_feature (model/feature_octree.py:237-244) -> [N,8]; also fills hierarchical_indices."""
    needs_grad = torch.is_grad_enabled() and (
        coord.requires_grad or any(p.requires_grad for p in octree.hier_features)
    )
    if needs_grad:
        ext = _ext.module()
        if ext is not None and coord.is_cuda and octree.featured_level_num <= 4:
            return _ext_query(ext, octree, coord)  # the C++ node (csrc/shine_torch_ext.cpp)
        return autograd_ops.OctreeInterp.apply(coord, octree, *octree.feature_list())
    return _interp_forward(octree, coord)


def _ext_query(ext, octree, coord):
    """autograd_ops.OctreeInterp.forward on the C++ side: shine_forward, with the decoder that consumed this octree's features
    last riding on the launch (FeatureSource.speculated)."""
    octree._require_tables()
    dec = octree.__dict__.get("_spec_decoder")
    dec = dec() if dec is not None else None
    mlp = dec.fused_params() if (dec is not None and dec.fusable) else []
    if mlp and not dec._params_on(coord.device, mlp):
        mlp = []
    st = octree._ext_state(ext)
    octree._reg_rider(st)  # (incremental mapping: cal_regularization's value rides on this launch — set up once per frame)
    feat, pred, reg = ext.query_feature(st, coord, octree.feature_list(), mlp)
    octree.__dict__["_spec_result"] = (pred, dec, mlp, autograd_ops.param_epoch(), [p._version for p in mlp]) if mlp else None
    octree._defer_indices(coord)
    octree.__dict__["_reg_riding"] = reg  # None, or this query's regulariser (a view of the rider's ring: clone to keep)
    if reg is not None:  # ... of the tensors as they are now (cal_regularization evaluates at call time)
        octree.__dict__["_reg_riding_versions"] = octree._reg_versions()
    return feat


def _interp_forward(octree, coord, want_indices=True, mlp=None, pred_out=None):
    """query_feature's forward (shine_forward: interpolation only).  want_indices=False: hierarchical_indices is not written
    (the octree computes it from `coord` if somebody reads it, FeatureOctree.hierarchical_indices)."""
    t = octree._require_tables()
    c = octree._check_coord(coord.detach())
    n = c.shape[0]
    feat = torch.empty((n, 8), dtype=torch.float32, device=c.device)
    idx = [torch.empty((n, 8), dtype=torch.int64, device=c.device) for _ in range(octree.featured_level_num)] \
        if want_indices else None
    cfg = octree.step_config()
    _lib.check(
        _lib.lib().shine_forward(
            t.handle, C.byref(cfg), c.data_ptr(), n, octree.feature_ptrs(), octree.row_counts(),
            _lib.ptr_array([p.data_ptr() for p in mlp]) if mlp is not None else None, feat.data_ptr(),
            pred_out.data_ptr() if pred_out is not None else None,
            _lib.ptr_array([o.data_ptr() for o in idx]) if idx is not None else None, None, _stream(),
        ),
        "shine_forward",
    )
    if idx is not None:
        octree.hierarchical_indices = idx
    else:
        octree._defer_indices(c)
    return feat


_DUMMY = {}
_WORKSPACE = {}


def _workspace(dev, cfg):
    """Scratch for the fused step (per-workgroup partial sums): one buffer per (device, stream), for the life of the process.

    It is allocated ONCE at the size of the largest launch geometry (the workgroup count is capped, so the bound is ~3 MB)
    and never replaced: a captured HIP graph (loop.GraphedIteration, bench.py) bakes its address in, so swapping it for a
    bigger one later would leave the graph writing into freed memory.  Per STREAM, because the partial sums of a step live
    in it between the step's two launches: two steps in flight on different streams (a graph replaying on its capture
    stream next to eager launches, two models in one process) must not share them."""
    key = (str(dev), int(_stream() or 0))
    ws = _WORKSPACE.get(key)
    if ws is None:
        nbytes = int(_lib.lib().shine_train_step_workspace_bytes(C.byref(cfg), -1))  # bound for any batch size
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _WORKSPACE[key] = ws
    return ws


def _dummy_mlp(dev):
    key = str(dev)
    if key not in _DUMMY:
        _DUMMY[key] = [torch.zeros(s, dtype=torch.float32, device=dev) for s in (256, 32, 1024, 32, 32, 1)]
    return _DUMMY[key]


def fused_regularization(octree, lambda_forget: float, touched, out=None, out_zeroed=False, keep_flags=False):
    """FeatureOctree.cal_regularization (model/feature_octree.py:246-255) on the rows the last fused step touched.

    Returns the UNWEIGHTED regulariser as a 0-dim float64 device tensor and adds lambda * d(reg)/dF into the feature
    grads of the levels whose features_last_frame copy is detached (octree._reg_grad_on; the reference's attached
    clone, :160, contributes value only).  `touched`: the per-level uint8 flag tensors passed to fused_train_step.
    `keep_flags`: the flags double as the optimiser's sticky active-row flags (FusedAdam.step(row_flags=touched)) — they are
    left as they are, and only the rows flagged by THIS iteration's step (bit 0) enter the regulariser."""
    import ctypes as _C

    L = octree.featured_level_num
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=octree.feature_list()[0].device)
        out_zeroed = False
    feats = octree.feature_list()
    last = [t.detach().contiguous() for t in octree.features_last_frame]
    imp = [t.contiguous() for t in octree.importance_weight]
    grads = [_dense_grad(p) for p in feats]
    grad_on = (_C.c_int32 * L)(*[1 if g else 0 for g in octree._reg_grad_on])
    _lib.check(
        _lib.lib().shine_regularize(
            L, _lib.ptr_array([t.data_ptr() for t in feats]), _lib.ptr_array([t.data_ptr() for t in last]),
            _lib.ptr_array([t.data_ptr() for t in imp]), _lib.ptr_array([g.data_ptr() for g in grads]),
            _lib.ptr_array([t.data_ptr() for t in touched]), octree.row_counts(), grad_on, float(lambda_forget),
            out.data_ptr(), 1 if out_zeroed else 0, 1 if keep_flags else 0, _stream(),
        ),
        "shine_regularize",
    )
    return out[0]


def touched_flags(octree):
    """Per-level uint8 row flags for fused_train_step(touched=...) / fused_regularization (zero-initialised; views of one
    buffer: one fill)."""
    feats = octree.feature_list()
    sizes = [(int(p.shape[0]) + 15) // 16 * 16 for p in feats]
    flat = torch.zeros(sum(sizes), dtype=torch.uint8, device=feats[0].device)
    out, off = [], 0
    for p, sz in zip(feats, sizes):
        out.append(flat[off:off + int(p.shape[0])])
        off += sz
    return out
