"""GraphedIteration — one training iteration captured in a HIP graph and replayed (launch-bound inner loops belong in
hipGraphs).

The reference's inner loop (shine_batch.py:105-210, shine_incre.py:114-181) at its own batch size (4096) is bound by the
host: ~7 kernel launches per iteration at ~100 us of Python/driver time against ~75 us of GPU time.  This helper captures

    loss = fused_train_step(..., pool=pool, idx=idx)          query + decode + loss + backward (the fused kernel only)
    opt.finish_iteration(...)                                 sums of the kernel's partial vectors + [regulariser,
                                                              incremental mapping only] + fused dense Adam + grads cleared
                                                              + idx = pool.draw(n) for the NEXT iteration (sorted batch
                                                              from the node-ordered pool; the first one is drawn up front)

once and replays it.  The scalars that change per iteration — the sampler's stream id and Adam's step count — live in
device memory and are advanced by the kernels themselves (shine_sample_sorted_dev / shine_adam_step_dev), so every
replay draws a fresh batch and applies the right bias correction.  Learning-rate decay stays outside the graph
(`opt.sync_lr()` after changing `param_groups`).  Re-create after `octree.update()` (parameters are re-allocated, like
the optimiser itself, shine_incre.py:108-109).

The routes, chosen by the constructor's arguments (a term or a combination outside this table is refused with a ValueError before
anything is allocated):

    route            launches per iteration                           needs                                    refuses
    ---------------  -----------------------------------------------  ---------------------------------------  ----------------------
    plain            fused step, tail — the library-built graph       a SortedPool; FusedAdam for the fold     —
                     (`native`) while n + 1 <= 16 K; not folded:      (else {step, [regulariser], Adam} as a
                     step, [regulariser], Adam                        captured stream graph)
    + sem=           + ops.fused_sem_step after the fused step;       the fold; SortedPool(sem_label=);        —
      SemTerm        + the head's own Adam launch after the tail      the head's six tensors all trained or
                     while the head trains                            all frozen
    + normal=        + ops.fused_normal_step after sem's; its grads   the fold; SortedPool(normal_label=)      —
      NormalTerm     land in the tensors the tail steps
    + consistency=   + ops.fused_consistency_step, last before the    the fold                                 lambda_forget != 0 (the
      Consistency-   tail: it draws K = min(count, n) pairs from a                                             reference regularises
      Term           draw state this object owns and flags the rows                                            coord_near's rows, an
                     its shifted points reach for the active-row Adam                                          accident of call order)
    time             draw, ops.fused_time_step, the optimiser's       a time-conditioned decoder in the        lambda_forget != 0,
                     graph-safe step with zero_grad (a captured       fusable shape (decoder.time_fusable);    sem=, normal=,
                     stream graph: not folded, `native` off)          SortedPool(ts=)                          consistency=
    ray=RayTerm      draw of n RAYS (+ the batch's surface count      a sampler.RayPool; the optimiser of      a time-conditioned
                     with the eikonal term), ops.fused_ray_step,      setup_optimizer(..., sigma_size) with    decoder, lambda_forget
                     the optimiser's graph-safe step with zero_grad   config.ray_loss: its step moves          != 0, sem=, normal=,
                     (as the time route)                              sigma_size too                           consistency=

The terms join one iteration in the order {fused, [sem], [normal], [consistency], tail, [head Adam]} on the batch the fused step read.
"""
import ctypes as C
from dataclasses import dataclass
from functools import partial

import torch

from . import _lib, autograd_ops
from .autograd_ops import bump_param_epoch
from .autograd_ops import CONSISTENCY_WORKSPACE_BYTES, NORMAL_WORKSPACE_BYTES, SEM_WORKSPACE_BYTES
from .ops import (StepOptions, fused_consistency_step, fused_normal_step, fused_ray_step, fused_regularization, fused_sem_step,
                  fused_time_step, fused_train_step, touched_flags)


@dataclass
class SemTerm:
    """The semantic term of GraphedIteration(sem=...): the semantic decoder (Decoder(config, is_geo_encoder=False)), the
    reference's config.weight_s and config.sem_label_decimation (shine_batch.py:132-133,200-204)."""

    decoder: object
    weight_s: float = 1.0
    decimation: int = 1


@dataclass
class NormalTerm:
    """The surface-normal term of GraphedIteration(normal=...): the reference's config.weight_n (normal_loss_on,
    shine_batch.py:192-197); the labels are the pool's (SortedPool(normal_label=...))."""

    weight_n: float = 0.01


@dataclass
class ConsistencyTerm:
    """The gradient-consistency term of GraphedIteration(consistency=...): the reference's config.weight_c, config.consistency_count
    and shift_scale = consistency_range * scale in the [-1,1] space (consistency_loss_on, shine_batch.py:149-158,187-190; the
    default is the reference's 0.1 m at a scale of 0.02); `seed`: of the pairs' own draws."""

    weight_c: float = 1.0
    count: int = 1000
    shift_scale: float = 0.002
    seed: int = 0


@dataclass
class RayTerm:
    """The ray route of GraphedIteration(ray=...): the learnable sigma_size of the rendering loss (a CUDA float32 tensor of one
    element, in the optimiser's last group: setup_optimizer(config, feats, geo_params, None, sigma_size) with config.ray_loss) and
    main_loss_type dr (False) / dr_neus (True) (shine_batch.py:160-170); the pool is a sampler.RayPool."""

    sigma_size: object
    neus_on: bool = False


_CAPTURE_STREAM = {}


def _capture(fn):
    """Capture fn() into a new HIP graph on a side stream -> (graph, fn's result).  What `with torch.cuda.graph(g)` does,
    minus its gc.collect() + torch.cuda.empty_cache(): incremental mapping re-captures the iteration every frame
    (the parameters are re-allocated when the octree grows), and emptying the allocator's cache each time makes the next
    frame's allocations go back to hipMalloc."""
    dev = torch.cuda.current_device()
    side = _CAPTURE_STREAM.get(dev)
    if side is None:
        side = _CAPTURE_STREAM[dev] = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize(dev)  # nothing of the eager warm-up (non-blocking copies, allocator activity) straddles the capture
    main = torch.cuda.current_stream()
    side.wait_stream(main)
    out, err = None, None
    try:
        with torch.cuda.stream(side):
            g.capture_begin()
            try:
                out = fn()
            except BaseException as e:  # keep the ORIGINAL error: ending a broken capture may raise one of its own
                err = e
            try:
                g.capture_end()
            except BaseException as e2:
                if err is None:
                    err = e2
    finally:
        main.wait_stream(side)  # the main stream re-joins the side stream on every path
    if err is not None:
        raise err
    return g, out


_WARMED = set()  # devices on which an iteration has run eagerly in this process


class IterationGraph:
    """A library-built HIP graph of `unroll` iterations (include/shine_hip.h shine_iter_graph_*): kernel nodes created from the
    launches fused_train_step(pending=..., graph=self) and FusedAdam.finish_iteration(..., graph=self) would make, re-bound in
    place (commit) when the buffers change — a new frame of incremental mapping costs no capture and no instantiation."""

    _cache = {}

    def __init__(self, unroll):
        self.unroll = int(unroll)
        self.handle = C.c_void_p()
        self.owner = None  # the GraphedIteration whose buffers the nodes currently name
        _lib.check(_lib.lib().shine_iter_graph_create(self.unroll, C.byref(self.handle)), "shine_iter_graph_create")
        self.image = None  # the decoder's operand image for small-batch steps: torch's allocation, handed to the graph

    def ensure_image(self, dev):
        if self.image is None or self.image.device != torch.device(dev):
            lib = _lib.lib()
            self.image = torch.empty(int(lib.shine_iter_graph_operand_image_floats()), dtype=torch.float32, device=dev)
            _lib.check(lib.shine_iter_graph_set_operand_image(self.handle, self.image.data_ptr()), "shine_iter_graph_set_operand_image")

    @classmethod
    def shared(cls, device, unroll, slot=0):
        """one graph per (device, unroll, slot) for the life of the process: incremental mapping builds a GraphedIteration per
        frame.  `slot`: a loop that lets the host run a frame ahead of the device alternates two slots — re-binding a graph waits
        for that graph's own last replay (shine_iter_graph_commit), and the other slot's replays are the ones still running"""
        key = (str(device), int(unroll), int(slot))
        g = cls._cache.get(key)
        if g is None:
            g = cls._cache[key] = cls(unroll)
        return g

    def commit(self):
        _lib.check(_lib.lib().shine_iter_graph_commit(self.handle), "shine_iter_graph_commit")

    def launch(self, replays):
        _lib.check(_lib.lib().shine_iter_graph_launch(self.handle, int(replays), _lib.current_stream_handle()),
                   "shine_iter_graph_launch")

    def stats(self):
        c, b = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().shine_iter_graph_stats(self.handle, C.byref(c), C.byref(b)), "shine_iter_graph_stats")
        return int(c.value), int(b.value)

    def __del__(self):
        try:
            if self.handle:
                _lib.lib().shine_iter_graph_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass


class GraphedIteration:
    """`eager_first` (default True): the constructor runs iteration 1 eagerly (it allocates the optimiser state and loads the
    kernels outside the capture), so a frame of K iterations is the constructor + run(K - 1).  False: nothing runs in the
    constructor — the optimiser's device state is created explicitly and the graph is captured straight away, so a frame is
    run(K); honoured only once an eager iteration has run on the device in this process (incremental mapping re-creates this
    object every frame: the eager iteration costs ~0.1 ms of launches that a replay does in a third of the time).
    `sem`, `normal`, `consistency`, `ray`: the terms and routes of the module docstring's table.  `sem_loss`, `normal_loss` and
    `consistency_loss` are the terms' 0-dim device tensors (None without the term) and `consistency_draws` = (near_index [K],
    shift [K,3]) holds the last iteration's pairs; on the time and ray routes (`time` is True / `ray` is the RayTerm) `loss` is the
    route's step's."""

    def __init__(self, octree, decoder, pool, opt, opts: StepOptions, n: int, lambda_forget: float = 0.0, unroll: int = 1,
                 fold: bool = True, eager_first: bool = True, active_rows: bool = True, native: bool = True, graph_slot: int = 0,
                 sem: SemTerm = None, *, normal: NormalTerm = None, consistency: ConsistencyTerm = None, ray: RayTerm = None):
        self.octree, self.decoder, self.pool, self.opt, self.opts, self.n = octree, decoder, pool, opt, opts, int(n)
        self.lambda_forget = float(lambda_forget)
        self.graph_slot = int(graph_slot)
        self.sem, self.normal, self.consistency, self.ray = sem, normal, consistency, ray
        self.time = bool(getattr(decoder, "time_fusable", False))
        # the single-launch routes (ray, time): {draw, the route's step, graph-safe Adam} — the non-folded form
        if self.ray is not None or hasattr(pool, "surf_per_ray") or self.time:
            fold = native = False
        self.fold = bool(fold)  # the iteration's tail as one launch (False: reduction, regulariser and Adam as three)
        self.regularize = self.lambda_forget != 0.0
        can_fold = self.fold and hasattr(opt, "finish_iteration") and hasattr(opt, "prepare_graph_safe")
        self._check_arguments(can_fold)  # (before anything is allocated)
        # EXACT active-row Adam (FusedAdam.finish_iteration(active_flags=...)): rows that have had no gradient since `opt` was
        # created are not read.  Valid for an optimiser that is new (this object creates the flags cleared, so it must be built
        # together with the optimiser, as shine_incre.py:107-109 does every frame) and whose feature groups carry no weight decay
        # (the reference's groups, utils/tools.py:68-72).
        feat_ids = {id(p) for p in octree.hier_features}
        feat_wd = [float(g.get("weight_decay", 0.0)) for g in getattr(opt, "param_groups", [])
                   if any(id(p) in feat_ids for p in g["params"])]
        fresh = getattr(opt, "steps_taken", lambda: 1)() == 0
        self.active_rows = bool(active_rows and can_fold and fresh and feat_wd and all(w == 0.0 for w in feat_wd))
        self.touched = touched_flags(octree) if (self.regularize or self.active_rows) else None
        self._epoch = octree._tables_epoch
        self._idx = torch.empty(self.n, dtype=torch.int32, device=pool.coord.device)
        # the eikonal term's surface count: per-block partial counts written by the draw itself, summed by the step's kernels
        # (... and the normal term's: both divide by the batch's surface count)
        if self.ray is not None:
            self._surf = pool.surf_buffer() if opts.ekional_loss_on else None
        else:
            self._surf = pool.surf_parts_buffer(self.n) if (opts.ekional_loss_on or self.normal is not None) else None
        self.loss = self.reg = None
        self._reg_out = torch.zeros(1, dtype=torch.float64, device=pool.coord.device) if self.regularize else None
        self._hooked = None  # StepOptions with the iteration hooks (made once the optimiser has its device state)
        self._ahead = False
        dev_key = str(pool.coord.device)
        # `native`: the graph is BUILT by the library from the two launches of an iteration and re-bound in place for this
        # object's buffers (IterationGraph) instead of being captured from the stream — nothing to warm up, nothing to capture:
        # the constructor runs no iteration whatever `eager_first` says.  Needs the two-launch iteration (fold, the next draw
        # inside the tail: n < 16 K) without a term: the library-built graph holds exactly those two launches.
        terms = sem is not None or normal is not None or consistency is not None
        self.native = bool(native and can_fold and self.n + 1 <= 16 * 1024 and not terms)
        self._init_buffers()
        self.ran_eager = (not self.native) and (bool(eager_first) or dev_key not in _WARMED or not can_fold)
        if can_fold:
            # the optimiser's device-side step state up front: the eager warm-up iteration then runs the SAME two launches the
            # graph replays (with active rows it has to: its rows must end up flagged "touched earlier")
            if sem is None:
                self.opt.prepare_graph_safe()
            else:  # (the head's lout never receives a gradient, model/decoder.py:89-101: it stays out of the stepped set)
                skip = list(sem.decoder.lout.parameters())
                if hasattr(decoder, "nclass_out"):  # (nor does the geometry decoder's class layer)
                    skip += list(decoder.nclass_out.parameters())
                self.opt.prepare_graph_safe(skip=skip)
        if self.ran_eager:
            # eager warm-up: allocates workspaces and optimiser state and loads the kernels outside the capture
            self.loss, self.reg = self._body()
            _WARMED.add(dev_key)
        # From here on the optimiser's launch also draws the NEXT iteration's batch (a few extra blocks, no launch of its own):
        # an iteration is {fused kernel, tail}.  `_idx` then holds the batch of the iteration to come; it is primed here.
        self._ahead = (self.fold and hasattr(self.opt, "finish_iteration") and hasattr(self.opt, "device_state")
                       and self.opt.device_state() is not None and self.n + 1 <= 16 * 1024)
        if self._ahead:
            self.pool.draw(self.n, out=self._idx, graph_safe=True, surf_parts=self._surf)
        # `unroll` iterations in ONE graph: an iteration is two small launches, and every graph boundary leaves the GPU idle
        # for ~8 us — run(n) replays the long graph n // unroll times.  A captured node costs ~16 us, so it pays when the
        # boundaries saved outweigh the nodes captured (a frame of 50 iterations: unroll 5, bench.py --unroll).  Both graphs
        # are captured when first needed: a frame whose length is a multiple of `unroll` never captures the one-iteration graph.
        self.unroll = max(1, int(unroll))
        # `loss` / `reg` always name the outputs of the launch that ran LAST (eager, one-iteration graph or unrolled graph:
        # each capture has its own output tensors)
        self.graph = self.graph_k = None
        self._out_1 = self._out_k = None
        self._native = {}  # unroll -> (IterationGraph, outputs, keep-alive) bound to this object's buffers

    def _term_buffers(self, nbytes):
        """(workspace, out, loss) of one term step: a zeroed workspace of its own (the captured graph holds the address), the
        one-element tensor the step writes, and the 0-dim view of it that the loop hands out"""
        dev = self.pool.coord.device
        ws = _lib.zeroed_workspace(nbytes, dev)
        out = torch.zeros(1, dtype=torch.float32, device=dev)
        return ws, out, out[0]

    def _init_buffers(self):
        """the buffers of the terms and of a single-launch route's step, all made here: a captured graph bakes their addresses in"""
        dev = self.pool.coord.device
        self.sem_loss = self.normal_loss = self.consistency_loss = self.consistency_draws = self._route = None
        if self.sem is not None:
            head = list(self.sem.decoder.sem_params())
            self._sem_head = head if head[0].requires_grad else []  # (the tensors of the head's own Adam launch)
            self._sem_ws, self._sem_out, self.sem_loss = self._term_buffers(SEM_WORKSPACE_BYTES)
        if self.normal is not None:
            self._normal_ws, self._normal_out, self.normal_loss = self._term_buffers(NORMAL_WORKSPACE_BYTES)
        if self.consistency is not None:
            k = self._consistency_k = min(int(self.consistency.count), self.n)
            self._consistency_ws, self._consistency_out, self.consistency_loss = self._term_buffers(CONSISTENCY_WORKSPACE_BYTES)
            self._consistency_state = torch.zeros(1, dtype=torch.int64, device=dev)  # the pairs' stream id, advanced by the kernel
            self.consistency_draws = (torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros((k, 3), dtype=torch.float32, device=dev))
        # a single-launch route: (the draw's surface-count keyword, the step but for its idx=, the loss the step writes); `_surf`
        # exists with the eikonal term only
        if self.ray is not None or self.time:
            nbytes = autograd_ops.ray_step_workspace_bytes() if self.ray is not None else autograd_ops.time_step_workspace_bytes()
            ws, out, loss = self._term_buffers(nbytes)
            batch = dict(n_surf=self._surf, pool=self.pool, out=out, workspace=ws)
            if self.ray is not None:
                self._route = ("surf_out", partial(fused_ray_step, self.octree, self.decoder, None, None, None, None,
                                                   self.ray.sigma_size, self.opts, None, neus_on=bool(self.ray.neus_on), **batch), loss)
            else:
                self._route = ("surf_parts", partial(fused_time_step, self.octree, self.decoder, None, None, None, None, self.opts,
                                                     **batch), loss)

    def _refuse_terms(self, wording):
        for name, term in (("sem", self.sem), ("normal", self.normal), ("consistency", self.consistency)):
            if term is not None:
                raise ValueError(wording % name)

    def _check_arguments(self, can_fold):
        """every argument error of the constructor, in the order ray, time, consistency, sem, normal"""
        pool, sem, term = self.pool, self.sem, self.consistency
        if self.ray is not None or hasattr(pool, "surf_per_ray"):
            if self.ray is None:
                raise ValueError("GraphedIteration with a RayPool needs ray=RayTerm(sigma_size, neus_on)")
            if not hasattr(pool, "surf_per_ray"):
                raise ValueError("GraphedIteration(ray=...) needs a sampler.RayPool (LiDARDataset.ray_pool())")
            if self.time or getattr(self.decoder, "is_time_conditioned", False):
                raise ValueError("GraphedIteration(ray=...) does not serve a time-conditioned decoder: the ray step decodes with the "
                                 "plain head")
            if self.regularize:
                raise ValueError("GraphedIteration(ray=...) does not serve lambda_forget != 0")
            self._refuse_terms("GraphedIteration(ray=...) does not serve %s=: ray mode combined with the other terms is out of scope")
        if self.time:
            if getattr(pool, "ts", None) is None:
                raise ValueError("GraphedIteration with a time-conditioned decoder needs a SortedPool built with ts=")
            if self.regularize:
                raise ValueError("GraphedIteration with a time-conditioned decoder does not serve lambda_forget != 0 yet")
            self._refuse_terms("GraphedIteration with a time-conditioned decoder does not serve %s= yet: its kernel decodes with the "
                               "plain head")
        if term is not None:
            if not can_fold:
                raise ValueError("GraphedIteration(consistency=...) needs the folded iteration (fold=True, a FusedAdam optimiser)")
            if self.regularize:
                raise ValueError("GraphedIteration(consistency=...) is not served with lambda_forget != 0: the reference regularises "
                                 "the rows of its last query_feature call (coord_near's), an accident of call order")
            if int(term.count) < 0 or not float(term.shift_scale) >= 0.0:
                raise ValueError("ConsistencyTerm: count >= 0 and shift_scale >= 0 (consistency_range * scale)")
        if sem is not None:
            if not can_fold:
                raise ValueError("GraphedIteration(sem=...) needs the folded iteration (fold=True, a FusedAdam optimiser)")
            if getattr(pool, "sem_label", None) is None:
                raise ValueError("GraphedIteration(sem=...) needs a SortedPool built with sem_label=")
            if int(sem.decimation) < 1:
                raise ValueError("sem_label_decimation must be >= 1")
            train = [p.requires_grad for p in sem.decoder.sem_params()]
            if any(train) != all(train):
                raise ValueError("the semantic head's six tensors must all train or all be frozen")
        if self.normal is not None:
            if not can_fold:
                raise ValueError("GraphedIteration(normal=...) needs the folded iteration (fold=True, a FusedAdam optimiser)")
            if getattr(pool, "normal_label", None) is None:
                raise ValueError("GraphedIteration(normal=...) needs a SortedPool built with normal_label=")

    def _graph_1(self):
        if self.graph is None:
            self.graph, self._out_1 = _capture(self._body)
        return self.graph

    def _graph_unrolled(self):
        if self.graph_k is None:
            def body_k():
                out = None
                for _ in range(self.unroll):
                    out = self._body()
                return out

            self.graph_k, self._out_k = _capture(body_k)
        return self.graph_k

    def _bound(self, unroll):
        """the library-built graph of `unroll` iterations, its kernel nodes naming this object's buffers"""
        ent = self._native.get(unroll)
        g = ent[0] if ent is not None else IterationGraph.shared(self.pool.coord.device, unroll, self.graph_slot)
        if ent is None or g.owner is not self:
            g.ensure_image(self.pool.coord.device)
            keep = {}
            out = self._body(graph=g, keep=keep)
            g.commit()
            g.owner = self
            ent = self._native[unroll] = (g, out, keep)
        return ent

    def _route_body(self):
        """a single-launch route's iteration: draw (n rays on the ray route), the one-launch step on pool / idx, the optimiser's
        graph-safe step"""
        count_kw, step, loss = self._route
        step(idx=self.pool.draw(self.n, out=self._idx, graph_safe=True, **{count_kw: self._surf}))
        self.opt.step(zero_grad=True, graph_safe=True)
        return loss, None

    def _body(self, graph=None, keep=None):
        if self._route is not None:
            return self._route_body()
        idx = self._idx if self._ahead else self.pool.draw(self.n, out=self._idx, graph_safe=True, surf_parts=self._surf)
        n_surf = self._surf if self.opts.ekional_loss_on else None
        # Iteration hooks: the step's reduction launch also counts the optimiser step (+ bias corrections) and clears the
        # regulariser's accumulator, so neither costs a launch of its own (an iteration at N = 4096 is a chain of small
        # launches: each one removed saves its run time and ~2 us of dependency gap).  The optimiser's device state exists
        # after its first graph-safe step — the eager warm-up call below runs unhooked and creates it.
        state = self.opt.device_state() if hasattr(self.opt, "device_state") else None
        hooked = state is not None
        if hooked and (self._hooked is None or self._hooked.adam_state is not state):
            import copy

            self._hooked = copy.copy(self.opts)
            self._hooked.adam_state, self._hooked.adam_betas = state, tuple(self.opt.betas)
            self._hooked.zero_f64 = self._reg_out
        opts = self._hooked if hooked else self.opts
        # hooked (every iteration but the eager warm-up): the fused kernel only, then ONE launch for {sums of its partial
        # vectors, regulariser, Adam, clearing the grads} (FusedAdam.finish_iteration) — 3 launches per iteration instead of 5
        fold = hooked and self.fold and hasattr(self.opt, "finish_iteration")
        pending = {} if fold else None
        if graph is not None and not (fold and self._ahead):
            raise RuntimeError("the library-built iteration graph holds the two-launch iteration (fold, next draw in the tail)")
        loss, _, _ = fused_train_step(self.octree, self.decoder, None, None, None, opts, n_surf=n_surf, pool=self.pool,
                                      idx=idx, touched=self.touched, pending=pending, graph=graph)
        if keep is not None:
            keep["pending"] = pending  # (every device buffer the nodes name stays alive with this object)
        sem, term = self.sem, self.consistency
        if not fold:
            if sem is not None or self.normal is not None or term is not None:
                raise RuntimeError("GraphedIteration(sem=... / normal=... / consistency=...): the optimiser has no device-side step "
                                   "state")
            reg = None
            if self.regularize:
                reg = fused_regularization(self.octree, self.lambda_forget, self.touched, out=self._reg_out, out_zeroed=hooked)
            self.opt.step(zero_grad=True, graph_safe=True, advanced=hooked)
            return loss, reg
        # semantic_on / normal_loss_on / consistency_loss_on: each term's step on the batch the fused step just read (the fused step's
        # touched flags cover the rows of the first two; the consistency step flags the rows its shifted points add), the tail on the
        # feature tables + decoder — the normal and consistency terms' decoder grads are in the six tensors it steps —, and, while
        # the semantic head trains, the head's own Adam launch
        head = []
        if sem is not None:
            fused_sem_step(self.octree, sem.decoder, None, None, float(sem.weight_s), int(sem.decimation), pool=self.pool, idx=idx,
                           out=self._sem_out, workspace=self._sem_ws)
            head = self._sem_head
        if self.normal is not None:
            fused_normal_step(self.octree, self.decoder, None, None, None, float(self.normal.weight_n), n_surf=self._surf,
                              pool=self.pool, idx=idx, out=self._normal_out, workspace=self._normal_ws)
        if term is not None:  # (last: its flags join the fused step's before the tail reads them)
            fused_consistency_step(self.octree, self.decoder, None, float(term.weight_c), n_pairs=self._consistency_k,
                                   shift_scale=float(term.shift_scale), seed=int(term.seed), draw_state=self._consistency_state,
                                   pool=self.pool, idx=idx, touched=self.touched, out=self._consistency_out,
                                   workspace=self._consistency_ws, draws_out=self.consistency_draws)
        self.opt.finish_iteration(pending, dict(lambda_forget=self.lambda_forget, touched=self.touched,
                                                out=self._reg_out) if self.regularize else None,
                                  next_draw=self.pool.next_draw(self.n, self._idx, self._surf) if self._ahead else None,
                                  active_flags=self.touched if self.active_rows else None, graph=graph, others=head)
        if head:
            self.opt.step_tensors_dev(head)
        return loss, (self._reg_out[0] if self.regularize else None)

    def __call__(self):
        """Run one iteration; returns the loss of the fused terms as a 0-dim device tensor (no host sync)."""
        return self.run(1)

    def run(self, n_iters: int):
        """n_iters iterations: replays of the `unroll`-iteration graph, the remainder one by one.  Returns the last loss."""
        if self.octree._tables_epoch != self._epoch:
            raise RuntimeError("the octree grew since this iteration was captured: build a new GraphedIteration")
        bump_param_epoch()  # (replays update the parameters without torch noticing)
        k = self.unroll if self.unroll > 1 else 0
        if self.native:
            if k and n_iters >= k:
                g, out, _ = self._bound(k)
                g.launch(n_iters // k)
                self.loss, self.reg = out
                n_iters %= k
            if n_iters:
                g, out, _ = self._bound(1)
                g.launch(n_iters)
                self.loss, self.reg = out
            return self.loss
        while k and n_iters >= k:
            self._graph_unrolled().replay()
            self.loss, self.reg = self._out_k
            n_iters -= k
        for _ in range(n_iters):
            self._graph_1().replay()
            self.loss, self.reg = self._out_1
        return self.loss
