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

With `sem=SemTerm(...)` (semantic_on) the iteration is {fused step, semantic step, tail} on the same batch: the semantic step
(ops.fused_sem_step, one launch) adds weight_s * d NLL / d {features, head} to the grads the tail's Adam consumes, and while the
head trains its six tensors get one more graph-safe Adam launch of their own (the tail keeps its feature-table + decoder set).
With `normal=NormalTerm(...)` (normal_loss_on) the normal step (ops.fused_normal_step, one launch) joins the same way: its
feature and decoder grads land in the tensors the tail steps, so it needs no Adam launch of its own; with both terms the iteration
is {fused step, semantic step, normal step, tail, the head's Adam}.
With `consistency=ConsistencyTerm(...)` (consistency_loss_on) the consistency step (ops.fused_consistency_step, one launch) goes
after the fused step and the other terms and before the tail: {fused, [sem], [normal], consistency, tail, [head Adam]}.  It draws its
own K = min(count, n) pairs on the device from a draw state this object owns (advanced by the kernel: a replay draws fresh pairs)
and flags the rows its shifted points reach, so the active-row Adam steps and clears them.  Not served with the regulariser
(lambda_forget != 0): the reference then regularises the rows of its LAST query_feature call, coord_near's, an accident of call
order (shine_incre.py:144,156).

With a TIME-CONDITIONED decoder (config.time_conditioned: Decoder(config, is_time_conditioned=True) in the fusable shape,
decoder.time_fusable) the iteration takes the time route: {draw, ops.fused_time_step on pool / idx (one launch: BCE [+ eikonal]
through the 9-wide head and the whole backward), the optimiser's graph-safe step with zero_grad}, captured as a stream graph —
the non-folded form, `native` off.  The pool carries the time stamps (SortedPool(ts=...)).  Not served on that route yet:
lambda_forget != 0, sem=, normal=, consistency= (their kernels decode with the plain head).

With `ray=RayTerm(sigma_size, neus_on)` (config.ray_loss, main_loss_type dr / dr_neus) and a sampler.RayPool the iteration takes
the ray route: {ray_pool.draw of n RAYS (+ the batch's surface count with the eikonal term), ops.fused_ray_step on pool / idx (one
launch: the head, the per-ray render, [the eikonal term] and the whole backward, sigma_size's gradient included), the optimiser's
graph-safe step with zero_grad}, captured as a stream graph — the non-folded form, `native` off.  The optimiser is
setup_optimizer(config, feats, geo_params, None, sigma_size) with config.ray_loss: its step moves sigma_size with the tables and
the decoder.  Not served on that route: a time-conditioned decoder, lambda_forget != 0, sem=, normal=, consistency=.
"""
import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
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


class _IterationTerms(type):
    """GraphedIteration(..., normal=NormalTerm(...)): loss terms added after `sem` are keyword arguments of the CALL, set on the
    object before its constructor runs — the constructor's own parameter list is what existing callers (and the suite) spell out
    position by position, and it stays as it is.
    A stopgap with known costs: inspect.signature, a subclass that overrides __init__ / __new__ and a direct __init__ call do not
    see the keyword.  tests/test_sem_step.py::test_public_surface pins the constructor's exact parameter list and a change that adds
    a loss term may not edit existing tests; a later change should relax that pin to "the leading parameters and their defaults",
    move `normal` into the constructor and delete this class.  A third term now hangs on the hook: `consistency`
    (ConsistencyTerm) rides the same way, under the same constraint."""

    def __call__(cls, *args, normal=None, consistency=None, ray=None, **kw):
        self = cls.__new__(cls)
        self.normal = normal
        self.consistency = consistency
        self.ray = ray  # (the ray route's RayTerm: a fourth keyword on the same hook)
        self.__init__(*args, **kw)
        return self


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


class GraphedIteration(metaclass=_IterationTerms):
    """`eager_first` (default True): the constructor runs iteration 1 eagerly (it allocates the optimiser state and loads the
    kernels outside the capture), so a frame of K iterations is the constructor + run(K - 1).  False: nothing runs in the
    constructor — the optimiser's device state is created explicitly and the graph is captured straight away, so a frame is
    run(K); honoured only once an eager iteration has run on the device in this process (incremental mapping re-creates this
    object every frame: the eager iteration costs ~0.1 ms of launches that a replay does in a third of the time).
    `normal=NormalTerm(...)` (a keyword of the call, see _IterationTerms): the surface-normal term of the same batch as one more
    launch between the fused step and the tail (ops.fused_normal_step); `normal_loss` is its 0-dim device tensor.
    `consistency=ConsistencyTerm(...)` (a keyword of the call too): the gradient-consistency term as the last launch before the
    tail (ops.fused_consistency_step, pairs drawn on the device); `consistency_loss` is its 0-dim device tensor and
    `consistency_draws` = (near_index [K], shift [K,3]) holds the last iteration's pairs.  Raises ValueError with
    lambda_forget != 0.
    `decoder` time-conditioned (decoder.time_fusable): the time route of the module docstring — `time` is True, `pool` must carry
    `ts`, and lambda_forget != 0 / sem= / normal= / consistency= raise ValueError before anything is allocated."""

    def __init__(self, octree, decoder, pool, opt, opts: StepOptions, n: int, lambda_forget: float = 0.0, unroll: int = 1,
                 fold: bool = True, eager_first: bool = True, active_rows: bool = True, native: bool = True, graph_slot: int = 0,
                 sem: SemTerm = None):
        self.octree, self.decoder, self.pool, self.opt, self.opts, self.n = octree, decoder, pool, opt, opts, int(n)
        self.lambda_forget = float(lambda_forget)
        self.graph_slot = int(graph_slot)
        # the ray route (ray=RayTerm(...) and a RayPool): {draw, fused_ray_step, graph-safe Adam} — the non-folded form
        self.ray = getattr(self, "ray", None)
        if self.ray is not None or hasattr(pool, "surf_per_ray"):  # (argument errors before anything is allocated)
            self._check_ray(sem)
            fold = native = False
        # the time route (a time-conditioned decoder): {draw, fused_time_step, graph-safe Adam} — the non-folded form
        self.time = bool(getattr(decoder, "time_fusable", False))
        if self.time:  # (argument errors before anything is allocated)
            self._check_time(sem)
            fold = native = False
        self.fold = bool(fold)  # the iteration's tail as one launch (False: reduction, regulariser and Adam as three)
        self.regularize = self.lambda_forget != 0.0
        can_fold = self.fold and hasattr(opt, "finish_iteration") and hasattr(opt, "prepare_graph_safe")
        self.consistency = getattr(self, "consistency", None)
        if self.consistency is not None:  # (argument errors before anything is allocated)
            self._check_consistency(can_fold)
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
        self.normal = getattr(self, "normal", None)
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
        # inside the tail: n < 16 K).
        self.native = bool(native and can_fold and self.n + 1 <= 16 * 1024)
        self.sem = sem
        self.sem_loss = None
        if sem is not None:
            self._init_sem(can_fold)
        self.normal_loss = None
        if self.normal is not None:
            self._init_normal(can_fold)
        self.consistency_loss = self.consistency_draws = None
        if self.consistency is not None:
            self._init_consistency(can_fold)
        if self.time:  # the time step's buffers, made here: a captured graph bakes their addresses in
            from .autograd_ops import time_step_workspace_bytes

            self._time_ws, self._time_out, self._time_loss = self._term_buffers(time_step_workspace_bytes())
        if self.ray is not None:  # the ray step's buffers, made here too
            from .autograd_ops import ray_step_workspace_bytes

            self._ray_ws, self._ray_out, self._ray_loss = self._term_buffers(ray_step_workspace_bytes())
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

    def _init_sem(self, can_fold):
        """the semantic term's buffers, all made here: a captured graph bakes their addresses in"""
        sem = self.sem
        if not can_fold:
            raise ValueError("GraphedIteration(sem=...) needs the folded iteration (fold=True, a FusedAdam optimiser)")
        if getattr(self.pool, "sem_label", None) is None:
            raise ValueError("GraphedIteration(sem=...) needs a SortedPool built with sem_label=")
        if int(sem.decimation) < 1:
            raise ValueError("sem_label_decimation must be >= 1")
        self.native = False  # (the library-built graph holds the two-launch iteration)
        self._sem_params = list(sem.decoder.sem_params())
        train = [p.requires_grad for p in self._sem_params]
        if any(train) != all(train):
            raise ValueError("the semantic head's six tensors must all train or all be frozen")
        self._sem_train = all(train)
        self._sem_ws, self._sem_out, self.sem_loss = self._term_buffers(SEM_WORKSPACE_BYTES)

    def _init_normal(self, can_fold):
        """the normal term's buffers, all made here: a captured graph bakes their addresses in"""
        if not can_fold:
            raise ValueError("GraphedIteration(normal=...) needs the folded iteration (fold=True, a FusedAdam optimiser)")
        if getattr(self.pool, "normal_label", None) is None:
            raise ValueError("GraphedIteration(normal=...) needs a SortedPool built with normal_label=")
        self.native = False  # (the library-built graph holds the two-launch iteration)
        self._normal_ws, self._normal_out, self.normal_loss = self._term_buffers(NORMAL_WORKSPACE_BYTES)

    def _check_time(self, sem):
        if getattr(self.pool, "ts", None) is None:
            raise ValueError("GraphedIteration with a time-conditioned decoder needs a SortedPool built with ts=")
        if self.lambda_forget != 0.0:
            raise ValueError("GraphedIteration with a time-conditioned decoder does not serve lambda_forget != 0 yet")
        for name, term in (("sem", sem), ("normal", getattr(self, "normal", None)),
                           ("consistency", getattr(self, "consistency", None))):
            if term is not None:
                raise ValueError("GraphedIteration with a time-conditioned decoder does not serve %s= yet: its kernel decodes "
                                 "with the plain head" % name)

    def _check_ray(self, sem):
        if self.ray is None:
            raise ValueError("GraphedIteration with a RayPool needs ray=RayTerm(sigma_size, neus_on)")
        if not hasattr(self.pool, "surf_per_ray"):
            raise ValueError("GraphedIteration(ray=...) needs a sampler.RayPool (LiDARDataset.ray_pool())")
        if getattr(self.decoder, "time_fusable", False) or getattr(self.decoder, "is_time_conditioned", False):
            raise ValueError("GraphedIteration(ray=...) does not serve a time-conditioned decoder: the ray step decodes with the "
                             "plain head")
        if self.lambda_forget != 0.0:
            raise ValueError("GraphedIteration(ray=...) does not serve lambda_forget != 0")
        for name, term in (("sem", sem), ("normal", getattr(self, "normal", None)),
                           ("consistency", getattr(self, "consistency", None))):
            if term is not None:
                raise ValueError("GraphedIteration(ray=...) does not serve %s=: ray mode combined with the other terms is out of "
                                 "scope" % name)

    def _check_consistency(self, can_fold):
        term = self.consistency
        if not can_fold:
            raise ValueError("GraphedIteration(consistency=...) needs the folded iteration (fold=True, a FusedAdam optimiser)")
        if self.regularize:
            raise ValueError("GraphedIteration(consistency=...) is not served with lambda_forget != 0: the reference regularises "
                             "the rows of its last query_feature call (coord_near's), an accident of call order")
        if int(term.count) < 0 or not float(term.shift_scale) >= 0.0:
            raise ValueError("ConsistencyTerm: count >= 0 and shift_scale >= 0 (consistency_range * scale)")

    def _init_consistency(self, can_fold):
        """the consistency term's buffers, all made here: a captured graph bakes their addresses in"""
        term = self.consistency
        self.native = False  # (the library-built graph holds the two-launch iteration)
        dev = self.pool.coord.device
        k = self._consistency_k = min(int(term.count), self.n)
        self._consistency_ws, self._consistency_out, self.consistency_loss = self._term_buffers(CONSISTENCY_WORKSPACE_BYTES)
        self._consistency_state = torch.zeros(1, dtype=torch.int64, device=dev)  # the pairs' stream id, advanced by the kernel
        self.consistency_draws = (torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros((k, 3), dtype=torch.float32, device=dev))

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

    def _time_body(self):
        """the time route's iteration: draw, the one-launch step on pool / idx, the optimiser's graph-safe step"""
        idx = self.pool.draw(self.n, out=self._idx, graph_safe=True, surf_parts=self._surf)
        fused_time_step(self.octree, self.decoder, None, None, None, None, self.opts,
                        n_surf=self._surf if self.opts.ekional_loss_on else None, pool=self.pool, idx=idx, out=self._time_out,
                        workspace=self._time_ws)
        self.opt.step(zero_grad=True, graph_safe=True)
        return self._time_loss, None

    def _ray_body(self):
        """the ray route's iteration: draw n rays, the one-launch step on pool / idx, the optimiser's graph-safe step"""
        idx = self.pool.draw(self.n, out=self._idx, graph_safe=True, surf_out=self._surf)
        fused_ray_step(self.octree, self.decoder, None, None, None, None, self.ray.sigma_size, self.opts, None,
                       neus_on=bool(self.ray.neus_on), n_surf=self._surf, pool=self.pool, idx=idx, out=self._ray_out,
                       workspace=self._ray_ws)
        self.opt.step(zero_grad=True, graph_safe=True)
        return self._ray_loss, None

    def _body(self, graph=None, keep=None):
        if self.ray is not None:
            return self._ray_body()
        if self.time:
            return self._time_body()
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
        if self.sem is not None or self.normal is not None or self.consistency is not None:
            return self._terms_tail(idx, fold, pending, loss)
        if fold:
            self.opt.finish_iteration(pending, dict(lambda_forget=self.lambda_forget, touched=self.touched,
                                                    out=self._reg_out) if self.regularize else None,
                                      next_draw=self.pool.next_draw(self.n, self._idx, self._surf) if self._ahead else None,
                                      active_flags=self.touched if self.active_rows else None, graph=graph)
            return loss, (self._reg_out[0] if self.regularize else None)
        reg = None
        if self.regularize:
            reg = fused_regularization(self.octree, self.lambda_forget, self.touched, out=self._reg_out, out_zeroed=hooked)
        self.opt.step(zero_grad=True, graph_safe=True, advanced=hooked)
        return loss, reg

    def _terms_tail(self, idx, fold, pending, loss):
        """semantic_on / normal_loss_on / consistency_loss_on: each term's step on the batch the fused step just read (the fused
        step's touched flags cover the rows of the first two; the consistency step flags the rows its shifted points add), the tail
        on the feature tables + decoder — the normal and consistency terms' decoder grads are in the six tensors it steps —, and,
        while the semantic head trains, the head's own Adam launch"""
        if not fold:
            raise RuntimeError("GraphedIteration(sem=... / normal=... / consistency=...): the optimiser has no device-side step "
                               "state")
        sem, head = self.sem, []
        if sem is not None:
            fused_sem_step(self.octree, sem.decoder, None, None, float(sem.weight_s), int(sem.decimation), pool=self.pool, idx=idx,
                           out=self._sem_out, workspace=self._sem_ws)
            head = self._sem_params if self._sem_train else []
        if self.normal is not None:
            fused_normal_step(self.octree, self.decoder, None, None, None, float(self.normal.weight_n), n_surf=self._surf,
                              pool=self.pool, idx=idx, out=self._normal_out, workspace=self._normal_ws)
        if self.consistency is not None:  # (last: its flags join the fused step's before the tail reads them)
            term = self.consistency
            fused_consistency_step(self.octree, self.decoder, None, float(term.weight_c), n_pairs=self._consistency_k,
                                   shift_scale=float(term.shift_scale), seed=int(term.seed), draw_state=self._consistency_state,
                                   pool=self.pool, idx=idx, touched=self.touched, out=self._consistency_out,
                                   workspace=self._consistency_ws, draws_out=self.consistency_draws)
        self.opt.finish_iteration(pending, dict(lambda_forget=self.lambda_forget, touched=self.touched,
                                                out=self._reg_out) if self.regularize else None,
                                  next_draw=self.pool.next_draw(self.n, self._idx, self._surf) if self._ahead else None,
                                  active_flags=self.touched if self.active_rows else None, others=head)
        if head:
            self.opt.step_tensors_dev(head)
        return loss, (self._reg_out[0] if self.regularize else None)

    def __call__(self):
        """Run one iteration; returns the loss of the fused terms as a 0-dim device tensor (no host sync)."""
        if self.octree._tables_epoch != self._epoch:
            raise RuntimeError("the octree grew since this iteration was captured: build a new GraphedIteration")
        bump_param_epoch()
        if self.native:
            g, out, _ = self._bound(1)
            g.launch(1)
            self.loss, self.reg = out
            return self.loss
        self._graph_1().replay()
        self.loss, self.reg = self._out_1
        return self.loss

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
