"""loop.GraphedIteration on host fakes: which calls one iteration makes, in which order, and which buffers each call gets — for
every route the loop serves (the folded iteration with each subset of {sem, normal, consistency}, the head trained or frozen, the
regulariser where it is served, the library-built graph, the non-folded iteration, the time route and the ray route) — and what
the constructor's signature promises (the terms are keyword-only PARAMETERS: inspect.signature, a subclass that forwards **kw and
the up-front argument errors see them).

The step functions, the optimiser and the pool are recorders; "capturing" a graph runs the body once, as a stream capture does, and
a replay runs nothing.  What the kernels compute is the GPU suites' business (tests/test_gpu_*_step.py)."""
import inspect
import itertools

import pytest
import torch

from shine_mapping_amd import StepOptions, autograd_ops, loop

N = 16
TERMS = ("sem", "normal", "consistency")
SUBSETS = [tuple(t for t, on in zip(TERMS, bits) if on) for bits in itertools.product((False, True), repeat=3)]
TIME_WS, RAY_WS = 4096, 8192


class Octree:
    _tables_epoch = 0

    def __init__(self):
        self.hier_features = [torch.nn.Parameter(torch.zeros(5, 8)), torch.nn.Parameter(torch.zeros(9, 8))]

    def feature_list(self):
        return list(self.hier_features)


class Opt:
    """FusedAdam's surface as the loop uses it; the device-side step state appears with prepare_graph_safe() or the first step"""
    betas = (0.9, 0.99)

    def __init__(self, calls, feats):
        self.calls, self.state = calls, None
        self.param_groups = [dict(params=list(feats), weight_decay=0.0)]

    def steps_taken(self):
        return 0

    def device_state(self):
        return self.state

    def prepare_graph_safe(self, skip=()):
        self.calls.append(("prepare_graph_safe", dict(skip=list(skip))))
        self.state = torch.zeros(8, dtype=torch.int64)

    def step(self, **kw):
        self.calls.append(("opt.step", kw))
        if self.state is None:
            self.state = torch.zeros(8, dtype=torch.int64)

    def finish_iteration(self, pending, regulariser=None, **kw):
        self.calls.append(("finish_iteration", dict(kw, pending=pending, regulariser=regulariser)))

    def step_tensors_dev(self, tensors):
        self.calls.append(("step_tensors_dev", dict(tensors=tensors)))


class Pool:
    """SortedPool's surface: labels of every term, time stamps, draw / next_draw / surf_parts_buffer"""

    def __init__(self, calls):
        self.calls = calls
        self.coord = torch.zeros(4, 3)
        self.sem_label = torch.zeros(4, dtype=torch.int32)
        self.normal_label = torch.zeros(4, 3)
        self.ts = torch.zeros(4)
        self.parts = []

    def surf_parts_buffer(self, n=None):
        self.parts.append(torch.zeros(64, dtype=torch.int64))
        return self.parts[-1]

    def draw(self, n, out=None, graph_safe=False, **kw):
        self.calls.append(("draw", dict(kw, n=n, out=out, graph_safe=graph_safe)))
        return out

    def next_draw(self, n, out=None, surf_parts=None):
        return ("next_draw", n, out, surf_parts)


class Rays(Pool):
    """sampler.RayPool's surface: one surface count per batch, written by the draw (surf_out=)"""
    surf_per_ray = torch.zeros(4, dtype=torch.int32)

    def surf_parts_buffer(self, n=None):
        raise AssertionError("a RayPool has no partial counts")

    def surf_buffer(self):
        self.parts.append(torch.zeros(1, dtype=torch.int64))
        return self.parts[-1]


class SemDecoder:
    def __init__(self, trains):
        self.head = [torch.nn.Parameter(torch.zeros(2), requires_grad=trains) for _ in range(6)]
        self.lout = torch.nn.Linear(2, 2)

    def sem_params(self):
        return list(self.head)


class Graph:
    """what loop._capture hands back; a replay launches nothing on the host"""
    replays = 0

    def replay(self):
        self.replays += 1


class LibraryGraph:
    """loop.IterationGraph without the library: one per (device, unroll, slot)"""
    made = {}

    def __init__(self, calls):
        self.calls, self.owner = calls, None

    def ensure_image(self, dev):
        pass

    def commit(self):
        self.calls.append(("commit", {}))

    def launch(self, replays):
        self.calls.append(("launch", dict(replays=replays)))


class World:
    def __init__(self, monkeypatch, pool=Pool, time=False):
        calls = self.calls = []
        self.octree = Octree()
        self.decoder = type("Dec", (), {"time_fusable": True} if time else {})()
        self.pool = pool(calls)
        self.opt = Opt(calls, self.octree.hier_features)

        def recorder(name, result=None):
            def fn(*a, **kw):
                calls.append((name, dict(kw, args=a)))
                return result
            return fn

        self.fused_loss = torch.zeros((), dtype=torch.float64)
        monkeypatch.setattr(loop, "fused_train_step", recorder("fused", (self.fused_loss, None, None)))
        for short in ("sem", "normal", "consistency", "time", "ray"):
            monkeypatch.setattr(loop, "fused_%s_step" % short, recorder(short))
        self.reg_value = torch.zeros((), dtype=torch.float64)
        monkeypatch.setattr(loop, "fused_regularization", recorder("regularization", self.reg_value))
        for name, nbytes in (("time_step_workspace_bytes", TIME_WS), ("ray_step_workspace_bytes", RAY_WS)):
            monkeypatch.setattr(autograd_ops, name, lambda nbytes=nbytes: nbytes)
            monkeypatch.setattr(loop, name, lambda nbytes=nbytes: nbytes, raising=False)

        def capture(fn):
            calls.append(("capture", {}))
            return Graph(), fn()

        monkeypatch.setattr(loop, "_capture", capture)
        graphs = {}

        class Shared(LibraryGraph):
            @classmethod
            def shared(cls, device, unroll, slot=0):
                return graphs.setdefault((str(device), unroll, slot), cls(calls))

        monkeypatch.setattr(loop, "IterationGraph", Shared)

    def build(self, opts=None, **kw):
        opts = opts if opts is not None else StepOptions(sigma=0.1, ekional_loss_on=True)
        return loop.GraphedIteration(self.octree, self.decoder, self.pool, self.opt, opts, N, **kw)

    def take(self):
        """the calls since the last take()"""
        out = list(self.calls)
        del self.calls[:]
        return out


def names(calls):
    return [name for name, _ in calls]


def same_storage(a, b):
    return a.data_ptr() == b.data_ptr()


def term_objects(subset, head_trains=True):
    sem = loop.SemTerm(SemDecoder(head_trains), weight_s=0.5, decimation=2) if "sem" in subset else None
    kw = {}
    if "normal" in subset:
        kw["normal"] = loop.NormalTerm(0.05)
    if "consistency" in subset:
        kw["consistency"] = loop.ConsistencyTerm(weight_c=0.5, count=10, shift_scale=0.01, seed=3)
    return sem, kw


FOLDED = [(subset, head, lam) for subset in SUBSETS for head in ((True, False) if "sem" in subset else (True,))
          for lam in ((0.0, 0.25) if "consistency" not in subset else (0.0,))]


@pytest.mark.parametrize("subset,head_trains,lam", FOLDED,
                         ids=["%s-%s-%s" % ("+".join(s) or "plain", "head" if h else "frozen", "reg" if lam else "noreg")
                              for s, h, lam in FOLDED])
def test_the_folded_iteration_runs_fused_terms_tail_in_that_order_on_its_own_buffers(monkeypatch, subset, head_trains, lam):
    w = World(monkeypatch)
    sem, kw = term_objects(subset, head_trains)
    it = w.build(lambda_forget=lam, native=False, sem=sem, **kw)
    assert it.fold and not it.native and it.ran_eager and not it.time and it.ray is None
    assert it.regularize == (lam != 0.0) and it.active_rows and it.touched is not None
    head = sem.decoder.head if (sem is not None and head_trains) else []
    body = ["fused"] + list(subset) + ["finish_iteration"] + (["step_tensors_dev"] if head else [])

    built = w.take()
    # the constructor: the optimiser's device state, the eager iteration on a batch it draws itself, then the first batch primed
    assert names(built) == ["prepare_graph_safe", "draw"] + body + ["draw"]
    skip = built[0][1]["skip"]
    assert len(skip) == (2 if sem is not None else 0) and all(any(p is q for q in sem.decoder.lout.parameters()) for p in skip)
    assert it() is it.loss and it.loss is w.fused_loss
    first = w.take()
    assert names(first) == ["capture"] + body
    assert it() is it.loss and w.take() == []  # (a replay: the graph is captured once)

    surf = w.pool.parts[0]
    assert len(w.pool.parts) == 1 and it._surf is surf
    for name, d in [built[1], built[-1]]:
        assert d["out"] is it._idx and d["graph_safe"] is True and d["surf_parts"] is surf and d["n"] == N
    eager, replayed = dict(built[2:-1]), dict(first[1:])
    for run, ahead in ((eager, False), (replayed, True)):
        f = run["fused"]
        assert f["args"][:2] == (w.octree, w.decoder) and f["pool"] is w.pool and f["idx"] is it._idx
        assert f["n_surf"] is surf and f["touched"] is it.touched and f["graph"] is None
        assert f["pending"] is run["finish_iteration"]["pending"] and isinstance(f["pending"], dict)
        assert f["args"][5] is it._hooked and it._hooked.adam_state is w.opt.state and it._hooked.zero_f64 is it._reg_out
        fin = run["finish_iteration"]
        if lam:
            assert fin["regulariser"] == dict(lambda_forget=lam, touched=it.touched, out=it._reg_out)
            assert same_storage(it.reg, it._reg_out) and it.reg.dim() == 0
        else:
            assert fin["regulariser"] is None and it.reg is None and it._reg_out is None
        assert fin["active_flags"] is it.touched and fin.get("graph") is None
        assert fin["next_draw"] == (("next_draw", N, it._idx, surf) if ahead else None)
        if head:
            assert len(fin["others"]) == 6 and all(a is b for a, b in zip(fin["others"], head))
            assert all(a is b for a, b in zip(run["step_tensors_dev"]["tensors"], head))
        else:
            assert not fin.get("others")
        if "sem" in subset:
            s = run["sem"]
            assert s["args"] == (w.octree, sem.decoder, None, None, 0.5, 2) and s["pool"] is w.pool and s["idx"] is it._idx
            assert same_storage(it.sem_loss, s["out"]) and it.sem_loss.dim() == 0
        if "normal" in subset:
            s = run["normal"]
            assert s["args"] == (w.octree, w.decoder, None, None, None, 0.05) and s["pool"] is w.pool and s["idx"] is it._idx
            assert s["n_surf"] is surf and same_storage(it.normal_loss, s["out"]) and it.normal_loss.dim() == 0
        if "consistency" in subset:
            s = run["consistency"]
            assert s["args"] == (w.octree, w.decoder, None, 0.5) and s["pool"] is w.pool and s["idx"] is it._idx
            assert s["touched"] is it.touched and s["touched"] is not None
            assert (s["n_pairs"], s["shift_scale"], s["seed"]) == (10, 0.01, 3)
            assert s["draw_state"] is it._consistency_state and s["draws_out"] is it.consistency_draws
            assert same_storage(it.consistency_loss, s["out"]) and it.consistency_loss.dim() == 0
    for t in subset:  # one out and one workspace per term, the same in the eager iteration and in the captured one
        assert eager[t]["out"] is replayed[t]["out"] and eager[t]["workspace"] is replayed[t]["workspace"]
    outs, spaces = [eager[t]["out"] for t in subset], [eager[t]["workspace"] for t in subset]
    assert len({o.data_ptr() for o in outs}) == len(subset) and len({s.data_ptr() for s in spaces}) == len(subset)
    sizes = dict(sem=autograd_ops.SEM_WORKSPACE_BYTES, normal=autograd_ops.NORMAL_WORKSPACE_BYTES,
                 consistency=autograd_ops.CONSISTENCY_WORKSPACE_BYTES)
    for t in subset:
        assert eager[t]["workspace"].numel() * eager[t]["workspace"].element_size() == sizes[t]
        assert not eager[t]["workspace"].any()
    for absent in set(TERMS) - set(subset):
        assert getattr(it, absent + "_loss") is None
    assert (it.consistency_draws is None) == ("consistency" not in subset)


@pytest.mark.parametrize("lam", [0.0, 0.25])
def test_the_plain_iteration_is_the_library_built_two_launch_graph(monkeypatch, lam):
    w = World(monkeypatch)
    it = w.build(lambda_forget=lam)
    assert it.native and it.fold and not it.ran_eager and it.loss is None
    built = w.take()
    assert names(built) == ["prepare_graph_safe", "draw"] and built[0][1]["skip"] == []  # (no iteration runs in the constructor)
    assert it() is w.fused_loss
    first = w.take()
    assert names(first) == ["fused", "finish_iteration", "commit", "launch"] and first[3][1] == dict(replays=1)
    f, fin = first[0][1], first[1][1]
    g = f["graph"]
    assert isinstance(g, LibraryGraph) and g.owner is it and fin["graph"] is g and f["pending"] is fin["pending"]
    assert f["idx"] is it._idx and f["n_surf"] is it._surf and f["touched"] is it.touched
    assert fin["next_draw"] == ("next_draw", N, it._idx, it._surf) and fin["active_flags"] is it.touched and not fin.get("others")
    assert fin["regulariser"] == (dict(lambda_forget=lam, touched=it.touched, out=it._reg_out) if lam else None)
    assert (it.reg is None) if not lam else same_storage(it.reg, it._reg_out)
    assert it.run(3) is w.fused_loss
    assert w.take() == [("launch", dict(replays=3))]  # (bound once: the nodes name this object's buffers already)


@pytest.mark.parametrize("lam", [0.0, 0.25])
def test_the_non_folded_iteration_is_step_regulariser_and_the_optimisers_step(monkeypatch, lam):
    w = World(monkeypatch)
    it = w.build(lambda_forget=lam, fold=False)
    assert not it.fold and not it.native and it.ran_eager and not it.active_rows and (it.touched is not None) == bool(lam)
    body = ["draw", "fused"] + (["regularization"] if lam else []) + ["opt.step"]
    built = w.take()
    assert names(built) == body  # (no prepare_graph_safe, no draw ahead: the eager iteration creates the step state)
    assert built[1][1]["args"][5] is it.opts and built[-1][1] == dict(zero_grad=True, graph_safe=True, advanced=False)
    it()
    first = w.take()
    assert names(first) == ["capture"] + body
    run = dict(first[1:])
    assert run["draw"]["out"] is it._idx and run["draw"]["surf_parts"] is it._surf and run["draw"]["graph_safe"] is True
    assert run["fused"]["args"][5] is it._hooked and run["fused"]["pending"] is None and run["fused"]["idx"] is it._idx
    assert run["opt.step"] == dict(zero_grad=True, graph_safe=True, advanced=True)
    if lam:
        r = run["regularization"]
        assert r["args"] == (w.octree, lam, it.touched) and r["out"] is it._reg_out and r["out_zeroed"] is True
        assert it.reg is w.reg_value
    else:
        assert it.reg is None


@pytest.mark.parametrize("eik", [False, True], ids=["bce", "eik"])
@pytest.mark.parametrize("route", ["time", "ray"])
def test_a_single_launch_route_is_draw_step_and_the_optimisers_graph_safe_step(monkeypatch, route, eik):
    w = World(monkeypatch, pool=Rays if route == "ray" else Pool, time=route == "time")
    opts = StepOptions(sigma=0.1, ekional_loss_on=eik)
    sigma_size = torch.ones(1)
    it = w.build(opts, **(dict(ray=loop.RayTerm(sigma_size, neus_on=True)) if route == "ray" else {}))
    assert it.time == (route == "time") and (it.ray is not None) == (route == "ray")
    assert not it.fold and not it.native and it.ran_eager and it.touched is None and it.reg is None
    body = ["draw", route, "opt.step"]
    built = w.take()
    assert names(built) == body
    assert it() is it.loss
    first = w.take()
    assert names(first) == ["capture"] + body
    assert len(w.pool.parts) == (1 if eik else 0) and it._surf is (w.pool.parts[0] if eik else None)
    count_kw = "surf_out" if route == "ray" else "surf_parts"
    for run in (dict(built), dict(first[1:])):
        assert run["draw"] == {"n": N, "out": it._idx, "graph_safe": True, count_kw: it._surf}
        s = run[route]
        if route == "time":
            assert s["args"] == (w.octree, w.decoder, None, None, None, None, opts)
        else:
            assert s["args"] == (w.octree, w.decoder, None, None, None, None, sigma_size, opts, None) and s["neus_on"] is True
        assert s["n_surf"] is it._surf and s["pool"] is w.pool and s["idx"] is it._idx
        assert same_storage(it.loss, s["out"]) and it.loss.dim() == 0 and it.loss.dtype == torch.float32
        assert s["workspace"].numel() * s["workspace"].element_size() == (RAY_WS if route == "ray" else TIME_WS)
        assert run["opt.step"] == dict(zero_grad=True, graph_safe=True)
    assert built[1][1]["out"] is first[2][1]["out"] and built[1][1]["workspace"] is first[2][1]["workspace"]


def test_run_replays_the_unrolled_graph_and_the_remainder_one_by_one(monkeypatch):
    w = World(monkeypatch)
    sem, kw = term_objects(("normal",))
    it = w.build(native=False, unroll=3, **kw)
    w.take()
    body = ["fused", "normal", "finish_iteration"]
    assert it.run(1) is it.loss and names(w.take()) == ["capture"] + body  # (1 < unroll: the one-iteration graph)
    assert it() is it.loss and w.take() == []
    it.run(7)
    assert names(w.take()) == ["capture"] + body * 3 and it.graph_k.replays == 2 and it.graph.replays == 3
    w.octree._tables_epoch = 1
    for call in (it, lambda: it.run(2)):
        with pytest.raises(RuntimeError, match="the octree grew since this iteration was captured"):
            call()


def test_a_term_without_device_side_step_state_raises_at_run_time(monkeypatch):
    w = World(monkeypatch)
    w.opt.prepare_graph_safe = lambda skip=(): None  # (an optimiser that folds by its surface but never makes the state)
    with pytest.raises(RuntimeError, match="the optimiser has no device-side step state"):
        w.build(native=False, normal=loop.NormalTerm(0.05))


# ---- the terms are parameters of the constructor
def test_the_signature_shows_the_terms_and_a_subclass_receives_them():
    p = inspect.signature(loop.GraphedIteration).parameters
    assert list(p)[-4:] == ["sem", "normal", "consistency", "ray"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("normal", "consistency", "ray"))
    assert p["sem"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and p["sem"].default is None
    assert type(loop.GraphedIteration) is type

    seen = {}

    class Sub(loop.GraphedIteration):
        def __init__(self, *a, **kw):
            seen.update(kw)
            raise StopIteration  # (what the base class does with them is the other tests' business)

    term = loop.NormalTerm(0.05)
    with pytest.raises(StopIteration):
        Sub(None, None, None, None, None, N, normal=term)
    assert seen == dict(normal=term)


def test_the_argument_errors_of_sem_and_normal_come_before_any_allocation(monkeypatch):
    w = World(monkeypatch)

    def refuse(*a, **kw):
        raise AssertionError("argument errors come first")

    w.pool.surf_parts_buffer = refuse
    w.opt.prepare_graph_safe = refuse
    monkeypatch.setattr(loop, "touched_flags", refuse)
    good = loop.SemTerm(SemDecoder(True))
    with pytest.raises(ValueError, match=r"sem=\.\.\.\) needs the folded iteration"):
        w.build(fold=False, sem=good)
    with pytest.raises(ValueError, match="sem_label_decimation must be >= 1"):
        w.build(sem=loop.SemTerm(SemDecoder(True), decimation=0))
    half = SemDecoder(True)
    half.head[3].requires_grad_(False)
    with pytest.raises(ValueError, match="must all train or all be frozen"):
        w.build(sem=loop.SemTerm(half))
    with pytest.raises(ValueError, match=r"normal=\.\.\.\) needs the folded iteration"):
        w.build(fold=False, normal=loop.NormalTerm())
    w.pool.normal_label = None
    with pytest.raises(ValueError, match="SortedPool built with normal_label="):
        w.build(normal=loop.NormalTerm())
    with pytest.raises(ValueError, match="SortedPool built with normal_label="):  # (sem's checks pass first: sem, then normal)
        w.build(sem=good, normal=loop.NormalTerm())
    w.pool.sem_label = None
    with pytest.raises(ValueError, match="SortedPool built with sem_label="):
        w.build(sem=good, normal=loop.NormalTerm())
    with pytest.raises(ValueError, match=r"consistency=\.\.\.\) needs the folded iteration"):  # (consistency before sem)
        w.build(fold=False, sem=good, consistency=loop.ConsistencyTerm())
    assert w.take() == []
