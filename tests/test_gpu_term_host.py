"""GPU: the host side the three term steps share — ops._term_batch / _term_targets / _term_out / _term_call
behind fused_sem_step, fused_normal_step and fused_consistency_step, and csrc/shine_term_host.hpp behind their entry points.
Table-driven over the three terms on one golden fixture's tree and decoder: a batch of 65 rows (one full 64-lane tile plus one
lane) and 33 pairs (one full 32-pair tile plus one).

1. one resolver: array mode, array + idx gather and pool mode read the same rows in the same order — one library call each, with
   the source, stride, idx and n expected (and the weights' address and stride, where the step reads them), and the same loss to
   the bit; malformed inputs are refused alike by all.  The time step (ops.fused_time_step, with the eikonal term) resolves its
   batch and its weights through the same helpers and is a fourth row of this part's table.
2. one prologue: a valid argument tuple with exactly one argument spoiled comes back SHINE_E_INVALID with the entry point's text
   for that defect, before anything is launched: the loss and the workspace are untouched (the workspace zero where its
   contract says so) and the valid call gives the same bits afterwards."""
import contextlib
import copy
import ctypes as C

import pytest
import torch

from conftest import load_golden, product_from_golden
from test_semantic import sem_config

pytestmark = pytest.mark.gpu

FIXTURE = "kitti_eik_L3"
N, K, CLASSES = 65, 33, 21
E_INVALID = -1  # include/shine_hip.h SHINE_E_INVALID

# per term: the entry point, and where its argument list holds what the tests look at (include/shine_hip.h)
TERMS = {
    "sem": dict(entry="shine_sem_train_step", n=6, feats=9, mlp=12, grad_mlp=14),
    "normal": dict(entry="shine_normal_train_step", n=10, feats=12, mlp=15, grad_mlp=16),
    "consistency": dict(entry="shine_consistency_train_step", n=5, feats=15, mlp=18, grad_mlp=19),
}
# part 1 alone: the time step ends differently (a size argument follows its workspace), and its own suite covers its refusals
RESOLVED = dict(TERMS, time=dict(entry="shine_time_step", n=11, weight=6))
RESOLVED["normal"] = dict(TERMS["normal"], weight=5)  # (`weight`: the weights' address; their stride follows it)
CFG, SRC, STRIDE, IDX = 1, 2, 3, 4  # the same places in all of them
LOSS, WS = -3, -2                   # ... as are the last three: loss_out, workspace, stream


@contextlib.contextmanager
def calls_of(entry):
    """(the arguments of every call of `entry` made inside the block, the entry point itself)"""
    from shine_mapping_amd import _lib

    lib, seen = _lib.lib(), []
    fn = getattr(lib, entry)
    setattr(lib, entry, lambda *a: (seen.append(a), fn(*a))[1])
    try:
        yield seen, fn
    finally:
        setattr(lib, entry, fn)


class Setup:
    """the fixture's tree and decoder, a semantic head, a pool over the fixture's samples carrying labels and normals, one
    draw of N rows, and the same rows as arrays"""

    def __init__(self):
        from shine_mapping_amd import Decoder, autograd_ops
        from shine_mapping_amd.sampler import SortedPool

        fx = load_golden(FIXTURE)
        self.cfg, self.octree, self.dec = product_from_golden(fx)
        torch.manual_seed(1)
        self.sem = Decoder(sem_config("cuda", CLASSES - 1), is_geo_encoder=False)
        self.timed = Decoder(self.cfg, is_time_conditioned=True).cuda()
        with torch.no_grad():
            self.timed.layers[0].weight[:, 8] *= 0.03  # (frame ids: the time column's share stays of the first bias's order)
        assert self.timed.time_fusable
        autograd_ops.time_step_workspace_bytes()  # (asked once, through the entry point: not among the calls counted below)
        coord, weight = fx["coord"].cuda(), fx["weight"].cuda()
        gen = torch.Generator(device="cuda").manual_seed(5)
        lab = torch.randint(0, CLASSES, (coord.shape[0],), generator=gen, device="cuda")
        nrm = torch.randn(coord.shape, generator=gen, device="cuda")
        nrm = (nrm / nrm.norm(dim=-1, keepdim=True)).contiguous()
        frame = torch.randint(0, 4, (coord.shape[0],), generator=gen, device="cuda")
        self.pool = pool = SortedPool(self.octree, coord, fx["sdf_label"].cuda(), weight, seed=3, sem_label=lab, n_class=CLASSES,
                                      normal_label=nrm, ts=frame)
        self.idx = idx = pool.draw(N)
        assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == N
        i = idx.long()
        self.all = dict(coord=pool.soa()[0], weight=pool.soa()[2], label=pool.sem_label, normal=pool.normal_label,
                        sdf=pool.soa()[1], ts=pool.ts)
        self.rows = {k: v[i].contiguous() for k, v in self.all.items()}
        assert int((self.rows["weight"] > 0).sum()) > 0
        self.near = torch.randint(0, N, (K,), generator=gen, device="cuda").to(torch.int32)
        cell = self.cfg.leaf_vox_size * self.cfg.scale
        self.shift = ((torch.rand(K, 3, generator=gen, device="cuda") * 2 - 1) * (0.5 * cell)).contiguous()

    def clear(self):
        for p in (list(self.octree.hier_features) + list(self.dec.parameters()) + list(self.sem.parameters())
                  + list(self.timed.parameters())):
            p.grad = None

    def mlp(self, term):
        return self.sem.sem_params() if term == "sem" else self.timed.time_params() if term == "time" else self.dec.fused_params()

    def step(self, term, mode="array", **kw):
        """one term step reading the N rows in `mode`: "array" (the rows), "gather" (the pool's arrays through idx), "pool\""""
        from shine_mapping_amd import StepOptions, ops

        src = dict(array=self.rows, gather=self.all, pool=dict.fromkeys(self.all))[mode]
        if mode == "gather":
            kw.setdefault("idx", self.idx)
        if mode == "pool":
            kw.setdefault("pool", self.pool)
            kw.setdefault("idx", self.idx)
        self.clear()
        if term == "sem":
            loss = ops.fused_sem_step(self.octree, self.sem, src["coord"], src["label"], 0.7, 1, **kw)
        elif term == "normal":
            loss = ops.fused_normal_step(self.octree, self.dec, src["coord"], src["weight"], src["normal"], 0.05, **kw)
        elif term == "time":
            opts = StepOptions(sigma=float(self.cfg.sigma_sigmoid), ekional_loss_on=True, weight_e=0.1)
            loss = ops.fused_time_step(self.octree, self.timed, src["coord"], src["sdf"], src["weight"], src["ts"], opts, **kw)
        else:
            loss = ops.fused_consistency_step(self.octree, self.dec, src["coord"], 0.1, near_index=self.near, shift=self.shift, **kw)
        out = loss.clone()
        self.clear()
        return out


@pytest.fixture(scope="module")
def setup():
    return Setup()


# ---- 1. one resolver
@pytest.mark.parametrize("term", list(RESOLVED))
def test_one_resolver(setup, term):
    s, at = setup, RESOLVED[term]
    pool, idx = s.pool, s.idx
    pool_src = (pool.rec, 8) if pool.rec is not None else (pool.soa()[0], 3)
    want = dict(array=(s.rows["coord"], 3, None), gather=(s.all["coord"], 3, idx), pool=pool_src + (idx,))
    if pool.rec is None:
        pool_weight = (pool.soa()[2].data_ptr(), 1)
    elif pool._weight_sep is None:  # word 4 of the 32-byte records
        pool_weight = (pool.rec.data_ptr() + 16, 8)
    else:
        pool_weight = (pool._weight_sep.data_ptr(), 1)
    weights = dict(array=(s.rows["weight"].data_ptr(), 1), gather=(s.all["weight"].data_ptr(), 1), pool=pool_weight)
    losses = {}
    for mode, (src, stride, ix) in want.items():
        with calls_of(at["entry"]) as (seen, _):
            losses[mode] = s.step(term, mode)
        assert len(seen) == 1, (term, mode, len(seen))
        a = seen[0]
        assert a[SRC] == src.data_ptr() and a[STRIDE] == stride and a[at["n"]] == N, (term, mode)
        assert a[IDX] == (ix.data_ptr() if ix is not None else None), (term, mode)
        if "weight" in at:
            assert (a[at["weight"]], a[at["weight"] + 1]) == weights[mode], (term, mode)
    print(term, {m: float(v) for m, v in losses.items()})
    assert bool(torch.isfinite(losses["array"])) and float(losses["array"]) > 0
    assert torch.equal(losses["gather"], losses["array"]) and torch.equal(losses["pool"], losses["array"]), (term, losses)

    # malformed inputs: the same refusal from every term, and no library call
    stale = copy.copy(pool)  # (a pool planned on an earlier state of the tables: the octree has grown since)
    stale.tables_epoch = pool.tables_epoch - 1
    strided = torch.arange(2 * N, dtype=torch.int32, device="cuda")[::2]
    assert not strided.is_contiguous()
    bad = [("gather", dict(idx=idx.long()), ValueError, "idx must be a contiguous CUDA int32 tensor"),
           ("gather", dict(idx=strided), ValueError, "idx must be a contiguous CUDA int32 tensor"),
           ("pool", dict(idx=None), ValueError, r"pool mode needs idx = SortedPool.draw\(n\) \(CUDA int32\)"),
           ("pool", dict(pool=stale), RuntimeError, "the octree grew since the pool was planned"),
           ("array", dict(out=torch.zeros(2, device="cuda")), ValueError, "out must be a CUDA float32 tensor of one element")]
    with calls_of(at["entry"]) as (seen, _):
        for mode, kw, exc, text in bad:
            with pytest.raises(exc, match=text):
                s.step(term, mode, **kw)
        mixed = s.mlp(term)[2]
        mixed.requires_grad_(False)
        try:
            with pytest.raises(ValueError, match="six tensors must all require grad or all be frozen"):
                s.step(term)
        finally:
            mixed.requires_grad_(True)
        assert seen == [], term
    assert torch.equal(s.step(term), losses["array"])


# ---- 2. one prologue
# The text of each refusal as the entry points' source has it (csrc/shine_term_host.hpp; make_level_set's, which carries no
# entry-point prefix; the semantic head's own fill_mlp).  All are SHINE_E_INVALID.
def _refusals(term, cfg_of, ptrs_without):
    at = TERMS[term]
    null_mlp = "decoder parameters / n_class (1..32)" if term == "sem" else "null decoder parameter"
    return [
        ("coord_stride = 5", {STRIDE: 5}, "coord_stride is 3 ([n,3] array) or 8 (32-byte pool records)"),
        ("n = -1", {at["n"]: -1}, "n < 0"),
        ("workspace = NULL", {WS: None}, "workspace"),
        ("workspace + 8", {WS: lambda ws: ws + 8}, "workspace"),
        ("feats = NULL", {at["feats"]: None}, "null argument"),
        ("loss_out = NULL", {LOSS: None}, "null argument"),
        ("a NULL entry in mlp", {at["mlp"]: ptrs_without(2)}, null_mlp),
        ("a NULL entry in grad_mlp", {at["grad_mlp"]: ptrs_without(4)}, "null weight-grad tensor"),
        ("n_levels off by one", {CFG: cfg_of(-1)}, "n_levels mismatch"),
        ("n_levels = 5", {CFG: cfg_of(5)}, "more than 4 featured levels"),
    ]


@pytest.mark.parametrize("term", list(TERMS))
def test_one_prologue(setup, term):
    from shine_mapping_amd import _lib, autograd_ops

    s, at = setup, TERMS[term]
    nbytes = dict(sem=autograd_ops.SEM_WORKSPACE_BYTES, normal=autograd_ops.NORMAL_WORKSPACE_BYTES,
                  consistency=autograd_ops.CONSISTENCY_WORKSPACE_BYTES)[term]
    ws = _lib.zeroed_workspace(nbytes, "cuda")
    out = torch.zeros(1, device="cuda")
    # every address of the captured tuple stays alive to the end of the test: the gradients go to buffers held here, and the
    # normal term's surface count is handed in
    mlp = s.sem.sem_params() if term == "sem" else s.dec.fused_params()
    kw = dict(workspace=ws, out=out, grad_buffers=([torch.zeros_like(p) for p in s.octree.hier_features],
                                                   [torch.zeros_like(p) for p in mlp]))
    if term == "normal":
        kw["n_surf"] = (s.rows["weight"] > 0).sum().reshape(1)
    with calls_of(at["entry"]) as (seen, fn):
        before = s.step(term, **kw)
    assert len(seen) == 1
    valid = seen[0]

    # what a call leaves zero (include/shine_hip.h): the whole workspace of the normal and consistency steps; of the semantic
    # step's ticket workspace the 256 bytes of counters — its partial sums are overwritten before they are read
    def zeroed(w):
        return w[:256 // 8] if term == "sem" else w

    left = ws.clone()
    assert not bool(zeroed(left).any())
    assert valid[WS] == ws.data_ptr() and valid[LOSS] == out.data_ptr() and valid[at["grad_mlp"]] is not None
    levels = s.octree.featured_level_num
    assert 1 < levels <= 4 and valid[CFG]._obj.n_levels == levels
    keep = []  # (what a spoiled tuple points to outlives the call)

    def cfg_of(n_levels):
        cfg = type(valid[CFG]._obj).from_buffer_copy(valid[CFG]._obj)
        cfg.n_levels = levels + n_levels if n_levels < 0 else n_levels
        keep.append(cfg)
        return C.byref(cfg)

    def ptrs_without(k):
        def spoil(arr):
            vals = list(arr)
            assert len(vals) == 6 and all(vals)
            vals[k] = None
            keep.append(_lib.ptr_array(vals))
            return keep[-1]
        return spoil

    lib = _lib.lib()
    out.fill_(-7.0)
    for what, spoiled, text in _refusals(term, cfg_of, ptrs_without):
        args = list(valid)
        for pos, v in spoiled.items():
            args[pos] = v(args[pos]) if callable(v) else v
        rc = fn(*args)
        msg = lib.shine_error_string(rc).decode()
        print(term, what, rc, msg)
        assert rc == E_INVALID, (term, what, rc, msg)
        assert text in msg, (term, what, msg)
        if text != "n_levels mismatch":
            assert msg.startswith(at["entry"] + ": "), (term, what, msg)
    torch.cuda.synchronize()
    assert float(out) == -7.0, "a refused call writes no loss"
    assert torch.equal(ws.view(torch.uint8), left.view(torch.uint8)), "a refused call does not touch the workspace"
    assert not bool(zeroed(ws).any()), "the workspace is all zero after the refusals"
    assert fn(*valid) == 0
    assert torch.equal(out[0], before), (term, float(out), float(before))
    assert not bool(zeroed(ws).any())
