"""CPU suite of the semantic training step (csrc/shine_sem_step.hip, ops.fused_sem_step, loop.GraphedIteration(sem=...)): the
entry point's host-side argument errors, the header / binding, the optimiser hooks the semantic loop uses, and that the
non-semantic GraphedIteration keeps its arguments.  The kernel itself is checked in tests/test_gpu_sem_step.py."""
import ctypes as C
import inspect
import os
import re

import torch

from conftest import ROOT


def _call(lib, table, cfg, stride=3, n=16, d=1, n_class=21, mlp=True, loss=True, ws=256):
    """shine_sem_train_step with stand-in (never dereferenced) pointers wherever the argument checks only look for NULL"""
    from shine_mapping_amd import _lib

    fake = 4096
    ptrs = _lib.ptr_array([fake] * 6)
    feats = _lib.ptr_array([fake] * 3)
    rows = _lib.i64_array([10, 10, 10])
    return lib.shine_sem_train_step(table, C.byref(cfg), fake, stride, None, fake, n, d, 1.0, feats, rows, None,
                                    ptrs if mlp else None, n_class, None, fake if loss else None, ws, None)


def test_argument_errors_come_back_without_touching_the_gpu():
    from shine_mapping_amd import _lib

    lib = _lib.lib()
    table = C.c_void_p()
    assert lib.shine_tables_create(3, C.byref(table)) == 0
    cfg = _lib.StepConfig()
    cfg.n_levels, cfg.max_level = 3, 12
    try:
        for kw, word in ((dict(stride=4), b"coord_stride"), (dict(stride=0), b"coord_stride"), (dict(d=0), b"decimation"),
                         (dict(d=-3), b"decimation"), (dict(n_class=0), b"n_class"), (dict(n_class=33), b"n_class"),
                         (dict(mlp=False), b"n_class"), (dict(loss=False), b"null argument"), (dict(n=-1), b"n < 0"),
                         (dict(ws=0), b"workspace"), (dict(ws=8), b"workspace")):
            rc = _call(lib, table, cfg, **kw)
            assert rc == -1 and word in lib.shine_error_string(rc), (kw, lib.shine_error_string(rc))
        rc = _call(lib, None, cfg)
        assert rc == -1 and b"null table handle" in lib.shine_error_string(rc)
        # every argument in order, but the handle's levels were never inserted: a state error, still on the host
        rc = _call(lib, table, cfg)
        assert rc == -4 and b"no table yet" in lib.shine_error_string(rc), lib.shine_error_string(rc)
        cfg.n_levels = 2  # (the handle has three)
        rc = _call(lib, table, cfg)
        assert rc == -1 and b"n_levels" in lib.shine_error_string(rc)
    finally:
        assert lib.shine_tables_destroy(table) == 0


def test_header_declares_the_entry_point_with_its_contract():
    from shine_mapping_amd import _lib

    text = open(os.path.join(ROOT, "include", "shine_hip.h")).read()
    assert re.search(r"\bint shine_sem_train_step\(", text)
    doc = text[:text.index("int shine_sem_train_step(")]
    doc = doc[doc.rindex("/* ----"):]
    for word in ("coord_stride", "decimation", "grad_mlp: NULL", "ACCUMULATED", "ADDED", "bit-identical", "n == 0",
                 "SHINE_SEM_WORKSPACE_BYTES", "SHINE_E_INVALID"):
        assert word in doc, word
    res, args = _lib._SIGNATURES["shine_sem_train_step"]
    assert res is C.c_int and len(args) == 18 and args[3] is C.c_int32 and args[8] is C.c_float


def test_public_surface():
    import shine_mapping_amd as s
    from shine_mapping_amd import loop, ops, sampler

    assert s.fused_sem_step is ops.fused_sem_step
    sig = inspect.signature(ops.fused_sem_step)
    assert list(sig.parameters)[:10] == ["octree", "sem_decoder", "coord", "sem_label", "weight_s", "decimation", "pool", "idx",
                                          "grad_buffers", "out"]
    assert sig.parameters["decimation"].default == 1
    # the non-semantic loop keeps its arguments and their defaults; the terms follow, off, the later three by keyword only
    g = inspect.signature(loop.GraphedIteration.__init__).parameters
    assert list(g) == ["self", "octree", "decoder", "pool", "opt", "opts", "n", "lambda_forget", "unroll", "fold", "eager_first",
                       "active_rows", "native", "graph_slot", "sem", "normal", "consistency", "ray"]
    assert all(g[k].default is None for k in ("sem", "normal", "consistency", "ray"))
    assert all(g[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("normal", "consistency", "ray"))
    assert all(g[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(g)[:15])
    assert g["native"].default is True and g["fold"].default is True
    term = loop.SemTerm(decoder=object())
    assert term.weight_s == 1.0 and term.decimation == 1
    for fn in (sampler.SortedPool.__init__, sampler.SortedPool.rebuild):
        p = inspect.signature(fn).parameters
        assert p["sem_label"].default is None and p["n_class"].default is None


def _sem_like_optimizer():
    """setup_optimizer's groups on host tensors: geo decoder (with its never-trained class layer), semantic decoder (with its
    never-trained lout), one feature level"""
    from shine_mapping_amd import Decoder, optim
    from test_semantic import sem_config

    torch.manual_seed(0)
    geo, sem = Decoder(sem_config("cpu", 20)), Decoder(sem_config("cpu", 20), is_geo_encoder=False)
    feat = torch.nn.Parameter(torch.zeros(9, 8))
    cfg = sem_config("cpu", 20)
    cfg.lr, cfg.weight_decay, cfg.tree_level_feat, cfg.semantic_on, cfg.opt_adam = 0.01, 1e-3, 1, True, True
    opt = optim.setup_optimizer(cfg, [feat], list(geo.parameters()), list(sem.parameters()), None)
    return opt, geo, sem, feat


def test_prepare_graph_safe_keeps_skipped_parameters_out_of_the_stepped_set():
    opt, geo, sem, feat = _sem_like_optimizer()
    skip = list(sem.lout.parameters()) + list(geo.nclass_out.parameters())
    opt.prepare_graph_safe(skip=skip)
    assert all(p.grad is None and p not in opt.state for p in skip)  # (torch.optim.Adam skips them the same way)
    stepped = [t[0] for t in opt._tensors()]
    assert len(stepped) == 6 + 6 + 1 and not any(p is q for p in skip for q in stepped)
    assert all(p.grad is not None and not p.grad.any() for p in stepped)
    # the semantic head's six tensors are consecutive members of that set, in sem_params() order: one lr pointer serves them
    pos = [next(i for i, q in enumerate(stepped) if q is p) for p in sem.sem_params()]
    assert pos == list(range(6, 12))
    assert opt.device_state() is not None and opt._dev[1].numel() == 13
    # without `skip` every parameter that requires grad gets a zero gradient: today's behaviour
    opt2, geo2, sem2, _ = _sem_like_optimizer()
    opt2.prepare_graph_safe()
    assert all(p.grad is not None for p in list(geo2.parameters()) + list(sem2.parameters()))


def test_step_tensors_dev_refuses_what_it_cannot_step():
    import pytest

    opt, geo, sem, feat = _sem_like_optimizer()
    with pytest.raises(RuntimeError, match="device-side step state"):
        opt.step_tensors_dev(sem.sem_params())
    opt.prepare_graph_safe(skip=list(sem.lout.parameters()) + list(geo.nclass_out.parameters()))
    head = sem.sem_params()
    with pytest.raises(NotImplementedError, match="consecutive"):
        opt.step_tensors_dev([head[0], head[2]])
    with pytest.raises(NotImplementedError, match="consecutive"):
        opt.step_tensors_dev(list(sem.lout.parameters()))
    with pytest.raises(ValueError, match="CUDA float32"):  # (host tensors: refused before any launch)
        opt.step_tensors_dev(head)
