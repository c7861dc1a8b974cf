"""CPU suite of FusedAdam's device-side step state (shine_mapping_amd/optim.py) on host tensors of 4 elements: the stepped set,
the steps a graph took on the device and how they are folded back, and what binds the state to its tensors.  Nothing here
launches; the device counter is written by hand where a graph would have advanced it.  What FusedAdam hands the library's entry
points is pinned in tests/test_gpu_optim_calls.py."""
import types

import pytest
import torch

from shine_mapping_amd.optim import FusedAdam


def _opt(lrs, frozen=()):
    """one tensor per group with its own learning rate; `frozen`: the positions that do not require grad"""
    ps = [torch.nn.Parameter(torch.zeros(4), requires_grad=i not in frozen) for i in range(len(lrs))]
    return FusedAdam([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)]), ps


def _lrs(*values):
    return torch.tensor(values, dtype=torch.float32)


def _swapped():
    """a, b train and c is frozen when the device state is made; then b is frozen and c trains: two tensors before and after"""
    opt, (a, b, c) = _opt([0.1, 0.2, 0.3], frozen=(2,))
    opt.prepare_graph_safe()
    b.requires_grad_(False)
    c.requires_grad_(True)
    c.grad = torch.zeros_like(c)
    return opt, a, b, c


# ---------------------------------------------------------------------------------------------------- the device counter

def test_device_steps_are_counted_in_and_folded_by_load_state_dict():
    opt, (a, b) = _opt([0.1, 0.2])
    state = opt.prepare_graph_safe()
    assert state is opt.device_state() and opt.steps_taken() == 0
    opt._dev[0][0] = 5  # (what five replays of a captured step leave)
    assert opt.steps_taken() == 5 and opt.step_count == 0
    sd = opt.state_dict()
    assert [float(sd["state"][k]["step"]) for k in (0, 1)] == [5.0, 5.0]
    assert opt.device_state() is state and opt.step_count == 0  # (state_dict reads the counter; the state stays live)
    opt.load_state_dict(sd)
    assert opt.device_state() is None and opt.step_count == 5 and opt.steps_taken() == 5
    assert opt._age[a] == 5 and opt._age[b] == 5


def test_freezing_a_member_folds_and_remakes_the_state():
    opt, (a, b) = _opt([0.1, 0.2])
    first = opt.prepare_graph_safe()
    opt._dev[0][0] = 5
    b.requires_grad_(False)
    second = opt.prepare_graph_safe()
    assert second is not first and second is opt.device_state()
    assert torch.equal(opt._dev[1], _lrs(0.1))  # (one learning rate fewer)
    assert opt.step_count == 5 and opt._age[a] == 5 and opt._age[b] == 5  # (the frozen tensor took those five steps too)
    assert int(second[0]) == 5 and opt.steps_taken() == 5  # (the new counter goes on where the old one stood)


def test_skipped_parameters_stay_without_grad_and_without_state():
    opt, (a, b) = _opt([0.1, 0.2])
    opt.prepare_graph_safe(skip=[b])
    assert b.grad is None and b not in opt.state
    assert a.grad is not None and not a.grad.any() and a in opt.state
    assert [t[0] for t in opt._tensors()] == [a] and opt._dev[1].numel() == 1


def _pending(tables, decoder_tensors=()):
    """what finish_iteration reads of a fused step's pending dict before it looks at the device: stand-ins"""
    return {"octree": types.SimpleNamespace(hier_features=list(tables)),
            "decoder": types.SimpleNamespace(fused_params=lambda: list(decoder_tensors)), "dec_grad": bool(decoder_tensors)}


def test_device_launches_need_the_device_state():
    opt, (a, b) = _opt([0.1, 0.2])
    a.grad, b.grad = torch.zeros_like(a), torch.zeros_like(b)
    with pytest.raises(RuntimeError, match="device-side step state"):
        opt.step_tensors_dev([a])
    with pytest.raises(RuntimeError, match="device-side step state"):
        opt.finish_iteration(_pending([a, b]))


# ------------------------------------------------------------------------------- one age, and a state bound to its tensors

def test_a_tensor_that_joins_late_is_refused_by_prepare_graph_safe():
    """b's first step would get the bias correction of step 6 from the shared device counter; torch's Adam gives it step 1.
    step(graph_safe=True) refuses this; prepare_graph_safe must as well."""
    opt, (a, b) = _opt([0.1, 0.2], frozen=(1,))
    opt.prepare_graph_safe()
    opt._dev[0][0] = 5
    b.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="same age"):
        opt.prepare_graph_safe()


def test_a_member_swap_at_equal_count_remakes_the_state():
    opt, a, b, c = _swapped()
    opt.prepare_graph_safe()
    assert torch.equal(opt._dev[1], _lrs(0.1, 0.3))
    bound = opt._dev.params
    assert len(bound) == 2 and bound[0] is a and bound[1] is c


def test_a_member_swap_after_device_steps_is_refused():
    opt, a, b, c = _swapped()
    opt._dev[0][0] = 5
    with pytest.raises(NotImplementedError, match="same age"):
        opt.prepare_graph_safe()


def test_step_tensors_dev_sees_a_member_swap():
    opt, a, b, c = _swapped()
    with pytest.raises(RuntimeError, match="set of tensors changed"):
        opt.step_tensors_dev([a])


def test_finish_iteration_sees_a_member_swap():
    opt, a, b, c = _swapped()
    with pytest.raises(RuntimeError, match="set of tensors changed"):
        opt.finish_iteration(_pending([a, c]))


def test_sync_lr_does_not_depend_on_who_holds_a_grad():
    """Tier A's order when step_lr_decay follows zero_grad(set_to_none=True)"""
    opt, (a, b) = _opt([0.1, 0.2])
    opt.prepare_graph_safe()
    opt.param_groups[1]["lr"] = 0.05
    opt.zero_grad(set_to_none=True)
    opt.sync_lr()
    assert torch.equal(opt._dev[1], _lrs(0.1, 0.05))
