"""`ssd_keras_amd.optimizers.SGD` on the GPU (csrc/ssdhip_optim.hip, sgd_tick_kernel / sgd_step_kernel): the default optimizer against
the legacy export ssdhip_sgd_momentum_step BIT FOR BIT (the yardstick: the state-block path must not change what the default computes),
both rules x Nesterov x decay against the NumPy restatement (tests/np_sgd.py) bit for bit, the hand-worked cases, more tensors than a
launch holds, the step captured once and replayed across a learning-rate change, checkpoints and copies.  Reference:
keras.optimizers.SGD as ssd300_training.ipynb:169 constructs it, under that notebook's LearningRateScheduler.  Needs an MI355X."""
import copy
import pickle

import numpy as np
import pytest

from tests import np_sgd
from tests import sgd_hand_cases as hand

pytestmark = pytest.mark.gpu

# a filter tensor; a tail only; across a 4096-value block and into a tail; no multiple of 4; channels_last (index 4)
SHAPES = [(64, 3, 3, 3), (7,), (4099,), (33, 5), (16, 8, 3, 3)]
MANY = [(5,)] * 150                                            # a launch carries 80 tensors in its arguments


def _params(torch, shapes, seed, channels_last=()):
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + i)))
          for i, s in enumerate(shapes)]
    with torch.no_grad():
        for i in channels_last:
            ps[i].data = ps[i].data.contiguous(memory_format=torch.channels_last)
            assert not ps[i].is_contiguous()
    return ps


def _grad_like(torch, p, gen):
    gr = torch.randn(p.shape, device="cuda", generator=gen)
    return gr.contiguous(memory_format=torch.channels_last) if p.dim() == 4 and not p.is_contiguous() else gr


def _flat(t):
    return t.detach().as_strided((t.numel(),), (1,))


def _memory(t):
    """The values of a dense tensor in MEMORY order (what the restatement, which knows no layouts, is compared with -- the update is
    element-wise, so any fixed order does)."""
    return _flat(t).cpu().numpy()


def _same_bits(opt, ps, ts, name, where):
    for i, (p, t) in enumerate(zip(ps, ts)):
        for what, got in (("p", _memory(p)), ("buf", _memory(opt.state[p][name]))):
            bad = int((got.view(np.int32) != t[what].view(np.int32)).sum())
            assert bad == 0, "%s: %s of tensor %d differs in %d of %d values (max |d| %.3g)" % (
                where, what, i, bad, got.size, float(np.abs(got.astype(np.float64) - t[what]).max()))


def test_default_sgd_is_the_legacy_export_bit_for_bit():
    """The yardstick: SGD with default arguments (rule 'torch', no Nesterov, no decay) goes through the tick and the state block, and
    over five steps its parameters and momentum buffers equal, bit for bit, those of `nat.sgd_momentum_step` -- the legacy export
    -- driven directly on clones with the same gradients.  Both kernels are one update body (csrc/ssdhip_optim_step.h), so that
    comparison alone would prove nothing: the legacy export's clones and buffers are also held, bit for bit, to the NumPy
    restatement (rule 'torch', no Nesterov, no decay).  Two groups (weight decay in one), every shape of the module, 150 small
    tensors."""
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.optimizers import SGD
    dev = torch.device("cuda", torch.cuda.current_device())
    ps = _params(torch, SHAPES + MANY, seed=11, channels_last=(4,))
    k = len(SHAPES)
    opt = SGD([{"params": ps[:k], "weight_decay": 1e-3}, {"params": ps[k:]}], lr=1e-2, momentum=0.9)
    twins = [p.detach().clone(memory_format=torch.preserve_format) for p in ps]
    bufs = [torch.zeros_like(t, memory_format=torch.preserve_format) for t in twins]
    refs = [np_sgd.SGD(lr=1e-2, momentum=0.9, weight_decay=1e-3), np_sgd.SGD(lr=1e-2, momentum=0.9)]
    ts = [np_sgd.fresh(_memory(t)) for t in twins]
    gen = torch.Generator(device="cuda").manual_seed(5)
    for step in range(5):
        grads = [_grad_like(torch, p, gen) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone(memory_format=torch.preserve_format)
        opt.step()
        for sl, wd in ((slice(0, k), 1e-3), (slice(k, None), 0.0)):
            table = nat.sgd_table([_flat(t) for t in twins[sl]], [_flat(g) for g in grads[sl]], [_flat(b) for b in bufs[sl]], dev)
            nat.sgd_momentum_step(table, 1e-2, 0.9, wd)
        torch.cuda.synchronize()
        refs[0].step(ts[:k], [_memory(g) for g in grads[:k]])
        refs[1].step(ts[k:], [_memory(g) for g in grads[k:]])
        for i, (t, b, r) in enumerate(zip(twins, bufs, ts)):
            for what, got in (("p", _memory(t)), ("buf", _memory(b))):
                assert np.array_equal(got.view(np.int32), r[what].view(np.int32)), "legacy export: %s of tensor %d, step %d" % (
                    what, i, step + 1)
        for i, (p, t, b) in enumerate(zip(ps, twins, bufs)):
            assert torch.equal(_flat(p).view(torch.int32), _flat(t).view(torch.int32)), "p of tensor %d, step %d" % (i, step + 1)
            assert torch.equal(_flat(opt.state[p]["momentum_buffer"]).view(torch.int32), _flat(b).view(torch.int32)), (i, step + 1)
    assert opt.iterations == 5 and "sgd_host" not in opt.state
    assert float((ps[0].detach() - twins[0]).abs().max()) == 0.0 and not torch.equal(twins[0], _params(torch, SHAPES[:1], 11)[0])


@pytest.mark.parametrize("decay", [0.0, 0.05])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("rule", ["torch", "keras"])
def test_one_launch_sgd_equals_the_restatement_bit_for_bit(rule, nesterov, decay):
    """Six steps with fresh gradients: two groups (weight decay in one; the second holds 150 tensors, two launches), p and the buffer
    bit-equal to the float32 restatement, `iterations` equal, every `_version` moves, buffers in their parameter's layout."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    ps = _params(torch, SHAPES + MANY, seed=31, channels_last=(4,))
    k = len(SHAPES)
    hyper = dict(lr=1e-2, momentum=0.9, decay=decay, nesterov=nesterov, rule=rule)
    opt = SGD([{"params": ps[:k], "weight_decay": 1e-3}, {"params": ps[k:]}], **hyper)
    refs = [np_sgd.SGD(weight_decay=1e-3, **hyper), np_sgd.SGD(**hyper)]
    ts = [np_sgd.fresh(_memory(p)) for p in ps]
    name = hand.BUFFER[rule]
    gen = torch.Generator(device="cuda").manual_seed(6)
    for step in range(6):
        v0 = [p._version for p in ps]
        grads = [_grad_like(torch, p, gen) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone(memory_format=torch.preserve_format)
        opt.step()
        assert all(p._version > v for p, v in zip(ps, v0))
        refs[0].step(ts[:k], [_memory(g) for g in grads[:k]])
        refs[1].step(ts[k:], [_memory(g) for g in grads[k:]])
        assert opt.iterations == step + 1 == refs[0].iterations == refs[1].iterations
        _same_bits(opt, ps, ts, name, "step %d" % (step + 1))
    assert opt.state[ps[4]][name].is_contiguous(memory_format=torch.channels_last)
    assert "sgd_host" not in opt.state                                     # nothing went through the tensor expressions
    assert all(other not in opt.state[p] for p in ps for other in hand.BUFFER.values() if other != name)


@pytest.mark.parametrize("case", hand.CASES, ids=[c["name"] for c in hand.CASES])
def test_kernel_on_the_hand_cases(case):
    """The hand-worked dyadic values through the kernel: every float32 operation is exact, so ==; the rate changed by `set_lr`."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    p = torch.nn.Parameter(torch.tensor(case["p0"], dtype=torch.float32, device="cuda"))
    opt = SGD([p], **case["kw"])
    for k, (g, lr, want) in enumerate(zip(case["grads"], case["set_lr"], case["expect"])):
        if lr is not None:
            opt.set_lr(lr)
        p.grad = torch.tensor(g, dtype=torch.float32, device="cuda")
        opt.step()
        assert p.detach().tolist() == want["p"], "p after step %d" % (k + 1)
        assert opt.state[p][hand.BUFFER[case["kw"]["rule"]]].tolist() == want["buf"], "buffer after step %d" % (k + 1)
    assert opt.iterations == len(case["grads"]) and "sgd_host" not in opt.state


def _captured_run(torch, rule):
    """init_state, `step()` captured once on static gradients, four replays, set_lr, four more: the parameters after each replay
    checked against the restatement under the same schedule.  Returns the final parameters."""
    from ssd_keras_amd.optimizers import SGD
    ps = _params(torch, SHAPES, seed=21, channels_last=(4,))
    hyper = dict(lr=1e-2, momentum=0.9, rule=rule)
    opt = SGD([{"params": ps[:1], "weight_decay": 1e-3}, {"params": ps[1:]}], **hyper)
    refs = [np_sgd.SGD(weight_decay=1e-3, **hyper), np_sgd.SGD(**hyper)]
    ts = [np_sgd.fresh(_memory(p)) for p in ps]
    gen = torch.Generator(device="cuda").manual_seed(8)
    for p in ps:
        p.grad = torch.zeros_like(p, memory_format=torch.preserve_format)
    opt.init_state()                                               # buffers and state block: a capture may not allocate
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert opt.iterations == 0                                     # a capture runs nothing
    for k in range(8):
        if k == 4:                                                 # from the fifth step on: ssd300_training.ipynb's schedule, 1e-3 -> 1e-4
            opt.set_lr(1e-3)
            for r in refs:
                r.lr = 1e-3
        grads = [_grad_like(torch, p, gen) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad.copy_(gr)
        graph.replay()
        refs[0].step(ts[:1], [_memory(g) for g in grads[:1]])
        refs[1].step(ts[1:], [_memory(g) for g in grads[1:]])
        torch.cuda.synchronize()
        _same_bits(opt, ps, ts, hand.BUFFER[rule], "%s, replay %d" % (rule, k + 1))
    assert opt.iterations == 8 and opt.param_groups[0]["lr"] == 1e-3
    return [_memory(p) for p in ps]


def test_captured_step_follows_set_lr_between_replays():
    """With the learning rate in the kernel arguments every replay would repeat the rate of the capture.  Both rules equal their
    restatement bit for bit over eight replays with the rate divided by ten after the fourth -- and differ from each other after the
    change (same parameters, same gradients: the velocity keeps the old rate on its history)."""
    import torch
    ends = {rule: _captured_run(torch, rule) for rule in ("keras", "torch")}
    assert all(not np.array_equal(a, b) for a, b in zip(ends["keras"], ends["torch"]))


def test_a_capture_without_state_is_refused_before_anything_is_recorded():
    import torch
    from ssd_keras_amd.optimizers import SGD
    ps = _params(torch, [(33, 5)], seed=41)
    opt = SGD(ps, lr=1e-2, momentum=0.9, rule="keras")
    ps[0].grad = torch.ones_like(ps[0])
    before = ps[0].detach().clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="init_state"):
        with torch.cuda.graph(graph):
            opt.step()
    torch.cuda.synchronize()
    assert not [k for k in opt.state if isinstance(k, str)] and "velocity" not in opt.state[ps[0]]
    assert opt.iterations == 0 and torch.equal(ps[0].detach(), before)
    # buffers without a block are refused too (a restored checkpoint of host steps, say): the block is created eagerly only
    opt.state[ps[0]]["velocity"] = torch.zeros_like(ps[0])
    with pytest.raises(RuntimeError, match="init_state"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            opt.step()
    torch.cuda.synchronize()
    opt.step()                                                     # and an eager step still works afterwards
    assert opt.iterations == 1 and torch.equal(ps[0].detach(), before - 1e-2)


def test_a_rate_set_through_param_groups_is_pushed_eagerly_and_refused_in_a_capture():
    import torch
    from ssd_keras_amd.optimizers import SGD
    ps = _params(torch, [(7,)], seed=51)
    opt = SGD(ps, lr=0.5, momentum=0.5, rule="keras")
    ref = np_sgd.SGD(lr=0.5, momentum=0.5, rule="keras")
    t = np_sgd.fresh(_memory(ps[0]))
    ps[0].grad = torch.ones_like(ps[0])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for _ in range(3):
        opt.step()
        ref.step([t], [np.ones(7, dtype=np.float32)])
        sched.step()
        ref.lr = ref.lr * 0.5
    _same_bits(opt, ps, [t], "velocity", "scheduler")
    opt.param_groups[0]["lr"] = 0.03125
    with pytest.raises(RuntimeError, match="before the capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            opt.step()
    torch.cuda.synchronize()
    opt.param_groups[0]["momentum"] = 0.25
    with pytest.raises(ValueError, match="only `lr`"):
        opt.step()


def test_fused_sgd_with_velocity_and_decay_survives_load_state_dict_and_copies():
    """The scenarios of test_fused_sgd_survives_load_state_dict_and_copies under rule='keras' with decay: step, load_state_dict of a
    checkpoint taken after step 1 (new buffer tensors, a new state block at count 1), step -- and the restored run's step 2 is the
    uninterrupted run's step 2 bit for bit (the rate of step 2, not of step 1); a pickled optimizer carries no table; a deep copy
    updates ITS tensors and ITS count."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    shapes = [(64, 3, 3, 3), (129,), (4099,)]
    a, b = _params(torch, shapes, seed=3), _params(torch, shapes, seed=3)
    kw = dict(lr=1e-2, momentum=0.9, weight_decay=1e-4, decay=0.5, rule="keras")
    ours, twin_run = SGD(a, **kw), SGD(b, **kw)
    gen = torch.Generator(device="cuda").manual_seed(7)
    grads = [[torch.randn(p.shape, device="cuda", generator=gen) for p in a] for _ in range(4)]

    def step(opt, ps, k):
        for p, gr in zip(ps, grads[k]):
            if p.grad is None:
                p.grad = gr.clone()
            else:                                                  # gradients stay where they are: only the state tensors move
                p.grad.copy_(gr)
        opt.step()

    step(ours, a, 0)
    step(twin_run, b, 0)
    ck = copy.deepcopy(ours.state_dict())
    after_1 = [p.detach().clone() for p in a]
    step(ours, a, 1)
    step(ours, a, 2)
    assert ours.iterations == 3
    ours.load_state_dict(ck)                                       # back to the velocities and the step count of step 1
    assert ours.iterations == 1
    with torch.no_grad():
        for p, was in zip(a, after_1):
            p.copy_(was)
    step(ours, a, 1)                                               # the restored run's step 2 ...
    step(twin_run, b, 1)                                           # ... and the uninterrupted run's
    assert ours.iterations == 2 == twin_run.iterations
    for p, q in zip(a, b):
        assert torch.equal(p, q) and torch.equal(ours.state[p]["velocity"], twin_run.state[q]["velocity"])
    clone = pickle.loads(pickle.dumps(ours))
    assert clone._tables == {} and clone.iterations == 2
    twin = copy.deepcopy(ours)
    before = [p.detach().clone() for p in a]
    tp = [p for grp in twin.param_groups for p in grp["params"]]
    for p, q in zip(tp, a):
        p.grad = q.grad.clone()
    twin.step()
    step(twin_run, b, 1)                                           # the uninterrupted run's step 3 on the same gradients
    for q, was in zip(a, before):
        assert torch.equal(q, was)                                 # the original's parameters were not touched by the copy's step
    assert all(not torch.equal(p, was) for p, was in zip(tp, before))
    assert all(torch.equal(p, q) for p, q in zip(tp, b))           # the copy's step 3 ran at the rate of step 3
    assert twin.iterations == 3 and ours.iterations == 2           # and the original's count stayed
