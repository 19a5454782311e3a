"""`master_weights=True` of ssd_keras_amd.optimizers on the GPU: ssdhip_adam_step_bf16 (csrc/ssdhip_adam.hip) and ssdhip_sgd_step_bf16
(csrc/ssdhip_optim.hip) -- bf16 parameters, bf16 gradients, float32 masters and moments in one launch -- against the float32
restatements tests/np_optim.py / tests/np_sgd.py fed float32(p0) and float32(g), BIT FOR BIT; the parameter as the exact rounding of
its master; the hand cases of tests/master_hand_cases.py; more tensors than a launch holds; the misaligned fall-back; the step replayed
as a HIP graph; the C ABI's refusals; and the bf16 SSD7 training step of models/keras_ssd7.py driven end to end.  Needs an MI355X.

The shapes reach every branch of the kernels (4096 values per block, eight per thread and pass, a scalar tail): fewer than eight
values, exactly eight, a tensor that crosses the block boundary with a 3-value tail in its second block, sizes that are no multiple
of 8, a channels_last filter."""
import copy
import ctypes

import numpy as np
import pytest

from tests import master_hand_cases as hand
from tests import np_optim, np_sgd
from tests.test_master_weights_cpu import run_adam_hand_case, run_sgd_hand_case
from tests.test_ssd7_fused_blocks_gpu import BATCH, _images
from tests.test_ssd7_fused_training_gpu import _state_equal, _train_model, deterministic_convolutions  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(64, 3, 3, 3), (7,), (8,), (4099,), (33, 5), (48, 32, 3, 3)]             # (the first one channels_last)


def _params(torch, shapes=SHAPES, seed=11, channels_last=(0,), dtype=None):
    dtype = dtype or torch.bfloat16
    ps = []
    for i, s in enumerate(shapes):
        t = torch.randn(s, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + i)).to(dtype)
        if i in channels_last and len(s) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(t))
    return ps


def _grad_like(torch, p, gen):
    gr = torch.randn(p.shape, device="cuda", generator=gen).to(p.dtype)
    return gr.contiguous(memory_format=torch.channels_last) if p.dim() == 4 and not p.is_contiguous() else gr


def _np32(t):
    return t.detach().float().cpu().numpy().copy()


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(opt, ps, ts, names, where):
    """Masters and buffers bit-equal to the restatement's float32 arrays (`names`: state key -> restatement key); p bit-equal to the
    rounding of its master."""
    import torch
    for i, (p, t) in enumerate(zip(ps, ts)):
        st = opt.state[p]
        if p.dtype != torch.bfloat16:                              # a float32 parameter of a mixed group: no master
            names_i = {("p" if k == "master" else k): v for k, v in names.items()}
            got_all = dict(st, p=p.detach())
        else:
            names_i, got_all = names, st
        for key, ref in names_i.items():
            got = got_all[key]
            assert got.dtype == torch.float32
            got = got.cpu().numpy()
            bad = int((_bits32(got) != _bits32(t[ref])).sum())
            assert bad == 0, "%s: %s of tensor %d differs in %d of %d values (max |d| %.3g)" % (
                where, key, i, bad, got.size, float(np.abs(got.astype(np.float64) - t[ref]).max()))
        if p.dtype == torch.bfloat16:
            want = hand.bf16_round_bits(st["master"].contiguous().cpu().numpy())
            assert np.array_equal(hand.bits_of(p).view(np.int16), want.view(np.int16)), "%s: p of tensor %d is not bf16(master)" % (where, i)


def _adam_names(amsgrad):
    return dict({"master": "p", "m": "m", "v": "v"}, **({"vhat": "vhat"} if amsgrad else {}))


def _run_against_restatement(torch, opt, ps, refs, ts, split, names, steps, gen, host_key):
    for step in range(steps):
        v0 = [p._version for p in ps]
        grads = [_grad_like(torch, p, gen) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone(memory_format=torch.preserve_format)
        opt.step()
        assert all(p._version > v for p, v in zip(ps, v0))
        refs[0].step(ts[:split], [_np32(g) for g in grads[:split]])
        if len(refs) > 1:
            refs[1].step(ts[split:], [_np32(g) for g in grads[split:]])
        assert opt.iterations == step + 1 == refs[0].iterations
        _same_bits(opt, ps, ts, names, "step %d" % (step + 1))
    assert host_key not in opt.state                              # nothing went through the expressions


@pytest.mark.parametrize("amsgrad,decay", [(False, 0.0), (True, 0.0), (False, 0.05), (True, 0.05)])
def test_adam_kernel_equals_the_float32_restatement_bit_for_bit(amsgrad, decay):
    import torch
    from ssd_keras_amd.optimizers import Adam
    ps = _params(torch)
    hyper = dict(lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=decay, amsgrad=amsgrad)
    opt = Adam([{"params": ps[:3], "weight_decay": 1e-3}, {"params": ps[3:]}], master_weights=True, **hyper)
    refs = [np_optim.Adam(weight_decay=1e-3, **hyper), np_optim.Adam(**hyper)]
    ts = [np_optim.fresh(_np32(p), amsgrad) for p in ps]
    _run_against_restatement(torch, opt, ps, refs, ts, 3, _adam_names(amsgrad), 5, torch.Generator(device="cuda").manual_seed(5), "adam_host")
    st = opt.state[ps[0]]
    assert all(st[n].is_contiguous(memory_format=torch.channels_last) and st[n].dtype == torch.float32 for n in _adam_names(amsgrad))


@pytest.mark.parametrize("rule,nesterov", [("torch", False), ("torch", True), ("keras", False), ("keras", True)])
def test_sgd_kernel_equals_the_float32_restatement_bit_for_bit(rule, nesterov):
    import torch
    from ssd_keras_amd.optimizers import SGD
    ps = _params(torch)
    hyper = dict(lr=1e-2, momentum=0.9, decay=0.05, nesterov=nesterov, rule=rule)
    opt = SGD([{"params": ps[:3], "weight_decay": 1e-3}, {"params": ps[3:]}], master_weights=True, **hyper)
    refs = [np_sgd.SGD(weight_decay=1e-3, **hyper), np_sgd.SGD(**hyper)]
    ts = [np_sgd.fresh(_np32(p)) for p in ps]
    name = "momentum_buffer" if rule == "torch" else "velocity"
    _run_against_restatement(torch, opt, ps, refs, ts, 3, {"master": "p", name: "buf"}, 5, torch.Generator(device="cuda").manual_seed(5), "sgd_host")
    st = opt.state[ps[0]]
    assert all(st[n].is_contiguous(memory_format=torch.channels_last) and st[n].dtype == torch.float32 for n in ("master", name))


def test_hand_cases_through_the_kernels():
    """tests/master_hand_cases.py on the GPU: three values, so the scalar tail of both kernels; the same assertions as on the CPU."""
    p, opt = run_sgd_hand_case("cuda", True)
    assert opt.iterations == hand.SGD_STEPS and "sgd_host" not in opt.state
    p, opt = run_adam_hand_case("cuda")
    assert opt.iterations == hand.ADAM_STEPS and "adam_host" not in opt.state
    stuck, opt = run_sgd_hand_case("cuda", False)                  # without masters: the expressions in bf16, and nothing moves
    assert stuck.detach().float().tolist() == hand.floats(hand.P0) and "sgd_host" in opt.state


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_more_tensors_than_one_launch_holds(kind):
    """150 tensors of 1 .. 150 values (a launch carries 64 resp. 80 in its arguments): every tensor is updated exactly once per step and
    `iterations` advances once per step, whatever the number of launches."""
    import torch
    from ssd_keras_amd.optimizers import SGD, Adam
    ps = _params(torch, [(k + 1,) for k in range(150)], seed=100, channels_last=())
    if kind == "adam":
        opt, ref = Adam(ps, lr=1e-2, epsilon=1e-8, master_weights=True), np_optim.Adam(lr=1e-2, epsilon=1e-8)
        ts, names, host = [np_optim.fresh(_np32(p)) for p in ps], _adam_names(False), "adam_host"
    else:
        opt, ref = SGD(ps, lr=1e-2, momentum=0.9, rule="keras", master_weights=True), np_sgd.SGD(lr=1e-2, momentum=0.9, rule="keras")
        ts, names, host = [np_sgd.fresh(_np32(p)) for p in ps], {"master": "p", "velocity": "buf"}, "sgd_host"
    _run_against_restatement(torch, opt, ps, [ref], ts, len(ps), names, 2, torch.Generator(device="cuda").manual_seed(6), host)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_mixed_group_takes_both_launches_behind_one_tick(kind):
    """float32 and bf16 parameters in ONE group: the float32 launch and the bf16 launch of the same step, the tick in front of the
    first only -- `iterations` advances by one per step and both halves follow the restatement."""
    import torch
    from ssd_keras_amd.optimizers import SGD, Adam
    shapes = [(33, 5), (4099,), (7,), (64, 3, 3, 3)]
    ps = _params(torch, shapes[:2], seed=30, channels_last=(), dtype=torch.float32) + _params(torch, shapes[2:], seed=40, channels_last=(1,))
    if kind == "adam":
        opt, ref = Adam(ps, lr=1e-2, epsilon=1e-8, decay=0.05, master_weights=True), np_optim.Adam(lr=1e-2, epsilon=1e-8, decay=0.05)
        ts, names, host = [np_optim.fresh(_np32(p)) for p in ps], _adam_names(False), "adam_host"
    else:
        opt, ref = SGD(ps, lr=1e-2, momentum=0.9, decay=0.05, master_weights=True), np_sgd.SGD(lr=1e-2, momentum=0.9, decay=0.05)
        ts, names, host = [np_sgd.fresh(_np32(p)) for p in ps], {"master": "p", "momentum_buffer": "buf"}, "sgd_host"
    _run_against_restatement(torch, opt, ps, [ref], ts, len(ps), names, 3, torch.Generator(device="cuda").manual_seed(7), host)
    tables = opt._planned(0, opt.param_groups[0], opt._tag(opt.param_groups[0]))[0]
    assert sorted(t[4] for t in tables) == [False, True] and len(opt._block_keys()) == 1
    assert all("master" not in opt.state[p] for p in ps[:2]) and all("master" in opt.state[p] for p in ps[2:])


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_misaligned_parameter_takes_the_expressions_with_the_same_bits(kind):
    """A view at a 2-byte offset into a larger bf16 tensor cannot take 16-byte accesses: it goes through the tensor expressions on its
    master and ends with the bits of an aligned copy that took the kernel."""
    import torch
    from ssd_keras_amd.optimizers import SGD, Adam
    n = 4099
    big = torch.randn(n + 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)).to(torch.bfloat16)
    guard = big.clone()
    odd, even = torch.nn.Parameter(big[1:n + 1]), torch.nn.Parameter(big[1:n + 1].clone())
    assert odd.data_ptr() % 16 == 2 and even.data_ptr() % 16 == 0 and torch.equal(odd, even)
    make = (lambda p: Adam([p], lr=1e-2, epsilon=1e-8, weight_decay=1e-3, amsgrad=True, master_weights=True)) if kind == "adam" else \
        (lambda p: SGD([p], lr=1e-2, momentum=0.9, weight_decay=1e-3, nesterov=True, rule="keras", master_weights=True))
    slow, fast = make(odd), make(even)
    gen = torch.Generator(device="cuda").manual_seed(4)
    for _ in range(3):
        gr = torch.randn(n, device="cuda", generator=gen).to(torch.bfloat16)
        odd.grad, even.grad = gr.clone(), gr.clone()
        slow.step()
        fast.step()
    host = kind + "_host"
    assert host in slow.state and host not in fast.state and slow.iterations == 3 == fast.iterations
    assert torch.equal(odd, even) and not torch.equal(even.detach(), guard[1:n + 1])
    for k in fast.state[even]:
        assert torch.equal(slow.state[odd][k], fast.state[even][k]), k
    assert torch.equal(odd.detach(), slow.state[odd]["master"].to(torch.bfloat16))
    assert torch.equal(big[:1], guard[:1]) and torch.equal(big[n + 1:], guard[n + 1:])          # the view's neighbours are untouched


def test_captured_step_replays_on_the_masters_with_the_scalars_of_its_own_step():
    """`opt.step()` captured ONCE on static gradient tensors, replayed eight times with fresh gradients copied in, `set_lr` after the
    fourth replay: masters and moments bit-equal to eight steps of the float32 restatement with that schedule, p their rounding."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    ps = _params(torch, [(64, 3, 3, 3), (129,), (4099,)], seed=21, channels_last=(0,))
    opt = Adam([{"params": ps[:1], "weight_decay": 1e-3}, {"params": ps[1:]}], lr=1e-2, epsilon=1e-8, amsgrad=True, master_weights=True)
    refs = [np_optim.Adam(lr=1e-2, epsilon=1e-8, amsgrad=True, weight_decay=1e-3), np_optim.Adam(lr=1e-2, epsilon=1e-8, amsgrad=True)]
    ts = [np_optim.fresh(_np32(p), True) for p in ps]
    gen = torch.Generator(device="cuda").manual_seed(8)
    for p in ps:
        p.grad = torch.zeros_like(p, memory_format=torch.preserve_format)
    opt.init_state()                                               # masters, moments and the state block: a capture may not allocate
    assert all(torch.equal(opt.state[p]["master"], p.detach().float()) for p in ps)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert opt.iterations == 0                                     # a capture runs nothing
    for k in range(8):
        grads = [_grad_like(torch, p, gen) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad.copy_(gr)
        graph.replay()
        refs[0].step(ts[:1], [_np32(g) for g in grads[:1]])
        refs[1].step(ts[1:], [_np32(g) for g in grads[1:]])
        if k == 3:                                                 # from the fifth step on
            opt.set_lr(2.5e-3)
            for r in refs:
                r.lr = 2.5e-3
        torch.cuda.synchronize()
        _same_bits(opt, ps, ts, _adam_names(True), "replay %d" % (k + 1))
    assert opt.iterations == 8 and "adam_host" not in opt.state


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_captures_that_would_go_wrong_are_refused_before_anything_is_recorded(kind):
    """No masters yet (no init_state(), no eager step): refused.  A parameter written behind its master: refused, naming
    sync_masters() -- the re-seeding copy would be part of the graph and run with every replay.  After sync_masters() the capture
    goes through and its replay starts from the written values."""
    import torch
    from ssd_keras_amd.optimizers import SGD, Adam
    ps = _params(torch, [(33, 5)], seed=41, channels_last=())
    opt = Adam(ps, lr=1e-2, epsilon=1e-8, master_weights=True) if kind == "adam" else \
        SGD(ps, lr=1e-2, momentum=0.9, rule="keras", master_weights=True)
    ps[0].grad = torch.ones_like(ps[0])
    before = ps[0].detach().clone()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="init_state"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            opt.step()
    torch.cuda.synchronize()
    assert "master" not in opt.state[ps[0]] and opt.iterations == 0 and torch.equal(ps[0].detach(), before)
    opt.step()                                                     # an eager step: masters, buffers, the block, a remembered version
    with torch.no_grad():
        ps[0].mul_(0.5)                                            # somebody else writes the parameter (exact in bf16)
    written = ps[0].detach().clone()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"sync_masters\(\)"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            opt.step()
    torch.cuda.synchronize()
    assert opt.iterations == 1 and torch.equal(ps[0].detach(), written)
    assert not torch.equal(opt.state[ps[0]]["master"], written.float())
    opt.sync_masters()
    assert torch.equal(opt.state[ps[0]]["master"], written.float())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    graph.replay()
    torch.cuda.synchronize()
    assert opt.iterations == 2
    master = opt.state[ps[0]]["master"]
    assert bool((master < written.float()).all()) and bool((written.float() - master < 0.05).all())       # one small step down from the written values
    assert torch.equal(ps[0].detach(), master.to(torch.bfloat16))


def test_a_capture_after_init_state_and_a_late_write_is_refused():
    """init_state() makes the masters and remembers the parameters' versions; weights written afterwards (a checkpoint loaded late) and
    a capture with no eager step in between: refused, naming sync_masters() -- not a replay that silently puts the old weights back."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    ps = _params(torch, [(33, 5), (8,)], seed=51, channels_last=())
    opt = Adam(ps, lr=1e-2, epsilon=1e-8, master_weights=True)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.init_state()
    with torch.no_grad():
        for p in ps:
            p.mul_(0.5)
    written = [p.detach().clone() for p in ps]
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"sync_masters\(\)"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            opt.step()
    torch.cuda.synchronize()
    assert opt.iterations == 0 and all(torch.equal(p.detach(), w) for p, w in zip(ps, written))
    opt.sync_masters()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    graph.replay()
    torch.cuda.synchronize()
    assert opt.iterations == 1
    for p, w in zip(ps, written):                                  # Adam's first step with gradient 1: lr down from the written values
        np.testing.assert_allclose(opt.state[p]["master"].cpu().numpy(), w.float().cpu().numpy() - 1e-2, rtol=1e-6, atol=1e-8)
        assert torch.equal(p.detach(), opt.state[p]["master"].to(torch.bfloat16))


def test_c_abi_refuses_bad_arguments_and_touches_nothing():
    """Direct calls of the two bf16 exports and, on float32 tensors, of ssdhip_adam_step, ssdhip_sgd_step and ssdhip_sgd_momentum_step
    (one host launcher behind all five): a null pointer, a misaligned master, numel = 0 and group = 64 return SSDHIP_E_BADARG (-1), and
    the buffers -- filled with a sentinel -- and the state block are what they were: nothing was launched, not even the tick."""
    import torch
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    n = 40
    p, g = torch.full((n,), 3.0, device="cuda", dtype=torch.bfloat16), torch.full((n,), 3.0, device="cuda", dtype=torch.bfloat16)
    floats = [torch.full((n + 4,), 3.0, device="cuda") for _ in range(4)]                  # master, m, v, vhat
    fp, fg = torch.full((n + 4,), 3.0, device="cuda"), torch.full((n + 4,), 3.0, device="cuda")   # a float32 parameter and its gradient
    adam_blk = torch.zeros((nat.adam_state_bytes(1),), dtype=torch.uint8, device="cuda")
    nat.adam_state_init(adam_blk, 1, 0, 1e-2, 0.9, 0.999, 1e-8, 0.0, 0.0)
    sgd_blk = torch.zeros((nat.sgd_state_bytes(1),), dtype=torch.uint8, device="cuda")
    nat.sgd_state_init(sgd_blk, 1, 0, 1e-2, 0.9, 0.0, 0.0)
    torch.cuda.synchronize()
    blocks = [adam_blk.clone(), sgd_blk.clone()]
    one = lambda t, off=0: (ctypes.c_void_p * 1)(t.data_ptr() + off)
    null = (ctypes.c_void_p * 1)(None)
    cnt, zero = (ctypes.c_longlong * 1)(n), (ctypes.c_longlong * 1)(0)
    w, m, v, vh = floats
    E = -1                                                         # SSDHIP_E_BADARG
    ab, sb = ctypes.c_void_p(adam_blk.data_ptr()), ctypes.c_void_p(sgd_blk.data_ptr())
    adam, sgd = lib.ssdhip_adam_step_bf16, lib.ssdhip_sgd_step_bf16
    refused = [
        adam(1, null, one(g), one(w), one(m), one(v), None, cnt, 0, ab, 1, None),
        adam(1, one(p), one(g), null, one(m), one(v), None, cnt, 0, ab, 1, None),
        adam(1, one(p), one(g), one(w), one(m), one(v), null, cnt, 0, ab, 1, None),
        adam(1, one(p), one(g), one(w, 4), one(m), one(v), None, cnt, 0, ab, 1, None),       # a master at 4 bytes past 16
        adam(1, one(p), one(g, 2), one(w), one(m), one(v), None, cnt, 0, ab, 1, None),
        adam(1, one(p), one(g), one(w), one(m), one(v), None, zero, 0, ab, 1, None),
        adam(1, one(p), one(g), one(w), one(m), one(v), None, cnt, 64, ab, 1, None),
        adam(1, one(p), one(g), one(w), one(m), one(v), None, cnt, 0, None, 1, None),
        adam(1, one(p), one(g), None, one(m), one(v), None, cnt, 0, ab, 1, None),
        sgd(1, null, one(g), one(w), one(m), cnt, 0, sb, 0, 0, 1, None),
        sgd(1, one(p), one(g), null, one(m), cnt, 0, sb, 0, 0, 1, None),
        sgd(1, one(p), one(g), one(w, 4), one(m), cnt, 0, sb, 0, 0, 1, None),
        sgd(1, one(p), one(g), one(w), one(m, 8), cnt, 0, sb, 0, 0, 1, None),
        sgd(1, one(p), one(g), one(w), one(m), zero, 0, sb, 0, 0, 1, None),
        sgd(1, one(p), one(g), one(w), one(m), cnt, 64, sb, 0, 0, 1, None),
        sgd(1, one(p), one(g), one(w), one(m), cnt, 0, sb, 2, 0, 1, None),                   # no such rule
        sgd(1, one(p), one(g), one(w), one(m), cnt, 0, None, 0, 0, 1, None),
        sgd(0, one(p), one(g), one(w), one(m), cnt, 0, sb, 0, 0, 1, None),
    ]
    adam, sgd, mom = lib.ssdhip_adam_step, lib.ssdhip_sgd_step, lib.ssdhip_sgd_momentum_step
    refused += [
        adam(1, null, one(fg), one(m), one(v), None, cnt, 0, ab, 1, None),
        adam(1, one(fp), one(fg), null, one(v), None, cnt, 0, ab, 1, None),
        adam(1, one(fp), one(fg), one(m), one(v), null, cnt, 0, ab, 1, None),
        adam(1, one(fp, 4), one(fg), one(m), one(v), None, cnt, 0, ab, 1, None),              # a parameter at 4 bytes past 16
        adam(1, one(fp), one(fg), one(m), one(v), one(vh, 4), cnt, 0, ab, 1, None),
        adam(1, one(fp), one(fg), one(m), one(v), None, zero, 0, ab, 1, None),
        adam(1, one(fp), one(fg), one(m), one(v), None, cnt, 64, ab, 1, None),
        adam(1, one(fp), one(fg), one(m), one(v), None, cnt, 0, None, 1, None),
        adam(1, one(fp), one(fg), None, one(v), None, cnt, 0, ab, 1, None),
        adam(0, one(fp), one(fg), one(m), one(v), None, cnt, 0, ab, 1, None),
        sgd(1, null, one(fg), one(m), cnt, 0, sb, 0, 0, 1, None),
        sgd(1, one(fp), one(fg), null, cnt, 0, sb, 0, 0, 1, None),
        sgd(1, one(fp), one(fg, 4), one(m), cnt, 0, sb, 0, 0, 1, None),
        sgd(1, one(fp), one(fg), one(m, 8), cnt, 0, sb, 0, 0, 1, None),
        sgd(1, one(fp), one(fg), one(m), zero, 0, sb, 0, 0, 1, None),
        sgd(1, one(fp), one(fg), one(m), cnt, 64, sb, 0, 0, 1, None),
        sgd(1, one(fp), one(fg), one(m), cnt, 0, sb, 2, 0, 1, None),                          # no such rule
        sgd(1, one(fp), one(fg), one(m), cnt, 0, None, 0, 0, 1, None),
        sgd(1, one(fp), None, one(m), cnt, 0, sb, 0, 0, 1, None),
        sgd(0, one(fp), one(fg), one(m), cnt, 0, sb, 0, 0, 1, None),
        mom(1, null, one(fg), one(m), cnt, 0.1, 0.9, 0.0, None),
        mom(1, one(fp), one(fg), null, cnt, 0.1, 0.9, 0.0, None),
        mom(1, one(fp), one(fg), one(m, 4), cnt, 0.1, 0.9, 0.0, None),
        mom(1, one(fp, 4), one(fg), one(m), cnt, 0.1, 0.9, 0.0, None),
        mom(1, one(fp), one(fg), one(m), zero, 0.1, 0.9, 0.0, None),
        mom(1, one(fp), one(fg), one(m), None, 0.1, 0.9, 0.0, None),
        mom(0, one(fp), one(fg), one(m), cnt, 0.1, 0.9, 0.0, None),
    ]
    assert refused == [E] * len(refused), refused
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in [p, g, fp, fg] + floats)
    assert int(nat.adam_state_read(adam_blk)[0]) == 0 and int(nat.sgd_state_read(sgd_blk)[0]) == 0           # no tick either
    assert torch.equal(adam_blk, blocks[0]) and torch.equal(sgd_blk, blocks[1])


# ---- SSD7 end to end -----------------------------------------------------------------------------------------------------------------
def _ssd7(seed=3):
    """The 76 x 68 test model of tests/test_ssd7_conv_training_gpu.py: bf16, channels_last, the libssdhip training route."""
    return _train_model(seed, None).fused_blocks(True, training=True, convolutions=True)


def _encoded_batch(model):
    import torch
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder
    enc = SSDInputEncoder(76, 68, 3, model.predictor_sizes(), min_scale=0.1, max_scale=0.9, aspect_ratios_global=[0.5, 1.0, 2.0],
                          two_boxes_for_ar1=True, clip_boxes=False, variances=[1.0, 1.0, 1.0, 1.0], matching_type="multi",
                          pos_iou_threshold=0.5, neg_iou_limit=0.3, normalize_coords=True)
    gt = syn.make_ground_truth(BATCH, 3, 76, 68, max_boxes=4, seed=0)
    return enc.encode_to_device(gt, device=torch.device("cuda", 0))[0]


def _loss_step(model, img, y_true):
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    loss = SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0).compute_loss(y_true, model(img).float()).mean()
    loss.backward()
    return loss


def test_ssd7_bf16_route_trains_through_the_masters(deterministic_convolutions):  # noqa: F811
    """The bf16 SSD7 of the libssdhip training route + HIP encoder + SSDLoss + Adam(lr=1e-3, epsilon=1e-8, master_weights=True), six
    steps: (a) a shadow parameter set driven through the tensor expressions (`_fused = False`) from the same gradients agrees bit for
    bit after every step, masters and parameters; (b) the loss is finite and lower at the end than at the start; (c) the same six steps
    with master_weights=False from the same weights leave at least one parameter tensor exactly where it started although its master
    moved -- at lr = 1e-3 these are the BatchNorm scales, whose magnitudes lie in [0.6, 1.4]: half a bf16 step there is 2e-3 or 4e-3,
    Adam moves a weight by about lr a step; (d) the whole step with the optimizer captured as one graph and replayed three times equals
    three eager steps."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    kw = dict(lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-8)
    img = _images()
    model = _ssd7()
    y_true = _encoded_batch(model)
    start = copy.deepcopy(model.state_dict())
    params = [p for p in model.parameters() if p.requires_grad]
    assert all(p.dtype == torch.bfloat16 for p in params)
    first = [p.detach().clone(memory_format=torch.preserve_format) for p in params]
    shadow = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in params]
    opt, plain = Adam(params, master_weights=True, **kw), Adam(shadow, master_weights=True, **kw)
    plain._fused = False
    losses = []
    for it in range(6):
        opt.zero_grad(set_to_none=True)
        losses.append(float(_loss_step(model, img, y_true).detach()))
        for p, q in zip(params, shadow):
            q.grad = p.grad.detach().clone(memory_format=torch.preserve_format)
        opt.step()
        plain.step()
        differing = sum(int((p.detach() != q.detach()).sum()) + int((opt.state[p]["master"] != plain.state[q]["master"]).sum())
                        for p, q in zip(params, shadow))
        print("step %d: loss %.5f, %d values differ between the kernel and the tensor expressions" % (it + 1, losses[-1], differing))
        assert differing == 0
    in_kernel = sum(len(t[1]) for t in opt._planned(0, opt.param_groups[0], opt._tag(opt.param_groups[0]))[0])
    print("%d of %d parameter tensors took ssdhip_adam_step_bf16" % (in_kernel, len(params)))
    assert in_kernel == len(params) and "adam_host" not in opt.state                    # every tensor: bf16, dense, aligned, gradient in its order
    assert opt.iterations == 6 == plain.iterations and "adam_host" in plain.state
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(torch.equal(p.detach(), opt.state[p]["master"].to(torch.bfloat16)) for p in params)

    # (c) the same six steps without masters
    bare = _ssd7()
    bare.load_state_dict(start)
    bare_params = [p for p in bare.parameters() if p.requires_grad]
    assert all(torch.equal(p.detach(), was) for p, was in zip(bare_params, first))
    bare_opt = Adam(bare_params, master_weights=False, **kw)
    for it in range(6):
        bare_opt.zero_grad(set_to_none=True)
        _loss_step(bare, img, y_true)
        bare_opt.step()
    stuck = [i for i, (p, was, q) in enumerate(zip(bare_params, first, params))
             if torch.equal(p.detach(), was) and not torch.equal(opt.state[q]["master"], was.float())]
    print("without masters %d of %d parameter tensors are where they started; their masters moved" % (len(stuck), len(params)))
    assert stuck

    # (d) forward + SSDLoss + backward + Adam on the masters as ONE graph, replayed three times, against three eager steps
    def step(m, o):
        o.zero_grad(set_to_none=True)
        _loss_step(m, img, y_true)
        o.step()

    eager, graphed = _ssd7(), _ssd7()
    eager.load_state_dict(start)
    eager_opt = Adam(eager.parameters(), master_weights=True, **kw)
    for _ in range(3):
        step(eager, eager_opt)
    graphed_opt = Adam(graphed.parameters(), master_weights=True, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _loss_step(graphed, img, y_true)                           # warm-up without an optimizer step: kernel choices, gradients in place
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.load_state_dict(start)                                 # (the running statistics moved)
    graphed_opt.init_state()                                       # masters from the restored weights, moments, the state block
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(graphed, graphed_opt)
    torch.cuda.synchronize()
    assert graphed_opt.iterations == 0
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert graphed_opt.iterations == 3 == eager_opt.iterations
    assert _state_equal(graphed, eager)
    for p, q in zip(graphed.parameters(), eager.parameters()):
        assert "master" in eager_opt.state[q]
        for k, want in eager_opt.state[q].items():
            assert torch.equal(graphed_opt.state[p][k], want), k
