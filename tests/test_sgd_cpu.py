"""`ssd_keras_amd.optimizers.SGD` without a GPU: the NumPy restatement of both update rules (tests/np_sgd.py: Keras 2.x SGD's velocity,
torch.optim.SGD's momentum buffer, Nesterov and the time-based decay in both) against cases worked out by hand
(tests/sgd_hand_cases.py) and against torch.optim.SGD; the package's tensor-expression path (what CPU parameters take) against the
restatement; argument validation; checkpoints; the C ABI of the state-block kernels.  Reference: keras.optimizers.SGD as
ssd300_training.ipynb:169 constructs it, under that notebook's LearningRateScheduler."""
import copy
import inspect
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import np_sgd
from tests import sgd_hand_cases as hand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["name"] for c in hand.CASES]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", hand.CASES, ids=IDS)
def test_restatement_equals_the_hand_cases(case, dtype):
    """Dyadic values: every operation is exact in float32 and float64, so the comparison is ==."""
    opt = np_sgd.SGD(**case["kw"])
    t = np_sgd.fresh(np.array(case["p0"], dtype=dtype))
    for k, (g, lr, want) in enumerate(zip(case["grads"], case["set_lr"], case["expect"])):
        if lr is not None:
            opt.lr = lr
        opt.step([t], [np.array(g, dtype=dtype)])
        assert opt.iterations == k + 1
        if want["lr_t"] is not None:
            assert opt.lr_t == want["lr_t"], "lr_t of step %d" % (k + 1)
        assert t["p"].dtype == dtype and t["p"].tolist() == want["p"], "p after step %d: %r" % (k + 1, t["p"])
        assert t["buf"].tolist() == want["buf"], "buffer after step %d: %r" % (k + 1, t["buf"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", hand.CASES, ids=IDS)
def test_package_sgd_on_cpu_equals_the_hand_cases(case, dtype):
    """The same through the package's tensor expressions, the learning rate changed through `set_lr`."""
    from ssd_keras_amd.optimizers import SGD
    p = torch.nn.Parameter(torch.tensor(case["p0"], dtype=dtype))
    opt = SGD([p], **case["kw"])
    for k, (g, lr, want) in enumerate(zip(case["grads"], case["set_lr"], case["expect"])):
        if lr is not None:
            opt.set_lr(lr)
        p.grad = torch.tensor(g, dtype=dtype)
        opt.step()
        assert opt.iterations == k + 1
        assert p.detach().tolist() == want["p"], "p after step %d" % (k + 1)
        assert opt.state[p][hand.BUFFER[case["kw"]["rule"]]].tolist() == want["buf"], "buffer after step %d" % (k + 1)


def test_the_two_rules_part_where_the_rate_changes():
    """The issue's worked example: equal through two steps at lr 1/2, then -15/8 (Keras) against -27/16 (torch) at lr 1/4."""
    from ssd_keras_amd.optimizers import SGD
    ends = {}
    for rule in ("keras", "torch"):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = SGD([p], lr=0.5, momentum=0.5, rule=rule)
        seen = []
        for lr in (0.5, 0.5, 0.25):
            opt.param_groups[0]["lr"] = lr                                 # as a torch.optim.lr_scheduler sets it
            p.grad = torch.ones(1)
            opt.step()
            seen.append(float(p.detach()))
        ends[rule] = seen
    assert ends["keras"] == [-0.5, -1.25, -1.875] and ends["torch"] == [-0.5, -1.25, -1.6875]


def _mk(dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = [(8, 3, 3, 3), (7,), (5, 11)]
    return [torch.nn.Parameter(torch.randn(s, generator=g, dtype=dtype)) for s in shapes]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("decay", [0.0, 0.05])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("rule", ["torch", "keras"])
def test_package_sgd_on_cpu_follows_the_restatement(rule, nesterov, decay, dtype):
    """CPU parameters take plain tensor expressions of the rule, the scalars advanced on the host: the same operations in the same
    order as the restatement, two groups (weight decay in one).  float32: every operation is a single correctly rounded IEEE
    operation in both, so bit for bit.  float64: the bounds tests/test_optim_cpu.py uses for Adam (p to 1e-13 relative, the state
    to 1e-14) -- there is no square root here, so nothing is expected to use them."""
    from ssd_keras_amd.optimizers import SGD
    ps = _mk(dtype)
    hyper = dict(lr=1e-2, momentum=0.9, decay=decay, nesterov=nesterov, rule=rule)
    opt = SGD([{"params": ps[:2], "weight_decay": 1e-3}, {"params": ps[2:]}], **hyper)
    refs = [np_sgd.SGD(weight_decay=1e-3, **hyper), np_sgd.SGD(**hyper)]
    ts = [np_sgd.fresh(p.detach().numpy().copy()) for p in ps]
    g = torch.Generator().manual_seed(9)
    for step in range(5):
        grads = [torch.randn(p.shape, generator=g, dtype=dtype) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        refs[0].step(ts[:2], [x.numpy() for x in grads[:2]])
        refs[1].step(ts[2:], [x.numpy() for x in grads[2:]])
        assert opt.iterations == step + 1 == refs[0].iterations
        for p, t in zip(ps, ts):
            buf = opt.state[p][hand.BUFFER[rule]].numpy()
            if dtype == torch.float32:
                assert np.array_equal(p.detach().numpy(), t["p"]) and np.array_equal(buf, t["buf"]), step
            else:
                np.testing.assert_allclose(p.detach().numpy(), t["p"], rtol=1e-13, atol=1e-15)
                np.testing.assert_allclose(buf, t["buf"], rtol=1e-14, atol=0)


def test_momentum_zero_keeps_no_state_and_is_plain_gradient_descent():
    from ssd_keras_amd.optimizers import SGD
    for rule in ("torch", "keras"):
        p = torch.nn.Parameter(torch.tensor([1.0, -2.0]))
        opt = SGD([p], lr=0.5, decay=1.0, rule=rule)
        for want in ([0.5, -1.0], [0.375, -0.75]):                         # lr 1/2, then 1/4: p - lr p
            p.grad = p.detach().clone()
            opt.step()
            assert p.detach().tolist() == want
        assert not [k for k in opt.state[p]] and opt.iterations == 2


@pytest.mark.parametrize("nesterov", [False, True])
def test_torch_rule_follows_torch_sgd_at_a_constant_rate(nesterov):
    """rule='torch' against torch.optim.SGD(nesterov=...) on the same parameters and gradients over five steps, with the tolerances
    of test_fused_sgd_momentum_step_follows_torch_sgd: rtol 3e-7 and atol 1e-7 per step (the framework may contract p + (-lr) buf
    into one fused multiply-add)."""
    from ssd_keras_amd.optimizers import SGD
    a, b = _mk(torch.float32), _mk(torch.float32)
    kw = dict(lr=1e-2, momentum=0.9, nesterov=nesterov)
    ours = SGD([{"params": a[:2], "weight_decay": 1e-3}, {"params": a[2:]}], **kw)
    ref = torch.optim.SGD([{"params": b[:2], "weight_decay": 1e-3}, {"params": b[2:]}], **kw)
    g = torch.Generator().manual_seed(5)
    for step in range(5):
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g)
            pa.grad, pb.grad = gr.clone(), gr.clone()
        ours.step()
        ref.step()
        for pa, pb in zip(a, b):
            torch.testing.assert_close(pa, pb, rtol=3e-7 * (step + 1), atol=1e-7 * (step + 1))
            torch.testing.assert_close(ours.state[pa]["momentum_buffer"], ref.state[pb]["momentum_buffer"], rtol=1e-6, atol=1e-6)


def test_constructor_signature_and_bad_hyperparameters():
    from ssd_keras_amd.optimizers import SGD
    sig = inspect.signature(SGD.__init__)
    assert list(sig.parameters)[1:] == ["params", "lr", "momentum", "weight_decay", "decay", "nesterov", "rule"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["lr"], d["momentum"], d["weight_decay"], d["decay"], d["nesterov"], d["rule"]) == (0.01, 0.0, 0.0, 0.0, False, "torch")
    p = torch.nn.Parameter(torch.zeros(3))
    opt = SGD([p], lr=0.001, momentum=0.9, decay=0.0, nesterov=False)          # ssd300_training.ipynb:169
    assert isinstance(opt, torch.optim.Optimizer) and opt.iterations == 0
    g0 = opt.param_groups[0]
    assert (g0["decay"], g0["nesterov"], g0["rule"]) == (0.0, False, "torch")
    SGD([p], momentum=0.9, decay=1e-4, nesterov=True, rule="keras")
    for bad in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(decay=-1.0), dict(nesterov=True),
                dict(nesterov=True, momentum=0.0), dict(rule="caffe"), dict(rule=None)):
        with pytest.raises(ValueError):
            SGD([p], **bad)
    with pytest.raises(ValueError):
        SGD([{"params": [p], "decay": -0.5}], momentum=0.9)
    with pytest.raises(ValueError):
        opt.set_lr(-1.0)
    # a learning-rate scheduler drives it through param_groups; set_lr writes them
    keras = SGD([p], lr=0.5, momentum=0.5, rule="keras")
    sched = torch.optim.lr_scheduler.StepLR(keras, step_size=2, gamma=0.5)
    for want in (-0.5, -1.25, -1.875):
        p.grad = torch.ones(3)
        keras.step()
        sched.step()
        assert p.detach().tolist() == [want] * 3
    assert keras.param_groups[0]["lr"] == 0.25
    keras.set_lr(0.125)
    assert keras.param_groups[0]["lr"] == 0.125


def test_group_limit_is_a_value_error_at_the_call():
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.optimizers import SGD
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in range(nat.ADAM_MAX_GROUPS + 1)]
    with pytest.raises(ValueError):
        SGD([{"params": [p]} for p in ps], momentum=0.9)
    opt = SGD([{"params": [p]} for p in ps[:-1]], momentum=0.9)
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [ps[-1]]})
    assert len(opt.param_groups) == nat.ADAM_MAX_GROUPS


def test_state_dict_round_trip_continues_at_the_saved_step():
    """A checkpoint taken after step 2 carries the step count and the velocities: with decay > 0 the restored optimizer's step 3 runs
    at the rate of step 3 (not of step 1) and equals the uninterrupted run's, in a fresh optimizer and through pickle."""
    from ssd_keras_amd.optimizers import SGD
    a, b = _mk(torch.float32), _mk(torch.float32)
    g = torch.Generator().manual_seed(1)
    grads = [[torch.randn(p.shape, generator=g) for p in a] for _ in range(3)]
    kw = dict(lr=1e-2, momentum=0.9, decay=0.5, nesterov=True, rule="keras")
    one = SGD(a, **kw)
    for k in range(2):
        for p, gr in zip(a, grads[k]):
            p.grad = gr.clone()
        one.step()
    ck = copy.deepcopy(one.state_dict())
    assert ck["state"]["sgd_host"]["iterations"] == 2
    saved = [one.state[p]["velocity"].clone() for p in a]
    with torch.no_grad():
        for p, q in zip(a, b):
            q.copy_(p)
    two = SGD(b, **kw)
    two.load_state_dict(ck)
    assert two.iterations == 2
    assert all(torch.equal(two.state[q]["velocity"], v) for q, v in zip(b, saved))
    three = pickle.loads(pickle.dumps(one))
    assert three.iterations == 2 and three._tables == {}
    for opt, ps in ((one, a), (two, b)):
        for p, gr in zip(ps, grads[2]):
            p.grad = gr.clone()
        opt.step()
        assert opt.iterations == 3
    for p, q in zip(a, b):
        assert torch.equal(p, q) and torch.equal(one.state[p]["velocity"], two.state[q]["velocity"])
    assert ck["state"]["sgd_host"]["iterations"] == 2                     # the checkpoint itself was not stepped
    # and the rate of step 3 was lr0 / (1 + decay * 2): a run restarted at count 0 differs
    ref = np_sgd.SGD(iterations=2, **kw)
    assert ref.tick() == 1e-2 / (1.0 + 0.5 * 2.0)


def test_sgd_exports_are_declared_documented_and_reject_bad_arguments():
    """The four exports have ctypes signatures in the one table of _native.py, prototypes and a description in include/ssdhip.h and
    rows in INTEGRATION.md; a null or misaligned pointer, an out-of-range group or rule return SSDHIP_E_BADARG (-1) before anything is
    launched -- no device is touched here."""
    import ctypes
    from ssd_keras_amd import _native as nat
    hdr = open(os.path.join(ROOT, "include", "ssdhip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("ssdhip_sgd_state_bytes", "ssdhip_sgd_state_init", "ssdhip_sgd_set_lr", "ssdhip_sgd_step"):
        assert name in nat.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in doc, name
    assert nat.SGD_GROUP.itemsize == 40 and nat.SGD_STATE_HEAD.itemsize == 16
    lib = nat.load()
    assert lib.ssdhip_sgd_state_bytes(2) == 16 + 2 * 40 and lib.ssdhip_sgd_state_bytes(0) == 0 and lib.ssdhip_sgd_state_bytes(65) == 0
    ok, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)            # never dereferenced: every call below is refused first
    assert lib.ssdhip_sgd_state_init(None, 1, 0, 1e-3, 0.9, 0.0, 0.0, 0, None) == -1
    assert lib.ssdhip_sgd_state_init(odd, 1, 0, 1e-3, 0.9, 0.0, 0.0, 0, None) == -1
    assert lib.ssdhip_sgd_state_init(ok, 1, 1, 1e-3, 0.9, 0.0, 0.0, 0, None) == -1        # group >= n_groups
    assert lib.ssdhip_sgd_state_init(ok, 65, 0, 1e-3, 0.9, 0.0, 0.0, 0, None) == -1
    assert lib.ssdhip_sgd_state_init(ok, 1, 0, -1e-3, 0.9, 0.0, 0.0, 0, None) == -1
    assert lib.ssdhip_sgd_state_init(ok, 1, 0, 1e-3, 0.9, -1.0, 0.0, 0, None) == -1
    assert lib.ssdhip_sgd_state_init(ok, 1, 0, 1e-3, 0.9, 0.0, 0.0, -1, None) == -1
    assert lib.ssdhip_sgd_set_lr(None, 0, 0.1, None) == -1
    assert lib.ssdhip_sgd_set_lr(odd, 0, 0.1, None) == -1
    assert lib.ssdhip_sgd_set_lr(ok, 64, 0.1, None) == -1
    assert lib.ssdhip_sgd_set_lr(ok, -1, 0.1, None) == -1
    assert lib.ssdhip_sgd_set_lr(ok, 0, -0.1, None) == -1
    one = (ctypes.c_void_p * 1)(4096)
    bad = (ctypes.c_void_p * 1)(4096 + 4)
    n = (ctypes.c_longlong * 1)(8)
    assert lib.ssdhip_sgd_step(0, None, None, None, None, 0, None, 0, 0, 0, None) == -1
    assert lib.ssdhip_sgd_step(1, one, one, one, n, 0, None, 0, 0, 1, None) == -1         # no state block
    assert lib.ssdhip_sgd_step(1, one, one, one, n, 0, odd, 0, 0, 1, None) == -1          # a misaligned one
    assert lib.ssdhip_sgd_step(1, one, one, one, n, 64, ok, 0, 0, 1, None) == -1          # group out of range
    assert lib.ssdhip_sgd_step(1, one, one, one, n, 0, ok, 2, 0, 1, None) == -1           # no such rule
    assert lib.ssdhip_sgd_step(1, one, bad, one, n, 0, ok, 0, 0, 1, None) == -1           # a misaligned gradient
    assert lib.ssdhip_sgd_step(1, one, one, None, n, 0, ok, 0, 0, 1, None) == -1
    assert lib.ssdhip_sgd_step(1, one, one, one, (ctypes.c_longlong * 1)(0), 0, ok, 0, 0, 1, None) == -1
