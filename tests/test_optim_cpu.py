"""`ssd_keras_amd.optimizers.Adam` without a GPU: the NumPy restatement of Keras 2.x Adam (tests/np_optim.py) against cases worked out
by hand (tests/adam_hand_cases.py) and against torch.optim.Adam where the two rules coincide; the package's tensor-expression path
(what CPU parameters take) against the restatement; checkpoints; the C ABI of the kernels.  Reference: keras.optimizers.Adam as the
notebooks construct it, ssd7_training.ipynb:153."""
import copy
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import adam_hand_cases as hand
from tests import np_optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kw(case):
    return {k: (float(v) if not isinstance(v, bool) else v) for k, v in case["kw"].items()}


@pytest.mark.parametrize("case", hand.CASES, ids=[c["name"] for c in hand.CASES])
def test_restatement_equals_the_hand_cases(case):
    opt = np_optim.Adam(**_kw(case))
    t = np_optim.fresh(np.array(hand.floats(case["p0"]), dtype=np.float64), amsgrad=opt.amsgrad)
    for k, (g, want) in enumerate(zip(case["grads"], case["expect"])):
        opt.step([t], [np.array(hand.floats(g), dtype=np.float64)])
        assert opt.iterations == k + 1
        for name, vals in want.items():
            np.testing.assert_allclose(t[name], hand.floats(vals), rtol=hand.RTOL, atol=0, err_msg="%s after step %d" % (name, k + 1))


@pytest.mark.parametrize("case", hand.CASES, ids=[c["name"] for c in hand.CASES])
def test_package_adam_on_cpu_equals_the_hand_cases(case):
    from ssd_keras_amd.optimizers import Adam
    p = torch.nn.Parameter(torch.tensor(hand.floats(case["p0"]), dtype=torch.float64))
    opt = Adam([p], **_kw(case))
    for k, (g, want) in enumerate(zip(case["grads"], case["expect"])):
        p.grad = torch.tensor(hand.floats(g), dtype=torch.float64)
        opt.step()
        assert opt.iterations == k + 1
        got = dict(p=p.detach(), **{n: opt.state[p][n] for n in want if n != "p"})
        for name, vals in want.items():
            np.testing.assert_allclose(got[name].numpy(), hand.floats(vals), rtol=hand.RTOL, atol=0, err_msg="%s after step %d" % (name, k + 1))


def test_restatement_is_torch_adam_when_epsilon_is_zero():
    """With epsilon = 0 Keras's and torch's rules are the same real-number expression (lr sqrt(1 - b2^t) / (1 - b1^t) m / sqrt(v)); in
    float64 over 20 steps they agree to 1e-12 relative -- which pins everything in the restatement but where epsilon sits."""
    rs = np.random.RandomState(0)
    p0 = rs.randn(257)
    ours = np_optim.Adam(lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=0.0)
    t = np_optim.fresh(p0.copy())
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    ref = torch.optim.Adam([q], lr=1e-2, betas=(0.9, 0.999), eps=0.0)
    for _ in range(20):
        g = rs.randn(257)
        ours.step([t], [g])
        q.grad = torch.from_numpy(g.copy())
        ref.step()
        np.testing.assert_allclose(t["p"], q.detach().numpy(), rtol=1e-12, atol=0)


def test_epsilon_sits_beside_the_uncorrected_sqrt():
    """epsilon = 1e-8 on gradients of 1e-6, step 1: the restatement equals the hand case (lr 50/51) and does NOT equal torch.optim.Adam
    (lr 100/101: its epsilon is added after sqrt(v) has been divided by sqrt(1 - b2^t))."""
    case = [c for c in hand.CASES if c["name"] == "epsilon_beside_the_uncorrected_sqrt"][0]
    kw = _kw(case)
    p0, g = np.array(hand.floats(case["p0"])), np.array(hand.floats(case["grads"][0]))
    ours = np_optim.Adam(**kw)
    t = np_optim.fresh(p0.copy())
    ours.step([t], [g])
    np.testing.assert_allclose(t["p"], hand.floats(case["expect"][0]["p"]), rtol=hand.RTOL, atol=0)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    ref = torch.optim.Adam([q], lr=kw["lr"], betas=(kw["beta_1"], kw["beta_2"]), eps=kw["epsilon"])
    q.grad = torch.from_numpy(g.copy())
    ref.step()
    moved_ours, moved_torch = p0 - t["p"], p0 - q.detach().numpy()
    np.testing.assert_allclose(moved_torch, kw["lr"] * np.sign(g) * 100 / 101, rtol=1e-12)
    assert np.all(np.abs(moved_ours / moved_torch - 1.0) > 5e-3)


def _mk(dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    shapes = [(8, 3, 3, 3), (7,), (5, 11)]
    return [torch.nn.Parameter(torch.randn(s, generator=g, dtype=dtype)) for s in shapes]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("amsgrad,decay", [(False, 0.0), (True, 0.0), (False, 0.05), (True, 0.05)])
def test_package_adam_on_cpu_follows_the_restatement(dtype, amsgrad, decay):
    """CPU parameters take plain tensor expressions of the rule, the scalars advanced on the host: the same operations in the same
    order as the restatement, two groups (weight decay in one), amsgrad and decay on and off.  float32: every operation is a single
    correctly rounded IEEE operation in both (the square root taken in float64 and rounded once), so bit for bit.  float64: the
    framework's vectorised CPU square root is NOT correctly rounded (one ulp off NumPy's on 0.7 % of a million values), which moves
    an update by at most ~2 ulp of itself and p by an ulp per step, fed back through the weight decay: m and v to 1e-14 relative, p
    to 1e-13 (five steps, 450 x the rounding unit)."""
    from ssd_keras_amd.optimizers import Adam
    ps = _mk(dtype)
    hyper = dict(lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=decay, amsgrad=amsgrad)
    opt = Adam([{"params": ps[:2], "weight_decay": 1e-3}, {"params": ps[2:]}], **hyper)
    refs = [np_optim.Adam(weight_decay=1e-3, **hyper), np_optim.Adam(**hyper)]
    ts = [np_optim.fresh(p.detach().numpy().copy(), amsgrad) for p in ps]
    g = torch.Generator().manual_seed(9)
    for step in range(5):
        grads = [torch.randn(p.shape, generator=g, dtype=dtype) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        refs[0].step(ts[:2], [x.numpy() for x in grads[:2]])
        refs[1].step(ts[2:], [x.numpy() for x in grads[2:]])
        assert opt.iterations == step + 1
        for p, t in zip(ps, ts):
            st = opt.state[p]
            if dtype == torch.float32:
                assert np.array_equal(p.detach().numpy(), t["p"]), step
                assert all(np.array_equal(st[n].numpy(), t[n]) for n in (("m", "v", "vhat") if amsgrad else ("m", "v"))), step
            else:
                np.testing.assert_allclose(p.detach().numpy(), t["p"], rtol=1e-13, atol=1e-15)    # (|p| <= 4: a p that lands near 0)
                for n in ("m", "v", "vhat") if amsgrad else ("m", "v"):
                    np.testing.assert_allclose(st[n].numpy(), t[n], rtol=1e-14, atol=0)


def test_state_dict_round_trip_continues_at_the_saved_step():
    """A checkpoint taken after step 2 carries the step count and the running products: the restored optimizer's step 3 is the
    uninterrupted run's step 3 (bias correction of step 3, not of step 1), in a fresh optimizer and through pickle / deepcopy."""
    import pickle
    from ssd_keras_amd.optimizers import Adam
    a, b = _mk(torch.float32), _mk(torch.float32)
    g = torch.Generator().manual_seed(1)
    grads = [[torch.randn(p.shape, generator=g) for p in a] for _ in range(3)]
    one = Adam(a, lr=1e-2, epsilon=1e-8, amsgrad=True)
    for k in range(2):
        for p, gr in zip(a, grads[k]):
            p.grad = gr.clone()
        one.step()
    ck = copy.deepcopy(one.state_dict())
    assert ck["state"]["adam_host"]["iterations"] == 2
    with torch.no_grad():
        for p, q in zip(a, b):
            q.copy_(p)
    two = Adam(b, lr=1e-2, epsilon=1e-8, amsgrad=True)
    two.load_state_dict(ck)
    assert two.iterations == 2
    three = pickle.loads(pickle.dumps(one))
    assert three.iterations == 2 and three._tables == {}
    for opt, ps in ((one, a), (two, b)):
        for p, gr in zip(ps, grads[2]):
            p.grad = gr.clone()
        opt.step()
        assert opt.iterations == 3
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    assert ck["state"]["adam_host"]["iterations"] == 2                    # the checkpoint itself was not stepped


def test_keras_names_defaults_and_bad_hyperparameters():
    from ssd_keras_amd.optimizers import Adam
    sig = inspect.signature(Adam.__init__)
    assert list(sig.parameters)[1:] == ["params", "lr", "beta_1", "beta_2", "epsilon", "decay", "amsgrad", "weight_decay"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["lr"], d["beta_1"], d["beta_2"], d["epsilon"], d["decay"], d["amsgrad"], d["weight_decay"]) == (0.001, 0.9, 0.999, None, 0.0, False, 0.0)
    p = torch.nn.Parameter(torch.zeros(3))
    opt = Adam([p])
    assert opt.param_groups[0]["epsilon"] == 1e-7 and opt.iterations == 0            # K.epsilon()
    assert isinstance(opt, torch.optim.Optimizer)
    for bad in (dict(lr=-1.0), dict(beta_1=1.0), dict(beta_1=-0.1), dict(beta_2=1.0), dict(epsilon=-1e-8), dict(decay=-1.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            Adam([p], **bad)
    with pytest.raises(ValueError):
        Adam([{"params": [p], "beta_2": 1.5}])
    # a learning-rate scheduler drives it through param_groups
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    p.grad = torch.ones(3)
    opt.step()
    sched.step()
    assert opt.param_groups[0]["lr"] == 0.0005
    ref = np_optim.Adam()
    t = np_optim.fresh(np.zeros(3, dtype=np.float32))
    ref.step([t], [np.ones(3, dtype=np.float32)])
    ref.lr = 0.0005
    ref.step([t], [np.ones(3, dtype=np.float32)])
    opt.step()
    assert np.array_equal(p.detach().numpy(), t["p"])
    opt.set_lr(0.25)
    assert opt.param_groups[0]["lr"] == 0.25


def test_adam_exports_are_declared_and_documented():
    """The four exports of csrc/ssdhip_adam.hip have ctypes signatures in the one table of _native.py, prototypes and a description
    in include/ssdhip.h, and rows in INTEGRATION.md."""
    from ssd_keras_amd import _native as nat
    hdr = open(os.path.join(ROOT, "include", "ssdhip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("ssdhip_adam_state_bytes", "ssdhip_adam_state_init", "ssdhip_adam_step", "ssdhip_optim_set_lr"):
        assert name in nat.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in doc, name
    assert nat.ADAM_GROUP.itemsize == 80 and nat.ADAM_STATE_HEAD.itemsize == 16
    lib = nat.load()
    assert lib.ssdhip_adam_state_bytes(2) == 16 + 2 * 80 and lib.ssdhip_adam_state_bytes(0) == 0 and lib.ssdhip_adam_state_bytes(65) == 0
    assert lib.ssdhip_adam_step(0, None, None, None, None, None, None, 0, None, 0, None) == -1          # SSDHIP_E_BADARG, no launch
    assert lib.ssdhip_optim_set_lr(None, 0, 0.1, None) == -1
    assert lib.ssdhip_adam_state_init(None, 1, 0, 1e-3, 0.9, 0.999, 1e-7, 0.0, 0.0, 0, None) == -1


def test_group_limit_is_a_value_error_at_the_call():
    """The device state block holds 64 parameter groups: the 65th is refused where it is added, in the constructor or later."""
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.optimizers import Adam
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in range(nat.ADAM_MAX_GROUPS + 1)]
    with pytest.raises(ValueError):
        Adam([{"params": [p]} for p in ps])
    opt = Adam([{"params": [p]} for p in ps[:-1]])
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [ps[-1]]})
    assert len(opt.param_groups) == nat.ADAM_MAX_GROUPS
