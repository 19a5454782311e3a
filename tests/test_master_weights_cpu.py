"""`master_weights=True` of ssd_keras_amd.optimizers without a GPU: bf16 parameters updated through float32 masters on the
tensor-expression path.  The hand cases of tests/master_hand_cases.py (and the defect they are about: without masters the same run
never moves), masters and moments bit for bit against the float32 restatements tests/np_sgd.py / tests/np_optim.py fed float32(p0) and
float32(g), the parameter as the exact rounding of its master, and the bookkeeping: checkpoints, copies, re-seeding after somebody
else wrote the parameter."""
import copy
import pickle

import numpy as np
import pytest
import torch

from tests import master_hand_cases as hand
from tests import np_optim, np_sgd

SHAPES = [(5,), (3, 2, 3, 3), (17,)]                       # (the second one channels_last)


def _params(seed=3, dtype=torch.bfloat16, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    ps = []
    for s in shapes:
        t = torch.randn(s, generator=g).to(dtype)
        if len(s) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(t))
    return ps


def _grads(ps, gen):
    out = []
    for p in ps:
        gr = torch.randn(p.shape, generator=gen).to(p.dtype)
        out.append(gr.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else gr)
    return out


def _set_grads(ps, grads):
    for p, gr in zip(ps, grads):
        p.grad = gr.clone(memory_format=torch.preserve_format)


def _np32(t):
    return t.detach().float().numpy().copy()


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _assert_master_state(opt, ps, ts, names, where):
    """Masters and buffers bit-equal to the restatement's float32 arrays (`names`: state key -> restatement key); p is the rounding of
    its master, bit for bit; everything float32 and in the parameter's layout."""
    for i, (p, t) in enumerate(zip(ps, ts)):
        st = opt.state[p]
        for key, ref in names.items():
            got = st[key]
            assert got.dtype == torch.float32 and got.stride() == p.stride(), (where, i, key)
            assert np.array_equal(_bits32(got.numpy()), _bits32(t[ref])), "%s: %s of tensor %d" % (where, key, i)
        assert p.dtype == torch.bfloat16
        assert np.array_equal(hand.bits_of(p).view(np.int16), hand.bf16_round_bits(st["master"].contiguous().numpy()).view(np.int16)), (where, i)


# ---- the hand cases ------------------------------------------------------------------------------------------------------------------
def run_sgd_hand_case(device, master_weights, check_each_step=True):
    """The SGD case of tests/master_hand_cases.py on `device`; returns (p, optimizer)."""
    from ssd_keras_amd.optimizers import SGD
    p = torch.nn.Parameter(torch.tensor(hand.floats(hand.P0), dtype=torch.bfloat16, device=device))
    opt = SGD([p], master_weights=master_weights, **hand.kwargs(hand.SGD_KW))
    for k in range(1, hand.SGD_STEPS + 1):
        p.grad = torch.tensor(hand.floats(hand.GRAD), dtype=torch.bfloat16, device=device)
        opt.step()
        if master_weights and check_each_step:
            st = opt.state[p]
            assert st["master"].dtype == torch.float32 and st["velocity"].dtype == torch.float32
            assert st["master"].tolist() == hand.floats([hand.sgd_master(w0, k) for w0 in hand.P0]), k         # exact: every value is dyadic
            assert st["velocity"].tolist() == hand.floats([hand.sgd_velocity(k)] * 3), k
            assert p.detach().float().tolist() == hand.floats([col[k - 1] for col in hand.SGD_P]), k
    return p, opt


def run_adam_hand_case(device):
    from ssd_keras_amd.optimizers import Adam
    p = torch.nn.Parameter(torch.tensor(hand.floats(hand.P0), dtype=torch.bfloat16, device=device))
    opt = Adam([p], master_weights=True, **hand.kwargs(hand.ADAM_KW))
    for k in range(1, hand.ADAM_STEPS + 1):
        p.grad = torch.tensor(hand.floats(hand.GRAD), dtype=torch.bfloat16, device=device)
        opt.step()
        master = opt.state[p]["master"].cpu()
        np.testing.assert_allclose(master.numpy(), hand.floats([hand.adam_master(w0, k) for w0 in hand.P0]), rtol=hand.ADAM_RTOL, atol=0,
                                   err_msg="master, step %d" % k)
        assert np.array_equal(hand.bits_of(p), hand.bf16_round_bits(master.numpy())), k                       # p == bf16(master), exactly
        assert p.detach().float().tolist() == hand.floats([col[k - 1] for col in hand.ADAM_P]), k
    return p, opt


def test_sgd_hand_case():
    p, opt = run_sgd_hand_case("cpu", True)
    assert opt.iterations == hand.SGD_STEPS
    # the step at which each value first leaves its start: worked out by hand, read off the table the run was checked against
    for col, p0, first in zip(hand.SGD_P, hand.P0, hand.SGD_FIRST_MOVE):
        assert [k + 1 for k, v in enumerate(col) if v != p0][0] == first


def test_adam_hand_case():
    p, opt = run_adam_hand_case("cpu")
    assert opt.iterations == hand.ADAM_STEPS


def test_without_masters_the_same_run_never_moves():
    """The defect the option is for, asserted so that `master_weights=False` stays what it was: every update is below half a bf16 step
    of the weight and rounds to nothing, twelve times.  With masters, every one of the three values has moved."""
    stuck, _ = run_sgd_hand_case("cpu", False)
    assert stuck.dtype == torch.bfloat16 and stuck.detach().float().tolist() == hand.floats(hand.P0)
    moved, _ = run_sgd_hand_case("cpu", True, check_each_step=False)
    assert all(a != b for a, b in zip(moved.detach().float().tolist(), hand.floats(hand.P0)))


# ---- masters against the float32 restatements ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,nesterov", [("torch", False), ("torch", True), ("keras", False), ("keras", True)])
def test_sgd_masters_follow_the_float32_restatement(rule, nesterov):
    from ssd_keras_amd.optimizers import SGD
    ps = _params()
    hyper = dict(lr=1e-2, momentum=0.9, decay=0.05, nesterov=nesterov, rule=rule)
    opt = SGD([{"params": ps[:2], "weight_decay": 1e-3}, {"params": ps[2:]}], master_weights=True, **hyper)
    refs = [np_sgd.SGD(weight_decay=1e-3, **hyper), np_sgd.SGD(**hyper)]
    ts = [np_sgd.fresh(_np32(p)) for p in ps]
    gen = torch.Generator().manual_seed(9)
    name = "momentum_buffer" if rule == "torch" else "velocity"
    for step in range(3):
        grads = _grads(ps, gen)
        _set_grads(ps, grads)
        opt.step()
        refs[0].step(ts[:2], [_np32(g) for g in grads[:2]])
        refs[1].step(ts[2:], [_np32(g) for g in grads[2:]])
        assert opt.iterations == step + 1
        _assert_master_state(opt, ps, ts, {"master": "p", name: "buf"}, "step %d" % (step + 1))


@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam_masters_follow_the_float32_restatement(amsgrad):
    from ssd_keras_amd.optimizers import Adam
    ps = _params()
    hyper = dict(lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.05, amsgrad=amsgrad)
    opt = Adam([{"params": ps[:2], "weight_decay": 1e-3}, {"params": ps[2:]}], master_weights=True, **hyper)
    refs = [np_optim.Adam(weight_decay=1e-3, **hyper), np_optim.Adam(**hyper)]
    ts = [np_optim.fresh(_np32(p), amsgrad) for p in ps]
    gen = torch.Generator().manual_seed(9)
    names = {"master": "p", "m": "m", "v": "v"}
    if amsgrad:
        names["vhat"] = "vhat"
    for step in range(3):
        grads = _grads(ps, gen)
        _set_grads(ps, grads)
        opt.step()
        refs[0].step(ts[:2], [_np32(g) for g in grads[:2]])
        refs[1].step(ts[2:], [_np32(g) for g in grads[2:]])
        assert opt.iterations == step + 1
        _assert_master_state(opt, ps, ts, names, "step %d" % (step + 1))


def test_sgd_without_momentum_keeps_a_master_too():
    """Momentum 0 keeps no buffer and always takes the expressions: the master is the only state."""
    from ssd_keras_amd.optimizers import SGD
    ps = _params()
    opt = SGD(ps, lr=1e-2, weight_decay=1e-3, master_weights=True)
    ref = np_sgd.SGD(lr=1e-2, momentum=0.9, weight_decay=1e-3)              # (one step from a zero buffer: buf = g, p -= lr g)
    ts = [np_sgd.fresh(_np32(p)) for p in ps]
    grads = _grads(ps, torch.Generator().manual_seed(2))
    _set_grads(ps, grads)
    opt.step()
    ref.step(ts, [_np32(g) for g in grads])
    assert all(set(opt.state[p]) == {"master"} for p in ps)
    _assert_master_state(opt, ps, ts, {"master": "p"}, "step 1")


# ---- state and bookkeeping -----------------------------------------------------------------------------------------------------------
def _make(kind, ps, **kw):
    from ssd_keras_amd.optimizers import SGD, Adam
    if kind == "sgd":
        return SGD(ps, lr=1e-2, momentum=0.9, weight_decay=1e-3, rule="keras", master_weights=True, **kw)
    return Adam(ps, lr=1e-2, epsilon=1e-8, amsgrad=True, weight_decay=1e-3, master_weights=True, **kw)


def _same_everything(opt_a, a, opt_b, b):
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        sa, sb = opt_a.state[p], opt_b.state[q]
        assert set(sa) == set(sb) and "master" in sa
        for k in sa:
            assert sa[k].dtype == torch.float32 and sb[k].dtype == torch.float32 and torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_checkpoints_and_copies_continue_bit_for_bit(kind):
    """state_dict -> a fresh optimizer -> load_state_dict, copy.deepcopy and pickle: each continues exactly as the uninterrupted run
    (the masters and float32 moments travel as ordinary per-parameter state; the framework's cast of loaded state to the parameter's
    dtype would have rounded them to bf16)."""
    a = _params()
    gen = torch.Generator().manual_seed(1)
    grads = [_grads(a, gen) for _ in range(4)]
    one = _make(kind, a)
    for k in range(2):
        _set_grads(a, grads[k])
        one.step()
    ck = copy.deepcopy(one.state_dict())
    b = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in a]
    two = _make(kind, b)
    two.load_state_dict(ck)
    assert two.iterations == 2 and all(two.state[q]["master"].dtype == torch.float32 for q in b)
    assert not any(torch.equal(two.state[q]["master"], q.detach().float()) for q in b)      # the master carries more than p does
    _set_grads(a, grads[2])                                       # (copies carry the gradients with them)
    three, four = copy.deepcopy(one), pickle.loads(pickle.dumps(one))
    assert three._tables == {} and four._tables == {}
    copies = [(two, b)] + [(o, [p for grp in o.param_groups for p in grp["params"]]) for o in (three, four)]
    for k in (2, 3):
        _set_grads(a, grads[k])
        one.step()
        for opt, ps in copies:
            _set_grads(ps, grads[k])
            opt.step()
            assert opt.iterations == k + 1
            _same_everything(one, a, opt, ps)


@pytest.mark.parametrize("explicit", [False, True], ids=["found_by_step", "sync_masters"])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_a_write_to_the_parameter_reseeds_its_master(kind, explicit):
    """Somebody else writes p between two steps (what model.load_state_dict does): the next step starts from float32(p), with the
    moments it had -- found through the parameter's `_version`, or on request through sync_masters()."""
    ps = _params()
    opt = _make(kind, ps)
    if kind == "sgd":
        ref, fresh, names = np_sgd.SGD(lr=1e-2, momentum=0.9, weight_decay=1e-3, rule="keras"), np_sgd.fresh, {"master": "p", "velocity": "buf"}
    else:
        ref, fresh = np_optim.Adam(lr=1e-2, epsilon=1e-8, amsgrad=True, weight_decay=1e-3), (lambda p: np_optim.fresh(p, True))
        names = {"master": "p", "m": "m", "v": "v", "vhat": "vhat"}
    ts = [fresh(_np32(p)) for p in ps]
    gen = torch.Generator().manual_seed(4)
    for step in range(3):
        if step == 2:
            written = _params(seed=77)
            with torch.no_grad():
                for p, w in zip(ps, written):
                    p.copy_(w)
            for t, w in zip(ts, written):
                t["p"] = _np32(w)
            if explicit:
                opt.sync_masters()
                assert all(torch.equal(opt.state[p]["master"], p.detach().float()) for p in ps)
        grads = _grads(ps, gen)
        _set_grads(ps, grads)
        opt.step()
        ref.step(ts, [_np32(g) for g in grads])
        _assert_master_state(opt, ps, ts, names, "step %d" % (step + 1))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_the_option_cannot_change_after_the_first_step(kind):
    ps = _params()
    opt = _make(kind, ps)
    _set_grads(ps, _grads(ps, torch.Generator().manual_seed(4)))
    opt.step()
    opt.param_groups[0]["master_weights"] = False
    with pytest.raises(ValueError, match="master_weights"):
        opt.step()
    opt.param_groups[0]["master_weights"] = True
    opt.step()
    assert opt.iterations == 2


def test_the_option_is_a_group_setting():
    from ssd_keras_amd.optimizers import SGD, Adam
    ps = _params()
    for cls in (SGD, Adam):
        assert cls(ps).defaults["master_weights"] is False
        opt = cls([{"params": ps[:1], "master_weights": True}, {"params": ps[1:]}])
        assert [g["master_weights"] for g in opt.param_groups] == [True, False]
        assert opt._tag(opt.param_groups[0]) != opt._tag(opt.param_groups[1])
    # per group: the first group's parameter gets a master, the others are updated in bf16 as before
    opt = SGD([{"params": ps[:1], "master_weights": True}, {"params": ps[1:]}], lr=1e-2, momentum=0.9)
    _set_grads(ps, _grads(ps, torch.Generator().manual_seed(4)))
    opt.step()
    assert "master" in opt.state[ps[0]] and opt.state[ps[0]]["momentum_buffer"].dtype == torch.float32
    assert all("master" not in opt.state[p] and opt.state[p]["momentum_buffer"].dtype == torch.bfloat16 for p in ps[1:])


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_a_mixed_group_updates_both_and_float32_parameters_are_untouched_by_the_option(kind):
    """One group of float32 and bf16 parameters: the bf16 ones get masters, the float32 ones none, and these end with the bits they
    have with `master_weights=False` (the all-float32 optimizer: test_float32_only_parameters_ignore_the_option)."""
    from ssd_keras_amd.optimizers import SGD, Adam
    make = (lambda ps, mw: SGD(ps, lr=1e-2, momentum=0.9, weight_decay=1e-3, master_weights=mw)) if kind == "sgd" else \
        (lambda ps, mw: Adam(ps, lr=1e-2, epsilon=1e-8, weight_decay=1e-3, master_weights=mw))
    runs = {}
    for mw in (True, False):
        ps = _params(dtype=torch.float32, shapes=SHAPES[:2]) + _params(seed=5, shapes=SHAPES[2:])
        opt = make(ps, mw)
        gen = torch.Generator().manual_seed(6)
        for _ in range(3):
            _set_grads(ps, _grads(ps, gen))
            opt.step()
        runs[mw] = (ps, opt)
    (on, opt_on), (off, opt_off) = runs[True], runs[False]
    for p, q in zip(on[:2], off[:2]):
        assert p.dtype == torch.float32 and torch.equal(p, q) and "master" not in opt_on.state[p]
        assert all(torch.equal(opt_on.state[p][k], opt_off.state[q][k]) for k in opt_off.state[q])
    assert "master" in opt_on.state[on[2]] and "master" not in opt_off.state[off[2]]
    assert not torch.equal(on[2], _params(seed=5, shapes=SHAPES[2:])[0])                 # the bf16 parameter was updated too
    assert torch.equal(on[2], opt_on.state[on[2]]["master"].to(torch.bfloat16))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_float32_only_parameters_ignore_the_option(kind):
    """`master_weights=True` on parameters that are all float32 is `master_weights=False`: three steps, equal parameter bits, equal
    state keys and tensors (the host's scalars too), and no `master` anywhere."""
    from ssd_keras_amd.optimizers import SGD, Adam
    make = (lambda ps, mw: SGD(ps, lr=1e-2, momentum=0.9, weight_decay=1e-3, decay=0.05, nesterov=True, master_weights=mw)) if kind == "sgd" else \
        (lambda ps, mw: Adam(ps, lr=1e-2, epsilon=1e-8, weight_decay=1e-3, decay=0.05, amsgrad=True, master_weights=mw))
    runs = {}
    for mw in (True, False):
        ps = _params(dtype=torch.float32)
        opt = make(ps, mw)
        gen = torch.Generator().manual_seed(6)
        for _ in range(3):
            _set_grads(ps, _grads(ps, gen))
            opt.step()
        runs[mw] = (ps, opt)
    (on, opt_on), (off, opt_off) = runs[True], runs[False]
    assert opt_on.iterations == 3 == opt_off.iterations
    assert not torch.equal(on[0], _params(dtype=torch.float32)[0])                       # (they were updated)
    for p, q in zip(on, off):
        assert p.dtype == torch.float32 and np.array_equal(_bits32(p.detach().numpy()), _bits32(q.detach().numpy()))
        sp, sq = opt_on.state[p], opt_off.state[q]
        assert set(sp) == set(sq) and "master" not in sp
        for k in sq:
            assert sp[k].dtype == torch.float32 and np.array_equal(_bits32(sp[k].numpy()), _bits32(sq[k].numpy())), k
    host = kind + "_host"
    assert opt_on.state[host] == opt_off.state[host]
    assert [k for k in opt_on.state if isinstance(k, str)] == [host]


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_weights_loaded_after_init_state_are_found(kind):
    """init_state() makes the masters; the model's weights are written afterwards (a checkpoint loaded late); the first step starts from
    the written values, not from the masters of init_state()."""
    ps = _params()
    opt = _make(kind, ps)
    gen = torch.Generator().manual_seed(4)
    grads = _grads(ps, gen)
    _set_grads(ps, grads)
    opt.init_state()
    assert all(torch.equal(opt.state[p]["master"], p.detach().float()) for p in ps)
    written = _params(seed=77)
    with torch.no_grad():
        for p, w in zip(ps, written):
            p.copy_(w)
    if kind == "sgd":
        ref, ts, names = np_sgd.SGD(lr=1e-2, momentum=0.9, weight_decay=1e-3, rule="keras"), [np_sgd.fresh(_np32(w)) for w in written], \
            {"master": "p", "velocity": "buf"}
    else:
        ref, ts = np_optim.Adam(lr=1e-2, epsilon=1e-8, amsgrad=True, weight_decay=1e-3), [np_optim.fresh(_np32(w), True) for w in written]
        names = {"master": "p", "m": "m", "v": "v", "vhat": "vhat"}
    opt.step()
    ref.step(ts, [_np32(g) for g in grads])
    _assert_master_state(opt, ps, ts, names, "step 1")


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_a_checkpoint_saved_without_masters_gets_float32_moments(kind):
    """A checkpoint of a `master_weights=False` run has bf16 moments.  Loaded, and the option switched on before the next step, the
    masters are made from the parameters and the moments widened (exact): the next step equals the float32 restatement started from
    float32(p) and float32(moments)."""
    from ssd_keras_amd.optimizers import SGD, Adam
    make = (lambda ps: SGD(ps, lr=1e-2, momentum=0.9, rule="keras")) if kind == "sgd" else (lambda ps: Adam(ps, lr=1e-2, epsilon=1e-8))
    ps = _params()
    old = make(ps)
    gen = torch.Generator().manual_seed(4)
    for _ in range(2):
        _set_grads(ps, _grads(ps, gen))
        old.step()
    new = make(ps)
    new.load_state_dict(copy.deepcopy(old.state_dict()))
    moments = ("velocity",) if kind == "sgd" else ("m", "v")
    assert all(new.state[p][n].dtype == torch.bfloat16 for p in ps for n in moments)
    for group in new.param_groups:
        group["master_weights"] = True
    if kind == "sgd":
        ref = np_sgd.SGD(lr=1e-2, momentum=0.9, rule="keras", iterations=2)
        ts = [{"p": _np32(p), "buf": _np32(new.state[p]["velocity"])} for p in ps]
        names = {"master": "p", "velocity": "buf"}
    else:
        ref = np_optim.Adam(lr=1e-2, epsilon=1e-8, iterations=2)
        ts = [{"p": _np32(p), "m": _np32(new.state[p]["m"]), "v": _np32(new.state[p]["v"]), "vhat": None} for p in ps]
        names = {"master": "p", "m": "m", "v": "v"}
    grads = _grads(ps, gen)
    _set_grads(ps, grads)
    new.step()
    ref.step(ts, [_np32(g) for g in grads])
    assert new.iterations == 3
    _assert_master_state(new, ps, ts, names, "step 3")
