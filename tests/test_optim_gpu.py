"""`ssd_keras_amd.optimizers.Adam` on the GPU (csrc/ssdhip_adam.hip): the one-launch update against the NumPy restatement of Keras 2.x
Adam (tests/np_optim.py) BIT FOR BIT -- same operations, same order, contraction off, correctly rounded float32 divide and square
root, float64 scalars by the same running products --, more tensors than a launch holds, checkpoints and copies, the step replayed as
a HIP graph with the learning rate changed between replays, SSD7 trained end to end, and SSD300's whole step with Adam as ONE graph.
Reference: keras.optimizers.Adam as the notebooks construct it, ssd7_training.ipynb:153.  Needs an MI355X."""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import adam_hand_cases as hand
from tests import np_optim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(64, 3, 3, 3), (7,), (512, 256, 3, 3), (1000003,), (33, 5)]      # ragged; > 1 M elements; not multiples of 4; channels_last


def _params(torch, shapes=SHAPES, seed=11, channels_last=(2,)):
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + i)))
          for i, s in enumerate(shapes)]
    with torch.no_grad():
        for i in channels_last:
            if i < len(ps) and ps[i].dim() == 4:
                ps[i].data = ps[i].data.contiguous(memory_format=torch.channels_last)
    return ps


def _grad_like(torch, p, gen):
    gr = torch.randn(p.shape, device="cuda", generator=gen)
    return gr.contiguous(memory_format=torch.channels_last) if p.dim() == 4 and not p.is_contiguous() else gr


def _same_bits(torch, opt, ps, ts, amsgrad, where):
    for i, (p, t) in enumerate(zip(ps, ts)):
        st = opt.state[p]
        for name, got in (("p", p.detach()), ("m", st["m"]), ("v", st["v"])) + ((("vhat", st["vhat"]),) if amsgrad else ()):
            got = got.cpu().numpy()
            bad = int((got.view(np.int32) != t[name].view(np.int32)).sum())
            assert bad == 0, "%s: %s of tensor %d differs in %d of %d values (max |d| %.3g)" % (
                where, name, i, bad, got.size, float(np.abs(got.astype(np.float64) - t[name]).max()))


@pytest.mark.parametrize("amsgrad,decay", [(False, 0.0), (True, 0.0), (False, 0.05), (True, 0.05)])
def test_one_launch_adam_equals_the_restatement_bit_for_bit(amsgrad, decay):
    """Five steps on ragged sizes (one above a million elements, sizes that are no multiple of 4, a channels_last filter tensor), two
    groups with weight decay in one: p, m, v, vhat bit-equal to the float32 restatement, `iterations` equal, every `_version` moves."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    ps = _params(torch)
    hyper = dict(lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=decay, amsgrad=amsgrad)
    opt = Adam([{"params": ps[:3], "weight_decay": 1e-3}, {"params": ps[3:]}], **hyper)
    refs = [np_optim.Adam(weight_decay=1e-3, **hyper), np_optim.Adam(**hyper)]
    ts = [np_optim.fresh(p.detach().cpu().numpy(), amsgrad) for p in ps]
    gen = torch.Generator(device="cuda").manual_seed(5)
    for step in range(5):
        v0 = [p._version for p in ps]
        grads = [_grad_like(torch, p, gen) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone(memory_format=torch.preserve_format)
        opt.step()
        assert all(p._version > v for p, v in zip(ps, v0))
        refs[0].step(ts[:3], [g.cpu().numpy() for g in grads[:3]])
        refs[1].step(ts[3:], [g.cpu().numpy() for g in grads[3:]])
        assert opt.iterations == step + 1 == refs[0].iterations
        _same_bits(torch, opt, ps, ts, amsgrad, "step %d" % (step + 1))
    assert opt.state[ps[2]]["m"].is_contiguous(memory_format=torch.channels_last)          # moments in the parameter's layout
    assert "adam_host" not in opt.state                                                    # nothing went through the expressions


@pytest.mark.parametrize("case", hand.CASES, ids=[c["name"] for c in hand.CASES])
def test_kernel_on_the_hand_cases(case):
    """The hand-worked values (exact fractions) through the kernel: float32 arithmetic, so to 1e-6 relative (a handful of roundings
    of 6e-8 each; the cancellation p - update loses at most a factor 4)."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    kw = {k: (float(v) if not isinstance(v, bool) else v) for k, v in case["kw"].items()}
    p = torch.nn.Parameter(torch.tensor(hand.floats(case["p0"]), dtype=torch.float32, device="cuda"))
    opt = Adam([p], **kw)
    for k, (g, want) in enumerate(zip(case["grads"], case["expect"])):
        p.grad = torch.tensor(hand.floats(g), dtype=torch.float32, device="cuda")
        opt.step()
        got = dict(p=p.detach(), **{n: opt.state[p][n] for n in want if n != "p"})
        for name, vals in want.items():
            np.testing.assert_allclose(got[name].cpu().numpy(), hand.floats(vals), rtol=1e-6, atol=0, err_msg="%s, step %d" % (name, k + 1))
    assert "adam_host" not in opt.state


def test_more_tensors_than_one_launch_holds():
    """150 small tensors (a launch carries 72 in its arguments): every tensor is updated exactly once per step and `iterations`
    advances once per step, whatever the number of launches."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    shapes = [(k + 1,) for k in range(150)]
    ps = _params(torch, shapes, seed=100, channels_last=())
    opt = Adam(ps, lr=1e-2, epsilon=1e-8)
    ref = np_optim.Adam(lr=1e-2, epsilon=1e-8)
    ts = [np_optim.fresh(p.detach().cpu().numpy()) for p in ps]
    gen = torch.Generator(device="cuda").manual_seed(6)
    for step in range(2):
        grads = [torch.randn(p.shape, device="cuda", generator=gen) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        ref.step(ts, [g.cpu().numpy() for g in grads])
        assert opt.iterations == step + 1
        _same_bits(torch, opt, ps, ts, False, "step %d" % (step + 1))


def test_fused_adam_survives_load_state_dict_and_copies():
    """The scenarios of test_fused_sgd_survives_load_state_dict_and_copies (the step caches raw pointers to the parameter, the
    gradient, m and v): step, load_state_dict of a checkpoint taken after step 1 (new buffer tensors, gradients where they were),
    step -- and the restored run's step 2 is the uninterrupted run's step 2 bit for bit (the bias correction of step 2, not of
    step 1); a pickled optimizer carries no table; a deep copy updates ITS tensors."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    shapes = [(64, 3, 3, 3), (129,), (256, 128, 3, 3)]
    a, b = _params(torch, shapes, seed=3, channels_last=()), _params(torch, shapes, seed=3, channels_last=())
    ours, twin_run = Adam(a, lr=1e-2, epsilon=1e-8, weight_decay=1e-4), Adam(b, lr=1e-2, epsilon=1e-8, weight_decay=1e-4)
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
    ours.load_state_dict(ck)                                       # back to the moments and the step count of step 1
    assert ours.iterations == 1
    with torch.no_grad():
        for p, was in zip(a, after_1):
            p.copy_(was)
    step(ours, a, 1)                                               # the restored run's step 2 ...
    step(twin_run, b, 1)                                           # ... and the uninterrupted run's
    assert ours.iterations == 2 == twin_run.iterations
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        assert torch.equal(ours.state[p]["m"], twin_run.state[q]["m"]) and torch.equal(ours.state[p]["v"], twin_run.state[q]["v"])
    # copies: no stale table travels, the first step of the copy rebuilds it against ITS tensors and ITS state block
    clone = pickle.loads(pickle.dumps(ours))
    assert clone._tables == {} and clone.iterations == 2
    twin = copy.deepcopy(ours)
    before = [p.detach().clone() for p in a]
    tp = [p for grp in twin.param_groups for p in grp["params"]]
    for p, q in zip(tp, a):
        p.grad = q.grad.clone()
    twin.step()
    for q, was in zip(a, before):
        assert torch.equal(q, was)                                 # the original's parameters were not touched by the copy's step
    assert all(not torch.equal(p, was) for p, was in zip(tp, before))
    assert twin.iterations == 3 and ours.iterations == 2           # nor was its step count


def test_captured_step_replays_with_the_scalars_of_its_own_step():
    """`opt.step()` captured ONCE on static gradient tensors (a linear graph), replayed eight times with fresh gradients copied in,
    `set_lr` after the fourth replay: parameters and moments bit-equal to eight steps of the restatement with that schedule.  With
    the bias correction or the learning rate in the kernel arguments every replay would repeat step 1."""
    import torch
    from ssd_keras_amd.optimizers import Adam
    ps = _params(torch, [(64, 3, 3, 3), (129,), (300000,)], seed=21, channels_last=(0,))
    opt = Adam([{"params": ps[:1], "weight_decay": 1e-3}, {"params": ps[1:]}], lr=1e-2, epsilon=1e-8, amsgrad=True)
    refs = [np_optim.Adam(lr=1e-2, epsilon=1e-8, amsgrad=True, weight_decay=1e-3), np_optim.Adam(lr=1e-2, epsilon=1e-8, amsgrad=True)]
    ts = [np_optim.fresh(p.detach().cpu().numpy(), True) for p in ps]
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
        grads = [_grad_like(torch, p, gen) for p in ps]
        for p, gr in zip(ps, grads):
            p.grad.copy_(gr)
        graph.replay()
        refs[0].step(ts[:1], [g.cpu().numpy() for g in grads[:1]])
        refs[1].step(ts[1:], [g.cpu().numpy() for g in grads[1:]])
        if k == 3:                                                 # from the fifth step on
            opt.set_lr(2.5e-3)
            for r in refs:
                r.lr = 2.5e-3
        torch.cuda.synchronize()
        _same_bits(torch, opt, ps, ts, True, "replay %d" % (k + 1))
    assert opt.iterations == 8


def test_ssd7_trains_with_adam_end_to_end():
    """build_model (SSD7) + HIP encoder + HIP SSDLoss + Adam(lr=0.001, epsilon=1e-08) as ssd7_training.ipynb:153 compiles it, six
    steps on synthetic data: the loss descends, and after every step the parameters equal those of a shadow copy driven by the
    tensor-expression path (the `_fused = False` test hook) from the SAME gradients.  Both are the same float32 operations in the same order with a
    correctly rounded root and quotient, so the tolerance is zero: bit for bit (measured on an MI355X: 0 differing values in each of
    the six steps, losses 20.93 -> 12.14; profiles/adam_pytest_optim_gpu.txt)."""
    import torch
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    from ssd_keras_amd.models.keras_ssd7 import build_model
    from ssd_keras_amd.optimizers import Adam
    from ssd_keras_amd.ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder
    cfg = syn.SSD7_300
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = build_model((300, 300, 3), cfg["n_classes"], mode="training", l2_regularization=0.0005, scales=cfg["scales"],
                        aspect_ratios_global=cfg["aspect_ratios_global"], variances=cfg["variances"], normalize_coords=True,
                        subtract_mean=127.5, divide_by_stddev=127.5).to(dev).train()
    enc = SSDInputEncoder(matching_type="multi", pos_iou_threshold=0.5, neg_iou_limit=0.3, **cfg)
    B = 4
    gt = syn.make_ground_truth(B, cfg["n_classes"], 300, 300, max_boxes=8, seed=0)
    images = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(B, 300, 300, 3)).astype(np.float32)).to(dev)
    y_true, _, _ = enc.encode_to_device(gt, device=dev)
    lf = SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0)
    params = [p for p in model.parameters() if p.requires_grad]
    shadow = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in params]
    opt = Adam(params, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-08, decay=0.0)
    plain = Adam(shadow, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-08, decay=0.0)
    plain._fused = False
    losses, worst = [], 0
    for it in range(6):
        loss = lf.compute_loss(y_true, model(images)).mean() + model.l2_regularization_loss()
        opt.zero_grad()
        loss.backward()
        for p, q in zip(params, shadow):
            q.grad = p.grad.detach().clone(memory_format=torch.preserve_format)
        opt.step()
        plain.step()
        losses.append(float(loss.detach()))
        differing = sum(int((p.detach() != q.detach()).sum()) for p, q in zip(params, shadow))
        worst = max(worst, differing)
        print("step %d: loss %.5f, %d values differ between the kernel and the tensor expressions" % (it + 1, losses[-1], differing))
    assert opt.iterations == 6 == plain.iterations and "adam_host" not in opt.state and "adam_host" in plain.state
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert worst == 0


def test_whole_ssd300_step_with_adam_as_one_graph_under_the_default_runtime():
    """In the manner of test_whole_step_with_its_optimizer_as_one_graph_under_the_default_runtime: forward + SSDLoss + backward + the
    Adam tick and update launches captured once (tools/debug_graph_rounds.py with DBG_ADAM=1) and replayed under the runtime's
    defaults -- per round the replay agrees with an eager forward + backward on the same weights, the weights move every round
    and the loss descends."""
    e = dict(os.environ)
    e.pop("DEBUG_CLR_GRAPH_PACKET_CAPTURE", None)
    e.update(DBG_LR="1e-7", DBG_ROUNDS="6", DBG_ADAM="1", DBG_OPT_IN_GRAPH="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "debug_graph_rounds.py")], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ROUNDS")][-1]
    print(line)
    assert "ADAM_ITERATIONS=8" in line, line                      # two eager warm-up steps + six replays, counted on the device
    rounds = [tuple(float(v) for v in x.split("/")) for x in line.split("|")[1].split()]
    assert len(rounds) == 6
    losses = []
    for i, (le, lg, worst) in enumerate(rounds):
        assert abs(lg - le) <= 1e-4 * abs(le), "round %d: %s" % (i, line)
        assert worst <= 5e-2, "round %d: %s" % (i, line)
        losses.append(lg)
    assert len(set(losses)) == 6 and losses[-1] < losses[0], "the weights move every round and the loss descends: %s" % line
