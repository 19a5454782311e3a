"""`SSD7.fused_blocks(True, training=True, heads=True)` (models/keras_ssd7.py, models/_train_fns.py: _Ssd7HeadFn, _AssembleTrainFn): the
training step whose predictor heads and prediction assembly run in libssdhip, on the 76 x 68 test model of
tests/test_ssd7_fused_blocks_gpu.py at batch 3 (head maps 9 x 8, 4 x 4, 2 x 2 and 1 x 1 with 64, 48, 48 and 32 channels; 4 boxes of
3 + 1 classes: 32 packed channels of 48).  The kernels' arithmetic is tests/test_ssd7_head_kernels_gpu.py's."""
import copy

import pytest

from tests.test_ssd7_conv_training_gpu import _count, _node_counts
from tests.test_ssd7_fused_blocks_gpu import SIZE, _images
from tests.test_ssd7_fused_training_gpu import (_distance, _grads_equal, _state_equal, _step, _train_model, _y_true,
                                                deterministic_convolutions)  # noqa: F401  (the last one is a fixture)

pytestmark = pytest.mark.gpu


def _head_model(seed, convolutions=True, dtype="bfloat16"):
    return _train_model(seed, None, dtype=dtype).fused_blocks(True, training=True, convolutions=convolutions, heads=True)


def _parent_model(seed, dtype="bfloat16"):
    """The route this one is measured against: the blocks and the trunk convolutions in libssdhip, the framework's heads."""
    return _train_model(seed, None, dtype=dtype).fused_blocks(True, training=True, convolutions=True)


def test_routing(deterministic_convolutions, monkeypatch):  # noqa: F811
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    img = _images()
    on, parent = _head_model(3), _parent_model(3)
    y_true = _y_true(on)
    packs, real = [], nat.ssd7_pack_heads

    def recording(*args, **kw):
        packs.append(len(args[0]))
        return real(*args, **kw)

    monkeypatch.setattr(nat, "ssd7_pack_heads", recording)
    hooked = []
    hooks = [conv.register_forward_hook(lambda _m, _i, out: hooked.append(out)) for conv in list(on.conf_heads) + list(on.loc_heads)]
    pred = on(img)
    counts = _node_counts(pred)
    SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0).compute_loss(y_true, pred.float()).mean().backward()
    for h in hooks:
        h.remove()
    counts_parent = _node_counts(_step(parent, img, y_true))
    # four packed head nodes and one assembly node; the eight framework convolutions of the heads are gone, and with them the softmax
    # and the concatenations; the trunk is the parent's
    assert _count(counts, "_Ssd7HeadFn") == 4 and _count(counts, "_AssembleTrainFn") == 1
    assert _count(counts_parent, "_Ssd7HeadFn") == 0 and _count(counts_parent, "_AssembleTrainFn") == 0
    assert _count(counts_parent, "ConvolutionBackward") - _count(counts, "ConvolutionBackward") == 8
    assert _count(counts, "SoftmaxBackward") == 0 and _count(counts, "CatBackward") == 0 and _count(counts_parent, "SoftmaxBackward") == 1
    assert _count(counts, "_Ssd7ConvFn") == _count(counts_parent, "_Ssd7ConvFn") and _count(counts, "_BnEluPoolFn") == 7
    assert not hooked and packs == [4]                              # the nn.Conv2d heads are not called; ONE pack launch for the four maps
    assert pred.shape == (3, y_true.shape[1], y_true.shape[2]) and pred.dtype == torch.float32
    for heads in (on.conf_heads, on.loc_heads):
        assert all(p.grad is not None and p.grad.dtype == p.dtype and p.grad.stride() == p.stride() and bool(torch.isfinite(p.grad).all())
                   for conv in heads for p in conv.parameters())
    assert all(p.grad is not None for p in on.parameters())
    # independent of `convolutions`: without it the trunk keeps the framework's convolutions, the heads still take the route
    counts = _node_counts(_step(_head_model(3, convolutions=False), img, y_true))
    assert _count(counts, "_Ssd7HeadFn") == 4 and _count(counts, "_Ssd7ConvFn") == 0 and _count(counts, "ConvolutionBackward") == 7


def test_existing_switch_positions_are_untouched(deterministic_convolutions):  # noqa: F811
    """fused_blocks(True, training=True) and (..., convolutions=True) without the keyword are bit-identical -- predictions, gradients,
    running statistics -- to heads=False given explicitly, and to a model on which heads=True was switched off again."""
    import torch
    img = _images()
    new = lambda: _train_model(3, None)
    pairs = [(new().fused_blocks(True, training=True), new().fused_blocks(True, training=True, heads=False)),
             (new().fused_blocks(True, training=True, convolutions=True), new().fused_blocks(True, training=True, convolutions=True, heads=False)),
             (_head_model(3).fused_blocks(True, training=True, convolutions=True), _parent_model(3)),
             (_head_model(3).fused_blocks(False), new())]
    y_true = _y_true(pairs[0][0])
    for without, explicit in pairs:
        pa, pb = _step(without, img, y_true), _step(explicit, img, y_true)
        assert "_Ssd7HeadFn" not in _node_counts(pa)
        assert torch.equal(pa, pb) and _grads_equal(without, explicit) and _state_equal(without, explicit)


def test_not_farther_from_float32_than_the_parent_route():
    """Relative L2 distance of all parameter gradients and of the predictions from the float32 framework model with the same weights:
    the route with libssdhip heads may be at most 1.1 x that of the parent route (training=True, convolutions=True), measured here
    (the rule and margin of tests/test_ssd7_fused_training_gpu.py).  Both pairs are printed; DESIGN.md 4.4 records them."""
    img = _images()
    truth = _train_model(3, None, dtype=None)
    truth.fused_training = False
    y_true = _y_true(truth)
    want = _step(truth, img, y_true)
    parent, new = _parent_model(3), _head_model(3)
    g_p, p_p = _distance(parent, truth, _step(parent, img, y_true), want)
    g_n, p_n = _distance(new, truth, _step(new, img, y_true), want)
    print("relative L2 distance from float32: parent route gradients %.4g predictions %.4g; libssdhip heads gradients %.4g "
          "predictions %.4g" % (g_p, p_p, g_n, p_n))
    assert g_n <= 1.1 * g_p and p_n <= 1.1 * p_p


def test_second_step_uses_the_updated_weights_and_a_stale_backward_raises():
    """After one SGD.step() the second step's predictions equal those of a fresh model loaded with the post-step state: the packed images
    and biases were rebuilt from the updated parameters.  A backward that runs after an in-place change of a head's filters raises."""
    import torch
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    from ssd_keras_amd.optimizers import SGD
    img = _images()
    model = _head_model(3)
    y_true = _y_true(model)
    opt = SGD(model.parameters(), lr=1e-2, momentum=0.9)
    first = _step(model, img, y_true).detach().clone()
    opt.step()
    opt.zero_grad(set_to_none=True)
    state = copy.deepcopy(model.state_dict())
    second = _step(model, img, y_true)
    fresh = _head_model(4)
    fresh.load_state_dict(state)
    assert not torch.equal(second, first) and torch.equal(_step(fresh, img, y_true), second) and _grads_equal(fresh, model)
    pred = model(img)
    with torch.no_grad():
        model.loc_heads[1].weight.mul_(0.5)
    with pytest.raises(RuntimeError, match="changed in place"):
        SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0).compute_loss(y_true, pred.float()).mean().backward()


def test_three_captured_steps_equal_three_eager_steps(deterministic_convolutions):  # noqa: F811
    """forward + SSDLoss + backward + SGD(master_weights=True) captured as ONE torch.cuda.graph and replayed three times, against three
    eager steps: parameters, buffers and the optimizer's state bit for bit; and the capture itself runs nothing (the protocol of
    tests/test_master_weights_gpu.py's SSD7 step)."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    img = _images()
    eager, graphed = _head_model(3), _head_model(3)
    y_true = _y_true(eager)
    start = copy.deepcopy(graphed.state_dict())
    kw = dict(lr=1e-3, momentum=0.9, master_weights=True)

    def step(model, opt):
        opt.zero_grad(set_to_none=True)
        _step(model, img, y_true)
        opt.step()

    eager_opt = SGD(eager.parameters(), **kw)
    for _ in range(3):
        step(eager, eager_opt)
    opt = SGD(graphed.parameters(), **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(graphed, img, y_true)                                # warm-up without an optimizer step: the model's buffers, gradients in place
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.load_state_dict(start)                                 # (the running statistics moved)
    opt.init_state()                                               # masters from the restored weights, the buffers, the state block
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(graphed, opt)
    torch.cuda.synchronize()
    assert _state_equal(graphed, _head_model(3)) and opt.iterations == 0   # a capture runs nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert opt.iterations == 3 == eager_opt.iterations
    assert _state_equal(graphed, eager)
    for p, q in zip(graphed.parameters(), eager.parameters()):
        assert "master" in eager_opt.state[q]
        for k, want in eager_opt.state[q].items():
            assert torch.equal(opt.state[p][k], want), k


def test_uncovered_input_keeps_what_it_had(deterministic_convolutions):  # noqa: F811
    import torch
    from ssd_keras_amd.models.keras_ssd7 import build_model
    img = _images()
    # 20 classes: 4 x (21 + 4) = 100 packed channels > 48 -- the framework's heads, bit-equal to heads=False
    def wide(heads):
        torch.manual_seed(5)
        m = build_model(SIZE, 20, mode="training", normalize_coords=True, subtract_mean=127.5, divide_by_stddev=127.5)
        m = m.cuda().to(memory_format=torch.channels_last).to(torch.bfloat16).train()
        return m.fused_blocks(True, training=True, convolutions=True, heads=heads)
    a, b = wide(True), wide(False)
    y_true = _y_true(a)
    pa, pb = _step(a, img, y_true), _step(b, img, y_true)
    assert "_Ssd7HeadFn" not in _node_counts(pa) and _count(_node_counts(pa), "ConvolutionBackward") == _count(_node_counts(pb), "ConvolutionBackward")
    assert torch.equal(pa, pb) and _grads_equal(a, b) and _state_equal(a, b)
    # a float32 model
    a, b = _head_model(3, dtype=None), _parent_model(3, dtype=None)
    y_true = _y_true(a)
    pa = _step(a, img, y_true)
    assert "_Ssd7HeadFn" not in _node_counts(pa)
    assert torch.equal(pa, _step(b, img, y_true)) and _grads_equal(a, b) and _state_equal(a, b)
    # eval(): the inference blocks, whatever the training switches say
    with torch.no_grad():
        assert torch.equal(_head_model(3).eval()(img), _parent_model(3).eval()(img))
    # train() under no_grad: the parent's forward, and the same running statistics
    quiet, same = _head_model(3), _parent_model(3)
    with torch.no_grad():
        assert torch.equal(quiet(img), same(img))
    assert _state_equal(quiet, same)
