"""`SSD7.fused_blocks(True, training=True, convolutions=True)` (models/keras_ssd7.py, models/_train_fns.py: _Ssd7ConvFn): the training
step whose seven trunk convolutions run in libssdhip too, on the 76 x 68 test model of tests/test_ssd7_fused_blocks_gpu.py at batch 3
(maps 76 x 68 -> 38 x 34 -> 19 x 17 -> 9 x 8 -> 4 x 4 -> 2 x 2 -> 1 x 1).  The kernels' arithmetic is
tests/test_ssd7_conv_kernels_gpu.py's."""
import copy

import numpy as np
import pytest

from tests import np_bn_elu as ref
from tests.test_ssd7_fused_blocks_gpu import _images
from tests.test_ssd7_fused_training_gpu import (_distance, _grads_equal, _state_equal, _step, _train_model, _y_true,
                                                deterministic_convolutions)  # noqa: F401  (the last one is a fixture)

pytestmark = pytest.mark.gpu


def _conv_model(seed, dtype="bfloat16"):
    """All seven layers routed, whatever set the measurements of DESIGN.md 4.4 leave in SSD7.TRAIN_CONVS: the mechanism is under test."""
    model = _train_model(seed, None, dtype=dtype).fused_blocks(True, training=True, convolutions=True)
    model.TRAIN_CONVS = frozenset(range(7))
    return model


def _node_counts(t):
    seen, todo, counts = set(), [t.grad_fn], {}
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        name = type(fn).__name__
        counts[name] = counts.get(name, 0) + 1
        todo.extend(f for f, _ in fn.next_functions)
    return counts


def _count(counts, part):
    return sum(n for name, n in counts.items() if part in name)


def test_routing(deterministic_convolutions, monkeypatch):  # noqa: F811
    import torch
    from ssd_keras_amd import _native as nat
    img = _images()
    on, blocks_only = _conv_model(3), _train_model(3, True)
    y_true = _y_true(on)
    before = [(bn.running_mean.double().cpu().numpy(), bn.running_var.double().cpu().numpy()) for bn in on.bns]
    seen, real = [], nat.ssd7_conv_bias

    def recording(*args, **kw):
        y = real(*args, **kw)
        seen.append(y.detach())
        return y

    monkeypatch.setattr(nat, "ssd7_conv_bias", recording)
    hooked = []
    hooks = [conv.register_forward_hook(lambda _m, _i, out: hooked.append(out)) for conv in on.convs]
    pred_on = on(img)
    counts_on = _node_counts(pred_on)
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0).compute_loss(y_true, pred_on.float()).mean().backward()
    for h in hooks:
        h.remove()
    monkeypatch.setattr(nat, "ssd7_conv_bias", real)
    pred_blocks = _step(blocks_only, img, y_true)
    counts_blocks = _node_counts(pred_blocks)
    # seven _Ssd7ConvFn nodes, seven framework convolutions fewer: only the eight predictor heads' remain
    assert _count(counts_on, "_Ssd7ConvFn") == 7 and _count(counts_blocks, "_Ssd7ConvFn") == 0
    assert _count(counts_blocks, "ConvolutionBackward") - _count(counts_on, "ConvolutionBackward") == 7
    assert _count(counts_on, "ConvolutionBackward") == 8 and _count(counts_on, "_BnEluPoolFn") == _count(counts_blocks, "_BnEluPoolFn")
    assert not hooked                                               # the nn.Conv2d modules are not called on this route
    assert pred_on.shape == pred_blocks.shape and all(p.grad is not None and p.grad.dtype == p.dtype and p.grad.stride() == p.stride()
                                                      for conv in on.convs for p in conv.parameters())
    # running statistics: nn.BatchNorm2d's update from the batch statistics of the maps the convolution launches wrote (seven forward
    # calls, then six data gradients), within one bf16 step as under training=True alone; num_batches_tracked is 1
    assert len(seen) == 13
    for bn, y, (rm, rv) in zip(on.bns, seen[:7], before):
        mean, _, var_u = ref.batch_stats(y.double().permute(0, 2, 3, 1).cpu().numpy())
        want_m, want_v = ref.running_update(rm, mean, bn.momentum), ref.running_update(rv, var_u, bn.momentum)
        assert np.all(np.abs(bn.running_mean.double().cpu().numpy() - want_m) <= ref.bf16_step(want_m))
        assert np.all(np.abs(bn.running_var.double().cpu().numpy() - want_v) <= ref.bf16_step(want_v))
        assert int(bn.num_batches_tracked) == 1


def test_existing_switch_positions_are_untouched(deterministic_convolutions):  # noqa: F811
    """fused_blocks(True, training=True) and fused_blocks(False) after convolutions=True are bit-identical -- predictions, gradients,
    state -- to models that never heard of the keyword."""
    import torch
    img = _images()
    pairs = [(_conv_model(3).fused_blocks(True, training=True), _train_model(3, True)),
             (_conv_model(3).fused_blocks(False), _train_model(3, None))]
    y_true = _y_true(pairs[0][0])
    for was_on, never in pairs:
        pa, pb = _step(was_on, img, y_true), _step(never, img, y_true)
        assert torch.equal(pa, pb) and _grads_equal(was_on, never) and _state_equal(was_on, never)


def test_not_farther_from_float32_than_the_default_bf16_path():
    """Relative L2 distance of all parameter gradients and of the predictions from the float32 framework model with the same weights:
    the route with libssdhip convolutions may be at most 1.1 x the default bf16 path's (the rule and margin of
    tests/test_ssd7_fused_training_gpu.py).  Both pairs are printed; DESIGN.md 4.4, "SSD7 training", records them."""
    img = _images()
    truth = _train_model(3, None, dtype=None)
    truth.fused_training = False
    y_true = _y_true(truth)
    want = _step(truth, img, y_true)
    default, new = _train_model(3, None), _conv_model(3)
    g_d, p_d = _distance(default, truth, _step(default, img, y_true), want)
    g_n, p_n = _distance(new, truth, _step(new, img, y_true), want)
    print("relative L2 distance from float32: default bf16 path gradients %.4g predictions %.4g; libssdhip convolutions gradients %.4g "
          "predictions %.4g" % (g_d, p_d, g_n, p_n))
    assert g_n <= 1.1 * g_d and p_n <= 1.1 * p_d


def test_second_step_uses_the_updated_weights():
    """After one SGD.step() the second step's predictions equal those of a fresh model loaded with the post-step state: the filter images
    were rebuilt from the updated parameters."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    img = _images()
    model = _conv_model(3)
    y_true = _y_true(model)
    opt = SGD(model.parameters(), lr=1e-2, momentum=0.9)
    first = _step(model, img, y_true).detach().clone()
    opt.step()
    opt.zero_grad(set_to_none=True)
    state = copy.deepcopy(model.state_dict())
    second = _step(model, img, y_true)
    fresh = _conv_model(4)
    fresh.load_state_dict(state)
    assert not torch.equal(second, first) and torch.equal(_step(fresh, img, y_true), second)


def test_three_captured_steps_equal_three_eager_steps(deterministic_convolutions):  # noqa: F811
    import torch
    from ssd_keras_amd.optimizers import SGD
    img = _images()
    eager, graphed = _conv_model(3), _conv_model(3)
    y_true = _y_true(eager)
    start = copy.deepcopy(graphed.state_dict())
    kw = dict(lr=1e-3, momentum=0.9)

    def steps(model, opt, n):
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            _step(model, img, y_true)
            opt.step()

    steps(eager, SGD(eager.parameters(), **kw), 3)
    opt = SGD(graphed.parameters(), **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        steps(graphed, opt, 1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.load_state_dict(start)
    for st in opt.state.values():
        for v in (st.values() if isinstance(st, dict) else ()):
            if torch.is_tensor(v):
                v.zero_()
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps(graphed, opt, 3)
    torch.cuda.synchronize()
    assert _state_equal(graphed, _conv_model(3))                 # a capture runs nothing
    graph.replay()
    torch.cuda.synchronize()
    assert _state_equal(graphed, eager)


def _captured_equals_eager(make, n_steps=3):
    """`n_steps` captured steps of forward + SSDLoss + backward + SGD replayed once against the same steps run eagerly: state bit for bit,
    and the capture itself runs nothing."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    img = _images()
    eager, graphed = make(), make()
    y_true = _y_true(eager)
    start = copy.deepcopy(graphed.state_dict())
    kw = dict(lr=1e-3, momentum=0.9)

    def steps(model, opt, n):
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            _step(model, img, y_true)
            opt.step()

    steps(eager, SGD(eager.parameters(), **kw), n_steps)
    opt = SGD(graphed.parameters(), **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        steps(graphed, opt, 1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.load_state_dict(start)
    for st in opt.state.values():
        for v in (st.values() if isinstance(st, dict) else ()):
            if torch.is_tensor(v):
                v.zero_()
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps(graphed, opt, n_steps)
    torch.cuda.synchronize()
    assert _state_equal(graphed, make())
    graph.replay()
    torch.cuda.synchronize()
    assert _state_equal(graphed, eager)


def test_the_shipped_layer_set(deterministic_convolutions):  # noqa: F811
    """The class's own TRAIN_CONVS, untouched (layers 1-3 as shipped): its layers run `_Ssd7ConvFn`, the others the framework's
    convolution on the outputs of `_BnEluPoolFn`, in one step.  One node more and one framework convolution fewer per routed layer
    (15 = 7 trunk + 8 heads without the route: 3 nodes and 12 with the shipped set); the routed layers' maps equal the all-layers
    model's bit for bit; captured steps equal eager ones."""
    import torch
    from ssd_keras_amd.models.keras_ssd7 import SSD7
    shipped = lambda: _train_model(3, None).fused_blocks(True, training=True, convolutions=True)
    model = shipped()
    assert "TRAIN_CONVS" not in model.__dict__ and model.TRAIN_CONVS is SSD7.TRAIN_CONVS and SSD7.TRAIN_CONVS <= frozenset(range(7))
    n = len(SSD7.TRAIN_CONVS)
    img = _images()
    y_true = _y_true(model)
    pred = _step(model, img, y_true)
    counts = _node_counts(pred)
    assert _count(counts, "_Ssd7ConvFn") == n and _count(counts, "ConvolutionBackward") == 15 - n
    assert _count(counts, "_BnEluPoolFn") == 7 and all(int(bn.num_batches_tracked) == 1 for bn in model.bns)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    # the mix computes what its parts compute: a routed layer's node equals the all-layers model's node on the same input, so the
    # maps of the leading routed layers are bit-equal between the two models
    if SSD7.TRAIN_CONVS == frozenset(range(n)) and n:
        from ssd_keras_amd import _native as nat
        seen = {}
        real = nat.ssd7_conv_bias
        for name, m in (("shipped", shipped()), ("all", _conv_model(3))):
            outs = seen.setdefault(name, [])

            def recording(*args, _outs=outs, **kw):
                y = real(*args, **kw)
                _outs.append(y.detach().clone())
                return y

            nat.ssd7_conv_bias = recording
            try:
                with torch.no_grad():
                    m(img)
            finally:
                nat.ssd7_conv_bias = real
        assert len(seen["shipped"]) == n and len(seen["all"]) == 7
        assert all(torch.equal(a, b) for a, b in zip(seen["shipped"], seen["all"]))
    _captured_equals_eager(shipped)


def test_uncovered_input_keeps_what_it_had(deterministic_convolutions):  # noqa: F811
    import torch
    img = _images()
    # a float32 model: the framework's chain, as under training=True alone
    a, b = _conv_model(3, dtype=None), _train_model(3, True, dtype=None)
    y_true = _y_true(a)
    assert torch.equal(_step(a, img, y_true), _step(b, img, y_true)) and _grads_equal(a, b) and _state_equal(a, b)
    # eval(): the inference blocks, whatever the training switches say
    with torch.no_grad():
        assert torch.equal(_conv_model(3).eval()(img), _train_model(3, True).eval()(img))
    # train() under no_grad: the forward launches run and move the running statistics as a step under grad does
    quiet, loud = _conv_model(3), _conv_model(3)
    with torch.no_grad():
        quiet(img)
    _step(loud, img, y_true)
    assert _state_equal(quiet, loud)
    # batch 1: block 7's map is one value per channel -- the default chain runs and raises what the framework raises
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        _conv_model(3)(img[:1])
