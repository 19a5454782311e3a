"""`SSD7.fused_blocks(training=True)` (models/keras_ssd7.py, models/_train_fns.py: _BnEluPoolFn): the training step's route around
csrc/ssdhip_bntrain.hip on the small model of tests/test_ssd7_fused_blocks_gpu.py (76 x 68 x 3, batch 3: maps 76 x 68 -> 38 x 34 ->
19 x 17 -> 9 x 8 -> 4 x 4 -> 2 x 2 -> 1 x 1, odd sizes in front of the pools).  The kernels' arithmetic is tests/test_bn_elu_train_gpu.py's."""
import copy

import numpy as np
import pytest

from tests import np_bn_elu as ref
from tests.test_ssd7_fused_blocks_gpu import BATCH, _images, _model

pytestmark = pytest.mark.gpu


def _train_model(seed, training, dtype="bfloat16"):
    import torch
    model = _model(seed, getattr(torch, dtype) if dtype else None)
    if training is not None:
        model.fused_blocks(True, training=training)
    return model.train()


def _y_true(model, seed=9):
    """A fixed encoded batch: every anchor background except one in sixteen, which carries a class and box offsets."""
    import torch
    n = int(sum(h * w * pb.n_boxes for (h, w), pb in zip(model.predictor_sizes(), model.priorboxes)))
    rng = np.random.RandomState(seed)
    y = np.zeros((BATCH, n, model.n_classes + 12), dtype=np.float32)
    pos = rng.rand(BATCH, n) < 1.0 / 16
    cls = rng.randint(1, model.n_classes, size=(BATCH, n))
    y[..., 0] = ~pos
    for k in range(1, model.n_classes):
        y[..., k] = pos & (cls == k)
    y[..., model.n_classes:model.n_classes + 4] = rng.randn(BATCH, n, 4) * 0.5 * pos[..., None]
    return torch.from_numpy(y).cuda()


def _step(model, img, y_true):
    """forward + SSDLoss + backward; returns the predictions."""
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    pred = model(img)
    SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0).compute_loss(y_true, pred.float()).mean().backward()
    return pred


def _node_names(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


def _state_equal(a, b):
    import torch
    sa, sb = a.state_dict(), b.state_dict()
    return list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def _grads_equal(a, b):
    import torch
    bad = [n for (n, p), q in zip(a.named_parameters(), b.parameters())
           if (p.grad is None) != (q.grad is None) or (p.grad is not None and not torch.equal(p.grad, q.grad))]
    if bad:
        print("gradients differ:", bad)
    return not bad


@pytest.fixture
def deterministic_convolutions():
    """The framework's convolution backward may pick an algorithm that adds in arrival order; bit-for-bit comparisons of gradients
    between two models need the deterministic ones."""
    import torch
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was


def test_routing(deterministic_convolutions):
    import torch
    img = _images()
    untouched, off, back, on = (_train_model(3, None), _train_model(3, False), _train_model(3, True).fused_blocks(False),
                                _train_model(3, True))
    y_true = _y_true(on)
    preds = [_step(m, img, y_true) for m in (untouched, off, back, on)]
    assert any("_BnEluPoolFn" in n for n in _node_names(preds[3]))
    assert not any("_BnEluPoolFn" in n for n in _node_names(preds[0]) | _node_names(preds[1]) | _node_names(preds[2]))
    assert preds[3].shape == preds[0].shape and not torch.equal(preds[3], preds[0])        # another path ran
    for m, p in ((off, preds[1]), (back, preds[2])):
        assert torch.equal(p, preds[0]) and _grads_equal(m, untouched) and _state_equal(m, untouched)
    assert all(int(bn.num_batches_tracked) == 1 for bn in on.bns)
    # eval(): the switch's training half changes nothing
    with torch.no_grad():
        plain = _model(3, torch.bfloat16).fused_blocks()(img)
        assert torch.equal(_model(3, torch.bfloat16).fused_blocks(True, training=True)(img), plain)
    # train() under no_grad: the forward launches run and move the running statistics exactly as a step under grad does (the
    # predictions are not compared: without autograd the predictor heads take the inference kernels)
    quiet, plain = _train_model(3, True), _train_model(3, None)
    with torch.no_grad():
        assert not torch.equal(quiet(img), plain(img))
    assert _state_equal(quiet, on) and not _state_equal(quiet, plain)


def test_running_statistics_after_one_step():
    import torch
    model = _train_model(3, True)
    before = [(bn.running_mean.double().cpu().numpy(), bn.running_var.double().cpu().numpy()) for bn in model.bns]
    seen = []
    hooks = [conv.register_forward_hook(lambda _m, _i, out: seen.append(out.detach())) for conv in model.convs]
    _step(model, _images(), _y_true(model))
    for h in hooks:
        h.remove()
    assert len(seen) == 7
    for bn, y, (rm, rv) in zip(model.bns, seen, before):
        mean, _, var_u = ref.batch_stats(y.double().permute(0, 2, 3, 1).cpu().numpy())
        want_m, want_v = ref.running_update(rm, mean, bn.momentum), ref.running_update(rv, var_u, bn.momentum)
        assert np.all(np.abs(bn.running_mean.double().cpu().numpy() - want_m) <= ref.bf16_step(want_m))
        assert np.all(np.abs(bn.running_var.double().cpu().numpy() - want_v) <= ref.bf16_step(want_v))
        assert int(bn.num_batches_tracked) == 1


def _distance(model, truth, pred, pred_truth):
    num = sum(float((p.grad.double() - q.grad.double()).pow(2).sum()) for p, q in zip(model.parameters(), truth.parameters()))
    den = sum(float(q.grad.double().pow(2).sum()) for q in truth.parameters())
    c = pred.shape[2] - 8
    pred, pred_truth = pred.detach(), pred_truth.detach()
    dp = float((pred[..., :c].double() - pred_truth[..., :c].double()).norm() / pred_truth[..., :c].double().norm())
    return (num / den) ** 0.5, dp


def test_not_farther_from_float32_than_the_default_bf16_path():
    """Relative L2 distance of all parameter gradients and of the predictions from the float32 framework model with the same weights:
    the new path's may be at most 1.1 x the default bf16 path's (the margin: the two may route a tied window differently).
    Both pairs of distances are printed; DESIGN.md 4.4, "SSD7 training", records them."""
    img = _images()
    truth = _train_model(3, None, dtype=None)
    truth.fused_training = False                  # SSDModel's switch for libssdhip convolution forwards under autograd: the truth is the framework's
    y_true = _y_true(truth)
    want = _step(truth, img, y_true)
    default, new = _train_model(3, None), _train_model(3, True)
    g_d, p_d = _distance(default, truth, _step(default, img, y_true), want)
    g_n, p_n = _distance(new, truth, _step(new, img, y_true), want)
    print("relative L2 distance from float32: default bf16 path gradients %.4g predictions %.4g; fused training path gradients %.4g "
          "predictions %.4g" % (g_d, p_d, g_n, p_n))
    assert g_n <= 1.1 * g_d and p_n <= 1.1 * p_d


def test_three_captured_steps_equal_three_eager_steps(deterministic_convolutions):
    import torch
    from ssd_keras_amd.optimizers import SGD
    img = _images()
    eager, graphed = _train_model(3, True), _train_model(3, True)
    y_true = _y_true(eager)
    start = copy.deepcopy(graphed.state_dict())
    kw = dict(lr=1e-3, momentum=0.9)

    def steps(model, opt, n):
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            _step(model, img, y_true)
            opt.step()

    steps(eager, SGD(eager.parameters(), **kw), 3)
    # warm up on a side stream (kernel choices, the optimizer's buffers), then put everything back to the start
    opt = SGD(graphed.parameters(), **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        steps(graphed, opt, 1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.load_state_dict(start)
    for st in opt.state.values():                                # the momentum buffers the warm-up step created: back to zero, in place
        for v in (st.values() if isinstance(st, dict) else ()):
            if torch.is_tensor(v):
                v.zero_()
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps(graphed, opt, 3)
    torch.cuda.synchronize()
    assert _state_equal(graphed, _train_model(3, True))          # a capture runs nothing
    graph.replay()
    torch.cuda.synchronize()
    assert _state_equal(graphed, eager)


def test_state_changes_and_uncovered_blocks(deterministic_convolutions):
    import torch
    img = _images()
    a, b = _train_model(3, True), _train_model(3, True)
    y_true = _y_true(a)
    _step(a, img, y_true)
    a.load_state_dict(_model(4, torch.bfloat16).state_dict())
    b.load_state_dict(_model(4, torch.bfloat16).state_dict())
    a.zero_grad(set_to_none=True)
    pa, pb = _step(a, img, y_true), _step(b, img, y_true)
    assert torch.equal(pa, pb) and _grads_equal(a, b) and _state_equal(a, b)      # the next step used the loaded gamma / beta / buffers
    # batch 1: block 7's map is one value per channel -- the default chain runs and raises what the framework raises
    single = _train_model(3, True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        single(img[:1])
