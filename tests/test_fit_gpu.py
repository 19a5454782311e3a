"""`ssd_keras_amd.training.fit_generator` on the 76 x 68 SSD7 test model of tests/test_ssd7_fused_training_gpu.py at batch 3, every
training route in libssdhip (`fused_blocks(True, training=True, convolutions=True, heads=True)`), SGD with float32 masters, fed by a
list of fixed batches: the captured loop against the eager one and against loops written out by hand, the reported loss against
tests/np_fit.py, validation, the learning-rate and NaN callbacks, and the checkpoint files."""
import itertools

import numpy as np
import pytest

from tests import np_fit
from tests.test_ssd7_conv_training_gpu import _node_counts
from tests.test_ssd7_fused_blocks_gpu import _images
from tests.test_ssd7_fused_training_gpu import (_state_equal, _train_model, _y_true,
                                                deterministic_convolutions)  # noqa: F401  (the last one is a fixture)

pytestmark = pytest.mark.gpu

L2 = 5e-4
KW = dict(lr=1e-3, momentum=0.9, master_weights=True)


def _model(l2=0.0, seed=3):
    model = _train_model(seed, None).fused_blocks(True, training=True, convolutions=True, heads=True)
    model.l2_regularization = l2
    return model


def _loss():
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    return SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0)


def _optimizer(model, **kw):
    from ssd_keras_amd.optimizers import SGD
    from ssd_keras_amd.training import regularized_param_groups
    return SGD(regularized_param_groups(model) if model.l2_regularization else model.parameters(), **dict(KW, **kw))


def _batches(model, n=3):
    return [(_images(seed=10 + k), _y_true(model, seed=20 + k)) for k in range(n)]


def _fit(batches, epochs=2, l2=0.0, graph=True, steps=None, **kw):
    from ssd_keras_amd.training import fit_generator
    model = _model(l2)
    opt = _optimizer(model)
    hist = fit_generator(model, itertools.cycle(batches), steps or len(batches), epochs, optimizer=opt, loss=_loss(), graph=graph, **kw)
    return model, opt, hist


def _optimizers_equal(a, model_a, b, model_b):
    import torch
    for p, q in zip(model_a.parameters(), model_b.parameters()):
        sa, sb = a.state[p], b.state[q]
        assert set(sa) == set(sb) and "master" in sa
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    return a.iterations == b.iterations


def _penalty_partials(model, opt):
    """The partials of the sum-of-squares launch from the host: every conv kernel in memory order, its master where there is one."""
    import torch
    srcs = []
    for m in model.modules():
        if isinstance(m, torch.nn.Conv2d):
            w = m.weight
            st = opt.state[w] if w in opt.state else {}
            t = st["master"] if "master" in st else w.detach().to(torch.float32, memory_format=torch.preserve_format)
            srcs.append(t.detach().as_strided((t.numel(),), (1,)).cpu().numpy())
    return np_fit.sumsq_kernel_order(srcs, 4)


def _by_hand(batches, epochs, l2=0.0, set_lr=None):
    """The loop written out: per step zero_grad, forward, loss, backward, step.  Returns (model, optimizer, [loss per epoch by
    np_fit.Meter from the per-step loss vectors and, with l2, the kernels' squares])."""
    model = _model(l2)
    opt, lf = _optimizer(model), _loss()
    losses = []
    for epoch in range(epochs):
        if set_lr is not None:
            set_lr(opt, epoch)
        meter = np_fit.Meter()
        for img, y in batches:
            opt.zero_grad(set_to_none=True)
            per = lf.compute_loss(y, model(img).float())
            per.mean().backward()
            meter.update(per.detach().cpu().numpy(), _penalty_partials(model, opt) if l2 else (), l2)
            opt.step()
        losses.append(meter.mean)
    return model, opt, losses


def test_captured_loop_equals_the_eager_loop_and_the_loop_by_hand(deterministic_convolutions):  # noqa: F811
    batches = _batches(_model())
    g_model, g_opt, g_hist = _fit(batches, graph=True)
    e_model, e_opt, e_hist = _fit(batches, graph=False)
    assert g_opt.iterations == 6 == e_opt.iterations
    assert _state_equal(g_model, e_model) and _optimizers_equal(g_opt, g_model, e_opt, e_model)
    assert g_hist.epoch == e_hist.epoch == [0, 1] and g_hist.history == e_hist.history and list(g_hist.history) == ["loss"]
    assert all(int(bn.num_batches_tracked) == 6 for bn in g_model.bns)
    # the reported loss is the NumPy statement of the meter, fed the per-step loss vectors of an independent loop
    h_model, h_opt, losses = _by_hand(batches, 2)
    print("loss per epoch: fit_generator %r, by hand %r" % (g_hist.history["loss"], losses))
    assert g_hist.history["loss"] == losses and all(np.isfinite(losses)) and losses[1] != losses[0]
    assert _state_equal(g_model, h_model) and _optimizers_equal(g_opt, g_model, h_opt, h_model)


def test_penalty_is_in_the_loss_and_costs_the_two_launches(deterministic_convolutions):  # noqa: F811
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from ssd_keras_amd import training as T
    from ssd_keras_amd.optimizers import SGD
    batches = _batches(_model())
    model, opt, hist = _fit(batches, epochs=2, l2=L2)
    assert [g["weight_decay"] for g in opt.param_groups] == [2 * L2, 0.0]
    h_model, h_opt, losses = _by_hand(batches, 2, l2=L2)
    plain = _by_hand(batches, 1)[2]
    print("loss per epoch with l2: fit_generator %r, by hand %r; without: %r" % (hist.history["loss"], losses, plain))
    assert hist.history["loss"] == losses and losses[0] > plain[0]
    assert _state_equal(model, h_model) and _optimizers_equal(opt, model, h_opt, h_model)

    # the step with the penalty dispatches exactly the framework operations of the step without it, and its autograd graph has the
    # same nodes: what it adds is one sum-of-squares launch (every kernel is a float32 master: one table) in front of the meter's
    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = {}

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops[str(func)] = self.ops.get(str(func), 0) + 1
            return func(*args, **(kwargs or {}))

    seen = {}
    for l2 in (0.0, L2):
        m = _model(l2)
        o, lf = SGD(T.regularized_param_groups(m), **KW), _loss()   # (two groups either way: weight_decay 2 l2, or 0)
        loop = T._Loop(m, o, lf, graph=False)
        with torch.cuda.stream(loop.stream):
            loop.train_meter.reset()
            loop.run("train", batches[0])                          # (the warm-up, the optimizer's state, the tables)
            with Count() as count:
                loop.run("train", batches[1])
            nodes = _node_counts(lf.compute_loss(batches[0][1], m(batches[0][0]).float()))
            torch.cuda.synchronize()
        seen[l2] = (count.ops, dict(loop.launches), nodes, loop.train_meter.read()["steps"])
    assert seen[0.0][1] == {"sumsq": 0, "meter": 1} and seen[L2][1] == {"sumsq": 1, "meter": 1}
    assert seen[0.0][0] == seen[L2][0] and seen[0.0][2] == seen[L2][2] and seen[0.0][3] == seen[L2][3] == 2
    assert seen[L2][0] and not any("pow" in k for k in seen[L2][0]), sorted(seen[L2][0])


def test_short_last_batch_gets_its_own_capture_and_a_third_shape_runs_eagerly(deterministic_convolutions, monkeypatch):  # noqa: F811
    import torch
    from ssd_keras_amd import training as T
    full = _batches(_model(), 2)
    short = (full[0][0][:2].clone(), full[1][1][:2].clone())
    wide = (torch.cat([full[1][0], full[0][0][:1]]), torch.cat([full[0][1], full[1][1][:1]]))
    batches = [full[0], full[1], short, wide]                      # 3, 3, 2, 4 samples
    captured, real = [], T._Loop._capture

    def recording(self, kind, images, y_true):
        captured.append((kind, int(images.shape[0])))
        return real(self, kind, images, y_true)

    monkeypatch.setattr(T._Loop, "_capture", recording)
    model, opt, hist = _fit(batches, epochs=2)
    assert captured == [("train", 3), ("train", 2)] and opt.iterations == 8
    h_model, h_opt, losses = _by_hand(batches, 2)
    assert hist.history["loss"] == losses                           # the mean weighted by 3, 3, 2, 4
    assert _state_equal(model, h_model) and _optimizers_equal(opt, model, h_opt, h_model)


def test_validation(deterministic_convolutions):  # noqa: F811
    import torch
    train = _batches(_model())
    val = [(_images(seed=40 + k), _y_true(_model(), seed=50 + k)) for k in range(2)]
    kw = dict(validation_data=itertools.cycle(val), validation_steps=2)
    model, opt, hist = _fit(train, epochs=2, l2=L2, **kw)
    assert model.training and list(hist.history) == ["loss", "val_loss"]
    # the eager loop reports the same numbers: in its second epoch the captured evaluation read tables rebuilt from the new weights
    e_model, e_opt, e_hist = _fit(train, epochs=2, l2=L2, graph=False, validation_data=itertools.cycle(val), validation_steps=2)
    assert hist.history == e_hist.history and hist.history["val_loss"][0] != hist.history["val_loss"][1]
    # training is what it is without validation: running statistics and num_batches_tracked untouched
    n_model, n_opt, n_hist = _fit(train, epochs=2, l2=L2)
    assert _state_equal(model, n_model) and _optimizers_equal(opt, model, n_opt, n_model) and n_hist.history["loss"] == hist.history["loss"]
    # the last epoch's val_loss by hand: eval mode, no_grad, on the trained model, penalty from the masters
    meter, lf = np_fit.Meter(), _loss()
    model.eval()
    with torch.no_grad():
        for img, y in val:
            meter.update(lf.compute_loss(y, model(img).float()).cpu().numpy(), _penalty_partials(model, opt), L2)
    model.train()
    print("val_loss %r, by hand %r" % (hist.history["val_loss"], meter.mean))
    assert hist.history["val_loss"][1] == meter.mean


def test_learning_rate_scheduler_between_replays(deterministic_convolutions):  # noqa: F811
    from ssd_keras_amd.training import LearningRateScheduler
    batches = _batches(_model())
    schedule = lambda epoch, lr: lr * 0.5 if epoch == 1 else lr
    model, opt, hist = _fit(batches, epochs=2, callbacks=[LearningRateScheduler(schedule)])
    h_model, h_opt, losses = _by_hand(batches, 2, set_lr=lambda o, epoch: o.set_lr(schedule(epoch, o.param_groups[0]["lr"])))
    assert opt.param_groups[0]["lr"] == KW["lr"] * 0.5 == h_opt.param_groups[0]["lr"]
    assert _state_equal(model, h_model) and _optimizers_equal(opt, model, h_opt, h_model) and hist.history["loss"] == losses
    same_rate = _by_hand(batches, 2)[0]
    assert not _state_equal(model, same_rate)                       # (the halved rate changed the second epoch)


def test_terminate_on_nan(capsys):
    import torch
    from ssd_keras_amd.training import TerminateOnNaN
    batches = _batches(_model(), 6)
    poisoned = batches[2][0].clone()
    poisoned[1, 5, 7, 0] = float("nan")
    labels = batches[2][1].clone()
    positive = int((labels[0, :, 0] == 0).nonzero()[0])
    labels[0, positive, labels.shape[2] - 12] = float("nan")        # ... and the first box offset of a positive anchor
    batches[2] = (poisoned, labels)
    nan_poll = 2
    model, opt, hist = _fit(batches, epochs=3, callbacks=[TerminateOnNaN()], nan_poll=nan_poll)
    out = capsys.readouterr().out
    assert "Batch 2: Invalid loss, terminating training" in out and out.count("Invalid loss") == 1
    assert model.stop_training
    taken = opt.iterations
    assert 3 <= taken <= 3 + nan_poll - 1                           # the bad step, and at most nan_poll - 1 further ones
    assert hist.epoch == [0] and list(hist.history) == ["loss"] and len(hist.history["loss"]) == 1
    assert not np.isfinite(hist.history["loss"][0])                 # Keras's aborted epoch: its logs hold the non-finite mean


def test_model_checkpoint_files(tmp_path):
    import torch
    from ssd_keras_amd.models.keras_weights import load_keras_weights
    from ssd_keras_amd.training import ModelCheckpoint
    batches = _batches(_model())
    pattern = str(tmp_path / "ssd7_epoch-{epoch:02d}_loss-{loss:.4f}.h5")
    model, opt, hist = _fit(batches, epochs=1, l2=L2, callbacks=[ModelCheckpoint(pattern, monitor="loss", save_best_only=True)])
    path = str(tmp_path / ("ssd7_epoch-01_loss-%.4f.h5" % hist.history["loss"][0]))
    fresh = _model(L2, seed=4)
    load_keras_weights(fresh, path)
    for (name, want), got in zip(model.state_dict().items(), fresh.state_dict().values()):
        if name.endswith("num_batches_tracked"):
            continue                                               # (not a Keras weight)
        assert torch.equal(got, want.float().to(got.dtype)), name   # float32 in the file, back to the model's dtype
    # the optimizer beside it: a restored optimizer's next step is the original's next step
    fresh.load_state_dict(model.state_dict())
    restored = _optimizer(fresh)
    restored.load_state_dict(torch.load(path + ".optim.pt"))
    assert restored.iterations == 3
    lf = _loss()
    img, y = batches[0]
    for m, o in ((model, opt), (fresh, restored)):
        o.zero_grad(set_to_none=True)
        lf.compute_loss(y, m(img).float()).mean().backward()
        o.step()
    assert _state_equal(model, fresh) and _optimizers_equal(opt, model, restored, fresh) and restored.iterations == 4
