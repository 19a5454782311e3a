"""The callbacks of ssd_keras_amd/training.py against Keras 2.2.4's state machines (keras/callbacks.py), driven with hand-written log
sequences on a stub model and optimizer: no GPU, no training."""
import warnings

import numpy as np
import pytest

from ssd_keras_amd import training as T


class _Optimizer:
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]
        self.set = []

    def set_lr(self, lr, group=None):
        self.set.append(lr)
        for g in self.param_groups:
            g["lr"] = lr

    def state_dict(self):
        return {"state": {}, "param_groups": self.param_groups}


class _Model:
    stop_training = False


def _wire(cb, lr=1e-3):
    model, opt = _Model(), _Optimizer(lr)
    cb.set_model(model)
    cb.set_optimizer(opt)
    cb.on_train_begin({})
    return model, opt


def _drive(cb, values, monitor="val_loss", begin=False):
    """on_epoch_end with {monitor: v} per epoch; returns the logs of every epoch."""
    out = []
    for epoch, v in enumerate(values):
        if begin:
            cb.on_epoch_begin(epoch, {})
        logs = {monitor: v}
        cb.on_epoch_end(epoch, logs)
        out.append(logs)
    return out


def test_reduce_lr_on_plateau_with_the_ssd7_notebooks_arguments():
    with pytest.warns(UserWarning, match="epsilon"):
        cb = T.ReduceLROnPlateau(monitor="val_loss", factor=0.2, patience=8, verbose=1, epsilon=0.001, cooldown=0, min_lr=0.00001)
    assert cb.min_delta == 0.001
    model, opt = _wire(cb, lr=1e-3)
    # epoch 0 sets best; epochs 1 .. 9 are a plateau (no improvement by more than 0.001): wait reaches 8 at epoch 8, ONE reduction
    logs = _drive(cb, [2.0] + [2.0 - 0.0005] * 9)
    assert [l["lr"] for l in logs] == [1e-3] * 9 + [1e-3 * 0.2]      # logs['lr'] is set first: the new rate shows one epoch later
    assert opt.set == [1e-3 * 0.2] and cb.wait == 1 and cb.best == 2.0
    # never below min_lr, and no call once it is there
    cb2 = T.ReduceLROnPlateau(factor=0.2, patience=1, min_delta=0.001, min_lr=1e-5)
    model, opt = _wire(cb2, lr=3e-5)
    _drive(cb2, [1.0, 1.0, 1.0, 1.0])
    assert opt.set == [1e-5] and opt.param_groups[0]["lr"] == 1e-5
    with pytest.raises(ValueError):
        T.ReduceLROnPlateau(factor=1.0)


def test_reduce_lr_on_plateau_cooldown():
    cb = T.ReduceLROnPlateau(factor=0.5, patience=2, min_delta=0.0, cooldown=2, min_lr=0)
    model, opt = _wire(cb, lr=1.0)
    # epoch: 0 best | 1 wait 1 | 2 wait 2 -> reduce, cooldown 2 | 3 counter 1, in cooldown | 4 counter 0, wait 1 | 5 wait 2 -> reduce
    waits, cools = [], []
    for epoch in range(6):
        cb.on_epoch_end(epoch, {"val_loss": 1.0})
        waits.append(cb.wait)
        cools.append(cb.cooldown_counter)
    assert waits == [0, 1, 0, 0, 1, 0] and cools == [0, 0, 2, 1, 0, 2]
    assert opt.set == [0.5, 0.25]
    # an improvement resets wait
    cb.on_epoch_end(6, {"val_loss": 0.5})
    assert cb.best == 0.5 and cb.wait == 0
    # a missing monitor warns and changes nothing but logs['lr']
    logs = {}
    with pytest.warns(RuntimeWarning):
        cb.on_epoch_end(7, logs)
    assert logs == {"lr": 0.25}


def test_early_stopping_patience_0_and_2():
    cb = T.EarlyStopping(monitor="val_loss", min_delta=0, patience=0)
    model, _ = _wire(cb)
    cb.on_epoch_end(0, {"val_loss": 1.0})
    assert not model.stop_training
    cb.on_epoch_end(1, {"val_loss": 1.0})                          # not strictly better: stops at once
    assert model.stop_training and cb.stopped_epoch == 1
    cb = T.EarlyStopping(monitor="val_loss", min_delta=0.1, patience=2)
    model, _ = _wire(cb)
    stops = []
    for epoch, v in enumerate([1.0, 0.95, 0.85, 0.8, 0.78]):        # 0.95: within min_delta; 0.85: 0.85 + 0.1 < 1.0, improves
        cb.on_epoch_end(epoch, {"val_loss": v})
        stops.append((cb.wait, model.stop_training))
    assert stops == [(0, False), (1, False), (0, False), (1, False), (2, True)] and cb.stopped_epoch == 4 and cb.best == 0.85
    with pytest.warns(RuntimeWarning):
        cb.on_epoch_end(5, {"loss": 1.0})
    cb = T.EarlyStopping(monitor="val_acc", patience=0)             # 'auto' maximises an accuracy
    model, _ = _wire(cb)
    _drive(cb, [0.5, 0.6], monitor="val_acc")
    assert not model.stop_training
    cb.on_epoch_end(2, {"val_acc": 0.6})
    assert model.stop_training


def test_model_checkpoint_period_best_only_and_file_name(tmp_path):
    saved = []
    pattern = str(tmp_path / "ssd7_epoch-{epoch:02d}_loss-{loss:.4f}_val_loss-{val_loss:.4f}.h5")
    cb = T.ModelCheckpoint(pattern, monitor="val_loss", verbose=1, save_best_only=False, save_weights_only=False, mode="auto", period=2)
    cb._save = saved.append
    _wire(cb)
    for epoch in range(5):
        cb.on_epoch_end(epoch, {"loss": 3.14159 - epoch, "val_loss": 2.5})
    assert saved == [str(tmp_path / "ssd7_epoch-02_loss-2.1416_val_loss-2.5000.h5"), str(tmp_path / "ssd7_epoch-04_loss-0.1416_val_loss-2.5000.h5")]
    # save_best_only: strict improvement on `best`, which is assignable; a missing monitor warns and skips
    saved.clear()
    cb = T.ModelCheckpoint(str(tmp_path / "w-{epoch:02d}.h5"), monitor="val_loss", save_best_only=True, save_weights_only=True)
    cb._save = saved.append
    _wire(cb)
    assert cb.best == np.inf
    cb.best = 1.0
    with pytest.warns(RuntimeWarning, match="val_loss"):
        cb.on_epoch_end(0, {"loss": 0.1})
    for epoch, v in enumerate([1.0, 0.9, 0.9, 0.8], start=1):
        cb.on_epoch_end(epoch, {"val_loss": v})
    assert saved == [str(tmp_path / "w-03.h5"), str(tmp_path / "w-05.h5")] and cb.best == 0.8
    assert T.ModelCheckpoint("x", monitor="val_acc").best == -np.inf and T.ModelCheckpoint("x", monitor="fmeasure_1").mode == "max"
    with pytest.warns(RuntimeWarning):
        assert T.ModelCheckpoint("x", mode="sideways").mode == "min"


def test_csv_logger_exact_bytes_and_append(tmp_path):
    path = str(tmp_path / "log.csv")
    cb = T.CSVLogger(filename=path, separator=",", append=True)      # the notebooks' call; no file yet: a header is written
    _wire(cb)
    cb.on_epoch_end(0, {"val_loss": 2.5, "loss": 3.25, "lr": 0.001})
    cb.on_epoch_end(1, {"val_loss": 2.0, "loss": 0.1, "lr": 0.0002})
    cb.on_train_end({})
    want = b"epoch,loss,lr,val_loss\r\n0,3.25,0.001,2.5\r\n1,0.1,0.0002,2.0\r\n"
    assert open(path, "rb").read() == want
    cb = T.CSVLogger(filename=path, separator=",", append=True)      # a second run: no second header
    _wire(cb)
    cb.on_epoch_end(2, {"val_loss": 1.5, "loss": float("nan"), "lr": 1e-05})
    cb.on_train_end({})
    assert open(path, "rb").read() == want + b"2,nan,1e-05,1.5\r\n"
    cb = T.CSVLogger(filename=path, separator=";")                   # append=False starts over
    model, _ = _wire(cb)
    cb.on_epoch_end(0, {"loss": 1.0, "val_loss": 2.0})
    model.stop_training = True                                       # an aborted epoch has no val_loss: 'NA'
    cb.on_epoch_end(1, {"loss": float("inf")})
    cb.on_train_end({})
    assert open(path, "rb").read() == b"epoch;loss;val_loss\r\n0;1.0;2.0\r\n1;inf;NA\r\n"


def test_learning_rate_scheduler():
    def ssd300_schedule(epoch):                                      # ssd300_training.ipynb: one argument
        return 0.001 if epoch < 2 else 0.0001

    cb = T.LearningRateScheduler(schedule=ssd300_schedule, verbose=1)
    _, opt = _wire(cb, lr=0.5)
    logs = _drive(cb, [1.0, 1.0, 1.0], begin=True)
    assert opt.set == [0.001, 0.001, 0.0001] and [l["lr"] for l in logs] == [0.001, 0.001, 0.0001]
    cb = T.LearningRateScheduler(lambda epoch, lr: lr * 0.5 if epoch >= 1 else lr)   # two arguments: the current rate comes in
    _, opt = _wire(cb, lr=0.5)
    _drive(cb, [1.0, 1.0, 1.0], begin=True)
    assert opt.set == [0.5, 0.25, 0.125]
    cb = T.LearningRateScheduler(lambda epoch: np.float32(0.25))
    _, opt = _wire(cb)
    cb.on_epoch_begin(0, {})
    assert opt.set == [0.25]
    cb = T.LearningRateScheduler(lambda epoch: 1)                    # an int is not a float
    _wire(cb)
    with pytest.raises(ValueError, match="float"):
        cb.on_epoch_begin(0, {})


def test_history_and_terminate_on_nan(capsys):
    h = T.History()
    _wire(h)
    h.on_epoch_end(3, {"loss": 1.0})
    h.on_epoch_end(4, {"loss": 0.5, "val_loss": 2.0})
    assert h.epoch == [3, 4] and h.history == {"loss": [1.0, 0.5], "val_loss": [2.0]}
    cb = T.TerminateOnNaN()
    model, _ = _wire(cb)
    cb.on_invalid_loss(2)
    assert model.stop_training and capsys.readouterr().out == "Batch 2: Invalid loss, terminating training\n"


def test_regularized_param_groups_and_the_one_time_warning():
    import torch
    from ssd_keras_amd.models.keras_ssd7 import build_model
    model = build_model((76, 68, 3), 3, mode="training", l2_regularization=5e-4)
    groups = T.regularized_param_groups(model)
    kernels = [m.weight for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    assert groups[0]["weight_decay"] == 2 * 5e-4 and groups[1]["weight_decay"] == 0.0
    assert [id(p) for p in groups[0]["params"]] == [id(p) for p in kernels] and all(p.dim() == 4 for p in kernels)
    assert len(groups[0]["params"]) + len(groups[1]["params"]) == len(list(model.parameters()))
    T._warned_penalty = False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T._check_penalty_gradient(model, _GroupsOnly(groups))        # the groups carry it: silent
    with pytest.warns(RuntimeWarning, match="regularized_param_groups"):
        T._check_penalty_gradient(model, _GroupsOnly([{"params": [], "weight_decay": 0.0}]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T._check_penalty_gradient(model, _GroupsOnly([{"params": [], "weight_decay": 0.0}]))   # once


class _GroupsOnly:
    def __init__(self, groups):
        self.param_groups = groups


def test_mark_replayed_bumps_versions_and_keeps_the_masters():
    """What the loop calls behind an epoch of replays: every parameter's `_version` moves once, and the optimizer takes that as its
    own write -- the next step continues from the master instead of taking it from the (rounded) parameter again."""
    import torch
    from ssd_keras_amd.optimizers import SGD
    p = torch.nn.Parameter(torch.ones(4, dtype=torch.bfloat16))
    p.grad = torch.full_like(p, 1e-3)
    opt = SGD([p], lr=1e-3, momentum=0.9, master_weights=True)
    opt.step()                                                       # master 1 - 1e-6; the bf16 parameter still reads 1
    assert bool((p == 1).all()) and bool((opt.state[p]["master"] < 1).all())
    version = p._version
    opt.mark_replayed()
    assert p._version == version + 1
    opt.step()                                                       # 1 - 1e-6 - 1.9e-6; from the parameter it would be 1 - 1.9e-6
    assert bool((opt.state[p]["master"] < 1 - 2.5e-6).all())


def test_a_cpu_model_fails_loudly():
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    from ssd_keras_amd.models.keras_ssd7 import build_model
    from ssd_keras_amd.optimizers import SGD
    model = build_model((76, 68, 3), 3, mode="training")
    with pytest.raises(nat.SsdHipError, match="GPU"):
        T.fit_generator(model, iter([]), 1, optimizer=SGD(model.parameters(), lr=1e-3, momentum=0.9), loss=SSDLoss())
