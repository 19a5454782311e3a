"""`val_mAP` in the epoch's logs: the callbacks of ssd_keras_amd/training.py that can monitor it behave as Keras 2.2.4's do when the key
is present and when it is absent (the epochs a `MeanAveragePrecision(period=...)` skips).  Stub model and optimizer, no GPU; the
callback's own evaluation runs in tests/test_fit_map_callback_gpu.py."""
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


class _Model:
    stop_training = False


def _wire(cb, lr=1e-3):
    model, opt = _Model(), _Optimizer(lr)
    cb.set_model(model)
    cb.set_optimizer(opt)
    cb.on_train_begin({})
    return model, opt


def test_model_checkpoint_saves_on_a_better_map_and_skips_an_epoch_without_one(tmp_path):
    saved = []
    cb = T.ModelCheckpoint(str(tmp_path / "w-{epoch:02d}_{val_mAP:.3f}.h5"), monitor="val_mAP", mode="max", save_best_only=True)
    cb._save = saved.append
    _wire(cb)
    assert cb.best == -np.inf
    for epoch, value in enumerate([0.25, 0.25, 0.5, 0.4]):
        cb.on_epoch_end(epoch, {"loss": 1.0, "val_mAP": value})
    assert saved == [str(tmp_path / "w-01_0.250.h5"), str(tmp_path / "w-03_0.500.h5")] and cb.best == 0.5
    saved.clear()
    cb = T.ModelCheckpoint(str(tmp_path / "w-{epoch:02d}.h5"), monitor="val_mAP", mode="max", save_best_only=True)
    cb._save = saved.append
    _wire(cb)
    with pytest.warns(RuntimeWarning, match="val_mAP"):
        cb.on_epoch_end(0, {"loss": 1.0})                          # absent: Keras warns and skips
    cb.on_epoch_end(1, {"loss": 1.0, "val_mAP": 0.1})
    assert saved == [str(tmp_path / "w-02.h5")]
    # 'auto' would MINIMISE it (the name has no 'acc'): the mode has to be given
    assert T.ModelCheckpoint("x", monitor="val_mAP").mode == "min"


def test_early_stopping_on_map():
    cb = T.EarlyStopping(monitor="val_mAP", mode="max", min_delta=0.01, patience=2)
    model, _ = _wire(cb)
    waits = []
    for epoch, value in enumerate([0.2, 0.205, 0.3, 0.3, 0.29]):
        cb.on_epoch_end(epoch, {"val_mAP": value})
        waits.append((cb.wait, model.stop_training))
    assert waits == [(0, False), (1, False), (0, False), (1, False), (2, True)] and cb.best == 0.3 and cb.stopped_epoch == 4
    cb = T.EarlyStopping(monitor="val_mAP", mode="max", patience=1)
    model, _ = _wire(cb)
    cb.on_epoch_end(0, {"val_mAP": 0.2})
    with pytest.warns(RuntimeWarning, match="val_mAP"):
        cb.on_epoch_end(1, {"loss": 1.0})                          # absent: a warning, no step of the state machine
    assert cb.wait == 0 and not model.stop_training


def test_reduce_lr_on_plateau_on_map():
    cb = T.ReduceLROnPlateau(monitor="val_mAP", mode="max", factor=0.5, patience=2, min_delta=0.0, min_lr=0)
    _, opt = _wire(cb, lr=1.0)
    for epoch, value in enumerate([0.3, 0.3, 0.3, 0.4]):
        cb.on_epoch_end(epoch, {"val_mAP": value})
    assert opt.set == [0.5] and cb.best == 0.4 and cb.wait == 0
    logs = {"loss": 1.0}
    with pytest.warns(RuntimeWarning):
        cb.on_epoch_end(4, logs)                                   # absent: only logs['lr'] is added
    assert logs == {"loss": 1.0, "lr": 0.5} and opt.set == [0.5] and cb.wait == 0


def test_csv_logger_takes_its_columns_from_the_first_epoch_as_keras_does(tmp_path):
    """keras/callbacks.py, CSVLogger.on_epoch_end: `self.keys = sorted(logs.keys())` at the first epoch, then `logs[key]` for each of
    them.  With period=1 the column is there; a key that first appears later is never written; a key of the first epoch that is
    absent later is Keras's KeyError (only an aborted epoch gets 'NA')."""
    path = str(tmp_path / "log.csv")
    cb = T.CSVLogger(filename=path)
    _wire(cb)
    cb.on_epoch_end(0, {"loss": 2.0, "val_mAP": 0.125})
    cb.on_epoch_end(1, {"loss": 1.5, "val_mAP": 0.25})
    with pytest.raises(KeyError, match="val_mAP"):
        cb.on_epoch_end(2, {"loss": 1.0})
    cb.on_train_end({})
    assert open(path, "rb").read() == b"epoch,loss,val_mAP\r\n0,2.0,0.125\r\n1,1.5,0.25\r\n"
    cb = T.CSVLogger(filename=path)                                # period=2: the first epoch has no val_mAP, the column never appears
    _wire(cb)
    cb.on_epoch_end(0, {"loss": 2.0})
    cb.on_epoch_end(1, {"loss": 1.5, "val_mAP": 0.25})
    cb.on_train_end({})
    assert open(path, "rb").read() == b"epoch,loss\r\n0,2.0\r\n1,1.5\r\n"


def test_period_and_arguments_without_a_gpu():
    calls = []

    class _Evaluator:
        model = None

        def __call__(self, *args, **kw):
            calls.append((args, kw))
            return np.float64(0.375)

    cb = T.MeanAveragePrecision("generator", 3, 76, 68, 4, period=2, data_generator_mode="pad", decoding_top_k=50)
    assert cb.provides_logs and cb.name == "val_mAP" and cb.collect == "device"

    class _Net(_Model):
        training = True

        def eval(self):
            self.training = False

        def train(self, mode=True):
            self.training = mode

    model = _Net()
    cb.set_model(model)
    cb.evaluator = _Evaluator()
    cb.evaluator.model = model
    state = np.random.get_state()[1].copy()
    logs0, logs1 = {"loss": 1.0}, {"loss": 0.5}
    cb.on_epoch_end(0, logs0)
    cb.on_epoch_end(1, logs1)
    assert logs0 == {"loss": 1.0} and logs1 == {"loss": 0.5, "val_mAP": 0.375} and type(logs1["val_mAP"]) is float
    assert calls == [((76, 68, 4), dict(collect="device", data_generator_mode="pad", decoding_top_k=50, verbose=False))]
    assert model.training and np.array_equal(np.random.get_state()[1], state)
    with pytest.raises(ValueError):
        T.MeanAveragePrecision("generator", 3, 76, 68, 4, period=0)
