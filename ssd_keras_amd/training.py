"""`model.fit_generator(...)` of ssd7_training.ipynb / ssd300_training.ipynb, and the callbacks those notebooks hand it, for this
package's models: the training loop as replays of ONE captured HIP graph per batch shape.

    from ssd_keras_amd.training import (fit_generator, regularized_param_groups, ModelCheckpoint, CSVLogger, EarlyStopping,
                                        ReduceLROnPlateau, LearningRateScheduler, TerminateOnNaN)
    optimizer = SGD(regularized_param_groups(model), lr=1e-3, momentum=0.9, master_weights=True)
    history = fit_generator(model, train_generator, steps_per_epoch, epochs, optimizer=optimizer, loss=SSDLoss(...),
                            callbacks=[...], validation_data=val_generator, validation_steps=n)

The step, in this order: `optimizer.zero_grad(set_to_none=True)`, forward, `loss.compute_loss`, `.mean().backward()`, the sum of
squares of every `nn.Conv2d` kernel (one libssdhip launch per dtype, only when `model.l2_regularization` is non-zero; the optimizer's
float32 master is read where it holds one, else the parameter), the meter update, `optimizer.step()`.  What Keras reports as `loss` and
`val_loss` -- the batch-size-weighted mean over the epoch of `mean(compute_loss) + l2 * sum(w^2)` -- is accumulated on the device by the
meter launch inside the graph (csrc/ssdhip_fit.hip); the host reads 48 bytes at the end of an epoch, and every `nan_poll` steps when a
`TerminateOnNaN` is present, through an asynchronous copy into pinned memory and an event it waits for -- never a device-wide
synchronisation.

The capture protocol (what tests/test_ssd7_head_training_gpu.py spells out), once per batch shape: a warm-up forward + backward on a
side stream with no optimizer step; the model's buffers put back (BatchNorm's running statistics and `num_batches_tracked` moved; the
parameters did not, so this is the restored `state_dict` -- without writing the parameters behind the optimizer's master weights);
`optimizer.init_state()`; capture.  A capture runs nothing.  `graph=False` follows the same protocol and runs the same step eagerly:
given the same batches the two leave bit-identical parameters, buffers, optimizer state and `History`.

Where this departs from Keras 2.2.4, on purpose:
  * the penalty's GRADIENT is not added here: it is the optimizer's `weight_decay = 2 * l2` on the convolution kernels
    (`regularized_param_groups`); a warning is emitted once when `model.l2_regularization` is set and no group carries it;
  * `History` runs first, then the caller's callbacks in list order (Keras runs it last): `history.history` has `loss` and `val_loss`,
    the `lr` the learning-rate callbacks add to the logs reaches the callbacks behind them (a `CSVLogger`), not `History`;
  * per-batch hooks are not called: nothing about a batch is known to the host when its replay has been enqueued;
  * `TerminateOnNaN` sees a non-finite batch loss at the next poll, so up to `nan_poll - 1` further updates are applied to weights
    that are already non-finite (Keras does not undo the bad update either); the batch index it prints is exact (the meter latches it);
  * `ModelCheckpoint(save_weights_only=False)` writes the Keras weight file plus `path + '.optim.pt'`, a `torch.save` of
    `optimizer.state_dict()`, in place of Keras's `optimizer_weights` group (DESIGN.md 7 leaves that group out of scope).
No CPU path: a CPU model or a missing GPU raises.  Single process: the meter is per process, nothing is reduced across
`DistributedDataParallel` ranks."""
from __future__ import annotations

import csv
import io
import os
import warnings
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from .optimizers import _bump_versions

__all__ = ["fit_generator", "regularized_param_groups", "Callback", "History", "ModelCheckpoint", "CSVLogger", "EarlyStopping",
           "ReduceLROnPlateau", "LearningRateScheduler", "TerminateOnNaN", "MeanAveragePrecision"]


# ---- callbacks (keras/callbacks.py, Keras 2.2.4) ----------------------------------------------------------------------------------
class Callback:
    """keras.callbacks.Callback: `self.model`, `self.optimizer` (Keras reaches it as `self.model.optimizer`) and `self.params`."""

    def __init__(self):
        self.model = None
        self.optimizer = None
        self.params = {}

    def set_params(self, params):
        self.params = params

    def set_model(self, model):
        self.model = model

    def set_optimizer(self, optimizer):
        self.optimizer = optimizer

    def on_train_begin(self, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass

    # learning rates: read from the first group, set through `set_lr` -- between replays the only way that works
    def _get_lr(self):
        return float(self.optimizer.param_groups[0]["lr"])

    def _set_lr(self, lr):
        self.optimizer.set_lr(float(lr))


class History(Callback):
    """What `fit_generator` returns: `epoch` (0-based) and `history[key]`, one list entry per epoch."""

    def on_train_begin(self, logs=None):
        self.epoch = []
        self.history = {}

    def on_epoch_end(self, epoch, logs=None):
        self.epoch.append(epoch)
        for k, v in (logs or {}).items():
            self.history.setdefault(k, []).append(v)


def _monitor_mode(name, monitor, mode):
    """'min' or 'max' for `mode`; 'auto' maximises a monitor whose name contains 'acc' or starts with 'fmeasure'."""
    if mode not in ("auto", "min", "max"):
        warnings.warn("%s mode %s is unknown, fallback to auto mode." % (name, mode), RuntimeWarning)
        mode = "auto"
    if mode == "auto":
        mode = "max" if ("acc" in monitor or monitor.startswith("fmeasure")) else "min"
    return mode


class ModelCheckpoint(Callback):
    """keras.callbacks.ModelCheckpoint.  Every `period` epochs: `filepath.format(epoch=epoch + 1, **logs)` receives
    `save_keras_weights_h5(export_keras_weights(model), path)`, the file `model.save_weights` writes; with `save_weights_only=False`
    also `path + '.optim.pt'`, a `torch.save` of `optimizer.state_dict()` -- this replaces the `optimizer_weights` group of Keras's
    full-model file, which this package does not write.  `best` is assignable before training, as the SSD300 notebook's
    commented line does."""

    def __init__(self, filepath, monitor="val_loss", verbose=0, save_best_only=False, save_weights_only=False, mode="auto", period=1):
        super().__init__()
        self.filepath, self.monitor, self.verbose = filepath, monitor, verbose
        self.save_best_only, self.save_weights_only, self.period = save_best_only, save_weights_only, period
        self.epochs_since_last_save = 0
        self.mode = _monitor_mode("ModelCheckpoint", monitor, mode)
        self.best = np.inf if self.mode == "min" else -np.inf

    def _improved(self, current):
        return current < self.best if self.mode == "min" else current > self.best

    def _save(self, path):
        from .models.keras_weights import export_keras_weights, save_keras_weights_h5
        save_keras_weights_h5(export_keras_weights(self.model), path)
        if not self.save_weights_only:
            torch.save(self.optimizer.state_dict(), path + ".optim.pt")

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        self.epochs_since_last_save += 1
        if self.epochs_since_last_save < self.period:
            return
        self.epochs_since_last_save = 0
        path = self.filepath.format(epoch=epoch + 1, **logs)
        if self.save_best_only:
            current = logs.get(self.monitor)
            if current is None:
                warnings.warn("Can save best model only with %s available, skipping." % self.monitor, RuntimeWarning)
                return
            if not self._improved(current):
                if self.verbose > 0:
                    print("\nEpoch %05d: %s did not improve from %0.5f" % (epoch + 1, self.monitor, self.best))
                return
            if self.verbose > 0:
                print("\nEpoch %05d: %s improved from %0.5f to %0.5f, saving model to %s" % (epoch + 1, self.monitor, self.best, current, path))
            self.best = current
        elif self.verbose > 0:
            print("\nEpoch %05d: saving model to %s" % (epoch + 1, path))
        self._save(path)


class CSVLogger(Callback):
    """keras.callbacks.CSVLogger: the header `epoch` + the sorted keys of the first epoch's logs, then one row per epoch with `str()` of
    every value (the csv module's excel dialect with `separator`: rows end in CR LF).  `append=True` on an existing, non-empty file
    writes no second header."""

    def __init__(self, filename, separator=",", append=False):
        super().__init__()
        self.filename, self.sep, self.append = filename, separator, append
        self.writer, self.keys, self.append_header, self.csv_file = None, None, True, None

    def on_train_begin(self, logs=None):
        mode = "w"
        if self.append:
            if os.path.exists(self.filename):
                with open(self.filename, "r") as f:
                    self.append_header = not bool(len(f.readline()))
            mode = "a"
        self.csv_file = io.open(self.filename, mode, newline="")

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        if self.keys is None:
            self.keys = sorted(logs.keys())
        if getattr(self.model, "stop_training", False):          # an aborted epoch: what is missing is 'NA'
            logs = dict((k, logs[k] if k in logs else "NA") for k in self.keys)
        if self.writer is None:
            class CustomDialect(csv.excel):
                delimiter = self.sep
            self.writer = csv.DictWriter(self.csv_file, fieldnames=["epoch"] + self.keys, dialect=CustomDialect)
            if self.append_header:
                self.writer.writeheader()
        row = OrderedDict({"epoch": epoch})
        row.update((key, str(logs[key])) for key in self.keys)
        self.writer.writerow(row)
        self.csv_file.flush()

    def on_train_end(self, logs=None):
        if self.csv_file is not None:
            self.csv_file.close()
        self.writer, self.csv_file = None, None


class EarlyStopping(Callback):
    """keras.callbacks.EarlyStopping: in min mode an epoch improves when `current + min_delta < best`; otherwise `wait += 1`, and at
    `wait >= patience` it sets `stopped_epoch` and `model.stop_training`."""

    def __init__(self, monitor="val_loss", min_delta=0, patience=0, verbose=0, mode="auto"):
        super().__init__()
        self.monitor, self.patience, self.verbose = monitor, patience, verbose
        self.min_delta = abs(min_delta)
        self.mode = _monitor_mode("EarlyStopping", monitor, mode)
        self.wait, self.stopped_epoch = 0, 0
        self.best = np.inf if self.mode == "min" else -np.inf

    def on_train_begin(self, logs=None):
        self.wait, self.stopped_epoch = 0, 0
        self.best = np.inf if self.mode == "min" else -np.inf

    def on_epoch_end(self, epoch, logs=None):
        current = (logs or {}).get(self.monitor)
        if current is None:
            warnings.warn("Early stopping conditioned on metric `%s` which is not available. Available metrics are: %s"
                          % (self.monitor, ",".join(list((logs or {}).keys()))), RuntimeWarning)
            return
        better = current + self.min_delta < self.best if self.mode == "min" else current - self.min_delta > self.best
        if better:
            self.best = current
            self.wait = 0
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self.stopped_epoch = epoch
                self.model.stop_training = True

    def on_train_end(self, logs=None):
        if self.stopped_epoch > 0 and self.verbose > 0:
            print("Epoch %05d: early stopping" % (self.stopped_epoch + 1))


class ReduceLROnPlateau(Callback):
    """keras.callbacks.ReduceLROnPlateau.  Each epoch: `logs['lr']` first; in cooldown the counter goes down and `wait = 0`; the epoch
    improves when `current < best - min_delta` (min mode); otherwise, outside cooldown, `wait += 1`, and at `wait >= patience` a rate
    above `min_lr` becomes `max(lr * factor, min_lr)`, the cooldown starts and `wait = 0`.  `epsilon` is the old name of `min_delta`
    (ssd7_training.ipynb passes it), accepted with a warning."""

    def __init__(self, monitor="val_loss", factor=0.1, patience=10, verbose=0, mode="auto", min_delta=1e-4, cooldown=0, min_lr=0,
                 epsilon=None):
        super().__init__()
        if factor >= 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0.")
        if epsilon is not None:
            min_delta = epsilon
            warnings.warn("`epsilon` argument is deprecated and will be removed, use `min_delta` instead.")
        self.monitor, self.factor, self.patience, self.verbose = monitor, factor, patience, verbose
        self.min_delta, self.cooldown, self.min_lr = min_delta, cooldown, min_lr
        self.mode = mode
        self._reset()

    def _reset(self):
        self._mode = _monitor_mode("Learning Rate Plateau Reducing", self.monitor, self.mode)
        self.best = np.inf if self._mode == "min" else -np.inf
        self.cooldown_counter, self.wait = 0, 0

    def _improved(self, current):
        return current < self.best - self.min_delta if self._mode == "min" else current > self.best + self.min_delta

    def in_cooldown(self):
        return self.cooldown_counter > 0

    def on_train_begin(self, logs=None):
        self._reset()

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        logs["lr"] = self._get_lr()
        current = logs.get(self.monitor)
        if current is None:
            warnings.warn("Reduce LR on plateau conditioned on metric `%s` which is not available. Available metrics are: %s"
                          % (self.monitor, ",".join(list(logs.keys()))), RuntimeWarning)
            return
        if self.in_cooldown():
            self.cooldown_counter -= 1
            self.wait = 0
        if self._improved(current):
            self.best = current
            self.wait = 0
        elif not self.in_cooldown():
            self.wait += 1
            if self.wait >= self.patience:
                old_lr = self._get_lr()
                if old_lr > self.min_lr:
                    new_lr = max(old_lr * self.factor, self.min_lr)
                    self._set_lr(new_lr)
                    if self.verbose > 0:
                        print("\nEpoch %05d: ReduceLROnPlateau reducing learning rate to %s." % (epoch + 1, new_lr))
                    self.cooldown_counter = self.cooldown
                    self.wait = 0


class LearningRateScheduler(Callback):
    """keras.callbacks.LearningRateScheduler: `schedule(epoch, lr)` at the beginning of every epoch (`schedule(epoch)` where the
    function takes one argument); the result must be a float.  Adds `logs['lr']` at the end of the epoch."""

    def __init__(self, schedule, verbose=0):
        super().__init__()
        self.schedule, self.verbose = schedule, verbose

    def on_epoch_begin(self, epoch, logs=None):
        lr = self._get_lr()
        try:
            lr = self.schedule(epoch, lr)
        except TypeError:                                    # the old API: schedule(epoch)
            lr = self.schedule(epoch)
        if not isinstance(lr, (float, np.float32, np.float64)):
            raise ValueError('The output of the "schedule" function should be float.')
        self._set_lr(float(lr))
        if self.verbose > 0:
            print("\nEpoch %05d: LearningRateScheduler setting learning rate to %s." % (epoch + 1, lr))

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            logs["lr"] = self._get_lr()


class TerminateOnNaN(Callback):
    """keras.callbacks.TerminateOnNaN.  The loop polls the meter every `nan_poll` steps when one of these is among the callbacks and
    calls `on_invalid_loss` with the index of the first batch of the epoch whose loss was not finite: Keras's message, and
    `model.stop_training`."""

    def on_invalid_loss(self, batch):
        print("Batch %d: Invalid loss, terminating training" % batch)
        self.model.stop_training = True


class MeanAveragePrecision(Callback):
    """Not in Keras: the Pascal VOC mean average precision of the model on `data_generator` (a `DataGenerator` with labels) as
    `logs[name]`, a Python float, every `period` epochs; on the other epochs the key is not set (a `ModelCheckpoint(save_best_only=True)`
    or `EarlyStopping` monitoring it then warns and skips that epoch, as Keras does for a missing monitor -- give them the same period;
    a `CSVLogger` takes its columns from the first epoch's keys, as Keras's does, so it logs the key only with `period=1`).
    It must come before the callbacks that monitor it: callbacks run in list order and each sees what the ones before it put into
    `logs`.  `fit_generator` itself runs it ahead of its `History`, so `history.history[name]` has one entry per evaluated epoch.

    `on_epoch_end` puts the model in `eval()`, calls an `Evaluator(model, n_classes, data_generator, model_mode='training')` -- built
    once, so the packed ground truth is reused -- with `collect` ('device': nothing between the decoder and the matcher leaves the GPU)
    and `evaluator_kwargs` (`data_generator_mode`, `average_precision_mode`, `decoding_*`, ...; `verbose` defaults to False), and puts
    `train()` back.  `fit_generator` has called its `settle()` by then, so the tensors the model derives for its inference path follow
    the replayed weights.  Training is not disturbed: the evaluation runs under `no_grad` in `eval()` (BatchNorm's statistics and
    `optimizer.iterations` do not move, no captured graph is touched), and the states of `np.random` and `random` -- which the 'pad'
    mode's transformations draw from -- are put back."""

    provides_logs = True

    def __init__(self, data_generator, n_classes, img_height, img_width, batch_size, period=1, name="val_mAP", collect="device",
                 **evaluator_kwargs):
        super().__init__()
        if period < 1:
            raise ValueError("period must be at least 1")
        self.data_generator, self.n_classes = data_generator, n_classes
        self.img_height, self.img_width, self.batch_size = img_height, img_width, batch_size
        self.period, self.name, self.collect = period, name, collect
        self.evaluator_kwargs = dict(evaluator_kwargs)
        self.evaluator_kwargs.setdefault("verbose", False)
        self.evaluator = None

    def on_epoch_end(self, epoch, logs=None):
        if (epoch + 1) % self.period:
            return
        import random
        from .eval_utils.average_precision_evaluator import Evaluator
        model = self.model
        if self.evaluator is None or self.evaluator.model is not model:
            self.evaluator = Evaluator(model, self.n_classes, self.data_generator, model_mode="training")
        was_training = model.training
        states = np.random.get_state(), random.getstate()
        model.eval()
        try:
            value = self.evaluator(self.img_height, self.img_width, self.batch_size, collect=self.collect, **self.evaluator_kwargs)
        finally:
            model.train(was_training)
            np.random.set_state(states[0])
            random.setstate(states[1])
        if logs is not None:
            logs[self.name] = float(value)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
def _conv_kernels(model):
    return [m.weight for m in model.modules() if isinstance(m, nn.Conv2d)]


def regularized_param_groups(model):
    """The two parameter groups that express Keras's `kernel_regularizer=l2(l2_reg)` for the optimizer: the kernels of every
    `nn.Conv2d` with `weight_decay = 2 * model.l2_regularization` (the gradient of `l2 * sum(w^2)`), every other parameter with 0."""
    kernels = _conv_kernels(model)
    ids = {id(p) for p in kernels}
    rest = [p for p in model.parameters() if id(p) not in ids]
    return [{"params": kernels, "weight_decay": 2.0 * float(model.l2_regularization or 0.0)}, {"params": rest, "weight_decay": 0.0}]


_warned_penalty = False


def _check_penalty_gradient(model, optimizer):
    global _warned_penalty
    l2 = float(getattr(model, "l2_regularization", 0.0) or 0.0)
    if l2 == 0.0 or _warned_penalty:
        return
    if not any(abs(float(g.get("weight_decay", 0.0)) - 2.0 * l2) <= 1e-12 * l2 for g in optimizer.param_groups):
        _warned_penalty = True
        warnings.warn("model.l2_regularization = %g, but no parameter group of the optimizer has weight_decay = %g: the reported loss "
                      "contains the penalty, the update does not follow its gradient.  Build the optimizer from "
                      "regularized_param_groups(model)." % (l2, 2.0 * l2), RuntimeWarning, stacklevel=3)


class _Meter:
    """A state block of csrc/ssdhip_fit.hip on the device and its pinned mirror on the host."""

    def __init__(self, device):
        n = nat.fit_meter_state_bytes()
        self.block = torch.zeros((n,), dtype=torch.uint8, device=device)
        self.host = torch.zeros((n,), dtype=torch.uint8).pin_memory()
        self.event = torch.cuda.Event()

    def reset(self):
        nat.fit_meter_reset(self.block)

    def read(self):
        """The block as the stream leaves it behind everything enqueued so far: an asynchronous copy into pinned memory and a wait for
        ITS event -- not a device-wide synchronisation."""
        self.host.copy_(self.block, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        return nat.fit_meter_parse(self.host.numpy())


class _Captured:
    def __init__(self, images, y_true):
        self.images, self.y_true = torch.empty_like(images), torch.empty(y_true.shape, dtype=torch.float32, device=images.device)
        self.graph = None


class _Loop:
    """The step, the validation step, and one capture of each per batch shape (two shapes at most; a third runs eagerly)."""

    MAX_CAPTURES = 2

    def __init__(self, model, optimizer, loss, graph):
        self.model, self.optimizer, self.loss, self.graph = model, optimizer, loss, bool(graph)
        params = list(model.parameters())
        if not torch.cuda.is_available() or not params or not all(p.is_cuda for p in params):
            raise nat.SsdHipError("fit_generator needs the model on a GPU: ssd_keras_amd has no CPU path")
        nat.load()
        self.device = params[0].device
        # Everything the loop enqueues -- staging copies, captures, replays, the callbacks' set_lr, the meter's reads -- goes to ONE
        # stream of its own: a capture needs a non-default stream, and every graph is replayed on the stream it was captured on.
        self.stream = torch.cuda.Stream(self.device)
        self.l2 =float(getattr(model, "l2_regularization", 0.0) or 0.0)
        self.train_meter, self.val_meter = _Meter(self.device), _Meter(self.device)
        self.captures = {"train": {}, "val": {}}
        self.ready = False                                   # the optimizer's state exists and the penalty's tables name it
        self.replayed = False                                # training replays since the last `settle`
        self.tables, self.partials = [], None
        self.launches = {"sumsq": 0, "meter": 0}             # native launches enqueued or recorded by the latest step

    # -- the penalty ------------------------------------------------------------------------------------------------------------------
    def _build_penalty(self):
        """The tables of the sum-of-squares launch: every conv kernel, its float32 master where the optimizer holds one; the float32
        tensors first, then the bf16 ones, each in `model.modules()` order, and one partial per chunk in that order."""
        self.tables, self.partials, self._penalty_keep = [], None, []
        if self.l2 == 0.0:
            return
        flat = lambda t: t.detach().as_strided((t.numel(),), (1,))
        sources = []
        for w in _conv_kernels(self.model):
            st = self.optimizer.state[w] if w in self.optimizer.state else {}
            sources.append(flat(st["master"]) if "master" in st else flat(w))
        by_dtype = [[t for t in sources if t.dtype == torch.float32], [t for t in sources if t.dtype == torch.bfloat16]]
        if sum(len(ts) for ts in by_dtype) != len(sources):
            raise nat.SsdHipError("fit_generator: convolution kernels must be float32 or bfloat16")
        tables = [nat.sumsq_table(ts, self.device) for ts in by_dtype if ts]
        self.partials = torch.zeros((sum(t[5] for t in tables),), dtype=torch.float32, device=self.device)
        at = 0
        for t in tables:
            self.tables.append((t, self.partials[at:at + t[5]]))
            at += t[5]
        self._penalty_keep = sources

    def _meter(self, meter, per_sample):
        self.launches = {"sumsq": 0, "meter": 0}
        for table, out in self.tables:
            nat.sumsq_partials(table, out)
            self.launches["sumsq"] += 1
        nat.fit_meter_update(meter.block, per_sample.detach(), self.partials, self.l2)
        self.launches["meter"] += 1

    # -- the two steps ------------------------------------------------------------------------------------------------------------------
    def _forward_backward(self, images, y_true):
        self.optimizer.zero_grad(set_to_none=True)
        per_sample = self.loss.compute_loss(y_true, self.model(images).float())
        per_sample.mean().backward()
        return per_sample

    def _train_step(self, images, y_true):
        per_sample = self._forward_backward(images, y_true)
        self._meter(self.train_meter, per_sample)
        self.optimizer.step()

    def _val_step(self, images, y_true):
        self._meter(self.val_meter, self.loss.compute_loss(y_true, self.model(images).float()))

    # -- the protocol -----------------------------------------------------------------------------------------------------------------
    def _warm_up(self, images, y_true):
        """A forward + backward with no optimizer step (on the loop's own stream, never the default one), then the model's buffers as
        they were: the gradients are in place, the optimizer's state and the penalty's tables exist."""
        buffers = [(b, b.detach().clone()) for b in self.model.buffers()]
        self._forward_backward(images, y_true)
        torch.cuda.synchronize(self.device)
        with torch.no_grad():
            for b, was in buffers:
                b.copy_(was)
        if not self.ready:
            self.optimizer.init_state()
            self._build_penalty()
            self.ready = True
        torch.cuda.synchronize(self.device)

    def _capture(self, kind, images, y_true):
        cap = _Captured(images, y_true)
        cap.images.copy_(images)
        cap.y_true.copy_(y_true)
        if kind == "train":
            self._warm_up(cap.images, cap.y_true)
        else:
            with torch.no_grad():                            # (twice: per-shape kernel choices and workspaces exist before the capture)
                for _ in range(2):
                    self.loss.compute_loss(cap.y_true, self.model(cap.images).float())
            torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream):
            if kind == "train":
                self._train_step(cap.images, cap.y_true)
            else:
                with torch.no_grad():
                    self._val_step(cap.images, cap.y_true)
        cap.graph = graph
        cap.derived_key = self._derived_key()
        return cap

    def _derived_key(self):
        key = getattr(self.model, "_derived_weights_key", None)
        return key() if key is not None else None

    def _refresh_derived(self, cap):
        """The tensors the model DERIVES from its parameters for the inference path (packed filters, BatchNorm tables): a captured
        evaluation reads them, so they are rebuilt in place when the training steps since the last evaluation changed their sources
        (what `SSDModel.graphed` does before its replays)."""
        key = self._derived_key()
        if key != cap.derived_key:
            self.model._refresh_derived_weights()
            cap.derived_key = key

    def settle(self):
        """Replays run no Python, so nothing has told the host that parameters and buffers changed: their `_version` is bumped here,
        once, as an eager step's in-place updates would have -- what the caches keyed on it (the model's derived inference tensors,
        which the evaluation reads) and the optimizer's masters go by.  Called behind an epoch's steps."""
        if self.replayed:
            self.optimizer.mark_replayed()
            buffers = [b for b in self.model.buffers() if b.is_cuda]
            if buffers:
                _bump_versions(buffers)
            self.replayed = False

    def _upload(self, batch):
        images, y_true = batch[0], batch[1]
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(np.ascontiguousarray(images))
        if isinstance(y_true, np.ndarray):
            y_true = torch.from_numpy(np.ascontiguousarray(y_true))
        return images, y_true

    def run(self, kind, batch):
        """One training or validation step on `batch` = (images, y_true): staged into the static buffers of its shape's capture and
        replayed, or -- without `graph`, and for a third and later shape -- run eagerly.  Returns the batch size."""
        images, y_true = self._upload(batch)
        key = (tuple(images.shape), images.dtype, tuple(y_true.shape))
        caps = self.captures[kind]
        cap = caps.get(key)
        if cap is None and self.graph and len(caps) < self.MAX_CAPTURES:
            cap = caps[key] = self._capture(kind, images.to(self.device), y_true.to(self.device))
        if cap is not None:
            cap.images.copy_(images, non_blocking=True)
            cap.y_true.copy_(y_true, non_blocking=True)          # (float64 labels of the device generator: cast in the copy)
            if kind == "val":
                self._refresh_derived(cap)
            else:
                self.replayed = True
            cap.graph.replay()
            return int(images.shape[0])
        images, y_true = images.to(self.device), y_true.to(self.device, dtype=torch.float32)
        if kind == "train":
            if not self.ready:
                self._warm_up(images, y_true)
            self._train_step(images, y_true)
        else:
            with torch.no_grad():
                self._val_step(images, y_true)
        return int(images.shape[0])


def _mean(state):
    return float(state["sum"] / state["seen"]) if state["seen"] else float("nan")


def fit_generator(model, generator, steps_per_epoch, epochs=1, *, optimizer, loss, callbacks=None, validation_data=None,
                  validation_steps=None, initial_epoch=0, verbose=0, graph=True, nan_poll=8):
    """Keras 2.2.4's `model.fit_generator` for an SSD7 / SSD300 / SSD512 of this package on a GPU.

    `generator`, `validation_data`: iterators (or iterables) that yield `(images, y_true)` -- what `DataGenerator.generate(...,
    device=...)` yields (uint8 NHWC images and float64 encoded labels on the device) or NumPy arrays, which are uploaded.  Every batch
    is copied into the static input buffers of its shape's captured step (images as they are, `y_true` as float32).  One capture per
    batch shape, two shapes (the full batch and the short last one of a dataset); a third and later shape runs eagerly.
    `optimizer`: `ssd_keras_amd.optimizers.SGD` or `Adam`; `loss`: an `SSDLoss`.  `graph=False` runs the same step eagerly.

    Per epoch, from `initial_epoch` to `epochs - 1`: `on_epoch_begin(epoch)`, `steps_per_epoch` steps, `validation_steps` validation
    steps (`model.eval()`, `no_grad`, their own capture and meter; BatchNorm's statistics are untouched and the model is put back in
    `train()`), `on_epoch_end(epoch, logs)` with `loss = sum / seen` of the meter, `val_loss` likewise (penalty included), and `lr`
    where a learning-rate callback adds it.  `History` runs first, then `callbacks` in order; it is returned.  Only a callback that
    declares `provides_logs` (`MeanAveragePrecision`) runs ahead of `History`, so that its key is in `history.history`.

    With a `TerminateOnNaN` among the callbacks the meter is read every `nan_poll` steps; on a latched non-finite loss the loop stops
    there -- up to `nan_poll - 1` further updates have then been applied to weights that are already non-finite; Keras does not undo
    the bad update either --, prints Keras's message with the exact batch index, sets `model.stop_training`, skips validation, calls
    `on_epoch_end` and returns, as Keras does.

    After it returns `optimizer.iterations` has advanced by the number of training steps taken, BatchNorm's `num_batches_tracked`
    likewise: warm-ups and captures leave no trace.  The meter is per process (no reduction across DistributedDataParallel ranks)."""
    if nan_poll < 1:
        raise ValueError("nan_poll must be at least 1")
    if validation_data is not None and not validation_steps:
        raise ValueError("validation_data needs validation_steps")
    loop = _Loop(model, optimizer, loss, graph)
    _check_penalty_gradient(model, optimizer)
    history = History()
    callbacks = list(callbacks or [])
    metrics = [cb for cb in callbacks if getattr(cb, "provides_logs", False)]      # (MeanAveragePrecision: its key is part of the History)
    cbs = metrics + [history] + [cb for cb in callbacks if cb not in metrics]
    terminators = [cb for cb in cbs if isinstance(cb, TerminateOnNaN)]
    params = {"epochs": epochs, "steps": steps_per_epoch, "verbose": verbose, "do_validation": validation_data is not None,
              "metrics": ["loss"] + (["val_loss"] if validation_data is not None else [])}
    for cb in cbs:
        cb.set_params(params)
        cb.set_model(model)
        if hasattr(cb, "set_optimizer"):
            cb.set_optimizer(optimizer)
    model.stop_training = False
    model.train()
    entered = torch.cuda.current_stream(loop.device)
    loop.stream.wait_stream(entered)
    try:
        with torch.cuda.stream(loop.stream):                 # (the generators run in here too: their device work is ordered with the steps)
            _epochs(loop, model, cbs, terminators, generator, steps_per_epoch, epochs, validation_data, validation_steps, initial_epoch,
                    verbose, nan_poll)
            torch.cuda.synchronize(loop.device)
    finally:
        entered.wait_stream(loop.stream)
    return history


def _epochs(loop, model, cbs, terminators, generator, steps_per_epoch, epochs, validation_data, validation_steps, initial_epoch, verbose,
            nan_poll):
    train_iter = iter(generator)
    val_iter = iter(validation_data) if validation_data is not None else None
    for cb in cbs:
        cb.on_train_begin({})
    for epoch in range(initial_epoch, epochs):
        for cb in cbs:
            cb.on_epoch_begin(epoch, {})
        loop.train_meter.reset()
        logs = {}
        for step in range(steps_per_epoch):
            loop.run("train", next(train_iter))
            if terminators and ((step + 1) % nan_poll == 0 or step + 1 == steps_per_epoch):
                bad = loop.train_meter.read()["first_bad"]
                if bad >= 0:
                    for cb in terminators:
                        cb.on_invalid_loss(bad)
                    break
        loop.settle()
        state = loop.train_meter.read()
        logs["loss"] = _mean(state)
        if val_iter is not None and not model.stop_training:
            model.eval()
            try:
                loop.val_meter.reset()
                for _ in range(validation_steps):
                    loop.run("val", next(val_iter))
                logs["val_loss"] = _mean(loop.val_meter.read())
            finally:
                model.train()
        if verbose:
            print("Epoch %d/%d - %s" % (epoch + 1, epochs, " - ".join("%s: %.4f" % kv for kv in logs.items())))
        for cb in cbs:
            cb.on_epoch_end(epoch, logs)
        if model.stop_training:
            break
    for cb in cbs:
        cb.on_train_end({})
