"""`ssd_keras_amd.training.MeanAveragePrecision` in `fit_generator`, on the SSD7 test model and fixed batches of tests/test_fit_gpu.py and
the 8-image CSV fixture of tests/data_generator_cases.py as validation set: training with the callback leaves, bit for bit, what training
without it leaves; `val_mAP` is what an `Evaluator` run by hand on a copy of the epoch's weights returns; `period` skips epochs."""
import copy
import itertools
import random
import types

import numpy as np
import pytest

from tests import data_generator_cases as dc
from tests.test_fit_gpu import _batches, _loss, _model, _optimizer, _optimizers_equal
from tests.test_ssd7_fused_training_gpu import _state_equal, deterministic_convolutions  # noqa: F401  (the last one is a fixture)

pytestmark = pytest.mark.gpu

# 'pad' draws from np.random; a low matching threshold, so that a barely trained model has true positives and the mAP is not 0
EVAL = dict(data_generator_mode='pad', decoding_confidence_thresh=0.05, decoding_top_k=40, matching_iou_threshold=0.1)


def _validation_set():
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    return dc.csv_generator(types.SimpleNamespace(DataGenerator=DataGenerator), load_images_into_memory=True, verbose=False)


def _fit(batches, callbacks, epochs=2):
    from ssd_keras_amd.training import fit_generator
    np.random.seed(77)
    random.seed(78)
    model = _model()
    opt = _optimizer(model)
    hist = fit_generator(model, itertools.cycle(batches), len(batches), epochs, optimizer=opt, loss=_loss(), callbacks=callbacks)
    return model, opt, hist, (np.random.get_state(), random.getstate())


def _recorder():
    from ssd_keras_amd.training import Callback

    class Recorder(Callback):
        def __init__(self):
            super().__init__()
            self.logs, self.weights, self.training = [], [], []

        def on_epoch_end(self, epoch, logs=None):
            self.logs.append(dict(logs))
            self.weights.append(copy.deepcopy(self.model.state_dict()))
            self.training.append(self.model.training)
    return Recorder()


def test_the_callback_does_not_disturb_training_and_reports_the_hand_run_map(deterministic_convolutions):  # noqa: F811
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator
    from ssd_keras_amd.training import MeanAveragePrecision
    batches = _batches(_model())
    plain_model, plain_opt, plain_hist, plain_rng = _fit(batches, [])
    rec = _recorder()
    cb = MeanAveragePrecision(_validation_set(), 3, 76, 68, 3, **EVAL)
    model, opt, hist, rng = _fit(batches, [cb, rec])
    assert _state_equal(model, plain_model) and _optimizers_equal(opt, model, plain_opt, plain_model)      # parameters, BatchNorm buffers, state
    assert opt.iterations == plain_opt.iterations == 2 * len(batches)
    assert hist.history["loss"] == plain_hist.history["loss"] and list(plain_hist.history) == ["loss"]
    assert all(np.array_equal(a, b) for a, b in zip(rng[0][1:], plain_rng[0][1:])) and np.array_equal(rng[0][1], plain_rng[0][1])
    assert rng[1] == plain_rng[1]
    assert rec.training == [True, True] and model.training
    # val_mAP: in the History, in the logs the later callbacks saw, a Python float, and the evaluator's own figure on those weights
    values = hist.history["val_mAP"]
    assert len(values) == 2 and all(type(v) is float for v in values) and [l["val_mAP"] for l in rec.logs] == values
    for weights, value in zip(rec.weights, values):
        twin = _model()
        twin.load_state_dict(weights)
        twin.eval()
        np.random.seed(77)                                       # the state the callback's evaluation started from (and put back)
        hand = Evaluator(twin, 3, _validation_set(), model_mode='training')
        by_hand = hand(76, 68, 3, verbose=False, collect='host', **EVAL)
        print("val_mAP %r, by hand %r, %d predictions" % (value, by_hand, sum(len(r) for r in hand.prediction_results)))
        assert value == float(by_hand)
    # the last epoch's evaluation is still on the callback's evaluator: the same predictions and per-class figures as by hand
    assert cb.evaluator.model is model and sum(len(r) for r in hand.prediction_results) > 0
    assert cb.evaluator.prediction_results == hand.prediction_results and cb.evaluator.average_precisions == hand.average_precisions
    assert all(np.array_equal(a, b) for a, b in zip(cb.evaluator.cumulative_true_positives[1:], hand.cumulative_true_positives[1:]))


def test_period_two_leaves_the_key_out_of_the_first_epoch(deterministic_convolutions):  # noqa: F811
    from ssd_keras_amd.training import MeanAveragePrecision
    batches = _batches(_model())
    rec = _recorder()
    model, opt, hist, _ = _fit(batches, [MeanAveragePrecision(_validation_set(), 3, 76, 68, 3, period=2, **EVAL), rec])
    assert "val_mAP" not in rec.logs[0] and "val_mAP" in rec.logs[1]
    assert hist.history["val_mAP"] == [rec.logs[1]["val_mAP"]] and len(hist.history["loss"]) == 2
