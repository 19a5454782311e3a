"""`Evaluator.predict_on_dataset(collect='device')` / `Evaluator.__call__(collect='device')` against the host route -- the oracle, pinned
itself to tests/golden/evaluator.npz -- on the 8-image CSV fixture of tests/data_generator_cases.py: `prediction_results` equal element
for element and type for type, everything downstream equal, the results files byte-identical; the refusals; what assigning to
`prediction_results` does.  All comparisons are exact."""
import os
import types

import numpy as np
import pytest

from tests import data_generator_cases as dc

pytestmark = pytest.mark.gpu

N_CLASSES = 3


def _generator():
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    g = dc.csv_generator(types.SimpleNamespace(DataGenerator=DataGenerator), load_images_into_memory=True, verbose=False)
    g.image_ids = ['%06d' % (11 * i + 3) for i in range(len(g.image_ids))]      # Pascal VOC ids: the results files print them as integers
    return g


def _inference_model(rows=9, seed=1, beyond=False):
    """A stand-in for an inference-mode model: per image `rows` rows [class, conf, box in input coordinates] that depend on the image's
    pixels, zero padding (class 0) in the middle and at the end, float32 like the DecodeDetections layer's output."""
    import torch
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((rows, 6), generator=g)

    def model(batch):
        assert batch.dtype == torch.float32 and batch.is_cuda and batch.dim() == 4 and batch.shape[3] == 3
        B, H, W = batch.shape[:3]
        key = batch.reshape(B, -1)[:, ::97].sum(dim=1)                         # (whole numbers: exact in any order)
        out = base.to(batch.device)[None].repeat(B, 1, 1)
        cls = (torch.arange(rows, device=batch.device)[None] + key[:, None].long()) % (N_CLASSES + 1)
        cls[:, rows // 2] = 0
        cls[:, -1] = 0
        if beyond:
            cls[-1, 0] = N_CLASSES + 1
        out[:, :, 0] = cls.float()
        out[:, :, 1] = (out[:, :, 1] + key[:, None] % 7 / 7.0) / 2.0
        out[:, :, 2:4] = out[:, :, 2:4] * 0.5 * torch.tensor([W, H], device=batch.device) - 3.3
        out[:, :, 4:6] = out[:, :, 2:4] + out[:, :, 4:6] * 0.5 * torch.tensor([W, H], device=batch.device) + 1.7
        return out
    return model


def _ssd7():
    from tests.test_ssd7_fused_blocks_gpu import _model
    return _model(5)


def _evaluate(model, model_mode, collect, tmp_path, **kw):
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator
    ev = Evaluator(model, N_CLASSES, _generator(), model_mode=model_mode)
    np.random.seed(3)                                            # 'pad' places each image on its canvas at random
    height, width = kw.pop("size", (300, 300))
    out = ev(height, width, 3, verbose=False, return_precisions=True, return_recalls=True, return_average_precisions=True, collect=collect, **kw)
    prefix = str(tmp_path / (collect + "_"))
    ev.write_predictions_to_txt(out_file_prefix=prefix, verbose=False)
    files = {name[len(collect) + 1:]: open(str(tmp_path / name), "rb").read() for name in sorted(os.listdir(str(tmp_path))) if name.startswith(collect + "_")}
    return ev, out, files


def _assert_same_evaluation(dev, host):
    (ev_d, out_d, files_d), (ev_h, out_h, files_h) = dev, host
    got, want = ev_d.prediction_results, ev_h.prediction_results
    assert len(got) == len(want) == N_CLASSES + 1 and sum(len(w) for w in want) > 0
    for c in range(N_CLASSES + 1):
        assert len(got[c]) == len(want[c]), c
        for a, b in zip(got[c], want[c]):
            assert a == b and [type(x) for x in a] == [type(x) for x in b], (c, a, b)
    for name in ("true_positives", "false_positives", "cumulative_true_positives", "cumulative_false_positives", "cumulative_precisions",
                 "cumulative_recalls"):
        for c in range(1, N_CLASSES + 1):
            g, w = np.asarray(getattr(ev_d, name)[c]), np.asarray(getattr(ev_h, name)[c])
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True), (name, c)
    assert np.array_equal(ev_d.num_gt_per_class, ev_h.num_gt_per_class)
    assert out_d[0] == out_h[0] and list(out_d[1]) == list(out_h[1])
    assert files_d == files_h and len(files_d) == N_CLASSES


@pytest.mark.parametrize("round_confidences", [False, 4])
@pytest.mark.parametrize("mode", ["resize", "pad"])
def test_inference_mode_stand_in_model(mode, round_confidences, tmp_path):
    model = _inference_model()
    np.random.seed(3)
    host = _evaluate(model, 'inference', 'host', tmp_path, data_generator_mode=mode, round_confidences=round_confidences)
    np.random.seed(3)
    dev = _evaluate(model, 'inference', 'device', tmp_path, data_generator_mode=mode, round_confidences=round_confidences)
    assert "_device_collection" in dev[0].__dict__ and dev[0].__dict__.get("_packed_pred_memo") is None     # the matcher read the device pack
    _assert_same_evaluation(dev, host)
    assert type(dev[0].prediction_results[1][0][1]) is np.float32


@pytest.mark.parametrize("mode", ["resize", "pad"])
def test_small_ssd7_in_training_mode(mode, tmp_path):
    model = _ssd7()
    kw = dict(size=(76, 68), data_generator_mode=mode, decoding_confidence_thresh=0.05, decoding_top_k=40)
    host = _evaluate(model, 'training', 'host', tmp_path, **kw)
    dev = _evaluate(model, 'training', 'device', tmp_path, **kw)
    _assert_same_evaluation(dev, host)
    assert type(dev[0].prediction_results[1][0][1]) is np.float64
    assert max(len(r) for r in host[0].prediction_results) > 8                    # more than one row per image somewhere


def test_predict_on_dataset_returns_the_lists():
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator
    model = _inference_model()
    want = Evaluator(model, N_CLASSES, _generator()).predict_on_dataset(300, 300, 4, verbose=False, ret=True)
    ev = Evaluator(model, N_CLASSES, _generator())
    assert ev.predict_on_dataset(300, 300, 4, verbose=False, collect='device') is None
    assert ev.__dict__.get("_prediction_results") is None                          # nothing downloaded yet
    got = ev.predict_on_dataset(300, 300, 4, verbose=False, ret=True, collect='device')
    assert got == want and got is ev.prediction_results


def test_refusals_come_before_anything_runs():
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator

    def model(batch):
        raise AssertionError("the model must not run")

    class _Foreign:
        labels, image_ids, eval_neutral = [], [], None

        def generate(self, **kw):
            raise AssertionError("the generator must not run")
    with pytest.raises(ValueError, match="DataGenerator"):
        Evaluator(model, N_CLASSES, _Foreign()).predict_on_dataset(300, 300, 3, verbose=False, collect='device')
    with pytest.raises(ValueError, match="top_k"):
        Evaluator(model, N_CLASSES, _generator(), model_mode='training').predict_on_dataset(300, 300, 3, decoding_top_k='all', verbose=False,
                                                                                           collect='device')
    with pytest.raises(ValueError, match="collect"):
        Evaluator(model, N_CLASSES, _generator()).predict_on_dataset(300, 300, 3, verbose=False, collect='gpu')


def test_an_inverter_without_a_description_is_refused(monkeypatch):
    from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Resize
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator
    real = Resize.__call__

    def undescribed(self, image, labels=None, return_inverter=False):
        out = real(self, image, labels, return_inverter)
        if not return_inverter:
            return out
        inverter = out[-1]
        return tuple(out[:-1]) + (lambda boxes: inverter(boxes),)
    monkeypatch.setattr(Resize, "__call__", undescribed)

    def model(batch):
        raise AssertionError("the model must not run")
    with pytest.raises(ValueError, match="describe"):
        Evaluator(model, N_CLASSES, _generator()).predict_on_dataset(300, 300, 3, verbose=False, collect='device')


def test_a_class_beyond_n_classes_is_an_index_error():
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator
    model = _inference_model(beyond=True)
    with pytest.raises(IndexError):
        Evaluator(model, N_CLASSES, _generator()).predict_on_dataset(300, 300, 3, verbose=False)
    ev = Evaluator(model, N_CLASSES, _generator())
    with pytest.raises(IndexError):
        ev.predict_on_dataset(300, 300, 3, verbose=False, collect='device')
    assert ev.prediction_results is None


def test_assigning_prediction_results_drops_the_device_copy():
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator
    model = _inference_model()
    ev = Evaluator(model, N_CLASSES, _generator())
    ev.predict_on_dataset(300, 300, 3, verbose=False, collect='device')
    first = ev.match_predictions(verbose=False, ret=True)
    results = ev.prediction_results
    # keep the first class only: the matcher must follow the assignment, not the device pack
    ev.prediction_results = [results[0], results[1], [], []]
    assert "_device_collection" not in ev.__dict__
    second = ev.match_predictions(verbose=False, ret=True)
    assert np.array_equal(second[0][1], first[0][1]) and len(first[0][2]) > 0 and len(second[0][2]) == 0 and len(second[0][3]) == 0
    # forget_packed_inputs() keeps the lists and drops the device copy too
    ev.predict_on_dataset(300, 300, 3, verbose=False, collect='device')
    ev.forget_packed_inputs()
    assert "_device_collection" not in ev.__dict__ and ev.prediction_results == results
    third = ev.match_predictions(verbose=False, ret=True)
    for a, b in zip(first, third):
        assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
