"""The NumPy statement of the collection kernels (tests/np_eval_collect.py) against the Evaluator's host route -- `_collect_batch`, the
loop body of `predict_on_dataset`, and `_packed_predictions` -- on inverters the real `Resize` / `RandomPadFixedAR` host code makes for
the images of tests/data_generator_cases.py.  No GPU: the transforms run on lazy images, as in the generator's batch paths, and the one
upload of `_packed_predictions` is replaced by the identity.  All comparisons are exact, element types included."""
import numpy as np
import pytest

from ssd_keras_amd import _native as nat
from ssd_keras_amd.data_generator import _image_ops as iop
from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Resize
from ssd_keras_amd.data_generator.object_detection_2d_patch_sampling_ops import RandomPadFixedAR
from ssd_keras_amd.data_generator.object_detection_2d_photometric_ops import ConvertTo3Channels
from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator, _DeviceCollection
from tests import data_generator_cases as dc
from tests import np_eval_collect as ref

N_CLASSES, OUT_H, OUT_W, R = 5, 30, 40, 7
IDS = ['a', 'b', 'c', 'b', 'e', 'f', 'g', 'h']                  # a duplicate id: its rows take the LAST index, as `_image_index` does


class _Dataset:
    def __init__(self, image_ids):
        self.image_ids, self.labels, self.eval_neutral = image_ids, [np.zeros((0, 5))] * len(image_ids), None


def inverters_of(mode):
    """Per image of dc.IMAGES the inverters of the evaluation's transformation list, the last applied first (the generator's `_walk`)."""
    np.random.seed(11)
    chain = [ConvertTo3Channels()] + ([RandomPadFixedAR(patch_aspect_ratio=OUT_W / OUT_H)] if mode == 'pad' else []) + [Resize(OUT_H, OUT_W)]
    takes = DataGenerator._takes_inverter(chain, True)
    return [DataGenerator._walk(chain, iop.GeoImage.of(shape[0], shape[1]), None, takes)[2] for _, shape in dc.IMAGES]


def make_rows(dtype, classes, seed):
    """(8, R, 6) rows in the resized frame: fractional coordinates, some outside the image; image 2 without rows; class-0 rows in the middle."""
    rng = np.random.RandomState(seed)
    rows = np.zeros((len(IDS), R, 6), dtype=np.float64)
    rows[:, :, 0] = rng.choice(classes, size=(len(IDS), R))
    rows[:, :, 1] = rng.uniform(0.0, 1.0, size=(len(IDS), R))
    rows[:, :, 2:] = rng.uniform(-5.0, 45.0, size=(len(IDS), R, 4))
    rows[:, 3, 0] = 0                                            # padding in the middle of every image
    rows[2, :, 0] = 0
    return rows.astype(dtype)


def host_lists(rows, count, inverters, round_confidences):
    """The oracle: the host route's per-class lists, the batch cut as `predict_on_dataset` / `_to_list` cut it."""
    ev = Evaluator(None, N_CLASSES, _Dataset(IDS))
    if count is None:
        per_image = [rows[i][rows[i, :, 0] != 0] for i in range(len(rows))]
    else:
        per_image = [rows[i, :count[i]].copy() if count[i] else np.array([]) for i in range(len(rows))]
    results = [list() for _ in range(N_CLASSES + 1)]
    ev._collect_batch(results, per_image, IDS, inverters, round_confidences)
    return ev, results


def stated_store(rows, count, inverters, round_confidences, splits=(3, 8)):
    """The statement: the batch appended in two calls."""
    index_of = {str(v): i for i, v in enumerate(IDS)}
    store = ref.new_store(len(IDS) * R, rows.dtype, N_CLASSES)
    lo = 0
    for hi in splits:
        desc = ref.make_desc([index_of[str(v)] for v in IDS[lo:hi]], [_DeviceCollection.program(inv) for inv in inverters[lo:hi]])
        ref.collect(store, rows[lo:hi], None if count is None else count[lo:hi], desc, len(IDS), N_CLASSES, 1, int(round_confidences or 0))
        lo = hi
    return store


def lists_of(store):
    rows, image, cls = store["rows"][:store["n"]], store["image"][:store["n"]], store["rows"][:store["n"], 0].astype(np.int64)
    return [list()] + [list(zip([IDS[i] for i in image[cls == c]], *(rows[cls == c][:, j] for j in range(1, 6)))) for c in range(1, N_CLASSES + 1)]


def assert_same_lists(got, want):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), c
        for a, b in zip(g, w):
            assert a == b, (c, a, b)
            assert [type(x) for x in a] == [type(x) for x in b], (c, a, b)


@pytest.mark.parametrize("round_confidences", [False, 4])
@pytest.mark.parametrize("rule", ["class", "count"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", ["resize", "pad"])
def test_statement_equals_the_host_route(mode, dtype, rule, round_confidences, monkeypatch):
    inverters = inverters_of(mode)
    assert all(len(inv) == (2 if mode == 'pad' else 1) for inv in inverters)
    rows = make_rows(dtype, [0, 2, 4], seed=3)                    # classes 1, 3 and 5 stay empty: first, middle, last
    count = None
    if rule == "count":
        count = np.array([R, 1, 0, 5, R, 2, 0, 3], dtype=np.int32)
        rows[:, :, 0] = np.where(rows[:, :, 0] == 0, 2, rows[:, :, 0])        # the decoder emits no class 0
    ev, want = host_lists(rows, count, inverters, round_confidences)
    store = stated_store(rows, count, inverters, round_confidences)
    assert store["overflow"] == 0 and store["bad"] == 0
    assert store["n"] == sum(len(w) for w in want) and list(store["class_count"]) == [len(w) for w in want[1:]]
    assert_same_lists(lists_of(store), want)
    assert not want[1] and want[2] and not want[3] and want[4] and not want[5]
    # pack == what `_packed_predictions` builds from the host lists (its upload replaced by the identity)
    import torch
    monkeypatch.setattr(nat, "to_device", lambda a, device=None, dtype=None: a)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    ev.prediction_results = want
    memo = ev._packed_predictions()
    pred, segment, slot, starts = ref.pack(store["rows"], store["image"], store["n"], len(IDS), N_CLASSES)
    for got, key in ((pred, "pred"), (segment, "segment"), (slot, "slot"), (starts, "starts")):
        assert got.dtype == memo[key].dtype and np.array_equal(got, memo[key]), key
    assert np.array_equal(starts, memo["starts_host"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_predictions_at_all(dtype, monkeypatch):
    inverters = inverters_of('resize')
    rows = make_rows(dtype, [0], seed=4)
    ev, want = host_lists(rows, None, inverters, False)
    store = stated_store(rows, None, inverters, False)
    assert store["n"] == 0 and not any(want)
    pred, segment, slot, starts = ref.pack(store["rows"], store["image"], 0, len(IDS), N_CLASSES)
    assert pred.shape == (0, 5) and segment.shape == (0,) and slot.shape == (0,) and not starts.any() and starts.shape == (N_CLASSES + 1,)


def test_out_of_range_classes_and_overflow_are_counted():
    inverters = inverters_of('resize')
    rows = make_rows(np.float64, [0, 2, N_CLASSES + 1], seed=5)
    with pytest.raises(IndexError):
        host_lists(rows, None, inverters, False)                  # the host route's `results[class_id]`
    store = stated_store(rows, None, inverters, False)
    assert store["bad"] == int((rows[:, :, 0] == N_CLASSES + 1).sum()) > 0
    pred, segment, slot, starts = ref.pack(store["rows"], store["image"], store["n"], len(IDS), N_CLASSES)
    assert pred.shape[0] == starts[-1] == store["n"] - store["bad"] and set(slot) == {1}
    small = ref.new_store(3, np.float64, N_CLASSES, fill=-1.0)
    ref.collect(small, rows[:1], None, ref.make_desc([0], [[]]), len(IDS), N_CLASSES)
    assert small["overflow"] == 1 and small["n"] == 0 and (small["rows"] == -1.0).all()


def test_round_is_numpy_scalar_round():
    """The rounding the statement and the kernels use is `round()` of a NumPy scalar, bit for bit, in both dtypes."""
    rng = np.random.RandomState(6)
    for dtype in (np.float32, np.float64):
        values = np.concatenate([rng.uniform(-500, 500, 4000), rng.uniform(0, 1, 4000), np.arange(-50, 50) + 0.05, np.arange(-50, 50) + 0.25]).astype(dtype)
        for decimals in (1, 4):
            want = np.array([round(v, decimals) for v in values])
            assert want.dtype == dtype and np.array_equal(ref._round(values, decimals), want)


def test_programs_of_the_inverters():
    (resize,), (resize_p, shift_p) = inverters_of('resize')[1], inverters_of('pad')[1]
    h, w = dc.IMAGES[1][1][:2]
    assert _DeviceCollection.program([resize]) == [(nat.EVAL_SCALE, h / OUT_H, w / OUT_W)]
    steps = _DeviceCollection.program([resize_p, None, shift_p])
    assert [s[0] for s in steps] == [nat.EVAL_SCALE, nat.EVAL_SHIFT] and steps[1][1:] == (0.0, float(shift_p.step[2]))
    with pytest.raises(ValueError):
        _DeviceCollection.program([lambda boxes: boxes])
    with pytest.raises(ValueError):
        _DeviceCollection.program([resize] * 5)
