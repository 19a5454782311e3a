"""The variable-input-size chain decided on the device: `augment_batch(images, labels, seeds=...)` and the stream mode behind
`seeds=None` against the per-image chain -- pixels, label values and dtypes and the whole MT19937 state (624 words + position), all
exactly.  Images are between 24 x 40 and 96 x 128 (tests/variable_chain_cases.py), out 30 x 36 or 64 x 48, batches of 6 - 8; the seeds
were chosen on the CPU so that the chain's own host code takes every branch of the table (asserted from its trace): patches inside the
image, larger than it, and cutting one axis while padding the other -- windows no caller had sent to the plan kernel before."""
import functools

import numpy as np
import pytest

from tests import variable_chain_cases as vc


def _shapes(images):
    return [tuple(int(v) for v in im.shape[:2]) for im in images]


@functools.lru_cache(maxsize=None)
def _default_reference():
    """The default configuration on `batch()` under BRANCH_SEEDS, image by image: computed once."""
    images, labels = vc.batch()
    return images, labels, vc.per_image(vc.chain(), images, labels, vc.BRANCH_SEEDS)


def _seeded_equals_the_chain(ch, images, labels, seeds, device_route=True, want=None, as_batch=False):
    import torch
    assert (ch._device_params(labels, shapes=_shapes(images)) is not None) == device_route
    want = vc.per_image(ch, images, labels, seeds) if want is None else want
    before = np.random.get_state()
    got_img, got_lab = ch.augment_batch(torch.from_numpy(np.stack(images)).cuda() if as_batch else images, labels, seeds=seeds)
    assert vc.same_state(np.random.get_state(), before), "augment_batch(seeds=...) moved the global generator"
    assert ch._last_generator_states.shape == (len(seeds), 625) and ch._last_generator_states.dtype == np.uint32
    assert tuple(got_img.shape) == (len(images), ch.resize.out_height, ch.resize.out_width, 3) and got_img.is_cuda
    vc.assert_equal(got_img, got_lab, want, ch._last_generator_states)
    return got_img, got_lab


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(10))
def test_the_references_own_cases(k):
    """Each golden variable-chain case of affine_ops.npz as a batch of one: the fixture's image, labels and np.random state."""
    case, img, labels, want = vc.golden_cases()[k]
    ch = vc.chain()
    assert ch._device_params([labels], shapes=[img.shape[:2]]) is not None
    np.random.seed(case["seed"])
    got_img, got_lab = ch.augment_batch([img], [labels])
    got = got_img.cpu().numpy()
    assert got.shape == (1,) + want["image"].shape and np.array_equal(got[0], want["image"]), case
    assert str(got_lab[0].dtype) == str(want["labels_dtype"]) and got_lab[0].shape == want["labels"].shape, case
    assert np.array_equal(got_lab[0], want["labels"]), (case, got_lab[0], want["labels"])
    assert vc.np_state_digest(vc.state_row(np.random.get_state())) == str(want["np_state"]), case


def _start(seed, position):
    np.random.seed(seed)
    if position is not None:
        st = np.random.get_state()
        np.random.set_state((st[0], st[1], position, 0, 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("position", [None, 621])
def test_stream_mode_on_a_ragged_batch_equals_the_call_loop_and_the_host_path(monkeypatch, position):
    """One generator state for the batch; 621 of 624: the walk crosses mt_twist inside the first image's photometric draws, a draw
    pair straddling it."""
    ch = vc.chain()
    images, labels = vc.batch()
    _start(vc.BRANCH_STREAM_SEED, position)
    if position is None:
        found = vc.branches(vc.trace(ch, _shapes(images), labels))
        assert found >= vc.BRANCHES, sorted(vc.BRANCHES - found)
    want = vc.call_loop(ch, images, labels)
    want_state = np.random.get_state()
    assert ch._device_params(labels, generator=want_state[0], shapes=_shapes(images)) is not None
    for host_path in ("0", "1"):
        monkeypatch.setenv("SSDHIP_AUG_HOST_STREAM", host_path)
        _start(vc.BRANCH_STREAM_SEED, position)
        got_img, got_lab = ch.augment_batch(images, labels)
        vc.assert_equal(got_img, got_lab, want)
        got = np.random.get_state()
        assert vc.same_state(got, want_state), (host_path, got[2], want_state[2])


@pytest.mark.gpu
def test_stream_mode_on_a_uniform_cuda_batch_equals_the_call_loop():
    import torch
    ch = vc.chain(out=(64, 48))
    images, labels = vc.batch(B=6, seed=13, sizes=[(57, 83)])
    np.random.seed(31)
    want = vc.call_loop(ch, images, labels)
    want_state = np.random.get_state()
    np.random.seed(31)
    got_img, got_lab = ch.augment_batch(torch.from_numpy(np.stack(images)).cuda(), labels)
    vc.assert_equal(got_img, got_lab, want)
    assert vc.same_state(np.random.get_state(), want_state)


@pytest.mark.gpu
def test_seeded_mode_on_a_ragged_list_takes_every_branch_and_equals_the_chain():
    images, labels, want = _default_reference()
    ch = vc.chain()
    rows = vc.trace(ch, _shapes(images), labels, vc.BRANCH_SEEDS)
    found = vc.branches(rows)
    assert found >= vc.BRANCHES, sorted(vc.BRANCHES - found)
    _seeded_equals_the_chain(ch, images, labels, vc.BRANCH_SEEDS, want=want)


@pytest.mark.gpu
def test_seeded_mode_does_not_depend_on_the_order_of_the_batch():
    images, labels, want = _default_reference()
    order = np.random.RandomState(3).permutation(len(labels))
    assert not np.array_equal(order, np.arange(len(labels)))
    _seeded_equals_the_chain(vc.chain(), [images[i] for i in order], [labels[i] for i in order], [vc.BRANCH_SEEDS[i] for i in order],
                             want=[want[i] for i in order])


@pytest.mark.gpu
def test_seeded_mode_on_a_uniform_cuda_batch():
    images, labels = vc.batch(B=6, seed=13, sizes=[(57, 83)])
    ch = vc.chain(out=(64, 48))
    seeds = list(range(300, 306))
    kinds = {r["kind"] for r in vc.trace(ch, _shapes(images), labels, seeds)}
    assert len(kinds - {None}) >= 2, kinds
    _seeded_equals_the_chain(ch, images, labels, seeds, as_batch=True)


@pytest.mark.gpu
def test_every_trial_rejected_leaves_image_and_labels_unaltered():
    images, labels = vc.batch()
    ch = vc.chain(bounds_validator=(0.99, 1.0))
    rows = vc.trace(ch, _shapes(images), labels, vc.UNALTERED_SEEDS)
    assert rows[6]["unaltered"] and not all(r["unaltered"] for r in rows), rows
    _seeded_equals_the_chain(ch, images, labels, vc.UNALTERED_SEEDS)


def _many_boxes(n, h, w, seed):
    rng = np.random.RandomState(seed)
    bw, bh = rng.randint(2, w // 3, size=n), rng.randint(2, h // 3, size=n)
    x0, y0 = rng.randint(0, w - bw), rng.randint(0, h - bh)
    return np.stack([rng.randint(1, 21, size=n), x0, y0, x0 + bw, y0 + bh], axis=1).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["int64", "float64", "permuted", "no_boxes", "max_boxes", "one_too_many"])
def test_label_layouts(layout):
    from ssd_keras_amd import _native as nat
    images, labels = vc.batch()
    labels = [lab.copy() for lab in labels]
    ch, device_route = vc.chain(), True
    if layout == "float64":
        labels = [lab.astype(np.float64) + np.array([[0.0, 0.25, 0.5, 0.75, 0.5]]) for lab in labels]
    elif layout == "permuted":
        ch = vc.chain(labels_format={'class_id': 4, 'xmin': 2, 'ymin': 0, 'xmax': 3, 'ymax': 1})
        labels = [lab[:, [2, 4, 1, 3, 0]] for lab in labels]
    elif layout == "no_boxes":
        labels[1] = np.zeros((0, 5), dtype=np.int64)
        labels[6] = np.zeros((0, 5), dtype=np.int64)
    elif layout == "max_boxes":
        labels[1] = _many_boxes(nat.AUG_MAX_BOXES, 96, 128, 5)
        labels[7] = _many_boxes(nat.AUG_MAX_BOXES, 77, 120, 6)
    elif layout == "one_too_many":
        labels[1] = _many_boxes(nat.AUG_MAX_BOXES + 1, 96, 128, 5)
        device_route = False
    _, got_lab = _seeded_equals_the_chain(ch, images, labels, vc.BRANCH_SEEDS, device_route)
    if layout == "no_boxes":                                  # n_boxes_min = 1: an image without boxes never validates
        rows = vc.trace(ch, _shapes(images), labels, vc.BRANCH_SEEDS)
        assert rows[1]["unaltered"] and rows[6]["unaltered"] and got_lab[1].shape == (0, 5) and got_lab[6].shape == (0, 5)
    elif layout == "max_boxes":
        assert any(len(lab) > 16 for lab in got_lab)


PARAMETERS = {
    "iou": dict(overlap_criterion='iou', bounds_validator=(0.02, 1.0), bounds_box_filter=(0.01, 1.0)),
    "center_point": dict(overlap_criterion='center_point'),
    "two_boxes": dict(n_boxes_min=2, bounds_validator=(0.3, 1.0)),
    "all_boxes": dict(n_boxes_min='all', bounds_validator=(0.1, 1.0)),
    "strict_lower_bound": dict(bounds_box_filter=(0.0, 1.0)),
    "no_clip": dict(clip_boxes=False),
    "no_trials": dict(n_trials_max=0),
    "one_trial": dict(n_trials_max=1),
    "never_flip": dict(random_flip=0.0),
    "always_flip": dict(random_flip=1.0),
    "background": dict(background=(12, 200, 7)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PARAMETERS))
def test_parameters_off_the_defaults(name):
    images, labels = vc.batch()
    ch = vc.chain(out=(64, 48) if name in ("iou", "no_clip") else vc.OUT, **PARAMETERS[name])
    if name == "background":
        # (the constructor's colour never reaches RandomPatch, as in the reference; the patch's own colour is what pads)
        ch.random_patch.sample_patch.background = (12, 200, 7)
    elif name == "all_boxes":
        labels = [lab.copy() for lab in labels]
        labels[2] = np.zeros((0, 5), dtype=np.int64)          # 'all' of no boxes: every patch validates
    rows = vc.trace(ch, _shapes(images), labels, vc.BRANCH_SEEDS)
    if name == "all_boxes":
        assert not rows[2]["unaltered"]
    elif name == "background":
        assert any(r["kind"] in ("larger", "crop_y_pad_x", "pad_y_crop_x") for r in rows)
    elif name in ("never_flip", "always_flip"):
        assert {r["flipped"] for r in rows} == {name == "always_flip"}
    elif name in ("no_trials", "one_trial"):
        assert {r["trial"] for r in rows} <= {0, 1} and any(r["unaltered"] for r in rows) and not all(r["unaltered"] for r in rows)
    got_img, _ = _seeded_equals_the_chain(ch, images, labels, vc.BRANCH_SEEDS)
    if name == "background":
        px = got_img.cpu().numpy().reshape(-1, 3)
        assert (px == np.array([12, 200, 7], dtype=np.uint8)).all(axis=1).any()


@pytest.mark.gpu
def test_data_generator_takes_the_route_by_itself(monkeypatch):
    """generate() with [DataAugmentationVariableInputSize] on a dataset of mixed sizes with one greyscale image: one decision launch
    per batch, and the batches and the final np.random state of the per-image loop."""
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    images, labels = vc.batch()
    images = list(images)
    images[2] = np.ascontiguousarray(images[2][:, :, 1])      # greyscale
    launches = []
    real = nat.var_augment_decide
    monkeypatch.setattr(nat, "var_augment_decide", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    runs = {}
    for route in ("batch", "loop"):
        if route == "loop":
            monkeypatch.setattr(DataGenerator, "_batch_path", staticmethod(lambda transformations, images, have_labels: None))
        g = DataGenerator(labels=[lab.copy() for lab in labels], verbose=False)
        g.images, g.dataset_size, g.dataset_indices = [im for im in images], 8, np.arange(8, dtype=np.int32)
        gen = g.generate(batch_size=4, shuffle=False, transformations=[vc.chain()], returns={'processed_images', 'processed_labels'},
                         keep_images_without_gt=True)
        del launches[:]
        np.random.seed(77)
        batches = [next(gen) for _ in range(3)]              # the third wraps into the second epoch
        assert len(launches) == (3 if route == "batch" else 0)
        runs[route] = (batches, np.random.get_state())
    (dev, dev_state), (host, host_state) = runs["batch"], runs["loop"]
    assert vc.same_state(dev_state, host_state)
    for (dx, dy), (hx, hy) in zip(dev, host):
        assert np.asarray(dx).shape == (4,) + vc.OUT + (3,) and np.array_equal(np.asarray(dx), np.asarray(hx))
        assert len(dy) == len(hy) == 4
        for a, b in zip(dy, hy):
            assert a.dtype == b.dtype and np.array_equal(a, b)
