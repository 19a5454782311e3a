"""The satellite chain decided on the device: `augment_batch(images, labels, seeds=...)` and the stream mode behind `seeds=None` against
the per-image chain -- pixels, label values and dtypes, np.random's whole MT19937 state (624 words + position) and, in stream mode, the
state of Python's `random`, all exactly.  Images are between 24 x 40 and 96 x 128 (tests/variable_chain_cases.py), out 30 x 36 or
64 x 48, batches of 6 - 8; the seeds were chosen on the CPU so that the chain's own host code takes every branch of the table (asserted
from its trace): no rotation and all three angles, both flips alone and in front of a rotation, and on a ROTATED image patches inside
it, larger than it, and cutting one axis while padding the other."""
import functools
import random

import numpy as np
import pytest

from tests import data_generator_cases as dgc
from tests import satellite_chain_cases as sc


def _shapes(images):
    return [tuple(int(v) for v in im.shape[:2]) for im in images]


@functools.lru_cache(maxsize=None)
def _default_reference():
    """The default configuration on `batch()` under BRANCH_SEEDS, image by image: computed once."""
    images, labels = sc.batch()
    return images, labels, sc.per_image(sc.chain(), images, labels, sc.BRANCH_SEEDS)


def _seeded_equals_the_chain(ch, images, labels, seeds, device_route=True, want=None, as_batch=False):
    import torch
    assert (ch._device_params(labels, shapes=_shapes(images)) is not None) == device_route
    want = sc.per_image(ch, images, labels, seeds) if want is None else want
    before, before_py = np.random.get_state(), random.getstate()
    got_img, got_lab = ch.augment_batch(torch.from_numpy(np.stack(images)).cuda() if as_batch else images, labels, seeds=seeds)
    assert sc.same_state(np.random.get_state(), before), "augment_batch(seeds=...) moved np.random"
    assert random.getstate() == before_py, "augment_batch(seeds=...) moved Python's random"
    assert ch._last_generator_states.shape == (len(seeds), 625) and ch._last_generator_states.dtype == np.uint32
    assert tuple(got_img.shape) == (len(images), ch.resize.out_height, ch.resize.out_width, 3) and got_img.is_cuda
    sc.assert_equal(got_img, got_lab, want, ch._last_generator_states)
    return got_img, got_lab


def _stream_equals_the_loop(ch, images, labels, start, device_route=True, as_batch=False, monkeypatch=None):
    """`start()` puts both generators where the batch begins; the call loop from there is the reference for pixels, labels and where
    both generators end -- for the device route and, with `monkeypatch`, the SSDHIP_AUG_HOST_STREAM=1 route too."""
    import torch
    start()
    want = sc.call_loop(ch, images, labels)
    want_state, want_py = np.random.get_state(), random.getstate()
    assert (ch._device_params(labels, generator=want_state[0], shapes=_shapes(images)) is not None) == device_route
    got_img = None
    for host_path in (("0", "1") if monkeypatch is not None else ("0",)):
        if monkeypatch is not None:
            monkeypatch.setenv("SSDHIP_AUG_HOST_STREAM", host_path)
        start()
        got_img, got_lab = ch.augment_batch(torch.from_numpy(np.stack(images)).cuda() if as_batch else images, labels)
        sc.assert_equal(got_img, got_lab, want)
        got = np.random.get_state()
        assert sc.same_state(got, want_state), (host_path, got[2], want_state[2])
        assert random.getstate() == want_py, "Python's random does not end where the call loop leaves it (route %s)" % host_path
    return got_img


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(10))
def test_the_references_own_cases(k):
    """Each golden satellite case of affine_ops.npz (seeds 740 .. 749) as a batch of one in stream mode: the fixture's image, labels,
    np.random state and `random` state.  In the host loop six of the ten rotate: seeds 740 by 270 degrees, 741, 745 and 748 by 90,
    742 and 746 by 180; 743, 744, 747 and 749 do not."""
    case, img, labels, want = sc.golden_cases()[k]
    ch = sc.chain()
    assert ch._device_params([labels], shapes=[img.shape[:2]]) is not None
    sc.seed_both(case["seed"])
    got_img, got_lab = ch.augment_batch([img], [labels])
    got = got_img.cpu().numpy()
    assert got.shape == (1,) + want["image"].shape and np.array_equal(got[0], want["image"]), case
    assert str(got_lab[0].dtype) == str(want["labels_dtype"]) and got_lab[0].shape == want["labels"].shape, case
    assert np.array_equal(got_lab[0], want["labels"]), (case, got_lab[0], want["labels"])
    assert sc.np_state_digest(sc.state_row(np.random.get_state())) == str(want["np_state"]), case
    assert sc.py_state_digest() == str(want["py_state"]), case


def _start(seed, position):
    sc.seed_both(seed)
    if position is not None:
        st = np.random.get_state()
        np.random.set_state((st[0], st[1], position, 0, 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("position", [None, 621])
def test_stream_mode_on_a_ragged_batch_equals_the_call_loop_and_the_host_path(monkeypatch, position):
    """One generator state for the batch; 621 of 624: the walk crosses mt_twist inside the first image's photometric draws, a draw
    pair straddling it."""
    ch = sc.chain()
    images, labels = sc.batch()
    if position is None:
        _start(sc.BRANCH_STREAM_SEED, None)
        found = sc.branches(sc.trace(ch, _shapes(images), labels))
        assert found >= sc.BRANCHES, sorted(sc.BRANCHES - found)
    _stream_equals_the_loop(ch, images, labels, lambda: _start(sc.BRANCH_STREAM_SEED, position), monkeypatch=monkeypatch)


@pytest.mark.gpu
def test_stream_mode_advances_pythons_generator_by_the_number_of_rotations():
    ch = sc.chain()
    images, labels = sc.batch()
    sc.seed_both(sc.ROTATING_STREAM_SEED)
    angles = [r["angle"] for r in sc.trace(ch, _shapes(images), labels) if r["angle"]]
    assert len(angles) >= 3 and set(angles) == {90, 180, 270}
    _stream_equals_the_loop(ch, images, labels, lambda: sc.seed_both(sc.ROTATING_STREAM_SEED))
    # the generator stands where len(angles) draws of random.choice leave it
    rnd = random.Random(sc.ROTATING_STREAM_SEED)
    assert [rnd.choice(ch.random_rotate.angles) for _ in angles] == angles and random.getstate() == rnd.getstate()


@pytest.mark.gpu
def test_stream_mode_on_a_uniform_cuda_batch_equals_the_call_loop():
    ch = sc.chain(out=(64, 48))
    images, labels = sc.batch(B=6, seed=13, sizes=[(57, 83)])
    sc.seed_both(35)
    assert {r["angle"] for r in sc.trace(ch, _shapes(images), labels)} == {0, 90, 180, 270}
    _stream_equals_the_loop(ch, images, labels, lambda: sc.seed_both(35), as_batch=True)


@pytest.mark.gpu
def test_seeded_mode_on_a_ragged_list_takes_every_branch_and_equals_the_chain():
    images, labels, want = _default_reference()
    ch = sc.chain()
    found = sc.branches(sc.trace(ch, _shapes(images), labels, sc.BRANCH_SEEDS))
    assert found >= sc.BRANCHES, sorted(sc.BRANCHES - found)
    _seeded_equals_the_chain(ch, images, labels, sc.BRANCH_SEEDS, want=want)


@pytest.mark.gpu
def test_seeded_mode_does_not_depend_on_the_order_of_the_batch():
    images, labels, want = _default_reference()
    order = np.random.RandomState(3).permutation(len(labels))
    assert not np.array_equal(order, np.arange(len(labels)))
    _seeded_equals_the_chain(sc.chain(), [images[i] for i in order], [labels[i] for i in order], [sc.BRANCH_SEEDS[i] for i in order],
                             want=[want[i] for i in order])


@pytest.mark.gpu
def test_seeded_mode_on_a_uniform_cuda_batch():
    images, labels = sc.batch(B=6, seed=13, sizes=[(57, 83)])
    ch = sc.chain(out=(64, 48))
    seeds = list(range(300, 306))
    rows = sc.trace(ch, _shapes(images), labels, seeds)
    assert {r["angle"] for r in rows} >= {0, 90} and len({r["angle"] for r in rows}) >= 3, rows
    _seeded_equals_the_chain(ch, images, labels, seeds, as_batch=True)


@pytest.mark.gpu
def test_a_configuration_off_the_defaults():
    """Always flipped both ways and turned by 270 degrees, a patch background that is not black, whole-valued float64 labels in a
    permuted column order: the rotation's black border and the patch's coloured padding in one image."""
    colour = (12, 200, 7)
    ch = sc.chain(random_flip=1.0, random_rotate=([270], 1.0), labels_format={'class_id': 4, 'xmin': 2, 'ymin': 0, 'xmax': 3, 'ymax': 1})
    ch.random_patch.sample_patch.background = colour
    images, labels = sc.batch()
    images = [np.maximum(im, 1) for im in images]             # no black source pixels: black can only be the rotation's border
    labels = [lab[:, [2, 4, 1, 3, 0]].astype(np.float64) for lab in labels]
    rows = sc.trace(ch, _shapes(images), labels, sc.BRANCH_SEEDS)
    assert all(r["angle"] == 270 and r["hflip"] and r["vflip"] for r in rows)
    # images whose patch begins left of the rotated image: it pads there AND takes in column 0, which a turn by 270 degrees leaves black
    both = [i for i, r in enumerate(rows) if r["patch"] is not None and r["patch"][1] < 0]
    assert both, rows
    got_img, got_lab = _seeded_equals_the_chain(ch, images, labels, sc.BRANCH_SEEDS)
    assert all(lab.dtype == np.float64 for lab in got_lab)
    px = got_img.cpu().numpy()
    assert all((px[i].reshape(-1, 3) == np.array(colour, dtype=np.uint8)).all(axis=1).any() for i in both)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fractional_labels", "narrow_image"])
def test_what_the_kernel_does_not_cover_falls_back_with_the_same_results(case):
    images, labels = sc.batch()
    if case == "fractional_labels":
        labels = [lab.astype(np.float64) + np.array([[0.0, 0.25, 0.5, 0.75, 0.5]]) for lab in labels]
    else:
        images = list(images)
        images[3] = np.ascontiguousarray(images[3][:, :3])      # 57 x 3
        labels = [lab.copy() for lab in labels]
        labels[3] = np.array([[5, 0, 10, 2, 40]], dtype=np.int64)
    ch = sc.chain()
    _stream_equals_the_loop(ch, images, labels, lambda: sc.seed_both(sc.ROTATING_STREAM_SEED), device_route=False)
    _seeded_equals_the_chain(ch, images, labels, sc.BRANCH_SEEDS, device_route=False)


@pytest.mark.gpu
def test_data_generator_takes_the_route_by_itself(monkeypatch):
    """generate() with [DataAugmentationSatellite] on the fixture images (mixed sizes, one grey, one RGBA): one decision launch for
    the batch, and the batch and the final states of both generators that the chain's `__call__` gives over the same items in a loop."""
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import object_detection_2d_data_generator as dg
    launches = []
    real = nat.sat_augment_decide
    monkeypatch.setattr(nat, "sat_augment_decide", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    g = dgc.csv_generator(dg)
    ch = sc.chain()
    gen = g.generate(batch_size=8, shuffle=False, transformations=[ch],
                     returns={'processed_images', 'processed_labels', 'original_images', 'original_labels'}, keep_images_without_gt=True)
    sc.seed_both(77)
    got_x, got_y, items, item_labels = next(gen)
    got_state, got_py = np.random.get_state(), random.getstate()
    assert len(launches) == 1 and len(items) == 8 and {im.ndim for im in items} == {2, 3} and {im.shape[-1] for im in items} >= {3, 4}
    assert dg.DataGenerator._batch_path([ch], items, True) == 'satellite' and dg.DataGenerator._batch_path([ch], items, False) is None
    sc.seed_both(77)
    want = [sc.chain()(im, np.asarray(lab)) for im, lab in zip(items, item_labels)]
    assert sc.same_state(np.random.get_state(), got_state) and random.getstate() == got_py
    got_x = np.asarray(got_x)
    assert got_x.shape == (8,) + sc.OUT + (3,) and len(got_y) == 8
    for i, (px, lb) in enumerate(want):
        assert np.array_equal(got_x[i], px), i
        assert np.asarray(got_y[i]).dtype == lb.dtype and np.array_equal(got_y[i], lb), (i, got_y[i], lb)
