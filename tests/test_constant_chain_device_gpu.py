"""The constant-input-size chain (SSD7's notebook chain) decided on the device: `augment_batch(images, labels, seeds=...)` and the stream
mode behind `seeds=None` against the per-image chain -- pixels, labels, label dtypes and MT19937 states, all exactly -- and the plan kernel
against `_image_ops.WarpImage.plan()`.  Images are 60 x 96 except where a size is named: small enough to be quick, large enough that
`min_area = 16` and the 0.03 ... 0.5 translations bite."""
import functools

import numpy as np
import pytest

from tests import np_const_plans as ncp
from tests.test_constant_chain_device_cpu import NOTEBOOK

H, W = 60, 96
SEEDS = list(range(100, 132))


def _chain(**kw):
    from ssd_keras_amd.data_generator.data_augmentation_chain_constant_input_size import DataAugmentationConstantInputSize
    return DataAugmentationConstantInputSize(**dict(NOTEBOOK, **kw))


def _batch(B=32, h=H, w=W, seed=9):
    """test_affine_ops_gpu._notebook_batch's labels scaled from 300 x 480 to h x w: every fourth image holds one small box in a corner
    (most translations / zooms lose it, so every trial fails), the others one to five boxes anywhere."""
    s = w / 480.0
    cw, ch, bw, bh = int(round(40 * s)), int(round(30 * s)), int(round(120 * s)), int(round(90 * s))
    rng = np.random.RandomState(seed)
    images = rng.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)
    labels = []
    for i in range(B):
        if i % 4 == 3:
            labels.append(np.array([[rng.randint(1, 6), 0, 0, cw, ch]]) + np.array([[0, w - cw - 1, h - ch - 1, w - cw - 1, h - ch - 1]]) * (i % 8 == 7))
            continue
        n = rng.randint(1, 6)
        x0, y0 = rng.randint(0, w - bw, size=n), rng.randint(0, h - bh, size=n)
        labels.append(np.stack([rng.randint(1, 6, size=n), x0, y0, x0 + rng.randint(max(2, int(8 * s)), bw, size=n),
                                y0 + rng.randint(max(2, int(6 * s)), bh, size=n)], axis=1))
    return images, labels


def _state_row(st):
    return np.concatenate([np.asarray(st[1], dtype=np.uint32), np.array([st[2]], dtype=np.uint32)])


def _per_image(chain, images, labels, seeds):
    """[(pixels, labels, generator state (625,))] of `np.random.seed(s); chain(image, labels)`; the global generator is put back."""
    saved = np.random.get_state()
    out = []
    for img, lab, s in zip(images, labels, seeds):
        np.random.seed(s)
        px, lb = chain(img, lab)
        out.append((px, lb, _state_row(np.random.get_state())))
    np.random.set_state(saved)
    return out


def _assert_equal(got_img, got_lab, want, states=None):
    g = got_img.cpu().numpy()
    assert g.dtype == np.uint8 and len(got_lab) == len(want) == g.shape[0]
    for i, (px, lb, st) in enumerate(want):
        assert np.array_equal(g[i], px), "image %d: %d pixels differ" % (i, int((g[i] != px).sum()))
        assert got_lab[i].dtype == lb.dtype and got_lab[i].shape == lb.shape and np.array_equal(got_lab[i], lb), (i, got_lab[i], lb)
        if states is not None:
            assert np.array_equal(states[i], st), "image %d: generator state differs (position %d, want %d)" % (i, states[i][624], st[624])


def _seeded_equals_the_chain(chain, images, labels, seeds, device_route=True):
    import torch
    assert (chain._device_params(labels) is not None) == device_route
    want = _per_image(chain, images, labels, seeds)
    before = np.random.get_state()
    got_img, got_lab = chain.augment_batch(torch.from_numpy(images).cuda(), labels, seeds=seeds)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert chain._last_generator_states.shape == (len(seeds), 625) and chain._last_generator_states.dtype == np.uint32
    _assert_equal(got_img, got_lab, want, chain._last_generator_states)
    return got_img, got_lab


def _trace(chain, labels, seeds, h=H, w=W):
    """What the per-image chain's own ops do to each image under its seed, observed on lazy images: sequence, translated?, zoomed?,
    flipped?, and how many trial loops gave up."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    validator = type(chain.image_validator)
    real, results = validator.__call__, []

    def watched(self, labels, image_height, image_width):
        ok = real(self, labels, image_height, image_width)
        results.append(ok)
        return ok

    saved, rows = np.random.get_state(), []
    validator.__call__ = watched
    try:
        chain._sync_formats()
        n_trials = max(1, chain.n_trials_max)
        for lab, s in zip(labels, seeds):
            np.random.seed(s)
            del results[:]
            seq, _, geometric = chain._draw()
            img = iop.WarpImage.of(h, w)
            for t in geometric:
                img, lab = t(img, lab)
            gave_up, k = 0, 0
            while k < len(results):                          # a loop ends at its first valid trial or after n_trials failures
                run = results[k:k + n_trials]
                if True in run:
                    k += run.index(True) + 1
                else:
                    gave_up += len(run) == n_trials
                    k += len(run)
            zoomed = img.M is not None and not np.array_equal(img.M, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
            translated = img.pre != (0, 0) or img.post not in (None, (0, 0))
            rows.append(dict(seq=seq, translated=translated, zoomed=zoomed, flipped=img.flip, gave_up=gave_up))
    finally:
        validator.__call__ = real
        np.random.set_state(saved)
    return rows


@functools.lru_cache(maxsize=None)
def _notebook_run():
    """The B = 32 run of the notebook's arguments under SEEDS, computed once: (images, labels, per-image reference, device results)."""
    import torch
    chain = _chain()
    images, labels = _batch()
    want = _per_image(chain, images, labels, SEEDS)
    before = np.random.get_state()
    got_img, got_lab = chain.augment_batch(torch.from_numpy(images).cuda(), labels, seeds=SEEDS)
    after = np.random.get_state()
    untouched = before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    return images, labels, want, got_img, got_lab, chain._last_generator_states.copy(), untouched


@pytest.mark.gpu
def test_seeded_mode_equals_the_per_image_chain():
    chain = _chain()
    images, labels, want, got_img, got_lab, states, untouched = _notebook_run()
    assert chain._device_params(labels) is not None
    assert untouched, "augment_batch(seeds=...) moved the global generator"
    assert states.shape == (32, 625) and states.dtype == np.uint32
    _assert_equal(got_img, got_lab, want, states)
    rows = _trace(chain, labels, SEEDS)
    assert {r["seq"] for r in rows} == {1, 2}, rows
    assert any(r["flipped"] for r in rows), rows
    assert any(r["translated"] and not r["zoomed"] for r in rows), rows
    assert any(r["zoomed"] and not r["translated"] for r in rows), rows
    assert any(r["zoomed"] and r["translated"] for r in rows), rows
    assert any(r["gave_up"] for r in rows), rows


@pytest.mark.gpu
def test_seeded_mode_does_not_depend_on_the_order_of_the_batch():
    import torch
    images, labels, want, _, _, _, _ = _notebook_run()
    order = np.random.RandomState(3).permutation(len(labels))
    assert not np.array_equal(order, np.arange(len(labels)))
    chain = _chain()
    got_img, got_lab = chain.augment_batch(torch.from_numpy(images[order]).cuda(), [labels[i] for i in order], seeds=[SEEDS[i] for i in order])
    _assert_equal(got_img, got_lab, [want[i] for i in order], chain._last_generator_states)


def _start(position):
    np.random.seed(2024)
    if position is not None:
        st = np.random.get_state()
        np.random.set_state((st[0], st[1], position, 0, 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("position", [None, 621])
def test_stream_mode_equals_the_call_loop_and_the_host_loop(monkeypatch, position):
    """Two batches in a row from one generator state; 621 of 624: the walk crosses mt_twist three draws into the first image."""
    import torch
    chain = _chain()
    images, labels = _batch(B=16, seed=11)
    _start(position)
    want = []
    for i in range(16):
        px, lb = chain(images[i], labels[i])
        want.append((px, lb, None))
    want_state = np.random.get_state()
    assert chain._device_params(labels, generator=want_state[0]) is not None
    for host_loop in ("0", "1"):
        monkeypatch.setenv("SSDHIP_AUG_HOST_STREAM", host_loop)
        _start(position)
        for lo in (0, 8):
            got_img, got_lab = chain.augment_batch(torch.from_numpy(images[lo:lo + 8]).cuda(), labels[lo:lo + 8])
            _assert_equal(got_img, got_lab, want[lo:lo + 8])
        got = np.random.get_state()
        assert got[0] == want_state[0] and np.array_equal(got[1], want_state[1]) and got[2:] == want_state[2:], (host_loop, got[2], want_state[2])


def _many_boxes(n, seed):
    rng = np.random.RandomState(seed)
    x0, y0 = rng.randint(0, W - 24, size=n), rng.randint(0, H - 18, size=n)
    return np.stack([rng.randint(1, 6, size=n), x0, y0, x0 + rng.randint(2, 24, size=n), y0 + rng.randint(2, 18, size=n)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["int64", "float64", "permuted", "no_boxes", "max_boxes", "one_too_many"])
def test_label_layouts(layout):
    from ssd_keras_amd import _native as nat
    images, labels = _batch(B=8, seed=21)
    chain, device_route = _chain(), True
    if layout == "float64":
        labels = [lab.astype(np.float64) + np.array([[0.0, 0.25, 0.5, 0.75, 0.5]]) for lab in labels]
    elif layout == "permuted":
        chain = _chain(labels_format={'class_id': 4, 'xmin': 2, 'ymin': 0, 'xmax': 3, 'ymax': 1})
        labels = [lab[:, [2, 4, 1, 3, 0]] for lab in labels]
    elif layout == "no_boxes":
        labels[1] = np.zeros((0, 5), dtype=np.int64)
        labels[6] = np.zeros((0, 5), dtype=np.int64)
    elif layout == "max_boxes":
        labels[2] = _many_boxes(nat.AUG_MAX_BOXES, 5)
        labels[5] = _many_boxes(nat.AUG_MAX_BOXES, 6)
    elif layout == "one_too_many":
        labels[2] = _many_boxes(nat.AUG_MAX_BOXES + 1, 5)
        device_route = False
    _, got_lab = _seeded_equals_the_chain(chain, images, labels, SEEDS[:8], device_route)
    if layout == "no_boxes":
        assert got_lab[1].shape == (0, 5) and got_lab[6].shape == (0, 5)
        rows = _trace(chain, labels, SEEDS[:8])
        assert not (rows[1]["translated"] or rows[1]["zoomed"] or rows[6]["translated"] or rows[6]["zoomed"])


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(n_trials_max=1), dict(random_flip=0.0), dict(random_flip=1.0),
                                dict(random_translate=((0.03, 0.5), (0.03, 0.5), 1.0), random_scale=(0.5, 2.0, 0.0)),
                                dict(random_translate=((0.03, 0.5), (0.03, 0.5), 0.0), random_scale=(0.5, 2.0, 1.0)),
                                dict(clip_boxes=False), dict(background=(12, 200, 7))],
                         ids=["one_trial", "never_flip", "always_flip", "always_translate_never_zoom", "never_translate_always_zoom",
                              "no_clip", "background"])
def test_parameters_off_the_notebooks(kw):
    images, labels = _batch(B=12, seed=31)
    _seeded_equals_the_chain(_chain(**kw), images, labels, SEEDS[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(60, 96), (300, 480)])
def test_the_plan_kernel_alone(h, w):
    import torch
    from ssd_keras_amd import _native as nat
    cases = ncp.hand_cases()
    rows = np.stack([c[1] for c in cases])
    geo, xtab, ytab = (t.cpu().numpy() for t in nat.const_augment_plans(torch.from_numpy(rows).cuda(), h, w))
    assert geo.dtype == xtab.dtype == ytab.dtype == np.int32
    for k, (name, _, case) in enumerate(cases):
        want_geo, want_x, want_y, _ = ncp.warp_image_of(case, h, w).plan()
        assert np.array_equal(geo[k], want_geo), (name, geo[k], want_geo)
        assert np.array_equal(xtab[k], want_x), name
        assert np.array_equal(ytab[k], want_y), name
    for got, want in zip((geo, xtab, ytab), ncp.plans(rows, h, w)):
        assert np.array_equal(got, want)


@pytest.mark.gpu
def test_seeded_mode_at_the_notebooks_image_size():
    from tests.test_affine_ops_gpu import _notebook_batch
    images, labels = _notebook_batch(B=8)
    _seeded_equals_the_chain(_chain(), images, labels, SEEDS[:8])


@pytest.mark.gpu
def test_data_generator_takes_the_device_route_by_itself(monkeypatch):
    """generate() with [DataAugmentationConstantInputSize] on eight images of one size: the same batches and the same np.random state
    with the device-side decisions and with the host loop."""
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    images, labels = _batch(B=8, seed=41)
    runs = {}
    for host_loop in ("0", "1"):
        monkeypatch.setenv("SSDHIP_AUG_HOST_STREAM", host_loop)
        g = DataGenerator(labels=[lab.copy() for lab in labels], verbose=False)
        g.images, g.dataset_size, g.dataset_indices = [im for im in images], 8, np.arange(8, dtype=np.int32)
        chain = _chain()
        calls = []
        real = chain.augment_batch
        monkeypatch.setattr(chain, "augment_batch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        gen = g.generate(batch_size=4, shuffle=False, transformations=[chain], returns={'processed_images', 'processed_labels'},
                         keep_images_without_gt=True)
        np.random.seed(77)
        batches = [next(gen) for _ in range(3)]              # the third wraps into the second epoch
        assert len(calls) == 3
        runs[host_loop] = (batches, np.random.get_state())
    (dev, dev_state), (host, host_state) = runs["0"], runs["1"]
    assert dev_state[0] == host_state[0] and np.array_equal(dev_state[1], host_state[1]) and dev_state[2:] == host_state[2:]
    for (dx, dy), (hx, hy) in zip(dev, host):
        assert np.asarray(dx).shape == (4, H, W, 3) and np.array_equal(np.asarray(dx), np.asarray(hx))
        assert len(dy) == len(hy) == 4
        for a, b in zip(dy, hy):
            assert a.dtype == b.dtype and np.array_equal(a, b)
