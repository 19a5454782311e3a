"""Translate / Scale / Rotate and the augmentation chains on the MI355X: the warpAffine kernel (csrc/ssdhip_warp.hip) against the hand
cases, every reference-generated fixture case through the drop-ins bit for bit, and the constant-input-size chain's batch path
(two pixel launches) against its per-image loop."""
import numpy as np
import pytest

from tests import affine_cases as ac
from tests import affine_hand_cases as hc
from tests.test_affine_ops_cpu import check_cases


@pytest.mark.gpu
def test_kernel_equals_the_hand_cases():
    import torch
    from ssd_keras_amd.data_generator import _image_ops as iop
    from tests import np_warp
    for name, src, M, dsize, bg, want in hc.CASES:
        got = iop.warp_affine(src, M, dsize, bg)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, got.tolist())
    # every channel count, odd / multiple-of-4 widths, images whose last pixel ends the buffer, a batch with per-image geometry
    rng = np.random.RandomState(5)
    for c in (1, 2, 3, 4):
        for h, w, oh, ow in ((7, 9, 7, 9), (13, 16, 11, 20), (5, 3, 6, 5)):
            imgs = rng.randint(0, 256, size=(3, h, w, c)).astype(np.uint8)
            mats = [iop.rotation_matrix_2d((w / 2, h / 2), a, s) for a, s in ((0, 1.37), (90, 1), (0, 0.61))]
            bg = rng.randint(0, 256, size=(3, c)).astype(np.uint8)
            geo = np.array([[0, 0, 0, 0, 0], [1, 2, -1, 0, 0], [1, 0, 0, -3, 2]], dtype=np.int32)
            tabs = [iop.warp_tables(M, oh, ow) for M in mats]
            got = iop.nat.image_warp_affine_u8(torch.from_numpy(imgs).cuda(), oh, ow, geo, np.stack([t[0] for t in tabs]),
                                               np.stack([t[1] for t in tabs]), bg).cpu().numpy()
            want = np_warp.apply_tables(imgs, oh, ow, geo, np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), bg)
            assert np.array_equal(got, want), (c, h, w, oh, ow)
            assert np.array_equal(got[0], np_warp.warp_affine(imgs[0], mats[0], (ow, oh), tuple(int(v) for v in bg[0])).reshape(oh, ow, c))


@pytest.mark.gpu
def test_drop_ins_match_the_reference():
    assert check_cases(include_boxes_kernel=True) == len(ac.CASES)


def _notebook_batch(B=32, H=300, W=480, seed=9):
    rng = np.random.RandomState(seed)
    images = rng.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    labels = []
    for i in range(B):
        if i % 4 == 3:                                       # one small box in a corner: most translations / zooms lose it
            labels.append(np.array([[rng.randint(1, 6), 0, 0, 40, 30]]) + np.array([[0, W - 41, H - 31, W - 41, H - 31]]) * (i % 8 == 7))
            continue
        n = rng.randint(1, 6)
        x0, y0 = rng.randint(0, W - 120, size=n), rng.randint(0, H - 90, size=n)
        labels.append(np.stack([rng.randint(1, 6, size=n), x0, y0, x0 + rng.randint(8, 120, size=n), y0 + rng.randint(6, 90, size=n)], axis=1))
    return images, labels


@pytest.mark.gpu
def test_augment_batch_equals_the_per_image_chain_and_is_two_launches(monkeypatch):
    """SSD7's notebook chain (ssd7_training.ipynb:301-316, its exact arguments) at the notebook's image size: `augment_batch` == the
    `__call__` loop from the same seed -- pixels, labels, dtypes and the full np.random state afterwards; the run holds both sequences,
    images where every trial failed, flips -- and its pixels are exactly two launches."""
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import object_detection_2d_geometric_ops as geo
    from ssd_keras_amd.data_generator.data_augmentation_chain_constant_input_size import DataAugmentationConstantInputSize
    chain = DataAugmentationConstantInputSize(random_brightness=(-48, 48, 0.5), random_contrast=(0.5, 1.8, 0.5),
                                              random_saturation=(0.5, 1.8, 0.5), random_hue=(18, 0.5), random_flip=0.5,
                                              random_translate=((0.03, 0.5), (0.03, 0.5), 0.5), random_scale=(0.5, 2.0, 0.5),
                                              n_trials_max=3, clip_boxes=True, overlap_criterion='area', bounds_box_filter=(0.3, 1.0),
                                              bounds_validator=(0.5, 1.0), n_boxes_min=1, background=(0, 0, 0))
    images, labels = _notebook_batch()
    # what happens to each image in the loop: sequence, flips, failed trial loops (the ops' own calls observed)
    seen = {"seq": [], "flip": 0, "failed": 0}
    real_draw, real_flip_call, real_validator = chain._draw, geo.Flip.__call__, chain.image_validator.__call__.__func__
    trials = []

    def draw():
        out = real_draw()
        seen["seq"].append(out[0])
        return out

    def flip_call(self, image, labels=None, return_inverter=False):
        seen["flip"] += 1
        return real_flip_call(self, image, labels, return_inverter)

    def validator(self, labels, image_height, image_width):
        ok = real_validator(self, labels, image_height, image_width)
        trials.append(ok)
        return ok

    monkeypatch.setattr(chain, "_draw", draw)
    monkeypatch.setattr(geo.Flip, "__call__", flip_call)
    monkeypatch.setattr(type(chain.image_validator), "__call__", validator)
    np.random.seed(2024)
    want = [chain(images[i], labels[i]) for i in range(len(labels))]
    want_state = np.random.get_state()
    monkeypatch.undo()
    streak = 0
    for ok in trials:                                        # three failed validations in a row = a trial loop that gave up
        streak = 0 if ok else streak + 1
        seen["failed"] += streak == 3
    assert set(seen["seq"]) == {1, 2} and seen["flip"] > 0 and seen["failed"] > 0, seen

    calls = {"program": 0, "warp": 0, "other": 0}
    for name in ("image_program", "image_warp_affine_u8", "image_resize_cv_u8", "image_resize_gather_cv_u8", "image_lut_u8"):
        real = getattr(nat, name)
        key = {"image_program": "program", "image_warp_affine_u8": "warp"}.get(name, "other")

        def counted(*a, _real=real, _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(nat, name, counted)
    np.random.seed(2024)
    got_img, got_lab = chain.augment_batch(torch.from_numpy(images).cuda(), labels)
    got_state = np.random.get_state()
    monkeypatch.undo()
    assert calls == {"program": 1, "warp": 1, "other": 0}, calls
    assert got_state[0] == want_state[0] and np.array_equal(got_state[1], want_state[1]) and got_state[2:] == want_state[2:]
    g = got_img.cpu().numpy()
    assert got_img.dtype == torch.uint8 and g.shape == images.shape
    for i in range(len(labels)):
        assert np.array_equal(g[i], want[i][0]), "image %d: %d pixels differ" % (i, int((g[i] != want[i][0]).sum()))
        assert got_lab[i].dtype == want[i][1].dtype and np.array_equal(got_lab[i], want[i][1]), i
