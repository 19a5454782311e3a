"""The constant-input-size chain's device route, the parts that need no GPU: the signature of `augment_batch`, what `_device_params`
covers and which fields it fills, and the NumPy restatement of the plan kernel against `_image_ops.WarpImage.plan()`."""
import inspect

import numpy as np
import pytest

from tests import np_const_plans as ncp

NOTEBOOK = dict(random_brightness=(-48, 48, 0.5), random_contrast=(0.5, 1.8, 0.5), random_saturation=(0.5, 1.8, 0.5),
                random_hue=(18, 0.5), random_flip=0.5, random_translate=((0.03, 0.5), (0.03, 0.5), 0.5), random_scale=(0.5, 2.0, 0.5),
                n_trials_max=3, clip_boxes=True, overlap_criterion='area', bounds_box_filter=(0.3, 1.0), bounds_validator=(0.5, 1.0),
                n_boxes_min=1, background=(0, 0, 0))


def _chain(**kw):
    from ssd_keras_amd.data_generator.data_augmentation_chain_constant_input_size import DataAugmentationConstantInputSize
    return DataAugmentationConstantInputSize(**dict(NOTEBOOK, **kw))


def test_seeds_is_a_parameter_of_augment_batch():
    from ssd_keras_amd.data_generator.data_augmentation_chain_constant_input_size import DataAugmentationConstantInputSize
    params = list(inspect.signature(DataAugmentationConstantInputSize.augment_batch).parameters.values())
    assert [p.name for p in params[:4]] == ["self", "images", "labels", "seeds"]
    assert params[3].default is None


def test_the_notebook_arguments_are_covered():
    p = _chain()._device_params()
    assert p == dict(photo_prob=[0.5, 0.5, 0.5, 0.5], photo_lower=[-48.0, 0.5, 0.5, -18.0], photo_upper=[48.0, 1.8, 1.8, 18.0],
                     translate_prob=0.5, dy_min=0.03, dy_max=0.5, dx_min=0.03, dx_max=0.5, zoom_in_prob=0.5, zoom_in_min=1.0,
                     zoom_in_max=2.0, zoom_out_prob=0.5, zoom_out_min=0.5, zoom_out_max=1.0, flip_prob=0.5, n_trials=3, clip_boxes=1,
                     n_boxes_min=1, validator_lower=0.5, validator_upper=1.0, filter_lower=0.3, filter_upper=1.0, filter_min_area=16.0)
    lab = [np.array([[1, 2, 3, 40, 50]]), np.zeros((0, 5), dtype=np.int64)]
    assert _chain()._device_params(lab) == p
    assert _chain()._device_params([a.astype(np.float64) for a in lab]) == p


def test_a_second_configuration_fills_the_fields_it_should():
    chain = _chain(random_brightness=(-10, 20, 0.25), random_contrast=(0.7, 1.1, 1.0), random_saturation=(0.9, 1.2, 0.0),
                   random_hue=(7, 0.75), random_flip=1.0, random_translate=((0.0, 0.1), (0.2, 0.4), 0.9), random_scale=(0.25, 3.0, 0.1),
                   n_trials_max=0, clip_boxes=False, bounds_box_filter=(0.0, 0.9), bounds_validator=(0.1, 0.8), n_boxes_min=2,
                   background=(12, 200, 7), labels_format={'class_id': 4, 'xmin': 0, 'ymin': 1, 'xmax': 2, 'ymax': 3})
    assert chain._device_params() == dict(
        photo_prob=[0.25, 1.0, 0.0, 0.75], photo_lower=[-10.0, 0.7, 0.9, -7.0], photo_upper=[20.0, 1.1, 1.2, 7.0], translate_prob=0.9,
        dy_min=0.0, dy_max=0.1, dx_min=0.2, dx_max=0.4, zoom_in_prob=0.1, zoom_in_min=1.0, zoom_in_max=3.0, zoom_out_prob=0.1,
        zoom_out_min=0.25, zoom_out_max=1.0, flip_prob=1.0, n_trials=1, clip_boxes=0, n_boxes_min=2, validator_lower=0.1,
        validator_upper=0.8, filter_lower=0.0, filter_upper=0.9, filter_min_area=16.0)


@pytest.mark.parametrize("name", ["iou", "center_point", "border", "all", "trials", "prob_photo", "prob_flip", "prob_translate",
                                  "prob_scale", "not_n5", "mixed_dtype", "float32", "int32", "too_many", "generator"])
def test_what_the_kernel_does_not_cover_returns_none(name):
    from ssd_keras_amd import _native as nat
    ok_lab = [np.array([[1, 2, 3, 40, 50]]), np.array([[2, 5, 6, 70, 80]])]
    chain, labels, generator = _chain(), None, 'MT19937'
    if name in ("iou", "center_point"):
        chain = _chain(overlap_criterion=name)
    elif name == "border":
        chain.image_validator.border_pixels = 'include'
    elif name == "all":
        chain = _chain(n_boxes_min='all')
    elif name == "trials":
        assert _chain(n_trials_max=nat.CONST_AUG_MAX_TRIALS)._device_params() is not None
        chain = _chain(n_trials_max=nat.CONST_AUG_MAX_TRIALS + 1)
    elif name == "prob_photo":
        chain = _chain(random_hue=(18, 1.5))
    elif name == "prob_flip":
        chain = _chain(random_flip=-0.1)
    elif name == "prob_translate":
        chain = _chain(random_translate=((0.03, 0.5), (0.03, 0.5), 1.01))
    elif name == "prob_scale":
        chain = _chain(random_scale=(0.5, 2.0, 2.0))
    elif name == "not_n5":
        labels = [ok_lab[0], np.array([[1, 2, 3, 40, 50, 0]])]
    elif name == "mixed_dtype":
        labels = [ok_lab[0], ok_lab[1].astype(np.float64)]
    elif name == "float32":
        labels = [a.astype(np.float32) for a in ok_lab]
    elif name == "int32":
        labels = [a.astype(np.int32) for a in ok_lab]
    elif name == "too_many":
        assert chain._device_params([np.tile(ok_lab[0], (nat.AUG_MAX_BOXES, 1))]) is not None
        labels = [np.tile(ok_lab[0], (nat.AUG_MAX_BOXES + 1, 1))]
    elif name == "generator":
        generator = 'PCG64'
    assert chain._device_params(labels, generator=generator) is None


@pytest.mark.parametrize("H,W", [(60, 96), (300, 480), (7, 9)])
def test_plan_restatement_equals_warp_image_plan(H, W):
    cases = ncp.hand_cases()
    assert len(cases) == 14
    geo, xtab, ytab = ncp.plans(np.stack([c[1] for c in cases]), H, W)
    for k, (name, _, case) in enumerate(cases):
        want_geo, want_x, want_y, _ = ncp.warp_image_of(case, H, W).plan()
        assert np.array_equal(geo[k], want_geo), (name, geo[k], want_geo)
        assert xtab[k].dtype == want_x.dtype and np.array_equal(xtab[k], want_x), name
        assert ytab[k].dtype == want_y.dtype and np.array_equal(ytab[k], want_y), name
    # post only exists behind a zoom; a zoom by exactly 1 is a translation by (0, 0), so the shift of sequence 2 stays `pre`
    g1 = ncp.plans(ncp.row(2, shift=(3, -2), factor=1.0), H, W)
    g0 = ncp.plans(ncp.row(2, shift=(3, -2)), H, W)
    assert all(np.array_equal(a, b) for a, b in zip(g1, g0)) and g1[0][0].tolist() == [0, 3, -2, 0, 0]


def test_exports_reject_bad_arguments_before_launching():
    """Every value the kernels loop over or index with is checked on the host, ahead of any launch: callable without a GPU."""
    import ctypes
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd import build
    assert build.build() == nat.lib_path()
    lib = nat.load()
    dummy = ctypes.create_string_buffer(64)
    a = ctypes.addressof(dummy)
    a += (-a) % 16                                                    # a non-null fake pointer (never dereferenced)

    def params(**kw):
        q = nat._ConstAugParams()
        d = dict(_chain()._device_params(), img_height=60, img_width=96)
        d.update(kw)
        for k, v in d.items():
            if isinstance(v, list):
                for i, e in enumerate(v):
                    getattr(q, k)[i] = e
            else:
                setattr(q, k, v)
        return q

    for name in ("ssdhip_const_augment_decide", "ssdhip_const_augment_decide_stream"):
        fn = getattr(lib, name)
        call = lambda q, B=2, ptrs=(a,) * 9: fn(ctypes.byref(q), B, *ptrs, None)
        assert fn(None, 2, *(a,) * 9, None) == -1
        assert call(params(), B=0) == -1
        for k in range(9):
            assert call(params(), ptrs=(a,) * k + (None,) + (a,) * (8 - k)) == -1, (name, k)
        for bad in (dict(img_height=0), dict(img_width=-3), dict(img_width=40000), dict(photo_prob=[0.5, 0.5, 1.5, 0.5]),
                    dict(photo_lower=[50.0, 0.5, 0.5, -18.0]), dict(translate_prob=-0.1), dict(zoom_in_prob=1.1), dict(zoom_out_prob=2.0),
                    dict(flip_prob=float("nan")), dict(dy_min=-0.1), dict(dx_max=0.01), dict(zoom_in_min=0.0), dict(zoom_out_max=0.4),
                    dict(n_trials=0), dict(n_trials=nat.CONST_AUG_MAX_TRIALS + 1), dict(n_boxes_min=0), dict(validator_upper=0.4),
                    dict(filter_lower=1.5), dict(filter_min_area=float("nan"))):
            assert call(params(**bad)) == -1, (name, bad)
    plans = lib.ssdhip_const_augment_plans
    assert plans(None, 2, 60, 96, a, a, a, None) == -1
    for bad in ((0, 60, 96), (70000, 60, 96), (2, 0, 96), (2, 60, 0), (2, 40000, 96), (2, 60, 40000)):
        assert plans(a, *bad, a, a, a, None) == -1, bad
    for k in range(3):
        assert plans(a, 2, 60, 96, *((a,) * k + (None,) + (a,) * (2 - k)), None) == -1


def test_seed_states_are_what_np_random_seed_leaves(monkeypatch):
    import ctypes
    from ssd_keras_amd.data_generator import data_augmentation_chain_constant_input_size as mod
    seeds = [0, 1, 100, 131, 2 ** 32 - 1, np.int64(77)]
    np.random.seed(5)
    before = np.random.get_state()
    got = mod._seed_states(seeds)
    monkeypatch.setattr(ctypes, "string_at", lambda address, size: bytes(size))      # a layout that is not NumPy's: every row from get_state()
    slow = mod._seed_states(seeds)
    monkeypatch.undo()
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert got.shape == slow.shape == (6, 625) and got.dtype == slow.dtype == np.uint32 and np.array_equal(got, slow)
    for row, s in zip(got, seeds):
        np.random.seed(s)
        st = np.random.get_state()
        assert np.array_equal(row[:624], st[1]) and int(row[624]) == st[2] == 624
