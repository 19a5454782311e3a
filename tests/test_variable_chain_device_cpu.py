"""The variable-input-size chain's device route, the parts that need no GPU: the signature of `augment_batch`, what `_device_params`
covers and which fields it fills, the NumPy restatement of the decision kernel's walk (tests/np_variable_chain.py) against the chain's
own `__call__` (kernels replaced by NumPy statements of their contracts) and against the reference's golden cases, `_lazy_of`, and
`augment_batch` with the decision exports replaced by that restatement against the `__call__` loop."""
import inspect

import numpy as np
import pytest

from tests import np_variable_chain as nvc
from tests import variable_chain_cases as vc

DEFAULTS = dict(photo_prob=[0.5, 0.5, 0.5, 0.5], photo_lower=[-48.0, 0.5, 0.5, -18.0], photo_upper=[48.0, 1.8, 1.8, 18.0], patch_prob=1.0,
                min_scale=0.3, max_scale=2.0, min_aspect_ratio=0.5, max_aspect_ratio=2.0, n_trials=3, clip_boxes=1, criterion=2,
                n_boxes_min=1, validator_lower=0.5, validator_upper=1.0, filter_lower=0.3, filter_upper=1.0, flip_prob=0.5, out_height=30,
                out_width=36, interpolation=1, resize_min_area=16.0)


def test_seeds_is_a_parameter_of_augment_batch():
    from ssd_keras_amd.data_generator.data_augmentation_chain_variable_input_size import DataAugmentationVariableInputSize
    params = list(inspect.signature(DataAugmentationVariableInputSize.augment_batch).parameters.values())
    assert [p.name for p in params[:4]] == ["self", "images", "labels", "seeds"]
    assert params[3].default is None


def test_the_default_constructor_is_covered_and_fills_every_field():
    from ssd_keras_amd import _native as nat
    p = vc.chain()._device_params()
    assert p == DEFAULTS
    assert sorted(p) == sorted(n for n, _ in nat._VarAugParams._fields_ if n not in ("img_height", "img_width"))
    lab = [np.array([[1, 2, 3, 40, 50]]), np.zeros((0, 5), dtype=np.int64)]
    assert vc.chain()._device_params(lab) == p
    assert vc.chain()._device_params([a.astype(np.float64) for a in lab], shapes=[(40, 48), (24, 40)]) == p


def test_a_second_configuration_fills_the_fields_it_should():
    ch = vc.chain(out=(64, 48), random_brightness=(-10, 20, 0.25), random_contrast=(0.7, 1.1, 1.0), random_saturation=(0.9, 1.2, 0.0),
                  random_hue=(7, 0.75), random_flip=1.0, min_scale=0.5, max_scale=1.5, min_aspect_ratio=0.8, max_aspect_ratio=1.25,
                  n_trials_max=0, clip_boxes=False, overlap_criterion='iou', bounds_box_filter=(0.0, 0.9), bounds_validator=(0.1, 0.8),
                  n_boxes_min='all', background=(12, 200, 7), labels_format={'class_id': 4, 'xmin': 0, 'ymin': 1, 'xmax': 2, 'ymax': 3})
    ch.resize.interpolation_mode = 3
    ch.random_patch.prob = 0.75
    assert ch._device_params() == dict(
        photo_prob=[0.25, 1.0, 0.0, 0.75], photo_lower=[-10.0, 0.7, 0.9, -7.0], photo_upper=[20.0, 1.1, 1.2, 7.0], patch_prob=0.75,
        min_scale=0.5, max_scale=1.5, min_aspect_ratio=0.8, max_aspect_ratio=1.25, n_trials=0, clip_boxes=0, criterion=1, n_boxes_min=0,
        validator_lower=0.1, validator_upper=0.8, filter_lower=0.0, filter_upper=0.9, flip_prob=1.0, out_height=64, out_width=48,
        interpolation=3, resize_min_area=16.0)
    assert vc.chain(overlap_criterion='center_point', n_boxes_min=2)._device_params() == dict(DEFAULTS, criterion=0, n_boxes_min=2)


@pytest.mark.parametrize("name", ["too_many", "float32", "int32", "mixed_dtype", "not_n5", "bound_generator_validator",
                                  "bound_generator_filter", "generator", "taps", "narrow", "empty_patch", "border", "can_fail",
                                  "criteria_differ", "prob", "interpolation", "vertical_flip"])
def test_what_the_kernel_does_not_cover_returns_none(name):
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator.object_detection_2d_image_boxes_validation_utils import BoundGenerator
    ok_lab = [np.array([[1, 2, 3, 40, 50]]), np.array([[2, 5, 6, 70, 80]])]
    ch, labels, generator, shapes = vc.chain(), None, 'MT19937', None
    if name == "too_many":
        assert ch._device_params([np.tile(ok_lab[0], (nat.AUG_MAX_BOXES, 1))]) is not None
        labels = [np.tile(ok_lab[0], (nat.AUG_MAX_BOXES + 1, 1))]
    elif name == "float32":
        labels = [a.astype(np.float32) for a in ok_lab]
    elif name == "int32":
        labels = [a.astype(np.int32) for a in ok_lab]
    elif name == "mixed_dtype":
        labels = [ok_lab[0], ok_lab[1].astype(np.float64)]
    elif name == "not_n5":
        labels = [ok_lab[0], np.array([[1, 2, 3, 40, 50, 0]])]
    elif name == "bound_generator_validator":
        ch.image_validator.bounds = BoundGenerator()
    elif name == "bound_generator_filter":
        ch.box_filter_patch.overlap_bounds = BoundGenerator()
    elif name == "generator":
        generator = 'PCG64'
    elif name == "taps":
        ch.resize.interpolation_mode = 3                       # INTER_AREA: ceil(2.0 * 500 / 0.5 / 30) + 2 = 69 taps
        assert ch._device_params(shapes=[(375, 400)]) is not None
        shapes = [(375, 500)]
    elif name == "narrow":
        ch = vc.chain(min_scale=0.8, max_aspect_ratio=1.5)
        assert ch._device_params(shapes=[(40, 4)]) is not None
        shapes = [(40, 4), (40, 3)]
    elif name == "empty_patch":                               # int(0.3 * 6) = 1 px wide, int(1 / 2.0) = 0 px high
        assert ch._device_params(shapes=[(40, 7)]) is not None
        shapes = [(40, 6)]
    elif name == "border":
        ch.image_validator.border_pixels = 'include'
    elif name == "can_fail":
        ch.random_patch.can_fail = True
    elif name == "criteria_differ":
        ch.image_validator.overlap_criterion = 'iou'
    elif name == "prob":
        ch = vc.chain(random_flip=1.5)
    elif name == "interpolation":
        ch.resize.interpolation_mode = 7
    elif name == "vertical_flip":
        ch.random_flip.dim = 'vertical'
    assert ch._device_params(labels, generator=generator, shapes=shapes) is None


def _walk_one(ch, img, labels, seed):
    """The restatement on one image under np.random.seed(seed): (pixels, labels in the caller's dtype, state row, geometry row)."""
    lab = np.asarray(labels)
    lab_in, n_in = np.zeros((1, 64, 5)), np.array([lab.shape[0]], dtype=np.int32)
    lab_in[0, :lab.shape[0]] = lab
    mt = vc.state_row(np.random.RandomState(seed).get_state())[None]
    p = ch._device_params([lab], shapes=[img.shape[:2]])
    ops, args, geo, lab_out, n_out, mt_out, _ = nvc.walk(p, mt, lab_in, n_in, [img.shape[:2]])
    px = nvc.pixels(img, ops[0], args[0], geo[0], p["out_height"], p["out_width"], ch.random_patch.sample_patch.background)
    return px, lab_out[0, :n_out[0]].astype(lab.dtype), mt_out[0], geo[0]


def test_restatement_equals_the_chain_and_the_reference_on_the_golden_cases(monkeypatch):
    vc.install_cpu_kernels(monkeypatch)
    cases = vc.golden_cases()
    assert len(cases) == 10
    for case, img, labels, want in cases:
        ch = vc.chain()
        (px, lb, st), = vc.per_image(ch, [img], [labels], [case["seed"]])
        got_px, got_lb, got_st, _ = _walk_one(ch, img, labels, case["seed"])
        assert np.array_equal(got_px, px) and got_lb.dtype == lb.dtype and np.array_equal(got_lb, lb) and np.array_equal(got_st, st), case
        # ... and the fixture generated from the reference itself
        assert np.array_equal(got_px, want["image"]) and np.array_equal(got_lb, want["labels"]), case
        assert str(got_lb.dtype) == str(want["labels_dtype"]) and vc.np_state_digest(got_st) == str(want["np_state"]), case


BRANCH_CONFIGS = {
    "default": dict(),
    "never_valid": dict(bounds_validator=(0.99, 1.0)),
    "iou": dict(overlap_criterion='iou', bounds_validator=(0.02, 1.0), bounds_box_filter=(0.01, 1.0)),
    "center_point": dict(overlap_criterion='center_point'),
    "all_boxes": dict(n_boxes_min='all', bounds_validator=(0.1, 1.0)),
    "two_boxes": dict(n_boxes_min=2, bounds_validator=(0.3, 1.0)),
    "strict_lower": dict(bounds_box_filter=(0.0, 1.0)),
    "no_clip": dict(clip_boxes=False),
    "no_trials": dict(n_trials_max=0),
    "one_trial": dict(n_trials_max=1),
    "never_flip": dict(random_flip=0.0),
    "always_flip": dict(random_flip=1.0),
}


@pytest.mark.parametrize("config", sorted(BRANCH_CONFIGS))
def test_restatement_equals_the_chain_on_the_branch_table(monkeypatch, config):
    vc.install_cpu_kernels(monkeypatch)
    ch = vc.chain(**BRANCH_CONFIGS[config])
    images, labels = vc.batch()
    seeds = vc.UNALTERED_SEEDS if config == "never_valid" else vc.BRANCH_SEEDS
    found = vc.branches(vc.trace(ch, [im.shape[:2] for im in images], labels, seeds))
    if config == "default":
        assert found >= vc.BRANCHES, sorted(vc.BRANCHES - found)
    elif config == "never_valid":
        assert "unaltered" in found
    want = vc.per_image(ch, images, labels, seeds)
    for img, lab, seed, (px, lb, st) in zip(images, labels, seeds, want):
        got_px, got_lb, got_st, _ = _walk_one(ch, img, lab, seed)
        assert np.array_equal(got_px, px), (config, seed)
        assert got_lb.dtype == lb.dtype and np.array_equal(got_lb, lb), (config, seed, got_lb, lb)
        assert np.array_equal(got_st, st), (config, seed, got_st[624], st[624])


def test_lazy_of_equals_the_image_the_chain_builds(monkeypatch):
    from ssd_keras_amd.data_generator import _image_ops as iop
    vc.install_cpu_kernels(monkeypatch)
    images, labels = vc.batch()
    kinds = set()
    for k, (img, lab) in enumerate(list(zip(images, labels)) * 2):
        # the second round with a validator that rejects every cropping patch: image 6 comes out unaltered
        ch, seed = (vc.chain(), vc.BRANCH_SEEDS[k]) if k < 8 else (vc.chain(bounds_validator=(0.99, 1.0)), vc.UNALTERED_SEEDS[k - 8])
        ch.random_patch.sample_patch.background = (9, 80, 200)
        h, w = img.shape[:2]
        _, _, _, g = _walk_one(ch, img, lab, seed)
        np.random.seed(seed)
        ch._draw()
        want = iop.GeoImage.of(h, w)
        for t in (ch.random_patch, ch.random_flip, ch.resize):
            want, lab = t(want, lab)
        got = ch._lazy_of(g, h, w)
        assert np.array_equal(got.ys, want.ys) and np.array_equal(got.xs, want.xs) and got.resized == want.resized
        assert got.background == want.background
        kinds.add((bool(g[0]), bool(g[10])))
    assert {k[0] for k in kinds} == {True, False} and {k[1] for k in kinds} == {True, False}      # patched / unaltered, flipped / not


@pytest.mark.parametrize("layout", ["int64", "float64", "permuted"])
def test_augment_batch_on_the_restatement_equals_the_call_loop(monkeypatch, layout):
    """The Python around the kernel -- packing, label dtype and column order, the write-back of the generator state, the routes."""
    calls = []
    vc.install_cpu_kernels(monkeypatch, calls)
    images, labels = vc.batch()
    ch = vc.chain()
    if layout == "float64":
        labels = [lab.astype(np.float64) + np.array([[0.0, 0.25, 0.5, 0.75, 0.5]]) for lab in labels]
    elif layout == "permuted":
        ch = vc.chain(labels_format={'class_id': 4, 'xmin': 2, 'ymin': 0, 'xmax': 3, 'ymax': 1})
        labels = [lab[:, [2, 4, 1, 3, 0]] for lab in labels]
    # ---- stream mode: np.random goes on behind the batch ----
    np.random.seed(vc.BRANCH_STREAM_SEED)
    want = vc.call_loop(ch, images, labels)
    want_state = np.random.get_state()
    np.random.seed(vc.BRANCH_STREAM_SEED)
    got_img, got_lab = ch.augment_batch(images, labels)
    assert calls == ["stream_ragged"]
    vc.assert_equal(got_img, got_lab, want)
    assert vc.same_state(np.random.get_state(), want_state)
    # ---- the forced host path gives the same and launches no decision kernel ----
    monkeypatch.setenv("SSDHIP_AUG_HOST_STREAM", "1")
    np.random.seed(vc.BRANCH_STREAM_SEED)
    got_img, got_lab = ch.augment_batch(images, labels)
    assert calls == ["stream_ragged"]
    vc.assert_equal(got_img, got_lab, want)
    assert vc.same_state(np.random.get_state(), want_state)
    monkeypatch.delenv("SSDHIP_AUG_HOST_STREAM")
    # ---- seeded mode: per-image streams, np.random untouched ----
    want = vc.per_image(ch, images, labels, vc.BRANCH_SEEDS)
    before = np.random.get_state()
    got_img, got_lab = ch.augment_batch(images, labels, seeds=vc.BRANCH_SEEDS)
    assert calls == ["stream_ragged", "decide"]
    assert vc.same_state(np.random.get_state(), before)
    vc.assert_equal(got_img, got_lab, want, ch._last_generator_states)
    # ---- a label layout the kernel does not cover: the host code under each seed, same results, state restored ----
    labels32 = [lab.astype(np.float32) for lab in labels]
    want = vc.per_image(ch, images, labels32, vc.BRANCH_SEEDS)
    got_img, got_lab = ch.augment_batch(images, labels32, seeds=vc.BRANCH_SEEDS)
    assert calls == ["stream_ragged", "decide"] and vc.same_state(np.random.get_state(), before)
    vc.assert_equal(got_img, got_lab, want, ch._last_generator_states)


def test_the_stream_seed_takes_every_branch(monkeypatch):
    vc.install_cpu_kernels(monkeypatch)
    images, labels = vc.batch()
    np.random.seed(vc.BRANCH_STREAM_SEED)
    found = vc.branches(vc.trace(vc.chain(), [im.shape[:2] for im in images], labels))
    assert found >= vc.BRANCHES, sorted(vc.BRANCHES - found)


def test_data_generator_routes_the_chain_when_labels_are_present():
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    images, _ = vc.batch(B=3)
    grey = images[0][:, :, 0]
    assert DataGenerator._batch_path([vc.chain()], images + [grey], True) == 'variable'
    assert DataGenerator._batch_path([vc.chain()], images, False) is None
    assert DataGenerator._batch_path([vc.chain(), vc.chain()], images, True) is None


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
        q = nat._VarAugParams()
        d = dict(vc.chain()._device_params(), img_height=40, img_width=48)
        d.update(kw)
        for k, v in d.items():
            if isinstance(v, list):
                for i, e in enumerate(v):
                    getattr(q, k)[i] = e
            else:
                setattr(q, k, v)
        return q

    bad_params = (dict(photo_prob=[0.5, 0.5, 1.5, 0.5]), dict(photo_lower=[50.0, 0.5, 0.5, -18.0]), dict(patch_prob=-0.1),
                  dict(flip_prob=float("nan")), dict(min_scale=2.5), dict(min_scale=0.0), dict(max_aspect_ratio=0.4),
                  dict(min_aspect_ratio=-1.0), dict(n_trials=-1), dict(criterion=3), dict(criterion=-1), dict(n_boxes_min=-1),
                  dict(validator_upper=0.4), dict(filter_lower=1.5), dict(out_height=0), dict(out_width=-2), dict(interpolation=5),
                  dict(resize_min_area=float("nan")))
    # name -> (takes a table?, the table may be null?)
    forms = {"ssdhip_var_augment_decide": (True, True), "ssdhip_var_augment_decide_stream": (False, False),
             "ssdhip_var_augment_decide_stream_ragged": (True, False)}
    for name, (has_table, table_optional) in forms.items():
        fn = getattr(lib, name)

        def rc(q, B=2, n_max=3, table=a, ptrs=(a,) * 9):
            return fn(ctypes.byref(q) if q is not None else None, B, n_max, *(((table,) if has_table else ()) + tuple(ptrs)), None)

        assert rc(None) == -1
        assert rc(params(), B=0) == -1 and rc(params(), B=-4) == -1
        assert rc(params(), n_max=65) == -1 and rc(params(), n_max=-1) == -1
        for k in range(9):
            assert rc(params(), ptrs=(a,) * k + (None,) + (a,) * (8 - k)) == -1, (name, k)
        for bad in bad_params:
            assert rc(params(**bad)) == -1, (name, bad)
        if has_table and not table_optional:
            assert rc(params(), table=None) == -1
        if not has_table or table_optional:                           # without a table the size comes from the parameter block
            kw = dict(table=None) if has_table else {}
            assert rc(params(img_height=0), **kw) == -1 and rc(params(img_width=-3), **kw) == -1
