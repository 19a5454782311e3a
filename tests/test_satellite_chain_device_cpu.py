"""The satellite chain's device route, the parts that need no GPU: the quarter turn as the index permutation `GeoImage` records, the
integer label rule of the decision kernel, what `_device_params` covers, the NumPy restatement of the kernel's walk
(tests/np_satellite_chain.py) against the chain's own `__call__` and the reference's golden cases, and `augment_batch` with the decision
exports replaced by that restatement against the `__call__` loop -- np.random's AND Python's generator included."""
import inspect
import random

import numpy as np
import pytest

from tests import np_satellite_chain as nsc
from tests import np_warp
from tests import satellite_chain_cases as sc

DEFAULTS = dict(photo_prob=[0.5, 0.5, 0.5, 0.5], photo_lower=[-48.0, 0.5, 0.5, -18.0], photo_upper=[48.0, 1.8, 1.8, 18.0], patch_prob=1.0,
                min_scale=0.3, max_scale=2.0, min_aspect_ratio=0.8, max_aspect_ratio=1.25, n_trials=3, clip_boxes=1, criterion=2,
                n_boxes_min=1, validator_lower=0.5, validator_upper=1.0, filter_lower=0.3, filter_upper=1.0, flip_prob=0.5, out_height=30,
                out_width=36, interpolation=1, resize_min_area=16.0, vflip_prob=0.5, rotate_prob=0.5)


def test_seeds_is_a_parameter_of_augment_batch():
    from ssd_keras_amd.data_generator.data_augmentation_chain_satellite import DataAugmentationSatellite
    params = list(inspect.signature(DataAugmentationSatellite.augment_batch).parameters.values())
    assert [p.name for p in params[:4]] == ["self", "images", "labels", "seeds"]
    assert params[3].default is None


def test_quarter_turn_is_the_permutation_warp_affine_computes():
    """GeoImage's quarter turn, executed with NumPy indexing, against cv2.warpAffine's arithmetic on Rotate's matrix: every H, W in
    1 .. 19 plus larger odd and even sizes, all three angles -- and through the op itself (Rotate on a lazy image)."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Rotate
    rng = np.random.RandomState(3)
    sizes = [(h, w) for h in range(1, 20) for w in range(1, 20)] + [(31, 57), (64, 83), (57, 31), (90, 128)]
    for h, w in sizes:
        img = rng.randint(1, 256, size=(h, w, 3)).astype(np.uint8)           # no zeros: a border pixel cannot pass for a source pixel
        for angle in (90, 180, 270):
            M, dsize = iop.quarter_turn_matrix(h, w, angle)
            want = np_warp.warp_affine(img, M, dsize, 0)
            lazy = Rotate(angle)(iop.GeoImage.of(h, w))
            assert lazy.shape == want.shape and lazy.transposed == (angle != 180), (h, w, angle)
            assert np.array_equal(nsc.index_maps(img, lazy), want), (h, w, angle)


def test_quarter_turns_compose_with_flips_and_windows():
    """Flips in front of the turn, a padding window with a coloured background behind it: the two fill values stay apart."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    rng = np.random.RandomState(4)
    for (h, w), angle in (((7, 12), 90), ((12, 7), 270), ((9, 9), 180), ((5, 16), 90)):
        img = rng.randint(1, 256, size=(h, w, 3)).astype(np.uint8)
        lazy = iop.GeoImage.of(h, w)[:, ::-1][::-1].turn(angle)
        M, dsize = iop.quarter_turn_matrix(h, w, angle)
        turned = np_warp.warp_affine(np.ascontiguousarray(img[:, ::-1][::-1]), M, dsize, 0)
        assert np.array_equal(nsc.index_maps(img, lazy), turned)
        rh, rw = turned.shape[:2]
        win = lazy.window(-2, 1, rh + 3, rw + 1, (9, 80, 200))
        want = np.empty((rh + 3, rw + 1, 3), dtype=np.uint8)
        want[:, :] = (9, 80, 200)
        want[2:2 + rh, :rw - 1] = turned[:, 1:]
        assert np.array_equal(nsc.index_maps(img, win), want)
        assert np.array_equal(nsc.index_maps(img, win[:, ::-1]), want[:, ::-1])


def test_lazy_images_take_rotates_warps_only():
    from ssd_keras_amd.data_generator import _image_ops as iop
    lazy = iop.GeoImage.of(10, 14)
    M, dsize = iop.quarter_turn_matrix(10, 14, 90)
    assert iop.warp_affine(lazy, M, dsize, 0).shape == (14, 10, 3)
    with pytest.raises(NotImplementedError):
        iop.warp_affine(lazy, M, dsize, (0, 3, 0))                              # a coloured border
    with pytest.raises(NotImplementedError):
        iop.warp_affine(lazy, M, (14, 10), 0)                                   # another output size
    with pytest.raises(NotImplementedError):
        iop.warp_affine(lazy, iop.quarter_turn_matrix(14, 10, 90)[0], dsize, 0)   # another image's matrix
    with pytest.raises(NotImplementedError):
        iop.warp_affine(lazy, iop.rotation_matrix_2d((7, 5), 30, 1), (14, 10), 0)
    with pytest.raises(NotImplementedError):
        lazy.window(-1, 0, 12, 14, (1, 2, 3)).turn(90)                          # a rotation behind a padding


@pytest.mark.parametrize("dtype", [np.int64, np.float64])
def test_integer_label_rule_equals_rotate(dtype):
    """The closed integer form of Rotate's label arithmetic against Rotate.__call__ on a lazy image: whole-valued boxes, boxes outside
    the image included, sizes from 1 x 1 to 4001 x 2999."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Rotate
    rng = np.random.RandomState(11)
    for h, w in ((1, 1), (1, 7), (2, 3), (19, 19), (40, 48), (57, 83), (300, 301), (375, 500), (1024, 768), (2999, 4001), (4001, 2999)):
        n = 40
        x0, y0 = rng.randint(-w - 5, 2 * w + 5, size=n), rng.randint(-h - 5, 2 * h + 5, size=n)
        lab = np.stack([rng.randint(1, 21, size=n), x0, y0, x0 + rng.randint(0, w + 9, size=n), y0 + rng.randint(0, h + 9, size=n)],
                       axis=1).astype(dtype)
        for turns in (1, 2, 3):
            _, want = Rotate(90 * turns)(iop.GeoImage.of(h, w), lab)
            got = lab.astype(np.float64)
            got[:, 1], got[:, 2], got[:, 3], got[:, 4] = nsc.rotate_labels(turns, float(h), float(w), *(lab[:, k].astype(np.float64)
                                                                                                          for k in (1, 2, 3, 4)))
            assert want.dtype == dtype and np.array_equal(got.astype(dtype), want), (h, w, turns)


def test_the_default_constructor_is_covered_and_fills_every_field():
    from ssd_keras_amd import _native as nat
    p = sc.chain()._device_params()
    assert p == DEFAULTS
    fields = [n for n, _ in nat._VarAugParams._fields_ if n not in ("img_height", "img_width")] + ["vflip_prob", "rotate_prob"]
    assert sorted(p) == sorted(fields)
    assert [n for n, _ in nat._SatAugParams._fields_] == ["var", "vflip_prob", "rotate_prob"]
    images, labels = sc.batch()
    shapes = [im.shape[:2] for im in images]
    assert isinstance(sc.chain()._device_params(labels, shapes=shapes), dict)
    assert sc.chain()._device_params([a.astype(np.float64) for a in labels], shapes=shapes) == p
    ch = sc.chain(random_flip=0.25, random_rotate=([270], 1.0))
    ch.random_vertical_flip.prob = 0.75
    assert ch._device_params() == dict(DEFAULTS, flip_prob=0.25, vflip_prob=0.75, rotate_prob=1.0)


@pytest.mark.parametrize("name", ["too_many", "float32", "int32", "mixed_dtype", "not_n5", "fractional", "bound_generator_validator",
                                  "bound_generator_filter", "generator", "taps", "narrow_width", "narrow_height", "empty_patch", "border",
                                  "can_fail", "criteria_differ", "prob", "interpolation", "hflip_dim", "vflip_dim", "vflip_prob",
                                  "angles_empty", "angles_other", "angles_not_a_list", "rotate_prob"])
def test_what_the_kernel_does_not_cover_returns_none(name):
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator.object_detection_2d_image_boxes_validation_utils import BoundGenerator
    ok_lab = [np.array([[1, 2, 3, 40, 50]]), np.array([[2, 5, 6, 70, 80]])]
    ch, labels, generator, shapes = sc.chain(), None, 'MT19937', None
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
    elif name == "fractional":
        assert ch._device_params([a.astype(np.float64) for a in ok_lab]) is not None
        labels = [ok_lab[0].astype(np.float64), ok_lab[1] + np.array([[0.0, 0.0, 0.5, 0.0, 0.0]])]
    elif name == "bound_generator_validator":
        ch.image_validator.bounds = BoundGenerator()
    elif name == "bound_generator_filter":
        ch.box_filter_patch.overlap_bounds = BoundGenerator()
    elif name == "generator":
        generator = 'PCG64'
    elif name == "taps":
        ch.resize.interpolation_mode = 3                       # INTER_AREA, the LARGER side counts: ceil(2.0 * side / 0.8 / 30) + 2 = 54 / 67
        assert ch._device_params(shapes=[(100, 620)]) is not None
        shapes = [(770, 100)]
    elif name == "narrow_width":
        ch = sc.chain(min_scale=0.8, max_aspect_ratio=1.5)
        assert ch._device_params(shapes=[(40, 4)]) is not None
        shapes = [(40, 4), (40, 3)]
    elif name == "narrow_height":                              # a rotation makes the height the width
        ch = sc.chain(min_scale=0.8, max_aspect_ratio=1.5)
        assert ch._device_params(shapes=[(4, 40)]) is not None
        shapes = [(4, 40), (3, 40)]
    elif name == "empty_patch":                               # int(0.3 * 6) = 1 px wide, int(1 / 1.25) = 0 px high
        assert ch._device_params(shapes=[(40, 7)]) is not None
        shapes = [(6, 40)]
    elif name == "border":
        ch.image_validator.border_pixels = 'include'
    elif name == "can_fail":
        ch.random_patch.can_fail = True
    elif name == "criteria_differ":
        ch.image_validator.overlap_criterion = 'iou'
    elif name == "prob":
        ch = sc.chain(random_flip=1.5)
    elif name == "interpolation":
        ch.resize.interpolation_mode = 7
    elif name == "hflip_dim":
        ch.random_horizontal_flip.dim = 'vertical'
    elif name == "vflip_dim":
        ch.random_vertical_flip.dim = 'horizontal'
    elif name == "vflip_prob":
        ch.random_vertical_flip.prob = -0.1
    elif name == "angles_empty":
        ch.random_rotate.angles = []
    elif name == "angles_other":
        ch.random_rotate.angles = [90, 45]
    elif name == "angles_not_a_list":
        ch.random_rotate.angles = 90
    elif name == "rotate_prob":
        ch.random_rotate.prob = 1.01
    assert ch._device_params(labels, generator=generator, shapes=shapes) is None


def _walk_one(ch, img, labels, seed):
    """The restatement on one image under np.random.seed(seed); random.seed(seed): (pixels, labels, state row, geometry row)."""
    lab = np.asarray(labels)
    lab_in, n_in = np.zeros((1, 64, 5)), np.array([lab.shape[0]], dtype=np.int32)
    lab_in[0, :lab.shape[0]] = lab
    mt = sc.state_row(np.random.RandomState(seed).get_state())[None]
    p = ch._device_params([lab], shapes=[img.shape[:2]])
    turns = [random.Random(seed).choice(ch.random_rotate.angles) // 90]
    ops, args, geo, lab_out, n_out, mt_out = nsc.walk(p, turns, mt, lab_in, n_in, [img.shape[:2]])
    from oracle import np_image as npi
    px = nsc.geometry(npi.run_program(img, ops[0], args[0]), geo[0], p["out_height"], p["out_width"],
                      ch.random_patch.sample_patch.background)
    return px, lab_out[0, :n_out[0]].astype(lab.dtype), mt_out[0], geo[0]


def test_restatement_equals_the_chain_and_the_reference_on_the_golden_cases(monkeypatch):
    sc.install_cpu_kernels(monkeypatch)
    cases = sc.golden_cases()
    assert len(cases) == 10
    for case, img, labels, want in cases:
        ch = sc.chain()
        (px, lb, st), = sc.per_image(ch, [img], [labels], [case["seed"]])
        got_px, got_lb, got_st, _ = _walk_one(ch, img, labels, case["seed"])
        assert np.array_equal(got_px, px) and got_lb.dtype == lb.dtype and np.array_equal(got_lb, lb) and np.array_equal(got_st, st), case
        assert np.array_equal(got_px, want["image"]) and np.array_equal(got_lb, want["labels"]), case
        assert str(got_lb.dtype) == str(want["labels_dtype"]) and sc.np_state_digest(got_st) == str(want["np_state"]), case


def test_the_golden_cases_rotate_as_the_gpu_test_says(monkeypatch):
    """What the docstring of the GPU test of these cases states, counted from the host loop's trace, not from the code under test."""
    sc.install_cpu_kernels(monkeypatch)
    angles = []
    for case, img, labels, _ in sc.golden_cases():
        sc.seed_both(case["seed"])
        angles.append(sc.trace(sc.chain(), [img.shape[:2]], [labels])[0]["angle"])
    assert angles == [270, 90, 180, 0, 0, 90, 180, 0, 90, 0]


BRANCH_CONFIGS = {
    "default": dict(),
    "iou": dict(overlap_criterion='iou', bounds_validator=(0.02, 1.0), bounds_box_filter=(0.01, 1.0)),
    "center_point": dict(overlap_criterion='center_point'),
    "all_boxes": dict(n_boxes_min='all', bounds_validator=(0.1, 1.0)),
    "no_clip": dict(clip_boxes=False),
    "always": dict(random_flip=1.0, random_rotate=([270, 90], 1.0)),
    "never": dict(random_flip=0.0, random_rotate=([180], 0.0)),
}


@pytest.mark.parametrize("config", sorted(BRANCH_CONFIGS))
def test_restatement_equals_the_chain_on_the_branch_table(monkeypatch, config):
    sc.install_cpu_kernels(monkeypatch)
    ch = sc.chain(**BRANCH_CONFIGS[config])
    images, labels = sc.batch()
    if config == "default":
        found = sc.branches(sc.trace(ch, [im.shape[:2] for im in images], labels, sc.BRANCH_SEEDS))
        assert found >= sc.BRANCHES, sorted(sc.BRANCHES - found)
    want = sc.per_image(ch, images, labels, sc.BRANCH_SEEDS)
    for img, lab, seed, (px, lb, st) in zip(images, labels, sc.BRANCH_SEEDS, want):
        got_px, got_lb, got_st, _ = _walk_one(ch, img, lab, seed)
        assert np.array_equal(got_px, px), (config, seed)
        assert got_lb.dtype == lb.dtype and np.array_equal(got_lb, lb), (config, seed, got_lb, lb)
        assert np.array_equal(got_st, st), (config, seed, got_st[624], st[624])


def test_the_stream_seeds_do_what_the_cases_module_says(monkeypatch):
    sc.install_cpu_kernels(monkeypatch)
    images, labels = sc.batch()
    shapes = [im.shape[:2] for im in images]
    sc.seed_both(sc.BRANCH_STREAM_SEED)
    found = sc.branches(sc.trace(sc.chain(), shapes, labels))
    assert found >= sc.BRANCHES, sorted(sc.BRANCHES - found)
    sc.seed_both(sc.ROTATING_STREAM_SEED)
    angles = [r["angle"] for r in sc.trace(sc.chain(), shapes, labels) if r["angle"]]
    assert len(angles) >= 3 and set(angles) == {90, 180, 270}


def test_lazy_of_equals_the_image_the_chain_builds(monkeypatch):
    from ssd_keras_amd.data_generator import _image_ops as iop
    sc.install_cpu_kernels(monkeypatch)
    images, labels = sc.batch()
    seen = set()
    for img, lab, seed in zip(images, labels, sc.BRANCH_SEEDS):
        ch = sc.chain()
        ch.random_patch.sample_patch.background = (9, 80, 200)
        h, w = img.shape[:2]
        _, _, _, g = _walk_one(ch, img, lab, seed)
        sc.seed_both(seed)
        ch._draw()
        want = iop.GeoImage.of(h, w)
        for t in (ch.random_horizontal_flip, ch.random_vertical_flip, ch.random_rotate, ch.random_patch, ch.resize):
            want, lab = t(want, lab)
        got = ch._lazy_of(g, h, w)
        assert np.array_equal(got.ys, want.ys) and np.array_equal(got.xs, want.xs) and got.resized == want.resized
        assert got.background == want.background and got.transposed == want.transposed
        seen.add(int(g[7]))
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("layout,stream_seed", [("int64", "branches"), ("float64", "branches"), ("permuted", "branches"),
                                                ("int64", "rotating")])
def test_augment_batch_on_the_restatement_equals_the_call_loop(monkeypatch, layout, stream_seed):
    """The Python around the kernel -- packing, label dtype and column order, the angles drawn in advance, the write-back of np.random's
    state and the advance of Python's generator, the routes."""
    calls = []
    sc.install_cpu_kernels(monkeypatch, calls)
    images, labels = sc.batch()
    ch = sc.chain()
    if layout == "float64":
        labels = [lab.astype(np.float64) for lab in labels]
    elif layout == "permuted":
        ch = sc.chain(labels_format={'class_id': 4, 'xmin': 2, 'ymin': 0, 'xmax': 3, 'ymax': 1})
        labels = [lab[:, [2, 4, 1, 3, 0]] for lab in labels]
    seed = sc.BRANCH_STREAM_SEED if stream_seed == "branches" else sc.ROTATING_STREAM_SEED
    # ---- stream mode: both generators go on behind the batch ----
    sc.seed_both(seed)
    want = sc.call_loop(ch, images, labels)
    want_state, want_py = np.random.get_state(), random.getstate()
    sc.seed_both(seed)
    assert random.getstate() != want_py
    got_img, got_lab = ch.augment_batch(images, labels)
    assert calls == ["stream_ragged"]
    sc.assert_equal(got_img, got_lab, want)
    assert sc.same_state(np.random.get_state(), want_state) and random.getstate() == want_py
    # ---- the forced host path gives the same and launches no decision kernel ----
    monkeypatch.setenv("SSDHIP_AUG_HOST_STREAM", "1")
    sc.seed_both(seed)
    got_img, got_lab = ch.augment_batch(images, labels)
    assert calls == ["stream_ragged"]
    sc.assert_equal(got_img, got_lab, want)
    assert sc.same_state(np.random.get_state(), want_state) and random.getstate() == want_py
    monkeypatch.delenv("SSDHIP_AUG_HOST_STREAM")
    # ---- seeded mode: per-image streams, both generators untouched ----
    want = sc.per_image(ch, images, labels, sc.BRANCH_SEEDS)
    before, before_py = np.random.get_state(), random.getstate()
    got_img, got_lab = ch.augment_batch(images, labels, seeds=sc.BRANCH_SEEDS)
    assert calls == ["stream_ragged", "decide"]
    assert sc.same_state(np.random.get_state(), before) and random.getstate() == before_py
    sc.assert_equal(got_img, got_lab, want, ch._last_generator_states)
    # ---- fractional labels: the host code, stream and seeded, same results ----
    frac = [lab.astype(np.float64) + 0.25 for lab in labels]
    sc.seed_both(seed)
    want = sc.call_loop(ch, images, frac)
    want_state, want_py = np.random.get_state(), random.getstate()
    sc.seed_both(seed)
    got_img, got_lab = ch.augment_batch(images, frac)
    sc.assert_equal(got_img, got_lab, want)
    assert sc.same_state(np.random.get_state(), want_state) and random.getstate() == want_py
    before, before_py = np.random.get_state(), random.getstate()
    want = sc.per_image(ch, images, frac, sc.BRANCH_SEEDS)
    got_img, got_lab = ch.augment_batch(images, frac, seeds=sc.BRANCH_SEEDS)
    assert calls == ["stream_ragged", "decide"]
    assert sc.same_state(np.random.get_state(), before) and random.getstate() == before_py
    sc.assert_equal(got_img, got_lab, want, ch._last_generator_states)


def test_data_generator_routes_the_chain_when_labels_are_present():
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    images, _ = sc.batch(B=3)
    grey = images[0][:, :, 0]
    assert DataGenerator._batch_path([sc.chain()], images + [grey], True) == 'satellite'
    assert DataGenerator._batch_path([sc.chain()], images, False) is None
    assert DataGenerator._batch_path([sc.chain(), sc.chain()], images, True) is None


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
        q = nat._SatAugParams()
        d = dict(sc.chain()._device_params(), img_height=40, img_width=48)
        d.update(kw)
        for k, v in d.items():
            target = q if k in ("vflip_prob", "rotate_prob") else q.var
            if isinstance(v, list):
                for i, e in enumerate(v):
                    getattr(target, k)[i] = e
            else:
                setattr(target, k, v)
        return q

    bad_params = (dict(photo_prob=[0.5, 0.5, 1.5, 0.5]), dict(patch_prob=-0.1), dict(flip_prob=float("nan")), dict(vflip_prob=1.5),
                  dict(vflip_prob=float("nan")), dict(rotate_prob=-0.5), dict(rotate_prob=2.0), dict(min_scale=0.0), dict(n_trials=-1),
                  dict(criterion=3), dict(out_height=0), dict(interpolation=5))
    forms = {"ssdhip_sat_augment_decide": (True, True), "ssdhip_sat_augment_decide_stream": (False, False),
             "ssdhip_sat_augment_decide_stream_ragged": (True, False)}
    for name, (has_table, table_optional) in forms.items():
        fn = getattr(lib, name)

        def rc(q, B=2, n_max=3, table=a, ptrs=(a,) * 10):
            return fn(ctypes.byref(q) if q is not None else None, B, n_max, *(((table,) if has_table else ()) + tuple(ptrs)), None)

        assert rc(None) == -1
        assert rc(params(), B=0) == -1 and rc(params(), n_max=65) == -1
        for k in range(10):
            assert rc(params(), ptrs=(a,) * k + (None,) + (a,) * (9 - k)) == -1, (name, k)
        for bad in bad_params:
            assert rc(params(**bad)) == -1, (name, bad)
        if has_table and not table_optional:
            assert rc(params(), table=None) == -1
        if not has_table or table_optional:
            kw = dict(table=None) if has_table else {}
            assert rc(params(img_height=0), **kw) == -1
    for name, lead in (("ssdhip_sat_augment_plans", (2, 40, 48)), ("ssdhip_sat_augment_plans_ragged", None)):
        fn = getattr(lib, name)

        def rc(B=2, out_h=30, out_w=36, n_taps=8, ptrs=(a,) * 6):
            head = (a, B) + lead[1:] if lead is not None else (a, a, B)
            return fn(*(head + (out_h, out_w, n_taps) + tuple(ptrs) + (None,)))

        assert rc(B=0) == -1 and rc(out_h=0) == -1 and rc(n_taps=7) == -1 and rc(n_taps=65) == -1
        for k in range(6):
            assert rc(ptrs=(a,) * k + (None,) + (a,) * (5 - k)) == -1, (name, k)
    turn = lib.ssdhip_image_resize_gather_turn_cv_u8
    assert turn(a, a, 2, 40, 48, 30, 36, 3, a, a, a, 8, a, a, 8, None, a, None) == -1
    assert turn(a, a, 2, 40, 48, 30, 36, 3, a, a, a, 1, a, a, 8, a, a, None) == -1
    ragged = lib.ssdhip_image_resize_gather_turn_ragged_u8
    assert ragged(a, a, a, 2, 30, 36, a, a, a, 8, a, a, 8, None, a, None) == -1
    assert ragged(a, None, a, 2, 30, 36, a, a, a, 8, a, a, 8, a, a, None) == -1
