"""DataGenerator without a GPU: its call surface, the parsers and the per-image `generate()` loop against the reference's own results
(tests/golden/data_generator.npz, made by tests/golden/make_data_generator_golden.py), parse_xml on hand-written VOC files, the pickled
dataset round trip, and the host-side argument checks of the ragged-batch exports."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

from tests import data_generator_cases as dc
from tests import util

GOLDEN = os.path.join(util.GOLDEN, "data_generator.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _ns():
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    return types.SimpleNamespace(DataGenerator=DataGenerator)


def _compare(got, golden, prefix):
    keys = sorted(k for k in golden if k.startswith(prefix))
    assert keys and sorted(k for k in got if k.startswith(prefix)) == keys
    for k in keys:
        assert got[k].shape == golden[k].shape, k
        np.testing.assert_array_equal(got[k], golden[k], err_msg=k)


def test_api_surface_matches_reference():
    """Parameter names, order and defaults == the reference's; generate() adds `device=None` behind them."""
    from tests import api_surface
    import ssd_keras_amd
    with open(os.path.join(util.GOLDEN, "api_surface_data_generator.json")) as f:
        want = json.load(f)
    root = os.path.dirname(os.path.abspath(ssd_keras_amd.__file__))
    got = api_surface.extract(root, surface={m: list(d) for m, d in want.items()})
    for module, entries in want.items():
        for qual, params in entries.items():
            expect = [list(p) for p in params] + ([["device", "None"]] if qual == "DataGenerator.generate" else [])
            assert got[module][qual] is not None, (module, qual)
            assert [list(p) for p in got[module][qual]] == expect, (module, qual)


def test_parsers_match_reference(golden):
    out = {}
    dc.record_parsers(_ns(), out)
    _compare(out, golden, "csv_")
    _compare(out, golden, "json_")


def test_generate_without_transformations_matches_reference(golden):
    """Order, removal of the image without ground truth, every return, the degenerate-box warning and the epoch wrap."""
    out = {}
    dc.run_plain(_ns(), out)
    _compare(out, golden, "plain_")
    assert "degenerate" in str(golden["plain_b0_warnings"][0])


VOC_XML = """<annotation><folder>VOC2007</folder><filename>{id}.jpg</filename>
<size><width>100</width><height>80</height><depth>3</depth></size>
{objects}</annotation>"""
VOC_OBJ = """<object><name>{name}</name><pose>Left</pose><truncated>{t}</truncated><difficult>{d}</difficult>
<bndbox><xmin>{x0}</xmin><ymin>{y0}</ymin><xmax>{x1}</xmax><ymax>{y1}</ymax></bndbox></object>"""


def _voc(tmp_path):
    ann = tmp_path / "Annotations"
    ann.mkdir()
    objs = {"000001": [("dog", 0, 0, 1, 2, 30, 40), ("person", 1, 0, 5, 6, 50, 60)],
            "000002": [("car", 0, 1, 10, 11, 20, 21), ("cat", 1, 1, 3, 4, 9, 9), ("dog", 0, 0, 0, 0, 99, 79)]}
    for image_id, rows in objs.items():
        body = "".join(VOC_OBJ.format(name=n, t=t, d=d, x0=a, y0=b, x1=c, y1=e) for n, t, d, a, b, c, e in rows)
        (ann / (image_id + ".xml")).write_text(VOC_XML.format(id=image_id, objects=body))
    sets = tmp_path / "trainval.txt"
    sets.write_text("000001\n000002\n")
    return str(tmp_path / "JPEGImages"), str(sets), str(ann)


def test_parse_xml_hand_derived(tmp_path):
    """Classes -> VOC ids (dog 12, person 15, car 7, cat 8), `difficult` -> eval_neutral, the truncated / difficult filters."""
    images_dir, sets, ann = _voc(tmp_path)
    g = _ns().DataGenerator()
    images, filenames, labels, ids, neutral = g.parse_xml([images_dir], [sets], [ann], ret=True, verbose=False)
    assert images is None and ids == ["000001", "000002"]
    assert filenames == [os.path.join(images_dir, "000001.jpg"), os.path.join(images_dir, "000002.jpg")]
    assert labels == [[[12, 1, 2, 30, 40], [15, 5, 6, 50, 60]], [[7, 10, 11, 20, 21], [8, 3, 4, 9, 9], [12, 0, 0, 99, 79]]]
    assert neutral == [[False, False], [True, True, False]]
    g.parse_xml([images_dir], [sets], [ann], exclude_truncated=True, verbose=False)
    assert g.labels == [[[12, 1, 2, 30, 40]], [[7, 10, 11, 20, 21], [12, 0, 0, 99, 79]]] and g.eval_neutral == [[False], [True, False]]
    g.parse_xml([images_dir], [sets], [ann], exclude_difficult=True, include_classes=[12, 8], verbose=False)
    assert g.labels == [[[12, 1, 2, 30, 40]], [[12, 0, 0, 99, 79]]] and g.eval_neutral == [[False], [False]]
    g.parse_xml([images_dir], [sets], verbose=False)
    assert g.labels is None and g.eval_neutral is None and g.get_dataset_size() == 2


def test_save_and_get_dataset_round_trip(tmp_path):
    DataGenerator = _ns().DataGenerator
    g = dc.csv_generator(_ns())
    paths = [str(tmp_path / n) for n in ("f.pkl", "l.pkl", "i.pkl", "e.pkl")]
    g.eval_neutral = [[False] * len(v) for v in g.labels]
    g.save_dataset(*paths)
    h = DataGenerator(filenames=paths[0], filenames_type='pickle', labels=paths[1], image_ids=paths[2], eval_neutral=paths[3])
    for a, b in zip(g.get_dataset(), h.get_dataset()):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    assert h.get_dataset_size() == g.get_dataset_size() == 8
    text = tmp_path / "names.txt"
    text.write_text("img_a.png\nimg_b.png\n")
    t = DataGenerator(filenames=str(text), images_dir=dc.FIXTURES)
    assert t.filenames == [os.path.join(dc.FIXTURES, "img_a.png"), os.path.join(dc.FIXTURES, "img_b.png")]


def test_dataset_errors():
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator, DatasetError, DegenerateBatchError
    assert issubclass(DegenerateBatchError, Exception)
    with pytest.raises(DatasetError, match="did not load a dataset"):
        next(DataGenerator().generate())
    with pytest.raises(DatasetError, match="HDF5"):
        DataGenerator(hdf5_dataset_path="dataset.h5")
    with pytest.raises(DatasetError, match="HDF5"):
        dc.csv_generator(_ns()).create_hdf5_dataset()


@pytest.fixture(scope="module")
def lib():
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd import build
    assert build.build() == nat.lib_path()
    return nat.load()


def test_ragged_exports_reject_bad_arguments(lib):
    """Null pointers and out-of-range sizes: SSDHIP_E_BADARG (-1) before any launch."""
    from ssd_keras_amd import _native as nat
    buf = (ctypes.c_ubyte * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    gather = lib.ssdhip_image_resize_gather_ragged_u8
    good = dict(x=a, table=a, y=a, B=2, Ho=8, Wo=8, plan=a, ix=a, wx=a, nx=2, iy=a, wy=a, ny=2, bg=a)
    for bad in ({"x": None}, {"table": None}, {"bg": None}, {"B": 0}, {"B": 70000}, {"Ho": 0}, {"Wo": -1}, {"nx": 1}, {"ny": 65}):
        kw = dict(good, **bad)
        assert gather(*kw.values(), None) == -1, bad
    prog = lib.ssdhip_image_program_ragged_u8
    assert prog(None, a, a, 2, 16, a, a, None) == -1
    assert prog(a, None, a, 2, 16, a, a, None) == -1
    assert prog(a, a, a, 0, 16, a, a, None) == -1
    assert prog(a, a, a, 2, 0, a, a, None) == -1
    assert prog(ctypes.c_void_p(ctypes.addressof(buf) + 1), a, a, 2, 16, a, a, None) == -1             # not dword-aligned
    plans = lib.ssdhip_augment_plans_ragged
    assert plans(a, None, 2, 300, 300, 8, a, a, a, a, a, None) == -1
    assert plans(a, a, 2, 300, 300, 7, a, a, a, a, a, None) == -1
    assert plans(a, a, 2, 0, 300, 8, a, a, a, a, a, None) == -1
    assert plans(a, a, 0, 300, 300, 8, a, a, a, a, a, None) == -1
    q, ph = nat._AugParams(), nat._AugPhoto()
    q.img_height = q.img_width = q.out_height = q.out_width = 300
    q.n_bounds = q.n_modes = q.n_trials = 1
    q.expand_min_scale, q.expand_max_scale, q.crop_min_scale, q.crop_max_scale = 1.0, 4.0, 0.3, 1.0
    decide = lib.ssdhip_ssd_augment_decide_stream_ragged
    assert decide(ctypes.byref(q), ctypes.byref(ph), 2, None, *([a] * 9), None) == -1
    assert decide(ctypes.byref(q), ctypes.byref(ph), 0, a, *([a] * 9), None) == -1
    ph.swap_prob = 0.5
    assert decide(ctypes.byref(q), ctypes.byref(ph), 2, a, *([a] * 9), None) == -1
    ph.swap_prob = 0.0
    q.img_height = 0
    assert decide(ctypes.byref(q), ctypes.byref(ph), 2, a, *([a] * 9), None) == -1
