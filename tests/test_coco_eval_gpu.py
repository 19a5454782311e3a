"""COCO bbox evaluation on the device (ssd_keras_amd/eval_utils/coco_eval.py, csrc/ssdhip_cocoeval.hip) against the hand cases and
against the restatement tests/np_cocoeval.py.  Needs an MI355X.  Bar: matches and flags exact, precision / recall / scores
bit-identical float64, the twelve statistics of the hand cases to 1e-12."""
import functools
import json

import numpy as np
import pytest

from tests import coco_eval_hand_cases as hc
from tests import np_cocoeval as ref

pytestmark = pytest.mark.gpu

IMAGES = [3 * i + 1 for i in range(40)]
CATS = [1, 2, 4, 7, 9, 11]


def _coco(dataset):
    from ssd_keras_amd.eval_utils.coco_eval import COCO
    c = COCO()
    c.dataset = dataset
    c.createIndex()
    return c


def _dataset(images, cats, gts):
    return dict(images=[dict(id=i) for i in images], categories=[dict(id=c, name="c%d" % c) for c in cats], annotations=gts)


def _box(rng):
    """[x, y, w, h] on a half-pixel grid; h is a whole even number so h / 2 and 3 h / 4 stay on the grid."""
    return [rng.randint(0, 400) / 2.0, rng.randint(0, 400) / 2.0, rng.randint(2, 160) / 2.0, 2.0 * rng.randint(1, 40)]


def _det_near(rng, g):
    """A detection derived from ground-truth box g: a copy, exactly half or three quarters of its height (IoU 0.5 / 0.75 exactly:
    i = w h f, u = w h f + w h - w h f = w h, and (w h f) / (w h) is exact for f = 1/2, 3/4), a box inside it, or a half-pixel shift."""
    x, y, w, h = g
    kind = rng.randint(0, 5)
    if kind == 0:
        return [x, y, w, h]
    if kind == 1:
        return [x, y, w, h / 2.0]
    if kind == 2:
        return [x, y, w, 3.0 * h / 4.0]
    if kind == 3:
        return [x + w / 4.0 if (w / 4.0) % 0.5 == 0 else x, y, w / 2.0 if (w / 2.0) % 0.5 == 0 else w, h / 2.0]
    return [x + rng.randint(-4, 5) / 2.0, y + rng.randint(-4, 5) / 2.0, w, h]


def make_dataset(seed, images=IMAGES, cats=CATS, counts=None):
    """Ground truth and results (lists of dicts, shuffled so no pair is contiguous in the input).  Per pair 0-12 ground truths (about
    10 % crowds, areas drawn independently of the boxes over all three ranges) and 0-130 detections with scores of 3 decimals."""
    rng = np.random.RandomState(seed)
    gts, dts = [], []
    for img in images:
        for cat in cats:
            if counts is not None:
                G, D = counts
            else:
                G = int(rng.choice([0, 0, 0, 1, 1, 2, 3, 5, 8, 12]))
                u = rng.rand()
                D = 0 if u < 0.15 else (int(rng.randint(1, 25)) if u < 0.85 else int(rng.randint(95, 131)))
            mine = []
            for _ in range(G):
                b = _box(rng)
                mine.append(b)
                gts.append(dict(image_id=img, category_id=cat, bbox=b, area=float(np.round(10 ** rng.uniform(1.5, 4.5), 1)),
                                iscrowd=int(rng.rand() < 0.1)))
            for _ in range(D):
                b = _det_near(rng, mine[rng.randint(0, G)]) if G and rng.rand() < 0.6 else _box(rng)
                dts.append(dict(image_id=img, category_id=cat, bbox=b, score=float(np.round(rng.rand(), 3))))
    gts = [gts[i] for i in rng.permutation(len(gts))]
    dts = [dts[i] for i in rng.permutation(len(dts))]
    for i, g in enumerate(gts):
        g["id"] = i                                   # annotation id 0 exists: it must be credited like any other
    dts = [dict(d, id=i + 1) for i, d in enumerate(dts)]
    return gts, dts


@functools.lru_cache(maxsize=None)
def seeded(seed):
    gts, dts = make_dataset(seed)
    ev, acc = ref.run(gts, dts, IMAGES, CATS)
    return gts, dts, ev, acc


def device_eval(images, cats, gts, dts, imgIds=None, catIds=None, params=None):
    from ssd_keras_amd.eval_utils.coco_eval import COCOeval
    gt = _coco(_dataset(images, cats, gts))
    plain = [{k: v for k, v in d.items() if k != "id"} for d in dts]
    e = COCOeval(cocoGt=gt, cocoDt=gt.loadRes(plain), iouType="bbox")
    if imgIds is not None:
        e.params.imgIds = imgIds
    if catIds is not None:
        e.params.catIds = catIds
    for k, v in (params or {}).items():
        setattr(e.params, k, v)
    e.evaluate()
    e.accumulate()
    return e


def assert_same(e, ev, acc):
    """Device evaluator `e` against the restatement's (ev, acc): accumulated arrays bit for bit, every pair's matches exactly."""
    assert e.eval["counts"] == acc["counts"]
    for name in ("precision", "recall", "scores"):
        got, want = e.eval[name], acc[name]
        assert got.dtype == np.float64 and got.shape == want.shape
        bad = np.argwhere(got != want)
        assert np.array_equal(got, want), "%s differs at %d entries, first %s: %r != %r" % (
            name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    for (k, i), want in ev["pairs"].items():
        got = e.matches(ev["imgIds"][i], ev["catIds"][k] if ev["params"]["useCats"] else None)
        for name in ("dtIds", "dtScores", "dtMatches", "dtIgnore", "gtIds", "gtIgnore"):
            assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), (name, k, i, got[name], want[name])


@pytest.mark.parametrize("case", hc.CASES, ids=[c["name"] for c in hc.CASES])
def test_hand_cases_on_the_device(case, capsys):
    e = device_eval(case["images"], case["categories"], case["gts"], case["dts"], params=case["params"])
    e.summarize()
    assert len(capsys.readouterr().out.splitlines()) == 12
    hc.check(case, lambda img, cat: e.matches(img, cat), e.eval["precision"], e.eval["recall"], e.stats)
    if case["name"] == "h_tp_fp_tp":
        e.summarize()
        assert capsys.readouterr().out.splitlines() == hc.SUMMARY_H


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_dataset_exercises_the_hard_parts(seed):
    """On the CPU, with the restatement: each generated dataset really holds a tie at the 100-cut, an IoU equal to a threshold, a crowd
    matched twice, a pair without ground truth and a pair without detections."""
    gts, dts, ev, acc = seeded(seed)
    thrs = ev["params"]["iouThrs"]
    tie = on_thr = crowd_twice = no_gt = no_dt = 0
    for pr in ev["pairs"].values():
        no_gt += pr["gtIds"].size == 0
        no_dt += pr["dtIds"].size == 0
        on_thr += bool(np.isin(pr["ious"], thrs).any())
        m = pr["dtMatches"][0, 0]
        for g in np.nonzero(pr["gtCrowd"])[0]:
            crowd_twice += np.count_nonzero(m == g + 1) >= 2
    by_pair = {}
    for d in dts:
        by_pair.setdefault((d["image_id"], d["category_id"]), []).append(d["score"])
    for scores in by_pair.values():
        if len(scores) > 100:
            s = np.sort(-np.asarray(scores), kind="mergesort")
            tie += s[99] == s[100]
    assert tie and on_thr and crowd_twice and no_gt and no_dt, (tie, on_thr, crowd_twice, no_gt, no_dt)
    assert any(g["id"] == 0 for g in gts)
    for a in range(4):                                   # every area range is populated
        assert any((~pr["gtIgnore"][a]).any() for pr in ev["pairs"].values())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_dataset_equals_the_restatement(seed):
    gts, dts, ev, acc = seeded(seed)
    assert_same(device_eval(IMAGES, CATS, gts, dts), ev, acc)


def test_large_ground_truth_pair():
    """G = 300 and D = 100 in one pair: past what the matching kernel keeps in LDS (G <= 64, D * G <= 1536)."""
    gts, dts = make_dataset(7, images=[5], cats=[2], counts=(300, 100))
    ev, acc = ref.run(gts, dts, [5], [2])
    assert ev["pairs"][(0, 0)]["gtIds"].size == 300 and ev["pairs"][(0, 0)]["dtIds"].size == 100
    assert ev["pairs"][(0, 0)]["dtMatches"].any()
    assert_same(device_eval([5], [2], gts, dts), ev, acc)


def test_pair_sizes_around_the_lds_limits():
    """Pairs on both sides of the two limits of the LDS path: G = 64 / 65, and D * G = 1536 / 1537-ish (D = 24, G = 64; D = 100, G = 16)."""
    for seed, counts in ((11, (64, 24)), (12, (65, 23)), (13, (16, 96)), (14, (16, 97))):
        gts, dts = make_dataset(seed, images=[5, 6], cats=[2], counts=counts)
        ev, acc = ref.run(gts, dts, [5, 6], [2])
        assert_same(device_eval([5, 6], [2], gts, dts), ev, acc)


@pytest.mark.parametrize("variation", ["imgIds", "catIds", "thresholds_and_caps", "useCats0"])
def test_parameter_variations(variation):
    gts, dts, _, _ = seeded(0)
    imgIds, catIds, params = IMAGES, CATS, {}
    if variation == "imgIds":
        imgIds = IMAGES[5:30:3]
    elif variation == "catIds":
        catIds = [11, 2, 4]
    elif variation == "thresholds_and_caps":
        imgIds, params = IMAGES[:20], dict(iouThrs=[0.3, 0.5], maxDets=[5, 50])
    else:
        imgIds, params = IMAGES[:12], dict(useCats=0)
    ev, acc = ref.run(gts, dts, imgIds, catIds, params)
    e = device_eval(IMAGES, CATS, gts, dts, imgIds=imgIds, catIds=catIds, params=params)
    assert_same(e, ev, acc)
    if variation == "thresholds_and_caps":
        with pytest.raises(ValueError, match="three detection caps"):
            e.summarize()


def test_notebook_flow(tmp_path, capsys):
    """The notebook's cell: a results file as predict_all_to_json writes it (scores of 3 decimals, boxes of 1), loadRes, the four calls."""
    from ssd_keras_amd.eval_utils.coco_eval import COCO, COCOeval
    gts = [dict(id=11, image_id=139, category_id=1, bbox=[10.0, 20.0, 100.5, 200.25], area=12000.5, iscrowd=0),
           dict(id=12, image_id=139, category_id=18, bbox=[300.0, 50.0, 40.0, 30.0], area=900.0, iscrowd=0),
           dict(id=13, image_id=285, category_id=1, bbox=[0.0, 0.0, 400.0, 300.0], area=80000.0, iscrowd=1),
           dict(id=14, image_id=285, category_id=18, bbox=[5.0, 5.0, 60.0, 60.0], area=3000.0, iscrowd=0)]
    results = [{"image_id": 139, "category_id": 1, "score": 0.912, "bbox": [12.3, 18.9, 98.7, 203.1]},
               {"image_id": 139, "category_id": 1, "score": 0.455, "bbox": [200.0, 100.0, 50.5, 60.1]},
               {"image_id": 139, "category_id": 18, "score": 0.873, "bbox": [301.2, 49.5, 38.8, 31.0]},
               {"image_id": 285, "category_id": 1, "score": 0.671, "bbox": [50.0, 50.0, 100.0, 100.0]},
               {"image_id": 285, "category_id": 18, "score": 0.333, "bbox": [4.1, 6.2, 58.0, 61.3]},
               {"image_id": 285, "category_id": 18, "score": 0.333, "bbox": [150.0, 150.0, 20.0, 20.0]}]
    ann_file, results_file = tmp_path / "instances_val.json", tmp_path / "detections_val_results.json"
    ann_file.write_text(json.dumps(_dataset([139, 285, 632], [1, 18, 44], gts)))
    results_file.write_text(json.dumps(results))
    image_ids = [139, 285, 632]

    coco_gt = COCO(str(ann_file))
    coco_dt = coco_gt.loadRes(str(results_file))
    cocoEval = COCOeval(cocoGt=coco_gt, cocoDt=coco_dt, iouType='bbox')
    cocoEval.params.imgIds = image_ids
    cocoEval.evaluate()
    cocoEval.accumulate()
    capsys.readouterr()
    cocoEval.summarize()
    assert len(capsys.readouterr().out.splitlines()) == 12

    ev, acc = ref.run(gts, [dict(d, id=i + 1) for i, d in enumerate(results)], image_ids, [1, 18, 44])
    assert np.array_equal(cocoEval.stats, ref.summarize(acc))
    assert_same(cocoEval, ev, acc)
    assert cocoEval.stats[0] > 0.3                     # the detections do match: the numbers are not all zero or -1


def test_repeat_evaluation_keeps_no_stale_state():
    from ssd_keras_amd.eval_utils.coco_eval import COCOeval
    gts, dts, _, _ = seeded(1)
    e = device_eval(IMAGES, CATS, gts, dts, imgIds=IMAGES[:25])
    first = e.eval["precision"].copy()
    e.params.imgIds = IMAGES[30:]
    e.evaluate()
    with pytest.raises(RuntimeError):
        e.summarize()                                  # the first call's arrays are gone
    e.accumulate()
    ev, acc = ref.run(gts, dts, IMAGES[30:], CATS)
    assert_same(e, ev, acc)
    assert not np.array_equal(first, e.eval["precision"])
    with pytest.raises(KeyError):
        e.matches(IMAGES[0], CATS[0])
    assert isinstance(e, COCOeval)
