"""COCO bbox evaluation, host side (no GPU): the restatement tests/np_cocoeval.py against the hand cases, the COCO loader, loadRes,
the parameter defaults and caps, and summarize()'s printed lines."""
import json

import numpy as np
import pytest

from tests import coco_eval_hand_cases as hc
from tests import np_cocoeval as ref


def _coco(dataset):
    from ssd_keras_amd.eval_utils.coco_eval import COCO
    c = COCO()
    c.dataset = dataset
    c.createIndex()
    return c


def _restated(case):
    ev, acc = ref.run(case["gts"], case["dts"], case["images"], case["categories"], case["params"])
    img_index = {v: i for i, v in enumerate(ev["imgIds"])}
    cat_index = {v: k for k, v in enumerate(ev["catIds"])}

    def matches(img, cat):
        return ev["pairs"][(cat_index[cat] if cat is not None else 0, img_index[img])]
    return matches, acc


@pytest.mark.parametrize("case", hc.CASES, ids=[c["name"] for c in hc.CASES])
def test_restatement_reproduces_the_hand_cases(case):
    matches, acc = _restated(case)
    hc.check(case, matches, acc["precision"], acc["recall"], ref.summarize(acc))


def test_hand_case_premises():
    """What the hand cases lean on: the default thresholds are these doubles."""
    p = ref.default_params()
    assert p["iouThrs"][0] == 0.5 and p["iouThrs"][5] == 0.75 and len(p["iouThrs"]) == 10
    assert p["recThrs"][50] == 0.5 and len(p["recThrs"]) == 101
    assert ref.iou([0, 0, 10, 5], [0, 0, 10, 10], 0) == 0.5 and ref.iou([0, 0, 16, 12], [0, 0, 16, 16], 0) == 0.75
    assert ref.iou([15, 15, 10, 10], [0, 0, 20, 20], 1) == 0.25          # crowd: the union is the detection's area
    assert hc.ONE_MINUS == 1.0 / (0.0 + 1.0 + np.spacing(1))


def test_coco_loader(tmp_path):
    from ssd_keras_amd.eval_utils.coco_eval import COCO
    case = hc.CASES[2]
    ds = hc.dataset(case)
    ds["images"].append(dict(id=7))
    ds["annotations"].append(dict(id=9, image_id=7, category_id=1, bbox=[1, 2, 3, 4], area=12, iscrowd=0))
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(ds))
    c = COCO(str(path))
    assert sorted(c.getImgIds()) == [1, 7] and c.getCatIds() == [1]
    assert sorted(c.anns) == [1, 2, 9] and sorted(c.imgs) == [1, 7] and sorted(c.cats) == [1]
    assert [a["id"] for a in c.imgToAnns[1]] == [1, 2] and c.catToImgs[1] == [1, 1, 7]
    assert c.getAnnIds() == [1, 2, 9]
    assert c.getAnnIds(imgIds=[7]) == [9] and c.getAnnIds(imgIds=7) == [9]
    assert c.getAnnIds(imgIds=[1, 7], catIds=[1]) == [1, 2, 9] and c.getAnnIds(catIds=[5]) == []
    assert c.getAnnIds(imgIds=[1], iscrowd=1) == [1]
    assert [a["bbox"] for a in c.loadAnns([9])] == [[1, 2, 3, 4]] and c.loadAnns(9)[0]["area"] == 12
    assert c.getImgIds(catIds=[1]) in ([1, 7], [7, 1])


def test_load_res_from_file_list_and_array(tmp_path):
    case = hc.CASES[2]
    gt = _coco(hc.dataset(case))
    plain = [dict(image_id=d["image_id"], category_id=d["category_id"], bbox=d["bbox"], score=d["score"]) for d in case["dts"]]
    path = tmp_path / "results.json"
    path.write_text(json.dumps(plain))
    arr = np.array([[d["image_id"]] + d["bbox"] + [d["score"], d["category_id"]] for d in plain], dtype=np.float64)
    loaded = [gt.loadRes(str(path)), gt.loadRes(plain), gt.loadRes(arr)]
    for res in loaded:
        anns = res.dataset["annotations"]
        assert [a["id"] for a in anns] == [1, 2, 3, 4]
        assert [a["area"] for a in anns] == [100, 100, 100, 100] and all(a["iscrowd"] == 0 for a in anns)
        assert [a["bbox"] for a in anns] == [d["bbox"] for d in plain] and [a["score"] for a in anns] == [d["score"] for d in plain]
        assert [a["image_id"] for a in anns] == [1] * 4 and [a["category_id"] for a in anns] == [1] * 4
        assert res.getImgIds() == gt.getImgIds() and sorted(res.anns) == [1, 2, 3, 4]
    assert "id" not in plain[0]                                      # the caller's dicts are left alone
    assert gt.loadRes([]).dataset["annotations"] == []


def test_load_res_errors():
    gt = _coco(hc.dataset(hc.CASES[2]))
    with pytest.raises(AssertionError):
        gt.loadRes([dict(image_id=99, category_id=1, bbox=[0, 0, 1, 1], score=0.5)])
    with pytest.raises(ValueError, match="bbox"):
        gt.loadRes([dict(image_id=1, category_id=1, segmentation=dict(size=[1, 1], counts="0"), score=0.5)])
    with pytest.raises(ValueError, match="bbox"):
        gt.loadRes([dict(image_id=1, category_id=1, keypoints=[0] * 51, score=0.5)])
    with pytest.raises(ValueError):
        gt.loadRes(np.zeros((3, 6)))


def test_parameter_defaults():
    from ssd_keras_amd.eval_utils.coco_eval import COCOeval
    gt = _coco(hc.dataset(hc.CASES[8]))
    ev = COCOeval(cocoGt=gt, cocoDt=gt.loadRes([]), iouType="bbox")
    p, want = ev.params, ref.default_params()
    assert p.imgIds == [1] and p.catIds == [1, 2, 3]
    assert np.array_equal(p.iouThrs, np.linspace(.5, .95, int(np.round((.95 - .5) / .05)) + 1))
    assert np.array_equal(p.recThrs, np.linspace(0, 1, 101)) and np.array_equal(p.recThrs, want["recThrs"])
    assert p.maxDets == [1, 10, 100]
    assert p.areaRng == [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
    assert p.areaRngLbl == ["all", "small", "medium", "large"] and p.useCats == 1
    assert ev.evalImgs == [] and "not populated" in COCOeval.__doc__.replace("NOT", "not")


def test_only_bbox():
    from ssd_keras_amd.eval_utils.coco_eval import COCOeval
    for kind in ("segm", "keypoints"):
        with pytest.raises(ValueError, match="only 'bbox' is implemented"):
            COCOeval(iouType=kind)


@pytest.mark.parametrize("name, value", [("iouThrs", np.linspace(0.1, 0.9, 33)), ("iouThrs", []), ("areaRng", [[0, 1]] * 9),
                                         ("maxDets", list(range(1, 10))), ("maxDets", [0, 10]), ("maxDets", [1.5]),
                                         ("recThrs", np.linspace(0, 1, 1025)), ("recThrs", [0.5, 0.2])])
def test_caps_raise_before_any_device_work(name, value):
    """A value beyond a cap raises ValueError at evaluate() (before the GPU is touched); nothing is truncated."""
    from ssd_keras_amd.eval_utils.coco_eval import COCOeval
    gt = _coco(hc.dataset(hc.CASES[7]))
    ev = COCOeval(gt, gt.loadRes(hc.CASES[7]["dts"]))
    setattr(ev.params, name, value)
    with pytest.raises(ValueError, match=name):
        ev.evaluate()


def test_summarize_prints_the_twelve_lines(capsys):
    """summarize() on case (h)'s accumulated arrays (taken from the restatement: accumulate() itself needs the GPU)."""
    from ssd_keras_amd.eval_utils.coco_eval import COCOeval
    case = hc.CASES[7]
    assert case["name"] == "h_tp_fp_tp"
    _, acc = _restated(case)
    gt = _coco(hc.dataset(case))
    ev = COCOeval(gt, gt.loadRes(case["dts"]))
    ev.eval = dict(params=ev.params, precision=acc["precision"], recall=acc["recall"], scores=acc["scores"])
    capsys.readouterr()
    ev.summarize()
    assert capsys.readouterr().out.splitlines() == hc.SUMMARY_H
    assert np.all(np.abs(ev.stats - np.asarray(case["expect"]["stats"], dtype=np.float64)) <= 1e-12)
    with pytest.raises(RuntimeError):
        COCOeval(gt, gt.loadRes([])).summarize()


def test_evaluate_needs_a_gpu(monkeypatch):
    """There is no CPU path: without a GPU evaluate() raises."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from ssd_keras_amd._native import SsdHipError
    from ssd_keras_amd.eval_utils.coco_eval import COCOeval
    gt = _coco(hc.dataset(hc.CASES[7]))
    with pytest.raises(SsdHipError, match="GPU"):
        COCOeval(gt, gt.loadRes(hc.CASES[7]["dts"])).evaluate()
