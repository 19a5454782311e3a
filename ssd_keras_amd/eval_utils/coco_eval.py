"""COCO bbox evaluation for the last cell of the reference's `ssd300_evaluation_COCO.ipynb`:

    from ssd_keras_amd.eval_utils.coco_eval import COCO, COCOeval
    coco_gt = COCO(annotations_file)
    coco_dt = coco_gt.loadRes(results_file)
    cocoEval = COCOeval(cocoGt=coco_gt, cocoDt=coco_dt, iouType='bbox')
    cocoEval.params.imgIds = image_ids
    cocoEval.evaluate(); cocoEval.accumulate(); cocoEval.summarize()

`COCO` and `COCOeval` carry pycocotools' names and call surface for the bounding-box protocol; pycocotools itself (a C extension
plus Python loops) is not a dependency.  The protocol is restated in `tests/np_cocoeval.py`.  `COCO` is host code (JSON, dicts);
`COCOeval.evaluate()` uploads flat arrays once and runs the grouping, the ordering and the greedy matching of every (image,
category) pair on the GPU, `accumulate()` the per-category sorts, cumulative sums, precision envelopes and recall-threshold
look-ups (`csrc/ssdhip_cocoeval.hip`); the host downloads `precision`, `recall` and `scores`.  There is no CPU path.

Differences from pycocotools, all deliberate:
  * only `iouType='bbox'`;
  * `evalImgs` is not populated -- `COCOeval.matches(imgId, catId)` downloads one pair's rows instead;
  * matches are recorded as index + 1 into the pair's ground truth, not as annotation ids, so a ground truth whose id is 0 is
    credited like any other (pycocotools tests `== 0` for "unmatched" and never credits it);
  * a detection's area is its box's `w * h` (what `loadRes` stores as `area`);
  * caps, beyond which `evaluate()` raises `ValueError`: at most 32 IoU thresholds, 8 area ranges, 8 detection caps (positive
    integers) and 1024 recall thresholds (non-decreasing).
"""
from __future__ import annotations

import copy
import datetime
import json
from collections import defaultdict

import numpy as np

MAX_IOU_THRS, MAX_AREA_RNG, MAX_MAX_DETS, MAX_REC_THRS = 32, 8, 8, 1024


class COCO:
    """Host-side loader of a COCO annotation file (detection subset of pycocotools.coco.COCO)."""

    def __init__(self, annotation_file=None):
        self.dataset, self.anns, self.cats, self.imgs = dict(), dict(), dict(), dict()
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        if annotation_file is not None:
            with open(annotation_file, 'r') as f:
                dataset = json.load(f)
            assert type(dataset) == dict, 'annotation file format {} not supported'.format(type(dataset))
            self.dataset = dataset
            self.createIndex()

    def createIndex(self):
        anns, cats, imgs = {}, {}, {}
        imgToAnns, catToImgs = defaultdict(list), defaultdict(list)
        for ann in self.dataset.get('annotations', []):
            imgToAnns[ann['image_id']].append(ann)
            anns[ann['id']] = ann
        for img in self.dataset.get('images', []):
            imgs[img['id']] = img
        for cat in self.dataset.get('categories', []):
            cats[cat['id']] = cat
        if 'categories' in self.dataset:
            for ann in self.dataset.get('annotations', []):
                catToImgs[ann['category_id']].append(ann['image_id'])
        self.anns, self.imgToAnns, self.catToImgs, self.imgs, self.cats = anns, imgToAnns, catToImgs, imgs, cats
        self._flat_cache = None

    @staticmethod
    def _list(v):
        return list(v) if isinstance(v, (list, tuple, set, np.ndarray)) else [v]

    def getImgIds(self, imgIds=[], catIds=[]):
        imgIds, catIds = self._list(imgIds), self._list(catIds)
        if len(imgIds) == len(catIds) == 0:
            ids = self.imgs.keys()
        else:
            ids = set(imgIds)
            for i, catId in enumerate(catIds):
                if i == 0 and len(ids) == 0:
                    ids = set(self.catToImgs[catId])
                else:
                    ids &= set(self.catToImgs[catId])
        return list(ids)

    def getCatIds(self, catNms=[], supNms=[], catIds=[]):
        catNms, supNms, catIds = self._list(catNms), self._list(supNms), self._list(catIds)
        cats = self.dataset.get('categories', [])
        if catNms:
            cats = [c for c in cats if c['name'] in catNms]
        if supNms:
            cats = [c for c in cats if c.get('supercategory') in supNms]
        if catIds:
            cats = [c for c in cats if c['id'] in catIds]
        return [c['id'] for c in cats]

    def getAnnIds(self, imgIds=[], catIds=[], areaRng=[], iscrowd=None):
        imgIds, catIds = self._list(imgIds), self._list(catIds)
        if len(imgIds) == len(catIds) == len(areaRng) == 0:
            anns = self.dataset.get('annotations', [])
        else:
            if len(imgIds) != 0:
                anns = [a for imgId in imgIds if imgId in self.imgToAnns for a in self.imgToAnns[imgId]]
            else:
                anns = self.dataset.get('annotations', [])
            if len(catIds) != 0:
                cs = set(catIds)
                anns = [a for a in anns if a['category_id'] in cs]
            if len(areaRng) != 0:
                anns = [a for a in anns if a['area'] > areaRng[0] and a['area'] < areaRng[1]]
        if iscrowd is not None:
            return [a['id'] for a in anns if a['iscrowd'] == iscrowd]
        return [a['id'] for a in anns]

    def loadAnns(self, ids=[]):
        if isinstance(ids, (list, tuple, np.ndarray)):
            return [self.anns[i] for i in ids]
        return [self.anns[ids]]

    def loadRes(self, resFile):
        """A results COCO object from a results JSON path, a list of result dicts or an (N, 7) float array
        [image_id, x, y, w, h, score, category_id].  Every result gets area = w * h, id = position + 1 and iscrowd = 0."""
        res = COCO()
        res.dataset['images'] = [img for img in self.dataset.get('images', [])]
        if isinstance(resFile, str):
            with open(resFile) as f:
                anns = json.load(f)
        elif isinstance(resFile, np.ndarray):
            data = np.asarray(resFile)
            if data.ndim != 2 or data.shape[1] != 7:
                raise ValueError("a results array must be (N, 7): [image_id, x, y, w, h, score, category_id]")
            anns = [{'image_id': int(r[0]), 'bbox': [float(r[1]), float(r[2]), float(r[3]), float(r[4])], 'score': float(r[5]),
                     'category_id': int(r[6])} for r in data]
        else:
            anns = resFile
        assert type(anns) == list, 'results in not an array of objects'
        missing = set(a['image_id'] for a in anns) - set(self.getImgIds())
        assert not missing, 'Results do not correspond to current coco set'
        if anns and 'bbox' not in anns[0]:
            raise ValueError("only bounding-box results are implemented: a result has no 'bbox' key")
        res.dataset['categories'] = copy.deepcopy(self.dataset.get('categories', []))
        out = []
        for pos, a in enumerate(anns):
            if 'bbox' not in a:
                raise ValueError("only bounding-box results are implemented: a result has no 'bbox' key")
            a = dict(a)
            bb = a['bbox']
            a['area'] = bb[2] * bb[3]
            a['id'] = pos + 1
            a['iscrowd'] = 0
            out.append(a)
        res.dataset['annotations'] = out
        res.createIndex()
        return res

    def _flat(self):
        """The annotations as flat arrays in file order (built once per object): image_id, category_id, bbox, area, iscrowd, score, id."""
        if getattr(self, '_flat_cache', None) is None:
            anns = self.dataset.get('annotations', [])
            n = len(anns)
            self._flat_cache = dict(
                image_id=np.fromiter((a['image_id'] for a in anns), dtype=np.int64, count=n),
                category_id=np.fromiter((a['category_id'] for a in anns), dtype=np.int64, count=n),
                bbox=np.array([a['bbox'] for a in anns], dtype=np.float64).reshape(n, 4),
                area=np.fromiter((a.get('area', 0.0) for a in anns), dtype=np.float64, count=n),
                iscrowd=np.fromiter((1 if a.get('iscrowd', 0) else 0 for a in anns), dtype=np.uint8, count=n),
                score=np.fromiter((a.get('score', 0.0) for a in anns), dtype=np.float64, count=n),
                id=np.fromiter((a['id'] for a in anns), dtype=np.int64, count=n))
        return self._flat_cache


class Params:
    """Evaluation parameters (pycocotools.cocoeval.Params for iouType='bbox')."""

    def __init__(self, iouType='bbox'):
        if iouType != 'bbox':
            raise ValueError("iouType %r: only 'bbox' is implemented" % (iouType,))
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.iouType = iouType


class COCOeval:
    """Bounding-box COCOeval on the GPU: evaluate(), accumulate(), summarize() with pycocotools' roles.

    `evalImgs` is NOT populated (it stays an empty list): per-pair results stay on the device, `matches(imgId, catId)` downloads one
    pair's.  Matches are index + 1 into the pair's ground truth (`gtIds`), 0 = unmatched -- not annotation ids."""

    def __init__(self, cocoGt=None, cocoDt=None, iouType='bbox'):
        if iouType != 'bbox':
            raise ValueError("iouType %r: only 'bbox' is implemented" % (iouType,))
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.evalImgs = []
        self.eval = {}
        self.params = Params(iouType=iouType)
        self._paramsEval = {}
        self.stats = []
        self._dev = None
        if cocoGt is not None:
            self.params.imgIds = sorted(cocoGt.getImgIds())
            self.params.catIds = sorted(cocoGt.getCatIds())

    # -- evaluate ---------------------------------------------------------------------------------------------------------------
    def _checked_params(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        if p.useCats:
            p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        iou, rec, rng = np.asarray(p.iouThrs, dtype=np.float64).reshape(-1), np.asarray(p.recThrs, dtype=np.float64).reshape(-1), \
            np.asarray(p.areaRng, dtype=np.float64)
        if not 1 <= iou.size <= MAX_IOU_THRS:
            raise ValueError("iouThrs: 1 to %d thresholds are supported, got %d" % (MAX_IOU_THRS, iou.size))
        if rng.ndim != 2 or rng.shape[1] != 2 or not 1 <= rng.shape[0] <= MAX_AREA_RNG:
            raise ValueError("areaRng: 1 to %d [lo, hi] ranges are supported" % MAX_AREA_RNG)
        if not 1 <= len(p.maxDets) <= MAX_MAX_DETS:
            raise ValueError("maxDets: 1 to %d caps are supported, got %d" % (MAX_MAX_DETS, len(p.maxDets)))
        if any(int(m) != m or m < 1 or m > 2 ** 30 for m in p.maxDets):
            raise ValueError("maxDets: caps must be positive integers, got %r" % (p.maxDets,))
        if not 1 <= rec.size <= MAX_REC_THRS:
            raise ValueError("recThrs: 1 to %d thresholds are supported, got %d" % (MAX_REC_THRS, rec.size))
        if np.any(np.diff(rec) < 0):
            raise ValueError("recThrs must be non-decreasing")
        if len(p.imgIds) == 0 or (p.useCats and len(p.catIds) == 0):
            raise ValueError("nothing to evaluate: imgIds or catIds is empty")
        K = len(p.catIds) if p.useCats else 1
        if K * len(p.imgIds) >= 2 ** 31 - 1:
            raise ValueError("too many (image, category) pairs: %d x %d" % (len(p.imgIds), K))
        return iou, rec, rng

    def _select(self, coco, imgIds, catIds, useCats):
        """Rows of coco's flat arrays that take part, in pair input order, and their pair index k * n_images + i."""
        f = coco._flat()
        n_img = len(imgIds)
        ii = np.searchsorted(imgIds, f['image_id'])
        keep = (ii < n_img) & (imgIds[np.minimum(ii, n_img - 1)] == f['image_id'])
        kk = np.searchsorted(catIds, f['category_id'])
        keep &= (kk < len(catIds)) & (catIds[np.minimum(kk, len(catIds) - 1)] == f['category_id'])
        rows = np.nonzero(keep)[0]
        if useCats:
            pair = kk[rows] * n_img + ii[rows]
        else:                               # pooled: category by category in catIds order, as a loop over the per-category lists gives
            rows = rows[np.argsort(kk[rows], kind='mergesort')]
            pair = ii[rows]
        return f, rows, pair.astype(np.int32)

    def evaluate(self):
        """Match every (image, category) pair on the device.  Results stay there until accumulate() / matches()."""
        from .. import _native as nat
        iou, rec, rng = self._checked_params()
        p = self.params
        imgIds = np.asarray(p.imgIds, dtype=np.int64)
        catIds = np.asarray(p.catIds, dtype=np.int64)          # under useCats=0 it still selects which annotations are pooled
        if catIds.size == 0:
            catIds = np.asarray(sorted(set(self.cocoGt._flat()['category_id'].tolist()) | set(self.cocoDt._flat()['category_id'].tolist())),
                                dtype=np.int64)
        catIds = np.unique(catIds)
        K = len(p.catIds) if p.useCats else 1
        gf, grows, gpair = self._select(self.cocoGt, imgIds, catIds, p.useCats)
        df, drows, dpair = self._select(self.cocoDt, imgIds, catIds, p.useCats)
        n_pairs = K * len(imgIds)
        self._dev = None
        r = nat.coco_match(dpair, df['bbox'][drows], df['score'][drows], gpair, gf['bbox'][grows], gf['area'][grows], gf['iscrowd'][grows],
                           n_pairs, iou, rng, int(p.maxDets[-1]))
        r.update(n_images=len(imgIds), K=K, rec_thrs=rec, max_dets=[int(m) for m in p.maxDets], det_rows=drows, gt_rows=grows,
                 imgIds=imgIds, catIds=np.asarray(p.catIds, dtype=np.int64) if p.useCats else np.asarray([-1]),
                 uploaded_bytes=int(dpair.nbytes + drows.size * 40 + gpair.nbytes + grows.size * 41 + iou.nbytes + rng.nbytes))
        self._dev = r
        self._paramsEval = copy.deepcopy(self.params)
        self.eval = {}

    def accumulate(self, p=None):
        """precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M] (float64, -1 where undefined) into `self.eval`."""
        from .. import _native as nat
        if self._dev is None:
            raise RuntimeError('Please run evaluate() first')
        if p is not None and p is not self.params:
            raise ValueError("accumulate() works on the parameters evaluate() ran with")
        r = self._dev
        pe = self._paramsEval
        precision, recall, scores = nat.coco_accumulate(r, r['n_images'], r['K'], r['max_dets'], r['rec_thrs'])
        T, R, K, A, M = precision.shape
        self.eval = {'params': pe, 'counts': [T, R, K, A, M], 'date': datetime.datetime.now().strftime('%Y-%m-%d %H:%M:%S'),
                     'precision': precision.cpu().numpy(), 'recall': recall.cpu().numpy(), 'scores': scores.cpu().numpy()}

    def matches(self, imgId, catId=None):
        """One pair's results as NumPy arrays: dtIds, dtScores (score order, cut to maxDets[-1]), dtMatches [A, T, D] (index + 1 into
        gtIds, 0 = unmatched), dtIgnore [A, T, D], gtIds (the pair's input order) and gtIgnore [A, G]."""
        if self._dev is None:
            raise RuntimeError('Please run evaluate() first')
        r = self._dev
        i = int(np.searchsorted(r['imgIds'], imgId))
        if i >= len(r['imgIds']) or r['imgIds'][i] != imgId:
            raise KeyError("image id %r was not evaluated" % (imgId,))
        k = 0
        if self._paramsEval.useCats:
            k = int(np.searchsorted(r['catIds'], catId))
            if k >= len(r['catIds']) or r['catIds'][k] != catId:
                raise KeyError("category id %r was not evaluated" % (catId,))
        pair = k * r['n_images'] + i
        d0, d1 = (int(v) for v in r['det_offsets'][pair:pair + 2].cpu())
        g0, g1 = (int(v) for v in r['gt_offsets'][pair:pair + 2].cpu())
        d1 = min(d1, d0 + r['max_det'])
        A, T = r['A'], r['T']
        code = r['det_match'][:, d0:d1].cpu().numpy().reshape(A, T, d1 - d0)
        dsrc = r['det_rows'][r['det_order'][d0:d1].cpu().numpy()] if d1 > d0 else np.zeros((0,), dtype=np.int64)
        gsrc = r['gt_rows'][r['gt_order'][g0:g1].cpu().numpy()] if g1 > g0 else np.zeros((0,), dtype=np.int64)
        df, gf = self.cocoDt._flat(), self.cocoGt._flat()
        return dict(dtIds=df['id'][dsrc], dtScores=df['score'][dsrc], dtMatches=(code >> 1).astype(np.int64), dtIgnore=(code & 1).astype(bool),
                    gtIds=gf['id'][gsrc], gtIgnore=r['gt_ignore'][:, g0:g1].cpu().numpy().reshape(A, g1 - g0).astype(bool))

    # -- summarize --------------------------------------------------------------------------------------------------------------
    def summarize(self):
        """Print the twelve statistics in pycocotools' format and store them in `self.stats`."""
        if not self.eval:
            raise RuntimeError('Please run accumulate() first')
        p = self.eval['params']
        if len(p.maxDets) < 3:
            raise ValueError("summarize() needs three detection caps (maxDets), got %r" % (p.maxDets,))

        def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
            iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
            titleStr = 'Average Precision' if ap == 1 else 'Average Recall'
            typeStr = '(AP)' if ap == 1 else '(AR)'
            iouStr = '{:0.2f}:{:0.2f}'.format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            s = self.eval['precision'] if ap == 1 else self.eval['recall']
            if iouThr is not None:
                s = s[np.where(iouThr == np.asarray(p.iouThrs))[0]]
            s = s[..., aind, :][..., mind]
            mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
            print(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
            return mean_s

        md = p.maxDets
        stats = np.zeros((12,))
        stats[0] = _summarize(1, maxDets=md[2])
        stats[1] = _summarize(1, iouThr=.5, maxDets=md[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=md[2])
        stats[3] = _summarize(1, areaRng='small', maxDets=md[2])
        stats[4] = _summarize(1, areaRng='medium', maxDets=md[2])
        stats[5] = _summarize(1, areaRng='large', maxDets=md[2])
        stats[6] = _summarize(0, maxDets=md[0])
        stats[7] = _summarize(0, maxDets=md[1])
        stats[8] = _summarize(0, maxDets=md[2])
        stats[9] = _summarize(0, areaRng='small', maxDets=md[2])
        stats[10] = _summarize(0, areaRng='medium', maxDets=md[2])
        stats[11] = _summarize(0, areaRng='large', maxDets=md[2])
        self.stats = stats

    def __str__(self):
        self.summarize()
        return ''
