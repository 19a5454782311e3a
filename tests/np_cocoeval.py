"""The COCO bbox evaluation protocol as plain Python / NumPy loops in float64: the restatement the device evaluator
(ssd_keras_amd/eval_utils/coco_eval.py, csrc/ssdhip_cocoeval.hip) is tested against.  Imports nothing from the package.

pycocotools is not available to this project, so the protocol is restated from its published description: evaluate() per
(image, category) pair and area range, accumulate() per (category, area range, detection cap), summarize() as twelve means.
One deliberate difference: matches are recorded as index + 1 into the pair's ground truth (0 = unmatched), not as annotation
ids, so a ground truth whose id is 0 is credited like any other.

    gts  list of dicts  image_id, category_id, bbox [x, y, w, h], area, iscrowd (optional, 0), id
    dts  list of dicts  image_id, category_id, bbox [x, y, w, h], score, id (optional)
"""
import numpy as np


def default_params():
    return dict(iouThrs=np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
                recThrs=np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
                maxDets=[1, 10, 100],
                areaRng=[[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]],
                areaRngLbl=['all', 'small', 'medium', 'large'],
                useCats=1)


def iou(d, g, crowd):
    """IoU of detection box d and ground-truth box g, both [x, y, w, h]; a crowd g divides by the detection's area."""
    da = float(d[2]) * float(d[3])
    ga = float(g[2]) * float(g[3])
    w = min(float(d[0]) + float(d[2]), float(g[0]) + float(g[2])) - max(float(d[0]), float(g[0]))
    if w <= 0:
        return 0.0
    h = min(float(d[1]) + float(d[3]), float(g[1]) + float(g[3])) - max(float(d[1]), float(g[1]))
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def evaluate_pair(gt, dt, iouThrs, areaRng, maxDet):
    """One pair.  gt, dt: the pair's dicts in input order.  Returns a dict with dtIds, dtScores, dtMatches [A, T, D] (index + 1
    into gt, 0 = unmatched), dtIgnore [A, T, D], gtIds and gtIgnore [A, G] (both in gt's input order); for the tests' own checks also the
    IoU matrix [D, G], the crowd flags and the number of detections before the cut."""
    T, A, G = len(iouThrs), len(areaRng), len(gt)
    scores = np.array([d['score'] for d in dt], dtype=np.float64)
    order = np.argsort(-scores, kind='mergesort')[:maxDet]
    dt = [dt[i] for i in order]
    D = len(dt)
    crowd = [int(g.get('iscrowd', 0)) for g in gt]
    ious = np.zeros((D, G))
    for di, d in enumerate(dt):
        for gi, g in enumerate(gt):
            ious[di, gi] = iou(d['bbox'], g['bbox'], crowd[gi])
    dtm = np.zeros((A, T, D), dtype=np.int64)
    dtig = np.zeros((A, T, D), dtype=bool)
    gtig = np.zeros((A, G), dtype=bool)
    for a, (lo, hi) in enumerate(areaRng):
        ign = [bool(crowd[gi]) or g['area'] < lo or g['area'] > hi for gi, g in enumerate(gt)]
        gtig[a] = ign
        gtind = np.argsort(np.array(ign, dtype=np.int64), kind='mergesort') if G else []
        for t, thr in enumerate(iouThrs):
            gtm = np.zeros(G, dtype=bool)
            for di, d in enumerate(dt):
                best = min([thr, 1 - 1e-10])
                m = -1
                for gi in gtind:
                    if gtm[gi] and not crowd[gi]:
                        continue
                    if m > -1 and not ign[m] and ign[gi]:
                        break
                    if ious[di, gi] < best:
                        continue
                    best = ious[di, gi]
                    m = gi
                if m == -1:
                    continue
                dtig[a, t, di] = ign[m]
                dtm[a, t, di] = m + 1
                gtm[m] = True
        for di, d in enumerate(dt):
            da = float(d['bbox'][2]) * float(d['bbox'][3])
            if da < lo or da > hi:
                dtig[a, :, di] |= dtm[a, :, di] == 0
    return dict(dtIds=np.array([d.get('id', -1) for d in dt], dtype=np.int64), dtScores=np.array([d['score'] for d in dt], dtype=np.float64),
                dtMatches=dtm, dtIgnore=dtig, gtIds=np.array([g['id'] for g in gt], dtype=np.int64), gtIgnore=gtig, ious=ious,
                gtCrowd=np.array(crowd, dtype=bool), nDt=len(scores))


def evaluate(gts, dts, imgIds, catIds, params=None):
    """All pairs.  Returns {'pairs': {(k, i): evaluate_pair(...)}, 'imgIds', 'catIds', 'params'}: k, i index the sorted unique catIds /
    imgIds ([-1] for the one pooled category under useCats=0).  Pairs with neither ground truth nor detections are absent."""
    p = dict(default_params())
    p.update(params or {})
    p['maxDets'] = sorted(p['maxDets'])
    imgIds = sorted(set(int(i) for i in imgIds))
    catIds = sorted(set(int(c) for c in catIds))
    img_index = {v: i for i, v in enumerate(imgIds)}
    cat_index = {v: k for k, v in enumerate(catIds)}
    G, D = {}, {}
    for src, into in ((gts, G), (dts, D)):
        if not p['useCats']:        # pooled: category by category in catIds order, as a loop over the per-category lists gives
            src = sorted(src, key=lambda a: a['category_id'])
        for a in src:
            if a['image_id'] not in img_index or a['category_id'] not in cat_index:
                continue
            k = cat_index[a['category_id']] if p['useCats'] else 0
            into.setdefault((k, img_index[a['image_id']]), []).append(a)
    if not p['useCats']:
        catIds = [-1]
    pairs = {}
    for key in sorted(set(G) | set(D)):
        pairs[key] = evaluate_pair(G.get(key, []), D.get(key, []), p['iouThrs'], p['areaRng'], p['maxDets'][-1])
    return dict(pairs=pairs, imgIds=imgIds, catIds=catIds, params=p)


def accumulate(ev):
    p = ev['params']
    T, R, K, A, M = len(p['iouThrs']), len(p['recThrs']), len(ev['catIds']), len(p['areaRng']), len(p['maxDets'])
    I = len(ev['imgIds'])
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        E = [ev['pairs'][(k, i)] for i in range(I) if (k, i) in ev['pairs']]
        if not E:
            continue
        for a in range(A):
            for m, maxDet in enumerate(p['maxDets']):
                dtScores = np.concatenate([e['dtScores'][:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind='mergesort')
                sorted_scores = dtScores[inds]
                dtm = np.concatenate([e['dtMatches'][a][:, :maxDet] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e['dtIgnore'][a][:, :maxDet] for e in E], axis=1)[:, inds]
                npig = int(sum(np.count_nonzero(~e['gtIgnore'][a]) for e in E))
                if npig == 0:
                    continue
                tps = np.logical_and(dtm != 0, np.logical_not(dtig))
                fps = np.logical_and(dtm == 0, np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    pis = np.searchsorted(rc, p['recThrs'], side='left')
                    for ri, pi in enumerate(pis):
                        if pi < nd:
                            q[ri] = pr[pi]
                            ss[ri] = sorted_scores[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return dict(params=p, counts=[T, R, K, A, M], precision=precision, recall=recall, scores=scores)


def _mean(s):
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def summarize(acc):
    """The twelve statistics (needs the default areaRngLbl and three detection caps)."""
    p = acc['params']
    iouThrs = np.asarray(p['iouThrs'])

    def one(ap, iouThr=None, areaRng='all', maxDets=100):
        aind = [i for i, lbl in enumerate(p['areaRngLbl']) if lbl == areaRng]
        mind = [i for i, md in enumerate(p['maxDets']) if md == maxDets]
        s = acc['precision'] if ap else acc['recall']
        if iouThr is not None:
            s = s[np.where(iouThr == iouThrs)[0]]
        s = s[..., aind, :][..., mind]
        return _mean(s)

    md = p['maxDets']
    return np.array([one(1, maxDets=md[2]), one(1, .5, maxDets=md[2]), one(1, .75, maxDets=md[2]),
                     one(1, areaRng='small', maxDets=md[2]), one(1, areaRng='medium', maxDets=md[2]), one(1, areaRng='large', maxDets=md[2]),
                     one(0, maxDets=md[0]), one(0, maxDets=md[1]), one(0, maxDets=md[2]),
                     one(0, areaRng='small', maxDets=md[2]), one(0, areaRng='medium', maxDets=md[2]), one(0, areaRng='large', maxDets=md[2])])


def run(gts, dts, imgIds, catIds, params=None):
    ev = evaluate(gts, dts, imgIds, catIds, params)
    acc = accumulate(ev)
    return ev, acc
