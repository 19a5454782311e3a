"""COCOeval on the device at val2017 size (GPU box): times `evaluate()` and `accumulate()` of ssd_keras_amd.eval_utils.coco_eval.

Synthetic input built here from a seed: 5 000 images, 80 categories, about 7 ground truths per image with COCO's rough area mix
(about 41 % small, 34 % medium, 24 % large; 1.5 % crowds) and 100 / 200 detections per image, half of them jittered copies of the
image's ground truth.  Host parsing (building the COCO objects and their flat arrays) is timed once and reported separately; the
timed calls are warmed up, repeated and end in a device synchronise (evaluate) or in the download of the three result arrays
(accumulate); median, minimum and maximum are reported.  The only yardstick available is this project's OWN Python restatement
(tests/np_cocoeval.py) on a 1/50 subsample on the same box's CPU -- it is not pycocotools, for which no timing exists.

    python tools/time_coco_eval.py [--out profiles/coco_eval.json] [--kernel-stats STATS.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/time_coco_eval.py --trace-run

`--trace-run` only runs four evaluations of the 100-detection input (for the kernel trace); `--kernel-stats` folds the trace's
per-kernel averages into the JSON."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IMAGES, N_CATS = 5000, 80


def synthetic(dets_per_image, seed=0, n_images=N_IMAGES):
    rng = np.random.RandomState(seed)
    cat_ids = np.sort(rng.choice(np.arange(1, 91), N_CATS, replace=False))
    cat_p = 1.0 / np.arange(1, N_CATS + 1) ** 0.8
    cat_p /= cat_p.sum()
    gts, det_rows = [], []
    for img in range(1, n_images + 1):
        G = rng.poisson(7)
        kind = rng.choice(3, size=G, p=[0.41, 0.35, 0.24])
        side = np.where(kind == 0, rng.uniform(6, 40, G), np.where(kind == 1, rng.uniform(40, 120, G), rng.uniform(120, 400, G)))
        w = np.round(side * rng.uniform(0.6, 1.6, G), 2)
        h = np.round(side * rng.uniform(0.6, 1.6, G), 2)
        x, y = np.round(rng.uniform(0, 640 - np.minimum(w, 600)), 2), np.round(rng.uniform(0, 480 - np.minimum(h, 440)), 2)
        cats = cat_ids[rng.choice(N_CATS, size=G, p=cat_p)]
        for j in range(G):
            gts.append(dict(id=len(gts) + 1, image_id=img, category_id=int(cats[j]), bbox=[float(x[j]), float(y[j]), float(w[j]), float(h[j])],
                            area=float(np.round(w[j] * h[j] * rng.uniform(0.4, 0.9), 1)), iscrowd=int(rng.rand() < 0.015)))
        D = dets_per_image
        near = (rng.rand(D) < 0.5) & (G > 0)
        src = rng.randint(0, max(G, 1), D)
        dw, dh = rng.uniform(10, 300, D), rng.uniform(10, 300, D)
        dx, dy = rng.uniform(0, 600, D), rng.uniform(0, 440, D)
        dc = cat_ids[rng.choice(N_CATS, size=D, p=cat_p)]
        if G > 0:
            jit = rng.normal(0, 0.08, (D, 4))
            dx = np.where(near, x[src] + jit[:, 0] * w[src], dx)
            dy = np.where(near, y[src] + jit[:, 1] * h[src], dy)
            dw = np.where(near, w[src] * (1 + jit[:, 2]), dw)
            dh = np.where(near, h[src] * (1 + jit[:, 3]), dh)
            dc = np.where(near, cats[src], dc)
        score = np.round(rng.rand(D) * np.where(near, 1.0, 0.6), 3)
        det_rows.append(np.stack([np.full(D, img, dtype=np.float64), np.round(dx, 1), np.round(dy, 1), np.round(np.maximum(dw, 1), 1),
                                  np.round(np.maximum(dh, 1), 1), score, dc.astype(np.float64)], axis=1))
    dataset = dict(images=[dict(id=i) for i in range(1, n_images + 1)], categories=[dict(id=int(c), name="c%d" % c) for c in cat_ids],
                   annotations=gts)
    return dataset, np.concatenate(det_rows)


def spread(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), runs=len(ms))


def build(dataset, det_array):
    from ssd_keras_amd.eval_utils.coco_eval import COCO, COCOeval
    t0 = time.perf_counter()
    gt = COCO()
    gt.dataset = dataset
    gt.createIndex()
    dt = gt.loadRes(det_array)
    gt._flat(), dt._flat()
    parse_s = time.perf_counter() - t0
    return COCOeval(gt, dt, 'bbox'), parse_s


def time_config(dets_per_image, reps, torch):
    dataset, det_array = synthetic(dets_per_image)
    e, parse_s = build(dataset, det_array)
    for _ in range(2):                                   # warm-up: code objects, workspace, allocator
        e.evaluate()
        e.accumulate()
    ev_ms, acc_ms = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.evaluate()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        e.accumulate()                                   # ends in the download of precision / recall / scores
        t2 = time.perf_counter()
        ev_ms.append((t1 - t0) * 1e3)
        acc_ms.append((t2 - t1) * 1e3)
    r = e._dev
    out = dict(detections_per_image=dets_per_image, n_detections=int(det_array.shape[0]), n_ground_truth=len(dataset["annotations"]),
               n_pairs=int(r["n_pairs"]), host_parse_s=round(parse_s, 3),
               evaluate=spread(ev_ms), accumulate=spread(acc_ms),
               evaluate_note="host selection of the rows (NumPy), upload, three sorts and the matching kernel; ends in a device synchronise",
               accumulate_note="two sorts, the accumulation kernel and the download of the three arrays",
               uploaded_bytes=int(r["uploaded_bytes"]),
               downloaded_bytes=int(sum(e.eval[k].nbytes for k in ("precision", "recall", "scores"))),
               det_match_bytes=int(r["det_match"].numel() * 4),
               AP=float(np.mean(e.eval["precision"][:, :, :, 0, 2][e.eval["precision"][:, :, :, 0, 2] > -1])))
    return out, dataset, det_array


def restatement_subsample(dataset, det_array, every=50):
    """The project's own Python restatement on every 50th image, on this box's CPU."""
    from tests import np_cocoeval as ref
    keep = set(range(1, N_IMAGES + 1, every))
    gts = [g for g in dataset["annotations"] if g["image_id"] in keep]
    dts = [dict(image_id=int(r[0]), bbox=[float(v) for v in r[1:5]], score=float(r[5]), category_id=int(r[6]), id=i + 1)
           for i, r in enumerate(det_array) if int(r[0]) in keep]
    cats = [c["id"] for c in dataset["categories"]]
    t0 = time.perf_counter()
    ev = ref.evaluate(gts, dts, sorted(keep), cats)
    t1 = time.perf_counter()
    ref.accumulate(ev)
    t2 = time.perf_counter()
    return dict(what="tests/np_cocoeval.py, the project's own Python / NumPy restatement (NOT pycocotools), one CPU core",
                images=len(keep), detections=len(dts), evaluate_s=round(t1 - t0, 3), accumulate_s=round(t2 - t1, 3))


def kernel_stats(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "coco_" in name or "rocprim" in name:
                head = name.replace("void ", "").split("<")[0].split("(")[0]
                short = ("rocprim " if "rocprim" in head else "") + head.split("::")[-1]
                rows.append(dict(kernel=short, calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 2),
                                 total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3)))
    merged = {}
    for r in rows:
        m = merged.setdefault(r["kernel"], dict(kernel=r["kernel"], calls=0, total_ms=0.0))
        m["calls"] += r["calls"]
        m["total_ms"] = round(m["total_ms"] + r["total_ms"], 3)
    for m in merged.values():
        m["average_us"] = round(m["total_ms"] * 1e3 / m["calls"], 2)
    return sorted(merged.values(), key=lambda m: -m["total_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    if args.trace_run:
        e, _ = build(*synthetic(100))
        for _ in range(4):
            e.evaluate()
            e.accumulate()
        torch.cuda.synchronize()
        return
    result = dict(workload="COCOeval bbox, synthetic val2017-sized input: %d images, %d categories" % (N_IMAGES, N_CATS),
                  device=torch.cuda.get_device_name(0), configs=[])
    first = None
    for dets in (100, 200):
        out, dataset, det_array = time_config(dets, args.reps, torch)
        result["configs"].append(out)
        if first is None:
            first = (dataset, det_array)
    result["python_restatement_1_in_50"] = restatement_subsample(*first)
    result["pycocotools"] = "not measured: pycocotools is not installed on the box, no timing of it exists"
    if args.kernel_stats:
        result["kernels_100_detections_per_image"] = dict(
            source="rocprofv3 --kernel-trace --stats of `--trace-run` (4 evaluate + accumulate calls), a run of its own",
            kernels=kernel_stats(args.kernel_stats))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
