"""What `Evaluator.predict_on_dataset(collect='device')` costs against the host route, on one MI355X.  Both routes alternate in ONE
process, `rounds` times after one untimed round each; per arm the median and the spread (max - min) of a host clock around work that
ends in a device synchronise.  "Faster" is the project's rule: the medians differ by more than the sum of the two arms' spreads.

  (a) collection alone: a stand-in inference-mode model that returns a FIXED device tensor (`rows` rows per image, a few of them zero
      padding) over a synthetic in-memory dataset of `images` images of mixed sizes (300-500 px per side), 20 classes, batch 32:
      `predict_on_dataset` + `match_predictions` each way; the first read of `prediction_results` after a device collection (the one
      download and the tuple lists built from it) is timed separately -- a user who only wants the mAP never pays it.
  (b) the whole `Evaluator.__call__` with a randomly initialised `ssd_300` in mode 'training' at `confidence_thresh=0.01`, `top_k=200`,
      on the same images, both ways.
Both routes' results are compared before anything is timed (the per-class counts, and in (b) the mAP).  Writes one JSON object to
stdout and to the path given as the first argument.  Results: profiles/evaluator_collect.json.

    python tools/time_evaluator_collect.py out.json [--images 4952] [--rounds 5] [--rounds-b 3] [--skip-b]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssd_keras_amd.data_generator import object_detection_2d_data_generator as odg  # noqa: E402
from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator  # noqa: E402

N_CLASSES, BATCH, ROWS, SIZE = 20, 32, 200, 300


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def dataset(n, seed=4, distinct=64):
    """n images of 300-500 px per side (`distinct` different arrays, cycled: the generator does the same work on each) with 1-5 boxes."""
    rng = np.random.RandomState(seed)
    pool = []
    for _ in range(distinct):
        h, w = int(rng.randint(300, 501)), int(rng.randint(300, 501))
        yy, xx = np.mgrid[0:h, 0:w]
        pool.append(np.stack([(o + a * yy + b * xx) % 256 for o, a, b in rng.uniform(-1, 1, size=(3, 3)) * [200, 0.5, 0.5]], -1).astype(np.uint8))
    images, labels = [], []
    for i in range(n):
        img = pool[i % distinct]
        h, w = img.shape[:2]
        k = int(rng.randint(1, 6))
        x0, y0 = rng.randint(0, w - 60, size=k), rng.randint(0, h - 60, size=k)
        images.append(img)
        labels.append(np.stack([rng.randint(1, N_CLASSES + 1, size=k), x0, y0, x0 + rng.randint(10, 60, size=k), y0 + rng.randint(10, 60, size=k)],
                               axis=1).astype(np.int64))
    return images, labels


def generator(images, labels):
    n = len(images)
    g = odg.DataGenerator(labels=list(labels), image_ids=list(range(n)))
    g.images, g.filenames = list(images), ["%d.jpg" % i for i in range(n)]
    g.dataset_size, g.dataset_indices = n, np.arange(n, dtype=np.int32)
    return g


def stand_in_model(seed=9, padding=10):
    """Returns the same (B, ROWS, 6) float32 device tensor for every batch: ROWS - padding detections per image and zero padding."""
    rng = np.random.RandomState(seed)
    rows = np.zeros((BATCH, ROWS, 6), dtype=np.float32)
    rows[:, :, 0] = rng.randint(1, N_CLASSES + 1, size=(BATCH, ROWS))
    rows[:, :, 1] = rng.uniform(0.01, 1.0, size=(BATCH, ROWS))
    rows[:, :, 2:4] = rng.uniform(0, SIZE - 40, size=(BATCH, ROWS, 2))
    rows[:, :, 4:6] = rows[:, :, 2:4] + rng.uniform(4, 120, size=(BATCH, ROWS, 2))
    rows[:, rng.choice(ROWS, size=padding, replace=False), :] = 0
    fixed = torch.from_numpy(rows).cuda()
    return lambda batch: fixed[:batch.shape[0]]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    print("  %.3f s" % t, file=sys.stderr, flush=True)                          # progress: a round of the host route takes a while
    return t, out


def summary(times):
    return {"median_s": round(statistics.median(times), 4), "spread_s": round(max(times) - min(times), 4), "rounds_s": [round(t, 4) for t in times]}


def verdict(host, device):
    gap = host["median_s"] - device["median_s"]
    noise = host["spread_s"] + device["spread_s"]
    return {"host_minus_device_s": round(gap, 4), "sum_of_spreads_s": round(noise, 4),
            "device_route": "faster" if gap > noise else ("slower" if -gap > noise else "within the spreads")}


def case_a(g, rounds):
    model = stand_in_model()

    def run(collect):
        ev = Evaluator(model, N_CLASSES, g, model_mode='inference')

        def work():
            ev.predict_on_dataset(SIZE, SIZE, BATCH, verbose=False, collect=collect)
            ev.match_predictions(verbose=False)
        return timed(work)[0], ev
    (_, ev_h), (_, ev_d) = run('host'), run('device')                           # untimed round; the results agree
    first_read, results = timed(lambda: ev_d.prediction_results)
    counts = [len(r) for r in ev_h.prediction_results]
    assert [len(r) for r in results] == counts and results[1][:50] == ev_h.prediction_results[1][:50]
    for name in ("true_positives", "cumulative_false_positives"):
        assert all(np.array_equal(a, b) for a, b in zip(getattr(ev_h, name)[1:], getattr(ev_d, name)[1:]))
    times = {"host": [], "device": []}
    reads = [first_read]
    for _ in range(rounds):
        for collect in ("host", "device"):
            t, ev = run(collect)
            times[collect].append(t)
            if collect == "device":
                reads.append(timed(lambda: ev.prediction_results)[0])
    out = {"what": "predict_on_dataset + match_predictions, stand-in model returning a fixed device tensor",
           "images": len(g.images), "boxes": int(sum(counts)), "host": summary(times["host"]), "device": summary(times["device"]),
           "device_first_read_of_prediction_results": summary(reads)}
    out["verdict"] = verdict(out["host"], out["device"])
    return out


def case_b(g, rounds):
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.models.keras_ssd300 import ssd_300
    cfg = syn.SSD300_VOC                                                          # the benchmark's model, bfloat16 as there
    assert cfg["n_classes"] == N_CLASSES
    torch.manual_seed(1)
    model = ssd_300((SIZE, SIZE, 3), N_CLASSES, mode='training', scales=cfg["scales"], aspect_ratios_per_layer=cfg["aspect_ratios_per_layer"],
                    steps=cfg["steps"], offsets=cfg["offsets"]).cuda()
    model = model.to(memory_format=torch.channels_last).eval().to(torch.bfloat16)
    kw = dict(verbose=False, decoding_confidence_thresh=0.01, decoding_top_k=200)

    def run(collect):
        ev = Evaluator(model, N_CLASSES, g, model_mode='training')
        t, value = timed(lambda: ev(SIZE, SIZE, BATCH, collect=collect, **kw))
        return t, value, ev
    (_, m_h, ev_h), (_, m_d, ev_d) = run('host'), run('device')
    assert m_h == m_d, (m_h, m_d)
    boxes = int(sum(len(r) for r in ev_h.prediction_results))
    times = {"host": [], "device": []}
    for _ in range(rounds):
        for collect in ("host", "device"):
            times[collect].append(run(collect)[0])
    out = {"what": "Evaluator.__call__, randomly initialised ssd_300 in mode 'training', confidence_thresh 0.01, top_k 200",
           "images": len(g.images), "boxes": boxes, "mAP": float(m_h), "host": summary(times["host"]), "device": summary(times["device"])}
    out["verdict"] = verdict(out["host"], out["device"])
    return out


def main():
    n, rounds, rounds_b = _arg("--images", 4952), _arg("--rounds", 5), _arg("--rounds-b", 3)
    g = generator(*dataset(n))
    res = {"what": "Evaluator collection, host route against collect='device', batch %d, %d x %d input, %d classes, one MI355X; host clock "
                   "around work ending in a device synchronise, the routes alternating in one process after one untimed round each"
                   % (BATCH, SIZE, SIZE, N_CLASSES),
           "a_collection_alone": case_a(g, rounds)}
    if "--skip-b" not in sys.argv:
        res["b_whole_call_ssd300"] = case_b(g, rounds_b)
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
