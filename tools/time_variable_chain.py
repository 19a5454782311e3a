"""DataAugmentationVariableInputSize on one MI355X: `augment_batch` on a ragged batch -- stream mode (one wave walks the batch on
np.random's state) and seeded mode (one wave per image) -- against the loop of `__call__` that `DataGenerator.generate()` ran for this
chain before it had a batch path (that loop's code is unchanged: it is the yardstick).

    python tools/time_variable_chain.py [OUT.json] [--rounds N]

Input: 32 VOC-sized uint8 images on the host, sizes drawn around 500 x 375, one to eight boxes each, resized to 300 x 300.  The three
arms are alternated in one process; each call is timed by the host clock from host images to a host batch (the batch arms end in the
download `generate()` makes, the loop returns host arrays by itself), after a device synchronise.  Reported per arm: median, spread
(90th - 10th percentile), min, max.  `batch_path_beats_the_loop` is the rule `generate()`'s routing rests on: the loop's median minus the
stream arm's must exceed the sum of both spreads.  Results: profiles/variable_chain_device.json."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ssd_keras_amd.data_generator.data_augmentation_chain_variable_input_size import DataAugmentationVariableInputSize  # noqa: E402

B, OUT = 32, (300, 300)


def inputs(seed=17):
    rng = np.random.RandomState(seed)
    images, labels = [], []
    for _ in range(B):
        landscape = rng.uniform() < 0.75
        long_side, short_side = int(rng.randint(420, 501)), int(rng.randint(300, 400))
        h, w = (short_side, long_side) if landscape else (long_side, short_side)
        images.append(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
        n = int(rng.randint(1, 9))
        bw, bh = rng.randint(w // 10, w // 2, size=n), rng.randint(h // 10, h // 2, size=n)
        x0, y0 = rng.randint(0, w - bw), rng.randint(0, h - bh)
        labels.append(np.stack([rng.randint(1, 21, size=n), x0, y0, x0 + bw, y0 + bh], axis=1).astype(np.int64))
    return images, labels


def main():
    args = sys.argv[1:]
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 30
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--rounds")]
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    images, labels = inputs()
    chain = DataAugmentationVariableInputSize(resize_height=OUT[0], resize_width=OUT[1])
    if chain._device_params(labels, shapes=[im.shape[:2] for im in images]) is None:
        raise SystemExit("the default arguments are not covered by the decision kernel")
    seeds = list(range(1000, 1000 + B))

    def run(mode, rep):
        np.random.seed(rep)
        t0 = time.perf_counter()
        if mode == "call_loop":
            pairs = [chain(im, lab) for im, lab in zip(images, labels)]
            out, out_labels = np.stack([p[0] for p in pairs]), [p[1] for p in pairs]
        else:
            dev, out_labels = chain.augment_batch(images, labels, seeds=seeds if mode == "seeded" else None)
            out = dev.cpu().numpy()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, out_labels

    modes = ("call_loop", "stream", "seeded")
    for mode in modes:                                           # warm-up: library load, first launches, allocator
        for rep in range(3):
            run(mode, rep)
    (_, li, ll), (_, si, sl) = run("call_loop", 7), run("stream", 7)
    same = bool(np.array_equal(li, si)) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(ll, sl))
    times = {m: [] for m in modes}
    for rep in range(rounds):
        for mode in modes:
            times[mode].append(run(mode, rep)[0])
    res = {"what": "tools/time_variable_chain.py on one MI355X: DataAugmentationVariableInputSize, default arguments, a ragged batch of %d "
                   "host images around 500 x 375 with 1 - 8 boxes each -> %d x %d; three arms alternated in one process, %d calls each, "
                   "host clock from host images to a host batch, ending in a device synchronise; spread = 90th - 10th percentile"
                   % (B, OUT[0], OUT[1], rounds),
           "call_loop_equals_stream_mode": same}
    for mode in modes:
        t = 1e3 * np.array(times[mode])
        res[mode] = {"median_ms": round(float(np.median(t)), 3), "spread_ms": round(float(np.percentile(t, 90) - np.percentile(t, 10)), 3),
                     "min_ms": round(float(t.min()), 3), "max_ms": round(float(t.max()), 3),
                     "images_per_s_at_median": round(B / (float(np.median(t)) * 1e-3), 0)}
    res["batch_path_beats_the_loop"] = bool(
        res["call_loop"]["median_ms"] - res["stream"]["median_ms"] > res["call_loop"]["spread_ms"] + res["stream"]["spread_ms"])
    print(json.dumps(res), flush=True)
    if paths:
        with open(paths[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
