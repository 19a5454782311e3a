"""DataAugmentationSatellite on one MI355X: `augment_batch` on a ragged batch -- stream mode (one wave walks the batch on np.random's
state) and seeded mode (one wave per image) -- against the loop of `__call__` that `DataGenerator.generate()` ran for this chain before
it had a batch path (that loop's code is unchanged: it is the yardstick).

    python tools/time_satellite_chain.py [OUT.json] [--rounds N]

Input: 32 VOC-sized uint8 images on the host, sizes drawn around 500 x 375, one to eight boxes each, resized to 300 x 300 (the inputs of
tools/time_variable_chain.py).  The three arms are alternated in one process; each call is timed by the host clock from host images to a
host batch (the batch arms end in the download `generate()` makes, the loop returns host arrays by itself), after a device synchronise.
Reported per arm: median, spread (90th - 10th percentile), min, max.  `batch_path_beats_the_loop` is the rule `generate()`'s routing
rests on: the loop's median minus the stream arm's must exceed the sum of both spreads.

`gather`: the four device launches of the seeded route (decisions, photometric programs, plans, gather) timed one by one with device
events on the same batch, once with a chain that never rotates and once with one that turns every image by 90 degrees -- a turned image
is read down source columns, so this is what a transposed read costs the gather, next to the rest of the batch's device time.
Results: profiles/satellite_chain_device.json."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ssd_keras_amd import _native as nat  # noqa: E402
from ssd_keras_amd.data_generator import _image_ops as iop  # noqa: E402
from ssd_keras_amd.data_generator import _chain_batch as cb  # noqa: E402
from ssd_keras_amd.data_generator.data_augmentation_chain_constant_input_size import _seed_states  # noqa: E402
from ssd_keras_amd.data_generator.data_augmentation_chain_satellite import DataAugmentationSatellite  # noqa: E402
from tools.time_variable_chain import B, OUT, inputs  # noqa: E402


def launch_times(chain, images, labels, seeds, turns, reps=30):
    """Median device time (ms, events) of each launch of the seeded route on this batch: decide, program, plans, gather."""
    packed = iop.pack_ragged(list(images))
    shapes = [(h, w) for h, w, _ in packed.shapes]
    params = chain._device_params(labels, shapes=shapes)
    _, lab_in, n_in = cb.pack_labels(labels, cb.label_cols(chain.labels_format))
    device = packed.data.device
    bg = nat.to_device(np.zeros((B, 3), dtype=np.uint8), device=device)
    n_taps = chain._n_taps(shapes)
    names = ("decide", "program", "plans", "gather")
    times = {n: [] for n in names}
    n_turned = 0
    for _ in range(reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        ops_dev, args_dev, geo_dev, fetch = nat.sat_augment_decide(params, turns, _seed_states(seeds), lab_in, n_in, device,
                                                                   table=packed.table)
        ev[1].record()
        distorted = nat.image_program_ragged_u8(packed.data, packed.table, packed.max_pixels, ops_dev, args_dev)
        ev[2].record()
        plans, ix, wx, iy, wy, tr = nat.sat_augment_plans(geo_dev, OUT[0], OUT[1], n_taps, table=packed.table)
        ev[3].record()
        nat.image_resize_gather_turn_u8(distorted, packed.table, OUT[0], OUT[1], plans, ix, wx, iy, wy, tr, bg)
        ev[4].record()
        torch.cuda.synchronize()
        n_turned = int(tr.sum().item())
        for k, n in enumerate(names):
            times[n].append(ev[k].elapsed_time(ev[k + 1]))
    out = {n + "_ms": round(float(np.median(times[n][3:])), 4) for n in names}       # (decide includes its upload)
    out["images_turned"] = n_turned
    return out


def main():
    args = sys.argv[1:]
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 30
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--rounds")]
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    import random
    images, labels = inputs()
    chain = DataAugmentationSatellite(resize_height=OUT[0], resize_width=OUT[1])
    if chain._device_params(labels, shapes=[im.shape[:2] for im in images]) is None:
        raise SystemExit("the default arguments are not covered by the decision kernel")
    seeds = list(range(1000, 1000 + B))

    def run(mode, rep):
        np.random.seed(rep)
        random.seed(rep)
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
    res = {"what": "tools/time_satellite_chain.py on one MI355X: DataAugmentationSatellite, default arguments, a ragged batch of %d "
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
    ones = np.ones((B,), dtype=np.int32)
    never = DataAugmentationSatellite(resize_height=OUT[0], resize_width=OUT[1], random_rotate=([90], 0.0))
    always = DataAugmentationSatellite(resize_height=OUT[0], resize_width=OUT[1], random_rotate=([90], 1.0))
    res["gather"] = {"what": "device events around each launch of the seeded route on the same batch, median of 30; no image turned / "
                             "every image turned by 90 degrees",
                     "unrotated": launch_times(never, images, labels, seeds, ones),
                     "all_90_degrees": launch_times(always, images, labels, seeds, ones)}
    g = res["gather"]
    rest = sum(g["all_90_degrees"][k] for k in ("decide_ms", "program_ms", "plans_ms"))
    g["turned_gather_over_unturned"] = round(g["all_90_degrees"]["gather_ms"] / g["unrotated"]["gather_ms"], 3)
    g["turned_gather_costs_more_than_the_rest_of_the_batch"] = bool(g["all_90_degrees"]["gather_ms"] > rest)
    print(json.dumps(res), flush=True)
    if paths:
        with open(paths[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
