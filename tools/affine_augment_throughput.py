"""Throughput of the constant-input-size chain (DataAugmentationConstantInputSize, SSD7's notebook arguments) at B = 32, 300 x 480, seeded:
the per-image `__call__` loop, `augment_batch` (two pixel launches), and the warp launch alone timed by device events.  Writes one JSON
object (stdout, and to the path given as the first argument).  The warp kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script with `--warp-only` (50 launches of the warp alone; the durations are in the
run's trace database).  Results: profiles/affine_augment_throughput.json.  `--device-decisions` times `augment_batch`'s three routes
instead -- the host loop, the stream mode and the seeded mode, alternated in one process (`device_decisions` below; results:
profiles/constant_chain_device.json).

    python tools/affine_augment_throughput.py out.json
    python tools/affine_augment_throughput.py --device-decisions out.json
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/affine_augment_throughput.py --warp-only"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssd_keras_amd import _native as nat  # noqa: E402
from ssd_keras_amd.data_generator import _image_ops as iop  # noqa: E402
from ssd_keras_amd.data_generator.data_augmentation_chain_constant_input_size import DataAugmentationConstantInputSize  # noqa: E402

B, H, W = 32, 300, 480


def inputs(seed=9):
    rng = np.random.RandomState(seed)
    images = rng.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    labels = []
    for _ in range(B):
        n = rng.randint(1, 6)
        x0, y0 = rng.randint(0, W - 120, size=n), rng.randint(0, H - 90, size=n)
        labels.append(np.stack([rng.randint(1, 6, size=n), x0, y0, x0 + rng.randint(8, 120, size=n), y0 + rng.randint(6, 90, size=n)], axis=1))
    return images, labels


def warp_args(dev):
    """A translate -> zoom -> flip geometry for every image: the shape of the chain's one warp launch."""
    rng = np.random.RandomState(3)
    tabs = [iop.warp_tables(iop.rotation_matrix_2d((W / 2, H / 2), 0, rng.uniform(0.5, 2.0)), H, W) for _ in range(B)]
    geo = np.stack([[i % 2, rng.randint(-100, 100), rng.randint(-60, 60), 0, 0] for i in range(B)]).astype(np.int32)
    return (nat.to_device(geo, device=dev), nat.to_device(np.stack([t[0] for t in tabs]), device=dev),
            nat.to_device(np.stack([t[1] for t in tabs]), device=dev), nat.to_device(np.zeros((B, 3), np.uint8), device=dev))


NOTEBOOK = dict(random_brightness=(-48, 48, 0.5), random_contrast=(0.5, 1.8, 0.5), random_saturation=(0.5, 1.8, 0.5),
                random_hue=(18, 0.5), random_flip=0.5, random_translate=((0.03, 0.5), (0.03, 0.5), 0.5), random_scale=(0.5, 2.0, 0.5),
                n_trials_max=3, clip_boxes=True, overlap_criterion='area', bounds_box_filter=(0.3, 1.0), bounds_validator=(0.5, 1.0),
                n_boxes_min=1, background=(0, 0, 0))


def device_decisions(out_path, rounds=40):
    """`--device-decisions`: augment_batch's three routes alternated in one process -- the host loop (SSDHIP_AUG_HOST_STREAM=1), the
    stream mode (one wave walks the batch on np.random's state) and the seeded mode (one wave per image) -- each timed by the host clock
    around a call that ends in a device synchronise; median and spread (90th - 10th percentile) of `rounds` calls each, after checking
    that the host loop and the stream mode return the same batch.  Results: profiles/constant_chain_device.json."""
    dev = torch.device("cuda", 0)
    images, labels = inputs()
    x = torch.from_numpy(images).to(dev)
    chain = DataAugmentationConstantInputSize(**NOTEBOOK)
    if chain._device_params(labels) is None:
        raise SystemExit("the notebook's arguments are not covered by the decision kernel")
    seeds = list(range(1000, 1000 + B))

    def run(mode, rep):
        os.environ["SSDHIP_AUG_HOST_STREAM"] = "1" if mode == "host_loop" else "0"
        np.random.seed(rep)
        t0 = time.perf_counter()
        out = chain.augment_batch(x, labels, seeds=seeds) if mode == "seeded" else chain.augment_batch(x, labels)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    modes = ("host_loop", "stream", "seeded")
    for mode in modes:                                           # warm-up: library load, first launches, allocator
        for rep in range(3):
            run(mode, rep)
    (_, (hi, hl)), (_, (si, sl)) = run("host_loop", 7), run("stream", 7)
    same = bool(torch.equal(hi, si)) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(hl, sl))
    times = {m: [] for m in modes}
    for rep in range(rounds):
        for mode in modes:
            times[mode].append(run(mode, rep)[0])
    res = {"what": "tools/affine_augment_throughput.py --device-decisions on one MI355X: DataAugmentationConstantInputSize.augment_batch, "
                   "SSD7 notebook arguments, B=32, 300x480 uint8; three routes alternated in one process, %d calls each, host clock "
                   "around a call ending in a device synchronise; spread = 90th - 10th percentile" % rounds,
           "host_loop_equals_stream_mode": same}
    for mode in modes:
        t = 1e3 * np.array(times[mode])
        res[mode] = {"median_ms": round(float(np.median(t)), 3), "spread_ms": round(float(np.percentile(t, 90) - np.percentile(t, 10)), 3),
                     "min_ms": round(float(t.min()), 3), "max_ms": round(float(t.max()), 3),
                     "images_per_s_at_median": round(B / (float(np.median(t)) * 1e-3), 0)}
    res["stream_beats_host_loop_by_more_than_both_spreads"] = bool(
        res["host_loop"]["median_ms"] - res["stream"]["median_ms"] > res["host_loop"]["spread_ms"] + res["stream"]["spread_ms"])
    print(json.dumps(res), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def main():
    if "--device-decisions" in sys.argv:
        paths = [a for a in sys.argv[1:] if not a.startswith("--")]
        return device_decisions(paths[0] if paths else None)
    dev = torch.device("cuda", 0)
    images, labels = inputs()
    x = torch.from_numpy(images).to(dev)
    geo, xtab, ytab, bg = warp_args(dev)
    if "--warp-only" in sys.argv:
        for _ in range(50):
            nat.image_warp_affine_u8(x, H, W, geo, xtab, ytab, bg)
        torch.cuda.synchronize()
        return
    for _ in range(5):
        nat.image_warp_affine_u8(x, H, W, geo, xtab, ytab, bg)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 100
    start.record()
    for _ in range(reps):
        nat.image_warp_affine_u8(x, H, W, geo, xtab, ytab, bg)
    end.record()
    torch.cuda.synchronize()
    warp_ms = start.elapsed_time(end) / reps
    chain = DataAugmentationConstantInputSize()
    np.random.seed(0)
    chain.augment_batch(x, labels)                             # warm-up (library load, first launches)
    torch.cuda.synchronize()
    per_image, batch = [], []
    for rep in range(3):
        np.random.seed(rep)
        t0 = time.perf_counter()
        for i in range(B):
            chain(images[i], labels[i])
        per_image.append(time.perf_counter() - t0)
        np.random.seed(rep)
        t0 = time.perf_counter()
        out, _ = chain.augment_batch(x, labels)
        torch.cuda.synchronize()
        batch.append(time.perf_counter() - t0)
    moved = 2 * B * H * W * 3
    res = {"what": "DataAugmentationConstantInputSize, SSD7 notebook arguments, B=32, 300x480 uint8, measured on one MI355X",
           "per_image_call_loop_ms_per_batch": round(1e3 * min(per_image), 3),
           "augment_batch_ms_per_batch": round(1e3 * min(batch), 3),
           "warp_launch_us_device_events": round(1e3 * warp_ms, 2),
           "warp_bytes_per_batch": moved,
           "warp_GBps_device_events": round(moved / (warp_ms * 1e-3) / 1e9, 1)}
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
