"""A composed transformation list through `DataGenerator.generate()` on one MI355X: the 'program' batch path against the per-image loop
(`_batch_path` forced to None -- what `generate()` did for such a list before it had this path; that loop's code is unchanged: it is the
yardstick).

    python tools/time_program_path.py [OUT.json] [--rounds N] [--warps]

Input: 32 VOC-sized uint8 images on the host, sizes drawn around 500 x 375, one to eight boxes each.  The list: ConvertTo3Channels,
ConvertDataType('float32'), RandomBrightness, RandomContrast, ConvertDataType('uint8'), ConvertColor(to='HSV'),
RandomHistogramEqualization, ConvertColor('HSV', 'RGB'), RandomGamma, RandomFlip, RandomPadFixedAR(1.0), Resize(300, 300)
(tests/program_path_cases.list_b).  The two arms are alternated in one process; each call is one batch of `generate()`, timed by the host
clock from host images to a host batch, after a device synchronise.  Reported per arm: median, spread (90th - 10th percentile), min,
max.  `program_path_beats_the_loop`: the loop's median minus the program path's exceeds the sum of both spreads.  Results:
profiles/program_path.json.

`--warps`: the list is ConvertTo3Channels, RandomTranslate, RandomScale, RandomFlip, Resize(300, 300)
(tests/program_warp_cases.list_i) and the arms are the generator's `compose_warps` switch on ('program': the staged lazy images, one
ragged warp launch and one gather per batch) and off ('loop': what `generate()` does for this list without the switch).  Results:
profiles/program_path_warps.json.  The warp kernel's own time comes from a kernel trace of this tool (`--trace-only`: warm-up and five
batches of the 'program' arm, nothing timed)."""
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import program_path_cases as pc  # noqa: E402
from tests import program_warp_cases as wc  # noqa: E402
from tools.time_variable_chain import B, inputs  # noqa: E402

OUT = (300, 300)


def main():
    args = sys.argv[1:]
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 20
    warps, trace_only = "--warps" in args, "--trace-only" in args
    paths = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--rounds")]
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    n = pc.ns()
    images, labels = inputs()
    transformations = wc.list_i(n, OUT) if warps else pc.list_b(n, OUT)
    assert n.DataGenerator._batch_path(transformations, images, True) == (None if warps else 'program')
    routed = staticmethod(n.DataGenerator._batch_path)
    launches = []

    def run(mode, rep):
        np.random.seed(rep)
        random.seed(rep)
        if not warps:
            n.DataGenerator._batch_path = routed if mode == "program" else staticmethod(lambda *a: None)
        try:
            generator = pc.array_generator(n, images, labels)
            generator.compose_warps = warps and mode == "program"
            gen = generator.generate(batch_size=B, shuffle=False, transformations=transformations,
                                     returns={'processed_images', 'processed_labels'})
            t0 = time.perf_counter()
            out, out_labels = next(gen)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out, out_labels
        finally:
            n.DataGenerator._batch_path = routed

    modes = ("loop", "program")
    for mode in modes:                                           # warm-up: library load, first launches, allocator
        for rep in range(2):
            run(mode, rep)
    if trace_only:
        for rep in range(5):
            run("program", rep)
        return
    (_, li, ll), (_, pi, pl) = run("loop", 7), run("program", 7)
    same = bool(li.dtype == pi.dtype and np.array_equal(li, pi)) and all(np.array_equal(a, b) for a, b in zip(ll, pl))
    from ssd_keras_amd import _native as nat
    real = nat.launch
    nat.launch = lambda name, device, *a: (launches.append(name), real(name, device, *a))[1]
    try:
        run("program", 7)
    finally:
        nat.launch = real
    times = {m: [] for m in modes}
    for rep in range(rounds):
        for mode in modes:
            times[mode].append(run(mode, rep)[0])
    what = ("the list of tests/program_warp_cases.list_i (Translate / Scale; 'program' = `compose_warps` on, 'loop' = off)" if warps
            else "the composed list of tests/program_path_cases.list_b")
    res = {"what": "tools/time_program_path.py%s on one MI355X: generate() with %s on a ragged "
                   "batch of %d host images around 500 x 375 with 1 - 8 boxes each -> %d x %d; two arms alternated in one process, %d "
                   "batches each, host clock from host images to a host batch, ending in a device synchronise; spread = 90th - 10th "
                   "percentile" % (" --warps" if warps else "", what, B, OUT[0], OUT[1], rounds),
           "loop_equals_program_path": same, "program_path_launches": launches}
    for mode in modes:
        t = 1e3 * np.array(times[mode])
        res[mode] = {"median_ms": round(float(np.median(t)), 3), "spread_ms": round(float(np.percentile(t, 90) - np.percentile(t, 10)), 3),
                     "min_ms": round(float(t.min()), 3), "max_ms": round(float(t.max()), 3),
                     "images_per_s_at_median": round(B / (float(np.median(t)) * 1e-3), 0)}
    res["program_path_beats_the_loop"] = bool(
        res["loop"]["median_ms"] - res["program"]["median_ms"] > res["loop"]["spread_ms"] + res["program"]["spread_ms"])
    print(json.dumps(res), flush=True)
    if paths:
        with open(paths[0], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
