"""Throughput of DataGenerator.generate() at B = 32, 300 x 300 output, images held in memory at VOC-like mixed sizes (300-500 px per side):
`[SSDDataAugmentation(300, 300)]` and `[ConvertTo3Channels, Resize(300, 300)]`, each through the ragged batch path and through the
reference's per-image loop (the batch path switched off).  ms per batch = best of 3 timed batches after a warm-up batch, host clock with
the device synchronised.  Writes one JSON object (stdout, and to the path given as the first argument).  The four ragged kernels' own
times come from a separate `rocprofv3 --kernel-trace --stats` run of this script with `--kernels-only` (20 batch-path batches of each
list).  Results: profiles/data_generator_throughput.json.

    python tools/data_generator_throughput.py out.json
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/data_generator_throughput.py --kernels-only"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ssd_keras_amd.data_generator import object_detection_2d_data_generator as odg  # noqa: E402
from ssd_keras_amd.data_generator.data_augmentation_chain_original_ssd import SSDDataAugmentation  # noqa: E402
from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Resize  # noqa: E402
from ssd_keras_amd.data_generator.object_detection_2d_photometric_ops import ConvertTo3Channels  # noqa: E402

B, N = 32, 128


def dataset(seed=4):
    """N smooth images of 300-500 px per side (JPEG-like content: gradients and flat boxes) with 1-5 boxes each."""
    rng = np.random.RandomState(seed)
    images, labels = [], []
    for _ in range(N):
        h, w = int(rng.randint(300, 501)), int(rng.randint(300, 501))
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([(o + a * yy + b * xx) % 256 for o, a, b in rng.uniform(-1, 1, size=(3, 3)) * [200, 0.5, 0.5]], -1).astype(np.uint8)
        images.append(img)
        n = int(rng.randint(1, 6))
        x0, y0 = rng.randint(0, w - 60, size=n), rng.randint(0, h - 60, size=n)
        labels.append(np.stack([rng.randint(1, 21, size=n), x0, y0, x0 + rng.randint(10, 60, size=n), y0 + rng.randint(10, 60, size=n)],
                               axis=1).astype(np.int64))
    return images, labels


def generator(images, labels):
    g = odg.DataGenerator(labels=list(labels), image_ids=list(range(N)))
    g.images, g.filenames = list(images), ["%d.jpg" % i for i in range(N)]
    g.dataset_size, g.dataset_indices = N, np.arange(N, dtype=np.int32)
    return g


def time_batches(g, transforms, reps=3):
    gen = g.generate(batch_size=B, shuffle=True, transformations=transforms, returns={'processed_images', 'processed_labels'})
    next(gen)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        next(gen)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return round(1e3 * best, 3)


def main():
    images, labels = dataset()
    lists = {"ssd_augmentation": lambda: [SSDDataAugmentation(300, 300)],
             "convert_resize": lambda: [ConvertTo3Channels(), Resize(300, 300)]}
    if "--kernels-only" in sys.argv:
        for make in lists.values():
            np.random.seed(0)
            gen = generator(images, labels).generate(batch_size=B, transformations=make(), returns={'processed_images'})
            for _ in range(20):
                next(gen)
        torch.cuda.synchronize()
        return
    res = {"what": "DataGenerator.generate(), B=32, 300x300 output, %d in-memory images of 300-500 px per side, measured on one MI355X" % N}
    for name, make in lists.items():
        np.random.seed(0)
        res[name + "_batch_path_ms_per_batch"] = time_batches(generator(images, labels), make())
        real = odg.DataGenerator.__dict__['_batch_path']
        odg.DataGenerator._batch_path = staticmethod(lambda *a: None)
        try:
            np.random.seed(0)
            res[name + "_per_image_loop_ms_per_batch"] = time_batches(generator(images, labels), make())
        finally:
            odg.DataGenerator._batch_path = real
        res[name + "_batch_path_img_per_s"] = round(B / (res[name + "_batch_path_ms_per_batch"] * 1e-3), 1)
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
