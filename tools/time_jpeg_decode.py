"""Time `jpeg_decode.decode_jpeg_batch` against the loop of PIL decodes it replaces (needs a GPU; run from the repository root).

    python tools/time_jpeg_decode.py [--out profiles/jpeg_decode.json] [--rounds 5]
    python tools/time_jpeg_decode.py --indexed [--out profiles/jpeg_index.json] [--rounds 5]

Synthetic 375 x 500 JPEGs at quality 75, 4:2:0 (a smooth pattern plus noise, 8 distinct images cycled to the batch size), without
restart markers, with one per MCU row and with one per MCU; batches of 32 and 256 files, given as bytes (no file system in either
arm).  Device arm: host bytes in -> device images ready (the call ends with the download of the status words, so it is synchronised).
Host arm: `_load_image` over the same bytes, one thread.  The arms alternate in one process, `--rounds` rounds after one warm-up
round; medians and the min..max spread are reported.  A second pass splits the device arm with events: host planning and packing
(host clock), upload, entropy, block and pixel stage.  The per-lane symbol rate is Huffman symbols of the longest segment over the
entropy stage's time (the stage ends when its slowest lane does).

`--indexed`: the files WITHOUT restart markers only, four arms alternating in one process: the device arm as above (no index: one
lane per file), the same call with an empty `JpegIndex` (cold: the sequential decode plus the recording of every MCU row's entry),
the same call with the index that cold call filled (warm: one lane per MCU row, each verifying its end), and the PIL loop; the
order of the arms rotates from round to round (a device arm behind the PIL loop meets an idle device).  The
entropy stage of the cold and the warm call is split off with events as above."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_jpeg(seed, restart):
    from PIL import Image
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:375, 0:500]
    base = np.stack([127 + 80 * np.sin(0.031 * xx + 0.7 * k + seed) * np.cos(0.023 * yy - 0.4 * k) + 30 * np.sin(0.4 * xx + 0.3 * yy + k)
                     for k in range(3)], axis=-1)
    img = np.clip(base + rng.normal(0, 10, base.shape), 0, 255).astype(np.uint8)
    kw = dict(quality=75, subsampling=2)
    if restart == "row":
        kw["restart_marker_rows"] = 1
    elif restart == "mcu":
        kw["restart_marker_blocks"] = 1
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def symbols_per_segment(data):
    """Huffman symbols of every segment of a file, counted from the coefficients of the NumPy restatement."""
    from tests import np_jpeg
    p = np_jpeg.parse(data)
    coef, status = np_jpeg.entropy(data, p)
    assert status == 0
    hs, vs, mcux, mcuy, grids = np_jpeg.geometry(p)
    zz = coef[:, np_jpeg.NATURAL]                                # zigzag order
    per_block = np.ones(len(zz), dtype=np.int64)                 # the DC symbol
    for b, row in enumerate(zz):
        nz = np.flatnonzero(row[1:]) + 1
        prev = 0
        for k in nz:
            per_block[b] += 1 + (k - prev - 1) // 16             # the coefficient's symbol and the ZRLs in front of it
            prev = k
        per_block[b] += prev < 63                                # EOB
    interval = p.interval or mcux * mcuy
    bases = np.concatenate([[0], np.cumsum([h * w for h, w in grids])])
    per_mcu = np.zeros(mcux * mcuy, dtype=np.int64)
    for c, (gh, gw) in enumerate(grids):
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        g = per_block[bases[c]:bases[c + 1]].reshape(mcuy, cv, mcux, ch).sum(axis=(1, 3))
        per_mcu += g.reshape(-1)
    return [int(per_mcu[s:s + interval].sum()) for s in range(0, mcux * mcuy, interval)]


def spread(values):
    return {"median_ms": round(1e3 * statistics.median(values), 3), "min_ms": round(1e3 * min(values), 3), "max_ms": round(1e3 * max(values), 3)}


def main_indexed(args):
    import torch
    from ssd_keras_amd.data_generator import jpeg_decode
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import _load_image

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    result = {"device": torch.cuda.get_device_name(0), "image": "375x500 quality 75 4:2:0, synthetic, no restart markers",
              "rounds": args.rounds, "cases": []}
    distinct = [make_jpeg(seed, None) for seed in range(8)]
    want = [_load_image(io.BytesIO(d)) for d in distinct]
    for batch in args.batches:
        datas = [distinct[i % 8] for i in range(batch)]
        plans = [jpeg_decode.plan_jpeg(d) for d in datas]
        warm_index = jpeg_decode.JpegIndex()
        for _ in range(2):                                       # warm-up of every arm (cold, then warm), and the check that they agree
            got = jpeg_decode.decode_jpeg_batch(datas, index=warm_index)
            assert all(torch.is_tensor(g) and np.array_equal(g.cpu().numpy(), want[i % 8]) for i, g in enumerate(got))
        jpeg_decode.decode_jpeg_batch(datas)
        arms = {k: [] for k in ("device_no_index", "cold_recording", "warm_indexed", "host_pil")}
        counters = dict(jpeg_decode.COUNTERS)
        calls = {"device_no_index": lambda: jpeg_decode.decode_jpeg_batch(datas),
                 "cold_recording": lambda: jpeg_decode.decode_jpeg_batch(datas, index=jpeg_decode.JpegIndex()),
                 "warm_indexed": lambda: jpeg_decode.decode_jpeg_batch(datas, index=warm_index),
                 "host_pil": lambda: [_load_image(io.BytesIO(d)) for d in datas]}
        order = list(calls)
        for r in range(args.rounds):                             # the order rotates: no arm always runs behind the same neighbour
            for name in order[r % 4:] + order[:r % 4]:
                arms[name].append(timed(calls[name]))
        moved = {k: jpeg_decode.COUNTERS[k] - counters[k] for k in counters}
        # (the digest keys make equal bytes one entry: a cold call records the 8 distinct files' entries batch / 8 times over)
        assert moved["recorded"] == moved["indexed"] == batch * args.rounds and moved["host"] == 0, moved
        rows = [warm_index[jpeg_decode.JpegIndex.key(d, d)] for d in datas]
        entropy = {"cold_recording": [], "warm_indexed": []}
        for _ in range(args.rounds):
            for name, index_rows in (("cold_recording", [jpeg_decode.RECORD] * batch), ("warm_indexed", rows)):
                marks = []

                def mark():
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    marks.append(e)

                _, status, _ = jpeg_decode.decode_planned(plans, datas, events=mark, index_rows=index_rows)
                torch.cuda.synchronize()
                assert not status.any()
                entropy[name].append(1e-3 * marks[0].elapsed_time(marks[1]))
        n_entries = sum(len(r) for r in rows)
        med = {k: statistics.median(v) for k, v in arms.items()}
        case = {"batch": batch, "file_bytes": int(np.mean([len(d) for d in distinct])), "entries": n_entries,
                "entry_lanes_per_wave": jpeg_decode.lanes_per_wave(n_entries), "index_bytes_per_file": int(32 * n_entries / batch),
                **{k: spread(v) for k, v in arms.items()},
                "entropy_stage": {k: spread(v) for k, v in entropy.items()},
                "warm_over_device_no_index": round(med["device_no_index"] / med["warm_indexed"], 3),
                "warm_over_host_pil": round(med["host_pil"] / med["warm_indexed"], 3),
                "cold_over_device_no_index": round(med["device_no_index"] / med["cold_recording"], 3)}
        print(json.dumps(case), flush=True)
        result["cases"].append(case)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--indexed", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_jpeg_decode.py measures on the GPU; none is visible")
    from ssd_keras_amd.data_generator import jpeg_decode
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import _load_image

    args.out = args.out or os.path.join("profiles", "jpeg_index.json" if args.indexed else "jpeg_decode.json")
    result = {"device": torch.cuda.get_device_name(0), "image": "375x500 quality 75 4:2:0, synthetic", "rounds": args.rounds, "cases": []}
    for restart in (() if args.indexed else (None, "row", "mcu")):
        distinct = [make_jpeg(seed, restart) for seed in range(8)]
        counts = [symbols_per_segment(d) for d in distinct]
        for batch in args.batches:
            datas = [distinct[i % 8] for i in range(batch)]
            want = [_load_image(io.BytesIO(d)) for d in distinct]
            got = jpeg_decode.decode_jpeg_batch(datas)           # warm-up of both arms, and the check that they agree
            assert all(torch.is_tensor(g) and np.array_equal(g.cpu().numpy(), want[i % 8]) for i, g in enumerate(got))
            dev, host = [], []
            for _ in range(args.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                jpeg_decode.decode_jpeg_batch(datas)
                torch.cuda.synchronize()
                dev.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                for d in datas:
                    _load_image(io.BytesIO(d))
                host.append(time.perf_counter() - t0)
            stages = {k: [] for k in ("plan_pack_host", "upload", "entropy", "block", "pixel")}
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                plans = [jpeg_decode.plan_jpeg(d) for d in datas]
                jpeg_decode.pack_plans(plans, datas)
                stages["plan_pack_host"].append(time.perf_counter() - t0)
                marks = []

                def mark():
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    marks.append(e)

                mark()
                jpeg_decode.decode_planned(plans, datas, events=mark)
                torch.cuda.synchronize()
                for name, a, b in zip(("upload", "entropy", "block", "pixel"), marks[:-1], marks[1:]):
                    stages[name].append(1e-3 * a.elapsed_time(b))
            entropy_s = statistics.median(stages["entropy"])
            n_segments = sum(len(c) for c in counts) * batch // 8
            case = {"restart": restart or "none", "batch": batch, "file_bytes": int(np.mean([len(d) for d in distinct])),
                    "segments": n_segments, "lanes_per_wave": jpeg_decode.lanes_per_wave(n_segments),
                    "symbols_per_image": int(np.mean([sum(c) for c in counts])), "symbols_longest_segment": max(max(c) for c in counts),
                    "device": spread(dev), "host_pil": spread(host),
                    "speedup_median": round(statistics.median(host) / statistics.median(dev), 3),
                    "stages": {k: spread(v) for k, v in stages.items()},
                    "symbols_per_second_per_lane": round(max(max(c) for c in counts) / entropy_s),
                    "symbols_per_second_all_lanes": round(sum(sum(c) for c in counts) * batch / 8 / entropy_s)}
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    if args.indexed:
        result = main_indexed(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
