"""SSD7 (300 x 300, 5 classes, mode='inference') graphed forward + decode with `fused_blocks()` off and on, in ONE process, alternating,
with bench.py's warm-up (eager steps, then 40 untimed graph replays); plus the time of every Conv+BatchNorm+ELU(+pool) block on both
paths.  Writes profiles/ssd7_fused_blocks.json.

    python tools/time_ssd7_forward.py [--out FILE] [--batches 8,32] [--rounds 7] [--steps 200]
"""
import argparse
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(torch):
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.models.keras_ssd7 import build_model
    torch.manual_seed(0)
    model = build_model((300, 300, 3), 5, mode="inference", scales=syn.SSD7_300["scales"], normalize_coords=True, subtract_mean=127.5,
                        divide_by_stddev=127.5)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                # statistics of a trained network's kind, not the identity BatchNorm of a fresh one
        for bn in model.bns:
            n = bn.num_features
            bn.running_mean.copy_(torch.randn(n, generator=g) * 0.3)
            bn.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.5)
            bn.weight.copy_(torch.rand(n, generator=g) * 0.8 + 0.6)
            bn.bias.copy_(torch.randn(n, generator=g) * 0.3)
    return model.cuda().to(memory_format=torch.channels_last).to(torch.bfloat16).eval()


def timed(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def block_times(torch, F, model, x, fused, reps=50):
    """ms per block (its pool included), eager launches back to back: best of three bursts."""
    from ssd_keras_amd import _native as nat
    out = []
    for i in range(7):
        conv, bn = model.convs[i], model.bns[i]
        if fused:
            packed, scale, shift = model._block_tables(i)
            if i < 3:
                fn = lambda: nat.conv_bn_elu(x, packed, scale, shift, 5 if i == 0 else 3, pool=True)
            elif i < 6:
                fn = lambda: model.max_pool(nat.conv_bn_elu(x, packed, scale, shift, 3, pool=False), 2, 2)
            else:
                fn = lambda: nat.conv_bn_elu(x, packed, scale, shift, 3, pool=False)
        elif i < 6:
            fn = lambda: model.max_pool(F.elu(bn(conv(x))), 2, 2)
        else:
            fn = lambda: F.elu(bn(conv(x)))
        y = fn()
        torch.cuda.synchronize()
        out.append(min(timed(torch, fn, reps) for _ in range(3)))
        x = y
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssd7_fused_blocks.json"))
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graph-warmup", type=int, default=40)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("time_ssd7_forward needs a GPU: a time taken anywhere else says nothing")
    result = {"model": "SSD7 300x300, 5 classes, mode='inference', bf16 channels_last, graphed forward + decode",
              "device": torch.cuda.get_device_name(0), "steps_per_round": args.steps, "rounds": args.rounds, "batches": {}}
    for batch in [int(v) for v in args.batches.split(",")]:
        off = build(torch)
        on = copy.deepcopy(off).fused_blocks()
        img = torch.from_numpy(np.random.RandomState(2).randint(0, 256, size=(batch, 300, 300, 3)).astype(np.float32)).cuda()
        with torch.no_grad():
            steps = {}
            for name, model in (("off", off), ("on", on)):
                for _ in range(args.warmup):
                    model(img)
                steps[name] = model.graphed(img)
                for _ in range(max(3, args.graph_warmup)):
                    steps[name]()
            torch.cuda.synchronize()
            ms = {"off": [], "on": []}
            for _ in range(args.rounds):                 # off, on, off, on, ...: drift and neighbours hit both paths alike
                for name in ("off", "on"):
                    ms[name].append(timed(torch, steps[name], args.steps))
            x = off.preprocess(img).to(torch.bfloat16)
            blocks = {"off": block_times(torch, F, off, x, False), "on": block_times(torch, F, on, x, True)}
        entry = {}
        for name in ("off", "on"):
            v = sorted(ms[name])
            entry[name] = {"ms_per_step_rounds": ms[name], "median_ms": v[len(v) // 2], "spread_ms": v[-1] - v[0],
                           "images_per_s": batch / v[len(v) // 2] * 1e3, "block_ms_eager": blocks[name]}
        entry["speedup_median"] = entry["off"]["median_ms"] / entry["on"]["median_ms"]
        entry["on_faster_by_more_than_the_spread"] = bool(max(ms["on"]) < min(ms["off"]))
        result["batches"][str(batch)] = entry
        print("batch %d: off %.4f ms (spread %.4f), on %.4f ms (spread %.4f), x%.3f" % (
            batch, entry["off"]["median_ms"], entry["off"]["spread_ms"], entry["on"]["median_ms"], entry["on"]["spread_ms"],
            entry["speedup_median"]), flush=True)
        print("  block ms off:", " ".join("%.4f" % t for t in blocks["off"]), flush=True)
        print("  block ms on: ", " ".join("%.4f" % t for t in blocks["on"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
