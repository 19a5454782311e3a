"""SSD7 (300 x 300, 5 classes) training step -- forward + SSDLoss + backward + ssd_keras_amd.optimizers.SGD as ONE HIP graph -- three
ways: `fused_blocks` off, `fused_blocks(training=True)` ("on") and `fused_blocks(training=True, convolutions=True)` ("conv"), in ONE
process, alternating: per batch size 40 untimed replays, then seven rounds of 200 replays each way; median and spread (max - min
over the rounds) of the step time.  Per trunk convolution, the framework's call against the libssdhip call for each of forward, data
gradient and weight gradient, as HIP graphs of their own under the same protocol, with the adoption rule of DESIGN.md 4.4 applied: a
pass is adopted if its median beats the framework's by more than the spread between rounds; a layer belongs in SSD7.TRAIN_CONVS if
its three passes together win, summed over the batch sizes, by more than the spreads summed the same way.  --all-layers routes all
seven layers on the "conv" arm instead of SSD7.TRAIN_CONVS (profiles/ssd7_conv_training_all_layers.json).  Plus the eager time of what lies between a
block's convolution and the next one's (BatchNorm with batch statistics, ELU, pool; forward + backward), each way, and the
same work as a HIP graph of its own (rounds alternating, median and spread).  Writes
profiles/ssd7_conv_training.json (its "off", "on" and "blocks" entries are what this tool wrote to
profiles/ssd7_fused_training.json before it had the third arm).

    python tools/time_ssd7_train_step.py [--out FILE] [--batches 8,32] [--rounds 7] [--steps 200] [--all-layers]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


ARMS = ("off", "on", "conv")


def build(torch, arm, all_layers=False):
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.models.keras_ssd7 import build_model
    torch.manual_seed(0)
    model = build_model((300, 300, 3), 5, mode="training", scales=syn.SSD7_300["scales"], normalize_coords=True, subtract_mean=127.5,
                        divide_by_stddev=127.5)
    model = model.cuda().to(memory_format=torch.channels_last).to(torch.bfloat16).train()
    if arm == "conv" and all_layers:
        model.TRAIN_CONVS = frozenset(range(7))
    return model if arm == "off" else model.fused_blocks(True, training=True, convolutions=arm == "conv")


def timed(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def graphed_step(torch, model, images, y_true):
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    from ssd_keras_amd.optimizers import SGD
    opt = SGD(model.parameters(), lr=1e-5, momentum=0.9)
    lf = SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0)

    def step():
        opt.zero_grad(set_to_none=True)
        lf.compute_loss(y_true, model(images).float()).mean().backward()
        opt.step()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    return graph.replay


def _graphed(torch, fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    torch.cuda.synchronize()
    return graph.replay


def block_times(torch, model, batch, reps=30, rounds=5, replays=100):
    """us per block of BatchNorm (batch statistics) -> ELU [-> pool] forward + backward behind the convolution's output, the
    framework's chain and the libssdhip node.  `*_us`: eager launches back to back, best of three bursts (on the small maps this is
    the host's launch rate, not the device's time).  `*_graph_us`: the same work captured into a HIP graph, as the step runs it --
    `rounds` rounds of `replays` replays each way, alternating; median and spread (max - min)."""
    import torch.nn.functional as F
    from ssd_keras_amd.models._train_fns import _BnEluPoolFn
    out = []
    n = 300
    g = torch.Generator(device="cuda").manual_seed(3)
    for i in range(7):
        bn = model.bns[i]
        c = bn.num_features
        y = torch.randn((batch, n, n, c), device="cuda", generator=g).to(torch.bfloat16).permute(0, 3, 1, 2).requires_grad_(True)
        pool, keep = i < 6, i >= 3
        wrt = [y, bn.weight, bn.bias]

        def default():
            full = F.elu(bn(y))
            outs = ([full] if keep else []) + ([model.max_pool(full, 2, 2)] if pool else [])
            return torch.autograd.grad(outs, wrt, [torch.ones_like(o) for o in outs])

        def fused():
            full, pooled = _BnEluPoolFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, pool, keep)[:2]
            outs = [o for o in (full, pooled) if o is not None]
            return torch.autograd.grad(outs, wrt, [torch.ones_like(o) for o in outs])

        row = {"block": i + 1, "map": [batch, n, n, c]}
        fns = {"default": default, "fused": fused}
        for name, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            row[name + "_us"] = round(1e3 * min(timed(torch, fn, reps) for _ in range(3)), 1)
        graphs = {name: _graphed(torch, fn) for name, fn in fns.items()}
        times = {name: [] for name in fns}
        for _ in range(rounds):
            for name, replay in graphs.items():
                times[name].append(1e3 * timed(torch, replay, replays))
        for name, ts in times.items():
            row[name + "_graph_us"] = round(float(np.median(ts)), 1)
            row[name + "_graph_spread_us"] = round(max(ts) - min(ts), 1)
        out.append(row)
        del graphs
        if pool:
            n //= 2
    return out


def conv_layer_times(torch, model, batch, rounds=5, replays=100):
    """us per trunk convolution and pass -- forward, data gradient, weight (+ bias) gradient -- the framework's call and the libssdhip
    call on the same operands, each captured into a HIP graph of its own: `rounds` rounds of `replays` replays each way, alternating;
    median and spread (max - min).  `adopt`: the libssdhip median beats the framework's by more than the larger spread."""
    import torch.nn.functional as F
    from ssd_keras_amd import _native as nat
    aten = torch.ops.aten
    out = []
    n = 300
    g = torch.Generator(device="cuda").manual_seed(4)
    for i, conv in enumerate(model.convs):
        w, b = conv.weight.detach(), conv.bias.detach()
        cout, cin, k, _ = w.shape
        pad = k // 2
        rand = lambda c: torch.randn((batch, n, n, c), device="cuda", generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
        x, dy = rand(cin), rand(cout)
        (image,), (flipped,) = nat.ssd7_pack_images([w])
        nat.ssd7_pack_filters([w], [image], [flipped])
        back = lambda mask: aten.convolution_backward(dy, x, w, [cout], [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, mask)
        passes = {"forward": (lambda: F.conv2d(x, w, b, padding=pad), lambda: nat.ssd7_conv_bias(x, image, b, cout, k)),
                  "wgrad": (lambda: back([False, True, True]), lambda: nat.ssd7_conv_wgrad(x, dy, k, like=w))}
        if flipped is not None:
            passes["dgrad"] = (lambda: back([True, False, False]), lambda: nat.ssd7_conv_bias(dy, flipped, None, cin, k))
        row = {"layer": i + 1, "x": [batch, n, n, cin], "cout": cout, "kernel": k}
        for name, fns in passes.items():
            graphs = [_graphed(torch, fn) for fn in fns]
            times = ([], [])
            for _ in range(rounds):
                for ts, replay in zip(times, graphs):
                    ts.append(1e3 * timed(torch, replay, replays))
            med = [float(np.median(ts)) for ts in times]
            spread = [max(ts) - min(ts) for ts in times]
            row[name] = {"framework_us": round(med[0], 1), "framework_spread_us": round(spread[0], 1), "libssdhip_us": round(med[1], 1),
                         "libssdhip_spread_us": round(spread[1], 1), "adopt": bool(med[0] - med[1] > max(spread))}
            del graphs
        row["framework_sum_us"] = round(sum(row[p]["framework_us"] for p in passes), 1)
        row["libssdhip_sum_us"] = round(sum(row[p]["libssdhip_us"] for p in passes), 1)
        row["spread_sum_us"] = round(sum(max(row[p]["framework_spread_us"], row[p]["libssdhip_spread_us"]) for p in passes), 1)
        out.append(row)
        if i < 6:
            n //= 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssd7_conv_training.json"))
    ap.add_argument("--all-layers", action="store_true", help="the conv arm routes all seven layers, not SSD7.TRAIN_CONVS")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_ssd7_train_step.py needs a GPU: there is nothing to time without one")
    result = {"device": torch.cuda.get_device_name(0), "model": "SSD7 300x300x3, 5 classes, bf16, train()",
              "step": "forward + SSDLoss + backward + ssd_keras_amd.optimizers.SGD, one HIP graph", "rounds": args.rounds,
              "steps_per_round": args.steps, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        images = torch.from_numpy(np.random.RandomState(100).randint(0, 256, size=(batch, 300, 300, 3)).astype(np.float32)).cuda()
        models = {arm: build(torch, arm, args.all_layers) for arm in ARMS}
        with torch.no_grad():
            n_anchor, width = models["off"].eval()(images[:1]).shape[1:]
        models["off"].train()
        rng = np.random.RandomState(7)
        y = np.zeros((batch, n_anchor, width), dtype=np.float32)
        pos = rng.rand(batch, n_anchor) < 1.0 / 16
        cls = rng.randint(1, width - 12, size=(batch, n_anchor))
        y[..., 0] = ~pos
        for k in range(1, width - 12):
            y[..., k] = pos & (cls == k)
        y[..., width - 12:width - 8] = rng.randn(batch, n_anchor, 4) * 0.5 * pos[..., None]
        y_true = torch.from_numpy(y).cuda()
        replays = {k: graphed_step(torch, m, images, y_true) for k, m in models.items()}
        for fn in replays.values():
            timed(torch, fn, 40)
        rounds = {arm: [] for arm in ARMS}
        for _ in range(args.rounds):
            for k in ARMS:
                rounds[k].append(timed(torch, replays[k], args.steps))
        entry = {}
        for k in ARMS:
            entry[k] = {"median_ms": round(float(np.median(rounds[k])), 4), "spread_ms": round(max(rounds[k]) - min(rounds[k]), 4),
                        "rounds_ms": [round(v, 4) for v in rounds[k]]}
        entry["blocks"] = block_times(torch, models["on"], batch)
        entry["convolutions"] = conv_layer_times(torch, models["conv"], batch)
        result["batches"][str(batch)] = entry
        print(json.dumps({"batch": batch, **entry}), flush=True)
        del replays, models
        torch.cuda.empty_cache()
    # the adoption rule: a layer's three passes together, summed over the batch sizes
    layers = {}
    for entry in result["batches"].values():
        for row in entry["convolutions"]:
            fw, own, spread = layers.get(row["layer"], (0.0, 0.0, 0.0))
            layers[row["layer"]] = (fw + row["framework_sum_us"], own + row["libssdhip_sum_us"], spread + row["spread_sum_us"])
    result["layers"] = [{"layer": i, "framework_us": round(fw, 1), "libssdhip_us": round(own, 1), "spread_us": round(spread, 1),
                         "adopt": fw - own > spread} for i, (fw, own, spread) in sorted(layers.items())]
    from ssd_keras_amd.models.keras_ssd7 import SSD7
    result["conv_arm_layers"] = sorted(i + 1 for i in (range(7) if args.all_layers else SSD7.TRAIN_CONVS))
    print(json.dumps({"layers": result["layers"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
