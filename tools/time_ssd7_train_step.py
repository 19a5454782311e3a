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

--master-weights times the optimizer's side of the same step instead, under the same protocol: the "conv" model (bf16 parameters) with
`--optimizer {sgd,adam}` built with `master_weights=False` (bf16 parameters through the optimizer's tensor expressions) and with
`master_weights=True` (float32 masters, ssdhip_sgd_step_bf16 / ssdhip_adam_step_bf16), alternating in one process; plus, after the
timings, the nodes of each captured graph by type and the kernel launches of one eager run of the same step.  Writes
profiles/ssd7_master_weights.json.

    python tools/time_ssd7_train_step.py --master-weights [--optimizer sgd|adam] [--out FILE] [--batches 8,32] [--rounds 7] [--steps 200]

--heads times `fused_blocks(True, training=True, convolutions=True, heads=True)` against its parent route, the same call without
`heads`, both with SGD(master_weights=True), under the same protocol; plus, per source map and pass of the predictor heads and for
the prediction assembly, the framework's calls against the libssdhip call (the weight gradient in both of libssdhip's forms), and
the nodes of each captured graph.  Writes profiles/ssd7_head_training.json.

    python tools/time_ssd7_train_step.py --heads [--out FILE] [--batches 8,32] [--rounds 7] [--steps 200]

--clipnorm VALUE times what gradient clipping adds to the `heads=True` step with SGD(master_weights=True): the optimizer built without
the keyword ("clip_off": the step of before, no launch added) against `clipnorm=VALUE` ("clip_on": one sum-of-squares launch per tensor
table, the finish launch, the clipped update), alternating in one process under the same protocol; plus the nodes of each captured
graph and the clipped arm's `clip_stats` and last `grad_norm`.  The cost does not depend on whether VALUE binds: the multiplication by
the scale always happens.  The result is one more entry of "visits" in profiles/optim_clip.json (the file is kept and appended to).

    python tools/time_ssd7_train_step.py --clipnorm 1.0 [--out FILE] [--batches 8,32] [--rounds 7] [--steps 200]

The unclipped arm against ANOTHER COMMIT (the parent of the change) is three more calls.  --clip-baseline is the same process with two
unclipped arms ("clip_off", "clip_off_twin": two models and two graphs alternating, as above); it uses nothing but this file and the
package's public interface, so a copy of this file runs it in a checkout of the other commit -- once before and once after the
--clipnorm run.  --clip-parents BEFORE,AFTER (no GPU needed) then writes the two into the last visit as "parent_commit", with
clip_off minus each and whether it lies within the sum of the two arms' spreads, and recounts "summary" over all visits.

    python tools/time_ssd7_train_step.py --clip-baseline --out FILE          (in the other commit's checkout, before and after)
    python tools/time_ssd7_train_step.py --clip-parents BEFORE,AFTER [--out profiles/optim_clip.json]
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


def graphed_step(torch, model, images, y_true, optimizer="sgd", master_weights=False, counted=False, clip=None):
    """The replay of the step captured as one HIP graph; with `counted` (replay, the eager step, the graph object kept for its nodes,
    the optimizer).  `clip`: the optimizer's clipping keywords."""
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    from ssd_keras_amd.optimizers import SGD, Adam
    if optimizer == "sgd":
        opt = SGD(model.parameters(), lr=1e-5, momentum=0.9, master_weights=master_weights, **(clip or {}))
    else:
        opt = Adam(model.parameters(), lr=1e-5, epsilon=1e-8, master_weights=master_weights, **(clip or {}))
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
    graph = None
    if counted:
        try:
            graph = torch.cuda.CUDAGraph(keep_graph=True)           # the captured graph stays readable: graph_nodes()
        except TypeError:
            pass
    graph = graph or torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    return (graph.replay, step, graph, opt) if counted else graph.replay


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


def synthetic_targets(batch, n_anchor, width):
    """A fixed encoded batch: every anchor background except one in sixteen, which carries a class and box offsets."""
    rng = np.random.RandomState(7)
    y = np.zeros((batch, n_anchor, width), dtype=np.float32)
    pos = rng.rand(batch, n_anchor) < 1.0 / 16
    cls = rng.randint(1, width - 12, size=(batch, n_anchor))
    y[..., 0] = ~pos
    for k in range(1, width - 12):
        y[..., k] = pos & (cls == k)
    y[..., width - 12:width - 8] = rng.randn(batch, n_anchor, 4) * 0.5 * pos[..., None]
    return y


def graph_nodes(graph):
    """{"kernel": n, "memcpy": n, "memset": n, "other": n} of a captured graph kept with keep_graph=True, read through the HIP runtime's
    hipGraphGetNodes / hipGraphNodeGetType (queries only); None where the framework or the runtime does not offer them."""
    import ctypes
    try:
        handle = ctypes.c_void_p(int(graph.raw_cuda_graph()))
        with open("/proc/self/maps") as maps:                        # the runtime the framework has loaded, not a second copy
            loaded = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
        if len(loaded) != 1:
            return None
        hip = ctypes.CDLL(loaded[0])
        n = ctypes.c_size_t(0)
        if hip.hipGraphGetNodes(handle, None, ctypes.byref(n)) != 0 or n.value == 0:
            return None
        nodes = (ctypes.c_void_p * n.value)()
        if hip.hipGraphGetNodes(handle, nodes, ctypes.byref(n)) != 0:
            return None
        names = {0: "kernel", 1: "memcpy", 2: "memset"}              # hipGraphNodeTypeKernel, ...Memcpy, ...Memset
        out = {"kernel": 0, "memcpy": 0, "memset": 0, "other": 0}
        for node in nodes[:n.value]:
            kind = ctypes.c_int(-1)
            if hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) != 0:
                return None
            out[names.get(kind.value, "other")] += 1
        return out
    except Exception:                                         # noqa: BLE001
        return None


def eager_launches(torch, fn):
    """Kernel launches of one EAGER call of `fn` (the launches a capture records), counted by the framework's profiler; None where it
    records no device activity."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "mem" not in e.name.lower())
        return n or None
    except Exception:                                         # noqa: BLE001
        return None


def master_weights_arms(torch, args):
    """The bf16 step of the "conv" model with the optimizer's masters off (the parameters updated in bf16 by the tensor expressions)
    and on (one or two libssdhip launches on float32 masters): arms alternating, median and spread as in main()."""
    arms = {"master_weights_off": False, "master_weights_on": True}
    result = {"device": torch.cuda.get_device_name(0), "model": "SSD7 300x300x3, 5 classes, bf16, train(), fused_blocks(True, training=True, "
              "convolutions=True)", "optimizer": args.optimizer,
              "step": "forward + SSDLoss + backward + ssd_keras_amd.optimizers.%s, one HIP graph" % args.optimizer.upper(),
              "rounds": args.rounds, "steps_per_round": args.steps, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        images = torch.from_numpy(np.random.RandomState(100).randint(0, 256, size=(batch, 300, 300, 3)).astype(np.float32)).cuda()
        models = {arm: build(torch, "conv") for arm in arms}
        with torch.no_grad():
            n_anchor, width = build(torch, "off").eval()(images[:1]).shape[1:]
        y_true = torch.from_numpy(synthetic_targets(batch, n_anchor, width)).cuda()
        captured = {arm: graphed_step(torch, models[arm], images, y_true, args.optimizer, on, counted=True) for arm, on in arms.items()}
        replays = {arm: c[0] for arm, c in captured.items()}
        for fn in replays.values():
            timed(torch, fn, 40)
        rounds = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                rounds[arm].append(timed(torch, replays[arm], args.steps))
        entry = {}
        for arm in arms:
            entry[arm] = {"median_ms": round(float(np.median(rounds[arm])), 4), "spread_ms": round(max(rounds[arm]) - min(rounds[arm]), 4),
                          "rounds_ms": [round(v, 4) for v in rounds[arm]]}
        for arm in arms:                                           # last: nothing here may disturb the timings above
            entry[arm]["graph_nodes"] = graph_nodes(captured[arm][2])
            entry[arm]["eager_kernel_launches"] = eager_launches(torch, captured[arm][1])
        off, on = entry["master_weights_off"], entry["master_weights_on"]
        entry["on_minus_off_ms"] = round(on["median_ms"] - off["median_ms"], 4)
        entry["not_slower"] = bool(on["median_ms"] - off["median_ms"] <= max(on["spread_ms"], off["spread_ms"]))
        result["batches"][str(batch)] = entry
        print(json.dumps({"batch": batch, **entry}), flush=True)
        del replays, captured, models
        torch.cuda.empty_cache()
    result["note"] = ("the step time is the only performance claim; convergence over a real training run is not measured.  "
                      "graph_nodes: the nodes of the captured step by type, read from the HIP graph itself; eager_kernel_launches: the "
                      "kernel activities the framework's profiler records for one eager run of the same step")
    return result


def _alternating(torch, fns, rounds, replays):
    """{name: (median us, spread us)} of the calls in `fns`, each captured into a HIP graph of its own: `rounds` rounds of `replays`
    replays each, alternating."""
    graphs = {name: _graphed(torch, fn) for name, fn in fns.items()}
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, replay in graphs.items():
            times[name].append(1e3 * timed(torch, replay, replays))
    return {name: (float(np.median(ts)), max(ts) - min(ts)) for name, ts in times.items()}


def head_times(torch, model, batch, rounds=5, replays=100):
    """us per source map and pass of the predictor heads -- forward, data gradient, parameter gradients -- the framework's calls (two
    convolutions; for the data gradient also their sum) against the one libssdhip call on the packed head, each captured into a HIP
    graph of its own, rounds alternating; median and spread (max - min).  The weight gradient is timed in both of libssdhip's forms:
    `libssdhip_us` is ssdhip_ssd7_head_wgrad (the padded position list), `tile_form_us` is ssdhip_ssd7_conv_wgrad on the same packed
    operands (8 x 32 position tiles; it returns the packed rows, not the four parameter gradients).  Last row: the prediction assembly,
    forward + backward, the framework's permute / reshape / cat / softmax / cat chain against `_AssembleTrainFn`."""
    import torch.nn.functional as F
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.models._train_fns import _AssembleTrainFn
    aten = torch.ops.aten
    out = []
    g = torch.Generator(device="cuda").manual_seed(5)
    conf_w, loc_w = [c.weight.detach() for c in model.conf_heads], [c.weight.detach() for c in model.loc_heads]
    conf_b, loc_b = [c.bias.detach() for c in model.conf_heads], [c.bias.detach() for c in model.loc_heads]
    fwd, flipped, bias = nat.ssd7_head_images(conf_w, loc_w)
    nat.ssd7_pack_heads(conf_w, loc_w, conf_b, loc_b, fwd, flipped, bias)
    sizes = [tuple(int(v) for v in s) for s in model.predictor_sizes()]
    rand = lambda n, h, w, c: torch.randn((n, h, w, c), device="cuda", generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
    for l, (h, w) in enumerate(sizes):
        wc, wl, bc, bl = conf_w[l], loc_w[l], conf_b[l], loc_b[l]
        nc, nl, cin = wc.shape[0], wl.shape[0], wc.shape[1]
        x, dy = rand(batch, h, w, cin), rand(batch, h, w, nat.SSD7_HEAD_CP)
        dyc, dyl = dy[:, :nc].contiguous(memory_format=torch.channels_last), dy[:, nc:nc + nl].contiguous(memory_format=torch.channels_last)
        back = lambda d, wt, mask: aten.convolution_backward(d, x, wt, [wt.shape[0]], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, mask)
        passes = {
            "forward": {"framework": lambda: (F.conv2d(x, wc, bc, padding=1), F.conv2d(x, wl, bl, padding=1)),
                        "libssdhip": lambda: nat.ssd7_conv_bias(x, fwd[l], bias[l], nat.SSD7_HEAD_CP, 3)},
            "dgrad": {"framework": lambda: back(dyc, wc, [True, False, False])[0] + back(dyl, wl, [True, False, False])[0],
                      "libssdhip": lambda: nat.ssd7_conv_bias(dy, flipped[l], None, cin, 3)},
            "wgrad": {"framework": lambda: (back(dyc, wc, [False, True, True]), back(dyl, wl, [False, True, True])),
                      "libssdhip": lambda: nat.ssd7_head_wgrad(x, dy, wc, wl),
                      "tile_form": lambda: nat.ssd7_conv_wgrad(x, dy, 3)}}
        row = {"map": l + 4, "x": [batch, h, w, cin], "packed": [nc, nl, nat.SSD7_HEAD_CP],
               "wgrad_plan": list(nat.ssd7_head_wgrad_plan(batch, h, w, cin)), "tile_form_plan": list(nat.ssd7_conv_wgrad_plan(batch, h, w, cin, 48, 3))}
        for name, fns in passes.items():
            got = _alternating(torch, fns, rounds, replays)
            row[name] = {k + "_us": round(v[0], 1) for k, v in got.items()}
            row[name].update({k + "_spread_us": round(v[1], 1) for k, v in got.items()})
            row[name]["adopt"] = bool(got["framework"][0] - got["libssdhip"][0] > max(got["framework"][1], got["libssdhip"][1]))
        row["framework_sum_us"] = round(sum(row[p]["framework_us"] for p in passes), 1)
        row["libssdhip_sum_us"] = round(sum(row[p]["libssdhip_us"] for p in passes), 1)
        out.append(row)
    # the assembly: forward + backward from the head maps to dL/d(head maps), the upstream gradient fixed
    n_boxes = [int(pb.n_boxes) for pb in model.priorboxes]
    ncls = model.n_classes
    anchors = model.anchors_and_variances(sizes, torch.device("cuda", torch.cuda.current_device()))
    ys = [rand(batch, h, w, nat.SSD7_HEAD_CP).requires_grad_(True) for h, w in sizes]
    confs = [rand(batch, h, w, nb * ncls).requires_grad_(True) for (h, w), nb in zip(sizes, n_boxes)]
    locs = [rand(batch, h, w, nb * 4).requires_grad_(True) for (h, w), nb in zip(sizes, n_boxes)]
    up = torch.randn((batch, anchors.shape[0], ncls + 12), device="cuda", generator=g)

    def chain():
        c = torch.softmax(torch.cat([t.permute(0, 2, 3, 1).reshape(batch, -1, ncls) for t in confs], dim=1).float(), dim=-1)
        lo = torch.cat([t.permute(0, 2, 3, 1).reshape(batch, -1, 4) for t in locs], dim=1).float()
        pred = torch.cat([c, lo, anchors.unsqueeze(0).expand(batch, -1, -1)], dim=2)
        return torch.autograd.grad([pred], confs + locs, [up])

    def own():
        return torch.autograd.grad([_AssembleTrainFn.apply(anchors, ncls, n_boxes, *ys)], ys, [up])

    got = _alternating(torch, {"framework": chain, "libssdhip": own}, rounds, replays)
    row = {"map": "assembly", "anchors": int(anchors.shape[0])}
    row.update({k + "_us": round(v[0], 1) for k, v in got.items()})
    row.update({k + "_spread_us": round(v[1], 1) for k, v in got.items()})
    row["adopt"] = bool(got["framework"][0] - got["libssdhip"][0] > max(got["framework"][1], got["libssdhip"][1]))
    out.append(row)
    return out


def heads_arms(torch, args):
    """The bf16 step with SGD(master_weights=True) on the parent route (`training=True, convolutions=True`) and with `heads=True` on top
    of it: arms alternating, median and spread as in main(); then the per-map, per-pass table and the nodes of each captured graph."""
    arms = {"parent": False, "heads": True}
    result = {"device": torch.cuda.get_device_name(0), "model": "SSD7 300x300x3, 5 classes, bf16, train(), fused_blocks(True, training=True, "
              "convolutions=True[, heads=True])",
              "step": "forward + SSDLoss + backward + ssd_keras_amd.optimizers.SGD(master_weights=True), one HIP graph",
              "rounds": args.rounds, "steps_per_round": args.steps, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        images = torch.from_numpy(np.random.RandomState(100).randint(0, 256, size=(batch, 300, 300, 3)).astype(np.float32)).cuda()
        models = {arm: build(torch, "conv").fused_blocks(True, training=True, convolutions=True, heads=on) for arm, on in arms.items()}
        with torch.no_grad():
            n_anchor, width = build(torch, "off").eval()(images[:1]).shape[1:]
        y_true = torch.from_numpy(synthetic_targets(batch, n_anchor, width)).cuda()
        captured = {arm: graphed_step(torch, models[arm], images, y_true, "sgd", True, counted=True) for arm in arms}
        replays = {arm: c[0] for arm, c in captured.items()}
        for fn in replays.values():
            timed(torch, fn, 40)
        rounds = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                rounds[arm].append(timed(torch, replays[arm], args.steps))
        entry = {}
        for arm in arms:
            entry[arm] = {"median_ms": round(float(np.median(rounds[arm])), 4), "spread_ms": round(max(rounds[arm]) - min(rounds[arm]), 4),
                          "rounds_ms": [round(v, 4) for v in rounds[arm]]}
        for arm in arms:                                           # last: nothing here may disturb the timings above
            entry[arm]["graph_nodes"] = graph_nodes(captured[arm][2])
            entry[arm]["eager_kernel_launches"] = eager_launches(torch, captured[arm][1])
        parent, heads = entry["parent"], entry["heads"]
        entry["heads_minus_parent_ms"] = round(heads["median_ms"] - parent["median_ms"], 4)
        entry["faster"] = bool(parent["median_ms"] - heads["median_ms"] > parent["spread_ms"] + heads["spread_ms"])
        entry["head_maps"] = head_times(torch, models["heads"], batch)
        result["batches"][str(batch)] = entry
        print(json.dumps({"batch": batch, **entry}), flush=True)
        del replays, captured, models
        torch.cuda.empty_cache()
    result["note"] = ("faster: the medians differ by more than the sum of the two arms' spreads (the rule behind SSD7.TRAIN_CONVS).  "
                      "graph_nodes: the nodes of the captured step by type, read from the HIP graph itself; eager_kernel_launches: the "
                      "kernel activities the framework's profiler records for one eager run of the same step")
    return result


def clip_arms(torch, args):
    """The `heads=True` step with SGD(master_weights=True) built without clipping keywords and with `clipnorm`: arms alternating, median
    and spread as in main(); then the nodes of each captured graph and what the clipped optimizer counted."""
    arms = {"clip_off": None, "clip_off_twin": None} if args.clip_baseline else {"clip_off": None, "clip_on": {"clipnorm": args.clipnorm}}
    result = {"device": torch.cuda.get_device_name(0), "model": "SSD7 300x300x3, 5 classes, bf16, train(), fused_blocks(True, training=True, "
              "convolutions=True, heads=True)", "clipnorm": args.clipnorm,
              "step": "forward + SSDLoss + backward + ssd_keras_amd.optimizers.SGD(master_weights=True[, clipnorm=...]), one HIP graph",
              "rounds": args.rounds, "steps_per_round": args.steps, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        images = torch.from_numpy(np.random.RandomState(100).randint(0, 256, size=(batch, 300, 300, 3)).astype(np.float32)).cuda()
        models = {arm: build(torch, "conv").fused_blocks(True, training=True, convolutions=True, heads=True) for arm in arms}
        with torch.no_grad():
            n_anchor, width = build(torch, "off").eval()(images[:1]).shape[1:]
        y_true = torch.from_numpy(synthetic_targets(batch, n_anchor, width)).cuda()
        captured = {arm: graphed_step(torch, models[arm], images, y_true, "sgd", True, counted=True, clip=clip) for arm, clip in arms.items()}
        replays = {arm: c[0] for arm, c in captured.items()}
        for fn in replays.values():
            timed(torch, fn, 40)
        rounds = {arm: [] for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                rounds[arm].append(timed(torch, replays[arm], args.steps))
        entry = {}
        for arm in arms:
            entry[arm] = {"median_ms": round(float(np.median(rounds[arm])), 4), "spread_ms": round(max(rounds[arm]) - min(rounds[arm]), 4),
                          "rounds_ms": [round(v, 4) for v in rounds[arm]]}
        for arm in arms:                                           # last: nothing here may disturb the timings above
            entry[arm]["graph_nodes"] = graph_nodes(captured[arm][2])
        if not args.clip_baseline:
            opt = captured["clip_on"][3]
            entry["clip_on"]["clip_stats"], entry["clip_on"]["grad_norm"] = opt.clip_stats, opt.grad_norm
            entry["on_minus_off_ms"] = round(entry["clip_on"]["median_ms"] - entry["clip_off"]["median_ms"], 4)
            del opt
        result["batches"][str(batch)] = entry
        print(json.dumps({"batch": batch, **entry}), flush=True)
        del replays, captured, models
        torch.cuda.empty_cache()
    if args.clip_baseline:
        return result
    whole = _clip_file(args.out) or {k: v for k, v in result.items() if k != "batches"}
    whole.setdefault("visits", []).append({"parent_protocol": CLIP_PROTOCOL, "batches": result["batches"]})
    return _clip_summary(whole)


CLIP_PROTOCOL = "--clip-baseline: two unclipped models and graphs alternating in the other commit's process, its first arm compared"
CLIP_NOTE = ("one entry of `visits` per --clipnorm run.  clip_off is the optimizer built without the keywords: the step of before, no launch "
             "added; on_minus_off_ms is what clipping costs and is reported, not gated.  parent_commit: the same step in a checkout of the "
             "parent commit, processes of their own before and after the --clipnorm run; off_minus_parent_ms: clip_off's median minus "
             "each; off_within_the_spreads: |that| <= the sum of the two arms' spreads (max - min over the rounds).  summary counts the "
             "comparisons of all visits.  graph_nodes: the nodes of the captured step by type, read from the HIP graph itself")


def _clip_file(path):
    if os.path.exists(path):
        with open(path) as f:
            whole = json.load(f)
        if "visits" in whole:
            return whole
    return None


def _clip_summary(whole):
    diffs, within = [], 0
    for visit in whole["visits"]:
        for entry in visit["batches"].values():
            for when, d in entry.get("off_minus_parent_ms", {}).items():
                diffs.append(round(1e3 * d, 1))
                within += bool(entry["off_within_the_spreads"][when])
    whole["summary"] = {"comparisons_with_the_parent_commit": len(diffs), "within_the_spreads": within,
                        "outside_the_spreads": len(diffs) - within, "off_minus_parent_us": diffs}
    whole["note"] = CLIP_NOTE
    return whole


def clip_parents(args):
    """--clip-parents BEFORE,AFTER: the other commit's two --clip-baseline runs into the last visit of the file."""
    whole = _clip_file(args.out)
    if whole is None:
        raise SystemExit("%s holds no --clipnorm visit to add the parent commit's runs to" % args.out)
    runs = {}
    for when, path in zip(("before", "after"), args.clip_parents.split(",")):
        with open(path) as f:
            runs[when] = json.load(f)["batches"]
    visit = whole["visits"][-1]
    visit["parent_protocol"] = CLIP_PROTOCOL
    for batch, entry in visit["batches"].items():
        off = entry["clip_off"]
        entry["parent_commit"] = {when: run[batch]["clip_off"] for when, run in runs.items()}
        entry["parent_commit_twin"] = {when: run[batch]["clip_off_twin"] for when, run in runs.items()}
        entry["off_minus_parent_ms"] = {when: round(off["median_ms"] - was["median_ms"], 4) for when, was in entry["parent_commit"].items()}
        entry["off_within_the_spreads"] = {when: bool(abs(off["median_ms"] - was["median_ms"]) <= off["spread_ms"] + was["spread_ms"])
                                           for when, was in entry["parent_commit"].items()}
    return _clip_summary(whole)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/ssd7_conv_training.json (profiles/ssd7_master_weights.json with "
                    "--master-weights)")
    ap.add_argument("--master-weights", action="store_true", help="time the optimizer's masters off against on instead of the three routes")
    ap.add_argument("--heads", action="store_true", help="time heads=True against the parent route (training=True, convolutions=True), "
                    "both with SGD(master_weights=True), instead of the three routes")
    ap.add_argument("--clipnorm", type=float, default=None, help="time SGD(master_weights=True) without and with clipnorm=VALUE on the "
                    "heads=True step instead of the three routes")
    ap.add_argument("--clip-baseline", action="store_true", help="the --clipnorm process with two unclipped arms: run by a copy of this "
                    "file in another commit's checkout")
    ap.add_argument("--clip-parents", default=None, metavar="BEFORE,AFTER", help="two --clip-baseline results of the parent commit into "
                    "the last visit of --out (no GPU)")
    ap.add_argument("--optimizer", choices=("sgd", "adam"), default="sgd", help="the optimizer of the --master-weights arms")
    ap.add_argument("--all-layers", action="store_true", help="the conv arm routes all seven layers, not SSD7.TRAIN_CONVS")
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    clipping = args.clipnorm is not None or args.clip_baseline
    if args.clip_parents:                                          # (arithmetic on files: no GPU)
        args.out = args.out or os.path.join(ROOT, "profiles", "optim_clip.json")
        result = clip_parents(args)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result["summary"]))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_ssd7_train_step.py needs a GPU: there is nothing to time without one")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "optim_clip.json" if clipping else
                                "ssd7_head_training.json" if args.heads else
                                "ssd7_master_weights.json" if args.master_weights else "ssd7_conv_training.json")
    if clipping or args.heads or args.master_weights:
        result = (clip_arms(torch, args) if clipping else
                  heads_arms(torch, args) if args.heads else master_weights_arms(torch, args))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
    result = {"device": torch.cuda.get_device_name(0), "model": "SSD7 300x300x3, 5 classes, bf16, train()",
              "step": "forward + SSDLoss + backward + ssd_keras_amd.optimizers.SGD, one HIP graph", "rounds": args.rounds,
              "steps_per_round": args.steps, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        images = torch.from_numpy(np.random.RandomState(100).randint(0, 256, size=(batch, 300, 300, 3)).astype(np.float32)).cuda()
        models = {arm: build(torch, arm, args.all_layers) for arm in ARMS}
        with torch.no_grad():
            n_anchor, width = models["off"].eval()(images[:1]).shape[1:]
        models["off"].train()
        y_true = torch.from_numpy(synthetic_targets(batch, n_anchor, width)).cuda()
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
