"""What `ssd_keras_amd.training.fit_generator` costs per step on top of the bare replay of the captured SSD7 training step, and what its
two launches (csrc/ssdhip_fit.hip) cost against the framework's expression of the same value.  Writes profiles/fit_generator.json.

    python tools/time_fit_epoch.py [--out FILE] [--batches 8,32] [--rounds 7] [--steps 200]

(a) SSD7 300 x 300, 5 classes, bf16, `fused_blocks(True, training=True, convolutions=True, heads=True)`, SGD(master_weights=True): ms
    per step of a `--steps`-step epoch through `fit_generator` (one device batch, staged into the static buffers every step) against
    a bare replay loop of the same step without meter or penalty (tools/time_ssd7_train_step.py::graphed_step) -- in ONE process,
    alternating: the bare loop's round runs at the end of every epoch of `fit_generator`; the first epoch / 40 replays are untimed;
    median and spread (max - min) over `--rounds`.  Twice: `l2_regularization` 0 (the meter alone) and 5e-4 (the sum of squares too).
    Beside it, the staging copies alone (eager) and the two launches alone (a graph), to say where an overhead goes.
(b) the sum-of-squares + meter launches against `loss.mean() + model.l2_regularization_loss()`, each a HIP graph of its own, on SSD7's
    kernels (float32 masters) and on SSD300's (float32 parameters, 24 M values), same protocol.
A difference counts when it exceeds the sum of the two arms' spreads."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.time_ssd7_train_step import build, graphed_step, synthetic_targets, timed  # noqa: E402


def _stats(ts, digits=4):
    return {"median": round(float(np.median(ts)), digits), "spread": round(max(ts) - min(ts), digits), "rounds": [round(v, digits) for v in ts]}


def _verdict(a, b):
    """b - a and whether it exceeds the sum of the two spreads."""
    return {"difference": round(b["median"] - a["median"], 4), "margin": round(a["spread"] + b["spread"], 4),
            "exceeds_margin": bool(abs(b["median"] - a["median"]) > a["spread"] + b["spread"])}


def _graph(torch, fn):
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


def _alternate(torch, fns, rounds, replays, scale=1e3):
    """{name: stats in us} of the replays in `fns`: 40 untimed replays each, then `rounds` rounds of `replays`, alternating."""
    for fn in fns.values():
        timed(torch, fn, 40)
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(scale * timed(torch, fn, replays))
    return {name: _stats(ts, 2) for name, ts in times.items()}


def loop_arms(torch, batch, args):
    from ssd_keras_amd import training as T
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    from ssd_keras_amd.optimizers import SGD
    new = lambda: build(torch, "conv").fused_blocks(True, training=True, convolutions=True, heads=True)
    images = torch.from_numpy(np.random.RandomState(100).randint(0, 256, size=(batch, 300, 300, 3)).astype(np.float32)).cuda()
    with torch.no_grad():
        n_anchor, width = build(torch, "off").eval()(images[:1]).shape[1:]
    y_true = torch.from_numpy(synthetic_targets(batch, n_anchor, width)).cuda()
    bare = graphed_step(torch, new(), images, y_true, "sgd", True)
    timed(torch, bare, 40)
    entry = {}
    for name, l2 in (("fit", 0.0), ("fit_l2", 5e-4)):
        model = new()
        model.l2_regularization = l2
        opt = SGD(T.regularized_param_groups(model), lr=1e-5, momentum=0.9, master_weights=True)
        rounds = {"bare": [], name: []}

        class Rounds(T.Callback):
            def on_epoch_begin(self, epoch, logs=None):
                torch.cuda.synchronize()
                self.t0 = time.perf_counter()

            def on_epoch_end(self, epoch, logs=None):              # (the loop has just read the meter: the epoch's work is done)
                took = 1e3 * (time.perf_counter() - self.t0) / args.steps
                if epoch > 0:                                       # the first epoch holds the capture
                    rounds[name].append(took)
                    torch.cuda.synchronize()
                    with torch.cuda.stream(torch.cuda.default_stream()):   # (where graphed_step's other users replay it)
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            bare()
                        torch.cuda.synchronize()
                        rounds["bare"].append(1e3 * (time.perf_counter() - t0) / args.steps)

        def batches():
            while True:
                yield images, y_true

        hist = T.fit_generator(model, batches(), args.steps, args.rounds + 1, optimizer=opt, loss=SSDLoss(neg_pos_ratio=3, n_neg_min=0, alpha=1.0),
                               callbacks=[Rounds()])
        a, b = _stats(rounds["bare"]), _stats(rounds[name])
        entry[name] = {"bare_ms_per_step": a, "fit_generator_ms_per_step": b, "overhead_ms": _verdict(a, b), "last_loss": hist.history["loss"][-1]}
        del model, opt
    # where an overhead goes: the staging copies (eager, as the loop issues them) and the two launches (a graph of their own)
    model = new()
    model.l2_regularization = 5e-4
    stage_img, stage_y = torch.empty_like(images), torch.empty_like(y_true)

    def staging():
        stage_img.copy_(images, non_blocking=True)
        stage_y.copy_(y_true, non_blocking=True)

    entry["staging_copies_us"] = _alternate(torch, {"copies": staging}, args.rounds, args.steps)["copies"]
    entry["launches_us"] = launch_arms(torch, model, [w.detach().float() for w in T._conv_kernels(model)], batch, args)
    return entry


def launch_arms(torch, model, kernels, batch, args):
    """The sum-of-squares + meter launches against loss.mean() + l2 * sum(w^2) in framework operations over the same float32 tensors."""
    from ssd_keras_amd import _native as nat
    l2 = 5e-4
    loss = torch.rand((batch,), device="cuda") * 10
    flat = [k.as_strided((k.numel(),), (1,)) for k in kernels]
    table = nat.sumsq_table(flat, loss.device)
    partials = torch.zeros((table[5],), dtype=torch.float32, device="cuda")
    block = torch.zeros((nat.fit_meter_state_bytes(),), dtype=torch.uint8, device="cuda")
    nat.fit_meter_reset(block)

    def own():
        nat.sumsq_partials(table, partials)
        nat.fit_meter_update(block, loss, partials, l2)

    def meter_only():
        nat.fit_meter_update(block, loss, None, 0.0)

    def framework():
        return loss.mean() + l2 * sum((k ** 2).sum() for k in kernels)

    got = _alternate(torch, {"framework": _graph(torch, framework), "libssdhip": _graph(torch, own), "meter_only": _graph(torch, meter_only)},
                     args.rounds, args.steps)
    got["tensors"], got["values"], got["partials"] = len(kernels), int(sum(k.numel() for k in kernels)), int(table[5])
    got["libssdhip_minus_framework"] = _verdict(got["framework"], got["libssdhip"])
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_generator.json"))
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_fit_epoch.py needs a GPU: there is nothing to time without one")
    result = {"device": torch.cuda.get_device_name(0), "model": "SSD7 300x300x3, 5 classes, bf16, train(), fused_blocks(True, training=True, "
              "convolutions=True, heads=True), SGD(master_weights=True)", "rounds": args.rounds, "steps_per_round": args.steps, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        result["batches"][str(batch)] = loop_arms(torch, batch, args)
        print(json.dumps({"batch": batch, **result["batches"][str(batch)]}), flush=True)
        torch.cuda.empty_cache()
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.models.keras_ssd300 import ssd_300
    cfg = syn.SSD300_VOC
    model = ssd_300((300, 300, 3), cfg["n_classes"], mode="training", l2_regularization=0.0005, scales=cfg["scales"],
                    aspect_ratios_per_layer=cfg["aspect_ratios_per_layer"], steps=cfg["steps"], offsets=cfg["offsets"]).cuda()
    from ssd_keras_amd.training import _conv_kernels
    result["ssd300_launches_us"] = launch_arms(torch, model, [w.detach() for w in _conv_kernels(model)], 32, args)
    print(json.dumps({"ssd300_launches_us": result["ssd300_launches_us"]}), flush=True)
    result["note"] = ("ms per step on the host's clock between the synchronised start of an epoch and the meter's read at its end; bare: the "
                      "same count of replays of the captured step without meter, penalty or staging.  exceeds_margin: the medians differ by "
                      "more than the sum of the two arms' spreads.  Step time is the only claim; convergence is not measured.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
