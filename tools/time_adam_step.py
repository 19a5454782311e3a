"""The optimizer step alone on SSD300's real parameter list with gradients in place (GPU box): ms per step of
  (a) ssd_keras_amd.optimizers.Adam.step() eager          (b) the same step as a HIP-graph replay
  (c) torch.optim.Adam, defaults, and fused=True where this framework build offers it
  (d) ssd_keras_amd.optimizers.SGD.step() eager, and as a graph replay
measured ALTERNATELY in rounds on one box after a warm-up (boxes of the pool differ by 15 %, a chip needs a dozen steps to reach its
clock).  Per variant: median / min / max over the rounds, the spread (max - min) / median and the launches per step.  Three modes:

    python tools/time_adam_step.py OUT.json                            the timings above (no profiler while they are taken)
    rocprofv3 --kernel-trace --stats ... -- python tools/time_adam_step.py --trace-only
                                                                       the two libssdhip optimizers alone, ONE parameter group each
                                                                       (71 tensors: one update launch per step), for the kernel trace;
                                                                       --repeat=3: the list three times (0.95 / 1.26 GB of state, far
                                                                       beyond the 256 MB Infinity Cache: neither kernel is helped by it)
    python tools/time_adam_step.py --merge-kernel-stats STATS.csv OUT.json [REPEAT]
                                                                       (no GPU) adam_step_kernel's and sgd_step_kernel's time per
                                                                       launch from that trace into OUT.json: bytes/s = algorithmic bytes
                                                                       (28 / 20 per parameter) over KERNEL time, and the two conditions
Conditions: (a) and (b) not slower than the faster form of (c) beyond the spread of the variants compared; adam_step_kernel's bytes/s not
below sgd_step_kernel's beyond the relative standard deviation of the two kernels' durations in the trace.
"""
import csv
import json
import os
import statistics
import sys

N_PARAMS = 26285486                                           # SSD300, 20 classes (asserted against the model below)


def merge_kernel_stats(stats_csv, out_json, repeat=1):
    res = json.load(open(out_json))
    rows = {}
    n_launch = {"adam_step_kernel": -(-71 * repeat // 72), "sgd_step_kernel": -(-71 * repeat // 80)}      # tensors per launch
    for r in csv.DictReader(open(stats_csv)):
        for key in ("adam_step_kernel", "sgd_step_kernel", "adam_tick_kernel"):
            if key in r["Name"]:
                rows[key] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                             "max_us": float(r["MaxNs"]) / 1e3, "rel_stddev": float(r["StdDev"]) / float(r["AverageNs"])}
    n = res["parameters"] * repeat
    for key, per_param in (("adam_step_kernel", 28), ("sgd_step_kernel", 20)):
        rows[key]["launches_per_step"] = n_launch[key]
        rows[key]["bytes_per_s"] = round(per_param * n / (rows[key]["average_us"] * n_launch[key] * 1e-6))
    if repeat != 1:                                           # the same kernels on the list repeated: footprints far beyond the L3
        rows["kernel_ratio"] = round(rows["adam_step_kernel"]["bytes_per_s"] / rows["sgd_step_kernel"]["bytes_per_s"], 4)
        res["kernels_list_x%d" % repeat] = rows
        json.dump(res, open(out_json, "w"), indent=1)
        print(json.dumps({"kernels_list_x%d" % repeat: rows}))
        return
    res["kernels"] = rows
    v = res["variants"]
    torch_best = min((k for k in v if k.startswith("c_")), key=lambda k: v[k]["ms_median"])
    ours = max(("a_adam_eager", "b_adam_graph"), key=lambda k: v[k]["ms_median"])
    tol_1 = max(v[ours]["spread"], v[torch_best]["spread"])
    tol_2 = max(rows["adam_step_kernel"]["rel_stddev"], rows["sgd_step_kernel"]["rel_stddev"])
    res["conditions"] = {
        "adam_eager_and_graph_not_slower_than_torch_adam": bool(v[ours]["ms_median"] <= v[torch_best]["ms_median"] * (1.0 + tol_1)),
        "compared": [ours, torch_best], "spread_allowed": round(tol_1, 4),
        "adam_kernel_bytes_per_s_not_below_sgd_kernel": bool(rows["adam_step_kernel"]["bytes_per_s"]
                                                             >= rows["sgd_step_kernel"]["bytes_per_s"] * (1.0 - tol_2)),
        "kernel_ratio": round(rows["adam_step_kernel"]["bytes_per_s"] / rows["sgd_step_kernel"]["bytes_per_s"], 4),
        "kernel_spread_allowed": round(tol_2, 4)}
    json.dump(res, open(out_json, "w"), indent=1)
    print(json.dumps({"kernels": rows, "conditions": res["conditions"]}))


if len(sys.argv) > 1 and sys.argv[1] == "--merge-kernel-stats":
    merge_kernel_stats(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 1)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ssd_keras_amd import synthetic as syn  # noqa: E402
from ssd_keras_amd.models.keras_ssd300 import ssd_300  # noqa: E402
from ssd_keras_amd.optimizers import SGD, Adam  # noqa: E402

TRACE_ONLY = "--trace-only" in sys.argv
REPEAT = int(next((a.split("=")[1] for a in sys.argv[1:] if a.startswith("--repeat=")), "1"))      # trace-only: the list this many times
OUT = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
ROUNDS, STEPS, WARM = 7, 50, 20
dev = torch.device("cuda:0")
cfg = syn.SSD300_VOC
torch.manual_seed(4321)
model = ssd_300((300, 300, 3), cfg["n_classes"], mode="training", l2_regularization=0.0005, scales=cfg["scales"],
                aspect_ratios_per_layer=cfg["aspect_ratios_per_layer"], steps=cfg["steps"], offsets=cfg["offsets"]).to(dev)
model = model.to(memory_format=torch.channels_last)
shapes = [(tuple(p.shape), p.is_contiguous()) for p in model.parameters()]
n_params = sum(p.numel() for p in model.parameters())
assert n_params == N_PARAMS, n_params
del model


def make_params():
    """A parameter list of SSD300's shapes and layouts of its own for every optimizer, small gradients in place."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    ps = []
    for shape, contiguous in shapes * REPEAT:
        t = torch.randn(shape, device=dev, generator=gen) * 0.05
        gr = torch.randn(shape, device=dev, generator=gen) * 1e-3
        if not contiguous:
            t, gr = t.contiguous(memory_format=torch.channels_last), gr.contiguous(memory_format=torch.channels_last)
        p = torch.nn.Parameter(t)
        p.grad = gr
        ps.append(p)
    return ps


def groups(ps):                                               # weight decay on the kernels only, as bench_extra.train_leg
    return [{"params": [p for p in ps if p.dim() > 1], "weight_decay": 1e-3}, {"params": [p for p in ps if p.dim() <= 1], "weight_decay": 0.0}]


def graphed(opt):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    torch.cuda.synchronize()
    return g.replay


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


if TRACE_ONLY:
    one_a = Adam(make_params(), lr=1e-5, epsilon=1e-8, weight_decay=1e-3).step
    one_s = SGD(make_params(), lr=1e-7, momentum=0.9, weight_decay=1e-3).step
    for _ in range(ROUNDS):                                   # alternating, as the timings
        print("adam %.4f ms  sgd %.4f ms (host-timed under the tracer: not the figures to quote)" % (timed(one_a, STEPS), timed(one_s, STEPS)), flush=True)
    sys.exit(0)

variants = {}
adam = Adam(groups(make_params()), lr=1e-5, epsilon=1e-8)
variants["a_adam_eager"] = adam.step
adam_g = Adam(groups(make_params()), lr=1e-5, epsilon=1e-8)
variants["b_adam_graph"] = graphed(adam_g)
variants["c_torch_adam_default"] = torch.optim.Adam(groups(make_params()), lr=1e-5, eps=1e-8).step
try:
    fused = torch.optim.Adam(groups(make_params()), lr=1e-5, eps=1e-8, fused=True)
    fused.step()
    variants["c_torch_adam_fused"] = fused.step
except Exception as exc:                                      # noqa: BLE001 -- this build has no fused Adam for the device
    print("torch.optim.Adam(fused=True) unavailable: %r" % (exc,), flush=True)
sgd = SGD(groups(make_params()), lr=1e-7, momentum=0.9)
variants["d_sgd_eager"] = sgd.step
sgd_g = SGD(groups(make_params()), lr=1e-7, momentum=0.9)
variants["d_sgd_graph"] = graphed(sgd_g)

for fn in variants.values():
    timed(fn, WARM)
times = {k: [] for k in variants}
for _ in range(ROUNDS):
    for k, fn in variants.items():
        times[k].append(timed(fn, STEPS))


def launches(fn):
    """Kernel launches of one step, counted by the framework's profiler (None where it records no device activity)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "mem" not in e.name.lower())
        return n or None
    except Exception:                                         # noqa: BLE001
        return None


res = {"device": torch.cuda.get_device_name(0), "parameters": n_params, "tensors": len(shapes), "rounds": ROUNDS, "steps_per_round": STEPS,
       "variants": {}}
for k, ts in times.items():
    med = statistics.median(ts)
    res["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                          "spread": round((max(ts) - min(ts)) / med, 4)}
print(json.dumps(res), flush=True)
if OUT:
    json.dump(res, open(OUT, "w"), indent=1)
for k, fn in variants.items():                                # last: the profiler must not disturb the timings above
    res["variants"][k]["launches_per_step"] = launches(fn)
res["launches_note"] = "device activities the framework's profiler records for one step; a graph replay shows one fewer than its eager form"
res["adam_iterations"] = {"eager": adam.iterations, "graph": adam_g.iterations}           # the device's counts (graph: one warm step more)
print(json.dumps(res), flush=True)
if OUT:
    json.dump(res, open(OUT, "w"), indent=1)
