"""The SGD step alone on SSD300's real parameter list with gradients in place (GPU box): ms per step of
  (a) ssd_keras_amd.optimizers.SGD.step() eager               (b) the same step as a HIP-graph replay
  (c) the legacy export ssdhip_sgd_momentum_step driven directly on the same two group tables, eager and replayed: the step
      without the state block (its learning rate in the kernel arguments) and without the optimizer's Python
  (d) torch.optim.SGD                                         (e) rule='keras' with Nesterov, replayed
measured ALTERNATELY in rounds on one box after a warm-up (boxes of the pool differ by 15 %, a chip needs a dozen steps to reach its
clock).  Per variant: median / min / max over the rounds and the spread (max - min) / median.  Modes:

    python tools/time_sgd_step.py OUT.json [--tree=DIR]             the timings above; --tree: import the package from another checkout
                                                                    (a parent commit without the state block: (e) is then skipped),
                                                                    so that two commits can be run alternately from one script
    rocprofv3 --kernel-trace --stats ... -- python tools/time_sgd_step.py --trace-only
                                                                    ONE parameter group (71 tensors: one update launch per step), per
                                                                    round 50 launches of sgd_momentum_kernel (the legacy export), then
                                                                    50 steps of SGD (sgd_tick_kernel + sgd_step_kernel<0, false>)
    python tools/time_sgd_step.py --merge-kernel-trace KERNEL_TRACE.csv OUT.json
                                                                    (no GPU) the two kernels' time per launch and per round from that
                                                                    trace into OUT.json, and the condition below
Condition: sgd_step_kernel<0, false> not slower than sgd_momentum_kernel beyond the spread (max - min) / median that
sgd_momentum_kernel's own per-round means show in that trace; both move 20 bytes per parameter.
"""
import csv
import json
import os
import statistics
import sys

N_PARAMS = 26285486                                           # SSD300, 20 classes (asserted against the model below)
ROUNDS, STEPS, WARM = 7, 50, 20


def merge_kernel_trace(trace_csv, out_json):
    res = json.load(open(out_json)) if os.path.exists(out_json) else {"parameters": N_PARAMS}
    runs = {"sgd_momentum_kernel": [], "sgd_step_kernel": [], "sgd_tick_kernel": []}
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for key in runs:
            if key in r["Kernel_Name"]:
                runs[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for key, us in runs.items():
        us = us[-ROUNDS * STEPS:]                             # the warm-up launches come first
        per_round = [statistics.mean(us[k * STEPS:(k + 1) * STEPS]) for k in range(len(us) // STEPS)]
        med = statistics.median(per_round)
        out[key] = {"launches": len(us), "us_median_of_rounds": round(med, 3), "us_rounds": [round(v, 3) for v in per_round],
                    "spread": round((max(per_round) - min(per_round)) / med, 4)}
        if key != "sgd_tick_kernel":
            out[key]["bytes_per_s"] = round(20 * res["parameters"] / (med * 1e-6))
    old, new = out["sgd_momentum_kernel"], out["sgd_step_kernel"]
    ratio = new["us_median_of_rounds"] / old["us_median_of_rounds"]
    res["kernels"] = out
    res["kernel_condition"] = {"time_ratio_new_over_legacy": round(ratio, 4), "legacy_spread_allowed": old["spread"],
                               "new_not_slower_than_legacy_beyond_its_spread": bool(ratio <= 1.0 + old["spread"])}
    json.dump(res, open(out_json, "w"), indent=1)
    print(json.dumps({"kernels": out, "kernel_condition": res["kernel_condition"]}))


if len(sys.argv) > 1 and sys.argv[1] == "--merge-kernel-trace":
    merge_kernel_trace(sys.argv[2], sys.argv[3])
    sys.exit(0)

TREE = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--tree=")), None)
sys.path.insert(0, os.path.abspath(TREE) if TREE else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ssd_keras_amd import _native as nat  # noqa: E402
from ssd_keras_amd import synthetic as syn  # noqa: E402
from ssd_keras_amd.models.keras_ssd300 import ssd_300  # noqa: E402
from ssd_keras_amd.optimizers import SGD, _bump_versions  # noqa: E402

TRACE_ONLY = "--trace-only" in sys.argv
OUT = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
HAS_BLOCK = hasattr(SGD, "set_lr")
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
    for shape, contiguous in shapes:
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


_flat = lambda t: t.detach().as_strided((t.numel(),), (1,))


def legacy(grps):
    """The step of the legacy export over parameter groups: one launch per group, the versions bumped as the optimizer does."""
    keep, calls = [], []
    for g in grps:
        ps = g["params"]
        bufs = [torch.zeros_like(p, memory_format=torch.preserve_format) for p in ps]
        keep.append(bufs)
        calls.append((nat.sgd_table([_flat(p) for p in ps], [_flat(p.grad) for p in ps], [_flat(b) for b in bufs], dev), g["weight_decay"], tuple(ps)))

    def step(_keep=keep):
        for table, wd, ps in calls:
            nat.sgd_momentum_step(table, 1e-7, 0.9, wd)
            _bump_versions(ps)
    return step


def graphed(step):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
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
    one_old = legacy([{"params": make_params(), "weight_decay": 1e-3}])
    one_new = SGD(make_params(), lr=1e-7, momentum=0.9, weight_decay=1e-3).step
    timed(one_old, WARM)
    timed(one_new, WARM)
    for _ in range(ROUNDS):                                   # alternating, as the timings
        print("legacy %.4f ms  state block %.4f ms (host-timed under the tracer: not the figures to quote)" % (
            timed(one_old, STEPS), timed(one_new, STEPS)), flush=True)
    sys.exit(0)

variants = {}
sgd = SGD(groups(make_params()), lr=1e-7, momentum=0.9)
variants["a_sgd_eager"] = sgd.step
sgd_g = SGD(groups(make_params()), lr=1e-7, momentum=0.9)
variants["b_sgd_graph"] = graphed(sgd_g.step)
variants["c_legacy_export_eager"] = legacy(groups(make_params()))
variants["c_legacy_export_graph"] = graphed(legacy(groups(make_params())))
variants["d_torch_sgd"] = torch.optim.SGD(groups(make_params()), lr=1e-7, momentum=0.9).step
if HAS_BLOCK:
    variants["e_sgd_keras_nesterov_graph"] = graphed(SGD(groups(make_params()), lr=1e-7, momentum=0.9, nesterov=True, rule="keras").step)

for fn in variants.values():
    timed(fn, WARM)
times = {k: [] for k in variants}
for _ in range(ROUNDS):
    for k, fn in variants.items():
        times[k].append(timed(fn, STEPS))

res = {"device": torch.cuda.get_device_name(0), "tree": TREE or ".", "state_block": HAS_BLOCK, "parameters": n_params, "tensors": len(shapes),
       "rounds": ROUNDS, "steps_per_round": STEPS, "variants": {}}
for k, ts in times.items():
    med = statistics.median(ts)
    res["variants"][k] = {"ms_median": round(med, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                          "spread": round((max(ts) - min(ts)) / med, 4)}
if HAS_BLOCK:
    res["sgd_iterations"] = {"eager": sgd.iterations, "graph": sgd_g.iterations}              # the device's counts
print(json.dumps(res), flush=True)
if OUT:
    json.dump(res, open(OUT, "w"), indent=1)
