"""Durations of the decode launches in a rocprofv3 kernel trace (`*_kernel_trace.csv`): per kernel the number of launches and the
fastest, median, mean, 95th-percentile and slowest launch in microseconds.  tools/time_decode.py times the decode of an ASSEMBLED
tensor stage by stage (`stages=` masks); the step itself decodes from the head outputs, and its scan kernel
(`scan_heads_rows_kernel<21>`, or `scan_heads_kernel` with SSDHIP_SCAN_ROWS=lds) runs nowhere else -- this reads it out of a trace
of the bench command, every launch of the run (eager warm-ups, graph replays, the eager steps behind them):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python bench.py --gpus 1 --steps 20 --warmup 5
    python tools/decode_kernel_durations.py DIR/.../run_kernel_trace.csv OUT.json

Two builds are compared on ONE box, each traced in a run of its own (profiles/scanrows_ab_*_decode_kernel_durations.json)."""
import csv
import json
import sys

NAMES = ("scan_heads", "scan_kernel", "scan_wide", "zero_words", "nms_kernel", "topk_kernel")


def main(trace, out):
    by = {}
    with open(trace) as f:
        for r in csv.DictReader(f):
            k = r["Kernel_Name"]
            if any(n in k for n in NAMES):
                by.setdefault(k.replace("void ", "")[:90], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = {}
    for k, d in sorted(by.items()):
        d = sorted(d)
        res[k] = {"launches": len(d), "min_us": round(d[0], 2), "median_us": round(d[len(d) // 2], 2), "mean_us": round(sum(d) / len(d), 2),
                  "p95_us": round(d[int(0.95 * (len(d) - 1))], 2), "max_us": round(d[-1], 2)}
        print("%-92s %s" % (k, res[k]))
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
