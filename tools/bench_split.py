#!/usr/bin/env python
"""Measures Table.random_split([0.9, 0.1], 0) over the table tools/bench_schema.py builds (three
string columns, 4e6 rows by default) and prints ONE JSON line: rows/s, input + output bytes per
second against the 8 TB/s HBM peak, and the device stages' times from HIP events (split = the
dq_split_rows launch and its count read-back; select = the index plans of both splits; gather =
every column of both splits).  The split is checked against the host restatement's counts.

    python tools/bench_split.py [--rows 4000000] [--steps 5] [--warmup 2]
"""
import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_BYTES_PER_S = 8e12
WEIGHTS, SEED = [0.9, 0.1], 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    import split_host as S
    from bench_schema import synth
    from deequ_amd.table import Table
    data = Table.from_arrow(synth(args.rows), device="cuda:0")

    def table_bytes(t):
        return sum(c.nbytes() for b in t.batches for c in b.values())

    events = []

    @contextlib.contextmanager
    def timer(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        events.append((name, a, b))

    stages, wall = {}, []
    for step in range(args.warmup + args.steps):
        events.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parts = data.random_split(WEIGHTS, SEED, stage_timer=timer)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if step >= args.warmup:
            wall.append(dt)
            per = {}
            for name, a, b in events:
                per[name] = per.get(name, 0.0) + a.elapsed_time(b)
            for name, ms in per.items():
                stages.setdefault(name + "_ms", []).append(ms)
    wall.sort()
    med = wall[len(wall) // 2]
    moved = table_bytes(data) + sum(table_bytes(t) for t in parts)
    a = S.assign(SEED, 0, args.rows, WEIGHTS)
    assert [t.num_rows for t in parts] == [int((a == k).sum()) for k in range(len(WEIGHTS))]

    def med_of(v):
        v = sorted(v)
        return round(v[len(v) // 2], 4)
    print(json.dumps({
        "workload": "random_split_0.9_0.1", "rows": args.rows, "steps": args.steps,
        "warmup": args.warmup, "split_rows": [t.num_rows for t in parts],
        "split_ms_median": round(med * 1e3, 3), "split_ms_min": round(wall[0] * 1e3, 3),
        "rows_per_s": round(args.rows / med), "bytes_in_plus_out": moved,
        "bytes_per_s": round(moved / med), "frac_of_8TBps": round(moved / med / PEAK_BYTES_PER_S, 5),
        "stage_ms_median_hip_events": {n: med_of(v) for n, v in stages.items()},
    }))


if __name__ == "__main__":
    main()
