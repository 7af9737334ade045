#!/usr/bin/env python
"""Measures RowLevelSchemaValidator.validate with the reference's integration-test schema (int id
not nullable, string name with max_length 10, timestamp event_time) over synthetic string columns
and prints ONE JSON line: rows/s, input + output bytes per second against the 8 TB/s HBM peak, the
device stages' times from HIP events (evaluate = the per-column evaluate launches and the verdict;
select = the three-phase index plan of both outputs; gather = every column of both outputs), and
the plain-Python restatement's rate on a bounded sample.

    python tools/bench_schema.py [--rows 4000000] [--steps 5] [--warmup 2]
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

PEAK_BYTES_PER_S = 8e12
MASK = "yyyy-MM-dd HH:mm:ss"


def synth(rows, seed=3):
    """id: decimal integers, 5% "N/A", 3% NULL; name: "Product <k>" of 9-17 characters (a third
    over max_length 10); event_time: timestamps in strict form, 4% NULL, 3% "yesterday morning"."""
    import numpy as np
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 10**6, rows).astype(str).astype(object)
    u = rng.random(rows)
    ids[u < 0.05] = "N/A"
    ids[(u >= 0.05) & (u < 0.08)] = None
    names = np.char.add("Product ", rng.integers(0, 10**rng.integers(1, 10, rows)).astype(str))
    sec = np.datetime64("1990-01-01", "s") + rng.integers(0, 86400 * 365 * 40, rows).astype("timedelta64[s]")
    ts = np.char.replace(np.datetime_as_string(sec, unit="s"), "T", " ").astype(object)
    u = rng.random(rows)
    ts[u < 0.04] = None
    ts[(u >= 0.04) & (u < 0.07)] = "yesterday morning"
    return pa.table({"id": pa.array(ids, pa.string()), "name": pa.array(names, pa.string()),
                     "event_time": pa.array(ts, pa.string())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-sample", type=int, default=20_000)
    args = ap.parse_args()

    import torch

    import schema_host as H
    from deequ_amd import RowLevelSchema, RowLevelSchemaValidator
    from deequ_amd.table import Table
    arrow = synth(args.rows)
    data = Table.from_arrow(arrow, device="cuda:0")
    schema = (RowLevelSchema().with_int_column("id", is_nullable=False)
              .with_string_column("name", max_length=10).with_timestamp_column("event_time", mask=MASK))

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
        res = RowLevelSchemaValidator.validate(data, schema, stage_timer=timer)
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
    moved = table_bytes(data) + table_bytes(res.valid_rows) + table_bytes(res.invalid_rows)

    # the restatement on a bounded sample, one core
    k = min(args.host_sample, args.rows)
    sample = {c: arrow.column(c).slice(0, k).to_pylist() for c in arrow.column_names}
    hs = [{"kind": "int", "name": "id", "is_nullable": False},
          {"kind": "string", "name": "name", "max_length": 10},
          {"kind": "timestamp", "name": "event_time", "mask": MASK}]
    t0 = time.perf_counter()
    hv, hi = H.validate(hs, sample)
    host_dt = time.perf_counter() - t0
    small = RowLevelSchemaValidator.validate(Table.from_arrow(arrow.slice(0, k), device="cuda:0"), schema)
    assert (small.num_valid_rows, small.num_invalid_rows) == (len(hv["id"]), len(hi["id"]))

    def med_of(v):
        v = sorted(v)
        return round(v[len(v) // 2], 4)
    print(json.dumps({
        "workload": "row_level_schema_integration", "rows": args.rows, "steps": args.steps,
        "warmup": args.warmup, "valid_rows": res.num_valid_rows, "invalid_rows": res.num_invalid_rows,
        "validate_ms_median": round(med * 1e3, 3), "validate_ms_min": round(wall[0] * 1e3, 3),
        "rows_per_s": round(args.rows / med), "bytes_in_plus_out": moved,
        "bytes_per_s": round(moved / med), "frac_of_8TBps": round(moved / med / PEAK_BYTES_PER_S, 5),
        "stage_ms_median_hip_events": {n: med_of(v) for n, v in stages.items() if n.endswith("_ms")},
        "host_restatement_rows_per_s": round(k / host_dt), "host_sample_rows": k, "host_cores": 1,
    }))


if __name__ == "__main__":
    main()
