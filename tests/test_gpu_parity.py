"""GPU parity against the ORACLE on seeded random tables: every scan aggregation, null rates
0 / 5 / 100 %, where filters, multi-batch tables, and the synthetic Item table (device generator
vs the numpy restatement).  Bar: bit-exact for counts / Long sums / min / max / HLL registers /
frequency counts; 1e-12 relative for fp64 moments (north_star)."""
import math

import numpy as np
import pyarrow as pa
import pytest

pytestmark = pytest.mark.gpu

REL = 1e-12


def rel_close(a, b, rel=REL):
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b or abs(a - b) <= rel * max(abs(a), abs(b))


def random_table(n, seed, null_rate):
    rng = np.random.default_rng(seed)
    def mask():
        return rng.random(n) < null_rate
    i64 = rng.integers(-10 ** 6, 10 ** 6, n)
    f64 = rng.normal(1000.0, 250.0, n)
    i32 = rng.integers(-50, 50, n).astype(np.int32)
    cats = np.array(["high", "low", "medium", "", "NullValue", "x" * 20])
    s = cats[rng.integers(0, len(cats), n)]
    return pa.table({
        "a": pa.array(i64, mask=mask(), type=pa.int64()),
        "b": pa.array(f64, mask=mask(), type=pa.float64()),
        "c": pa.array(i32, mask=mask(), type=pa.int32()),
        "s": pa.array([None if m else v for v, m in zip(s, mask())], type=pa.string()),
    })


def oracle_of(t):
    from oracle.deequ_oracle import OTable
    types = {"a": "long", "b": "double", "c": "int", "s": "string"}
    return OTable({k: t.column(k).to_pylist() for k in t.column_names}, types)


@pytest.mark.parametrize("n,null_rate,batch", [(1, 0.0, None), (1000, 0.0, None),
                                               (4097, 0.05, None), (50_000, 0.05, 8192),
                                               (70_000, 1.0, None), (20_011, 0.3, 4096)])
def test_scan_suite_matches_oracle(n, null_rate, batch, gpu_device):
    from deequ_amd import Analysis, Table
    from deequ_amd.analyzers import (ApproxCountDistinct, Completeness, Compliance, Correlation,
                                     Maximum, Mean, Minimum, Size, StandardDeviation, Sum)
    from oracle import deequ_oracle as O
    t = random_table(n, n, null_rate)
    df = Table.from_arrow(t, device=gpu_device, max_batch_rows=batch)
    ot = oracle_of(t)
    where = "c > -20"
    suite = [Size(), Size(where), Completeness("a"), Completeness("s", where),
             Compliance("nn", "a >= 0"), Compliance("in", "s IS NULL OR s IN ('high','low')"),
             Compliance("rng", "b IS NULL OR (b >= 900.0 AND b <= 1100.0)"),
             Compliance("w", "c < 10", where), Compliance("x", "a > c"),
             Sum("a"), Sum("b"), Sum("c", where), Mean("a"), Mean("b", where),
             Minimum("a"), Maximum("a"), Minimum("b"), Maximum("c", where),
             StandardDeviation("a"), StandardDeviation("b"), StandardDeviation("c", where),
             Correlation("a", "b"), Correlation("c", "b", where),
             ApproxCountDistinct("a"), ApproxCountDistinct("s"), ApproxCountDistinct("b", where)]
    ctx = Analysis(suite).run(df)

    def state(a):
        return a.from_aggregation_result(_row(df, a), 0)

    # counts and Long sums: bit-exact
    assert ctx.metric(Size()).value.get() == n
    exp = O.agg_conditional_count(ot, where)
    st = _state_of(df, Size(where))
    assert (None if st is None else st.num_matches) == exp
    assert _state_of(df, Completeness("a")).num_matches == O.agg_sum_notnull(ot, "a", None)
    for name, pred, w in [("nn", "a >= 0", None), ("in", "s IS NULL OR s IN ('high','low')", None),
                          ("rng", "b IS NULL OR (b >= 900.0 AND b <= 1100.0)", None),
                          ("w", "c < 10", where), ("x", "a > c", None)]:
        st = _state_of(df, Compliance(name, pred, w))
        exp = O.agg_compliance(ot, pred, w)
        assert (st.num_matches if st else None) == exp, name
    for col, w in [("a", None), ("c", where)]:
        st = _state_of(df, Sum(col, w))
        exp = O.agg_sum(ot, col, w)
        assert (None if st is None else st.sum_value) == exp
    st = _state_of(df, Sum("b"))
    exp = O.agg_sum(ot, "b", None)
    assert (st is None and exp is None) or rel_close(st.sum_value, exp)
    for a, fn in [(Minimum("a"), O.agg_min), (Maximum("a"), O.agg_max), (Minimum("b"), O.agg_min)]:
        st = _state_of(df, a)
        exp = fn(ot, a.column, a.where)
        assert (None if st is None else (st.min_value if hasattr(st, "min_value") else st.max_value)) == exp
    # fp64 moments: 1e-12 relative
    for col, w in [("a", None), ("b", None), ("c", where)]:
        st = _state_of(df, StandardDeviation(col, w))
        n_, avg, m2 = O.agg_stddev(ot, col, w)
        if n_ == 0:
            assert st is None
        else:
            assert st.n == n_ and rel_close(st.avg, avg) and rel_close(st.m2, m2)
            assert rel_close(st.metric_value(), math.sqrt(m2 / n_))
    for x, y, w in [("a", "b", None), ("c", "b", where)]:
        st = _state_of(df, Correlation(x, y, w))
        exp = O.agg_corr(ot, x, y, w)
        if exp[0] == 0:
            assert st is None
        else:
            assert st.n == exp[0]
            got = st.metric_value()
            ref = exp[3] / math.sqrt(exp[4] * exp[5]) if exp[4] * exp[5] > 0 else float("nan")
            assert rel_close(got, ref)
    # HLL registers: bit-exact
    for col, w in [("a", None), ("s", None), ("b", where)]:
        st = _state_of(df, ApproxCountDistinct(col, w))
        assert list(st.words) == O.agg_hll(ot, col, w), col


def _row(df, analyzer):
    from deequ_amd.runners.engine import run_scan
    return run_scan(df, analyzer.aggregation_functions())


def _state_of(df, analyzer):
    return analyzer.from_aggregation_result(_row(df, analyzer), 0)


@pytest.mark.parametrize("n,batch", [(100_000, 1 << 14), (300_001, None)])
def test_synthetic_item_table_device_equals_numpy(n, batch, gpu_device):
    import torch
    from deequ_amd.synth import item_columns_numpy, item_table_device
    df = item_table_device(n, seed=11, batch_rows=batch or (1 << 26), device=gpu_device)
    ref = item_columns_numpy(n, seed=11)
    ids, vw = [], []
    valid = {"id": [], "numViews": []}
    prio, names = [], []
    for b in df.batches:
        m = b["id"].length
        ids.append(b["id"].values[:m].cpu().numpy())
        vw.append(b["numViews"].values[:m].cpu().numpy())
        for c in ("id", "numViews"):
            bits = np.unpackbits(b[c].validity.cpu().numpy(), bitorder="little")[:m]
            valid[c].append(bits.astype(bool))
        for c, out in (("priority", prio), ("name", names)):
            off = b[c].values[: m + 1].cpu().numpy()
            data = b[c].data.cpu().numpy().tobytes()
            bits = np.unpackbits(b[c].validity.cpu().numpy(), bitorder="little")[:m]
            out.extend(data[off[i]:off[i + 1]].decode() if bits[i] else None for i in range(m))
    assert np.array_equal(np.concatenate(valid["id"]), ref["id_valid"])
    assert np.array_equal(np.concatenate(ids), ref["id"])
    assert np.array_equal(np.concatenate(valid["numViews"]), ref["numViews_valid"])
    assert np.array_equal(np.concatenate(vw), ref["numViews"])
    assert prio == ref["priority"]
    assert names == ref["name"]


def test_s10_on_synthetic_items_matches_c_oracle(gpu_device):
    """S10 on 2^22 + 12345 synthetic rows in 3 batches vs the C oracle (Spark local[16])."""
    from deequ_amd import Analysis
    from deequ_amd.analyzers import (Completeness, Compliance, Maximum, Mean, Minimum, Size,
                                     StandardDeviation, Sum)
    from deequ_amd.synth import item_table_device
    from oracle import c_oracle as C
    n = (1 << 22) + 12345
    df = item_table_device(n, seed=3, batch_rows=1 << 21, device=gpu_device)
    suite = s10_suite()
    ctx = Analysis(suite).run(df)
    # oracle over the same device buffers copied to the host, batch by batch
    num = None
    comp_id = comp_name = 0
    pt = pn = 0
    parts = []
    for b in df.batches:
        m = b["id"].length
        v = b["numViews"].values[:m].cpu().numpy()
        vb = b["numViews"].validity.cpu().numpy()
        parts.append(C.numeric_i64(v, vb, op=17, lit=0, threads=16))
        comp_id += C.validity_count(b["id"].validity.cpu().numpy(), m, 16)
        comp_name += C.validity_count(b["name"].validity.cpu().numpy(), m, 16)
        t, nn = C.str_in(b["priority"].values.cpu().numpy(), b["priority"].data.cpu().numpy(),
                         b["priority"].validity.cpu().numpy(), m, ["high", "low"], True, 16)
        pt += t
        pn += nn
    cnt = sum(p.count for p in parts)
    s = sum(p.sum_long for p in parts)
    assert ctx.metric(Size()).value.get() == n
    assert ctx.metric(Completeness("id")).value.get() == comp_id / n
    assert ctx.metric(Completeness("name")).value.get() == comp_name / n
    assert ctx.metric(suite[3]).value.get() == sum(p.pred_true for p in parts) / n
    assert ctx.metric(suite[4]).value.get() == pt / n
    assert ctx.metric(Sum("numViews")).value.get() == float(s)
    assert ctx.metric(Mean("numViews")).value.get() == float(s) / n
    assert ctx.metric(Minimum("numViews")).value.get() == float(min(p.min for p in parts))
    assert ctx.metric(Maximum("numViews")).value.get() == float(max(p.max for p in parts))
    # merge the per-batch Welford states like Spark partitions
    from oracle.deequ_oracle import moments_merge
    st = (0.0, 0.0, 0.0)
    for p in parts:
        st = moments_merge(st, (p.n, p.avg, p.m2))
    assert rel_close(ctx.metric(StandardDeviation("numViews")).value.get(),
                     math.sqrt(st[2] / st[0]))


def s10_suite():
    from deequ_amd.analyzers import (Completeness, Compliance, Maximum, Mean, Minimum, Size,
                                     StandardDeviation, Sum)
    return [Size(), Completeness("id"), Completeness("name"),
            Compliance("numViews is Fnon-negative", "numViews >= 0"),
            Compliance("priority contained in high,low",
                       "priority IS NULL OR priority IN ('high','low')"),
            Sum("numViews"), Mean("numViews"), StandardDeviation("numViews"),
            Minimum("numViews"), Maximum("numViews")]


@pytest.mark.parametrize("n,null_rate,batch", [(1000, 0.0, None), (50_000, 0.05, 8192),
                                               (70_001, 0.3, None)])
def test_fused_hll_and_comoments_match_oracle(n, null_rate, batch, gpu_device):
    """ApproxCountDistinct(x) beside Correlation(x, y) (BASELINE.json configs[3]) runs as ONE pass
    (BC_CORR_HLL): the HLL registers must equal the oracle's bit for bit, with the HLL column as
    either side of the correlation, NaNs in the hashed doubles, NULLs, where filters and row
    counts off the 1024-row vector chunk."""
    from deequ_amd.analyzers import ApproxCountDistinct, Correlation
    from deequ_amd.runners.engine import get_plan, run_scan
    from deequ_amd.table import Table
    from oracle import deequ_oracle as O
    t = random_table(n, n + 7, null_rate)
    vals = t.column("b").to_pylist()
    nulls = np.array([v is None for v in vals])
    b = np.array([0.0 if v is None else v for v in vals])
    b[::97] = np.nan                                       # NaN payloads hash as the canonical NaN
    b[1::97] = np.frombuffer(np.uint64(0x7ff0000000000123).tobytes(), np.float64)[0]
    t = t.set_column(1, "b", pa.array(b, mask=nulls, type=pa.float64()))
    df = Table.from_arrow(t, device=gpu_device, max_batch_rows=batch)
    ot = oracle_of(t)
    where = "c > -20"
    cases = [(ApproxCountDistinct("a"), Correlation("a", "b")),
             (ApproxCountDistinct("b"), Correlation("a", "b")),
             (ApproxCountDistinct("a", where), Correlation("b", "a", where))]
    for hll, corr in cases:
        aggs = hll.aggregation_functions() + corr.aggregation_functions()
        explain = get_plan(df.schema, aggs).explain()
        assert "+hll[" in explain, explain                 # the plan did fuse the two
        row = run_scan(df, aggs)
        st = hll.from_aggregation_result(row, 0)
        assert list(st.words) == O.agg_hll(ot, hll.column, hll.where), str(hll)
        cst = corr.from_aggregation_result(row, len(hll.aggregation_functions()))
        exp = O.agg_corr(ot, corr.first_column, corr.second_column, corr.where)
        if exp[0] == 0:
            assert cst is None
        else:
            assert cst.n == exp[0]
            ref = exp[3] / math.sqrt(exp[4] * exp[5]) if exp[4] * exp[5] > 0 else float("nan")
            assert rel_close(cst.metric_value(), ref)


@pytest.mark.parametrize("n,batch", [(5_000, None), (40_000, 6_000)])
def test_hll_strings_of_every_length_match_oracle(n, batch, gpu_device):
    """TK_HLL over utf8: strings of 0..100 bytes (the register path takes <= 64, longer ones
    xxh_bytes' loop), multibyte characters, NULLs and a where filter; registers bit-exact."""
    from deequ_amd import Table
    from deequ_amd.analyzers import ApproxCountDistinct
    from oracle import deequ_oracle as O
    rng = np.random.default_rng(n)
    alphabet = list("abcXYZ019 _-") + ["é", "ß", "€", "漢"]
    vals = []
    for i in range(n):
        if rng.random() < 0.05:
            vals.append(None)
            continue
        target = int(rng.integers(0, 101))
        s = ""
        while len(s.encode()) < target:
            s += alphabet[int(rng.integers(0, len(alphabet)))]
        vals.append(s)
    ks = rng.integers(0, 3, n).astype(np.int32)
    t = pa.table({"s": pa.array(vals, type=pa.string()), "k": pa.array(ks, type=pa.int32())})
    df = Table.from_arrow(t, device=gpu_device, max_batch_rows=batch)
    ot = O.OTable({"s": vals, "k": ks.tolist()}, {"s": "string", "k": "int"})
    for w in (None, "k > 0"):
        st = _state_of(df, ApproxCountDistinct("s", w))
        assert list(st.words) == O.agg_hll(ot, "s", w), w


from moment_cases import exact_moments as _exact_moments  # noqa: E402  (moved; the name stays)


@pytest.mark.parametrize("n,null_rate,batch,rho", [(4097, 0.05, None, 0.0), (20_011, 0.3, 4096, 0.0),
                                                   (30_000, 0.05, 7000, 0.8), (9_000, 0.0, None, -0.99)])
def test_moments_against_exact_arithmetic(n, null_rate, batch, rho, gpu_device):
    """Mean / StdDev / Correlation states against EXACT rational arithmetic of the same formulas.
    Bound: every state component within 1e-12 of its scale -- the averages over
    Σ|x|/n, the co-moment ck over Σ|dx·dy|, the second moments (sums of squares) relative -- for
    the device AND for the oracle's row-sequential Spark update, so the two are within 2e-12 of
    each other on that scale.  The correlation metric is then within 1e-12 relative whenever
    |corr| >= 1e-3 · Σ|dx·dy| / sqrt(xMk·yMk) (for these independent columns, |corr| ~ 1e-3 and the
    metric still meets 1e-12 relative: measured 3e-15 device, 5e-14 oracle)."""
    from fractions import Fraction as F
    from deequ_amd import Table
    from deequ_amd.analyzers import Correlation, StandardDeviation
    from deequ_amd.runners.engine import run_scan
    from oracle import deequ_oracle as O
    t = random_table(n, n + 17, null_rate)
    if rho:  # a column correlated with b (well-conditioned ck)
        rng = np.random.default_rng(n)
        b = t.column("b").to_numpy(zero_copy_only=False)
        d = rho * (b - 1000.0) + math.sqrt(1 - rho * rho) * rng.normal(0.0, 250.0, n)
        t = t.append_column("d", pa.array(d, mask=np.asarray(t.column("b").is_null())))
    df = Table.from_arrow(t, device=gpu_device, max_batch_rows=batch)
    ot = oracle_of(t)
    if rho:
        ot.types["d"] = "double"
    pairs = [("a", "b", None), ("c", "b", "c > -20")] + ([("d", "b", None)] if rho else [])
    for cx, cy, w in pairs:
        a = Correlation(cx, cy, w)
        st = a.from_aggregation_result(run_scan(df, a.aggregation_functions()), 0)
        sel = [(float(x), float(y)) for x, y in zip(O._sel(ot, cx, w), O._sel(ot, cy, w))
               if x is not None and y is not None]
        e = _exact_moments([x for x, _ in sel], [y for _, y in sel])
        orc = O.agg_corr(ot, cx, cy, w)
        ex_corr = float(e["ck"]) / math.sqrt(float(e["xm"]) * float(e["ym"]))
        for who, s in (("device", (st.n, st.x_avg, st.y_avg, st.ck, st.x_mk, st.y_mk)), ("oracle", orc)):
            assert s[0] == e["n"], who
            assert abs(F(s[1]) - e["mx"]) <= F(1, 10 ** 12) * e["sx"], (who, "xAvg")
            assert abs(F(s[2]) - e["my"]) <= F(1, 10 ** 12) * e["sy"], (who, "yAvg")
            assert abs(F(s[3]) - e["ck"]) <= F(1, 10 ** 12) * e["sck"], (who, "ck")
            assert abs(F(s[4]) - e["xm"]) <= F(1, 10 ** 12) * e["xm"], (who, "xMk")
            assert abs(F(s[5]) - e["ym"]) <= F(1, 10 ** 12) * e["ym"], (who, "yMk")
            corr = s[3] / math.sqrt(s[4] * s[5])
            assert rel_close(corr, ex_corr), (who, corr, ex_corr)
        assert rel_close(st.metric_value(), orc[3] / math.sqrt(orc[4] * orc[5]))
    for col, w in [("a", None), ("b", None), ("c", "c > -20")]:
        sd = StandardDeviation(col, w)
        st = sd.from_aggregation_result(run_scan(df, sd.aggregation_functions()), 0)
        xs = [float(v) for v in O._sel(ot, col, w) if v is not None]
        e = _exact_moments(xs, xs)
        assert st.n == e["n"]
        assert abs(F(st.avg) - e["mx"]) <= F(1, 10 ** 12) * e["sx"], col
        assert abs(F(st.m2) - e["xm"]) <= F(1, 10 ** 12) * e["xm"], col
        assert rel_close(st.metric_value(), math.sqrt(float(e["xm"]) / e["n"]))
