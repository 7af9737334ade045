"""Moments and co-moments of the fused scan on ill-conditioned and poisoned inputs
(tests/moment_cases.py), through run_scan / the analyzers and the C ABI.

  a. conditioning, per body: Sum / Mean / StandardDeviation on every family and element type at
     the row counts that take each path of num_item (and dec_item for decimal(20, 4)), with and
     without a where filter, multi-batch, and the unaligned route (num_chunk_slow);
  b. co-moments, per path: Correlation over eight type pairs, rho in {0.8, -0.99}, asymmetric
     NULLs; the 8-byte pairs also fused with ApproxCountDistinct (corr_hll_chunk8), with
     DQ_NO_FUSE=1 and unaligned (the scalar loop of corr_rows on 8-byte types);
  c. merge paths: batches with means +1e9, -1e9, 0, 1e12 in one run and as per-batch states merged
     through State.sum; bit-identical from run to run;
  d. hidden rows: poison in NULL slots and under where-FALSE rows changes no bit of any result;
  e. visible non-finite and degenerate values against the oracle.

Bound: |got - exact| <= max(1e-12, C kappa 2^-52) scale, C measured on the oracle alone
(moment_cases.C; DESIGN.md section 6, "Moment conditioning").  Every figure is printed before it
is asserted."""
import math
import struct
from fractions import Fraction as F

import numpy as np
import pyarrow as pa
import pytest

import moment_cases as MC

pytestmark = pytest.mark.gpu

E12 = F(1, 10 ** 12)


def _specs(analyzers):
    return [s for a in analyzers for s in a.aggregation_functions()]


def _table(t, device, batch=None):
    from deequ_amd import Table
    return Table.from_arrow(t, device=device, max_batch_rows=batch)


def _check(fails, who, name, got, exact, allowed):
    err = abs(F(got) - exact)
    print(who, name, "got", got, "error", float(err), "allowed", float(allowed))
    if err > allowed:
        fails.append((who, name, got, float(exact), float(err), float(allowed)))


def _check_state(fails, who, state, e):
    """A (n, avg, m2) or six-component device state against exact_moments' e."""
    b = MC.component_bounds(e)
    if state[0] != e["n"]:
        fails.append((who, "n", state[0], e["n"]))
    names = ("xAvg", "xMk") if len(state) == 3 else ("xAvg", "yAvg", "ck", "xMk", "yMk")
    for name, got in zip(names, state[1:]):
        _check(fails, who, name, got, *b[name])


def _check_corr_metric(fails, who, st, e):
    ref = MC.exact_corr(e)
    if ref is None:
        return
    got = st.metric_value()
    print(who, "corr", got, "exact", ref[0], "allowed", ref[1])
    if not abs(got - ref[0]) <= ref[1]:
        fails.append((who, "corr", got, ref[0], ref[1]))


def _bits(v):
    """A result row as comparable bits: floats by their IEEE bytes, every NaN alike."""
    if isinstance(v, (tuple, list)):
        return tuple(_bits(x) for x in v)
    if isinstance(v, float):
        return "nan" if math.isnan(v) else struct.pack("<d", v)
    return v


def _same(a, b):
    """Exact, NaN-aware, sign-of-zero-blind (test_gpu_predicates._same)."""
    if a is None or b is None:
        return a is None and b is None
    return (math.isnan(a) and math.isnan(b)) or a == b


# ------------------------------------------------------------------------------------------------
# a. conditioning, per body
# ------------------------------------------------------------------------------------------------
def _moment_suite(where):
    from deequ_amd.analyzers import Mean, StandardDeviation, Sum
    return [Sum("x", where), Mean("x", where), StandardDeviation("x", where)]


def _check_moment_row(fails, who, row, c, w, is_exact_sum):
    """row = run_scan of _moment_suite: [sum, sum, count(*), (n, avg, m2)]."""
    from oracle import deequ_oracle as O
    e = c.exact[w]
    if e is None:
        if row[0] is not None or row[3][0] != 0:
            fails.append((who, "empty selection", row))
        return
    if is_exact_sum:                       # wrapping Long sums / exact decimal sums: bit-exact
        exp = O.agg_sum(c.otable, "x", w)
        print(who, "sum", row[0], exp)
        if row[0] != exp:
            fails.append((who, "sum", row[0], exp))
    else:
        _check(fails, who, "sum", row[0], e["mx"] * e["n"], E12 * e["sx"] * e["n"])
    if row[1] != row[0] or row[2] != c.n:
        fails.append((who, "mean's sum / count", row[1], row[2]))
    _check_state(fails, who, row[3], e)


@pytest.mark.parametrize("fam", MC.FAMILIES, ids=[f.name for f in MC.FAMILIES])
def test_conditioning_per_body(fam, gpu_device):
    """Sum / Mean / StandardDeviation of one family at 1, 7, 8, 9, 1023, 1024, 1025, 4097 rows,
    20 011 rows in batches of 4096 and (8-byte types) 33 000 rows, 5 % NULLs, with and without the
    where filter: n exact, integer and decimal sums exact, avg and m2 inside the bound."""
    from deequ_amd.runners.engine import run_scan
    fails = []
    for n, batch in MC.moment_cases(fam.name):
        c = MC.moment_case(fam.name, n, batch)
        df = _table(c.arrow, gpu_device, batch)
        for w in (None, MC.WHERE):
            row = run_scan(df, _specs(_moment_suite(w)))
            _check_moment_row(fails, (fam.name, n, w), row, c, w, fam.type not in ("f32", "f64"))
    assert not fails, fails


@pytest.mark.parametrize("name", ["i64_1e15", "i32_2e9", "i16_top", "i8_top"])
def test_conditioning_unaligned(name, gpu_device):
    """The same through num_chunk_slow: values 13 elements into their device buffer (vec_ok = 0),
    once per element width; the sums bit-identical to the aligned copy, the moments of both inside
    the bound."""
    from deequ_amd import Table
    from deequ_amd.runners.engine import run_scan
    from test_gpu_predicates import _ArrowDeviceColumn
    n, off = 4097, 13
    c = MC.moment_case(name, n + off)
    arr = c.arrow.column("x").combine_chunks()
    sl = arr.slice(off)
    t = pa.table({"x": pa.concat_arrays([sl]), "g": MC.side_column(n)})
    aligned = _table(t, gpu_device)
    x = _ArrowDeviceColumn(arr, off, gpu_device)
    try:
        assert x.column.values % 16 != 0
        batch = dict(aligned.batches[0])
        batch["x"] = x
        unaligned = Table(aligned.schema, [batch], gpu_device)
        vals = np.array(MC.doubles(MC.FAMILY[name].type, MC.family_values(name, n + off)))[off:]
        valid = ~np.asarray(sl.is_null())
        g = np.arange(n) % 8
        fails = []
        for w, m in ((None, valid), (MC.WHERE, valid & (g < 5))):
            specs = _specs(_moment_suite(w))
            got, ref = run_scan(unaligned, specs), run_scan(aligned, specs)
            e = MC.exact_moments([float(v) for v in vals[m]])
            print(name, w, got, ref)
            assert _bits(got[:3]) == _bits(ref[:3]) and got[3][0] == ref[3][0] == e["n"]
            _check_state(fails, (name, "unaligned", w), got[3], e)
            _check_state(fails, (name, "aligned", w), ref[3], e)
        assert not fails, fails
    finally:
        x.release()


# ------------------------------------------------------------------------------------------------
# b. co-moments, per path
# ------------------------------------------------------------------------------------------------
def _corr_state(row, k=0):
    from deequ_amd.analyzers import Correlation
    return Correlation("x", "y").from_aggregation_result(row, k)


def _check_corr_row(fails, who, row, k, c, w):
    e = c.exact[w]
    st = _corr_state(row, k)
    if e is None:
        if st is not None:
            fails.append((who, "empty selection", row[k]))
        return
    if st is None:
        fails.append((who, "no state", row[k]))
        return
    _check_state(fails, who, row[k], e)
    _check_corr_metric(fails, who, st, e)


@pytest.mark.parametrize("rho", MC.RHOS)
@pytest.mark.parametrize("tx,ty", MC.PAIRS)
def test_comoments_per_path(tx, ty, rho, gpu_device):
    """Correlation(x, y) at 1, 2, 511, 512, 513, 1024, 1025, 4097 rows and 20 011 rows in batches of
    4096; x NULL where y is not and the reverse, with runs of 64 such rows across the 512- and
    1024-row edges: all six components and the metric inside the bound."""
    from deequ_amd.analyzers import Correlation
    from deequ_amd.runners.engine import run_scan
    fails = []
    for n, batch in MC.pair_rows():
        c = MC.pair_case(tx, ty, rho, n, batch)
        df = _table(c.arrow, gpu_device, batch)
        for w in (None, MC.WHERE):
            row = run_scan(df, _specs([Correlation("x", "y", w)]))
            _check_corr_row(fails, (tx, ty, rho, n, w), row, 0, c, w)
    assert not fails, fails


@pytest.mark.parametrize("rho", MC.RHOS)
@pytest.mark.parametrize("tx,ty", MC.WIDE_PAIRS)
def test_comoments_fused_with_hll_and_unfused(tx, ty, rho, gpu_device, monkeypatch):
    """The 8-byte pairs beside ApproxCountDistinct(x) / (y): the plan fuses (corr_hll_chunk8), the
    state is inside the bound and bit-identical to the two-pass plan built under DQ_NO_FUSE=1; the
    HLL registers equal the oracle's."""
    from deequ_amd import _native as N
    from deequ_amd.analyzers import ApproxCountDistinct, Correlation
    from deequ_amd.runners.engine import Plan, get_plan, read_row, run_scan, scan_into
    from oracle import deequ_oracle as O
    fails = []
    for n, batch in [(1024, None), (1025, None), (4097, None), MC.ROWS_BATCHED]:
        c = MC.pair_case(tx, ty, rho, n, batch)
        df = _table(c.arrow, gpu_device, batch)
        for w in (None, MC.WHERE):
            for side in ("x", "y"):
                specs = _specs([ApproxCountDistinct(side, w), Correlation("x", "y", w)])
                explain = get_plan(df.schema, specs).explain()
                assert "+hll[" in explain, explain
                fused = run_scan(df, specs)
                monkeypatch.setenv("DQ_NO_FUSE", "1")
                plan = Plan(df.schema, specs)                # (uncached: the switch is read here)
                monkeypatch.delenv("DQ_NO_FUSE")
                assert "+hll[" not in plan.explain(), plan.explain()
                st = plan.state(df.device_index())
                N.check(N.lib.dq_state_reset(st))
                scan_into(df, plan, st)
                unfused = read_row(plan, st)
                who = (tx, ty, rho, n, w, "hll " + side)
                print(who, fused[1], unfused[1])
                assert _bits(fused) == _bits(unfused), who
                if n <= 4097:
                    assert list(fused[0]) == O.agg_hll(c.otable, side, w), who
                _check_corr_row(fails, who, fused, 1, c, w)
    assert not fails, fails


@pytest.mark.parametrize("tx,ty", MC.WIDE_PAIRS)
def test_comoments_unaligned_8_byte_pairs(tx, ty, gpu_device):
    """vec_ok = 0 on 8-byte columns: x sits 13 elements into its device buffer, so corr_rows runs
    its scalar loop over the whole item; inside the bound, n equal to the aligned run."""
    from deequ_amd import Table
    from deequ_amd.analyzers import Correlation
    from deequ_amd.runners.engine import run_scan
    from test_gpu_predicates import _ArrowDeviceColumn
    n, off, rho = 4097, 13, 0.8
    c = MC.pair_case(tx, ty, rho, n + off)
    full = c.arrow.slice(off)
    t = pa.table({k: pa.concat_arrays(full.column(k).chunks) for k in ("x", "y")})
    t = t.append_column("g", MC.side_column(n))
    aligned = _table(t, gpu_device)
    x = _ArrowDeviceColumn(c.arrow.column("x").combine_chunks(), off, gpu_device)
    try:
        assert x.column.values % 16 != 0
        batch = dict(aligned.batches[0])
        batch["x"] = x
        unaligned = Table(aligned.schema, [batch], gpu_device)
        vx = ~np.asarray(t.column("x").is_null())
        vy = ~np.asarray(t.column("y").is_null())
        xd = t.column("x").combine_chunks().fill_null(0).to_numpy().astype(np.float64)
        yd = t.column("y").combine_chunks().fill_null(0).to_numpy().astype(np.float64)
        g = np.arange(n) % 8
        fails = []
        for w, m in ((None, vx & vy), (MC.WHERE, vx & vy & (g < 5))):
            specs = _specs([Correlation("x", "y", w)])
            got, ref = run_scan(unaligned, specs), run_scan(aligned, specs)
            e = MC.exact_moments([float(v) for v in xd[m]], [float(v) for v in yd[m]])
            print(tx, ty, w, got, ref)
            assert got[0][0] == ref[0][0] == e["n"]
            _check_state(fails, (tx, ty, "unaligned", w), got[0], e)
            _check_state(fails, (tx, ty, "aligned", w), ref[0], e)
            _check_corr_metric(fails, (tx, ty, "unaligned", w), _corr_state(got), e)
        assert not fails, fails
    finally:
        x.release()


# ------------------------------------------------------------------------------------------------
# c. merge paths
# ------------------------------------------------------------------------------------------------
def test_merge_paths_across_batches_of_distant_means(gpu_device):
    """Four 2048-row batches with means +1e9, -1e9, 0, 1e12 (sd 1): one run over all batches and
    the per-batch states merged through State.sum are both inside the bound of the exact moments,
    within twice the bound of each other, and a second run is bit-identical to the first."""
    from deequ_amd.analyzers import Correlation, StandardDeviation
    from deequ_amd.analyzers.base import merge_states
    from deequ_amd.runners.engine import run_scan
    rows = 2048
    rng = np.random.default_rng(31)
    means = np.repeat([1e9, -1e9, 0.0, 1e12], rows)
    n = len(means)
    z, e_ = rng.normal(0.0, 1.0, n), rng.normal(0.0, 1.0, n)
    x = means + z
    y = -0.5 * means + 0.8 * z + 0.6 * e_
    vx, vy = rng.random(n) >= 0.05, rng.random(n) >= 0.05
    t = pa.table({"x": MC.arrow_array(x, vx), "y": MC.arrow_array(y, vy)})
    whole = _table(t, gpu_device, rows)
    assert len(whole.batches) == 4
    parts = [_table(t.slice(k * rows, rows), gpu_device) for k in range(4)]
    ex = MC.exact_moments([float(v) for v in x[vx]])
    exy = MC.exact_moments([float(v) for v in x[vx & vy]], [float(v) for v in y[vx & vy]])
    fails = []
    for a, e in ((StandardDeviation("x"), ex), (Correlation("x", "y"), exy)):
        specs = a.aggregation_functions()
        one = run_scan(whole, specs)
        assert _bits(run_scan(whole, specs)) == _bits(one)
        merged = merge_states(*[a.compute_state_from(p) for p in parts])
        again = merge_states(*[a.compute_state_from(p) for p in parts])
        assert merged == again
        if isinstance(a, StandardDeviation):
            m = (merged.n, merged.avg, merged.m2)
        else:
            m = (merged.n, merged.x_avg, merged.y_avg, merged.ck, merged.x_mk, merged.y_mk)
        _check_state(fails, (str(a), "one run"), one[0], e)
        _check_state(fails, (str(a), "merged states"), m, e)
        b = MC.component_bounds(e)
        names = ("xAvg", "xMk") if len(m) == 3 else ("xAvg", "yAvg", "ck", "xMk", "yMk")
        for name, p, q in zip(names, one[0][1:], m[1:]):
            assert abs(F(p) - F(q)) <= 2 * b[name][1], (str(a), name, p, q)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------
# d. hidden rows
# ------------------------------------------------------------------------------------------------
def _hidden_suites(col, where, lo, hi):
    """Two plans: the aggregates with a plain (vector or scalar) Correlation, and the HLL tasks
    beside a Correlation (fused on 8-byte columns)."""
    from deequ_amd.analyzers import (ApproxCountDistinct, Completeness, Compliance, Correlation, Maximum,
                                     Mean, Minimum, StandardDeviation, Sum)
    rng_pred = f"{col} IS NULL OR ({col} >= {lo} AND {col} <= {hi})"
    plain = [Sum(col, where), Mean(col, where), Minimum(col, where), Maximum(col, where),
             StandardDeviation(col, where), Completeness(col, where), Compliance("r", rng_pred, where),
             Correlation(col, "y", where), Correlation("y", col, where)]
    hll = [ApproxCountDistinct(col, where), Correlation(col, "y", where), ApproxCountDistinct("y", where)]
    return plain, hll


def _check_hidden_against_oracle(row_plain, row_hll, ot, col, where, lo, hi):
    """The rows of _hidden_suites against the oracle (exact arithmetic for the moments)."""
    from oracle import deequ_oracle as O
    xs = [v for v in O._sel(ot, col, where)]
    ys = [v for v in O._sel(ot, "y", where)]
    sel = [float(v) for v in xs if v is not None]
    e = MC.exact_moments(sel)
    is_int = ot.types[col] in ("byte", "short", "int", "long")
    fails = []
    if is_int:
        assert row_plain[0] == O.agg_sum(ot, col, where)
    else:
        _check(fails, col, "sum", row_plain[0], e["mx"] * e["n"], E12 * e["sx"] * e["n"])
    assert row_plain[1] == row_plain[0] and row_plain[2] == ot.n
    assert _same(row_plain[3], O.agg_min(ot, col, where)) and _same(row_plain[4], O.agg_max(ot, col, where))
    _check_state(fails, (col, where, "stddev"), row_plain[5], e)
    assert row_plain[6] == O.agg_sum_notnull(ot, col, where)
    assert row_plain[7] == O.agg_conditional_count(ot, where)
    pred = f"{col} IS NULL OR ({col} >= {lo} AND {col} <= {hi})"
    assert row_plain[8] == O.agg_compliance(ot, pred, where)
    pairs = [(float(a), float(b)) for a, b in zip(xs, ys) if a is not None and b is not None]
    exy = MC.exact_moments([p[0] for p in pairs], [p[1] for p in pairs])
    eyx = MC.exact_moments([p[1] for p in pairs], [p[0] for p in pairs])
    _check_state(fails, (col, where, "corr x y"), row_plain[10], exy)
    _check_state(fails, (col, where, "corr y x"), row_plain[11], eyx)
    _check_state(fails, (col, where, "corr beside hll"), row_hll[1], exy)
    assert list(row_hll[0]) == O.agg_hll(ot, col, where)
    assert list(row_hll[2]) == O.agg_hll(ot, "y", where)
    assert not fails, fails


@pytest.mark.parametrize("n", [4097, 33_000])
@pytest.mark.parametrize("ty", MC.NUMERIC)
def test_hidden_rows_stay_hidden(ty, n, gpu_device):
    """Every poison value of the type cycled through the NULL slots of x (30 % NULLs) and of its
    float64 partner y, and through the rows of z that the filter f = 1 drops, against the same
    table with zeros there: every result bit-identical -- Sum, Mean, Minimum, Maximum,
    StandardDeviation, Completeness, a fused range Compliance, Correlation (vector path for the
    8-byte types, scalar loop for the others, fused with HLL), ApproxCountDistinct's registers --
    and, at 4097 rows, equal to the oracle."""
    from deequ_amd.runners.engine import get_plan, run_scan
    h = MC.hidden_case(ty, n)
    dfp, dfz = _table(h.poison, gpu_device), _table(h.zeros, gpu_device)
    lo, hi = (-50, 150) if ty in ("f32", "f64", "i8") else (-20_000, 500_000)
    for col, where in (("x", None), ("x", "f = 1"), ("z", "f = 1")):
        plain, hll = _hidden_suites(col, where, lo, hi)
        sp, sh = _specs(plain), _specs(hll)
        if ty in ("i64", "f64"):
            assert "+hll[" in get_plan(dfp.schema, sh).explain()
        assert " numeric " in get_plan(dfp.schema, sp).explain()
        rp, rz = run_scan(dfp, sp), run_scan(dfz, sp)
        hp, hz = run_scan(dfp, sh), run_scan(dfz, sh)
        print(ty, n, col, where, rp, rz)
        assert _bits(rp) == _bits(rz), (ty, n, col, where, rp, rz)
        assert _bits(hp) == _bits(hz), (ty, n, col, where)
        assert not any(isinstance(v, float) and math.isnan(v) for v in rp[:5])
        if n == 4097:
            _check_hidden_against_oracle(rp, hp, h.otable, col, where, lo, hi)


def test_all_null_column_full_of_nan(gpu_device):
    """33 000 NULL rows whose slots all hold NaN (and a second column with +Inf there): the same
    empty results as over zeros."""
    from deequ_amd.analyzers import (ApproxCountDistinct, Completeness, Correlation, Maximum, Mean, Minimum,
                                     StandardDeviation, Sum)
    from deequ_amd.runners.engine import run_scan
    n = 33_000
    none = np.zeros(n, bool)
    y = np.random.default_rng(3).normal(0.0, 1.0, n)
    rows = []
    for fill in (np.nan, 0.0):
        t = pa.table({"x": MC.arrow_array(np.full(n, fill), none),
                      "y": MC.arrow_array(y, np.ones(n, bool))})
        suite = [Sum("x"), Mean("x"), Minimum("x"), Maximum("x"), StandardDeviation("x"),
                 Completeness("x"), Correlation("x", "y"), Correlation("y", "x"), ApproxCountDistinct("x")]
        rows.append(run_scan(_table(t, gpu_device), _specs(suite)))
    print(rows[0])
    assert _bits(rows[0]) == _bits(rows[1])
    r = rows[0]
    assert r[0] is None and r[1] is None and r[3] is None and r[4] is None
    assert r[5][0] == 0 and r[6] == 0 and r[7] == n and r[8][0] == 0 and r[9][0] == 0
    assert not any(r[10])


# ------------------------------------------------------------------------------------------------
# e. visible non-finite and degenerate values
# ------------------------------------------------------------------------------------------------
def _visible_cases(ty):
    dt = MC.NP[ty]
    rng = np.random.default_rng(41)
    n = 1025
    base = rng.normal(100.0, 30.0, n).astype(dt)
    y = rng.normal(-5.0, 2.0, n)

    def put(**at):
        v = base.copy()
        for k, val in at.items():
            v[int(k[1:])] = val
        return v
    return [("one +Inf", put(r512=np.inf), y), ("+Inf and -Inf", put(r341=np.inf, r683=-np.inf), y),
            ("NaN at row 0", put(r0=np.nan), y), ("NaN at the last row", put(r1024=np.nan), y),
            ("constant 7", np.full(n, 7.0, dt), y), ("constant 0.1", np.full(n, 0.1, dt), y),
            ("both constant", np.full(n, 0.1, dt), np.full(n, -2.5)),
            ("n = 1", np.array([3.5], dt), y[:1]), ("n = 2", np.array([3.5, -1.25], dt), y[:2]),
            ("Inf on the y side only", base, np.where(np.arange(n) == 700, np.inf, y))]


def _same_kind(got, exp):
    """NaN where the oracle has NaN, the same infinity where it has one."""
    if math.isnan(exp):
        return math.isnan(got)
    if math.isinf(exp):
        return got == exp
    return math.isfinite(got)


VISIBLE = ["one +Inf", "+Inf and -Inf", "NaN at row 0", "NaN at the last row", "constant 7", "constant 0.1",
           "both constant", "n = 1", "n = 2", "Inf on the y side only"]


@pytest.mark.parametrize("case", VISIBLE)
@pytest.mark.parametrize("ty", ["f64", "f32"])
def test_visible_non_finite_and_degenerate_values(ty, case, gpu_device):
    """+-Inf, NaN, constant columns, n = 1 and n = 2 in StandardDeviation, Sum, Mean and
    Correlation against the oracle: n exact, every component NaN / infinite exactly where the
    oracle's is, the finite ones inside the bound (against exact arithmetic where the data are
    finite, on the finite side alone where they are not).

    Pins a finding ("Moment conditioning"): 1025 rows of float64 0.1 gave
    m2 = xMk = 1.973964903000188e-31 and Correlation -0.0004122234873349561 where the oracle has 0
    and NaN (0 / 0) -- a lane's block mean sum / nb is not the constant, 0.1 + 0.1 + 0.1 already
    rounds -- until the block mean was clamped into the block's [min, max] (clamp_block_mean,
    scan.hip)."""
    from deequ_amd.analyzers import Correlation, Mean, StandardDeviation, Sum
    from deequ_amd.runners.engine import run_scan
    from oracle import deequ_oracle as O
    fails = []
    for name, x, y in [c for c in _visible_cases(ty) if c[0] == case]:
        n = len(x)
        t = pa.table({"x": pa.array(x), "y": pa.array(y)})
        ot = MC.oracle_table(t, {"x": ty, "y": "f64"})
        suite = [Sum("x"), Mean("x"), StandardDeviation("x"), Correlation("x", "y"), Correlation("y", "x")]
        row = run_scan(_table(t, gpu_device), _specs(suite))
        osd = O.agg_stddev(ot, "x", None)
        oxy, oyx = O.agg_corr(ot, "x", "y", None), O.agg_corr(ot, "y", "x", None)
        print(ty, name, row, osd, oxy)
        who = (ty, name)
        osum = O.agg_sum(ot, "x", None)                 # (a finite sum: 1e-12 of sum|x|)
        if not (_same(row[0], osum) or (math.isfinite(osum) and math.isfinite(row[0]) and
                                        abs(row[0] - osum) <= 1e-12 * float(np.abs(x).sum()))):
            fails.append((who, "sum", row[0], osum))
        if row[2] != n or row[3][0] != n or row[4][0] != n or row[5][0] != n:
            fails.append((who, "n", row))
        finite = bool(np.isfinite(x).all() and np.isfinite(y).all())
        xs, ys = [float(v) for v in x], [float(v) for v in y]
        for part, got, exp in (("stddev", row[3], osd), ("corr x y", row[4], oxy), ("corr y x", row[5], oyx)):
            for k, (g, o) in enumerate(zip(got[1:], exp[1:])):
                if not _same_kind(g, o):
                    fails.append((who, part, "component", k + 1, g, o))
            if finite:
                e = MC.exact_moments(*{"stddev": (xs,), "corr x y": (xs, ys), "corr y x": (ys, xs)}[part])
                _check_state(fails, who + (part,), got, e)
        if finite:
            for k, a in ((4, Correlation("x", "y")), (5, Correlation("y", "x"))):
                got = a.from_aggregation_result(row, k).metric_value()
                o = oxy if k == 4 else oyx
                den = math.sqrt(o[4] * o[5])
                exp = o[3] / den if den else float("nan")
                print(who, "metric", got, exp)
                if math.isnan(exp) != math.isnan(got):
                    fails.append((who, "corr metric", got, exp))
                elif not math.isnan(exp):
                    _check_corr_metric(fails, who, a.from_aggregation_result(row, k),
                                       MC.exact_moments(xs, ys) if k == 4 else MC.exact_moments(ys, xs))
            sd = StandardDeviation("x").from_aggregation_result(row, 3).metric_value()
            if "constant" in name and sd != 0.0:
                fails.append((who, "stddev of a constant", sd))
        elif np.isfinite(y).all():                      # the finite side keeps finite moments
            e = MC.exact_moments(ys)
            b = MC.component_bounds(e)
            _check(fails, who, "yAvg", row[4][2], *b["xAvg"])
            _check(fails, who, "yMk", row[4][5], *b["xMk"])
            _check(fails, who, "xMk of (y, x)", row[5][4], *b["xMk"])
        elif np.isfinite(x).all():
            e = MC.exact_moments(xs)
            b = MC.component_bounds(e)
            _check_state(fails, who + ("stddev",), row[3], e)
            _check(fails, who, "xAvg", row[4][1], *b["xAvg"])
            _check(fails, who, "xMk", row[4][4], *b["xMk"])
            _check(fails, who, "yMk of (y, x)", row[5][5], *b["xMk"])
    assert not fails, fails
