"""Row-exact conformance of the device's value-to-text printers under RLIKE against the oracle.

`x RLIKE p` over a double, float, decimal, date or timestamp x (a column, or casts over one) runs
in expr_kernel's XI_REGEX case (csrc/expr.hip), which prints Spark's cast of x to string per lane
-- jfmt::double_to_java / float_to_java (csrc/jfmt.h), dec_format / date_format / ts_format
(csrc/decimal.h) -- and walks the automaton over that text.  The cases are tests/format_cases.py
(checked on the host by tests/test_format_cases.py, where the host build of the same headers gives
the oracle's text on every row): per family a few hundred to a few thousand values in two device
batches, and a set of probes that determines every byte of every row's text.

Per probe p the device reports Sum(w, where=p), Sum(w, where=NOT (p)) and Size(where=p) over random
weights; all three must equal the exact integers over the oracle's TRUE and FALSE rows, as written
and under `where g = 0` (every eighth row).  FC.PROBES_PER_SCAN probes share one scan; explain()
must show each as an expr-bitmap task.

On a mismatch nothing is retried: `AND id BETWEEN a AND b` bisects to the first row whose verdict
differs (about log2(rows) scans), the probes restricted to that row spell the text the device
printed, and the failure names the probe, the sums, the row, its value bits and both texts.
"""
import time

import numpy as np
import pytest

import format_cases as FC
import regex_cases as RC

pytestmark = pytest.mark.gpu


def _device_table(fam, device):
    from deequ_amd.table import Table
    tables = [Table.from_arrow(t, device=device) for t in FC.arrow_batches(fam)]
    df = Table(tables[0].schema, [b for t in tables for b in t.batches], device)
    assert len(df.batches) == 2 and df.num_rows == len(fam.values)
    assert [b[fam.column].length for b in df.batches] == [fam.cut, len(fam.values) - fam.cut]
    return df


def _scan(df, fam, chunk, extra=None):
    """[(sum over TRUE rows, sum over FALSE rows, count of TRUE rows)] per probe of the chunk."""
    from deequ_amd.runners.engine import get_plan, run_scan
    specs = FC.scan_specs(fam, chunk, extra)
    FC.check_plan(get_plan(df.schema, specs).explain(), len(chunk))
    row = run_scan(df, specs)
    return [tuple(row[3 * k:3 * k + 3]) for k in range(len(chunk))]


def _want(tv, w, sel=None):
    """What _scan must report for a probe with truth vector tv among the selected rows.  Size
    counts over every row, so a row the filter rejects is FALSE there (regex_cases.kleene_and)."""
    e = RC.expected(tv, w, sel)
    size = e["count"] if sel is None else RC.expected(RC.kleene_and(tv, sel), w)["count"]
    return (e["sum_true"], e["sum_false"], size)


def _truth(pr, texts):
    """regex_cases' truth vector (True / False, None for a NULL row) of the probe."""
    return tuple(None if v < 0 else bool(v) for v in FC.truth(pr, texts).tolist())


def _diagnose(df, fam, pr, tv, w):
    """The first row at which the device's verdict on the probe differs, and the text the device
    printed there as all probes restricted to that row spell it."""
    n = len(tv)
    ids = np.arange(n)
    lo, hi = 0, n - 1
    while lo < hi:      # the first `mid` at which rows lo..mid differ (rows before lo agree)
        mid = (lo + hi) // 2
        sel = (ids >= lo) & (ids <= mid)
        got = _scan(df, fam, [pr], f"id BETWEEN {lo} AND {mid}")[0]
        if got != _want(tv, w, list(sel)):
            hi = mid
        else:
            lo = mid + 1
    row = lo
    verdicts = {}
    for chunk in FC.chunks(FC.probes(fam.alphabet, fam.lmax)):
        for q, got in zip(chunk, _scan(df, fam, chunk, f"id = {row}")):
            verdicts[q] = got[2] == 1
    return row, FC.decode(fam.alphabet, fam.lmax, lambda q: verdicts[q])


def _check(df, fam, extra, sel):
    w = RC.weights(len(fam.texts))
    ps = FC.probes(fam.alphabet, fam.lmax)
    scans = 0
    for chunk in FC.chunks(ps):
        got = _scan(df, fam, chunk, extra)
        scans += 1
        for pr, g in zip(chunk, got):
            tv = _truth(pr, fam.texts)
            want = _want(tv, w, sel)
            if g == want:
                continue
            row, printed = _diagnose(df, fam, pr, tv, w)
            pytest.fail(f"{fam.name}: {fam.operand} RLIKE {pr.pattern!r} under {extra}: "
                        f"(sum TRUE, sum FALSE, TRUE rows) device {g}, oracle {want} "
                        f"({sum(v is True for v in tv)} TRUE rows in all); first differing row {row}: "
                        f"{fam.raw[row]}, column value {fam.values[row]!r}, oracle text {fam.texts[row]!r}, "
                        f"device text {printed!r}")
    return len(ps), scans


@pytest.mark.parametrize("name", FC.family_names())
def test_printed_text_matches_the_oracle_on_every_row(name, gpu_device):
    fam = FC.family(name)
    t0 = time.perf_counter()
    df = _device_table(fam, gpu_device)
    n = len(fam.values)
    n_probes, scans = _check(df, fam, None, None)
    sel = [r % 8 == 0 for r in range(n)]
    scans += _check(df, fam, "g = 0", sel)[1]
    print(f"{name}: {n} rows, {n_probes} probes, {scans} scans, {time.perf_counter() - t0:.2f} s")
