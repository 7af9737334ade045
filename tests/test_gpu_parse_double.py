"""The correctly rounded Double.parseDouble on the device: the two-pass string cast (dq_cast_utf8,
csrc/cast.hip), the profiler over a column of repr() strings, and the predicate interpreter's
CAST(s AS DOUBLE) and string-against-number comparisons (csrc/expr.hip).  The reference is
cast_cases.java_parse_double, never the oracle (which does not read hex).

The cast is called the way tests/test_gpu_cast_rows.py calls it (its helpers are used here): the
outputs poisoned, NULL input rows whose bytes spell values, a sliced column.  Batches are composed
from rows the first kernel decides (EASY) and rows only the exact fallback decides (HARD, checked
with the host build of the same parser), so that the undecided list is in turn empty, one entry,
every row, and more entries than one block of the second kernel (64) handles; undecided rows share
validity bytes with decided, NULL-input and rejected rows.
"""
import ctypes
import math

import numpy as np
import pyarrow as pa
import pytest

import cast_cases as CC
import parse_double_cases as PD
import test_gpu_cast_rows as R

pytestmark = pytest.mark.gpu

REJECTED = [b"abc", b"1.2.3", b"", b"- 1", b"1e", b"0x1"]
NON_PLAIN = [b"1e5", b"NaN", b"0x1p3", b"1.5f", b"-Infinity", b"2.5E-3d"]


def _needs_fallback(b):
    from deequ_amd import _native as N
    before = N.parse_double_fallbacks()
    N.parse_double_utf8(b)
    return N.parse_double_fallbacks() != before


@pytest.fixture(scope="module")
def pools():
    """(EASY, HARD): plain decimals of at most 700 bytes that Java reads, split by whether the host
    build of the parser needs the exact fallback for them."""
    plain = [b for b in PD.HALFWAY_PLAIN + PD.RANDOM["20 to 40 digits"] + PD.RANDOM["17 to 19 digits"]
             + PD.RANDOM["scaled decimals"][:300] + CC.TABLES["window edges"]
             if PD.is_plain(b) and len(b) <= 700 and CC.java_parse_double(b)[0] == CC.VALUE]
    hard = [b for b in plain if _needs_fallback(b)]
    easy = [b for b in plain if not _needs_fallback(b)]
    assert len(hard) > 100 and len(easy) > 1000
    return easy, hard


def _cast_double(rows, device):
    from deequ_amd import _native as N
    col = R._device_column(rows, device)
    return R._cast(col.to_c(), len(rows), N.FLOAT64, device)


def _check_plain(rows, device):
    """All-plain input: nothing unsupported, validity and bits per row."""
    valid, values, bad = _cast_double(rows, device)
    assert bad == 0
    for i, b in enumerate(rows):
        cls, ref = (CC.NULL, None) if b is None else CC.java_parse_double(b)
        assert bool(valid[i]) == (cls == CC.VALUE), (i, b if b is None else b[:60])
        if valid[i]:
            assert PD.same_double(float(values[i]), ref), (i, b[:60], float(values[i]).hex(), ref.hex())
    CC.check_double(rows, valid, values, bad)


def _mixed(n, easy, hard):
    """Period 11 against 8 rows per validity byte: every kind of row meets every bit position."""
    pattern = ("hard", "easy", "null", "rejected", "hard", "easy", "easy", "hard", "rejected",
               "easy", "null")
    rows = []
    for i in range(n):
        kind = pattern[i % len(pattern)]
        rows.append(None if kind == "null" else hard[i % len(hard)] if kind == "hard"
                    else easy[i % len(easy)] if kind == "easy" else REJECTED[i % len(REJECTED)])
    return rows


@pytest.mark.parametrize("name", ["window edges", *PD.RANDOM, "halfway plain", "hard"])
def test_plain_tables(name, gpu_device):
    rows = {"window edges": CC.TABLES["window edges"], "halfway plain": PD.HALFWAY_PLAIN,
            "hard": PD.HARD, **PD.RANDOM}[name]
    rows = [b for b in rows if CC.java_parse_double(b)[0] == CC.NULL or PD.is_plain(b)]
    assert len(rows) >= 10
    _check_plain(rows, gpu_device)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 6001])
def test_row_counts_with_undecided_rows_in_shared_validity_bytes(n, pools, gpu_device):
    _check_plain(_mixed(n, *pools), gpu_device)


def test_undecided_list_empty_single_and_every_row(pools, gpu_device):
    easy, hard = pools
    none = [easy[i % len(easy)] for i in range(2049)]
    _check_plain(none, gpu_device)
    for at in (0, 1000, 2048):
        one = list(none)
        one[at] = hard[at % len(hard)]
        _check_plain(one, gpu_device)
    for n in (1, 9, 6001):     # 6001 rows: 751 entries, twelve blocks of the second kernel
        _check_plain([hard[i % len(hard)] for i in range(n)], gpu_device)


def test_non_plain_forms_are_still_counted_exactly(pools, gpu_device):
    rows = _mixed(2049, *pools)
    for i in range(3, len(rows), 7):
        rows[i] = NON_PLAIN[i % len(NON_PLAIN)]
    valid, values, bad = _cast_double(rows, gpu_device)
    want = sum(b is not None and not PD.is_plain(b) and CC.java_parse_double(b)[0] == CC.VALUE
               for b in rows)
    assert bad == want and want > 200
    CC.check_double(rows, valid, values, bad)
    for i, b in enumerate(rows):
        if b is not None and PD.is_plain(b):
            assert bool(valid[i]) == (CC.java_parse_double(b)[0] == CC.VALUE), (i, b[:60])


@pytest.mark.parametrize("offset", [3, 11])
def test_sliced_column(offset, pools, gpu_device):
    import torch
    from deequ_amd import _native as N
    from deequ_amd.loader import ArrowArrayC, ArrowSchemaC
    whole = _mixed(300, *pools)
    rows = whole[offset:len(whole) - 5]
    validity, offsets, data = R._host_buffers(whole)
    dev = [torch.from_numpy(a.copy()).to(gpu_device) for a in (validity, offsets, data)]
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in dev])
    a = ArrowArrayC(length=len(rows), null_count=sum(b is None for b in rows), offset=offset,
                    n_buffers=3, n_children=0, buffers=ptrs)
    s = ArrowSchemaC(format=b"u", name=b"s", flags=2)
    col = N.dq_column()
    N.check(N.lib.dq_column_from_arrow(ctypes.addressof(a), ctypes.addressof(s), ctypes.byref(col)))
    try:
        valid, values, bad = R._cast(col, len(rows), N.FLOAT64, gpu_device)
        assert bad == 0
        CC.check_double(rows, valid, values, bad)
        assert [bool(v) for v in valid] == [b is not None and CC.java_parse_double(b)[0] == CC.VALUE
                                            for b in rows]
    finally:
        N.lib.dq_column_release(ctypes.byref(col))


# ------------------------------------------------------------------------------------------------
# The profiler
# ------------------------------------------------------------------------------------------------
def test_profile_of_a_column_of_repr_strings(gpu_device):
    """repr() of a double has up to 17 significant digits: the parent build raised
    NotImplementedError here."""
    from deequ_amd.analyzers.datatype import DataTypeInstances
    from deequ_amd.profiles import ColumnProfilerRunner, NumericColumnProfile
    from deequ_amd.table import Table
    rng = np.random.default_rng(7)
    xs = (rng.uniform(-1000, 1000, 2600) * 10.0 ** rng.integers(-2, 6, 2600)).tolist()
    xs = [x for x in xs if "e" not in repr(x)][:2000] + [0.30000000000000004, 0.1 + 0.7]
    assert len(xs) == 2002 and sum(len(repr(x).replace("-", "").replace(".", "")) >= 17
                                   for x in xs) > 300
    vals = [None if i % 97 == 5 else x for i, x in enumerate(xs)]
    texts = [None if x is None else repr(x) for x in vals]
    df = Table.from_pydict({"s": texts, "d": vals}, {"s": "string", "d": "float64"},
                           device=gpu_device)
    profiles = (ColumnProfilerRunner().on_data(df).only_consider_column_subset(["s", "d"])
                .run().profiles)
    s, d = profiles["s"], profiles["d"]
    assert isinstance(s, NumericColumnProfile)
    print([(p.minimum, p.maximum, p.mean, p.sum) for p in (s, d)])
    assert s.data_type == DataTypeInstances.Fractional and s.is_data_type_inferred
    assert s.completeness == d.completeness
    assert (s.minimum, s.maximum) == (d.minimum, d.maximum)
    assert (s.minimum, s.maximum) == (min(x for x in vals if x is not None),
                                      max(x for x in vals if x is not None))
    for got, want in ((s.mean, d.mean), (s.sum, d.sum)):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)


# ------------------------------------------------------------------------------------------------
# The predicate interpreter
# ------------------------------------------------------------------------------------------------
def _predicate_rows():
    rows = (PD.java_forms_padded() + PD.HARD + PD.HEX + [b for b, _ in PD.BEYOND_REFERENCE]
            + [b for b in PD.HALFWAY_PLAIN + PD.HALFWAY_EXP if len(b) <= 420]
            + PD.RANDOM["20 to 40 digits"][:150] + PD.RANDOM["17 to 19 digits"][:100])
    out = []
    for b in rows:
        try:
            text = b.decode("utf-8")
        except UnicodeDecodeError:
            continue
        out.append((b, text))
    return out


def _reference(b):
    beyond = dict(PD.BEYOND_REFERENCE)
    return (CC.VALUE, beyond[b]) if b in beyond else CC.java_parse_double(b)


def _metric(ctx, a):
    return ctx.metric(a).value.get()


def test_cast_in_predicates_matches_the_reference_for_every_form(gpu_device):
    """d holds the reference value, or on every third readable row its neighbour, so TRUE, FALSE and
    NULL rows all occur; Spark's NaN = NaN is TRUE."""
    from deequ_amd import Analysis
    from deequ_amd.analyzers import Compliance, Size, Sum
    from deequ_amd.table import Table
    rows = _predicate_rows()
    rng = np.random.default_rng(3)
    w = rng.integers(0, 2 ** 40, len(rows)).tolist()
    d, truth = [], []
    for i, (b, _) in enumerate(rows):
        cls, ref = _reference(b)
        if cls == CC.NULL:
            d.append(1.0)
            truth.append(None)
        elif i % 3 == 0 and ref == ref and abs(ref) != math.inf:
            d.append(math.nextafter(ref, math.inf))
            truth.append(False)
        else:
            d.append(ref)
            truth.append(True)
    kinds = {k: sum(t is k for t in truth) for k in (True, False, None)}
    print(len(rows), "rows", kinds)
    assert min(kinds.values()) > 50
    assert any(r != r for r in d) and sum(b.lower().lstrip(b" +-\x00").startswith(b"0x")
                                          for (b, _), t in zip(rows, truth) if t) > 10
    df = Table.from_pydict({"s": [t for _, t in rows], "d": d, "w": w},
                           {"s": "string", "d": "float64", "w": "int64"}, device=gpu_device)
    p = "CAST(s AS DOUBLE) = d"
    suite = [Compliance("p", p), Size(where="CAST(s AS DOUBLE) IS NULL"),
             Sum("w", where=p), Sum("w", where=f"NOT ({p})"), Size(where=p)]
    ctx = Analysis(suite).run(df)
    sums = {k: sum(x for x, t in zip(w, truth) if t is k) for k in (True, False)}
    assert sum(w) < 2 ** 53
    assert _metric(ctx, suite[2]) == sums[True], "rows the interpreter calls TRUE"
    assert _metric(ctx, suite[3]) == sums[False], "rows the interpreter calls FALSE"
    assert _metric(ctx, suite[4]) == kinds[True]
    assert _metric(ctx, suite[1]) == kinds[None]
    assert _metric(ctx, suite[0]) == kinds[True] / len(rows)


def test_string_against_a_literal_one_ulp_around_it(gpu_device):
    """`s > literal` promotes s to double.  Around each literal y: strings just below and just above
    the midpoints that separate y from its neighbours, so the rounding of s decides the row."""
    from deequ_amd import Analysis
    from deequ_amd.analyzers import Compliance, Sum
    from deequ_amd.table import Table
    for y in (0.30000000000000004, 9007199254740994.0, 123456.78901234567):
        texts = []
        for lo in (math.nextafter(y, -math.inf), y):
            digits, scale = PD.midpoint(lo)
            for v in ((str(int(digits) - 1), scale), (digits, scale), (str(int(digits) + 1), scale)):
                texts += [PD.render_plain(*v).decode(), PD.render_exp(*v).decode()]
        texts += [repr(y), repr(math.nextafter(y, math.inf)), repr(math.nextafter(y, -math.inf)),
                  "0x1p-1074", "NaN", "abc", "-Infinity"]
        ref = [CC.java_parse_double(t.encode())[1] for t in texts]
        # Spark's order: NaN is greater than every number
        truth = [None if r is None else (r != r or r > y) for r in ref]
        assert sum(r == y for r in ref if r is not None) >= 5
        w = [1 << i for i in range(len(texts))]
        df = Table.from_pydict({"s": texts, "w": w}, {"s": "string", "w": "int64"},
                               device=gpu_device)
        p = f"s > {y!r}"
        suite = [Sum("w", where=p), Sum("w", where=f"NOT ({p})"), Compliance("p", p)]
        ctx = Analysis(suite).run(df)
        print(p, truth)
        assert _metric(ctx, suite[0]) == sum(x for x, t in zip(w, truth) if t is True)
        assert _metric(ctx, suite[1]) == sum(x for x, t in zip(w, truth) if t is False)
        assert _metric(ctx, suite[2]) == sum(t is True for t in truth) / len(texts)
