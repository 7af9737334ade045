"""RowLevelSchemaValidator on the device against the plain-Python restatement
(tests/schema_host.py): the reference's seven tests, the line-246 NULL verdict, randomised row-for-row
parity over every batch-size edge of the selection kernels, and the selection primitive through
the C ABI alone.  All comparisons are exact."""
import ctypes
import random

import numpy as np
import pytest

import schema_host as H
from test_schema_host import DECIMAL_CASES, INT_CASES, MASK, TS_CASES

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def engine_schema(defs):
    from deequ_amd import RowLevelSchema
    s = RowLevelSchema()
    for d in defs:
        kw = {k: v for k, v in d.items() if k not in ("kind", "name")}
        s = getattr(s, f"with_{d['kind']}_column")(d["name"], **kw)
    return s


def column_to_list(c):
    """One device ColumnBatch as Python values (None = NULL; decimals as unscaled ints)."""
    from deequ_amd import _native as N
    n = c.length
    valid = np.ones(n, bool)
    if c.validity is not None:
        valid = np.unpackbits(c.validity.cpu().numpy(), bitorder="little")[:n].astype(bool)
    tid = N.type_id(c.dtype)
    if tid == N.UTF8:
        off = c.values.cpu().numpy()[:n + 1]
        data = c.data.cpu().numpy().tobytes()
        assert n == 0 or off[0] == 0
        vals = [data[off[i]:off[i + 1]].decode("utf-8") for i in range(n)]
    elif tid == N.BOOL:
        vals = [bool(x) for x in np.unpackbits(c.values.cpu().numpy(), bitorder="little")[:n]]
    elif tid == N.DECIMAL128:
        w = c.values.cpu().numpy().view(np.uint64)[:2 * n].tolist()
        vals = [((w[2 * i + 1] << 64) | w[2 * i]) - ((1 << 128) if w[2 * i + 1] >> 63 else 0)
                for i in range(n)]
    else:
        vals = c.values.cpu().numpy()[:n].tolist()
    return [v if ok else None for v, ok in zip(vals, valid)]


def table_to_lists(t):
    return {f.name: [v for b in t.batches for v in column_to_list(b[f.name])] for f in t.schema.fields}


def string_table(columns, device, extra=None, extra_types=None):
    import pyarrow as pa
    from deequ_amd.table import Table
    cols = dict(columns)
    types = {c: pa.string() for c in columns}
    cols.update(extra or {})
    types.update(extra_types or {})
    return Table.from_pydict(cols, types, device=device)


def type_names(t):
    return {f.name: f.type_name for f in t.schema.fields}


# ------------------------------------------------------------------------------------------------
# the reference's tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.load_known_answers(), ids=lambda c: c["name"])
def test_known_answers_on_the_device(gpu_device, case):
    from deequ_amd import RowLevelSchemaValidator
    from deequ_amd import _native as N
    data = string_table(case["columns"], gpu_device)
    res = RowLevelSchemaValidator.validate(data, engine_schema(case["schema"]))
    valid, invalid = table_to_lists(res.valid_rows), table_to_lists(res.invalid_rows)
    H.assert_known_answer(case, valid, invalid, res.num_valid_rows, res.num_invalid_rows,
                          type_names(res.valid_rows), type_names(res.invalid_rows))
    # and row for row what the restatement gives, declared columns cast to their types
    want_valid, want_invalid = H.validate(case["schema"], case["columns"])
    assert valid == want_valid and invalid == want_invalid
    assert res.valid_rows.num_rows == res.num_valid_rows
    assert res.invalid_rows.num_rows == res.num_invalid_rows
    for d in case["schema"]:
        got = res.valid_rows.schema[d["name"]].dtype
        want = {"int": N.INT32, "string": N.UTF8, "timestamp": N.TIMESTAMP_US}.get(d["kind"]) or \
            N.decimal_type(d["precision"], d["scale"])
        assert got == want
        assert res.invalid_rows.schema[d["name"]].dtype == N.UTF8


def test_null_verdict_of_line_246(gpu_device):
    """Derived by reading RowLevelSchemaValidator.scala:246: `colIsNull.isNull` is always false, so
    a NULL in a nullable int column with a min_value makes the row's verdict NULL and the row is in
    neither output.  The reference's tests do not reach this."""
    from deequ_amd import RowLevelSchema, RowLevelSchemaValidator
    data = string_table({"id": ["5", None, "x"]}, gpu_device)
    res = RowLevelSchemaValidator.validate(data, RowLevelSchema().with_int_column("id", min_value=0))
    assert (res.num_valid_rows, res.num_invalid_rows) == (1, 1)
    assert table_to_lists(res.valid_rows) == {"id": [5]}
    assert table_to_lists(res.invalid_rows) == {"id": ["x"]}
    # max_value alone decides the NULL row (:250 keeps colIsNull)
    res = RowLevelSchemaValidator.validate(data, RowLevelSchema().with_int_column("id", max_value=9))
    assert table_to_lists(res.valid_rows) == {"id": [5, None]}
    assert table_to_lists(res.invalid_rows) == {"id": ["x"]}


def test_unsupported_value_is_refused_not_guessed(gpu_device):
    from deequ_amd import RowLevelSchema, RowLevelSchemaValidator, SchemaValueNotSupported
    data = string_table({"t": ["2012-07-22 22:59:59", "2012-7-22 22:59:59", "N/A", "2012-07-22 1"],
                         "d": ["1", "1e10000", "x", "１"]}, gpu_device)
    with pytest.raises(SchemaValueNotSupported, match=r"column t: 2 value"):
        RowLevelSchemaValidator.validate(data, RowLevelSchema().with_timestamp_column("t", MASK))
    with pytest.raises(SchemaValueNotSupported, match=r"column d: 2 value"):
        RowLevelSchemaValidator.validate(data, RowLevelSchema().with_decimal_column("d", 5, 0))


# ------------------------------------------------------------------------------------------------
# randomised parity
# ------------------------------------------------------------------------------------------------
SCHEMA = [
    {"kind": "int", "name": "i", "min_value": -10, "max_value": 1000},
    {"kind": "string", "name": "s", "min_length": 1, "max_length": 12, "matches": "^[a-zé0-9 ]+$"},
    {"kind": "decimal", "name": "d", "precision": 10, "scale": 2},
    {"kind": "timestamp", "name": "t", "mask": MASK, "is_nullable": False},
]


class Pools:
    """Value pools per declared column (hand-derived cases + random strings), each value with its
    clause verdict and cast from the restatement; no value is UNSUPPORTED (checked here, on the
    CPU)."""

    def __init__(self):
        rng = random.Random(11)
        junk = ["".join(rng.choice("0123456789+-.eE xyz:") for _ in range(rng.randint(0, 24)))
                for _ in range(300)]
        raw = {
            "i": [t for t, _ in INT_CASES] + junk + [str(rng.randint(-40, 1300)) for _ in range(300)],
            "s": [None, "", "hello", "héllo wörld", "€€€€€€€€€€€€", "€€€€€€€€€€€€€", "Hello", "a" * 12,
                  "a" * 13, "x y z", "𝄞"] + junk + ["w%d" % rng.randint(0, 999) for _ in range(200)],
            "d": [t for t, _, _, _ in DECIMAL_CASES] + junk +
                 ["%d.%03d" % (rng.randint(-10**8, 10**8), rng.randint(0, 999)) for _ in range(300)],
            "t": [t for t, m, _ in TS_CASES if m == MASK] + junk + [None] +
                 ["%04d-%02d-%02d %02d:%02d:%02d" % (rng.randint(1583, 9999), rng.randint(1, 12),
                                                     rng.randint(1, 28), rng.randint(0, 23),
                                                     rng.randint(0, 59), rng.randint(0, 59))
                  for _ in range(300)],
        }
        self.values, self.verdict, self.cast = {}, {}, {}
        for d in SCHEMA:
            c = d["name"]
            vals, seen = [], set()
            for v in raw[c]:
                if v in seen:
                    continue
                seen.add(v)
                verdict = H.row_verdict([d], {c: v})
                if verdict == H.UNSUPPORTED:
                    continue
                vals.append(v)
                self.verdict[c, v] = verdict
                self.cast[c, v] = H.cast_value(d, v)
            self.values[c] = vals
        assert all(len(v) > 200 for v in self.values.values())
        assert any(v is None for v in self.verdict.values())  # the line-246 NULL verdict is drawn

    def rows(self, n, seed, mode="mixed"):
        rng = random.Random(seed)
        cols = {}
        for d in SCHEMA:
            c = d["name"]
            pool = self.values[c]
            if mode == "valid":
                pool = [v for v in pool if self.verdict[c, v] is True]
            elif mode == "invalid" and c == "t":
                pool = [v for v in pool if self.verdict[c, v] is False]
            elif mode == "mixed":  # most values pass, so whole rows do too
                good = [v for v in pool if self.verdict[c, v] is True]
                pool = good * 6 + pool + ([None] * 30 if c == "i" else [])  # (NULL verdicts)
            cols[c] = [rng.choice(pool) for _ in range(n)]
        return cols

    def expect(self, cols, extra):
        """(valid, invalid) of tests/schema_host.validate, from the per-value clause verdicts (the
        CNF is an AND over the columns' clauses, R/:226)."""
        names = list(cols) + list(extra)
        valid = {c: [] for c in names}
        invalid = {c: [] for c in names}
        n = len(cols["i"])
        for r in range(n):
            verdict = True
            for c in cols:
                verdict = H.k_and(verdict, self.verdict[c, cols[c][r]])
            if verdict is None:
                continue
            out = valid if verdict else invalid
            for c in cols:
                out[c].append(self.cast[c, cols[c][r]] if verdict else cols[c][r])
            for c in extra:
                out[c].append(extra[c][r])
        return valid, invalid


@pytest.fixture(scope="module")
def pools():
    return Pools()


def passthrough(n, seed, with_nulls=True):
    """Undeclared columns of every kind the gather handles."""
    import decimal

    import pyarrow as pa
    rng = random.Random(seed)

    def maybe(v):
        return None if with_nulls and rng.random() < 0.2 else v
    extra = {
        "p_i64": [maybe(rng.randint(-2**62, 2**62)) for _ in range(n)],
        "p_f64": [rng.random() * 1e6 - 5e5 for _ in range(n)],  # no validity buffer
        "p_bool": [maybe(rng.random() < 0.5) for _ in range(n)],
        "p_dec": [maybe(rng.randint(-10**19, 10**19)) for _ in range(n)],
        "p_i8": [maybe(rng.randint(-128, 127)) for _ in range(n)],
        "p_i16": [rng.randint(-2**15, 2**15 - 1) for _ in range(n)],
        "p_str": ["r%d" % rng.randint(0, 10**rng.randint(0, 9)) for _ in range(n)],  # no validity buffer
    }
    types = {"p_i64": pa.int64(), "p_f64": pa.float64(), "p_bool": pa.bool_(),
             "p_dec": pa.decimal128(20, 4), "p_i8": pa.int8(), "p_i16": pa.int16(),
             "p_str": pa.string()}
    arrow = dict(extra)
    arrow["p_dec"] = [None if v is None else decimal.Decimal(v).scaleb(-4) for v in extra["p_dec"]]
    return extra, arrow, types


def run_and_compare(pools, device, cols_per_batch, seed, with_nulls=True):
    from deequ_amd import RowLevelSchemaValidator
    from deequ_amd.table import Table
    tables, want = [], []
    for k, cols in enumerate(cols_per_batch):
        extra, arrow, types = passthrough(len(cols["i"]), seed + k, with_nulls)
        tables.append(string_table(cols, device, arrow, types))
        want.append(pools.expect(cols, extra))
    data = Table(tables[0].schema, [b for t in tables for b in t.batches], device)
    res = RowLevelSchemaValidator.validate(data, engine_schema(SCHEMA))
    assert len(res.valid_rows.batches) == len(res.invalid_rows.batches) == len(cols_per_batch)
    n_valid = n_invalid = 0
    for k, (wv, wi) in enumerate(want):
        gv = {c: column_to_list(b) for c, b in res.valid_rows.batches[k].items()}
        gi = {c: column_to_list(b) for c, b in res.invalid_rows.batches[k].items()}
        for c in wv:
            assert gv[c] == wv[c], (k, "valid", c)
            assert gi[c] == wi[c], (k, "invalid", c)
        assert list(gv) == list(wv) and list(gi) == list(wi)  # every column, in order
        n_valid += len(wv["i"])
        n_invalid += len(wi["i"])
    assert (res.num_valid_rows, res.num_invalid_rows) == (n_valid, n_invalid)
    # a column without a validity buffer yields none
    for t in (res.valid_rows, res.invalid_rows):
        assert all(b["p_f64"].validity is None and b["p_str"].validity is None for b in t.batches)
    return res, n_valid, n_invalid


def _tile():
    from deequ_amd import _native as N
    return N.SELECT_TILE_ROWS


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, "tile-1", "tile", "tile+1", 100_003])
def test_randomised_parity_with_the_restatement(gpu_device, pools, n):
    n = {"tile-1": _tile() - 1, "tile": _tile(), "tile+1": _tile() + 1}.get(n, n)
    _, n_valid, n_invalid = run_and_compare(pools, gpu_device, [pools.rows(n, seed=n)], seed=n)
    if n > 1000:  # all three verdicts occur
        assert n_valid > n // 10 and n_invalid > n // 10 and n_valid + n_invalid < n


@pytest.mark.parametrize("mode", ["valid", "invalid"])
def test_all_valid_and_none_valid_tables(gpu_device, pools, mode):
    n = 2 * _tile() + 77
    res, n_valid, n_invalid = run_and_compare(pools, gpu_device, [pools.rows(n, 5, mode)], seed=5)
    assert (n_valid, n_invalid) == ((n, 0) if mode == "valid" else (0, n))


def test_no_validity_buffers_at_all(gpu_device, pools):
    cols = pools.rows(3000, 21)
    for c in cols:  # no NULLs: Arrow delivers the columns without validity buffers
        stand = next(v for v in pools.values[c] if v is not None and pools.verdict[c, v] is True)
        cols[c] = [stand if v is None else v for v in cols[c]]
    run_and_compare(pools, gpu_device, [cols], seed=21, with_nulls=False)


def test_three_batches_of_unequal_length(gpu_device, pools):
    sizes = [_tile() + 5, 0, 1234]
    run_and_compare(pools, gpu_device, [pools.rows(n, 31 + k) for k, n in enumerate(sizes)], seed=31)


# ------------------------------------------------------------------------------------------------
# downstream use
# ------------------------------------------------------------------------------------------------
def test_analysis_runs_on_valid_rows(gpu_device):
    import datetime

    import pyarrow as pa
    from deequ_amd import Analysis, RowLevelSchemaValidator
    from deequ_amd.analyzers import Completeness, Maximum, Size
    from deequ_amd.table import Table
    case = H.load_known_answers()[6]
    schema = [dict(d) for d in case["schema"]]
    schema[1] = {"kind": "string", "name": "name"}  # keep more rows: 123, 456, 789, 101
    res = RowLevelSchemaValidator.validate(string_table(case["columns"], gpu_device),
                                           engine_schema(schema))
    ts = datetime.datetime(2012, 7, 22, 22, 59, 59)
    hand = Table.from_pydict(
        {"id": [123, 456, 789, 101],
         "name": ["Product A", "Product D, a must buy", "Product D, another must buy", "Product E"],
         "event_time": [ts, ts, ts, ts]},
        {"id": pa.int32(), "name": pa.string(), "event_time": pa.timestamp("us")}, device=gpu_device)
    assert table_to_lists(res.valid_rows) == table_to_lists(hand)
    suite = [Size(), Completeness("event_time"), Completeness("name"), Maximum("id")]
    got, want = Analysis(suite).run(res.valid_rows), Analysis(suite).run(hand)
    for a in suite:
        assert got.metric(a).value.get() == want.metric(a).value.get(), str(a)
    assert got.metric(Size()).value.get() == 4.0 and got.metric(Maximum("id")).value.get() == 789.0


# ------------------------------------------------------------------------------------------------
# the selection primitive through the ABI alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["ones", "zeros", "alternating", "last"])
def test_select_and_gather_through_the_abi(gpu_device, pattern):
    import pyarrow as pa
    import torch
    from deequ_amd import _native as N
    from deequ_amd.table import Table
    n = _tile() + 70  # two tiles, the second one a partial word
    rng = random.Random(3)
    strs = [None if rng.random() < 0.1 else "v%d" % rng.randint(0, 10**rng.randint(0, 12)) for _ in range(n)]
    flags = [None if rng.random() < 0.1 else rng.random() < 0.5 for _ in range(n)]
    t = Table.from_pydict({"s": strs, "b": flags}, {"s": pa.string(), "b": pa.bool_()}, device=gpu_device)
    cs, cb = t.batches[0]["s"], t.batches[0]["b"]
    keep = {"ones": [True] * n, "zeros": [False] * n, "alternating": [r % 2 == 1 for r in range(n)],
            "last": [r == n - 1 for r in range(n)]}[pattern]
    bits = np.packbits(np.array(keep + [True] * (-n % 64), bool), bitorder="little")  # tail bits set:
    bitmap = torch.from_numpy(bits).to(gpu_device)                                    # they are ignored
    rows = [r for r in range(n) if keep[r]]
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)

    index = torch.full((max(1, len(rows)),), -1, dtype=torch.int32, device=gpu_device)
    n_sel = ctypes.c_int64()
    nbytes = (ctypes.c_int64 * 1)()
    ccols = (N.dq_column * 1)(cs.to_c())
    N.check(N.lib.dq_select_plan(bitmap.data_ptr(), n, index.data_ptr(), len(rows), ctypes.byref(n_sel),
                                 ccols, 1, nbytes, stream))
    assert n_sel.value == len(rows)
    assert index.cpu().tolist()[:len(rows)] == rows
    need = nbytes[0]
    assert need == sum(len(strs[r].encode()) for r in rows if strs[r] is not None)
    if rows:  # an index list one entry short is refused with the count, nothing written
        short = torch.full((len(rows),), -1, dtype=torch.int32, device=gpu_device)
        st = N.lib.dq_select_plan(bitmap.data_ptr(), n, short.data_ptr(), len(rows) - 1,
                                  ctypes.byref(n_sel), ccols, 1, (ctypes.c_int64 * 1)(), stream)
        assert st == N.ERR_INVALID_ARGUMENT and n_sel.value == len(rows)
        assert short.cpu().tolist() == [-1] * len(rows)

    m = len(rows)
    for col, src in ((cs, strs), (cb, flags)):
        out_validity = torch.zeros((m + 63) // 64 * 8 + 16, dtype=torch.uint8, device=gpu_device)
        if col.dtype == N.UTF8:
            out_values = torch.full((m + 1 + 4,), -1, dtype=torch.int32, device=gpu_device)
            out_data = torch.zeros(need + 16, dtype=torch.uint8, device=gpu_device)
        else:
            out_values = torch.zeros((m + 63) // 64 * 8 + 16, dtype=torch.uint8, device=gpu_device)
            out_data = None
        cin, cout = col.to_c(), N.dq_column()
        cout.type, cout.validity, cout.values = col.dtype, out_validity.data_ptr(), out_values.data_ptr()
        if out_data is not None:
            cout.data, cout.data_bytes = out_data.data_ptr(), need
        N.check(N.lib.dq_gather_column(ctypes.byref(cin), index.data_ptr(), m, ctypes.byref(cout), stream))
        assert cout.length == m
        from deequ_amd.table import ColumnBatch
        got = column_to_list(ColumnBatch(col.dtype, m, out_validity, out_values, out_data, 0))
        assert got == [src[r] for r in rows]
        if col.dtype == N.UTF8:
            assert cout.data_bytes == need
            assert out_values.cpu().tolist()[m + 1:] == [-1] * 4  # nothing past the m + 1 offsets
            if need:  # a data buffer one byte short is refused
                cout.data_bytes = need - 1
                assert N.lib.dq_gather_column(ctypes.byref(cin), index.data_ptr(), m, ctypes.byref(cout),
                                              stream) == N.ERR_INVALID_ARGUMENT
