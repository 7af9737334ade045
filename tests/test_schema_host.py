"""CPU tests of the row-level schema validator's semantics: the plain-Python restatement
(tests/schema_host.py) reproduces the reference's seven tests, hand-derived cast / length /
timestamp cases, and the refusals that need no device (schema.py's checks run before any device
work)."""
import pytest

import schema_host as H

U = H.UNSUPPORTED


@pytest.mark.parametrize("case", H.load_known_answers(), ids=lambda c: c["name"])
def test_restatement_reproduces_the_reference_tests(case):
    valid, invalid = H.validate(case["schema"], case["columns"])
    first = next(iter(case["columns"]))
    H.assert_known_answer(case, valid, invalid, len(valid[first]), len(invalid[first]))


# derived by hand from UTF8String.toInt (Spark 2.2): sign, digits, '.' + digits truncated, no trim
INT_CASES = [("1.9", 1), ("+", None), ("-", None), ("", None), ("2147483648", None),
             ("2147483647", 2147483647), ("-2147483648", -2147483648), ("-2147483649", None),
             (" 1", None), ("1 ", None), ("+7", 7), ("-0", 0), ("1.", 1), (".", 0), ("1.2.3", None),
             ("1e2", None), ("0000000000000012", 12), ("١٢", None), (None, None)]


@pytest.mark.parametrize("text,expected", INT_CASES)
def test_int_cast(text, expected):
    assert H.cast_int(text) == expected


# derived by hand from BigDecimal(String) + setScale(s, HALF_UP) + the 10^p bound
DECIMAL_CASES = [("99.995", 4, 2, None), ("99.994", 4, 2, 9999), ("-0.005", 3, 2, -1),
                 ("-0.004", 3, 2, 0), (".5", 3, 1, 5), ("1.", 3, 1, 10), ("1e2", 5, 1, 1000),
                 ("1E-3", 5, 3, 1), ("1E-3", 5, 2, 0), ("5E-3", 5, 2, 1), (".", 5, 2, None),
                 ("1_0", 5, 2, None), (" 1", 5, 2, None), ("NaN", 5, 2, None), ("", 5, 2, None),
                 ("+", 5, 2, None), ("1e", 5, 2, None), ("1e+", 5, 2, None), ("e5", 5, 2, None),
                 ("9" * 39, 38, 0, None), ("9" * 38, 38, 0, 10**38 - 1),
                 ("0" * 40 + "7", 38, 0, 7), ("9" * 38 + ".5", 38, 0, None),
                 ("-" + "9" * 38 + ".4", 38, 0, -(10**38 - 1)), ("1e37", 38, 0, 10**37),
                 ("1e38", 38, 0, None), ("1e-9999", 38, 38, 0), ("1e9999", 38, 0, None),
                 ("1e10000", 38, 0, U), ("1e00001", 38, 0, U), ("１", 5, 0, U), ("1é", 5, 0, U),
                 ("299.000", 10, 2, 29900), ("+.5e1", 4, 2, 500), ("0.000", 1, 1, 0),
                 (None, 5, 2, None)]


@pytest.mark.parametrize("text,p,s,expected", DECIMAL_CASES)
def test_decimal_cast(text, p, s, expected):
    assert H.cast_decimal(text, p, s) == expected


def test_character_length_of_a_multi_byte_string():
    s = "héllo wörld €𝄞"  # 14 characters in 21 bytes
    assert len(s.encode("utf-8")) == 21
    assert H.char_length(s) == 14
    schema = [{"kind": "string", "name": "c", "max_length": 14, "min_length": 14}]
    valid, invalid = H.validate(schema, {"c": [s, s + "x", s[1:]]})
    assert valid["c"] == [s] and invalid["c"] == [s + "x", s[1:]]


MASK = "yyyy-MM-dd HH:mm:ss"
TS_CASES = [
    ("2012-07-22 22:59:59", MASK, 1342997999000000),  # accept: 15543 days + 82799 s
    ("1970-01-01 00:00:00", MASK, 0),
    ("2000-02-29 00:00:01", MASK, 951782401000000),
    ("N/A", MASK, None),                # a letter at a numeric field: definite NULL
    ("yesterday night", MASK, None),
    ("", MASK, None),                   # the text has ended at a field
    ("2012-07", MASK, None),            # the text has ended at a literal
    ("2012/07/22 22:59:59", MASK, None),  # a literal differs, neither byte blank
    ("2012-7-22 22:59:59", MASK, U),    # too few digits
    ("02012-07-22 22:59:59", MASK, U),  # a fifth digit: the lenient year would take it
    ("2012-07-22 22:59:599", MASK, U),  # too many digits
    ("2012-13-22 22:59:59", MASK, U),   # rolls over in lenient mode
    ("2011-02-29 00:00:00", MASK, U),
    ("2012-07-22 22:59:59 ", MASK, U),  # trailing text
    ("1582-07-22 22:59:59", MASK, U),   # before the Gregorian cutover year
    ("-012-07-22 22:59:59", MASK, U),   # a sign
    ("2012-07-22  2:59:59", MASK, U),   # a blank at a numeric field
    ("2012-07-22T22:59:59", MASK, U),   # a blank literal against another byte
    ("2012-13-22 22:59:xx", MASK, None),  # out of range, then a definite failure
    ("20120722", "yyyyMMdd", 1342915200000000),
    ("201207221", "yyyyMMdd", U),
    ("2012-07-22T22:59", "yyyy-MM-dd'T'HH:mm", 1342997940000000),
    ("12 o'clock 2012", "HH 'o''clock' yyyy", (15340 * 86400 + 12 * 3600) * 1000000),
]


@pytest.mark.parametrize("text,mask,expected", TS_CASES)
def test_timestamp_three_way(text, mask, expected):
    assert H.parse_ts(text, mask) == expected


BAD_MASKS = ["yyyy-MM-dd hh:mm:ss", "yy-MM-dd", "yyyy-MMM-dd", "yyyy-MM-dd HH:mm:ss.SSS",
             "yyyy-MM-dd'T", "yyyy-MM-yyyy", "--", "", "yyyy0MM", "yyyy→MM", "yyyy-MM-dd Z"]


@pytest.mark.parametrize("mask", BAD_MASKS)
def test_masks_outside_the_grammar_are_refused(mask):
    from deequ_amd.schema import compile_mask
    with pytest.raises(ValueError):
        H.compile_mask(mask)
    with pytest.raises(ValueError):
        compile_mask(mask)


@pytest.mark.parametrize("mask", [MASK, "yyyyMMdd", "HH 'o''clock' yyyy", "dd.MM.yyyy", "''yyyy"])
def test_engine_mask_tokens_agree_with_the_restatement(mask):
    from deequ_amd.schema import compile_mask
    kinds = {"Y": 1, "M": 2, "D": 3, "h": 4, "m": 5, "s": 6}
    want = [(0, ord(a)) if k == "lit" else (kinds[k], a) for k, a in H.compile_mask(mask)]
    assert compile_mask(mask) == want


def test_null_verdict_of_line_246_in_the_restatement():
    """Derived by reading RowLevelSchemaValidator.scala:246 (`colIsNull.isNull`): a NULL in a
    nullable int column with a min_value gives a NULL verdict; the reference's tests do not
    reach it."""
    schema = [{"kind": "int", "name": "id", "min_value": 0}]
    assert [H.row_verdict(schema, {"id": v}) for v in ["5", None, "x", "-1"]] == \
        [True, None, False, False]
    valid, invalid = H.validate(schema, {"id": ["5", None, "x"]})
    assert valid["id"] == [5] and invalid["id"] == ["x"]
    # with max_value only, or not nullable, the NULL row is decided
    assert H.row_verdict([{"kind": "int", "name": "id", "max_value": 9}], {"id": None}) is True
    assert H.row_verdict([{"kind": "int", "name": "id", "min_value": 0, "is_nullable": False}],
                         {"id": None}) is False


# ------------------------------------------------------------------------------------------------
# validate()'s refusals: raised before any device work, so a hand-built Table without buffers does
# ------------------------------------------------------------------------------------------------
def _table(fields, rows=3):
    from deequ_amd.table import ColumnBatch, StructField, StructType, Table
    from deequ_amd import _native as N
    fs = [StructField(n, t, arrow_type="list<int32>" if t == N.UNSUPPORTED else None)
          for n, t in fields]
    batch = {n: ColumnBatch(N.INT8 if t == N.UNSUPPORTED else t, rows, None, None, None, 0,
                            stand_in=t == N.UNSUPPORTED) for n, t in fields}
    return Table(StructType(fs), [batch], "cuda:0")


def _refused(table, schema, needle):
    from deequ_amd import RowLevelSchemaValidator
    with pytest.raises(ValueError) as e:
        RowLevelSchemaValidator.validate(table, schema)
    assert needle in str(e.value), str(e.value)


def test_validate_refusals_name_the_column():
    from deequ_amd import RowLevelSchema
    from deequ_amd import _native as N
    from deequ_amd.regex import PatternNotSupported
    t = _table([("id", N.UTF8), ("n", N.INT64), ("s", N.UTF8)])
    _refused(t, RowLevelSchema().with_int_column("nope"), "nope")
    _refused(t, RowLevelSchema().with_int_column("n"), "n is LongType")
    _refused(t, RowLevelSchema().with_int_column("id").with_string_column("id"), "id is declared twice")
    for p, s in [(0, 0), (39, 0), (5, 6), (5, -1)]:
        _refused(t, RowLevelSchema().with_decimal_column("id", p, s), "id")
    _refused(t, RowLevelSchema().with_timestamp_column("s", "yyyy-MM-dd hh"), "column s")
    _refused(_table([("id", N.UTF8)], rows=2**31), RowLevelSchema().with_int_column("id"), "id")
    _refused(_table([("id", N.UTF8), ("l", N.UNSUPPORTED)]), RowLevelSchema().with_int_column("id"),
             "column l")
    from deequ_amd import RowLevelSchemaValidator
    with pytest.raises(PatternNotSupported):
        RowLevelSchemaValidator.validate(t, RowLevelSchema().with_string_column("s", matches="(a*)*\\1"))


def test_schema_builder_is_immutable():
    from deequ_amd import RowLevelSchema
    a = RowLevelSchema()
    b = a.with_int_column("x", min_value=1)
    c = b.with_decimal_column("y", 10, 2, is_nullable=False)
    assert a.column_definitions == () and len(b.column_definitions) == 1
    assert [d.name for d in c.column_definitions] == ["x", "y"]
    assert c.column_definitions[1].precision == 10 and not c.column_definitions[1].is_nullable
    with pytest.raises(Exception):
        b.column_definitions = ()


def test_abi_status_codes_need_no_device():
    """dq_schema_evaluate / dq_select_plan / dq_gather_column answer a bad argument, a batch over
    2^31-1 rows and an automaton over 255 states with a status code before any device work."""
    import ctypes
    import struct

    from deequ_amd import _native as N
    col = N.dq_column()
    col.type, col.length = N.UTF8, 2**31
    cols = (N.dq_column * 1)(col)
    d = (N.dq_schema_column * 1)()
    d[0].kind, d[0].column, d[0].is_nullable = N.SCHEMA_STRING, 0, 1
    nv, ni, bad = ctypes.c_int64(), ctypes.c_int64(), (ctypes.c_int64 * 1)()

    def evaluate(rows):
        return N.lib.dq_schema_evaluate(d, 1, cols, 1, rows, None, None, ctypes.byref(nv),
                                        ctypes.byref(ni), bad, None)
    assert evaluate(2**31) == N.ERR_UNSUPPORTED and b"2^31-1" in N.lib.dq_last_error()
    assert evaluate(-1) == N.ERR_INVALID_ARGUMENT
    cols[0].length = 5
    assert evaluate(4) == N.ERR_INVALID_ARGUMENT  # the column has another row count
    d[0].column = 1
    assert evaluate(5) == N.ERR_NO_SUCH_COLUMN
    d[0].column = 0
    cols[0].type = N.INT64
    assert evaluate(5) == N.ERR_WRONG_TYPE
    cols[0].type, cols[0].length = N.UTF8, 0
    blob = ctypes.create_string_buffer(struct.pack("<4i", 300, 2, 0, 0) + bytes(256 + 300 + 1200), 1772)
    d[0].regex, d[0].regex_bytes = ctypes.addressof(blob), 1772
    assert evaluate(0) == N.ERR_UNSUPPORTED and b"300 states" in N.lib.dq_last_error()
    d[0].regex = None
    d[0].kind, d[0].precision, d[0].scale = N.SCHEMA_DECIMAL, 39, 0
    assert evaluate(0) == N.ERR_INVALID_ARGUMENT
    d[0].kind = N.SCHEMA_TIMESTAMP
    mask = ctypes.create_string_buffer(bytes([1, 4, 1, 4]), 4)  # yyyy twice
    d[0].mask, d[0].mask_tokens = ctypes.addressof(mask), 2
    assert evaluate(0) == N.ERR_INVALID_ARGUMENT
    d[0].mask_tokens = 1
    assert evaluate(0) == N.DQ_OK and (nv.value, ni.value) == (0, 0)

    n_sel = ctypes.c_int64()
    assert N.lib.dq_select_plan(None, 2**31, None, 0, ctypes.byref(n_sel), None, 0, None,
                                None) == N.ERR_UNSUPPORTED
    assert N.lib.dq_select_plan(None, -1, None, 0, ctypes.byref(n_sel), None, 0, None,
                                None) == N.ERR_INVALID_ARGUMENT
    assert N.lib.dq_select_plan(None, 0, None, 0, ctypes.byref(n_sel), None, 0, None, None) == N.DQ_OK
    out = N.dq_column()
    out.type = N.INT32
    col.type, col.length = N.INT64, 4
    assert N.lib.dq_gather_column(ctypes.byref(col), None, 2**31, ctypes.byref(out), None) == N.ERR_UNSUPPORTED
    assert N.lib.dq_gather_column(ctypes.byref(col), None, 1, ctypes.byref(out), None) == N.ERR_WRONG_TYPE
    assert N.lib.dq_gather_column(ctypes.byref(col), None, -1, ctypes.byref(out), None) == N.ERR_INVALID_ARGUMENT
