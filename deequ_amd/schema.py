"""RowLevelSchemaValidator (schema/RowLevelSchemaValidator.scala): a table of string columns is
checked row by row against a declared schema; the conforming rows come back cast to the declared
types, the non-conforming rows as they came, with both counts.

The verdict, the casts and the row selection run on the device (csrc/rowschema.hip behind
dq_schema_evaluate / dq_select_plan / dq_gather_column); this module builds the schema, refuses
what the engine does not decide, and assembles the two result tables from gathered buffers.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Tuple

from . import _native as N
from .regex import compile_java_regex

MAX_BATCH_ROWS = 2**31 - 1
_MAX_MASK_TOKENS = 48
# mask letters the engine reads: run -> (dq_schema_column.mask kind, width)
_MASK_FIELDS = {"yyyy": (1, 4), "MM": (2, 2), "dd": (3, 2), "HH": (4, 2), "mm": (5, 2), "ss": (6, 2)}


class SchemaValueNotSupported(NotImplementedError):
    """A declared column holds values whose outcome under Java this engine does not decide (a
    lenient SimpleDateFormat form, a decimal string with non-ASCII bytes or a long exponent)."""


def compile_mask(mask: str) -> List[Tuple[int, int]]:
    """A SimpleDateFormat mask as (kind, value) tokens: (0, byte) for a literal, (k, width) for the
    numeric field k of _MASK_FIELDS.  Supported: the runs yyyy MM dd HH mm ss, each at most once;
    non-letter ASCII literals except digits (the lenient number parse before them would swallow
    a digit); 'quoted' literals with '' as the quote.  Anything else raises ValueError."""
    tokens: List[Tuple[int, int]] = []
    seen = set()
    i, n = 0, len(mask)

    def literal(ch: str) -> None:
        if ord(ch) >= 0x80 or ch.isdigit():
            raise ValueError(f"timestamp mask {mask!r}: literal {ch!r} is not supported "
                             "(ASCII and no digit)")
        tokens.append((0, ord(ch)))

    while i < n:
        ch = mask[i]
        if ch == "'":
            if i + 1 < n and mask[i + 1] == "'":
                literal("'")
                i += 2
                continue
            i += 1
            while True:
                if i >= n:
                    raise ValueError(f"timestamp mask {mask!r}: unterminated quote")
                if mask[i] == "'":
                    if i + 1 < n and mask[i + 1] == "'":
                        literal("'")
                        i += 2
                        continue
                    i += 1
                    break
                literal(mask[i])
                i += 1
        elif ch.isascii() and ch.isalpha():
            j = i
            while j < n and mask[j] == ch:
                j += 1
            run = mask[i:j]
            if run not in _MASK_FIELDS:
                raise ValueError(f"timestamp mask {mask!r}: field {run!r} is not supported "
                                 f"(only {', '.join(_MASK_FIELDS)})")
            if run in seen:
                raise ValueError(f"timestamp mask {mask!r}: field {run!r} appears twice")
            seen.add(run)
            tokens.append(_MASK_FIELDS[run])
            i = j
        else:
            literal(ch)
            i += 1
    if not seen:
        raise ValueError(f"timestamp mask {mask!r}: no field")
    if len(tokens) > _MAX_MASK_TOKENS:
        raise ValueError(f"timestamp mask {mask!r}: more than {_MAX_MASK_TOKENS} tokens")
    return tokens


@dataclass(frozen=True)
class ColumnDefinition:
    name: str
    is_nullable: bool = True


@dataclass(frozen=True)
class StringColumnDefinition(ColumnDefinition):
    min_length: Optional[int] = None
    max_length: Optional[int] = None
    matches: Optional[str] = None


@dataclass(frozen=True)
class IntColumnDefinition(ColumnDefinition):
    min_value: Optional[int] = None
    max_value: Optional[int] = None


@dataclass(frozen=True)
class DecimalColumnDefinition(ColumnDefinition):
    precision: int = 10
    scale: int = 0


@dataclass(frozen=True)
class TimestampColumnDefinition(ColumnDefinition):
    mask: str = ""


@dataclass(frozen=True)
class RowLevelSchema:
    """RowLevelSchema (RowLevelSchemaValidator.scala:73-151): an immutable builder."""
    column_definitions: Tuple[ColumnDefinition, ...] = ()

    def _with(self, d: ColumnDefinition) -> "RowLevelSchema":
        return RowLevelSchema(self.column_definitions + (d,))

    def with_string_column(self, name: str, is_nullable: bool = True,
                           min_length: Optional[int] = None, max_length: Optional[int] = None,
                           matches: Optional[str] = None) -> "RowLevelSchema":
        return self._with(StringColumnDefinition(name, is_nullable, min_length, max_length, matches))

    def with_int_column(self, name: str, is_nullable: bool = True,
                        min_value: Optional[int] = None,
                        max_value: Optional[int] = None) -> "RowLevelSchema":
        return self._with(IntColumnDefinition(name, is_nullable, min_value, max_value))

    def with_decimal_column(self, name: str, precision: int, scale: int,
                            is_nullable: bool = True) -> "RowLevelSchema":
        return self._with(DecimalColumnDefinition(name, is_nullable, precision, scale))

    def with_timestamp_column(self, name: str, mask: str,
                              is_nullable: bool = True) -> "RowLevelSchema":
        return self._with(TimestampColumnDefinition(name, is_nullable, mask))


@dataclass
class RowLevelSchemaValidationResult:
    """RowLevelSchemaValidator.scala:161-166."""
    valid_rows: object  # Table
    num_valid_rows: int
    invalid_rows: object  # Table
    num_invalid_rows: int


def _int32(name: str, what: str, v: Optional[int]) -> int:
    if v is None:
        return 0
    if not -2**31 <= int(v) < 2**31:
        raise ValueError(f"column {name}: {what} {v} is not an Int")
    return int(v)


def cast_type(d: ColumnDefinition) -> int:
    """The type word of a declared column in valid_rows (castExpression, :29, :47, :57, :66-68)."""
    if isinstance(d, IntColumnDefinition):
        return N.INT32
    if isinstance(d, DecimalColumnDefinition):
        return N.decimal_type(d.precision, d.scale)
    if isinstance(d, TimestampColumnDefinition):
        return N.TIMESTAMP_US
    return N.UTF8


def check_schema(schema: RowLevelSchema, fields) -> list:
    """The refusals that need no data: per definition (index into `fields`, compiled regex blob or
    None, mask tokens or None).  `fields` are the table's StructFields."""
    names = [f.name for f in fields]
    out, seen = [], set()
    for d in schema.column_definitions:
        if d.name in seen:
            raise ValueError(f"column {d.name} is declared twice")
        seen.add(d.name)
        if d.name not in names:
            raise ValueError(f"column {d.name} is declared but the data has no such column")
        f = fields[names.index(d.name)]
        if f.dtype != N.UTF8 or f.type_name != "StringType":
            raise ValueError(f"column {d.name} is {f.type_name}: a declared column must be StringType")
        blob = tokens = None
        if isinstance(d, DecimalColumnDefinition):
            if not (isinstance(d.precision, int) and isinstance(d.scale, int)
                    and 1 <= d.precision <= 38 and 0 <= d.scale <= d.precision):
                raise ValueError(f"column {d.name}: decimal({d.precision},{d.scale}) is outside "
                                 "1 <= p <= 38, 0 <= s <= p")
        elif isinstance(d, TimestampColumnDefinition):
            try:
                tokens = compile_mask(d.mask)
            except ValueError as e:
                raise ValueError(f"column {d.name}: {e}") from None
        elif isinstance(d, StringColumnDefinition):
            _int32(d.name, "min_length", d.min_length)
            _int32(d.name, "max_length", d.max_length)
            if d.matches is not None:
                rx = compile_java_regex(d.matches)  # PatternNotSupported is a ValueError
                if rx.n_states > 255:
                    raise ValueError(f"column {d.name}: the automaton of /{d.matches}/ has "
                                     f"{rx.n_states} states (at most 255)")
                blob = rx.blob()
        elif isinstance(d, IntColumnDefinition):
            _int32(d.name, "min_value", d.min_value)
            _int32(d.name, "max_value", d.max_value)
        out.append((names.index(d.name), blob, tokens))
    for f in fields:
        if f.dtype == N.UNSUPPORTED:
            raise ValueError(f"column {f.name} is {f.type_name}: its rows cannot be selected")
    return out


_CAST_WIDTH = {N.INT32: 4, N.TIMESTAMP_US: 8}


def _alloc(nbytes: int, device, dtype=None):
    """nbytes of device memory, zero-padded to a multiple of 16 bytes (+16) like table.py's buffers."""
    import torch
    padded = (nbytes + 15) // 16 * 16 + 16
    t = N.retry_on_oom(torch.empty, padded, dtype=torch.uint8, device=device)
    t[nbytes:].zero_()
    return t if dtype is None else t.view(dtype)


def _torch_dtype(dtype: int):
    import torch
    tid = N.type_id(dtype)
    return {N.BOOL: torch.uint8, N.INT8: torch.int8, N.INT16: torch.int16, N.INT32: torch.int32,
            N.INT64: torch.int64, N.FLOAT32: torch.float32, N.FLOAT64: torch.float64,
            N.UTF8: torch.int32, N.DECIMAL128: torch.uint64, N.DATE32: torch.int32,
            N.TIMESTAMP_US: torch.int64}[tid]


def _value_bytes(dtype: int, n: int) -> int:
    tid = N.type_id(dtype)
    if tid == N.BOOL:
        return (n + 63) // 64 * 8
    if tid == N.UTF8:
        return 4 * (n + 1)
    return n * {N.INT8: 1, N.INT16: 2, N.INT32: 4, N.INT64: 8, N.FLOAT32: 4, N.FLOAT64: 8,
                N.DECIMAL128: 16, N.DATE32: 4, N.TIMESTAMP_US: 8}[tid]


def gather_column(col, index, n_out: int, data_bytes: int, device, stream):
    """dq_gather_column of one ColumnBatch into freshly allocated buffers."""
    from .table import ColumnBatch
    validity = _alloc((n_out + 63) // 64 * 8, device) if col.validity is not None else None
    values = _alloc(_value_bytes(col.dtype, n_out), device, _torch_dtype(col.dtype))
    data = _alloc(data_bytes, device) if N.type_id(col.dtype) == N.UTF8 else None
    out = ColumnBatch(col.dtype, n_out, validity, values, data, 0)
    cin, cout = col.to_c(), out.to_c()
    cout.data_bytes = data_bytes
    N.check(N.lib.dq_gather_column(ctypes.byref(cin), index.data_ptr() if index is not None else None,
                                   n_out, ctypes.byref(cout), stream))
    return out


def select_plan(bitmap, rows: int, utf8_cols, device, stream, capacity: Optional[int] = None):
    """dq_select_plan: (index tensor or None, n_selected, [bytes per utf8 column])."""
    import torch
    capacity = rows if capacity is None else capacity
    index = N.retry_on_oom(torch.empty, max(capacity, 1), dtype=torch.int32, device=device)
    n_sel = ctypes.c_int64()
    ccols = (N.dq_column * max(1, len(utf8_cols)))(*[c.to_c() for c in utf8_cols])
    nbytes = (ctypes.c_int64 * max(1, len(utf8_cols)))()
    N.check(N.lib.dq_select_plan(bitmap.data_ptr(), rows, index.data_ptr(), capacity,
                                 ctypes.byref(n_sel), ccols, len(utf8_cols), nbytes, stream))
    return index, n_sel.value, list(nbytes)[:len(utf8_cols)]


class RowLevelSchemaValidator:
    """RowLevelSchemaValidator.scala:169-282."""

    @staticmethod
    def validate(data, schema: RowLevelSchema, stage_timer=None) -> RowLevelSchemaValidationResult:
        """stage_timer (tools/bench_schema.py): a callable name -> context manager entered around
        each device stage (evaluate, select, gather)."""
        import contextlib

        import torch
        timer = stage_timer or (lambda name: contextlib.nullcontext())
        from .table import ColumnBatch, StructField, StructType, Table
        fields = data.schema.fields
        compiled = check_schema(schema, fields)
        defs = schema.column_definitions
        for b in data.batches:
            for f in fields:
                if b[f.name].stand_in:
                    raise ValueError(f"column {f.name} is {f.type_name}: its rows cannot be selected")
                if b[f.name].length > MAX_BATCH_ROWS:
                    raise ValueError(f"column {f.name}: a batch of {b[f.name].length} rows "
                                     f"(at most {MAX_BATCH_ROWS})")
        device = data.device
        casts = {d.name: cast_type(d) for d in defs}
        valid_fields = [StructField(f.name, casts.get(f.name, f.dtype),
                                    None if f.name in casts else f.spark_name) for f in fields]
        valid_batches, invalid_batches = [], []
        n_valid_total = n_invalid_total = 0
        with torch.cuda.device(device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            for b in data.batches:
                rows = b[fields[0].name].length if fields else 0
                words = (rows + 63) // 64
                cols = [b[f.name] for f in fields]
                ccols = (N.dq_column * max(1, len(cols)))(*[c.to_c() for c in cols])
                cdefs = (N.dq_schema_column * max(1, len(defs)))()
                keep = []  # host buffers the struct array points to
                staging = {}
                for k, (d, (ci, blob, tokens)) in enumerate(zip(defs, compiled)):
                    c = cdefs[k]
                    c.column, c.is_nullable = ci, 1 if d.is_nullable else 0
                    if isinstance(d, StringColumnDefinition):
                        c.kind = N.SCHEMA_STRING
                        c.has_min, c.min_value = d.min_length is not None, d.min_length or 0
                        c.has_max, c.max_value = d.max_length is not None, d.max_length or 0
                        if blob is not None:
                            buf = ctypes.create_string_buffer(blob, len(blob))
                            keep.append(buf)
                            c.regex, c.regex_bytes = ctypes.addressof(buf), len(blob)
                        continue
                    t = casts[d.name]
                    if isinstance(d, IntColumnDefinition):
                        c.kind = N.SCHEMA_INT
                        c.has_min, c.min_value = d.min_value is not None, d.min_value or 0
                        c.has_max, c.max_value = d.max_value is not None, d.max_value or 0
                    elif isinstance(d, DecimalColumnDefinition):
                        c.kind, c.precision, c.scale = N.SCHEMA_DECIMAL, d.precision, d.scale
                    else:
                        c.kind = N.SCHEMA_TIMESTAMP
                        flat = bytes(x for tok in tokens for x in tok)
                        buf = ctypes.create_string_buffer(flat, len(flat))
                        keep.append(buf)
                        c.mask, c.mask_tokens = ctypes.addressof(buf), len(tokens)
                    vals = _alloc(_value_bytes(t, rows), device, _torch_dtype(t))
                    vld = _alloc(words * 8, device)
                    c.cast_values, c.cast_validity = vals.data_ptr(), vld.data_ptr()
                    staging[d.name] = ColumnBatch(t, rows, vld, vals, None, 0)
                valid_bm = _alloc(words * 8, device)
                invalid_bm = _alloc(words * 8, device)
                n_valid, n_invalid = ctypes.c_int64(), ctypes.c_int64()
                bad = (ctypes.c_int64 * max(1, len(defs)))()
                with timer("evaluate"):
                    N.check(N.lib.dq_schema_evaluate(cdefs, len(defs), ccols, len(cols), rows,
                                                     valid_bm.data_ptr(), invalid_bm.data_ptr(),
                                                     ctypes.byref(n_valid), ctypes.byref(n_invalid),
                                                     bad, stream))
                for d, nb in zip(defs, list(bad)):
                    if nb:
                        raise SchemaValueNotSupported(
                            f"column {d.name}: {nb} value(s) in a form this build does not decide "
                            "(a timestamp outside the mask's strict form that SimpleDateFormat's "
                            "lenient parse may still read, or a decimal string with non-ASCII "
                            "bytes or an exponent of more than 4 digits)")
                n_valid_total += n_valid.value
                n_invalid_total += n_invalid.value
                for bitmap, count, source, sink in (
                        (valid_bm, n_valid.value, [staging.get(f.name, b[f.name]) for f in fields],
                         valid_batches),
                        (invalid_bm, n_invalid.value, cols, invalid_batches)):
                    utf8 = [c for c in source if N.type_id(c.dtype) == N.UTF8]
                    with timer("select"):
                        index, n_sel, nbytes = select_plan(bitmap, rows, utf8, device, stream, count)
                    assert n_sel == count, (n_sel, count)
                    sizes = iter(nbytes)
                    with timer("gather"):
                        sink.append({f.name: gather_column(
                            c, index, n_sel, next(sizes) if N.type_id(c.dtype) == N.UTF8 else 0,
                            device, stream) for f, c in zip(fields, source)})
        if not data.batches:
            valid_batches = Table(StructType(valid_fields), [], device).select_rows(0, 0).batches
            invalid_batches = Table(data.schema, [], device).select_rows(0, 0).batches
        return RowLevelSchemaValidationResult(
            Table(StructType(valid_fields), valid_batches, device), n_valid_total,
            Table(data.schema, invalid_batches, device), n_invalid_total)
