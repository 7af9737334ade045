"""Dictionary-encoded Arrow columns at the boundary, without a GPU: Table.from_arrow(device="cpu")
imports dictionary<I, V> as the decoded column (same schema, same buffers as the decoded input),
the host-fed tables refuse it by name, and the two new entry points are part of the ABI."""
import decimal
import os

import numpy as np
import pyarrow as pa
import pytest

from deequ_amd import _native as N
from deequ_amd.loader import HostTable
from deequ_amd.table import Table, arrow_field_type

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dictionary_table():
    D = decimal.Decimal
    cols = {
        "s": pa.DictionaryArray.from_arrays(pa.array([0, 1, None, 2, 1, 0, 3], pa.int8()),
                                            pa.array(["high", "low", None, ""])),
        "i": pa.DictionaryArray.from_arrays(pa.array([2, 2, 0, None, 1, 0, 1], pa.int16()),
                                            pa.array([7, -1, 1 << 40], pa.int64())),
        "d": pa.DictionaryArray.from_arrays(pa.array([0, 1, 2, 3, 3, None, 0], pa.uint8()),
                                            pa.array([1.5, float("nan"), -0.0, None], pa.float64())),
        "m": pa.DictionaryArray.from_arrays(pa.array([1, 0, 1, None, 0, 0, 1], pa.int32()),
                                            pa.array([D("12.34"), D("-0.05")], pa.decimal128(10, 2))),
    }
    return pa.table(cols)


def _decoded(t):
    return pa.table({c: t.column(c).combine_chunks().dictionary_decode() if t.num_rows else
                     pa.array([], t.schema.field(c).type.value_type) for c in t.column_names})


def _assert_same_column(a, b):
    assert (a.dtype, a.length, a.null_count, a.stand_in) == (b.dtype, b.length, b.null_count, b.stand_in)
    for k, (x, y) in enumerate(((a.validity, b.validity), (a.values, b.values), (a.data, b.data))):
        assert (x is None) == (y is None)
        if x is None:
            continue
        assert x.dtype == y.dtype and x.shape == y.shape
        if k == 0 or (k == 1 and a.dtype == N.BOOL):
            # a bitmap: the bits of the batch's rows (a batch cut from a longer array on a byte
            # boundary keeps the neighbouring rows' bits in its last byte; nothing reads them)
            x, y = (np.unpackbits(v.numpy(), bitorder="little")[:a.length] for v in (x, y))
        assert x.numpy().tobytes() == y.numpy().tobytes() if k and a.dtype != N.BOOL else (x == y).all()


@pytest.mark.parametrize("max_batch_rows", [None, 4])
def test_from_arrow_cpu_equals_the_decoded_table(max_batch_rows):
    t = _dictionary_table()
    got = Table.from_arrow(t, device="cpu", max_batch_rows=max_batch_rows)
    ref = Table.from_arrow(_decoded(t), device="cpu", max_batch_rows=max_batch_rows)
    assert [f.dtype for f in got.schema.fields] == [f.dtype for f in ref.schema.fields]
    assert [f.type_name for f in got.schema.fields] == [f.type_name for f in ref.schema.fields]
    assert [f.type_name for f in got.schema.fields] == ["StringType", "LongType", "DoubleType",
                                                        "DecimalType(10,2)"]
    assert len(got.batches) == len(ref.batches)
    for gb, rb in zip(got.batches, ref.batches):
        for c in t.column_names:
            assert not gb[c].stand_in and gb[c].encoded is None  # (host decode: nothing kept)
            _assert_same_column(gb[c], rb[c])


def test_sliced_and_chunked_with_different_dictionaries():
    a = pa.DictionaryArray.from_arrays(pa.array([0, 1, 1, None, 0, 2, 2, 1, 0, 1, 2], pa.int8()),
                                       pa.array(["x", "yy", "zzz"])).slice(3, 7)
    b = pa.DictionaryArray.from_arrays(pa.array([1, 0, 0], pa.int8()), pa.array(["yy", "w"]))
    t = pa.table({"c": pa.chunked_array([a, b])})
    for mbr in (None, 5):
        got = Table.from_arrow(t, device="cpu", max_batch_rows=mbr)
        ref = Table.from_arrow(pa.table({"c": pa.chunked_array([a.dictionary_decode(),
                                                                b.dictionary_decode()])}),
                               device="cpu", max_batch_rows=mbr)
        assert len(got.batches) == len(ref.batches)
        for gb, rb in zip(got.batches, ref.batches):
            _assert_same_column(gb["c"], rb["c"])


def test_value_types_that_need_a_cast_and_wide_indices():
    ts = pa.DictionaryArray.from_arrays(pa.array([0, 1, 0], pa.int64()),
                                        pa.array([1_000, 2_000], pa.timestamp("ms")))
    d64 = pa.DictionaryArray.from_arrays(pa.array([1, None, 0], pa.uint32()),
                                         pa.array([86_400_000, 0], pa.date64()))
    ls = pa.DictionaryArray.from_arrays(pa.array([0, 0, 1], pa.uint64()),
                                        pa.array(["a", "bc"], pa.large_string()))
    t = pa.table({"ts": ts, "d64": d64, "ls": ls})
    got = Table.from_arrow(t, device="cpu")
    ref = Table.from_arrow(_decoded(t), device="cpu")
    assert [f.type_name for f in got.schema.fields] == ["TimestampType", "DateType", "StringType"]
    for c in t.column_names:
        _assert_same_column(got.batches[0][c], ref.batches[0][c])


def test_unsupported_value_type_stays_unsupported():
    t = pa.dictionary(pa.int8(), pa.list_(pa.int32()))
    assert arrow_field_type(t)[0] == N.UNSUPPORTED
    assert arrow_field_type(pa.dictionary(pa.int16(), pa.string()))[0] == N.UTF8
    assert arrow_field_type(pa.dictionary(pa.uint64(), pa.binary()))[:2] == (N.UTF8, "BinaryType")


def test_host_tables_refuse_a_dictionary_column_by_name():
    t = pa.table({"id": pa.array([1, 2, 3], pa.int64()),
                  "priority": pa.array(["a", "b", "a"]).dictionary_encode()})
    with pytest.raises(TypeError, match="priority"):
        HostTable.from_arrow(t)
    with pytest.raises(TypeError, match="priority"):
        HostTable.from_arrow_c(t.to_batches())


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "deequ_amd.h")).read()
    for name in ("dq_dict_decode", "dq_freq_add_dict_device"):
        assert name + "(" in header
        assert name in N.EXPORTED
        assert getattr(N.lib, name, None) is not None
    for k, name in enumerate(["INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64"], 1):
        assert f"DQ_INDEX_{name} = {k}" in header and getattr(N, "INDEX_" + name) == k
