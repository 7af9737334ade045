"""Row-exact conformance of the device string casts (dq_cast_utf8, csrc/cast.hip) against the host
restatement of Spark 2.2's Cast in tests/cast_cases.py (checked on the host by test_cast_cases.py).

dq_cast_utf8 is called directly, one call per batch as profiles._cast_column does, so that
n_unsupported is read as a number.  For each target type and each table every row is pinned by
cast_cases.check_long / check_double (the rules are in that module's docstring): the long's value
and validity, the double's bits with the sign of zero wherever the device converts, NULL told from
unsupported through the exact count, and plain_in_window as the floor of what must convert -- which
holds the device's fp64 multiply and divide by 10^k to the correctly rounded result at w = 2^53,
|exponent| = 22, the rescale of larger exponents and the 19-digit cut.  Around the call: a NULL
input row stays NULL whatever bytes its offsets span, values at NULL rows are 0, the padding bits of
the last validity byte are 0, and nothing is written past either output.

Layouts: row counts around 8 (one thread writes one validity byte) and 2048 (rows per block), with
and without an input bitmap, a column sliced at rows 3 and 11 (first offset not 0, bitmap re-based
on the device), batches of 128 rows, an empty column.
"""
import ctypes
import math

import numpy as np
import pyarrow as pa
import pytest

import cast_cases as CC

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements / bytes after each output that the kernel must not touch
SENTINEL = 0x5A5A5A5A5A5A5A5A
# what a NULL row's offsets span: read as a string it would be unsupported, a value, or NULL
GARBAGE = [b"1e5", b"12", b"\xff\xfe", b"NaN", b"", b"9007199254740993", b"0x1p3"]

EDGES = CC.TABLES["window edges"]


def _tiled(n):
    return [EDGES[i % len(EDGES)] for i in range(n)]


def _with_nulls(rows, seed):
    """About 10 % NULL rows, the last row among them (the edge of the last validity byte)."""
    mask = np.random.default_rng(seed).random(len(rows)) < 0.1
    mask[-1] = True
    return [None if m else b for b, m in zip(rows, mask)]


def _host_buffers(rows):
    """(validity or None, offsets, data) in Arrow's utf8 layout; a NULL row spans garbage."""
    spans = [GARBAGE[i % len(GARBAGE)] if b is None else b for i, b in enumerate(rows)]
    offsets = np.zeros(len(rows) + 1 + 4, np.int32)
    offsets[1:len(rows) + 1] = np.cumsum([len(s) for s in spans])
    offsets[len(rows) + 1:] = offsets[len(rows)]
    data = np.frombuffer(b"".join(spans) + bytes(16), np.uint8)
    validity = None
    if any(b is None for b in rows):
        bits = np.array([b is not None for b in rows], np.uint8)
        validity = np.concatenate([np.packbits(bits, bitorder="little"), np.zeros(16, np.uint8)])
    return validity, offsets, data


def _device_column(rows, device):
    import torch
    from deequ_amd import _native as N
    from deequ_amd.table import ColumnBatch
    validity, offsets, data = _host_buffers(rows)
    up = lambda a: None if a is None else torch.from_numpy(a.copy()).to(device)  # noqa: E731
    return ColumnBatch(N.UTF8, len(rows), up(validity), up(offsets), up(data))


def _cast(col_c, length, to_type, device):
    """One dq_cast_utf8 call -> (valid, values, n_unsupported); the outputs start out poisoned."""
    import torch
    from deequ_amd import _native as N
    nbytes = (length + 7) // 8
    values = torch.full((length + GUARD,), SENTINEL, dtype=torch.int64, device=device)
    validity = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=device)
    bad = ctypes.c_int64(-1)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    N.check(N.lib.dq_cast_utf8(ctypes.byref(col_c), to_type, values.data_ptr(), validity.data_ptr(),
                               ctypes.byref(bad), stream))
    v, b = values.cpu().numpy(), validity.cpu().numpy()
    assert (v[length:] == SENTINEL).all(), "values written past the last row"
    assert (b[nbytes:] == 0xFF).all(), "validity written past its last byte"
    bits = np.unpackbits(b[:nbytes], bitorder="little")
    assert not bits[length:].any(), "padding bits of the last validity byte"
    v = v[:length] if to_type == N.INT64 else v[:length].view(np.float64)
    return bits[:length].astype(bool), v, bad.value


def _check(rows, col_c, device):
    from deequ_amd import _native as N
    CC.check_long(rows, *_cast(col_c, len(rows), N.INT64, device))
    CC.check_double(rows, *_cast(col_c, len(rows), N.FLOAT64, device))


@pytest.mark.parametrize("name", list(CC.TABLES))
def test_long_rows(name, gpu_device):
    from deequ_amd import _native as N
    rows = CC.TABLES[name]
    col = _device_column(rows, gpu_device)
    CC.check_long(rows, *_cast(col.to_c(), len(rows), N.INT64, gpu_device))


@pytest.mark.parametrize("name", list(CC.TABLES))
def test_double_rows(name, gpu_device):
    from deequ_amd import _native as N
    rows = CC.TABLES[name]
    col = _device_column(rows, gpu_device)
    valid, values, bad = _cast(col.to_c(), len(rows), N.FLOAT64, gpu_device)
    print(name, "rows", len(rows), "converted", int(valid.sum()), "unsupported", bad)
    CC.check_double(rows, valid, values, bad)


@pytest.mark.parametrize("nulls", [False, True], ids=["no bitmap", "10% NULL"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 4099])
def test_row_counts_around_a_validity_byte_and_a_block(n, nulls, gpu_device):
    rows = _with_nulls(_tiled(n), n) if nulls else _tiled(n)
    col = _device_column(rows, gpu_device)
    assert (col.validity is not None) == nulls
    _check(rows, col.to_c(), gpu_device)


@pytest.mark.parametrize("offset", [3, 11])
def test_sliced_column(offset, gpu_device):
    """An Arrow slice over device buffers: the offsets pointer moves, the first offset is not 0,
    the characters are the unsliced buffer, the bitmap is re-based to bit 0 on the device."""
    import torch
    from deequ_amd import _native as N
    from deequ_amd.loader import ArrowArrayC, ArrowSchemaC
    whole = _with_nulls(_tiled(2 * len(EDGES) + 29), offset)
    rows = whole[offset:len(whole) - 5]
    validity, offsets, data = _host_buffers(whole)
    assert offsets[offset] > 0 and any(b is None for b in rows)
    dev = [torch.from_numpy(a.copy()).to(gpu_device) for a in (validity, offsets, data)]
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in dev])
    a = ArrowArrayC(length=len(rows), null_count=sum(b is None for b in rows), offset=offset,
                    n_buffers=3, n_children=0, buffers=ptrs)
    s = ArrowSchemaC(format=b"u", name=b"s", flags=2)
    col = N.dq_column()
    N.check(N.lib.dq_column_from_arrow(ctypes.addressof(a), ctypes.addressof(s), ctypes.byref(col)))
    try:
        assert col.values == dev[1].data_ptr() + 4 * offset and col.data == dev[2].data_ptr()
        assert col.validity != dev[0].data_ptr()
        _check(rows, col, gpu_device)
    finally:
        N.lib.dq_column_release(ctypes.byref(col))


def test_batches_of_128_rows(gpu_device):
    from deequ_amd.table import Table
    rows = _with_nulls(_tiled(1000), 128)
    arr = pa.array([None if b is None else b.decode("utf-8") for b in rows], pa.string())
    df = Table.from_arrow(pa.table({"s": arr}), device=gpu_device, max_batch_rows=128)
    assert [b["s"].length for b in df.batches] == [128] * 7 + [104]
    at = 0
    for b in df.batches:
        _check(rows[at:at + b["s"].length], b["s"].to_c(), gpu_device)
        at += b["s"].length


def test_empty_column(gpu_device):
    from deequ_amd import _native as N
    from deequ_amd.table import Table
    df = Table.from_arrow(pa.table({"s": pa.array([], pa.string())}), device=gpu_device)
    col = df.batches[0]["s"]
    assert col.length == 0
    for to_type in (N.INT64, N.FLOAT64):
        valid, values, bad = _cast(col.to_c(), 0, to_type, gpu_device)
        assert len(valid) == len(values) == 0 and bad == 0


def test_profile_of_a_fractional_string_column(gpu_device):
    """DataType's regex calls all four strings Fractional; Cast gives 1.0, 0.5, NULL ("- 1.5":
    Java rejects the inner space) and 1e20.  The profile is that of the three values."""
    from deequ_amd.analyzers.datatype import DataTypeInstances
    from deequ_amd.profiles import ColumnProfiler, NumericColumnProfile
    from deequ_amd.table import Table
    texts = ["1.", ".5", "- 1.5", "1" + "0" * 20 + ".0"]
    ref = [CC.java_parse_double(t.encode())[1] for t in texts]
    assert ref == [1.0, 0.5, None, 1e20]
    xs = [x for x in ref if x is not None]
    df = Table.from_pydict({"s": texts}, {"s": "string"}, device=gpu_device)
    p = ColumnProfiler.profile(df, ["s"], False, 1).profiles["s"]
    print(p)
    assert isinstance(p, NumericColumnProfile)
    assert p.data_type == DataTypeInstances.Fractional and p.is_data_type_inferred
    assert p.type_counts == {"Boolean": 0, "Fractional": 4, "Integral": 0, "Unknown": 0, "String": 0}
    assert p.completeness == 1.0
    assert (p.minimum, p.maximum) == (0.5, 1e20)
    # 1e20 + 1.5 rounds to 1e20 in any order of the three additions (ulp(1e20) = 16384)
    assert p.sum == 1e20
    # Mean.scala:40 divides sum(column) by count("*"): the NULL row counts in the denominator
    mean = math.fsum(xs) / len(texts)
    assert abs(p.mean - mean) <= 1e-12 * mean           # the suite's contract for averages
    avg = math.fsum(xs) / 3                             # StandardDeviation: the three values alone
    sd = math.sqrt(math.fsum((x - avg) ** 2 for x in xs) / 3)
    assert abs(p.std_dev - sd) <= 1e-12 * sd
    assert set(p.approx_percentiles) <= set(xs) and len(p.approx_percentiles) == 100
    assert p.approx_percentiles == sorted(p.approx_percentiles)
