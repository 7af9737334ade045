"""dq_split_rows and Table.random_split on the device against the host restatement of the draw
(tests/split_host.py).  All comparisons are exact."""
import ctypes
import os
import re

import numpy as np
import pytest

import split_host as S

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deequ_amd", "csrc")


def _constant(file, name):
    m = re.search(rf"constexpr int {name} = (\d+);", open(os.path.join(CSRC, file)).read())
    assert m, f"{name} is no longer a literal in {file}"
    return int(m.group(1))


# split.hip: kSplitBlock = kBlock threads, one row per lane, so a block takes kBlock rows per pass;
# the grid is capped at kSplitMaxBlocks blocks, beyond which the blocks stride over the words.
assert "kSplitBlock = kBlock;" in open(os.path.join(CSRC, "split.hip")).read()
BLOCK_ROWS = _constant("engine.h", "kBlock")
GRID_ROWS = _constant("split.hip", "kSplitMaxBlocks") * BLOCK_ROWS
ROWS = [0, 1, 63, 64, 65, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 100_003,
        GRID_ROWS - 1, GRID_ROWS, GRID_ROWS + 65]
EIGHT = [1.0] * 8
# every row_base, seed and weight vector of the issue, each at least once
COMBOS = [(0, 0, [0.9, 0.1]), (2**33 + 5, 1, [1, 1, 1]), (0, 2**63, [0.5, 0.5]),
          (2**33 + 5, 2**64 - 1, [1e-9, 1]), (0, 1, EIGHT), (2**33 + 5, 0, [0.9, 0.1]),
          (0, 2**64 - 1, [1, 1, 1]), (2**33 + 5, 2**63, EIGHT)]
SENTINEL = 0xA5A5A5A5A5A5A5A5


def call_split(device, rows, row_base, seed, bounds, n_splits=None, null=()):
    """dq_split_rows into sentinel-filled bitmaps with one guard word each:
    (status, [uint64 words incl. the guard], counts)."""
    import torch
    from deequ_amd import _native as N
    k = len(bounds) if n_splits is None else n_splits
    words = (max(rows, 0) + 63) // 64 if rows < 2**31 else 1
    fill = np.full(words + 1, SENTINEL, np.uint64).view(np.int64)
    maps = [torch.from_numpy(fill.copy()).to(device) for _ in range(max(k, 1))]
    ptrs = (ctypes.c_void_p * max(k, 1))(*[m.data_ptr() for m in maps])
    for j in null:
        if isinstance(j, int):
            ptrs[j] = None
    counts = (ctypes.c_int64 * N.SPLIT_MAX)(*([-1] * N.SPLIT_MAX))
    cb = (ctypes.c_double * max(len(bounds), 1))(*bounds)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    status = N.lib.dq_split_rows(rows, row_base, seed, None if "bounds" in null else cb, k,
                                 None if "bitmaps" in null else ptrs,
                                 None if "counts" in null else counts, stream)
    torch.cuda.synchronize()
    return status, [m.cpu().numpy().view(np.uint64) for m in maps], list(counts)


@pytest.mark.parametrize("rows", ROWS)
def test_bitmaps_and_counts_match_the_restatement(gpu_device, rows):
    for row_base, seed, weights in COMBOS:
        bounds = S.bounds(weights)
        status, maps, counts = call_split(gpu_device, rows, row_base, seed, bounds)
        assert status == 0
        want_maps, want_counts = S.bitmaps(seed, row_base, rows, weights)
        k, words = len(weights), (rows + 63) // 64
        assert counts[:k] == want_counts and sum(counts[:k]) == rows
        union = np.zeros(words, np.uint64)
        total = 0
        for got, want, count in zip(maps, want_maps, counts):
            assert got[words] == SENTINEL  # nothing written past the last word
            assert np.array_equal(got[:words], want), (rows, row_base, seed, weights)
            assert not (union & got[:words]).any()  # a row is in one bitmap only
            union |= got[:words]
            pop = int(np.unpackbits(got[:words].view(np.uint8)).sum())
            assert pop == count
            total += pop
        assert total == rows
        if rows:  # every row in some bitmap, padding bits of the last word zero
            full = np.full(words, ~np.uint64(0))
            if rows % 64:
                full[-1] = np.uint64((1 << (rows % 64)) - 1)
            assert np.array_equal(union, full)


def test_argument_errors(gpu_device):
    from deequ_amd import _native as N
    inv, uns = N.ERR_INVALID_ARGUMENT, N.ERR_UNSUPPORTED
    ok = [0.9, 1.0]
    cases = [
        (dict(rows=100, row_base=0, seed=0, bounds=ok, null=("bounds",)), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=ok, null=("bitmaps",)), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=ok, null=("counts",)), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=ok, null=(1,)), inv),  # one bitmap NULL
        (dict(rows=-1, row_base=0, seed=0, bounds=ok), inv),
        (dict(rows=100, row_base=-1, seed=0, bounds=ok), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=ok, n_splits=0), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=[1.0] * 9), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=[0.6, 0.5, 1.0]), inv),  # decreasing
        (dict(rows=100, row_base=0, seed=0, bounds=[0.0, 1.0]), inv),       # not in (0, 1]
        (dict(rows=100, row_base=0, seed=0, bounds=[-0.5, 1.0]), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=[0.5, 1.5]), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=[float("nan"), 1.0]), inv),
        (dict(rows=100, row_base=0, seed=0, bounds=[0.5, 0.75]), inv),      # the last is not 1
        (dict(rows=2**31, row_base=0, seed=0, bounds=ok), uns),
    ]
    for kwargs, want in cases:
        status, maps, _ = call_split(gpu_device, **kwargs)
        assert status == want, kwargs
        assert N.lib.dq_last_error()
        for m in maps:  # nothing was launched: the bitmaps are as they were
            assert (m == SENTINEL).all(), kwargs
    # rows == 0 succeeds, zeroes the counts and needs no bitmaps
    status, maps, counts = call_split(gpu_device, 0, 0, 0, ok, null=(0, 1))
    assert status == 0 and counts[:2] == [0, 0]
    # equal bounds are non-decreasing: a split of weight zero gets no rows
    status, maps, counts = call_split(gpu_device, 1000, 0, 3, [0.5, 0.5, 1.0])
    assert status == 0 and counts[1] == 0 and counts[0] + counts[2] == 1000


# ------------------------------------------------------------------------------------------------
# Table.random_split
# ------------------------------------------------------------------------------------------------
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
    # (NaN as text, so that lists compare)
    return [("NaN" if isinstance(v, float) and v != v else v) if ok else None
            for v, ok in zip(vals, valid)]


def table_to_lists(t):
    return {f.name: [v for b in t.batches for v in column_to_list(b[f.name])] for f in t.schema.fields}


N_ROWS = 1000


def arrow_source():
    import datetime
    from decimal import Decimal

    import pyarrow as pa
    rng = np.random.default_rng(11)
    n = N_ROWS
    null = lambda p: rng.random(n) < p  # noqa: E731
    f64 = rng.normal(size=n)
    f64[::17] = np.nan
    f32 = rng.normal(size=n).astype(np.float32)
    f32[5::23] = np.nan
    words = ["", "a", "grün", "日本語", "x" * 40, "né", "\U0001F600"]
    text = [words[i] for i in rng.integers(0, len(words), n)]
    cats = ["low", "high", None, "mid"]
    cols = {
        "b": pa.array(rng.random(n) < 0.5, mask=null(0.1), type=pa.bool_()),
        "i8": pa.array(rng.integers(-128, 128, n).astype(np.int8), mask=null(0.1)),
        "i16": pa.array(rng.integers(-2**15, 2**15, n).astype(np.int16), mask=null(0.1)),
        "i32": pa.array(rng.integers(-2**31, 2**31, n).astype(np.int32), mask=null(0.1)),
        "i64": pa.array(rng.integers(-2**62, 2**62, n), mask=null(0.1), type=pa.int64()),
        "f32": pa.array(f32, mask=null(0.1)),
        "f64": pa.array(f64, mask=null(0.1)),
        "s": pa.array([None if m else t for t, m in zip(text, null(0.15))], pa.string()),
        "dec": pa.array([None if m else Decimal(int(v) * 10**10 + 7).scaleb(-18) for v, m in
                         zip(rng.integers(-10**18, 10**18, n), null(0.1))],
                        pa.decimal128(38, 18)),
        "d": pa.array([None if m else datetime.date(1970, 1, 1) + datetime.timedelta(int(v))
                       for v, m in zip(rng.integers(-20000, 20000, n), null(0.1))], pa.date32()),
        "ts": pa.array(rng.integers(-10**15, 10**15, n), mask=null(0.1), type=pa.int64())
        .cast(pa.timestamp("us")),
        "dict": pa.DictionaryArray.from_arrays(
            pa.array(rng.integers(0, len(cats), n).astype(np.int16), mask=null(0.1)),
            pa.array(cats, pa.string())),
        "dense": pa.array(np.arange(n, dtype=np.int64)),  # no validity buffer
        "nulls": pa.array([None] * n, pa.int32()),
    }
    return pa.table(cols)


@pytest.fixture(scope="module")
def source(gpu_device):
    """(arrow table, the one-batch device table, its columns as lists): computed once."""
    from deequ_amd.table import Table
    arrow = arrow_source()
    table = Table.from_arrow(arrow, device=gpu_device)
    lists = table_to_lists(table)
    # anchor the read-back helper on columns whose Python values are Arrow's own
    assert lists["i64"] == arrow.column("i64").to_pylist()
    assert lists["s"] == arrow.column("s").to_pylist()
    assert lists["dict"] == arrow.column("dict").to_pylist()
    assert lists["dense"] == list(range(N_ROWS)) and lists["nulls"] == [None] * N_ROWS
    assert table.batches[0]["dense"].validity is None
    assert table.batches[0]["dict"].encoded is not None
    return arrow, table, lists


def expected_splits(lists, seed, weights):
    a = S.assign(seed, 0, N_ROWS, weights)
    return [{name: [v for v, s in zip(vals, a) if s == k] for name, vals in lists.items()}
            for k in range(len(weights))]


@pytest.mark.parametrize("seed,weights", [(0, [0.9, 0.1]), (7, [1, 1, 1]), (2**63, EIGHT)])
def test_random_split_selects_the_restated_rows(gpu_device, source, seed, weights):
    _, table, lists = source
    splits = table.random_split(weights, seed)
    want = expected_splits(lists, seed, weights)
    assert len(splits) == len(weights)
    assert sum(t.num_rows for t in splits) == N_ROWS
    for t, w in zip(splits, want):
        assert t.schema == table.schema
        assert table_to_lists(t) == w
        assert t.num_rows == len(w["dense"])
        for b in t.batches:
            assert b["dict"].encoded is None       # the decoded column, no encoded pair
            assert b["dense"].validity is None     # no validity buffer in, none out


@pytest.mark.parametrize("max_batch_rows", [64, 192])
def test_random_split_does_not_depend_on_the_batches(gpu_device, source, max_batch_rows):
    from deequ_amd.table import Table
    arrow, _, lists = source
    table = Table.from_arrow(arrow, device=gpu_device, max_batch_rows=max_batch_rows)
    assert len(table.batches) == -(-N_ROWS // max_batch_rows)
    want = expected_splits(lists, 5, [0.5, 0.3, 0.2])
    got = table.random_split([0.5, 0.3, 0.2], 5)
    assert [table_to_lists(t) for t in got] == want


def test_negative_seed_is_its_twin_mod_2_64(gpu_device, source):
    _, table, lists = source
    a = [table_to_lists(t) for t in table.random_split([0.9, 0.1], -5)]
    b = [table_to_lists(t) for t in table.random_split([0.9, 0.1], 2**64 - 5)]
    assert a == b == expected_splits(lists, 2**64 - 5, [0.9, 0.1])
    assert a != expected_splits(lists, 5, [0.9, 0.1])
    # no seed: a fresh one is drawn; the splits still partition the table
    parts = table.random_split([1, 1])
    assert sorted(v for t in parts for v in table_to_lists(t)["dense"]) == list(range(N_ROWS))


def test_a_split_without_rows_is_an_empty_table(gpu_device, source):
    from deequ_amd import Analysis
    from deequ_amd.analyzers import Completeness, Size
    _, table, lists = source
    assert (S.assign(0, 0, N_ROWS, [1e-9, 1]) == 1).all()  # the restatement: nothing in split 0
    empty, rest = table.random_split([1e-9, 1], 0)
    assert empty.num_rows == 0 and empty.schema == table.schema and len(empty.batches) == 1
    assert table_to_lists(rest) == lists
    ctx = Analysis([Size(), Completeness("i32")]).run(empty)
    assert ctx.metric(Size()).value.get() == 0.0


def test_random_split_refusals(gpu_device, source):
    import pyarrow as pa
    from deequ_amd.table import Table
    _, table, _ = source
    for weights in ([], [0.5, 0], [1, -1], [float("nan"), 1], [float("inf"), 1], ["1", 1],
                    [True, 1], [1] * 9):
        with pytest.raises(ValueError, match="random_split"):
            table.random_split(weights, 0)
    for seed in (2**64, -2**63 - 1, 1.5, "0"):
        with pytest.raises(ValueError, match="seed"):
            table.random_split([1, 1], seed)
    lists_col = pa.table({"id": pa.array([1, 2, 3]), "l": pa.array([[1], None, [2, 3]])})
    with pytest.raises(ValueError, match=r"column l is UnsupportedType"):
        Table.from_arrow(lists_col, device=gpu_device).random_split([1, 1], 0)
