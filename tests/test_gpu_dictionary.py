"""Dictionary-encoded Arrow columns on the GPU: dq_dict_decode through Table.from_arrow against
Table.from_arrow of the decoded array (byte for byte), bad indices as input validation, and every
analyzer over dictionary columns against the same analyzer over the decoded table -- exactly, fp64
bit for bit: the scans run the same kernels on the same bytes, and the frequency metrics come
from integer counts through the 128-bit fixed-point sums."""
import ctypes
import decimal
import json
import os
import struct

import numpy as np
import pyarrow as pa
import pytest

from fixtures import arrow_table

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                     "reference_known_answers.json")))
NP = {"int8": np.int8, "uint8": np.uint8, "int16": np.int16, "int32": np.int32, "int64": np.int64}
BATCH = 128


def _dict_array(index_type, values, mask, dictionary):
    idx = pa.array(np.asarray(values, NP[index_type]), mask=np.asarray(mask, bool))
    return pa.DictionaryArray.from_arrays(idx, dictionary, safe=False)


STRINGS = pa.array(["hi", "", None, "lo", "héllo wörld", "日本語", "hi", "unused", "x" * 20, "lo"])
# entries 2 (NULL), 7 ("unused": never named below), 0 / 6 and 3 / 9 (duplicates)


def _string_case(index_type, rows, seed=0):
    rng = np.random.default_rng(seed + rows)
    used = np.array([0, 1, 2, 3, 4, 5, 6, 8, 9])
    values = used[rng.integers(0, len(used), rows)]
    mask = rng.random(rows) < 0.2
    if rows:
        values[0], mask[0] = 2, rows > 1  # a NULL index that names the NULL entry
    return _dict_array(index_type, values, mask, STRINGS)


def _decode_cases():
    D = decimal.Decimal
    cases = []
    for it in NP:
        for rows in (0, 1, 7, 8, 9, 63, 64, 65, 1100):
            cases.append((f"{it}-{rows}", _string_case(it, rows)))
    cases.append(("empty-dictionary", _dict_array("int8", [0] * 70, [True] * 70, pa.array([], pa.string()))))
    rng = np.random.default_rng(5)
    long_dict = pa.array(["ab", "cd", "L" * 300, "ef", "é" * 2500, "gh"])  # 2-, 300- and 5,000-byte entries
    cases.append(("long-entries", _dict_array("int16", rng.integers(0, 6, 600), rng.random(600) < 0.1,
                                              long_dict)))
    cases.append(("short-only", _dict_array("uint8", rng.integers(0, 3, 1100), [False] * 1100,
                                            pa.array(["high", "low", "medium"]))))
    cases.append(("slice-3-77", _string_case("int32", 200, seed=9).slice(3, 77)))
    cases.append(("two-chunks", pa.chunked_array([
        _dict_array("int8", rng.integers(0, 3, 150), rng.random(150) < 0.1, pa.array(["a", "bb", None])),
        _dict_array("int8", rng.integers(0, 4, 170), rng.random(170) < 0.1, pa.array(["bb", "q", "a", "zz"]))])))
    fixed = {
        "int8": pa.array([5, -7, None, 0], pa.int8()), "int16": pa.array([300, -1, None, 2], pa.int16()),
        "int32": pa.array([1 << 20, -3, None, 9], pa.int32()), "int64": pa.array([1 << 40, -5, None, 1], pa.int64()),
        "float": pa.array([1.5, -0.0, None, float("nan")], pa.float32()),
        "double": pa.array([2.5, -0.0, None, float("nan")], pa.float64()),
        "bool": pa.array([True, False, None, True]),
        "date32": pa.array([18000, -1, None, 0], pa.date32()),
        "date64": pa.array([86_400_000 * 3, 0, None, 86_400_000], pa.date64()),
        "timestamp": pa.array([1_600_000_000_123, 0, None, -1], pa.timestamp("ms", tz="UTC")),
        "decimal-10-2": pa.array([D("12.34"), D("-0.05"), None, D("0")], pa.decimal128(10, 2)),
        "decimal-38-18": pa.array([D("1234567890123456789.5"), D("-1"), None, D("0")], pa.decimal128(38, 18)),
    }
    for name, d in fixed.items():
        cases.append((f"fixed-{name}", _dict_array("int16", rng.integers(0, 4, 203), rng.random(203) < 0.15, d)))
    cases.append(("fixed-no-nulls", _dict_array("uint8", rng.integers(0, 2, 65), [False] * 65,
                                                pa.array([4, 9], pa.int64()))))
    return cases


def _plain(col):
    if isinstance(col, pa.ChunkedArray):
        return pa.chunked_array([c.dictionary_decode() for c in col.chunks])
    return col.dictionary_decode()


def _bits(t, n):
    return np.unpackbits(t.cpu().numpy(), bitorder="little")[:n].astype(bool)


def _assert_decoded_equal(got, ref):
    from deequ_amd import _native as N
    n = ref.length
    assert (got.dtype, got.length, got.stand_in, got.null_count) == (ref.dtype, n, False, ref.null_count)
    for x, y in ((got.validity, ref.validity), (got.values, ref.values), (got.data, ref.data)):
        assert (x is None) == (y is None)
        assert x is None or (x.dtype == y.dtype and x.shape == y.shape)  # (the same padding)
    valid = _bits(ref.validity, n) if ref.validity is not None else np.ones(n, bool)
    if got.validity is not None:  # the rows' bits; a device-decoded bitmap is zero beyond them
        assert (_bits(got.validity, n) == valid).all()
        assert not np.unpackbits(got.validity.cpu().numpy(), bitorder="little")[n:].any()
    if got.dtype == N.UTF8:
        go, ro = got.values.cpu().numpy(), ref.values.cpu().numpy()
        assert (go[:n + 1] == ro[:n + 1]).all() and not go[n + 1:].any()
        last = int(ro[n])
        gd, rd = got.data.cpu().numpy(), ref.data.cpu().numpy()
        assert gd[:last].tobytes() == rd[:last].tobytes() and not gd[last:].any()
    elif got.dtype == N.BOOL:
        g, r = _bits(got.values, n), _bits(ref.values, n)
        assert (g[valid] == r[valid]).all() and not g[~valid].any()
    else:
        width = 2 if N.is_decimal(got.dtype) else 1
        g = got.values.cpu().numpy()[:width * n].reshape(n, width).view(np.uint8).reshape(n, -1)
        r = ref.values.cpu().numpy()[:width * n].reshape(n, width).view(np.uint8).reshape(n, -1)
        assert (g[valid] == r[valid]).all() and not g[~valid].any()
        assert not got.values.cpu().numpy()[width * n:].view(np.uint8).any()


@pytest.mark.parametrize("name,col", _decode_cases(), ids=[c[0] for c in _decode_cases()])
def test_decode_parity(name, col, gpu_device):
    from deequ_amd import Table
    got = Table.from_arrow(pa.table({"c": col}), device=gpu_device, max_batch_rows=BATCH)
    ref = Table.from_arrow(pa.table({"c": _plain(col)}), device=gpu_device, max_batch_rows=BATCH)
    assert got.schema.fields[0].dtype == ref.schema.fields[0].dtype
    assert got.schema.fields[0].type_name == ref.schema.fields[0].type_name
    assert len(got.batches) == len(ref.batches) and got.num_rows == len(col)
    for gb, rb in zip(got.batches, ref.batches):
        assert gb["c"].length == 0 or gb["c"].encoded is not None
        _assert_decoded_equal(gb["c"], rb["c"])
    if isinstance(col, pa.ChunkedArray):  # without a batch size: one batch per dictionary
        one = Table.from_arrow(pa.table({"c": col}), device=gpu_device)
        assert [b["c"].length for b in one.batches] == [len(c) for c in col.chunks]
        for b, c in zip(one.batches, col.chunks):
            _assert_decoded_equal(b["c"], Table.from_arrow(pa.table({"c": c.dictionary_decode()}),
                                                           device=gpu_device).batches[0]["c"])


def test_bad_indices_are_refused(gpu_device):
    """Input validation, as dq_gather_column's: the kernels compare every index with the bounds
    before they use it, so nothing here depends on a read out of range."""
    import torch

    from deequ_amd import Table
    from deequ_amd import _native as N
    from deequ_amd.analyzers import FrequencyTable
    from deequ_amd.table import EncodedColumn, _array_to_device, _to_device
    dictionary = pa.array(["a", "b", "c"])
    idx = np.array([0, -1, 2, 3, 1, 0, 0, 2, 1, 1] + [0] * 16, np.int32)  # -1 and len(dictionary)
    bad = pa.DictionaryArray.from_arrays(pa.array(idx[:10]), dictionary, safe=False)
    with pytest.raises(ValueError, match=r"column c: 2 of 10 rows"):
        Table.from_arrow(pa.table({"c": bad}), device=gpu_device)
    table = FrequencyTable(["c"], [N.UTF8], 0)
    good = Table.from_arrow(pa.table({"c": pa.array(["a", "b", "a", None]).dictionary_encode()}),
                            device=gpu_device)
    table.add([good.batches[0]["c"]], encoded=True)
    before = (table.num_rows, sorted(table.export()))
    enc = EncodedColumn(N.INDEX_INT32, 10, _to_device(idx, gpu_device), None,
                        _array_to_device(dictionary, N.UTF8, gpu_device))
    cidx, cdict = enc.indices_c(), enc.dictionary.to_c()
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    status = N.lib.dq_freq_add_dict_device(table.handle, ctypes.byref(cidx), enc.index_type,
                                           ctypes.byref(cdict), 0, stream)
    assert status == N.ERR_INVALID_ARGUMENT
    assert b"2 of the 10 rows" in N.lib.dq_last_error()
    assert (table.num_rows, sorted(table.export())) == before == (4, [(("a",), 2), (("b",), 1)])


# ------------------------------------------------------------------------------------------------
# Analyzer parity
# ------------------------------------------------------------------------------------------------
ROWS = 3000
# dq_freq_add_dict_device's count kernel: registers up to 8 entries, per-wave LDS counters up to
# 1,024, one LDS copy up to 16,384 (dict.hip kDictLdsMax), global atomics above
LDS_MAX = 16384


def _skewed(rng, entries, rows):
    """Indices whose two most frequent entries are 0 and 1, far ahead of the rest and of each other.
    dq_freq_topk returns ties in any order (as the reference's rdd.top does), so a Histogram cut
    at max_detail_bins is only determined when no tie straddles the cut: the data has none."""
    p = np.full(entries, 0.5 / (entries - 2))
    p[0], p[1] = 0.3, 0.2
    return rng.choice(entries, rows, p=p)


def _parity_tables():
    rng = np.random.default_rng(11)
    p3 = _dict_array("int8", _skewed(rng, 3, ROWS), rng.random(ROWS) < 0.05, pa.array(["a", "b", "c"]))
    c700 = _dict_array("int16", _skewed(rng, 700, ROWS), rng.random(ROWS) < 0.02,
                       pa.array([f"v{i:03d}" if i != 13 else "NullValue" for i in range(700)]))
    i64 = _dict_array("uint8", _skewed(rng, 40, ROWS), rng.random(ROWS) < 0.03,
                      pa.array(rng.integers(-1 << 50, 1 << 50, 40), pa.int64()))
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000123))[0]  # a second NaN payload
    dbl = _dict_array("int32", _skewed(rng, 7, ROWS), rng.random(ROWS) < 0.04,
                      pa.array([1.5, -0.0, float("nan"), 0.0, nan2, None, 2.25], pa.float64()))
    t = pa.table({"p3": p3, "c700": c700, "i64": i64, "dbl": dbl})
    return t, pa.table({c: _plain(t.column(c).combine_chunks()) for c in t.column_names})


def _suite():
    from deequ_amd.analyzers import (ApproxCountDistinct, ApproxQuantile, Completeness, Compliance,
                                     CountDistinct, DataType, Distinctness, Entropy, Histogram, Maximum,
                                     Mean, Minimum, MutualInformation, PatternMatch, Size,
                                     StandardDeviation, Sum, UniqueValueRatio, Uniqueness)
    out = [Size(), MutualInformation(["p3", "c700"]), MutualInformation(["i64", "dbl"])]
    for c in ("p3", "c700"):
        out += [Completeness(c), Compliance(f"{c} in", f"{c} IS NULL OR {c} IN ('a','b')"),
                Compliance(f"{c} like", f"{c} LIKE 'a%'"), PatternMatch(c, r"^[av]\d*$"), DataType(c),
                ApproxCountDistinct(c)]
    for c in ("i64", "dbl"):
        out += [Completeness(c), DataType(c), ApproxCountDistinct(c), Minimum(c), Maximum(c), Sum(c),
                Mean(c), StandardDeviation(c), ApproxQuantile(c, 0.5)]
    for c in ("p3", "c700", "i64", "dbl"):
        out += [Uniqueness([c]), Distinctness([c]), UniqueValueRatio([c]), CountDistinct([c]), Entropy(c),
                Histogram(c, max_detail_bins=2), Histogram(c)]
    return out


def _canon(metric):
    v = metric.value
    if not v.is_success:
        return ("failure", type(v.failed).__name__, str(v.failed))
    x = v.get()
    if isinstance(x, float):
        return ("double", struct.pack("<d", x))
    if hasattr(x, "number_of_bins"):
        return ("distribution", x.number_of_bins,
                sorted((k, d.absolute, struct.pack("<d", d.ratio)) for k, d in x.values.items()))
    if isinstance(x, dict):
        return ("keyed", sorted((k, struct.pack("<d", float(d))) for k, d in x.items()))
    return ("other", repr(x))


def _assert_same_metrics(enc_table, plain_table, analyzers):
    from deequ_amd.runners import AnalysisRunner
    got = AnalysisRunner.do_analysis_run(enc_table, analyzers)
    ref = AnalysisRunner.do_analysis_run(plain_table, analyzers)
    for a in analyzers:
        assert _canon(got.metric(a)) == _canon(ref.metric(a)), str(a)
    return ref


def test_analyzers_equal_the_decoded_table(gpu_device):
    from deequ_amd import Table
    from deequ_amd.analyzers import Histogram, MutualInformation, Uniqueness
    enc_arrow, plain_arrow = _parity_tables()
    enc = Table.from_arrow(enc_arrow, device=gpu_device, max_batch_rows=BATCH)
    plain = Table.from_arrow(plain_arrow, device=gpu_device, max_batch_rows=BATCH)
    assert len(enc.batches) == (ROWS + BATCH - 1) // BATCH
    ref = _assert_same_metrics(enc, plain, _suite())
    assert ref.metric(Uniqueness(["p3"])).value.is_success and ref.metric(Histogram("dbl")).value.is_success
    for c in ("p3", "c700", "i64", "dbl"):
        for null_as_group, analyzer in ((False, Uniqueness([c])), (True, Histogram(c))):
            e, p = analyzer.compute_state_from(enc).frequencies, analyzer.compute_state_from(plain).frequencies
            assert e.encoded_batches == len(enc.batches) and p.encoded_batches == 0
            assert e.num_rows == p.num_rows == ROWS
            counts_e, offs_e, raw_e = e.export_raw()
            counts_p, offs_p, raw_p = p.export_raw()
            groups = [sorted((raw[o[k]:o[k + 1]].tobytes(), int(n[k])) for k in range(len(n)))
                      for n, o, raw in ((counts_e, offs_e, raw_e), (counts_p, offs_p, raw_p))]
            assert groups[0] == groups[1]
            se, sp = e.summarize(), p.summarize()
            assert [(s.num_rows, s.n_groups, s.n_unique, s.n_null_key_rows, struct.pack("<d", s.entropy))
                    for s in (se,)] == [(s.num_rows, s.n_groups, s.n_unique, s.n_null_key_rows,
                                         struct.pack("<d", s.entropy)) for s in (sp,)]
            assert e.null_literal() == p.null_literal() and e.folded_nan_rows() == p.folded_nan_rows()
            assert sorted(n for _, n in e.topk(3)) == sorted(n for _, n in p.topk(3))
    joint = MutualInformation(["p3", "c700"]).compute_state_from(enc).frequencies
    assert joint.encoded_batches == 0


def test_dictionary_above_the_lds_threshold(gpu_device):
    """40,000 entries over 60,000 rows: the count kernel's global-atomic regime."""
    from deequ_amd import Table
    from deequ_amd.analyzers import CountDistinct, Distinctness, Entropy, Histogram, UniqueValueRatio, Uniqueness
    rows, entries = 60_000, 40_000
    assert entries > LDS_MAX
    rng = np.random.default_rng(3)
    # entries 0 and 1 far ahead, 2 .. 999 twenty rows each, the other 39,000 entries share the rest
    # (a handful of rows each): no tie straddles a cut at 2 or at 1,000 detail bins (_skewed)
    idx = np.concatenate([np.zeros(60, np.int32), np.ones(40, np.int32), np.repeat(np.arange(2, 1000), 20),
                          rng.integers(1000, entries, rows - 100 - 998 * 20)]).astype(np.int32)
    rng.shuffle(idx)
    col = pa.DictionaryArray.from_arrays(pa.array(idx, mask=rng.random(rows) < 0.01),
                                         pa.array([f"key-{i}" for i in range(entries)]))
    enc = Table.from_arrow(pa.table({"big": col}), device=gpu_device, max_batch_rows=8192)
    plain = Table.from_arrow(pa.table({"big": col.dictionary_decode()}), device=gpu_device, max_batch_rows=8192)
    _assert_decoded_equal(enc.batches[1]["big"], plain.batches[1]["big"])
    _assert_same_metrics(enc, plain, [Uniqueness(["big"]), Distinctness(["big"]), UniqueValueRatio(["big"]),
                                      CountDistinct(["big"]), Entropy("big"),
                                      Histogram("big", max_detail_bins=2), Histogram("big")])
    assert Uniqueness(["big"]).compute_state_from(enc).frequencies.encoded_batches == len(enc.batches)


@pytest.mark.parametrize("case", [h for h in GOLDEN["histograms"]
                                  if (h["fixture"], h["column"]) == ("dfMissing", "att1")],
                         ids=lambda c: c["cite"])
def test_reference_histogram_through_a_dictionary_column(case, gpu_device):
    from deequ_amd import Table
    from deequ_amd.analyzers import Histogram
    t = arrow_table("dfMissing")
    t = t.set_column(t.schema.get_field_index("att1"), "att1", t.column("att1").dictionary_encode())
    data = Table.from_arrow(t, device=gpu_device)
    assert data.batches[0]["att1"].encoded is not None
    d = Histogram("att1", max_detail_bins=case["max_detail_bins"]).calculate(data).value.get()
    assert d.number_of_bins == case["bins"] and set(d.values) == set(case["keys"])
    assert d.values["NullValue"].absolute == 6 and d.values["a"].absolute == 4


def test_profiler_and_state_provider(gpu_device, tmp_path):
    from deequ_amd import Table
    from deequ_amd.analyzers import HdfsStateProvider, Histogram
    from deequ_amd.profiles import ColumnProfiler, ColumnProfiles
    enc_arrow, plain_arrow = _parity_tables()
    enc = Table.from_arrow(enc_arrow.slice(0, 600), device=gpu_device, max_batch_rows=BATCH)
    plain = Table.from_arrow(plain_arrow.slice(0, 600), device=gpu_device, max_batch_rows=BATCH)
    got, ref = ColumnProfiler.profile(enc), ColumnProfiler.profile(plain)
    assert ColumnProfiles.to_json(list(got.profiles.values())) == ColumnProfiles.to_json(list(ref.profiles.values()))
    provider = HdfsStateProvider(str(tmp_path / "state"), allow_overwrite=True)
    analyzer = Histogram("p3")
    state = analyzer.compute_state_from(enc)
    assert state.frequencies.encoded_batches > 0
    provider.persist(analyzer, state)
    loaded = provider.load(analyzer)
    assert loaded.num_rows == state.num_rows
    # (a persisted Histogram state is the reference's: keyed by string, NULL folded into "NullValue")
    assert loaded.string_groups() == state.string_groups()
    plain_provider = HdfsStateProvider(str(tmp_path / "plain"), allow_overwrite=True)
    plain_provider.persist(analyzer, analyzer.compute_state_from(plain))
    assert (sorted(loaded.frequencies.export(), key=repr)
            == sorted(plain_provider.load(analyzer).frequencies.export(), key=repr))
    assert _canon(analyzer.compute_metric_from(loaded)) == _canon(analyzer.compute_metric_from(state))
