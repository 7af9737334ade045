"""bench.py --dump-outputs: the row of the last timed step lands in DIR/row.npy as float64, one
value per scalar of the row in order, NULL as NaN (bench.dump_outputs; no GPU involved)."""
import numpy as np

import bench


def test_row_is_flattened_to_float64(tmp_path):
    row = [1_000_000_000, None, 952723355687.0, (950002794.0, 1002.8637407217984, 9.6e14), -18653.0]
    out = tmp_path / "nested" / "dir"
    bench.dump_outputs(str(out), row)
    got = np.load(out / "row.npy")
    assert got.dtype == np.float64 and got.shape == (7,)
    exp = np.array([1e9, np.nan, 952723355687.0, 950002794.0, 1002.8637407217984, 9.6e14, -18653.0])
    assert np.array_equal(got, exp, equal_nan=True)
    assert [p.name for p in out.iterdir()] == ["row.npy"]
