"""bench.py --dump-outputs (dump_outputs) and the command line of a plain run, on the host: the files are float32 / float64, stay
within 64 MB, hold the junction table in a fixed order, and a table too large for that is the same seeded sample every time."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake_rows(n, seed=1):
    from portcullis_amd import ffi

    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=ffi.ROW_DTYPE)
    for f in ffi.ROW_DTYPE.names:
        if f.startswith("_"):
            continue
        base = ffi.ROW_DTYPE[f].base
        shape = (n,) + ffi.ROW_DTYPE[f].shape
        if base.kind == "f":
            rows[f] = rng.random(shape)
        else:
            rows[f] = rng.integers(0, min(np.iinfo(base).max, 1 << 30), shape, dtype=np.int64).astype(base)
    rows["refid"] = rng.integers(0, 25, n)
    return rows


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_whole_table_in_a_fixed_order(tmp_path):
    import bench

    rows = fake_rows(1000)
    regs = {t: {k: 10 * t + i for i, k in enumerate(bench.REGION_FIELDS)} for t in (2, 0, 1)}
    n = bench.dump_outputs(str(tmp_path / "a"), rows, regs)
    got = load_dir(tmp_path / "a")
    assert n == sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in got)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["rows_index"], np.arange(1000))
    order = np.lexsort((rows["cons_strand"], rows["read_strand"], rows["end"], rows["start"], rows["refid"]))
    for f in rows.dtype.names:
        if not f.startswith("_"):
            assert np.array_equal(got["rows_" + f], rows[f][order]), f
    assert got["rows_jad"].shape == (1000, 20) and got["rows_entropy"].dtype == np.float64
    assert got["regions"].shape == (3, 1 + len(bench.REGION_FIELDS)) and list(got["regions"][:, 0]) == [0, 1, 2]
    assert got["regions"][2, -1] == 20 + len(bench.REGION_FIELDS) - 1
    # the same rows in another order give the same files
    bench.dump_outputs(str(tmp_path / "b"), rows[::-1].copy(), regs)
    again = load_dir(tmp_path / "b")
    assert all(np.array_equal(got[k], again[k]) for k in got)


def test_large_table_is_a_seeded_sample_within_64_mb(tmp_path):
    import bench

    rows = fake_rows(300_000)
    n1 = bench.dump_outputs(str(tmp_path / "a"), rows)
    n2 = bench.dump_outputs(str(tmp_path / "b"), rows)
    assert n1 == n2 <= bench.DUMP_BYTES <= 64 * 10**6 and n1 > bench.DUMP_BYTES - (1 << 20)
    a, b = load_dir(tmp_path / "a"), load_dir(tmp_path / "b")
    assert "regions" not in a and a.keys() == b.keys()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["rows_index"].astype(np.int64)
    assert 0 < len(idx) < len(rows) and np.all(np.diff(idx) > 0) and idx[-1] < len(rows)
    order = np.lexsort((rows["cons_strand"], rows["read_strand"], rows["end"], rows["start"], rows["refid"]))
    assert np.array_equal(a["rows_start"], rows["start"][order[idx]].astype(np.float64))


def test_command_line():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr
