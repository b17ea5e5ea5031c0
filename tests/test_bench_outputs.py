"""`bench.py --dump-outputs DIR`: the result of the timed path's last step as DIR/<column>.npy (float32 / float64), written from
inputs generated with fixed seeds, so that two builds of the project can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import supersonic_amd as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FetchedPlan(object):
    """what dump_outputs reads of a Plan whose result was fetched to the host: its result schema"""

    def __init__(self, schema):
        self.result_schema = schema


def _load(d, name):
    return np.load(os.path.join(str(d), name + ".npy"))


def test_dump_outputs_writes_every_column_keys_sorted_nulls_as_nan(tmp_path):
    schema = ss.TupleSchema([ss.Attribute("k1", ss.INT32), ss.Attribute("k2", ss.INT32), ss.Attribute("s", ss.INT64, ss.NULLABLE),
                             ss.Attribute("f", ss.FLOAT)])
    view = ss.View(schema, [np.array([2, 1, 1]), np.array([0, 5, 3]), (np.array([10, 20, 30]), np.array([False, True, False])),
                            np.array([0.5, 1.5, 2.5])])
    bench.dump_outputs(str(tmp_path), _FetchedPlan(schema), view, key_columns=2)
    assert _load(tmp_path, "k1").tolist() == [1, 1, 2] and _load(tmp_path, "k2").tolist() == [3, 5, 0]
    s = _load(tmp_path, "s")
    assert s.dtype == np.float64 and s[0] == 30 and np.isnan(s[1]) and s[2] == 10
    f = _load(tmp_path, "f")
    assert f.dtype == np.float32 and f.tolist() == [2.5, 1.5, 0.5]
    assert _load(tmp_path, "row_count").tolist() == [3.0]


def test_dump_outputs_writes_a_fixed_sample_of_a_large_result(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 1000)
    n = 5000
    schema = ss.TupleSchema([ss.Attribute("x", ss.INT64)])
    view = ss.View(schema, [np.arange(n)])
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), _FetchedPlan(schema), view)
    one, two = _load(tmp_path / "one", "x"), _load(tmp_path / "two", "x")
    assert one.tolist() == two.tolist()
    assert 0 < len(one) <= 1000 and (np.diff(one) > 0).all() and one[-1] < n
    assert _load(tmp_path / "one", "row_count").tolist() == [float(n)]


def _run_bench(out_dir, *extra):
    env = dict(os.environ)
    env.pop("SSGPU_SPECIALIZE", None)
    env.pop("SSGPU_GROUP_DENSE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--rows", "1000000",
                        "--dump-outputs", str(out_dir)] + list(extra), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_headline_result(tmp_path):
    line = _run_bench(tmp_path)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert not {"configs", "cpu_baseline", "default_options"} & set(line)      # a plain run measures its headline only
    got = [_load(tmp_path, n) for n in ("sum_s", "cnt", "sum_c", "min_d", "max_d0", "sum_d1", "sum_p")]
    assert all(g.dtype == np.float64 and g.shape == (1,) for g in got)
    assert [g[0] for g in got] == [float(v) for v in line["result_row"]]
    assert _load(tmp_path, "row_count").tolist() == [1.0]


@pytest.mark.gpu
def test_bench_dumps_a_seeded_sample_of_a_large_device_result(tmp_path):
    _run_bench(tmp_path, "--query", "sort")
    d = _load(tmp_path, "d")
    assert _load(tmp_path, "row_count").tolist() == [1e6]
    assert 0 < len(d) < 1000000 and (np.diff(d) >= 0).all()
    assert all(len(_load(tmp_path, n)) == len(d) for n in ("a", "b", "c", "d0", "d1", "d2", "d3"))
