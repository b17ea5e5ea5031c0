"""File -> device block for a View file with a STRING key: the device path (FileInput(..., device_strings=True): lengths and bytes
staged into HBM, dictionary built and codes written by string_dict_kernels.hip) against the host path the library had before
(read_view_file, the plan's StringDictionary over collect_strings, encode, upload).  Prints one JSON line.

    python tools/string_file_bench.py [--rows 10000000] [--distinct 100000] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import supersonic_amd as ss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=0, help="rows of the host-path run (0: --rows)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    # keys of 6..18 bytes (12 on average), 5 % NULL; an INT64 value column
    lens = rng.integers(6, 19, a.distinct)
    keys = np.array(sorted({bytes(rng.integers(97, 123, n, dtype=np.uint8)) for n in lens}), dtype=object)
    schema = ss.TupleSchema([ss.Attribute("key", ss.STRING, ss.NULLABLE), ss.Attribute("v", ss.INT64)])
    ctx = ss.Context(0)
    tmp = tempfile.mkdtemp()

    def make(rows, name):
        path = os.path.join(tmp, name)
        out = ss.FileOutput(path)
        for lo in range(0, rows, 1 << 20):
            n = min(1 << 20, rows - lo)
            out.Write(ss.View(schema, [ss.Column(keys[rng.integers(0, len(keys), n)], rng.random(n) < 0.05), rng.integers(0, 1 << 40, n)]))
        out.Finalize()
        return path

    path = make(a.rows, "dev.ssv")
    size = os.path.getsize(path)
    dev_s = []
    for _ in range(a.reps + 1):                  # the first read warms the page cache and the library's allocations
        t0 = time.perf_counter()
        blk = ss.FileInput(schema, path, ctx, device_strings=True)
        dev_s.append(time.perf_counter() - t0)
        assert blk.row_count() == a.rows
        n_dict = len(blk.dictionary)
        del blk
    dev = min(dev_s[1:])
    host_rows = a.host_rows or a.rows
    hpath = path if host_rows == a.rows else make(host_rows, "host.ssv")
    t0 = time.perf_counter()
    view = ss.read_view_file(schema, hpath)
    t1 = time.perf_counter()
    plan = ss.Plan(ss.Project(ss.ProjectAllAttributes(), ss.ScanView(view)), ctx)     # StringDictionary(collect_strings(...))
    t2 = time.perf_counter()
    plan._columns_for(view)                      # encode + upload
    ctx.synchronize()
    t3 = time.perf_counter()
    host = t3 - t0
    line = {"bench": "string_file", "rows": a.rows, "distinct": int(n_dict), "file_bytes": size,
            "device_path_s": round(dev, 4), "device_rows_per_s": round(a.rows / dev), "device_file_GBps": round(size / dev / 1e9, 3),
            "device_runs_s": [round(x, 4) for x in dev_s],
            "host_rows": host_rows, "host_path_s": round(host, 3), "host_read_s": round(t1 - t0, 3), "host_dict_s": round(t2 - t1, 3),
            "host_encode_upload_s": round(t3 - t2, 3), "host_rows_per_s": round(host_rows / host)}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
