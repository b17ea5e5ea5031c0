"""PARSE_STRING (ParseStringQuiet / ParseStringNulling): what the parse tables cost to build and to read.

Table build: D distinct decimal strings -- the values' indices spelled with a sign, a fraction or an exponent now and then --
through ssgpu_dict_parse per target type: pack + upload of the dictionary, the kernel, and for a floating target the host's
share (read-back of the failure bytes, strtof / strtod of what the device left, the patched tables' way back), each between
device events (the context's debug_timing line), and the whole call by the host clock (it ends in a stream synchronise and
includes the copy of both tables back).  host_share = the host's share of the call.
Per-row cost: ROWS rows of codes of a 1e5-value dictionary, SUM(ParseStringNulling(INT64, s)) against SUM of an INT64 column
that holds the same numbers, alternating, interpreted and specialised kernels; the run's time is the host clock around
run + fetch of the one result row.  Writes one JSON document.

    python tools/string_parse_bench.py [--distinct 10000000] [--rows 100000000] [--rounds 10] [--out profiles/string_parse_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import supersonic_amd as ss  # noqa: E402
from string_fn_bench import Stderr, dictionary_of, stats  # noqa: E402

TARGETS = [("INT32", ss.INT32), ("UINT32", ss.UINT32), ("INT64", ss.INT64), ("UINT64", ss.UINT64), ("FLOAT", ss.FLOAT), ("DOUBLE", ss.DOUBLE), ("BOOL", ss.BOOL)]


def note(text):
    print("[string_parse_bench] " + text, file=sys.stderr, flush=True)


def make_decimals(n):
    """n distinct decimal strings, packed (heap, offsets), not sorted: index i as 9 digits, every 7th with a '-' in front, every 5th
    with the fraction ".25" behind (no integer), of the others every 11th with the exponent "e3" -- all inside the floating fast path."""
    idx = np.arange(n, dtype=np.int64)
    cells = np.zeros((n, 13), np.uint8)                  # [sign][9 digits][up to 3 more]; keep: which cells a value has
    keep = np.zeros((n, 13), bool)
    cells[:, 0], keep[:, 0] = 45, idx % 7 == 0
    for k in range(9):
        cells[:, 1 + k] = 48 + (idx // 10 ** (8 - k)) % 10
    keep[:, 1:10] = True
    frac = idx % 5 == 0
    cells[frac, 10:13], keep[frac, 10:13] = (46, 50, 53), True
    ex = (idx % 11 == 0) & ~frac
    cells[ex, 10:12], keep[ex, 10:12] = (101, 51), True
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=offs[1:])
    return cells[keep], offs


def bench_build(ctx, n, reps):
    heap, offs = make_decimals(n)
    d = dictionary_of(heap, offs)
    out = {"distinct": n, "heap_bytes": int(offs[-1]), "targets": {}}
    ctx.set_option("debug_timing", 1)
    for name, t in TARGETS:
        note("tables over %d values to %s" % (n, name))
        upload, kernel, host, call, resolved = [], [], [], [], 0
        for r in range(reps + 1):                          # the first call warms the code object and the allocations
            with Stderr() as err:
                t0 = time.perf_counter()
                _values, failed, resolved = d.parse(t, context=ctx)
                dt = time.perf_counter() - t0
            m = re.search(r"upload_ms ([0-9.]+) kernel_ms ([0-9.]+) host_ms ([0-9.]+)", err.text)
            assert m, err.text
            if r:
                upload.append(float(m.group(1)))
                kernel.append(float(m.group(2)))
                host.append(float(m.group(3)))
                call.append(dt * 1e3)
        k, c, h = stats(kernel), stats(call), stats(host)
        out["targets"][name] = {"device_pack_and_upload_ms": stats(upload), "device_kernel_ms": k, "host_ms": h, "call_ms": c, "host_resolved": resolved,
                                "failed": int(failed.sum()), "host_share_of_call": h["median"] / c["median"],
                                "kernel_heap_gb_per_s": int(offs[-1]) / (k["median"] * 1e-3) / 1e9}
    ctx.set_option("debug_timing", 0)
    return out


def bench_rows(rows, rounds):
    n = 100000
    numbers = np.arange(n, dtype=np.int64) * 7 - 350000
    values = [b"%d" % v for v in numbers]
    rng = np.random.default_rng(1)
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING), ss.Attribute("v", ss.INT64)])
    out = {"rows": rows, "distinct": n, "modes": {}}
    for mode, name in ((0, "interpreted"), (1, "specialized")):
        note("per-row cost, %d rows, %s" % (rows, name))
        ctx = ss.Context(0)
        ctx.set_option("specialize", mode)
        block = ss.DeviceBlock(schema, rows, ctx)
        view = block.view()

        def sum_of(expr):
            spec = ss.AggregationSpecification().AddAggregation(ss.SUM, "x", "sum")
            return ss.Plan(ss.ScalarAggregate(spec, ss.Compute(ss.CompoundExpression().AddAs("x", expr), ss.ScanView(view))), ctx, extra_strings=values)
        plans = {"parse": sum_of(ss.ParseStringNulling(ss.INT64, ss.NamedAttribute("s"))), "column": sum_of(ss.NamedAttribute("v"))}
        d = plans["parse"].strings
        assert len(d) == n
        code_of_number = np.array([d.code_of(v) for v in values], np.int32)
        pick = rng.integers(0, n, rows)
        codes, ints = code_of_number[pick], numbers[pick]
        ctx.check(ctx.lib.ssgpu_block_upload(block.handle, 0, codes.ctypes.data_as(C.c_void_p), None, 0, rows))
        ctx.check(ctx.lib.ssgpu_block_upload(block.handle, 1, ints.ctypes.data_as(C.c_void_p), None, 0, rows))
        ctx.synchronize()
        want = int(ints.sum())
        del pick, codes, ints
        times = {k: [] for k in plans}
        for r in range(rounds + 2):                        # two warm-up rounds: code objects, tables, allocations
            for k, plan in plans.items():                   # back to back, alternating
                t0 = time.perf_counter()
                plan.run()
                got = plan.fetch()
                dt = time.perf_counter() - t0
                assert int(got.column(0).data[0]) == want, (k, got.column(0).data[0], want)
                if r >= 2:
                    times[k].append(dt * 1e3)
        res = {k: dict(stats(v), rows_per_s=rows / (stats(v)["median"] * 1e-3)) for k, v in times.items()}
        res["parse_over_column"] = res["parse"]["median"] / res["column"]["median"]
        res["compiled_stages"] = {k: p.specialized() for k, p in plans.items()}
        out["modes"][name] = res
        del plans, view, block
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", default="10000000")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = ss.Context(0)                                     # no device: an error, never a host number in the device's place
    doc = {"tool": "tools/string_parse_bench.py", "table_build": [bench_build(ctx, int(n), a.reps) for n in a.distinct.split(",") if n],
           "per_row": bench_rows(a.rows, a.rounds) if a.rows else None}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
