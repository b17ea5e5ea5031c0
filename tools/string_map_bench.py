"""String-producing functions (Trim / ToUpper / Substring / StringReplace): what closing a dictionary costs, and what a row pays afterwards.

Closing: D distinct values of 12..40 bytes, a third of them with 1..3 trailing spaces.  StringDictionary.close under ONE step, TRIM,
TO_UPPER and STRING_REPLACE("cd" -> "D"; the two constants join the dictionary, as a plan's would), by the host clock (it includes packing and uploading the dictionary, the copy of the distinct bytes back and the new
host dictionary) and, from the context's debug_timing lines, the step's two parts: the image kernels (length pass, scan, copy of
the base bytes, write pass) and the re-encode of the 2n-row domain (hash, insert, compact, sort, rank, codes, gather and the copy
back) -- against the images computed on the host by a single-threaded loop: CPython, one bytes.strip / bytes.upper / bytes.replace per value over
the packed heap (the images only: no sort, no codes).
Per-row cost: ROWS rows of codes of a 1e5-value dictionary, GROUP BY TRIM(s) against GROUP BY s with COUNT(*), alternating; the
run's time is the host clock around run + fetch (a device synchronise).  Writes one JSON document.

    python tools/string_map_bench.py [--distinct 10000000] [--rows 100000000] [--rounds 5] [--out profiles/string_map_bench.json]
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
from string_fn_bench import Stderr, dictionary_of, make_values, stats  # noqa: E402

TRIM, TO_UPPER, STRING_REPLACE = 412, 416, 480
NEEDLE, SUBSTITUTE = b"cd", b"D"


def note(text):
    print("[string_map_bench] " + text, file=sys.stderr, flush=True)


def spaced_values(n, seed):
    """string_fn_bench's values (sorted, distinct by their 8-letter index prefix) with the last 1..3 bytes of every third one turned
    into spaces: a trimmed value is then in nobody else's place, so TRIM adds n / 3 values and TO_UPPER n."""
    heap, offs = make_values(n, seed)
    rng = np.random.default_rng(seed + 1)
    pick = np.arange(0, n, 3)
    run = rng.integers(1, 4, len(pick))
    for k in range(1, 4):
        heap[offs[pick[run >= k] + 1] - k] = 32
    return heap, offs


def host_images(heap, offs, fn):
    big = heap.tobytes()
    o = offs.tolist()
    t0 = time.perf_counter()
    if fn == TRIM:
        out = [big[o[i]:o[i + 1]].strip(b" ") for i in range(len(o) - 1)]
    elif fn == STRING_REPLACE:
        out = [big[o[i]:o[i + 1]].replace(NEEDLE, SUBSTITUTE) for i in range(len(o) - 1)]
    else:
        out = [big[o[i]:o[i + 1]].upper() for i in range(len(o) - 1)]
    return out, time.perf_counter() - t0


def bench_close(ctx, n, reps):
    heap, offs = spaced_values(n, seed=n)
    d = dictionary_of(heap, offs)
    out = {"distinct": n, "heap_bytes": int(offs[-1]), "steps": {}}
    ctx.set_option("debug_timing", 1)
    with_consts, _remap = d.extend([NEEDLE, SUBSTITUTE])   # a replace step's constants are values of the dictionary it closes
    for name, fn in (("TRIM", TRIM), ("TO_UPPER", TO_UPPER), ("STRING_REPLACE", STRING_REPLACE)):
        note("closing %d values under %s" % (n, name))
        base, step = (with_consts, (fn, NEEDLE, SUBSTITUTE)) if fn == STRING_REPLACE else (d, (fn,))
        images, host_s = host_images(heap, offs, fn)
        new_values = len(set(images)) if n <= 1000000 else None
        del images
        maps, encodes, calls, size = [], [], [], 0
        for r in range(reps + 1):                          # the first call warms the code objects and the allocations
            with Stderr() as err:
                t0 = time.perf_counter()
                closed, remap = base.close([step], ctx)
                dt = time.perf_counter() - t0
            m = re.search(r"values (\d+) -> (\d+) map_ms ([0-9.]+) encode_ms ([0-9.]+)", err.text)
            assert m and int(m.group(1)) == len(base), err.text
            size = len(closed)
            assert size == int(m.group(2)) and len(remap) == len(base)
            del closed
            if r:
                maps.append(float(m.group(3)))
                encodes.append(float(m.group(4)))
                calls.append(dt * 1e3)
        mk, ek, ck = stats(maps), stats(encodes), stats(calls)
        out["steps"][name] = {"closed_size": size, "host_distinct_images": new_values,
                              "image_kernels_ms": mk, "reencode_2n_rows_ms": ek, "close_call_ms": ck,
                              "reencode_share_of_call": ek["median"] / ck["median"], "image_kernels_share_of_call": mk["median"] / ck["median"],
                              "host_side_rest_ms": ck["median"] - mk["median"] - ek["median"],
                              "host_loop": "CPython, single thread: bytes.strip(b' ') / bytes.upper() / bytes.replace(b'cd', b'D') per value over the packed heap (images only)",
                              "host_loop_ms": host_s * 1e3, "host_loop_over_image_kernels": host_s * 1e3 / mk["median"]}
    ctx.set_option("debug_timing", 0)
    return out


def bench_rows(rows, rounds):
    heap, offs = spaced_values(100000, seed=7)
    values = [heap[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    rng = np.random.default_rng(1)
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING)])
    ctx = ss.Context(0)
    idx = rng.integers(0, len(values), rows)
    spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n")
    runs = {}
    for name, key in (("group_by_trim", lambda: ss.Trim(ss.NamedAttribute("s"))), ("group_by_s", lambda: ss.NamedAttribute("s"))):
        note("per-row cost, %d rows, %s" % (rows, name))
        block = ss.DeviceBlock(schema, rows, ctx)
        op = ss.GroupAggregate(ss.ProjectNamedAttributes(["g"]), spec, None, ss.Compute(ss.CompoundExpression().AddAs("g", key()), ss.ScanView(block.view())))
        plan = ss.Plan(op, ctx, extra_strings=values)
        codes = plan.strings.encode(values, None)[idx].astype(np.int32)          # the rows in codes of THIS plan's dictionary
        ctx.check(ctx.lib.ssgpu_block_upload(block.handle, 0, codes.ctypes.data_as(C.c_void_p), None, 0, rows))
        ctx.synchronize()
        groups = len({v.strip(b" ") for v in values}) if name == "group_by_trim" else int(np.unique(idx).size)
        runs[name] = (plan, block, groups)
    times = {k: [] for k in runs}
    for r in range(rounds + 2):                            # two warm-up rounds: shapes, tables, allocations
        for k, (plan, _block, groups) in runs.items():     # back to back, alternating
            t0 = time.perf_counter()
            plan.run()
            got = plan.fetch()
            dt = time.perf_counter() - t0
            assert got.row_count() == groups and int(got.column(1).data.sum()) == rows, (k, got.row_count(), groups)
            if r >= 2:
                times[k].append(dt * 1e3)
    res = {k: dict(stats(v), rows_per_s=rows / (stats(v)["median"] * 1e-3), groups=runs[k][2], dictionary=len(runs[k][0].strings)) for k, v in times.items()}
    res["trim_over_plain"] = res["group_by_trim"]["median"] / res["group_by_s"]["median"]
    return dict(res, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", default="10000000")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = ss.Context(0)                                     # no device: an error, never a host number in the device's place
    doc = {"tool": "tools/string_map_bench.py", "close": [bench_close(ctx, int(n), a.reps) for n in a.distinct.split(",") if n],
           "per_row": bench_rows(a.rows, a.rounds) if a.rows else None}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
