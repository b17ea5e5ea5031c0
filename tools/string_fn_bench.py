"""Functions of a STRING value (Length / StringOffset / StringContains): what the dictionary tables cost to build and to read.

Table build: D distinct values of 12..40 bytes, one 5-byte needle.  ssgpu_dict_eval on the device -- pack + upload of the
dictionary and the kernel, each between device events (the context's debug_timing line), and the whole call by the host clock
(it ends in a stream synchronise and includes the copy of the table back) -- against the same table computed on the host by a
single-threaded loop: CPython, one bytes.find (memmem) per value over the packed heap.
Per-row cost: ROWS rows of codes of a 1e5-value dictionary, COUNT(*) WHERE StringContains(s, c) against COUNT(*) WHERE s = c on
the same block, alternating, interpreted and specialised kernels; the run's time is the host clock around run + fetch of the one
result row (a device synchronise).  Writes one JSON document.

    python tools/string_fn_bench.py [--distinct 100000,10000000] [--rows 100000000] [--rounds 10] [--out profiles/string_fn_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import supersonic_amd as ss  # noqa: E402

NEEDLE = b"abcda"


def make_values(n, seed):
    """n distinct values in sorted order, packed: 8 letters a..p spelling the index (so the order of generation is the dictionary's
    order), then 4..32 letters a..d -- the needle occurs in a few percent of them."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(12, 41, n)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    heap = rng.integers(97, 101, int(offs[-1]), dtype=np.uint8)
    idx = np.arange(n, dtype=np.int64)
    for k in range(8):
        heap[offs[:-1] + k] = 97 + ((idx >> (4 * (7 - k))) & 15)
    return heap, offs


def dictionary_of(heap, offs):
    """ssgpu_dict_create over the packed values without a Python object per value."""
    n = len(offs) - 1
    lib = ss._lib.load()
    ptrs = (heap.ctypes.data + offs[:-1]).astype(np.uint64)
    lens = np.diff(offs).astype(np.int32)
    h = C.c_void_p()
    rc = lib.ssgpu_dict_create(C.cast(ptrs.ctypes.data, C.POINTER(C.c_char_p)), lens.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(h))
    assert rc == 0 and lib.ssgpu_dict_size(h) == n
    d = ss.StringDictionary.__new__(ss.StringDictionary)
    d.lib, d.handle = lib, h
    return d


def host_table(heap, offs, needle):
    big = heap.tobytes()
    o = offs.tolist()
    t0 = time.perf_counter()
    out = [big.find(needle, o[i], o[i + 1]) for i in range(len(o) - 1)]
    dt = time.perf_counter() - t0
    return np.array([0 if p < 0 else p - o[i] + 1 for i, p in enumerate(out)], np.int32), dt


class Stderr(object):
    """The library's own lines on file descriptor 2 during a call."""
    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def note(text):
    print("[string_fn_bench] " + text, file=sys.stderr, flush=True)


def bench_build(ctx, n, reps):
    note("table build over %d values" % n)
    heap, offs = make_values(n, seed=n)
    d = dictionary_of(heap, offs)
    want, host_s = host_table(heap, offs, NEEDLE)
    upload, kernel, call = [], [], []
    ctx.set_option("debug_timing", 1)
    for r in range(reps + 1):                              # the first call warms the code object and the allocations
        with Stderr() as err:
            t0 = time.perf_counter()
            got = d.eval(ss.StringDictionary.STRING_OFFSET, NEEDLE, context=ctx)
            dt = time.perf_counter() - t0
        m = re.search(r"upload_ms ([0-9.]+) kernel_ms ([0-9.]+)", err.text)
        assert m, err.text
        assert np.array_equal(got, want)
        if r:
            upload.append(float(m.group(1)))
            kernel.append(float(m.group(2)))
            call.append(dt * 1e3)
    ctx.set_option("debug_timing", 0)
    heap_bytes = int(offs[-1])
    k = stats(kernel)
    return {"distinct": n, "heap_bytes": heap_bytes, "needle": NEEDLE.decode(), "values_with_a_match": int((want > 0).sum()),
            "device_pack_and_upload_ms": stats(upload), "device_kernel_ms": k, "device_call_ms": stats(call),
            "kernel_heap_gb_per_s": heap_bytes / (k["median"] * 1e-3) / 1e9,
            "host_loop": "CPython, single thread: bytes.find(needle, start, end) (memmem) per value over the packed heap", "host_loop_ms": host_s * 1e3,
            "host_over_device_upload_plus_kernel": host_s * 1e3 / (stats(upload)["median"] + k["median"])}


def bench_rows(rows, rounds):
    heap, offs = make_values(100000, seed=7)
    values = [heap[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    equal_to = values[len(values) // 2]
    extra = values + [NEEDLE]
    rng = np.random.default_rng(1)
    schema = ss.TupleSchema([ss.Attribute("s", ss.STRING)])
    out = {"rows": rows, "distinct": len(extra), "modes": {}}
    for mode, name in ((0, "interpreted"), (1, "specialized")):
        note("per-row cost, %d rows, %s" % (rows, name))
        ctx = ss.Context(0)
        ctx.set_option("specialize", mode)
        block = ss.DeviceBlock(schema, rows, ctx)
        codes = rng.integers(0, len(extra), rows).astype(np.int32)
        ctx.check(ctx.lib.ssgpu_block_upload(block.handle, 0, codes.ctypes.data_as(C.c_void_p), None, 0, rows))
        ctx.synchronize()
        view = block.view()

        def count_where(pred):
            spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n")
            return ss.Plan(ss.ScalarAggregate(spec, ss.Filter(pred, ss.ProjectAllAttributes(), ss.ScanView(view))), ctx, extra_strings=extra)
        plans = {"contains": count_where(ss.StringContains(ss.NamedAttribute("s"), ss.ConstString(NEEDLE))),
                 "equal": count_where(ss.Equal(ss.NamedAttribute("s"), ss.ConstString(equal_to)))}
        d = plans["contains"].strings
        assert len(d) == len(extra) and len(plans["equal"].strings) == len(extra)
        table = d.eval(ss.StringDictionary.STRING_OFFSET, NEEDLE, context=ctx)
        want = {"contains": int((table[codes] > 0).sum()), "equal": int((codes == d.code_of(equal_to)).sum())}
        times = {k: [] for k in plans}
        for r in range(rounds + 2):                        # two warm-up rounds: code objects, tables, allocations
            for k, plan in plans.items():                   # back to back, alternating
                t0 = time.perf_counter()
                plan.run()
                got = plan.fetch()
                dt = time.perf_counter() - t0
                assert int(got.column(0).data[0]) == want[k], (k, got.column(0).data[0], want[k])
                if r >= 2:
                    times[k].append(dt * 1e3)
        res = {k: dict(stats(v), rows_per_s=rows / (stats(v)["median"] * 1e-3), count=want[k]) for k, v in times.items()}
        res["contains_over_equal"] = res["contains"]["median"] / res["equal"]["median"]
        res["compiled_stages"] = {k: p.specialized() for k, p in plans.items()}
        out["modes"][name] = res
        del plans, view, block
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", default="100000,10000000")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = ss.Context(0)                                     # no device: an error, never a host number in the device's place
    doc = {"tool": "tools/string_fn_bench.py", "table_build": [bench_build(ctx, int(n), a.reps) for n in a.distinct.split(",") if n],
           "per_row": bench_rows(a.rows, a.rounds) if a.rows else None}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
