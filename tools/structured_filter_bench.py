"""ForeignFilter and RowidMergeJoin against the formulation the library offered before them: a UNIQUE INNER HashJoin whose rhs table
carries an explicit row-number column.

Shape: ROWS input rows x 4 columns (fk INT64, a INT64, b INT32, d DOUBLE) resident on the device, a TABLE-row filter / parent table,
about half of the input rows matching the filter.  Per operator two plans that compute the same rows --

  ForeignFilter(id, fk, filter, input)              against  HashJoin(INNER, fk, id, [rn AS fk, a, b, d], UNIQUE, input, filter + rn)
  RowidMergeJoin(fk, [a, b, d, w, v], input, parent)  against  HashJoin(INNER, fk, rn, [a, b, d, w, v], UNIQUE, input, parent + rn)

-- each as the plan's root (the rows are materialised) and under a ScalarAggregate (COUNT, SUM of a result column), where the result
is one row and the probe is what is left.  The pairs run back to back, alternating, after two warm-up rounds; a run's time is the host
clock around run + a device synchronise.  The results of a pair are compared (row count, the aggregate row) before anything is timed.

A HashJoin rebuilds its index at the start of every run, a ForeignFilter verifies the order of its table there, a RowidMergeJoin does
neither: that FIXED part is measured on its own, as the same plan over a ONE-row input (everything a run costs that does not depend
on the input), and reported next to the 100 M-row run; `rows_ms` is their difference.  Writes one JSON document.

    python tools/structured_filter_bench.py [--rows 100000000] [--table 1000000] [--rounds 10] [--specialize 0,1] [--out profiles/structured_filter_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import supersonic_amd as ss  # noqa: E402


def note(text):
    print("[structured_filter_bench] " + text, file=sys.stderr, flush=True)


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def device_view(ctx, schema, columns, rows):
    block = ss.DeviceBlock(schema, max(rows, 1), ctx)
    for i, col in enumerate(columns):
        col = np.ascontiguousarray(col)
        if rows:
            ctx.check(ctx.lib.ssgpu_block_upload(block.handle, i, col.ctypes.data_as(C.c_void_p), None, 0, rows))
    ctx.synchronize()
    return block.view(rows)


INPUT = [("fk", ss.INT64), ("a", ss.INT64), ("b", ss.INT32), ("d", ss.DOUBLE)]


def input_columns(rows, key_range, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, key_range, rows), rng.integers(-1000, 1000, rows), rng.integers(-1000, 1000, rows).astype(np.int32),
            rng.integers(-4000, 4000, rows) * 0.25]


def schema_of(pairs):
    return ss.TupleSchema([ss.Attribute(n, t) for n, t in pairs])


def timed(ctx, plan, view):
    t0 = time.perf_counter()
    res = plan.run(view)
    ctx.synchronize()
    rows = ctx.lib.ssgpu_result_row_count(res)
    dt = time.perf_counter() - t0
    assert rows >= 0, ctx.last_error()
    return dt * 1e3, rows


def compare(ctx, name, plans, big, one, rounds, aggregated):
    """plans: {"new": Plan, "hash_join": Plan}.  -> per plan: the run over `big`, the fixed part (over `one`), their difference."""
    first = {}
    for k, plan in plans.items():
        _ms, rows = timed(ctx, plan, big)
        got = plan.fetch() if aggregated else None
        first[k] = (rows, None if got is None else [got.column(i).data.tolist() for i in range(got.column_count())])
    assert first["new"] == first["hash_join"], (name, first)
    times = {k: {"run": [], "fixed": []} for k in plans}
    for r in range(rounds + 2):                            # two warm-up rounds: code objects, allocations, the compiled kernels
        for k, plan in plans.items():                       # back to back, alternating
            ms, _rows = timed(ctx, plan, big)
            fixed, _rows = timed(ctx, plan, one)
            if r >= 2:
                times[k]["run"].append(ms)
                times[k]["fixed"].append(fixed)
    out = {"result_rows": first["new"][0]}
    for k, t in times.items():
        run, fixed = stats(t["run"]), stats(t["fixed"])
        out[k] = {"run_ms": run, "fixed_ms_one_row_input": fixed, "rows_ms": run["median"] - fixed["median"], "compiled_stages": plans[k].specialized()}
    out["new_over_hash_join_run"] = out["new"]["run_ms"]["median"] / out["hash_join"]["run_ms"]["median"]
    out["new_over_hash_join_rows"] = out["new"]["rows_ms"] / out["hash_join"]["rows_ms"]
    note("%s: new %.3f ms (fixed %.3f), HashJoin %.3f ms (fixed %.3f)" % (name, out["new"]["run_ms"]["median"], out["new"]["fixed_ms_one_row_input"]["median"],
                                                                          out["hash_join"]["run_ms"]["median"], out["hash_join"]["fixed_ms_one_row_input"]["median"]))
    return out


def bench(rows, table, rounds, specialize):
    ctx = ss.Context(0)                                     # no device: an error, never a host number in the device's place
    ctx.set_option("specialize", specialize)
    rng = np.random.default_rng(3)
    out = {"specialize": specialize}
    count_sum = lambda col: ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n").AddAggregation(ss.SUM, col, "s")     # noqa: E731

    # ---- ForeignFilter: `table` ascending keys out of [0, 2 * table): half of the uniform input keys are among them -------------------
    note("ForeignFilter, specialize = %d: building the inputs" % specialize)
    fkeys = np.flatnonzero(rng.random(2 * table) < 0.5).astype(np.int64)
    cols = input_columns(rows, 2 * table, seed=1)
    big = device_view(ctx, schema_of(INPUT), cols, rows)
    one = device_view(ctx, schema_of(INPUT), [c[:1] for c in cols], 1)
    filt = device_view(ctx, schema_of([("id", ss.INT64)]), [fkeys], len(fkeys))
    filt_rn = device_view(ctx, schema_of([("id", ss.INT64), ("rn", ss.INT64)]), [fkeys, np.arange(len(fkeys), dtype=np.int64)], len(fkeys))
    ff = lambda: ss.ForeignFilter(ss.ProjectNamedAttribute("id"), ss.ProjectNamedAttribute("fk"), ss.ScanView(filt), ss.ScanView(big))     # noqa: E731
    hj = lambda: ss.HashJoin(ss.INNER, ss.ProjectNamedAttribute("fk"), ss.ProjectNamedAttribute("id"),     # noqa: E731
                             ss.CompoundMultiSourceProjector().add(1, ss.ProjectNamedAttributeAs("rn", "fk")).add(0, ss.ProjectNamedAttributes(["a", "b", "d"])),
                             ss.UNIQUE, ss.ScanView(big), ss.ScanView(filt_rn))
    out["foreign_filter"] = {
        "filter_rows": len(fkeys),
        "materialised": compare(ctx, "ForeignFilter, materialised", {"new": ss.Plan(ff(), ctx), "hash_join": ss.Plan(hj(), ctx)}, big, one, rounds, False),
        "aggregated": compare(ctx, "ForeignFilter, aggregated", {"new": ss.Plan(ss.ScalarAggregate(count_sum("fk"), ff()), ctx),
                                                                 "hash_join": ss.Plan(ss.ScalarAggregate(count_sum("fk"), hj()), ctx)}, big, one, rounds, True)}
    del big, one, filt, filt_rn, cols

    # ---- RowidMergeJoin: every input key is a row of the `table`-row parent ------------------------------------------------------------
    note("RowidMergeJoin, specialize = %d: building the inputs" % specialize)
    cols = input_columns(rows, table, seed=2)
    big = device_view(ctx, schema_of(INPUT), cols, rows)
    one = device_view(ctx, schema_of(INPUT), [c[:1] for c in cols], 1)
    w, v = rng.integers(-1000, 1000, table), rng.integers(-4000, 4000, table) * 0.25
    parent = device_view(ctx, schema_of([("w", ss.INT64), ("v", ss.DOUBLE)]), [w, v], table)
    parent_rn = device_view(ctx, schema_of([("rn", ss.INT64), ("w", ss.INT64), ("v", ss.DOUBLE)]), [np.arange(table, dtype=np.int64), w, v], table)
    proj = lambda: ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttributes(["a", "b", "d"])).add(1, ss.ProjectNamedAttributes(["w", "v"]))     # noqa: E731
    rmj = lambda: ss.RowidMergeJoin(ss.ProjectNamedAttribute("fk"), proj(), ss.ScanView(big), ss.ScanView(parent))     # noqa: E731
    hj2 = lambda: ss.HashJoin(ss.INNER, ss.ProjectNamedAttribute("fk"), ss.ProjectNamedAttribute("rn"), proj(), ss.UNIQUE, ss.ScanView(big), ss.ScanView(parent_rn))     # noqa: E731
    out["rowid_merge_join"] = {
        "parent_rows": table,
        "materialised": compare(ctx, "RowidMergeJoin, materialised", {"new": ss.Plan(rmj(), ctx), "hash_join": ss.Plan(hj2(), ctx)}, big, one, rounds, False),
        "aggregated": compare(ctx, "RowidMergeJoin, aggregated", {"new": ss.Plan(ss.ScalarAggregate(count_sum("w"), rmj()), ctx),
                                                                  "hash_join": ss.Plan(ss.ScalarAggregate(count_sum("w"), hj2()), ctx)}, big, one, rounds, True)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--table", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--specialize", default="0,1")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    doc = {"tool": "tools/structured_filter_bench.py", "rows": a.rows, "columns": [n for n, _t in INPUT], "table_rows": a.table, "rounds": a.rounds,
           "modes": [bench(a.rows, a.table, a.rounds, int(m)) for m in a.specialize.split(",") if m]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
