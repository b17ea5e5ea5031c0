"""The pipeline kernel on the device with its tile loop, its finish and its count / scan / store passes ON their edges, against the
independent reference of tests/pipeline_reference.py.

ssgpu_pipeline_kernel as run_scalar_agg and run_materialize launch it (supersonic_amd/csrc/runtime.cpp, pipeline_kernels.hip), with
ssgpu_finish_slots_kernel, ssgpu_scan_counts_kernel and the count and store passes, carries every other operator.  The parity tests
feed it random data at sizes where a workgroup takes ONE tile; here `grid_limit` gives a workgroup two to six trips at a few thousand
rows, `tile_map` permutes which workgroup owns which tile, and `pipeline_reference` plants the inputs:
  A. the tile loop of ScalarAggregate: 512 / 1024 / 2048-row tiles on 1 / 2 / 3 / 8 / 16 workgroups, g .. 3 g - 1 tiles, last tiles of
     T / 1 / 2 / 3 / T - 1 rows; the unique MIN and MAX on row 0, the end of a full tile, the start of the partial tile, the second row
     of a lane pair and row n - 1; the only non-NULL value for FIRST in the last tile, for LAST in tile 0 (row 0 included); a column
     that is NULL everywhere; FIRST on the last register slot, LAST on the first LDS slot;
  B. a NaN of a floating MIN / MAX in a workgroup's second tile, in the partial tile, leading, leading but dropped by the Filter;
  C. plans of 8, 9, 64 and 65 aggregations, every kind once on slot 7 and once on slot 8; fuse_emit 0 and 1;
  D. 8 / 9, 4 / 5, 2 / 3 staged arrays at 512 / 1024 / 2048-row tiles (the register prefetch file exactly full, and one array beyond
     it) in columns of 8, 4 and 1 bytes, a NULLABLE column without an is_null vector, a BOOL column at an odd device address;
  E. the materialising Filter: 2048 m + d rows, six survivor patterns, grid_limit 1 / 3 / 8, tile_map 0 / 1 (a count tile of 2048 rows
     over store tiles of 512, the last one partial); 8193 store tiles (the scan's second trip); a result that is an arena, then
     buffers of its own, then an arena again;
  F. a Compute behind a GroupAggregate that reads its row count on the device: 0, 1, T - 1, T, T + 1 groups, async_handoff 1 and 0;
  G. the one inexact DOUBLE sum, within 1 ULP of math.fsum.
Every test builds its own context, runs every plan at least twice over an input, compares EVERY run with the reference -- rows in
order (F: sorted), bit for bit, no tolerance (G: 1 ULP, the bound of DESIGN.md section 5) -- and asserts the `counters()` facts the
case states (tests/test_pipeline_reference_cpu.py checks reference, facts and planted rows without a GPU).

Out of reach at test size: tile indices and row ids beyond 2^31 (tests/test_beyond_2_32_rows_gpu.py holds the row ids), more than
65536 store tiles (the three-kernel scan: 33 M rows), a grid of cu_count x wgs_per_cu workgroups making several trips (the 100 M-row
property tests), and folds of partial states across shards, which test_partial_state_fold_across_shards already holds."""
import time

import numpy as np
import pytest

import pipeline_reference as pr
import supersonic_amd as ss
from helpers import assert_cols_equal, schema_list, sort_rows, to_cols, ulp_distance

pytestmark = pytest.mark.gpu

_expected = {}       # the reference's answer per input, shared by the cases that differ in context options only


def expected(case):
    if case.data_key not in _expected:
        _expected[case.data_key] = case.expected()
    return _expected[case.data_key]


def context(options, specialize=0):
    ctx = ss.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_option("specialize", specialize)
    return ctx


def check_run(plan, case, where):
    schema, want = expected(case)
    got = plan.fetch()
    assert schema_list(got.schema()) == schema, where
    assert got.row_count() == len(want[0][0]), (where, got.row_count(), len(want[0][0]))
    inexact = case.notes.get("inexact", ())
    exact = [i for i, s in enumerate(schema) if s[0] not in inexact]
    cols = to_cols(got)
    assert_cols_equal([cols[i] for i in exact], [want[i] for i in exact], context=where)
    for i in (i for i in range(len(schema)) if i not in exact):
        ulp = ulp_distance(cols[i][0], want[i][0])
        print("%s %s: got %r, math.fsum %r, %g ULP" % (where, schema[i][0], cols[i][0][0], want[i][0][0], ulp[0]))
        assert not cols[i][1][0] and ulp[0] <= 1, (where, schema[i][0], cols[i][0], want[i][0], ulp)
    c = plan.counters()
    assert c.tile_rows == case.facts["tile_rows"], (where, c.tile_rows, case.facts)
    if case.facts["grid"] is not None:
        assert c.grid == case.facts["grid"], (where, c.grid, case.facts)


def run_cases(cases, specialize=0, runs=2, one_plan=True):
    """One context with the cases' options; one plan over all of their inputs (or one per case), every input run `runs` times, every run
    compared.  Returns the last plan."""
    ctx = context(cases[0].options, specialize)
    plan = None
    for case in cases:
        assert case.options == cases[0].options
        view = case.view()
        if plan is None or not one_plan:
            plan = ss.Plan(case.op(view), ctx)
        for run in range(runs):
            plan.run(view)
            check_run(plan, case, "%s, specialize %d, run %d" % (case.name, specialize, run))
        if specialize:
            assert plan.specialized() > 0, (case.name, plan.specialize_reason())
    return plan


# ---- A. the tile loop of ScalarAggregate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", pr.GRID_LIMITS)
@pytest.mark.parametrize("T", pr.TILES)
def test_tile_loop(T, g):
    run_cases(pr.tile_loop_sweep(T, g))


@pytest.mark.parametrize("tile_map", [0, 2])
@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("T", pr.TILES)
def test_tile_loop_under_tile_map(T, g, tile_map):
    # tile_map 2 hands workgroup b the tiles (b % 8) g / 8 + b / 8 + it g: FIRST / LAST across workgroups rest on the row ids alone
    run_cases(pr.tile_loop_sweep(T, g, tile_map))


@pytest.mark.parametrize("T,g,tile_map", [(512, 3, None), (1024, 8, 2), (2048, 16, None)])
def test_tile_loop_specialised(T, g, tile_map):
    run_cases(pr.tile_loop_sweep(T, g, tile_map), specialize=1)


# ---- B. the NaN flag across trips --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [512, 2048])
@pytest.mark.parametrize("kind", pr.NAN_KINDS)
def test_nan_of_a_floating_min_max_in_a_later_trip(kind, T):
    # the flag is kept per lane over all trips and reported once; the flagged run is repeated in the NaN-exact form, which keeps a
    # leading NaN and no other
    case = pr.nan_case(kind, T)
    plan = run_cases([case], runs=3)
    assert ("NaN-exact" in plan.describe()) == case.notes["flagged"], plan.describe()


# ---- C. slots ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_aggs", pr.SLOT_COUNTS[:3])
def test_every_kind_on_the_last_register_slot_and_the_first_lds_slot(n_aggs):
    run_cases([pr.slot_case(n_aggs, rot) for rot in range(6)], one_plan=False)


def test_65_aggregations_are_refused():
    case = pr.slot_case(65, 0)
    with pytest.raises(ss.SupersonicException) as e:
        ss.Plan(case.op(case.view()), context(case.options))
    assert e.value.return_code == ss.ERROR_NOT_IMPLEMENTED, e.value


def test_fuse_emit_gives_the_same_row():
    # fuse_emit 1: the finish launch writes the result row; 0: an emit launch of its own does -- both rows equal the reference's
    for rot in (0, 3):
        for fuse in (0, 1):
            run_cases([pr.slot_case(9, rot, fuse)])


# ---- D. staging forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", pr.STAGING_FAMILIES)
@pytest.mark.parametrize("staged,T", pr.STAGING_SHAPES)
def test_staging_at_the_prefetch_file_s_edge(staged, T, family):
    run_cases([pr.staging_case(staged, T, family)])


def test_bool_column_at_an_odd_device_address():
    case = pr.odd_address_case()
    ctx = context(case.options)
    block = ss.BlockFromColumns(case.schema(), pr.block_columns(case), ctx)
    ptrs = [(data + pr.ODD_OFFSET_ROWS * c.data.dtype.itemsize, nulls + pr.ODD_OFFSET_ROWS if nulls else 0) for (data, nulls), c in zip(block._ptrs, case.cols)]
    assert ptrs[0][0] % 2 == 1 and ptrs[2][0] % 2 == 1 and block.row_count() == case.rows + pr.ODD_OFFSET_ROWS
    view = ss.DeviceView(case.schema(), ptrs, case.rows)      # the row-offset view of the block: its pointers moved on by one row
    view._owner = block
    plan = ss.Plan(case.op(view), ctx)
    for run in range(2):
        plan.run()
        check_run(plan, case, "%s, run %d" % (case.name, run))


# ---- E. materialising Filter ---------------------------------------------------------------------------------------------------------------
def filter_cases(grid_limit, tile_map):
    return [pr.filter_case(n, kind, grid_limit, tile_map) for n in pr.FILTER_ROWS for kind in pr.SURVIVORS]


@pytest.mark.parametrize("tile_map", pr.FILTER_MAPS)
@pytest.mark.parametrize("grid_limit", pr.FILTER_GRIDS)
def test_materialising_filter(grid_limit, tile_map):
    # ONE plan over all 96 inputs: counts, offsets and the total of a run must not reach the next one
    run_cases(filter_cases(grid_limit, tile_map))


@pytest.mark.parametrize("grid_limit,tile_map", [(3, 1), (8, 0)])
def test_materialising_filter_specialised(grid_limit, tile_map):
    run_cases(filter_cases(grid_limit, tile_map), specialize=1)


def test_scan_of_8193_tile_counts():
    # 512 x 8192 + 1 rows: the fewest for which the scan carries into a second trip -- the size is the scan chunk's, not a choice
    t0 = time.time()
    case = pr.scan_carry_case()
    t1 = time.time()
    expected(case)
    t2 = time.time()
    run_cases([case])
    t3 = time.time()
    print("scan carry: building %.2f s, reference %.2f s, device (two runs, with views and comparison) %.2f s" % (t1 - t0, t2 - t1, t3 - t2))


def test_result_switches_to_an_arena_and_back():
    cases = [pr.arena_case(run) for run in range(3)]
    assert [c.notes["result_bytes"] >= pr.ARENA_MIN for c in cases] == [True, False, True]
    run_cases(cases, runs=1)


# ---- F. device row count --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", pr.HANDOFF_GROUPS)
def test_compute_reads_the_group_count_on_the_device(groups):
    case = pr.HandoffCase(groups)
    want = case.expected_sorted()
    rows = {}
    for handoff in (1, 0):
        ctx = context({"tile_rows": pr.HANDOFF_T, "async_handoff": handoff})
        view = case.view()
        plan = ss.Plan(case.op(view), ctx)
        for run in range(2):
            plan.run(view)          # the SIGNALING division would fail the run on a row beyond the count
            got = plan.fetch()
            where = "%s, async_handoff %d, run %d" % (case.name, handoff, run)
            assert [s[0] for s in schema_list(got.schema())] == ["k", "q", "s2"] and got.row_count() == groups, (where, got.row_count())
            rows[handoff] = sort_rows(to_cols(got))
            assert_cols_equal(rows[handoff], want, context=where)
            assert plan.counters().tile_rows == pr.HANDOFF_T
    assert_cols_equal(rows[1], rows[0], context=case.name)


# ---- G. one inexact DOUBLE sum ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("specialize", [0, 1])
def test_inexact_double_sum_within_one_ulp(specialize):
    run_cases([pr.inexact_sum_case()], specialize=specialize)
