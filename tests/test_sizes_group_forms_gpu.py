"""GroupAggregate on the device in every execution shape, with its tables and row counts ON their edges, against the oracle.

run_group_agg / run_group_agg_partitioned (supersonic_amd/csrc/runtime.cpp) pick among the direct shape (an LDS table in front of a
global table that regrows x4), hash partitions (VM scatter below 65536 rows, plain scatter from there; LDS tables probed 32 deep,
partitions doubled when a cluster is longer, segments grown x4, heavy hitters aggregated apart), the one-table form (records or
resident) and dense slots (one table, or partitions of slot ranges).  The other GroupAggregate tests feed them random keys at round
sizes; here `group_reference` plants the inputs: a table exactly full and one past it, a probe cluster of exactly 32 and of 33, chains
across the end of a 64-entry table, row counts on the 65536-row and tile edges, dense ranges on cfull, rows / 4 and 2^21 slots, 32 and
33 heavy hitters.  Every test builds its own context, runs its plan twice, compares EVERY run with the oracle -- sorted rows, bit for
bit, no tolerance -- and asserts the stage_info facts the case states: they are read from the code, and they fail if the device hashes
or sizes otherwise than the mirrors that placed the keys (tests/test_group_reference_cpu.py checks mirrors and cases without a GPU).

Not here: part_n reaching 8192, segment growth reaching 64 through the VM scatter (group_reference)."""
import time

import numpy as np
import pytest

import group_reference as gr
import supersonic_amd as ss
from helpers import assert_cols_equal, schema_list, sort_rows, to_cols
from oracle import oracle

pytestmark = pytest.mark.gpu

STAGE_GROUP_AGG = 3
_expected = {}       # the oracle's answer per input, shared by the cases that differ in context options only


def expected(case, key):
    if key not in _expected:
        _expected[key] = oracle.run(case.op(case.view()))
    return _expected[key]


def holds(value, want):
    return value >= 1 if want == ">=1" else value == want


def run_case(case, key, specialize=0, runs=2):
    """One context with the case's options, one plan, `runs` runs: every run's rows against the oracle's, every run's stage_info against
    the case's facts (a value: every run; a list: one per run).  Returns the runs' stage_info of the GroupAggregate stage."""
    oschema, want = expected(case, key)
    want = sort_rows(want)
    ctx = ss.Context(0)
    for k, v in case.options.items():
        ctx.set_option(k, v)
    ctx.set_option("specialize", specialize)
    plan = ss.Plan(case.op(case.view()), ctx)
    infos = []
    for run in range(runs):
        plan.run()
        got = plan.fetch()
        where = "%s, specialize %d, run %d" % (case.name, specialize, run)
        assert schema_list(got.schema()) == oschema, where
        assert got.row_count() == len(want[0][0]) == len(case.groups()), (where, got.row_count(), len(want[0][0]), len(case.groups()))
        assert_cols_equal(sort_rows(to_cols(got)), want, context=where)
        infos.append([st for st in plan.stage_info() if st["kind"] == STAGE_GROUP_AGG][-1])
    for name, want_fact in case.facts.items():
        per_run = want_fact if isinstance(want_fact, list) else [want_fact] * runs
        got_fact = [info[name] for info in infos]
        assert all(holds(g, w) for g, w in zip(got_fact, per_run)), "%s: %s is %s, expected %s (%s)" % (case.name, name, got_fact, per_run, infos)
    return infos


# ---- A. direct shape ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("local", [1, 0])
@pytest.mark.parametrize("kind", gr.DIRECT_KINDS)
def test_direct_shape_on_a_table_of_64_slots(kind, local):
    # full: 64 keys in 64 slots, no rerun; the all-ones key owns slot `capacity`, so 65 groups still fit; 65 ordinary keys regrow the table
    # once, and the plan keeps the larger one; one_chain: all 64 keys home on slot 61 -- the longest chain there is, across the table's
    # end; the all-ones key alone (every extraction tile but the last is empty); a Filter that drops all 70 000 rows
    for specialize in ((0, 1) if kind in ("full_and_all_ones", "one_past_full") else (0,)):
        run_case(gr.direct_case(kind, local), ("direct", kind), specialize)


# ---- B. hash partitions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [65536, 65535], ids=["plain_scatter", "vm_scatter"])
@pytest.mark.parametrize("kind", gr.PARTITION_KINDS)
def test_hash_partitions_of_64_entry_tables(kind, rows):
    # chain32: the target partition's 32 keys share a home entry -- the last is found by probe 31, no rerun (and the all-ones key, routed
    # to the same partition, takes no entry); chain33: one key more re-partitions to 32 (chains of 17 and 16), which the plan keeps;
    # wrap5 / wrap3_4: chains across entry 63 -> 0; one_partition: 80 rows, all in one partition, every other segment empty
    for specialize in ((0, 1) if kind in ("chain32", "chain32_and_all_ones", "chain33") else (0,)):
        run_case(gr.partition_case(kind, rows), ("partitions", kind, rows), specialize)


@pytest.mark.parametrize("rows", gr.LAST_TILE_ROWS)
def test_plain_scatter_last_tile(rows):
    run_case(gr.last_tile_case(rows), ("last tile", rows))


@pytest.mark.parametrize("shape", ["partitions", "one_table", "dense"])
def test_a_filter_that_drops_every_row(shape):
    case = gr.filtered_case(shape)
    run_case(case, ("filtered", shape))
    assert len(expected(case, ("filtered", shape))[0]) == len(case.keys) + len(gr.SPECS[case.spec][0])       # zero rows, every column


# ---- C. one-table form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [1, 0])
@pytest.mark.parametrize("kind", gr.ONE_TABLE_KINDS)
def test_one_table_form_at_its_capacity(kind, resident):
    # full: C_FULL groups in one tile fill the table to the last entry; one_past_full: the table overflows, the stage moves to the hash
    # partitions for good; three_tiles: C_FULL + 1 groups of which no workgroup sees more than C_FULL - 100 -- three tables merged
    for specialize in ((0, 1) if kind == "full" else (0,)):
        run_case(gr.one_table_case(kind, resident), ("one table", kind), specialize)


# ---- D. dense slots ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("specialize", [0, 1])
@pytest.mark.parametrize("over", [0, 1], ids=["cfull", "cfull_plus_1"])
def test_dense_slots_at_the_one_table_capacity(over, specialize):
    run_case(gr.dense_table_edge_case(gr.C_FULL + over), ("dense table", over), specialize)


@pytest.mark.parametrize("rows", [20000, 19999])
def test_dense_slots_need_four_rows_per_slot(rows):
    run_case(gr.dense_rows_bound_case(rows), ("dense rows", rows))


@pytest.mark.parametrize("kind", gr.DENSE_MAX_KINDS)
def test_dense_slots_at_two_to_the_21(kind):
    # 8 388 608 rows: the fewest for which 2^21 slots pass the rows / 4 bound -- the size is the bound's, not a choice
    t0 = time.time()
    case = gr.dense_max_slots_case(kind)
    t1 = time.time()
    expected(case, ("dense max", kind))
    t2 = time.time()
    run_case(case, ("dense max", kind))
    t3 = time.time()
    print("dense slots %s: building %.2f s, oracle %.2f s, device (two runs, with views and comparison) %.2f s" % (kind, t1 - t0, t2 - t1, t3 - t2))


@pytest.mark.parametrize("partitioned", [False, True], ids=["one_table", "parts7"])
def test_dense_span_edges(partitioned):
    run_case(gr.dense_span_edge_case("span_edges", partitioned), ("dense span", "span_edges"))


@pytest.mark.parametrize("kind", ["all_null", "all_null_and_ordinary"])
def test_dense_key_column_that_is_entirely_null(kind):
    run_case(gr.dense_span_edge_case(kind, False), ("dense span", kind))


@pytest.mark.parametrize("parts", [7, 256])
def test_dense_partition_corners(parts):
    run_case(gr.dense_partition_corner_case(parts), ("dense corners", parts))


@pytest.mark.parametrize("rows", gr.DENSE_PARTITION_ROWS)
def test_dense_partitions_over_one_to_nine_tiles(rows):
    run_case(gr.dense_partitioned_rows_case(rows), ("dense partitioned", rows))


# ---- E. heavy hitters ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gr.HOT_KINDS)
def test_heavy_hitters(kind):
    # 32 keys of 5243 rows: all found, aggregated apart, segments as sized; 33 of equal counts: the threshold doubling passes all of
    # them, the segments grow (or the direct shape takes over); 33 of falling counts: the 32 largest; the all-ones key is never hot
    infos = run_case(gr.hot_case(kind), ("hot", kind))
    if kind == "33_equal_keys":
        assert all(i["part_seg_growth"] > 1 or i["group_shape"] == 0 for i in infos), infos
