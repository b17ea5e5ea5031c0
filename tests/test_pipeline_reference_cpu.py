"""tests/pipeline_reference.py without a GPU: its reference against the oracle on every case up to 300 000 rows, bit for bit; every
case's stated facts (tile_rows, n_tiles, grid) against the mirrors of layout_program and grid_for over the plan's own programs
(plan.describe() on a bind-only context); where the planted rows fall (tile, sub-tile, lane pair, first or second row); and the
mirror of the tile_map permutation against "every tile is owned exactly once"."""
import numpy as np
import pytest

import pipeline_reference as pr
import supersonic_amd as ss
from helpers import assert_cols_equal, sort_rows
from oracle import oracle

ORACLE_MAX_ROWS = 300000


@pytest.fixture(scope="module")
def bind_ctx():
    return ss.Context(-1)          # bind-only: plans lower and describe themselves without a device


def programs(case, ctx):
    return pr.parse_programs(ss.Plan(case.op(case.view()), ctx).describe())


def test_type_codes_are_the_api_s():
    assert all(getattr(ss, name) == code for name, code in pr.TYPE_CODE.items())
    assert (ss.NOT_NULLABLE, ss.NULLABLE) == (0, 1)


# ---- the reference against the oracle --------------------------------------------------------------------------------------------------
def against_oracle(case):
    schema, want = oracle.run(case.op(case.view()))
    rschema, got = case.expected()
    assert rschema == schema, (case.name, rschema, schema)
    inexact = case.notes.get("inexact", ())
    keep = [i for i, (name, _t, _n) in enumerate(schema) if name not in inexact]
    assert_cols_equal([got[i] for i in keep], [want[i] for i in keep], context=case.name)
    for i in (i for i in range(len(schema)) if i not in keep):
        # the oracle folds row after row, math.fsum is exact: they agree to the sequential fold's error bound, (n - 1) eps sum|x|
        x = case.cols[0].data
        assert abs(got[i][0][0] - want[i][0][0]) <= (len(x) - 1) * 2.0 ** -53 * np.abs(x).sum(), (case.name, got[i], want[i])


@pytest.mark.parametrize("T", pr.TILES)
def test_tile_loop_reference_matches_the_oracle(T):
    for g in pr.GRID_LIMITS:
        for case in pr.tile_loop_sweep(T, g):
            assert case.rows <= ORACLE_MAX_ROWS
            against_oracle(case)


def test_other_references_match_the_oracle():
    families, n = set(), 0
    for case in pr.all_cases(ORACLE_MAX_ROWS):
        if case.name.startswith("tile-loop"):
            continue
        against_oracle(case)
        families.add(case.name.split("-")[0])
        n += 1
    assert families == {"nan", "slots", "staging", "inexact", "filter"} and n >= 150, (families, n)


def test_the_cases_beyond_the_oracle_s_size_are_the_two_the_edges_dictate():
    small = {c.name for c in pr.all_cases(ORACLE_MAX_ROWS)}
    assert pr.SCAN_CARRY_ROWS > ORACLE_MAX_ROWS and min(pr.ARENA_ROWS) > ORACLE_MAX_ROWS
    assert not any(name.startswith(("filter-scan-carry", "filter-arena")) for name in small)


@pytest.mark.parametrize("groups", pr.HANDOFF_GROUPS)
def test_handoff_rows_match_the_oracle(groups):
    case = pr.HandoffCase(groups)
    schema, want = oracle.run(case.op(case.view()))
    assert [s[0] for s in schema] == ["k", "q", "s2"] and len(want[0][0]) == groups
    assert_cols_equal(case.expected_sorted(), sort_rows(want), context=case.name)


def test_leading_nan_rule_of_the_reference():
    for T in (512, 2048):
        for kind in pr.NAN_KINDS:
            case = pr.nan_case(kind, T)
            _schema, cols = case.expected()
            nan = [bool(np.isnan(cols[i][0][0])) for i in range(4)]
            assert nan == [case.notes["leading"]] * 4, (case.name, nan)
            assert not any(cols[i][1][0] for i in range(5))


# ---- stated facts against the mirrors of layout_program and grid_for ------------------------------------------------------------------
def check_facts(case, ctx):
    progs = programs(case, ctx)
    main = [p for p in progs if p["name"] == "main"][-1]
    K = pr.tile_k(main, case.options.get("tile_rows", 0))
    assert pr.TILE_UNIT * K == case.facts["tile_rows"], (case.name, K, main)
    assert case.facts["n_tiles"] == pr.ceil_div(case.rows, case.facts["tile_rows"])
    grid = case.notes.get("agg_grid", case.facts["grid"])      # (a NaN case states the grid of its repeat's last stage; agg_grid is the aggregate's)
    if grid is not None:
        assert grid == pr.grid_size(case.facts["n_tiles"], case.options["grid_limit"], pr.lds_bytes(main, K)), case.name
    return progs, main, K


def test_facts_of_every_case(bind_ctx):
    layouts = set()
    for case in pr.all_cases(ORACLE_MAX_ROWS):
        progs, main, K = check_facts(case, bind_ctx)
        layouts.add((case.name.split("-")[0], K))
        if "staged" in case.notes:
            assert main["n_staged"] == case.notes["staged"], (case.name, main)
        if "count_tile" in case.notes:
            count = [p for p in progs if p["name"] == "count pass"][0]
            assert count["n_staged"] == 1 and pr.TILE_UNIT * pr.count_pass_k(count, K) == case.notes["count_tile"], (case.name, count)
    assert {k for _f, k in layouts} == {1, 2, 4}


def test_staging_shapes_sit_on_the_prefetch_file_s_edge(bind_ctx):
    for staged, T in pr.STAGING_SHAPES:
        units = staged * T // pr.TILE_UNIT
        assert units == pr.PF_UNITS or units - T // pr.TILE_UNIT == pr.PF_UNITS, (staged, T)    # exactly full, or ONE array beyond it
    mixed = pr.staging_case(9, 512, "mixed")
    assert {c.type for c in mixed.cols} >= {"INT64", "INT32", "BOOL"} and mixed.cols[-1].nullable and mixed.cols[-1].nulls is None


def test_wide_plan_puts_first_on_the_last_register_slot_and_last_on_the_first_lds_slot():
    kinds = [fn for fn, _c, _o in pr.WIDE_AGGS]
    assert kinds[pr.FAST_SLOTS - 1] == "FIRST" and kinds[pr.FAST_SLOTS] == "LAST"


def test_slot_rotations_put_every_kind_on_slots_7_and_8():
    for n in pr.SLOT_COUNTS[:3]:
        on = {slot: {pr.slot_case(n, rot).notes["aggs"][slot][0] for rot in range(6)} for slot in (7, 8) if slot < n}
        assert all(kinds == set(pr.SLOT_KINDS) for kinds in on.values()), (n, on)
        for rot in range(6):
            case = pr.slot_case(n, rot)
            nullable = {c.name for c in case.cols if c.nullable}
            assert all(col in nullable for fn, col, _o in case.notes["aggs"] if fn == "COUNT")       # a COUNT that owns its slot
            assert pr.ceil_div(case.facts["n_tiles"], case.facts["grid"]) == 2


def test_65_aggregations_are_refused(bind_ctx):
    assert pr.SLOT_COUNTS == (pr.FAST_SLOTS, pr.FAST_SLOTS + 1, pr.MAX_SLOTS, pr.MAX_SLOTS + 1)
    case = pr.slot_case(65, 0)
    with pytest.raises(ss.SupersonicException) as e:
        ss.Plan(case.op(case.view()), bind_ctx)
    assert e.value.return_code == ss.ERROR_NOT_IMPLEMENTED, e.value
    ss.Plan(pr.slot_case(64, 0).op(pr.slot_case(64, 0).view()), bind_ctx)


def test_large_cases_sit_on_their_edges(bind_ctx):
    assert pr.ceil_div(pr.SCAN_CARRY_ROWS, 512) == pr.SCAN_CHUNK + 1
    assert [64 * n >= pr.ARENA_MIN for n in pr.ARENA_ROWS] == [True, False, True] and 64 * pr.ARENA_ROWS[0] == pr.ARENA_MIN
    # the layouts do not depend on the rows: the same plans over a few rows
    scan = pr.PipeCase("scan", [pr.Col("v", "INT32", np.arange(5)), pr.Col("keep", "BOOL", np.ones(5))], pr.SCAN_CARRY_STEPS, pr.SCAN_CARRY_OPTIONS, pr.stated_facts(5, 512, 0))
    arena = pr.PipeCase("arena", [pr.Col("c%d" % j, "INT64", np.arange(5)) for j in range(8)] + [pr.Col("keep", "BOOL", np.ones(5))], pr.ARENA_STEPS, {}, pr.stated_facts(5, 512, 0))
    for small in (scan, arena):
        progs, _main, K = check_facts(small, bind_ctx)
        assert pr.TILE_UNIT * pr.count_pass_k([p for p in progs if p["name"] == "count pass"][0], K) == pr.COUNT_T


# ---- geometry of the planted rows -------------------------------------------------------------------------------------------------------
def test_geometry_of_the_tile_loop_cases():
    positions = {}
    for T in pr.TILES:
        for g in pr.GRID_LIMITS:
            sweep = pr.tile_loop_sweep(T, g)
            assert {c.facts["n_tiles"] for c in sweep} == set(pr.tile_counts(g)) and {c.notes["last"] for c in sweep} == set(pr.last_sizes(T))
            assert max(c.rows for c in sweep) == max(pr.tile_counts(g)) * T <= 3 * 16 * 2048 + 2047
            for case in sweep:
                n, nt, grid = case.rows, case.facts["n_tiles"], case.facts["grid"]
                assert grid == min(g, nt) and (nt - 1) * T + case.notes["last"] == n
                trips = [len(pr.tiles_of(b, grid, nt, False)) for b in range(grid)]
                assert sum(trips) == nt and max(trips) == pr.ceil_div(nt, grid) and (max(trips) >= 2) == (nt > g)
                keep = case.kept()
                for which in ("min", "max"):
                    row, at = case.notes[which + "_row"], case.notes[which + "_at"]
                    tile, k, t, second = pr.locate(row, T)
                    assert keep[row]
                    positions.setdefault((T, g, at), []).append((tile, k, t, second))
                    if at == "row_0":
                        assert (tile, k, t, second) == (0, 0, 0, 0)
                    elif at == "last_row":
                        assert row == n - 1 and tile == nt - 1
                    elif at == "partial_first":
                        assert (tile, k, t, second) == (nt - 1, 0, 0, 0)
                    elif at == "full_tile_end" and n >= T:
                        assert (k, t, second) == (T // pr.TILE_UNIT - 1, pr.THREADS - 1, 1) and (tile + 1) * T <= n
                        assert tile == g or (tile + 2) * T > n                       # workgroup 0's second trip, or the last full tile there is
                    elif at == "pair_second" and n - tile * T > 1:
                        assert second == 1 and tile == min(g, nt - 1)
                # the only value below the MIN / above the MAX of the kept rows sits on a dropped row
                d, d0 = case.cols[3].data, case.cols[4].data
                assert d[keep].min() == d[case.notes["min_row"]] and (d[keep] == d[keep].min()).sum() == 1
                assert d0[keep].max() == d0[case.notes["max_row"]] and (d0[keep] == d0[keep].max()).sum() == 1
                if (~keep).any():
                    assert d[~keep].min() < d[keep].min() and d0[~keep].max() > d0[keep].max()
                zn, zk, zr = case.cols[8].nulls, case.notes["z_kind"], case.notes["z_row"]
                if zk == "first_in_last_tile":
                    assert pr.locate(zr, T)[0] == nt - 1 and np.nonzero(~zn & keep)[0].tolist() == [zr]
                    assert not (~keep).any() or np.nonzero(~zn)[0][0] < zr or n < 3
                elif zk == "last_in_tile_0":
                    assert pr.locate(zr, T)[0] == 0 and np.nonzero(~zn & keep)[0].tolist() == [zr]
                elif zk == "all_null":
                    assert zn.all()
            assert {at for (t_, g_, at) in positions if (t_, g_) == (T, g)} == set(pr.POSITIONS)
            assert {c.notes["z_kind"] for c in sweep} == set(pr.Z_KINDS)
    # over the sweep a planted row sits in every sub-tile of the largest tile and on both rows of a pair
    seen = [loc for (T, _g, _at), locs in positions.items() if T == 2048 for loc in locs]
    assert {k for _tile, k, _t, _s in seen} == {0, 1, 2, 3} and {s for _tile, _k, _t, s in seen} == {0, 1}
    assert any(pr.tile_loop_sweep(512, 1)[i].notes["z_row"] == 0 for i in range(len(pr.tile_loop_sweep(512, 1))))


def test_geometry_of_the_nan_cases():
    for T in (512, 2048):
        for kind in pr.NAN_KINDS:
            case = pr.nan_case(kind, T)
            assert case.facts == {"tile_rows": T, "n_tiles": 11, "grid": 1 if case.notes["flagged"] else 2} and case.notes["agg_grid"] == 2
            assert pr.grid_size(1, 2, 1) == 1                            # the one result row under grid_limit 2
            assert [len(pr.tiles_of(b, 2, 11, False)) for b in (0, 1)] == [6, 5]
            at = case.notes["nan_at"]
            if kind == "second_tile":
                assert pr.tiles_of(0, 2, 11, False)[1] == pr.locate(at, T)[0] and pr.locate(at, T)[3] == 1
            elif kind == "partial_tile":
                assert pr.locate(at, T)[0] == 10 and at == case.rows - 1 and case.rows % T == 100
            if at is not None:
                assert case.kept()[at] == (kind != "row_0_dropped") and np.isnan(case.cols[1].data).sum() == 1 and np.isnan(case.cols[2].data).sum() == 1
                assert case.kept()[:2].tolist() == ([True, False] if kind != "row_0_dropped" else [False, False])


def test_geometry_of_the_filter_cases():
    assert sorted(pr.FILTER_ROWS) == sorted(2048 * m + d for m in (1, 3) for d in (0, 1, 511, 512, 513, 1536, 1537, 2047))
    for n in pr.FILTER_ROWS:
        store_tiles, count_tiles = pr.ceil_div(n, pr.STORE_T), pr.ceil_div(n, pr.COUNT_T)
        assert store_tiles <= 4 * count_tiles            # the last count tile publishes 1 .. 4 counts
        k = {kind: pr.survivors(kind, n) for kind in pr.SURVIVORS}
        assert k["all"].all() and not k["none"].any() and np.nonzero(k["last_row"])[0].tolist() == [n - 1]
        assert np.nonzero(k["first_of_512"])[0].tolist() == [pr.STORE_T * t for t in range(store_tiles)]
        assert k["every_other"].sum() == n // 2 and not k["every_other"][0]
        per_tile = np.add.reduceat(k["one_per_2048"].astype(int), np.arange(0, n, pr.COUNT_T))
        assert (per_tile[: n // pr.COUNT_T] == 1).all() and per_tile.max() == 1
        assert len({int(r) % pr.COUNT_T for r in np.nonzero(k["one_per_2048"])[0]}) == k["one_per_2048"].sum()      # a different place in every tile
    assert {pr.ceil_div(n, pr.STORE_T) % 4 for n in pr.FILTER_ROWS} == {0, 1, 2, 3}


# ---- the tile_map permutation -----------------------------------------------------------------------------------------------------------
def test_tile_map_permutation_owns_every_tile_exactly_once():
    for grid in list(range(1, 41)) + [64, 256, 768]:
        for n_tiles in (grid, grid + 1, 2 * grid, 2 * grid + 1, 3 * grid - 1, 5 * grid + 3):
            for chunks in (False, True):
                owned = [0] * n_tiles                                   # brute force: walk every workgroup's trips as the kernel does
                for b in range(grid):
                    first = pr.first_tile(b, grid, chunks)
                    assert 0 <= first < grid
                    it = 0
                    while first + it * grid < n_tiles:
                        owned[first + it * grid] += 1
                        it += 1
                    assert it == len(pr.tiles_of(b, grid, n_tiles, chunks))
                assert owned == [1] * n_tiles, (grid, n_tiles, chunks)
                firsts = [pr.first_tile(b, grid, chunks) for b in range(grid)]
                if chunks and grid % 8 == 0:
                    for xcd in range(8):                                # XCD b % 8 owns a contiguous eighth of every round
                        mine = sorted(firsts[b] for b in range(grid) if b % 8 == xcd)
                        assert mine == list(range(xcd * grid // 8, (xcd + 1) * grid // 8))
                else:
                    assert firsts == list(range(grid))
    assert pr.uses_chunks(2, False) and not pr.uses_chunks(1, False) and pr.uses_chunks(1, True) and not pr.uses_chunks(0, True)


def test_locate_is_the_kernel_s_row_order():
    # vm.h: thread t of a K-unit tile holds the pairs p = k * 256 + t; pair p the rows 2 p and 2 p + 1 of the tile
    for T in pr.TILES:
        rows = [tile * T + 2 * (k * pr.THREADS + t) + s for tile in (0, 3) for k in range(T // pr.TILE_UNIT) for t in (0, 1, 63, 64, 255) for s in (0, 1)]
        assert [pr.locate(r, T) for r in rows] == [(tile, k, t, s) for tile in (0, 3) for k in range(T // pr.TILE_UNIT) for t in (0, 1, 63, 64, 255) for s in (0, 1)]
