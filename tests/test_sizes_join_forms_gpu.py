"""HashJoin on the device at the sizes where its index, probe and expansion change shape, against an order-exact reference.

build_joins (supersonic_amd/csrc/runtime.cpp) sizes the index by the rhs row count; a NOT_UNIQUE join adds a scan over `cap + 1` run
counts (three kernels beyond 65536 elements, the reserved slot `cap` of the all-ones key last) and a stable sort of the rhs rows by
slot (tiles of 4096 rows); run_join_expand scans the lhs rows' run counts (the same two scan forms) and finds every output row's
lhs row by binary search.  Linear probing wraps at the table's end (ssgpu_join_build_kernel, VM_JOIN_PROBE, VM_JOIN_PROBE_WIDE).  The
other join tests stay below 700 rhs rows and compare with the oracle's nested loop; here `join_reference` plants the inputs on
those edges and gives the expected rows -- lhs order, one lhs row's matches in ascending rhs row -- which are compared in order and
bit for bit, never as a multiset (tests/test_join_reference_cpu.py checks the reference and the layouts without a GPU).

Not here: pass 3 of the rhs-row sort with more than two digit values needs more than 8 M distinct slots (join_reference)."""
import numpy as np
import pytest

import join_reference as jr
import supersonic_amd as ss
from test_chunked_gpu import blocks_of

pytestmark = pytest.mark.gpu

NA = ss.NamedAttribute
JOIN_TYPES = (jr.INNER, jr.LEFT_OUTER)
DECLARATIONS = [True, False]
DECLARATION_IDS = ["unique", "not_unique"]
STAGE_JOIN_EXPAND = 6


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])       # floats as integers


def assert_result(got, want, context):
    """Every column of the fetched View `got` against `want` ([(data, nulls or None), ...]): the same rows in the same order, NULL
    masks exactly (and exactly the columns that should have one), data bit for bit wherever the expected row is not NULL."""
    assert got.column_count() == len(want), (context, got.column_count(), len(want))
    for i, (wd, wz) in enumerate(want):
        where = "%s, column %d (%s)" % (context, i, got.schema().attribute(i).name())
        gd, gz = got.column(i).data, got.column(i).is_null
        assert len(gd) == len(wd) == got.row_count(), "%s: %d rows, expected %d" % (where, len(gd), len(wd))
        assert (gz is None) == (wz is None), "%s: NULL mask %s" % (where, "missing" if gz is None else "unexpected")
        live = np.ones(len(wd), bool)
        if wz is not None:
            bad = np.nonzero(gz != wz)[0]
            assert len(bad) == 0, "%s: NULL masks differ in %d rows, first at %s" % (where, len(bad), bad[:8])
            live = ~wz
        if wd.dtype == object:
            g, w = gd[live], wd[live]
        else:
            g, w = bits_of(gd)[live], bits_of(wd)[live]
            assert g.dtype == w.dtype, (where, gd.dtype, wd.dtype)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: %d rows differ, first at %s: got %s want %s" % (where, len(bad), np.flatnonzero(live)[bad[:8]], g[bad[:8]], w[bad[:8]])


def run_join_case(ctx, case, join_type, unique, context, degenerate=False):
    """HashJoin(join_type, UNIQUE if `unique` else NOT_UNIQUE) over the case's views, keeping lid and ri, rw, rs: one plan, two runs,
    each compared with the reference in order and bit for bit.  Returns the reference's (lhs_row, rhs_row)."""
    if not degenerate:
        matched, unmatched = case.matched_and_unmatched()
        assert matched > 0 and unmatched > 0, (context, matched, unmatched)
    if unique:
        assert not jr.has_duplicate_key(case.rhs_keys), context
    lview, rview = jr.views(case)
    pairs, want = jr.expected(case, join_type)
    plan = ss.Plan(jr.join_op(case, join_type, unique, lview, rview), ctx)
    for run in range(2):
        plan.run()
        assert_result(plan.fetch(), want, "%s, %s %s, run %d" % (context, join_type, "UNIQUE" if unique else "NOT_UNIQUE", run))
    kinds = [st["kind"] for st in plan.stage_info()]
    assert (STAGE_JOIN_EXPAND in kinds) == (not unique), kinds
    return pairs


# ---- a. index sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", JOIN_TYPES)
@pytest.mark.parametrize("unique", DECLARATIONS, ids=DECLARATION_IDS)
@pytest.mark.parametrize("shape", ["i64", "i64i64"])
@pytest.mark.parametrize("m", jr.INDEX_SIZES)
def test_index_sizes(gpu_ctx, m, shape, unique, join_type):
    # 8 / 9: 16 and 32 slots (8 UNIQUE keys: load one half); 4096 / 4097: one and two tiles of the rhs-row sort; 16384 / 16385: the scan
    # over cap + 1 = 32769 / 65537 run counts in one kernel / in three, slot `cap` alone in its last chunk; 32768 / 32769: 65536 slots
    # at load one half / 131072.  NOT_UNIQUE: keys on 1..4 rows in random row order -- a key's rows lie tiles apart and must come out
    # in ascending row (the sort is stable) --, NULL-key rows, the all-ones key
    case = jr.index_case(m, shape, unique)
    run_join_case(gpu_ctx, case, join_type, unique, "m = %d, %s" % (m, shape))


# ---- b. the reserved key -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lhs_has", [0, 1], ids=["lhs_without", "lhs_with"])
@pytest.mark.parametrize("rhs_has", [0, 1], ids=["rhs_without", "rhs_with"])
@pytest.mark.parametrize("shape", jr.ONE_WORD_SHAPES)
def test_the_all_ones_key_and_its_near_misses_unique(gpu_ctx, shape, rhs_has, lhs_has):
    # INT64 -1, UINT64 2^64 - 1, (INT32 -1, INT32 -1), (UINT32 max, INT32 -1) pack to VM_KEY_EMPTY: such a row owns the special entry, not
    # a slot.  All ones minus one and (-1, -2) are ordinary keys, on the rhs or only probed for
    for join_type in JOIN_TYPES:
        for m in (300, 16385):
            run_join_case(gpu_ctx, jr.reserved_case(shape, rhs_has, lhs_has, run=1, m=m), join_type, True, "%s, m = %d" % (shape, m))
        run_join_case(gpu_ctx, jr.reserved_case(shape, rhs_has, lhs_has, run=1, near_on_rhs=False), join_type, True, "%s, near misses absent" % shape)


RESERVED_RUNS = [(1, 300), (3, 300), (300, 600), (1, 16385), (3, 16385), (300, 16385)]


@pytest.mark.parametrize("run,m", RESERVED_RUNS, ids=["run%d-m%d" % c for c in RESERVED_RUNS])
@pytest.mark.parametrize("shape", jr.ONE_WORD_SHAPES)
def test_the_all_ones_key_on_a_run_of_rhs_rows_not_unique(gpu_ctx, shape, run, m):
    # the run of the all-ones key is counted in slot `cap`: the last element of the scan over cap + 1 counts (m = 16385: of its three-kernel form)
    for join_type in JOIN_TYPES:
        pairs = run_join_case(gpu_ctx, jr.reserved_case(shape, 1, 1, run=run, m=m), join_type, False, "%s, run of %d in %d rows" % (shape, run, m))
        assert np.bincount(pairs[0][pairs[1] >= 0]).max() == run           # (the longest run of the case)


@pytest.mark.parametrize("rhs_has,lhs_has", [(0, 0), (0, 1), (1, 0)], ids=["neither", "lhs_only", "rhs_only"])
@pytest.mark.parametrize("shape", jr.ONE_WORD_SHAPES)
def test_the_all_ones_key_on_one_side_only_not_unique(gpu_ctx, shape, rhs_has, lhs_has):
    for join_type in JOIN_TYPES:
        run_join_case(gpu_ctx, jr.reserved_case(shape, rhs_has, lhs_has, run=3), join_type, False, "%s, rhs %d lhs %d" % (shape, rhs_has, lhs_has))


FAR_DUPLICATES = [("i64", True), ("u64", True), ("i32i32", True), ("u32i32", True), ("i64", False), ("i32i32", False), ("i64i64", False)]


@pytest.mark.parametrize("shape,reserved", FAR_DUPLICATES, ids=["%s-%s" % (s, "all_ones" if r else "ordinary") for s, r in FAR_DUPLICATES])
def test_a_key_on_the_first_and_the_last_of_16385_rows_fails_a_unique_join(gpu_ctx, shape, reserved):
    case = jr.far_duplicate_case(shape, reserved)
    assert jr.has_duplicate_key(case.rhs_keys)
    lview, rview = jr.views(case)
    for join_type in JOIN_TYPES:
        plan = ss.Plan(jr.join_op(case, join_type, True, lview, rview), gpu_ctx)
        with pytest.raises(ss.SupersonicException) as e:
            plan.run()
        assert e.value.return_code == ss.ERROR_INVALID_ARGUMENT_VALUE, e.value
    run_join_case(gpu_ctx, case, jr.INNER, False, "%s: the same table, declared NOT_UNIQUE" % shape, degenerate=True)      # (every lhs row has a match)


# ---- c. probe chains -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", JOIN_TYPES)
@pytest.mark.parametrize("unique", DECLARATIONS, ids=DECLARATION_IDS)
@pytest.mark.parametrize("shape", ["i64", "i64i64"])
@pytest.mark.parametrize("length", jr.CHAIN_LENGTHS)
def test_a_probe_chain_across_the_end_of_the_table(gpu_ctx, length, shape, unique, join_type):
    # every rhs key homes on the last three slots (2 keys: on the last): the build wraps to slot 0 and on; the lhs finds every member and,
    # for absent keys homing at the chain's head, walks the whole chain across the wrap to the first free slot
    case = jr.chain_case(length, shape, unique)
    pairs = run_join_case(gpu_ctx, case, join_type, unique, "chain of %d, %s" % (length, shape))
    members = np.arange(length)                                           # the first `length` lhs rows probe the members, the next 8 the absent keys
    assert np.isin(members, pairs[0][pairs[1] >= 0]).all() and not np.isin(np.arange(length, length + 8), pairs[0][pairs[1] >= 0]).any()


# ---- d. expansion --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fanout", ["ones", "mixed"])
@pytest.mark.parametrize("n_stage", jr.EXPAND_N)
@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_lhs_rows_reaching_the_expand_stage(gpu_ctx, join_type, n_stage, fanout):
    # the scan of the run counts: one kernel up to 65536 rows (chunks of 8192 inside it), three beyond; 73729 = 9 * 8192 + 1.  INNER: the
    # match filter runs first, so n_stage counts matched rows; LEFT_OUTER: all rows, unmatched ones at both ends and 9000 in a row
    case = jr.expand_case(jr.expand_fan(n_stage, join_type, fanout))
    matched, _unmatched = case.matched_and_unmatched()
    assert (matched if join_type == jr.INNER else case.n) == n_stage
    run_join_case(gpu_ctx, case, join_type, False, "%d rows to expand, %s" % (n_stage, fanout), degenerate=(n_stage == 1 and join_type == jr.LEFT_OUTER))


@pytest.mark.parametrize("total", [65536, 65537])
@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_results_of_exactly_65536_and_65537_rows(gpu_ctx, join_type, total):
    case = jr.expand_case(jr.fan_with_output(total, join_type))
    pairs = run_join_case(gpu_ctx, case, join_type, False, "%d result rows" % total)
    assert len(pairs[0]) == total


@pytest.mark.parametrize("where", ["first", "last", "adjacent"])
@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_one_lhs_row_matching_20000_rhs_rows(gpu_ctx, join_type, where):
    # the binary search of ssgpu_join_expand_kernel over a run of 20 000 output rows: at row 0, at the last row, two such rows side by side
    case = jr.expand_case(jr.big_run_fan(where), big=True)
    pairs = run_join_case(gpu_ctx, case, join_type, False, "20 000 matches, %s" % where)
    assert np.bincount(pairs[0]).max() == jr.BIG_RUN


def test_an_inner_join_without_a_match_has_no_rows(gpu_ctx):
    case = jr.expand_case(np.zeros(5000, dtype=np.int64))
    pairs = run_join_case(gpu_ctx, case, jr.INNER, False, "nothing matched", degenerate=True)
    assert len(pairs[0]) == 0
    pairs = run_join_case(gpu_ctx, case, jr.LEFT_OUTER, False, "nothing matched", degenerate=True)
    assert len(pairs[0]) == 5000 and (pairs[1] < 0).all()


# ---- e. chunked forms ----------------------------------------------------------------------------------------------------------------
def chunked_plan(case, join_type, unique, lview, rview):
    """(operation, expected columns).  UNIQUE: Filter(a > 499) over Compute(lid, a, ri, rw, rs, s = a + ri) over the join, all in one
    pipeline; NOT_UNIQUE: the join alone (materialise + expand per chunk)."""
    if not unique:
        return jr.join_op(case, join_type, False, lview, rview), jr.expected(case, join_type)[1]
    join = jr.join_op(case, join_type, True, lview, rview, lhs_names=("lid", "a"))
    e = ss.CompoundExpression()
    for name in ["lid", "a"] + jr.RHS_NAMES:
        e.Add(NA(name))
    e.AddAs("s", ss.Plus(NA("a"), NA("ri")))
    op = ss.Filter(ss.Greater(NA("a"), ss.ConstInt64(499)), ss.ProjectAllAttributes(), ss.Compute(e, join))
    cols = jr.expected(case, join_type, lhs_names=("lid", "a"))[1]
    (a, _), (ri, ri_null) = cols[1], cols[2]
    cols.append((a + ri, ri_null))                                        # NULL where ri is (LEFT_OUTER, unmatched)
    keep = a > 499
    return op, [(d[keep], None if z is None else z[keep]) for d, z in cols]


def run_chunked_case(ctx, case, join_type, unique, context):
    lview, rview = jr.views(case)
    op, want = chunked_plan(case, join_type, unique, lview, rview)
    plan = ss.Plan(op, ctx)
    assert plan.chunked_form()[0] == 2
    for chunk in (1000, 4096, 0):
        for again in range(2):
            plan.run_host(chunk_rows=chunk)
            assert_result(plan.fetch(), want, "%s, run_host chunk_rows = %d, run %d" % (context, chunk, again))
    plan.run()
    assert_result(plan.fetch(), want, "%s, run" % context)
    plan.stream(blocks_of(lview, 1024))
    assert_result(plan.fetch(), want, "%s, pushed blocks" % context)
    return want


@pytest.mark.parametrize("n", jr.CHUNKED_N)
@pytest.mark.parametrize("join_type", JOIN_TYPES)
@pytest.mark.parametrize("unique", DECLARATIONS, ids=DECLARATION_IDS)
def test_a_join_over_host_chunks(gpu_ctx, unique, join_type, n):
    # runtime.cpp and ssgpu.h call HashJoin plans row-local (chunked staging, form 2): every chunk's result rows are appended, the
    # whole result is the reference's over the whole input whatever the chunking
    case = jr.chunked_case(n, unique)
    if n >= 1000:
        matched, unmatched = case.matched_and_unmatched()
        assert matched > 0 and unmatched > 0
    want = run_chunked_case(gpu_ctx, case, join_type, unique, "n = %d, %s %s" % (n, join_type, "UNIQUE" if unique else "NOT_UNIQUE"))
    assert n < 1000 or len(want[0][0]) > n // 8                          # (the Filter keeps half of the rows, INNER 60 % of those)


def test_an_inner_not_unique_join_with_chunks_that_match_nothing(gpu_ctx):
    case = jr.chunked_case(70001, False, barren=True)
    matched, unmatched = case.matched_and_unmatched()
    assert matched > 0 and unmatched > 16384
    run_chunked_case(gpu_ctx, case, jr.INNER, False, "whole chunks without a match")
