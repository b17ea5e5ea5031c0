"""Every element-wise operator and every aggregate sink on the device at integer and IEEE edge values, against the exact reference of
tests/expression_reference.py (which tests/test_expression_reference_cpu.py checks against literals and against the oracle).

The other suites pin the operators whose device path changes with the input SIZE; their values are small and finite.  Here the inputs are
the edge pools -- INT_MIN / INT_MAX, 2^31, 2^53 + 1, 2^63, infinities, NaNs, subnormals, rounding ties -- and one tile of rows:
  * every operator family as column o column (NOT NULL and NULLABLE), column o constant and constant o column (one plan per constant: the
    stride-0 immediate), constant o constant (the host fold), and for the comparisons as a Filter predicate;
  * the signaling forms fail on a selected zero divisor / negative root and run clean when a Filter drops those rows;
  * each family once more as a kernel compiled for the plan (specialize = 1), which folds the plan's constants itself;
  * the aggregate sinks of ScalarAggregate (register and LDS slots) and GroupAggregate (direct, hash partitions, dense slots) at 1, 64
    and 1025 rows on two workgroups: MIN / MAX whose only value is the accumulator's identity, all-NULL columns, wrapping integer sums,
    floating sums over infinities and NaNs, FIRST / LAST of a NaN with a payload.
Results compare bit for bit; where the expected ARITHMETIC result is a NaN any NaN passes, a MOVED value keeps its bits; NULL rows compare
by mask; the one inexact DOUBLE sum is held to 1 ULP of math.fsum.  No row is skipped, no operator masked."""
import numpy as np
import pytest

import expression_reference as er
import supersonic_amd as ss
from helpers import schema_list, to_cols

pytestmark = pytest.mark.gpu

STAGE_GROUP_AGG = 3


def context(options=None, specialize=0):
    ctx = ss.Context(0)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    ctx.set_option("specialize", specialize)
    return ctx


def run_case(ctx, case, specialize=0):
    where = "%s, specialize %d" % (case.name, specialize)
    if case.error is not None:
        with pytest.raises(ss.SupersonicException) as e:
            ss.drain(case.op().CreateCursor(ctx))
        assert e.value.return_code == case.error, (where, e.value)
        return None
    schema, want, moved = case.expected()
    plan = ss.Plan(case.op(), ctx)
    plan.run()
    got = plan.fetch()
    assert schema_list(got.schema()) == schema, (where, schema_list(got.schema()), schema)
    er.same(to_cols(got), want, moved, where)
    if specialize:
        assert plan.specialized() >= 1, (where, plan.specialize_reason())
    return plan


PARAMS = [(family, t) for family, types in er.FAMILIES.items() for t in types]


@pytest.mark.parametrize("family,t", PARAMS, ids=["%s-%s" % (f, er.type_id(t)) for f, t in PARAMS])
def test_operator_family_at_the_edges(family, t):
    ctx = context()
    forms = er.family_forms(family, t)
    for form in sorted(forms):
        for case in forms[form]:
            run_case(ctx, case)


@pytest.mark.parametrize("t", er.NUMERIC, ids=er.type_id)
def test_signaling_forms_fail_on_a_selected_row_only(t):
    ctx = context()
    for failing, filtered in er.signaling_cases(t):
        run_case(ctx, failing)
        run_case(ctx, filtered)
    if t not in (er.UINT32, er.UINT64):
        run_case(ctx, er.sqrt_signaling_failure(t))


def test_logic_over_all_nine_value_null_pairs():
    ctx = context()
    for case in er.logic_cases():
        run_case(ctx, case)


@pytest.mark.parametrize("t", sorted(er.MOVE_POOL), ids=er.type_id)
def test_selection_moves_edge_values_unchanged(t):
    ctx = context()
    for case in er.selection_cases(t):
        run_case(ctx, case)


@pytest.mark.parametrize("name", sorted(er.compiled_cases()))
def test_operator_family_compiled_for_the_plan(name):
    run_case(context(specialize=1), er.compiled_cases()[name], specialize=1)


# ---- aggregate sinks ------------------------------------------------------------------------------------------------------------------------------
def group_facts(shape, n, info, plain=True):
    """What stage_info must say of the forced shape (the options of expression_reference.AGG_OPTIONS, as tests/group_reference.py sets them)."""
    if shape == "direct":
        return info["group_shape"] == 0 and info["dense_slots"] == 0
    if shape == "partitions":
        return info["group_shape"] == 1 and info["dense_slots"] == 0
    if not plain:                     # (no plain scatter, no dense slots: dense_eligible, runtime.cpp)
        return info["dense_slots"] == 0
    # dense: one slot per value of the NOT NULL key's range 0 .. groups - 1 (dense_configure), all in the one resident table
    return info["dense_slots"] == min(er.GROUPS, n) and info["group_shape"] == 3


def run_aggregates(shape, n, specialize=0, only=None):
    ctx = context(er.AGG_OPTIONS[shape], specialize)
    for case in er.agg_cases(shape, n, only):
        where = "%s, specialize %d" % (case.name, specialize)
        schema, want, moved, inexact = case.expected()
        plan = ss.Plan(case.op(), ctx)
        for run in range(2):
            plan.run()
            got = plan.fetch()
            assert schema_list(got.schema()) == schema, (where, schema_list(got.schema()), schema)
            cols = to_cols(got)
            if shape != "scalar":
                assert got.row_count() == case.groups(), (where, got.row_count())
                order = np.argsort(cols[0][0], kind="stable")
                cols = [(d[order], None if z is None else z[order]) for d, z in cols]
                info = [st for st in plan.stage_info() if st["kind"] == STAGE_GROUP_AGG][-1]
                assert group_facts(shape, n, info, case.plain()), (where, run, info)
            er.same_aggregates(cols, want, moved, inexact, "%s, run %d" % (where, run))
        if specialize:
            assert plan.specialized() >= 1, (where, plan.specialize_reason())


@pytest.mark.parametrize("n", er.AGG_ROWS)
@pytest.mark.parametrize("shape", er.AGG_SHAPES)
def test_aggregate_sinks_at_identities_and_non_finite_values(shape, n):
    run_aggregates(shape, n)


@pytest.mark.parametrize("shape", ["scalar", "partitions"])
def test_aggregate_sinks_compiled_for_the_plan(shape):
    # one plan: its first eight aggregations on register slots, the last two on LDS slots
    run_aggregates(shape, 1025, specialize=1, only=er.COMPILED_AGGS)
