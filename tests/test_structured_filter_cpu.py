"""ForeignFilter and RowidMergeJoin without a GPU: the numpy model (structured_filter_reference) reproduces every vector of the
reference's own tests, and a bind-only context gives the operators' result schemas and bind errors (foreign_filter.cc:188-244,
rowid_merge_join.cc:186-240)."""
import numpy as np
import pytest

import structured_filter_reference as sfr
import supersonic_amd as ss

GOLDEN = sfr.golden()
FF_CASES = GOLDEN["foreign_filter"]
RMJ_CASES = GOLDEN["rowid_merge_join"]
FF_NAMES = ["IdentityFilterIsPassThru", "IdentityFilterIsPassThru2", "AlternatingEmpty", "AlternatingMatching", "EmptyFilter", "EmptyInput", "Projectors"]
RMJ_NAMES = ["OneToOne", "OneToZeroOrOne", "OneToMany", "OneToManyWithNulls", "ReferentialIntegrity"]


@pytest.fixture(scope="module")
def ctx():
    return ss.Context(-1)


def schema_list(schema):
    return [(schema.attribute(i).name(), schema.attribute(i).type(), schema.attribute(i).is_nullable()) for i in range(schema.attribute_count())]


def bind_error(op, ctx):
    with pytest.raises(ss.SupersonicException) as e:
        ss.Plan(op, ctx)
    return e.value.return_code, str(e.value)


# ---- the model against the reference's vectors -----------------------------------------------------------------------------------
def test_the_golden_file_holds_the_reference_tests():
    assert [c["name"] for c in FF_CASES] == FF_NAMES
    assert [c["name"] for c in RMJ_CASES] == RMJ_NAMES
    for c in FF_CASES + RMJ_CASES:
        assert "_test.cc:" in c["source"]


@pytest.mark.parametrize("case", FF_CASES, ids=FF_NAMES)
def test_model_reproduces_foreign_filter_vector(case):
    filt = sfr.table(case["filter_types"], case["filter"])
    inp = sfr.table(case["input_types"], case["input"])
    got = sfr.foreign_filter(filt[case["filter_key"]][0], inp, case["foreign_key"])
    assert sfr.same_table(got, sfr.table(case["input_types"], case["expected"])), got


@pytest.mark.parametrize("case", RMJ_CASES, ids=RMJ_NAMES)
def test_model_reproduces_rowid_merge_join_vector(case):
    left = sfr.table(case["left_types"], case["left"])
    right = sfr.table(case["right_types"], case["right"])
    projector = [(s, p) for s, p, _n in case["projector"]]
    if "expected_error" in case:
        with pytest.raises(sfr.ForeignKeyInvalid) as e:
            sfr.rowid_merge_join(left, case["left_key"], right, projector)
        assert e.value.return_code == case["expected_error"] == 501
        assert str(e.value) == "No parent record with ID > %d" % len(case["right"])
        return
    got = sfr.rowid_merge_join(left, case["left_key"], right, projector)
    want = sfr.table(case["expected_types"], case["expected"])
    # a result column is NULLABLE when its source is; the expected table's builder only sees the values
    want = [(d, z if z is not None else (np.zeros(len(d), bool) if gz is not None else None)) for (d, z), (_g, gz) in zip(want, got)]
    assert sfr.same_table(got, want), got


def test_model_compares_signed_and_ignores_the_input_order():
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    filt = np.array([lo, -1, 0, hi], dtype=np.int64)
    keys = np.array([hi, 0, 5, -1, lo, lo + 1, 0], dtype=np.int64)
    kept, new = sfr.filter_rows(filt, keys)
    assert list(kept) == [0, 1, 3, 4, 6] and list(new) == [3, 2, 1, 0, 2]
    with pytest.raises(ValueError):
        sfr.filter_rows(np.array([1, 1], dtype=np.int64), keys)
    with pytest.raises(ValueError):
        sfr.filter_rows(np.array([2, 1], dtype=np.int64), keys)


def test_model_checks_the_64_bit_key_and_only_selected_rows():
    right = [(np.array([10, 11, 12], dtype=np.int64), None)]
    for bad in (3, -1, np.iinfo(np.int64).min, 1 << 32):
        left = [(np.array([0, bad, 2], dtype=np.int64), None)]
        with pytest.raises(sfr.ForeignKeyInvalid):
            sfr.rowid_merge_join(left, 0, right, [(1, 0)])
        got = sfr.rowid_merge_join(left, 0, right, [(1, 0)], selected=np.array([True, False, True]))
        assert list(got[0][0]) == [10, 12]


# ---- result schemas -------------------------------------------------------------------------------------------------------------------
def test_abi_version_is_unchanged(ctx):
    assert ctx.lib.ssgpu_abi_version() == 10


def test_the_op_kinds_and_return_codes():
    assert (ss._lib.OP_FOREIGN_FILTER, ss._lib.OP_ROWID_MERGE_JOIN) == (11, 12)
    assert (ss.ERROR_ATTRIBUTE_IS_NULLABLE, ss.ERROR_FOREIGN_KEY_INVALID) == (406, 501)


@pytest.mark.parametrize("case", FF_CASES, ids=FF_NAMES)
def test_foreign_filter_result_schema_is_the_inputs(ctx, case):
    filt = sfr.view(case["filter_types"], sfr.table(case["filter_types"], case["filter"]))
    inp = sfr.view(case["input_types"], sfr.table(case["input_types"], case["input"]))
    plan = ss.Plan(sfr.foreign_filter_op(case, filt, inp), ctx)
    assert schema_list(plan.result_schema) == schema_list(inp.schema())
    k = case["foreign_key"]
    assert schema_list(plan.result_schema)[k] == ("col%d" % k, ss.INT64, False)


def test_foreign_filter_keeps_names_order_types_and_nullability(ctx):
    inp = ss.View(ss.TupleSchema([ss.Attribute("s", ss.STRING, ss.NULLABLE), ss.Attribute("d", ss.DOUBLE, ss.NULLABLE), ss.Attribute("parent", ss.INT64),
                                  ss.Attribute("i", ss.INT32, ss.NULLABLE), ss.Attribute("n", ss.INT64)]),
                  [ss.Column([b"x"], [False]), ss.Column([0.5], [False]), [7], ss.Column([1], [True]), [3]])
    filt = ss.View(ss.TupleSchema([ss.Attribute("w", ss.DOUBLE), ss.Attribute("id", ss.INT64)]), [[0.0], [7]])
    plan = ss.Plan(ss.ForeignFilter(ss.ProjectNamedAttribute("id"), ss.ProjectNamedAttribute("parent"), ss.ScanView(filt), ss.ScanView(inp)), ctx)
    assert schema_list(plan.result_schema) == [("s", ss.STRING, True), ("d", ss.DOUBLE, True), ("parent", ss.INT64, False), ("i", ss.INT32, True), ("n", ss.INT64, False)]
    # under a Project that renames the key: the renamed column is the one replaced
    renamed = ss.Project(ss.CompoundSingleSourceProjector().add(ss.ProjectNamedAttributeAs("parent", "fk")).add(ss.ProjectNamedAttribute("s")), ss.ScanView(inp))
    plan = ss.Plan(ss.ForeignFilter(ss.ProjectNamedAttribute("id"), ss.ProjectNamedAttribute("fk"), ss.ScanView(filt), renamed), ctx)
    assert schema_list(plan.result_schema) == [("fk", ss.INT64, False), ("s", ss.STRING, True)]
    assert "ForeignFilter" in plan.describe()


@pytest.mark.parametrize("case", RMJ_CASES, ids=RMJ_NAMES)
def test_rowid_merge_join_result_schema(ctx, case):
    left_cols, right_cols = sfr.table(case["left_types"], case["left"]), sfr.table(case["right_types"], case["right"])
    left, right = sfr.view(case["left_types"], left_cols), sfr.view(case["right_types"], right_cols)
    plan = ss.Plan(sfr.rowid_merge_join_op(case, left, right), ctx)
    want = []
    for source, position, name in case["projector"]:
        types, cols = (case["left_types"], left_cols) if source == 0 else (case["right_types"], right_cols)
        want.append((name, {"INT64": ss.INT64, "STRING": ss.STRING}[types[position]], cols[position][1] is not None))
    assert schema_list(plan.result_schema) == want
    assert "RowidMergeJoin" in plan.describe()


def test_rowid_merge_join_projector_is_bound_like_a_hash_joins(ctx):
    left = ss.View(ss.TupleSchema([ss.Attribute("k", ss.INT64), ss.Attribute("a", ss.INT32, ss.NULLABLE)]), [[0], ss.Column([1], [False])])
    right = ss.View(ss.TupleSchema([ss.Attribute("x", ss.DOUBLE, ss.NULLABLE), ss.Attribute("y", ss.INT64)]), [ss.Column([0.5], [False]), [9]])
    proj = ss.CompoundMultiSourceProjector().add(1, ss.ProjectAllAttributes("R.")).add(0, ss.ProjectAllAttributes())
    plan = ss.Plan(ss.RowidMergeJoin(ss.ProjectNamedAttribute("k"), proj, ss.ScanView(left), ss.ScanView(right)), ctx)
    assert schema_list(plan.result_schema) == [("R.x", ss.DOUBLE, True), ("R.y", ss.INT64, False), ("k", ss.INT64, False), ("a", ss.INT32, True)]
    dup = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttribute("k")).add(1, ss.ProjectNamedAttributeAs("y", "k"))
    assert bind_error(ss.RowidMergeJoin(ss.ProjectNamedAttribute("k"), dup, ss.ScanView(left), ss.ScanView(right)), ctx)[0] == ss.ERROR_ATTRIBUTE_EXISTS
    missing = ss.CompoundMultiSourceProjector().add(1, ss.ProjectNamedAttribute("k"))
    assert bind_error(ss.RowidMergeJoin(ss.ProjectNamedAttribute("k"), missing, ss.ScanView(left), ss.ScanView(right)), ctx)[0] == ss.ERROR_ATTRIBUTE_MISSING


# ---- bind errors ---------------------------------------------------------------------------------------------------------------------
def key_views():
    """A table whose columns are every way a key can be wrong: ok INT64 NOT NULL, n INT64 NULLABLE, i INT32, d DOUBLE, s STRING."""
    schema = ss.TupleSchema([ss.Attribute("ok", ss.INT64), ss.Attribute("n", ss.INT64, ss.NULLABLE), ss.Attribute("i", ss.INT32),
                             ss.Attribute("d", ss.DOUBLE), ss.Attribute("s", ss.STRING)])
    return ss.View(schema, [[0], ss.Column([0], [False]), [0], [0.0], [b"a"]])


def ff(filter_key, foreign_key, filt=None, inp=None):
    return ss.ForeignFilter(filter_key, foreign_key, filt if filt is not None else ss.ScanView(key_views()), inp if inp is not None else ss.ScanView(key_views()))


def rmj(left_key, right=None):
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttribute("ok")).add(1, ss.ProjectNamedAttributeAs("d", "rd"))
    return ss.RowidMergeJoin(left_key, proj, ss.ScanView(key_views()), right if right is not None else ss.ScanView(key_views()))


BAD_KEYS = [
    ("two_attributes", lambda: ss.ProjectNamedAttributes(["ok", "i"]), ss.ERROR_ATTRIBUTE_COUNT_MISMATCH, "Expected exactly 1 attribute for the key; found: 2"),
    ("all_attributes", lambda: ss.ProjectAllAttributes(), ss.ERROR_ATTRIBUTE_COUNT_MISMATCH, "Expected exactly 1 attribute for the key; found: 5"),
    ("no_attribute", lambda: ss.CompoundSingleSourceProjector(), ss.ERROR_ATTRIBUTE_COUNT_MISMATCH, "Expected exactly 1 attribute for the key; found: 0"),
    ("int32", lambda: ss.ProjectNamedAttribute("i"), ss.ERROR_ATTRIBUTE_TYPE_MISMATCH, "Column i designated as a key has type INT32; expected INT64"),
    ("double", lambda: ss.ProjectNamedAttribute("d"), ss.ERROR_ATTRIBUTE_TYPE_MISMATCH, "Column d designated as a key has type DOUBLE; expected INT64"),
    ("string", lambda: ss.ProjectNamedAttribute("s"), ss.ERROR_ATTRIBUTE_TYPE_MISMATCH, "Column s designated as a key has type STRING; expected INT64"),
    ("nullable", lambda: ss.ProjectNamedAttribute("n"), ss.ERROR_ATTRIBUTE_IS_NULLABLE,
     "Column n designated as a key is nullable. Please remove nullability explicitly (by casting, or using NVL)"),
]
BAD_IDS = [b[0] for b in BAD_KEYS]


@pytest.mark.parametrize("name,key,code,message", BAD_KEYS, ids=BAD_IDS)
def test_a_bad_key_is_a_bind_error(ctx, name, key, code, message):
    good = ss.ProjectNamedAttribute("ok")
    assert code in (401, 402, 406)
    for op in (ff(key(), good), ff(good, key()), rmj(key())):
        got = bind_error(op, ctx)
        assert got[0] == code and message in got[1], got


def test_the_filter_key_is_checked_before_the_foreign_key(ctx):
    code, message = bind_error(ff(ss.ProjectNamedAttribute("n"), ss.ProjectNamedAttribute("i")), ctx)
    assert code == ss.ERROR_ATTRIBUTE_IS_NULLABLE and "Column n " in message


def test_a_missing_key_attribute_is_the_projectors_error(ctx):
    good = ss.ProjectNamedAttribute("ok")
    for op in (ff(ss.ProjectNamedAttribute("nope"), good), ff(good, ss.ProjectNamedAttribute("nope")), rmj(ss.ProjectNamedAttribute("nope"))):
        assert bind_error(op, ctx)[0] == ss.ERROR_ATTRIBUTE_MISSING


def test_an_auxiliary_side_that_is_not_a_scan_is_not_implemented(ctx):
    good = ss.ProjectNamedAttribute("ok")
    for sub in (lambda: ss.Filter(ss.Less(ss.NamedAttribute("ok"), ss.ConstInt64(5)), ss.ProjectAllAttributes(), ss.ScanView(key_views())),
                lambda: ss.Project(ss.ProjectAllAttributes(), ss.ScanView(key_views()))):
        assert bind_error(ff(good, good, filt=sub()), ctx)[0] == ss.ERROR_NOT_IMPLEMENTED == 103
        assert bind_error(rmj(good, right=sub()), ctx)[0] == ss.ERROR_NOT_IMPLEMENTED


def test_one_auxiliary_table_per_plan(ctx):
    # a ForeignFilter feeding a RowidMergeJoin in ONE plan would need two auxiliary tables: refused, two plans are the way
    good = ss.ProjectNamedAttribute("ok")
    parent = ss.View(ss.TupleSchema([ss.Attribute("name", ss.INT64)]), [[5]])
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttribute("ok")).add(1, ss.ProjectNamedAttribute("name"))
    code, message = bind_error(ss.RowidMergeJoin(good, proj, ff(good, good), ss.ScanView(parent)), ctx)
    assert code == ss.ERROR_NOT_IMPLEMENTED and "one auxiliary table" in message
    # both against the SAME table is one auxiliary table: the plan binds
    table = key_views()
    proj = ss.CompoundMultiSourceProjector().add(0, ss.ProjectNamedAttribute("ok")).add(1, ss.ProjectNamedAttributeAs("d", "rd"))
    same = ss.RowidMergeJoin(good, proj, ss.ForeignFilter(good, good, ss.ScanView(table), ss.ScanView(key_views())), ss.ScanView(table))
    assert schema_list(ss.Plan(same, ctx).result_schema) == [("ok", ss.INT64, False), ("rd", ss.DOUBLE, False)]


@pytest.mark.parametrize("operator", ["foreign_filter", "rowid_merge_join"])
def test_the_auxiliary_row_count_stays_below_vm_none(ctx, operator):
    # VM_NONE = 2^32 - 1 is "no row" in the matched-row register of both instructions, and the row count travels as a u32:
    # ssgpu_plan_set_aux_input refuses a table of that many rows or more (it reads no memory: a bind-only context answers)
    if operator == "foreign_filter":
        case = FF_CASES[3]
        aux = sfr.view(case["filter_types"], sfr.table(case["filter_types"], case["filter"]))
        plan = ss.Plan(sfr.foreign_filter_op(case, aux, sfr.view(case["input_types"], sfr.table(case["input_types"], case["input"]))), ctx)
    else:
        case = RMJ_CASES[0]
        aux = sfr.view(case["right_types"], sfr.table(case["right_types"], case["right"]))
        plan = ss.Plan(sfr.rowid_merge_join_op(case, sfr.view(case["left_types"], sfr.table(case["left_types"], case["left"])), aux), ctx)
    n = aux.schema().attribute_count()
    cols = (ss._lib.Column * n)()
    bind = lambda rows: ctx.lib.ssgpu_plan_set_aux_input(plan.handle, cols, n, rows)      # noqa: E731
    for rows in ((1 << 32) - 1, 1 << 32, -1):
        assert bind(rows) == ss.ERROR_INVALID_ARGUMENT_VALUE == 407, rows
        assert "bad row count" in ctx.last_error()
    assert bind((1 << 32) - 2) == ss.OK
    assert bind(0) == ss.OK
    assert ctx.lib.ssgpu_plan_set_aux_input(plan.handle, cols, n + 1, 5) == ss.ERROR_ATTRIBUTE_COUNT_MISMATCH


def test_chunked_form_is_row_local(ctx):
    case = FF_CASES[3]
    filt = sfr.view(case["filter_types"], sfr.table(case["filter_types"], case["filter"]))
    inp = sfr.view(case["input_types"], sfr.table(case["input_types"], case["input"]))
    assert ss.Plan(sfr.foreign_filter_op(case, filt, inp), ctx).chunked_form()[0] == 2
    case = RMJ_CASES[0]
    left = sfr.view(case["left_types"], sfr.table(case["left_types"], case["left"]))
    right = sfr.view(case["right_types"], sfr.table(case["right_types"], case["right"]))
    assert ss.Plan(sfr.rowid_merge_join_op(case, left, right), ctx).chunked_form()[0] == 2
    spec = ss.AggregationSpecification().AddAggregation(ss.COUNT, "", "n")
    assert ss.Plan(ss.ScalarAggregate(spec, sfr.rowid_merge_join_op(case, left, right)), ctx).chunked_form()[0] == 1
    grouped = ss.GroupAggregate(ss.ProjectNamedAttributes(["col1"]), spec, None, sfr.rowid_merge_join_op(case, left, right))
    assert ss.Plan(grouped, ctx).chunked_form()[0] == 3


def test_running_needs_a_device(ctx):
    case = RMJ_CASES[0]
    left = sfr.view(case["left_types"], sfr.table(case["left_types"], case["left"]))
    right = sfr.view(case["right_types"], sfr.table(case["right_types"], case["right"]))
    with pytest.raises(ss.SupersonicException) as e:
        ss.Plan(sfr.rowid_merge_join_op(case, left, right), ctx).run()
    assert e.value.return_code == ss.ERROR_NO_DEVICE
