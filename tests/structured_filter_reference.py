"""A numpy model of ForeignFilter and RowidMergeJoin (cursor/core/foreign_filter.h:25-47, rowid_merge_join.h:29-41), pinned on the
reference's own test vectors (tests/golden/structured_filter_cases.json, tests/test_structured_filter_cpu.py).

A table is a list of columns, a column a pair (data, nulls): `data` a numpy array (STRING: an object array of bytes), `nulls` a bool
array or None for a NOT_NULLABLE column.

ForeignFilter: the filter keys are strictly ascending INT64, so the row that holds a key is np.searchsorted on the signed values; an
input row survives when the key found there is its own, and its key becomes that row's number.  Nothing depends on the order of the
input's keys.  RowidMergeJoin: the left key IS the right row, so the right columns are fancy-indexed by it after a range check on the
signed 64-bit value; one key outside [0, right rows) fails the whole join."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "structured_filter_cases.json")
ERROR_FOREIGN_KEY_INVALID = 501


class ForeignKeyInvalid(Exception):
    """ERROR_FOREIGN_KEY_INVALID with the reference's message (rowid_merge_join.cc:99-102)."""

    def __init__(self, right_rows):
        Exception.__init__(self, "No parent record with ID > %d" % right_rows)
        self.return_code = ERROR_FOREIGN_KEY_INVALID


def strictly_ascending(keys):
    keys = np.asarray(keys, dtype=np.int64)
    return bool(np.all(keys[:-1] < keys[1:]))


def filter_rows(filter_keys, input_keys):
    """(kept, new_keys): the input rows whose key is one of the strictly ascending `filter_keys`, in input order, and for each of
    them the row of the filter that holds its key."""
    fk = np.ascontiguousarray(filter_keys, dtype=np.int64)
    ik = np.ascontiguousarray(input_keys, dtype=np.int64)
    if not strictly_ascending(fk):
        raise ValueError("the filter keys must be unique and ascending")
    at = np.searchsorted(fk, ik, side="left")                # signed compares: the arrays are int64
    inside = at < len(fk)
    hit = np.zeros(len(ik), dtype=bool)
    hit[inside] = fk[at[inside]] == ik[inside]
    kept = np.flatnonzero(hit)
    return kept, at[kept].astype(np.int64)


def take(column, rows):
    data, nulls = column
    return data[rows], (None if nulls is None else nulls[rows])


def foreign_filter(filter_keys, input_columns, foreign_key):
    """The result table: the input's columns in the input's order, column `foreign_key` replaced by the filter row (INT64, never NULL)."""
    kept, new_keys = filter_rows(filter_keys, input_columns[foreign_key][0])
    out = [take(c, kept) for c in input_columns]
    out[foreign_key] = (new_keys, None)
    return out


def rowid_merge_join(left_columns, left_key, right_columns, projector, selected=None):
    """projector: [(source, position), ...] with source 0 = left, 1 = right.  `selected`: the left rows a Filter below keeps (a bool
    array; None = all) -- only those are checked and joined."""
    keys = np.ascontiguousarray(left_columns[left_key][0], dtype=np.int64)
    rows = np.arange(len(keys)) if selected is None else np.flatnonzero(selected)
    keys = keys[rows]
    right_rows = len(right_columns[0][0]) if right_columns else 0
    if np.any((keys < 0) | (keys >= right_rows)):
        raise ForeignKeyInvalid(right_rows)
    return [take(left_columns[pos], rows) if source == 0 else take(right_columns[pos], keys) for source, pos in projector]


# ---- tables from the golden file (the reference's TestDataBuilder: rows of values, None = NULL) -------------------------------------
NUMPY_TYPES = {"INT64": np.int64, "INT32": np.int32, "DOUBLE": np.float64}


def table(types, rows):
    """Columns of a list of rows; a column is NULLABLE exactly when it holds a NULL (block_builder.h: columns without nulls are
    optimised to NOT_NULLABLE)."""
    cols = []
    for j, t in enumerate(types):
        values = [r[j] for r in rows]
        nulls = np.array([v is None for v in values], dtype=bool)
        if t == "STRING":
            data = np.empty(len(values), dtype=object)
            data[:] = [b"" if v is None else v.encode() for v in values]
        else:
            data = np.array([0 if v is None else v for v in values], dtype=NUMPY_TYPES[t])
        cols.append((data, nulls if nulls.any() else None))
    return cols


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def same_table(got, want):
    """Two tables are the same: NULL masks where expected, equal masks, and equal bits / bytes wherever the row is not NULL."""
    if len(got) != len(want):
        return False
    for (gd, gz), (wd, wz) in zip(got, want):
        if len(gd) != len(wd) or (gz is None) != (wz is None):
            return False
        live = np.ones(len(wd), dtype=bool) if wz is None else ~wz
        if wz is not None and not np.array_equal(gz, wz):
            return False
        if wd.dtype == object:
            if list(gd[live]) != list(wd[live]):
                return False
        elif gd.dtype != wd.dtype or not np.array_equal(np.ascontiguousarray(gd[live]).view(np.uint8), np.ascontiguousarray(wd[live]).view(np.uint8)):
            return False
    return True


# ---- the same tables as host Views and the operations over them ----------------------------------------------------------------------
def view(types, columns, names=None):
    import supersonic_amd as ss
    ss_types = {"INT64": ss.INT64, "INT32": ss.INT32, "DOUBLE": ss.DOUBLE, "STRING": ss.STRING}
    names = names or ["col%d" % j for j in range(len(types))]
    attrs = [ss.Attribute(n, ss_types[t], ss.NULLABLE if z is not None else ss.NOT_NULLABLE) for n, t, (_d, z) in zip(names, types, columns)]
    return ss.View(ss.TupleSchema(attrs), [ss.Column(d, z) for d, z in columns], len(columns[0][0]) if columns else 0)


def foreign_filter_op(case, filter_view, input_view):
    import supersonic_amd as ss
    return ss.ForeignFilter(ss.ProjectAttributeAt(case["filter_key"]), ss.ProjectAttributeAt(case["foreign_key"]),
                            ss.ScanView(filter_view), ss.ScanView(input_view))


def projector_of(entries):
    import supersonic_amd as ss
    # the reference's ProjectAttributeAtAs(position, name); the golden tables name their columns col<position>
    proj = ss.CompoundMultiSourceProjector()
    for source, position, name in entries:
        proj.add(source, ss.ProjectNamedAttributeAs("col%d" % position, name))
    return proj


def rowid_merge_join_op(case, left_view, right_view):
    import supersonic_amd as ss
    return ss.RowidMergeJoin(ss.ProjectAttributeAt(case["left_key"]), projector_of(case["projector"]), ss.ScanView(left_view), ss.ScanView(right_view))
