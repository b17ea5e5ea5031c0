// ForeignFilter and RowidMergeJoin through the C++ mirror, written against the reference's include paths for the two operators
// (cursor/core/foreign_filter.h, cursor/core/rowid_merge_join.h) and built with nothing but -I<repo>/include -lssgpu.
//   structured_filter_test bind   (no GPU: schemas and bind errors)       structured_filter_test run   (GPU: one reference vector per
//   operator -- AlternatingMatching, foreign_filter_test.cc:34-56,168-180; OneToManyWithNulls and ReferentialIntegrity,
//   rowid_merge_join_test.cc:205-291 -- as in tests/golden/structured_filter_cases.json)
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "supersonic/cursor/core/foreign_filter.h"
#include "supersonic/cursor/core/rowid_merge_join.h"

using namespace supersonic;  // NOLINT (as the reference's tests)

static int g_fail = 0;
static bool g_run = false;
#define EXPECT_TRUE(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)
#define EXPECT_EQ(a, b) do { if (!((a) == (b))) { printf("FAIL %s:%d: %s == %s\n", __FILE__, __LINE__, #a, #b); ++g_fail; } } while (0)

// a two-column table (INT64, STRING) and a one-column one (STRING), as the reference's tests build them; nulls: "" with a flag
struct KeyedStrings {
  KeyedStrings(const std::vector<int64>& k, const std::vector<const char*>& s, bool nullable) : keys(k) {
    for (const char* c : s) { cells.push_back(c ? StringPiece(c) : StringPiece()); nulls.push_back(c == nullptr); }
    schema.add_attribute(Attribute("col0", INT64, NOT_NULLABLE));
    schema.add_attribute(Attribute("col1", STRING, nullable ? NULLABLE : NOT_NULLABLE));
    view.reset(new View(schema));
    view->mutable_column(0)->Reset(keys.data(), nullptr);
    view->mutable_column(1)->Reset(cells.data(), nullable ? reinterpret_cast<const bool*>(nulls.data()) : nullptr);
    view->set_row_count(keys.size());
  }
  std::vector<int64> keys; std::vector<StringPiece> cells; std::vector<char> nulls;
  TupleSchema schema; std::unique_ptr<View> view;
};
struct Strings {
  Strings(const std::vector<const char*>& s, bool nullable) {
    for (const char* c : s) { cells.push_back(c ? StringPiece(c) : StringPiece()); nulls.push_back(c == nullptr); }
    schema.add_attribute(Attribute("col0", STRING, nullable ? NULLABLE : NOT_NULLABLE));
    view.reset(new View(schema));
    view->mutable_column(0)->Reset(cells.data(), nullable ? reinterpret_cast<const bool*>(nulls.data()) : nullptr);
    view->set_row_count(cells.size());
  }
  std::vector<StringPiece> cells; std::vector<char> nulls;
  TupleSchema schema; std::unique_ptr<View> view;
};
struct Keys {
  explicit Keys(const std::vector<int64>& k) : keys(k) {
    schema.add_attribute(Attribute("col0", INT64, NOT_NULLABLE));
    view.reset(new View(schema));
    view->mutable_column(0)->Reset(keys.data(), nullptr);
    view->set_row_count(keys.size());
  }
  std::vector<int64> keys; TupleSchema schema; std::unique_ptr<View> view;
};

static const MultiSourceProjector* Col1ThenRightCol0() {   // ->add(0, ProjectAttributeAtAs(1, "col0"))->add(1, ProjectAttributeAtAs(0, "col1"))
  return (new CompoundMultiSourceProjector)->add(0, ProjectNamedAttributeAs("col1", "col0"))->add(1, ProjectNamedAttributeAs("col0", "col1"));
}

static void ExpectBindError(Operation* operation, ReturnCode code, const char* text) {
  std::unique_ptr<Operation> op(operation);
  FailureOrOwned<Cursor> c = op->CreateCursor();
  EXPECT_TRUE(c.is_failure());
  if (!c.is_failure()) return;
  EXPECT_EQ(c.exception().return_code(), code);
  if (c.exception().message().find(text) == std::string::npos) { printf("FAIL: message '%s' lacks '%s'\n", c.exception().message().c_str(), text); ++g_fail; }
}

// ---- ForeignFilter ----------------------------------------------------------------------------------------------------------------
static void ScenarioForeignFilter() {
  Keys filter({1, 3, 5, 7, 9});
  KeyedStrings input({1, 1, 3, 3, 5, 5, 7, 9}, {"A", "B", "C", "D", "E", "F", "G", "H"}, false);
  std::unique_ptr<Operation> op(ForeignFilter(ProjectAttributeAt(0), ProjectAttributeAt(0), ScanView(*filter.view), ScanView(*input.view)));
  EXPECT_EQ(op->DebugDescription(), std::string("ForeignFilter(ScanView(), ScanView())"));
  FailureOrOwned<Cursor> c = op->CreateCursor();
  EXPECT_TRUE(c.is_success());
  if (!c.is_success()) { printf("  %s\n", c.exception().message().c_str()); return; }
  EXPECT_EQ(c->GetCursorId(), FOREIGN_FILTER);
  EXPECT_EQ(c->schema().attribute_count(), 2);
  EXPECT_EQ(c->schema().attribute(0).name(), std::string("col0"));
  EXPECT_EQ(c->schema().attribute(0).type(), INT64);
  EXPECT_TRUE(!c->schema().attribute(0).is_nullable());
  EXPECT_EQ(c->schema().attribute(1).type(), STRING);
  if (!g_run) return;
  ResultView r = c->Next(Cursor::kDefaultRowCount);
  EXPECT_TRUE(r.has_data());
  if (!r.has_data()) { if (r.is_failure()) printf("  %s\n", r.exception().message().c_str()); return; }
  const int64 want_key[8] = {0, 0, 1, 1, 2, 2, 3, 4};
  const char* want_text[8] = {"A", "B", "C", "D", "E", "F", "G", "H"};
  EXPECT_EQ(r.view().row_count(), static_cast<rowcount_t>(8));
  for (rowcount_t i = 0; i < r.view().row_count() && i < 8; ++i) {
    EXPECT_EQ(r.view().column(0).typed_data<INT64>()[i], want_key[i]);
    EXPECT_TRUE(r.view().column(1).typed_data<STRING>()[i] == StringPiece(want_text[i]));
  }
  EXPECT_TRUE(c->Next(Cursor::kDefaultRowCount).is_eos());
}

// ---- RowidMergeJoin ---------------------------------------------------------------------------------------------------------------
static void ScenarioRowidMergeJoin() {
  KeyedStrings left({0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 3, 3, 3, 3, 3, 3},
                    {"A1", "A2", "A3", "A4", "A5", "B1", "B2", "B3", "B4", "B5", nullptr, "D2", "D3", nullptr, "D5", "D6"}, true);
  Strings right({"AA", nullptr, "CC", "DD"}, true);
  std::unique_ptr<Operation> op(RowidMergeJoin(ProjectAttributeAt(0), Col1ThenRightCol0(), ScanView(*left.view), ScanView(*right.view)));
  EXPECT_EQ(op->DebugDescription(), std::string("RowidMergeJoin(ScanView(), ScanView())"));
  FailureOrOwned<Cursor> c = op->CreateCursor();
  EXPECT_TRUE(c.is_success());
  if (!c.is_success()) { printf("  %s\n", c.exception().message().c_str()); return; }
  EXPECT_EQ(c->GetCursorId(), ROWID_MERGE_JOIN);
  EXPECT_EQ(c->schema().attribute_count(), 2);
  EXPECT_EQ(c->schema().attribute(0).name(), std::string("col0"));
  EXPECT_EQ(c->schema().attribute(1).name(), std::string("col1"));
  EXPECT_TRUE(c->schema().attribute(0).is_nullable() && c->schema().attribute(1).is_nullable());
  if (!g_run) return;
  ResultView r = c->Next(Cursor::kDefaultRowCount);
  EXPECT_TRUE(r.has_data());
  if (!r.has_data()) { if (r.is_failure()) printf("  %s\n", r.exception().message().c_str()); return; }
  const char* want_right[4] = {"AA", nullptr, "CC", "DD"};
  EXPECT_EQ(r.view().row_count(), static_cast<rowcount_t>(16));
  for (rowcount_t i = 0; i < r.view().row_count() && i < 16; ++i) {
    const char* wl = left.nulls[i] ? nullptr : left.cells[i].data();
    const char* wr = want_right[left.keys[i]];
    EXPECT_EQ(static_cast<bool>(r.view().column(0).is_null()[i]), wl == nullptr);
    EXPECT_EQ(static_cast<bool>(r.view().column(1).is_null()[i]), wr == nullptr);
    if (wl) EXPECT_TRUE(r.view().column(0).typed_data<STRING>()[i] == left.cells[i]);
    if (wr) EXPECT_TRUE(r.view().column(1).typed_data<STRING>()[i] == StringPiece(wr));
  }
}

static void ScenarioReferentialIntegrity() {
  KeyedStrings left({0, 1, 1, 1, 3, 3, 3}, {"A", "B1", "B2", "B3", "D1", "D2", "D3"}, false);
  Strings right({"AA", "BB", "CC"}, false);
  std::unique_ptr<Operation> op(RowidMergeJoin(ProjectAttributeAt(0), Col1ThenRightCol0(), ScanView(*left.view), ScanView(*right.view)));
  FailureOrOwned<Cursor> c = op->CreateCursor();
  EXPECT_TRUE(c.is_success());
  if (!c.is_success() || !g_run) return;
  ResultView r = c->Next(Cursor::kDefaultRowCount);
  EXPECT_TRUE(r.is_failure());
  if (!r.is_failure()) return;
  EXPECT_EQ(r.exception().return_code(), ERROR_FOREIGN_KEY_INVALID);
  EXPECT_EQ(r.exception().message(), std::string("No parent record with ID > 3"));
}

// ---- bind errors (foreign_filter.cc:188-213, rowid_merge_join.cc:186-211) ------------------------------------------------------------
static void ScenarioBindErrors() {
  TupleSchema schema;
  schema.add_attribute(Attribute("ok", INT64, NOT_NULLABLE));
  schema.add_attribute(Attribute("n", INT64, NULLABLE));
  schema.add_attribute(Attribute("i", INT32, NOT_NULLABLE));
  View table(schema);
  ExpectBindError(ForeignFilter(ProjectNamedAttribute("ok"), ProjectAllAttributes(), ScanView(table), ScanView(table)),
                  ERROR_ATTRIBUTE_COUNT_MISMATCH, "Expected exactly 1 attribute for the key; found: 3");
  ExpectBindError(ForeignFilter(ProjectNamedAttribute("i"), ProjectNamedAttribute("ok"), ScanView(table), ScanView(table)),
                  ERROR_ATTRIBUTE_TYPE_MISMATCH, "Column i designated as a key has type INT32; expected INT64");
  ExpectBindError(ForeignFilter(ProjectNamedAttribute("ok"), ProjectNamedAttribute("n"), ScanView(table), ScanView(table)),
                  ERROR_ATTRIBUTE_IS_NULLABLE, "Column n designated as a key is nullable");
  const auto all = []() { return (new CompoundMultiSourceProjector)->add(0, ProjectAllAttributes("L."))->add(1, ProjectAllAttributes("R.")); };
  ExpectBindError(RowidMergeJoin(ProjectNamedAttributes({"ok", "i"}), all(), ScanView(table), ScanView(table)),
                  ERROR_ATTRIBUTE_COUNT_MISMATCH, "Expected exactly 1 attribute for the key; found: 2");
  ExpectBindError(RowidMergeJoin(ProjectNamedAttribute("i"), all(), ScanView(table), ScanView(table)), ERROR_ATTRIBUTE_TYPE_MISMATCH, "expected INT64");
  ExpectBindError(RowidMergeJoin(ProjectNamedAttribute("n"), all(), ScanView(table), ScanView(table)), ERROR_ATTRIBUTE_IS_NULLABLE, "is nullable");
  // the auxiliary side is a scan of a table, nothing else
  ExpectBindError(ForeignFilter(ProjectNamedAttribute("ok"), ProjectNamedAttribute("ok"), Project(ProjectAllAttributes(), ScanView(table)), ScanView(table)),
                  ERROR_NOT_IMPLEMENTED, "scan of the auxiliary input");
  ExpectBindError(RowidMergeJoin(ProjectNamedAttribute("ok"), all(), ScanView(table), Project(ProjectAllAttributes(), ScanView(table))),
                  ERROR_NOT_IMPLEMENTED, "scan of the auxiliary input");
  // one auxiliary table per plan: the chain ForeignFilter -> RowidMergeJoin against ANOTHER table is two plans, never a plan that
  // binds both operators against the second table (positional projectors, as the reference's tests use them, would bind)
  TupleSchema parent_schema;
  parent_schema.add_attribute(Attribute("id", INT64, NOT_NULLABLE));
  View parent(parent_schema);
  ExpectBindError(RowidMergeJoin(ProjectAttributeAt(0), (new CompoundMultiSourceProjector)->add(0, ProjectAttributeAt(0))->add(1, ProjectNamedAttributeAs("i", "ri")),
                                 ForeignFilter(ProjectAttributeAt(0), ProjectAttributeAt(0), ScanView(table), ScanView(table)), ScanView(parent)),
                  ERROR_NOT_IMPLEMENTED, "one auxiliary table");
  // ... while both against the SAME table is one auxiliary table
  std::unique_ptr<Operation> same(RowidMergeJoin(ProjectAttributeAt(0), (new CompoundMultiSourceProjector)->add(0, ProjectAttributeAt(0))->add(1, ProjectNamedAttributeAs("i", "ri")),
                                                 ForeignFilter(ProjectAttributeAt(0), ProjectAttributeAt(0), ScanView(table), ScanView(table)), ScanView(table)));
  EXPECT_TRUE(same->CreateCursor().is_success());
}

int main(int argc, char** argv) {
  g_run = argc > 1 && !strcmp(argv[1], "run");
  ScenarioForeignFilter();
  ScenarioRowidMergeJoin();
  ScenarioReferentialIntegrity();
  ScenarioBindErrors();
  printf(g_fail ? "FAILED (%d)\n" : "PASSED\n", g_fail);
  return g_fail ? 1 : 0;
}
