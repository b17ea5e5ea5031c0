// supersonic/cursor/core/rowid_merge_join.h -- the reference's include path for RowidMergeJoin.  The MI355X-native mirror keeps
// the whole builder API of the path in one header (RowidMergeJoin is defined there); this file only makes the reference's
// #include line resolve.
#ifndef SSGPU_FWD_SUPERSONIC_CURSOR_CORE_ROWID_MERGE_JOIN_H_
#define SSGPU_FWD_SUPERSONIC_CURSOR_CORE_ROWID_MERGE_JOIN_H_
#include "../../../supersonic_amd/supersonic.h"
#endif  // SSGPU_FWD_SUPERSONIC_CURSOR_CORE_ROWID_MERGE_JOIN_H_
