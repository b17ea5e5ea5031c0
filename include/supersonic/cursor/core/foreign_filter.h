// supersonic/cursor/core/foreign_filter.h -- the reference's include path for ForeignFilter.  The MI355X-native mirror keeps the
// whole builder API of the path in one header (ForeignFilter is defined there); this file only makes the reference's #include
// line resolve.
#ifndef SSGPU_FWD_SUPERSONIC_CURSOR_CORE_FOREIGN_FILTER_H_
#define SSGPU_FWD_SUPERSONIC_CURSOR_CORE_FOREIGN_FILTER_H_
#include "../../../supersonic_amd/supersonic.h"
#endif  // SSGPU_FWD_SUPERSONIC_CURSOR_CORE_FOREIGN_FILTER_H_
