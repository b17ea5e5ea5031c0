// supersonic/expression/core/string_expressions.h -- the reference's include path for this header.  The MI355X-native mirror
// keeps the whole builder API of the path in one header (Length, StringOffset, StringContains, StringContainsCI, ToLower, Ltrim,
// Rtrim, Trim, ToUpper, Substring, TrailingSubstring, StringReplace among it); this file only makes the reference's #include line resolve.
#ifndef SSGPU_FWD_SUPERSONIC_EXPRESSION_CORE_STRING_EXPRESSIONS_H_
#define SSGPU_FWD_SUPERSONIC_EXPRESSION_CORE_STRING_EXPRESSIONS_H_
#include "../../../supersonic_amd/supersonic.h"
#endif  // SSGPU_FWD_SUPERSONIC_EXPRESSION_CORE_STRING_EXPRESSIONS_H_
