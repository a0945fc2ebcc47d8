// The sinks and number printers of the tables printed on the device (tables.hip, cellgeno.hip, genecounts.hip, hccv.hip): a row is
// printed twice, first into a sink that only counts (its length), then into one that stores (its bytes).  What the host does between the
// two kernels - the rows' places from their lengths, the table's buffer - is text_table.h.  The sinks and printers themselves are plain
// C++ a host program shares (text_core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "text_core.h"

namespace lsg {
using lsgt::n_digits;
using lsgt::LenSink;
using lsgt::PutSink;
using lsgt::put_i64;
using lsgt::put_p4;
using lsgt::put_ratio;
} // namespace lsg
