// grb_compact.hpp — bitmap compaction: a byte array (presence bytes, keep flags) to the packed places of its non-zero bytes, and the entries scattered there.
// The one flag / scan / scatter of the format kernels (grb_compact.hip); the tuples path keeps its own ballot form (grb_tuples.hip).
//
// THE CONTRACT OF pos.  The caller owns `pos`, n + 1 words.  After present_positions, pos[i] = |{ j < i : bytes[j] != 0 }| for every i in [0, n]: the place of
// position i among the present ones, and pos[n] the total.  A byte is present when it is != 0 (GrBX_Vector_import_Bitmap makes values other than 1 legal).
#pragma once
#include "grb_index.hpp"

namespace grb {

// Enqueues the scan on the library stream; no synchronisation.  `pos` may be a row pointer (a column's places ARE its row pointer; a diagonal's likewise).
void present_positions(const uint8_t* bytes, uint64_t n, uint32_t* pos, uint64_t grid_cap = 4096);
// The same, then pos[n] read back through the pinned scratch: one synchronisation, for the callers that allocate by the total.
uint32_t present_positions_total(const uint8_t* bytes, uint64_t n, uint32_t* pos, uint64_t grid_cap = 4096);

// the column written for position i
enum CompactCol { COMPACT_COL_INDEX = 0,   // i            (a vector as a row)
                  COMPACT_COL_MOD = 1,     // i % ncols    (a row-major bitmap of rows of ncols positions)
                  COMPACT_COL_ZERO = 2 };  // 0            (a vector as a column)
// For every i < n with bytes[i] != 0 and w = base + pos[i]: ocol[w] = column(i) unless ocol is NULL, oval[w] = val[i] (one word of ts bytes) unless oval is
// NULL — then no value is loaded and ts, val are not looked at.  Enqueues one kernel; no synchronisation.
void scatter_present(const uint8_t* bytes, const uint32_t* pos, uint64_t n, uint32_t base, CompactCol column, uint64_t ncols, uint32_t* ocol, size_t ts, const void* val, void* oval,
                     uint64_t grid_cap = 4096);

}  // namespace grb
