// grb_spmm_geom.hpp — the integer side of the product with a FULL right operand (grb_spmm.hpp, the spmm_full route of GrB_mxm): the constants of the kernels'
// shape and the integer functions host code and kernels share.  Plain integers only — no HIP types, no containers — so that a stand-alone program can check it
// under the sanitizers (tests/spmm_geometry_check.cpp).  Every function is constexpr: host code and the kernels call the same text.
//
// THE SHAPES (T = A (+).(x) B, A any CSR m x n, B full n x k; a PIECE is a run of at most SPMM_L consecutive entries of one row of A)
//   narrow   k <= 64: a group of G = spmm_group(k) lanes (the power of two >= k) owns a piece, lane j of the group column j; 64 / G pieces per wave.
//   wide     k > 64: a wave owns a piece times a SLAB of SPMM_SLAB consecutive columns; lane t holds columns t, t + 64, ... of the slab (SPMM_SLAB / 64 of them).
//   A row of at most SPMM_L entries is one piece and its sums go straight into T.  A longer row is cut into spmm_chunks(len) pieces whose partial sums go to a
//   scratch array and are folded in ascending chunk order by a second kernel: a hub row never serialises on one wave, and the order is fixed.
//   Workgroups of SPMM_WAVES waves, a grid capped at SPMM_GRID_CAP workgroups with a loop past the cap.
// None of the constants has been swept (DESIGN.md "Products with a full operand" says what they rest on and what was measured with them).
#pragma once
#include <stdint.h>

namespace grb {

constexpr uint32_t SPMM_L = 256;              // entries of A per piece: longer rows are cut into chunks of this many
constexpr uint32_t SPMM_SLAB = 256;           // columns per slab of the wide kernel: four per lane
constexpr uint32_t SPMM_WAVES = 4;            // waves per workgroup
constexpr uint32_t SPMM_GRID_CAP = 2048;      // workgroups: eight per compute unit, a loop past it
constexpr uint32_t SPMM_NARROW_MAX = 64;      // the widest k the narrow kernel takes: one wave of columns
constexpr uint64_t SPMM_ENTRY_MAX = 0xFFFFFFF0ull;      // entries a device CSR may hold: 2^32 - 16 (the bound of GrBX_Matrix_import_CSR)

static_assert(SPMM_SLAB % 64 == 0 && SPMM_SLAB >= 64, "a slab is a whole number of columns per lane");

// lanes that own one piece in the narrow kernel: the power of two >= k, for 1 <= k <= SPMM_NARROW_MAX
constexpr uint32_t spmm_group(uint32_t k) { uint32_t g = 1; while (g < k) g <<= 1; return g; }
// slabs of the wide kernel for k columns
constexpr uint32_t spmm_slabs(uint32_t k) { return (k + SPMM_SLAB - 1) / SPMM_SLAB; }
// what the plan string reports: group = 0 and the slab count for the wide kernel, the group width and one slab for the narrow one
constexpr bool spmm_narrow(uint32_t k) { return k <= SPMM_NARROW_MAX; }
// pieces a row of `len` entries is cut into when it is long; a row of at most SPMM_L entries is not cut (0: it has no chunks)
constexpr bool spmm_long(uint32_t len) { return len > SPMM_L; }
constexpr uint32_t spmm_chunks(uint32_t len) { return spmm_long(len) ? (len - 1) / SPMM_L + 1 : 0; }      // (no len + L: a row may hold nearly 2^32 entries)
// the entries [begin, end) of chunk c of a row that holds [rs, re)
constexpr uint32_t spmm_chunk_begin(uint32_t rs, uint32_t c) { return rs + c * SPMM_L; }
constexpr uint32_t spmm_chunk_end(uint32_t rs, uint32_t re, uint32_t c) { return (uint64_t)rs + (uint64_t)(c + 1) * SPMM_L < re ? rs + (c + 1) * SPMM_L : re; }
// The scratch SLOT of chunk 0 of a long row, in closed form (no scan over the chunk counts): the row's first entry rs and its rank q among the long rows.  The
// chunks of a row take consecutive slots, and the runs of two long rows never overlap: with rs = a L + r and len = b L + t the run ends at a + q + b + (t > 0)
// <= (rs + len) / L + q + 1, the first slot of the next long row at the earliest.  Slots between the runs stay unused.
constexpr uint32_t spmm_slot_base(uint32_t rs, uint32_t q) { return rs / SPMM_L + q; }
// slots to allocate for `nnz` entries of A of which `nlong` rows are long
constexpr uint64_t spmm_slots(uint64_t nnz, uint64_t nlong) { return nlong ? nnz / SPMM_L + nlong + 1 : 0; }

// T's row pointer: row i starts at k times the number of non-empty rows of A before it
constexpr uint64_t spmm_rowptr(uint64_t nonempty_before, uint32_t k) { return nonempty_before * k; }
// T does not fit the 32-bit layout
constexpr bool spmm_overflows(uint64_t nonempty_rows, uint64_t k) { return k != 0 && nonempty_rows > (SPMM_ENTRY_MAX - 1) / k; }      // nonempty_rows k >= 2^32 - 16, without the product
// full: every position holds an entry
constexpr bool spmm_is_full(uint64_t nrows, uint64_t ncols, uint64_t nnz) { return nrows != 0 && ncols != 0 && nnz / ncols == nrows && nnz % ncols == 0; }

// the grids
constexpr uint32_t spmm_pieces_per_workgroup(uint32_t k) { return spmm_narrow(k) ? SPMM_WAVES * (64 / spmm_group(k)) : SPMM_WAVES; }
constexpr uint32_t spmm_grid(uint64_t tasks, uint32_t per_workgroup) {
  const uint64_t b = (tasks + per_workgroup - 1) / per_workgroup;
  return b < 1 ? 1u : b > SPMM_GRID_CAP ? SPMM_GRID_CAP : (uint32_t)b;
}

}  // namespace grb
