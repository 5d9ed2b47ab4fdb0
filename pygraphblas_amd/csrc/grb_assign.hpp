// grb_assign.hpp — host interface of the index-list assign kernels (grb_assign.hip): C(I, J) = A, C(i, J) = u, C(I, j) = u, w(I) = u.
#pragma once
#include "grb_extract.hpp"

namespace grb {

// The inverse of an index argument over `dim` positions: x -> the k with I[k] == x, or none.  GrB_ALL and the range triples are inverted in closed form by
// the kernels; an explicit list gets a table of `dim` uint32 (0xFFFFFFFF = not named), scattered from the uploaded list (x.list must be set: extract_upload).
// Returns false when the list names an index twice (the specification leaves that undefined; the caller keeps the host route, which takes the last one).
// EVERY other function of this file requires index arguments that passed this test: a repeat would make two source rows share one destination.
// Also false for a list over more than ASSIGN_TABLE_MAX_DIM positions: the table (4 bytes per position of the container, whatever the list's length) is not
// built for it, the host route works on the entries instead.
constexpr uint64_t ASSIGN_TABLE_MAX_DIM = 1ull << 26;                // 256 MB of table at the bound, as extract's column table
bool assign_inverse(const ExIdx& x, uint64_t dim, DevBuf& inv);

struct AssignPlan { bool rowsort = false; };

// T = A moved into C's coordinates: entry (a, b) of A becomes (I[a], J[b]) of the crows x ccols matrix T (CSR, columns sorted within a row, values untouched).
// A is |I| x |J|.
void assign_relocate(const DevCSR& A, size_t ts, const ExIdx& I, const ExIdx& J, uint32_t crows, uint32_t ccols, DevCSR& T, AssignPlan& plan);
// keep[p] = 0 for the entries of C inside I x J, 1 for the others (`inv_i` / `inv_j`: the tables of assign_inverse, unused for ALL / ranges)
void assign_region_keep(const DevCSR& C, const ExIdx& I, const DevBuf& inv_i, const ExIdx& J, const DevBuf& inv_j, uint8_t* keep);
// w<allow, replace>(I) = accum(w(I), u) on bitmaps, in place, everything in the type `code`; accum < 0: none; allow == nullptr: everything allowed
void assign_vector(int code, uint64_t n, void* wval, uint8_t* wpres, const uint8_t* allow, const ExIdx& I, const DevBuf& inv, const void* uval, const uint8_t* upres, int accum, bool replace);
// dst[i] = cast(src[i]) at the positions the assign above wrote (allowed, inside the region, u present there), nothing elsewhere: the way back from the
// accumulator's domain touches no other value of w
void assign_cast_touched(int dst_code, void* dst, int src_code, const void* src, uint64_t n, const uint8_t* allow, const ExIdx& I, const DevBuf& inv, const uint8_t* upres);
// a bitmap of n positions as a 1 x n (`as_row`) or n x 1 CSR
void assign_line_to_csr(size_t ts, uint64_t n, const void* lval, const uint8_t* lpres, bool as_row, DevCSR& T);

}  // namespace grb
