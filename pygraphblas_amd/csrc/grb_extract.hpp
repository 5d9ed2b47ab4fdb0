// grb_extract.hpp — host interface of the index-list extract kernels (grb_extract.hip): sub-matrix, row / column, sub-vector.
#pragma once
#include "grb_api.hpp"
#include "grb_opcommon.hpp"

namespace grb {

// An index argument (I, ni) of extract as the kernels take it: never expanded.  Position k names the source index
//   EX_ALL: k      EX_RANGE: lo + k step      EX_BACK: lo - k step      EX_LIST: list[k]
enum { EX_ALL = 0, EX_RANGE = 1, EX_BACK = 2, EX_LIST = 3 };
struct ExIdx {
  int kind = EX_ALL; uint32_t lo = 0, step = 1; uint64_t n = 0;
  const uint32_t* list = nullptr;     // device copy of an explicit list (uploaded once per call by extract_upload)
  bool increasing = true;             // strictly increasing in k
  std::vector<uint32_t> host;         // the explicit list, narrowed after validation
  bool hbm = false;                   // the list was parsed where it lay, in HBM (index_parse_device): `host` stays empty, extract_upload has nothing to do
  DevBuf own;                         // ... and this holds the narrowed list `list` points into
};
// An index argument as an entry point received it: (I, n) as in the C API, and whether an explicit list lies in HBM (the GrBX_*_at entry points with location 1,
// the GrBX_*_Vector entry points) or on the host.  GrB_ALL is GrB_ALL either way.
struct IdxArg { const GrB_Index* I; GrB_Index n; bool hbm; bool in_hbm() const { return hbm && I != GrB_ALL; } };
// Validates (I, ni) against `dim` with the errors of expand_index_list (GrB_NULL_POINTER, GrB_INDEX_OUT_OF_BOUNDS, GrB_INVALID_VALUE),
// ranges in closed form.  dim <= GRB_DIM_DEVICE_MAX.
inline void extract_parse(ExIdx& x, const GrB_Index* I, GrB_Index ni, uint64_t dim, const char* what) {
  if (I == GrB_ALL) { x.kind = EX_ALL; x.n = dim; return; }
  if (!I) fail(GrB_NULL_POINTER, std::string(what) + ": index list is NULL");
  auto oob = [&]() { fail(GrB_INDEX_OUT_OF_BOUNDS, std::string(what) + ": index out of bounds"); };
  if (ni == GXB_RANGE || ni == GXB_STRIDE || ni == GXB_BACKWARDS) {
    const uint64_t b = I[0], e = I[1], st = ni == GXB_RANGE ? 1 : I[2];
    x.kind = ni == GXB_BACKWARDS ? EX_BACK : EX_RANGE; x.n = 0;
    if (st == 0) return;
    if (ni == GXB_BACKWARDS) { if (b >= e) { if (b >= dim) oob(); x.n = (b - e) / st + 1; } }
    else if (b <= e) { x.n = (e - b) / st + 1; if (b >= dim || (x.n - 1) > (dim - 1 - b) / st) oob(); }
    if (x.n <= 1) { x.kind = EX_RANGE; x.step = 1; }                       // (one index: increasing either way)
    else if (st > 0xFFFFFFFFull) { x.n = 1; x.kind = EX_RANGE; x.step = 1; } // (unreachable for n > 1 within dim; keeps step in 32 bits)
    else x.step = (uint32_t)st;
    x.lo = x.n ? (uint32_t)b : 0; x.increasing = x.kind == EX_RANGE;
    return;
  }
  if (ni > (1ull << 40)) fail(GrB_INVALID_VALUE, std::string(what) + ": index count is not plausible");
  x.kind = EX_LIST; x.n = ni; x.host.resize(ni);
  uint64_t prev = 0;
  for (uint64_t k = 0; k < ni; k++) { const uint64_t v = I[k]; if (v >= dim) oob(); if (k && v <= prev) x.increasing = false; prev = v; x.host[k] = (uint32_t)v; }
}

// ---- grb_index.hip: the parse of an explicit list that lies in HBM ----
// One workgroup of k_index_parse takes INDEX_PARSE_THREADS * INDEX_PARSE_PER_LANE indices per round, the grid is capped at INDEX_PARSE_GRID_CAP workgroups
// (GrBX_index_geometry reports both: the tests take their edges from them).
constexpr uint32_t INDEX_PARSE_THREADS = 256, INDEX_PARSE_PER_LANE = 2, INDEX_PARSE_GRID_CAP = 4096;
inline unsigned index_parse_grid(uint64_t n) {
  const uint64_t per = (uint64_t)INDEX_PARSE_THREADS * INDEX_PARSE_PER_LANE; uint64_t b = (n + per - 1) / per;
  if (b < 1) b = 1; if (b > INDEX_PARSE_GRID_CAP) b = INDEX_PARSE_GRID_CAP; return (unsigned)b;
}
// extract_parse for `ni` 64-bit indices at the device address I: the same errors (NULL, out of bounds — before anything else of the call is looked at), x.list /
// x.n / x.increasing from one kernel, nothing downloaded but the status word.  After it returns the caller's array is not read again.
void index_parse_device(ExIdx& x, const GrB_Index* I, GrB_Index ni, uint64_t dim, const char* what);
inline void extract_parse(ExIdx& x, const IdxArg& a, uint64_t dim, const char* what) {
  if (a.in_hbm()) index_parse_device(x, a.I, a.n, dim, what); else extract_parse(x, a.I, a.n, dim, what);
}
// out[k] = x[k] as a 64-bit index for n device values of the integer type `code` (signed: sign-extended, so negative values are out of bounds)
void index_widen(int code, const void* x, uint64_t n, uint64_t* out);

struct ExtractPlan { const char* cols = "all"; bool rowsort = false, transposed = false; uint64_t src_entries = 0; };   // src_entries: entries of the selected rows (read twice)

// Columns a general list may address through the `first` table (4 (ncols + 1) bytes: 256 MB at the bound); wider operands bisect the sorted list.
constexpr uint64_t EXTRACT_TABLE_MAX_COLS = 1ull << 26;

void extract_upload(ExIdx& x, DevBuf& keep);                        // explicit list -> device (x.list); ranges / ALL need nothing
// T = A(I, J): CSR in, CSR out, columns sorted within a row.  `ts`: bytes per value (1, 2, 4, 8), moved untouched.
void extract_csr(const DevCSR& A, size_t ts, const ExIdx& I, const ExIdx& J, bool force_bisect, DevCSR& T, ExtractPlan& plan);
// t(k) = A(I[k], j) (`row_of_csr` false: column j of the CSR) or A(j, I[k]) (true: row j), as a bitmap of I.n positions
void extract_line(const DevCSR& A, size_t ts, bool row_of_csr, uint32_t j, const ExIdx& I, void* tval, uint8_t* tpres);
// t(k) = u(I[k]) on bitmaps
void extract_vector(size_t ts, const void* uval, const uint8_t* upres, const ExIdx& I, void* tval, uint8_t* tpres);

// grb_matrix_ops.cpp: C<M,replace> = accum(C, T).  `t_masked`: T already has no entry the mask forbids.  T is consumed.
void matrix_write_back(GrB_Matrix C, DevCSR& T, int tcode, GrB_Matrix M, const DescView& dv, GrB_BinaryOp accum, bool t_masked);

}  // namespace grb
