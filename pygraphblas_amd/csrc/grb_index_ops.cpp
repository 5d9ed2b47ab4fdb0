// grb_index_ops.cpp — index lists that lie in HBM, for the seven extract / assign operations of grb_extract_ops.cpp and grb_assign_ops.cpp (grb_index_ops.hpp):
//
//   GrBX_{Vector,Col,Matrix}_extract_at, GrBX_{Vector,Matrix,Row,Col}_assign_at   <- tensors as I, J (pygraphblas_amd/matrix.py, vector.py: extract / assign with torch tensors)
//   GrBX_Vector_extract_Vector, GrBX_Vector_assign_Vector, GrBX_Matrix_extract_Vector   <- vectors as I, J (GxB_*_Vector of newer SuiteSparse; no reference counterpart)
//   GrBX_index_geometry, GrBX_index_parse                                          <- the parse alone, for the tests' edges and tools/index_probe.py
//
// The kernels are in grb_index.hip (parse, widen) and grb_tuples.hip (bitmap compaction).  Route: a list in HBM forces the device route of its operation wherever
// that route is legal (`forced` of route_first, grb_route.hpp); nothing is decided here.
#include "grb_hostmap.hpp"
#include "grb_index_ops.hpp"
#include "grb_tuples.hpp"

using namespace grb;
using namespace grb::hostmap;

// ---- a vector as an index list: the VALUES of its entries, in index order (what extractTuples returns as X) -----------------------
// With a device the list is made in HBM and nothing visits the host: the bitmap compaction of grb_tuples.hip (skipped for a vector whose facts say "all
// present": its value array is the list), then k_index_widen (skipped for the two 64-bit types), then the parse of grb_index.hip like any list in HBM.
// Without a device, or for an index vector that has no HBM layout, the list is made from the host mirror and the call is the host-list call.
namespace {
struct VecList {
  DevBuf compact, wide; std::vector<GrB_Index> host; std::string kernels;
  const GrB_Index* I = GrB_ALL; GrB_Index n = 0; bool hbm = false;
  IdxArg arg() const { return IdxArg{I, n, hbm}; }
};
void vector_as_list(GrB_Vector iv, GrB_Vector out, VecList& L) {
  if (!iv) return;                                                        // no vector: GrB_ALL
  check_v(iv, "index vector");
  if (iv == out) fail(GrB_INVALID_VALUE, "the index vector must not be the output");
  const int code = iv->type->code; const size_t ts = iv->type->size;
  if (code < T_INT8 || code > T_UINT64) fail(GrB_DOMAIN_MISMATCH, "an index vector must have an integer type");
  const bool is_signed = code == T_INT8 || code == T_INT16 || code == T_INT32 || code == T_INT64;
  if (!device_ok() || !dev_capable(iv) || iv->n > GRB_DIM_DEVICE_MAX) {
    vec_to_host(iv); L.n = iv->hi.size(); L.host.resize(L.n ? L.n : 1);
    for (GrB_Index k = 0; k < L.n; k++) cast_scalar(is_signed ? T_INT64 : T_UINT64, &L.host[k], code, &iv->hx[k * ts]);      // (sign-extended, then read as unsigned)
    L.I = L.host.data(); return;
  }
  L.hbm = true;
  vec_to_device(iv);                                                      // deferred work that writes it completes, queued edits are applied, a host-resident vector is uploaded
  const uint64_t len = iv->n; const void* vals = iv->dval.p;
  if (len && iv->facts.dnvals_known && iv->facts.dnvals == len) L.n = len;
  else if (len) {
    DevBuf offs;
    L.n = tuples_count_bitmap(iv->dpres.as<uint8_t>(), len, offs);
    iv->facts.dnvals = L.n; iv->facts.dnvals_known = true;                // (learnt by reading the image, as GrBX_Vector_extractTuples_at records it)
    L.kernels = "k_tuples_count ";
    if (L.n) { L.compact.alloc(L.n * ts + 8); tuples_from_bitmap(iv->dpres.as<uint8_t>(), iv->dval.p, ts, len, offs, nullptr, L.compact.p); L.kernels += "k_tuples_scatter "; }
    GRB_HIP(hipStreamSynchronize(stream()));                              // `offs` goes out of scope
    vals = L.compact.p;
  }
  if (!L.n) { L.wide.alloc(8); L.I = L.wide.as<GrB_Index>(); return; }     // (an empty list still needs an address that is not NULL)
  if (ts == 8) { L.I = (const GrB_Index*)vals; return; }
  L.wide.alloc(L.n * 8); index_widen(code, vals, L.n, L.wide.as<uint64_t>()); L.kernels += "k_index_widen ";
  L.I = L.wide.as<GrB_Index>();
}
// The list's own kernels go in front of the operation's in the plan string — only when THIS call wrote one: the plan is set aside before the dispatch, and a
// call that ended on a host route (which writes none) gets the earlier word back untouched.
struct VectorListPlan {
  std::string before;
  VectorListPlan() { before.swap(g_last_plan); }
  void done(const VecList& a, const VecList& b) {
    if (g_last_plan.empty()) { g_last_plan.swap(before); return; }
    const size_t at = g_last_plan.find("> ");
    if (at != std::string::npos) g_last_plan.insert(at + 2, a.kernels + b.kernels);
  }
};
bool is_range_code(GrB_Index n) { return n == GXB_RANGE || n == GXB_STRIDE || n == GXB_BACKWARDS; }
// the `location` of an index argument: 0 a host array (or GrB_ALL, or a range triple), 1 a list of `ni` 64-bit indices in HBM (or GrB_ALL)
GrB_Info location_ok(int location, const GrB_Index* I, GrB_Index ni) {
  if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  if (location == 1 && I != GrB_ALL && is_range_code(ni)) return GrB_INVALID_VALUE;
  return GrB_SUCCESS;
}
}  // namespace

extern "C" {

// ---- the seven with an index list that may lie in HBM: location 0 is the GrB_ call (a host array, GrB_ALL or a range triple); location 1: `ni` 64-bit indices at a device address (GrB_ALL is
// accepted with either value; a range code as the count of a list in HBM is GrB_INVALID_VALUE).  The call takes the device route wherever that route is legal —
// the entry-count thresholds do not apply, GRB_MI355X_EXTRACT / GRB_MI355X_ASSIGN = 0 still force the host route — and the list is parsed where it lies
// (grb_index.hip).  Where the device route is not legal (a hypersparse, complex, full one-valued or bitmap-only container, an operand that is the output, an assign
// whose list names an index twice) the list is copied down once and the host route answers.
GrB_Info GrBX_Vector_extract_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, const GrB_Descriptor desc, int location) {
  if (!w) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, I, ni)) return e;
  return vector_extract_any(w, mask, accum, u, IdxArg{I, ni, location == 1}, desc);
}
GrB_Info GrBX_Col_extract_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc, int location) {
  if (!w) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, I, ni)) return e;
  return col_extract_any(w, mask, accum, A, IdxArg{I, ni, location == 1}, j, desc);
}
GrB_Info GrBX_Matrix_extract_at(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj,
                                const GrB_Descriptor desc, int location_i, int location_j) {
  if (!C) return GrB_NULL_POINTER;
  if (const GrB_Info e = location_ok(location_i, I, ni)) return e; if (const GrB_Info e = location_ok(location_j, J, nj)) return e;
  return matrix_extract_any(C, Mask, accum, A, IdxArg{I, ni, location_i == 1}, IdxArg{J, nj, location_j == 1}, desc);
}
GrB_Info GrBX_Vector_assign_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, const GrB_Descriptor desc, int location) {
  if (!w) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, I, ni)) return e;
  return vector_assign_any(w, mask, accum, u, IdxArg{I, ni, location == 1}, desc);
}
GrB_Info GrBX_Matrix_assign_at(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj,
                               const GrB_Descriptor desc, int location_i, int location_j) {
  if (!C) return GrB_NULL_POINTER;
  if (const GrB_Info e = location_ok(location_i, I, ni)) return e; if (const GrB_Info e = location_ok(location_j, J, nj)) return e;
  return matrix_assign_any(C, Mask, accum, A, IdxArg{I, ni, location_i == 1}, IdxArg{J, nj, location_j == 1}, desc);
}
GrB_Info GrBX_Row_assign_at(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const GrB_Index* J, GrB_Index nj, const GrB_Descriptor desc, int location) {
  if (!C) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, J, nj)) return e;
  return row_assign_any(C, mask, accum, u, i, IdxArg{J, nj, location == 1}, desc);
}
GrB_Info GrBX_Col_assign_at(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index* I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc, int location) {
  if (!C) return GrB_NULL_POINTER; if (const GrB_Info e = location_ok(location, I, ni)) return e;
  return col_assign_any(C, mask, accum, u, IdxArg{I, ni, location == 1}, j, desc);
}
GrB_Info GrBX_index_geometry(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = (uint64_t)INDEX_PARSE_THREADS * INDEX_PARSE_PER_LANE; out[1] = INDEX_PARSE_GRID_CAP; return GrB_SUCCESS;
}

// the parse alone (tools/index_probe.py times it): `ni` 64-bit indices in HBM against `dim`, with the errors of the entry points above
GrB_Info GrBX_index_parse(const GrB_Index* I, GrB_Index ni, GrB_Index dim, int* increasing) {
  if (!increasing) return GrB_NULL_POINTER;
  return guarded((GrB_Vector) nullptr, [&] { need_device(); ExIdx x; index_parse_device(x, I, ni, dim, "index parse"); *increasing = x.increasing ? 1 : 0; });
}

// ---- vectors as index lists (GxB_Vector_extract_Vector / GxB_Vector_assign_Vector / GxB_Matrix_extract_Vector of newer SuiteSparse): a NULL vector means all
GrB_Info GrBX_Vector_extract_Vector(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Vector Ivec, const GrB_Descriptor desc) {
  if (!w || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  VecList L; if (const GrB_Info e = guarded(w, [&] { vector_as_list(Ivec, w, L); })) return e;
  VectorListPlan plan; const GrB_Info info = vector_extract_any(w, mask, accum, u, L.arg(), desc);
  plan.done(L, VecList()); return info;
}
GrB_Info GrBX_Vector_assign_Vector(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Vector Ivec, const GrB_Descriptor desc) {
  if (!w || !u) return GrB_NULL_POINTER; if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  VecList L; if (const GrB_Info e = guarded(w, [&] { vector_as_list(Ivec, w, L); })) return e;
  VectorListPlan plan; const GrB_Info info = vector_assign_any(w, mask, accum, u, L.arg(), desc);
  plan.done(L, VecList()); return info;
}
GrB_Info GrBX_Matrix_extract_Vector(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Vector Ivec, const GrB_Vector Jvec, const GrB_Descriptor desc) {
  if (!C || !A) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  VecList Li, Lj; if (const GrB_Info e = guarded(C, [&] { vector_as_list(Ivec, nullptr, Li); vector_as_list(Jvec, nullptr, Lj); })) return e;
  VectorListPlan plan; const GrB_Info info = matrix_extract_any(C, Mask, accum, A, Li.arg(), Lj.arg(), desc);
  plan.done(Li, Lj); return info;
}

}  // extern "C"
