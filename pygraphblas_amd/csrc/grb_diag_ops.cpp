// grb_diag_ops.cpp — a vector as the k-th diagonal of a matrix and back, both routes.
//
//   GxB_Matrix_diag, GxB_Vector_diag                            <- Matrix.from_diag, Matrix.vector_diag (pygraphblas/matrix.py:333-375, 2225-2277)
//
// The host route works on the host mirror (grb_hostmap.hpp); the kernels of the device route and the geometry of a diagonal are in grb_diag.hip / grb_diag.hpp.
// The argument and dimension checks come before the choice and are the same on both routes.
//
// Route (the rule and the two DIAG_*_DEVICE_MIN_ENTRIES: grb_route.hpp): hook GRB_MI355X_DIAG; legal when the matrix (mat_capable) and the vector (dev_capable)
// have an HBM layout; by size on the operand's host-mirror count.  Small host-resident containers — the 3 x 3 docstring examples — keep the host route.
#include "grb_hostmap.hpp"
#include "grb_diag.hpp"
#include "grb_matops.hpp"

using namespace grb;
using namespace grb::hostmap;

namespace {
bool diag_matrix_on_device(GrB_Matrix C, GrB_Vector v) {
  const RouteStep s = route_first(route_env("GRB_MI355X_DIAG"), device_ok(), mat_capable(C) && dev_capable(v), false);
  if (s != ROUTE_BY_SIZE) return s == ROUTE_DEVICE;
  vec_gate(v);                                                          // deferred work that involves v is completed first, as every reader does
  return route_by_host_count(v, DIAG_MATRIX_DEVICE_MIN_ENTRIES);
}
bool diag_vector_on_device(GrB_Vector v, GrB_Matrix A) {
  const RouteStep s = route_first(route_env("GRB_MI355X_DIAG"), device_ok(), mat_capable(A) && dev_capable(v), false);
  return s == ROUTE_BY_SIZE ? route_by_host_count(A, DIAG_VECTOR_DEVICE_MIN_ENTRIES) : s == ROUTE_DEVICE;
}
}  // namespace
extern "C" {
GrB_Info GrBX_diag_thresholds(uint64_t* matrix_min_entries, uint64_t* vector_min_entries) {
  if (!matrix_min_entries || !vector_min_entries) return GrB_NULL_POINTER;
  *matrix_min_entries = DIAG_MATRIX_DEVICE_MIN_ENTRIES; *vector_min_entries = DIAG_VECTOR_DEVICE_MIN_ENTRIES; return GrB_SUCCESS;
}
// (the descriptor has no field either operation reads: it is ignored on both routes)
GrB_Info GxB_Matrix_diag(GrB_Matrix C, const GrB_Vector v, int64_t k, const GrB_Descriptor desc) {
  (void)desc; if (!C || !v) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    check_v(v, "diag");
    const uint64_t ak = diag_abs(k); uint64_t n = 0;
    if (!diag_dim(v->n, k, &n) || C->nrows != n || C->ncols != n) fail(GrB_DIMENSION_MISMATCH, "diag: C must be square of dimension size(v) + |k|");
    g_last_plan.clear();
    if (diag_matrix_on_device(C, v)) {
      vec_to_device(v);                                                  // (completes deferred work on v: a lazily filled `v[:] = s` arrives as its bitmap)
      DevCSR T;
      const bool full = diag_to_csr(v->type->code, v->n, v->dval.p, v->dpres.as<uint8_t>(), k, T, v->facts.dnvals_known && v->facts.dnvals == v->n);
      g_last_plan = std::string("diag_matrix<k=") + std::to_string(k) + ",full=" + (full ? "1" : "0") + "> k_diag_fill ";
      const DescView dv(nullptr);
      matrix_write_back(C, T, v->type->code, nullptr, dv, nullptr, false);      // C becomes exactly T in C's type: its entries and pending edits are gone, as below
      return;
    }
    Map V = load(v), out;
    for (auto& kv : V) { const uint64_t i = kv.first.first; out[k >= 0 ? std::make_pair(i, i + ak) : std::make_pair(i + ak, i)] = cast(C->type->code, v->type->code, kv.second); }
    store(C, out);
  });
}
GrB_Info GxB_Vector_diag(GrB_Vector v, const GrB_Matrix A, int64_t k, const GrB_Descriptor desc) {
  (void)desc; if (!v || !A) return GrB_NULL_POINTER; if (!check_obj(v)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(v, [&] {
    check_m(A, "diag");
    const uint64_t len = diag_len(A->nrows, A->ncols, k);
    if (v->n != len) fail(GrB_DIMENSION_MISMATCH, "diag: the vector must have the length of the k-th diagonal");
    g_last_plan.clear();
    if (diag_vector_on_device(v, A)) {
      mat_to_device(A);
      const size_t ts = A->type->size;
      DevBuf tval(len * ts + 8), tpres(len + 1);
      csr_diag_to_bitmap(ts, A->csr, k, len, tval.p, tpres.as<uint8_t>());
      g_last_plan = std::string("diag_vector<k=") + std::to_string(k) + "> k_diag_read ";
      vec_overwritten(v);
      vector_write_back(v, A->type->code, tval, tpres, nullptr, nullptr, false, false);
      return;
    }
    mat_to_host(A); Map out;                                              // one pass over A's sorted tuples: no map of the whole matrix
    const uint64_t r0 = diag_row0(k), c0 = diag_col0(k);
    for (size_t p = 0; p < A->hi.size(); p++) {
      const uint64_t i = A->hi[p], j = A->hj[p];
      if (i >= r0 && j >= c0 && i - r0 == j - c0) out[{i - r0, 0}] = cast(v->type->code, A->type->code, val_at(A, p));
    }
    store(v, out);
  });
}
}  // extern "C"
