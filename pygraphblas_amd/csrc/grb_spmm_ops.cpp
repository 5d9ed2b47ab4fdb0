// grb_spmm_ops.cpp — full matrices across the C ABI: GrBX_Matrix_import_Full / GrBX_Matrix_export_Full (a row-major dense array in, the value array out) and
// GrBX_spmm_geometry / GrBX_sddmm_geometry / GrBX_gemm_geometry / GrBX_gemv_geometry.  A full matrix has no format of its own: it is the CSR whose row pointer and columns are closed form (rowptr[i] = i ncols,
// col[p] = p mod ncols) and whose value array IS the dense array, so the import is one value copy plus the fill kernel the spmm_full route of GrB_mxm uses for
// T's pattern (grb_spmm.hip), and the export is one copy.  Nothing passes through tuples or a host mirror.
#include "grb_container.hpp"
#include "grb_spmm.hpp"
#include "grb_sddmm.hpp"
#include "grb_gemm.hpp"
#include "grb_gemv.hpp"

using namespace grb;

extern "C" {

GrB_Info GrBX_Matrix_import_Full(GrB_Matrix* A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, const void* values, int location) {
  if (!A || !type) return GrB_NULL_POINTER; if (!check_obj(type)) return GrB_UNINITIALIZED_OBJECT;
  if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  if (type->code >= T_FC32) return GrB_DOMAIN_MISMATCH;
  const bool empty = nrows == 0 || ncols == 0;
  if (!empty && (nrows > GRB_DIM_DEVICE_MAX || ncols > GRB_DIM_DEVICE_MAX || spmm_overflows(nrows, ncols))) return GrB_INVALID_VALUE;
  if (!empty && !values) return GrB_NULL_POINTER;
  GrB_Matrix m = nullptr; GrB_Info info = GrB_Matrix_new(&m, type, nrows, ncols); if (info) return info;
  if (empty) { *A = m; return GrB_SUCCESS; }
  info = guarded(m, [&] {
    need_device();
    const uint64_t nnz = nrows * ncols; const size_t ts = type->size;
    DevCSR& c = m->csr; c.clear(); c.nrows = (uint32_t)nrows; c.ncols = (uint32_t)ncols; c.nnz = nnz;
    c.rowptr.alloc(((size_t)nrows + 1) * 4); c.col.alloc(nnz * 4 + 8); c.val.alloc(nnz * ts + 16);
    full_pattern_fill(c.nrows, c.ncols, nnz, nullptr, c.rowptr.as<uint32_t>(), c.col.as<uint32_t>());
    GRB_HIP(hipMemcpyAsync(c.val.p, values, nnz * ts, location ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
    c.valid = true; m->dev_valid = true; m->host_valid = false;
    g_last_plan = "import_full<rows=" + std::to_string(nrows) + ",cols=" + std::to_string(ncols) + "> k_full_pattern ";
  });
  if (info) { GrB_Matrix_free(&m); return info; }
  *A = m; return GrB_SUCCESS;
}

GrB_Info GrBX_Matrix_export_Full(const GrB_Matrix A, void* values, int location) {
  CHECK_MAT(A); if (location != 0 && location != 1) return GrB_INVALID_VALUE;
  return guarded(A, [&] {
    const uint64_t nv = mat_nvals(A);
    const bool full = (A->nrows && A->ncols) ? spmm_is_full(A->nrows, A->ncols, nv) : nv == 0;
    if (!full) fail(GrB_INVALID_VALUE, "export_Full: the matrix does not hold every position");
    if (!nv) return;
    if (!values) fail(GrB_NULL_POINTER, "export_Full: values");
    need_device(); mat_to_device(A);
    GRB_HIP(hipMemcpyAsync(values, A->csr.val.p, A->csr.nnz * A->type->size, location ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
  });
}

GrB_Info GrBX_spmm_geometry(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = SPMM_L; out[1] = SPMM_SLAB; out[2] = SPMM_WAVES; out[3] = SPMM_GRID_CAP; out[4] = SPMM_FULL_MIN_PRODUCTS; return GrB_SUCCESS;
}

// the shape of the masked product of two full matrices (grb_sddmm_geom.hpp): what its tests take their edges from
GrB_Info GrBX_sddmm_geometry(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = SDDMM_TILE; out[1] = SDDMM_WAVES; out[2] = SDDMM_GRID_CAP; out[3] = SDDMM_MIN_WORK; return GrB_SUCCESS;
}

// the shape of the product of two full matrices (grb_gemm_geom.hpp): what its tests take their edges from
GrB_Info GrBX_gemm_geometry(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = GEMM_TM_WIDE; out[1] = GEMM_TN_WIDE; out[2] = GEMM_TM_TALL; out[3] = GEMM_TN_TALL; out[4] = GEMM_KT; out[5] = GEMM_WAVES; out[6] = GEMM_GRID_CAP;
  out[7] = GEMM_FULL_MIN_WORK; out[8] = GEMM_TALL_MAX_N; return GrB_SUCCESS;
}

// the shape of a full matrix times a vector (grb_gemv_geom.hpp): what its tests take their edges from
GrB_Info GrBX_gemv_geometry(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = GEMV_LOAD_BYTES; out[1] = GEMV_N_GROUP_MAX; out[2] = GEMV_N_CHUNK; out[3] = GEMV_WAVES; out[4] = GEMV_GRID_CAP; out[5] = GEMV_T_CHUNK;
  out[6] = GEMV_T_MAX_CHUNKS; out[7] = GEMV_FULL_MIN_WORK; out[8] = GEMV_N_UNROLL; out[9] = GEMV_MAX_PACK; return GrB_SUCCESS;
}

}  // extern "C"
