// grb_internal.hpp — object model of the MI355X GraphBLAS backend (not part of the C ABI).
//
// Layout in HBM:
//   Matrix : CSR  rowptr u32[nrows+1] | col u32[nnz] (sorted within a row) | val T[nnz]
//            + a lazily built, cached CSR of the transpose ("CSC view") and what the products derive from a CSR (grb_devcsr.hpp: CsrDerived).
//   Vector : bitmap  val T[n] | present u8[n]   (+ nvals); sparse index lists are transient.
// Host mirrors (sorted tuples) exist only for element-wise host access (setElement /
// extractTuples) and are synchronised lazily in either direction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include <mutex>
#include <stdlib.h>
#include <memory>
#include "grb_ops.hpp"
#include "grb_vecfacts.hpp"
#include "grb_devcsr.hpp"
#include "grb_route.hpp"

typedef uint64_t GrB_Index;

// GrB_Info: positive v1.3 / SuiteSparse-5 numbering (reference: pygraphblas/base.py:189-203)
enum GrB_Info_e : int {
  GrB_SUCCESS = 0, GrB_NO_VALUE = 1, GrB_UNINITIALIZED_OBJECT = 2, GrB_INVALID_OBJECT = 3,
  GrB_NULL_POINTER = 4, GrB_INVALID_VALUE = 5, GrB_INVALID_INDEX = 6, GrB_DOMAIN_MISMATCH = 7,
  GrB_DIMENSION_MISMATCH = 8, GrB_OUTPUT_NOT_EMPTY = 9, GrB_OUT_OF_MEMORY = 10,
  GrB_INSUFFICIENT_SPACE = 11, GrB_INDEX_OUT_OF_BOUNDS = 12, GrB_PANIC = 13
};
typedef int GrB_Info;

// descriptor fields / values (SuiteSparse v5.1 numbering)
enum { GrB_OUTP = 0, GrB_MASK = 1, GrB_INP0 = 2, GrB_INP1 = 3,
       GxB_DESCRIPTOR_NTHREADS = 5, GxB_DESCRIPTOR_CHUNK = 7, GxB_DESCRIPTOR_GPU_CONTROL = 21,
       GxB_DESCRIPTOR_GPU_CHUNK = 22, GxB_AxB_METHOD = 1000, GxB_SORT = 35 };
enum { GxB_DEFAULT = 0, GrB_REPLACE = 1, GrB_COMP = 2, GrB_TRAN = 3, GrB_STRUCTURE = 4,
       GxB_AxB_GUSTAVSON = 1001, GxB_AxB_DOT = 1003, GxB_AxB_HASH = 1004, GxB_AxB_SAXPY = 1005 };

#define GRB_MAGIC 0x72657473786f62ULL
#define GRB_FREED 0x6c6c756e786f62ULL
#define GRB_DIM_DEVICE_MAX 0xFFFFFFF0ULL   // device containers use 32-bit indices
#define GXB_INDEX_MAX ((GrB_Index)1 << 60)

struct GrB_Type_opaque { uint64_t magic; int code; size_t size; char name[32]; };
// `defn`: a user-defined operator (GxB_UnaryOp_new / GxB_BinaryOp_new, grb_userop.cpp; opcode >= U_USER / B_USER) owns a copy of its C definition; nullptr for built-ins
struct GrB_UnaryOp_opaque { uint64_t magic; int opcode; GrB_Type_opaque* xtype; GrB_Type_opaque* ztype; char name[40]; void* fn; char* defn; };
struct GrB_BinaryOp_opaque { uint64_t magic; int opcode; GrB_Type_opaque* xtype; GrB_Type_opaque* ytype; GrB_Type_opaque* ztype; char name[40]; void* fn; char* defn; };
// `usersr`: made by GrBX_Monoid_new_user / GrBX_Semiring_new_user (grb_usersr.cpp) — such an object always runs through the compiled kernels of user-defined semirings,
// also when all of its operators are built-in, so that its rules (the identity is never combined into a result) do not depend on what it is made of
struct GrB_Monoid_opaque { uint64_t magic; GrB_BinaryOp_opaque* op; uint8_t identity[16]; bool has_terminal; uint8_t terminal[16]; char name[48]; bool builtin; bool usersr; };
struct GrB_Semiring_opaque { uint64_t magic; GrB_Monoid_opaque* add; GrB_BinaryOp_opaque* mul; char name[56]; bool builtin; bool usersr; };
struct GrB_Descriptor_opaque { uint64_t magic; int outp, mask, inp0, inp1, axb, nthreads, sort; double chunk; bool builtin; char name[16]; };
// a user-defined select operator (GxB_SelectOp_new, grb_userop.cpp; opcode >= SEL_USER) has its value and thunk types and owns a copy of its C definition; built-ins: nullptr
struct GxB_SelectOp_opaque { uint64_t magic; int opcode; char name[40]; void* fn; GrB_Type_opaque* xtype; GrB_Type_opaque* ttype; char* defn; };

typedef GrB_Type_opaque* GrB_Type;
typedef GrB_UnaryOp_opaque* GrB_UnaryOp;
typedef GrB_BinaryOp_opaque* GrB_BinaryOp;
typedef GrB_Monoid_opaque* GrB_Monoid;
typedef GrB_Semiring_opaque* GrB_Semiring;
typedef GrB_Descriptor_opaque* GrB_Descriptor;
typedef GxB_SelectOp_opaque* GxB_SelectOp;

enum SelectCode { SEL_TRIL = 0, SEL_TRIU, SEL_DIAG, SEL_OFFDIAG, SEL_NONZERO, SEL_EQ_ZERO, SEL_GT_ZERO,
                  SEL_GE_ZERO, SEL_LT_ZERO, SEL_LE_ZERO, SEL_NE_THUNK, SEL_EQ_THUNK, SEL_GT_THUNK,
                  SEL_GE_THUNK, SEL_LT_THUNK, SEL_LE_THUNK, SEL_USER };

namespace grb {

// ---- device memory ----------------------------------------------------------------------
bool device_ok();                 // a HIP device was found at init
const char* device_error();       // why not
hipStream_t stream();             // the stream every kernel of the library is launched on
void dev_pool_release();          // return cached blocks to the driver
size_t dev_bytes_in_use();
int device_cus();                 // compute units of the device (256 on MI355X)

struct GrbError { int info; std::string msg; };
[[noreturn]] void fail(int info, const std::string& msg);
#define GRB_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
  ::grb::fail(GrB_PANIC, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// DevBuf (owning device buffer, dev_alloc / dev_free), DevCSR with its CsrDerived record, DevBitmap: grb_devcsr.hpp

}  // namespace grb

struct GrB_Matrix_opaque {
  uint64_t magic = GRB_MAGIC;
  GrB_Type type = nullptr;
  GrB_Index nrows = 0, ncols = 0;
  // host mirror: tuples sorted by (i, j), values packed at type->size each
  bool host_valid = true;
  std::vector<GrB_Index> hi, hj; std::vector<uint8_t> hx;
  // pending host edits (setElement / removeElement), applied in order at assemble time
  struct Pending { GrB_Index i, j; bool del; uint8_t x[16]; };
  std::vector<Pending> pending;
  // a full, one-valued ("iso") container of a dimension beyond both layouts — what `Matrix.dense(T)` / `Matrix.iso(x)` make with
  // the default GxB_INDEX_MAX dimensions (pygraphblas/matrix.py:220-230, 234-266): it can be read element-wise, nothing more
  bool iso_full = false; uint8_t iso_val[16] = {0};
  // device
  bool dev_valid = false;
  uint32_t dev_elem_ops = 0; // element reads / writes served on the device in a row (grb_edit_ops.cpp: after a few dozen the host mirror takes over)
  grb::DevCSR csr;          // by-row
  grb::DevCSR csc;          // CSR of the transpose (cached; invalidated with csr)
  grb::DevBitmap bm;        // the bitmap form of a batch matrix (cached beside the CSR, or the only valid form)
  int format = 0;           // GxB_BY_ROW(0) / GxB_BY_COL(1): stored option only
  int sparsity_control = 15;
  double hyper_switch = 0.0625;
  std::string err;
};

struct GrB_Vector_opaque {
  uint64_t magic = GRB_MAGIC;
  GrB_Type type = nullptr;
  GrB_Index n = 0;
  bool host_valid = true;
  std::vector<GrB_Index> hi; std::vector<uint8_t> hx;
  struct Pending { GrB_Index i; bool del; uint8_t x[16]; };
  std::vector<Pending> pending;
  bool iso_full = false; uint8_t iso_val[16] = {0};   // as for matrices: `Vector.iso(x)` of the default size
  bool dev_valid = false;
  grb::DevBuf dval, dpres;   // T[n], u8[n]
  // everything remembered about the device image beyond its bytes.  The rule (grb_vecfacts.hpp): a fact is valid only for the image it was recorded for, and
  // every writer of the image passes one of facts.image_dropped() / image_replaced(nvals, known) / image_extended() before it states what it knows of the new one
  grb::VecFacts facts;
  // ---- non-blocking state (grb_lazy.cpp; the library is initialised GrB_NONBLOCKING by the reference, pygraphblas/__init__.py:251-256) ----
  // lazy == 1: `w(:) = lazy_fill` over every index was requested and nothing has been written yet (no buffers): a product that
  //            accumulates into w with its monoid's operator folds the fill into its own store; anything else materialises it.
  // lazy == 2: w is the output of queued element-wise operations (its stored value, if any, is the old one).
  // q_reads:   queued operations that read this vector's stored value — it must not change before they ran.
  // Every access goes through vec_gate() (vec_to_device / vec_to_host / vec_nvals in grb_mirror.cpp / the entry points of grb_container.cpp).
  int lazy = 0; uint8_t lazy_fill[16] = {0}; int q_reads = 0;
  grb::DevBuf dcode;   // the buffer of the code bytes (facts.code_valid): a buffer, not a fact — kept across the transitions and reused
  uint32_t dev_elem_ops = 0;   // element reads served on the device in a row (grb_edit_ops.cpp: after a few dozen the host mirror takes over)
  int sparsity_control = 15;
  std::string err;
};

struct GxB_Scalar_opaque {
  uint64_t magic = GRB_MAGIC;
  GrB_Type type = nullptr; bool has = false; uint8_t x[16] = {0};
  std::string err;
};

typedef GrB_Matrix_opaque* GrB_Matrix;
typedef GrB_Vector_opaque* GrB_Vector;
typedef GxB_Scalar_opaque* GxB_Scalar;

namespace grb {

// ---- containers (the images and their transitions: grb_mirror.cpp; what only the object-model files share: grb_container.hpp) ----
void mat_host_assemble(GrB_Matrix A);     // apply pending edits to the host mirror
void mat_to_host(GrB_Matrix A);           // ensure host mirror valid (downloads if needed)
void mat_to_device(GrB_Matrix A);         // ensure device CSR valid (assembles + uploads)
void mat_invalidate_host(GrB_Matrix A);   // the device image was replaced as a whole: the host mirror, the edit queue, csc, bm and everything in csr.derived go
void mat_invalidate_device(GrB_Matrix A); // host was written: no device image
uint64_t mat_nvals(GrB_Matrix A);
// batch matrices (a few very long rows) in bitmap form — grb_mxm_rows.cpp
bool mat_batch_shape(uint64_t nrows, uint64_t ncols, int type_code);   // <= 64 rows of >= 65536 (a multiple of 64) columns, a non-complex type, < 2^32 positions
grb::DevBitmap& mat_bitmap(GrB_Matrix A);          // ensure the bitmap form is valid (made from the CSR when it is not)
void mat_bitmap_to_csr(GrB_Matrix A);              // ... and the CSR from the bitmap (what mat_to_device does for a matrix that lives as a bitmap)
uint64_t mat_bitmap_nvals(GrB_Matrix A);           // entries of the bitmap (counted once, then remembered)
inline bool mat_bitmap_only(GrB_Matrix A) { return A->bm.valid && !A->dev_valid && !A->host_valid; }
// hypersparse containers (a dimension beyond the device layouts): the products and eWise operations on the index sets that occur (grb_hyper.cpp)
bool is_hyper(const GrB_Matrix_opaque* A); bool is_hyper(const GrB_Vector_opaque* v);
void hyper_mxv_like(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, GrB_Semiring semiring, GrB_Matrix A, GrB_Vector u, GrB_Descriptor desc, bool is_vxm);
void hyper_mxm(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, GrB_Semiring semiring, GrB_Matrix A, GrB_Matrix B, GrB_Descriptor desc);
// What an element-wise operation makes of a position only ONE operand holds: eWiseMult has no entry there, eWiseAdd copies the operand's (the operator is not
// called), GxB_eWiseUnion calls the operator with a scalar in the missing operand's place — op(a, beta) / op(alpha, b).  (0 / 1: what `bool is_union` was.)
enum EwiseKind { EW_MULT = 0, EW_ADD = 1, EW_UNION = 2 };
struct EwiseMode {
  int kind; GxB_Scalar alpha = nullptr, beta = nullptr;      // the union's scalars as the caller gave them (checked: initialised, with an entry, not complex)
  bool whole() const { return kind != EW_MULT; }              // T's pattern is the union of the operands' patterns (else the intersection)
  bool fills() const { return kind == EW_UNION; }
  // alpha in the operator's x type, beta in its y type (16 bytes each), as the bound scalar of apply_BinaryOp1st / 2nd is cast
  void cast_fill(int xcode, int ycode, uint8_t* a16, uint8_t* b16) const;
};
void hyper_vec_ewise(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, GrB_BinaryOp op, GrB_Vector u, GrB_Vector v, GrB_Descriptor desc, const EwiseMode& mode);
void hyper_mat_ewise(GrB_Matrix C, GrB_Matrix M, GrB_BinaryOp accum, GrB_BinaryOp op, GrB_Matrix A, GrB_Matrix B, GrB_Descriptor desc, const EwiseMode& mode);
// scalar into a region on the host mirror (grb_assign_ops.cpp): for complex containers and for dimensions beyond the device layout
void host_assign_scalar(GrB_Matrix C, GrB_Matrix Mask, GrB_BinaryOp accum, const void* x, int xcode, const GrB_Index* I, GrB_Index ni, const GrB_Index* J, GrB_Index nj, GrB_Descriptor desc);
void host_assign_scalar(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, const void* x, int xcode, const GrB_Index* I, GrB_Index ni, GrB_Descriptor desc);
void vec_resolve(GrB_Vector v);           // complete deferred work that involves v (grb_lazy.cpp)
// the edit queue of a container that lives in HBM only (grb_edit_ops.cpp): `pending` with host_valid == false holds setElement / removeElement records that the
// device image has not seen yet; they are applied there (grb_edit.hip) before anything reads or replaces that image
inline bool mat_edits_queued(const GrB_Matrix_opaque* A) { return !A->pending.empty() && !A->host_valid; }
inline bool vec_edits_queued(const GrB_Vector_opaque* v) { return !v->pending.empty() && !v->host_valid; }
void mat_edit_flush(GrB_Matrix A);
void vec_edit_flush(GrB_Vector v);
inline void vec_gate(GrB_Vector v) { if (v->lazy | v->q_reads) vec_resolve(v); if (vec_edits_queued(v)) vec_edit_flush(v); }
void vec_overwritten(GrB_Vector v);       // v's value is about to be replaced as a whole: deferred work that only produced it is dropped
uint32_t* any_true_acquire(uint32_t* tag);        // (grb_any_true.cpp) a device word a BOOL product kernel sets to the (fresh, non-zero) tag when it writes a true value (see VecFacts::lor_state)
void any_true_written(GrB_Vector w_or_null, const void* key, uint32_t tag, uint64_t fe_key = 0, uint32_t fe_nblocks = 0);    // a kernel honoured it; w's device buffers `key` are the result it describes (nullptr: nobody's); fe_key != 0: the kernel also filled the edge summary (counted in the row pointers with that serial)
bool dist_exchange_pending();                   // grb_dist.cpp: GrBX_Vector_allgatherv_start without its GrBX_dist_wait yet
// GRB_MI355X_DETERMINISTIC=1: floating-point PLUS results are the same bits in every run (mxm: grb_matrix_ops.cpp; vxm / mxv: no push step, whose atomics land in any order)
inline bool deterministic_env() { const char* e = getenv("GRB_MI355X_DETERMINISTIC"); return e && atoi(e) != 0; }
unsigned long long* fe_summary_host();      // SpmvCall::fe_host: the page-locked pairs of the result summary (device address), for the product that just called any_true_acquire
bool any_true_lookup(GrB_Vector u, bool* value);
bool nonblocking();                       // GrB_init(GrB_NONBLOCKING) and not GRB_MI355X_BLOCKING=1
void vec_host_assemble(GrB_Vector v);
void vec_to_host(GrB_Vector v);
void vec_to_device(GrB_Vector v);
void vec_invalidate_host(GrB_Vector v, uint64_t nvals = 0, bool known = false);   // a kernel replaced the device image (facts.image_replaced): the host mirror goes
void vec_device_extended(GrB_Vector v);   // ... or only added entries to it (facts.image_extended)
void vec_invalidate_device(GrB_Vector v); // host was written: the device image goes (facts.image_dropped)
uint64_t vec_nvals(GrB_Vector v);
uint64_t vec_dev_nvals(GrB_Vector v);   // entry count of the (valid) device bitmap
const DevCSR& mat_csc(GrB_Matrix A);      // cached CSR of A^T (device)

bool check_obj(const void* p);            // magic check
GrB_Type type_by_code(int code);

// ---- what the route predicates read of a container (the policy and the thresholds: grb_route.hpp) ----
inline int route_env(const char* name) { const char* e = getenv(name); return (e && *e) ? (atoi(e) != 0 ? 1 : 0) : -1; }      // a route's test hook: 0 host, 1 device, -1 not set
// an HBM layout exists: not hypersparse, not complex, not a full one-valued container (nullptr: no such operand) ... and for mat_capable not a bitmap-only batch matrix
inline bool dev_capable(GrB_Matrix A) { return !A || (!is_hyper(A) && A->type->code < T_FC32 && !A->iso_full); }
inline bool dev_capable(GrB_Vector v) { return !v || (!is_hyper(v) && v->type->code < T_FC32 && !v->iso_full); }
inline bool mat_capable(GrB_Matrix A) { return dev_capable(A) && !(A && mat_bitmap_only(A)); }
inline bool hbm_only(GrB_Matrix A) { return A->dev_valid && !A->host_valid; }      // it lives in HBM: it is not downloaded to pick a route
inline bool hbm_only(GrB_Vector v) { return v->dev_valid && !v->host_valid; }
// (the count of a valid host mirror, or of the device CSR: no device work.  With element edits queued on an HBM-only matrix — grb_edit_ops.cpp — the CSR header is read
//  WITHOUT a flush here: the count is off by at most the queue's length, and it only picks a route.)
inline uint64_t entries_of(GrB_Matrix A) { return A->host_valid ? mat_nvals(A) : (uint64_t)A->csr.nnz; }
inline uint64_t entries_known(GrB_Vector u) { return u->host_valid ? vec_nvals(u) : (u->facts.dnvals_known ? u->facts.dnvals : 0); }      // (no device work for a count)
// the second stage for an operand whose count is taken from a valid host mirror only (extract, diag, sort)
inline bool route_by_host_count(GrB_Matrix A, uint64_t min_entries) { return route_by_size(hbm_only(A), A->host_valid, A->host_valid ? mat_nvals(A) : 0, min_entries); }
inline bool route_by_host_count(GrB_Vector u, uint64_t min_entries) { return route_by_size(hbm_only(u), u->host_valid, u->host_valid ? vec_nvals(u) : 0, min_entries); }

// scalar conversion between any two built-in real types through host code
void cast_scalar(int dst_code, void* dst, int src_code, const void* src);

// ---- kernels launched from the op drivers (see the respective .hip files) -----------------------
// grb_transpose.hip
void csr_transpose(const DevCSR& A, size_t tsize, DevCSR& At);
// grb_vecops.hip
void vec_cast_values(int dst_code, void* dst, int src_code, const void* src, uint64_t n);
void vec_cast_fill_values(int dst_code, void* dst, int src_code, const void* src, const uint8_t* pres, uint64_t n, const void* fill);
void build_allow(uint64_t n, int mcode, const void* mval, const uint8_t* mpres, bool structural,
                 bool complement, uint8_t* allow);
uint64_t count_present(const uint8_t* pres, uint64_t n);
void init_entries_small(uint32_t k, const uint64_t* idx_host, const uint8_t* vals_host, size_t ts, void* val, uint8_t* pres, uint64_t n);      // zero both arrays of an n-vector and write k <= 16 entries: one launch   // k <= 16, ts <= 8: entries passed as kernel arguments (no staging, no synchronisation)
void write_small_list(uint32_t k, const uint32_t* idx_host, uint32_t* out_dev);   // k <= 64 indices passed as kernel arguments
void scatter_entries(uint32_t k, const uint32_t* idx_dev, const void* vals_dev, size_t ts, void* val, uint8_t* pres);   // val[idx[e]] = vals[e], pres[idx[e]] = 1
uint64_t frontier_edges(const uint8_t* pres, const uint32_t* rowptr, uint64_t n);
uint64_t frontier_edges_and_count(const uint8_t* pres, const uint32_t* rowptr, uint64_t n, uint64_t* count);

}  // namespace grb
