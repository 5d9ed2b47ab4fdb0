// grb_usersr.cpp — user-defined monoids and semirings: the objects, the text of their two kernels and the launches.
//
//   GrBX_Monoid_new_user   (&m, op, identity)     op: a user-defined binary operator (GxB_BinaryOp_new) or a built-in of the list below; identity: one value of op's type
//   GrBX_Semiring_new_user (&s, add, mul)         add: such a monoid or a built-in monoid of the list; mul: as op
// GrB_Monoid_new_<T> / GrB_Semiring_new keep refusing a user-defined operator (grb_runtime.cpp); these two are the way in.  All of an object's types are ONE of
// the 11 real built-in types.  The built-ins the generated text can express: FIRST, SECOND, PAIR, PLUS, MINUS, TIMES, MIN, MAX on every such type and LOR / LAND /
// LXOR on BOOL, each emitted so that it gives the bits of apply_binop (grb_ops.hpp): integers wrap, floating MIN / MAX are fmin / fmax, BOOL arithmetic is logic.
// The objects keep POINTERS to their operators (freeing one while the object lives is the caller's error, as in SuiteSparse), have no terminal value, and are
// released by GrB_Monoid_free / GrB_Semiring_free.  Nothing up to here needs a device.
//
// Running one — GrB_mxm, GrB_mxv, GrB_vxm (the off-table drivers of grb_matrix_ops.cpp / grb_mxv.cpp, through a SemiringRoute: grb_opcommon.hpp) and
// GrB_Matrix_reduce_Monoid (a block of do_reduce_vector) — goes through two kernels
// generated around the definitions like grb_userop.cpp's (every function of a definition made a device function, each definition in a namespace of its own so that
// two operators may share a function name) and compiled through the same table and code-object cache (`usersr-<hash>.co`):
//   grb_usersr_rows      mxv / vxm / reduce_rows: a wave64 per row of the CSR the driver picked, rows in a grid-stride loop; lanes stride over the row's entries,
//                        fold their products in ascending position starting from the first, then combine in a fixed tree of (value, has) pairs
//   grb_usersr_product   mxm: a wave64 per row i of a T whose pattern exists; k walks A(i,:) in ascending position, lanes stride over B(k,:), bisect the column in
//                        T(i,:) and fold into that slot — accumulators and `seen` flags in LDS for rows of <= 128 entries, in T.val and a byte array otherwise
// Two rules: the monoid's identity is never combined into a result (presence is carried by flags, never by a value), and the multiplier's argument order —
// mul(A(i,k), B(k,j)) for mxv and mxm, mul(u(i), A(i,j)) for vxm — is a constant of the text.
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_userop.hpp"
#include <sstream>

namespace grb {
namespace {

constexpr int PRODUCT_LDS_ROW = 128;      // entries of a row of T whose accumulators live in LDS (4 waves x 128 x (8 + 1) bytes per workgroup)

const char* kind_name(int kind) { switch (kind) { case USK_MXV: return "mxv"; case USK_VXM: return "vxm"; case USK_MXM: return "mxm"; default: return "reduce_rows"; } }

// can the text express this built-in operator on this type?
bool expressible(int op, int tcode) {
  switch (op) {
    case B_FIRST: case B_SECOND: case B_PAIR: case B_PLUS: case B_MINUS: case B_TIMES: case B_MIN: case B_MAX: return true;
    case B_LOR: case B_LAND: case B_LXOR: return tcode == T_BOOL;
    default: return false;
  }
}

// the expression of a built-in operator over `a` and `b` of type T (U: its unsigned counterpart): the bits of apply_binop<T>
std::string builtin_expr(int op, int tcode) {
  const bool is_bool = tcode == T_BOOL, is_fp = tcode == T_FP32 || tcode == T_FP64;
  if (is_bool) switch (op) {
    case B_FIRST: return "a"; case B_SECOND: return "b"; case B_PAIR: return "true";
    case B_MIN: case B_TIMES: case B_LAND: return "(a && b)";
    case B_MAX: case B_PLUS: case B_LOR: return "(a || b)";
    case B_MINUS: case B_LXOR: return "(a != b)";
    default: break;
  }
  else switch (op) {
    case B_FIRST: return "a"; case B_SECOND: return "b"; case B_PAIR: return "(T)1";
    case B_PLUS: return is_fp ? "(a + b)" : "(T)((U)a + (U)b)";
    case B_MINUS: return is_fp ? "(a - b)" : "(T)((U)a - (U)b)";
    case B_TIMES: return is_fp ? "(a * b)" : "(T)(U)((unsigned long long)(U)a * (unsigned long long)(U)b)";
    case B_MIN: return is_fp ? (tcode == T_FP32 ? "fminf(a, b)" : "fmin(a, b)") : "(a < b ? a : b)";
    case B_MAX: return is_fp ? (tcode == T_FP32 ? "fmaxf(a, b)" : "fmax(a, b)") : "(a > b ? a : b)";
    default: break;
  }
  fail(GrB_PANIC, "user-defined semiring: the kernel text cannot express built-in operator code " + std::to_string(op) + " (usersr_check lets none through)");
}
const char* unsigned_c_type(int tcode) {
  switch (type_size(tcode)) { case 1: return "unsigned char"; case 2: return "unsigned short"; case 4: return "unsigned int"; default: return "unsigned long long"; }
}

// grb_<role>_f(a, b): the user's function called through pointers, or a built-in's expression
void emit_operator(std::ostringstream& o, const char* role, const GrB_BinaryOp_opaque* op, int tcode) {
  if (is_user(op)) {
    o << "namespace grb_" << role << "_ns {\n#pragma clang force_cuda_host_device begin\n" << op->defn << "\n#pragma clang force_cuda_host_device end\n}\n"
      << "__device__ __forceinline__ T grb_" << role << "_f(T a, T b) { T z; grb_" << role << "_ns::" << op->name << "(&z, &a, &b); return z; }\n";
  } else {
    o << "__device__ __forceinline__ T grb_" << role << "_f(T a, T b) { return " << builtin_expr(op->opcode, tcode) << "; }      // " << op->name << "\n";
  }
}

// One text per (add, mul, type, kind): the operator section (plain C++ once __device__ and __forceinline__ are defined away — the CPU suite compiles it for the
// host), then the kernel of the kind.
std::string generate(int kind, const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul, int tcode) {
  std::ostringstream o;
  o << userop_prelude() << "typedef " << userop_c_type(tcode) << " T; typedef " << unsigned_c_type(tcode) << " U;\n";
  emit_operator(o, "add", add, tcode);
  if (kind != USK_REDUCE_ROWS) emit_operator(o, "mul", mul, tcode);
  o << "// ---- kernel ----\n"
       "#define GRB_KIND " << kind << "      // 0 mxv: mul(a, u)   1 vxm: mul(u, a)   2 mxm: mul(a, b)   3 reduce_rows: the matrix value itself\n"
       "__device__ __forceinline__ T grb_down(T v, int d) {      // the value of lane + d\n"
       "  union { T t; int i[2]; } w; w.i[0] = 0; w.i[1] = 0; w.t = v;\n"
       "  w.i[0] = __shfl_down(w.i[0], d, 64); if (sizeof(T) == 8) w.i[1] = __shfl_down(w.i[1], d, 64);\n"
       "  return w.t;\n"
       "}\n";
  if (kind != USK_MXM) {
    // rowptr / col / aval: the CSR whose rows are the output's positions; uval / upres: the operand vector (upres 0: full); allow: 0 = every row
    o << "extern \"C\" __global__ void __launch_bounds__(256) grb_usersr_rows(const unsigned* rowptr, const unsigned* col, const T* aval, const T* uval, const unsigned char* upres,\n"
         "    const unsigned char* allow, T* tval, unsigned char* tpres, unsigned nrows) {\n"
         "  const unsigned lane = threadIdx.x & 63u;\n"
         "  const unsigned long long nwaves = (unsigned long long)gridDim.x * 4ull;\n"
         "  for (unsigned long long r = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) >> 6; r < nrows; r += nwaves) {      // (r is the same in every lane of a wave)\n"
         "    if (allow && !allow[r]) { if (lane == 0) { tval[r] = (T)0; tpres[r] = 0; } continue; }\n"
         "    const unsigned pb = rowptr[r], pe = rowptr[r + 1];\n"
         "    T acc = (T)0; bool has = false;\n"
         "    for (unsigned p = pb + lane; p < pe; p += 64u) {      // a lane's products in ascending position, from its first\n"
         "#if GRB_KIND == 3\n"
         "      const T prod = aval[p];\n"
         "#else\n"
         "      const unsigned j = col[p];\n"
         "      if (upres && !upres[j]) continue;\n"
         "      const T a = aval[p], u = uval[j];\n"
         "#if GRB_KIND == 1\n"
         "      const T prod = grb_mul_f(u, a);\n"
         "#else\n"
         "      const T prod = grb_mul_f(a, u);\n"
         "#endif\n"
         "#endif\n"
         "      acc = has ? grb_add_f(acc, prod) : prod; has = true;\n"
         "    }\n"
         "#pragma unroll\n"
         "    for (int d = 32; d >= 1; d >>= 1) {      // the fixed tree: lane l takes lane l + d, the lower lane's sum on the left\n"
         "      const T oacc = grb_down(acc, d); const int ohas = __shfl_down(has ? 1 : 0, d, 64);\n"
         "      if (lane + d < 64u && ohas) { acc = has ? grb_add_f(acc, oacc) : oacc; has = true; }\n"
         "    }\n"
         "    if (lane == 0) { tval[r] = has ? acc : (T)0; tpres[r] = has ? 1 : 0; }\n"
         "  }\n"
         "}\n";
  } else {
    // crp / ccol: T's pattern (columns ascending within a row); cval: its values; seen: one byte per entry of T, all 0 at the start (rows beyond the LDS capacity)
    o << "#define GRB_CAP " << PRODUCT_LDS_ROW << "\n"
         "extern \"C\" __global__ void __launch_bounds__(256) grb_usersr_product(const unsigned* arp, const unsigned* acol, const T* aval, const unsigned* brp, const unsigned* bcol,\n"
         "    const T* bval, const unsigned* crp, const unsigned* ccol, T* cval, unsigned char* seen, unsigned nrows) {\n"
         "  __shared__ T lacc[4][GRB_CAP]; __shared__ unsigned char lseen[4][GRB_CAP];\n"
         "  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;\n"
         "  const unsigned long long nwaves = (unsigned long long)gridDim.x * 4ull;\n"
         "  for (unsigned long long i = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) >> 6; i < nrows; i += nwaves) {      // (i is the same in every lane of a wave)\n"
         "    const unsigned cb = crp[i], ce = crp[i + 1], len = ce - cb;\n"
         "    if (!len) continue;\n"
         "    const bool in_lds = len <= GRB_CAP;\n"
         "    if (in_lds) for (unsigned q = lane; q < len; q += 64u) lseen[w][q] = 0;\n"
         "    // a slot written by one lane at one k is read by another lane of this wave at the next: every step ends with the wave's stores complete and visible\n"
         "    __threadfence_block();\n"
         "    for (unsigned pa = arp[i]; pa < arp[i + 1]; pa++) {      // k in ascending position\n"
         "      const unsigned k = acol[pa]; const T a = aval[pa];\n"
         "      const unsigned bb = brp[k], be = brp[k + 1];\n"
         "      for (unsigned pb = bb + lane; pb < be; pb += 64u) {      // the columns of B(k,:) are distinct: no two lanes share a slot within one k\n"
         "        const unsigned j = bcol[pb];\n"
         "        unsigned lo = cb, hi = ce;\n"
         "        while (lo < hi) { const unsigned mid = lo + ((hi - lo) >> 1); if (ccol[mid] < j) lo = mid + 1; else hi = mid; }\n"
         "        if (lo >= ce || ccol[lo] != j) continue;      // not in T's row: the mask dropped it\n"
         "        const T prod = grb_mul_f(a, bval[pb]);\n"
         "        if (in_lds) { const unsigned q = lo - cb; lacc[w][q] = lseen[w][q] ? grb_add_f(lacc[w][q], prod) : prod; lseen[w][q] = 1; }\n"
         "        else { cval[lo] = seen[lo] ? grb_add_f(cval[lo], prod) : prod; seen[lo] = 1; }      // (a store of T's own width: the neighbours belong to other lanes)\n"
         "      }\n"
         "      __threadfence_block();\n"
         "    }\n"
         "    if (in_lds) for (unsigned q = lane; q < len; q += 64u) cval[cb + q] = lseen[w][q] ? lacc[w][q] : (T)0;\n"
         "    __threadfence_block();      // (the LDS rows are free for the wave's next row)\n"
         "  }\n"
         "}\n";
  }
  return o.str();
}

std::string both_names(const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul) {
  std::string s;
  if (is_user(add)) s = add->name;
  if (mul && is_user(mul) && s != mul->name) s += (s.empty() ? "" : " / ") + std::string(mul->name);
  return s.empty() ? std::string(add->name) : s;
}

// a wave per row (row_launch_blocks, grb_device.hpp: the kernels stride)
void launch_rows(hipFunction_t fn, uint64_t nrows, void** args) {
  GRB_HIP(hipModuleLaunchKernel(fn, row_launch_blocks(nrows), 1, 1, 256, 1, 1, 0, stream(), args, nullptr));
  userop_count_launch();
}

int checked_type(const GrB_BinaryOp_opaque* add) {
  const int tcode = add->ztype->code;
  if (!userop_c_type(tcode)) fail(GrB_DOMAIN_MISMATCH, std::string("user-defined semiring over ") + add->name + ": not one of the real built-in types");
  return tcode;
}

// why `op` cannot be an operator of a user-defined monoid / semiring ("" when it can)
std::string operator_refusal(const GrB_BinaryOp_opaque* op) {
  const std::string who = std::string(is_user(op) ? "user-defined operator " : "operator ") + op->name;
  if (op->xtype != op->ztype || op->ytype != op->ztype) return who + ": the types of a user-defined monoid's or semiring's operators must be one type (a comparison, or differing types, cannot be used)";
  if (!userop_c_type(op->ztype->code)) return who + ": complex and user-defined types are out of the scope of user-defined monoids and semirings";
  if (!is_user(op) && !expressible(op->opcode, op->ztype->code))
    return who + ": the built-in operators of a user-defined monoid or semiring are FIRST, SECOND, PAIR, PLUS, MINUS, TIMES, MIN, MAX, and LOR / LAND / LXOR on BOOL";
  return "";
}

// why the pair cannot run ("" when it can): each operator on its own, then the multiplier's type against the monoid's
std::string pair_refusal(const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul) {
  std::string why = mul ? operator_refusal(mul) : std::string();
  if (why.empty()) why = operator_refusal(add);
  if (why.empty() && mul && mul->ztype != add->ztype)
    why = std::string(is_user(mul) ? "user-defined operator " : "operator ") + mul->name + ": its type differs from the type of the monoid's operator " + add->name;
  return why;
}

}  // namespace

void usersr_check(const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul) {
  const std::string why = pair_refusal(add, mul);
  if (!why.empty()) fail(GrB_DOMAIN_MISMATCH, "user-defined semiring: " + why);
}

std::string usersr_plan(int kind, const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul) {
  return std::string("usersr<add=") + add->name + ",mul=" + (mul ? mul->name : "none") + ",type=" + add->ztype->name + ",kind=" + kind_name(kind) + "> ";
}

void usersr_rows(int kind, const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul, const DevCSR& R, const void* aval, const void* uval, const uint8_t* upres,
                 const uint8_t* allow, void* tval, uint8_t* tpres) {
  usersr_check(add, kind == USK_REDUCE_ROWS ? nullptr : mul);
  const int tcode = checked_type(add);
  hipFunction_t fn = userop_kernel_of(generate(kind, add, mul, tcode), both_names(add, mul).c_str(), "grb_usersr_rows", "usersr");
  g_last_plan = usersr_plan(kind, add, mul) + "grb_usersr_rows ";
  if (!R.nrows) return;
  const uint32_t* rowptr = R.rowptr.as<uint32_t>(); const uint32_t* col = R.col.as<uint32_t>(); unsigned nrows = R.nrows;
  void* args[] = {(void*)&rowptr, (void*)&col, (void*)&aval, (void*)&uval, (void*)&upres, (void*)&allow, (void*)&tval, (void*)&tpres, (void*)&nrows};
  launch_rows(fn, R.nrows, args);
}

void usersr_product_values(const GrB_BinaryOp_opaque* add, const GrB_BinaryOp_opaque* mul, const DevCSR& A, const void* aval, const DevCSR& B, const void* bval, DevCSR& T) {
  usersr_check(add, mul);
  const int tcode = checked_type(add);
  hipFunction_t fn = userop_kernel_of(generate(USK_MXM, add, mul, tcode), both_names(add, mul).c_str(), "grb_usersr_product", "usersr");
  g_last_plan += "grb_usersr_product ";
  if (!T.nnz || !T.nrows) return;
  DevBuf seen(T.nnz + 16);
  GRB_HIP(hipMemsetAsync(seen.p, 0, T.nnz, stream()));
  const uint32_t* arp = A.rowptr.as<uint32_t>(); const uint32_t* acol = A.col.as<uint32_t>(); const uint32_t* brp = B.rowptr.as<uint32_t>(); const uint32_t* bcol = B.col.as<uint32_t>();
  const uint32_t* crp = T.rowptr.as<uint32_t>(); const uint32_t* ccol = T.col.as<uint32_t>(); void* cval = T.val.p; uint8_t* sp = seen.as<uint8_t>(); unsigned nrows = T.nrows;
  void* args[] = {(void*)&arp, (void*)&acol, (void*)&aval, (void*)&brp, (void*)&bcol, (void*)&bval, (void*)&crp, (void*)&ccol, (void*)&cval, (void*)&sp, (void*)&nrows};
  launch_rows(fn, T.nrows, args);
  GRB_HIP(hipStreamSynchronize(stream()));      // `seen` returns to the pool when this scope ends
}

}  // namespace grb

using namespace grb;

extern "C" {

GrB_Info GrBX_Monoid_new_user(GrB_Monoid* m, GrB_BinaryOp op, const void* identity) {
  if (!m || !op || !identity) return GrB_NULL_POINTER;
  if (!check_obj(op)) return GrB_UNINITIALIZED_OBJECT;
  const std::string why = operator_refusal(op);
  if (!why.empty()) { g_last_error = "GrBX_Monoid_new_user: " + why; return GrB_DOMAIN_MISMATCH; }
  auto* r = new (std::nothrow) GrB_Monoid_opaque{GRB_MAGIC, op, {0}, false, {0}, "", false, true};
  if (!r) return GrB_OUT_OF_MEMORY;
  memcpy(r->identity, identity, op->ztype->size);
  snprintf(r->name, sizeof r->name, "user_%s", op->name); *m = r; return GrB_SUCCESS;
}

GrB_Info GrBX_Semiring_new_user(GrB_Semiring* s, GrB_Monoid add, GrB_BinaryOp mul) {
  if (!s || !add || !mul) return GrB_NULL_POINTER;
  if (!check_obj(add) || !check_obj(mul) || !check_obj(add->op)) return GrB_UNINITIALIZED_OBJECT;
  const std::string why = pair_refusal(add->op, mul);
  if (!why.empty()) { g_last_error = "GrBX_Semiring_new_user: " + why; return GrB_DOMAIN_MISMATCH; }
  auto* r = new (std::nothrow) GrB_Semiring_opaque{GRB_MAGIC, add, mul, "", false, true};
  if (!r) return GrB_OUT_OF_MEMORY;
  snprintf(r->name, sizeof r->name, "user_%.24s_%.24s", add->op->name, mul->name); *s = r; return GrB_SUCCESS;
}

// SuiteSparse's introspection of a monoid, for built-in and user-defined ones alike: the identity (one value of the operator's type), and whether a terminal value
// exists (a GrBX_Monoid_new_user monoid has none)
GrB_Info GxB_Monoid_identity(void* identity, GrB_Monoid m) {
  if (!identity || !m) return GrB_NULL_POINTER; if (!check_obj(m)) return GrB_UNINITIALIZED_OBJECT;
  memcpy(identity, m->identity, m->op->ztype->size); return GrB_SUCCESS;
}
GrB_Info GxB_Monoid_terminal(bool* has_terminal, void* terminal, GrB_Monoid m) {
  if (!has_terminal || !terminal || !m) return GrB_NULL_POINTER; if (!check_obj(m)) return GrB_UNINITIALIZED_OBJECT;
  *has_terminal = m->has_terminal; if (m->has_terminal) memcpy(terminal, m->terminal, m->op->ztype->size); return GrB_SUCCESS;
}

// the text that is compiled for the monoid `add` and the multiplier `mul` (NULL for kind 3) in an operation of `kind` (0 mxv, 1 vxm, 2 mxm, 3 reduce_rows)
GrB_Info GrBX_usersr_source(GrB_Monoid add, GrB_BinaryOp mul, int kind, char* buf, size_t len) {
  if (!add || !buf || !len || (!mul && kind != USK_REDUCE_ROWS)) return GrB_NULL_POINTER;
  if (!check_obj(add) || !check_obj(add->op) || (mul && !check_obj(mul))) return GrB_UNINITIALIZED_OBJECT;
  if (kind < USK_MXV || kind > USK_REDUCE_ROWS) return GrB_INVALID_VALUE;
  const std::string why = pair_refusal(add->op, kind == USK_REDUCE_ROWS ? nullptr : mul);
  if (!why.empty()) { g_last_error = "GrBX_usersr_source: " + why; return GrB_DOMAIN_MISMATCH; }
  const std::string src = generate(kind, add->op, kind == USK_REDUCE_ROWS ? nullptr : mul, add->op->ztype->code);
  if (src.size() + 1 > len) return GrB_INSUFFICIENT_SPACE;
  memcpy(buf, src.c_str(), src.size() + 1); return GrB_SUCCESS;
}

}  // extern "C"
