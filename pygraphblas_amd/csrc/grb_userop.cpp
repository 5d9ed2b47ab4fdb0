// grb_userop.cpp — user-defined unary and binary operators, handed over as C source and compiled for the device.
//
//   GxB_UnaryOp_new  (&op, fn, ztype, xtype,        name, defn)      defn: "void NAME (T *z, const T *x) { ... }"
//   GxB_BinaryOp_new (&op, fn, ztype, xtype, ytype, name, defn)      defn: "void NAME (T *z, const T *x, const T *y) { ... }"
// are SuiteSparse 7's forms: `defn` is the C definition of the function `name` (helper functions may precede it in the same string), T the C type of the
// GraphBLAS type, `fn` a host function pointer that a device cannot call — it is kept and never used.  All of an operator's types are ONE of the 11 real
// built-in types (what the reference's binary_op(arg_type) / unary_op(arg_type) decorators offer, pygraphblas/binaryop.py:137, unaryop.py:101).
//
// The object carries a fresh opcode beyond the built-in ones (>= U_USER / B_USER, so every switch over built-in opcodes sees a value it does not
// know and the drivers refuse it before they get there: check_binop, grb_opcommon.hpp), its name and a copy of `defn`.  Nothing here needs a device.
//
// Running one (GrB_apply, GxB_apply_BinaryOp1st / 2nd, eWiseAdd, eWiseMult) goes through the drivers of the built-in operators in grb_matrix_ops.cpp /
// grb_vector_ops.cpp: do_apply / vec_apply_op take an ElemOp (grb_opcommon.hpp), whose elem_eval calls userop_run where a built-in operator's kernel would
// run; do_ewise / vec_ewise_op call it in their general tail.  A block `if (user)` at the top of each driver refuses containers without an HBM layout
// (user_needs_layout, here) and looks at the accumulator BEFORE the dimensions; such a call is never queued and completes deferred work first.  In
// userop_run the definition is embedded in the text of ONE streaming kernel per (operator, kind, type) — every function of the definition made a device
// function by `#pragma clang force_cuda_host_device`, the kind (apply | bind1st | bind2nd | eadd | emult | eunion) a constant of the text — compiled with hipRTC
// through the chain compiler's build_kernel and its code-object cache on disk (grb_jit.hpp: source + architecture + hipRTC version + options; a second
// process compiles nothing), at first use and outside the table's lock.  The kernel is entry-parallel: a lane owns four consecutive positions of the value
// arrays, loaded and stored as one 16-byte pack (4-byte types; two for 8-byte ones), presence bytes as one 4-byte word.  Entries are computed by the
// user's code only; where eWiseAdd finds an entry in one operand alone, the value is copied and the operator is not called; GxB_eWiseUnion (eunion) calls it
// there too, with alpha / beta — two scalar arguments of the kernel — in the missing operand's place.
// A definition that does not compile, or a machine without hipRTC: the operation fails with an error code and the operator's name and the compiler's
// log in the object's error string — there is no interpreter and no host route behind it.
//
//   GxB_SelectOp_new (&op, fn, xtype, ttype, name, defn)             defn: "bool NAME (GrB_Index i, GrB_Index j, const X *x, const K *thunk) { ... }"
// is the same for select: a predicate over an entry's row, column, value (X: the C type of xtype) and the thunk (K: of ttype; NULL: xtype).  GxB_Matrix_select /
// GxB_Vector_select (do_select, vec_select: the built-in select operators' drivers, whose keep bytes it makes) run it through userselect_run: one text per (definition, name, xtype, ttype, matrix | vector) with the kernel grb_userselect, which writes
// one keep byte per stored entry (matrix: per CSR position; vector: per bitmap position, i the position and j 0); the drivers compact / write back as for the
// built-in select operators.
//
// The table of compiled texts, the prelude and the launch counter are shared with the kernels of user-defined monoids and semirings (grb_usersr.cpp:
// userop_kernel_of, userop_prelude, userop_count_launch), the one way a user-defined operator reaches mxm / mxv / vxm and the matrix-to-vector reduction.
#include "grb_api.hpp"
#include "grb_device.hpp"
#include "grb_jit.hpp"
#include "grb_userop.hpp"
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <sstream>

namespace grb {
namespace {

std::atomic<int> g_next_unop{U_NOPS}, g_next_binop{B_NOPS}, g_next_selop{SEL_USER};
std::atomic<uint64_t> g_stat_compiled{0}, g_stat_from_disk{0}, g_stat_launched{0};

const char* c_type(int code) {
  switch (code) {
    case T_BOOL: return "bool"; case T_INT8: return "signed char"; case T_UINT8: return "unsigned char"; case T_INT16: return "short";
    case T_UINT16: return "unsigned short"; case T_INT32: return "int"; case T_UINT32: return "unsigned int"; case T_INT64: return "long long";
    case T_UINT64: return "unsigned long long"; case T_FP32: return "float"; case T_FP64: return "double"; default: return nullptr;
  }
}
const char* kind_name(int kind) {
  switch (kind) { case UK_APPLY: return "apply"; case UK_BIND1ST: return "bind1st"; case UK_BIND2ND: return "bind2nd"; case UK_EADD: return "eadd"; case UK_EUNION: return "eunion"; default: return "emult"; }
}

// what the definition may assume, as <stdint.h>, <stdbool.h> and <math.h> would give it (hipRTC has no system headers; its built-in ones declare the math functions)
const char* PRELUDE =
  "typedef signed char grb_i8; typedef unsigned char grb_u8; typedef short grb_i16; typedef unsigned short grb_u16;\n"
  "typedef int grb_i32; typedef unsigned int grb_u32; typedef long long grb_i64; typedef unsigned long long grb_u64;\n"
  "#define int8_t grb_i8\n#define uint8_t grb_u8\n#define int16_t grb_i16\n#define uint16_t grb_u16\n#define int32_t grb_i32\n#define uint32_t grb_u32\n"
  "#define int64_t grb_i64\n#define uint64_t grb_u64\n"
  "#ifndef INFINITY\n#define INFINITY (__builtin_huge_val())\n#endif\n#ifndef NAN\n#define NAN (__builtin_nan(\"\"))\n#endif\n";

// the kernel around the definition.  One text per (definition, name, kind, type): all of them are part of the cache key because they are part of the text.
std::string generate(int kind, const char* name, const char* defn, int tcode) {
  const int ts = type_size(tcode);
  const bool unary = kind == UK_APPLY;
  std::ostringstream o;
  o << PRELUDE << "#pragma clang force_cuda_host_device begin\n" << defn << "\n#pragma clang force_cuda_host_device end\n"
    << "typedef " << c_type(tcode) << " T;\n"
    << "struct __attribute__((aligned(" << (4 * ts > 16 ? 16 : 4 * ts) << "))) P4 { T v[4]; }; struct __attribute__((aligned(4))) B4 { unsigned char v[4]; };\n";
  if (unary) o << "__device__ __forceinline__ T grb_f(T a, T b) { T z; " << name << "(&z, &a); return z; }\n";
  else o << "__device__ __forceinline__ T grb_f(T a, T b) { T z; " << name << "(&z, &a, &b); return z; }\n";
  // x / y: operand values; px / py: presence bytes (0 = all present); both: eadd over aligned values; s: the bound scalar; z / q: result values / presence;
  // eunion alone has s2: s / s2 stand in for x / y where the other operand alone has the entry
  o << "extern \"C\" __global__ void __launch_bounds__(256) grb_userop(const T* x, const unsigned char* px, const T* y, const unsigned char* py, const unsigned char* both,\n"
       "    T s, " << (kind == UK_EUNION ? "T s2, " : "") << "T* z, unsigned char* q, unsigned long long n, int packed) {\n"
       "  const unsigned long long stride = (unsigned long long)gridDim.x * 1024ull;\n"
       "  for (unsigned long long base = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 4ull; base < n; base += stride) {\n"
       "    const int nv = n - base >= 4ull ? 4 : (int)(n - base);\n"
       "    T a[4], b[4], r[4]; bool ap[4], bp[4], bo[4], rp[4];\n"
       "    if (nv == 4 && packed) {\n"
       "      const P4 va = *(const P4*)(x + base); P4 vb = va; if (y) vb = *(const P4*)(y + base);\n"
       "      B4 wa = {{1, 1, 1, 1}}, wb = {{1, 1, 1, 1}}, wo = {{1, 1, 1, 1}};\n"
       "      if (px) wa = *(const B4*)(px + base); if (py) wb = *(const B4*)(py + base); if (both) wo = *(const B4*)(both + base);\n"
       "#pragma unroll\n"
       "      for (int h = 0; h < 4; h++) { a[h] = va.v[h]; b[h] = vb.v[h]; ap[h] = wa.v[h] != 0; bp[h] = wb.v[h] != 0; bo[h] = wo.v[h] != 0; }\n"
       "    } else {\n"
       "#pragma unroll\n"
       "      for (int h = 0; h < 4; h++) { const unsigned long long i = h < nv ? base + h : base;\n"
       "        a[h] = x[i]; b[h] = y ? y[i] : a[h]; ap[h] = px ? px[i] != 0 : true; bp[h] = py ? py[i] != 0 : true; bo[h] = both ? both[i] != 0 : true; }\n"
       "    }\n"
       "#pragma unroll\n"
       "    for (int h = 0; h < 4; h++) {\n";
  switch (kind) {
    case UK_APPLY:   o << "      rp[h] = ap[h]; r[h] = ap[h] ? grb_f(a[h], a[h]) : (T)0;\n"; break;
    case UK_BIND1ST: o << "      rp[h] = ap[h]; r[h] = ap[h] ? grb_f(s, a[h]) : (T)0;\n"; break;
    case UK_BIND2ND: o << "      rp[h] = ap[h]; r[h] = ap[h] ? grb_f(a[h], s) : (T)0;\n"; break;
    case UK_EMULT:   o << "      rp[h] = ap[h] && bp[h]; r[h] = rp[h] ? grb_f(a[h], b[h]) : (T)0;\n"; break;
    case UK_EUNION:  o << "      rp[h] = ap[h] || bp[h]; r[h] = rp[h] ? grb_f(ap[h] ? a[h] : s, bp[h] ? b[h] : s2) : (T)0;\n"; break;      // the operator is called on every entry
    default:         o << "      const bool two = ap[h] && bp[h] && bo[h]; rp[h] = ap[h] || bp[h];\n"      // one operand alone has the entry: its value is copied, the operator is not called
                          "      r[h] = two ? grb_f(a[h], b[h]) : (ap[h] ? a[h] : (bp[h] ? b[h] : (T)0));\n"; break;
  }
  o << "    }\n"
       "    if (nv == 4 && packed) {\n"
       "      P4 t; B4 u;\n"
       "#pragma unroll\n"
       "      for (int h = 0; h < 4; h++) { t.v[h] = r[h]; u.v[h] = rp[h] ? 1 : 0; }\n"
       "      *(P4*)(z + base) = t; if (q) *(B4*)(q + base) = u;\n"
       "    } else { for (int h = 0; h < nv; h++) { z[base + h] = r[h]; if (q) q[base + h] = rp[h] ? 1 : 0; } }\n"
       "  }\n"
       "}\n";
  return o.str();
}

// the select kernel around a predicate.  One text per (definition, name, xtype, ttype, matrix | vector).  The geometry is grb_userop's: 256 threads, a lane owns
// four consecutive entries.  Packed path (every array aligned, a whole group): row indices, column indices and 4-byte values one 16-byte pack each (8-byte
// values two, narrower ones one narrower pack), presence one 4-byte word, the four keep bytes one 4-byte word; the last partial group and unaligned views
// go entry by entry.  Indices are widened unsigned to GrB_Index; the predicate is not evaluated for an absent position (&& short-circuits).
std::string generate_select(const char* name, const char* defn, int xcode, int tcode, bool on_vector) {
  const int ts = type_size(xcode);
  std::ostringstream o;
  o << PRELUDE << "typedef unsigned long long GrB_Index;\n"
    << "#pragma clang force_cuda_host_device begin\n" << defn << "\n#pragma clang force_cuda_host_device end\n"
    << "typedef " << c_type(xcode) << " X; typedef " << c_type(tcode) << " K;\n"
    << "#define GRB_ON_VECTOR " << (on_vector ? 1 : 0) << "\n"
    << "struct __attribute__((aligned(" << (4 * ts > 16 ? 16 : 4 * ts) << "))) P4 { X v[4]; }; struct __attribute__((aligned(16))) U4 { unsigned v[4]; };\n"
       "struct __attribute__((aligned(4))) B4 { unsigned char v[4]; };\n"
    // rowidx / col: the entries' row and column indices (vector: unused, i is the position and j is 0); x: values; pres: presence bytes (0 = all present);
    // thunk: already in K; keep: one byte per entry
    << "extern \"C\" __global__ void __launch_bounds__(256) grb_userselect(const unsigned* rowidx, const unsigned* col, const X* x, const unsigned char* pres, K thunk,\n"
       "    unsigned char* keep, unsigned long long n, int packed) {\n"
       "  const unsigned long long stride = (unsigned long long)gridDim.x * 1024ull;\n"
       "  const bool positions = GRB_ON_VECTOR || !rowidx;\n"
       "  for (unsigned long long base = ((unsigned long long)blockIdx.x * 256ull + threadIdx.x) * 4ull; base < n; base += stride) {\n"
       "    const int nv = n - base >= 4ull ? 4 : (int)(n - base);\n"
       "    X a[4]; GrB_Index ri[4], cj[4]; bool ap[4]; unsigned char r[4];\n"
       "    if (nv == 4 && packed) {\n"
       "      const P4 va = *(const P4*)(x + base);\n"
       "      B4 wa = {{1, 1, 1, 1}}; if (pres) wa = *(const B4*)(pres + base);\n"
       "      U4 vr = {{0, 0, 0, 0}}, vc = {{0, 0, 0, 0}};\n"
       "      if (!positions) { vr = *(const U4*)(rowidx + base); vc = *(const U4*)(col + base); }\n"
       "#pragma unroll\n"
       "      for (int h = 0; h < 4; h++) { a[h] = va.v[h]; ap[h] = wa.v[h] != 0; ri[h] = positions ? base + h : (GrB_Index)vr.v[h]; cj[h] = positions ? 0ull : (GrB_Index)vc.v[h]; }\n"
       "    } else {\n"
       "#pragma unroll\n"
       "      for (int h = 0; h < 4; h++) { const unsigned long long p = h < nv ? base + h : base;\n"
       "        a[h] = x[p]; ap[h] = pres ? pres[p] != 0 : true; ri[h] = positions ? p : (GrB_Index)rowidx[p]; cj[h] = positions ? 0ull : (GrB_Index)col[p]; }\n"
       "    }\n"
       "#pragma unroll\n"
       "    for (int h = 0; h < 4; h++) r[h] = (ap[h] && " << name << "(ri[h], cj[h], &a[h], &thunk)) ? 1 : 0;\n"
       "    if (nv == 4 && packed) { B4 u; u.v[0] = r[0]; u.v[1] = r[1]; u.v[2] = r[2]; u.v[3] = r[3]; *(B4*)(keep + base) = u; }\n"
       "    else { for (int h = 0; h < nv; h++) keep[base + h] = r[h]; }\n"
       "  }\n"
       "}\n";
  return o.str();
}

struct Entry { bool compiling = false, failed = false; hipFunction_t fn = nullptr; hipModule_t mod = nullptr; std::string log; };
std::map<std::string, Entry> g_cache;      // keyed by the generated text
std::mutex g_mu;
std::condition_variable g_cv;

// the compiled kernel `entry` of the text `src` (code objects on disk: `prefix`-<hash>.co), for the operator `name`
hipFunction_t kernel_of(const std::string& src, const char* name, const char* entry, const char* prefix) {
  if (!jit_available()) fail(GrB_PANIC, std::string("user-defined operator ") + name + ": libhiprtc was not found, and a user-defined operator has no other way to run");
  std::unique_lock<std::mutex> lk(g_mu);
  Entry& en = g_cache[src];
  g_cv.wait(lk, [&] { return !en.compiling; });      // (another thread is compiling this very text: its result serves both)
  if (!en.fn && !en.failed) {
    en.compiling = true;
    lk.unlock();                                     // the compilation (or the read of its cached code object) holds no lock
    hipModule_t mod = nullptr; hipFunction_t f = nullptr; bool from_disk = false; std::string log;
    const bool ok = jit_build_kernel(src, entry, prefix, &mod, &f, &from_disk, &log);
    lk.lock();
    en.compiling = false;
    if (ok) { en.mod = mod; en.fn = f; if (from_disk) g_stat_from_disk++; else g_stat_compiled++; }
    else { en.failed = true; en.log = log.empty() ? std::string("(no compiler log)") : log; }
    g_cv.notify_all();
  }
  if (en.failed) fail(GrB_INVALID_VALUE, std::string("user-defined operator ") + name + ": its definition does not compile for the device:\n" + en.log);
  return en.fn;
}

// the alignment a packed access needs: four values of the type, 16 bytes at the most (8-byte values go as two packs)
size_t pack_bytes(int tcode) { const size_t b = 4 * (size_t)type_size(tcode); return b > 16 ? 16 : b; }
bool aligned(const void* p, size_t a) { return !p || ((uintptr_t)p % a) == 0; }
// both kernels' launch: 256 threads, a lane owns four consecutive entries, at most 16 workgroups per compute unit (the kernels stride)
void launch(hipFunction_t fn, uint64_t n, void** args) {
  uint64_t blocks = (n + 1023) / 1024, cap = (uint64_t)device_cus() * 16; if (cap < 1) cap = 1; if (blocks > cap) blocks = cap;
  GRB_HIP(hipModuleLaunchKernel(fn, (unsigned)blocks, 1, 1, 256, 1, 1, 0, stream(), args, nullptr));
  g_stat_launched++;
}

}  // namespace

hipFunction_t userop_kernel_of(const std::string& src, const char* name, const char* entry, const char* prefix) { return kernel_of(src, name, entry, prefix); }
const char* userop_c_type(int code) { return c_type(code); }
const char* userop_prelude() { return PRELUDE; }
void userop_count_launch() { g_stat_launched++; }

void userop_refuse(const char* opname, const char* where) {
  fail(GrB_DOMAIN_MISMATCH, std::string("user-defined operator ") + opname + " cannot be used as " + where +
                            ": user-defined operators run in apply, apply with a bound scalar, eWiseAdd, eWiseMult and select, and as the operators of a "
                            "GrBX_Monoid_new_user / GrBX_Semiring_new_user object in mxm, mxv, vxm and the matrix-to-vector reduction only");
}

void user_needs_layout(const char* opname, const char* extent, bool hyper, bool cplx) {
  if (hyper) fail(GrB_DOMAIN_MISMATCH, std::string("user-defined operator ") + opname + ": hypersparse containers (a " + extent + " beyond the device layout) are out of its scope");
  if (cplx) fail(GrB_DOMAIN_MISMATCH, std::string("user-defined operator ") + opname + ": complex containers are out of its scope");
}

void userop_run(int kind, const char* name, const char* defn, int tcode, uint64_t n, const void* x, const uint8_t* px, const void* y, const uint8_t* py,
                const uint8_t* both, const void* scalar, void* z, uint8_t* q, const void* scalar2) {
  if (!c_type(tcode) || !defn) fail(GrB_DOMAIN_MISMATCH, std::string("user-defined operator ") + name + ": not one of the real built-in types");
  hipFunction_t fn = kernel_of(generate(kind, name, defn, tcode), name, "grb_userop", "userop");
  g_last_plan = std::string("userop<name=") + name + ",kind=" + kind_name(kind) + ",type=" + type_by_code(tcode)->name + "> grb_userop ";
  if (!n) return;
  const size_t pa = pack_bytes(tcode);
  int packed = aligned(x, pa) && aligned(y, pa) && aligned(z, pa) && aligned(px, 4) && aligned(py, 4) && aligned(both, 4) && aligned(q, 4) ? 1 : 0;
  uint8_t s[16] = {0}, s2[16] = {0}; if (scalar) memcpy(s, scalar, (size_t)type_size(tcode)); if (scalar2) memcpy(s2, scalar2, (size_t)type_size(tcode));
  unsigned long long nn = n;
  void* args[] = {(void*)&x, (void*)&px, (void*)&y, (void*)&py, (void*)&both, (void*)s, (void*)&z, (void*)&q, (void*)&nn, (void*)&packed};
  void* uargs[] = {(void*)&x, (void*)&px, (void*)&y, (void*)&py, (void*)&both, (void*)s, (void*)s2, (void*)&z, (void*)&q, (void*)&nn, (void*)&packed};      // (the union's text has one parameter more)
  launch(fn, n, kind == UK_EUNION ? uargs : args);
}

void userselect_run(const char* name, const char* defn, int xcode, int tcode, bool on_vector, uint64_t n, const uint32_t* rowidx, const uint32_t* col, const void* x,
                    const uint8_t* pres, const void* thunk, uint8_t* keep) {
  if (!c_type(xcode) || !c_type(tcode) || !defn) fail(GrB_DOMAIN_MISMATCH, std::string("user-defined operator ") + name + ": not one of the real built-in types");
  hipFunction_t fn = kernel_of(generate_select(name, defn, xcode, tcode, on_vector), name, "grb_userselect", "userselect");
  g_last_plan = std::string("userselect<name=") + name + ",xtype=" + type_by_code(xcode)->name + ",ttype=" + type_by_code(tcode)->name + ",on=" + (on_vector ? "vector" : "matrix") + "> grb_userselect ";
  if (!n) return;
  if (on_vector) { rowidx = nullptr; col = nullptr; }
  else if (!rowidx || !col) fail(GrB_PANIC, std::string("user-defined operator ") + name + ": select on a matrix without its index arrays");
  int packed = aligned(rowidx, 16) && aligned(col, 16) && aligned(x, pack_bytes(xcode)) && aligned(pres, 4) && aligned(keep, 4) ? 1 : 0;
  uint8_t s[16] = {0}; if (thunk) memcpy(s, thunk, (size_t)type_size(tcode));
  unsigned long long nn = n;
  void* args[] = {(void*)&rowidx, (void*)&col, (void*)&x, (void*)&pres, (void*)s, (void*)&keep, (void*)&nn, (void*)&packed};
  launch(fn, n, args);
}

}  // namespace grb

using namespace grb;

static bool real_type(GrB_Type t) { return t->code >= T_BOOL && t->code <= T_FP64; }
static char* copy_text(const char* t) { const size_t n = strlen(t); char* c = (char*)malloc(n + 1); if (c) memcpy(c, t, n + 1); return c; }
// the name is spliced into the kernel's text as the function to call: it has to be a C identifier
static bool is_identifier(const char* s) {
  if (!*s || (*s >= '0' && *s <= '9')) return false;
  for (; *s; s++) if (!((*s >= 'a' && *s <= 'z') || (*s >= 'A' && *s <= 'Z') || (*s >= '0' && *s <= '9') || *s == '_')) return false;
  return true;
}

// What GxB_UnaryOp_new / GxB_BinaryOp_new / GxB_SelectOp_new (`who`) share: the arguments are there and initialised, the operator's `types` are real built-in
// types (`one_type`: and all the same one), the name is a C identifier, the definition is copied; `make(text)` allocates the object around the copy.
template <class Op, class Make>
static GrB_Info new_userop(Op** op, const char* who, const char* name, const char* defn, std::initializer_list<GrB_Type> types, bool one_type, Make make) {
  if (!op || !name || !defn) return GrB_NULL_POINTER;
  for (GrB_Type t : types) if (!t) return GrB_NULL_POINTER;
  for (GrB_Type t : types) if (!check_obj(t)) return GrB_UNINITIALIZED_OBJECT;
  bool ok = true; for (GrB_Type t : types) ok = ok && real_type(t) && (!one_type || t == *types.begin());
  if (!ok) { g_last_error = std::string(who) + " " + name + (one_type ? ": the operator's types must be one real built-in type" : ": the operator's value and thunk types must be real built-in types"); return GrB_DOMAIN_MISMATCH; }
  if (!is_identifier(name) || strlen(name) >= 40) { g_last_error = std::string(who) + ": the name must be the C identifier of the defined function (at most 39 characters)"; return GrB_INVALID_VALUE; }
  char* text = copy_text(defn); if (!text) return GrB_OUT_OF_MEMORY;
  Op* r = make(text);
  if (!r) { free(text); return GrB_OUT_OF_MEMORY; }
  snprintf(r->name, sizeof r->name, "%s", name); *op = r; return GrB_SUCCESS;
}
// built-in handles stay untouched; a user operator is released and the caller's variable set to NULL (a second free of that variable is a no-op)
template <class Op> static GrB_Info free_userop(Op** op) {
  if (op && *op && check_obj(*op) && is_user(*op)) { (*op)->magic = GRB_FREED; free((*op)->defn); delete *op; *op = nullptr; }
  return GrB_SUCCESS;
}
static GrB_Info copy_out(const std::string& src, char* buf, size_t len) {
  if (src.size() + 1 > len) return GrB_INSUFFICIENT_SPACE;
  memcpy(buf, src.c_str(), src.size() + 1); return GrB_SUCCESS;
}

extern "C" {

GrB_Info GxB_UnaryOp_new(GrB_UnaryOp* op, void* fn, GrB_Type ztype, GrB_Type xtype, const char* name, const char* defn) {
  return new_userop(op, "GxB_UnaryOp_new", name, defn, {ztype, xtype}, true,
                    [&](char* text) { return new (std::nothrow) GrB_UnaryOp_opaque{GRB_MAGIC, g_next_unop++, xtype, ztype, "", fn, text}; });
}
GrB_Info GxB_BinaryOp_new(GrB_BinaryOp* op, void* fn, GrB_Type ztype, GrB_Type xtype, GrB_Type ytype, const char* name, const char* defn) {
  return new_userop(op, "GxB_BinaryOp_new", name, defn, {ztype, xtype, ytype}, true,
                    [&](char* text) { return new (std::nothrow) GrB_BinaryOp_opaque{GRB_MAGIC, g_next_binop++, xtype, ytype, ztype, "", fn, text}; });
}
// a predicate "bool NAME (GrB_Index i, GrB_Index j, const X *x, const K *thunk)": X the C type of xtype, K of ttype (NULL: the same as xtype), both real built-in types
GrB_Info GxB_SelectOp_new(GxB_SelectOp* op, void* fn, GrB_Type xtype, GrB_Type ttype, const char* name, const char* defn) {
  if (!ttype) ttype = xtype;
  return new_userop(op, "GxB_SelectOp_new", name, defn, {xtype, ttype}, false,
                    [&](char* text) { return new (std::nothrow) GxB_SelectOp_opaque{GRB_MAGIC, g_next_selop++, "", fn, xtype, ttype, text}; });
}
GrB_Info GrB_UnaryOp_free(GrB_UnaryOp* op) { return free_userop(op); }
GrB_Info GrB_BinaryOp_free(GrB_BinaryOp* op) { return free_userop(op); }
GrB_Info GxB_SelectOp_free(GxB_SelectOp* op) { return free_userop(op); }
// the text that is compiled for a select operator (`ttype` NULL: the same as `xtype`) used on a matrix (on_vector 0) or on a vector (1)
GrB_Info GrBX_selectop_source(const char* name, const char* defn, GrB_Type xtype, GrB_Type ttype, int on_vector, char* buf, size_t len) {
  if (!name || !defn || !xtype || !buf || !len) return GrB_NULL_POINTER;
  if (!check_obj(xtype) || (ttype && !check_obj(ttype))) return GrB_UNINITIALIZED_OBJECT;
  if (!ttype) ttype = xtype;
  if (xtype->code > T_FP64 || ttype->code > T_FP64) return GrB_DOMAIN_MISMATCH;
  return copy_out(generate_select(name, defn, xtype->code, ttype->code, on_vector != 0), buf, len);
}
GrB_Info GrBX_userop_stats(uint64_t* compiled, uint64_t* loaded_from_disk, uint64_t* launched) {
  if (compiled) *compiled = g_stat_compiled.load(); if (loaded_from_disk) *loaded_from_disk = g_stat_from_disk.load(); if (launched) *launched = g_stat_launched.load();
  return GrB_SUCCESS;
}
// the text that is compiled for an operator of `type` named `name` with the definition `defn` in an operation of `kind` (0 apply, 1 bind1st, 2 bind2nd, 3 eadd, 4 emult)
GrB_Info GrBX_userop_source(const char* name, const char* defn, GrB_Type type, int kind, char* buf, size_t len) {
  if (!name || !defn || !type || !buf || !len) return GrB_NULL_POINTER;
  if (!check_obj(type)) return GrB_UNINITIALIZED_OBJECT;
  if (type->code > T_FP64 || kind < UK_APPLY || kind > UK_EMULT) return GrB_DOMAIN_MISMATCH;
  return copy_out(generate(kind, name, defn, type->code), buf, len);
}
// which images of a container are valid right now (bit 0: the host mirror, bit 1: the HBM image) — looks, changes nothing, completes no deferred work
GrB_Info GrBX_Matrix_residency(const GrB_Matrix A, int* where) {
  if (!A || !where) return GrB_NULL_POINTER; if (!check_obj(A)) return GrB_UNINITIALIZED_OBJECT;
  *where = (A->host_valid ? 1 : 0) | ((A->dev_valid || A->bm.valid) ? 2 : 0); return GrB_SUCCESS;
}
GrB_Info GrBX_Vector_residency(const GrB_Vector v, int* where) {
  if (!v || !where) return GrB_NULL_POINTER; if (!check_obj(v)) return GrB_UNINITIALIZED_OBJECT;
  *where = (v->host_valid ? 1 : 0) | (v->dev_valid ? 2 : 0); return GrB_SUCCESS;
}
// the message of this thread's most recent failure: what the calls without an object to hang it on leave (GxB_*Op_new, GrB_Monoid_new, GrB_Semiring_new)
GrB_Info GrBX_last_error(char* buf, int len) { if (buf && len > 0) snprintf(buf, len, "%s", g_last_error.c_str()); return GrB_SUCCESS; }

}  // extern "C"
