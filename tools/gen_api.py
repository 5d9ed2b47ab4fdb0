#!/usr/bin/env python3
"""Generate the built-in object registry of libgrb_mi355x and the public C header.

Outputs (both committed):
  include/grb_mi355x.h                      public C ABI (also the text the CFFI shim cdef()s)
  pygraphblas_amd/csrc/registry_gen.inc     definitions of every built-in type / operator /
                                            monoid / semiring / descriptor handle

The *names* are the GraphBLAS C API 1.3 + SuiteSparse v5.1 names that pygraphblas discovers by
regex over dir(lib) (reference: pygraphblas/semiring.py:87-121, monoid.py:81-93,
binaryop.py:104-112, unaryop.py:55-63, descriptor.py:148-182, types.py:182-342).  Nothing here is
derived from SuiteSparse sources; the operator set is enumerated from those regexes.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REAL = ["BOOL", "INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64", "FP32", "FP64"]
NUM = REAL[1:]
INTS = ["INT8", "UINT8", "INT16", "UINT16", "INT32", "UINT32", "INT64", "UINT64"]
UINTS = ["UINT8", "UINT16", "UINT32", "UINT64"]
FLOATS = ["FP32", "FP64"]
CTYPE = {"BOOL": "bool", "INT8": "int8_t", "UINT8": "uint8_t", "INT16": "int16_t", "UINT16": "uint16_t",
         "INT32": "int32_t", "UINT32": "uint32_t", "INT64": "int64_t", "UINT64": "uint64_t",
         "FP32": "float", "FP64": "double"}

types = [("GrB_" + t, "T_" + t) for t in REAL] + [("GxB_FC32", "T_FC32"), ("GxB_FC64", "T_FC64")]

unops = []   # (cname, opcode, xtype, ztype)
binops = []  # (cname, opcode, xtype, ytype, ztype)
monoids = []  # (cname, binop cname)
semirings = []  # (cname, monoid cname, binop cname)
_bin_by_key = {}
_mon_by_key = {}


def add_binop(cname, op, x, y, z):
    binops.append((cname, op, x, y, z))
    _bin_by_key.setdefault((op, x), cname)


# ---- unary ops -----------------------------------------------------------------------------
for t in REAL:
    for pre, op in [("GrB", "IDENTITY"), ("GrB", "AINV"), ("GrB", "MINV"), ("GrB", "ABS"), ("GxB", "ABS"),
                    ("GxB", "ONE"), ("GxB", "LNOT")]:
        unops.append((f"{pre}_{op}_{t}", "U_" + op, t, t))
unops.append(("GrB_LNOT", "U_LNOT", "BOOL", "BOOL"))
for t in INTS:
    unops.append((f"GrB_BNOT_{t}", "U_BNOT", t, t))
for t in FLOATS:
    for op in ["SQRT", "LOG", "EXP", "LOG2", "SIN", "COS", "TAN", "ACOS", "ASIN", "ATAN", "SINH", "COSH", "TANH",
               "ACOSH", "ASINH", "ATANH", "SIGNUM", "CEIL", "FLOOR", "ROUND", "TRUNC", "EXP2", "EXPM1", "LOG10",
               "LOG1P", "LGAMMA", "TGAMMA", "ERF", "ERFC", "FREXPX", "FREXPE"]:
        unops.append((f"GxB_{op}_{t}", "U_" + op, t, t))
    for op in ["ISINF", "ISNAN", "ISFINITE"]:
        unops.append((f"GxB_{op}_{t}", "U_" + op, t, "BOOL"))
# positional unary operators (round 6; pygraphblas/unaryop.py:55-63 lists them): the result is the entry's row / column index (0- or 1-based), whatever the input holds
for t in ["INT32", "INT64"]:
    for op in ["POSITIONI", "POSITIONI1", "POSITIONJ", "POSITIONJ1"]:
        unops.append((f"GxB_{op}_{t}", "U_" + op, t, t))

# ---- binary ops ----------------------------------------------------------------------------
for t in REAL:
    for op in ["FIRST", "SECOND", "MIN", "MAX", "PLUS", "MINUS", "TIMES", "DIV"]:
        add_binop(f"GrB_{op}_{t}", "B_" + op, t, t, t)
    for op in ["EQ", "NE", "GT", "LT", "GE", "LE"]:
        add_binop(f"GrB_{op}_{t}", "B_" + op, t, t, "BOOL")
    for op in ["PAIR", "ANY", "RMINUS", "RDIV", "POW", "ISEQ", "ISNE", "ISGT", "ISLT", "ISGE", "ISLE",
               "LOR", "LAND", "LXOR"]:
        add_binop(f"GxB_{op}_{t}", "B_" + op, t, t, t)
for op in ["LOR", "LAND", "LXOR", "LXNOR"]:
    add_binop(f"GrB_{op}", "B_" + op, "BOOL", "BOOL", "BOOL")
_bin_by_key[("B_LXNOR", "BOOL")] = "GrB_LXNOR"
for t in INTS:
    for op in ["BOR", "BAND", "BXOR", "BXNOR"]:
        add_binop(f"GrB_{op}_{t}", "B_" + op, t, t, t)
    for op in ["BGET", "BSET", "BCLR"]:
        add_binop(f"GxB_{op}_{t}", "B_" + op, t, t, t)
for t in FLOATS:
    for op in ["ATAN2", "HYPOT", "FMOD", "REMAINDER", "COPYSIGN", "LDEXP"]:
        add_binop(f"GxB_{op}_{t}", "B_" + op, t, t, t)


def bin_of(op, t):
    return _bin_by_key[("B_" + op, t)]


# ---- monoids -------------------------------------------------------------------------------
def add_monoid(cname, op, t):
    monoids.append((cname, bin_of(op, t)))
    _mon_by_key.setdefault((op, t), cname)


for t in NUM:
    for op in ["MIN", "MAX", "PLUS", "TIMES"]:
        add_monoid(f"GrB_{op}_MONOID_{t}", op, t)
        add_monoid(f"GxB_{op}_{t}_MONOID", op, t)
    add_monoid(f"GxB_ANY_{t}_MONOID", "ANY", t)
for op in ["LOR", "LAND", "LXOR", "LXNOR"]:
    add_monoid(f"GrB_{op}_MONOID_BOOL", op, "BOOL")
for op in ["ANY", "LOR", "LAND", "LXOR"]:
    add_monoid(f"GxB_{op}_BOOL_MONOID", op, "BOOL")
monoids.append(("GxB_EQ_BOOL_MONOID", "GrB_LXNOR"))
_mon_by_key[("EQ", "BOOL")] = "GxB_EQ_BOOL_MONOID"
for t in UINTS:
    for op in ["BOR", "BAND", "BXOR", "BXNOR"]:
        add_monoid(f"GxB_{op}_{t}_MONOID", op, t)


def mon_of(op, t):
    return _mon_by_key[(op, t)]


# ---- semirings: same-type multiply first; the comparison-multiply ones (a BOOL monoid over GrB_<cmp>_<T>) follow the _BOOL column ---------
MULS = ["FIRST", "SECOND", "PAIR", "MIN", "MAX", "PLUS", "MINUS", "RMINUS", "TIMES", "DIV", "RDIV",
        "ISEQ", "ISNE", "ISGT", "ISLT", "ISGE", "ISLE", "LOR", "LAND", "LXOR"]
for t in NUM:
    for add in ["MIN", "MAX", "PLUS", "TIMES", "ANY"]:
        for mul in MULS:
            semirings.append((f"GxB_{add}_{mul}_{t}", mon_of(add, t), bin_of(mul, t)))
    for add, mul in [("PLUS", "TIMES"), ("PLUS", "MIN"), ("MIN", "PLUS"), ("MIN", "TIMES"), ("MIN", "FIRST"),
                     ("MIN", "SECOND"), ("MIN", "MAX"), ("MAX", "PLUS"), ("MAX", "TIMES"), ("MAX", "FIRST"),
                     ("MAX", "SECOND"), ("MAX", "MIN")]:
        semirings.append((f"GrB_{add}_{mul}_SEMIRING_{t}", mon_of(add, t), bin_of(mul, t)))
BOOL_MULS = ["FIRST", "SECOND", "PAIR", "LOR", "LAND", "LXOR", "EQ", "GT", "LT", "GE", "LE"]
for add in ["LOR", "LAND", "LXOR", "EQ", "ANY"]:
    for mul in BOOL_MULS:
        semirings.append((f"GxB_{add}_{mul}_BOOL", mon_of(add, "BOOL"), bin_of(mul, "BOOL")))
for add, mul in [("LOR", "LAND"), ("LAND", "LOR"), ("LXOR", "LAND")]:
    semirings.append((f"GrB_{add}_{mul}_SEMIRING_BOOL", mon_of(add, "BOOL"), bin_of(mul, "BOOL")))
semirings.append(("GrB_LXNOR_LOR_SEMIRING_BOOL", "GrB_LXNOR_MONOID_BOOL", "GrB_LOR"))
# comparison semirings (pygraphblas/semiring.py:87-121, `boolean_re`): a BOOL monoid over the comparison GrB_<cmp>_<T> of a non-Boolean type — T x T -> BOOL.  They run
# in mxm / mxv / vxm through the kernels of grb_cmpsr.hip; the _BOOL column above stays on the operator table
for t in NUM:
    for add in ["LOR", "LAND", "LXOR", "EQ", "ANY"]:
        for mul in ["EQ", "NE", "GT", "LT", "GE", "LE"]:
            semirings.append((f"GxB_{add}_{mul}_{t}", mon_of(add, "BOOL"), bin_of(mul, t)))
# positional semirings (pygraphblas/semiring.py:87-93 names their multipliers): the product term's coordinate in INT32 / INT64, whatever the operands hold.  Their
# multipliers are INTERNAL binary operators — objects that GxB_Semiring_multiply returns and the printers name, with no exported handle: nothing but mxm / mxv /
# vxm runs them, and the exported binary-operator set is the one tests/operator_model.py mirrors
POSITIONAL = ["FIRSTI", "FIRSTI1", "FIRSTJ", "FIRSTJ1", "SECONDI", "SECONDI1", "SECONDJ", "SECONDJ1"]
posops = []  # (cname, opcode, type): defined in the registry, absent from the header
for t in ["INT32", "INT64"]:
    for mul in POSITIONAL:
        posops.append((f"GxB_{mul}_{t}", "B_" + mul, t))
    for add in ["MIN", "MAX", "ANY", "PLUS", "TIMES"]:
        for mul in POSITIONAL:
            semirings.append((f"GxB_{add}_{mul}_{t}", mon_of(add, t), f"GxB_{mul}_{t}"))

# ---- descriptors ---------------------------------------------------------------------------
descs = []
for r in ["", "R"]:
    for s in ["", "S"]:
        for c in ["", "C"]:
            for tt in ["", "T0", "T1", "T0T1"]:
                nm = r + s + c + tt
                if nm:
                    descs.append(nm)
assert len(descs) == 31

selectops = ["TRIL", "TRIU", "DIAG", "OFFDIAG", "NONZERO", "EQ_ZERO", "GT_ZERO", "GE_ZERO", "LT_ZERO", "LE_ZERO",
             "NE_THUNK", "EQ_THUNK", "GT_THUNK", "GE_THUNK", "LT_THUNK", "LE_THUNK"]

# ============================================================================================
# registry_gen.inc
# ============================================================================================
inc = ["// GENERATED by tools/gen_api.py — do not edit.\n"]
for cname, code in types:
    inc.append(f'static GrB_Type_opaque ty_{cname} = {{GRB_MAGIC, grb::{code}, 0, "{cname}"}};\n'
               f'extern "C" GrB_Type {cname} = &ty_{cname};\n')


def ty(t):
    return "&ty_GrB_" + t


for cname, op, x, z in unops:
    inc.append(f'static GrB_UnaryOp_opaque uo_{cname} = {{GRB_MAGIC, grb::{op}, {ty(x)}, {ty(z)}, "{cname}", nullptr}};\n'
               f'extern "C" GrB_UnaryOp {cname} = &uo_{cname};\n')
for cname, op, x, y, z in binops:
    inc.append(f'static GrB_BinaryOp_opaque bo_{cname} = {{GRB_MAGIC, grb::{op}, {ty(x)}, {ty(y)}, {ty(z)}, "{cname}", nullptr}};\n'
               f'extern "C" GrB_BinaryOp {cname} = &bo_{cname};\n')
for cname, op, t in posops:      # (no extern "C" handle)
    inc.append(f'static GrB_BinaryOp_opaque bo_{cname} = {{GRB_MAGIC, grb::{op}, {ty(t)}, {ty(t)}, {ty(t)}, "{cname}", nullptr}};\n')
for cname, b in monoids:
    inc.append(f'static GrB_Monoid_opaque mo_{cname} = {{GRB_MAGIC, &bo_{b}, {{0}}, false, {{0}}, "{cname}", true}};\n'
               f'extern "C" GrB_Monoid {cname} = &mo_{cname};\n')
for cname, m, b in semirings:
    inc.append(f'static GrB_Semiring_opaque sr_{cname} = {{GRB_MAGIC, &mo_{m}, &bo_{b}, "{cname}", true}};\n'
               f'extern "C" GrB_Semiring {cname} = &sr_{cname};\n')
for nm in descs:
    outp = "GrB_REPLACE" if "R" in nm.replace("T0", "").replace("T1", "") else "GxB_DEFAULT"
    core = nm.replace("T0", "").replace("T1", "")
    mask = ("GrB_STRUCTURE" if "S" in core else "0") + " + " + ("GrB_COMP" if "C" in core else "0")
    inp0 = "GrB_TRAN" if "T0" in nm else "GxB_DEFAULT"
    inp1 = "GrB_TRAN" if "T1" in nm else "GxB_DEFAULT"
    inc.append(f'static GrB_Descriptor_opaque de_{nm} = {{GRB_MAGIC, {outp}, {mask}, {inp0}, {inp1}, 0, 0, 0, 0.0, true, "{nm}"}};\n'
               f'extern "C" GrB_Descriptor GrB_DESC_{nm} = &de_{nm};\n')
for i, nm in enumerate(selectops):
    inc.append(f'static GxB_SelectOp_opaque so_{nm} = {{GRB_MAGIC, SEL_{nm}, "GxB_{nm}", nullptr, nullptr, nullptr}};\n'
               f'extern "C" GxB_SelectOp GxB_{nm} = &so_{nm};\n')
inc.append("static GrB_Type_opaque* const all_types[] = {" + ", ".join(f"&ty_{c}" for c, _ in types) + "};\n")
inc.append("static GrB_Monoid_opaque* const all_monoids[] = {" + ", ".join(f"&mo_{c}" for c, _ in monoids) + "};\n")
inc.append("static GrB_BinaryOp_opaque* const all_binops[] = {" + ", ".join(f"&bo_{c[0]}" for c in binops) + "};\n")
inc.append("static GrB_UnaryOp_opaque* const all_unops[] = {" + ", ".join(f"&uo_{c[0]}" for c in unops) + "};\n")
inc.append("static GrB_Semiring_opaque* const all_semirings[] = {" + ", ".join(f"&sr_{c[0]}" for c in semirings) + "};\n")
with open(os.path.join(ROOT, "pygraphblas_amd/csrc/registry_gen.inc"), "w") as f:
    f.write("".join(inc))

# ============================================================================================
# include/grb_mi355x.h
# ============================================================================================
H = []
H.append("""/* grb_mi355x.h — C ABI of libgrb_mi355x.so, an MI355X (gfx950) GraphBLAS hot-path backend.
 *
 * GENERATED by tools/gen_api.py.  The file is deliberately plain C declarations without
 * preprocessor logic so that a CFFI `ffi.cdef()` can consume it verbatim (shim/).
 *
 * What each group replaces in the reference (Graphegon/pygraphblas, files under /root/reference):
 *   GrB_mxm   <- lib.GrB_mxm   called at pygraphblas/matrix.py:2572-2583   (Matrix.mxm)
 *   GrB_mxv   <- lib.GrB_mxv   called at pygraphblas/matrix.py:2714-2725   (Matrix.mxv)
 *   GrB_vxm   <- lib.GrB_vxm   called at pygraphblas/vector.py:960-970     (Vector.vxm)
 *   GrB_Matrix_reduce_<T> <- pygraphblas/matrix.py:1799-1803 (Matrix.reduce_int et al.)
 *   GrB_Vector_reduce_<T> <- pygraphblas/vector.py:1132-1202
 *   object model (new, free, build, setElement, extractElement, extractTuples, nvals, ...) <- the `lib.` calls listed by
 *       grep -oh "lib\\.G[rx]B_[A-Za-z0-9_]*" pygraphblas/*.py  (SURVEY.md §8b)
 *   error convention: positive GrB_Info codes 0..13 as mapped at pygraphblas/base.py:189-203.
 * Signatures are GraphBLAS C API 1.3 with SuiteSparse v5.1-era GxB_ extensions.
 * GrBX_* functions are extensions of this backend (bulk/device import-export, timing).
 */
typedef uint64_t GrB_Index;
typedef int GrB_Info;
typedef int GrB_Mode;
typedef int GrB_Desc_Field;
typedef int GrB_Desc_Value;
typedef int GxB_Option_Field;
typedef int GxB_Format_Value;
typedef void (*GxB_unary_function)(void *, const void *);
typedef void (*GxB_binary_function)(void *, const void *, const void *);
typedef bool (*GxB_select_function)(GrB_Index i, GrB_Index j, const void *x, const void *thunk);
typedef struct GrB_Type_opaque *GrB_Type;
typedef struct GrB_UnaryOp_opaque *GrB_UnaryOp;
typedef struct GrB_BinaryOp_opaque *GrB_BinaryOp;
typedef struct GrB_Monoid_opaque *GrB_Monoid;
typedef struct GrB_Semiring_opaque *GrB_Semiring;
typedef struct GrB_Descriptor_opaque *GrB_Descriptor;
typedef struct GxB_SelectOp_opaque *GxB_SelectOp;
typedef struct GxB_Scalar_opaque *GxB_Scalar;
typedef struct GrB_Vector_opaque *GrB_Vector;
typedef struct GrB_Matrix_opaque *GrB_Matrix;

/* GrB_Info values */
#define GrB_SUCCESS 0
#define GrB_NO_VALUE 1
#define GrB_UNINITIALIZED_OBJECT 2
#define GrB_INVALID_OBJECT 3
#define GrB_NULL_POINTER 4
#define GrB_INVALID_VALUE 5
#define GrB_INVALID_INDEX 6
#define GrB_DOMAIN_MISMATCH 7
#define GrB_DIMENSION_MISMATCH 8
#define GrB_OUTPUT_NOT_EMPTY 9
#define GrB_OUT_OF_MEMORY 10
#define GrB_INSUFFICIENT_SPACE 11
#define GrB_INDEX_OUT_OF_BOUNDS 12
#define GrB_PANIC 13
/* modes */
#define GrB_NONBLOCKING 0
#define GrB_BLOCKING 1
/* descriptor fields and values */
#define GrB_OUTP 0
#define GrB_MASK 1
#define GrB_INP0 2
#define GrB_INP1 3
#define GxB_DESCRIPTOR_NTHREADS 5
#define GxB_DESCRIPTOR_CHUNK 7
#define GxB_AxB_METHOD 1000
#define GxB_SORT 35
#define GxB_DEFAULT 0
#define GrB_REPLACE 1
#define GrB_COMP 2
#define GrB_TRAN 3
#define GrB_STRUCTURE 4
#define GxB_AxB_GUSTAVSON 1001
#define GxB_AxB_DOT 1003
#define GxB_AxB_HASH 1004
#define GxB_AxB_SAXPY 1005
/* options */
#define GxB_HYPER_SWITCH 0
#define GxB_BITMAP_SWITCH 34
#define GxB_FORMAT 1
#define GxB_GLOBAL_NTHREADS 5
#define GxB_GLOBAL_CHUNK 7
#define GxB_BURBLE 99
#define GxB_SPARSITY_STATUS 33
#define GxB_SPARSITY_CONTROL 32
#define GxB_BY_ROW 0
#define GxB_BY_COL 1
#define GxB_HYPERSPARSE 1
#define GxB_SPARSE 2
#define GxB_BITMAP 4
#define GxB_FULL 8
#define GxB_AUTO_SPARSITY 15
#define GxB_RANGE 9223372036854775807
#define GxB_STRIDE 9223372036854775806
#define GxB_BACKWARDS 9223372036854775805
#define GxB_BEGIN 0
#define GxB_END 1
#define GxB_INC 2
#define GxB_INDEX_MAX 1152921504606846976
#define GxB_IMPLEMENTATION_MAJOR 0
#define GxB_IMPLEMENTATION_MINOR 1
#define GxB_IMPLEMENTATION_SUB 0
#define GxB_SPEC_MAJOR 1
#define GxB_SPEC_MINOR 3
#define GxB_SPEC_SUB 0

extern const uint64_t *GrB_ALL;

""")
H.append("/* ---- built-in types ---- */\n")
for cname, _ in types:
    H.append(f"extern GrB_Type {cname};\n")
H.append("/* ---- built-in unary operators ---- */\n")
for c in unops:
    H.append(f"extern GrB_UnaryOp {c[0]};\n")
H.append("/* ---- built-in binary operators ---- */\n")
for c in binops:
    H.append(f"extern GrB_BinaryOp {c[0]};\n")
H.append("/* ---- built-in monoids ---- */\n")
for c in monoids:
    H.append(f"extern GrB_Monoid {c[0]};\n")
H.append("/* ---- built-in semirings ---- */\n")
for c in semirings:
    H.append(f"extern GrB_Semiring {c[0]};\n")
H.append("/* ---- predefined descriptors ---- */\n")
for nm in descs:
    H.append(f"extern GrB_Descriptor GrB_DESC_{nm};\n")
H.append("/* ---- select operators ---- */\n")
for nm in selectops:
    H.append(f"extern GxB_SelectOp GxB_{nm};\n")

H.append("""
/* ---- context ---- */
GrB_Info GrB_init(int mode);
GrB_Info GxB_init(int mode, void *(*user_malloc)(size_t), void *(*user_calloc)(size_t, size_t),
                  void *(*user_realloc)(void *, size_t), void (*user_free)(void *), bool user_malloc_is_thread_safe);
GrB_Info GrB_finalize(void);
GrB_Info GrB_getVersion(unsigned int *version, unsigned int *subversion);
GrB_Info GxB_Global_Option_set(int field, ...);
GrB_Info GxB_Global_Option_get(int field, ...);

/* ---- introspection of operator objects ---- */
GrB_Info GxB_Semiring_add(GrB_Monoid *add, GrB_Semiring semiring);
GrB_Info GxB_Semiring_multiply(GrB_BinaryOp *multiply, GrB_Semiring semiring);
GrB_Info GxB_Monoid_operator(GrB_BinaryOp *op, GrB_Monoid monoid);
GrB_Info GxB_BinaryOp_ztype(GrB_Type *ztype, GrB_BinaryOp op);
GrB_Info GxB_BinaryOp_xtype(GrB_Type *xtype, GrB_BinaryOp op);
GrB_Info GxB_BinaryOp_ytype(GrB_Type *ytype, GrB_BinaryOp op);
GrB_Info GxB_UnaryOp_ztype(GrB_Type *ztype, GrB_UnaryOp op);
GrB_Info GxB_UnaryOp_xtype(GrB_Type *xtype, GrB_UnaryOp op);
GrB_Info GxB_Type_size(size_t *size, GrB_Type type);
GrB_Info GxB_Semiring_fprint(GrB_Semiring semiring, const char *name, int pr, FILE *f);
GrB_Info GxB_Monoid_fprint(GrB_Monoid monoid, const char *name, int pr, FILE *f);
GrB_Info GxB_BinaryOp_fprint(GrB_BinaryOp op, const char *name, int pr, FILE *f);
GrB_Info GxB_UnaryOp_fprint(GrB_UnaryOp op, const char *name, int pr, FILE *f);
GrB_Info GxB_SelectOp_fprint(GxB_SelectOp op, const char *name, int pr, FILE *f);
GrB_Info GxB_Matrix_fprint(GrB_Matrix A, const char *name, int pr, FILE *f);
GrB_Info GxB_Vector_fprint(GrB_Vector v, const char *name, int pr, FILE *f);

/* ---- descriptors ---- */
GrB_Info GrB_Descriptor_new(GrB_Descriptor *descriptor);
GrB_Info GrB_Descriptor_set(GrB_Descriptor desc, int field, int val);
GrB_Info GxB_Desc_get(GrB_Descriptor desc, int field, ...);
GrB_Info GxB_Desc_set(GrB_Descriptor desc, int field, ...);
GrB_Info GrB_Descriptor_free(GrB_Descriptor *descriptor);

/* ---- user-defined algebra made of built-in operators ---- */
GrB_Info GrB_Semiring_new(GrB_Semiring *semiring, GrB_Monoid add, GrB_BinaryOp multiply);
GrB_Info GrB_Semiring_free(GrB_Semiring *semiring);
GrB_Info GrB_Monoid_free(GrB_Monoid *monoid);

/* ---- user-defined unary / binary operators, handed over as C source and compiled for the device at first use (grb_userop.cpp) ----
 * `defn` is the C definition of the function `name`, in SuiteSparse 7's form: "void NAME (T *z, const T *x) { ... }" or
 * "void NAME (T *z, const T *x, const T *y) { ... }", T the C type of the GraphBLAS type; helper functions may precede it in the same string.
 * `fn` (a host function pointer) is never called and may be NULL.  All of the operator's types must be ONE of the 11 real built-in types
 * (GrB_DOMAIN_MISMATCH otherwise).  Such an operator runs in GrB_*_apply, GxB_*_apply_BinaryOp1st / 2nd, GrB_*_eWiseAdd_BinaryOp and
 * GrB_*_eWiseMult_BinaryOp on containers with an HBM layout; every other use returns GrB_DOMAIN_MISMATCH.  The function-pointer forms
 * GrB_UnaryOp_new / GrB_BinaryOp_new and GrB_Type_new do not exist (DESIGN.md section 8).
 * A user-defined select operator is the same for GxB_Matrix_select / GxB_Vector_select: `defn` defines the predicate
 * "bool NAME (GrB_Index i, GrB_Index j, const X *x, const K *thunk) { ... }", X the C type of `xtype`, K of `ttype` (NULL: the same as `xtype`), both one of
 * the 11 real built-in types; an entry is kept where it returns true (a vector's entry: i its position, j 0). */
GrB_Info GxB_UnaryOp_new(GrB_UnaryOp *unaryop, void *function, GrB_Type ztype, GrB_Type xtype, const char *name, const char *defn);
GrB_Info GxB_BinaryOp_new(GrB_BinaryOp *binaryop, void *function, GrB_Type ztype, GrB_Type xtype, GrB_Type ytype, const char *name, const char *defn);
GrB_Info GrB_UnaryOp_free(GrB_UnaryOp *unaryop);     /* releases a user-defined operator and sets the variable to NULL; built-in handles are left alone */
GrB_Info GrB_BinaryOp_free(GrB_BinaryOp *binaryop);
GrB_Info GxB_SelectOp_new(GxB_SelectOp *selectop, void *function, GrB_Type xtype, GrB_Type ttype, const char *name, const char *defn);
GrB_Info GxB_SelectOp_free(GxB_SelectOp *selectop);  /* releases a user-defined select operator and sets the variable to NULL; the built-in GxB_TRIL ... are left alone */
GrB_Info GrBX_userop_stats(uint64_t *compiled, uint64_t *loaded_from_disk, uint64_t *launched); /* user-operator kernels compiled with hipRTC, loaded from the code-object cache on disk instead, and launches through them */
GrB_Info GrBX_userop_source(const char *name, const char *defn, GrB_Type type, int kind, char *buf, size_t len); /* the kernel text compiled for such an operator in an operation of `kind` (0 apply, 1 bind1st, 2 bind2nd, 3 eadd, 4 emult) */
GrB_Info GrBX_selectop_source(const char *name, const char *defn, GrB_Type xtype, GrB_Type ttype, int on_vector, char *buf, size_t len); /* the kernel text compiled for a select operator used on a matrix (on_vector 0) or a vector (1) */
/* User-defined monoids and semirings.  GrB_Monoid_new_<T> / GrB_Semiring_new refuse a user-defined operator; these two make the objects that GrB_mxm, GrB_mxv,
 * GrB_vxm and GrB_Matrix_reduce_Monoid run through compiled kernels.  `op` / `mul`: a user-defined binary operator or one of the built-ins FIRST, SECOND, PAIR, PLUS,
 * MINUS, TIMES, MIN, MAX (LOR / LAND / LXOR on BOOL); `add`: a monoid made here or a built-in monoid of one of those operators; `identity`: one value of op's type.
 * All types are ONE of the 11 real built-in types.  The identity is never combined into a result; mxv and mxm call mul(A(i,k), B(k,j)), vxm calls mul(u(i), A(i,j)).
 * The objects keep pointers to their operators, have no terminal value and are released by GrB_Monoid_free / GrB_Semiring_free (DESIGN.md section 8). */
GrB_Info GrBX_Monoid_new_user(GrB_Monoid *monoid, GrB_BinaryOp op, const void *identity);
GrB_Info GrBX_Semiring_new_user(GrB_Semiring *semiring, GrB_Monoid add, GrB_BinaryOp mul);
GrB_Info GrBX_usersr_source(GrB_Monoid add, GrB_BinaryOp mul, int kind, char *buf, size_t len); /* the kernel text compiled for them in an operation of `kind` (0 mxv, 1 vxm, 2 mxm, 3 reduce_rows: mul may be NULL) */
GrB_Info GxB_Monoid_identity(void *identity, GrB_Monoid monoid);
GrB_Info GxB_Monoid_terminal(bool *has_terminal, void *terminal, GrB_Monoid monoid);
GrB_Info GrBX_Matrix_residency(const GrB_Matrix A, int *where);   /* which images of the container are valid: bit 0 the host mirror, bit 1 the HBM image (a look: nothing is moved, no deferred work completed) */
GrB_Info GrBX_Vector_residency(const GrB_Vector v, int *where);
GrB_Info GrBX_last_error(char *buf, int len);        /* the message of the calling thread's most recent failure (for calls that have no container to ask: GxB_*Op_new, GrB_Monoid_new_*, GrB_Semiring_new) */

/* ---- matrices ---- */
GrB_Info GrB_Matrix_new(GrB_Matrix *A, GrB_Type type, GrB_Index nrows, GrB_Index ncols);
GrB_Info GrB_Matrix_dup(GrB_Matrix *C, const GrB_Matrix A);
GrB_Info GrB_Matrix_clear(GrB_Matrix A);
GrB_Info GrB_Matrix_free(GrB_Matrix *A);
GrB_Info GrB_Matrix_nrows(GrB_Index *nrows, const GrB_Matrix A);
GrB_Info GrB_Matrix_ncols(GrB_Index *ncols, const GrB_Matrix A);
GrB_Info GrB_Matrix_nvals(GrB_Index *nvals, const GrB_Matrix A);
GrB_Info GrB_Matrix_wait(GrB_Matrix *A);
GrB_Info GrB_Matrix_error(const char **error, const GrB_Matrix A);
GrB_Info GrB_Matrix_resize(GrB_Matrix A, GrB_Index nrows_new, GrB_Index ncols_new);
GrB_Info GrB_Matrix_removeElement(GrB_Matrix C, GrB_Index i, GrB_Index j);
GrB_Info GxB_Matrix_type(GrB_Type *type, const GrB_Matrix A);
GrB_Info GxB_Matrix_Option_set(GrB_Matrix A, int field, ...);
GrB_Info GxB_Matrix_Option_get(GrB_Matrix A, int field, ...);
GrB_Info GxB_Matrix_memoryUsage(size_t *size, const GrB_Matrix A);

/* ---- vectors ---- */
GrB_Info GrB_Vector_new(GrB_Vector *v, GrB_Type type, GrB_Index n);
GrB_Info GrB_Vector_dup(GrB_Vector *w, const GrB_Vector u);
GrB_Info GrB_Vector_clear(GrB_Vector v);
GrB_Info GrB_Vector_free(GrB_Vector *v);
GrB_Info GrB_Vector_size(GrB_Index *n, const GrB_Vector v);
GrB_Info GrB_Vector_nvals(GrB_Index *nvals, const GrB_Vector v);
GrB_Info GrB_Vector_wait(GrB_Vector *v);
GrB_Info GrB_Vector_error(const char **error, const GrB_Vector v);
GrB_Info GrB_Vector_resize(GrB_Vector v, GrB_Index n_new);
GrB_Info GrB_Vector_removeElement(GrB_Vector v, GrB_Index i);
GrB_Info GxB_Vector_type(GrB_Type *type, const GrB_Vector v);
GrB_Info GxB_Vector_Option_set(GrB_Vector v, int field, ...);
GrB_Info GxB_Vector_Option_get(GrB_Vector v, int field, ...);
GrB_Info GxB_Vector_memoryUsage(size_t *size, const GrB_Vector v);

/* ---- scalars ---- */
GrB_Info GxB_Scalar_new(GxB_Scalar *s, GrB_Type type);
GrB_Info GxB_Scalar_dup(GxB_Scalar *s, const GxB_Scalar t);
GrB_Info GxB_Scalar_clear(GxB_Scalar s);
GrB_Info GxB_Scalar_free(GxB_Scalar *s);
GrB_Info GxB_Scalar_nvals(GrB_Index *nvals, const GxB_Scalar s);
GrB_Info GxB_Scalar_wait(GxB_Scalar *s);
GrB_Info GxB_Scalar_type(GrB_Type *type, const GxB_Scalar s);

/* ==== THE HOT PATH (HIP kernels; fail with GrB_PANIC when no gfx950 device is present) ==== */
GrB_Info GrB_mxm(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Semiring semiring,
                 const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);
GrB_Info GrB_mxv(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Semiring semiring,
                 const GrB_Matrix A, const GrB_Vector u, const GrB_Descriptor desc);
GrB_Info GrB_vxm(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Semiring semiring,
                 const GrB_Vector u, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_reduce_Monoid(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                 const GrB_Monoid monoid, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GrB_transpose(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A,
                 const GrB_Descriptor desc);

/* ---- O(n) / O(nnz) companions of the hot path ("next" rows of SURVEY.md §8f) ---- */
GrB_Info GrB_Vector_eWiseAdd_BinaryOp(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                 const GrB_BinaryOp op, const GrB_Vector u, const GrB_Vector v, const GrB_Descriptor desc);
GrB_Info GrB_Vector_eWiseAdd_Monoid(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                 const GrB_Monoid op, const GrB_Vector u, const GrB_Vector v, const GrB_Descriptor desc);
GrB_Info GrB_Vector_eWiseAdd_Semiring(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                 const GrB_Semiring op, const GrB_Vector u, const GrB_Vector v, const GrB_Descriptor desc);
GrB_Info GrB_Vector_eWiseMult_BinaryOp(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                 const GrB_BinaryOp op, const GrB_Vector u, const GrB_Vector v, const GrB_Descriptor desc);
GrB_Info GrB_Vector_eWiseMult_Monoid(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                 const GrB_Monoid op, const GrB_Vector u, const GrB_Vector v, const GrB_Descriptor desc);
GrB_Info GrB_Vector_eWiseMult_Semiring(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum,
                 const GrB_Semiring op, const GrB_Vector u, const GrB_Vector v, const GrB_Descriptor desc);
GrB_Info GrB_Vector_apply(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_UnaryOp op,
                 const GrB_Vector u, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_eWiseAdd_BinaryOp(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                 const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_eWiseAdd_Monoid(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                 const GrB_Monoid op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_eWiseAdd_Semiring(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                 const GrB_Semiring op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_eWiseMult_BinaryOp(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                 const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_eWiseMult_Monoid(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                 const GrB_Monoid op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_eWiseMult_Semiring(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum,
                 const GrB_Semiring op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_apply(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_UnaryOp op,
                 const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GxB_Matrix_select(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GxB_SelectOp op,
                 const GrB_Matrix A, const GxB_Scalar Thunk, const GrB_Descriptor desc);
GrB_Info GxB_Vector_select(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GxB_SelectOp op,
                 const GrB_Vector u, const GxB_Scalar Thunk, const GrB_Descriptor desc);

/* ---- backend extensions: bulk / device-resident import-export, timing, stream ---- */
/* location: 0 = host pointers, 1 = device (HBM) pointers.  Arrays are copied. */
GrB_Info GrBX_Matrix_import_CSR(GrB_Matrix *A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, GrB_Index nvals,
                 const uint32_t *rowptr, const uint32_t *colidx, const void *values, int location);
GrB_Info GrBX_Matrix_export_CSR(const GrB_Matrix A, uint32_t *rowptr, uint32_t *colidx, void *values, int location);
GrB_Info GrBX_Vector_import_Full(GrB_Vector *v, GrB_Type type, GrB_Index n, const void *values, int location);
/* present[i] != 0 means "position i holds an entry": ANY non-zero byte, not only 1.  The bytes are copied as they are (NULL: every position
   holds an entry); every operation, nvals included, reads them by that rule, and export_Bitmap hands back 1 for an entry the library wrote and
   the caller's own byte for an entry it never touched. */
GrB_Info GrBX_Vector_import_Bitmap(GrB_Vector *v, GrB_Type type, GrB_Index n, const void *values,
                 const uint8_t *present, int location);
GrB_Info GrBX_Vector_export_Bitmap(const GrB_Vector v, void *values, uint8_t *present, int location);
/* raw HBM addresses of a vector's value / presence arrays (valid until the vector is next written) */
GrB_Info GrBX_Vector_device_view(GrB_Vector v, void **values, uint8_t **present, GrB_Index *nvals);
GrB_Info GrBX_Vector_device_touch(GrB_Vector v);   /* caller wrote through the device view: recount entries */
GrB_Info GrBX_set_stream(void *hip_stream);        /* all kernels are launched on this HIP stream (default: 0) */
GrB_Info GrBX_device_synchronize(void);
GrB_Info GrBX_timer_start(void);                   /* hipEventRecord on the library stream */
GrB_Info GrBX_timer_stop(float *milliseconds);     /* hipEventRecord + synchronize + elapsed */
GrB_Info GrBX_device_info(char *name, int name_len, int *compute_units, size_t *hbm_bytes);
GrB_Info GrBX_memory_in_use(size_t *bytes);
GrB_Info GrBX_last_kernel_plan(char *buf, int len); /* which kernels the last hot-path call launched; the device route of an index-list extract leaves "extract_matrix<cols=all|range|table|bisect,rowsort=0|1,transpose=0|1> ...", "extract_col<...>" or "extract_vector<...>", that of an index-list assign "assign_matrix<rows=..,cols=..,rowsort=0|1,transpose=0|1,accum=..> ...", "assign_row<...>", "assign_col<...>" or "assign_vector<index=..,accum=..>", that of a Kronecker product "kronecker<op=..,transpose0=0|1,transpose1=0|1,accum=..> k_kron_rowptr k_kron_fill" */
GrB_Info GrBX_last_plan_build_ms(float *milliseconds); /* device time of the most recent SpMV plan build (kernel X), 0 if none */
/* A read-only view of the kernel-X plan a matrix carries (transposed 0: the plan of the by-row image, what GrB_mxv multiplies with; 1: of the cached transpose, GrB_vxm).
   Neither call builds or changes a plan; GrB_NO_VALUE when there is none.  facts: out[0] H (slots of an LDS table), [1] HOT (columns a table serves), [2] S, [3] NP,
   [4] NS (streams), [5] own, [6] F (sub-rows), [7] ncold (entries whose column no table serves), [8] vbytes, [9] has_vals, [10] m_ok, [11] m_wide, [12] m_nblocks,
   [13] m_slots, [14] WP_ENT, [15] WP_CHUNK, [16] XM_ROWS, [17] XM_TARGET, [18] XM_SLOTS, [19] bytes of the value type, [20] tiles of all streams, [21] 1 = 16-bit column
   plane, 0 = 32-bit words, [22] XP_RB (rows per block of the fallback merge), [23] 1 = lane-per-piece layout; then per stream k at [24 + 4 k]: ne, ntiles, nhot,
   tiles_per_chunk.  nout >= 24 + 4 NS (280 always suffices), else GrB_INVALID_VALUE.  tiles: two words per tile in stream order, {sub-row of the tile's first entry,
   index of its first cold entry among the cold entries of all tiles} (tinfo; with 32-bit words trow and the cold flags counted); ntiles must be out[20].  bstart (may be
   NULL; written when m_ok): the first row of every merge block, nbstart = m_nblocks + 1. */
GrB_Info GrBX_Matrix_xcd_plan_facts(const GrB_Matrix A, int transposed, uint64_t *out, GrB_Index nout);
GrB_Info GrBX_Matrix_xcd_plan_tiles(const GrB_Matrix A, int transposed, uint32_t *tiles, GrB_Index ntiles, uint32_t *bstart, GrB_Index nbstart);
GrB_Info GrBX_lazy_stats(uint64_t *chains, uint64_t *nodes, uint64_t *fills_folded, uint64_t *reduces_fused); /* non-blocking mode: element-wise chain kernels run, operations they carried, `w(:) = s` fills folded into a product's store, reductions fused into a chain */
GrB_Info GrBX_chain_jit_stats(uint64_t *compiled, uint64_t *launched); /* deferred element-wise chains compiled with hipRTC (grb_chain_jit.cpp): kernels compiled, launches through them */
GrB_Info GrBX_chain_jit_stats2(uint64_t *compiled, uint64_t *launched, uint64_t *loaded_from_disk); /* ... and the kernels whose code object came from the disk cache (GRB_MI355X_CACHE_DIR) instead of a compilation */
GrB_Info GrBX_exact_sum_host(const double *terms, uint64_t n, int significand_bits, double *sum, int *unit_exp_out); /* the 128-bit integer accumulation of the masked product's deterministic mode (grb_exact.hpp) run on the host over `terms`: the exact sum rounded once to 53 / 24 bits */
GrB_Info GrBX_Vector_iseq(bool *equal, const GrB_Vector u, const GrB_Vector v); /* same size, pattern and values of two vectors of one built-in real type in ONE pass (pygraphblas/vector.py:188-235 Vector.iseq composes it from five calls); GrB_NO_VALUE when that is not the case at hand (types differ, complex, hypersparse): compose it then */
GrB_Info GrBX_xcd_mapping(char *buf, int len);      /* how workgroups of a full-chip launch map to XCDs ("roundrobin8", or what was observed) */
/* The exchange steps of the row-partitioned path (one process per GPU; RCCL over xGMI; grb_dist.cpp).  The reference has no
 * distributed code: these replace nothing in it, they are what BASELINE.json's north star adds (SURVEY.md section 8e). */
/* Index-list extract / assign, kronecker and apply with a GxB_Scalar operand: the element-wise container surface (grb_extract_ops.cpp, grb_assign_ops.cpp, grb_kron_ops.cpp, grb_apply_scalar.cpp).
 * Small host-resident containers are computed on the host mirror like setElement; extract, assign and kronecker run in HBM
 * (grb_extract.hip, grb_assign.hip, grb_kron.hip) for device-resident and large ones. */
GrB_Info GrB_Vector_extract(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc);
GrB_Info GrB_Col_extract(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_extract(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc);
GrB_Info GrB_Vector_assign(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_assign(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc);
GrB_Info GrB_Row_assign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc);
GrB_Info GrB_Col_assign(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index *I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_kronecker_BinaryOp(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_kronecker_Monoid(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Monoid op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);   /* the monoid's operator */
GrB_Info GrB_Matrix_kronecker_Semiring(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Semiring op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);   /* the semiring's multiplier */
GrB_Info GxB_kron(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Matrix B, const GrB_Descriptor desc);   /* the SuiteSparse 3 spelling of the BinaryOp form */
GrB_Info GrBX_kron_fill_ms(float *milliseconds);   /* device time of k_kron_fill in the most recent device-route Kronecker product of this thread, measured when GRB_MI355X_KRON_TIME=1 (0 otherwise) */
GrB_Info GxB_Matrix_diag(GrB_Matrix C, const GrB_Vector v, int64_t k, const GrB_Descriptor desc);   /* Matrix.from_diag, pygraphblas/matrix.py:333-375 */
GrB_Info GxB_Vector_diag(GrB_Vector v, const GrB_Matrix A, int64_t k, const GrB_Descriptor desc);   /* Matrix.vector_diag, pygraphblas/matrix.py:2225-2277 */
GrB_Info GrBX_diag_thresholds(uint64_t *matrix_min_entries, uint64_t *vector_min_entries);   /* entries of a host-resident operand from which GxB_Matrix_diag / GxB_Vector_diag take their device route (an operand that lives in HBM only always does) */
/* Sorting by value (the SuiteSparse 6.1 entry points) and top-k selection.  Row i of C holds the values of A's row i in sorted order at columns 0 .. len - 1, P (GrB_INT64)
   the column each came from; GrB_INP0 = GrB_TRAN sorts columns (C(k, j) is the k-th value of column j, P(k, j) its row).  C or P may be NULL, not both; C may be A;
   no mask, no accumulator.  op is GrB_LT_<T> or GrB_GT_<T> of a real type (else GrB_DOMAIN_MISMATCH) and compares A's values cast to T.  The order is total: ties by
   the smaller index, -0.0 ties +0.0, NaNs after every number under LT and GT alike.  select_topk keeps the first min(k, len) entries of every row (column under
   GrB_TRAN; the whole vector) in that order, at their own coordinates.  The device route leaves "sort<on=matrix,by=row|col,op=lt|gt,key=32|64,wave=N,lds=N,prim=N> ..." or
   "topk<...,k=K> ..." in GrBX_last_kernel_plan (the vector forms: on=vector,...,nvals=N). */
GrB_Info GxB_Matrix_sort(GrB_Matrix C, GrB_Matrix P, const GrB_BinaryOp op, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GxB_Vector_sort(GrB_Vector w, GrB_Vector p, const GrB_BinaryOp op, const GrB_Vector u, const GrB_Descriptor desc);
GrB_Info GrBX_Matrix_select_topk(GrB_Matrix C, const GrB_BinaryOp op, const GrB_Matrix A, GrB_Index k, const GrB_Descriptor desc);
GrB_Info GrBX_Vector_select_topk(GrB_Vector w, const GrB_BinaryOp op, const GrB_Vector u, GrB_Index k, const GrB_Descriptor desc);
GrB_Info GrBX_sort_thresholds(uint64_t *wave_max, uint64_t *lds_max);   /* the longest row one wave sorts in registers, the longest one workgroup sorts in LDS (longer rows: segmented radix sort) */
/* Tiling (the SuiteSparse 5.1 entry points).  Tiles is an m x n grid, row-major: tile (a, b) is Tiles[a*n + b].
   concat: C exists (any real built-in type); its previous content is discarded.  Tiles of a tile-row share nrows, tiles of a tile-column ncols, the sums are C's
   shape (else GrB_DIMENSION_MISMATCH); m == 0, n == 0 or C among the tiles is GrB_INVALID_VALUE; a NULL array or tile GrB_NULL_POINTER.  The same tile may stand
   at several positions.  Values are typecast to C's type.  No mask, no accumulator; the descriptor may be NULL and is ignored.
   split: creates m n new matrices of A's type, Tile_nrows[a] x Tile_ncols[b]; the sizes add up to A's shape (else GrB_DIMENSION_MISMATCH); a size of 0, m == 0 or
   n == 0 is GrB_INVALID_VALUE.  On any failure no handle stays allocated and Tiles[] is left as it was.  A is only read.
   The device route (GRB_MI355X_TILE: 0 host, 1 device) leaves "concat<m=M,n=N,cast=K> k_concat_count k_concat_fill" or "split<m=M,n=N> k_split_count k_split_totals
   k_split_rowptr k_split_scatter" in GrBX_last_kernel_plan; its results live in HBM only. */
GrB_Info GxB_Matrix_concat(GrB_Matrix C, const GrB_Matrix *Tiles, const GrB_Index m, const GrB_Index n, const GrB_Descriptor desc);
GrB_Info GxB_Matrix_split(GrB_Matrix *Tiles, const GrB_Index m, const GrB_Index n, const GrB_Index *Tile_nrows, const GrB_Index *Tile_ncols, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GrBX_tile_thresholds(uint64_t *concat_min_entries, uint64_t *split_min_entries);   /* entries (the sum over the tiles / of A) from which host-resident operands take the device route (an operand that lives in HBM only always does) */
GrB_Info GrBX_tile_geometry(uint64_t *out);   /* out[0] entries per chunk of the two fill kernels, out[1] their grid cap in workgroups, out[2] consecutive entries one lane of the concat fill stores: what the tests take their edges from */
/* build from tuples that may live in HBM: I / J are 64-bit indices, X holds values of the container's own type; location 0 = host arrays,
   1 = device arrays (read where they are on the device route, downloaded once for the host route).  Same outcomes as GrB_*_build_<T>. */
GrB_Info GrBX_Matrix_build_at(GrB_Matrix C, const GrB_Index *I, const GrB_Index *J, const void *X, GrB_Index nvals, const GrB_BinaryOp dup, int location);
GrB_Info GrBX_Vector_build_at(GrB_Vector w, const GrB_Index *I, const void *X, GrB_Index nvals, const GrB_BinaryOp dup, int location);
GrB_Info GrBX_build_thresholds(uint64_t *out);   /* three words: tuples from which a build takes its device route; the run of duplicates one lane folds; the longest run of an operator that is not exactly associative the device folds (beyond it: host route) */
/* extractTuples into arrays that may live in HBM: I / J are 64-bit indices, X holds values of the container's own type (no cast); *n is the capacity on entry and
   nvals on return; any of I / J / X may be NULL (that stream is not written; all NULL: only nvals).  location 0 = host arrays: exactly GrB_*_extractTuples_<own type>;
   1 = device arrays, filled in HBM (grb_tuples.hip) without a host mirror being built.  *n < nvals with an output: GrB_INSUFFICIENT_SPACE, nothing written. */
GrB_Info GrBX_Matrix_extractTuples_at(GrB_Index *I, GrB_Index *J, void *X, GrB_Index *n, const GrB_Matrix A, int location);
GrB_Info GrBX_Vector_extractTuples_at(GrB_Index *I, void *X, GrB_Index *n, const GrB_Vector v, int location);
GrB_Info GrBX_tuples_geometry(uint64_t *out);   /* out[0] entries per tile of the matrix kernel, out[1] positions per tile of the vector kernel, out[2] the grid cap in workgroups: what the tests take their edges from */
/* full matrices (every position holds an entry): values is the row-major nrows x ncols array of the type's own values, location 0 = a host array, 1 = a device
   array; the values are copied.  A full matrix is stored as the CSR whose row pointer and columns are closed form, built in HBM by one copy and one fill kernel
   (no tuples, no host mirror).  import: a complex type is GrB_DOMAIN_MISMATCH, nrows * ncols >= 2^32 - 16 GrB_INVALID_VALUE, a zero dimension gives an empty
   matrix.  export: one copy of the value array; GrB_INVALID_VALUE unless nvals == nrows * ncols.  GrB_mxm with such a matrix as its right operand may take the
   one-pass "spmm_full<k=K,group=G,slabs=S,long=N,cast=0|1> ..." route (GRB_MI355X_FULL: 0 never, 1 wherever legal). */
GrB_Info GrBX_Matrix_import_Full(GrB_Matrix *A, GrB_Type type, GrB_Index nrows, GrB_Index ncols, const void *values, int location);
GrB_Info GrBX_Matrix_export_Full(const GrB_Matrix A, void *values, int location);   /* GrB_INVALID_VALUE unless nvals == nrows * ncols */
GrB_Info GrBX_spmm_geometry(uint64_t *out);   /* out[0] L, out[1] columns per slab, out[2] waves per workgroup, out[3] grid cap in workgroups, out[4] SPMM_FULL_MIN_PRODUCTS */
/* GrB_mxm of two FULL matrices under a plain mask, S<M> = X (+).(x) Y' (X m x k, Y n x k: C.mxm(X, Y, mask = M, desc = T1); sampled dense-dense product), may
   take the one-pass "sddmm<k=K,group=G,entries=E,cast=0|1> k_sddmm" route: T's pattern is the mask's, every entry the dot product of two contiguous rows
   (GRB_MI355X_SDDMM: 0 never, 1 wherever legal; by itself from SDDMM_MIN_WORK = m k n).  Fold order, a function of k alone: with G = pow2ceil(min(k, 64)) lane g
   of an entry's group folds its products l = g, g + G, ... left to right from the first one, then p_g = p_g (+) p_{g + s} for s = G / 2 ... 1 where
   g + s < min(k, G): the oracle's left-to-right order for k <= 2 only; the same bits on every run and wherever the entry lies in the mask. */
GrB_Info GrBX_sddmm_geometry(uint64_t *out);   /* out[0] mask entries per tile (= per workgroup), out[1] waves per workgroup, out[2] grid cap in workgroups, out[3] SDDMM_MIN_WORK */
/* GrB_mxm of two FULL matrices, T = op(A) (+).(x) op(B) (X.mxm(W), X.mxm(Y, desc = T1): the dense update of a GNN layer, a Gram matrix, all-pairs MIN_PLUS on a
   dense block), may take the one-pass "gemm_full<m=M,n=N,k=K,tile=TMxTN,layout=NN|NT|TN|TT,cast=0|1> k_full_pattern k_gemm_full" route: a register-tiled kernel
   that stages both operands in LDS and reads a transposed operand where it lies (GRB_MI355X_GEMM: 0 never, 1 wherever legal; by itself without a plain mask,
   from 2 columns, GEMM_FULL_MIN_WORK = m k n and 16 tiles of the result, and not while GRB_MI355X_FULL is set).  Fold order: T(i, j) is the left-to-right fold of its products in
   ascending l from the first one, for every k, whatever the tile, the tile shape, the layout, the grid or the run. */
GrB_Info GrBX_gemm_geometry(uint64_t *out);   /* out[0], out[1] TM, TN of the wide tile, out[2], out[3] of the tall tile, out[4] KT, out[5] waves per workgroup, out[6] grid cap in workgroups, out[7] GEMM_FULL_MIN_WORK, out[8] the widest result (n) that takes the tall tile */
/* GrB_mxv / GrB_vxm with a FULL matrix (X.mxv(w), y.vxm(X): a linear model's scores, the halves X'(X w) of a power iteration, attention logits) may take the
   one-pass "gemv_full<m=M,k=K,layout=N|T,holes=0|1,chunks=C,cast=0|1> k_gemv_n_short|k_gemv_n_wave|k_gemv_t [k_gemv_fold]" route (m the outer length, k the
   inner): a stream over A's own value array in either orientation — no column words, no SpMV plan, no transposed copy (GRB_MI355X_GEMV: 0 never, 1 wherever
   legal; by itself from GEMV_FULL_MIN_WORK = nrows ncols; not when GRB_MI355X_SPMV names a kernel).  Fold order: a function of k, the layout, the value size and
   u's pattern alone; every fold starts from its first existing product; the oracle's left-to-right order for k <= 2 (N) and k <= 65 (T). */
GrB_Info GrBX_gemv_geometry(uint64_t *out);   /* out[0] bytes per lane load, out[1] the longest row (N) that shares a wave, out[2] products per chunk (N), out[3] waves per workgroup, out[4] grid cap in workgroups, out[5] fewest rows per chunk (T), out[6] most chunks per column (T), out[7] GEMV_FULL_MIN_WORK, out[8] packets in flight per lane (N), out[9] values per packet at most */
/* index-list extract / assign with a list that may lie in HBM: the arguments of the GrB_ namesake plus the location of each list.  location 0 = a host array, GrB_ALL
   or a GxB_RANGE / GxB_STRIDE / GxB_BACKWARDS triple: exactly the GrB_ call.  1 = `ni` 64-bit indices at a device address (or GrB_ALL; a range code as the count is
   GrB_INVALID_VALUE): parsed where they lie (grb_index.hip), the device route wherever it is legal, else the list is copied down once for the host route.
   Same outcomes as the GrB_ call with the same list on the host. */
GrB_Info GrBX_Vector_extract_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc, int location);
GrB_Info GrBX_Col_extract_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc, int location);
GrB_Info GrBX_Matrix_extract_at(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc, int location_i, int location_j);
GrB_Info GrBX_Vector_assign_at(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc, int location);
GrB_Info GrBX_Matrix_assign_at(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc, int location_i, int location_j);
GrB_Info GrBX_Row_assign_at(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, GrB_Index i, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc, int location);
GrB_Info GrBX_Col_assign_at(GrB_Matrix C, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Index *I, GrB_Index ni, GrB_Index j, const GrB_Descriptor desc, int location);
/* a vector as an index list: the VALUES of its entries in index order (one of the eight integer types, else GrB_DOMAIN_MISMATCH; signed values are sign-extended
   and read as unsigned, so a negative value is out of bounds); NULL = all; the output itself as the index vector is GrB_INVALID_VALUE.  The list is made in HBM. */
GrB_Info GrBX_Vector_extract_Vector(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Vector Ivec, const GrB_Descriptor desc);
GrB_Info GrBX_Vector_assign_Vector(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Vector u, const GrB_Vector Ivec, const GrB_Descriptor desc);
GrB_Info GrBX_Matrix_extract_Vector(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_Matrix A, const GrB_Vector Ivec, const GrB_Vector Jvec, const GrB_Descriptor desc);
GrB_Info GrBX_index_parse(const GrB_Index *I, GrB_Index ni, GrB_Index dim, int *increasing);   /* the parse of a list in HBM alone (bounds against dim, the strictly-increasing flag): what tools/index_probe.py times */
GrB_Info GrBX_index_geometry(uint64_t *out);   /* out[0] indices one workgroup of the parse kernel takes per round, out[1] its grid cap in workgroups: what the tests take their edges from */
GrB_Info GxB_Matrix_apply_BinaryOp1st(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GxB_Scalar x, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GxB_Matrix_apply_BinaryOp2nd(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, const GxB_Scalar y, const GrB_Descriptor desc);
GrB_Info GxB_Vector_apply_BinaryOp1st(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GxB_Scalar x, const GrB_Vector u, const GrB_Descriptor desc);
GrB_Info GxB_Vector_apply_BinaryOp2nd(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Vector u, const GxB_Scalar y, const GrB_Descriptor desc);
/* Element-wise union with fill values (the SuiteSparse 6 entry points): on the union of the two patterns T(i,j) = add(A(i,j), B(i,j)) where both operands hold an
   entry, add(A(i,j), beta) where only A does, add(alpha, B(i,j)) where only B does — eWiseAdd copies the single entry there and never calls the operator, which is
   wrong for MINUS, DIV and the comparisons.  Then C<Mask, replace> = accum(C, T) as in eWiseAdd; GrB_INP0 / GrB_INP1 transpose A / B (matrix form); C may be A or B.
   alpha is typecast into add's x type and beta into its y type, A and B as in eWiseAdd; add may be user-defined (GxB_BinaryOp_new).  A NULL C, add, A, B, alpha or
   beta: GrB_NULL_POINTER; an uninitialised object: GrB_UNINITIALIZED_OBJECT; a scalar without an entry: GrB_INVALID_VALUE — these three before a device is asked
   for; a complex scalar or container: GrB_DOMAIN_MISMATCH; then the dimensions.  Runs eagerly (never queued in non-blocking mode; deferred work is completed
   first).  GrBX_last_kernel_plan names the route: "ewise_union<on=matrix|vector,op=...> k_merge_fill<union> | k_vec_ewise_fused<union> | k_vec_ewise<union>",
   "ewise_batch<... as one vector, union>", "ewise_rows<N x vector eWise union>", "userop<name=...,kind=eunion,...>".  No Monoid / Semiring forms. */
GrB_Info GxB_Matrix_eWiseUnion(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp add, const GrB_Matrix A, const GxB_Scalar alpha, const GrB_Matrix B, const GxB_Scalar beta, const GrB_Descriptor desc);
GrB_Info GxB_Vector_eWiseUnion(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp add, const GrB_Vector u, const GxB_Scalar alpha, const GrB_Vector v, const GxB_Scalar beta, const GrB_Descriptor desc);
extern double GxB_ALWAYS_HYPER;
extern double GxB_NEVER_HYPER;
extern double GxB_HYPER_DEFAULT;
GrB_Info GrBX_dist_unique_id(void *id, int len);      /* 128 bytes, made on one rank and handed to all (any channel) */
GrB_Info GrBX_dist_init(int rank, int world, const void *id, int len);   /* ncclCommInitRank on this process's GPU */
GrB_Info GrBX_dist_finalize(void);
GrB_Info GrBX_dist_info(int *rank, int *world);
GrB_Info GrBX_dist_transport(char *buf, int len);      /* file name of the RCCL-ABI library bound for the exchange (librccl, or a test stand-in named by GRB_MI355X_RCCL); "" before the first use */
GrB_Info GrBX_Vector_allgatherv_start(GrB_Vector full, const GrB_Vector local, const GrB_Index *bounds, int presence);
GrB_Info GrBX_dist_wait(void);                        /* the compute stream waits for the exchange started above */
GrB_Info GrBX_Vector_allgatherv(GrB_Vector full, const GrB_Vector local, const GrB_Index *bounds, int presence);
GrB_Info GrBX_Vector_allgatherv_bits(GrB_Vector full, const GrB_Vector local, const GrB_Index *bounds);   /* BOOL frontier, 1 bit per vertex */
GrB_Info GrBX_dist_allreduce(void *host_buf, GrB_Index count, GrB_Type type, GrB_BinaryOp op);
""")

# typed families
for t in REAL:
    c = CTYPE[t]
    H.append(f"""
GrB_Info GrB_Matrix_build_{t}(GrB_Matrix C, const GrB_Index *I, const GrB_Index *J, const {c} *X, GrB_Index nvals, const GrB_BinaryOp dup);
GrB_Info GrB_Matrix_setElement_{t}(GrB_Matrix C, {c} x, GrB_Index i, GrB_Index j);
GrB_Info GrB_Matrix_extractElement_{t}({c} *x, const GrB_Matrix A, GrB_Index i, GrB_Index j);
GrB_Info GrB_Matrix_extractTuples_{t}(GrB_Index *I, GrB_Index *J, {c} *X, GrB_Index *nvals, const GrB_Matrix A);
GrB_Info GrB_Matrix_reduce_{t}({c} *c, const GrB_BinaryOp accum, const GrB_Monoid monoid, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GrB_Vector_build_{t}(GrB_Vector w, const GrB_Index *I, const {c} *X, GrB_Index nvals, const GrB_BinaryOp dup);
GrB_Info GrB_Vector_setElement_{t}(GrB_Vector w, {c} x, GrB_Index i);
GrB_Info GrB_Vector_extractElement_{t}({c} *x, const GrB_Vector v, GrB_Index i);
GrB_Info GrB_Vector_extractTuples_{t}(GrB_Index *I, {c} *X, GrB_Index *nvals, const GrB_Vector v);
GrB_Info GrB_Vector_reduce_{t}({c} *c, const GrB_BinaryOp accum, const GrB_Monoid monoid, const GrB_Vector u, const GrB_Descriptor desc);
GrB_Info GrB_Vector_assign_{t}(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, {c} x, const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc);
GrB_Info GrB_Matrix_assign_{t}(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, {c} x, const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc);
GrB_Info GxB_Vector_apply_BinaryOp1st_{t}(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, {c} x, const GrB_Vector u, const GrB_Descriptor desc);
GrB_Info GxB_Vector_apply_BinaryOp2nd_{t}(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Vector u, {c} y, const GrB_Descriptor desc);
GrB_Info GxB_Matrix_apply_BinaryOp1st_{t}(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, {c} x, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GxB_Matrix_apply_BinaryOp2nd_{t}(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, {c} y, const GrB_Descriptor desc);
GrB_Info GxB_Scalar_setElement_{t}(GxB_Scalar s, {c} x);
GrB_Info GxB_Scalar_extractElement_{t}({c} *x, const GxB_Scalar s);
GrB_Info GrB_Monoid_new_{t}(GrB_Monoid *monoid, GrB_BinaryOp op, {c} identity);
""")
# complex types: the handles and the 17 typed entry points exist so that the reference's type registry imports
# (pygraphblas/types.py:87-110 resolves them for all 13 types).  Complex containers are kept on the host: entries can be
# built, set, read, listed and assigned; everything that would compute on them returns GrB_DOMAIN_MISMATCH
H.append("""
/* ---- complex types: host-side containers (build / set / extract / assign a scalar); arithmetic on them
 *      (reduce, apply, monoids, every device operation) returns GrB_DOMAIN_MISMATCH ---- */
typedef struct { float re; float im; } GxB_FC32_t;
typedef struct { double re; double im; } GxB_FC64_t;
""")
for t, c in (("FC32", "GxB_FC32_t"), ("FC64", "GxB_FC64_t")):
    H.append(f"""
GrB_Info GxB_Matrix_build_{t}(GrB_Matrix C, const GrB_Index *I, const GrB_Index *J, const {c} *X, GrB_Index nvals, const GrB_BinaryOp dup);
GrB_Info GxB_Vector_build_{t}(GrB_Vector w, const GrB_Index *I, const {c} *X, GrB_Index nvals, const GrB_BinaryOp dup);
GrB_Info GxB_Matrix_setElement_{t}(GrB_Matrix C, {c} x, GrB_Index i, GrB_Index j);
GrB_Info GxB_Matrix_extractElement_{t}({c} *x, const GrB_Matrix A, GrB_Index i, GrB_Index j);
GrB_Info GxB_Matrix_extractTuples_{t}(GrB_Index *I, GrB_Index *J, {c} *X, GrB_Index *nvals, const GrB_Matrix A);
GrB_Info GxB_Matrix_reduce_{t}({c} *c, const GrB_BinaryOp accum, const GrB_Monoid monoid, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GxB_Vector_setElement_{t}(GrB_Vector w, {c} x, GrB_Index i);
GrB_Info GxB_Vector_extractElement_{t}({c} *x, const GrB_Vector v, GrB_Index i);
GrB_Info GxB_Vector_extractTuples_{t}(GrB_Index *I, {c} *X, GrB_Index *nvals, const GrB_Vector v);
GrB_Info GxB_Vector_reduce_{t}({c} *c, const GrB_BinaryOp accum, const GrB_Monoid monoid, const GrB_Vector u, const GrB_Descriptor desc);
GrB_Info GxB_Vector_assign_{t}(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, {c} x, const GrB_Index *I, GrB_Index ni, const GrB_Descriptor desc);
GrB_Info GxB_Matrix_assign_{t}(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, {c} x, const GrB_Index *I, GrB_Index ni, const GrB_Index *J, GrB_Index nj, const GrB_Descriptor desc);
GrB_Info GxB_Vector_apply_BinaryOp1st_{t}(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, {c} x, const GrB_Vector u, const GrB_Descriptor desc);
GrB_Info GxB_Vector_apply_BinaryOp2nd_{t}(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Vector u, {c} y, const GrB_Descriptor desc);
GrB_Info GxB_Matrix_apply_BinaryOp1st_{t}(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, {c} x, const GrB_Matrix A, const GrB_Descriptor desc);
GrB_Info GxB_Matrix_apply_BinaryOp2nd_{t}(GrB_Matrix C, const GrB_Matrix Mask, const GrB_BinaryOp accum, const GrB_BinaryOp op, const GrB_Matrix A, {c} y, const GrB_Descriptor desc);
GrB_Info GxB_Scalar_setElement_{t}(GxB_Scalar s, {c} x);
GrB_Info GxB_Scalar_extractElement_{t}({c} *x, const GxB_Scalar s);
GrB_Info GxB_Monoid_new_{t}(GrB_Monoid *monoid, GrB_BinaryOp op, {c} identity);
""")
with open(os.path.join(ROOT, "include/grb_mi355x.h"), "w") as f:
    f.write("".join(H))
print(f"types={len(types)} unops={len(unops)} binops={len(binops)} monoids={len(monoids)} "
      f"semirings={len(semirings)} descs={len(descs)}")
