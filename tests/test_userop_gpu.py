"""User-defined operators on the device: apply, apply with a bound scalar (typed and GxB_Scalar entry points), eWiseAdd and eWiseMult on matrices and
vectors, for FP32, FP64 and INT64 operators — plain, under value / structural / complemented masks, with replace, with the accumulator PLUS, with transposed
inputs and with an operand of another type.

The model is the Python function itself, applied entry by entry on the host, with the cast and accumulator rules of tests/companion_model.py (`wrap`,
`binop`) and the C API's mask / replace rule written out below.  Patterns must be identical; arithmetic-only operators must be bit-exact.

Operators that call the math library: the convention of tests/test_operator_table_gpu.py — the largest relative error measured on the device against the
host's double evaluation goes into MEASURED below (and DESIGN.md section 8) and the bound becomes twice that value.  Until a value is measured the bound is
the project's existing one for one math call (FP64: relative 1e-12, FP32: one ulp) times the number of math calls in the operator.
    MEASURED = {(operator, type): largest relative error (FP64) / largest error in ulp (FP32) over this file's inputs}"""
import ctypes as C
import math
import os
import subprocess
import sys
import zlib
from math import exp, log1p

import numpy as np
import pytest

from companion_model import wrap, binop

pytestmark = pytest.mark.gpu

# measured on an MI355X (ROCm 7 device math library) over the inputs of test_math_library_operators_within_the_stated_bound, matrices and vectors, all four kinds;
# the float32 results are the double evaluation rounded once, and every one of them equalled the host's: 0 ulp, so the bound (twice that) asks for equality
MEASURED = {("log_plus", "FP64"): 4.802e-15, ("softplus", "FP64"): 2.201e-16, ("log_plus", "FP32"): 0.0, ("softplus", "FP32"): 0.0}
MATH_CALLS = {"log_plus": 2, "softplus": 2}
HALF = 0.5


# ---- the operators (module level: the translator reads their source) ---------------------------------------------------------------------------------
def f_arith(x, y):
    return x * y - (x + y) * HALF


def i_arith(x, y):
    return (x * 3 + y) // 2 - (x % 5)


def log_plus(x, y):                                   # Log-Semiring.ipynb: Log32.PLUS
    return x + log1p(exp(y - x))


def f_unary(x):
    return x * x + 1


def i_unary(x):
    return (x << 1) ^ 3


def softplus(x):
    return log1p(exp(x))


def const9(x, y):
    return 9


def one_bit_off(i, j):                                # N-Cube-Graphs.ipynb, as it stands there
    def bit_count(i):
        assert 0 <= i < 0x100000000
        i = i - ((i >> 1) & 0x55555555)
        i = (i & 0x33333333) + ((i >> 2) & 0x33333333)
        return (((i + (i >> 4) & 0xF0F0F0F) * 0x1010101) & 0xffffffff) >> 24

    if bit_count(i ^ j) == 1:
        return 1
    return 0


BIN = {"FP32": f_arith, "FP64": f_arith, "INT64": i_arith}
UN = {"FP32": f_unary, "FP64": f_unary, "INT64": i_unary}
NPT = {"FP32": np.float32, "FP64": np.float64, "INT64": np.int64, "INT32": np.int32, "BOOL": np.bool_}
OTHER = {"FP32": "INT32", "FP64": "FP32", "INT64": "INT32"}      # the "operand of another type" of each operator type
_OPS = {}


def user_op(gb, func, typ, nargs):
    key = (func.__name__, typ, nargs)
    if key not in _OPS:
        _OPS[key] = (gb.binary_op if nargs == 2 else gb.unary_op)(getattr(gb, typ))(func)
    return _OPS[key]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------------
def pyval(typ, x):
    return bool(x) if typ == "BOOL" else (float(x) if typ.startswith("FP") else int(x))


def to_type(typ, r):
    """A Python number as a value of the GraphBLAS type: float32 rounds, integers take companion_model's C cast."""
    if typ == "FP32":
        return float(np.float32(r))
    if typ == "FP64":
        return float(r)
    return wrap(typ, int(r) if isinstance(r, float) else r)


def call(func, typ, *args):
    """The operator on values cast into its type, its result converted to its type."""
    return to_type(typ, func(*[pyval(typ, to_type(typ, a)) for a in args]))


def model_T(kind, func, typ, A, B=None, scalar=None):
    if kind == "apply":
        return {p: call(func, typ, a) for p, a in A.items()}
    if kind == "bind1st":
        return {p: call(func, typ, scalar, a) for p, a in A.items()}
    if kind == "bind2nd":
        return {p: call(func, typ, a, scalar) for p, a in A.items()}
    if kind == "emult":
        return {p: call(func, typ, A[p], B[p]) for p in A if p in B}
    out = {}
    for p in set(A) | set(B):                        # eWiseAdd: one operand alone has the entry -> it is copied (cast into the operator's type), no call
        out[p] = call(func, typ, A[p], B[p]) if (p in A and p in B) else to_type(typ, A[p] if p in A else B[p])
    return out


def model_write_back(Cd, ctyp, T, ttyp, mask, structural, comp, replace, accum_plus):
    """C<M, replace> = accum(C, T) of the C API: Z = T or accum(C, T) on the union; where the mask allows, C takes Z's entry or loses its own; where it does not,
    C keeps its entry unless replace."""
    def plus(c, t):                                    # the accumulator PLUS of C's type on (C's entry, T's entry cast into that type)
        if ctyp == "FP32":
            return float(np.float32(c) + np.float32(to_type(ctyp, t)))
        if ctyp == "FP64":
            return c + to_type(ctyp, t)
        return binop("PLUS", ctyp, c, to_type(ctyp, t))
    if accum_plus:
        Z = {p: plus(Cd[p], T[p]) if (p in Cd and p in T) else to_type(ctyp, Cd[p] if p in Cd else T[p]) for p in set(Cd) | set(T)}
    else:
        Z = {p: to_type(ctyp, x) for p, x in T.items()}
    out = {}
    for p in set(Cd) | set(Z) | (set(mask) if mask is not None else set()):
        if mask is None:
            allowed = not comp
        else:
            allowed = (p in mask and (structural or bool(mask[p]))) != comp
        if allowed:
            if p in Z:
                out[p] = Z[p]
        elif not replace and p in Cd:
            out[p] = Cd[p]
    return out


# ---- operands -----------------------------------------------------------------------------------------------------------------------------------------------
def values(rng, typ, n):
    if typ.startswith("FP"):
        return (rng.integers(-24, 25, n) / 8.0).astype(NPT[typ])
    if typ == "BOOL":
        return rng.integers(0, 2, n).astype(np.bool_)
    return rng.integers(-40, 41, n).astype(NPT[typ])


def rand_mat(gb, rng, typ, nr, nc, density):
    k = max(1, int(nr * nc * density))
    flat = np.sort(rng.choice(nr * nc, size=k, replace=False))
    I, J = np.divmod(flat, nc)
    X = values(rng, typ, k)
    d = {(int(i), int(j)): pyval(typ, x) for i, j, x in zip(I, J, X)}
    return gb.Matrix.from_arrays(I.astype(np.uint64), J.astype(np.uint64), X, nr, nc, getattr(gb, typ)), d


def rand_vec(gb, rng, typ, n, density):
    k = max(1, int(n * density))
    I = np.sort(rng.choice(n, size=k, replace=False))
    X = values(rng, typ, k)
    return gb.Vector.from_arrays(I.astype(np.uint64), X, n, getattr(gb, typ)), {int(i): pyval(typ, x) for i, x in zip(I, X)}


def got_dict(obj):
    arrs = obj.to_arrays()
    typ = obj.type.__name__
    if len(arrs) == 3:
        return {(int(i), int(j)): pyval(typ, x) for i, j, x in zip(*arrs)}
    return {int(i): pyval(typ, x) for i, x in zip(*arrs)}


def same_bits(a, b):
    if isinstance(a, float) or isinstance(b, float):
        return (a == b and math.copysign(1.0, a) == math.copysign(1.0, b)) or (a != a and b != b)
    return a == b


def compare(got, want, what, typ=None, opname=None):
    assert set(got) == set(want), f"{what}: pattern differs: {sorted(set(got) ^ set(want))[:8]}"
    calls = MATH_CALLS.get(opname)
    worst = 0.0
    for p in want:
        g, w = got[p], want[p]
        if calls is None or not typ.startswith("FP"):
            assert same_bits(g, w), f"{what}: entry {p}: got {g!r}, the model has {w!r} (bit-exact required)"
            continue
        if not math.isfinite(w):
            assert same_bits(g, w) or str(g) == str(w), f"{what}: entry {p}: got {g!r}, the model has {w!r}"
            continue
        if typ == "FP64":
            err = abs(g - w) / abs(w) if w else abs(g - w)
            bound = 2 * MEASURED[(opname, typ)] if (opname, typ) in MEASURED else 1e-12 * calls
        else:
            err = abs(g - w) / float(np.spacing(np.float32(abs(w)))) if w else abs(g - w) / float(np.finfo(np.float32).tiny)
            bound = 2 * MEASURED[(opname, typ)] if (opname, typ) in MEASURED else 1.0 * calls
        worst = max(worst, err)
        assert err <= bound, f"{what}: entry {p}: got {g!r}, the model has {w!r}: error {err:.3e} beyond {bound:.3e}"
    if calls is not None and typ.startswith("FP"):
        print(f"  largest error of {opname} {typ} ({what}): {worst:.3e} {'relative' if typ == 'FP64' else 'ulp'}")
    return worst


def residency(gb, obj):
    w = C.c_int(-1)
    fn = gb.lib.GrBX_Matrix_residency if obj._kind == "matrix" else gb.lib.GrBX_Vector_residency
    assert fn(obj._h, C.byref(w)) == 0
    return w.value


def scalar_handle(gb, typ, x):
    s = C.c_void_p()
    T = getattr(gb, typ)
    assert gb.lib.GxB_Scalar_new(C.byref(s), C.c_void_p(T._h)) == 0
    assert getattr(gb.lib, "GxB_Scalar_setElement_" + typ)(s, T._c(x)) == 0
    return s


KINDS = ["apply", "bind1st", "bind2nd", "bind1st_scalar", "bind2nd_scalar", "eadd", "emult"]
# (name, mask: None | "value" | "struct", complemented, replace, accumulator PLUS, transposed inputs, operand of another type)
VARIANTS = [("plain", None, False, False, False, False, False), ("value mask", "value", False, False, False, False, False),
            ("structural mask", "struct", False, False, False, False, False), ("complemented mask", "value", True, False, False, False, False),
            ("complemented structural mask + replace", "struct", True, True, False, False, False), ("mask + replace", "value", False, True, False, False, False),
            ("accum PLUS", None, False, False, True, False, False), ("mask + accum PLUS", "value", False, False, True, False, False),
            ("transposed", None, False, False, False, True, False), ("transposed + mask + accum", "struct", False, False, True, True, False),
            ("other type", None, False, False, False, False, True), ("other type + mask + replace + accum", "value", False, True, True, False, True)]


def descriptor(gb, structural, comp, replace, t0, t1):
    name = ("R" if replace else "") + ("S" if structural else "") + ("C" if comp else "") + ("T0" if t0 else "") + ("T1" if t1 else "")
    return getattr(gb.descriptor, name) if name else None


def run_kind(gb, kind, op, typ, A, B, scalar, out, mask, accum, desc):
    lib = gb.lib
    stem = "Matrix" if A._kind == "matrix" else "Vector"
    if kind == "apply":
        return A.apply(op, out=out, mask=mask, accum=accum, desc=desc)
    if kind in ("eadd", "emult"):
        return getattr(A, kind)(B, op, out=out, mask=mask, accum=accum, desc=desc)
    from pygraphblas_amd.matrix import get_args
    mh, ah, dh = get_args(mask, accum, desc)
    oph = C.c_void_p(op.get_op())
    T = getattr(gb, typ)
    if kind == "bind1st":
        gb.base.check(getattr(lib, f"GxB_{stem}_apply_BinaryOp1st_{typ}")(out._h, mh, ah, oph, T._c(scalar), A._h, dh), out)
    elif kind == "bind2nd":
        gb.base.check(getattr(lib, f"GxB_{stem}_apply_BinaryOp2nd_{typ}")(out._h, mh, ah, oph, A._h, T._c(scalar), dh), out)
    else:
        s = scalar_handle(gb, typ, scalar)
        try:
            if kind == "bind1st_scalar":
                gb.base.check(getattr(lib, f"GxB_{stem}_apply_BinaryOp1st")(out._h, mh, ah, oph, s, A._h, dh), out)
            else:
                gb.base.check(getattr(lib, f"GxB_{stem}_apply_BinaryOp2nd")(out._h, mh, ah, oph, A._h, s, dh), out)
        finally:
            lib.GxB_Scalar_free(C.byref(s))
    return out


@pytest.mark.parametrize("typ", ["FP32", "FP64", "INT64"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("container", ["matrix", "vector"])
def test_small_random_against_the_python_function(gb, gpu, container, kind, typ):
    rng = np.random.default_rng(zlib.crc32(f"{container} {kind} {typ}".encode()))
    func = UN[typ] if kind == "apply" else BIN[typ]
    op = user_op(gb, func, typ, 1 if kind == "apply" else 2)
    mkind = kind.split("_")[0]
    scalar = 1.25 if typ.startswith("FP") else 7
    nr, nc = 23, 17
    for name, mask_kind, comp, replace, accum_plus, transposed, other in VARIANTS:
        if container == "vector" and transposed:
            continue                                                       # (a vector has no transpose)
        atyp = OTHER[typ] if other else typ
        ctyp = typ
        if container == "matrix":
            A, Ad = rand_mat(gb, rng, atyp, nc if transposed else nr, nr if transposed else nc, 0.3)
            B, Bd = rand_mat(gb, rng, typ, nc if transposed else nr, nr if transposed else nc, 0.3)
            Cm, Cd = rand_mat(gb, rng, ctyp, nr, nc, 0.25)
            M, Md = rand_mat(gb, rng, "INT32", nr, nc, 0.5) if mask_kind else (None, None)
            if transposed:
                Ad = {(j, i): x for (i, j), x in Ad.items()}
                Bd = {(j, i): x for (i, j), x in Bd.items()}
        else:
            A, Ad = rand_vec(gb, rng, atyp, 301, 0.4)
            B, Bd = rand_vec(gb, rng, typ, 301, 0.4)
            Cm, Cd = rand_vec(gb, rng, ctyp, 301, 0.3)
            M, Md = rand_vec(gb, rng, "INT32", 301, 0.5) if mask_kind else (None, None)
        two = mkind in ("eadd", "emult")
        desc = descriptor(gb, mask_kind == "struct", comp, replace, transposed, transposed and two)
        accum = getattr(gb, ctyp).PLUS if accum_plus else None
        T = model_T(mkind, func, typ, Ad, Bd if two else None, scalar)
        want = model_write_back(Cd, ctyp, T, typ, Md, mask_kind == "struct", comp, replace, accum_plus)
        run_kind(gb, kind, op, typ, A, B, scalar, Cm, M, accum, desc)
        plan = gb.last_kernel_plan()
        assert plan.startswith(f"userop<name={func.__name__},kind={mkind},type=GrB_{typ}>"), plan
        compare(got_dict(Cm), want, f"{container} {kind} {typ} [{name}]")


@pytest.mark.parametrize("typ", ["FP32", "FP64"])
@pytest.mark.parametrize("container", ["matrix", "vector"])
def test_math_library_operators_within_the_stated_bound(gb, gpu, container, typ):
    rng = np.random.default_rng(5)
    b = user_op(gb, log_plus, typ, 2)
    u = user_op(gb, softplus, typ, 1)
    if container == "matrix":
        A, Ad = rand_mat(gb, rng, typ, 40, 33, 0.4); B, Bd = rand_mat(gb, rng, typ, 40, 33, 0.4)
    else:
        A, Ad = rand_vec(gb, rng, typ, 2000, 0.5); B, Bd = rand_vec(gb, rng, typ, 2000, 0.5)
    worst = {}
    worst["log_plus"] = max(compare(got_dict(A.eadd(B, b)), model_T("eadd", log_plus, typ, Ad, Bd), f"{container} eadd", typ, "log_plus"),
                            compare(got_dict(A.emult(B, b)), model_T("emult", log_plus, typ, Ad, Bd), f"{container} emult", typ, "log_plus"),
                            compare(got_dict(A.apply_second(b, 0.75)), model_T("bind2nd", log_plus, typ, Ad, scalar=0.75), f"{container} bind2nd", typ, "log_plus"))
    worst["softplus"] = compare(got_dict(A.apply(u)), model_T("apply", softplus, typ, Ad), f"{container} apply", typ, "softplus")
    print(f"MEASURED candidates {container} {typ}: {worst}")


def rmat18(gb, typ, seed):
    from pygraphblas_amd import rmat
    rp, ci = rmat.csr_numpy(18, seed=seed)
    rng = np.random.default_rng(seed)
    x = values(rng, typ, len(ci))
    return gb.Matrix.from_csr(getattr(gb, typ), 1 << 18, 1 << 18, rp, ci, x), rp.astype(np.int64), ci.astype(np.int64), x


def test_rmat18_apply_eadd_emult(gb, gpu):
    typ = "FP64"
    A, arp, aci, ax = rmat18(gb, typ, 42)
    B, brp, bci, bx = rmat18(gb, typ, 43)
    n = 1 << 18
    un, bi = user_op(gb, f_unary, typ, 1), user_op(gb, f_arith, typ, 2)
    # apply: the same pattern, the function on every value
    rp, ci, x = A.apply(un).to_csr()
    assert np.array_equal(rp, arp) and np.array_equal(ci, aci)
    assert np.array_equal(x, ax * ax + 1)
    akey = np.repeat(np.arange(n, dtype=np.int64), np.diff(arp)) * n + aci
    bkey = np.repeat(np.arange(n, dtype=np.int64), np.diff(brp)) * n + bci
    both, ia, ib = np.intersect1d(akey, bkey, assume_unique=True, return_indices=True)
    fboth = ax[ia] * bx[ib] - (ax[ia] + bx[ib]) * HALF
    # eWiseMult: the intersection
    rp, ci, x = A.emult(B, bi).to_csr()
    gkey = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64))) * n + ci
    assert np.array_equal(gkey, both) and np.array_equal(x, fboth)
    # eWiseAdd: the union; the operator where both have the entry, the one value elsewhere
    rp, ci, x = A.eadd(B, bi).to_csr()
    gkey = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64))) * n + ci
    ukey = np.union1d(akey, bkey)
    assert np.array_equal(gkey, ukey)
    want = np.empty(len(ukey))
    want[np.searchsorted(ukey, akey)] = ax
    want[np.searchsorted(ukey, bkey)] = bx
    want[np.searchsorted(ukey, both)] = fboth
    assert np.array_equal(x, want)
    assert gb.last_kernel_plan().startswith("userop<name=f_arith,kind=eadd,type=GrB_FP64>")


def test_eadd_does_not_call_the_operator_where_one_side_is_missing(gb, gpu):
    op = user_op(gb, const9, "INT64", 2)
    A = gb.Matrix.from_lists([0, 0, 1, 2], [0, 1, 1, 2], [1, 2, 3, 4], 3, 3)
    B = gb.Matrix.from_lists([0, 1, 2, 2], [1, 0, 0, 2], [10, 20, 30, 40], 3, 3)
    assert got_dict(A.eadd(B, op)) == {(0, 0): 1, (0, 1): 9, (1, 0): 20, (1, 1): 3, (2, 0): 30, (2, 2): 9}
    assert got_dict(A.emult(B, op)) == {(0, 1): 9, (2, 2): 9}
    u = gb.Vector.from_lists([0, 2, 5], [1, 2, 3], 8)
    v = gb.Vector.from_lists([2, 3, 5], [10, 20, 30], 8)
    assert got_dict(u.eadd(v, op)) == {0: 1, 2: 9, 3: 20, 5: 9}
    assert got_dict(u.emult(v, op)) == {2: 9, 5: 9}


def test_operands_stay_in_hbm_and_the_result_is_made_there(gb, gpu):
    rng = np.random.default_rng(9)
    A0, _ = rand_mat(gb, rng, "FP64", 50, 50, 0.2)
    B0, _ = rand_mat(gb, rng, "FP64", 50, 50, 0.2)
    A, B = A0.apply(gb.FP64.AINV), B0.apply(gb.FP64.ABS)                  # results of device operations: their only valid image is in HBM
    assert residency(gb, A) == 2 and residency(gb, B) == 2
    bi, un = user_op(gb, f_arith, "FP64", 2), user_op(gb, f_unary, "FP64", 1)
    for make in (lambda: A.eadd(B, bi), lambda: A.emult(B, bi), lambda: A.apply(un), lambda: A.apply_first(2.0, bi), lambda: A.apply_second(bi, 2.0)):
        R = make()
        assert residency(gb, A) == 2 and residency(gb, B) == 2 and residency(gb, R) == 2
    u0, _ = rand_vec(gb, rng, "FP64", 500, 0.5)
    v0, _ = rand_vec(gb, rng, "FP64", 500, 0.5)
    with gb.descriptor.S:                                                  # (any eager device operation: a masked apply is never queued)
        u, v = u0.apply(gb.FP64.AINV, mask=u0), v0.apply(gb.FP64.ABS, mask=v0)
    assert residency(gb, u) == 2 and residency(gb, v) == 2
    for make in (lambda: u.eadd(v, bi), lambda: u.emult(v, bi), lambda: u.apply(un), lambda: u.apply_first(2.0, bi), lambda: u.apply_second(bi, 2.0)):
        r = make()
        assert residency(gb, u) == 2 and residency(gb, v) == 2 and residency(gb, r) == 2


_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import pygraphblas_amd as gb
import test_userop_gpu as t
A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
op = gb.binary_op(gb.FP64)(t.f_arith); un = gb.unary_op(gb.FP64)(t.f_unary)
print(sorted(t.got_dict(A.eadd(A, op)).items()), sorted(t.got_dict(A.apply(un)).items()))
c, d, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
gb.lib.GrBX_userop_stats(C.byref(c), C.byref(d), C.byref(l))
print("STATS", c.value, d.value, l.value)
"""


def test_a_second_process_compiles_nothing(gb, gpu, tmp_path):
    env = dict(os.environ, GRB_MI355X_CACHE_DIR=str(tmp_path / "cache"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD.format(root=root, tests=os.path.join(root, "tests"))
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout.strip().splitlines())
    first, second = (o[-1].split() for o in outs)
    assert first[0] == "STATS" and int(first[1]) == 2 and int(first[2]) == 0 and int(first[3]) == 2, outs[0]
    assert int(second[1]) == 0 and int(second[2]) == 2 and int(second[3]) == 2, outs[1]      # nothing compiled: both kernels came from the disk cache
    assert outs[0][0] == outs[1][0]
    assert len([f for f in os.listdir(tmp_path / "cache") if f.startswith("userop-") and f.endswith(".co")]) == 2


def new_binop(gb, typ, name, defn):
    h, t = C.c_void_p(), C.c_void_p(getattr(gb, typ)._h)
    assert gb.lib.GxB_BinaryOp_new(C.byref(h), None, t, t, t, name.encode(), defn.encode()) == 0
    return h


def test_a_definition_that_does_not_compile_is_an_error_with_the_log(gb, gpu):
    h = new_binop(gb, "FP64", "broken", "void broken (double *z, const double *x, const double *y) { (*z) = (*x) +* ; }")
    A = gb.Matrix.from_lists([0, 1], [1, 0], [1.0, 2.0])
    out = gb.Matrix.from_lists([0], [0], [5.0], 2, 2)
    info = gb.lib.GrB_Matrix_eWiseAdd_BinaryOp(out._h, None, None, h, A._h, A._h, None)
    assert info not in (0, gb._capi.constants["GrB_PANIC"])
    s = C.c_char_p()
    assert gb.lib.GrB_Matrix_error(C.byref(s), out._h) == 0
    msg = s.value.decode()
    assert "broken" in msg and "error" in msg and "expected expression" in msg, msg
    assert got_dict(out) == {(0, 0): 5.0}
    assert gb.lib.GrB_Matrix_eWiseAdd_BinaryOp(out._h, None, None, h, A._h, A._h, None) == info      # (remembered: not compiled again, the same answer)
    gb.lib.GrB_BinaryOp_free(C.byref(h))


def test_every_other_use_is_refused_and_leaves_the_output_alone(gb, gpu):
    DM = gb.DomainMismatch
    op = user_op(gb, f_arith, "FP64", 2)
    un = user_op(gb, f_unary, "FP64", 1)
    A = gb.Matrix.from_lists([0, 1, 2], [1, 2, 0], [1.0, 2.0, 3.0])
    v = gb.Vector.from_lists([0, 1, 2], [2.0, 3.0, 4.0])
    out = gb.Matrix.from_lists([0], [0], [5.0], 3, 3)
    w = gb.Vector.from_lists([1], [6.0], 3)
    calls = [
        ("accumulator of mxm", lambda: A.mxm(A, out=out, accum=op)), ("accumulator of eWiseAdd", lambda: A.eadd(A, gb.FP64.PLUS, out=out, accum=op)),
        ("accumulator of apply", lambda: A.apply(gb.FP64.AINV, out=out, accum=op)), ("accumulator of a user apply", lambda: A.apply(un, out=out, accum=op)),
        ("accumulator of mxv", lambda: A.mxv(v, out=w, accum=op)), ("accumulator of a vector eWiseMult", lambda: v.emult(v, gb.FP64.TIMES, out=w, accum=op)),
        ("accumulator of transpose", lambda: A.transpose(out=out, accum=op)), ("kronecker", lambda: A.kronecker(A, op, out=gb.Matrix.sparse(gb.FP64, 9, 9))),
        ("accumulator of a scalar assign", lambda: gb.base.check(gb.lib.GrB_Vector_assign_FP64(w._h, None, C.c_void_p(op.get_op()), C.c_double(1), gb._capi.all_indices(), C.c_uint64(3), None), w)),
    ]
    for what, fn in calls:
        with pytest.raises(DM, match="f_arith"):
            fn()
        assert got_dict(out) == {(0, 0): 5.0} and got_dict(w) == {1: 6.0}, what
    # reduce: as a scalar reduction's accumulator; a monoid or a semiring cannot be made of it at all
    x = C.c_double(1.5)
    assert gb.lib.GrB_Matrix_reduce_FP64(C.byref(x), C.c_void_p(op.get_op()), C.c_void_p(gb.FP64.PLUS_MONOID.get_op()), A._h, None) == gb._capi.constants["GrB_DOMAIN_MISMATCH"]
    assert x.value == 1.5
    m = C.c_void_p()
    assert gb.lib.GrB_Monoid_new_FP64(C.byref(m), C.c_void_p(op.get_op()), C.c_double(0)) == gb._capi.constants["GrB_DOMAIN_MISMATCH"] and m.value is None
    assert gb.lib.GrB_Semiring_new(C.byref(m), C.c_void_p(gb.FP64.PLUS_MONOID.get_op()), C.c_void_p(op.get_op())) == gb._capi.constants["GrB_DOMAIN_MISMATCH"] and m.value is None
    with pytest.raises(DM, match="f_arith"):                               # reduce_vector's accumulator
        A.reduce_vector(out=w, accum=op)
    assert got_dict(w) == {1: 6.0}
    # select takes a GxB_SelectOp: a user-defined one cannot be made (GxB_SelectOp_new does not exist); its accumulator is refused like every other
    with pytest.raises(DM, match="f_arith"):
        A.select(">0", out=out, accum=op)
    assert got_dict(out) == {(0, 0): 5.0}
    # hypersparse containers (a dimension beyond the device layout)
    H = gb.Matrix.sparse(gb.FP64)
    H[3, 1 << 40] = 2.0
    H2 = gb.Matrix.sparse(gb.FP64)
    H2[7, 7] = 1.0
    for fn in (lambda: H.eadd(H, op, out=H2), lambda: H.emult(H, op, out=H2), lambda: H.apply(un, out=H2), lambda: H.apply_second(op, 1.0, out=H2)):
        with pytest.raises(DM, match="hypersparse"):
            fn()
        assert got_dict(H2) == {(7, 7): 1.0}
    hv, hv2 = gb.Vector.sparse(gb.FP64), gb.Vector.sparse(gb.FP64)
    hv[1 << 40] = 2.0
    hv2[5] = 1.0
    for fn in (lambda: hv.eadd(hv, op, out=hv2), lambda: hv.apply(un, out=hv2)):
        with pytest.raises(DM, match="hypersparse"):
            fn()
        assert got_dict(hv2) == {5: 1.0}


_MODE_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import pygraphblas_amd as gb
import test_userop_gpu as t
n = 100000
rng = np.random.default_rng(1)
u = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), rng.integers(-16, 17, n) / 8.0, n, gb.FP64)
v = gb.Vector.from_arrays(np.arange(n, dtype=np.uint64), rng.integers(-16, 17, n) / 8.0, n, gb.FP64)
un = gb.unary_op(gb.FP64)(t.f_unary); bi = gb.binary_op(gb.FP64)(t.f_arith)
w = u.eadd(v, gb.FP64.PLUS)            # deferred in non-blocking mode
w = w.apply(gb.FP64.AINV)              # ... and chained
r = w.apply(un)                        # the user operator: the pending chain is completed, then this runs eagerly
plan = gb.last_kernel_plan()
s = r.eadd(w, bi)
w2 = s.apply(gb.FP64.ABS)              # built-in work queued AFTER a user result reads it correctly too
I, X = w2.to_arrays()
print(plan.split(">")[0])
print(float(X.sum()), float(np.abs(X).max()), len(I), X[:5].tolist())
"""


def test_nonblocking_chain_then_user_apply_equals_blocking(gb, gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _MODE_CHILD.format(root=root, tests=os.path.join(root, "tests"))
    outs = []
    for blocking in ("0", "1"):
        env = dict(os.environ, GRB_MI355X_BLOCKING=blocking)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout.strip().splitlines()[-2:])
    assert outs[0] == outs[1], outs
    assert outs[0][0] == "userop<name=f_unary,kind=apply,type=GrB_FP64"
    # and against the model
    rng = np.random.default_rng(1)
    a = rng.integers(-16, 17, 100000) / 8.0
    b = rng.integers(-16, 17, 100000) / 8.0
    w = -(a + b)
    r = w * w + 1
    x = np.abs(r * w - (r + w) * HALF)
    assert outs[0][1].startswith(repr(float(x.sum())) + " ")


# ---- end to end, with the notebooks' own code ---------------------------------------------------------------------------------------------------------
def test_n_cube_notebook(gb, gpu):
    op = gb.binary_op(gb.INT64)(one_bit_off)

    def n_cube(n):
        n = 2 ** n
        A = gb.Matrix.dense(gb.INT64, n, n, fill=1)
        Ai = A.apply(gb.INT64.POSITIONI)               # the notebook's A.positioni() / A.positionj()
        Aj = A.apply(gb.INT64.POSITIONJ)
        return Ai.eadd(Aj, op).nonzero()

    N3 = n_cube(3)
    edges = {(i, j) for i in range(8) for j in range(8) if bin(i ^ j).count("1") == 1}
    assert len(edges) == 24
    assert got_dict(N3) == {e: 1 for e in edges}
    assert n_cube(2).nvals == 8


def test_log_semiring_plus(gb, gpu):
    class Log32(gb.FP32):
        @gb.binary_op(gb.FP32)
        def PLUS(x, y):
            return x + log1p(exp(y - x))

    rng = np.random.default_rng(2)
    a = rng.random(64) + 0.25
    b = rng.random(64) + 0.25
    idx = np.arange(64, dtype=np.uint64)
    A = gb.Vector.from_arrays(idx, np.log(a).astype(np.float32), 64, gb.FP32)
    B = gb.Vector.from_arrays(idx, np.log(b).astype(np.float32), 64, gb.FP32)
    I, X = A.eadd(B, Log32.PLUS).to_arrays()
    la, lb = np.log(a).astype(np.float32).astype(np.float64), np.log(b).astype(np.float32).astype(np.float64)
    want = np.log(np.exp(la) + np.exp(lb))
    assert np.array_equal(I, idx)
    # log(exp(a) + exp(b)) in float32: within a few float32 spacings of the double value (two math calls: two ulp, plus the rounding of the result)
    assert np.all(np.abs(X.astype(np.float64) - want) <= 3 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-7)
    with Log32.PLUS:                                                      # as the default eWise operator of a block
        I2, X2 = A.eadd(B).to_arrays()
    assert np.array_equal(X, X2)
