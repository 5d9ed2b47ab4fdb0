"""`Matrix` — the host-side mirror of pygraphblas.Matrix for the mxm / mxv hot path.

Same names, argument meaning and error behaviour as the reference class
(pygraphblas/matrix.py): `Matrix.sparse/dense/from_lists/random/identity`, `nrows/ncols/nvals`,
`mxm` (:2401-2584), `mxv` (:2586-2726), `@`, `@=`, `A.plus_times(B)` (:1607-1613), `iseq` (:1436-1453),
`reduce_int/float/bool` (:1759-1804), `transpose`, `tril/triu/offdiag/select`, `eadd/emult`, `apply`.
Every method is a thin call into the C ABI (include/grb_mi355x.h); arithmetic happens in HIP kernels.
Bulk constructors `from_arrays` / `from_csr` exist because the reference's per-element
`from_lists` loop (:325-330) cannot load benchmark-sized graphs.
"""
import ctypes as C
import random as _random
from functools import partial

import numpy as np

from . import _capi, types, descriptor as _d
from ._capi import lib, u64
from .base import check, eunion, NoValue, DomainMismatch
from .types import current_semiring, current_accum, current_binop, current_monoid

NULL = None


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def get_args(mask, accum, desc):
    """mask handle, accum op handle, descriptor handle from arguments or context
    (reference: Matrix._get_args, pygraphblas/matrix.py:2380-2399)."""
    mh = C.c_void_p(mask._h.value) if mask is not None else None
    if accum is None:
        accum = current_accum.get(None)
    ah = C.c_void_p(accum.get_op()) if accum is not None else None
    if desc is None:
        desc = _d.current_desc.get(None)
    dh = C.c_void_p(desc.get_desc()) if desc is not None else None
    return mh, ah, dh


class _IndexArg(tuple):
    """What build_range returns: the 4-tuple (I pointer, ni, size or None, keep-alive object), and beside it where the list lies — `location` 1: `ni` int64
    indices in HBM (a GPU tensor), for the GrBX_*_at entry points — or the `vector` whose values are the list, for the GrBX_*_Vector entry points."""
    def __new__(cls, I, ni, size, keep, location=0, vector=None):
        self = super().__new__(cls, (I, ni, size, keep))
        self.location, self.vector = location, vector
        return self


def _is_tensor(x):
    import sys
    torch = sys.modules.get("torch")                 # (a tensor cannot exist before torch was imported: no import here)
    return torch is not None and isinstance(x, torch.Tensor)


def _tensor_index(t):
    """A torch tensor as an index list: one-dimensional, contiguous, int64.  On the GPU it is read where it is (location 1) once whatever produced it has finished;
    on the CPU it is a host list."""
    import torch
    if t.dtype != torch.int64:
        raise TypeError(f"an index tensor must be int64, not {t.dtype} (use I.to(torch.int64) first)")
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError("an index tensor must be contiguous and one-dimensional")
    n = int(t.numel())
    if t.device.type != "cuda" or n == 0:            # (an empty tensor has no address: the empty host list)
        keep = np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)
        return _IndexArg(_p(keep), n, n, keep)
    torch.cuda.current_stream(t.device).synchronize()      # whatever produced the tensor has finished before the library's stream reads it
    return _IndexArg(C.c_void_p(t.data_ptr()), n, n, t, location=1)


def _vector_index_tensor(v):
    """The values of an index vector as an int64 tensor (for the operations that have no GrBX_*_Vector form): made in HBM by to_tensors."""
    import torch
    if v.type not in (types.INT8, types.UINT8, types.INT16, types.UINT16, types.INT32, types.UINT32, types.INT64, types.UINT64):
        raise DomainMismatch("an index vector must have an integer type")
    return v.to_tensors()[1].to(torch.int64).contiguous()


def _no_device_list(*indices):
    """Scalar assign takes host lists only."""
    from .vector import Vector
    for x in indices:
        if _is_tensor(x) or isinstance(x, Vector):
            raise TypeError("scalar assign through a tensor or a vector as the index list is not supported: pass the list as a numpy array")


def build_range(rslice, stop_val, vector_ok=False):
    """An index argument of the slicing operations -> (I pointer, ni, size or None, keep-alive array): a list, `None` / `:` for
    all, or a slice — whose `stop` is INCLUSIVE, as in the reference (`_build_range`, pygraphblas/base.py:216-250: GxB_RANGE /
    GxB_STRIDE / GxB_BACKWARDS index triples).  Also a torch int64 tensor (on the GPU: read in HBM, `.location` 1) and a Vector, whose values are the list
    (`vector_ok`: the caller has a GrBX_*_Vector entry point and gets `.vector`; otherwise the values become a tensor first)."""
    from .vector import Vector
    if isinstance(rslice, Vector):
        if vector_ok:
            return _IndexArg(None, 0, rslice.nvals, rslice, vector=rslice)
        rslice = _vector_index_tensor(rslice)
    if _is_tensor(rslice):
        return _tensor_index(rslice)
    if isinstance(rslice, (list, tuple, np.ndarray, range)):
        keep = np.ascontiguousarray(rslice, np.uint64)
        return _IndexArg(_p(keep), len(keep), len(keep), keep)
    if rslice is None or rslice == slice(None):
        return _IndexArg(_capi.all_indices(), 0, None, None)
    start = 0 if rslice.start is None else rslice.start
    stop = stop_val if rslice.stop is None else rslice.stop
    step = rslice.step
    if step is None:
        keep, ni, size = np.array([start, stop], np.uint64), _capi.constants["GxB_RANGE"], stop - start + 1
    elif step < 0:
        keep, ni, size = np.array([start, stop, -step], np.uint64), _capi.constants["GxB_BACKWARDS"], (0 if start < stop else (start - stop) // -step + 1)
    else:
        keep, ni, size = np.array([start, stop, step], np.uint64), _capi.constants["GxB_STRIDE"], (0 if start > stop or step == 0 else (stop - start) // step + 1)
    return _IndexArg(_p(keep), ni, size, keep)


def _types_by_dtype_name():
    """dtype name ("float64", "bool", ...: numpy's and torch's names agree) -> the GraphBLAS type stored as that dtype: the map `from_tensors` reads forwards and
    `to_tensors` backwards."""
    return {str(np.dtype(t._np)): t for t in (types.BOOL, types.INT8, types.UINT8, types.INT16, types.UINT16, types.INT32, types.UINT32, types.INT64,
                                              types.UINT64, types.FP32, types.FP64)}


def _torch_dtype(typ):
    """The torch dtype of a type's values (the reverse of _types_by_dtype_name); TypeError for a type without one in the installed torch."""
    import torch
    for name, t in _types_by_dtype_name().items():
        if t is typ:
            dt = getattr(torch, name, None)
            if isinstance(dt, torch.dtype):
                return dt
            raise TypeError(f"the installed torch has no dtype {name}: no tensors for a {typ.__name__} container")
    raise TypeError(f"no torch dtype for a {typ.__name__} container")


def _tensor_target():
    """(torch device, location) of the tensors `to_tensors` returns: the library's GPU (GRB_MI355X_DEVICE, else LOCAL_RANK modulo the device count, else 0 — what
    GrB_init selects) filled through location 1, or the CPU through location 0 when there is no device."""
    import os
    import torch
    if not (_capi.device_info()["ok"] and torch.cuda.is_available()):
        return torch.device("cpu"), 0
    dev = os.environ.get("GRB_MI355X_DEVICE")
    rank = os.environ.get("LOCAL_RANK")
    index = int(dev) if dev else int(rank) % torch.cuda.device_count() if rank else 0
    return torch.device("cuda", index), 1


def _tensor_ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _tensor_tuples(typ, indices, V):
    """(type, [index pointers..., value pointer], n, location) of the torch tensors of a `from_tensors` call: all on one device, contiguous, int64 indices
    (non-negative: read as the 64-bit unsigned indices of the C ABI), values of the type's dtype.  location 1 = HBM pointers, 0 = host pointers."""
    import torch
    by_dtype = _types_by_dtype_name()
    name = str(V.dtype).replace("torch.", "")
    if typ is None:
        if name not in by_dtype:
            raise TypeError(f"no GraphBLAS type for tensors of dtype {V.dtype}")
        typ = by_dtype[name]
    if name != str(np.dtype(typ._np)):
        raise TypeError(f"values of dtype {V.dtype} for a {typ.__name__} container: from_tensors does not cast (use V.to(...) first)")
    n = int(V.numel())
    for t in tuple(indices) + (V,):
        if t.device != V.device or not t.is_contiguous() or t.dim() != 1 or int(t.numel()) != n:
            raise ValueError("from_tensors takes contiguous one-dimensional tensors of one length on one device")
    for t in indices:
        if t.dtype != torch.int64:
            raise TypeError("from_tensors takes int64 index tensors")
    on_gpu = V.device.type == "cuda"
    if on_gpu:
        torch.cuda.current_stream(V.device).synchronize()      # whatever produced the tensors has finished before the library's stream reads them
    return typ, [C.c_void_p(t.data_ptr()) for t in tuple(indices) + (V,)], n, 1 if on_gpu else 0


_diag_min = None


def _diag_matrix_min_entries():
    """Entries from which `GxB_Matrix_diag` takes its device route (the library's own number: GrBX_diag_thresholds); infinite without a device."""
    global _diag_min
    if _diag_min is None:
        a, b = u64(0), u64(0)
        check(lib.GrBX_diag_thresholds(C.byref(a), C.byref(b)))
        _diag_min = a.value if _capi.device_info()["ok"] else float("inf")
    return _diag_min


class Matrix:
    _kind = "matrix"

    def __init__(self, handle, typ=None):
        self._h = handle  # ctypes c_void_p owning a GrB_Matrix
        if typ is None:
            t = C.c_void_p()
            check(lib.GxB_Matrix_type(C.byref(t), self._h))
            typ = types.type_of_handle(t.value)
        self.type = typ

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and lib is not None:
            lib.GrB_Matrix_free(C.byref(h))

    # ---- construction ---------------------------------------------------------------------------------
    @classmethod
    def sparse(cls, typ, nrows=None, ncols=None, fill=None, mask=None):
        """An empty matrix; with `mask`, one that holds `fill` (default: the type's zero) where the mask is true — `fill` without a mask is ignored
        (reference: matrix.py:120-181)."""
        imax = _capi.constants["GxB_INDEX_MAX"]
        h = C.c_void_p()
        check(lib.GrB_Matrix_new(C.byref(h), C.c_void_p(typ._h), u64(imax if nrows is None else nrows),
                                 u64(imax if ncols is None else ncols)))
        m = cls(h, typ)
        if mask is not None:
            m.assign_scalar(typ.default_zero if fill is None else fill, mask=mask)
        return m

    @classmethod
    def dense(cls, typ, nrows, ncols, fill=None):
        if fill is None:
            fill = typ.default_zero
        if 0 < nrows * ncols < (1 << 32) - 16 and _capi.device_info()["ok"]:  # one fill kernel in HBM (the ns x n batches of the BC sweeps): the
            m = cls.sparse(typ, nrows, ncols)                                  # reference's own `m[:, :] = fill` (pygraphblas/matrix.py:220-230)
            ALL = _capi.all_indices()
            check(getattr(lib, "GrB_Matrix_assign_" + typ.__name__)(m._h, None, None, typ._c(fill), ALL, u64(nrows), ALL, u64(ncols), None), m)
            return m
        I, J = np.divmod(np.arange(nrows * ncols, dtype=np.uint64), np.uint64(ncols))
        return cls.from_arrays(I, J, np.full(nrows * ncols, fill, dtype=typ._np), nrows, ncols, typ)

    @classmethod
    def from_lists(cls, I, J, V=None, nrows=None, ncols=None, typ=None):
        """Build from coordinate lists; the type is inferred from V[0] when not given."""
        if V is None:
            V = [True] * len(I)
        elif not hasattr(V, "__len__"):
            V = [V] * len(I)
        if typ is None:
            typ = types.from_python_value(V[0])
        if nrows is None:
            nrows = max(I) + 1
        if ncols is None:
            ncols = max(J) + 1
        return cls.from_arrays(np.asarray(I, np.uint64), np.asarray(J, np.uint64), np.asarray(V, typ._np), nrows, ncols, typ)

    @classmethod
    def from_arrays(cls, I, J, V, nrows, ncols, typ, dup=None):
        """Bulk build through GrB_Matrix_build_<T> (duplicates combined with `dup`, default: error)."""
        m = cls.sparse(typ, nrows, ncols)
        I = np.ascontiguousarray(I, np.uint64); J = np.ascontiguousarray(J, np.uint64); V = np.ascontiguousarray(V, typ._np)
        fn = getattr(lib, "GrB_Matrix_build_" + typ.__name__)
        check(fn(m._h, _p(I), _p(J), _p(V), u64(len(I)), C.c_void_p(dup.get_op()) if dup is not None else None), m)
        return m

    @classmethod
    def from_tensors(cls, I, J, V, nrows, ncols, typ=None, dup=None):
        """Bulk build from contiguous torch tensors (int64 indices, V of the type's dtype) through GrBX_Matrix_build_at.  Tensors that live on the GPU are read where
        they are: on the device route (large builds, see GrBX_build_thresholds) the tuples never visit the host.  CPU tensors are host arrays, as in from_arrays."""
        typ, args, n, location = _tensor_tuples(typ, (I, J), V)
        m = cls.sparse(typ, nrows, ncols)
        check(lib.GrBX_Matrix_build_at(m._h, args[0], args[1], args[2], u64(n), C.c_void_p(dup.get_op()) if dup is not None else None, location), m)
        return m

    @classmethod
    def from_dense(cls, X, typ=None):
        """The FULL matrix whose entries are the 2-D array `X` (a numpy array, or a torch tensor on the CPU or on the library's GPU: read where it is), through
        GrBX_Matrix_import_Full: one copy of the values and one fill kernel for the closed-form pattern, no tuples.  The type comes from the dtype when not given;
        a numpy array of another dtype is cast, a tensor is not (use X.to(...) first).  `A.mxm(Matrix.from_dense(H))` is the product with a full operand."""
        by_dtype = _types_by_dtype_name()
        tensor = not isinstance(X, np.ndarray) and hasattr(X, "data_ptr")
        if not tensor:
            X = np.asarray(X)
        if len(X.shape) != 2:
            raise ValueError("from_dense takes a two-dimensional array")
        name = str(X.dtype).replace("torch.", "")
        if typ is None:
            if name not in by_dtype:
                raise TypeError(f"no GraphBLAS type for an array of dtype {X.dtype}")
            typ = by_dtype[name]
        location = 0
        if tensor:
            if name != str(np.dtype(typ._np)):
                raise TypeError(f"values of dtype {X.dtype} for a {typ.__name__} container: from_dense does not cast a tensor (use X.to(...) first)")
            X = X.contiguous()
            if X.device.type == "cuda":
                import torch
                torch.cuda.current_stream(X.device).synchronize()      # whatever produced the tensor has finished before the library's stream reads it
                location = 1
            ptr = _tensor_ptr(X)
        else:
            X = np.ascontiguousarray(X, typ._np)
            ptr = _p(X)
        h = C.c_void_p()
        check(lib.GrBX_Matrix_import_Full(C.byref(h), C.c_void_p(typ._h), u64(X.shape[0]), u64(X.shape[1]), ptr, C.c_int(location)))
        return cls(h, typ)

    # ---- text formats: one numpy parse + one bulk build instead of one setElement per entry -------------
    @staticmethod
    def _read_triples(path, skip, delimiter=None):
        """(I, J, V-or-None) of a whitespace / delimiter separated coordinate file as numpy columns."""
        try:
            import pandas as pd
            df = pd.read_csv(path, sep=delimiter if delimiter is not None else r"\s+", header=None, skiprows=skip, comment="%", engine="c" if delimiter else "python")
            cols = [df[c].to_numpy() for c in df.columns]
        except ImportError:                                    # pragma: no cover
            a = np.loadtxt(path, skiprows=skip, comments="%", delimiter=delimiter, ndmin=2); cols = [a[:, k] for k in range(a.shape[1])]
        if len(cols) > 3:
            raise TypeError("File can contain only 3 columns: row, col and val")
        return cols[0], cols[1], (cols[2] if len(cols) == 3 else None)

    @classmethod
    def from_mm(cls, mm_file, typ=None):
        """Matrix Market coordinate file -> Matrix (reference: pygraphblas/matrix.py:377-409).  The element type comes from
        `typ`, else from a `%%GraphBLAS GrB_<T>` comment line, else from the field of the banner (integer -> INT64, real -> FP64,
        pattern -> BOOL).  Symmetric / skew-symmetric storage is expanded; a repeated coordinate keeps its last value, like
        the reference's element-wise assignment."""
        banner = None; gtype = None; skip = 0
        with open(mm_file) as f:
            for line in f:
                if line.startswith("%%MatrixMarket"): banner = line.split()
                elif line.startswith("%%GraphBLAS"): gtype = line.split()[1]
                if not line.startswith("%"):
                    if line.strip():
                        size = line.split(); break
                skip += 1
            else:
                raise ValueError("Matrix Market file has no size line")
        if banner is None or len(banner) < 5 or banner[1].lower() != "matrix" or banner[2].lower() != "coordinate":
            raise ValueError("only 'matrix coordinate' Matrix Market files are supported")
        field, storage = banner[3].lower(), banner[4].lower()
        if field == "complex" or storage == "hermitian":
            raise TypeError("complex Matrix Market files are not supported (no FC32/FC64 containers)")
        nrows, ncols, nvals = int(size[0]), int(size[1]), int(size[2])
        if typ is None:
            typ = getattr(types, gtype[4:]) if gtype and gtype.startswith("GrB_") and hasattr(types, gtype[4:]) else \
                  {"integer": types.INT64, "real": types.FP64, "double": types.FP64, "pattern": types.BOOL}[field]
        if nvals == 0:
            return cls.sparse(typ, nrows, ncols)
        I, J, V = cls._read_triples(mm_file, skip + 1)
        I = I.astype(np.int64) - 1; J = J.astype(np.int64) - 1
        V = np.ones(len(I), typ._np) if V is None else V.astype(typ._np)
        if storage in ("symmetric", "skew-symmetric"):
            off = I != J
            I, J, V = np.concatenate([I, J[off]]), np.concatenate([J, I[off]]), np.concatenate([V, (-V[off] if storage == "skew-symmetric" else V[off])])
        return cls.from_arrays(I.astype(np.uint64), J.astype(np.uint64), V, nrows, ncols, typ, dup=typ.SECOND)

    @classmethod
    def from_csv(cls, csv_file, typ, nrows, ncols, one_based=True, delimiter=","):
        """`row<delimiter>col<delimiter>value` lines -> Matrix (reference: pygraphblas/matrix.py:428-479)."""
        I, J, V = cls._read_triples(csv_file, 0, delimiter)
        if V is None:
            raise TypeError("File must contain 3 columns: row, col and val")
        I = I.astype(np.int64) - (1 if one_based else 0); J = J.astype(np.int64) - (1 if one_based else 0)
        return cls.from_arrays(I.astype(np.uint64), J.astype(np.uint64), V.astype(typ._np), nrows, ncols, typ, dup=typ.SECOND)

    @classmethod
    def from_tsv(cls, tsv_file, typ, nrows, ncols, one_based=True):
        """Tab separated triples (reference: pygraphblas/matrix.py:411-426)."""
        return cls.from_csv(tsv_file, typ, nrows, ncols, one_based=one_based, delimiter="\t")

    # ---- the SuiteSparse / LAGraph ".grb" binary format (gap/prmark.py:42-48 and gap/bcmark.py:77-83 load nothing else) ----------
    # Layout (little endian), as written by the third-party suitesparse_graphblas.io.binary.binwrite the reference calls
    # (pygraphblas/matrix.py:489-497, 935-942; that package is absent from /root/reference — the layout below is pinned to the
    # reference's own fixture docs/test_binfile.grb, whose 1021 bytes it accounts for exactly):
    #   512-byte space-padded ASCII header ("SuiteSparse:GraphBLAS matrix\nv... (LAGraph DRAFT)\nnrows: ...type: GrB_<T> ...")
    #   int32 format (0 by row, 1 by column) | int32 sparsity (1 hypersparse, 2 sparse, 4 bitmap, 8 full) | f64 hyper_switch
    #   u64 nrows | u64 ncols | i64 nonempty | u64 nvec | u64 nvals | int32 typecode | u64 typesize
    #   hypersparse: Ap u64[nvec+1], Ah u64[nvec], Ai u64[nvals], Ax | sparse: Ap u64[nvec+1], Ai u64[nvals], Ax
    #   bitmap: Ab i8[nrows*ncols], Ax T[nrows*ncols] | full: Ax T[nrows*ncols]
    _GRB_TYPECODES = ["BOOL", "INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64", "FP32", "FP64"]

    @classmethod
    def binread(cls, bin_file, opener=None):
        """Read a SuiteSparse binary (.grb) file: one numpy parse and one bulk build."""
        import struct
        if opener is not None:
            with opener(bin_file, "rb") as f:
                raw = f.read()
        else:
            with open(bin_file, "rb") as f:
                raw = f.read()
        if len(raw) < 512 + 68 or not raw.startswith(b"SuiteSparse:GraphBLAS matrix"):
            raise ValueError("not a SuiteSparse:GraphBLAS binary matrix file")
        fmt, kind, _hs, nrows, ncols, _nonempty, nvec, nvals, tcode, tsize = struct.unpack_from("<iidQQqQQiQ", raw, 512)
        if not 0 <= tcode < len(cls._GRB_TYPECODES):
            raise TypeError(f"type code {tcode} of the file is not supported (complex / user-defined types have no containers here)")
        typ = getattr(types, cls._GRB_TYPECODES[tcode])
        if np.dtype(typ._np).itemsize != tsize:
            raise ValueError("type size in the file does not match its type code")
        pos = 512 + 68

        def take(dtype, count):
            nonlocal pos
            nbytes = np.dtype(dtype).itemsize * count
            if pos + nbytes > len(raw):
                raise ValueError("truncated .grb file")
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=pos); pos += nbytes
            return a
        nmajor, nminor = (nrows, ncols) if fmt == 0 else (ncols, nrows)
        if kind in (1, 2):                                   # (hyper)sparse: compressed vectors
            Ap = take("<u8", nvec + 1)
            Ah = take("<u8", nvec) if kind == 1 else np.arange(nvec, dtype=np.uint64)
            Ai = take("<u8", nvals); Ax = take(np.dtype(typ._np).newbyteorder("<"), nvals)
            major = np.repeat(Ah, np.diff(Ap.astype(np.int64))); minor = Ai
        elif kind in (4, 8):                                 # bitmap / full: dense vectors
            Ab = take("i1", nmajor * nminor) if kind == 4 else np.ones(nmajor * nminor, np.int8)
            Ax = take(np.dtype(typ._np).newbyteorder("<"), nmajor * nminor)
            flat = np.flatnonzero(Ab).astype(np.uint64)
            major, minor = np.divmod(flat, np.uint64(max(nminor, 1))); Ax = Ax[flat.astype(np.int64)]
        else:
            raise ValueError(f"unknown sparsity code {kind} in .grb file")
        if len(major) != nvals:
            raise ValueError(".grb file: entry count does not match its header")
        I, J = (major, minor) if fmt == 0 else (minor, major)
        return cls.from_arrays(I.astype(np.uint64), J.astype(np.uint64), np.ascontiguousarray(Ax, typ._np), nrows, ncols, typ)

    from_binfile = binread

    def binwrite(self, filename, comments="", opener=None):
        """Write the matrix in the same format (sparse, by row) — what `to_binfile` produces for the gap/ drivers' cache."""
        import struct
        I, ci, av = self.to_arrays()                               # sorted by (row, column)
        typ = self.type; nrows, ncols, nvals = self.nrows, self.ncols, len(ci)
        rp = np.zeros(nrows + 1, np.uint64); np.cumsum(np.bincount(I.astype(np.int64), minlength=nrows), out=rp[1:])
        head = (f"SuiteSparse:GraphBLAS matrix\nv4.0.1 (LAGraph DRAFT)\nnrows:  {nrows}\nncols:  {ncols}\nnvec:   {nrows}\nnvals:  {nvals}\n"
                f"format: SPARSER\nsize:   {np.dtype(typ._np).itemsize}\ntype:   GrB_{typ.__name__}\n{comments}\n").encode()
        if len(head) > 511:
            raise ValueError("comments too long for the 512-byte header")
        blob = head.ljust(511, b" ") + b"\0"
        blob += struct.pack("<iidQQqQQiQ", 0, 2, 0.0625, nrows, ncols, -1, nrows, nvals, self._GRB_TYPECODES.index(typ.__name__), np.dtype(typ._np).itemsize)
        blob += rp.astype("<u8").tobytes() + ci.astype("<u8").tobytes() + np.ascontiguousarray(av, typ._np).tobytes()
        if opener is not None:
            with opener(filename, "wb") as f:
                f.write(blob)
        else:
            with open(filename, "wb") as f:
                f.write(blob)

    to_binfile = binwrite

    @classmethod
    def from_csr(cls, typ, nrows, ncols, rowptr, colidx, values, device=False):
        """Import CSR arrays (u32 rowptr/colidx).  `device=True`: the arguments are raw HBM addresses (ints)."""
        h = C.c_void_p()
        if device:
            rp, ci, vv, nvals = C.c_void_p(rowptr), C.c_void_p(colidx), C.c_void_p(values[0]), values[1]
        else:
            rowptr = np.ascontiguousarray(rowptr, np.uint32); colidx = np.ascontiguousarray(colidx, np.uint32)
            values = np.ascontiguousarray(values, typ._np)
            rp, ci, vv, nvals = _p(rowptr), _p(colidx), _p(values), len(colidx)
        check(lib.GrBX_Matrix_import_CSR(C.byref(h), C.c_void_p(typ._h), u64(nrows), u64(ncols), u64(nvals), rp, ci, vv,
                                         C.c_int(1 if device else 0)))
        return cls(h, typ)

    @classmethod
    def from_scipy_sparse(cls, m, typ=None):
        m = m.tocsr(); m.sort_indices()
        typ = typ or {np.dtype(np.float64): types.FP64, np.dtype(np.float32): types.FP32, np.dtype(np.int64): types.INT64,
                      np.dtype(np.int32): types.INT32, np.dtype(np.bool_): types.BOOL}[m.dtype]
        return cls.from_csr(typ, m.shape[0], m.shape[1], m.indptr, m.indices, m.data)

    @classmethod
    def identity(cls, typ, nrows, one=None):
        one = typ.default_one if one is None else one
        if nrows >= _diag_matrix_min_entries():               # a fill and the all-present path of from_diag in HBM: no tuples on the host
            from .vector import Vector
            return cls.from_diag(Vector.dense(typ, nrows, fill=one))
        idx = np.arange(nrows, dtype=np.uint64)
        return cls.from_arrays(idx, idx, np.full(nrows, one, typ._np), nrows, nrows, typ)

    @classmethod
    def random(cls, typ, nvals, nrows=None, ncols=None, make_pattern=False, make_symmetric=False, make_skew_symmetric=False,
               make_hermitian=True, no_diagonal=False, seed=None):
        """The reference's generator, call for call (pygraphblas/matrix.py:499-571): Python's `random`, seeded if asked;
        per entry `randint(0, nrows-1)`, `randint(0, ncols-1)`, then the value draw of the type (signed integers
        from -(2^(b-1))+1, floats from `random()`); a repeated coordinate overwrites, so nvals is an upper bound.
        The make_* / no_diagonal flags are accepted and — as in the reference's loop (:567-570) — do not change
        what is generated.  `Matrix.random(INT8, 4, 10, 10, seed=42)` holds [62, 46, -70, 24]
        (reference tests/test_matrix.py:1060-1064)."""
        nrows = _capi.constants["GxB_INDEX_MAX"] if nrows is None else nrows
        ncols = _capi.constants["GxB_INDEX_MAX"] if ncols is None else ncols
        m = cls.sparse(typ, nrows, ncols)
        if seed is not None:
            _random.seed(seed)
        if nrows == 0 or ncols == 0:
            nvals = 0
        if typ is types.BOOL:
            f = partial(_random.randint, 0, 1)
        elif typ in (types.FP32, types.FP64):
            f = _random.random
        else:
            info = np.iinfo(typ._np)
            f = partial(_random.randint, 0 if info.min == 0 else int(info.min) + 1, int(info.max))
        for _ in range(nvals):
            i = _random.randint(0, nrows - 1)
            j = _random.randint(0, ncols - 1)
            m[i, j] = f()
        return m

    def dup(self):
        h = C.c_void_p()
        check(lib.GrB_Matrix_dup(C.byref(h), self._h), self)
        return Matrix(h, self.type)

    # ---- properties -----------------------------------------------------------------------------------
    def _index(self, fn):
        n = u64()
        check(fn(C.byref(n), self._h), self)
        return n.value

    @property
    def nrows(self):
        return self._index(lib.GrB_Matrix_nrows)

    @property
    def ncols(self):
        return self._index(lib.GrB_Matrix_ncols)

    @property
    def shape(self):
        return (self.nrows, self.ncols)

    @property
    def nvals(self):
        return self._index(lib.GrB_Matrix_nvals)

    @property
    def T(self):
        return self.transpose()

    def __len__(self):
        return self.nvals

    def clear(self):
        check(lib.GrB_Matrix_clear(self._h), self)

    def wait(self):
        check(lib.GrB_Matrix_wait(C.byref(self._h)), self)

    def resize(self, nrows=_capi.constants["GxB_INDEX_MAX"], ncols=_capi.constants["GxB_INDEX_MAX"]):
        """Resize the matrix; entries that fall outside the new dimensions are deleted (reference: matrix.py:978-1001).  A matrix that lives in HBM
        is resized there (grb_edit.hip) unless a new dimension is beyond the device range."""
        check(lib.GrB_Matrix_resize(self._h, u64(nrows), u64(ncols)), self)

    # ---- element access ---------------------------------------------------------------------------------
    def to_arrays(self):
        n = self.nvals
        I, J, X = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, self.type._np)
        nn = u64(n)
        fn = getattr(lib, "GrB_Matrix_extractTuples_" + self.type.__name__)
        check(fn(_p(I), _p(J), _p(X), C.byref(nn), self._h), self)
        return I, J, X

    def to_lists(self):
        I, J, X = self.to_arrays()
        return [I.tolist(), J.tolist(), X.tolist()]

    def to_tensors(self, values=True):
        """(I, J, V) — `values=False`: (I, J) — as contiguous torch tensors on the library's GPU: int64 indices, V of the type's dtype, row-major with ascending
        columns inside a row, bit for bit what to_arrays returns.  Filled in HBM through GrBX_Matrix_extractTuples_at (grb_tuples.hip): a matrix that lives there
        is expanded where it is and no host mirror is built.  Without a GPU: CPU tensors.  `Matrix.from_tensors(*A.to_tensors(), nrows, ncols)` reproduces A."""
        import torch
        vdt = _torch_dtype(self.type) if values else None
        dev, location = _tensor_target()
        n = self.nvals
        I, J = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
        V = torch.empty(n, dtype=vdt, device=dev) if values else None
        if n:
            if location:
                torch.cuda.current_stream(dev).synchronize()
            nn = u64(n)
            check(lib.GrBX_Matrix_extractTuples_at(_tensor_ptr(I), _tensor_ptr(J), _tensor_ptr(V), C.byref(nn), self._h, C.c_int(location)), self)
        return (I, J, V) if values else (I, J)

    def to_csr(self):
        n = self.nvals
        rp, ci, x = np.zeros(self.nrows + 1, np.uint32), np.zeros(n, np.uint32), np.zeros(n, self.type._np)
        check(lib.GrBX_Matrix_export_CSR(self._h, _p(rp), _p(ci), _p(x), C.c_int(0)), self)
        return rp, ci, x

    def to_csr_tensors(self):
        """(rowptr, colidx, values) as torch tensors on the library's GPU — the library's own CSR layout, copied in HBM by GrBX_Matrix_export_CSR(..., 1): int32
        row pointers and columns (the bits of the unsigned 32-bit words), values of the type's dtype.  Like to_csr it needs a device: the CSR is the HBM layout."""
        import torch
        vdt = _torch_dtype(self.type)
        dev, location = _tensor_target()
        n = self.nvals
        rp, ci = torch.empty(self.nrows + 1, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        x = torch.empty(n, dtype=vdt, device=dev)
        if location:
            torch.cuda.current_stream(dev).synchronize()
        check(lib.GrBX_Matrix_export_CSR(self._h, _tensor_ptr(rp), _tensor_ptr(ci), _tensor_ptr(x), C.c_int(location)), self)
        return rp, ci, x

    @property
    def is_full(self):
        """Every position holds an entry: what makes the matrix a full operand of `mxm` (and what `to_dense_tensor` needs)."""
        return self.nvals == self.nrows * self.ncols

    def to_dense_tensor(self):
        """The values of a FULL matrix as a (nrows, ncols) torch tensor of the type's dtype on the library's GPU (CPU without one): one copy of the value array
        through GrBX_Matrix_export_Full.  A matrix with a position that holds no entry raises InvalidValue."""
        import torch
        if not self.is_full:
            check(lib.GrBX_Matrix_export_Full(self._h, None, C.c_int(0)), self)      # (the library's own refusal, before anything of that shape is allocated)
        vdt = _torch_dtype(self.type)
        dev, location = _tensor_target()
        out = torch.empty((self.nrows, self.ncols), dtype=vdt, device=dev)
        if location:
            torch.cuda.current_stream(dev).synchronize()
        check(lib.GrBX_Matrix_export_Full(self._h, _tensor_ptr(out), C.c_int(location)), self)
        return out

    def to_scipy_sparse(self):
        import scipy.sparse as sp
        rp, ci, x = self.to_csr()
        return sp.csr_matrix((x, ci.astype(np.int64), rp.astype(np.int64)), shape=self.shape)

    def __iter__(self):
        I, J, X = self.to_arrays()
        return iter(zip(I.tolist(), J.tolist(), X.tolist()))

    def __setitem__(self, index, value):
        """`M[i, j] = x`, `M[i] = v` / `M[i, :] = v` (row), `M[:, j] = v` (column), `M[I, J] = A` (sub-matrix), `M[Mask] = A` (masked), and a scalar
        in place of the vector or matrix: `M[i] = s`, `M[a:b] = s`, `M[i, J] = s`, `M[I, j] = s`, `M[I, J] = s`, `M[Mask] = s` — reference: matrix.py:3236-3330."""
        from .vector import Vector
        scalar = isinstance(value, (bool, int, float, complex, np.generic))
        if isinstance(index, int):
            return self.assign_scalar(value, index) if scalar else self.assign_row(index, value)
        if isinstance(index, slice):
            return self.assign_scalar(value, index, None) if scalar else self.assign_matrix(value, index, None)
        if isinstance(index, Matrix):
            if isinstance(value, Matrix):
                return self.assign_matrix(value, mask=index)
            if not scalar:
                raise TypeError("a masked assignment takes a matrix or a scalar")
            return self.assign_scalar(value, mask=index)
        i, j = index
        if isinstance(i, int) and isinstance(j, int):
            fn = getattr(lib, "GrB_Matrix_setElement_" + self.type.__name__)
            check(fn(self._h, self.type._c(value), u64(i), u64(j)), self)
        elif isinstance(i, int) and isinstance(value, Vector):
            self.assign_row(i, value, j)
        elif isinstance(j, int) and isinstance(value, Vector):
            self.assign_col(j, value, i)
        elif isinstance(value, Matrix):
            self.assign_matrix(value, i, j)
        elif scalar:
            self.assign_scalar(value, i, j)
        else:
            raise TypeError("unsupported index / value combination")

    def __getitem__(self, index):
        """`M[i, j]` (element), `M[i]` / `M[i, :]` (row vector), `M[:, j]` (column vector), `M[a:b, c:d]` / `M[[..], [..]]` (sub-matrix;
        slices include their stop, as in the reference: matrix.py:2967-3003)."""
        if isinstance(index, int):
            return self.extract_row(index)
        if isinstance(index, slice):
            return self.extract_matrix(index, None)
        i, j = index
        if isinstance(i, int) and isinstance(j, int):
            out = self.type._c()
            fn = getattr(lib, "GrB_Matrix_extractElement_" + self.type.__name__)
            check(fn(C.byref(out), self._h, u64(i), u64(j)), self)
            return out.value
        if isinstance(i, int):
            return self.extract_row(i, j)
        if isinstance(j, int):
            return self.extract_col(j, i)
        return self.extract_matrix(i, j)

    # ---- slices (grb_extract_ops.cpp, grb_assign_ops.cpp: extract and assign run in HBM for device-resident or large containers, grb_extract.hip / grb_assign.hip; small host-resident ones on the host mirror) ----
    def extract_matrix(self, row_index=None, col_index=None, out=None, mask=None, accum=None, desc=None):
        """`out<mask> = accum(out, op(self)(I, J))` (reference: matrix.py:2807-2900)."""
        t0 = desc is not None and _d.T0 in desc
        nr, nc = (self.ncols, self.nrows) if t0 else (self.nrows, self.ncols)
        from .vector import Vector
        both = all(x is None or isinstance(x, Vector) for x in (row_index, col_index))      # vectors (or all) on both sides: GrBX_Matrix_extract_Vector; mixed: the vector's values as a tensor
        ri = build_range(row_index, nr - 1, vector_ok=both); ci = build_range(col_index, nc - 1, vector_ok=both)
        (I, ni, isz, k1), (J, nj, jsz, k2) = ri, ci
        if out is None:
            out = Matrix.sparse(self.type, nr if isz is None else isz, nc if jsz is None else jsz)
        mh, ah, dh = get_args(mask, accum, desc)
        if ri.vector is not None or ci.vector is not None:
            check(lib.GrBX_Matrix_extract_Vector(out._h, mh, ah, self._h, ri.vector._h if ri.vector is not None else None, ci.vector._h if ci.vector is not None else None, dh), out)
        elif ri.location or ci.location:
            check(lib.GrBX_Matrix_extract_at(out._h, mh, ah, self._h, I, u64(ni), J, u64(nj), dh, C.c_int(ri.location), C.c_int(ci.location)), out)
        else:
            check(lib.GrB_Matrix_extract(out._h, mh, ah, self._h, I, u64(ni), J, u64(nj), dh), out)
        return out

    def extract_col(self, col_index, row_slice=None, out=None, mask=None, accum=None, desc=None):
        """Column `col_index` of op(self) as a vector (reference: matrix.py:2902-2941)."""
        from .vector import Vector
        t0 = desc is not None and _d.T0 in desc
        length = self.ncols if t0 else self.nrows
        ix = build_range(row_slice, length - 1); I, ni, size, keep = ix
        if out is None:
            out = Vector.sparse(self.type, length if size is None else size)
        mh, ah, dh = get_args(mask, accum, desc)
        if ix.location:
            check(lib.GrBX_Col_extract_at(out._h, mh, ah, self._h, I, u64(ni), u64(col_index), dh, C.c_int(1)), out)
        else:
            check(lib.GrB_Col_extract(out._h, mh, ah, self._h, I, u64(ni), u64(col_index), dh), out)
        return out

    def extract_row(self, row_index, col_slice=None, out=None, mask=None, accum=None, desc=None):
        """Row `row_index` as a vector: the column of the transpose (reference: matrix.py:2943-2965)."""
        return self.extract_col(row_index, col_slice, out, mask, accum, (desc & _d.T0) if desc is not None else _d.T0)

    def assign_col(self, col_index, value, row_slice=None, mask=None, accum=None, desc=None):
        """`self(I, j)<mask> = accum(self(I, j), value)` (reference: matrix.py:3005-3029)."""
        ix = build_range(row_slice, self.nrows - 1); I, ni, size, keep = ix
        mh, ah, dh = get_args(mask, accum, desc)
        if ix.location:
            check(lib.GrBX_Col_assign_at(self._h, mh, ah, value._h, I, u64(ni), u64(col_index), dh, C.c_int(1)), self)
        else:
            check(lib.GrB_Col_assign(self._h, mh, ah, value._h, I, u64(ni), u64(col_index), dh), self)

    def assign_row(self, row_index, value, col_slice=None, mask=None, accum=None, desc=None):
        """`self(i, J)<mask> = accum(self(i, J), value)` (reference: matrix.py:3031-3055)."""
        jx = build_range(col_slice, self.ncols - 1); J, nj, size, keep = jx
        mh, ah, dh = get_args(mask, accum, desc)
        if jx.location:
            check(lib.GrBX_Row_assign_at(self._h, mh, ah, value._h, u64(row_index), J, u64(nj), dh, C.c_int(1)), self)
        else:
            check(lib.GrB_Row_assign(self._h, mh, ah, value._h, u64(row_index), J, u64(nj), dh), self)

    @classmethod
    def from_diag(cls, v, k=0):
        """The matrix with `v` on its k-th diagonal (reference: matrix.py:333-375)."""
        n = v.size + abs(k)
        out = cls.sparse(v.type, n, n)
        check(lib.GxB_Matrix_diag(out._h, v._h, C.c_int64(k), None), out)
        return out

    def vector_diag(self, k=0):
        """The k-th diagonal as a vector (reference: matrix.py:2225-2277)."""
        from .vector import Vector
        m, n = self.nrows, self.ncols
        length = min(m, n - k) if 0 <= k < n else (min(m + k, n) if -m < k < 0 else 0)
        out = Vector.sparse(self.type, length)
        check(lib.GxB_Vector_diag(out._h, self._h, C.c_int64(k), None), out)
        return out

    def sort(self, op=None, desc=None, values=True, perm=True):
        """`GxB_Matrix_sort`: `(C, P)` — row i of C holds the values of row i in sorted order at columns 0 .. len - 1, P (INT64) the column each came from;
        under a descriptor with the first input transposed the columns are sorted (`C[k, j]` is the k-th value of column j, `P[k, j]` its row).  `op` is the
        type's `LT` (ascending, the default) or `GT`; ties keep the smaller index first and NaNs come last under both.  The part not asked for is None."""
        if op is None:
            op = self.type.LT
        Cm = Matrix.sparse(self.type, self.nrows, self.ncols) if values else None
        Pm = Matrix.sparse(types.INT64, self.nrows, self.ncols) if perm else None
        _, _, dh = get_args(None, None, desc)
        check(lib.GxB_Matrix_sort(Cm._h if values else None, Pm._h if perm else None, C.c_void_p(op.get_op()), self._h, dh), Cm if values else Pm)
        return Cm, Pm

    def topk(self, k, largest=True, desc=None):
        """`GrBX_Matrix_select_topk`: the k largest (`largest=False`: smallest) entries of every row, at their own coordinates — of every column under a
        descriptor with the first input transposed.  Among equal values the smaller index is kept."""
        out = Matrix.sparse(self.type, self.nrows, self.ncols)
        op = self.type.GT if largest else self.type.LT
        _, _, dh = get_args(None, None, desc)
        check(lib.GrBX_Matrix_select_topk(out._h, C.c_void_p(op.get_op()), self._h, C.c_uint64(k), dh), out)
        return out

    # ---- tiles (grb_tile_ops.cpp: in HBM for device-resident or large operands, grb_tile.hip; small host-resident ones on the host mirror) ----
    @classmethod
    def concat(cls, tiles, typ=None):
        """`GxB_Matrix_concat`: the matrix made of the grid `tiles` (a list of rows, each a list of matrices): tiles of one grid row share their height, tiles
        of one grid column their width; values are typecast to `typ` (default: the first tile's type).  The same matrix may stand at several positions."""
        m = len(tiles); n = len(tiles[0]) if m else 0
        if any(len(row) != n for row in tiles):
            raise ValueError("concat: every row of the grid holds the same number of tiles")
        if typ is None:
            typ = tiles[0][0].type if m and n else types.BOOL
        out = cls.sparse(typ, sum(row[0].nrows for row in tiles) if n else 0, sum(t.ncols for t in tiles[0]) if m else 0)
        handles = (C.c_void_p * max(m * n, 1))(*[t._h.value for row in tiles for t in row])
        check(lib.GxB_Matrix_concat(out._h, handles, u64(m), u64(n), None), out)
        return out

    def split(self, row_sizes, col_sizes):
        """`GxB_Matrix_split`: the grid of tiles (a list of rows) that `row_sizes` x `col_sizes` cut this matrix into; the sizes add up to its shape and none
        is 0.  `Matrix.concat(A.split(r, c))` is A again."""
        m, n = len(row_sizes), len(col_sizes)
        handles = (C.c_void_p * max(m * n, 1))()
        rs, cs = (u64 * max(m, 1))(*row_sizes), (u64 * max(n, 1))(*col_sizes)
        check(lib.GxB_Matrix_split(handles, u64(m), u64(n), rs, cs, self._h, None), self)
        return [[Matrix(C.c_void_p(handles[a * n + b]), self.type) for b in range(n)] for a in range(m)]

    @classmethod
    def hstack(cls, tiles, typ=None):
        return cls.concat([list(tiles)], typ)

    @classmethod
    def vstack(cls, tiles, typ=None):
        return cls.concat([[t] for t in tiles], typ)

    def kronecker(self, other, op=None, cast=None, out=None, mask=None, accum=None, desc=None):
        """Kronecker product (reference: matrix.py:2728-2805)."""
        if op is None:
            op = current_binop.get(None) or types.promote(self.type, other.type)._default_multop()
        if out is None:
            out = Matrix.sparse(cast or types.promote(self.type, other.type), self.nrows * other.nrows, self.ncols * other.ncols)
        mh, ah, dh = get_args(mask, accum, desc)
        check(lib.GrB_Matrix_kronecker_BinaryOp(out._h, mh, ah, C.c_void_p(op.get_op()), self._h, other._h, dh), out)
        return out

    def kronpow(self, exponent):
        """"Kronecker power": 0 gives the identity of the matrix's type, 1 the matrix itself, otherwise a copy is replaced by its
        Kronecker product with itself `exponent - 1` times — the reference's loop as it stands (matrix.py:1732-1757), so the
        dimension is nrows ** (2 ** (exponent - 1)).  Each squaring is one pass of the device kernels once the product is large."""
        if exponent == 0:
            return Matrix.identity(self.type, self.nrows)
        if exponent == 1:
            return self
        result = self.dup()
        for _ in range(1, exponent):
            result = result.kronecker(result)
        return result

    def get(self, i, j, default=None):
        try:
            return self[i, j]
        except NoValue:
            return default

    def __delitem__(self, index):
        i, j = index
        check(lib.GrB_Matrix_removeElement(self._h, u64(i), u64(j)), self)

    def __contains__(self, index):
        return self.get(*index) is not None

    # ---- the hot path -------------------------------------------------------------------------------------
    def mxm(self, other, semiring=None, cast=None, out=None, mask=None, accum=None, desc=None):
        """Matrix-matrix multiply `C<mask> = accum(C, self (+).(x) other)`  (reference: matrix.py:2401-2584)."""
        if semiring is None:
            semiring = current_semiring.get(None)
        if out is None:
            if cast is not None:
                typ = cast
            elif semiring is not None:
                typ = semiring.ztype
            else:
                typ = types.promote(self.type, other.type)
            out = Matrix.sparse(typ, self.nrows, other.ncols)
        if semiring is None:
            semiring = out.type._default_semiring()
        mh, ah, dh = get_args(mask, accum, desc)
        check(lib.GrB_mxm(out._h, mh, ah, C.c_void_p(semiring.get_op()), self._h, other._h, dh), out)
        return out

    def sddmm(self, X, Y, semiring=None, out=None, accum=None, structural=True):
        """The sampled dense-dense product on this matrix's pattern: `S<self> = X (+).(x) Y'`, S(i, j) = (+)_l X(i, l) (x) Y(j, l) for the entries (i, j) of `self`
        (m x n), with X m x k and Y n x k — attention / edge scores, link-prediction scores on candidate edges, the residual of a factorisation on the observed
        entries.  Sugar for `X.mxm(Y, semiring, mask=self, out=out, accum=accum, desc=ST1)` (`T1` when `structural` is false: entries of `self` that hold a false
        value are then left out).  With X and Y full (`Matrix.from_dense`) the call takes the one-pass `sddmm` route of GrB_mxm and reads Y as it lies."""
        if semiring is None:
            semiring = current_semiring.get(None)
        if out is None:
            out = Matrix.sparse(semiring.ztype if semiring is not None else types.promote(X.type, Y.type), self.nrows, self.ncols)
        return X.mxm(Y, semiring=semiring, mask=self, out=out, accum=accum, desc=_d.ST1 if structural else _d.T1)

    def mxv(self, other, semiring=None, cast=None, out=None, mask=None, accum=None, desc=None):
        """Matrix-vector multiply `w<mask> = accum(w, self (+).(x) other)`  (reference: matrix.py:2586-2726)."""
        from .vector import Vector
        if semiring is None:
            semiring = current_semiring.get(None)
        if out is None:
            # the reference sizes by ncols whenever *any* explicit descriptor is passed
            # (Descriptor.__contains__ quirk); only a transposing one should
            transposed = desc is not None and _d.T0 in desc
            if cast is not None:
                typ = cast
            elif semiring is not None:
                typ = semiring.ztype
            else:
                typ = types.promote(self.type, other.type)
            out = Vector.sparse(typ, self.ncols if transposed else self.nrows)
        if semiring is None:
            semiring = out.type._default_semiring()
        mh, ah, dh = get_args(mask, accum, desc)
        check(lib.GrB_mxv(out._h, mh, ah, C.c_void_p(semiring.get_op()), self._h, other._h, dh), out)
        return out

    def __matmul__(self, other):
        from .vector import Vector
        if isinstance(other, Matrix):
            return self.mxm(other)
        if isinstance(other, Vector):
            return self.mxv(other)
        raise TypeError("Right argument to @ must be Matrix or Vector.")

    def __imatmul__(self, other):
        return self.mxm(other, out=self)

    def __getattr__(self, name):
        # A.plus_times(B) -> FP64.plus_times(A, B)   (reference: matrix.py:1607-1613)
        if name.startswith("_"):
            raise AttributeError(name)
        typ = self.__dict__.get("type")
        op = getattr(typ, name, None) if typ is not None else None
        if isinstance(op, (types.Semiring, types.BinaryOp)):
            return partial(op, self)
        raise AttributeError(name)

    # ---- reductions -----------------------------------------------------------------------------------------
    def _reduce_scalar(self, suffix, ctype, default_type, mon, accum, desc):
        if mon is None:
            mon = current_monoid.get(getattr(default_type, "LOR_MONOID" if default_type is types.BOOL else "PLUS_MONOID"))
        out = ctype(0)
        _, ah, dh = get_args(None, accum, desc)
        fn = getattr(lib, "GrB_Matrix_reduce_" + suffix)
        check(fn(C.byref(out), ah, C.c_void_p(mon.get_op()), self._h, dh), self)
        return out.value

    def reduce_bool(self, mon=None, accum=None, desc=None):
        return self._reduce_scalar("BOOL", C.c_bool, types.BOOL, mon, accum, desc)

    def reduce_int(self, mon=None, accum=None, desc=None):
        """Reduce to a Python int with INT64.PLUS_MONOID by default (reference: matrix.py:1782-1804)."""
        return self._reduce_scalar("INT64", C.c_int64, types.INT64, mon, accum, desc)

    def reduce_float(self, mon=None, accum=None, desc=None):
        return self._reduce_scalar("FP64", C.c_double, types.FP64, mon, accum, desc)

    def reduce_vector(self, mon=None, out=None, mask=None, accum=None, desc=None):
        from .vector import Vector
        if mon is None:
            mon = current_monoid.get(self.type.PLUS_MONOID if self.type is not types.BOOL else types.BOOL.LOR_MONOID)
        if out is None:
            out = Vector.sparse(self.type, self.nrows)
        mh, ah, dh = get_args(mask, accum, desc)
        check(lib.GrB_Matrix_reduce_Monoid(out._h, mh, ah, C.c_void_p(mon.get_op()), self._h, dh), out)
        return out

    # ---- companions of the hot path -------------------------------------------------------------------------
    def transpose(self, cast=None, out=None, mask=None, accum=None, desc=None):
        """`GrB_transpose`; with desc T0 the input is transposed first, so the result has the matrix's own shape (reference: pygraphblas/matrix.py:1003-1061,
        pinned by tests/test_matrix.py:324-325)."""
        if out is None:
            t0 = desc is not None and _d.T0 in desc
            out = Matrix.sparse(cast or self.type, *((self.nrows, self.ncols) if t0 else (self.ncols, self.nrows)))
        mh, ah, dh = get_args(mask, accum, desc)
        check(lib.GrB_transpose(out._h, mh, ah, self._h, dh), out)
        return out

    def _ewise(self, fn_stem, other, op, cast, out, mask, accum, desc, default):
        if op is None:
            op = current_binop.get(None) or default(types.promote(self.type, other.type))
        if out is None:
            out = Matrix.sparse(cast or types.promote(self.type, other.type), self.nrows, self.ncols)
        kind = {"BinaryOp": "BinaryOp", "Monoid": "Monoid", "Semiring": "Semiring"}[op.kind]
        mh, ah, dh = get_args(mask, accum, desc)
        fn = getattr(lib, f"GrB_Matrix_{fn_stem}_{kind}")
        check(fn(out._h, mh, ah, C.c_void_p(op.get_op()), self._h, other._h, dh), out)
        return out

    def eadd(self, other, add_op=None, cast=None, out=None, mask=None, accum=None, desc=None):
        """Element-wise union (reference: matrix.py:1103-1262)."""
        return self._ewise("eWiseAdd", other, add_op, cast, out, mask, accum, desc, lambda t: t._default_addop())

    def emult(self, other, mult_op=None, cast=None, out=None, mask=None, accum=None, desc=None):
        """Element-wise intersection (reference: matrix.py:1264-1413)."""
        return self._ewise("eWiseMult", other, mult_op, cast, out, mask, accum, desc, lambda t: t._default_multop())

    def eunion(self, other, op, alpha, beta, cast=None, out=None, mask=None, accum=None, desc=None):
        """`GxB_Matrix_eWiseUnion`: on the union of the two patterns `op(A, B)` where both hold an entry, `op(A, beta)` where only `self` does and `op(alpha, B)`
        where only `other` does — `A.eunion(B, T.MINUS, 0, 0)` is A - B, where `eadd` would copy B's lone entries unnegated.  `alpha` / `beta` are Python numbers
        of the promoted type; `op=None` picks the default as `eadd` does; a binary operator only (there are no Monoid / Semiring forms)."""
        typ = types.promote(self.type, other.type)
        if op is None:
            op = current_binop.get(None) or typ._default_addop()
        if op.kind != "BinaryOp":
            raise TypeError("eunion takes a binary operator")
        if out is None:
            out = Matrix.sparse(cast or typ, self.nrows, self.ncols)
        mh, ah, dh = get_args(mask, accum, desc)
        return eunion(lib.GxB_Matrix_eWiseUnion, out, mh, ah, op, self, alpha, other, beta, dh, typ)

    def iseq(self, other, eq_op=None):
        """True when both matrices have the same pattern and equal values (reference: matrix.py:1436-1453)."""
        if self.nrows != other.nrows or self.ncols != other.ncols or self.nvals != other.nvals:
            return False
        if eq_op is None:
            eq_op = types.promote(self.type, other.type).EQ
        c = self.emult(other, eq_op, cast=types.BOOL)
        if c.nvals != self.nvals:
            return False
        return c.reduce_bool(types.BOOL.LAND_MONOID)

    def apply(self, op, out=None, mask=None, accum=None, desc=None):
        if out is None:
            out = Matrix.sparse(self.type, self.nrows, self.ncols)
        mh, ah, dh = get_args(mask, accum, desc)
        check(lib.GrB_Matrix_apply(out._h, mh, ah, C.c_void_p(op.get_op()), self._h, dh), out)
        return out

    def apply_first(self, first, op, out=None, mask=None, accum=None, desc=None):
        """`op(first, A(i,j))` with a bound scalar (reference: pygraphblas/matrix.py:1965-2005)."""
        if out is None:
            out = Matrix.sparse(self.type, self.nrows, self.ncols)
        mh, ah, dh = get_args(mask, accum, desc)
        fn = getattr(lib, "GxB_Matrix_apply_BinaryOp1st_" + self.type.__name__)
        check(fn(out._h, mh, ah, C.c_void_p(op.get_op()), self.type._c(first), self._h, dh), out)
        return out

    def apply_second(self, op, second, out=None, mask=None, accum=None, desc=None):
        """`op(A(i,j), second)` with a bound scalar (reference: pygraphblas/matrix.py:2007-2040)."""
        if out is None:
            out = Matrix.sparse(self.type, self.nrows, self.ncols)
        mh, ah, dh = get_args(mask, accum, desc)
        fn = getattr(lib, "GxB_Matrix_apply_BinaryOp2nd_" + self.type.__name__)
        check(fn(out._h, mh, ah, C.c_void_p(op.get_op()), self._h, self.type._c(second), dh), out)
        return out

    def cast(self, cast, out=None):
        """The same entries in another type (reference: pygraphblas/matrix.py:1063-1086)."""
        if out is None:
            out = Matrix.sparse(cast, self.nrows, self.ncols)
        check(lib.GrB_Matrix_apply(out._h, None, None, C.c_void_p(cast.IDENTITY.get_op()), self._h, None), out)
        return out

    def __neg__(self):
        return self.apply(self.type.AINV)

    def __abs__(self):
        return self.apply(self.type.ABS)

    def __invert__(self):
        return self.apply(self.type.MINV)

    def assign_matrix(self, value, rindex=None, cindex=None, mask=None, accum=None, desc=None):
        """`C(I,J)<mask> = accum(C(I,J), value)` (reference: pygraphblas/matrix.py:3057-3130); index lists or None for all."""
        mh, ah, dh = get_args(mask, accum, desc)
        ri = build_range(rindex, self.nrows - 1); ci = build_range(cindex, self.ncols - 1)
        (I, ni, _s1, k1), (J, nj, _s2, k2) = ri, ci
        if ri.location or ci.location:
            check(lib.GrBX_Matrix_assign_at(self._h, mh, ah, value._h, I, u64(ni), J, u64(nj), dh, C.c_int(ri.location), C.c_int(ci.location)), self)
        else:
            check(lib.GrB_Matrix_assign(self._h, mh, ah, value._h, I, u64(ni), J, u64(nj), dh), self)

    assign = assign_matrix

    def assign_scalar(self, value, row_slice=None, col_slice=None, mask=None, accum=None, desc=None):
        """`C(I,J)<mask> = accum(C(I,J), value)` (reference: pygraphblas/matrix.py:3106-3239): `None` is every row / column, an int that one, a slice
        includes its stop, a list names explicit indices.  T is built in HBM (grb_assign_scalar.hip): from the mask's pattern when there is a mask that is
        not complemented — `A[M] = s` costs O(nvals(M) + nvals(A)) whatever the region's size —, else as the block in closed form."""
        mh, ah, dh = get_args(mask, accum, desc)
        if isinstance(row_slice, (int, np.integer)):
            row_slice = slice(int(row_slice), int(row_slice))
        if isinstance(col_slice, (int, np.integer)):
            col_slice = slice(int(col_slice), int(col_slice))
        _no_device_list(row_slice, col_slice)
        I, ni, _s1, k1 = build_range(row_slice, self.nrows - 1); J, nj, _s2, k2 = build_range(col_slice, self.ncols - 1)
        fn = self.type.__dict__.get("_matrix_assign_fn")
        if fn is None:
            fn = getattr(lib, "GrB_Matrix_assign_" + self.type.__name__); setattr(self.type, "_matrix_assign_fn", fn)      # (looked up once per type)
        check(fn(self._h, mh, ah, self.type._c(value), I, u64(ni), J, u64(nj), dh), self)

    def select(self, op, thunk=None, out=None, mask=None, accum=None, desc=None):
        """`GxB_Matrix_select` with a built-in select operator name ("TRIL", ">0", ...) or a `@select_op` operator (reference: matrix.py:2042-2140)."""
        user = isinstance(op, types.SelectOp)
        opname = None if user else {"tril": "TRIL", "triu": "TRIU", "diag": "DIAG", "offdiag": "OFFDIAG", "nonzero": "NONZERO",
                  "!=0": "NONZERO", "==0": "EQ_ZERO", ">0": "GT_ZERO", ">=0": "GE_ZERO", "<0": "LT_ZERO", "<=0": "LE_ZERO",
                  "!=": "NE_THUNK", "==": "EQ_THUNK", ">": "GT_THUNK", ">=": "GE_THUNK", "<": "LT_THUNK", "<=": "LE_THUNK"}.get(op, op)
        oph = C.c_void_p(op.get_op() if user else _capi.handle("GxB_" + opname))
        if out is None:
            out = Matrix.sparse(self.type, self.nrows, self.ncols)
        th = None
        if thunk is not None:
            th = C.c_void_p()
            ttyp = op.thunk_type if user else (types.INT64 if opname in ("TRIL", "TRIU", "DIAG", "OFFDIAG") else self.type)
            check(lib.GxB_Scalar_new(C.byref(th), C.c_void_p(ttyp._h)))
            check(getattr(lib, "GxB_Scalar_setElement_" + ttyp.__name__)(th, ttyp._c(thunk)))
        mh, ah, dh = get_args(mask, accum, desc)
        try:
            check(lib.GxB_Matrix_select(out._h, mh, ah, oph, self._h, th, dh), out)
        finally:
            if th is not None:
                lib.GxB_Scalar_free(C.byref(th))
        return out

    def tril(self, thunk=None):
        return self.select("TRIL", thunk)

    def triu(self, thunk=None):
        return self.select("TRIU", thunk)

    def diag(self, thunk=None):
        """The entries of the `thunk`-th diagonal, as a matrix of the same shape (reference: matrix.py:2202-2230)."""
        return self.select("DIAG", thunk)

    def offdiag(self, thunk=None):
        return self.select("OFFDIAG", thunk)

    def nonzero(self):
        return self.select("NONZERO")

    def pattern(self, typ=types.BOOL):
        """The structure of the matrix as a matrix of ones (reference: matrix.py:887-922)."""
        out = Matrix.sparse(typ, self.nrows, self.ncols)
        check(lib.GrB_Matrix_apply(out._h, None, None, C.c_void_p(typ.ONE.get_op()), self._h, None), out)
        return out

    def __repr__(self):
        return f"<Matrix ({self.nrows}x{self.ncols} : {self.nvals}:{self.type.__name__})>"
