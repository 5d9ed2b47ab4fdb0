// grb_kron.hip — the Kronecker product in HBM: T = A (x)_op B, CSR in, CSR out (behind GrB_Matrix_kronecker_BinaryOp, grb_kron_ops.cpp).
//
// Everything about T is known in closed form, so there is no count pass, no scan, no atomics, no sort and no size read back:
//   nnz(T)                  = nnz(A) nnz(B)
//   rowptr_T[ia br + ib]    = rowptr_A[ia] nnz(B) + len_A(ia) rowptr_B[ib]
//   entry t of row (ia, ib) = A's entry t / len_B(ib) of row ia  with  B's entry t % len_B(ib) of row ib, column ja bc + jb
// and the columns of a row come out sorted when A's and B's rows are.
//
//   k_kron_rowptr  one thread per output row (ar br + 1 of them) writes the closed form: 4 bytes per row, two cached reads.
//   k_kron_fill    ENTRY-PARALLEL: a lane owns KRON_EPL = 4 consecutive entries of T's column / value arrays.  It finds the first one's (ia, ib, ka, kb)
//                  by bisecting rowptr_A scaled by nnz(B), then rowptr_B scaled by len_A(ia) (products in 64 bits: they pass 2^32 long before the
//                  entry count does), and steps to the next three (kb, then ka; a new bisection only where the output row ends).  A hub row times a
//                  hub row — 10^5 x 10^5 = 10^10 entries — is simply that many lanes: no long-row path, no parts, no per-row workgroup.
//                  The four columns leave as ONE 16-byte store, the four values as one (4-byte types), two (8-byte) or a narrower one: a wave
//                  instruction writes 1 KiB of contiguous columns.  The last, partial group of the array is stored entry by entry.
//   traffic        written: nnz(T) (4 + sizeof T) bytes, once, coalesced — the whole cost.  Read: A and B through the caches (tiny next to T): per
//                  lane ~log2(ar) + log2(br) row-pointer words and up to 4 + 4 entries.
// A side the operator ignores (FIRST / SECOND / PAIR / ANY) is passed as nullptr and never dereferenced.
#include "grb_kron.hpp"
#include "grb_index.hpp"

namespace grb {
namespace {

constexpr int KRON_EPL = 4;                                                  // entries per lane: 16 bytes of columns

template <class T> struct alignas(sizeof(T) * KRON_EPL > 16 ? 16 : sizeof(T) * KRON_EPL) ValPack { T v[KRON_EPL]; };
struct alignas(16) ColPack { uint32_t c[KRON_EPL]; };

__global__ void k_kron_rowptr(uint32_t ar, uint32_t br, uint32_t nnzb, uint64_t nnzt, const uint32_t* __restrict__ arp, const uint32_t* __restrict__ brp, uint32_t* __restrict__ trp) {
  const uint64_t nrows = (uint64_t)ar * br;
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= nrows; r += gridDim.x * 256ull) {
    uint64_t v = nnzt;
    if (r < nrows) {
      const uint32_t ia = (uint32_t)r / br, ib = (uint32_t)r - ia * br;      // (nrows <= GRB_DIM_DEVICE_MAX: r fits 32 bits)
      const uint32_t pa = arp[ia], la = arp[ia + 1] - pa;
      v = (uint64_t)pa * nnzb + (uint64_t)la * brp[ib];
    }
    trp[r] = (uint32_t)v;                                                      // (v <= nnzt <= KRON_MAX_ENTRIES)
  }
}

// where entry q of T comes from
struct KronPos { uint32_t pa, la, ka, pb, lb, kb; };
__device__ __forceinline__ KronPos kron_locate(uint64_t q, uint32_t ar, uint32_t br, uint32_t nnzb, const uint32_t* __restrict__ arp, const uint32_t* __restrict__ brp) {
  KronPos p;
  uint32_t lo = 0, hi = ar;                                                  // rowptr_A[lo] nnzb <= q < rowptr_A[hi] nnzb (q < nnz(A) nnzb): ends at the non-empty row that holds q
  while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)arp[mid] * nnzb <= q) lo = mid; else hi = mid; }
  p.pa = arp[lo]; p.la = arp[lo + 1] - p.pa;
  const uint64_t r = q - (uint64_t)p.pa * nnzb;                              // position within A's row block: < la nnzb
  lo = 0; hi = br;                                                           // la rowptr_B[lo] <= r < la rowptr_B[hi]
  while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((uint64_t)p.la * brp[mid] <= r) lo = mid; else hi = mid; }
  p.pb = brp[lo]; p.lb = brp[lo + 1] - p.pb;
  const uint32_t t = (uint32_t)(r - (uint64_t)p.la * p.pb);                  // position within the output row: < la lb <= nnz(T) < 2^32
  p.ka = t / p.lb; p.kb = t - p.ka * p.lb;
  return p;
}

// OPC >= 0: the operator is known when the kernel is compiled and the switch of apply_binop folds away (TIMES, the default multiplier of Matrix.kronecker and
// the one Kronecker powers use: at most 40 VGPRs).  OPC < 0: any built-in operator, chosen by `op` (wave-uniform); the whole switch, divisions included, is
// unrolled over the lane's four entries and costs ~130 VGPRs for the floating-point types — fewer waves to hide the bisection's latency behind.
template <class T, bool MATH, int OPC>
__global__ __launch_bounds__(256) void k_kron_fill(uint64_t nnzt, uint32_t ar, uint32_t br, uint32_t bc, uint32_t nnzb, const uint32_t* __restrict__ arp, const uint32_t* __restrict__ acol,
                                                   const T* __restrict__ aval, const uint32_t* __restrict__ brp, const uint32_t* __restrict__ bcol, const T* __restrict__ bval, int op,
                                                   uint32_t* __restrict__ ocol, T* __restrict__ oval) {
  const uint64_t ngroups = (nnzt + KRON_EPL - 1) / KRON_EPL;
  for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < ngroups; g += gridDim.x * 256ull) {
    const uint64_t q0 = g * KRON_EPL;
    const int n = nnzt - q0 >= (uint64_t)KRON_EPL ? KRON_EPL : (int)(nnzt - q0);
    KronPos p = kron_locate(q0, ar, br, nnzb, arp, brp);
    uint64_t ja = (uint64_t)acol[p.pa + p.ka] * bc;
    T av = aval ? aval[p.pa + p.ka] : T(0);
    ColPack c; ValPack<T> v;
#pragma unroll
    for (int j = 0; j < KRON_EPL; j++) {
      if (j < n) {
        if (j) {
          if (++p.kb == p.lb) {
            p.kb = 0;
            if (++p.ka == p.la) p = kron_locate(q0 + j, ar, br, nnzb, arp, brp);      // the output row ended: the next non-empty one
            ja = (uint64_t)acol[p.pa + p.ka] * bc;
            if (aval) av = aval[p.pa + p.ka];
          }
        }
        const uint32_t eb = p.pb + p.kb;
        c.c[j] = (uint32_t)(ja + bcol[eb]);                                  // (< ac bc <= GRB_DIM_DEVICE_MAX)
        v.v[j] = apply_binop<T, true, MATH>(OPC >= 0 ? OPC : op, av, bval ? bval[eb] : T(0));
      } else { c.c[j] = 0; v.v[j] = T(0); }
    }
    if (n == KRON_EPL) {
      *reinterpret_cast<ColPack*>(ocol + q0) = c;
      *reinterpret_cast<ValPack<T>*>(oval + q0) = v;
    } else {
      for (int j = 0; j < n; j++) { ocol[q0 + j] = c.c[j]; oval[q0 + j] = v.v[j]; }
    }
  }
}

struct FillTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~FillTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

}  // namespace

void kron_csr(int code, int opcode, const DevCSR& A, const void* aval, const DevCSR& B, const void* bval, DevCSR& T, float* fill_ms) {
  const uint64_t nrows = (uint64_t)A.nrows * B.nrows, ncols = (uint64_t)A.ncols * B.ncols, nnz = A.nnz * B.nnz;
  if (nrows > GRB_DIM_DEVICE_MAX || ncols > GRB_DIM_DEVICE_MAX || A.nnz > KRON_MAX_ENTRIES || B.nnz > KRON_MAX_ENTRIES || nnz > KRON_MAX_ENTRIES)
    fail(GrB_PANIC, "kronecker: the product does not fit the 32-bit device layout");      // (the entry point checked it: the kernels' bounds depend on it)
  if (fill_ms) *fill_ms = 0.0f;
  const size_t ts = type_size(code);
  const uint64_t grid_cap = (uint64_t)device_cus() * 8;
  T.clear(); T.nrows = (uint32_t)nrows; T.ncols = (uint32_t)ncols; T.nnz = nnz;
  T.rowptr.alloc((nrows + 1) * 4); T.col.alloc(nnz * 4 + 4); T.val.alloc(nnz * ts + 8);
  if (!nnz) { GRB_HIP(hipMemsetAsync(T.rowptr.p, 0, (nrows + 1) * 4, stream())); GRB_HIP(hipStreamSynchronize(stream())); T.valid = true; return; }
  hipLaunchKernelGGL(k_kron_rowptr, dim3(grid_1d(nrows + 1, grid_cap)), dim3(256), 0, stream(), A.nrows, B.nrows, (uint32_t)B.nnz, nnz, A.rowptr.as<uint32_t>(), B.rowptr.as<uint32_t>(), T.rowptr.as<uint32_t>());
  FillTimer tm;
  if (fill_ms) { GRB_HIP(hipEventCreate(&tm.e0)); GRB_HIP(hipEventCreate(&tm.e1)); GRB_HIP(hipEventRecord(tm.e0, stream())); }
  const unsigned grid = grid_1d((nnz + KRON_EPL - 1) / KRON_EPL, grid_cap);
#define GRB_KRON_FILL(MATH, OPC) hipLaunchKernelGGL((k_kron_fill<V, MATH, OPC>), dim3(grid), dim3(256), 0, stream(), nnz, A.nrows, B.nrows, B.ncols, (uint32_t)B.nnz, A.rowptr.as<uint32_t>(), \
    A.col.as<uint32_t>(), (const V*)aval, B.rowptr.as<uint32_t>(), B.col.as<uint32_t>(), (const V*)bval, opcode, T.col.as<uint32_t>(), T.val.as<V>())
  dispatch_type(code, [&]<class V>() {
    if (opcode == B_TIMES) GRB_KRON_FILL(false, B_TIMES);
    else if (binop_needs_math(opcode)) GRB_KRON_FILL(true, -1);
    else GRB_KRON_FILL(false, -1);
  });
#undef GRB_KRON_FILL
  GRB_HIP(hipGetLastError());
  if (fill_ms) GRB_HIP(hipEventRecord(tm.e1, stream()));
  GRB_HIP(hipStreamSynchronize(stream()));                                   // the caller's cast copies of the operands' values are released when it returns
  if (fill_ms) GRB_HIP(hipEventElapsedTime(fill_ms, tm.e0, tm.e1));
  T.valid = true;
}

}  // namespace grb
