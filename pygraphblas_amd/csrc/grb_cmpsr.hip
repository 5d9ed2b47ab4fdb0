// grb_cmpsr.hip — the kernels of the comparison semirings (grb_cmpsr.hpp): gather-bound pulls, wave64, no atomics.  Templated on (monoid, T); WHICH comparison
// runs is the CmpSel passed by value — three mask words over (a == b, a < b, a > b) and a negation, combined without a branch — so the 300 semirings x 3
// operations are 50 instantiations of each kernel, not 300, and vxm's mirrored comparison costs no instantiation at all.
//
//   k_cmpsr_rows      mxv / vxm.  A wave per row of the CSR the driver picked (rows in a grid-stride loop, row_launch_blocks); a row whose allow byte is 0 is
//                     skipped.  Lanes stride over the row: col[p] and aval[p] stream, upres[k] is gathered, uval[k] only where upres[k] says there is an entry.
//                     Every stride ends in two ballots — the lanes with a term, the lanes whose term is true — and the BOOL monoids fold those masks, no value is
//                     shuffled: LOR any true term, LAND no false term, LXOR the parity of the true terms, EQ (LXNOR) the parity of the false terms, ANY the
//                     lowest lane with a term of the first stride that has one (reproducible).  LOR stops at the first stride with a true term, LAND at the
//                     first with a false one, ANY at the first with any.  The loop bound is wave-uniform: every lane reaches every ballot.
//   k_cmpsr_product   mxm, on a T whose pattern exists (columns ascending).  The shape of k_possr_product: a wave per row i walks k over A(i,:); lanes stride over
//                     B(k,:) and bisect j in T(i,:) — a j not found was dropped by the mask — and fold cmp(A(i,k), B(k,j)) into that slot: one-byte accumulators
//                     and `seen` bytes in LDS for rows of <= 128 entries, in T.val and a byte array beyond.  The columns of B(k,:) are distinct, so no two lanes
//                     share a slot within one k; a workgroup-scope fence after each k orders the wave's own stores before its next loads.  No __syncthreads.
// Traffic of a rows call: (4 + sizeof T) bytes per entry of the CSR streamed + one presence byte and at most one value gathered per entry + (n + 1) row pointers
// + 2 bytes written per row, against n x sizeof T written by the MAX_ISEQ_<T> workaround before its cast.
#include "grb_cmpsr.hpp"
#include "grb_api.hpp"
#include "grb_device.hpp"

namespace grb {
namespace {

constexpr int CMPSR_LDS_ROW = 128;      // entries of a row of T whose accumulators live in LDS: 4 waves x 128 x (1 + 1) bytes per workgroup

// NaN: none of the three outcomes holds, so only NE (the negation of EQ) is true.  -0.0 == 0.0.  Unsigned T compares as unsigned: the operators are T's own.
template <class T> __device__ __forceinline__ bool compare(CmpSel c, T a, T b) {
  const uint32_t r = ((a == b) ? c.eq : 0u) | ((a < b) ? c.lt : 0u) | ((a > b) ? c.gt : 0u);
  return (r ^ c.inv) != 0u;
}

// z = add(x, y) of a BOOL monoid (ANY keeps what it has)
template <int ADD> __device__ __forceinline__ bool fold2(bool x, bool y) {
  if constexpr (ADD == B_LOR) return x || y;
  else if constexpr (ADD == B_LAND) return x && y;
  else if constexpr (ADD == B_LXOR) return x != y;
  else if constexpr (ADD == B_LXNOR) return x == y;
  else return x;
}

template <int ADD, class T>
__global__ __launch_bounds__(256) void k_cmpsr_rows(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, const T* __restrict__ aval,
                                                    const T* __restrict__ uval, const uint8_t* __restrict__ upres, const uint8_t* __restrict__ allow,
                                                    uint8_t* __restrict__ tval, uint8_t* __restrict__ tpres, uint32_t nrows, CmpSel c) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4ull;
  for (uint64_t r = ((uint64_t)blockIdx.x * 256ull + threadIdx.x) >> 6; r < nrows; r += nwaves) {      // (r is the same in every lane of a wave)
    if (allow && !allow[r]) { if (lane == 0) { tval[r] = 0; tpres[r] = 0; } continue; }
    const uint32_t pb = rowptr[r], pe = rowptr[r + 1];
    bool has = false, val = false;      // wave-uniform: functions of ballots only
    uint32_t parity = 0;
    for (uint32_t p0 = pb; p0 < pe; p0 += 64u) {      // (the loop bound is wave-uniform: every lane reaches the ballots)
      const uint32_t p = p0 + lane;
      bool present = false, t = false;
      if (p < pe) {
        const uint32_t k = col[p];
        present = !upres || upres[k];
        if (present) t = compare<T>(c, aval[p], uval[k]);      // (an absent u(k) holds whatever was left there: never read)
      }
      const unsigned long long terms = __ballot(present), trues = __ballot(t);      // (t implies present)
      if (!terms) continue;
      has = true;
      if constexpr (ADD == B_LOR) { val = trues != 0ull; if (val) break; }
      else if constexpr (ADD == B_LAND) { val = trues == terms; if (!val) break; }
      else if constexpr (ADD == B_LXOR) parity ^= (uint32_t)__popcll(trues) & 1u;
      else if constexpr (ADD == B_LXNOR) parity ^= (uint32_t)__popcll(terms & ~trues) & 1u;
      else { val = ((trues >> (__ffsll((long long)terms) - 1)) & 1ull) != 0ull; break; }
    }
    if constexpr (ADD == B_LXOR) val = parity != 0u;
    if constexpr (ADD == B_LXNOR) val = parity == 0u;      // x1 xnor ... xnor xn is true iff an even number of the x are false
    if (lane == 0) { tval[r] = has && val ? 1 : 0; tpres[r] = has ? 1 : 0; }
  }
}

template <int ADD, class T>
__global__ __launch_bounds__(256) void k_cmpsr_product(const uint32_t* __restrict__ arp, const uint32_t* __restrict__ acol, const T* __restrict__ aval,
                                                       const uint32_t* __restrict__ brp, const uint32_t* __restrict__ bcol, const T* __restrict__ bval,
                                                       const uint32_t* __restrict__ crp, const uint32_t* __restrict__ ccol, uint8_t* cval, uint8_t* seen,
                                                       uint32_t nrows, CmpSel c) {
  __shared__ uint8_t lacc[4][CMPSR_LDS_ROW]; __shared__ uint8_t lseen[4][CMPSR_LDS_ROW];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4ull;
  for (uint64_t i = ((uint64_t)blockIdx.x * 256ull + threadIdx.x) >> 6; i < nrows; i += nwaves) {      // (i is the same in every lane of a wave)
    const uint32_t cb = crp[i], ce = crp[i + 1], len = ce - cb;
    if (!len) continue;
    const bool in_lds = len <= (uint32_t)CMPSR_LDS_ROW;
    if (in_lds) for (uint32_t q = lane; q < len; q += 64u) lseen[w][q] = 0;
    // a slot written by one lane at one k is read by another lane of this wave at the next: every step ends with the wave's stores complete and visible
    __threadfence_block();
    for (uint32_t pa = arp[i]; pa < arp[i + 1]; pa++) {
      const uint32_t k = acol[pa];
      const T a = aval[pa];
      const uint32_t bb = brp[k], be = brp[k + 1];
      for (uint32_t pb = bb + lane; pb < be; pb += 64u) {      // the columns of B(k,:) are distinct: no two lanes share a slot within one k
        const uint32_t j = bcol[pb];
        uint32_t lo = cb, hi = ce;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (ccol[mid] < j) lo = mid + 1; else hi = mid; }
        if (lo >= ce || ccol[lo] != j) continue;      // not in T's row: the mask dropped it
        const bool prod = compare<T>(c, a, bval[pb]);
        if (in_lds) { const uint32_t q = lo - cb; lacc[w][q] = (lseen[w][q] ? fold2<ADD>(lacc[w][q] != 0, prod) : prod) ? 1 : 0; lseen[w][q] = 1; }
        else { cval[lo] = (seen[lo] ? fold2<ADD>(cval[lo] != 0, prod) : prod) ? 1 : 0; seen[lo] = 1; }
      }
      __threadfence_block();
    }
    if (in_lds) for (uint32_t q = lane; q < len; q += 64u) cval[cb + q] = lseen[w][q] ? lacc[w][q] : (uint8_t)0;
    __threadfence_block();      // (the LDS rows are free for the wave's next row)
  }
}

// f.template operator()<ADD, T>() for the monoid and the comparison type of the call
template <class F> void with_monoid_and_type(int addop, int xcode, F&& f) {
  auto by_type = [&]<int ADD>() {
    switch (xcode) {
      case T_INT8: f.template operator()<ADD, int8_t>(); break;
      case T_UINT8: f.template operator()<ADD, uint8_t>(); break;
      case T_INT16: f.template operator()<ADD, int16_t>(); break;
      case T_UINT16: f.template operator()<ADD, uint16_t>(); break;
      case T_INT32: f.template operator()<ADD, int32_t>(); break;
      case T_UINT32: f.template operator()<ADD, uint32_t>(); break;
      case T_INT64: f.template operator()<ADD, int64_t>(); break;
      case T_UINT64: f.template operator()<ADD, uint64_t>(); break;
      case T_FP32: f.template operator()<ADD, float>(); break;
      case T_FP64: f.template operator()<ADD, double>(); break;
      default: fail(GrB_PANIC, "comparison semiring: its multiplier compares one of the 10 non-Boolean real types");
    }
  };
  switch (addop) {
    case B_LOR: by_type.template operator()<B_LOR>(); break;
    case B_LAND: by_type.template operator()<B_LAND>(); break;
    case B_LXOR: by_type.template operator()<B_LXOR>(); break;
    case B_LXNOR: by_type.template operator()<B_LXNOR>(); break;
    case B_ANY: by_type.template operator()<B_ANY>(); break;
    default: fail(GrB_PANIC, "comparison semiring: its monoid is LOR, LAND, LXOR, EQ or ANY on BOOL");
  }
}

const char* monoid_word(int addop) { switch (addop) { case B_LOR: return "LOR"; case B_LAND: return "LAND"; case B_LXOR: return "LXOR"; case B_LXNOR: return "EQ"; case B_ANY: return "ANY"; default: return "?"; } }
const char* mul_word(int mulop) { switch (mulop) { case B_EQ: return "EQ"; case B_NE: return "NE"; case B_GT: return "GT"; case B_LT: return "LT"; case B_GE: return "GE"; case B_LE: return "LE"; default: return "?"; } }

}  // namespace

CmpSel cmp_sel(int mulop, int kind) {
  CmpSel c{0u, 0u, 0u, 0u};
  switch (mulop) {
    case B_EQ: c.eq = 1u; break;
    case B_NE: c.eq = 1u; c.inv = 1u; break;
    case B_LT: c.lt = 1u; break;
    case B_GT: c.gt = 1u; break;
    case B_LE: c.eq = 1u; c.lt = 1u; break;
    case B_GE: c.eq = 1u; c.gt = 1u; break;
    default: fail(GrB_PANIC, "comparison semiring: its multiplier is EQ, NE, GT, LT, GE or LE");
  }
  // vxm: cmp(u(k), A(k,j)), and the kernel holds A(k,j) first — a < b is b > a
  if (kind == CK_VXM) { const uint32_t t = c.lt; c.lt = c.gt; c.gt = t; }
  return c;
}

void cmpsr_needs_layout(const GrB_Semiring_opaque* s, bool hyper, bool cplx) {
  if (hyper) fail(GrB_DOMAIN_MISMATCH, std::string("comparison semiring ") + s->name + ": hypersparse containers (a dimension or size beyond the device layout) are out of its scope");
  if (cplx) fail(GrB_DOMAIN_MISMATCH, std::string("comparison semiring ") + s->name + ": complex containers are out of its scope");
}

std::string cmpsr_plan(int kind, const GrB_Semiring_opaque* s) {
  const char* tn = s->mul->xtype->name;      // "GrB_INT64"
  return std::string("cmpsr<add=") + monoid_word(s->add->op->opcode) + ",mul=" + mul_word(s->mul->opcode) + ",type=" + (strncmp(tn, "GrB_", 4) ? tn : tn + 4) +
         ",kind=" + (kind == CK_MXV ? "mxv" : kind == CK_VXM ? "vxm" : "mxm") + "> ";
}

void cmpsr_rows(int addop, int xcode, CmpSel c, const DevCSR& R, const void* aval, const void* uval, const uint8_t* upres, const uint8_t* allow, uint8_t* tval, uint8_t* tpres) {
  g_last_plan += "k_cmpsr_rows ";
  if (!R.nrows) return;
  with_monoid_and_type(addop, xcode, [&]<int ADD, class T>() {
    hipLaunchKernelGGL((k_cmpsr_rows<ADD, T>), dim3(row_launch_blocks(R.nrows)), dim3(256), 0, stream(), R.rowptr.as<uint32_t>(), R.col.as<uint32_t>(), (const T*)aval, (const T*)uval,
                       upres, allow, tval, tpres, R.nrows, c);
  });
  GRB_HIP(hipGetLastError());
}

void cmpsr_product_values(int addop, int xcode, CmpSel c, const DevCSR& A, const void* aval, const DevCSR& B, const void* bval, DevCSR& T) {
  g_last_plan += "k_cmpsr_product ";
  if (!T.nnz || !T.nrows) return;
  DevBuf seen(T.nnz + 16);
  GRB_HIP(hipMemsetAsync(seen.p, 0, T.nnz, stream()));
  with_monoid_and_type(addop, xcode, [&]<int ADD, class V>() {
    hipLaunchKernelGGL((k_cmpsr_product<ADD, V>), dim3(row_launch_blocks(T.nrows)), dim3(256), 0, stream(), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(), (const V*)aval,
                       B.rowptr.as<uint32_t>(), B.col.as<uint32_t>(), (const V*)bval, T.rowptr.as<uint32_t>(), T.col.as<uint32_t>(), T.val.as<uint8_t>(), seen.as<uint8_t>(), T.nrows, c);
  });
  GRB_HIP(hipGetLastError());
  GRB_HIP(hipStreamSynchronize(stream()));      // `seen` returns to the pool when this scope ends
}

}  // namespace grb
