// grb_possr.hip — the kernels of the positional semirings (grb_possr.hpp): gather-bound pulls, wave64, no LDS crossbar beyond the product's accumulators, no
// atomics.  Templated on (monoid, T in {int32, int64}); which coordinate a product is — and the + 1 of the ...1 forms — is the PosCoord passed by value, so the
// 80 semirings x 3 operations are 10 instantiations of each kernel.
//
//   k_possr_rows      mxv / vxm.  A wave per row of the CSR the driver picked (rows in a grid-stride loop, at most 16 workgroups per compute unit); a row whose
//                     allow byte is 0 is skipped.  Lanes stride over the row's column indices and gather ONLY the operand's presence byte: neither value array
//                     is an argument.  sel == k: every lane folds coord(k) with the monoid from its first present term, carrying a `has` flag, and the 64
//                     (value, has) pairs combine by lane shuffles at 32, 16 ... 1.  ANY stops at the first stride in which a lane found a term and takes the
//                     lowest such lane (reproducible).  MIN / MAX never stop early: the containers carry no flag that says a row's columns ascend.
//                     sel == row / zero: every term has the same value v, so the wave only counts the terms — MIN / MAX / ANY: v if any (ANY stops at the first
//                     stride with one); PLUS: v * count, wrapped; TIMES: v ^ count by repeated squaring, wrapped.
//   k_possr_product   mxm, on a T whose pattern exists (columns ascending).  A wave per row i walks k over A(i,:); lanes stride over B(k,:) and bisect j in
//                     T(i,:) — a j not found was dropped by the mask — and combine coord(i, k, j) into that slot: accumulators and `seen` bytes in LDS for
//                     rows of <= 128 entries, in T.val and a byte array beyond.  The columns of B(k,:) are distinct, so no two lanes share a slot within one k;
//                     a workgroup-scope fence after each k orders the wave's own stores before its next loads.  No __syncthreads: the waves of a workgroup walk
//                     rows of different lengths.
//   k_possr_fill      mxm with FIRSTI / SECONDJ under MIN / MAX / ANY: the value is i or j of T's own pattern — one streaming pass over T, no k loop.
// Traffic of a rows call: 4 bytes per entry of the CSR + one presence byte gathered per entry + (n + 1) row pointers, against + 8 value bytes per entry gathered
// from a POSITIONI copy of the matrix in the MIN_SECOND workaround.
#include "grb_possr.hpp"
#include "grb_api.hpp"
#include "grb_device.hpp"

namespace grb {
namespace {

constexpr int POSSR_LDS_ROW = 128;      // entries of a row of T whose accumulators live in LDS: 4 waves x 128 x (8 + 1) bytes per workgroup

template <class T> __device__ __forceinline__ T coord_value(PosCoord c, uint32_t row, uint32_t k, uint32_t col) {
  const uint64_t x = c.sel == PS_ROW ? row : c.sel == PS_K ? k : c.sel == PS_COL ? col : 0u;
  return (T)(x + (uint64_t)c.plus1);      // the C cast of the index: INT32 wraps
}

// v ^ n in T's unsigned arithmetic (n >= 1)
template <class T> __device__ __forceinline__ T wrap_pow(T v, uint32_t n) {
  T r = (T)1, b = v;
  while (n) { if (n & 1u) r = apply_binop<T, false>(B_TIMES, r, b); b = apply_binop<T, false>(B_TIMES, b, b); n >>= 1; }
  return r;
}

template <int ADD, class T>
__global__ __launch_bounds__(256) void k_possr_rows(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, const uint8_t* __restrict__ upres,
                                                    const uint8_t* __restrict__ allow, T* __restrict__ tval, uint8_t* __restrict__ tpres, uint32_t nrows, PosCoord c) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4ull;
  for (uint64_t r = ((uint64_t)blockIdx.x * 256ull + threadIdx.x) >> 6; r < nrows; r += nwaves) {      // (r is the same in every lane of a wave)
    if (allow && !allow[r]) { if (lane == 0) { tval[r] = (T)0; tpres[r] = 0; } continue; }
    const uint32_t pb = rowptr[r], pe = rowptr[r + 1];
    T acc = (T)0; bool has = false;
    if (c.sel == PS_K) {
      if constexpr (ADD == B_ANY) {
        for (uint32_t p0 = pb; p0 < pe; p0 += 64u) {      // (the loop bound is wave-uniform: every lane reaches the ballot)
          const uint32_t p = p0 + lane;
          uint32_t k = 0; bool hit = false;
          if (p < pe) { k = col[p]; hit = !upres || upres[k]; }
          const unsigned long long found = __ballot(hit);
          if (found) { acc = coord_value<T>(c, (uint32_t)r, (uint32_t)__shfl((int)k, __ffsll((long long)found) - 1, 64), 0u); has = true; break; }
        }
      } else {
        for (uint32_t p = pb + lane; p < pe; p += 64u) {
          const uint32_t k = col[p];
          if (upres && !upres[k]) continue;
          const T v = coord_value<T>(c, (uint32_t)r, k, 0u);
          acc = has ? apply_binop<T, false>(ADD, acc, v) : v; has = true;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {      // lane l takes lane l + d
          const T oacc = shfl_down_t<T>(acc, d); const int ohas = __shfl_down(has ? 1 : 0, d, 64);
          if (lane + d < 64u && ohas) { acc = has ? apply_binop<T, false>(ADD, acc, oacc) : oacc; has = true; }
        }
      }
    } else {
      // every term of the row has the value v: the row's answer is a function of (v, number of terms)
      uint32_t cnt = 0;
      for (uint32_t p0 = pb; p0 < pe; p0 += 64u) {
        const uint32_t p = p0 + lane;
        const bool hit = p < pe && (!upres || upres[col[p]]);
        cnt += (uint32_t)__popcll(__ballot(hit));      // (wave-uniform)
        if (cnt && (ADD == B_ANY || ADD == B_MIN || ADD == B_MAX)) break;
      }
      if (cnt) {
        const T v = coord_value<T>(c, (uint32_t)r, 0u, 0u);
        has = true;
        if constexpr (ADD == B_PLUS) acc = apply_binop<T, false>(B_TIMES, v, (T)cnt);
        else if constexpr (ADD == B_TIMES) acc = wrap_pow<T>(v, cnt);
        else acc = v;
      }
    }
    if (lane == 0) { tval[r] = has ? acc : (T)0; tpres[r] = has ? 1 : 0; }
  }
}

template <int ADD, class T>
__global__ __launch_bounds__(256) void k_possr_product(const uint32_t* __restrict__ arp, const uint32_t* __restrict__ acol, const uint32_t* __restrict__ brp,
                                                       const uint32_t* __restrict__ bcol, const uint32_t* __restrict__ crp, const uint32_t* __restrict__ ccol,
                                                       T* cval, uint8_t* seen, uint32_t nrows, PosCoord c) {
  __shared__ T lacc[4][POSSR_LDS_ROW]; __shared__ uint8_t lseen[4][POSSR_LDS_ROW];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4ull;
  for (uint64_t i = ((uint64_t)blockIdx.x * 256ull + threadIdx.x) >> 6; i < nrows; i += nwaves) {      // (i is the same in every lane of a wave)
    const uint32_t cb = crp[i], ce = crp[i + 1], len = ce - cb;
    if (!len) continue;
    const bool in_lds = len <= (uint32_t)POSSR_LDS_ROW;
    if (in_lds) for (uint32_t q = lane; q < len; q += 64u) lseen[w][q] = 0;
    // a slot written by one lane at one k is read by another lane of this wave at the next: every step ends with the wave's stores complete and visible
    __threadfence_block();
    for (uint32_t pa = arp[i]; pa < arp[i + 1]; pa++) {
      const uint32_t k = acol[pa];
      const uint32_t bb = brp[k], be = brp[k + 1];
      for (uint32_t pb = bb + lane; pb < be; pb += 64u) {      // the columns of B(k,:) are distinct: no two lanes share a slot within one k
        const uint32_t j = bcol[pb];
        uint32_t lo = cb, hi = ce;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (ccol[mid] < j) lo = mid + 1; else hi = mid; }
        if (lo >= ce || ccol[lo] != j) continue;      // not in T's row: the mask dropped it
        const T prod = coord_value<T>(c, (uint32_t)i, k, j);
        if (in_lds) { const uint32_t q = lo - cb; lacc[w][q] = lseen[w][q] ? apply_binop<T, false>(ADD, lacc[w][q], prod) : prod; lseen[w][q] = 1; }
        else { cval[lo] = seen[lo] ? apply_binop<T, false>(ADD, cval[lo], prod) : prod; seen[lo] = 1; }
      }
      __threadfence_block();
    }
    if (in_lds) for (uint32_t q = lane; q < len; q += 64u) cval[cb + q] = lseen[w][q] ? lacc[w][q] : (T)0;
    __threadfence_block();      // (the LDS rows are free for the wave's next row)
  }
}

template <class T>
__global__ __launch_bounds__(256) void k_possr_fill(const uint32_t* __restrict__ crp, const uint32_t* __restrict__ ccol, T* __restrict__ cval, uint32_t nrows, PosCoord c) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4ull;
  for (uint64_t i = ((uint64_t)blockIdx.x * 256ull + threadIdx.x) >> 6; i < nrows; i += nwaves)
    for (uint32_t p = crp[i] + lane; p < crp[i + 1]; p += 64u) cval[p] = coord_value<T>(c, (uint32_t)i, 0u, ccol[p]);
}

// f.template operator()<ADD, T>() for the monoid and the type of the call
template <class F> void with_monoid_and_type(int addop, int zcode, F&& f) {
  auto by_type = [&]<int ADD>() {
    if (zcode == T_INT32) f.template operator()<ADD, int32_t>();
    else if (zcode == T_INT64) f.template operator()<ADD, int64_t>();
    else fail(GrB_PANIC, "positional semiring: its type is INT32 or INT64");
  };
  switch (addop) {
    case B_MIN: by_type.template operator()<B_MIN>(); break;
    case B_MAX: by_type.template operator()<B_MAX>(); break;
    case B_PLUS: by_type.template operator()<B_PLUS>(); break;
    case B_TIMES: by_type.template operator()<B_TIMES>(); break;
    case B_ANY: by_type.template operator()<B_ANY>(); break;
    default: fail(GrB_PANIC, "positional semiring: its monoid is MIN, MAX, PLUS, TIMES or ANY");
  }
}

const char* monoid_word(int addop) { switch (addop) { case B_MIN: return "MIN"; case B_MAX: return "MAX"; case B_PLUS: return "PLUS"; case B_TIMES: return "TIMES"; case B_ANY: return "ANY"; default: return "?"; } }
const char* mul_word(int mulop) {
  static const char* const w[] = {"FIRSTI", "FIRSTI1", "FIRSTJ", "FIRSTJ1", "SECONDI", "SECONDI1", "SECONDJ", "SECONDJ1"};
  return binop_is_positional(mulop) ? w[mulop - B_FIRSTI] : "?";
}

}  // namespace

void possr_needs_layout(const GrB_Semiring_opaque* s, bool hyper, bool cplx) {
  if (hyper) fail(GrB_DOMAIN_MISMATCH, std::string("positional semiring ") + s->name + ": hypersparse containers (a dimension or size beyond the device layout) are out of its scope");
  if (cplx) fail(GrB_DOMAIN_MISMATCH, std::string("positional semiring ") + s->name + ": complex containers are out of its scope");
}

void possr_refuse_elementwise(const GrB_Semiring_opaque* s, const char* where) {
  if (check_obj(s) && check_obj(s->mul) && is_positional_semiring(s))
    fail(GrB_DOMAIN_MISMATCH, std::string("positional semiring ") + s->name + " cannot be used in " + where + ": positional semirings run in mxm, mxv and vxm only");
}

std::string possr_plan(int kind, const GrB_Semiring_opaque* s) {
  const char* tn = s->add->op->ztype->name;      // "GrB_INT64"
  return std::string("possr<add=") + monoid_word(s->add->op->opcode) + ",mul=" + mul_word(s->mul->opcode) + ",type=" + (strncmp(tn, "GrB_", 4) ? tn : tn + 4) +
         ",kind=" + (kind == PK_MXV ? "mxv" : kind == PK_VXM ? "vxm" : "mxm") + "> ";
}

void possr_rows(int addop, int zcode, PosCoord c, const DevCSR& R, const uint8_t* upres, const uint8_t* allow, void* tval, uint8_t* tpres) {
  g_last_plan += "k_possr_rows ";
  if (!R.nrows) return;
  with_monoid_and_type(addop, zcode, [&]<int ADD, class T>() {
    hipLaunchKernelGGL((k_possr_rows<ADD, T>), dim3(row_launch_blocks(R.nrows)), dim3(256), 0, stream(), R.rowptr.as<uint32_t>(), R.col.as<uint32_t>(), upres, allow, (T*)tval, tpres,
                       R.nrows, c);
  });
  GRB_HIP(hipGetLastError());
}

void possr_product_values(int addop, int zcode, PosCoord c, const DevCSR& A, const DevCSR& B, DevCSR& T) {
  const bool fill = c.sel != PS_K && (addop == B_MIN || addop == B_MAX || addop == B_ANY);      // i or j of T's own pattern
  g_last_plan += fill ? "k_possr_fill " : "k_possr_product ";
  if (!T.nnz || !T.nrows) return;
  if (fill) {
    if (zcode == T_INT32) hipLaunchKernelGGL((k_possr_fill<int32_t>), dim3(row_launch_blocks(T.nrows)), dim3(256), 0, stream(), T.rowptr.as<uint32_t>(), T.col.as<uint32_t>(), T.val.as<int32_t>(), T.nrows, c);
    else hipLaunchKernelGGL((k_possr_fill<int64_t>), dim3(row_launch_blocks(T.nrows)), dim3(256), 0, stream(), T.rowptr.as<uint32_t>(), T.col.as<uint32_t>(), T.val.as<int64_t>(), T.nrows, c);
    GRB_HIP(hipGetLastError());
    return;
  }
  DevBuf seen(T.nnz + 16);
  GRB_HIP(hipMemsetAsync(seen.p, 0, T.nnz, stream()));
  with_monoid_and_type(addop, zcode, [&]<int ADD, class V>() {
    hipLaunchKernelGGL((k_possr_product<ADD, V>), dim3(row_launch_blocks(T.nrows)), dim3(256), 0, stream(), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(), B.rowptr.as<uint32_t>(),
                       B.col.as<uint32_t>(), T.rowptr.as<uint32_t>(), T.col.as<uint32_t>(), T.val.as<V>(), seen.as<uint8_t>(), T.nrows, c);
  });
  GRB_HIP(hipGetLastError());
  GRB_HIP(hipStreamSynchronize(stream()));      // `seen` returns to the pool when this scope ends
}

}  // namespace grb
