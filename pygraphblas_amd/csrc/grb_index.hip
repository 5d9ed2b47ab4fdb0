// grb_index.hip — an explicit index list that already lies in HBM (GrBX_*_extract_at / GrBX_*_assign_at with location 1, a vector as an index list): the
// device side of extract_parse (grb_extract.hpp).  The list is n 64-bit indices in an array the caller owns (a torch tensor, usually); the extract and assign
// kernels take a 32-bit list, its length and whether it is strictly increasing (ExIdx), and that is all this file produces — the list never visits the host.
//
//   k_index_parse     one streaming pass, wave64, 256 threads, a capped grid with a loop past the cap (INDEX_PARSE_GRID_CAP).  A lane holds two neighbouring
//                     indices: one 16-byte load, both tested against `dim` as 64-bit unsigned values (a low word in range with a high word set is out of
//                     bounds, and so is every negative int64), one 8-byte store of the narrowed pair.  "Strictly increasing" needs the predecessor of a
//                     lane's first index: it is the second index of the lane below (one __shfl_up of the narrowed word — a comparison of narrowed words is the
//                     comparison of the indices unless one is out of bounds, and then the call fails whatever the order); only a wave's first lane reads
//                     I[k - 1] from memory.  A pointer that is only 8-byte aligned (a tensor view t[1:]) gets a scalar head element so that the pairs start
//                     on a 16-byte boundary, an odd rest a scalar tail; the narrowed list is allocated one word off in that case, so that the pair stores
//                     stay 8-byte aligned.  The two flags are OR-ed over the wave's rounds in a register, across the wave by two ballots, and one vector atomic
//                     OR per wave that has anything to report goes to the status word, which the host reads back (as assign_inverse reads its repeat flag):
//                     that read-back is also the point after which the caller's array is never read again.
//   k_index_widen     a vector's values (the eight integer types) as 64-bit indices: signed values sign-extended and then read as unsigned, so a negative
//                     value is out of bounds for k_index_parse.
#include "grb_index.hpp"

namespace grb {
namespace {

static_assert(INDEX_PARSE_THREADS == 256 && INDEX_PARSE_PER_LANE == 2, "k_index_parse is written for 256 threads and pairs");

struct alignas(16) U64x2 { uint64_t a, b; };
struct alignas(8) U32x2 { uint32_t a, b; };
enum : uint32_t { IDX_OUT_OF_BOUNDS = 1u, IDX_NOT_INCREASING = 2u };

// I: n indices; `head`: 1 when I is not 16-byte aligned (then I + 1 is), else 0; out + head is 8-byte aligned.
__global__ __launch_bounds__(256) void k_index_parse(const uint64_t* __restrict__ I, uint64_t n, uint64_t dim, uint32_t head, uint32_t* __restrict__ out, uint32_t* __restrict__ status) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t npairs = (n - head) >> 1;                                   // (n >= head: the host launches nothing for n == 0)
  uint32_t f = 0;
  // the loop bound depends on the wave only: every lane takes part in the shuffle and the ballots
  for (uint64_t base = blockIdx.x * 256ull + (threadIdx.x & ~63u); base < npairs; base += gridDim.x * 256ull) {
    const uint64_t p = base + lane; const bool active = p < npairs;
    const uint64_t k = head + 2 * p;                                         // the position of the pair's first index
    U64x2 v{0, 0};
    if (active) v = *(const U64x2*)(I + k);
    const uint32_t below = (uint32_t)__shfl_up((int)(uint32_t)v.b, 1, 64);
    if (active) {
      uint32_t prev = below; bool has_prev = true;
      if (lane == 0) { has_prev = k != 0; if (has_prev) prev = (uint32_t)I[k - 1]; }
      if (v.a >= dim || v.b >= dim) f |= IDX_OUT_OF_BOUNDS;
      if (v.b <= v.a || (has_prev && (uint32_t)v.a <= prev)) f |= IDX_NOT_INCREASING;
      *(U32x2*)(out + k) = U32x2{(uint32_t)v.a, (uint32_t)v.b};
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head) { const uint64_t a = I[0]; if (a >= dim) f |= IDX_OUT_OF_BOUNDS; out[0] = (uint32_t)a; }
    const uint64_t k = head + 2 * npairs;                                    // an odd rest: the last index
    if (k < n) {
      const uint64_t a = I[k];
      if (a >= dim) f |= IDX_OUT_OF_BOUNDS;
      if (k != 0 && (uint32_t)a <= (uint32_t)I[k - 1]) f |= IDX_NOT_INCREASING;
      out[k] = (uint32_t)a;
    }
  }
  const uint32_t wf = (__ballot(f & IDX_OUT_OF_BOUNDS) ? IDX_OUT_OF_BOUNDS : 0u) | (__ballot(f & IDX_NOT_INCREASING) ? IDX_NOT_INCREASING : 0u);
  if (lane == 0 && wf) atomicOr(status, wf);
}

template <class T> __global__ void k_index_widen(const T* __restrict__ x, uint64_t n, uint64_t* __restrict__ out) {
  for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < n; k += gridDim.x * 256ull) out[k] = (uint64_t)(int64_t)x[k];      // (unsigned T: zero-extended by the first cast)
}

}  // namespace

void index_parse_device(ExIdx& x, const GrB_Index* I, GrB_Index ni, uint64_t dim, const char* what) {
  if (!I) fail(GrB_NULL_POINTER, std::string(what) + ": index list is NULL");
  if (ni > (1ull << 40)) fail(GrB_INVALID_VALUE, std::string(what) + ": index count is not plausible");
  if (dim > GRB_DIM_DEVICE_MAX) fail(GrB_INVALID_VALUE, std::string(what) + ": the dimension is beyond the 32-bit device layout");      // (the order test compares narrowed words)
  if (((uintptr_t)I & 7u) != 0) fail(GrB_INVALID_VALUE, std::string(what) + ": a device index list must be 8-byte aligned");
  x.kind = EX_LIST; x.n = ni; x.hbm = true; x.increasing = true; x.host.clear();
  if (!ni) return;
  const uint32_t head = ((uintptr_t)I & 15u) ? 1u : 0u;
  x.own.alloc((ni + 4) * 4);                                                 // [0 .. head): padding, then the list, then the status word on its own 4 bytes
  uint32_t* list = x.own.as<uint32_t>() + head;                              // list + head is 8-byte aligned either way
  uint32_t* status = x.own.as<uint32_t>() + ni + 3;
  GRB_HIP(hipMemsetAsync(status, 0, 4, stream()));
  hipLaunchKernelGGL(k_index_parse, dim3(index_parse_grid(ni)), dim3(INDEX_PARSE_THREADS), 0, stream(), (const uint64_t*)I, (uint64_t)ni, dim, head, list, status);
  GRB_HIP(hipGetLastError());
  uint32_t* pin = (uint32_t*)pinned_scratch();
  GRB_HIP(hipMemcpyAsync(pin, status, 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  const uint32_t f = pin[0];
  if (f & IDX_OUT_OF_BOUNDS) { x.own.reset(); fail(GrB_INDEX_OUT_OF_BOUNDS, std::string(what) + ": index out of bounds"); }
  x.list = list; x.increasing = !(f & IDX_NOT_INCREASING);
}

void index_widen(int code, const void* x, uint64_t n, uint64_t* out) {
  if (!n) return;
  auto go = [&]<class T>() { hipLaunchKernelGGL((k_index_widen<T>), dim3(grid_1d(n)), dim3(256), 0, stream(), (const T*)x, n, out); };
  switch (code) {
    case T_INT8: go.template operator()<int8_t>(); break;     case T_UINT8: go.template operator()<uint8_t>(); break;
    case T_INT16: go.template operator()<int16_t>(); break;   case T_UINT16: go.template operator()<uint16_t>(); break;
    case T_INT32: go.template operator()<int32_t>(); break;   case T_UINT32: go.template operator()<uint32_t>(); break;
    case T_INT64: go.template operator()<int64_t>(); break;   case T_UINT64: go.template operator()<uint64_t>(); break;
    default: fail(GrB_DOMAIN_MISMATCH, "an index vector must have an integer type");
  }
  GRB_HIP(hipGetLastError());
}

}  // namespace grb
