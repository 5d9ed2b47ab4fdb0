// grb_spmv.hip — the SpMV / SpMSpV kernels behind GrB_mxv and GrB_vxm  (HBM-bound; no MFMA).
//
//   t(i) = (+)_j  mult(M(i,j), u(j))      M in CSR (u32 rowptr/col, sorted rows), u and t bitmap
//
// Three hand-written kernels, all wave64:
//  A  k_spmv_adaptive   row-block ("CSR-adaptive" style) pull kernel — the FP64 PLUS_TIMES
//                       north-star path.  A block of 256 threads owns a run of consecutive rows
//                       holding <= 2048 entries: col/val are read fully coalesced (every lane a
//                       consecutive entry, 8 independent loads in flight per lane before the
//                       first use), u is gathered (n*8 B = 32 MiB at R-MAT-22: L2/Infinity-Cache
//                       resident), products are staged in LDS and each row is reduced from LDS
//                       in a fixed left-to-right order (deterministic).  Rows longer than a
//                       block are split into 8192-entry parts; the last part to arrive combines
//                       the partials in part order (agent-scope fence + ticket, guide §6 G16).
//  B  k_spmv_rowgroup   G lanes per row with mask skip and monoid-terminal early exit — the
//                       pull step of BFS (complemented visited mask, LOR terminal).
//  C  k_spmspv_push     frontier-driven scatter with atomics — the push step when u is sparse.
// Algorithmic bytes per call: nnz*(sizeof(T)+4) + (nrows+1)*4 + ncols*T + nrows*T.
#include "grb_api.hpp"
#include "grb_compact.hpp"
#include "grb_semiring.hpp"
#include "grb_spmv.hpp"
#include "grb_spmv_xcd.hpp"
#include <vector>

namespace grb {

float g_xcd_plan_build_ms = 0;

// per-type kernel instantiations live in grb_spmv_inst.hip (compiled once per value type, in parallel)
template <class T> void run_pull(const SpmvCall& c, const SemiringDesc& d);
template <class T> void run_push(const SpmvCall& c, const SemiringDesc& d, const uint32_t* fidx, uint64_t u_nvals, uint32_t* longlist);

// ---- plan: greedy row blocking, once per matrix -------------------------------------------------------------
void spmv_build_plan(const DevCSR& M) {
  CsrDerived& D = M.derived;
  if (D.has_plan) return;
  std::vector<uint32_t> rp((size_t)M.nrows + 1);
  GRB_HIP(hipMemcpyAsync(rp.data(), M.rowptr.p, rp.size() * 4, hipMemcpyDeviceToHost, stream()));
  GRB_HIP(hipStreamSynchronize(stream()));
  std::vector<SpmvBlock> blocks; blocks.reserve(M.nnz / SPMV_NNZ * 2 + 16);
  uint32_t nslots = 0, nlong = 0;
  uint32_t r = 0; const uint32_t n = M.nrows;
  while (r < n) {
    const uint32_t len = rp[r + 1] - rp[r];
    if (len > (uint32_t)SPMV_NNZ) {
      const uint32_t parts = (len + SPMV_LONG_CHUNK - 1) / SPMV_LONG_CHUNK;
      for (uint32_t p = 0; p < parts; p++) blocks.push_back({r, p, parts, nslots});
      if (parts > 1) { nslots += parts; nlong++; }
      r++;
    } else {
      uint32_t e = r, tot = 0;
      while (e < n && e - r < (uint32_t)SPMV_MAX_ROWS) {
        const uint32_t l = rp[e + 1] - rp[e];
        if (tot + l > (uint32_t)SPMV_NNZ) break;
        tot += l; e++;
      }
      blocks.push_back({r, e, 0, 0});
      r = e;
    }
  }
  D.plan_nblocks = (uint32_t)blocks.size(); D.plan_nlong = nslots;
  D.plan_blocks.alloc(blocks.size() * sizeof(SpmvBlock) + 16);
  GRB_HIP(hipMemcpyAsync(D.plan_blocks.p, blocks.data(), blocks.size() * sizeof(SpmvBlock), hipMemcpyHostToDevice, stream()));
  // aux: [partials 8 B * nslots] [tickets u32 * nslots] [partial flags u8 * nslots]  (tickets indexed by `slot`; the 8-byte
  // partials come first so that they are 8-byte aligned whatever nslots is)
  const size_t aux = (size_t)(nslots + 1) * 8 + (size_t)(nslots + 1) * 4 + (size_t)(nslots + 1);
  D.plan_aux.alloc(aux);
  GRB_HIP(hipMemsetAsync(D.plan_aux.p, 0, aux, stream()));
  GRB_HIP(hipStreamSynchronize(stream()));
  D.has_plan = true;
}

bool spmv_rowlane_applies(const DevCSR& M, const SemiringDesc& d, int method) {
  if (method != SPMV_AUTO || !d.has_terminal) return false;
  const double avg = M.nrows ? (double)M.nnz / M.nrows : 0;
  static const bool no_lane = getenv("GRB_MI355X_NO_ROWLANE") && atoi(getenv("GRB_MI355X_NO_ROWLANE")) != 0;
  return avg <= 96 && !no_lane;
}

void spmv_pull(const SpmvCall& c, const SemiringDesc& d) {
  dispatch_type(d.zcode, [&]<class T>() { run_pull<T>(c, d); });
  GRB_HIP(hipGetLastError());
}

bool spmspv_push_supported(const SemiringDesc& d) {
  const int ts = type_size(d.zcode);
  if (d.zcode == T_BOOL) return d.addop == B_LOR || d.addop == B_ANY || d.addop == B_PLUS || d.addop == B_MAX;
  if (ts < 4) return false;
  if (d.addop == B_PLUS && (d.zcode == T_FP32 || d.zcode == T_FP64) && deterministic_env()) return false;      // floating-point sums by atomics: the pull kernels add in a fixed order
  return d.addop == B_PLUS || d.addop == B_MIN || d.addop == B_MAX;
}

void spmspv_push(const SpmvCall& c, const SemiringDesc& d, uint64_t u_nvals) {
  // c.M here is the CSR whose ROWS are indexed like u (i.e. the transpose of the pull operand)
  const DevCSR& M = *c.M; const uint64_t nu = M.nrows, nout = M.ncols;
  DevBuf pos, fidx((u_nvals + 1) * 4), longlist((u_nvals + 2) * 4);
  if (c.small_idx && c.small_n == u_nvals && u_nvals <= 64) {
    // the frontier is known on the host: its list travels as kernel arguments of run_push's first launch (k_push_init), which also clears
    // the presence bytes and the hub-row counter
  } else {
    GRB_HIP(hipMemsetAsync(longlist.p, 0, 4, stream()));
    // the indices of u's present entries, ascending -> fidx; nothing is read back (u_nvals is known)
    pos.alloc((nu + 1) * 4);
    present_positions(c.upres, nu, pos.as<uint32_t>());
    scatter_present(c.upres, pos.as<uint32_t>(), nu, 0, COMPACT_COL_INDEX, 0, fidx.as<uint32_t>(), 0, nullptr, nullptr);
    GRB_HIP(hipMemsetAsync(c.tpres, 0, nout ? nout : 1, stream()));
  }
  dispatch_type(d.zcode, [&]<class T>() { run_push<T>(c, d, fidx.as<uint32_t>(), u_nvals, longlist.as<uint32_t>()); });
  GRB_HIP(hipGetLastError());
}

}  // namespace grb

// ---- how a full-chip launch maps workgroups to XCDs ------------------------------------------------------------------------
// Kernel X gives workgroup b the column panel b % 8 and is fast when that workgroup runs on XCD b % 8 (every XCD's L2 then
// holds one eighth of the operand).  The round-robin dispatch is observed, not documented, and other partition modes deal
// differently — so it is probed once (XCC_ID of every workgroup of a one-workgroup-per-CU launch) and reported with the plan.
namespace grb {
static __global__ __launch_bounds__(1024) void k_xcc_probe(uint32_t* __restrict__ out) {
  uint32_t x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  if (threadIdx.x == 0) out[blockIdx.x] = x & 0xFu;
}
const std::string& xcd_mapping() {
  static std::string res;
  static const bool reprobe = getenv("GRB_MI355X_XCD_REPROBE") != nullptr;      // measurement hook: probe at every call (tools/xcd_probe.py)
  if (reprobe) res.clear();
  if (!res.empty() || !device_ok()) return res;
  const int ncu = device_cus();
  if (ncu <= 0) { res = "unknown"; return res; }
  DevBuf d((size_t)ncu * 4);
  hipLaunchKernelGGL(k_xcc_probe, dim3(ncu), dim3(1024), 0, stream(), d.as<uint32_t>());
  std::vector<uint32_t> h(ncu);
  if (hipMemcpyAsync(h.data(), d.p, (size_t)ncu * 4, hipMemcpyDeviceToHost, stream()) != hipSuccess || hipStreamSynchronize(stream()) != hipSuccess) { (void)hipGetLastError(); res = "unknown"; return res; }
  int match = 0; uint32_t seen = 0;
  for (int b = 0; b < ncu; b++) { match += (h[b] == (uint32_t)(b & 7)); seen |= 1u << h[b]; }
  const int nx = __builtin_popcount(seen);
  if (match == ncu) { res = "roundrobin8"; return res; }
  // a rotated deal (workgroup b on XCD (b + r) % 8: the dispatcher started at another XCD) serves kernel X as well: every panel still
  // has one XCD to itself for the launch
  for (int r = 1; r < 8; r++) {
    int m = 0; for (int b = 0; b < ncu; b++) m += (h[b] == (uint32_t)((b + r) & 7));
    if (m == ncu) { res = "roundrobin8+" + std::to_string(r); return res; }
  }
  res = "xcds=" + std::to_string(nx) + ",workgroups_on_xcd_b%8=" + std::to_string(match) + "/" + std::to_string(ncu);
  return res;
}
}  // namespace grb

extern "C" GrB_Info GrBX_last_plan_build_ms(float* ms) { if (!ms) return GrB_NULL_POINTER; *ms = grb::g_xcd_plan_build_ms; return GrB_SUCCESS; }
// ---- a read-only view of a matrix's kernel-X plan (tests/test_spmv_xcd_at_size_gpu.py asserts from it that a case reached the edge it was built for) ----
// Nothing here builds or changes a plan: the scalars are the plan's own fields, the per-stream numbers come out of its argument block, the per-tile
// words are copies of tinfo (16-bit column plane) or of trow plus the tiles' cold counts, counted from the 32-bit column words the plan keeps.
namespace grb {
constexpr uint64_t XF_HEAD = 24, XF_PER_STREAM = 4;
static const XcdPlan* xcd_plan_of(GrB_Matrix A, int transposed) {
  const DevCSR& R = transposed ? A->csc : A->csr;
  const XcdPlan* P = R.valid ? static_cast<const XcdPlan*>(R.derived.xcd.get()) : nullptr;
  return P && (P->tsize == 4 || P->tsize == 8) ? P : nullptr;
}
static uint32_t xcd_total_tiles(const XcdPlan* P) { return P->tbase[P->NS]; }
// 32-bit format: index of every tile's first cold entry among the cold entries of all tiles (what tinfo[2t + 1] is in the 16-bit format); returns their number
static uint64_t xcd_cold_prefix(const XcdPlan* P, std::vector<uint32_t>& first) {
  const uint32_t ntiles = xcd_total_tiles(P);
  first.assign((size_t)ntiles + 1, 0u);
  if (!ntiles || !P->pcol.p) return 0;
  DevBuf tcnt(((size_t)ntiles + 1) * 4);
  unsigned nb = (ntiles + 3) / 4; if (nb > 16384) nb = 16384;
  hipLaunchKernelGGL(k_xc_count, dim3(nb), dim3(256), 0, stream(), P->pcol.as<uint32_t>(), ntiles, 0u, tcnt.as<uint32_t>());
  std::vector<uint32_t> cnt(ntiles);
  GRB_HIP(hipMemcpyAsync(cnt.data(), tcnt.p, (size_t)ntiles * 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  uint64_t tot = 0;
  for (uint32_t t = 0; t < ntiles; t++) { first[t] = (uint32_t)tot; tot += cnt[t]; }
  first[ntiles] = (uint32_t)tot;
  return tot;
}
}  // namespace grb

extern "C" GrB_Info GrBX_Matrix_xcd_plan_facts(const GrB_Matrix A, int transposed, uint64_t* out, GrB_Index nout) {
  using namespace grb;
  if (!A || !out) return GrB_NULL_POINTER;
  if (!check_obj(A)) return GrB_UNINITIALIZED_OBJECT;
  const XcdPlan* P = xcd_plan_of(A, transposed);
  if (!P) return GrB_NO_VALUE;
  if (nout < XF_HEAD + XF_PER_STREAM * (uint64_t)P->NS) return GrB_INVALID_VALUE;
  try {
    const bool c16 = P->tsize == 8 ? xt_fmt<uint64_t>::C16 : xt_fmt<uint32_t>::C16;
    const uint64_t H = P->tsize == 8 ? (uint64_t)xt_hot<uint64_t>::H : (uint64_t)xt_hot<uint32_t>::H;
    const uint64_t HOT0 = P->tsize == 8 ? (uint64_t)xt_hot<uint64_t>::HOT : (uint64_t)xt_hot<uint32_t>::HOT;
    static_assert(sizeof(XtPanel<uint32_t>) == sizeof(XtPanel<uint64_t>), "the argument block has one layout for every value type");
    std::vector<XtPanel<uint64_t>> ha(XPMAX);
    GRB_HIP(hipMemcpyAsync((void*)ha.data(), P->args.p, sizeof(XtPanel<uint64_t>) * XPMAX, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
    uint64_t ncold = P->ncold;
    if (!c16) { std::vector<uint32_t> first; ncold = xcd_cold_prefix(P, first); }
    const uint64_t head[XF_HEAD] = {H, P->sell && HOT0 == H ? H - 1 : HOT0, (uint64_t)P->S, (uint64_t)P->NP, (uint64_t)P->NS, P->own ? 1u : 0u, P->F, ncold,
                                    (uint64_t)P->vbytes, P->has_vals ? 1u : 0u, P->m_ok ? 1u : 0u, P->m_wide ? 1u : 0u, P->m_nblocks, P->m_slots,
                                    (uint64_t)WP_ENT, WP_CHUNK, XM_ROWS, XM_TARGET, XM_SLOTS, (uint64_t)P->tsize, xcd_total_tiles(P), c16 ? 1u : 0u, XP_RB, P->sell ? 1u : 0u};
    for (uint64_t i = 0; i < XF_HEAD; i++) out[i] = head[i];
    for (int k = 0; k < P->NS; k++) {
      uint64_t* o = out + XF_HEAD + XF_PER_STREAM * (uint64_t)k;
      o[0] = P->ne[k]; o[1] = P->ntiles[k]; o[2] = P->nhot[k]; o[3] = ha[k].tiles_per_chunk;
    }
  } catch (...) { return GrB_PANIC; }
  return GrB_SUCCESS;
}
extern "C" GrB_Info GrBX_Matrix_xcd_plan_tiles(const GrB_Matrix A, int transposed, uint32_t* tiles, GrB_Index ntiles, uint32_t* bstart, GrB_Index nbstart) {
  using namespace grb;
  if (!A || !tiles) return GrB_NULL_POINTER;
  if (!check_obj(A)) return GrB_UNINITIALIZED_OBJECT;
  const XcdPlan* P = xcd_plan_of(A, transposed);
  if (!P) return GrB_NO_VALUE;
  const uint32_t nt = xcd_total_tiles(P);
  if (ntiles != nt || (bstart && P->m_ok && nbstart != (GrB_Index)P->m_nblocks + 1)) return GrB_INVALID_VALUE;
  try {
    if (P->tinfo.p) {
      if (nt) GRB_HIP(hipMemcpyAsync(tiles, P->tinfo.p, (size_t)nt * 8, hipMemcpyDeviceToHost, stream()));
    } else {
      if (!P->trow.p || !P->pcol.p) return GrB_NO_VALUE;
      std::vector<uint32_t> first, trow(nt);
      xcd_cold_prefix(P, first);
      if (nt) GRB_HIP(hipMemcpyAsync(trow.data(), P->trow.p, (size_t)nt * 4, hipMemcpyDeviceToHost, stream()));
      GRB_HIP(hipStreamSynchronize(stream()));
      for (uint32_t t = 0; t < nt; t++) { tiles[2 * (size_t)t] = trow[t]; tiles[2 * (size_t)t + 1] = first[t]; }
    }
    if (bstart && P->m_ok) GRB_HIP(hipMemcpyAsync(bstart, P->m_bstart.p, ((size_t)P->m_nblocks + 1) * 4, hipMemcpyDeviceToHost, stream()));
    GRB_HIP(hipStreamSynchronize(stream()));
  } catch (...) { return GrB_PANIC; }
  return GrB_SUCCESS;
}
extern "C" GrB_Info GrBX_xcd_mapping(char* buf, int len) {
  if (!buf || len <= 0) return GrB_NULL_POINTER;
  if (!grb::device_ok()) { snprintf(buf, len, "no device"); return GrB_NO_VALUE; }
  try { snprintf(buf, len, "%s", grb::xcd_mapping().c_str()); } catch (...) { snprintf(buf, len, "unknown"); }
  return GrB_SUCCESS;
}
