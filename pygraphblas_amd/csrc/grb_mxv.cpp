// grb_mxv.cpp — GrB_mxv and GrB_vxm: the SpMV half of the hot path.
//
// Replaces lib.GrB_mxv (reference call site pygraphblas/matrix.py:2714-2725, Matrix.mxv) and
// lib.GrB_vxm (pygraphblas/vector.py:960-970, Vector.vxm); semantics per SURVEY.md App. A:
//   w<mask,replace> = accum(w, op(A) (+).(x) u)         mxv: multiply is A(i,j) (x) u(j),  desc.INP0 transposes A
//   w'<mask',replace> = accum(w', u' (+).(x) op(A))     vxm: multiply is u(i) (x) A(i,j),  desc.INP1 transposes A
// Both are executed in "mxv orientation" t = M (+).(x) u with M = op(A) (mxv) or op(A)^T (vxm);
// whichever of CSR(A) / CSR(A^T) the chosen direction needs is taken from the matrix (the transpose
// is built once on the device and cached).
#include "grb_opcommon.hpp"
#include "grb_spmv.hpp"
#include "grb_lazy.hpp"
#include "grb_bigholes.hpp"
#include "grb_gemv.hpp"
#include "grb_spmm_geom.hpp"      // spmm_is_full
#include <cmath>
#include <algorithm>

using namespace grb;
static_assert(BH_INT32 == T_INT32 && BH_INT64 == T_INT64 && BH_FP32 == T_FP32 && BH_FP64 == T_FP64, "grb_bigholes.hpp names the type codes by number");

static int g_force_method = SPMV_AUTO;   // test hook: GRB_MI355X_SPMV=adaptive|rowgroup|push
// Where the next product on this thread writes T (round 6, grb_mxm_rows.cpp): a row of a batch matrix's bitmap.  The kernels write the row sums and presence
// bytes there instead of into fresh buffers, and when the write-back makes w exactly T — the batch products' case — w ends up as a VIEW of that row: the
// ns x (n values + n bytes) copies per product of the first bitmap version (3.8 of 14 ms of the BC driver at R-MAT-22) are gone.  One-shot: cleared by the call.
namespace grb { thread_local void* g_mxv_dest_val = nullptr; thread_local uint8_t* g_mxv_dest_pres = nullptr; }
// The next product on this thread is the compacted form of a hypersparse call (grb_hyper.cpp): it keeps the SpMV routes.  One-shot: cleared by the call.
namespace grb { thread_local bool g_mxv_compacted = false; }

// A semiring that does not run through SemiringDesc — user-defined, positional or comparison (SemiringRoute, grb_opcommon.hpp): one driver for all three.  What is refused before
// a device is asked for was refused by the caller; a user-defined semiring's layout refusal comes here, then the accumulator is looked at BEFORE the dimensions;
// the call is never queued and completes deferred work first.  T — unmasked, or under the allow bytes of any mask form — comes from the route's row kernel over
// the CSR of the orientation the built-in product pulls over (the cached transpose for vxm / GrB_INP0); operand values are cast into T's type (a comparison semiring: its multiplier's argument
// type) where the route reads them at all, and the argument order of the multiplier is the kernel's kind, not a flag.  The write-back is the built-in semirings' own.  A call that may
// write nothing (no mask + the complement flag) leaves the plan string empty.
static void off_table_mxv_like(const SemiringRoute& route, GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, GrB_Matrix A, GrB_Vector u, GrB_Descriptor desc, bool is_vxm) {
  route.refuse_after_device(no_layout(A, w, u, mask), "dimension or size");
  if (accum) check_binop(accum, "accum");
  const DescView dv(desc);
  const bool useT = is_vxm ? !dv.tran1 : dv.tran0;           // M = useT ? A^T : A
  const uint64_t mr = useT ? A->ncols : A->nrows, mc = useT ? A->nrows : A->ncols;
  if (u->n != mc || w->n != mr || (mask && mask->n != mr)) fail(GrB_DIMENSION_MISMATCH, "mxv/vxm: dimensions do not conform");
  lazy_flush(); vec_gate(w);
  const int product = is_vxm ? PK_VXM : PK_MXV;
  g_last_plan = route.plan(product);
  DevBuf allow_buf; bool nothing = false;
  const uint8_t* allow = vector_allow(mask, dv, mr, allow_buf, &nothing);
  if (nothing) { g_last_plan.clear(); if (dv.replace) GrB_Vector_clear(w); return; }
  mat_to_device(A); vec_to_device(u);
  const DevCSR& R = useT ? mat_csc(A) : A->csr;
  const int zc = route.zcode();
  DevBuf tval(mr * type_size(zc) + 16), tpres(mr + 16), ucast, acast;
  const void* av = route.operand_values(A->type->code, R.val.p, R.nnz, acast);
  const void* uv = route.operand_values(u->type->code, u->dval.p, u->n, ucast);
  route.rows(product, R, av, uv, u->dpres.as<uint8_t>(), allow, tval.p, tpres.as<uint8_t>());
  vector_write_back(w, zc, tval, tpres, allow, accum, dv.replace, /*t_only_allowed=*/true);
}

// The direction of a product (Beamer-style): push walks the rows of the frontier, pull scans the rows of the output.  Push is considered only for a sparse operand
// and a monoid with a native atomic; it is taken when the edges leaving the frontier (an exact count on the device) are < 1/16 of all entries.  Both operands are
// resident.  Counts u where that is needed, and records the edge count in u->facts.fe_lb / fe_lb_key.
struct Direction { bool push, tiny; uint64_t u_nvals; bool u_full; };      // tiny: pushed from the host's list of <= 64 entries; u_nvals: n - 1 ("has holes") where u was not counted
static Direction choose_direction(int method, const SemiringDesc& sd, GrB_Matrix A, GrB_Vector u, bool useT) {
  // the entry count of u and (for the direction choice below) the edges leaving it come from one kernel and one round
  // trip when the count is not known yet — the usual state inside a BFS loop, where u was just updated under a mask
  uint64_t fe_cached = ~0ull;
  bool stays_pull = false;            // the operand was too heavy for a push step when it was last counted and has only grown since
  // (masked products — the frontier-like operands of a BFS — and, since round 4, unmasked ones whose operand has an unknown count: the
  //  sweeps of the shortest-path loop, whose operand only gains entries; never build a transpose just for this)
  if (method == SPMV_AUTO && spmspv_push_supported(sd) && u->n && (useT || A->csc.valid)) {
    const DevCSR& P0 = useT ? A->csr : mat_csc(A);
    if (u->facts.fe_lb_key == P0.rowptr.serial && P0.rowptr.serial && u->facts.fe_lb * 16 >= P0.nnz + 16) stays_pull = true;      // no kernel, no host round trip (whether or not the count is known: `w.iseq(v)` of the shortest-path loop counts v)
    else if (!u->facts.dnvals_known) {
      uint64_t cnt = 0;
      fe_cached = frontier_edges_and_count(u->dpres.as<uint8_t>(), P0.rowptr.as<uint32_t>(), u->n, &cnt);
      u->facts.dnvals = cnt; u->facts.dnvals_known = true; u->facts.fe_lb = fe_cached; u->facts.fe_lb_key = P0.rowptr.serial; u->facts.fe_lb_true = false;
    }
  }
  const uint64_t u_nvals = stays_pull && !u->facts.dnvals_known ? (u->n ? u->n - 1 : 0) : vec_dev_nvals(u);             // (not counted: treated as "has holes")
  const bool u_full = u_nvals == u->n;
  bool push = false;
  // an operand of at most 64 entries known as a list on the host (the first level of a BFS): push without counting its edges — 64 rows,
  // the long ones split over all workgroups, are never worth a pull over every row of a large matrix
  const bool tiny = u->facts.small_valid && u->facts.small_idx.size() == u_nvals && u_nvals <= 64 && (uint64_t)A->csr.nnz >= (1u << 20) && (useT || A->csc.valid);
  if (method == SPMV_PUSH) push = spmspv_push_supported(sd);
  else if (method == SPMV_AUTO && !stays_pull && spmspv_push_supported(sd) && !u_full && u_nvals * 16 < (uint64_t)A->csr.nnz + 16) {
    if (tiny) push = true;
    else {
      const DevCSR& P = useT ? A->csr : mat_csc(A);
      const uint64_t fe = fe_cached != ~0ull ? fe_cached : frontier_edges(u->dpres.as<uint8_t>(), P.rowptr.as<uint32_t>(), u->n);
      push = fe * 16 < P.nnz + 16;
      u->facts.fe_lb = fe; u->facts.fe_lb_key = P.rowptr.serial; u->facts.fe_lb_true = false;                       // (exact now, a lower bound while entries are only added)
    }
  }
  return {push, tiny, u_nvals, u_full};
}

// "Big holes": a MIN_PLUS / MAX_PLUS product over an operand with holes and no mask (the sweeps of the reference's shortest-path
// loop, `v<accum MIN> = v MIN_PLUS A`: v has no entry for the vertices not reached yet).  The full-operand pipeline kernels cannot
// skip absent entries, and no value z makes a + z the monoid's identity for every a.  But when the values are small against the
// type's range, a BIG fill does the same job exactly: every sum that touches a hole lands beyond a threshold no real sum can
// reach, so "T(i) is an entry" is "T(i) is on the near side of the threshold" — one pass over the result.  Conditions (else the
// bitmap variant of the row-block kernel runs, as before): |A's values| and |u's values| below a quarter of BIG (integers: BIG =
// 2^(bits-2), so nothing wraps; floating point: BIG = infinity and every value finite, sums not overflowing), measured once per
// matrix and once per call.  R-MAT-22 INT64: 1.0 -> 0.3 ms per sweep.
// `eligible`: a pull over an operand with holes that the identity fill does not serve, no mask, no forced method.  The constants: grb_bigholes.hpp.
struct BigHoles { bool on; uint8_t fill[16], thresh[16]; double uabs, aabs; };
static BigHoles plan_big_holes(bool eligible, const SemiringDesc& sd, GrB_Matrix A, GrB_Vector u, bool useT, uint64_t u_nvals) {
  BigHoles big{false, {0}, {0}, 0, 0};
  if (!(eligible && !sd.flip && sd.mulop == B_PLUS && (sd.addop == B_MIN || sd.addop == B_MAX) &&
        (sd.zcode == T_INT32 || sd.zcode == T_INT64 || sd.zcode == T_FP32 || sd.zcode == T_FP64) && A->type->code == sd.zcode && u->type->code == sd.zcode)) return big;
  const DevCSR& R = useT ? mat_csc(A) : A->csr;
  if (!(R.nnz >= (1u << 20) && u_nvals * 64 >= u->n)) return big;                       // a product the pipeline kernels take, an operand that is not nearly empty
  uint8_t mn[8], mx[8]; uint64_t bad = 0, cnt = 0;
  if (R.derived.range_state == 0) {                       // the matrix's range: measured once, cached with the CSR
    R.derived.range_state = 2;
    if (value_range(sd.zcode, R.nnz, R.val.p, nullptr, mn, mx, &bad, &cnt) && bad == 0 && cnt) { R.derived.range_abs = range_abs_of(sd.zcode, mn, mx); R.derived.range_state = 1; }
  }
  if (R.derived.range_state != 1) return big;
  bad = 0; cnt = 0;
  const bool bound_known = u->facts.abs_bound >= 0 && u->lazy == 0 && u->dev_valid;          // left by the previous sweep: no kernel, no read-back
  if (!bound_known && !(value_range(sd.zcode, u->n, u->dval.p, u->dpres.as<uint8_t>(), mn, mx, &bad, &cnt) && bad == 0 && cnt)) return big;
  big.uabs = bound_known ? std::fabs(u->facts.abs_bound) : range_abs_of(sd.zcode, mn, mx); big.aabs = R.derived.range_abs;
  const BigHolesConstants c = big_holes_constants(sd.zcode, sd.addop == B_MIN, big.aabs, big.uabs);
  big.on = c.admitted; memcpy(big.fill, c.fill, 16); memcpy(big.thresh, c.thresh, 16);
  return big;
}

// ---- the gemv_full route: A holds every position (judged on its own device image, queued edits applied) — a linear model's scores X w, the two halves X'(X w) of a
// power iteration, GAT's logits H a.  One more producer of (tval, tpres): both layouts read A's OWN value array (grb_gemv.hpp) — no column words, no SpMV plan and,
// for vxm and GrB_INP0, no transposed copy of a dense matrix.  T is computed at every position and the write-back filters it through the allow bytes; the fused
// epilogues, the hole fills, the code bytes, the any_true word and the frontier-edge summary of the sparse path are not used and nothing of them is acquired.
// GRB_MI355X_GEMV (read per call: a test hook, and the yardstick of tools/gemv_probe.py): 0 never, 1 wherever legal; by itself where gemv_by_default
// admits the shape (grb_gemv_geom.hpp, GEMV_FULL_MIN_WORK of grb_route.hpp: the measured wins).  A kernel asked for by name (GRB_MI355X_SPMV, g_force_method), the Boolean `mask == u` form of the BFS loop and a product whose T goes into a
// batch matrix's row keep their routes.
static bool gemv_full_wanted(GrB_Matrix A, int method, bool mask_is_u, bool useT, bool compacted) {
  if (compacted || method != SPMV_AUTO || mask_is_u || g_mxv_dest_val || g_mxv_dest_pres || !A->csr.valid) return false;
  if (!spmm_is_full(A->csr.nrows, A->csr.ncols, A->csr.nnz)) return false;
  const int env = route_env("GRB_MI355X_GEMV");
  return env >= 0 ? env == 1 : gemv_by_default(A->csr.nrows, A->csr.ncols, useT, GEMV_FULL_MIN_WORK);
}
static void gemv_full_route(GrB_Vector w, const uint8_t* allow, GrB_BinaryOp accum, const SemiringDesc& sd, GrB_Matrix A, GrB_Vector u, bool useT, uint64_t mr, uint64_t mc, bool replace) {
  if (w->lazy) vec_gate(w);                                   // a pending `w(:) = s`: written now, the write-back reads it
  const uint64_t u_nvals = vec_dev_nvals(u);
  const size_t zs = type_size(sd.zcode);
  DevBuf tval(mr * zs + 16), tpres(mr + 16), ucast, acast;
  GemvPlan p; p.m = mr; p.k = mc; p.layout = useT ? GEMV_T : GEMV_N; p.holes = u_nvals != u->n; p.chunks = 0;
  bool cast = false;
  if (u_nvals == 0) GRB_HIP(hipMemsetAsync(tpres.p, 0, mr, stream()));      // no product exists: T is empty, no launch
  else {
    const bool uses_a = sd.flip ? binop_uses_y(sd.mulop) : binop_uses_x(sd.mulop), uses_u = sd.flip ? binop_uses_x(sd.mulop) : binop_uses_y(sd.mulop);
    const void* av = uses_a ? cast_values(sd.zcode, A->type->code, A->csr.val.p, A->csr.nnz, acast) : nullptr;
    const void* uv = uses_u ? cast_values(sd.zcode, u->type->code, u->dval.p, u->n, ucast) : nullptr;
    cast = (uses_a && A->type->code != sd.zcode) || (uses_u && u->type->code != sd.zcode);
    gemv_full(p.layout, mr, mc, av, uv, u_nvals == u->n ? nullptr : u->dpres.as<uint8_t>(), sd, tval.p, p);
    GRB_HIP(hipMemsetAsync(tpres.p, 1, mr, stream()));
  }
  g_last_plan = "gemv_full<m=" + std::to_string(p.m) + ",k=" + std::to_string(p.k) + ",layout=" + (p.layout == GEMV_T ? "T" : "N") + ",holes=" + (p.holes ? "1" : "0") +
                ",chunks=" + std::to_string(p.chunks) + ",cast=" + (cast ? "1" : "0") + "> " + (u_nvals ? std::string(p.kernel) + " " + (p.chunks > 1 ? "k_gemv_fold " : "") : std::string());
  vector_write_back(w, sd.zcode, tval, tpres, allow, accum, replace, /*t_only_allowed=*/false, u_nvals ? mr : 0);
}

static void mxv_like(GrB_Vector w, GrB_Vector mask, GrB_BinaryOp accum, GrB_Semiring semiring, GrB_Matrix A, GrB_Vector u,
                     GrB_Descriptor desc, bool is_vxm) {
  const bool compacted = g_mxv_compacted; g_mxv_compacted = false;
  const SemiringRoute route = semiring_route(semiring);
  const bool initialised = check_obj(w) && check_obj(A) && check_obj(u) && (!mask || check_obj(mask));
  if (route.off_table()) {
    const NoLayout nl = initialised ? no_layout(A, w, u, mask) : NoLayout{};
    route.refuse_before_device(initialised ? &nl : nullptr, accum);
  }
  need_device();
  if (!initialised) fail(GrB_UNINITIALIZED_OBJECT, "mxv/vxm: uninitialised operand");
  if (route.off_table()) { off_table_mxv_like(route, w, mask, accum, A, u, desc, is_vxm); return; }
  if (is_hyper(A) || is_hyper(w) || is_hyper(u) || is_hyper(mask)) { hyper_mxv_like(w, mask, accum, semiring, A, u, desc, is_vxm); return; }   // dimensions beyond the device layouts
  if (w->q_reads || w->lazy == 2) vec_gate(w);                // deferred element-wise work on the output completes first (a pending fill, lazy == 1, is dealt with below)
  const DescView dv(desc);
  const bool useT = is_vxm ? !dv.tran1 : dv.tran0;           // M = useT ? A^T : A
  const uint64_t mr = useT ? A->ncols : A->nrows, mc = useT ? A->nrows : A->ncols;
  if (u->n != mc || w->n != mr || (mask && mask->n != mr)) fail(GrB_DIMENSION_MISMATCH, "mxv/vxm: dimensions do not conform");
  SemiringDesc sd = make_semiring_desc(semiring, /*swap_mult_args=*/is_vxm);
  const char* env = getenv("GRB_MI355X_SPMV");
  int method = g_force_method;
  if (env) method = !strcmp(env, "adaptive") ? SPMV_ADAPTIVE : !strcmp(env, "rowgroup") ? SPMV_ROWGROUP : !strcmp(env, "push") ? SPMV_PUSH : !strcmp(env, "wavepipe") ? SPMV_WAVEPIPE : !strcmp(env, "xcd") ? SPMV_XCD : SPMV_AUTO;
  g_last_plan.clear();

  DevBuf allow_buf, ubool; bool nothing = false;
  const uint8_t* allow = nullptr;
  // the mask is also the operand and the semiring is Boolean (`v.vxm(A, mask=v, desc=RC)` on the UINT8 level vector of a BFS): its allow
  // bytes and its values as BOOL come out of ONE pass instead of a k_allow and a k_cast — made below, once the direction is known: the
  // masked pull of a one-byte vector reads the vector itself and needs neither (SpmvCall::fm_val)
  const bool mask_is_u = mask && mask == u && sd.zcode == T_BOOL && u->type->code != T_BOOL && mr;
  if (mask_is_u) vec_to_device(u);
  else allow = vector_allow(mask, dv, mr, allow_buf, &nothing);
  if (nothing) {   // no mask + complement: nothing may be written; replace clears w
    if (dv.replace) { w->hi.clear(); w->hx.clear(); w->pending.clear(); w->host_valid = true; vec_invalidate_device(w); }
    return;
  }
  mat_to_device(A); vec_to_device(u);
  if (mr && mc && gemv_full_wanted(A, method, mask_is_u, useT, compacted)) { gemv_full_route(w, allow, accum, sd, A, u, useT, mr, mc, dv.replace); return; }
  const auto [push, tiny, u_nvals, u_full] = choose_direction(method, sd, A, u, useT);

  // does the multiply read the matrix / vector values at all?
  const bool uses_a = sd.flip ? binop_uses_y(sd.mulop) : binop_uses_x(sd.mulop);
  const bool uses_u = sd.flip ? binop_uses_x(sd.mulop) : binop_uses_y(sd.mulop);

  bool fused_mask = false, excl_small = false;
  if (mask_is_u) {
    // (the pull operand — for vxm the cached transpose, built on first need — is looked at only when the product pulls: a BFS that
    //  stays in push for every level never pays for a transpose it does not use)
    fused_mask = !push && !accum && dv.replace && type_size(u->type->code) == 1 && spmv_rowlane_applies(useT ? mat_csc(A) : A->csr, sd, method);
    // the first level of a BFS: the operand is a short list known on the host, it is also the (complemented) mask and every listed value is true — the
    // push kernels skip the listed positions themselves and multiply by `true`: no allow bytes, no BOOL copy of the operand (a pass over all positions)
    // (only for `w<!u, replace> = ...` without an accumulator, like the fused pull: with `allow == nullptr` the write-back makes w exactly T, which is
    //  right only when the listed positions are to be deleted anyway and nothing of w's old content survives — ADVICE round 5)
    excl_small = !fused_mask && push && tiny && !accum && dv.replace && dv.mask_comp && u->facts.small_truthy;
    if (!fused_mask && !excl_small) {
      allow_buf.alloc(mr); ubool.alloc(mr + 1);
      build_allow_and_bool(mr, u->type->code, u->dval.p, u->dpres.as<uint8_t>(), dv.mask_struct, dv.mask_comp, allow_buf.as<uint8_t>(), ubool.as<uint8_t>());
      allow = allow_buf.as<uint8_t>();
    }
  }
  const size_t zs = type_size(sd.zcode);
  DevBuf tval, tpres, ucast, acast;
  if (g_mxv_dest_val && g_mxv_dest_pres) { tval.borrow(g_mxv_dest_val, mr * zs); tpres.borrow(g_mxv_dest_pres, mr); } else { tval.alloc(mr * zs + 1); tpres.alloc(mr + 1); }
  g_mxv_dest_val = nullptr; g_mxv_dest_pres = nullptr;
  // An operand with holes whose product is accumulated into a full vector with the monoid's own operator, no mask (PageRank:
  // r<accum PLUS> += A' (+).second w, w = t / d has no entry for dangling vertices — gap/prmark.py:21-23): where T has no
  // entry the output keeps its value, and where T's entries would come from absent operand entries only, accumulating the
  // monoid's identity keeps it too.  So the pattern of T does not matter, and the holes can be filled with a value z for
  // which mult(a, z) is the identity — z = identity for SECOND (any monoid), 0 for integer PLUS_TIMES, false for LOR_LAND —
  // in the same pass that casts the operand; the product then runs as a full-operand one (kernel X / W instead of the
  // bitmap variant of the row-block kernel: 0.60 -> 0.17 ms at R-MAT-22).
  // w is full: resident in HBM with every position present, or `w(:) = s` was requested and not written yet (non-blocking mode, grb_lazy.cpp)
  const bool w_fill = w->lazy == 1 && w != u && w != mask;
  const bool w_full = w_fill || (w->lazy == 0 && w->dev_valid && !w->host_valid && w->facts.dnvals_known && w->facts.dnvals == w->n && w != u);
  const bool accum_is_monoid = !mask && accum && check_obj(accum) && accum->opcode == sd.addop && accum->xtype->code == sd.zcode && accum->ytype->code == sd.zcode &&
                               accum->ztype->code == sd.zcode && w->type->code == sd.zcode;
  bool fill_holes = false;
  if (!push && !u_full && accum_is_monoid && method == SPMV_AUTO && !sd.flip && w_full) {
    const bool is_int = sd.zcode != T_FP32 && sd.zcode != T_FP64 && sd.zcode != T_BOOL;
    // (the accumulator must leave w alone when it meets the identity: true for these monoid operators, not for ANY)
    const bool neutral = sd.addop == B_PLUS || sd.addop == B_TIMES || sd.addop == B_MIN || sd.addop == B_MAX || sd.addop == B_LOR || sd.addop == B_LAND || sd.addop == B_LXOR;
    fill_holes = neutral && (sd.mulop == B_SECOND || (sd.mulop == B_TIMES && sd.addop == B_PLUS && is_int) || (sd.mulop == B_LAND && sd.addop == B_LOR && sd.zcode == T_BOOL));
  }
  const BigHoles big = plan_big_holes(!push && !u_full && !fill_holes && !allow && method == SPMV_AUTO, sd, A, u, useT, u_nvals);
  const void* uval = nullptr;
  const bool zero_fill = [&] { for (size_t b = 0; b < zs; b++) if (sd.identity[b]) return false; return true; }();
  if (uses_u && fill_holes && u->facts.holes_zero && u->type->code == sd.zcode && zero_fill) {
    uval = u->dval.p;                                     // written by the element-wise chain kernel with zeros in the holes: no pass at all
  } else if (big.on) {
    // the fill goes into u's OWN buffer (the values of absent positions are nobody's business: holes_zero is dropped) and is remembered: the
    // sweeps of the shortest-path loop only add entries — real values, written by the merge's store — so from the second sweep on the operand
    // is ready as it stands (a cast-and-fill pass over the vector per sweep before: 18 us of 357 at R-MAT-22)
    // (the operand is an INPUT: its stored entries never change, only the bytes behind its holes do — a write all the same.  Not while queued work
    //  still reads the vector, nor while an exchange writes into vector buffers on the second stream: then the fill goes into a copy, as before round 4)
    if (u->facts.holes_big && memcmp(u->facts.holes_big_val, big.fill, zs) == 0) uval = u->dval.p;
    else if (u->q_reads || dist_exchange_pending()) {
      ucast.alloc(u->n * zs + 1);
      vec_cast_fill_values(sd.zcode, ucast.p, u->type->code, u->dval.p, u->dpres.as<uint8_t>(), u->n, big.fill);
      uval = ucast.p;
    } else {
      vec_cast_fill_values(sd.zcode, u->dval.p, u->type->code, u->dval.p, u->dpres.as<uint8_t>(), u->n, big.fill);      // (same type: plan_big_holes requires it; element-wise, in place)
      u->facts.holes_hold(big.fill);
      uval = u->dval.p;
    }
  } else if (uses_u && fill_holes) {
    ucast.alloc(u->n * zs + 1);
    vec_cast_fill_values(sd.zcode, ucast.p, u->type->code, u->dval.p, u->dpres.as<uint8_t>(), u->n, sd.identity);   // (identity of PLUS / LOR is the 0 / false the two other cases need)
    uval = ucast.p;
  } else if (uses_u && (fused_mask || excl_small)) uval = nullptr;  // (the kernel reads the vector's own bytes / takes every operand value as true)
  else if (uses_u) uval = ubool.p ? ubool.p : cast_values(sd.zcode, u->type->code, u->dval.p, u->n, ucast);

  SpmvCall call{};
  call.uval = uval; call.allow = allow; call.tval = tval.p; call.tpres = tpres.as<uint8_t>(); call.method = method;
  // a BOOL result that replaces w: the kernel notes whether it wrote a true value, and the `q.reduce_bool()` that follows a BFS
  // level (tests/test_bfs.py loop: `while q.reduce_bool() and level <= n`) reads that word instead of scanning q
  bool any_done = false;
  bool fe_done = false; uint64_t fe_key = 0; uint32_t fe_nblocks = 0;
  if (sd.zcode == T_BOOL && w->type->code == T_BOOL && !accum && method == SPMV_AUTO) {
    call.any_true = any_true_acquire(&call.any_true_tag); call.any_true_done = &any_done;
    // ... and, on a square matrix, the edges leaving the result's true entries in the row pointers the direction choice above counts in:
    // the product after `v[q] = level` then knows its operand is too heavy for a push step without counting (SpmvCall::fe_slots)
    if (mr == mc && (useT || A->csc.valid)) {
      const DevCSR& P0 = useT ? A->csr : mat_csc(A);
      if (P0.nrows == mr && P0.rowptr.serial) { call.fe_rowptr = P0.rowptr.as<uint32_t>(); call.fe_host = fe_summary_host(); call.fe_done = &fe_done; call.fe_nblocks = &fe_nblocks; fe_key = P0.rowptr.serial; }
    }
  }
  const void* const tkey = tval.p;
  if (push) {
    // push walks rows of M^T:  M^T = useT ? A : A^T
    const DevCSR& P = useT ? A->csr : mat_csc(A);
    call.M = &P; call.upres = u->dpres.as<uint8_t>();
    if (u->facts.small_valid && u->facts.small_idx.size() == u_nvals) { call.small_idx = u->facts.small_idx.data(); call.small_n = (uint32_t)u_nvals; call.excl_small = excl_small; }
    call.aval = uses_a ? cast_values(sd.zcode, A->type->code, P.val.p, P.nnz, acast) : nullptr;
    spmspv_push(call, sd, u_nvals);
  } else {
    const DevCSR& R = useT ? mat_csc(A) : A->csr;
    call.M = &R; call.upres = (u_full || fill_holes || big.on) ? nullptr : u->dpres.as<uint8_t>();
    if (fused_mask) {
      call.upres = u->dpres.as<uint8_t>(); call.fm_val = u->dval.as<uint8_t>(); call.fm_flags = (uint8_t)((dv.mask_struct ? 1 : 0) | (dv.mask_comp ? 2 : 0));
      // the vector's code bytes (one gather per neighbour instead of two): left behind by the masked assign that wrote it (`v[q] = level`), else made by one pass
      // over the vector when the matrix is large enough for the pull to repay it (GRB_MI355X_CODE_BYTES=0: never)
      const char* ce = getenv("GRB_MI355X_CODE_BYTES"); const bool code_off = ce && atoi(ce) == 0;      // (read per call: a test hook)
      if (!code_off && u->n >= (1u << 16) && R.nnz >= (1u << 20)) {
        if (!u->facts.code_valid) {
          if (!u->dcode.p || u->dcode.bytes < u->n + 16) u->dcode.alloc(u->n + 16);
          vec_code_bytes(u->n, u->dval.as<uint8_t>(), u->dpres.as<uint8_t>(), u->dcode.as<uint8_t>());
          u->facts.code_valid = true;
        }
        call.fm_code = u->dcode.as<uint8_t>();
      }
    }
    call.aval = uses_a ? cast_values(sd.zcode, A->type->code, R.val.p, R.nnz, acast) : nullptr;
    // `w += M (+).(x) u` with the monoid's own operator into a full w, no mask: the kernel that writes the row sums can apply the
    // accumulator in the same store — and when w is a fill that was never written (`r[:] = teleport` before the product of
    // gap/prmark.py:21-23), the fill folds into that store too and w is never read
    bool epi_done = false;
    if (accum_is_monoid && w_full && method == SPMV_AUTO && !big.on) {       // (with big holes every row has a sum: the threshold must see it first — epi 3)
      call.epi = w_fill ? 2 : 1; call.epi_w = w_fill ? nullptr : w->dval.p; call.epi_done = &epi_done;
      if (w_fill) memcpy(call.epi_fill, w->lazy_fill, 16);
    }
    // big holes + `w<accum MIN> = ...` with the monoid's own operator (the sweeps of the shortest-path loop, `v.vxm(A, MIN_PLUS, accum=MIN, out=v)`):
    // the merge kernel applies the threshold and the accumulator in its store — no threshold pass over T, no accumulate epilogue, no T at all
    const bool big_epi = big.on && accum_is_monoid && method == SPMV_AUTO && w->lazy == 0 && !w->q_reads;
    if (big_epi) {
      vec_to_device(w);
      call.epi = 3; call.epi_w = w->dval.p; call.epi_wpres = w->dpres.as<uint8_t>(); memcpy(call.epi_fill, big.thresh, 16); call.epi_done = &epi_done;
    }
    spmv_pull(call, sd);
    if (epi_done && call.epi == 3) {
      const bool keep_big = w == u && u->facts.holes_big; uint8_t held[16]; memcpy(held, u->facts.holes_big_val, 16);
      vec_device_extended(w);                       // (entries were only added: the lower bound fe_lb of the edges leaving them stays valid — the next sweep needs no count)
      if (keep_big) w->facts.holes_hold(held);      // (the store wrote real values into former holes, nothing else: the others still hold the fill)
      if (w == u) w->facts.abs_bound = big.uabs + big.aabs;       // every sum that passed the threshold is within |u| + |A|; MIN / MAX select among such values and w's own
      return;
    }
    if (epi_done) {
      if (w_fill) {
        lazy_fill_consumed(w);
        w->dval = std::move(tval); w->dpres = std::move(tpres);
        w->dev_valid = true; w->host_valid = false; w->hi.clear(); w->hx.clear(); w->pending.clear();
        w->facts.image_replaced(w->n, true);
      } else vec_invalidate_host(w, w->n, true);
      return;
    }
  }
  if (big.on) big_to_absent(sd.zcode, mr, tval.p, tpres.as<uint8_t>(), big.thresh, sd.addop == B_MIN);       // sums made of fill values only are no entries
  const bool w_is_u = w == u; const bool w_was_empty = !w_is_u && w->lazy == 0 && w->facts.dnvals_known && w->facts.dnvals == 0 && !w->host_valid;
  vector_write_back(w, sd.zcode, tval, tpres, allow, accum, dv.replace, /*t_only_allowed=*/true);
  // every sum that survived the threshold is within |u| + |A|: the bound of the result when w held nothing else (w was empty / is
  // replaced as a whole), or when w is u itself and the accumulator SELECTS one of its arguments (`v<accum MIN> = v MIN_PLUS A`: MIN,
  // MAX, FIRST, SECOND, ANY).  An arithmetic accumulator (PLUS, TIMES ...) can leave |w| beyond it: then no bound is recorded and the
  // next sweep measures the range again.
  const bool accum_selects = accum && check_obj(accum) && (accum->opcode == B_MIN || accum->opcode == B_MAX || accum->opcode == B_FIRST || accum->opcode == B_SECOND || accum->opcode == B_ANY);
  if (big.on && w->type->code == sd.zcode && (!accum || w_was_empty || (w_is_u && accum_selects))) w->facts.abs_bound = big.uabs + big.aabs;
  if (any_done) any_true_written(w->lazy == 0 && w->dev_valid && w->dval.p == tkey ? w : nullptr, tkey, call.any_true_tag, fe_done ? fe_key : 0, fe_nblocks);       // (adopted as they are: w is exactly T)
}

extern "C" {

GrB_Info GrB_mxv(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Semiring semiring,
                 const GrB_Matrix A, const GrB_Vector u, const GrB_Descriptor desc) {
  if (!w || !A || !u || !semiring) return GrB_NULL_POINTER;
  if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] { mxv_like(w, mask, accum, semiring, A, u, desc, false); });
}

GrB_Info GrB_vxm(GrB_Vector w, const GrB_Vector mask, const GrB_BinaryOp accum, const GrB_Semiring semiring,
                 const GrB_Vector u, const GrB_Matrix A, const GrB_Descriptor desc) {
  if (!w || !A || !u || !semiring) return GrB_NULL_POINTER;
  if (!check_obj(w)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(w, [&] { mxv_like(w, mask, accum, semiring, A, u, desc, true); });
}

}  // extern "C"
