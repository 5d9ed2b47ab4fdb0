// grb_hostmap.hpp — the host-mirror model that every host route of the container operations shares (grb_extract_ops.cpp, grb_assign_ops.cpp, grb_kron_ops.cpp,
// grb_diag_ops.cpp, grb_sort_ops.cpp): a container as a map from position to value bytes, or as a line of its sorted tuples.
//
// None of this is on the hot path (mxm / mxv / vxm and the O(n) / O(nnz) operations of the BFS, PageRank and
// triangle-count loops, all HIP): it is the element-wise container surface — notebook slicing `M[2]`, `v[1:3]`,
// `M[1, :] = v` — beside setElement / extractElement, and like those it edits the host mirror of the container (sorted
// tuples); the HBM image is rebuilt lazily the next time a kernel needs it.  Semantics: C API 1.3: T is
// formed, then C<M,replace> = accum(C, T); for assign the mask spans all of C (GrB_assign), for row / column assign only that
// row / column.  Also here: the words of the device routes' plan strings (kind_name, parse_name, accum_name) and HostList, the way a list in HBM reaches a host route.
#pragma once
#include "grb_opcommon.hpp"
#include "grb_extract.hpp"
#include <algorithm>
#include <array>
#include <map>

namespace grb {
namespace hostmap {

typedef std::array<uint8_t, 16> Val;
typedef std::map<std::pair<uint64_t, uint64_t>, Val> Map;     // (row, column) -> value bytes in some type

inline Map load(GrB_Matrix A, bool transpose) {
  mat_to_host(A); Map m; const size_t ts = A->type->size;
  for (size_t p = 0; p < A->hi.size(); p++) { Val v{}; memcpy(v.data(), &A->hx[p * ts], ts); m[transpose ? std::make_pair(A->hj[p], A->hi[p]) : std::make_pair(A->hi[p], A->hj[p])] = v; }
  return m;
}
inline Map load(GrB_Vector u) {
  vec_to_host(u); Map m; const size_t ts = u->type->size;
  for (size_t p = 0; p < u->hi.size(); p++) { Val v{}; memcpy(v.data(), &u->hx[p * ts], ts); m[{u->hi[p], 0}] = v; }
  return m;
}
inline void store(GrB_Matrix C, const Map& m) {
  const size_t ts = C->type->size;
  C->hi.clear(); C->hj.clear(); C->hx.clear(); C->pending.clear();
  for (auto& kv : m) { C->hi.push_back(kv.first.first); C->hj.push_back(kv.first.second); C->hx.insert(C->hx.end(), kv.second.data(), kv.second.data() + ts); }
  C->host_valid = true; mat_invalidate_device(C);
}
inline void store(GrB_Vector w, const Map& m) {
  const size_t ts = w->type->size;
  w->hi.clear(); w->hx.clear(); w->pending.clear();
  for (auto& kv : m) { w->hi.push_back(kv.first.first); w->hx.insert(w->hx.end(), kv.second.data(), kv.second.data() + ts); }
  w->host_valid = true; vec_invalidate_device(w);
}
inline Val cast(int dst, int src, const Val& v) { Val o{}; cast_scalar(dst, o.data(), src, v.data()); return o; }
inline bool truth(int code, const Val& v) { Val b = cast(T_BOOL, code, v); return b[0] != 0; }
inline Val combine(GrB_BinaryOp op, int ccode, const Val& c, int tcode, const Val& t) {          // accum(c, t) in the operator's domain, result in C's type
  const int ac = op->xtype->code; if (ac >= T_FC32) fail(GrB_DOMAIN_MISMATCH, "operators on complex values are out of scope");
  Val a = cast(ac, ccode, c), b = cast(ac, tcode, t), z{};
  dispatch_type(ac, [&]<class T>() { T x, y; memcpy(&x, a.data(), sizeof(T)); memcpy(&y, b.data(), sizeof(T)); T r = apply_binop<T>(op->opcode, x, y); memcpy(z.data(), &r, sizeof(T)); });
  return cast(ccode, op->ztype->code, z);
}
struct MaskView { const Map* m; int code; bool structural, comp, present;
  bool allows(const std::pair<uint64_t, uint64_t>& p) const {
    if (!present) return !comp;
    auto it = m->find(p); const bool t = it != m->end() && (structural || truth(code, it->second));
    return t != comp;
  } };

// C<M,replace> = accum(C, T) on maps.  `in_scope(p)`: positions the mask / replace step may touch (all of C, or one row / column)
template <class Scope> void write_back(Map& C, int ccode, const Map& T, int tcode, const MaskView& mk, bool replace, GrB_BinaryOp accum, Scope in_scope) {
  if (accum) check_binop(accum, "accum");
  Map Z;
  if (accum) {
    Z = C;
    for (auto& kv : T) { auto it = Z.find(kv.first); if (it == Z.end()) Z[kv.first] = cast(ccode, tcode, kv.second); else it->second = combine(accum, ccode, it->second, tcode, kv.second); }
  } else for (auto& kv : T) Z[kv.first] = cast(ccode, tcode, kv.second);
  Map out;
  for (auto& kv : C) { const bool scope = in_scope(kv.first); if (!scope || (!mk.allows(kv.first) && !replace)) out[kv.first] = kv.second; }   // what survives untouched
  for (auto& kv : Z) if (in_scope(kv.first) && mk.allows(kv.first)) out[kv.first] = kv.second;
  C.swap(out);                                                          // (outside the scope Z == C under an accumulator: already kept)
}
inline bool everywhere(const std::pair<uint64_t, uint64_t>&) { return true; }
template <class M> MaskView mask_view(const Map& Mm, const M* mask, const DescView& dv) { return MaskView{&Mm, mask ? mask->type->code : 0, dv.mask_struct, dv.mask_comp, mask != nullptr}; }

inline bool strictly_increasing(const std::vector<uint64_t>& v) { for (size_t k = 1; k < v.size(); k++) if (v[k] <= v[k - 1]) return false; return true; }
// an index list that is never materialised when it is GrB_ALL (the identity map): the default-dimension (2^60) hypersparse
// containers are sliced with it (`H[1]`, `H[:, 2]`), and a vector of `dim` indices cannot exist there
struct Sel {
  bool all = false; uint64_t dim = 0; std::vector<uint64_t> v;
  Sel(const GrB_Index* I, GrB_Index ni, uint64_t d, const char* what) : all(I == GrB_ALL), dim(d) { if (!all) v = expand_index_list(I, ni, d, what); }
  uint64_t size() const { return all ? dim : v.size(); }
  bool increasing() const { return all || strictly_increasing(v); }
  // position of source index x in an increasing list, or ~0
  uint64_t find_sorted(uint64_t x) const { if (all) return x < dim ? x : ~0ull; const auto a = std::lower_bound(v.begin(), v.end(), x); return (a == v.end() || *a != x) ? ~0ull : (uint64_t)(a - v.begin()); }
};
inline void check_m(GrB_Matrix A, const char* w) { if (!check_obj(A)) fail(GrB_UNINITIALIZED_OBJECT, std::string(w) + ": uninitialised matrix"); }
inline void check_v(GrB_Vector A, const char* w) { if (!check_obj(A)) fail(GrB_UNINITIALIZED_OBJECT, std::string(w) + ": uninitialised vector"); }

// ---- the common slices on the sorted tuples themselves (no map of the whole matrix): `M[i]`, `M[:, j]`, `M[i] = v`, `M[a:b, c:d]` ----
typedef std::vector<std::pair<uint64_t, Val>> Line;                     // (index, value bytes), sorted by index
inline Val val_at(const GrB_Matrix A, size_t p) { Val v{}; memcpy(v.data(), &A->hx[p * A->type->size], A->type->size); return v; }
inline std::pair<size_t, size_t> row_range(const GrB_Matrix A, uint64_t i) {
  const auto lo = std::lower_bound(A->hi.begin(), A->hi.end(), i), hi = std::upper_bound(lo, A->hi.end(), i);
  return {(size_t)(lo - A->hi.begin()), (size_t)(hi - A->hi.begin())};
}
// column j of op(A): a row of A is a contiguous run of its tuples, a column is picked out in one pass
inline Line line_of(GrB_Matrix A, bool transposed, uint64_t j) {
  mat_to_host(A); Line out;
  if (transposed) { const auto r = row_range(A, j); out.reserve(r.second - r.first); for (size_t p = r.first; p < r.second; p++) out.push_back({A->hj[p], val_at(A, p)}); }
  else for (size_t p = 0; p < A->hj.size(); p++) if (A->hj[p] == j) out.push_back({A->hi[p], val_at(A, p)});
  return out;
}
// row i (or column i) of C := `line` (values already in C's type)
inline void replace_line(GrB_Matrix C, bool is_row, uint64_t i, const Line& line) {
  const size_t ts = C->type->size;
  if (is_row) {
    const auto r = row_range(C, i);
    std::vector<GrB_Index> nj; std::vector<uint8_t> nx; nj.reserve(line.size()); nx.reserve(line.size() * ts);
    for (auto& e : line) { nj.push_back(e.first); nx.insert(nx.end(), e.second.data(), e.second.data() + ts); }
    C->hi.erase(C->hi.begin() + r.first, C->hi.begin() + r.second); C->hi.insert(C->hi.begin() + r.first, line.size(), i);
    C->hj.erase(C->hj.begin() + r.first, C->hj.begin() + r.second); C->hj.insert(C->hj.begin() + r.first, nj.begin(), nj.end());
    C->hx.erase(C->hx.begin() + r.first * ts, C->hx.begin() + r.second * ts); C->hx.insert(C->hx.begin() + r.first * ts, nx.begin(), nx.end());
  } else {
    const size_t n = C->hi.size();
    std::vector<GrB_Index> ni, nj; std::vector<uint8_t> nx; ni.reserve(n + line.size()); nj.reserve(n + line.size()); nx.reserve((n + line.size()) * ts);
    size_t q = 0;
    auto emit = [&](const std::pair<uint64_t, Val>& e) { ni.push_back(e.first); nj.push_back(i); nx.insert(nx.end(), e.second.data(), e.second.data() + ts); };
    for (size_t p = 0; p < n; p++) {
      while (q < line.size() && (line[q].first < C->hi[p] || (line[q].first == C->hi[p] && i < C->hj[p]))) emit(line[q++]);
      if (C->hj[p] == i) continue;                                      // the column's old entry
      ni.push_back(C->hi[p]); nj.push_back(C->hj[p]); nx.insert(nx.end(), &C->hx[p * ts], &C->hx[p * ts] + ts);
    }
    while (q < line.size()) emit(line[q++]);
    C->hi.swap(ni); C->hj.swap(nj); C->hx.swap(nx);
  }
  C->host_valid = true; mat_invalidate_device(C);
}
// the line C gets from `C(line) = accum(C(line), u)` over ALL positions, no mask: u's entries (cast), united with C's under accum
inline Line assigned_line(const Line& cur, int ccode, GrB_Vector u, GrB_BinaryOp accum) {
  if (accum) check_binop(accum, "accum");
  vec_to_host(u); const size_t us = u->type->size; const int ucode = u->type->code;
  Line out; out.reserve(cur.size() + u->hi.size());
  size_t a = 0, b = 0;
  auto uval = [&](size_t k) { Val v{}; memcpy(v.data(), &u->hx[k * us], us); return v; };
  while (a < cur.size() || b < u->hi.size()) {
    if (b >= u->hi.size() || (a < cur.size() && cur[a].first < u->hi[b])) { if (accum) out.push_back(cur[a]); a++; }          // C only: kept under accum, deleted without
    else if (a >= cur.size() || u->hi[b] < cur[a].first) { out.push_back({u->hi[b], cast(ccode, ucode, uval(b))}); b++; }
    else { out.push_back({u->hi[b], accum ? combine(accum, ccode, cur[a].second, ucode, uval(b)) : cast(ccode, ucode, uval(b))}); a++; b++; }
  }
  return out;
}

// ---- the words of a device route's plan string, and a list in HBM on its way to a host route ----
inline const char* kind_name(const ExIdx& x) { return x.kind == EX_ALL ? "all" : x.kind == EX_LIST ? (x.hbm ? "list@hbm" : "list") : "range"; }
// the plan's word for a list that was parsed in HBM (grb_index.hip); nothing for every other index argument, so that host-list calls keep their strings
inline std::string parse_name(const ExIdx& x) { return (x.hbm && x.n) ? std::string("k_index_parse<increasing=") + (x.increasing ? "1" : "0") + "> " : std::string(); }
// The host route of a call whose list lies in HBM: the list is copied down once, and the route's own parse reports what it always reports.
struct HostList {
  std::vector<GrB_Index> v;
  const GrB_Index* get(const IdxArg& a) {
    if (!a.in_hbm() || !a.I) return a.I;
    need_device(); v.resize(a.n ? a.n : 1);
    if (a.n) { GRB_HIP(hipMemcpyAsync(v.data(), a.I, a.n * 8, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream())); }
    return v.data();
  }
};

// the region update: positions of the index grid take A's entry (or lose theirs), combined with accum when given
inline void region_update(Map& C, int ccode, const Map& A, int acode, const std::vector<uint64_t>& ri, const std::vector<uint64_t>& ci, GrB_BinaryOp accum, const MaskView& mk, bool replace,
                   bool whole_mask /* GrB_assign: mask and replace span all of C */, bool row_scope, bool col_scope, uint64_t fixed) {
  if (accum) check_binop(accum, "accum");
  Map out;
  // new values over the region
  std::map<std::pair<uint64_t, uint64_t>, std::pair<bool, Val>> upd;               // position -> (has value, value in C's type)
  for (size_t a = 0; a < ri.size(); a++) for (size_t b = 0; b < ci.size(); b++) {
    const std::pair<uint64_t, uint64_t> p{ri[a], ci[b]};
    auto ia = A.find({a, b}); auto ic = C.find(p);
    if (accum) {
      if (ia != A.end() && ic != C.end()) upd[p] = {true, combine(accum, ccode, ic->second, acode, ia->second)};
      else if (ia != A.end()) upd[p] = {true, cast(ccode, acode, ia->second)};
      else if (ic != C.end()) upd[p] = {true, ic->second};
      else upd[p] = {false, Val{}};
    } else upd[p] = ia != A.end() ? std::make_pair(true, cast(ccode, acode, ia->second)) : std::make_pair(false, Val{});
  }
  auto in_scope = [&](const std::pair<uint64_t, uint64_t>& p) { return whole_mask || (row_scope && p.first == fixed) || (col_scope && p.second == fixed); };
  auto mkey = [&](const std::pair<uint64_t, uint64_t>& p) { return row_scope ? std::make_pair(p.second, (uint64_t)0) : (col_scope ? std::make_pair(p.first, (uint64_t)0) : p); };
  for (auto& kv : C) {
    const bool touched = upd.count(kv.first) != 0;
    const bool allowed = mk.allows(mkey(kv.first));
    if (touched && allowed) continue;                                    // replaced below
    if (!allowed && replace && in_scope(kv.first)) continue;             // deleted by replace
    out[kv.first] = kv.second;
  }
  for (auto& kv : upd) if (kv.second.first && mk.allows(mkey(kv.first))) out[kv.first] = kv.second.second;
  C.swap(out);
}
inline const char* accum_name(GrB_BinaryOp accum) { return accum ? accum->name : "none"; }
inline const DescView no_desc(nullptr);

}  // namespace hostmap
}  // namespace grb
