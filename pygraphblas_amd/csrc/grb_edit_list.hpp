// grb_edit_list.hpp — the queue of element edits (setElement / removeElement) of a container that lives in HBM only, as plain arithmetic: no HIP in
// here, so the stand-alone check (tests/edit_list_check.cpp) compiles it with the host compiler.  grb_edit.hip applies the list on the device.
//
//   edit_normalise   the queue in program order -> the indices of the records that count, in (i, j) order: a stable sort by coordinate, the LAST record of a
//                    coordinate wins.
//   EditClass        what a normalised edit does to the stored matrix, decided on the device by bisecting its row (k_edit_locate): overwrite a stored entry,
//                    insert a new one, delete a stored one, or nothing (the delete of an absent entry).
//   edit_prefixes    insb[m] / delb[m] = the inserts / deletes among the first m normalised edits (m = 0 .. k).
//   edit_dest        where the stored entry at position p goes: p + inserts before its coordinate - deletes before it.  `pos[e]` is the position of the first
//                    stored entry whose coordinate is not below edit e's (non-decreasing in e), so "edits before the coordinate of p" is an upper bound of p
//                    in pos[], less the one edit that names p's own coordinate (the last with pos == p, an overwrite or a delete).
//   edit_lookup      the answer of the queue to a read of one coordinate: the last record that names it.
//   edit_merge_host  the same queue applied to a HOST mirror (tuples sorted by coordinate, values packed): the merge of mat_host_assemble / vec_host_assemble.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>

#if defined(__HIPCC__)
#define GRB_EDIT_HD __host__ __device__ inline
#else
#define GRB_EDIT_HD inline
#endif

namespace grb {

enum EditClass : uint8_t { EDIT_NOTHING = 0, EDIT_OVERWRITE = 1, EDIT_INSERT = 2, EDIT_DELETE = 3 };
GRB_EDIT_HD uint8_t edit_classify(bool stored, bool del) { return del ? (stored ? EDIT_DELETE : EDIT_NOTHING) : (stored ? EDIT_OVERWRITE : EDIT_INSERT); }

// P: a queue record (members i, del, x; j for a matrix); the result indexes `q`
template <class P, class Less, class Same>
inline std::vector<uint32_t> edit_normalise_by(const std::vector<P>& q, Less less, Same same) {
  std::vector<uint32_t> ord(q.size()), out;
  std::iota(ord.begin(), ord.end(), 0u);
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return less(q[a], q[b]); });
  out.reserve(ord.size());
  for (size_t k = 0; k < ord.size(); k++) if (k + 1 == ord.size() || !same(q[ord[k]], q[ord[k + 1]])) out.push_back(ord[k]);      // the last of a run of one coordinate
  return out;
}
template <class P> inline std::vector<uint32_t> edit_normalise_ij(const std::vector<P>& q) {
  return edit_normalise_by(q, [](const P& a, const P& b) { return a.i != b.i ? a.i < b.i : a.j < b.j; }, [](const P& a, const P& b) { return a.i == b.i && a.j == b.j; });
}
template <class P> inline std::vector<uint32_t> edit_normalise_i(const std::vector<P>& q) {
  return edit_normalise_by(q, [](const P& a, const P& b) { return a.i < b.i; }, [](const P& a, const P& b) { return a.i == b.i; });
}

inline void edit_prefixes(const uint8_t* cls, size_t k, std::vector<uint32_t>& insb, std::vector<uint32_t>& delb) {
  insb.assign(k + 1, 0); delb.assign(k + 1, 0);
  for (size_t e = 0; e < k; e++) { insb[e + 1] = insb[e] + (cls[e] == EDIT_INSERT ? 1u : 0u); delb[e + 1] = delb[e] + (cls[e] == EDIT_DELETE ? 1u : 0u); }
}

// edits e < k with pos[e] <= p
GRB_EDIT_HD uint32_t edit_upper_bound(const uint32_t* pos, uint32_t k, uint32_t p) {
  uint32_t lo = 0, hi = k;
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (pos[mid] <= p) lo = mid + 1; else hi = mid; }
  return lo;
}
// t = edit_upper_bound(pos, k, p).  False: the entry at p is deleted; else *dest is its new position.
GRB_EDIT_HD bool edit_dest_at(const uint32_t* pos, const uint8_t* cls, const uint32_t* insb, const uint32_t* delb, uint32_t t, uint32_t p, uint32_t* dest) {
  uint32_t m = t;
  if (t > 0 && pos[t - 1] == p && (cls[t - 1] == EDIT_OVERWRITE || cls[t - 1] == EDIT_DELETE)) { m = t - 1; if (cls[m] == EDIT_DELETE) return false; }
  *dest = p + insb[m] - delb[m];
  return true;
}
GRB_EDIT_HD bool edit_dest(const uint32_t* pos, const uint8_t* cls, const uint32_t* insb, const uint32_t* delb, uint32_t k, uint32_t p, uint32_t* dest) {
  return edit_dest_at(pos, cls, insb, delb, edit_upper_bound(pos, k, p), p, dest);
}
// where edit e itself writes (an insert or an overwrite)
GRB_EDIT_HD uint32_t edit_own_dest(const uint32_t* pos, const uint32_t* insb, const uint32_t* delb, uint32_t e) { return pos[e] + insb[e] - delb[e]; }

// the last record of the queue that names a coordinate, or nullptr
template <class P, class Same> inline const P* edit_lookup(const std::vector<P>& q, Same names) {
  for (size_t k = q.size(); k-- > 0;) if (names(q[k])) return &q[k];
  return nullptr;
}

// ---- the queue applied to a host mirror --------------------------------------------------------------------------------------------------------------
// Sorted tuples: `hi`, with `hj` for a matrix (nullptr: a vector, every column reads 0), values in `hx` at `ts` bytes each.
// the first position whose coordinate is not below (i, j) ...
inline size_t tuples_lower_bound(const std::vector<uint64_t>& hi, const std::vector<uint64_t>* hj, uint64_t i, uint64_t j) {
  size_t lo = 0, end = hi.size();
  while (lo < end) { const size_t m = lo + (end - lo) / 2; if (hi[m] < i || (hj && hi[m] == i && (*hj)[m] < j)) lo = m + 1; else end = m; }
  return lo;
}
// ... and whether position p holds exactly (i, j)
inline bool tuples_hold(const std::vector<uint64_t>& hi, const std::vector<uint64_t>* hj, size_t p, uint64_t i, uint64_t j) {
  return p < hi.size() && hi[p] == i && (!hj || (*hj)[p] == j);
}
constexpr size_t EDIT_IN_PLACE_MAX = 8;      // a queue this short edits the arrays where they are
// Applies the queue in program order: per coordinate the last record wins, a delete of an absent entry does nothing.  The queue itself is left as it was.
template <class P>
inline void edit_merge_host(std::vector<uint64_t>& hi, std::vector<uint64_t>* hj, std::vector<uint8_t>& hx, size_t ts, const std::vector<P>& q) {
  constexpr bool has_j = requires(const P& r) { r.j; };
  auto col = [](const P& r) -> uint64_t { if constexpr (has_j) return r.j; else return 0; };
  if (q.size() <= EDIT_IN_PLACE_MAX) {      // a few edits (`M[i, j] = x` then a read): one memmove each, instead of rebuilding the tuple arrays
    for (const P& e : q) {
      const size_t p = tuples_lower_bound(hi, hj, e.i, col(e)); const bool found = tuples_hold(hi, hj, p, e.i, col(e));
      if (e.del) { if (found) { hi.erase(hi.begin() + p); if (hj) hj->erase(hj->begin() + p); hx.erase(hx.begin() + p * ts, hx.begin() + (p + 1) * ts); } }
      else if (found) memcpy(&hx[p * ts], e.x, ts);
      else { hi.insert(hi.begin() + p, e.i); if (hj) hj->insert(hj->begin() + p, col(e)); hx.insert(hx.begin() + p * ts, e.x, e.x + ts); }
    }
    return;
  }
  std::vector<uint32_t> ord;
  if constexpr (has_j) ord = edit_normalise_ij(q); else ord = edit_normalise_i(q);
  const size_t nb = hi.size(); size_t b = 0;
  std::vector<uint64_t> ni, nj; std::vector<uint8_t> nx;
  ni.reserve(nb + ord.size()); if (hj) nj.reserve(nb + ord.size()); nx.reserve((nb + ord.size()) * ts);
  auto push_base = [&](size_t s) { ni.push_back(hi[s]); if (hj) nj.push_back((*hj)[s]); nx.insert(nx.end(), &hx[s * ts], &hx[s * ts] + ts); };
  for (const uint32_t o : ord) {
    const P& e = q[o];
    while (b < nb && (hi[b] < e.i || (hj && hi[b] == e.i && (*hj)[b] < col(e)))) push_base(b++);
    if (tuples_hold(hi, hj, b, e.i, col(e))) b++;      // replaced or deleted
    if (!e.del) { ni.push_back(e.i); if (hj) nj.push_back(col(e)); nx.insert(nx.end(), e.x, e.x + ts); }
  }
  while (b < nb) push_base(b++);
  hi.swap(ni); if (hj) hj->swap(nj); hx.swap(nx);
}

}  // namespace grb
