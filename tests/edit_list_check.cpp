// edit_list_check.cpp — the edit-list arithmetic of grb_edit_list.hpp against a brute-force replay of the queue on a std::map: a stand-alone host program
// (tests/test_edit_host.py builds it with the host compiler, once more with the address and undefined-behaviour sanitizers, and runs it).
// For random stored matrices and random queues (0, 1, 8, 9 and 5 000 records; repeats, set-after-delete, delete-after-set) it checks
//   * the normalised list: one record per touched coordinate, in (i, j) order, the one the replay applied last;
//   * the classes and the two prefix arrays: inserts / deletes counted by the replay before every edit;
//   * the destinations: every stored entry and every insert lands exactly where the replayed map has it, every slot of the result written once;
//   * the row pointer built from the prefix arrays; the queue's answer to a read (edit_lookup); the vector form of the normalisation;
//   * the host merge (edit_merge_host), matrix form and vector form, value widths 1 and 16: tuples and value bytes are the replay's — the queue sizes span
//     both sides of the in-place limit — and by hand: an empty stored list, edits before the first and after the last stored entry.
#include "grb_edit_list.hpp"
#include <array>
#include <map>
#include <random>
#include <stdio.h>
#include <stdlib.h>
#include <utility>

using namespace grb;

struct Rec { uint64_t i, j; bool del; uint8_t x[16]; };          // the shape of GrB_Matrix_opaque::Pending
struct VRec { uint64_t i; bool del; uint8_t x[16]; };            // ... and of GrB_Vector_opaque::Pending
typedef std::pair<uint64_t, uint64_t> Key;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (case %d)\n", __LINE__, #c, g_case); exit(1); } } while (0)
static int g_case = 0;

// ---- edit_merge_host against the replay: the matrix form (hj given) or the vector form (no hj: every key has column 0); returns the entries left ----
typedef std::array<uint8_t, 16> Bytes;
static Bytes stored_bytes(int v) { Bytes b; for (int t = 0; t < 16; t++) b[t] = (uint8_t)(v * 5 + t); return b; }
static uint64_t col_of(const Rec& r) { return r.j; }
static uint64_t col_of(const VRec&) { return 0; }
template <class R> static size_t check_merge(const std::map<Key, Bytes>& base, const std::vector<R>& q, bool matrix, size_t ts) {
  std::vector<uint64_t> hi, hj; std::vector<uint8_t> hx;
  for (auto& kv : base) { hi.push_back(kv.first.first); hj.push_back(kv.first.second); hx.insert(hx.end(), kv.second.begin(), kv.second.begin() + ts); }
  std::map<Key, Bytes> fin = base;
  for (const R& r : q) { const Key k(r.i, col_of(r)); if (r.del) fin.erase(k); else { Bytes b; memcpy(b.data(), r.x, 16); fin[k] = b; } }
  edit_merge_host(hi, matrix ? &hj : nullptr, hx, ts, q);
  CHECK(hi.size() == fin.size() && hx.size() == fin.size() * ts && (!matrix || hj.size() == fin.size()));
  size_t d = 0;
  for (auto& kv : fin) { CHECK(hi[d] == kv.first.first && (!matrix || hj[d] == kv.first.second) && memcmp(&hx[d * ts], kv.second.data(), ts) == 0); d++; }
  return fin.size();
}
static Rec rec(uint64_t i, uint64_t j, bool del, uint8_t x) { Rec r{}; r.i = i; r.j = j; r.del = del; for (int b = 0; b < 16; b++) r.x[b] = (uint8_t)(x + b); return r; }
static VRec vrec(uint64_t i, bool del, uint8_t x) { VRec r{}; r.i = i; r.del = del; for (int b = 0; b < 16; b++) r.x[b] = (uint8_t)(x + b); return r; }
static void merge_by_hand() {
  g_case++;
  const size_t widths[] = {1, 16}; const int repeats[] = {1, 5};      // each list once (in place) and five times over (beyond EDIT_IN_PLACE_MAX: rebuilt)
  for (size_t ts : widths) for (int reps : repeats) {
    // an empty stored list: set, then delete of the same coordinate, leaves nothing
    std::vector<Rec> q; std::vector<VRec> vq;
    for (int t = 0; t < reps; t++) { q.push_back(rec(3, 4, false, 9)); q.push_back(rec(3, 4, true, 0)); vq.push_back(vrec(3, false, 9)); vq.push_back(vrec(3, true, 0)); }
    CHECK((reps == 1) == (q.size() <= EDIT_IN_PLACE_MAX));
    CHECK(check_merge({}, q, true, ts) == 0 && check_merge({}, vq, false, ts) == 0);
    // ... and a set alone fills it
    CHECK(check_merge({}, std::vector<Rec>(1, rec(0, 0, false, 1)), true, ts) == 1 && check_merge({}, std::vector<VRec>(1, vrec(0, false, 1)), false, ts) == 1);
    // edits before the first and after the last stored entry: sets that land there, deletes of absent coordinates there
    const std::map<Key, Bytes> mb = {{Key(5, 5), stored_bytes(1)}, {Key(6, 1), stored_bytes(2)}}, vb = {{Key(5, 0), stored_bytes(1)}, {Key(6, 0), stored_bytes(2)}};
    q.clear(); vq.clear();
    for (int t = 0; t < reps; t++) {
      q.push_back(rec(9, 9, false, 10 + t)); q.push_back(rec(0, 0, false, 20 + t)); q.push_back(rec(0, 1, true, 0)); q.push_back(rec(5, 4, false, 30 + t));
      q.push_back(rec(6, 2, false, 40 + t)); q.push_back(rec(10, 0, true, 0));
      vq.push_back(vrec(9, false, 10 + t)); vq.push_back(vrec(0, false, 20 + t)); vq.push_back(vrec(2, true, 0)); vq.push_back(vrec(12, true, 0));
    }
    CHECK(check_merge(mb, q, true, ts) == 6 && check_merge(vb, vq, false, ts) == 4);
  }
}

static void one_case(std::mt19937_64& rng, uint32_t nrows, uint32_t ncols, size_t nstored, size_t nq) {
  g_case++;
  auto rnd = [&](uint64_t n) { return (uint64_t)(rng() % n); };
  std::map<Key, int> base;
  while (base.size() < nstored && base.size() < (size_t)nrows * ncols) base[Key(rnd(nrows), rnd(ncols))] = (int)rnd(100) + 1;
  std::vector<Key> keys; std::vector<int> vals; std::vector<uint32_t> rp(nrows + 1, 0);
  for (auto& kv : base) { keys.push_back(kv.first); vals.push_back(kv.second); rp[kv.first.first + 1]++; }
  for (uint32_t r = 0; r < nrows; r++) rp[r + 1] += rp[r];
  // the queue: half of the records aim at stored coordinates or at coordinates the queue already named
  std::vector<Rec> q;
  for (size_t t = 0; t < nq; t++) {
    Rec r{}; const uint64_t how = rnd(4);
    if (how == 0 && !keys.empty()) { const Key k = keys[rnd(keys.size())]; r.i = k.first; r.j = k.second; }
    else if (how == 1 && !q.empty()) { const Rec& o = q[rnd(q.size())]; r.i = o.i; r.j = o.j; }
    else { r.i = rnd(nrows); r.j = rnd(ncols); }
    r.del = rnd(3) == 0; r.x[0] = (uint8_t)(rnd(200) + 1);
    for (int b = 1; b < 16; b++) r.x[b] = (uint8_t)(r.x[0] * 3 + b);
    q.push_back(r);
  }
  // replay
  std::map<Key, int> fin = base; std::map<Key, const Rec*> last;
  for (const Rec& r : q) { if (r.del) fin.erase(Key(r.i, r.j)); else fin[Key(r.i, r.j)] = 1000 + r.x[0]; last[Key(r.i, r.j)] = &r; }
  // normalised list
  const std::vector<uint32_t> ord = edit_normalise_ij(q);
  CHECK(ord.size() == last.size());
  { size_t e = 0; for (auto& kv : last) { CHECK(&q[ord[e]] == kv.second); e++; } }
  const uint32_t k = (uint32_t)ord.size();
  // locate (what k_edit_locate does per edit) and classify
  std::vector<uint32_t> pos(k), ei(k); std::vector<uint8_t> cls(k);
  uint32_t nins = 0, ndel = 0;
  for (uint32_t e = 0; e < k; e++) {
    const Rec& r = q[ord[e]]; const Key key(r.i, r.j);
    const size_t p = std::lower_bound(keys.begin(), keys.end(), key) - keys.begin();
    const bool stored = p < keys.size() && keys[p] == key;
    CHECK(p >= rp[r.i] && p <= rp[r.i + 1]);
    pos[e] = (uint32_t)p; ei[e] = (uint32_t)r.i; cls[e] = edit_classify(stored, r.del);
    CHECK(cls[e] == (r.del ? (base.count(key) ? EDIT_DELETE : EDIT_NOTHING) : (base.count(key) ? EDIT_OVERWRITE : EDIT_INSERT)));
    nins += cls[e] == EDIT_INSERT; ndel += cls[e] == EDIT_DELETE;
  }
  std::vector<uint32_t> insb, delb; edit_prefixes(cls.data(), k, insb, delb);
  CHECK(insb.size() == k + 1 && delb.size() == k + 1 && insb[k] == nins && delb[k] == ndel);
  for (uint32_t e = 0; e < k; e++) {                       // counted by brute force
    uint32_t a = 0, b = 0; if (k <= 64) { for (uint32_t f = 0; f < e; f++) { a += cls[f] == EDIT_INSERT; b += cls[f] == EDIT_DELETE; } CHECK(insb[e] == a && delb[e] == b); }
    CHECK(insb[e + 1] - insb[e] == (cls[e] == EDIT_INSERT ? 1u : 0u) && delb[e + 1] - delb[e] == (cls[e] == EDIT_DELETE ? 1u : 0u));
  }
  CHECK(fin.size() == base.size() + nins - ndel);
  // destinations
  const size_t nout = fin.size();
  std::vector<Key> okey(nout); std::vector<int> oval(nout), writes(nout, 0);
  for (uint32_t p = 0; p < keys.size(); p++) {
    uint32_t d = 0; const bool stays = edit_dest(pos.data(), cls.data(), insb.data(), delb.data(), k, p, &d);
    CHECK(stays == (fin.count(keys[p]) != 0));
    if (stays) { CHECK(d < nout); okey[d] = keys[p]; oval[d] = vals[p]; writes[d]++; }
  }
  for (uint32_t e = 0; e < k; e++) if (cls[e] == EDIT_INSERT || cls[e] == EDIT_OVERWRITE) {      // after the stream pass, as k_edit_place
    const uint32_t d = edit_own_dest(pos.data(), insb.data(), delb.data(), e); const Rec& r = q[ord[e]];
    CHECK(d < nout);
    if (cls[e] == EDIT_INSERT) { okey[d] = Key(r.i, r.j); writes[d]++; } else CHECK(okey[d] == Key(r.i, r.j) && writes[d] == 1);
    oval[d] = 1000 + r.x[0];
  }
  { size_t d = 0; for (auto& kv : fin) { CHECK(writes[d] == 1 && okey[d] == kv.first && oval[d] == kv.second); d++; } }
  // row pointer: old + inserts - deletes among the edits of the rows before r
  std::vector<uint32_t> want(nrows + 1, 0);
  for (auto& kv : fin) want[kv.first.first + 1]++;
  for (uint32_t r = 0; r < nrows; r++) want[r + 1] += want[r];
  for (uint32_t r = 0; r <= nrows; r++) { const uint32_t m = (uint32_t)(std::lower_bound(ei.begin(), ei.end(), r) - ei.begin()); CHECK(rp[r] + insb[m] - delb[m] == want[r]); }
  // a read answered by the queue
  for (int t = 0; t < 50; t++) {
    const Key key = (t & 1) && !q.empty() ? Key(q[rnd(q.size())].i, q[rnd(q.size())].j) : Key(rnd(nrows), rnd(ncols));
    const Rec* r = edit_lookup(q, [&](const Rec& o) { return o.i == key.first && o.j == key.second; });
    CHECK(r == (last.count(key) ? last[key] : nullptr));
  }
  // the vector form: column 0 of the same queue
  std::vector<VRec> vq; std::map<uint64_t, const VRec*> vlast;
  for (const Rec& r : q) { VRec v{}; v.i = r.i; v.del = r.del; memcpy(v.x, r.x, 16); vq.push_back(v); }
  for (const VRec& v : vq) vlast[v.i] = &v;
  const std::vector<uint32_t> vord = edit_normalise_i(vq);
  CHECK(vord.size() == vlast.size());
  { size_t e = 0; for (auto& kv : vlast) { CHECK(&vq[vord[e]] == kv.second); e++; } }
  // the host merge of the same stored entries and the same queue: the matrix, and its first entry of every row as a vector
  std::map<Key, Bytes> mb, vb;
  for (auto& kv : base) { mb[kv.first] = stored_bytes(kv.second); vb.emplace(Key(kv.first.first, 0), stored_bytes(kv.second)); }
  const size_t widths[] = {1, 16};
  for (size_t ts : widths) { CHECK(check_merge(mb, q, true, ts) == fin.size()); check_merge(vb, vq, false, ts); }
}

int main() {
  merge_by_hand();
  std::mt19937_64 rng(12345);
  const size_t queues[] = {0, 1, 8, 9, 5000};
  for (size_t nq : queues)
    for (int rep = 0; rep < (nq == 5000 ? 6 : 60); rep++) {
      one_case(rng, 1, 1, rep & 1, nq);                                     // 1 x 1
      one_case(rng, 5, 5, 0, nq);                                           // inserts into nnz = 0
      one_case(rng, 7, 9, 20, nq);                                          // dense enough for every class
      one_case(rng, 300, 300, 2000, nq);
      one_case(rng, 3, 4000, 3000, nq);                                     // long rows
    }
  printf("edit list ok (%d cases)\n", g_case);
  return 0;
}
