// edit_list_check.cpp — the edit-list arithmetic of grb_edit_list.hpp against a brute-force replay of the queue on a std::map: a stand-alone host program
// (tests/test_edit_host.py builds it with the host compiler, once more with the address and undefined-behaviour sanitizers, and runs it).
// For random stored matrices and random queues (0, 1, 8, 9 and 5 000 records; repeats, set-after-delete, delete-after-set) it checks
//   * the normalised list: one record per touched coordinate, in (i, j) order, the one the replay applied last;
//   * the classes and the two prefix arrays: inserts / deletes counted by the replay before every edit;
//   * the destinations: every stored entry and every insert lands exactly where the replayed map has it, every slot of the result written once;
//   * the row pointer built from the prefix arrays; the queue's answer to a read (edit_lookup); the vector form of the normalisation.
#include "grb_edit_list.hpp"
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
  for (const Rec& r : q) { VRec v{}; v.i = r.i; v.del = r.del; v.x[0] = r.x[0]; vq.push_back(v); }
  for (const VRec& v : vq) vlast[v.i] = &v;
  const std::vector<uint32_t> vord = edit_normalise_i(vq);
  CHECK(vord.size() == vlast.size());
  { size_t e = 0; for (auto& kv : vlast) { CHECK(&vq[vord[e]] == kv.second); e++; } }
}

int main() {
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
