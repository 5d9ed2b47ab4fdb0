// grb_tile_ops.cpp — tile matrices: a grid of matrices into one, one matrix into a grid, both routes.
//
//   GxB_Matrix_concat, GxB_Matrix_split                         <- Matrix.concat / hstack / vstack, Matrix.split (SuiteSparse 5.1's entry points; the
//                                                                  reference package does not call them: the rules are in include/grb_mi355x.h)
//
// The host route works on the host mirrors (sorted tuples, grb_hostmap.hpp's casts): concat merges the tiles of a tile-row row by row, split hands every tuple
// to its tile — both linear in the entries, no map.  The kernels of the device route are in grb_tile.hip, the geometry and the argument verdicts in
// grb_tile_geom.hpp.  The argument and dimension checks come before the choice and are the same on both routes.
//
// Route (the rule and CONCAT_ / SPLIT_DEVICE_MIN_ENTRIES: grb_route.hpp): hook GRB_MI355X_TILE; legal when every container of the call has an HBM layout
// (mat_capable) and the result fits the 32-bit device layout (dimensions <= GRB_DIM_DEVICE_MAX, entries <= KRON_MAX_ENTRIES; split: n nrows(A) count words too);
// by size when a tile / A lives in HBM only, else on the entries of the host mirrors.  The results of the device route live in HBM only.
#include "grb_hostmap.hpp"
#include "grb_kron.hpp"
#include "grb_tile.hpp"
#include "grb_matops.hpp"

using namespace grb;
using namespace grb::hostmap;

namespace {

static_assert(TILE_DIM_MAX == GRB_DIM_DEVICE_MAX && TILE_MAX_ENTRIES == KRON_MAX_ENTRIES, "the geometry header repeats the bounds of the device layout");

constexpr uint64_t TILE_MAX_TILES = 1ull << 24;      // tiles of one call (either route): the grid is an array the caller filled

void check_grid_size(GrB_Index m, GrB_Index n, const char* what) {
  if (m > TILE_MAX_TILES || n > TILE_MAX_TILES || m * n > TILE_MAX_TILES) fail(GrB_INSUFFICIENT_SPACE, std::string(what) + ": more than 2^24 tiles");
}
int verdict_info(TileVerdict v) { return v == TILE_NULL ? GrB_NULL_POINTER : v == TILE_INVALID ? GrB_INVALID_VALUE : v == TILE_MISMATCH ? GrB_DIMENSION_MISMATCH : GrB_SUCCESS; }
bool narrow_grid(TileGrid& g, GrB_Index m, GrB_Index n, const std::vector<uint64_t>& rowb, const std::vector<uint64_t>& colb) {
  if (rowb[m] > GRB_DIM_DEVICE_MAX || colb[n] > GRB_DIM_DEVICE_MAX) return false;
  g.m = (uint32_t)m; g.n = (uint32_t)n; g.rowb.assign(rowb.begin(), rowb.end()); g.colb.assign(colb.begin(), colb.end());
  return true;
}

bool concat_on_device(GrB_Matrix C, const GrB_Matrix* Tiles, uint64_t ntiles) {
  bool capable = mat_capable(C);
  for (uint64_t t = 0; capable && t < ntiles; t++) capable = mat_capable(Tiles[t]);
  const RouteStep s = route_first(route_env("GRB_MI355X_TILE"), device_ok(), capable, false);
  if (s == ROUTE_HOST) return false;
  if (C->nrows > GRB_DIM_DEVICE_MAX || C->ncols > GRB_DIM_DEVICE_MAX) return false;
  uint64_t total = 0; bool in_hbm = false;
  for (uint64_t t = 0; t < ntiles; t++) { total += entries_of(Tiles[t]); in_hbm = in_hbm || hbm_only(Tiles[t]); if (total > KRON_MAX_ENTRIES) return false; }
  return s == ROUTE_DEVICE || route_by_size(in_hbm, true, total, CONCAT_DEVICE_MIN_ENTRIES);
}
bool split_on_device(GrB_Matrix A, GrB_Index n) {
  const RouteStep s = route_first(route_env("GRB_MI355X_TILE"), device_ok(), mat_capable(A), false);
  if (s == ROUTE_HOST) return false;
  if (A->nrows > GRB_DIM_DEVICE_MAX || A->ncols > GRB_DIM_DEVICE_MAX || n * A->nrows > KRON_MAX_ENTRIES) return false;      // (n <= 2^24, nrows < 2^32: no wrap)
  return s == ROUTE_DEVICE || route_by_host_count(A, SPLIT_DEVICE_MIN_ENTRIES);
}

void concat_device(GrB_Matrix C, const GrB_Matrix* Tiles, const TileGrid& g) {
  const uint64_t ntiles = (uint64_t)g.m * g.n; const int cc = C->type->code;
  std::vector<TileSrc> src(ntiles); std::vector<DevBuf> casts; casts.reserve(ntiles);
  std::map<GrB_Matrix, const void*> seen;                                // a tile object that stands at several grid positions is uploaded and cast once
  uint64_t ncast = 0;
  for (uint64_t t = 0; t < ntiles; t++) {
    GrB_Matrix T = Tiles[t];
    auto it = seen.find(T);
    if (it == seen.end()) {
      mat_to_device(T);
      casts.emplace_back();
      const void* v = cast_values(cc, T->type->code, T->csr.val.p, T->csr.nnz, casts.back());
      if (v != T->csr.val.p) ncast++;
      it = seen.emplace(T, v).first;
    }
    src[t] = TileSrc{&T->csr, it->second};
  }
  DevCSR out;
  concat_csr(C->type->size, g, src, out);
  g_last_plan = "concat<m=" + std::to_string(g.m) + ",n=" + std::to_string(g.n) + ",cast=" + std::to_string(ncast) + "> k_concat_count k_concat_fill ";
  matrix_write_back(C, out, cc, nullptr, no_desc, nullptr, false);      // C becomes exactly `out`: its entries, pending edits and everything derived from its old image are gone
}

// rows of one tile-row, merged: the tuples of each tile are sorted by (row, column) and the column origins grow with b
void concat_host(GrB_Matrix C, const GrB_Matrix* Tiles, GrB_Index m, GrB_Index n, const std::vector<uint64_t>& rowb, const std::vector<uint64_t>& colb) {
  const int cc = C->type->code; const size_t cs = C->type->size;
  for (uint64_t t = 0; t < m * n; t++) {
    mat_to_host(Tiles[t]);
    if (Tiles[t]->type->code != cc && (Tiles[t]->type->code >= T_FC32 || cc >= T_FC32)) fail(GrB_DOMAIN_MISMATCH, "concat: complex values are not typecast");
  }
  std::vector<GrB_Index> oi, oj; std::vector<uint8_t> ox;
  std::vector<size_t> cur(n);
  for (uint64_t a = 0; a < m; a++) {
    std::fill(cur.begin(), cur.end(), 0);
    for (;;) {
      uint64_t row = ~0ull;                                              // the next row any tile of the tile-row has entries in
      for (uint64_t b = 0; b < n; b++) { const GrB_Matrix T = Tiles[a * n + b]; if (cur[b] < T->hi.size() && T->hi[cur[b]] < row) row = T->hi[cur[b]]; }
      if (row == ~0ull) break;
      for (uint64_t b = 0; b < n; b++) {
        const GrB_Matrix T = Tiles[a * n + b]; const size_t ts = T->type->size; const int tc = T->type->code;
        size_t p = cur[b];
        for (; p < T->hi.size() && T->hi[p] == row; p++) {
          oi.push_back(rowb[a] + row); oj.push_back(colb[b] + T->hj[p]);
          const size_t at = ox.size(); ox.resize(at + cs);
          if (tc == cc) memcpy(&ox[at], &T->hx[p * ts], cs); else cast_scalar(cc, &ox[at], tc, &T->hx[p * ts]);
        }
        cur[b] = p;                                                      // (one cursor per POSITION: the same object may stand at several)
      }
    }
  }
  C->hi.swap(oi); C->hj.swap(oj); C->hx.swap(ox); C->pending.clear(); C->iso_full = false;
  C->host_valid = true; mat_invalidate_device(C);
}

struct NewTiles {                                                        // the handles of a split until it has succeeded
  std::vector<GrB_Matrix> h;
  ~NewTiles() { for (GrB_Matrix& x : h) GrB_Matrix_free(&x); }
  void make(GrB_Type type, GrB_Index m, GrB_Index n, const std::vector<uint64_t>& rowb, const std::vector<uint64_t>& colb) {
    h.assign(m * n, nullptr);
    for (uint64_t a = 0; a < m; a++) for (uint64_t b = 0; b < n; b++) {
      const GrB_Info info = GrB_Matrix_new(&h[a * n + b], type, rowb[a + 1] - rowb[a], colb[b + 1] - colb[b]);
      if (info) fail(info, "split: a tile could not be created");
    }
  }
};

void split_device(NewTiles& nt, GrB_Matrix A, const TileGrid& g) {
  mat_to_device(A);
  std::vector<DevCSR> out;
  split_csr(A->type->size, g, A->csr, out);
  for (size_t t = 0; t < out.size(); t++) { GrB_Matrix T = nt.h[t]; T->csr = std::move(out[t]); T->csr.valid = true; T->dev_valid = true; T->host_valid = false; }
  g_last_plan = "split<m=" + std::to_string(g.m) + ",n=" + std::to_string(g.n) + "> k_split_count k_split_totals k_split_rowptr k_split_scatter ";
}
void split_host(NewTiles& nt, GrB_Matrix A, GrB_Index m, GrB_Index n, const std::vector<uint64_t>& rowb, const std::vector<uint64_t>& colb) {
  mat_to_host(A); const size_t ts = A->type->size;
  uint64_t a = 0;
  for (size_t p = 0; p < A->hi.size(); p++) {                            // sorted by (row, column): every tile receives its tuples in order
    const uint64_t i = A->hi[p], j = A->hj[p];
    while (i >= rowb[a + 1]) a++;
    const uint64_t b = tile_block_of<uint64_t>(colb.data(), (uint32_t)n, j);
    GrB_Matrix T = nt.h[a * n + b];
    T->hi.push_back(i - rowb[a]); T->hj.push_back(j - colb[b]); T->hx.insert(T->hx.end(), &A->hx[p * ts], &A->hx[p * ts] + ts);
  }
}

}  // namespace

extern "C" {

GrB_Info GrBX_tile_thresholds(uint64_t* concat_min_entries, uint64_t* split_min_entries) {
  if (!concat_min_entries || !split_min_entries) return GrB_NULL_POINTER;
  *concat_min_entries = CONCAT_DEVICE_MIN_ENTRIES; *split_min_entries = SPLIT_DEVICE_MIN_ENTRIES; return GrB_SUCCESS;
}
GrB_Info GrBX_tile_geometry(uint64_t* out) {
  if (!out) return GrB_NULL_POINTER;
  out[0] = TILE_CHUNK; out[1] = TILE_GRID_CAP; out[2] = TILE_EPL; return GrB_SUCCESS;
}

// (the descriptor has no field either operation reads: it is ignored on both routes)
GrB_Info GxB_Matrix_concat(GrB_Matrix C, const GrB_Matrix* Tiles, const GrB_Index m, const GrB_Index n, const GrB_Descriptor desc) {
  (void)desc; if (!C || !Tiles) return GrB_NULL_POINTER; if (!check_obj(C)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(C, [&] {
    if (m == 0 || n == 0) fail(GrB_INVALID_VALUE, "concat: the grid has no tiles");
    check_grid_size(m, n, "concat");
    const uint64_t ntiles = m * n;
    for (uint64_t t = 0; t < ntiles; t++) if (!Tiles[t]) fail(GrB_NULL_POINTER, "concat: a tile is NULL");
    for (uint64_t t = 0; t < ntiles; t++) { check_m(Tiles[t], "concat"); if (Tiles[t] == C) fail(GrB_INVALID_VALUE, "concat: the output is one of the tiles"); }
    std::vector<uint64_t> sr(ntiles), sc(ntiles), rowb(m + 1), colb(n + 1);
    for (uint64_t t = 0; t < ntiles; t++) { sr[t] = Tiles[t]->nrows; sc[t] = Tiles[t]->ncols; }
    const TileVerdict v = tile_check_concat(m, n, sr.data(), sc.data(), C->nrows, C->ncols, rowb.data(), colb.data());
    if (v != TILE_OK) fail(verdict_info(v), "concat: the tiles' dimensions do not conform to each other or to C");
    g_last_plan.clear();
    TileGrid g;
    if (concat_on_device(C, Tiles, ntiles) && narrow_grid(g, m, n, rowb, colb)) { concat_device(C, Tiles, g); return; }
    concat_host(C, Tiles, m, n, rowb, colb);
  });
}

GrB_Info GxB_Matrix_split(GrB_Matrix* Tiles, const GrB_Index m, const GrB_Index n, const GrB_Index* Tile_nrows, const GrB_Index* Tile_ncols, const GrB_Matrix A, const GrB_Descriptor desc) {
  (void)desc; if (!Tiles || !Tile_nrows || !Tile_ncols || !A) return GrB_NULL_POINTER; if (!check_obj(A)) return GrB_UNINITIALIZED_OBJECT;
  return guarded(A, [&] {
    if (m == 0 || n == 0) fail(GrB_INVALID_VALUE, "split: the grid has no tiles");
    check_grid_size(m, n, "split");
    std::vector<uint64_t> rowb(m + 1), colb(n + 1);
    const TileVerdict v = tile_check_split(m, n, Tile_nrows, Tile_ncols, A->nrows, A->ncols, rowb.data(), colb.data());
    if (v == TILE_INVALID) fail(GrB_INVALID_VALUE, "split: a tile size of 0 is refused");      // (GrB_Matrix_new's code for a dimension it refuses)
    if (v != TILE_OK) fail(verdict_info(v), "split: the tile sizes do not add up to A's dimensions");
    g_last_plan.clear();
    NewTiles nt; nt.make(A->type, m, n, rowb, colb);
    TileGrid g;
    if (split_on_device(A, n) && narrow_grid(g, m, n, rowb, colb)) split_device(nt, A, g);
    else split_host(nt, A, m, n, rowb, colb);
    for (uint64_t t = 0; t < m * n; t++) Tiles[t] = nt.h[t];             // only now: a failed split leaves Tiles[] as it was and no handle allocated
    nt.h.clear();
  });
}

}  // extern "C"
