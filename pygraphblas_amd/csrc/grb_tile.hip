// grb_tile.hip — GxB_Matrix_concat and GxB_Matrix_split in HBM: a grid of CSR tiles into one CSR and back (behind grb_tile_ops.cpp; the integer geometry is
// grb_tile_geom.hpp).  Both are closed-form O(nvals) streams: a count, the library's scan, one pass that reads every entry once and writes it once.  No sort,
// no atomics, no LDS; the number of launches does not depend on the number of tiles, which the kernels reach through ONE descriptor table (TileDesc per tile,
// the two bounds arrays behind it).  All kernels: wave64, 256 threads, a capped grid with a loop past the cap, plain vector stores; values move as words of
// their size (1, 2, 4, 8 bytes), never by type.
//
// concat
//   k_concat_count   one thread per row r of C: its tile-row a by bisecting rowb, then the sum of the row's lengths in the n tiles of that tile-row.
//   (scan)           exclusive_scan_u32 over the counts IS C's row pointer.  nvals(C) is the sum of the tiles' counts, known on the host: no read-back.
//   k_concat_fill    ENTRY-PARALLEL over C's entries in chunks of TILE_CHUNK (R-MAT rows are skewed: never rows).  The workgroup brackets its chunk's rows
//                    (tuples_row_of / tuples_row_from, grb_tuples_geom.hpp); a lane owns TILE_EPL = 4 consecutive entries of C: it finds the first one's
//                    row by bisecting inside the bracket and its source by walking the row's tiles (tile_segment: the place inside the output row is
//                    recomputed from the tiles' row pointers, nothing is stored per (row, column block)), then steps through the source run; a new walk
//                    only where a tile's row ends.  The four columns (+ colb[b]) leave as ONE 16-byte store, the four values as one (4-byte words), two
//                    (8-byte) or a narrower one.  The chunk's tail that is not a whole group is stored entry by entry.
// split
//   k_split_count    one thread per row of A: the row is cut at the n - 1 inner block boundaries by bisecting its sorted columns; the n counts go to the flat
//                    count buffer, ordered tile by tile (tile_count_base).
//   (scan)           ONE exclusive scan S over the flat buffer holds every tile's row pointer and total.
//   k_split_totals   total of tile t = S[next base] - S[base]: m n words, read back in one copy to size the tiles' col / val arrays.
//   k_split_rowptr   one thread per flat position writes rowptr_t[lr] = S[pos] - S[base] through the table (a tile's last row writes the closing word too).
//   k_split_scatter  ENTRY-PARALLEL over A's entries in chunks, rows bracketed as above: an entry's block by bisecting colb with its column, its tile-row by
//                    bisecting rowb, its place inside the output row by an in-row bisect for the block's first entry (O(log len), independent of n).
//                    Reads of A are coalesced; the stores are contiguous runs per (row, block).
//   auxiliary HBM    concat: rows + 1 words.  split: 2 (n rows + 1) words (the counts and their scan: the size of the tiles' row pointers) + m n.
#include "grb_tile.hpp"
#include "grb_tuples_geom.hpp"
#include "grb_index.hpp"

namespace grb {
namespace {

static_assert(TILE_GRID_CAP == 4096, "the cap grid_1d gives the other O(nnz) kernels");

struct alignas(16) ColPack { uint32_t c[TILE_EPL]; };
template <int TS> struct alignas(TS * TILE_EPL > 16 ? 16 : TS * TILE_EPL) ValPack { typename WordOf<TS>::type v[TILE_EPL]; };

// ---- concat ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_concat_count(const TileDesc* __restrict__ table, const uint32_t* __restrict__ rowb, uint32_t m, uint32_t n, uint32_t nrows, uint32_t* __restrict__ counts) {
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= nrows; r += gridDim.x * 256ull) {
    uint32_t sum = 0;
    if (r < nrows) {
      const uint32_t a = tile_block_of<uint32_t>(rowb, m, (uint32_t)r), lr = (uint32_t)r - rowb[a];
      const TileDesc* d = table + (uint64_t)a * n;
      for (uint32_t b = 0; b < n; b++) { const uint32_t* rp = d[b].rowptr; sum += rp[lr + 1] - rp[lr]; }      // (the total is <= TILE_MAX_ENTRIES: no row's sum wraps)
    }
    counts[r] = sum;                                                     // (the word behind the last row is 0: the scan's last word is the total)
  }
}

// where entry q of C comes from: the tile's record, the position in its col / val arrays, and how many entries of that tile's row follow from there
struct ConcatPos { const TileDesc* d; uint32_t src, left; };
__device__ __forceinline__ ConcatPos concat_locate(uint32_t q, const uint32_t* __restrict__ crp, uint32_t rlo, uint32_t rhi, const TileDesc* __restrict__ table,
                                                   const uint32_t* __restrict__ rowb, uint32_t m, uint32_t n) {
  const uint32_t r = tuples_row_of(crp, rlo, rhi, q);
  const uint32_t a = tile_block_of<uint32_t>(rowb, m, r), lr = r - rowb[a];
  const TileDesc* d = table + (uint64_t)a * n;
  const TileSeg s = tile_segment(n, q - crp[r], [&](uint32_t b) { const uint32_t* rp = d[b].rowptr; return rp[lr + 1] - rp[lr]; });
  return ConcatPos{d + s.b, d[s.b].rowptr[lr] + s.at, s.left};
}

template <int TS>
__global__ __launch_bounds__(256) void k_concat_fill(const TileDesc* __restrict__ table, const uint32_t* __restrict__ rowb, uint32_t m, uint32_t n, const uint32_t* __restrict__ crp, uint32_t nrows,
                                                     uint64_t nnz, uint64_t nchunks, uint32_t* __restrict__ ocol, uint8_t* __restrict__ oval) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uint64_t base = tile_chunk_begin(c), end = tile_chunk_end(c, nnz);      // base < end <= nnz <= TILE_MAX_ENTRIES: entries are 32-bit words in crp
    const uint32_t rlo = tuples_row_of(crp, 0, nrows - 1, (uint32_t)base), rhi = tuples_row_from(crp, rlo, nrows - 1, (uint32_t)(end - 1));
    for (uint64_t q0 = base + (uint64_t)TILE_EPL * threadIdx.x; q0 < end; q0 += (uint64_t)TILE_EPL * TILE_THREADS) {      // q0 is a multiple of 4: ocol + q0 is 16-byte aligned
      const int cnt = end - q0 >= (uint64_t)TILE_EPL ? (int)TILE_EPL : (int)(end - q0);
      ConcatPos p = concat_locate((uint32_t)q0, crp, rlo, rhi, table, rowb, m, n);
      ColPack cp; ValPack<TS> vp;
#pragma unroll
      for (int j = 0; j < (int)TILE_EPL; j++) {
        if (j < cnt) {
          if (j && p.left == 0) p = concat_locate((uint32_t)(q0 + j), crp, rlo, rhi, table, rowb, m, n);      // the tile's row ended: the next tile of the row, or the next row
          cp.c[j] = p.d->col[p.src] + p.d->col0;                         // (< colb[b + 1] <= C.ncols)
          vp.v[j] = ((const W*)p.d->val)[p.src];
          p.src++; p.left--;
        } else { cp.c[j] = 0; vp.v[j] = 0; }
      }
      if (cnt == (int)TILE_EPL) {
        *reinterpret_cast<ColPack*>(ocol + q0) = cp;
        *reinterpret_cast<ValPack<TS>*>(oval + q0 * TS) = vp;
      } else {
        for (int j = 0; j < cnt; j++) { ocol[q0 + j] = cp.c[j]; ((W*)oval)[q0 + j] = vp.v[j]; }
      }
    }
  }
}

// ---- split ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_split_count(const uint32_t* __restrict__ arp, const uint32_t* __restrict__ acol, const uint32_t* __restrict__ rowb, const uint32_t* __restrict__ colb,
                                                     uint32_t m, uint32_t n, uint32_t nrows, uint32_t* __restrict__ counts) {
  for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= nrows; r += gridDim.x * 256ull) {
    if (r == nrows) { counts[(uint64_t)n * nrows] = 0; continue; }      // the scan's last word is the total
    const uint32_t a = tile_block_of<uint32_t>(rowb, m, (uint32_t)r), nr = rowb[a + 1] - rowb[a], lr = (uint32_t)r - rowb[a];
    uint32_t* out = counts + (uint64_t)n * rowb[a] + lr;               // + b nr: tile_count_base(rowb, n, a, b) + lr
    uint32_t lo = arp[r]; const uint32_t hi = arp[r + 1];
    for (uint32_t b = 0; b < n; b++) {
      const uint32_t cut = b + 1 < n ? tile_lower_bound(acol, lo, hi, colb[b + 1]) : hi;
      out[(uint64_t)b * nr] = cut - lo; lo = cut;
    }
  }
}

__global__ __launch_bounds__(256) void k_split_totals(const uint32_t* __restrict__ S, const uint32_t* __restrict__ rowb, uint32_t m, uint32_t n, uint32_t* __restrict__ totals) {
  const uint64_t ntiles = (uint64_t)m * n;
  for (uint64_t t = blockIdx.x * 256ull + threadIdx.x; t < ntiles; t += gridDim.x * 256ull) {
    const uint32_t a = (uint32_t)(t / n), b = (uint32_t)(t - (uint64_t)a * n);
    const uint64_t base = tile_count_base(rowb, n, a, b);
    totals[t] = S[base + (rowb[a + 1] - rowb[a])] - S[base];
  }
}

__global__ __launch_bounds__(256) void k_split_rowptr(const uint32_t* __restrict__ S, const TileDesc* __restrict__ table, const uint32_t* __restrict__ rowb, uint32_t m, uint32_t n, uint64_t npos) {
  for (uint64_t pos = blockIdx.x * 256ull + threadIdx.x; pos < npos; pos += gridDim.x * 256ull) {
    const uint32_t a = tile_count_row_of(rowb, m, n, pos), nr = rowb[a + 1] - rowb[a];
    const uint64_t within = pos - (uint64_t)n * rowb[a];
    const uint32_t b = (uint32_t)(within / nr), lr = (uint32_t)(within - (uint64_t)b * nr);
    const uint32_t s0 = S[pos - lr];
    uint32_t* rp = table[(uint64_t)a * n + b].rowptr;                    // nr + 1 words
    rp[lr] = S[pos] - s0;
    if (lr + 1 == nr) rp[nr] = S[pos + 1] - s0;                           // (pos + 1 <= npos: S has npos + 1 words)
  }
}

template <int TS>
__global__ __launch_bounds__(256) void k_split_scatter(const uint32_t* __restrict__ arp, uint32_t nrows, const uint32_t* __restrict__ acol, const uint8_t* __restrict__ aval, uint64_t nnz, uint64_t nchunks,
                                                       const TileDesc* __restrict__ table, const uint32_t* __restrict__ rowb, const uint32_t* __restrict__ colb, uint32_t m, uint32_t n) {
  typedef typename WordOf<TS>::type W;
  for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const uint64_t base = tile_chunk_begin(c), end = tile_chunk_end(c, nnz);
    const uint32_t rlo = tuples_row_of(arp, 0, nrows - 1, (uint32_t)base), rhi = tuples_row_from(arp, rlo, nrows - 1, (uint32_t)(end - 1));
    for (uint64_t e64 = base + threadIdx.x; e64 < end; e64 += TILE_THREADS) {
      const uint32_t e = (uint32_t)e64;
      const uint32_t r = tuples_row_of(arp, rlo, rhi, e), col = acol[e];
      const uint32_t b = tile_block_of<uint32_t>(colb, n, col), a = tile_block_of<uint32_t>(rowb, m, r);
      const TileDesc d = table[(uint64_t)a * n + b];
      const uint32_t first = tile_lower_bound(acol, arp[r], e, colb[b]);      // the block's first entry in the row (e itself when none lies before it)
      const uint32_t dst = d.rowptr[r - rowb[a]] + (e - first);               // (< the tile's total: the count pass cut the row at the same boundaries)
      d.col[dst] = col - colb[b];
      ((W*)d.val)[dst] = ((const W*)aval)[e];
    }
  }
}

// [TileDesc x m n][rowb][colb] in one buffer, one copy
struct TableImage {
  DevBuf dev; std::vector<uint8_t> host; size_t rowb_at = 0, colb_at = 0;
  TableImage(const TileGrid& g, size_t ndesc) {
    rowb_at = ndesc * sizeof(TileDesc); colb_at = rowb_at + ((size_t)g.m + 1) * 4;
    host.assign(colb_at + ((size_t)g.n + 1) * 4, 0);
    memcpy(host.data() + rowb_at, g.rowb.data(), ((size_t)g.m + 1) * 4); memcpy(host.data() + colb_at, g.colb.data(), ((size_t)g.n + 1) * 4);
  }
  TileDesc* desc() { return (TileDesc*)host.data(); }
  void upload() { dev.alloc(host.size()); GRB_HIP(hipMemcpyAsync(dev.p, host.data(), host.size(), hipMemcpyHostToDevice, stream())); }
  const TileDesc* table() const { return (const TileDesc*)dev.p; }
  const uint32_t* rowb() const { return (const uint32_t*)((const uint8_t*)dev.p + rowb_at); }
  const uint32_t* colb() const { return (const uint32_t*)((const uint8_t*)dev.p + colb_at); }
};

void check_grid(const TileGrid& g, const char* what) {
  if (!g.m || !g.n || g.rowb.size() != (size_t)g.m + 1 || g.colb.size() != (size_t)g.n + 1) fail(GrB_PANIC, std::string(what) + ": the tile grid is not well formed");
}

}  // namespace

void concat_csr(size_t ts, const TileGrid& g, const std::vector<TileSrc>& tiles, DevCSR& T) {
  check_value_size(ts, "concat"); check_grid(g, "concat");
  const uint64_t ntiles = (uint64_t)g.m * g.n, nrows = g.rowb[g.m], ncols = g.colb[g.n];
  if (tiles.size() != ntiles) fail(GrB_PANIC, "concat: the tile grid is not well formed");
  uint64_t nnz = 0;
  for (uint64_t t = 0; t < ntiles; t++) {                                  // (the entry point checked all of it: the kernels' bounds depend on it)
    const DevCSR& s = *tiles[t].csr; const uint32_t a = (uint32_t)(t / g.n), b = (uint32_t)(t % g.n);
    if (!s.valid || s.nrows != g.rowb[a + 1] - g.rowb[a] || s.ncols != g.colb[b + 1] - g.colb[b]) fail(GrB_PANIC, "concat: a tile does not conform to the grid");
    nnz += s.nnz;
  }
  if (nnz > TILE_MAX_ENTRIES) fail(GrB_PANIC, "concat: the result does not fit the 32-bit device layout");
  T.clear(); T.nrows = (uint32_t)nrows; T.ncols = (uint32_t)ncols; T.nnz = nnz;
  T.rowptr.alloc((nrows + 1) * 4); T.col.alloc(nnz * 4 + 16); T.val.alloc(nnz * ts + 16);
  if (!nnz) { GRB_HIP(hipMemsetAsync(T.rowptr.p, 0, (nrows + 1) * 4, stream())); GRB_HIP(hipStreamSynchronize(stream())); T.valid = true; return; }
  TableImage img(g, ntiles);
  uint64_t before = 0;
  for (uint64_t t = 0; t < ntiles; t++) {
    const DevCSR& s = *tiles[t].csr;
    img.desc()[t] = TileDesc{s.rowptr.as<uint32_t>(), s.col.as<uint32_t>(), (uint8_t*)tiles[t].val, g.rowb[t / g.n], g.colb[t % g.n], before};
    before += s.nnz;
  }
  img.upload();
  DevBuf counts((nrows + 1) * 4);
  hipLaunchKernelGGL(k_concat_count, dim3(grid_1d(nrows + 1)), dim3(256), 0, stream(), img.table(), img.rowb(), g.m, g.n, (uint32_t)nrows, counts.as<uint32_t>());
  GRB_HIP(hipGetLastError());
  exclusive_scan_u32(counts.as<uint32_t>(), T.rowptr.as<uint32_t>(), nrows + 1);
  const uint64_t nchunks = tile_chunks(nnz);
  dispatch_value_size(ts, [&]<int TS>() {
    hipLaunchKernelGGL((k_concat_fill<TS>), dim3(tile_grid(nchunks)), dim3(TILE_THREADS), 0, stream(), img.table(), img.rowb(), g.m, g.n, T.rowptr.as<uint32_t>(), (uint32_t)nrows, nnz, nchunks,
                       T.col.as<uint32_t>(), T.val.as<uint8_t>());
  });
  GRB_HIP(hipGetLastError());
  GRB_HIP(hipStreamSynchronize(stream()));                                 // the table's host image and the caller's cast copies of the tiles' values are released when it returns
  T.valid = true;
}

void split_csr(size_t ts, const TileGrid& g, const DevCSR& A, std::vector<DevCSR>& out) {
  check_value_size(ts, "split"); check_grid(g, "split");
  const uint64_t ntiles = (uint64_t)g.m * g.n, nrows = A.nrows, npos = (uint64_t)g.n * nrows;
  bool ok = A.valid && nrows && g.rowb[g.m] == A.nrows && g.colb[g.n] == A.ncols && A.nnz <= TILE_MAX_ENTRIES && npos <= TILE_MAX_ENTRIES;
  for (uint32_t a = 0; ok && a < g.m; a++) ok = g.rowb[a + 1] > g.rowb[a];
  for (uint32_t b = 0; ok && b < g.n; b++) ok = g.colb[b + 1] > g.colb[b];
  if (!ok) fail(GrB_PANIC, "split: the grid does not conform to the matrix or to the 32-bit device layout");      // (the entry point checked it: the kernels' bounds depend on it)
  TableImage img(g, ntiles);
  img.upload();                                                            // (the bounds now; the records once the totals have sized the outputs)
  DevBuf counts((npos + 1) * 4), S((npos + 1) * 4), totals(ntiles * 4);
  hipLaunchKernelGGL(k_split_count, dim3(grid_1d(nrows + 1)), dim3(256), 0, stream(), A.rowptr.as<uint32_t>(), A.col.as<uint32_t>(), img.rowb(), img.colb(), g.m, g.n, (uint32_t)nrows, counts.as<uint32_t>());
  GRB_HIP(hipGetLastError());
  exclusive_scan_u32(counts.as<uint32_t>(), S.as<uint32_t>(), npos + 1);
  hipLaunchKernelGGL(k_split_totals, dim3(grid_1d(ntiles)), dim3(256), 0, stream(), S.as<uint32_t>(), img.rowb(), g.m, g.n, totals.as<uint32_t>());
  GRB_HIP(hipGetLastError());
  std::vector<uint32_t> tot(ntiles);
  GRB_HIP(hipMemcpyAsync(tot.data(), totals.p, ntiles * 4, hipMemcpyDeviceToHost, stream())); GRB_HIP(hipStreamSynchronize(stream()));
  out.clear(); out.resize(ntiles);
  uint64_t before = 0;
  for (uint64_t t = 0; t < ntiles; t++) {
    const uint32_t a = (uint32_t)(t / g.n), b = (uint32_t)(t % g.n);
    DevCSR& o = out[t]; o.nrows = g.rowb[a + 1] - g.rowb[a]; o.ncols = g.colb[b + 1] - g.colb[b]; o.nnz = tot[t];
    o.rowptr.alloc(((size_t)o.nrows + 1) * 4); o.col.alloc((size_t)o.nnz * 4 + 8); o.val.alloc((size_t)o.nnz * ts + 8);
    img.desc()[t] = TileDesc{o.rowptr.as<uint32_t>(), o.col.as<uint32_t>(), o.val.as<uint8_t>(), g.rowb[a], g.colb[b], before};
    before += o.nnz;
  }
  if (before != A.nnz) fail(GrB_PANIC, "split: the tiles' counts do not add up to the matrix");
  GRB_HIP(hipMemcpyAsync(img.dev.p, img.host.data(), img.host.size(), hipMemcpyHostToDevice, stream()));      // the table, in one copy
  hipLaunchKernelGGL(k_split_rowptr, dim3(grid_1d(npos)), dim3(256), 0, stream(), S.as<uint32_t>(), img.table(), img.rowb(), g.m, g.n, npos);
  GRB_HIP(hipGetLastError());
  if (A.nnz) {
    const uint64_t nchunks = tile_chunks(A.nnz);
    dispatch_value_size(ts, [&]<int TS>() {
      hipLaunchKernelGGL((k_split_scatter<TS>), dim3(tile_grid(nchunks)), dim3(TILE_THREADS), 0, stream(), A.rowptr.as<uint32_t>(), (uint32_t)nrows, A.col.as<uint32_t>(), A.val.as<uint8_t>(), A.nnz, nchunks,
                         img.table(), img.rowb(), img.colb(), g.m, g.n);
    });
    GRB_HIP(hipGetLastError());
  }
  GRB_HIP(hipStreamSynchronize(stream()));                                 // the table's host image is released when it returns
  for (DevCSR& o : out) o.valid = true;
}

}  // namespace grb
