// grb_gemv_geom.hpp — the integer side of a FULL matrix times a vector (grb_gemv.hpp, the gemv_full route of GrB_mxv / GrB_vxm): the constants of the kernels'
// shape and the integer functions host code and the kernels share.  Plain integers only — no HIP types, no containers — so that a stand-alone program can check
// it under the sanitizers (tests/gemv_geometry_check.cpp).  Every function is constexpr: host code and the kernels call the same text.
//
// THE SHAPE (t(o) = (+)_l M(o, l) (x) u(l) for o < m, l < k; m the OUTER length, k the INNER one; A full and row-major, read where it lies)
//   layout N   M = A, m x k: an output's operands are one contiguous row.
//     k <= GEMV_N_GROUP_MAX   a group of G = gemv_group(k) lanes owns a row, lane g its product l = g; 64 / G rows a wave, GEMV_WAVES waves a workgroup.
//     longer                  the row is cut into gemv_n_chunks(k) chunks of GEMV_N_CHUNK products and a wave owns a (row, chunk) UNIT, unit = row * chunks + chunk.
//                             Inside a chunk the products are dealt out in PACKETS of V = min(GEMV_LOAD_BYTES / size, GEMV_MAX_PACK) consecutive l: lane g folds the packets g, g + 64, ...
//                             of its chunk left to right (one load of the whole packet where its address is aligned to the packet's size, V scalar loads of the same elements
//                             where not: the assignment, and so the order, never depends on the alignment), then the lanes are folded by a fixed butterfly.
//   layout T   M = A', A k x m: lanes own columns of A.  The rows are cut into gemv_t_chunks(k) chunks of gemv_t_chunk(k) rows (a function of k ALONE), a chunk
//              into GEMV_WAVES consecutive pieces, one per wave of the workgroup that owns the (slab, chunk) unit, unit = chunk * slabs + slab.  A slab is
//              64 * VT columns, lane g the VT consecutive ones from 64 VT slab + VT g; VT = V where V divides m (every row then starts aligned), else 1.
//   partials   a unit that is not its output's only chunk writes its partial and a "has a value" byte into slot gemv_slot(layout, o, chunk, m, chunks); k_gemv_fold
//              folds an output's slots in ascending chunk order, skipping those without a value.
// Not swept: none of the constants below (DESIGN.md "Full matrix times a vector").
#pragma once
#include <stdint.h>

namespace grb {

constexpr uint32_t GEMV_LOAD_BYTES = 16;         // bytes a lane loads at once: the widest global load (cdna guide: per-lane width bounds a stream); not swept
constexpr uint32_t GEMV_MAX_PACK = 4;             // values a packet holds at most: 16 bytes of FP32, 8 of INT16, 4 of INT8 — with 16 one-byte values a lane the run-time-operator kernels indexed their packets through scratch memory (80 and 144 bytes a lane); not swept
constexpr uint32_t GEMV_N_GROUP_MAX = 64;        // layout N: rows up to here share a wave (a lane per product); not swept
constexpr uint32_t GEMV_N_CHUNK = 8192;          // layout N: products per (row, chunk) unit — 32 KB of FP32, a multiple of 64 packets of every type; not swept
constexpr uint32_t GEMV_N_UNROLL = 4;            // layout N: packets of a lane whose loads are issued together; not swept
constexpr uint32_t GEMV_WAVES = 4;               // waves per workgroup, every kernel; not swept
constexpr uint32_t GEMV_GRID_CAP = 2048;         // workgroups: eight per compute unit, a loop past it (the siblings' value); not swept
constexpr uint32_t GEMV_T_CHUNK = 256;           // layout T: the fewest rows of a chunk (64 per wave); not swept
constexpr uint32_t GEMV_T_MAX_CHUNKS = 256;      // layout T: chunks per column at most — what one thread of k_gemv_fold reads serially; longer columns get longer chunks; not swept
constexpr uint32_t GEMV_T_UNROLL = 8;            // layout T: rows whose loads are issued together; not swept

static_assert(GEMV_N_CHUNK % (64 * GEMV_LOAD_BYTES) == 0, "a chunk is whole rounds of the wave's packets, whatever the value size");
static_assert(GEMV_T_CHUNK % GEMV_WAVES == 0 && (GEMV_T_CHUNK & (GEMV_T_CHUNK - 1)) == 0, "a chunk is one piece per wave; chunk lengths are powers of two");

constexpr uint64_t gemv_pow2ceil(uint64_t x) { uint64_t p = 1; while (p < x && p < (1ull << 63)) p <<= 1; return p; }
constexpr uint64_t gemv_ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }      // (no a + b: a may be near 2^64)

// values a lane loads at once
constexpr uint32_t gemv_vec(uint32_t size) { return GEMV_LOAD_BYTES / size < GEMV_MAX_PACK ? GEMV_LOAD_BYTES / size : GEMV_MAX_PACK; }

// ---- layout N ----
constexpr bool gemv_n_short(uint64_t k) { return k <= GEMV_N_GROUP_MAX; }
constexpr uint32_t gemv_group(uint64_t k) { return (uint32_t)gemv_pow2ceil(k < GEMV_N_GROUP_MAX ? (k ? k : 1) : GEMV_N_GROUP_MAX); }
constexpr uint32_t gemv_rows_per_wave(uint64_t k) { return 64 / gemv_group(k); }
constexpr uint32_t gemv_rows_per_workgroup(uint64_t k) { return GEMV_WAVES * gemv_rows_per_wave(k); }
constexpr uint64_t gemv_n_chunks(uint64_t k) { return k ? gemv_ceil_div(k, GEMV_N_CHUNK) : 1; }
constexpr uint64_t gemv_n_chunk_begin(uint64_t c) { return c * GEMV_N_CHUNK; }
constexpr uint64_t gemv_n_chunk_end(uint64_t k, uint64_t c) { return k - c * GEMV_N_CHUNK > GEMV_N_CHUNK ? (c + 1) * GEMV_N_CHUNK : k; }      // for c < gemv_n_chunks(k)

// ---- layout T ----
constexpr uint64_t gemv_t_chunk(uint64_t k) { const uint64_t r = gemv_pow2ceil(k) / GEMV_T_MAX_CHUNKS; return r > GEMV_T_CHUNK ? r : GEMV_T_CHUNK; }
constexpr uint64_t gemv_t_chunks(uint64_t k) { return k ? gemv_ceil_div(k, gemv_t_chunk(k)) : 1; }
constexpr uint64_t gemv_t_piece(uint64_t k) { return gemv_t_chunk(k) / GEMV_WAVES; }
// the rows [begin, end) of piece w < GEMV_WAVES of chunk c < gemv_t_chunks(k); empty (begin == end) past k
constexpr uint64_t gemv_t_piece_begin(uint64_t k, uint64_t c, uint32_t w) { const uint64_t b = c * gemv_t_chunk(k) + w * gemv_t_piece(k); return b < k ? b : k; }
constexpr uint64_t gemv_t_piece_end(uint64_t k, uint64_t c, uint32_t w) { const uint64_t b = gemv_t_piece_begin(k, c, w); return k - b > gemv_t_piece(k) ? b + gemv_t_piece(k) : k; }
constexpr uint32_t gemv_t_vt(uint64_t m, uint32_t size) { return m % gemv_vec(size) == 0 ? gemv_vec(size) : 1; }
constexpr uint64_t gemv_t_slab(uint64_t m, uint32_t size) { return 64ull * gemv_t_vt(m, size); }
constexpr uint64_t gemv_t_slabs(uint64_t m, uint32_t size) { return m ? gemv_ceil_div(m, gemv_t_slab(m, size)) : 1; }

// ---- both ----
enum { GEMV_N = 0, GEMV_T = 1 };
constexpr uint64_t gemv_chunks(int layout, uint64_t k) { return layout == GEMV_N ? (gemv_n_short(k) ? 1 : gemv_n_chunks(k)) : gemv_t_chunks(k); }
// the scratch slot of chunk c of output o: N keeps an output's slots together, T a chunk's (consecutive lanes, consecutive words); m * chunks slots in all
constexpr uint64_t gemv_slot(int layout, uint64_t o, uint64_t c, uint64_t m, uint64_t chunks) { return layout == GEMV_N ? o * chunks + c : c * m + o; }
// units of work a workgroup loop walks, saturating, and the grid for them (`per_wg` units a workgroup and round)
constexpr uint64_t gemv_mul_sat(uint64_t a, uint64_t b) { return a == 0 || b == 0 ? 0 : a > ~0ull / b ? ~0ull : a * b; }
constexpr uint32_t gemv_grid(uint64_t units, uint64_t per_wg) { const uint64_t g = gemv_ceil_div(units, per_wg); return g < 1 ? 1u : g > GEMV_GRID_CAP ? GEMV_GRID_CAP : (uint32_t)g; }

// The default rule, from the measurements (profiles/gemv_full_probe.jsonl, DESIGN.md "Full matrix times a vector"): against the SpMV kernels with a WARM plan the
// route won every measured point of layout N (not transposed: rows are the outputs) with an inner length of at least GEMV_DEFAULT_MIN_INNER and min_work entries,
// for FP32, FP64 and INT8; it lost points of layout N with shorter rows (2^20 x 16, 2^20 x 64, 2^16 x 256) and most points of layout T, which therefore stay with
// the SpMV kernels unless GRB_MI355X_GEMV=1.
constexpr uint64_t GEMV_DEFAULT_MIN_INNER = 1ull << 16;
constexpr uint64_t gemv_work(uint64_t rows, uint64_t cols) { return gemv_mul_sat(rows, cols); }
constexpr bool gemv_by_default(uint64_t rows, uint64_t cols, bool transposed, uint64_t min_work) {
  return !transposed && rows != 0 && cols >= GEMV_DEFAULT_MIN_INNER && gemv_work(rows, cols) >= min_work;
}

}  // namespace grb
