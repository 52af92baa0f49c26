// Time-localised matching: the score matrices of many (query, song) pairs and their local alignment (include/nsid.h nsid_pair_sim /
// nsid_local_align).
//
// The reference stops at "which song" (eval.py:250-258 keeps the reconstructed index "for calculating histogram-based matching score" in
// "future implementations"; sample100-ext annotates where every occurrence lies in both tracks). This file answers where.
//
// pair_sim: one wave per 32x32 tile of one pair's S = q x^T; the tiles of all pairs come from a host-built table (largest pairs first).
// The dot is the chain of csrc/search.hip: one k-ordered fp32 fmaf chain on v_mfma_f32_32x32x2_f32, the same for every (i, j) whichever
// tile, lane or pair holds it (up to d = 256 the pairing of l2_topk_split_kernel, above it the pairing of l2_topk_wide_kernel).
// pair_sim_norm is the same tile with another store epilogue: the cell normalised by the cohort statistics of its two rows
// (csrc/cohort.hip computes them); the walks below do not know which of the two wrote their S.
//
// The walk (al_walk): one workgroup per pair walks the rows of S_p; threads own columns. The rule (stated in include/nsid.h) needs rows
// i - 1 and i - 2 only, so all columns of a row are independent: three rotating rows of (H, origin) cells in LDS, 8 bytes a cell, one
// barrier per row (it orders LDS only), S read eight rows at a time with all loads in flight together. A row's result (its best cell
// that itself passes the threshold) is reduced per wave (DPP), left in LDS, combined during the next row and handed to the caller's
// sink. No atomics; a pair's result depends on nothing but the pair. The rule is written once, there; a pass of the walk covers the
// rows of a strip over a range of columns, and three kernels call it:
//
// local_align: one pass over the whole matrix from zeros; the sink stores (H, j, packed origin) per row. After the walk the same
// workgroup reads the row results back and forms the occurrences with the quadratic compares of csrc/vote.hip.
//
// local_align_strip / align_occurrences: one pass from two carried rows to two carried rows, so that a recording of any length goes
// through in strips; the sink stores (H, j, i0, j0) with i0 a global row. The occurrences of a run of rows of any length come from
// its row results (include/nsid.h, below nsid_local_align).
//
// local_align_panels / align_occurrences_span: for songs of up to 16384 rows, the strip in one pass per panel of at most 4096 columns
// with two carried columns (the halo) between panels, so the LDS rows keep their width; the sink keeps a row's best over the panels
// in LDS and stores the row's halo. The occurrence kernel takes the width of a group's window per run (include/nsid.h, below
// nsid_align_occurrences).
//
// align_paths: the path of an occurrence (which song row each query row was aligned to), which the walk drops: the rule on the
// occurrence's own box with every cell's step kept, 2 bits a cell in a byte workspace, then the steps followed back from the box's
// last cell. That is cell for cell the path of the whole matrix (include/nsid.h, nsid_align_paths; the proof is in DESIGN.md,
// "Alignment paths"). Its row is written beside al_walk, not through it: the three kernels above are measured and stay as they are.
//
// The helpers beside the walk are what the strip and the panels share: the rows of a pair without cells (al_no_cells), the fill of
// the three LDS rows (al_fill), the carry out (al_carry_out) and open_h (al_open_h). On the host one macro picks 256 or 1024 threads
// for all three entries (AL_LAUNCH), and one function checks the arguments the strip and the panels share (align_strip_args).
#include "nsid_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int AL_MAX_ROWS = NSID_ALIGN_MAX_ROWS;
constexpr int AL_MAX_COLS = NSID_ALIGN_MAX_COLS;
constexpr int AL_MAX_TOP = NSID_ALIGN_MAX_TOP;
constexpr int AL_CPT = 4;             // columns (and, after the walk, rows) per thread at the most
constexpr int AL_RB = 8;              // rows of S a thread loads at a time during the walk
constexpr int AL_CHUNK = 8;           // LDS entries per step of the compare loops
static_assert(AL_MAX_ROWS <= (1 << 15) && AL_MAX_COLS <= (1 << 16), "row_org packs (i0, j0) into 16 bits each of an int32 >= 0");
static_assert(AL_MAX_ROWS <= 1024 * AL_CPT && AL_MAX_COLS <= 1024 * AL_CPT, "1024 threads own at most AL_CPT columns / rows each");

// ---- pair_sim -------------------------------------------------------------------------------------------------------------------
// Lane (r, h) = (lane & 31, lane >> 5) holds query row i0 + r as the A operand and song row j0 + r as the B operand; accumulator
// register g is query row i0 + (g & 3) + 8 (g >> 2) + 4 h against song row j0 + r. WIDE = false: MFMA step (b, e) pairs k = 8 b + e
// (h = 0) with k = 8 b + 4 + e (h = 1), 16 contiguous bytes per lane and block. WIDE = true: step t pairs k = 2 t with k = 2 t + 1.
// Rows past a pair's end are read from its last row and never stored.
template <bool WIDE>
__global__ __launch_bounds__(64) void pair_sim_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ x, int ldx,
                                                      long nx, int d, const int* __restrict__ q_start, const int* __restrict__ q_len,
                                                      const int64_t* __restrict__ x_start, const int* __restrict__ x_len,
                                                      const int64_t* __restrict__ s_off, const int* __restrict__ s_ld, int npairs,
                                                      const int* __restrict__ tiles, float* __restrict__ S, int64_t s_len) {
  const int lane = lane_id(), r = lane & 31, h = lane >> 5;
  const int* t = tiles + 3 * (size_t)blockIdx.x;
  const int p = t[0], i0 = t[1], j0 = t[2];
  if (p < 0 || p >= npairs) return;
  const int Lq = q_len[p], Lr = x_len[p];
  const long qs = q_start[p], xs = x_start[p], so = s_off[p], ld = s_ld[p];
  // the caller checks the table; this only keeps a bad entry in bounds (uniform)
  if (i0 < 0 || j0 < 0 || i0 >= Lq || j0 >= Lr || qs < 0 || xs < 0 || qs + Lq > nq || xs + Lr > nx || ld < Lr || so < 0 ||
      so + (long)(Lq - 1) * ld + Lr > s_len)
    return;
  const float* qp = q + (size_t)(qs + min(i0 + r, Lq - 1)) * ldq;
  const float* xp = x + (size_t)(xs + min(j0 + r, Lr - 1)) * ldx;
  f32x16 acc = {};
  const int nb = d / 8;
  if (!WIDE) {
    qp += 4 * h;
    xp += 4 * h;
    for (int b = 0; b < nb; b += 2) {                 // d % 16 == 0: two blocks' loads in flight per step
      const f32x4 a0 = ld4(qp + 8 * b), c0 = ld4(xp + 8 * b), a1 = ld4(qp + 8 * b + 8), c1 = ld4(xp + 8 * b + 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], c0[e], acc, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], c1[e], acc, 0, 0, 0);
    }
  } else {
    for (int b = 0; b < nb; ++b) {
      const f32x4 a0 = ld4(qp + 8 * b), a1 = ld4(qp + 8 * b + 4), c0 = ld4(xp + 8 * b), c1 = ld4(xp + 8 * b + 4);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a0[1] : a0[0], h ? c0[1] : c0[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a0[3] : a0[2], h ? c0[3] : c0[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a1[1] : a1[0], h ? c1[1] : c1[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a1[3] : a1[2], h ? c1[3] : c1[2], acc, 0, 0, 0);
    }
  }
  const int col = j0 + r;
  float* sp = S + so + col;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = i0 + (g & 3) + 8 * (g >> 2) + 4 * h;
    if (row < Lq && col < Lr) sp[(size_t)row * ld] = acc[g];
  }
}

// ---- pair_sim_norm (nsid_pair_sim_norm): pair_sim_kernel with the cohort-normalised cell in its store epilogue, the statistics
// indexed by the absolute rows of q and x. pair_sim_kernel is measured and stays as it is, instruction for instruction; the tile is
// restated here in the same words, as align_paths restates the walk's cell.

// the normalised cell of include/nsid.h ("cohort score normalisation"): five fp32 operations, each rounded once, none contracted
__device__ __forceinline__ float sim_norm_cell(float s, float mq, float rq, float mx, float rx) {
#pragma clang fp contract(off)
  const float zq = (s - mq) * rq;
  const float zx = (s - mx) * rx;
  const float sum = zq + zx;
  return 0.5f * sum;
}

template <bool WIDE>
__global__ __launch_bounds__(64) void pair_sim_norm_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ x,
                                                           int ldx, long nx, int d, const int* __restrict__ q_start,
                                                           const int* __restrict__ q_len, const int64_t* __restrict__ x_start,
                                                           const int* __restrict__ x_len, const int64_t* __restrict__ s_off,
                                                           const int* __restrict__ s_ld, int npairs, const int* __restrict__ tiles,
                                                           float* __restrict__ S, int64_t s_len, const float* __restrict__ q_mu,
                                                           const float* __restrict__ q_rs, const float* __restrict__ x_mu,
                                                           const float* __restrict__ x_rs) {
  const int lane = lane_id(), r = lane & 31, h = lane >> 5;
  const int* t = tiles + 3 * (size_t)blockIdx.x;
  const int p = t[0], i0 = t[1], j0 = t[2];
  if (p < 0 || p >= npairs) return;
  const int Lq = q_len[p], Lr = x_len[p];
  const long qs = q_start[p], xs = x_start[p], so = s_off[p], ld = s_ld[p];
  // the caller checks the table; this only keeps a bad entry in bounds (uniform)
  if (i0 < 0 || j0 < 0 || i0 >= Lq || j0 >= Lr || qs < 0 || xs < 0 || qs + Lq > nq || xs + Lr > nx || ld < Lr || so < 0 ||
      so + (long)(Lq - 1) * ld + Lr > s_len)
    return;
  const float* qp = q + (size_t)(qs + min(i0 + r, Lq - 1)) * ldq;
  const float* xp = x + (size_t)(xs + min(j0 + r, Lr - 1)) * ldx;
  f32x16 acc = {};
  const int nb = d / 8;
  if (!WIDE) {
    qp += 4 * h;
    xp += 4 * h;
    for (int b = 0; b < nb; b += 2) {                 // d % 16 == 0: two blocks' loads in flight per step
      const f32x4 a0 = ld4(qp + 8 * b), c0 = ld4(xp + 8 * b), a1 = ld4(qp + 8 * b + 8), c1 = ld4(xp + 8 * b + 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], c0[e], acc, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], c1[e], acc, 0, 0, 0);
    }
  } else {
    for (int b = 0; b < nb; ++b) {
      const f32x4 a0 = ld4(qp + 8 * b), a1 = ld4(qp + 8 * b + 4), c0 = ld4(xp + 8 * b), c1 = ld4(xp + 8 * b + 4);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a0[1] : a0[0], h ? c0[1] : c0[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a0[3] : a0[2], h ? c0[3] : c0[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a1[1] : a1[0], h ? c1[1] : c1[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a1[3] : a1[2], h ? c1[3] : c1[2], acc, 0, 0, 0);
    }
  }
  const int col = j0 + r;
  float* sp = S + so + col;
  if (col >= Lr) return;                       // after the last MFMA: a lane without a column stores nothing
  const float mx = x_mu[xs + col], rx = x_rs[xs + col];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = i0 + (g & 3) + 8 * (g >> 2) + 4 * h;
    if (row < Lq) sp[(size_t)row * ld] = sim_norm_cell(acc[g], q_mu[qs + row], q_rs[qs + row], mx, rx);
  }
}

// ---- local alignment: a row's key, the empty result ----------------------------------------------------------------------------------
// a row's best cell as one key: H's bits (H > 0, so they order as the floats do) above the complement of j (ties: the smaller j wins a max);
// 0 = the row has no cell that passes the threshold
__device__ __forceinline__ unsigned long long al_key(float h, int j) {
  return ((unsigned long long)__builtin_bit_cast(unsigned, h) << 32) | (0xffffffffu - (unsigned)j);
}

// 64-lane max of the keys with DPP only, the steps of nsid_common.h's wave_sum (0 is the identity of the max, as of the sum there): no
// LDS permutes on the row's critical path. Every lane receives the result.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long al_key_dpp_max(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROW_MASK, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xF, true);
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o > v ? o : v;
}
__device__ __forceinline__ unsigned long long al_wave_key_max(unsigned long long v) {
  v = al_key_dpp_max<0xB1, 0xF>(v);
  v = al_key_dpp_max<0x4E, 0xF>(v);
  v = al_key_dpp_max<0x141, 0xF>(v);
  v = al_key_dpp_max<0x140, 0xF>(v);
  v = al_key_dpp_max<0x142, 0xA>(v);
  v = al_key_dpp_max<0x143, 0xC>(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ void al_empty(int p, int top, int n, int tid, int* __restrict__ occ, float* __restrict__ occ_score,
                                         int* __restrict__ n_occ) {
  if (tid < top) {
    int* o = occ + ((size_t)p * top + tid) * 4;
    o[0] = o[1] = o[2] = o[3] = -1;
    occ_score[(size_t)p * top + tid] = 0.f;
  }
  if (tid == 0) n_occ[p] = n;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------
// A cell keeps its origin as (i0 mod 2^15) << 16 | j0 (sign bit clear, -1 = none), i0 a GLOBAL query row: every step of a path advances
// j by at least 1 and i by at most 2, so i - i0 <= 2 (Lr - 1) < 2^15 and i0 = i - ((i - m) mod 2^15).
constexpr int AL_I0_MOD = 1 << 15;
constexpr int AL_SPAN = 2 * (AL_MAX_COLS - 1);    // i - i0 of a cell at the most, songs of up to AL_MAX_COLS rows
constexpr int AL_MAX_SONG_ROWS = NSID_ALIGN_MAX_SONG_ROWS;
static_assert(AL_SPAN < AL_I0_MOD && AL_MAX_COLS <= (1 << 16), "a cell's origin row is recovered from its low 15 bits");
static_assert(AL_MAX_SONG_ROWS <= (1 << 16), "a cell's origin column keeps its 16 bits");
static_assert(2 * (AL_MAX_SONG_ROWS - 1) < AL_I0_MOD, "a cell's origin row is recovered from its low 15 bits: i - i0 <= 2 (Lr - 1)");
// local_align_kernel's rows are global rows 0 .. AL_MAX_ROWS - 1 < 2^15 (the first static_assert of this file), so there the packing
// is (i0 << 16) | j0 itself: row_org's documented packing, bit for bit.
static_assert(3 * (AL_MAX_COLS + 2) * 8 + AL_MAX_ROWS * 12 + 4096 <= NSID_LDS_MAX, "three rows of cells and the strip's row results in LDS");

__device__ __forceinline__ int al_pack_org(int i0, int j0) { return (i0 < 0 || j0 < 0) ? -1 : (((i0 & (AL_I0_MOD - 1)) << 16) | j0); }
// the origin row of a cell of global row i (org >= 0)
__device__ __forceinline__ int al_org_row(int i, int org) { return i - ((i - (org >> 16)) & (AL_I0_MOD - 1)); }

// A pair's cells in memory, (H, i0, j0) each: the two carried rows (the carry) or the two columns between panels (the halo).
struct AlCells {
  float* h;                    // the pair's first cell
  int* i0;
  int* j0;
  __device__ __forceinline__ AlCells(float* h_, int* i0_, int* j0_, int64_t off) : h(h_ + off), i0(i0_ + off), j0(j0_ + off) {}
  __device__ __forceinline__ AlCells() : h(nullptr), i0(nullptr), j0(nullptr) {}
  __device__ __forceinline__ int2 load(int64_t a) const { return int2{__builtin_bit_cast(int, h[a]), al_pack_org(i0[a], j0[a])}; }
  // row: the global row of the cell
  __device__ __forceinline__ void store(int64_t a, int row, int2 c) const {
    h[a] = __builtin_bit_cast(float, c.x);
    i0[a] = c.y >= 0 ? al_org_row(row, c.y) : -1;
    j0[a] = c.y >= 0 ? (c.y & 0xffff) : -1;
  }
  // the halo cell (row, k): column c0 - 2 + k of strip row `row` (-2, -1: the carried rows) for the panel that starts at c0
  __device__ __forceinline__ int64_t at(int row, int k) const { return 2 * (int64_t)(row + 2) + k; }
};

// One pass of the walk: rows [0, Lq) of the columns [c0, c0 + pw) of a pair's S; row 0 is global row `base`. cell: three LDS rows of
// `cols` cells (row 0 = row i, row 1 = row i - 2, row 2 = row i - 1 at the start), two cells in front of each standing for columns
// c0 - 1 and c0 - 2. The last three members are read by al_walk<., true> only.
struct AlPass {
  const float* Sp;
  size_t ld;
  float theta;
  int Lq, base, c0, pw;
  int2* cell;
  int cols;
  bool first;                  // the panel at c0 == 0: zeros in front of every row
  AlCells halo;
  int2 (*hst)[2 * AL_RB];      // the packed halo cells of the current and the next block of rows
};
struct AlRows {
  int2* prev1;                 // rows Lq - 1 and Lq - 2 after the walk (the rows the fill left, where the pass has fewer rows)
  int2* prev2;
};

// The rows of a pair without cells (bad: its lengths are outside the launch's limits, which the caller checks: this only keeps it in
// bounds; or it has no column) and its open_h.
template <int THREADS>
__device__ __forceinline__ void al_no_cells(bool bad, int Lq, int max_q, float* __restrict__ row_h, int* __restrict__ row_j,
                                            int* __restrict__ row_i0, int* __restrict__ row_j0, float* __restrict__ open_h) {
  const int n = bad ? min(max(Lq, 0), max_q) : Lq;
  for (int i = threadIdx.x; i < n; i += THREADS) {
    row_h[i] = 0.f;
    row_j[i] = -1;
    row_i0[i] = -1;
    row_j0[i] = -1;
  }
  if (threadIdx.x == 0) *open_h = bad ? -1.f : 0.f;
}

// The three LDS rows before a pass: zeros (H = +0.0, no origin), in rows i - 1 and i - 2 the pass's slice of the carry if the pair is
// carried, and in front of them the carried rows' halo in every panel but the first. The caller's barrier follows.
template <int THREADS>
__device__ __forceinline__ void al_fill(const AlPass& w, bool carried, const AlCells& carry, int Lr) {
  for (int t = threadIdx.x; t < 3 * w.cols; t += THREADS) {
    const int r = t / w.cols, j = t - r * w.cols - 2;
    int2 v = int2{0, -1};
    if (r > 0 && j >= 0) {
      if (carried && j < w.pw) v = carry.load((r == 2 ? 0 : Lr) + w.c0 + j);
    } else if (r > 0 && !w.first) {
      v = w.halo.load(w.halo.at(r == 2 ? -1 : -2, j + 2));
    }
    w.cell[t] = v;
  }
}

// The pass's slice of the carry out: rows.prev1 / prev2 are global rows last and last - 1 (with Lq == 1 the latter is the old row -1;
// store = false with Lq == 0: nothing moved and nothing is stored). Returns m joined with the largest H of the thread's cells.
template <int THREADS>
__device__ __forceinline__ float al_carry_out(const AlPass& w, const AlRows& rows, const AlCells& carry, int Lr, int last, bool store,
                                              float m) {
  for (int j = threadIdx.x; j < w.pw; j += THREADS) {
    const int2 c1 = rows.prev1[j + 2], c2 = rows.prev2[j + 2];
    m = fmaxf(m, fmaxf(__builtin_bit_cast(float, c1.x), __builtin_bit_cast(float, c2.x)));
    if (store) {
      carry.store(w.c0 + j, last, c1);
      carry.store(Lr + w.c0 + j, last - 1, c2);
    }
  }
  return m;
}

// open_h = the workgroup's largest m
template <int THREADS>
__device__ __forceinline__ void al_open_h(float m, float* __restrict__ open_h) {
  constexpr int NW = THREADS / NSID_WAVE;
  __shared__ float wmax[NW];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, NSID_WAVE));
  if ((threadIdx.x & (NSID_WAVE - 1)) == 0) wmax[threadIdx.x / NSID_WAVE] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = 0.f;
    for (int u = 0; u < NW; ++u) v = fmaxf(v, wmax[u]);
    *open_h = v;
  }
}

// The walk itself, the one place where the rule of include/nsid.h is written: threads own columns, one barrier per row. A row's best
// key and that cell's origin reach sink(row, key, org, buf) between the barriers of rows `row` and `row + 1` (the last row's after the
// last barrier); buf is the row's cells. HALO: the pass is a panel; the cells in front of each row come from w.hst (w.first: zeros),
// a block of rows ahead of their use.
template <int THREADS, bool HALO, class Sink>
__device__ __forceinline__ AlRows al_walk(const AlPass& w, Sink&& sink) {
  constexpr int NW = THREADS / NSID_WAVE;
  __shared__ unsigned long long part[2][NW];
  const int tid = threadIdx.x, lane = tid & (NSID_WAVE - 1), wave = tid / NSID_WAVE;

  // the waves' keys of the row -> its result. Every wave does the (broadcast) reads, so that they are scheduled among the row's own
  // reads and no wave is later at the barrier than the others; the sink says which threads store
  auto combine = [&](int row, const int2* buf) {
    unsigned long long k = 0;
#pragma unroll
    for (int u = 0; u < NW; ++u) {
      const unsigned long long v = part[row & 1][u];
      k = v > k ? v : k;
    }
    const int j = k ? (int)(0xffffffffu - (unsigned)k) : -1;
    sink(row, k, buf[max(j - w.c0, 0) + 2].y, buf);
  };

  int2* cur = w.cell;                    // row i
  int2* prev1 = w.cell + 2 * w.cols;     // row i - 1
  int2* prev2 = w.cell + w.cols;         // row i - 2
  const bool stage = HALO && !w.first && tid < 2 * AL_RB;      // this thread loads the halo cell (row tid / 2, column tid % 2) of a block
  // AL_RB rows of S per thread at a time, all their loads in flight together: the memory latency is paid once per AL_RB rows, not per row
  // (columns past the pass's end read its last column and are not used)
  for (int ib = 0; ib < w.Lq; ib += AL_RB) {
    float sv[AL_RB][AL_CPT];
#pragma unroll
    for (int r = 0; r < AL_RB; ++r) {
      const float* rp = w.Sp + (size_t)min(ib + r, w.Lq - 1) * w.ld + w.c0;
#pragma unroll
      for (int c = 0; c < AL_CPT; ++c) sv[r][c] = rp[min(tid + c * THREADS, w.pw - 1)];
    }
    const int hb = (ib / AL_RB) & 1;
    const bool more = stage && ib + AL_RB < w.Lq;              // the halo of the next block of rows is loaded during this one
    int2 hnext = int2{0, -1};
#pragma unroll
    for (int r = 0; r < AL_RB; ++r) {
      const int i = ib + r;
      if (i >= w.Lq) break;              // uniform
      if (i > 0) combine(i - 1, prev1);
      if constexpr (HALO) {
        // issued when half of the block's S is consumed (the registers are free by then), stored four rows later
        if (r == AL_RB / 2 && more) hnext = w.halo.load(w.halo.at(min(ib + AL_RB + (tid >> 1), w.Lq - 1), tid & 1));
      }
      const int own = (((w.base + i) & (AL_I0_MOD - 1)) << 16) | w.c0;      // a path that starts in this row, at local column 0
      unsigned long long key = 0;
      // branch-free over the thread's columns (a column past the pass's end reads the last one and writes nothing), so that the LDS
      // reads of all of them are in flight together
      int2 d11[AL_CPT], d12[AL_CPT], d21[AL_CPT];
#pragma unroll
      for (int c = 0; c < AL_CPT; ++c) {
        const int jc = min(tid + c * THREADS, w.pw - 1);
        d11[c] = prev1[jc + 1];
        d12[c] = prev1[jc];
        d21[c] = prev2[jc + 1];
      }
      if constexpr (HALO) {
        if (tid < 2) cur[tid] = w.first ? int2{0, -1} : w.hst[hb][2 * r + tid];
        if (r == AL_RB - 1 && more) w.hst[hb ^ 1][tid] = hnext;             // read from the next row on, after this row's barrier
      }
#pragma unroll
      for (int c = 0; c < AL_CPT; ++c) {
        const int j = tid + c * THREADS;
        const float e = sv[r][c] - w.theta;
        float best = 0.f;
        int from = -1;
        const float h11 = __builtin_bit_cast(float, d11[c].x), h12 = __builtin_bit_cast(float, d12[c].x),
                    h21 = __builtin_bit_cast(float, d21[c].x);
        if (h11 > best) {
          best = h11;
          from = d11[c].y;
        }
        if (h12 > best) {
          best = h12;
          from = d12[c].y;
        }
        if (h21 > best) {
          best = h21;
          from = d21[c].y;
        }
        const float v = best + e;
        const bool pos = v > 0.f;
        if (j < w.pw) cur[j + 2] = int2{pos ? __builtin_bit_cast(int, v) : 0, pos ? (from >= 0 ? from : (own + j)) : -1};
        const unsigned long long k = (j < w.pw && e > 0.f) ? al_key(v, w.c0 + j) : 0ull;
        key = k > key ? k : key;
      }
      key = al_wave_key_max(key);
      if (lane == 0) part[i & 1][wave] = key;
      int2* t = prev2;
      prev2 = prev1;
      prev1 = cur;
      cur = t;
      // the row's barrier orders LDS only: a sink's stores to memory, which nobody reads before the walk ends, stay in flight over it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    }
  }
  if (w.Lq > 0) combine(w.Lq - 1, prev1);
  return AlRows{prev1, prev2};
}

// ---- local_align: the walk over the whole matrix from zeros, then the pair's occurrences -------------------------------------------
// cols: cells per LDS row = max_x + 2. Dynamic LDS: three rows of cells during the walk, then the row results (h, origin) of the pair.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void local_align_kernel(const float* __restrict__ S, const int64_t* __restrict__ s_off,
                                                              const int* __restrict__ s_ld, const int* __restrict__ q_len,
                                                              const int* __restrict__ x_len, int max_q, int max_x, int cols, float theta,
                                                              float min_score, int top, const int64_t* __restrict__ row_off,
                                                              float* __restrict__ row_h, int* __restrict__ row_j,
                                                              int* __restrict__ row_org, int* __restrict__ occ,
                                                              float* __restrict__ occ_score, int* __restrict__ n_occ) {
  constexpr int NW = THREADS / NSID_WAVE;
  extern __shared__ __attribute__((aligned(16))) char al_smem[];
  __shared__ int o_occ[AL_MAX_TOP][4];
  __shared__ float o_sc[AL_MAX_TOP];
  __shared__ int wcnt[NW];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (NSID_WAVE - 1), w = tid / NSID_WAVE;
  const int Lq = q_len[p], Lr = x_len[p];
  // every return below is uniform over the workgroup and ahead of every barrier
  if (Lq < 0 || Lr < 0 || Lq > max_q || Lr > max_x) {       // the caller checks the lengths; this only keeps a bad pair in bounds
    al_empty(p, top, -1, tid, occ, occ_score, n_occ);
    return;
  }
  if (Lq == 0 || Lr == 0) {
    al_empty(p, top, 0, tid, occ, occ_score, n_occ);
    for (int i = tid; i < Lq; i += THREADS) {                // rows without a column: no cell, so 0, -1, -1
      row_h[row_off[p] + i] = 0.f;
      row_j[row_off[p] + i] = -1;
      row_org[row_off[p] + i] = -1;
    }
    return;
  }
  const int64_t ro = row_off[p];

  int2* cell = reinterpret_cast<int2*>(al_smem);
  for (int t = tid; t < 3 * cols; t += THREADS) cell[t] = int2{0, -1};        // H = +0.0, no origin
  if (tid < AL_MAX_TOP) {
    o_occ[tid][0] = o_occ[tid][1] = o_occ[tid][2] = o_occ[tid][3] = -1;
    o_sc[tid] = 0.f;
  }
  __syncthreads();

  al_walk<THREADS, false>(AlPass{S + s_off[p], (size_t)s_ld[p], theta, Lq, 0, 0, Lr, cell, cols, true, {}, nullptr},
                          [&](int row, unsigned long long k, int org, const int2*) {
                            if (tid == 0) {
                              row_h[ro + row] = __builtin_bit_cast(float, (unsigned)(k >> 32));
                              row_j[ro + row] = k ? (int)(0xffffffffu - (unsigned)k) : -1;
                              row_org[ro + row] = k ? org : -1;
                            }
                          });
  __syncthreads();                   // the row results are in memory for the whole workgroup; the cells are dead

  // ---- occurrences: the rows grouped by origin, a group's best row, the kept ones ranked
  float* rh = reinterpret_cast<float*>(al_smem);
  int* rg = reinterpret_cast<int*>(al_smem) + max_q;
  for (int i = tid; i < Lq; i += THREADS) {
    rh[i] = row_h[ro + i];
    rg[i] = row_org[ro + i];
  }
  __syncthreads();
  unsigned keep_mask = 0;
  int n_keep = 0;
#pragma unroll
  for (int c = 0; c < AL_CPT; ++c) {
    const int i = tid + c * THREADS;
    if (i >= Lq) continue;
    const int og = rg[i];
    const float hi = rh[i];
    bool rep = og >= 0 && hi >= min_score;
    for (int i0 = 0; i0 < Lq && rep; i0 += AL_CHUNK) {
      bool hit = false;
#pragma unroll
      for (int u = 0; u < AL_CHUNK; ++u) {
        const int a = i0 + u, ac = min(a, Lq - 1);
        const float ha = rh[ac];
        hit |= (a < Lq) & (rg[ac] == og) & ((ha > hi) | ((ha == hi) & (a < i)));
      }
      rep = !hit;
    }
    if (rep) {
      keep_mask |= 1u << c;
      ++n_keep;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_keep += __shfl_xor(n_keep, o, NSID_WAVE);
  if (lane == 0) wcnt[w] = n_keep;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < AL_CPT; ++c) {
    const int i = tid + c * THREADS;
    if (i < Lq && !((keep_mask >> c) & 1u)) rg[i] = -1;         // from here on rg >= 0 marks a kept occurrence
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < AL_CPT; ++c) {
    const int i = tid + c * THREADS;
    if (!((keep_mask >> c) & 1u)) continue;
    const int og = rg[i];
    const float hi = rh[i];
    int rank = 0;
    for (int i0 = 0; i0 < Lq && rank < top; i0 += AL_CHUNK) {
#pragma unroll
      for (int u = 0; u < AL_CHUNK; ++u) {
        const int a = i0 + u, ac = min(a, Lq - 1);
        const float ha = rh[ac];
        const int oa = rg[ac];
        rank += ((a < Lq) & (oa >= 0) & ((ha > hi) | ((ha == hi) & (oa < og)))) ? 1 : 0;
      }
    }
    if (rank < top) {
      o_occ[rank][0] = og >> 16;
      o_occ[rank][1] = i;
      o_occ[rank][2] = og & 0xffff;
      o_occ[rank][3] = row_j[ro + i];
      o_sc[rank] = hi;
    }
  }
  __syncthreads();
  if (tid < top) {
    int* o = occ + ((size_t)p * top + tid) * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = o_occ[tid][u];
    occ_score[(size_t)p * top + tid] = o_sc[tid];
  }
  if (tid == 0) {
    int n = 0;
    for (int u = 0; u < NW; ++u) n += wcnt[u];
    n_occ[p] = n;
  }
}

// ---- local_align_strip: the walk over the whole width from two carried rows to two carried rows ------------------------------------
// (include/nsid.h nsid_local_align_strip.) The carry stands where local_align's zeros stand, and after the walk the two LDS rows that
// are rows -1 and -2 at that point go back to the carry; open_h = the largest H in them.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void local_align_strip_kernel(
    const float* __restrict__ S, const int64_t* __restrict__ s_off, const int* __restrict__ s_ld, const int* __restrict__ q_len,
    const int* __restrict__ x_len, const int* __restrict__ row_base, const int* __restrict__ fresh, int max_q, int max_x, int cols,
    float theta, const int64_t* __restrict__ carry_off, float* carry_h, int* carry_i0, int* carry_j0,
    const int64_t* __restrict__ row_off, float* __restrict__ row_h, int* __restrict__ row_j, int* __restrict__ row_i0,
    int* __restrict__ row_j0, float* __restrict__ open_h) {
  extern __shared__ __attribute__((aligned(16))) char al_smem[];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int Lq = q_len[p], Lr = x_len[p], base = row_base[p];
  const int64_t ro = row_off[p];
  // every return below is uniform over the workgroup and ahead of every barrier
  const bool bad = Lq < 0 || Lr < 0 || Lq > max_q || Lr > max_x || base < 0 || (int64_t)base + Lq > 0x7fffffffLL;
  if (bad || Lr == 0) {
    al_no_cells<THREADS>(bad, Lq, max_q, row_h + ro, row_j + ro, row_i0 + ro, row_j0 + ro, open_h + p);
    return;
  }
  const AlCells carry(carry_h, carry_i0, carry_j0, carry_off[p]);
  const AlPass w{S + s_off[p], (size_t)s_ld[p], theta, Lq, base, 0, Lr, reinterpret_cast<int2*>(al_smem), cols, true, {}, nullptr};
  al_fill<THREADS>(w, fresh[p] == 0, carry, Lr);
  __syncthreads();
  const AlRows rows = al_walk<THREADS, false>(w, [&](int row, unsigned long long k, int org, const int2*) {
    if (tid == 0) {
      const bool has = k != 0 && org >= 0;
      row_h[ro + row] = __builtin_bit_cast(float, (unsigned)(k >> 32));
      row_j[ro + row] = k ? (int)(0xffffffffu - (unsigned)k) : -1;
      row_i0[ro + row] = has ? al_org_row(base + row, org) : -1;
      row_j0[ro + row] = has ? (org & 0xffff) : -1;
    }
  });
  al_open_h<THREADS>(al_carry_out<THREADS>(w, rows, carry, Lr, base + Lq - 1, Lq > 0, 0.f), open_h + p);
}

// ---- local_align_panels: the strip in passes of pcols columns, for songs of up to AL_MAX_SONG_ROWS rows -----------------------------
// (include/nsid.h nsid_local_align_panels.) The rule reads (i-1, j-1), (i-1, j-2) and (i-2, j-1), so a panel that starts at column c0
// needs from its left only columns c0 - 2 and c0 - 1 of every row, the two carried ones included: the halo. The two cells in front of
// each LDS row, zeros in the first panel, hold the halo of that row in every later one. The halo cells of a block of AL_RB rows are
// loaded during the block before, a cell a thread, and left packed in LDS before that block's last barrier; threads 0 and 1 put them
// in front of the row being computed (al_walk<., true>) and, after the row's barrier, store the row's last two cells over them for
// the next panel (the sink; a row's halo is consumed at least one barrier before it is overwritten). A panel stores the halo of the
// carried rows before its slice of the carry is overwritten. A row's best key over the panels so far and that cell's origin stay in
// LDS behind the cells; a later panel replaces them only with a strictly larger H (it has the larger j), and the rows go to memory
// once, after the last panel.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void local_align_panels_kernel(
    const float* __restrict__ S, const int64_t* __restrict__ s_off, const int* __restrict__ s_ld, const int* __restrict__ q_len,
    const int* __restrict__ x_len, const int* __restrict__ row_base, const int* __restrict__ fresh, int max_q, int max_x, int pcols,
    float theta, const int64_t* __restrict__ carry_off, float* carry_h, int* carry_i0, int* carry_j0,
    const int64_t* __restrict__ halo_off, float* halo_h, int* halo_i0, int* halo_j0, const int64_t* __restrict__ row_off,
    float* __restrict__ row_h, int* __restrict__ row_j, int* __restrict__ row_i0, int* __restrict__ row_j0,
    float* __restrict__ open_h) {
  extern __shared__ __attribute__((aligned(16))) char al_smem[];
  __shared__ int2 hst[2][2 * AL_RB];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int Lq = q_len[p], Lr = x_len[p], base = row_base[p];
  const int64_t ro = row_off[p];
  // every return below is uniform over the workgroup and ahead of every barrier
  const bool bad = Lq < 0 || Lr < 0 || Lq > max_q || Lr > max_x || base < 0 || (int64_t)base + Lq > 0x7fffffffLL;
  if (bad || Lr == 0) {
    al_no_cells<THREADS>(bad, Lq, max_q, row_h + ro, row_j + ro, row_i0 + ro, row_j0 + ro, open_h + p);
    return;
  }
  const AlCells carry(carry_h, carry_i0, carry_j0, carry_off[p]), halo(halo_h, halo_i0, halo_j0, halo_off[p]);
  const bool carried = fresh[p] == 0;
  const int cols = pcols + 2;

  // LDS: three rows of cells, then per strip row the best key so far and that cell's packed origin
  int2* cell = reinterpret_cast<int2*>(al_smem);
  unsigned long long* rkey = reinterpret_cast<unsigned long long*>(cell + 3 * cols);
  int* rorg = reinterpret_cast<int*>(rkey + max_q);
  for (int i = tid; i < Lq; i += THREADS) {
    rkey[i] = 0ull;
    rorg[i] = -1;
  }

  float m = 0.f;
  for (int c0 = 0; c0 < Lr; c0 += pcols) {
    const int pw = min(pcols, Lr - c0);                       // only the last panel can be narrower (and only it can have one column)
    const bool first = c0 == 0, last = c0 + pw >= Lr;
    const AlPass w{S + s_off[p], (size_t)s_ld[p], theta, Lq, base, c0, pw, cell, cols, first, halo, hst};
    al_fill<THREADS>(w, carried, carry, Lr);
    if (!first && tid < 2 * AL_RB && Lq > 0) hst[0][tid] = halo.load(halo.at(min(tid >> 1, Lq - 1), tid & 1));      // the first block's halo
    __syncthreads();
    // the carried rows' cells for the next panel, before this panel's slice of the carry is overwritten
    if (!last && tid < 2) {
      halo.store(halo.at(-2, tid), base - 2, cell[cols + pw + tid]);
      halo.store(halo.at(-1, tid), base - 1, cell[2 * cols + pw + tid]);
    }
    // the row's best of this panel against its best of the earlier panels; its last two cells for the next panel
    const AlRows rows = al_walk<THREADS, true>(w, [&](int row, unsigned long long k, int org, const int2* buf) {
      if (tid == 0 && (k >> 32) > (rkey[row] >> 32)) {
        rkey[row] = k;
        rorg[row] = org;
      }
      if (!last && tid < 2) halo.store(halo.at(row, tid), base + row, buf[pw + tid]);
    });
    m = al_carry_out<THREADS>(w, rows, carry, Lr, base + Lq - 1, Lq > 0, m);
    __syncthreads();                   // the cells are dead, the halo and the row keys are written: the next panel may start
  }

  for (int i = tid; i < Lq; i += THREADS) {
    const unsigned long long k = rkey[i];
    const int org = rorg[i];
    const bool has = k != 0 && org >= 0;
    row_h[ro + i] = __builtin_bit_cast(float, (unsigned)(k >> 32));
    row_j[ro + i] = k ? (int)(0xffffffffu - (unsigned)k) : -1;
    row_i0[ro + i] = has ? al_org_row(base + i, org) : -1;
    row_j0[ro + i] = has ? (org & 0xffff) : -1;
  }
  al_open_h<THREADS>(m, open_h + p);
}

// The dynamic LDS of the three, as each entry asks for it.
size_t align_lds_bytes(int max_q, int max_x) {
  const size_t walk = 3 * (size_t)(max_x + 2) * sizeof(int2), rows = 2 * (size_t)max_q * sizeof(int);
  return (std::max(walk, rows) + 15) / 16 * 16;
}
size_t align_strip_lds_bytes(int max_x) { return (3 * (size_t)(max_x + 2) * sizeof(int2) + 15) / 16 * 16; }
size_t align_panels_lds_bytes(int max_q, int pcols) {
  return (3 * (size_t)(pcols + 2) * sizeof(int2) + (size_t)max_q * 12 + 15) / 16 * 16;
}

// 256 threads own every column (in local_align also every row) of a pass up to `width` = 1024; above that 1024 threads do. The results
// do not depend on it. The entry ends here.
#define AL_LAUNCH(kernel, width, npairs, lds, st, ...)                                                  \
  do {                                                                                                  \
    if ((width) <= 256 * AL_CPT) {                                                                      \
      nsid_took(#kernel "<256>");                                                                       \
      NSID_LAUNCH_LDS((kernel<256>), dim3(npairs), dim3(256), lds, st, __VA_ARGS__);                    \
    } else {                                                                                            \
      nsid_took(#kernel "<1024>");                                                                      \
      NSID_LAUNCH_LDS((kernel<1024>), dim3(npairs), dim3(1024), lds, st, __VA_ARGS__);                  \
    }                                                                                                   \
    return nsid_launch_status();                                                                        \
  } while (0)

// ---- align_paths: the path of an occurrence, traced back through its own box ----------------------------------------------------------
// (include/nsid.h nsid_align_paths.) One workgroup per box. The forward pass is the rule on the box alone from zeros; a thread owns
// AL_PATH_CPT = 4 neighbouring columns, so that their step codes (2 bits a cell: 0 none, 1 = (1,1), 2 = (1,2), 3 = (2,1)) are one
// byte that it alone stores: no atomics. Three rotating LDS rows of H alone (two zeros in front of each, a row a multiple of 16 bytes),
// one barrier per row that orders LDS only, S read AL_RB rows at a time as in al_walk. This is the second statement of the rule in
// this file: al_walk keeps origins, reduces a row's best key and serves three measured kernels, so it stays as it is and the cell is
// restated here in the same words. The traceback reads codes that other threads stored to memory, so it stands behind a
// __syncthreads(), whose fences cover memory; thread 0 follows the codes from the last cell (a path has at most min(rows, columns)
// cells: every step advances both indices) and leaves the cells in LDS, over the dead rows; the workgroup stores them in forward order.
constexpr int AL_PATH_MAX = NSID_ALIGN_PATH_MAX;
constexpr int AL_PATH_CPT = 4;
static_assert(AL_PATH_MAX <= 1024 * AL_PATH_CPT, "1024 threads own AL_PATH_CPT columns each");
static_assert(AL_PATH_MAX <= (1 << 15), "a path cell is kept as i << 16 | j in LDS");
// floats of one LDS row: columns -2 .. max_cols + 3 (a thread writes its four columns whole), rounded to 16 bytes
constexpr int al_path_ld(int max_cols) { return (max_cols + 2 + AL_PATH_CPT + 3) / 4 * 4; }
size_t align_paths_lds_bytes(int max_cols) { return 3 * (size_t)al_path_ld(max_cols) * sizeof(float); }
static_assert(3 * (size_t)al_path_ld(AL_PATH_MAX) * sizeof(float) + 1024 <= NSID_LDS_MAX, "three rows of H in LDS");

template <int THREADS>
__global__ __launch_bounds__(THREADS) void align_paths_kernel(
    const float* __restrict__ S, const int64_t* __restrict__ s_off, const int* __restrict__ s_ld, const int* __restrict__ n_rows,
    const int* __restrict__ n_cols, const int* __restrict__ i_base, const int* __restrict__ j_base, int max_cols, float theta,
    const int64_t* __restrict__ path_off, const int64_t* __restrict__ dir_off, uint8_t* dirs, int* __restrict__ path_len,
    int* __restrict__ path_i, int* __restrict__ path_j, float* __restrict__ path_s, float* __restrict__ end_h) {
  extern __shared__ __attribute__((aligned(16))) char al_smem[];
  __shared__ int s_n;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nr = n_rows[p], nc = n_cols[p];
  const int ib0 = i_base ? i_base[p] : 0, jb0 = j_base ? j_base[p] : 0;
  // every return below is uniform over the workgroup and ahead of every barrier
  if (nr < 0 || nc < 0 || nr > AL_PATH_MAX || nc > max_cols || ib0 < 0 || jb0 < 0 || (int64_t)ib0 + nr > 0x7fffffffLL ||
      (int64_t)jb0 + nc > 0x7fffffffLL) {                   // the box is not read
    if (tid == 0) {
      path_len[p] = -2;
      end_h[p] = 0.f;
    }
    return;
  }
  if (nr == 0 || nc == 0) {
    if (tid == 0) {
      path_len[p] = 0;
      end_h[p] = 0.f;
    }
    return;
  }
  const int ld = al_path_ld(max_cols);
  float* row = reinterpret_cast<float*>(al_smem);
  for (int t = tid; t < 3 * ld; t += THREADS) row[t] = 0.f;            // H = +0.0 everywhere, the two cells in front of each row for good
  __syncthreads();

  const float* Sp = S + s_off[p];
  const size_t sld = (size_t)s_ld[p];
  uint8_t* dp = dirs + dir_off[p];
  const int dld = (nc + AL_PATH_CPT - 1) / AL_PATH_CPT;                // bytes of a row of step codes
  const int j = AL_PATH_CPT * tid;                                      // this thread's first column
  const bool mine = j < nc;                                             // tid < dld
  float* cur = row;                      // row i; element c + 2 is column c
  float* prev1 = row + 2 * ld;           // row i - 1
  float* prev2 = row + ld;               // row i - 2
  for (int ib = 0; ib < nr; ib += AL_RB) {
    float sv[AL_RB][AL_PATH_CPT];
    if (mine) {                          // columns past the box's end read its last column and are not used
#pragma unroll
      for (int r = 0; r < AL_RB; ++r) {
        const float* rp = Sp + (size_t)min(ib + r, nr - 1) * sld;
#pragma unroll
        for (int c = 0; c < AL_PATH_CPT; ++c) sv[r][c] = rp[min(j + c, nc - 1)];
      }
    }
#pragma unroll
    for (int r = 0; r < AL_RB; ++r) {
      const int i = ib + r;
      if (i >= nr) break;                // uniform
      if (mine) {
        // columns j - 2 .. j + 2 of row i - 1 and j - 1 .. j + 2 of row i - 2
        const f32x4 a = *reinterpret_cast<const f32x4*>(prev1 + j), b = *reinterpret_cast<const f32x4*>(prev2 + j);
        const float p1[AL_PATH_CPT + 1] = {a[0], a[1], a[2], a[3], prev1[j + 4]};
        const float p2[AL_PATH_CPT + 1] = {b[0], b[1], b[2], b[3], prev2[j + 4]};
        float h[AL_PATH_CPT];
        unsigned codes = 0;
#pragma unroll
        for (int c = 0; c < AL_PATH_CPT; ++c) {
          const float e = sv[r][c] - theta;
          float best = 0.f;
          unsigned from = 0;
          const float h11 = p1[c + 1], h12 = p1[c], h21 = p2[c + 1];
          if (h11 > best) {
            best = h11;
            from = 1;
          }
          if (h12 > best) {
            best = h12;
            from = 2;
          }
          if (h21 > best) {
            best = h21;
            from = 3;
          }
          const float v = best + e;
          const bool pos = v > 0.f;
          h[c] = pos ? v : 0.f;
          codes |= ((pos && j + c < nc) ? from : 0u) << (2 * c);
        }
        *reinterpret_cast<float2*>(cur + j + 2) = float2{h[0], h[1]};
        *reinterpret_cast<float2*>(cur + j + 4) = float2{h[2], h[3]};
        dp[(size_t)i * dld + tid] = (uint8_t)codes;
      }
      float* t = prev2;
      prev2 = prev1;
      prev1 = cur;
      cur = t;
      // the row's barrier orders LDS only: the step codes, which nobody reads before the walk ends, stay in flight over it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    }
  }
  __syncthreads();                       // memory too: every thread's step codes are visible to the workgroup

  int* cells = reinterpret_cast<int*>(al_smem);       // the path, last cell first; thread 0 has read the last H before it writes here
  if (tid == 0) {
    const float hl = prev1[nc - 1 + 2];
    int n = -1;
    if (hl > 0.f) {
      int i = nr - 1, c = nc - 1;
      n = 0;
      for (;;) {
        cells[n++] = (i << 16) | c;
        const unsigned code = ((unsigned)dp[(size_t)i * dld + (c >> 2)] >> (2 * (c & 3))) & 3u;
        if (code == 0) break;            // the path's first cell
        i -= code == 3 ? 2 : 1;
        c -= code == 2 ? 2 : 1;
        if (i < 0 || c < 0) break;       // never with the codes of this pass (a chosen predecessor has H > 0, so it lies in the box)
      }
      if (i != 0 || c != 0) n = -1;      // the path starts elsewhere: the box is not an occurrence
    }
    s_n = n;
    path_len[p] = n;
    end_h[p] = hl;
  }
  __syncthreads();
  const int n = s_n;
  const int64_t po = path_off[p];
  for (int k = tid; k < n; k += THREADS) {
    const int cell = cells[n - 1 - k], i = cell >> 16, c = cell & 0xffff;
    path_i[po + k] = ib0 + i;
    path_j[po + k] = jb0 + c;
    path_s[po + k] = Sp[(size_t)i * sld + c];
  }
}

// ---- align_occurrences ------------------------------------------------------------------------------------------------------------
// One workgroup per run of rows. A group's rows lie within [i0, i0 + AL_SPAN], so a row is its group's representative when no row of
// that window with the same origin beats it; the kept rows are one bit each in LDS (a wave's ballot per 64 rows), and a kept row's rank
// is a walk over the set bits. The rows themselves are read from memory (they stay in the caches). span: per run the width of that
// window (nsid_align_occurrences_span: 2 (x_len - 1) for a song of x_len rows); null = AL_SPAN, the bound of a song of AL_MAX_COLS rows.
constexpr int AL_OCC_THREADS = 1024;
static_assert(NSID_ALIGN_OCC_MAX_ROWS / 8 + 4096 <= NSID_LDS_MAX, "one bit per row of the longest run in LDS");

__global__ __launch_bounds__(AL_OCC_THREADS) void align_occurrences_kernel(
    const float* __restrict__ row_h, const int* __restrict__ row_j, const int* __restrict__ row_i0, const int* __restrict__ row_j0,
    const int64_t* __restrict__ row_off, const int* __restrict__ n_rows, const int* __restrict__ first_row,
    const int* __restrict__ span, int max_rows, float min_score, int top, int* __restrict__ occ, float* __restrict__ occ_score,
    int* __restrict__ n_occ) {
  constexpr int NW = AL_OCC_THREADS / NSID_WAVE;
  extern __shared__ __attribute__((aligned(16))) unsigned al_keep[];
  __shared__ int o_occ[AL_MAX_TOP][4];
  __shared__ float o_sc[AL_MAX_TOP];
  __shared__ int wcnt[NW];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (NSID_WAVE - 1), w = tid / NSID_WAVE;
  const int n = n_rows[p], first = first_row[p], sp = span ? span[p] : AL_SPAN;
  // every return below is uniform over the workgroup and ahead of every barrier
  if (n < 0 || n > max_rows || first < 0 || (int64_t)first + n > 0x7fffffffLL || sp < 0) {
    al_empty(p, top, -1, tid, occ, occ_score, n_occ);
    return;
  }
  if (n == 0) {
    al_empty(p, top, 0, tid, occ, occ_score, n_occ);
    return;
  }
  const int64_t ro = row_off[p];
  const float* rh = row_h + ro;
  const int* rj = row_j + ro;
  const int* ri = row_i0 + ro;
  const int* rc = row_j0 + ro;
  if (tid < AL_MAX_TOP) {
    o_occ[tid][0] = o_occ[tid][1] = o_occ[tid][2] = o_occ[tid][3] = -1;
    o_sc[tid] = 0.f;
  }
  const int nblk = (n + NSID_WAVE - 1) / NSID_WAVE;
  int cnt = 0;
  for (int b = w; b < nblk; b += NW) {
    const int i = b * NSID_WAVE + lane;
    bool rep = false;
    if (i < n) {
      const int gi = ri[i], gj = rc[i];
      const float hi = rh[i];
      rep = gi >= 0 && hi >= min_score;
      const int64_t lo = max((int64_t)0, (int64_t)gi - first), last = min((int64_t)n - 1, (int64_t)gi + sp - first);
      for (int64_t a0 = lo; a0 <= last && rep; a0 += AL_CHUNK) {
        bool hit = false;
#pragma unroll
        for (int u = 0; u < AL_CHUNK; ++u) {
          const int64_t a = a0 + u, ac = min(a, last);
          const float ha = rh[ac];
          hit |= (a <= last) & (ri[ac] == gi) & (rc[ac] == gj) & ((ha > hi) | ((ha == hi) & (ac < i)));
        }
        rep = !hit;
      }
    }
    const unsigned long long m = __ballot(rep);
    if (lane == 0) {
      al_keep[2 * b] = (unsigned)m;
      al_keep[2 * b + 1] = (unsigned)(m >> 32);
      cnt += __popcll(m);
    }
  }
  if (lane == 0) wcnt[w] = cnt;
  __syncthreads();
  const int nwords = 2 * nblk;
  for (int b = w; b < nblk; b += NW) {
    const int i = b * NSID_WAVE + lane;
    if (!((al_keep[i >> 5] >> (i & 31)) & 1u)) continue;       // bits past the run's end are 0; no barrier inside the loop
    const int gi = ri[i], gj = rc[i];
    const float hi = rh[i];
    int rank = 0;
    for (int wd = 0; wd < nwords && rank < top; ++wd) {
      unsigned bits = al_keep[wd];
      while (bits) {
        const int a = wd * 32 + __builtin_ctz(bits);
        bits &= bits - 1;
        const float ha = rh[a];
        const int ai = ri[a], aj = rc[a];
        rank += ((ha > hi) | ((ha == hi) & ((ai < gi) | ((ai == gi) & (aj < gj))))) ? 1 : 0;
      }
    }
    if (rank < top) {
      o_occ[rank][0] = gi;
      o_occ[rank][1] = first + i;
      o_occ[rank][2] = gj;
      o_occ[rank][3] = rj[i];
      o_sc[rank] = hi;
    }
  }
  __syncthreads();
  if (tid < top) {
    int* o = occ + ((size_t)p * top + tid) * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = o_occ[tid][u];
    occ_score[(size_t)p * top + tid] = o_sc[tid];
  }
  if (tid == 0) {
    int k = 0;
    for (int u = 0; u < NW; ++u) k += wcnt[u];
    n_occ[p] = k;
  }
}

static inline bool al_aligned(const void* p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

bool sim_d_ok(int d) { return (d % 16 == 0 && d >= 16 && d <= 256) || (d % 64 == 0 && d > 256 && d <= 2048); }

}  // namespace

extern "C" int nsid_pair_sim(const float* q, int ldq, int nq, const float* x, int ldx, long nx, int d, const int* q_start,
                             const int* q_len, const int64_t* x_start, const int* x_len, const int64_t* s_off, const int* s_ld,
                             int npairs, const int* tiles, int ntiles, float* S, int64_t s_len, void* stream) {
  NSID_REQUIRE(sim_d_ok(d) && nq >= 0 && nx >= 0 && npairs >= 0 && ntiles >= 0 && s_len >= 0);
  if (npairs == 0 || ntiles == 0) return NSID_OK;
  NSID_REQUIRE(q && x && q_start && q_len && x_start && x_len && s_off && s_ld && tiles && S);
  NSID_REQUIRE(ldq >= d && ldq % 4 == 0 && ldx >= d && ldx % 4 == 0 && nsid_aligned16(q) && nsid_aligned16(x));
  hipStream_t st = static_cast<hipStream_t>(stream);
  nsid_count(NSID_C_pair_sim);
  if (d > 256) {
    NSID_LAUNCH(pair_sim_kernel<true>, dim3(ntiles), dim3(64), 0, st, q, ldq, nq, x, ldx, nx, d, q_start, q_len, x_start, x_len, s_off,
                s_ld, npairs, tiles, S, s_len);
  } else {
    NSID_LAUNCH(pair_sim_kernel<false>, dim3(ntiles), dim3(64), 0, st, q, ldq, nq, x, ldx, nx, d, q_start, q_len, x_start, x_len, s_off,
                s_ld, npairs, tiles, S, s_len);
  }
  return nsid_launch_status();
}

extern "C" int nsid_pair_sim_norm(const float* q, int ldq, int nq, const float* x, int ldx, long nx, int d, const int* q_start,
                                  const int* q_len, const int64_t* x_start, const int* x_len, const int64_t* s_off, const int* s_ld,
                                  int npairs, const int* tiles, int ntiles, float* S, int64_t s_len, const float* q_mu,
                                  const float* q_rs, const float* x_mu, const float* x_rs, void* stream) {
  NSID_REQUIRE(sim_d_ok(d) && nq >= 0 && nx >= 0 && npairs >= 0 && ntiles >= 0 && s_len >= 0);
  if (npairs == 0 || ntiles == 0) return NSID_OK;
  NSID_REQUIRE(q && x && q_start && q_len && x_start && x_len && s_off && s_ld && tiles && S && q_mu && q_rs && x_mu && x_rs);
  NSID_REQUIRE(ldq >= d && ldq % 4 == 0 && ldx >= d && ldx % 4 == 0 && nsid_aligned16(q) && nsid_aligned16(x));
  NSID_REQUIRE(al_aligned(q_mu, 4) && al_aligned(q_rs, 4) && al_aligned(x_mu, 4) && al_aligned(x_rs, 4));
  hipStream_t st = static_cast<hipStream_t>(stream);
  nsid_count(NSID_C_pair_sim_norm);
  if (d > 256) {
    NSID_LAUNCH(pair_sim_norm_kernel<true>, dim3(ntiles), dim3(64), 0, st, q, ldq, nq, x, ldx, nx, d, q_start, q_len, x_start, x_len,
                s_off, s_ld, npairs, tiles, S, s_len, q_mu, q_rs, x_mu, x_rs);
  } else {
    NSID_LAUNCH(pair_sim_norm_kernel<false>, dim3(ntiles), dim3(64), 0, st, q, ldq, nq, x, ldx, nx, d, q_start, q_len, x_start, x_len,
                s_off, s_ld, npairs, tiles, S, s_len, q_mu, q_rs, x_mu, x_rs);
  }
  return nsid_launch_status();
}

extern "C" int nsid_local_align(const float* S, const int64_t* s_off, const int* s_ld, const int* q_len, const int* x_len, int npairs,
                                int max_q_len, int max_x_len, float theta, float min_score, int top, const int64_t* row_off,
                                float* row_h, int* row_j, int* row_org, int* occ, float* occ_score, int* n_occ, void* stream) {
  NSID_REQUIRE(npairs >= 0 && max_q_len >= 0 && max_q_len <= AL_MAX_ROWS && max_x_len >= 0 && max_x_len <= AL_MAX_COLS && top >= 1 &&
               top <= AL_MAX_TOP && theta == theta && min_score == min_score);
  if (npairs == 0) return NSID_OK;
  NSID_REQUIRE(s_off && s_ld && q_len && x_len && row_off && occ && occ_score && n_occ);
  NSID_REQUIRE((max_q_len == 0 || max_x_len == 0) || (S && row_h && row_j && row_org));
  nsid_count(NSID_C_local_align);
  AL_LAUNCH(local_align_kernel, std::max(max_q_len, max_x_len), npairs, align_lds_bytes(max_q_len, max_x_len),
            static_cast<hipStream_t>(stream), S, s_off, s_ld, q_len, x_len, max_q_len, max_x_len, max_x_len + 2, theta, min_score, top,
            row_off, row_h, row_j, row_org, occ, occ_score, n_occ);
}

namespace {
// The arguments nsid_local_align_strip and nsid_local_align_panels share (max_cols: the entry's bound of max_x_len). With npairs == 0
// only the limits are looked at, as before either entry returns NSID_OK for it.
int align_strip_args(const float* S, const int64_t* s_off, const int* s_ld, const int* q_len, const int* x_len, const int* row_base,
                     const int* fresh, int npairs, int max_q_len, int max_x_len, int max_cols, float theta, const int64_t* carry_off,
                     const float* carry_h, const int* carry_i0, const int* carry_j0, const int64_t* row_off, const float* row_h,
                     const int* row_j, const int* row_i0, const int* row_j0, const float* open_h) {
  NSID_REQUIRE(npairs >= 0 && max_q_len >= 0 && max_q_len <= AL_MAX_ROWS && max_x_len >= 0 && max_x_len <= max_cols && theta == theta);
  if (npairs == 0) return NSID_OK;
  NSID_REQUIRE(s_off && s_ld && q_len && x_len && row_base && fresh && carry_off && row_off && open_h);
  NSID_REQUIRE(max_q_len == 0 || (row_h && row_j && row_i0 && row_j0));
  NSID_REQUIRE(max_x_len == 0 || (carry_h && carry_i0 && carry_j0));
  NSID_REQUIRE((max_q_len == 0 || max_x_len == 0) || S);
  NSID_REQUIRE(al_aligned(s_off, 8) && al_aligned(carry_off, 8) && al_aligned(row_off, 8));
  for (const void* q : {(const void*)S, (const void*)s_ld, (const void*)q_len, (const void*)x_len, (const void*)row_base,
                        (const void*)fresh, (const void*)carry_h, (const void*)carry_i0, (const void*)carry_j0, (const void*)row_h,
                        (const void*)row_j, (const void*)row_i0, (const void*)row_j0, (const void*)open_h})
    NSID_REQUIRE(al_aligned(q, 4));
  return NSID_OK;
}
}  // namespace

extern "C" int nsid_local_align_strip(const float* S, const int64_t* s_off, const int* s_ld, const int* q_len, const int* x_len,
                                      const int* row_base, const int* fresh, int npairs, int max_q_len, int max_x_len, float theta,
                                      const int64_t* carry_off, float* carry_h, int* carry_i0, int* carry_j0, const int64_t* row_off,
                                      float* row_h, int* row_j, int* row_i0, int* row_j0, float* open_h, void* stream) {
  const int rc = align_strip_args(S, s_off, s_ld, q_len, x_len, row_base, fresh, npairs, max_q_len, max_x_len, AL_MAX_COLS, theta,
                                  carry_off, carry_h, carry_i0, carry_j0, row_off, row_h, row_j, row_i0, row_j0, open_h);
  if (rc != NSID_OK || npairs == 0) return rc;
  nsid_count(NSID_C_local_align_strip);
  AL_LAUNCH(local_align_strip_kernel, max_x_len, npairs, align_strip_lds_bytes(max_x_len), static_cast<hipStream_t>(stream), S, s_off,
            s_ld, q_len, x_len, row_base, fresh, max_q_len, max_x_len, max_x_len + 2, theta, carry_off, carry_h, carry_i0, carry_j0,
            row_off, row_h, row_j, row_i0, row_j0, open_h);
}

namespace {
int align_occurrences_launch(const float* row_h, const int* row_j, const int* row_i0, const int* row_j0, const int64_t* row_off,
                             const int* n_rows, const int* first_row, const int* span, bool with_span, int npairs, int max_rows,
                             float min_score, int top, int* occ, float* occ_score, int* n_occ, void* stream) {
  NSID_REQUIRE(npairs >= 0 && max_rows >= 0 && max_rows <= NSID_ALIGN_OCC_MAX_ROWS && top >= 1 && top <= AL_MAX_TOP &&
               min_score == min_score);
  if (npairs == 0) return NSID_OK;
  NSID_REQUIRE(row_off && n_rows && first_row && occ && occ_score && n_occ && (!with_span || span));
  NSID_REQUIRE(max_rows == 0 || (row_h && row_j && row_i0 && row_j0));
  NSID_REQUIRE(al_aligned(row_off, 8));
  for (const void* q : {(const void*)row_h, (const void*)row_j, (const void*)row_i0, (const void*)row_j0, (const void*)n_rows,
                        (const void*)first_row, (const void*)span, (const void*)occ, (const void*)occ_score, (const void*)n_occ})
    NSID_REQUIRE(al_aligned(q, 4));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = ((size_t)(max_rows + NSID_WAVE - 1) / NSID_WAVE * 8 + 15) / 16 * 16;
  nsid_count(with_span ? NSID_C_align_occurrences_span : NSID_C_align_occurrences);
  nsid_took("align_occurrences_kernel");
  NSID_LAUNCH_LDS(align_occurrences_kernel, dim3(npairs), dim3(AL_OCC_THREADS), lds, st, row_h, row_j, row_i0, row_j0, row_off, n_rows,
                  first_row, span, max_rows, min_score, top, occ, occ_score, n_occ);
  return nsid_launch_status();
}
}  // namespace

extern "C" int nsid_align_occurrences(const float* row_h, const int* row_j, const int* row_i0, const int* row_j0,
                                      const int64_t* row_off, const int* n_rows, const int* first_row, int npairs, int max_rows,
                                      float min_score, int top, int* occ, float* occ_score, int* n_occ, void* stream) {
  return align_occurrences_launch(row_h, row_j, row_i0, row_j0, row_off, n_rows, first_row, nullptr, false, npairs, max_rows, min_score,
                                  top, occ, occ_score, n_occ, stream);
}

extern "C" int nsid_align_occurrences_span(const float* row_h, const int* row_j, const int* row_i0, const int* row_j0,
                                           const int64_t* row_off, const int* n_rows, const int* first_row, const int* span,
                                           int npairs, int max_rows, float min_score, int top, int* occ, float* occ_score, int* n_occ,
                                           void* stream) {
  return align_occurrences_launch(row_h, row_j, row_i0, row_j0, row_off, n_rows, first_row, span, true, npairs, max_rows, min_score, top,
                                  occ, occ_score, n_occ, stream);
}

extern "C" int nsid_local_align_panels(const float* S, const int64_t* s_off, const int* s_ld, const int* q_len, const int* x_len,
                                       const int* row_base, const int* fresh, int npairs, int max_q_len, int max_x_len, int panel_cols,
                                       float theta, const int64_t* carry_off, float* carry_h, int* carry_i0, int* carry_j0,
                                       const int64_t* halo_off, float* halo_h, int* halo_i0, int* halo_j0, const int64_t* row_off,
                                       float* row_h, int* row_j, int* row_i0, int* row_j0, float* open_h, void* stream) {
  NSID_REQUIRE(panel_cols >= 2 && panel_cols <= AL_MAX_COLS);
  const int rc = align_strip_args(S, s_off, s_ld, q_len, x_len, row_base, fresh, npairs, max_q_len, max_x_len, AL_MAX_SONG_ROWS, theta,
                                  carry_off, carry_h, carry_i0, carry_j0, row_off, row_h, row_j, row_i0, row_j0, open_h);
  if (rc != NSID_OK || npairs == 0) return rc;
  NSID_REQUIRE(halo_off && halo_h && halo_i0 && halo_j0);     // every pair has the two carried rows' cells
  NSID_REQUIRE(al_aligned(halo_off, 8) && al_aligned(halo_h, 4) && al_aligned(halo_i0, 4) && al_aligned(halo_j0, 4));
  nsid_count(NSID_C_local_align_panels);
  AL_LAUNCH(local_align_panels_kernel, panel_cols, npairs, align_panels_lds_bytes(max_q_len, panel_cols),
            static_cast<hipStream_t>(stream), S, s_off, s_ld, q_len, x_len, row_base, fresh, max_q_len, max_x_len, panel_cols, theta,
            carry_off, carry_h, carry_i0, carry_j0, halo_off, halo_h, halo_i0, halo_j0, row_off, row_h, row_j, row_i0, row_j0, open_h);
}

extern "C" int nsid_align_paths(const float* S, const int64_t* s_off, const int* s_ld, const int* n_rows, const int* n_cols,
                                const int* i_base, const int* j_base, int nboxes, int max_cols, float theta, const int64_t* path_off,
                                const int64_t* dir_off, uint8_t* dirs, int* path_len, int* path_i, int* path_j, float* path_s,
                                float* end_h, void* stream) {
  NSID_REQUIRE(nboxes >= 0 && max_cols >= 0 && max_cols <= AL_PATH_MAX && theta == theta);
  if (nboxes == 0) return NSID_OK;
  NSID_REQUIRE(s_off && s_ld && n_rows && n_cols && path_off && dir_off && path_len && end_h);
  NSID_REQUIRE(max_cols == 0 || (S && dirs && path_i && path_j && path_s));
  NSID_REQUIRE(al_aligned(s_off, 8) && al_aligned(path_off, 8) && al_aligned(dir_off, 8));
  for (const void* q : {(const void*)S, (const void*)s_ld, (const void*)n_rows, (const void*)n_cols, (const void*)i_base,
                        (const void*)j_base, (const void*)path_len, (const void*)path_i, (const void*)path_j, (const void*)path_s,
                        (const void*)end_h})
    NSID_REQUIRE(al_aligned(q, 4));
  nsid_count(NSID_C_align_paths);
  AL_LAUNCH(align_paths_kernel, max_cols, nboxes, align_paths_lds_bytes(max_cols), static_cast<hipStream_t>(stream), S, s_off, s_ld,
            n_rows, n_cols, i_base, j_base, max_cols, theta, path_off, dir_off, dirs, path_len, path_i, path_j, path_s, end_h);
}
