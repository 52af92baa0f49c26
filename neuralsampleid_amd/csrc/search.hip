// Exact flat-L2 fingerprint search (include/nsid.h nsid_row_sqnorm / nsid_flat_l2_topk / nsid_seq_scores).
//
// Reference: eval.py eval_faiss with index_type='l2' (faiss.IndexFlatL2 over dummy_db ++ ref_db, then the sequence score of every
// candidate, eval.py:318-331). The ranking key of database row j for query row i is ||x_j||^2 - 2 q_i.x_j: the dot is one k-ordered
// fp32 fmaf chain on v_mfma_f32_32x32x2_f32, the same chain for every (i, j) whatever tile or lane holds it, so a query row's result is
// bitwise independent of the other rows of the call and of the split of the database. Ties in the key go to the smaller id.
//
// flat_l2_topk runs in two phases:
//  1. one wave per (32-row query tile, database split): the tile's rows sit in registers as MFMA A fragments; the split's rows are
//     read straight from HBM as B fragments (two chunks in flight). Per query row the wave keeps a sorted top-k list in LDS; its k-th
//     entry is the threshold, so almost every score is rejected by one compare. Survivors are appended to a per-row LDS queue, which
//     is merged into the list (rank by the total order (key, id, slot)) when it fills. The list goes to the workspace.
//  2. one workgroup per query row merges the splits' lists the same way and writes D = max(0, ||q||^2 + key) and int64 ids.
// Above d = 256 (the ResNet-IBN baseline's 2048-d fingerprints) phase 1 is l2_topk_wide_kernel, which stages both operands through
// LDS per K chunk; lists, queues, phase 2 and every invariant are the same.
// nsid_flat_l2_topk_excl is the same search with one range of database rows per query row that does not compete (a catalogue song
// as the query: its own rows would otherwise take every slot). Phase 1 runs its EX instantiations: an excluded (row, column) is a
// column that does not exist for that row, decided ahead of the threshold compare, so the lists hold exactly what the plain search
// holds over the database without those rows, under the same total order. The plain entry launches the EX = false instantiations.
// nsid_flat_norm_topk is the same search under another key: the cohort-normalised cell of nsid_pair_sim_norm (five fp32 operations
// on the dot, csrc/align.hip sim_norm_cell), negated, so that the largest z is the smallest key. Phase 1 runs its NM instantiations:
// the column's (x_mu, x_rs) come where ||x_j||^2 comes, the wave's 32 (q_mu, q_rs) are staged in LDS once, as the ranges are. A NaN
// key passes no compare and so never competes. Phase 2 is the same merge and writes Z = -key. The NM = false instantiations are
// what they were.
// No atomics anywhere on the ranking path.
#include "nsid_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int L2_QT = 32;            // query rows per wave (the 32x32 MFMA tile)
constexpr int L2_LIST = NSID_SEARCH_MAX_K;   // list slots per row (k <= 64)
constexpr int L2_Q1 = 32;            // survivor queue per row, phase 1 (one half-wave's candidates at most per append)
constexpr int L2_Q2 = 64;            // phase 2
constexpr int L2_UNITS = 2048;       // waves phase 1 aims at: 256 CUs x 8
constexpr int L2_MIN_SPLIT = 1024;   // database rows per split at the least
constexpr int L2_PAD_ID = 0x7fffffff;

struct KI {
  float k;
  int i;
};

__device__ __forceinline__ KI ki_pad() { return KI{__builtin_inff(), L2_PAD_ID}; }

// the total order of a merge: key, then id, then slot (slots only separate the padding entries, ids of real entries are distinct)
__device__ __forceinline__ bool ki_less(KI a, int sa, KI b, int sb) {
  return a.k < b.k || (a.k == b.k && (a.i < b.i || (a.i == b.i && sa < sb)));
}
__device__ __forceinline__ bool ki_before(KI a, KI thr) { return a.k < thr.k || (a.k == thr.k && a.i < thr.i); }

// one wave: list[0..k) <- the k smallest of list[0..k) and queue[0..cnt) (cnt <= 64). Every lane reads everything before any
// lane writes: the LDS operations of one wave complete in order.
__device__ __forceinline__ void merge_queue(KI* list, const KI* queue, int cnt, int k, int lane) {
  const KI e0 = lane < k ? list[lane] : ki_pad();
  const KI e1 = lane < cnt ? queue[lane] : ki_pad();
  int r0 = 0, r1 = 0;
  for (int f = 0; f < k; ++f) {
    const KI v = list[f];
    r0 += ki_less(v, f, e0, lane) ? 1 : 0;
    r1 += ki_less(v, f, e1, L2_LIST + lane) ? 1 : 0;
  }
  for (int f = 0; f < cnt; ++f) {
    const KI v = queue[f];
    r0 += ki_less(v, L2_LIST + f, e0, lane) ? 1 : 0;
    r1 += ki_less(v, L2_LIST + f, e1, L2_LIST + lane) ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < k && r0 < k) list[r0] = e0;
  if (lane < cnt && r1 < k) list[r1] = e1;
  __builtin_amdgcn_wave_barrier();
}

// the four vectors of the normalised key (nsid_flat_norm_topk); all null for the L2 key
struct L2Norm {
  const float *q_mu, *q_rs, *x_mu, *x_rs;
};

// the key of the normalised search: -z, z the cell of nsid_pair_sim_norm bit for bit (five fp32 operations, each rounded once, none
// contracted; the sign flip is exact). qs = (q_mu, q_rs) of the query row, (mx, rx) of the database row.
__device__ __forceinline__ float norm_key(float s, float2 qs, float mx, float rx) {
#pragma clang fp contract(off)
  const float zq = (s - qs.x) * qs.y;
  const float zx = (s - mx) * rx;
  const float sum = zq + zx;
  return -(0.5f * sum);
}

// one wave, one finished 32x32 tile: accumulator register g of lane (r, h) = (lane & 31, lane >> 5) is query row
// (g & 3) + 8 (g >> 2) + 4 h of the tile against database row `col` (cv: the row exists, xv its squared norm). Scores that pass
// their row's threshold (the k-th list entry) go to the row's queue, which is merged into the list when it would overflow.
// EX: exr[row] = the row's excluded range {lo, hi}; exh (wave-uniform): this column tile meets the hull of the tile's ranges. A
// half-wave's register g is one query row, so the range is one broadcast LDS read, and only on tiles inside the hull.
// NM: the key is norm_key; xv = x_mu[col], xr = x_rs[col], qst[row] = the row's (q_mu, q_rs), one broadcast LDS read likewise.
template <bool EX, bool NM = false>
__device__ __forceinline__ void offer_tile(KI (*list)[L2_LIST], KI (*queue)[L2_Q1], int* cnt, const f32x16& acc, int col, bool cv,
                                           float xv, int k, int lane, const int2* exr = nullptr, bool exh = false, float xr = 0.f,
                                           const float2* qst = nullptr) {
  const int h = lane >> 5;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
    KI c{0.f, col};
    if constexpr (NM) c.k = norm_key(acc[g], qst[row], xv, xr);
    else c.k = xv - (acc[g] + acc[g]);
    bool keep = cv;
    if constexpr (EX) {
      if (exh) {
        const int2 e = exr[row];
        keep = cv && !(col >= e.x && col < e.y);
      }
    }
    const bool pass = keep && ki_before(c, list[row][k - 1]);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
    if (m == 0) continue;
    const int n0 = __builtin_popcountll(m & 0xffffffffull), n1 = __builtin_popcountll(m >> 32);
    const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)) - (h ? n0 : 0);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int n = hh ? n1 : n0;
      if (n == 0) continue;
      const int rr = (g & 3) + 8 * (g >> 2) + 4 * hh;
      int c0 = __builtin_amdgcn_readfirstlane(cnt[rr]);
      if (c0 + n > L2_Q1) {
        merge_queue(list[rr], queue[rr], c0, k, lane);
        c0 = 0;
      }
      if (pass && h == hh) queue[rr][c0 + pos] = c;
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) cnt[rr] = c0 + n;
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// EX: the ranges of the wave's 32 query rows q0.. go to LDS once (a row past nq or with lo >= hi: a range no column is in); hlo / hhi
// = their hull [min lo, max hi), wave-uniform. The values are only ever compared with column ids. The caller's wave barrier follows.
constexpr int L2_EX_NONE_LO = 0x7fffffff, L2_EX_NONE_HI = (-0x7fffffff - 1);
__device__ __forceinline__ void stage_ranges(int2* exr, const int* __restrict__ exlo, const int* __restrict__ exhi, int q0, int nq,
                                             int lane, int& hlo, int& hhi) {
  int lo = L2_EX_NONE_LO, hi = L2_EX_NONE_HI;
  if (lane < L2_QT && q0 + lane < nq) {
    const int a = exlo[q0 + lane], b = exhi[q0 + lane];
    if (a < b) lo = a, hi = b;
  }
  if (lane < L2_QT) exr[lane] = int2{lo, hi};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  hlo = __builtin_amdgcn_readfirstlane(lo);
  hhi = __builtin_amdgcn_readfirstlane(hi);
}
// does the column tile [c0, c0 + 32) meet the hull?
__device__ __forceinline__ bool in_hull(int c0, int hlo, int hhi) { return c0 < hhi && (long)c0 + 31 >= (long)hlo; }

// NM: (q_mu, q_rs) of the wave's 32 query rows q0.. go to LDS once (a row past nq: zeros; its threshold lets nothing pass). The
// caller's wave barrier follows.
__device__ __forceinline__ void stage_qstats(float2* qst, const L2Norm& nm, int q0, int nq, int lane) {
  if (lane < L2_QT) qst[lane] = q0 + lane < nq ? float2{nm.q_mu[q0 + lane], nm.q_rs[q0 + lane]} : float2{0.f, 0.f};
}

// the wave's lists of query rows q0.. go to workspace slot `slot` of `nslot` per row
__device__ __forceinline__ void flush_lists(KI (*list)[L2_LIST], KI (*queue)[L2_Q1], const int* cnt, int q0, int nq, int nslot, int slot,
                                            int k, int lane, float* __restrict__ wkey, int* __restrict__ wid) {
  for (int rr = 0; rr < L2_QT; ++rr) {
    if (q0 + rr >= nq) break;
    const int c0 = __builtin_amdgcn_readfirstlane(cnt[rr]);
    if (c0 > 0) merge_queue(list[rr], queue[rr], c0, k, lane);
    if (lane < k) {
      const size_t o = ((size_t)(q0 + rr) * nslot + slot) * k + lane;
      wkey[o] = list[rr][lane].k;
      wid[o] = list[rr][lane].i;
    }
  }
}

// ---- phase 1 ----------------------------------------------------------------------------------------------------------------
// Lane (r, h) = (lane & 31, lane >> 5). MFMA step (b, e) pairs k = 8b + e (h = 0) with k = 8b + 4 + e (h = 1), so a lane reads
// 16 contiguous bytes of its row per block and the two halves read the adjacent 32 bytes. Accumulator register g of lane (r, h)
// is query row (g & 3) + 8 (g >> 2) + 4 h of the tile against database row j0 + r.
template <int D, int CH, bool EX, bool NM>
__global__ __launch_bounds__(64) void l2_topk_split_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ x,
                                                           int ldx, int nx, const float* __restrict__ xn, int k, int nqt, int S,
                                                           int chunk, float* __restrict__ wkey, int* __restrict__ wid,
                                                           const int* __restrict__ exlo, const int* __restrict__ exhi, L2Norm nm) {
  constexpr int NB = D / 8;          // 8-float blocks per row
  constexpr int NC = NB / CH;        // chunks per tile
  __shared__ KI list[L2_QT][L2_LIST];
  __shared__ KI queue[L2_QT][L2_Q1];
  __shared__ int cnt[L2_QT];
  __shared__ int2 exr[EX ? L2_QT : 1];            // never referenced, so not allocated, without EX
  __shared__ float2 qst[NM ? L2_QT : 1];          // likewise without NM

  const int lane = lane_id();
  const int r = lane & 31, h = lane >> 5;
  const int qt = blockIdx.x % nqt, s = blockIdx.x / nqt;
  const int q0 = qt * L2_QT;
  const int lo = s * chunk, hi = min(nx, lo + chunk);

  for (int t = lane; t < L2_QT * L2_LIST; t += 64) list[t / L2_LIST][t % L2_LIST] = ki_pad();
  if (lane < L2_QT) cnt[lane] = 0;
  // rows past nq get a threshold nothing passes
  if (lane < L2_QT && q0 + lane >= nq) list[lane][k - 1] = KI{-__builtin_inff(), 0};
  int hlo = 0, hhi = 0;
  if constexpr (EX) stage_ranges(exr, exlo, exhi, q0, nq, lane, hlo, hhi);
  if constexpr (NM) stage_qstats(qst, nm, q0, nq, lane);
  __builtin_amdgcn_wave_barrier();

  f32x4 a[NB];
  {
    const bool ok = q0 + r < nq;
    const float* qp = q + (size_t)(ok ? q0 + r : 0) * ldq + 4 * h;
#pragma unroll
    for (int b = 0; b < NB; ++b) a[b] = ok ? ld4(qp + 8 * b) : f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int ntile = hi > lo ? (hi - lo + 31) / 32 : 0;
  f32x4 bc[CH], bn[CH];
  auto load_chunk = [&](f32x4* dst, int tile, int c) {
    const int j = min(lo + tile * 32 + r, hi - 1);
    const float* xp = x + (size_t)j * ldx + 4 * h + 8 * CH * c;
#pragma unroll
    for (int b = 0; b < CH; ++b) dst[b] = ld4(xp + 8 * b);
  };
  if (ntile > 0) load_chunk(bc, 0, 0);

  for (int tile = 0; tile < ntile; ++tile) {
    f32x16 acc = {};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c + 1 < NC) load_chunk(bn, tile, c + 1);
      else if (tile + 1 < ntile) load_chunk(bn, tile + 1, 0);
#pragma unroll
      for (int b = 0; b < CH; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c * CH + b][e], bc[b][e], acc, 0, 0, 0);
#pragma unroll
      for (int b = 0; b < CH; ++b) bc[b] = bn[b];
    }

    const int col = lo + tile * 32 + r;
    const bool cv = col < hi;
    if constexpr (NM) {
      const float mx = cv ? nm.x_mu[col] : 0.f, rx = cv ? nm.x_rs[col] : 0.f;
      if constexpr (EX)
        offer_tile<true, true>(list, queue, cnt, acc, col, cv, mx, k, lane, exr, in_hull(lo + tile * 32, hlo, hhi), rx, qst);
      else
        offer_tile<false, true>(list, queue, cnt, acc, col, cv, mx, k, lane, nullptr, false, rx, qst);
    } else if constexpr (EX)
      offer_tile<true>(list, queue, cnt, acc, col, cv, cv ? xn[col] : 0.f, k, lane, exr, in_hull(lo + tile * 32, hlo, hhi));
    else
      offer_tile<false>(list, queue, cnt, acc, col, cv, cv ? xn[col] : 0.f, k, lane);
  }

  flush_lists(list, queue, cnt, q0, nq, S, s, k, lane, wkey, wid);
}

// ---- phase 1, wide rows (256 < d <= 2048) -------------------------------------------------------------------------------------
// A 32-row query tile no longer fits in registers (d / 8 f32x4 per lane), so a workgroup of 4 waves walks K in chunks of 32 floats
// and stages a block of query rows and a block of database rows per chunk through LDS. Wave w = (wq, wc) owns query rows
// 32 wq.. of the block and NACC column tiles of 32 database rows, one accumulator each: NACC independent MFMA chains keep the
// 64-cycle v_mfma_f32_32x32x2_f32 issuing back to back, and the accumulator of an (i, j) pair stays in one lane for the whole
// K loop. MFMA step t of chunk c pairs k = 32c + 2t (h = 0) with k = 32c + 2t + 1 (h = 1): the chain runs k = 0 .. d-1 in order
// whatever block, wave or split holds the pair.
//   WQ = 4: 128 query rows x 128 database rows, every wave 4 accumulators over the whole column block.
//   WQ = 1 (nq <= 32, nx > 128): 32 query rows x 256 database rows, every wave 2 accumulators over its own 64 columns; the four
//     waves keep separate lists, which phase 2 merges like splits (workspace slot 4 s + wc).
// Stages are k-major, [32][rows + 1] floats: the MFMA operand is one float per lane, A[i = l & 31][k = l >> 5], so a half-wave
// reads 32 consecutive floats of one k (32 banks; a row-major [row][32] stage would put them all on one). The +1 pad serves the
// transposing store: a thread holds 4 consecutive k of one row, 8 threads share a row, and with a stride = 1 mod 32 the 32 lanes of
// a half-wave (4 rows x 8 k-quads) write 32 different banks. One stage per operand, the next two chunks prefetched in registers.
// LDS: the lists, queues and counters of the narrow kernel per wave (4 x 24.1 KB) + 2 x 16.1 KB (WQ = 4) or 4.1 + 32.1 KB of stages;
// EX adds the waves' ranges behind them (4 x 256 B), NM the waves' (q_mu, q_rs) behind those (4 x 256 B).
constexpr int L2W_KC = 32;           // floats of K per stage
constexpr int L2W_UNITS = 512;       // workgroups phase 1 aims at: one per CU fits (LDS), two rounds of 256
template <int WQ>
struct L2Wide {
  static constexpr int WC = 4 / WQ, NACC = WQ == 4 ? 4 : 2;
  static constexpr int BQ = 32 * WQ, BC = 32 * WC * NACC;
  static constexpr int QS = BQ + 1, XS = BC + 1;
  static constexpr size_t lds = 4 * (sizeof(KI) * L2_QT * (L2_LIST + L2_Q1) + sizeof(int) * L2_QT) + sizeof(float) * L2W_KC * (QS + XS);
  static constexpr size_t lds_ex = lds + 4 * sizeof(int2) * L2_QT;
  static_assert(lds % alignof(int2) == 0, "the ranges follow the stages");
  static constexpr size_t bytes(bool ex, bool nm) { return (ex ? lds_ex : lds) + (nm ? 4 * sizeof(float2) * L2_QT : 0); }
};

template <int WQ, bool EX, bool NM>
__global__ __launch_bounds__(256) void l2_topk_wide_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ x,
                                                           int ldx, int nx, const float* __restrict__ xn, int d, int k, int nqb, int S,
                                                           int chunk, float* __restrict__ wkey, int* __restrict__ wid,
                                                           const int* __restrict__ exlo, const int* __restrict__ exhi, L2Norm nm) {
  using C = L2Wide<WQ>;
  constexpr int WC = C::WC, NACC = C::NACC, BQ = C::BQ, BC = C::BC, QS = C::QS, XS = C::XS;
  constexpr int QL = BQ / 32, XL = BC / 32;      // f32x4 per thread and chunk
  extern __shared__ __attribute__((aligned(16))) char l2w_smem[];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  KI(*list)[L2_LIST] = reinterpret_cast<KI(*)[L2_LIST]>(l2w_smem) + w * L2_QT;
  KI(*queue)[L2_Q1] = reinterpret_cast<KI(*)[L2_Q1]>(l2w_smem + 4 * sizeof(KI) * L2_QT * L2_LIST) + w * L2_QT;
  int* cnt = reinterpret_cast<int*>(l2w_smem + 4 * sizeof(KI) * L2_QT * (L2_LIST + L2_Q1)) + w * L2_QT;
  float* qs = reinterpret_cast<float*>(l2w_smem + 4 * (sizeof(KI) * L2_QT * (L2_LIST + L2_Q1) + sizeof(int) * L2_QT));
  float* xs = qs + L2W_KC * QS;
  [[maybe_unused]] int2* exr = reinterpret_cast<int2*>(l2w_smem + C::lds) + w * L2_QT;       // EX only: the launch sizes LDS by lds_ex
  [[maybe_unused]] float2* qst = reinterpret_cast<float2*>(l2w_smem + (EX ? C::lds_ex : C::lds)) + w * L2_QT;   // NM only, likewise

  const int r = lane & 31, h = lane >> 5;
  const int wq = w % WQ, wc = w / WQ;
  const int qb = blockIdx.x % nqb, s = blockIdx.x / nqb;
  const int q0 = qb * BQ, wq0 = q0 + 32 * wq;
  const int lo = s * chunk, hi = min(nx, lo + chunk);
  const bool active = wq0 < nq;                  // a wave whose rows all lie past nq only helps staging

  for (int t = lane; t < L2_QT * L2_LIST; t += 64) list[t / L2_LIST][t % L2_LIST] = ki_pad();
  if (lane < L2_QT) cnt[lane] = 0;
  if (lane < L2_QT && wq0 + lane >= nq) list[lane][k - 1] = KI{-__builtin_inff(), 0};
  int hlo = 0, hhi = 0;
  if constexpr (EX) stage_ranges(exr, exlo, exhi, wq0, nq, lane, hlo, hhi);
  if constexpr (NM) stage_qstats(qst, nm, wq0, nq, lane);
  __builtin_amdgcn_wave_barrier();

  const int nblk = hi > lo ? (hi - lo + BC - 1) / BC : 0;
  const int nkc = d / L2W_KC;                    // even: d % 64 == 0
  const int ng = nblk * nkc;                     // chunks in all; two are in flight in registers (g0 / g1: even / odd chunks)
  const int kq = tid & 7, rb = tid >> 3;         // the thread's k-quad of the chunk and its row (+ 32 i) of the block
  f32x4 gq0[QL], gx0[XL], gq1[QL], gx1[XL];
  int lblk = 0, lc = 0;                          // the next chunk to load
  auto gload = [&](f32x4* gq, f32x4* gx) {
    const int ko = L2W_KC * lc + 4 * kq;
#pragma unroll
    for (int i = 0; i < QL; ++i)                 // rows past nq: any valid row, their scores meet a threshold nothing passes
      gq[i] = ld4(q + (size_t)min(q0 + rb + 32 * i, nq - 1) * ldq + ko);
#pragma unroll
    for (int i = 0; i < XL; ++i) gx[i] = ld4(x + (size_t)min(lo + lblk * BC + rb + 32 * i, hi - 1) * ldx + ko);
    if (++lc == nkc) {
      lc = 0;
      ++lblk;
    }
  };
  auto stage = [&](const f32x4* gq, const f32x4* gx) {
    __syncthreads();                             // every wave has read the previous chunk
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int i = 0; i < QL; ++i) qs[(4 * kq + e) * QS + rb + 32 * i] = gq[i][e];
#pragma unroll
      for (int i = 0; i < XL; ++i) xs[(4 * kq + e) * XS + rb + 32 * i] = gx[i][e];
    }
    __syncthreads();
  };

  f32x16 acc[NACC];
#pragma unroll
  for (int n = 0; n < NACC; ++n) acc[n] = f32x16{};
  const float* ap = qs + h * QS + 32 * wq + r;
  const float* bp = xs + h * XS + 32 * NACC * wc + r;
  // one staged chunk: 16 MFMA steps; the operands of step t + AHEAD are read from LDS before the MFMAs of step t issue, and the
  // fences keep the compiler from gathering the reads in front of the chunk (registers) or behind their use (LDS latency exposed).
  // The first AHEAD steps are read (first_reads) before the next chunk's global loads are issued, the rest inside run_chunk.
  constexpr int NT = L2W_KC / 2, AHEAD = 4;
  float a[2 * AHEAD], b[2 * AHEAD][NACC];
  auto rd = [&](int t) {
    a[t % (2 * AHEAD)] = ap[2 * t * QS];
#pragma unroll
    for (int n = 0; n < NACC; ++n) b[t % (2 * AHEAD)][n] = bp[2 * t * XS + 32 * n];
  };
  auto first_reads = [&]() {
#pragma unroll
    for (int t = 0; t < AHEAD; ++t) rd(t);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto run_chunk = [&]() {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t + AHEAD < NT) rd(t + AHEAD);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int n = 0; n < NACC; ++n)
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t % (2 * AHEAD)], b[t % (2 * AHEAD)][n], acc[n], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  if (ng > 0) {
    gload(gq0, gx0);
    gload(gq1, gx1);
  }
  for (int g = 0; g < ng; g += 2) {
    stage(gq0, gx0);
    if (active) first_reads();
    if (g + 2 < ng) gload(gq0, gx0);
    if (active) run_chunk();
    stage(gq1, gx1);
    if (active) first_reads();
    if (g + 3 < ng) gload(gq1, gx1);
    if (active) run_chunk();
    if ((g + 2) % nkc != 0) continue;
    const int blk = g / nkc;                     // the block's last chunk: its tiles meet the lists
    if (active) {
      auto offer_n = [&](const f32x16& tile, int n) {
        const int col = lo + blk * BC + 32 * (NACC * wc + n) + r;
        const bool cv = col < hi;
        if constexpr (NM) {
          const float mx = cv ? nm.x_mu[col] : 0.f, rx = cv ? nm.x_rs[col] : 0.f;
          if constexpr (EX)
            offer_tile<true, true>(list, queue, cnt, tile, col, cv, mx, k, lane, exr, in_hull(__builtin_amdgcn_readfirstlane(col - r), hlo, hhi), rx, qst);
          else
            offer_tile<false, true>(list, queue, cnt, tile, col, cv, mx, k, lane, nullptr, false, rx, qst);
        } else if constexpr (EX)
          offer_tile<true>(list, queue, cnt, tile, col, cv, cv ? xn[col] : 0.f, k, lane, exr, in_hull(__builtin_amdgcn_readfirstlane(col - r), hlo, hhi));
        else
          offer_tile<false>(list, queue, cnt, tile, col, cv, cv ? xn[col] : 0.f, k, lane);
      };
      offer_n(acc[0], 0);                        // spelled out: a loop the compiler declines to unroll would index acc through scratch
      offer_n(acc[1], 1);
      if constexpr (NACC == 4) {
        offer_n(acc[2], 2);
        offer_n(acc[3], 3);
      }
    }
#pragma unroll
    for (int n = 0; n < NACC; ++n) acc[n] = f32x16{};
  }

  if (active) flush_lists(list, queue, cnt, wq0, nq, S * WC, s * WC + wc, k, lane, wkey, wid);
}

// ---- phase 2: one workgroup of 4 waves per query row ---------------------------------------------------------------------------
__device__ __forceinline__ void offer(KI* list, KI* queue, int& cnt, int k, int lane, KI c, bool valid) {
  const bool pass = valid && ki_before(c, list[k - 1]);
  const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
  if (m == 0) return;
  const int n = __builtin_popcountll(m);
  if (cnt + n > L2_Q2) {
    merge_queue(list, queue, cnt, k, lane);
    cnt = 0;
  }
  const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  if (pass) queue[cnt + pos] = c;
  cnt += n;
  __builtin_amdgcn_wave_barrier();
}

// what phase 2 writes. L2_OUT_DIST: D = max(0, ||q||^2 + key), pads I = -1, D = +inf. L2_OUT_RAW (the pre-filter's coarse lists,
// IdT = int): D / I get the merged keys and ids as they are, pads included; qn is not read. L2_OUT_NEG (the normalised search):
// D = -key, the score itself, pads I = -1, D = -inf; qn is not read.
enum { L2_OUT_DIST = 0, L2_OUT_RAW = 1, L2_OUT_NEG = 2 };
template <typename IdT, int OUT>
__global__ __launch_bounds__(256) void l2_topk_merge_kernel(const float* __restrict__ wkey, const int* __restrict__ wid, int S, int k,
                                                            const float* __restrict__ qn, float* __restrict__ D, IdT* __restrict__ I) {
  __shared__ KI list[4][L2_LIST];
  __shared__ KI queue[4][L2_Q2];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int row = blockIdx.x;
  for (int t = lane; t < L2_LIST; t += 64) list[w][t] = ki_pad();
  __builtin_amdgcn_wave_barrier();

  const long total = (long)S * k;
  const long lo = total * w / 4, hi = total * (w + 1) / 4;
  const float* kp = wkey + (size_t)row * total;
  const int* ip = wid + (size_t)row * total;
  int cnt = 0;
  long i = lo + lane;
  KI nxt = i < hi ? KI{kp[i], ip[i]} : ki_pad();
  for (long base = lo; base < hi; base += 64) {
    const KI cur = nxt;
    const bool v = base + lane < hi;
    i = base + 64 + lane;
    nxt = i < hi ? KI{kp[i], ip[i]} : ki_pad();
    offer(list[w], queue[w], cnt, k, lane, cur, v);
  }
  if (cnt > 0) merge_queue(list[w], queue[w], cnt, k, lane);
  __syncthreads();
  if (w != 0) return;
  cnt = 0;
  for (int o = 1; o < 4; ++o) offer(list[0], queue[0], cnt, k, lane, lane < k ? list[o][lane] : ki_pad(), lane < k);
  if (cnt > 0) merge_queue(list[0], queue[0], cnt, k, lane);
  if (lane < k) {
    const KI e = list[0][lane];
    if constexpr (OUT == L2_OUT_RAW) {
      D[(size_t)row * k + lane] = e.k;
      I[(size_t)row * k + lane] = e.i;
    } else if constexpr (OUT == L2_OUT_NEG) {
      const bool real = e.i != L2_PAD_ID;
      D[(size_t)row * k + lane] = real ? -e.k : -__builtin_inff();
      I[(size_t)row * k + lane] = real ? (int64_t)e.i : (int64_t)-1;
    } else {
      const bool real = e.i != L2_PAD_ID;
      D[(size_t)row * k + lane] = real ? fmaxf(0.f, qn[row] + e.k) : __builtin_inff();
      I[(size_t)row * k + lane] = real ? (int64_t)e.i : (int64_t)-1;
    }
  }
}

// ---- squared norms: 16 lanes per row, lane partials over float4 chunks in order, then a fixed butterfly ------------------------
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ x, int ldx, int n, int d, float* __restrict__ out) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  float acc = 0.f;
  if (row < n) {
    const float* p = x + (size_t)row * ldx;
    for (int c = l; c < d / 4; c += 16) {
      const f32x4 v = ld4(p + 4 * c);
      acc = fmaf(v[0], v[0], acc);
      acc = fmaf(v[1], v[1], acc);
      acc = fmaf(v[2], v[2], acc);
      acc = fmaf(v[3], v[3], acc);
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
  if (row < n && l == 0) out[row] = acc;
}

// ---- sequence scores: one wave per (pair, candidate) -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seq_scores_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ x, int ldx,
                                                         int nx, int d, const int64_t* __restrict__ I, int k,
                                                         const int* __restrict__ starts, const int* __restrict__ lens,
                                                         float* __restrict__ out, int ldo) {
  const int p = blockIdx.x;
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int s = starts[p], L = lens[p];
  if (j >= ldo) return;
  if (j >= L * k) {
    if (lane == 0) out[(size_t)p * ldo + j] = __builtin_nanf("");
    return;
  }
  const int64_t cid = I[(size_t)(s + j / k) * k + j % k];
  float v = __builtin_nanf("");
  if (cid >= 0 && cid < nx) {
    const int n = min((int64_t)L, (int64_t)nx - cid);
    float acc = 0.f;
    for (int i = 0; i < n; ++i) {
      const float* qp = q + (size_t)(s + i) * ldq;
      const float* xp = x + (size_t)(cid + i) * ldx;
      for (int c = lane; c < d; c += 64) acc = fmaf(qp[c], xp[c], acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    v = acc / (float)n;
  }
  if (lane == 0) out[(size_t)p * ldo + j] = v;
}

bool l2_wide(int d) { return d > 256; }
bool l2_shape_ok(int d) { return (d % 16 == 0 && d >= 16 && d <= 256) || (d % 64 == 0 && l2_wide(d) && d <= 2048); }

template <int D, bool EX, bool NM>
int launch_split(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* xn, int k, int nqt, int S, int chunk,
                 float* wkey, int* wid, const int* exlo, const int* exhi, const L2Norm& nm, hipStream_t st) {
  constexpr int NB = D / 8;
  constexpr int CH = (D <= 128 && NB % 8 == 0) ? 8 : (NB % 4 == 0 ? 4 : 2);
  NSID_LAUNCH((l2_topk_split_kernel<D, CH, EX, NM>), dim3(nqt * S), dim3(64), 0, st, q, ldq, nq, x, ldx, nx, xn, k, nqt, S, chunk, wkey,
              wid, exlo, exhi, nm);
  return nsid_launch_status();
}

template <bool EX, bool NM, int... Ds>
int dispatch_split(int d, const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* xn, int k, int nqt, int S,
                   int chunk, float* wkey, int* wid, const int* exlo, const int* exhi, const L2Norm& nm, hipStream_t st) {
  int rc = NSID_EINVAL;
  ((d == Ds ? (rc = launch_split<Ds, EX, NM>(q, ldq, nq, x, ldx, nx, xn, k, nqt, S, chunk, wkey, wid, exlo, exhi, nm, st), 0) : 0), ...);
  return rc;
}

// split plan of the wide phase 1: query blocks of 128 rows (32 in the WQ = 1 form), splits of whole column blocks;
// *slots = lists per query row in the workspace
// the 32 x 256 form spreads the database over the four waves' columns; up to one 128-row column block there is nothing to spread
bool l2_wide_one(long nq, long nx) { return nq <= L2_QT && nx > L2Wide<4>::BC; }

void l2_plan_wide(long nq, long nx, int* splits, int* chunk, int* slots) {
  const bool one = l2_wide_one(nq, nx);
  const long bq = one ? L2Wide<1>::BQ : L2Wide<4>::BQ, bc = one ? L2Wide<1>::BC : L2Wide<4>::BC;
  const long nqb = (nq + bq - 1) / bq;
  long S = nqb > 0 ? (L2W_UNITS + nqb - 1) / nqb : 1;
  S = std::min(S, std::max(1L, nx / L2_MIN_SPLIT));
  long c = (nx + S - 1) / S;
  c = (c + bc - 1) / bc * bc;
  if (c == 0) c = bc;
  S = std::max(1L, (nx + c - 1) / c);
  *splits = (int)S;
  *chunk = (int)c;
  *slots = (int)(S * (one ? L2Wide<1>::WC : L2Wide<4>::WC));
}

template <int WQ, bool EX, bool NM>
int launch_wide(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* xn, int d, int k, int S, int chunk,
                float* wkey, int* wid, const int* exlo, const int* exhi, const L2Norm& nm, hipStream_t st) {
  const int nqb = (nq + L2Wide<WQ>::BQ - 1) / L2Wide<WQ>::BQ;
  NSID_LAUNCH_LDS((l2_topk_wide_kernel<WQ, EX, NM>), dim3(nqb * S), dim3(256), L2Wide<WQ>::bytes(EX, NM), st, q, ldq, nq, x, ldx, nx, xn,
                  d, k, nqb, S, chunk, wkey, wid, exlo, exhi, nm);
  return nsid_launch_status();
}

}  // namespace

// split plan of phase 1: enough waves for 256 CUs x 8, splits of at least L2_MIN_SPLIT rows, each a multiple of 32 rows
void nsid_l2_plan(long nq, long nx, int* splits, int* chunk) {
  const long nqt = (nq + L2_QT - 1) / L2_QT;
  long S = nqt > 0 ? (L2_UNITS + nqt - 1) / nqt : 1;
  S = std::min(S, std::max(1L, nx / L2_MIN_SPLIT));
  long c = (nx + S - 1) / S;
  c = (c + 31) / 32 * 32;
  if (c == 0) c = 32;
  S = std::max(1L, (nx + c - 1) / c);
  *splits = (int)S;
  *chunk = (int)c;
}

// enough for either plan: the caller of nsid_workspace_bytes does not say d
long nsid_l2_ws_bytes(long nq, long nx, int k) {
  int S, c, Sw, slots;
  nsid_l2_plan(nq, nx, &S, &c);
  l2_plan_wide(nq, nx, &Sw, &c, &slots);
  return (long)std::max(S, slots) * nq * k * (long)(sizeof(float) + sizeof(int));
}

extern "C" int nsid_row_sqnorm(const float* x, int ldx, int n, int d, float* out, void* stream) {
  NSID_REQUIRE(n >= 0 && l2_shape_ok(d));
  if (n == 0) return NSID_OK;
  NSID_REQUIRE(x && out && ldx >= d && ldx % 4 == 0 && nsid_aligned16(x));
  nsid_count(NSID_C_row_sqnorm);
  NSID_LAUNCH(row_sqnorm_kernel, dim3((n + 15) / 16), dim3(256), 0, static_cast<hipStream_t>(stream), x, ldx, n, d, out);
  return nsid_launch_status();
}

namespace {
bool l2_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// the body of the search entries; EX: with the per-row ranges exlo / exhi; NM: the normalised key of nm (x_sqnorm, q_sqnorm unused)
template <bool EX, bool NM>
int l2_topk_entry(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* x_sqnorm, const float* q_sqnorm,
                  const int* exlo, const int* exhi, const L2Norm& nm, int d, int k, float* D, int64_t* I, void* ws, size_t ws_bytes,
                  void* stream) {
  NSID_REQUIRE(nq >= 0 && nx >= 0 && l2_shape_ok(d) && k >= 1 && k <= L2_LIST);
  if (nq == 0) return NSID_OK;
  NSID_REQUIRE(q && D && I && ws && ldq >= d && ldq % 4 == 0 && nsid_aligned16(q) && nsid_aligned16(ws));
  NSID_REQUIRE(nx == 0 || (x && ldx >= d && ldx % 4 == 0 && nsid_aligned16(x)));
  if constexpr (NM) {
    NSID_REQUIRE(nm.q_mu && nm.q_rs && l2_aligned4(nm.q_mu) && l2_aligned4(nm.q_rs));
    NSID_REQUIRE(nx == 0 || (nm.x_mu && nm.x_rs && l2_aligned4(nm.x_mu) && l2_aligned4(nm.x_rs)));
  } else {
    NSID_REQUIRE(q_sqnorm && (nx == 0 || x_sqnorm));
  }
  NSID_REQUIRE(!EX || (exlo && exhi));
  int S, chunk, slots;
  if (l2_wide(d)) {
    l2_plan_wide(nq, nx, &S, &chunk, &slots);
  } else {
    nsid_l2_plan(nq, nx, &S, &chunk);
    slots = S;
  }
  const size_t per = (size_t)slots * nq * k;
  NSID_REQUIRE(ws_bytes >= per * (sizeof(float) + sizeof(int)));
  float* wkey = static_cast<float*>(ws);
  int* wid = reinterpret_cast<int*>(wkey + per);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nqt = (nq + L2_QT - 1) / L2_QT;
  nsid_count(NM ? NSID_C_flat_norm_topk : EX ? NSID_C_flat_l2_topk_excl : NSID_C_flat_l2_topk);
  int rc;
  if (l2_wide(d)) {
    nsid_count(NM ? NSID_C_flat_norm_topk_wide : EX ? NSID_C_flat_l2_topk_wide_excl : NSID_C_flat_l2_topk_wide);
    const bool one = l2_wide_one(nq, nx);
    if constexpr (NM)
      nsid_took(one ? (EX ? "l2_topk_wide_kernel<1,excl,norm>" : "l2_topk_wide_kernel<1,norm>")
                    : (EX ? "l2_topk_wide_kernel<4,excl,norm>" : "l2_topk_wide_kernel<4,norm>"));
    rc = one ? launch_wide<1, EX, NM>(q, ldq, nq, x, ldx, nx, x_sqnorm, d, k, S, chunk, wkey, wid, exlo, exhi, nm, st)
             : launch_wide<4, EX, NM>(q, ldq, nq, x, ldx, nx, x_sqnorm, d, k, S, chunk, wkey, wid, exlo, exhi, nm, st);
  } else {
    if constexpr (NM) nsid_took(EX ? "l2_topk_split_kernel<excl,norm>" : "l2_topk_split_kernel<norm>");
    rc = dispatch_split<EX, NM, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256>(
        d, q, ldq, nq, x, ldx, nx, x_sqnorm, k, nqt, S, chunk, wkey, wid, exlo, exhi, nm, st);
  }
  if (rc != NSID_OK) return rc;
  NSID_LAUNCH((l2_topk_merge_kernel<int64_t, NM ? L2_OUT_NEG : L2_OUT_DIST>), dim3(nq), dim3(256), 0, st, wkey, wid, slots, k, q_sqnorm, D, I);
  return nsid_launch_status();
}
}  // namespace

extern "C" int nsid_flat_l2_topk(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* x_sqnorm,
                                 const float* q_sqnorm, int d, int k, float* D, int64_t* I, void* ws, size_t ws_bytes, void* stream) {
  return l2_topk_entry<false, false>(q, ldq, nq, x, ldx, nx, x_sqnorm, q_sqnorm, nullptr, nullptr, L2Norm{}, d, k, D, I, ws, ws_bytes,
                                     stream);
}

extern "C" int nsid_flat_l2_topk_excl(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* x_sqnorm,
                                      const float* q_sqnorm, const int* ex_lo, const int* ex_hi, int d, int k, float* D, int64_t* I,
                                      void* ws, size_t ws_bytes, void* stream) {
  return l2_topk_entry<true, false>(q, ldq, nq, x, ldx, nx, x_sqnorm, q_sqnorm, ex_lo, ex_hi, L2Norm{}, d, k, D, I, ws, ws_bytes, stream);
}

extern "C" int nsid_flat_norm_topk(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* q_mu, const float* q_rs,
                                   const float* x_mu, const float* x_rs, const int* ex_lo, const int* ex_hi, int d, int k, float* Z,
                                   int64_t* I, void* ws, size_t ws_bytes, void* stream) {
  NSID_REQUIRE((ex_lo == nullptr) == (ex_hi == nullptr));
  const L2Norm nm{q_mu, q_rs, x_mu, x_rs};
  if (ex_lo) return l2_topk_entry<true, true>(q, ldq, nq, x, ldx, nx, nullptr, nullptr, ex_lo, ex_hi, nm, d, k, Z, I, ws, ws_bytes, stream);
  return l2_topk_entry<false, true>(q, ldq, nq, x, ldx, nx, nullptr, nullptr, nullptr, nullptr, nm, d, k, Z, I, ws, ws_bytes, stream);
}

extern "C" int nsid_seq_scores(const float* q, int ldq, const float* x, int ldx, int nx, int d, const int64_t* I, int k,
                               const int* starts, const int* lens, int npairs, float* out, int ldo, void* stream) {
  NSID_REQUIRE(npairs >= 0 && nx >= 0 && l2_shape_ok(d) && k >= 1 && k <= L2_LIST && ldo >= 0 && ldo <= 4 * 65535);
  if (npairs == 0 || ldo == 0) return NSID_OK;
  NSID_REQUIRE(q && x && I && starts && lens && out && ldq >= d && ldx >= d);
  nsid_count(NSID_C_seq_scores);
  NSID_LAUNCH(seq_scores_kernel, dim3(npairs, (ldo + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), q, ldq, x, ldx, nx, d,
              I, k, starts, lens, out, ldo);
  return nsid_launch_status();
}

// ---- the certified bf16 pre-filter (include/nsid.h nsid_bf16_rows / nsid_flat_l2_topk_coarse / nsid_flat_l2_rescore; the rule and
// the derivation of its error bound: DESIGN.md section 7) ---------------------------------------------------------------------------
// A bf16 pass proposes L2_LIST candidates per query row under the coarse key ||x_j||^2 - 2 dot_bf16(q~, x~_j); the candidates are
// re-scored with the exact chain of l2_topk_split_kernel, and a row is certified when no database row outside the candidates can have
// an exact key among its k smallest. The bf16 data never reaches a result: (D, I) of a certified row are the plain search's bits, and
// an uncertified row is the caller's to search with the plain entry.
namespace {

// a non-negative double as a float that is not below it (NaN stays NaN); below the normal range: the smallest normal float
__device__ __forceinline__ float f32_up(double v) {
  float f = (float)v;
  if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);
  if (v > 0.0 && f < 0x1p-126f) f = 0x1p-126f;
  return f;
}

// 16 lanes per row: RNE bf16 image, ||x - x~|| and max(||x||, ||x~||) from fp64 sums (every term exact in fp64), rounded upwards
__global__ __launch_bounds__(256) void bf16_rows_kernel(const float* __restrict__ x, int ldx, int n, int d, __bf16* __restrict__ xb,
                                                        int ldb, float* __restrict__ err, float* __restrict__ nrm) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  double se = 0.0, sx = 0.0, sb = 0.0;
  if (row < n) {
    const float* p = x + (size_t)row * ldx;
    __bf16* o = xb + (size_t)row * ldb;
    for (int c = l; c < d / 8; c += 16) {
      const f32x4 v0 = ld4(p + 8 * c), v1 = ld4(p + 8 * c + 4);
      bf16x8 w;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = e < 4 ? v0[e & 3] : v1[e & 3];
        w[e] = (__bf16)v;                                  // RNE (v_cvt_pk_bf16_f32)
        const double t = (double)v, u = (double)(float)w[e], dlt = t - u;
        se += dlt * dlt;
        sx += t * t;
        sb += u * u;
      }
      *reinterpret_cast<bf16x8*>(o + 8 * c) = w;
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    se += __shfl_xor(se, o, 16);
    sx += __shfl_xor(sx, o, 16);
    sb += __shfl_xor(sb, o, 16);
  }
  if (row < n && l == 0) {
    double m = sx >= sb ? sx : sb;
    if (sx != sx) m = sx;                                  // NaN in, NaN out
    err[row] = f32_up(sqrt(se) * (1.0 + 0x1p-40));         // the factor covers the fp64 roundings of the sums and of the root
    nrm[row] = f32_up(sqrt(m) * (1.0 + 0x1p-40));
  }
}

// ---- coarse phase 1: a workgroup of 4 waves owns 128 query rows (wave w rows 32 w.., as bf16 A fragments in registers) and walks
// its database split in blocks of 64 rows staged through LDS, so a staged block serves four waves. Lane (r, h) holds
// A[row r][k = 16 s + 8 h + j] of k-step s in element j; the B fragment of database row r is the 16 bytes at 32 s + 16 h of its staged
// row. Staged rows are 2 D + 16 bytes apart: 16 lanes then read 16 different 16-byte bank groups. The next block travels in
// registers while this one is multiplied. Lists, queues and counters per wave as in l2_topk_split_kernel, at k = L2_LIST.
constexpr int L2C_BQ = 128;          // query rows per workgroup
constexpr int L2C_BC = 64;           // database rows per stage
constexpr int L2C_UNITS = 256;       // workgroups aimed at: LDS holds one per CU
template <int D>
struct L2Coarse {
  static constexpr int STR = 2 * D + 16;
  static constexpr size_t wave = sizeof(KI) * L2_QT * (L2_LIST + L2_Q1) + sizeof(int) * L2_QT;
  static constexpr size_t lds = 4 * wave + (size_t)L2C_BC * STR;
  static constexpr size_t lds_ex = lds + 4 * sizeof(int2) * L2_QT;
  static_assert((4 * wave) % 16 == 0 && lds % alignof(int2) == 0, "the stage is read in 16-byte chunks; the ranges follow it");
};

// offer_tile with the rows' thresholds (the L2_LIST-th list entries) in registers: tk / ti [g] belong to accumulator register g of
// this lane. A tile none of whose 16 x 64 scores reaches its row's threshold key costs the compares and one ballot. Otherwise the
// scores are compared on the exact order (key, id), the queues the tile would overflow are merged (which refreshes those rows'
// thresholds), and the per-register append of offer_tile runs.
template <bool EX>
__device__ __forceinline__ void offer_tile_thr(KI (*list)[L2_LIST], KI (*queue)[L2_Q1], int* cnt, float (&tk)[16], int (&ti)[16],
                                               const f32x16& acc, int col, bool cv, float xv, int lane, const int2* exr, bool exh) {
  constexpr int k = L2_LIST;
  const int h = lane >> 5;
  bool any = false;
#pragma unroll
  for (int g = 0; g < 16; ++g) any |= (xv - (acc[g] + acc[g])) <= tk[g];
  if (__builtin_amdgcn_ballot_w64(cv && any) == 0) return;
  // the exact compares: m[g] = the lanes whose score of register g goes to its row's queue
  unsigned long long m[16], anym = 0;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
    const KI c{xv - (acc[g] + acc[g]), col};
    bool keep = cv;
    if constexpr (EX) {
      if (exh) {
        const int2 e = exr[row];
        keep = cv && !(col >= e.x && col < e.y);
      }
    }
    m[g] = __builtin_amdgcn_ballot_w64(keep && ki_before(c, KI{tk[g], ti[g]}));
    anym |= m[g];
  }
  if (anym == 0) return;
  // lane l < 32 looks after row l (register gs of half hs): a queue this tile would overflow is merged first, one merge_queue in
  // the code instead of one per register and half; its row's threshold is refreshed in the registers that hold the row
  {
    const int gs = (lane & 3) + 4 * ((lane & 31) >> 3), hs = (lane >> 2) & 1;
    int mine = 0;
#pragma unroll
    for (int g = 0; g < 16; ++g)
      if (g == gs) mine = __builtin_popcount(hs ? (unsigned)(m[g] >> 32) : (unsigned)m[g]);
    const int have = lane < L2_QT ? cnt[lane] : 0;
    unsigned long long need = __builtin_amdgcn_ballot_w64(lane < L2_QT && mine > 0 && have + mine > L2_Q1);
    while (need) {
      const int rr = __builtin_ctzll(need);
      need &= need - 1;
      merge_queue(list[rr], queue[rr], __builtin_amdgcn_readfirstlane(cnt[rr]), k, lane);
      if (lane == 0) cnt[rr] = 0;
      __builtin_amdgcn_wave_barrier();
      const KI t = list[rr][k - 1];
#pragma unroll
      for (int g = 0; g < 16; ++g)
        if ((g & 3) + 8 * (g >> 2) + 4 * h == rr) tk[g] = t.k, ti[g] = t.i;
    }
  }
  // the per-register append of offer_tile; every queue now has room
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    if (m[g] == 0) continue;
    const bool pass = (m[g] >> lane) & 1;
    const KI c{xv - (acc[g] + acc[g]), col};
    const int n0 = __builtin_popcountll(m[g] & 0xffffffffull), n1 = __builtin_popcountll(m[g] >> 32);
    const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m[g] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m[g], 0u)) - (h ? n0 : 0);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int n = hh ? n1 : n0;
      if (n == 0) continue;
      const int rr = (g & 3) + 8 * (g >> 2) + 4 * hh;
      const int c0 = __builtin_amdgcn_readfirstlane(cnt[rr]);
      if (pass && h == hh) queue[rr][c0 + pos] = c;
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) cnt[rr] = c0 + n;
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <int D, bool EX>
__global__ __launch_bounds__(256) void l2_coarse_kernel(const __bf16* __restrict__ q, int ldq, int nq, const __bf16* __restrict__ x,
                                                        int ldx, int nx, const float* __restrict__ xn, int nqb, int S, int chunk,
                                                        float* __restrict__ wkey, int* __restrict__ wid,
                                                        const int* __restrict__ exlo, const int* __restrict__ exhi) {
  using C = L2Coarse<D>;
  constexpr int NS = D / 16, STR = C::STR, RC = D / 8, NCH = L2C_BC * RC, PT = (NCH + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char l2c_smem[];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  KI(*list)[L2_LIST] = reinterpret_cast<KI(*)[L2_LIST]>(l2c_smem) + w * L2_QT;
  KI(*queue)[L2_Q1] = reinterpret_cast<KI(*)[L2_Q1]>(l2c_smem + 4 * sizeof(KI) * L2_QT * L2_LIST) + w * L2_QT;
  int* cnt = reinterpret_cast<int*>(l2c_smem + 4 * sizeof(KI) * L2_QT * (L2_LIST + L2_Q1)) + w * L2_QT;
  char* stage = l2c_smem + 4 * C::wave;
  [[maybe_unused]] int2* exr = reinterpret_cast<int2*>(l2c_smem + C::lds) + w * L2_QT;       // EX only: the launch sizes LDS by lds_ex

  const int r = lane & 31, h = lane >> 5;
  const int qb = blockIdx.x % nqb, s = blockIdx.x / nqb;
  const int wq0 = qb * L2C_BQ + 32 * w;
  const int lo = s * chunk, hi = min(nx, lo + chunk);
  const bool active = wq0 < nq;                  // a wave whose rows all lie past nq only helps staging

  for (int t = lane; t < L2_QT * L2_LIST; t += 64) list[t / L2_LIST][t % L2_LIST] = ki_pad();
  if (lane < L2_QT) cnt[lane] = 0;
  if (lane < L2_QT && wq0 + lane >= nq) list[lane][L2_LIST - 1] = KI{-__builtin_inff(), 0};   // a threshold nothing passes
  int hlo = 0, hhi = 0;
  if constexpr (EX) stage_ranges(exr, exlo, exhi, wq0, nq, lane, hlo, hhi);
  __builtin_amdgcn_wave_barrier();

  float tk[16];
  int ti[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const bool ok = wq0 + (g & 3) + 8 * (g >> 2) + 4 * h < nq;
    tk[g] = ok ? __builtin_inff() : -__builtin_inff();
    ti[g] = ok ? L2_PAD_ID : 0;
  }

  bf16x8 a[NS];
  {
    const bool ok = wq0 + r < nq;
    const __bf16* qp = q + (size_t)(ok ? wq0 + r : 0) * ldq + 8 * h;
#pragma unroll
    for (int i = 0; i < NS; ++i) a[i] = ok ? *reinterpret_cast<const bf16x8*>(qp + 16 * i) : bf16x8{};
  }

  const int nblk = hi > lo ? (hi - lo + L2C_BC - 1) / L2C_BC : 0;
  u32x4 gx[PT];
  float xv0 = 0.f, xv1 = 0.f, nv0 = 0.f, nv1 = 0.f;     // the squared norms of this lane's two columns: this block's, the next one's
  auto gload = [&](int blk) {
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int idx = tid + 256 * i;
      if (NCH % 256 == 0 || idx < NCH) {
        const int j = min(lo + blk * L2C_BC + idx / RC, hi - 1);
        gx[i] = *reinterpret_cast<const u32x4*>(x + (size_t)j * ldx + 8 * (idx % RC));
      }
    }
    const int c = lo + blk * L2C_BC + r;
    nv0 = c < hi ? xn[c] : 0.f;
    nv1 = c + 32 < hi ? xn[c + 32] : 0.f;
  };
  if (nblk > 0) gload(0);

  const char* bp = stage + r * STR + 16 * h;
  for (int blk = 0; blk < nblk; ++blk) {
    __syncthreads();                             // every wave has read the previous block
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int idx = tid + 256 * i;
      if (NCH % 256 == 0 || idx < NCH) *reinterpret_cast<u32x4*>(stage + (idx / RC) * STR + 16 * (idx % RC)) = gx[i];
    }
    xv0 = nv0, xv1 = nv1;
    __syncthreads();
    if (blk + 1 < nblk) gload(blk + 1);
    if (!active) continue;
    f32x16 acc0 = {}, acc1 = {};
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(bp + 32 * i);
      const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(bp + 32 * STR + 32 * i);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b1, acc1, 0, 0, 0);
    }
    const int c0 = lo + blk * L2C_BC;            // uniform
    const int col = c0 + r;
    offer_tile_thr<EX>(list, queue, cnt, tk, ti, acc0, col, col < hi, xv0, lane, exr, EX && in_hull(c0, hlo, hhi));
    offer_tile_thr<EX>(list, queue, cnt, tk, ti, acc1, col + 32, col + 32 < hi, xv1, lane, exr, EX && in_hull(c0 + 32, hlo, hhi));
  }

  if (active) flush_lists(list, queue, cnt, wq0, nq, S, s, L2_LIST, lane, wkey, wid);
}

void l2_plan_coarse(long nq, long nx, int* splits, int* chunk) {
  const long nqb = (nq + L2C_BQ - 1) / L2C_BQ;
  long S = nqb > 0 ? (L2C_UNITS + nqb - 1) / nqb : 1;
  S = std::min(S, std::max(1L, nx / L2_MIN_SPLIT));
  long c = (nx + S - 1) / S;
  c = (c + L2C_BC - 1) / L2C_BC * L2C_BC;
  if (c == 0) c = L2C_BC;
  S = std::max(1L, (nx + c - 1) / c);
  *splits = (int)S;
  *chunk = (int)c;
}

template <int D, bool EX>
int launch_coarse(const __bf16* q, int ldq, int nq, const __bf16* x, int ldx, int nx, const float* xn, int S, int chunk, float* wkey,
                  int* wid, const int* exlo, const int* exhi, hipStream_t st) {
  const int nqb = (nq + L2C_BQ - 1) / L2C_BQ;
  NSID_LAUNCH_LDS((l2_coarse_kernel<D, EX>), dim3(nqb * S), dim3(256), EX ? L2Coarse<D>::lds_ex : L2Coarse<D>::lds, st, q, ldq, nq, x,
                  ldx, nx, xn, nqb, S, chunk, wkey, wid, exlo, exhi);
  return nsid_launch_status();
}

template <bool EX, int... Ds>
int dispatch_coarse(int d, const __bf16* q, int ldq, int nq, const __bf16* x, int ldx, int nx, const float* xn, int S, int chunk,
                    float* wkey, int* wid, const int* exlo, const int* exhi, hipStream_t st) {
  int rc = NSID_EINVAL;
  ((d == Ds ? (rc = launch_coarse<Ds, EX>(q, ldq, nq, x, ldx, nx, xn, S, chunk, wkey, wid, exlo, exhi, st), 0) : 0), ...);
  return rc;
}

// ---- re-score: one wave per query row. The row is the A operand of every tile row, its L2_LIST candidates are the columns of two
// tiles, and the MFMA steps run in l2_topk_split_kernel's order (step (b, e): k = 8 b + e and 8 b + 4 + e), so the key of a
// candidate has the bits the plain search gives that (query row, database row) pair. Sorted by (key, id, slot) like a merge; the
// first k are the result. The certificate is evaluated in fp64 with every rounding against it.
__global__ __launch_bounds__(256) void l2_rescore_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ x,
                                                         int ldx, int nx, const float* __restrict__ xn, const float* __restrict__ qn,
                                                         const float* __restrict__ qerr, const float* __restrict__ qnrm,
                                                         const float* __restrict__ xmax, const float* __restrict__ exmax,
                                                         const float* __restrict__ ckey, const int* __restrict__ cid, int d, int k,
                                                         float* __restrict__ D, int64_t* __restrict__ I, float* __restrict__ E,
                                                         uint8_t* __restrict__ cert) {
  __shared__ KI cand[4][L2_LIST];
  __shared__ KI srt[4][L2_LIST];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  if (row >= nq) return;                         // uniform over the wave; no workgroup barrier below
  const int r = lane & 31, h = lane >> 5;
  const int id0 = cid[(size_t)row * L2_LIST + r], id1 = cid[(size_t)row * L2_LIST + 32 + r];
  const bool real0 = id0 >= 0 && id0 < nx, real1 = id1 >= 0 && id1 < nx;      // a pad (or anything that is no row id) is read nowhere
  const float* qp = q + (size_t)row * ldq + 4 * h;
  const float* x0 = x + (size_t)(real0 ? id0 : 0) * ldx + 4 * h;
  const float* x1 = x + (size_t)(real1 ? id1 : 0) * ldx + 4 * h;
  f32x16 acc0 = {}, acc1 = {};
  for (int b = 0; b < d / 8; ++b) {
    const f32x4 a = ld4(qp + 8 * b);
    const f32x4 b0 = real0 ? ld4(x0 + 8 * b) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 b1 = real1 ? ld4(x1 + 8 * b) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b0[e], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b1[e], acc1, 0, 0, 0);
    }
  }
  // every tile row is the same query row: register 0 of lane (r, h) is the pair (row, column r) in both halves
  const KI c0 = real0 ? KI{xn[id0] - (acc0[0] + acc0[0]), id0} : ki_pad();
  const KI c1 = real1 ? KI{xn[id1] - (acc1[0] + acc1[0]), id1} : ki_pad();
  cand[w][lane] = h ? c1 : c0;
  __builtin_amdgcn_wave_barrier();
  const KI e = cand[w][lane];
  int rank = 0;
  for (int f = 0; f < L2_LIST; ++f) rank += ki_less(cand[w][f], f, e, lane) ? 1 : 0;
  srt[w][rank] = e;                              // distinct ranks unless a key is NaN, and then the row is not certified
  __builtin_amdgcn_wave_barrier();
  if (lane < k) {
    const KI o = srt[w][lane];
    const bool real = o.i != L2_PAD_ID;
    D[(size_t)row * k + lane] = real ? fmaxf(0.f, qn[row] + o.k) : __builtin_inff();
    I[(size_t)row * k + lane] = real ? (int64_t)o.i : (int64_t)-1;
  }
  if (lane != 0) return;
  const double Nq = (double)qnrm[row], eq = (double)qerr[row], X = (double)*xmax, EX = (double)*exmax;
  // E = 2 (||q - q~|| Xmax + Nq EXmax) + slack; the last factor covers the fp64 roundings of this line
  const double Ed = (2.0 * (eq * X + Nq * EX) + 0x1p-24 * (16.0 * d * Nq * X + 8.0 * X * X) + 0x1p-100 * (1.0 + Nq + X)) * (1.0 + 0x1p-40);
  const float Ef = f32_up(Ed);
  const float thr = ckey[(size_t)row * L2_LIST + L2_LIST - 1];
  const bool thr_pad = cid[(size_t)row * L2_LIST + L2_LIST - 1] == L2_PAD_ID;
  const float kk = srt[w][k - 1].k;
  // no certificate where a norm is NaN, infinite or so large that a dot or a squared norm could overflow
  bool ok = Nq < 0x1p60 && X < 0x1p60 && EX < 0x1p60 && eq < 0x1p60 && Ef < __builtin_inff();
  if (ok && !thr_pad) {
    double lhs = (double)thr - (double)Ef;
    lhs -= fabs(lhs) * 0x1p-50;                  // the fp64 subtraction rounds: only ever towards "not certified"
    ok = fabsf(thr) < __builtin_inff() && fabsf(kk) < __builtin_inff() && lhs > (double)kk;
  }
  E[row] = Ef;
  cert[row] = ok ? 1 : 0;
}

}  // namespace

long nsid_l2_coarse_ws_bytes(long nq, long nx) {
  int S, c;
  l2_plan_coarse(nq, nx, &S, &c);
  return (long)S * nq * L2_LIST * (long)(sizeof(float) + sizeof(int));
}

extern "C" int nsid_bf16_rows(const float* x, int ldx, int n, int d, void* xb, int ldb, float* err, float* nrm, void* stream) {
  NSID_REQUIRE(n >= 0 && l2_shape_ok(d));
  if (n == 0) return NSID_OK;
  NSID_REQUIRE(x && xb && err && nrm && ldx >= d && ldx % 4 == 0 && nsid_aligned16(x) && ldb >= d && ldb % 8 == 0 && nsid_aligned16(xb));
  nsid_count(NSID_C_bf16_rows);
  NSID_LAUNCH(bf16_rows_kernel, dim3((n + 15) / 16), dim3(256), 0, static_cast<hipStream_t>(stream), x, ldx, n, d,
              static_cast<__bf16*>(xb), ldb, err, nrm);
  return nsid_launch_status();
}

extern "C" int nsid_flat_l2_topk_coarse(const void* qb, int ldq, int nq, const void* xb, int ldx, int nx, const float* x_sqnorm,
                                        const int* ex_lo, const int* ex_hi, int d, float* ckey, int* cid, void* ws, size_t ws_bytes,
                                        void* stream) {
  NSID_REQUIRE(nq >= 0 && nx >= 0 && d % 16 == 0 && d >= 16 && d <= 256);
  if (nq == 0) return NSID_OK;
  NSID_REQUIRE(qb && ckey && cid && ws && ldq >= d && ldq % 8 == 0 && nsid_aligned16(qb) && nsid_aligned16(ws));
  NSID_REQUIRE(nx == 0 || (xb && x_sqnorm && ldx >= d && ldx % 8 == 0 && nsid_aligned16(xb)));
  NSID_REQUIRE((ex_lo == nullptr) == (ex_hi == nullptr));
  int S, chunk;
  l2_plan_coarse(nq, nx, &S, &chunk);
  const size_t per = (size_t)S * nq * L2_LIST;
  NSID_REQUIRE(ws_bytes >= per * (sizeof(float) + sizeof(int)));
  float* wkey = static_cast<float*>(ws);
  int* wid = reinterpret_cast<int*>(wkey + per);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const __bf16* q = static_cast<const __bf16*>(qb);
  const __bf16* x = static_cast<const __bf16*>(xb);
  nsid_count(NSID_C_flat_l2_topk_coarse);
  const int rc = ex_lo ? dispatch_coarse<true, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256>(
                             d, q, ldq, nq, x, ldx, nx, x_sqnorm, S, chunk, wkey, wid, ex_lo, ex_hi, st)
                       : dispatch_coarse<false, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256>(
                             d, q, ldq, nq, x, ldx, nx, x_sqnorm, S, chunk, wkey, wid, nullptr, nullptr, st);
  if (rc != NSID_OK) return rc;
  NSID_LAUNCH((l2_topk_merge_kernel<int, L2_OUT_RAW>), dim3(nq), dim3(256), 0, st, wkey, wid, S, L2_LIST, nullptr, ckey, cid);
  return nsid_launch_status();
}

extern "C" int nsid_flat_l2_rescore(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* x_sqnorm,
                                    const float* q_sqnorm, const float* q_err, const float* q_nrm, const float* xmax,
                                    const float* exmax, const float* ckey, const int* cid, int d, int k, float* D, int64_t* I, float* E,
                                    uint8_t* cert, void* stream) {
  NSID_REQUIRE(nq >= 0 && nx >= 0 && d % 16 == 0 && d >= 16 && d <= 256 && k >= 1 && k <= L2_LIST);
  if (nq == 0) return NSID_OK;
  NSID_REQUIRE(q && q_sqnorm && q_err && q_nrm && xmax && exmax && ckey && cid && D && I && E && cert && ldq >= d && ldq % 4 == 0 &&
               nsid_aligned16(q));
  NSID_REQUIRE(nx == 0 || (x && x_sqnorm && ldx >= d && ldx % 4 == 0 && nsid_aligned16(x)));
  nsid_count(NSID_C_flat_l2_rescore);
  NSID_LAUNCH(l2_rescore_kernel, dim3((nq + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), q, ldq, nq, x, ldx, nx, x_sqnorm,
              q_sqnorm, q_err, q_nrm, xmax, exmax, ckey, cid, d, k, D, I, E, cert);
  return nsid_launch_status();
}
