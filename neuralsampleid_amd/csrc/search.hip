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
// No atomics anywhere on the ranking path.
#include "nsid_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int L2_QT = 32;            // query rows per wave (the 32x32 MFMA tile)
constexpr int L2_LIST = 64;          // list slots per row (k <= 64)
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

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

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

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ---- phase 1 ----------------------------------------------------------------------------------------------------------------
// Lane (r, h) = (lane & 31, lane >> 5). MFMA step (b, e) pairs k = 8b + e (h = 0) with k = 8b + 4 + e (h = 1), so a lane reads
// 16 contiguous bytes of its row per block and the two halves read the adjacent 32 bytes. Accumulator register g of lane (r, h)
// is query row (g & 3) + 8 (g >> 2) + 4 h of the tile against database row j0 + r.
template <int D, int CH>
__global__ __launch_bounds__(64) void l2_topk_split_kernel(const float* __restrict__ q, int ldq, int nq, const float* __restrict__ x,
                                                           int ldx, int nx, const float* __restrict__ xn, int k, int nqt, int S,
                                                           int chunk, float* __restrict__ wkey, int* __restrict__ wid) {
  constexpr int NB = D / 8;          // 8-float blocks per row
  constexpr int NC = NB / CH;        // chunks per tile
  __shared__ KI list[L2_QT][L2_LIST];
  __shared__ KI queue[L2_QT][L2_Q1];
  __shared__ int cnt[L2_QT];

  const int lane = lane_id();
  const int r = lane & 31, h = lane >> 5;
  const int qt = blockIdx.x % nqt, s = blockIdx.x / nqt;
  const int q0 = qt * L2_QT;
  const int lo = s * chunk, hi = min(nx, lo + chunk);

  for (int t = lane; t < L2_QT * L2_LIST; t += 64) list[t / L2_LIST][t % L2_LIST] = ki_pad();
  if (lane < L2_QT) cnt[lane] = 0;
  // rows past nq get a threshold nothing passes
  if (lane < L2_QT && q0 + lane >= nq) list[lane][k - 1] = KI{-__builtin_inff(), 0};
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
    const float xv = cv ? xn[col] : 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int row = (g & 3) + 8 * (g >> 2) + 4 * h;
      const KI c{xv - (acc[g] + acc[g]), col};
      const bool pass = cv && ki_before(c, list[row][k - 1]);
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

  for (int rr = 0; rr < L2_QT; ++rr) {
    if (q0 + rr >= nq) break;
    const int c0 = __builtin_amdgcn_readfirstlane(cnt[rr]);
    if (c0 > 0) merge_queue(list[rr], queue[rr], c0, k, lane);
    if (lane < k) {
      const size_t o = ((size_t)(q0 + rr) * S + s) * k + lane;
      wkey[o] = list[rr][lane].k;
      wid[o] = list[rr][lane].i;
    }
  }
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

__global__ __launch_bounds__(256) void l2_topk_merge_kernel(const float* __restrict__ wkey, const int* __restrict__ wid, int S, int k,
                                                            const float* __restrict__ qn, float* __restrict__ D, int64_t* __restrict__ I) {
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
    const bool real = e.i != L2_PAD_ID;
    D[(size_t)row * k + lane] = real ? fmaxf(0.f, qn[row] + e.k) : __builtin_inff();
    I[(size_t)row * k + lane] = real ? (int64_t)e.i : (int64_t)-1;
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

bool l2_shape_ok(int d) { return d % 16 == 0 && d >= 16 && d <= 256; }

template <int D>
int launch_split(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* xn, int k, int nqt, int S, int chunk,
                 float* wkey, int* wid, hipStream_t st) {
  constexpr int NB = D / 8;
  constexpr int CH = (D <= 128 && NB % 8 == 0) ? 8 : (NB % 4 == 0 ? 4 : 2);
  hipLaunchKernelGGL((l2_topk_split_kernel<D, CH>), dim3(nqt * S), dim3(64), 0, st, q, ldq, nq, x, ldx, nx, xn, k, nqt, S, chunk,
                     wkey, wid);
  return hipGetLastError() == hipSuccess ? NSID_OK : NSID_ELAUNCH;
}

template <int... Ds>
int dispatch_split(int d, const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* xn, int k, int nqt, int S,
                   int chunk, float* wkey, int* wid, hipStream_t st) {
  int rc = NSID_EINVAL;
  ((d == Ds ? (rc = launch_split<Ds>(q, ldq, nq, x, ldx, nx, xn, k, nqt, S, chunk, wkey, wid, st), 0) : 0), ...);
  return rc;
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

long nsid_l2_ws_bytes(long nq, long nx, int k) {
  int S, c;
  nsid_l2_plan(nq, nx, &S, &c);
  return (long)S * nq * k * (long)(sizeof(float) + sizeof(int));
}

extern "C" int nsid_row_sqnorm(const float* x, int ldx, int n, int d, float* out, void* stream) {
  NSID_REQUIRE(n >= 0 && l2_shape_ok(d));
  if (n == 0) return NSID_OK;
  NSID_REQUIRE(x && out && ldx >= d && ldx % 4 == 0 && nsid_aligned16(x));
  nsid_count(NSID_C_row_sqnorm);
  hipLaunchKernelGGL(row_sqnorm_kernel, dim3((n + 15) / 16), dim3(256), 0, static_cast<hipStream_t>(stream), x, ldx, n, d, out);
  return hipGetLastError() == hipSuccess ? NSID_OK : NSID_ELAUNCH;
}

extern "C" int nsid_flat_l2_topk(const float* q, int ldq, int nq, const float* x, int ldx, int nx, const float* x_sqnorm,
                                 const float* q_sqnorm, int d, int k, float* D, int64_t* I, void* ws, size_t ws_bytes, void* stream) {
  NSID_REQUIRE(nq >= 0 && nx >= 0 && l2_shape_ok(d) && k >= 1 && k <= L2_LIST);
  if (nq == 0) return NSID_OK;
  NSID_REQUIRE(q && q_sqnorm && D && I && ws && ldq >= d && ldq % 4 == 0 && nsid_aligned16(q) && nsid_aligned16(ws));
  NSID_REQUIRE(nx == 0 || (x && x_sqnorm && ldx >= d && ldx % 4 == 0 && nsid_aligned16(x)));
  int S, chunk;
  nsid_l2_plan(nq, nx, &S, &chunk);
  const size_t per = (size_t)S * nq * k;
  NSID_REQUIRE(ws_bytes >= per * (sizeof(float) + sizeof(int)));
  float* wkey = static_cast<float*>(ws);
  int* wid = reinterpret_cast<int*>(wkey + per);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nqt = (nq + L2_QT - 1) / L2_QT;
  nsid_count(NSID_C_flat_l2_topk);
  const int rc = dispatch_split<16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256>(
      d, q, ldq, nq, x, ldx, nx, x_sqnorm, k, nqt, S, chunk, wkey, wid, st);
  if (rc != NSID_OK) return rc;
  hipLaunchKernelGGL(l2_topk_merge_kernel, dim3(nq), dim3(256), 0, st, wkey, wid, S, k, q_sqnorm, D, I);
  return hipGetLastError() == hipSuccess ? NSID_OK : NSID_ELAUNCH;
}

extern "C" int nsid_seq_scores(const float* q, int ldq, const float* x, int ldx, int nx, int d, const int64_t* I, int k,
                               const int* starts, const int* lens, int npairs, float* out, int ldo, void* stream) {
  NSID_REQUIRE(npairs >= 0 && nx >= 0 && l2_shape_ok(d) && k >= 1 && k <= L2_LIST && ldo >= 0 && ldo <= 4 * 65535);
  if (npairs == 0 || ldo == 0) return NSID_OK;
  NSID_REQUIRE(q && x && I && starts && lens && out && ldq >= d && ldx >= d);
  nsid_count(NSID_C_seq_scores);
  hipLaunchKernelGGL(seq_scores_kernel, dim3(npairs, (ldo + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), q, ldq, x, ldx,
                     nx, d, I, k, starts, lens, out, ldo);
  return hipGetLastError() == hipSuccess ? NSID_OK : NSID_ELAUNCH;
}
