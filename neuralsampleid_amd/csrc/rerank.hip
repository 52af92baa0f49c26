// Classifier re-rank pair scores (include/nsid.h nsid_clf_node_rows / nsid_clf_pair_scores, and their _n forms for up to 128 nodes).
//
// Reference: downstream.py:30-78 CrossAttentionClassifier in eval mode, called per candidate by eval_hr.py::eval_faiss_clf and
// eval_map.py::eval_faiss_map_clf. For one pair (query x_i, candidate x_j, both (N, C) node rows, C = 512, H = 4 heads of dh = 128):
//   A_h = softmax(Q_h K_h^T / sqrt(dh)),  m = mean_n (concat_h A_h V_h) Wo^T + bo,  s = sigmoid(w2 . relu(W1 m + b1) + b2).
// Nothing between out_proj, the node mean and fc.0 is nonlinear, so with a_h = the column mean of A_h (length N) and G = W1 Wo:
//   W1 m + b1 = g + sum_h G_h V_h^T a_h,   g = W1 bo + b1,   G_h = G[:, h dh : (h+1) dh].
// The candidate side is folded one step further: P_h = V_h G_h^T = X_j (G_h Wv_h)^T + G_h bv_h is a plain linear of the candidate's
// node rows, computed once per segment next to K (the caller's GEMM). Per pair this kernel then does Q K^T on the fp32 MFMA, the row
// softmax, the column mean, hidden = g + sum_h a_h^T P_h (16 k MAC), relu, the w2 dot and the sigmoid; only the score reaches HBM.
//
// One workgroup (8 waves) per (group, candidate, chunk of query segments): the candidate's K and P rows are staged into LDS once
// (128 KB); each wave takes query segments of the chunk in turn and streams their Q rows from global memory as MFMA B fragments.
// Every sum runs in one fixed order that depends on nothing but the pair, so a pair's score is bitwise independent of the rest of the
// call; there are no atomics.
//
// Widths: the kernel is a template on <C, DH> with C = 4 DH in {512, 640, 768, 1024}; P stays 4 x 128 (fc.0's width per head), so a
// candidate row is [K | P] of C + 512 floats. K (32 x (C + 4) floats) next to P (64 KB) fits the 160 KB of a workgroup up to C = 640
// (148 KB); at 768 and 1024 (164 / 197 KB) P alone is staged and every wave reads its K fragments from global memory, as it reads Q:
// the candidate's K rows are shared by the 64 segments of the chunk and stay in L2. The order of every sum is the same in both forms.
//
// Nodes: clf_pair_kernel covers N <= 32 (one 32 x 32 tile per head). 33 <= N <= 128 (evaluation only) is clf_pair_wide_kernel below:
// up to 4 x 4 tiles per head, P staged one head at a time; it has its own entries and leaves the N <= 32 kernels and scores alone.
//
// The tile arithmetic (register map, masked softmax, column sums), the pair-list decode and the folded tail are clf_common.h's,
// shared with the training kernels; what differs between the kernels here is how K, P and Q are staged.
#include "clf_common.h"

namespace {

constexpr int RR_WAVES = 8;
constexpr int RR_QCH = NSID_CLF_QCHUNK;      // query segments per workgroup
// K next to P in LDS (rows of C + 4 floats: +16 B so that the 32 rows of a fragment read start in different banks), else P alone
constexpr bool rr_k_in_lds(int C) { return (CLF_TILE * (C + 4) + CLF_TILE * CLF_PW + RR_WAVES * CLF_TILE) * 4 <= NSID_LDS_MAX; }

// grp, out_off, tile_off and cidx: the pair lists, see clf_tile_decode
template <int C, int DH>
__global__ __launch_bounds__(512) void clf_pair_kernel(const float* __restrict__ q, int nq_seg, const float* __restrict__ kp,
                                                       int nc_seg, int N, const int* __restrict__ grp,
                                                       const int64_t* __restrict__ out_off, const int* __restrict__ tile_off,
                                                       int ngroups, const int* __restrict__ cidx, const float* __restrict__ tail,
                                                       float* __restrict__ out, int64_t out_len) {
  static_assert(C == CLF_H * DH && DH % 8 == 0, "4 heads of DH channels");
  constexpr bool KLDS = rr_k_in_lds(C);
  static_assert(KLDS || DH % 64 == 0, "the streamed form loads K and Q eight k-steps at a time");
  constexpr int KLD = C + 4;           // LDS row of K
  constexpr int LDKP = C + CLF_PW;      // the candidates' projected rows: [K | P]
  __shared__ __attribute__((aligned(16))) float ks[KLDS ? CLF_TILE : 1][KLDS ? KLD : 4];
  __shared__ __attribute__((aligned(16))) float ps[CLF_TILE][CLF_PW];
  __shared__ float abar[RR_WAVES][CLF_TILE];

  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;

  const clf_tile t = clf_tile_decode(grp, tile_off, ngroups, cidx);
  if (t.cand < 0 || t.cand >= nc_seg) return;          // the host checks the lists; this only keeps a bad list in bounds

  // stage K and P of the candidate (rows >= N are zero)
  const float* kc = kp + (size_t)t.cand * N * LDKP;
  if constexpr (KLDS && C == CLF_PW) {
    for (int i = tid; i < CLF_TILE * (C / 4); i += 512) {
      const int n = i / (C / 4), c = 4 * (i % (C / 4));
      f32x4 kv = {0.f, 0.f, 0.f, 0.f}, pv = {0.f, 0.f, 0.f, 0.f};
      if (n < N) {
        kv = ld4(kc + (size_t)n * LDKP + c);
        pv = ld4(kc + (size_t)n * LDKP + C + c);
      }
      *reinterpret_cast<f32x4*>(&ks[n][c]) = kv;
      *reinterpret_cast<f32x4*>(&ps[n][c]) = pv;
    }
  } else {
    if constexpr (KLDS) {
      for (int i = tid; i < CLF_TILE * (C / 4); i += 512) {
        const int n = i / (C / 4), c = 4 * (i % (C / 4));
        *reinterpret_cast<f32x4*>(&ks[n][c]) = n < N ? ld4(kc + (size_t)n * LDKP + c) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    for (int i = tid; i < CLF_TILE * (CLF_PW / 4); i += 512) {
      const int n = i / (CLF_PW / 4), c = 4 * (i % (CLF_PW / 4));
      *reinterpret_cast<f32x4*>(&ps[n][c]) = n < N ? ld4(kc + (size_t)n * LDKP + C + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __syncthreads();

  const float invN = 1.0f / (float)N;
  const int s_end = min(t.qn, (t.qc + 1) * RR_QCH);
  const int jf = clf_lane_key(r, hh);

  for (int s = t.qc * RR_QCH + w; s < s_end; s += RR_WAVES) {
    const int qseg = t.q0 + s;
    if (qseg < 0 || qseg >= nq_seg) continue;
    const int64_t o = out_off[t.g] + (int64_t)s * t.cn + t.jpos;
    if (o < 0 || o >= out_len) continue;
    const float* qp = q + ((size_t)qseg * N + (r < N ? r : 0)) * C + 4 * hh;
    float part0 = 0.f, part1 = 0.f;             // hidden[lane], hidden[64 + lane] without g

    // K in LDS: the next head's Q fragments are fetched while this head's run (DH / 8 f32x4 in flight)
    f32x4 qf[KLDS ? DH / 8 : 1];
    if constexpr (KLDS) {
#pragma unroll
      for (int bb = 0; bb < DH / 8; ++bb) qf[bb] = r < N ? ld4(qp + 8 * bb) : f32x4{0.f, 0.f, 0.f, 0.f};
    }

#pragma unroll
    for (int h = 0; h < CLF_H; ++h) {
      // S^T[key][query]: A = K rows (LDS), B = Q rows; lane (r, hh) supplies dims 8 bb + 4 hh + e of row r at step (bb, e)
      f32x16 acc = {};
      if constexpr (KLDS) {
#pragma unroll
        for (int bb = 0; bb < DH / 8; ++bb) {
          const f32x4 ka = *reinterpret_cast<const f32x4*>(&ks[r][h * DH + 8 * bb + 4 * hh]);
          const f32x4 qb = qf[bb];
          if (h + 1 < CLF_H) qf[bb] = r < N ? ld4(qp + (h + 1) * DH + 8 * bb) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[e], qb[e], acc, 0, 0, 0);
        }
      } else {
        // K from global memory (L2): both fragments are loaded 8 steps at a time, which bounds the registers in flight
        const float* kr = kc + (size_t)(r < N ? r : 0) * LDKP + h * DH + 4 * hh;
#pragma unroll 1
        for (int b0 = 0; b0 < DH / 8; b0 += 8) {
          f32x4 ka[8], qb[8];
#pragma unroll
          for (int bb = 0; bb < 8; ++bb) {
            ka[bb] = r < N ? ld4(kr + 8 * (b0 + bb)) : f32x4{0.f, 0.f, 0.f, 0.f};
            qb[bb] = r < N ? ld4(qp + h * DH + 8 * (b0 + bb)) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int bb = 0; bb < 8; ++bb)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[bb][e], qb[bb][e], acc, 0, 0, 0);
        }
      }
      // softmax over the keys of query r, then the mean over the queries
      float v[16];
      clf_tile_softmax<false>(acc, v, hh, N, r < N, 1.0f);
      const float cs = clf_colsum(v, r);
      if ((r & 1) == 0) abar[w][jf] = cs * invN;
      __builtin_amdgcn_wave_barrier();
      // hidden += a_h^T P_h
      for (int m = 0; m < N; ++m) {
        const float a = abar[w][m];
        part0 = fmaf(a, ps[m][h * CLF_HID + lane], part0);
        part1 = fmaf(a, ps[m][h * CLF_HID + 64 + lane], part1);
      }
      __builtin_amdgcn_wave_barrier();
    }
    clf_tail_store(part0, part1, tail, lane, out + o);
  }
}

// ---- 33 <= N <= 128 (nsid_clf_pair_scores_n): the attention of a head is up to 4 x 4 tiles of 32 x 32 --------------------------------
// One workgroup (8 waves) per (group, candidate, chunk of 64 query segments), as above, and the same arithmetic. The candidate's P
// (N x 512 floats, 256 KB at N = 128) no longer fits the LDS, one head's P_h (128 x 128 floats, 64 KB) does: the waves walk the four
// heads together, P_h is staged per head, and every wave runs its segments of the chunk (at most 8) against it. K and Q fragments
// stream from global memory (L2), as in the C >= 768 form above: one query tile's fragment is used against the up to four key tiles
// (4 x 16 accumulator registers), so a row's max and sum are in registers; the column sums of a key tile accumulate over the query
// tiles in their order. A pair's partial hidden vector waits in LDS between two heads (lane-private slots). Keys >= N get no weight,
// query rows >= N no share in the column mean, which divides by N; no row >= N of a segment is addressed.
// The query-tile loop below is, statement for statement, clf_common.h's clf_wide_logits / _softmax / _colsums with SCALED = false
// and an empty sink, which the training forward calls. It is written out here because the helper form measured 0.2 % slower on the
// hit-rate-like block at 128 nodes (docs/experiments.md, "One multi-tile head"); a change to either goes into both.
constexpr int RW_SLOTS = RR_QCH / RR_WAVES;   // segments of a chunk per wave

template <int C, int DH>
__global__ __launch_bounds__(512) void clf_pair_wide_kernel(const float* __restrict__ q, int nq_seg, const float* __restrict__ kp,
                                                            int nc_seg, int N, const int* __restrict__ grp,
                                                            const int64_t* __restrict__ out_off, const int* __restrict__ tile_off,
                                                            int ngroups, const int* __restrict__ cidx,
                                                            const float* __restrict__ tail, float* __restrict__ out,
                                                            int64_t out_len) {
  static_assert(C == CLF_H * DH && DH % 32 == 0, "4 heads of DH channels; K and Q are loaded four k-steps of 8 at a time");
  constexpr int LDKP = C + CLF_PW;      // the candidates' projected rows: [K | P]
  __shared__ __attribute__((aligned(16))) float ps[CLF_MAX_NODES][CLF_HID];          // P_h of the candidate
  __shared__ float hacc[RR_QCH][CLF_HID];                                   // the pairs' hidden vectors between two heads
  __shared__ float abar[RR_WAVES][CLF_MAX_NODES];

  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;

  const clf_tile t = clf_tile_decode(grp, tile_off, ngroups, cidx);
  if (t.cand < 0 || t.cand >= nc_seg) return;          // the host checks the lists; this only keeps a bad list in bounds (uniform)

  const float* kc = kp + (size_t)t.cand * N * LDKP;
  const int nT = (N + 31) >> 5;
  const float invN = 1.0f / (float)N;
  const int s_end = min(t.qn, (t.qc + 1) * RR_QCH);
  const int jf = clf_lane_key(r, hh);

#pragma unroll 1
  for (int h = 0; h < CLF_H; ++h) {
    __syncthreads();                                   // every wave is done with the last head's P_h
    for (int i = tid; i < N * (CLF_HID / 4); i += 512) {
      const int n = i / (CLF_HID / 4), c = 4 * (i % (CLF_HID / 4));
      *reinterpret_cast<f32x4*>(&ps[n][c]) = ld4(kc + (size_t)n * LDKP + C + h * CLF_HID + c);
    }
    __syncthreads();

#pragma unroll 1
    for (int slot = 0; slot < RW_SLOTS; ++slot) {
      const int s = t.qc * RR_QCH + w + slot * RR_WAVES;
      if (s >= s_end) break;
      const int qseg = t.q0 + s;
      if (qseg < 0 || qseg >= nq_seg) continue;
      const int64_t o = out_off[t.g] + (int64_t)s * t.cn + t.jpos;
      if (o < 0 || o >= out_len) continue;
      const float* qs = q + (size_t)qseg * N * C + h * DH + 4 * hh;
      const float* kh = kc + h * DH + 4 * hh;

      float cs[CLF_MAX_TILES] = {0.f, 0.f, 0.f, 0.f};  // column sums of the key tiles (even lanes: key 32 kt + jf)
#pragma unroll 1
      for (int qt = 0; qt < nT; ++qt) {
        // S^T[key][query] of query tile qt against every key tile: A = K rows, B = Q rows; lane (r, hh) supplies dims
        // 8 bb + 4 hh + e of its row at step (bb, e)
        const int qrow = 32 * qt + r;
        const bool qok = qrow < N;
        const float* qp = qs + (size_t)(qok ? qrow : 0) * C;
        f32x16 acc[CLF_MAX_TILES] = {};
#pragma unroll 1
        for (int b0 = 0; b0 < DH / 8; b0 += 4) {
          f32x4 qb[4], ka[CLF_MAX_TILES][4];
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) qb[bb] = qok ? ld4(qp + 8 * (b0 + bb)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
            if (kt < nT) {
              const int krow = 32 * kt + r;
              const float* kr = kh + (size_t)(krow < N ? krow : 0) * LDKP;
#pragma unroll
              for (int bb = 0; bb < 4; ++bb) ka[kt][bb] = krow < N ? ld4(kr + 8 * (b0 + bb)) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
          }
#pragma unroll
          for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
            if (kt < nT) {
#pragma unroll
              for (int bb = 0; bb < 4; ++bb)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[kt][bb][e], qb[bb][e], acc[kt], 0, 0, 0);
            }
          }
        }
        // the softmax of query qrow runs over the registers of all key tiles (tile kt: keys from 32 kt) and the two lane halves
        float mx = -__builtin_inff();
#pragma unroll
        for (int kt = 0; kt < CLF_MAX_TILES; ++kt)
          if (kt < nT) mx = clf_tile_max<false>(acc[kt], 32 * kt, hh, N, 1.0f, mx);
        mx = clf_half_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < CLF_MAX_TILES; ++kt)
          if (kt < nT) sum = clf_tile_exp<false>(acc[kt], acc[kt], 32 * kt, hh, N, 1.0f, mx, sum);
        sum = clf_half_sum(sum);
#pragma unroll
        for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
          if (kt < nT) {
            float v[16];
            clf_tile_norm(acc[kt], v, qok, sum);
            cs[kt] += clf_colsum(v, r);
          }
        }
      }
      if ((r & 1) == 0) {
#pragma unroll
        for (int kt = 0; kt < CLF_MAX_TILES; ++kt)
          if (kt < nT) abar[w][32 * kt + jf] = cs[kt] * invN;
      }
      __builtin_amdgcn_wave_barrier();
      // hidden += a_h^T P_h
      const int pair = w * RW_SLOTS + slot;
      float part0 = h ? hacc[pair][lane] : 0.f, part1 = h ? hacc[pair][64 + lane] : 0.f;      // hidden[lane], hidden[64 + lane] without g
      for (int m = 0; m < N; ++m) {
        const float a = abar[w][m];
        part0 = fmaf(a, ps[m][lane], part0);
        part1 = fmaf(a, ps[m][64 + lane], part1);
      }
      __builtin_amdgcn_wave_barrier();
      if (h + 1 < CLF_H) {
        hacc[pair][lane] = part0;
        hacc[pair][64 + lane] = part1;
        continue;
      }
      clf_tail_store(part0, part1, tail, lane, out + o);
    }
  }
}

// (S, C, N) node matrices -> (S N, C) node rows (+ pos[n][c]); 32 channels per workgroup through an LDS tile of NMAX nodes
template <int NMAX>
__global__ __launch_bounds__(256) void clf_node_rows_kernel(const float* __restrict__ x, int C, int N, const float* __restrict__ pos,
                                                            float* __restrict__ rows) {
  __shared__ float tile[32][NMAX + 1];
  const int s = blockIdx.x, c0 = blockIdx.y * 32;
  for (int i = threadIdx.x; i < 32 * N; i += 256) {
    const int c = i / N, n = i % N;
    tile[c][n] = x[((size_t)s * C + c0 + c) * N + n];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 32 * N; i += 256) {
    const int n = i / 32, c = i % 32;
    rows[((size_t)s * N + n) * C + c0 + c] = tile[c][n] + (pos ? pos[(size_t)n * C + c0 + c] : 0.f);
  }
}

// the entries have checked C and N <= NMAX
template <int NMAX>
int launch_node_rows(const float* x, int S, int C, int N, const float* pos, float* rows, void* stream, NsidCounterKey key) {
  if (S == 0) return NSID_OK;
  NSID_REQUIRE(x && rows);
  nsid_count(key);
  NSID_LAUNCH(clf_node_rows_kernel<NMAX>, dim3(S, C / 32), dim3(256), 0, static_cast<hipStream_t>(stream), x, C, N, pos, rows);
  return nsid_launch_status();
}

// wide: clf_pair_wide_kernel (N <= 128), else clf_pair_kernel (N <= 32)
int launch_pair_scores(bool wide, const float* q, int nq_seg, const float* kp, int nc_seg, int C, int N, const int* groups,
                       const int64_t* out_off, const int* tile_off, int ngroups, int ntiles, const int* cidx, const float* tail,
                       float* out, int64_t out_len, void* stream) {
  NSID_REQUIRE(clf_width_ok(C));
  NSID_REQUIRE(nq_seg >= 0 && nc_seg >= 0 && N >= 1 && N <= (wide ? CLF_MAX_NODES : CLF_TILE) && ngroups >= 0 && ntiles >= 0 &&
               out_len >= 0);
  if (ngroups == 0 || ntiles == 0) return NSID_OK;
  NSID_REQUIRE(q && kp && groups && out_off && tile_off && cidx && tail && out && nsid_aligned16(q) && nsid_aligned16(kp));
  nsid_count(wide ? NSID_C_clf_pair_scores_n : NSID_C_clf_pair_scores);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (wide) {
    CLF_LAUNCH_C(C, clf_pair_wide_kernel, dim3(ntiles), dim3(512), st, q, nq_seg, kp, nc_seg, N, groups, out_off, tile_off, ngroups,
                 cidx, tail, out, out_len);
  } else {
    CLF_LAUNCH_C(C, clf_pair_kernel, dim3(ntiles), dim3(512), st, q, nq_seg, kp, nc_seg, N, groups, out_off, tile_off, ngroups, cidx,
                 tail, out, out_len);
  }
  return nsid_launch_status();
}

}  // namespace

extern "C" int nsid_clf_node_rows(const float* x, int S, int C, int N, const float* pos, float* rows, void* stream) {
  NSID_REQUIRE(S >= 0 && C > 0 && C % 32 == 0 && C <= 32 * 65535 && N >= 1 && N <= CLF_TILE);
  return launch_node_rows<CLF_TILE>(x, S, C, N, pos, rows, stream, NSID_C_clf_node_rows);
}

extern "C" int nsid_clf_node_rows_n(const float* x, int S, int C, int N, const float* pos, float* rows, void* stream) {
  NSID_REQUIRE(clf_width_ok(C));
  NSID_REQUIRE(S >= 0 && N >= 1 && N <= CLF_MAX_NODES);
  return launch_node_rows<CLF_MAX_NODES>(x, S, C, N, pos, rows, stream, NSID_C_clf_node_rows_n);
}

extern "C" int nsid_clf_pair_scores_n(const float* q, int nq_seg, const float* kp, int nc_seg, int C, int N, const int* groups,
                                      const int64_t* out_off, const int* tile_off, int ngroups, int ntiles, const int* cidx,
                                      const float* tail, float* out, int64_t out_len, void* stream) {
  return launch_pair_scores(true, q, nq_seg, kp, nc_seg, C, N, groups, out_off, tile_off, ngroups, ntiles, cidx, tail, out, out_len,
                            stream);
}

extern "C" int nsid_clf_pair_scores_c(const float* q, int nq_seg, const float* kp, int nc_seg, int C, int N, const int* groups,
                                      const int64_t* out_off, const int* tile_off, int ngroups, int ntiles, const int* cidx,
                                      const float* tail, float* out, int64_t out_len, void* stream) {
  return launch_pair_scores(false, q, nq_seg, kp, nc_seg, C, N, groups, out_off, tile_off, ngroups, ntiles, cidx, tail, out, out_len,
                            stream);
}

extern "C" int nsid_clf_pair_scores(const float* q, int nq_seg, const float* kp, int nc_seg, int N, const int* groups,
                                    const int64_t* out_off, const int* tile_off, int ngroups, int ntiles, const int* cidx,
                                    const float* tail, float* out, int64_t out_len, void* stream) {
  return nsid_clf_pair_scores_c(q, nq_seg, kp, nc_seg, NSID_CLF_C, N, groups, out_off, tile_off, ngroups, ntiles, cidx, tail, out, out_len,
                                stream);
}

