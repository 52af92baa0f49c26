// The attention tile of the stage-2 classifier (downstream.py:30-78 CrossAttentionClassifier), shared by its evaluation kernels
// (rerank.hip) and its training kernels (clf_train.hip): the constants, the 32 x 32 MFMA register map, the masked row softmax, the
// column sums, the workgroup -> (group, candidate, query chunk) decode, the folded tail and the dispatch over the widths. The head
// of up to 4 x 4 such tiles (33 .. 128 nodes) is here as well, clf_wide_logits / _softmax / _colsums: clf_attn_fwd_wide_kernel runs
// these three per query tile, and clf_pair_wide_kernel spells the same statements out (rerank.hip says why). So are the two small
// pieces that the training kernels of both node ranges share, clf_av_head and clf_da.
//
// One tile is S^T[key][query] of 32 keys x 32 queries from v_mfma_f32_32x32x2f32 with A = K rows and B = Q rows: lane (r, hh), r =
// lane & 31, hh = lane >> 5, holds in register i the score of query r against key acc_row(i, hh). The softmax of a query therefore
// runs over the 16 registers of a lane and the two lane halves, the mean over the queries over the 32 lanes of a half. Every sum here
// runs in one fixed order, and the evaluation and training kernels spell it the same way: a trained state scores in evaluation
// exactly what a training forward with a ones mask gives (tests/test_clf_train_gpu.py).
#pragma once
#include "nsid_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CLF_H = NSID_CLF_H;          // heads; node channels C = 4 DH are template parameters of the kernels
constexpr int CLF_TILE = 32;               // nodes of one 32 x 32 MFMA tile
constexpr int CLF_HID = NSID_CLF_HID;      // fc.0 width
constexpr int CLF_PW = CLF_H * CLF_HID;    // P row of the folded candidate side: one fc.0-wide block per head
static_assert(CLF_PW == NSID_CLF_PW && NSID_CLF_KP == NSID_CLF_C + NSID_CLF_PW, "include/nsid.h states the row widths");
static_assert(NSID_CLF_MAX_N == CLF_TILE, "the entries with one tile per side take a tile of nodes at most");
constexpr int CLF_MAX_NODES = NSID_CLF_MAX_N_EVAL;         // nodes at most of the _n entries (the multi-tile kernels)
constexpr int CLF_MAX_TILES = CLF_MAX_NODES / CLF_TILE;    // tiles per side at most
static_assert(CLF_MAX_TILES == 4, "one wave of a workgroup per query / key tile; 4 x 16 accumulators per lane");

// 1 / sqrt(DH), rounded to fp32
template <int DH> struct clf_scale;
template <> struct clf_scale<128> { static constexpr float v = 0.08838834764831845f; };
template <> struct clf_scale<160> { static constexpr float v = 0.07905694150420949f; };
template <> struct clf_scale<192> { static constexpr float v = 0.07216878364870323f; };
template <> struct clf_scale<256> { static constexpr float v = 0.0625f; };

static inline bool clf_width_ok(int C) { return C == 512 || C == 640 || C == 768 || C == 1024; }
// one launch of KERNEL<C, C / 4> for the supported widths
#define CLF_LAUNCH_C(C, KERNEL, grid, block, st, ...)                                    \
  switch (C) {                                                                           \
    case 512: NSID_LAUNCH((KERNEL<512, 128>), grid, block, 0, st, __VA_ARGS__); break;   \
    case 640: NSID_LAUNCH((KERNEL<640, 160>), grid, block, 0, st, __VA_ARGS__); break;   \
    case 768: NSID_LAUNCH((KERNEL<768, 192>), grid, block, 0, st, __VA_ARGS__); break;   \
    default: NSID_LAUNCH((KERNEL<1024, 256>), grid, block, 0, st, __VA_ARGS__); break;   \
  }

// key row of accumulator register i on lane half hh (the 32x32 C/D map)
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// ---- masked row softmax of a query over its keys. SCALED: the logits are acc * scale (training; the evaluation kernels get the
// scale folded into the caller's projection and pass acc as it stands). key0 = first key of the tile; keys >= N get no weight.
// One tile: clf_tile_softmax. Several key tiles of one query row: clf_tile_max over all of them, clf_half_max, clf_tile_exp over all
// of them in tile order, clf_half_sum, then clf_tile_norm of each. The masked values are computed on every register and then
// selected, which keeps the tile free of branches.
template <bool SCALED> __device__ __forceinline__ float clf_logit(float a, float scale) { return SCALED ? a * scale : a; }
template <bool SCALED>
__device__ __forceinline__ float clf_tile_max(const f32x16& acc, int key0, int hh, int N, float scale, float mx) {
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (key0 + acc_row(i, hh) < N) mx = fmaxf(mx, clf_logit<SCALED>(acc[i], scale));
  return mx;
}
__device__ __forceinline__ float clf_half_max(float mx) { return fmaxf(mx, __shfl_xor(mx, 32)); }

// e = exp(logit - mx), 0 on the keys >= N; returns sum + the 16 weights, added in register order. E: float[16] or f32x16, and e may
// be acc itself (the kernel with several key tiles keeps the weights in the accumulators)
template <bool SCALED, class E>
__device__ __forceinline__ float clf_tile_exp(const f32x16& acc, E& e, int key0, int hh, int N, float scale, float mx, float sum) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float x = expf(clf_logit<SCALED>(acc[i], scale) - mx);       // training: one fma, as acc * scale - mx contracts
    e[i] = key0 + acc_row(i, hh) < N ? x : 0.f;
    sum += e[i];
  }
  return sum;
}
__device__ __forceinline__ float clf_half_sum(float sum) { return sum + __shfl_xor(sum, 32); }

// v = the attention weights of the tile; a query row >= N (rowok false) has none. v may be e itself.
template <class E>
__device__ __forceinline__ void clf_tile_norm(const E& e, float (&v)[16], bool rowok, float sum) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float x = e[i] / sum;
    v[i] = rowok ? x : 0.f;
  }
}

template <bool SCALED>
__device__ __forceinline__ void clf_tile_softmax(const f32x16& acc, float (&v)[16], int hh, int N, bool rowok, float scale) {
  const float mx = clf_half_max(clf_tile_max<SCALED>(acc, 0, hh, N, scale, -__builtin_inff()));
  const float sum = clf_half_sum(clf_tile_exp<SCALED>(acc, v, 0, hh, N, scale, mx, 0.f));
  clf_tile_norm(v, v, rowok, sum);
}

// ---- column sums of a tile's weights v over the 32 query lanes of each half: a reduce-scatter that halves the registers at every
// step (16 .. 2: the lane with bit `off` of r set keeps the upper half and sends the lower), then one add across lanes r ^ 1. Both
// lanes of a pair return the sum of key clf_lane_key(r, hh); v is used up.
__device__ __forceinline__ float clf_colsum(float (&v)[16], int r) {
#pragma unroll
  for (int c = 16, off = 16; c > 1; c >>= 1, off >>= 1) {
    const bool up = (r & off) != 0;
#pragma unroll
    for (int i = 0; i < c / 2; ++i) {
      const float got = __shfl_xor(up ? v[i] : v[i + c / 2], off);      // sent first: the kept half is picked under its latency
      v[i] = (up ? v[i + c / 2] : v[i]) + got;
    }
  }
  return v[0] + __shfl_xor(v[0], 1);
}
// the key whose column sum clf_colsum leaves on lane (r, hh): bit 4 of r chose bit 3 of the register, bit 3 bit 2, bit 2 bit 1 and
// bit 1 bit 0; that register's row on this lane half
__device__ __forceinline__ int clf_lane_key(int r, int hh) {
  const int gf = (((r >> 4) & 1) << 3) | (((r >> 3) & 1) << 2) | (((r >> 2) & 1) << 1) | ((r >> 1) & 1);
  return acc_row(gf, hh);
}

// ---- the head of several tiles (N <= CLF_MAX_NODES, nT = ceil(N / 32) tiles per side): one query tile at a time against every key
// tile, so a row's max and sum stay in registers. K rows have LDK floats, Q rows LDQ; kh / qh = row 0 of the head's K / Q + 4 hh.
// Keys >= N get no weight, query rows >= N no share in the column sums; row 0 is addressed in place of a row >= N. The kt loops
// are unrolled over CLF_MAX_TILES with `kt < nT` inside, which keeps acc[] in registers.

// acc[kt] = S^T[key][query] of query tile qt against key tile kt < nT: A = K rows, B = Q rows, lane (r, hh) supplies dims
// 8 bb + 4 hh + e of its row at step (bb, e). Both fragments stream from global memory (L2) four k-steps of 8 at a time, which
// bounds the registers in flight.
template <int DH, int LDK, int LDQ>
__device__ __forceinline__ void clf_wide_logits(const float* kh, const float* qh, int qt, int r, int N, int nT,
                                                f32x16 (&acc)[CLF_MAX_TILES]) {
  static_assert(DH % 32 == 0, "K and Q are loaded four k-steps of 8 at a time");
  const int qrow = CLF_TILE * qt + r;
  const bool qok = qrow < N;
  const float* qp = qh + (size_t)(qok ? qrow : 0) * LDQ;
#pragma unroll 1
  for (int b0 = 0; b0 < DH / 8; b0 += 4) {
    f32x4 qb[4], ka[CLF_MAX_TILES][4];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) qb[bb] = qok ? ld4(qp + 8 * (b0 + bb)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
      if (kt < nT) {
        const int krow = CLF_TILE * kt + r;
        const float* kr = kh + (size_t)(krow < N ? krow : 0) * LDK;
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
}

// the softmax of a query row over the registers of all key tiles (tile kt: keys from 32 kt) and the two lane halves: the weights
// before the division replace the logits in acc, their sum is returned
template <bool SCALED>
__device__ __forceinline__ float clf_wide_softmax(f32x16 (&acc)[CLF_MAX_TILES], int hh, int N, int nT, float scale) {
  float mx = -__builtin_inff();
#pragma unroll
  for (int kt = 0; kt < CLF_MAX_TILES; ++kt)
    if (kt < nT) mx = clf_tile_max<SCALED>(acc[kt], CLF_TILE * kt, hh, N, scale, mx);
  mx = clf_half_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int kt = 0; kt < CLF_MAX_TILES; ++kt)
    if (kt < nT) sum = clf_tile_exp<SCALED>(acc[kt], acc[kt], CLF_TILE * kt, hh, N, scale, mx, sum);
  return clf_half_sum(sum);
}

// per key tile: v = the attention weights of tile (qt, kt), handed to sink(kt, v), then added to the tile's column sums cs[kt]
// (even lanes: key 32 kt + clf_lane_key). The sums accumulate over the query tiles in the order of the calls. Training's sink saves
// the tile.
template <class Sink>
__device__ __forceinline__ void clf_wide_colsums(const f32x16 (&acc)[CLF_MAX_TILES], bool rowok, float sum, int r, int nT,
                                                 float (&cs)[CLF_MAX_TILES], Sink&& sink) {
#pragma unroll
  for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
    if (kt < nT) {
      float v[16];
      clf_tile_norm(acc[kt], v, rowok, sum);
      sink(kt, v);
      cs[kt] += clf_colsum(v, r);
    }
  }
}

// ---- training, both node ranges. obar_h = a_h^T V_h: ah = the head's N column means (LDS), vh = V_h of the candidate's row 0 (rows
// of LDV floats), oh = the head's DH columns of the pair's obar. One wave, 64 columns at a time (the last block of DH = 160 is half
// full).
template <int DH, int LDV>
__device__ __forceinline__ void clf_av_head(const float* ah, const float* vh, int N, int lane, float* oh) {
  constexpr int OB = (DH + 63) / 64;
  float o[OB];
#pragma unroll
  for (int t = 0; t < OB; ++t) o[t] = 0.f;
  for (int m = 0; m < N; ++m) {
    const float a = ah[m];
#pragma unroll
    for (int t = 0; t < OB; ++t)
      if (DH % 64 == 0 || 64 * t + lane < DH) o[t] = fmaf(a, vh[(size_t)m * LDV + 64 * t + lane], o[t]);
  }
#pragma unroll
  for (int t = 0; t < OB; ++t)
    if (DH % 64 == 0 || 64 * t + lane < DH) oh[64 * t + lane] = o[t];
}

// V_h[key] . do_h on both lane halves of the key's lane: half hh of the DH dims on each, the halves added in one order on both. vh as
// above; a key >= N is not read and gives 0
template <int DH, int LDV>
__device__ __forceinline__ float clf_da(const float* vh, const float* doh, int key, int N, int hh) {
  constexpr int HALF = DH / 2;
  float part = 0.f;
  if (key < N) {
    const float* vr = vh + (size_t)key * LDV + HALF * hh;
    const float* dr = doh + HALF * hh;
#pragma unroll 4
    for (int e = 0; e < HALF; e += 4) {
      const f32x4 a = ld4(vr + e), b = ld4(dr + e);
      part = fmaf(a[0], b[0], part);
      part = fmaf(a[1], b[1], part);
      part = fmaf(a[2], b[2], part);
      part = fmaf(a[3], b[3], part);
    }
  }
  const float other = __shfl_xor(part, 32);
  return hh == 0 ? part + other : other + part;
}

// ---- pair lists of the evaluation kernels. Group g: {first query segment, query segments, offset into cidx, candidates}; its
// scores are the row-major (q count x c count) block at out + out_off[g]. tile_off: prefix sums of the groups' workgroups (c count x
// query chunks), ngroups + 1 entries. Workgroup b of the launch takes candidate jpos of group g (segment cand: not range-checked
// here) and the query chunk qc.
struct clf_tile { int g, q0, qn, cn, jpos, qc, cand; };
__device__ __forceinline__ clf_tile clf_tile_decode(const int* grp, const int* tile_off, int ngroups, const int* cidx) {
  // the last g with tile_off[g] <= blockIdx.x
  int lo = 0, hi = ngroups - 1;
  const int b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_off[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const int coff = grp[4 * lo + 2], cn = grp[4 * lo + 3], i = b - tile_off[lo];
  return clf_tile{lo, grp[4 * lo], grp[4 * lo + 1], cn, i % cn, i / cn, cidx[coff + i % cn]};
}

// ---- the tail. Sums over the wave are __shfl_xor trees over the offsets 32 .. 1: wave_sum (DPP) adds in another order.
__device__ __forceinline__ float clf_xor_sum(float z) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off);
  return z;
}
__device__ __forceinline__ float clf_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// folded tail of a pair: part0 / part1 = hidden[lane] / hidden[64 + lane] without g; tail = {g (128), w2 (128), b2}. Lane 0 stores
// s = sigmoid(w2 . relu(hidden + g) + b2).
__device__ __forceinline__ void clf_tail_store(float part0, float part1, const float* tail, int lane, float* dst) {
  const float h0 = fmaxf(part0 + tail[lane], 0.f), h1 = fmaxf(part1 + tail[64 + lane], 0.f);
  const float z = clf_xor_sum(fmaf(tail[CLF_HID + 64 + lane], h1, tail[CLF_HID + lane] * h0));
  if (lane == 0) *dst = clf_sigmoid(z + tail[2 * CLF_HID]);
}
