// Classifier training (include/nsid.h nsid_clf_mine_hard_negatives ... nsid_clf_seg_reduce).
//
// Reference: downstream.py:82-140, mine_hard_negatives and train: the stage-2 CrossAttentionClassifier (downstream.py:30-78) in
// training mode on the node matrices of the frozen encoder. For one pair (query segment x_q, candidate segment x_c, (N, C) node rows
// with the positional embedding added, C = 512, H = 4 heads of dh = 128):
//   Q = x_q Wq^T + bq,  [K | V] = x_c [Wk ; Wv]^T + [bk ; bv]           (per segment: the caller's fp32 GEMMs)
//   A_h = softmax(Q_h K_h^T / sqrt(dh)),  a_h = mean over query nodes of A_h (length N),  o_h = a_h^T V_h   (per pair: this file)
//   M = o Wo^T + bo,  H = M W1^T + b1                                    (per pair: the caller's fp32 GEMMs)
//   s = sigmoid(w2 . (relu(H) * keep) + b2)                              (per pair: this file; keep = the dropout mask / (1 - p))
// The node mean commutes with out_proj, so o (P x 512) is the only per-pair attention output that reaches HBM. The backward of the
// attention, with do_h = dL/do_h:
//   da_h = V_h do_h,  dV_p = a_h (x) do_h,  dS = A o (da / N - rowsum(A o da / N)),  dQ_p = dS K_h / sqrt(dh),  dK_p = dS^T Q_h / sqrt(dh)
// dQ_p and dK_p go to HBM per pair; nsid_clf_seg_reduce sums them (and forms dV) per segment in pair order, so every result here is
// a fixed-order sum: no atomics, and a pair's scores and per-pair gradients depend on nothing but the pair.
//
// Widths: the attention kernels and the per-segment sums are templates on <C, DH>, C = 4 DH in {512, 640, 768, 1024}; the saved
// attention layout (P, 4, 16, 64) and abar (P, 4, 32) do not depend on C. Mining and the head (fc.0 width 128) are the same at every C.
//
// Nodes: N <= 32 (CLF_TILE), one 32 x 32 tile per head. The tile arithmetic (register map, masked softmax, column sums) and the
// width dispatch are clf_common.h's, shared with the evaluation kernels, so a trained state scores there what it scores here.
// 1 <= N <= 128 (the _n entries): the *_wide_kernel forms below run a head's attention as up to 4 x 4 such tiles; the forward's head
// is clf_common.h's clf_wide_logits / _softmax / _colsums, statement for statement the evaluation kernel's for these node counts.
// Saved attention (P, 4, nT, nT, 16, 64), nT = ceil(N / 32), abar (P, 4, 128). Both node ranges share clf_av_head (obar) and clf_da
// (the backward's da) from there; each operation has one host function, launch_*(wide, ...), behind its _c, _n and C = 512 entries.
#include "clf_common.h"

namespace {

constexpr int CT_MINE_MAXN = NSID_CLF_MINE_MAX_ROWS;   // rows of the mining pool (2B) at most: their dots live in LDS
constexpr int CT_MINE_MAXD = NSID_CLF_MINE_MAX_D;
constexpr int CT_RED_THREADS = 512;  // nsid_clf_seg_reduce: one workgroup per segment, C / 64 float4 per thread cover N x C

// ------------------------------------------------------------------------------------------------ hard-negative mining
// (v, j) precedes (w, k) in the descending order with ties to the smaller index
__device__ __forceinline__ bool precedes(float v, int j, float w, int k) { return v > w || (v == w && j < k); }

// one workgroup per query row: the fp32 dots against all na pool rows (each a sequential fma chain over d) into LDS, then k + 1
// rounds of a block arg-max, each over the rows that come after the previous pick; ranks 1..k are written.
__global__ __launch_bounds__(256) void clf_mine_kernel(const float* __restrict__ zq, const float* __restrict__ za, int na, int d,
                                                       int k, int64_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float qs[CT_MINE_MAXD];
  __shared__ float dots[CT_MINE_MAXN];
  __shared__ float rv[4];
  __shared__ int rj[4];
  const int row = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  for (int e = tid; e < d; e += 256) qs[e] = zq[(size_t)row * d + e];
  __syncthreads();
  for (int j = tid; j < na; j += 256) {
    const float* zr = za + (size_t)j * d;
    float acc = 0.f;
    for (int e = 0; e < d; e += 4) {
      const f32x4 a = ld4(zr + e), q = *reinterpret_cast<const f32x4*>(&qs[e]);
      acc = fmaf(q[0], a[0], acc);
      acc = fmaf(q[1], a[1], acc);
      acc = fmaf(q[2], a[2], acc);
      acc = fmaf(q[3], a[3], acc);
    }
    dots[j] = acc;
  }
  __syncthreads();
  float pv = 0.f;
  int pj = -1;                                         // previous pick (none before rank 0)
  for (int r = 0; r <= k; ++r) {
    float bv = -__builtin_inff();
    int bj = 0x7fffffff;
    for (int j = tid; j < na; j += 256) {
      const float v = dots[j];
      if ((pj < 0 || precedes(pv, pj, v, j)) && precedes(v, j, bv, bj)) { bv = v; bj = j; }
    }
    // (v, j) is a total order on distinct j: any reduction tree finds the same winner
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oj = __shfl_xor(bj, off);
      if (precedes(ov, oj, bv, bj)) { bv = ov; bj = oj; }
    }
    if ((tid & 63) == 0) { rv[w] = bv; rj[w] = bj; }
    __syncthreads();
    bv = rv[0];
    bj = rj[0];
    for (int i = 1; i < 4; ++i)
      if (precedes(rv[i], rj[i], bv, bj)) { bv = rv[i]; bj = rj[i]; }
    __syncthreads();
    if (r > 0 && tid == 0) out[(size_t)row * k + r - 1] = bj;
    pv = bv;
    pj = bj;
  }
}

// ------------------------------------------------------------------------------------------------ attention forward
// One wave per pair, 4 pairs per workgroup. S^T[key][query] on the fp32 MFMA in clf_common.h's tile layout (A = K rows, B = Q rows,
// both streamed from global memory as fragments); the softmax runs over the keys of each query lane. A is stored in its register layout,
// (P, 4, 16, 64): the backward reloads the same registers. abar (P, 4, 32) = a_h; obar (P, C) = concat_h a_h^T V_h, 64 columns of
// a head at a time (the last block of DH = 160 is half full).
template <int C, int DH>
__global__ __launch_bounds__(256) void clf_attn_fwd_kernel(const float* __restrict__ q, int nq_seg, const float* __restrict__ kv,
                                                           int nc_seg, int N, const int* __restrict__ qi, const int* __restrict__ ci,
                                                           int P, float* __restrict__ obar, float* __restrict__ attn,
                                                           float* __restrict__ abar) {
  static_assert(C == CLF_H * DH && DH % 32 == 0, "4 heads of DH channels");
  constexpr int CT_C = C, CT_DH = DH, CT_KV = 2 * C;        // [K | V] rows
  __shared__ float abs_[4][CLF_TILE];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int p = blockIdx.x * 4 + w;
  if (p >= P) return;
  const int qs = qi[p], cs = ci[p];
  if (qs < 0 || qs >= nq_seg || cs < 0 || cs >= nc_seg) return;      // the host checks the lists; this only keeps a bad one in bounds
  const float scale = clf_scale<DH>::v;
  const float invN = 1.0f / (float)N;
  const bool rin = r < N;
  const float* qp = q + ((size_t)qs * N + (rin ? r : 0)) * CT_C + 4 * hh;
  const float* kp = kv + ((size_t)cs * N + (rin ? r : 0)) * CT_KV + 4 * hh;
  const float* vb = kv + (size_t)cs * N * CT_KV + CT_C;
  const int jf = clf_lane_key(r, hh);

#pragma unroll 1
  for (int h = 0; h < CLF_H; ++h) {
    f32x16 acc = {};
#pragma unroll
    for (int bb = 0; bb < CT_DH / 8; ++bb) {
      const f32x4 ka = rin ? ld4(kp + h * CT_DH + 8 * bb) : f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 qb = rin ? ld4(qp + h * CT_DH + 8 * bb) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[e], qb[e], acc, 0, 0, 0);
    }
    float v[16];
    clf_tile_softmax<true>(acc, v, hh, N, rin, scale);
    float* ap = attn + ((size_t)p * CLF_H + h) * 16 * 64 + lane;
#pragma unroll
    for (int i = 0; i < 16; ++i) ap[i * 64] = v[i];
    const float cs = clf_colsum(v, r);
    if ((r & 1) == 0) {
      abs_[w][jf] = cs * invN;
      abar[((size_t)p * CLF_H + h) * CLF_TILE + jf] = cs * invN;
    }
    __builtin_amdgcn_wave_barrier();
    clf_av_head<DH, CT_KV>(abs_[w], vb + h * CT_DH, N, lane, obar + (size_t)p * CT_C + h * CT_DH);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- 1 <= N <= 128 (nsid_clf_attn_fwd_n): a head's attention is nT x nT tiles of 32 x 32, nT = ceil(N / 32) ----------------------------
// One workgroup per pair, wave h = head h (the heads write disjoint columns of obar). The head's logits, softmax and column sums
// are clf_common.h's clf_wide_logits / _softmax / _colsums, statement for statement what clf_pair_wide_kernel scores with; the sink saves each tile here. Saved attention:
// (P, 4, nT, nT, 16, 64), tile (qt, kt) of a head in the register layout above (zero on keys >= N and query rows >= N).
// abar (P, 4, 128), zero past N. No row >= N of a segment is addressed.
template <int C, int DH>
__global__ __launch_bounds__(256) void clf_attn_fwd_wide_kernel(const float* __restrict__ q, int nq_seg, const float* __restrict__ kv,
                                                                int nc_seg, int N, const int* __restrict__ qi,
                                                                const int* __restrict__ ci, int P, float* __restrict__ obar,
                                                                float* __restrict__ attn, float* __restrict__ abar) {
  static_assert(C == CLF_H * DH, "4 heads of DH channels");
  constexpr int CT_C = C, CT_DH = DH, CT_KV = 2 * C;        // [K | V] rows
  __shared__ float abs_[CLF_H][CLF_MAX_NODES];
  const int lane = lane_id(), h = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int p = blockIdx.x;                                  // the grid is P workgroups
  const int qseg = qi[p], cseg = ci[p];
  if (qseg < 0 || qseg >= nq_seg || cseg < 0 || cseg >= nc_seg) return;      // uniform over the workgroup
  const float invN = 1.0f / (float)N;
  const int nT = (N + CLF_TILE - 1) / CLF_TILE;
  const float* qh = q + (size_t)qseg * N * CT_C + h * CT_DH + 4 * hh;
  const float* kh = kv + (size_t)cseg * N * CT_KV + h * CT_DH + 4 * hh;
  const float* vh = kv + (size_t)cseg * N * CT_KV + CT_C + h * CT_DH;
  float* ap = attn + ((size_t)p * CLF_H + h) * nT * nT * (16 * 64) + lane;
  const int jf = clf_lane_key(r, hh);

  float cs[CLF_MAX_TILES] = {0.f, 0.f, 0.f, 0.f};  // column sums of the key tiles (even lanes: key 32 kt + jf)
#pragma unroll 1
  for (int qt = 0; qt < nT; ++qt) {
    f32x16 acc[CLF_MAX_TILES] = {};
    clf_wide_logits<DH, CT_KV, CT_C>(kh, qh, qt, r, N, nT, acc);
    const float sum = clf_wide_softmax<true>(acc, hh, N, nT, clf_scale<DH>::v);
    clf_wide_colsums(acc, CLF_TILE * qt + r < N, sum, r, nT, cs, [&](int kt, const float (&v)[16]) {
      float* at = ap + (size_t)(qt * nT + kt) * (16 * 64);      // the saved tile (qt, kt)
#pragma unroll
      for (int i = 0; i < 16; ++i) at[i * 64] = v[i];
    });
  }
  if ((r & 1) == 0) {
#pragma unroll
    for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
      const float a = kt < nT ? cs[kt] * invN : 0.f;
      abs_[h][CLF_TILE * kt + jf] = a;
      abar[((size_t)p * CLF_H + h) * CLF_MAX_NODES + CLF_TILE * kt + jf] = a;
    }
  }
  __builtin_amdgcn_wave_barrier();
  clf_av_head<DH, CT_KV>(abs_[h], vh, N, lane, obar + (size_t)p * CT_C + h * CT_DH);
}

// ------------------------------------------------------------------------------------------------ head: relu, dropout, fc.3, sigmoid
__device__ __forceinline__ float relu_keep(float h, float keep) { return (h < 0.f ? 0.f : h) * keep; }

// one wave per pair: s = sigmoid(w2 . (relu(H) * keep) + b2)
__global__ __launch_bounds__(256) void clf_head_fwd_kernel(const float* __restrict__ hid, const float* __restrict__ keep,
                                                           const float* __restrict__ w2, const float* __restrict__ b2, int P,
                                                           float* __restrict__ s) {
  const int lane = lane_id(), p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;
  const float* hp = hid + (size_t)p * CLF_HID;
  const float* kp = keep + (size_t)p * CLF_HID;
  const float z = clf_xor_sum(fmaf(w2[64 + lane], relu_keep(hp[64 + lane], kp[64 + lane]), w2[lane] * relu_keep(hp[lane], kp[lane])));
  if (lane == 0) s[p] = clf_sigmoid(z + b2[0]);
}

// one wave per pair: dz = ds (1 - s) s (torch's sigmoid backward), dH = dz w2 keep where H > 0
__global__ __launch_bounds__(256) void clf_head_bwd_kernel(const float* __restrict__ ds, const float* __restrict__ s,
                                                           const float* __restrict__ hid, const float* __restrict__ keep,
                                                           const float* __restrict__ w2, int P, float* __restrict__ dh,
                                                           float* __restrict__ dz) {
  const int lane = lane_id(), p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;
  const float sp = s[p];
  const float g = ds[p] * (1.0f - sp) * sp;
  const size_t o = (size_t)p * CLF_HID;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int j = lane + 64 * t;
    dh[o + j] = hid[o + j] > 0.f ? g * w2[j] * keep[o + j] : 0.f;
  }
  if (lane == 0) dz[p] = g;
}

// one workgroup of 8 x 128 threads: dw2[j] = sum_p dz[p] (relu(H[p][j]) keep[p][j]) and db2 = sum_p dz[p]. Row group g sums the
// pairs p = g (mod 8) in pair order, then the 8 partials are added in group order: a fixed order that does not depend on the GPU.
constexpr int CT_WG_GROUPS = 8;
__global__ __launch_bounds__(CT_WG_GROUPS * CLF_HID) void clf_head_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ hid,
                                                                             const float* __restrict__ keep, int P,
                                                                             float* __restrict__ dw2, float* __restrict__ db2) {
  __shared__ float part[CT_WG_GROUPS][CLF_HID + 1];
  const int j = threadIdx.x % CLF_HID, g = threadIdx.x / CLF_HID;
  float acc = 0.f, accb = 0.f;
#pragma unroll 8
  for (int p = g; p < P; p += CT_WG_GROUPS) {
    const float d = dz[p];
    acc = fmaf(d, relu_keep(hid[(size_t)p * CLF_HID + j], keep[(size_t)p * CLF_HID + j]), acc);
    accb += d;
  }
  part[g][j] = acc;
  if (j == 0) part[g][CLF_HID] = accb;
  __syncthreads();
  if (threadIdx.x <= CLF_HID) {
    float s = part[0][threadIdx.x];
    for (int i = 1; i < CT_WG_GROUPS; ++i) s += part[i][threadIdx.x];
    if (threadIdx.x < CLF_HID) dw2[threadIdx.x] = s;
    else db2[0] = s;
  }
}

// ------------------------------------------------------------------------------------------------ attention backward
// One wave per pair, 4 pairs per workgroup. Per head: da (VALU: a 32 x DH matrix-vector product), dS in the forward's register
// layout (query on the lane, keys in the registers), dQ = dS K on the fp32 MFMA with dS as the A operand as it stands, then dS
// through LDS once (key on the lane) for dK = dS^T Q. 1 / sqrt(dh) is applied to dS. Rows >= N are neither read nor written.
template <int C, int DH>
__global__ __launch_bounds__(256) void clf_attn_bwd_kernel(const float* __restrict__ dobar, const float* __restrict__ attn,
                                                           const float* __restrict__ q, int nq_seg, const float* __restrict__ kv,
                                                           int nc_seg, int N, const int* __restrict__ qi, const int* __restrict__ ci,
                                                           int P, float* __restrict__ dq, float* __restrict__ dk) {
  static_assert(C == CLF_H * DH && DH % 32 == 0, "4 heads of DH channels");
  constexpr int CT_C = C, CT_DH = DH, CT_KV = 2 * C;
  __shared__ float dsT[4][CLF_TILE][CLF_TILE + 1];
  __shared__ float das[4][CLF_TILE];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int p = blockIdx.x * 4 + w;
  if (p >= P) return;
  const int qs = qi[p], cs = ci[p];
  if (qs < 0 || qs >= nq_seg || cs < 0 || cs >= nc_seg) return;
  const float scale = clf_scale<DH>::v;
  const float invN = 1.0f / (float)N;
  const bool rin = r < N;
  const float* qrow = q + (size_t)qs * N * CT_C;              // Q of the query segment (N x C)
  const float* krow = kv + (size_t)cs * N * CT_KV;            // [K | V] of the candidate (N x 2C)
  const float* dop = dobar + (size_t)p * CT_C;
  float* dqp = dq + (size_t)p * N * CT_C;
  float* dkp = dk + (size_t)p * N * CT_C;

#pragma unroll 1
  for (int h = 0; h < CLF_H; ++h) {
    // da[key r] = V[r][h] . do[h] / N
    const float da = clf_da<DH, CT_KV>(krow + CT_C + h * CT_DH, dop + h * CT_DH, r, N, hh);
    if (hh == 0) das[w][r] = rin ? da * invN : 0.f;
    __builtin_amdgcn_wave_barrier();
    const float* ap = attn + ((size_t)p * CLF_H + h) * 16 * 64 + lane;
    float a[16], g[16];
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      a[i] = ap[i * 64];
      g[i] = das[w][acc_row(i, hh)];
      t = fmaf(a[i], g[i], t);
    }
    const float to = __shfl_xor(t, 32);
    const float tr = hh == 0 ? t + to : to + t;          // rowsum over the 32 keys of query r
    float dS[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) dS[i] = a[i] * (g[i] - tr) * scale;

    // dQ[query][d0 + c] = sum_key dS[query][key] K[key][d0 + c]; step s: k index hh = key acc_row(s, hh)
#pragma unroll 1
    for (int d0 = 0; d0 < CT_DH; d0 += 32) {
      f32x16 acc = {};
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int key = acc_row(s, hh);
        const float kb = key < N ? krow[(size_t)key * CT_KV + h * CT_DH + d0 + r] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dS[s], kb, acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, hh);
        if (row < N) dqp[(size_t)row * CT_C + h * CT_DH + d0 + r] = acc[i];
      }
    }
    // dS^T through LDS: dsT[key][query]
#pragma unroll
    for (int i = 0; i < 16; ++i) dsT[w][acc_row(i, hh)][r] = dS[i];
    __builtin_amdgcn_wave_barrier();
    // dK[key][d0 + c] = sum_query dS[query][key] Q[query][d0 + c]; step s: k index hh = query 2 s + hh
#pragma unroll 1
    for (int d0 = 0; d0 < CT_DH; d0 += 32) {
      f32x16 acc = {};
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int qn = 2 * s + hh;
        const float qb = qn < N ? qrow[(size_t)qn * CT_C + h * CT_DH + d0 + r] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dsT[w][r][qn], qb, acc, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, hh);
        if (row < N) dkp[(size_t)row * CT_C + h * CT_DH + d0 + r] = acc[i];
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- 1 <= N <= 128 (nsid_clf_attn_bwd_n) ---------------------------------------------------------------------------------------------
// One workgroup of four waves per (pair, head). Wave w first forms da of key tile w into LDS. After a barrier wave qt (< nT) reloads
// the saved tiles (qt, *), takes t = rowsum(A o da) over all key tiles in tile order, forms dS = A o (da - t) / sqrt(dh) in the
// forward's register layout, leaves it in the LDS plane dS[query][key] (128 x 129 floats) and writes its dQ rows, dS K over all
// keys, once. After the second barrier wave kt (< nT) reads its key columns of the plane (key on the lane) and writes the dK rows of
// key tile kt, the query tiles summed in tile order inside the accumulators. No wave leaves ahead of a barrier: a skipped pair is
// skipped by the whole workgroup. Rows >= N are neither read nor written.
template <int C, int DH>
__global__ __launch_bounds__(256) void clf_attn_bwd_wide_kernel(const float* __restrict__ dobar, const float* __restrict__ attn,
                                                                const float* __restrict__ q, int nq_seg, const float* __restrict__ kv,
                                                                int nc_seg, int N, const int* __restrict__ qi,
                                                                const int* __restrict__ ci, int P, float* __restrict__ dq,
                                                                float* __restrict__ dk) {
  static_assert(C == CLF_H * DH && DH % 32 == 0, "4 heads of DH channels");
  constexpr int CT_C = C, CT_DH = DH, CT_KV = 2 * C;
  __shared__ float dsp[CLF_MAX_NODES][CLF_MAX_NODES + 1];                      // dS[query][key] of the head
  __shared__ float das[CLF_MAX_NODES];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int p = (int)(blockIdx.x >> 2), h = (int)(blockIdx.x & 3);      // the grid is 4 P workgroups
  const int qseg = qi[p], cseg = ci[p];
  if (qseg < 0 || qseg >= nq_seg || cseg < 0 || cseg >= nc_seg) return;      // uniform over the workgroup, ahead of every barrier
  const float scale = clf_scale<DH>::v;
  const float invN = 1.0f / (float)N;
  const int nT = (N + CLF_TILE - 1) / CLF_TILE;
  const float* qrow = q + (size_t)qseg * N * CT_C + h * CT_DH;              // Q_h of the query segment (row stride C)
  const float* krow = kv + (size_t)cseg * N * CT_KV + h * CT_DH;            // K_h of the candidate (row stride 2 C)
  const float* dop = dobar + (size_t)p * CT_C + h * CT_DH;
  float* dqp = dq + (size_t)p * N * CT_C + h * CT_DH;
  float* dkp = dk + (size_t)p * N * CT_C + h * CT_DH;

  {  // da[key] = V_h[key] . do_h / N for the keys of tile w
    const int key = CLF_TILE * w + r;
    const float da = clf_da<DH, CT_KV>(krow + CT_C, dop, key, N, hh);
    if (hh == 0) das[key] = key < N ? da * invN : 0.f;
  }
  __syncthreads();

  if (w < nT) {
    const int qt = w;
    const float* ap = attn + (((size_t)p * CLF_H + h) * nT + qt) * nT * (16 * 64) + lane;
    float dS[CLF_MAX_TILES][16];
    float t = 0.f;
#pragma unroll
    for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
      if (kt < nT) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          dS[kt][i] = ap[(size_t)kt * (16 * 64) + i * 64];
          t = fmaf(dS[kt][i], das[CLF_TILE * kt + acc_row(i, hh)], t);
        }
      }
    }
    const float to = __shfl_xor(t, 32);
    const float tr = hh == 0 ? t + to : to + t;          // rowsum over all keys of query 32 qt + r
#pragma unroll
    for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
      if (kt < nT) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = CLF_TILE * kt + acc_row(i, hh);
          dS[kt][i] = dS[kt][i] * (das[key] - tr) * scale;
          dsp[CLF_TILE * qt + r][key] = dS[kt][i];
        }
      }
    }
    // dQ[query][d0 + c] = sum_key dS[query][key] K[key][d0 + c]; step (kt, s): k index hh = key 32 kt + acc_row(s, hh)
#pragma unroll 1
    for (int d0 = 0; d0 < CT_DH; d0 += 32) {
      f32x16 acc = {};
#pragma unroll
      for (int kt = 0; kt < CLF_MAX_TILES; ++kt) {
        if (kt < nT) {
#pragma unroll
          for (int s = 0; s < 16; ++s) {
            const int key = CLF_TILE * kt + acc_row(s, hh);
            const float kb = key < N ? krow[(size_t)key * CT_KV + d0 + r] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dS[kt][s], kb, acc, 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = CLF_TILE * qt + acc_row(i, hh);
        if (row < N) dqp[(size_t)row * CT_C + d0 + r] = acc[i];
      }
    }
  }
  __syncthreads();

  if (w < nT) {
    const int kt = w;
    // dK[key][d0 + c] = sum_query dS[query][key] Q[query][d0 + c]; step (qt, s): k index hh = query 32 qt + 2 s + hh
    float dT[CLF_MAX_TILES][16];
#pragma unroll
    for (int qt = 0; qt < CLF_MAX_TILES; ++qt) {
      if (qt < nT) {
#pragma unroll
        for (int s = 0; s < 16; ++s) dT[qt][s] = dsp[CLF_TILE * qt + 2 * s + hh][CLF_TILE * kt + r];
      }
    }
#pragma unroll 1
    for (int d0 = 0; d0 < CT_DH; d0 += 32) {
      f32x16 acc = {};
#pragma unroll
      for (int qt = 0; qt < CLF_MAX_TILES; ++qt) {
        if (qt < nT) {
#pragma unroll
          for (int s = 0; s < 16; ++s) {
            const int qn = CLF_TILE * qt + 2 * s + hh;
            const float qb = qn < N ? qrow[(size_t)qn * CT_C + d0 + r] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dT[qt][s], qb, acc, 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = CLF_TILE * kt + acc_row(i, hh);
        if (row < N) dkp[(size_t)row * CT_C + d0 + r] = acc[i];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ per-segment sums
// One workgroup per segment: blocks [0, nq_seg) sum dQ_p over the pairs with qi[p] == seg, blocks [nq_seg, nq_seg + nc_seg) sum
// dK_p and dV_p = a_h (x) do_h over the pairs with ci[p] == seg. The pair list is scanned in chunks of 512 (a ballot per wave), the
// matches are added in pair order; a segment with no pairs gets zeros.
// The workgroup sums rows [n0, n0 + rows) of its segment, rows <= 32 (the float4 budget of a thread); abar has ABAR_LD floats per head.
template <int C, int DH, int ABAR_LD>
__device__ __forceinline__ void clf_seg_reduce_rows(const float* __restrict__ dq, const float* __restrict__ dk,
                                                    const float* __restrict__ abar, const float* __restrict__ dobar,
                                                    const int* __restrict__ qi, const int* __restrict__ ci, int P, int N, int nq_seg,
                                                    float* __restrict__ dq_seg, float* __restrict__ dkv_seg, int n0, int rows) {
  static_assert(C == CLF_H * DH && DH % 4 == 0 && (CLF_TILE * C) % (4 * CT_RED_THREADS) == 0, "4 heads of DH channels");
  constexpr int CT_C = C, CT_DH = DH, CT_KV = 2 * C;
  __shared__ uint64_t masks[CT_RED_THREADS / 64];
  const int tid = threadIdx.x, w = tid >> 6;
  const bool isq = (int)blockIdx.x < nq_seg;
  const int seg = isq ? (int)blockIdx.x : (int)blockIdx.x - nq_seg;
  const int* idx = isq ? qi : ci;
  const int nel = rows * CT_C;                               // elements of the workgroup's rows (a multiple of 128)
  constexpr int U = CLF_TILE * CT_C / (4 * CT_RED_THREADS);      // float4 per thread
  f32x4 acc[U], accv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) acc[u] = accv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* src = isq ? dq : dk;

  for (int base = 0; base < P; base += CT_RED_THREADS) {
    const int pp = base + tid;
    const bool hit = pp < P && idx[pp] == seg;
    const uint64_t m = __ballot(hit);
    if ((tid & 63) == 0) masks[w] = m;
    __syncthreads();
    for (int ww = 0; ww < CT_RED_THREADS / 64; ++ww) {
      uint64_t mm = masks[ww];
      while (mm) {
        const int b = __builtin_ctzll(mm);
        mm &= mm - 1;
        const int p = base + 64 * ww + b;
        const float* sp = src + ((size_t)p * N + n0) * CT_C;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = 4 * (tid + CT_RED_THREADS * u);
          if (e < nel) acc[u] += ld4(sp + e);
        }
        if (!isq) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int e = 4 * (tid + CT_RED_THREADS * u);
            if (e < nel) {
              const int n = e / CT_C, c = e % CT_C;
              const float a = abar[((size_t)p * CLF_H + c / CT_DH) * ABAR_LD + n0 + n];
              const f32x4 d = ld4(dobar + (size_t)p * CT_C + c);
#pragma unroll
              for (int x = 0; x < 4; ++x) accv[u][x] = fmaf(a, d[x], accv[u][x]);
            }
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = 4 * (tid + CT_RED_THREADS * u);
    if (e >= nel) continue;
    const int n = n0 + e / CT_C, c = e % CT_C;
    if (isq) {
      *reinterpret_cast<f32x4*>(dq_seg + ((size_t)seg * N + n) * CT_C + c) = acc[u];
    } else {
      float* o = dkv_seg + ((size_t)seg * N + n) * CT_KV + c;
      *reinterpret_cast<f32x4*>(o) = acc[u];
      *reinterpret_cast<f32x4*>(o + CT_C) = accv[u];
    }
  }
}

template <int C, int DH>
__global__ __launch_bounds__(CT_RED_THREADS) void clf_seg_reduce_kernel(const float* __restrict__ dq, const float* __restrict__ dk,
                                                                        const float* __restrict__ abar, const float* __restrict__ dobar,
                                                                        const int* __restrict__ qi, const int* __restrict__ ci, int P,
                                                                        int N, int nq_seg, float* __restrict__ dq_seg,
                                                                        float* __restrict__ dkv_seg) {
  clf_seg_reduce_rows<C, DH, CLF_TILE>(dq, dk, abar, dobar, qi, ci, P, N, nq_seg, dq_seg, dkv_seg, 0, N);
}

// nsid_clf_seg_reduce_n: grid (segments, node tiles); workgroup (seg, t) owns rows [32 t, min(N, 32 t + 32)) of its segment
template <int C, int DH>
__global__ __launch_bounds__(CT_RED_THREADS) void clf_seg_reduce_wide_kernel(const float* __restrict__ dq, const float* __restrict__ dk,
                                                                             const float* __restrict__ abar,
                                                                             const float* __restrict__ dobar, const int* __restrict__ qi,
                                                                             const int* __restrict__ ci, int P, int N, int nq_seg,
                                                                             float* __restrict__ dq_seg, float* __restrict__ dkv_seg) {
  const int n0 = CLF_TILE * (int)blockIdx.y;
  clf_seg_reduce_rows<C, DH, CLF_MAX_NODES>(dq, dk, abar, dobar, qi, ci, P, N, nq_seg, dq_seg, dkv_seg, n0, min(CLF_TILE, N - n0));
}

// ---- one host function per operation. wide: the _n entry (N <= 128, the *_wide_kernel and its grid), else the _c entry (N <= 32)
int launch_attn_fwd(bool wide, const float* q, int nq_seg, const float* kv, int nc_seg, int C, int N, const int* qi, const int* ci,
                    int P, float* obar, float* attn, float* abar, void* stream) {
  NSID_REQUIRE(clf_width_ok(C));
  NSID_REQUIRE(nq_seg >= 1 && nc_seg >= 1 && N >= 1 && N <= (wide ? CLF_MAX_NODES : CLF_TILE) && P >= 0 && P <= (1 << 28));
  if (P == 0) return NSID_OK;
  NSID_REQUIRE(q && kv && qi && ci && obar && attn && abar && nsid_aligned16(q) && nsid_aligned16(kv));
  nsid_count(wide ? NSID_C_clf_attn_fwd_n : NSID_C_clf_attn_fwd);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (wide) {      // a workgroup per pair
    CLF_LAUNCH_C(C, clf_attn_fwd_wide_kernel, dim3(P), dim3(256), st, q, nq_seg, kv, nc_seg, N, qi, ci, P, obar, attn, abar);
  } else {         // a wave per pair
    CLF_LAUNCH_C(C, clf_attn_fwd_kernel, dim3((P + 3) / 4), dim3(256), st, q, nq_seg, kv, nc_seg, N, qi, ci, P, obar, attn, abar);
  }
  return nsid_launch_status();
}

int launch_attn_bwd(bool wide, const float* dobar, const float* attn, const float* q, int nq_seg, const float* kv, int nc_seg, int C,
                    int N, const int* qi, const int* ci, int P, float* dq, float* dk, void* stream) {
  NSID_REQUIRE(clf_width_ok(C));
  NSID_REQUIRE(nq_seg >= 1 && nc_seg >= 1 && N >= 1 && N <= (wide ? CLF_MAX_NODES : CLF_TILE) && P >= 0 && P <= (1 << 28));
  if (P == 0) return NSID_OK;
  NSID_REQUIRE(dobar && attn && q && kv && qi && ci && dq && dk && nsid_aligned16(dobar) && nsid_aligned16(kv));
  nsid_count(wide ? NSID_C_clf_attn_bwd_n : NSID_C_clf_attn_bwd);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (wide) {      // a workgroup per (pair, head)
    CLF_LAUNCH_C(C, clf_attn_bwd_wide_kernel, dim3(4u * (unsigned)P), dim3(256), st, dobar, attn, q, nq_seg, kv, nc_seg, N, qi, ci, P,
                 dq, dk);
  } else {         // a wave per pair
    CLF_LAUNCH_C(C, clf_attn_bwd_kernel, dim3((P + 3) / 4), dim3(256), st, dobar, attn, q, nq_seg, kv, nc_seg, N, qi, ci, P, dq, dk);
  }
  return nsid_launch_status();
}

int launch_seg_reduce(bool wide, const float* dq, const float* dk, const float* abar, const float* dobar, const int* qi, const int* ci,
                      int P, int C, int N, int nq_seg, int nc_seg, float* dq_seg, float* dkv_seg, void* stream) {
  NSID_REQUIRE(clf_width_ok(C));
  NSID_REQUIRE(P >= 0 && P <= (1 << 28) && N >= 1 && N <= (wide ? CLF_MAX_NODES : CLF_TILE) && nq_seg >= 0 && nc_seg >= 0 &&
               nq_seg + nc_seg <= (1 << 30));
  if (nq_seg + nc_seg == 0) return NSID_OK;
  NSID_REQUIRE((P == 0 || (dq && dk && abar && dobar && qi && ci)) && dq_seg && dkv_seg);
  NSID_REQUIRE(nsid_aligned16(dq) && nsid_aligned16(dk) && nsid_aligned16(dobar) && nsid_aligned16(dq_seg) && nsid_aligned16(dkv_seg));
  nsid_count(wide ? NSID_C_clf_seg_reduce_n : NSID_C_clf_seg_reduce);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (wide) {      // a workgroup per (segment, node tile)
    CLF_LAUNCH_C(C, clf_seg_reduce_wide_kernel, dim3(nq_seg + nc_seg, (N + CLF_TILE - 1) / CLF_TILE), dim3(CT_RED_THREADS), st, dq, dk,
                 abar, dobar, qi, ci, P, N, nq_seg, dq_seg, dkv_seg);
  } else {         // a workgroup per segment
    CLF_LAUNCH_C(C, clf_seg_reduce_kernel, dim3(nq_seg + nc_seg), dim3(CT_RED_THREADS), st, dq, dk, abar, dobar, qi, ci, P, N, nq_seg,
                 dq_seg, dkv_seg);
  }
  return nsid_launch_status();
}

}  // namespace

extern "C" int nsid_clf_mine_hard_negatives(const float* zq, int nq, const float* za, int na, int d, int k, int64_t* out,
                                            void* stream) {
  NSID_REQUIRE(nq >= 0 && na >= 1 && na <= CT_MINE_MAXN && d >= 4 && d <= CT_MINE_MAXD && d % 4 == 0 && k >= 1 && k <= na - 1);
  if (nq == 0) return NSID_OK;
  NSID_REQUIRE(zq && za && out && nsid_aligned16(za));
  nsid_count(NSID_C_clf_mine);
  NSID_LAUNCH(clf_mine_kernel, dim3(nq), dim3(256), 0, static_cast<hipStream_t>(stream), zq, za, na, d, k, out);
  return nsid_launch_status();
}

extern "C" int nsid_clf_head_fwd(const float* hid, const float* keep, const float* w2, const float* b2, int P, float* s, void* stream) {
  NSID_REQUIRE(P >= 0 && P <= (1 << 28));
  if (P == 0) return NSID_OK;
  NSID_REQUIRE(hid && keep && w2 && b2 && s);
  nsid_count(NSID_C_clf_head_fwd);
  NSID_LAUNCH(clf_head_fwd_kernel, dim3((P + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), hid, keep, w2, b2, P, s);
  return nsid_launch_status();
}

extern "C" int nsid_clf_head_bwd(const float* ds, const float* s, const float* hid, const float* keep, const float* w2, int P,
                                 float* dh, float* dz, float* dw2, float* db2, void* stream) {
  NSID_REQUIRE(P >= 0 && P <= (1 << 28));
  NSID_REQUIRE(ds && s && hid && keep && w2 && dh && dz && dw2 && db2);
  nsid_count(NSID_C_clf_head_bwd);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (P > 0) {
    NSID_LAUNCH(clf_head_bwd_kernel, dim3((P + 3) / 4), dim3(256), 0, st, ds, s, hid, keep, w2, P, dh, dz);
    if (nsid_launch_status() != NSID_OK) return NSID_ELAUNCH;
  }
  NSID_LAUNCH(clf_head_wgrad_kernel, dim3(1), dim3(CT_WG_GROUPS * CLF_HID), 0, st, dz, hid, keep, P, dw2, db2);
  return nsid_launch_status();
}

// ---- the attention and the per-segment sums: _c at N <= 32, _n at 1 <= N <= 128 (the multi-tile kernels), the plain names at C = 512
extern "C" int nsid_clf_attn_fwd_c(const float* q, int nq_seg, const float* kv, int nc_seg, int C, int N, const int* qi, const int* ci,
                                   int P, float* obar, float* attn, float* abar, void* stream) {
  return launch_attn_fwd(false, q, nq_seg, kv, nc_seg, C, N, qi, ci, P, obar, attn, abar, stream);
}

extern "C" int nsid_clf_attn_fwd_n(const float* q, int nq_seg, const float* kv, int nc_seg, int C, int N, const int* qi, const int* ci,
                                   int P, float* obar, float* attn, float* abar, void* stream) {
  return launch_attn_fwd(true, q, nq_seg, kv, nc_seg, C, N, qi, ci, P, obar, attn, abar, stream);
}

extern "C" int nsid_clf_attn_fwd(const float* q, int nq_seg, const float* kv, int nc_seg, int N, const int* qi, const int* ci,
                                 int P, float* obar, float* attn, float* abar, void* stream) {
  return launch_attn_fwd(false, q, nq_seg, kv, nc_seg, NSID_CLF_C, N, qi, ci, P, obar, attn, abar, stream);
}

extern "C" int nsid_clf_attn_bwd_c(const float* dobar, const float* attn, const float* q, int nq_seg, const float* kv, int nc_seg,
                                   int C, int N, const int* qi, const int* ci, int P, float* dq, float* dk, void* stream) {
  return launch_attn_bwd(false, dobar, attn, q, nq_seg, kv, nc_seg, C, N, qi, ci, P, dq, dk, stream);
}

extern "C" int nsid_clf_attn_bwd_n(const float* dobar, const float* attn, const float* q, int nq_seg, const float* kv, int nc_seg,
                                   int C, int N, const int* qi, const int* ci, int P, float* dq, float* dk, void* stream) {
  return launch_attn_bwd(true, dobar, attn, q, nq_seg, kv, nc_seg, C, N, qi, ci, P, dq, dk, stream);
}

extern "C" int nsid_clf_attn_bwd(const float* dobar, const float* attn, const float* q, int nq_seg, const float* kv, int nc_seg,
                                 int N, const int* qi, const int* ci, int P, float* dq, float* dk, void* stream) {
  return launch_attn_bwd(false, dobar, attn, q, nq_seg, kv, nc_seg, NSID_CLF_C, N, qi, ci, P, dq, dk, stream);
}

extern "C" int nsid_clf_seg_reduce_c(const float* dq, const float* dk, const float* abar, const float* dobar, const int* qi,
                                     const int* ci, int P, int C, int N, int nq_seg, int nc_seg, float* dq_seg, float* dkv_seg,
                                     void* stream) {
  return launch_seg_reduce(false, dq, dk, abar, dobar, qi, ci, P, C, N, nq_seg, nc_seg, dq_seg, dkv_seg, stream);
}

extern "C" int nsid_clf_seg_reduce_n(const float* dq, const float* dk, const float* abar, const float* dobar, const int* qi,
                                     const int* ci, int P, int C, int N, int nq_seg, int nc_seg, float* dq_seg, float* dkv_seg,
                                     void* stream) {
  return launch_seg_reduce(true, dq, dk, abar, dobar, qi, ci, P, C, N, nq_seg, nc_seg, dq_seg, dkv_seg, stream);
}

extern "C" int nsid_clf_seg_reduce(const float* dq, const float* dk, const float* abar, const float* dobar, const int* qi,
                                   const int* ci, int P, int N, int nq_seg, int nc_seg, float* dq_seg, float* dkv_seg,
                                   void* stream) {
  return launch_seg_reduce(false, dq, dk, abar, dobar, qi, ci, P, NSID_CLF_C, N, nq_seg, nc_seg, dq_seg, dkv_seg, stream);
}
