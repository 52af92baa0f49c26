// Training objective of the ResNet-IBN baseline (simclr/triplet.py:6-61, baseline/train.py:64-77): pair cross-entropy and the
// semi-hard triplet loss, forward and backward, for embeddings of up to 2048 features and up to 2048 rows; and the step objective of a
// data-parallel rank (nsid_baseline_objective_rows_fwd_bwd): the forward over the gathered global batch of up to 4096 rows, the
// backward for the pairs the rank owns.
//
//   bl_normalize_kernel : zn = z / max(|z|, 1e-12) per row (the step's second F.normalize), |z| kept for its backward
//   bl_sim_kernel       : S = E E^T in exact fp32 on v_mfma_f32_16x16x4_f32, 64 x 64 tiles, K loop over D; S is MATERIALISED
//                         (Mp x Mp, Mp = M rounded up to 64: <= 16 MB, resident in L2 / Infinity Cache). blockIdx.z picks one of two
//                         operand sets: the objective needs S of the raw rows (cross-entropy) and of the re-normalised rows (triplet).
//   bl_rows_kernel      : one wave per row of S: masked log-sum-exp + target pick; row max over the positives, thresholded row min
//                         over the negatives, both with the FIRST index on exact ties (torch.max / torch.min on a row); the values of
//                         the chosen pairs are then recomputed in double
//   bl_finish_kernel    : the means, the count of valid anchors, beta / gamma and the weight of the triplet backward, on the device
//   bl_ce_bwd_kernel    : dz = (beta / M) Q z, Q_ab = exp(S_ab - lse_a) + exp(S_ab - lse_b) - 2 [b == a +- B]: the second MFMA product,
//                         Q tiles built from S on the way into LDS
//   bl_trip_bwd_kernel  : the sparse backward without floating-point atomics: output row i adds its own anchor's term, then the
//                         terms of the anchors that chose it, found by a scan of the two index arrays and visited in ascending order
//                         (bitwise reproducible); with `norm` it also applies the backward of the normalisation
// Both backward kernels write the output rows an `Owned` names. Every output row sums over ALL M columns / anchors in ascending
// order whatever the owned range is, so a row's gradient does not depend on how the batch is sharded, bit for bit.
#include "nsid_common.h"

namespace {

constexpr int TB = 64;          // tile edge of both MFMA products
constexpr int LDT = TB + 4;     // LDS row stride (floats): 16-byte aligned rows, rows 4 apart land on different banks
constexpr int BL_MAX = NSID_BL_MAX;    // rows and features
constexpr int BL_ROWS_MAX = NSID_BL_ROWS_MAX;   // rows of the gathered batch of the sharded objective

// rows [0, split) of the row matrix live at a, the rest at b (the two views); a single matrix has split = M
struct RowSet {
  const float* a;
  const float* b;
  int split;
};
__device__ __forceinline__ const float* row_of(const RowSet& R, int r, int D) {
  return r < R.split ? R.a + (long)r * D : R.b + (long)(r - R.split) * D;
}
__device__ __forceinline__ float* row_of(float* a, float* b, int split, int r, int D) {
  return r < split ? a + (long)r * D : b + (long)(r - split) * D;
}

// The output rows of a backward launch: o in [0, rows) is row (o < n ? p0 + o : B + p0 + o - n) of the row matrix, i.e. pairs
// [p0, p0 + n) of both views, and is written to row o of (d_a | d_b) split at n. The unsharded entries own every row: p0 = 0,
// n = the split of their row matrix, rows = M.
struct Owned {
  int p0, n, B, rows;
};
__device__ __forceinline__ int owned_row(const Owned& O, int o) { return o < O.n ? O.p0 + o : O.B + O.p0 + (o - O.n); }

// deterministic sum over the 256 threads of a workgroup (red: 4 floats of LDS); every thread receives it
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void bl_normalize_kernel(RowSet R, int D, float* __restrict__ zn, float* __restrict__ norm) {
  __shared__ double red[4];
  const int r = blockIdx.x;
  const float* src = row_of(R, r, D);
  f32x4 v[2];
  double ss = 0.0;                               // the norm in double: its error would scale a whole row of similarities
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = 4 * ((int)threadIdx.x + 256 * u);
    v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < D) v[u] = ld4(src + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += (double)v[u][e] * (double)v[u][e];
  }
  const double n = fmax(sqrt(block_sum_d(ss, red)), 1e-12);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int c = 4 * ((int)threadIdx.x + 256 * u);
    if (c < D)
      *reinterpret_cast<f32x4*>(zn + (long)r * D + c) =
          f32x4{(float)(v[u][0] / n), (float)(v[u][1] / n), (float)(v[u][2] / n), (float)(v[u][3] / n)};
  }
  if (threadIdx.x == 0) norm[r] = (float)n;
}

// S[i][j] = E_i . E_j for the 64 x 64 tile (blockIdx.y, blockIdx.x); rows past M are read as zeros, so all of Mp x Mp is written
__global__ __launch_bounds__(256) void bl_sim_kernel(RowSet R0, RowSet R1, int M, int Mp, int D, float* __restrict__ S0,
                                                     float* __restrict__ S1) {
  __shared__ __attribute__((aligned(16))) float As[TB * LDT];
  __shared__ __attribute__((aligned(16))) float Bs[TB * LDT];
  const RowSet R = blockIdx.z ? R1 : R0;
  float* S = blockIdx.z ? S1 : S0;
  const int i0 = blockIdx.y * TB, j0 = blockIdx.x * TB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, rq = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < D; k0 += TB) {
    const int kw = min(TB, D - k0);            // a multiple of 16
    f32x4 va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = threadIdx.x + 256 * u, rr = q >> 4, c = (q & 15) * 4;
      va[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      vb[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < kw) {
        if (i0 + rr < M) va[u] = ld4(row_of(R, i0 + rr, D) + k0 + c);
        if (j0 + rr < M) vb[u] = ld4(row_of(R, j0 + rr, D) + k0 + c);
      }
    }
    __syncthreads();                           // the previous chunk has been consumed
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = threadIdx.x + 256 * u, rr = q >> 4, c = (q & 15) * 4;
      *reinterpret_cast<f32x4*>(As + rr * LDT + c) = va[u];
      *reinterpret_cast<f32x4*>(Bs + rr * LDT + c) = vb[u];
    }
    __syncthreads();
    // A operand: row i = 16 * wave + lr, B operand: row j = 16 * u + lr; reduction index (rq, e) on both
    const float* pa = As + (16 * wave + lr) * LDT + 4 * rq;
    const float* pb = Bs + lr * LDT + 4 * rq;
    for (int ch = 0; ch < kw; ch += 16) {
      const f32x4 fa = ld4(pa + ch);
      f32x4 fb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) fb[u] = ld4(pb + 16 * u * LDT + ch);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[e], fb[u][e], acc[u], 0, 0, 0);
    }
  }
  // C/D layout: row 4 * rq + e of the wave's 16 rows, column lr of tile u
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) S[(long)(i0 + 16 * wave + 4 * rq + e) * Mp + j0 + 16 * u + lr] = acc[u][e];
}

// (value, index) reductions over a wave: the larger / smaller value wins, the smaller index on equal values
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
  }
}
__device__ __forceinline__ void wave_argmin(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (v2 < v || (v2 == v && i2 < i)) { v = v2; i = i2; }
  }
}

constexpr int NO_INDEX = 0x7fffffff;
constexpr int F_VALID = 1, F_ACTIVE = 2;

// labels == nullptr: the step's labels cat(arange(B), arange(B))
__device__ __forceinline__ long label_of(const long long* labels, int r, int B) {
  return labels ? (long)labels[r] : (long)(r < B ? r : r - B);
}

// E_a . E_b in double over the lanes of a wave (every lane receives it)
__device__ __forceinline__ double wave_dot_d(const float* __restrict__ x, const float* __restrict__ y, int D, int lane) {
  double s = 0.0;
  for (int k = 4 * lane; k < D; k += 256) {
    const f32x4 a = ld4(x + k), b = ld4(y + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)a[e] * (double)b[e];
  }
  return wave_sum_d(s);
}

// The DECISIONS are taken on the fp32 similarities, as the reference takes them. The VALUES that enter the means are then formed in
// double: the log-sum-exp of a row, and pos / neg of an anchor as two dot products of the chosen rows (2 M dot products in all), so
// the losses carry no more than the final rounding to fp32.
__global__ __launch_bounds__(256) void bl_rows_kernel(const float* __restrict__ Sc, const float* __restrict__ St, RowSet E, int D,
                                                      const long long* __restrict__ labels, int M, int Mp, int B, float margin_f,
                                                      double margin, float* __restrict__ lse, double* __restrict__ rowloss,
                                                      double* __restrict__ hinge, int* __restrict__ pidx, int* __restrict__ nidx,
                                                      int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= M) return;                            // wave-uniform; no barrier below
  const float inf = __builtin_inff();
  if (Sc != nullptr) {                           // cross-entropy of row a against its target (a + B) mod M, diagonal masked
    const float* s = Sc + (long)a * Mp;
    float m = -inf;
    for (int b = lane; b < M; b += 64)
      if (b != a) m = fmaxf(m, s[b]);
    m = wave_max(m);
    double sum = 0.0;
    for (int b = lane; b < M; b += 64)
      if (b != a) sum += exp((double)s[b] - (double)m);
    sum = wave_sum_d(sum);
    const double l = (double)m + log(sum);
    if (lane == 0) {
      lse[a] = (float)l;
      rowloss[a] = l - (double)s[a + B < M ? a + B : a + B - M];
    }
  }
  if (St != nullptr) {
    const float* s = St + (long)a * Mp;
    const long la = label_of(labels, a, B);
    float pos = -inf;
    int pi = NO_INDEX;
    for (int b = lane; b < M; b += 64) {         // ascending b: a lane keeps the first index of its maximum
      const float v = s[b];
      if (b != a && label_of(labels, b, B) == la && (v > pos || pi == NO_INDEX)) { pos = v; pi = b; }
    }
    wave_argmax(pos, pi);
    const float thr = pos - margin_f;            // -inf without a positive: every negative is semi-hard
    float neg = inf;
    int ni = NO_INDEX;
    for (int b = lane; b < M; b += 64) {
      const float v = s[b];
      if (label_of(labels, b, B) != la && v > thr && v < neg) { neg = v; ni = b; }
    }
    wave_argmin(neg, ni);
    const bool valid = ni != NO_INDEX;
    double h = 0.0;
    if (valid && pi != NO_INDEX) {                // wave-uniform
      const float* ea = row_of(E, a, D);
      h = wave_dot_d(ea, row_of(E, pi, D), D, lane) - wave_dot_d(ea, row_of(E, ni, D), D, lane) + margin;
    }
    if (lane == 0) {
      hinge[a] = h > 0.0 ? h : 0.0;
      pidx[a] = pi == NO_INDEX ? -1 : pi;
      nidx[a] = valid ? ni : -1;
      flags[a] = (valid ? F_VALID : 0) | (h > 0.0 ? F_ACTIVE : 0);
    }
  }
}

// res[0] = beta * cls + gamma * trip, res[1] = cls, res[2] = trip, res[3] = n_valid, res[4] = gamma / n_valid (0 without a valid
// anchor): the weight of every active anchor in the triplet backward
__global__ __launch_bounds__(256) void bl_finish_kernel(const double* __restrict__ rowloss, const double* __restrict__ hinge,
                                                        const int* __restrict__ flags, int M, int do_cls, int do_trip, double beta,
                                                        double gamma, float* __restrict__ res, float* __restrict__ o_loss,
                                                        float* __restrict__ o_cls, float* __restrict__ o_trip,
                                                        float* __restrict__ o_nv) {
  __shared__ double red[3][4];
  double c = 0.0, t = 0.0, n = 0.0;
  for (int i = threadIdx.x; i < M; i += blockDim.x) {
    if (do_cls) c += rowloss[i];
    if (do_trip) {
      t += hinge[i];
      n += (double)(flags[i] & F_VALID);
    }
  }
  c = wave_sum_d(c);
  t = wave_sum_d(t);
  n = wave_sum_d(n);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = c; red[1][threadIdx.x >> 6] = t; red[2][threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    c = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    t = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    n = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    c = do_cls ? c / (double)M : 0.0;
    t = n > 0.0 ? t / n : 0.0;
    const float cls = (float)c, trip = (float)t;
    const float loss = (float)((do_cls ? beta * c : 0.0) + (do_trip ? gamma * t : 0.0));     // one rounding, of the double sum
    res[0] = loss; res[1] = cls; res[2] = trip; res[3] = (float)n;
    res[4] = n > 0.0 ? (float)(gamma / n) : 0.f;
    if (o_loss) o_loss[0] = loss;
    if (o_cls) o_cls[0] = cls;
    if (o_trip) o_trip[0] = trip;
    if (o_nv) o_nv[0] = (float)n;
  }
}

// dz[o][c] = scale * sum_j Q_ij z[j][c], i = owned_row(o), for the tile of 64 owned rows o (blockIdx.y) and 64 features c
// (blockIdx.x); the tile may straddle the two owned ranges or end short of 64 rows. The sum over j runs on two levels: the 64
// columns of a tile in the fp32 MFMA accumulator, the tiles in double. One fp32 accumulator over all M columns sits at M times the
// result's magnitude for M / 4 roundings: at M = 4096 that alone is 6 x the distance of the reference's own fp32 run from fp64.
__global__ __launch_bounds__(256) void bl_ce_bwd_kernel(RowSet R, const float* __restrict__ S, const float* __restrict__ lse, int M,
                                                        int Mp, int D, int B, Owned O, double scale, float* __restrict__ dz_a,
                                                        float* __restrict__ dz_b) {
  __shared__ __attribute__((aligned(16))) float Qs[TB * LDT];
  __shared__ __attribute__((aligned(16))) float Zs[TB * LDT];
  const int i0 = blockIdx.y * TB, c0 = blockIdx.x * TB;
  const int cw = min(TB, D - c0);              // a multiple of 16
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, rq = lane >> 4;
  double tot[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) tot[u][e] = 0.0;
  float lse_i[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = i0 + (((int)threadIdx.x + 256 * u) >> 4);
    lse_i[u] = o < O.rows ? lse[owned_row(O, o)] : 0.f;
  }
  for (int j0 = 0; j0 < M; j0 += TB) {
    f32x4 vq[4], vz[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = threadIdx.x + 256 * u, rr = q >> 4, c = (q & 15) * 4;
      const bool own = i0 + rr < O.rows;
      const int i = own ? owned_row(O, i0 + rr) : 0;           // (a tile row past the owned ones reads row 0 and contributes zeros)
      const f32x4 s = ld4(S + (long)i * Mp + j0 + c);          // inside Mp x Mp
      const f32x4 lj = ld4(lse + j0 + c);                      // inside lse[Mp]; entries past M are not used
      const int tgt = i + B < M ? i + B : i + B - M;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + c + e;
        float v = 0.f;
        if (own && j < M && j != i) v = expf(s[e] - lse_i[u]) + expf(s[e] - lj[e]) - (j == tgt ? 2.f : 0.f);
        vq[u][e] = v;
      }
      vz[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j0 + rr < M && c < cw) vz[u] = ld4(row_of(R, j0 + rr, D) + c0 + c);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = threadIdx.x + 256 * u, rr = q >> 4, c = (q & 15) * 4;
      *reinterpret_cast<f32x4*>(Qs + rr * LDT + c) = vq[u];
      *reinterpret_cast<f32x4*>(Zs + rr * LDT + c) = vz[u];
    }
    __syncthreads();
    // A = Q (row i = 16 * wave + lr, reduction (rq, e) <-> j = jj + 4 * rq + e), B = z[j][16 * u + lr]
    const float* pa = Qs + (16 * wave + lr) * LDT + 4 * rq;
    const float* pb = Zs + 4 * rq * LDT + lr;
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < TB; jj += 16) {
      const f32x4 fa = ld4(pa + jj);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[e], pb[(jj + e) * LDT + 16 * u], acc[u], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[u][e] += (double)acc[u][e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int o = i0 + 16 * wave + 4 * rq + e;
    if (o >= O.rows) continue;
    float* dst = row_of(dz_a, dz_b, O.n, o, D) + c0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (16 * u + lr < cw) dst[16 * u + lr] = (float)(tot[u][e] * scale);
  }
}

// Output row o of the triplet backward, i = owned_row(o): g = w [ (E[p_i] - E[n_i]) [i active] + sum_{a active, p_a = i} E[a] - sum_{a active, n_a = i} E[a] ].
// norm != nullptr: E = zn and the result is taken through the normalisation: (g - zn_i (zn_i . g)) / norm_i.
// accumulate: added to what the cross-entropy backward left in the row (one owner per row: no atomics).
__global__ __launch_bounds__(256) void bl_trip_bwd_kernel(RowSet E, int M, int D, const int* __restrict__ pidx,
                                                          const int* __restrict__ nidx, const int* __restrict__ flags,
                                                          const float* __restrict__ res, const float* __restrict__ norm,
                                                          int accumulate, Owned O, float* __restrict__ d_a,
                                                          float* __restrict__ d_b) {
  __shared__ unsigned hit_p[BL_ROWS_MAX / 32], hit_n[BL_ROWS_MAX / 32];
  __shared__ float red[4];
  const int i = owned_row(O, blockIdx.x);
  if (threadIdx.x < BL_ROWS_MAX / 32) { hit_p[threadIdx.x] = 0u; hit_n[threadIdx.x] = 0u; }
  __syncthreads();
  for (int a = threadIdx.x; a < M; a += blockDim.x) {
    if (flags[a] & F_ACTIVE) {                   // integer OR: the bitmaps do not depend on the order of arrival
      if (pidx[a] == i) atomicOr(&hit_p[a >> 5], 1u << (a & 31));
      if (nidx[a] == i) atomicOr(&hit_n[a >> 5], 1u << (a & 31));
    }
  }
  __syncthreads();
  const int c[2] = {4 * (int)threadIdx.x, 4 * ((int)threadIdx.x + 256)};
  f32x4 g[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (flags[i] & F_ACTIVE) {
    const float* ep = row_of(E, pidx[i], D);
    const float* en = row_of(E, nidx[i], D);
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (c[u] < D) g[u] = ld4(ep + c[u]) - ld4(en + c[u]);
  }
  const int words = (M + 31) >> 5;
  for (int w = 0; w < words; ++w) {              // uniform control flow: every thread reads the same words
    for (unsigned m = hit_p[w]; m != 0u; m &= m - 1u) {
      const float* ea = row_of(E, 32 * w + __builtin_ctz(m), D);
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (c[u] < D) g[u] += ld4(ea + c[u]);
    }
  }
  for (int w = 0; w < words; ++w) {
    for (unsigned m = hit_n[w]; m != 0u; m &= m - 1u) {
      const float* ea = row_of(E, 32 * w + __builtin_ctz(m), D);
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (c[u] < D) g[u] -= ld4(ea + c[u]);
    }
  }
  const float wgt = res[4];
  g[0] *= wgt;
  g[1] *= wgt;
  if (norm != nullptr) {
    const float* zi = row_of(E, i, D);
    f32x4 z[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    float dot = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (c[u] < D) z[u] = ld4(zi + c[u]);
      dot += (g[u][0] * z[u][0] + g[u][1] * z[u][1]) + (g[u][2] * z[u][2] + g[u][3] * z[u][3]);
    }
    dot = block_sum(dot, red);
    const float n = norm[i];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) g[u][e] = (g[u][e] - z[u][e] * dot) / n;
  }
  float* dst = row_of(d_a, d_b, O.n, (int)blockIdx.x, D);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (c[u] >= D) continue;
    f32x4 o = g[u];
    if (accumulate) o += ld4(dst + c[u]);
    *reinterpret_cast<f32x4*>(dst + c[u]) = o;
  }
}

// ---- workspace (floats): [lse | pidx | nidx | flags | norm] of Mp entries each, [rowloss | hinge] of Mp doubles each, 64 result
// floats, S0, S1 (Mp x Mp), zn (Mp x D)
struct Workspace {
  float *lse, *norm, *res, *S0, *S1, *zn;
  double *rowloss, *hinge;
  int *pidx, *nidx, *flags;
  int Mp;
};
inline int padded(int M) { return (M + TB - 1) / TB * TB; }
inline Workspace carve(float* ws, int M) {
  Workspace w;
  const long Mp = padded(M);
  w.Mp = (int)Mp;
  w.lse = ws;
  w.pidx = reinterpret_cast<int*>(ws + Mp);
  w.nidx = reinterpret_cast<int*>(ws + 2 * Mp);
  w.flags = reinterpret_cast<int*>(ws + 3 * Mp);
  w.norm = ws + 4 * Mp;
  w.rowloss = reinterpret_cast<double*>(ws + 5 * Mp);
  w.hinge = reinterpret_cast<double*>(ws + 7 * Mp);
  w.res = ws + 9 * Mp;
  w.S0 = ws + 9 * Mp + 64;
  w.S1 = w.S0 + Mp * Mp;
  w.zn = w.S1 + Mp * Mp;
  return w;
}

// cls: rows (z_a | z_b) of the cross-entropy; trip: rows of the triplet loss (renorm: the normalised cls rows, made here);
// own: the rows whose gradient goes to (d_a | d_b). The forward always covers all M rows.
int run(const float* z_a, const float* z_b, int split, const long long* labels, int M, int D, int B, double margin, double beta,
        double gamma, bool do_cls, bool do_trip, bool renorm, float* ws, float* o_loss, float* o_cls, float* o_trip, float* o_nv,
        float* d_a, float* d_b, Owned own, hipStream_t s) {
  const Workspace w = carve(ws, M);
  const int Mp = w.Mp, tiles = Mp / TB;
  const RowSet raw{z_a, z_b, split};
  RowSet trip = raw;
  if (renorm) {
    NSID_LAUNCH(bl_normalize_kernel, dim3(M), dim3(256), 0, s, raw, D, w.zn, w.norm);
    trip = RowSet{w.zn, w.zn, M};
  }
  const bool two = do_cls && do_trip;
  float* St = two ? w.S1 : w.S0;
  NSID_LAUNCH(bl_sim_kernel, dim3(tiles, tiles, two ? 2 : 1), dim3(256), 0, s, do_cls ? raw : trip, trip, M, Mp, D, w.S0, w.S1);
  NSID_LAUNCH(bl_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, s, do_cls ? w.S0 : nullptr, do_trip ? St : nullptr, trip, D, labels, M,
              Mp, B, (float)margin, margin, w.lse, w.rowloss, w.hinge, w.pidx, w.nidx, w.flags);
  NSID_LAUNCH(bl_finish_kernel, dim3(1), dim3(256), 0, s, w.rowloss, w.hinge, w.flags, M, (int)do_cls, (int)do_trip, beta, gamma,
              w.res, o_loss, o_cls, o_trip, o_nv);
  if (d_a != nullptr) {
    if (do_cls)
      NSID_LAUNCH(bl_ce_bwd_kernel, dim3((D + TB - 1) / TB, (own.rows + TB - 1) / TB), dim3(256), 0, s, raw, w.S0, w.lse, M, Mp, D, B,
                  own, beta / M, d_a, d_b);
    if (do_trip)
      NSID_LAUNCH(bl_trip_bwd_kernel, dim3(own.rows), dim3(256), 0, s, trip, M, D, w.pidx, w.nidx, w.flags, w.res,
                  renorm ? w.norm : nullptr, (int)do_cls, own, d_a, d_b);
  }
  return nsid_launch_status();
}

inline bool shape_ok(int M, int D) { return D % 16 == 0 && D >= 16 && D <= BL_MAX && M >= 1 && M <= BL_MAX; }

}  // namespace

extern "C" size_t nsid_baseline_loss_ws_floats(int M, int D) {
  if (M < 1 || D < 1) return 0;
  const size_t Mp = (size_t)padded(M);
  return 9 * Mp + 64 + 2 * Mp * Mp + Mp * (size_t)D;
}

extern "C" int nsid_pair_ce_fwd_bwd(const float* z_i, const float* z_j, int B, int D, float* ws, float* out, float* dz_i,
                                    float* dz_j, void* stream) {
  NSID_REQUIRE(z_i && z_j && ws && out && B >= 1 && shape_ok(2 * B, D));
  NSID_REQUIRE(nsid_aligned16(z_i) && nsid_aligned16(z_j) && nsid_aligned16(ws) && nsid_aligned16(dz_i) && nsid_aligned16(dz_j));
  NSID_REQUIRE((dz_i == nullptr) == (dz_j == nullptr));
  nsid_count(NSID_C_pair_ce);
  return run(z_i, z_j, B, nullptr, 2 * B, D, B, 0.0, 1.0, 0.0, true, false, false, ws, out, nullptr, nullptr, nullptr, dz_i, dz_j,
             Owned{0, B, B, 2 * B}, static_cast<hipStream_t>(stream));
}

extern "C" int nsid_triplet_fwd_bwd(const float* e, const int64_t* labels, int M, int D, double margin, float* ws, float* out,
                                    float* de, void* stream) {
  NSID_REQUIRE(e && labels && ws && out && shape_ok(M, D));
  NSID_REQUIRE(nsid_aligned16(e) && nsid_aligned16(ws) && nsid_aligned16(de));
  nsid_count(NSID_C_triplet);
  return run(e, e, M, reinterpret_cast<const long long*>(labels), M, D, M, margin, 0.0, 1.0, false, true, false, ws, out, nullptr,
             nullptr, out + 1, de, de, Owned{0, M, M, M}, static_cast<hipStream_t>(stream));
}

extern "C" int nsid_baseline_objective_fwd_bwd(const float* z_i, const float* z_j, int B, int D, double margin, double beta,
                                               double gamma, float* ws, float* out, float* dz_i, float* dz_j, void* stream) {
  NSID_REQUIRE(z_i && z_j && ws && out && B >= 1 && shape_ok(2 * B, D));
  NSID_REQUIRE(nsid_aligned16(z_i) && nsid_aligned16(z_j) && nsid_aligned16(ws) && nsid_aligned16(dz_i) && nsid_aligned16(dz_j));
  NSID_REQUIRE((dz_i == nullptr) == (dz_j == nullptr));
  nsid_count(NSID_C_baseline_objective);
  return run(z_i, z_j, B, nullptr, 2 * B, D, B, margin, beta, gamma, true, true, true, ws, out, out + 1, out + 2, out + 3, dz_i,
             dz_j, Owned{0, B, B, 2 * B}, static_cast<hipStream_t>(stream));
}

// The sharded form keeps both similarity matrices whole (the forward needs every row of both): the layout of the unsharded workspace.
extern "C" size_t nsid_baseline_loss_rows_ws_floats(int M, int D) { return nsid_baseline_loss_ws_floats(M, D); }

extern "C" int nsid_baseline_objective_rows_fwd_bwd(const float* z_i_all, const float* z_j_all, int Bg, int D, int p0, int npairs,
                                                    double margin, double beta, double gamma, float* ws, float* out, float* dz_i,
                                                    float* dz_j, void* stream) {
  NSID_REQUIRE(z_i_all && z_j_all && ws && out && Bg >= 1 && Bg <= BL_ROWS_MAX / 2 && D % 16 == 0 && D >= 16 && D <= BL_MAX);
  NSID_REQUIRE(p0 >= 0 && npairs >= 1 && npairs <= Bg && p0 <= Bg - npairs);
  NSID_REQUIRE(nsid_aligned16(z_i_all) && nsid_aligned16(z_j_all) && nsid_aligned16(ws) && nsid_aligned16(dz_i) &&
               nsid_aligned16(dz_j));
  NSID_REQUIRE((dz_i == nullptr) == (dz_j == nullptr));
  nsid_count(NSID_C_baseline_objective_rows);
  return run(z_i_all, z_j_all, Bg, nullptr, 2 * Bg, D, Bg, margin, beta, gamma, true, true, true, ws, out, out + 1, out + 2, out + 3,
             dz_i, dz_j, Owned{p0, npairs, Bg, 2 * npairs}, static_cast<hipStream_t>(stream));
}
