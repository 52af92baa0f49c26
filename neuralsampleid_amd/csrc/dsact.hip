// The Downsample chain of the DGL-variant encoder (encoder/dgl/graph_encoder.py, reference :8-31 and :120-127): three
// Conv1d(k = 3, stride 2, pad 1) + BatchNorm1d + ReLU layers in a row, the first behind the stem's BatchNorm2d + LeakyReLU.
// Every layer keeps only its RAW conv output r (node-major rows, fp32 or bf16 storage); the BatchNorm + activation of the
// layer in front is applied by the next layer's operand load (prologue), as in csrc/gemm.hip.
//
// The conv is a GEMM over a zero-padded strided view of the input, with no im2col matrix (reduction index kk = t*C + c):
//   out[b*No + n][o] = bias[o] + sum_{t, c} w[o][c][t] * act(sc[c] * x[b*N + 2n-1+t][c] + sh[c])
// Row 2n-1+t outside [0, N) is the conv's zero padding. The conv pads the ACTIVATED tensor, so such an operand is exactly 0:
// the prologue is never applied to it (act(sc*0 + sh) = relu(sh) is not 0 in general).
//
//   dsact_fwd_kernel   : the forward (bias + training BatchNorm partial statistics of 128-row tiles, or the eval-mode BatchNorm
//                        folded into an affine + activation in the epilogue). No atomics: bitwise reproducible.
//   dsact_wgrad_kernel : dw[o][c][t] += sum_m dr[m][o] * act(sc*x + sh)[view], fp32 atomics over row splits.
//   dsact_dgrad_kernel : dy[2q] = dr[q] . W_1, dy[2q+1] = dr[q] . W_2 + dr[q+1] . W_0 (two row parities of one launch), times the
//                        activation derivative of the layer in front (recomputed from its r, sc, sh), plus that layer's
//                        BatchNorm-backward column sums (sum g, sum g * xhat) per 128-row tile: no separate reduce pass.
//
// Tiles: 256 threads = 16 x 16; a 128 x 64 output tile (8 x 4 per thread) for forward / data gradient, 64 x 64 (4 x 4) for the
// weight gradient; 16-deep reduction stages through LDS; fp32 fmaf accumulation (the reference's arithmetic).
#include <algorithm>
#include "nsid_common.h"

namespace {

constexpr int DS_BK = 16;

struct DsFwdArgs {
  const void* x; const float* sc; const float* sh; int act_in;
  const float* w; const float* bias;
  void* out; float* stat; long stat_plane;
  const float* osc; const float* osh; int act_out;
  int B, N, No, C, Co, M;
};

struct DsWgradArgs {
  const void* dr; const void* x; const float* sc; const float* sh; int act_in;
  float* dw;
  int B, N, No, C, Co, M, rchunk;
};

struct DsDgradArgs {
  const void* dr; const float* w; void* dy;
  const void* r; const float* sc; const float* sh; const float* mean; const float* invstd; int act;
  float* partial; long part_plane; int tiles_par;
  int B, N, No, C, Co;
};

template <typename T> __device__ __forceinline__ float ldf(const T* p) { return (float)*p; }

// acc[I][J] += As[k][ty*I + i] * Bs[k][tx*J + j] over the 16 stage rows (LDS reads of 16 bytes)
template <int I, int J, int LDA, int LDB>
__device__ __forceinline__ void stage_fma(const float (*As)[LDA], const float (*Bs)[LDB], int tx, int ty, float (&acc)[I][J]) {
#pragma unroll
  for (int k = 0; k < DS_BK; ++k) {
    float a[I], b[J];
#pragma unroll
    for (int i = 0; i < I; i += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&As[k][ty * I + i]);
      a[i] = v[0]; a[i + 1] = v[1]; a[i + 2] = v[2]; a[i + 3] = v[3];
    }
    const f32x4 v = *reinterpret_cast<const f32x4*>(&Bs[k][tx * J]);
    b[0] = v[0]; b[1] = v[1]; b[2] = v[2]; b[3] = v[3];
#pragma unroll
    for (int i = 0; i < I; ++i)
#pragma unroll
      for (int j = 0; j < J; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
  }
}

// per-column sums of a thread's 8 x 4 values over the 16 row groups, in a fixed order; thread t < 64 gets column t's pair
__device__ __forceinline__ void column_pair(float (*red)[64], const float (&s0)[4], const float (&s1)[4], int tx, int ty,
                                            float& a0, float& a1) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    red[ty][tx * 4 + j] = s0[j];
    red[16 + ty][tx * 4 + j] = s1[j];
  }
  __syncthreads();
  a0 = a1 = 0.f;
  if (threadIdx.x < 64)
    for (int g = 0; g < 16; ++g) {
      a0 += red[g][threadIdx.x];
      a1 += red[16 + g][threadIdx.x];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dsact_fwd_kernel(const DsFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float As[DS_BK][128 + 4];
  __shared__ __attribute__((aligned(16))) float Bs[DS_BK][64 + 4];
  __shared__ float red[32][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.y * 128, o0 = blockIdx.x * 64;
  const T* x = static_cast<const T*>(a.x);
  const int C = a.C, K3 = 3 * C;
  float acc[8][4] = {};
  // this thread's operand row of the A stage, fixed for the whole reduction
  const int am = tid >> 1, akb = (tid & 1) * 8, amg = m0 + am;
  int ab = 0, an = 0;
  if (amg < a.M) { ab = amg / a.No; an = amg - ab * a.No; }
  const int bo = tid >> 2, bkb = (tid & 3) * 4, bog = o0 + bo;
  for (int k0 = 0; k0 < K3; k0 += DS_BK) {
    const int t = k0 / C, c0 = k0 - t * C;        // C % 16 == 0: a stage lies inside one tap
    {
      const int p = 2 * an - 1 + t;
      float v[8] = {};
      if (amg < a.M && p >= 0 && p < a.N) {        // padding rows stay exactly 0: no prologue on them
        const T* src = x + ((long)ab * a.N + p) * C + c0 + akb;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float u = ldf(src + e);
          if (a.sc != nullptr) u = a.sc[c0 + akb + e] * u + a.sh[c0 + akb + e];
          v[e] = nsid_act(u, a.act_in);
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) As[akb + e][am] = v[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      Bs[bkb + e][bo] = bog < a.Co ? a.w[((long)bog * C + c0 + bkb + e) * 3 + t] : 0.f;
    __syncthreads();
    stage_fma<8, 4, 128 + 4, 64 + 4>(As, Bs, tx, ty, acc);
    __syncthreads();
  }
  T* out = static_cast<T*>(a.out);
  float s0[4] = {}, s1[4] = {};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = o0 + tx * 4 + j;
    if (col >= a.Co) continue;
    const float bj = a.bias != nullptr ? a.bias[col] : 0.f;
    const float osc = a.osc != nullptr ? a.osc[col] : 1.f, osh = a.osc != nullptr ? a.osh[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = m0 + ty * 8 + i;
      if (row >= a.M) continue;
      float y = acc[i][j] + bj;
      if (a.osc != nullptr) y = nsid_act(osc * y + osh, a.act_out);
      const T yt = (T)y;
      out[(long)row * a.Co + col] = yt;
      const float yr = (float)yt;                  // the statistics of the stored values
      s0[j] += yr;
      s1[j] += yr * yr;
    }
  }
  if (a.stat == nullptr) return;                   // (uniform over the block)
  float t0, t1;
  column_pair(red, s0, s1, tx, ty, t0, t1);
  if (tid < 64 && o0 + tid < a.Co) {
    a.stat[(long)blockIdx.y * a.Co + o0 + tid] = t0;
    a.stat[a.stat_plane + (long)blockIdx.y * a.Co + o0 + tid] = t1;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dsact_wgrad_kernel(const DsWgradArgs a) {
  __shared__ __attribute__((aligned(16))) float As[DS_BK][64 + 4];
  __shared__ __attribute__((aligned(16))) float Bs[DS_BK][64 + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int j0 = blockIdx.x * 64, o0 = blockIdx.y * 64;
  const int rbeg = blockIdx.z * a.rchunk, rend = min(a.M, rbeg + a.rchunk);
  const T* dr = static_cast<const T*>(a.dr);
  const T* x = static_cast<const T*>(a.x);
  const int C = a.C, K3 = 3 * C;
  float acc[4][4] = {};
  const int lk = tid >> 4, lb = (tid & 15) * 4;
  // this thread's B columns kk = j0 + lb + e: tap and channel, fixed for the whole reduction
  int bt[4], bc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int kk = j0 + lb + e;
    bt[e] = kk < K3 ? kk / C : -1;
    bc[e] = kk < K3 ? kk - bt[e] * C : 0;
  }
  for (int r0 = rbeg; r0 < rend; r0 += DS_BK) {
    const int m = r0 + lk;
    const bool mok = m < rend;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int og = o0 + lb + e;
      As[lk][lb + e] = (mok && og < a.Co) ? ldf(dr + (long)m * a.Co + og) : 0.f;
    }
    int b = 0, n = 0;
    if (mok) { b = m / a.No; n = m - b * a.No; }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int p = 2 * n - 1 + bt[e];
      float v = 0.f;
      if (mok && bt[e] >= 0 && p >= 0 && p < a.N) {     // padding rows stay exactly 0
        float u = ldf(x + ((long)b * a.N + p) * C + bc[e]);
        if (a.sc != nullptr) u = a.sc[bc[e]] * u + a.sh[bc[e]];
        v = nsid_act(u, a.act_in);
      }
      Bs[lk][lb + e] = v;
    }
    __syncthreads();
    stage_fma<4, 4, 64 + 4, 64 + 4>(As, Bs, tx, ty, acc);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = o0 + ty * 4 + i;
    if (o >= a.Co) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kk = j0 + tx * 4 + j;
      if (kk >= K3) continue;
      const int t = kk / C, c = kk - t * C;
      atomicAdd(a.dw + ((long)o * C + c) * 3 + t, acc[i][j]);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dsact_dgrad_kernel(const DsDgradArgs a) {
  __shared__ __attribute__((aligned(16))) float As[DS_BK][128 + 4];
  __shared__ __attribute__((aligned(16))) float Bs[DS_BK][64 + 4];
  __shared__ float red[32][64];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int par = blockIdx.z, c0 = blockIdx.x * 64, i0 = blockIdx.y * 128;
  const int Q = par ? a.N / 2 : (a.N + 1) / 2;      // rows p = 2q + par of every clip
  const int rows = a.B * Q, C = a.C, Co = a.Co;
  const long prow = (long)par * a.tiles_par + blockIdx.y;
  if (i0 >= rows) {                                  // (odd parity, last tiles): an empty tile contributes zero sums
    if (a.partial != nullptr && tid < 64 && c0 + tid < C) {
      a.partial[prow * C + c0 + tid] = 0.f;
      a.partial[a.part_plane + prow * C + c0 + tid] = 0.f;
    }
    return;
  }
  const T* dr = static_cast<const T*>(a.dr);
  float acc[8][4] = {};
  const int am = tid >> 1, akb = (tid & 1) * 8, aig = i0 + am;
  int ab = 0, aq = 0;
  if (aig < rows) { ab = aig / Q; aq = aig - ab * Q; }
  const int bk = tid >> 4, bcb = (tid & 15) * 4;
  const int R = par ? 2 * Co : Co;
  for (int r0 = 0; r0 < R; r0 += DS_BK) {
    const int seg = r0 / Co, ob = r0 - seg * Co;     // Co % 16 == 0: a stage lies inside one segment
    const int t = par == 0 ? 1 : (seg == 0 ? 2 : 0);  // p = 2q: tap 1 of node q; p = 2q+1: tap 2 of node q, tap 0 of node q+1
    {
      const int n = aq + seg;
      float v[8] = {};
      if (aig < rows && n < a.No) {
        const T* src = dr + ((long)ab * a.No + n) * Co + ob + akb;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ldf(src + e);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) As[akb + e][am] = v[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + bcb + e;
      Bs[bk][bcb + e] = c < C ? a.w[((long)(ob + bk) * C + c) * 3 + t] : 0.f;
    }
    __syncthreads();
    stage_fma<8, 4, 128 + 4, 64 + 4>(As, Bs, tx, ty, acc);
    __syncthreads();
  }
  T* dy = static_cast<T*>(a.dy);
  const T* r = static_cast<const T*>(a.r);
  float s0[4] = {}, s1[4] = {};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + tx * 4 + j;
    if (c >= C) continue;
    const float sc = r != nullptr ? a.sc[c] : 1.f, sh = r != nullptr ? a.sh[c] : 0.f;
    const float mu = a.partial != nullptr ? a.mean[c] : 0.f, is = a.partial != nullptr ? a.invstd[c] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ig = i0 + ty * 8 + i;
      if (ig >= rows) continue;
      const int b = ig / Q, q = ig - b * Q;
      const long row = (long)b * a.N + 2 * q + par;
      float g = acc[i][j];
      float rv = 0.f;
      if (r != nullptr) {
        rv = ldf(r + row * C + c);
        g *= nsid_act_grad(sc * rv + sh, a.act);
      }
      const T gt = (T)g;
      dy[row * C + c] = gt;
      const float gs = (float)gt;
      s0[j] += gs;
      s1[j] += gs * ((rv - mu) * is);
    }
  }
  if (a.partial == nullptr) return;
  float t0, t1;
  column_pair(red, s0, s1, tx, ty, t0, t1);
  if (tid < 64 && c0 + tid < C) {
    a.partial[prow * C + c0 + tid] = t0;
    a.partial[a.part_plane + prow * C + c0 + tid] = t1;
  }
}

inline int ds_out(int N) { return (N - 1) / 2 + 1; }

}  // namespace

extern "C" int nsid_dsact_fwd(const void* x, int B, int N, int C, const float* in_scale, const float* in_shift, int act_in,
                              const float* w, const float* bias, void* out, int Cout, float* stat, const float* out_scale,
                              const float* out_shift, int act_out, int act_dtype, void* stream) {
  NSID_REQUIRE(x && w && out && B > 0 && N > 0 && C > 0 && Cout > 0 && C % DS_BK == 0 && NSID_DTYPE_OK(act_dtype));
  NSID_REQUIRE((in_scale == nullptr) == (in_shift == nullptr) && (out_scale == nullptr) == (out_shift == nullptr));
  NSID_REQUIRE(!(stat != nullptr && out_scale != nullptr));       // statistics are of the raw conv output
  DsFwdArgs a{};
  a.x = x; a.sc = in_scale; a.sh = in_shift; a.act_in = act_in;
  a.w = w; a.bias = bias; a.out = out; a.stat = stat;
  a.osc = out_scale; a.osh = out_shift; a.act_out = act_out;
  a.B = B; a.N = N; a.No = ds_out(N); a.C = C; a.Co = Cout;
  const long M = (long)B * a.No;
  NSID_REQUIRE(M < (1L << 31) / 2);
  a.M = (int)M;
  const int tiles = nsid_row_tiles(a.M);
  a.stat_plane = (long)tiles * Cout;
  const dim3 grid((Cout + 63) / 64, tiles);
  NSID_DISPATCH_DTYPE(act_dtype, T, NSID_LAUNCH(dsact_fwd_kernel<T>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a));
  return nsid_launch_status();
}

extern "C" int nsid_dsact_bwd_weight(const void* dout, const void* x, const float* in_scale, const float* in_shift, int act_in,
                                     float* dw, int B, int N, int C, int Cout, int act_dtype, void* stream) {
  NSID_REQUIRE(dout && x && dw && B > 0 && N > 0 && C > 0 && Cout > 0 && NSID_DTYPE_OK(act_dtype));
  NSID_REQUIRE((in_scale == nullptr) == (in_shift == nullptr));
  DsWgradArgs a{};
  a.dr = dout; a.x = x; a.sc = in_scale; a.sh = in_shift; a.act_in = act_in; a.dw = dw;
  a.B = B; a.N = N; a.No = ds_out(N); a.C = C; a.Co = Cout;
  const long M = (long)B * a.No;
  NSID_REQUIRE(M < (1L << 31) / 2);
  a.M = (int)M;
  const long tiles = (long)((3 * C + 63) / 64) * ((Cout + 63) / 64);
  // row splits: about two thousand workgroups, each at least 256 rows deep
  long S = std::max<long>(1, (2048 + tiles - 1) / tiles);
  S = std::min<long>(S, std::max<long>(1, M / 256));
  a.rchunk = (int)(((M + S - 1) / S + DS_BK - 1) / DS_BK * DS_BK);
  S = (M + a.rchunk - 1) / a.rchunk;
  const dim3 grid((3 * C + 63) / 64, (Cout + 63) / 64, (unsigned)S);
  NSID_DISPATCH_DTYPE(act_dtype, T, NSID_LAUNCH(dsact_wgrad_kernel<T>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a));
  return nsid_launch_status();
}

extern "C" int nsid_dsact_part_rows(int B, int N) { return 2 * nsid_row_tiles(B * ((N + 1) / 2)); }

extern "C" int nsid_dsact_bwd_data(const void* dout, const float* w, void* dx, int B, int N, int C, int Cout, const void* r_prev,
                                   const float* scale, const float* shift, const float* mean, const float* invstd, int act,
                                   float* partial, int act_dtype, void* stream) {
  NSID_REQUIRE(dout && w && dx && B > 0 && N > 0 && C > 0 && Cout > 0 && Cout % DS_BK == 0 && NSID_DTYPE_OK(act_dtype));
  NSID_REQUIRE(r_prev == nullptr || (scale && shift));
  NSID_REQUIRE(partial == nullptr || (r_prev && mean && invstd));
  NSID_REQUIRE((long)B * N < (1L << 31) / 2);
  DsDgradArgs a{};
  a.dr = dout; a.w = w; a.dy = dx;
  a.r = r_prev; a.sc = scale; a.sh = shift; a.mean = mean; a.invstd = invstd; a.act = act;
  a.B = B; a.N = N; a.No = ds_out(N); a.C = C; a.Co = Cout;
  a.tiles_par = nsid_row_tiles(B * ((N + 1) / 2));
  a.partial = partial; a.part_plane = 2L * a.tiles_par * C;
  const dim3 grid((C + 63) / 64, a.tiles_par, 2);
  NSID_DISPATCH_DTYPE(act_dtype, T, NSID_LAUNCH(dsact_dgrad_kernel<T>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a));
  return nsid_launch_status();
}
