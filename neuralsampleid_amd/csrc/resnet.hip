// The ResNet-IBN baseline (encoder/resnet_ibn.py of the reference), the first 2-D convolutional network of this library: its eval-mode
// forward, and the backward of its residual blocks (training mode: conv2d_kernel<T, true>, conv2d_wgrad_kernel, col_stat_kernel,
// ibn_relu_bwd_kernel and the block tail, each described where it stands). Activations are channels-last rows (B*H*W, C), fp32 or
// bf16 storage, fp32 accumulation.
//
//   conv2d_kernel      : Conv2d 3x3 (pad 1) / 1x1 (pad 0), stride 1 / 2, as an IMPLICIT GEMM on MFMA: out[m][o] = bias[o] +
//                        sum_{kh, kw, c} x[b][ho*s - pad + kh][wo*s - pad + kw][c] * wp[o][(kh*KW + kw)*C + c] (+ addend) (ReLU).
//                        The im2col matrix is never formed: a thread keeps the (clip, row, column) of its two operand rows and
//                        steps through (tap, channel chunk); a tap outside the image is staged as zeros (top, bottom, left and
//                        right edge of every clip, so nothing leaks between image rows or between the clips of a batch).
//                        128 x 128 output tile over the FLATTENED rows of the batch (layer4 has 84 pixels per clip: tiles are
//                        filled from the batch), 4 waves of 64 x 64, 64-byte reduction stages (32 bf16 / 16 fp32) double
//                        buffered in LDS, the global loads of the next stage (bf16) / next two stages (fp32) in flight under the MFMA block.
//                        bf16 storage: v_mfma_f32_16x16x32_bf16 with bf16 weights. fp32 storage: v_mfma_f32_16x16x4_f32 with
//                        fp32 weights (the parity path); its accumulators are flushed into a second set every 256 reduction
//                        elements, so the rounding error of a K = 9 216 sum grows like that of a K = 256 one.
//                        The MFMA operands are swapped (weights first): a lane then holds 4 consecutive output CHANNELS of one
//                        row and stores 16 (fp32) / 8 (bf16) contiguous bytes.
//   ibn_relu_kernel    : IBN + ReLU. One workgroup per (clip, 64 channels). Instance-norm half: mean, then the biased variance
//                        around it (two passes over the stored values, fixed summation order, no atomics), then the apply;
//                        BatchNorm half: the given per-channel affine. A clip's result depends on that clip only.
//   stem7_pool_kernel  : Conv 7x7 s2 p3 (1 -> 64) + folded BatchNorm + ReLU + MaxPool 3x3 s2 p1. One workgroup per (clip, pooled
//                        row, 16 pooled columns): the 3 x 33 conv pixels under them are computed into LDS (64 channels = the 64
//                        lanes of a wave, the 49 weights of a channel in registers, the input patch broadcast from LDS) and pooled
//                        from there; a conv pixel outside the conv map is -inf for the pool.
//   gem_pool_kernel    : (mean over HW of max(x, eps)^p)^(1/p) per (clip, channel); p is read from device memory.
//   gem_pool_bwd_kernel: its backward (dx fp32, one dp partial per workgroup; gem_dp_sum_kernel adds them: no atomics).
#include "nsid_common.h"

namespace {

constexpr int CV_BM = 128, CV_BN = 128;
constexpr int CV_ROWB = 64;       // bytes of one operand row in one reduction stage
constexpr int CV_LD = 80;         // its LDS stride: 16-byte aligned, 20 banks apart (the 16 rows of a fragment read hit 16 distinct bank quads)
constexpr int CV_FLUSH = 16;      // fp32 path: stages (of 16 elements) per accumulator flush

struct ConvArgs {
  const void* x; const void* w; const float* bias; const void* addend; void* out;
  int B, H, W, C, Ho, Wo, Co, KW, taps, stride, pad, relu, M, tiles_n;
};

// BWD = false: the forward above. BWD = true: the backward-data GATHER of the same convolution through the same loop. The roles are
// swapped by the host: a.x = dy (B, a.H, a.W, a.C) is the conv's OUTPUT map, a.w the (Cin, taps * Cout) packing of pack_conv_bwd, the
// rows written are the conv's INPUT pixels (a.Ho, a.Wo) with a.Co = Cin columns. Input pixel (hi, wi) meets tap (kh, kw) at output
// pixel ((hi + pad - kh) / s, (wi + pad - kw) / s) where both divide and the pixel lies inside the map; every other tap is staged as
// zeros, so a pixel no output pixel reads (three of four under a 1x1 stride-2 conv) comes out as exactly 0.0 (+ addend). a.Co need
// not fill the last column tile: weight rows past it are staged as zeros and not stored.
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void conv2d_kernel(const ConvArgs a) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int EPC = 16 / (int)sizeof(T);            // elements of a 16-byte chunk
  constexpr int BKE = CV_ROWB / (int)sizeof(T);       // reduction elements of a stage
  constexpr int STAGE = (CV_BM + CV_BN) * CV_LD;
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, rq = lane >> 4;
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
  const int tn = blockIdx.x % a.tiles_n, tm = blockIdx.x / a.tiles_n;
  const int m0 = tm * CV_BM, n0 = tn * CV_BN;
  const int C = a.C, K = a.taps * C;
  const T* x = static_cast<const T*>(a.x);
  const T* w = static_cast<const T*>(a.w);

  // the two operand chunks of this thread per stage: rows (tid >> 2) and 64 + (tid >> 2), 16-byte chunk tid & 3 of the 64-byte row
  const int ch = tid & 3;
  long abase[2];          // element offset of (clip, hi0, wi0, channel chunk); only used where the tap is inside the image
  int hi0[2], wi0[2];
  bool aok[2];
  const T* wrow[2];
  [[maybe_unused]] int clip[2];
  [[maybe_unused]] bool wok[2];
  [[maybe_unused]] const int sh = a.stride - 1;      // stride 1 or 2: the division is a shift
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = (tid >> 2) + 64 * q, m = m0 + row;
    aok[q] = m < a.M;
    int b = 0, ho = 0, wo = 0;
    if (aok[q]) {
      b = m / (a.Ho * a.Wo);
      const int r = m - b * (a.Ho * a.Wo);
      ho = r / a.Wo;
      wo = r - ho * a.Wo;
    }
    if constexpr (BWD) {
      hi0[q] = ho + a.pad;
      wi0[q] = wo + a.pad;
      clip[q] = b;
      abase[q] = ch * EPC;
      wok[q] = n0 + row < a.Co;
      wrow[q] = w + (long)min(n0 + row, a.Co - 1) * K + ch * EPC;
    } else {
      hi0[q] = ho * a.stride - a.pad;
      wi0[q] = wo * a.stride - a.pad;
      abase[q] = (((long)b * a.H + hi0[q]) * a.W + wi0[q]) * C + ch * EPC;
      wrow[q] = w + (long)(n0 + row) * K + ch * EPC;
    }
  }

  // Global loads go to registers one (bf16) or two (fp32) stages ahead of the MFMA block that uses them. Past the last stage the
  // load state stops advancing, so a phantom stage re-reads the last one (valid addresses) and is never computed on.
  f32x4 ra[2][2], rb[2][2];
  const int nstage = K / BKE;
  int ld_st = 0, ld_k0 = 0, ld_c0 = 0, ld_kh = 0, ld_kw = 0;      // the stage the next issue() loads (uniform)
  auto issue = [&](f32x4 (&sa)[2], f32x4 (&sb)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      sa[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (BWD) {
        const int th = hi0[q] - ld_kh, tw = wi0[q] - ld_kw;
        const int hi = th >> sh, wi = tw >> sh;
        const bool ok = aok[q] && th >= 0 && tw >= 0 && ((th | tw) & sh) == 0 && hi < a.H && wi < a.W;
        if (ok) sa[q] = *reinterpret_cast<const f32x4*>(x + (((long)clip[q] * a.H + hi) * a.W + wi) * C + abase[q] + ld_c0);
        sb[q] = *reinterpret_cast<const f32x4*>(wrow[q] + ld_k0);
        if (!wok[q]) sb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
        const int hi = hi0[q] + ld_kh, wi = wi0[q] + ld_kw;
        const bool ok = aok[q] && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;      // the conv's zero padding, in both dimensions
        if (ok) sa[q] = *reinterpret_cast<const f32x4*>(x + abase[q] + ((long)ld_kh * a.W + ld_kw) * C + ld_c0);
        sb[q] = *reinterpret_cast<const f32x4*>(wrow[q] + ld_k0);
      }
    }
    if (++ld_st < nstage) {
      ld_k0 += BKE;
      ld_c0 += BKE;
      if (ld_c0 == C) {
        ld_c0 = 0;
        if (++ld_kw == a.KW) { ld_kw = 0; ++ld_kh; }
      }
    }
  };
  auto commit = [&](const f32x4 (&sa)[2], const f32x4 (&sb)[2], int buf) {
    char* dst = lds + buf * STAGE;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int row = (tid >> 2) + 64 * q;
      *reinterpret_cast<f32x4*>(dst + row * CV_LD + ch * 16) = sa[q];
      *reinterpret_cast<f32x4*>(dst + (CV_BM + row) * CV_LD + ch * 16) = sb[q];
    }
  };

  f32x4 acc[4][4], tot[BF ? 1 : 4][BF ? 1 : 4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (!BF) tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  auto compute = [&](int st) {
    const char* la = lds + (st & 1) * STAGE;
    const char* lb = la + CV_BM * CV_LD;
    if constexpr (BF) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(la + (wm0 + 16 * i + lr) * CV_LD + 16 * rq);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(lb + (wn0 + 16 * j + lr) * CV_LD + 16 * rq);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    } else {
      f32x4 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const f32x4*>(la + (wm0 + 16 * i + lr) * CV_LD + 16 * rq);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const f32x4*>(lb + (wn0 + 16 * j + lr) * CV_LD + 16 * rq);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[j][s], fa[i][s], acc[i][j], 0, 0, 0);
      if ((st % CV_FLUSH) == CV_FLUSH - 1) {           // uniform
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            tot[i][j] += acc[i][j];
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
  };

  if constexpr (BF) {
    // bf16: ONE stage in flight. Measured at batch 256 (18 launches of one forward): 5.14 ms against 5.44 ms with two stages in
    // flight; the loop is bound by LDS traffic (8 KB of fragment reads per wave and stage against 16 MFMAs), not by load latency.
    issue(ra[0], rb[0]);
    commit(ra[0], rb[0], 0);
    __syncthreads();
    for (int st = 0; st < nstage; ++st) {
      const bool more = st + 1 < nstage;
      if (more) issue(ra[0], rb[0]);                      // lands under the MFMA block below
      compute(st);
      if (more) commit(ra[0], rb[0], (st + 1) & 1);
      __syncthreads();
    }
  } else {
    // fp32: TWO stages in flight (+15 % over one). Invariant at the top of sub-step u of an iteration: LDS[s & 1] holds stage
    // s = st + u, register set u is free (it held stage s), the other set holds stage s + 1 in flight.
    issue(ra[0], rb[0]);
    commit(ra[0], rb[0], 0);
    issue(ra[1], rb[1]);
    __syncthreads();
    int st = 0;
    for (; st + 1 < nstage; st += 2) {
      issue(ra[0], rb[0]);                                // stage st + 2
      __builtin_amdgcn_sched_barrier(0);
      compute(st);
      __builtin_amdgcn_sched_barrier(0);
      commit(ra[1], rb[1], 1);                            // stage st + 1
      __syncthreads();
      issue(ra[1], rb[1]);                                // stage st + 3
      __builtin_amdgcn_sched_barrier(0);
      compute(st + 1);
      __builtin_amdgcn_sched_barrier(0);
      commit(ra[0], rb[0], 0);                            // stage st + 2 (a phantom past the end: never computed on)
      __syncthreads();
    }
    if (st < nstage) compute(st);                         // an odd stage count: the last stage sits in LDS[0]
  }

  // epilogue. Operands swapped: lane (lr, rq), register r of acc[i][j] is row m = 16 i + lr, channel n = 16 j + 4 rq + r
  T* out = static_cast<T*>(a.out);
  const T* add = static_cast<const T*>(a.addend);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn0 + 16 * j + 4 * rq;
    if constexpr (BWD) {
      if (n >= a.Co) continue;
    }
    f32x4 bj = {0.f, 0.f, 0.f, 0.f};
    if (a.bias != nullptr) bj = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm0 + 16 * i + lr;
      if (m >= a.M) continue;
      f32x4 v = acc[i][j];
      if constexpr (!BF) v += tot[i][j];
      v += bj;
      const long o = (long)m * a.Co + n;
      if (add != nullptr) {
        if constexpr (BF) {
          const bf16x4 h = *reinterpret_cast<const bf16x4*>(add + o);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)h[r];
        } else {
          v += *reinterpret_cast<const f32x4*>(add + o);
        }
      }
      if (a.relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = nsid_act(v[r], NSID_ACT_RELU);
      }
      if constexpr (BF) {
        *reinterpret_cast<bf16x4*>(out + o) = __builtin_convertvector(v, bf16x4);
      } else {
        *reinterpret_cast<f32x4*>(out + o) = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- IBN + ReLU
struct IbnArgs {
  const void* x; void* out;
  const float* gamma; const float* beta; const float* sc; const float* sh;
  int HW, C;
  float eps;
};
constexpr int IBN_CW = 64;        // channels per workgroup
constexpr int IBN_U = 4;          // independent row loads in flight per thread (a pass is a chain of load latencies otherwise)

// rows r, r + RL, ... (IBN_U of them) of this thread's chunk column; rows past the end read as zeros
template <typename T, int RL>
__device__ __forceinline__ void load_rows(const T* x, int r, int HW, int C, float (&v)[IBN_U][Chunk<T>::N]) {
#pragma unroll
  for (int u = 0; u < IBN_U; ++u) {
    const int ru = r + u * RL;
    Chunk<T>::load(x + (long)min(ru, HW - 1) * C, v[u]);        // unconditional (clamped): the IBN_U loads issue back to back
    if (ru >= HW) {
#pragma unroll
      for (int e = 0; e < Chunk<T>::N; ++e) v[u][e] = 0.f;
    }
  }
}

// Instance-norm statistics of a workgroup's 64 channels over its clip's HW rows: the mean, then the biased variance around it (two
// passes over the stored values, fixed summation order). Shared by the forward and the backward: the backward's ReLU mask is then
// the forward's bit for bit. x points at (clip row 0, this thread's chunk column).
template <typename T, int RL>
__device__ __forceinline__ void ibn_in_stats(const T* x, int HW, int C, float eps, int tid, int rl, int cc, float (*red)[IBN_CW],
                                             float (*stat)[IBN_CW], float (&mu)[Chunk<T>::N], float (&istd)[Chunk<T>::N]) {
  constexpr int N = Chunk<T>::N;
  float s[N];
#pragma unroll
  for (int e = 0; e < N; ++e) s[e] = 0.f;
  for (int r = rl; r < HW; r += IBN_U * RL) {
    float v[IBN_U][N];
    load_rows<T, RL>(x, r, HW, C, v);
#pragma unroll
    for (int u = 0; u < IBN_U; ++u)
#pragma unroll
      for (int e = 0; e < N; ++e) s[e] += v[u][e];           // rows past the end were loaded as zeros
  }
#pragma unroll
  for (int e = 0; e < N; ++e) red[rl][cc + e] = s[e];
  __syncthreads();
  if (tid < IBN_CW) {
    float t = 0.f;
    for (int g = 0; g < RL; ++g) t += red[g][tid];
    stat[0][tid] = t / (float)HW;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < N; ++e) { mu[e] = stat[0][cc + e]; s[e] = 0.f; }
  for (int r = rl; r < HW; r += IBN_U * RL) {
    float v[IBN_U][N];
    load_rows<T, RL>(x, r, HW, C, v);
#pragma unroll
    for (int u = 0; u < IBN_U; ++u) {
      if (r + u * RL >= HW) break;
#pragma unroll
      for (int e = 0; e < N; ++e) { const float d = v[u][e] - mu[e]; s[e] = fmaf(d, d, s[e]); }
    }
  }
#pragma unroll
  for (int e = 0; e < N; ++e) red[rl][cc + e] = s[e];
  __syncthreads();
  if (tid < IBN_CW) {
    float t = 0.f;
    for (int g = 0; g < RL; ++g) t += red[g][tid];
    stat[1][tid] = 1.f / sqrtf(t / (float)HW + eps);
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < N; ++e) istd[e] = stat[1][cc + e];
}

template <typename T>
__global__ __launch_bounds__(256) void ibn_relu_kernel(const IbnArgs a) {
  constexpr int N = Chunk<T>::N;
  constexpr int CPR = IBN_CW / N;          // chunks per row of the workgroup's channel block
  constexpr int RL = 256 / CPR;            // row lanes
  __shared__ float red[RL][IBN_CW];
  __shared__ float stat[2][IBN_CW];
  const int tid = threadIdx.x, cc = (tid % CPR) * N, rl = tid / CPR;
  const int c0 = blockIdx.x * IBN_CW, half = a.C / 2;
  const long base = (long)blockIdx.y * a.HW * a.C + c0 + cc;
  const T* x = static_cast<const T*>(a.x) + base;
  T* out = static_cast<T*>(a.out) + base;
  float mu[N], scale[N], shift[N];
  if (c0 < half) {                           // (uniform) instance norm: statistics of this clip's HW rows, two passes
    float istd[N];
    ibn_in_stats<T, RL>(x, a.HW, a.C, a.eps, tid, rl, cc, red, stat, mu, istd);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      scale[e] = a.gamma[c0 + cc + e] * istd[e];
      shift[e] = a.beta[c0 + cc + e];
    }
  } else {                                   // eval-mode BatchNorm half: the given affine
#pragma unroll
    for (int e = 0; e < N; ++e) {
      mu[e] = 0.f;
      scale[e] = a.sc[c0 - half + cc + e];
      shift[e] = a.sh[c0 - half + cc + e];
    }
  }
  for (int r = rl; r < a.HW; r += IBN_U * RL) {
    float v[IBN_U][N];
    load_rows<T, RL>(x, r, a.HW, a.C, v);
#pragma unroll
    for (int u = 0; u < IBN_U; ++u) {
      if (r + u * RL >= a.HW) break;
#pragma unroll
      for (int e = 0; e < N; ++e) v[u][e] = nsid_act(fmaf(v[u][e] - mu[e], scale[e], shift[e]), NSID_ACT_RELU);
      Chunk<T>::store(out + (long)(r + u * RL) * a.C, v[u]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- stem
struct StemArgs {
  const float* x; const float* w; const float* bias; void* out;
  int H, W, Hc, Wc, Hp, Wp;
};
constexpr int ST_PW = 16;                    // pooled columns per workgroup
constexpr int ST_CW = 2 * ST_PW + 1;         // conv columns under them
constexpr int ST_PR = 11, ST_PC = 2 * (ST_CW - 1) + 7;     // input patch: 11 rows x 71 columns

// conv pixel (i, j) of a workgroup's patch against the 49 weights of one channel: THE summation order of the stem. The training
// forward (folded weights), its statistics and its backward all go through it, so the backward's ReLU mask and window winner are the
// forward's bit for bit.
__device__ __forceinline__ float stem7_conv(const float (&patch)[ST_PR][ST_PC + 1], int i, int j, const float (&wk)[49]) {
  float s = 0.f;
#pragma unroll
  for (int kh = 0; kh < 7; ++kh)
#pragma unroll
    for (int kw = 0; kw < 7; ++kw) s = fmaf(patch[2 * i + kh][2 * j + kw], wk[kh * 7 + kw], s);
  return s;
}

// the input patch under the 3 x 33 conv pixels of tile (b, hp, wp0 .. wp0 + 15); outside the image: the conv's zero padding
__device__ __forceinline__ void stem7_load_patch(float (&patch)[ST_PR][ST_PC + 1], const float* __restrict__ x, int H, int W, int b,
                                                 int hp, int wp0, int tid) {
  const int r0 = 4 * hp - 5, q0 = 4 * wp0 - 5;
  const float* xb = x + (long)b * H * W;
  for (int idx = tid; idx < ST_PR * ST_PC; idx += 256) {
    const int pr = idx / ST_PC, pc = idx - pr * ST_PC;
    const int r = r0 + pr, q = q0 + pc;
    patch[pr][pc] = (r >= 0 && r < H && q >= 0 && q < W) ? xb[(long)r * W + q] : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void stem7_pool_kernel(const StemArgs a) {
  __shared__ float patch[ST_PR][ST_PC + 1];
  __shared__ float cmap[3 * ST_CW][64];
  const int tid = threadIdx.x, chn = tid & 63, g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wp0 = blockIdx.x * ST_PW, hp = blockIdx.y, b = blockIdx.z;
  // conv pixel (i, j) of the workgroup is (2 hp - 1 + i, 2 wp0 - 1 + j); its tap (kh, kw) reads input (4 hp - 5 + 2 i + kh, 4 wp0 - 5 + 2 j + kw)
  const int r0 = 4 * hp - 5, q0 = 4 * wp0 - 5;
  const float* xb = a.x + (long)b * a.H * a.W;
  for (int idx = tid; idx < ST_PR * ST_PC; idx += 256) {
    const int pr = idx / ST_PC, pc = idx - pr * ST_PC;
    const int r = r0 + pr, q = q0 + pc;
    patch[pr][pc] = (r >= 0 && r < a.H && q >= 0 && q < a.W) ? xb[(long)r * a.W + q] : 0.f;      // the conv's zero padding
  }
  float wk[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) wk[t] = a.w[chn * 49 + t];
  const float bias = a.bias[chn];
  __syncthreads();
  for (int pix = g; pix < 3 * ST_CW; pix += 4) {           // uniform per wave: the patch reads are broadcasts
    const int i = pix / ST_CW, j = pix - i * ST_CW;
    const int hc = 2 * hp - 1 + i, wc = 2 * wp0 - 1 + j;
    float v = -INFINITY;                                    // the pool's padding
    if (hc >= 0 && hc < a.Hc && wc >= 0 && wc < a.Wc) {
      v = nsid_act(stem7_conv(patch, i, j, wk) + bias, NSID_ACT_RELU);
    }
    cmap[pix][chn] = v;
  }
  __syncthreads();
  T* out = static_cast<T*>(a.out);
  for (int pw = g; pw < ST_PW; pw += 4) {
    const int wp = wp0 + pw;
    if (wp >= a.Wp) break;
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) m = fmaxf(m, cmap[i * ST_CW + 2 * pw + j][chn]);
    out[(((long)b * a.Hp + hp) * a.Wp + wp) * 64 + chn] = (T)m;
  }
}

// ---------------------------------------------------------------------------------------------------------------- stem, training
// Training mode: bn1 normalises with batch statistics. stem7_stat_kernel leaves the per-channel sum / sum of squares of the RAW conv
// output r (each conv pixel is computed once and summed directly: no Gram matrix of the input); nsid_bn_finalize turns them into
// the affine; stem7_fold_kernel folds it into the weights on the device (wf = w * scale, bias = shift) and stem7_pool_kernel runs as
// in eval mode. Nothing of the conv plane is stored: stem7_bwd_kernel recomputes it from x.
//
// Backward (input: dpool on the pooled rows; the network's input is data, so there is no dx). With q(P, c) the conv pixel that wins
// pooled pixel P's window in channel c (first maximum in scan order), g = dpool[P, c] where the winning value is > 0 (else 0),
// xh = (r - mean) * invstd, N = B * Hc * Wc and patch_t(q) the input under tap t of conv pixel q:
//   dbeta_c = a_c = sum_P g            dgamma_c = b_c = sum_P g * xh_c(q)
//   A_ct = sum_P g * patch_t(q)        S_t = sum_{all q} patch_t(q)         X_ct = sum_{all q} xh_c(q) * patch_t(q)
//   dW_ct = gamma_c * invstd_c * (A_ct - (a_c / N) * S_t - (b_c / N) * X_ct)
// Every g-dependent term is a sum over POOLED pixels, so the g map of the conv plane is never formed and workgroups exchange nothing.
// ONE pass over the input: a workgroup walks tiles of the forward's shape (clip, pooled row, 16 pooled columns), recomputes the
// 3 x 33 conv pixels with the folded weights through stem7_conv (mask and winner are the forward's) and with the raw ones (r - mean,
// which X is accumulated from: centred per pixel, no difference of two large sums), adds the conv pixels it OWNS (rows 2 hp, 2 hp + 1,
// columns 2 wp0 .. 2 wp0 + 31: every conv pixel belongs to exactly one tile) into X and S, and its pooled pixels into a, b, A.
// Channel = lane; A and X are 2 x 49 registers per thread. A workgroup leaves ONE partial set; stem7_bwd_finalize_kernel adds the
// sets in workgroup order in fp64 and applies the closed form. No atomics: the result is bitwise reproducible.
constexpr int STB_MAX_WG = 256;                   // partial sets of the backward (its registers allow one workgroup per CU)
constexpr int STS_MAX_WG = NSID_STEM7_STAT_MAX;    // statistics tiles of stem7_stat_kernel (nsid_bn_finalize accepts up to this count)
constexpr int STB_PART = 2 * 49 * 64 + 3 * 64;    // floats per set: A[49][64], X[49][64], a[64], b[64], S[49] (padded to 64)

struct StemTrainArgs {
  const float* x; const float* w; const float* scale; const float* shift; const float* mean; const float* invstd;
  const void* dpool; float* part;
  int H, W, Hc, Wc, Hp, Wp, tiles_w, ntiles;
};

__global__ __launch_bounds__(256) void stem7_fold_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                                         float* __restrict__ wf) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 64 * 49) wf[i] = w[i] * scale[i / 49];
}

__global__ __launch_bounds__(256) void stem7_stat_kernel(const StemTrainArgs a) {
  __shared__ float patch[ST_PR][ST_PC + 1];
  __shared__ float red[2][4][64];
  const int tid = threadIdx.x, chn = tid & 63, g = __builtin_amdgcn_readfirstlane(tid >> 6);
  float wk[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) wk[t] = a.w[chn * 49 + t];
  float s = 0.f, q = 0.f;
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int tw = tile % a.tiles_w, rest = tile / a.tiles_w;
    const int hp = rest % a.Hp, b = rest / a.Hp, wp0 = tw * ST_PW;
    __syncthreads();                                        // the previous tile's patch has been read
    stem7_load_patch(patch, a.x, a.H, a.W, b, hp, wp0, tid);
    __syncthreads();
    for (int pix = g; pix < 2 * 2 * ST_PW; pix += 4) {      // the owned conv pixels: i = 1, 2, j = 1 .. 32
      const int i = 1 + pix / (2 * ST_PW), j = 1 + pix % (2 * ST_PW);
      if (2 * hp - 1 + i < a.Hc && 2 * wp0 - 1 + j < a.Wc) {
        const float r = stem7_conv(patch, i, j, wk);
        s += r;
        q = fmaf(r, r, q);
      }
    }
  }
  red[0][g][chn] = s;
  red[1][g][chn] = q;
  __syncthreads();
  if (tid < 64) {
    a.part[(long)blockIdx.x * 64 + tid] = ((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid];
    a.part[((long)gridDim.x + blockIdx.x) * 64 + tid] = ((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void stem7_bwd_kernel(const StemTrainArgs a) {
  constexpr int NPIX = 3 * ST_CW;
  __shared__ float patch[ST_PR][ST_PC + 1];
  __shared__ float lds[2 * NPIX * 64];                      // cmap | rmap; the four waves' accumulators at the end
  float (*cmap)[64] = reinterpret_cast<float (*)[64]>(lds);                 // relu(bn(r)) as the forward computes it (-inf: pool padding)
  float (*rmap)[64] = reinterpret_cast<float (*)[64]>(lds + NPIX * 64);     // r - mean
  const int tid = threadIdx.x, chn = tid & 63, g = __builtin_amdgcn_readfirstlane(tid >> 6);
  float wr[49], wf[49];
  {
    const float sc = a.scale[chn];
#pragma unroll
    for (int t = 0; t < 49; ++t) {
      wr[t] = a.w[chn * 49 + t];
      wf[t] = wr[t] * sc;                                   // stem7_fold_kernel's product
    }
  }
  const float shift = a.shift[chn], mean = a.mean[chn], invstd = a.invstd[chn];
  const int kh_l = (chn < 49 ? chn : 0) / 7, kw_l = (chn < 49 ? chn : 0) % 7;      // lane t < 49 sums S_t
  float A[49], X[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) A[t] = X[t] = 0.f;
  float sa = 0.f, sb = 0.f, S = 0.f;
  const T* dpool = static_cast<const T*>(a.dpool);
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int tw = tile % a.tiles_w, rest = tile / a.tiles_w;
    const int hp = rest % a.Hp, b = rest / a.Hp, wp0 = tw * ST_PW;
    __syncthreads();                                        // the previous tile's maps and patch have been read
    stem7_load_patch(patch, a.x, a.H, a.W, b, hp, wp0, tid);
    __syncthreads();
    for (int pix = g; pix < NPIX; pix += 4) {               // uniform per wave: the patch reads are broadcasts
      const int i = pix / ST_CW, j = pix - i * ST_CW;
      const int hc = 2 * hp - 1 + i, wc = 2 * wp0 - 1 + j;
      float v = -INFINITY, rc = 0.f;
      if (hc >= 0 && hc < a.Hc && wc >= 0 && wc < a.Wc) {
        v = nsid_act(stem7_conv(patch, i, j, wf) + shift, NSID_ACT_RELU);
        rc = stem7_conv(patch, i, j, wr) - mean;
        if (i >= 1 && j >= 1 && j <= 2 * ST_PW) {           // owned by this tile
#pragma unroll
          for (int kh = 0; kh < 7; ++kh)
#pragma unroll
            for (int kw = 0; kw < 7; ++kw) X[kh * 7 + kw] = fmaf(rc, patch[2 * i + kh][2 * j + kw], X[kh * 7 + kw]);
          if (chn < 49) S += patch[2 * i + kh_l][2 * j + kw_l];
        }
      }
      cmap[pix][chn] = v;
      rmap[pix][chn] = rc;
    }
    __syncthreads();
    for (int pw = g; pw < ST_PW; pw += 4) {
      const int wp = wp0 + pw;
      if (wp >= a.Wp) break;
      float m = -INFINITY;
      int win = ST_CW + 2 * pw + 1;                         // the window's centre is always inside the conv map
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int p = i * ST_CW + 2 * pw + j;
          const float v = cmap[p][chn];
          if (v > m) { m = v; win = p; }                    // strict: the first maximum in scan order
        }
      const float gv = m > 0.f ? (float)dpool[(((long)b * a.Hp + hp) * a.Wp + wp) * 64 + chn] : 0.f;
      const int wi = win / ST_CW, wj = win - wi * ST_CW;
      sa += gv;
      sb = fmaf(gv, rmap[win][chn] * invstd, sb);
#pragma unroll
      for (int kh = 0; kh < 7; ++kh)
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) A[kh * 7 + kw] = fmaf(gv, patch[2 * wi + kh][2 * wj + kw], A[kh * 7 + kw]);
    }
  }
  // the four waves' sums in wave order; set layout: A[t][c], X[t][c], a[c], b[c], S[t]
  float* part = a.part + (long)blockIdx.x * STB_PART;
  float (*acc)[49][64] = reinterpret_cast<float (*)[49][64]>(lds);
  for (int which = 0; which < 2; ++which) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 49; ++t) acc[g][t][chn] = which == 0 ? A[t] : X[t];
    __syncthreads();
    for (int t = g; t < 49; t += 4)
      part[which * 49 * 64 + t * 64 + chn] = ((acc[0][t][chn] + acc[1][t][chn]) + acc[2][t][chn]) + acc[3][t][chn];
  }
  __syncthreads();
  acc[g][0][chn] = sa;
  acc[g][1][chn] = sb;
  acc[g][2][chn] = S;
  __syncthreads();
  if (g < 3) part[2 * 49 * 64 + g * 64 + chn] = ((acc[0][g][chn] + acc[1][g][chn]) + acc[2][g][chn]) + acc[3][g][chn];
}

// one workgroup per tap t, 4 x 64 threads = (quarter of the partial sets) x channel: the sets in order, fp64, then the closed form
__global__ __launch_bounds__(256) void stem7_bwd_finalize_kernel(const float* __restrict__ part, int nset, double N,
                                                                 const float* __restrict__ gamma, const float* __restrict__ invstd,
                                                                 float* __restrict__ dw, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta) {
  __shared__ double red[5][4][64];
  const int t = blockIdx.x, c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int per = (nset + 3) / 4, s0 = g * per, s1 = min(nset, s0 + per);
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int off[5] = {t * 64 + c, 49 * 64 + t * 64 + c, 2 * 49 * 64 + c, 2 * 49 * 64 + 64 + c, 2 * 49 * 64 + 128 + t};
  constexpr int UB = 4;                         // loads of a batch issue before the first add; the order of the adds is the set order
  int s = s0;
  for (; s + UB <= s1; s += UB) {
    float l[UB][5];
#pragma unroll
    for (int u = 0; u < UB; ++u)
#pragma unroll
      for (int k = 0; k < 5; ++k) l[u][k] = part[(long)(s + u) * STB_PART + off[k]];
#pragma unroll
    for (int u = 0; u < UB; ++u)
#pragma unroll
      for (int k = 0; k < 5; ++k) v[k] += (double)l[u][k];
  }
  for (; s < s1; ++s)
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] += (double)part[(long)s * STB_PART + off[k]];
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][g][c] = v[k];
  __syncthreads();
  if (g != 0) return;
#pragma unroll
  for (int k = 0; k < 5; ++k) v[k] = ((red[k][0][c] + red[k][1][c]) + red[k][2][c]) + red[k][3][c];
  const double A = v[0], X = v[1] * (double)invstd[c], sa = v[2], sb = v[3], S = v[4];
  dw[c * 49 + t] = (float)((double)gamma[c] * (double)invstd[c] * (A - sa / N * S - sb / N * X));
  if (t == 0) {
    dgamma[c] = (float)sb;
    dbeta[c] = (float)sa;
  }
}

// ---------------------------------------------------------------------------------------------------------------- GeM
template <typename T>
__global__ __launch_bounds__(256) void gem_pool_kernel(const T* __restrict__ x, int HW, int C, const float* __restrict__ p_dev,
                                                       float eps, float* __restrict__ out) {
  __shared__ float red[4][64];
  const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  const int c0 = blockIdx.x * 64, b = blockIdx.y;
  const float p = p_dev[0];
  const T* xb = x + (long)b * HW * C + c0 + c;
  float s = 0.f;
  for (int r = g; r < HW; r += 4) s += powf(fmaxf((float)xb[(long)r * C], eps), p);
  red[g][c] = s;
  __syncthreads();
  if (tid < 64) {
    const float t = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    out[(long)b * C + c0 + tid] = powf(t / (float)HW, 1.f / p);
  }
}

// Backward of gem_pool_kernel for the same (64 channels, clip) tile. With xh = max(x, eps), m = mean_hw xh^p, y = m^(1/p):
//   dx = dy y^(1-p) xh^(p-1) / HW where x > eps, else 0
//   dp = sum_{b,c} dy y ( sum_hw xh^p ln xh / (p HW m) - ln m / p^2 ): one partial per workgroup, summed by gem_dp_sum_kernel
template <typename T>
__global__ __launch_bounds__(256) void gem_pool_bwd_kernel(const T* __restrict__ x, const float* __restrict__ dy, int HW, int C,
                                                           const float* __restrict__ p_dev, float eps, float* __restrict__ dx,
                                                           float* __restrict__ dp_part) {
  __shared__ double red[2][4][64];
  __shared__ float coef[64];
  const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  const int c0 = blockIdx.x * 64, b = blockIdx.y;
  const float p = p_dev[0];
  const T* xb = x + (long)b * HW * C + c0 + c;
  double s = 0.0, sl = 0.0;          // dp is a difference of two nearly equal means: sums and the per-channel factors in double
  for (int r = g; r < HW; r += 4) {
    const float xh = fmaxf((float)xb[(long)r * C], eps);
    const float xp = powf(xh, p);
    s += (double)xp;
    sl += (double)xp * (double)logf(xh);
  }
  red[0][g][c] = s;
  red[1][g][c] = sl;
  __syncthreads();
  if (tid < 64) {
    const double t = ((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid];
    const double tl = ((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid];
    const double pd = (double)p, m = t / (double)HW;
    const double y = pow(m, 1.0 / pd);
    const double g_y = (double)dy[(long)b * C + c0 + tid];
    coef[tid] = (float)(g_y * pow(y, 1.0 - pd) / (double)HW);
    const double part = wave_sum_d(g_y * y * (tl / (pd * (double)HW * m) - log(m) / (pd * pd)));
    if (tid == 0) dp_part[(long)b * gridDim.x + blockIdx.x] = (float)part;
  }
  __syncthreads();
  const float k = coef[c];
  float* db = dx + (long)b * HW * C + c0 + c;
  for (int r = g; r < HW; r += 4) {
    const float xv = (float)xb[(long)r * C];
    db[(long)r * C] = xv > eps ? k * powf(xv, p - 1.f) : 0.f;
  }
}

__global__ __launch_bounds__(256) void gem_dp_sum_kernel(const float* __restrict__ part, int n, float* __restrict__ dp) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += (double)part[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) dp[0] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

// ---------------------------------------------------------------------------------------------------------------- conv weight gradient
// dw[o][(kh*KW + kw)*C + c] += sum_m dy[m][o] * x[gather(m, kh, kw)][c]: the forward's packed layout. One workgroup per (row split,
// 128 output channels, tap, 128 input channels); the reduction runs over the rows m, the strided dimension of both operands, so a
// stage is KB rows x 128 columns of each operand as they lie in memory and the MFMA fragments come from transposing LDS reads
// (bf16: ds_read_b64_tr_b16 with the row layout of gemm.hip's i/j-major tiles; fp32: one 4-byte read per MFMA operand, the row pitch
// 16 banks past a multiple of 64 so that the four reduction rows of a read do not collide). A tap outside the image and the rows
// past M are staged as zeros. Split over the rows: split sp writes its 128 x 128 tile into part[sp] (the whole dw layout per split),
// conv2d_wgrad_sum_kernel adds the splits in order into dw: no atomics, two calls give the same bits. One split: straight into dw.
struct ConvWgArgs {
  const void* dy; const void* x; float* out;
  int H, W, C, Ho, Wo, Co, KW, taps, stride, pad, M, tiles_c, splits, stages_per;
};

template <typename T>
__global__ __launch_bounds__(256) void conv2d_wgrad_kernel(const ConvWgArgs a) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int KB = BF ? 32 : 16;                    // reduction rows of a stage
  constexpr int EPC = 16 / (int)sizeof(T);
  constexpr int CPR = 128 / EPC;                      // 16-byte chunks of a 128-column row: 16 (bf16) / 32 (fp32)
  constexpr int RPP = 256 / CPR;                      // rows the 256 threads cover in one pass: 16 / 8 (two passes per stage)
  constexpr int LD = BF ? 288 : 576;                  // LDS row pitch in bytes
  constexpr int OPB = BF ? KB * LD + (KB / 8) * 128 : KB * LD;      // one operand of one stage
  static_assert(KB == 2 * RPP, "a stage is two passes");
  __shared__ __attribute__((aligned(16))) char lds[4 * OPB];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, rq = lane >> 4;
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
  const int sp = blockIdx.x;
  int t = blockIdx.y;
  const int tc = t % a.tiles_c;
  t /= a.tiles_c;
  const int tap = t % a.taps, to = t / a.taps;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int o0 = to * 128, c0 = tc * 128;
  const int cch = (tid % CPR) * EPC, rr = tid / CPR;
  const bool cok = c0 + cch < a.C;
  const T* dy = static_cast<const T*>(a.dy);
  const T* x = static_cast<const T*>(a.x);
  const int nst_all = (a.M + KB - 1) / KB;
  const int st0 = sp * a.stages_per, st1 = min(st0 + a.stages_per, nst_all);
  const unsigned HoWo = (unsigned)(a.Ho * a.Wo);

  auto rowoff = [](int k) { return BF ? k * LD + (k >> 3) * 128 : k * LD; };
  f32x4 ra[2], rb[2];
  auto issue = [&](int st) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int m = st * KB + rr + RPP * q;
      ra[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      rb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m < a.M) {
        const unsigned b = (unsigned)m / HoWo, r = (unsigned)m - b * HoWo;
        const int ho = (int)(r / (unsigned)a.Wo), wo = (int)r - ho * a.Wo;
        const int hi = ho * a.stride - a.pad + kh, wi = wo * a.stride - a.pad + kw;
        ra[q] = *reinterpret_cast<const f32x4*>(dy + (long)m * a.Co + o0 + cch);
        if (cok && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W)
          rb[q] = *reinterpret_cast<const f32x4*>(x + (((long)b * a.H + hi) * a.W + wi) * a.C + c0 + cch);
      }
    }
  };
  auto commit = [&](int buf) {
    char* dst = lds + buf * 2 * OPB;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int off = rowoff(rr + RPP * q) + cch * (int)sizeof(T);
      *reinterpret_cast<f32x4*>(dst + off) = ra[q];
      *reinterpret_cast<f32x4*>(dst + OPB + off) = rb[q];
    }
  };

  f32x4 acc[4][4], tot[BF ? 1 : 4][BF ? 1 : 4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (!BF) tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  auto compute = [&](int it) {
    const char* la = lds + (it & 1) * 2 * OPB;
    const char* lb = la + OPB;
    if constexpr (BF) {
      typedef bf16x4 __attribute__((address_space(3))) * lds_bf16x4_ptr;
      // lane 4q + p of a 16-lane group addresses reduction row 8 rq + q (then + 4), columns 4p .. 4p + 3 of the fragment's 16; the
      // hardware hands lane lr column lr of those rows (all 64 lanes are active here: the loop is uniform)
      const int fo = (8 * rq + (lr >> 2)) * LD + rq * 128 + 8 * (lr & 3);
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const char* p = la + fo + 2 * (wm0 + 16 * i);
        const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p));
        const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p + 4 * LD));
        fa[i] = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const char* p = lb + fo + 2 * (wn0 + 16 * j);
        const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p));
        const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p + 4 * LD));
        fb[j] = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = *reinterpret_cast<const float*>(la + (4 * s + rq) * LD + 4 * (wm0 + 16 * i + lr));
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const float*>(lb + (4 * s + rq) * LD + 4 * (wn0 + 16 * j + lr));
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[j], fa[i], acc[i][j], 0, 0, 0);
      }
      if ((it % CV_FLUSH) == CV_FLUSH - 1) {           // uniform: as in the forward, every 256 reduction rows
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            tot[i][j] += acc[i][j];
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
  };

  if (st0 < st1) {                                      // uniform
    issue(st0);
    commit(0);
    __syncthreads();
    for (int st = st0; st < st1; ++st) {
      const bool more = st + 1 < st1;
      if (more) issue(st + 1);                          // lands under the MFMA block below
      compute(st - st0);
      if (more) commit((st + 1 - st0) & 1);
      __syncthreads();
    }
  }

  // lane (lr, rq), register r of acc[i][j]: output channel o = 16 i + lr, input channel c = 16 j + 4 rq + r (operands swapped as in
  // the forward: 16 contiguous bytes per lane)
  const long K = (long)a.taps * a.C;
  float* out = a.out + (a.splits > 1 ? (long)sp * a.Co * K : 0L);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + wn0 + 16 * j + 4 * rq;
    if (c >= a.C) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = o0 + wm0 + 16 * i + lr;
      f32x4 v = acc[i][j];
      if constexpr (!BF) v += tot[i][j];
      f32x4* p = reinterpret_cast<f32x4*>(out + (long)o * K + (long)tap * a.C + c);
      if (a.splits > 1) *p = v; else *p += v;
    }
  }
}

__global__ __launch_bounds__(256) void conv2d_wgrad_sum_kernel(const float* __restrict__ part, int splits, long n4, float* __restrict__ dw) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(part) + i;
  f32x4 s = p[0];
  for (int sp = 1; sp < splits; ++sp) s += p[(long)sp * n4];      // fixed order
  reinterpret_cast<f32x4*>(dw)[i] += s;
}

// ---------------------------------------------------------------------------------------------------------------- column statistics
// Per-channel sum and sum of squares of the stored rows (M, C) with row pitch ld, one workgroup per (64 channels, 128-row tile), into
// the [2][row tiles][C] layout bn_finalize_kernel reads: the batch statistics of a conv2d output (bn2, the stride-2 downsample) and of
// the BatchNorm half of the IBN (a column slice of conv1's output).
template <typename T>
__global__ __launch_bounds__(256) void col_stat_kernel(const T* __restrict__ x, long ld, int M, int C, float* __restrict__ stat, int tiles) {
  __shared__ float red[2][4][64];
  const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  const int c0 = blockIdx.x * 64, tile = blockIdx.y;
  const int r1 = min(M, (tile + 1) * NSID_ROW_TILE);
  float s = 0.f, q = 0.f;
  for (int r = tile * NSID_ROW_TILE + g; r < r1; r += 4) {
    const float v = (float)x[(long)r * ld + c0 + c];
    s += v;
    q = fmaf(v, v, q);
  }
  red[0][g][c] = s;
  red[1][g][c] = q;
  __syncthreads();
  if (tid < 64) {
    stat[(long)tile * C + c0 + tid] = ((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid];
    stat[((long)tiles + tile) * C + c0 + tid] = ((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid];
  }
}

// ---------------------------------------------------------------------------------------------------------------- IBN + ReLU backward
// y = relu(IBN(r)). With g = dy * [y > 0] and xh = (r - mean) * invstd, over the rows the statistics were taken over (the clip's HW
// rows for the instance-norm half, all B * HW rows for the BatchNorm half):
//   dr = gamma * invstd * (g - mean(g) - xh * mean(g * xh)),   dgamma = sum g * xh,   dbeta = sum g
// ibn_relu_bwd_kernel, one workgroup per (clip, 64 channels) as in the forward: the instance-norm half recomputes its statistics
// with the forward's code, reduces and writes dr; both halves leave their per-clip (sum g, sum g xh) in part[2][B][C].
// ibn_bwd_finalize_kernel adds the clips in order (fp64) into the four parameter gradients and leaves the BatchNorm half's two means;
// ibn_bwd_bn_apply_kernel writes the BatchNorm half's dr. The mask is fmaf(r - mu, scale, shift) > 0 exactly as the forward evaluates it.
struct IbnBwdArgs {
  const void* dy; const void* r; void* dr;
  const float* gamma; const float* beta; const float* sc; const float* sh; const float* mean; const float* invstd;
  float* part; float* coef;
  int B, HW, C;
  float eps;
};

template <typename T, int RL>
__device__ __forceinline__ void ibn_col_sums(const float (&s0)[Chunk<T>::N], const float (&s1)[Chunk<T>::N], int tid, int rl, int cc,
                                             float (*red)[IBN_CW], float (*stat)[IBN_CW]) {
  constexpr int N = Chunk<T>::N;
#pragma unroll
  for (int e = 0; e < N; ++e) red[rl][cc + e] = s0[e];
  __syncthreads();
  if (tid < IBN_CW) {
    float t = 0.f;
    for (int g = 0; g < RL; ++g) t += red[g][tid];
    stat[0][tid] = t;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < N; ++e) red[rl][cc + e] = s1[e];
  __syncthreads();
  if (tid < IBN_CW) {
    float t = 0.f;
    for (int g = 0; g < RL; ++g) t += red[g][tid];
    stat[1][tid] = t;
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void ibn_relu_bwd_kernel(const IbnBwdArgs a) {
  constexpr int N = Chunk<T>::N;
  constexpr int CPR = IBN_CW / N;
  constexpr int RL = 256 / CPR;
  __shared__ float red[RL][IBN_CW];
  __shared__ float stat[2][IBN_CW];
  const int tid = threadIdx.x, cc = (tid % CPR) * N, rl = tid / CPR;
  const int c0 = blockIdx.x * IBN_CW, half = a.C / 2, b = blockIdx.y;
  const long base = (long)b * a.HW * a.C + c0 + cc;
  const T* x = static_cast<const T*>(a.r) + base;
  const T* dy = static_cast<const T*>(a.dy) + base;
  T* dr = static_cast<T*>(a.dr) + base;
  const bool in_half = c0 < half;            // uniform
  float mu[N], istd[N], scale[N], shift[N], mmu[N];       // mmu: what the forward subtracts before its fmaf (the mask's arithmetic)
  if (in_half) {
    ibn_in_stats<T, RL>(x, a.HW, a.C, a.eps, tid, rl, cc, red, stat, mu, istd);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      scale[e] = a.gamma[c0 + cc + e] * istd[e];
      shift[e] = a.beta[c0 + cc + e];
      mmu[e] = mu[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const int c = c0 - half + cc + e;
      mu[e] = a.mean[c];
      istd[e] = a.invstd[c];
      scale[e] = a.sc[c];
      shift[e] = a.sh[c];
      mmu[e] = 0.f;
    }
  }
  float s0[N], s1[N];
#pragma unroll
  for (int e = 0; e < N; ++e) s0[e] = s1[e] = 0.f;
  for (int r = rl; r < a.HW; r += IBN_U * RL) {
    float v[IBN_U][N], d[IBN_U][N];
    load_rows<T, RL>(x, r, a.HW, a.C, v);
    load_rows<T, RL>(dy, r, a.HW, a.C, d);              // rows past the end: d = 0, so they add nothing
#pragma unroll
    for (int u = 0; u < IBN_U; ++u)
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float g = fmaf(v[u][e] - mmu[e], scale[e], shift[e]) > 0.f ? d[u][e] : 0.f;
        s0[e] += g;
        s1[e] = fmaf(g, (v[u][e] - mu[e]) * istd[e], s1[e]);
      }
  }
  ibn_col_sums<T, RL>(s0, s1, tid, rl, cc, red, stat);
  if (tid < IBN_CW) {
    a.part[(long)b * a.C + c0 + tid] = stat[0][tid];
    a.part[((long)a.B + b) * a.C + c0 + tid] = stat[1][tid];
  }
  if (!in_half) return;                       // uniform
  float mg[N], mgx[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    mg[e] = stat[0][cc + e] / (float)a.HW;
    mgx[e] = stat[1][cc + e] / (float)a.HW;
  }
  for (int r = rl; r < a.HW; r += IBN_U * RL) {
    float v[IBN_U][N], d[IBN_U][N];
    load_rows<T, RL>(x, r, a.HW, a.C, v);
    load_rows<T, RL>(dy, r, a.HW, a.C, d);
#pragma unroll
    for (int u = 0; u < IBN_U; ++u) {
      if (r + u * RL >= a.HW) break;
      float o[N];
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float g = fmaf(v[u][e] - mmu[e], scale[e], shift[e]) > 0.f ? d[u][e] : 0.f;
        o[e] = scale[e] * (g - mg[e] - (v[u][e] - mu[e]) * istd[e] * mgx[e]);
      }
      Chunk<T>::store(dr + (long)(r + u * RL) * a.C, o);
    }
  }
}

// one thread per channel: the clips' partial sums in clip order, fp64
__global__ __launch_bounds__(128) void ibn_bwd_finalize_kernel(const float* __restrict__ part, int B, int HW, int C, float* dg_in,
                                                               float* db_in, float* dg_bn, float* db_bn, float* __restrict__ coef) {
  const int c = blockIdx.x * 128 + threadIdx.x;
  if (c >= C) return;
  const float* p0 = part + c;
  const float* p1 = part + (long)B * C + c;
  double sg = 0.0, sgx = 0.0;
  constexpr int UB = 8;                       // loads of a batch issue before the first add; the order of the adds is the clip order
  int b = 0;
  for (; b + UB <= B; b += UB) {
    float va[UB], vb[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) { va[u] = p0[(long)(b + u) * C]; vb[u] = p1[(long)(b + u) * C]; }
#pragma unroll
    for (int u = 0; u < UB; ++u) { sg += (double)va[u]; sgx += (double)vb[u]; }
  }
  for (; b < B; ++b) { sg += (double)p0[(long)b * C]; sgx += (double)p1[(long)b * C]; }
  const int half = C / 2;
  if (c < half) {
    dg_in[c] += (float)sgx;
    db_in[c] += (float)sg;
  } else {
    dg_bn[c - half] += (float)sgx;
    db_bn[c - half] += (float)sg;
    const double M = (double)B * (double)HW;
    coef[c - half] = (float)(sg / M);
    coef[half + c - half] = (float)(sgx / M);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ibn_bwd_bn_apply_kernel(const IbnBwdArgs a) {
  constexpr int N = Chunk<T>::N;
  constexpr int CPR = IBN_CW / N;
  constexpr int RL = 256 / CPR;
  const int tid = threadIdx.x, cc = (tid % CPR) * N, rl = tid / CPR;
  const int half = a.C / 2, ch0 = blockIdx.x * IBN_CW + cc;          // channel of the BatchNorm half
  const long base = (long)blockIdx.y * a.HW * a.C + half + ch0;
  const T* x = static_cast<const T*>(a.r) + base;
  const T* dy = static_cast<const T*>(a.dy) + base;
  T* dr = static_cast<T*>(a.dr) + base;
  float mu[N], istd[N], scale[N], shift[N], mg[N], mgx[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    mu[e] = a.mean[ch0 + e];
    istd[e] = a.invstd[ch0 + e];
    scale[e] = a.sc[ch0 + e];
    shift[e] = a.sh[ch0 + e];
    mg[e] = a.coef[ch0 + e];
    mgx[e] = a.coef[half + ch0 + e];
  }
  for (int r = rl; r < a.HW; r += IBN_U * RL) {
    float v[IBN_U][N], d[IBN_U][N];
    load_rows<T, RL>(x, r, a.HW, a.C, v);
    load_rows<T, RL>(dy, r, a.HW, a.C, d);
#pragma unroll
    for (int u = 0; u < IBN_U; ++u) {
      if (r + u * RL >= a.HW) break;
      float o[N];
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float g = fmaf(v[u][e] - 0.f, scale[e], shift[e]) > 0.f ? d[u][e] : 0.f;
        o[e] = scale[e] * (g - mg[e] - (v[u][e] - mu[e]) * istd[e] * mgx[e]);
      }
      Chunk<T>::store(dr + (long)(r + u * RL) * a.C, o);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- block tail
// out = relu(sc3 * r3 + sh3 + identity), identity = scd * rd + shd (the downsample's BatchNorm) or the block's input as it is
// (scd == nullptr): the tail of a training-mode block, where bn3's affine comes from batch statistics and cannot be folded.
// Every thread keeps ONE column chunk for the whole kernel (the launch makes the thread count a multiple of the chunks per row, as
// nsid_bn_bwd_apply does), so the four per-channel vectors are loaded once and U rows are in flight per iteration.
template <typename T, int U>
__global__ __launch_bounds__(256) void bn_add_relu_kernel(const T* __restrict__ r3, const float* __restrict__ sc3,
                                                          const float* __restrict__ sh3, const T* __restrict__ idn,
                                                          const float* __restrict__ scd, const float* __restrict__ shd,
                                                          T* __restrict__ out, long rows, int CV) {
  constexpr int N = Chunk<T>::N;
  const long t = (long)blockIdx.x * 256 + threadIdx.x, total = (long)gridDim.x * 256;
  const int cq = (int)(t % CV), c = cq * N;
  const long rstep = total / CV;                  // total % CV == 0 (host)
  const bool ds = scd != nullptr;                 // uniform
  float a3[N], b3[N], ad[N], bd[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    a3[e] = sc3[c + e];
    b3[e] = sh3[c + e];
    ad[e] = ds ? scd[c + e] : 1.f;
    bd[e] = ds ? shd[c + e] : 0.f;
  }
  for (long row = t / CV; row < rows; row += U * rstep) {
    float v[U][N], w[U][N];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long rr = row + u * rstep;
      if (rr < rows) {
        Chunk<T>::load(r3 + (rr * CV + cq) * N, v[u]);
        Chunk<T>::load(idn + (rr * CV + cq) * N, w[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long rr = row + u * rstep;
      if (rr < rows) {
        float o[N];
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const float id = ds ? fmaf(ad[e], w[u][e], bd[e]) : w[u][e];
          o[e] = nsid_act(fmaf(a3[e], v[u][e], b3[e]) + id, NSID_ACT_RELU);
        }
        Chunk<T>::store(out + (rr * CV + cq) * N, o);
      }
    }
  }
}

// g = dy where the stored output y is positive, else 0: the gradient behind that ReLU, shared by the main branch and the shortcut
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, T* __restrict__ g, long nchunks) {
  constexpr int N = Chunk<T>::N;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (long)gridDim.x * 256) {
    float d[N], v[N];
    Chunk<T>::load(dy + i * N, d);
    Chunk<T>::load(y + i * N, v);
#pragma unroll
    for (int e = 0; e < N; ++e) d[e] = v[e] > 0.f ? d[e] : 0.f;
    Chunk<T>::store(g + i * N, d);
  }
}

}  // namespace

extern "C" int nsid_conv2d_fwd(const void* x, int B, int H, int W, int C, const void* w, int w_dtype, const float* bias,
                               const void* addend, void* out, int Cout, int ksize, int stride, int act_out, int act_dtype,
                               void* stream) {
  NSID_REQUIRE(x && w && out && B > 0 && H > 0 && W > 0 && C > 0 && Cout > 0 && NSID_DTYPE_OK(act_dtype));
  NSID_REQUIRE(w_dtype == act_dtype);              // bf16 weights with bf16 activations, fp32 weights on the fp32 MFMA
  NSID_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2));
  NSID_REQUIRE(act_out == NSID_ACT_NONE || act_out == NSID_ACT_RELU);
  NSID_REQUIRE(C % (act_dtype == NSID_BF16 ? 32 : 16) == 0 && Cout % CV_BN == 0);
  NSID_REQUIRE(nsid_aligned16(x) && nsid_aligned16(w) && nsid_aligned16(out) && nsid_aligned16(bias) && nsid_aligned16(addend));
  ConvArgs a{};
  a.x = x; a.w = w; a.bias = bias; a.addend = addend; a.out = out;
  a.B = B; a.H = H; a.W = W; a.C = C; a.Co = Cout;
  a.KW = ksize; a.taps = ksize * ksize; a.stride = stride; a.pad = ksize / 2;
  a.Ho = (H + 2 * a.pad - ksize) / stride + 1;
  a.Wo = (W + 2 * a.pad - ksize) / stride + 1;
  a.relu = act_out == NSID_ACT_RELU;
  const long M = (long)B * a.Ho * a.Wo;
  NSID_REQUIRE(M < (1L << 31) / 2 && (long)B * H * W < (1L << 31) / 2);
  a.M = (int)M;
  a.tiles_n = Cout / CV_BN;
  const long wgs = ((M + CV_BM - 1) / CV_BM) * a.tiles_n;
  NSID_REQUIRE(wgs < (1L << 31) - 1);
  nsid_count(ksize == 3 ? NSID_C_conv2d_3x3 : NSID_C_conv2d_1x1);
  NSID_DISPATCH_DTYPE(act_dtype, T,
                      NSID_LAUNCH((conv2d_kernel<T, false>), dim3((unsigned)wgs), dim3(256), 0, static_cast<hipStream_t>(stream), a));
  return nsid_launch_status();
}

extern "C" int nsid_ibn_relu_fwd(const void* x, int B, int HW, int C, const float* in_gamma, const float* in_beta, float eps,
                                 const float* bn_scale, const float* bn_shift, void* out, int dtype, void* stream) {
  NSID_REQUIRE(x && out && in_gamma && in_beta && bn_scale && bn_shift && B > 0 && B <= 65535 && HW > 0 && C > 0);
  NSID_REQUIRE(NSID_DTYPE_OK(dtype) && C % (2 * IBN_CW) == 0 && eps >= 0.f && nsid_aligned16(x) && nsid_aligned16(out));
  IbnArgs a{};
  a.x = x; a.out = out; a.gamma = in_gamma; a.beta = in_beta; a.sc = bn_scale; a.sh = bn_shift;
  a.HW = HW; a.C = C; a.eps = eps;
  nsid_count(NSID_C_ibn_relu);
  NSID_DISPATCH_DTYPE(dtype, T,
                      NSID_LAUNCH(ibn_relu_kernel<T>, dim3(C / IBN_CW, B), dim3(256), 0, static_cast<hipStream_t>(stream), a));
  return nsid_launch_status();
}

extern "C" int nsid_stem7_pool_fwd(const float* x, int B, int H, int W, const float* w, const float* bias, void* out, int out_dtype,
                                   void* stream) {
  NSID_REQUIRE(x && w && bias && out && B > 0 && B <= 65535 && H > 0 && W > 0 && NSID_DTYPE_OK(out_dtype));
  StemArgs a{};
  a.x = x; a.w = w; a.bias = bias; a.out = out;
  a.H = H; a.W = W;
  a.Hc = (H - 1) / 2 + 1; a.Wc = (W - 1) / 2 + 1;          // (H + 6 - 7) / 2 + 1
  a.Hp = (a.Hc - 1) / 2 + 1; a.Wp = (a.Wc - 1) / 2 + 1;    // (Hc + 2 - 3) / 2 + 1
  NSID_REQUIRE(a.Hp <= 65535 && (long)B * a.Hp * a.Wp < (1L << 31) / 64);
  nsid_count(NSID_C_stem7_pool);
  const dim3 grid((a.Wp + ST_PW - 1) / ST_PW, a.Hp, B);
  NSID_DISPATCH_DTYPE(out_dtype, T, NSID_LAUNCH(stem7_pool_kernel<T>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a));
  return nsid_launch_status();
}

static inline void stem_train_dims(StemTrainArgs& a, int H, int W) {
  a.H = H; a.W = W;
  a.Hc = (H - 1) / 2 + 1; a.Wc = (W - 1) / 2 + 1;
  a.Hp = (a.Hc - 1) / 2 + 1; a.Wp = (a.Wc - 1) / 2 + 1;
  a.tiles_w = (a.Wp + ST_PW - 1) / ST_PW;
}

// tiles of the training-mode stem kernels (clip, pooled row, 16 pooled columns) for rows = B * Hp and cols = Wp, and the number of
// partial sets the statistics (which = 0) / the backward (which = 1) leave
extern "C" long nsid_stem7_partials(long rows, long cols, int which) {
  const long tiles = rows * ((cols + ST_PW - 1) / ST_PW);
  const long cap = which == 0 ? STS_MAX_WG : STB_MAX_WG;
  return tiles < cap ? tiles : cap;
}
extern "C" long nsid_stem7_bwd_set_floats(void) { return STB_PART; }

extern "C" int nsid_stem7_stat(const float* x, int B, int H, int W, const float* w, float* stat, void* stream) {
  NSID_REQUIRE(x && w && stat && B > 0 && B <= 65535 && H > 0 && W > 0);
  StemTrainArgs a{};
  a.x = x; a.w = w; a.part = stat;
  stem_train_dims(a, H, W);
  NSID_REQUIRE(a.Hp <= 65535 && (long)B * a.Hp * a.Wp < (1L << 31) / 64);
  a.ntiles = B * a.Hp * a.tiles_w;
  nsid_count(NSID_C_stem7_stat);
  NSID_LAUNCH(stem7_stat_kernel, dim3((unsigned)nsid_stem7_partials((long)B * a.Hp, a.Wp, 0)), dim3(256), 0,
              static_cast<hipStream_t>(stream), a);
  return nsid_launch_status();
}

extern "C" int nsid_stem7_pool_train_fwd(const float* x, int B, int H, int W, const float* w, const float* scale, const float* shift,
                                         float* wf, void* out, int out_dtype, void* stream) {
  NSID_REQUIRE(x && w && scale && shift && wf && out && B > 0 && B <= 65535 && H > 0 && W > 0 && NSID_DTYPE_OK(out_dtype));
  StemArgs a{};
  a.x = x; a.w = wf; a.bias = shift; a.out = out;
  a.H = H; a.W = W;
  a.Hc = (H - 1) / 2 + 1; a.Wc = (W - 1) / 2 + 1;
  a.Hp = (a.Hc - 1) / 2 + 1; a.Wp = (a.Wc - 1) / 2 + 1;
  NSID_REQUIRE(a.Hp <= 65535 && (long)B * a.Hp * a.Wp < (1L << 31) / 64);
  nsid_count(NSID_C_stem7_pool_train);
  hipStream_t s = static_cast<hipStream_t>(stream);
  NSID_LAUNCH(stem7_fold_kernel, dim3((64 * 49 + 255) / 256), dim3(256), 0, s, w, scale, wf);
  const dim3 grid((a.Wp + ST_PW - 1) / ST_PW, a.Hp, B);
  NSID_DISPATCH_DTYPE(out_dtype, T, NSID_LAUNCH(stem7_pool_kernel<T>, grid, dim3(256), 0, s, a));
  return nsid_launch_status();
}

extern "C" int nsid_stem7_bwd(const void* dpool, int dpool_dtype, const float* x, int B, int H, int W, const float* w,
                              const float* scale, const float* shift, const float* mean, const float* invstd, const float* gamma,
                              float* ws, float* dw, float* dgamma, float* dbeta, void* stream) {
  NSID_REQUIRE(dpool && x && w && scale && shift && mean && invstd && gamma && ws && dw && dgamma && dbeta);
  NSID_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && NSID_DTYPE_OK(dpool_dtype));
  StemTrainArgs a{};
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.mean = mean; a.invstd = invstd; a.dpool = dpool; a.part = ws;
  stem_train_dims(a, H, W);
  NSID_REQUIRE(a.Hp <= 65535 && (long)B * a.Hp * a.Wp < (1L << 31) / 64);
  a.ntiles = B * a.Hp * a.tiles_w;
  const int nset = (int)nsid_stem7_partials((long)B * a.Hp, a.Wp, 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  nsid_count(NSID_C_stem7_bwd);
  NSID_DISPATCH_DTYPE(dpool_dtype, T, NSID_LAUNCH(stem7_bwd_kernel<T>, dim3((unsigned)nset), dim3(256), 0, s, a));
  NSID_LAUNCH(stem7_bwd_finalize_kernel, dim3(49), dim3(256), 0, s, ws, nset, (double)B * a.Hc * a.Wc, gamma, invstd, dw, dgamma,
              dbeta);
  return nsid_launch_status();
}

extern "C" int nsid_gem_pool_fwd(const void* x, int B, int HW, int C, const float* p, float eps, float* out, int x_dtype,
                                 void* stream) {
  NSID_REQUIRE(x && p && out && B > 0 && B <= 65535 && HW > 0 && C > 0 && C % 64 == 0 && eps > 0.f && NSID_DTYPE_OK(x_dtype));
  nsid_count(NSID_C_gem_pool);
  NSID_DISPATCH_DTYPE(x_dtype, T, NSID_LAUNCH(gem_pool_kernel<T>, dim3(C / 64, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                                              static_cast<const T*>(x), HW, C, p, eps, out));
  return nsid_launch_status();
}

extern "C" int nsid_gem_pool_bwd(const void* x, const float* dy, int B, int HW, int C, const float* p, float eps, float* dx,
                                 float* dp_part, float* dp, int x_dtype, void* stream) {
  NSID_REQUIRE(x && dy && p && dx && dp_part && dp && B > 0 && B <= 65535 && HW > 0 && C > 0 && C % 64 == 0 && eps > 0.f);
  NSID_REQUIRE(NSID_DTYPE_OK(x_dtype) && (long)B * (C / 64) < (1L << 31));
  nsid_count(NSID_C_gem_pool_bwd);
  hipStream_t s = static_cast<hipStream_t>(stream);
  NSID_DISPATCH_DTYPE(x_dtype, T, NSID_LAUNCH(gem_pool_bwd_kernel<T>, dim3(C / 64, B), dim3(256), 0, s, static_cast<const T*>(x), dy,
                                              HW, C, p, eps, dx, dp_part));
  NSID_LAUNCH(gem_dp_sum_kernel, dim3(1), dim3(256), 0, s, dp_part, B * (C / 64), dp);
  return nsid_launch_status();
}

// ---- training: backward of the convolution and of IBN + ReLU, the batch statistics of a conv2d output, the block tail
extern "C" int nsid_conv2d_bwd_data(const void* dy, int B, int H, int W, int C, const void* wt, int w_dtype, const void* addend,
                                    void* dx, int Cout, int ksize, int stride, int act_dtype, void* stream) {
  NSID_REQUIRE(dy && wt && dx && B > 0 && H > 0 && W > 0 && C > 0 && Cout > 0 && NSID_DTYPE_OK(act_dtype));
  NSID_REQUIRE(w_dtype == act_dtype);
  NSID_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2));
  NSID_REQUIRE(C % (act_dtype == NSID_BF16 ? 32 : 16) == 0 && Cout % CV_BN == 0);
  NSID_REQUIRE(nsid_aligned16(dy) && nsid_aligned16(wt) && nsid_aligned16(dx) && nsid_aligned16(addend));
  const int pad = ksize / 2;
  ConvArgs a{};                                  // the roles of the two maps are swapped: see conv2d_kernel<T, true>
  a.x = dy; a.w = wt; a.bias = nullptr; a.addend = addend; a.out = dx;
  a.B = B;
  a.H = (H + 2 * pad - ksize) / stride + 1;      // the map that is gathered from: the conv's output
  a.W = (W + 2 * pad - ksize) / stride + 1;
  a.C = Cout;                                    // the reduction runs over (tap, output channel)
  a.Ho = H; a.Wo = W; a.Co = C;                  // the rows that are written: the conv's input
  a.KW = ksize; a.taps = ksize * ksize; a.stride = stride; a.pad = pad;
  a.relu = 0;
  const long M = (long)B * H * W;
  NSID_REQUIRE(M < (1L << 31) / 2);
  a.M = (int)M;
  a.tiles_n = (C + CV_BN - 1) / CV_BN;
  const long wgs = ((M + CV_BM - 1) / CV_BM) * a.tiles_n;
  NSID_REQUIRE(wgs < (1L << 31) - 1);
  nsid_count(NSID_C_conv2d_bwd_data);
  NSID_DISPATCH_DTYPE(act_dtype, T,
                      NSID_LAUNCH((conv2d_kernel<T, true>), dim3((unsigned)wgs), dim3(256), 0, static_cast<hipStream_t>(stream), a));
  return nsid_launch_status();
}

// row splits of nsid_conv2d_bwd_weight: enough workgroups for two per CU, at least 256 rows each; a function of the output rows and
// the weight elements alone, so that nsid_workspace_bytes can answer from those two
extern "C" int nsid_conv2d_wgrad_splits(long M, long welems) {
  const long tiles = welems / (128 * 128) > 0 ? welems / (128 * 128) : 1;
  long s = (512 + tiles - 1) / tiles;
  const long cap = (M + 255) / 256;
  if (s > cap) s = cap;
  if (s > 64) s = 64;
  return (int)(s < 1 ? 1 : s);
}

extern "C" int nsid_conv2d_bwd_weight(const void* dy, const void* x, int B, int H, int W, int C, float* dw, float* ws, int Cout,
                                      int ksize, int stride, int act_dtype, void* stream) {
  NSID_REQUIRE(dy && x && dw && B > 0 && H > 0 && W > 0 && C > 0 && Cout > 0 && NSID_DTYPE_OK(act_dtype));
  NSID_REQUIRE((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2));
  NSID_REQUIRE(C % (act_dtype == NSID_BF16 ? 32 : 16) == 0 && Cout % CV_BN == 0);
  NSID_REQUIRE(nsid_aligned16(dy) && nsid_aligned16(x) && nsid_aligned16(dw) && nsid_aligned16(ws));
  ConvWgArgs a{};
  a.dy = dy; a.x = x;
  a.H = H; a.W = W; a.C = C; a.Co = Cout;
  a.KW = ksize; a.taps = ksize * ksize; a.stride = stride; a.pad = ksize / 2;
  a.Ho = (H + 2 * a.pad - ksize) / stride + 1;
  a.Wo = (W + 2 * a.pad - ksize) / stride + 1;
  const long M = (long)B * a.Ho * a.Wo;
  NSID_REQUIRE(M < (1L << 31) / 2 && (long)B * H * W < (1L << 31) / 2);
  a.M = (int)M;
  a.tiles_c = (C + 127) / 128;
  const long welems = (long)Cout * a.taps * C;
  a.splits = nsid_conv2d_wgrad_splits(M, welems);
  NSID_REQUIRE(a.splits == 1 || ws != nullptr);
  const int KB = act_dtype == NSID_BF16 ? 32 : 16;
  const int nst = (int)((M + KB - 1) / KB);
  a.stages_per = (nst + a.splits - 1) / a.splits;
  a.out = a.splits > 1 ? ws : dw;
  const long tiles = (long)(Cout / 128) * a.taps * a.tiles_c;
  NSID_REQUIRE(tiles <= 65535);
  hipStream_t s = static_cast<hipStream_t>(stream);
  nsid_count(NSID_C_conv2d_bwd_weight);
  NSID_DISPATCH_DTYPE(act_dtype, T, NSID_LAUNCH(conv2d_wgrad_kernel<T>, dim3(a.splits, (unsigned)tiles), dim3(256), 0, s, a));
  if (a.splits > 1) {
    const long n4 = welems / 4;
    NSID_LAUNCH(conv2d_wgrad_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, ws, a.splits, n4, dw);
  }
  return nsid_launch_status();
}

extern "C" int nsid_col_stat(const void* x, int ldx, int M, int C, float* stat, int dtype, void* stream) {
  NSID_REQUIRE(x && stat && M > 0 && C > 0 && C % 64 == 0 && ldx >= C && NSID_DTYPE_OK(dtype));
  const int tiles = (M + NSID_ROW_TILE - 1) / NSID_ROW_TILE;
  NSID_REQUIRE(tiles <= 65535);
  nsid_count(NSID_C_col_stat);
  NSID_DISPATCH_DTYPE(dtype, T, NSID_LAUNCH(col_stat_kernel<T>, dim3(C / 64, tiles), dim3(256), 0, static_cast<hipStream_t>(stream),
                                            static_cast<const T*>(x), (long)ldx, M, C, stat, tiles));
  return nsid_launch_status();
}

extern "C" int nsid_ibn_relu_bwd(const void* dy, const void* r, int B, int HW, int C, const float* in_gamma, const float* in_beta,
                                 float eps, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                 const float* bn_invstd, void* dr, float* ws, float* d_in_gamma, float* d_in_beta, float* d_bn_gamma,
                                 float* d_bn_beta, int dtype, void* stream) {
  NSID_REQUIRE(dy && r && dr && ws && in_gamma && in_beta && bn_scale && bn_shift && bn_mean && bn_invstd);
  NSID_REQUIRE(d_in_gamma && d_in_beta && d_bn_gamma && d_bn_beta && B > 0 && B <= 65535 && HW > 0 && C > 0);
  NSID_REQUIRE(NSID_DTYPE_OK(dtype) && C % (2 * IBN_CW) == 0 && eps >= 0.f);
  NSID_REQUIRE(nsid_aligned16(dy) && nsid_aligned16(r) && nsid_aligned16(dr));
  IbnBwdArgs a{};
  a.dy = dy; a.r = r; a.dr = dr; a.gamma = in_gamma; a.beta = in_beta; a.sc = bn_scale; a.sh = bn_shift; a.mean = bn_mean;
  a.invstd = bn_invstd; a.part = ws; a.coef = ws + 2L * B * C;
  a.B = B; a.HW = HW; a.C = C; a.eps = eps;
  hipStream_t s = static_cast<hipStream_t>(stream);
  nsid_count(NSID_C_ibn_relu_bwd);
  NSID_DISPATCH_DTYPE(dtype, T, NSID_LAUNCH(ibn_relu_bwd_kernel<T>, dim3(C / IBN_CW, B), dim3(256), 0, s, a));
  NSID_LAUNCH(ibn_bwd_finalize_kernel, dim3((C + 127) / 128), dim3(128), 0, s, a.part, B, HW, C, d_in_gamma, d_in_beta, d_bn_gamma,
              d_bn_beta, a.coef);
  NSID_DISPATCH_DTYPE(dtype, T, NSID_LAUNCH(ibn_bwd_bn_apply_kernel<T>, dim3(C / 2 / IBN_CW, B), dim3(256), 0, s, a));
  return nsid_launch_status();
}

static inline unsigned rn_stream_grid(long nchunks) {
  const long b = (nchunks + 255) / 256;
  return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b));         // capped, grid-stride
}

extern "C" int nsid_bn_add_relu_fwd(const void* r3, const float* scale3, const float* shift3, const void* identity,
                                    const float* scale_d, const float* shift_d, void* out, int M, int C, int dtype, void* stream) {
  NSID_REQUIRE(r3 && scale3 && shift3 && identity && out && M > 0 && C > 0 && NSID_DTYPE_OK(dtype));
  NSID_REQUIRE((scale_d == nullptr) == (shift_d == nullptr) && C % (dtype == NSID_BF16 ? 8 : 4) == 0);
  NSID_REQUIRE(nsid_aligned16(r3) && nsid_aligned16(identity) && nsid_aligned16(out));
  nsid_count(NSID_C_bn_add_relu);
  NSID_DISPATCH_DTYPE(dtype, T, {
    constexpr int U = 4;
    const int CV = C / Chunk<T>::N;
    const long nchunks = (long)M * CV;
    int g0 = CV, d256 = 256;                        // thread count: a multiple of the chunks per row
    while (d256 % 2 == 0 && g0 % 2 == 0) { d256 /= 2; g0 /= 2; }          // g0 = CV / gcd(CV, 256)
    long want = (nchunks + 256L * U - 1) / (256L * U);
    if (want > 2048) want = 2048;                   // this pass runs alone on its stream: it may take every wave slot
    const long grid = (want + g0 - 1) / g0 * g0;
    NSID_LAUNCH((bn_add_relu_kernel<T, U>), dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                static_cast<const T*>(r3), scale3, shift3, static_cast<const T*>(identity), scale_d, shift_d, static_cast<T*>(out),
                (long)M, CV);
  });
  return nsid_launch_status();
}

extern "C" int nsid_relu_bwd(const void* dy, const void* y, void* g, long n, int dtype, void* stream) {
  NSID_REQUIRE(dy && y && g && n > 0 && NSID_DTYPE_OK(dtype) && n % (dtype == NSID_BF16 ? 8 : 4) == 0);
  NSID_REQUIRE(nsid_aligned16(dy) && nsid_aligned16(y) && nsid_aligned16(g));
  nsid_count(NSID_C_relu_bwd);
  NSID_DISPATCH_DTYPE(dtype, T, {
    const long nchunks = n / Chunk<T>::N;
    NSID_LAUNCH(relu_bwd_kernel<T>, dim3(rn_stream_grid(nchunks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                static_cast<const T*>(dy), static_cast<const T*>(y), static_cast<T*>(g), nchunks);
  });
  return nsid_launch_status();
}
