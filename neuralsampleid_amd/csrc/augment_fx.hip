// The baseline's waveform effects for a batch of clips (include/nsid.h nsid_aug_compress / _biquad / _frames): what the reference's
// fx_util chain adds to Gain / TimeStretch / PitchShift (augment.hip) for arch 'resnet-ibn' -- Compressor and BandEQ on the sample
// stems, FrameLevelCorruption on the mix. modules/transformations.GPUBaselineWaveAugment chains them with the four launches of
// augment.hip; DESIGN.md "Baseline waveform augmentations" is the definition, tests/baseline_augment_oracle.py restates it.
//
//   nsid_aug_compress  the level follower g of fx_util.Compressor.apply, fp64, one wave per clip: the target level and the two
//                      products that do not depend on g are computed by all lanes for a block of samples, the recurrence walks
//                      the block serially, y = fp32(fp64(x) * g) is applied by all lanes
//   nsid_aug_biquad    up to 64 cascaded second-order sections (transposed direct form II, fp64), one wave per clip: lane s runs
//                      section s on sample k - s at step k and hands its output to lane s + 1: L + n_sec - 1 steps, not L * n_sec
//   nsid_aug_frames    frame duplicate / remove / silence as a gather over the mix gain * t1 + x_i
// A clip whose mode selects another transform is neither read nor written. Every per-clip parameter is clamped on the device into a
// range in which no index can leave a row; nothing depends on the batch a clip is in.
#include <math.h>

#include "nsid_common.h"

// Every result here is defined operation by operation (the compressor and the frame mix bit for bit, the cascade in sosfilt's order):
// no contraction into fused multiply-adds anywhere in this file (the library compiles with -ffp-contract=fast-honor-pragmas).
#pragma clang fp contract(off)

constexpr int FX_BLOCK = 1024;            // samples taken at a time (compressor, biquad): global memory is touched between blocks
                                          // only, so no load or store is outstanding while the serial loops run
constexpr int FX_PER = FX_BLOCK / NSID_WAVE;
constexpr int FX_MAX_SEC = NSID_AUG_FX_MAX_SECTIONS;    // sections per clip: one lane each
static_assert(NSID_AUG_FX_MAX_SECTIONS == NSID_WAVE, "one lane per section");
constexpr int FX_MAX_FRAMES = NSID_AUG_FX_MAX_FRAMES;   // frames per clip: one thread each
constexpr int FX_FR_THREADS = 256;
constexpr int FX_FR_PER = 4;              // output samples per thread of the frame gather

// the first cnt (<= FX_BLOCK) samples at src into LDS, zeros behind them: every load is issued before the first one is waited for
__device__ __forceinline__ void fx_stage(const float* __restrict__ src, const int cnt, const int lane, float* __restrict__ dst) {
  float r[FX_BLOCK / NSID_WAVE];
#pragma unroll
  for (int j = 0; j < FX_BLOCK / NSID_WAVE; ++j) {
    const int i = j * NSID_WAVE + lane;
    r[j] = i < cnt ? src[i] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < FX_BLOCK / NSID_WAVE; ++j) dst[j * NSID_WAVE + lane] = r[j];
}

// ---- compressor. threshold >= 0, ratio >= 1, attack / release in [0, 1]; a NaN becomes the lower end of its range.
struct FxCmp { double thr, ratio, att, rel; };
__device__ __forceinline__ FxCmp fx_cmp_params(const double* __restrict__ c) {
  return FxCmp{fmax(c[0], 0.0), fmax(c[1], 1.0), fmin(fmax(c[2], 0.0), 1.0), fmin(fmax(c[3], 0.0), 1.0)};
}

// A wave takes a block of 1 024 samples at a time, 16 per lane. What does not depend on g -- the target level t of a sample above the
// threshold and the products (1 - attack) t, (1 - release) t -- is computed by the sample's lane and left in LDS; the walk then visits
// the samples in order, every lane carrying the same g (the LDS reads are wave-uniform); lane l keeps the g of its samples and
// applies it. (Measured alternatives, docs/experiments.md: the three values read from the owning lane with v_readlane and a scalar
// branch over the samples below the threshold, and a select-free form with hold coefficients (1, 0) in LDS, were both slower.)

// one step of the follower: every operation rounded on its own, in the reference's order
__device__ __forceinline__ double fx_follow(const double g, const double t, const double pa, const double pr, const double att,
                                            const double rel) {
  const double ma = att * g, mr = rel * g;
  const double ga = ma + pa, gr = mr + pr;
  const double gn = g > t ? ga : gr;
  return t >= 0.0 ? gn : g;                // t = -1 marks a sample at or below the threshold: g is held
}

__global__ __launch_bounds__(NSID_WAVE) void aug_compress_kernel(const float* __restrict__ x, const long stride_x, const int L,
                                                                const int* __restrict__ mode1, const double* __restrict__ cmp,
                                                                float* __restrict__ out, const long stride_o) {
  __shared__ double st[FX_BLOCK], spa[FX_BLOCK], spr[FX_BLOCK];
  const int clip = blockIdx.x, lane = threadIdx.x;
  if (mode1[clip] != 1) return;
  const FxCmp p = fx_cmp_params(cmp + 4L * clip);
  const float* const xs = x + (long)clip * stride_x;
  float* const os = out + (long)clip * stride_o;
  double g = 1.0;
  for (int n0 = 0; n0 < L; n0 += FX_BLOCK) {
    float xr[FX_PER];
    {
      const double oma = 1.0 - p.att, omr = 1.0 - p.rel;
#pragma unroll
      for (int j = 0; j < FX_PER; ++j) {
        const int i = j * NSID_WAVE + lane, n = n0 + i;
        xr[j] = n < L ? xs[n] : 0.f;
        const double a = fabs((double)xr[j]);
        const bool above = n < L && a > p.thr;
        const double d = a - p.thr;
        const double q = d / p.ratio;
        const double t = p.thr + q;
        st[i] = above ? t : -1.0;
        spa[i] = oma * t;
        spr[i] = omr * t;
      }
    }
    __syncthreads();
    double gl[FX_PER];
#pragma unroll
    for (int j = 0; j < FX_PER; ++j) {
      gl[j] = g;
#pragma unroll 8
      for (int l = 0; l < NSID_WAVE; ++l) {
        const int i = j * NSID_WAVE + l;
        g = fx_follow(g, st[i], spa[i], spr[i], p.att, p.rel);      // every lane walks the same values
        if (lane == l) gl[j] = g;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FX_PER; ++j) {
      const int n = n0 + j * NSID_WAVE + lane;
      if (n < L) os[n] = (float)((double)xr[j] * gl[j]);
    }
  }
}

// ---- biquad cascade. The double a lane hands on travels as two 32-bit DPP moves (wave_shr:1: lane s reads lane s - 1). The input
// of 64 steps sits in one register per lane and the finished samples of 64 steps go back into one: no LDS on the chain.
// (Blocks of 1 024 steps are staged through LDS so that global memory is touched between blocks only.)
__device__ __forceinline__ double fx_from_lane_below(const double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int slo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xF, 0xF, false);
  const int shi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xF, 0xF, false);
  return __hiloint2double(shi, slo);
}

__global__ __launch_bounds__(NSID_WAVE) void aug_biquad_kernel(const float* __restrict__ x, const long stride_x, const int L,
                                                              const int* __restrict__ mode1, const double* __restrict__ sos,
                                                              const int S, const int* __restrict__ n_sec, float* __restrict__ out,
                                                              const long stride_o) {
  __shared__ float xin[FX_BLOCK], yout[FX_BLOCK];
  const int clip = blockIdx.x, lane = threadIdx.x;
  if (mode1[clip] != 0) return;
  const int ns = min(max(n_sec[clip], 0), S);
  const float* const xs = x + (long)clip * stride_x;
  float* const os = out + (long)clip * stride_o;
  if (ns == 0) {                            // no section: the samples as they are
    for (int n = lane; n < L; n += NSID_WAVE) os[n] = xs[n];
    return;
  }
  double b0 = 1.0, b1 = 0.0, b2 = 0.0, a1 = 0.0, a2 = 0.0, post = 1.0;       // lanes past the last section pass through, unread
  if (lane < ns) {
    const double* const c = sos + ((long)clip * S + lane) * 6;
    b0 = c[0]; b1 = c[1]; b2 = c[2]; a1 = c[3]; a2 = c[4]; post = c[5];
  }
  double z1 = 0.0, z2 = 0.0, o = 0.0;
  const int last = ns - 1;
  const long steps = (long)L + last;        // step k: lane s holds sample k - s; the last section finishes sample k - last
  for (long k0 = 0; k0 < steps; k0 += FX_BLOCK) {
    fx_stage(xs + k0, (int)max(0L, min((long)FX_BLOCK, L - k0)), lane, xin);      // past the clip: zeros push the last samples through
    __syncthreads();
    const int cnt = (int)min((long)FX_BLOCK, steps - k0);
    for (int c0 = 0; c0 < cnt; c0 += NSID_WAVE) {
      const float xv = xin[c0 + lane];      // lane l: the input of step k0 + c0 + l
      const int ccnt = min(NSID_WAVE, cnt - c0);
      float yv = 0.f;
      for (int i = 0; i < ccnt; ++i) {
        const float x0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, xv), i));
        const double below = fx_from_lane_below(o);
        const double u = lane == 0 ? (double)x0 : below;
        const double y = b0 * u + z1;
        z1 = (b1 * u - a1 * y) + z2;
        z2 = b2 * u - a2 * y;
        o = y * post;
        const float done = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, (float)o), last));
        if (lane == i) yv = done;
      }
      yout[c0 + lane] = yv;
    }
    __syncthreads();
    for (int i = lane; i < cnt; i += NSID_WAVE) {
      const long m = k0 + i - last;
      if (m >= 0) os[m] = yout[i];          // m < L: k0 + i < steps
    }
    __syncthreads();
  }
}

// ---- frame edits. ops bit 1: the frame twice, 2: dropped (wins over the others), 4: zeros (with bit 1: two frames of zeros).
__global__ __launch_bounds__(FX_FR_THREADS) void aug_frames_kernel(const float* __restrict__ x_i, const long stride_i,
                                                                  const float* __restrict__ t1, const long stride_t,
                                                                  const float* __restrict__ gain, const int L,
                                                                  const int* __restrict__ mode2, const int* __restrict__ frame_size,
                                                                  const int* __restrict__ frame_ops, const int F,
                                                                  float* __restrict__ out, const long stride_o) {
  __shared__ int start[FX_MAX_FRAMES + 1];          // start[f]: first output sample of frame f; start[nf]: the edited length
  const int clip = blockIdx.y, tid = threadIdx.x;
  const int md = mode2[clip];
  if (md < 2 || md > 4) return;
  const int lo = (L + F - 1) / F;                   // at most F frames
  const int fsz = min(max(frame_size[clip], lo), L);
  const int nf = (L + fsz - 1) / fsz;
  const int* const ops = frame_ops + (long)clip * F;
  int mine = 0;
  if (tid < nf) {
    const int len = min(fsz, L - tid * fsz), op = ops[tid];
    mine = (op & 2) ? 0 : (op & 1) ? 2 * len : len;
  }
  // inclusive scan over the frames (FX_MAX_FRAMES = FX_FR_THREADS), shifted by one on the way out
  start[tid + 1] = mine;
  if (tid == 0) start[0] = 0;
  __syncthreads();
  for (int d = 1; d < FX_FR_THREADS; d <<= 1) {
    const int v = tid >= d ? start[tid + 1 - d] : 0;
    __syncthreads();
    start[tid + 1] += v;
    __syncthreads();
  }
  const int total = start[nf];                      // <= 2 L < 2^31
  const float* const xi = x_i + (long)clip * stride_i;
  const float* const ts = t1 + (long)clip * stride_t;
  float* const os = out + (long)clip * stride_o;
  const float g = gain[clip];
#pragma unroll
  for (int j = 0; j < FX_FR_PER; ++j) {
    const long nl = ((long)blockIdx.x * FX_FR_PER + j) * FX_FR_THREADS + tid;
    if (nl >= L) break;
    const int n = (int)nl;
    float v = 0.f;
    if (n < total) {
      int a = 0, b = nf;                            // start[a] <= n < start[b]
      while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (start[m] <= n) a = m; else b = m;
      }
      const int len = min(fsz, L - a * fsz);
      int off = n - start[a];
      if (off >= len) off -= len;                   // the second copy of a doubled frame
      if (!(ops[a] & 4)) {
        const int src = a * fsz + off;              // < L
        const float pg = g * ts[src];
        v = pg + xi[src];
      }
    }
    os[n] = v;
  }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static inline bool fx_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

extern "C" int nsid_aug_compress(const float* x, long stride_x, int B, long L, const int* mode1, const double* cmp, float* out,
                                 long stride_o, void* stream) {
  NSID_REQUIRE(x && mode1 && cmp && out);
  NSID_REQUIRE(B >= 1 && L >= 1 && L < (1L << 30));
  NSID_REQUIRE(B == 1 || (stride_x >= L && stride_o >= L));
  NSID_REQUIRE(fx_aligned8(cmp));
  nsid_count(NSID_C_aug_compress);
  NSID_LAUNCH(aug_compress_kernel, dim3((unsigned)B), dim3(NSID_WAVE), 0, static_cast<hipStream_t>(stream), x, stride_x, (int)L, mode1,
              cmp, out, stride_o);
  return nsid_launch_status();
}

extern "C" int nsid_aug_biquad(const float* x, long stride_x, int B, long L, const int* mode1, const double* sos, int S,
                               const int* n_sec, float* out, long stride_o, void* stream) {
  NSID_REQUIRE(x && mode1 && sos && n_sec && out);
  NSID_REQUIRE(B >= 1 && L >= 1 && L < (1L << 30));
  NSID_REQUIRE(S >= 1 && S <= FX_MAX_SEC);
  NSID_REQUIRE(B == 1 || (stride_x >= L && stride_o >= L));
  NSID_REQUIRE(fx_aligned8(sos));
  nsid_count(NSID_C_aug_biquad);
  NSID_LAUNCH(aug_biquad_kernel, dim3((unsigned)B), dim3(NSID_WAVE), 0, static_cast<hipStream_t>(stream), x, stride_x, (int)L, mode1,
              sos, S, n_sec, out, stride_o);
  return nsid_launch_status();
}

extern "C" int nsid_aug_frames(const float* x_i, long stride_i, const float* t1, long stride_t, const float* gain, int B, long L,
                               const int* mode2, const int* frame_size, const int* frame_ops, int F, float* out, long stride_o,
                               void* stream) {
  NSID_REQUIRE(x_i && t1 && gain && mode2 && frame_size && frame_ops && out);
  NSID_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L < (1L << 30));
  NSID_REQUIRE(F >= 1 && F <= FX_MAX_FRAMES);
  NSID_REQUIRE(B == 1 || (stride_i >= L && stride_t >= L && stride_o >= L));
  nsid_count(NSID_C_aug_frames);
  const long per = (long)FX_FR_THREADS * FX_FR_PER;
  NSID_LAUNCH(aug_frames_kernel, dim3((unsigned)((L + per - 1) / per), (unsigned)B), dim3(FX_FR_THREADS), 0,
              static_cast<hipStream_t>(stream), x_i, stride_i, t1, stride_t, gain, (int)L, mode2, frame_size, frame_ops, F, out,
              stride_o);
  return nsid_launch_status();
}
