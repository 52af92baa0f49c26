// Waveform augmentations for a batch of clips (include/nsid.h nsid_aug_*): the reference's GPUTransformSampleID(cpu=True) branch
// for arch 'grafp' -- Gain on the sample stems, then per clip a TimeStretch or a PitchShift of the mix -- as four launches:
//   nsid_aug_stft      gain * x_j + x_i -> STFT (n_fft 2 048, hop 512, periodic Hann, center / zero padding), (B, T_in, 1 025) complex
//   nsid_aug_vocoder   phase vocoder by the clip's rate -> (B, T_out, 1 025) complex, one thread per (clip, bin) walking the frames
//   nsid_aug_istft     inverse real FFT, window, overlap-add as a gather, / sum w^2, first n_fft/2 samples dropped -> n_s samples
//   nsid_aug_finish    stretch: cut / zero-fill to L;  pitch: band-limited resampling by the rate (tabulated Kaiser sinc), then to L
// The definition is DESIGN.md's "Waveform augmentations"; tests/augment_oracle.py restates it in fp64.
//
// Every index (frame positions, lengths, resampling positions) is fp64 arithmetic on r = (double)clamp(rate_f32, lo, hi); every
// sample and spectrum value is fp32. Grids and workspace extents come from the host-side bounds lo / hi only, and the kernels clamp
// the per-clip rate into them (fminf(fmaxf(x, lo), hi) maps a NaN to lo), so no parameter value can index outside a workspace.
// No atomics and a fixed summation order everywhere: a clip's result does not depend on the batch it is in.
//
// The 2 048-point real transform is a 1 024-point complex FFT of z[n] = x[2n] + i x[2n+1] plus the untangling pass, the scheme of
// frontend.hip one size up: the 1 024-point FFT is two 512-point FFTs (fft512.h) of the even and the odd elements and one radix-2
// pass, F[q] = E[q] + W1024^q O[q], F[q + 512] = E[q] - W1024^q O[q]. Twiddles: W2048^j, j < 2 048, from a host fp64 table.
#include <float.h>
#include <math.h>

#include "nsid_common.h"
#include "fft512.h"

constexpr int AG_N = NSID_AUG_N_FFT;      // n_fft
constexpr int AG_HOP = NSID_AUG_HOP;
constexpr int AG_M = AG_N / 2;            // complex points
constexpr int AG_BINS = AG_M + 1;
static_assert(AG_BINS == NSID_AUG_BINS, "include/nsid.h states the bins of a spectrum");
constexpr int AG_RUN = 8;                 // STFT: frames per workgroup
constexpr int AG_WAVES = 4;               // STFT: waves per workgroup
constexpr int AG_CH = 8;                  // inverse STFT: hops of output per (one-wave) workgroup
constexpr int AG_ZC = NSID_AUG_ZEROS;     // resampling filter: zero crossings,
constexpr int AG_TP = NSID_AUG_PRECISION; // table points per zero crossing
constexpr float AG_TWO_PI = 6.28318530717958647692f;
constexpr float AG_INV_TWO_PI = 0.15915494309189533577f;
constexpr float AG_HALF_PI = 1.57079632679489661923f;

FE_HD double ag_rate(const float* __restrict__ rate, const int clip, const float lo, const float hi) {
  return (double)fminf(fmaxf(rate[clip], lo), hi);
}
// frames after the vocoder and samples after the inverse STFT, as librosa counts them: len(arange(0, T_in, r)) and rint(L / r)
FE_HD long ag_frames_out(const long T_in, const double r) { return (long)ceil((double)T_in / r); }
FE_HD long ag_stretched(const long L, const double r) { return (long)rint((double)L / r); }
FE_HD float ag_wrap(const float d) { return d - AG_TWO_PI * rintf(d * AG_INV_TWO_PI); }

FE_HD void ag_load_twiddles(const int lane, const f32x2* __restrict__ tw, FeTw& t) {
  const int c = lane & 7;
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    t.t1[k - 1] = tw[(4 * lane * k) & (AG_N - 1)];        // W512^(lane k0)
    t.t2[k - 1] = tw[32 * c * k];                         // W64^(c k1), 32 * 49 < n_fft
  }
}

// 512-point FFT of the 8 elements a lane holds (v[a] = element lane + 64 a) -> v[k] = F[lane + 64 k]; buf: FE_BUF elements of LDS.
// Every wave of the workgroup calls it the same number of times (the barriers are workgroup-wide).
__device__ __forceinline__ void ag_fft512(const int lane, const FeTw& t, f32x2* v, f32x2* buf) {
  fe_radix8(v);
  buf[lane] = v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) buf[72 * k + lane] = fe_cmul(v[k], t.t1[k - 1]);
  __syncthreads();
  fe_read1(lane, buf, v);
  __syncthreads();
  fe_pass2(lane, t, v, buf);
  __syncthreads();
  fe_read2(lane, buf, v);
  __syncthreads();
  fe_radix8(v);
}
// 1 024-point FFT: e[a] = z[2 (lane + 64 a)], o[a] = z[2 (lane + 64 a) + 1] -> e[k] = F[q], o[k] = F[q + 512], q = lane + 64 k
__device__ __forceinline__ void ag_fft1024(const int lane, const FeTw& t, const f32x2* __restrict__ tw, f32x2* e, f32x2* o,
                                           f32x2* buf) {
  ag_fft512(lane, t, e, buf);
  ag_fft512(lane, t, o, buf);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const f32x2 wo = fe_cmul(o[k], tw[2 * (lane + 64 * k)]);
    o[k] = e[k] - wo;
    e[k] = e[k] + wo;
  }
}

// ---- stage 1: mix + STFT. A workgroup of four waves takes AG_RUN consecutive frames of one clip; the samples they cover are mixed
// and staged once in LDS (zero outside the clip: center=True with zero padding), a wave transforms one frame at a time.
__global__ __launch_bounds__(AG_WAVES* NSID_WAVE) void aug_stft_kernel(
    const float* __restrict__ x_i, const long stride_i, const float* __restrict__ x_j, const long stride_j,
    const float* __restrict__ gain, const int L, const int T, const int runs, const float* __restrict__ win,
    const f32x2* __restrict__ tw, f32x2* __restrict__ spec) {
  extern __shared__ __attribute__((aligned(16))) float ag_lds[];
  constexpr int span = (AG_RUN - 1) * AG_HOP + AG_N;
  f32x2* const bufs = reinterpret_cast<f32x2*>(ag_lds);                   // [AG_WAVES][AG_M]: exchange region, then Z
  float* const stage = ag_lds + 2 * AG_WAVES * AG_M;                      // [span]
  const int tid = threadIdx.x, lane = tid & (NSID_WAVE - 1), w = tid / NSID_WAVE;
  const int clip = blockIdx.x / runs, t0 = (blockIdx.x % runs) * AG_RUN;
  const float* xi = x_i + (long)clip * stride_i;
  const float* xj = x_j + (long)clip * stride_j;
  const float g = gain[clip];
  const int first = t0 * AG_HOP - AG_N / 2;                                // t0 * hop <= L: no overflow
  for (int i = tid; i < span; i += AG_WAVES * NSID_WAVE) {
    const int j = first + i;
    stage[i] = (j >= 0 && j < L) ? g * xj[j] + xi[j] : 0.f;
  }
  FeTw t;
  ag_load_twiddles(lane, tw, t);
  f32x2* const buf = bufs + w * AG_M;
  __syncthreads();
  for (int f = w; f < AG_RUN; f += AG_WAVES) {
    const float* fr = stage + f * AG_HOP;
    f32x2 e[8], o[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      const int i = 4 * (lane + 64 * a);
      const f32x4 x = *reinterpret_cast<const f32x4*>(fr + i), h = ld4(win + i);
      e[a] = f32x2{x[0] * h[0], x[1] * h[1]};
      o[a] = f32x2{x[2] * h[2], x[3] * h[3]};
    }
    ag_fft1024(lane, t, tw, e, o, buf);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      buf[lane + 64 * k] = e[k];
      buf[lane + 64 * k + AG_M / 2] = o[k];
    }
    __syncthreads();
    // untangling: with a = Z[k], b = Z[1024-k], 2E = a + conj b, 2O = -i (a - conj b): X[k] = E + W2048^k O and
    // X[1024-k] = conj(E - W2048^k O); frames past T compute on zeros and are not stored
    const int tf = t0 + f;
    if (tf < T) {
      f32x2* const dst = spec + ((long)clip * T + tf) * AG_BINS;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = lane + 64 * j;
        const f32x2 a = buf[k], b = buf[(AG_M - k) & (AG_M - 1)];
        const f32x2 ee = f32x2{a[0] + b[0], a[1] - b[1]};
        const f32x2 oo = f32x2{a[1] + b[1], b[0] - a[0]};
        const f32x2 wo = fe_cmul(oo, tw[k]);
        const f32x2 s = ee + wo, d = ee - wo;
        dst[k] = f32x2{0.5f * s[0], 0.5f * s[1]};
        dst[AG_M - k] = f32x2{0.5f * d[0], -0.5f * d[1]};
      }
      if (lane == 0) {
        const f32x2 m = buf[AG_M / 2];                    // X[512] = conj Z[512]
        dst[AG_M / 2] = f32x2{m[0], -m[1]};
      }
    }
    __syncthreads();
  }
}

// ---- stage 2: phase vocoder, one thread per (clip, bin). Output frame t reads the input columns c = floor(t r) and c + 1 (zero past
// the last one): magnitude interpolated, phase the running sum acc_{t+1} = acc_t + phi_k + wrap(angle D[c+1] - angle D[c] - phi_k)
// kept wrapped to [-pi, pi]; phi_k = 2 pi hop k / n_fft enters as its residue (k mod 4) pi / 2.
__global__ __launch_bounds__(256) void aug_vocoder_kernel(const f32x2* __restrict__ D, const int T_in,
                                                          const float* __restrict__ rate, const float lo, const float hi,
                                                          f32x2* __restrict__ out, const int T_max) {
  const int k = blockIdx.x * 256 + threadIdx.x, clip = blockIdx.y;
  if (k >= AG_BINS) return;
  const double r = ag_rate(rate, clip, lo, hi);
  const int T_out = (int)min(ag_frames_out(T_in, r), (long)T_max);
  const float phi = (float)(k & 3) * AG_HALF_PI;
  const f32x2* const d = D + (long)clip * T_in * AG_BINS + k;
  f32x2* const o = out + (long)clip * T_max * AG_BINS + k;
  const f32x2 first = d[0];
  float acc = atan2f(first[1], first[0]);
  for (int t = 0; t < T_out; ++t) {
    const double st = (double)t * r, fl = floor(st);
    const long c = (long)fl;
    const float a = (float)(st - fl);
    const f32x2 z = f32x2{0.f, 0.f};
    const f32x2 x0 = c < T_in ? d[c * AG_BINS] : z;
    const f32x2 x1 = c + 1 < T_in ? d[(c + 1) * AG_BINS] : z;
    const float m0 = sqrtf(x0[0] * x0[0] + x0[1] * x0[1]), m1 = sqrtf(x1[0] * x1[0] + x1[1] * x1[1]);
    const float mag = (1.0f - a) * m0 + a * m1;
    o[(long)t * AG_BINS] = f32x2{mag * cosf(acc), mag * sinf(acc)};
    const float dp = ag_wrap(atan2f(x1[1], x1[0]) - atan2f(x0[1], x0[0]) - phi);
    acc = ag_wrap(acc + phi + dp);
  }
}

// ---- stage 3: inverse STFT as a gather. A one-wave workgroup owns AG_CH hops of the (n_fft/2-padded) output and runs the frames that
// reach them in ascending order, each one an inverse real FFT (conj FFT conj of Z = E + i O, E = (X[k] + conj X[1024-k]) / 2,
// O = (X[k] - conj X[1024-k]) / 2 W2048^-k; the imaginary parts of X[0] and X[1024] are ignored, as a c2r transform does), windowed
// and added into LDS. An output sample is the sum of its <= 4 frames in frame order whatever the chunking, divided by the sum of the
// same frames' w^2 where that exceeds the smallest normal float.
__global__ __launch_bounds__(NSID_WAVE) void aug_istft_kernel(const f32x2* __restrict__ S, const int T_max, const int T_in, const int L,
                                                             const float* __restrict__ rate, const float lo, const float hi,
                                                             const float* __restrict__ win, const f32x2* __restrict__ tw,
                                                             float* __restrict__ wave, const long wave_stride, const int groups) {
  __shared__ f32x2 xs[AG_BINS + 1];
  __shared__ f32x2 buf[FE_BUF];
  __shared__ float acc[AG_CH * AG_HOP];
  const int lane = threadIdx.x;
  const int clip = blockIdx.x / groups, c0 = (blockIdx.x % groups) * AG_CH;
  const double r = ag_rate(rate, clip, lo, hi);
  const int T_out = (int)min(ag_frames_out(T_in, r), (long)T_max);
  const long n_s = min(ag_stretched(L, r), wave_stride);
  const long p0 = (long)c0 * AG_HOP;                                       // first padded position of this workgroup
  if (p0 >= AG_N / 2 + n_s) return;
  for (int i = lane; i < AG_CH * AG_HOP; i += NSID_WAVE) acc[i] = 0.f;
  FeTw t;
  ag_load_twiddles(lane, tw, t);
  const int tlo = max(0, c0 - 3), thi = min(T_out - 1, c0 + AG_CH - 1);
  __syncthreads();
  for (int tf = tlo; tf <= thi; ++tf) {
    const f32x2* const src = S + ((long)clip * T_max + tf) * AG_BINS;
    for (int k = lane; k < AG_BINS; k += NSID_WAVE) {
      f32x2 x = src[k];
      if (k == 0 || k == AG_M) x[1] = 0.f;
      xs[k] = x;
    }
    __syncthreads();
    f32x2 e[8], o[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = 2 * (lane + 64 * a) + h;
        const f32x2 xa = xs[q], xb = xs[AG_M - q], wq = tw[q];
        const f32x2 ee = f32x2{xa[0] + xb[0], xa[1] - xb[1]};
        const f32x2 dd = f32x2{xa[0] - xb[0], xa[1] + xb[1]};
        const f32x2 oo = f32x2{dd[0] * wq[0] + dd[1] * wq[1], dd[1] * wq[0] - dd[0] * wq[1]};      // dd * conj W2048^q
        const f32x2 zc = f32x2{ee[0] - oo[1], -(ee[1] + oo[0])};                                  // conj(2 Z[q])
        if (h == 0) e[a] = zc; else o[a] = zc;
      }
    }
    ag_fft1024(lane, t, tw, e, o, buf);
    // z[n] = conj F[n] / 2048: sample 2n = Re, sample 2n + 1 = -Im; frame sample i lands on padded position tf * hop + i
    const long base = (long)tf * AG_HOP - p0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int n = lane + 64 * k + h * (AG_M / 2);
        const f32x2 f = h == 0 ? e[k] : o[k];
        const f32x2 wv = *reinterpret_cast<const f32x2*>(win + 2 * n);
        const long pos = base + 2 * n;
        if (pos >= 0 && pos < AG_CH * AG_HOP) {                            // pos is even: the pair stays inside
          acc[pos] += (f[0] * (1.0f / AG_N)) * wv[0];
          acc[pos + 1] += (-f[1] * (1.0f / AG_N)) * wv[1];
        }
      }
    }
    __syncthreads();
  }
  for (int i = lane; i < AG_CH * AG_HOP; i += NSID_WAVE) {
    const long p = p0 + i, j = p - AG_N / 2;
    if (j < 0 || j >= n_s) continue;
    const int fhi = (int)min((long)(T_out - 1), p / AG_HOP);
    float wss = 0.f;
    for (int f = max(0, (int)(p / AG_HOP) - 3); f <= fhi; ++f) {
      const float wv = win[p - (long)f * AG_HOP];
      wss += wv * wv;
    }
    float v = acc[i];
    if (wss > FLT_MIN) v /= wss;
    wave[(long)clip * wave_stride + j] = v;
  }
}

// ---- stage 4: to L samples. Stretch clips copy; pitch clips resample by r: out[m] = c sum_j h(|m / r - j| c) s[j], c = min(1, r),
// h the tabulated filter (AG_ZC zero crossings, AG_TP points each, linear interpolation), one thread per output sample, j ascending.
__global__ __launch_bounds__(256) void aug_finish_kernel(const float* __restrict__ wave, const long wave_stride, const int L,
                                                         const int* __restrict__ mode, const float* __restrict__ rate, const float lo,
                                                         const float hi, const float* __restrict__ tab, float* __restrict__ out,
                                                         const long out_stride) {
  const int m = blockIdx.x * 256 + threadIdx.x, clip = blockIdx.y;
  if (m >= L) return;
  const double r = ag_rate(rate, clip, lo, hi);
  const long n_s = min(ag_stretched(L, r), wave_stride);
  const float* const s = wave + (long)clip * wave_stride;
  float v = 0.f;
  if (mode[clip] != 1) {
    if (m < n_s) v = s[m];
  } else if (m < (long)ceil((double)n_s * r)) {
    const double c = fmin(1.0, r), pos = (double)m / r, half = (double)AG_ZC / c, scale = c * (double)AG_TP;
    const long jlo = max(0L, (long)ceil(pos - half)), jhi = min(n_s - 1, (long)floor(pos + half));
    float sum = 0.f;
    for (long j = jlo; j <= jhi; ++j) {
      const double x = fabs(pos - (double)j) * scale;
      if (x < (double)(AG_ZC * AG_TP)) {
        const int i0 = (int)x;
        const float f = (float)(x - (double)i0), h0 = tab[i0], h1 = tab[i0 + 1];
        sum += (h0 + f * (h1 - h0)) * s[j];
      }
    }
    v = (float)c * sum;
  }
  out[(long)clip * out_stride + m] = v;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static inline bool ag_bounds_ok(const float lo, const float hi) { return lo > 0.f && lo <= hi; }      // false for NaN too

extern "C" int nsid_aug_stft(const float* x_i, long stride_i, const float* x_j, long stride_j, int B, long L, const float* gain,
                             const float* window, const float* twiddle, float* spec, void* stream) {
  NSID_REQUIRE(x_i && x_j && gain && window && twiddle && spec);
  NSID_REQUIRE(B >= 1 && L >= 1 && L < (1L << 30));
  NSID_REQUIRE(B == 1 || (stride_i >= L && stride_j >= L));
  NSID_REQUIRE((reinterpret_cast<uintptr_t>(twiddle) & 7u) == 0 && nsid_aligned16(window) && (reinterpret_cast<uintptr_t>(spec) & 7u) == 0);
  const long T = 1 + L / AG_HOP;
  const long runs = (T + AG_RUN - 1) / AG_RUN;
  NSID_REQUIRE(runs * B < (1L << 31));
  const size_t lds = sizeof(float) * (2 * AG_WAVES * AG_M + (AG_RUN - 1) * AG_HOP + AG_N);
  nsid_count(NSID_C_aug_stft);
  NSID_LAUNCH(aug_stft_kernel, dim3((unsigned)(runs * B)), dim3(AG_WAVES * NSID_WAVE), lds, static_cast<hipStream_t>(stream), x_i,
              stride_i, x_j, stride_j, gain, (int)L, (int)T, (int)runs, window, reinterpret_cast<const f32x2*>(twiddle),
              reinterpret_cast<f32x2*>(spec));
  return nsid_launch_status();
}

extern "C" int nsid_aug_vocoder(const float* spec, int B, long L, const float* rate, float rate_lo, float rate_hi, float* out,
                                long T_out_max, void* stream) {
  NSID_REQUIRE(spec && rate && out);
  NSID_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L < (1L << 30));
  NSID_REQUIRE(ag_bounds_ok(rate_lo, rate_hi));
  NSID_REQUIRE((reinterpret_cast<uintptr_t>(spec) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0);
  const long T = 1 + L / AG_HOP;
  NSID_REQUIRE(T_out_max >= ag_frames_out(T, (double)rate_lo) && T_out_max < (1L << 31));
  nsid_count(NSID_C_aug_vocoder);
  NSID_LAUNCH(aug_vocoder_kernel, dim3((AG_BINS + 255) / 256, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
              reinterpret_cast<const f32x2*>(spec), (int)T, rate, rate_lo, rate_hi, reinterpret_cast<f32x2*>(out), (int)T_out_max);
  return nsid_launch_status();
}

extern "C" int nsid_aug_istft(const float* spec, long T_out_max, int B, long L, const float* rate, float rate_lo, float rate_hi,
                              const float* window, const float* twiddle, float* wave, long wave_stride, void* stream) {
  NSID_REQUIRE(spec && rate && window && twiddle && wave);
  NSID_REQUIRE(B >= 1 && L >= 1 && L < (1L << 30));
  NSID_REQUIRE(ag_bounds_ok(rate_lo, rate_hi));
  NSID_REQUIRE((reinterpret_cast<uintptr_t>(twiddle) & 7u) == 0 && (reinterpret_cast<uintptr_t>(window) & 7u) == 0 &&
               (reinterpret_cast<uintptr_t>(spec) & 7u) == 0);
  const long T = 1 + L / AG_HOP;
  NSID_REQUIRE(T_out_max >= ag_frames_out(T, (double)rate_lo) && T_out_max < (1L << 31));
  const long s_max = ag_stretched(L, (double)rate_lo);
  NSID_REQUIRE(wave_stride >= s_max && s_max >= 1);
  const long groups = (AG_N / 2 + s_max + AG_CH * AG_HOP - 1) / (AG_CH * AG_HOP);
  NSID_REQUIRE(groups * B < (1L << 31));
  nsid_count(NSID_C_aug_istft);
  NSID_LAUNCH(aug_istft_kernel, dim3((unsigned)(groups * B)), dim3(NSID_WAVE), 0, static_cast<hipStream_t>(stream),
              reinterpret_cast<const f32x2*>(spec), (int)T_out_max, (int)T, (int)L, rate, rate_lo, rate_hi, window,
              reinterpret_cast<const f32x2*>(twiddle), wave, wave_stride, (int)groups);
  return nsid_launch_status();
}

extern "C" int nsid_aug_finish(const float* wave, long wave_stride, int B, long L, const int* mode, const float* rate,
                               float rate_lo, float rate_hi, const float* table, float* out, long out_stride, void* stream) {
  NSID_REQUIRE(wave && mode && rate && table && out);
  NSID_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L < (1L << 30));
  NSID_REQUIRE(ag_bounds_ok(rate_lo, rate_hi));
  NSID_REQUIRE(wave_stride >= ag_stretched(L, (double)rate_lo) && (B == 1 || out_stride >= L));
  nsid_count(NSID_C_aug_finish);
  NSID_LAUNCH(aug_finish_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), wave,
              wave_stride, (int)L, mode, rate, rate_lo, rate_hi, table, out, out_stride);
  return nsid_launch_status();
}
