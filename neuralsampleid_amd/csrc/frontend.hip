// Batched log-mel front end in ONE launch (include/nsid.h nsid_logmel_fft): waveforms (B, L) -> log-mel (B, n_mels, T),
// T = 1 + L / hop = torchaudio MelSpectrogram(center=True / reflect, periodic Hann, power 2, HTK mel, norm None) +
// AmplitudeToDB(power), the `augment` of the reference's train.py:58 and, with B = 1, the evaluation branch
// (modules/transformations.py:27-34, :94-105).
//
// A workgroup of four waves takes a run of FE_RUN consecutive frames of one clip. The samples the run covers are staged once in
// LDS with the reflection done by index arithmetic on that load (no padded copy); a wave then transforms one frame at a time:
//   real FFT of the windowed 1 024-sample frame = 512-point complex FFT of z[n] = x[2n] + i x[2n+1] + the untangling pass.
//   512 = 8 x 8 x 8: three radix-8 passes in registers (8 points per lane), two transposes through LDS between them.
//   n = 64a + 8b + c, k = k0 + 8k1 + 64k2:  pass 1 sums over a (lane = 8b + c), twiddle W512^((8b+c) k0);
//                                           pass 2 sums over b (lane = 8k0 + c), twiddle W64^(c k1);
//                                           pass 3 sums over c (lane = k0 + 8k1) and leaves Z[k] in natural order.
//   untangling: with a = Z[k], b = Z[512-k], E = (a + conj b)/2, O = -i (a - conj b)/2: X[k] = E + W1024^k O and
//   X[512-k] = conj(E - W1024^k O), so one lane produces the power of bins k and 512-k from one pair of reads.
//   power -> mel sums over each band's non-zero bins -> 10 log10(max(., 1e-10)), collected per run in LDS and stored with the
//   frame index fastest.
// Neither the frame matrix nor the spectrum reaches global memory. Twiddles come from a table the host evaluates in fp64
// (W_n_fft^j, j < n_fft). No atomics: a clip's result does not depend on the batch it is in.
//
// LDS layout (8-byte complex elements; a ds_write_b64 is conflict-free when 16 consecutive lanes hit distinct elements mod 16, a
// ds_read_b64 when 32 consecutive lanes hit distinct elements mod 32, MI355X LDS banking):
//   transpose 1: element 72 k0 + 8b + c   written at lane 8b + c (consecutive), read at lane 8k0' + c' for each b: the row
//                pitch 72 = 64 + 8 moves the four k0' of a 32-lane group to four different 8-element bank octets;
//   transpose 2: element 66 c + k0 + 8k1  written at lane 8k0 + c for each k1 (pitch 66: 2c + k0 distinct mod 16), read at
//                lane k0 + 8k1 (consecutive);
//   spectrum:    element k = lane + 64 k2 (consecutive), read back at k and 512 - k.
// The power-of-two strides of the plain Stockham layout (64 and 8 elements) would be 4-way and 8-way conflicts.
#include "nsid_common.h"
#include "fft512.h"      // fe_cmul, fe_radix8, FeTw and the transposes: shared with augment.hip

constexpr int FE_N = 1024;                // n_fft of the tuned form
constexpr int FE_M = FE_N / 2;            // complex points
constexpr int FE_RUN = NSID_LOGMEL_RUN;   // frames per workgroup
constexpr int FE_WAVES = 4;

// the per-lane twiddles of the three passes (FeTw): constant over frames, loaded once per wave
FE_HD void fe_load_twiddles(const int lane, const f32x2* __restrict__ tw, FeTw& t) {
  const int c = lane & 7;
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    t.t1[k - 1] = tw[(2 * lane * k) & (FE_N - 1)];        // W512^(lane k0)
    t.t2[k - 1] = tw[16 * c * k];                         // W64^(c k1), 16 * 49 < n_fft
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) t.tu[j] = tw[lane + 64 * j];    // W1024^k, k = lane + 64 j
}

// pass 1: the windowed frame (fr = its first sample in the staged run) -> transpose 1
FE_HD void fe_pass1(const int lane, const float* fr, const float* __restrict__ win, const FeTw& t, f32x2* buf) {
  f32x2 v[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int i = 2 * (lane + 64 * a);
    v[a] = f32x2{fr[i] * win[i], fr[i + 1] * win[i + 1]};
  }
  fe_radix8(v);
  buf[lane] = v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) buf[72 * k + lane] = fe_cmul(v[k], t.t1[k - 1]);
}
// pass 3 -> Z[k] in natural order
FE_HD void fe_pass3(const int lane, f32x2* v, f32x2* buf) {
  fe_radix8(v);
#pragma unroll
  for (int k = 0; k < 8; ++k) buf[lane + 64 * k] = v[k];
}
// untangling: power of bins k = lane + 64 j and 512 - k (j < 4), and of bin 256 at lane 0
FE_HD void fe_untangle(const int lane, const f32x2* buf, const FeTw& t, float* plo, float* phi, float& pmid) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = lane + 64 * j;
    const f32x2 a = buf[k], b = buf[(FE_M - k) & (FE_M - 1)];
    // 2E and 2O: the halves are taken once on the power (exact), which also keeps a packed FMA with a constant multiplier out
    const f32x2 e = f32x2{a[0] + b[0], a[1] - b[1]};
    const f32x2 o = f32x2{a[1] + b[1], b[0] - a[0]};
    const f32x2 wo = fe_cmul(o, t.tu[j]);
    const f32x2 s = e + wo, d = e - wo;
    plo[j] = 0.25f * (s[0] * s[0] + s[1] * s[1]);
    phi[j] = 0.25f * (d[0] * d[0] + d[1] * d[1]);
  }
  const f32x2 m = buf[FE_M / 2];                      // X[256] = conj Z[256]
  pmid = m[0] * m[0] + m[1] * m[1];
}
FE_HD void fe_store_power(const int lane, const float* plo, const float* phi, const float pmid, float* pw) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = lane + 64 * j;
    pw[k] = plo[j];
    pw[FE_M - k] = phi[j];
  }
  if (lane == 0) pw[FE_M / 2] = pmid;
}
// mel sums over each band's non-zero bins, in bin order, and dB
FE_HD void fe_mel_db(const int lane, const float* pw, const float* __restrict__ fb, const int* __restrict__ band, const int n_mels,
                     float* dst) {
  for (int m = lane; m < n_mels; m += NSID_WAVE) {
    const float* row = fb + (long)m * (FE_M + 1);
    const int hi = band[2 * m + 1];
    float acc = 0.f;
    for (int f = band[2 * m]; f < hi; ++f) acc += row[f] * pw[f];
    dst[m] = 10.0f * log10f(fmaxf(acc, 1e-10f));       // AmplitudeToDB: amin 1e-10, ref 1.0
  }
}

// torch 'reflect' (no edge repeat) of sample index j into [0, L); indices of frames past the clip's last one are clamped
FE_HD int fe_reflect(int j, const int L) {
  j = j < 0 ? -j : j;
  j = j >= L ? 2 * (L - 1) - j : j;
  return j < 0 ? 0 : (j >= L ? L - 1 : j);
}

// one run: the frames t0 .. t0 + FE_RUN - 1 of the clip x (L samples, T frames) -> o[m * out_mel_stride + f], f < min(FE_RUN, T - t0).
// The whole workgroup calls it with the same arguments (it holds workgroup-wide barriers); both work maps below end in it.
__device__ __forceinline__ void fe_run(const float* __restrict__ x, const int L, const int hop, const int T, const int t0,
                                       const float* __restrict__ win, const f32x2* __restrict__ tw, const float* __restrict__ fb,
                                       const int* __restrict__ band, const int n_mels, float* __restrict__ o,
                                       const long out_mel_stride) {
  extern __shared__ __attribute__((aligned(16))) float fe_lds[];
  const int span = (FE_RUN - 1) * hop + FE_N;
  f32x2* const bufs = reinterpret_cast<f32x2*>(fe_lds);                   // [FE_WAVES][FE_BUF]
  float* const res = fe_lds + 2 * FE_WAVES * FE_BUF;                      // [FE_RUN][n_mels]
  float* const stage = res + FE_RUN * n_mels;                             // [span]
  const int tid = threadIdx.x, lane = tid & (NSID_WAVE - 1), w = tid / NSID_WAVE;
  const int first = t0 * hop - FE_N / 2;                                   // t0 * hop <= L: no overflow
  for (int i = tid; i < span; i += FE_WAVES * NSID_WAVE) stage[i] = x[fe_reflect(first + i, L)];
  FeTw t;
  fe_load_twiddles(lane, tw, t);
  f32x2* const buf = bufs + w * FE_BUF;
  float* const pw = reinterpret_cast<float*>(buf);
  __syncthreads();
  // every wave runs the same number of frames (the barriers are workgroup-wide); frames past T compute on clamped samples and
  // are not stored
  for (int f = w; f < FE_RUN; f += FE_WAVES) {
    f32x2 v[8];
    fe_pass1(lane, stage + f * hop, win, t, buf);
    __syncthreads();
    fe_read1(lane, buf, v);
    __syncthreads();
    fe_pass2(lane, t, v, buf);
    __syncthreads();
    fe_read2(lane, buf, v);
    __syncthreads();
    fe_pass3(lane, v, buf);
    __syncthreads();
    float plo[4], phi[4], pmid;
    fe_untangle(lane, buf, t, plo, phi, pmid);
    __syncthreads();
    fe_store_power(lane, plo, phi, pmid, pw);
    __syncthreads();
    fe_mel_db(lane, pw, fb, band, n_mels, res + f * n_mels);
    __syncthreads();
  }
  const int nf = min(FE_RUN, T - t0);
  for (int i = tid; i < n_mels * FE_RUN; i += FE_WAVES * NSID_WAVE) {
    const int m = i / FE_RUN, f = i % FE_RUN;
    if (f < nf) o[(long)m * out_mel_stride + f] = res[f * n_mels + m];
  }
}

__global__ __launch_bounds__(FE_WAVES* NSID_WAVE) void logmel_fft_kernel(
    const float* __restrict__ wave, const long in_stride, const int L, const int hop, const int T, const int runs,
    const float* __restrict__ win, const f32x2* __restrict__ tw, const float* __restrict__ fb, const int* __restrict__ band,
    const int n_mels, float* __restrict__ out, const long out_clip_stride, const long out_mel_stride) {
  const int clip = blockIdx.x / runs, t0 = (blockIdx.x % runs) * FE_RUN;
  fe_run(wave + (long)clip * in_stride, L, hop, T, t0, win, tw, fb, band, n_mels, out + (long)clip * out_clip_stride + t0,
         out_mel_stride);
}

// The same over a PACK of songs of different lengths (include/nsid.h nsid_logmel_fft_ragged): workgroup b takes run b - prefix_i of
// the song i with prefix_i <= b < prefix_(i+1), found by a bisection every lane of the workgroup makes alike (it depends on
// blockIdx alone). songs: NSID_PACK_COLS longs per song {first sample, samples, first output column, runs before the song}. A run
// stays inside its song: the reflection is by that song's length, and a song's columns are bit-equal to the song in a launch of
// its own.
__global__ __launch_bounds__(FE_WAVES* NSID_WAVE) void logmel_fft_ragged_kernel(
    const float* __restrict__ pack, const long* __restrict__ songs, const int n_songs, const int hop,
    const float* __restrict__ win, const f32x2* __restrict__ tw, const float* __restrict__ fb, const int* __restrict__ band,
    const int n_mels, float* __restrict__ out, const long ld) {
  const long b = blockIdx.x;
  const int i = nsid_pack_song(songs, n_songs, b);
  const long* sg = songs + (long)NSID_PACK_COLS * i;
  const int L = (int)sg[1], t0 = (int)(b - sg[3]) * FE_RUN;
  fe_run(pack + sg[0], L, hop, 1 + L / hop, t0, win, tw, fb, band, n_mels, out + sg[2] + t0, ld);
}

#ifndef FE_HOST_TEST
extern "C" int nsid_logmel_fft(const float* wave, long in_stride, int B, long L, int n_fft, int hop, const float* window,
                               const float* twiddle, const float* fb, const int* band, int n_mels, float* out,
                               long out_clip_stride, long out_mel_stride, void* stream) {
  NSID_REQUIRE(wave && window && twiddle && fb && band && out);
  NSID_REQUIRE(n_fft == FE_N);                                   // other sizes: refused before any launch
  NSID_REQUIRE(hop >= 1 && hop <= n_fft && B >= 1 && n_mels >= 1 && n_mels <= 1024);
  NSID_REQUIRE(L > n_fft / 2 && L < (1L << 30));                 // torch's reflect pad raises for L <= n_fft/2
  NSID_REQUIRE(B == 1 || in_stride >= L);
  NSID_REQUIRE((reinterpret_cast<uintptr_t>(twiddle) & 7u) == 0);
  const long T = 1 + L / hop;
  NSID_REQUIRE(out_mel_stride >= T && (B == 1 || out_clip_stride >= T));
  const long runs = (T + FE_RUN - 1) / FE_RUN;
  NSID_REQUIRE(runs * B < (1L << 31));
  const size_t lds = sizeof(float) * (2 * FE_WAVES * FE_BUF + (size_t)FE_RUN * n_mels + (FE_RUN - 1) * hop + FE_N);
  NSID_REQUIRE(lds <= 64 * 1024);
  nsid_count(NSID_C_logmel_fft);
  NSID_LAUNCH(logmel_fft_kernel, dim3((unsigned)(runs * B)), dim3(FE_WAVES * NSID_WAVE), lds, static_cast<hipStream_t>(stream),
              wave, in_stride, (int)L, hop, (int)T, (int)runs, window, reinterpret_cast<const f32x2*>(twiddle), fb, band, n_mels,
              out, out_clip_stride, out_mel_stride);
  return nsid_launch_status();
}

extern "C" int nsid_logmel_fft_ragged(const float* pack, const long* songs, int n_songs, long max_len, long total_runs,
                                      long total_cols, int n_fft, int hop, const float* window, const float* twiddle,
                                      const float* fb, const int* band, int n_mels, float* out, long ld, void* stream) {
  NSID_REQUIRE(pack && songs && window && twiddle && fb && band && out);
  NSID_REQUIRE(n_fft == FE_N);
  NSID_REQUIRE(hop >= 1 && hop <= n_fft && n_songs >= 1 && n_mels >= 1 && n_mels <= 1024);
  NSID_REQUIRE(max_len > n_fft / 2 && max_len < (1L << 30));
  NSID_REQUIRE((reinterpret_cast<uintptr_t>(twiddle) & 7u) == 0);
  NSID_REQUIRE(total_cols >= 1 && ld >= total_cols);
  NSID_REQUIRE(total_runs >= n_songs && total_runs < (1L << 31));
  const size_t lds = sizeof(float) * (2 * FE_WAVES * FE_BUF + (size_t)FE_RUN * n_mels + (FE_RUN - 1) * hop + FE_N);
  NSID_REQUIRE(lds <= 64 * 1024);
  nsid_count(NSID_C_logmel_fft_ragged);
  NSID_LAUNCH(logmel_fft_ragged_kernel, dim3((unsigned)total_runs), dim3(FE_WAVES * NSID_WAVE), lds,
              static_cast<hipStream_t>(stream), pack, songs, n_songs, hop, window, reinterpret_cast<const f32x2*>(twiddle), fb, band,
              n_mels, out, ld);
  return nsid_launch_status();
}
#endif
