// Stem pairs for a batch of clips from a device-resident bank of resampled tracks (include/nsid.h nsid_resample_sinc,
// nsid_stem_pairs_gate / _build): the per-sample DSP of the reference's NeuralSampleIDDataset.__getitem__ (modules/data.py:45-150)
// behind the decoder. modules/data.py (StemBank, GPUStemPairSampler, GPUResample) owns the buffers and the draws; DESIGN.md "Stem
// pairs" is the definition, tests/stem_pairs_oracle.py restates it.
//
//   nsid_resample_sinc     torchaudio's Resample(orig, new) (sinc_interp_hann, width 6, rolloff 0.99) with the mono downmix on the load:
//                          the polyphase table is walked over its live taps only and sits in LDS
//   nsid_stem_pairs_gate   one workgroup per candidate clip: the SNR gate over the W = L + O samples of the three stems (fp64 sums),
//                          the random split into x_i / x_j, the silence test over the two crops -> status, snr and the split plan
//   nsid_stem_pairs_build  writes the two crops: row c of a (N, L) pair (rejected rows zero), or packed -- the accepted candidates in
//                          order in the first rows of a (B, L) pair, zeros behind them, and their count
// Every per-clip parameter is clamped on the device into a range in which no index can leave the clip's track, and a track whose
// table entry does not lie inside the bank is rejected (status 3), not read. No atomics; nothing depends on the batch a clip is in.
#include <math.h>

#include "nsid_common.h"

// The sampler's outputs are defined operation by operation; the resampler's accumulation uses explicit fmaf.
#pragma clang fp contract(off)

// ---- resampler -----------------------------------------------------------------------------------------------------------------------
constexpr int RS_THREADS = 256;
constexpr int RS_PER = 16;                           // outputs per thread: a workgroup stages the table once for 4 096 outputs
constexpr int RS_TILE = RS_THREADS * RS_PER;
constexpr int RS_MAX_C = NSID_RESAMPLE_MAX_C;
constexpr long RS_LDS_BYTES = NSID_RESAMPLE_LDS_BYTES;

// the mono sample j: the fp32 sum of the channels in channel order, divided by C
__device__ __forceinline__ float rs_mono(const float* __restrict__ x, const long stride_x, const int C, const float Cf, const long j) {
  float v = x[j];
  if (C > 1) {
    for (int c = 1; c < C; ++c) v = v + x[(long)c * stride_x + j];
    v = v / Cf;
  }
  return v;
}

__global__ __launch_bounds__(RS_THREADS) void resample_sinc_kernel(const float* __restrict__ x, const long stride_x, const int C,
                                                                  const long T, const int orig, const int nw, const int width,
                                                                  const float* __restrict__ table, const int* __restrict__ first,
                                                                  const int ntap, const int ts, float* __restrict__ y,
                                                                  const long T_out) {
  extern __shared__ float rs_lds[];                  // nw rows of ts floats (ts odd: phases of neighbouring lanes in different banks),
  int* const lfirst = reinterpret_cast<int*>(rs_lds + (long)nw * ts);       // then the first live tap of every phase
  const int tid = threadIdx.x;
  for (int i = tid; i < nw * ts; i += RS_THREADS) rs_lds[i] = table[i];
  for (int i = tid; i < nw; i += RS_THREADS) lfirst[i] = first[i];
  __syncthreads();
  const long n0 = (long)blockIdx.x * RS_TILE;
  const long q0 = n0 / nw;
  const int r0 = (int)(n0 - q0 * nw);
  const float Cf = (float)C;
#pragma unroll 1
  for (int k = 0; k < RS_PER; ++k) {
    const int l = k * RS_THREADS + tid;
    const long n = n0 + l;
    if (n >= T_out) break;
    const unsigned lr = (unsigned)(r0 + l);          // < nw + RS_TILE
    const unsigned dq = lr / (unsigned)nw;
    const int p = (int)(lr - dq * (unsigned)nw);
    const long j0 = (q0 + dq) * orig + lfirst[p] - width;     // index into x of the phase's first live tap
    const float* const row = rs_lds + p * ts;
    float acc = 0.f;
    if (j0 >= 0 && j0 + ntap <= T) {
      for (int i = 0; i < ntap; ++i) acc = fmaf(row[i], rs_mono(x, stride_x, C, Cf, j0 + i), acc);
    } else {
      for (int i = 0; i < ntap; ++i) {
        const long j = j0 + i;
        const float v = (j >= 0 && j < T) ? rs_mono(x, stride_x, C, Cf, j) : 0.f;       // the zero padding of both ends
        acc = fmaf(row[i], v, acc);
      }
    }
    y[n] = acc;
  }
}

// ---- sampler -------------------------------------------------------------------------------------------------------------------------
constexpr int SP_GATE_THREADS = 512;                 // one workgroup per clip streams 3 W floats; two workgroups fit a CU
constexpr int SP_GATE_WAVES = SP_GATE_THREADS / NSID_WAVE;
constexpr int SP_BUILD_THREADS = 256;
constexpr int SP_BUILD_PER = 16;
constexpr int SP_BUILD_CHUNK = SP_BUILD_THREADS * SP_BUILD_PER;
constexpr int SP_NONE = 3;                           // plan: no second addend of x_j

struct SpClip {
  const float* rows;                                 // the track's three rows, `len` apart
  int len, start;
};

// The clip's track and window, clamped: track into [0, n_tracks), start into [0, len - W]. false: the table entry lies outside the
// bank or the track is shorter than W -- nothing of it is read.
__device__ __forceinline__ bool sp_locate(const float* __restrict__ bank, const long bank_elems, const long* __restrict__ base,
                                          const int* __restrict__ length, const int n_tracks, const int track, const int start,
                                          const int W, SpClip& c) {
  const int t = min(max(track, 0), n_tracks - 1);
  const long b = base[t];
  const int len = length[t];
  if (len < W || b < 0 || b > bank_elems || 3L * len > bank_elems - b) return false;
  c.rows = bank + b;
  c.len = len;
  c.start = min(max(start, 0), len - W);
  return true;
}
__device__ __forceinline__ int sp_offset(const int off, const int O) { return min(max(off, 0), O - 1); }

// x_j at position m of the window: one stem, or the fp32 sum of two
__device__ __forceinline__ float sp_xj(const float* __restrict__ ra, const float* __restrict__ rb, const bool two, const int m) {
  const float a = ra[m];
  return two ? a + rb[m] : a;
}

__global__ __launch_bounds__(SP_GATE_THREADS) void stem_pairs_gate_kernel(
    const float* __restrict__ bank, const long bank_elems, const long* __restrict__ base, const int* __restrict__ length,
    const int n_tracks, const int* __restrict__ track, const int* __restrict__ start, const float* __restrict__ key,
    const int* __restrict__ off_i, const int* __restrict__ off_j, const int L, const int O, const float silence,
    int* __restrict__ status, float* __restrict__ snr, int* __restrict__ plan) {
  __shared__ double red[SP_GATE_WAVES][6];
  __shared__ float redm[SP_GATE_WAVES][2];
  __shared__ double tot6[6];
  __shared__ int sh_plan, sh_status;
  const int clip = blockIdx.x, tid = threadIdx.x, wave = tid / NSID_WAVE;
  const int W = L + O;
  SpClip c;
  if (!sp_locate(bank, bank_elems, base, length, n_tracks, track[clip], start[clip], W, c)) {      // uniform
    if (tid < 3) snr[3L * clip + tid] = __builtin_nanf("");
    if (tid == 0) { status[clip] = 3; plan[clip] = 0; }
    return;
  }
  const float* const r0 = c.rows + c.start;
  const float* const r1 = r0 + c.len;
  const float* const r2 = r1 + c.len;
  // gate: per stem c, sig = (s0 + s1 + s2) - s_c and d = sig - s_c, one fp32 operation each; the squares are exact in fp64
  double ps0 = 0.0, ps1 = 0.0, ps2 = 0.0, pn0 = 0.0, pn1 = 0.0, pn2 = 0.0;
#pragma unroll 4
  for (int n = tid; n < W; n += SP_GATE_THREADS) {
    const float s0 = r0[n], s1 = r1[n], s2 = r2[n];
    const float t01 = s0 + s1;
    const float tot = t01 + s2;
    const float g0 = tot - s0, g1 = tot - s1, g2 = tot - s2;
    const float d0 = g0 - s0, d1 = g1 - s1, d2 = g2 - s2;
    ps0 += (double)g0 * (double)g0;
    ps1 += (double)g1 * (double)g1;
    ps2 += (double)g2 * (double)g2;
    pn0 += (double)d0 * (double)d0;
    pn1 += (double)d1 * (double)d1;
    pn2 += (double)d2 * (double)d2;
  }
  ps0 = wave_sum_d(ps0); ps1 = wave_sum_d(ps1); ps2 = wave_sum_d(ps2);
  pn0 = wave_sum_d(pn0); pn1 = wave_sum_d(pn1); pn2 = wave_sum_d(pn2);
  if ((tid & (NSID_WAVE - 1)) == 0) {
    red[wave][0] = ps0; red[wave][1] = ps1; red[wave][2] = ps2;
    red[wave][3] = pn0; red[wave][4] = pn1; red[wave][5] = pn2;
  }
  __syncthreads();
  if (tid < 6) {
    double a = red[0][tid];
#pragma unroll 1
    for (int w = 1; w < SP_GATE_WAVES; ++w) a += red[w][tid];           // a fixed order: the same bits run to run
    tot6[tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    const double Wd = (double)W;
    const double floor_sum = 1e-8 * Wd;
    bool valid[3];
    float k[3];
    int nv = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double p_sig = tot6[e], p_n = tot6[3 + e];
      const double rhs = 0.1 * (p_n + floor_sum);
      valid[e] = p_sig >= rhs;
      nv += valid[e] ? 1 : 0;
      const double den = p_n / Wd + 1e-8;
      const double ratio = (p_sig / Wd) / den;
      snr[3L * clip + e] = p_sig == 0.0 ? -INFINITY : (float)(10.0 * log10(ratio));
      k[e] = key[3L * clip + e];
    }
    int st = 0, pl = 0;
    if (nv < 2) {
      st = 1;
    } else {
      // the valid stems by key ascending, ties to the lower index: the last one is x_i, the others are x_j
      int si = 0, oa = SP_NONE, ob = SP_NONE;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        int rank = 0;
#pragma unroll
        for (int f = 0; f < 3; ++f)
          if (f != e && valid[f] && (k[f] < k[e] || (k[f] == k[e] && f < e))) ++rank;
        if (valid[e] && rank == nv - 1) si = e;
      }
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (valid[e] && e != si) {
          if (oa == SP_NONE) oa = e; else ob = e;
        }
      pl = si | (oa << 2) | (ob << 4);
    }
    sh_status = st;
    sh_plan = pl;
  }
  __syncthreads();
  int st = sh_status;
  const int pl = sh_plan;
  if (st == 0) {                                     // uniform
    // silence: max |x_i|, max |x_j| over the two crops
    const int oi = sp_offset(off_i[clip], O), oj = sp_offset(off_j[clip], O);
    const float* const ri = r0 + (long)(pl & 3) * c.len + oi;
    const float* const ra = r0 + (long)((pl >> 2) & 3) * c.len + oj;
    const bool two = ((pl >> 4) & 3) != SP_NONE;
    const float* const rb = two ? r0 + (long)((pl >> 4) & 3) * c.len + oj : ra;
    float mi = 0.f, mj = 0.f;
#pragma unroll 4
    for (int n = tid; n < L; n += SP_GATE_THREADS) {
      mi = fmaxf(mi, fabsf(ri[n]));
      mj = fmaxf(mj, fabsf(sp_xj(ra, rb, two, n)));
    }
    mi = wave_max(mi);
    mj = wave_max(mj);
    if ((tid & (NSID_WAVE - 1)) == 0) { redm[wave][0] = mi; redm[wave][1] = mj; }
    __syncthreads();
    if (tid == 0) {
      float a = redm[0][0], b = redm[0][1];
      for (int w = 1; w < SP_GATE_WAVES; ++w) { a = fmaxf(a, redm[w][0]); b = fmaxf(b, redm[w][1]); }
      if (a < silence || b < silence) st = 2;
    }
  }
  if (tid == 0) { status[clip] = st; plan[clip] = pl; }
}

// grid.x: N candidate rows, then (packed) B_out tail rows; grid.y: chunks of SP_BUILD_CHUNK samples.
// Packed: an accepted candidate goes to row = the number of accepted candidates before it (rows >= B_out are dropped); tail row r is
// zero-filled iff r >= the number of accepted candidates. Every workgroup counts for itself: no atomics, no order between workgroups.
__global__ __launch_bounds__(SP_BUILD_THREADS) void stem_pairs_build_kernel(
    const float* __restrict__ bank, const long bank_elems, const long* __restrict__ base, const int* __restrict__ length,
    const int n_tracks, const int* __restrict__ track, const int* __restrict__ start, const int* __restrict__ off_i,
    const int* __restrict__ off_j, const int* __restrict__ status, const int* __restrict__ plan, const int N, const int L, const int O,
    const int packed, const int B_out, float* __restrict__ x_i, const long stride_i, float* __restrict__ x_j, const long stride_j,
    int* __restrict__ n_ok) {
  __shared__ int cnt[SP_BUILD_THREADS / NSID_WAVE][2];
  const int tid = threadIdx.x, c = blockIdx.x;
  const int n_lo = blockIdx.y * SP_BUILD_CHUNK;
  int before = 0, total = 0;
  if (packed) {
    const int upto = c < N ? c : N;
    for (int e = tid; e < N; e += SP_BUILD_THREADS) {
      const int ok = status[e] == 0 ? 1 : 0;
      total += ok;
      before += e < upto ? ok : 0;
    }
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o, 64); total += __shfl_xor(total, o, 64); }
    if ((tid & (NSID_WAVE - 1)) == 0) { cnt[tid / NSID_WAVE][0] = before; cnt[tid / NSID_WAVE][1] = total; }
    __syncthreads();
    before = total = 0;
    for (int w = 0; w < SP_BUILD_THREADS / NSID_WAVE; ++w) { before += cnt[w][0]; total += cnt[w][1]; }
  }
  int row;
  bool write_zero;
  if (c >= N) {                                      // tail row of the packed form
    row = c - N;
    if (row == 0 && blockIdx.y == 0 && tid == 0 && n_ok) *n_ok = min(total, B_out);
    if (row < total) return;
    write_zero = true;
  } else {
    SpClip cl;
    const bool ok = status[c] == 0 && sp_locate(bank, bank_elems, base, length, n_tracks, track[c], start[c], L + O, cl);
    if (packed) {
      if (!ok || before >= B_out) return;
      row = before;
      write_zero = false;
    } else {
      row = c;
      write_zero = !ok;
    }
    if (!write_zero) {
      const int pl = plan[c];
      const int oi = sp_offset(off_i[c], O), oj = sp_offset(off_j[c], O);
      const float* const r0 = cl.rows + cl.start;
      const float* const ri = r0 + (long)(pl & 3) * cl.len + oi;
      const float* const ra = r0 + (long)((pl >> 2) & 3) * cl.len + oj;
      const bool two = ((pl >> 4) & 3) != SP_NONE;
      const float* const rb = two ? r0 + (long)((pl >> 4) & 3) * cl.len + oj : ra;
      float* const oi_p = x_i + (long)row * stride_i;
      float* const oj_p = x_j + (long)row * stride_j;
#pragma unroll 4
      for (int k = 0; k < SP_BUILD_PER; ++k) {
        const int n = n_lo + k * SP_BUILD_THREADS + tid;
        if (n < L) {
          oi_p[n] = ri[n];
          oj_p[n] = sp_xj(ra, rb, two, n);
        }
      }
      return;
    }
  }
  float* const oi_p = x_i + (long)row * stride_i;
  float* const oj_p = x_j + (long)row * stride_j;
#pragma unroll 4
  for (int k = 0; k < SP_BUILD_PER; ++k) {
    const int n = n_lo + k * SP_BUILD_THREADS + tid;
    if (n < L) {
      oi_p[n] = 0.f;
      oj_p[n] = 0.f;
    }
  }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static inline bool sp_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

extern "C" int nsid_resample_sinc(const float* x, long stride_x, int C, long T, int orig, int nw, int width, const float* table,
                                  const int* first, int ntap, int ts, float* y, long T_out, void* stream) {
  NSID_REQUIRE(x && table && first && y);
  NSID_REQUIRE(C >= 1 && C <= RS_MAX_C && T >= 1 && T < (1L << 31));
  NSID_REQUIRE(C == 1 || stride_x >= T);
  NSID_REQUIRE(orig >= 1 && nw >= 1 && width >= 0 && ntap >= 1 && ts >= ntap && ntap <= 2L * width + orig);
  NSID_REQUIRE(((long)nw * ts + nw) * 4 <= RS_LDS_BYTES);
  NSID_REQUIRE(T_out == ((long)nw * T + orig - 1) / orig && T_out < (1L << 31));
  nsid_count(NSID_C_resample_sinc);
  const long grid = (T_out + RS_TILE - 1) / RS_TILE;
  NSID_LAUNCH(resample_sinc_kernel, dim3((unsigned)grid), dim3(RS_THREADS), (size_t)(((long)nw * ts + nw) * 4),
              static_cast<hipStream_t>(stream), x, stride_x, C, T, orig, nw, width, table, first, ntap, ts, y, T_out);
  return nsid_launch_status();
}

static inline bool sp_common_ok(const float* bank, long bank_elems, const long* base, const int* length, int n_tracks, int N, long L,
                                long O) {
  return bank && base && length && bank_elems >= 1 && n_tracks >= 1 && N >= 1 && N <= 65535 && L >= 1 && O >= 1 &&
         L + O < (1L << 30) && sp_aligned(base, 8);
}

extern "C" int nsid_stem_pairs_gate(const float* bank, long bank_elems, const long* base, const int* length, int n_tracks,
                                    const int* track, const int* start, const float* key, const int* off_i, const int* off_j, int N,
                                    long L, long O, float silence, int* status, float* snr, int* plan, void* stream) {
  NSID_REQUIRE(sp_common_ok(bank, bank_elems, base, length, n_tracks, N, L, O));
  NSID_REQUIRE(track && start && key && off_i && off_j && status && snr && plan);
  nsid_count(NSID_C_stem_pairs_gate);
  NSID_LAUNCH(stem_pairs_gate_kernel, dim3((unsigned)N), dim3(SP_GATE_THREADS), 0, static_cast<hipStream_t>(stream), bank, bank_elems,
              base, length, n_tracks, track, start, key, off_i, off_j, (int)L, (int)O, silence, status, snr, plan);
  return nsid_launch_status();
}

extern "C" int nsid_stem_pairs_build(const float* bank, long bank_elems, const long* base, const int* length, int n_tracks,
                                     const int* track, const int* start, const int* off_i, const int* off_j, const int* status,
                                     const int* plan, int N, long L, long O, int packed, int B_out, float* x_i, long stride_i,
                                     float* x_j, long stride_j, int* n_ok, void* stream) {
  NSID_REQUIRE(sp_common_ok(bank, bank_elems, base, length, n_tracks, N, L, O));
  NSID_REQUIRE(track && start && off_i && off_j && status && plan && x_i && x_j);
  NSID_REQUIRE(stride_i >= L && stride_j >= L);
  NSID_REQUIRE(packed == 0 || (packed == 1 && B_out >= 1 && B_out <= 65535 && n_ok));
  nsid_count(NSID_C_stem_pairs_build);
  const long rows = (long)N + (packed ? B_out : 0);
  const long chunks = (L + SP_BUILD_CHUNK - 1) / SP_BUILD_CHUNK;
  NSID_REQUIRE(chunks <= 65535);
  NSID_LAUNCH(stem_pairs_build_kernel, dim3((unsigned)rows, (unsigned)chunks), dim3(SP_BUILD_THREADS), 0,
              static_cast<hipStream_t>(stream), bank, bank_elems, base, length, n_tracks, track, start, off_i, off_j, status, plan, N,
              (int)L, (int)O, packed, B_out, x_i, stride_i, x_j, stride_j, n_ok);
  return nsid_launch_status();
}
