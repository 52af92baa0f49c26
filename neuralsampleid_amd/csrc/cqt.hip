// Constant-Q transform of a batch of clips in ONE launch (include/nsid.h nsid_cqt): waveforms (B, L) -> magnitudes (B, n_bins, T),
// T = 1 + L / hop = nnAudio CQT1992v2(sr, hop_length, fmin 32.70, n_bins 84, bins_per_octave 12, norm 1, Hann, center=True /
// reflect, magnitude output, normalization_type 'librosa'), the input of the ResNet-IBN baseline (the reference's
// modules/transformations.py:36,48):
//   out[b][k][t] = sqrt(l_k) * | sum_n x_b[reflect(t hop + n - width/2)] taps_k[n] |,   taps_k non-zero on [start_k, start_k + l_k)
//
// Banded: bin lengths fall from 11 341 taps (bin 0, fs 22050) to 94 (bin 83), so the dense 84 x 16 384 complex matrix is 85 % zeros.
// The host sorts the bins into GROUPS of up to 8 neighbouring bins = 16 re/im columns of one 16-wide MFMA tile; a group's reduction
// runs over [first_tap, first_tap + extent) only, the support of its lowest (longest) bin. A workgroup takes (group, clip, CQ_F = 32
// consecutive frames); the grid is group-major with the longest group first, so the 100x spread of work per group is scheduled long
// items first.
//
// The reduction index is split by the hop: n = first_tap + q hop + r, 0 <= r < hop, so that
//   out[t][c] = sum_q sum_r X[t + q][r] H_q[r][c],     X[u][r] = x[reflect(u hop + r + first_tap - width/2)]
// and a sample row X[u] serves the frames t = u - q of every q. Per chunk of CQ_RC = 256 values of r the workgroup stages the rows
// u = t0 .. t0 + CQ_F + Q - 2 once in LDS (reflection by index arithmetic on that load: no padded copy, no frame matrix), and every
// row is then read by up to min(Q, CQ_F) frames x 16 columns. Products and sums are exact fp32 on the matrix cores
// (v_mfma_f32_16x16x4_f32: A = frames x taps from LDS, B = taps x columns straight from the packed table, which is L2-resident).
//   MFMA lane l: i = l & 15 (frame of the tile / column of the table), kq = l >> 4. Over the four MFMAs e = 0..3 of a step mm the
//   lane supplies r = r0 + 64 kq + 4 mm + e, i.e. ONE 16-byte read of each operand per four MFMAs.
//   The four waves of a workgroup split mm (wave w: mm = 4w .. 4w + 3) and each accumulates both 16-frame tiles, so a table fragment
//   feeds two MFMA chains; the four partial sums meet in LDS and are added in wave order (no atomics, nothing depends on B: clip b of
//   a batch is bit-equal to the clip alone). re/im never reach global memory: the epilogue scales by sqrt(l_k), takes the magnitude
//   and stores with the frame index fastest.
//
// Packed table (host, fp64 -> fp32 once): group g owns Q_g * hopP rows (hopP = hop rounded up to CQ_RC, Q_g = ceil(extent / hop)) of
// 16 columns (re, im of its bins; unused columns, r >= hop and taps outside a bin are zero), stored as [row / 4][column][row % 4] so
// that a lane's four e-values are one aligned 16-byte load and 16 lanes read 256 contiguous bytes. Zeros inside the extent are
// multiplied; the all-zero rows of the dense form (6.9x) are not.
//
// LDS layout (staged rows, pitch CQ_PITCH = 260 floats): consecutive frames are hop floats apart in the waveform, 0 modulo the bank
// count at hop 512, so a "lane = frame" read of a linear span would be a 16-way conflict. Here lane (i, kq) reads 16 bytes at float
// (16 ft + i + q) * 260 + 64 kq + 4 mm: the 16-byte slot (of the 16 in a 256-byte bank row) is (65 (16 ft + i + q) + 16 kq + mm)
// mod 16 = (i + q + mm) mod 16, independent of kq (that is why kq strides by 64 floats, not by 4) and distinct over the 16 values of i,
// so each of the four 16-lane groups of a ds_read_b128 — whatever mix of i and kq it holds — touches 16 distinct slots: conflict-free.
// The staging write is one float per lane at consecutive addresses (conflict-free, ds_write_b32).
#include "nsid_common.h"

constexpr int CQ_F = NSID_CQT_TILE;       // frames per workgroup (two 16-frame MFMA tiles)
constexpr int CQ_FT = CQ_F / 16;
constexpr int CQ_WAVES = 4;
constexpr int CQ_RC = NSID_CQT_RC;        // values of r per staged chunk: 4 kq x 16 mm x 4 e
constexpr int CQ_PITCH = CQ_RC + 4;       // floats per staged row
constexpr int CQ_COLS = 16;               // re/im columns of a group
static_assert(CQ_COLS == 2 * NSID_CQT_GROUP_BINS, "two columns per bin of a group");
constexpr int CQ_MAXG = 32;               // groups per launch (the descriptors travel in the kernel arguments)
constexpr int CQ_RED = CQ_WAVES * CQ_F * CQ_COLS;      // floats of the partial-sum exchange

struct CqGroup {                          // include/nsid.h: five ints per group
  int bin0, nbins, tap0, extent, table;   // table: offset of the group's first row in the packed table, in floats
};
struct CqArgs {
  int n;
  CqGroup g[CQ_MAXG];
};

// torch 'reflect' (no edge repeat) of sample index j into [0, L); indices of frames past the clip's last one are clamped
__device__ __forceinline__ int cq_reflect(int j, const int L) {
  j = j < 0 ? -j : j;
  j = j >= L ? 2 * (L - 1) - j : j;
  return j < 0 ? 0 : (j >= L ? L - 1 : j);
}

// one tile: the frames t0 .. t0 + CQ_F - 1 of the clip x (L samples, T frames) for the bins of group g ->
// o[(g.bin0 + b) * out_bin_stride + t0 + f], t0 + f < T (o: the clip's first output column). The whole workgroup calls it with the
// same arguments (it holds workgroup-wide barriers); both work maps below end in it.
__device__ __forceinline__ void cq_tile(const float* __restrict__ x, const int L, const int hop, const int hopP, const int half,
                                        const int T, const int t0, const CqGroup g, const float* __restrict__ taps,
                                        const float* __restrict__ scale, float* __restrict__ o, const long out_bin_stride) {
  extern __shared__ __attribute__((aligned(16))) float cq_lds[];
  float* const red = cq_lds;                              // [CQ_WAVES][CQ_F][CQ_COLS]
  float* const stage = cq_lds + CQ_RED;                   // [CQ_F + Q - 1][CQ_PITCH]
  const int tid = threadIdx.x, lane = tid & (NSID_WAVE - 1), w = tid / NSID_WAVE;
  const int Q = (g.extent - 1) / hop + 1;
  const int rows = CQ_F + Q - 1;
  const float* tbl = taps + g.table;
  const int i = lane & 15, kq = lane >> 4;
  const int base = t0 * hop + g.tap0 - half;              // sample of row 0, r = 0 (may be negative)

  f32x4 acc[CQ_FT];
#pragma unroll
  for (int ft = 0; ft < CQ_FT; ++ft) acc[ft] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int r0 = 0; r0 < hopP && r0 < g.extent; r0 += CQ_RC) {
    __syncthreads();                                      // the previous chunk has been consumed
    {
      const int r = r0 + tid;                             // CQ_RC == threads of the workgroup: one column per thread
      const bool live = r < hop;
      // s >= -width/2 > -L reflects into the clip; rows past the clip's frames (tile padding) clamp. The entry has checked that
      // every s fits an int. Eight independent loads are in flight per thread (the tail repeats the last row: same value, same slot).
      for (int u0 = 0; u0 < rows; u0 += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = x[cq_reflect(base + min(u0 + k, rows - 1) * hop + r, L)];
#pragma unroll
        for (int k = 0; k < 8; ++k) stage[min(u0 + k, rows - 1) * CQ_PITCH + tid] = live ? v[k] : 0.f;
      }
    }
    __syncthreads();
    // the q with a tap of this chunk inside the extent (the rows after them are all zero); the table fragments of q + 1 are
    // loaded before the MFMAs of q (the last iteration re-loads its own)
    const int Qc = (g.extent - r0 - 1) / hop + 1;
    const float* bq = tbl + ((long)(r0 + 64 * kq + 16 * w) * CQ_COLS + 4 * i);
    const float* aq = stage + i * CQ_PITCH + 64 * kq + 16 * w;
    const long bstep = (long)hopP * CQ_COLS;
    auto load_b = [&](const int q, f32x4* f) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) f[mi] = ld4(bq + min(q, Qc - 1) * bstep + mi * 4 * CQ_COLS);
    };
    auto mfma_q = [&](const int q, const f32x4* f) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int ft = 0; ft < CQ_FT; ++ft) {
          const f32x4 fa = *reinterpret_cast<const f32x4*>(aq + (q + ft * 16) * CQ_PITCH + 4 * mi);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[e], f[mi][e], acc[ft], 0, 0, 0);
        }
      }
    };
    f32x4 fb0[4], fb1[4];                                 // two fragment sets in turn: no register copies behind a load
    load_b(0, fb0);
    int q = 0;
    for (; q + 1 < Qc; q += 2) {
      load_b(q + 1, fb1);
      __builtin_amdgcn_sched_barrier(0);                  // the loads are issued here, a whole q ahead of their use
      mfma_q(q, fb0);
      __builtin_amdgcn_sched_barrier(0);
      load_b(q + 2, fb0);                                 // clamped to the last q: an odd count ends on fb0 below
      __builtin_amdgcn_sched_barrier(0);
      mfma_q(q + 1, fb1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (q < Qc) mfma_q(q, fb0);
  }
  // C/D map: column = lane & 15, row (frame) = 4 (lane >> 4) + reg
#pragma unroll
  for (int ft = 0; ft < CQ_FT; ++ft)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[(w * CQ_F + 16 * ft + 4 * kq + e) * CQ_COLS + i] = acc[ft][e];
  __syncthreads();
  {
#pragma clang fp contract(off)
    const int f = tid % CQ_F, b = tid / CQ_F;             // 256 threads = 32 frames x 8 bins, frame fastest
    if (b < g.nbins && t0 + f < T) {
      float re = 0.f, im = 0.f;
#pragma unroll
      for (int ww = 0; ww < CQ_WAVES; ++ww) {
        re += red[(ww * CQ_F + f) * CQ_COLS + 2 * b];
        im += red[(ww * CQ_F + f) * CQ_COLS + 2 * b + 1];
      }
      const float s = scale[g.bin0 + b];
      re = re * s;
      im = -im * s;
      o[(long)(g.bin0 + b) * out_bin_stride + t0 + f] = sqrtf(re * re + im * im);
    }
  }
}

__global__ __launch_bounds__(CQ_WAVES* NSID_WAVE) void cqt_kernel(
    const float* __restrict__ wave, const long in_stride, const int L, const int hop, const int hopP, const int half, const int T,
    const int tiles, const int B, const CqArgs ga, const float* __restrict__ taps, const float* __restrict__ scale,
    float* __restrict__ out, const long out_clip_stride, const long out_bin_stride) {
  const int per_group = B * tiles;
  const int gi = blockIdx.x / per_group, rest = blockIdx.x % per_group;
  const int clip = rest / tiles, t0 = (rest % tiles) * CQ_F;
  cq_tile(wave + (long)clip * in_stride, L, hop, hopP, half, T, t0, ga.g[gi], taps, scale, out + (long)clip * out_clip_stride,
          out_bin_stride);
}

// The same over a PACK of songs of different lengths (include/nsid.h nsid_cqt_ragged). The grid stays group-major with the longest
// group first; within a group, item b of the pack's `tiles` tiles belongs to the song i with prefix_i <= b < prefix_(i+1)
// (nsid_pack_song: a bisection that depends on blockIdx alone, so the workgroup's barriers stay uniform). A tile stays inside its
// song: the reflection is by that song's length, and a song's columns are bit-equal to the song in a launch of its own.
__global__ __launch_bounds__(CQ_WAVES* NSID_WAVE) void cqt_ragged_kernel(
    const float* __restrict__ pack, const long* __restrict__ songs, const int n_songs, const int tiles, const int hop,
    const int hopP, const int half, const CqArgs ga, const float* __restrict__ taps, const float* __restrict__ scale,
    float* __restrict__ out, const long ld) {
  const int gi = blockIdx.x / tiles;
  const long b = blockIdx.x % tiles;
  const int i = nsid_pack_song(songs, n_songs, b);
  const long* sg = songs + (long)NSID_PACK_COLS * i;
  const int L = (int)sg[1], t0 = (int)(b - sg[3]) * CQ_F;
  cq_tile(pack + sg[0], L, hop, hopP, half, 1 + L / hop, t0, ga.g[gi], taps, scale, out + sg[2], ld);
}

// the host array of group descriptors -> the kernel argument, checked against the table; qmax: the most hops a group's extent spans
static int cq_read_groups(const int* groups, const int n_groups, const int n_bins, const int hop, const int width,
                          const long taps_len, CqArgs& ga, int& qmax) {
  NSID_REQUIRE(n_groups >= 1 && n_groups <= CQ_MAXG);
  const long hopP = ((long)hop + CQ_RC - 1) / CQ_RC * CQ_RC;
  ga.n = n_groups;
  int next_bin = 0;
  qmax = 1;
  for (int k = 0; k < n_groups; ++k) {
    CqGroup& g = ga.g[k];
    g.bin0 = groups[5 * k]; g.nbins = groups[5 * k + 1]; g.tap0 = groups[5 * k + 2]; g.extent = groups[5 * k + 3];
    g.table = groups[5 * k + 4];
    NSID_REQUIRE(g.bin0 == next_bin && g.nbins >= 1 && g.nbins <= 8);      // the groups cover the bins once, in order
    NSID_REQUIRE(g.tap0 >= 0 && g.extent >= 1 && (long)g.tap0 + g.extent <= width);
    const long Q = ((long)g.extent - 1) / hop + 1;
    NSID_REQUIRE(g.table >= 0 && (g.table & 3) == 0 && (long)g.table + Q * hopP * CQ_COLS <= taps_len);
    NSID_REQUIRE(Q * hopP * CQ_COLS < (1L << 31));
    qmax = Q > qmax ? (int)Q : qmax;
    next_bin += g.nbins;
  }
  NSID_REQUIRE(next_bin == n_bins);
  for (int k = n_groups; k < CQ_MAXG; ++k) ga.g[k] = CqGroup{0, 0, 0, 0, 0};
  return NSID_OK;
}

extern "C" int nsid_cqt(const float* wave, long in_stride, int B, long L, int hop, int width, int n_bins, const int* groups,
                        int n_groups, const float* taps, long taps_len, const float* scale, float* out, long out_clip_stride,
                        long out_bin_stride, void* stream) {
  static_assert(CQ_RC == CQ_WAVES * NSID_WAVE && CQ_F * 8 == CQ_WAVES * NSID_WAVE, "one staged column and one output per thread");
  NSID_REQUIRE(wave && groups && taps && scale && out);
  NSID_REQUIRE(B >= 1 && hop >= 1 && n_bins >= 1 && width >= 2 && (width & 1) == 0);
  NSID_REQUIRE(L > width / 2 && L < (1L << 28) && hop < (1 << 24));        // torch's reflect pad raises for L <= width/2
  NSID_REQUIRE(in_stride >= L);
  NSID_REQUIRE(nsid_aligned16(taps));                                      // 16-byte table fragments
  const long hopP = ((long)hop + CQ_RC - 1) / CQ_RC * CQ_RC;
  CqArgs ga;
  int qmax;
  NSID_REQUIRE(cq_read_groups(groups, n_groups, n_bins, hop, width, taps_len, ga, qmax) == NSID_OK);
  const long T = 1 + L / hop;
  NSID_REQUIRE(out_bin_stride >= T && out_clip_stride >= (long)(n_bins - 1) * out_bin_stride + T);
  const long tiles = (T + CQ_F - 1) / CQ_F;
  NSID_REQUIRE(tiles * B * n_groups < (1L << 31));
  NSID_REQUIRE((tiles * CQ_F + qmax) * (long)hop + width < (1L << 31));     // staged sample indices stay in int range
  const size_t lds = sizeof(float) * (CQ_RED + (size_t)(CQ_F + qmax - 1) * CQ_PITCH);
  NSID_REQUIRE(lds <= 64 * 1024);                                          // a group's longest bin spans at most 24 hops
  nsid_count(NSID_C_cqt);
  NSID_LAUNCH(cqt_kernel, dim3((unsigned)(tiles * B * n_groups)), dim3(CQ_WAVES * NSID_WAVE), lds,
              static_cast<hipStream_t>(stream), wave, in_stride, (int)L, hop, (int)hopP, width / 2, (int)T, (int)tiles, B, ga, taps,
              scale, out, out_clip_stride, out_bin_stride);
  return nsid_launch_status();
}

extern "C" int nsid_cqt_ragged(const float* pack, const long* songs, int n_songs, long max_len, long total_tiles, long total_cols,
                               int hop, int width, int n_bins, const int* groups, int n_groups, const float* taps, long taps_len,
                               const float* scale, float* out, long ld, void* stream) {
  NSID_REQUIRE(pack && songs && groups && taps && scale && out);
  NSID_REQUIRE(n_songs >= 1 && hop >= 1 && n_bins >= 1 && width >= 2 && (width & 1) == 0);
  NSID_REQUIRE(max_len > width / 2 && max_len < (1L << 28) && hop < (1 << 24));     // the longest song of the pack
  NSID_REQUIRE(nsid_aligned16(taps));
  const long hopP = ((long)hop + CQ_RC - 1) / CQ_RC * CQ_RC;
  CqArgs ga;
  int qmax;
  NSID_REQUIRE(cq_read_groups(groups, n_groups, n_bins, hop, width, taps_len, ga, qmax) == NSID_OK);
  NSID_REQUIRE(total_cols >= 1 && ld >= total_cols);
  NSID_REQUIRE(total_tiles >= n_songs && total_tiles < (1L << 31) && total_tiles * n_groups < (1L << 31));
  const long tiles_max = (1 + max_len / hop + CQ_F - 1) / CQ_F;
  NSID_REQUIRE((tiles_max * CQ_F + qmax) * (long)hop + width < (1L << 31));  // staged sample indices stay in int range
  const size_t lds = sizeof(float) * (CQ_RED + (size_t)(CQ_F + qmax - 1) * CQ_PITCH);
  NSID_REQUIRE(lds <= 64 * 1024);
  nsid_count(NSID_C_cqt_ragged);
  NSID_LAUNCH(cqt_ragged_kernel, dim3((unsigned)(total_tiles * n_groups)), dim3(CQ_WAVES * NSID_WAVE), lds,
              static_cast<hipStream_t>(stream), pack, songs, n_songs, (int)total_tiles, hop, (int)hopP, width / 2, ga, taps, scale,
              out, ld);
  return nsid_launch_status();
}
