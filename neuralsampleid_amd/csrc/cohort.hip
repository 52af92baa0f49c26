// Cohort score normalisation: the background statistics of fingerprint rows over a fixed cohort (include/nsid.h nsid_cohort_stats).
//
// A row's scores against the cohort are pair_sim's dots (csrc/align.hip): the same k-ordered fp32 fmaf chain on v_mfma_f32_32x32x2_f32,
// the split pairing up to d = 256 and the wide pairing above, so s_m has the bits pair_sim gives for the same two rows. Their sum and
// sum of squares are taken in fp64 in the one order the header states, which depends on the cohort alone: not on the rows of the
// call, on a row's place in it or on the launch.
//
// cohort_partial: one wave per (block of 32 rows, chunk of NSID_COHORT_CHUNK cohort rows). Lane (r, h) = (lane & 31, lane >> 5) holds
// row i0 + r as the A operand and cohort row m0 + 32 t + r as the B operand of tile t; accumulator register g of a tile is row
// i0 + (g & 3) + 8 (g >> 2) + 4 h against that cohort row. So a lane keeps, for each of its 16 rows, the fp64 sums of column class r
// over the chunk's tiles in ascending m; the 32 classes are combined by the xor butterfly (every lane of a half ends with the same
// bits: an fp64 add commutes), and the chunk's sums go to the workspace, [chunk][padded row][2] doubles. No atomics, no scratch.
//
// cohort_finalize: a thread per row adds the chunks in ascending order from chunk 0's value and forms mu and rs, every fp64 operation
// rounded once (no contraction).
#include "nsid_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CO_CHUNK = NSID_COHORT_CHUNK;
constexpr int CO_TILE = 32;
static_assert(CO_CHUNK % CO_TILE == 0, "a chunk is whole tiles");
static_assert(NSID_COHORT_MAX / CO_CHUNK <= 65535, "the chunks are the grid's y dimension");

bool cohort_d_ok(int d) { return (d % 16 == 0 && d >= 16 && d <= 256) || (d % 64 == 0 && d > 256 && d <= 2048); }
long cohort_pad_rows(long n) { return (n + CO_TILE - 1) / CO_TILE * CO_TILE; }

template <bool WIDE>
__global__ __launch_bounds__(64) void cohort_partial_kernel(const float* __restrict__ x, int ldx, int n, const float* __restrict__ cohort,
                                                            int ldc, int M, int d, double* __restrict__ ws, long n_pad) {
  const int lane = lane_id(), r = lane & 31, h = lane >> 5;
  const int i0 = CO_TILE * (int)blockIdx.x, chunk = (int)blockIdx.y, m0 = chunk * CO_CHUNK;
  if (i0 >= n || m0 >= M) return;                                // uniform; the host's grid has no such wave
  // rows past the call's end are read from its last row and never stored
  const float* xp = x + (size_t)min(i0 + r, n - 1) * ldx + (WIDE ? 0 : 4 * h);
  double sa[16], sb[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) sa[g] = sb[g] = 0.0;
  const int nb = d / 8;
  for (int t = 0; t < CO_CHUNK / CO_TILE; ++t) {
    const int m = m0 + CO_TILE * t + r;
    if (m - r >= M) break;                                       // uniform: the cohort ends inside this chunk
    // cohort rows past M are read from the last row and not summed
    const float* cp = cohort + (size_t)min(m, M - 1) * ldc + (WIDE ? 0 : 4 * h);
    f32x16 acc = {};
    if (!WIDE) {
      for (int b = 0; b < nb; b += 2) {                          // d % 16 == 0: two blocks' loads in flight per step
        const f32x4 a0 = ld4(xp + 8 * b), c0 = ld4(cp + 8 * b), a1 = ld4(xp + 8 * b + 8), c1 = ld4(cp + 8 * b + 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], c0[e], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], c1[e], acc, 0, 0, 0);
      }
    } else {
      for (int b = 0; b < nb; ++b) {
        const f32x4 a0 = ld4(xp + 8 * b), a1 = ld4(xp + 8 * b + 4), c0 = ld4(cp + 8 * b), c1 = ld4(cp + 8 * b + 4);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a0[1] : a0[0], h ? c0[1] : c0[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a0[3] : a0[2], h ? c0[3] : c0[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a1[1] : a1[0], h ? c1[1] : c1[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h ? a1[3] : a1[2], h ? c1[3] : c1[2], acc, 0, 0, 0);
      }
    }
    if (m < M) {
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const double s = (double)acc[g];
        sa[g] += s;
        sb[g] = fma(s, s, sb[g]);                                // s * s is exact in fp64: the same number as sb + s * s
      }
    }
  }
  // the 32 column classes: a[r] += a[r ^ dist]; dist < 32 stays inside the lane's half
#pragma unroll
  for (int dist = 1; dist < CO_TILE; dist <<= 1) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      sa[g] += __shfl_xor(sa[g], dist, NSID_WAVE);
      sb[g] += __shfl_xor(sb[g], dist, NSID_WAVE);
    }
  }
  // lane (r = g, h) stores register g: row i0 + (g & 3) + 8 (g >> 2) + 4 h (the padded rows exist in the workspace)
  double* wp = ws + ((size_t)chunk * n_pad + i0 + 4 * h) * 2;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    if (r == g) {
      double* o = wp + 2 * ((g & 3) + 8 * (g >> 2));
      o[0] = sa[g];
      o[1] = sb[g];
    }
  }
}

__global__ __launch_bounds__(256) void cohort_finalize_kernel(const double* __restrict__ ws, int n, long n_pad, int nchunks, int M,
                                                              float* __restrict__ mu, float* __restrict__ rs) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double A = ws[2 * i], B = ws[2 * i + 1];
  for (int c = 1; c < nchunks; ++c) {
    const double* p = ws + ((size_t)c * n_pad + i) * 2;
    A += p[0];
    B += p[1];
  }
  const double m64 = A / (double)M;
  const double sq = m64 * m64;
  const double var = fmax(B / (double)M - sq, 1e-12);
  mu[i] = (float)m64;
  rs[i] = (float)(1.0 / sqrt(var));
}

}  // namespace

// the bytes of nsid_cohort_stats' workspace for n rows against a cohort of M rows (nsid_workspace_bytes("cohort_stats", n, M))
long nsid_cohort_ws_bytes(long n, long M) {
  return (M + CO_CHUNK - 1) / CO_CHUNK * cohort_pad_rows(n) * 2 * (long)sizeof(double);
}

extern "C" int nsid_cohort_stats(const float* x, int ldx, int n, const float* cohort, int ldc, int M, int d, float* mu, float* rs,
                                 void* ws, void* stream) {
  NSID_REQUIRE(cohort_d_ok(d) && n >= 0 && M >= NSID_COHORT_MIN && M <= NSID_COHORT_MAX);
  if (n == 0) return NSID_OK;
  NSID_REQUIRE(x && cohort && mu && rs && ws);
  NSID_REQUIRE(ldx >= d && ldx % 4 == 0 && ldc >= d && ldc % 4 == 0 && nsid_aligned16(x) && nsid_aligned16(cohort));
  NSID_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(mu) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(rs) & 3u) == 0);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nchunks = (M + CO_CHUNK - 1) / CO_CHUNK;
  const long n_pad = cohort_pad_rows(n);
  const dim3 grid((unsigned)(n_pad / CO_TILE), (unsigned)nchunks);
  double* w = static_cast<double*>(ws);
  nsid_count(NSID_C_cohort_stats);
  if (d > 256) {
    NSID_LAUNCH(cohort_partial_kernel<true>, grid, dim3(64), 0, st, x, ldx, n, cohort, ldc, M, d, w, n_pad);
  } else {
    NSID_LAUNCH(cohort_partial_kernel<false>, grid, dim3(64), 0, st, x, ldx, n, cohort, ldc, M, d, w, n_pad);
  }
  NSID_LAUNCH(cohort_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, n, n_pad, nchunks, M, mu, rs);
  return nsid_launch_status();
}
