// Song-level vote of a query's search result (include/nsid.h nsid_song_vote / nsid_song_vote_clf / nsid_vote_candidates).
//
// Reference: eval.py:296-367 (the vote of eval_faiss on sequence scores) and eval_hr.py:85-156 (the vote of eval_faiss_clf on
// classifier scores): the candidates of a (start, length) pair are walked in the row-major order of its rows of I, every candidate
// that passes the rules adds its score to its song in a Python dict of floats, and the songs are ranked with a stable
// sorted(reverse=True). search.aggregate_hit_rates and rerank.vote_hit_rates_clf are the host forms.
//
// One workgroup per pair. The at most VOTE_MAX_CAND candidates of the pair are staged into LDS as (song code, fp64 value), 12 bytes
// each, -1 for a skipped candidate. A candidate is its song's LEADER when no earlier candidate has the same song; a leader sums its
// song's values from its own position on, in walk order and in fp64 from 0.0: the additions and their order are those of the
// dict, so the totals are the host's bit for bit. The rank of a leader is the number of leaders with a larger total, or an equal total
// and an earlier position: the stable descending sort. Both steps are quadratic compares over LDS in which every lane of a wave
// reads the same address per step (a broadcast); there are no atomics, and a pair's result depends on nothing but the pair.
#include "nsid_common.h"

namespace {

constexpr int VOTE_MAX_CAND = NSID_VOTE_MAX_CAND;   // L k of a pair at most: 48 KB of LDS
constexpr int VOTE_MAX_K = NSID_SEARCH_MAX_K;
constexpr int VOTE_MAX_TOP = NSID_VOTE_MAX_TOP;
constexpr int VOTE_THREADS = 256;
constexpr int VOTE_PER_THREAD = VOTE_MAX_CAND / VOTE_THREADS;
constexpr int VOTE_CHUNK = 8;         // LDS entries per step of the compare loops
static_assert(VOTE_PER_THREAD <= 32, "a thread's leaders are kept as a bit mask");

// CLF = false: the value of walk position j is scores[p lds + j]. CLF = true: max over i < L of S[s_off[p] + i s_ld[p] + j] (NaN
// wins, as numpy's max), and the candidate is skipped unless that is >= threshold.
template <bool CLF>
__global__ __launch_bounds__(VOTE_THREADS) void song_vote_kernel(const int64_t* __restrict__ I, int k, const float* __restrict__ S,
                                                                 int lds, const int64_t* __restrict__ s_off,
                                                                 const int* __restrict__ s_ld, const int* __restrict__ starts,
                                                                 const int* __restrict__ lens, const int* __restrict__ song_of,
                                                                 int n_ref, int n_dummy, const int* __restrict__ exclude,
                                                                 float threshold, int top, int* __restrict__ songs,
                                                                 double* __restrict__ totals, int* __restrict__ n_songs) {
  __shared__ int sg[VOTE_MAX_CAND];
  __shared__ double tot[VOTE_MAX_CAND];
  __shared__ int osong[VOTE_MAX_TOP];
  __shared__ double otot[VOTE_MAX_TOP];
  __shared__ int wcnt[VOTE_THREADS / NSID_WAVE];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int s = starts[p], L = lens[p];
  const long Ml = (long)L * k;
  if (L < 1 || Ml > VOTE_MAX_CAND || (!CLF && Ml > lds)) {      // the caller checks the pairs; this only keeps a bad one in bounds (uniform)
    if (tid < top) {
      songs[(size_t)p * top + tid] = -1;
      totals[(size_t)p * top + tid] = 0.0;
    }
    if (tid == 0) n_songs[p] = -1;
    return;
  }
  const int M = (int)Ml;
  const int excl = exclude ? exclude[p] : -1;
  const int64_t ref_end = (int64_t)n_dummy + n_ref;

  for (int j = tid; j < M; j += VOTE_THREADS) {
    const int64_t cid = I[(size_t)(s + j / k) * k + j % k];
    int song = -1;
    float v = 0.f;
    if (cid >= 0 && cid >= n_dummy && cid < ref_end) {
      const int sc = song_of[cid - n_dummy];
      if (sc >= 0 && sc != excl) {
        if (CLF) {
          const float* col = S + s_off[p] + j;
          const size_t ld = (size_t)s_ld[p];
          float m = col[0];
          for (int i = 1; i < L; ++i) {
            const float x = col[i * ld];
            m = (x > m || x != x) ? x : m;
          }
          if (m >= threshold) {
            song = sc;
            v = m;
          }
        } else {
          song = sc;
          v = S[(size_t)p * lds + j];
        }
      }
    }
    sg[j] = song;
    tot[j] = (double)v;
  }
  if (tid < VOTE_MAX_TOP) {
    osong[tid] = -1;
    otot[tid] = 0.0;
  }
  __syncthreads();

  // leaders and their totals. A leader USES the values of its own song only (what it loads of other songs' entries is discarded by
  // the select) and writes its own slot only, after its sum: no value that enters a sum changes before the barrier
  unsigned lead_mask = 0;
  int n_lead = 0;
  for (int r = 0, j = tid; j < M; j += VOTE_THREADS, ++r) {
    const int sj = sg[j];
    bool lead = sj >= 0;
    // VOTE_CHUNK entries per step, loaded unconditionally (index clamped into the walk) so that the LDS reads of a step are in flight
    // together; one dependent read per step is what this kernel's time would otherwise be
    for (int i0 = 0; i0 < j && lead; i0 += VOTE_CHUNK) {
      bool hit = false;
#pragma unroll
      for (int u = 0; u < VOTE_CHUNK; ++u) {
        const int i = i0 + u;
        hit |= (i < j) & (sg[min(i, M - 1)] == sj);
      }
      lead = !hit;
    }
    if (lead) {
      // acc is never -0.0 (it starts at +0.0, and round-to-nearest sums give -0.0 only from two -0.0), so adding +0.0 for an entry of
      // another song leaves its bits alone: the chain is the dict's additions, in its order
      double acc = 0.0;
      for (int i0 = j; i0 < M; i0 += VOTE_CHUNK) {
#pragma unroll
        for (int u = 0; u < VOTE_CHUNK; ++u) {
          const int i = i0 + u, ic = min(i, M - 1);
          const double v = tot[ic];
          acc += ((i < M) & (sg[ic] == sj)) ? v : 0.0;
        }
      }
      tot[j] = acc;
      lead_mask |= 1u << r;
      ++n_lead;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_lead += __shfl_xor(n_lead, o, NSID_WAVE);
  if ((tid & (NSID_WAVE - 1)) == 0) wcnt[tid / NSID_WAVE] = n_lead;
  __syncthreads();
  for (int r = 0, j = tid; j < M; j += VOTE_THREADS, ++r) {
    if (!((lead_mask >> r) & 1u)) sg[j] = -1;                   // from here on sg >= 0 marks a leader
  }
  __syncthreads();

  for (int r = 0, j = tid; j < M; j += VOTE_THREADS, ++r) {
    if (!((lead_mask >> r) & 1u)) continue;
    const double tj = tot[j];
    int rank = 0;
    for (int i0 = 0; i0 < M && rank < top; i0 += VOTE_CHUNK) {
#pragma unroll
      for (int u = 0; u < VOTE_CHUNK; ++u) {
        const int i = i0 + u, ic = min(i, M - 1);
        const double ti = tot[ic];
        rank += ((i < M) & (sg[ic] >= 0) & ((ti > tj) | ((ti == tj) & (i < j)))) ? 1 : 0;
      }
    }
    if (rank < top) {
      osong[rank] = sg[j];
      otot[rank] = tj;
    }
  }
  __syncthreads();
  if (tid < top) {
    songs[(size_t)p * top + tid] = osong[tid];
    totals[(size_t)p * top + tid] = otot[tid];
  }
  if (tid == 0) {
    int n = 0;
    for (int w = 0; w < VOTE_THREADS / NSID_WAVE; ++w) n += wcnt[w];
    n_songs[p] = n;
  }
}

__global__ __launch_bounds__(256) void vote_candidates_kernel(const int64_t* __restrict__ I, long n, int n_dummy, int n_ref,
                                                              int* __restrict__ cidx) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t cid = I[i];
  cidx[i] = (cid >= n_dummy && cid < (int64_t)n_dummy + n_ref) ? (int)(cid - n_dummy) : 0;
}

bool vote_limits_ok(int k, int npairs, int n_ref, int n_dummy, int top) {
  return k >= 1 && k <= VOTE_MAX_K && top >= 1 && top <= VOTE_MAX_TOP && npairs >= 0 && n_ref >= 0 && n_dummy >= 0;
}

}  // namespace

extern "C" int nsid_song_vote(const int64_t* I, int k, const float* scores, int lds, const int* starts, const int* lens, int npairs,
                              const int* song_of, int n_ref, int n_dummy, const int* exclude, int top, int* songs, double* totals,
                              int* n_songs, void* stream) {
  NSID_REQUIRE(vote_limits_ok(k, npairs, n_ref, n_dummy, top) && lds >= 1 && lds <= VOTE_MAX_CAND);
  if (npairs == 0) return NSID_OK;
  NSID_REQUIRE(I && scores && starts && lens && (song_of || n_ref == 0) && songs && totals && n_songs);
  nsid_count(NSID_C_song_vote);
  NSID_LAUNCH(song_vote_kernel<false>, dim3(npairs), dim3(VOTE_THREADS), 0, static_cast<hipStream_t>(stream), I, k, scores, lds,
              static_cast<const int64_t*>(nullptr), static_cast<const int*>(nullptr), starts, lens, song_of, n_ref, n_dummy, exclude, 0.f,
              top, songs, totals, n_songs);
  return nsid_launch_status();
}

extern "C" int nsid_song_vote_clf(const int64_t* I, int k, const float* S, const int64_t* s_off, const int* s_ld, const int* starts,
                                  const int* lens, int npairs, const int* song_of, int n_ref, int n_dummy, const int* exclude,
                                  float threshold, int top, int* songs, double* totals, int* n_songs, void* stream) {
  NSID_REQUIRE(vote_limits_ok(k, npairs, n_ref, n_dummy, top));
  if (npairs == 0) return NSID_OK;
  NSID_REQUIRE(I && S && s_off && s_ld && starts && lens && (song_of || n_ref == 0) && songs && totals && n_songs);
  nsid_count(NSID_C_song_vote_clf);
  NSID_LAUNCH(song_vote_kernel<true>, dim3(npairs), dim3(VOTE_THREADS), 0, static_cast<hipStream_t>(stream), I, k, S, 0, s_off, s_ld,
              starts, lens, song_of, n_ref, n_dummy, exclude, threshold, top, songs, totals, n_songs);
  return nsid_launch_status();
}

extern "C" int nsid_vote_candidates(const int64_t* I, long n, int n_dummy, int n_ref, int* cidx, void* stream) {
  NSID_REQUIRE(n >= 0 && n < (1L << 39) && n_dummy >= 0 && n_ref >= 0);
  if (n == 0) return NSID_OK;
  NSID_REQUIRE(I && cidx);
  nsid_count(NSID_C_vote_candidates);
  NSID_LAUNCH(vote_candidates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), I, n, n_dummy,
              n_ref, cidx);
  return nsid_launch_status();
}
