// Diagonal-histogram vote of a query's search result (include/nsid.h nsid_diag_vote): the songs whose hits (query row i, reference
// row r) line up along a diagonal r - i = const, wherever in the window the diagonal starts. The reference leaves this score to
// "future implementations" (eval.py:249-258); the rule is stated in the header and in tests/diag_vote_oracle.py.
//
// One workgroup per pair. Every hit of the pair becomes one 64-bit key (song code << 32 | narrow bin), a skipped hit the largest
// key, and the keys are sorted in LDS (bitonic, padded to a power of two). After the sort a (song, narrow bin) is a run of equal
// keys, the next narrow bin of the song is the next run, and a song is a stretch of runs: a run's head finds with one binary search
// the end of the keys {key, key + 1}, which is the count of the wide bin that STARTS at its narrow bin, and with a second one its
// song's first position, where an LDS atomic max keeps (count, smallest position). Only wide bins that start at a non-empty narrow
// bin are looked at: the wide bin b with cnt[b] == 0 holds the hits of narrow bin b + 1 alone, which the wide bin b + 1 holds too,
// so it never has more hits than its neighbour, and where it ties it names the same hits; no output names b itself. The songs'
// heads are then sorted as 32-bit keys (4096 - count, position): count descending, code ascending. The row ranges of the `top`
// winning bins come from a second walk over the pair's hits (LDS atomic min / max). Integer sums and extrema are order-free, so the
// result is the rule's in every bit; there are no global atomics and a pair's result depends on nothing but the pair.
#include "nsid_common.h"

namespace {

constexpr int DV_MAX_CAND = NSID_VOTE_MAX_CAND;
constexpr int DV_MAX_TOP = NSID_VOTE_MAX_TOP;
constexpr int DV_THREADS = 256;
constexpr int DV_POS_BITS = 12;       // a sorted position
constexpr unsigned DV_POS_MASK = (1u << DV_POS_BITS) - 1;
constexpr uint64_t DV_NONE = ~uint64_t(0);
static_assert(DV_MAX_CAND == 1 << DV_POS_BITS, "a count and a position share 32 bits");
static_assert(DV_MAX_TOP <= DV_THREADS, "one thread per output column");

// ascending, in place; P a power of two, the same for every thread of the workgroup. Ends behind a barrier.
template <typename T>
__device__ __forceinline__ void dv_sort(T* a, const int P, const int tid) {
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (int t = tid; t < (P >> 1); t += DV_THREADS) {
        const int i = ((t & ~(j2 - 1)) << 1) | (t & (j2 - 1)), l = i | j2;
        const T x = a[i], y = a[l];
        if ((x > y) == ((i & k2) == 0)) {
          a[i] = y;
          a[l] = x;
        }
      }
      __syncthreads();
    }
  }
}

// the first position of the sorted a[0 .. P) that holds a key >= x
__device__ __forceinline__ int dv_lower_bound(const uint64_t* a, const int P, const uint64_t x) {
  int lo = 0, hi = P;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the key of walk position j, DV_NONE for a skipped hit; qi = the query row, r = the reference row (set for a hit that counts)
__device__ __forceinline__ uint64_t dv_key(const int64_t* __restrict__ I, const int k, const int s, const int L, const int j,
                                           const int* __restrict__ song_of, const int n_dummy, const int64_t ref_end, const int excl,
                                           const int B, int& qi, int& r) {
  qi = s + j / k;
  const int64_t cid = I[(size_t)qi * k + j % k];
  if (cid < 0 || cid < n_dummy || cid >= ref_end) return DV_NONE;
  r = (int)(cid - n_dummy);
  const int c = song_of[r];
  if (c < 0 || c == excl) return DV_NONE;
  const int delta = r - (qi - s) + (L - 1);                    // >= 0, < n_ref + 4096 < 2^31
  return (uint64_t)c << 32 | (unsigned)(delta / B);
}

__global__ __launch_bounds__(DV_THREADS) void diag_vote_kernel(const int64_t* __restrict__ I, int k, const int* __restrict__ starts,
                                                               const int* __restrict__ lens, const int* __restrict__ song_of,
                                                               int n_ref, int n_dummy, const int* __restrict__ exclude, int B, int top,
                                                               int* __restrict__ songs, int* __restrict__ counts,
                                                               int* __restrict__ i_lo, int* __restrict__ i_hi, int* __restrict__ r_lo,
                                                               int* __restrict__ r_hi, int* __restrict__ n_songs) {
  __shared__ uint64_t key[DV_MAX_CAND];                // 32 KB
  __shared__ unsigned aux[DV_MAX_CAND];                // per song head: (count, bin position) by atomic max; then the songs' sort keys
  __shared__ unsigned short win_at[DV_MAX_CAND];       // per song head: the sorted position of its winning bin's head
  __shared__ uint64_t wkey[DV_MAX_TOP];
  __shared__ int wcnt[DV_MAX_TOP];
  __shared__ int box[4][DV_MAX_TOP];                   // i_lo, i_hi, r_lo, r_hi of the winners
  __shared__ int wsongs[DV_THREADS / NSID_WAVE];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int s = starts[p], L = lens[p];
  const long Ml = (long)L * k;
  if (L < 1 || Ml > DV_MAX_CAND) {                     // the caller checks the pairs; this only keeps a bad one in bounds (uniform)
    if (tid < top) {
      const size_t o = (size_t)p * top + tid;
      songs[o] = -1;
      counts[o] = 0;
      i_lo[o] = i_hi[o] = r_lo[o] = r_hi[o] = -1;
    }
    if (tid == 0) n_songs[p] = -1;
    return;
  }
  const int M = (int)Ml;
  int P = 2;
  while (P < M) P <<= 1;
  const int excl = exclude ? exclude[p] : -1;
  const int64_t ref_end = (int64_t)n_dummy + n_ref;

  for (int j = tid; j < P; j += DV_THREADS) {
    int qi = 0, r = -1;
    key[j] = j < M ? dv_key(I, k, s, L, j, song_of, n_dummy, ref_end, excl, B, qi, r) : DV_NONE;
    aux[j] = 0u;
  }
  if (tid < DV_MAX_TOP) {
    wkey[tid] = DV_NONE;
    wcnt[tid] = 0;
    box[0][tid] = box[2][tid] = 0x7fffffff;
    box[1][tid] = box[3][tid] = -1;
  }
  __syncthreads();
  dv_sort(key, P, tid);

  // run heads: the wide bin that starts here, to its song's head
  for (int t = tid; t < P; t += DV_THREADS) {
    const uint64_t kk = key[t];
    if (kk == DV_NONE || (t > 0 && key[t - 1] == kk)) continue;
    const int end = dv_lower_bound(key, P, kk + 2);              // the keys {kk, kk + 1} are [t, end); the bin never carries into the code
    const int sh = dv_lower_bound(key, P, kk & ~uint64_t(0xffffffffu));
    atomicMax(&aux[sh], (unsigned)(end - t) << DV_POS_BITS | (DV_POS_MASK - (unsigned)t));   // larger count, then smaller position
  }
  __syncthreads();

  // song heads: their sort key. A thread reads and writes its own slots of aux only
  int n_heads = 0;
  for (int t = tid; t < P; t += DV_THREADS) {
    const uint64_t kk = key[t];
    unsigned k2 = ~0u;
    if (kk != DV_NONE && (t == 0 || (key[t - 1] >> 32) != (kk >> 32))) {
      const unsigned b = aux[t];
      win_at[t] = (unsigned short)(DV_POS_MASK - (b & DV_POS_MASK));
      k2 = ((unsigned)DV_MAX_CAND - (b >> DV_POS_BITS)) << DV_POS_BITS | (unsigned)t;
      ++n_heads;
    }
    aux[t] = k2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_heads += __shfl_xor(n_heads, o, NSID_WAVE);
  if ((tid & (NSID_WAVE - 1)) == 0) wsongs[tid / NSID_WAVE] = n_heads;
  __syncthreads();
  dv_sort(aux, P, tid);

  int total = 0;
  for (int w = 0; w < DV_THREADS / NSID_WAVE; ++w) total += wsongs[w];
  const int n_win = min(total, top);
  if (tid < n_win) {                                   // n_win <= the song heads <= P
    const unsigned k2 = aux[tid];
    wkey[tid] = key[win_at[k2 & DV_POS_MASK]];
    wcnt[tid] = DV_MAX_CAND - (int)(k2 >> DV_POS_BITS);
  }
  __syncthreads();

  // the rows of the winning bins: the hits whose key is a winner's or the next narrow bin's
  for (int j = tid; j < M; j += DV_THREADS) {
    int qi = 0, r = -1;
    const uint64_t kk = dv_key(I, k, s, L, j, song_of, n_dummy, ref_end, excl, B, qi, r);
    if (kk == DV_NONE) continue;
    for (int u = 0; u < n_win; ++u) {
      const uint64_t wk = wkey[u];
      if (kk == wk || kk == wk + 1) {
        atomicMin(&box[0][u], qi);
        atomicMax(&box[1][u], qi);
        atomicMin(&box[2][u], r);
        atomicMax(&box[3][u], r);
        break;                                         // the winners are different songs
      }
    }
  }
  __syncthreads();
  if (tid < top) {
    const size_t o = (size_t)p * top + tid;
    const bool won = tid < n_win;
    songs[o] = won ? (int)(wkey[tid] >> 32) : -1;
    counts[o] = won ? wcnt[tid] : 0;
    i_lo[o] = won ? box[0][tid] : -1;
    i_hi[o] = won ? box[1][tid] : -1;
    r_lo[o] = won ? box[2][tid] : -1;
    r_hi[o] = won ? box[3][tid] : -1;
  }
  if (tid == 0) n_songs[p] = total;
}

}  // namespace

extern "C" int nsid_diag_vote(const int64_t* I, int k, const int* starts, const int* lens, int npairs, const int* song_of, int n_ref,
                              int n_dummy, const int* exclude, int bin_rows, int top, int* songs, int* counts, int* i_lo, int* i_hi,
                              int* r_lo, int* r_hi, int* n_songs, void* stream) {
  NSID_REQUIRE(k >= 1 && k <= NSID_SEARCH_MAX_K && top >= 1 && top <= DV_MAX_TOP && bin_rows >= 1 && bin_rows <= NSID_DIAG_MAX_BIN &&
               npairs >= 0 && n_dummy >= 0 && n_ref >= 0 && (int64_t)n_ref + DV_MAX_CAND < (int64_t(1) << 31));
  if (npairs == 0) return NSID_OK;
  NSID_REQUIRE(I && starts && lens && (song_of || n_ref == 0) && songs && counts && i_lo && i_hi && r_lo && r_hi && n_songs);
  nsid_count(NSID_C_diag_vote);
  NSID_LAUNCH(diag_vote_kernel, dim3(npairs), dim3(DV_THREADS), 0, static_cast<hipStream_t>(stream), I, k, starts, lens, song_of, n_ref,
              n_dummy, exclude, bin_rows, top, songs, counts, i_lo, i_hi, r_lo, r_hi, n_songs);
  return nsid_launch_status();
}
