// Grouped weight gradients on 256x256 output tiles with LDS-DMA operand staging (gfx950): dW[Nout, K] += dY[R, Nout]^T f(X[R, K]),
// fp32 atomics; one class of nsid_linear_bwd_weight_grouped (gemm.hip), for problems with Nout % 256 == 0 and K % 256 == 0.
//
// Why (wgrad.hip): the wide weight gradients are bound by the L2 -> LDS bytes of re-reading operand panels, 2*R*Nout*K*(1/BM + 1/BN),
// and by the fp32 atomics of the split reduction. A 256x256 tile moves half the panel bytes per flop of the 128x128 class. Its 128 KB
// workgroup owns its CU, which lost inside the two-stream chains (gemm256.hip); the deferred phase runs alone, so that cost is gone there.
//   * 512 threads = 8 waves as 2 (rows of dW) x 4 (columns); wave tile 128 x 64 = 8 x 4 MFMA 16x16x32 tiles = 128 accumulators;
//   * the reduction (over rows of dY and X) advances through a ring of four 32-row stages of 32 KB (dY 32x256 + X 32x256 bf16), three
//     in flight while one is consumed; a stage is fetched by FOUR LDS-DMA per thread (waves 0-3 stage dY, 4-7 X, 8 rows each), ONE
//     workgroup barrier per stage: before it every wave has waited for its own DMA of the stage (vmcnt) and for its fragment reads of
//     the previous one (lgkmcnt), behind it the slot of the previous stage takes the stage three ahead;
//   * both operands are row-major with the reduction over rows, so MFMA fragments come from ds_read_b64_tr_b16 (16 lanes read 4 rows x
//     16 columns). LDS-DMA writes 64 lanes x 16 B linearly, so the image is unpadded 512-byte rows and the swizzle goes on the SOURCE
//     address: the 32-byte unit u of row r sits at u ^ f(r), f(r) = (r & 3) | ((r >> 3) & 1) << 2. The 32 lanes a transposed read serves
//     together take rows {0-3, 8-11} (+ 16 k, + 4) of one unit: eight distinct f = eight disjoint 32-byte bank ranges, conflict-free;
//   * the producer's BatchNorm affine + activation of X (per column j) is applied to the X fragments in registers after the read
//     (LDS-DMA cannot transform data in flight): a lane's X fragment is one column, so it needs one scale / shift pair per fragment;
//   * epilogue: fp32 atomics straight from the accumulators (no LDS), as the 128x128 class.
// Work items as every grouped class (nsid_common.h wgg_decode): one output tile x one row chunk of one segment (view).
#include <cstdlib>
#include "nsid_common.h"

namespace {

constexpr int W4_T = 256, W4_BK = 32, W4_THREADS = 512;
constexpr int W4_ROW = W4_T * 2;                 // bytes of one operand row in LDS (unpadded: LDS-DMA writes lane-linearly)
constexpr int W4_OP = W4_BK * W4_ROW;            // 16 KB: one operand of one stage
constexpr int W4_SLOT = 2 * W4_OP;               // dY then X
constexpr int W4_RING = 4 * W4_SLOT;             // 128 KB
static_assert(W4_RING <= NSID_LDS_MAX, "one workgroup per CU");

typedef __attribute__((address_space(3))) void* w4_lds_ptr;

// (the LDS-DMA and its explicit waits, wait_vm / wait_lgkm0: nsid_common.h. The DMA is not in the compiler's vmcnt bookkeeping:
// every wait on these loads is explicit.)
__device__ __forceinline__ bf16x8 w4_frag(const char* p) {
  typedef bf16x4 __attribute__((address_space(3))) * lds_bf16x4_ptr;
  const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p));
  const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p + 4 * W4_ROW));
  return __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <bool BAFF>
__device__ __forceinline__ void wgrad4_item(const WgProb& q, const int split, const int tile, const int g, const int seg, char* lds) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int lr = lane & 15, rq = lane >> 4;
  const int tiles_j = q.J / W4_T;
  const int i0 = (tile / tiles_j) * W4_T, j0 = (tile % tiles_j) * W4_T;
  const int rbeg = split * q.rchunk;
  const int nst = q.rchunk / W4_BK;              // a multiple of 4 (host: rchunk % 128 == 0)

  // ---- LDS-DMA source addressing: wave w & 3 stages rows 8 (w & 3) .. + 7 of its operand, two rows per instruction (lanes 0-31 the
  // first, 32-63 the second); lane l writes physical 16-byte chunk l & 31 of its row, i.e. it fetches the logical chunk whose 32-byte unit
  // is (l & 31) >> 1 ^ f(row). Of f(row) only bit 1 changes between the four instructions (row & 3 = 2 (i & 1) + (l >> 5), bit 3 = w & 1).
  const bool stage_x = wave >= 4;
  const long ld2 = (long)(stage_x ? q.ldb : q.lda) * 2;
  const int h = lane >> 5, sw = wave & 3;
  unsigned voff[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int f = (2 * par + h) | ((sw & 1) << 2);
    voff[par] = (unsigned)(h * ld2) + ((unsigned)((lane & 31) * 16) ^ (unsigned)(f << 5));
  }
  const char* gbase = stage_x ? static_cast<const char*>(q.B[seg]) + ((long)g * q.J + j0) * 2
                              : static_cast<const char*>(q.A[seg]) + ((long)g * q.I + i0) * 2;
  gbase += (long)(rbeg + 8 * sw) * ld2;
  const unsigned lds0 = (unsigned)(size_t)(w4_lds_ptr)lds + (stage_x ? W4_OP : 0) + sw * 8 * W4_ROW;
  auto issue = [&](int st, int slot) {           // stage st (clamped by the caller) -> ring slot
    const char* s = gbase + (long)st * W4_BK * ld2;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(s + 2 * i * ld2, voff[i & 1], lds0 + slot * W4_SLOT + 2 * i * W4_ROW);
  };

  // ---- fragment addressing: lane (lr, rq) reads row 8 rq + (lr >> 2) (+ 4), columns 4 (lr & 3) .. + 3 of a 16-column unit
  const int fr = lr >> 2, fsw = fr | ((rq & 1) << 2);
  const int fbase = (8 * rq + fr) * W4_ROW + 8 * (lr & 3);
  int aoff[8], boff[4];
#pragma unroll
  for (int a = 0; a < 8; ++a) aoff[a] = fbase + (((wr * 8 + a) ^ fsw) << 5);
#pragma unroll
  for (int b = 0; b < 4; ++b) boff[b] = W4_OP + fbase + (((wc * 4 + b) ^ fsw) << 5);

  float bsc[4], bsh[4];
  if (BAFF) {                                    // the lane's X column of fragment b: j0 + 64 wc + 16 b + lr
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const long jj = (long)g * q.J + j0 + 64 * wc + 16 * b + lr;
      bsc[b] = q.bsc[seg][jj];
      bsh[b] = q.bsh[seg][jj];
    }
  }
  const float slope = q.slope;

  f32x4 acc[8][4];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int slot) {
    const char* st = lds + slot * W4_SLOT;
    bf16x8 fa[8], fb[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) fb[b] = w4_frag(st + boff[b]);
#pragma unroll
    for (int a = 0; a < 8; ++a) fa[a] = w4_frag(st + aoff[a]);
    if (BAFF) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {              // packed fp32 math; slope in [0, 1]: max(v, v*slope) == (v < 0 ? v*slope : v)
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const f32x2 v = f32x2{bsc[b], bsc[b]} * f32x2{(float)fb[b][e], (float)fb[b][e + 1]} + f32x2{bsh[b], bsh[b]};
          const f32x2 w = v * slope;
          o[e] = (__bf16)fmaxf(v[0], w[0]);
          o[e + 1] = (__bf16)fmaxf(v[1], w[1]);
        }
        fb[b] = o;
      }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
  };

  // ---- main loop. Stage st lives in slot st & 3; three stages are in flight ahead of the one consumed (4 LDS-DMA each per thread).
  // Top of stage st: vmcnt(8) = this thread's DMA of st landed (loads retire in order; st + 1, st + 2 may still fly), lgkmcnt(0) = its
  // fragment reads of st - 1 are in registers; the barrier makes both hold for every wave: slot (st - 1) & 3 takes stage st + 3.
  // Stages past the end are clamped to the last one (uniform counts) and land in a slot nothing reads any more.
  const int last = nst - 1;
  issue(0, 0);
  issue(min(1, last), 1);
  issue(min(2, last), 2);
#define NSID_W4_STEP(U)                                        \
  do {                                                         \
    wait_vm<8>();                                           \
    wait_lgkm0();                                           \
    __builtin_amdgcn_s_barrier();                              \
    __builtin_amdgcn_sched_barrier(0);                         \
    issue(min(st + (U) + 3, last), ((U) + 3) & 3);             \
    compute(U);                                                \
    __builtin_amdgcn_sched_barrier(0);                         \
  } while (0)
  for (int st = 0; st < nst; st += 4) {
    NSID_W4_STEP(0);
    NSID_W4_STEP(1);
    NSID_W4_STEP(2);
    NSID_W4_STEP(3);
  }
#undef NSID_W4_STEP
  // the three clamped stages still in flight target slots 0-2, which the next item's prologue writes: drain them (this thread's own;
  // every wave stages its own region of a slot). Slot 3 (the last stage, possibly still being read by other waves) is not touched.
  wait_vm<0>();

  // ---- epilogue: lane (lr, rq), reg r of acc[a][b] = dW[i0 + 128 wr + 16 a + 4 rq + r][j0 + 64 wc + 16 b + lr]
  float* C = q.C + (long)g * q.I * q.J;
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        atomicAdd(C + (long)(i0 + 128 * wr + 16 * a + 4 * rq + r) * q.J + (j0 + 64 * wc + 16 * b + lr), acc[a][b][r]);
}

// plain and affine problems in ONE launch (the phase then has one tail less): the item body is instantiated for both, chosen per problem
__global__ __launch_bounds__(W4_THREADS, 2) void wgrad4_grouped_kernel(const WgGroupArgs ga) {
  __shared__ __attribute__((aligned(1024))) char lds[W4_RING];
  const int total = ga.wg0[ga.n];
  for (int w = blockIdx.x; w < total; w += gridDim.x) {
    int pi, split, bid, g, seg;
    if (wgg_decode(ga, w, pi, split, bid, g, seg)) {
      const WgProb& q = ga.prob[pi];
      if (q.bsc[seg] != nullptr) wgrad4_item<true>(q, split, bid, g, seg, lds);
      else wgrad4_item<false>(q, split, bid, g, seg, lds);
    }
  }
}

}  // namespace

int nsid_wgrad4_grouped_launch(const WgGroupArgs& ga, int grid, hipStream_t stream) {
  NSID_LAUNCH(wgrad4_grouped_kernel, dim3(grid), dim3(W4_THREADS), 0, stream, ga);
  return nsid_launch_status();
}
