// Small HBM-bound kernels of the path: downsample row gather, peak-extractor patchify, node mean, ELU', L2
// normalise, clip+Adam, and the (B,C,N) <-> node-major layout change at the module boundary.
#include <algorithm>
#include "nsid_common.h"

namespace {

inline int grid_for(long n, int cap = 2048) {
  long b = (n + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

// ------------------------------------------------------------------ Downsample (3-tap stride-2 conv along N)
template <typename T>
__global__ __launch_bounds__(256) void im2col3_fwd_kernel(const T* __restrict__ x, int B, int N, int No, int C,
                                                          T* __restrict__ col) {
  constexpr int NV = Chunk<T>::N;
  const int CV = C / NV;
  const long total = (long)B * No * 3 * CV;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int cv = (int)(q % CV);
    const int t = (int)((q / CV) % 3);
    const long orow = q / (3L * CV);
    const int b = (int)(orow / No), no = (int)(orow % No);
    const int n = 2 * no - 1 + t;
    float v[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) v[e] = 0.f;
    if (n >= 0 && n < N) Chunk<T>::load(x + ((long)b * N + n) * C + NV * cv, v);
    Chunk<T>::store(col + orow * (3L * C) + (long)t * C + NV * cv, v);
  }
}

// dx[b,n,:] = sum over (n', t) with 2n'-1+t == n of dcol[b,n', t*C:(t+1)*C]   (gather form: no atomics)
template <typename T>
__global__ __launch_bounds__(256) void im2col3_bwd_kernel(const T* __restrict__ dcol, int B, int N, int No, int C,
                                                          T* __restrict__ dx) {
  constexpr int NV = Chunk<T>::N;
  const int CV = C / NV;
  const long total = (long)B * N * CV;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int cv = (int)(q % CV);
    const long row = q / CV;
    const int b = (int)(row / N), n = (int)(row % N);
    float s[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) s[e] = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int m = n + 1 - t;            // 2n' = n+1-t
      if (m >= 0 && (m & 1) == 0 && (m >> 1) < No) {
        float v[NV];
        Chunk<T>::load(dcol + ((long)b * No + (m >> 1)) * (3L * C) + (long)t * C + NV * cv, v);
#pragma unroll
        for (int e = 0; e < NV; ++e) s[e] += v[e];
      }
    }
    Chunk<T>::store(dx + row * C + NV * cv, s);
  }
}

__global__ void pack_ds_weight_kernel(const float* __restrict__ w, int Cout, int Cin, float* __restrict__ wp) {
  const long total = (long)Cout * 3 * Cin;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int c = (int)(q % Cin), t = (int)((q / Cin) % 3);
    const long o = q / (3L * Cin);
    wp[q] = w[((o * Cin + c) * 3 + t) * 3 + 1];     // w[o][c][t][1]
  }
}
// backward-data weights of the odd input rows: wb[r][c] = w[o][c][2][1] for r = o < Cout, w[o][c][0][1] for r = Cout + o
__global__ void pack_ds_weight_bwd_kernel(const float* __restrict__ w, int Cout, int Cin, float* __restrict__ wb) {
  const long total = 2L * Cout * Cin;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int c = (int)(q % Cin);
    const long r = q / Cin;
    const long o = r % Cout;
    const int t = r < Cout ? 2 : 0;
    wb[q] = w[((o * Cin + c) * 3 + t) * 3 + 1];
  }
}
__global__ void unpack_ds_wgrad_kernel(const float* __restrict__ dwp, int Cout, int Cin, float* __restrict__ dw) {
  const long total = (long)Cout * 3 * Cin;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int c = (int)(q % Cin), t = (int)((q / Cin) % 3);
    const long o = q / (3L * Cin);
    atomicAdd(dw + ((o * Cin + c) * 3 + t) * 3 + 1, dwp[q]);     // both views may accumulate concurrently
  }
}

// Step-scoped preparation of ALL Downsample conv weights in one launch (round 4): a training step used to spend 36 small launches on
// the three Downsample layers — pack (forward) + pack (backward) + two bf16 conversions + a zero fill and an unpack of the packed
// gradient, per layer AND per view. Here one launch at the start of the step writes, for every layer, the packed forward weight
// wp[o][t*Cin + c] = w[o][c][t][1] and the packed backward weight wb = [W_2 ; W_0] straight to bf16 and zeroes the layer's two packed
// gradient buffers (one per view; each view still unpacks its own right after its weight-gradient GEMM, so a parameter's .grad is
// complete when backward returns).
constexpr int DSP_LAYERS = NSID_DS_PREPACK_MAX_LAYERS;
#define NSID_DS_SLOTS 2
struct DsPrepArgs {
  const float* w[DSP_LAYERS]; __bf16* wp16[DSP_LAYERS]; __bf16* wb16[DSP_LAYERS]; float* dwp[DSP_LAYERS];
  int Cout[DSP_LAYERS], Cin[DSP_LAYERS];
};
__global__ __launch_bounds__(256) void ds_prepack_kernel(const DsPrepArgs a) {
  const int l = blockIdx.y;
  const float* w = a.w[l];
  const int Cout = a.Cout[l], Cin = a.Cin[l];
  const long total = (long)Cout * 3 * Cin;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int c = (int)(q % Cin), t = (int)((q / Cin) % 3);
    const long o = q / (3L * Cin);
    a.wp16[l][q] = (__bf16)w[((o * Cin + c) * 3 + t) * 3 + 1];
    if (a.dwp[l] != nullptr) {                       // NSID_DS_SLOTS packed gradient buffers per layer (one per view), contiguous
#pragma unroll
      for (int v = 0; v < NSID_DS_SLOTS; ++v) a.dwp[l][v * total + q] = 0.f;
    }
    if (q < 2L * Cout * Cin) {                       // wb[r][c] = w[o][c][2][1] for r = o < Cout, w[o][c][0][1] for r = Cout + o
      const long r = q / Cin, ob = r % Cout;
      const int tb = r < Cout ? 2 : 0;
      a.wb16[l][q] = (__bf16)w[((ob * Cin + c) * 3 + tb) * 3 + 1];
    }
  }
}

// ------------------------------------------------------------------ GPUPeakExtractorv2
// torch.linspace(0,1,steps)[i]: start + i*step in the lower half, end - (steps-1-i)*step in the upper half
// acc + a * b with the product ROUNDED before the addition: no contraction into an fma, whatever the surrounding code (HIP compiles with
// -ffp-contract=fast-honor-pragmas; __fadd_rn / __fmul_rn are plain operators in this toolchain and do get contracted)
__device__ __forceinline__ float add_unfused(float acc, float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return acc + p;
}
// (the upper half as one fused multiply-add: the form rounds 1-3 compiled; pinned for the same reason as the accumulation in
// patchify_fwd_kernel)
__device__ __forceinline__ float linspace01(int i, int steps) {
  const float step = 1.0f / (float)(steps - 1);
  return (i < steps / 2) ? __fmul_rn((float)i, step) : fmaf(-(float)(steps - 1 - i), step, 1.0f);
}

// Both kernels stage the whole clip in LDS first (H*W fp32 = 32 KB, vectorised coalesced loads, the min-max
// normalisation applied once): the per-patch loops then read LDS instead of issuing dependent strided global loads (the
// first versions were pure load-latency chains: 85 us forward, 214 us backward for a 2 MFLOP op).
constexpr int PATCH_PAD = 8;     // row stride W+8 floats: the pb rows of a patch fall on different banks
// PB, PF > 0: the patch shape at compile time (GraFP: 4 x 8). The time / frequency ramps of a patch are then PF + PB values instead of
// two more per-element planes (64 registers less: 216 -> under 128 VGPRs, four workgroups per CU instead of two), same accumulation order.
template <typename T, int MAXPATCH, int PB = 0, int PF = 0>
__global__ __launch_bounds__(256) void patchify_fwd_kernel(const float* __restrict__ spec, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int H, int W, int pb_,
                                                           int pf_, int F, T* __restrict__ out, int ldo,
                                                           float* __restrict__ minmax) {
  constexpr bool FIX = PB > 0;
  const int pb = FIX ? PB : pb_, pf = FIX ? PF : pf_;
  extern __shared__ __attribute__((aligned(16))) float sm[];   // weights [F][3][pb][pf], scratch [8], clip [H][W+pad]
  const int b = blockIdx.x, t = threadIdx.x;
  const float* x = spec + (long)b * H * W;
  const int wn = F * 3 * pb * pf, LDW = W + PATCH_PAD;
  float* wl = sm;
  float* red = sm + wn;      // [2][4 waves]
  float* xs = red + 8;
  for (int i = t; i < wn; i += blockDim.x) wl[i] = w[i];
  float lo = __builtin_inff(), hi = -__builtin_inff();
  constexpr int XB = 8;                                          // loads of a batch are issued before the first use
  for (int i0 = t; i0 < H * W / 4; i0 += XB * blockDim.x) {      // W % 4 == 0: a float4 never straddles a row
    f32x4 v[XB];
#pragma unroll
    for (int u = 0; u < XB; ++u) {
      const int i = i0 + u * blockDim.x;
      if (i < H * W / 4) v[u] = *reinterpret_cast<const f32x4*>(x + 4 * i);
    }
#pragma unroll
    for (int u = 0; u < XB; ++u) {
      const int i = i0 + u * blockDim.x;
      if (i < H * W / 4) {
        const int hh = (4 * i) / W, ww = (4 * i) % W;
        *reinterpret_cast<f32x4*>(xs + hh * LDW + ww) = v[u];
        lo = fminf(fminf(lo, v[u][0]), fminf(v[u][1], fminf(v[u][2], v[u][3])));
        hi = fmaxf(fmaxf(hi, v[u][0]), fmaxf(v[u][1], fmaxf(v[u][2], v[u][3])));
      }
    }
  }
  lo = wave_min(lo); hi = wave_max(hi);
  if ((t & 63) == 0) { red[t >> 6] = lo; red[4 + (t >> 6)] = hi; }
  __syncthreads();
  lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  if (t == 0 && minmax != nullptr) { minmax[2 * b] = lo; minmax[2 * b + 1] = hi; }
  const float range = hi - lo;
  const int Hp = H / pb, Wp = W / pf, NP = Hp * Wp;
  // MAXPATCH >= pb*pf (host-checked; the instantiation with MAXPATCH == pb*pf has no predicates): the patch's three
  // input planes sit in registers, one division per spectrogram value
  for (int p = t; p < NP; p += blockDim.x) {
    const int ph = p / Wp, pw = p % Wp;
    T* dst = out + ((long)b * NP + p) * ldo;
    constexpr int NLW = FIX ? PF : MAXPATCH, NLH = FIX ? PB : MAXPATCH;
    float sv[MAXPATCH], lw[NLW], lh[NLH];
#pragma unroll
    for (int q = 0; q < MAXPATCH; ++q) {
      if (q < pb * pf) {
        const int i = q / pf, j = q % pf;
        sv[q] = (xs[(ph * pb + i) * LDW + pw * pf + j] - lo) / range;
        if constexpr (!FIX) {
          lw[q] = linspace01(pw * pf + j, W);
          lh[q] = linspace01(ph * pb + i, H);
        }
      }
    }
    if constexpr (FIX) {
#pragma unroll
      for (int j = 0; j < PF; ++j) lw[j] = linspace01(pw * PF + j, W);
#pragma unroll
      for (int i = 0; i < PB; ++i) lh[i] = linspace01(ph * PB + i, H);
    }
    constexpr int NV = Chunk<T>::N;                          // filters per 16-byte store (the encoder's stem: F = 8 bf16 = one store)
    for (int f0 = 0; f0 < F; f0 += NV) {
      float res[NV];
#pragma unroll
      for (int ff = 0; ff < NV; ++ff) {
        const int f = f0 + ff;
        res[ff] = 0.f;
        if (f < F) {
          float acc = bias[f];
          // the filter's weights straight from (read-only) global memory: the index is uniform, so they arrive by scalar loads and feed
          // the FMAs as SGPR operands -- from the LDS copy they were 96 broadcast ds_read_b32 per filter and thread
          const float* wf = (MAXPATCH == 32 ? w : wl) + f * 3 * pb * pf;
#pragma unroll
          for (int q = 0; q < MAXPATCH; ++q) {
            if (q < pb * pf) {                   // accumulation order: (i, j) row-major, planes time/freq/spec
              // Pinned arithmetic: the time-plane term is ONE fused multiply-add, the frequency- and spectrogram-plane products are
              // rounded before they are added. That is how rounds 1-3 compiled this loop (the compiler packed the two products
              // into one v_pk_mul_f32 and added them separately); contracting all three moves half of the non-zero outputs by an ulp
              // or two (max 1.9e-6; 6.0e-7 instead of 8.3e-7 max against the peak_b8 golden, both far inside its 1e-5), and the
              // B = 256 / bf16-emulation tests carry bounds measured at 3x what THIS rounding gives through 12 max-relative layers
              // (all-fma: global gradient norm 1.4e-3 instead of 3.5e-4 of the reference's at B = 256). Written out so that the
              // values no longer depend on what the vectoriser does with the surrounding code.
              acc = fmaf(wf[q], lw[FIX ? q % (FIX ? PF : 1) : q], acc);
              acc = add_unfused(acc, wf[pb * pf + q], lh[FIX ? q / (FIX ? PF : 1) : q]);
              acc = add_unfused(acc, wf[2 * pb * pf + q], sv[q]);
            }
          }
          res[ff] = acc < 0.f ? 0.f : acc;       // NaN (constant clip: 0/0) propagates, as in the reference
        }
      }
      if (f0 + NV <= F && ldo % NV == 0 && (reinterpret_cast<size_t>(out) & 15) == 0) {
        Chunk<T>::store(dst + f0, res);          // (the eight 2-byte stores of a patch were the kernel's store traffic: 16 B rows)
      } else {
#pragma unroll
        for (int ff = 0; ff < NV; ++ff)
          if (f0 + ff < F) dst[f0 + ff] = (T)res[ff];
      }
    }
  }
}

// dw[f][c][i][j] += sum_{b,p} g[b,p,f] * img_c[b, ph*pb+i, pw*pf+j], g = dout * (out > 0); one block per clip
template <typename T>
__global__ __launch_bounds__(256) void patchify_bwd_kernel(const float* __restrict__ spec,
                                                           const float* __restrict__ minmax,
                                                           const T* __restrict__ out,
                                                           const T* __restrict__ dout, int ldo, int B, int H,
                                                           int W, int pb, int pf, int F, float* __restrict__ dw,
                                                           float* __restrict__ dbias, int bands) {
  extern __shared__ __attribute__((aligned(16))) float sm[];   // g [NP][F], then the normalised clip [H][W+pad]
  const int t = threadIdx.x;
  // bands > 1 (a clip beyond the LDS, e.g. 256 mel bins): a clip is walked as `bands` bands of patch rows — the sums over patches are
  // sums over bands, only the frequency ramp needs the band's offset. H / Hp / NP below are ONE BAND's; Hall is the clip's height.
  const int Hall = H;
  H /= bands;
  const int Hp = H / pb, Wp = W / pf, NP = Hp * Wp;
  const int per_f = 3 * pb * pf, LDW = W + PATCH_PAD;
  float* xs = sm + NP * F;
  float* red = xs + H * LDW;                                   // [(Wp + Hp)][F] partial sums of g
  // A workgroup walks clips b, b + grid, ... with its sums in registers: one atomic per workgroup and output
  constexpr int MAXQ = 4;                                      // outputs per thread: F*per_f <= 4*256
  float wacc[MAXQ] = {0.f, 0.f, 0.f, 0.f}, bacc = 0.f;
  constexpr int NV = Chunk<T>::N;
  const bool vec = (F % NV == 0) && (ldo % NV == 0);          // 16-byte rows of out / dout (F = 8 bf16: one chunk a patch)
  for (int vb = blockIdx.x; vb < B * bands; vb += gridDim.x) {
    const int b = vb / bands, band = vb - b * bands;
    const float* x = spec + ((long)b * bands + band) * H * W;
    const float lo = minmax[2 * b], range = minmax[2 * b + 1] - lo;
    __syncthreads();                                           // previous clip's readers are done with sm
    // staging: every global load of a batch is issued before its first use (these loops were serial round trips)
    if (vec) {
      const int FC = F / NV;
      for (int q = t; q < NP * FC; q += blockDim.x) {
        const int p = q / FC, f = (q % FC) * NV;
        const long o = ((long)vb * NP + p) * ldo + f;
        float ov[NV], dv[NV];
        Chunk<T>::load(out + o, ov);
        Chunk<T>::load(dout + o, dv);
#pragma unroll
        for (int e = 0; e < NV; ++e) sm[p * F + f + e] = ov[e] > 0.f ? dv[e] : 0.f;
      }
    } else {
      for (int q = t; q < NP * F; q += blockDim.x) {
        const int p = q / F, f = q % F;
        const long o = ((long)vb * NP + p) * ldo + f;
        sm[q] = (float)out[o] > 0.f ? (float)dout[o] : 0.f;
      }
    }
    constexpr int XB = 8;
    for (int i0 = t; i0 < H * W / 4; i0 += XB * blockDim.x) {
      f32x4 v[XB];
#pragma unroll
      for (int u = 0; u < XB; ++u) {
        const int i = i0 + u * blockDim.x;
        if (i < H * W / 4) v[u] = *reinterpret_cast<const f32x4*>(x + 4 * i);
      }
#pragma unroll
      for (int u = 0; u < XB; ++u) {
        const int i = i0 + u * blockDim.x;
        if (i < H * W / 4) {
          const int hh = (4 * i) / W, ww = (4 * i) % W;
          *reinterpret_cast<f32x4*>(xs + hh * LDW + ww) =
              f32x4{(v[u][0] - lo) / range, (v[u][1] - lo) / range, (v[u][2] - lo) / range, (v[u][3] - lo) / range};
        }
      }
    }
    __syncthreads();
    // the two ramp planes depend on the patch column (time ramp) or row (frequency ramp) only: reduce g over the other
    // patch index first (Wp*F + Hp*F sums), so only the spectrogram plane walks all NP patches
    for (int q = t; q < (Wp + Hp) * F; q += blockDim.x) {
      const int f = q % F, k2 = q / F;
      float a = 0.f;
      if (k2 < Wp) { for (int ph = 0; ph < Hp; ++ph) a += sm[(ph * Wp + k2) * F + f]; }
      else { for (int pw = 0; pw < Wp; ++pw) a += sm[((k2 - Wp) * Wp + pw) * F + f]; }
      red[q] = a;                                              // [Wp][F] column sums, then [Hp][F] row sums
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < MAXQ; ++u) {
      const int q = t + u * 256;
      if (q < F * per_f) {
        const int f = q / per_f, rem = q % per_f;
        const int c = rem / (pb * pf), i = (rem / pf) % pb, j = rem % pf;
        float acc = 0.f;
        if (c == 0) {
          for (int pw = 0; pw < Wp; ++pw) acc += red[pw * F + f] * linspace01(pw * pf + j, W);
        } else if (c == 1) {
          for (int ph = 0; ph < Hp; ++ph) acc += red[(Wp + ph) * F + f] * linspace01((band * Hp + ph) * pb + i, Hall);
        } else {
          constexpr int UB = 4;                                // independent LDS chains, no division in the loops
          float part[UB] = {0.f, 0.f, 0.f, 0.f};
          for (int ph = 0; ph < Hp; ++ph) {
            const float* srow = sm + (ph * Wp) * F + f;
            const float* xrow = xs + (ph * pb + i) * LDW + j;
            for (int pw0 = 0; pw0 < Wp; pw0 += UB) {
#pragma unroll
              for (int v = 0; v < UB; ++v)
                if (pw0 + v < Wp) part[v] += srow[(pw0 + v) * F] * xrow[(pw0 + v) * pf];
            }
          }
          acc = (part[0] + part[1]) + (part[2] + part[3]);
        }
        wacc[u] += acc;
      }
    }
    if (t < F) {
      float acc = 0.f;
      for (int p = 0; p < NP; ++p) acc += sm[p * F + t];
      bacc += acc;
    }
  }
#pragma unroll
  for (int u = 0; u < MAXQ; ++u) {
    const int q = t + u * 256;
    if (q < F * per_f) atomicAdd(dw + q, wacc[u]);
  }
  if (t < F) atomicAdd(dbias + t, bacc);
}

// ---- GraFP's patch (4 x 8, 8 filters, 64 x 128 clips) with a workspace: the form above spends most of its 44 us in its last lines —
// 512 workgroups (two views) adding 776 values each into the SAME 776 addresses (memory-side atomics on one 3 KB row run 14x below
// their rate) — and executes its three plane branches one after the other in every wave. Here a workgroup writes its clip's 776
// partial sums to ws[b][776] with plain stores and a second launch adds them up (one atomic per output and view); the 768 outputs
// are laid over the 256 threads as (filter, position in the patch) so that every thread computes all three planes without branches.
constexpr int PB2_OUT = 8 * 3 * 32 + 8;           // 768 weight gradients + 8 bias gradients per clip

template <typename T>
__global__ __launch_bounds__(256) void patchify_bwd2_kernel(const float* __restrict__ spec, const float* __restrict__ minmax,
                                                            const T* __restrict__ out, const T* __restrict__ dout, int ldo,
                                                            float* __restrict__ ws) {
  constexpr int H = 64, W = 128, PBk = 4, PFk = 8, F = 8, Hp = 16, Wp = 16, NP = 256, LDW = W + PATCH_PAD;
  __shared__ __attribute__((aligned(16))) float g[NP * F];          // g[p][f] = dout where out > 0
  __shared__ __attribute__((aligned(16))) float xs[H * LDW];        // the normalised clip
  __shared__ float red[(Wp + Hp) * F];                              // column sums [pw][f], then row sums [ph][f]
  const int t = threadIdx.x, b = blockIdx.x;
  const float* x = spec + (long)b * H * W;
  const float lo = minmax[2 * b], range = minmax[2 * b + 1] - lo;
  {
    const long o = ((long)b * NP + t) * ldo;                         // patch t: F = 8 values = one chunk (bf16) or two (fp32)
    float ov[8], dv[8];
    if constexpr (Chunk<T>::N == 8) {
      Chunk<T>::load(out + o, ov);
      Chunk<T>::load(dout + o, dv);
    } else {
      Chunk<T>::load(out + o, ov); Chunk<T>::load(out + o + 4, ov + 4);
      Chunk<T>::load(dout + o, dv); Chunk<T>::load(dout + o + 4, dv + 4);
    }
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(x + 4 * (t + 256 * u));
#pragma unroll
    for (int e = 0; e < 8; ++e) g[t * F + e] = ov[e] > 0.f ? dv[e] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i4 = 4 * (t + 256 * u), hh = i4 / W, ww = i4 % W;
      *reinterpret_cast<f32x4*>(xs + hh * LDW + ww) =
          f32x4{(v[u][0] - lo) / range, (v[u][1] - lo) / range, (v[u][2] - lo) / range, (v[u][3] - lo) / range};
    }
  }
  __syncthreads();
  {
    const int f = t % F, k2 = t / F;                                 // 32 x 8 sums: one per thread
    float a = 0.f;
    if (k2 < Wp) { for (int ph = 0; ph < Hp; ++ph) a += g[(ph * Wp + k2) * F + f]; }
    else { for (int pw = 0; pw < Wp; ++pw) a += g[((k2 - Wp) * Wp + pw) * F + f]; }
    red[t] = a;
  }
  __syncthreads();
  const int f = t >> 5, ij = t & 31, i = ij >> 3, j = ij & 7;
  float a_t = 0.f, a_f = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    a_t += red[q * F + f] * linspace01(q * PFk + j, W);
    a_f += red[(Wp + q) * F + f] * linspace01(q * PBk + i, H);
  }
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ph = 0; ph < Hp; ++ph) {
    const float* srow = g + (ph * Wp) * F + f;
    const float* xrow = xs + (ph * PBk + i) * LDW + j;
#pragma unroll
    for (int pw = 0; pw < Wp; ++pw) part[pw & 3] += srow[pw * F] * xrow[pw * PFk];
  }
  float* wsb = ws + (long)b * PB2_OUT;
  wsb[f * 96 + ij] = a_t;
  wsb[f * 96 + 32 + ij] = a_f;
  wsb[f * 96 + 64 + ij] = (part[0] + part[1]) + (part[2] + part[3]);
  if (t < F) {
    float a = 0.f;
    for (int pw = 0; pw < Wp; ++pw) a += red[pw * F + t];
    wsb[768 + t] = a;
  }
}

// dw[q] += sum_b ws[b][q] (q < 768), dbias[f] += sum_b ws[b][768 + f]: 64 outputs x 4 clip slices per workgroup
__global__ __launch_bounds__(256) void patchify_bwd2_reduce_kernel(const float* __restrict__ ws, int B, float* __restrict__ dw,
                                                                   float* __restrict__ dbias) {
  __shared__ float part[256];
  const int t = threadIdx.x, q = blockIdx.x * 64 + (t & 63), sl = t >> 6;
  float a = 0.f;
  if (q < PB2_OUT)
    for (int b = sl; b < B; b += 4) a += ws[(long)b * PB2_OUT + q];
  part[t] = a;
  __syncthreads();
  if (sl == 0 && q < PB2_OUT) {
    a = (part[t] + part[t + 64]) + (part[t + 128] + part[t + 192]);
    atomicAdd(q < 768 ? dw + q : dbias + (q - 768), a);
  }
}

// ------------------------------------------------------------------ node mean
template <typename T>
__global__ __launch_bounds__(256) void node_mean_fwd_kernel(const T* __restrict__ x, int N, int C,
                                                            float* __restrict__ out) {
  constexpr int NV = Chunk<T>::N;
  const int b = blockIdx.x, CV = C / NV;
  for (int cv = blockIdx.y * blockDim.x + threadIdx.x; cv < CV; cv += gridDim.y * blockDim.x) {
    float s[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) s[e] = 0.f;
    for (int n = 0; n < N; ++n) {
      float v[NV];
      Chunk<T>::load(x + ((long)b * N + n) * C + NV * cv, v);
#pragma unroll
      for (int e = 0; e < NV; ++e) s[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) out[(long)b * C + NV * cv + e] = s[e] / (float)N;
  }
}
template <typename T>
__global__ __launch_bounds__(256) void node_mean_bwd_kernel(const float* __restrict__ dout, int N, int C,
                                                            long nchunks, T* __restrict__ dx) {
  constexpr int NV = Chunk<T>::N;
  const int CV = C / NV;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nchunks; q += (long)gridDim.x * blockDim.x) {
    const int cv = (int)(q % CV);
    const long b = q / ((long)CV * N);
    float v[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) v[e] = dout[b * C + NV * cv + e] / (float)N;
    Chunk<T>::store(dx + q * NV, v);
  }
}

// ------------------------------------------------------------------ ELU', L2 normalise
__global__ void elu_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, long n,
                               float* __restrict__ din) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float o = out[i];
    din[i] = dout[i] * (o > 0.f ? 1.f : o + 1.f);      // d/dx elu(x) = exp(x) = elu(x)+1 for x<=0
  }
}

// z = p / max(|p|, eps): one wave per row
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* __restrict__ p, int B, int d, float eps,
                                                         float* __restrict__ z, float* __restrict__ norm) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;
  float ss = 0.f;
  for (int c = lane; c < d; c += 64) { const float v = p[(long)row * d + c]; ss += v * v; }
  ss = wave_sum(ss);
  const float nr = sqrtf(ss), den = fmaxf(nr, eps);
  for (int c = lane; c < d; c += 64) z[(long)row * d + c] = p[(long)row * d + c] / den;
  if (lane == 0) norm[row] = nr;
}
// dp = (dz - z (z.dz)) / |p|  when |p| > eps, else dz / eps
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ z,
                                                         const float* __restrict__ norm, int B, int d, float eps,
                                                         float* __restrict__ dp) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;
  float dot = 0.f;
  for (int c = lane; c < d; c += 64) dot += z[(long)row * d + c] * dz[(long)row * d + c];
  dot = wave_sum(dot);
  const float nr = norm[row];
  for (int c = lane; c < d; c += 64) {
    const long o = (long)row * d + c;
    dp[o] = nr > eps ? (dz[o] - z[o] * dot) / nr : dz[o] / eps;
  }
}

// ------------------------------------------------------------------ clip_grad_norm_ + Adam
constexpr int SUMSQ_PER_BLOCK = 256 * 4 * 16;
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, float* __restrict__ partial) {
  __shared__ double red[4];
  const long base = (long)blockIdx.x * SUMSQ_PER_BLOCK;
  double s = 0.0;
  for (int it = 0; it < 16; ++it) {
    const long i = base + ((long)it * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
      s += (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3];
    } else {
      for (long j = i; j < n && j < i + 4; ++j) s += (double)g[j] * g[j];
    }
  }
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (float)(red[0] + red[1] + red[2] + red[3]);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long n,
                                                   const float* __restrict__ hyper, const int64_t* __restrict__ step,
                                                   const float* __restrict__ partial, int nblocks,
                                                   float* __restrict__ gnorm_out) {
  __shared__ float coef_s;
  __shared__ int skip_s;
  __shared__ double red[4];
  {  // every block recomputes the global norm from the partials (<= a few thousand floats, L2-resident)
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += blockDim.x) s += (double)partial[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float norm = (float)sqrt(red[0] + red[1] + red[2] + red[3]);
      const float max_norm = hyper[4];
      float c = 1.f;
      if (max_norm > 0.f) { c = max_norm / (norm + 1e-6f); c = c < 1.f ? c : 1.f; }   // torch: clamp(max=1)
      coef_s = c;
      skip_s = !isfinite(norm);     // NaN/Inf loss => NaN/Inf gradients: skip the batch like train.py:65-68
      if (blockIdx.x == 0 && gnorm_out != nullptr) gnorm_out[0] = norm;
    }
    __syncthreads();
  }
  if (skip_s) return;
  const float coef = coef_s;
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3];
  const double t = (double)(*step + 1);                 // the host-visible counter is bumped by adam_tick_kernel
  const float bc1 = (float)(1.0 - pow((double)b1, t));
  const float bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, t));
  const float step_size = lr / bc1;
  // 16 bytes per lane and access (seven streams of 73.5 MB: the scalar form ran at 3.7 TB/s); same per-element expressions
  const long n4 = (reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                   reinterpret_cast<uintptr_t>(v)) % 16 == 0 ? n / 4 : 0;
  auto upd = [&](float gi_, float& mi_, float& vi_, float& pi_) {
    const float gi = gi_ * coef;
    const float mi = mi_ * b1 + (1.f - b1) * gi;        // exp_avg.lerp_(grad, 1-beta1)
    const float vi = vi_ * b2 + (1.f - b2) * gi * gi;
    mi_ = mi;
    vi_ = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi_ -= step_size * (mi / denom);
  };
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 g4 = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 m4 = reinterpret_cast<f32x4*>(m)[i], v4 = reinterpret_cast<f32x4*>(v)[i], p4 = reinterpret_cast<f32x4*>(p)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {          // (vector elements do not bind to references)
      float me = m4[e], ve = v4[e], pe = p4[e];
      upd(g4[e], me, ve, pe);
      m4[e] = me; v4[e] = ve; p4[e] = pe;
    }
    reinterpret_cast<f32x4*>(m)[i] = m4;
    reinterpret_cast<f32x4*>(v)[i] = v4;
    reinterpret_cast<f32x4*>(p)[i] = p4;
  }
  for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    upd(g[i], m[i], v[i], p[i]);
}
__global__ void adam_tick_kernel(int64_t* step, const float* gnorm) {
  if (gnorm == nullptr || isfinite(gnorm[0])) *step += 1;
}

// ------------------------------------------------------------------ (B,C,N) <-> rows (B*N, C): 32x32 LDS transpose
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void transpose_kernel(const TS* __restrict__ src, long src_batch, long src_ld,
                                                        TD* __restrict__ dst, long dst_batch, long dst_ld,
                                                        int R, int S) {   // src[b][r][s] -> dst[b][s][r]
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int r0 = blockIdx.y * 32, s0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;    // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int rr = r0 + i, ss = s0 + tx;
    if (rr < R && ss < S) tile[i][tx] = (float)src[b * src_batch + (long)rr * src_ld + ss];
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int ss = s0 + i, rr = r0 + tx;
    if (rr < R && ss < S) dst[b * dst_batch + (long)ss * dst_ld + rr] = (TD)tile[tx][i];
  }
}

}  // namespace

extern "C" int nsid_im2col3_fwd(const void* x, int B, int N, int C, void* col, int dtype, void* stream) {
  NSID_REQUIRE(x && col && B > 0 && N > 0 && C > 0 && NSID_DTYPE_OK(dtype) && nsid_aligned16(x) && nsid_aligned16(col));
  const int nv = dtype == NSID_BF16 ? 8 : 4;
  NSID_REQUIRE(C % nv == 0);
  const int No = (N - 1) / 2 + 1;
  NSID_DISPATCH_DTYPE(dtype, T, {
    NSID_LAUNCH((im2col3_fwd_kernel<T>), dim3(grid_for((long)B * No * 3 * (C / nv))), dim3(256), 0,
                static_cast<hipStream_t>(stream), static_cast<const T*>(x), B, N, No, C, static_cast<T*>(col));
  });
  return nsid_launch_status();
}
extern "C" int nsid_im2col3_bwd(const void* dcol, int B, int N, int C, void* dx, int dtype, void* stream) {
  NSID_REQUIRE(dcol && dx && B > 0 && N > 0 && C > 0 && NSID_DTYPE_OK(dtype) && nsid_aligned16(dcol) && nsid_aligned16(dx));
  const int nv = dtype == NSID_BF16 ? 8 : 4;
  NSID_REQUIRE(C % nv == 0);
  const int No = (N - 1) / 2 + 1;
  NSID_DISPATCH_DTYPE(dtype, T, {
    NSID_LAUNCH((im2col3_bwd_kernel<T>), dim3(grid_for((long)B * N * (C / nv))), dim3(256), 0,
                static_cast<hipStream_t>(stream), static_cast<const T*>(dcol), B, N, No, C, static_cast<T*>(dx));
  });
  return nsid_launch_status();
}
extern "C" int nsid_pack_ds_weight(const float* w, int Cout, int Cin, float* wp, void* stream) {
  NSID_REQUIRE(w && wp && Cout > 0 && Cin > 0);
  NSID_LAUNCH(pack_ds_weight_kernel, dim3(grid_for((long)Cout * 3 * Cin)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), w, Cout, Cin, wp);
  return nsid_launch_status();
}
extern "C" int nsid_pack_ds_weight_bwd(const float* w, int Cout, int Cin, float* wb, void* stream) {
  NSID_REQUIRE(w && wb && Cout > 0 && Cin > 0);
  NSID_LAUNCH(pack_ds_weight_bwd_kernel, dim3(grid_for(2L * Cout * Cin)), dim3(256), 0, static_cast<hipStream_t>(stream),
              w, Cout, Cin, wb);
  return nsid_launch_status();
}
extern "C" int nsid_unpack_ds_wgrad(const float* dwp, int Cout, int Cin, float* dw, void* stream) {
  NSID_REQUIRE(dwp && dw && Cout > 0 && Cin > 0);
  NSID_LAUNCH(unpack_ds_wgrad_kernel, dim3(grid_for((long)Cout * 3 * Cin)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), dwp, Cout, Cin, dw);
  return nsid_launch_status();
}

extern "C" int nsid_ds_prepack(int n, const float* const* w, void* const* wp16, void* const* wb16, float* const* dwp, const int* Cout,
                               const int* Cin, void* stream) {
  NSID_REQUIRE(n > 0 && n <= DSP_LAYERS && w && wp16 && wb16 && Cout && Cin);
  DsPrepArgs a{};
  long most = 0;
  for (int i = 0; i < n; ++i) {
    NSID_REQUIRE(w[i] && wp16[i] && wb16[i] && Cout[i] > 0 && Cin[i] > 0);
    a.w[i] = w[i]; a.wp16[i] = static_cast<__bf16*>(wp16[i]); a.wb16[i] = static_cast<__bf16*>(wb16[i]);
    a.dwp[i] = dwp ? dwp[i] : nullptr; a.Cout[i] = Cout[i]; a.Cin[i] = Cin[i];
    most = std::max(most, (long)Cout[i] * 3 * Cin[i]);
  }
  NSID_LAUNCH(ds_prepack_kernel, dim3(grid_for(most, 256), n), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return nsid_launch_status();
}
extern "C" int nsid_peak_patchify_fwd(const float* spec, const float* w, const float* bias, int B, int H, int W, int pb,
                                      int pf, int F, void* out, int ldo, float* minmax, int out_dtype, void* stream) {
  NSID_REQUIRE(spec && w && bias && out && B > 0 && H > 1 && W > 1 && pb > 0 && pf > 0 && F > 0);
  NSID_REQUIRE(H % pb == 0 && W % pf == 0 && ldo >= F && NSID_DTYPE_OK(out_dtype));
  const size_t bytes = ((size_t)F * 3 * pb * pf + 8 + (size_t)H * (W + 8)) * sizeof(float);
  // the clip is staged whole (its min / max come first): 35 KB for grafp.yaml's 64 x 128, 139 KB for a 256-mel input
  NSID_REQUIRE(bytes <= NSID_LDS_MAX && W % 4 == 0 && (F * 3 * pb * pf) % 4 == 0 && nsid_aligned16(spec) && pb * pf <= 64);
  NSID_DISPATCH_DTYPE(out_dtype, T, {
    if (pb == 4 && pf == 8) {
      NSID_LAUNCH_LDS((patchify_fwd_kernel<T, 32, 4, 8>), dim3(B), dim3(256), bytes, static_cast<hipStream_t>(stream), spec, w,
                      bias, H, W, pb, pf, F, static_cast<T*>(out), ldo, minmax);
    } else if (pb * pf == 32) {
      NSID_LAUNCH_LDS((patchify_fwd_kernel<T, 32>), dim3(B), dim3(256), bytes, static_cast<hipStream_t>(stream), spec, w,
                      bias, H, W, pb, pf, F, static_cast<T*>(out), ldo, minmax);
    } else {
      NSID_LAUNCH_LDS((patchify_fwd_kernel<T, 64>), dim3(B), dim3(256), bytes, static_cast<hipStream_t>(stream), spec, w,
                      bias, H, W, pb, pf, F, static_cast<T*>(out), ldo, minmax);
    }
  });
  return nsid_launch_status();
}
extern "C" int nsid_peak_patchify_bwd(const float* spec, const float* minmax, const void* out, const void* dout,
                                      int ldo, int B, int H, int W, int pb, int pf, int F, float* dw, float* dbias,
                                      int out_dtype, void* stream) {
  NSID_REQUIRE(spec && minmax && out && dout && dw && dbias && B > 0 && H % pb == 0 && W % pf == 0 && ldo >= F);
  NSID_REQUIRE(NSID_DTYPE_OK(out_dtype));
  // a clip beyond 64 KB of LDS (256 mel bins: 172 KB) goes through in bands of patch rows, the fewest that fit
  int bands = 1;
  auto lds_bytes = [&](int nb) {
    const int Hb = H / nb;
    return ((size_t)(Hb / pb) * (W / pf) * F + (size_t)Hb * (W + 8) + (size_t)(Hb / pb + W / pf) * F) * sizeof(float);
  };
  while (lds_bytes(bands) > 64 * 1024 && (H / pb) % (2 * bands) == 0) bands *= 2;
  const size_t bytes = lds_bytes(bands);
  NSID_REQUIRE(bytes <= 64 * 1024 && (long)F * 3 * pb * pf <= 4 * 256 && F <= 256 && W % 4 == 0 && nsid_aligned16(spec));
  NSID_REQUIRE(((H / bands / pb) * (W / pf) * F) % 4 == 0 && (long)B * bands < (1L << 30));
  NSID_DISPATCH_DTYPE(out_dtype, T, {
    NSID_LAUNCH((patchify_bwd_kernel<T>), dim3(B * bands < 256 ? B * bands : 256), dim3(256), bytes, static_cast<hipStream_t>(stream),
                spec, minmax, static_cast<const T*>(out), static_cast<const T*>(dout), ldo, B, H, W, pb, pf, F, dw, dbias, bands);
  });
  return nsid_launch_status();
}

// the same with a caller-provided workspace of B * 776 floats (GraFP's patch: pb = 4, pf = 8, F = 8, 64 x 128 clips): partial sums per
// clip by plain stores + one reduce launch instead of B * 776 atomics on 776 addresses. Other shapes: nsid_peak_patchify_bwd.
extern "C" int nsid_peak_patchify_bwd_ws(const float* spec, const float* minmax, const void* out, const void* dout, int ldo, int B,
                                         int H, int W, int pb, int pf, int F, float* dw, float* dbias, float* ws, int out_dtype,
                                         void* stream) {
  NSID_REQUIRE(spec && minmax && out && dout && dw && dbias && ws && B > 0 && ldo >= F && NSID_DTYPE_OK(out_dtype));
  NSID_REQUIRE(H == 64 && W == 128 && pb == 4 && pf == 8 && F == 8 && ldo % (out_dtype == NSID_BF16 ? 8 : 4) == 0);
  NSID_REQUIRE(nsid_aligned16(spec) && nsid_aligned16(out) && nsid_aligned16(dout));
  hipStream_t s = static_cast<hipStream_t>(stream);
  NSID_DISPATCH_DTYPE(out_dtype, T, {
    NSID_LAUNCH((patchify_bwd2_kernel<T>), dim3(B), dim3(256), 0, s, spec, minmax, static_cast<const T*>(out),
                static_cast<const T*>(dout), ldo, ws);
  });
  NSID_LAUNCH(patchify_bwd2_reduce_kernel, dim3((PB2_OUT + 63) / 64), dim3(256), 0, s, ws, B, dw, dbias);
  return nsid_launch_status();
}

extern "C" int nsid_node_mean_fwd(const void* x, int B, int N, int C, float* out, int x_dtype, void* stream) {
  NSID_REQUIRE(x && out && B > 0 && N > 0 && C > 0 && NSID_DTYPE_OK(x_dtype) && nsid_aligned16(x));
  const int nv = x_dtype == NSID_BF16 ? 8 : 4;
  NSID_REQUIRE(C % nv == 0);
  NSID_DISPATCH_DTYPE(x_dtype, T, {
    NSID_LAUNCH((node_mean_fwd_kernel<T>), dim3(B, (C / nv + 255) / 256), dim3(256), 0,
                static_cast<hipStream_t>(stream), static_cast<const T*>(x), N, C, out);
  });
  return nsid_launch_status();
}
extern "C" int nsid_node_mean_bwd(const float* dout, int B, int N, int C, void* dx, int dx_dtype, void* stream) {
  NSID_REQUIRE(dout && dx && B > 0 && N > 0 && C > 0 && NSID_DTYPE_OK(dx_dtype) && nsid_aligned16(dx));
  const int nv = dx_dtype == NSID_BF16 ? 8 : 4;
  NSID_REQUIRE(C % nv == 0);
  const long nchunks = (long)B * N * (C / nv);
  NSID_DISPATCH_DTYPE(dx_dtype, T, {
    NSID_LAUNCH((node_mean_bwd_kernel<T>), dim3(grid_for(nchunks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                dout, N, C, nchunks, static_cast<T*>(dx));
  });
  return nsid_launch_status();
}
extern "C" int nsid_elu_bwd(const float* dout, const float* out, long n, float* din, void* stream) {
  NSID_REQUIRE(dout && out && din && n > 0);
  NSID_LAUNCH(elu_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), dout, out, n,
                     din);
  return nsid_launch_status();
}
extern "C" int nsid_l2norm_fwd(const float* p, int B, int d, float eps, float* z, float* norm, void* stream) {
  NSID_REQUIRE(p && z && norm && B > 0 && d > 0);
  NSID_LAUNCH(l2norm_fwd_kernel, dim3((B + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), p, B, d, eps,
                     z, norm);
  return nsid_launch_status();
}
extern "C" int nsid_l2norm_bwd(const float* dz, const float* z, const float* norm, int B, int d, float eps, float* dp,
                               void* stream) {
  NSID_REQUIRE(dz && z && norm && dp && B > 0 && d > 0);
  NSID_LAUNCH(l2norm_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), dz, z, norm,
                     B, d, eps, dp);
  return nsid_launch_status();
}

extern "C" int nsid_sumsq_blocks(long n) { return (int)((n + SUMSQ_PER_BLOCK - 1) / SUMSQ_PER_BLOCK); }
extern "C" int nsid_sumsq_partial(const float* g, long n, float* partial, void* stream) {
  NSID_REQUIRE(g && partial && n > 0 && nsid_aligned16(g));
  NSID_LAUNCH(sumsq_kernel, dim3(nsid_sumsq_blocks(n)), dim3(256), 0, static_cast<hipStream_t>(stream), g, n,
                     partial);
  return nsid_launch_status();
}
extern "C" int nsid_adam_step(float* p, const float* g, float* m, float* v, long n, const float* hyper, int64_t* step,
                              const float* partial, int nblocks, float* gnorm_out, void* stream) {
  NSID_REQUIRE(p && g && m && v && hyper && step && partial && n > 0 && nblocks > 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  NSID_LAUNCH(adam_kernel, dim3(grid_for(n, 4096)), dim3(256), 0, s, p, g, m, v, n, hyper, step, partial,
                     nblocks, gnorm_out);
  NSID_LAUNCH(adam_tick_kernel, dim3(1), dim3(1), 0, s, step, (const float*)gnorm_out);
  return nsid_launch_status();
}

// ------------------------------------------------------------------ log-mel front end (modules/transformations.py:27-34,
// :94-105 = torchaudio MelSpectrogram(n_fft, win_length, hop, n_mels; center=True reflect, Hann periodic, power 2, HTK mel,
// norm None) + AmplitudeToDB(power, top_db None) + unfold(size=n_frames, step=n_frames*(1-overlap)))
// The STFT itself is a fp32 MFMA GEMM: frames (row stride = hop, overlapping) x [window*cos | -window*sin] (nsid_linear_fwd).
__global__ void reflect_pad_kernel(const float* __restrict__ x, long L, int pad, float* __restrict__ out) {
  const long n = L + 2L * pad;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    long j = i - pad;
    if (j < 0) j = -j;                           // torch 'reflect': no edge repeat
    if (j >= L) j = 2 * (L - 1) - j;
    out[i] = x[j];
  }
}

// one block per frame: power spectrum of the frame into LDS, then one thread per mel band sums its (contiguous) non-zero
// filter range; out is (n_mels, T) like torchaudio
__global__ __launch_bounds__(256) void power_mel_db_kernel(const float* __restrict__ spec, long ld, int n_freq,
                                                           const float* __restrict__ fb, const int* __restrict__ band,
                                                           int n_mels, int T, float* __restrict__ out) {
  extern __shared__ float pw[];                  // [n_freq]
  const int t = blockIdx.x;
  const float* row = spec + (long)t * ld;
  for (int f = threadIdx.x; f < n_freq; f += blockDim.x) {
    const float re = row[f], im = row[n_freq + f];
    pw[f] = re * re + im * im;
  }
  __syncthreads();
  for (int m = threadIdx.x; m < n_mels; m += blockDim.x) {
    float acc = 0.f;
    for (int f = band[2 * m]; f < band[2 * m + 1]; ++f) acc += fb[(long)m * n_freq + f] * pw[f];
    out[(long)m * T + t] = 10.0f * log10f(fmaxf(acc, 1e-10f));          // AmplitudeToDB: amin 1e-10, ref 1.0
  }
}

// (n_mels, T) -> (S, n_mels, n_frames): segment s covers frames [s*step, s*step + n_frames)
__global__ void unfold_segments_kernel(const float* __restrict__ lm, int n_mels, int T, int n_frames, int step, int S,
                                       float* __restrict__ out) {
  const long n = (long)S * n_mels * n_frames;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)(i % n_frames), m = (int)((i / n_frames) % n_mels);
    const long s = i / ((long)n_frames * n_mels);
    out[i] = lm[(long)m * T + s * step + f];
  }
}

// the same out of a PACK of songs (n_rows, ld) with the songs side by side in the columns: segments s0 .. s0 + nseg - 1 of the
// pack's segment list, segment s starting at column seg_col[s] -> out (nseg, n_rows, n_frames)
__global__ void unfold_segments_ragged_kernel(const float* __restrict__ spec, long ld, int n_rows, int n_frames,
                                              const long* __restrict__ seg_col, long s0, int nseg, float* __restrict__ out) {
  const long n = (long)nseg * n_rows * n_frames;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)(i % n_frames), m = (int)((i / n_frames) % n_rows);
    const long s = i / ((long)n_frames * n_rows);
    out[i] = spec[(long)m * ld + seg_col[s0 + s] + f];
  }
}

extern "C" int nsid_unfold_segments_ragged(const float* spec, long ld, int n_rows, int n_frames, const long* seg_col, long s0,
                                           int nseg, float* out, void* stream) {
  NSID_REQUIRE(spec && seg_col && out && n_rows > 0 && n_frames > 0 && ld >= n_frames && s0 >= 0 && nseg > 0);
  nsid_count(NSID_C_unfold_segments_ragged);
  NSID_LAUNCH(unfold_segments_ragged_kernel, dim3(grid_for((long)nseg * n_rows * n_frames)), dim3(256), 0,
              static_cast<hipStream_t>(stream), spec, ld, n_rows, n_frames, seg_col, s0, nseg, out);
  return nsid_launch_status();
}

extern "C" int nsid_reflect_pad(const float* x, long L, int pad, float* out, void* stream) {
  NSID_REQUIRE(x && out && L > 1 && pad >= 0 && pad < L);
  NSID_LAUNCH(reflect_pad_kernel, dim3(grid_for(L + 2L * pad)), dim3(256), 0, static_cast<hipStream_t>(stream), x, L, pad,
              out);
  return nsid_launch_status();
}
extern "C" int nsid_power_mel_db(const float* spec, long ld, int n_freq, const float* fb, const int* band, int n_mels,
                                 int T, float* out, void* stream) {
  NSID_REQUIRE(spec && fb && band && out && n_freq > 0 && n_mels > 0 && T > 0 && ld >= 2L * n_freq);
  NSID_REQUIRE((size_t)n_freq * sizeof(float) <= 48 * 1024);
  NSID_LAUNCH(power_mel_db_kernel, dim3(T), dim3(256), (size_t)n_freq * sizeof(float), static_cast<hipStream_t>(stream),
              spec, ld, n_freq, fb, band, n_mels, T, out);
  return nsid_launch_status();
}
extern "C" int nsid_unfold_segments(const float* logmel, int n_mels, int T, int n_frames, int step, int S, float* out,
                                    void* stream) {
  NSID_REQUIRE(logmel && out && n_mels > 0 && n_frames > 0 && step > 0 && S > 0 && (long)(S - 1) * step + n_frames <= T);
  NSID_LAUNCH(unfold_segments_kernel, dim3(grid_for((long)S * n_mels * n_frames)), dim3(256), 0,
              static_cast<hipStream_t>(stream), logmel, n_mels, T, n_frames, step, S, out);
  return nsid_launch_status();
}

// bf16 shadow copy of weights (RNE, the rounding the GEMMs apply when they stage fp32 weights): n % 8 == 0
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, long n8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float v[8];
    Chunk<float>::load(src + 8 * i, v);
    Chunk<float>::load(src + 8 * i + 4, v + 4);
    Chunk<__bf16>::store(dst + 8 * i, v);
  }
}
extern "C" int nsid_f32_to_bf16(const float* src, void* dst, long n, void* stream) {
  NSID_REQUIRE(src && dst && n > 0 && n % 8 == 0 && nsid_aligned16(src) && nsid_aligned16(dst));
  NSID_LAUNCH(f32_to_bf16_kernel, dim3(grid_for(n / 8, 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), src,
              static_cast<__bf16*>(dst), n / 8);
  return nsid_launch_status();
}

extern "C" int nsid_bcn_to_rows(const float* x, int B, int C, int N, void* rows, int ld, int rows_dtype, void* stream) {
  NSID_REQUIRE(x && rows && B > 0 && C > 0 && N > 0 && ld >= C && NSID_DTYPE_OK(rows_dtype));
  NSID_DISPATCH_DTYPE(rows_dtype, T, {
    NSID_LAUNCH((transpose_kernel<float, T>), dim3((N + 31) / 32, (C + 31) / 32, B), dim3(256), 0,
                static_cast<hipStream_t>(stream), x, (long)C * N, (long)N, static_cast<T*>(rows), (long)N * ld, (long)ld,
                C, N);
  });
  return nsid_launch_status();
}
extern "C" int nsid_rows_to_bcn(const void* rows, int ld, int B, int C, int N, float* x, int rows_dtype, void* stream) {
  NSID_REQUIRE(x && rows && B > 0 && C > 0 && N > 0 && ld >= C && NSID_DTYPE_OK(rows_dtype));
  NSID_DISPATCH_DTYPE(rows_dtype, T, {
    NSID_LAUNCH((transpose_kernel<T, float>), dim3((C + 31) / 32, (N + 31) / 32, B), dim3(256), 0,
                static_cast<hipStream_t>(stream), static_cast<const T*>(rows), (long)N * ld, (long)ld, x, (long)C * N,
                (long)N, N, C);
  });
  return nsid_launch_status();
}

// ------------------------------------------------------------------ step plumbing that used to be ATen kernels inside the
// captured step (zero_grad's fill, the loss hand-over copy, autograd's "grad_output *" scaling of the NT-Xent gradients)
__global__ __launch_bounds__(256) void fill_zero_kernel(f32x4* __restrict__ p, long n16) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) p[i] = z;
}
__global__ void fill_zero_tail_kernel(unsigned char* __restrict__ p, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = 0;
}
// out[i] = x[i] * (s ? s[0] : 1)   (out may alias x)
__global__ void scale_f32_kernel(const float* __restrict__ x, const float* __restrict__ s, long n, float* __restrict__ out) {
  const float f = s != nullptr ? s[0] : 1.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = x[i] * f;
}

extern "C" int nsid_fill_zero(void* p, size_t bytes, void* stream) {
  NSID_REQUIRE(p && bytes > 0 && nsid_aligned16(p));
  const long n16 = (long)(bytes / 16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n16 > 0) {
    NSID_LAUNCH(fill_zero_kernel, dim3(grid_for(n16, 2048)), dim3(256), 0, s, static_cast<f32x4*>(p), n16);
    if (nsid_launch_status() != NSID_OK) return NSID_ELAUNCH;
  }
  if (bytes % 16) {
    NSID_LAUNCH(fill_zero_tail_kernel, dim3(1), dim3(64), 0, s, static_cast<unsigned char*>(p) + 16 * n16,
                (long)(bytes % 16));
    return nsid_launch_status();
  }
  return NSID_OK;
}
extern "C" int nsid_scale_f32(const float* x, const float* scale, long n, float* out, void* stream) {
  NSID_REQUIRE(x && out && n > 0);
  NSID_LAUNCH(scale_f32_kernel, dim3(grid_for(n, 1024)), dim3(256), 0, static_cast<hipStream_t>(stream), x, scale, n, out);
  return nsid_launch_status();
}
