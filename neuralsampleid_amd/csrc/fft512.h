// The 512-point complex FFT of one wave, shared by frontend.hip (real FFT of 1 024 samples) and augment.hip (2 048 samples):
// 512 = 8 x 8 x 8, three radix-8 passes in registers (8 points per lane) with two transposes through LDS between them.
//   n = 64a + 8b + c, k = k0 + 8k1 + 64k2:  pass 1 sums over a (lane = 8b + c), twiddle W512^((8b+c) k0);
//                                           pass 2 sums over b (lane = 8k0 + c), twiddle W64^(c k1);
//                                           pass 3 sums over c (lane = k0 + 8k1) and leaves Z[k] in natural order.
// LDS layout of the two transposes (8-byte complex elements): see the head of frontend.hip.
#pragma once
#include "nsid_common.h"

#ifndef FE_HD
#define FE_HD __host__ __device__ __forceinline__
#endif

constexpr int FE_BUF = 72 * 8;            // complex elements of a wave's private exchange region (the largest of the three layouts)
constexpr float FE_RSQRT2 = 0.70710678118654752440f;

FE_HD f32x2 fe_cmul(const f32x2 a, const f32x2 w) { return f32x2{a[0] * w[0] - a[1] * w[1], a[0] * w[1] + a[1] * w[0]}; }

// y[k] = sum_a v[a] e^(-2 pi i a k / 8), in place
FE_HD void fe_radix8(f32x2* v) {
  // no contraction here: the 1/sqrt 2 products would fuse with the following sums into packed FMAs with a constant multiplier,
  // the form tests/test_cabi.py keeps out of the library
#pragma clang fp contract(off)
  f32x2 u[4], w[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    u[a] = v[a] + v[a + 4];
    w[a] = v[a] - v[a + 4];
  }
  w[1] = f32x2{(w[1][0] + w[1][1]) * FE_RSQRT2, (w[1][1] - w[1][0]) * FE_RSQRT2};       // * W8^1 = (1 - i)/sqrt 2
  w[2] = f32x2{w[2][1], -w[2][0]};                                                      // * W8^2 = -i
  w[3] = f32x2{(w[3][1] - w[3][0]) * FE_RSQRT2, -(w[3][0] + w[3][1]) * FE_RSQRT2};      // * W8^3 = (-1 - i)/sqrt 2
  {
    const f32x2 p0 = u[0] + u[2], p1 = u[0] - u[2], q0 = u[1] + u[3], d = u[1] - u[3];
    const f32x2 q1 = f32x2{d[1], -d[0]};
    v[0] = p0 + q0; v[4] = p0 - q0; v[2] = p1 + q1; v[6] = p1 - q1;
  }
  {
    const f32x2 p0 = w[0] + w[2], p1 = w[0] - w[2], q0 = w[1] + w[3], d = w[1] - w[3];
    const f32x2 q1 = f32x2{d[1], -d[0]};
    v[1] = p0 + q0; v[5] = p0 - q0; v[3] = p1 + q1; v[7] = p1 - q1;
  }
}

// the per-lane twiddles of the passes: constant over frames, loaded once per wave (tu: the untangling pass of frontend.hip)
struct FeTw {
  f32x2 t1[7], t2[7], tu[4];
};

// read side of transpose 1 at lane 8 k0 + c
FE_HD void fe_read1(const int lane, const f32x2* buf, f32x2* v) {
  const int k0 = lane >> 3, c = lane & 7;
#pragma unroll
  for (int b = 0; b < 8; ++b) v[b] = buf[72 * k0 + 8 * b + c];
}
// pass 2 -> transpose 2
FE_HD void fe_pass2(const int lane, const FeTw& t, f32x2* v, f32x2* buf) {
  const int k0 = lane >> 3, c = lane & 7;
  fe_radix8(v);
  buf[66 * c + k0] = v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) buf[66 * c + k0 + 8 * k] = fe_cmul(v[k], t.t2[k - 1]);
}
// read side of transpose 2 at lane k0 + 8 k1
FE_HD void fe_read2(const int lane, const f32x2* buf, f32x2* v) {
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = buf[66 * c + lane];
}
