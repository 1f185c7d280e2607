// The per-pixel code of the two-stage resize (both resizes of Sam.postprocess_masks computed per output pixel), shared by
// amg_resize.hip and amg_crops.hip: the taps of every variant and the walk of one workgroup over rows of one plane. The header of
// amg_resize.hip says where each rounding comes from. Everything below runs with contraction off, whatever the including file's
// own setting: the pragma holds to the end of the translation unit.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

struct RsTap {
  int i0, i1;
  float l0, l1;
};

// Taps of interp.h's lin2 / lin_src as the kernels named there were compiled: the first stage of every bilinear variant, and the
// second stage of variant 0.
__device__ __forceinline__ RsTap rs_tap(int dst, int in_size, int out_size, int align) {
  float s;
  if (align) {
    const float sc = out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
    s = sc * (float)dst;
  } else {
    const float sc = (float)in_size / (float)out_size;
    s = fmaf(sc, (float)dst + 0.5f, -0.5f);
    s = s < 0.f ? 0.f : s;
  }
  int i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  RsTap r;
  r.i0 = i0;
  r.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  float l1 = s - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
  r.l1 = l1;
  r.l0 = 1.f - l1;
  return r;
}
// Taps of resize2d_kernel mode 1 (align_corners=True): the second stage of variant 1.
__device__ __forceinline__ RsTap rs_tap_ac(int dst, int in_size, int out_size) {
  const float sc = out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
  const float f = sc * (float)dst;
  RsTap r;
  r.i0 = min((int)f, in_size - 1);
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = fmaf(sc, (float)dst, -(float)r.i0);
  r.l0 = 1.f - r.l1;
  return r;
}
// nearest source index of both stages: min(floor(dst * in / out), in - 1)
__device__ __forceinline__ int rs_near(int dst, int in_size, int out_size) {
  const float sc = (float)in_size / (float)out_size;
  const int s = (int)floorf((float)dst * sc);
  return s < in_size - 1 ? s : in_size - 1;
}
// up_sample's bilinear value at first-stage row taps y, column taps x
__device__ __forceinline__ float rs_first(const float* __restrict__ p, int IN, const RsTap& y, const RsTap& x) {
  const float* r0 = p + (size_t)y.i0 * IN;
  const float* r1 = p + (size_t)y.i1 * IN;
  const float a = r0[x.i0], b = r0[x.i1], c = r1[x.i0], d = r1[x.i1];
  const float X = fmaf(x.l0, a, x.l1 * b), Y = fmaf(x.l0, c, x.l1 * d);
  return y.l0 * X + y.l1 * Y;
}
// the second stage's blend of the four first-stage values a b / c d
template <int V>
__device__ __forceinline__ float rs_second(const RsTap& y, const RsTap& x, float a, float b, float c, float d) {
  const float X = V == 0 ? fmaf(x.l0, a, x.l1 * b) : fmaf(x.l1, b, x.l0 * a);
  const float Y = fmaf(x.l0, c, x.l1 * d);
  return y.l0 * X + y.l1 * Y;
}

// f(y, x, value) for the output pixels of rows [y0, y1) of one plane, columns strided over the workgroup
template <int V, class F>
__device__ __forceinline__ void rs_walk(const float* __restrict__ src, int IN, int MID, int ih, int iw, int OH, int OW, int y0,
                                        int y1, F&& f) {
  for (int x = threadIdx.x; x < OW; x += blockDim.x) {
    if (V == 2) {
      const int sx = rs_near(rs_near(x, iw, OW), IN, MID);
      for (int y = y0; y < y1; ++y) {
        const int sy = rs_near(rs_near(y, ih, OH), IN, MID);
        f(y, x, src[(size_t)sy * IN + sx]);
      }
    } else {
      const RsTap tx = V == 0 ? rs_tap(x, iw, OW, 0) : rs_tap_ac(x, iw, OW);
      const RsTap fx0 = rs_tap(tx.i0, IN, MID, V == 1), fx1 = rs_tap(tx.i1, IN, MID, V == 1);
      int c0 = -1, c1 = -1;                    // the first-stage rows held in (a, b) and (c, d)
      float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
      for (int y = y0; y < y1; ++y) {
        const RsTap ty = V == 0 ? rs_tap(y, ih, OH, 0) : rs_tap_ac(y, ih, OH);
        float na, nb, nc, nd;
        if (ty.i0 == c0) {
          na = a; nb = b;
        } else if (ty.i0 == c1) {
          na = c; nb = d;
        } else {
          const RsTap fy = rs_tap(ty.i0, IN, MID, V == 1);
          na = rs_first(src, IN, fy, fx0); nb = rs_first(src, IN, fy, fx1);
        }
        if (ty.i1 == ty.i0) {
          nc = na; nd = nb;
        } else if (ty.i1 == c1) {
          nc = c; nd = d;
        } else if (ty.i1 == c0) {
          nc = a; nd = b;
        } else {
          const RsTap fy = rs_tap(ty.i1, IN, MID, V == 1);
          nc = rs_first(src, IN, fy, fx0); nd = rs_first(src, IN, fy, fx1);
        }
        a = na; b = nb; c = nc; d = nd;
        c0 = ty.i0; c1 = ty.i1;
        f(y, x, rs_second<V>(ty, tx, a, b, c, d));
      }
    }
  }
}
