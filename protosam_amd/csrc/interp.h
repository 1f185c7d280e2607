// Interpolation helpers shared by several translation units (resample.hip, decoder.hip, coarse_batch.hip). Moved here
// unchanged so that every kernel that resamples computes the same bits.
#pragma once
#include "common.h"

// ATen's area_pixel_compute_source_index (align_corners=False), see resample.hip's header comment.
struct Lin {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lin lin_src(int dst, float scale, int in_size) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  int i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  Lin r;
  r.i0 = i0;
  r.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  float l1 = s - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
  r.l1 = l1;
  r.l0 = 1.f - l1;
  return r;
}
__device__ __forceinline__ float bilerp(const float* __restrict__ p, int W, const Lin& y, const Lin& x) {
  const float* r0 = p + (size_t)y.i0 * W;
  const float* r1 = p + (size_t)y.i1 * W;
  return y.l0 * (x.l0 * r0[x.i0] + x.l1 * r0[x.i1]) + y.l1 * (x.l0 * r1[x.i0] + x.l1 * r1[x.i1]);
}

// Mask post-processing. variant 0: bilinear align_corners=False (pip segment_anything 1.0 `Sam`),
// 1: bilinear align_corners=True (vendored `SamBatched`, sam.py:313-320), 2: nearest (vendored `Sam`, sam.py:154-160),
// 3: sigmoid, then bilinear align_corners=False (MedSAM inference, models/ProtoMedSAM.py:49-60; threshold 0.5).
struct Lin2 {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lin2 lin2(int dst, int in_size, int out_size, int align) {
  float s;
  if (align) {
    const float sc = out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
    s = sc * (float)dst;
  } else {
    const float sc = (float)in_size / (float)out_size;
    s = sc * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
  }
  int i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  Lin2 r;
  r.i0 = i0;
  r.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  float l1 = s - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
  r.l1 = l1;
  r.l0 = 1.f - l1;
  return r;
}
__device__ __forceinline__ float up_sample(const float* __restrict__ p, int IN, int MID, int y, int x, int variant) {
  // value of interpolate(p[IN,IN] -> [MID,MID]) at (y, x)
  if (variant == 2) {
    const float sc = (float)IN / (float)MID;
    int sy = (int)floorf((float)y * sc), sx = (int)floorf((float)x * sc);
    sy = sy < IN - 1 ? sy : IN - 1;
    sx = sx < IN - 1 ? sx : IN - 1;
    return p[(size_t)sy * IN + sx];
  }
  Lin2 ly = lin2(y, IN, MID, variant == 1), lx = lin2(x, IN, MID, variant == 1);
  const float* r0 = p + (size_t)ly.i0 * IN;
  const float* r1 = p + (size_t)ly.i1 * IN;
  float a = r0[lx.i0], b = r0[lx.i1], c = r1[lx.i0], d = r1[lx.i1];
  if (variant == 3) {  // torch.sigmoid(low_res_logits) BEFORE the bilinear resize (models/ProtoMedSAM.py:49-56)
    a = 1.f / (1.f + expf(-a));
    b = 1.f / (1.f + expf(-b));
    c = 1.f / (1.f + expf(-c));
    d = 1.f / (1.f + expf(-d));
  }
  return ly.l0 * (lx.l0 * a + lx.l1 * b) + ly.l1 * (lx.l0 * c + lx.l1 * d);
}
