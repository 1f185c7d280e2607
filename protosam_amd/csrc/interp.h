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

// Anti-aliased bilinear taps of one output index along one axis (aten UpSampleKernel.cpp,
// `_compute_indices_min_size_weights_aa` with the triangle filter), shared by psam_resize_aa and psam_image_intake so that
// the fused intake computes the bits of the unfused chain: scale = in / out, support = max(scale, 1), centre =
// scale * (i + 0.5), taps [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the input, weights
// triangle((j - centre + 0.5) / max(scale, 1)) normalised to sum 1. All fp32, one rounding per written operation.
struct AaTap {
  int xmin, xsize;
  float center, invscale, total;
};
__device__ __forceinline__ AaTap aa_tap(int i, int in_len, int out_len) {
  const float scale = (float)in_len / (float)out_len;
  const float support = scale >= 1.f ? scale : 1.f;
  AaTap t;
  t.invscale = scale >= 1.f ? 1.f / scale : 1.f;
  t.center = scale * ((float)i + 0.5f);
  int xmin = (int)(t.center - support + 0.5f);
  xmin = xmin > 0 ? xmin : 0;
  int xmax = (int)(t.center + support + 0.5f);
  xmax = xmax < in_len ? xmax : in_len;
  t.xmin = xmin;
  t.xsize = xmax - xmin;
  float total = 0.f;
  for (int j = 0; j < t.xsize; ++j) {
    float a = fabsf(((float)(j + xmin) - t.center + 0.5f) * t.invscale);
    total += a < 1.f ? 1.f - a : 0.f;
  }
  t.total = total;
  return t;
}
__device__ __forceinline__ float aa_weight(const AaTap& t, int j) {
  float a = fabsf(((float)(j + t.xmin) - t.center + 0.5f) * t.invscale);
  float w = a < 1.f ? 1.f - a : 0.f;
  if (t.total != 0.f) w /= t.total;
  return w;
}
// acc + w * v as one fused multiply-add (what the compiler made of `acc += w * v` in resize_aa_pass_kernel; spelled out so
// that every kernel that accumulates taps rounds alike whatever the contraction setting)
__device__ __forceinline__ float aa_mac(float acc, float w, float v) { return fmaf(w, v, acc); }

// Sam.preprocess normalisation of one value (modeling/sam.py:163-168), shared by psam_normalize_chw and psam_image_intake
__device__ __forceinline__ float norm_px(float v, float mean, float sd) { return (v - mean) / sd; }
