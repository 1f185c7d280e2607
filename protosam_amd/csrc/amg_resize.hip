// Automatic mask generation for images that are not at the model's input size, and for crops: the candidate statistics and the
// binary masks straight from the low-resolution logits, with BOTH resizes of Sam.postprocess_masks (modeling/sam.py:132-160 /
// :296-320) computed per output pixel and no plane written in between.
//
//  psam_mask_stats_resized    : psam_mask_stats' int32 [planes, 8] table over the OH x OW image
//  psam_mask_stats_resized_scored : the same, skipping the candidates that the predicted-IoU filter drops anyway
//  psam_mask_binarize_resized : psam_mask_binarize's uint8 masks (and {tp, fp, fn} against a label), written into a rectangle of
//                               larger frames (the generator's uncrop_masks placement)
//
// The value of output pixel (y, x) is the second-stage interpolation (source size ih x iw = predictor.input_size, so its taps
// clamp at ih - 1 / iw - 1 and never reach the padding) of the first-stage map IN -> MID. It has the bits of the chain it replaces,
// psam_mask_upsample -> crop to [ih, iw] -> psam_resize2d. Those kernels are compiled with -ffp-contract=fast, which lets the
// compiler choose the products it fuses, and it chose differently in each. Read from the gfx950 assembly of decoder.hip and
// resample.hip (hipcc -O3 --offload-arch=gfx950 -S):
//   mask_upsample_kernel (and mask_stats_kernel / mask_binarize_kernel, which inline the same up_sample)
//     align_corners=False: s = fma(scale, dst + 0.5, -0.5) in one rounding; align_corners=True: s = scale * dst, l1 = s - i0 on
//     the rounded s; blend X = fma(x.l0, a, x.l1 * b), Y = fma(x.l0, c, x.l1 * d), then y.l0 * X + y.l1 * Y with both products
//     rounded before the add (v_pk_mul_f32, v_pk_fma_f32, v_pk_mul_f32, v_add_f32).
//   bilinear_nchw_kernel (psam_resize2d mode 0): s = fma(scale, dst + 0.5, -0.5); the same blend as mask_upsample_kernel.
//   resize2d_kernel mode 1: i0 = (int)(scale * dst) on the rounded product, but l1 = fma(scale, dst, -i0) in one rounding, no
//     clamp of l1; blend X = fma(x.l1, b, x.l0 * a) - the OTHER product rounded - and Y = fma(x.l0, c, x.l1 * d), then
//     y.l0 * X + y.l1 * Y with both products rounded.
//   nearest (variant 2, mode 2): floor(scale * dst), nothing to fuse.
// All scales are IEEE fp32 divisions. This file spells those operations out with contraction off, so it gives these bits whatever
// its own code shape.
//
// Work distribution: mask_stats_kernel's - one workgroup of 256 lanes takes RS_ROWS output rows of one plane (planes in grid y,
// hence at most 65535 planes per call), a lane owns the columns x = lane, lane + 256, ... and walks down its rows, one set of
// atomics per wave. A lane keeps the first-stage values of its two current source rows in registers: when up-scaling, consecutive
// output rows share them, so a first-stage sample is computed about once instead of four times (the row test is uniform over the
// workgroup). The logits are read from L2 (256 KB per plane).
#include "common.h"
#include "resize_walk.h"   // RsTap, rs_tap*, rs_first, rs_second, rs_walk: the per-pixel code (contraction off)

#define RS_ROWS 32
#define RS_MAX_PLANES 65535

__global__ void rs_stats_init_kernel(int* __restrict__ stats, int planes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= planes * 8) return;
  const int f = i & 7;
  stats[i] = (f == 3 || f == 4) ? 0x7fffffff : ((f == 5 || f == 6) ? -1 : 0);
}

template <int V>
__global__ __launch_bounds__(256) void mask_stats_resized_kernel(const float* __restrict__ low, int C, int first, int nsel, int IN,
                                                                 int MID, int ih, int iw, int OH, int OW, float thr, float off,
                                                                 const float* __restrict__ score, float score_thr,
                                                                 int* __restrict__ stats) {
  const int p = blockIdx.y;
  // a candidate the generator's first filter drops (predicted IoU > threshold as float32, NaN fails) keeps its empty row
  if (score && !(score[(size_t)(p / nsel) * C + first + p % nsel] > score_thr)) return;
  const float* src = low + ((size_t)(p / nsel) * C + first + p % nsel) * IN * IN;
  const int y0 = blockIdx.x * RS_ROWS, y1 = min(y0 + RS_ROWS, OH);
  const float thi = thr + off, tlo = thr - off;
  int hi = 0, lo = 0, ar = 0, mnx = 0x7fffffff, mny = 0x7fffffff, mxx = -1, mxy = -1;
  rs_walk<V>(src, IN, MID, ih, iw, OH, OW, y0, y1, [&](int y, int x, float v) {
    hi += v > thi;
    lo += v > tlo;
    if (v > thr) {
      ++ar;
      mnx = min(mnx, x); mxx = max(mxx, x);
      mny = min(mny, y); mxy = max(mxy, y);
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hi += __shfl_xor(hi, o, 64); lo += __shfl_xor(lo, o, 64); ar += __shfl_xor(ar, o, 64);
    mnx = min(mnx, __shfl_xor(mnx, o, 64)); mny = min(mny, __shfl_xor(mny, o, 64));
    mxx = max(mxx, __shfl_xor(mxx, o, 64)); mxy = max(mxy, __shfl_xor(mxy, o, 64));
  }
  if ((threadIdx.x & 63) == 0 && (lo || ar)) {
    int* s = stats + (size_t)p * 8;
    if (hi) atomicAdd(s + 0, hi);
    if (lo) atomicAdd(s + 1, lo);
    if (ar) {
      atomicAdd(s + 2, ar);
      atomicMin(s + 3, mnx); atomicMin(s + 4, mny); atomicMax(s + 5, mxx); atomicMax(s + 6, mxy);
    }
  }
}

static int rs_stats_launch(const float* low, int B, int C, int first, int nsel, int IN, int MID, int ih, int iw, int OH, int OW,
                           int variant, float thr, float off, const float* score, float score_thr, int* stats, void* stream) {
  if (!low || !stats || B <= 0 || first < 0 || nsel <= 0 || first > C - nsel || variant < 0 || variant > 2 || IN <= 0 || MID <= 0 ||
      ih <= 0 || iw <= 0 || OH <= 0 || OW <= 0 || ih > MID || iw > MID || !(off >= 0.f) ||
      (long long)B * nsel > RS_MAX_PLANES)
    return PSAM_ERR_ARG;
  const int planes = B * nsel;
  hipLaunchKernelGGL(rs_stats_init_kernel, dim3((planes * 8 + 255) / 256), dim3(256), 0, (hipStream_t)stream, stats, planes);
  const dim3 grid((OH + RS_ROWS - 1) / RS_ROWS, planes);
#define RS_LAUNCH(V)                                                                                                             \
  hipLaunchKernelGGL(mask_stats_resized_kernel<V>, grid, dim3(256), 0, (hipStream_t)stream, low, C, first, nsel, IN, MID, ih, iw, \
                     OH, OW, thr, off, score, score_thr, stats)
  if (variant == 0) RS_LAUNCH(0);
  else if (variant == 1) RS_LAUNCH(1);
  else RS_LAUNCH(2);
#undef RS_LAUNCH
  return psam_launch_status();
}
extern "C" int psam_mask_stats_resized(const float* low, int B, int C, int first, int nsel, int IN, int MID, int ih, int iw, int OH,
                                       int OW, int variant, float thr, float off, int* stats, void* stream) {
  return rs_stats_launch(low, B, C, first, nsel, IN, MID, ih, iw, OH, OW, variant, thr, off, nullptr, 0.f, stats, stream);
}
// the same table, computed only for the candidates whose score (fp32 [B, C], the decoder's predicted IoUs, indexed like low's planes)
// passes `score > (float)score_thresh`; every other row holds the empty-mask values. The generator applies that filter first (on the
// host or in psam_amg_select, as the same float32 comparison), so it never reads the rows left out.
extern "C" int psam_mask_stats_resized_scored(const float* low, const float* score, double score_thresh, int B, int C, int first,
                                              int nsel, int IN, int MID, int ih, int iw, int OH, int OW, int variant, float thr,
                                              float off, int* stats, void* stream) {
  if (!score) return PSAM_ERR_ARG;
  return rs_stats_launch(low, B, C, first, nsel, IN, MID, ih, iw, OH, OW, variant, thr, off, score, (float)score_thresh, stats,
                         stream);
}

template <int V>
__global__ __launch_bounds__(256) void mask_binarize_resized_kernel(const float* __restrict__ low, const int* __restrict__ idx,
                                                                    int IN, int MID, int ih, int iw, int OH, int OW, float thr,
                                                                    uint8_t* __restrict__ out, int FH, int FW, int fy0, int fx0,
                                                                    const uint8_t* __restrict__ label,
                                                                    unsigned long long* __restrict__ counts) {
  const int i = blockIdx.y;
  const float* src = low + (size_t)idx[i] * IN * IN;
  uint8_t* frame = out + (size_t)i * FH * FW;
  const int y0 = blockIdx.x * RS_ROWS, y1 = min(y0 + RS_ROWS, OH);
  int tp = 0, fp = 0, fn = 0;
  rs_walk<V>(src, IN, MID, ih, iw, OH, OW, y0, y1, [&](int y, int x, float v) {
    const int m = v > thr;
    const size_t o = (size_t)(fy0 + y) * FW + fx0 + x;
    frame[o] = (uint8_t)m;
    if (label) {
      const int l = label[o] != 0;
      tp += m & l; fp += m & (!l); fn += (!m) & l;
    }
  });
  if (!label) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    tp += __shfl_xor(tp, o, 64); fp += __shfl_xor(fp, o, 64); fn += __shfl_xor(fn, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (tp) atomicAdd(counts + (size_t)i * 3 + 0, (unsigned long long)tp);
    if (fp) atomicAdd(counts + (size_t)i * 3 + 1, (unsigned long long)fp);
    if (fn) atomicAdd(counts + (size_t)i * 3 + 2, (unsigned long long)fn);
  }
}

extern "C" int psam_mask_binarize_resized(const float* low, const int* idx, int n, int IN, int MID, int ih, int iw, int OH, int OW,
                                          int variant, float thr, uint8_t* out, int FH, int FW, int y0, int x0,
                                          const uint8_t* label, long long* counts, void* stream) {
  if (!low || !idx || !out || n <= 0 || n > RS_MAX_PLANES || variant < 0 || variant > 2 || IN <= 0 || MID <= 0 || ih <= 0 ||
      iw <= 0 || OH <= 0 || OW <= 0 || ih > MID || iw > MID || FH <= 0 || FW <= 0 || y0 < 0 || x0 < 0 || OH > FH - y0 ||
      OW > FW - x0 || (label && !counts))
    return PSAM_ERR_ARG;
  if (label) (void)hipMemsetAsync(counts, 0, sizeof(long long) * 3 * n, (hipStream_t)stream);
  const dim3 grid((OH + RS_ROWS - 1) / RS_ROWS, n);
#define RS_LAUNCH(V)                                                                                                              \
  hipLaunchKernelGGL(mask_binarize_resized_kernel<V>, grid, dim3(256), 0, (hipStream_t)stream, low, idx, IN, MID, ih, iw, OH, OW, \
                     thr, out, FH, FW, y0, x0, label, (unsigned long long*)counts)
  if (variant == 0) RS_LAUNCH(0);
  else if (variant == 1) RS_LAUNCH(1);
  else RS_LAUNCH(2);
#undef RS_LAUNCH
  return psam_launch_status();
}
