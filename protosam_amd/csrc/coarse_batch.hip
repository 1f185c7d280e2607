// Batched post-processing of ProtoMedSAM (many slices x many classes per call): HBM-bound, one launch per stage.
//
//  psam_prob2_argmax   : P planes of 2-class scores [P,2,IH,IW] -> [bilinear to (OH,OW)] -> softmax -> argmax (uint8) and
//                        foreground count per plane -> softmax of the probabilities again, foreground channel only
//                        (models/ProtoMedSAM.py:176-187; util/utils.py:474-494, the second softmax at :485). What
//                        psam_prob_argmax twice wrote as two [2,OH,OW] fp32 planes plus a second uint8 plane (26 MB per
//                        1024^2 plane) is 5 MB here: the uint8 labels and the one fp32 plane psam_ccl_batch reads.
//  psam_scores_prob_argmax : the same for ProtoSAM (models/ProtoSAM.py:592-602), which needs both softmax channels: P planes
//                        of grid-resolution class scores [P,2,g,g] -> bilinear to the image size (IH,IW) (FewShotSeg.forward,
//                        models/grid_proto_fewshot.py:272-273) -> bilinear to (OH,OW) -> softmax -> argmax. The [P,2,IH,IW]
//                        intermediate is never written: each output pixel recomputes its four image-size samples from the
//                        grid, with psam_bilinear_nchw's arithmetic, so prob / pred / fg_sum are the bits of psam_bilinear_nchw
//                        followed by psam_prob_argmax.
//  psam_mask_union_seg : every output mask of a batch of decoder calls in one launch: out[seg.o] = OR over the segment's
//                        prompts of (up-sample -> > thr), nearest-resized MID -> OUT, as uint8 (models/ProtoMedSAM.py:49-60,
//                        :219-220). Per segment the same bits as psam_mask_union + .to(torch.uint8).
//
// Both kernels: 256 lanes, 4 consecutive pixels of one row per lane (16-byte fp32 / 4-byte uint8 stores), one work item = one
// 1024-pixel chunk of one row of one plane; at most PB_MAX_BLOCKS workgroups, each walking a contiguous run of items (so the
// foreground count of a plane is flushed with one atomic per workgroup and plane). No allocation, no synchronisation.
#include "common.h"
#include "interp.h"

#define PB_ROW 1024          // pixels per work item (256 lanes x 4)
#define PB_MAX_BLOCKS 2048   // 256 CUs x 8 workgroups

static inline int pb_grid(long long items, int* per_block) {
  const long long g = items < PB_MAX_BLOCKS ? items : PB_MAX_BLOCKS;
  const long long per = (items + g - 1) / g;
  *per_block = (int)per;
  return (int)((items + per - 1) / per);
}

// sum of `v` over the workgroup, added to *dst by one lane (all 256 lanes must call it)
__device__ __forceinline__ void pb_flush(int v, int* __restrict__ dst, int* wsum) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (t) atomicAdd(dst, t);
  }
  __syncthreads();   // wsum is reused by the next flush
}

// The per-pixel arithmetic is prob_argmax_kernel's (resample.hip), applied twice: the first time to the (resampled) scores, the
// second time to the probabilities on its same-size path. Same expressions, same order: the same bits.
__global__ __launch_bounds__(256) void prob2_argmax_kernel(const float* __restrict__ scores, int P, int IH, int IW, int OH,
                                                           int OW, int per_block, int vec, uint8_t* __restrict__ pred,
                                                           float* __restrict__ pfg2, float* __restrict__ prob,
                                                           int* __restrict__ fg_sum) {
  __shared__ int wsum[4];
  const int nch = (OW + PB_ROW - 1) / PB_ROW;
  const long long per_plane = (long long)OH * nch;
  const long long total = per_plane * P;
  long long i = (long long)blockIdx.x * per_block;
  const long long iend = min(i + (long long)per_block, total);
  if (i >= iend) return;                                    // (uniform over the workgroup)
  const bool same = (IH == OH && IW == OW);
  const float sh = (float)IH / (float)OH, sw = (float)IW / (float)OW;
  const size_t plane = (size_t)OH * OW;
  int cur = (int)(i / per_plane), fgc = 0;
  for (; i < iend; ++i) {
    const int p = (int)(i / per_plane);
    if (p != cur) {
      if (fg_sum) pb_flush(fgc, fg_sum + cur, wsum);
      fgc = 0;
      cur = p;
    }
    const int rem = (int)(i - (long long)p * per_plane);
    const int y = rem / nch;
    const int x0 = (rem % nch) * PB_ROW + threadIdx.x * 4;
    if (x0 >= OW) continue;
    const float* l0p = scores + ((size_t)p * 2 + 0) * IH * IW;
    const float* l1p = l0p + (size_t)IH * IW;
    Lin ly = lin_src(y, sh, IH);
    float p0v[4], p1v[4], q1v[4];
    uint8_t fgv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = min(x0 + k, OW - 1);
      float l0, l1;
      if (same) {
        l0 = l0p[(size_t)y * IW + x];
        l1 = l1p[(size_t)y * IW + x];
      } else {
        Lin lx = lin_src(x, sw, IW);
        l0 = bilerp(l0p, IW, ly, lx);
        l1 = bilerp(l1p, IW, ly, lx);
      }
      const float m = fmaxf(l0, l1);
      const float e0 = expf(l0 - m), e1 = expf(l1 - m);
      const float s = e0 + e1;
      p0v[k] = e0 / s;
      p1v[k] = e1 / s;
      fgv[k] = p1v[k] > p0v[k] ? 1 : 0;  // argmax returns the first maximum on ties
      if (x0 + k < OW) fgc += fgv[k];
      // get_connected_components re-applies softmax to the probabilities (util/utils.py:485)
      const float m2 = fmaxf(p0v[k], p1v[k]);
      const float f0 = expf(p0v[k] - m2), f1 = expf(p1v[k] - m2);
      const float s2 = f0 + f1;
      q1v[k] = f1 / s2;
    }
    const size_t o = (size_t)p * plane + (size_t)y * OW + x0;
    if (vec && x0 + 3 < OW) {
      *reinterpret_cast<uchar4*>(pred + o) = make_uchar4(fgv[0], fgv[1], fgv[2], fgv[3]);
      *reinterpret_cast<float4*>(pfg2 + o) = make_float4(q1v[0], q1v[1], q1v[2], q1v[3]);
      if (prob) {
        const size_t o2 = (size_t)p * 2 * plane + (size_t)y * OW + x0;
        *reinterpret_cast<float4*>(prob + o2) = make_float4(p0v[0], p0v[1], p0v[2], p0v[3]);
        *reinterpret_cast<float4*>(prob + o2 + plane) = make_float4(p1v[0], p1v[1], p1v[2], p1v[3]);
      }
    } else {
      for (int k = 0; k < 4 && x0 + k < OW; ++k) {
        pred[o + k] = fgv[k];
        pfg2[o + k] = q1v[k];
        if (prob) {
          const size_t o2 = (size_t)p * 2 * plane + (size_t)y * OW + x0 + k;
          prob[o2] = p0v[k];
          prob[o2 + plane] = p1v[k];
        }
      }
    }
  }
  if (fg_sum) pb_flush(fgc, fg_sum + cur, wsum);
}

extern "C" int psam_prob2_argmax(const float* scores, int P, int IH, int IW, int OH, int OW, void* pred, float* pfg2,
                                 int* fg_sum, float* prob, void* stream) {
  if (P <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0 || !scores || !pred || !pfg2) return PSAM_ERR_ARG;
  const long long items = (long long)P * OH * ((OW + PB_ROW - 1) / PB_ROW);
  int per_block = 0;
  const int grid = pb_grid(items, &per_block);
  // 16-byte fp32 / 4-byte uint8 stores need every row start aligned: OW % 4 == 0 and aligned bases
  const int vec = (OW % 4 == 0) && ((uintptr_t)pred % 4 == 0) && ((uintptr_t)pfg2 % 16 == 0) && ((uintptr_t)prob % 16 == 0);
  hipLaunchKernelGGL(prob2_argmax_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, scores, P, IH, IW, OH, OW, per_block,
                     vec, (uint8_t*)pred, pfg2, prob, fg_sum);
  return psam_launch_status();
}

// bilerp's expression as the two kernels this one replaces were compiled (fp-contract=fast lets the compiler choose which products
// to fuse, and it chose differently for each): both fuse x.l0 * a into x.l1 * b; bilinear_nchw_kernel then rounds both row terms
// (y.l0 * X + y.l1 * Y), prob_argmax_kernel fuses y.l0 * X into y.l1 * Y. Spelled out here with contraction off, so that this
// kernel gives their bits whatever its own code shape.
__device__ __forceinline__ float pb_lerp_nchw(const Lin& y, const Lin& x, float a, float b, float c, float d) {
#pragma clang fp contract(off)
  const float X = fmaf(x.l0, a, x.l1 * b), Y = fmaf(x.l0, c, x.l1 * d);
  return y.l0 * X + y.l1 * Y;
}
__device__ __forceinline__ float pb_lerp_prob(const Lin& y, const Lin& x, float a, float b, float c, float d) {
#pragma clang fp contract(off)
  const float X = fmaf(x.l0, a, x.l1 * b), Y = fmaf(x.l0, c, x.l1 * d);
  return fmaf(y.l0, X, y.l1 * Y);
}

// psam_bilinear_nchw's value at (y, x) of the (IH, IW) resize of the g x g plane `gp`: lin_src rows / columns, its blend
__device__ __forceinline__ float pb_grid_sample(const float* __restrict__ gp, int GH, int GW, float gsh, float gsw, int y, int x) {
  const Lin ly = lin_src(y, gsh, GH), lx = lin_src(x, gsw, GW);
  const float* r0 = gp + (size_t)ly.i0 * GW;
  const float* r1 = gp + (size_t)ly.i1 * GW;
  return pb_lerp_nchw(ly, lx, r0[lx.i0], r0[lx.i1], r1[lx.i0], r1[lx.i1]);
}

// prob_argmax_kernel's per-pixel arithmetic (resample.hip) on logits that bilinear_nchw_kernel would have produced: the same
// operations in the same order, the image-size samples computed instead of loaded.
__global__ __launch_bounds__(256) void scores_prob_argmax_kernel(const float* __restrict__ scores, int P, int GH, int GW, int IH,
                                                                 int IW, int OH, int OW, int per_block, int vec,
                                                                 float* __restrict__ prob, uint8_t* __restrict__ pred,
                                                                 int* __restrict__ fg_sum) {
  __shared__ int wsum[4];
  const int nch = (OW + PB_ROW - 1) / PB_ROW;
  const long long per_plane = (long long)OH * nch;
  const long long total = per_plane * P;
  long long i = (long long)blockIdx.x * per_block;
  const long long iend = min(i + (long long)per_block, total);
  if (i >= iend) return;                                    // (uniform over the workgroup)
  const bool same = (IH == OH && IW == OW);
  const float gsh = (float)GH / (float)IH, gsw = (float)GW / (float)IW;   // psam_bilinear_nchw: grid -> image size
  const float sh = (float)IH / (float)OH, sw = (float)IW / (float)OW;     // psam_prob_argmax: image size -> output
  const size_t plane = (size_t)OH * OW;
  int cur = (int)(i / per_plane), fgc = 0;
  for (; i < iend; ++i) {
    const int p = (int)(i / per_plane);
    if (p != cur) {
      if (fg_sum) pb_flush(fgc, fg_sum + cur, wsum);
      fgc = 0;
      cur = p;
    }
    const int rem = (int)(i - (long long)p * per_plane);
    const int y = rem / nch;
    const int x0 = (rem % nch) * PB_ROW + threadIdx.x * 4;
    if (x0 >= OW) continue;
    const float* g0p = scores + ((size_t)p * 2 + 0) * GH * GW;
    const float* g1p = g0p + (size_t)GH * GW;
    Lin ly = lin_src(y, sh, IH);
    float p0v[4], p1v[4];
    uint8_t fgv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = min(x0 + k, OW - 1);
      float l0, l1;
      if (same) {
        l0 = pb_grid_sample(g0p, GH, GW, gsh, gsw, y, x);
        l1 = pb_grid_sample(g1p, GH, GW, gsh, gsw, y, x);
      } else {
        Lin lx = lin_src(x, sw, IW);
        l0 = pb_lerp_prob(ly, lx, pb_grid_sample(g0p, GH, GW, gsh, gsw, ly.i0, lx.i0), pb_grid_sample(g0p, GH, GW, gsh, gsw, ly.i0, lx.i1),
                    pb_grid_sample(g0p, GH, GW, gsh, gsw, ly.i1, lx.i0), pb_grid_sample(g0p, GH, GW, gsh, gsw, ly.i1, lx.i1));
        l1 = pb_lerp_prob(ly, lx, pb_grid_sample(g1p, GH, GW, gsh, gsw, ly.i0, lx.i0), pb_grid_sample(g1p, GH, GW, gsh, gsw, ly.i0, lx.i1),
                    pb_grid_sample(g1p, GH, GW, gsh, gsw, ly.i1, lx.i0), pb_grid_sample(g1p, GH, GW, gsh, gsw, ly.i1, lx.i1));
      }
      const float m = fmaxf(l0, l1);
      const float e0 = expf(l0 - m), e1 = expf(l1 - m);
      const float s = e0 + e1;
      p0v[k] = e0 / s;
      p1v[k] = e1 / s;
      fgv[k] = p1v[k] > p0v[k] ? 1 : 0;  // argmax returns the first maximum on ties
      if (x0 + k < OW) fgc += fgv[k];
    }
    const size_t o = (size_t)p * plane + (size_t)y * OW + x0;
    const size_t o2 = (size_t)p * 2 * plane + (size_t)y * OW + x0;
    if (vec && x0 + 3 < OW) {
      *reinterpret_cast<float4*>(prob + o2) = make_float4(p0v[0], p0v[1], p0v[2], p0v[3]);
      *reinterpret_cast<float4*>(prob + o2 + plane) = make_float4(p1v[0], p1v[1], p1v[2], p1v[3]);
      *reinterpret_cast<uchar4*>(pred + o) = make_uchar4(fgv[0], fgv[1], fgv[2], fgv[3]);
    } else {
      for (int k = 0; k < 4 && x0 + k < OW; ++k) {
        prob[o2 + k] = p0v[k];
        prob[o2 + k + plane] = p1v[k];
        pred[o + k] = fgv[k];
      }
    }
  }
  if (fg_sum) pb_flush(fgc, fg_sum + cur, wsum);
}

extern "C" int psam_scores_prob_argmax(const float* scores, int P, int GH, int GW, int IH, int IW, int OH, int OW, float* prob,
                                       void* pred, int* fg_sum, void* stream) {
  if (P <= 0 || GH <= 0 || GW <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0 || !scores || !prob || !pred) return PSAM_ERR_ARG;
  const long long items = (long long)P * OH * ((OW + PB_ROW - 1) / PB_ROW);
  int per_block = 0;
  const int grid = pb_grid(items, &per_block);
  const int vec = (OW % 4 == 0) && ((uintptr_t)pred % 4 == 0) && ((uintptr_t)prob % 16 == 0);
  hipLaunchKernelGGL(scores_prob_argmax_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, scores, P, GH, GW, IH, IW, OH, OW,
                     per_block, vec, prob, (uint8_t*)pred, fg_sum);
  return psam_launch_status();
}

// out[seg.o, y, x] (uint8 {0,1}) = OR_{b in [seg.first, seg.first + seg.count)} ( up_sample(low[b, sel])[ny(y), nx(x)] > thr ),
// mask_union_kernel's arithmetic (decoder.hip) per segment. A row of `segs` that points outside low or out is skipped.
__global__ __launch_bounds__(256) void mask_union_seg_kernel(const float* __restrict__ low, int Pm, int C, int sel, int IN,
                                                             const int* __restrict__ segs, int nseg, int nout, int MID, int OUT,
                                                             int variant, float thr, int per_block, int vec,
                                                             uint8_t* __restrict__ out) {
  const int nch = (OUT + PB_ROW - 1) / PB_ROW;
  const long long per_seg = (long long)OUT * nch;
  const long long total = per_seg * nseg;
  long long i = (long long)blockIdx.x * per_block;
  const long long iend = min(i + (long long)per_block, total);
  const float sc = (float)MID / (float)OUT;
  for (; i < iend; ++i) {
    const int s = (int)(i / per_seg);
    const int first = segs[3 * s + 0], count = segs[3 * s + 1], o = segs[3 * s + 2];
    if (first < 0 || count < 0 || first > Pm - count || o < 0 || o >= nout) continue;
    const int rem = (int)(i - (long long)s * per_seg);
    const int y = rem / nch;
    const int x0 = (rem % nch) * PB_ROW + threadIdx.x * 4;
    if (x0 >= OUT) continue;
    int sy = (int)floorf((float)y * sc);
    sy = sy < MID - 1 ? sy : MID - 1;
    uint8_t m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = min(x0 + k, OUT - 1);
      int sx = (int)floorf((float)x * sc);
      sx = sx < MID - 1 ? sx : MID - 1;
      int any = 0;
      for (int b = first; b < first + count; ++b) {
        const float v = up_sample(low + ((size_t)b * C + sel) * IN * IN, IN, MID, sy, sx, variant);
        any |= (v > thr);
      }
      m[k] = any ? 1 : 0;
    }
    uint8_t* dst = out + ((size_t)o * OUT + y) * OUT + x0;
    if (vec && x0 + 3 < OUT) {
      *reinterpret_cast<uchar4*>(dst) = make_uchar4(m[0], m[1], m[2], m[3]);
    } else {
      for (int k = 0; k < 4 && x0 + k < OUT; ++k) dst[k] = m[k];
    }
  }
}

extern "C" int psam_mask_union_seg(const float* low, int Pm, int C, int sel, int IN, const int* segs, int nseg, int nout,
                                   int MID, int OUT, int variant, float thr, void* out, void* stream) {
  if (Pm < 0 || C <= 0 || sel < 0 || sel >= C || IN <= 0 || nseg <= 0 || nout <= 0 || MID <= 0 || OUT <= 0 || variant < 0 ||
      variant > 3 || !segs || !out || (Pm > 0 && !low))
    return PSAM_ERR_ARG;
  const long long items = (long long)nseg * OUT * ((OUT + PB_ROW - 1) / PB_ROW);
  int per_block = 0;
  const int grid = pb_grid(items, &per_block);
  const int vec = (OUT % 4 == 0) && ((uintptr_t)out % 4 == 0);
  hipLaunchKernelGGL(mask_union_seg_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, low, Pm, C, sel, IN, segs, nseg, nout,
                     MID, OUT, variant, thr, per_block, vec, (uint8_t*)out);
  return psam_launch_status();
}
