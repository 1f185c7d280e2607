// Box NMS and the automatic mask generator's candidate selection on the device.
//
// Replaces the host stage of SamAutomaticMaskGenerator._candidates (automatic_mask_generator.py:293-303 score filters, :262-268
// batched_nms; restated in numpy as utils/amg.py nms_xyxy): a download of the statistics table, two numpy filters, a Python loop
// with one round of numpy calls per kept box, and an upload of the surviving plane indices. The contract is that host code,
// bit for bit: exact integer and IEEE fp32 arithmetic in the same order of operations, no tolerance.
//
// Candidates come in G groups (group g = rows offsets[g] .. offsets[g+1] of the inputs), at most NMS_MAX_GROUP per group.
// Per call, ordered by separate launches on one stream (no flags, no waits between workgroups, every loop bounded by the group):
//   1. nms_prep_kernel / amg_prep_kernel: one thread per candidate -> its fp32 box and its 64-bit key; 0 = filtered out
//      (psam_amg_select_crop: also where the box is near a crop edge, is_box_near_crop_edge).
//      key = order-preserving transform of the score's bits << 32 | ~index: all keys of a group differ, larger score first,
//      lower index first among equal scores (argsort(-s, kind="stable"); -0.0 is keyed as +0.0), whatever the scheduling.
//   2. nms_rank_kernel: rank = number of larger keys of the group (tiles of 256 keys through LDS; <= 2^28 comparisons at the
//      capacity) -> boxes and indices in visiting order; the number of live candidates.
//   3. nms_walk_kernel: one workgroup of 1024 threads per group. Thread t keeps the boxes at positions t, t + 1024, ... in
//      registers (16 at the capacity); the removed set is 16384 bits of LDS. Per step, thread 0 finds the next position that is
//      not removed (a removed box is never visited, so it suppresses nothing) and appends it to the kept list while the slot is
//      below `cap`; every thread marks its later positions whose IoU with that box exceeds the threshold. Two barriers per step.
//   4. amg_records_kernel (psam_amg_select): one thread per kept candidate writes its record.
// IoU as nms_xyxy: area = (x1 - x0) * (y1 - y0), iw = max(0, min(x1) - max(x0)), inter = iw * ih, inter / (area_i + area_j -
// inter), every operation a separately rounded fp32 one (this file is compiled with -ffp-contract=off and the two functions carry
// the pragma: no product is contracted into a sum - the header's __fmul_rn is a plain `*` that the caller's setting does not reach;
// crop boxes of an 8192-pixel image have areas beyond 2^24), a correctly rounded division, the quotient widened to double and compared
// `> threshold`: IoU == threshold is kept, 0 / 0 of two empty boxes is NaN and suppresses nothing. Boxes and scores are finite.
#include "common.h"

#define NMS_MAX_GROUP 16384
#define NMS_WALK_THREADS 1024
#define NMS_SLOTS (NMS_MAX_GROUP / NMS_WALK_THREADS)   // boxes a walking thread keeps in registers
#define AMG_REC 9                                       // int32 words of a psam_amg_select record

static_assert(NMS_MAX_GROUP % NMS_WALK_THREADS == 0 && NMS_MAX_GROUP % 32 == 0, "whole slots and whole words of the removed set");

struct NmsScratch {
  unsigned long long* key;   // [G * maxg] 0 = not a candidate
  float4* ubox;              // [G * maxg] boxes in input order
  float4* sbox;              // [G * maxg] boxes in visiting order
  int* sidx;                 // [G * maxg] group-local input index at every visiting position
  int* kept;                 // [G * maxg] psam_amg_select: the kept list before it becomes records
  int* live;                 // [G] candidates the walk visits or suppresses; -1: the group's offsets are unusable
};

static long long nms_scratch_bytes(int G, int maxg) {
  const long long c = (long long)G * maxg;
  return c * (8 + 16 + 16 + 4 + 4) + (((long long)G * 4 + 15) & ~15LL);
}

static NmsScratch nms_carve(void* scratch, int G, int maxg) {
  const size_t c = (size_t)G * maxg;
  NmsScratch s;
  char* p = (char*)scratch;
  s.ubox = (float4*)p; p += c * 16;
  s.sbox = (float4*)p; p += c * 16;
  s.key = (unsigned long long*)p; p += c * 8;
  s.sidx = (int*)p; p += c * 4;
  s.kept = (int*)p; p += c * 4;
  s.live = (int*)p;
  return s;
}

// rows of group g: -> count, or -1 where the offsets are not ascending, leave [0, n] or hold more than maxg rows
__device__ __forceinline__ int nms_group(const int* __restrict__ offsets, int g, int n, int maxg, int* base) {
  const int lo = offsets[g], hi = offsets[g + 1];
  *base = lo;
  if (lo < 0 || hi < lo || hi > n || hi - lo > maxg) return -1;
  return hi - lo;
}

__device__ __forceinline__ unsigned long long nms_key(float score, int i) {
  unsigned u = __float_as_uint(score == 0.f ? 0.f : score);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(~(unsigned)i);
}

__device__ __forceinline__ float nms_area(float4 b) {
#pragma clang fp contract(off)
  return (b.z - b.x) * (b.w - b.y);
}

// nms_xyxy's `iou.astype(float64) > thr` for a kept box a (area aa) against a later box b (area ab)
__device__ __forceinline__ bool nms_over(float4 a, float aa, float4 b, float ab, double thr) {
#pragma clang fp contract(off)
  float iw = fminf(a.z, b.z) - fmaxf(a.x, b.x);
  float ih = fminf(a.w, b.w) - fmaxf(a.y, b.y);
  iw = iw > 0.f ? iw : 0.f;
  ih = ih > 0.f ? ih : 0.f;
  const float inter = iw * ih;
  const float iou = inter / ((aa + ab) - inter);
  return (double)iou > thr;
}

__global__ __launch_bounds__(256) void nms_prep_kernel(const void* __restrict__ boxes, int boxes_fp32, const float* __restrict__ scores,
                                                       const int* __restrict__ offsets, int n, int maxg, NmsScratch s) {
  const int g = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  int base;
  const int m = nms_group(offsets, g, n, maxg, &base);
  if (i >= m) return;
  const size_t c = (size_t)base + i, o = (size_t)g * maxg + i;
  float4 b;
  if (boxes_fp32) {
    b = ((const float4*)boxes)[c];
  } else {
    const int4 v = ((const int4*)boxes)[c];
    b = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
  }
  s.ubox[o] = b;
  s.key[o] = nms_key(scores[c], i);
}

// psam_amg_select_crop: the crop's box and the image's box (XYXY, pixels) of is_box_near_crop_edge; use = 0 for psam_amg_select
struct AmgCrop { int use; int crop[4]; int orig[4]; };

// utils/amg.py:199-206 for integer pixel coordinates: the box, moved by the crop's origin into the image's frame, has an edge
// within 20 pixels of the crop's edge that is not within 20 pixels of the image's edge
__device__ __forceinline__ bool amg_near_crop_edge(const int b[4], const AmgCrop& c) {
  bool near = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long v = (long long)b[k] + c.crop[k & 1];
    const long long dc = v - c.crop[k], di = v - c.orig[k];
    near = near || ((dc < 0 ? -dc : dc) <= 20 && !((di < 0 ? -di : di) <= 20));
  }
  return near;
}

// The two score filters and the box rule of automatic_mask_generator.py:125-133 in front of the same keys. stats int32 [M, 8] as
// psam_mask_stats writes it; iou4 fp32 [M / 3 rounded up, 4]: candidate c's predicted IoU is row c / 3, column 1 + c % 3.
__global__ __launch_bounds__(256) void amg_prep_kernel(const int* __restrict__ stats, const float* __restrict__ iou4,
                                                       const int* __restrict__ offsets, int n, int maxg, int use_iou, float iou_thr,
                                                       int use_stab, float stab_thr, AmgCrop crop, NmsScratch s) {
  const int g = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  int base;
  const int m = nms_group(offsets, g, n, maxg, &base);
  if (i >= m) return;
  const size_t c = (size_t)base + i, o = (size_t)g * maxg + i;
  const int* st = stats + c * 8;
  const float iou = iou4[(c / 3) * 4 + 1 + c % 3];
  const float stab = (float)st[0] / (float)st[1];
  bool ok = true;
  if (use_iou) ok = iou > iou_thr;                // float32 > float32, as numpy compares a float32 array with a Python float
  if (use_stab) ok = ok && stab >= stab_thr;      // NaN (0 / 0) fails
  int bi[4] = {0, 0, 0, 0};                       // empty mask -> [0, 0, 0, 0]
  if (st[2] != 0) { bi[0] = st[3]; bi[1] = st[4]; bi[2] = st[5]; bi[3] = st[6]; }
  if (crop.use) ok = ok && !amg_near_crop_edge(bi, crop);   // :309-311, after the score filters as on the host
  const float4 b = make_float4((float)bi[0], (float)bi[1], (float)bi[2], (float)bi[3]);
  s.ubox[o] = b;
  s.key[o] = ok ? nms_key(iou, i) : 0ull;
}

__global__ __launch_bounds__(256) void nms_rank_kernel(const int* __restrict__ offsets, int n, int maxg, NmsScratch s) {
  __shared__ unsigned long long tile[256];
  const int g = blockIdx.y, t = threadIdx.x, i = blockIdx.x * 256 + t;
  int base;
  const int m = nms_group(offsets, g, n, maxg, &base);
  if (m <= 0) {                                   // (uniform over the workgroup)
    if (i == 0) s.live[g] = m;
    return;
  }
  const size_t o = (size_t)g * maxg;
  const unsigned long long mine = i < m ? s.key[o + i] : 0ull;
  int larger = 0, live = 0;
  for (int lo = 0; lo < m; lo += 256) {           // every thread of the workgroup takes every turn: the barriers are uniform
    tile[t] = lo + t < m ? s.key[o + lo + t] : 0ull;
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < 256; ++j) {
      const unsigned long long k = tile[j];
      larger += k > mine;
      live += k != 0ull;
    }
    __syncthreads();
  }
  if (i == 0) s.live[g] = live;
  if (mine != 0ull) {                             // distinct keys: ranks 0 .. live - 1, each once
    s.sbox[o + larger] = s.ubox[o + i];
    s.sidx[o + larger] = i;
  }
}

__global__ __launch_bounds__(NMS_WALK_THREADS) void nms_walk_kernel(NmsScratch s, int maxg, double thr, int* __restrict__ kept,
                                                                    long long kept_stride, int cap, int* __restrict__ count) {
  __shared__ unsigned removed[NMS_MAX_GROUP / 32];
  __shared__ int next;
  const int g = blockIdx.x, t = threadIdx.x;
  const int live = s.live[g];
  if (live < 0) {                                 // unusable offsets (uniform)
    if (t == 0) count[g] = -1;
    return;
  }
  const int nv = live < maxg ? live : maxg;       // (live <= m <= maxg <= NMS_MAX_GROUP by construction; the clamp guards the LDS)
  const float4* sb = s.sbox + (size_t)g * maxg;
  const int* si = s.sidx + (size_t)g * maxg;
  int* out = kept + (size_t)g * kept_stride;
  for (int w = t; w < NMS_MAX_GROUP / 32; w += NMS_WALK_THREADS) removed[w] = 0u;
  const int slots = (nv + NMS_WALK_THREADS - 1) / NMS_WALK_THREADS;
  float4 b[NMS_SLOTS];
  float ar[NMS_SLOTS];
#pragma unroll
  for (int k = 0; k < NMS_SLOTS; ++k) {
    const int q = k * NMS_WALK_THREADS + t;
    b[k] = q < nv ? sb[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    ar[k] = nms_area(b[k]);
  }
  int p = 0, cnt = 0;
  for (int step = 0; step < nv; ++step) {         // at most one kept box per step
    if (t == 0) {
      int q = p;
      while (q < nv) {                            // the lowest position >= p whose bit is clear: at most nv / 32 + 1 words
        const unsigned w = ~removed[q >> 5] & (0xffffffffu << (q & 31));
        if (w) {
          q = (q & ~31) + __ffs((int)w) - 1;
          break;
        }
        q = (q & ~31) + 32;
      }
      next = q;
    }
    __syncthreads();
    p = next;
    if (p >= nv) break;                           // (uniform: every thread read the same word)
    if (t == 0 && cnt < cap) out[cnt] = si[p];
    ++cnt;
    const float4 bp = sb[p];
    const float ap = nms_area(bp);
#pragma unroll
    for (int k = 0; k < NMS_SLOTS; ++k) {
      if (k < slots) {                            // (uniform)
        const int q = k * NMS_WALK_THREADS + t;
        if (q > p && q < nv && nms_over(bp, ap, b[k], ar[k], thr)) atomicOr(&removed[q >> 5], 1u << (q & 31));
      }
    }
    ++p;
    __syncthreads();
  }
  if (t == 0) count[g] = cnt;
}

// record j of group g = {candidate (row of stats), plane of low.view(-1, 256, 256), predicted IoU bits, stability bits, area,
// x0, y0, x1, y1} of the j-th kept candidate
__global__ __launch_bounds__(256) void amg_records_kernel(const int* __restrict__ stats, const float* __restrict__ iou4,
                                                          const int* __restrict__ offsets, NmsScratch s, int maxg, int cap,
                                                          const int* __restrict__ count, int* __restrict__ records) {
  const int g = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  const int cnt = count[g];
  if (j >= cap || j >= cnt || j >= maxg) return;
  const size_t c = (size_t)offsets[g] + s.kept[(size_t)g * maxg + j];
  const int* st = stats + c * 8;
  const size_t plane = (c / 3) * 4 + 1 + c % 3;
  int* r = records + ((size_t)g * cap + j) * AMG_REC;
  const bool empty = st[2] == 0;
  r[0] = (int)c;
  r[1] = (int)plane;
  r[2] = __float_as_int(iou4[plane]);
  const float stab = (float)st[0] / (float)st[1];
  r[3] = stab != stab ? 0x7fc00000 : __float_as_int(stab);   // 0 / 0 (only with the filter off): one NaN, whatever the divider makes
  r[4] = st[2];
  r[5] = empty ? 0 : st[3];
  r[6] = empty ? 0 : st[4];
  r[7] = empty ? 0 : st[5];
  r[8] = empty ? 0 : st[6];
}

extern "C" int psam_nms_workspace(int G, int max_group, long long* bytes) {
  if (G <= 0 || G > 65535 || max_group < 1 || max_group > NMS_MAX_GROUP || !bytes) return PSAM_ERR_ARG;
  *bytes = nms_scratch_bytes(G, max_group);
  return PSAM_OK;
}

static bool nms_args_ok(int n, int G, int max_group, int cap, const void* scratch, long long scratch_bytes) {
  long long need = 0;
  if (n < 0 || n > 0x7fffffff / 8 || cap <= 0 || !scratch || ((uintptr_t)scratch & 15)) return false;
  return psam_nms_workspace(G, max_group, &need) == PSAM_OK && scratch_bytes >= need;
}

extern "C" int psam_box_nms(const void* boxes, int boxes_fp32, const float* scores, const int* offsets, int n, int G,
                            int max_group, double thr, int* kept, int cap, int* count, void* scratch, long long scratch_bytes,
                            void* stream) {
  if (!nms_args_ok(n, G, max_group, cap, scratch, scratch_bytes) || !offsets || !kept || !count || (n > 0 && (!boxes || !scores)) ||
      ((uintptr_t)boxes & 15) || thr != thr)
    return PSAM_ERR_ARG;
  const int maxg = max_group;
  const NmsScratch s = nms_carve(scratch, G, maxg);
  hipStream_t st = (hipStream_t)stream;
  const dim3 per((unsigned)((maxg + 255) / 256), (unsigned)G);
  hipLaunchKernelGGL(nms_prep_kernel, per, dim3(256), 0, st, boxes, boxes_fp32, scores, offsets, n, maxg, s);
  hipLaunchKernelGGL(nms_rank_kernel, per, dim3(256), 0, st, offsets, n, maxg, s);
  hipLaunchKernelGGL(nms_walk_kernel, dim3((unsigned)G), dim3(NMS_WALK_THREADS), 0, st, s, maxg, thr, kept, (long long)cap, cap, count);
  return psam_launch_status();
}

static int amg_select_launch(const int* stats, const float* iou4, const int* offsets, int n, int G, int max_group,
                             double pred_iou_thresh, double stability_thresh, double nms_thresh, const AmgCrop& crop, int* records,
                             int cap, int* count, void* scratch, long long scratch_bytes, void* stream) {
  if (!nms_args_ok(n, G, max_group, cap, scratch, scratch_bytes) || !offsets || !records || !count || (n > 0 && (!stats || !iou4)) ||
      nms_thresh != nms_thresh || pred_iou_thresh != pred_iou_thresh || stability_thresh != stability_thresh)
    return PSAM_ERR_ARG;
  const int maxg = max_group;
  const NmsScratch s = nms_carve(scratch, G, maxg);
  hipStream_t st = (hipStream_t)stream;
  const dim3 per((unsigned)((maxg + 255) / 256), (unsigned)G);
  const int reach = cap < maxg ? cap : maxg;
  hipLaunchKernelGGL(amg_prep_kernel, per, dim3(256), 0, st, stats, iou4, offsets, n, maxg, pred_iou_thresh > 0.0 ? 1 : 0,
                     (float)pred_iou_thresh, stability_thresh > 0.0 ? 1 : 0, (float)stability_thresh, crop, s);
  hipLaunchKernelGGL(nms_rank_kernel, per, dim3(256), 0, st, offsets, n, maxg, s);
  hipLaunchKernelGGL(nms_walk_kernel, dim3((unsigned)G), dim3(NMS_WALK_THREADS), 0, st, s, maxg, nms_thresh, s.kept, (long long)maxg,
                     maxg, count);
  hipLaunchKernelGGL(amg_records_kernel, dim3((unsigned)((reach + 255) / 256), (unsigned)G), dim3(256), 0, st, stats, iou4, offsets, s,
                     maxg, cap, count, records);
  return psam_launch_status();
}

extern "C" int psam_amg_select(const int* stats, const float* iou4, const int* offsets, int n, int G, int max_group,
                               double pred_iou_thresh, double stability_thresh, double nms_thresh, int* records, int cap,
                               int* count, void* scratch, long long scratch_bytes, void* stream) {
  AmgCrop crop = {};
  return amg_select_launch(stats, iou4, offsets, n, G, max_group, pred_iou_thresh, stability_thresh, nms_thresh, crop, records, cap,
                           count, scratch, scratch_bytes, stream);
}

// psam_amg_select for the candidates of a crop: one more condition in the prep kernel, a candidate whose box is near a crop edge
// (amg_near_crop_edge) gets key 0. crop_box / orig_box: HOST int[4], XYXY; the boxes of the records stay in the crop's frame.
extern "C" int psam_amg_select_crop(const int* stats, const float* iou4, const int* offsets, int n, int G, int max_group,
                                    double pred_iou_thresh, double stability_thresh, double nms_thresh, const int* crop_box,
                                    const int* orig_box, int* records, int cap, int* count, void* scratch, long long scratch_bytes,
                                    void* stream) {
  if (!crop_box || !orig_box) return PSAM_ERR_ARG;
  AmgCrop crop;
  crop.use = 1;
  for (int k = 0; k < 4; ++k) {
    crop.crop[k] = crop_box[k];
    crop.orig[k] = orig_box[k];
  }
  return amg_select_launch(stats, iou4, offsets, n, G, max_group, pred_iou_thresh, stability_thresh, nms_thresh, crop, records, cap,
                           count, scratch, scratch_bytes, stream);
}
