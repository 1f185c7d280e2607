// The automatic mask generator's crop layers on the device (automatic_mask_generator.py:194-262): what lies between a crop's own
// selection (psam_amg_select_crop) and the final records of the image, without the host in between.
//
//  psam_amg_keep_planes     : after a crop's selection - the crop's kept records join the image's merged table, translated into the
//                             image's frame, and their 256 x 256 logit planes are copied into the image's plane pool (the decoder's
//                             output buffer is overwritten by the next crop)
//  psam_amg_crops_nms       : cross-crop NMS over the merged table (:208-218: score = 1 / crop area, smaller crops first), whose
//                             length is a device count -> the final records in suppression order and their count in one tensor
//  psam_mask_binarize_crops : the final records' masks in frames of the original image, every record with the geometry of its own
//                             crop, zero outside the crop (uncrop_masks) - the bits of psam_mask_binarize_resized at that origin
//
// Tables (int32, device memory):
//   merged [pool_cap, AMG_CREC]: a psam_amg_select record {candidate, plane of the decoder's output, predicted IoU bits, stability
//          bits, area, x0, y0, x1, y1} with the box in the IMAGE's frame, then {crop index, row of the pool}.
//   bases  [ncrops + 1]: bases[c] = records of the crops before c = the first pool row of crop c. Crop c's call reads bases[c] (0 for
//          c = 0) and writes bases[c + 1]: the calls of an image are ordered by the stream, so this counter needs no atomic and no
//          clearing. It counts on past pool_cap; rows >= pool_cap are written nowhere, and bases[ncrops] > pool_cap is the overflow
//          that psam_amg_crops_nms reports.
//   geom   [ncrops, AMG_GEOM]: {x0, y0, crop width, crop height, ih, iw (predictor.input_size of the crop), bits of the float32 NMS
//          score 1 / crop area, 0}.
// All three are index kernels bound by memory traffic or launch latency: the plane copy moves 256 KB per record in 16-byte accesses
// that are contiguous over the workgroup; a launch is sized for the capacity and the workgroups past the device count leave at once.
// The NMS itself is psam_box_nms (csrc/nms.hip), which reads its group's offsets from device memory: the rule and the tie order
// are its own.
#include "resize_walk.h"

#define AMG_REC 9          // int32 words of a psam_amg_select record (csrc/nms.hip)
#define AMG_CREC 11        // ... of a merged / final record
#define AMG_GEOM 8         // ... of a row of the crop geometry table
#define NMS_MAX_GROUP 16384
#define KP_SPLIT 4         // workgroups that share one plane copy
#define RS_ROWS 32

extern "C" int psam_nms_workspace(int G, int max_group, long long* bytes);
extern "C" int psam_box_nms(const void* boxes, int boxes_fp32, const float* scores, const int* offsets, int n, int G, int max_group,
                            double thr, int* kept, int cap, int* count, void* scratch, long long scratch_bytes, void* stream);

// grid (cap, KP_SPLIT): workgroup (j, part) copies quarter `part` of the plane of the crop's record j; part 0 writes the merged record
__global__ __launch_bounds__(256) void amg_keep_planes_kernel(const float* __restrict__ low, int low_planes, int plane_elems,
                                                              const int* __restrict__ records, const int* __restrict__ count, int cap,
                                                              int crop, int x0, int y0, float* __restrict__ pool, int pool_cap,
                                                              int* __restrict__ merged, int* __restrict__ bases) {
  const int j = blockIdx.x, part = blockIdx.y, t = threadIdx.x;
  int k = count[0];
  k = k < 0 ? 0 : (k > cap ? cap : k);           // count may exceed cap: only the first cap records were stored
  const int base = crop == 0 ? 0 : bases[crop];
  if (j == 0 && part == 0 && t == 0) {           // (before the early exit: a crop without records still hands the counter on)
    if (crop == 0) bases[0] = 0;
    bases[crop + 1] = base + k;
  }
  if (j >= k) return;
  const long long row = (long long)base + j;
  if (base < 0 || row >= pool_cap) return;       // pool overflow: nothing is written, bases[] carries the report
  const int* r = records + (size_t)j * AMG_REC;
  if (part == 0 && t < AMG_CREC) {
    int v;
    if (t < AMG_REC) v = r[t] + (t >= 5 ? ((t & 1) ? x0 : y0) : 0);   // words 5, 7 are x, words 6, 8 are y
    else v = t == AMG_REC ? crop : (int)row;
    merged[(size_t)row * AMG_CREC + t] = v;
  }
  const int plane = r[1];
  if (plane < 0 || plane >= low_planes) return;  // (a record table that this library wrote never has one)
  const float4* src = (const float4*)(low + (size_t)plane * plane_elems);
  float4* dst = (float4*)(pool + (size_t)row * plane_elems);
  for (int i = part * 256 + t; i < plane_elems / 4; i += 256 * KP_SPLIT) dst[i] = src[i];
}

extern "C" int psam_amg_keep_planes(const float* low, int low_planes, int IN, const int* records, const int* count, int cap, int crop,
                                    int ncrops, int x0, int y0, float* pool, int pool_cap, int* merged, int* bases, void* stream) {
  if (!low || !records || !count || !pool || !merged || !bases || low_planes <= 0 || IN <= 0 || IN > 4096 || (IN * IN) % 4 != 0 ||
      cap <= 0 || crop < 0 || ncrops <= 0 || crop >= ncrops || x0 < 0 || y0 < 0 || pool_cap <= 0 || pool_cap > NMS_MAX_GROUP ||
      ((uintptr_t)low & 15) || ((uintptr_t)pool & 15))
    return PSAM_ERR_ARG;
  hipLaunchKernelGGL(amg_keep_planes_kernel, dim3((unsigned)cap, KP_SPLIT), dim3(256), 0, (hipStream_t)stream, low, low_planes, IN * IN,
                     records, count, cap, crop, x0, y0, pool, pool_cap, merged, bases);
  return psam_launch_status();
}

// ---- cross-crop NMS -------------------------------------------------------------------------------------------------------------
struct CropsScratch {
  int4* boxes;      // [pool_cap] the merged boxes
  float* scores;    // [pool_cap] 1 / crop area of every merged record
  int* kept;        // [pool_cap] merged rows in final order
  int* offsets;     // [2] the one group of psam_box_nms: {0, merged records}
  int* count;       // [1] final records
  void* nms;        // psam_box_nms' own scratch
};

static long long crops_head_bytes(int pool_cap) { return (long long)pool_cap * (16 + 4 + 4) + 16; }

static CropsScratch crops_carve(void* scratch, int pool_cap) {
  CropsScratch s;
  char* p = (char*)scratch;
  s.boxes = (int4*)p; p += (size_t)pool_cap * 16;
  s.scores = (float*)p; p += (size_t)pool_cap * 4;
  s.kept = (int*)p; p += (size_t)pool_cap * 4;
  s.offsets = (int*)p;
  s.count = s.offsets + 2;
  p += 16;
  s.nms = (void*)(((uintptr_t)p + 15) & ~(uintptr_t)15);
  return s;
}

extern "C" int psam_amg_crops_workspace(int pool_cap, long long* bytes) {
  long long nms = 0;
  if (!bytes || pool_cap <= 0 || pool_cap > NMS_MAX_GROUP || psam_nms_workspace(1, pool_cap, &nms) != PSAM_OK) return PSAM_ERR_ARG;
  *bytes = crops_head_bytes(pool_cap) + 16 + nms;
  return PSAM_OK;
}

// one thread per pool row: the NMS inputs of the merged records; without NMS (a single crop box) the final order is the merged one
__global__ __launch_bounds__(256) void amg_crops_prep_kernel(const int* __restrict__ merged, const int* __restrict__ bases, int ncrops,
                                                             const int* __restrict__ geom, int pool_cap, int use_nms, CropsScratch s) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int total = bases[ncrops];
  const int n = (total < 0 || total > pool_cap) ? 0 : total;      // overflow: an empty group, reported by the gather kernel
  if (i == 0) {
    s.offsets[0] = 0;
    s.offsets[1] = n;
    if (!use_nms) s.count[0] = n;
  }
  if (i >= n) return;
  const int* r = merged + (size_t)i * AMG_CREC;
  s.boxes[i] = make_int4(r[5], r[6], r[7], r[8]);
  const int c = r[AMG_REC];
  s.scores[i] = (c >= 0 && c < ncrops) ? __int_as_float(geom[(size_t)c * AMG_GEOM + 6]) : 0.f;
  if (!use_nms) s.kept[i] = i;
}

// out [pool_cap * AMG_CREC + 2]: final record j = merged record kept[j]; then the count (-1: pool overflow) and the merged total
__global__ __launch_bounds__(256) void amg_crops_gather_kernel(const int* __restrict__ merged, const int* __restrict__ bases, int ncrops,
                                                               int pool_cap, CropsScratch s, int* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int total = bases[ncrops];
  const bool over = total < 0 || total > pool_cap;
  int m = s.count[0];
  m = m < 0 ? 0 : (m > pool_cap ? pool_cap : m);
  if (i == 0) {
    out[(size_t)pool_cap * AMG_CREC] = over ? -1 : m;
    out[(size_t)pool_cap * AMG_CREC + 1] = total;
  }
  if (over || i >= m * AMG_CREC) return;
  const int j = i / AMG_CREC, w = i - j * AMG_CREC;
  const int src = s.kept[j];
  out[i] = (src >= 0 && src < pool_cap) ? merged[(size_t)src * AMG_CREC + w] : 0;
}

extern "C" int psam_amg_crops_nms(const int* merged, const int* bases, int ncrops, const int* geom, int pool_cap, double thr,
                                  int use_nms, int* out, void* scratch, long long scratch_bytes, void* stream) {
  long long need = 0;
  if (!merged || !bases || !geom || !out || !scratch || ((uintptr_t)scratch & 15) || ncrops <= 0 || thr != thr ||
      psam_amg_crops_workspace(pool_cap, &need) != PSAM_OK || scratch_bytes < need)
    return PSAM_ERR_ARG;
  const CropsScratch s = crops_carve(scratch, pool_cap);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(amg_crops_prep_kernel, dim3((unsigned)((pool_cap + 255) / 256)), dim3(256), 0, st, merged, bases, ncrops, geom,
                     pool_cap, use_nms ? 1 : 0, s);
  if (use_nms) {
    const long long nms_bytes = scratch_bytes - (long long)((char*)s.nms - (char*)scratch);
    const int rc = psam_box_nms(s.boxes, 0, s.scores, s.offsets, pool_cap, 1, pool_cap, thr, s.kept, pool_cap, s.count, s.nms, nms_bytes,
                                stream);
    if (rc != PSAM_OK) return rc;
  }
  hipLaunchKernelGGL(amg_crops_gather_kernel, dim3((unsigned)((pool_cap * AMG_CREC + 255) / 256)), dim3(256), 0, st, merged, bases, ncrops,
                     pool_cap, s, out);
  return psam_launch_status();
}

// ---- the final records' masks ---------------------------------------------------------------------------------------------------
// grid (ceil(H / RS_ROWS), m): workgroup (b, i) writes rows [b * RS_ROWS, ...) of frame i - zero outside the rectangle of record i's
// crop, and inside it the two-stage value of the record's pool plane > thr (rs_walk over the rows of the crop that fall into the band)
template <int V>
__global__ __launch_bounds__(256) void mask_binarize_crops_kernel(const float* __restrict__ pool, int pool_cap,
                                                                  const int* __restrict__ final_records, const int* __restrict__ geom,
                                                                  int ncrops, int IN, int MID, float thr, uint8_t* __restrict__ out,
                                                                  int H, int W) {
  const int i = blockIdx.y;
  const int* r = final_records + (size_t)i * AMG_CREC;
  const int crop = r[AMG_REC], row = r[AMG_REC + 1];
  uint8_t* frame = out + (size_t)i * H * W;
  const int Y0 = blockIdx.x * RS_ROWS, Y1 = min(Y0 + RS_ROWS, H);
  int x0 = 0, y0 = 0, cw = 0, ch = 0, ih = 1, iw = 1;
  if (crop >= 0 && crop < ncrops && row >= 0 && row < pool_cap) {
    const int* g = geom + (size_t)crop * AMG_GEOM;
    x0 = g[0]; y0 = g[1]; cw = g[2]; ch = g[3]; ih = g[4]; iw = g[5];
    // a rectangle that leaves the frame, or a source size outside the first-stage map, would read or write out of bounds: an empty one
    if (x0 < 0 || y0 < 0 || cw <= 0 || ch <= 0 || cw > W - x0 || ch > H - y0 || ih <= 0 || iw <= 0 || ih > MID || iw > MID) cw = ch = 0;
  }
  for (int y = Y0; y < Y1; ++y) {
    const bool in_rows = y >= y0 && y < y0 + ch;
    uint8_t* line = frame + (size_t)y * W;
    for (int x = threadIdx.x; x < W; x += 256)
      if (!(in_rows && x >= x0 && x < x0 + cw)) line[x] = 0;
  }
  const int a = max(Y0, y0) - y0, b = min(Y1, y0 + ch) - y0;      // rows of the crop inside this band
  if (cw <= 0 || a >= b) return;
  const float* src = pool + (size_t)row * IN * IN;
  rs_walk<V>(src, IN, MID, ih, iw, ch, cw, a, b, [&](int y, int x, float v) {
    frame[(size_t)(y0 + y) * W + x0 + x] = (uint8_t)(v > thr);
  });
}

extern "C" int psam_mask_binarize_crops(const float* pool, int pool_cap, const int* final_records, int m, const int* geom, int ncrops,
                                        int IN, int MID, int variant, float thr, unsigned char* out, int H, int W, void* stream) {
  if (!pool || !final_records || !geom || !out || pool_cap <= 0 || pool_cap > NMS_MAX_GROUP || m <= 0 || m > pool_cap || ncrops <= 0 ||
      IN <= 0 || MID <= 0 || variant < 0 || variant > 2 || H <= 0 || W <= 0)
    return PSAM_ERR_ARG;
  const dim3 grid((unsigned)((H + RS_ROWS - 1) / RS_ROWS), (unsigned)m);
#define CR_LAUNCH(V)                                                                                                          \
  hipLaunchKernelGGL(mask_binarize_crops_kernel<V>, grid, dim3(256), 0, (hipStream_t)stream, pool, pool_cap, final_records, geom, \
                     ncrops, IN, MID, thr, out, H, W)
  if (variant == 0) CR_LAUNCH(0);
  else if (variant == 1) CR_LAUNCH(1);
  else CR_LAUNCH(2);
#undef CR_LAUNCH
  return psam_launch_status();
}
