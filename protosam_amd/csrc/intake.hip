// psam_image_intake: a batch of uint8 images of different sizes -> resized, normalised, zero-padded fp32 [n, C, S, S] in ONE launch.
//
// The device form of the image-file intake of the reference (dataloaders/PolypDataset.py:319-348 `process_image_gt` through
// models/segment_anything/utils/transforms.py:62-110 `apply_image_torch` + `preprocess`, and predictor.py:47-58 `set_image`
// through `apply_image`): resize to (oh, ow) = get_preprocess_shape(H, W, S), (v - mean[c]) / std[c], then F.pad with zeros to
// S x S - the pad comes AFTER the normalisation, so the pad value is 0.0f, not -mean / std.
//
// Two arithmetic conventions, because the reference has two:
//   mode 0 (ATen)   F.interpolate(..., 'bilinear', antialias=True) on the float image: the taps, weights and fused multiply-adds
//                   of psam_resize_aa (interp.h `aa_tap` / `aa_weight` / `aa_mac`), width first with an fp32 intermediate, so
//                   the result is bit-identical to uint8 -> float, psam_resize_aa, psam_normalize_chw, pad. C = 1 with
//                   `threshold`: v > 0.5f ? 1 : 0 instead of the normalisation (PolypDataset.py:332-333).
//   mode 1 (Pillow) Image.resize((ow, oh), BILINEAR) on the uint8 image (what torchvision's `resize(to_pil_image(..))` reaches):
//                   Pillow's 8-bit resampling (src/libImaging/Resample.c: `precompute_coeffs`, `normalize_coeffs_8bpc`,
//                   `ImagingResampleHorizontal_8bpc` / `Vertical_8bpc`): double-precision triangle weights normalised to sum
//                   1, each turned into int(0.5 + w * 2^22); a pass accumulates in int32 from 1 << 21, shifts right by 22 and
//                   clips to 0..255; width first with a uint8 intermediate; a pass whose size does not change is skipped
//                   (here: one tap of weight 2^22, which is the identity). The doubles are computed with the round-to-nearest
//                   intrinsics, one per C operation, so nothing is contracted. Then norm_px of the uint8 value.
//
// Layout of the work: a workgroup of 4 waves makes a tile of `ty` output rows x 64 output columns of one image, all C channels.
// It first tabulates, in LDS, the taps of its 64 columns and ty rows (so a weight is divided once per workgroup, not once per
// source row). Then, for every source row the tile's taps reach, one wave copies the row's byte span into its LDS staging line
// (16-byte global loads between the first and last 16-byte boundary of the span, single bytes outside them: nothing is read
// outside the span) and its 64 lanes run the width pass from there into `mid` [C][rows][64] in LDS. The height pass reads
// `mid` (conflict-free: lane = column) and each wave stores whole 256-byte rows. There is no scratch in global memory.
// `ty` is the largest of 8, 4, 2, 1 with which the workgroup's LDS stays within 80 KiB, half of the CU's 160 KiB, so at least two
// workgroups share a CU at the largest supported scale (16), and eight at the scales of everyday images (<= 2, about 20 KiB).
#include "common.h"
#include "interp.h"

#define INTAKE_TX 64
#define INTAKE_MAX_SIDE 8192
#define INTAKE_MAX_SCALE 16
#define INTAKE_MAX_S 16384
#define INTAKE_LDS_CAP (80 * 1024)
#define INTAKE_ROW_WORDS 5   // byte offset, H, W, oh, ow (int64 each)

// taps of output index i along one axis into LDS: *mn = first source index, *sz = number of taps, w[j * stride] = weight j
// (fp32 bits in mode 0, the 22-bit fixed-point integer in mode 1). At most kmax weights are written; sz is left as computed.
template <int MODE>
__device__ __forceinline__ void intake_taps(int i, int in_len, int out_len, int kmax, float* w, int stride, int* mn, int* sz) {
  if (MODE == 0) {
    const AaTap t = aa_tap(i, in_len, out_len);
    *mn = t.xmin;
    *sz = t.xsize;
    const int n = t.xsize < kmax ? t.xsize : kmax;
    for (int j = 0; j < n; ++j) w[j * stride] = aa_weight(t, j);
  } else {
    if (in_len == out_len) {   // Pillow skips the pass
      *mn = i;
      *sz = 1;
      w[0] = __int_as_float(1 << 22);
      return;
    }
    const double scale = __ddiv_rn((double)in_len, (double)out_len);
    const double fs = scale < 1.0 ? 1.0 : scale;    // filterscale; support = 1.0 * filterscale for the triangle
    const double center = __dmul_rn(__dadd_rn((double)i, 0.5), scale);
    const double ss = __ddiv_rn(1.0, fs);
    int xmin = (int)__dadd_rn(__dsub_rn(center, fs), 0.5);
    xmin = xmin < 0 ? 0 : xmin;
    int xmax = (int)__dadd_rn(__dadd_rn(center, fs), 0.5);
    xmax = xmax > in_len ? in_len : xmax;
    const int xs = xmax - xmin;
    *mn = xmin;
    *sz = xs;
    double ww = 0.0;
    for (int j = 0; j < xs; ++j) {
      double a = __dmul_rn(__dadd_rn(__dsub_rn((double)(j + xmin), center), 0.5), ss);
      a = a < 0.0 ? -a : a;
      ww = __dadd_rn(ww, a < 1.0 ? __dsub_rn(1.0, a) : 0.0);
    }
    const int n = xs < kmax ? xs : kmax;
    for (int j = 0; j < n; ++j) {
      double a = __dmul_rn(__dadd_rn(__dsub_rn((double)(j + xmin), center), 0.5), ss);
      a = a < 0.0 ? -a : a;
      double k = a < 1.0 ? __dsub_rn(1.0, a) : 0.0;
      if (ww != 0.0) k = __ddiv_rn(k, ww);
      const int q = k < 0.0 ? (int)__dadd_rn(-0.5, __dmul_rn(k, 4194304.0)) : (int)__dadd_rn(0.5, __dmul_rn(k, 4194304.0));
      w[j * stride] = __int_as_float(q);
    }
  }
}

template <int C, int MODE>
__global__ __launch_bounds__(256) void image_intake_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ rows,
                                                           int S, int ty, int rows_max, int cols_max, int kmax, int stage_bytes,
                                                           int threshold, float m0, float m1, float m2, float s0, float s1,
                                                           float s2, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char intake_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.z, x0 = blockIdx.x * INTAKE_TX, y0 = blockIdx.y * ty;
  const long long* rw = rows + (size_t)b * INTAKE_ROW_WORDS;
  const long long off = rw[0];
  const int H = (int)rw[1], W = (int)rw[2], oh = (int)rw[3], ow = (int)rw[4];
  float* ob = out + (size_t)b * C * S * S;
  const int x = x0 + lane;
  if (y0 >= oh || x0 >= ow) {   // the whole tile is padding (uniform over the workgroup: no barrier has been met)
    for (int k = wv; k < ty * C; k += 4) {
      const int c = k / ty, y = y0 + k % ty;
      if (y < S && x < S) ob[((size_t)c * S + y) * S + x] = 0.f;
    }
    return;
  }
  unsigned char* stage = intake_lds + (size_t)wv * stage_bytes;
  float* mid = reinterpret_cast<float*>(intake_lds + (size_t)4 * stage_bytes);
  float* wx = mid + (size_t)C * rows_max * INTAKE_TX;
  float* wy = wx + (size_t)kmax * INTAKE_TX;
  int* xmin_s = reinterpret_cast<int*>(wy + (size_t)ty * kmax);
  int* xsize_s = xmin_s + INTAKE_TX;
  int* ymin_s = xsize_s + INTAKE_TX;
  int* ysize_s = ymin_s + 8;

  if (tid < INTAKE_TX) {
    if (x < ow) intake_taps<MODE>(x, W, ow, kmax, wx + lane, INTAKE_TX, xmin_s + lane, xsize_s + lane);
  } else if (tid < INTAKE_TX + ty) {
    const int yy = tid - INTAKE_TX;
    if (y0 + yy < oh) intake_taps<MODE>(y0 + yy, H, oh, kmax, wy + (size_t)yy * kmax, 1, ymin_s + yy, ysize_s + yy);
  }
  __syncthreads();

  const int nvy = min(ty, oh - y0), nvx = min(INTAKE_TX, ow - x0);
  const int r0 = ymin_s[0], r1 = ymin_s[nvy - 1] + ysize_s[nvy - 1];      // first taps and ends of taps grow with the index
  const int c0 = xmin_s[0], c1 = xmin_s[nvx - 1] + xsize_s[nvx - 1];
  // The launcher sized LDS from bounds on these spans. Should they not hold, nothing is staged and the tile is NaN.
  const bool fits = r0 >= 0 && c0 >= 0 && r1 <= H && c1 <= W && r1 - r0 <= rows_max && c1 - c0 <= cols_max;

  const int xm = x < ow ? xmin_s[lane] : c0;
  const int xs = x < ow ? xsize_s[lane] : 0;
  const int len = (c1 - c0) * C;
  if (fits) {
    for (int rb = r0; rb < r1; rb += 4) {
      const int r = rb + wv;
      int shift = 0;
      if (r < r1) {
        const uint8_t* g = src + off + ((long long)r * W + c0) * C;
        shift = (int)(reinterpret_cast<uintptr_t>(g) & 15);
        int head = (16 - shift) & 15;
        head = head < len ? head : len;
        const int nvec = (len - head) >> 4;
        if (lane < head) stage[shift + lane] = g[lane];
        const uint4* gv = reinterpret_cast<const uint4*>(g + head);       // 16-byte aligned when nvec > 0
        uint4* sv = reinterpret_cast<uint4*>(stage + shift + head);
        for (int i = lane; i < nvec; i += 64) sv[i] = gv[i];
        const int tail0 = head + (nvec << 4);
        if (tail0 + lane < len) stage[shift + tail0 + lane] = g[tail0 + lane];
      }
      __syncthreads();
      if (r < r1 && xs > 0 && xs <= kmax) {
        const unsigned char* sp = stage + shift + (xm - c0) * C;
        float* mo = mid + (size_t)(r - r0) * INTAKE_TX + lane;
        if (MODE == 0) {
          float acc[C];
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = 0.f;
          for (int j = 0; j < xs; ++j) {
            const float w = wx[j * INTAKE_TX + lane];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = aa_mac(acc[c], w, (float)sp[j * C + c]);
          }
#pragma unroll
          for (int c = 0; c < C; ++c) mo[(size_t)c * rows_max * INTAKE_TX] = acc[c];
        } else {
          int acc[C];
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
          for (int j = 0; j < xs; ++j) {
            const int k = __float_as_int(wx[j * INTAKE_TX + lane]);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)sp[j * C + c] * k;
          }
#pragma unroll
          for (int c = 0; c < C; ++c) {
            int v = acc[c] >> 22;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            mo[(size_t)c * rows_max * INTAKE_TX] = __int_as_float(v);
          }
        }
      }
      __syncthreads();
    }
  }

  for (int yy = wv; yy < ty; yy += 4) {
    const int y = y0 + yy;
    if (y >= S || x >= S) continue;
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = 0.f;
    if (y < oh && x < ow) {
      const int ys = ysize_s[yy];
      if (!fits || xs > kmax || ys > kmax) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = __int_as_float(0x7fc00000);
      } else {
        const float* mi = mid + (size_t)(ymin_s[yy] - r0) * INTAKE_TX + lane;
        const float* wr = wy + (size_t)yy * kmax;
        if (MODE == 0) {
          for (int j = 0; j < ys; ++j) {
            const float w = wr[j];
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = aa_mac(v[c], w, mi[((size_t)c * rows_max + j) * INTAKE_TX]);
          }
        } else {
          int acc[C];
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
          for (int j = 0; j < ys; ++j) {
            const int k = __float_as_int(wr[j]);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += __float_as_int(mi[((size_t)c * rows_max + j) * INTAKE_TX]) * k;
          }
#pragma unroll
          for (int c = 0; c < C; ++c) {
            int q = acc[c] >> 22;
            q = q < 0 ? 0 : (q > 255 ? 255 : q);
            v[c] = (float)q;
          }
        }
        if (threshold) {
#pragma unroll
          for (int c = 0; c < C; ++c) v[c] = v[c] > 0.5f ? 1.f : 0.f;
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) v[c] = norm_px(v[c], c == 0 ? m0 : (c == 1 ? m1 : m2), c == 0 ? s0 : (c == 1 ? s1 : s2));
        }
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) ob[((size_t)c * S + y) * S + x] = v[c];
  }
}

// rows_host: n rows of {byte offset of the image in src, H, W, oh, ow} (int64 each, HOST memory). They are checked here, then
// copied to rows_dev (n * 5 int64 of DEVICE memory), which is the table the kernel reads.
extern "C" int psam_image_intake(const void* src, long long src_bytes, const long long* rows_host, void* rows_dev, int n, int C,
                                 int S, int mode, int threshold, const float* mean3, const float* std3, float* out,
                                 void* stream) {
  if (!src || !rows_host || !rows_dev || !out || src_bytes <= 0 || n <= 0 || n > 65535 || (C != 1 && C != 3) || S <= 0 ||
      S > INTAKE_MAX_S || mode < 0 || mode > 1 || threshold < 0 || threshold > 1)
    return PSAM_ERR_ARG;
  if (threshold ? (C != 1 || mode != 0) : (!mean3 || !std3)) return PSAM_ERR_ARG;
  double sy = 1.0, sx = 1.0;   // largest scale (source side / resized side, at least 1) along each axis over the batch
  for (int i = 0; i < n; ++i) {
    const long long* r = rows_host + (size_t)i * INTAKE_ROW_WORDS;
    const long long off = r[0], H = r[1], W = r[2], oh = r[3], ow = r[4];
    if (H < 1 || W < 1 || H > INTAKE_MAX_SIDE || W > INTAKE_MAX_SIDE || oh < 1 || ow < 1 || oh > S || ow > S ||
        H > INTAKE_MAX_SCALE * oh || W > INTAKE_MAX_SCALE * ow || off < 0 || off > src_bytes || H * W * C > src_bytes - off)
      return PSAM_ERR_ARG;
    const double ay = (double)H / (double)oh, ax = (double)W / (double)ow;
    sy = ay > sy ? ay : sy;
    sx = ax > sx ? ax : sx;
  }
  // taps of one output index: int(c + s + .5) - int(c - s + .5) <= floor(2 s) + 1 (+ 1 for the fp32 rounding of c +- s);
  // source span of t consecutive output indices: (t - 1) * scale + 2 s + 1, likewise
  const double sm = sy > sx ? sy : sx;
  const int kmax = (int)(2.0 * sm) + 2;
  const int cols_max = (int)((INTAKE_TX - 1) * sx + 2.0 * sx) + 2;
  const int stage_bytes = (cols_max * C + 16 + 15) & ~15;
  int ty = 8, rows_max = 0;
  size_t lds = 0;
  for (;; ty >>= 1) {
    rows_max = (int)((ty - 1) * sy + 2.0 * sy) + 2;
    lds = (size_t)4 * stage_bytes + ((size_t)C * rows_max * INTAKE_TX + (size_t)kmax * INTAKE_TX + (size_t)ty * kmax + 2 * INTAKE_TX + 16) * 4;
    if (lds <= INTAKE_LDS_CAP || ty == 1) break;
  }
  if (lds > INTAKE_LDS_CAP) return PSAM_ERR_ARG;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)image_intake_kernel<1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, INTAKE_LDS_CAP);
    (void)hipFuncSetAttribute((const void*)image_intake_kernel<1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, INTAKE_LDS_CAP);
    (void)hipFuncSetAttribute((const void*)image_intake_kernel<3, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, INTAKE_LDS_CAP);
    (void)hipFuncSetAttribute((const void*)image_intake_kernel<3, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, INTAKE_LDS_CAP);
    attr_set = true;
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(rows_dev, rows_host, (size_t)n * INTAKE_ROW_WORDS * sizeof(long long), hipMemcpyHostToDevice, st) != hipSuccess) {
    (void)hipGetLastError();
    return PSAM_ERR_LAUNCH;
  }
  const dim3 grid((S + INTAKE_TX - 1) / INTAKE_TX, (S + ty - 1) / ty, n), block(256);
  const float zero3[3] = {0.f, 0.f, 0.f}, one3[3] = {1.f, 1.f, 1.f};
  const float* m = threshold ? zero3 : mean3;
  const float* s = threshold ? one3 : std3;
  const float m1 = C == 3 ? m[1] : m[0], m2 = C == 3 ? m[2] : m[0], s1 = C == 3 ? s[1] : s[0], s2 = C == 3 ? s[2] : s[0];
#define INTAKE_LAUNCH(CC, MM)                                                                                                  \
  hipLaunchKernelGGL((image_intake_kernel<CC, MM>), grid, block, lds, st, (const uint8_t*)src, (const long long*)rows_dev, S, ty, \
                     rows_max, cols_max, kmax, stage_bytes, threshold, m[0], m1, m2, s[0], s1, s2, out)
  if (C == 3) {
    if (mode == 0) INTAKE_LAUNCH(3, 0); else INTAKE_LAUNCH(3, 1);
  } else {
    if (mode == 0) INTAKE_LAUNCH(1, 0); else INTAKE_LAUNCH(1, 1);
  }
#undef INTAKE_LAUNCH
  return psam_launch_status();
}
