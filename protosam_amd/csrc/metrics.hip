// Scoring of segmentation masks on the device: confusion counts and bounding boxes of many (prediction plane, label plane)
// pairs in one launch. Replaces the host side of the reference's evaluation loops: get_dice_iou_precision_recall and
// get_bounding_box per slice (validation_protosam.py:49-62,169-185,400-409) and Metric.record per slice and label
// (util/metric.py:50-107), which run on `query_pred.cpu()`.
//
//  psam_seg_counts : rows int32 [n, 4] = (pred plane, pred value, label plane, label value). Pixel i of a row is PREDICTED iff
//    pred[pred plane][i] == pred value and TRUE iff label[label plane][i] == label value. out int64 [n, 12] =
//    {tp, fp, fn, tn, pred x0, pred y0, pred x1, pred y1, gt x0, gt y0, gt x1, gt y1}.
//
// Shape of the kernel. A streaming reduction: every byte of a plane is used once per row, so the floor is bytes over the HBM
// rate. A plane [H, W] is contiguous, so it is read as a flat run of pixels, not row by row: a lane takes a UNIT of PX =
// 16 / max(sizeof pred, sizeof label) pixels, i.e. one 16-byte load of the wider type and a 4..16-byte load of the other, and
// the 64 lanes of a wave read 64 consecutive units. Units start where the PREDICTION plane is PX-element aligned (it is the
// larger stream: C prediction planes per label plane); the pixels before the first and after the last whole unit (< 2 PX) are
// read one by one by the workgroup of chunk 0. The label plane of an odd storage offset is then read through loads the
// compiler knows to be unaligned. A unit becomes two PX-bit masks (uint8: four pixels per 32-bit word by a carry-free
// zero-byte test), the counts are popcounts, and the boxes come from the lowest / highest set bit unless the unit crosses
// the end of an image row (then bit by bit). x, y of a lane's first unit cost one division; the next units step by a
// wave-uniform (dx, dy).
// A workgroup (256 lanes) reduces SC_UNROLL * 256 units of ONE row: wave64 shuffles, 4 x 12 ints through LDS, then ONE set
// of at most 12 int64 atomics (add for the counts, min / max for the boxes; zero sums and empty boxes are not sent). Integer
// atomics: the table does not depend on scheduling.
// Rows that share a label plane (the C classes of a slice, rows k*C .. k*C+C-1 of class_rows): the grid is one-dimensional
// (any n, no 65535 limit), LOGICAL workgroup g -> chunk g / n, row g % n, so the C workgroups that read the same piece of a
// label plane are neighbours, and xcd_remap gives each XCD a contiguous range of g: the neighbours run on one XCD at about
// the same time and the second..C-th read of the piece is served by that XCD's L2 (or, failing that, by the 256 MiB
// Infinity Cache, which a whole call's planes fit in). This is placement for speed only; nothing depends on it.
#include "common.h"
#include <type_traits>

#define SC_THREADS 256
#define SC_UNROLL 4
#define SC_COLS 12
#define SC_EMPTY_MIN 0x7fffffff

template <typename T>
__device__ __forceinline__ bool sc_eq(T v, int value) {
  if constexpr (std::is_same<T, float>::value) return v == (float)value;   // by value: -0. == 0, NaN equals nothing
  else return (int)v == value;
}

// PX elements of T as they lie in memory
template <typename T, int PX>
struct ScRaw {
  uint32_t w[PX * sizeof(T) / 4];
};
template <typename T, int PX>
__device__ __forceinline__ void sc_load(ScRaw<T, PX>& r, const T* __restrict__ p) {   // p is element-aligned only
  __builtin_memcpy(r.w, p, sizeof(r.w));
}

// The mask of a unit: pixel j -> bit 8 * (j % 4) + j / 4 (the order in which the uint8 form below delivers them; counts do
// not care, sc_box_add undoes it).
template <typename T, int PX>
__device__ __forceinline__ uint32_t sc_eq_mask(const ScRaw<T, PX>& r, int value) {
  uint32_t m = 0;
  if constexpr (sizeof(T) == 1) {
    const uint32_t pat = (uint32_t)(value & 255) * 0x01010101u;
#pragma unroll
    for (int k = 0; k < PX / 4; ++k) {                            // four pixels per word
      const uint32_t x = r.w[k] ^ pat;
      const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // 0x80 in every byte of x that is 0, no carries
      m |= z >> (7 - k);
    }
    return (unsigned)value > 255u ? 0u : m;
  } else {
    T v[PX];
    __builtin_memcpy(v, r.w, sizeof(r.w));
#pragma unroll
    for (int j = 0; j < PX; ++j) m |= (uint32_t)sc_eq<T>(v[j], value) << (8 * (j & 3) + (j >> 2));
    return m;
  }
}

struct ScBox {
  int x0, y0, x1, y1;
};
__device__ __forceinline__ void sc_box_point(ScBox& b, int x, int y) {
  b.x0 = min(b.x0, x); b.x1 = max(b.x1, x);
  b.y0 = min(b.y0, y); b.y1 = max(b.y1, y);
}

// m: the mask of the PX pixels x .. x + PX - 1 of image row y, running on into the next rows where x + j >= W
template <int PX>
__device__ __forceinline__ void sc_box_add(ScBox& b, uint32_t m, int x, int y, int W) {
  if (!m) return;
  if (x + PX <= W) {
    const uint32_t any = (m | (m >> 8) | (m >> 16) | (m >> 24)) & 0xffu;      // bit k: some pixel with j / 4 == k
    const int klo = __builtin_ctz(any), khi = 31 - __builtin_clz(any);
    const int jlo = 4 * klo + (__builtin_ctz((m >> klo) & 0x01010101u) >> 3);
    const int jhi = 4 * khi + ((31 - __builtin_clz((m >> khi) & 0x01010101u)) >> 3);
    b.x0 = min(b.x0, x + jlo); b.x1 = max(b.x1, x + jhi);
    b.y0 = min(b.y0, y); b.y1 = max(b.y1, y);
    return;
  }
  while (m) {
    const int pos = __builtin_ctz(m);
    m &= m - 1;
    const int xj = x + 4 * (pos & 7) + (pos >> 3), q = xj / W;
    sc_box_point(b, xj - q * W, y + q);
  }
}

__global__ void seg_counts_init_kernel(long long* __restrict__ out, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % SC_COLS);
  out[i] = c < 4 ? 0 : (((c - 4) & 3) < 2 ? (long long)SC_EMPTY_MIN : -1);
}

template <typename P, typename L>
__global__ __launch_bounds__(SC_THREADS) void seg_counts_kernel(const P* __restrict__ pred, int pred_planes, long long pred_stride,
                                                                const L* __restrict__ label, int label_planes,
                                                                long long label_stride, int W, int N,
                                                                const int* __restrict__ rows, int n, long long* __restrict__ out) {
  constexpr int PX = 16 / (int)(sizeof(P) > sizeof(L) ? sizeof(P) : sizeof(L));
  constexpr int UPC = SC_THREADS * SC_UNROLL;                     // units per workgroup
  const int g = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int row = g % n, chunk = g / n;
  const int pp = rows[4 * row + 0], pv = rows[4 * row + 1], lp = rows[4 * row + 2], lv = rows[4 * row + 3];
  if (pp < 0 || pp >= pred_planes || lp < 0 || lp >= label_planes) return;     // (uniform in the workgroup)
  const P* __restrict__ ps = pred + (long long)pp * pred_stride;
  const L* __restrict__ ls = label + (long long)lp * label_stride;
  constexpr unsigned ALIGN = PX * sizeof(P);
  const int head = min(N, (int)(((ALIGN - (unsigned)((uintptr_t)ps % ALIGN)) % ALIGN) / sizeof(P)));
  const int U = (N - head) / PX;                                  // whole units
  const int tid = threadIdx.x;

  int npx = 0, np = 0, nl = 0, nt = 0;
  ScBox bp = {SC_EMPTY_MIN, SC_EMPTY_MIN, -1, -1}, bl = bp;

  const int u0 = chunk * UPC + tid;
  if (u0 < U) {
    ScRaw<P, PX> rp[SC_UNROLL];
    ScRaw<L, PX> rl[SC_UNROLL];
#pragma unroll
    for (int it = 0; it < SC_UNROLL; ++it) {                      // every load of the lane is in flight before the first use
      const int i = head + min(u0 + it * SC_THREADS, U - 1) * PX; // (past the last unit: that unit again, not counted below)
      sc_load<P, PX>(rp[it], ps + i);
      sc_load<L, PX>(rl[it], ls + i);
    }
    const int i0 = head + u0 * PX;
    int y = i0 / W, x = i0 - y * W;
    const int dy = (SC_THREADS * PX) / W, dx = (SC_THREADS * PX) - dy * W;      // wave-uniform step of one iteration
#pragma unroll
    for (int it = 0; it < SC_UNROLL; ++it) {
      if (u0 + it * SC_THREADS < U) {
        const uint32_t mp = sc_eq_mask<P, PX>(rp[it], pv), ml = sc_eq_mask<L, PX>(rl[it], lv);
        npx += PX; np += __builtin_popcount(mp); nl += __builtin_popcount(ml); nt += __builtin_popcount(mp & ml);
        sc_box_add<PX>(bp, mp, x, y, W);
        sc_box_add<PX>(bl, ml, x, y, W);
        x += dx; y += dy;
        if (x >= W) { x -= W; ++y; }
      }
    }
  }
  if (chunk == 0) {                                               // the < PX pixels before and the < PX after the units
    const int tail0 = head + U * PX;
    if (tid < head + (N - tail0)) {
      const int i = tid < head ? tid : tail0 + (tid - head);
      const int mp = sc_eq<P>(ps[i], pv), ml = sc_eq<L>(ls[i], lv);
      const int y = i / W, x = i - y * W;
      npx += 1; np += mp; nl += ml; nt += mp & ml;
      if (mp) sc_box_point(bp, x, y);
      if (ml) sc_box_point(bl, x, y);
    }
  }

  int v[SC_COLS] = {nt, np - nt, nl - nt, npx - np - nl + nt, bp.x0, bp.y0, bp.x1, bp.y1, bl.x0, bl.y0, bl.x1, bl.y1};
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < SC_COLS; ++c) {
      const int t = __shfl_xor(v[c], o, 64);
      v[c] = c < 4 ? v[c] + t : (((c - 4) & 3) < 2 ? min(v[c], t) : max(v[c], t));
    }
  }
  __shared__ int red[SC_THREADS / WAVE][SC_COLS];
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < SC_COLS; ++c) red[tid >> 6][c] = v[c];
  }
  __syncthreads();
  if (tid < SC_COLS) {
    const int c = tid;
    const bool is_sum = c < 4, is_min = ((c - 4) & 3) < 2;
    int r = red[0][c];
#pragma unroll
    for (int w = 1; w < SC_THREADS / WAVE; ++w) {
      const int t = red[w][c];
      r = is_sum ? r + t : (is_min ? min(r, t) : max(r, t));
    }
    long long* dst = out + (long long)row * SC_COLS + c;
    if (is_sum) {
      if (r) atomicAdd((unsigned long long*)dst, (unsigned long long)r);
    } else if (is_min) {
      if (r != SC_EMPTY_MIN) atomicMin(dst, (long long)r);
    } else if (r >= 0) {
      atomicMax(dst, (long long)r);
    }
  }
}

template <typename P, typename L>
static void seg_counts_launch(const void* pred, int pred_planes, long long pred_stride, const void* label, int label_planes,
                              long long label_stride, int W, int N, const int* rows, int n, long long* out, hipStream_t s) {
  constexpr int PX = 16 / (int)(sizeof(P) > sizeof(L) ? sizeof(P) : sizeof(L));
  const int units = (N + PX - 1) / PX, upc = SC_THREADS * SC_UNROLL;
  const long long chunks = (units + upc - 1) / upc;               // >= 1; chunk 0 also takes the edge pixels
  hipLaunchKernelGGL((seg_counts_kernel<P, L>), dim3((unsigned)(chunks * n)), dim3(SC_THREADS), 0, s, (const P*)pred,
                     pred_planes, pred_stride, (const L*)label, label_planes, label_stride, W, N, rows, n, out);
}

template <typename P>
static int seg_counts_label(int label_dtype, const void* pred, int pred_planes, long long pred_stride, const void* label,
                            int label_planes, long long label_stride, int W, int N, const int* rows, int n, long long* out,
                            hipStream_t s) {
#define SC_GO(L) seg_counts_launch<P, L>(pred, pred_planes, pred_stride, label, label_planes, label_stride, W, N, rows, n, out, s)
  switch (label_dtype) {
    case 0: SC_GO(int16_t); return PSAM_OK;
    case 1: SC_GO(float); return PSAM_OK;
    case 2: SC_GO(uint8_t); return PSAM_OK;
    case 3: SC_GO(int32_t); return PSAM_OK;
  }
#undef SC_GO
  return PSAM_ERR_ARG;
}

static int sc_elem_size(int dtype) {
  return dtype == 0 ? 2 : (dtype == 1 || dtype == 3) ? 4 : dtype == 2 ? 1 : 0;
}

extern "C" int psam_seg_counts(const void* pred, int pred_dtype, int pred_planes, long long pred_stride, const void* label,
                               int label_dtype, int label_planes, long long label_stride, int H, int W, const int* rows, int n,
                               long long* out, void* stream) {
  const int sp = sc_elem_size(pred_dtype), sl = sc_elem_size(label_dtype);
  if (!pred || !label || !rows || !out || sp == 0 || sl == 0 || pred_planes <= 0 || label_planes <= 0 || H <= 0 || W <= 0 ||
      n <= 0 || pred_stride < 0 || label_stride < 0 || (long long)H * W > 0x7fffffffLL - 16 * SC_THREADS ||
      (uintptr_t)pred % sp || (uintptr_t)label % sl)
    return PSAM_ERR_ARG;
  const int N = H * W, px = 16 / (sp > sl ? sp : sl);
  const long long units = (N + px - 1) / px, chunks = (units + SC_THREADS * SC_UNROLL - 1) / (SC_THREADS * SC_UNROLL);
  if (chunks * n > 0x7fffffffLL) return PSAM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)n * SC_COLS;
  hipLaunchKernelGGL(seg_counts_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, out, total);
  int st = PSAM_ERR_ARG;
  switch (pred_dtype) {
    case 0: st = seg_counts_label<int16_t>(label_dtype, pred, pred_planes, pred_stride, label, label_planes, label_stride, W, N, rows, n, out, s); break;
    case 1: st = seg_counts_label<float>(label_dtype, pred, pred_planes, pred_stride, label, label_planes, label_stride, W, N, rows, n, out, s); break;
    case 2: st = seg_counts_label<uint8_t>(label_dtype, pred, pred_planes, pred_stride, label, label_planes, label_stride, W, N, rows, n, out, s); break;
    case 3: st = seg_counts_label<int32_t>(label_dtype, pred, pred_planes, pred_stride, label, label_planes, label_stride, W, N, rows, n, out, s); break;
  }
  return st != PSAM_OK ? st : psam_launch_status();
}
