// Surface-distance metrics on the device: Hausdorff distance (HD), its 95th percentile (HD95) and the average symmetric
// surface distance (ASSD) of many (prediction, ground truth) pairs, per slice (depth 1) or per scan (depth D), with voxel spacing.
// The definitions are MedPy's hd / hd95 / asd / assd with connectivity=1, restated:
//   surface S(M) : the voxels of M with a face neighbour (4 in a plane when D == 1, 6 when D > 1) that is background or lies
//                  outside the row's D x H x W range (= M ^ binary_erosion(M, cross) with border_value 0);
//   d(p)         : min over the OTHER surface of the Euclidean distance with spacing, squared in fp32 from exact integer offsets
//                  with every operation rounded separately, d2 = ((dx*sx)*(dx*sx) + (dy*sy)*(dy*sy)) + (dz*sz)*(dz*sz)
//                  (a min over fp32 values is order-independent: d2 has one right bit pattern);
//   hd = max of the two directed maxima, hd95 = numpy.percentile(both directed sets, 95) (linear), asd_pg / asd_gp = the directed
//   means, assd = their mean, all float64 functions of sqrt((double)d2); NaN where either surface is empty.
//
//  psam_surface_points : rows int32 [n,5] = (first pred plane, pred value, first label plane, label value, depth D), comparisons
//    and plane addressing as psam_seg_counts. Count (integer atomics, one per wave and side) -> counts [n,2]; one exclusive scan
//    of the 2n counts -> offsets [2n+1]; fill -> points [cap], a voxel as its linear index in the row's D*H*W range, segment
//    2r = S(P) of row r, 2r+1 = S(G). A row whose segments end beyond cap is flagged (status 1) and not filled.
//  psam_surface_dist   : all pairs, the n-body shape. A workgroup owns SURF_TILE query points of ONE segment and streams the other
//    segment of the row through LDS, SURF_TILE points at a time, decoded to float (x, y, z) once per tile; a lane keeps its
//    minimum in a register. The grid is sized from cap (at most cap / SURF_TILE + 2n tiles); a workgroup finds its segment and
//    tile in the device-side tile scan and leaves when there is none.
//  psam_surface_stats  : one workgroup per row over the d2 of its two segments, each sorted ascending: sums in float64 in a
//    fixed order (lane-strided partial sums, then a fixed tree), the two order statistics of hd95 by a k-th-of-two-sorted-arrays
//    search. No float atomics: the table is the same bits run to run and for any cap that fits.
#include "common.h"
#include <type_traits>

#define SURF_THREADS 256
#define SURF_UNROLL 8
#define SURF_TILE 256
#define SURF_COLS 8

template <typename T>
__device__ __forceinline__ bool sf_eq(T v, int value) {                   // as sc_eq of metrics.hip
  if constexpr (std::is_same<T, float>::value) return v == (float)value;
  else return (int)v == value;
}

// voxel (z, rem) of the row's range is set: is it a surface voxel?
template <typename T>
__device__ __forceinline__ bool sf_surface(const T* __restrict__ base, long long stride, int D, int H, int W, int z, int rem,
                                           int value) {
  const int y = rem / W, x = rem - y * W;
  if (x == 0 || x == W - 1 || y == 0 || y == H - 1) return true;
  const T* p = base + (long long)z * stride + rem;
  if (!sf_eq<T>(p[-1], value) || !sf_eq<T>(p[1], value) || !sf_eq<T>(p[-W], value) || !sf_eq<T>(p[W], value)) return true;
  if (D > 1) {
    if (z == 0 || z == D - 1) return true;
    if (!sf_eq<T>(p[-stride], value) || !sf_eq<T>(p[stride], value)) return true;
  }
  return false;
}

__device__ __forceinline__ bool sf_row_ok(const int* __restrict__ rows, int row, int pred_planes, int label_planes, int max_depth) {
  const int pp = rows[5 * row + 0], lp = rows[5 * row + 2], D = rows[5 * row + 4];
  return D >= 1 && D <= max_depth && pp >= 0 && lp >= 0 && (long long)pp + D <= pred_planes && (long long)lp + D <= label_planes;
}

__global__ void surface_init_kernel(int* __restrict__ counts, int* __restrict__ cursors, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) { counts[i] = 0; cursors[i] = 0; }
}

// FILL = false: counts[2 row + side] += surface voxels. FILL = true: the same voxels go to points[offsets[2 row + side] ..).
template <typename P, typename L, bool FILL>
__global__ __launch_bounds__(SURF_THREADS) void surface_voxels_kernel(const P* __restrict__ pred, int pred_planes, long long pred_stride,
                                                                      const L* __restrict__ label, int label_planes,
                                                                      long long label_stride, int H, int W, int max_depth,
                                                                      const int* __restrict__ rows, int n, int* __restrict__ counts,
                                                                      const int* __restrict__ offsets, const int* __restrict__ status,
                                                                      int* __restrict__ cursors, int* __restrict__ points) {
  const int g = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int row = g % n, chunk = g / n;
  if (!sf_row_ok(rows, row, pred_planes, label_planes, max_depth)) return;                // (uniform in the workgroup)
  if (FILL && status[row] != 0) return;
  const int pv = rows[5 * row + 1], lv = rows[5 * row + 3], D = rows[5 * row + 4];
  const int N = H * W, total = D * N;
  const int first = chunk * (SURF_THREADS * SURF_UNROLL);
  if (first >= total) return;
  const P* __restrict__ ps = pred + (long long)rows[5 * row + 0] * pred_stride;
  const L* __restrict__ ls = label + (long long)rows[5 * row + 2] * label_stride;
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  int end[2] = {0, 0}, off[2] = {0, 0};
  if (FILL) {
    off[0] = offsets[2 * row]; off[1] = offsets[2 * row + 1];
    end[0] = off[1]; end[1] = offsets[2 * row + 2];
  }
  int cnt[2] = {0, 0};
#pragma unroll
  for (int it = 0; it < SURF_UNROLL; ++it) {
    const int i = first + it * SURF_THREADS + tid;
    bool f[2] = {false, false};
    if (i < total) {
      const int z = D > 1 ? i / N : 0, rem = i - z * N;
      if (sf_eq<P>(ps[(long long)z * pred_stride + rem], pv)) f[0] = sf_surface<P>(ps, pred_stride, D, H, W, z, rem, pv);
      if (sf_eq<L>(ls[(long long)z * label_stride + rem], lv)) f[1] = sf_surface<L>(ls, label_stride, D, H, W, z, rem, lv);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const unsigned long long m = __ballot(f[s]);
      if (!FILL) {
        cnt[s] += __builtin_popcountll(m);
      } else if (m) {                                                     // one atomic per wave: its voxels take a run of the segment
        int base = 0;
        if (lane == 0) base = atomicAdd(&cursors[2 * row + s], __builtin_popcountll(m));
        base = __shfl(base, 0, 64);
        const int pos = off[s] + base + __builtin_popcountll(m & below);
        if (f[s] && pos < end[s]) points[pos] = i;
      }
    }
  }
  if (!FILL && lane == 0) {
    if (cnt[0]) atomicAdd(&counts[2 * row], cnt[0]);
    if (cnt[1]) atomicAdd(&counts[2 * row + 1], cnt[1]);
  }
}

// One workgroup: exclusive scan of the 2n counts (int64 inside, saturated to INT_MAX in offsets), the rows' status, and the
// exclusive scan of the distance tiles of the rows that fit.
__global__ __launch_bounds__(SURF_THREADS) void surface_scan_kernel(const int* __restrict__ rows, int n, int pred_planes, int label_planes,
                                                                    int max_depth, const int* __restrict__ counts, int cap,
                                                                    int* __restrict__ offsets, int* __restrict__ tiles,
                                                                    int* __restrict__ status) {
  __shared__ long long part[SURF_THREADS];
  const int tid = threadIdx.x, per = (n + SURF_THREADS - 1) / SURF_THREADS;
  const int r0 = min(n, tid * per), r1 = min(n, r0 + per);
  long long sum = 0;
  for (int r = r0; r < r1; ++r) sum += (long long)counts[2 * r] + counts[2 * r + 1];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int t = 0; t < SURF_THREADS; ++t) { const long long v = part[t]; part[t] = run; run += v; }
  }
  __syncthreads();
  long long off = part[tid];
  long long nt = 0;
  for (int r = r0; r < r1; ++r) {
    const int cp = counts[2 * r], cg = counts[2 * r + 1];
    offsets[2 * r] = (int)min(off, (long long)0x7fffffff);
    offsets[2 * r + 1] = (int)min(off + cp, (long long)0x7fffffff);
    off += (long long)cp + cg;
    const bool fits = off <= cap || cp + cg == 0;                         // (an empty row takes no room)
    status[r] = !sf_row_ok(rows, r, pred_planes, label_planes, max_depth) ? 2 : (fits ? 0 : 1);
    if (fits) nt += (cp + SURF_TILE - 1) / SURF_TILE + (cg + SURF_TILE - 1) / SURF_TILE;
  }
  if (r1 == n && r0 < n) offsets[2 * n] = (int)min(off, (long long)0x7fffffff);
  __syncthreads();
  part[tid] = nt;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int t = 0; t < SURF_THREADS; ++t) { const long long v = part[t]; part[t] = run; run += v; }
  }
  __syncthreads();
  int t = (int)part[tid];                                                 // (<= cap / SURF_TILE + 2n: fits int32)
  for (int r = r0; r < r1; ++r) {
    const bool fits = status[r] != 1;
    tiles[2 * r] = t;
    if (fits) t += (counts[2 * r] + SURF_TILE - 1) / SURF_TILE;
    tiles[2 * r + 1] = t;
    if (fits) t += (counts[2 * r + 1] + SURF_TILE - 1) / SURF_TILE;
  }
  if (r1 == n && r0 < n) tiles[2 * n] = t;
}

template <bool Z3>
__device__ __forceinline__ void sf_decode(int idx, int N, int W, float& x, float& y, float& z) {
  int zi = 0;
  if (Z3) { zi = idx / N; idx -= zi * N; }
  const int yi = idx / W;
  x = (float)(idx - yi * W); y = (float)yi; z = (float)zi;
}

template <bool Z3>
__device__ __forceinline__ float sf_d2(float qx, float qy, float qz, float x, float y, float z, float sx, float sy, float sz) {
  const float dx = __fmul_rn(__fsub_rn(qx, x), sx), dy = __fmul_rn(__fsub_rn(qy, y), sy);      // the differences are exact
  float d = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
  if (Z3) {
    const float dz = __fmul_rn(__fsub_rn(qz, z), sz);
    d = __fadd_rn(d, __fmul_rn(dz, dz));
  }
  return d;
}

template <bool Z3>
__global__ __launch_bounds__(SURF_TILE) void surface_dist_kernel(const int* __restrict__ points, const int* __restrict__ offsets,
                                                                 const int* __restrict__ tiles, int n, int N, int W, float sz, float sy,
                                                                 float sx, float* __restrict__ d2, long long* __restrict__ keys) {
  __shared__ __attribute__((aligned(16))) float lx[SURF_TILE];
  __shared__ __attribute__((aligned(16))) float ly[SURF_TILE];
  __shared__ __attribute__((aligned(16))) float lz[SURF_TILE];
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= tiles[2 * n]) return;                                          // (uniform) no such tile
  int lo = 0, hi = 2 * n;                                                 // the segment s with tiles[s] <= g < tiles[s + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tiles[mid] <= g) lo = mid; else hi = mid;
  }
  const int s = lo, o = s ^ 1;
  const int q0 = offsets[s], qn = offsets[s + 1] - q0, o0 = offsets[o], on = offsets[o + 1] - o0;
  const int qi = (g - tiles[s]) * SURF_TILE + tid;
  const bool valid = qi < qn;
  float qx, qy, qz;
  sf_decode<Z3>(valid ? points[q0 + qi] : 0, N, W, qx, qy, qz);
  float best = __builtin_inff();
  for (int base = 0; base < on; base += SURF_TILE) {
    __syncthreads();
    {
      const int j = base + tid;
      float x = __builtin_inff(), y = 0.f, z = 0.f;                       // past the segment: at infinity, never the minimum
      if (j < on) sf_decode<Z3>(points[o0 + j], N, W, x, y, z);
      lx[tid] = x; ly[tid] = y;
      if (Z3) lz[tid] = z;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < SURF_TILE; k += 4) {                              // every lane reads the same address: LDS broadcasts
      const f32x4 xs = *(const f32x4*)&lx[k], ys = *(const f32x4*)&ly[k];
      f32x4 zs = {0.f, 0.f, 0.f, 0.f};
      if (Z3) zs = *(const f32x4*)&lz[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) best = fminf(best, sf_d2<Z3>(qx, qy, qz, xs[e], ys[e], zs[e], sx, sy, sz));
    }
  }
  if (valid) {
    d2[q0 + qi] = best;
    if (keys) keys[q0 + qi] = ((long long)s << 32) | (long long)__float_as_uint(best);
  }
}

// value k (0-based) of the merge of two ascending arrays a [na], b [nb] (element i of either at v[i * stride]); 0 <= k < na + nb
__device__ __forceinline__ float sf_kth(const float* a, int na, const float* b, int nb, int stride, long long k) {
  long long lo = k + 1 - nb > 0 ? k + 1 - nb : 0, hi = k + 1 < na ? k + 1 : na;      // how many of the k + 1 smallest come from a
  while (lo < hi) {
    const long long i = (lo + hi) >> 1, j = k + 1 - i;
    if (a[i * stride] < b[(j - 1) * stride]) lo = i + 1; else hi = i;
  }
  const long long i = lo, j = k + 1 - lo;
  float v = -__builtin_inff();
  if (i > 0) v = fmaxf(v, a[(i - 1) * stride]);
  if (j > 0) v = fmaxf(v, b[(j - 1) * stride]);
  return v;
}

__global__ __launch_bounds__(SURF_THREADS) void surface_stats_kernel(const float* __restrict__ sorted, int stride,
                                                                     const int* __restrict__ counts, const int* __restrict__ offsets,
                                                                     const int* __restrict__ status, double* __restrict__ out) {
  __shared__ double red[2][SURF_THREADS];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int np = counts[2 * row], ng = counts[2 * row + 1], st = status[row];
  double* dst = out + (long long)row * SURF_COLS;
  const double nan = __builtin_nan("");
  if (st != 0 || np == 0 || ng == 0) {                                    // (uniform)
    if (tid == 0) {
      dst[0] = np; dst[1] = ng;
      for (int c = 2; c < 7; ++c) dst[c] = nan;
      dst[7] = st;
    }
    return;
  }
  const float* a = sorted + (long long)offsets[2 * row] * stride;
  const float* b = sorted + (long long)offsets[2 * row + 1] * stride;
  double sa = 0.0, sb = 0.0;                                              // lane-strided partial sums, ascending index
  for (int i = tid; i < np; i += SURF_THREADS) sa += sqrt((double)a[(long long)i * stride]);
  for (int i = tid; i < ng; i += SURF_THREADS) sb += sqrt((double)b[(long long)i * stride]);
  red[0][tid] = sa; red[1][tid] = sb;
  __syncthreads();
  for (int w = SURF_THREADS / 2; w > 0; w >>= 1) {                        // fixed tree
    if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; }
    __syncthreads();
  }
  if (tid != 0) return;
  const double asd_pg = red[0][0] / np, asd_gp = red[1][0] / ng;
  const float top = fmaxf(a[(long long)(np - 1) * stride], b[(long long)(ng - 1) * stride]);
  const long long m = (long long)np + ng;
  const double pos = (double)(m - 1) * 0.95;                              // numpy.percentile(., 95), method "linear"
  const double fl = floor(pos), t = pos - fl;
  const long long k0 = (long long)fl, k1 = k0 + 1 < m ? k0 + 1 : m - 1;
  const double v0 = sqrt((double)sf_kth(a, np, b, ng, stride, k0)), v1 = sqrt((double)sf_kth(a, np, b, ng, stride, k1));
  const double diff = v1 - v0;
  const double hd95 = t >= 0.5 ? v1 - diff * (1.0 - t) : v0 + diff * t;   // numpy's _lerp
  dst[0] = np; dst[1] = ng;
  dst[2] = sqrt((double)top);
  dst[3] = hd95;
  dst[4] = (asd_pg + asd_gp) * 0.5;
  dst[5] = asd_pg;
  dst[6] = asd_gp;
  dst[7] = 0.0;
}

struct SurfArgs {
  const void *pred, *label;
  int pred_planes, label_planes;
  long long pred_stride, label_stride;
  int H, W, max_depth, n;
  const int* rows;
  int *counts, *offsets, *status, *cursors, *points;
  hipStream_t s;
};

template <typename P, typename L, bool FILL>
static void surface_voxels_launch(const SurfArgs& a) {
  const long long total = (long long)a.max_depth * a.H * a.W, per = SURF_THREADS * SURF_UNROLL;
  const long long chunks = (total + per - 1) / per;
  hipLaunchKernelGGL((surface_voxels_kernel<P, L, FILL>), dim3((unsigned)(chunks * a.n)), dim3(SURF_THREADS), 0, a.s, (const P*)a.pred,
                     a.pred_planes, a.pred_stride, (const L*)a.label, a.label_planes, a.label_stride, a.H, a.W, a.max_depth, a.rows,
                     a.n, a.counts, a.offsets, a.status, a.cursors, a.points);
}

template <typename P, bool FILL>
static int surface_voxels_label(int label_dtype, const SurfArgs& a) {
  switch (label_dtype) {
    case 0: surface_voxels_launch<P, int16_t, FILL>(a); return PSAM_OK;
    case 1: surface_voxels_launch<P, float, FILL>(a); return PSAM_OK;
    case 2: surface_voxels_launch<P, uint8_t, FILL>(a); return PSAM_OK;
    case 3: surface_voxels_launch<P, int32_t, FILL>(a); return PSAM_OK;
  }
  return PSAM_ERR_ARG;
}

template <bool FILL>
static int surface_voxels_pred(int pred_dtype, int label_dtype, const SurfArgs& a) {
  switch (pred_dtype) {
    case 0: return surface_voxels_label<int16_t, FILL>(label_dtype, a);
    case 1: return surface_voxels_label<float, FILL>(label_dtype, a);
    case 2: return surface_voxels_label<uint8_t, FILL>(label_dtype, a);
    case 3: return surface_voxels_label<int32_t, FILL>(label_dtype, a);
  }
  return PSAM_ERR_ARG;
}

static int sf_elem_size(int dtype) {
  return dtype == 0 ? 2 : (dtype == 1 || dtype == 3) ? 4 : dtype == 2 ? 1 : 0;
}

static bool sf_geometry_ok(int H, int W, int max_depth) {
  const int lim = 1 << 24;                                                // coordinates are exact as floats
  return H >= 1 && W >= 1 && max_depth >= 1 && H <= lim && W <= lim && max_depth <= lim &&
         (long long)max_depth * H * W <= 0x7fffffffLL - 16 * SURF_THREADS;
}

extern "C" int psam_surface_points(const void* pred, int pred_dtype, int pred_planes, long long pred_stride, const void* label,
                                   int label_dtype, int label_planes, long long label_stride, int H, int W, int max_depth,
                                   const int* rows, int n, int* counts, int* offsets, int* tiles, int* status, int* cursors,
                                   int* points, int cap, void* stream) {
  const int sp = sf_elem_size(pred_dtype), sl = sf_elem_size(label_dtype);
  if (!pred || !label || !rows || !counts || !offsets || !tiles || !status || !cursors || !points || sp == 0 || sl == 0 ||
      pred_planes <= 0 || label_planes <= 0 || n <= 0 || n > (1 << 28) || cap < 1 || cap > 0x7ffffffe || pred_stride < 0 ||
      label_stride < 0 || !sf_geometry_ok(H, W, max_depth) || (uintptr_t)pred % sp || (uintptr_t)label % sl)
    return PSAM_ERR_ARG;
  const long long total = (long long)max_depth * H * W, per = SURF_THREADS * SURF_UNROLL;
  if ((total + per - 1) / per * n > 0x7fffffffLL) return PSAM_ERR_ARG;
  SurfArgs a = {pred, label, pred_planes, label_planes, pred_stride, label_stride, H, W, max_depth, n, rows,
                counts, offsets, status, cursors, points, (hipStream_t)stream};
  hipLaunchKernelGGL(surface_init_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, a.s, counts, cursors, 2 * n);
  int st = surface_voxels_pred<false>(pred_dtype, label_dtype, a);
  if (st != PSAM_OK) return st;
  hipLaunchKernelGGL(surface_scan_kernel, dim3(1), dim3(SURF_THREADS), 0, a.s, rows, n, pred_planes, label_planes, max_depth,
                     (const int*)counts, cap, offsets, tiles, status);
  st = surface_voxels_pred<true>(pred_dtype, label_dtype, a);
  return st != PSAM_OK ? st : psam_launch_status();
}

extern "C" int psam_surface_dist(const int* points, const int* offsets, const int* tiles, int n, int H, int W, int max_depth,
                                 double sz, double sy, double sx, int cap, float* d2, long long* keys, void* stream) {
  const float fz = (float)sz, fy = (float)sy, fx = (float)sx;
  if (!points || !offsets || !tiles || !d2 || n <= 0 || n > (1 << 28) || cap < 1 || cap > 0x7ffffffe ||
      !sf_geometry_ok(H, W, max_depth) || !(fz > 0.f) || !(fy > 0.f) || !(fx > 0.f) || fz == __builtin_inff() ||
      fy == __builtin_inff() || fx == __builtin_inff() || (uintptr_t)keys % 8)
    return PSAM_ERR_ARG;
  const long long grid = (long long)cap / SURF_TILE + 2LL * n;            // >= the tiles of any set of segments that fits cap
  if (grid > 0x7fffffffLL) return PSAM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (max_depth > 1)
    hipLaunchKernelGGL(surface_dist_kernel<true>, dim3((unsigned)grid), dim3(SURF_TILE), 0, s, points, offsets, tiles, n, H * W, W, fz,
                       fy, fx, d2, keys);
  else
    hipLaunchKernelGGL(surface_dist_kernel<false>, dim3((unsigned)grid), dim3(SURF_TILE), 0, s, points, offsets, tiles, n, H * W, W, fz,
                       fy, fx, d2, keys);
  return psam_launch_status();
}

extern "C" int psam_surface_stats(const void* sorted, int stride, const int* counts, const int* offsets, const int* status, int n,
                                  double* out, void* stream) {
  if (!sorted || !counts || !offsets || !status || !out || n <= 0 || n > 0x7fffffff / SURF_COLS || (stride != 1 && stride != 2) ||
      (uintptr_t)sorted % 4 || (uintptr_t)out % 8)
    return PSAM_ERR_ARG;
  hipLaunchKernelGGL(surface_stats_kernel, dim3((unsigned)n), dim3(SURF_THREADS), 0, (hipStream_t)stream, (const float*)sorted, stride,
                     counts, offsets, status, out);
  return psam_launch_status();
}
