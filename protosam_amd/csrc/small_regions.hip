// Small-region removal for a batch of masks on the device: remove_small_regions(mask, t, "holes") followed by
// remove_small_regions(., t, "islands") (segment_anything/utils/amg.py:267-291, the stage of automatic_mask_generator.py:332-380),
// bit for bit, for m masks per call, without a table of regions and therefore without a limit on their number.
//
// Per mask:
//   holes   : label the 8-connected regions of the complement; every region with (double)area < t is filled (the outer background
//             too when it is that small); changed_holes = such a region exists.
//   islands : on the hole-filled mask, label the 8-connected regions of the foreground; if none is below t nothing changes;
//             otherwise every region below t is dropped, and if that drops all of them the largest stays - among equal largest the
//             one whose first pixel comes first in raster order, which is the smallest root (ccl_uf.h): the maximum of
//             area << 32 | ~root over the roots. changed_islands = a region below t exists (also in the keep-largest case).
//   out     : the new mask {0, 1}; info = {changed_holes, changed_islands, area of out, 0}; box = XYXY min / max of out, or
//             {0, 0, 0, 0} for an empty mask (batched_mask_to_box); score = 1.0f if neither flag is set, else 0.0f - int32 boxes
//             and fp32 scores as psam_box_nms reads them.
//
// Areas are counted per ROOT: after the union-find every pixel finds its final root, and the flatten pass adds wave-aggregated
// counts (a 64-pixel segment nearly always holds one root) into an int32 array at the root's pixel index. Scratch is that array
// and the parent array, 8 bytes per pixel and mask in flight, plus 64 bytes of accumulators per mask; the entry walks the m masks
// in chunks of `chunk` and enqueues every launch, no host wait in between.
//
// A chunk is eleven launches with blockIdx.z = mask of the chunk, ordered by the stream alone (no flags, no waits between
// workgroups; the only data-dependent loops are uf_find / uf_union and the per-root loop of a wave's aggregation, at most 64 turns):
//   clear | holes: init, merge, flatten + area, rewrite | islands: init, merge, flatten + area, roots, rewrite | finalize
// Integer work throughout; the one floating comparison is (double)area < t.
#include "common.h"
#include "ccl_uf.h"

#define SR_ACC 16         // int32 words of a mask's accumulators (64 bytes, the u64 key first)
#define SR_ROWS 16        // rows one wave of the last rewrite walks with its box and area in registers
#define SR_MAX_Z 65535

// accumulators of one mask: words 0-1 = the largest island's key (u64), then
enum { SR_SMALL_H = 2, SR_SMALL_I = 3, SR_BIG_I = 4, SR_AREA = 5, SR_MINX = 6, SR_MINY = 7, SR_MAXX = 8, SR_MAXY = 9 };

struct SrChunk {
  int* parent;   // [chunk][n]
  int* area;     // [chunk][n]  pixels of the region whose root is this pixel
  int* acc;      // [chunk][SR_ACC]
};

__device__ __forceinline__ void sr_row_block(int nxb, int* x, int* y) {
  const int by = blockIdx.x / nxb;
  *x = (blockIdx.x - by * nxb) * 256 + threadIdx.x;
  *y = by;
}

__device__ __forceinline__ void sr_flag(int* word) {   // one lane: set a flag that other waves may have set already
  if (*(volatile int*)word == 0) atomicOr(word, 1);
}

__global__ __launch_bounds__(256) void sr_clear_kernel(int* __restrict__ acc, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count * SR_ACC) return;
  const int k = i % SR_ACC;
  acc[i] = (k == SR_MINX || k == SR_MINY) ? 0x7fffffff : (k == SR_MAXX || k == SR_MAXY) ? -1 : 0;
}

// INV: the foreground of the labelling is the complement of `src` (holes)
template <bool INV>
__global__ __launch_bounds__(256) void sr_init_kernel(const uint8_t* __restrict__ src, int H, int W, int nxb, SrChunk c) {
  const size_t n = (size_t)H * W;
  src += blockIdx.z * n;
  int* parent = c.parent + blockIdx.z * n;
  int* area = c.area + blockIdx.z * n;
  int x, y;
  sr_row_block(nxb, &x, &y);
  const size_t p = (size_t)y * W + x;
  const bool fg = x < W && ((src[p] != 0) != INV);
  const int par = uf_run_start(fg, x, y, W, threadIdx.x & 63);
  if (x >= W) return;
  parent[p] = par;
  area[p] = 0;
}

template <bool INV>
__global__ __launch_bounds__(256) void sr_merge_kernel(const uint8_t* __restrict__ src, int H, int W, int nxb, SrChunk c) {
  const size_t n = (size_t)H * W;
  src += blockIdx.z * n;
  int* parent = c.parent + blockIdx.z * n;
  int x, y;
  sr_row_block(nxb, &x, &y);
  if (x >= W) return;
  const int p = y * W + x;
  if ((src[p] != 0) == INV) return;
  uf_merge_pixel(parent, p, x, y, W, (threadIdx.x & 63) == 0, [&](int q) { return (src[q] != 0) != INV; });
}

// flatten + area: parent[i] := the root of i (the roots are final after the merge kernel; a thread that meets a parent another
// thread has already flattened reads the old ancestor or the root, both on the path to the same root), and the root's count grows
// by the number of lanes of the wave that found it - one atomic per (wave, root).
__global__ __launch_bounds__(256) void sr_flatten_area_kernel(int n, SrChunk c) {
  int* parent = c.parent + blockIdx.z * (size_t)n;
  int* area = c.area + blockIdx.z * (size_t)n;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int r = -1;
  if (i < (unsigned)n) {
    const int p0 = parent[i];
    if (p0 >= 0) {
      r = uf_find(parent, (int)i);
      if (r != p0) parent[i] = r;
    }
  }
  unsigned long long todo = __ballot(r >= 0);
  while (todo) {                                   // (wave-uniform: at most 64 turns, one per distinct root of the wave)
    const int leader = __ffsll((long long)todo) - 1;
    const int R = __shfl(r, leader, 64);
    const unsigned long long same = __ballot(r == R);
    todo &= ~same;
    if (lane == leader) atomicAdd(&area[R], __popcll(same));
  }
}

// holes: out = src | (complement region below the threshold); flags the mask when a pixel was filled
__global__ __launch_bounds__(256) void sr_fill_kernel(const uint8_t* src, uint8_t* out, int n, double thr,
                                                      SrChunk c) {
  src += blockIdx.z * (size_t)n;
  out += blockIdx.z * (size_t)n;
  const int* parent = c.parent + blockIdx.z * (size_t)n;
  const int* area = c.area + blockIdx.z * (size_t)n;
  int* acc = c.acc + blockIdx.z * SR_ACC;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  bool filled = false;
  if (i < (unsigned)n) {
    uint8_t v = src[i] != 0;
    if (!v) {
      filled = (double)area[parent[i]] < thr;      // a complement pixel always has a root
      v = filled;
    }
    out[i] = v;
  }
  if (__ballot(filled) && (threadIdx.x & 63) == 0) sr_flag(&acc[SR_SMALL_H]);
}

// islands: one pass over the roots -> is there a region below the threshold, is there one at or above it, and the largest
__global__ __launch_bounds__(256) void sr_roots_kernel(int n, double thr, SrChunk c) {
  const int* parent = c.parent + blockIdx.z * (size_t)n;
  const int* area = c.area + blockIdx.z * (size_t)n;
  int* acc = c.acc + blockIdx.z * SR_ACC;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const bool root = i < (unsigned)n && parent[i] == (int)i;
  if (!__ballot(root)) return;                     // (wave-uniform)
  const int a = root ? area[i] : 0;
  const bool small = root && (double)a < thr;
  unsigned long long key = root ? (((unsigned long long)(unsigned)a << 32) | (unsigned long long)(~i)) : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  const bool any_small = __ballot(small) != 0ull, any_big = __ballot(root && !small) != 0ull;
  if ((threadIdx.x & 63) == 0) {
    if (any_small) sr_flag(&acc[SR_SMALL_I]);
    if (any_big) sr_flag(&acc[SR_BIG_I]);
    unsigned long long* best = (unsigned long long*)acc;
    if (key > *(volatile unsigned long long*)best) atomicMax(best, key);
  }
}

// islands: out &= (region at or above the threshold, or the largest one when none is), and the new mask's area and box. One wave
// walks a 64-pixel-wide strip of SR_ROWS rows with the sums in registers: five atomics per (wave, strip) that holds a pixel.
__global__ __launch_bounds__(256) void sr_drop_kernel(uint8_t* __restrict__ out, int H, int W, int nxb, double thr, SrChunk c) {
  const size_t n = (size_t)H * W;
  out += blockIdx.z * n;
  const int* parent = c.parent + blockIdx.z * n;
  const int* area = c.area + blockIdx.z * n;
  int* acc = c.acc + blockIdx.z * SR_ACC;
  int x, strip;
  sr_row_block(nxb, &x, &strip);
  const int lane = threadIdx.x & 63;
  const bool any_small = acc[SR_SMALL_I] != 0, any_big = acc[SR_BIG_I] != 0;   // (written by sr_roots_kernel, an earlier launch)
  const int best_root = (int)~(unsigned)(*(const unsigned long long*)acc & 0xffffffffull);
  const int y0 = strip * SR_ROWS, y1 = min(y0 + SR_ROWS, H);
  int cnt = 0, mnx = 0x7fffffff, mxx = -1, mny = 0x7fffffff, mxy = -1;        // (wave-uniform)
  for (int y = y0; y < y1; ++y) {
    bool keep = false;
    if (x < W) {
      const size_t p = (size_t)y * W + x;
      keep = out[p] != 0;
      if (keep && any_small) {
        const int r = parent[p];
        keep = any_big ? !((double)area[r] < thr) : r == best_root;
        if (!keep) out[p] = 0;
      }
    }
    const unsigned long long m = __ballot(keep);
    if (m) {
      const int x0 = x - lane;
      cnt += __popcll(m);
      mnx = min(mnx, x0 + __ffsll((long long)m) - 1);
      mxx = max(mxx, x0 + 63 - __clzll((long long)m));
      mny = min(mny, y);
      mxy = y;
    }
  }
  if (cnt && lane == 0) {
    atomicAdd(&acc[SR_AREA], cnt);
    atomicMin(&acc[SR_MINX], mnx);
    atomicMin(&acc[SR_MINY], mny);
    atomicMax(&acc[SR_MAXX], mxx);
    atomicMax(&acc[SR_MAXY], mxy);
  }
}

__global__ __launch_bounds__(256) void sr_finalize_kernel(const int* __restrict__ acc, int count, int* __restrict__ boxes,
                                                          float* __restrict__ scores, int* __restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int* a = acc + (size_t)i * SR_ACC;
  const bool empty = a[SR_AREA] == 0;
  const int ch = a[SR_SMALL_H] != 0, ci = a[SR_SMALL_I] != 0;
  info[i * 4 + 0] = ch;
  info[i * 4 + 1] = ci;
  info[i * 4 + 2] = a[SR_AREA];
  info[i * 4 + 3] = 0;
  boxes[i * 4 + 0] = empty ? 0 : a[SR_MINX];
  boxes[i * 4 + 1] = empty ? 0 : a[SR_MINY];
  boxes[i * 4 + 2] = empty ? 0 : a[SR_MAXX];
  boxes[i * 4 + 3] = empty ? 0 : a[SR_MAXY];
  scores[i] = (ch || ci) ? 0.0f : 1.0f;
}

static bool sr_shape_ok(int H, int W, int chunk) {
  // (the row kernels launch whole 256-pixel blocks per row: their thread count has to fit the launch's 32 bits as well)
  return H > 0 && W > 0 && chunk >= 1 && (long long)H * W <= 0x7fffffffLL && (long long)((W + 255) / 256) * H * 256 <= 0xffffffffLL;
}

static long long sr_scratch_bytes(int H, int W, int chunk) {
  return (long long)chunk * ((long long)H * W * 8 + SR_ACC * 4);
}

extern "C" int psam_small_regions_workspace(int H, int W, int chunk, long long* bytes) {
  if (!sr_shape_ok(H, W, chunk) || !bytes) return PSAM_ERR_ARG;
  *bytes = sr_scratch_bytes(H, W, chunk);
  return PSAM_OK;
}

extern "C" int psam_small_regions(const void* masks, int m, int H, int W, double area_thresh, int chunk, void* out, int* boxes,
                                  float* scores, int* info, void* scratch, long long scratch_bytes, void* stream) {
  if (m < 0 || !sr_shape_ok(H, W, chunk) || area_thresh != area_thresh) return PSAM_ERR_ARG;
  if (m == 0) return PSAM_OK;
  if (!masks || !out || !boxes || !scores || !info || !scratch || ((uintptr_t)scratch & 7) ||
      scratch_bytes < sr_scratch_bytes(H, W, chunk))
    return PSAM_ERR_ARG;
  const int n = H * W;
  const int nxb = (W + 255) / 256;
  const int strips = (H + SR_ROWS - 1) / SR_ROWS;
  hipStream_t s = (hipStream_t)stream;
  SrChunk c;
  c.parent = (int*)scratch;
  c.area = c.parent + (size_t)chunk * n;
  c.acc = c.area + (size_t)chunk * n;
  const int step = chunk < SR_MAX_Z ? chunk : SR_MAX_Z;   // (grid.z; a larger chunk only leaves scratch unused)
  const dim3 B(256);
  for (int lo = 0; lo < m; lo += step) {
    const int k = m - lo < step ? m - lo : step;
    const unsigned Z = (unsigned)k;
    const uint8_t* src = (const uint8_t*)masks + (size_t)lo * n;
    uint8_t* dst = (uint8_t*)out + (size_t)lo * n;
    const dim3 rows((unsigned)nxb * (unsigned)H, 1, Z), flat((unsigned)(((long long)n + 255) / 256), 1, Z);
    hipLaunchKernelGGL(sr_clear_kernel, dim3((unsigned)((k * SR_ACC + 255) / 256)), B, 0, s, c.acc, k);
    hipLaunchKernelGGL(sr_init_kernel<true>, rows, B, 0, s, src, H, W, nxb, c);
    hipLaunchKernelGGL(sr_merge_kernel<true>, rows, B, 0, s, src, H, W, nxb, c);
    hipLaunchKernelGGL(sr_flatten_area_kernel, flat, B, 0, s, n, c);
    hipLaunchKernelGGL(sr_fill_kernel, flat, B, 0, s, src, dst, n, area_thresh, c);
    hipLaunchKernelGGL(sr_init_kernel<false>, rows, B, 0, s, (const uint8_t*)dst, H, W, nxb, c);
    hipLaunchKernelGGL(sr_merge_kernel<false>, rows, B, 0, s, (const uint8_t*)dst, H, W, nxb, c);
    hipLaunchKernelGGL(sr_flatten_area_kernel, flat, B, 0, s, n, c);
    hipLaunchKernelGGL(sr_roots_kernel, flat, B, 0, s, n, area_thresh, c);
    hipLaunchKernelGGL(sr_drop_kernel, dim3((unsigned)nxb * (unsigned)strips, 1, Z), B, 0, s, dst, H, W, nxb, area_thresh, c);
    hipLaunchKernelGGL(sr_finalize_kernel, dim3((unsigned)((k + 255) / 256)), B, 0, s, (const int*)c.acc, k, boxes + (size_t)lo * 4,
                       scores + lo, info + (size_t)lo * 4);
  }
  return psam_launch_status();
}
