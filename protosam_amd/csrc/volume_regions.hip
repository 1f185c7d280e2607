// Connected-component clean-up of binary volumes on the device: label the 6- / 18- / 26-connected components of R volumes of
// D x H x W voxels, drop every component with fewer than min_voxels voxels (size < min_voxels, in integers) and, with keep_largest,
// keep only the largest survivor - among equally large ones the one whose first voxel comes first in raster order (z, y, x), which
// is the smallest root (ccl_uf.h): the maximum of size << 32 | ~root over the roots, the key of small_regions.hip.
// Unlike the mask generator's islands stage (small_regions.hip: "if the threshold drops every region the largest stays"), a
// min_voxels that removes every component leaves the volume EMPTY, with and without keep_largest: a clean-up that asks for at
// least min_voxels voxels must not hand back a smaller component.
//
// Voxel (r, z, y, x) of the input and of `out` lies at base + r * stride_r + z * stride_z + y * W + x, so a slice-major
// [Z, C, S, S] buffer (stride_r = S * S, stride_z = C * S * S) is read and written in place; scratch and `labels` are indexed by
// the linear index (z * H + y) * W + x inside the volume (int32: D * H * W < 2^31).
//
// labels (optional): the components of the INPUT, before any filtering, numbered 1..n per volume by the raster order of their first
// voxel - the numbering of scipy.ndimage.label. A component's first voxel is its root, so its number is 1 + the count of roots
// before it: a prefix count over the voxels, done as a two-level scan (roots per 256-voxel block, one scan of the block counts per
// volume, then the position inside the block from ballots). There is no table of components and no limit on their number.
//
// Sizes are counted per ROOT as in small_regions.hip. Scratch per volume in flight: parent and size arrays (8 bytes per voxel), 64
// bytes of accumulators and, with labels, one int32 per 256-voxel block. The entry walks the R volumes in chunks of `chunk` and
// only enqueues; blockIdx.z = volume of the chunk. One chain per chunk, ordered by the stream alone (no flags, no waits between
// workgroups; the data-dependent loops are uf_find / uf_union, which end because parents only decrease, and the per-root loop of a
// wave's aggregation, at most 64 turns):
//   clear | init | merge | flatten + sizes | roots: largest key, counts | ranks: scan of block counts, numbers at the roots (only
//   with labels) | rewrite + box (+ labels) | finalize
// The rewrite reads scratch only, never the source: out == vol is allowed.
#include "common.h"
#include "ccl_uf.h"
#include "ccl_uf3d.h"

#define VR_ACC 16         // int32 words of a volume's accumulators (64 bytes, the u64 key first)
#define VR_ROWS 16        // rows of one plane a wave of the rewrite walks with its box and count in registers
#define VR_MAX_Z 65535
#define VR_SCAN_PER 16    // block counts one thread of the scan sums serially: 4096 per turn of the workgroup
#define VR_INFO 12

// accumulators of one volume: words 0-1 = the largest component's key (u64), then
enum { VR_NCOMP = 2, VR_NSURV = 3, VR_VOX_IN = 4, VR_VOX_OUT = 5, VR_MINZ = 6, VR_MINY = 7, VR_MINX = 8, VR_MAXZ = 9, VR_MAXY = 10,
       VR_MAXX = 11 };

struct VrChunk {
  int* parent;   // [chunk][n]
  int* size;     // [chunk][n]     voxels of the component whose root is this voxel
  int* acc;      // [chunk][VR_ACC]
  int* bsum;     // [chunk][nblk]  roots per 256-voxel block, then their exclusive scan (only with labels)
};

struct VrGeom {
  int D, H, W, nxb;
  long long stride_r, stride_z;
};

// a row kernel's block: 256 voxels of row `row` = z * H + y
__device__ __forceinline__ void vr_row_block(int nxb, int* x, int* row) {
  const int by = blockIdx.x / nxb;
  *x = (blockIdx.x - by * nxb) * 256 + threadIdx.x;
  *row = by;
}

__global__ __launch_bounds__(256) void vr_clear_kernel(int* __restrict__ acc, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count * VR_ACC) return;
  const int k = i % VR_ACC;
  acc[i] = (k >= VR_MINZ && k <= VR_MINX) ? 0x7fffffff : (k >= VR_MAXZ && k <= VR_MAXX) ? -1 : 0;
}

__global__ __launch_bounds__(256) void vr_init_kernel(const uint8_t* __restrict__ src, VrGeom g, VrChunk c) {
  const size_t n = (size_t)g.D * g.H * g.W;
  int* parent = c.parent + blockIdx.z * n;
  int* size = c.size + blockIdx.z * n;
  int x, row;
  vr_row_block(g.nxb, &x, &row);
  const int z = row / g.H, y = row - z * g.H;
  const bool fg = x < g.W && src[blockIdx.z * g.stride_r + z * g.stride_z + (long long)y * g.W + x] != 0;
  const int par = uf_run_start(fg, x, row, g.W, threadIdx.x & 63);
  if (x >= g.W) return;
  const size_t p = (size_t)row * g.W + x;
  parent[p] = par;
  size[p] = 0;
}

// (foreground is read from the parent array the init kernel wrote: parent >= 0, and a union never makes a parent negative)
template <int CONN>
__global__ __launch_bounds__(256) void vr_merge_kernel(VrGeom g, VrChunk c) {
  int* parent = c.parent + blockIdx.z * ((size_t)g.D * g.H * g.W);
  int x, row;
  vr_row_block(g.nxb, &x, &row);
  if (x >= g.W) return;
  const int z = row / g.H, y = row - z * g.H;
  const int p = row * g.W + x;
  if (parent[p] < 0) return;
  uf3_merge_voxel<CONN>(parent, p, x, y, z, g.W, g.H, (threadIdx.x & 63) == 0, [&](int q) { return parent[q] >= 0; });
}

// flatten + sizes: as sr_flatten_area_kernel - parent[i] := the root of i, and the root's count grows by the number of lanes of the
// wave that found it, one atomic per (wave, root)
__global__ __launch_bounds__(256) void vr_flatten_size_kernel(int n, VrChunk c) {
  int* parent = c.parent + blockIdx.z * (size_t)n;
  int* size = c.size + blockIdx.z * (size_t)n;
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
    if (lane == leader) atomicAdd(&size[R], __popcll(same));
  }
}

__device__ __forceinline__ int vr_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one pass over the roots: components found, components at or above min_voxels, voxels in, the largest component's key and, with
// labels, the roots of every 256-voxel block (level one of the scan)
template <bool RANKS>
__global__ __launch_bounds__(256) void vr_roots_kernel(int n, int nblk, long long min_voxels, VrChunk c) {
  const int* parent = c.parent + blockIdx.z * (size_t)n;
  const int* size = c.size + blockIdx.z * (size_t)n;
  int* acc = c.acc + blockIdx.z * VR_ACC;
  __shared__ int wroots[4];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool root = i < (unsigned)n && parent[i] == (int)i;
  const unsigned long long rm = __ballot(root);
  if (RANKS) {
    if (lane == 0) wroots[threadIdx.x >> 6] = __popcll(rm);
    __syncthreads();
    if (threadIdx.x == 0) c.bsum[blockIdx.z * (size_t)nblk + blockIdx.x] = wroots[0] + wroots[1] + wroots[2] + wroots[3];
  }
  if (!rm) return;                                 // (wave-uniform, after the block's barrier)
  const int a = root ? size[i] : 0;
  const unsigned long long sm = __ballot(root && (long long)a >= min_voxels);
  unsigned long long key = root ? (((unsigned long long)(unsigned)a << 32) | (unsigned long long)(~i)) : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  const int vox = vr_wave_sum(a);
  if (lane == 0) {
    atomicAdd(&acc[VR_NCOMP], __popcll(rm));
    if (sm) atomicAdd(&acc[VR_NSURV], __popcll(sm));
    atomicAdd(&acc[VR_VOX_IN], vox);
    unsigned long long* best = (unsigned long long*)acc;
    if (key > *(volatile unsigned long long*)best) atomicMax(best, key);
  }
}

// level two of the scan: bsum := its exclusive prefix sum, one workgroup per volume walking the counts 4096 at a time with a carry
__global__ __launch_bounds__(256) void vr_scan_kernel(int nblk, VrChunk c) {
  int* bsum = c.bsum + blockIdx.z * (size_t)nblk;
  __shared__ int wtot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;                                   // (the same in every thread)
  for (int base = 0; base < nblk; base += 256 * VR_SCAN_PER) {   // (uniform bounds: every thread reaches both barriers)
    const int i0 = base + threadIdx.x * VR_SCAN_PER;             // a thread owns VR_SCAN_PER consecutive counts
    int loc[VR_SCAN_PER];
    int v = 0;
#pragma unroll
    for (int k = 0; k < VR_SCAN_PER; ++k) {
      loc[k] = i0 + k < nblk ? bsum[i0 + k] : 0;
      v += loc[k];
    }
    int s = v;                                     // inclusive scan of the threads' sums inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(s, o, 64);
      if (lane >= o) s += t;
    }
    if (lane == 63) wtot[wave] = s;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int t = wtot[w];
      if (w < wave) before += t;
      total += t;
    }
    int run = carry + before + s - v;
#pragma unroll
    for (int k = 0; k < VR_SCAN_PER; ++k) {
      if (i0 + k < nblk) bsum[i0 + k] = run;
      run += loc[k];
    }
    carry += total;
    __syncthreads();                               // (wtot is rewritten by the next turn)
  }
}

// the number of a component at its root: 1 + roots before it = scanned block count + roots of the earlier waves of the block +
// roots of the lower lanes. Voxels that are no root are filled from their root's entry by the rewrite, a later launch.
__global__ __launch_bounds__(256) void vr_rank_kernel(int n, int nblk, int* __restrict__ labels, VrChunk c) {
  const int* parent = c.parent + blockIdx.z * (size_t)n;
  labels += blockIdx.z * (size_t)n;
  __shared__ int wroots[4];
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool root = i < (unsigned)n && parent[i] == (int)i;
  const unsigned long long rm = __ballot(root);
  if (lane == 0) wroots[wave] = __popcll(rm);
  __syncthreads();
  if (!root) return;
  int before = c.bsum[blockIdx.z * (size_t)nblk + blockIdx.x];
  for (int w = 0; w < wave; ++w) before += wroots[w];
  before += __popcll(rm & ((1ull << lane) - 1ull));
  labels[i] = before + 1;
}

// rewrite + box: out = 1 where the voxel's component stays, else 0, written everywhere; the count and the box of `out`; with
// labels, every voxel that is no root takes its root's number (background 0). One wave walks a 64-voxel-wide strip of VR_ROWS rows
// of one plane with the sums in registers: seven atomics per (wave, strip) that holds a kept voxel. Reads scratch only.
template <bool LABELS>
__global__ __launch_bounds__(256) void vr_rewrite_kernel(uint8_t* __restrict__ out, VrGeom g, int strips, long long min_voxels,
                                                         int keep_largest, int* __restrict__ labels, VrChunk c) {
  const size_t n = (size_t)g.D * g.H * g.W;
  const int* parent = c.parent + blockIdx.z * n;
  const int* size = c.size + blockIdx.z * n;
  int* acc = c.acc + blockIdx.z * VR_ACC;
  if (LABELS) labels += blockIdx.z * n;
  int x, ps;
  vr_row_block(g.nxb, &x, &ps);
  const int z = ps / strips, strip = ps - z * strips;
  const int lane = threadIdx.x & 63;
  const unsigned long long best = *(const unsigned long long*)acc;            // (written by vr_roots_kernel, an earlier launch)
  const int best_root = (int)~(unsigned)(best & 0xffffffffull);
  const bool best_stays = (long long)(best >> 32) >= min_voxels;
  out += blockIdx.z * g.stride_r + z * g.stride_z;
  const int y0 = strip * VR_ROWS, y1 = min(y0 + VR_ROWS, g.H);
  int cnt = 0, mnx = 0x7fffffff, mxx = -1, mny = 0x7fffffff, mxy = -1;        // (wave-uniform)
  for (int y = y0; y < y1; ++y) {
    bool keep = false;
    if (x < g.W) {
      const size_t p = ((size_t)z * g.H + y) * g.W + x;
      const int r = parent[p];
      if (r >= 0) keep = keep_largest ? (best_stays && r == best_root) : (long long)size[r] >= min_voxels;
      out[(size_t)y * g.W + x] = keep;
      if (LABELS && (size_t)r != p) labels[p] = r >= 0 ? labels[r] : 0;       // (labels[r]: a root's entry, which nobody writes here)
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
    atomicAdd(&acc[VR_VOX_OUT], cnt);
    atomicMin(&acc[VR_MINZ], z);
    atomicMin(&acc[VR_MINY], mny);
    atomicMin(&acc[VR_MINX], mnx);
    atomicMax(&acc[VR_MAXZ], z);
    atomicMax(&acc[VR_MAXY], mxy);
    atomicMax(&acc[VR_MAXX], mxx);
  }
}

__global__ __launch_bounds__(256) void vr_finalize_kernel(const int* __restrict__ acc, int count, long long min_voxels,
                                                          int keep_largest, long long* __restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int* a = acc + (size_t)i * VR_ACC;
  long long* o = info + (size_t)i * VR_INFO;
  const unsigned long long best = *(const unsigned long long*)a;
  const bool any = a[VR_NCOMP] != 0, empty = a[VR_VOX_OUT] == 0;
  o[0] = a[VR_NCOMP];
  o[1] = keep_largest ? (a[VR_NSURV] != 0 ? 1 : 0) : a[VR_NSURV];
  o[2] = a[VR_VOX_IN];
  o[3] = a[VR_VOX_OUT];
  o[4] = any ? (long long)(best >> 32) : 0;
  o[5] = any ? (long long)(int)~(unsigned)(best & 0xffffffffull) : -1;
  for (int k = 0; k < 6; ++k) o[6 + k] = empty ? -1 : a[VR_MINZ + k];
}

static bool vr_shape_ok(int D, int H, int W, int chunk) {
  // (the row kernels launch whole 256-voxel blocks per row: their thread count has to fit the launch's 32 bits as well)
  if (D <= 0 || H <= 0 || W <= 0 || chunk < 1) return false;
  const long long rows = (long long)D * H;
  return rows * W < 0x80000000LL && (long long)((W + 255) / 256) * rows * 256 <= 0xffffffffLL;
}

static long long vr_scratch_bytes(int D, int H, int W, int chunk, bool labels) {
  const long long n = (long long)D * H * W;
  return (long long)chunk * (n * 8 + VR_ACC * 4 + (labels ? ((n + 255) / 256) * 4 : 0));
}

extern "C" int psam_volume_regions(const void* vol, int R, int D, int H, int W, long long stride_r, long long stride_z,
                                   int connectivity, long long min_voxels, int keep_largest, int chunk, void* out, long long* info,
                                   int* labels, void* scratch, long long scratch_bytes, void* stream) {
  if (R < 0 || !vr_shape_ok(D, H, W, chunk)) return PSAM_ERR_ARG;
  if (connectivity != 6 && connectivity != 18 && connectivity != 26) return PSAM_ERR_ARG;
  if (min_voxels < 0 || (keep_largest != 0 && keep_largest != 1)) return PSAM_ERR_ARG;
  const long long plane = (long long)H * W;
  if (stride_z < plane || stride_r < plane) return PSAM_ERR_ARG;
  if (R == 0) return PSAM_OK;
  if (!vol || !out || !info || !scratch || ((uintptr_t)scratch & 7) ||
      scratch_bytes < vr_scratch_bytes(D, H, W, chunk, labels != nullptr))
    return PSAM_ERR_ARG;
  const int n = (int)(plane * D);
  const int nblk = (int)(((long long)n + 255) / 256);
  const int strips = (H + VR_ROWS - 1) / VR_ROWS;
  hipStream_t s = (hipStream_t)stream;
  VrGeom g;
  g.D = D; g.H = H; g.W = W; g.nxb = (W + 255) / 256;
  g.stride_r = stride_r; g.stride_z = stride_z;
  VrChunk c;
  c.parent = (int*)scratch;
  c.size = c.parent + (size_t)chunk * n;
  c.acc = c.size + (size_t)chunk * n;
  c.bsum = c.acc + (size_t)chunk * VR_ACC;
  const int step = chunk < VR_MAX_Z ? chunk : VR_MAX_Z;   // (grid.z; a larger chunk only leaves scratch unused)
  const dim3 B(256);
  for (int lo = 0; lo < R; lo += step) {
    const int k = R - lo < step ? R - lo : step;
    const unsigned Z = (unsigned)k;
    const uint8_t* src = (const uint8_t*)vol + (long long)lo * stride_r;
    uint8_t* dst = (uint8_t*)out + (long long)lo * stride_r;
    int* lab = labels ? labels + (size_t)lo * n : nullptr;
    const dim3 rows((unsigned)g.nxb * (unsigned)D * (unsigned)H, 1, Z), flat((unsigned)nblk, 1, Z);
    const dim3 strip_grid((unsigned)g.nxb * (unsigned)D * (unsigned)strips, 1, Z);
    hipLaunchKernelGGL(vr_clear_kernel, dim3((unsigned)((k * VR_ACC + 255) / 256)), B, 0, s, c.acc, k);
    hipLaunchKernelGGL(vr_init_kernel, rows, B, 0, s, src, g, c);
    if (connectivity == 6) hipLaunchKernelGGL(vr_merge_kernel<6>, rows, B, 0, s, g, c);
    else if (connectivity == 18) hipLaunchKernelGGL(vr_merge_kernel<18>, rows, B, 0, s, g, c);
    else hipLaunchKernelGGL(vr_merge_kernel<26>, rows, B, 0, s, g, c);
    hipLaunchKernelGGL(vr_flatten_size_kernel, flat, B, 0, s, n, c);
    if (lab) {
      hipLaunchKernelGGL(vr_roots_kernel<true>, flat, B, 0, s, n, nblk, min_voxels, c);
      hipLaunchKernelGGL(vr_scan_kernel, dim3(1, 1, Z), B, 0, s, nblk, c);
      hipLaunchKernelGGL(vr_rank_kernel, flat, B, 0, s, n, nblk, lab, c);
      hipLaunchKernelGGL(vr_rewrite_kernel<true>, strip_grid, B, 0, s, dst, g, strips, min_voxels, keep_largest, lab, c);
    } else {
      hipLaunchKernelGGL(vr_roots_kernel<false>, flat, B, 0, s, n, nblk, min_voxels, c);
      hipLaunchKernelGGL(vr_rewrite_kernel<false>, strip_grid, B, 0, s, dst, g, strips, min_voxels, keep_largest, lab, c);
    }
    hipLaunchKernelGGL(vr_finalize_kernel, dim3((unsigned)((k + 255) / 256)), B, 0, s, (const int*)c.acc, k, min_voxels,
                       keep_largest, info + (size_t)lo * VR_INFO);
  }
  return psam_launch_status();
}
