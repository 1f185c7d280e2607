// Uncompressed COCO run-length encoding of binary masks on the device, and its inverse. Replaces the host side of the
// generator's RLE output: `mask_to_rle_pytorch` / `rle_to_mask` (utils/amg.py:107-149), which the reference runs on the
// GPU with a transpose, a flatten and a `nonzero` per mask, and which this project ran on a host copy of every mask.
//
// Format. Pixels are walked column-major, p = x * H + y; `counts` alternates zero-run and one-run lengths and starts with a
// zero-run (a set first pixel gives a leading 0); any non-zero byte is set; a mask has at most H * W + 1 counts.
//
// Encode. Pixel (y, x) STARTS a run iff p == 0, or y > 0 and m[y][x] != m[y-1][x], or y == 0 and m[0][x] != m[H-1][x-1].
// The starts, ranked by p, give the counts as differences; the last run ends at H * W. So the mask is never transposed:
// lanes run along x (every row read is coalesced; 4 columns per lane as one 32-bit load where W % 4 == 0 and the base is
// 4-byte aligned, bytes otherwise) and a lane compares each row with the one above. The mask is cut into CELLS of one
// column x RLE_SEG rows; in column-major cell order (column outer, segment inner) positions increase, so
//   pass 1 (rle_pass_kernel<VEC, false>): per cell, the number of starts and the position of its last start (-1: none);
//   pass 2 (rle_scan_kernel, one workgroup per mask): exclusive sum of the numbers (the rank of a cell's first start) and
//           exclusive running maximum of the positions (the start that precedes the cell), in place; the mask's number of
//           starts and its last start go to the two words after the cells, the number of counts to `totals`;
//   pass 3 (rle_pass_kernel<VEC, true>): the same walk; the start at p with rank r > 0 closes the run before it,
//           counts[base + r - 1 + lead] = p - previous start; one lane writes the leading 0 and the final run.
// No atomics anywhere: every count has one writer and its index is computed, so the output is the same bits on every run.
// Streaming kernels: a mask is read twice (passes 1 and 3), the cells (8 bytes per 64 pixels) are written, scanned and read.
//
// Decode. One lane per output pixel (row-major, coalesced byte stores): a binary search of p in the running sum of the
// mask's counts; the parity of the run found is the pixel. A pixel past the sum of a short list is 0.
#include "common.h"

#define RLE_SEG 64            // rows of a cell
#define RLE_WAVES 4           // row segments of a pass-1/3 workgroup, one per wave
#define RLE_SCAN_T 1024       // lanes of the pass-2 workgroup
#define RLE_MAX_GRID_Y 65535

// 0x80 in every non-zero byte of w (no carries between bytes)
__device__ __forceinline__ uint32_t rle_set4(uint32_t w) {
  return (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
}

// the set-ness of VEC consecutive pixels as 0x80 per set byte
template <int VEC>
__device__ __forceinline__ uint32_t rle_load(const uint8_t* __restrict__ p) {
  if constexpr (VEC == 4) return rle_set4(*reinterpret_cast<const uint32_t*>(p));
  else return *p ? 0x80u : 0u;
}

template <int VEC, bool WRITE>
__global__ __launch_bounds__(WAVE * RLE_WAVES) void rle_pass_kernel(const uint8_t* __restrict__ masks, int H, int W, int nseg,
                                                                    int nstrip, long long per, int* __restrict__ cells,
                                                                    const long long* __restrict__ offsets,
                                                                    int* __restrict__ counts) {
  const int strip = (int)(blockIdx.x % (unsigned)nstrip), grp = (int)(blockIdx.x / (unsigned)nstrip);
  const int z = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = grp * RLE_WAVES + wave;
  const long long xl = ((long long)strip * WAVE + lane) * VEC;
  if (s >= nseg || xl >= W) return;                                 // (no barrier in this kernel)
  const int x0 = (int)xl;
  const long long HW = (long long)H * W;
  const uint8_t* __restrict__ m = masks + (long long)z * HW;
  int* __restrict__ cz = cells + (long long)z * per;
  const long long ncell = (long long)W * nseg;
  const int y0 = s * RLE_SEG, y1 = min(H, y0 + RLE_SEG);

  // the pixels that precede the lane's columns at row y0: the row above, or, for y0 == 0, the last row one column to the left
  uint32_t prev;
  if (y0 > 0) {
    prev = rle_load<VEC>(m + (long long)(y0 - 1) * W + x0);
  } else {
    const uint8_t* __restrict__ bottom = m + (long long)(H - 1) * W;
    const uint32_t left = x0 > 0 ? (bottom[x0 - 1] ? 0x80u : 0u) : (m[0] ? 0u : 0x80u);   // p == 0 always starts a run
    if constexpr (VEC == 4) prev = (rle_load<4>(bottom + x0) << 8) | left;
    else prev = left;
  }

  int num[VEC], pos[VEC];                                           // COUNT: starts / last start; WRITE: rank / previous start
  long long base = 0, end = 0;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    if constexpr (WRITE) {
      const long long c = (long long)(x0 + j) * nseg + s;
      num[j] = cz[c];
      pos[j] = cz[ncell + c];
    } else {
      num[j] = 0;
      pos[j] = -1;
    }
  }
  if constexpr (WRITE) {
    base = offsets[z] + (m[0] ? 1 : 0);
    end = offsets[z + 1];
  }

#pragma unroll 8
  for (int y = y0; y < y1; ++y) {
    const uint32_t cur = rle_load<VEC>(m + (long long)y * W + x0);
    const uint32_t d = cur ^ prev;
    prev = cur;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if ((d >> (8 * j + 7)) & 1u) {
        const int p = (x0 + j) * H + y;                             // < H * W <= 2^31 - 1
        if constexpr (WRITE) {
          const long long idx = base + num[j] - 1;
          if (num[j] > 0 && idx < end) counts[idx] = p - pos[j];
        }
        num[j] += 1;
        pos[j] = p;
      }
    }
  }

  if constexpr (WRITE) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {                      // (segment 0, column 0: never returned above)
      const int nstart = cz[2 * ncell], last = cz[2 * ncell + 1];
      if (m[0] && offsets[z] < end) counts[offsets[z]] = 0;
      const long long idx = base + nstart - 1;
      if (idx < end) counts[idx] = (int)(HW - last);
    }
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const long long c = (long long)(x0 + j) * nseg + s;
      cz[c] = num[j];
      cz[ncell + c] = pos[j];
    }
  }
}

__global__ __launch_bounds__(RLE_SCAN_T) void rle_scan_kernel(const uint8_t* __restrict__ masks, long long HW, long long ncell,
                                                              long long per, int* __restrict__ cells,
                                                              long long* __restrict__ totals) {
  constexpr int NW = RLE_SCAN_T / WAVE;
  __shared__ int wsum[NW], wmax[NW];
  const int z = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* __restrict__ cz = cells + (long long)z * per;
  int carry = 0, carry_pos = -1;                                    // over the tiles before this one
  for (long long t0 = 0; t0 < ncell; t0 += RLE_SCAN_T) {
    const long long i = t0 + tid;
    const int c = i < ncell ? cz[i] : 0, l = i < ncell ? cz[ncell + i] : -1;
    int sc = c, sl = l;                                             // inclusive over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int tc = __shfl_up(sc, o, 64), tl = __shfl_up(sl, o, 64);
      if (lane >= o) { sc += tc; sl = max(sl, tl); }
    }
    if (lane == 63) { wsum[wave] = sc; wmax[wave] = sl; }
    __syncthreads();
    int pc = carry, pl = carry_pos, tc = 0, tl = -1;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int a = wsum[w], b = wmax[w];
      if (w < wave) { pc += a; pl = max(pl, b); }
      tc += a; tl = max(tl, b);
    }
    int el = __shfl_up(sl, 1, 64);
    if (lane == 0) el = -1;
    if (i < ncell) {
      cz[i] = pc + sc - c;
      cz[ncell + i] = max(pl, el);
    }
    carry += tc;
    carry_pos = max(carry_pos, tl);
    __syncthreads();
  }
  if (tid == 0) {
    cz[2 * ncell] = carry;
    cz[2 * ncell + 1] = carry_pos;
    totals[z] = (long long)carry + (masks[(long long)z * HW] ? 1 : 0);
  }
}

__global__ __launch_bounds__(256) void rle_decode_kernel(const long long* __restrict__ ends, const long long* __restrict__ offsets,
                                                         int H, int W, uint8_t* __restrict__ out) {
  const int z = blockIdx.y;
  const long long HW = (long long)H * W, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  const int y = (int)(i / W), x = (int)(i - (long long)y * W);
  const long long p = (long long)x * H + y;
  const long long lo = offsets[z], hi = offsets[z + 1];
  const long long base = lo > 0 ? ends[lo - 1] : 0;
  long long a = lo, b = hi;                                         // the first run whose end lies past p
  while (a < b) {
    const long long mid = (a + b) >> 1;
    if (ends[mid] - base > p) b = mid; else a = mid + 1;
  }
  out[(long long)z * HW + i] = a < hi ? (uint8_t)((a - lo) & 1) : (uint8_t)0;
}

static bool rle_shape_ok(int n, int H, int W) {
  return n > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL;
}
static int rle_nseg(int H) { return (H + RLE_SEG - 1) / RLE_SEG; }
static long long rle_per_mask(int H, int W) { return 2LL * W * rle_nseg(H) + 2; }

template <bool WRITE>
static int rle_pass_launch(const unsigned char* masks, int n, int H, int W, int* cells, const long long* offsets, int* counts,
                           hipStream_t s) {
  const bool vec = (W % 4) == 0 && ((uintptr_t)masks % 4) == 0;
  const int nseg = rle_nseg(H);
  const long long nstrip = ((long long)W + (vec ? 4 : 1) * WAVE - 1) / ((vec ? 4 : 1) * WAVE);
  const long long tiles = nstrip * ((nseg + RLE_WAVES - 1) / RLE_WAVES);
  if (tiles > 0x7fffffffLL) return PSAM_ERR_ARG;
  const long long HW = (long long)H * W, per = rle_per_mask(H, W);
  for (int z0 = 0; z0 < n; z0 += RLE_MAX_GRID_Y) {
    const int nz = n - z0 < RLE_MAX_GRID_Y ? n - z0 : RLE_MAX_GRID_Y;
    const dim3 grid((unsigned)tiles, (unsigned)nz), block(WAVE * RLE_WAVES);
    const unsigned char* mz = masks + z0 * HW;
    int* cz = cells + z0 * per;
    const long long* oz = offsets ? offsets + z0 : nullptr;
    if (vec) hipLaunchKernelGGL((rle_pass_kernel<4, WRITE>), grid, block, 0, s, mz, H, W, nseg, (int)nstrip, per, cz, oz, counts);
    else hipLaunchKernelGGL((rle_pass_kernel<1, WRITE>), grid, block, 0, s, mz, H, W, nseg, (int)nstrip, per, cz, oz, counts);
  }
  return PSAM_OK;
}

extern "C" int psam_rle_workspace(int H, int W, long long* ints_per_mask) {
  if (!rle_shape_ok(1, H, W) || !ints_per_mask) return PSAM_ERR_ARG;
  *ints_per_mask = rle_per_mask(H, W);
  return PSAM_OK;
}

extern "C" int psam_rle_count(const unsigned char* masks, int n, int H, int W, int* cells, long long* totals, void* stream) {
  if (!rle_shape_ok(n, H, W) || !masks || !cells || !totals) return PSAM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int st = rle_pass_launch<false>(masks, n, H, W, cells, nullptr, nullptr, s);
  if (st != PSAM_OK) return st;
  const long long HW = (long long)H * W, per = rle_per_mask(H, W), ncell = (long long)W * rle_nseg(H);
  hipLaunchKernelGGL(rle_scan_kernel, dim3((unsigned)n), dim3(RLE_SCAN_T), 0, s, masks, HW, ncell, per, cells, totals);
  return psam_launch_status();
}

extern "C" int psam_rle_write(const unsigned char* masks, int n, int H, int W, const int* cells, const long long* offsets,
                              int* counts, void* stream) {
  if (!rle_shape_ok(n, H, W) || !masks || !cells || !offsets || !counts) return PSAM_ERR_ARG;
  const int st = rle_pass_launch<true>(masks, n, H, W, const_cast<int*>(cells), offsets, counts, (hipStream_t)stream);
  return st != PSAM_OK ? st : psam_launch_status();
}

extern "C" int psam_rle_decode(const long long* ends, const long long* offsets, int n, int H, int W, unsigned char* masks_out,
                               void* stream) {
  if (!rle_shape_ok(n, H, W) || !ends || !offsets || !masks_out) return PSAM_ERR_ARG;
  const long long HW = (long long)H * W;
  for (int z0 = 0; z0 < n; z0 += RLE_MAX_GRID_Y) {
    const int nz = n - z0 < RLE_MAX_GRID_Y ? n - z0 : RLE_MAX_GRID_Y;
    hipLaunchKernelGGL(rle_decode_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)nz), dim3(256), 0, (hipStream_t)stream,
                       ends, offsets + z0, H, W, masks_out + z0 * HW);
  }
  return psam_launch_status();
}
