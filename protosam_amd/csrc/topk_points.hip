// The k most confident pixels of every connected component, on the device (num_points_for_sam = k > 1).
//
// Replaces the host loop of models/ProtoSAM.py:266-289 `get_most_conf_points` (`torch.topk(output_p_fg[mask], k)` per component,
// called from get_sam_input_points :349-450 on a downloaded probability map and label image) with the convention the component
// table (csrc/ccl.hip, k = 1) and the negative points already follow: largest probability first, first pixel in raster order
// among equals. A pixel's key is (float bits of p_fg) << 32 | (0xFFFFFFFF - pixel index), p_fg >= 0: all keys of a plane differ,
// so "the k largest keys of component c in descending order" is one bit pattern whatever order the pixels arrive in.
//
// Algorithm, per (plane, row) - a row is a component of the table, or with only_best the one component tab[3]:
//   1. radix select of the k-th largest key, most significant byte first. Each pass histograms the byte at `shift` of the keys
//      that agree with the row's prefix so far (tk_hist_kernel: a wave first groups its 64 pixels by (row, byte) with ballots
//      and keeps the running group across its pixels, so a saturated soft-max - one bin for the whole component - costs one
//      atomic per wave, not one per pixel), then one workgroup per row walks the 256 bins from the top (tk_select_kernel) and
//      extends the prefix. Bytes of the index word above log2(H*W) are 0xFF in every key and are not passed over:
//      4 + ceil(log2(H*W) / 8) passes, 7 at 1024^2. A row with fewer than k pixels takes them all (threshold 0).
//   2. tk_compact_kernel: every pixel whose key is >= its row's threshold draws a slot from the row's counter (one atomic per
//      wave and row) and stores its key there; exactly k pixels per row do (the slot is still checked against k).
//   3. tk_sort_kernel: one workgroup per row sorts its <= 256 keys in LDS (bitonic, descending) and writes all k slots, zeros
//      beyond the row's pixel count. Rows of components that do not exist come out as zeros the same way.
// Integer atomics only; nothing is read back by the host. Scratch: per row 256 uint32 bins and one TkState.
#include "common.h"

#define CC_STRIDE 12
#define CC_HDR 8
#define TK_MAX_K (PSAM_MAX_PROMPT_TOKENS - 5)   // what a prompt set holds beside the decoder's 5 output tokens
#define TK_SORT 256                             // keys one workgroup sorts: >= TK_MAX_K
#define TK_PIX 8                                // pixels per thread of the passes over the image
#define TK_NONE 0xffffffffu

struct TkState {
  unsigned long long prefix;   // the bytes of the k-th largest key found so far; after the last pass the key itself (threshold)
  unsigned int krem;           // how many keys with this prefix are still wanted; 0: the row takes every pixel it has
  unsigned int cnt;            // slots drawn by tk_compact_kernel
};

static_assert(TK_MAX_K <= TK_SORT, "one workgroup sorts a row");

__device__ __forceinline__ unsigned long long tk_key(float p, long long idx) {
  return ((unsigned long long)__float_as_uint(p) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)idx);
}

// label -> row of this call, or -1 (background, a component beyond max_comp, or with only_best any but the kept one)
__device__ __forceinline__ int tk_row(int lab, int R, int best_lab) {
  if (lab <= 0) return -1;
  if (best_lab) return lab == best_lab ? 0 : -1;
  return lab <= R ? lab - 1 : -1;
}

__device__ __forceinline__ int tk_best_label(const double* tab, int only_best) {
  if (!only_best) return 0;
  return (int)tab[1] > 0 ? (int)tab[3] + 1 : 0x7fffffff;
}

__global__ __launch_bounds__(256) void tk_init_kernel(unsigned* __restrict__ hist, TkState* __restrict__ state, long long rows,
                                                      unsigned long long prefix0, unsigned k) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * 256) return;
  hist[i] = 0u;
  if ((i & 255) == 0) {
    TkState s = {prefix0, k, 0u};
    state[i >> 8] = s;
  }
}

__global__ __launch_bounds__(256) void tk_hist_kernel(const int* __restrict__ labels, const float* __restrict__ pfg,
                                                      const double* __restrict__ tabs, int n, int R, int only_best, int shift,
                                                      unsigned* __restrict__ hist, const TkState* __restrict__ state,
                                                      long long pfg_stride, long long tab_stride) {
  const int plane = blockIdx.y;
  labels += (size_t)plane * n;
  pfg += (size_t)plane * pfg_stride;
  hist += (size_t)plane * R * 256;
  state += (size_t)plane * R;
  const int best_lab = tk_best_label(tabs + (size_t)plane * tab_stride, only_best);
  const int lane = threadIdx.x & 63;
  unsigned pl = TK_NONE, pcnt = 0;   // the wave's running (row, byte) group and its size
  const long long base = (long long)blockIdx.x * (256 * TK_PIX) + threadIdx.x;
  for (int it = 0; it < TK_PIX; ++it) {
    const long long p = base + it * 256;
    unsigned combo = TK_NONE;
    if (p < n) {
      const int row = tk_row(labels[p], R, best_lab);
      if (row >= 0) {
        const TkState s = state[row];
        const unsigned long long key = tk_key(pfg[p], p);
        if (s.krem != 0 && (shift == 56 || (key >> (shift + 8)) == (s.prefix >> (shift + 8))))
          combo = ((unsigned)row << 8) | (unsigned)((key >> shift) & 255);
      }
    }
    unsigned long long todo = __ballot(combo != TK_NONE);
    while (todo) {   // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned L = __shfl(combo, leader, 64);
      const unsigned long long mask = __ballot(combo == L);
      todo &= ~mask;
      if (pl != L) {
        if (pl != TK_NONE && lane == 0) atomicAdd(&hist[pl], pcnt);   // pl = row * 256 + byte, row < R
        pl = L;
        pcnt = 0;
      }
      pcnt += __popcll(mask);
    }
  }
  if (pl != TK_NONE && lane == 0) atomicAdd(&hist[pl], pcnt);
}

// One workgroup per (row, plane): the byte at `shift` of the row's k-th largest key = the highest bin at which the count from
// the top reaches krem. Clears the bins for the next pass.
__global__ __launch_bounds__(256) void tk_select_kernel(unsigned* __restrict__ hist, TkState* __restrict__ state, int R, int shift) {
  __shared__ unsigned wt[4];
  const size_t r = (size_t)blockIdx.y * R + blockIdx.x;
  unsigned* h = hist + r * 256;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const unsigned v = h[255 - t];   // thread 0 holds the highest byte
  h[255 - t] = 0u;
  const TkState s = state[r];
  if (s.krem == 0) return;         // (uniform over the workgroup)
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wt[w] = inc;
  __syncthreads();
  unsigned off = 0, total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < w) off += wt[i];
    total += wt[i];
  }
  inc += off;
  const unsigned exc = inc - v;
  if (total < s.krem) {            // fewer than k pixels in this row (first pass): every one of them is taken
    if (t == 0) {
      state[r].prefix = 0ull;
      state[r].krem = 0u;
    }
    return;
  }
  if (exc < s.krem && inc >= s.krem) {   // exactly one thread
    state[r].prefix = s.prefix | ((unsigned long long)(255 - t) << shift);
    state[r].krem = s.krem - exc;
  }
}

__global__ __launch_bounds__(256) void tk_compact_kernel(const int* __restrict__ labels, const float* __restrict__ pfg,
                                                         const double* __restrict__ tabs, int n, int R, int only_best, int k,
                                                         TkState* __restrict__ state, unsigned long long* __restrict__ keys,
                                                         long long pfg_stride, long long tab_stride) {
  const int plane = blockIdx.y;
  labels += (size_t)plane * n;
  pfg += (size_t)plane * pfg_stride;
  state += (size_t)plane * R;
  keys += (size_t)plane * R * k;
  const int best_lab = tk_best_label(tabs + (size_t)plane * tab_stride, only_best);
  const int lane = threadIdx.x & 63;
  const long long base = (long long)blockIdx.x * (256 * TK_PIX) + threadIdx.x;
  for (int it = 0; it < TK_PIX; ++it) {
    const long long p = base + it * 256;
    int row = -1;
    unsigned long long key = 0ull;
    if (p < n) {
      row = tk_row(labels[p], R, best_lab);
      if (row >= 0) {
        key = tk_key(pfg[p], p);
        if (key < state[row].prefix) row = -1;
      }
    }
    unsigned long long todo = __ballot(row >= 0);
    while (todo) {   // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int L = __shfl(row, leader, 64);
      const unsigned long long mask = __ballot(row == L);
      todo &= ~mask;
      unsigned first = 0;
      if (lane == leader) first = atomicAdd(&state[L].cnt, (unsigned)__popcll(mask));   // L < R
      first = __shfl(first, leader, 64);
      if (row == L) {
        const unsigned slot = first + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
        if (slot < (unsigned)k) keys[(size_t)L * k + slot] = key;
      }
    }
  }
}

// One workgroup per (row, plane): the row's keys in descending order, zeros behind them; writes all k slots.
__global__ __launch_bounds__(TK_SORT) void tk_sort_kernel(const TkState* __restrict__ state, unsigned long long* __restrict__ keys,
                                                          int R, int k) {
  __shared__ unsigned long long a[TK_SORT];
  const size_t r = (size_t)blockIdx.y * R + blockIdx.x;
  const int t = threadIdx.x;
  unsigned cnt = state[r].cnt;
  cnt = cnt < (unsigned)k ? cnt : (unsigned)k;
  unsigned long long* row = keys + r * k;
  a[t] = (unsigned)t < cnt ? row[t] : 0ull;
  for (int size = 2; size <= TK_SORT; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int q = t ^ stride;
      if (q > t) {
        const unsigned long long x = a[t], y = a[q];
        const bool desc = (t & size) == 0;
        if (desc ? x < y : x > y) {
          a[t] = y;
          a[q] = x;
        }
      }
    }
  }
  __syncthreads();
  if (t < k) row[t] = a[t];
}

static long long tk_rows(int P, int max_comp, int only_best) { return (long long)P * (only_best ? 1 : max_comp); }

extern "C" int psam_topk_points_workspace(int P, int max_comp, int only_best, long long* bytes) {
  if (P <= 0 || max_comp < 1 || !bytes) return PSAM_ERR_ARG;
  *bytes = tk_rows(P, max_comp, only_best) * (long long)(256 * sizeof(unsigned) + sizeof(TkState));
  return PSAM_OK;
}

extern "C" int psam_topk_points_batch(const int* labels, const float* pfg, long long pfg_stride, const double* tabs, int cap, int P,
                                      int H, int W, int k, int max_comp, int only_best, unsigned long long* keys, void* scratch,
                                      long long scratch_bytes, void* stream) {
  if (H <= 0 || W <= 0 || P <= 0 || P > 65535 || (long long)H * W > 0x7fffffffLL || cap <= 0 || cap > 4096 || k < 1 ||
      k > TK_MAX_K || max_comp < 1 || max_comp > cap || pfg_stride < 0 || !labels || !pfg || !tabs || !keys || !scratch ||
      ((uintptr_t)scratch & 7))
    return PSAM_ERR_ARG;
  long long need = 0;
  if (psam_topk_points_workspace(P, max_comp, only_best, &need) != PSAM_OK || scratch_bytes < need) return PSAM_ERR_ARG;
  const int n = H * W, R = only_best ? 1 : max_comp;
  const long long rows = (long long)P * R;
  unsigned* hist = (unsigned*)scratch;
  TkState* state = (TkState*)(hist + rows * 256);
  hipStream_t s = (hipStream_t)stream;
  // index bits: idx < 2^lb, so every bit >= lb of 0xFFFFFFFF - idx is set; a byte that lies wholly there needs no pass
  int lb = 0;
  while (lb < 31 && (1LL << lb) < (long long)n) ++lb;
  unsigned long long prefix0 = 0ull;
  int shifts[8], ns = 0;
  for (int b = 7; b >= 4; --b) shifts[ns++] = 8 * b;
  for (int b = 3; b >= 0; --b) {
    if (8 * b >= lb) prefix0 |= 0xFFull << (8 * b);
    else shifts[ns++] = 8 * b;
  }
  const long long tab_stride = (long long)CC_HDR + (long long)CC_STRIDE * cap;
  const dim3 img((unsigned)(((long long)n + 256 * TK_PIX - 1) / (256 * TK_PIX)), (unsigned)P), per_row((unsigned)R, (unsigned)P);
  hipLaunchKernelGGL(tk_init_kernel, dim3((unsigned)rows), dim3(256), 0, s, hist, state, rows, prefix0, (unsigned)k);
  for (int i = 0; i < ns; ++i) {
    hipLaunchKernelGGL(tk_hist_kernel, img, dim3(256), 0, s, labels, pfg, tabs, n, R, only_best, shifts[i], hist, state, pfg_stride,
                       tab_stride);
    hipLaunchKernelGGL(tk_select_kernel, per_row, dim3(256), 0, s, hist, state, R, shifts[i]);
  }
  hipLaunchKernelGGL(tk_compact_kernel, img, dim3(256), 0, s, labels, pfg, tabs, n, R, only_best, k, state, keys, pfg_stride,
                     tab_stride);
  hipLaunchKernelGGL(tk_sort_kernel, per_row, dim3(TK_SORT), 0, s, state, keys, R, k);
  return psam_launch_status();
}

extern "C" int psam_topk_points(const int* labels, const float* pfg, const double* tab, int cap, int H, int W, int k, int max_comp,
                                int only_best, unsigned long long* keys, void* scratch, long long scratch_bytes, void* stream) {
  return psam_topk_points_batch(labels, pfg, 0LL, tab, cap, 1, H, W, k, max_comp, only_best, keys, scratch, scratch_bytes, stream);
}
