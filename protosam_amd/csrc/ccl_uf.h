// The 8-connected union-find pieces shared by csrc/ccl.hip (component table of one prediction) and csrc/small_regions.hip (holes
// and islands of a batch of masks): lock-free find / union, the run-start initialisation and the reduced set of merges.
//
// Every loop here terminates because parents only decrease: uf_union hangs the larger root under the smaller one with atomicMin,
// so a component's root is its first pixel in raster order, whatever the scheduling.
#pragma once
#include "common.h"

__device__ __forceinline__ int uf_find(const int* parent, int a) {
  int p = parent[a];
  while (p != a) {
    a = p;
    p = parent[a];
  }
  return a;
}

__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      int t = a;
      a = b;
      b = t;
    }
    // a > b: hang a under b if a is still a root
    int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;  // somebody re-parented a concurrently; retry from its new parent
  }
}

// init: a foreground pixel points at the start of its horizontal run inside its 64-pixel wave segment (found with one ballot, no
// atomics), so horizontal connectivity inside a segment costs nothing and find() paths stay short; background gets -1. Every lane
// of the wave calls this (lanes right of the row pass fg = false); `lane` = threadIdx.x & 63 and the wave covers x - lane .. + 63.
__device__ __forceinline__ int uf_run_start(bool fg, int x, int y, int W, int lane) {
  const unsigned long long mask = __ballot(fg);
  if (!fg) return -1;
  const unsigned long long below = lane ? (~mask & ((1ull << lane) - 1ull)) : 0ull;  // background lanes left of me
  const int start = below ? 64 - __clzll((long long)below) : 0;
  return y * W + (x - lane) + start;
}

// merge: unions only where connectivity is not already implied by a horizontal run (Playne/Hawick-style reduction):
//   W  : only for the first lane of a segment (runs crossing a 64-pixel boundary)
//   N  : unless W and NW are both foreground (then W already linked to NW, which is in N's run)
//   NW : only if N and W are background
//   NE : only if N is background
// `fg(q)` = pixel q is foreground; the caller has checked x < W and fg(p), p = y * W + x.
template <typename Fg>
__device__ __forceinline__ void uf_merge_pixel(int* parent, int p, int x, int y, int W, bool seg_first, Fg fg) {
  const bool w = x > 0 && fg(p - 1);
  if (w && seg_first) uf_union(parent, p, p - 1);
  if (y == 0) return;
  const int q = p - W;
  const bool n = fg(q);
  const bool nw = x > 0 && fg(q - 1);
  const bool ne = x + 1 < W && fg(q + 1);
  if (n) {
    if (!(w && nw)) uf_union(parent, p, q);
  } else {
    if (nw && !w) uf_union(parent, p, q - 1);
    if (ne) uf_union(parent, p, q + 1);
  }
}
