// The 3-D merge of csrc/volume_regions.hip on top of the union-find of ccl_uf.h: the unions of one foreground voxel with its
// "earlier" neighbours (the 13 of the 26 that come before it in raster order z, y, x), as far as the connectivity admits them:
//   6  : faces                     - W, N, and U = (z-1, y, x)
//   18 : faces and edges           - the plane's 4 earlier 8-neighbours, U and the 4 face neighbours of U in plane z-1
//   26 : faces, edges and corners  - the plane's 4 earlier 8-neighbours and all 9 of plane z-1
// The parent array is indexed by (z * H + y) * W + x and initialised per row with uf_run_start, so a horizontal run inside a
// 64-voxel wave segment is linked before the merge starts. Termination: ccl_uf.h (parents only decrease).
//
// Unions are left out where the link is already implied. The argument is an induction over the raster order with the claim
//   (*) after the merge, every foreground voxel is in the same set as each of its foreground earlier neighbours (of its connectivity)
// and a union may be skipped when (*) for EARLIER voxels, plus the unions this voxel does make, already give it:
//   in the plane, 18 / 26 : the reduced set of uf_merge_pixel as it stands (8-connectivity in the plane);
//   in the plane, 6       : W only for a segment's first lane (the run start links the rest), N always;
//   U, any connectivity   : skipped when W and UW = (z-1, y, x-1) are set: W is in my run or linked by the W rule, UW is the up
//                           neighbour of W (linked to W by (*) for W), and UW - U are face neighbours in plane z-1 ((*) for U);
//   rest of plane z-1     : skipped altogether when U is set: each of the other 8 is an 8-neighbour of U in plane z-1 (a face
//                           neighbour for the 4 that 18 admits), linked to U by (*) for whichever of the two comes later, and I am
//                           linked to U by the rule above. With U background:
//     UW : skipped when W is set (UW is W's up neighbour: (*) for W);   UN : skipped when N is set (UN is N's up neighbour, and
//          I am linked to N by the plane's rules);   UE, US : always (E and S come after me);
//     corners (26 only) UNW, UNE, USW, USE : skipped when one of the two edge neighbours of plane z-1 beside the corner is set
//          (UNW: UN or UW, ...): the corner is that voxel's face neighbour in plane z-1, and I am linked to that voxel by the
//          rules above.
#pragma once
#include "ccl_uf.h"

// `fg(q)` = voxel q (linear index in the volume) is foreground; the caller has checked x < W and fg(p), p = (z * H + y) * W + x;
// seg_first = first lane of its 64-voxel wave segment.
template <int CONN, typename Fg>
__device__ __forceinline__ void uf3_merge_voxel(int* parent, int p, int x, int y, int z, int W, int H, bool seg_first, Fg fg) {
  const bool xm = x > 0, xp = x + 1 < W, ym = y > 0, yp = y + 1 < H;
  const bool w = xm && fg(p - 1);
  const bool n = ym && fg(p - W);
  if (CONN == 6) {
    if (w && seg_first) uf_union(parent, p, p - 1);
    if (n) uf_union(parent, p, p - W);
  } else {
    uf_merge_pixel(parent, p, x, y, W, seg_first, fg);
  }
  if (z == 0) return;
  const int u = p - H * W;
  const bool uw = xm && fg(u - 1);
  if (fg(u)) {
    if (!(w && uw)) uf_union(parent, p, u);
    return;
  }
  if (CONN == 6) return;
  const bool ue = xp && fg(u + 1);
  const bool un = ym && fg(u - W);
  const bool us = yp && fg(u + W);
  if (uw && !w) uf_union(parent, p, u - 1);
  if (ue) uf_union(parent, p, u + 1);
  if (un && !n) uf_union(parent, p, u - W);
  if (us) uf_union(parent, p, u + W);
  if (CONN == 26) {
    if (xm && ym && !un && !uw && fg(u - W - 1)) uf_union(parent, p, u - W - 1);
    if (xp && ym && !un && !ue && fg(u - W + 1)) uf_union(parent, p, u - W + 1);
    if (xm && yp && !us && !uw && fg(u + W - 1)) uf_union(parent, p, u + W - 1);
    if (xp && yp && !us && !ue && fg(u + W + 1)) uf_union(parent, p, u + W + 1);
  }
}
