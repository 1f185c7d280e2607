// Work tables of the persistent kernels, as plain C++: which tile, K range, (image, head, query block) or (image, head, window) a
// workgroup takes next. No HIP include: the HIP translation units take this through common.h, and tests/work_tables_dump.cpp compiles
// it with the host compiler alone (tests/test_work_tables_cpu.py checks every table against oracle/gemm.py and oracle/attention.py).
// The builders return host data only; device_tables.h uploads and caches it.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

#ifdef __HIPCC__
#define PSAM_HD __host__ __device__ __forceinline__
#else
#define PSAM_HD inline
#endif

// XCD-aware bijective block remap (8 XCDs; block b runs on XCD b % 8): gives each XCD a
// contiguous chunk of the logical tile space so neighbouring tiles share an L2.
PSAM_HD int xcd_remap(int bid, int nwg) {
  const int nx = 8;
  int xcd = bid % nx, idx = bid / nx;
  int q = nwg / nx, r = nwg % nx;
  int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

// ---- tile -> workgroup mapping ------------------------------------------------------------------------------------
// Block b runs on XCD b % 8 (observed placement; used for speed only, never for correctness) and every XCD has a
// private 4 MiB L2. The tiles an XCD works on CONCURRENTLY (32 CUs x blocks/CU) should therefore share as many A row
// panels and W column panels as possible: the 8 XCDs are laid out as an xm x xn grid over the tile space (the split
// that minimises rows + cols per region) and each XCD walks its region in 4-row strips, column by column, so any 32
// consecutive tiles of an XCD form a ~4 x 8 patch (12 operand panels instead of 33 for a row-major chunk).
// Measured on 8192^3 (256x256 tiles): DMA-only time 1213 us (contiguous chunk per XCD) -> 500 us (2-D spread).
// The split, for the host functions below; tile_map keeps the same four candidates written out in its body, because calling this
// there reorders the scalar code of every HIP GEMM kernel (the instruction streams are compared with the previous build's).
// tests/test_work_tables_cpu.py holds the two together: tile_map over tile_map_grid hands out every tile once.
inline void xcd_split(int ntm, int ntn, int& xm, int& xn) {
  xm = 8; xn = 1;
  int best = (ntm + 7) / 8 + ntn;
  int c = (ntm + 3) / 4 + (ntn + 1) / 2;
  if (c < best) { best = c; xm = 4; xn = 2; }
  c = (ntm + 1) / 2 + (ntn + 3) / 4;
  if (c < best) { best = c; xm = 2; xn = 4; }
  c = ntm + (ntn + 7) / 8;
  if (c < best) { best = c; xm = 1; xn = 8; }
}
// mode 0: the 2-D XCD-region map; 1: identity; 2: a contiguous chunk per XCD. false: block `bid` has no tile
PSAM_HD bool tile_map(int bid, int ntm, int ntn, int mode, int& tm, int& tn) {
  if (mode == 1) {
    if (bid >= ntm * ntn) return false;
    tm = bid / ntn;
    tn = bid % ntn;
    return true;
  }
  if (mode == 2) {
    if (bid >= ntm * ntn) return false;
    const int t = xcd_remap(bid, ntm * ntn);
    tm = t / ntn;
    tn = t % ntn;
    return true;
  }
  const int xcd = bid & 7, idx = bid >> 3;
  int xm = 8, xn = 1, best = (ntm + 7) / 8 + ntn;
  {
    int c = (ntm + 3) / 4 + (ntn + 1) / 2;
    if (c < best) { best = c; xm = 4; xn = 2; }
    c = (ntm + 1) / 2 + (ntn + 3) / 4;
    if (c < best) { best = c; xm = 2; xn = 4; }
    c = ntm + (ntn + 7) / 8;
    if (c < best) { best = c; xm = 1; xn = 8; }
  }
  // proportional (balanced) split: region rx owns rows [rx*ntm/xm, (rx+1)*ntm/xm)
  const int rx = xcd / xn, cx = xcd % xn;
  const int r0 = (rx * ntm) / xm, c0 = (cx * ntn) / xn;
  const int nr = ((rx + 1) * ntm) / xm - r0, nc = ((cx + 1) * ntn) / xn - c0;
  if (nr <= 0 || nc <= 0 || idx >= nr * nc) return false;
  const int strip = idx / (4 * nc), rem = idx - strip * 4 * nc;
  const int rows = (nr - strip * 4) < 4 ? (nr - strip * 4) : 4;
  tm = r0 + strip * 4 + rem % rows;
  tn = c0 + rem / rows;
  return true;
}
// Largest number of tiles any XCD region of the 2-D map (mode 0) holds. One workgroup per CU and 32 CUs per
// XCD: a region of 33 tiles costs two rounds where a balanced split costs one (85 x 3 tiles: five regions of 11 x 3).
inline int tile_map_max_region(int ntm, int ntn) {
  int xm, xn, mx = 0;
  xcd_split(ntm, ntn, xm, xn);
  for (int x = 0; x < 8; ++x) {
    const int rx = x / xn, cx = x % xn;
    const int nr = ((rx + 1) * ntm) / xm - (rx * ntm) / xm, nc = ((cx + 1) * ntn) / xn - (cx * ntn) / xn;
    mx = nr * nc > mx ? nr * nc : mx;
  }
  return mx;
}
// grid size that covers every region of tile_map
inline int tile_map_grid(int ntm, int ntn, int mode) {
  if (mode != 0) return ntm * ntn;
  int xm, xn;
  xcd_split(ntm, ntn, xm, xn);
  return 8 * ((ntm + xm - 1) / xm) * ((ntn + xn - 1) / xn);
}
// map for the one-workgroup-per-CU kernels on a device of `cus` CUs in `xcds` XCDs: the 2-D region map unless its fullest region needs
// more rounds than a balanced split of the tiles (then contiguous, balanced chunks per XCD: mode 2); the identity where the device is
// not the 8-XCD geometry the region maps are laid out for
inline int pick_map_mode(int ntm, int ntn, int cus, int xcds) {
  if (xcds != 8 || cus % 8 != 0) return 1;
  const int total = ntm * ntn, per_xcd = cus / 8;
  const int rounds_region = (tile_map_max_region(ntm, ntn) + per_xcd - 1) / per_xcd, rounds_even = (total + cus - 1) / cus;
  return rounds_region > rounds_even ? 2 : 0;
}
// How many K ranges the split-K form of the assembly tile uses for M x N x K on `ncu` CUs (0: the shape does not pay - few tiles AND a
// long K are needed: every range keeps >= 16 K-tiles, the items fill >= 3/4 of the CUs in one round). N <= 2048: the reduce pass
// holds a row in registers.
constexpr int SPLITK_MAX_N = 2048;
inline int splitk_ranges(int M, int N, int K, int ncu) {
  if (M <= 0 || N <= 0 || K <= 0 || (N % 256) || (K % 64) || N > SPLITK_MAX_N) return 0;
  const int tiles = ((M + 255) / 256) * (N / 256), nkt = K / 64;
  if (tiles * 2 > ncu) return 0;
  int ks = ncu / tiles;
  if (ks > 8) ks = 8;
  while (ks >= 2 && nkt / ks < 16) --ks;
  if (ks < 2 || tiles * ks * 4 < ncu * 3) return 0;
  return ks;
}

// ---- the tables -------------------------------------------------------------------------------------------------------------------
// `words` is what the kernel reads (empty: the builder refuses the shape), `grid` the workgroups to launch, `rows` the depth of a
// column-per-workgroup list (0 where the table is not one).
struct WorkTable { std::vector<int> words; int grid = 0, rows = 0; };

// column-per-workgroup layout: entry i of workgroup b at words[i * G + b], -1 from the end of its list on, `pad` rows of -1 below the
// longest list (the kernels read that far ahead)
inline WorkTable work_table_columns(const std::vector<std::vector<int>>& lists, int pad) {
  WorkTable t;
  const size_t G = lists.size();
  size_t rows = 0;
  for (auto& l : lists) rows = l.size() > rows ? l.size() : rows;
  rows += pad;
  t.words.assign(rows * G, -1);
  for (size_t b = 0; b < G; ++b)
    for (size_t i = 0; i < lists[b].size(); ++i) t.words[i * G + b] = lists[b][i];
  t.grid = (int)G;
  t.rows = (int)rows;
  return t;
}

// The assembly GEMM kernels (gemm_asm_gen.py): ntm x ntn tiles in the order of tile_map(mode), dealt round-robin to min(G, blocks of
// the map) workgroups. Entry tm | tn << 16 (a positive int: tn below 2^15), three rows of -1 below the longest list.
inline WorkTable gemm_work_table(int ntm, int ntn, int mode, int G) {
  if (ntm < 1 || ntn < 1 || G < 1 || ntm >= 4096 || ntn >= (1 << 15)) return {};
  const int total = tile_map_grid(ntm, ntn, mode);
  if (total < G) G = total;
  std::vector<std::vector<int>> lists(G);
  for (int b = 0; b < G; ++b)
    for (int idx = b; idx < total; idx += G) {
      int tm = 0, tn = 0;
      if (tile_map(idx, ntm, ntn, mode, tm, tn)) lists[b].push_back(tm | (tn << 16));
    }
  return work_table_columns(lists, 3);
}

// Split-K on the assembly tile (psam_gemm_asm_f32_sk): an item is (tile, K range), entry tm | r << 12 | tn << 16, the ks ranges of a
// tile neighbours (they share both operand panels' rows); item i goes to workgroup i % G, G = min(G, items). Three rows of -1.
inline WorkTable splitk_work_table(int ntm, int ntn, int mode, int ks, int G) {
  if (ntm < 1 || ntn < 1 || G < 1 || ntm >= 4096 || ntn >= (1 << 15) || ks < 2 || ks > 8) return {};
  const int ntiles = tile_map_grid(ntm, ntn, mode);
  std::vector<int> items;
  for (int idx = 0; idx < ntiles; ++idx) {
    int tm = 0, tn = 0;
    if (!tile_map(idx, ntm, ntn, mode, tm, tn)) continue;
    for (int r = 0; r < ks; ++r) items.push_back(tm | (r << 12) | (tn << 16));
  }
  const int total = (int)items.size();
  if (total < G) G = total;
  WorkTable t;
  t.grid = G;
  t.rows = (total + G - 1) / G + 3;
  t.words.assign((size_t)t.rows * G, -1);
  for (int i = 0; i < total; ++i) t.words[i] = items[i];
  return t;
}

// The global attention kernels (gattn_asm_gen.py): entry wg = (b * H + h) << 10 | query block, -1 = none.
// Workgroup wg runs on XCD wg % 8 (observed placement, speed only): the (b, h)-major item list is cut into `xcds` equal contiguous
// runs, XCD x walks run x - the same number of workgroups on every XCD, and the ones of an XCD that run side by side read the same
// K / V. (12 heads x 21 query blocks of one 1022^2 DINOv2 image: 252 items = one round of 256 CUs; the arithmetic map of round 4
// - eight (b, h) pairs per row of XCDs - ran it in two.)
inline WorkTable gattn_work_table(int BH, int nqb, int xcds) {
  if (BH < 1 || nqb < 1 || nqb > 1023 || xcds < 1 || (long long)BH * nqb >= (1 << 21)) return {};
  const long long items = (long long)BH * nqb;
  const int per = (int)((items + xcds - 1) / xcds);
  WorkTable t;
  t.words.assign((size_t)per * xcds, -1);
  for (int x = 0; x < xcds; ++x) {
    const long long i0 = items * x / xcds, i1 = items * (x + 1) / xcds;
    for (long long i = i0; i < i1; ++i) t.words[(size_t)(i - i0) * xcds + x] = (int)(((i / nqb) << 10) | (i % nqb));
  }
  t.grid = per * xcds;
  return t;
}

// The window kernel (wattn_asm_gen.py; 25 windows of 14 x 14 on the 64 x 64 token map): per workgroup its (image, head, window)
// items, entry b | h << 8 | wy << 16 | wx << 24, in the XCD-aware order of wattn_p_kernel (windows of one XCD together, the heads of
// a window back to back). Two rows of -1.
inline WorkTable wattn_work_list(int B, int H, int grid) {
  if (B < 1 || B > 255 || H < 1 || H > 255 || grid < 1) return {};
  const int nwin = 25, ngrp = B * nwin;
  std::vector<std::vector<int>> lists(grid);
  for (int wg = 0; wg < grid; ++wg) {
    const int x = wg & 7, sx = wg >> 3;
    const int nwg_x = (grid + 7 - x) >> 3;
    const int nwin_x = (ngrp + 7 - x) >> 3;        // windows (b, wy, wx) of XCD x: grp = q * 8 + x
    auto push = [&](int grpq, int hh) {
      const int grp = grpq * 8 + x, win = grp % nwin, b = grp / nwin;
      lists[wg].push_back(b | (hh << 8) | ((win / 5) << 16) | ((win % 5) << 24));
    };
    if (nwg_x % H == 0) {
      // the workgroups of an XCD that run side by side take the H heads of the SAME window(s): a token's q / k / v rows of adjacent
      // heads are 160-byte neighbours, i.e. they share 128-byte lines - fetched once into the XCD's L2 instead of once per head
      // (measured, 16 slices: FETCH_SIZE 834 -> see DESIGN.md; a workgroup keeps ONE head and walks the windows)
      const int lanes = nwg_x / H, hh = sx % H, lane = sx / H;
      for (int q = lane; q < nwin_x; q += lanes) push(q, hh);
    } else {
      const long long cnt_x = (long long)nwin_x * H;
      const int it0 = (int)((long long)sx * cnt_x / nwg_x), it1 = (int)((long long)(sx + 1) * cnt_x / nwg_x);
      for (int i = it0; i < it1; ++i) push(i / H, i % H);
    }
  }
  return work_table_columns(lists, 2);
}

// DMA geometry of the window kernel for a token row stride of rs2 bytes: per (image kind, piece of 64 lanes, lane) the byte offset of
// the lane's 16-byte chunk relative to the window's first token, its offset inside a pad row, and per edge class (partial last
// window row / column) the exec masks "token row" / "pad row" of every piece.
constexpr int WATTN_GEOM_P = 42, WATTN_GEOM_NP = 35;
inline WorkTable wattn_geometry_table(long long rs2) {
  constexpr int P = WATTN_GEOM_P, NP = WATTN_GEOM_NP, WS = 14, GWID = 64;
  if (rs2 < 160 || ((WS - 1) * GWID + WS - 1) * rs2 + 9 * 16 > 0xffffffffLL) return {};
  std::vector<unsigned> h((size_t)3 * P * 64 + (size_t)4 * 2 * P * 4, 0u);
  for (int img = 0; img < 2; ++img)
    for (int pc = 0; pc < NP; ++pc)
      for (int l = 0; l < 64; ++l) {
        const int S = pc * 64 + l, R = S / 10, c = S - R * 10;
        int ky, kx;
        if (img == 0) { ky = R >> 4; kx = R & 15; }
        else { const int C = R >> 5, rho = R & 31; ky = 2 * C + ((rho >> 3) & 1); kx = 4 * (2 * (rho >> 4) + ((rho >> 2) & 1)) + (rho & 3); }
        const bool valid = kx < WS && ky < WS;
        h[((size_t)img * P + pc) * 64 + l] = valid ? (unsigned)((long long)(ky * GWID + kx) * rs2 + c * 16) : 0u;
        h[((size_t)2 * P + pc) * 64 + l] = (unsigned)(c * 16);
        for (int cls = 0; cls < 4; ++cls) {
          const bool ey = cls & 2, ex = cls & 1;
          const bool in = valid && !(ey && ky >= 8) && !(ex && kx >= 8), pad = valid && !in;
          unsigned* m = &h[(size_t)3 * P * 64 + (((size_t)cls * 2 + img) * P + pc) * 4];
          if (in) m[l >> 5] |= 1u << (l & 31);
          if (pad) m[2 + (l >> 5)] |= 1u << (l & 31);
        }
      }
  WorkTable t;
  t.words.resize(h.size());
  memcpy(t.words.data(), h.data(), h.size() * sizeof(unsigned));
  return t;
}
