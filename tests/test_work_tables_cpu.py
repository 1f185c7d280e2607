"""No GPU: the work tables of the persistent kernels, from the C++ the launchers upload.

protosam_amd/csrc/work_tables.h has no HIP include. tests/work_tables_dump.cpp, a program of its own that includes nothing else of the
library, is compiled here with the host compiler under the address and undefined-behaviour sanitizers and run once per family; its
tables are compared

  * with the restatements in Python, value for value: oracle/gemm.py (tile_map, tile_map_grid, pick_map_mode, splitk_ranges) and
    oracle/attention.py (gattn_asm_table, wattn_asm_lists) - so those, which the GPU tests name their branches from, are checks of the
    real code and not stand-ins for it;
  * with what a table must hold whatever built it: every tile, (tile, K range), (image, head, query block), (image, head, window) and
    (key row, key column, 16-byte chunk) exactly once, the -1 rows below the lists, the refusals;
  * with tests/golden/work_tables_sha256.json: the SHA-256 of each table's words (little-endian int32), recorded from the builders as
    they stood inside csrc/gemm.hip and csrc/attention.hip before they moved to the header.
"""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import attention as A
from oracle import gemm as G

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "work_tables_sha256.json")))
TABLE_KINDS = ("gemm_table", "splitk_table", "gattn_table", "wattn_worklist", "wattn_geometry")

# ---- the shapes --------------------------------------------------------------------------------------------------------------------
SWEEP_GRIDS = tuple(sorted({((c.M + c.th - 1) // c.th, c.N // c.tw) for c in G.cases() if c.path == "map1"}))
GEMM_GRIDS = tuple(dict.fromkeys(SWEEP_GRIDS + ((256, 5), (256, 15), (256, 20), (16, 5), (16, 20), (21, 3), (21, 12), (85, 3), (1, 1), (1, 8))))
GEMM_G = (256, 128, 64, 8192)               # 8192: more workgroups than any grid here has blocks
MODES = (0, 1, 2)
GEOMETRIES = ((256, 8), (128, 8), (64, 8), (24, 8), (256, 4), (20, 8), (304, 38))      # (CUs, XCDs); the last three: no 8-XCD geometry
SPLITK_GRID = (16, 5)
SPLITK_RANGES = ([(M, N, K, wgs, ks) for M, N, K, wgs, ks in G.SPLITK_LN] + [(M, N, K, wgs, 0) for M, N, K, wgs in G.SPLITK_LN_DECLINED]
                 + [(4096, 1280, 5120, 256, 3), (4096, 768, 3072, 256, 0)])             # the rows of tests/test_gemm_reference_cpu.py
GATTN_BH = tuple(B * H for B, H in A.ITEMS_ASM_BH + A.ITEMS_ASM_EDGES)
GATTN_NQB = (1, 6, 16, 21)
WATTN_BH = ((1, 1), (1, 16), (16, 16), (2, 12), (7, 16), (3, 33), (5, 3))
WATTN_CUS = (256, 64)
WATTN_RS2 = tuple(3 * H * 80 * 2 for H in (1, 12, 16))       # bytes between two tokens of a token-major qkv, hd = 80


def gemm_args():
    a = [f"tile_map:{m}:{n}:{mode}" for m, n in GEMM_GRIDS for mode in MODES]
    a += [f"pick_map_mode:{m}:{n}:{cus}:{x}" for m, n in GEMM_GRIDS for cus, x in GEOMETRIES]
    a += [f"gemm_table:{m}:{n}:{mode}:{g}" for m, n in GEMM_GRIDS for mode in MODES for g in GEMM_G]
    a += [f"splitk_table:{SPLITK_GRID[0]}:{SPLITK_GRID[1]}:{mode}:{ks}:{g}" for mode in MODES for ks in range(1, 10) for g in GEMM_G]
    a += [f"splitk_ranges:{M}:{N}:{K}:{wgs}" for M, N, K, wgs, _ in SPLITK_RANGES]
    return a


def gattn_args():
    return [f"gattn_table:{bh}:{nqb}:{x}" for bh in GATTN_BH for nqb in GATTN_NQB for x in (8, 4)]


def wattn_grid(B, H, cus):
    return min(B * A.NWIN64 * H, cus)


def wattn_worklist_args():
    return list(dict.fromkeys(f"wattn_worklist:{B}:{H}:{wattn_grid(B, H, cus)}" for B, H in WATTN_BH for cus in WATTN_CUS))   # (1, 1): 25 twice


def wattn_geometry_args():
    return [f"wattn_geometry:{rs2}" for rs2 in WATTN_RS2]


# ---- the program ---------------------------------------------------------------------------------------------------------------------
def parse(stdout):
    """label -> (grid, rows, words as int32), or None where the builder refused"""
    out = {}
    for line in stdout.splitlines():
        f = line.split(" | ")
        if f[1] == "refused":
            out[f[0]] = None
        else:
            grid, rows = map(int, f[1].split())
            out[f[0]] = (grid, rows, np.array(f[2].split(), dtype=np.int64).astype(np.int32))
    return out


def sha256(words):
    return hashlib.sha256(np.asarray(words).astype("<i4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or "g++"
    assert shutil.which(cxx), f"no host C++ compiler ({cxx})"
    exe = str(tmp_path_factory.mktemp("work_tables") / "work_tables_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "work_tables_dump.cpp"), "-o", exe], check=True)

    done = {}

    def run(args):
        if tuple(args) in done:                                      # one run per family, shared by the tests that read it
            return done[tuple(args)]
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        tabs = parse(r.stdout)
        assert list(tabs) == [a.replace(":", " ") for a in args]
        for label, t in tabs.items():                                # parent equality: the words the builders gave before they moved
            if label.split()[0] in TABLE_KINDS and t is not None:
                assert label in GOLDEN, f"no digest recorded for '{label}'"
                assert sha256(t[2]) == GOLDEN[label], f"'{label}' differs from the table the parent commit built"
        done[tuple(args)] = tabs
        return tabs
    return run


def columns(lists, pad):
    """the column-per-workgroup layout: entry i of workgroup b at [i * G + b], -1 below"""
    rows = max(len(l) for l in lists) + pad
    w = np.full((rows, len(lists)), -1, dtype=np.int32)
    for b, l in enumerate(lists):
        w[:len(l), b] = l
    return rows, w.reshape(-1)


def check_columns(words, grid, rows, pad):
    """every list is entries then -1 to the bottom, and `pad` whole rows of -1 lie below the longest: the kernels read ahead"""
    w = words.reshape(rows, grid)
    n = (w >= 0).sum(0)
    assert all((w[:n[b], b] >= 0).all() and (w[n[b]:, b] == -1).all() for b in range(grid))
    assert rows == n.max() + pad and (w[rows - pad:] == -1).all()
    return [w[:n[b], b].tolist() for b in range(grid)]


# ---- GEMM ------------------------------------------------------------------------------------------------------------------------------
def test_gemm_maps_and_tables(dump):
    assert len(SWEEP_GRIDS) == 9
    tabs = dump(gemm_args())
    picked = set()
    for ntm, ntn in GEMM_GRIDS:
        tiles = [(i, j) for i in range(ntm) for j in range(ntn)]
        for cus, xcds in GEOMETRIES:
            mode = int(tabs[f"pick_map_mode {ntm} {ntn} {cus} {xcds}"][2][0])
            assert mode == G.pick_map_mode(ntm, ntn, cus, xcds), (ntm, ntn, cus, xcds)
            assert (mode == 1) == (xcds != 8 or cus % 8 != 0)
            picked.add(mode)
        for mode in MODES:
            total, _, words = tabs[f"tile_map {ntm} {ntn} {mode}"]
            assert total == G.tile_map_grid(ntm, ntn, mode) == len(words)
            py = [G.tile_map(b, ntm, ntn, mode) for b in range(total)]
            assert words.tolist() == [-1 if t is None else t[0] | t[1] << 16 for t in py], (ntm, ntn, mode)
            assert sorted(t for t in py if t is not None) == tiles
            order = [t[0] | t[1] << 16 for t in py if t is not None]
            for g in GEMM_G:
                grid, rows, words = tabs[f"gemm_table {ntm} {ntn} {mode} {g}"]
                assert grid == min(g, total)
                want = [[t[0] | t[1] << 16 for t in py[b::grid] if t is not None] for b in range(grid)]
                want_rows, want_words = columns(want, 3)
                assert rows == want_rows and np.array_equal(words, want_words), (ntm, ntn, mode, g)
                lists = check_columns(words, grid, rows, 3)
                assert sorted(e for l in lists for e in l) == sorted(order)          # every tile exactly once
    assert picked == {0, 1, 2}
    assert G.pick_map_mode(85, 3) == 2 == int(tabs["pick_map_mode 85 3 256 8"][2][0])


def test_splitk_tables_and_ranges(dump):
    tabs = dump(gemm_args())
    ntm, ntn = SPLITK_GRID
    for mode in MODES:
        py = [t for t in (G.tile_map(b, ntm, ntn, mode) for b in range(G.tile_map_grid(ntm, ntn, mode))) if t is not None]
        for g in GEMM_G:
            for ks in (1, 9):
                assert tabs[f"splitk_table {ntm} {ntn} {mode} {ks} {g}"] is None           # refused: r << 12 below tn << 16, ks in 2..8
            for ks in range(2, 9):
                grid, rows, words = tabs[f"splitk_table {ntm} {ntn} {mode} {ks} {g}"]
                items = [tm | r << 12 | tn << 16 for tm, tn in py for r in range(ks)]      # a tile's ranges adjacent, in order
                assert len(set(items)) == len(items) == ntm * ntn * ks
                assert grid == min(g, len(items)) and rows == -(-len(items) // grid) + 3
                assert words[:len(items)].tolist() == items and (words[len(items):] == -1).all() and len(words) == rows * grid
                assert (words.reshape(rows, grid)[rows - 3:] == -1).all()
                for i in range(0, len(items), ks):                                        # the same, read from the table itself
                    e = words[i:i + ks]
                    assert ((e & ~0xf000) == (e[0] & ~0xf000)).all() and ((e >> 12) & 15).tolist() == list(range(ks))
    for M, N, K, wgs, ks in SPLITK_RANGES:
        assert int(tabs[f"splitk_ranges {M} {N} {K} {wgs}"][2][0]) == ks == G.splitk_ranges(M, N, K, wgs), (M, N, K, wgs)


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def test_global_attention_tables(dump):
    tabs = dump(gattn_args())
    for B, H in A.ITEMS_ASM_BH + A.ITEMS_ASM_EDGES:
        for nqb in GATTN_NQB:
            for xcds in (8, 4):
                grid, _, words = tabs[f"gattn_table {B * H} {nqb} {xcds}"]
                assert words.tolist() == A.gattn_asm_table(B * H, nqb, xcds), (B, H, nqb, xcds)
                assert grid == len(words) == -(-B * H * nqb // xcds) * xcds
                got = A.gattn_asm_decode(words.tolist(), H)           # b = (grp * ceil(2^16 / H)) >> 16, as the kernels divide
                assert len(got) == B * H * nqb and set(got) == {(b, h, q) for b in range(B) for h in range(H) for q in range(nqb)}


def test_window_work_lists(dump):
    tabs = dump(wattn_worklist_args())
    reached = set()
    for B, H in WATTN_BH:
        for cus in WATTN_CUS:
            g = wattn_grid(B, H, cus)
            grid, rows, words = tabs[f"wattn_worklist {B} {H} {g}"]
            py, one_head = A.wattn_asm_lists(B, H, g)
            want_rows, want = columns([[b | h << 8 | (w // 5) << 16 | (w % 5) << 24 for b, h, w in l] for l in py], 2)
            assert grid == g and rows == want_rows and np.array_equal(words, want), (B, H, cus)
            lists = check_columns(words, grid, rows, 2)
            items = [(e & 255, (e >> 8) & 255, 5 * ((e >> 16) & 255) + (e >> 24)) for l in lists for e in l]
            assert len(items) == B * H * A.NWIN64 and set(items) == {(b, h, w) for b in range(B) for h in range(H) for w in range(A.NWIN64)}
            for wg, x, sx, nwg_x, nwin_x, it0, it1 in A.wattn_shares(B, H, A.NWIN64, g):
                assert one_head[wg] == (nwg_x % H == 0)
                if nwg_x % H == 0:                                   # one head per workgroup, striding over the XCD's windows
                    assert {h for _, h, _ in py[wg]} <= {sx % H}
                    reached.add("nwg_x % H == 0" + (", grid == CUs" if g == cus else ", grid < CUs"))
                else:                                                # the contiguous share [it0, it1) of the XCD's (window, head) list
                    assert py[wg] == [((i // H * 8 + x) // A.NWIN64, i % H, (i // H * 8 + x) % A.NWIN64) for i in range(it0, it1)]
                    reached.add("nwg_x % H != 0")
    assert reached >= {"nwg_x % H == 0, grid == CUs", "nwg_x % H == 0, grid < CUs", "nwg_x % H != 0"}


def test_window_geometry(dump):
    P, NP = 42, 35                                                   # pieces of 64 lanes: allotted and used
    tabs = dump(wattn_geometry_args())
    for rs2 in WATTN_RS2:
        words = tabs[f"wattn_geometry {rs2}"][2].view(np.uint32).astype(np.int64)
        assert len(words) == 3 * P * 64 + 4 * 2 * P * 4
        off = words[:2 * P * 64].reshape(2, P, 64)
        pad_off = words[2 * P * 64:3 * P * 64].reshape(P, 64)
        masks = words[3 * P * 64:].reshape(4, 2, P, 4)               # [edge class][image kind][piece]: token lo, hi, pad lo, hi
        bits = ((masks[..., None] >> np.arange(32)) & 1).reshape(4, 2, P, 2, 64).astype(bool)
        tok, pad = bits[:, :, :, 0], bits[:, :, :, 1]
        slot = np.arange(NP * 64).reshape(NP, 64)
        assert np.array_equal(pad_off[:NP], slot % 10 * 16) and not pad_off[NP:].any() and not off[:, NP:].any()
        assert not tok[:, :, NP:].any() and not pad[:, :, NP:].any()
        for img in range(2):
            valid = tok[0, img]                                      # class 0, no partial edge: every valid lane is a token lane
            assert not pad[0, img].any()
            o = off[img][valid]
            key, c = o // rs2, o % rs2
            assert (c % 16 == 0).all() and (c < 160).all()
            ky, kx, c = key // 64, key % 64, c // 16
            got = list(zip(ky.tolist(), kx.tolist(), c.tolist()))
            assert len(got) == len(set(got)) == 14 * 14 * 10 and set(got) == {(y, x, k) for y in range(14) for x in range(14) for k in range(10)}
            assert not off[img][~valid].any()
            KY, KX = np.zeros((P, 64), np.int64), np.zeros((P, 64), np.int64)
            KY[valid], KX[valid] = ky, kx
            for cls in range(4):                                     # bit 1: partial last window row, bit 0: partial last window column
                assert not (tok[cls, img] & pad[cls, img]).any() and np.array_equal(tok[cls, img] | pad[cls, img], valid)
                inside = valid & ~(bool(cls & 2) & (KY >= 8)) & ~(bool(cls & 1) & (KX >= 8))
                assert np.array_equal(tok[cls, img], inside)
