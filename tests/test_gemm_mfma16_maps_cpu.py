"""The 16x16x32 form of the assembly GEMM tile (csrc/gemm_asm_gen.py sched "mfma", csrc/gemm.hip tile 17), checked on the host.

The lane maps of the kernel are computed by its own setup code, so the test runs that code: a small interpreter of the integer
VALU / SALU instructions the prologue uses executes the generated text of each kernel for the four waves of a workgroup up to the
first branch, and the checks read the registers it leaves behind (fragment read addresses, DMA offsets, park and emit addresses).
Everything after the prologue that matters here is immediate (register numbers and `offset:` fields), and is taken from the text."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "protosam_amd", "csrc")
if CSRC not in sys.path:
    sys.path.insert(0, CSRC)
import gemm_asm_gen as G  # noqa: E402

LDS_BYTES = 160 * 1024
LDA = LDW = 320          # elements per operand row in the interpreted launch (bytes per row: 640)
LDO = 512
KINDS = [("f16", G.EPI_F16, False), ("gelu", G.EPI_GELU_F16, False), ("f32", G.EPI_F32, False),
         ("f16_ln", G.EPI_F16, True), ("gelu_ln", G.EPI_GELU_F16, True), ("f32_ln", G.EPI_F32, True)]


def _sched(ln):
    base = G.default_sched()
    return G.m16_sched(dict(base, ln_cons=True, ln_prod=True, store16_policy=" nt") if ln else base)


_cache = {}


def _kernel(kind):
    if kind not in _cache:
        name, epi, ln = [k for k in KINDS if k[0] == kind][0]
        g = G.Gen("psam_gemm_asm_%s_m16" % name, epi, _sched(ln))
        g.kernel()
        _cache[kind] = g
    return _cache[kind]


# ------------------------------------------------------------------ interpreter of the prologue
class Wave:
    """registers of one wave: v[n] = 64 uint32 lanes, s[n] = python ints (mod 2^32)"""

    def __init__(self, wv, kernarg):
        self.v = {0: (np.arange(64, dtype=np.uint64) + 64 * wv)}
        self.s = {2: 0}
        self.scc = 0
        self.vcc = np.zeros(64, dtype=bool)
        self.kernarg = kernarg

    def src(self, tok):
        tok = tok.strip()
        if tok.startswith("|"):
            raise NotImplementedError(tok)
        if re.fullmatch(r"v\d+", tok):
            return self.v[int(tok[1:])]
        if re.fullmatch(r"s\d+", tok):
            return np.uint64(self.s[int(tok[1:])])
        if tok == "m0":
            return np.uint64(self.s["m0"])
        return np.uint64(int(tok, 0) & 0xffffffff)

    def setv(self, tok, val):
        self.v[int(tok.strip()[1:])] = np.broadcast_to(np.asarray(val, dtype=np.uint64) & np.uint64(0xffffffff), (64,)).copy()

    def sets(self, tok, val):
        tok = tok.strip()
        self.s["m0" if tok == "m0" else int(tok[1:])] = int(val) & 0xffffffff


def _run_prologue(lines, wv):
    """executes `lines` for wave wv until the first s_cbranch; returns the Wave"""
    # kernarg dwords: pointers are 0 except bias / resid / gamma (non-null), M N K lda ldw ldo ldr G flags pad
    ka = [0] * 32
    ka[4], ka[8], ka[10] = 0x1000, 0x2000, 0x3000          # bias, resid, gamma (low halves)
    ka[14:24] = [512, 512, 320, LDA, LDW, LDO, LDO, 1, 1, 0xffffffff]
    ka[26], ka[28], ka[30] = 0x4000, 0x5000, LDO           # producer: out16, stats, ld16
    w = Wave(wv, ka)
    M = np.uint64(0xffffffff)
    for ln in lines:
        ln = ln.split("//")[0].strip()
        if not ln or ln.endswith(":") or ln.startswith("."):
            continue
        op, _, rest = ln.partition(" ")
        a = [t.strip() for t in rest.split(",")] if rest else []
        if op.startswith("s_cbranch"):
            return w
        if op in ("s_waitcnt", "s_nop", "s_barrier"):
            continue
        if op.startswith("s_load_dword"):
            m = re.fullmatch(r"s\[(\d+):(\d+)\]", a[0])
            lo, hi = (int(m.group(1)), int(m.group(2))) if m else (int(a[0][1:]), int(a[0][1:]))
            if a[1] == "s[0:1]":
                off = int(a[2], 0) // 4
                for i in range(lo, hi + 1):
                    w.s[i] = ka[off + i - lo]
            else:                                           # the work list: tile (0, 0)
                for i in range(lo, hi + 1):
                    w.s[i] = 0
            continue
        S = w.src
        if op == "v_and_b32": w.setv(a[0], S(a[1]) & S(a[2]))
        elif op == "v_or_b32": w.setv(a[0], S(a[1]) | S(a[2]))
        elif op == "v_xor_b32": w.setv(a[0], S(a[1]) ^ S(a[2]))
        elif op == "v_lshrrev_b32": w.setv(a[0], S(a[2]) >> (S(a[1]) & np.uint64(31)))
        elif op == "v_lshlrev_b32": w.setv(a[0], S(a[2]) << (S(a[1]) & np.uint64(31)))
        elif op == "v_add_u32": w.setv(a[0], S(a[1]) + S(a[2]))
        elif op == "v_lshl_add_u32": w.setv(a[0], (S(a[1]) << S(a[2])) + S(a[3]))
        elif op == "v_mul_lo_u32": w.setv(a[0], (S(a[1]) * S(a[2])) & M)
        elif op == "v_mad_u32_u24": w.setv(a[0], (S(a[1]) & np.uint64(0xffffff)) * (S(a[2]) & np.uint64(0xffffff)) + S(a[3]))
        elif op == "v_bfe_u32": w.setv(a[0], (S(a[1]) >> S(a[2])) & ((np.uint64(1) << S(a[3])) - np.uint64(1)))
        elif op == "v_mov_b32": w.setv(a[0], S(a[1]))
        elif op == "v_readfirstlane_b32": w.sets(a[0], int(np.asarray(S(a[1])).reshape(-1)[0]))
        elif op == "v_cmp_eq_u32": w.vcc = np.broadcast_to(S(a[1]) == S(a[2]), (64,)).copy()
        elif op == "v_cmp_ne_u32": w.vcc = np.broadcast_to(S(a[1]) != S(a[2]), (64,)).copy()
        elif op == "v_cndmask_b32": w.setv(a[0], np.where(w.vcc, np.broadcast_to(S(a[2]), (64,)), np.broadcast_to(S(a[1]), (64,))))
        elif op == "s_mov_b32": w.sets(a[0], S(a[1]))
        elif op == "s_mov_b64": pass
        elif op == "s_lshl_b32": w.sets(a[0], int(S(a[1])) << (int(S(a[2])) & 31))
        elif op == "s_lshr_b32": w.sets(a[0], int(S(a[1])) >> (int(S(a[2])) & 31))
        elif op == "s_and_b32": w.sets(a[0], int(S(a[1])) & int(S(a[2])))
        elif op == "s_andn2_b32": w.sets(a[0], int(S(a[1])) & ~int(S(a[2])))
        elif op == "s_or_b32": w.sets(a[0], int(S(a[1])) | int(S(a[2])))
        elif op == "s_add_u32":
            r = int(S(a[1])) + int(S(a[2])); w.scc = r >> 32; w.sets(a[0], r)
        elif op == "s_addc_u32":
            r = int(S(a[1])) + int(S(a[2])) + w.scc; w.scc = r >> 32; w.sets(a[0], r)
        elif op == "s_sub_u32":
            r = int(S(a[1])) - int(S(a[2])); w.scc = int(r < 0); w.sets(a[0], r)
        elif op == "s_mul_i32": w.sets(a[0], int(S(a[1])) * int(S(a[2])))
        elif op == "s_bfe_u32":
            c = int(S(a[2])); w.sets(a[0], (int(S(a[1])) >> (c & 31)) & ((1 << ((c >> 16) & 0x7f)) - 1))
        elif op == "s_cmp_eq_u32": w.scc = int(int(S(a[0])) == int(S(a[1])))
        elif op == "s_cmp_lt_u32": w.scc = int(int(S(a[0])) < int(S(a[1])))
        elif op == "s_cselect_b32": w.sets(a[0], S(a[1]) if w.scc else S(a[2]))
        else:
            raise NotImplementedError(ln)
    raise AssertionError("no branch found")


_waves = {}


def _waves_of(kind):
    if kind not in _waves:
        _waves[kind] = [_run_prologue(_kernel(kind).L, wv) for wv in range(4)]
    return _waves[kind]


def _dma_image(kind):
    """LDS image of one K-tile as the sixteen DMA pieces of the four waves write it (buffer 0): byte address of a 16-byte slot ->
    (operand 'A' / 'B', row of the 256-row operand tile, source k-slot 0..7). A piece lands at m0 + lane * 16."""
    g = _kernel(kind)
    img = {}
    for wv, w in enumerate(_waves_of(kind)):
        for p in range(16):
            m = re.fullmatch(r"s_add_u32 m0, s%d, (0x[0-9a-f]+)" % G.S_M0BASE, g.dma_m0(p))
            m0 = w.s[G.S_M0BASE] + int(m.group(1), 16)
            off = w.v[(G.V_DA + p) if p < 8 else (G.V_DB + p - 8)]
            ld2 = 2 * (LDA if p < 8 else LDW)
            for lane in range(64):
                o = int(off[lane])
                row, slot = o // ld2, (o % ld2) // 16
                assert (o % ld2) % 16 == 0 and slot < 8 and row < 256
                addr = m0 + 16 * lane
                assert addr not in img, "two DMA lanes write LDS byte %d" % addr
                img[addr] = ("A" if p < 8 else "B", row, slot)
    return img


@pytest.mark.parametrize("kind", [k[0] for k in KINDS])
def test_dma_covers_each_half_tile_once(kind):
    img = _dma_image(kind)
    assert len(img) == 4 * 128 * 8
    assert min(img) == 0 and max(img) + 16 <= G.LDS_SLAB <= LDS_BYTES          # below the epilogue slabs
    seen = sorted(img.values())
    assert seen == sorted((o, r, s) for o in "AB" for r in range(256) for s in range(8))
    # a half-tile (128 rows) is one contiguous 16 KiB image
    for addr, (o, r, s) in img.items():
        half = (0 if o == "A" else 2) + r // 128
        assert addr // (2 * G.LDS_BUF) == half and addr % (2 * G.LDS_BUF) < G.LDS_BUF


def _frag_reads(g):
    """(k-step, idx, first register, address register, offset) of the 32 fragment reads of the steady-state K-tile"""
    out = []
    for ks in range(2):
        for idx in range(16):
            m = re.fullmatch(r"ds_read_b128 v\[(\d+):(\d+)\], v(\d+) offset:(\d+)", g.frag_read16(ks, idx))
            assert int(m.group(2)) == int(m.group(1)) + 3
            out.append((ks, idx, int(m.group(1)), int(m.group(3)), int(m.group(4))))
    return out


@pytest.mark.parametrize("kind", [k[0] for k in KINDS])
def test_fragment_reads_match_the_mfma_operand_layout(kind):
    g, img = _kernel(kind), _dma_image(kind)
    reads = _frag_reads(g)
    # the K-tile text holds exactly these reads, each once in the loop body
    text = "\n".join(g.L)
    body = text[text.index("L_loop_%s:" % g.name):text.index("s_cbranch_scc0 L_loop_%s" % g.name)]
    for ks, idx, reg, areg, off in reads:
        assert body.count(g.frag_read16(ks, idx) + "\n") == 1
    assert body.count("ds_read_b128") == 32 and body.count("v_mfma_f32_16x16x32_f16") == 128
    dests = sorted(r[2] for r in reads)
    assert dests == list(range(32, 160, 4))                       # 32 fragments, four registers each, no overlap
    for wv, w in enumerate(_waves_of(kind)):
        wr, wc = wv >> 1, wv & 1
        for ks, idx, reg, areg, off in reads:
            addr = w.v[areg].astype(np.int64) + off
            assert addr.min() >= 0 and addr.max() + 16 <= LDS_BYTES
            got = [img[int(x)] for x in addr]                     # KeyError: a read of bytes no DMA lane wrote
            assert len(set(got)) == 64, "two lanes of a fragment read the same (row, k-slot)"
            for lane, (opd, row, slot) in enumerate(got):
                # v_mfma_f32_16x16x32_f16: lane supplies row lane & 15, k = 8 (lane >> 4) ... + 7 of the k-step's 32
                assert slot == 4 * ks + (lane >> 4)               # the same k mapping for X and W
                if idx < 8:
                    assert (opd, row) == ("A", wr * 128 + idx * 16 + (lane & 15))
                else:
                    assert (opd, row) == ("B", wc * 128 + (idx - 8) * 16 + (lane & 15))
    # per wave and K-tile: each of its 128 rows x 8 slots of both half-tiles exactly once
    for w in _waves_of(kind):
        cover = []
        for ks, idx, reg, areg, off in reads:
            cover += [img[int(x) + off] for x in w.v[areg]]
        assert len(cover) == len(set(cover)) == 2 * 128 * 8


@pytest.mark.parametrize("kind", [k[0] for k in KINDS])
def test_mfma_blocks_and_accumulators(kind):
    g = _kernel(kind)
    text = "\n".join(g.L)
    body = text[text.index("L_loop_%s:" % g.name):text.index("s_cbranch_scc0 L_loop_%s" % g.name)]
    pat = re.compile(r"v_mfma_f32_16x16x32_f16 a\[(\d+):(\d+)\], v\[(\d+):(\d+)\], v\[(\d+):(\d+)\], a\[(\d+):(\d+)\]")
    ms = [tuple(int(x) for x in m.groups()) for m in pat.finditer(body)]
    assert len(ms) == 128
    owner = {}
    for i, (d0, d1, a0, a1, b0, b1, c0, c1) in enumerate(ms):
        ks, rb, cb = i // 64, (i % 64) // 8, i % 8
        assert (d0, d1) == (c0, c1) == ((rb * 8 + cb) * 4, (rb * 8 + cb) * 4 + 3)
        assert (a0, a1) == (G.V_SET[2 * ks] + 32 + 4 * cb, G.V_SET[2 * ks] + 35 + 4 * cb)      # W fragment of column block cb
        assert (b0, b1) == (G.V_SET[2 * ks] + 4 * rb, G.V_SET[2 * ks] + 4 * rb + 3)            # X fragment of row block rb
        for r in range(d0, d1 + 1):
            assert owner.setdefault(r, (rb, cb)) == (rb, cb)
    assert sorted(owner) == list(range(256))                     # every accumulator register belongs to exactly one block
    # the C = 0 copy of k-step 0 writes each accumulator once
    head = text[text.index("L_tile_begin_%s:" % g.name):text.index("L_loop_%s:" % g.name)]
    z = re.findall(r"v_mfma_f32_16x16x32_f16 a\[(\d+):(\d+)\], v\[\d+:\d+\], v\[\d+:\d+\], 0\n", head)
    assert sorted(int(a) for a, b in z) == list(range(0, 256, 4))


def _slab_maps(kind):
    """park: for every park write of the epilogue, (slab index, {LDS byte address of an element: (row, column) of the wave's 128x128
    tile}); emit: the same for what the emit half stores to (row, column) from each address it reads. Per wave."""
    g = _kernel(kind)
    f32 = g.epi == G.EPI_F32
    esz = 4 if f32 else 2
    text = "\n".join(g.L)
    epi = text[text.index("---- epilogue"):]
    out = []
    for wv, w in enumerate(_waves_of(kind)):
        lane = np.arange(64)
        l16, grp = lane & 15, lane >> 4
        parks, emits, slab = [], [], {}
        acc_of = {}
        nslab = 0
        rows_done = 0
        for ln in epi.split("\n"):
            ln = ln.strip()
            m = re.fullmatch(r"v_accvgpr_read_b32 v(\d+), a(\d+)", ln)
            if m:
                acc_of[int(m.group(1))] = int(m.group(2))
                continue
            m = None if f32 else re.fullmatch(r"v_cvt_pk_f16_f32 v(\d+), v(\d+), v(\d+)", ln)
            if m:
                acc_of[("pk", int(m.group(1)))] = (acc_of[int(m.group(2))], acc_of[int(m.group(3))])
                continue
            m = re.fullmatch(r"ds_write_b64 v(\d+), v\[(\d+):(\d+)\] offset:(\d+)", ln) if not f32 else re.fullmatch(r"ds_write_b128 v(\d+), a\[(\d+):(\d+)\] offset:(\d+)", ln)
            if m:
                areg, r0, r1, off = (int(x) for x in m.groups())
                accs = list(range(r0, r1 + 1)) if f32 else list(acc_of[("pk", r0)] + acc_of[("pk", r0 + 1)])
                assert len(accs) == 4 and accs == list(range(accs[0], accs[0] + 4)) and accs[0] % 4 == 0
                rb, cb = accs[0] // 32, (accs[0] // 4) % 8
                for ln_ in lane:
                    for i in range(4):
                        a = int(w.v[areg][ln_]) + off + esz * i
                        assert G.LDS_SLAB + 8192 * wv <= a < G.LDS_SLAB + 8192 * (wv + 1)
                        assert a not in slab, "two park writes of a slab hit byte %d" % a
                        slab[a] = (rb * 16 + int(l16[ln_]), cb * 16 + 4 * int(grp[ln_]) + i)
                continue
            m = re.fullmatch(r"ds_read_b128 v\[(\d+):(\d+)\], v(\d+) offset:(\d+)", ln)
            if m and int(m.group(3)) in range(G.V_EADDR, G.V_EADDR + 4):
                if slab:
                    parks.append(slab)
                    slab = {}
                    emits.append([])
                emits[-1].append((int(m.group(3)), int(m.group(4))))
        out.append((parks, emits))
    return out


@pytest.mark.parametrize("kind", [k[0] for k in KINDS])
def test_park_writes_meet_the_emit_reads(kind):
    g = _kernel(kind)
    f32 = g.epi == G.EPI_F32
    esz, per = (4, 4) if f32 else (2, 8)                # bytes per element, elements per 16-byte emit read
    width = 64 if f32 else 128                            # columns of a slab
    maps = _slab_maps(kind)
    for wv, (parks, emits) in enumerate(maps):
        w = _waves_of(kind)[wv]
        assert len(parks) == len(emits) == (8 if f32 else 4)
        seen = set()
        for si, (slab, reads) in enumerate(zip(parks, emits)):
            rb32, h = (si >> 1, si & 1) if f32 else (si, 0)
            # the slab holds each (row, column) of its 32 x width block exactly once
            assert sorted(slab.values()) == [(rb32 * 32 + r, h * 64 + c) for r in range(32) for c in range(width)]
            assert len(reads) == 8
            for it, (areg, off) in enumerate(reads):
                for lane in range(64):
                    base = int(w.v[areg][lane]) + off
                    row, col0 = rb32 * 32 + it * 4 + lane // 16, h * 64 + (lane & 15) * per
                    for i in range(per):
                        assert slab[base + esz * i] == (row, col0 + i)
            seen |= set(slab.values())
        assert len(seen) == 128 * 128


def _makefile_assembler():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*\??=\s*(.+)$", mk, re.M))
    m = re.search(r"^gemm_asm\.co: gemm_asm\.s\n\t(.+)$", mk, re.M)
    cmd = m.group(1)
    for k, v in var.items():
        cmd = cmd.replace("$(%s)" % k, os.environ.get(k, v))
    return cmd


def test_generated_text_assembles(tmp_path):
    lines, meta = [], []
    for kind, _, _ in KINDS:
        g = _kernel(kind)
        lines += g.L
        meta.append(g.metadata())
    src = tmp_path / "gemm_asm.s"
    src.write_text(G.module_text(lines, meta))
    cmd = _makefile_assembler().replace("$<", str(src)).replace("gemm_asm_dev.o", str(tmp_path / "gemm_asm_dev.o"))
    assert "-x assembler" in cmd and "gfx950" in cmd
    r = subprocess.run(cmd, shell=True, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "gemm_asm_dev.o").stat().st_size > 0


def test_side_instructions_one_per_gap():
    """at most one side instruction per 16-cycle gap (a barrier with its wait, a branch with its return label count as one), a DMA
    piece alone in its gap with its m0 in the gap before, no two pieces in neighbouring gaps"""
    g = _kernel("gelu_ln")
    for zero in (False, True):
        slots = g.build_slots16(zero)
        assert len(slots) == 128
        dma = [i for i, s in enumerate(slots) if any("buffer_load_dwordx4" in x for x in s)]
        assert len(dma) == 16 and all(b - a >= 3 for a, b in zip(dma, dma[1:]))
        for i, s in enumerate(slots):
            real = [x for x in s if not x.endswith(":") and not x.startswith("s_waitcnt")]
            assert len(real) <= 1, (i, s)
            if i in dma:
                assert len(s) == 1 and slots[i - 1] and slots[i - 1][0].startswith("s_add_u32 m0")
    assert sum(len([x for x in s if not x.endswith(":")]) for s in g.build_slots16()) in range(76, 90)


@pytest.mark.parametrize("kind", ["f16", "gelu", "f16_ln", "gelu_ln"])
def test_epilogue_operand_lanes(kind):
    """bias (fp16 forms): a lane's four columns cb * 16 + 4 (lane >> 4) + 0..3; folded-LayerNorm consumer: the rank-1 operands come
    from lanes 0..15 only (k = 0..3 of v_mfma_f32_16x16x16_f16), rstd is the lane's own row"""
    g = _kernel(kind)
    lane = np.arange(64)
    text = "\n".join(g.L)
    for wv, w in enumerate(_waves_of(kind)):
        wr, wc = wv >> 1, wv & 1
        assert (w.v[G.V_TMP + 11] == (wc * 128 + 4 * (lane >> 4)) * 4).all()
        if not g.lnc:
            continue
        far = 16 * 512                                            # beyond the [N][8] / [M][8] fp16 fragment arrays of the launch
        for reg, blk in ((G.V_SFOFF, wc), (G.V_MFOFF, wr)):
            assert (w.v[reg][:16] == blk * 128 * 16 + 16 * lane[:16]).all() and (w.v[reg][16:] >= far).all()
        assert (w.v[G.V_RSOFF] == (wr * 128 + (lane & 15)) * 8 + 4).all()
    if g.lnc:
        upd = re.findall(r"v_mfma_f32_16x16x16_f16 a\[(\d+):\d+\], v\[(\d+):\d+\], v\[(\d+):\d+\], a\[(\d+):\d+\]", text)
        assert [(int(d), int(a), int(b)) for d, a, b, c in upd] == [((rb * 8 + cb) * 4, g.M16_SF + 2 * cb, g.M16_MF + 2 * rb) for rb in range(8) for cb in range(8)]
        for cb in range(8):
            assert "buffer_load_dwordx2 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (g.M16_SF + 2 * cb, g.M16_SF + 2 * cb + 1, G.V_SFOFF, G.SRD_SF, G.SRD_SF + 3, G.S_T2, cb * 256) in text


def _regs(tok):
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok.strip())
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


@pytest.mark.parametrize("kind", ["f16", "f32_ln"])
def test_counted_waits_cover_every_mfma_operand(kind):
    """LDS reads of a wave complete in issue order and `s_waitcnt lgkmcnt(n)` leaves at most n outstanding: walk the instructions as
    a wave executes them (the reads before the loop, a tile's first K-tile through the C = 0 copy, two more K-tiles through the loop
    body) and require that no MFMA reads a register an outstanding ds_read still has to write, and that no ds_read overwrites a
    fragment an MFMA of the same K-tile has yet to read."""
    g = _kernel(kind)
    L = [ln.strip() for ln in g.L]
    at = {ln[:-1]: i for i, ln in enumerate(L) if ln.endswith(":")}
    n = g.name
    begin, loop, after = at["L_tile_begin_%s" % n], at["L_loop_%s" % n], at["L_after_ks0_%s" % n]
    back = L.index("s_cbranch_scc0 L_loop_%s" % n)
    first_read = next(i for i, ln in enumerate(L) if ln.startswith("ds_read_b128"))
    jump = next(i for i in range(begin, loop) if L[i] == "s_branch L_after_ks0_%s" % n)
    stream = L[first_read:begin] + L[begin:jump] + L[after:back] + (L[loop:back]) * 2
    outstanding = []                                   # destination register sets, oldest first
    mfmas = reads = 0
    for ln in stream:
        if ln.startswith("s_waitcnt") and "lgkmcnt" in ln:
            k = int(re.search(r"lgkmcnt\((\d+)\)", ln).group(1))
            outstanding = outstanding[len(outstanding) - k:] if k < len(outstanding) else outstanding
            if k == 0:
                outstanding = []
        elif ln.startswith("ds_read_b128"):
            outstanding.append(_regs(ln.split(" ", 1)[1].split(",")[0]))
            reads += 1
        elif ln.startswith("v_mfma_f32_16x16x32_f16"):
            ops_ = re.findall(r"v\[\d+:\d+\]", ln)
            need = _regs(ops_[0]) | _regs(ops_[1])
            for dst in outstanding:
                assert not (dst & need), "an MFMA reads %s while a ds_read into it may be in flight: %s" % (sorted(dst & need), ln)
            mfmas += 1
    assert mfmas == 64 + 64 + 2 * 128 and reads == 16 + 3 * 32
    # write-after-read inside the loop body: a read into a fragment register comes after the last MFMA of this K-tile that uses it
    body = L[loop:back]
    last_use = {}
    for i, ln in enumerate(body):
        if ln.startswith("v_mfma_f32_16x16x32_f16"):
            ops_ = re.findall(r"v\[\d+:\d+\]", ln)
            for r in _regs(ops_[0]) | _regs(ops_[1]):
                last_use[r] = i
    for i, ln in enumerate(body):
        if ln.startswith("ds_read_b128"):
            dst = _regs(ln.split(" ", 1)[1].split(",")[0])
            ks1 = min(dst) >= G.V_SET[2]
            for r in dst:                               # k-step 1's registers are free from the previous K-tile's end, k-step 0's after MFMA 63
                assert ks1 or i > last_use[r]
            if ks1:
                first_use = min(j for j, l2 in enumerate(body) if l2.startswith("v_mfma") and (_regs(re.findall(r"v\[\d+:\d+\]", l2)[0]) | _regs(re.findall(r"v\[\d+:\d+\]", l2)[1])) & dst)
                assert i < first_use
