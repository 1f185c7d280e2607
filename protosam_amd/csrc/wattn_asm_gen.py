#!/usr/bin/env python3
"""Generator of the hand-written gfx950 window-attention kernel `psam_wattn_asm_80` (SAM ViT-H window blocks: 14 x 14 windows of the
64 x 64 token grid, hd = 80, softmax(q k^T * scale + rel_h + rel_w) v with the decomposed rel-pos terms computed in-kernel;
models/segment_anything/modeling/image_encoder.py:178-188 (window partition / unpartition as index math), :235-251, :337-372).

Why assembly: the HIP kernel (csrc/attention.hip wattn_p_kernel) compiles to ~1900 instructions per (window, head) item and wave - 540
of them scalar bookkeeping, every LDS fragment read awaited right behind its issue - on SIMDs that are instruction-issue bound.
This kernel does the same work in ~700, with a different arrangement of the window that removes most of the rel-pos machinery:

  * one persistent workgroup of 14 waves per CU walks a host-built list of (image, head, window) items; wave w owns the 14 queries of
    WINDOW ROW w (a 16-row MFMA query tile, two rows idle), and a 16-key MFMA tile is one window row of keys (14 keys + 2 masked slots);
  * so rel_h[q][ky] is ONE scalar per (query, key tile): it is folded into the exponent offset of that tile (like the global kernel's
    rel_h), computed per item by 6 MFMAs of the query tile against the wave's slice of the rel_pos_h table, pre-shifted by the wave's
    own row (no gather); and rel_w[q][kx] is the same 16 x 16 matrix for every key tile: it is computed once per item (12 MFMAs + a
    4-value gather through a wave-private LDS scratch), divided by the scale and used as the ACCUMULATOR INPUT of the first score MFMA
    of every tile (-inf in the two masked key slots): no bias arithmetic per score, no one-hot operands, no fp16 rounding of the bias;
  * K / V of an item arrive by LDS-DMA (`buffer_load_dwordx4 ... lds`) as [224 rows][80] fp16 images, K double-buffered one item ahead,
    V requested at the end of the previous item; per-lane source offsets and the exec masks of the pieces (valid slot / beyond the
    image's last row / last column -> the padded map's value, fp16(qkv bias)) come from a host-built table; every wave issues the
    same number of memory operations per item, so all waits are counted;
  * online softmax over chunks of four key tiles with a lazy rescale (only when a row maximum grows by more than 2^8), base-2 exponent,
    probabilities packed in place into the score registers (the B operand of the P V product as they stand), row sums by an all-ones
    MFMA, fragment reads several fragments ahead through one register ring.

Measured (16 slices: 6400 items, us per call; HIP wattn_p_kernel on the same box 340-355): 308. With parts left out (results
wrong): without the two barriers per item 273, without the K / V DMA 248, without both 218 (= the instruction streams alone), without any
arithmetic (DMA, query loads, stores, barriers only) 198, without the rel-pos prologue 270, without softmax 267, without P V / scores
277 / 273: the memory side and the arithmetic each take ~200 us and overlap only in part. Tried: the three images rotating (K, V,
next K) so that the next item's V pieces are requested right behind this item's last score MFMA instead of at its very end - needs a
third barrier per item: 341 us, dropped (the barriers of 14 waves cost more than the V pieces' flight time).

Layouts of the K / V images and of the transposing V reads are attention.hip's (wattn_kernel), with (tile, row) = (ky, kx).
Run through gemm_asm_gen.py (same code object).
"""

HD, RLD = 80, 160
WS, GW = 14, 64
NROW = 224                        # 14 key tiles of 16 slots
IMG = NROW * RLD                  # 35 840 bytes per K / V image
K0_BASE, K1_BASE, V_BASE = 0, IMG, 2 * IMG
TAB_BASE = 3 * IMG                # [2 tables][2 parts (hi, lo)][32 rows][160 bytes]
TAB_PART = 32 * RLD
SCR_BASE = TAB_BASE + 4 * TAB_PART
SCR_WAVE = 2304                   # per wave: [36 rows][16 queries] fp32 (rel_w gather; rows biased by 2), or [16 queries][16] (rel_h)
NW = 14
LDS_BYTES = SCR_BASE + NW * SCR_WAVE
NPIECE = 35                       # 64-lane DMA pieces per image (2240 slots of 16 bytes), 3 per wave (the third exists for waves 0..6)
GEOM_PIECES = 42                  # table rows per image (14 waves x 3)

# ---- SGPRs (102 available)
S_KARG = 0
S_WG = 2
S_QKV, S_OUT, S_RPK, S_PAD, S_WORK, S_GEOM = 4, 6, 8, 10, 12, 14
S_N, S_H, S_RS2, S_HS2, S_WS2, S_OROW, S_G, S_SL2, S_ISC = 16, 17, 18, 19, 20, 21, 22, 23, 24
SRD_K, SRD_V, SRD_Q, SRD_P, SRD_O = 28, 32, 36, 40, 44        # buffer descriptors (P: pad row of the image being loaded)
S_WV, S_CUR, S_STRIDE, S_ENT, S_ENTN = 48, 49, 50, 51, 52
S_CLASS = 53                      # edge class (2 ey + ex) the piece masks in S_MSK belong to
S_T0, S_T1, S_T2, S_T3, S_T4, S_T5 = 54, 55, 56, 57, 58, 59
S_KCUR, S_KNXT = 60, 61          # LDS byte offsets of the K buffer being read / being filled
S_M0P = 62                        # wave * 1024: this wave's first piece inside an image
S_IMGB = 63                       # bytes per image of qkv: N * rs2
S_QMASK, S_QMASK8 = 64, 66       # exec of the output stores: lanes with li < 14 / li < 8
S_G3 = 68                         # s[68:69]: lanes with g == 3
S_OCUR, S_ONXT = 70, 72          # s[70:71] / s[72:73]: output base of the item being computed / of the next one
S_CEY, S_CEX = 74, 75             # partial last row / column (0 / 1) of the item being computed
S_MSK = 76                        # s[76:99]: [img K, V][piece 0..2]{image lanes, pad lanes} x 2 dwords, for edge class S_CLASS
S_NEY, S_NEX = 100, 101           # the same flags of the next item
NUM_SGPR = 102

# ---- VGPRs (arch v0..63, accumulation registers a0..63: 128 per wave, four waves per SIMD)
V_TID, V_VQ, V_VQ2, V_VO, V_KRD, V_KRDN, V_VRD, V_TH, V_TW, V_SW, V_SG, V_SH = range(12)
V_DK, V_DV, V_C16 = 12, 15, 18
V_G = 21                          # lane >> 4
V_MRUN, V_MX = 22, 23
V_BH = 24                         # v24..39: rel_h * log2(e) per key tile (14 used; v38 / v39 double as temporaries)
V_RW = 40                         # v40..43: rel_w / scale of this lane's four key slots (-inf: masked)
V_S = 44                          # v44..59: scores of a chunk [tile][4]; packed probabilities in place
V_T = 60                          # v60..63 temporaries
V_T5, V_T6 = 38, 39
A_Q, A_RING, A_ONES, A_O, A_L = 0, 12, 36, 40, 60
RING = 6                          # fragment slots of four registers: a12..35
AH = 4                            # fragments requested ahead of their use

from asm_common import AsmWriter, LdsCounter, kernel_begin, kernel_end, kernel_metadata, module_text


class GenW(AsmWriter):
    def __init__(self, name="psam_wattn_asm_80"):
        AsmWriter.__init__(self, name)
        self.ldsq = LdsCounter(self.e)   # LDS operations complete in order: counted lgkmcnt waits
        self.frag_n = 0                  # fragments requested so far (ring slot = n % RING)

    # ------------------------------------------------------------------ LDS bookkeeping (asm_common.LdsCounter)
    def ds(self, text):
        return self.ldsq.issue(text)

    def need(self, op):
        self.ldsq.need(op)

    def ds_sync(self):
        self.ldsq.sync()

    def ds_reset(self):
        self.ldsq.reset()

    # ------------------------------------------------------------------ fragment ring
    def run_mfmas(self, ops):
        """ops: list of (kind, payload). kind "mfma": payload = (fmt, frag) - fmt has one %s for the fragment's registers, frag = a
        list of LDS read formats (each with one %s for its destination registers: 1 read of 4 registers or 2 of 2) or None; kind
        "raw": text. Fragment reads are issued AH fragments ahead of their MFMA through the ring."""
        frags = [(i, p[1]) for i, (k, p) in enumerate(ops) if k == "mfma" and p[1] is not None]
        issued = {}
        nxt = 0

        def issue(j):
            i, reads = frags[j]
            slot = A_RING + 4 * (self.frag_n % RING)
            self.frag_n += 1
            last = None
            if len(reads) == 1:
                last = self.ds(reads[0] % ("a[%d:%d]" % (slot, slot + 3)))
            else:
                self.ds(reads[0] % ("a[%d:%d]" % (slot, slot + 1)))
                last = self.ds(reads[1] % ("a[%d:%d]" % (slot + 2, slot + 3)))
            issued[i] = (slot, last)
        while nxt < min(AH, len(frags)):
            issue(nxt)
            nxt += 1
        for i, (k, p) in enumerate(ops):
            if k == "raw":
                if p.endswith(":"):
                    self.lab(p[:-1])
                elif p.startswith("//"):
                    self.c(p[2:].strip())
                else:
                    self.e(p)
                continue
            if k == "call":
                p()
                continue
            fmt, reads = p
            if reads is None:
                self.e(fmt)
                continue
            slot, last = issued[i]
            self.need(last)
            self.e(fmt % ("a[%d:%d]" % (slot, slot + 3)))
            if nxt < len(frags):
                issue(nxt)
                nxt += 1

    # ------------------------------------------------------------------ pieces of the program
    def entry_fields(self, ent):
        """b, h, wy, wx of a work-list entry -> S_T0 .. S_T3"""
        e = self.e
        e("s_and_b32 s%d, s%d, 0xff" % (S_T0, ent))                   # b
        e("s_bfe_u32 s%d, s%d, 0x80008" % (S_T1, ent))                # h
        e("s_bfe_u32 s%d, s%d, 0x80010" % (S_T2, ent))                # wy
        e("s_lshr_b32 s%d, s%d, 24" % (S_T3, ent))                    # wx

    def scalars_dma(self, ent):
        """entry `ent` (SGPR: b | h << 8 | wy << 16 | wx << 24, or -1: none) -> K / V / pad-row descriptors of the item to load (empty
        ranges when there is none) and the piece masks of its edge class"""
        e = self.e
        none, out, same = self.u("L_sd_none"), self.u("L_sd_out"), self.u("L_sd_same")
        e("s_cmp_eq_u32 s%d, -1" % ent)
        e("s_cbranch_scc1 %s" % none)
        self.entry_fields(ent)
        # edge class 2 * (wy == 4) + (wx == 4): the masks of the three pieces per image change with it (rarely: items are window-major)
        e("s_cmp_eq_u32 s%d, %d" % (S_T2, GW // WS))
        e("s_cselect_b32 s%d, 2, 0" % S_T4)
        e("s_cmp_eq_u32 s%d, %d" % (S_T3, GW // WS))
        e("s_cselect_b32 s%d, 1, 0" % S_T5)
        e("s_or_b32 s%d, s%d, s%d" % (S_T4, S_T4, S_T5))
        e("s_cmp_eq_u32 s%d, s%d" % (S_T4, S_CLASS))
        e("s_cbranch_scc1 %s" % same)
        e("s_mov_b32 s%d, s%d" % (S_CLASS, S_T4))
        for img in range(2):
            for i in range(3):
                # masks [class][img][42 pieces]{image lanes, pad lanes}: 16 bytes each, behind the three offset tables
                e("s_lshl_b32 s%d, s%d, 1" % (S_T5, S_CLASS))
                e("s_add_u32 s%d, s%d, %d" % (S_T5, S_T5, img))
                e("s_mul_i32 s%d, s%d, %d" % (S_T5, S_T5, GEOM_PIECES))
                e("s_add_u32 s%d, s%d, s%d" % (S_T5, S_T5, S_WV))
                e("s_add_u32 s%d, s%d, %d" % (S_T5, S_T5, i * NW))
                e("s_lshl_b32 s%d, s%d, 4" % (S_T5, S_T5))
                e("s_add_u32 s%d, s%d, %d" % (S_T5, S_T5, 3 * GEOM_PIECES * 256))
                m = S_MSK + (img * 3 + i) * 4
                e("s_load_dwordx4 s[%d:%d], s[%d:%d], s%d" % (m, m + 3, S_GEOM, S_GEOM + 1, S_T5))
        e("s_waitcnt lgkmcnt(0)")
        self.lab(same)
        # first token of the window: (wy * 14) * 64 + wx * 14
        e("s_mul_i32 s%d, s%d, %d" % (S_T2, S_T2, WS * GW))
        e("s_mul_i32 s%d, s%d, %d" % (S_T3, S_T3, WS))
        e("s_add_u32 s%d, s%d, s%d" % (S_T2, S_T2, S_T3))             # tok0
        # k: qkv + b * N * rs2 + tok0 * rs2 + h * hs2 + ws2; v: + ws2
        e("s_mul_i32 s%d, s%d, s%d" % (S_T4, S_T0, S_IMGB))
        e("s_mul_hi_u32 s%d, s%d, s%d" % (S_T5, S_T0, S_IMGB))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T3, S_T2, S_RS2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_T3))
        e("s_addc_u32 s%d, s%d, 0" % (S_T5, S_T5))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T3, S_T1, S_HS2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T3, S_T3, S_WS2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_T3))
        e("s_addc_u32 s%d, s%d, 0" % (S_T5, S_T5))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_K, S_QKV, S_T4))
        e("s_addc_u32 s%d, s%d, s%d" % (SRD_K + 1, S_QKV + 1, S_T5))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_V, SRD_K, S_WS2))
        e("s_addc_u32 s%d, s%d, 0" % (SRD_V + 1, SRD_K + 1))
        # ranges: to the end of this image (tokens of a partial window beyond it are masked to the pad row anyway)
        e("s_mul_i32 s%d, s%d, s%d" % (S_T4, S_T2, S_RS2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_T3))
        e("s_sub_u32 s%d, s%d, s%d" % (SRD_K + 2, S_IMGB, S_T4))
        e("s_sub_u32 s%d, s%d, s%d" % (SRD_V + 2, SRD_K + 2, S_WS2))
        # pad rows [3][H][80] fp16: k at (H + h) * 160 (the v row is H * 160 further: dma_image(1) moves the base)
        e("s_add_u32 s%d, s%d, s%d" % (S_T3, S_T1, S_H))
        e("s_mul_i32 s%d, s%d, %d" % (S_T3, S_T3, HD * 2))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_P, S_PAD, S_T3))
        e("s_addc_u32 s%d, s%d, 0" % (SRD_P + 1, S_PAD + 1))
        e("s_mov_b32 s%d, %d" % (SRD_P + 2, HD * 2))
        e("s_branch %s" % out)
        self.lab(none)
        for srd in (SRD_K, SRD_V, SRD_P):
            e("s_mov_b32 s%d, 0" % (srd + 2))
        self.lab(out)

    def scalars_compute(self, ent):
        """entry `ent` -> query descriptor, output base S_ONXT and edge flags S_NEY / S_NEX of that item (empty query range if none)"""
        e = self.e
        none, out = self.u("L_sc_none"), self.u("L_sc_out")
        e("s_cmp_eq_u32 s%d, -1" % ent)
        e("s_cbranch_scc1 %s" % none)
        self.entry_fields(ent)
        e("s_cmp_eq_u32 s%d, %d" % (S_T2, GW // WS))
        e("s_cselect_b32 s%d, 1, 0" % S_NEY)
        e("s_cmp_eq_u32 s%d, %d" % (S_T3, GW // WS))
        e("s_cselect_b32 s%d, 1, 0" % S_NEX)
        e("s_mul_i32 s%d, s%d, %d" % (S_T2, S_T2, WS * GW))
        e("s_mul_i32 s%d, s%d, %d" % (S_T3, S_T3, WS))
        e("s_add_u32 s%d, s%d, s%d" % (S_T2, S_T2, S_T3))             # tok0
        e("s_mul_i32 s%d, s%d, s%d" % (S_T4, S_T0, S_IMGB))
        e("s_mul_hi_u32 s%d, s%d, s%d" % (S_T5, S_T0, S_IMGB))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T3, S_T2, S_RS2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_T3))
        e("s_addc_u32 s%d, s%d, 0" % (S_T5, S_T5))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T3, S_T1, S_HS2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_T3))
        e("s_addc_u32 s%d, s%d, 0" % (S_T5, S_T5))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_Q, S_QKV, S_T4))
        e("s_addc_u32 s%d, s%d, s%d" % (SRD_Q + 1, S_QKV + 1, S_T5))
        # range: to the end of this image (query rows of a partial window beyond it read zeros; they are never stored)
        e("s_mul_i32 s%d, s%d, s%d" % (S_T4, S_T2, S_RS2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_T3))
        e("s_sub_u32 s%d, s%d, s%d" % (SRD_Q + 2, S_IMGB, S_T4))
        # out + (b * N + tok0) * orow + h * 160
        e("s_mul_i32 s%d, s%d, s%d" % (S_T4, S_T0, S_N))
        e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_T2))
        e("s_mul_hi_u32 s%d, s%d, s%d" % (S_T5, S_T4, S_OROW))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T4, S_T4, S_OROW))
        e("s_mul_i32 s%d, s%d, %d" % (S_T3, S_T1, HD * 2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_T3))
        e("s_addc_u32 s%d, s%d, 0" % (S_T5, S_T5))
        e("s_add_u32 s%d, s%d, s%d" % (S_ONXT, S_OUT, S_T4))
        e("s_addc_u32 s%d, s%d, s%d" % (S_ONXT + 1, S_OUT + 1, S_T5))
        e("s_branch %s" % out)
        self.lab(none)
        e("s_mov_b32 s%d, 0" % (SRD_Q + 2))
        self.lab(out)

    def dma_image(self, img, lds_base_sgpr, lds_base_const):
        """this wave's three pieces of the K (img 0) / V (img 1) image of the item whose descriptors are set: per piece one load from
        the token rows and one from the pad row under complementary exec masks (both counted by vmcnt in every wave: six per image)"""
        e = self.e
        srd = SRD_K if img == 0 else SRD_V
        voff = V_DK if img == 0 else V_DV
        if img == 1:      # the v pad row
            e("s_mul_i32 s%d, s%d, %d" % (S_T0, S_H, HD * 2))
            e("s_add_u32 s%d, s%d, s%d" % (SRD_P, SRD_P, S_T0))
            e("s_addc_u32 s%d, s%d, 0" % (SRD_P + 1, SRD_P + 1))
        def set_m0(i):
            if lds_base_sgpr is not None:
                e("s_add_u32 s%d, s%d, %d" % (S_T0, lds_base_sgpr, i * NW * 1024))
                e("s_add_u32 m0, s%d, s%d" % (S_T0, S_M0P))
            else:
                e("s_add_u32 m0, s%d, %d" % (S_M0P, lds_base_const + i * NW * 1024))
        for i in range(3):
            m = S_MSK + (img * 3 + i) * 4
            set_m0(i)
            e("s_mov_b64 exec, s[%d:%d]" % (m, m + 1))
            e("buffer_load_dwordx4 v%d, s[%d:%d], 0 offen lds" % (voff + i, srd, srd + 3))
        # the pad-row pieces exist only for windows with a partial last row / column (9 of 25): every wave of the workgroup takes
        # the same branch, and the counted waits use the smaller number of requests (a stricter wait where the pad pieces exist)
        nopad = self.u("L_nopad")
        e("s_cmp_eq_u32 s%d, 0" % S_CLASS)
        e("s_cbranch_scc1 %s" % nopad)
        for i in range(3):
            m = S_MSK + (img * 3 + i) * 4
            set_m0(i)
            e("s_mov_b64 exec, s[%d:%d]" % (m + 2, m + 3))
            e("buffer_load_dwordx4 v%d, s[%d:%d], 0 offen lds" % (V_C16 + i, SRD_P, SRD_P + 3))
        self.lab(nopad)
        e("s_mov_b64 exec, -1")

    def q_loads(self):
        """query fragments of the item whose Q descriptor is set: [k-step] 8 halfs at token (row w, column li), column s * 32 + g * 8;
        k-step 2: the lanes g >= 2 read beyond the buffer (zeros)"""
        e = self.e
        for s in range(3):
            r = A_Q + 4 * s
            if s < 2:
                e("buffer_load_dwordx4 a[%d:%d], v%d, s[%d:%d], 0 offen offset:%d" % (r, r + 3, V_VQ, SRD_Q, SRD_Q + 3, s * 64))
            else:
                e("buffer_load_dwordx4 a[%d:%d], v%d, s[%d:%d], 0 offen" % (r, r + 3, V_VQ2, SRD_Q, SRD_Q + 3))

    def k_frag(self, T, s):
        return ["ds_read_b128 %%s, v%d offset:%d" % (V_KRD, T * 16 * RLD + s * 64)]

    def v_frag(self, u, dt):
        off = u * 32 * RLD + dt * 32
        return ["ds_read_b64_tr_b16 %%s, v%d offset:%d" % (V_VRD, off), "ds_read_b64_tr_b16 %%s, v%d offset:%d" % (V_VRD, off + 8 * RLD)]

    def prologue_relpos(self):
        """rel_h * log2(e) of the 14 key rows into V_BH, rel_w / scale of this lane's four key slots into V_RW"""
        e = self.e
        self.c("---- rel-pos terms of this wave's query row")
        # rel_h: D[j][q] = q . Rh[w + 13 - j] (table rows pre-shifted by this wave's row: V_TH), hi + lo parts
        ops = []
        first = True
        for part in range(2):
            for s in range(3):
                fmt = "v_mfma_f32_16x16x32_f16 v[%d:%d], %%s, a[%d:%d], %s" % (V_S, V_S + 3, A_Q + 4 * s, A_Q + 4 * s + 3,
                                                                             "0" if first else "v[%d:%d]" % (V_S, V_S + 3))
                ops.append(("mfma", (fmt, ["ds_read_b128 %%s, v%d offset:%d" % (V_TH, part * TAB_PART + s * 64)])))
                first = False
        # rel_w: D[j][q] = q . Rw[j], j = tile * 16 + MFMA row
        for t in range(2):
            first = True
            d = V_S + 4 + 4 * t
            for part in range(2):
                for s in range(3):
                    fmt = "v_mfma_f32_16x16x32_f16 v[%d:%d], %%s, a[%d:%d], %s" % (d, d + 3, A_Q + 4 * s, A_Q + 4 * s + 3,
                                                                                 "0" if first else "v[%d:%d]" % (d, d + 3))
                    ops.append(("mfma", (fmt, ["ds_read_b128 %%s, v%d offset:%d" % (V_TW, t * 16 * RLD + part * TAB_PART + s * 64)])))
                    first = False
        self.run_mfmas(ops)
        e("s_nop 7")
        e("s_nop 7")
        # rel_h: [q][ky] through the scratch (one 16-byte write, four 16-byte reads: every lane of a query gets all 16 values)
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_T, V_G, V_SH))
        self.ds("ds_write_b128 v%d, v[%d:%d]" % (V_T, V_S, V_S + 3))
        rd = None
        for i in range(4):
            rd = self.ds("ds_read_b128 v[%d:%d], v%d offset:%d" % (V_BH + 4 * i, V_BH + 4 * i + 3, V_SH, i * 16))
        # rel_w: rows j + 2 of the scratch (written behind the rel_h reads: LDS operations of a wave complete in order)
        for t in range(2):
            d = V_S + 4 + 4 * t
            if t == 1:
                e("v_add_u32 v%d, 1024, v%d" % (V_T, V_SW))
            a = V_SW if t == 0 else V_T
            self.ds("ds_write2_b32 v%d, v%d, v%d offset1:16" % (a, d, d + 1))
            self.ds("ds_write2_b32 v%d, v%d, v%d offset0:32 offset1:48" % (a, d + 2, d + 3))
        g = None
        for r in range(4):       # key slot kx = 4 g + r  <-  D[li + 13 - kx]
            g = self.ds("ds_read_b32 v%d, v%d offset:%d" % (V_RW + r, V_SG, (3 - r) * 64))
        self.need(rd)
        for i in range(14):
            e("v_mul_f32 v%d, 0x3fb8aa3b, v%d" % (V_BH + i, V_BH + i))                            # * log2(e)
        self.need(g)
        for r in range(4):
            e("v_mul_f32 v%d, s%d, v%d" % (V_RW + r, S_ISC, V_RW + r))                             # / scale
        e("s_mov_b64 exec, s[%d:%d]" % (S_G3, S_G3 + 1))                                           # key slots 14 / 15 do not exist
        e("v_mov_b32 v%d, 0xff800000" % (V_RW + 2))
        e("v_mov_b32 v%d, 0xff800000" % (V_RW + 3))
        e("s_mov_b64 exec, -1")

    def chunk_ops(self, T0, nt, first, last_qk_hook=None):
        """key tiles T0 .. T0 + nt - 1 (nt = 4 or 2) as two operation lists for run_mfmas: [scores, softmax] and [P V]. The lists of the
        whole item are run as ONE stream (kernel()), so that the fragment reads of a phase are requested AH fragments ahead, i.e. from
        inside the previous phase: they are in flight during the softmax arithmetic / the tail of the previous MFMA run."""
        A, B = [], []
        raw = lambda t: A.append(("raw", t))
        raw("// ---- key tiles %d..%d" % (T0, T0 + nt - 1))
        for s in range(3):
            for t in range(nt):
                d = V_S + 4 * t
                c = "v[%d:%d]" % (V_RW, V_RW + 3) if s == 0 else "v[%d:%d]" % (d, d + 3)
                fmt = "v_mfma_f32_16x16x32_f16 v[%d:%d], %%s, a[%d:%d], %s" % (d, d + 3, A_Q + 4 * s, A_Q + 4 * s + 3, c)
                A.append(("mfma", (fmt, self.k_frag(T0 + t, s))))
        if last_qk_hook:
            A.append(("call", last_qk_hook))
        raw("s_nop 7")
        raw("s_nop 7")
        # row maxima in the exponent domain: max_r(s) * scale log2(e) + rel_h log2(e)
        mt = [V_T + i for i in range(4)]
        for t in range(nt):
            s0 = V_S + 4 * t
            raw("v_max3_f32 v%d, v%d, v%d, v%d" % (mt[t], s0, s0 + 1, s0 + 2))
        for t in range(nt):
            raw("v_max_f32 v%d, v%d, v%d" % (mt[t], mt[t], V_S + 4 * t + 3))
        for t in range(nt):
            raw("v_fma_f32 v%d, v%d, s%d, v%d" % (mt[t], mt[t], S_SL2, V_BH + T0 + t))
        if nt == 4:
            raw("v_max3_f32 v%d, v%d, v%d, v%d" % (V_MX, mt[0], mt[1], mt[2]))
            raw("v_max_f32 v%d, v%d, v%d" % (V_MX, V_MX, mt[3]))
        else:
            raw("v_max_f32 v%d, v%d, v%d" % (V_MX, mt[0], mt[1]))
        # the four lanes of a query hold different keys: the first chunk reduces its maxima across them (the running maximum starts
        # there); later chunks compare per lane - the offset only has to keep the exponentials in range - and reduce inside the
        # (rare) rescale
        for swap in (("v_permlane16_swap_b32", "v_permlane32_swap_b32") if first else ()):
            raw("v_mov_b32 v%d, v%d" % (V_T5, V_MX))
            raw("v_mov_b32 v%d, v%d" % (V_T6, V_MX))
            raw("s_nop 1")
            raw("%s v%d, v%d" % (swap, V_T5, V_T6))
            raw("v_max_f32 v%d, v%d, v%d" % (V_MX, V_T5, V_T6))
        tag = "c%d" % T0
        if first:
            raw("v_mov_b32 v%d, v%d" % (V_MRUN, V_MX))
        else:
            # lazy rescale: only when some row's maximum grew by more than 2^8 (the probabilities stay below 2^8 otherwise)
            raw("v_add_f32 v%d, 0x41000000, v%d" % (V_T, V_MRUN))
            raw("v_cmp_gt_f32 vcc, v%d, v%d" % (V_MX, V_T))
            raw("s_cbranch_vccnz L_resc_%s_%s" % (tag, self.name))
            raw("L_resc_ret_%s_%s:" % (tag, self.name))
            self.resc_tags.append(tag)
        off = [V_T + i for i in range(4)]
        for t in range(nt):
            raw("v_sub_f32 v%d, v%d, v%d" % (off[t], V_BH + T0 + t, V_MRUN))
        for t in range(nt):
            s0 = V_S + 4 * t
            for r in range(4):
                raw("v_fma_f32 v%d, v%d, s%d, v%d" % (s0 + r, s0 + r, S_SL2, off[t]))
            for r in range(4):
                raw("v_exp_f32 v%d, v%d" % (s0 + r, s0 + r))
        for u in range(nt // 2):      # packed in place: k-slots 0..3 = tile 2u, 4..7 = tile 2u + 1  ->  the four registers of tile 2u
            a, b = V_S + 8 * u, V_S + 8 * u + 4
            raw("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (a, a, a + 1))
            raw("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (a + 1, a + 2, a + 3))
            raw("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (a + 2, b, b + 1))
            raw("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (a + 3, b + 2, b + 3))
        if first:
            # V of this item complete in every wave: the only younger requests of this wave are the next item's six K pieces
            raw("s_waitcnt vmcnt(3)")          # (three or six K pieces of the next item are younger)
            raw("s_barrier")
        raw("s_nop 4")            # VALU write (the packed probabilities) -> MFMA operand read: wait states (the MFMA reads stale data otherwise)
        for uu in range(nt // 2):
            u = T0 // 2 + uu
            p = V_S + 8 * uu
            zero = first and uu == 0
            B.append(("mfma", ("v_mfma_f32_16x16x32_f16 a[%d:%d], a[%d:%d], v[%d:%d], %s" % (
                A_L, A_L + 3, A_ONES, A_ONES + 3, p, p + 3, "0" if zero else "a[%d:%d]" % (A_L, A_L + 3)), None)))
            for dt in range(5):
                o = A_O + 4 * dt
                fmt = "v_mfma_f32_16x16x32_f16 a[%d:%d], %%s, v[%d:%d], %s" % (o, o + 3, p, p + 3, "0" if zero else "a[%d:%d]" % (o, o + 3))
                B.append(("mfma", (fmt, self.v_frag(u, dt))))
        return A, B

    def rescale_routine(self, tag):
        e = self.e
        self.lab("L_resc_%s_%s" % (tag, self.name))
        for swap in ("v_permlane16_swap_b32", "v_permlane32_swap_b32"):
            e("v_mov_b32 v%d, v%d" % (V_T5, V_MX))
            e("v_mov_b32 v%d, v%d" % (V_T6, V_MX))
            e("s_nop 1")
            e("%s v%d, v%d" % (swap, V_T5, V_T6))
            e("s_nop 1")
            e("v_max_f32 v%d, v%d, v%d" % (V_MX, V_T5, V_T6))
        e("v_max_f32 v%d, v%d, v%d" % (V_T, V_MRUN, V_MX))
        e("v_sub_f32 v%d, v%d, v%d" % (V_T + 1, V_MRUN, V_T))
        e("v_mov_b32 v%d, v%d" % (V_MRUN, V_T))
        e("v_exp_f32 v%d, v%d" % (V_T + 1, V_T + 1))
        e("s_nop 7")
        e("s_nop 7")
        for r in list(range(A_L, A_L + 4)) + list(range(A_O, A_O + 20)):
            e("v_accvgpr_read_b32 v%d, a%d" % (V_T + 2, r))
            e("s_nop 0")
            e("v_mul_f32 v%d, v%d, v%d" % (V_T + 2, V_T + 2, V_T + 1))
            e("s_nop 0")
            e("v_accvgpr_write_b32 a%d, v%d" % (r, V_T + 2))
        e("s_nop 3")
        e("s_branch L_resc_ret_%s_%s" % (tag, self.name))

    # ------------------------------------------------------------------ kernel
    def kernel(self):
        e, n = self.e, self.name
        self.resc_tags = []
        self.L += kernel_begin(n)
        e("s_load_dwordx16 s[4:19], s[0:1], 0x0")
        e("s_load_dwordx8 s[20:27], s[0:1], 0x40")
        e("v_lshrrev_b32 v%d, 6, v0" % V_T)
        e("s_nop 1")
        e("v_readfirstlane_b32 s%d, v%d" % (S_WV, V_T))
        e("s_waitcnt lgkmcnt(0)")
        for srd in (SRD_K, SRD_V, SRD_Q, SRD_P, SRD_O):
            e("s_mov_b32 s%d, 0x00020000" % (srd + 3))
            e("s_mov_b32 s%d, 0" % (srd + 2))
        e("s_mul_i32 s%d, s%d, s%d" % (S_IMGB, S_N, S_RS2))
        e("s_lshl_b32 s%d, s%d, 10" % (S_M0P, S_WV))
        e("s_mov_b32 s%d, -1" % S_CLASS)
        e("s_lshl_b32 s%d, s2, 2" % S_CUR)
        e("s_lshl_b32 s%d, s%d, 2" % (S_STRIDE, S_G))
        e("s_load_dword s%d, s[%d:%d], s%d" % (S_ENT, S_WORK, S_WORK + 1, S_CUR))
        e("s_add_u32 s%d, s%d, s%d" % (S_CUR, S_CUR, S_STRIDE))
        e("s_load_dword s%d, s[%d:%d], s%d" % (S_ENTN, S_WORK, S_WORK + 1, S_CUR))
        # ---- zero the whole LDS (pad slots of the images stay zero: no DMA piece writes them; fragment reads of the last k-step
        #      run 32 bytes past a row), then copy the rel-pos tables
        for i in range(4):
            e("v_mov_b32 v%d, 0" % (V_S + i))
        e("v_lshlrev_b32 v%d, 4, v0" % V_T)                            # tid * 16
        PASS = NW * 64 * 16
        nz = (LDS_BYTES + PASS - 1) // PASS
        for i in range(nz):
            if (i + 1) * PASS > LDS_BYTES:                             # last pass: only the threads still inside
                e("v_cmp_gt_u32 vcc, %d, v%d" % (LDS_BYTES - i * PASS, V_T))
                e("s_and_b64 exec, exec, vcc")
            if i * PASS < 65536:
                e("ds_write_b128 v%d, v[%d:%d] offset:%d" % (V_T, V_S, V_S + 3, i * PASS))
            else:
                if (i - 1) * PASS < 65536:
                    e("v_add_u32 v%d, %d, v%d" % (V_T + 1, i * PASS, V_T))
                else:
                    e("v_add_u32 v%d, %d, v%d" % (V_T + 1, PASS, V_T + 1))
                e("ds_write_b128 v%d, v[%d:%d]" % (V_T + 1, V_S, V_S + 3))
        e("s_mov_b64 exec, -1")
        e("s_waitcnt lgkmcnt(0)")
        e("s_barrier")
        # tables: global [4][32][96 halfs] -> LDS [4][32][160 bytes]: chunk id = tid + pass * 896 < 1280: row = id / 10, c = id % 10
        e("s_mov_b32 s%d, s%d" % (SRD_O, S_RPK)); e("s_mov_b32 s%d, s%d" % (SRD_O + 1, S_RPK + 1)); e("s_mov_b32 s%d, %d" % (SRD_O + 2, 4 * 32 * 192))
        e("s_mov_b32 s%d, 0xcccccccd" % S_T0)
        for p in range(2):
            e("v_add_u32 v%d, %d, v0" % (V_T, p * NW * 64))
            e("v_mul_hi_u32 v%d, v%d, s%d" % (V_T + 1, V_T, S_T0))
            e("v_lshrrev_b32 v%d, 3, v%d" % (V_T + 1, V_T + 1))        # row
            e("v_mul_u32_u24 v%d, 10, v%d" % (V_T + 2, V_T + 1))
            e("v_sub_u32 v%d, v%d, v%d" % (V_T + 2, V_T, V_T + 2))     # c
            e("v_cmp_gt_u32 vcc, 1280, v%d" % V_T)
            e("s_and_b64 exec, exec, vcc")
            e("v_mul_u32_u24 v%d, 192, v%d" % (V_S, V_T + 1))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_S, V_T + 2, V_S))          # source: row * 192 + c * 16
            e("v_mul_u32_u24 v%d, %d, v%d" % (V_S + 1, RLD, V_T + 1))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_S + 1, V_T + 2, V_S + 1))  # LDS: row * 160 + c * 16
            e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen" % (V_S + 4, V_S + 7, V_S, SRD_O, SRD_O + 3))
            e("s_waitcnt vmcnt(0)")
            e("v_add_u32 v%d, %d, v%d" % (V_S + 1, TAB_BASE, V_S + 1))
            e("ds_write_b128 v%d, v[%d:%d]" % (V_S + 1, V_S + 4, V_S + 7))
            e("s_mov_b64 exec, -1")
        # ---- lane constants
        LI = V_T + 3
        e("v_and_b32 v%d, 63, v0" % V_T)
        e("v_and_b32 v%d, 15, v%d" % (LI, V_T))
        e("v_lshrrev_b32 v%d, 4, v%d" % (V_G, V_T))
        # query token of this lane: (w * 64 + li); V_VQ = tok * rs2 + g * 16, V_VO = tok * orow + g * 8
        e("s_lshl_b32 s%d, s%d, 6" % (S_T0, S_WV))
        e("v_add_u32 v%d, s%d, v%d" % (V_T, S_T0, LI))
        e("v_mul_lo_u32 v%d, v%d, s%d" % (V_VQ, V_T, S_RS2))
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_VQ, V_G, V_VQ))
        e("v_add_u32 v%d, 128, v%d" % (V_VQ2, V_VQ))
        e("v_mov_b32 v%d, 0x40000000" % (V_T + 1))
        e("v_cmp_gt_u32 vcc, 2, v%d" % V_G)
        e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (V_VQ2, V_T + 1, V_VQ2))
        e("v_mul_lo_u32 v%d, v%d, s%d" % (V_VO, V_T, S_OROW))
        e("v_lshl_add_u32 v%d, v%d, 3, v%d" % (V_VO, V_G, V_VO))
        # K fragment reads: li * 160 + g * 16 (+ buffer)
        e("v_mul_u32_u24 v%d, %d, v%d" % (V_KRD, RLD, LI))
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_KRD, V_G, V_KRD))
        e("v_add_u32 v%d, %d, v%d" % (V_KRDN, K1_BASE, V_KRD))
        # rel-pos table reads: rel_w rows li, rel_h rows clamp(w + 13 - li, 0)
        e("v_add_u32 v%d, %d, v%d" % (V_TW, TAB_BASE + 2 * TAB_PART, V_KRD))
        e("s_add_u32 s%d, s%d, 13" % (S_T0, S_WV))
        e("v_sub_u32 v%d, s%d, v%d" % (V_T, S_T0, LI))
        e("v_max_i32 v%d, 0, v%d" % (V_T, V_T))
        e("v_mul_u32_u24 v%d, %d, v%d" % (V_TH, RLD, V_T))
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_TH, V_G, V_TH))
        e("v_add_u32 v%d, %d, v%d" % (V_TH, TAB_BASE, V_TH))
        # V fragment reads (transposing): row (g >> 1) * 16 + (g & 1) * 4 + (li >> 2), + (li & 3) * 8 bytes
        e("v_lshrrev_b32 v%d, 1, v%d" % (V_T, V_G))
        e("v_lshlrev_b32 v%d, 4, v%d" % (V_T, V_T))
        e("v_and_b32 v%d, 1, v%d" % (V_T + 1, V_G))
        e("v_lshl_add_u32 v%d, v%d, 2, v%d" % (V_T, V_T + 1, V_T))
        e("v_lshrrev_b32 v%d, 2, v%d" % (V_T + 1, LI))
        e("v_add_u32 v%d, v%d, v%d" % (V_T, V_T, V_T + 1))
        e("v_mul_u32_u24 v%d, %d, v%d" % (V_T, RLD, V_T))
        e("v_and_b32 v%d, 3, v%d" % (V_T + 1, LI))
        e("v_lshl_add_u32 v%d, v%d, 3, v%d" % (V_VRD, V_T + 1, V_T))
        e("v_add_u32 v%d, %d, v%d" % (V_VRD, V_BASE, V_VRD))
        # scratch of this wave
        e("s_mul_i32 s%d, s%d, %d" % (S_T0, S_WV, SCR_WAVE))
        e("s_add_u32 s%d, s%d, %d" % (S_T0, S_T0, SCR_BASE))
        e("v_lshlrev_b32 v%d, 6, v%d" % (V_SH, LI))                       # rel_h: [q][16] fp32
        e("v_add_u32 v%d, s%d, v%d" % (V_SH, S_T0, V_SH))
        e("v_lshl_add_u32 v%d, v%d, 2, 2" % (V_T, V_G))                   # rel_w write: row 4 g + 2 (+ r), column li
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_T, V_T, LI))
        e("v_lshlrev_b32 v%d, 2, v%d" % (V_T, V_T))
        e("v_add_u32 v%d, s%d, v%d" % (V_SW, S_T0, V_T))
        e("v_lshlrev_b32 v%d, 2, v%d" % (V_T, V_G))                       # rel_w gather: row li + 13 - (4 g + 3) + 2 for r = 3
        e("v_sub_u32 v%d, v%d, v%d" % (V_T, LI, V_T))
        e("v_add_u32 v%d, 12, v%d" % (V_T, V_T))
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_T, V_T, LI))
        e("v_lshlrev_b32 v%d, 2, v%d" % (V_T, V_T))
        e("v_add_u32 v%d, s%d, v%d" % (V_SG, S_T0, V_T))
        # exec masks: output stores (li < 14, li < 8), lanes g == 3
        e("v_cmp_gt_u32 vcc, 14, v%d" % LI)
        e("s_mov_b64 s[%d:%d], vcc" % (S_QMASK, S_QMASK + 1))
        e("v_cmp_gt_u32 vcc, 8, v%d" % LI)
        e("s_mov_b64 s[%d:%d], vcc" % (S_QMASK8, S_QMASK8 + 1))
        e("v_cmp_eq_u32 vcc, 3, v%d" % V_G)
        e("s_mov_b64 s[%d:%d], vcc" % (S_G3, S_G3 + 1))
        # ---- DMA source offsets of this wave's pieces (host table): K offsets [42][64], V offsets [42][64], pad offsets [42][64]
        e("s_mov_b32 s%d, s%d" % (SRD_O, S_GEOM)); e("s_mov_b32 s%d, s%d" % (SRD_O + 1, S_GEOM + 1))
        e("s_mov_b32 s%d, %d" % (SRD_O + 2, 3 * GEOM_PIECES * 256))
        e("v_and_b32 v%d, 63, v0" % V_T)
        e("v_lshlrev_b32 v%d, 2, v%d" % (V_T, V_T))
        for i in range(3):
            e("s_add_u32 s%d, s%d, %d" % (S_T0, S_WV, i * NW))           # piece
            e("s_lshl_b32 s%d, s%d, 8" % (S_T0, S_T0))
            e("buffer_load_dword v%d, v%d, s[%d:%d], s%d offen" % (V_DK + i, V_T, SRD_O, SRD_O + 3, S_T0))
            e("s_add_u32 s%d, s%d, %d" % (S_T1, S_T0, GEOM_PIECES * 256))
            e("buffer_load_dword v%d, v%d, s[%d:%d], s%d offen" % (V_DV + i, V_T, SRD_O, SRD_O + 3, S_T1))
            e("s_add_u32 s%d, s%d, %d" % (S_T1, S_T0, 2 * GEOM_PIECES * 256))
            e("buffer_load_dword v%d, v%d, s[%d:%d], s%d offen" % (V_C16 + i, V_T, SRD_O, SRD_O + 3, S_T1))
        e("v_mov_b32 v%d, 0x3c003c00" % V_T)
        for i in range(4):
            e("v_accvgpr_write_b32 a%d, v%d" % (A_ONES + i, V_T))
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")
        e("s_mov_b32 s%d, 0" % (SRD_O + 2))
        e("s_mov_b32 s%d, %d" % (S_KCUR, K0_BASE))
        e("s_mov_b32 s%d, %d" % (S_KNXT, K1_BASE))
        e("s_barrier")                                                    # tables in place
        # ---- first item: K, V, Q
        e("s_cmp_eq_u32 s%d, -1" % S_ENT)
        e("s_cbranch_scc1 L_exit_%s" % n)
        self.scalars_dma(S_ENT)
        self.dma_image(0, S_KCUR, None)
        self.dma_image(1, None, V_BASE)
        self.scalars_compute(S_ENT)
        self.q_loads()
        e("s_mov_b64 s[%d:%d], s[%d:%d]" % (S_OCUR, S_OCUR + 1, S_ONXT, S_ONXT + 1))
        e("s_mov_b32 s%d, s%d" % (S_CEY, S_NEY))
        e("s_mov_b32 s%d, s%d" % (S_CEX, S_NEX))
        e("s_waitcnt vmcnt(0)")
        e("s_barrier")
        # ---- the item loop
        self.lab("L_item_%s" % n)
        self.ldsq.n, self.ldsq.done, self.frag_n = 0, -1, 0
        # requests for the next item: its K image into the other buffer
        self.scalars_dma(S_ENTN)
        self.dma_image(0, S_KNXT, None)
        self.prologue_relpos()

        def after_last_qk():
            # the query fragments of the next item may land in the registers now (no score MFMA of this item is left)
            self.scalars_compute(S_ENTN)
            self.q_loads()
        a0, b0 = self.chunk_ops(0, 4, True)
        self.run_mfmas(a0)                     # (no V read before the barrier at its end)
        rest = b0
        for (T0, nt, hook) in ((4, 4, None), (8, 4, None), (12, 2, after_last_qk)):
            a, b = self.chunk_ops(T0, nt, False, hook)
            rest += a + b
        self.run_mfmas(rest)
        # ---- output: O / l -> fp16, 8-byte stores out[q][h * 80 + dt * 16 + g * 4 .. + 3]
        self.ds_sync()
        e("s_nop 7")
        e("s_nop 7")
        e("v_accvgpr_read_b32 v%d, a%d" % (V_T, A_L))
        e("s_mov_b64 s[%d:%d], s[%d:%d]" % (SRD_O, SRD_O + 1, S_OCUR, S_OCUR + 1))
        e("s_mov_b32 s%d, 0x20000000" % (SRD_O + 2))
        e("v_rcp_f32 v%d, v%d" % (V_T, V_T))
        # exec of the stores: li < 14 (li < 8 in a partial last window column); nothing for a wave whose row is beyond the image
        e("s_cmp_eq_u32 s%d, 0" % S_CEX)
        e("s_cselect_b64 s[%d:%d], s[%d:%d], s[%d:%d]" % (S_T0, S_T0 + 1, S_QMASK, S_QMASK + 1, S_QMASK8, S_QMASK8 + 1))
        e("s_cmp_lt_u32 s%d, 8" % S_WV)
        e("s_cselect_b32 s%d, 1, 0" % S_T2)                              # row inside a partial last window row
        e("s_xor_b32 s%d, s%d, 1" % (S_T3, S_CEY))
        e("s_or_b32 s%d, s%d, s%d" % (S_T2, S_T2, S_T3))                 # 1: store
        e("s_cmp_eq_u32 s%d, 0" % S_T2)
        e("s_cselect_b64 s[%d:%d], 0, s[%d:%d]" % (S_T0, S_T0 + 1, S_T0, S_T0 + 1))
        for dt in range(5):
            o = A_O + 4 * dt
            for j in range(4):
                e("v_accvgpr_read_b32 v%d, a%d" % (V_S + j, o + j))
            e("s_nop 1")
            for j in range(4):
                e("v_mul_f32 v%d, v%d, v%d" % (V_S + j, V_S + j, V_T))
            e("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (V_S + 4 + 2 * dt, V_S, V_S + 1))
            e("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (V_S + 5 + 2 * dt, V_S + 2, V_S + 3))
        e("s_mov_b64 exec, s[%d:%d]" % (S_T0, S_T0 + 1))
        for dt in range(5):           # (five stores in every wave, under an empty exec mask where there is nothing to store: counted waits)
            e("buffer_store_dwordx2 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d" % (V_S + 4 + 2 * dt, V_S + 5 + 2 * dt, V_VO, SRD_O, SRD_O + 3, dt * 32))
        e("s_mov_b64 exec, -1")
        # ---- end of the item: the next item's K pieces (older than its 3 query loads and the 5 stores) have landed; every wave is
        #      done with K / V of this item
        e("s_waitcnt vmcnt(8)")
        e("s_barrier")
        e("s_cmp_eq_u32 s%d, -1" % S_ENTN)
        e("s_cbranch_scc1 L_exit_%s" % n)
        # V of the next item (the descriptors of the loaded item are still set), then advance
        self.dma_image(1, None, V_BASE)
        e("s_mov_b32 s%d, s%d" % (S_T0, S_KCUR))
        e("s_mov_b32 s%d, s%d" % (S_KCUR, S_KNXT))
        e("s_mov_b32 s%d, s%d" % (S_KNXT, S_T0))
        e("v_swap_b32 v%d, v%d" % (V_KRD, V_KRDN))
        e("s_mov_b64 s[%d:%d], s[%d:%d]" % (S_OCUR, S_OCUR + 1, S_ONXT, S_ONXT + 1))
        e("s_mov_b32 s%d, s%d" % (S_CEY, S_NEY))
        e("s_mov_b32 s%d, s%d" % (S_CEX, S_NEX))
        e("s_mov_b32 s%d, s%d" % (S_ENT, S_ENTN))
        e("s_add_u32 s%d, s%d, s%d" % (S_CUR, S_CUR, S_STRIDE))
        e("s_load_dword s%d, s[%d:%d], s%d" % (S_ENTN, S_WORK, S_WORK + 1, S_CUR))
        # the query fragments of the new item (requested before the five stores, the barrier and the V pieces)
        e("s_waitcnt vmcnt(8) lgkmcnt(0)")   # (five stores and three or six V pieces are younger)
        e("s_branch L_item_%s" % n)
        self.lab("L_exit_%s" % n)
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")
        e("s_endpgm")
        for tag in self.resc_tags:
            self.rescale_routine(tag)
        self.L += kernel_end(n, LDS_BYTES, 96, NUM_SGPR, next_free_vgpr=128, accum_offset=64)

    def metadata(self):
        # kernarg: WattnAsmArgs of csrc/attention.hip (six pointers, twelve 32-bit values)
        return kernel_metadata(self.name, ["ptr"] * 6 + ["i32"] * 12, LDS_BYTES, NUM_SGPR, vgprs=128, agprs=64, wg_size=NW * 64)


def build_all():
    g = GenW()
    g.kernel()
    return g.L, [g.metadata()]


if __name__ == "__main__":
    import sys
    sys.stdout.write(module_text(*build_all()))
