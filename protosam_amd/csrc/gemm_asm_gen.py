#!/usr/bin/env python3
"""Generator of the hand-scheduled gfx950 (CDNA4) assembly GEMM behind psam_gemm_f16 (tile 15).

out[M,N] = epilogue(A[M,K] . W[N,K]^T), fp16 operands (K contiguous), fp32 accumulation: the Linear layers of
/root/reference/models/segment_anything/modeling/image_encoder.py:223-249 and common.py:13-26.

Why assembly: three HIP schedules of this GEMM (csrc/gemm.hip tiles 10 / 11 / 13) sit at ~2900 cycles per 256x256x64
K-tile against 2048 of MFMA issue; what is left needs every instruction of the k-loop placed by hand.

Structure (one persistent workgroup of FOUR waves per CU, one wave per SIMD, 512 registers per lane):
  * wave tile 128x128 as 4x4 blocks of v_mfma_f32_32x32x16_f16 (256 accumulator AGPRs), computed transposed
    (D^T = W_frag . X_frag^T) so a lane owns 4 consecutive output columns;
  * LDS: two K-tile buffers of 64 KiB ([A0 A1 B0 B1] half-tiles of [128][64] fp16, 16-byte slots XOR-swizzled by
    (row >> 1) & 7; the swizzle lives on the DMA's source side and on the fragment reads) + one 8 KiB slab per wave for
    the epilogue's transposition = 160 KiB;
  * global -> LDS by `buffer_load_dwordx4 ... lds` (sixteen 1 KiB pieces per wave and K-tile) through buffer descriptors
    whose range check zero-fills rows beyond M (and turns the DMA into a no-op once the work list is exhausted), the
    descriptor base advanced by scalar adds, one offset VGPR per piece: no vector address arithmetic in the loop;
  * the WHOLE K-tile's fragments live in registers (four sets of 32 VGPRs), so a buffer is free for the DMA of K-tile
    t+2 after the first quarter of K-tile t; two barriers per K-tile; waits are counted (`vmcnt(n)` never 0 in the loop);
  * MFMAs issue back to back with at most a few side instructions (ds_read / DMA / SALU) in each 32-cycle shadow;
  * the K-tile stream is continuous across output tiles: the DMA side runs two K-tiles ahead of the MFMA side through
    the workgroup's list of tiles (host-built table, XCD-aware order), the epilogue of a finished tile runs with the next
    tile's first two K-tiles already in flight.

Run:  python3 gemm_asm_gen.py [--trace] > gemm_asm.s      (--meta: the header csrc/gemm.hip includes instead)
"""
import sys

from asm_common import AsmWriter, kernel_begin, kernel_end, kernel_metadata, module_text, younger

# GELU of the fp16 epilogue (gelu_quad): gelu(x) = x / (1 + exp2(x Q(x^2))), Q of degree 4. The bit patterns of -log2(e) Q's coefficients
# as the kernel holds them: c4, c2, c1, c0 in the SGPR pairs s[S_C:S_C+7] (both halves of a packed operand), c3 in two VGPRs (an
# instruction takes one SGPR operand). oracle/pointwise.py evaluates the same polynomial from these names.
GELU_SGPR_CONSTS = [0xb658b1ce, 0xb658b1ce, 0x39bce2fa, 0x39bce2fa, 0xbdd78116, 0xbdd78116, 0xc01354b6, 0xc01354b6]
GELU_C3 = 0x38b90ca2

# ---------------------------------------------------------------- register map
# SGPRs
S_KARG = 0          # s[0:1] kernarg pointer
S_WG = 2            # workgroup id
S_A, S_W, S_BIAS, S_OUT, S_RES, S_GAM, S_TAB = 4, 6, 8, 10, 12, 14, 16
S_M, S_N, S_K, S_LDA, S_LDW, S_LDO, S_LDR, S_G, S_FLAGS = 18, 19, 20, 21, 22, 23, 24, 25, 26
S_RMASK = 27        # kernarg `pad`: resid_mod - 1 (residual row = output row & mask: a [resid_mod, N] table added to every image, resid_mod a power of two >= 256) or -1
SRD_A, SRD_B, SRD_O, SRD_R, SRD_BIAS, SRD_GAM = 28, 32, 36, 40, 44, 48
S_M0BASE = 68
S_KREM, S_DKREM, S_NK = 69, 70, 71
S_TCUR, S_TDMA, S_TNEXT, S_CUR, S_STRIDE = 72, 73, 74, 75, 76
S_WV, S_WR, S_WC = 77, 78, 79
S_FA, S_FB = 80, 81            # fragment half-tile bases of this wave
S_LDA2, S_LDW2 = 82, 83
S_T0, S_T1, S_T2, S_T3, S_T4 = 84, 85, 86, 87, 88
S_ROW4, S_TOFF, S_N0X4, S_ROFF, S_RROW4 = 89, 90, 91, 92, 93
S_C = 52            # s[52:59] GELU constants (pairs): GELU_SGPR_CONSTS
S_ROW28, S_RROW28 = 65, 66
S_ACC_LOOP, S_ACC_EPI, S_NKT = 67, 94, 95     # trace variants: cycles inside k-loops / epilogues, K-tiles done
S_TS0, S_TS1, S_TRP = 96, 98, 100              # s_memtime stamps, trace pointer
S_SKQ, S_SKREM, S_SKR, S_SKT = 96, 97, 98, 99  # split-K variant (never traced): K-tiles per range (quotient, remainder), range of an item, temp
NUM_SGPR = 102

# VGPRs (architectural file, 0..255); accumulators are a[0:255]
V_TID = 0
V_FA = 1            # v1..v4   A-fragment read addresses per k-step
V_FB = 5            # v5..v8
V_DA = 9            # v9..v16  DMA offsets, A pieces
V_DB = 17           # v17..v24 DMA offsets, B pieces
V_LANE, V_LR, V_LG, V_T0, V_T1, V_T2, V_T3 = 25, 26, 27, 28, 29, 30, 31
V_SFOFF, V_MFOFF, V_RSOFF, V_RSTD = 25, 26, 27, 28     # folded-LayerNorm consumer: lane offsets of the operand loads, rstd of the 4 row blocks
                                                        # (the setup temporaries v25..v31 are dead once the first tile starts)
# ... producer (fp32 epilogue): descriptors of the fp16 copy and of the statistics, strides; temporaries / running offsets
SRD_O16, SRD_ST = 96, 52
S_LD16X2, S_O16ROW4, S_STROW4, S_O16ROW28, S_STROW28, S_PARTS8, S_O16OFF, S_STOFF = 56, 57, 58, 59, 60, 61, 62, 63
S_EXROW = 100                                           # s[64:65]: exec mask of the lanes 0 / 16 / 32 / 48 (one per row of an emit pass)
V_O16, V_ST, V_SQ, V_SUM = 25, 254, 26, 252             # v[26:27] squares / fp16 pairs, v[252:253] (sum, sum of squares)
SRD_MR, SRD_SF, SRD_MF = 40, 48, 96                     # ... its descriptors: (mean, rstd) rows / s fragments / -mean fragments
V_SET = [32, 64, 96, 128]      # fragment sets S0..S3: +0..15 X (A) fragments rb=0..3, +16..31 W (B) fragments cb=0..3
V_PARK = 160        # 16 park addresses (fp16) / 8 (fp32)
V_EADDR = 176       # 4 emit read addresses
V_EM = [180, 212]   # two sets of 32 emit registers
V_TMP = 244         # 12 temporaries
V_BIAS = 96         # epilogue: bias in the S2 / S3 area (64 regs, fp16 epilogues) / residual double buffer (fp32)
# epilogue addressing: lane parts / running offsets of `out` and `resid` (inside V_TMP: +4..+7)
V_OLANE, V_RLANE, V_O, V_R = 248, 249, 250, 251
# fp32 epilogue: bias (4) + gamma (4) per column half; half 0 behind the 8 fp32 park addresses, half 1 in V_TMP / the setup temporaries
V_BG0, V_GG0, V_BG1, V_GG1 = 168, 172, 244, 28

LDS_BUF = 16384     # distance between the two buffers of one half-tile
LDS_SLAB = 131072   # epilogue slabs: 4 x 8 KiB

EPI_F16, EPI_GELU_F16, EPI_F32 = 0, 1, 2


class Gen(AsmWriter):
    def __init__(self, name, epi, sched):
        AsmWriter.__init__(self, name)
        self.epi, self.sched = epi, sched
        # LayerNorm folded into the GEMMs either side of it (csrc/gemm.hip psam_gemm_f16_ln): `lnc` = the consuming GEMM (fp16 / GELU
        # epilogues: out = rstd_row * (x16 . W'^T - mean_row * s_col) + t_col), `lnp` = the producing one (fp32 epilogue: also writes
        # fp16(x) and per-row (sum, sum of squares) over its 64-column groups)
        self.lnc = bool(sched.get("ln_cons")) and epi != EPI_F32
        self.lnp = bool(sched.get("ln_prod")) and epi == EPI_F32
        # split-K (round 6, psam_gemm_f16_splitk_ln): a work item is (tile, K range); the kernarg `pad` carries the number of ranges, the
        # fp32 epilogue (no bias, no residual) stores range r's partial sums to plane r of `out`
        self.sk = bool(sched.get("splitk")) and epi == EPI_F32 and not self.lnp
        assert not (self.sk and sched.get("trace"))
        # sched "mfma": "32x32x16" (4x4 blocks of 16 accumulators, 64 MFMA slots per K-tile) or "16x16x32" (8x8 blocks of 4, 128 slots)
        self.m16 = sched.get("mfma", "32x32x16") == "16x16x32"
        assert not (self.m16 and self.sk)

    # ------------------------------------------------------------ pieces of the program
    def item_rows_cols(self, item):
        """S_T0 = tile row index, S_T1 = tile column index of work item `item` (an SGPR): row | col << 16; the split-K variant keeps
        the item's K range in bits 12..15 of the row half"""
        e = self.e
        e("s_and_b32 s%d, s%d, 0x%x" % (S_T0, item, 0xfff if self.sk else 0xffff))
        e("s_lshr_b32 s%d, s%d, 16" % (S_T1, item))

    def item_ktiles(self, item, dst):
        """split-K: dst = the number of K-tiles of `item`'s range r = bits 12..15: q + (r < rem); S_SKR = r"""
        e = self.e
        e("s_bfe_u32 s%d, s%d, 0x4000c" % (S_SKR, item))                  # 4 bits from bit 12
        e("s_cmp_lt_u32 s%d, s%d" % (S_SKR, S_SKREM))
        e("s_addc_u32 s%d, s%d, 0" % (dst, S_SKQ))

    def switch_tile(self):
        """DMA side moves to the next tile of the workgroup's list (entry prefetched in S_TNEXT)."""
        e = self.e
        done, out = self.u("L_sw_none"), self.u("L_sw_out")
        e("s_mov_b32 s%d, s%d" % (S_TDMA, S_TNEXT))
        e("s_cmp_eq_u32 s%d, -1" % S_TDMA)
        e("s_cbranch_scc1 %s" % done)
        self.item_rows_cols(S_TDMA)
        e("s_lshl_b32 s%d, s%d, 8" % (S_T0, S_T0))          # row0
        e("s_lshl_b32 s%d, s%d, 8" % (S_T1, S_T1))          # col0
        e("s_mul_i32 s%d, s%d, s%d" % (S_T2, S_T0, S_LDA2))
        e("s_mul_hi_u32 s%d, s%d, s%d" % (S_T3, S_T0, S_LDA2))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_A, S_A, S_T2))
        e("s_addc_u32 s%d, s%d, s%d" % (SRD_A + 1, S_A + 1, S_T3))
        e("s_sub_u32 s%d, s%d, s%d" % (S_T4, S_M, S_T0))
        e("s_mul_i32 s%d, s%d, s%d" % (SRD_A + 2, S_T4, S_LDA2))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T2, S_T1, S_LDW2))
        e("s_mul_hi_u32 s%d, s%d, s%d" % (S_T3, S_T1, S_LDW2))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_B, S_W, S_T2))
        e("s_addc_u32 s%d, s%d, s%d" % (SRD_B + 1, S_W + 1, S_T3))
        e("s_sub_u32 s%d, s%d, s%d" % (S_T4, S_N, S_T1))
        e("s_mul_i32 s%d, s%d, s%d" % (SRD_B + 2, S_T4, S_LDW2))
        if self.sk:
            # the item's K range: first K-tile r * q + min(r, rem), 128 bytes per K-tile of a row; both operand windows start there
            self.item_ktiles(S_TDMA, S_DKREM)
            e("s_min_u32 s%d, s%d, s%d" % (S_SKT, S_SKR, S_SKREM))
            e("s_mul_i32 s%d, s%d, s%d" % (S_T4, S_SKR, S_SKQ))
            e("s_add_u32 s%d, s%d, s%d" % (S_T4, S_T4, S_SKT))
            e("s_lshl_b32 s%d, s%d, 7" % (S_T4, S_T4))
            for srd in (SRD_A, SRD_B):
                e("s_add_u32 s%d, s%d, s%d" % (srd, srd, S_T4))
                e("s_addc_u32 s%d, s%d, 0" % (srd + 1, srd + 1))
                e("s_max_u32 s%d, s%d, s%d" % (srd + 2, srd + 2, S_T4))
                e("s_sub_u32 s%d, s%d, s%d" % (srd + 2, srd + 2, S_T4))
        else:
            e("s_mov_b32 s%d, s%d" % (S_DKREM, S_NK))
        e("s_add_u32 s%d, s%d, s%d" % (S_CUR, S_CUR, S_STRIDE))
        e("s_load_dword s%d, s[%d:%d], s%d" % (S_TNEXT, S_TAB, S_TAB + 1, S_CUR))
        e("s_branch %s" % out)
        self.lab(done)
        e("s_mov_b32 s%d, 0" % (SRD_A + 2))
        e("s_mov_b32 s%d, 0" % (SRD_B + 2))
        e("s_mov_b32 s%d, 0x7fffffff" % S_DKREM)
        self.lab(out)

    def dma_m0(self, p):
        j = p & 7
        const = (65536 if p >= 8 else 0) + (j >> 2) * 32768 + (j & 3) * 4096
        return "s_add_u32 m0, s%d, 0x%x" % (S_M0BASE, const)

    def dma_issue(self, p):
        if p < 8:
            return "buffer_load_dwordx4 v%d, s[%d:%d], 0 offen lds" % (V_DA + p, SRD_A, SRD_A + 3)
        return "buffer_load_dwordx4 v%d, s[%d:%d], 0 offen lds" % (V_DB + p - 8, SRD_B, SRD_B + 3)

    def dma_advance(self):
        out = []
        for srd in (SRD_A, SRD_B):
            out += ["s_add_u32 s%d, s%d, 128" % (srd, srd), "s_addc_u32 s%d, s%d, 0" % (srd + 1, srd + 1),
                    "s_max_u32 s%d, s%d, 128" % (srd + 2, srd + 2), "s_sub_u32 s%d, s%d, 128" % (srd + 2, srd + 2)]
        out.append("s_sub_u32 s%d, s%d, 1" % (S_DKREM, S_DKREM))
        return out

    def frag_read(self, st, ks, idx):
        """idx 0..3: X (A) fragment of row block idx; 4..7: W (B) fragment of column block idx-4 - of k-step ks into set st"""
        if idx < 4:
            return "ds_read_b128 v[%d:%d], v%d offset:%d" % (V_SET[st] + 4 * idx, V_SET[st] + 4 * idx + 3, V_FA + ks, idx * 4096)
        j = idx - 4
        return "ds_read_b128 v[%d:%d], v%d offset:%d" % (V_SET[st] + 16 + 4 * j, V_SET[st] + 16 + 4 * j + 3, V_FB + ks, j * 4096)

    # The 16x16x32 form. A fragment is 16 rows x 4 sixteen-byte k-slots: lane -> row lane & 15, slot 4 * k-step + (lane >> 4), for X
    # and W alike (the MFMA's own k order: lane group g supplies k = 8 g ... 8 g + 7 of its 32), read at the same swizzled place
    # row * 128 + ((slot ^ (row >> 1) & 7) << 4) the DMA wrote it to. Sixteen lanes of a group cover 16 distinct 16-byte columns of
    # two 128-byte row parities: conflict-free like the 32-row form. A k-step's 8 X + 8 W fragments fill two of the four register
    # sets (k-step 0: S0 S1 = v32..95, k-step 1: S2 S3 = v96..159): +0..31 X fragments of row blocks 0..7, +32..63 W of column blocks.
    RD16_ORDER = tuple(range(8, 16)) + tuple(range(8))        # W fragments first: MFMA slot 0 needs all eight and X block 0
    M16_FA, M16_FB = (1, 2), (3, 8)                           # read addresses of the X / W fragments per k-step

    def frag_read16(self, ks, idx):
        """idx 0..7: X fragment of 16-row block idx; 8..15: W fragment of 16-column block idx - 8 - of k-step ks (0 / 1)"""
        base = V_SET[2 * ks]
        if idx < 8:
            return "ds_read_b128 v[%d:%d], v%d offset:%d" % (base + 4 * idx, base + 4 * idx + 3, self.M16_FA[ks], idx * 2048)
        j = idx - 8
        return "ds_read_b128 v[%d:%d], v%d offset:%d" % (base + 32 + 4 * j, base + 32 + 4 * j + 3, self.M16_FB[ks], j * 2048)

    def mfma16(self, ks, rb, cb, zero):
        """D^T block: lane owns output row rb * 16 + (lane & 15) and the columns cb * 16 + 4 (lane >> 4) + 0..3 in a[blk:blk+3]"""
        blk, base = (rb * 8 + cb) * 4, V_SET[2 * ks]
        a = "v[%d:%d]" % (base + 32 + 4 * cb, base + 32 + 4 * cb + 3)
        b = "v[%d:%d]" % (base + 4 * rb, base + 4 * rb + 3)
        cc = "0" if zero else "a[%d:%d]" % (blk, blk + 3)
        return "v_mfma_f32_16x16x32_f16 a[%d:%d], %s, %s, %s" % (blk, blk + 3, a, b, cc)

    def build_slots16(self, zero_copy=False):
        """side instructions behind each of the 128 MFMAs of a K-tile (slot = k-step * 64 + rb * 8 + cb): at most one per 16-cycle gap
        (a compare and its branch take two gaps), a DMA piece alone in its gap with its m0 in the gap before. zero_copy: the slots of
        k-step 0 as the C = 0 copy of a tile's first K-tile carries them (own return label of the tile switch; no operand requests:
        a tile has at least two K-tiles)"""
        sc = self.sched
        z = "_z" if zero_copy else ""
        slots = [[] for _ in range(128)]
        def put(s, ins):
            assert not slots[s], (s, ins, slots[s])
            slots[s].append(ins)
        # fragment reads of k-step 1 of THIS tile during k-step 0
        for i, idx in enumerate(self.RD16_ORDER):
            put(sc["rd1"][i], self.frag_read16(1, idx))
        for i, r in enumerate((self.M16_FA[1], self.M16_FB[1])):
            put(sc["tog1"][i], "v_xor_b32 v%d, 0x%x, v%d" % (r, LDS_BUF, r))
        if not zero_copy:
            put(sc["pre_slot"], "s_cmp_eq_u32 s%d, 1" % S_KREM)
            slots[sc["pre_slot"] + 1] += ["s_cbranch_scc1 L_pre_%s" % self.name, "L_pre_ret_%s:" % self.name]
        # barrier A: every wave has its fragments of this K-tile -> its buffer may be refilled
        a = sc["barA"]
        slots[a] += ["s_waitcnt lgkmcnt(0)", "s_barrier"]
        put(a + 1, "s_cmp_eq_u32 s%d, 0" % S_DKREM)
        slots[a + 2] += ["s_cbranch_scc1 L_switch%s_%s" % (z, self.name), "L_switch_ret%s_%s:" % (z, self.name)]
        # DMA pieces of K-tile t+2
        for p in range(16):
            s = sc["dma"][p]
            assert p == 0 or s - sc["dma"][p - 1] >= 3
            put(s - 1, self.dma_m0(p))
            put(s, self.dma_issue(p))
        # barrier B: K-tile t+1 has landed
        b = sc["barB"]
        issued = sum(1 for p in range(16) if sc["dma"][p] <= b)
        assert not slots[b]
        slots[b] += ["s_waitcnt vmcnt(%d)" % issued, "s_barrier"]
        # fragment reads of k-step 0 of the NEXT K-tile, then the DMA side's advance
        for i, idx in enumerate(self.RD16_ORDER):
            assert sc["rd0"][i] > b
            put(sc["rd0"][i], self.frag_read16(0, idx))
        for i, ins in enumerate(self.dma_advance()):
            assert sc["adv"] + i > sc["dma"][15]
            put(sc["adv"] + i, ins)
        return slots

    def lgkm_waits16(self):
        """slot -> operand of the s_waitcnt in front of its MFMA. LDS reads complete in order: the sixteen of k-step 0 were issued
        W0..7, X0..7 at the end of the previous K-tile, X block rb is needed at slot 8 rb; by then the reads of k-step 1 issued in
        this K-tile's earlier gaps are outstanding too. From barrier A on (lgkmcnt(0)) everything has arrived."""
        sc = self.sched
        out = {}
        for rb in range(8):
            s = 8 * rb
            if s > sc["barA"]:
                break
            out[s] = min(15, (7 - rb) + sum(1 for x in sc["rd1"] if x < s))
        return out

    def mfma(self, st, rb, cb, zero):
        blk = (rb * 4 + cb) * 16
        a = "v[%d:%d]" % (V_SET[st] + 16 + 4 * cb, V_SET[st] + 16 + 4 * cb + 3)   # W fragment: MFMA A operand
        b = "v[%d:%d]" % (V_SET[st] + 4 * rb, V_SET[st] + 4 * rb + 3)             # X fragment: MFMA B operand
        cc = "0" if zero else "a[%d:%d]" % (blk, blk + 15)
        return "v_mfma_f32_32x32x16_f16 a[%d:%d], %s, %s, %s" % (blk, blk + 15, a, b, cc)

    # ------------------------------------------------------------ the K-tile body
    def build_slots(self):
        """side instructions behind each of the 64 MFMAs of a K-tile (slot = k-step * 16 + rb * 4 + cb)"""
        sc = self.sched
        slots = [[] for _ in range(64)]
        # fragment reads of k-steps 2 / 3 of THIS tile (sets S2, S3) during k-step 0
        for i in range(16):
            slots[sc["rd23"][i]].append(self.frag_read(2 + i // 8, 2 + i // 8, i % 8))
        # toggles of the addresses used above (next use: next K-tile)
        for i, r in enumerate((V_FA + 2, V_FA + 3, V_FB + 2, V_FB + 3)):
            slots[sc["tog23"] + i].append("v_xor_b32 v%d, 0x%x, v%d" % (r, LDS_BUF, r))
        # the last K-tile of a tile requests the epilogue's operands (out of line)
        slots[sc.get("pre_slot", 17)] += ["s_cmp_eq_u32 s%d, 1" % S_KREM, "s_cbranch_scc1 L_pre_%s" % self.name, "L_pre_ret_%s:" % self.name]
        if self.lnc:
            slots[48] += ["s_cmp_eq_u32 s%d, 1" % S_KREM, "s_cbranch_scc1 L_pre2_%s" % self.name, "L_pre2_ret_%s:" % self.name]
        # barrier A: every wave has its fragments of this K-tile -> its buffer may be refilled
        a = sc["barA"]
        slots[a] += ["s_waitcnt lgkmcnt(0)", "s_barrier"]
        slots[a] += ["s_cmp_eq_u32 s%d, 0" % S_DKREM, "s_cbranch_scc1 L_switch_%s" % self.name, "L_switch_ret_%s:" % self.name]
        # DMA pieces of K-tile t+2
        for p in range(16):
            s = sc["dma"][p]
            slots[s - 1].append(self.dma_m0(p))
            slots[s].append(self.dma_issue(p))
        last = sc["dma"][15]
        adv = self.dma_advance()
        for i, ins in enumerate(adv):
            slots[min(63, last + 1 + i // 3)].append(ins)
        slots[min(63, last + 1)].append("s_xor_b32 s%d, s%d, 0x%x" % (S_M0BASE, S_M0BASE, LDS_BUF))
        # barrier B: K-tile t+1 has landed
        b = sc["barB"]
        issued = sum(1 for p in range(16) if sc["dma"][p] <= b)
        slots[b] += ["s_waitcnt vmcnt(%d)" % issued, "s_barrier"]
        # fragment reads of k-steps 0 / 1 of the NEXT tile (sets S0, S1)
        for i in range(16):
            s = sc["rd01"][i]
            assert s > b
            slots[s].append(self.frag_read(i // 8, i // 8, i % 8))
        return slots

    def ktile(self, slots, zero_first):
        e = self.e
        for s in range(64):
            ks, rb, cb = s // 16, (s % 16) // 4, s % 4
            if s == 0:
                e("s_waitcnt lgkmcnt(8)")
            if s == 16:
                e("s_waitcnt lgkmcnt(15)")
            e(self.mfma(ks, rb, cb, zero_first and ks == 0))
            for ins in slots[s]:
                if ins.endswith(":"):
                    self.lab(ins[:-1])
                else:
                    e(ins)
            if s == 15 and zero_first:
                e("s_branch L_after_ks0_%s" % self.name)
                return

    # ------------------------------------------------------------ epilogues
    def gelu_quad(self, xa, ta, xb, tb):
        """Two pairs at once, their instruction streams interleaved (a VALU instruction that reads the result of v_exp_f32 / v_rcp_f32 in
        the very next issue slot gets the OLD value on gfx950: no interlock). gelu(x) = x / (1 + exp2(x Q(x^2))) with a degree-4
        Q - the minimax fit of -log2(e) logit(Phi(x)) / x, leading coefficient of logit side positive so that the sigmoid saturates the
        right way for any |x| - 12 instructions per pair instead of the 18 of the A&S erf form, within 3.4e-6 of gelu(x) over the whole
        line in fp32 (the fp16 rounding of the result is 5e-4 |y|; fit: tools/r05/gelu_fit.py)."""
        e = self.e
        P = ((xa, ta, ta + 2), (xb, tb, tb + 2))          # (x, u, q) pairs of registers
        for (x, u, q) in P:
            e("v_pk_mul_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (u, u + 1, x, x + 1, x, x + 1))                                       # u = x^2
        for (x, u, q) in P:
            e("v_pk_fma_f32 v[%d:%d], v[%d:%d], s[%d:%d], v[%d:%d] op_sel_hi:[1,0,1]" % (q, q + 1, u, u + 1, S_C, S_C + 1, V_TMP + 8, V_TMP + 9))
        for k in range(3):
            for (x, u, q) in P:
                e("v_pk_fma_f32 v[%d:%d], v[%d:%d], v[%d:%d], s[%d:%d] op_sel_hi:[1,1,0]" % (q, q + 1, q, q + 1, u, u + 1, S_C + 2 + 2 * k, S_C + 3 + 2 * k))
        for (x, u, q) in P:
            e("v_pk_mul_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (q, q + 1, x, x + 1, q, q + 1))                                       # -log2(e) x Q(x^2)
        for i in range(2):
            for (x, u, q) in P:
                e("v_exp_f32 v%d, v%d" % (q + i, q + i))
        for (x, u, q) in P:
            e("v_pk_add_f32 v[%d:%d], v[%d:%d], 1.0 op_sel_hi:[1,0]" % (q, q + 1, q, q + 1))
        for i in range(2):
            for (x, u, q) in P:
                e("v_rcp_f32 v%d, v%d" % (q + i, q + i))
        for (x, u, q) in P:
            e("v_pk_mul_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (x, x + 1, x, x + 1, q, q + 1))

    def tile_offsets(self, esize):
        """S_T0 = row0, S_T1 = col0 of the finished tile; S_TOFF = byte offset of its origin in `out`, S_N0X4 = col0 * 4"""
        e = self.e
        self.item_rows_cols(S_TCUR)
        e("s_lshl_b32 s%d, s%d, 8" % (S_T0, S_T0))
        e("s_lshl_b32 s%d, s%d, 8" % (S_T1, S_T1))
        e("s_mul_i32 s%d, s%d, s%d" % (S_TOFF, S_T0, S_LDO))
        e("s_add_u32 s%d, s%d, s%d" % (S_TOFF, S_TOFF, S_T1))
        e("s_lshl_b32 s%d, s%d, %d" % (S_TOFF, S_TOFF, 1 if esize == 2 else 2))
        if self.sk:            # partial sums of range r go to plane r of the workspace: [ranges][M rounded up to whole tiles][ldo] fp32
            e("s_bfe_u32 s%d, s%d, 0x4000c" % (S_SKR, S_TCUR))
            e("s_add_u32 s%d, s%d, 255" % (S_SKT, S_M))
            e("s_andn2_b32 s%d, s%d, 255" % (S_SKT, S_SKT))
            e("s_mul_i32 s%d, s%d, s%d" % (S_SKT, S_SKT, S_LDO))
            e("s_lshl_b32 s%d, s%d, 2" % (S_SKT, S_SKT))
            e("s_mul_i32 s%d, s%d, s%d" % (S_SKT, S_SKT, S_SKR))
            e("s_add_u32 s%d, s%d, s%d" % (S_TOFF, S_TOFF, S_SKT))
        e("s_lshl_b32 s%d, s%d, 2" % (S_N0X4, S_T1))

    # Register plan of the epilogues. Their global operands (bias; for the fp32 form bias, gamma and the first two residual
    # slabs) are requested from inside the LAST K-tile of the tile (pre_epilogue, an out-of-line routine the loop branches to when
    # one iteration is left) into registers the k-loop does not use, so the epilogue starts with its operands on chip instead of
    # paying one (fp16) or eight (fp32: one per slab, the prefetch was one slab deep) exposed memory latencies per tile:
    #   fp16 / GELU : bias v180..v243 (the former emit sets), emit sets in the fragment sets S2 / S3 (free in the epilogue)
    #   fp32        : residual ring of three slabs v180..v211, v212..v243, v96..v127 (the third only from the epilogue on),
    #                 one emit set v128..v159
    F16_BIAS, F16_EM = 180, (96, 128)
    F32_RING, F32_EM = (180, 212, 96), 128

    def resid_loads(self, slab, vm):
        """requests the 32x64 residual slab `slab` (emit layout: pass `it` = four rows, 16 lanes x 16 bytes each) into its slot of
        the ring of three VGPR sets"""
        e = self.e
        rb, h = slab >> 1, slab & 1
        base = self.F32_RING[slab % 3]
        for it in range(8):
            e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d%s" % (base + 4 * it, base + 4 * it + 3, V_R, SRD_R, SRD_R + 3, h * 256,
                                                                                  self.sched.get("resid_policy", "")))
            vm.append(("res", slab))
            if it < 7:
                e("v_add_u32 v%d, s%d, v%d" % (V_R, S_RROW4, V_R))
        if h == 0:   # same rows again for the second column half
            e("v_subrev_u32 v%d, s%d, v%d" % (V_R, S_RROW28, V_R))
        else:
            e("v_add_u32 v%d, s%d, v%d" % (V_R, S_RROW4, V_R))

    def pre_epilogue(self):
        """out of line, executed once per tile from the last K-tile's iteration: requests the epilogue's operands"""
        e = self.e
        vm = []
        self.item_rows_cols(S_TCUR)
        e("s_lshl_b32 s%d, s%d, 8" % (S_T0, S_T0))
        e("s_lshl_b32 s%d, s%d, 8" % (S_T1, S_T1))
        e("s_lshl_b32 s%d, s%d, 2" % (S_N0X4, S_T1))
        if self.epi == EPI_F32:
            if self.sched.get("trace"):
                e("s_mul_i32 s%d, s%d, s%d" % (S_ROFF, S_T0, S_LDR))
            else:                  # (the trace variants keep a time stamp in s27: no residual table there)
                e("s_and_b32 s%d, s%d, s%d" % (S_T2, S_T0, S_RMASK))
                e("s_mul_i32 s%d, s%d, s%d" % (S_ROFF, S_T2, S_LDR))
            e("s_add_u32 s%d, s%d, s%d" % (S_ROFF, S_ROFF, S_T1))
            e("s_lshl_b32 s%d, s%d, 2" % (S_ROFF, S_ROFF))
            e("v_add_u32 v%d, s%d, v%d" % (V_R, S_ROFF, V_RLANE))
            for h in range(2):
                bb, gg = (V_BG0, V_GG0) if h == 0 else (V_BG1, V_GG1)
                e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (bb, bb + 3, V_TMP + 11, SRD_BIAS, SRD_BIAS + 3, S_N0X4, h * 256))
                e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (gg, gg + 3, V_TMP + 11, SRD_GAM, SRD_GAM + 3, S_N0X4, h * 256))
                vm += [("bg", 0), ("bg", 0)]
            self.resid_loads(0, vm)
            self.resid_loads(1, vm)
        elif self.m16:             # a lane's columns: cb * 16 + 4 (lane >> 4) + 0..3 -> v180..211
            for cb in range(8):
                r = self.F16_BIAS + cb * 4
                e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (r, r + 3, V_TMP + 11, SRD_BIAS, SRD_BIAS + 3, S_N0X4, cb * 64))
                vm.append(("bias", 0))
        else:
            for cb in range(4):
                for q in range(4):
                    r = self.F16_BIAS + (cb * 4 + q) * 4
                    e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (r, r + 3, V_TMP + 11, SRD_BIAS, SRD_BIAS + 3, S_N0X4, (cb * 32 + 8 * q) * 4))
                    vm.append(("bias", 0))
        return vm

    def pre2_epilogue(self):
        """folded-LayerNorm consumer, out of line from slot 48 of a tile's last K-tile: the correction operands.
        v96..111: s fragments of the four column blocks, v112..127: -mean fragments of the four row blocks (MFMA operands: lanes
        0..31 hold {hi, lo, hi, 0 x 5} / {hi, hi, lo, 0 x 5} in k = 0..7, lanes 32..63 read beyond the buffer = 0), v28..31: rstd"""
        e = self.e
        vm = []
        e("s_and_b32 s%d, s%d, 0xffff" % (S_T0, S_TCUR))
        e("s_lshr_b32 s%d, s%d, 16" % (S_T1, S_TCUR))
        e("s_lshl_b32 s%d, s%d, 12" % (S_T2, S_T1))                     # col0 * 16 bytes
        e("s_lshl_b32 s%d, s%d, 12" % (S_T3, S_T0))                     # row0 * 16
        e("s_lshl_b32 s%d, s%d, 11" % (S_T4, S_T0))                     # row0 * 8
        if self.m16:
            # 16x16 blocks: the rank-1 update is one v_mfma_f32_16x16x16_f16 per block, whose operands are the first 8 bytes of a
            # fragment row (k = 0..3 of lanes 0..15; lanes 16..63 read beyond the buffer = 0): s of the eight column blocks in
            # v212..227, -mean of the eight row blocks in v228..243, rstd in four register pairs (M16_RSTD)
            for cb in range(8):
                e("buffer_load_dwordx2 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (self.M16_SF + 2 * cb, self.M16_SF + 2 * cb + 1, V_SFOFF, SRD_SF, SRD_SF + 3, S_T2, cb * 256))
                vm.append(("sf", 0))
            for rb in range(8):
                e("buffer_load_dwordx2 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (self.M16_MF + 2 * rb, self.M16_MF + 2 * rb + 1, V_MFOFF, SRD_MF, SRD_MF + 3, S_T3, rb * 256))
                vm.append(("mf", 0))
            for rb in range(8):
                e("buffer_load_dword v%d, v%d, s[%d:%d], s%d offen offset:%d" % (self.M16_RSTD[rb >> 1] + (rb & 1), V_RSOFF, SRD_MR, SRD_MR + 3, S_T4, rb * 128))
                vm.append(("rs", 0))
            return vm
        for cb in range(4):
            e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (96 + 4 * cb, 99 + 4 * cb, V_SFOFF, SRD_SF, SRD_SF + 3, S_T2, cb * 512))
            vm.append(("sf", 0))
        for rb in range(4):
            e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (112 + 4 * rb, 115 + 4 * rb, V_MFOFF, SRD_MF, SRD_MF + 3, S_T3, rb * 512))
            vm.append(("mf", 0))
        for rb in range(4):
            e("buffer_load_dword v%d, v%d, s[%d:%d], s%d offen offset:%d" % (V_RSTD + rb, V_RSOFF, SRD_MR, SRD_MR + 3, S_T4, rb * 256))
            vm.append(("rs", 0))
        return vm

    M16_SF, M16_MF = 212, 228
    M16_RSTD = (28, 30, 4, 6)                    # aligned pairs; v4..v7 are free: the 16x16x32 form has two read addresses per operand (M16_FA / M16_FB)

    def younger(self, vm, tag):
        return younger(vm, tag)

    def epilogue_f16_m16(self, gelu, vm):
        """the fp16 epilogues of the 16x16x32 form: the PARK half differs (a 32-row slab is 2 x 8 blocks of 4 registers; a lane's four
        columns cb * 16 + 4 g + 0..3 are half of the 16-byte chunk 2 cb + (g >> 1) of its row), the emit half is epilogue_f16's"""
        e = self.e
        self.c("---- epilogue (16x16x32 accumulators): bias (+ GELU) -> fp16, through the wave's slab so that 16 lanes store one 256-byte row piece")
        e("s_nop 7")
        e("s_nop 7")
        self.tile_offsets(2)
        e("v_add_u32 v%d, s%d, v%d" % (V_O, S_TOFF, V_OLANE))
        e("s_waitcnt vmcnt(%d)" % self.younger(vm, ("bias", 0)))
        if self.lnc:
            self.c("folded LayerNorm: acc -= mean_row * s_col, one rank-1 MFMA per 16x16 block (fp16 hi / lo operands: fp32-accurate)")
            e("s_waitcnt vmcnt(%d)" % self.younger(vm, ("rs", 0)))
            for rb in range(8):
                for cb in range(8):
                    blk = (rb * 8 + cb) * 4
                    e("v_mfma_f32_16x16x16_f16 a[%d:%d], v[%d:%d], v[%d:%d], a[%d:%d]" % (blk, blk + 3, self.M16_SF + 2 * cb, self.M16_SF + 2 * cb + 1,
                                                                                      self.M16_MF + 2 * rb, self.M16_MF + 2 * rb + 1, blk, blk + 3))
            e("s_nop 7")
            e("s_nop 7")
            e("s_nop 3")
        for rb32 in range(4):
            em = self.F16_EM[rb32 & 1]
            for sub in range(2):
                rb = 2 * rb32 + sub
                for cb in range(8):
                    blk = (rb * 8 + cb) * 4
                    t = V_TMP
                    for i in range(4):
                        e("v_accvgpr_read_b32 v%d, a%d" % (t + i, blk + i))
                    b = self.F16_BIAS + cb * 4
                    if self.lnc:
                        rp, hs = self.M16_RSTD[rb >> 1], rb & 1
                        for hh in range(2):
                            e("v_pk_fma_f32 v[%d:%d], v[%d:%d], v[%d:%d], v[%d:%d] op_sel:[0,%d,0] op_sel_hi:[1,%d,1]" % (
                                t + 2 * hh, t + 2 * hh + 1, t + 2 * hh, t + 2 * hh + 1, rp, rp + 1, b + 2 * hh, b + 2 * hh + 1, hs, hs))
                    else:
                        e("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (t, t + 1, t, t + 1, b, b + 1))
                        e("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (t + 2, t + 3, t + 2, t + 3, b + 2, b + 3))
                    if gelu:
                        self.gelu_quad(t, self.F16_EM[(rb32 + 1) & 1], t + 2, self.F16_EM[(rb32 + 1) & 1] + 8)
                    e("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (t, t, t + 1))
                    e("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (t + 1, t + 2, t + 3))
                    e("ds_write_b64 v%d, v[%d:%d] offset:%d" % (V_PARK + cb, t, t + 1, sub * 4096))
            for it in range(8):
                e("ds_read_b128 v[%d:%d], v%d offset:%d" % (em + 4 * it, em + 4 * it + 3, V_EADDR + (it & 3), (it >> 2) * 4096))
            for it in range(8):
                e("s_waitcnt lgkmcnt(%d)" % (7 - it))
                e("buffer_store_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen%s" % (em + 4 * it, em + 4 * it + 3, V_O, SRD_O, SRD_O + 3, self.sched.get("store_policy", "")))
                e("v_add_u32 v%d, s%d, v%d" % (V_O, S_ROW4, V_O))

    def epilogue_f16(self, gelu, vm):
        if self.m16:
            return self.epilogue_f16_m16(gelu, vm)
        e = self.e
        self.c("---- epilogue: bias (+ GELU) -> fp16, through the wave's slab so that 16 lanes store one 256-byte row piece")
        e("s_nop 7")
        self.tile_offsets(2)
        e("v_add_u32 v%d, s%d, v%d" % (V_O, S_TOFF, V_OLANE))
        e("s_waitcnt vmcnt(%d)" % self.younger(vm, ("bias", 0)))     # (requested in the last K-tile: long landed)
        if self.lnc:
            self.c("folded LayerNorm: acc -= mean_row * s_col, one rank-1 MFMA per block (fp16 hi / lo operands: fp32-accurate)")
            e("s_waitcnt vmcnt(%d)" % self.younger(vm, ("rs", 0)))
            for rb in range(4):
                for cb in range(4):
                    blk = (rb * 4 + cb) * 16
                    e("v_mfma_f32_32x32x16_f16 a[%d:%d], v[%d:%d], v[%d:%d], a[%d:%d]" % (blk, blk + 15, 96 + 4 * cb, 99 + 4 * cb, 112 + 4 * rb, 115 + 4 * rb, blk, blk + 15))
            e("s_nop 7")
            e("s_nop 7")
            e("s_nop 3")
        for rb in range(4):
            em = self.F16_EM[rb & 1]
            for cb in range(4):
                for q in range(4):
                    blk = (rb * 4 + cb) * 16 + 4 * q
                    t = V_TMP
                    for i in range(4):
                        e("v_accvgpr_read_b32 v%d, a%d" % (t + i, blk + i))
                    b = self.F16_BIAS + (cb * 4 + q) * 4
                    if self.lnc:     # rstd_row * acc' + t_col (the caller passes t as `bias`); rstd of row block rb = v(28 + rb)
                        rp, hs = V_RSTD + (rb & ~1), rb & 1
                        for hh in range(2):
                            e("v_pk_fma_f32 v[%d:%d], v[%d:%d], v[%d:%d], v[%d:%d] op_sel:[0,%d,0] op_sel_hi:[1,%d,1]" % (
                                t + 2 * hh, t + 2 * hh + 1, t + 2 * hh, t + 2 * hh + 1, rp, rp + 1, b + 2 * hh, b + 2 * hh + 1, hs, hs))
                    else:
                        e("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (t, t + 1, t, t + 1, b, b + 1))
                        e("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (t + 2, t + 3, t + 2, t + 3, b + 2, b + 3))
                    if gelu:
                        self.gelu_quad(t, self.F16_EM[(rb + 1) & 1], t + 2, self.F16_EM[(rb + 1) & 1] + 8)   # the other emit set is idle: temporaries
                    e("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (t, t, t + 1))
                    e("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (t + 1, t + 2, t + 3))
                    e("ds_write_b64 v%d, v[%d:%d]" % (V_PARK + cb * 4 + q, t, t + 1))
            for it in range(8):
                e("ds_read_b128 v[%d:%d], v%d offset:%d" % (em + 4 * it, em + 4 * it + 3, V_EADDR + (it & 3), (it >> 2) * 4096))
            for it in range(8):
                e("s_waitcnt lgkmcnt(%d)" % (7 - it))
                e("buffer_store_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen%s" % (em + 4 * it, em + 4 * it + 3, V_O, SRD_O, SRD_O + 3, self.sched.get("store_policy", "")))
                e("v_add_u32 v%d, s%d, v%d" % (V_O, S_ROW4, V_O))

    def epilogue_f32(self, vm):
        e = self.e
        self.c("---- epilogue: out = resid + gamma * (acc + bias) in fp32; eight 32x64 slabs through the wave's 8 KiB; the residual")
        self.c("     slabs come through a ring of three (two requested in the last K-tile, one more ahead of every slab processed).")
        # (A deeper ring was measured and dropped: every parked slab frees 32 accumulator registers, a VMEM load may land in AGPRs, so
        # all eight slabs can be in flight by the time the third is parked. No change - 23.7k vs 24.3k cycles per epilogue at
        # 65536x1280x1280, wall equal: the epilogue is not bound by the number of requests a wave's registers can hold.)
        e("s_nop 7")
        if self.m16:
            e("s_nop 7")
        self.tile_offsets(4)
        e("v_add_u32 v%d, s%d, v%d" % (V_O, S_TOFF, V_OLANE))
        if self.lnp:
            self.lnp_setup()
        self.resid_loads(2, vm)
        nog = self.u("L_gamma")
        e("s_bitcmp1_b32 s%d, 0" % S_FLAGS)             # flag bit 0: gamma present
        e("s_cbranch_scc1 %s" % nog)
        e("s_waitcnt vmcnt(%d)" % self.younger(vm, ("bg", 0)))
        for gg in (V_GG0, V_GG1):
            for i in range(4):
                e("v_mov_b32 v%d, 1.0" % (gg + i))
        self.lab(nog)
        em = self.F32_EM
        for slab in range(8):
            rb, h = slab >> 1, slab & 1
            if self.m16:         # 2 x 4 blocks of 4 registers: the lane's columns cbl * 16 + 4 g + 0..3 of the slab are its row's chunk 4 cbl + g
                for sub in range(2):
                    for cbl in range(4):
                        blk = ((2 * rb + sub) * 8 + 4 * h + cbl) * 4
                        e("ds_write_b128 v%d, a[%d:%d] offset:%d" % (V_PARK + cbl, blk, blk + 3, sub * 4096))
            for cbl in range(0 if self.m16 else 2):
                for q in range(4):
                    blk = (rb * 4 + 2 * h + cbl) * 16 + 4 * q
                    e("ds_write_b128 v%d, a[%d:%d]" % (V_PARK + cbl * 4 + q, blk, blk + 3))
            for it in range(8):
                e("ds_read_b128 v[%d:%d], v%d offset:%d" % (em + 4 * it, em + 4 * it + 3, V_EADDR + (it & 3), (it >> 2) * 4096))
            rbase = self.F32_RING[slab % 3]
            bb, gg = (V_BG0, V_GG0) if h == 0 else (V_BG1, V_GG1)
            e("s_waitcnt vmcnt(%d)" % self.younger(vm, ("res", slab)))
            for it in range(8):
                e("s_waitcnt lgkmcnt(%d)" % (7 - it))
                r = em + 4 * it
                rr = rbase + 4 * it
                for half in range(2):
                    e("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (r + 2 * half, r + 2 * half + 1, r + 2 * half, r + 2 * half + 1, bb + 2 * half, bb + 2 * half + 1))
                for half in range(2):
                    e("v_pk_fma_f32 v[%d:%d], v[%d:%d], v[%d:%d], v[%d:%d]" % (r + 2 * half, r + 2 * half + 1, r + 2 * half, r + 2 * half + 1, gg + 2 * half, gg + 1 + 2 * half,
                                                                      rr + 2 * half, rr + 2 * half + 1))
                e("buffer_store_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d%s" % (r, r + 3, V_O, SRD_O, SRD_O + 3, h * 256, self.sched.get("store_policy", "")))
                vm.append(("st", slab))
                if self.lnp:
                    self.ln_producer_row(r, h, vm, slab)
                if it < 7:
                    e("v_add_u32 v%d, s%d, v%d" % (V_O, S_ROW4, V_O))
                    if self.lnp:
                        e("v_add_u32 v%d, s%d, v%d" % (V_O16, S_O16ROW4, V_O16))
                        e("v_add_u32 v%d, s%d, v%d" % (V_ST, S_STROW4, V_ST))
            if h == 0:
                e("v_subrev_u32 v%d, s%d, v%d" % (V_O, S_ROW28, V_O))
            else:
                e("v_add_u32 v%d, s%d, v%d" % (V_O, S_ROW4, V_O))
            if self.lnp:
                for vv, r28, r4 in ((V_O16, S_O16ROW28, S_O16ROW4), (V_ST, S_STROW28, S_STROW4)):
                    e(("v_subrev_u32 v%d, s%d, v%d" if h == 0 else "v_add_u32 v%d, s%d, v%d") % (vv, r28 if h == 0 else r4, vv))
            if slab < 5:                # the VGPR set just consumed takes the slab three on
                self.resid_loads(slab + 3, vm)

    def lnp_setup(self):
        e = self.e
        e("s_lshl_b32 s%d, s%d, 7" % (S_T2, S_WR))
        e("s_add_u32 s%d, s%d, s%d" % (S_T2, S_T2, S_T0))                 # first row of this wave's tile
        e("s_lshl_b32 s%d, s%d, 7" % (S_T3, S_WC))
        e("s_add_u32 s%d, s%d, s%d" % (S_T3, S_T3, S_T1))                 # first column
        e("s_mul_i32 s%d, s%d, s%d" % (S_O16OFF, S_T2, S_LD16X2))
        e("s_lshl_b32 s%d, s%d, 1" % (S_T4, S_T3))
        e("s_add_u32 s%d, s%d, s%d" % (S_O16OFF, S_O16OFF, S_T4))
        e("s_mul_i32 s%d, s%d, s%d" % (S_STOFF, S_T2, S_PARTS8))
        e("s_lshr_b32 s%d, s%d, 6" % (S_T4, S_T3))
        e("s_lshl_b32 s%d, s%d, 3" % (S_T4, S_T4))
        e("s_add_u32 s%d, s%d, s%d" % (S_STOFF, S_STOFF, S_T4))
        e("v_bfe_u32 v%d, v0, 4, 2" % V_SQ)                                # lane / 16: row inside an emit pass
        e("v_mul_lo_u32 v%d, v%d, s%d" % (V_ST, V_SQ, S_PARTS8))
        e("v_add_u32 v%d, s%d, v%d" % (V_ST, S_STOFF, V_ST))
        e("v_mul_lo_u32 v%d, v%d, s%d" % (V_O16, V_SQ, S_LD16X2))
        e("v_and_b32 v%d, 15, v0" % V_SQ)
        e("v_lshl_add_u32 v%d, v%d, 3, v%d" % (V_O16, V_SQ, V_O16))       # + (lane & 15) * 4 columns * 2 bytes
        e("v_add_u32 v%d, s%d, v%d" % (V_O16, S_O16OFF, V_O16))

    def ln_producer_row(self, r, h, vm, slab):
        """folded-LayerNorm producer: v[r:r+3] = four consecutive final values of one row (16 lanes hold the row's 64 columns of this
        slab): their fp16 copy goes to out16, the row's (sum, sum of squares) over the 64 columns to stats[row][column group]."""
        e = self.e
        self.ln_producer_valu(r)
        e("buffer_store_dwordx2 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d%s" % (V_SQ, V_SQ + 1, V_O16, SRD_O16, SRD_O16 + 3, h * 128, self.sched.get("store16_policy", "")))
        vm.append(("st", slab))
        e("s_mov_b64 exec, s[%d:%d]" % (S_EXROW, S_EXROW + 1))
        e("buffer_store_dwordx2 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d" % (V_SUM, V_SUM + 1, V_ST, SRD_ST, SRD_ST + 3, h * 8))
        vm.append(("st", slab))
        e("s_mov_b64 exec, -1")

    def ln_producer_valu(self, r):
        e = self.e
        e("v_pk_add_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (V_SUM, V_SUM + 1, r, r + 1, r + 2, r + 3))
        e("v_pk_mul_f32 v[%d:%d], v[%d:%d], v[%d:%d]" % (V_SQ, V_SQ + 1, r, r + 1, r, r + 1))
        e("v_pk_fma_f32 v[%d:%d], v[%d:%d], v[%d:%d], v[%d:%d]" % (V_SQ, V_SQ + 1, r + 2, r + 3, r + 2, r + 3, V_SQ, V_SQ + 1))
        e("v_add_f32 v%d, v%d, v%d" % (V_SUM, V_SUM, V_SUM + 1))
        e("v_add_f32 v%d, v%d, v%d" % (V_SUM + 1, V_SQ, V_SQ + 1))
        # butterfly over the 16 lanes of the row (a DPP read of a VGPR needs two wait states after the VALU write: the two chains
        # and the fp16 conversions are interleaved)
        dpp = ("quad_perm:[1,0,3,2]", "quad_perm:[2,3,0,1]", "row_half_mirror", "row_mirror")
        fill = ["v_cvt_pk_f16_f32 v%d, v%d, v%d" % (V_SQ, r, r + 1), "v_cvt_pk_f16_f32 v%d, v%d, v%d" % (V_SQ + 1, r + 2, r + 3), "s_nop 0", "s_nop 0"]
        e("s_nop 0")
        for st in range(4):
            e("v_add_f32_dpp v%d, v%d, v%d %s row_mask:0xf bank_mask:0xf" % (V_SUM, V_SUM, V_SUM, dpp[st]))
            e("v_add_f32_dpp v%d, v%d, v%d %s row_mask:0xf bank_mask:0xf" % (V_SUM + 1, V_SUM + 1, V_SUM + 1, dpp[st]))
            e(fill[st])

    # ------------------------------------------------------------ whole kernel
    def kernel(self):
        e, n = self.e, self.name
        esize = 4 if self.epi == EPI_F32 else 2
        self.L += kernel_begin(n)
        e("s_load_dwordx16 s[4:19], s[0:1], 0x0")
        e("s_load_dwordx8 s[20:27], s[0:1], 0x40")
        if self.sched.get("trace"):
            e("s_load_dwordx2 s[%d:%d], s[0:1], 0x60" % (S_TRP, S_TRP + 1))
            e("s_memtime s[%d:%d]" % (S_TS0, S_TS0 + 1))
            e("s_waitcnt lgkmcnt(0)")
            e("s_mov_b32 s3, s%d" % S_TS0)                # kernel entry stamp (low half)
            e("s_memrealtime s[%d:%d]" % (S_TS0, S_TS0 + 1))
            e("s_waitcnt lgkmcnt(0)")
            e("s_mov_b32 s27, s%d" % S_TS0)               # the same on the constant 100 MHz clock
            for r in (S_ACC_LOOP, S_ACC_EPI, S_NKT):
                e("s_mov_b32 s%d, 0" % r)
        e("v_and_b32 v%d, 63, v0" % V_LANE)
        e("v_lshrrev_b32 v%d, 6, v0" % V_T0)
        e("s_nop 1")
        e("v_readfirstlane_b32 s%d, v%d" % (S_WV, V_T0))
        # lane -> (row of an MFMA block, k group): 32 rows x 2 groups, or 16 x 4 in the 16x16x32 form
        e("v_and_b32 v%d, %d, v%d" % (V_LR, 15 if self.m16 else 31, V_LANE))
        e("v_lshrrev_b32 v%d, %d, v%d" % (V_LG, 4 if self.m16 else 5, V_LANE))
        e("s_waitcnt lgkmcnt(0)")
        e("s_lshr_b32 s%d, s%d, 1" % (S_WR, S_WV))
        e("s_and_b32 s%d, s%d, 1" % (S_WC, S_WV))
        e("s_lshl_b32 s%d, s%d, 15" % (S_FA, S_WR))                       # A half-tile wr: (wr * 2) * 16384
        e("s_lshl_b32 s%d, s%d, 15" % (S_FB, S_WC))
        e("s_add_u32 s%d, s%d, 0x10000" % (S_FB, S_FB))                   # B half-tile wc: (2 + wc) * 2 * 16384
        e("s_lshl_b32 s%d, s%d, 1" % (S_LDA2, S_LDA))
        e("s_lshl_b32 s%d, s%d, 1" % (S_LDW2, S_LDW))
        e("s_lshr_b32 s%d, s%d, 6" % (S_NK, S_K))
        if self.sk:            # K-tiles per range: q = NK / ranges, rem = NK % ranges (ranges = kernarg `pad`, 2 ... 8: a few subtractions)
            lp, dn = self.u("L_skdiv"), self.u("L_skdiv_done")
            e("s_mov_b32 s%d, 0" % S_SKQ)
            e("s_mov_b32 s%d, s%d" % (S_SKREM, S_NK))
            self.lab(lp)
            e("s_cmp_lt_u32 s%d, s%d" % (S_SKREM, S_RMASK))
            e("s_cbranch_scc1 %s" % dn)
            e("s_sub_u32 s%d, s%d, s%d" % (S_SKREM, S_SKREM, S_RMASK))
            e("s_add_u32 s%d, s%d, 1" % (S_SKQ, S_SKQ))
            e("s_branch %s" % lp)
            self.lab(dn)
        e("s_lshl_b32 s%d, s%d, 10" % (S_M0BASE, S_WV))
        e("s_lshl_b32 s%d, s%d, 2" % (S_CUR, S_WG))
        e("s_lshl_b32 s%d, s%d, 2" % (S_STRIDE, S_G))
        e("s_load_dword s%d, s[%d:%d], s%d" % (S_TNEXT, S_TAB, S_TAB + 1, S_CUR))
        # descriptors: word 3, num_records of the epilogue operands
        for srd in (SRD_A, SRD_B, SRD_O, SRD_R, SRD_BIAS, SRD_GAM):
            e("s_mov_b32 s%d, 0x00020000" % (srd + 3))
        e("s_mov_b32 s%d, s%d" % (SRD_O, S_OUT)); e("s_mov_b32 s%d, s%d" % (SRD_O + 1, S_OUT + 1))
        e("s_mul_i32 s%d, s%d, s%d" % (SRD_O + 2, S_M, S_LDO)); e("s_lshl_b32 s%d, s%d, %d" % (SRD_O + 2, SRD_O + 2, 1 if esize == 2 else 2))
        if self.sk:            # all planes, each of whole tiles' rows (a last tile's rows beyond M land in its own plane's padding)
            e("s_add_u32 s%d, s%d, 255" % (S_T0, S_M))
            e("s_andn2_b32 s%d, s%d, 255" % (S_T0, S_T0))
            e("s_mul_i32 s%d, s%d, s%d" % (SRD_O + 2, S_T0, S_LDO))
            e("s_lshl_b32 s%d, s%d, 2" % (SRD_O + 2, SRD_O + 2))
            e("s_mul_i32 s%d, s%d, s%d" % (SRD_O + 2, SRD_O + 2, S_RMASK))
        e("s_mov_b32 s%d, s%d" % (SRD_R, S_RES)); e("s_mov_b32 s%d, s%d" % (SRD_R + 1, S_RES + 1))
        if self.sched.get("trace") or self.epi != EPI_F32 or self.sk:
            e("s_mul_i32 s%d, s%d, s%d" % (SRD_R + 2, S_M, S_LDR)); e("s_lshl_b32 s%d, s%d, 2" % (SRD_R + 2, SRD_R + 2))
        else:                      # rows of the residual operand: M, or resid_mod (mask + 1) when it is a per-image table
            e("s_add_u32 s%d, s%d, 1" % (S_T0, S_RMASK))
            e("s_cmp_eq_u32 s%d, -1" % S_RMASK)
            e("s_cselect_b32 s%d, s%d, s%d" % (S_T0, S_M, S_T0))
            e("s_mul_i32 s%d, s%d, s%d" % (SRD_R + 2, S_T0, S_LDR)); e("s_lshl_b32 s%d, s%d, 2" % (SRD_R + 2, SRD_R + 2))
        e("s_mov_b32 s%d, s%d" % (SRD_BIAS, S_BIAS)); e("s_mov_b32 s%d, s%d" % (SRD_BIAS + 1, S_BIAS + 1))
        e("s_lshl_b32 s%d, s%d, 2" % (SRD_BIAS + 2, S_N))
        e("s_mov_b32 s%d, s%d" % (SRD_GAM, S_GAM)); e("s_mov_b32 s%d, s%d" % (SRD_GAM + 1, S_GAM + 1))
        e("s_lshl_b32 s%d, s%d, 2" % (SRD_GAM + 2, S_N))
        # null operands: zero-sized descriptors (loads return 0)
        for ptr, srd in ((S_BIAS, SRD_BIAS), (S_RES, SRD_R), (S_GAM, SRD_GAM)):
            e("s_or_b32 s%d, s%d, s%d" % (S_T0, ptr, ptr + 1))
            e("s_cmp_eq_u32 s%d, 0" % S_T0)
            e("s_cselect_b32 s%d, 0, s%d" % (srd + 2, srd + 2))
        # ---- fragment read addresses
        e("v_lshrrev_b32 v%d, 1, v%d" % (V_T0, V_LR))
        e("v_and_b32 v%d, 7, v%d" % (V_T0, V_T0))                          # sw = (lr >> 1) & 7
        e("v_lshlrev_b32 v%d, 7, v%d" % (V_T1, V_LR))                      # lr * 128
        for ks in range(2 if self.m16 else 4):
            e("v_or_b32 v%d, %d, v%d" % (V_T2, (4 if self.m16 else 2) * ks, V_LG))
            e("v_xor_b32 v%d, v%d, v%d" % (V_T2, V_T2, V_T0))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_T2, V_T2, V_T1))
            e("v_add_u32 v%d, s%d, v%d" % (self.M16_FA[ks] if self.m16 else V_FA + ks, S_FA, V_T2))
            e("v_add_u32 v%d, s%d, v%d" % (self.M16_FB[ks] if self.m16 else V_FB + ks, S_FB, V_T2))
        # ---- DMA offsets: piece j covers rows j*32 + wv*8 + lane/8, LDS slot lane%8 <- source chunk slot ^ ((row>>1)&7)
        e("v_lshrrev_b32 v%d, 3, v%d" % (V_T0, V_LANE))
        e("s_lshl_b32 s%d, s%d, 3" % (S_T0, S_WV))
        e("v_add_u32 v%d, s%d, v%d" % (V_T0, S_T0, V_T0))                  # r_in = wv*8 + lane/8
        e("v_lshrrev_b32 v%d, 1, v%d" % (V_T1, V_T0))
        e("v_and_b32 v%d, 7, v%d" % (V_T1, V_T1))
        e("v_and_b32 v%d, 7, v%d" % (V_T2, V_LANE))
        e("v_xor_b32 v%d, v%d, v%d" % (V_T1, V_T1, V_T2))
        e("v_lshlrev_b32 v%d, 4, v%d" % (V_T1, V_T1))                      # chunk * 16 bytes
        for j in range(8):
            e("v_add_u32 v%d, %d, v%d" % (V_T2, j * 32, V_T0))
            e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T3, V_T2, S_LDA2))
            e("v_add_u32 v%d, v%d, v%d" % (V_DA + j, V_T3, V_T1))
            e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T3, V_T2, S_LDW2))
            e("v_add_u32 v%d, v%d, v%d" % (V_DB + j, V_T3, V_T1))
        # ---- epilogue lane constants
        e("s_lshl_b32 s%d, s%d, 13" % (S_T0, S_WV))
        e("s_add_u32 s%d, s%d, 0x%x" % (S_T0, S_T0, LDS_SLAB))             # slab base of this wave
        e("v_and_b32 v%d, 15, v%d" % (V_T0, V_LR))                          # lr & 15
        e("v_lshlrev_b32 v%d, 8, v%d" % (V_T1, V_LR))                       # lr * 256
        e("v_add_u32 v%d, s%d, v%d" % (V_T1, S_T0, V_T1))
        if self.m16 and self.epi == EPI_F32:
            e("v_xor_b32 v%d, v%d, v%d" % (V_T0, V_T0, V_LG))                # row ^ g
            for cbl in range(4):                                            # chunk16 = cbl*4 (+ g)
                e("v_xor_b32 v%d, %d, v%d" % (V_T2, 4 * cbl, V_T0))
                e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_PARK + cbl, V_T2, V_T1))
        elif self.m16:
            e("v_lshrrev_b32 v%d, 1, v%d" % (V_T2, V_LG))
            e("v_xor_b32 v%d, v%d, v%d" % (V_T0, V_T0, V_T2))                # row ^ (g >> 1)
            e("v_and_b32 v%d, 1, v%d" % (V_T2, V_LG))
            e("v_lshl_add_u32 v%d, v%d, 3, v%d" % (V_T1, V_T2, V_T1))        # + (g & 1) * 8
            for cb in range(8):                                             # chunk16 = cb*2 (+ g >> 1)
                e("v_xor_b32 v%d, %d, v%d" % (V_T2, 2 * cb, V_T0))
                e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_PARK + cb, V_T2, V_T1))
        elif self.epi == EPI_F32:
            e("v_xor_b32 v%d, v%d, v%d" % (V_T0, V_T0, V_LG))                # (lr & 15) ^ lg
            for cq in range(8):                                             # chunk16 = cbl*8 + 2q (+ lg)
                e("v_xor_b32 v%d, %d, v%d" % (V_T2, (cq >> 2) * 8 + 2 * (cq & 3), V_T0))
                e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_PARK + cq, V_T2, V_T1))
        else:
            e("v_lshl_add_u32 v%d, v%d, 3, v%d" % (V_T1, V_LG, V_T1))        # + lg * 8
            for cq in range(16):
                e("v_xor_b32 v%d, %d, v%d" % (V_T2, cq, V_T0))
                e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_PARK + cq, V_T2, V_T1))
        # emit reads: row = it*4 + lane/16, chunk = (lane & 15) ^ (row & 15); 256-byte rows
        e("v_lshrrev_b32 v%d, 4, v%d" % (V_T0, V_LANE))                     # lane / 16
        e("v_and_b32 v%d, 15, v%d" % (V_T1, V_LANE))
        for i in range(4):
            e("v_add_u32 v%d, %d, v%d" % (V_T2, 4 * i, V_T0))               # row (it = i)
            e("v_xor_b32 v%d, v%d, v%d" % (V_T3, V_T2, V_T1))
            e("v_and_b32 v%d, 15, v%d" % (V_T3, V_T3))
            e("v_lshlrev_b32 v%d, 4, v%d" % (V_T3, V_T3))
            e("v_lshl_add_u32 v%d, v%d, 8, v%d" % (V_T3, V_T2, V_T3))
            e("v_add_u32 v%d, s%d, v%d" % (V_EADDR + i, S_T0, V_T3))
        # output lane offsets: row wr*128 + lane/16, column wc*128 + (lane&15) * (16 bytes / esize)
        e("s_lshl_b32 s%d, s%d, 7" % (S_T1, S_WR))
        e("v_add_u32 v%d, s%d, v%d" % (V_T2, S_T1, V_T0))                    # row in tile
        e("s_lshl_b32 s%d, s%d, 7" % (S_T2, S_WC))                           # wc * 128 columns
        cols = 8 if esize == 2 else 4
        e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T3, V_T2, S_LDO))
        e("v_mad_u32_u24 v%d, v%d, %d, v%d" % (V_T3, V_T1, cols, V_T3))
        e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T2, V_T3))
        e("v_lshlrev_b32 v%d, %d, v%d" % (V_OLANE, 1 if esize == 2 else 2, V_T3))
        e("s_lshl_b32 s%d, s%d, %d" % (S_ROW4, S_LDO, 3 if esize == 2 else 4))    # 4 rows of out, bytes
        e("s_mul_i32 s%d, s%d, 7" % (S_ROW28, S_ROW4))
        if self.epi == EPI_F32:
            e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T3, V_T2, S_LDR))
            e("v_mad_u32_u24 v%d, v%d, 4, v%d" % (V_T3, V_T1, V_T3))
            e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T2, V_T3))
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_RLANE, V_T3))
            e("s_lshl_b32 s%d, s%d, 4" % (S_RROW4, S_LDR))
            e("s_mul_i32 s%d, s%d, 7" % (S_RROW28, S_RROW4))
            # bias / gamma lane offset (emit layout): (wc*128 + (lane&15)*4) * 4 bytes
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_T3, V_T1))
            e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T2, V_T3))
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_TMP + 11, V_T3))
        else:
            # bias lane offset (accumulator layout): (wc*128 + 4*lg) * 4 bytes
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_T3, V_LG))
            e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T2, V_T3))
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_TMP + 11, V_T3))
        if self.epi == EPI_GELU_F16:                # the polynomial of gelu_quad: [0:1] c4, [2:3] c2, [4:5] c1, [6:7] c0; c3 in two VGPRs
            for i, cst in enumerate(GELU_SGPR_CONSTS):
                e("s_mov_b32 s%d, 0x%08x" % (S_C + i, cst))
            e("v_mov_b32 v%d, 0x%08x" % (V_TMP + 8, GELU_C3))
            e("v_mov_b32 v%d, 0x%08x" % (V_TMP + 9, GELU_C3))
        if self.lnp:
            # kernarg 104: out16 pointer, 112: stats pointer, 120: ld16
            e("s_load_dwordx4 s[%d:%d], s[0:1], 0x68" % (SRD_O16, SRD_O16 + 3))
            e("s_load_dword s%d, s[0:1], 0x78" % S_LD16X2)
            e("s_waitcnt lgkmcnt(0)")
            e("s_mov_b32 s%d, s%d" % (SRD_ST, SRD_O16 + 2)); e("s_mov_b32 s%d, s%d" % (SRD_ST + 1, SRD_O16 + 3))
            e("s_lshl_b32 s%d, s%d, 1" % (S_LD16X2, S_LD16X2))                  # bytes per row of out16
            e("s_mul_i32 s%d, s%d, s%d" % (SRD_O16 + 2, S_M, S_LD16X2)); e("s_mov_b32 s%d, 0x00020000" % (SRD_O16 + 3))
            e("s_lshr_b32 s%d, s%d, 6" % (S_PARTS8, S_N)); e("s_lshl_b32 s%d, s%d, 3" % (S_PARTS8, S_PARTS8))   # bytes per row of stats
            e("s_mul_i32 s%d, s%d, s%d" % (SRD_ST + 2, S_M, S_PARTS8)); e("s_mov_b32 s%d, 0x00020000" % (SRD_ST + 3))
            e("s_lshl_b32 s%d, s%d, 2" % (S_O16ROW4, S_LD16X2)); e("s_mul_i32 s%d, s%d, 7" % (S_O16ROW28, S_O16ROW4))
            e("s_lshl_b32 s%d, s%d, 2" % (S_STROW4, S_PARTS8)); e("s_mul_i32 s%d, s%d, 7" % (S_STROW28, S_STROW4))
            e("s_mov_b32 s%d, 0x00010001" % S_EXROW); e("s_mov_b32 s%d, 0x00010001" % (S_EXROW + 1))
        if self.lnc:
            # `resid` = fp32 (mean, rstd) [M][2] followed by the fp16 fragments of -mean [M][8]; `gamma` = the fp16 fragments of s [N][8]
            e("s_mov_b32 s%d, s%d" % (SRD_MR, S_RES)); e("s_mov_b32 s%d, s%d" % (SRD_MR + 1, S_RES + 1))
            e("s_lshl_b32 s%d, s%d, 3" % (SRD_MR + 2, S_M)); e("s_mov_b32 s%d, 0x00020000" % (SRD_MR + 3))
            e("s_add_u32 s%d, s%d, s%d" % (SRD_MF, S_RES, SRD_MR + 2)); e("s_addc_u32 s%d, s%d, 0" % (SRD_MF + 1, S_RES + 1))
            e("s_lshl_b32 s%d, s%d, 4" % (SRD_MF + 2, S_M)); e("s_mov_b32 s%d, 0x00020000" % (SRD_MF + 3))
            e("s_mov_b32 s%d, s%d" % (SRD_SF, S_GAM)); e("s_mov_b32 s%d, s%d" % (SRD_SF + 1, S_GAM + 1))
            e("s_lshl_b32 s%d, s%d, 4" % (SRD_SF + 2, S_N)); e("s_mov_b32 s%d, 0x00020000" % (SRD_SF + 3))
            e("v_lshlrev_b32 v%d, 4, v%d" % (V_T0, V_LR))                     # (lane & 31) * 16
            e("s_lshl_b32 s%d, s%d, 11" % (S_T0, S_WC))                       # wc * 128 * 16
            e("s_lshl_b32 s%d, s%d, 11" % (S_T1, S_WR))
            e("v_add_u32 v%d, s%d, v%d" % (V_T1, S_T0, V_T0))
            e("v_add_u32 v%d, s%d, v%d" % (V_T2, S_T1, V_T0))
            e("v_mov_b32 v%d, 0x40000000" % V_T3)                             # lanes 32..63 (k = 8..15): far beyond the buffers -> zeros
            e(("v_cmp_ne_u32 vcc, 0, v%d" if self.m16 else "v_cmp_eq_u32 vcc, 1, v%d") % V_LG)     # (16x16x32 form: lanes 16..63)
            e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (V_T1, V_T1, V_T3))
            e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (V_T2, V_T2, V_T3))
            e("v_lshlrev_b32 v%d, 3, v%d" % (V_T0, V_LR))                     # (lane & 31) * 8: (mean, rstd) row
            e("s_lshl_b32 s%d, s%d, 10" % (S_T1, S_WR))
            e("s_add_u32 s%d, s%d, 4" % (S_T1, S_T1))
            e("v_add_u32 v%d, s%d, v%d" % (V_RSOFF, S_T1, V_T0))
            e("v_mov_b32 v%d, v%d" % (V_SFOFF, V_T1))
            e("v_mov_b32 v%d, v%d" % (V_MFOFF, V_T2))
        # ---- first tile
        e("s_waitcnt lgkmcnt(0)")
        e("s_cmp_eq_u32 s%d, -1" % S_TNEXT)
        e("s_cbranch_scc1 L_exit_%s" % n)
        self.switch_tile()
        for kt in range(2):
            for p in range(16):
                e(self.dma_m0(p))
                e("s_nop 0")
                e(self.dma_issue(p))
            for ins in self.dma_advance():
                e(ins)
            e("s_xor_b32 s%d, s%d, 0x%x" % (S_M0BASE, S_M0BASE, LDS_BUF))
        e("s_mov_b32 s%d, s%d" % (S_TCUR, S_TDMA))
        if self.sk:
            self.item_ktiles(S_TCUR, S_KREM)
        else:
            e("s_mov_b32 s%d, s%d" % (S_KREM, S_NK))
        e("s_waitcnt vmcnt(16)")
        e("s_barrier")
        if self.m16:
            self.kloop16()
        else:
            self.kloop32()
        self.after_kloop()

    def kloop16(self):
        """the K-tile loop of the 16x16x32 form: 2 k-steps of 64 MFMAs; k-step 0 exists twice (C = 0 for a tile's first K-tile)"""
        e, n = self.e, self.name
        for idx in self.RD16_ORDER:
            e(self.frag_read16(0, idx))
        for r in (self.M16_FA[0], self.M16_FB[0]):
            e("v_xor_b32 v%d, 0x%x, v%d" % (r, LDS_BUF, r))
        slots, zslots, waits = self.build_slots16(), self.build_slots16(True), self.lgkm_waits16()
        def run(sl, lo, hi, zero):
            for s in range(lo, hi):
                if s in waits:
                    e("s_waitcnt lgkmcnt(%d)" % waits[s])
                e(self.mfma16(s // 64, (s % 64) // 8, s % 8, zero))
                for ins in sl[s]:
                    if ins.endswith(":"):
                        self.lab(ins[:-1])
                    else:
                        e(ins)
        self.lab("L_tile_begin_%s" % n)
        if self.sched.get("trace"):
            e("s_memtime s[%d:%d]" % (S_TS0, S_TS0 + 1))
        run(zslots, 0, 64, True)
        e("s_branch L_after_ks0_%s" % n)
        self.L.append(".p2align 4")
        self.lab("L_loop_%s" % n)
        run(slots, 0, 64, False)
        self.lab("L_after_ks0_%s" % n)
        run(slots, 64, 128, False)
        e("s_xor_b32 s%d, s%d, 0x%x" % (S_M0BASE, S_M0BASE, LDS_BUF))
        for r in (self.M16_FA[0], self.M16_FB[0]):
            e("v_xor_b32 v%d, 0x%x, v%d" % (r, LDS_BUF, r))
        e("s_sub_u32 s%d, s%d, 1" % (S_KREM, S_KREM))
        e("s_cmp_eq_u32 s%d, 0" % S_KREM)
        e("s_cbranch_scc0 L_loop_%s" % n)

    def kloop32(self):
        e, n = self.e, self.name
        for i in range(16):
            e(self.frag_read(i // 8, i // 8, i % 8))
        for r in (V_FA, V_FA + 1, V_FB, V_FB + 1):
            e("v_xor_b32 v%d, 0x%x, v%d" % (r, LDS_BUF, r))
        slots = self.build_slots()
        # k-step 0 exists twice: with C = 0 (first K-tile of an output tile) and accumulating
        self.lab("L_tile_begin_%s" % n)
        if self.sched.get("trace"):
            e("s_memtime s[%d:%d]" % (S_TS0, S_TS0 + 1))
        self.ktile(slots, True)
        self.L.append(".p2align 4")
        self.lab("L_loop_%s" % n)
        e("s_waitcnt lgkmcnt(8)")
        for s in range(16):
            e(self.mfma(0, s // 4, s % 4, False))
            for ins in slots[s]:
                e(ins)
        self.lab("L_after_ks0_%s" % n)
        for s in range(16, 64):
            ks, rb, cb = s // 16, (s % 16) // 4, s % 4
            if s == 16:
                e("s_waitcnt lgkmcnt(15)")
            e(self.mfma(ks, rb, cb, False))
            for ins in slots[s]:
                if ins.endswith(":"):
                    self.lab(ins[:-1])
                else:
                    e(ins)
        for r in (V_FA, V_FA + 1, V_FB, V_FB + 1):
            e("v_xor_b32 v%d, 0x%x, v%d" % (r, LDS_BUF, r))
        e("s_sub_u32 s%d, s%d, 1" % (S_KREM, S_KREM))
        e("s_cmp_eq_u32 s%d, 0" % S_KREM)
        e("s_cbranch_scc0 L_loop_%s" % n)

    def after_kloop(self):
        e, n = self.e, self.name
        esize = 4 if self.epi == EPI_F32 else 2
        # ---- tile finished
        if self.sched.get("trace"):
            e("s_memtime s[%d:%d]" % (S_TS1, S_TS1 + 1))
            e("s_waitcnt lgkmcnt(0)")
            e("s_sub_u32 s%d, s%d, s%d" % (S_T0, S_TS1, S_TS0))
            e("s_add_u32 s%d, s%d, s%d" % (S_ACC_LOOP, S_ACC_LOOP, S_T0))
            e("s_add_u32 s%d, s%d, s%d" % (S_NKT, S_NKT, S_NK))
        # memory operations between the operand requests of the last K-tile and the epilogue: that K-tile's DMA pieces
        n_dma_after = sum(1 for p in range(16) if self.sched["dma"][p] > self.sched.get("pre_slot", 17))
        assert not self.m16 or n_dma_after in (0, 16)
        pre_lines = self.L
        self.L = []
        vm = self.pre_epilogue()
        self.pre_code = self.L
        self.L = pre_lines
        # (the 16x16x32 form requests the folded-LayerNorm operands with the others: all sixteen pieces follow)
        n_late = n_dma_after if self.m16 else sum(1 for p in range(16) if self.sched["dma"][p] > 48)
        vm += [("dma", 0)] * (n_dma_after - n_late)
        if self.lnc:
            pre_lines = self.L
            self.L = []
            vm += self.pre2_epilogue()
            self.pre2_code = self.L
            self.L = pre_lines
        vm += [("dma", 0)] * n_late
        if self.epi == EPI_F32:
            self.epilogue_f32(vm)
        else:
            self.epilogue_f16(self.epi == EPI_GELU_F16, vm)
        if self.sched.get("trace"):
            e("s_memtime s[%d:%d]" % (S_TS0, S_TS0 + 1))
            e("s_waitcnt lgkmcnt(0)")
            e("s_sub_u32 s%d, s%d, s%d" % (S_T0, S_TS0, S_TS1))
            e("s_add_u32 s%d, s%d, s%d" % (S_ACC_EPI, S_ACC_EPI, S_T0))
        e("s_mov_b32 s%d, s%d" % (S_TCUR, S_TDMA))
        if self.sk:
            self.item_ktiles(S_TCUR, S_KREM)
        else:
            e("s_mov_b32 s%d, s%d" % (S_KREM, S_NK))
        e("s_cmp_eq_u32 s%d, -1" % S_TCUR)
        e("s_cbranch_scc0 L_tile_begin_%s" % n)
        self.lab("L_exit_%s" % n)
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")
        if self.sched.get("trace"):
            done = self.u("L_trace_done")
            e("s_cmp_eq_u32 s%d, 0" % S_WV)
            e("s_cbranch_scc0 %s" % done)
            e("s_lshl_b32 s%d, s%d, 4" % (S_T0, S_WG))
            e("v_mov_b32 v%d, s%d" % (V_T0, S_T0))
            e("v_mov_b32 v%d, s%d" % (V_EM[0], S_ACC_LOOP))
            e("v_mov_b32 v%d, s%d" % (V_EM[0] + 1, S_ACC_EPI))
            e("v_mov_b32 v%d, s%d" % (V_EM[0] + 2, S_NKT))
            e("s_memtime s[%d:%d]" % (S_TS0, S_TS0 + 1))
            e("s_waitcnt lgkmcnt(0)")
            e("s_sub_u32 s3, s%d, s3" % S_TS0)
            e("v_mov_b32 v%d, s3" % (V_EM[0] + 3))          # cycles from kernel entry to the last store's completion
            e("global_store_dwordx4 v%d, v[%d:%d], s[%d:%d]" % (V_T0, V_EM[0], V_EM[0] + 3, S_TRP, S_TRP + 1))
            e("s_memrealtime s[%d:%d]" % (S_TS0, S_TS0 + 1))
            e("s_waitcnt lgkmcnt(0)")
            e("s_sub_u32 s27, s%d, s27" % S_TS0)
            e("s_lshl_b32 s%d, s%d, 4" % (S_T0, S_G))
            e("v_add_u32 v%d, s%d, v%d" % (V_T0, S_T0, V_T0))
            e("v_mov_b32 v%d, s27" % V_EM[0])               # second array (behind the first): entry -> exit in 10 ns ticks
            e("global_store_dwordx4 v%d, v[%d:%d], s[%d:%d]" % (V_T0, V_EM[0], V_EM[0] + 3, S_TRP, S_TRP + 1))
            e("s_waitcnt vmcnt(0)")
            self.lab(done)
        e("s_endpgm")
        # out of line: DMA side switches to the next tile
        self.lab("L_switch_%s" % n)
        self.switch_tile()
        e("s_branch L_switch_ret_%s" % n)
        if self.m16:               # the same from the C = 0 copy of k-step 0
            self.lab("L_switch_z_%s" % n)
            self.switch_tile()
            e("s_branch L_switch_ret_z_%s" % n)
        self.lab("L_pre_%s" % n)
        self.L += self.pre_code
        if self.lnc and self.m16:
            self.L += self.pre2_code
        e("s_branch L_pre_ret_%s" % n)
        if self.lnc and not self.m16:
            self.lab("L_pre2_%s" % n)
            self.L += self.pre2_code
            e("s_branch L_pre2_ret_%s" % n)
        self.L += kernel_end(n, 163840, 128 if self.lnp else 104, NUM_SGPR)

    def metadata(self):
        # kernarg: A, W, bias, out, resid, gamma, table; M, N, K, lda, ldw, ldo, ldr, G, flags, pad; trace; producer: out16, stats; ld16, pad
        args = ["ptr"] * 7 + ["i32"] * 10 + ["ptr"] + (["ptr"] * 2 + ["i32"] * 2 if self.lnp else [])
        return kernel_metadata(self.name, args, 163840, NUM_SGPR)


def default_sched():
    # slot = index of the MFMA (0..63) a side instruction is emitted behind
    return {
        "rd23": list(range(16)),                 # S2 / S3 reads: one per MFMA of k-step 0
        "tog23": 16,
        "barA": 19,
        "dma": [21 + (5 * p) // 2 for p in range(16)],   # one piece per 2.5 MFMAs: the four waves issue in lockstep and the CU's vector L1 takes
                                                          # 64 cycles for their 4 KiB (cycles per K-tile: consecutive slots 2700, 1.5 slots 2350,
                                                          # 2 slots 2250, 2.5 slots 2190, 2.75 slots 2210)
        "barB": 46,
        "rd01": [47 + i for i in range(16)],
        # the residual rows are read once: as streaming loads (nt) they do not displace the operand panels the OTHER workgroups of
        # the XCD are re-reading from its L2 - with the default policy every fp32-epilogue launch ran its k-loops at ~3000 cycles per
        # K-tile instead of ~2370 (65536x1280x1280: 3040 -> 2380; streaming stores alone change nothing)
        "resid_policy": " nt",
        # ... and the output rows are written once and read by the NEXT launch (at 16 slices 0.3-0.7 GB, far beyond the L2): as
        # streaming stores they leave the operand panels in the L2 too (k-loop of qkv 2230 -> 2170, fc1 2330 -> 2160 cycles per K-tile;
        # qkv / proj / fc1 / fc2 at 65536 rows +3.3 / +3 / +4 / +1 %)
        "store_policy": " nt",
    }


def m16_sched(base=None):
    """the 16x16x32 schedule of the same tile: slot = index of the MFMA (0..127, 16 cycles each) a side instruction is emitted behind.
    One DMA piece per 5 slots = 80 cycles (the 2.5 32-cycle slots of the form above), each alone in its gap, its m0 in the gap before."""
    dma = [41 + 5 * p for p in range(16)]
    busy = set(dma) | set(d - 1 for d in dma)
    free = [s for s in range(93, 128) if s not in busy]
    return dict(base or default_sched(), mfma="16x16x32",
                rd1=[1 + 2 * i for i in range(16)],      # k-step 1's reads: every second gap of the first 32
                tog1=(32, 35), pre_slot=33, barA=36, dma=dma, barB=92,
                rd0=free[:16], adv=free[16])             # the next K-tile's k-step 0 in the free gaps behind barrier B, then the nine SALU of the advance


# Measured against these schedules and dropped: a start-time stagger of the workgroups, so that their epilogue bursts do not coincide.
# 2 / 4 / 8 groups 8k or 16k cycles apart (every XCD holds all groups): 65536x1280x1280 897 / 850 TFLOP/s unstaggered against
# 739-888 / 824-876. The two halves of the chip (XCDs 0..3 / 4..7) 16k ... 48k cycles apart: 884 / 849 against 719-861,
# 65536x1280x5120 1153 / 1178 against 1144-1183, 131072x1280x1280 910 / 891 against 887-913. Nothing on any of the four SAM shapes: the
# epilogue's ~24 bytes per cycle and CU are not a share of a saturated memory system (the other half of the chip being in its k-loops
# does not make it faster).


def variants(trace=False):
    """(kernel name, epilogue, schedule) of every kernel of the library; trace: also the `_v1` forms that count cycles per K-tile loop
    and per epilogue (tools/gemm_asm_ab.py reads them back; psam_gemm_asm_variant(1) selects them)"""
    base = default_sched()
    out = [("psam_gemm_asm_f16", EPI_F16, base), ("psam_gemm_asm_gelu", EPI_GELU_F16, base), ("psam_gemm_asm_f32", EPI_F32, base)]
    # the same kernels with the default cache policy for the epilogue's loads and stores: for outputs the next launch finds in the L2
    # (one slice at a time: 10-30 MB), where the streaming forms cost ~0.5 % of the step
    keep = dict(base, resid_policy="", store_policy="")
    out += [("psam_gemm_asm_f16_l2", EPI_F16, keep), ("psam_gemm_asm_gelu_l2", EPI_GELU_F16, keep), ("psam_gemm_asm_f32_l2", EPI_F32, keep)]
    # LayerNorm folded into the GEMMs either side of it (psam_gemm_f16_ln): consumers (fp16 / GELU) and the producer (fp32)
    # (what the producer's extra work costs, 65536x1280x1280 / x5120 TFLOP/s, plain kernel 785 / 1169: full 741 / 1145 - without the
    # fp16 copy's stores 787 / 1166, without the statistics' stores 756 / 1133, without their arithmetic 732 / 1140, without all
    # three 815 / 1178)
    # split-K form of the fp32 kernel (round 6): items are (tile, K range), the partial sums of a range go to its plane of the workspace
    # (default cache policy: the reduce pass behind it reads them from the L2 / memory-side cache)
    out += [("psam_gemm_asm_f32_sk", EPI_F32, dict(keep, splitk=True))]
    ln = dict(base, ln_cons=True, ln_prod=True, store16_policy=" nt")
    out += [("psam_gemm_asm_f16_ln", EPI_F16, ln), ("psam_gemm_asm_gelu_ln", EPI_GELU_F16, ln), ("psam_gemm_asm_f32_ln", EPI_F32, ln)]
    # the same tile on v_mfma_f32_16x16x32_f16 (csrc/gemm.hip tile 17): plain and folded-LayerNorm forms
    out += [("psam_gemm_asm_f16_m16", EPI_F16, m16_sched(base)), ("psam_gemm_asm_gelu_m16", EPI_GELU_F16, m16_sched(base)), ("psam_gemm_asm_f32_m16", EPI_F32, m16_sched(base))]
    out += [("psam_gemm_asm_f16_ln_m16", EPI_F16, m16_sched(ln)), ("psam_gemm_asm_gelu_ln_m16", EPI_GELU_F16, m16_sched(ln)), ("psam_gemm_asm_f32_ln_m16", EPI_F32, m16_sched(ln))]
    if trace:
        traced = dict(base, trace=True)
        for suffix, sc in (("_m16_v1", m16_sched(traced)), ("_v1", traced)):
            out += [("psam_gemm_asm_f16" + suffix, EPI_F16, sc), ("psam_gemm_asm_gelu" + suffix, EPI_GELU_F16, sc), ("psam_gemm_asm_f32" + suffix, EPI_F32, sc)]
    return out


def main():
    """no argument: the module of the library; --trace: with the traced `_v1` kernels; --meta: the header gemm_asm_meta.h"""
    trace = "--trace" in sys.argv[1:]
    import gemm_asm2_gen                      # the half-tile ping-pong kernels (tile 16) live in the same code object
    l2, meta2, es = gemm_asm2_gen.build_all(trace)
    if "--meta" in sys.argv[1:]:                  # header for csrc/gemm.hip: K-tile iterations the hidden epilogues need
        out = ["// generated by gemm_asm_gen.py --meta: a half-tile's epilogue is spread over E K-tile iterations of the next one"]
        for nm in ("f16", "gelu", "f32"):
            out.append("#define PSAM_ASM2_E_%s %d" % (nm.upper(), es["psam_gemm_asm2_" + nm]))
        sys.stdout.write("\n".join(out) + "\n")
        return
    ks = variants(trace)
    lines = []
    meta = []
    for name, epi, sc in ks:
        g = Gen(name, epi, sc)
        g.kernel()
        lines += g.L
        meta.append(g.metadata())
    lines += l2
    meta += meta2
    import gattn_asm_gen                      # the hand-scheduled global attention kernel shares the code object
    l3, meta3 = gattn_asm_gen.build_all()
    lines += l3
    meta += meta3
    import wattn_asm_gen                      # ... and the window attention kernel
    l4, meta4 = wattn_asm_gen.build_all()
    lines += l4
    meta += meta4
    sys.stdout.write(module_text(lines, meta))


if __name__ == "__main__":
    main()
