#!/usr/bin/env python3
"""Generator of the second assembly GEMM of psam_gemm_f16 (tile 16): half-tile ping-pong with a hidden epilogue.

Same product as gemm_asm_gen.py (out = epilogue(A[M,K] . W[N,K]^T), fp16 operands, fp32 accumulation; the Linear layers of
/root/reference/models/segment_anything/modeling/image_encoder.py:223-249, common.py:13-26). What changes is WHEN the epilogue
runs. Measured on the first kernel (tools/gemm_asm_ab.py): the k-loop takes 2240 cycles per 256x256x64 K-tile (2048 of MFMA
issue), but the epilogue of a tile takes 5.5k (fp16) / 20k (GELU: VALU-bound) / 26k (fp32 residual: store- and load-issue
bound) cycles during which the matrix pipe idles - 11 ... 36 % of a tile.

Here a workgroup (four waves, one per SIMD) walks HALF-tiles of 256 rows x 128 columns; a wave owns 128 x 64 of it = 8 blocks
of v_mfma_f32_32x32x16_f16 = 128 accumulator registers, and there are TWO accumulator sets: while half-tile i accumulates into
one, the epilogue of half-tile i-1 (bias / GELU / residual, transposition through the wave's LDS slab, stores) drains the other
from inside the MFMA shadows of the first E K-tile iterations - its instructions are placed by a small list scheduler into the
slots behind the MFMAs (VALU capped per slot, LDS traffic only where no fragment read is in flight, memory operations behind the
barrier whose counted wait they ride on). Price: a 256x128 tile re-reads the A panel, 1.5x the LDS-DMA bytes per MFMA.

  * LDS: three K-tile buffers of 48 KiB ([A0 A1 B] half-tiles of [128][64] fp16, XOR-swizzled) + 4 KiB slab per wave = 160 KiB;
    the DMA runs three K-tiles ahead of the MFMAs (twelve 1 KiB pieces per wave and K-tile, spread over the iteration);
  * the whole K-tile's fragments in registers (four sets of 24 VGPRs), two barriers per K-tile, counted waits;
  * the K-tile stream is continuous across half-tiles; the first half-tile of a workgroup runs a dummy epilogue with a
    zero-sized output descriptor, the last one is followed by a stand-alone drain of the same instruction stream.

Run:  python3 gemm_asm2_gen.py [--trace] > gemm_asm2.s
"""
import sys

from asm_common import AsmWriter, kernel_begin, kernel_end, kernel_metadata, module_text, younger

# ---------------------------------------------------------------- register map
S_WG = 2
S_A, S_W, S_BIAS, S_OUT, S_RES, S_GAM, S_TAB = 4, 6, 8, 10, 12, 14, 16
S_M, S_N, S_K, S_LDA, S_LDW, S_LDO, S_LDR, S_G, S_FLAGS = 18, 19, 20, 21, 22, 23, 24, 25, 26
SRD_A, SRD_B, SRD_O, SRD_R, SRD_BIAS, SRD_GAM = 28, 32, 36, 40, 44, 48
S_C = 52                         # s[52:54] scalar constants of the GELU
S_BUFP, S_BUFM = 56, 57           # +1 buffer / -2 buffers in bytes
S_ROW24, S_RROW24 = 60, 61
S_TPREV, S_ONREC, S_BUFI = 65, 66, 67
S_M0BASE = 68
S_KREM, S_DKREM, S_NK = 69, 70, 71
S_TCUR, S_TDMA, S_TNEXT, S_CUR, S_STRIDE = 72, 73, 74, 75, 76
S_WV, S_WR, S_WC = 77, 78, 79
S_FA, S_FB = 80, 81
S_LDA2, S_LDW2 = 82, 83
S_T0, S_T1, S_T2, S_T3, S_T4 = 84, 85, 86, 87, 88
S_ROW8, S_TOFF, S_N0X4, S_ROFF, S_RROW8 = 89, 90, 91, 92, 93
S_D23, S_D01 = 94, 95
S_ACC_LOOP, S_ACC_EPI, S_NKT = 62, 63, 64
S_TS0, S_TS1, S_TRP = 96, 98, 100
NUM_SGPR = 102

V_FA, V_FB = 1, 5                # fragment read addresses per k-step
V_DA, V_DB = 9, 17               # DMA offsets: 8 A pieces, 4 B pieces
V_LANE, V_LR, V_LG, V_T0, V_T1, V_T2, V_T3 = 21, 22, 23, 24, 25, 26, 27
V_SET = [32, 56, 80, 104]        # fragment sets: +0..15 X (A) fragments rb = 0..3, +16..23 W (B) fragments cb = 0..1
V_OLANE, V_O, V_RLANE, V_R = 128, 129, 130, 131
V_PARK = 132                     # 8 (fp16) / 4 (fp32) park addresses
V_EADDR = 140                    # 2 emit read addresses (even / odd 8-row group)
V_EM = [144, 160]                # two sets of 16 emit registers
V_GAM = 160                      # fp32: LayerScale gamma in the emit layout, [accumulator set][cb][4] (the fp32 epilogue uses one emit set)
V_BIAS = 176                     # 32 bias registers in the accumulator layout: the C operand of a half-tile's first MFMAs
V_GT = 208                       # 16 temporaries of the GELU
V_AT = 224                       # 4 accumulator temporaries
V_PK = 228                       # 4 pairs of packed results waiting for their slab write
V_GC = 236                       # 5 polynomial constants of the GELU (236..240)
V_RES = 208                      # fp32: ring of three residual blocks (3 x 16 registers, 208..255)
V_BOFF, V_GOFF = 28, 29          # lane offsets of bias (accumulator layout) / gamma (emit layout)

BUF = 49152
LDS_SLAB = 3 * BUF               # 4 x 4 KiB

EPI_F16, EPI_GELU_F16, EPI_F32 = 0, 1, 2

# slots of one K-tile iteration (index of the MFMA an instruction is emitted behind)
RD23 = [0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7]
BAR_A = 9
DS_WIN = list(range(10, 22))
LGKM0 = 21
BAR_B = 22
RD01 = [23, 23, 24, 24, 25, 25, 26, 27, 28, 29, 30, 31]
ST_WIN = list(range(23, 32))
DMA_SLOTS = [10, 12, 14, 16, 18, 20, 21, 24, 26, 27, 28, 30]


class Op:
    __slots__ = ("kind", "text", "tag")

    def __init__(self, kind, text, tag=None):
        self.kind, self.text, self.tag = kind, text, tag   # kind: valu salu ds st ld wait_vm misc


class GenP(AsmWriter):
    def __init__(self, name, epi, opts=None):
        AsmWriter.__init__(self, name)
        self.epi, self.o = epi, dict(opts or {})

    # ------------------------------------------------------------ DMA side
    def switch_tile(self):
        e = self.e
        done, out = self.u("L_sw_none"), self.u("L_sw_out")
        e("s_mov_b32 s%d, s%d" % (S_TDMA, S_TNEXT))
        e("s_cmp_eq_u32 s%d, -1" % S_TDMA)
        e("s_cbranch_scc1 %s" % done)
        e("s_and_b32 s%d, s%d, 0xffff" % (S_T0, S_TDMA))
        e("s_lshr_b32 s%d, s%d, 16" % (S_T1, S_TDMA))
        e("s_lshl_b32 s%d, s%d, 8" % (S_T0, S_T0))          # row0 = tm * 256
        e("s_lshl_b32 s%d, s%d, 7" % (S_T1, S_T1))          # col0 = tn * 128
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
        const = (p >> 2) * 16384 + (p & 3) * 4096 if p < 8 else 32768 + (p - 8) * 4096
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

    def rotate(self):
        """end of an iteration: DMA target and buffer bookkeeping move one buffer on (S_BUFI = t % 3 of the NEXT iteration)"""
        return ["s_add_u32 s%d, s%d, s%d" % (S_M0BASE, S_M0BASE, S_D23),
                "s_add_u32 s%d, s%d, 1" % (S_BUFI, S_BUFI),
                "s_cmp_eq_u32 s%d, 3" % S_BUFI,
                "s_cselect_b32 s%d, 0, s%d" % (S_BUFI, S_BUFI),
                "s_cmp_eq_u32 s%d, 2" % S_BUFI,
                "s_cselect_b32 s%d, s%d, s%d" % (S_D23, S_BUFM, S_BUFP),
                "s_cmp_eq_u32 s%d, 1" % S_BUFI,
                "s_cselect_b32 s%d, s%d, s%d" % (S_D01, S_BUFM, S_BUFP)]

    # ------------------------------------------------------------ MFMA side
    def frag_read(self, st, ks, idx):
        if idx < 4:
            return "ds_read_b128 v[%d:%d], v%d offset:%d" % (V_SET[st] + 4 * idx, V_SET[st] + 4 * idx + 3, V_FA + ks, idx * 4096)
        j = idx - 4
        return "ds_read_b128 v[%d:%d], v%d offset:%d" % (V_SET[st] + 16 + 4 * j, V_SET[st] + 16 + 4 * j + 3, V_FB + ks, j * 4096)

    def mfma(self, par, s, zero):
        ks, rb, cb = s >> 3, (s & 7) >> 1, s & 1
        blk = par * 128 + (rb * 2 + cb) * 16
        a = "v[%d:%d]" % (V_SET[ks] + 16 + 4 * cb, V_SET[ks] + 16 + 4 * cb + 3)
        b = "v[%d:%d]" % (V_SET[ks] + 4 * rb, V_SET[ks] + 4 * rb + 3)
        cc = "a[%d:%d]" % (blk, blk + 15)     # (the accumulators were initialised with the bias: acc_init)
        return "v_mfma_f32_32x32x16_f16 a[%d:%d], %s, %s, %s" % (blk, blk + 15, a, b, cc)

    def base_slots(self):
        """the k-loop's own side instructions of one iteration: list per slot of Op"""
        slots = [[] for _ in range(32)]
        for i in range(12):
            slots[RD23[i]].append(Op("ds", self.frag_read(2 + i // 6, 2 + i // 6, i % 6)))
        # SRD advance of the previous iteration's pieces (the prologue leaves it to iteration 0)
        for i, ins in enumerate(self.dma_advance()):
            slots[1 + i // 3].append(Op("salu", ins))
        for i, r in enumerate((V_FA + 2, V_FA + 3, V_FB + 2, V_FB + 3)):
            slots[8 + i // 2].append(Op("valu", "v_add_u32 v%d, s%d, v%d" % (r, S_D23, r)))
        slots[BAR_A] += [Op("misc", "s_waitcnt lgkmcnt(0)"), Op("misc", "s_barrier")]
        slots[BAR_A] += [Op("salu", "s_cmp_eq_u32 s%d, 0" % S_DKREM), Op("misc", "SWITCH")]
        for p in range(12):
            s = DMA_SLOTS[p]
            slots[s - 1].append(Op("salu", self.dma_m0(p)))
            slots[s].append(Op("dma", self.dma_issue(p)))
        issued = sum(1 for p in range(12) if DMA_SLOTS[p] <= BAR_B)
        slots[BAR_B] += [Op("misc", "s_waitcnt vmcnt(%d)" % (12 + issued)), Op("misc", "s_barrier")]
        for i in range(12):
            slots[RD01[i]].append(Op("ds", self.frag_read(i // 6, i // 6, i % 6)))
        for i, r in enumerate((V_FA, V_FA + 1, V_FB, V_FB + 1)):
            slots[31].append(Op("valu", "v_add_u32 v%d, s%d, v%d" % (r, S_D01, r)))
        for ins in self.rotate():
            slots[31].append(Op("salu", ins))
        return slots

    def emit_iter(self, par, slots, zero, drain=False):
        """one K-tile iteration: MFMAs of accumulator set `par` + the side instructions of `slots`"""
        e = self.e
        for s in range(32):
            if not drain:
                if s == 0:
                    e("s_waitcnt lgkmcnt(6)")
                if s == 8:
                    e("s_waitcnt lgkmcnt(12)")
                e(self.mfma(par, s, zero))
            for op in slots[s]:
                if drain and op.kind in ("dma",) :
                    continue
                if op.text == "SWITCH":
                    if drain:
                        continue
                    back = self.u("L_swret")
                    e("s_cbranch_scc1 %s" % self.switch_label(back))
                    self.lab(back)
                    continue
                e(op.text)

    def switch_label(self, back):
        lab = self.u("L_switch")
        self.pending_switch.append((lab, back))
        return lab

    # ------------------------------------------------------------ epilogue instruction streams
    def gelu_scalar(self, x, t):
        """x: VGPR holding the pre-activation (overwritten with gelu(x)); t: 3 temporaries. 13 instructions per element:
        gelu(x) = max(x, 0) - |x| h,  h = (1 - |erf(x / sqrt 2)|) / 2 = t (c1 + t (c2 + ...)) exp(-x^2 / 2),  t = 1 / (1 + p |x| / sqrt 2)
        (erf by Abramowitz & Stegun 7.1.26 as common.h gelu_erf; the 1/sqrt(2) and the 1/2 folded into the constants)."""
        d, n, p = t, t + 1, t + 2
        return [
            "v_fma_f32 v%d, |v%d|, s%d, 1.0" % (d, x, S_C),            # 1 + p |x| / sqrt(2)
            "v_mul_f32 v%d, v%d, v%d" % (n, x, x),
            "v_rcp_f32 v%d, v%d" % (d, d),
            "v_mul_f32 v%d, s%d, v%d" % (n, S_C + 1, n),               # -x^2 / 2 * log2(e)
            "v_exp_f32 v%d, v%d" % (n, n),
            "v_fma_f32 v%d, v%d, v%d, v%d" % (p, d, V_GC, V_GC + 1),
            "v_fma_f32 v%d, v%d, v%d, v%d" % (p, p, d, V_GC + 2),
            "v_fma_f32 v%d, v%d, v%d, v%d" % (p, p, d, V_GC + 3),
            "v_fma_f32 v%d, v%d, v%d, v%d" % (p, p, d, V_GC + 4),
            "v_mul_f32 v%d, v%d, v%d" % (p, d, p),
            "v_mul_f32 v%d, v%d, v%d" % (p, p, n),                     # h
            "v_max_f32 v%d, 0, v%d" % (n, x),
            "v_fma_f32 v%d, -|v%d|, v%d, v%d" % (x, x, p, n),
        ]

    def tile_setup_ops(self, which):
        """SALU / VALU that turn the coordinates of a half-tile (S_TPREV for the epilogue proper, S_TCUR for the loads of its
        own operands) into byte offsets"""
        esize = 4 if self.epi == EPI_F32 else 2
        src = S_TPREV if which == "prev" else S_TCUR
        ops = [Op("salu", "s_and_b32 s%d, s%d, 0xffff" % (S_T0, src)), Op("salu", "s_lshr_b32 s%d, s%d, 16" % (S_T1, src)),
               Op("salu", "s_lshl_b32 s%d, s%d, 8" % (S_T0, S_T0)), Op("salu", "s_lshl_b32 s%d, s%d, 7" % (S_T1, S_T1))]
        if which == "prev":
            ops += [Op("salu", "s_mul_i32 s%d, s%d, s%d" % (S_TOFF, S_T0, S_LDO)), Op("salu", "s_add_u32 s%d, s%d, s%d" % (S_TOFF, S_TOFF, S_T1)),
                    Op("salu", "s_lshl_b32 s%d, s%d, %d" % (S_TOFF, S_TOFF, 1 if esize == 2 else 2)),
                    Op("valu", "v_add_u32 v%d, s%d, v%d" % (V_O, S_TOFF, V_OLANE))]
        else:
            ops += [Op("salu", "s_lshl_b32 s%d, s%d, 2" % (S_N0X4, S_T1))]
            if self.epi == EPI_F32:
                ops += [Op("salu", "s_mul_i32 s%d, s%d, s%d" % (S_ROFF, S_T0, S_LDR)), Op("salu", "s_add_u32 s%d, s%d, s%d" % (S_ROFF, S_ROFF, S_T1)),
                        Op("salu", "s_lshl_b32 s%d, s%d, 2" % (S_ROFF, S_ROFF)), Op("valu", "v_add_u32 v%d, s%d, v%d" % (V_R, S_ROFF, V_RLANE))]
        return ops

    def resid_loads(self, b):
        """residual rows of block b = (rb, cb) in the emit layout into ring slot b % 3; leaves V_R at the first row of the next block"""
        rb, cb = b >> 1, b & 1
        base = V_RES + 16 * (b % 3)
        ops = []
        for it in range(4):
            ops.append(Op("ld", "buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d" % (base + 4 * it, base + 4 * it + 3, V_R, SRD_R, SRD_R + 3, cb * 128), ("res", b)))
            if it < 3:
                ops.append(Op("valu", "v_add_u32 v%d, s%d, v%d" % (V_R, S_RROW8, V_R)))
        ops.append(Op("valu", ("v_subrev_u32 v%d, s%d, v%d" % (V_R, S_RROW24, V_R)) if cb == 0 else ("v_add_u32 v%d, s%d, v%d" % (V_R, S_RROW8, V_R))))
        return ops

    def bias_loads(self, src):
        """bias of the half-tile whose table entry is in SGPR `src`, accumulator layout (the C operand of its first MFMAs)"""
        ops = [Op("salu", "s_lshr_b32 s%d, s%d, 16" % (S_T1, src)), Op("salu", "s_lshl_b32 s%d, s%d, 9" % (S_T1, S_T1))]   # col0 * 4
        for cb in range(2):
            for q in range(4):
                r = V_BIAS + (cb * 4 + q) * 4
                ops.append(Op("ld", "buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (r, r + 3, V_BOFF, SRD_BIAS, SRD_BIAS + 3, S_T1, (cb * 32 + 8 * q) * 4), ("bias", 0)))
        return ops

    def acc_init(self, par):
        """accumulator set `par` := bias of the half-tile that will use it next (V_BIAS, accumulator layout)"""
        return [Op("valu", "v_accvgpr_write_b32 a%d, v%d" % (par * 128 + (rb * 2 + cb) * 16 + r, V_BIAS + cb * 16 + r))
                for rb in range(4) for cb in range(2) for r in range(16)]

    def own_loads(self, par):
        """fp32: LayerScale gamma and the first residual block of the half-tile being computed (its epilogue runs under the next one)"""
        if self.epi != EPI_F32:
            return []
        ops = self.tile_setup_ops("cur")
        skip = self.u("L_nogamma")
        grp = ["s_bitcmp1_b32 s%d, 0" % S_FLAGS, "s_cbranch_scc0 %s" % skip]
        for cb in range(2):
            g = V_GAM + 8 * par + 4 * cb
            grp.append("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (g, g + 3, V_GOFF, SRD_GAM, SRD_GAM + 3, S_N0X4, cb * 128))
        grp.append("%s:" % skip)
        ops.append(Op("ld", "\n  ".join(grp), ("gam", 0)))      # (kept together: the branch must not jump over MFMAs)
        ops += self.resid_loads(0)
        return ops

    def schedule_epilogue(self, par_q):
        """the epilogue of accumulator set par_q as per-iteration slot lists (only its own instructions).
        Returns (list of iterations, each a list of 32 lists of Op)."""
        # VALU capacity behind MFMA s of an iteration (docs/history/tools/r04/exp12.sh: independent fillers in the k-loop: 4 per slot behind
        # MFMAs 8..31 cost nothing, 4 behind MFMAs 0..7 - the fragment reads and the descriptor advance - cost 52 cycles);
        # a transcendental counts like any other VALU instruction
        caps = [2] * 8 + [4] * 24
        iters = []

        def slot(it, s):
            while len(iters) <= it:
                iters.append([[] for _ in range(32)])
            return iters[it][s]

        # cursors: (iteration, slot)
        state = {"v": (0, ST_WIN[0]), "vn": 0, "ds": (0, ST_WIN[0]), "st": (0, 0)}

        def place_valu(ops):
            it, s = state["v"]
            for op in ops:
                while state["vn"] + 1 > caps[s]:
                    s += 1
                    state["vn"] = 0
                    if s == 32:
                        it, s = it + 1, 0
                slot(it, s).append(op)
                state["vn"] += 1
            state["v"] = (it, s)

        def next_in(window, pos, strict=False):
            it, s = pos
            if strict:
                s += 1
            while True:
                for w in window:
                    if w >= s:
                        return (it, w)
                it, s = it + 1, 0

        def later(a, b):
            return a if a >= b else b

        # the epilogue starts behind barrier B of iteration 0 (bias went into the accumulators with the first MFMAs)
        for op in self.tile_setup_ops("prev"):
            slot(0, ST_WIN[0]).append(op)
        state["vn"] = 99      # keep that slot for the set-up

        if self.epi != EPI_F32:
            gelu = self.epi == EPI_GELU_F16
            park_pos = {}
            read_pos = {}
            g = 0
            for rb in range(4):
                last_park = None
                for cb in range(2):
                    for q in range(4):
                        if g >= 4 and park_pos[g - 4] > state["v"]:    # the packed pair this group writes must have left for the slab
                            state["v"] = park_pos[g - 4]
                            state["vn"] = 0
                        t, r = V_AT, V_PK + 2 * (g % 4)
                        blk = par_q * 128 + (rb * 2 + cb) * 16 + 4 * q
                        ops = [Op("valu", "v_accvgpr_read_b32 v%d, a%d" % (t + i, blk + i)) for i in range(4)]
                        if gelu:      # the four elements' chains interleaved: a dependent VALU pair issues 1.7x slower than an independent one
                            chains = [self.gelu_scalar(t + i, V_GT + 4 * i) for i in range(4)]
                            for j in range(len(chains[0])):
                                ops += [Op("valu", c[j]) for c in chains]
                        ops += [Op("valu", "v_cvt_pk_f16_f32 v%d, v%d, v%d" % (r, t, t + 1)), Op("valu", "v_cvt_pk_f16_f32 v%d, v%d, v%d" % (r + 1, t + 2, t + 3))]
                        place_valu(ops)
                        pos = next_in(DS_WIN, later(state["ds"], (state["v"][0], state["v"][1] + 1)))
                        slot(*pos).append(Op("ds", "ds_write_b64 v%d, v[%d:%d]" % (V_PARK + cb * 4 + q, r, r + 1)))
                        state["ds"] = pos
                        park_pos[g] = pos
                        last_park = pos
                        g += 1
                em = V_EM[rb & 1]
                pos = next_in(DS_WIN, last_park)
                if pos[1] > LGKM0 - 1:
                    pos = next_in(DS_WIN, (pos[0] + 1, 0))
                for it in range(4):
                    slot(*pos).append(Op("ds", "ds_read_b128 v[%d:%d], v%d offset:%d" % (em + 4 * it, em + 4 * it + 3, V_EADDR + (it & 1), it * 1024)))
                state["ds"] = pos
                spos = later((pos[0], ST_WIN[1]), state["st"])
                assert rb < 2 or spos >= read_pos[rb - 2], "emit registers reused before their stores"
                read_pos[rb] = pos
                for it in range(4):
                    spos = next_in(ST_WIN[1:], spos)
                    slot(*spos).append(Op("st", "buffer_store_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen" % (em + 4 * it, em + 4 * it + 3, V_O, SRD_O, SRD_O + 3)))
                    slot(*spos).append(Op("valu", "v_add_u32 v%d, s%d, v%d" % (V_O, S_ROW8, V_O)))
                    spos = (spos[0], spos[1] + 2)
                state["st"] = spos
        else:
            for b in range(8):
                rb, cb = b >> 1, b & 1
                it_b = b + 2                      # block b: residual rows requested in iteration b (block 0: iteration EL of its own
                em = V_EM[0]                      # half-tile), parked / read back / finished in iteration b + 2
                for q in range(4):
                    blk = par_q * 128 + (rb * 2 + cb) * 16 + 4 * q
                    slot(it_b, DS_WIN[q]).append(Op("ds", "ds_write_b128 v%d, a[%d:%d]" % (V_PARK + q, blk, blk + 3)))
                for it in range(4):
                    slot(it_b, DS_WIN[4 + it]).append(Op("ds", "ds_read_b128 v[%d:%d], v%d offset:%d" % (em + 4 * it, em + 4 * it + 3, V_EADDR + (it & 1), it * 1024)))
                s0 = ST_WIN[0]
                slot(it_b, s0).append(Op("wait_vm", None, ("res", b)))
                gg = V_GAM + 8 * par_q + 4 * cb
                rr = V_RES + 16 * (b % 3)
                for it in range(4):
                    sl = slot(it_b, s0 + it)
                    r = em + 4 * it
                    for i in range(4):
                        sl.append(Op("valu", "v_fma_f32 v%d, v%d, v%d, v%d" % (r + i, r + i, gg + i, rr + 4 * it + i)))
                    sl = slot(it_b, s0 + it + 1)
                    sl.append(Op("st", "buffer_store_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d" % (r, r + 3, V_O, SRD_O, SRD_O + 3, cb * 128)))
                    if it < 3:
                        sl.append(Op("valu", "v_add_u32 v%d, s%d, v%d" % (V_O, S_ROW8, V_O)))
                    else:
                        sl.append(Op("valu", ("v_subrev_u32 v%d, s%d, v%d" % (V_O, S_ROW24, V_O)) if cb == 0 else ("v_add_u32 v%d, s%d, v%d" % (V_O, S_ROW8, V_O))))
                if b >= 1:
                    for k, op in enumerate(self.resid_loads(b)):
                        slot(b, s0 + 5 + k // 3).append(op)
            while len(iters) < 10:
                iters.append([[] for _ in range(32)])
        # iteration 1 requests the NEXT half-tile's bias (the registers are free since the first MFMAs of this one)
        while len(iters) < 2:
            iters.append([[] for _ in range(32)])
        for k, op in enumerate(self.bias_loads(S_TNEXT)):
            iters[1][ST_WIN[0] + min(k // 2, 8)].append(op)
        # the iteration whose DS window carries epilogue traffic ends it with lgkmcnt(0) (no fragment read is in flight there)
        for itl in iters:
            if any(op.kind == "ds" for s in DS_WIN for op in itl[s]):
                itl[LGKM0].append(Op("misc", "s_waitcnt lgkmcnt(0)"))
        return iters

    def merge(self, base, epi):
        out = [[] for _ in range(32)]
        for s in range(32):
            # k-loop instructions first (its counted waits assume that order), except that barrier slots keep the epilogue's
            # pre-barrier instructions (the lgkmcnt(0) of the DS window) in front
            pre = [op for op in epi[s] if s == LGKM0 and op.text and op.text.startswith("s_waitcnt lgkmcnt(0)")]
            rest = [op for op in epi[s] if op not in pre]
            out[s] = pre + list(base[s]) + rest
        return out

    def resolve_waits(self, seq):
        """seq: list of iterations (slot lists) executed back to back. Replaces wait_vm Ops by exact counted s_waitcnt vmcnt(n):
        n = VMEM instructions issued after the awaited group up to the wait."""
        flat = [op for itl in seq for s in range(32) for op in itl[s]]
        issued = []              # the VMEM instructions in issue order: a load's tag, or None for DMA pieces / stores
        for op in flat:
            if op.kind == "wait_vm":
                # (a group that was never requested cannot occur inside a kernel: it is requested in iteration EL)
                op.text = "s_waitcnt vmcnt(%d)" % (younger(issued, op.tag) if op.tag in issued else 0)
            elif op.kind in ("dma", "st", "ld"):
                issued.append(op.tag if op.kind == "ld" else None)

    # ------------------------------------------------------------ whole kernel
    def kernel(self):
        e, n = self.e, self.name
        esize = 4 if self.epi == EPI_F32 else 2
        trace = self.o.get("trace")
        self.pending_switch = []
        self.L += kernel_begin(n)
        e("s_load_dwordx16 s[4:19], s[0:1], 0x0")
        e("s_load_dwordx8 s[20:27], s[0:1], 0x40")
        if trace:
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
        e("v_and_b32 v%d, 31, v%d" % (V_LR, V_LANE))
        e("v_lshrrev_b32 v%d, 5, v%d" % (V_LG, V_LANE))
        e("s_waitcnt lgkmcnt(0)")
        e("s_lshr_b32 s%d, s%d, 1" % (S_WR, S_WV))
        e("s_and_b32 s%d, s%d, 1" % (S_WC, S_WV))
        e("s_lshl_b32 s%d, s%d, 14" % (S_FA, S_WR))                       # A half-tile wr
        e("s_lshl_b32 s%d, s%d, 13" % (S_FB, S_WC))                       # B rows wc * 64
        e("s_add_u32 s%d, s%d, 0x8000" % (S_FB, S_FB))
        e("s_lshl_b32 s%d, s%d, 1" % (S_LDA2, S_LDA))
        e("s_lshl_b32 s%d, s%d, 1" % (S_LDW2, S_LDW))
        e("s_lshr_b32 s%d, s%d, 6" % (S_NK, S_K))
        e("s_lshl_b32 s%d, s%d, 10" % (S_M0BASE, S_WV))
        e("s_lshl_b32 s%d, s%d, 2" % (S_CUR, S_WG))
        e("s_lshl_b32 s%d, s%d, 2" % (S_STRIDE, S_G))
        e("s_load_dword s%d, s[%d:%d], s%d" % (S_TNEXT, S_TAB, S_TAB + 1, S_CUR))
        for srd in (SRD_A, SRD_B, SRD_O, SRD_R, SRD_BIAS, SRD_GAM):
            e("s_mov_b32 s%d, 0x00020000" % (srd + 3))
        e("s_mov_b32 s%d, s%d" % (SRD_O, S_OUT)); e("s_mov_b32 s%d, s%d" % (SRD_O + 1, S_OUT + 1))
        e("s_mul_i32 s%d, s%d, s%d" % (S_ONREC, S_M, S_LDO)); e("s_lshl_b32 s%d, s%d, %d" % (S_ONREC, S_ONREC, 1 if esize == 2 else 2))
        e("s_mov_b32 s%d, 0" % (SRD_O + 2))                                # the first half-tile's (dummy) epilogue stores nothing
        e("s_mov_b32 s%d, s%d" % (SRD_R, S_RES)); e("s_mov_b32 s%d, s%d" % (SRD_R + 1, S_RES + 1))
        e("s_mul_i32 s%d, s%d, s%d" % (SRD_R + 2, S_M, S_LDR)); e("s_lshl_b32 s%d, s%d, 2" % (SRD_R + 2, SRD_R + 2))
        e("s_mov_b32 s%d, s%d" % (SRD_BIAS, S_BIAS)); e("s_mov_b32 s%d, s%d" % (SRD_BIAS + 1, S_BIAS + 1))
        e("s_lshl_b32 s%d, s%d, 2" % (SRD_BIAS + 2, S_N))
        e("s_mov_b32 s%d, s%d" % (SRD_GAM, S_GAM)); e("s_mov_b32 s%d, s%d" % (SRD_GAM + 1, S_GAM + 1))
        e("s_lshl_b32 s%d, s%d, 2" % (SRD_GAM + 2, S_N))
        for ptr, srd in ((S_BIAS, SRD_BIAS), (S_RES, SRD_R), (S_GAM, SRD_GAM)):
            e("s_or_b32 s%d, s%d, s%d" % (S_T0, ptr, ptr + 1))
            e("s_cmp_eq_u32 s%d, 0" % S_T0)
            e("s_cselect_b32 s%d, 0, s%d" % (srd + 2, srd + 2))
        # ---- fragment read addresses (buffer 0)
        e("v_lshrrev_b32 v%d, 1, v%d" % (V_T0, V_LR))
        e("v_and_b32 v%d, 7, v%d" % (V_T0, V_T0))
        e("v_lshlrev_b32 v%d, 7, v%d" % (V_T1, V_LR))
        for ks in range(4):
            e("v_or_b32 v%d, %d, v%d" % (V_T2, 2 * ks, V_LG))
            e("v_xor_b32 v%d, v%d, v%d" % (V_T2, V_T2, V_T0))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_T2, V_T2, V_T1))
            e("v_add_u32 v%d, s%d, v%d" % (V_FA + ks, S_FA, V_T2))
            e("v_add_u32 v%d, s%d, v%d" % (V_FB + ks, S_FB, V_T2))
        # ---- DMA offsets
        e("v_lshrrev_b32 v%d, 3, v%d" % (V_T0, V_LANE))
        e("s_lshl_b32 s%d, s%d, 3" % (S_T0, S_WV))
        e("v_add_u32 v%d, s%d, v%d" % (V_T0, S_T0, V_T0))
        e("v_lshrrev_b32 v%d, 1, v%d" % (V_T1, V_T0))
        e("v_and_b32 v%d, 7, v%d" % (V_T1, V_T1))
        e("v_and_b32 v%d, 7, v%d" % (V_T2, V_LANE))
        e("v_xor_b32 v%d, v%d, v%d" % (V_T1, V_T1, V_T2))
        e("v_lshlrev_b32 v%d, 4, v%d" % (V_T1, V_T1))
        for j in range(8):
            e("v_add_u32 v%d, %d, v%d" % (V_T2, j * 32, V_T0))
            e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T3, V_T2, S_LDA2))
            e("v_add_u32 v%d, v%d, v%d" % (V_DA + j, V_T3, V_T1))
            if j < 4:
                e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T3, V_T2, S_LDW2))
                e("v_add_u32 v%d, v%d, v%d" % (V_DB + j, V_T3, V_T1))
        # ---- epilogue lane constants: slab of 32 rows x 128 bytes, 16-byte chunks swizzled by (row >> 1) & 7
        e("s_lshl_b32 s%d, s%d, 12" % (S_T0, S_WV))
        e("s_add_u32 s%d, s%d, 0x%x" % (S_T0, S_T0, LDS_SLAB))
        e("v_lshrrev_b32 v%d, 1, v%d" % (V_T0, V_LR))
        e("v_and_b32 v%d, 7, v%d" % (V_T0, V_T0))                          # (lr >> 1) & 7
        e("v_lshlrev_b32 v%d, 7, v%d" % (V_T1, V_LR))
        e("v_add_u32 v%d, s%d, v%d" % (V_T1, S_T0, V_T1))                  # slab + lr * 128
        if self.epi == EPI_F32:
            for q in range(4):
                e("v_or_b32 v%d, %d, v%d" % (V_T2, 2 * q, V_LG))
                e("v_xor_b32 v%d, v%d, v%d" % (V_T2, V_T2, V_T0))
                e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_PARK + q, V_T2, V_T1))
        else:
            e("v_lshl_add_u32 v%d, v%d, 3, v%d" % (V_T1, V_LG, V_T1))
            for cq in range(8):
                e("v_xor_b32 v%d, %d, v%d" % (V_T2, cq, V_T0))
                e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_PARK + cq, V_T2, V_T1))
        e("v_lshrrev_b32 v%d, 3, v%d" % (V_T0, V_LANE))                     # lane / 8: row inside an 8-row group
        e("v_and_b32 v%d, 7, v%d" % (V_T1, V_LANE))                         # chunk
        e("v_lshrrev_b32 v%d, 4, v%d" % (V_T2, V_LANE))
        e("v_xor_b32 v%d, v%d, v%d" % (V_T2, V_T2, V_T1))                   # chunk ^ (lane >> 4)   (even groups)
        e("v_lshlrev_b32 v%d, 7, v%d" % (V_T3, V_T0))
        e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T0, V_T3))
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_EADDR, V_T2, V_T3))
        e("v_xor_b32 v%d, 4, v%d" % (V_T2, V_T2))
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_EADDR + 1, V_T2, V_T3))
        # output lane offsets: row wr*128 + lane/8, column wc*64 + (lane & 7) * (16 bytes / esize)
        e("s_lshl_b32 s%d, s%d, 7" % (S_T1, S_WR))
        e("v_add_u32 v%d, s%d, v%d" % (V_T2, S_T1, V_T0))
        e("s_lshl_b32 s%d, s%d, 6" % (S_T2, S_WC))
        cols = 8 if esize == 2 else 4
        e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T3, V_T2, S_LDO))
        e("v_mad_u32_u24 v%d, v%d, %d, v%d" % (V_T3, V_T1, cols, V_T3))
        e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T2, V_T3))
        e("v_lshlrev_b32 v%d, %d, v%d" % (V_OLANE, 1 if esize == 2 else 2, V_T3))
        e("v_mov_b32 v%d, v%d" % (V_O, V_OLANE))
        e("s_lshl_b32 s%d, s%d, %d" % (S_ROW8, S_LDO, 4 if esize == 2 else 5))
        e("s_mul_i32 s%d, s%d, 3" % (S_ROW24, S_ROW8))
        if self.epi == EPI_F32:
            e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T3, V_T2, S_LDR))
            e("v_mad_u32_u24 v%d, v%d, 4, v%d" % (V_T3, V_T1, V_T3))
            e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T2, V_T3))
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_RLANE, V_T3))
            e("v_mov_b32 v%d, v%d" % (V_R, V_RLANE))
            e("s_lshl_b32 s%d, s%d, 5" % (S_RROW8, S_LDR))
            e("s_mul_i32 s%d, s%d, 3" % (S_RROW24, S_RROW8))
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_T3, V_T1))                    # (lane & 7) * 4 columns
            e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T2, V_T3))
            e("v_lshlrev_b32 v%d, 2, v%d" % (V_GOFF, V_T3))
            for i in range(16):
                e("v_mov_b32 v%d, 1.0" % (V_GAM + i))                        # LayerScale absent: ones
        e("v_lshlrev_b32 v%d, 2, v%d" % (V_T3, V_LG))                        # bias, accumulator layout: (wc*64 + 4*lg) * 4 bytes
        e("v_add_u32 v%d, s%d, v%d" % (V_T3, S_T2, V_T3))
        e("v_lshlrev_b32 v%d, 2, v%d" % (V_BOFF, V_T3))
        if self.epi == EPI_GELU_F16:
            for i, cst in enumerate([0x3e6d3388, 0xbf38aa3b, 0x7fffffff]):      # p / sqrt(2) = 0.23164189, -log2(e) / 2, abs mask
                e("s_mov_b32 s%d, 0x%08x" % (S_C + i, cst))
            for i, cst in enumerate([0x3f07dc22, 0xbf3a00e3, 0x3f35f0e3, 0xbe11a98e, 0x3e027906]):     # a5 ... a1 of 7.1.26, halved
                e("v_mov_b32 v%d, 0x%08x" % (V_GC + i, cst))
        # gamma absent: ones (the loads of a zero-sized descriptor would bring zeros) - done once the first loads have landed
        # ---- first half-tile
        e("s_waitcnt lgkmcnt(0)")
        e("s_cmp_eq_u32 s%d, -1" % S_TNEXT)
        e("s_cbranch_scc1 L_exit_%s" % n)
        self.switch_tile()
        e("s_mov_b32 s%d, s%d" % (S_TCUR, S_TDMA))
        e("s_mov_b32 s%d, s%d" % (S_TPREV, S_TDMA))
        for op in self.bias_loads(S_TCUR):       # the first half-tile's bias: ahead of the DMA, so the wait below covers it
            e(op.text)
        for kt in range(3):
            for p in range(12):
                e(self.dma_m0(p))
                e("s_nop 0")
                e(self.dma_issue(p))
            if kt < 2:
                for ins in self.dma_advance():
                    e(ins)
                e("s_add_u32 s%d, s%d, 0x%x" % (S_M0BASE, S_M0BASE, BUF))
        e("s_sub_u32 s%d, s%d, 0x%x" % (S_M0BASE, S_M0BASE, 2 * BUF))
        e("s_mov_b32 s%d, 0" % S_BUFI)
        e("s_mov_b32 s%d, 0x%x" % (S_BUFP, BUF))
        e("s_mov_b32 s%d, 0x%x" % (S_BUFM, (-2 * BUF) & 0xffffffff))
        e("s_mov_b32 s%d, 0x%x" % (S_D23, BUF))
        e("s_mov_b32 s%d, 0x%x" % (S_D01, BUF))
        e("s_waitcnt vmcnt(24)")
        for op in self.acc_init(0):
            e(op.text)
        e("s_barrier")
        for i in range(12):
            e(self.frag_read(i // 6, i // 6, i % 6))
        for r in (V_FA, V_FA + 1, V_FB, V_FB + 1):
            e("v_add_u32 v%d, 0x%x, v%d" % (r, BUF, r))

        base = self.base_slots()
        E = None
        for par in range(2):
            q = 1 - par
            epi_iters = self.schedule_epilogue(q)
            if E is None:
                E = len(epi_iters)
            assert E == len(epi_iters)
            # iteration EL (behind the E epilogue iterations): the next half-tile's accumulators := its bias (requested in
            # iteration 1), this half-tile's own epilogue operands (fp32), output descriptor switched on
            def make_el():
                el = [[] for _ in range(32)]
                el[0].append(Op("wait_vm", None, ("bias", 0)))
                for k, op in enumerate(self.acc_init(q)):
                    el[k // 4].append(op)
                el[ST_WIN[0]].append(Op("salu", "s_mov_b32 s%d, s%d" % (SRD_O + 2, S_ONREC)))
                for k, op in enumerate(self.own_loads(par)):
                    el[ST_WIN[0] + min(k // 3, 8)].append(op)
                return el
            seq = [self.merge(base, make_el())] + [self.merge(base, it) for it in epi_iters] + [self.merge(base, make_el())]
            self.resolve_waits(seq)
            self.lab("L_half_%d_%s" % (par, n))
            if trace:
                e("s_memtime s[%d:%d]" % (S_TS0, S_TS0 + 1))
            for i in range(E):
                self.emit_iter(par, seq[1 + i], zero=False)
            self.emit_iter(par, seq[E + 1], zero=False)
            e("s_sub_u32 s%d, s%d, %d" % (S_KREM, S_NK, E + 1))
            e("s_cmp_le_i32 s%d, 0" % S_KREM)               # (K < 64 (E + 1) is refused by the host; a kernel must not hang on it)
            e("s_cbranch_scc1 L_half_done_%d_%s" % (par, n))
            self.L.append(".p2align 4")
            self.lab("L_loop_%d_%s" % (par, n))
            self.emit_iter(par, base, zero=False)
            e("s_sub_u32 s%d, s%d, 1" % (S_KREM, S_KREM))
            e("s_cmp_eq_u32 s%d, 0" % S_KREM)
            e("s_cbranch_scc0 L_loop_%d_%s" % (par, n))
            self.lab("L_half_done_%d_%s" % (par, n))
            if trace:
                e("s_memtime s[%d:%d]" % (S_TS1, S_TS1 + 1))
                e("s_waitcnt lgkmcnt(0)")
                e("s_sub_u32 s%d, s%d, s%d" % (S_T0, S_TS1, S_TS0))
                e("s_add_u32 s%d, s%d, s%d" % (S_ACC_LOOP, S_ACC_LOOP, S_T0))
                e("s_add_u32 s%d, s%d, s%d" % (S_NKT, S_NKT, S_NK))
            e("s_mov_b32 s%d, s%d" % (S_TPREV, S_TCUR))
            e("s_mov_b32 s%d, s%d" % (S_TCUR, S_TDMA))
            e("s_cmp_eq_u32 s%d, -1" % S_TCUR)
            e("s_cbranch_scc0 L_half_%d_%s" % (1 - par, n))
            # ---- drain: the epilogue of THIS accumulator set, stand-alone (same instruction stream, no MFMAs)
            for itl in self.schedule_epilogue(par):
                for s in range(32):
                    for op in itl[s]:
                        if op.kind == "wait_vm":
                            e("s_waitcnt vmcnt(0)")
                        else:
                            e(op.text)
                    if s == LGKM0:
                        e("s_waitcnt lgkmcnt(0)")
            e("s_branch L_exit_%s" % n)
        self.lab("L_exit_%s" % n)
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")
        if trace:
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
        for lab, back in self.pending_switch:
            self.lab(lab)
            self.switch_tile()
            e("s_branch %s" % back)
        self.E = E
        self.L += kernel_end(n, 163840, 104, NUM_SGPR)

    def metadata(self):
        # the kernarg layout of gemm_asm_gen.py's kernels (no producer fields)
        return kernel_metadata(self.name, ["ptr"] * 7 + ["i32"] * 10 + ["ptr"], 163840, NUM_SGPR)


def variants(trace=False):
    """trace: also the `_v1` forms that count cycles per K-tile loop (gemm_asm_gen.variants)"""
    out = [("psam_gemm_asm2_f16", EPI_F16, {}), ("psam_gemm_asm2_gelu", EPI_GELU_F16, {}), ("psam_gemm_asm2_f32", EPI_F32, {})]
    if trace:
        out += [(name + "_v1", epi, dict(trace=True)) for name, epi, _ in out]
    return out


def build_all(trace=False):
    """-> (assembly lines, metadata entries, {kernel name: E})"""
    lines, meta, es = [], [], {}
    for name, epi, o in variants(trace):
        g = GenP(name, epi, o)
        g.kernel()
        lines += g.L
        meta.append(g.metadata())
        es[name] = g.E
    return lines, meta, es


def main():
    lines, meta, es = build_all("--trace" in sys.argv[1:])
    trailer = ["// %s: E = %d epilogue iterations (needs K >= %d)" % (k, v, 64 * (v + 1)) for k, v in es.items()]
    sys.stdout.write(module_text(lines, meta, trailer))


if __name__ == "__main__":
    main()
