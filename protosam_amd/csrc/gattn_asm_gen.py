#!/usr/bin/env python3
"""Generator of the hand-scheduled gfx950 global attention kernels `psam_gattn_asm_80_rel` / `psam_gattn_asm_64_rel` (SAM ViT-H / ViT-B
global blocks: softmax(q k^T * scale + rel_h + rel_w) v, hd = 80 / 64, 64x64 tokens; models/segment_anything/modeling/image_encoder.py:235-251, 337-372).

Why assembly: the HIP kernel (csrc/attention.hip gattn_kernel) runs at the SUM of its MFMA and VALU issue time (two waves per SIMD
do not overlap the two, and the compiler cannot be steered into interleaving them inside one wave - DESIGN.md). Here ONE wave per
SIMD (4 waves, 512 registers) owns 64 query rows and its instruction stream is built so that every v_mfma_f32_16x16x32_f16 (16
cycles of the matrix pipe = 4 issue slots) is followed by ~3 VALU / LDS instructions of the softmax:

  iteration i (one 64-key tile = one row of the token grid; K / V tile t lives in buffer t % 3 of three):
    open      DMA K(i+3) -> K buffer i % 3, V(i+1) -> V buffer (i+1) % 3 (six pieces per wave, woven into phase 1), rel_h of tile i+1
    phase 1   MFMA: row sums + O^T += V(i-1)^T P(i-1)^T   |  VALU: row max of S(i) (in-lane tree + two lane swaps), + rel_h;
                                                              LDS: rel_w / scale of tile i+1 straight into the idle score set
    decision  lazy rescale of O / l when a row maximum grows by more than 2^8 (out of line)
    phase 2   MFMA: S(i+1)^T = rel_w / scale + K(i+1) Q^T    |  VALU: exp2(scale log2e S - offset), fp16 packing of P(i)
    close     s_waitcnt vmcnt(6) (everything but this iteration's own six pieces has landed); s_barrier; rotate the buffer offsets

Data layouts are attention.hip's: the K / V tiles arrive by LDS-DMA as [64 rows][80] fp16 images (K rows in MFMA-row order, V rows
in the order the transposing reads want), the scores are computed transposed (a lane owns one query column: 16 keys x 4 registers
per 16-key tile), P is the B operand of the second product as it stands, rel_w (times log2 e) is staged once per workgroup in LDS,
rel_h is one scalar per query and tile.

Three forms of the kernel (round 5), one generator:
  rel    psam_gattn_asm_{80,64}_rel     rel_h / rel_w fp32 [B,H,N,64] from HBM (psam_relpos wrote them): the round-3 / 4 kernel
  fused  psam_gattn_asm_{80,64}_fused   the decomposed rel-pos terms (image_encoder.py:325-372) are computed HERE from the packed
                                        tables (ops.pack_rel_tables): no psam_relpos launch, no 2 x B H N 64 fp32 round trip.
           rel_w[q][kx] = q . Rw[qx - kx + 63]: once per workgroup, 120 MFMAs per wave (table rows as the A operand in hi / lo
             halves against the wave's query fragments) scattered along the diagonals into the LDS stage the tile loop reads;
           rel_h[q][ky] = q . Rh[qy - ky + 63]: a wave's 64 queries are ONE row qy of the token map, so a key tile (= key row ky)
             needs ONE table row for all of them: 4 x KS MFMAs per tile whose A operand holds that row (hi in the even MFMA rows,
             lo in the odd ones; three 16-byte loads per lane and tile, one tile ahead) - a lane ends up with hi.q and lo.q of
             its query, one add.
  norel  psam_gattn_asm_64_norel        no bias (DINOv2: models/grid_proto_fewshot.py:88-98 -> the hub model's Attention), ANY token
                                        count: the last key tile is masked (-inf into the score registers of keys >= N before its
                                        softmax), an odd tile count takes a second tail, rows beyond N of the last query block load
                                        zeros and store nothing (buffer range checks).
All three take their (b, h, query block) from a host-built work table (attention.hip gattn_worklist): equal shares per XCD.

Run through gemm_asm_gen.py (same code object).
"""

LOG2E = 1.4426950408889634
HD, RLD = 80, 160                 # head dim, bytes per LDS row
IMG = 64 * RLD                    # 10 240 bytes per K / V image
K_BASE, V_BASE, RW_BASE = 0, 3 * IMG, 6 * IMG      # three K images, three V images (tile t in buffer t % 3), the rel_w stage
LDS_BYTES = RW_BASE + 256 * 256   # + rel_w stage: 256 queries x 64 floats

# ---- SGPRs
S_QKV, S_OUT, S_RH, S_RWP = 4, 6, 8, 10
S_N, S_H, S_LGNQB, S_LGH, S_SL2, S_RS2, S_HS2, S_WS2, S_NT, S_OROW, S_RWMUL = 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22   # kernarg ints / floats
SRD_K, SRD_V, SRD_RH, SRD_Q, SRD_O = 24, 28, 32, 36, 40
S_WV, S_B, S_HH, S_QBLK, S_T0, S_T1, S_T2, S_T3 = 44, 45, 46, 47, 48, 49, 50, 51
S_KSTEP, S_M0K, S_M0V, S_LOOP, S_RHT = 52, 53, 54, 55, 56      # 64 * rs2; M0 bases of this wave's first DMA piece; loop counter; tile * 4
S_QT = 57                                                        # s57..59: qt * 4096 (rel_h rows) for qt = 1..3
S_OQT = 60                                                       # s60..62: qt * 16 * out row bytes
S_CMP = 64                                                       # s[64:65], s[66:67]: compare masks
S_8 = 68
S_DMAEX = 66                                                    # s[66:67]: EXEC of this wave's third DMA piece (all lanes: waves 0 / 1, none: waves 2 / 3)
S_R0, S_R1, S_R2 = 69, 70, 71                                   # byte offsets of the buffers (i % 3, (i + 1) % 3, (i + 2) % 3) in iteration i
S_M0K0, S_M0V0 = 72, 73                                         # this wave's first DMA piece inside K / V buffer 0
S_NQB8, S_NVALID, S_TAB = 76, 77, 78                            # kernarg tail: (spare); valid keys of the last tile (1..64); s[78:79] work table
NUM_SGPR = 80
JUNK_BASE = LDS_BYTES                                           # fused: where the off-diagonal lanes of the rel_w scatter write
LDS_BYTES_FUSED = LDS_BYTES + 3 * 4096 + 1024

# ---- VGPRs
V_TID = 0
V_KRD = 1            # v1..3: K fragment read address per k-step
V_VRD = 4
V_RW = 5             # v5..8: rel_w read address per key tile tt
V_DK, V_DV = 9, 12   # v9..11 / v12..14: DMA offsets of this wave's pieces
V_QO, V_OO, V_RHO = 15, 16, 17
V_T = 18             # v18..31 temporaries
V_S = [32, 96]       # score sets: [tt][qt][r] = base + (tt * 4 + qt) * 4 + r
V_P = 160            # P fragments: [qt][s2] 4 registers each
V_KA = 192           # v192..194: K fragment read addresses inside the buffer this iteration reads, v195: the same for V
V_VA = 195
V_RHF = 196          # fused: v196..207 the table-row fragments of the next tile's rel_h (KS x 4)
V_RHA = 208          # fused: v208..223 [qt] 4 each: hi . q (register 0) and lo . q (register 1) of the next tile's rel_h
V_NINF = 196         # norel: -inf
V_MXT = 25           # v25..31: temporaries of the max trees / swaps
V_MRUN, V_MX, V_BH, V_BHN, V_MOFF = 232, 236, 240, 244, 248
V_LI, V_G = 252, 253
# ---- AGPRs
A_O, A_LT, A_Q, A_ONES = 0, 80, 96, 144      # O^T [d][qt] 4 each; l [qt] 4; Q fragments [qt][s] 4; ones
A_KF, A_VF, RING = 148, 172, 6               # rings of six K / V fragments (LDS reads land in AGPRs, the MFMAs take them from there)


from asm_common import AsmWriter, LdsCounter, kernel_begin, kernel_end, kernel_metadata, module_text

PER2 = 3             # side instructions per MFMA in phase 2 (4: no change)
# The running maximum only has to keep exp2(score - offset) inside fp16 / fp32 range, not to be the exact row maximum: every lane
# compares its OWN 16 scores of a query against the running offset + 8, and only when some lane trips does the out-of-line rescale
# reduce the maxima across the four lanes that share the query (two lane swaps per query tile). The common iteration then carries
# no cross-lane traffic at all: 32 instructions fewer per tile and wave than with the swaps in every iteration, 3727 -> 3650 cycles.
# (Tried with it: K pieces 8 / 9 to waves 0 / 1 and V pieces 8 / 9 to waves 2 / 3, five real DMA pieces per wave instead of six /
# four - no change, 3760 vs 3745 cycles: the barrier's cost is not the waves' DMA imbalance.)
# Also measured and dropped: the exp2 / packing of one or two of a tile's four 16-key blocks deferred to phase 1 of the next
# iteration. Phase 2 carries 160 softmax instructions on 48-60 MFMAs, phase 1 some 50 on 48, and the P V MFMAs of the tile's second key
# half (the only readers of block 3's probabilities) run in the second half of that phase 1 - by a per-phase max(VALU, MFMA) model worth
# 300 of 3700 cycles. 16-slice ViT-H layer, fused / rel: none 1962-1971 / 1905-1916 us, block 3 1973-1988 / 1882-1889, blocks 2 and 3
# 1963-1974 / 1870-1872, block 2 1970-1998 / 1875-1902 - nothing beyond the run-to-run spread: the loop is not bound by the balance of
# its phases but by the instruction issue of its one wave per SIMD ("What comes next").


class GenA(AsmWriter):
    def __init__(self, name="psam_gattn_asm_80_rel", hd=HD, mode="rel"):
        """mode: "rel" / "fused" / "norel" (module docstring). hd = 80 (SAM ViT-H) or 64 (SAM ViT-B / MedSAM): the LDS images keep their 160-byte rows for both (a 128-byte row would put
        every second MFMA row on the same banks); with hd = 64 the lanes of the two spare 16-byte chunks of a row fetch beyond the
        buffer (zeros, no traffic), the scores take two k-steps instead of three and O^T four 16-row blocks instead of five."""
        AsmWriter.__init__(self, name)
        assert hd in (64, 80) and mode in ("rel", "fused", "norel")
        self.hd, self.mode = hd, mode
        self.HDP2 = (hd + 31) // 32 * 32 * 2   # bytes per row of the packed rel-pos tables (ops.pack_rel_tables: [2][2][128][HDP] fp16)
        self.KS = (hd + 31) // 32          # k-steps of a score MFMA chain
        self.DB = hd // 16                 # 16-row blocks of O^T

    def ltag(self, tag):
        return "%s_%d_%s" % (tag, self.hd, self.mode)

    # ------------------------------------------------------------------ interleaver
    def merge(self, pre, mfmas, fillers, per=3):
        """pre: ops emitted first; mfmas: list of (text, [keys of the LDS reads it needs], [ops pinned right behind it]);
        fillers: ordered ops spread `per` behind every MFMA (the rest after the last). An op is ("ds", text, key) - an LDS read -,
        ("v", text, [keys]) - needs those reads - or ("s", text). LDS operations return in order: the lgkmcnt waits are counted."""
        e = self.e
        issued = {}
        lds = LdsCounter(e)

        def need(keys):
            if keys:
                lds.need(max(issued[k] for k in keys))

        def emit(op):
            if op[0] == "ds":
                issued[op[2]] = lds.issue(op[1])
            elif op[0] == "v":
                need(op[2])
                e(op[1])
            else:
                e(op[1])

        for op in pre:
            emit(op)
        fi = 0
        for (txt, deps, pinned) in mfmas:
            need(deps)
            e(txt)
            for op in pinned:
                emit(op)
            for _ in range(per):
                if fi < len(fillers):
                    emit(fillers[fi])
                    fi += 1
        while fi < len(fillers):
            emit(fillers[fi])
            fi += 1
        e("s_waitcnt lgkmcnt(0)")

    # ------------------------------------------------------------------ pieces
    def s_idx(self, st, tt, qt):
        return V_S[st] + (tt * 4 + qt) * 4

    def v_read(self, k, vbuf):
        """the k-th V fragment (s2 = k / 5, d = k % 5) into ring slot k % 3: two transposing reads"""
        s2, d = k // self.DB, k % self.DB
        r = A_VF + 4 * (k % RING)
        base = V_BASE + s2 * 5120 + d * 32
        return [("ds", "ds_read_b64_tr_b16 a[%d:%d], v%d offset:%d" % (r, r + 1, V_VA, base), ("vfa", k)),
                ("ds", "ds_read_b64_tr_b16 a[%d:%d], v%d offset:%d" % (r + 2, r + 3, V_VA, base + 8 * RLD), ("vf", k))]

    def k_read(self, k, kbuf):
        """the k-th K fragment (tt = k / 3, k-step k % 3) into ring slot k % 3"""
        tt, s = k // self.KS, k % self.KS
        r = A_KF + 4 * (k % RING)
        return [("ds", "ds_read_b128 a[%d:%d], v%d offset:%d" % (r, r + 3, V_KA + s, K_BASE + tt * 16 * RLD), ("kf", k))]

    def pv_mfmas(self, vbuf):
        """row sums and O^T += V^T P^T of the tile whose P sits in V_P; fragment k is read right behind the last MFMA of fragment
        k - 2 (its ring slot was fragment k - 3's), the first two up front"""
        AH = RING - 2          # fragments in flight ahead of the one being consumed
        pre = []
        for k in range(AH):
            pre += self.v_read(k, vbuf)
        M = []
        for s2 in range(2):
            for qt in range(4):
                p = V_P + (qt * 2 + s2) * 4
                M.append(["v_mfma_f32_16x16x32_f16 a[%d:%d], a[%d:%d], v[%d:%d], a[%d:%d]" % (
                    A_LT + 4 * qt, A_LT + 4 * qt + 3, A_ONES, A_ONES + 3, p, p + 3, A_LT + 4 * qt, A_LT + 4 * qt + 3), [], []])
            for d in range(self.DB):
                k = s2 * self.DB + d
                r = A_VF + 4 * (k % RING)
                for qt in range(4):
                    p = V_P + (qt * 2 + s2) * 4
                    o = A_O + (d * 4 + qt) * 4
                    M.append(["v_mfma_f32_16x16x32_f16 a[%d:%d], a[%d:%d], v[%d:%d], a[%d:%d]" % (o, o + 3, r, r + 3, p, p + 3, o, o + 3),
                              [("vf", k)] if qt == 0 else [], []])
                if k + AH < 2 * self.DB:
                    M[-1][2] += self.v_read(k + AH, vbuf)
        return pre, [tuple(m) for m in M]

    def qk_mfmas(self, nst, kbuf):
        """S^T = K Q^T of the next tile into score set `nst`"""
        AH = RING - 2
        pre = []
        for k in range(AH):
            pre += self.k_read(k, kbuf)
        M = []
        for k in range(4 * self.KS):
            tt, s = k // self.KS, k % self.KS
            r = A_KF + 4 * (k % RING)
            for qt in range(4):
                d0 = self.s_idx(nst, tt, qt)       # (holds rel_w / scale of this block: the scores accumulate on top of it)
                q = A_Q + (qt * 3 + s) * 4
                cin = "0" if (self.mode == "norel" and s == 0) else "v[%d:%d]" % (d0, d0 + 3)      # (no bias: start from zero)
                M.append(["v_mfma_f32_16x16x32_f16 v[%d:%d], a[%d:%d], a[%d:%d], %s" % (d0, d0 + 3, r, r + 3, q, q + 3, cin),
                          [("kf", k)] if qt == 0 else [], []])
            if k + AH < 4 * self.KS:
                M[-1][2] += self.k_read(k + AH, kbuf)
        return pre, [tuple(m) for m in M]

    def rw_reads(self, nst):
        """rel_w / scale of the NEXT tile's 16 blocks straight into the idle score set: the accumulator input of its score MFMAs"""
        F = []
        for tt in range(4):
            for qt in range(4):
                d0 = self.s_idx(nst, tt, qt)
                F.append(("ds", "ds_read_b128 v[%d:%d], v%d offset:%d" % (d0, d0 + 3, V_RW + tt, qt * 4096), ("rw", tt * 4 + qt)))
        return F

    def soft1(self, st):
        """the row maxima of score set `st` (raw scores + rel_w / scale; times scale log2 e, + rel_h): the VALU stream of phase 1"""
        F = []
        # in-lane maxima of the 16 values of every query tile (two independent v_max3 chains each), then scale / rel_h (the maxima
        # across the lanes that share a query: rescale_routine, only when a lane trips)
        t = [V_MXT + i for i in range(4)]
        for qt in range(4):
            vals = [self.s_idx(st, tt, qt) + j for tt in range(4) for j in range(4)]
            m = V_MX + qt
            F.append(("v", "v_max3_f32 v%d, v%d, v%d, v%d" % (m, vals[0], vals[1], vals[2]), []))
            for i in range(4):
                F.append(("v", "v_max3_f32 v%d, v%d, v%d, v%d" % (t[i], vals[3 + 3 * i], vals[4 + 3 * i], vals[5 + 3 * i]), []))
            F.append(("v", "v_max3_f32 v%d, v%d, v%d, v%d" % (m, m, t[0], t[1]), []))
            F.append(("v", "v_max3_f32 v%d, v%d, v%d, v%d" % (t[2], t[2], t[3], vals[15]), []))
            F.append(("v", "v_max_f32 v%d, v%d, v%d" % (m, m, t[2]), []))
        for qt in range(4):
            F.append(("v", "v_fma_f32 v%d, v%d, s%d, v%d" % (V_MX + qt, V_MX + qt, S_SL2, V_BH + qt), []))   # * scale log2(e) + rel_h of this row of keys
        return F

    def soft2(self, st):
        """exp2 and fp16 packing of the four key blocks of score set `st` into P: the VALU stream of phase 2"""
        F = []
        for tt in range(4):
            for qt in range(4):
                s0 = self.s_idx(st, tt, qt)
                for j in range(4):
                    F.append(("v", "v_fma_f32 v%d, v%d, s%d, -v%d" % (s0 + j, s0 + j, S_SL2, V_MOFF + qt), []))
                for j in range(4):
                    F.append(("v", "v_exp_f32 v%d, v%d" % (s0 + j, s0 + j), []))
                p = V_P + (qt * 2 + (tt >> 1)) * 4 + (tt & 1) * 2
                F.append(("v", "v_cvt_pk_f16_f32 v%d, v%d, v%d" % (p, s0, s0 + 1), []))
                F.append(("v", "v_cvt_pk_f16_f32 v%d, v%d, v%d" % (p + 1, s0 + 2, s0 + 3), []))
        return F

    def decision(self, tag):
        """rows whose maximum grew by more than 2^8 over the running one: rescale (out of line); then the exp offsets"""
        e = self.e
        for qt in range(4):
            e("v_add_f32 v%d, s%d, v%d" % (V_T + qt, S_8, V_MRUN + qt))
        e("v_cmp_gt_f32 vcc, v%d, v%d" % (V_MX, V_T))
        e("s_mov_b64 s[%d:%d], vcc" % (S_CMP, S_CMP + 1))
        for qt in range(1, 4):
            e("v_cmp_gt_f32 vcc, v%d, v%d" % (V_MX + qt, V_T + qt))
            e("s_or_b64 s[%d:%d], s[%d:%d], vcc" % (S_CMP, S_CMP + 1, S_CMP, S_CMP + 1))
        e("s_cmp_lg_u64 s[%d:%d], 0" % (S_CMP, S_CMP + 1))
        tag = self.ltag(tag)
        e("s_cbranch_scc1 L_resc_%s" % tag)
        self.lab("L_resc_ret_%s" % tag)
        for qt in range(4):
            e("v_sub_f32 v%d, v%d, v%d" % (V_MOFF + qt, V_MRUN + qt, V_BH + qt))

    def rescale_routine(self, tag):
        e = self.e
        tag = self.ltag(tag)
        self.lab("L_resc_%s" % tag)
        e("s_nop 7")
        e("s_nop 7")
        # the lanes' own maxima -> the maxima of the query rows (the four lanes li, li + 16, li + 32, li + 48 share a query)
        xs = [V_T + i for i in range(4)]          # v18..21 / v22..24 + v29: free outside the decision / rescale code
        ys = [V_T + 4, V_T + 5, V_T + 6, V_MXT + 4]
        for swap in ("v_permlane16_swap_b32", "v_permlane32_swap_b32"):
            for qt in range(4):
                e("v_mov_b32 v%d, v%d" % (xs[qt], V_MX + qt))
                e("v_mov_b32 v%d, v%d" % (ys[qt], V_MX + qt))
            e("s_nop 1")
            for qt in range(4):
                e("%s v%d, v%d" % (swap, xs[qt], ys[qt]))
            e("s_nop 1")
            for qt in range(4):
                e("v_max_f32 v%d, v%d, v%d" % (V_MX + qt, xs[qt], ys[qt]))
        for qt in range(4):
            e("v_max_f32 v%d, v%d, v%d" % (V_T + 4, V_MRUN + qt, V_MX + qt))
            e("v_sub_f32 v%d, v%d, v%d" % (V_T + 5, V_MRUN + qt, V_T + 4))
            e("v_mov_b32 v%d, v%d" % (V_MRUN + qt, V_T + 4))
            e("v_exp_f32 v%d, v%d" % (V_T + 5, V_T + 5))
            regs = [A_LT + 4 * qt + j for j in range(4)] + [A_O + (d * 4 + qt) * 4 + j for d in range(self.DB) for j in range(4)]
            for r in regs:
                e("v_accvgpr_read_b32 v%d, a%d" % (V_T + 6, r))
                e("s_nop 0")
                e("v_mul_f32 v%d, v%d, v%d" % (V_T + 6, V_T + 6, V_T + 5))
                e("s_nop 0")
                e("v_accvgpr_write_b32 a%d, v%d" % (r, V_T + 6))
        e("s_nop 3")
        e("s_branch L_resc_ret_%s" % tag)

    # ------------------------------------------------------------------ fused: rel_h of the next tile
    def rh_mfmas(self, frags=None):
        """rel_h of the NEXT tile for the wave's 64 queries: A = the tile's table row (hi in the even MFMA rows, lo in the odd ones:
        V_RHF, loaded an iteration ago), B = the query fragments. Lane (li, g) gets rows 4 g + j of column li: register 0 = hi . q,
        register 1 = lo . q of query qt * 16 + li (rh_finish adds them). k-steps outermost: dependent MFMAs are four apart."""
        M = []
        frags = frags or [V_RHF + 4 * s_ for s_ in range(self.KS)]
        for s_ in range(self.KS):
            for qt in range(4):
                d0 = V_RHA + 4 * qt
                q = A_Q + (qt * 3 + s_) * 4
                cin = "0" if s_ == 0 else "v[%d:%d]" % (d0, d0 + 3)
                M.append(("v_mfma_f32_16x16x32_f16 v[%d:%d], v[%d:%d], a[%d:%d], %s" % (d0, d0 + 3, frags[s_], frags[s_] + 3, q, q + 3, cin), [], []))
        return M

    def rh_loads(self):
        """the table row of the tile after next into V_RHF (issued behind the MFMAs that read the current contents, and BEFORE this
        iteration's DMA pieces: loads return in order, and the closing vmcnt(6) leaves only the six pieces in flight). Row r = qy -
        tile + 63, one row down per tile, clamped at row 0 beyond the last tile (values unused)."""
        ops = [("s", "s_sub_i32 s%d, s%d, %d" % (S_RHT, S_RHT, self.HDP2)), ("s", "s_max_i32 s%d, s%d, 0" % (S_RHT, S_RHT))]
        for s_ in range(self.KS):
            ops.append(("s", "buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (
                V_RHF + 4 * s_, V_RHF + 4 * s_ + 3, V_RHO, SRD_RH, SRD_RH + 3, S_RHT, s_ * 64)))
        return ops

    def rh_finish(self):
        e = self.e
        for qt in range(4):
            e("v_add_f32 v%d, v%d, v%d" % (V_BH + qt, V_RHA + 4 * qt, V_RHA + 4 * qt + 1))
        for qt in range(4):
            e("v_mul_f32 v%d, 0x%08x, v%d" % (V_BH + qt, 0x3fb8aa3b, V_BH + qt))     # * log2(e)

    def fused_prologue(self):
        """rel_w / scale of the wave's 64 queries against the 64 key columns into its rows of the LDS stage, rel_h of tile 0 into V_BH,
        the table row of tile 1 into V_RHF. Runs once per workgroup, with the first K / V images in flight.
        rel_w[q][kx] = q . Rw[qx - kx + 63] (image_encoder.py:355-372): query tile qt (qx = 16 qt + li) meets table rows 16 qt ...
        16 qt + 78 = the five 16-row blocks rb = qt ... qt + 4. Per (qt, rb): 2 KS MFMAs (hi, lo halves of the block as the A operand,
        the query fragments as B) leave rows r = 16 rb + 4 g + j of query 16 qt + li in lane (li, g), register j: key column
        kx = 16 (qt - rb) + li - 4 g + 63 - j, written to the stage if 0 <= kx < 64 (else to a junk area: no EXEC games). Groups of
        four pairs: the scatter of a group runs behind the MFMAs of the next (accumulators in spare AGPRs)."""
        e, KS, HDP2 = self.e, self.KS, self.HDP2
        F0 = V_S[0]                                 # fragments [rb][ks][hl] 4 registers each: v32 ... (hd = 80: 48 x 4 = v32..v223)
        A_ACC = 196                                 # eight accumulator sets a196..a227
        v_rwoff, v_kb, v_rowb, v_junk = V_T, V_T + 1, V_T + 2, V_T + 3
        TW = 2 * 128 * HDP2
        e("v_mul_u32_u24 v%d, %d, v%d" % (v_rwoff, HDP2, V_LI))
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (v_rwoff, V_G, v_rwoff))            # li * row + g * 16
        e("v_lshlrev_b32 v%d, 2, v%d" % (v_kb, V_G))
        e("v_sub_u32 v%d, v%d, v%d" % (v_kb, V_LI, v_kb))
        e("v_add_u32 v%d, 63, v%d" % (v_kb, v_kb))                                 # li - 4 g + 63
        e("s_lshl_b32 s%d, s%d, 14" % (S_T1, S_WV))
        e("s_add_u32 s%d, s%d, 0x%x" % (S_T1, S_T1, RW_BASE))
        e("v_lshlrev_b32 v%d, 8, v%d" % (v_rowb, V_LI))
        e("v_add_u32 v%d, s%d, v%d" % (v_rowb, S_T1, v_rowb))                      # RW_BASE + (wv * 64 + li) * 256
        e("v_and_b32 v%d, 63, v0" % v_junk)
        e("v_lshlrev_b32 v%d, 2, v%d" % (v_junk, v_junk))
        e("v_add_u32 v%d, 0x%x, v%d" % (v_junk, JUNK_BASE, v_junk))
        nf = 0
        for rb in range(8):
            for ks in range(KS):
                for hl in range(2):
                    e("s_mov_b32 s%d, %d" % (S_T0, TW + hl * 128 * HDP2 + rb * 16 * HDP2))
                    r = F0 + 4 * nf
                    e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (r, r + 3, v_rwoff, SRD_RH, SRD_RH + 3, S_T0, ks * 64))
                    nf += 1
        # rel_h: the table row of tile 0 (r = qy + 63, qy = qblk * 4 + wv) behind them
        e("s_lshl_b32 s%d, s%d, 2" % (S_RHT, S_QBLK))
        e("s_add_u32 s%d, s%d, s%d" % (S_RHT, S_RHT, S_WV))
        e("s_add_u32 s%d, s%d, 63" % (S_RHT, S_RHT))
        e("s_mul_i32 s%d, s%d, %d" % (S_RHT, S_RHT, HDP2))
        PRO = [224, 228, 244]      # (V_RHF / V_RHA lie inside the hd = 80 fragment range v32..v223: tile 0's row goes elsewhere)
        for s_ in range(KS):
            e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (
                PRO[s_], PRO[s_] + 3, V_RHO, SRD_RH, SRD_RH + 3, S_RHT, s_ * 64))
        e("s_waitcnt vmcnt(0)")
        pairs = [(qt, rb) for rb in range(8) for qt in range(4) if qt <= rb <= qt + 4]
        groups = [pairs[i:i + 4] for i in range(0, len(pairs), 4)]

        def mfmas(gi):
            out = []
            for step in range(2 * KS):
                ks, hl = step >> 1, step & 1
                for pi, (qt, rb) in enumerate(groups[gi]):
                    acc = A_ACC + 4 * ((gi & 1) * 4 + pi)
                    fr = F0 + 4 * ((rb * KS + ks) * 2 + hl)
                    q = A_Q + (qt * 3 + ks) * 4
                    cin = "0" if step == 0 else "a[%d:%d]" % (acc, acc + 3)
                    out.append("v_mfma_f32_16x16x32_f16 a[%d:%d], v[%d:%d], a[%d:%d], %s" % (acc, acc + 3, fr, fr + 3, q, q + 3, cin))
            return out

        def scatter(gi):
            out = []
            for pi, (qt, rb) in enumerate(groups[gi]):
                acc = A_ACC + 4 * ((gi & 1) * 4 + pi)
                for j in range(4):
                    t, c, t3, val = (V_T + 4, V_T + 5, V_T + 6, V_T + 7) if (j & 1) == 0 else (V_T + 8, V_T + 9, V_T + 10, V_T + 11)
                    out += ["v_add_u32 v%d, %d, v%d" % (t, 16 * (qt - rb) - j, v_kb),
                            "v_cmp_gt_u32 vcc, 64, v%d" % t,
                            "v_lshrrev_b32 v%d, 2, v%d" % (c, t),
                            "v_xor_b32 v%d, v%d, v%d" % (c, c, V_LI),
                            "v_and_b32 v%d, 3, v%d" % (t3, t),
                            "v_lshlrev_b32 v%d, 4, v%d" % (c, c),
                            "v_lshl_add_u32 v%d, v%d, 2, v%d" % (c, t3, c),
                            "v_add_u32 v%d, v%d, v%d" % (c, v_rowb, c),
                            "v_cndmask_b32 v%d, v%d, v%d, vcc" % (c, v_junk, c),
                            "v_accvgpr_read_b32 v%d, a%d" % (val, acc + j),
                            "v_mul_f32 v%d, s%d, v%d" % (val, S_RWMUL, val),
                            "ds_write_b32 v%d, v%d offset:%d" % (c, val, qt * 4096)]
            return out
        for m in mfmas(0):
            e(m)
        for gi in range(1, len(groups)):
            M, F = mfmas(gi), scatter(gi - 1)
            per = -(-len(F) // (len(M) - 2))
            fi = 0
            for mi, m in enumerate(M):
                e(m)
                if mi == 1:
                    e("s_nop 7")       # (the previous group's last MFMA is now 2 MFMAs + 8 states old: its accumulators may be read)
                if mi >= 1:
                    for _ in range(per):
                        if fi < len(F):
                            e(F[fi])
                            fi += 1
            while fi < len(F):
                e(F[fi])
                fi += 1
        # rel_h of tile 0 from V_RHF while the last group's accumulators settle, then its scatter
        for (txt, _, _) in self.rh_mfmas(PRO):
            e(txt)
        e("s_nop 7")
        for op in scatter(len(groups) - 1):
            e(op)
        e("s_nop 7")
        e("s_nop 7")
        self.rh_finish()
        for op in self.rh_loads():          # the table row of tile 1
            e(op[1])

    def mask_last_tile(self, st, tag):
        """norel: keys >= N of the LAST tile (score set `st`) -> -inf. Register (tt, j) of lane group g holds key (tt >> 1) * 32 +
        g * 8 + (tt & 1) * 4 + j of the tile (the MFMA-row order of the K image)."""
        e = self.e
        lab = "L_nomask_%s" % self.ltag(tag)
        e("s_cmp_ge_u32 s%d, 64" % S_NVALID)
        e("s_cbranch_scc1 %s" % lab)
        e("v_lshlrev_b32 v%d, 3, v%d" % (V_T, V_G))
        for tt in range(4):
            for j in range(4):
                c = (tt >> 1) * 32 + (tt & 1) * 4 + j
                e("s_sub_i32 s%d, s%d, %d" % (S_T0, S_NVALID, c))            # masked when g * 8 >= nvalid - c
                e("v_cmp_le_i32 vcc, s%d, v%d" % (S_T0, V_T))
                for qt in range(4):
                    r = self.s_idx(st, tt, qt) + j
                    e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (r, r, V_NINF))
        self.lab(lab)

    def dma_ops(self):
        """this wave's pieces of the next K image and the next V image as filler operations (descriptors advance by one tile each).
        The third piece exists for waves 0 / 1 only: issued under an empty EXEC mask elsewhere, so that every wave has the same
        number of memory operations in flight."""
        ops = []
        for which, (srd, m0, vo) in enumerate(((SRD_K, S_M0K, V_DK), (SRD_V, S_M0V, V_DV))):
            for i in range(3):
                ops.append(("s", "s_add_u32 m0, s%d, %d" % (m0, i * 4096)))
                if i == 2:
                    ops.append(("s", "s_mov_b64 exec, s[%d:%d]" % (S_DMAEX, S_DMAEX + 1)))
                ops.append(("s", "buffer_load_dwordx4 v%d, s[%d:%d], 0 offen lds" % (vo + i, srd, srd + 3)))
                if i == 2:
                    ops.append(("s", "s_mov_b64 exec, -1"))
            ops.append(("s", "s_add_u32 s%d, s%d, s%d" % (srd, srd, S_KSTEP)))
            ops.append(("s", "s_addc_u32 s%d, s%d, 0" % (srd + 1, srd + 1)))
            ops.append(("s", "s_max_u32 s%d, s%d, s%d" % (srd + 2, srd + 2, S_KSTEP)))
            ops.append(("s", "s_sub_u32 s%d, s%d, s%d" % (srd + 2, srd + 2, S_KSTEP)))
        return ops

    def dma(self):
        for op in self.dma_ops():
            self.e(op[1])

    def buffers(self):
        """iteration i: DMA targets K buffer i % 3 / V buffer (i + 1) % 3; the scores read K buffer (i + 1) % 3, P V reads V buffer (i + 2) % 3"""
        e = self.e
        e("s_add_u32 s%d, s%d, s%d" % (S_M0K, S_M0K0, S_R0))
        e("s_add_u32 s%d, s%d, s%d" % (S_M0V, S_M0V0, S_R1))
        for s_ in range(3):
            e("v_add_u32 v%d, s%d, v%d" % (V_KA + s_, S_R1, V_KRD + s_))
        e("v_add_u32 v%d, s%d, v%d" % (V_VA, S_R2, V_VRD))

    def bh_loads(self):
        """rel_h of the NEXT tile for this lane's four query rows"""
        e = self.e
        e("s_add_u32 s%d, s%d, 4" % (S_RHT, S_RHT))
        e("buffer_load_dword v%d, v%d, s[%d:%d], s%d offen" % (V_BHN, V_RHO, SRD_RH, SRD_RH + 3, S_RHT))
        for qt in range(1, 4):
            e("s_add_u32 s%d, s%d, s%d" % (S_T0, S_RHT, S_QT + qt - 1))
            e("buffer_load_dword v%d, v%d, s[%d:%d], s%d offen" % (V_BHN + qt, V_RHO, SRD_RH, SRD_RH + 3, S_T0))

    def iteration(self, par, has_pv, has_qk, tag):
        """tile i with i & 1 == par: scores in set `par`, P V of tile i-1 from V buffer (i-1) & 1 = par ^ 1, scores of tile i+1 from
        K buffer par ^ 1 into set par ^ 1. The DMA of K(i+2) / V(i) goes into the buffers the previous iteration's barrier released."""
        e = self.e
        self.buffers()
        if self.mode == "rel":
            self.bh_loads()
        if self.mode == "norel" and not has_qk:
            self.mask_last_tile(par, tag)
        F = self.soft1(par)
        if has_qk and self.mode != "norel":   # rel_w / scale of the next tile: one read per five other operations (needed in phase 2 only)
            rw = self.rw_reads(par ^ 1)
            out, k = [], 0
            for i, op in enumerate(F):
                if i % 5 == 0 and k < len(rw):
                    out.append(rw[k])
                    k += 1
                out.append(op)
            F = out + rw[k:]
        # the six DMA pieces of an iteration: woven into phase 1 behind its first MFMAs (no-bias kernel), or issued back to back in the
        # MFMA-free stretch between the phases (rel-pos kernels: 1951 -> 1909 us per 16-slice ViT-H call, 1227 -> 1195 ViT-B; the no-bias
        # kernel runs 4 % slower that way: its phase 1 has no rel_w reads to share the slots with)
        dma_late = self.mode != "norel"
        if not dma_late:
            F = self.dma_ops() + F
        pre, M = self.pv_mfmas(par ^ 1) if has_pv else ([], [])
        self.merge(pre, M, F, 3)
        if dma_late:
            self.dma()
        self.decision(tag)
        pre, M = self.qk_mfmas(par ^ 1, par ^ 1) if has_qk else ([], [])
        rh = self.mode == "fused" and has_qk
        if rh:
            # rel_h of tile i + 1 BEHIND the score MFMAs of phase 2 - the phase that carries 160 softmax instructions on 48 MFMAs gets
            # twelve more to hide them behind (ahead of the P V MFMAs of phase 1, the first form: 4600 cycles per tile against 3690 of
            # the _rel kernel in the back-to-back benchmark). Its table row was requested an iteration ago, behind the six DMA pieces of
            # that iteration: everything but this iteration's own six pieces has landed at vmcnt(6); the row of tile i + 2 is requested
            # behind the last of these MFMAs (they have read the old one), so the closing wait leaves 6 + KS requests in flight.
            RM = self.rh_mfmas()
            M[-1] = (M[-1][0], M[-1][1], list(M[-1][2]) + [("s", "s_waitcnt vmcnt(6)")])
            RM[-1] = (RM[-1][0], [], self.rh_loads())
            M = M + RM
        F = self.soft2(par)
        self.merge(pre, M, F, max(PER2, -(-len(F) // max(len(M), 1))))      # (hd = 64: 32 score MFMAs carry the same 160 instructions)
        # K(i+2), V(i) (requested an iteration ago) and rel_h of the next tile have landed; the six pieces this iteration
        # requested (every wave issues six, see dma_ops) may stay in flight
        e("s_waitcnt vmcnt(%d)" % (6 + (self.KS if rh else 0)))
        e("s_mov_b32 s%d, s%d" % (S_T0, S_R0))
        e("s_mov_b32 s%d, s%d" % (S_R0, S_R1))
        e("s_mov_b32 s%d, s%d" % (S_R1, S_R2))
        e("s_mov_b32 s%d, s%d" % (S_R2, S_T0))
        if self.mode == "rel":
            for qt in range(4):
                e("v_mul_f32 v%d, 0x%08x, v%d" % (V_BH + qt, 0x3fb8aa3b, V_BHN + qt))     # * log2(e)
        elif rh:
            e("s_nop 7")          # (the last rel_h MFMA is ~15 instructions old: its accumulator read below stays clear of the XDL write hazard)
            self.rh_finish()
        e("s_barrier")

    # ------------------------------------------------------------------ kernel
    def kernel(self):
        e, n = self.e, self.name
        self.L += kernel_begin(n)
        e("s_load_dwordx8 s[4:11], s[0:1], 0x0")
        e("s_load_dwordx8 s[12:19], s[0:1], 0x20")
        e("s_load_dwordx4 s[20:23], s[0:1], 0x40")
        e("s_load_dwordx4 s[%d:%d], s[0:1], 0x50" % (S_NQB8, S_NQB8 + 3))
        e("v_and_b32 v%d, 63, v0" % (V_T))                        # lane
        e("v_lshrrev_b32 v%d, 6, v0" % (V_T + 1))
        e("s_nop 1")
        e("v_readfirstlane_b32 s%d, v%d" % (S_WV, V_T + 1))
        e("v_and_b32 v%d, 15, v%d" % (V_LI, V_T))
        e("v_lshrrev_b32 v%d, 4, v%d" % (V_G, V_T))
        e("s_waitcnt lgkmcnt(0)")
        # ---- workgroup -> (b, h, query block): as attention.hip (the eight XCDs work on eight (b, h) pairs, all their query blocks)
        # (round 5: a host-built table, entry wg = (b * H + h) << 10 | query block, -1 = none. Workgroup wg runs on XCD wg % 8: the table
        # gives every XCD the same number of items, a contiguous run of the (b, h)-major item list - its workgroups that run side by
        # side share K / V in the XCD's L2 -, whatever B * H is: twelve heads of one 5330-token image are 252 items = ONE round of the
        # 256 CUs (the arithmetic map of round 4 gave four XCDs two (b, h) pairs and four one: two rounds, 190 instead of ~100 us))
        # (tried in round 4: the two (b, h) groups an XCD runs side by side as ADJACENT heads, whose 160-byte rows share 128-byte lines:
        # FETCH_SIZE 705 -> 595 MB raw per 16-slice call, time unchanged (1686 vs 1684 us) - the kernel is not fetch-bound)
        e("s_lshl_b32 s%d, s2, 2" % S_T0)
        e("s_load_dword s%d, s[%d:%d], s%d" % (S_T1, S_TAB, S_TAB + 1, S_T0))
        e("s_waitcnt lgkmcnt(0)")
        e("s_cmp_lt_i32 s%d, 0" % S_T1)
        e("s_cbranch_scc1 L_nowork_%s" % n)
        e("s_and_b32 s%d, s%d, 0x3ff" % (S_QBLK, S_T1))
        e("s_lshr_b32 s%d, s%d, 10" % (S_T1, S_T1))               # grp = b * H + h
        # b = grp / H, h = grp % H: the host passes ceil(2^16 / H) (exact for grp < 2^16 / H ... H = 12 and 16 alike)
        e("s_mul_i32 s%d, s%d, s%d" % (S_B, S_T1, S_LGH))
        e("s_lshr_b32 s%d, s%d, 16" % (S_B, S_B))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T3, S_B, S_H))
        e("s_sub_u32 s%d, s%d, s%d" % (S_HH, S_T1, S_T3))
        # ---- descriptors
        # q / k / v of (b, h): qkv + b * N * rs2 + h * hs2 (+ ws2, 2 ws2)
        e("s_mul_i32 s%d, s%d, s%d" % (S_T0, S_N, S_RS2))                       # bytes per image
        e("s_mul_hi_u32 s%d, s%d, s%d" % (S_T3, S_B, S_T0))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T2, S_B, S_T0))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T1, S_HH, S_HS2))
        e("s_add_u32 s%d, s%d, s%d" % (S_T2, S_T2, S_T1))
        e("s_addc_u32 s%d, s%d, 0" % (S_T3, S_T3))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_Q, S_QKV, S_T2))
        e("s_addc_u32 s%d, s%d, s%d" % (SRD_Q + 1, S_QKV + 1, S_T3))
        e("s_mov_b32 s%d, s%d" % (SRD_Q + 2, S_T0))
        e("s_mov_b32 s%d, 0x00020000" % (SRD_Q + 3))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_K, SRD_Q, S_WS2))
        e("s_addc_u32 s%d, s%d, 0" % (SRD_K + 1, SRD_Q + 1))
        e("s_mov_b32 s%d, s%d" % (SRD_K + 2, S_T0))
        e("s_mov_b32 s%d, 0x00020000" % (SRD_K + 3))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_V, SRD_K, S_WS2))
        e("s_addc_u32 s%d, s%d, 0" % (SRD_V + 1, SRD_K + 1))
        e("s_mov_b32 s%d, s%d" % (SRD_V + 2, S_T0))
        e("s_mov_b32 s%d, 0x00020000" % (SRD_V + 3))
        e("s_lshl_b32 s%d, s%d, 6" % (S_KSTEP, S_RS2))
        if self.mode == "rel":
            # rel_h / rel_w rows of (b, h): ((b * H + h) * N) * 256 bytes
            e("s_mul_i32 s%d, s%d, s%d" % (S_T1, S_B, S_H))
            e("s_add_u32 s%d, s%d, s%d" % (S_T1, S_T1, S_HH))
            e("s_mul_i32 s%d, s%d, s%d" % (S_T1, S_T1, S_N))
            e("s_lshr_b32 s%d, s%d, 24" % (S_T3, S_T1))
            e("s_lshl_b32 s%d, s%d, 8" % (S_T2, S_T1))
            e("s_add_u32 s%d, s%d, s%d" % (SRD_RH, S_RH, S_T2))
            e("s_addc_u32 s%d, s%d, s%d" % (SRD_RH + 1, S_RH + 1, S_T3))
            e("s_lshl_b32 s%d, s%d, 8" % (SRD_RH + 2, S_N))
            e("s_mov_b32 s%d, 0x00020000" % (SRD_RH + 3))
            # rel_w rows of this query block (staging source): + qblk * 65536; the descriptor lives in the output's registers for now
            e("s_lshl_b32 s%d, s%d, 16" % (S_T0, S_QBLK))
            e("s_add_u32 s%d, s%d, s%d" % (S_T2, S_T2, S_T0))
            e("s_addc_u32 s%d, s%d, 0" % (S_T3, S_T3))
            e("s_add_u32 s%d, s%d, s%d" % (SRD_O, S_RWP, S_T2))
            e("s_addc_u32 s%d, s%d, s%d" % (SRD_O + 1, S_RWP + 1, S_T3))
            e("s_mov_b32 s%d, 0x10000" % (SRD_O + 2))
            e("s_mov_b32 s%d, 0x00020000" % (SRD_O + 3))
            # ---- stage rel_w * log2(e): 256 queries x 64 floats, 16 x 16 bytes per thread; chunk slot ^ (row & 15)
            e("v_lshlrev_b32 v%d, 4, v0" % (V_T + 2))                   # source: tid * 16
            e("v_lshrrev_b32 v%d, 4, v0" % (V_T + 3))                   # tid >> 4 = row (mod 16 per pass)
            e("v_and_b32 v%d, 15, v0" % (V_T + 4))
            e("v_and_b32 v%d, 15, v%d" % (V_T + 5, V_T + 3))
            e("v_xor_b32 v%d, v%d, v%d" % (V_T + 4, V_T + 4, V_T + 5))
            e("v_lshlrev_b32 v%d, 4, v%d" % (V_T + 4, V_T + 4))
            e("v_lshl_add_u32 v%d, v%d, 8, v%d" % (V_T + 4, V_T + 3, V_T + 4))
            e("v_add_u32 v%d, 0x%x, v%d" % (V_T + 4, RW_BASE, V_T + 4))
            e("s_mov_b32 s%d, 0" % S_T0)
            for it in range(16):
                e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], s%d offen" % (V_S[0] + 4 * it, V_S[0] + 4 * it + 3, V_T + 2, SRD_O, SRD_O + 3, S_T0))
                e("s_add_u32 s%d, s%d, 4096" % (S_T0, S_T0))
            for it in range(16):
                e("s_waitcnt vmcnt(%d)" % (15 - it))
                for j in range(4):
                    e("v_mul_f32 v%d, s%d, v%d" % (V_S[0] + 4 * it + j, S_RWMUL, V_S[0] + 4 * it + j))
                e("ds_write_b128 v%d, v[%d:%d] offset:%d" % (V_T + 4, V_S[0] + 4 * it, V_S[0] + 4 * it + 3, it * 4096))
        elif self.mode == "fused":
            # the packed tables [2 (h, w)][2 (hi, lo)][128][HDP] fp16 (ops.pack_rel_tables) behind one descriptor
            e("s_mov_b32 s%d, s%d" % (SRD_RH, S_RH))
            e("s_mov_b32 s%d, s%d" % (SRD_RH + 1, S_RH + 1))
            e("s_mov_b32 s%d, %d" % (SRD_RH + 2, 4 * 128 * self.HDP2))
            e("s_mov_b32 s%d, 0x00020000" % (SRD_RH + 3))
        # ---- output descriptor: out + b * N * orow
        e("s_mul_i32 s%d, s%d, s%d" % (S_T0, S_N, S_OROW))
        e("s_mul_hi_u32 s%d, s%d, s%d" % (S_T3, S_B, S_T0))
        e("s_mul_i32 s%d, s%d, s%d" % (S_T2, S_B, S_T0))
        e("s_add_u32 s%d, s%d, s%d" % (SRD_O, S_OUT, S_T2))
        e("s_addc_u32 s%d, s%d, s%d" % (SRD_O + 1, S_OUT + 1, S_T3))
        e("s_mov_b32 s%d, s%d" % (SRD_O + 2, S_T0))
        e("s_mov_b32 s%d, 0x00020000" % (SRD_O + 3))
        # ---- lane constants
        # first query row of this wave: qblk * 256 + wv * 64; this lane's row (qt = 0): + li
        e("s_lshl_b32 s%d, s%d, 8" % (S_T0, S_QBLK))
        e("s_lshl_b32 s%d, s%d, 6" % (S_T1, S_WV))
        e("s_add_u32 s%d, s%d, s%d" % (S_T0, S_T0, S_T1))
        e("v_add_u32 v%d, s%d, v%d" % (V_T + 6, S_T0, V_LI))          # q row
        e("v_mul_lo_u32 v%d, v%d, s%d" % (V_QO, V_T + 6, S_RS2))
        e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_QO, V_G, V_QO))      # + g * 8 halfs
        e("v_mul_lo_u32 v%d, v%d, s%d" % (V_OO, V_T + 6, S_OROW))
        e("s_mul_i32 s%d, s%d, %d" % (S_T1, S_HH, self.hd * 2))
        e("v_add_u32 v%d, s%d, v%d" % (V_OO, S_T1, V_OO))
        e("v_lshl_add_u32 v%d, v%d, 3, v%d" % (V_OO, V_G, V_OO))      # + g * 4 halfs
        if self.mode == "rel":
            e("v_lshlrev_b32 v%d, 8, v%d" % (V_RHO, V_T + 6))             # rel_h row: q * 256 bytes
        elif self.mode == "fused":                                      # table row fragment: (li & 1) * [lo half] + g * 16 bytes
            e("v_and_b32 v%d, 1, v%d" % (V_T + 7, V_LI))
            e("v_mul_u32_u24 v%d, %d, v%d" % (V_T + 7, 128 * self.HDP2, V_T + 7))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_RHO, V_G, V_T + 7))
        e("s_mov_b32 s%d, 4096" % S_QT); e("s_mov_b32 s%d, 8192" % (S_QT + 1)); e("s_mov_b32 s%d, 12288" % (S_QT + 2))
        e("s_lshl_b32 s%d, s%d, 4" % (S_OQT, S_OROW)); e("s_lshl_b32 s%d, s%d, 5" % (S_OQT + 1, S_OROW)); e("s_mul_i32 s%d, s%d, 48" % (S_OQT + 2, S_OROW))
        e("s_mov_b32 s%d, 0x41000000" % S_8)                            # 8.0
        # K fragment read addresses: li * 160 + kc * 16, kc = s * 4 + g (k-step 2: min(8 + g, 9))
        e("v_mul_u32_u24 v%d, %d, v%d" % (V_T + 7, RLD, V_LI))
        for s in range(3):
            if s < 2:
                e("v_add_u32 v%d, %d, v%d" % (V_T + 8, 4 * s, V_G))
            else:
                e("v_add_u32 v%d, 8, v%d" % (V_T + 8, V_G))
                e("v_min_u32 v%d, 9, v%d" % (V_T + 8, V_T + 8))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_KRD + s, V_T + 8, V_T + 7))
        # V fragment read address: vrow = (g >> 1) * 16 + (g & 1) * 4 + (li >> 2); + (li & 3) * 8 bytes
        e("v_lshrrev_b32 v%d, 1, v%d" % (V_T + 8, V_G))
        e("v_lshlrev_b32 v%d, 4, v%d" % (V_T + 8, V_T + 8))
        e("v_and_b32 v%d, 1, v%d" % (V_T + 9, V_G))
        e("v_lshl_add_u32 v%d, v%d, 2, v%d" % (V_T + 8, V_T + 9, V_T + 8))
        e("v_lshrrev_b32 v%d, 2, v%d" % (V_T + 9, V_LI))
        e("v_add_u32 v%d, v%d, v%d" % (V_T + 8, V_T + 8, V_T + 9))
        e("v_mul_u32_u24 v%d, %d, v%d" % (V_T + 8, RLD, V_T + 8))
        e("v_and_b32 v%d, 3, v%d" % (V_T + 9, V_LI))
        e("v_lshl_add_u32 v%d, v%d, 3, v%d" % (V_VRD, V_T + 9, V_T + 8))
        # rel_w read addresses: RW_BASE + (wv * 64 + li) * 256 + ((c4 ^ li) << 4), c4 = (tt >> 1) * 8 + g * 2 + (tt & 1)
        e("s_lshl_b32 s%d, s%d, 14" % (S_T1, S_WV))
        e("s_add_u32 s%d, s%d, 0x%x" % (S_T1, S_T1, RW_BASE))
        e("v_lshlrev_b32 v%d, 8, v%d" % (V_T + 8, V_LI))
        e("v_add_u32 v%d, s%d, v%d" % (V_T + 8, S_T1, V_T + 8))
        for tt in range(4):
            e("v_lshl_add_u32 v%d, v%d, 1, %d" % (V_T + 9, V_G, (tt >> 1) * 8 + (tt & 1)))
            e("v_xor_b32 v%d, v%d, v%d" % (V_T + 9, V_T + 9, V_LI))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_RW + tt, V_T + 9, V_T + 8))
        # DMA offsets: piece p = wv + 4 i: S = p * 64 + lane, R = S / 10, c = S % 10; key offsets inside the tile as attention.hip
        e("v_and_b32 v%d, 63, v0" % (V_T + 8))
        for i in range(3):
            e("s_lshl_b32 s%d, s%d, 6" % (S_T1, S_WV))
            e("s_add_u32 s%d, s%d, %d" % (S_T1, S_T1, i * 256))
            e("v_add_u32 v%d, s%d, v%d" % (V_T + 9, S_T1, V_T + 8))               # S
            e("s_mov_b32 s%d, 0xcccccccd" % S_T2)
            e("v_mul_hi_u32 v%d, s%d, v%d" % (V_T + 10, S_T2, V_T + 9))
            e("v_lshrrev_b32 v%d, 3, v%d" % (V_T + 10, V_T + 10))                  # R = S / 10
            e("v_mul_u32_u24 v%d, 10, v%d" % (V_T + 11, V_T + 10))
            e("v_sub_u32 v%d, v%d, v%d" % (V_T + 11, V_T + 9, V_T + 11))          # c
            if self.hd == 64:      # chunks 8 / 9 of a 160-byte LDS row do not exist in a 128-byte head slice: out of range -> zeros
                e("v_cmp_lt_u32 vcc, 7, v%d" % (V_T + 11))
                e("v_mov_b32 v%d, 0x04000000" % (V_T + 14))
                e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (V_T + 11, V_T + 11, V_T + 14))      # chunk 2^26: 2^30 bytes away
            e("v_and_b32 v%d, 31, v%d" % (V_T + 12, V_T + 10))                     # rho
            e("v_lshrrev_b32 v%d, 5, v%d" % (V_T + 13, V_T + 10))                  # C
            # K: C * 32 + ((rho >> 2) & 3) * 8 + (rho >> 4) * 4 + (rho & 3)
            e("v_bfe_u32 v%d, v%d, 2, 2" % (V_T + 9, V_T + 12))
            e("v_lshlrev_b32 v%d, 3, v%d" % (V_T + 9, V_T + 9))
            e("v_lshrrev_b32 v%d, 4, v%d" % (V_T + 10, V_T + 12))
            e("v_lshl_add_u32 v%d, v%d, 2, v%d" % (V_T + 9, V_T + 10, V_T + 9))
            e("v_and_b32 v%d, 3, v%d" % (V_T + 10, V_T + 12))
            e("v_add_u32 v%d, v%d, v%d" % (V_T + 9, V_T + 9, V_T + 10))
            e("v_lshl_add_u32 v%d, v%d, 5, v%d" % (V_T + 9, V_T + 13, V_T + 9))
            e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T + 9, V_T + 9, S_RS2))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_DK + i, V_T + 11, V_T + 9))
            # V: C * 32 + ((rho >> 4) * 2 + ((rho >> 2) & 1)) * 8 + ((rho >> 3) & 1) * 4 + (rho & 3)
            e("v_lshrrev_b32 v%d, 4, v%d" % (V_T + 9, V_T + 12))
            e("v_bfe_u32 v%d, v%d, 2, 1" % (V_T + 10, V_T + 12))
            e("v_lshl_add_u32 v%d, v%d, 1, v%d" % (V_T + 9, V_T + 9, V_T + 10))
            e("v_lshlrev_b32 v%d, 3, v%d" % (V_T + 9, V_T + 9))
            e("v_bfe_u32 v%d, v%d, 3, 1" % (V_T + 10, V_T + 12))
            e("v_lshl_add_u32 v%d, v%d, 2, v%d" % (V_T + 9, V_T + 10, V_T + 9))
            e("v_and_b32 v%d, 3, v%d" % (V_T + 10, V_T + 12))
            e("v_add_u32 v%d, v%d, v%d" % (V_T + 9, V_T + 9, V_T + 10))
            e("v_lshl_add_u32 v%d, v%d, 5, v%d" % (V_T + 9, V_T + 13, V_T + 9))
            e("v_mul_lo_u32 v%d, v%d, s%d" % (V_T + 9, V_T + 9, S_RS2))
            e("v_lshl_add_u32 v%d, v%d, 4, v%d" % (V_DV + i, V_T + 11, V_T + 9))
        e("s_lshl_b32 s%d, s%d, 10" % (S_M0K0, S_WV))
        e("s_add_u32 s%d, s%d, 0x%x" % (S_M0V0, S_M0K0, V_BASE))
        e("s_mov_b32 s%d, 0" % S_R0); e("s_mov_b32 s%d, %d" % (S_R1, IMG)); e("s_mov_b32 s%d, %d" % (S_R2, 2 * IMG))
        e("s_cmp_lt_u32 s%d, 2" % S_WV)
        e("s_cselect_b32 s%d, -1, 0" % S_DMAEX)
        e("s_mov_b32 s%d, s%d" % (S_DMAEX + 1, S_DMAEX))
        # ---- query fragments: [qt][s] 8 halfs at row qt * 16 + li, column s * 32 + g * 8 (k-step 2: lanes g >= 2 hold zeros)
        e("s_lshl_b32 s%d, s%d, 4" % (S_T1, S_RS2))                    # 16 rows
        e("v_mov_b32 v%d, v%d" % (V_T + 8, V_QO))
        e("v_cmp_gt_u32 vcc, 2, v%d" % V_G)
        e("v_mov_b32 v%d, 0x40000000" % (V_T + 10))
        for qt in range(4):
            for s in range(self.KS):
                r = V_S[0] + (qt * 3 + s) * 4
                if s < 2:
                    e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d" % (r, r + 3, V_T + 8, SRD_Q, SRD_Q + 3, s * 64))
                else:
                    e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (V_T + 9, V_T + 10, V_T + 8))
                    e("buffer_load_dwordx4 v[%d:%d], v%d, s[%d:%d], 0 offen offset:128" % (r, r + 3, V_T + 9, SRD_Q, SRD_Q + 3))
            e("v_add_u32 v%d, s%d, v%d" % (V_T + 8, S_T1, V_T + 8))
        e("s_waitcnt vmcnt(0)")
        for i in range(48):
            e("v_accvgpr_write_b32 a%d, v%d" % (A_Q + i, V_S[0] + i))
        e("v_mov_b32 v%d, 0x3c003c00" % (V_T + 9))
        for i in range(4):
            e("v_accvgpr_write_b32 a%d, v%d" % (A_ONES + i, V_T + 9))
        for i in range(96):
            e("v_accvgpr_write_b32 a%d, 0" % (A_O + i))
        for qt in range(4):
            e("v_mov_b32 v%d, 0xff800000" % (V_MRUN + qt))
        # ---- K(0), K(1), K(2) into the three K buffers, V(0) into V buffer 0 (in flight under what follows)
        ops_all = self.dma_ops()
        kops, vops = ops_all[:len(ops_all) // 2], ops_all[len(ops_all) // 2:]
        for which in range(3):
            e("s_add_u32 s%d, s%d, %d" % (S_M0K, S_M0K0, which * IMG))
            for op in kops:
                e(op[1])
        e("s_mov_b32 s%d, s%d" % (S_M0V, S_M0V0))
        for op in vops:
            e(op[1])
        if self.mode == "rel":
            # ---- rel_h of tile 0
            e("s_mov_b32 s%d, 0" % S_RHT)
            e("buffer_load_dword v%d, v%d, s[%d:%d], 0 offen" % (V_BHN, V_RHO, SRD_RH, SRD_RH + 3))
            for qt in range(1, 4):
                e("buffer_load_dword v%d, v%d, s[%d:%d], s%d offen" % (V_BHN + qt, V_RHO, SRD_RH, SRD_RH + 3, S_QT + qt - 1))
            e("s_waitcnt vmcnt(0)")
            for qt in range(4):
                e("v_mul_f32 v%d, 0x3fb8aa3b, v%d" % (V_BH + qt, V_BHN + qt))
        elif self.mode == "fused":
            self.fused_prologue()
        else:
            for qt in range(4):
                e("v_mov_b32 v%d, 0" % (V_BH + qt))
            e("v_mov_b32 v%d, 0xff800000" % V_NINF)
        for s_ in range(3):
            e("v_mov_b32 v%d, v%d" % (V_KA + s_, V_KRD + s_))
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")
        e("s_barrier")
        # scores of tile 0 into set 0 (nothing to overlap with): rel_w / scale first, the products on top
        if self.mode != "norel":
            for op in self.rw_reads(0):
                e(op[1])
            e("s_waitcnt lgkmcnt(0)")
        pre, M = self.qk_mfmas(0, 0)
        self.merge(pre, M, [], 0)
        e("s_nop 7")
        e("s_barrier")
        # (iteration 0 opens with K(2) -> K buffer 0, V(0) -> V buffer 0)
        # ---- the tile loop: first | (odd, even) x L | tail, L = (NT - 2) / 2. Even NT: the tail is the last tile (parity 1); odd NT
        # (norel only: 1297 tokens are 21 tiles): one more full iteration, then the last tile with parity 0.
        e("s_sub_u32 s%d, s%d, 2" % (S_LOOP, S_NT))
        e("s_lshr_b32 s%d, s%d, 1" % (S_LOOP, S_LOOP))
        self.iteration(0, False, True, "first")
        e("s_cmp_eq_u32 s%d, 0" % S_LOOP)
        e("s_cbranch_scc1 L_tail_%s" % n)
        self.lab("L_loop_%s" % n)
        self.iteration(1, True, True, "odd")
        self.iteration(0, True, True, "even")
        e("s_sub_u32 s%d, s%d, 1" % (S_LOOP, S_LOOP))
        e("s_cmp_eq_u32 s%d, 0" % S_LOOP)
        e("s_cbranch_scc0 L_loop_%s" % n)
        self.lab("L_tail_%s" % n)
        tails = [("last", [(1, True, False, "last")])]
        if self.mode == "norel":
            e("s_bitcmp1_b32 s%d, 0" % S_NT)
            e("s_cbranch_scc1 L_oddtail_%s" % n)
            tails.append(("oddtail", [(1, True, True, "odd2"), (0, True, False, "last0")]))
        for ti, (tname, its) in enumerate(tails):
            if ti:
                self.lab("L_oddtail_%s" % n)
            for (par, has_pv, has_qk, tag) in its:
                self.iteration(par, has_pv, has_qk, tag)
            # ---- P V of the last tile (the rotation has moved on: its V buffer is "(i + 2) % 3" of the iteration that does not exist)
            e("v_add_u32 v%d, s%d, v%d" % (V_VA, S_R2, V_VRD))
            pre, M = self.pv_mfmas(1)
            self.merge(pre, M, [], 0)
            if len(tails) > 1 and ti == 0:
                e("s_branch L_store_%s" % n)
        self.lab("L_store_%s" % n)
        e("s_nop 7")
        e("s_nop 7")
        # ---- O / l -> fp16, 8-byte stores: out[q][h * 80 + d * 16 + g * 4 .. + 3]
        for qt in range(4):
            e("v_accvgpr_read_b32 v%d, a%d" % (V_T + 8, A_LT + 4 * qt))
            e("s_nop 1")
            e("v_rcp_f32 v%d, v%d" % (V_T + 8, V_T + 8))
            for d in range(self.DB):
                o = A_O + (d * 4 + qt) * 4
                for j in range(4):
                    e("v_accvgpr_read_b32 v%d, a%d" % (V_T + 9 + j, o + j))
                e("s_nop 1")
                for j in range(4):
                    e("v_mul_f32 v%d, v%d, v%d" % (V_T + 9 + j, V_T + 9 + j, V_T + 8))
                e("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (V_T + 6, V_T + 9, V_T + 10))
                e("v_cvt_pk_f16_f32 v%d, v%d, v%d" % (V_T + 7, V_T + 11, V_T + 12))
                if qt == 0:
                    e("buffer_store_dwordx2 v[%d:%d], v%d, s[%d:%d], 0 offen offset:%d" % (V_T + 6, V_T + 7, V_OO, SRD_O, SRD_O + 3, d * 32))
                else:
                    e("buffer_store_dwordx2 v[%d:%d], v%d, s[%d:%d], s%d offen offset:%d" % (V_T + 6, V_T + 7, V_OO, SRD_O, SRD_O + 3, S_OQT + qt - 1, d * 32))
        e("s_waitcnt vmcnt(0)")
        self.lab("L_nowork_%s" % n)
        e("s_endpgm")
        for tag in ("first", "odd", "even", "last") + (("odd2", "last0") if self.mode == "norel" else ()):
            self.rescale_routine(tag)
        self.L += kernel_end(n, self.lds_bytes(), 96, NUM_SGPR)

    def lds_bytes(self):
        return LDS_BYTES_FUSED if self.mode == "fused" else LDS_BYTES

    def metadata(self):
        # kernarg: qkv, out, rel_h, rel_w; N, H, log2(query blocks), ceil(2^16 / H), scale * log2 e, ... , B * H (last); row / head / which strides, tiles, out row, rel_w factor
        # (+ spare, valid keys of the last tile, the work table)
        return kernel_metadata(self.name, ["ptr"] * 4 + ["i32"] * 14 + ["ptr"], self.lds_bytes(), NUM_SGPR)


def build_all():
    lines, meta = [], []
    for name, hd, mode in (("psam_gattn_asm_80_rel", 80, "rel"), ("psam_gattn_asm_64_rel", 64, "rel"),
                           ("psam_gattn_asm_80_fused", 80, "fused"), ("psam_gattn_asm_64_fused", 64, "fused"),
                           ("psam_gattn_asm_64_norel", 64, "norel")):
        g = GenA(name, hd, mode)
        g.kernel()
        lines += g.L
        meta.append(g.metadata())
    return lines, meta


if __name__ == "__main__":
    import sys
    sys.stdout.write(module_text(*build_all()))
