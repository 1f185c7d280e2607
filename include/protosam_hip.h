/* protosam_hip.h -- C ABI of libprotosam_hip.so (hand-written gfx950 / CDNA4 kernels for ProtoSAM's hot path).
 *
 * The reference (levayz/ProtoSAM) is pure Python on PyTorch and has no FFI layer: its drop-in boundary is the Python
 * class API (`ProtoSAM.forward`, `FewShotSeg`, `MultiProtoAsConv`, `sam_model_registry`, `SamPredictor`, ...; see
 * SURVEY.md 8b), mirrored by the `protosam_amd` package. This header is the native boundary underneath it: each entry
 * point replaces one chain of stock torch ops of the reference and cites it (paths relative to the reference repo).
 *
 * Conventions: plain pointers and sizes only (no torch types). All pointers are DEVICE pointers unless marked
 * "host". No ownership transfer: the caller allocates every buffer. `stream` is a hipStream_t (0 = default stream);
 * launches are asynchronous on it. Every function returns 0 on success, 1 = bad argument, 2 = launch error.
 * "half" = IEEE fp16 (`_Float16`). Matrices are row-major with the stated leading dimension in ELEMENTS.
 */
#ifndef PROTOSAM_HIP_H
#define PROTOSAM_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- contraction engine --------------------------------------------------------------------------------------
 * out[M,N] = epi(A[M,K] . W[N,K]^T + bias[N]); A, W half (K contiguous), fp32 accumulate on MFMA.
 * epilogue 0: half out;  1: half out = gelu_erf(.);  2: fp32 out = (resid ? resid[r,:] : 0) + (gamma ? gamma : 1)*(.)
 *   3: half out = relu(. + resid16[m,:]) with `resid` pointing at a HALF [*, ldr] map or null (conv + folded BatchNorm
 *   (+ identity) + ReLU of a torchvision ResNet Bottleneck; models/backbone/torchvision_backbones.py:19-23)
 *   resid row r = resid_mod ? m % resid_mod : m (epilogue 2 only: epilogue 3 reads its half residual at row m and rejects
 *   resid_mod != 0 with status 1).  out row = out_seg ? (m/out_seg)*out_seg_stride + out_seg_off + m%out_seg : m.
 * N % 128 == 0, K % 64 == 0. Replaces every nn.Linear / 1x1 conv / patch-embed conv / ConvTranspose2d(2,2) GEMM:
 *   models/segment_anything/modeling/image_encoder.py:223-249 (qkv, proj), modeling/common.py:13-26 (MLPBlock),
 *   image_encoder.py:375-406 (PatchEmbed), :90-106 (neck), modeling/transformer.py:218-240 (image-side projections),
 *   modeling/mask_decoder.py:53-55 (first ConvTranspose2d); DINOv2 Attention/Mlp/PatchEmbed (hub model, call site
 *   models/grid_proto_fewshot.py:88-91). */
int psam_gemm_f16(const void* A, const void* W, const float* bias, void* out, const float* resid, const float* gamma,
                  int M, int N, int K, int lda, int ldw, int ldo, int ldr, int resid_mod, int out_seg,
                  int out_seg_stride, int out_seg_off, int epilogue, void* stream);
/* The packed qkv projection with a head-major result: out half [N / hd planes][M][hd] (plane = which*H + h of
 * `self.qkv(x).reshape(B, N, 3, H, hd)`, image_encoder.py:236-238), read by psam_attention_f16 / psam_relpos with
 * head_major = 1: a head's Q / K / V rows are then contiguous hd-vectors. Same arithmetic as epilogue 0. */
int psam_gemm_f16_heads(const void* A, const void* W, const float* bias, void* out, int M, int N, int K, int lda, int ldw,
                        int hd, void* stream);
/* psam_gemm_f16 with a LayerNorm folded into the GEMMs either side of it (no LayerNorm pass, no cast pass):
 *   epilogue 2 (x = resid + gamma*(a w^T + bias)) also writes out16 = half(x) [.., ld16] and stats: per row and 64-column
 *              group (sum, sum of squares) of x, float [M][N/64][2] (either may be null);
 *   epilogue 0 / 1 take A = half(x), W already multiplied by the LayerNorm weight, bias' = bias + W . ln_bias, and
 *              ln_mr = the buffer psam_ln_finalize fills: float [M][2] = (mean, rstd), then half [M][8] = {hi, hi, lo, 0 x 5} of
 *              -mean; ln_s = float [N] row sums of the fp16 W', then half [N][8] = {hi, lo, hi, 0 x 5} of the same sums (the MFMA
 *              operands of the assembly kernels' rank-1 correction acc -= mean (x) ln_s; ops.fold_layernorm builds ln_s):
 *              out = act(rstd * (acc - mean * ln_s[n]) + bias'[n]).
 * modeling/image_encoder.py:174-193 (norm1 -> attn.qkv, norm2 -> mlp.lin1); DINOv2 Block (norm1 / norm2). */
int psam_gemm_f16_ln(const void* A, const void* W, const float* bias, void* out, const float* resid, const float* gamma,
                     int M, int N, int K, int lda, int ldw, int ldo, int ldr, int resid_mod, int out_seg,
                     int out_seg_stride, int out_seg_off, int epilogue, void* out16, int ld16, float* stats,
                     const float* ln_mr, const float* ln_s, void* stream);
/* stats [M][D/64][2] -> mr: float [M][2] = (mean, 1/sqrt(var + eps)), biased variance (nn.LayerNorm), followed by half [M][8] =
 * {hi, hi, lo, 0, 0, 0, 0, 0} of -mean: 6 floats per row in all */
int psam_ln_finalize(const float* stats, int M, int D, float eps, float* mr, void* stream);


/* One slice through a residual Linear with FEW 256 x 256 tiles and a LONG K (SAM ViT-H mlp.lin2 of one image: 4096 x 1280 x 5120, 80 tiles
 * for 256 CUs), and the LayerNorm that follows it in the block stack, as one split-K launch of the assembly tile + one reduce pass:
 *   x[M,N] (fp32, in place) += A[M,K] . W[N,K]^T + bias;  out16 (optional half [M, ld16]) = LayerNorm(x; ln_w, ln_b, eps), or half(x) when
 *   ln_w is null.
 * `ks` K ranges per tile (ks * tiles workgroups side by side); ws: CALLER-OWNED fp32 scratch of >= ks * Mp * N elements, Mp = M rounded up
 * to a multiple of 256; the ranges are summed in a fixed order (deterministic). The first call per (M, N, ks) on a device builds the
 * work list of the launch in device memory (hipMalloc + a synchronous hipMemcpy), so it must run OUTSIDE stream capture; later calls of
 * that shape allocate nothing and may be captured into a graph (the Python path runs every call once eagerly before it captures).
 * psam_gemm_splitk_ranges returns the ks this device would use for the shape (0: the shape does not pay, or the assembly kernel is not
 * loaded) - a count, not a status; psam_gemm_f16_splitk_ln takes exactly that ks (>= 2), N % 256 == 0, N <= 2048, K % 64 == 0.
 * modeling/common.py:13-26 (MLPBlock.lin2) + image_encoder.py:174-193 (x = x + mlp(...), then the next block's norm1). */
int psam_gemm_splitk_ranges(int M, int N, int K);
int psam_gemm_f16_splitk_ln(const void* A, const void* W, const float* bias, float* x, int M, int N, int K, int lda, int ldw, int ldx,
                            int ks, float* ws, const float* ln_w, const float* ln_b, float eps, void* out16, int ld16, void* stream);

/* Tile override for psam_gemm_f16: 0 auto (default; also env PSAM_GEMM_TILE), 1 = 128x128x64 (HIP), 11 = 256x256x64 persistent
 * 8-wave kernel (HIP), 15 = assembly kernels (csrc/gemm_asm_gen.py, the default large tile), 16 = half-tile ping-pong assembly
 * kernels (csrc/gemm_asm2_gen.py, experimental), 17 = tile 15 with its k-loop on v_mfma_f32_16x16x32_f16 (same shapes as 15; within
 * rounding of it, not bit-identical); a tile that cannot take the call's layout falls back (16 -> 15 -> 11 -> 1, 17 -> 11 -> 1). */
int psam_gemm_set_tile(int tile);
/* *tile = the tile the most recent psam_gemm_f16 / psam_gemm_f16_ln call of this process was dispatched to, after every fallback
 * (0 before the first call): what tests and A/B tools check a forced tile against. 12 (four-deep ring) and 13 (64x64) are reported
 * whenever those kernels ran, forced or chosen for a small launch; a forced 12 / 13 that cannot take the call reports 1. */
int psam_gemm_last_tile(int* tile);
/* Variant of the assembly GEMM (tiles 15 / 16 / 17): 0 = the shipped kernels; 1 = their traced forms, which count cycles per K-tile
 * loop and per epilogue (read back with PSAM_GEMM_ASM_TRACE set) and exist only in a library built with `make GENFLAGS=--trace`
 * (csrc/gemm_asm_gen.py). Any value whose kernels the library does not hold makes the next GEMM return an error. */
int psam_gemm_asm_variant(int variant);
/* Dispatch switches of psam_gemm_f16 (1 = on, the default; initial values also from the environment): "asm" (PSAM_GEMM_ASM) the
 * assembly kernels for the large tiles, "half_tiles" (PSAM_GEMM_HALF) the half-tile assembly kernels for shapes with few 256x256
 * tiles, "splitk" (PSAM_GEMM_SPLITK), "nsplit" (PSAM_GEMM_NSPLIT) the column split of one-slice fc1 shapes; "max_wgs"
 * (PSAM_GEMM_MAX_WGS, an integer, 0 = none) caps the persistent grids of the assembly kernels - two streams then run their GEMMs
 * side by side on disjoint CUs; "mfma16" (PSAM_GEMM_MFMA16) what the automatic choice does where it would pick tile 15: 0 keep 15,
 * 1 take tile 17 wherever it is eligible, negative / unset the measured per-shape rule (csrc/gemm.hip mfma16_auto). Unknown name:
 * error. */
int psam_gemm_set_option(const char* name, int value);
/* Device scratch for the split-K form of psam_gemm_f16 (fp32 partial sums, [ksplit][M][N]): used only when registered and
 * large enough; EPI 2 on few 256x256 tiles with K >= 2048 then runs `ksplit` workgroups per tile + one reduce pass
 * (deterministic). 16-byte aligned; the caller keeps it alive and must not share it between concurrently running streams.
 * ptr = NULL unregisters (no split-K). Env PSAM_GEMM_SPLITK=0 disables the path. */
int psam_gemm_set_workspace(void* ptr, size_t bytes);

/* Row LayerNorm, fp32 in; out_dtype 0: half out (+ optional fp32 copy y2), 1: fp32 out. Appends `zero_tail_rows`
 * all-zero rows. torch.nn.LayerNorm of image_encoder.py:174-193, transformer.py:133-144 and LayerNorm2d
 * (modeling/common.py:31-43) on token-major rows; DINOv2 norm1/norm2/norm. */
int psam_layernorm(const float* x, const float* w, const float* b, void* y, float* y2, int M, int D, int ldx, int ldy,
                   float eps, int out_dtype, int zero_tail_rows, void* stream);

/* Fused multi-head attention on the packed projection qkv half [B,N,3,H,hd] -> out half [B,N,H*hd]; hd in {64, 80}.
 * mode 0 global (DINOv2 Attention); mode 1 global + decomposed rel-pos (rel_h/rel_w fp32, gw == 64); mode 2 ws x ws
 * windows with the reference's zero padding (pad_row half [3,H,hd] = qkv bias) + rel-pos folded into the score MFMA
 * as 32 extra k-slots (relq half [B,H,N,2,32] from psam_relpos, or relq = null and rpack = psam_relpos' windowed table
 * pack: the query-side terms are then computed inside the kernel and never touch HBM).
 * mode 1 with rel_h = rel_w = null and rpack = psam_relpos' GLOBAL table pack: the decomposed rel-pos terms are computed inside the
 * assembly kernel (psam_gattn_asm_{80,64}_fused) for the shapes psam_attention_fused_relpos reports; PSAM_ERR_ARG elsewhere.
 * mode 1 with gw != 64: any gh x gw token map with 1 <= gh, gw <= 64 (N = gh * gw; SAM encoders built for 256 / 384 / 512 pixel inputs)
 * from `rpack` alone (rel_h = rel_w = null): gattn_any_kernel computes the terms itself, both qkv layouts; larger maps PSAM_ERR_ARG.
 * mode 0 with hd = 64 and N >= 128 (DINOv2 at 1297 / 5330 tokens) runs the assembly kernel psam_gattn_asm_64_norel: any token count,
 * the last key tile masked; models/grid_proto_fewshot.py:88-98 (the hub model's Attention.forward).
 * head_major = 0: qkv is token-major [B,N,3,H,hd]; 1: head-major [3,H,B*N,hd] as written by psam_gemm_f16_heads.
 * image_encoder.py:235-251 (Attention.forward), :254-300 (window_partition / unpartition), :337-372. */
int psam_attention_f16(const void* qkv, void* out, const float* rel_h, const float* rel_w, const void* relq,
                       const void* rpack, const void* pad_row, int B, int N, int H, int hd, float scale, int mode, int gh,
                       int gw, int ws, int head_major, void* stream);
/* kernel selection of psam_attention_f16 (A/B, tests; default 5). bit 0: V2 softmax of the HIP global kernels (0 = the serial round-1
 * form); bits 1-2: window kernel (0 attn_kernel, 1 wattn_kernel, 2 the assembly kernel of csrc/wattn_asm_gen.py where it applies -
 * rpack given, hd = 80, 14 x 14 windows of a 64 x 64 token map, token-major qkv - and the persistent wattn_p_kernel elsewhere, 3
 * wattn_p_kernel everywhere); bit 3: the register-staged HIP
 * global kernel; bit 5: mode 1 with `rpack` alone runs the any-map kernel at gw == 64 too (tests, A/B); bit 4: the DMA-fed HIP global kernel everywhere; neither bit 3 nor 4: the assembly global kernel
 * (csrc/gattn_asm_gen.py) where it applies - rel-pos: hd = 80 or 64, N a multiple of 256; no bias: hd = 64, N >= 128; any head count
 * and batch - and the DMA-fed HIP kernel elsewhere. */
int psam_attention_set_variant(int v);
/* *id = the kernel the most recent psam_attention_f16 / psam_relpos call of this process launched, after every fallback (0 before
 * the first call): what tests and A/B tools check a label or a forced variant against. The low byte names the kernel family; the
 * bits above it the template choice that changes the code that ran. Written at the point of launch: a call refused for its arguments leaves the value as it was. */
#define PSAM_ATTN_KERNEL_ATTN 1        /* attn_kernel (register-staged; windows and both global modes) */
#define PSAM_ATTN_KERNEL_WATTN 2       /* wattn_kernel */
#define PSAM_ATTN_KERNEL_WATTN_P 3     /* wattn_p_kernel (persistent) */
#define PSAM_ATTN_KERNEL_GATTN 4       /* gattn_kernel (DMA-fed) */
#define PSAM_ATTN_KERNEL_GATTN_ANY 5   /* gattn_any_kernel */
#define PSAM_ATTN_KERNEL_ASM_REL 6     /* psam_gattn_asm_{80,64}_rel */
#define PSAM_ATTN_KERNEL_ASM_FUSED 7   /* psam_gattn_asm_{80,64}_fused */
#define PSAM_ATTN_KERNEL_ASM_NOREL 8   /* psam_gattn_asm_64_norel */
#define PSAM_ATTN_KERNEL_ASM_WINDOW 9  /* psam_wattn_asm_80 */
#define PSAM_ATTN_KERNEL_RELPOS 10     /* relpos_mfma_kernel (psam_relpos) */
#define PSAM_ATTN_KERNEL_FAMILY 0xff   /* mask of the family */
#define PSAM_ATTN_KERNEL_FULL 0x100    /* the `full` instance (N a multiple of 64) of attn_kernel / gattn_kernel / gattn_any_kernel in
                                        * modes 0 / 1; clear: the ragged instance, or a kernel that has one form */
#define PSAM_ATTN_KERNEL_STAGE64 0x200 /* gattn_any_kernel with stage rows of 64 floats (a map side above 32); clear: 32 */
#define PSAM_ATTN_KERNEL_QT4 0x400     /* relpos_mfma_kernel with four query tiles per wave (N a multiple of 256); clear: one */
#define PSAM_ATTN_KERNEL_V2 0x800      /* attn_kernel in modes 0 / 1 with the V2 softmax; clear: the serial form */
int psam_attention_last_kernel(int* id);
/* 1 when psam_attention_f16(mode 1) computes the rel-pos terms itself from `rpack` for this shape (64 x 64 token map, hd 80 / 64,
 * token-major qkv, the assembly kernels selected), else 0: the caller then runs psam_relpos first.
 * image_encoder.py:325-372 (add_decomposed_rel_pos) inside :235-251. Returns 0 / 1, not a status. */
int psam_attention_fused_relpos(int B, int N, int H, int hd, int gh, int gw);

/* rel_h[b,h,n,k] = q . Rh[qy - k + K-1], rel_w likewise (UNSCALED q), as an MFMA GEMM against the whole table followed by
 * a scatter. Rpack half [2 (h,w)][2 (hi,lo)][RP][HDP] (RP = 128 global / 32 windowed, zero padded).
 * global: rel_h, rel_w fp32 [B,H,N,64]. windowed: relq half [B,H,N,2,32] = hi/lo of (rel_h | rel_w | 0) / scale.
 * image_encoder.py:303-372 (get_rel_pos, add_decomposed_rel_pos). */
int psam_relpos(const void* qkv, const void* Rpack, float* rel_h, float* rel_w, void* relq, int B, int N, int H, int hd,
                int gw, int K, int windowed, float scale, int head_major, void* stream);

/* ---- ALP module ------------------------------------------------------------------------------------------------
 * Prototype bank from token-major support features sup fp32 [h*w, C] (row stride ld) and the foreground mask fp32
 * [MH,MW] (bmask optional, default 1 - mask): nearest resize, avg-pool coverage > thresh, pooled prototypes,
 * global masked-average prototype, safe_norm. bank fp32 [2*cap, C]; meta int[8] = {n_bg, n_fg, fg_mode, n_fg_cells}.
 * force_mode -1: reference FewShotSeg rule; 0 'mask'; 1 'gridconv+'; 2 'gridconv'.
 * models/alpmodule.py:97-159 (get_prototypes), :14-18 (safe_norm); models/grid_proto_fewshot.py:228-231,253-256. */
int psam_alp_bank(const float* sup, int ld, int h, int w, int C, const float* mask, const float* bmask, int MH, int MW,
                  int pool_w, int kernel_size, float thresh, float eps, float* bank, int cap, int* meta, int* slot_bg,
                  int* slot_fg, float* mres, int force_mode, void* stream);

/* pred[b, {bg,fg}, pix] = sum_p softmax_p(d) * d, d = sim_scale * cos(qry[pix], proto_p), fp32 MFMA.
 * models/alpmodule.py:57-94 (get_prediction_from_prototypes), :195. which_only -1: both banks. */
int psam_alp_sim(const float* qry, long long q_bstride, int ld, int B, int npix, int C, const float* bank, int cap,
                 const int* meta, float eps, float sim_scale, float* part, float* pred, int which_only, void* stream);
/* psam_alp_sim over a table of (query slice, bank) entries in one launch (grid: pixel tiles x 96-prototype groups x entries).
 * tab: device array of n_entries 32-byte entries {const float* bank; const int* meta; int cap; int b; int flags; int plane;},
 * flags bit 0 = which (0 bg, 1 fg), bit 1 = direct (the plane's only entry and ceil(cap/96) == 1); entries that feed one output
 * plane are adjacent. Plane pred + plane*npix gets exactly what psam_alp_sim writes for that slice and bank, and the fmaxf over
 * its entries in table order when several feed it (the foreground of K shots). max_groups = max ceil(cap/96) over the entries;
 * part: scratch fp32 [n_entries * max_groups * npix_pad * 3], npix_pad = ceil(npix/64)*64, null when every entry is direct.
 * models/alpmodule.py:57-94 (get_prediction_from_prototypes), :195; models/grid_proto_fewshot.py:244-266 (shots). */
int psam_alp_sim_pairs(const float* qry, long long q_bstride, int ld, int npix, int C, const void* tab, int n_entries,
                       int max_groups, float eps, float sim_scale, float* part, float* pred, void* stream);

/* ---- resampling / packing --------------------------------------------------------------------------------------
 * Every entry point of this section returns 1 before any launch (outputs untouched) when a count or an extent is not positive
 * (B, planes, C, D, n, n_per_img, plane, IH, IW, OH, OW, H, W, S, P, ih, iw, oh, ow), and on the conditions named with it. */
/* F.interpolate(img,(S,S),'bilinear') + im2col of a PxP/stride-P conv -> half [B*(S/P)^2, Kpad].
 * models/grid_proto_fewshot.py:88-89 + DINOv2 PatchEmbed; also SAM PatchEmbed when H == S. Columns C*P*P .. Kpad-1 are zero.
 * Status 1: S % P != 0, Kpad < C*P*P. */
int psam_patchify_bilinear(const float* img, int B, int C, int H, int W, int S, int P, int Kpad, void* out, void* stream);
/* F.interpolate(x, (OH,OW), 'bilinear', align_corners=False), fp32 planes. grid_proto_fewshot.py:272-273; ProtoSAM.py:592-594 */
int psam_bilinear_nchw(const float* in, int planes, int IH, int IW, int OH, int OW, float* out, void* stream);
/* The same resize in the conventions of the vendored SAM copies' postprocess_masks: mode 0 as above, 1 = bilinear
 * align_corners=True (SamBatched, modeling/sam.py:313-320), 2 = nearest (vendored Sam, modeling/sam.py:154-160).
 * Status 1: mode outside 0..2. */
int psam_resize2d(const float* in, int planes, int IH, int IW, int OH, int OW, int mode, float* out, void* stream);
/* token-major feature-map resize fp32 [B][ih*iw,C] -> [B][oh*ow,C] (the 32x32 upsample of grid_proto_fewshot.py:96-98) */
int psam_bilinear_tokens(const float* in, long long in_bstride, int ld, int B, int ih, int iw, int C, int oh, int ow,
                         float* out, void* stream);
/* [bilinear to OHxOW] -> softmax(dim=1) -> argmax for 2-class logits; prob fp32 [B,2,OH,OW], pred u8, fg_sum int[B]
 * (accumulated, caller zeroes; or NULL). With OW % 4 == 0 the rows are stored 16 bytes (prob) and 4 bytes (pred) at a time:
 * prob must then be 16-byte and pred 4-byte aligned. models/ProtoSAM.py:592-602 */
int psam_prob_argmax(const float* logits, int B, int IH, int IW, int OH, int OW, float* prob, void* pred, int* fg_sum,
                     void* stream);
int psam_broadcast_rows(const float* row, int D, float* out, int B, long long stride, long long off, void* stream);
/* psam_prob_argmax twice, for P planes in one launch, keeping only what the connected components read: scores fp32 [P,2,IH,IW]
 * -> [bilinear to OHxOW, align_corners=False] -> softmax -> argmax -> pred u8 [P,OH,OW], fg_sum int[P] (accumulated, caller
 * zeroes; or NULL) -> softmax of the probabilities -> pfg2 fp32 [P,OH,OW] = its foreground channel (psam_ccl_batch's pfg,
 * pfg_stride = OH*OW); prob fp32 [P,2,OH,OW] = the first softmax, or NULL. Replaces models/ProtoMedSAM.py:176-187 and
 * util/utils.py:474-494 (the second softmax: util/utils.py:485). */
int psam_prob2_argmax(const float* scores, int P, int IH, int IW, int OH, int OW, void* pred, float* pfg2, int* fg_sum,
                      float* prob, void* stream);
/* psam_bilinear_nchw then psam_prob_argmax, for P planes in one launch, without the intermediate: grid-resolution class scores
 * fp32 [P,2,GH,GW] -> bilinear to the image size IHxIW (models/grid_proto_fewshot.py:272-273) -> bilinear to OHxOW (skipped when
 * equal) -> softmax -> prob fp32 [P,2,OH,OW] (both channels), argmax -> pred u8 [P,OH,OW], fg_sum int[P] (accumulated, caller
 * zeroes; or NULL). Bit-identical to the two-launch chain. models/ProtoSAM.py:592-602 */
int psam_scores_prob_argmax(const float* scores, int P, int GH, int GW, int IH, int IW, int OH, int OW, float* prob, void* pred,
                            int* fg_sum, void* stream);
/* per-image min/max (order-preserving uint32 pairs); x needs 4-byte alignment only.  models/ProtoSAM.py:660 */
int psam_minmax(const float* x, int B, long long n_per_img, void* mm, void* stream);
/* ((x-min)/(max-min)*255).astype(uint8) -> (u8 - mean)/std -> im2col(16x16) half; mean3/std3 are HOST pointers.
 * models/ProtoSAM.py:651-660; modeling/sam.py:163-173; predictor.py:56-58,88. quantise 0 = ProtoMedSAM.py:203-205.
 * A constant image (max == min) divides by zero as the reference does: the call returns 0, the other images of the batch are
 * unaffected, what that image's rows and u8out hold is unspecified. Status 1: S % P != 0, mean3 or std3 NULL. */
int psam_sam_patchify(const float* img, const void* mm, int B, int S, int P, const float* mean3, const float* std3,
                      int quantise, void* out, void* u8out, void* stream);
/* (x - mean[c]) / std[c] on [B,3,plane]; in_u8: x is uint8. mean3/std3 HOST pointers (NULL: status 1). modeling/sam.py:163-168 */
int psam_normalize_chw(const void* x, int in_u8, int B, long long plane, const float* mean3, const float* std3,
                       float* y, void* stream);
/* im2col of the neck's 3x3/pad-1 conv on a token-major half map (16-byte accesses). Status 1: C % 8 != 0. image_encoder.py:98-104 */
int psam_im2col3x3(const void* in, int B, int H, int W, int C, void* out, void* stream);
/* fp32 -> half, round to nearest even. Status 1: n % 8 != 0. x and y 16-byte aligned (as for the three passes below). */
int psam_cast_f16(const float* x, void* y, long long n, void* stream);
/* The element-wise passes of the reference-width mode of the SAM image encoder (every Linear of a block through psam_gemm_f32x3, fp32 in
 * and out): half -> fp32 (the attention output on its way to attn.proj, modeling/image_encoder.py:249; n % 8 == 0) and nn.GELU in its erf
 * form, in place on fp32 (MLPBlock, modeling/common.py:25-26; n % 4 == 0). Status 1 otherwise. */
int psam_cast_f32(const void* x, float* y, long long n, void* stream);
int psam_gelu_f32(float* x, long long n, void* stream);
/* fp32 -> fp16 pair hi = half(x), lo = half(x - hi) (write_hi = 0: hi is read, e.g. the copy a folded-LayerNorm GEMM wrote). Operands of
 * the split-fp16 GEMMs (hi W_hi + lo W_hi + hi W_lo) of the image encoder's neck: modeling/image_encoder.py:90-106. n % 8 == 0
 * (status 1 otherwise, and for a NULL pointer). */
int psam_split_f16(const float* x, void* hi, void* lo, long long n, int write_hi, void* stream);

/* ---- connected components + per-component statistics ------------------------------------------------------------
 * util/utils.py:474-494 (cv2.connectedComponentsWithStats, confidences), models/ProtoSAM.py:242-289 (bbox, most
 * confident point). tab fp64: [n_found, n_kept, sum(pred), argmax_conf, 0,0,0,0] then 12 doubles per component:
 * {area, sum_x, sum_y, min_x, min_y, max_x, max_y, conf, best_x, best_y, best_p, 0}. */
int psam_ccl(const void* pred, const float* pfg, int H, int W, int cap, int* labels, int* parent, int* counters,
             int* roots, int* acc_i, void* acc_u, double* acc_d, const int* fg_sum, double* tab, void* stream);
/* psam_ccl for B images in one chain of six launches (blockIdx.z = image): pred u8 [B,H,W], pfg with `pfg_stride` floats between
 * images, every scratch array B times the single-image size (contiguous per image), fg_sum int32 [B] or NULL, tab fp64
 * [B][8 + 12*cap]. Replaces the per-slice loop over util/utils.py:468-541 of a batch of slices. */
int psam_ccl_batch(const void* pred, const float* pfg, long long pfg_stride, int B, int H, int W, int cap, int* labels, int* parent,
                   int* counters, int* roots, int* acc_i, void* acc_u, double* acc_d, const int* fg_sum, double* tab, void* stream);

/* ---- SAM prompt encoder / mask decoder --------------------------------------------------------------------------- */
/* grouped fp32 y = act((x [+ x2]) W^T + b) (+ resid); act 1 = ReLU.  transformer.py:218-240, mask_decoder.py:154-176 */
int psam_small_linear(const float* x, const float* x2, const float* W, const float* b, const float* resid, float* y,
                      int G, int M, int N, int K, long long xg, long long wg, long long bg, long long yg, int ldx,
                      int ldy, int act, void* stream);
/* One fp32 linear y = x W^T + b (+ resid) with few rows and a long contraction (the two-way block's MLP output 2048 -> 256,
 * modeling/transformer.py:170-171, common.py:13-26) as `ks` K ranges in one launch + a fixed-order sum: parts fp32 [ks][M][N] is
 * caller-owned scratch. W [N, K] row-major, K % (64 ks) == 0, ks >= 2. */
int psam_small_linear_splitk(const float* x, const float* W, const float* b, const float* resid, float* y, float* parts, int M, int N,
                             int K, int ks, int ldx, int ldy, void* stream);
/* softmax(q k^T / sqrt(hd)) v with <= 16 keys (token self-attention; image->token attention). transformer.py:151-182 */
int psam_small_attention(const void* q, const float* k, const float* v, void* out, int B, int Tq, int Tk, int NH, int hd,
                         int ldq, int ldk, int ldv, int ldo, int q_f16, void* stream);
/* Tokens per prompt set (5 output tokens + sparse prompts: 251 points, or a box and 249 points) up to which the decoder's token
 * kernels run (csrc/common.h carries the same definition). The Python layers refuse more: ops.MAX_PROMPT_TOKENS is the same number. */
#define PSAM_MAX_PROMPT_TOKENS 256
/* psam_small_attention for 1 <= Tk <= PSAM_MAX_PROMPT_TOKENS keys, same arguments and strides: the keys in chunks of 16 staged in
 * LDS once per workgroup (256 (query row, head) threads of one prompt set), chunk-local softmax sums merged online. hd 32 with
 * fp32 q / out (token self-attention) or hd 16 with fp32 or fp16 q / out (image -> token). NH <= 8; k / v 16-byte aligned and
 * ldk, ldv multiples of 4. transformer.py:151-182,218-240 */
int psam_token_attention(const void* q, const float* k, const float* v, void* out, int B, int Tq, int Tk, int NH, int hd,
                         int ldq, int ldk, int ldv, int ldo, int q_f16, void* stream);
/* token -> image cross attention over Nk <= 4096 keys; K, V fp32 (kv_f32 = 1) or half.  transformer.py:163-167, 98-103.
 * 64 <= Nk and T <= PSAM_MAX_PROMPT_TOKENS: one wave per token, 16 tokens per workgroup; otherwise one workgroup per (token, head). */
int psam_t2i_attention(const float* q, const void* K, const void* V, float* out, int B, int T, int Nk, int NH,
                       int kv_f32, void* stream);
/* The same with the 4096 keys of every (prompt set, head) split over S workgroups (1 <= S <= 16; one slice at a time a launch is 8-16
 * workgroups of latency-bound waves otherwise) and a second small launch that merges the partial (max, sum, weighted values) in the
 * order of the split index: `part` fp32 scratch of >= B * NH * S * T * 18 elements, T <= PSAM_MAX_PROMPT_TOKENS, Nk >= 64. Same
 * reference lines as psam_t2i_attention. */
int psam_t2i_attention_split(const float* q, const void* K, const void* V, float* out, int B, int T, int Nk, int NH,
                             int kv_f32, int S, float* part, void* stream);
/* out = (a [+ a2[m % a2_mod]]) w^T + bias [+ resid], all fp32 on the exact-fp32 MFMA: the decoder's projections of the
 * 4096 image tokens (keys [+ key_pe]) and ConvTranspose2d #1 as a GEMM. K % 32 == 0, N % 64 == 0, lds % 4 == 0.
 * transformer.py:163-167,176-180,98-103,218-240 (k_proj / v_proj / q_proj / out_proj); mask_decoder.py:54,137 */
int psam_gemm_f32(const float* a, const float* a2, int a2_mod, const float* w, const float* bias, const float* resid,
                  float* out, int M, int N, int K, int lda, int ldw, int ldo, void* stream);
/* psam_gemm_f32 with a HEAD-MAJOR result: out fp32 [M / nk][N / hd][nk][hd] (image, head, key, channel) - the K / V projections of the
 * two-way transformer's token-to-image attention (modeling/transformer.py:228-230 on the 4096-token operand), read by psam_t2i_attention
 * with bit 1 of kv_f32 set. M % nk == 0, N % hd == 0, hd % 4 == 0; no residual. */
int psam_gemm_f32_heads(const float* a, const float* a2, int a2_mod, const float* w, const float* bias, float* out, int M, int N, int K,
                        int lda, int ldw, int nk, int hd, void* stream);

/* psam_gemm_f32 / psam_gemm_f32_heads at fp32 accuracy on the fp16 matrix pipe (three v_mfma_f32_32x32x16_f16 products on (hi, lo) fp16
 * halves, fp32 accumulation; the dropped lo x lo term is 2^-22 of a product): out[M,N] = (a [+ a2[m % a2_mod]]) @ (wh + wl)^T + bias
 * [+ resid], the product times acc_scale. a / a2 / bias / resid / out fp32; wh / wl fp16 [N, ldw]: the halves of the fp32 weight times a
 * power of two 2^s (so that the lo half of a small weight stays a normal fp16), split once by the caller (wh = half(w 2^s), wl =
 * half(w 2^s - wh)); acc_scale = 2^-s. nk > 0: head-major output [M / nk][N / hd][nk][hd], no residual. K % 32 == 0, N % 64 == 0,
 * every pointer 16-byte aligned. The image-token side of the two-way transformer (modeling/transformer.py:163-167,176-180,98-103,228-230)
 * and the first transposed convolution of the upscaling (modeling/mask_decoder.py:137) as a GEMM. */
int psam_gemm_f32x3(const float* a, const float* a2, int a2_mod, const void* wh, const void* wl, const float* bias, const float* resid,
                    float* out, int M, int N, int K, int lda, int ldw, int ldo, int nk, int hd, float acc_scale, void* stream);
/* y = [LayerNorm](x[src row] + add_vec); emits fp32 y, half y, half (y + pe[row % pe_mod]). With in_mod > 0 the input
 * is one [in_mod,256] embedding per image and prompt row/in_mod reads image img_of_prompt[prompt] (null: image 0).
 * mask_decoder.py:126-127; transformer.py:164,178,180 */
int psam_ln_pe(const float* x, const float* add_vec, const float* w, const float* b, const float* pe, float* y32,
               void* y16, void* ype16, int M, int in_mod, int pe_mod, float eps, int do_ln, const int* img_of_prompt,
               void* stream);
/* PromptEncoder.get_dense_pe (prompt_encoder.py:62-71,195-206), token-major fp32 [gh*gw, 256] */
int psam_dense_pe(const float* G, int gh, int gw, float* pe, void* stream);
/* output tokens ++ point / box-corner embeddings.  prompt_encoder.py:73-101,208-214; mask_decoder.py:121-123 */
int psam_prompt_tokens(const float* coords, const int* labels, const float* G, const float* type_emb,
                       const float* out_tok, int B, int Ns, float img_size, float* tokens, void* stream);
/* LayerNorm2d -> GELU -> ConvTranspose2d(64->32) -> GELU -> hyper-network product.  mask_decoder.py:53-59,137-144 */
int psam_upscale_tail(const float* u1, const float* lnw, const float* lnb, const float* W2r, const float* b2,
                      const float* hyper, float* masks, int B, int g, void* stream);
/* Sam.postprocess_masks first stage; variant 0 upstream (bilinear, align_corners=False), 1 vendored SamBatched
 * (align_corners=True, modeling/sam.py:313-320), 2 vendored Sam (nearest, sam.py:154-160). */
int psam_mask_upsample(const float* low, int planes, int IN, int MID, int variant, float* out, void* stream);
/* pred = OR_b(upsample(low[b,sel]) > thr) sampled by F.interpolate(..., 'nearest') to OUT.  models/ProtoSAM.py:669-676 */
int psam_mask_union(const float* low, int B, int C, int sel, int IN, int MID, int OUT, int variant, float thr,
                    float* pred, void* stream);
/* psam_mask_union for many output masks in one launch, uint8: segs int32 [nseg,3] = (first prompt, prompt count, output index);
 * out u8 [nout,OUT,OUT][segs[s,2]] = OR over low[first .. first+count-1, sel] of (upsample to MID > thr), nearest to OUT; a
 * count of 0 writes zeros, a row pointing outside low [Pm,C,IN,IN] or out is skipped. variant 3 = sigmoid before the resize.
 * Replaces models/ProtoMedSAM.py:49-60 (sigmoid -> bilinear -> > 0.5) and :219-220, per (slice, class). */
int psam_mask_union_seg(const float* low, int Pm, int C, int sel, int IN, const int* segs, int nseg, int nout, int MID, int OUT,
                        int variant, float thr, void* out, void* stream);

/* Candidate statistics of SamAutomaticMaskGenerator without the full-resolution masks: for plane p (prompt p / nsel,
 * channel first + p % nsel of low [B,C,IN,IN]) over y < H, x < W of the MID x MID up-sampling, stats int32 [B*nsel, 8] =
 * {count(v > thr+off), count(v > thr-off), count(v > thr), min_x, min_y, max_x, max_y, 0} (empty: min = INT_MAX, max = -1).
 * automatic_mask_generator.py:293-310; utils/amg.py:156-176 (calculate_stability_score), :303-346 (batched_mask_to_box) */
int psam_mask_stats(const float* low, int B, int C, int first, int nsel, int IN, int MID, int H, int W, int variant,
                    float thr, float off, int* stats, void* stream);
/* out uint8 [n,H,W] = upsample(low plane idx[i]) > thr (automatic_mask_generator.py:305, predictor.py:238-239); with
 * label uint8 [H,W]: counts int64 [n,3] = {tp, fp, fn} against it (models/SamWrapper.py:8-13 get_iou). */
int psam_mask_binarize(const float* low, const int* idx, int n, int IN, int MID, int H, int W, int variant, float thr,
                       unsigned char* out, const unsigned char* label, long long* counts, void* stream);
/* psam_mask_binarize's {tp, fp, fn} for rows chosen on the device, without the masks: row i's plane (into low viewed as
 * [planes,IN,IN]) is rows[i * row_stride] - the plane field of a psam_amg_select record - and the number of rows is *count (device
 * memory) clamped to max_rows; rows beyond it, and rows whose plane is outside [0, planes), do nothing. counts int64 [max_rows,3],
 * zeroed here for all max_rows. Nothing returns to the host. max_rows <= 65535. models/SamWrapper.py:8-13 */
int psam_mask_counts(const float* low, int planes, const int* rows, int row_stride, const int* count, int max_rows, int IN, int MID,
                     int H, int W, int variant, float thr, const unsigned char* label, long long* counts, void* stream);
/* The row the loop of models/SamWrapper.py:40-46 picks from counts int64 [.,3] over the first min(*count, max_rows) rows: IoU =
 * tp / (tp + fp + fn) in float64, row 0 is taken whatever its IoU (NaN included: nothing beats NaN), a later row wins only with
 * `>`. best int32 [4] = {plane of the winner = rows[row * row_stride], its row, 1 if there is no row (then plane 0, row -1),
 * rows looked at}; *iou = the winner's IoU (NaN if there is no row). One wave. */
int psam_best_iou(const long long* counts, const int* rows, int row_stride, const int* count, int max_rows, int* best, double* iou,
                  void* stream);
/* the same statistics (and the binary masks, out uint8 [n,H,W] or null) of MATERIALISED candidate planes fp32 [n,H,W]: the
 * generator's crop layers / images not at the model input size (second resize of postprocess_masks).
 * automatic_mask_generator.py:221-316; utils/amg.py:156-176, 303-346 */
int psam_plane_stats(const float* planes, int n, int H, int W, float thr, float off, int* stats, void* out, void* stream);
/* psam_mask_stats / psam_mask_binarize for an image that is NOT at the model's input size (or a crop): both resizes of
 * Sam.postprocess_masks (modeling/sam.py:132-160 / :296-320) per output pixel, nothing written in between. The value at (y, x) of
 * the OH x OW image is the second-stage interpolation - source size ih x iw = predictor.input_size, the un-padded corner of the
 * MID x MID first-stage map, so its taps clamp at ih - 1 / iw - 1 - of the first-stage values IN -> MID; variant 0 / 1 / 2 =
 * bilinear align_corners False / True / nearest in BOTH stages (psam_mask_upsample's variants, psam_resize2d's modes), 3 is
 * refused. Bit for bit the values of psam_mask_upsample -> [..., :ih, :iw] -> psam_resize2d (csrc/amg_resize.hip).
 * psam_mask_stats_resized: low fp32 [B,C,IN,IN], plane p = prompt p / nsel, channel first + p % nsel -> stats int32 [B*nsel, 8]
 *   with psam_mask_stats' fields and empty-mask values, box in the OH x OW image's frame.
 * psam_mask_binarize_resized: mask i = plane idx[i] of low viewed as [planes,IN,IN], written as {0,1} into the rectangle
 *   [y0, y0+OH) x [x0, x0+OW) of frame i of out uint8 [n,FH,FW] (uncrop_masks, utils/amg.py:255-265); bytes outside the rectangle
 *   are not touched. With label uint8 [FH,FW]: counts int64 [n,3] = {tp, fp, fn} over the rectangle (zeroed here).
 * Planes are the grid's y dimension: B * nsel <= 65535, n <= 65535. PSAM_ERR_ARG for non-positive sizes, ih > MID, iw > MID, a
 * rectangle outside the frame, first < 0 or first + nsel > C, off < 0, label without counts, more planes than the limit.
 * automatic_mask_generator.py:293-316; utils/amg.py:156-176, 303-346 */
int psam_mask_stats_resized(const float* low, int B, int C, int first, int nsel, int IN, int MID, int ih, int iw, int OH, int OW,
                            int variant, float thr, float off, int* stats, void* stream);
/* psam_mask_stats_resized for the candidates that pass the generator's first filter only: score fp32 [B,C] (the decoder's predicted
 * IoUs, indexed like low's planes); a plane whose score fails `score > (float)score_thresh` (NaN fails) keeps the empty-mask row and
 * costs nothing. The generator drops those candidates before it reads their statistics (automatic_mask_generator.py:293-295), on
 * the host and in psam_amg_select with this same float32 comparison. score = NULL is refused. */
int psam_mask_stats_resized_scored(const float* low, const float* score, double score_thresh, int B, int C, int first, int nsel,
                                   int IN, int MID, int ih, int iw, int OH, int OW, int variant, float thr, float off, int* stats,
                                   void* stream);
int psam_mask_binarize_resized(const float* low, const int* idx, int n, int IN, int MID, int ih, int iw, int OH, int OW, int variant,
                               float thr, unsigned char* out, int FH, int FW, int y0, int x0, const unsigned char* label,
                               long long* counts, void* stream);

/* Uncompressed COCO run-length code of binary masks uint8 [n,H,W] (any non-zero byte is set), on the device: pixels in
 * column-major order p = x*H + y, counts alternate zero-run / one-run lengths and start with a zero-run (a set first pixel
 * gives a leading 0), at most H*W + 1 counts per mask. Replaces mask_to_rle_pytorch / rle_to_mask, utils/amg.py:107-149
 * (called at automatic_mask_generator.py:312-313), without transposing the mask. No atomics: the output is bit-identical
 * from run to run. Encoding is two calls, because the caller sizes `counts` from the totals in between:
 * psam_rle_workspace: *ints_per_mask = int32 words of `cells` per mask; host arithmetic only, no launch.
 * psam_rle_count: totals int64 [n] = number of counts of each mask; fills `cells` (int32 [n * ints_per_mask]) for
 *   psam_rle_write. utils/amg.py:107-135
 * psam_rle_write: offsets int64 [n+1] = exclusive running sum of totals (offsets[0] = 0); counts int32 [offsets[n]], mask i
 *   at counts[offsets[i] .. offsets[i+1]). `masks` and `cells` unchanged since psam_rle_count. utils/amg.py:107-135
 * psam_rle_decode: masks_out uint8 {0,1} [n,H,W] from `ends` int64 [offsets[n]] = the INCLUSIVE running sum of the flat
 *   counts (over all masks) and the same offsets; a pixel past the end of a short list is 0. utils/amg.py:138-149
 * Status 1 before any launch: n, H or W <= 0, H*W > 2^31 - 1, a null pointer. Any n (chunked inside over the grid limit). */
int psam_rle_workspace(int H, int W, long long* ints_per_mask);
int psam_rle_count(const unsigned char* masks, int n, int H, int W, int* cells, long long* totals, void* stream);
int psam_rle_write(const unsigned char* masks, int n, int H, int W, const int* cells, const long long* offsets, int* counts,
                   void* stream);
int psam_rle_decode(const long long* ends, const long long* offsets, int n, int H, int W, unsigned char* masks_out,
                    void* stream);

/* Scoring: confusion counts and boxes of n (prediction plane, label plane) pairs in one launch, exact (integer atomics).
 * rows int32 [n,4] = (pred plane, pred value, label plane, label value); pixel i of a row is predicted iff
 * pred[pred plane][i] == pred value and true iff label[label plane][i] == label value (float planes compare by value).
 * pred / label: [planes, H, W] with contiguous planes `*_stride` ELEMENTS apart, element type `*_dtype` as vol_dtype below
 * (0 int16, 1 float32, 2 uint8, 3 int32); element-aligned, no other alignment asked for.
 * out int64 [n,12], columns in this order:
 *   0 tp, 1 fp, 2 fn, 3 tn, 4 pred x0, 5 pred y0, 6 pred x1, 7 pred y1, 8 gt x0, 9 gt y0, 10 gt x1, 11 gt y1
 * (inclusive extremes; an empty set gives x0 = y0 = INT_MAX, x1 = y1 = -1, as psam_mask_stats). A row whose pred plane is
 * outside [0, pred_planes) or whose label plane is outside [0, label_planes) is skipped: its out row keeps these initial values
 * with four zero counts, and nothing is read for it. n >= 1 (no 65535 limit), H, W >= 1, H * W < 2^31 - 4096.
 * Replaces validation_protosam.py:49-62 (get_bounding_box), :169-185 (get_dice_iou_precision_recall), :400-409 (their use per
 * slice) and util/metric.py:50-107 (Metric.record), all of which work on a host copy of the mask. */
int psam_seg_counts(const void* pred, int pred_dtype, int pred_planes, long long pred_stride, const void* label,
                    int label_dtype, int label_planes, long long label_stride, int H, int W, const int* rows, int n,
                    long long* out, void* stream);

/* Surface-distance metrics (csrc/surface.hip): Hausdorff distance, its 95th percentile and the average (symmetric) surface
 * distance of n (prediction, ground truth) pairs, MedPy's hd / hd95 / asd / assd with connectivity=1.
 * rows int32 [n,5] = (first pred plane, pred value, first label plane, label value, depth D): the row covers D consecutive planes
 * of each tensor; comparisons, dtypes and strides as psam_seg_counts. The surface of a set is its voxels with a face neighbour
 * (4 in the plane for D == 1, 6 for D > 1) that is not in the set or lies outside the row's D x H x W range. Segment 2r is the
 * prediction's surface of row r, segment 2r + 1 the ground truth's.
 * psam_surface_points: counts int32 [2n] = the true surface sizes; offsets int32 [2n+1] = their exclusive scan (saturated at
 *   INT_MAX); status int32 [n]: 0 filled, 1 the row's segments end beyond cap (not filled; an empty row always fits), 2 the row
 *   is outside the planes or its depth outside 1 .. max_depth (nothing read, counts 0); points int32 [cap]: a surface voxel as
 *   its index (z * H + y) * W + x in the row's range, in no particular order inside a segment; tiles int32 [2n+1] and cursors
 *   int32 [2n] are work tables (tiles: the scan of the distance tiles, read by psam_surface_dist).
 * psam_surface_dist: d2 fp32 [cap]: for every filled point the minimum over the other segment of its row of
 *   ((dx*sx)*(dx*sx) + (dy*sy)*(dy*sy)) + (dz*sz)*(dz*sz), each operation a separately rounded fp32 one on exact integer offsets and
 *   the spacing rounded to fp32; +inf where the other segment is empty. keys (may be null) int64 [cap]: segment << 32 | bits of d2,
 *   so that ONE ascending sort of keys sorts every segment in place. Positions that are not filled are not written.
 *   The grid is cap / 256 + 2n workgroups whatever the counts are; max_depth == 1 takes the two-term form.
 * psam_surface_stats: sorted = the d2 of every segment ascending, element i at 4 * stride bytes * i (stride 1: the fp32 array,
 *   2: the low words of sorted keys). out float64 [n,8] = {n_pred, n_gt, hd, hd95, assd, asd_pg, asd_gp, status}: hd the larger
 *   directed maximum, hd95 numpy.percentile(., 95) of both directed sets together, asd_pg / asd_gp the directed means (prediction
 *   to ground truth and back), assd their mean; all of sqrt((double)d2), summed in a fixed order: the same bits run to run and for
 *   every cap that fits. The five are NaN where a surface is empty or status != 0.
 * Status 1 before any launch: a null pointer, n < 1, cap outside 1 .. 2^31 - 2, H, W or max_depth outside 1 .. 2^24,
 * max_depth * H * W > 2^31 - 4097, a spacing that is not positive and finite as fp32, stride not 1 or 2. */
int psam_surface_points(const void* pred, int pred_dtype, int pred_planes, long long pred_stride, const void* label,
                        int label_dtype, int label_planes, long long label_stride, int H, int W, int max_depth, const int* rows,
                        int n, int* counts, int* offsets, int* tiles, int* status, int* cursors, int* points, int cap,
                        void* stream);
int psam_surface_dist(const int* points, const int* offsets, const int* tiles, int n, int H, int W, int max_depth, double sz,
                      double sy, double sx, int cap, float* d2, long long* keys, void* stream);
int psam_surface_stats(const void* sorted, int stride, const int* counts, const int* offsets, const int* status, int n,
                       double* out, void* stream);

/* PromptEncoder.mask_downscaling for mask prompts: masks fp32 [n,4g,4g] -> dense embeddings fp32 token-major [n,g*g,256].
 * wts = c1w[4][4] c1b[4] n1w[4] n1b[4] c2w[16][4][2][2] c2b[16] n2w[16] n2b[16] c3w[256][16] c3b[256] (4684 floats).
 * prompt_encoder.py:51-59,102-105; common.py:31-43 (LayerNorm2d) */
int psam_mask_downscale(const float* masks, const float* wts, int n, int g, float eps, float* out, void* stream);

/* Negative point prompts: keys[0] = most confident background pixel with p_bg >= thr (ProtoSAM.py:361-372), keys[1+k] = most
 * confident background pixel of the ring dilate_r(component k) \ component k, r iterations of a 3x3 dilation
 * (ProtoSAM.py:395-419; labels / tab as written by psam_ccl). key = float_bits(p_bg) << 32 | (0xFFFFFFFF - y*W - x); 0 = none. */
int psam_neg_points(const int* labels, const float* pbg, const double* tab, int H, int W, int max_comp, int r, float thr,
                    unsigned long long* keys, void* stream);
/* psam_neg_points for P planes in one launch (ProtoSAM.py:361-372,395-419 per (slice, class) plane): labels int32 [P,H,W] as
 * psam_ccl_batch writes them, pbg fp32 with pbg_stride floats between planes, tabs fp64 [P][8 + 12*cap], keys [P][max_comp+1]
 * (max_comp <= cap, P*(max_comp+1) <= 65535); plane p's keys are those of psam_neg_points on plane p. */
int psam_neg_points_batch(const int* labels, const float* pbg, long long pbg_stride, const double* tabs, int cap, int P, int H,
                          int W, int max_comp, int r, float thr, unsigned long long* keys, void* stream);

/* The k most confident pixels of every component (num_points_for_sam = k > 1), models/ProtoSAM.py:266-289 (get_most_conf_points:
 * torch.topk(output_p_fg[mask], k) per component), with the tie rule of the component table: largest p_fg first, first pixel in
 * raster order among equals. labels int32 [P,H,W] as psam_ccl_batch writes them (0 = background or a component beyond the table,
 * component c = label c + 1), pfg fp32 >= 0 with pfg_stride floats between planes, tabs fp64 [P][8 + 12*cap] (read on the device
 * for tab[1] and tab[3]). keys uint64 [P][R][k], R = max_comp, or R = 1 with only_best (the row of component tab[3], what use_cca
 * keeps): row c = the k largest keys float_bits(p_fg) << 32 | (0xFFFFFFFF - y*W - x) of component c's pixels in descending order;
 * a component of fewer than k pixels fills its first `area` slots, the others are 0; rows of components >= min(tab[1], max_comp)
 * are 0; every element of keys is written. Radix select with per-component byte histograms (integer atomics, pre-aggregated per
 * wave), compaction, one bitonic sort per row (csrc/topk_points.hip). scratch: 8-byte aligned, psam_topk_points_workspace bytes.
 * Status 1 before any launch: k < 1 or k > PSAM_MAX_PROMPT_TOKENS - 5, max_comp < 1 or > cap, cap > 4096, P, H or W <= 0,
 * P > 65535, H*W > 2^31 - 1, a null pointer, scratch too small or misaligned. */
int psam_topk_points_workspace(int P, int max_comp, int only_best, long long* bytes);
int psam_topk_points_batch(const int* labels, const float* pfg, long long pfg_stride, const double* tabs, int cap, int P, int H,
                           int W, int k, int max_comp, int only_best, unsigned long long* keys, void* scratch,
                           long long scratch_bytes, void* stream);
/* psam_topk_points_batch for one plane (models/ProtoSAM.py:266-289): labels int32 [H,W], pfg fp32 [H,W], tab fp64 [8 + 12*cap],
 * keys uint64 [R][k]. */
int psam_topk_points(const int* labels, const float* pfg, const double* tab, int cap, int H, int W, int k, int max_comp,
                     int only_best, unsigned long long* keys, void* scratch, long long scratch_bytes, void* stream);

/* Box NMS and the automatic mask generator's candidate selection on the device (csrc/nms.hip), bit for bit the host code of
 * segment_anything/utils/amg.py nms_xyxy (the contract of torchvision's batched_nms, automatic_mask_generator.py:262-268) and of
 * the score filters in front of it (automatic_mask_generator.py:293-303). Rows come in G groups: group g is rows offsets[g] ..
 * offsets[g+1] (int32 [G+1] in DEVICE memory, ascending, within [0, n]); max_group >= the largest group, 1 <= max_group <= 16384
 * (a 64 x 64 point grid gives 12288 candidates). A group whose offsets break these rules gets count[g] = -1 and nothing else.
 * psam_nms_workspace: bytes of scratch for G groups of up to max_group rows; host arithmetic only.
 * psam_box_nms: boxes [n,4] (x0, y0, x1, y1) int32, or fp32 with boxes_fp32; scores fp32 [n]; both finite, boxes 16-byte aligned.
 *   Rows are visited by decreasing score, equal scores in index order (-0.0 == 0.0); a visited row is kept and removes every later
 *   row whose IoU with it, widened to double, is > thr (== thr stays; 0 / 0 of two empty boxes is NaN and removes nothing); a
 *   removed row removes nothing. Areas, intersection, union and the correctly rounded quotient are separately rounded fp32
 *   operations. kept int32 [G,cap]: group g's kept rows (indices inside the group) in visiting order; count int32 [G]: how many
 *   were kept - which may exceed cap: only the first cap are stored, the rest of a kept row is not written.
 * psam_amg_select: stats int32 [n,8] as psam_mask_stats writes it; iou4 fp32 [(n+2)/3, 4], the decoder's predicted IoUs read in
 *   place: candidate c is row c / 3, column 1 + c % 3. A candidate passes if iou > (float)pred_iou_thresh (applied only when
 *   pred_iou_thresh > 0) and (float)stats[0] / (float)stats[1] >= (float)stability_thresh (only when > 0; 0 / 0 fails); its box is
 *   stats[3..6], or [0,0,0,0] where stats[2] == 0; its score is the predicted IoU. records int32 [G,cap,9], per kept candidate in
 *   visiting order {c, plane (c / 3) * 4 + 1 + c % 3 of the decoder's [.,4,256,256] output viewed as planes, predicted IoU bits,
 *   stability bits (a NaN, 0 / 0 with the filter off, as 0x7fc00000), area, x0, y0, x1, y1}; count as above. One copy of records and count gives the host every field of a record.
 * Status 1 before any launch: G < 1 or > 65535, max_group outside 1 .. 16384, n < 0, cap < 1, a NaN threshold, a null or
 * misaligned (16 bytes) pointer, scratch too small. Stream-ordered launches only, no flags or waits between workgroups; every
 * loop is bounded by the group's size. */
int psam_nms_workspace(int G, int max_group, long long* bytes);
int psam_box_nms(const void* boxes, int boxes_fp32, const float* scores, const int* offsets, int n, int G, int max_group,
                 double thr, int* kept, int cap, int* count, void* scratch, long long scratch_bytes, void* stream);
int psam_amg_select(const int* stats, const float* iou4, const int* offsets, int n, int G, int max_group, double pred_iou_thresh,
                    double stability_thresh, double nms_thresh, int* records, int cap, int* count, void* scratch,
                    long long scratch_bytes, void* stream);
/* psam_amg_select for the candidates of one crop (automatic_mask_generator.py:309-311): a candidate that passes the score filters
 * is also dropped when its box is near a crop edge, utils/amg.py:199-206 in integers - with v = box[k] + crop_box[k % 2] (the box in
 * the image's frame), some k has |v - crop_box[k]| <= 20 and not |v - orig_box[k]| <= 20. The box is stats[3..6], or [0,0,0,0]
 * where stats[2] == 0, as everywhere else; the records keep boxes in the crop's frame. crop_box, orig_box: HOST int[4], XYXY (the
 * crop inside the image, and [0, 0, W, H]); NULL is status 1. Everything else as psam_amg_select. */
int psam_amg_select_crop(const int* stats, const float* iou4, const int* offsets, int n, int G, int max_group,
                         double pred_iou_thresh, double stability_thresh, double nms_thresh, const int* crop_box,
                         const int* orig_box, int* records, int cap, int* count, void* scratch, long long scratch_bytes,
                         void* stream);

/* ---- crop layers of the automatic mask generator on the device (csrc/amg_crops.hip) ----------------------------------------------
 * What lies between the per-crop selection (psam_amg_select_crop) and the image's final records, automatic_mask_generator.py:194-262,
 * with nothing read back in between. Device tables, int32:
 *   merged [pool_cap,11]: a psam_amg_select record with its box in the IMAGE's frame, then {crop index, pool row};
 *   bases  [ncrops+1]   : bases[c] = merged records of the crops before c. Crop c's call reads bases[c] (0 for c = 0) and writes
 *                         bases[c+1]; the calls of one image must be issued in crop order on one stream. No clearing needed.
 *   geom   [ncrops,8]   : {x0, y0, crop width, crop height, ih, iw (predictor.input_size of the crop), bits of the float32 NMS score
 *                         1 / crop area (utils/amg.py / automatic_mask_generator.py:208-213), 0}.
 * psam_amg_keep_planes: records int32 [cap,9] and count int32 [1] as psam_amg_select_crop wrote them for crop `crop`, whose origin in
 *   the image is (x0, y0); low fp32 [low_planes,IN,IN] the decoder's output that the records' plane indices refer to. The first
 *   k = min(count, cap) records (count is read on the device; the launch is sized for cap) are appended to `merged` at rows bases[crop] ..,
 *   box moved by (x0, y0), and each record's plane is copied to the same row of pool fp32 [pool_cap,IN,IN]. Rows >= pool_cap are written
 *   nowhere; bases keeps counting, and psam_amg_crops_nms reports the overflow.
 * psam_amg_crops_workspace: bytes of scratch psam_amg_crops_nms needs; host arithmetic only.
 * psam_amg_crops_nms: cross-crop NMS of the bases[ncrops] merged records: psam_box_nms (its rule, its order among equal scores)
 *   with every record scored by its crop's geom score; use_nms = 0 (a single crop box, :208) keeps all in merged order.
 *   out int32 [pool_cap*11 + 2]: the final records in suppression order, then the final count (-1: bases[ncrops] > pool_cap, the pool
 *   overflowed and nothing else of out is meaningful), then bases[ncrops]. One copy of out gives the host the whole decision.
 * psam_mask_binarize_crops: out uint8 [m,H,W], every byte written: frame i is zero outside the rectangle of final record i's crop and
 *   holds, inside it, the bits of psam_mask_binarize_resized of the record's pool plane with that crop's (ih, iw), crop size and
 *   origin. One launch serves records of crops of different sizes. A record whose crop index, pool row or geometry is out of range
 *   gives a zero frame.
 * Status 1 before any launch: pool_cap outside 1 .. 16384 (the group limit of psam_box_nms), crop outside [0, ncrops), negative
 * origin, cap < 1, IN*IN not a multiple of 4, low or pool not 16-byte aligned, m outside 1 .. pool_cap, variant outside 0 .. 2,
 * a NaN threshold, a null pointer, scratch too small or misaligned (16 bytes). */
int psam_amg_keep_planes(const float* low, int low_planes, int IN, const int* records, const int* count, int cap, int crop, int ncrops,
                         int x0, int y0, float* pool, int pool_cap, int* merged, int* bases, void* stream);
int psam_amg_crops_workspace(int pool_cap, long long* bytes);
int psam_amg_crops_nms(const int* merged, const int* bases, int ncrops, const int* geom, int pool_cap, double thr, int use_nms,
                       int* out, void* scratch, long long scratch_bytes, void* stream);
int psam_mask_binarize_crops(const float* pool, int pool_cap, const int* final_records, int m, const int* geom, int ncrops, int IN,
                             int MID, int variant, float thr, unsigned char* out, int H, int W, void* stream);

/* ---- small-region removal for a batch of masks (csrc/small_regions.hip) --------------------------------------------------
 * Per mask, bit for bit remove_small_regions(mask, t, "holes") then remove_small_regions(., t, "islands")
 * (segment_anything/utils/amg.py:267-291; the stage of automatic_mask_generator.py:332-380), 8-connected:
 *   holes   : every region of the complement with (double)area < area_thresh is filled, the outer background included;
 *             changed_holes = such a region exists.
 *   islands : on the filled mask; if no foreground region is below the threshold nothing changes, otherwise every such region is
 *             dropped, and if that drops all of them the largest stays (among equal largest: the one whose first pixel comes first
 *             in raster order). changed_islands = a region below the threshold exists.
 * masks uint8 [m,H,W], 0 / non-0 -> out uint8 [m,H,W], 0 / 1 (equal to the input's 0 / 1 form where nothing changed);
 * info int32 [m,4] = {changed_holes, changed_islands, area of out, 0}; boxes int32 [m,4] = XYXY min / max of out, {0,0,0,0} for
 * an empty mask; scores fp32 [m] = 1 if neither flag is set, else 0 (the reference's float(not changed)) - boxes and scores as
 * psam_box_nms reads them. Regions are counted per union-find root: there is no limit on their number.
 * The m masks are walked in chunks of `chunk` (<= 65535 per launch), every launch enqueued, no host wait: scratch holds a chunk,
 * psam_small_regions_workspace bytes = chunk * (8 * H * W + 64), 8-byte aligned. Eleven stream-ordered launches per chunk; no
 * flags or waits between workgroups.
 * Status 1 before any launch: m < 0, H or W <= 0, H * W beyond int32 (or H * (W rounded up to 256) beyond 2^32 - 1), chunk < 1,
 * a NaN threshold, and with m > 0 a NULL pointer, misaligned or short scratch. m == 0 does nothing and returns 0. */
int psam_small_regions_workspace(int H, int W, int chunk, long long* bytes);
int psam_small_regions(const void* masks, int m, int H, int W, double area_thresh, int chunk, void* out, int* boxes, float* scores,
                       int* info, void* scratch, long long scratch_bytes, void* stream);

/* ---- connected-component clean-up of binary volumes (csrc/volume_regions.hip) -----------------------------------------------
 * R volumes of D x H x W uint8 voxels (non-0 = set); voxel (r, z, y, x) of `vol` and of `out` lies at
 * base + r * stride_r + z * stride_z + y * W + x: a class-major [R,D,H,W] buffer has stride_r = D*H*W, stride_z = H*W, a
 * slice-major [Z,C,S,S] buffer of kept masks is cleaned where it lies with stride_r = S*S, stride_z = C*S*S.
 * connectivity 6 / 18 / 26 = face, face + edge, face + edge + corner neighbours (scipy's generate_binary_structure(3, 1 | 2 | 3);
 * with D == 1 they are 4 / 8 / 8 in the plane). Every component with size < min_voxels is dropped; keep_largest = 1 keeps only
 * the largest survivor, among equally large ones the one whose first voxel comes first in raster order (z, y, x). A min_voxels
 * above every size leaves `out` empty (psam_small_regions keeps the largest island in that case; this entry does not).
 * out uint8 {0, 1}, same geometry as vol; out == vol is allowed. info int64 [R,12] = components found, components kept, voxels
 * in, voxels out, size of the input's largest component, its root as (z * H + y) * W + x (-1 for an empty volume), the box of
 * out z0, y0, x0, z1, y1, x1 inclusive (all -1 for an empty out). labels (NULL skips it) int32 [R,D,H,W] contiguous: 0 for
 * background, the input's components before any filtering numbered 1..n per volume in the raster order of their first voxel
 * (scipy.ndimage.label's numbering), by a two-level prefix count of the roots: no limit on their number.
 * The R volumes are walked in chunks of `chunk` (<= 65535 per launch), every launch enqueued on `stream`, no host wait. scratch,
 * 8-byte aligned, holds a chunk: chunk * (8 * D*H*W + 64 + (labels ? 4 * ceil(D*H*W / 256) : 0)) bytes.
 * Status 1 before any launch: R < 0, D, H or W <= 0, D*H*W >= 2^31 (or D * H * (W rounded up to 256) beyond 2^32 - 1), chunk < 1,
 * connectivity not 6 / 18 / 26, min_voxels < 0, keep_largest not 0 / 1, a stride below H*W, and with R > 0 a NULL vol, out, info
 * or scratch, misaligned or short scratch. R == 0 does nothing and returns 0. */
int psam_volume_regions(const void* vol, int R, int D, int H, int W, long long stride_r, long long stride_z, int connectivity,
                        long long min_voxels, int keep_largest, int chunk, void* out, long long* info, int* labels, void* scratch,
                        long long scratch_bytes, void* stream);

/* Slice hand-off from a scan volume (raw NIfTI voxels [Z,H,W]; vol_dtype 0 int16, 1 float32, 2 uint8, 3 int32).
 * psam_volume_stats: out[0] = sum(x), out[1] = sum(x^2) in fp64, x = voxel*slope + inter  (MR_normalize / get_CT_statistics,
 *   dataloaders/dataset_utils.py:76-108).
 * psam_volume_slices: out fp32 [Z,tile,S,S] = tile copies of cv2.resize((x - mean) * inv_std, (S,S), INTER_LINEAR) per slice
 *   (mode 0), or cv2.INTER_NEAREST of the raw values for label volumes (mode 1).
 *   dataloaders/ManualAnnoDatasetv2.py:165-187 (read_dataset), :317-327 (tile_z_dim).
 * Status 1 before any launch: n <= 0; Z, H, W, S or tile <= 0; mode outside 0 / 1; vol_dtype outside 0 .. 3. */
int psam_volume_stats(const void* vol, int vol_dtype, long long n, float slope, float inter, double* out, void* stream);
int psam_volume_slices(const void* vol, int vol_dtype, int Z, int H, int W, float slope, float inter, float mean,
                       float inv_std, int S, int tile, int mode, float* out, void* stream);

/* Convolution front-end of the ResNet-101 encoder (models/backbone/torchvision_backbones.py:12-52; torchvision's
 * deeplabv3_resnet101 backbone, output stride 8): im2col on token-major (NHWC) half maps for any kernel / stride / dilation /
 * padding, the 7x7 stride-2 stem straight from the fp32 NCHW image, and MaxPool2d(3, 2, 1). The convolutions themselves are
 * psam_gemm_f16 with BatchNorm folded into weights and bias (epilogue 3).
 * psam_maxpool3x3s2 keeps the maximum with fmaxf, which drops a NaN where F.max_pool2d propagates it: its input is a post-ReLU
 *   half map, which holds none.
 * Status 1 before any launch: psam_im2col with B, H, W, C, kh, kw, stride or dil <= 0, pad < 0, C % 8, ldo % 8, ldo < kh*kw*C
 *   or no output pixel (the map smaller than the dilated kernel); psam_im2col_stem with B, H or W <= 0, ldo < 147 (so 144) or
 *   ldo % 8; psam_maxpool3x3s2 with B, H, W or C <= 0. */
int psam_im2col(const void* in, int B, int H, int W, int C, int kh, int kw, int stride, int dil, int pad, int ldo, void* out,
                void* stream);
int psam_im2col_stem(const float* img, int B, int H, int W, int ldo, void* out, void* stream);
int psam_maxpool3x3s2(const void* in, int B, int H, int W, int C, void* out, void* stream);

/* ---- rotation test-time augmentation: ProtoSAM.forward(..., degrees_rotate != 0) ---------------------------------------------
 * Replaces util/utils.py:66-83 `rotate_tensor_no_crop` (torchvision `rotate(expand=True)` + `resize(antialias=True)`) and
 * util/utils.py:40-59 `reverse_tensor` (`resize` + `rotate(expand=False)` + centre crop), called from models/ProtoSAM.py:544
 * and :553. torchvision 0.15.2 (requirements.txt:65) is not in /root/reference: restated from its tensor code path
 * (affine grid + grid_sample NEAREST / aten _upsample_bilinear2d_aa), see oracle/rotate.py.
 * psam_rotate_nearest: planes [C,H,W] fp32 -> [C,outH,outW]; xg / yg = the base-grid linspace values of the (expanded)
 *   canvas, rt6 = host pointer to the 3x2 rescaled theta (row-major), crop_* = first canvas row / column kept.
 *   The index arithmetic is written with round-to-nearest intrinsics, one per operation (no contraction): bit-reproducible.
 * psam_resize_aa: anti-aliased bilinear [C,H,W] -> [C,OH,OW] (tmp = fp32 scratch [C,H,OW]).
 * Status 1 before any launch: a non-positive extent, a negative crop, a null rt6 / xg / yg (rotate) or a null tmp (resize). */
int psam_rotate_nearest(const float* src, float* dst, const float* xg, const float* yg, const float* rt6, int C, int H, int W,
                        int crop_y, int crop_x, int outH, int outW, void* stream);
int psam_resize_aa(const float* src, float* tmp, float* dst, int C, int H, int W, int OH, int OW, void* stream);

/* Fused intake of n uint8 images of different sizes, packed in `src` (src_bytes long): resize to (oh, ow), (v - mean[c]) / std[c],
 * zero padding to S x S -> out fp32 [n, C, S, S], one launch, no global scratch. dataloaders/PolypDataset.py:319-348 through
 * models/segment_anything/utils/transforms.py:62-110 (mode 0) and predictor.py:47-58 through transforms.py:30-38 (mode 1).
 * rows_host: n rows of 5 int64 in HOST memory: byte offset of the image in src, H, W, oh, ow ((oh, ow) = get_preprocess_shape(H, W,
 *   S) for the reference's use; any 1 <= oh, ow <= S is served). They are checked here and copied to rows_dev (n * 5 int64 of DEVICE
 *   memory), the table the kernel reads.
 * C = 3: interleaved [H, W, 3] images; C = 1: [H, W] planes (normalised with mean3[0] / std3[0]).
 * mode 0: aten _upsample_bilinear2d_aa in fp32, bit-identical to uint8 -> float, psam_resize_aa, psam_normalize_chw, pad.
 *   threshold = 1 (C = 1, mode 0 only; mean3 / std3 may be NULL): v > 0.5f ? 1 : 0 instead of the normalisation.
 * mode 1: Pillow's Image.resize((ow, oh), BILINEAR) of the uint8 image, exactly, then the normalisation of the uint8 value.
 * mean3 / std3 are HOST pointers. Status 1, with `out` and rows_dev untouched: a null pointer, n outside [1, 65535], C not 1 or 3,
 *   S outside [1, 16384], a bad mode / threshold combination, a source side outside [1, 8192], oh or ow outside [1, S], a source side
 *   above 16 times its resized side, an image that does not lie inside [0, src_bytes). */
int psam_image_intake(const void* src, long long src_bytes, const long long* rows_host, void* rows_dev, int n, int C, int S, int mode,
                      int threshold, const float* mean3, const float* std3, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
