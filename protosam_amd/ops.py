"""Thin tensor -> raw-pointer adapters over the C-ABI kernels. PyTorch is used here only for device
memory and the current HIP stream; all arithmetic happens in ``libprotosam_hip.so``."""
import torch

from . import _lib

EPI_F16, EPI_GELU_F16, EPI_F32, EPI_RELU_F16 = 0, 1, 2, 3


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """the current HIP stream's handle. (torch.cuda.current_stream() builds a Stream object through five Python layers - 3 us a call,
    0.7 ms per slice of a one-slice forward with its ~230 launches; the raw accessors are two C calls)"""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event bracket around every launch of one C-ABI entry (used by bench.py for the roofline object:
    events are recorded on the stream the kernel is launched on). `work` is the algorithmic FLOPs or bytes per launch."""

    def __init__(self):
        self.records = []  # (start_event, end_event, work)
        self.tags = {}     # record index -> tag

    def start(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stop(self, e0, work, tag=None):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.records.append((e0, e1, work))
        if tag is not None:
            self.tags[len(self.records) - 1] = tag

    def by_tag(self):
        """{tag: (launches, seconds, work)} over the tagged records (the GEMM timer tags a launch with (M, N, K, epilogue, folded))."""
        out = {}
        for i, tag in self.tags.items():
            a, b, w = self.records[i]
            n, t, f = out.get(tag, (0, 0.0, 0.0))
            out[tag] = (n + 1, t + a.elapsed_time(b) * 1e-3, f + float(w[0] if isinstance(w, tuple) else w))
        return out

    def summary(self):
        """(n_launches, total_seconds, total_work) -- call after a device synchronize. `work` may be a tuple (bytes, flops):
        the first member is summed here, `summary2` sums the second."""
        t = sum(a.elapsed_time(b) for a, b, _ in self.records) * 1e-3
        return len(self.records), t, float(sum((w[0] if isinstance(w, tuple) else w) for _, _, w in self.records))

    def summary2(self):
        return float(sum(w[1] for _, _, w in self.records if isinstance(w, tuple)))


GEMM_TIMER = None  # set to a KernelTimer to time psam_gemm_f16 launches
# further optional per-entry timers for bench.py's HBM-side roofline entries: name -> KernelTimer, work = ALGORITHMIC bytes
# of the launch (inputs read once + outputs written once). Names: layernorm, alp_sim, prob_argmax, ccl, attention_window,
# attention_global.
TIMERS = {}


def _tstart(name):
    t = TIMERS.get(name)
    return None if t is None else (t, t.start())


def _tstop(h, work):
    if h is not None:
        h[0].stop(h[1], work)

# packed qkv layout between the projection GEMM and the attention kernels: the reference's token-major [B,N,3,H,hd]
# (default) or head-major [3,H,B*N,hd] (PSAM_QKV_HEAD_MAJOR=1: contiguous per-head rows for the attention kernels, but
# scattered 160-byte stores for the GEMM; measured on MI355X at 16 slices: 108.8 / 109.2 vs 109.8 / 109.2 slices/s - a wash)
import os as _os
QKV_HEAD_MAJOR = _os.environ.get("PSAM_QKV_HEAD_MAJOR", "0") != "0"
# window layers: compute the decomposed rel-pos query terms inside the attention kernel (default) instead of a psam_relpos
# launch that writes them to HBM (PSAM_FUSE_WINDOW_RELPOS=0, kept for A/B)
FUSE_WINDOW_RELPOS = _os.environ.get("PSAM_FUSE_WINDOW_RELPOS", "1") != "0"
# global layers: the same inside the assembly global-attention kernel (round 5; attention_fused_relpos)
FUSE_GLOBAL_RELPOS = _os.environ.get("PSAM_FUSE_GLOBAL_RELPOS", "1") != "0"


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _req(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (protosam_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")


def _req_rows(t, dtype, name):
    """_req for a table that may have no rows (an empty tensor's strides say nothing, so only device and dtype are asked)"""
    if t is not None and t.is_cuda and t.dtype == dtype and t.numel() == 0:
        return
    _req(t, dtype, name)


def _req_aligned(t, nbytes, name):
    """The kernel behind reads or writes `t` in `nbytes` pieces from its base pointer: a view that starts inside a storage, off
    that boundary, is refused here, on the host, before any call into the library."""
    if t is not None and t.data_ptr() % nbytes:
        raise ValueError(f"{name}: data pointer must be {nbytes}-byte aligned (got a view at offset {t.data_ptr() % nbytes})")


def gemm(a, w, bias=None, out=None, epilogue=EPI_F16, resid=None, gamma=None, resid_mod=0, out_seg=0,
         out_seg_stride=0, out_seg_off=0, M=None, out16=None, stats=None, ln_mr=None, ln_s=None):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T + bias). a/w fp16 (K contiguous); out fp16 or fp32 by epilogue.
    Folded LayerNorm (psam_gemm_f16_ln): with EPI_F32, `out16` (fp16 [rows, N]) receives half(out) and `stats` (fp32
    [rows, N/64, 2]) per-row partial (sum, sum of squares); with EPI_F16 / EPI_GELU_F16, `ln_mr` (the 6-floats-per-row buffer of
    `ln_finalize`: fp32 (mean, rstd) [rows, 2], then the fp16 MFMA fragments of -mean [rows, 8]) and `ln_s` (the s_ext of
    `fold_layernorm`: fp32 [N], then fp16 fragments [N, 8]) apply out = act(rstd * (acc - mean * ln_s) + bias)."""
    _req(a, torch.float16, "a"); _req(w, torch.float16, "w")
    _req(bias, torch.float32, "bias"); _req(gamma, torch.float32, "gamma")
    _req(resid, torch.float16 if epilogue == EPI_RELU_F16 else torch.float32, "resid")   # epilogue 3 adds a half map
    a2 = a.reshape(-1, a.shape[-1]) if a.dim() != 2 else a
    if M is None:
        M = a2.shape[0]
    K = a2.shape[1]
    N = w.shape[0]
    assert w.shape[1] == K, (w.shape, K)
    odt = torch.float32 if epilogue == EPI_F32 else torch.float16
    if out is None:
        out = torch.empty((M, N), dtype=odt, device=a.device)
    _req(out, odt, "out")
    out2 = out.reshape(-1, out.shape[-1]) if out.dim() != 2 else out
    ldr = 0
    if resid is not None:
        r2 = resid.reshape(-1, resid.shape[-1]) if resid.dim() != 2 else resid
        ldr = r2.stride(0)
    fold = out16 is not None or stats is not None or ln_mr is not None
    if fold:
        _req(out16, torch.float16, "out16"); _req(stats, torch.float32, "stats")
        _req(ln_mr, torch.float32, "ln_mr"); _req(ln_s, torch.float32, "ln_s")
        # extended layouts of the assembly kernels (no size travels across the C ABI): ln_mr = ln_mr_buffer() as psam_ln_finalize
        # fills it (6 floats per row), ln_s = the s_ext of fold_layernorm (N floats + N fp16 fragments of 8 = 5 N floats), stats
        # [rows, N / 64, 2]
        if ln_mr is not None:
            assert ln_s is not None and ln_mr.numel() >= 6 * M and ln_s.numel() >= 5 * N, (ln_mr.numel(), 6 * M, ln_s.numel(), 5 * N)
        if stats is not None:
            assert stats.numel() >= M * (N // 64) * 2 and N % 64 == 0
        if out16 is not None:
            assert out16.shape[-1] >= N and out16.numel() >= M * N
    if epilogue == EPI_F32 and a.device.index not in _GEMM_WS:
        _ensure_gemm_workspace(a.device)
    t0 = GEMM_TIMER.start() if GEMM_TIMER is not None else None
    if fold:
        st = _lib.lib().psam_gemm_f16_ln(_ptr(a2), _ptr(w), _ptr(bias), _ptr(out2), _ptr(resid), _ptr(gamma), M, N, K,
                                        a2.stride(0), w.stride(0), out2.stride(0), ldr, resid_mod, out_seg,
                                        out_seg_stride, out_seg_off, epilogue, _ptr(out16),
                                        0 if out16 is None else out16.stride(-2), _ptr(stats), _ptr(ln_mr), _ptr(ln_s),
                                        _stream())
    else:
        st = _lib.lib().psam_gemm_f16(_ptr(a2), _ptr(w), _ptr(bias), _ptr(out2), _ptr(resid), _ptr(gamma), M, N, K,
                                     a2.stride(0), w.stride(0), out2.stride(0), ldr, resid_mod, out_seg,
                                     out_seg_stride, out_seg_off, epilogue, _stream())
    if t0 is not None:
        GEMM_TIMER.stop(t0, 2.0 * M * N * K, tag=(M, N, K, epilogue, 1 if fold else 0))
    _lib.check(st, "psam_gemm_f16_ln" if fold else "psam_gemm_f16")
    return out


_SPLITK = {}


def gemm_splitk_ranges(M, N, K):
    """K ranges `gemm_splitk_ln` would use for x[M,N] += a[M,K] w[N,K]^T on the current device, 0 when the shape does not pay (few 256-tiles
    and a long K are needed: one SAM ViT-H / ViT-L image through mlp.lin2). PSAM_GEMM_SPLITK_ASM=0 switches the path off (A/B)."""
    if _os.environ.get("PSAM_GEMM_SPLITK_ASM", "1") == "0":
        return 0
    key = (M, N, K, torch.cuda.current_device(), DISPATCH_EPOCH)
    if key not in _SPLITK:
        _SPLITK[key] = int(_lib.lib().psam_gemm_splitk_ranges(M, N, K))
    return _SPLITK[key]


def splitk_rows(M):
    """rows of one plane of gemm_splitk_ln's workspace: M rounded up to whole 256-row tiles"""
    return (M + 255) // 256 * 256


def gemm_splitk_ln(a, w, bias, x, ks, ws, ln_w=None, ln_b=None, eps=1e-6, out16=None):
    """x[M,N] (fp32, in place) += a[M,K] @ w[N,K]^T + bias as `ks` K ranges per 256-tile in one launch of the assembly kernel, then one
    pass that sums the ranges (fixed order) and writes out16 = LayerNorm(x) (or fp16(x) when ln_w is None). ws: fp32 scratch of at least
    ks * splitk_rows(M) * N elements owned by the caller (psam_gemm_f16_splitk_ln)."""
    _req(a, torch.float16, "a"); _req(w, torch.float16, "w"); _req(bias, torch.float32, "bias"); _req(x, torch.float32, "x")
    _req(ws, torch.float32, "ws"); _req(ln_w, torch.float32, "ln_w"); _req(ln_b, torch.float32, "ln_b"); _req(out16, torch.float16, "out16")
    M, K = a.shape
    N = w.shape[0]
    assert x.shape == (M, N) and w.shape[1] == K and ws.is_contiguous() and ws.numel() >= ks * splitk_rows(M) * N
    assert out16 is None or (out16.shape[0] >= M and out16.shape[-1] >= N)
    t0 = GEMM_TIMER.start() if GEMM_TIMER is not None else None
    st = _lib.lib().psam_gemm_f16_splitk_ln(_ptr(a), _ptr(w), _ptr(bias), _ptr(x), M, N, K, a.stride(0), w.stride(0), x.stride(0), ks,
                                           _ptr(ws), _ptr(ln_w), _ptr(ln_b), float(eps), _ptr(out16),
                                           0 if out16 is None else out16.stride(-2), _stream())
    if t0 is not None:
        GEMM_TIMER.stop(t0, 2.0 * M * N * K, tag=(M, N, K, EPI_F32, 0))
    _lib.check(st, "psam_gemm_f16_splitk_ln")
    return x


_CU_COUNT = {}


def fold_pays(M, D, device, min_fill=0.8):
    """Whether the folded LayerNorm is worth it for residual-stream GEMMs of M rows x D columns: its producer / consumer epilogues
    live in the 256x256-tile assembly kernels (and, slower, in the HIP kernels), so the launches must fill the CUs with 256-tiles -
    one slice at a time (80 tiles for 256 CUs) the half-tile kernels with separate LayerNorm passes are faster (85 vs 73 slices/s)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _CU_COUNT:
        _CU_COUNT[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return ((M + 255) // 256) * (D // 256) >= min_fill * _CU_COUNT[idx]


def ln_mr_buffer(M, device):
    """(mean, rstd) buffer of psam_ln_finalize: fp32 [M][2] followed by the fp16 MFMA fragments of -mean [M][8] (6 floats per row)."""
    return torch.empty(6 * M, dtype=torch.float32, device=device)


def ln_finalize(stats, M, D, eps, mr=None):
    """stats fp32 [rows, D/64, 2] (partial sums from a folded-LayerNorm producer GEMM) -> mr (see ln_mr_buffer): fp32 [rows, 2] =
    (mean, rstd), then fp16 [rows, 8] = {hi, hi, lo, 0 x 5} of -mean (the assembly GEMM's rank-1 correction operand)."""
    _req(stats, torch.float32, "stats")
    if mr is None:
        mr = ln_mr_buffer(M, stats.device)
    _req(mr, torch.float32, "mr")
    assert mr.numel() >= 6 * M and mr.is_contiguous()
    st = _lib.lib().psam_ln_finalize(_ptr(stats), M, D, float(eps), _ptr(mr), _stream())
    _lib.check(st, "psam_ln_finalize")
    return mr


def fold_layernorm(weight, bias, ln_weight, ln_bias):
    """One-time weight transform for a Linear that consumes LayerNorm(x): -> (W' fp16 = half(W * ln_weight), ln_s fp32 [N] =
    row sums of the ROUNDED W', bias' fp32 = bias + W . ln_bias), so that  Linear(LN(x)) = rstd * (x W'^T - mean * ln_s) + bias'."""
    W = weight.detach().float()
    Wp = (W * ln_weight.detach().float()[None, :]).half().contiguous()
    s = Wp.float().sum(1).contiguous()
    b = bias.detach().float() if bias is not None else torch.zeros(W.shape[0], dtype=torch.float32, device=W.device)
    # ln_s as psam_gemm_f16_ln takes it: fp32 [N], then the fp16 MFMA fragments {hi, lo, hi, 0 x 5} of s [N][8] (the assembly
    # GEMM subtracts mean_row * s_col with one rank-1 MFMA per block: hi * hi + lo * hi + hi * lo)
    hi = s.half()
    frag = torch.zeros((s.numel(), 8), dtype=torch.float16, device=s.device)
    frag[:, 0], frag[:, 1], frag[:, 2] = hi, (s - hi.float()).half(), hi
    s_ext = torch.cat([s, frag.reshape(-1).view(torch.float32)]).contiguous()
    return Wp, s_ext, (b + W @ ln_bias.detach().float()).contiguous()


def gemm_heads(a, w, bias, hd, out=None, M=None):
    """The packed qkv projection written head-major: half [N/hd, M, hd] (plane = which*H + h). a/w fp16, K contiguous."""
    _req(a, torch.float16, "a"); _req(w, torch.float16, "w"); _req(bias, torch.float32, "bias")
    a2 = a.reshape(-1, a.shape[-1]) if a.dim() != 2 else a
    if M is None:
        M = a2.shape[0]
    K, N = a2.shape[1], w.shape[0]
    assert w.shape[1] == K and N % hd == 0
    if out is None:
        out = torch.empty((N // hd, M, hd), dtype=torch.float16, device=a.device)
    _req(out, torch.float16, "out")
    assert out.is_contiguous() and out.numel() == M * N
    t0 = GEMM_TIMER.start() if GEMM_TIMER is not None else None
    st = _lib.lib().psam_gemm_f16_heads(_ptr(a2), _ptr(w), _ptr(bias), _ptr(out), M, N, K, a2.stride(0), w.stride(0), hd,
                                       _stream())
    if t0 is not None:
        GEMM_TIMER.stop(t0, 2.0 * M * N * K)
    _lib.check(st, "psam_gemm_f16_heads")
    return out


_GEMM_WS = {}     # device index -> scratch buffer registered with the library for that device
GEMM_WORKSPACE_MB = int(_os.environ.get("PSAM_GEMM_WORKSPACE_MB", "64"))


def _ensure_gemm_workspace(device):
    """Scratch for the split-K form of the fp32-residual GEMM (csrc/gemm.hip launch8kp_splitk): partial sums of one slice through
    fc2 are 63 MB. Allocated once per DEVICE from torch's allocator and registered with the library for that device (the library
    orders users on different streams through an event); 0 MB = no split-K."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _GEMM_WS:
        n = GEMM_WORKSPACE_MB << 20
        with torch.cuda.device(idx):
            buf = torch.empty(max(n, 16), dtype=torch.uint8, device=torch.device("cuda", idx))
            _lib.check(_lib.lib().psam_gemm_set_workspace(buf.data_ptr() if n else 0, n), "psam_gemm_set_workspace")
        _GEMM_WS[idx] = buf
        _GEMM_WS[None] = buf


DISPATCH_EPOCH = 0     # bumped by every set_* switch below: part of the key of captured graphs (a graph bakes the dispatch in)


def _bump_dispatch():
    global DISPATCH_EPOCH
    DISPATCH_EPOCH += 1


def dispatch_key():
    """what a captured graph of a forward depends on besides shapes and weights: every run-time dispatch switch of this module"""
    return (DISPATCH_EPOCH, QKV_HEAD_MAJOR, FUSE_WINDOW_RELPOS, FUSE_GLOBAL_RELPOS)


def gemm_set_tile(tile):
    """0 auto, 1 = 128x128 (HIP), 11 = 256x256 persistent (HIP), 15 / 16 / 17 = the assembly kernels (see csrc/gemm.hip pick_tile)."""
    _bump_dispatch()
    _lib.check(_lib.lib().psam_gemm_set_tile(int(tile)), "psam_gemm_set_tile")


def gemm_last_tile():
    """The tile the most recent gemm() call was dispatched to, after every fallback (0 before the first call)."""
    import ctypes
    t = ctypes.c_int(0)
    _lib.check(_lib.lib().psam_gemm_last_tile(ctypes.byref(t)), "psam_gemm_last_tile")
    return t.value


def gemm_set_option(name, value):
    """Dispatch switches of the GEMM: "asm", "half_tiles", "splitk", "nsplit" (0 / 1), "max_wgs" (cap on the persistent grids,
    0 = none), "mfma16" (0 / 1 / negative = the measured rule: tile 17 in place of tile 15) (see include/protosam_hip.h)."""
    _bump_dispatch()
    _lib.check(_lib.lib().psam_gemm_set_option(name.encode(), int(value)), "psam_gemm_set_option")


def gemm_asm_variant(v):
    """0 = the shipped assembly GEMM kernels; 1 = their traced forms (cycles per K-tile loop and per epilogue), which only a library
    built with `make GENFLAGS=--trace` holds: without them the next GEMM raises."""
    _bump_dispatch()
    _lib.check(_lib.lib().psam_gemm_asm_variant(int(v)), "psam_gemm_asm_variant")


def im2col(x, B, H, W, C, kh, kw, stride, dil, pad, ldo=None, out=None):
    """token-major half map [B, H*W, C] -> half [B*Ho*Wo, ldo] (column (ky*kw+kx)*C + c; zero K padding up to ldo)."""
    _req(x, torch.float16, "x")
    assert x.is_contiguous()
    Ho = (H + 2 * pad - dil * (kh - 1) - 1) // stride + 1 if stride > 0 else 0
    Wo = (W + 2 * pad - dil * (kw - 1) - 1) // stride + 1 if stride > 0 else 0
    if ldo is None:
        ldo = kh * kw * C
    if out is None:
        # sized from the same formulas as the library: what it would reject (status 1) must not reach the allocation
        if min(B, H, W, C, kh, kw, stride, dil) <= 0 or pad < 0 or Ho <= 0 or Wo <= 0:
            raise ValueError(f"im2col: no output for B={B} {H}x{W}x{C}, kernel {kh}x{kw} stride {stride} dil {dil} pad {pad}")
        out = torch.empty((B * Ho * Wo, ldo), dtype=torch.float16, device=x.device)
    st = _lib.lib().psam_im2col(_ptr(x), B, H, W, C, kh, kw, stride, dil, pad, ldo, _ptr(out), _stream())
    _lib.check(st, "psam_im2col")
    return out, Ho, Wo


def im2col_stem(img, ldo=192, out=None):
    """fp32 NCHW [B,3,H,W] -> half [B*Ho*Wo, ldo] patches of the 7x7 / stride 2 / pad 3 stem conv."""
    _req(img, torch.float32, "img")
    assert img.is_contiguous() and img.shape[1] == 3
    B, _, H, W = img.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((B * Ho * Wo, ldo), dtype=torch.float16, device=img.device)
    st = _lib.lib().psam_im2col_stem(_ptr(img), B, H, W, ldo, _ptr(out), _stream())
    _lib.check(st, "psam_im2col_stem")
    return out, Ho, Wo


def maxpool3x3s2(x, B, H, W, C, out=None):
    _req(x, torch.float16, "x")
    assert x.is_contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        if min(B, H, W, C) <= 0:      # (the library rejects these with status 1; no allocation from them)
            raise ValueError(f"maxpool3x3s2: no output for B={B} {H}x{W}x{C}")
        out = torch.empty((B * Ho * Wo, C), dtype=torch.float16, device=x.device)
    st = _lib.lib().psam_maxpool3x3s2(_ptr(x), B, H, W, C, _ptr(out), _stream())
    _lib.check(st, "psam_maxpool3x3s2")
    return out, Ho, Wo


def rotate_nearest(img, xg, yg, rt, crop_y, crop_x, out_h, out_w, out=None):
    """torchvision-style affine NEAREST resampling of fp32 [B,C,H,W] (protosam_amd/rotate.py); rt = host fp32 [3,2]."""
    _req(img, torch.float32, "img"); _req(xg, torch.float32, "xg"); _req(yg, torch.float32, "yg")
    assert img.is_contiguous() and rt.dtype == torch.float32 and rt.device.type == "cpu" and rt.is_contiguous()
    B, C, H, W = img.shape
    if out is None:
        out = torch.empty((B, C, out_h, out_w), dtype=torch.float32, device=img.device)
    _req(out, torch.float32, "out")
    assert out.is_contiguous() and out.numel() >= B * C * max(out_h, 0) * max(out_w, 0)
    st = _lib.lib().psam_rotate_nearest(_ptr(img), _ptr(out), _ptr(xg), _ptr(yg), rt.data_ptr(), B * C, H, W, crop_y, crop_x,
                                        out_h, out_w, _stream())
    _lib.check(st, "psam_rotate_nearest")
    return out


def resize_aa(img, oh, ow, out=None):
    """anti-aliased bilinear resize of fp32 [B,C,H,W] (aten _upsample_bilinear2d_aa semantics)."""
    _req(img, torch.float32, "img")
    assert img.is_contiguous()
    B, C, H, W = img.shape
    tmp = torch.empty((B * C, H, max(ow, 0)), dtype=torch.float32, device=img.device)
    if out is None:
        out = torch.empty((B, C, oh, ow), dtype=torch.float32, device=img.device)
    _req(out, torch.float32, "out")
    assert out.is_contiguous() and out.numel() >= B * C * max(oh, 0) * max(ow, 0)
    st = _lib.lib().psam_resize_aa(_ptr(img), _ptr(tmp), _ptr(out), B * C, H, W, oh, ow, _stream())
    _lib.check(st, "psam_resize_aa")
    return out


def layernorm(x, weight, bias, eps, out=None, out_dtype=torch.float16, out2=None, zero_tail_rows=0, M=None):
    """Row LayerNorm of fp32 x[M,D]. Optionally writes `zero_tail_rows` all-zero rows after row M-1."""
    _req(x, torch.float32, "x"); _req(weight, torch.float32, "weight"); _req(bias, torch.float32, "bias")
    x2 = x.reshape(-1, x.shape[-1]) if x.dim() != 2 else x
    if M is None:
        M = x2.shape[0]
    D = x2.shape[1]
    if out is None:
        out = torch.empty((M + zero_tail_rows, D), dtype=out_dtype, device=x.device)
    o2 = out.reshape(-1, out.shape[-1]) if out.dim() != 2 else out
    if out2 is not None:
        # the kernel writes out2 only next to an fp16 `out`, as fp32, and indexes it with the row stride of `out`
        if out.dtype != torch.float16:
            raise ValueError("out2: the second copy is written only next to an fp16 out (an fp32 out is that copy already)")
        if out2.dtype != torch.float32:
            raise ValueError(f"out2: expected torch.float32, got {out2.dtype}")
        _req(out2, torch.float32, "out2")
        y2 = out2.reshape(-1, out2.shape[-1]) if out2.dim() != 2 else out2
        if y2.shape[0] < M or y2.shape[1] < D or (y2.stride(0) != o2.stride(0) and M > 1):
            raise ValueError(f"out2: needs at least {M} rows of {D} columns with the row stride of out ({o2.stride(0)}), got "
                             f"{tuple(y2.shape)} with row stride {y2.stride(0)}")
    h = _tstart("layernorm")
    st = _lib.lib().psam_layernorm(_ptr(x2), _ptr(weight), _ptr(bias), _ptr(o2), _ptr(out2), M, D, x2.stride(0),
                                  o2.stride(0), float(eps), 0 if out.dtype == torch.float16 else 1,
                                  zero_tail_rows, _stream())
    _tstop(h, M * D * (4 + out.element_size()) + 8 * D)
    _lib.check(st, "psam_layernorm")
    return out


def attention(qkv, B, N, H, hd, scale, out=None, mode=0, rel_h=None, rel_w=None, relq=None, pad_row=None, gh=0, gw=0,
              ws=0, head_major=False, rpack=None):
    """qkv fp16 [B,N,3,H,hd] (packed as nn.Linear(dim,3*dim) emits it) or, head_major, [3,H,B*N,hd] (gemm_heads)
    -> fp16 [B,N,H*hd]. mode 1 (global + decomposed rel-pos) on a gh x gw token map: gw == 64 with rel_h / rel_w from `relpos` (or
    `rpack` alone where `attention_fused_relpos` says so); any other map with 1 <= gh, gw <= 64 with `rpack` alone
    (`pack_rel_tables`, global form) - the kernel computes the terms itself, both layouts."""
    _req(qkv, torch.float16, "qkv"); _req(rel_h, torch.float32, "rel_h"); _req(rel_w, torch.float32, "rel_w")
    _req(pad_row, torch.float16, "pad_row"); _req(relq, torch.float16, "relq"); _req(rpack, torch.float16, "rpack")
    assert qkv.is_contiguous()
    if out is None:
        out = torch.empty((B, N, H * hd), dtype=torch.float16, device=qkv.device)
    h = _tstart("attention_window" if mode == 2 else "attention_global")
    st = _lib.lib().psam_attention_f16(_ptr(qkv), _ptr(out), _ptr(rel_h), _ptr(rel_w), _ptr(relq), _ptr(rpack), _ptr(pad_row), B, N,
                                      H, hd, float(scale), mode, gh, gw, ws, 1 if head_major else 0, _stream())
    # qkv read once, out written once (fp16) + the global kernel's rel-pos terms (fp32 [B,H,N,64] x 2); work2 = FLOPs
    # 4*B*H*N*Nk*hd with Nk = the window's 196 keys (14x14) or all N keys
    nk = ws * ws if mode == 2 else N
    _tstop(h, (B * N * 4 * H * hd * 2 + (2 * B * H * N * 64 * 4 if (mode == 1 and rel_h is not None) else 0),
               4.0 * B * H * N * nk * hd))
    _lib.check(st, "psam_attention_f16")
    return out


_FUSED_RELPOS = {}


def attention_fused_relpos(B, N, H, hd, gh, gw):
    """True when attention(mode=1) takes `rpack` (pack_rel_tables, global form) in place of rel_h / rel_w: the assembly kernels
    psam_gattn_asm_*_fused compute the decomposed rel-pos terms themselves - no psam_relpos launch, no fp32 [B,H,N,64] x 2 round trip
    (PSAM_FUSE_GLOBAL_RELPOS=0: the two-kernel path, for A/B)."""
    if not FUSE_GLOBAL_RELPOS or QKV_HEAD_MAJOR:
        return False
    key = (B, N, H, hd, gh, gw, DISPATCH_EPOCH)
    if key not in _FUSED_RELPOS:
        _FUSED_RELPOS[key] = bool(_lib.lib().psam_attention_fused_relpos(B, N, H, hd, gh, gw))
    return _FUSED_RELPOS[key]


def attention_set_variant(v):
    """bit 0: V2 softmax in the global kernels (0 = round-1 serial form); bits 1-2: window kernel of the fused rel-pos path
    (0 attn_kernel, 1 wattn_kernel, 2 the persistent wattn_p_kernel); bit 3: the register-staged HIP global kernel; bit 4: the
    DMA-fed HIP global kernel everywhere (neither: the assembly global kernel where it applies, see include/protosam_hip.h); bit 5:
    mode 1 with `rpack` alone runs the any-map kernel at gw == 64 too.
    Default 5; for A/B and the equivalence tests."""
    _bump_dispatch()
    _lib.check(_lib.lib().psam_attention_set_variant(int(v)), "psam_attention_set_variant")


# what attention_last_kernel() reports (include/protosam_hip.h PSAM_ATTN_KERNEL_*): the family in the low byte, flags above it
ATTN_KERNEL_ATTN, ATTN_KERNEL_WATTN, ATTN_KERNEL_WATTN_P, ATTN_KERNEL_GATTN, ATTN_KERNEL_GATTN_ANY = 1, 2, 3, 4, 5
ATTN_KERNEL_ASM_REL, ATTN_KERNEL_ASM_FUSED, ATTN_KERNEL_ASM_NOREL, ATTN_KERNEL_ASM_WINDOW, ATTN_KERNEL_RELPOS = 6, 7, 8, 9, 10
ATTN_KERNEL_FAMILY = 0xff
ATTN_KERNEL_FULL, ATTN_KERNEL_STAGE64, ATTN_KERNEL_QT4, ATTN_KERNEL_V2 = 0x100, 0x200, 0x400, 0x800
ATTN_KERNEL_NAMES = {1: "attn_kernel", 2: "wattn_kernel", 3: "wattn_p_kernel", 4: "gattn_kernel", 5: "gattn_any_kernel",
                     6: "psam_gattn_asm_rel", 7: "psam_gattn_asm_fused", 8: "psam_gattn_asm_64_norel", 9: "psam_wattn_asm_80",
                     10: "relpos_mfma_kernel"}


def attention_last_kernel():
    """The kernel the most recent attention() / relpos() call launched, after every fallback (0 before the first call): an
    ATTN_KERNEL_* family, or-ed with FULL (the full-tile instance of the HIP global kernels), STAGE64 (gattn_any_kernel's 64-float
    stage), QT4 (relpos with four query tiles per wave), V2 (attn_kernel's V2 softmax)."""
    import ctypes
    k = ctypes.c_int(0)
    _lib.check(_lib.lib().psam_attention_last_kernel(ctypes.byref(k)), "psam_attention_last_kernel")
    return k.value


def attention_kernel_name(kid):
    """"gattn_any_kernel+full+stage64" for an id of attention_last_kernel(): what tests print and compare in their messages."""
    flags = [n for bit, n in ((ATTN_KERNEL_FULL, "full"), (ATTN_KERNEL_STAGE64, "stage64"), (ATTN_KERNEL_QT4, "qt4"),
                              (ATTN_KERNEL_V2, "v2")) if kid & bit]
    return "+".join([ATTN_KERNEL_NAMES.get(kid & ATTN_KERNEL_FAMILY, f"kernel {kid & ATTN_KERNEL_FAMILY}")] + flags)


def pack_rel_tables(rel_pos_h, rel_pos_w, windowed, hd):
    """fp32 (2K-1, hd) tables -> fp16 [2 (h,w)][2 (hi,lo)][RP][HDP] for psam_relpos (one-time weight packing)."""
    RP = 32 if windowed else 128
    HDP = (hd + 31) // 32 * 32
    out = torch.zeros((2, 2, RP, HDP), dtype=torch.float16, device=rel_pos_h.device)
    for t, R in enumerate((rel_pos_h, rel_pos_w)):
        R = R.detach().float()
        assert R.shape[0] <= RP and R.shape[1] == hd
        hi = R.half()
        lo = (R - hi.float()).half()
        out[t, 0, :R.shape[0], :hd] = hi
        out[t, 1, :R.shape[0], :hd] = lo
    if not windowed:
        return out.contiguous()
    # window form: the tables, then the constants of the 14 x 14 window geometry the window-attention kernel reads (csrc/attention.hip
    # wattn_kernel): the one-hot key-side fragments of the folded bias, [13 key tiles][64 lanes][8 k-slots], and a zero row
    return torch.cat([out.reshape(-1), _window_onehot_table().to(out.device), out.new_zeros(128)]).contiguous()


_ONEHOT = None


def _window_onehot_table(ws=14):
    """fp16 [13*64*8]: lane (li, g) of key tile T holds k-slots 8g..8g+7 of its key's row: 1 at slot kh and at slot 14 + kw, where
    key = 32 (T >> 1) + 8 (li >> 2) + 4 (T & 1) + (li & 3) (the MFMA row -> key map of the kernels), zero rows for keys >= 196."""
    global _ONEHOT
    if _ONEHOT is None:
        T = torch.arange(13).view(13, 1, 1)
        lane = torch.arange(64).view(1, 64, 1)
        e = torch.arange(8).view(1, 1, 8)
        li, g = lane & 15, lane >> 4
        key = (T >> 1) * 32 + (li >> 2) * 8 + (T & 1) * 4 + (li & 3)
        slot = g * 8 + e
        hot = ((slot == key // ws) | (slot == ws + key % ws)) & (key < ws * ws)
        _ONEHOT = hot.to(torch.float16).reshape(-1)
    return _ONEHOT


def relpos(qkv, rpack, B, N, H, hd, gw, K, windowed, scale, rel_h=None, rel_w=None, relq=None, head_major=False):
    """global: returns (rel_h, rel_w) fp32 [B,H,N,64]; windowed: returns relq fp16 [B,H,N,2,32] (zero-initialised once)."""
    _req(qkv, torch.float16, "qkv"); _req(rpack, torch.float16, "rpack")
    assert rpack.is_contiguous()
    if windowed:
        if relq is None:
            relq = torch.zeros((B, H, N, 2, 32), dtype=torch.float16, device=qkv.device)
    else:
        if rel_h is None:
            rel_h = torch.empty((B, H, N, 64), dtype=torch.float32, device=qkv.device)
        if rel_w is None:
            rel_w = torch.empty((B, H, N, 64), dtype=torch.float32, device=qkv.device)
    st = _lib.lib().psam_relpos(_ptr(qkv), _ptr(rpack), _ptr(rel_h), _ptr(rel_w), _ptr(relq), B, N, H, hd, gw, K,
                               1 if windowed else 0, float(scale), 1 if head_major else 0, _stream())
    _lib.check(st, "psam_relpos")
    return relq if windowed else (rel_h, rel_w)


# ---- ALP -----------------------------------------------------------------------------------------------
META_NBG, META_NFG, META_FGMODE, META_NCELL_FG = 0, 1, 2, 3


class AlpBank:
    """Fixed-capacity prototype bank + device-side counts (see csrc/alp.hip)."""

    def __init__(self, ncell, C, device):
        self.cap = ncell + 1
        self.C = C
        self.bank = torch.zeros((2 * self.cap, C), dtype=torch.float32, device=device)
        self.meta = torch.zeros(8, dtype=torch.int32, device=device)
        self.slot_bg = torch.empty(ncell, dtype=torch.int32, device=device)
        self.slot_fg = torch.empty(ncell, dtype=torch.int32, device=device)
        self.mres = None


def alp_bank(sup, ld, h, w, C, mask, pool_w, kernel_size, thresh=0.95, eps=1e-4, bank=None, force_mode=-1, bmask=None):
    """sup: fp32 token-major support features (row stride ld); mask fp32 [MH,MW] foreground mask."""
    _req(sup, torch.float32, "sup"); _req(mask, torch.float32, "mask")
    assert mask.dim() == 2 and mask.is_contiguous()
    ncell = (h // pool_w) * (w // pool_w)
    if bank is None:
        bank = AlpBank(ncell, C, sup.device)
    if bank.mres is None or bank.mres.numel() != 2 * h * w:
        bank.mres = torch.empty(2 * h * w, dtype=torch.float32, device=sup.device)
    if bmask is not None:
        _req(bmask, torch.float32, "bmask")
        assert bmask.shape == mask.shape and bmask.is_contiguous()
    st = _lib.lib().psam_alp_bank(_ptr(sup), ld, h, w, C, _ptr(mask), _ptr(bmask), mask.shape[0], mask.shape[1], pool_w,
                                 kernel_size,
                                 float(thresh), float(eps), _ptr(bank.bank), bank.cap, _ptr(bank.meta),
                                 _ptr(bank.slot_bg), _ptr(bank.slot_fg), _ptr(bank.mres), force_mode, _stream())
    _lib.check(st, "psam_alp_bank")
    return bank


def alp_sim(qry, q_bstride, ld, B, npix, C, bank, pred=None, part=None, eps=1e-4, sim_scale=20.0, which_only=-1):
    """qry fp32 token-major [B][npix, C] -> pred fp32 [B, 2, npix] (bg, fg)."""
    _req(qry, torch.float32, "qry")
    npt = (bank.cap + 63) // 64
    npix_pad = (npix + 63) // 64 * 64
    if part is None:
        part = torch.empty(2 * B * npt * npix_pad * 3, dtype=torch.float32, device=qry.device)
    if pred is None:
        pred = torch.empty((B, 2, npix), dtype=torch.float32, device=qry.device)
    h = _tstart("alp_sim")
    st = _lib.lib().psam_alp_sim(_ptr(qry), q_bstride, ld, B, npix, C, _ptr(bank.bank), bank.cap, _ptr(bank.meta),
                                float(eps), float(sim_scale), _ptr(part), _ptr(pred), which_only, _stream())
    # bytes: bank at capacity (an upper bound); FLOPs: every query pixel against 2 x cap prototypes on the fp32 MFMA (also an upper bound:
    # the kernel walks the occupied slots only) - this kernel's roof is the 157 TFLOP/s fp32-MFMA rate, not HBM
    _tstop(h, (B * npix * C * 4 + 2 * bank.cap * C * 4 + B * 2 * npix * 4, 2.0 * B * npix * C * 2 * bank.cap))
    _lib.check(st, "psam_alp_sim")
    return pred


def plan_alp_pairs(class_runs, B):
    """The entry list of `alp_sim_pairs` for C classes x B query slices (pure Python). class_runs[c]: the runs of class c in batch
    order, each (bg, fgs, n): the next n slices are matched against background bank `bg` and foreground banks `fgs` (one per shot;
    bg is the shots' merged bank when there are several). Banks are whatever handles the caller uses (indices into its bank list).
    Output planes follow FewShotSeg.class_scores' class-major layout [C, B, 2, ...]: plane (c*B + b)*2 + which. -> (entries, n_planes),
    entries = [(bank, b, which, plane), ...] ordered by plane, a plane's shots adjacent in shot order."""
    entries = []
    for c, runs in enumerate(class_runs):
        if sum(n for _, _, n in runs) != B or any(n < 0 for _, _, n in runs):
            raise ValueError(f"class {c}: the run counts {[n for _, _, n in runs]} do not sum to the {B} query slices")
        b0 = 0
        for bg, fgs, n in runs:
            if not fgs:
                raise ValueError(f"class {c}: a run without a foreground bank")
            for b in range(b0, b0 + n):
                plane = (c * B + b) * 2
                entries.append((bg, b, 0, plane))
                entries.extend((f, b, 1, plane + 1) for f in fgs)
            b0 += n
    return entries, 2 * B * len(class_runs)


def alp_sim_pairs(qry, q_bstride, ld, B, npix, C, banks, entries, n_planes, pred=None, part=None, eps=1e-4, sim_scale=20.0):
    """qry fp32 token-major [B][npix, C]; banks: AlpBank list; entries: [(bank index, slice b, which, plane), ...] (`plan_alp_pairs`)
    -> pred fp32 [n_planes, npix]: plane p = psam_alp_sim's (slice b, which) plane for the entry's bank, the element-wise max over
    the entries when several feed p (in their order). One small host-to-device copy of the entry table, one psam_alp_sim_pairs."""
    _req(qry, torch.float32, "qry")
    if not entries:
        raise ValueError("alp_sim_pairs: no entries")
    count = {}
    last = None
    for i, (k, b, which, plane) in enumerate(entries):
        if not (0 <= k < len(banks) and 0 <= b < B and which in (0, 1) and 0 <= plane < n_planes):
            raise ValueError(f"alp_sim_pairs: entry {i} {(k, b, which, plane)} is out of range")
        if plane != last and plane in count:
            raise ValueError(f"alp_sim_pairs: the entries of plane {plane} are not adjacent")
        count[plane] = count.get(plane, 0) + 1
        last = plane
    for bk in banks:
        if bk.C != C or bk.bank.device != qry.device:
            raise ValueError("alp_sim_pairs: every bank must have the query's channel count and device")
    rows, ngmax, direct = [], 1, True
    for k, b, which, plane in entries:
        bk = banks[k]
        ng = (bk.cap + 95) // 96
        ngmax = max(ngmax, ng)
        d = count[plane] == 1 and ng == 1
        direct = direct and d
        rows.append([bk.bank.data_ptr(), bk.meta.data_ptr(), bk.cap | (b << 32), (which | (2 if d else 0)) | (plane << 32)])
    npix_pad = (npix + 63) // 64 * 64
    if part is None and not direct:
        part = torch.empty(len(entries) * ngmax * npix_pad * 3, dtype=torch.float32, device=qry.device)
    assert part is None or part.numel() >= len(entries) * ngmax * npix_pad * 3
    if pred is None:
        pred = torch.empty((n_planes, npix), dtype=torch.float32, device=qry.device)
    _req(pred, torch.float32, "pred")
    assert pred.is_contiguous() and pred.numel() >= n_planes * npix
    # (a pinned staging tensor: the caching host allocator keeps it until the copy has run)
    tab = torch.tensor(rows, dtype=torch.int64).pin_memory().to(qry.device, non_blocking=True)
    h = _tstart("alp_sim")
    st = _lib.lib().psam_alp_sim_pairs(_ptr(qry), q_bstride, ld, npix, C, _ptr(tab), len(entries), ngmax, float(eps), float(sim_scale),
                                       _ptr(part), _ptr(pred), _stream())
    _tstop(h, (B * npix * C * 4 + sum(2 * bk.cap * C * 4 for bk in banks) + n_planes * npix * 4,
               sum(2.0 * npix * C * banks[k].cap for k, _, _, _ in entries)))
    _lib.check(st, "psam_alp_sim_pairs")
    return pred


# ---- resampling / packing ---------------------------------------------------------------------------------
def patchify_bilinear(img, S, P, Kpad, out=None):
    _req(img, torch.float32, "img")
    assert img.is_contiguous() and img.dim() == 4
    B, C, H, W = img.shape
    if out is None:
        out = torch.empty((B * (S // P) ** 2, Kpad), dtype=torch.float16, device=img.device)
    st = _lib.lib().psam_patchify_bilinear(_ptr(img), B, C, H, W, S, P, Kpad, _ptr(out), _stream())
    _lib.check(st, "psam_patchify_bilinear")
    return out


def bilinear_nchw(x, OH, OW, out=None):
    _req(x, torch.float32, "x")
    assert x.is_contiguous()
    planes = x.numel() // (x.shape[-1] * x.shape[-2])
    if out is None:
        out = torch.empty(tuple(x.shape[:-2]) + (OH, OW), dtype=torch.float32, device=x.device)
    st = _lib.lib().psam_bilinear_nchw(_ptr(x), planes, x.shape[-2], x.shape[-1], OH, OW, _ptr(out), _stream())
    _lib.check(st, "psam_bilinear_nchw")
    return out


def resize2d(x, OH, OW, mode, out=None):
    """F.interpolate of fp32 [..., H, W] planes: mode 0 bilinear, 1 bilinear align_corners=True, 2 nearest."""
    _req(x, torch.float32, "x")
    assert x.is_contiguous()
    planes = x.numel() // (x.shape[-1] * x.shape[-2])
    if out is None:
        out = torch.empty(tuple(x.shape[:-2]) + (OH, OW), dtype=torch.float32, device=x.device)
    st = _lib.lib().psam_resize2d(_ptr(x), planes, x.shape[-2], x.shape[-1], OH, OW, mode, _ptr(out), _stream())
    _lib.check(st, "psam_resize2d")
    return out


def prob_argmax(logits, OH, OW, prob=None, pred=None, fg_sum=None):
    _req(logits, torch.float32, "logits")
    assert logits.is_contiguous() and logits.dim() == 4 and logits.shape[1] == 2
    B = logits.shape[0]
    if prob is None:
        prob = torch.empty((B, 2, OH, OW), dtype=torch.float32, device=logits.device)
    if pred is None:
        pred = torch.empty((B, OH, OW), dtype=torch.uint8, device=logits.device)
    if OW % 4 == 0:                # the vector store path: 16 bytes of each probability row, 4 bytes of labels per lane
        _req_aligned(prob, 16, "prob"); _req_aligned(pred, 4, "pred")
    h = _tstart("prob_argmax")
    st = _lib.lib().psam_prob_argmax(_ptr(logits), B, logits.shape[2], logits.shape[3], OH, OW, _ptr(prob), _ptr(pred),
                                    _ptr(fg_sum), _stream())
    _tstop(h, B * (2 * logits.shape[2] * logits.shape[3] * 4 + OH * OW * 9))
    _lib.check(st, "psam_prob_argmax")
    return prob, pred


def prob2_argmax(scores, OH, OW, pred=None, pfg2=None, fg_sum=None, prob=None):
    """scores fp32 [P,2,IH,IW] -> (pred uint8 [P,OH,OW], pfg2 fp32 [P,OH,OW]) in one launch (psam_prob2_argmax): bilinear to
    (OH,OW) unless equal, softmax, argmax, then the foreground channel of a second softmax - the same bits as `prob_argmax` applied
    twice (ProtoMedSAM.py:176-187, util/utils.py:485). fg_sum int32 [P] is accumulated (zero it first); prob (optional, fp32
    [P,2,OH,OW]) receives the first softmax."""
    _req(scores, torch.float32, "scores")
    assert scores.is_contiguous() and scores.dim() == 4 and scores.shape[1] == 2
    P, dev = scores.shape[0], scores.device
    if pred is None:
        pred = torch.empty((P, OH, OW), dtype=torch.uint8, device=dev)
    if pfg2 is None:
        pfg2 = torch.empty((P, OH, OW), dtype=torch.float32, device=dev)
    _req(pfg2, torch.float32, "pfg2"); _req(prob, torch.float32, "prob")
    assert pred.dtype == torch.uint8 and pred.is_contiguous() and pred.numel() >= P * OH * OW
    assert pfg2.is_contiguous() and pfg2.numel() >= P * OH * OW
    assert prob is None or (prob.is_contiguous() and prob.numel() >= P * 2 * OH * OW)
    assert fg_sum is None or (fg_sum.dtype == torch.int32 and fg_sum.is_contiguous() and fg_sum.numel() >= P)
    h = _tstart("prob2_argmax")
    st = _lib.lib().psam_prob2_argmax(_ptr(scores), P, scores.shape[2], scores.shape[3], OH, OW, _ptr(pred), _ptr(pfg2),
                                      _ptr(fg_sum), _ptr(prob), _stream())
    _tstop(h, P * (2 * scores.shape[2] * scores.shape[3] * 4 + OH * OW * (5 + (8 if prob is not None else 0))))
    _lib.check(st, "psam_prob2_argmax")
    return pred, pfg2


def scores_prob_argmax(scores, IH, IW, OH, OW, prob=None, pred=None, fg_sum=None):
    """scores fp32 [P,2,g,g] (grid resolution) -> (prob fp32 [P,2,OH,OW], pred uint8 [P,OH,OW]) in one launch
    (psam_scores_prob_argmax): bilinear to the image size (IH,IW), bilinear to (OH,OW) unless equal, softmax, argmax - the bits of
    `prob_argmax(bilinear_nchw(scores, IH, IW), OH, OW)` without the [P,2,IH,IW] intermediate. fg_sum int32 [P] is accumulated
    (zero it first)."""
    _req(scores, torch.float32, "scores")
    assert scores.is_contiguous() and scores.dim() == 4 and scores.shape[1] == 2
    P, dev = scores.shape[0], scores.device
    if prob is None:
        prob = torch.empty((P, 2, OH, OW), dtype=torch.float32, device=dev)
    if pred is None:
        pred = torch.empty((P, OH, OW), dtype=torch.uint8, device=dev)
    _req(prob, torch.float32, "prob")
    assert prob.is_contiguous() and prob.numel() >= P * 2 * OH * OW
    assert pred.dtype == torch.uint8 and pred.is_cuda and pred.is_contiguous() and pred.numel() >= P * OH * OW
    assert fg_sum is None or (fg_sum.dtype == torch.int32 and fg_sum.is_cuda and fg_sum.is_contiguous() and fg_sum.numel() >= P)
    h = _tstart("scores_prob_argmax")
    st = _lib.lib().psam_scores_prob_argmax(_ptr(scores), P, scores.shape[2], scores.shape[3], IH, IW, OH, OW, _ptr(prob),
                                            _ptr(pred), _ptr(fg_sum), _stream())
    _tstop(h, P * (2 * scores.shape[2] * scores.shape[3] * 4 + OH * OW * 9))
    _lib.check(st, "psam_scores_prob_argmax")
    return prob, pred


def broadcast_rows(row, out, B, stride, off):
    _req(row, torch.float32, "row"); _req(out, torch.float32, "out")
    st = _lib.lib().psam_broadcast_rows(_ptr(row), row.numel(), _ptr(out), B, stride, off, _stream())
    _lib.check(st, "psam_broadcast_rows")


def minmax(x, B, mm=None):
    _req(x, torch.float32, "x")
    assert x.is_contiguous()
    if mm is None:
        mm = torch.empty(2 * B, dtype=torch.int32, device=x.device)
    st = _lib.lib().psam_minmax(_ptr(x), B, x.numel() // B, _ptr(mm), _stream())
    _lib.check(st, "psam_minmax")
    return mm


def sam_patchify(img, mm, S, P, mean3, std3, quantise=True, out=None, u8out=None):
    import ctypes
    _req(img, torch.float32, "img")
    assert img.is_contiguous() and img.shape[-1] == S and img.shape[-2] == S
    B = img.shape[0]
    if out is None:
        out = torch.empty((B * (S // P) ** 2, 3 * P * P), dtype=torch.float16, device=img.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean3])
    s = (ctypes.c_float * 3)(*[float(v) for v in std3])
    st = _lib.lib().psam_sam_patchify(_ptr(img), _ptr(mm), B, S, P, m, s, 1 if quantise else 0, _ptr(out), _ptr(u8out),
                                     _stream())
    _lib.check(st, "psam_sam_patchify")
    return out


def im2col3x3(x, B, H, W, C, out=None):
    _req(x, torch.float16, "x")
    assert x.is_contiguous()
    if out is None:
        out = torch.empty((B * H * W, 9 * C), dtype=torch.float16, device=x.device)
    st = _lib.lib().psam_im2col3x3(_ptr(x), B, H, W, C, _ptr(out), _stream())
    _lib.check(st, "psam_im2col3x3")
    return out


def cast_f16(x, out=None):
    _req(x, torch.float32, "x")
    assert x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _req_aligned(x, 16, "x"); _req_aligned(out, 16, "out")
    st = _lib.lib().psam_cast_f16(_ptr(x), _ptr(out), x.numel(), _stream())
    _lib.check(st, "psam_cast_f16")
    return out


def cast_f32(x, out=None):
    """fp16 -> fp32 (the reference-width encoder mode: the attention output on its way to psam_gemm_f32x3)."""
    _req(x, torch.float16, "x")
    assert x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _req(out, torch.float32, "out")
    _req_aligned(x, 16, "x"); _req_aligned(out, 16, "out")
    st = _lib.lib().psam_cast_f32(_ptr(x), _ptr(out), x.numel(), _stream())
    _lib.check(st, "psam_cast_f32")
    return out


def gelu_f32_(x):
    """nn.GELU (erf form) in place on fp32 (the reference-width encoder mode, between lin1 and lin2)."""
    _req(x, torch.float32, "x")
    assert x.is_contiguous()
    _req_aligned(x, 16, "x")
    st = _lib.lib().psam_gelu_f32(_ptr(x), x.numel(), _stream())
    _lib.check(st, "psam_gelu_f32")
    return x


def split_f16(x, hi=None, lo=None, write_hi=True):
    """fp32 x -> (hi = half(x), lo = half(x - hi)); write_hi=False: `hi` already holds half(x) (a folded-LayerNorm GEMM wrote it)."""
    _req(x, torch.float32, "x")
    assert x.is_contiguous()
    if hi is None:
        assert write_hi
        hi = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    if lo is None:
        lo = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    _req(hi, torch.float16, "hi"); _req(lo, torch.float16, "lo")
    _req_aligned(x, 16, "x"); _req_aligned(hi, 16, "hi"); _req_aligned(lo, 16, "lo")
    st = _lib.lib().psam_split_f16(_ptr(x), _ptr(hi), _ptr(lo), x.numel(), 1 if write_hi else 0, _stream())
    _lib.check(st, "psam_split_f16")
    return hi, lo


def split_weight_f16(w, scale=1.0):
    """fp32 weight -> (hi, lo) fp16 pair of w * scale (one-time packing; scale a power of two: gemm_f32x3 undoes it)."""
    w = w.detach().float()
    # |w * scale| must stay inside fp16 (hi = inf, lo = -inf, NaN products otherwise): halve the scale until it does
    amax = float(w.abs().max()) if w.numel() else 0.0
    if not amax < float("inf"):
        raise ValueError("split_weight_f16: non-finite weight")
    if amax * scale >= 6.0e4:
        raise ValueError(f"split_weight_f16: max |w| = {amax:.4g} times the scale {scale:g} overflows fp16; use `split_scale_for(w)`")
    w = w * scale
    hi = w.half()
    return hi.contiguous(), (w - hi.float()).half().contiguous()


def split_scale_for(w, want=256.0):
    """the largest power of two <= `want` that keeps max |w| * scale below the fp16 range (gemm_f32x3's weight scale)"""
    amax = float(w.detach().abs().max()) if w.numel() else 0.0
    s = float(want)
    while s > 2.0 ** -14 and amax * s >= 6.0e4:
        s *= 0.5
    return s


X3_WEIGHT_SCALE = 256.0      # gemm_f32x3: weights are split as w * 2^8 (a lo half is a normal fp16 down to |w| = 5e-4; |w| < 255)


# ---- SAM prompt encoder / mask decoder -----------------------------------------------------------------------
def small_linear(x, W, b=None, out=None, act=0, resid=None, x2=None, G=1, M=None, N=None, K=None, xg=0, wg=0, bg=0, yg=0,
                 ldx=None, ldy=None):
    """Grouped fp32 y[g,m,:] = act(x[g,m,:] @ W[g]^T + b[g]) (+ resid). Defaults: one group, x [M,K], W [N,K]."""
    _req(x, torch.float32, "x"); _req(W, torch.float32, "W"); _req(b, torch.float32, "b")
    _req(resid, torch.float32, "resid")
    if M is None:
        M = x.shape[-2]
    if K is None:
        K = x.shape[-1]
    if N is None:
        N = W.shape[-2]
    if ldx is None:
        ldx = x.stride(-2)
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float32, device=x.device)
    if ldy is None:
        ldy = out.stride(-2)
    _req(x2, torch.float32, "x2")
    st = _lib.lib().psam_small_linear(_ptr(x), _ptr(x2), _ptr(W), _ptr(b), _ptr(resid), _ptr(out), G, M, N, K, xg, wg, bg, yg,
                                     ldx, ldy, act, _stream())
    _lib.check(st, "psam_small_linear")
    return out


def small_attention(q, k, v, out, B, Tq, Tk, NH, hd, ldq, ldk, ldv, ldo):
    q16 = q.dtype == torch.float16
    _req(k, torch.float32, "k"); _req(v, torch.float32, "v")
    assert out.dtype == q.dtype
    st = _lib.lib().psam_small_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Tq, Tk, NH, hd, ldq, ldk, ldv, ldo,
                                        1 if q16 else 0, _stream())
    _lib.check(st, "psam_small_attention")
    return out


MAX_PROMPT_TOKENS = 256     # tokens per prompt set (5 output tokens + sparse prompts): PSAM_MAX_PROMPT_TOKENS of the C side


def token_attention(q, k, v, out, B, Tq, Tk, NH, hd, ldq, ldk, ldv, ldo):
    """small_attention for up to MAX_PROMPT_TOKENS keys (psam_token_attention: the keys in chunks of 16 through LDS)."""
    q16 = q.dtype == torch.float16
    _req(k, torch.float32, "k"); _req(v, torch.float32, "v")
    assert out.dtype == q.dtype
    st = _lib.lib().psam_token_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Tq, Tk, NH, hd, ldq, ldk, ldv, ldo,
                                        1 if q16 else 0, _stream())
    _lib.check(st, "psam_token_attention")
    return out


def prompt_attention(q, k, v, out, B, Tq, Tk, NH, hd, ldq, ldk, ldv, ldo):
    """attention over the Tk tokens of a prompt set: small_attention up to 16 keys (scores in registers), token_attention above"""
    return (small_attention if Tk <= 16 else token_attention)(q, k, v, out, B, Tq, Tk, NH, hd, ldq, ldk, ldv, ldo)


def t2i_split(B, NH, T, Nk, n_cu=256):
    """into how many key ranges a token-to-image attention launch is split (PSAM_T2I_SPLIT: "auto", or a number to force): the unsplit
    launch has B * NH * ceil(T / 16) workgroups whose waves each walk all keys, 64 dependent round trips"""
    mode = _os.environ.get("PSAM_T2I_SPLIT", "auto")
    if T > MAX_PROMPT_TOKENS or Nk < 512 or mode in ("0", "1"):        # (a forced count of 1 is one range: no split)
        return 1
    if mode != "auto":
        return max(1, min(16, Nk // 256, int(mode)))
    return max(1, min(16, Nk // 256, n_cu // (B * NH * max(1, (T + 15) // 16))))


def t2i_attention(q, K, V, out, B, T, Nk, NH, head_major=False, split=None):
    """head_major: K / V are [B][NH][Nk][16] (gemm_f32(..., heads=(Nk, 16))) instead of token-major [B][Nk][NH * 16].
    split = (S, part): the keys in S ranges per (prompt set, head), merged by a second small launch - part fp32 scratch of at least
    B * NH * S * T * 18 elements."""
    _req(q, torch.float32, "q"); _req(K, K.dtype, "K"); _req(V, K.dtype, "V"); _req(out, torch.float32, "out")
    assert K.dtype in (torch.float16, torch.float32)
    if q.shape[-1] != NH * 16:     # the kernels (and the head-major K / V layout) are written for 16-wide heads: C = NH * 16
        raise ValueError(f"psam_t2i_attention: head size {q.shape[-1]}/{NH} is not 16 (SAM: 128 channels, 8 heads)")
    flags = (1 if K.dtype == torch.float32 else 0) | (2 if head_major else 0)
    if split is not None and split[0] > 1:
        S, part = split
        _req(part, torch.float32, "part")
        assert part.numel() >= B * NH * S * T * 18
        st = _lib.lib().psam_t2i_attention_split(_ptr(q), _ptr(K), _ptr(V), _ptr(out), B, T, Nk, NH, flags, S, _ptr(part), _stream())
        _lib.check(st, "psam_t2i_attention_split")
        return out
    st = _lib.lib().psam_t2i_attention(_ptr(q), _ptr(K), _ptr(V), _ptr(out), B, T, Nk, NH, flags, _stream())
    _lib.check(st, "psam_t2i_attention")
    return out


def small_linear_splitk(x, W, b, resid, out, parts, ks):
    """out[M,N] = x[M,K] @ W[N,K]^T + b (+ resid) as `ks` K ranges in one launch + a fixed-order sum (few rows, long contraction);
    parts: fp32 scratch of at least ks * M * N elements."""
    _req(x, torch.float32, "x"); _req(W, torch.float32, "W"); _req(b, torch.float32, "b"); _req(resid, torch.float32, "resid")
    _req(out, torch.float32, "out"); _req(parts, torch.float32, "parts")
    M, K = x.shape[-2], x.shape[-1]
    N = W.shape[0]
    assert W.shape[1] == K and W.is_contiguous() and parts.numel() >= ks * M * N and out.stride(-1) == 1
    assert resid is None or resid.stride(-2) == out.stride(-2)
    st = _lib.lib().psam_small_linear_splitk(_ptr(x), _ptr(W), _ptr(b), _ptr(resid), _ptr(out), _ptr(parts), M, N, K, ks, x.stride(-2),
                                            out.stride(-2), _stream())
    _lib.check(st, "psam_small_linear_splitk")
    return out


def gemm_f32(a, w, bias=None, out=None, resid=None, a2=None, a2_mod=0, heads=None):
    """out[M,N] = (a[M,K] [+ a2[m % a2_mod]]) @ w[N,K]^T + bias [+ resid]; everything fp32 (exact-fp32 MFMA).
    heads = (nk, hd): the result is written head-major, out fp32 [M / nk][N / hd][nk][hd] (no residual)."""
    if heads is not None:
        _req(a, torch.float32, "a"); _req(w, torch.float32, "w"); _req(bias, torch.float32, "bias"); _req(a2, torch.float32, "a2")
        nk, hd = heads
        M, K = a.shape
        N = w.shape[0]
        assert resid is None and out is not None and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= M * N
        assert a2 is None or (a2.stride(0) == a.stride(0) and a2_mod > 0)
        st = _lib.lib().psam_gemm_f32_heads(_ptr(a), _ptr(a2), a2_mod, _ptr(w), _ptr(bias), _ptr(out), M, N, K, a.stride(0), w.stride(0),
                                           nk, hd, _stream())
        _lib.check(st, "psam_gemm_f32_heads")
        return out
    _req(a, torch.float32, "a"); _req(w, torch.float32, "w"); _req(bias, torch.float32, "bias")
    _req(resid, torch.float32, "resid"); _req(a2, torch.float32, "a2")
    assert a.dim() == 2 and w.dim() == 2 and w.shape[1] == a.shape[1]
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _req(out, torch.float32, "out")
    assert out.shape == (M, N) and (resid is None or (resid.shape == (M, N) and resid.stride(0) == out.stride(0)))
    assert a2 is None or (a2.stride(0) == a.stride(0) and a2_mod > 0)
    st = _lib.lib().psam_gemm_f32(_ptr(a), _ptr(a2), a2_mod, _ptr(w), _ptr(bias), _ptr(resid), _ptr(out), M, N, K,
                                 a.stride(0), w.stride(0), out.stride(0), _stream())
    _lib.check(st, "psam_gemm_f32")
    return out


def gemm_f32x3(a, w_split, bias=None, out=None, resid=None, a2=None, a2_mod=0, heads=None):
    """gemm_f32 at fp32 accuracy on the fp16 matrix pipe: w_split = split_weight_f16(w) - the (hi, lo) fp16 halves of the fp32 weight;
    a (fp32) is split on chip, three MFMA products per k step, fp32 accumulation (psam_gemm_f32x3). heads = (nk, hd) as gemm_f32.
    w_split may carry a third element: the power of two the weight was scaled by before the split (default 1)."""
    wh, wl = w_split[0], w_split[1]
    wscale = float(w_split[2]) if len(w_split) > 2 else 1.0
    _req(a, torch.float32, "a"); _req(wh, torch.float16, "wh"); _req(wl, torch.float16, "wl"); _req(bias, torch.float32, "bias")
    _req(resid, torch.float32, "resid"); _req(a2, torch.float32, "a2")
    assert a.dim() == 2 and wh.dim() == 2 and wh.shape == wl.shape and wh.shape[1] == a.shape[1] and wh.stride(0) == wl.stride(0)
    M, K = a.shape
    N = wh.shape[0]
    assert a2 is None or (a2.stride(0) == a.stride(0) and a2_mod > 0)
    nk, hd = heads if heads is not None else (0, 0)
    if heads is not None:
        assert resid is None and out is not None and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= M * N
        ldo = N
    else:
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=a.device)
        _req(out, torch.float32, "out")
        assert out.shape == (M, N) and (resid is None or (resid.shape == (M, N) and resid.stride(0) == out.stride(0)))
        ldo = out.stride(0)
    st = _lib.lib().psam_gemm_f32x3(_ptr(a), _ptr(a2), a2_mod, _ptr(wh), _ptr(wl), _ptr(bias), _ptr(resid), _ptr(out), M, N, K,
                                   a.stride(0), wh.stride(0), ldo, nk, hd, 1.0 / wscale, _stream())
    _lib.check(st, "psam_gemm_f32x3")
    return out


def ln_pe(x, pe, M, y32=None, y16=None, ype16=None, add_vec=None, w=None, b=None, in_mod=0, pe_mod=4096, eps=1e-5,
          img_of_prompt=None):
    _req(x, torch.float32, "x"); _req(pe, torch.float32, "pe"); _req(img_of_prompt, torch.int32, "img_of_prompt")
    st = _lib.lib().psam_ln_pe(_ptr(x), _ptr(add_vec), _ptr(w), _ptr(b), _ptr(pe), _ptr(y32), _ptr(y16), _ptr(ype16), M,
                              in_mod, pe_mod, float(eps), 1 if w is not None else 0, _ptr(img_of_prompt), _stream())
    _lib.check(st, "psam_ln_pe")


def dense_pe(G, gh, gw):
    _req(G, torch.float32, "G")
    pe = torch.empty((gh * gw, 256), dtype=torch.float32, device=G.device)
    st = _lib.lib().psam_dense_pe(_ptr(G), gh, gw, _ptr(pe), _stream())
    _lib.check(st, "psam_dense_pe")
    return pe


def prompt_tokens(coords, labels, G, type_emb, out_tok, B, Ns, img_size, tokens=None):
    _req(coords, torch.float32, "coords"); _req(labels, torch.int32, "labels")
    if tokens is None:
        tokens = torch.empty((B, 5 + Ns, 256), dtype=torch.float32, device=G.device)
    st = _lib.lib().psam_prompt_tokens(_ptr(coords), _ptr(labels), _ptr(G), _ptr(type_emb), _ptr(out_tok), B, Ns,
                                      float(img_size), _ptr(tokens), _stream())
    _lib.check(st, "psam_prompt_tokens")
    return tokens


def upscale_tail(u1, lnw, lnb, W2r, b2, hyper, B, g, masks=None):
    _req(u1, torch.float32, "u1"); _req(hyper, torch.float32, "hyper")
    if masks is None:
        masks = torch.empty((B, 4, 4 * g, 4 * g), dtype=torch.float32, device=u1.device)
    st = _lib.lib().psam_upscale_tail(_ptr(u1), _ptr(lnw), _ptr(lnb), _ptr(W2r), _ptr(b2), _ptr(hyper), _ptr(masks), B, g,
                                     _stream())
    _lib.check(st, "psam_upscale_tail")
    return masks


def mask_upsample(low, MID, variant, out=None):
    _req(low, torch.float32, "low")
    assert low.is_contiguous()
    IN = low.shape[-1]
    planes = low.numel() // (IN * IN)
    if out is None:
        out = torch.empty(tuple(low.shape[:-2]) + (MID, MID), dtype=torch.float32, device=low.device)
    st = _lib.lib().psam_mask_upsample(_ptr(low), planes, IN, MID, variant, _ptr(out), _stream())
    _lib.check(st, "psam_mask_upsample")
    return out


def mask_union(low, sel, MID, OUT, variant, thr=0.0, pred=None):
    _req(low, torch.float32, "low")
    assert low.is_contiguous() and low.dim() == 4
    B, C, IN, _ = low.shape
    if pred is None:
        pred = torch.empty((OUT, OUT), dtype=torch.float32, device=low.device)
    st = _lib.lib().psam_mask_union(_ptr(low), B, C, sel, IN, MID, OUT, variant, float(thr), _ptr(pred), _stream())
    _lib.check(st, "psam_mask_union")
    return pred


def mask_union_seg(low, sel, segs, nout, MID, OUT, variant, thr, out=None):
    """Every output mask of a batch in one launch (psam_mask_union_seg): low fp32 [Pm,C,IN,IN] (None when Pm = 0), segs int32
    [nseg,3] device tensor of (first prompt, prompt count, output index) -> out uint8 [nout,OUT,OUT], out[o] = what
    `mask_union(low[first:first+count], sel, MID, OUT, variant, thr).to(torch.uint8)` gives (zeros for a count of 0). Outputs no
    segment names are left as they are."""
    assert segs.dtype == torch.int32 and segs.is_cuda and segs.is_contiguous() and segs.dim() == 2 and segs.shape[1] == 3
    if low is not None:
        _req(low, torch.float32, "low")
        assert low.is_contiguous() and low.dim() == 4
        Pm, C, IN, _ = low.shape
    else:
        Pm, C, IN = 0, sel + 1, 1
    if out is None:
        out = torch.empty((nout, OUT, OUT), dtype=torch.uint8, device=segs.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= nout * OUT * OUT
    nseg = segs.shape[0]
    if nseg == 0:
        return out
    h = _tstart("mask_union_seg")
    st = _lib.lib().psam_mask_union_seg(_ptr(low), Pm, C, sel, IN, _ptr(segs), nseg, nout, MID, OUT, variant, float(thr), _ptr(out),
                                        _stream())
    _tstop(h, nseg * OUT * OUT)
    _lib.check(st, "psam_mask_union_seg")
    return out


def mask_downscale(masks, wts, g, eps=1e-6, out=None):
    """PromptEncoder.mask_downscaling: masks fp32 [n,4g,4g] -> dense embeddings fp32 [n, g*g, 256] (token-major)."""
    _req(masks, torch.float32, "masks"); _req(wts, torch.float32, "wts")
    assert masks.is_contiguous() and masks.shape[-1] == 4 * g and masks.shape[-2] == 4 * g and wts.numel() == 4684
    n = masks.numel() // (16 * g * g)
    if out is None:
        out = torch.empty((n, g * g, 256), dtype=torch.float32, device=masks.device)
    st = _lib.lib().psam_mask_downscale(_ptr(masks), _ptr(wts), n, g, float(eps), _ptr(out), _stream())
    _lib.check(st, "psam_mask_downscale")
    return out


def mask_stats(low, first, nsel, MID, H, W, variant, thr=0.0, off=1.0, stats=None):
    """int32 [B*nsel, 8] = {n(v>thr+off), n(v>thr-off), n(v>thr), min_x, min_y, max_x, max_y, 0} per selected plane of
    low [B,C,IN,IN] over the [H,W] corner of its MID x MID up-sampling."""
    _req(low, torch.float32, "low")
    assert low.is_contiguous() and low.dim() == 4
    B, C, IN, _ = low.shape
    if stats is None:
        stats = torch.empty((B * nsel, 8), dtype=torch.int32, device=low.device)
    st = _lib.lib().psam_mask_stats(_ptr(low), B, C, first, nsel, IN, MID, H, W, variant, float(thr), float(off),
                                   _ptr(stats), _stream())
    _lib.check(st, "psam_mask_stats")
    return stats


def plane_stats(planes, thr=0.0, off=1.0, binarize=True, stats=None, out=None):
    """planes fp32 [n,H,W] -> (stats int32 [n,8] as mask_stats, uint8 [n,H,W] = plane > thr or None)."""
    _req(planes, torch.float32, "planes")
    assert planes.is_contiguous() and planes.dim() == 3
    n, H, W = planes.shape
    if stats is None:
        stats = torch.empty((n, 8), dtype=torch.int32, device=planes.device)
    if out is None and binarize:
        out = torch.empty((n, H, W), dtype=torch.uint8, device=planes.device)
    assert stats.dtype == torch.int32 and stats.is_contiguous() and stats.numel() >= n * 8
    assert out is None or (out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= n * H * W)
    st = _lib.lib().psam_plane_stats(_ptr(planes), n, H, W, float(thr), float(off), _ptr(stats), _ptr(out), _stream())
    _lib.check(st, "psam_plane_stats")
    return stats, out


def mask_binarize(low, idx, MID, H, W, variant, thr=0.0, label=None, out=None):
    """uint8 [n,H,W] = upsample(low.view(-1,IN,IN)[idx[i]]) > thr; with `label` uint8 [H,W] also int64 [n,3] {tp,fp,fn}."""
    _req(low, torch.float32, "low"); _req(idx, torch.int32, "idx")
    assert low.is_contiguous() and idx.is_contiguous()
    IN, n = low.shape[-1], idx.numel()
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.uint8, device=low.device)
    counts = None
    if label is not None:
        _req(label, torch.uint8, "label")
        assert label.is_contiguous() and tuple(label.shape) == (H, W)
        counts = torch.empty((n, 3), dtype=torch.int64, device=low.device)
    st = _lib.lib().psam_mask_binarize(_ptr(low), _ptr(idx), n, IN, MID, H, W, variant, float(thr), _ptr(out),
                                      _ptr(label), _ptr(counts), _stream())
    _lib.check(st, "psam_mask_binarize")
    return out, counts


def mask_stats_resized(low, first, nsel, MID, in_size, out_size, variant, thr=0.0, off=1.0, stats=None, score=None,
                       score_thresh=0.0):
    """mask_stats for an image that is not at the model's input size: int32 [B*nsel, 8] over the out_size = (OH, OW) image, whose
    pixels are the second resize of postprocess_masks - from the in_size = (ih, iw) corner of the MID x MID up-sampling - computed
    on the fly from low [B,C,IN,IN]. The bits of mask_upsample -> crop -> resize2d -> plane_stats. With `score` fp32 [B,C] (the
    decoder's predicted IoUs) and score_thresh > 0, planes whose score is not above float32(score_thresh) are skipped and keep the
    empty-mask row: the generator's first filter drops them whatever their statistics."""
    _req(low, torch.float32, "low")
    assert low.is_contiguous() and low.dim() == 4
    B, C, IN, _ = low.shape
    (ih, iw), (OH, OW) = (int(v) for v in in_size), (int(v) for v in out_size)
    if stats is None:
        stats = torch.empty((B * nsel, 8), dtype=torch.int32, device=low.device)
    assert stats.dtype == torch.int32 and stats.is_contiguous() and stats.numel() >= B * nsel * 8
    if score is not None and score_thresh > 0.0:
        _req(score, torch.float32, "score")
        assert score.is_contiguous() and tuple(score.shape) == (B, C)
        st = _lib.lib().psam_mask_stats_resized_scored(_ptr(low), _ptr(score), float(score_thresh), B, C, first, nsel, IN, MID, ih, iw,
                                                       OH, OW, variant, float(thr), float(off), _ptr(stats), _stream())
        _lib.check(st, "psam_mask_stats_resized_scored")
        return stats
    st = _lib.lib().psam_mask_stats_resized(_ptr(low), B, C, first, nsel, IN, MID, ih, iw, OH, OW, variant, float(thr), float(off),
                                            _ptr(stats), _stream())
    _lib.check(st, "psam_mask_stats_resized")
    return stats


def mask_binarize_resized(low, idx, MID, in_size, out_size, variant, thr=0.0, label=None, out=None, origin=(0, 0)):
    """mask_binarize with the second resize of postprocess_masks: mask i = (plane idx[i] of low.view(-1,IN,IN), up-sampled to MID,
    cropped to in_size = (ih, iw), resized to out_size = (OH, OW)) > thr, written into the rectangle of that size at origin = (y0, x0)
    of frame i of `out` uint8 [n,FH,FW]. A new `out` is [n,y0+OH,x0+OW] and zero outside the rectangle; a given one keeps its bytes
    there. With `label` uint8 [FH,FW] also int64 [n,3] {tp,fp,fn} over the rectangle."""
    _req(low, torch.float32, "low"); _req(idx, torch.int32, "idx")
    assert low.is_contiguous() and idx.is_contiguous()
    IN, n = low.shape[-1], idx.numel()
    (ih, iw), (OH, OW), (y0, x0) = (int(v) for v in in_size), (int(v) for v in out_size), (int(v) for v in origin)
    if out is None:
        make = torch.empty if (y0, x0) == (0, 0) else torch.zeros
        out = make((n, y0 + OH, x0 + OW), dtype=torch.uint8, device=low.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.dim() == 3 and out.shape[0] >= n
    FH, FW = out.shape[1:]
    counts = None
    if label is not None:
        _req(label, torch.uint8, "label")
        assert label.is_contiguous() and tuple(label.shape) == (FH, FW)
        counts = torch.empty((n, 3), dtype=torch.int64, device=low.device)
    st = _lib.lib().psam_mask_binarize_resized(_ptr(low), _ptr(idx), n, IN, MID, ih, iw, OH, OW, variant, float(thr), _ptr(out), FH,
                                               FW, y0, x0, _ptr(label), _ptr(counts), _stream())
    _lib.check(st, "psam_mask_binarize_resized")
    return out, counts


NMS_MAX_GROUP = 16384   # candidates psam_box_nms / psam_amg_select take per group (csrc/nms.hip)
AMG_REC = 9             # int32 words of a psam_amg_select record: candidate, plane, IoU bits, stability bits, area, x0, y0, x1, y1
_nms_scratch = {}
_nms_offsets = {}


def nms_workspace(G, max_group):
    """Bytes of scratch psam_box_nms / psam_amg_select need for G groups of up to max_group rows (psam_nms_workspace)."""
    nbytes = _lib.c_longlong(0)
    _lib.check(_lib.lib().psam_nms_workspace(G, max_group, nbytes), "psam_nms_workspace")
    return nbytes.value


def _nms_groups(offsets, n, device):
    """Host-side check of the group offsets (a sequence of G + 1 ascending ints from 0 to n, no group above NMS_MAX_GROUP) ->
    (device int32 copy, cached per value, G, largest group or 1)."""
    off = tuple(int(v) for v in offsets)
    if len(off) < 2 or off[0] != 0 or off[-1] != n or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError(f"offsets must ascend from 0 to {n} over at least one group, got {off[:8]}{'...' if len(off) > 8 else ''}")
    big = max(b - a for a, b in zip(off, off[1:]))
    if big > NMS_MAX_GROUP:
        raise ValueError(f"a group of {big} candidates exceeds the capacity of {NMS_MAX_GROUP}")
    key = (str(device), off)
    if key not in _nms_offsets:
        if len(_nms_offsets) > 64:
            _nms_offsets.clear()
        _nms_offsets[key] = torch.tensor(off, dtype=torch.int32).to(device)
    return _nms_offsets[key], len(off) - 1, max(big, 1)


def _nms_scratch_for(G, maxg, device, scratch):
    if scratch is None:
        key = (str(device), G, maxg)
        if key not in _nms_scratch:
            _nms_scratch[key] = torch.empty((nms_workspace(G, maxg) + 7) // 8, dtype=torch.int64, device=device)
        scratch = _nms_scratch[key]
    if not scratch.is_cuda or scratch.dtype != torch.int64 or not scratch.is_contiguous():
        raise TypeError("scratch: expected a contiguous int64 device tensor")
    _req_aligned(scratch, 16, "scratch")
    return scratch


def box_nms(boxes, scores, offsets, iou_threshold, cap=None, kept=None, count=None, scratch=None):
    """Box NMS per group on the device (psam_box_nms), equal to utils.amg.nms_xyxy on every group: boxes int32 or fp32 [n,4] (x0,
    y0, x1, y1), scores fp32 [n], `offsets` a HOST sequence of G + 1 ascending ints (group g = rows offsets[g]:offsets[g+1], at most
    NMS_MAX_GROUP each) -> (kept int32 [G,cap]: indices inside the group in suppression order, count int32 [G]: the number kept,
    which may exceed cap - then only the first cap are stored). cap defaults to the largest group. `scratch`: int64 tensor of
    nms_workspace bytes (default: cached per shape); calls on one stream share it in order."""
    if boxes is None or scores is None or not torch.is_tensor(boxes) or not torch.is_tensor(scores):
        raise TypeError("boxes, scores: expected tensors")
    if boxes.dtype not in (torch.int32, torch.float32):
        raise TypeError(f"boxes: expected torch.int32 or torch.float32, got {boxes.dtype}")
    _req_rows(boxes, boxes.dtype, "boxes"); _req_rows(scores, torch.float32, "scores")
    if boxes.dim() != 2 or boxes.shape[1] != 4 or not boxes.is_contiguous() or not scores.is_contiguous():
        raise ValueError(f"boxes: expected a contiguous [n, 4], got {tuple(boxes.shape)}")
    n = boxes.shape[0]
    if scores.numel() != n:
        raise ValueError(f"scores: expected {n} values, got {scores.numel()}")
    _req_aligned(boxes, 16, "boxes")
    off_d, G, maxg = _nms_groups(offsets, n, boxes.device)
    cap = maxg if cap is None else int(cap)
    if cap < 1:
        raise ValueError(f"cap must be at least 1, got {cap}")
    if kept is None:
        kept = torch.empty((G, cap), dtype=torch.int32, device=boxes.device)
    if count is None:
        count = torch.empty((G,), dtype=torch.int32, device=boxes.device)
    _req(kept, torch.int32, "kept"); _req(count, torch.int32, "count")
    assert kept.is_contiguous() and kept.numel() >= G * cap and count.is_contiguous() and count.numel() >= G
    scratch = _nms_scratch_for(G, maxg, boxes.device, scratch)
    st = _lib.lib().psam_box_nms(_ptr(boxes), 1 if boxes.dtype == torch.float32 else 0, _ptr(scores), _ptr(off_d), n, G, maxg,
                                 float(iou_threshold), _ptr(kept), cap, _ptr(count), _ptr(scratch), scratch.numel() * 8, _stream())
    _lib.check(st, "psam_box_nms")
    return kept, count


def amg_select(stats, iou4, offsets, pred_iou_thresh, stability_score_thresh, box_nms_thresh, cap=None, out=None, scratch=None,
               _crop=None):
    """The generator's score filters and box NMS on the device (psam_amg_select), equal to automatic_mask_generator.py's host lines:
    stats int32 [n,8] (mask_stats), iou4 fp32 [ceil(n/3),4] (the decoder's IoU output, candidate c = row c // 3, column 1 + c % 3),
    `offsets` as box_nms. -> (records int32 [G,cap,AMG_REC], count int32 [G]), both views of ONE int32 tensor `out` of G * cap *
    AMG_REC + G words (records first), so that one copy brings everything to the host. A filter threshold <= 0 switches that filter
    off. count may exceed cap (default: the largest group): only the first cap records are stored."""
    _req_rows(stats, torch.int32, "stats"); _req_rows(iou4, torch.float32, "iou4")
    if stats is None or iou4 is None:
        raise TypeError("stats, iou4: expected tensors")
    if stats.dim() != 2 or stats.shape[1] != 8 or not stats.is_contiguous():
        raise ValueError(f"stats: expected a contiguous [n, 8], got {tuple(stats.shape)}")
    n = stats.shape[0]
    if iou4.dim() != 2 or iou4.shape[1] != 4 or not iou4.is_contiguous() or iou4.shape[0] * 3 < n:
        raise ValueError(f"iou4: expected a contiguous [>= {(n + 2) // 3}, 4], got {tuple(iou4.shape)}")
    off_d, G, maxg = _nms_groups(offsets, n, stats.device)
    cap = maxg if cap is None else int(cap)
    if cap < 1:
        raise ValueError(f"cap must be at least 1, got {cap}")
    words = G * cap * AMG_REC + G
    if out is None:
        out = torch.empty((words,), dtype=torch.int32, device=stats.device)
    _req(out, torch.int32, "out")
    assert out.is_contiguous() and out.numel() >= words
    records, count = out[:G * cap * AMG_REC].view(G, cap, AMG_REC), out[G * cap * AMG_REC:words]
    scratch = _nms_scratch_for(G, maxg, stats.device, scratch)
    head = (_ptr(stats), _ptr(iou4), _ptr(off_d), n, G, maxg, float(pred_iou_thresh), float(stability_score_thresh),
            float(box_nms_thresh))
    tail = (_ptr(records), cap, _ptr(count), _ptr(scratch), scratch.numel() * 8, _stream())
    if _crop is None:
        _lib.check(_lib.lib().psam_amg_select(*head, *tail), "psam_amg_select")
    else:
        _lib.check(_lib.lib().psam_amg_select_crop(*head, (_lib.c_int * 4)(*_crop[0]), (_lib.c_int * 4)(*_crop[1]), *tail),
                   "psam_amg_select_crop")
    return records, count


def amg_select_crop(stats, iou4, offsets, pred_iou_thresh, stability_score_thresh, box_nms_thresh, crop_box, orig_box, cap=None,
                    out=None, scratch=None):
    """amg_select for the candidates of one crop (psam_amg_select_crop): a candidate whose box is near a crop edge
    (utils.amg.is_box_near_crop_edge with `crop_box` and `orig_box`, HOST sequences of 4 ints XYXY) is dropped with the score
    filters. The records keep boxes in the crop's frame. Everything else as amg_select."""
    cb, ob = tuple(int(v) for v in crop_box), tuple(int(v) for v in orig_box)
    if len(cb) != 4 or len(ob) != 4:
        raise ValueError(f"crop_box, orig_box: expected 4 ints each, got {cb} and {ob}")
    return amg_select(stats, iou4, offsets, pred_iou_thresh, stability_score_thresh, box_nms_thresh, cap=cap, out=out,
                      scratch=scratch, _crop=(cb, ob))


AMG_CREC = 11           # int32 words of a merged / final crop record: an AMG_REC record (box in the image's frame), crop index, pool row
AMG_GEOM = 8            # int32 words of a crop geometry row: x0, y0, crop width, crop height, ih, iw, float32 bits of 1 / crop area, 0
_crops_scratch = {}


def amg_crop_geometry(crop_boxes, in_sizes):
    """The crop geometry table of the crops route, on the host: crop_boxes [ncrops] XYXY ints, in_sizes [ncrops] (ih, iw) =
    predictor.input_size of every crop -> numpy int32 [ncrops, AMG_GEOM]. The score is the float32 1 / crop area of
    SamAutomaticMaskGenerator._generate_general's cross-crop NMS, computed by its numpy expression."""
    import numpy as np
    cb = np.asarray(crop_boxes, dtype=np.int64).reshape(-1, 4)
    ins = np.asarray(in_sizes, dtype=np.int64).reshape(-1, 2)
    if len(ins) != len(cb):
        raise ValueError(f"{len(cb)} crop boxes but {len(ins)} input sizes")
    f = cb.astype(np.float32)
    scores = (1.0 / ((f[:, 2] - f[:, 0]) * (f[:, 3] - f[:, 1]))).astype(np.float32)
    g = np.zeros((len(cb), AMG_GEOM), np.int32)
    g[:, 0], g[:, 1], g[:, 2], g[:, 3] = cb[:, 0], cb[:, 1], cb[:, 2] - cb[:, 0], cb[:, 3] - cb[:, 1]
    g[:, 4:6] = ins
    g[:, 6] = scores.view(np.int32)
    return g


def _pool_args(pool, merged, bases, ncrops):
    _req(pool, torch.float32, "pool"); _req(merged, torch.int32, "merged"); _req(bases, torch.int32, "bases")
    if pool.dim() != 3 or pool.shape[1] != pool.shape[2] or not pool.is_contiguous():
        raise ValueError(f"pool: expected a contiguous [pool_cap, IN, IN], got {tuple(pool.shape)}")
    pool_cap = pool.shape[0]
    if not 1 <= pool_cap <= NMS_MAX_GROUP:
        raise ValueError(f"a pool of {pool_cap} planes is outside 1 .. {NMS_MAX_GROUP}, the group limit of the cross-crop NMS")
    if not merged.is_contiguous() or merged.numel() < pool_cap * AMG_CREC:
        raise ValueError(f"merged: expected at least {pool_cap * AMG_CREC} contiguous words, got {merged.numel()}")
    if not bases.is_contiguous() or bases.numel() < ncrops + 1 or ncrops < 1:
        raise ValueError(f"bases: expected at least {ncrops + 1} contiguous words for {ncrops} crops, got {bases.numel()}")
    return pool_cap


def amg_keep_planes(low, records, count, crop, ncrops, origin, pool, merged, bases):
    """After crop `crop`'s amg_select_crop (psam_amg_keep_planes): its first min(count, cap) records - records int32 [cap, AMG_REC],
    count int32 [1], both on the device, nothing is read back - join `merged` int32 [pool_cap, AMG_CREC] at the rows that `bases`
    int32 [ncrops + 1] counts, with the box moved by origin = (x0, y0) into the image's frame, and their planes of low
    [n, 4, IN, IN] are copied into the same rows of pool fp32 [pool_cap, IN, IN]. The calls of one image go in crop order on one
    stream. Rows past the pool are not written; amg_crops_nms reports that."""
    _req(low, torch.float32, "low"); _req(records, torch.int32, "records"); _req(count, torch.int32, "count")
    pool_cap = _pool_args(pool, merged, bases, ncrops)
    IN = pool.shape[1]
    if not low.is_contiguous() or low.shape[-1] != IN or low.shape[-2] != IN:
        raise ValueError(f"low: expected contiguous planes of {IN} x {IN}, got {tuple(low.shape)}")
    if records.dim() != 2 or records.shape[1] != AMG_REC or records.stride(1) != 1 or records.stride(0) != AMG_REC:
        raise ValueError(f"records: expected a dense [cap, {AMG_REC}], got {tuple(records.shape)}")
    cap = records.shape[0]
    x0, y0 = (int(v) for v in origin)
    st = _lib.lib().psam_amg_keep_planes(_ptr(low), low.numel() // (IN * IN), IN, _ptr(records), _ptr(count), cap, int(crop), int(ncrops),
                                         x0, y0, _ptr(pool), pool_cap, _ptr(merged), _ptr(bases), _stream())
    _lib.check(st, "psam_amg_keep_planes")


def amg_crops_workspace(pool_cap):
    """Bytes of scratch psam_amg_crops_nms needs for a pool of pool_cap planes."""
    nbytes = _lib.c_longlong(0)
    _lib.check(_lib.lib().psam_amg_crops_workspace(int(pool_cap), nbytes), "psam_amg_crops_workspace")
    return nbytes.value


def amg_crops_nms(merged, bases, geom, ncrops, pool_cap, iou_threshold, use_nms=True, out=None, scratch=None):
    """Cross-crop NMS on the device (psam_amg_crops_nms) over the bases[ncrops] merged records, equal to utils.amg.nms_xyxy with
    the float32 score 1 / crop area of every record's crop (geom int32 [ncrops, AMG_GEOM] on the device, amg_crop_geometry);
    use_nms=False (a single crop box) keeps every record in merged order. -> out int32 [pool_cap * AMG_CREC + 2]: the final records
    in suppression order, the final count (-1 where the pool overflowed) and the merged total; one copy of it is the decision."""
    _req(merged, torch.int32, "merged"); _req(bases, torch.int32, "bases"); _req(geom, torch.int32, "geom")
    pool_cap, ncrops = int(pool_cap), int(ncrops)
    if not 1 <= pool_cap <= NMS_MAX_GROUP:
        raise ValueError(f"a pool of {pool_cap} planes is outside 1 .. {NMS_MAX_GROUP}, the group limit of the cross-crop NMS")
    assert merged.is_contiguous() and merged.numel() >= pool_cap * AMG_CREC and bases.is_contiguous() and bases.numel() >= ncrops + 1
    assert geom.is_contiguous() and geom.numel() >= ncrops * AMG_GEOM and ncrops >= 1
    words = pool_cap * AMG_CREC + 2
    if out is None:
        out = torch.empty((words,), dtype=torch.int32, device=merged.device)
    _req(out, torch.int32, "out")
    assert out.is_contiguous() and out.numel() >= words
    if scratch is None:
        key = (str(merged.device), pool_cap)
        if key not in _crops_scratch:
            _crops_scratch[key] = torch.empty((amg_crops_workspace(pool_cap) + 7) // 8, dtype=torch.int64, device=merged.device)
        scratch = _crops_scratch[key]
    if not scratch.is_cuda or scratch.dtype != torch.int64 or not scratch.is_contiguous():
        raise TypeError("scratch: expected a contiguous int64 device tensor")
    _req_aligned(scratch, 16, "scratch")
    st = _lib.lib().psam_amg_crops_nms(_ptr(merged), _ptr(bases), ncrops, _ptr(geom), pool_cap, float(iou_threshold), 1 if use_nms else 0,
                                       _ptr(out), _ptr(scratch), scratch.numel() * 8, _stream())
    _lib.check(st, "psam_amg_crops_nms")
    return out


def mask_binarize_crops(pool, final_records, m, geom, ncrops, MID, size, variant, thr=0.0, out=None):
    """The masks of the first m final records (psam_mask_binarize_crops): final_records int32 [>= m * AMG_CREC] on the device (the
    `out` of amg_crops_nms), pool fp32 [pool_cap, IN, IN], geom int32 [ncrops, AMG_GEOM] -> uint8 [m, H, W] for size = (H, W): frame i
    holds mask_binarize_resized of record i's pool plane with its crop's input size, crop size and origin, and is zero elsewhere."""
    _req(pool, torch.float32, "pool"); _req(final_records, torch.int32, "final_records"); _req(geom, torch.int32, "geom")
    assert pool.is_contiguous() and pool.dim() == 3 and final_records.is_contiguous() and geom.is_contiguous()
    pool_cap, IN = pool.shape[0], pool.shape[1]
    m, ncrops = int(m), int(ncrops)
    H, W = (int(v) for v in size)
    if not 1 <= m <= pool_cap or final_records.numel() < m * AMG_CREC or geom.numel() < ncrops * AMG_GEOM:
        raise ValueError(f"mask_binarize_crops: {m} records of a pool of {pool_cap}, {final_records.numel()} record words")
    if out is None:
        out = torch.empty((m, H, W), dtype=torch.uint8, device=pool.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (m, H, W)
    st = _lib.lib().psam_mask_binarize_crops(_ptr(pool), pool_cap, _ptr(final_records), m, _ptr(geom), ncrops, IN, MID, variant, float(thr),
                                             _ptr(out), H, W, _stream())
    _lib.check(st, "psam_mask_binarize_crops")
    return out


SMALL_REGIONS_BUDGET = 256 << 20   # bytes of scratch small_regions sizes its chunk for (8 bytes per pixel and mask in flight)
_sr_scratch = {}


def small_regions_workspace(H, W, chunk):
    """Bytes of scratch psam_small_regions needs for `chunk` masks of H x W in flight (psam_small_regions_workspace)."""
    nbytes = _lib.c_longlong(0)
    _lib.check(_lib.lib().psam_small_regions_workspace(int(H), int(W), int(chunk), nbytes), "psam_small_regions_workspace")
    return nbytes.value


def small_regions_chunk(m, H, W, budget=None):
    """Masks in flight for m masks of H x W under a scratch budget in bytes (default SMALL_REGIONS_BUDGET): at least one."""
    budget = SMALL_REGIONS_BUDGET if budget is None else int(budget)
    return max(1, min(max(int(m), 1), budget // (8 * H * W + 64)))


def small_regions(masks_u8, area_thresh, out=None, chunk=None, scratch=None):
    """Holes and islands below `area_thresh` pixels removed from m masks at once (psam_small_regions), per mask equal to
    utils.amg's remove_small_regions(mask, t, "holes") then (., t, "islands"): masks_u8 uint8 [m,H,W] (0 / non-0) ->
    (out uint8 [m,H,W] 0 / 1, boxes int32 [m,4] XYXY of `out` ([0,0,0,0] for an empty mask), scores fp32 [m] = 1.0 where nothing
    changed else 0.0, info int32 [m,4] = {changed_holes, changed_islands, area of out, 0}). `chunk`: masks in flight (default: what
    fits SMALL_REGIONS_BUDGET bytes of scratch, at least one); `scratch`: int64 device tensor of small_regions_workspace bytes
    (default: cached per shape). Regions are counted per union-find root: no limit on their number."""
    if masks_u8 is None or not torch.is_tensor(masks_u8):
        raise TypeError("masks_u8: expected a tensor")
    _req_rows(masks_u8, torch.uint8, "masks_u8")
    if masks_u8.dim() != 3 or not masks_u8.is_contiguous():
        raise ValueError(f"masks_u8: expected a contiguous [m, H, W], got {tuple(masks_u8.shape)}")
    m, H, W = masks_u8.shape
    if H <= 0 or W <= 0 or H * W > 0x7fffffff:
        raise ValueError(f"masks_u8: H and W must be positive with H * W within int32, got {H} x {W}")
    t = float(area_thresh)
    if t != t:
        raise ValueError("area_thresh must not be NaN")
    if chunk is None:
        chunk = small_regions_chunk(m, H, W)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    dev = masks_u8.device
    if out is None:
        out = torch.empty((m, H, W), dtype=torch.uint8, device=dev)
    _req_rows(out, torch.uint8, "out")
    if tuple(out.shape) != (m, H, W) or not out.is_contiguous():
        raise ValueError(f"out: expected a contiguous {(m, H, W)}, got {tuple(out.shape)}")
    boxes = torch.empty((m, 4), dtype=torch.int32, device=dev)
    scores = torch.empty((m,), dtype=torch.float32, device=dev)
    info = torch.empty((m, 4), dtype=torch.int32, device=dev)
    need = small_regions_workspace(H, W, chunk)
    if scratch is None:
        key = (str(dev), H, W, chunk)
        if key not in _sr_scratch:
            _sr_scratch.clear()                      # (one working set at a time: it is sized by a byte budget)
            _sr_scratch[key] = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)
        scratch = _sr_scratch[key]
    if not torch.is_tensor(scratch) or not scratch.is_cuda or scratch.dtype != torch.int64 or not scratch.is_contiguous():
        raise TypeError("scratch: expected a contiguous int64 device tensor")
    if scratch.numel() * 8 < need:
        raise ValueError(f"scratch: {scratch.numel() * 8} bytes, {need} needed for {chunk} masks of {H} x {W} in flight")
    st = _lib.lib().psam_small_regions(_ptr(masks_u8), m, H, W, t, chunk, _ptr(out), _ptr(boxes), _ptr(scores), _ptr(info),
                                       _ptr(scratch), scratch.numel() * 8, _stream())
    _lib.check(st, "psam_small_regions")
    return out, boxes, scores, info


def small_regions_select(masks_u8, area_thresh, nms_thresh, chunk=None, scratch=None):
    """small_regions and the box NMS of the generator's small-region stage behind it (psam_box_nms, one group, scores 1.0 for
    unchanged masks and 0.0 for changed ones, so unchanged masks are visited first): -> (out uint8 [m,H,W], table), `table` ONE
    int32 device tensor of 1 + 9 m words so that a single copy brings the whole decision to the host:
    table[0] = count kept, table[1:1+m] = kept indices in suppression order (the first `count` are valid),
    table[1+m:1+5m] = info [m,4], table[1+5m:1+9m] = boxes [m,4]. `small_regions_table(host_table, m)` splits a host copy.
    More than NMS_MAX_GROUP masks raise."""
    if masks_u8 is None or not torch.is_tensor(masks_u8):
        raise TypeError("masks_u8: expected a tensor")
    m = masks_u8.shape[0] if masks_u8.dim() == 3 else 0
    if m > NMS_MAX_GROUP:
        raise ValueError(f"{m} masks exceed the capacity of {NMS_MAX_GROUP} of one NMS group")
    out, boxes, scores, info = small_regions(masks_u8, area_thresh, chunk=chunk, scratch=scratch)
    table = torch.empty((1 + 9 * m,), dtype=torch.int32, device=masks_u8.device)
    if m == 0:
        table.zero_()
        return out, table
    box_nms(boxes, scores, (0, m), nms_thresh, cap=m, kept=table[1:1 + m].view(1, m), count=table[:1])
    table[1 + m:1 + 5 * m].copy_(info.view(-1))
    table[1 + 5 * m:].copy_(boxes.view(-1))
    return out, table


def small_regions_table(table, m):
    """The host copy (numpy int32) of small_regions_select's table -> (kept int64 [count], info [m,4], boxes [m,4])."""
    count = min(int(table[0]), m)
    return (table[1:1 + count].astype("int64"), table[1 + m:1 + 5 * m].reshape(m, 4), table[1 + 5 * m:1 + 9 * m].reshape(m, 4))


# ---- connected-component clean-up of volumes (csrc/volume_regions.hip) --------------------------------------
VOLUME_REGIONS_BUDGET = 1 << 30    # bytes of scratch volume_regions sizes its chunk for (8 bytes per voxel and volume in flight)
VOLREG_COLS = ("components", "kept", "voxels_in", "voxels_out", "largest_size", "largest_root", "z0", "y0", "x0", "z1", "y1", "x1")
_vr_scratch = {}


def _volreg_shape(D, H, W):
    D, H, W = int(D), int(H), int(W)
    if D <= 0 or H <= 0 or W <= 0 or D * H * W >= 1 << 31 or D * H * ((W + 255) // 256) * 256 > 0xffffffff:
        raise ValueError(f"volume: D, H and W must be positive with D * H * W below 2^31, got {D} x {H} x {W}")
    return D, H, W


def volume_regions_workspace(D, H, W, chunk, labels=False):
    """Bytes of scratch psam_volume_regions needs for `chunk` volumes of D x H x W in flight: parent and size arrays, 64 bytes of
    accumulators and, with labels, one int32 per 256-voxel block (the scan's block sums)."""
    D, H, W = _volreg_shape(D, H, W)
    if int(chunk) < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    n = D * H * W
    return int(chunk) * (8 * n + 64 + (4 * ((n + 255) // 256) if labels else 0))


def volume_regions_chunk(R, D, H, W, budget=None):
    """Volumes in flight for R volumes of D x H x W under a scratch budget in bytes (default VOLUME_REGIONS_BUDGET): at least one."""
    budget = VOLUME_REGIONS_BUDGET if budget is None else int(budget)
    return max(1, min(max(int(R), 1), budget // volume_regions_workspace(D, H, W, 1, labels=True)))


def volume_regions(vol, connectivity=26, min_voxels=0, keep_largest=False, labels=False, out=None, chunk=None, scratch=None,
                   layout="rdhw"):
    """3-D connected components per volume and the clean-up on top of them (psam_volume_regions), nothing synchronised.
    vol uint8 (0 / non-0): [D, H, W] (one volume), [R, D, H, W] (layout "rdhw", class-major) or the slice-major [Z, C, H, W] of
    kept masks (layout "zchw": volume r is class r, read where it lies); [H, W] planes contiguous, outer strides free.
    connectivity 6 / 18 / 26; components with size < min_voxels are dropped (all of them: then `out` is empty); keep_largest keeps
    the largest survivor only, ties to the first in raster order.
    -> (out, info[, labels]): out uint8 {0, 1} shaped and strided as vol (out= may be vol itself: in place); info int64 [R, 12]
    (VOLREG_COLS; `volume_regions_table` reads a host copy); labels=True adds int32 [R, D, H, W] (contiguous and class-major for
    either layout, [D, H, W] for a 3-D vol): the input's components numbered as scipy.ndimage.label numbers them, or pass an int32
    tensor of that shape to fill. `chunk`: volumes in flight (default: what fits VOLUME_REGIONS_BUDGET, at least one); `scratch`:
    int64 device tensor of volume_regions_workspace bytes (default: cached per shape)."""
    if vol is None or not torch.is_tensor(vol):
        raise TypeError("vol: expected a tensor")
    if vol.dtype != torch.uint8:
        raise TypeError(f"vol: expected {torch.uint8}, got {vol.dtype}")
    if layout not in ("rdhw", "zchw"):
        raise ValueError(f"layout must be 'rdhw' or 'zchw', got {layout!r}")
    if int(connectivity) not in (6, 18, 26) or connectivity != int(connectivity):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity}")
    if min_voxels != int(min_voxels) or int(min_voxels) < 0:
        raise ValueError(f"min_voxels must be a non-negative integer, got {min_voxels}")
    if keep_largest not in (0, 1, False, True):
        raise ValueError(f"keep_largest must be 0 or 1, got {keep_largest}")
    if vol.dim() == 3 and layout == "rdhw":
        R, (D, H, W), sr, sz = 1, vol.shape, None, vol.stride(0)
    elif vol.dim() == 4 and layout == "rdhw":
        (R, D, H, W), sr, sz = vol.shape, vol.stride(0), vol.stride(1)
    elif vol.dim() == 4:
        (D, R, H, W), sr, sz = vol.shape, vol.stride(1), vol.stride(0)
    else:
        raise ValueError(f"vol: expected [D, H, W], [R, D, H, W] or, with layout='zchw', [Z, C, H, W]; got {tuple(vol.shape)}")
    D, H, W = _volreg_shape(D, H, W)
    if R == 0:
        raise ValueError(f"vol: no volume in {tuple(vol.shape)}")
    if (W > 1 and vol.stride(-1) != 1) or (H > 1 and vol.stride(-2) != W):
        raise ValueError(f"vol: [H, W] planes must be contiguous, got strides {tuple(vol.stride())}")
    _req(vol, torch.uint8, "vol")
    sr = D * H * W if sr is None or R == 1 and sr < H * W else sr
    sz = H * W if D == 1 and sz < H * W else sz
    if sr < H * W or sz < H * W:
        raise ValueError(f"vol: planes overlap, strides {tuple(vol.stride())}")
    if chunk is None:
        chunk = volume_regions_chunk(R, D, H, W)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    dev = vol.device
    if out is None:
        out = torch.empty_strided(tuple(vol.shape), tuple(vol.stride()), dtype=torch.uint8, device=dev)
    _req(out, torch.uint8, "out")
    if tuple(out.shape) != tuple(vol.shape) or tuple(out.stride()) != tuple(vol.stride()):
        raise ValueError(f"out: expected shape {tuple(vol.shape)} and strides {tuple(vol.stride())}, got {tuple(out.shape)} and "
                         f"{tuple(out.stride())}")
    lab_shape = (D, H, W) if vol.dim() == 3 else (R, D, H, W)
    lab = None
    if torch.is_tensor(labels):
        lab = labels
        _req(lab, torch.int32, "labels")
        if tuple(lab.shape) != lab_shape or not lab.is_contiguous():
            raise ValueError(f"labels: expected a contiguous {lab_shape}, got {tuple(lab.shape)}")
    elif labels:
        lab = torch.empty(lab_shape, dtype=torch.int32, device=dev)
    need = volume_regions_workspace(D, H, W, chunk, labels=lab is not None)
    if scratch is None:
        key = (str(dev), D, H, W, chunk, lab is not None)
        if key not in _vr_scratch:
            _vr_scratch.clear()                      # (one working set at a time: it is sized by a byte budget)
            _vr_scratch[key] = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)
        scratch = _vr_scratch[key]
    if not torch.is_tensor(scratch) or not scratch.is_cuda or scratch.dtype != torch.int64 or not scratch.is_contiguous():
        raise TypeError("scratch: expected a contiguous int64 device tensor")
    if scratch.numel() * 8 < need:
        raise ValueError(f"scratch: {scratch.numel() * 8} bytes, {need} needed for {chunk} volumes of {D} x {H} x {W} in flight")
    info = torch.empty((R, 12), dtype=torch.int64, device=dev)
    st = _lib.lib().psam_volume_regions(_ptr(vol), R, D, H, W, sr, sz, int(connectivity), int(min_voxels), int(keep_largest), chunk,
                                        _ptr(out), _ptr(info), _ptr(lab), _ptr(scratch), scratch.numel() * 8, _stream())
    _lib.check(st, "psam_volume_regions")
    return (out, info) if lab is None else (out, info, lab)


def volume_regions_table(info):
    """The `info` of volume_regions (device or host) -> one dict per volume, keyed by VOLREG_COLS, plus "voxels_dropped" and "box"
    (z0, y0, x0, z1, y1, x1, or None for an empty result). A device tensor is copied, which waits for the stream."""
    host = info.detach().cpu().numpy() if torch.is_tensor(info) else info
    rows = []
    for r in host.reshape(-1, len(VOLREG_COLS)).tolist():
        d = dict(zip(VOLREG_COLS, (int(v) for v in r)))
        d["voxels_dropped"] = d["voxels_in"] - d["voxels_out"]
        d["box"] = None if d["voxels_out"] == 0 else tuple(int(v) for v in r[6:12])
        rows.append(d)
    return rows


def mask_counts(low, records, count, MID, H, W, variant, label, thr=0.0, counts=None):
    """int64 [cap,3] {tp, fp, fn} against `label` uint8 [H,W] of the first min(count, cap) records of ONE group (records int32
    [cap,AMG_REC], count int32 [1], both on the device, as amg_select leaves them): mask_binarize's counts without the masks and
    without the host knowing how many rows there are. Rows beyond the count stay zero."""
    _req(low, torch.float32, "low"); _req(records, torch.int32, "records"); _req(count, torch.int32, "count")
    _req(label, torch.uint8, "label")
    if low is None or records is None or count is None or label is None:
        raise TypeError("low, records, count, label: expected tensors")
    if records.dim() != 2 or records.shape[1] != AMG_REC or not records.is_contiguous() or count.numel() != 1:
        raise ValueError(f"records / count: expected one group [cap, {AMG_REC}] and [1], got {tuple(records.shape)}, {tuple(count.shape)}")
    cap = records.shape[0]
    if cap < 1 or cap > 65535:
        raise ValueError(f"records: 1 .. 65535 rows, got {cap}")
    assert low.is_contiguous() and label.is_contiguous() and tuple(label.shape) == (H, W)
    IN = low.shape[-1]
    if counts is None:
        counts = torch.empty((cap, 3), dtype=torch.int64, device=low.device)
    _req(counts, torch.int64, "counts")
    assert counts.is_contiguous() and counts.numel() >= cap * 3
    st = _lib.lib().psam_mask_counts(_ptr(low), low.numel() // (IN * IN), _ptr(records[:, 1:]), AMG_REC, _ptr(count), cap, IN, MID, H,
                                     W, variant, float(thr), _ptr(label), _ptr(counts), _stream())
    _lib.check(st, "psam_mask_counts")
    return counts


def best_iou(counts, records, count, best=None, iou=None):
    """The row SamWrapper.forward's loop picks among the first min(count, cap) rows of counts int64 [cap,3] (psam_best_iou): IoU =
    tp / (tp + fp + fn) in float64, row 0 whatever its IoU, a later row only with `>`. -> (best int32 [4] = {plane of the winner
    (records[row, 1]), its row, 1 if there is no row (then plane 0, row -1), rows looked at}, iou float64 [1]), on the device."""
    _req(counts, torch.int64, "counts"); _req(records, torch.int32, "records"); _req(count, torch.int32, "count")
    if counts is None or records is None or count is None:
        raise TypeError("counts, records, count: expected tensors")
    if records.dim() != 2 or records.shape[1] != AMG_REC or not records.is_contiguous() or count.numel() != 1:
        raise ValueError(f"records / count: expected one group [cap, {AMG_REC}] and [1], got {tuple(records.shape)}, {tuple(count.shape)}")
    cap = records.shape[0]
    if cap < 1 or counts.dim() != 2 or counts.shape[1] != 3 or counts.shape[0] < cap or not counts.is_contiguous():
        raise ValueError(f"counts: expected a contiguous [>= {cap}, 3], got {tuple(counts.shape)}")
    if best is None:
        best = torch.empty((4,), dtype=torch.int32, device=counts.device)
    if iou is None:
        iou = torch.empty((1,), dtype=torch.float64, device=counts.device)
    _req(best, torch.int32, "best"); _req(iou, torch.float64, "iou")
    assert best.numel() >= 4 and iou.numel() >= 1
    st = _lib.lib().psam_best_iou(_ptr(counts), _ptr(records[:, 1:]), AMG_REC, _ptr(count), cap, _ptr(best), _ptr(iou), _stream())
    _lib.check(st, "psam_best_iou")
    return best, iou


def _rle_masks(masks):
    if not masks.is_cuda:
        raise RuntimeError("masks: expected a device tensor (protosam_amd has no CPU path)")
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    if masks.dtype != torch.uint8:
        raise TypeError(f"masks: expected torch.uint8 or torch.bool, got {masks.dtype}")
    if masks.dim() == 2:
        masks = masks[None]
    if masks.dim() != 3:
        raise ValueError(f"masks: expected [n, H, W] or [H, W], got {tuple(masks.shape)}")
    return masks.contiguous()


def rle_encode(masks):
    """masks uint8 / bool [n,H,W] or [H,W] (any non-zero byte is set) -> (counts int32 [total], offsets int64 [n+1]), both on the
    device: mask i's uncompressed COCO run lengths (column-major, starting with a zero-run) are counts[offsets[i]:offsets[i+1]].
    One scalar crosses to the host between the two launches (offsets[n], to size `counts`); it is the only synchronisation."""
    masks = _rle_masks(masks)
    n, H, W = masks.shape
    dev = masks.device
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    if n == 0:
        return torch.empty((0,), dtype=torch.int32, device=dev), offsets
    if H == 0 or W == 0:
        raise ValueError(f"masks: empty planes {tuple(masks.shape)}")
    L = _lib.lib()
    per = _lib.c_longlong(0)
    _lib.check(L.psam_rle_workspace(H, W, per), "psam_rle_workspace")
    cells = torch.empty((n * per.value,), dtype=torch.int32, device=dev)
    totals = torch.empty((n,), dtype=torch.int64, device=dev)
    _lib.check(L.psam_rle_count(_ptr(masks), n, H, W, _ptr(cells), _ptr(totals), _stream()), "psam_rle_count")
    torch.cumsum(totals, 0, out=offsets[1:])
    counts = torch.empty((int(offsets[n].item()),), dtype=torch.int32, device=dev)
    _lib.check(L.psam_rle_write(_ptr(masks), n, H, W, _ptr(cells), _ptr(offsets), _ptr(counts), _stream()), "psam_rle_write")
    return counts, offsets


def rle_decode(counts, offsets, H, W):
    """The inverse of `rle_encode`: counts int32 [total], offsets int64 [n+1] (device) -> uint8 {0,1} [n,H,W]. The lists are taken
    as they are (a pixel past the end of a short list is 0); `utils.amg.rle_to_mask_device` validates host-made lists."""
    _req(counts, torch.int32, "counts"); _req(offsets, torch.int64, "offsets")
    assert counts.dim() == 1 and offsets.dim() == 1 and offsets.numel() >= 1
    n = offsets.numel() - 1
    out = torch.empty((n, H, W), dtype=torch.uint8, device=counts.device)
    if n == 0:
        return out
    off = offsets.cpu()                                        # n + 1 numbers: the kernel indexes `counts` with them
    if int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()) or int(off[-1]) > counts.numel() or counts.numel() == 0:
        raise ValueError("offsets: expected 0 = offsets[0] <= ... <= offsets[n] <= len(counts), and at least one count")
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    st = _lib.lib().psam_rle_decode(_ptr(ends), _ptr(offsets), n, H, W, _ptr(out), _stream())
    _lib.check(st, "psam_rle_decode")
    return out


_SEG_DT = {torch.int16: 0, torch.float32: 1, torch.uint8: 2, torch.int32: 3}      # (slice_io._TORCH_DT: the codes of psam_volume_*)
SEG_COLS = ("tp", "fp", "fn", "tn", "px0", "py0", "px1", "py1", "gx0", "gy0", "gx1", "gy1")


def _seg_planes(t, name):
    """t [planes, H, W] or [n, C, H, W] with contiguous [H, W] planes one stride apart -> (tensor to pass, planes, stride, H, W).
    int64 is cast once on the device (to int32; label ids and {0, 1} masks fit)."""
    if t.dim() not in (3, 4):
        raise ValueError(f"{name}: expected [planes, H, W] or [n, C, H, W], got {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (protosam_amd has no CPU path)")
    if t.dtype == torch.int64:
        t = t.to(torch.int32)
    if t.dtype not in _SEG_DT:
        raise TypeError(f"{name}: expected one of {sorted(str(d) for d in _SEG_DT)} or int64, got {t.dtype}")
    H, W = t.shape[-2:]
    if H > 0 and W > 0 and (t.stride(-1) != 1 or t.stride(-2) != W):
        t = t.contiguous()
    if t.dim() == 4:
        n, C = t.shape[:2]
        if n > 1 and C > 1 and t.stride(0) != C * t.stride(1):      # planes are not evenly spaced
            t = t.contiguous()
        planes, stride = n * C, (t.stride(1) if C > 1 else t.stride(0))
    else:
        planes, stride = t.shape[0], t.stride(0)
    return t, planes, stride, H, W


def seg_counts(pred, label, rows, out=None):
    """Confusion counts and boxes of many (prediction plane, label plane) pairs in one launch (psam_seg_counts).
    pred / label: device tensors [planes, H, W] or [n, C, H, W] (planes numbered n-major) of int16 / float32 / uint8 / int32
    (int64 is cast), same H, W; views with a storage offset or a plane stride are passed as they are.
    rows: (pred plane, pred value, label plane, label value) per output row - a Python list / array (range-checked here, ValueError,
    before anything touches the device) or an int32 device tensor [n, 4] (rows outside the planes are skipped by the kernel).
    -> out int64 [n, 12], columns SEG_COLS; asynchronous on the current stream."""
    if tuple(pred.shape[-2:]) != tuple(label.shape[-2:]):
        raise ValueError(f"pred planes {tuple(pred.shape[-2:])} and label planes {tuple(label.shape[-2:])} differ")
    if not isinstance(rows, torch.Tensor):
        import numpy as np
        r = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
        n_pred, n_lab = int(np.prod(pred.shape[:-2])), int(np.prod(label.shape[:-2]))
        for k, (pp, _, lp, _) in enumerate(r.tolist()):
            if not 0 <= pp < n_pred:
                raise ValueError(f"rows[{k}]: prediction plane {pp} outside [0, {n_pred})")
            if not 0 <= lp < n_lab:
                raise ValueError(f"rows[{k}]: label plane {lp} outside [0, {n_lab})")
        if r.size and (np.abs(r) > 0x7fffffff).any():
            raise ValueError("rows: a value does not fit int32")
        rows = torch.from_numpy(r.astype(np.int32)).to(pred.device)
    pred, n_pred, s_pred, H, W = _seg_planes(pred, "pred")
    label, n_lab, s_lab, _, _ = _seg_planes(label, "label")
    _req(rows, torch.int32, "rows")
    assert rows.is_contiguous() and rows.dim() == 2 and rows.shape[1] == 4
    n = rows.shape[0]
    if out is None:
        out = torch.empty((n, 12), dtype=torch.int64, device=pred.device)
    _req(out, torch.int64, "out")
    assert out.is_contiguous() and out.numel() >= n * 12
    st = _lib.lib().psam_seg_counts(_ptr(pred), _SEG_DT[pred.dtype], n_pred, s_pred, _ptr(label), _SEG_DT[label.dtype], n_lab, s_lab,
                                   H, W, _ptr(rows), n, _ptr(out), _stream())
    _lib.check(st, "psam_seg_counts")
    return out


# ---- surface distances: HD, HD95, ASSD (csrc/surface.hip) ---------------------------------------------------
SURFACE_TILE = 256                   # query points per workgroup and points per LDS tile of psam_surface_dist (SURF_TILE)
SURF_COLS = ("n_pred", "n_gt", "hd", "hd95", "assd", "asd_pg", "asd_gp", "status")
SURFACE_OK, SURFACE_OVERFLOW, SURFACE_BAD_ROW = 0, 1, 2         # the status column
SURFACE_CAP_FLOOR, SURFACE_CAP_DIVISOR = 65536, 8
_SURFACE_MAX_VOXELS = 0x7fffffff - 4096
_SURFACE_MAX_SIDE = 1 << 24


def _surface_spacing(spacing):
    """(sz, sy, sx) as floats; a pair is (sy, sx) of a slice. ValueError unless every one is positive and finite as float32."""
    import numpy as np
    sp = tuple(float(v) for v in spacing)
    if len(sp) == 2:
        sp = (1.0,) + sp
    if len(sp) != 3:
        raise ValueError(f"spacing: expected (sz, sy, sx) or (sy, sx), got {spacing!r}")
    with np.errstate(over="ignore"):
        f = np.asarray(sp, dtype=np.float64).astype(np.float32)
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError(f"spacing: every value must be positive and finite in float32, got {spacing!r}")
    return sp


def _surface_geometry(H, W, max_depth):
    if H < 1 or W < 1 or max_depth < 1:
        raise ValueError(f"surface: planes {H} x {W} and depth {max_depth} must be at least 1")
    if max(H, W, max_depth) > _SURFACE_MAX_SIDE or max_depth * H * W > _SURFACE_MAX_VOXELS:
        raise ValueError(f"surface: a row of {max_depth} x {H} x {W} voxels is outside int32 indexing (at most 2^31 - 4097 voxels, "
                         f"2^24 a side)")


def _surface_rows(rows, n_pred, n_lab, max_depth, device):
    """rows as a list / array [n, 5] (range-checked, ValueError) or an int32 device tensor (then max_depth must be given).
    -> (int32 device tensor, n, max_depth, list of depths or None)"""
    if isinstance(rows, torch.Tensor):
        _req(rows, torch.int32, "rows")
        if rows.dim() != 2 or rows.shape[1] != 5 or not rows.is_contiguous() or rows.shape[0] < 1:
            raise ValueError(f"rows: expected a contiguous int32 [n >= 1, 5] table, got {tuple(rows.shape)}")
        if max_depth is None:
            raise ValueError("rows on the device: max_depth= must be given (the launch is sized from it)")
        return rows, rows.shape[0], int(max_depth), None
    import numpy as np
    r = np.asarray(rows, dtype=np.int64)
    if r.size == 0 or r.ndim != 2 or r.shape[1] != 5:
        raise ValueError(f"rows: expected [n >= 1, 5] = (pred plane, pred value, label plane, label value, depth), got {r.shape}")
    for k, (pp, _, lp, _, D) in enumerate(r.tolist()):
        if D < 1:
            raise ValueError(f"rows[{k}]: depth {D} < 1")
        if not (0 <= pp and pp + D <= n_pred):
            raise ValueError(f"rows[{k}]: prediction planes {pp} .. {pp + D - 1} outside [0, {n_pred})")
        if not (0 <= lp and lp + D <= n_lab):
            raise ValueError(f"rows[{k}]: label planes {lp} .. {lp + D - 1} outside [0, {n_lab})")
    if (np.abs(r) > 0x7fffffff).any():
        raise ValueError("rows: a value does not fit int32")
    depths = r[:, 4].tolist()
    md = max(depths) if max_depth is None else int(max_depth)
    if md < max(depths):
        raise ValueError(f"max_depth {md} is below the deepest row ({max(depths)})")
    return torch.from_numpy(r.astype(np.int32)).to(device), r.shape[0], md, depths


def surface_default_cap(covered_voxels):
    """The default pool size of surface_distances: an eighth of the voxels the rows cover (a closed surface of a region of v voxels
    has far fewer than v / 8 voxels once the region is more than a few voxels thick, and a row holds two surfaces), at least 65536
    points. A row that does not fit is flagged, never truncated."""
    return int(min(max(SURFACE_CAP_FLOOR, int(covered_voxels) // SURFACE_CAP_DIVISOR), 0x7ffffffe))


def surface_workspace(n, cap):
    """Bytes of device memory one surface_distances call over n rows with a pool of cap points allocates: the work tables
    (9n + 2 int32), points and d2 (4 bytes a point each), the sort keys and the sorted keys with the sort's index output
    (8 bytes a point each), and the table [n, 8] float64. torch.sort's own temporaries are not counted."""
    return 4 * (9 * n + 2) + cap * (4 + 4 + 8 + 8 + 8) + 64 * n


def surface_points(pred, label, rows, cap, max_depth=None):
    """Surface voxels of both sides of every row, compacted into one pool (psam_surface_points).
    pred / label as seg_counts; rows [n, 5] = (first pred plane, pred value, first label plane, label value, depth D): the row
    compares D consecutive planes of each. The surface of a set: its voxels with a face neighbour (4 in the plane for D == 1,
    6 for D > 1) that is not in the set or lies outside the row's D x H x W range (scipy: M ^ binary_erosion(M, cross)).
    -> dict `work`: counts int32 [n, 2] (the true sizes of S(pred), S(label), whatever cap is), offsets int32 [2n + 1] (their
    exclusive scan: segment 2r = S(pred) of row r, 2r + 1 = S(label)), status int32 [n] (SURFACE_OK / SURFACE_OVERFLOW: the row's
    segments end beyond cap and are not filled / SURFACE_BAD_ROW: a device row outside the planes), points int32 [cap] (linear
    index (z * H + y) * W + x in the row's range; any order inside a segment), and the geometry. Asynchronous."""
    if tuple(pred.shape[-2:]) != tuple(label.shape[-2:]):
        raise ValueError(f"pred planes {tuple(pred.shape[-2:])} and label planes {tuple(label.shape[-2:])} differ")
    if pred.dim() not in (3, 4) or label.dim() not in (3, 4):
        raise ValueError(f"expected [planes, H, W] or [n, C, H, W], got {tuple(pred.shape)} and {tuple(label.shape)}")
    import numpy as np
    n_pred, n_lab = int(np.prod(pred.shape[:-2])), int(np.prod(label.shape[:-2]))
    if not (pred.is_cuda and label.is_cuda):
        raise RuntimeError("surface_points: expected device tensors (protosam_amd has no CPU path)")
    rows, n, md, _ = _surface_rows(rows, n_pred, n_lab, max_depth, pred.device)
    H, W = (int(v) for v in pred.shape[-2:])
    _surface_geometry(H, W, md)
    cap = int(cap)
    if not 1 <= cap <= 0x7ffffffe:
        raise ValueError(f"cap must be in 1 .. 2^31 - 2, got {cap}")
    pred, n_pred, s_pred, _, _ = _seg_planes(pred, "pred")
    label, n_lab, s_lab, _, _ = _seg_planes(label, "label")
    tab = torch.empty(9 * n + 2, dtype=torch.int32, device=pred.device)
    work = {"counts": tab[:2 * n].view(n, 2), "offsets": tab[2 * n:4 * n + 1], "tiles": tab[4 * n + 1:6 * n + 2],
            "status": tab[6 * n + 2:7 * n + 2], "cursors": tab[7 * n + 2:],
            "points": torch.empty(cap, dtype=torch.int32, device=pred.device),
            "n": n, "H": H, "W": W, "max_depth": md, "cap": cap}
    st = _lib.lib().psam_surface_points(_ptr(pred), _SEG_DT[pred.dtype], n_pred, s_pred, _ptr(label), _SEG_DT[label.dtype], n_lab,
                                       s_lab, H, W, md, _ptr(rows), n, _ptr(work["counts"]), _ptr(work["offsets"]),
                                       _ptr(work["tiles"]), _ptr(work["status"]), _ptr(work["cursors"]), _ptr(work["points"]), cap,
                                       _stream())
    _lib.check(st, "psam_surface_points")
    return work


def surface_dist(work, spacing=(1.0, 1.0, 1.0), keys=False):
    """For every filled point of `work` (surface_points) the squared distance to the nearest point of the other surface of its row
    (psam_surface_dist): the fp32 minimum of ((dx*sx)*(dx*sx) + (dy*sy)*(dy*sy)) + (dz*sz)*(dz*sz) over that segment, every
    operation rounded separately (no FMA) on exact integer offsets, spacing (sz, sy, sx) rounded to fp32; +inf where the other
    surface is empty. -> d2 fp32 [cap] (positions outside the filled segments hold +inf); keys=True also leaves
    work["keys"] int64 [cap] = segment << 32 | bits of d2 (the largest int64 outside the segments). Asynchronous."""
    sz, sy, sx = _surface_spacing(spacing)
    cap, dev = work["cap"], work["points"].device
    d2 = torch.full((cap,), float("inf"), dtype=torch.float32, device=dev)
    kt = torch.full((cap,), 0x7fffffffffffffff, dtype=torch.int64, device=dev) if keys else None
    st = _lib.lib().psam_surface_dist(_ptr(work["points"]), _ptr(work["offsets"]), _ptr(work["tiles"]), work["n"], work["H"],
                                     work["W"], work["max_depth"], sz, sy, sx, cap, _ptr(d2), _ptr(kt), _stream())
    _lib.check(st, "psam_surface_dist")
    work["d2"], work["keys"] = d2, kt
    return d2


def surface_stats(sorted_d2, work, out=None):
    """The table of psam_surface_stats from the d2 of every segment sorted ascending: sorted_d2 fp32 [>= filled points], or the
    sorted int64 keys of surface_dist(keys=True). -> out float64 [n, 8], columns SURF_COLS: n_pred, n_gt (surface sizes), hd (the
    larger directed maximum), hd95 (numpy.percentile(both directed sets together, 95), linear interpolation), assd (mean of the
    two directed means), asd_pg, asd_gp (directed means, prediction to ground truth and back), status - float64 functions of
    sqrt((double)d2), the sums in a fixed order (the same bits run to run and for any cap that fits). The five metrics are NaN where
    a surface is empty (MedPy raises there) or the row was not filled. Asynchronous."""
    if sorted_d2.dtype not in (torch.float32, torch.int64):
        raise TypeError(f"sorted_d2: expected float32 values or int64 keys, got {sorted_d2.dtype}")
    _req(sorted_d2, sorted_d2.dtype, "sorted_d2")
    n = work["n"]
    if sorted_d2.dim() != 1 or sorted_d2.numel() < work["cap"]:
        raise ValueError(f"sorted_d2: expected [{work['cap']}] values, got {tuple(sorted_d2.shape)}")
    if out is None:
        out = torch.empty((n, 8), dtype=torch.float64, device=sorted_d2.device)
    _req(out, torch.float64, "out")
    assert out.is_contiguous() and out.numel() >= n * 8
    st = _lib.lib().psam_surface_stats(_ptr(sorted_d2), 2 if sorted_d2.dtype == torch.int64 else 1, _ptr(work["counts"]),
                                      _ptr(work["offsets"]), _ptr(work["status"]), n, _ptr(out), _stream())
    _lib.check(st, "psam_surface_stats")
    return out


def surface_distances(pred, label, rows, spacing=(1.0, 1.0, 1.0), cap=None, out=None, max_depth=None):
    """HD, HD95 and ASSD of every row, on the device: surface_points, surface_dist, ONE torch.sort of the int64 keys (non-negative
    fp32 values order as their bit patterns) and surface_stats, all enqueued on the current stream; nothing comes to the host.
    cap: the pool of surface points shared by the rows of the call; default surface_default_cap(voxels the rows cover) (rows on the
    device: n * max_depth * H * W). Rows that do not fit are flagged SURFACE_OVERFLOW in the status column with their true counts
    (metrics.surface_table recomputes exactly those). -> out float64 [n, 8] (SURF_COLS)."""
    _surface_spacing(spacing)
    if cap is None:
        if isinstance(rows, torch.Tensor):
            if max_depth is None:
                raise ValueError("rows on the device: max_depth= must be given (the launch is sized from it)")
            covered = rows.shape[0] * int(max_depth) * int(pred.shape[-2]) * int(pred.shape[-1])
        else:
            import numpy as np
            r = np.asarray(rows, dtype=np.int64)
            covered = int(r.reshape(-1, 5)[:, 4].clip(min=0).sum()) * int(pred.shape[-2]) * int(pred.shape[-1]) if r.size else 0
        cap = surface_default_cap(covered)
    work = surface_points(pred, label, rows, cap, max_depth=max_depth)
    surface_dist(work, spacing, keys=True)
    return surface_stats(torch.sort(work["keys"])[0], work, out=out)


def normalize_chw(x, mean3, std3, out=None):
    """(x - mean[c]) / std[c] on [B,3,H,W]; x uint8 or fp32."""
    import ctypes
    assert x.is_cuda and x.is_contiguous() and x.dim() == 4 and x.shape[1] == 3
    assert x.dtype in (torch.uint8, torch.float32)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean3])
    s = (ctypes.c_float * 3)(*[float(v) for v in std3])
    st = _lib.lib().psam_normalize_chw(_ptr(x), 1 if x.dtype == torch.uint8 else 0, x.shape[0],
                                      x.shape[2] * x.shape[3], m, s, _ptr(out), _stream())
    _lib.check(st, "psam_normalize_chw")
    return out



INTAKE_MAX_SIDE, INTAKE_MAX_SCALE = 8192, 16        # the size range of psam_image_intake (csrc/intake.hip)


def intake_shape(h, w, S):
    """(oh, ow) of an [h, w] image resized so that its long side is S: `ResizeLongestSide.get_preprocess_shape`."""
    scale = S * 1.0 / max(h, w)
    return (int(h * scale + 0.5), int(w * scale + 0.5))


def intake_supported(h, w, S):
    """whether psam_image_intake serves an [h, w] source at model size S (sides 1..8192, at most 16 source pixels per resized one)"""
    if not (1 <= h <= INTAKE_MAX_SIDE and 1 <= w <= INTAKE_MAX_SIDE and S >= 1):
        return False
    oh, ow = intake_shape(h, w, S)
    return 1 <= oh <= S and 1 <= ow <= S and h <= INTAKE_MAX_SCALE * oh and w <= INTAKE_MAX_SCALE * ow


def image_intake_packed(buf, rows, C, S, mode, mean3, std3, threshold=False, out=None):
    """psam_image_intake on images already packed in the uint8 device buffer `buf`; rows: per image (byte offset, H, W, oh, ow).
    -> out fp32 [n, C, S, S]."""
    import ctypes
    _req(buf, torch.uint8, "buf")
    assert buf.is_contiguous() and buf.dim() == 1
    n = len(rows)
    flat = [int(v) for r in rows for v in r]
    assert len(flat) == 5 * n
    rows_host = (ctypes.c_longlong * max(len(flat), 1))(*flat)
    rows_dev = torch.empty((max(n, 1), 5), dtype=torch.int64, device=buf.device)
    if out is None:
        out = torch.empty((n, C, max(S, 0), max(S, 0)), dtype=torch.float32, device=buf.device)
    _req(out, torch.float32, "out")
    assert out.is_contiguous() and out.numel() >= n * C * max(S, 0) * max(S, 0)
    m = None if mean3 is None else (ctypes.c_float * 3)(*[float(v) for v in mean3])
    sd = None if std3 is None else (ctypes.c_float * 3)(*[float(v) for v in std3])
    st = _lib.lib().psam_image_intake(_ptr(buf), buf.numel(), rows_host, _ptr(rows_dev), n, C, S, int(mode), 1 if threshold else 0,
                                     m, sd, _ptr(out), _stream())
    _lib.check(st, "psam_image_intake")
    return out


def image_intake(images, S, mode, mean3, std3, threshold=False, out=None):
    """Resize + normalise + zero-pad a list of uint8 device images of any sizes in one launch (psam_image_intake).
    images: uint8 device tensors, all [H, W, 3] (interleaved RGB) or all [H, W]. Each is resized to (oh, ow) =
    get_preprocess_shape(H, W, S). mode 0: aten antialiased bilinear (bit-identical to float -> resize_aa -> normalize_chw -> pad);
    mode 1: Pillow's BILINEAR resize of the uint8 image, exactly. threshold (masks, mode 0): v > 0.5 ? 1 : 0 instead of the
    normalisation. -> (out fp32 [n, C, S, S], [(oh, ow)])."""
    if not images:
        raise ValueError("images: expected at least one image")
    C = 3 if images[0].dim() == 3 else 1
    rows, sizes, flat, off = [], [], [], 0
    for k, im in enumerate(images):
        _req(im, torch.uint8, f"images[{k}]")
        if (im.dim() == 3 and im.shape[2] == 3) != (C == 3) or im.dim() not in (2, 3):
            raise ValueError(f"images[{k}]: expected {'[H, W, 3]' if C == 3 else '[H, W]'}, got {tuple(im.shape)}")
        h, w = int(im.shape[0]), int(im.shape[1])
        oh, ow = intake_shape(h, w, S) if h > 0 and w > 0 and S > 0 else (0, 0)
        rows.append((off, h, w, oh, ow))
        sizes.append((oh, ow))
        flat.append(im.contiguous().reshape(-1))
        off += h * w * C
    buf = flat[0] if len(flat) == 1 else torch.cat(flat)
    if buf.numel() == 0:
        buf = torch.zeros((1,), dtype=torch.uint8, device=images[0].device)        # (an empty image: the launcher refuses its row)
    return image_intake_packed(buf, rows, C, S, mode, mean3, std3, threshold, out), sizes


# ---- HIP graph replay of a launch-only forward -------------------------------------------------------------------
def graph_wanted(x, max_batch_rows):
    """PSAM_HIPGRAPH = auto (default: small calls only) / 1 / 0. Never while per-kernel timers are attached (they need the launches
    themselves) or inside another capture."""
    import os
    mode = os.environ.get("PSAM_HIPGRAPH", "auto")
    if mode == "0" or not x.is_cuda or torch.cuda.is_current_stream_capturing():
        return False
    if TIMERS or GEMM_TIMER is not None:
        return False
    return mode == "1" or x.shape[0] <= max_batch_rows


class GraphCache:
    """fn(static_input) -> output living in a persistent workspace, captured once per key and replayed: one host call instead of the
    forward's hundred-odd launches. A failed capture (a runtime that cannot record these launches) falls back to eager, once."""

    def __init__(self, what, limit=4):
        self.what, self.limit, self.graphs = what, limit, {}

    def run(self, key, x, fn):
        """x: a tensor or a tuple of tensors (the inputs that change from call to call: copied into static clones); fn(*statics)."""
        xs = x if isinstance(x, (tuple, list)) else (x,)
        ent = self.graphs.get(key)
        if ent is None:
            if len(self.graphs) >= self.limit:
                self.graphs.clear()
            statics = tuple(t.contiguous().clone() for t in xs)
            try:
                # warm-up outside the capture (work lists, workspaces and weight packs are built on first use), then the capture
                dev = xs[0].device
                cur = torch.cuda.current_stream(dev)
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    fn(*statics)
                cur.wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = fn(*statics)
                ent = self.graphs[key] = (g, statics, out)
            except Exception as e:
                import sys
                ent = self.graphs[key] = (None, None, None)
                print(f"protosam_amd: HIP graph capture of {self.what} failed ({e!r}); running eagerly", file=sys.stderr)
        g, statics, out = ent
        if g is None:
            return None
        for st, t in zip(statics, xs):
            st.copy_(t)
        g.replay()
        return out

# ---- connected components --------------------------------------------------------------------------------------
CC_HDR, CC_STRIDE = 8, 12


class CclWorkspace:
    """Scratch for psam_ccl plus `slots` result tables (one per image of a batch), and their pinned host mirror."""

    def __init__(self, H, W, cap, device, slots=1):
        n = H * W
        self.H, self.W, self.cap, self.slots = H, W, cap, slots
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=device)  # noqa: E731
        # every scratch array `slots` times (ccl_batch works on all images of a batch at once; ccl on image 0's part)
        self.parent_b, self.labels_b = i32(slots * n).view(slots, n), i32(slots * n).view(slots, n)
        self.counters_b, self.roots_b, self.acc_i_b = i32(slots * 2), i32(slots * cap), i32(slots * 5 * cap)
        self.acc_u_b = torch.empty(slots * 3 * cap, dtype=torch.int64, device=device)
        self.acc_d_b = torch.empty(slots * cap, dtype=torch.float64, device=device)
        self.parent, self.labels, self.counters, self.roots = self.parent_b[0], self.labels_b[0], self.counters_b[:2], self.roots_b[:cap]
        self.acc_i, self.acc_u, self.acc_d = self.acc_i_b[:5 * cap], self.acc_u_b[:3 * cap], self.acc_d_b[:cap]
        self.tabs = torch.zeros((slots, CC_HDR + CC_STRIDE * cap), dtype=torch.float64, device=device)
        self.tabs_host = torch.empty((slots, CC_HDR + CC_STRIDE * cap), dtype=torch.float64).pin_memory()

    @property
    def tab(self):
        return self.tabs[0]

    @property
    def tab_host(self):
        return self.tabs_host[0]


def ccl(pred_u8, pfg, ws, fg_sum=None, slot=0):
    """pred uint8 [H,W], pfg fp32 [H,W] -> ws.labels (int32 [H*W]) and ws.tabs[slot] (fp64 table, see csrc/ccl.hip)."""
    assert pred_u8.dtype == torch.uint8 and pred_u8.is_cuda and pred_u8.is_contiguous()
    _req(pfg, torch.float32, "pfg")
    h = _tstart("ccl")
    st = _lib.lib().psam_ccl(_ptr(pred_u8), _ptr(pfg), ws.H, ws.W, ws.cap, _ptr(ws.labels), _ptr(ws.parent),
                            _ptr(ws.counters), _ptr(ws.roots), _ptr(ws.acc_i), _ptr(ws.acc_u), _ptr(ws.acc_d),
                            _ptr(fg_sum), _ptr(ws.tabs[slot]), _stream())
    _tstop(h, ws.H * ws.W * (1 + 4 + 4))      # pred u8 + p_fg fp32 in, labels int32 out (the table is a few KB)
    _lib.check(st, "psam_ccl")
    return ws


def ccl_batch(pred_u8, prob, ws, fg_sum=None):
    """pred uint8 [B,H,W], prob fp32 [B,2,H,W] (foreground = channel 1) -> ws.labels_b[b], ws.tabs[b] for every image in ONE chain of
    six launches (psam_ccl_batch)."""
    B = pred_u8.shape[0]
    assert pred_u8.dtype == torch.uint8 and pred_u8.is_cuda and pred_u8.is_contiguous() and B <= ws.slots
    _req(prob, torch.float32, "prob")
    assert prob.is_contiguous() and prob.shape[1] == 2
    h = _tstart("ccl")
    st = _lib.lib().psam_ccl_batch(_ptr(pred_u8), _ptr(prob[0, 1]), 2 * ws.H * ws.W, B, ws.H, ws.W, ws.cap, _ptr(ws.labels_b),
                                  _ptr(ws.parent_b), _ptr(ws.counters_b), _ptr(ws.roots_b), _ptr(ws.acc_i_b), _ptr(ws.acc_u_b),
                                  _ptr(ws.acc_d_b), _ptr(fg_sum), _ptr(ws.tabs), _stream())
    _tstop(h, B * ws.H * ws.W * (1 + 4 + 4))
    _lib.check(st, "psam_ccl_batch")
    return ws


def ccl_planes(pred_u8, pfg, ws, fg_sum=None):
    """`ccl_batch` on planes whose foreground probability is a plane of its own: pred uint8 [B,H,W], pfg fp32 [B,H,W] (e.g.
    prob2_argmax's pfg2) -> ws.labels_b[b], ws.tabs[b]."""
    B = pred_u8.shape[0]
    assert pred_u8.dtype == torch.uint8 and pred_u8.is_cuda and pred_u8.is_contiguous() and B <= ws.slots
    _req(pfg, torch.float32, "pfg")
    assert pfg.is_contiguous() and pfg.shape[0] == B and pfg[0].numel() == ws.H * ws.W
    h = _tstart("ccl")
    st = _lib.lib().psam_ccl_batch(_ptr(pred_u8), _ptr(pfg), ws.H * ws.W, B, ws.H, ws.W, ws.cap, _ptr(ws.labels_b),
                                  _ptr(ws.parent_b), _ptr(ws.counters_b), _ptr(ws.roots_b), _ptr(ws.acc_i_b), _ptr(ws.acc_u_b),
                                  _ptr(ws.acc_d_b), _ptr(fg_sum), _ptr(ws.tabs), _stream())
    _tstop(h, B * ws.H * ws.W * (1 + 4 + 4))
    _lib.check(st, "psam_ccl_batch")
    return ws


def neg_points(ws, pbg, tab, max_comp, r=10, thr=0.95, keys=None, labels=None):
    """int64 keys [max_comp+1] (see psam_neg_points) from ws.labels (the CCL of the SAME image) and p_bg fp32 [H,W]."""
    _req(pbg, torch.float32, "pbg")
    assert pbg.is_contiguous() and tab.dtype == torch.float64
    if keys is None:
        keys = torch.empty(max_comp + 1, dtype=torch.int64, device=pbg.device)
    st = _lib.lib().psam_neg_points(_ptr(ws.labels if labels is None else labels), _ptr(pbg), _ptr(tab), ws.H, ws.W, max_comp, r,
                                   float(thr), _ptr(keys), _stream())
    _lib.check(st, "psam_neg_points")
    return keys


def neg_points_batch(labels, pbg, tabs, max_comp, r=10, thr=0.95, keys=None):
    """`neg_points` for P planes in one launch (psam_neg_points_batch): labels int32 [P,H*W] or [P,H,W] (psam_ccl_batch's,
    e.g. ws.labels_b[:P]), p_bg fp32 [P,H,W] view with any plane stride (channel 0 of a [P,2,H,W] probability map), tabs fp64
    [P, 8 + 12*cap] -> int64 keys [P, max_comp+1], row p = `neg_points` of plane p."""
    _req(pbg, torch.float32, "pbg")
    assert labels.dtype == torch.int32 and labels.is_cuda and labels.is_contiguous()
    assert tabs.dtype == torch.float64 and tabs.is_cuda and tabs.is_contiguous() and tabs.dim() == 2
    P, H, W = pbg.shape
    assert pbg.stride(1) == W and labels.numel() == P * H * W and tabs.shape[0] == P
    assert (tabs.shape[1] - CC_HDR) % CC_STRIDE == 0
    cap = (tabs.shape[1] - CC_HDR) // CC_STRIDE
    if keys is None:
        keys = torch.empty((P, max_comp + 1), dtype=torch.int64, device=pbg.device)
    assert keys.dtype == torch.int64 and keys.is_contiguous() and keys.numel() >= P * (max_comp + 1)
    st = _lib.lib().psam_neg_points_batch(_ptr(labels), _ptr(pbg), pbg.stride(0), _ptr(tabs), cap, P, H, W, max_comp, r,
                                          float(thr), _ptr(keys), _stream())
    _lib.check(st, "psam_neg_points_batch")
    return keys


def decode_point_key(key, W):
    """key (python int, possibly negative from the int64 view) -> (x, y, p) or None."""
    key &= (1 << 64) - 1
    if key == 0:
        return None
    import struct
    idx = 0xFFFFFFFF - (key & 0xFFFFFFFF)
    return idx % W, idx // W, struct.unpack("<f", struct.pack("<I", key >> 32))[0]


_topk_scratch = {}


def topk_points_workspace(P, max_comp, only_best=False):
    """Bytes of scratch psam_topk_points(_batch) needs for P planes (psam_topk_points_workspace)."""
    nbytes = _lib.c_longlong(0)
    _lib.check(_lib.lib().psam_topk_points_workspace(P, max_comp, 1 if only_best else 0, nbytes), "psam_topk_points_workspace")
    return nbytes.value


def _topk_workspace(P, max_comp, only_best, device):
    """int64 scratch of topk_points_workspace bytes, one per (device, planes, rows) seen. Calls on one stream share it in order."""
    key = (str(device), P, max_comp, bool(only_best))
    if key not in _topk_scratch:
        _topk_scratch[key] = torch.empty((topk_points_workspace(P, max_comp, only_best) + 7) // 8, dtype=torch.int64, device=device)
    return _topk_scratch[key]


def topk_points_batch(labels, pfg, tabs, k, max_comp, only_best=False, keys=None, scratch=None):
    """The k most confident pixels of every component of P planes in one launch chain (psam_topk_points_batch): labels int32
    [P,H*W] or [P,H,W] (psam_ccl_batch's, e.g. ws.labels_b[:P]), p_fg fp32 [P,H,W] view with any plane stride (channel 1 of a
    [P,2,H,W] probability map), tabs fp64 [P, 8 + 12*cap] -> int64 keys [P, R, k], R = max_comp or 1 with only_best (the component
    tab[3]): row c = component c's k largest point keys in descending order (largest p_fg first, raster order among equals), zeros
    behind a component of fewer than k pixels and in the rows of components that do not exist. `scratch`: int64 tensor of
    topk_points_workspace bytes (default: cached per shape)."""
    _req(pfg, torch.float32, "pfg")
    assert labels.dtype == torch.int32 and labels.is_cuda and labels.is_contiguous()
    assert tabs.dtype == torch.float64 and tabs.is_cuda and tabs.is_contiguous() and tabs.dim() == 2
    P, H, W = pfg.shape
    assert pfg.stride(1) == W and labels.numel() == P * H * W and tabs.shape[0] == P
    assert (tabs.shape[1] - CC_HDR) % CC_STRIDE == 0
    cap = (tabs.shape[1] - CC_HDR) // CC_STRIDE
    R = 1 if only_best else max_comp
    if keys is None:
        keys = torch.empty((P, R, k), dtype=torch.int64, device=pfg.device)
    assert keys.dtype == torch.int64 and keys.is_cuda and keys.is_contiguous() and keys.numel() >= P * R * k
    if scratch is None:
        scratch = _topk_workspace(P, max_comp, only_best, pfg.device)
    assert scratch.dtype == torch.int64 and scratch.is_cuda and scratch.is_contiguous()
    st = _lib.lib().psam_topk_points_batch(_ptr(labels), _ptr(pfg), pfg.stride(0), _ptr(tabs), cap, P, H, W, k, max_comp,
                                           1 if only_best else 0, _ptr(keys), _ptr(scratch), scratch.numel() * 8, _stream())
    _lib.check(st, "psam_topk_points_batch")
    return keys


def topk_points(ws, pfg, tab, k, max_comp, only_best=False, keys=None, labels=None, scratch=None):
    """int64 keys [R, k] (see topk_points_batch) of one plane: ws.labels (the CCL of the SAME image; or `labels`), p_fg fp32
    [H,W], tab the fp64 table of that labelling (capacity ws.cap)."""
    _req(pfg, torch.float32, "pfg")
    assert pfg.is_contiguous() and tab.dtype == torch.float64 and tab.is_cuda and tab.is_contiguous()
    assert tab.numel() == CC_HDR + CC_STRIDE * ws.cap and pfg.numel() == ws.H * ws.W
    labels = ws.labels if labels is None else labels
    assert labels.dtype == torch.int32 and labels.is_cuda and labels.is_contiguous() and labels.numel() == ws.H * ws.W
    R = 1 if only_best else max_comp
    if keys is None:
        keys = torch.empty((R, k), dtype=torch.int64, device=pfg.device)
    assert keys.dtype == torch.int64 and keys.is_cuda and keys.is_contiguous() and keys.numel() >= R * k
    if scratch is None:
        scratch = _topk_workspace(1, max_comp, only_best, pfg.device)
    assert scratch.dtype == torch.int64 and scratch.is_cuda and scratch.is_contiguous()
    st = _lib.lib().psam_topk_points(_ptr(labels), _ptr(pfg), _ptr(tab), ws.cap, ws.H, ws.W, k, max_comp, 1 if only_best else 0,
                                     _ptr(keys), _ptr(scratch), scratch.numel() * 8, _stream())
    _lib.check(st, "psam_topk_points")
    return keys


def decode_topk_keys(row, W):
    """One row of topk_points keys (ints, possibly negative from the int64 view) -> [(x, y, p), ...] in the row's order, up to the
    first 0 (a component of fewer pixels than the row has slots)."""
    out = []
    for key in row:
        pt = decode_point_key(int(key), W)
        if pt is None:
            break
        out.append(pt)
    return out


def volume_stats(vol, vol_dtype, slope=1.0, inter=0.0):
    """fp64 [2] = {sum(x), sum(x^2)} of x = voxel*slope + inter over a raw device volume (psam_volume_stats)."""
    assert vol.is_cuda and vol.is_contiguous()
    out = torch.empty(2, dtype=torch.float64, device=vol.device)
    st = _lib.lib().psam_volume_stats(_ptr(vol), vol_dtype, vol.numel(), float(slope), float(inter), _ptr(out), _stream())
    _lib.check(st, "psam_volume_stats")
    return out


def volume_slices(vol, vol_dtype, Z, H, W, slope, inter, mean, inv_std, S, tile, mode, out=None):
    """fp32 [Z,tile,S,S]: normalise + cv2-style resize (mode 0 linear, 1 nearest) + channel tiling (psam_volume_slices)."""
    assert vol.is_cuda and vol.is_contiguous()
    if out is None:
        out = torch.empty((Z, tile, S, S), dtype=torch.float32, device=vol.device)
    st = _lib.lib().psam_volume_slices(_ptr(vol), vol_dtype, Z, H, W, float(slope), float(inter), float(mean), float(inv_std),
                                      S, tile, mode, _ptr(out), _stream())
    _lib.check(st, "psam_volume_slices")
    return out


def bilinear_tokens(tok, in_bstride, ld, B, ih, iw, C, oh, ow, out=None):
    """fp32 token-major [B][ih*iw, C] (strided) -> contiguous [B, oh*ow, C]."""
    _req(tok, torch.float32, "tok")
    if out is None:
        out = torch.empty((B, oh * ow, C), dtype=torch.float32, device=tok.device)
    st = _lib.lib().psam_bilinear_tokens(_ptr(tok), in_bstride, ld, B, ih, iw, C, oh, ow, _ptr(out), _stream())
    _lib.check(st, "psam_bilinear_tokens")
    return out
