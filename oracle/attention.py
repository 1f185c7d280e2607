"""Float64 reference for the attention kernels of csrc/attention.hip (`ops.attention`, modes 0 / 1 / 2), a model of the roundings those
kernels document, inputs on which every key, every query row and every rel-pos table row is pinned individually, and the checks the
GPU tests hold the kernels to. Test infrastructure only (see oracle/__init__.py); no HIP, torch on CPU or GPU tensors.

  mode 0  softmax(scale q k^T) v over all N tokens
  mode 1  + q . Rh[qy - ky + gh - 1] + q . Rw[qx - kx + gw - 1] on a gh x gw map, the terms from the UNSCALED q
          (image_encoder.py:337-372, restated here in index form; tests/test_attention_reference_cpu.py pins it to
          oracle.sam_image_encoder.decomposed_rel_pos_terms)
  mode 2  the same inside 14 x 14 windows over the gh x gw map (image_encoder.py:254-300): positions beyond the map carry `pad_row`
          (q, k and v), the result is un-partitioned to [B, N, H * hd]

Everything works on one (image, head) at a time: an N = 4096 case holds one [N, N] float64 matrix (and its temporaries) at a time.

tests/test_attention_reference_cpu.py pins the reference to stock torch and shows, by injecting faults into the float64 arithmetic
(`fault=`), that the checks below catch what a 2e-3 tolerance passes; tests/test_attention_exact_gpu.py holds the kernels to them.
"""
import math
from types import SimpleNamespace

import torch

WS = 14
MARGIN_NATS = 32.0          # every non-target P is exactly zero in fp16 even against a running maximum that lags by 2^8
U16 = 2.0 ** -11            # unit roundoff of fp16
TINY16 = 2.0 ** -24         # smallest fp16 subnormal: what a P that underflows can lose per key
RMS_FACTOR = 3.0

# what a wrong map from workgroup id to (image, head, window or query block) does: the arithmetic of every item is right, its place
# is not. An item is one (image, head, window) in mode 2 and one (image, head, block of `item_rows` queries) in modes 0 / 1.
ITEM_FAULTS = ("drop_item", "swap_heads", "wrong_image", "repeat_item_skip_next")
FAULTS = ("drop_key", "phantom_tail", "swap_keys", "relh_transposed", "rel_row_off_by_one", "rel_scaled_q", "pad_key_zero",
          "unpartition_shift") + ITEM_FAULTS


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def window_tokens(gh, gw, ws=WS):
    """[nW, ws * ws] int64: the token index y * gw + x of every position of every window, windows row-major, -1 beyond the map."""
    nwy, nwx = -(-gh // ws), -(-gw // ws)
    y = torch.arange(nwy * ws).view(nwy, 1, ws, 1)
    x = torch.arange(nwx * ws).view(1, nwx, 1, ws)
    tok = torch.where((y < gh) & (x < gw), y * gw + x, torch.full_like(y * x, -1))
    return tok.reshape(nwy * nwx, ws * ws)


def n_keys(mode, N, ws=WS):
    """keys per query: N, or ws * ws for windows."""
    return ws * ws if mode == 2 else N


def phantom_count(n):
    """keys of the 64-key tail tile beyond the n real ones."""
    return 64 * (-(-n // 64)) - n


def _regions(mode, N, gh, gw, ws, device):
    """-> (tok [G, n] token of every key / query slot or -1, (rh, rw) the region the rel-pos terms index, or None)."""
    if mode == 2:
        return window_tokens(gh, gw, ws).to(device), (ws, ws)
    tok = torch.arange(N, device=device).view(1, N)
    return tok, ((gh, gw) if mode == 1 else None)


def _gather_rel(t, idx):
    """t [G, n, R] (q against every table row), idx [n, K] -> [G, n, K]."""
    return t.gather(2, idx.unsqueeze(0).expand(t.shape[0], -1, -1))


def _rel_index(n, rh, rw, device, fault):
    a = torch.arange(n, device=device)
    qy, qx = a // rw, a % rw
    ih = qy[:, None] - torch.arange(rh, device=device)[None, :] + rh - 1
    iw = qx[:, None] - torch.arange(rw, device=device)[None, :] + rw - 1
    if fault == "relh_transposed":
        ih = torch.arange(rh, device=device)[None, :] - qy[:, None] + rh - 1
    if fault == "rel_row_off_by_one":
        ih, iw = (ih + 1).clamp(max=2 * rh - 2), (iw + 1).clamp(max=2 * rw - 2)
    return ih, iw


def item_slots(mode, N, gh=0, gw=0, item_rows=256, ws=WS, device="cpu"):
    """[items per (image, head), slots] int64: the token of every query slot of every item, -1 where the slot holds no token (beyond
    the map in a window, beyond N in the last query block)."""
    if mode == 2:
        return window_tokens(gh, gw, ws).to(device)
    nqb = -(-N // item_rows)
    t = torch.arange(nqb * item_rows, device=device).view(nqb, item_rows)
    return torch.where(t < N, t, torch.full_like(t, -1))


def item_fault(o, fault, arg, slots, mode, H, hd, guard):
    """o [B, N, H * hd] of the sound arithmetic -> [B + guard, N, H * hd] as a kernel with a broken item map would leave a NaN-filled
    buffer with `guard` images of guard rows behind it.
      drop_item              arg (b, h, r): item r of (b, h) is never run - its rows keep the prefill
      swap_heads             arg (b, h, h2): the results of heads h and h2 of image b exchanged
      wrong_image            arg (b, h, b2): every item of (b, h) computed from image b2's q / k / v
      repeat_item_skip_next  arg (b, h, r): the result of item i = (b, h, r) is also written to the place of item i + 1, which is never
                             run; i + 1 in the order the kernels walk: the next head of the window, then the next window, then the
                             next image (mode 2) / the next query block of the head, then the next head, then the next image"""
    B, N, C = o.shape
    buf = torch.full((B + guard, N, C), float("nan"), dtype=o.dtype, device=o.device)
    buf[:B] = o

    def cols(h):
        return slice(h * hd, (h + 1) * hd)

    if fault == "drop_item":
        b, h, r = arg
        t = slots[r]
        buf[b, t[t >= 0], cols(h)] = float("nan")
    elif fault == "swap_heads":
        b, h, h2 = arg
        assert h != h2
        buf[b, :, cols(h)], buf[b, :, cols(h2)] = o[b, :, cols(h2)], o[b, :, cols(h)]
    elif fault == "wrong_image":
        b, h, b2 = arg
        assert b != b2
        buf[b, :, cols(h)] = o[b2, :, cols(h)]
    else:
        b, h, r = arg
        R = slots.shape[0]
        if mode == 2:
            h2 = (h + 1) % H
            r2 = r + (h2 == 0)
            b2, r2 = b + (r2 == R), r2 % R
        else:
            r2 = (r + 1) % R
            h2 = h + (r2 == 0)
            b2, h2 = b + (h2 == H), h2 % H
        assert b2 < B + guard, "the repeated write falls behind the buffer: give the fault guard rows to land in"
        src, dst = slots[r], slots[r2]
        val = torch.full((slots.shape[1], hd), float("nan"), dtype=o.dtype, device=o.device)
        val[src >= 0] = o[b, src[src >= 0], cols(h)]
        buf[b2, dst[dst >= 0], cols(h2)] = val[dst >= 0]
    return buf


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def reference(qkv, mode, scale=None, Rh=None, Rw=None, pad_row=None, gh=0, gw=0, ws=WS, budget=True, model=False, targets=None,
              fault=None, fault_arg=None, item_rows=256, guard=0):
    """qkv fp16 [B, N, 3, H, hd] (token-major), Rh / Rw fp32 [2 rh - 1, hd] tables (modes 1 / 2), pad_row fp16 [3, H, hd] (mode 2).

    Returns a namespace of float64 tensors:
      o      [B, N, H * hd]  softmax(scale q k^T [+ rel_h + rel_w]) v from the fp16 operands
      A      [B, N, H * hd]  sum_j p_ij |v_jd|                                                          (budget=True)
      ds     [B, H, N]       2^-17 max_j (scale sum_c |q_ic k_jc| + sum_c |q_ic| (|Rh_c| + |Rw_c|))        (budget=True)
      model  [B, N, H * hd]  the same arithmetic with the roundings the kernels document in attention.hip (model=True): scores
                             in fp32, P relative to the row maximum rounded to fp16, the row sum over the rounded P (:60-62),
                             the output rounded to fp16
      margin [B, H, N]       score of the target key minus the largest score of a key that carries another (k, v) row
                             (targets = int64 [B, H, G, n], a key slot per query slot of every region; padded keys of a window
                             all carry pad_row and count as one)
    `fault` (tests only) breaks the float64 arithmetic the way a kernel could: see FAULTS. An ITEM_FAULTS fault leaves the arithmetic
    alone and misplaces whole items (`item_fault`): `o` is then [B + guard, N, H * hd], NaN where nothing was written."""
    assert fault is None or fault in FAULTS
    B, N, three, H, hd = qkv.shape
    assert three == 3 and qkv.dtype == torch.float16
    dev = qkv.device
    scale = hd ** -0.5 if scale is None else scale
    tok, region = _regions(mode, N, gh, gw, ws, dev)
    G, n = tok.shape
    real = tok >= 0
    tokc = tok.clamp(min=0)
    use_rel = region is not None and Rh is not None
    if region is not None:
        assert Rh is not None and Rw is not None and region[0] * region[1] == n
        Rh64, Rw64 = Rh.to(dev).double(), Rw.to(dev).double()
        ih, iw = _rel_index(n, region[0], region[1], dev, fault)
    out = SimpleNamespace(o=torch.zeros((B, N, H * hd), dtype=torch.float64, device=dev), A=None, ds=None, model=None, margin=None)
    if budget:
        out.A = torch.zeros_like(out.o)
        out.ds = torch.zeros((B, H, N), dtype=torch.float64, device=dev)
    if model:
        out.model = torch.zeros_like(out.o)
    if targets is not None:
        out.margin = torch.zeros((B, H, N), dtype=torch.float64, device=dev)
        cls = torch.where(real, tokc, torch.full_like(tok, -1))                                   # [G, n]: padded keys are one class

    def scatter(dst, val, h):                    # val [G, n, hd] -> dst[b][token, h * hd : (h + 1) * hd]
        if fault == "unpartition_shift":
            val = val.roll(1, 0)
        dst[tok[real], h * hd:(h + 1) * hd] = val[real]

    for b in range(B):
        for h in range(H):
            q, k, v = (qkv[b, :, i, h].double() for i in range(3))
            q, k, v = q[tokc], k[tokc], v[tokc]                                                   # [G, n, hd]
            if mode == 2:
                pq, pk, pv = (pad_row[i, h].to(dev).double() for i in range(3))
                if fault == "pad_key_zero":
                    pk, pv = torch.zeros_like(pk), torch.zeros_like(pv)
                m3 = real.unsqueeze(-1)
                q, k, v = torch.where(m3, q, pq), torch.where(m3, k, pk), torch.where(m3, v, pv)
            s = scale * (q @ k.transpose(1, 2))                                                   # [G, n, n]
            if use_rel:
                rh, rw = region
                qr = q * scale if fault == "rel_scaled_q" else q
                rel_h = _gather_rel(qr @ Rh64.t(), ih)                                            # [G, n, rh]
                rel_w = _gather_rel(qr @ Rw64.t(), iw)                                            # [G, n, rw]
                s = (s.view(G, n, rh, rw) + rel_h.unsqueeze(-1) + rel_w.unsqueeze(-2)).view(G, n, n)
            mx = s.max(-1, keepdim=True).values
            e = torch.exp(s - mx)
            extra = 0.0
            if fault == "drop_key":
                e[:, :, fault_arg] = 0.0
            elif fault == "swap_keys":
                j1, j2 = fault_arg
                e[:, :, [j1, j2]] = e[:, :, [j2, j1]]
            elif fault == "phantom_tail":                                                         # zero k: score 0; zero v: nothing added
                extra = phantom_count(n) * torch.exp(-mx)
            l = e.sum(-1, keepdim=True) + extra
            scatter(out.o[b], (e @ v) / l, h)
            if budget:
                scatter(out.A[b], (e @ v.abs()) / l, h)
                sa = scale * (q.abs() @ k.abs().transpose(1, 2))
                if use_rel:
                    ah = _gather_rel(q.abs() @ Rh64.abs().t(), ih)
                    aw = _gather_rel(q.abs() @ Rw64.abs().t(), iw)
                    sa = (sa.view(G, n, rh, rw) + ah.unsqueeze(-1) + aw.unsqueeze(-2)).view(G, n, n)
                out.ds[b, h][tok[real]] = 2.0 ** -17 * sa.max(-1).values[real]
                del sa
            if model:
                s32 = s.float().double()
                p16 = torch.exp(s32 - s32.max(-1, keepdim=True).values).half().double()
                scatter(out.model[b], ((p16 @ v) / p16.sum(-1, keepdim=True)).half().double(), h)
                del s32, p16
            if targets is not None:
                t = targets[b, h].to(dev)                                                         # [G, n]
                st = s.gather(2, t.unsqueeze(-1)).squeeze(-1)
                same = cls.gather(1, t).unsqueeze(-1) == cls.unsqueeze(1)                          # [G, n query, n key]
                other = s.masked_fill(same, -math.inf).max(-1).values
                out.margin[b, h][tok[real]] = (st - other)[real]
            del s, e
    if fault in ITEM_FAULTS:
        out.o = item_fault(out.o, fault, fault_arg, item_slots(mode, N, gh, gw, item_rows, ws, dev), mode, H, hd, guard)
    return out


def rounding_model(qkv, mode, **kw):
    """The reference arithmetic with the kernels' documented roundings (see `reference`): float64 values of an fp16 result."""
    return reference(qkv, mode, budget=False, model=True, **kw).model


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _directions(shape, norm, g):
    """random directions of the given norm along the last axis, float64."""
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    return x * (norm / x.norm(dim=-1, keepdim=True))


def _geometry(mode, N, gh, gw):
    if mode == 0:
        assert N > 0
        return N, 0, 0
    assert gh > 0 and gw > 0
    return gh * gw, gh, gw


def _case(mode, qkv, B, H, hd, gh, gw, dev, **kw):
    c = SimpleNamespace(mode=mode, qkv=qkv.to(dev).contiguous(), B=B, N=qkv.shape[1], H=H, hd=hd, scale=hd ** -0.5, gh=gh, gw=gw,
                        Rh=None, Rw=None, pad_row=None, targets=None, expected=None, c=None)
    for name, val in kw.items():
        setattr(c, name, val.to(dev).contiguous() if torch.is_tensor(val) else val)
    return c


def ref_kwargs(case):
    """what `reference` / `rounding_model` take besides (qkv, mode)."""
    return dict(scale=case.scale, Rh=case.Rh, Rw=case.Rw, pad_row=case.pad_row, gh=case.gh, gw=case.gw)


def _tables(mode, gh, gw, hd, g, std):
    """fp32 (2 side - 1, hd) tables: of the map for mode 1, of the window for mode 2; none for mode 0."""
    if mode == 0:
        return None, None
    rh, rw = (WS, WS) if mode == 2 else (gh, gw)
    return (torch.randn((2 * rh - 1, hd), generator=g) * std, torch.randn((2 * rw - 1, hd), generator=g) * std)


def _permutations(B, H, G, n, g):
    """[B, H, G, n]: a random permutation of the n key slots per region; never the identity where n > 1."""
    t = torch.empty((B, H, G, n), dtype=torch.int64)
    for i in range(B * H * G):
        p = torch.randperm(n, generator=g)
        if n > 1 and bool((p == torch.arange(n)).all()):
            p = p.roll(1)
        t.view(-1, n)[i] = p
    return t


def _selector_expected(mode, qkv, pad_row, targets, gh, gw):
    """fp16 [B, N, H * hd]: the v row of every query's target key (pad_row's v for a padded target)."""
    B, N, _, H, hd = qkv.shape
    tok, _ = _regions(mode, N, gh, gw, WS, qkv.device)
    real = tok >= 0
    exp = torch.zeros((B, N, H, hd), dtype=torch.float16)
    for b in range(B):
        for h in range(H):
            kt = tok.gather(1, targets[b, h])                                                     # token of the target key, or -1
            v = qkv[b, :, 2, h][kt.clamp(min=0)]
            if mode == 2:
                v = torch.where((kt >= 0).unsqueeze(-1), v, pad_row[2, h])
            exp[b, tok[real], h] = v[real]
    return exp.reshape(B, N, H * hd)


def selector_qk(mode, B, H, hd, N=0, gh=0, gw=0, seed=0, device="cpu", gain=16.0):
    """QK selector: k rows are random directions of norm sqrt(hd) rounded to fp16, q_i = gain * k_pi(i) (exact in fp16 for a power of
    two), v random, rel tables zero. Every query's softmax is one-hot on its target, the targets form a permutation per region (the
    whole sequence, or each window's 196 positions). pad_row's k is one more such row; padded queries select nothing."""
    N, gh, gw = _geometry(mode, N, gh, gw)
    g = _gen(seed)
    k = _directions((B, N, H, hd), math.sqrt(hd), g).half()
    v = torch.randn((B, N, H, hd), generator=g).half()
    pad = None
    if mode == 2:
        pad = torch.stack([torch.randn((H, hd), generator=g).half(), _directions((H, hd), math.sqrt(hd), g).half(),
                           torch.randn((H, hd), generator=g).half()])
    tok, _ = _regions(mode, N, gh, gw, WS, "cpu")
    G, n = tok.shape
    targets = _permutations(B, H, G, n, g)
    q = torch.zeros((B, N, H, hd), dtype=torch.float16)
    real = tok >= 0
    for b in range(B):
        for h in range(H):
            kt = tok.gather(1, targets[b, h])
            kk = k[b, :, h][kt.clamp(min=0)]
            if mode == 2:
                kk = torch.where((kt >= 0).unsqueeze(-1), kk, pad[1, h])
            q[b, tok[real], h] = (kk[real].float() * gain).half()
    qkv = torch.stack([q, k, v], dim=2)
    Rh, Rw = _tables(mode, gh, gw, hd, g, 0.0)
    return _case(mode, qkv, B, H, hd, gh, gw, device, Rh=Rh, Rw=Rw, pad_row=pad, targets=targets,
                 expected=_selector_expected(mode, qkv, pad, targets, gh, gw))


def selector_relpos(mode, B, H, hd, gh, gw, seed=0, device="cpu", gain=2.0):
    """Rel-pos selector (modes 1 / 2): every k row, pad_row's included, is one small random vector - QK adds a per-query constant
    that softmax cancels while the K path still runs; Rh rows live in channels [0, hd / 2), Rw rows in [hd / 2, hd), each a random
    direction of norm sqrt(hd); q_i = gain * (Rh[qy - ky + rh - 1] + Rw[qx - kx + rw - 1]) for the target (ky, kx) = pi(i), positions
    and sides those of the map (mode 1) or of the window (mode 2). Pins orientation and offset of both table gathers for every
    (query row, key row) pair."""
    assert mode in (1, 2)
    N, gh, gw = _geometry(mode, 0, gh, gw)
    g = _gen(seed)
    rh, rw = (WS, WS) if mode == 2 else (gh, gw)
    Rh = torch.zeros((2 * rh - 1, hd), dtype=torch.float64)
    Rw = torch.zeros((2 * rw - 1, hd), dtype=torch.float64)
    Rh[:, :hd // 2] = _directions((2 * rh - 1, hd // 2), math.sqrt(hd), g)
    Rw[:, hd // 2:] = _directions((2 * rw - 1, hd - hd // 2), math.sqrt(hd), g)
    Rh, Rw = Rh.float(), Rw.float()
    k0 = (torch.randn((H, hd), generator=g) * 0.25).half()
    k = k0.view(1, 1, H, hd).expand(B, N, H, hd)
    v = torch.randn((B, N, H, hd), generator=g).half()
    pad = None
    if mode == 2:
        pad = torch.stack([torch.randn((H, hd), generator=g).half(), k0, torch.randn((H, hd), generator=g).half()])
    tok, _ = _regions(mode, N, gh, gw, WS, "cpu")
    G, n = tok.shape
    targets = _permutations(B, H, G, n, g)
    a = torch.arange(n)
    qy, qx = (a // rw).view(1, n), (a % rw).view(1, n)
    q = torch.zeros((B, N, H, hd), dtype=torch.float16)
    real = tok >= 0
    for b in range(B):
        for h in range(H):
            t = targets[b, h]                                                                     # [G, n] key slots
            rows = gain * (Rh.double()[qy - t // rw + rh - 1] + Rw.double()[qx - t % rw + rw - 1])
            q[b, tok[real], h] = rows[real].half()
    qkv = torch.stack([q, k, v], dim=2)
    return _case(mode, qkv, B, H, hd, gh, gw, device, Rh=Rh, Rw=Rw, pad_row=pad, targets=targets,
                 expected=_selector_expected(mode, qkv, pad, targets, gh, gw))


def spike(qkv, mode, gh, gw):
    """In place, on the fp32 qkv before it is rounded: keys aligned with a query far beyond the 2^8 lazy-rescale threshold, late in
    the key order - the patterns of tests/test_kernels_core_gpu.py (global: the last key, one 70 from the end, the middle, an early
    one for the last query; windows: the last key of window 0 for query 0, a middle key of it for the query at (1, 3))."""
    N = qkv.shape[1]
    if mode == 2:
        last = min(13, gh - 1) * gw + min(13, gw - 1)
        pairs = ((0, last, 25.0), (gw + 3, 5 * gw + 6, 40.0))
    else:
        pairs = ((17, N - 1, 40.0), (70, N - 70, 25.0), (N - 3, N // 2, 60.0), (N - 1, 3, 30.0))
    for qi, ki, gain in pairs:
        qkv[0, ki % N, 1, 0] = qkv[0, qi % N, 0, 0] * gain
    return qkv


def diffuse(mode, B, H, hd, N=0, gh=0, gw=0, std=0.5, seed=0, device="cpu", spiky=False, table_std=0.3):
    """q, k, v at std * randn (optionally with the spike pattern), rel tables at table_std * randn where the mode has them."""
    N, gh, gw = _geometry(mode, N, gh, gw)
    g = _gen(seed)
    qkv = torch.randn((B, N, 3, H, hd), generator=g) * std
    if spiky:
        spike(qkv, mode, gh, gw)
    pad = (torch.randn((3, H, hd), generator=g) * std).half() if mode == 2 else None
    Rh, Rw = _tables(mode, gh, gw, hd, g, table_std)
    return _case(mode, qkv.half(), B, H, hd, gh, gw, device, Rh=Rh, Rw=Rw, pad_row=pad)


def constant_v(mode, B, H, hd, N=0, gh=0, gw=0, seed=0, device="cpu", spiky=False):
    """Every v row, pad_row's included, is one fp16 vector c per head with |c_d| in [0.5, 2) and mixed signs; q, k at 0.5 * randn,
    once diffuse and once with the spike pattern. Any correct softmax returns c. (c differs between heads, not between images: a
    result on the wrong head fails here, one from the wrong image only on the selectors.)"""
    case = diffuse(mode, B, H, hd, N, gh, gw, 0.5, seed, "cpu", spiky)
    g = _gen(seed + 7919)
    mag = 0.5 + 1.49 * torch.rand((H, hd), generator=g)
    sign = torch.where(torch.rand((H, hd), generator=g) < 0.5, -1.0, 1.0)
    c = (mag * sign).half()
    assert float(c.abs().min()) >= 0.5 and float(c.abs().max()) < 2.0 and bool((c > 0).any()) and bool((c < 0).any())
    case.qkv[:, :, 2] = c
    if mode == 2:
        case.pad_row[2] = c
    case.c = c
    for name in ("qkv", "pad_row", "Rh", "Rw", "c"):
        val = getattr(case, name)
        if val is not None:
            setattr(case, name, val.to(device).contiguous())
    return case


# ---- checks ------------------------------------------------------------------------------------------------------------------
def _where(flat_index, N, H, hd):
    b, r = divmod(int(flat_index), N * H * hd)
    i, r = divmod(r, H * hd)
    h, d = divmod(r, hd)
    return b, h, i, d


def _ordinal(x):
    """fp16 -> int32 that counts representable values: adjacent fp16 numbers differ by one."""
    bits = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(bits < 0, -(bits & 0x7fff), bits)


def _finite(out, N, H, hd):
    bad = ~torch.isfinite(out.float())
    if bool(bad.any()):
        b, h, i, d = _where(bad.flatten().nonzero()[0], N, H, hd)
        raise AssertionError(f"not finite at image {b}, head {h}, query {i}, channel {d}")


def check_selector(out, case):
    """out fp16 [B, N, H * hd] against the selector case's expected v rows: every element within one fp16 ulp. Returns the number of
    elements that are not bit-equal; raises with the first offending (image, head, query, key, channel)."""
    exp = case.expected.to(out.device)
    assert out.dtype == torch.float16 and out.shape == exp.shape, (out.dtype, out.shape, exp.shape)
    B, N, H, hd = case.B, case.N, case.H, case.hd
    _finite(out, N, H, hd)
    dist = (_ordinal(out) - _ordinal(exp)).abs()
    bad = dist > 1
    if bool(bad.any()):
        b, h, i, d = _where(bad.flatten().nonzero()[0], N, H, hd)
        tok, _ = _regions(case.mode, N, case.gh, case.gw, WS, "cpu")
        reg, slot = (tok == i).nonzero()[0].tolist()
        key = int(tok[reg, int(case.targets[b, h, reg, slot])])
        raise AssertionError(f"image {b}, head {h}, query {i} (target key {key if key >= 0 else 'pad_row'}), channel {d}: got "
                             f"{float(out[b, i, h * hd + d])}, the key's v is {float(exp[b, i, h * hd + d])}; {int(bad.sum())} of "
                             f"{bad.numel()} elements beyond one ulp, on {int(bad.view(B, N, -1).any(-1).sum())} query rows")
    return int((dist != 0).sum())


def constant_v_bound(c, nk):
    return (2.0 ** -10 + nk * TINY16) * c.double().abs()


def check_constant_v(out, case):
    """|out_d - c_d| <= (2^-10 + N_k 2^-24) |c_d|: 2^-11 from P rounded to fp16 while the row sum may be taken before the rounding,
    2^-11 from the fp16 output, 2^-24 per key from P that underflows. Returns the largest error / bound."""
    B, N, H, hd = case.B, case.N, case.H, case.hd
    assert out.dtype == torch.float16 and out.shape == (B, N, H * hd)
    _finite(out, N, H, hd)
    c = case.c.to(out.device).double().view(1, 1, H * hd)
    ratio = (out.double() - c).abs() / constant_v_bound(c, n_keys(case.mode, N))
    bad = ratio > 1.0
    if bool(bad.any()):
        b, h, i, d = _where(bad.flatten().nonzero()[0], N, H, hd)
        raise AssertionError(f"image {b}, head {h}, query {i}, channel {d}: got {float(out[b, i, h * hd + d])} for c = "
                             f"{float(c[0, 0, h * hd + d])}, {float(ratio[b, i, h * hd + d]):.1f} x the bound; {int(bad.sum())} of "
                             f"{bad.numel()} elements beyond it")
    return float(ratio.max())


def budget_bound(ref, nk, H):
    B, N, C = ref.o.shape
    ds = ref.ds.permute(0, 2, 1).unsqueeze(-1).expand(B, N, H, C // H).reshape(B, N, C)
    return (2.0 ** -10 + nk * TINY16 + 2.0 * ds) * ref.A + U16 * ref.o.abs()


def check_budget(out, case, ref):
    """Elementwise |out - o| <= (2^-10 + N_k 2^-24 + 2 ds_i) A_id + 2^-11 |o_id|, and per (image, head)
    rms(out - o) <= 3 rms(rounding model - o). `ref` = reference(..., budget=True, model=True).
    Returns (largest error / bound, largest rms / model rms); raises with the first offending element or (image, head)."""
    B, N, H, hd = case.B, case.N, case.H, case.hd
    assert out.dtype == torch.float16 and out.shape == ref.o.shape
    _finite(out, N, H, hd)
    err = (out.double() - ref.o).abs()
    ratio = err / budget_bound(ref, n_keys(case.mode, N), H)
    bad = ratio > 1.0
    if bool(bad.any()):
        b, h, i, d = _where(bad.flatten().nonzero()[0], N, H, hd)
        raise AssertionError(f"image {b}, head {h}, query {i}, channel {d}: got {float(out[b, i, h * hd + d])}, float64 "
                             f"{float(ref.o[b, i, h * hd + d]):.6g}, {float(ratio[b, i, h * hd + d]):.1f} x the bound; "
                             f"{int(bad.sum())} of {bad.numel()} elements beyond it")

    def rms(x):
        return x.view(B, N, H, hd).pow(2).mean(dim=(1, 3)).sqrt()                                 # [B, H]

    got, mdl = rms(out.double() - ref.o), rms(ref.model - ref.o)
    r = got / mdl
    if bool((r > RMS_FACTOR).any()):
        b, h = divmod(int((r > RMS_FACTOR).flatten().nonzero()[0]), H)
        raise AssertionError(f"image {b}, head {h}: rms error {float(got[b, h]):.3e} is {float(r[b, h]):.2f} x the rounding "
                             f"model's {float(mdl[b, h]):.3e} (limit {RMS_FACTOR}); max error / bound {float(ratio.max()):.3f}")
    return float(ratio.max()), float(r.max())


def check_guard(buf, B):
    """buf fp16 [B + guard, N, C], NaN before the launch: the images behind the B real ones must still be NaN everywhere. Returns the
    number of guard elements."""
    tail = buf[B:]
    assert tail.numel() > 0, "no guard rows"
    bad = ~torch.isnan(tail.float())
    if bool(bad.any()):
        i, r, col = bad.nonzero()[0].tolist()
        raise AssertionError(f"guard row {r} behind the last image (guard image {i}), column {col} was written: "
                             f"{float(tail[i, r, col])}; {int(bad.sum())} guard elements written")
    return tail.numel()


def check_margin(case, ref):
    """The selector's condition, asserted on the float64 reference before a kernel output is looked at. Returns the least margin."""
    m = float(ref.margin.min())
    assert m >= MARGIN_NATS, f"least margin {m:.1f} nats < {MARGIN_NATS}: raise the constructor's gain"
    assert torch.equal(ref.o.half().cpu(), case.expected.cpu()), "the float64 softmax does not round to the target's v row"
    return m


# ---- the shapes tests/test_attention_exact_gpu.py runs (tests/test_attention_reference_cpu.py proves the inputs at each) -------
MODE0_ASM_N = (128, 192, 449, 1297, 1301)                                   # hd = 64, the assembly kernel from N >= 128
MODE0_HIP = ((64, 64), (64, 200), (64, 1297), (80, 200), (80, 320))         # (hd, N) on the HIP kernels
MODE1_GH_AT_GW64 = (4, 16, 64)
ANY_MAPS = ((5, 7), (3, 1), (20, 28), (32, 32), (64, 33), (40, 40))
WINDOW_MAPS = (64, 32, 20)
HEAD_DIMS = (64, 80)


def shapes():
    """every distinct (mode, N, gh, gw, hd) of the GPU file, sorted."""
    s = {(0, n, 0, 0, 64) for n in MODE0_ASM_N} | {(0, n, 0, 0, hd) for hd, n in MODE0_HIP}
    for hd in HEAD_DIMS:
        s |= {(1, gh * 64, gh, 64, hd) for gh in MODE1_GH_AT_GW64}
        s |= {(1, gh * gw, gh, gw, hd) for gh, gw in ANY_MAPS}
        s |= {(2, g * g, g, g, hd) for g in WINDOW_MAPS}
    return sorted(s)


# ---- the (image, head) sweeps of tests/test_attention_items_gpu.py: the item maps of the kernels, not their arithmetic ---------------
ITEMS_WINDOW64_BH = ((1, 1), (1, 3), (1, 5), (3, 5), (2, 7), (1, 12), (3, 12), (2, 16), (1, 32), (3, 32), (11, 1))   # 64 x 64 map, hd = 80
ITEMS_WINDOW_SMALL = (tuple((g, hd, B, H) for g in (32, 20) for hd in HEAD_DIMS for B, H in ((1, 12), (7, 16), (5, 3)))
                      + tuple((14, hd, B, H) for hd in HEAD_DIMS for B, H in ((1, 1), (1, 2), (3, 1))))
ITEMS_ASM_BH = ((1, 1), (1, 7), (1, 12), (5, 12), (2, 16), (3, 33))
# the last (B, H) the work table of the global assembly kernels admits for H = 48 and 64, each followed by the first it refuses
ITEMS_ASM_EDGES = ((28, 48), (29, 48), (15, 64), (16, 64))
ITEMS_FUSED_BH = ((1, 5), (1, 12), (2, 16))
ITEMS_HIP_BH = ((1, 1), (1, 7), (5, 12), (2, 16))
ITEMS_ANY_MAPS = ((5, 7), (20, 28))


def gattn_asm_admits(B, H):
    """the work table of the global assembly kernels packs b * H + h and divides it by H with ceil(2^16 / H): csrc/attention.hip
    gattn_asm_eligible admits B * H < 65536 // H (and H <= 64)."""
    return 1 <= H <= 64 and B * H < 65536 // H


# ---- the host-built work tables of the assembly kernels (csrc/work_tables.h), restated: tests/test_work_tables_cpu.py compares them
# with the C++ entry for entry, tests/test_attention_items_gpu.py names the branches a case exercises from them --------------------------
XCDS = 8                                   # as the kernels assume (workgroup wg on XCD wg & 7)
NWIN64 = 25                                # 14 x 14 windows of the 64 x 64 map


def wattn_shares(B, H, nwin, grid):
    """per workgroup of wattn_p_kernel (and of wattn_work_list where it cuts contiguous shares): (wg, x, sx, nwg_x, windows of the
    XCD, it0, it1)."""
    ngrp = B * nwin
    for wg in range(grid):
        x, sx = wg & 7, wg >> 3
        nwg_x = (grid + 7 - x) >> 3
        nwin_x = (ngrp + 7 - x) >> 3
        cnt_x = nwin_x * H
        yield wg, x, sx, nwg_x, nwin_x, sx * cnt_x // nwg_x, (sx + 1) * cnt_x // nwg_x


def wattn_asm_lists(B, H, grid):
    """wattn_work_list of psam_wattn_asm_80 (the 64 x 64 map: 25 windows): per workgroup its list of (b, h, window), and whether it
    keeps one head and strides over the windows (nwg_x % H == 0) or takes a contiguous share."""
    nwin = NWIN64
    lists, one_head = [], []
    for wg, x, sx, nwg_x, nwin_x, it0, it1 in wattn_shares(B, H, nwin, grid):
        if nwg_x % H == 0:
            lanes, hh, lane = nwg_x // H, sx % H, sx // H
            l = [(q, hh) for q in range(lane, nwin_x, lanes)]
        else:
            l = [divmod(i, H) for i in range(it0, it1)]
        one_head.append(nwg_x % H == 0)
        lists.append([((q * 8 + x) // nwin, h, (q * 8 + x) % nwin) for q, h in l])
    return lists, one_head


def gattn_asm_table(BH, nqb, xcds=XCDS):
    """gattn_work_table: BH * nqb items cut into `xcds` equal runs, padded with -1, an entry (b * H + h) << 10 | query block."""
    items = BH * nqb
    per = -(-items // xcds)
    tab = [-1] * (per * xcds)
    for x in range(xcds):
        i0, i1 = items * x // xcds, items * (x + 1) // xcds
        for i in range(i0, i1):
            tab[(i - i0) * xcds + x] = ((i // nqb) << 10) | (i % nqb)
    return tab


def gattn_asm_decode(tab, H):
    """the kernels' decode of the table's entries, b = (grp * ceil(2^16 / H)) >> 16: the list of (b, h, query block)."""
    M = (65536 + H - 1) // H
    out = []
    for e in tab:
        if e >= 0:
            grp, qb = e >> 10, e & 0x3ff
            b = (grp * M) >> 16
            out.append((b, grp - b * H, qb))
    return out


def item_shapes_cpu():
    """(mode, B, H, hd, N, gh, gw, item_rows) of the sweeps that the CPU can afford: tests/test_attention_reference_cpu.py injects
    the item faults at each. item_rows: 256 queries per item in the assembly kernels, 128 in the HIP global kernels."""
    return [(0, 5, 12, 64, 128, 0, 0, 256), (0, 28, 48, 64, 128, 0, 0, 256), (0, 1, 7, 64, 449, 0, 0, 256),
            (0, 5, 12, 80, 200, 0, 0, 128), (0, 2, 16, 64, 200, 0, 0, 128),
            (1, 5, 12, 64, 256, 4, 64, 256), (1, 2, 48, 80, 256, 4, 64, 256), (1, 5, 12, 80, 35, 5, 7, 128),
            (1, 2, 16, 64, 560, 20, 28, 128),
            (2, 5, 3, 64, 400, 20, 20, 0), (2, 1, 12, 80, 1024, 32, 32, 0), (2, 3, 1, 64, 196, 14, 14, 0),
            (2, 1, 5, 80, 4096, 64, 64, 0), (2, 2, 12, 80, 4096, 64, 64, 0)]
