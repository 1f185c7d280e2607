"""Oracle: the ALP prototype kernels of csrc/alp.hip one by one, in float64 (numpy / torch-CPU). Test infrastructure only.

Written from the header comments of csrc/alp.hip and from oracle/alp.py. Every value function returns, beside the float64 value, an
element-wise ERROR BOUND for an fp32 kernel that evaluates the same formula with the kernel's summation structure; the bounds are
rounding counts (units of u = 2^-24, gamma(k) = k u / (1 - k u)), never figures taken from a kernel.
tests/test_alp_reference_cpu.py pins the values to oracle/alp.py and shows that stock fp32 torch stays inside every bound on every
input of tests/test_alp_kernels_gpu.py; the input builders of both files live here so that the two files see the same numbers.

Decisions (cell selected or not, fg mode, nearest source index) are index rules, not arithmetic to be widened: they are restated in
fp32 exactly as the kernel states them, and the inputs are chosen so that every one of them is exact (binary masks, thresholds
further than 1e-6 from every coverage k / pool_w^2 and k / kernel_size^2 - `decision_margin` - except in the tie cases, where the
coverage 3/4 and the threshold 0.75 are the same fp32 number).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
NAN = float("nan")
META_NBG, META_NFG, META_FGMODE, META_NCELL_FG = 0, 1, 2, 3


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- nearest resize ------------------------------------------------------------------------------------------------------------
def nearest_index(out_size, in_size):
    """`nearest_src` of csrc/alp.hip: min(floor(float32(dst) * float32(in / out)), in - 1), scale and product in fp32."""
    scale = np.float32(np.float32(in_size) / np.float32(out_size))
    prod = np.arange(out_size, dtype=np.float32) * scale
    assert prod.dtype == np.float32
    return np.minimum(np.floor(prod).astype(np.int64), in_size - 1)


def nearest_index_exact(out_size, in_size):
    """The same rule in exact integer arithmetic: min(floor(dst * in / out), in - 1)."""
    return np.minimum(np.arange(out_size, dtype=np.int64) * in_size // out_size, in_size - 1)


def nearest_resize(mask, h, w):
    """mask [MH, MW] -> [h, w], F.interpolate(mode='nearest') by the fp32 index rule above."""
    m = torch.as_tensor(mask)
    iy = torch.from_numpy(nearest_index(h, m.shape[0]))
    ix = torch.from_numpy(nearest_index(w, m.shape[1]))
    return m[iy][:, ix]


def search_nearest_pair(limit=1024, h_min=1):
    """The first (MH, h, dst) in ascending (h, MH), h >= h_min, both below `limit`, at which the fp32 index differs from the exact one;
    None when there is none. (There are many: the first is MH = 62, h = 14, where dst = 7 reads row 30, not 31.)"""
    for h in range(h_min, limit):
        MH = np.arange(1, limit, dtype=np.int64)
        dst = np.arange(h, dtype=np.int64)
        scale = (MH.astype(np.float32) / np.float32(h)).astype(np.float32)
        f = np.minimum(np.floor(dst[None, :].astype(np.float32) * scale[:, None]).astype(np.int64), MH[:, None] - 1)
        e = np.minimum(dst[None, :] * MH[:, None] // h, MH[:, None] - 1)
        bad = np.argwhere(f != e)
        if len(bad):
            return int(MH[bad[0][0]]), h, int(bad[0][1])
    return None


SEARCHED = ((62, 14), (150, 18))      # (MH, h) and (MW, w): search_nearest_pair(1024, 1)[:2] and (1024, 15)[:2], asserted on the CPU


# ---- psam_alp_bank -------------------------------------------------------------------------------------------------------------
def _cells(m, pw):
    """[h, w] -> per-cell sums [h // pw, w // pw] (trailing rows / columns ignored, as avg_pool2d does)."""
    ch, cw = m.shape[0] // pw, m.shape[1] // pw
    return m[:ch * pw, :cw * pw].reshape(ch, pw, cw, pw).sum(axis=(1, 3))


def _cover32(sums, n):
    return (sums.astype(np.float32) / np.float32(n)).astype(np.float32)


def bank_ref(sup, h, w, mask, bmask, pool_w, kernel_size, thresh, eps, force_mode, cap):
    """Float64 restatement of psam_alp_bank. sup: [h*w, C] (token-major values, any storage), mask / bmask: [MH, MW] (bmask None =
    1 - mask). -> dict: meta (n_bg, n_fg, fg_mode, n_cells_fg), slot_bg / slot_fg (row-major cells, -1 = not selected), rows_bg /
    rows_fg (float64, occupied rows only; the global row sum(x m) / (sum(m) + 1e-5) last in rows_fg unless mode 2), bound_bg /
    bound_fg (element-wise), the kind of every fg row ('cell' / 'global'), and the exact coverages (cover_fg, cover_bg, cover_ks)
    for `decision_margin`.

    Decisions: a cell is selected when float32(sum) / float32(pw^2) > float32(thresh) (strict), the mode is gridconv+ (1) when some
    kernel_size cell has float32(sum) / float32(ks^2) >= float32(thresh), else mask (0); force_mode >= 0 overrides the mode. In mode 0
    no fg cell is kept (slot_fg = -1 everywhere); in mode 2 there is no global row.

    Error bound of a row p = v / max(|v|, eps), v the un-normalised row with element-wise error E:
      pooled row    v_k = (x_1 + .. + x_n) / n, n = pw^2, summed in sequence: n - 1 additions and one division, every rounding relative
                    to a partial sum of magnitude <= sum |x_i|:  E_k = gamma(n) mean_i |x_ik|.
      global row    the h*w products x_ik m_i are split over 16 chains (four waves x four accumulators, pixel i in chain i mod 16
                    while a wave has four pixels left); a wave's last one to three pixels all go to its first accumulator, so the
                    longest chain has up to L = ceil(h w / 16) + 3 terms (7x9, wave 3: 3 + 3): one product rounding and up to L additions
                    per term; the chains are combined by (s0 + s1) + (s2 + s3) (2 roundings) and ((p0 + p1) + p2) + p3 (3); the
                    denominator is a 64-lane sum of h w mask values (ceil(h w / 64) additions per lane, 6 shuffle levels - exact for a
                    binary mask, counted all the same: bank_ref takes any mask) plus 1e-5 (1), and one division follows. All of
                    them act on partial sums of magnitude <= A_k = sum_i |x_ik m_i|, not on the (cancelling) result:
                    E_k = gamma(L + 6 + ceil(h w / 64) + 7 + 1) A_k / (sum m + 1e-5).
      normalisation the kernel sums v_k^2 per lane (ceil(C / 64) terms, product and addition: ceil(C / 64) + 1 roundings), 6 shuffle
                    levels, sqrt (halves the relative error, adds 1), then one division: relative t = gamma((ceil(C / 64) + 7) / 2 + 2)
                    on the row it was given; and the error E of that row moves v_k / N, N = max(|v|, eps), by at most
                    E_k / N + |v_k| (sum_j |v_j| E_j) / N^3 (first order; x 1.01 for the rest - E / |v| is ~1e-6).
      bound_k = 1.01 (E_k / N + |v_k| sum_j |v_j| E_j / N^3) + t |v_k| / N + 2^-126.
    """
    x = torch.as_tensor(sup).double().numpy().reshape(h * w, -1)
    C = x.shape[1]
    mask = np.asarray(torch.as_tensor(mask).double().numpy())
    iy, ix = nearest_index(h, mask.shape[0]), nearest_index(w, mask.shape[1])
    mf = mask[iy][:, ix]
    mb = 1.0 - mf if bmask is None else np.asarray(torch.as_tensor(bmask).double().numpy())[iy][:, ix]
    t32 = np.float32(thresh)
    pw, ks = pool_w, kernel_size
    cov_f, cov_b = _cells(mf, pw), _cells(mb, pw)
    sel_f = (_cover32(cov_f, pw * pw) > t32).reshape(-1)
    sel_b = (_cover32(cov_b, pw * pw) > t32).reshape(-1)
    cov_k = _cells(mf, ks) if (h // ks) * (w // ks) > 0 else np.zeros((0, 0))
    any_full = bool((_cover32(cov_k, ks * ks) >= t32).any())
    mode = force_mode if force_mode >= 0 else (1 if any_full else 0)
    nc = sel_f.size
    assert nc + 1 <= cap
    slot_b = np.where(sel_b, np.cumsum(sel_b) - sel_b, -1).astype(np.int64)
    slot_f = np.where(sel_f & (mode != 0), np.cumsum(sel_f) - sel_f, -1).astype(np.int64)
    n_bg = int(sel_b.sum())
    ncell_fg = int(sel_f.sum()) if mode else 0
    n_fg = ncell_fg + (0 if mode == 2 else 1)

    ch, cw = h // pw, w // pw
    xc = x.reshape(h, w, C)[:ch * pw, :cw * pw].reshape(ch, pw, cw, pw, C)
    pooled = xc.mean(axis=(1, 3)).reshape(nc, C)
    pooled_E = gamma(pw * pw) * np.abs(xc).mean(axis=(1, 3)).reshape(nc, C)
    npx = h * w
    den = mf.sum() + float(np.float32(1e-5))
    glob = (x * mf.reshape(npx, 1)).sum(axis=0) / den
    kg = math.ceil(npx / 16) + 3 + 6 + math.ceil(npx / 64) + 7 + 1
    glob_E = gamma(kg) * (np.abs(x) * np.abs(mf).reshape(npx, 1)).sum(axis=0) / den

    def norm(v, E):
        N = np.maximum(np.sqrt((v * v).sum(axis=1, keepdims=True)), eps)
        t = gamma((math.ceil(C / 64) + 7) / 2 + 2)
        bound = 1.01 * (E / N + np.abs(v) * (np.abs(v) * E).sum(axis=1, keepdims=True) / N ** 3) + t * np.abs(v) / N + 2.0 ** -126
        return v / N, bound

    rows_bg, bound_bg = norm(pooled[sel_b], pooled_E[sel_b])
    vf, Ef, kinds = [], [], []
    if mode:
        vf.append(pooled[sel_f]); Ef.append(pooled_E[sel_f]); kinds += ["cell"] * ncell_fg
    if mode != 2:
        vf.append(glob[None]); Ef.append(glob_E[None]); kinds.append("global")
    if vf:
        rows_fg, bound_fg = norm(np.concatenate(vf), np.concatenate(Ef))
    else:
        rows_fg, bound_fg = np.zeros((0, C)), np.zeros((0, C))
    assert rows_fg.shape[0] == n_fg and rows_bg.shape[0] == n_bg
    return dict(meta=(n_bg, n_fg, mode, ncell_fg), slot_bg=slot_b, slot_fg=slot_f,
                rows_bg=torch.from_numpy(rows_bg), rows_fg=torch.from_numpy(rows_fg),
                bound_bg=torch.from_numpy(bound_bg), bound_fg=torch.from_numpy(bound_fg), kinds=kinds,
                cover_fg=cov_f / (pw * pw), cover_bg=cov_b / (pw * pw), cover_ks=cov_k / (ks * ks), mres_fg=mf, mres_bg=mb)


def decision_margin(ref, thresh):
    """(smallest |coverage - float32(thresh)| over every cell and kernel cell of a bank_ref result, number of exact ties)."""
    t = float(np.float32(thresh))
    d = np.concatenate([np.abs(ref[k].reshape(-1) - t) for k in ("cover_fg", "cover_bg", "cover_ks")])
    ties = int((d == 0).sum())
    rest = d[d > 0]
    return (float(rest.min()) if rest.size else float("inf")), ties


# ---- psam_alp_sim --------------------------------------------------------------------------------------------------------------
def sim_ref(qry, protos, eps=1e-4, sim_scale=20.0, path="d2"):
    """qry [npix, C], protos [n, C] as given (no normalisation of the prototypes: the bank rows are what they are) ->
    (S, bound) float64 [npix]: d_i = sim_scale q.p_i / max(|q|, eps), S = sum_i softmax(d)_i d_i. n = 0 gives NaN (0 / 0).

    Bound of an fp32 kernel with the structure of kernel D2 (path 'd2': groups of 96 prototypes) or kernels D + E ('d': tiles of 64):
      dd_i   the dot product is a C-term fp32 fma chain: gamma(C) sum_k |q_k p_ik|. |q|^2 is a sum of C positive terms - 'd2': per
             lane half 4 C / 32 partial sums of four terms ((a + b) + (c + d): product + 2 additions) in sequence, one shuffle addition:
             kq = C / 8 + 4 roundings; 'd': one chain, kq = C + 1 - of which the sqrt keeps half and adds one, the division
             sim_scale / max(.) one and acc * qinv one: |d_i| (kq / 2 + 3) u. With |d_i| <= sim_scale sum_k |q_k p_ik| / |q|:
             dd_i = gamma(C + kq / 2 + 3) sim_scale sum_k |q_k p_ik| / max(|q|, eps), scaled by the products' magnitudes, not by |d_i|.
      S(d)   dS / dd_i = s_i (1 + d_i - S): first order sum_i s_i |1 + d_i - S| dd_i; the second-order rest is at most
             1/2 max(dd)^2 sum_ij |H_ij| <= 1/2 max(dd)^2 (4 + 3 M), M = sum_i s_i |d_i - S| - taken twice, the Hessian being evaluated
             at the reference.
      exp / merge   every e_i = exp(d_i - m) the kernel forms is used for both Z and W, and so is every rescaling factor of the online
             merges (lane, lane half, groups): a relative error r_i of e_i moves S by s_i r_i (d_i - S). The subtractions' arguments
             telescope to m - d_i (u (m - d_i) in all), expf is taken as 2 ulp = 4 u, each of the <= G + 1 rescalings (G groups) is
             an expf and a product (5 u): r_i <= u ((m - d_i) + 4 + 5 (G + 1)). The sums: Z takes nadd additions, W one product
             more; 'd2': 48 per lane, 2 for the in-lane merge, 2 for the lane halves, 2 per group; 'd': 16, 1, 2, 2 per tile; then one
             division: gamma(nadd + 2) (sum_i s_i |d_i| + |S|).
    (This last part is k u (1 + |S|) in the issue. W is a signed sum, and its roundings act on sum_i e_i |d_i|, which |S| bounds only
    when the weighted logits share a sign; so the magnitude is written as what the roundings act on, sum_i s_i |d_i| + |S| - at most
    2 |S| for logits of one sign. It is not a materially looser form: on the GPU file's inputs (sum_i s_i |d_i| + |S|) / (1 + |S|) is
    at most 1.9, measured and asserted below 2 by tests/test_alp_reference_cpu.py.)"""
    q = torch.as_tensor(qry).double()
    p = torch.as_tensor(protos).double()
    npix, C = q.shape
    n = p.shape[0]
    if n == 0:
        return torch.full((npix,), NAN, dtype=torch.float64), torch.zeros(npix, dtype=torch.float64)
    N = q.norm(dim=1).clamp_min(eps)[:, None]
    d = sim_scale * (q @ p.t()) / N
    a = sim_scale * (q.abs() @ p.abs().t()) / N
    s = torch.softmax(d, dim=1)
    S = (s * d).sum(dim=1)
    kq = C / 8 + 4 if path == "d2" else C + 1
    G = math.ceil(n / (96 if path == "d2" else 64))
    nadd = (52 if path == "d2" else 19) + 2 * G
    dd = gamma(C + kq / 2 + 3) * a
    dev = (d - S[:, None]).abs()
    M = (s * dev).sum(dim=1)
    first = (s * (1 + d - S[:, None]).abs() * dd).sum(dim=1)
    second = dd.max(dim=1)[0] ** 2 * (4 + 3 * M)
    m = d.max(dim=1)[0][:, None]
    rnd = U * (s * dev * ((m - d) + 4 + 5 * (G + 1))).sum(dim=1) + gamma(nadd + 2) * ((s * d.abs()).sum(dim=1) + S.abs())
    return S, first + second + rnd


def pairs_ref(qry, entries, n_planes, eps=1e-4, sim_scale=20.0):
    """qry [B, npix, C]; entries [(protos [n, C], slice b, plane), ...] in table order -> (S, bound) [n_planes, npix]: a plane is its
    first entry's score, then fmaxf(plane, next entry's) in table order (fmaxf returns the other operand for a NaN); planes that no
    entry names are NaN. |max(a, b) - max(a', b')| <= max(|a - a'|, |b - b'|): the bound of a plane is the largest of its entries'."""
    npix = qry.shape[1]
    S = np.full((n_planes, npix), NAN)
    bound = np.zeros((n_planes, npix))
    seen = set()
    for protos, b, plane in entries:
        v, bd = sim_ref(qry[b], protos, eps, sim_scale, "d2")
        S[plane] = v.numpy() if plane not in seen else np.fmax(S[plane], v.numpy())
        bound[plane] = np.maximum(bound[plane], bd.numpy())
        seen.add(plane)
    return torch.from_numpy(S), torch.from_numpy(bound)


def merge_ref(rows, counts):
    """MultiProtoAsConv.merge_banks: the occupied rows (the first counts[i] of rows[i]) concatenated in bank order."""
    return torch.cat([torch.as_tensor(r)[:n] for r, n in zip(rows, counts)], dim=0)


# ---- input builders ------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rect_mask(MH, MW, y0, y1, x0, x1):
    m = torch.zeros((MH, MW))
    m[y0:y1, x0:x1] = 1
    return m


# name -> (h, w, pool_w, kernel_size, C, ld - C, misaligned, (MH, MW), mask, bmask, thresh, force_mode). Masks: ('rect', y0, y1, x0, x1)
# in fractions of (MH, MW) scaled to pixels, 'ones', 'zeros', ('pixel', y, x), ('px', [(y0, y1, x0, x1), ...]) in pixels.
BANK_CASES = {
    # rectangle edges inside cells (rows 3..6 of 8: cells 1 and 3 half covered) and on cell borders (columns 2..6)
    "8x8_inside":      (8, 8, 2, 2, 32, 0, False, (8, 8), ("px", [(3, 7, 2, 6)]), None, 0.95, -1),
    "8x8_on_border":   (8, 8, 2, 2, 32, 4, False, (8, 8), ("px", [(2, 6, 0, 4)]), None, 0.95, -1),
    "8x8_ld_odd":      (8, 8, 2, 2, 96, 1, False, (8, 8), ("px", [(2, 6, 0, 4)]), None, 0.95, -1),
    "8x8_force0":      (8, 8, 2, 2, 32, 0, False, (8, 8), ("px", [(2, 6, 0, 4)]), None, 0.95, 0),
    "8x8_force1":      (8, 8, 2, 2, 32, 0, False, (8, 8), ("px", [(3, 4, 3, 4)]), None, 0.95, 1),     # the rule alone would say 0
    "8x8_force2":      (8, 8, 2, 2, 32, 0, False, (8, 8), ("px", [(2, 6, 0, 4)]), None, 0.95, 2),
    "8x8_ones":        (8, 8, 2, 2, 96, 0, False, (8, 8), "ones", None, 0.95, -1),
    "8x8_zeros":       (8, 8, 2, 2, 96, 4, False, (8, 8), "zeros", None, 0.95, -1),
    "8x8_zeros_c256":  (8, 8, 2, 2, 256, 0, False, (8, 8), "zeros", None, 0.95, -1),
    "8x8_pixel":       (8, 8, 2, 2, 32, 0, False, (8, 8), ("px", [(5, 6, 2, 3)]), None, 0.95, -1),
    "8x8_bmask":       (8, 8, 2, 2, 32, 0, False, (8, 8), ("px", [(2, 6, 2, 6)]), ("px", [(0, 2, 0, 8), (6, 8, 0, 6)]), 0.95, -1),
    "8x8_one_cell":    (8, 8, 8, 8, 32, 0, False, (8, 8), "ones", None, 0.95, -1),
    "8x8_one_cell_no": (8, 8, 8, 4, 32, 0, False, (8, 8), ("px", [(0, 4, 0, 4)]), None, 0.95, -1),
    # thresh = 0.75 = 3/4 exactly: the 2x2 cells (1,1), (1,2) hold three fg pixels, cell (2,1) three bg pixels, no cell is full
    "8x8_tie":         (8, 8, 2, 2, 32, 0, False, (8, 8), ("px", [(2, 3, 2, 6), (3, 4, 2, 3), (3, 4, 5, 6), (5, 6, 2, 3)]), None, 0.75, -1),
    "8x8_tie_512":     (8, 8, 2, 2, 32, 0, False, (512, 512),
                        ("px", [(128, 192, 128, 384), (192, 256, 128, 192), (192, 256, 320, 384), (320, 384, 128, 192)]), None, 0.75, -1),
    "8x8_c768_odd":    (8, 8, 2, 2, 768, 1, False, (512, 512), ("rect", 0.2, 0.8, 0.3, 0.9), None, 0.95, -1),
    "7x9":             (7, 9, 2, 2, 96, 4, False, (512, 512), ("rect", 0.1, 0.9, 0.2, 0.7), None, 0.95, -1),
    "7x9_100x130":     (7, 9, 2, 2, 32, 0, False, (100, 130), ("rect", 0.0, 0.6, 0.3, 1.0), None, 0.95, -1),
    "12x20_f4":        (12, 20, 4, 2, 256, 0, False, (100, 130), ("rect", 0.1, 0.8, 0.15, 0.75), None, 0.95, -1),
    "12x20_ld4":       (12, 20, 4, 2, 256, 4, False, (512, 512), ("rect", 0.1, 0.8, 0.15, 0.75), None, 0.95, -1),
    "12x20_scalar":    (12, 20, 4, 2, 256, 1, False, (100, 130), ("rect", 0.1, 0.8, 0.15, 0.75), None, 0.95, -1),
    "12x20_misalign":  (12, 20, 4, 2, 256, 0, True, (12, 20), ("px", [(0, 8, 4, 16)]), None, 0.95, -1),
    "14x18_searched":  (14, 18, 2, 2, 32, 0, False, (62, 150), ("px", [(31, 62, 125, 150)]), None, 0.95, -1),
    "36x36":           (36, 36, 2, 4, 768, 0, False, (512, 512), ("rect", 0.2, 0.75, 0.25, 0.8), None, 0.95, -1),
    "36x36_c96":       (36, 36, 2, 4, 96, 4, False, (100, 130), ("rect", 0.2, 0.75, 0.25, 0.8), None, 0.95, -1),
    "73x73":           (73, 73, 2, 9, 32, 4, False, (512, 512), ("rect", 0.13, 0.8, 0.2, 0.9), None, 0.95, -1),
    "73x73_c256":      (73, 73, 2, 9, 256, 0, False, (73, 73), ("px", [(5, 60, 11, 52)]), None, 0.95, -1),
}
TIE_CASES = ("8x8_tie", "8x8_tie_512")


def _mask_of(spec, MH, MW):
    if spec == "ones":
        return torch.ones((MH, MW))
    if spec == "zeros":
        return torch.zeros((MH, MW))
    if spec[0] == "rect":
        return rect_mask(MH, MW, round(spec[1] * MH), round(spec[2] * MH), round(spec[3] * MW), round(spec[4] * MW))
    m = torch.zeros((MH, MW))
    for y0, y1, x0, x1 in spec[1]:
        m[y0:y1, x0:x1] = 1
    return m


def bank_case(name):
    """-> dict(h, w, pool_w, kernel_size, C, ld, misaligned, sup [h*w, C] fp32 (values), mask, bmask (or None), thresh, force_mode)."""
    h, w, pw, ks, C, ldx, mis, (MH, MW), mspec, bspec, thresh, force = BANK_CASES[name]
    g = _gen(h, w, C, len(name))
    # a smooth field + noise + an offset per channel: cell means and the masked mean are neither tiny nor equal
    sup = torch.randn((h * w, C), generator=g) + 0.5 * torch.randn((1, C), generator=g) + \
        torch.linspace(-1, 1, h * w)[:, None] * torch.randn((1, C), generator=g)
    return dict(name=name, h=h, w=w, pool_w=pw, kernel_size=ks, C=C, ld=C + ldx, misaligned=mis, sup=sup.contiguous(),
                mask=_mask_of(mspec, MH, MW), bmask=None if bspec is None else _mask_of(bspec, MH, MW), thresh=thresh,
                force_mode=force, eps=1e-4)


def bank_case_ref(case, cap=None):
    c = case
    ncell = (c["h"] // c["pool_w"]) * (c["w"] // c["pool_w"])
    return bank_ref(c["sup"], c["h"], c["w"], c["mask"], c["bmask"], c["pool_w"], c["kernel_size"], c["thresh"], c["eps"],
                    c["force_mode"], cap or ncell + 1)


def unit_rows(n, C, *key):
    """n random rows of norm 1 (fp32, as a bank holds them)."""
    r = torch.randn((n, C), generator=_gen(n, C, *key))
    return (r / r.norm(dim=1, keepdim=True)).float()


def queries(B, npix, C, protos, *key):
    """[B, npix, C] fp32: noise plus a random multiple (cosine 0 .. 0.7) of one of `protos` per pixel, at norms from 0.1 to 10: the
    softmax is neither flat nor one-hot."""
    g = _gen(B, npix, C, *key)
    q = torch.randn((B, npix, C), generator=g)
    if protos is not None and protos.shape[0]:
        j = torch.randint(0, protos.shape[0], (B, npix), generator=g)
        q = q + torch.rand((B, npix, 1), generator=g) * math.sqrt(C) * protos[j]
    return (q * (10.0 ** (2 * torch.rand((B, npix, 1), generator=g) - 1))).float()


SIM_COUNTS = (1, 31, 32, 33, 95, 96, 97, 192, 193)
SIM_C = (32, 64, 96, 768)
SIM_NPIX = (1, 31, 33, 127, 128, 129, 200)
SIM_D_COUNTS = (1, 63, 64, 65, 97, 129)          # kernel D: prototype tiles of 64
SIM_D_C = (32, 96)
SIM_D_NPIX = (1, 33, 64, 65, 200)


# count n -> (n_bg, n_fg): the halves differ (and swap), cap = max + 1 = n + 1
SIM_BANKS = {1: (1, 1), 31: (31, 1), 32: (31, 32), 33: (33, 32), 95: (33, 95), 96: (96, 95), 97: (97, 96), 192: (97, 192),
             193: (193, 192), 63: (63, 1), 64: (63, 64), 65: (65, 64), 129: (97, 129)}


def sim_case(n_bg, n_fg, C, npix, B=2):
    """-> (qry [B, npix, C], rows_bg [n_bg, C], rows_fg [n_fg, C]), fp32."""
    rb, rf = unit_rows(n_bg, C, 0), unit_rows(n_fg, C, 1)
    both = torch.cat([rb, rf]) if n_bg + n_fg else None
    return queries(B, npix, C, both, n_bg, n_fg), rb, rf


def structured_case(C=64):
    """Banks and query rows with known answers. -> (qry [1, 8, C], banks {name: rows}).
    Rows: 0: 3 p0; 1: -0.7 p0; 2: all zero; 3: 1e-6 p0 (norm below eps = 1e-4: d = sim_scale q.p / eps); 4: +-1 in channels 0..3;
    5: e0 - e2; 6: 1000 p0; 7: p1 (random unit). Banks: 'same' (97 copies of p0: S = d), 'anti' (p0 and 96 x -p0: S ~ +-20 on the
    rows along p0), 'dup' (p0, p0, p1, p1, p1: duplicates), 'pm' (rows of +-1/2 in channels 0..3: every dot product of rows 4, 5 is a
    small integer / 2, exact in fp32)."""
    p0, p1 = unit_rows(2, C, 7)
    q = torch.zeros((8, C))
    q[0], q[1], q[3], q[6], q[7] = 3 * p0, -0.7 * p0, 1e-6 * p0, 1000 * p0, p1
    q[4, :4] = torch.tensor([1.0, -1.0, 1.0, 1.0])
    q[5, 0], q[5, 2] = 1.0, -1.0
    pm = torch.zeros((16, C))
    for i in range(16):
        pm[i, :4] = torch.tensor([0.5 if (i >> b) & 1 else -0.5 for b in range(4)])
    banks = {"same": p0[None].repeat(97, 1), "anti": torch.cat([p0[None], -p0[None].repeat(96, 1)]),
             "dup": torch.stack([p0, p0, p1, p1, p1]), "pm": pm}
    return q[None].float().contiguous(), {k: v.float() for k, v in banks.items()}


# fp32 torch, the arithmetic of oracle/alp.py, on the same inputs: what tests/test_alp_reference_cpu.py holds against the bounds
def sim_fp32(qry, protos, eps=1e-4, sim_scale=20.0):
    q, p = torch.as_tensor(qry).float(), torch.as_tensor(protos).float()
    qn = q / q.norm(dim=1, keepdim=True).clamp_min(eps)
    d = (qn @ p.t()) * sim_scale
    return (torch.softmax(d, dim=1) * d).sum(dim=1)
