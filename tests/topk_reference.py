"""Host restatement of psam_topk_points that the top-k point tests compare against (numpy only, no GPU, no project code).

`topk_keys`     per component the k largest point keys in descending order: largest p_fg first, first pixel in raster order
                among equals; the key is oracle.ccl.point_key's (float bits of p) << 32 | (0xFFFFFFFF - pixel index), 0 = empty
                slot. One lexsort over the foreground, no loop over the components. `tie="last"` is the WRONG tie rule (last
                raster index first), kept for the injected-fault tests.
`mismatches`    the comparison helper of the GPU tests: exact uint64 equality, slot by slot, with a readable report.
`decode`        key -> (x, y, p)
"""
import numpy as np

U32 = 0xFFFFFFFF


def as_u64(keys):
    """int64 view of the kernel (torch or numpy) or uint64 -> numpy uint64 of the same bits"""
    a = keys.cpu().numpy() if hasattr(keys, "cpu") else np.asarray(keys)
    return a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)


def topk_keys(labels, pfg, n, k, max_comp, only_best=None, tie="first"):
    """labels int [H,W] (0 = background, component c = label c + 1), pfg float32 [H,W] >= 0, n = components the table holds ->
    uint64 [R, k], R = max_comp, or R = 1 with only_best = the component whose row is wanted. Row c: component c's k largest keys
    in descending order, zeros behind a component of fewer than k pixels; rows >= min(n, max_comp) are zeros; pixels whose label
    exceeds min(n, max_comp) belong to no row."""
    labels = np.asarray(labels)
    R = max_comp if only_best is None else 1
    out = np.zeros((R, k), dtype=np.uint64)
    flat = labels.ravel()
    idx = np.flatnonzero(flat).astype(np.int64)
    lab = flat[idx].astype(np.int64) - 1
    bits = np.ascontiguousarray(pfg, dtype=np.float32).ravel().view(np.uint32)[idx].astype(np.int64)
    keep = lab < (min(n, max_comp) if only_best is None else n)
    if only_best is not None:
        keep &= lab == int(only_best)
    idx, lab, bits = idx[keep], lab[keep], bits[keep]
    if idx.size == 0:
        return out
    # for p >= 0 the float bits order like the values: label, then -bits (largest p first), then the raster index
    order = np.lexsort((idx if tie == "first" else -idx, -bits, lab))
    idx, lab, bits = idx[order], lab[order], bits[order]
    rank = np.arange(lab.size) - np.searchsorted(lab, lab, side="left")
    sel = rank < k
    keys = (bits[sel].astype(np.uint64) << np.uint64(32)) | (np.uint64(U32) - idx[sel].astype(np.uint64))
    out[lab[sel] if only_best is None else 0, rank[sel]] = keys
    return out


def decode(key, W):
    """-> (x, y, p) or None for an empty slot"""
    key = int(key) & ((1 << 64) - 1)
    if key == 0:
        return None
    i = U32 - (key & U32)
    return i % W, i // W, float(np.array(key >> 32, dtype=np.uint32).view(np.float32))


def mismatches(got, ref, W, limit=5):
    """Exact comparison of two key arrays [..., R, k] (bit for bit, no tolerance) -> list of strings, empty when they agree."""
    got, ref = as_u64(got), as_u64(ref)
    if got.shape != ref.shape:
        return [f"shape {got.shape} != {ref.shape}"]
    bad = np.argwhere(got != ref)
    return [f"{len(bad)} slots differ"] + [f"slot {tuple(int(v) for v in b)}: got {decode(got[tuple(b)], W)} (0x{int(got[tuple(b)]):016x}), "
                                          f"expected {decode(ref[tuple(b)], W)} (0x{int(ref[tuple(b)]):016x})"
                                          for b in bad[:limit]] if len(bad) else []


def assert_keys(got, ref, W):
    bad = mismatches(got, ref, W)
    assert not bad, "\n".join(bad)
