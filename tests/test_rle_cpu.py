"""CPU: the COCO string form of an uncompressed RLE (`coco_encode_rle` / `coco_decode_rle`, restated from the COCO API's
published `rleToString` / `rleFrString`) and the host-side validation of `rle_to_mask_device`.

pycocotools is optional: where it imports, the strings are also compared with `mask_utils.frPyObjects`; elsewhere the form is
pinned by vectors derived by hand from the published algorithm and by the round trip."""
import numpy as np
import pytest

from protosam_amd.segment_anything.utils import amg


def _rle(counts, size=None):
    return {"size": list(size) if size else [1, int(sum(counts))], "counts": list(counts)}


@pytest.mark.parametrize("counts,string", [
    # 2 -> '2', 3 -> '3', 1 -> '1'; the fourth count is stored as 1 - 3 = -2: low five bits 30, the rest is -1 and bit 0x10 is
    # set, so nothing follows: chr(48 + 30) = 'N'
    ([2, 3, 1, 1], "231N"),
    # 100 = 3 * 32 + 4: group 4 with "more" (4 + 32 + 48 = 84 = 'T'), then 3 ('3')
    ([100], "T3"),
    # 2**20: four zero groups with "more" (32 + 48 = 80 = 'P'), then 1
    ([1048576], "PPPP1"),
])
def test_coco_string_hand_vectors(counts, string):
    enc = amg.coco_encode_rle(_rle(counts, (7, 9)))
    assert enc == {"size": [7, 9], "counts": string}
    assert amg.coco_decode_rle(enc) == _rle(counts, (7, 9))
    assert amg.coco_decode_rle({"size": [7, 9], "counts": string.encode("ascii")}) == _rle(counts, (7, 9))   # pycocotools: bytes


def test_coco_string_round_trip_random_counts():
    rng = np.random.default_rng(5)
    for trial in range(400):
        n = int(rng.integers(1, 41))
        counts = rng.integers(0, 2 ** 20 + 1, size=n)
        counts[rng.random(n) < 0.15] = 0                           # zero-length runs
        if trial % 7 == 0:
            counts[rng.integers(n)] = 2 ** 20
        r = _rle(counts.tolist(), (3, 5))
        enc = amg.coco_encode_rle(r)
        assert isinstance(enc["counts"], str) and all(48 <= ord(c) < 48 + 64 for c in enc["counts"])
        assert amg.coco_decode_rle(enc) == r


@pytest.mark.parametrize("density", [0.0, 0.02, 0.5, 1.0])
def test_coco_string_round_trip_masks(density):
    rng = np.random.default_rng(int(density * 100) + 1)
    for h, w in ((1, 1), (5, 3), (64, 65), (257, 130)):
        m = rng.random((h, w)) < density
        for first in (False, True):
            if first:
                m = m.copy()
                m[0, 0] = True                                      # a set first pixel: the list starts with a 0
            r = amg.mask_to_rle(m)
            assert (r["counts"][0] == 0) == bool(m[0, 0])
            back = amg.coco_decode_rle(amg.coco_encode_rle(r))
            assert back == r
            np.testing.assert_array_equal(amg.rle_to_mask(back), m)


def test_coco_string_vs_pycocotools():
    mask_utils = pytest.importorskip("pycocotools.mask")
    rng = np.random.default_rng(9)
    for h, w, p in ((5, 3, 0.5), (64, 65, 0.02), (48, 44, 0.5), (33, 17, 1.0), (16, 16, 0.0)):
        r = amg.mask_to_rle(rng.random((h, w)) < p)
        ref = mask_utils.frPyObjects(r, h, w)
        assert amg.coco_encode_rle(r)["counts"] == ref["counts"].decode("utf-8")
        assert amg.coco_decode_rle(ref) == r


def test_rle_to_mask_device_validates_on_the_host(monkeypatch):
    """A negative count, or counts that do not sum to h * w, raise ValueError before any device call."""
    from protosam_amd import ops

    def no_device_call(*a, **k):
        raise AssertionError("rle_decode was reached")
    monkeypatch.setattr(ops, "rle_decode", no_device_call)
    good = amg.mask_to_rle(np.eye(4, 6, dtype=bool))
    for bad in ({"size": [4, 6], "counts": [5, -1, 20]},            # sums to 24, one count negative
                {"size": [4, 6], "counts": [5, 18]},                # one short
                {"size": [4, 6], "counts": [5, 20]},                # one over
                {"size": [4, 6], "counts": []},
                {"size": [6, 4], "counts": good["counts"]}):        # another size than the first record's
        with pytest.raises(ValueError):
            amg.rle_to_mask_device([good, bad], "cuda:0")
    with pytest.raises(ValueError):
        amg.rle_to_mask_device([], "cuda:0")
    with pytest.raises(AssertionError, match="rle_decode was reached"):   # a valid list does get that far
        amg.rle_to_mask_device([good], "cpu")


def test_rle_ops_reject_cpu_tensors():
    import torch
    from protosam_amd import ops
    with pytest.raises(RuntimeError):
        ops.rle_encode(torch.zeros((2, 4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ops.rle_decode(torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), 4, 4)
