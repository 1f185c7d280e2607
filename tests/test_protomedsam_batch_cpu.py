"""CPU: runner.run_slices_classes (the multi-class volume driver of ProtoMedSAM.forward_classes_batch) - batching, cuts at
z-part boundaries and where each slice's masks land - with a stub model that records its calls."""
import torch

from protosam_amd.runner import part_assign, run_slices_classes


class _Stub:
    """forward_classes_batch contract: results[b][c] = (mask, [conf]); classes with a prompt are views of `out`, the others int64
    zeros. The mask of class c of slice z (whose image is the constant z) is the constant z * 10 + c."""

    def __init__(self, empty=()):
        self.calls = []
        self.empty = set(empty)                 # (z, c) pairs that have no component
        self.last_stats = {}

    def forward_classes_batch(self, q, sup_img, sup_masks, out=None):
        B, C = q.shape[0], len(sup_masks)
        zs = [int(q[b, 0, 0, 0]) for b in range(B)]
        self.calls.append((zs, int(sup_img[0, 0, 0, 0]), [int(m[0, 0, 0]) for m in sup_masks]))
        assert out is not None and out.shape == (B, C) + tuple(q.shape[-2:]) and out.dtype == torch.uint8
        res, prompt = [], {}
        for b, z in enumerate(zs):
            row = []
            for c in range(C):
                if (z, c) in self.empty:
                    out[b, c].zero_()
                    row.append((torch.zeros(q.shape[-2:], dtype=torch.int64), [0]))
                elif c == C - 1:                # a mask that is not a view of `out`: the runner copies it
                    row.append((torch.full(q.shape[-2:], z * 10 + c, dtype=torch.uint8), [0.5]))
                    prompt[(b, c)] = len(prompt)
                else:
                    out[b, c].fill_(z * 10 + c)
                    row.append((out[b, c], [0.5]))
                    prompt[(b, c)] = len(prompt)
            res.append(row)
        self.last_stats = dict(prompt=prompt)
        return res


def _volume(n, S):
    return torch.arange(n, dtype=torch.float32)[:, None, None].expand(n, S, S).contiguous()


def test_run_slices_classes_batches_parts_and_placement():
    n, S, C = 9, 8, 3
    vol = _volume(n, S)
    sup_imgs = [torch.full((1, 3, S, S), 100.0 + p) for p in range(3)]
    sup_masks = [[torch.full((1, S, S), 10 * p + c, dtype=torch.float32) for c in range(C)] for p in range(3)]
    stub = _Stub(empty={(4, 1), (7, 0), (7, 1), (7, 2)})
    zs = [8, 0, 1, 2, 3, 4, 5, 6, 7]
    out, stats = run_slices_classes(stub, vol, sup_imgs, sup_masks, zs, torch.device("cpu"), batch=2)
    assert out.shape == (len(zs), C, S, S) and out.dtype == torch.uint8
    # batches of at most 2 slices, never across a z-part (parts of 9 slices: 0-2, 3-5, 6-8)
    assert [c[0] for c in stub.calls] == [[8], [0, 1], [2], [3, 4], [5], [6, 7]]
    for zb, sup, masks in stub.calls:
        p = part_assign(zb[0], n)
        assert all(part_assign(z, n) == p for z in zb)
        assert sup == 100 + p and masks == [10 * p + c for c in range(C)]
    for i, z in enumerate(zs):
        for c in range(C):
            want = 0 if (z, c) in stub.empty else z * 10 + c
            assert torch.equal(out[i, c], torch.full((S, S), want, dtype=torch.uint8)), (z, c)
        assert stats[i] == C - sum(1 for c in range(C) if (z, c) in stub.empty)


def test_run_slices_classes_one_call_per_part_when_batch_is_large():
    n, S = 6, 4
    vol = _volume(n, S)
    sup_imgs = [torch.full((1, 3, S, S), float(p)) for p in range(3)]
    sup_masks = [[torch.ones((1, S, S))] * 2 for _ in range(3)]
    stub = _Stub()
    out, stats = run_slices_classes(stub, vol, sup_imgs, sup_masks, list(range(n)), torch.device("cpu"), batch=32)
    assert [c[0] for c in stub.calls] == [[0, 1], [2, 3], [4, 5]] and stats == [2] * n
    assert out.shape == (n, 2, S, S) and int(out[5, 1, 0, 0]) == 51
