"""GPU: psam_seg_counts against numpy, exactly (counts and boxes are integers); `metrics.Metric` on device tensors against the outputs
recorded from the reference's `util.metric.Metric`; the evaluate_* drivers of the runner against the masks they leave in `keep=`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_scoring_cpu import INT_MAX, check_against_fixture, load_fixture, np_counts   # noqa: E402

EMPTY_BOX = [INT_MAX, INT_MAX, -1, -1]


def _planes(t):
    return t.reshape((-1,) + tuple(t.shape[-2:])).cpu().numpy()


def _check(pred, label, rows):
    """ops.seg_counts == numpy on the host copies, element for element"""
    from protosam_amd import ops
    got = ops.seg_counts(pred, label, rows)
    torch.cuda.synchronize()
    r = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else rows
    want = np_counts(_planes(pred), _planes(label), r)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    bad = np.nonzero((got.cpu().numpy() != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got.cpu().numpy()[bad[:5]], want[bad[:5]])
    return want


def _random_case(dev, n, C, H, W, density, seed, pred_dtype=torch.uint8, label_dtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    pred = (torch.rand((n, C, H, W), generator=g) < density).to(pred_dtype).to(dev)
    label = (torch.rand((n, H, W), generator=g) < density).to(torch.int64) * torch.randint(1, C + 1, (n, H, W), generator=g)
    return pred, label.to(label_dtype).to(dev)


@pytest.mark.parametrize("n,C,H,W", [(3, 4, 1024, 1024), (16, 4, 512, 512), (2, 3, 37, 53), (2, 2, 1, 1), (2, 2, 5, 4099)])
@pytest.mark.parametrize("density", [0.5, 0.001])
def test_shapes_and_densities(dev, n, C, H, W, density):
    from protosam_amd.metrics import class_rows
    pred, label = _random_case(dev, n, C, H, W, density, seed=H + W)
    want = _check(pred, label, class_rows(n, list(range(1, C + 1))).tolist())
    if H * W > 10000 and density == 0.5:
        assert (want[:, 0] > 0).all() and (want[:, 4:8] != EMPTY_BOX).all()


@pytest.mark.parametrize("pred_dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int16, torch.int32, torch.float32, torch.int64])
def test_types(dev, pred_dtype, label_dtype):
    from protosam_amd.metrics import class_rows
    for (H, W) in ((64, 96), (7, 29)):
        pred, label = _random_case(dev, 3, 4, H, W, 0.4, seed=W, pred_dtype=pred_dtype, label_dtype=label_dtype)
        _check(pred, label, class_rows(3, [1, 2, 3, 4]).tolist())
    # int64 masks go through the wrapper's cast as well; int16 / int32 predictions
    for dt in (torch.int64, torch.int16, torch.int32):
        pred, label = _random_case(dev, 2, 2, 33, 65, 0.4, seed=3, pred_dtype=dt, label_dtype=label_dtype)
        _check(pred, label, class_rows(2, [1, 2]).tolist())
    # values a uint8 plane cannot hold match nothing; float planes compare by value
    pred, label = _random_case(dev, 1, 1, 16, 48, 0.5, seed=4, pred_dtype=pred_dtype, label_dtype=label_dtype)
    want = _check(pred, label, [(0, 257, 0, 1), (0, 1, 0, -255), (0, 0, 0, 0)])
    assert want[0, 0] + want[0, 1] == 0 and want[1, 0] + want[1, 2] == 0 and want[2, 0] > 0


def test_views_and_unaligned_storage(dev):
    from protosam_amd.metrics import class_rows
    n, C, H, W = 3, 4, 37, 53
    big, label = _random_case(dev, n + 1, C, H, W, 0.5, seed=11)
    rows = class_rows(n, [1, 2, 3, 4], label_planes=[1, 2, 3]).tolist()
    view = big[1:]                                            # [n, C, H, W] view whose first plane is offset
    assert view.data_ptr() != big.data_ptr()
    _check(view, label, rows)
    _check(big[:, 1], label, class_rows(n + 1).tolist())      # plane stride C*H*W: every C-th plane
    _check(big[:, 1:3], label, class_rows(n + 1, [1, 2]).tolist())   # unevenly spaced planes (the wrapper packs them)
    for H, W in ((37, 53), (64, 64), (5, 4099)):
        for shift_pred, shift_label in ((1, 0), (0, 3), (5, 2), (1, 1)):
            g = torch.Generator().manual_seed(H + shift_pred)
            flat_p = (torch.rand(2 * H * W + 16, generator=g) < 0.5).to(torch.uint8).to(dev)
            flat_l = (torch.rand(2 * H * W + 16, generator=g) < 0.5).to(torch.uint8).to(dev)
            pred = flat_p[shift_pred:shift_pred + 2 * H * W].view(2, H, W)
            lab = flat_l[shift_label:shift_label + 2 * H * W].view(2, H, W)
            assert pred.storage_offset() == shift_pred and pred.data_ptr() % 16 == (flat_p.data_ptr() + shift_pred) % 16
            _check(pred, lab, [(0, 1, 0, 1), (1, 1, 1, 1), (1, 0, 0, 1)])
    # float32 planes at an element offset that is not 16-byte aligned, against uint8 and int16 labels at odd offsets
    g = torch.Generator().manual_seed(2)
    flat = (torch.rand(2 * 40 * 51 + 8, generator=g) < 0.5)
    for lt in (torch.uint8, torch.int16):
        pred = flat.float().to(dev)[3:3 + 2 * 40 * 51].view(2, 40, 51)
        lab = flat.flip(0).to(lt).to(dev)[1:1 + 2 * 40 * 51].view(2, 40, 51)
        _check(pred, lab, [(0, 1, 0, 1), (1, 1, 1, 0)])


def test_contents_and_boxes(dev):
    H, W = 5, 4099                                           # 20495 pixels: 1280 units of 16 and a tail of 15
    pred = torch.zeros((8, H, W), dtype=torch.uint8, device=dev)
    label = torch.zeros((4, H, W), dtype=torch.uint8, device=dev)
    pred[1] = 1                                              # full plane
    label[1] = 1
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for k, (y, x) in enumerate(corners):
        pred[2 + k, y, x] = 1
    pred[6].view(-1)[H * W - 15] = 1                         # first and last pixel of the vector tail, and the last whole unit
    pred[7].view(-1)[H * W - 16] = 1
    label[2, 2, 17], label[2, 4, W - 1], label[2, 0, 3] = 1, 1, 1
    label[3, :, W - 1] = 1                                   # the last column
    rows = [(p, 1, l, 1) for p in range(8) for l in range(4)]
    want = _check(pred, label, rows)
    t = want.reshape(8, 4, 12)
    assert t[0, 0, :4].tolist() == [0, 0, 0, H * W] and t[0, 0, 4:].tolist() == EMPTY_BOX * 2          # both empty
    assert t[0, 1, :4].tolist() == [0, 0, H * W, 0] and t[1, 0, :4].tolist() == [0, H * W, 0, 0]      # empty pred / empty gt
    assert t[1, 1, :4].tolist() == [H * W, 0, 0, 0] and t[1, 1, 4:].tolist() == [0, 0, W - 1, H - 1] * 2
    for k, (y, x) in enumerate(corners):
        assert t[2 + k, 0, 4:8].tolist() == [x, y, x, y]
    assert t[6, 0, 4:8].tolist() == [W - 15, H - 1, W - 15, H - 1] and t[7, 0, 4:8].tolist() == [W - 16, H - 1, W - 16, H - 1]
    assert t[0, 2, 8:].tolist() == [3, 0, W - 1, 4] and t[0, 3, 8:].tolist() == [W - 1, 0, W - 1, H - 1]
    # two rows on the same planes with different values, and a label map against a label map (Metric.record(labels=None))
    g = torch.Generator().manual_seed(9)
    a = torch.randint(0, 5, (3, 48, 40), generator=g).to(torch.uint8).to(dev)
    b = torch.randint(0, 5, (3, 48, 40), generator=g).to(torch.int16).to(dev)
    want = _check(a, b, [(k, j, k, j) for k in range(3) for j in range(5)] + [(0, 1, 0, 2), (0, 2, 0, 1)])
    assert want[:15, :3].sum() > 0


def test_row_counts_and_rows_outside(dev):
    g = torch.Generator().manual_seed(21)
    pred = torch.randint(0, 3, (64, 9, 7), generator=g).to(torch.uint8).to(dev)
    label = torch.randint(0, 3, (16, 9, 7), generator=g).to(torch.uint8).to(dev)
    for n in (1, 257, 70000):
        rows = torch.stack([torch.randint(0, 64, (n,), generator=g), torch.randint(0, 3, (n,), generator=g),
                            torch.randint(0, 16, (n,), generator=g), torch.randint(0, 3, (n,), generator=g)], dim=1).to(torch.int32)
        _check(pred, label, rows.tolist())
    # a device row table is not checked on the host: rows outside the planes keep the initial values, the others are right
    rows = torch.tensor([(0, 1, 0, 1), (64, 1, 0, 1), (3, 1, 16, 1), (-1, 1, 2, 1), (5, 2, -7, 1), (63, 2, 15, 2)], dtype=torch.int32)
    want = _check(pred, label, rows.to(dev))
    for k in (1, 2, 3, 4):
        assert want[k].tolist() == [0, 0, 0, 0] + EMPTY_BOX * 2
    assert want[0, :4].sum() == 63 and want[5, :4].sum() == 63


def test_bad_arguments_are_status_1(dev):
    from protosam_amd import ops
    ok = torch.zeros((2, 4, 4), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="psam_seg_counts failed with status 1"):
        ops.seg_counts(torch.zeros((2, 0, 4), dtype=torch.uint8, device=dev), torch.zeros((2, 0, 4), dtype=torch.uint8, device=dev),
                       [(0, 1, 0, 1)])
    with pytest.raises(RuntimeError, match="psam_seg_counts failed with status 1"):
        ops.seg_counts(ok, ok, torch.zeros((0, 4), dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        ops.seg_counts(ok.double(), ok, [(0, 1, 0, 1)])
    torch.cuda.synchronize()


def test_two_streams_no_hidden_state(dev):
    from protosam_amd import ops
    from protosam_amd.metrics import class_rows
    pa, la = _random_case(dev, 4, 4, 512, 512, 0.5, seed=1)
    pb, lb = _random_case(dev, 4, 4, 512, 512, 0.1, seed=2)
    rows = torch.from_numpy(class_rows(4, [1, 2, 3, 4])).to(dev)
    one_a, one_b = ops.seg_counts(pa, la, rows), ops.seg_counts(pb, lb, rows)
    torch.cuda.synchronize()
    ta, tb = torch.empty_like(one_a), torch.empty_like(one_b)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for _ in range(3):
        with torch.cuda.stream(s1):
            ops.seg_counts(pa, la, rows, out=ta)
        with torch.cuda.stream(s2):
            ops.seg_counts(pb, lb, rows, out=tb)
    torch.cuda.synchronize()
    assert torch.equal(ta, one_a) and torch.equal(tb, one_b) and not torch.equal(ta, tb)


def test_metric_on_device_reproduces_the_reference(dev):
    from protosam_amd.metrics import Metric
    f, res = load_fixture()
    gt, pred, organs = torch.from_numpy(f["gt"]).to(dev), torch.from_numpy(f["pred"]).to(dev), f["organs"]
    S, Z, L = gt.shape[0], gt.shape[1], organs.shape[1] - 1
    A, B, C, A4, B3 = Metric(L, S), Metric(L, S), Metric(L), Metric(L, S), Metric(L, S)
    for s in range(S):
        cls = [lb for lb in range(1, L + 1) if organs[s, lb]]
        for z in range(Z):
            for lb in cls:
                A.record((pred[s, z] == lb).to(torch.uint8), (gt[s, z] == lb).to(torch.uint8), labels=[lb], n_scan=s)
            B.record(pred[s, z], gt[s, z], n_scan=s)
            if s == 0:
                C.record(pred[s, z].long(), gt[s, z].long())
        A4.record_batch(torch.stack([(pred[s] == lb).to(torch.uint8) for lb in cls], dim=1), gt[s], cls, s)
        B3.record_batch(pred[s], gt[s], None, s)
    assert len(A4._pending) == 3 and A.tp_lst[0][0][1] != A.tp_lst[0][0][1]      # nothing has come to the host yet (NaN)
    for m, name, n in ((A, "A", S), (B, "B", S), (C, "C", 1), (A4, "A", S), (B3, "B", S)):
        assert check_against_fixture(m, name, n, res) > 40
    # record_batch equals the loop of record, entry for entry
    for one, many in ((A, A4), (B, B3)):
        for lst in ("tp_lst", "fp_lst", "fn_lst"):
            for s in range(S):
                assert np.array_equal(np.vstack(getattr(one, lst)[s]), np.vstack(getattr(many, lst)[s]), equal_nan=True)
        assert one.slice_counter == many.slice_counter


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _two_organ_case(dev, Z=6, S=512):
    """query volume, label volume with organs 1 (the synthetic organ) and 2 (an ellipse beside it), supports per z-part"""
    from protosam_amd.runner import support_set
    from protosam_amd.synth import ellipse_mask, synth_volume
    vol, qlab = synth_volume(Z, S, seed=0)
    svol, slab = synth_volume(Z, S, seed=1)
    sup_imgs, sup_masks = support_set(svol.to(dev), slab.to(dev))
    extra = torch.from_numpy(ellipse_mask(S, 0.3, 0.7, 0.1, 0.12)[None]).to(dev)
    labels = (qlab > 0).to(torch.uint8)
    labels[(labels == 0) & (extra.cpu()[0] > 0)[None]] = 2
    return vol.to(dev), labels.to(dev), sup_imgs, sup_masks, extra


def _table_checks(table, masks, labels, rows, what):
    from protosam_amd.metrics import get_dice_iou_precision_recall, score_slices
    torch.cuda.synchronize()
    want = np_counts(_planes(masks), labels.cpu().numpy(), rows)
    assert np.array_equal(table.cpu().numpy(), want), what
    non_empty = int((want[:, 0] + want[:, 1] > 0).sum())
    print(f"{what}: {non_empty} of {len(rows)} rows have a non-empty prediction")
    assert 4 * non_empty >= len(rows), (what, non_empty, len(rows))
    sc = score_slices(table)
    flat = masks.reshape((-1,) + tuple(masks.shape[-2:]))
    for i, k in enumerate(sc["rows"]):
        pp, _, lp, lv = rows[k]
        ref = float(get_dice_iou_precision_recall(flat[pp].float(), (labels[lp] == lv).float())["dice"])
        assert abs(sc["dice"][i] - ref) < 1e-6, (what, k, sc["dice"][i], ref)
    assert len(sc["rows"]) > 0
    return want


def test_evaluate_slices_classes_end_to_end(dev):
    from test_protosam_gpu import _build
    from protosam_amd.metrics import class_rows
    from protosam_amd.runner import evaluate_slices, evaluate_slices_classes, run_slices, run_slices_classes
    S, Z, classes = 512, 6, [1, 2]
    model, _ = _build(dev, "random:vit_b:1234:2", 2, use_bbox=True, use_points=True, point_mode="both")
    vol, labels, sup_imgs, sup_masks, extra = _two_organ_case(dev, Z, S)
    per_part = [[m, extra] for m in sup_masks]
    zs = list(range(Z))
    keep = torch.full((Z, 2, S, S), 7, dtype=torch.uint8, device=dev)
    table, st = evaluate_slices_classes(model, vol, labels, sup_imgs, per_part, zs, classes, dev, batch=4, keep=keep)
    assert table.is_cuda and tuple(table.shape) == (Z * 2, 12)
    rows = class_rows(Z, classes, label_planes=zs).tolist()
    _table_checks(table, keep, labels, rows, "evaluate_slices_classes")
    ref, st_ref = run_slices_classes(model, vol, sup_imgs, per_part, zs, dev, batch=4)
    assert torch.equal(keep, ref) and st == st_ref
    table2, st2 = evaluate_slices_classes(model, vol, labels, sup_imgs, per_part, zs, classes, dev, batch=4)     # one batch buffer
    assert torch.equal(table2, table) and st2 == st
    # the one-class form, on a subset of slices in another order
    zs1 = [5, 0, 2, 3]
    keep1 = torch.full((4, S, S), 7, dtype=torch.uint8, device=dev)
    t1, s1 = evaluate_slices(model, vol, labels, sup_imgs, sup_masks, zs1, dev, batch=3, keep=keep1)
    _table_checks(t1, keep1, labels, class_rows(4, None, label_planes=zs1).tolist(), "evaluate_slices")
    ref1, s1_ref = run_slices(model, vol, sup_imgs, sup_masks, zs1, dev, batch=3)
    assert torch.equal(keep1, ref1) and s1 == s1_ref
    t1b, _ = evaluate_slices(model, vol, labels, sup_imgs, sup_masks, zs1, dev, batch=3)
    assert torch.equal(t1b, t1)


def test_evaluate_slices_class_supports_end_to_end(dev):
    from test_class_supports_gpu import _inp
    from test_protosam_gpu import _build
    from protosam_amd.metrics import class_rows
    from protosam_amd.runner import class_part_table, evaluate_slices_class_supports, run_slices_class_supports
    S, Z, classes = 512, 6, [1, 2]
    model, _ = _build(dev, "random:vit_b:1234:2", 2, use_bbox=True, use_points=True, point_mode="both")
    vol, labels, sup_imgs, sup_masks, extra = _two_organ_case(dev, Z, S)
    masks = [sup_masks, [extra] * 3]
    supports = [[_inp(dev, vol[:1], [sup_imgs[p]], [masks[c][p]]) for p in range(3)] for c in range(2)]
    part_table = class_part_table(labels, classes)
    zs = list(range(Z))
    keep = torch.full((Z, 2, S, S), 7, dtype=torch.uint8, device=dev)
    table, st = evaluate_slices_class_supports(model, vol, labels, supports, part_table, zs, classes, batch=4, keep=keep)
    _table_checks(table, keep, labels, class_rows(Z, classes, label_planes=zs).tolist(), "evaluate_slices_class_supports")
    ref, st_ref = run_slices_class_supports(model, vol, supports, part_table, zs, batch=4)
    assert torch.equal(keep, ref) and st == st_ref
    table2, _ = evaluate_slices_class_supports(model, vol, labels, supports, part_table, zs, classes, batch=4)
    assert torch.equal(table2, table)
