"""CPU: the host bookkeeping of ProtoSAM.forward_classes_batch (decoder rows per (slice, class), mask_union_seg segments)."""
import numpy as np
import pytest


def test_plan_rows_segments_and_prompts():
    from protosam_amd.protosam import plan_class_prompts
    B, C = 3, 2
    sets = {(0, 1): ([[1.0, 2.0]], [[1]]),
            (0, 0): ([[3.0, 4.0], [5.0, 6.0]], [[1], [1]]),
            (2, 0): ([[7.0, 8.0]], [[0]]),
            (1, 1): ([], [])}                                     # a plane without prompt sets is not prompted
    plan = plan_class_prompts(B, C, sets, feat_row=[0, -1, 1])
    assert plan["prompt"] == {(0, 0): 0, (0, 1): 2, (2, 0): 3}
    assert plan["spans"] == {(0, 0): (0, 2), (0, 1): (2, 1), (2, 0): (3, 1)}
    assert plan["coords"] == [[3.0, 4.0], [5.0, 6.0], [1.0, 2.0], [7.0, 8.0]]
    assert plan["img_idx"] == [0, 0, 0, 1]
    assert plan["plane_idx"] == [0, 0, 3, 2]                      # class-major planes c * B + b
    segs = plan["segs"]
    assert segs.dtype == np.int32 and segs.shape == (B * C, 3)
    assert segs.tolist() == [[0, 2, 0], [2, 1, 1], [0, 0, 2], [0, 0, 3], [3, 1, 4], [0, 0, 5]]


def test_plan_mask_prompts_and_missing_embedding():
    from protosam_amd.protosam import plan_class_prompts
    plan = plan_class_prompts(1, 2, {(0, 1): (None, [3, 5])}, feat_row=[0])
    assert plan["labels"] == [3, 5] and plan["coords"] == [] and plan["segs"].tolist() == [[0, 0, 0], [0, 2, 1]]
    with pytest.raises(ValueError):
        plan_class_prompts(1, 1, {(0, 0): (None, [1])}, feat_row=[-1])
