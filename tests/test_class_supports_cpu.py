"""Host logic of the per-class support path: the z-part table (dataloaders/common.py:236-249), the support slice per (class, part)
(ManualAnnoDatasetv2.py:457-477) and the entry planner of psam_alp_sim_pairs. No GPU."""
import numpy as np
import pytest

from protosam_amd.ops import plan_alp_pairs
from protosam_amd.runner import class_part_table, class_support_slices


def _labels(Z, extents):
    """label volume [Z,4,4]: class c (1, 2, ...) present on the slices of extents[c - 1]"""
    lab = np.zeros((Z, 4, 4), dtype=np.int64)
    for c, zs in enumerate(extents, start=1):
        for z in zs:
            lab[z, c - 1, 0] = c                   # (one pixel per class: the classes never overwrite each other)
    return lab


def test_class_part_table_unequal_extents():
    # class 1 on z 2..8, class 2 on z 5..6, class 3 on z 4 only; Z = 12
    lab = _labels(12, [range(2, 9), [5, 6], [4]])
    tab = class_part_table(lab, [1, 2, 3], n_parts=3)
    assert tab.shape == (3, 12) and tab.dtype.kind == "i"
    # class 1: z_min 2, z_max 8, width 6 / 3 = 2.0: (z - 2) // 2.0, clipped; z_max itself is (8 - 2) // 2 = 3 -> clipped to 2
    assert tab[0].tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2, 2]
    # class 2: z_min 5, z_max 6, width 1 / 3: (z - 5) // 0.333.. -> z = 5: 0, z = 6: 1 // (1/3) = 2 (float floor: 2.9999...)
    expect2 = [min(max(int((z - 5) // ((6 - 5) / 3)), 0), 2) for z in range(12)]
    assert tab[1].tolist() == expect2
    assert tab[1, 5] == 0 and tab[1, 6] == expect2[6] and tab[1, 11] == 2 and tab[1, 0] == 0
    # class 3: z_max == z_min -> ZeroDivisionError in the reference -> part 0 everywhere
    assert tab[2].tolist() == [0] * 12
    # the same slice in different parts for different classes
    assert tab[0, 5] == 1 and tab[1, 5] == 0


def test_class_part_table_boundaries_and_one_part():
    lab = _labels(10, [range(0, 10)])
    tab = class_part_table(lab, [1], n_parts=3)
    # width 9 / 3 = 3.0: z 0..2 -> 0, 3..5 -> 1, 6..8 -> 2, z_max = 9 -> 3 clipped to 2
    assert tab[0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2]
    assert class_part_table(lab, [1], n_parts=1)[0].tolist() == [0] * 10


def test_class_part_table_absent_class():
    lab = _labels(6, [[1, 2]])
    with pytest.raises(ValueError):
        class_part_table(lab, [1, 2])


def test_class_support_slices():
    lab = _labels(40, [range(3, 33), range(10, 13), [7]])
    sl = class_support_slices(lab, [1, 2, 3], n_parts=3)
    # pcts = 1/6, 1/2, 5/6; class 1: zlist 3..32 (30 slices) -> indices int(5.0)=5 -> z 8, 15 -> z 18, int(25.0)=24/25 -> z
    zl = list(range(3, 33))
    pcts = [1 / 6, 1 / 6 + (1 - 1 / 3) / 2, 1 / 6 + 2 * (1 - 1 / 3) / 2]
    assert sl[0] == [zl[int(p * 30)] for p in pcts]
    assert sl[1] == [10, 11, 12]
    assert sl[2] == [7, 7, 7]
    assert class_support_slices(lab, [1, 2, 3], n_parts=1) == [[zl[15]], [11], [7]]
    with pytest.raises(ValueError):
        class_support_slices(lab, [1, 4])
    with pytest.raises(ValueError):
        class_support_slices(lab, [1], n_parts=2)         # the reference asserts an odd number of parts


def test_plan_alp_pairs_entries():
    # class 0: one bank for all three slices; class 1: slices 0-1 against bank 1, slice 2 against a 2-shot support (fg banks 2, 3,
    # merged background bank 4)
    runs = [[(0, [0], 3)], [(1, [1], 2), (4, [2, 3], 1)]]
    entries, n_planes = plan_alp_pairs(runs, 3)
    assert n_planes == 2 * 3 * 2
    assert entries == [(0, 0, 0, 0), (0, 0, 1, 1), (0, 1, 0, 2), (0, 1, 1, 3), (0, 2, 0, 4), (0, 2, 1, 5),
                       (1, 0, 0, 6), (1, 0, 1, 7), (1, 1, 0, 8), (1, 1, 1, 9),
                       (4, 2, 0, 10), (2, 2, 1, 11), (3, 2, 1, 11)]
    # every plane is fed, the entries of one plane are adjacent and in shot order
    planes = [e[3] for e in entries]
    assert sorted(set(planes)) == list(range(n_planes)) and planes == sorted(planes)
    # a 3-shot foreground: three entries into one plane
    entries, _ = plan_alp_pairs([[(9, [5, 6, 7], 1)]], 1)
    assert entries == [(9, 0, 0, 0), (5, 0, 1, 1), (6, 0, 1, 1), (7, 0, 1, 1)]


def test_plan_alp_pairs_errors():
    with pytest.raises(ValueError, match="do not sum"):
        plan_alp_pairs([[(0, [0], 2), (1, [1], 2)]], 3)
    with pytest.raises(ValueError, match="do not sum"):
        plan_alp_pairs([[(0, [0], 3)], [(1, [1], 2)]], 3)
    with pytest.raises(ValueError):
        plan_alp_pairs([[(0, [], 3)]], 3)
