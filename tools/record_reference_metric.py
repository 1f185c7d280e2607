"""Records tests/golden/reference_metric.npz: inputs and outputs of the reference's own scoring code on small seeded label maps.

    python tools/record_reference_metric.py --reference /path/to/the/reference/checkout

Runs the reference's `util.metric.Metric` (numpy only) and the function `get_dice_iou_precision_recall` of its
`validation_protosam.py` (taken out of the file by name and run on torch CPU tensors: the module itself needs cv2 and sacred). Only
DATA goes into the fixture: the seeded maps, which organs each scan records, and what every `get_*` returned.

Layout of the fixture (3 scans x 8 slices of 48 x 40 maps, labels 0..4):
  gt, pred            uint8 [3, 8, 48, 40] label maps
  organs              uint8 [3, 5]: organ lb of scan s is recorded by metric A iff organs[s, lb] (scan 1 never records organ 3: NaN path;
                      organ 4 is absent from scan 2 in both maps but recorded: tp + fp + fn == 0)
  metric A            Metric(4, 3), per slice and recorded organ `record(pred == lb, gt == lb, labels=[lb], n_scan=s)` (validation.py:304)
  metric B            Metric(4, 3), per slice `record(pred, gt, n_scan=s)` on the label maps
  metric C            Metric(4) (one scan), per slice of scan 0 `record(pred, gt)`
  results.names / .shapes / .offsets / .values: the returned tuples, packed (one zip member per array would cost more than
                      the data): names[i] = "<m>.<method>.<variant>.<element>" for element i of the tuple that method returned,
                      variant = all | all_raw | scan<k> | scan<k>_raw, shapes[i] its shape ("" scalar, "2,5", or "none" for an element
                      that is None), values[offsets[i]:offsets[i + 1]] its float64 entries; "<m>.<method>.<variant>.len" = tuple length
  formula.*           dice / iou / precision / recall of get_dice_iou_precision_recall for (scan, slice, organ) triples with a
                      non-empty ground truth
"""
import argparse
import ast
import contextlib
import io
import os
import sys

import numpy as np

S, Z, H, W, L = 3, 8, 48, 40, 4


def make_maps(seed=20240607):
    rng = np.random.default_rng(seed)
    gt = np.zeros((S, Z, H, W), dtype=np.uint8)
    pred = np.zeros_like(gt)
    yy, xx = np.mgrid[:H, :W]
    for s in range(S):
        for z in range(Z):
            for lb in range(1, L + 1):
                if s == 2 and lb == 4:
                    continue                                                        # organ 4 is absent from scan 2
                cy, cx = 8 + 8 * lb + rng.integers(-2, 3), 6 + 7 * lb + rng.integers(-2, 3)
                ry, rx = 3 + rng.integers(0, 3), 3 + rng.integers(0, 3)
                gt[s, z][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = lb
                py, px = cy + rng.integers(-1, 2), cx + rng.integers(-1, 2)
                pred[s, z][((yy - py) / (ry + 0.5)) ** 2 + ((xx - px) / rx) ** 2 <= 1] = lb
            noise = rng.random((H, W)) < 0.01
            pred[s, z][noise] = rng.integers(0, 4, size=int(noise.sum()))          # (never organ 4: scan 2 keeps none)
    organs = np.ones((S, L + 1), dtype=np.uint8)
    organs[:, 0] = 0
    organs[1, 3] = 0
    return gt, pred, organs


CALLS = [("get_mIoU", False), ("get_mDice", True), ("get_mPrecRecall", True), ("get_mIoU_binary", False)]


def variants(n_scans):
    """(variant name, kwargs) of every form of the get_* calls"""
    out = [("all", {}, False), ("all_raw", {"give_raw": True}, True)]
    for k in range(n_scans):
        out += [(f"scan{k}", {"n_scan": k}, False), (f"scan{k}_raw", {"n_scan": k, "give_raw": True}, True)]
    return out


def dump(store, name, metric, n_scans):
    for method, has_raw in CALLS:
        for var, kw, raw in variants(n_scans):
            if raw and not has_raw:
                continue
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                res = getattr(metric, method)(**kw)
            store[f"{name}.{method}.{var}.len"] = np.array(float(len(res)))
            for i, v in enumerate(res):
                store[f"{name}.{method}.{var}.{i}"] = None if v is None else np.asarray(v, dtype=np.float64)


def pack(results):
    names, shapes, offsets, values = [], [], [0], []
    for k, v in results.items():
        names.append(k)
        shapes.append("none" if v is None else ",".join(str(d) for d in v.shape))
        if v is not None:
            values.append(v.ravel())
        offsets.append(offsets[-1] + (0 if v is None else v.size))
    return {"results.names": np.array(names), "results.shapes": np.array(shapes), "results.offsets": np.array(offsets, dtype=np.int64),
            "results.values": np.concatenate(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "reference_metric.npz"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from util.metric import Metric
    gt, pred, organs = make_maps()
    store = {"gt": gt, "pred": pred, "organs": organs}

    A, B, C = Metric(L, S), Metric(L, S), Metric(L)
    for s in range(S):
        for z in range(Z):
            for lb in range(1, L + 1):
                if organs[s, lb]:
                    A.record((pred[s, z] == lb).astype(np.int64), (gt[s, z] == lb).astype(np.int64), labels=[lb], n_scan=s)
            B.record(pred[s, z].astype(np.int64), gt[s, z].astype(np.int64), n_scan=s)
            if s == 0:
                C.record(pred[s, z].astype(np.int64), gt[s, z].astype(np.int64))
    results = {}
    dump(results, "A", A, S)
    dump(results, "B", B, S)
    dump(results, "C", C, 1)
    store.update(pack(results))

    import torch
    src = open(os.path.join(a.reference, "validation_protosam.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_dice_iou_precision_recall")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "validation_protosam.py", "exec"), ns)
    triples, vals = [], []
    for s in range(S):
        for z in range(0, Z, 3):
            for lb in range(1, L + 1):
                g = torch.from_numpy((gt[s, z] == lb).astype(np.float32))
                if g.sum() == 0:
                    continue
                m = ns["get_dice_iou_precision_recall"](torch.from_numpy((pred[s, z] == lb).astype(np.float32)), g)
                triples.append((s, z, lb))
                vals.append([float(m[k]) for k in ("dice", "iou", "precision", "recall")])
    store["formula.triples"] = np.array(triples, dtype=np.int64)
    store["formula.values"] = np.array(vals, dtype=np.float64)
    np.savez_compressed(a.out, **store)
    print(f"wrote {a.out}: {len(store)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
