"""GPU: psam_image_intake (resize + normalise + zero-pad of a batch of uint8 images of different sizes in one launch) against Pillow,
against the unfused device chain it replaces, and against the float64 restatement of tests/intake_reference.py; then
`SamPredictor.set_image` through it against the host route. `S` is the kernel's parameter here, not a model's."""
import numpy as np
import pytest
import torch

import intake_reference as ir

pytestmark = pytest.mark.gpu

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
GUARD, SENTINEL = 256, 12345.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(n, C, S, dev):
    """an output tensor [n, C, S, S] that is the front of a longer buffer filled with a sentinel -> (out, whole buffer)"""
    buf = torch.full((n * C * S * S + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return buf[:n * C * S * S].view(n, C, S, S), buf


def _guard_intact(buf):
    return bool((buf[-GUARD:] == SENTINEL).all())


def _images(h, w, c):
    return [ir.random_image(h, w, c, 11 + h + w), ir.single_pixel_image(h, w, c)]


@pytest.mark.parametrize("hw,S", ir.SIZES)
def test_mode1_equals_pillow(dev, hw, S):
    from PIL import Image
    from protosam_amd import ops
    h, w = hw
    oh, ow = ir.preprocess_shape(h, w, S)
    for img in _images(h, w, 3):
        pil = np.array(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        t = torch.from_numpy(img).to(dev)
        raw, sizes = ops.image_intake([t], S, 1, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))             # mean 0 / std 1: the uint8 values themselves
        assert sizes == [(oh, ow)] and tuple(raw.shape) == (1, 3, S, S)
        got = raw[0, :, :oh, :ow].permute(1, 2, 0).cpu().numpy()
        assert np.array_equal(got, pil.astype(np.float32)), int((got != pil).sum())
        out, buf = _guarded(1, 3, S, dev)
        ops.image_intake([t], S, 1, MEAN, STD, out=out)
        ref = ops.normalize_chw(torch.from_numpy(pil).to(dev).permute(2, 0, 1)[None].contiguous(), MEAN, STD)
        assert torch.equal(_bits(out[:, :, :oh, :ow]), _bits(ref))
        pad = torch.ones((S, S), dtype=torch.bool, device=dev)
        pad[:oh, :ow] = False
        assert (_bits(out)[0][:, pad] == 0).all()                                               # +0.0 by bit pattern
        assert _guard_intact(buf)


def _chain(t, oh, ow, S):
    """the unfused device route: uint8 -> float, ops.resize_aa, (x - mean) / std, pad"""
    from protosam_amd import ops
    x = (t.permute(2, 0, 1) if t.dim() == 3 else t[None])[None].float().contiguous()
    r = ops.resize_aa(x, oh, ow)
    if t.dim() == 3:
        r = ops.normalize_chw(r, MEAN, STD)
    out = torch.zeros((1, r.shape[1], S, S), dtype=torch.float32, device=t.device)
    out[:, :, :oh, :ow] = r
    return out, r


@pytest.mark.parametrize("hw,S", ir.SIZES)
def test_mode0_equals_unfused_chain_and_float64(dev, hw, S):
    from protosam_amd import ops
    h, w = hw
    oh, ow = ir.preprocess_shape(h, w, S)
    for img in _images(h, w, 3):
        t = torch.from_numpy(img).to(dev)
        out, buf = _guarded(1, 3, S, dev)
        ops.image_intake([t], S, 0, MEAN, STD, out=out)
        chain, _ = _chain(t, oh, ow, S)
        assert torch.equal(_bits(out), _bits(chain)), int((_bits(out) != _bits(chain)).sum())
        assert _guard_intact(buf)
        ref, budget = ir.aten_f64(img.transpose(2, 0, 1), oh, ow, np.float32(MEAN), np.float32(STD))
        err = np.abs(out[0, :, :oh, :ow].cpu().numpy().astype(np.float64) - ref)
        print(f"{hw} -> {(oh, ow)}: max error {err.max():.3e}, largest share of the budget {(err / budget).max():.4f}")
        assert (err <= budget).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_mixed_batch_equals_single_launches(dev, mode):
    from protosam_amd import ops
    S = 128
    imgs = [torch.from_numpy(ir.random_image(h, w, 3, 5 + k)).to(dev) for k, ((h, w), _) in enumerate(ir.SIZES)]
    offs = np.cumsum([0] + [int(t.numel()) for t in imgs])[:-1]
    assert sum(1 for o in offs if o % 4) >= 3                   # images that start off every 4- and 16-byte boundary
    out, buf = _guarded(len(imgs), 3, S, dev)
    _, sizes = ops.image_intake(imgs, S, mode, MEAN, STD, out=out)
    assert _guard_intact(buf)
    for k, t in enumerate(imgs):
        one, sz = ops.image_intake([t], S, mode, MEAN, STD)
        assert sz[0] == sizes[k] == ir.preprocess_shape(t.shape[0], t.shape[1], S)
        assert torch.equal(_bits(out[k]), _bits(one[0])), k
    planes = [torch.from_numpy(ir.random_image(h, w, 0, 50 + k)).to(dev) for k, ((h, w), _) in enumerate(ir.SIZES)]
    outp, _ = ops.image_intake(planes, S, mode, MEAN, STD)
    for k, t in enumerate(planes):
        one, _ = ops.image_intake([t], S, mode, MEAN, STD)
        assert torch.equal(_bits(outp[k]), _bits(one[0])), k


# rectangles: (y0, y1, x0, x1). On the dyadic case the top and left edges sit at odd coordinates, where the resized value is exactly
# 0.5 (taps 1/8, 3/8, 3/8, 1/8: 3/8 + 1/8 inside), and the other two at even ones (1/8 or 7/8).
MASK_CASES = [((256, 256), 128, [(41, 100, 31, 110)]), ((100, 75), 64, [(20, 70, 10, 50)])]


@pytest.mark.parametrize("hw,S,rects", MASK_CASES)
def test_thresholded_masks(dev, hw, S, rects):
    from protosam_amd import ops
    h, w = hw
    oh, ow = ir.preprocess_shape(h, w, S)
    m = ir.rect_mask(h, w, rects)
    ref, budget = ir.aten_f64(m[None], oh, ow)
    decided = np.abs(ref[0] - 0.5) > budget[0]
    left_out = 1.0 - decided.mean()
    print(f"{hw} -> {(oh, ow)}: {100 * left_out:.3f} % of pixels within the budget of 0.5, nearest other value "
          f"{np.abs(ref[0] - 0.5)[decided].min():.4f} away")
    assert left_out <= 0.005                                     # the reference alone stays within the cap, before the GPU is asked
    t = torch.from_numpy(m).to(dev)
    out, buf = _guarded(1, 1, S, dev)
    ops.image_intake([t], S, 0, None, None, threshold=True, out=out)
    assert _guard_intact(buf)
    _, r = _chain(t, oh, ow, S)
    want = torch.zeros((1, 1, S, S), dtype=torch.float32, device=dev)
    want[:, :, :oh, :ow] = (r > 0.5).float()
    assert torch.equal(_bits(out), _bits(want))
    got = out[0, 0, :oh, :ow].cpu().numpy()
    assert set(np.unique(got)) <= {0.0, 1.0}
    assert np.array_equal(got[decided], (ref[0] > 0.5)[decided].astype(np.float32))
    half = ref[0] == 0.5
    if hw == (256, 256):
        assert half.sum() >= 60                                  # the odd edges do produce exact halves
    assert (got[half] == 0).all()                                # 0.5 is not above the threshold


def test_bad_arguments_leave_out_untouched(dev):
    from protosam_amd import ops
    S = 64
    out, buf = _guarded(1, 3, S, dev)
    good = torch.zeros((40, 50, 3), dtype=torch.uint8, device=dev)

    def refused(images, s, **kw):
        with pytest.raises(RuntimeError, match="status 1"):
            ops.image_intake(images, s, kw.pop("mode", 1), MEAN, STD, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
    refused([torch.zeros((0, 50, 3), dtype=torch.uint8, device=dev)], S)                        # a source side of 0
    refused([torch.zeros((40, 0, 3), dtype=torch.uint8, device=dev)], S)
    refused([torch.zeros((64 * 16 + 16, 100, 3), dtype=torch.uint8, device=dev)], S)            # 1040 rows -> 64: scale above 16
    refused([good], 0)                                                                          # S = 0
    refused([good], -1)
    refused([good], S, mode=2)
    refused([good], S, mode=1, threshold=True)                                                  # the threshold is for [H, W] planes in mode 0
    ops.image_intake([good], S, 1, MEAN, STD, out=out)                                          # and the good call goes through
    torch.cuda.synchronize()
    assert _guard_intact(buf) and not bool((out == SENTINEL).any())


def test_set_image_equals_host_route(dev):
    """`SamPredictor.set_image` (one uint8 upload, mode-1 intake) gives the tokens of the host route bit for bit."""
    from PIL import Image
    from protosam_amd import anysize_cases as ac
    from protosam_amd.segment_anything import SamPredictor
    from protosam_amd.synth import synth_state_dict
    sam = ac.build_sam_512()
    sam.load_state_dict(synth_state_dict(sam, ac.SAM_SEED))
    sam = sam.to(dev).eval()
    name, img, _ = ac.predictor_cases()[1]
    assert img.shape[:2] == (600, 900)
    pred = SamPredictor(sam)
    pred.set_image(img)
    assert pred.input_size == (341, 512) and tuple(pred.original_size) == (600, 900)
    with torch.no_grad():
        rz = np.array(Image.fromarray(img).resize((512, 341), Image.BILINEAR))
        t = torch.as_tensor(rz, device=dev).permute(2, 0, 1).contiguous()[None]
        tokens = sam.image_encoder.forward_tokens(sam.preprocess(t)).clone()
    assert torch.equal(_bits(pred.features_tokens), _bits(tokens))


def test_apply_image_torch_and_preprocess_on_the_device(dev):
    """Device tensors of the three ranks go through ops.resize_aa; preprocess pads them with zeros."""
    from protosam_amd import ops
    from protosam_amd.segment_anything.utils.transforms import ResizeLongestSide
    t = ResizeLongestSide(64)
    g = torch.Generator().manual_seed(9)
    for shape in ((37, 53), (3, 100, 75), (2, 3, 50, 20)):
        x = (torch.rand(shape, generator=g) * 255).to(dev)
        target = t.get_preprocess_shape(shape[-2], shape[-1], 64)
        got = t.apply_image_torch(x)
        ref = ops.resize_aa(x.reshape((-1, 1) + tuple(shape[-2:])).contiguous(), *target)
        assert tuple(got.shape) == tuple(shape[:-2]) + target and got.is_cuda
        assert torch.equal(_bits(got).reshape(-1), _bits(ref).reshape(-1))
        f64, budget = ir.aten_f64(x.reshape((-1,) + tuple(shape[-2:])).cpu().numpy(), *target)
        assert (np.abs(got.reshape(f64.shape).cpu().numpy().astype(np.float64) - f64) <= budget).all()
    y = t.preprocess(t.apply_image_torch((torch.rand((3, 100, 75), generator=g) * 255).to(dev)))
    assert tuple(y.shape) == (3, 64, 64) and (_bits(y[:, :, 48:]) == 0).all() and bool((y[:, :, :48] != 0).any())
