"""GPU: tf_image_prepare_jitter / ops.image_prepare(jitter=) / datasets.augment.process_inputs(color_jitter=) against the numpy restatement
of the colour jitter (tests/color_jitter_ref.py, pinned to Pillow by tests/test_color_jitter.py) applied to the uint8 image of the oracle's
image_prepare restatement, then ToTensor + Normalize in float32: every comparison is np.array_equal on the fp32 output.

Shapes: source 37 x 53, as it is and resized to 74 x 106, output 41 x 70 (OW % 64 != 0, OH % 4 != 0: two block columns, eleven block rows, the
last of each partial), the window pasted off the corner so that the mean-colour padding takes part in the contrast mean, mirrored and not."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import color_jitter_ref as R
from redzone import assert_guards, assert_written, guarded, guarded_workspace, unwritten
from test_oracle_augment import synth_image

pytestmark = pytest.mark.gpu

MEAN, STD, BG = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), (123, 116, 103)
OUT_HW = (41, 70)
# resized_hw, crop (y, x, h, w) of the resized image, paste (y, x), flip
GEOS = [((37, 53), (0, 0, 37, 53), (3, 11), False), ((37, 53), (0, 0, 37, 53), (3, 11), True),
        ((74, 106), (9, 20, 38, 64), (2, 5), False), ((74, 106), (9, 20, 38, 64), (2, 5), True)]
FACTORS = (0.0, 0.3, 0.875, 1.0, 1.25, 1.6, 2.0, 3.7)
FULL = {"brightness": 1.3, "contrast": 0.6, "saturation": 1.7, "hue": 0.12}


@functools.lru_cache(maxsize=None)
def source(seed=11, h=37, w=53):
    img = synth_image(seed, h, w)
    img.setflags(write=False)
    return img


def augmented_u8(img, geo, out_hw=OUT_HW):
    """The uint8 image the reference's process_inputs would hand to the transforms, through the oracle's restatement."""
    from oracle import augment as oa
    (rh, rw), (cy, cx, ch, cw), (py, px), flip = geo
    full = oa.pil_resize_u8(img, rh, rw) if (rh, rw) != img.shape[:2] else img
    buf = np.zeros(out_hw + (3,), np.uint8)
    buf[:] = BG
    buf[py:py + ch, px:px + cw] = full[cy:cy + ch, cx:cx + cw]
    return np.fliplr(buf).copy() if flip else buf


@functools.lru_cache(maxsize=None)
def base_u8(g):
    img = augmented_u8(source(), GEOS[g])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def source_on_device():
    return torch.from_numpy(source().copy()).cuda()


def normalized(u8):
    from oracle import augment as oa
    return oa.to_normalized_tensor(u8, MEAN, STD)


def prepare(img_t, geo, jitter=None, out_hw=OUT_HW, out=None):
    from tinyfaces import ops
    rhw, crop, paste, flip = geo
    return ops.image_prepare(img_t, resized_hw=rhw, crop=crop, paste=paste, flip=flip, out_hw=out_hw, mean=MEAN, std=STD, jitter=jitter, out=out)


def raw_call(hip, img_t, geo, codes, factors, out, ws=None, ws_bytes=None, out_hw=OUT_HW):
    """tf_image_prepare_jitter itself: (return code, workspace bytes the query asks for)."""
    (rh, rw), (cy, cx, ch, cw), (py, px), flip = geo
    a = hip.ImagePrepareArgs()
    a.img, a.H, a.W, a.RH, a.RW = img_t.data_ptr(), img_t.shape[0], img_t.shape[1], rh, rw
    a.crop_y, a.crop_x, a.crop_h, a.crop_w, a.paste_y, a.paste_x, a.flip, a.OH, a.OW = cy, cx, ch, cw, py, px, int(flip), out_hw[0], out_hw[1]
    for c in range(3):
        a.mean[c], a.std[c], a.bg[c] = MEAN[c], STD[c], BG[c]
    a.out = out.data_ptr()
    n = len(codes)
    op, fac = (C.c_int * 4)(*codes), (C.c_float * 4)(*factors)
    need = hip.lib().tf_image_prepare_jitter_workspace_bytes(out_hw[0], out_hw[1], n, op)
    rc = hip.lib().tf_image_prepare_jitter(C.byref(a), n, op, fac, 0 if ws is None else ws.data_ptr(),
                                           (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    return rc, need


@pytest.mark.parametrize("g", range(len(GEOS)))
def test_each_op_alone(g):
    plain = prepare(source_on_device(), GEOS[g]).cpu().numpy()
    assert np.array_equal(plain, normalized(base_u8(g)))
    for kind in ("brightness", "contrast", "saturation"):
        for f in FACTORS:
            got = prepare(source_on_device(), GEOS[g], [(kind, f)]).cpu().numpy()
            assert np.array_equal(got, normalized(R.apply_chain(base_u8(g), [(kind, f)]))), (kind, f)
            if f == 1.0:
                assert np.array_equal(got, plain), kind                  # factor 1 is the identity, bit for bit
    for hf in (0.0, 1.5 / 255, 0.25, 0.5, -0.5, -1.5 / 255):
        got = prepare(source_on_device(), GEOS[g], [("hue", hf)]).cpu().numpy()
        assert np.array_equal(got, normalized(R.apply_chain(base_u8(g), [("hue", hf)]))), hf


@pytest.mark.parametrize("g", range(len(GEOS)))
def test_hue_shifts_through_the_c_abi(hip, g):
    for shift in (0, 1, 127, 128, 255):
        out = torch.empty(3, *OUT_HW, dtype=torch.float32, device="cuda")
        rc, need = raw_call(hip, source_on_device(), GEOS[g], [3], [float(shift)], out)
        assert rc == 0 and need == 0
        want = R.hue(base_u8(g), shift)
        assert np.array_equal(out.cpu().numpy(), normalized(want)), shift
        if shift == 0:
            assert not np.array_equal(want, base_u8(g))                  # the round trip alone is not the identity


def test_all_orders_of_the_four_ops():
    g = 3
    for order in itertools.permutations(FULL):
        chain = [(k, FULL[k]) for k in order]
        got = prepare(source_on_device(), GEOS[g], chain).cpu().numpy()
        assert np.array_equal(got, normalized(R.apply_chain(base_u8(g), chain))), order


@pytest.mark.parametrize("g", range(len(GEOS)))
def test_contrast_first_last_and_alone(g):
    for chain in ([("contrast", 1.45)], [("contrast", 0.55), ("hue", -0.2), ("brightness", 1.2), ("saturation", 0.4)],
                  [("saturation", 1.9), ("brightness", 0.7), ("hue", 0.31), ("contrast", 1.8)], [("brightness", 1.4), ("contrast", 0.0)],
                  [("contrast", 2.5), ("saturation", 0.0)]):
        got = prepare(source_on_device(), GEOS[g], chain).cpu().numpy()
        assert np.array_equal(got, normalized(R.apply_chain(base_u8(g), chain))), chain


@pytest.mark.parametrize("flip", [False, True])
def test_planted_half_integer_mean(flip):
    """Greys in the window so that, padding included, the mean L is exactly k + 0.5 (rounds up), then one grey less (rounds down)."""
    geo = (GEOS[0][0], GEOS[0][1], GEOS[0][2], flip)
    n, k = OUT_HW[0] * OUT_HW[1], 105
    pad_l = int(R.luma(np.array(BG, np.uint8)))
    need = k * n + n // 2 - (n - 37 * 53) * pad_l - 37 * 53 * 100            # greys of 100, `need` of them 101
    assert n % 2 == 0 and 0 < need < 37 * 53
    for below in (False, True):
        v = np.full(37 * 53, 100, np.uint8)
        v[:need - int(below)] = 101
        src = np.repeat(np.random.RandomState(4).permutation(v).reshape(37, 53, 1), 3, axis=2)
        base = augmented_u8(src, geo)
        S = int(R.luma(base).astype(np.int64).sum())
        assert 2 * S + n == (2 * (k + 1) * n if not below else 2 * (k + 1) * n - 2) and R.contrast_mean(base) == (k if below else k + 1)
        for chain in ([("contrast", 1.6)], [("contrast", 0.3), ("saturation", 1.2)]):
            got = prepare(torch.from_numpy(src).cuda(), geo, chain).cpu().numpy()
            assert np.array_equal(got, normalized(R.apply_chain(base, chain))), (below, chain)


def test_training_window_500():
    img = synth_image(77, 300, 420)
    geo = ((600, 840), (37, 111, 400, 333), (60, 90), True)
    base = augmented_u8(img, geo, (500, 500))
    chain = [("saturation", 1.35), ("contrast", 0.72), ("hue", -0.07), ("brightness", 1.18)]
    d = torch.from_numpy(img).cuda()
    got = prepare(d, geo, chain, out_hw=(500, 500)).cpu().numpy()
    assert np.array_equal(got, normalized(R.apply_chain(base, chain)))
    got = prepare(d, geo, chain[2:], out_hw=(500, 500)).cpu().numpy()       # the one-launch form
    assert np.array_equal(got, normalized(R.apply_chain(base, chain[2:])))


def test_second_run_gives_the_same_bits():
    chain = [("brightness", 1.3), ("contrast", 1.7), ("saturation", 0.5)]
    first = prepare(source_on_device(), GEOS[2], chain).cpu().numpy()
    prepare(source_on_device(), GEOS[1], [("contrast", 0.2)])                 # leaves another image and other sums in the workspace
    again = prepare(source_on_device(), GEOS[2], chain).cpu().numpy()
    assert np.array_equal(first, again) and np.array_equal(first, normalized(R.apply_chain(base_u8(2), chain)))


@pytest.mark.parametrize("g", [1, 2])
def test_writes_stay_inside_out_and_workspace(hip, g):
    chain = [("brightness", 1.2), ("contrast", 1.5), ("hue", 0.1)]
    codes, factors = [0, 1, 3], [1.2, 1.5, float(R.hue_shift_of(0.1))]
    out = guarded((3,) + OUT_HW, torch.float32, "cuda")
    blocks = ((OUT_HW[1] + 63) // 64) * ((OUT_HW[0] + 3) // 4)
    need = (blocks * 4 + 255) // 256 * 256 + 3 * OUT_HW[0] * OUT_HW[1]      # the documented formula
    ws = guarded_workspace(need, "cuda", pitch_bytes=3 * OUT_HW[1])
    rc, asked = raw_call(hip, source_on_device(), GEOS[g], codes, factors, out, ws)
    assert rc == 0 and asked == need
    assert_guards(out, "out")
    assert_guards(ws, "workspace")
    assert_written(out, what="out")
    assert unwritten(ws[:blocks * 4].view(torch.int32))[0] == 0             # every partial sum the second launch reads was written
    assert np.array_equal(out.cpu().numpy(), normalized(R.apply_chain(base_u8(g), chain)))
    # the one-launch form touches no workspace
    out1 = guarded((3,) + OUT_HW, torch.float32, "cuda")
    ws1 = guarded_workspace(need, "cuda")
    rc, asked = raw_call(hip, source_on_device(), GEOS[g], [2, 0], [1.4, 0.8], out1, ws1)
    assert rc == 0 and asked == 0
    assert_guards(out1, "out")
    assert_written(out1, what="out")
    assert unwritten(ws1)[0] == ws1.numel()
    assert np.array_equal(out1.cpu().numpy(), normalized(R.apply_chain(base_u8(g), [("saturation", 1.4), ("brightness", 0.8)])))


def test_refusals_enqueue_nothing(hip):
    from tinyfaces import ops
    out = guarded((3,) + OUT_HW, torch.float32, "cuda")
    rc, need = raw_call(hip, source_on_device(), GEOS[0], [1], [1.5], torch.empty(3, *OUT_HW, device="cuda"), torch.empty(1 << 16, dtype=torch.uint8, device="cuda"))
    assert rc == 0 and need > 0
    ws = guarded_workspace(need, "cuda")
    bad = [([1, 1], [1.5, 1.2], None), ([4], [1.0], None), ([-1], [1.0], None), ([0], [-0.5], None), ([2], [float("nan")], None),
           ([1], [float("inf")], None), ([3], [256.0], None), ([3], [-1.0], None), ([3], [1.5], None), ([0, 1], [1.0, 1.5], need - 1), ([1], [1.5], 0)]
    for codes, factors, ws_bytes in bad:
        rc, _ = raw_call(hip, source_on_device(), GEOS[0], codes, factors, out, ws, ws_bytes)
        assert rc == (-4 if ws_bytes is not None else -1), (codes, factors, ws_bytes)
    a_bad_window = (GEOS[0][0], (0, 0, 38, 53), GEOS[0][2], False)          # what tf_image_prepare refuses
    assert raw_call(hip, source_on_device(), a_bad_window, [0], [1.2], out, ws)[0] == -1
    torch.cuda.synchronize()
    assert unwritten(out)[0] == out.numel() and unwritten(ws)[0] == ws.numel()
    assert_guards(out, "out")
    assert_guards(ws, "workspace")
    with pytest.raises(ValueError):
        ops.image_prepare(source_on_device(), jitter=[("contrast", 1.0), ("contrast", 1.0)])
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.image_prepare(torch.from_numpy(source().copy()), jitter=[("contrast", 1.2)])
    with pytest.raises(ValueError, match="2\\^24"):                         # raised on the host, in front of the library call
        ops.image_prepare(source_on_device(), out_hw=(4097, 4096), out=torch.empty(1, device="cuda"), jitter=[("contrast", 1.2)])


def test_process_inputs_with_color_jitter():
    from oracle import augment as oa
    from tinyfaces.datasets import augment as da
    img = synth_image(21, 200, 260)
    d = torch.from_numpy(img).cuda()
    boxes = np.array([[30., 40., 90., 120.], [150., 60., 200., 130.]])
    amps, size, scales = (0.4, 0.5, 0.6, 0.2), (120, 150), set()
    for seed in range(5):
        ref = oa.process_inputs(img, boxes.copy(), input_size=size, rng=np.random.RandomState(seed))
        scales.add(ref["scale"])
        x0, b0, paste0, flip0 = da.process_inputs(d, boxes.copy(), input_size=size, rng=np.random.RandomState(seed), color_jitter=None)
        assert np.array_equal(x0.cpu().numpy(), normalized(ref["img"])) and np.array_equal(b0, ref["bboxes"])       # off: what it always gave
        chain = []
        x, b, paste, flip = da.process_inputs(d, boxes.copy(), input_size=size, rng=np.random.RandomState(seed), color_jitter=amps, chain_out=chain)
        assert np.array_equal(b, b0) and paste == paste0 == ref["paste_box"] and flip == flip0 == ref["flip"]
        assert sorted(k for k, _ in chain) == sorted(R.KINDS)
        assert np.array_equal(x.cpu().numpy(), normalized(R.apply_chain(ref["img"], chain))), seed
    assert len(scales) > 1


def test_widerface_collate_with_color_jitter(tmp_path, templates):
    from tinyfaces.datasets import augment as da
    from tinyfaces.datasets.wider_face import WIDERFace
    ann = tmp_path / "train.txt"
    ann.write_text("0--Parade/a.png\n1\n50 60 120 150 0 0 0 0 0 0\n")
    amps = (0.3, 0.3, 0.3, 0.05)
    samples = [(synth_image(40 + k, 300, 420), np.array([[50., 60., 170., 210.]])) for k in range(2)]
    ds = WIDERFace(ann, templates, split="train", color_jitter=amps)
    np.random.seed(77)
    x, cm, rm = ds.collate(samples)
    torch.cuda.synchronize()
    np.random.seed(77)
    for i, (img, bb) in enumerate(samples):
        xi, _, _, _ = da.process_inputs(torch.from_numpy(img).cuda(), bb, color_jitter=amps)
        assert torch.equal(xi, x[i]), i
    assert cm.shape == (2, 25, 63, 63) and rm.shape == (2, 100, 63, 63)
    off = WIDERFace(ann, templates, split="train")
    np.random.seed(77)
    x_off, _, _ = off.collate(samples)
    assert off.color_jitter is None and not torch.equal(x_off, x)


def test_synthetic_faces_collate_with_color_jitter(templates):
    from tinyfaces.datasets import SyntheticFaces
    from tinyfaces.datasets import augment as da
    amps = (0.4, 0.4, 0.4, 0.1)
    plain, jit, zero = (SyntheticFaces(templates, length=2, seed=3, color_jitter=cj) for cj in (None, amps, (0, 0, 0, 0)))
    batch = [jit[0], jit[1]]
    assert batch[0][0].dtype == torch.uint8 and batch[0][0].shape == (500, 500, 3)
    np.random.seed(5)
    x, cm, rm = jit.collate(batch)
    np.random.seed(5)
    for i, (u8, _) in enumerate(batch):
        chain = da.draw_color_jitter(amps)
        assert np.array_equal(x[i].cpu().numpy(), normalized(R.apply_chain(u8.numpy(), chain))), i
    x0 = plain.collate([plain[0], plain[1]])[0]
    xz = zero.collate([zero[0], zero[1]])[0]
    assert torch.equal(x0, xz) and not torch.equal(x0, x)                   # amplitudes of 0: the host-normalised samples, bit for bit
