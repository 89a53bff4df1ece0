"""CPU: the colour jitter's arithmetic (tests/color_jitter_ref.py, the numpy restatement of include/tinyfaces_hip.h's definition) pinned to
Pillow -- torchvision's ColorJitter on a PIL image IS Pillow's ImageEnhance plus a round trip through mode "HSV" -- and the host half of the
feature: the np.random draws of datasets/augment.py, validation, the --color-jitter parser."""
import numpy as np
import pytest

import color_jitter_ref as R

FACTORS = (0, 0.3, 0.875, 1, 1.25, 1.6, 2)


def _pil(img):
    Image = pytest.importorskip("PIL.Image")
    return Image.fromarray(np.ascontiguousarray(img), "RGB")


def _random_image(seed, h=37, w=53):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def planted_mean_image(k, below=False, h=20, w=30):
    """Greys whose mean L is exactly k + 0.5 (L of a grey is the grey); below=True: one pixel less, the largest mean that rounds to k."""
    n = h * w
    assert n % 2 == 0
    v = np.full(n, k, np.uint8)
    v[:n // 2] = k + 1
    v[0:6] = (k + 41, k - 39, k + 8, k - 7, k - 19, k + 22)                 # some spread, the same sum as six times k + 1
    if below:
        v[n - 1] = k - 1
    return np.repeat(np.random.RandomState(k).permutation(v).reshape(h, w, 1), 3, axis=2)


def test_blend_equals_pillow_brightness_on_all_values():
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    for f in FACTORS:
        want = np.asarray(ImageEnhance.Brightness(_pil(img)).enhance(f))
        assert np.array_equal(R.brightness(img, f), want), f


def test_luma_contrast_and_saturation_equal_pillow():
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    cases = [_random_image(s) for s in range(4)] + [_random_image(9, 500, 500), planted_mean_image(100), planted_mean_image(100, below=True)]
    for n, img in enumerate(cases):
        assert np.array_equal(R.luma(img), np.asarray(_pil(img).convert("L"))), n
        for f in FACTORS:
            assert np.array_equal(R.contrast(img, f), np.asarray(ImageEnhance.Contrast(_pil(img)).enhance(f))), (n, f)
            assert np.array_equal(R.saturation(img, f), np.asarray(ImageEnhance.Color(_pil(img)).enhance(f))), (n, f)


def test_planted_means_round_as_planted():
    assert R.contrast_mean(planted_mean_image(100)) == 101                  # exactly 100.5
    assert R.contrast_mean(planted_mean_image(100, below=True)) == 100      # 100.5 - 1 / n


def test_hsv_conversions_equal_pillow_on_all_triples():
    Image = pytest.importorskip("PIL.Image")
    v = np.arange(256, dtype=np.uint8)
    every = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(4096, 4096, 3)
    assert np.array_equal(R.rgb_to_hsv(every), np.asarray(Image.fromarray(every, "RGB").convert("HSV")))
    assert np.array_equal(R.hsv_to_rgb(every), np.asarray(Image.fromarray(every, "HSV").convert("RGB")))


def test_hue_equals_the_pil_round_trip_with_a_wrapped_shift():
    """torchvision.transforms.functional (PIL path) adjust_hue: split HSV, h += uint8(hue_factor * 255) with wrap-around, merge, back to RGB."""
    Image = pytest.importorskip("PIL.Image")
    img = _random_image(3)
    for hf in (-0.5, -0.3, -1 / 255, 0.0, 0.004, 0.25, 0.5):
        h, s, v = _pil(img).convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h += np.array(int(hf * 255)).astype(np.uint8)
        want = np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
        assert np.array_equal(R.hue(img, R.hue_shift_of(hf)), want), hf
    assert [R.hue_shift_of(x) for x in (0.0, 0.5, -0.5, -1 / 255, 0.999 / 255)] == [0, 127, 129, 255, 0]


def test_integer_mean_equals_the_double_form():
    for n in (1, 2, 3, 7, 2870, 250000, (1 << 24) - 1, 1 << 24):
        for k in (0, 1, 116, 127, 128, 253, 254):
            for d in range(-3, 4):
                for S in (k * n + n // 2 + d, k * n + (n + 1) // 2 + d, k * n + d, (k + 1) * n + d):
                    if 0 <= S <= 255 * n:
                        assert R.mean_int(S, n) == R.mean_double(S, n), (S, n)
        assert R.mean_int(255 * n, n) == R.mean_double(255 * n, n) == 255


# ---------------------------------------------------------------------------------------------- the host half
class _DeviceImage:
    """What process_inputs asks of the image before the launch."""
    is_cuda = True

    def __init__(self, h, w):
        self.shape = (h, w, 3)


@pytest.fixture
def launches(monkeypatch):
    from tinyfaces import ops
    calls = []
    monkeypatch.setattr(ops, "image_prepare", lambda img, **kw: calls.append(kw) or "x")
    return calls


BOXES = np.array([[100., 120., 180., 220.], [300., 310., 340., 360.]])


def test_draws_are_untouched_when_the_feature_is_off(launches):
    from tinyfaces.datasets import augment as da
    for seed in range(6):
        rng, ref = np.random.RandomState(seed), np.random.RandomState(seed)
        _, boxes, paste, flip = da.process_inputs(_DeviceImage(600, 800), BOXES, rng=rng)
        rnd = ref.rand()                                                  # the reference's draws, by hand: scale, crop x / y, paste x / y, flip
        rh, rw = (300, 400) if rnd < 1 / 3 else ((1200, 1600) if rnd > 2 / 3 else (600, 800))
        crop, paste_ref, _ = da.crop_decisions(rh, rw, BOXES * rh / 600, rng=ref)
        flip_ref = bool(ref.rand() > 0.5)
        assert (paste, flip) == (paste_ref, flip_ref) and launches[-1]["crop"] == crop
        assert launches[-1]["jitter"] is None
        assert rng.rand() == ref.rand()                                   # nothing else was drawn


def test_draws_come_after_the_flip_in_the_documented_order(launches):
    from tinyfaces.datasets import augment as da
    amps = (0.4, 0.3, 0.0, 0.1)
    for seed in range(6):
        rng, ref = np.random.RandomState(seed), np.random.RandomState(seed)
        chain = []
        _, boxes, paste, flip = da.process_inputs(_DeviceImage(600, 800), BOXES, rng=rng, color_jitter=amps, chain_out=chain)
        _, boxes0, paste0, flip0 = da.process_inputs(_DeviceImage(600, 800), BOXES, rng=ref)
        assert np.array_equal(boxes, boxes0) and paste == paste0 and flip == flip0
        assert {k: v for k, v in launches[-2].items() if k != "jitter"} == {k: v for k, v in launches[-1].items() if k != "jitter"}
        order = ref.permutation(4)
        b, c, h = ref.uniform(0.6, 1.4), ref.uniform(0.7, 1.3), ref.uniform(-0.1, 0.1)      # saturation has amplitude 0: no draw
        want = [{0: ("brightness", b), 1: ("contrast", c), 3: ("hue", h)}[k] for k in order.tolist() if k != 2]
        assert chain == want and launches[-2]["jitter"] == want
        assert rng.rand() == ref.rand()


def test_draw_ranges_and_zero_amplitudes():
    from tinyfaces.datasets import augment as da
    rng = np.random.RandomState(5)
    seen = set()
    for _ in range(300):
        chain = da.draw_color_jitter((1.5, 0.2, 0.9, 0.5), rng)
        seen.add(tuple(k for k, _ in chain))
        f = dict(chain)
        assert 0.0 <= f["brightness"] <= 2.5 and 0.8 <= f["contrast"] <= 1.2 and 0.1 - 1e-12 <= f["saturation"] <= 1.9 and -0.5 <= f["hue"] <= 0.5
    assert len(seen) == 24                                                # every order turns up
    rng, ref = np.random.RandomState(7), np.random.RandomState(7)
    assert da.draw_color_jitter((0, 0, 0, 0), rng) == []
    ref.permutation(4)                                                    # the order is drawn, no factor is
    assert rng.rand() == ref.rand()


def test_amplitudes_are_validated():
    from tinyfaces.datasets import augment as da
    assert da.check_color_jitter(None) is None and da.check_color_jitter([0.4, 0, 1, 0.5]) == (0.4, 0.0, 1.0, 0.5)
    for bad in ((0.1, 0.1, 0.1), (0.1, 0.1, 0.1, 0.6), (-0.1, 0, 0, 0), (0, float("nan"), 0, 0), (0, 0, float("inf"), 0), (0, 0, 0, -0.1), "abcd", 0.4):
        with pytest.raises(ValueError, match="color_jitter"):
            da.check_color_jitter(bad)
    with pytest.raises(ValueError, match="color_jitter"):
        da.process_inputs(_DeviceImage(60, 80), BOXES, color_jitter=(0, 0, 0, 1))


def test_jitter_chain_of_the_op_is_validated():
    from tinyfaces import ops
    assert ops.jitter_chain([("hue", -1 / 255), ("contrast", 1.5), ("brightness", 0), ("saturation", 2)]) == ([3, 1, 0, 2], [255.0, 1.5, 0.0, 2.0])
    assert ops.jitter_chain([("hue", 0.5)]) == ([3], [127.0]) and ops.jitter_chain([("hue", -0.5)]) == ([3], [129.0])
    for bad in ([("gamma", 1.0)], [("contrast", 1.0), ("contrast", 1.1)], [("brightness", -0.1)], [("saturation", float("nan"))],
                [("contrast", float("inf"))], [("hue", 0.51)], [("hue", float("nan"))]):
        with pytest.raises(ValueError, match="image_prepare"):
            ops.jitter_chain(bad)


def test_cpu_image_still_raises():
    import torch
    from tinyfaces import ops
    from tinyfaces.datasets import augment as da
    img = torch.zeros(20, 30, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.image_prepare(img, jitter=[("contrast", 1.2)])
    with pytest.raises(RuntimeError, match="no CPU"):
        da.process_inputs(img, BOXES, color_jitter=(0.4, 0.4, 0.4, 0.1))


def test_loader_hands_the_amplitudes_to_the_datasets(tmp_path, capsys):
    from types import SimpleNamespace
    from tinyfaces.datasets import get_dataloader
    ann = tmp_path / "train.txt"
    ann.write_text("0--Parade/a.png\n1\n50 60 120 150 0 0 0 0 0 0\n")
    args = SimpleNamespace(batch_size=2, workers=0, dataset_root=str(tmp_path), debug=False, synthetic_len=2)
    for path in (ann, "synthetic-faces"):
        assert get_dataloader(path, args)[0].dataset.color_jitter is None
        assert get_dataloader(path, args, color_jitter=[0.4, 0.3, 0.2, 0.1])[0].dataset.color_jitter == (0.4, 0.3, 0.2, 0.1)
        with pytest.raises(ValueError, match="color_jitter"):
            get_dataloader(path, args, color_jitter=(0, 0, 0, 0.7))
    capsys.readouterr()


def test_main_parses_color_jitter(capsys):
    import main
    args = main.trunk_arguments(["synthetic", "synthetic"])
    assert args.color_jitter is None and main.jitter_description(args) == "colour jitter off"
    args = main.trunk_arguments(["synthetic", "synthetic", "--color-jitter", "0.4", "0.3", "0", "0.1", "--epochs", "2"])
    assert args.color_jitter == (0.4, 0.3, 0.0, 0.1) and args.epochs == 2
    assert "brightness 0.4, contrast 0.3, saturation 0, hue 0.1" in main.jitter_description(args)
    for bad in (["0.4", "0.4", "0.4", "0.6"], ["-1", "0", "0", "0"], ["nan", "0", "0", "0"], ["inf", "0", "0", "0"], ["1", "2", "3"]):
        with pytest.raises(SystemExit):
            main.trunk_arguments(["synthetic", "synthetic", "--color-jitter"] + bad)
    capsys.readouterr()
