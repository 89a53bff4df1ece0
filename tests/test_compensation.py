"""CPU: the rule of the scale-compensated anchor matching (include/tinyfaces_hip.h) as tests/comp_ref.py restates it, the argument
validation of its Python surface, of the C entry point and of main.py's flag, and the band statistics that motivate it."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import comp_ref
from oracle import targets as otgt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_worked_map():
    """3 x 4 cells, one template, two faces.  Flat index = y * 4 + x.  Face 0 owns the left half (x < 2), face 1 the right half."""
    v = np.zeros((3, 4, 1, 2))
    v[:, :, 0, 0] = [[0.50, 0.20, 0.0, 0.0], [0.75, 0.40, 0.0, 0.0], [0.20, 0.05, 0.0, 0.0]]
    v[:, :, 0, 1] = [[0.0, 0.0, 0.25, 0.25], [0.0, 0.0, 0.29, 0.10], [0.0, 0.0, 0.25, 0.02]]
    F = -np.ones((3, 4, 1))
    F[1, 0, 0] = 1                                   # IoU 0.75 >= 0.7
    F[0, 0, 0] = F[1, 1, 0] = 0                      # ignored band
    pad = np.zeros((3, 4, 1), bool)
    pad[0, 2, 0] = True                              # one of face 1's three tied anchors is padded
    out, counts = comp_ref.compensate(F, v, pad, 3, 0.1)
    want = F.copy()
    want[0, 0, 0] = want[1, 1, 0] = 1                # face 0: count 1, its two best candidates 0.50 and 0.40 (0.20 twice stays)
    want[1, 2, 0] = want[0, 3, 0] = want[2, 2, 0] = 1      # face 1: count 0; 0.29, then the tie at 0.25: flat 3 before flat 10 (flat 2 is padded)
    assert np.array_equal(out, want) and counts.tolist() == [3, 3]
    # N = 2: face 1 takes 0.29 and the LOWER flat index of the tie
    out, counts = comp_ref.compensate(F, v, pad, 2, 0.1)
    assert out[1, 2, 0] == 1 and out[0, 3, 0] == 1 and out[2, 2, 0] == -1 and out[0, 0, 0] == 1 and out[1, 1, 0] == 0 and counts.tolist() == [2, 2]
    # T above every candidate of face 1; N above the candidates of face 0: all of them, no more
    out, counts = comp_ref.compensate(F, v, pad, 64, 0.3)
    assert counts.tolist() == [3, 0] and int((out == 1).sum()) == 3
    # nothing else changed
    assert np.array_equal(out[want != 1], F[want != 1])


def _random_image(seed, templates, sizes=(8, 120), g=12):
    rng = np.random.RandomState(seed)
    s = rng.uniform(sizes[0], sizes[1], g)
    x, y = rng.uniform(-10, 480, g), rng.uniform(-10, 480, g)
    boxes = np.stack([x, y, x + 0.8 * s, y + s], 1)
    paste = [int(rng.randint(0, 60)), int(rng.randint(0, 60)), int(rng.randint(440, 501)), int(rng.randint(440, 501))]
    return boxes, paste, int(rng.randint(0, 2)), rng.rand(63, 63, 25, g)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_promotions_respect_the_rule(templates, seed):
    boxes, paste, flip, noise = _random_image(seed, templates)
    for N, T in ((1, 0.1), (3, 0.1), (3, 0.3), (64, 0.05), (5, 0.5)):
        cm, F, rm, counts = comp_ref.compensated_maps(boxes, templates, paste, flip, noise, N, T)
        pad = otgt.get_padding(templates, paste)
        pad = np.fliplr(pad) if flip else pad
        ocm, orm, iou = otgt.get_heatmaps(boxes.copy(), templates, pad, noise=noise)
        assert np.array_equal(cm, ocm) and np.array_equal(rm, orm)          # the regression map passes through: the rule never sees it
        changed = F != cm
        assert bool((F[changed] == 1).all()) and not bool((changed & pad).any()) and not bool((changed & (cm == 1)).any())
        own, best = iou.argmax(axis=3), iou.max(axis=3)
        assert bool((best[changed] >= T).all())
        before = comp_ref.owned_positives(cm, iou)
        for g in range(boxes.shape[0]):
            added = int((changed & (own == g)).sum())
            assert added <= max(0, N - int(before[g])) and int(counts[g]) == int(before[g]) + added
            if before[g] >= N:
                assert added == 0
            elif added < N - before[g]:                                          # fewer candidates than needed: every one was promoted
                left = (own == g) & ~pad & (F != 1) & (best >= T)
                assert not bool(left.any())
            # the promoted ones are the best: no candidate left behind beats a promoted one
            left = (own == g) & ~pad & (F != 1) & (best >= T)
            if added and left.any():
                assert float(best[left].max()) <= float(best[changed & (own == g)].min())


def test_faces_with_enough_positives_leave_the_map_alone(templates):
    k = templates[[5, 12, 20]]
    cx, cy = -1 + 8 * np.array([10, 30, 50]), -1 + 8 * np.array([12, 40, 22])
    boxes = np.stack([cx + k[:, 0], cy + k[:, 1], cx + k[:, 2], cy + k[:, 3]], 1)
    noise = np.random.RandomState(4).rand(63, 63, 25, 3)
    cm, F, rm, counts = comp_ref.compensated_maps(boxes, templates, [0, 0, 500, 500], 0, noise, 3, 0.1)
    assert bool((counts >= 3).all()) and np.array_equal(cm, F)


def test_the_rule_does_not_know_the_regression_map():
    assert list(inspect.signature(comp_ref.compensate).parameters) == ["class_map", "iou", "pad", "N", "T"]
    F = -np.ones((2, 2, 1))
    out = comp_ref.compensate(F, np.full((2, 2, 1, 1), 0.2), np.zeros((2, 2, 1), bool), 2, 0.1)
    assert len(out) == 2 and out[0].shape == F.shape and out[1].tolist() == [2] and int((F == 1).sum()) == 0      # (the input is not modified)


def test_python_surface_validates_compensate(templates):
    import torch
    from tinyfaces import ops
    from tinyfaces.datasets import SyntheticFaces
    from tinyfaces.datasets.augment import collate_device
    assert ops.check_compensate(None) is None and ops.check_compensate((3, 0.1)) == (3, 0.1) and ops.check_compensate([np.int64(64), 0.01]) == (64, 0.01)
    assert ops.check_compensate((1, 0.69999)) == (1, 0.69999) and ops.check_compensate((2, 0.75), pos_thresh=0.8) == (2, 0.75)
    bad = [(0, 0.1), (65, 0.1), (-1, 0.1), (2.0, 0.1), (True, 0.1), ("3", 0.1), (3, 0.0099), (3, 0.7), (3, 1.0), (3, float("nan")), (3, float("inf")),
           (3, -0.1), (3, "0.1"), (3,), (3, 0.1, 1), 3, "ab"]
    for c in bad:
        with pytest.raises(ValueError):
            ops.check_compensate(c)
        with pytest.raises(ValueError):                               # refused before the device is looked at
            ops.dense_overlap_targets([np.zeros((1, 4))], templates, device="cpu", compensate=c)
        with pytest.raises(ValueError):
            SyntheticFaces(templates, length=1, anchor_compensation=c)
    with pytest.raises(ValueError):
        ops.dense_overlap_targets([np.zeros((1, 4))], templates, device="cpu", return_match_count=True)
    with pytest.raises(ValueError):
        ops.dense_overlap_targets_device(torch.zeros(1, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 1, torch.zeros(25, 5, dtype=torch.float64),
                                         compensate=(0, 0.1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a valid pair goes on to the usual refusal: there is no host path
        ops.dense_overlap_targets([np.zeros((1, 4))], templates, device="cpu", compensate=(3, 0.1))
    for fn, name in ((ops.dense_overlap_targets, "compensate"), (ops.dense_overlap_targets_device, "compensate"), (collate_device, "compensate"),
                     (SyntheticFaces.__init__, "anchor_compensation")):
        assert inspect.signature(fn).parameters[name].default is None
    from tinyfaces.datasets import get_dataloader
    from tinyfaces.datasets.wider_face import WIDERFace
    assert inspect.signature(get_dataloader).parameters["anchor_compensation"].default is None
    assert inspect.signature(WIDERFace.__init__).parameters["anchor_compensation"].default is None
    assert SyntheticFaces(templates, length=1).compensation_stats is None
    assert SyntheticFaces(templates, length=1, anchor_compensation=(3, 0.1)).assigner.compensate == (3, 0.1)


def test_main_flag(capsys):
    import main
    base = ["synthetic-faces", "synthetic-faces"]
    assert main.trunk_arguments(base).anchor_compensation is None
    a = main.trunk_arguments(base + ["--anchor-compensation", "3", "0.1"])
    assert a.anchor_compensation == (3, 0.1) and isinstance(a.anchor_compensation[0], int)
    assert "3 positive anchors" in main.compensation_description(a) and "0.1" in main.compensation_description(a)
    assert "off" in main.compensation_description(main.trunk_arguments(base))
    for bad in (["0", "0.1"], ["65", "0.1"], ["2.5", "0.1"], ["3", "0.7"], ["3", "0.005"], ["3", "nan"], ["3", "inf"], ["x", "0.1"], ["3"]):
        with pytest.raises(SystemExit):
            main.trunk_arguments(base + ["--anchor-compensation"] + bad)
    capsys.readouterr()


def test_entry_point_refuses_before_it_enqueues(hip):
    """tf_dense_overlap_targets_comp: N outside 1..64, T outside [0.01, pos_thresh) or not finite, and a workspace that is too small come back
    as error codes.  Runs without a GPU: the operands are host memory nobody dereferences."""
    l = hip.lib()
    ERR_ARG, ERR_WORKSPACE = -1, -4
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    wsb = l.tf_targets_comp_workspace_bytes(10, 2, 3, 5, 7)
    assert wsb >= 10 * 16 + 2 * 3 * 5 * 7 * 12 and l.tf_targets_comp_workspace_bytes(11, 2, 3, 5, 7) > wsb
    assert l.tf_targets_comp_workspace_bytes(0, 2, 3, 5, 7) == l.tf_targets_comp_workspace_bytes(1, 2, 3, 5, 7)
    assert l.tf_targets_comp_workspace_bytes(100, 12, 25, 63, 63) > l.tf_targets_workspace_bytes(100) + 12 * 25 * 63 * 63 * 12 - 1

    def call(N=3, T=0.1, ws=p, ws_bytes=wsb, pos=0.7, cls=p):
        return l.tf_dense_overlap_targets_comp(p, p, 2, p, 3, 5, 5, 7, -1, -1, 8, 8, None, None, None, None, 0, pos, 0.3, N, T, None, cls, p, ws, ws_bytes, None)

    for N in (0, -1, 65, 1 << 20):
        assert call(N=N) == ERR_ARG
    for T in (0.0, 0.00999, 0.7, 0.9, -0.5, float("nan"), float("inf"), -float("inf")):
        assert call(T=T) == ERR_ARG
    assert call(T=0.75, pos=0.7) == ERR_ARG
    assert call(cls=None) == ERR_ARG
    small = l.tf_targets_comp_workspace_bytes(1, 2, 3, 5, 7)
    assert call(ws_bytes=small - 1) == ERR_WORKSPACE and call(ws_bytes=0) == ERR_WORKSPACE and call(ws=None) == ERR_WORKSPACE
    assert call(N=0, ws=None, ws_bytes=0) == ERR_ARG                   # the arguments are judged first


BANDS = ((8, 16), (16, 40), (40, 120))


def band_statistics(templates):
    """30 seeded faces per size band on the 500 x 500 canvas, one image per band: positives per face (by owner) without the stage and with
    (3, 0.1).  np.random.RandomState(0); per band: side s, aspect a in [0.7, 1.0], x, y, then the noise."""
    rng = np.random.RandomState(0)
    rows = []
    for lo, hi in BANDS:
        s = rng.uniform(lo, hi, 30)
        a = rng.uniform(0.7, 1.0, 30)
        x = rng.uniform(0, 500 - s * a)
        y = rng.uniform(0, 500 - s)
        boxes = np.stack([x, y, x + s * a, y + s], 1)
        noise = rng.rand(63, 63, 25, 30)
        cm, F, _, after = comp_ref.compensated_maps(boxes, templates, [0, 0, 500, 500], 0, noise, 3, 0.1)
        _, _, iou = otgt.get_heatmaps(boxes.copy(), templates, otgt.get_padding(templates, [0, 0, 500, 500]), noise=noise)
        before = comp_ref.owned_positives(cm, iou)
        rows.append(dict(band=(lo, hi), before=before, after=after, positives_before=int((cm == 1).sum()), positives_after=int((F == 1).sum())))
    return rows


def test_band_statistics(templates):
    rows = band_statistics(templates)
    lines = ["# positives per face (anchors labelled +1 that the face owns), 30 seeded faces per size band, golden templates, 500 x 500 canvas;",
             "# without the stage and with compensate=(3, 0.1).  Written by tests/test_compensation.py::test_band_statistics (numpy oracle, no GPU).",
             "# No accuracy claim: this counts training targets, it does not train.",
             "# face side (px) | median | share < 3 | faces with none | positives || with (3, 0.1): median | share < 3 | positives"]
    for r in rows:
        b, a = r["before"], r["after"]
        lines.append(f"{r['band'][0]}-{r['band'][1]} | {np.median(b):g} | {100 * (b < 3).mean():.0f} % | {int((b == 0).sum())} | {r['positives_before']} || "
                     f"{np.median(a):g} | {100 * (a < 3).mean():.0f} % | {r['positives_after']}")
    try:
        with open(os.path.join(ROOT, "profiles", "anchor_compensation_stats.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                         # a read-only checkout still checks the facts below
    tiny, _, large = rows
    assert bool((tiny["before"] < 3).all())                          # every 8-16-px face has fewer than 3 positives without the stage
    assert float((tiny["after"] < 3).mean()) <= 0.10                 # with (3, 0.1) at most 10 % still do
    assert np.array_equal(large["before"], large["after"]) and large["positives_before"] == large["positives_after"]
