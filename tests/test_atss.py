"""CPU: the rule of the ATSS target assignment (include/tinyfaces_hip.h, "ATSS") as tests/atss_ref.py restates it -- by hand on a small map and
by property on seeded images --, the argument validation of its Python surface, of the C entry point and of main.py's flags, and the band
statistics that motivate it (profiles/atss_stats.txt)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import atss_ref
from oracle import targets as otgt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 17 x 21 and 9 x 11 pixels (x1, y1, x2, y2, scale)
T2 = np.array([[-8.0, -10.0, 8.0, 10.0, 1.0], [-4.0, -5.0, 4.0, 5.0, 1.0]])


def test_hand_worked_map():
    """5 x 7 cells (centres x = -1 + 8 i, y = -1 + 8 j), 2 templates, 2 faces, k = 2.
    Face 0 = [17, 7, 29, 23] (13 x 17 px, area 221) is centred on cell (2, 3) = (23, 15).  Nearest cells: (2, 3) at distance 0, then four cells
    at 64 -- (1, 3), (2, 2), (2, 4), (3, 3) -- of which the lowest cell index, (1, 3) = 10, is taken.  IoUs, list order:
      t0 (2, 3): the face lies inside the anchor [15, 5, 31, 25] (357)                       221 / 357      = 0.619
      t0 (1, 3): anchor [15, -3, 31, 17]: 13 x 11 = 143 over 357 + 221 - 143                 143 / 435      = 0.329
      t1 (2, 3): the anchor [19, 10, 27, 20] (99) lies inside the face                        99 / 221      = 0.448
      t1 (1, 3): anchor [19, 2, 27, 12]: 9 x 6 = 54 over 99 + 221 - 54                         54 / 266      = 0.203
    mean 0.400, std 0.177: only 0.619 >= 0.577 passes, its centre (23, 15) is inside: face 0 claims (t0, 2, 3).
    Face 1 = [14, 4, 34, 28] (21 x 25 px, area 525), centre (24, 16).  Nearest: (2, 3) at 2, then (2, 4) and (3, 3) tie at 50: (2, 4) = 18.
      t0 (2, 3): anchor inside the face                                                      357 / 525      = 0.680
      t0 (2, 4): anchor [23, 5, 39, 25]: 12 x 21 = 252 over 357 + 525 - 252                  252 / 630      = 0.400
      t1 (2, 3): anchor inside the face                                                       99 / 525      = 0.189
      t1 (2, 4): anchor [27, 10, 35, 20]: 8 x 11 = 88 over 99 + 525 - 88                       88 / 536      = 0.164
    mean 0.358, std 0.239: only 0.680 >= 0.597 passes, centre inside: face 1 claims (t0, 2, 3) as well, and wins it with the larger IoU.
    Face 0 is left with nothing: the losers are not compensated."""
    f0, f1 = [17.0, 7.0, 29.0, 23.0], [14.0, 4.0, 34.0, 28.0]
    hm = (5, 7)
    cm, rm, counts, faces, owner = atss_ref.atss_maps(np.array([f0, f1]), T2, k=2, hm=hm, details=True)
    assert faces[0]["cand"] == [(0, 2, 3), (0, 1, 3), (1, 2, 3), (1, 1, 3)]
    assert faces[0]["v"] == [221 / 357, 143 / 435, 99 / 221, 54 / 266]
    assert faces[0]["mean"] == pytest.approx(0.39969, abs=1e-5) and faces[0]["var"] ** 0.5 == pytest.approx(0.1772, abs=1e-4)
    assert faces[0]["passing"] == [0] and faces[0]["positive"] == [0] and faces[0]["fallback"] is None and faces[0]["claims"] == [0]
    assert faces[1]["cand"] == [(0, 2, 3), (0, 2, 4), (1, 2, 3), (1, 2, 4)]
    assert faces[1]["v"] == [357 / 525, 252 / 630, 99 / 525, 88 / 536]
    assert faces[1]["claims"] == [0]
    want = -np.ones((5, 7, 2))
    want[2, 3, 0] = 1
    assert np.array_equal(cm, want) and counts.tolist() == [0, 1] and owner[2, 3, 0] == 1 and int((owner >= 0).sum()) == 1
    wr = np.zeros((5, 7, 8), dtype=np.float32)
    wr[2, 3, 0], wr[2, 3, 2], wr[2, 3, 4], wr[2, 3, 6] = (24 - 23) / 17, (16 - 15) / 21, np.log(21 / 17), np.log(25 / 21)
    assert np.array_equal(rm, wr) and rm.dtype == np.float32
    # the other input order: the same anchor, the same winner, now face 0
    cm2, rm2, counts2 = atss_ref.atss_maps(np.array([f1, f0]), T2, k=2, hm=hm)
    assert np.array_equal(cm2, want) and np.array_equal(rm2, wr) and counts2.tolist() == [1, 0]
    # two identical faces: the lower index wins everything
    _, _, counts3 = atss_ref.atss_maps(np.array([f0, f0]), T2, k=2, hm=hm)
    assert counts3.tolist() == [1, 0]
    # face 0 alone, with a paste box that pads template 0 everywhere (its 21 px do not fit 18 rows) and leaves template 1 the cells
    # x in 1..5 of row 2 only: the list is t1 (2, 3), then the tie (2, 2) / (2, 4) -> (2, 2): 99 / 221 and 33 / 287 (3 x 11 px shared).  Two candidates of
    # different IoU: d^2 = var / 2 < var for both, neither passes, and the fallback claims the better one.
    cm4, _, counts4, faces4, _ = atss_ref.atss_maps(np.array([f0]), T2, paste=[2, 9, 45, 21], k=2, hm=hm, details=True)
    assert faces4[0]["cand"] == [(1, 2, 3), (1, 2, 2)] and faces4[0]["v"] == [99 / 221, 33 / 287]
    assert faces4[0]["passing"] == [] and faces4[0]["fallback"] == 0 and counts4.tolist() == [1] and cm4[2, 3, 1] == 1 and int((cm4 == 1).sum()) == 1
    # mirrored: the unpadded cells of the flipped mask are the same here (x in 1..5 is symmetric on 7 columns)
    cm5, _, _ = atss_ref.atss_maps(np.array([f0]), T2, paste=[2, 9, 45, 21], flip=1, k=2, hm=hm)
    assert np.array_equal(cm5, cm4)


def _random_image(seed, g=10):
    rng = np.random.RandomState(seed)
    s = rng.uniform(6, 200, g)
    x, y = rng.uniform(-10, 480, g), rng.uniform(-10, 480, g)
    boxes = np.stack([x, y, x + 0.8 * s, y + s], 1)
    boxes[1] = boxes[0] + 3.0                                  # an overlapping pair that competes
    paste = [int(rng.randint(0, 60)), int(rng.randint(0, 60)), int(rng.randint(440, 501)), int(rng.randint(440, 501))]
    return boxes, paste, int(rng.randint(0, 2))


@pytest.mark.parametrize("seed,k", [(0, 9), (1, 1), (2, 16)])
def test_positives_respect_the_rule(templates, seed, k):
    boxes, paste, flip = _random_image(seed)
    cm, rm, counts, faces, owner = atss_ref.atss_maps(boxes, templates, paste, flip, k, details=True)
    pad = atss_ref.padding(templates, paste, flip, otgt.RF, otgt.HEATMAP_SIZE)
    assert set(np.unique(cm)) <= {-1.0, 1.0} and np.array_equal(cm == 1, owner >= 0)          # exactly one owner per +1 anchor, none elsewhere
    assert int(counts.sum()) == int((cm == 1).sum()) and not bool(((cm == 1) & pad).any())
    nt = templates.shape[0]
    assert not bool(rm.reshape(63, 63, 4, nt)[np.broadcast_to((cm != 1)[:, :, None, :], (63, 63, 4, nt))].any())
    for y, x, t in zip(*np.nonzero(cm == 1)):
        f = faces[int(owner[y, x, t])]
        assert (t, y, x) in f["cand"]
        i = f["cand"].index((t, y, x))
        assert (i in f["positive"]) or (not f["positive"] and i == f["fallback"])
        rivals = [(h["v"][h["cand"].index((t, y, x))], -g) for g, h in enumerate(faces) if (t, y, x) in h["cand"] and h["cand"].index((t, y, x)) in h["claims"]]
        assert (f["v"][i], -int(owner[y, x, t])) == max(rivals)
    for f in faces:
        assert len(f["cand"]) == len(set(f["cand"])) <= k * nt and all(not pad[y, x, t] for t, y, x in f["cand"])
        assert len(f["claims"]) >= 1 or not f["cand"]


def test_python_surface_validates_the_assigner(templates):
    import torch
    from tinyfaces import ops
    from tinyfaces.datasets import SyntheticFaces, TargetAssigner, get_dataloader
    from tinyfaces.datasets.augment import collate_device
    from tinyfaces.datasets.wider_face import WIDERFace
    assert ops.check_assigner("dense_overlap", 9) == ("dense_overlap", 9) and ops.check_assigner("atss", np.int64(16)) == ("atss", 16)
    assert ops.check_assigner("atss", 1) == ("atss", 1)
    for k in (0, 17, -1, 9.0, True, "9", None):
        with pytest.raises(ValueError):
            ops.check_assigner("atss", k)
        with pytest.raises(ValueError):                               # refused before the device is looked at
            ops.atss_targets([np.zeros((1, 4))], templates, device="cpu", topk=k)
        with pytest.raises(ValueError):
            SyntheticFaces(templates, length=1, assigner="atss", atss_topk=k)
        with pytest.raises(ValueError):
            ops.atss_targets_device(torch.zeros(1, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 1, torch.zeros(25, 5, dtype=torch.float64), topk=k)
    for a in ("ATSS", "dense-overlap", "", None, 3):
        with pytest.raises(ValueError):
            ops.check_assigner(a, 9)
        with pytest.raises(ValueError):
            SyntheticFaces(templates, length=1, assigner=a)
    with pytest.raises(ValueError, match="compensat"):
        ops.check_assigner("atss", 9, (3, 0.1))
    with pytest.raises(ValueError, match="compensat"):
        SyntheticFaces(templates, length=1, assigner="atss", anchor_compensation=(3, 0.1))
    with pytest.raises(ValueError, match="compensat"):
        TargetAssigner(templates, assigner="atss", compensate=(3, 0.1))
    with pytest.raises(ValueError, match="compensat"):
        collate_device([], None, assigner="atss", compensate=(3, 0.1))
    with pytest.raises(ValueError):
        ops.atss_targets([np.zeros((1, 4))], templates, device="cpu", return_ignored_count=True)
    with pytest.raises(ValueError):
        ops.atss_targets([np.zeros((1, 4))], templates, device="cpu", ignore_boxes=[np.zeros((0, 4))], ignore=("iou", 2.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # valid arguments, the ignore combination included, go on to the usual refusal
        ops.atss_targets([np.zeros((1, 4))], templates, device="cpu", topk=16, ignore_boxes=[np.zeros((1, 4))], ignore=("iou", 0.3))
    for fn in (SyntheticFaces.__init__, TargetAssigner.__init__, WIDERFace.__init__, get_dataloader, collate_device):
        sig = inspect.signature(fn).parameters
        assert sig["assigner"].default == "dense_overlap" and sig["atss_topk"].default == 9
    assert inspect.signature(ops.atss_targets).parameters["topk"].default == 9
    plain = SyntheticFaces(templates, length=1)
    assert plain.compensation_stats is None and plain.assigner.assigner == "dense_overlap"
    atss = SyntheticFaces(templates, length=1, assigner="atss", atss_topk=7)
    assert atss.assigner.assigner == "atss" and atss.assigner.atss_topk == 7 and atss.compensation_stats.atss and atss.compensation_stats.n == 3


def test_main_flags(capsys):
    import main
    base = ["synthetic-faces", "synthetic-faces"]
    a = main.trunk_arguments(base)
    assert a.assigner == "dense_overlap" and a.atss_topk == 9 and "dense-overlap" in main.assigner_description(a) and "0.7" in main.assigner_description(a)
    a = main.trunk_arguments(base + ["--assigner", "atss"])
    assert a.assigner == "atss" and a.atss_topk == 9 and "ATSS" in main.assigner_description(a) and " 9 nearest" in main.assigner_description(a)
    a = main.trunk_arguments(base + ["--assigner", "atss", "--atss-topk", "16"])
    assert a.atss_topk == 16 and isinstance(a.atss_topk, int) and " 16 nearest" in main.assigner_description(a)
    assert main.trunk_arguments(base + ["--assigner", "dense-overlap", "--anchor-compensation", "3", "0.1"]).anchor_compensation == (3, 0.1)
    for bad in (["--assigner", "ATSS"], ["--assigner", "atss", "--atss-topk", "0"], ["--assigner", "atss", "--atss-topk", "17"], ["--atss-topk", "2.5"],
                ["--atss-topk", "x"], ["--assigner"], ["--assigner", "atss", "--anchor-compensation", "3", "0.1"]):
        with pytest.raises(SystemExit):
            main.trunk_arguments(base + bad)
    assert "--anchor-compensation" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                  # a parser error, not a traceback from the loader
        main.trunk_arguments(["synthetic", "synthetic", "--assigner", "atss"])
    assert "synthetic crops" in capsys.readouterr().err
    assert main.trunk_arguments(["synthetic", "synthetic"]).assigner == "dense_overlap"


def test_entry_point_refuses_before_it_enqueues(hip):
    """tf_targets_atss: k outside 1..16, NULL maps / templates / offsets, tstride < 4, strides <= 0, a workspace that is too small and sizes beyond
    int32 come back as error codes.  Runs without a GPU: the operands are host memory nobody dereferences."""
    l = hip.lib()
    ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -3, -4
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    wsb = l.tf_targets_atss_workspace_bytes(10, 2, 3, 5, 7)
    assert wsb >= 10 * 16 * 3 * 12 + 2 * 3 * 5 * 7 * 12 and l.tf_targets_atss_workspace_bytes(11, 2, 3, 5, 7) > wsb
    assert l.tf_targets_atss_workspace_bytes(0, 2, 3, 5, 7) == l.tf_targets_atss_workspace_bytes(1, 2, 3, 5, 7)

    def call(k=9, ws=p, ws_bytes=wsb, cls=p, reg=p, tpl=p, offs=p, tstride=5, sty=8, stx=8, nt=3, vsy=5, vsx=7):
        return l.tf_targets_atss(p, offs, 2, tpl, nt, tstride, vsy, vsx, -1, -1, sty, stx, None, None, k, None, cls, reg, ws, ws_bytes, None)

    for k in (0, -1, 17, 1 << 20):
        assert call(k=k) == ERR_ARG
    assert call(cls=None) == ERR_ARG and call(reg=None) == ERR_ARG and call(tpl=None) == ERR_ARG and call(offs=None) == ERR_ARG
    assert call(tstride=3) == ERR_ARG and call(sty=0) == ERR_ARG and call(stx=-8) == ERR_ARG
    small = l.tf_targets_atss_workspace_bytes(1, 2, 3, 5, 7)
    assert call(ws_bytes=small - 1) == ERR_WORKSPACE and call(ws_bytes=0) == ERR_WORKSPACE and call(ws=None) == ERR_WORKSPACE
    assert call(k=0, ws=None, ws_bytes=0) == ERR_ARG                   # the arguments are judged first
    assert call(nt=1 << 12, vsy=1 << 10, vsx=1 << 10) == ERR_UNSUPPORTED
    assert call(vsx=1 << 20, stx=1 << 12) == ERR_UNSUPPORTED


SIZES = (6, 8, 12, 16, 24, 40, 80, 160, 300)


def band_statistics(templates, k=9):
    """30 seeded faces per size on the 63 x 63 stride-8 grid, no padding, every face on its own (no conflicts): positives before the fallback
    of step 5.  np.random.RandomState(0); per size: w = size * U(0.9, 1.1), h = w * U(1.1, 1.4), then x, y inside the 500 x 500 canvas."""
    rng = np.random.RandomState(0)
    pad = np.zeros((63, 63, templates.shape[0]), bool)
    rows = []
    for size in SIZES:
        w = size * rng.uniform(0.9, 1.1, 30)
        h = w * rng.uniform(1.1, 1.4, 30)
        x, y = rng.uniform(0, 500 - w), rng.uniform(0, 500 - h)
        faces = [atss_ref.face_claims(b, templates, pad, k, otgt.RF, otgt.HEATMAP_SIZE) for b in np.stack([x, y, x + w, y + h], 1)]
        rows.append(dict(size=size, positives=np.array([len(f["positive"]) for f in faces]), claims=np.array([len(f["claims"]) for f in faces]),
                         cands=np.array([len(f["cand"]) for f in faces]),
                         thresh=np.array([f["mean"] + f["var"] ** 0.5 for f in faces])))
    return rows


def test_band_statistics(templates):
    rows = band_statistics(templates)
    lines = ["# ATSS positives per face BEFORE the fallback of step 5 (include/tinyfaces_hip.h, \"ATSS\"): 30 seeded faces per size, golden templates,",
             "# 63 x 63 stride-8 grid, k = 9, no padding, every face on its own.  Written by tests/test_atss.py::test_band_statistics (numpy restatement, no GPU).",
             "# No accuracy claim: this counts training targets, it does not train.",
             "# face size (px) | mean positives | min | faces with none | mean threshold (mean + std of the candidates' IoUs)"]
    for r in rows:
        p = r["positives"]
        lines.append(f"{r['size']} | {p.mean():.1f} | {int(p.min())} | {int((p == 0).sum())} | {r['thresh'].mean():.2f}")
    try:
        with open(os.path.join(ROOT, "profiles", "atss_stats.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                         # a read-only checkout still checks the facts below
    for r in rows:
        if r["size"] >= 12:
            assert int((r["positives"] == 0).sum()) == 0, r["size"]    # no 12-300 px face is without a positive before the fallback
        assert bool((r["claims"][r["cands"] > 0] >= 1).all())            # after it no face with a candidate has none
        assert bool((r["cands"] == 9 * templates.shape[0]).all())
