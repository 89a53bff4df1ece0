"""-m gpu: the ATSS target assignment (tf_targets_atss, csrc/targets_atss.hip) against tests/atss_ref.py, the numpy restatement of the rule in
include/tinyfaces_hip.h.  Every case is one small call held to: class map, regression map (the float64 values cast to float32) and match_count
array_equal to the restatement -- no tolerance anywhere."""
import numpy as np
import pytest
import torch

import atss_ref
import ignore_ref
import loss_cases as lc
import redzone
from oracle import targets as otgt

pytestmark = pytest.mark.gpu

# small template sets for the small maps (x1, y1, x2, y2, scale): 17 x 21, 9 x 11 and 33 x 41 pixels
T3 = np.array([[-8.0, -10.0, 8.0, 10.0, 1.0], [-4.0, -5.0, 4.0, 5.0, 1.0], [-16.0, -20.0, 16.0, 20.0, 1.0]])
# The kernel has one workgroup per face and no tile of faces.  The one tile it has is kChunk: the candidates of a face pass through LDS in
# chunks of 256 for the two serial sums (csrc/targets_atss.hip: kThreads), so the list lengths n = k * nt around 256 are the edge.
K_CHUNK = 256


def _hwc(x):
    return x.cpu().numpy().transpose(0, 2, 3, 1)


def _reference(boxes, t, hm, pastes, flips, k):
    out = []
    for b, bx in enumerate(boxes):
        out.append(atss_ref.atss_maps(bx, t, None if pastes is None else pastes[b], 0 if flips is None else flips[b], k, hm=hm))
    return out


def _hold(got_cm, got_rm, got_mc, ref, name):
    cm, rm = _hwc(got_cm), _hwc(got_rm)
    for b, (wcm, wrm, _) in enumerate(ref):
        assert np.array_equal(cm[b], wcm), f"{name}: image {b}: {int((cm[b] != wcm).sum())} labels differ from the rule"
        assert np.array_equal(rm[b], wrm), f"{name}: image {b}: {int((rm[b] != wrm).sum())} regression values differ"
    want = np.concatenate([r[2] for r in ref]) if ref else np.zeros(0, np.int32)
    assert got_mc.dtype == torch.int32 and np.array_equal(got_mc.cpu().numpy(), want), f"{name}: match_count {got_mc.tolist()} != {want.tolist()}"


def _run(boxes, t, hm, pastes, flips, k, name=""):
    from tinyfaces import ops
    cm, rm, mc = ops.atss_targets(boxes, t, heatmap_size=hm, paste_boxes=pastes, flips=flips, topk=k, return_match_count=True)
    ref = _reference(boxes, t, hm, pastes, flips, k)
    _hold(cm, rm, mc, ref, name)
    return ref, cm, rm, mc


def _faces(rng, g, hm):
    """g faces on the map: tiny, medium, hanging over the canvas, larger than the map, overlapping pairs."""
    vsy, vsx = hm
    W, H = 8.0 * vsx, 8.0 * vsy
    out = []
    for i in range(g):
        kind = i % 5
        if kind == 0:
            w, h = rng.uniform(4, 9, 2)
            x, y = rng.uniform(0, W - 8), rng.uniform(0, H - 8)
        elif kind == 1:
            w, h = rng.uniform(10, 40, 2)
            x, y = rng.uniform(-5, W - 5), rng.uniform(-5, H - 5)
        elif kind == 2:
            w, h = rng.uniform(6, 30, 2)
            x, y = rng.choice([-w / 2, W - w / 2, -2.0]), rng.choice([-h / 2, H - h / 2, -2.0])
        elif kind == 3:
            w, h = W * rng.uniform(1.1, 1.6), H * rng.uniform(1.1, 1.6)
            x, y = -rng.uniform(0, w - W), -rng.uniform(0, h - H)
        else:
            p = out[-1]
            dx, dy = rng.uniform(-4, 4, 2)
            out.append([p[0] + dx, p[1] + dy, p[2] + dx + 3, p[3] + dy + 2])
            continue
        out.append([x, y, x + w, y + h])
    return np.round(np.array(out, dtype=np.float64).reshape(-1, 4), 3)


GRID = [(hm, nt, g, k) for hm in ((5, 7), (9, 9)) for nt in (1, 2, 3) for g, k in ((0, 9), (1, 1), (2, 2), (3, 9), (5, 16))]


@pytest.mark.parametrize("ci", range(len(GRID)))
def test_small_maps_and_parameters(ci):
    """5 x 7 and 9 x 9 maps, 1-3 templates, 0-5 faces, k in {1, 2, 9, 16}; without padding, with a paste box, and mirrored."""
    hm, nt, g, k = GRID[ci]
    rng = np.random.RandomState(700 + ci)
    paste = [[6, 4, 8 * hm[1] - 9, 8 * hm[0] - 5]]
    pastes, flips = [(None, None), (paste, [0]), (paste, [1])][ci % 3]
    ref, _, _, _ = _run([_faces(rng, g, hm)], T3[:nt], hm, pastes, flips, k, name=f"grid[{hm},{nt},{g},{k}]")
    assert int(ref[0][2].sum()) == int((ref[0][0] == 1).sum())


def test_k_above_the_number_of_unpadded_cells():
    """A paste box that leaves the 9 x 11 template 2 x 2 cells and the others none: k = 9 and 16 take all four."""
    hm, paste = (9, 9), [[18, 17, 36, 38]]                              # cx - 4 >= 19, cx + 4 <= 36: cx in {23, 31}; cy - 5 >= 18, cy + 5 <= 38: cy in {23, 31}
    pad = atss_ref.padding(T3, paste[0], 0, otgt.RF, hm)
    assert (~pad).sum(axis=(0, 1)).tolist() == [0, 4, 0]
    for k in (9, 16, 3):
        for flip in (0, 1):
            _run([np.array([[20.0, 18.0, 33.0, 36.0], [5.0, 5.0, 60.0, 60.0]])], T3, hm, paste, [flip], k, name=f"2 x 2 cells, k = {k}")


def test_distance_ties():
    """A face centred exactly on a cell, on the midpoint of two cells (in x, and in y), and on the corner of four: the lower cell index first."""
    hm = (5, 7)
    cx, cy = -1 + 8 * 3, -1 + 8 * 2
    for ox, oy in ((0.0, 0.0), (4.0, 0.0), (0.0, 4.0), (4.0, 4.0)):
        for hw, hh in ((3.0, 4.0), (9.0, 11.0)):
            box = np.array([[cx + ox - hw, cy + oy - hh, cx + ox + hw, cy + oy + hh]])
            for k in (1, 2, 3, 5):
                _run([box], T3[:2], hm, None, None, k, name=f"tie {ox, oy} k = {k}")
    _, _, _, faces, _ = atss_ref.atss_maps(np.array([[cx + 4.0 - 3, cy + 4.0 - 4, cx + 4.0 + 3, cy + 4.0 + 4]]), T3[:1], k=4, hm=hm, details=True)
    assert faces[0]["cand"] == [(0, 2, 3), (0, 2, 4), (0, 3, 3), (0, 3, 4)]      # the four tied corners in cell-index order


def test_statistics_edges():
    hm = (5, 7)
    cx, cy = -1 + 8 * 3, -1 + 8 * 2
    on_cell = np.array([[cx - 6.0, cy - 8.0, cx + 6.0, cy + 8.0]])
    # n = 1: var = 0, the single candidate passes (d = 0 >= 0, 0 >= 0)
    ref, _, _, mc = _run([on_cell], T3[:1], hm, None, None, 1, name="n = 1")
    assert mc.tolist() == [1]
    # two candidates of different IoU: neither passes, the fallback fires
    _, _, _, faces, _ = atss_ref.atss_maps(on_cell, T3[:1], k=2, hm=hm, details=True)
    assert len(set(faces[0]["v"])) == 2 and faces[0]["passing"] == [] and faces[0]["fallback"] == 0
    _run([on_cell], T3[:1], hm, None, None, 2, name="two unequal candidates")
    # candidates of equal IoU: a face centred between two cells, k = 2: var = 0 exactly, both pass; the centres are strictly inside
    mid = np.array([[cx + 4.0 - 9, cy - 8.0, cx + 4.0 + 9, cy + 8.0]])
    _, _, _, faces, _ = atss_ref.atss_maps(mid, T3[:1], k=2, hm=hm, details=True)
    assert faces[0]["v"][0] == faces[0]["v"][1] and faces[0]["var"] == 0.0 and faces[0]["positive"] == [0, 1]
    ref, _, _, mc = _run([mid], T3[:1], hm, None, None, 2, name="equal IoUs")
    assert mc.tolist() == [2]
    # a face edge exactly on an anchor centre: the strict inequality excludes it.  x1 = 23 = the centre of column 3; k = 1 with one template
    # makes the only candidate pass, so only the centre test can keep it out -- and then the fallback claims it all the same; with k = 2 over
    # columns 3 and 4 the equal-IoU pair shows the difference: only column 4 is a positive
    edge = np.array([[23.0, cy - 8.0, 35.0, cy + 8.0]])                 # centre x = 29: columns 3 (23) and 4 (31) at 36 and 4
    _, _, _, faces, _ = atss_ref.atss_maps(edge, T3[:1], k=1, hm=hm, details=True)
    assert faces[0]["cand"] == [(0, 2, 4)]
    edge2 = np.array([[23.0, cy - 8.0, 31.0, cy + 8.0]])                # centre x = 27 = the midpoint; both edges ON the centres of columns 3 and 4
    _, _, _, faces, _ = atss_ref.atss_maps(edge2, T3[:1], k=2, hm=hm, details=True)
    assert faces[0]["passing"] == [0, 1] and faces[0]["positive"] == [] and faces[0]["fallback"] == 0
    ref, _, _, mc = _run([edge2], T3[:1], hm, None, None, 2, name="edge on the centres")
    assert mc.tolist() == [1]
    _run([edge], T3[:2], hm, None, None, 2, name="edge on one centre")
    # a face that overlaps no candidate: far outside the map.  Every v is 0, all pass (var = 0), no centre is inside: the fallback with v = 0
    far = np.array([[400.0, 300.0, 420.0, 330.0]])
    _, _, _, faces, _ = atss_ref.atss_maps(far, T3[:2], k=2, hm=hm, details=True)
    assert set(faces[0]["v"]) == {0.0} and faces[0]["positive"] == [] and faces[0]["fallback"] == 0
    ref, _, _, mc = _run([far], T3[:2], hm, None, None, 2, name="v = 0 fallback")
    assert mc.tolist() == [1]


def test_conflicts():
    hm = (5, 7)
    f0, f1 = [17.0, 7.0, 29.0, 23.0], [14.0, 4.0, 34.0, 28.0]           # tests/test_atss.py::test_hand_worked_map: both claim (t0, 2, 3), f1 wins
    ref, _, _, mc = _run([np.array([f0, f1])], T3[:2], hm, None, None, 2, name="shared anchor")
    assert mc.tolist() == [0, 1]
    ref, _, _, mc = _run([np.array([f1, f0])], T3[:2], hm, None, None, 2, name="shared anchor, other order")
    assert mc.tolist() == [1, 0]
    ref, _, _, mc = _run([np.array([f0, f0])], T3[:2], hm, None, None, 9, name="identical faces")
    assert mc[0] > 0 and mc[1] == 0
    ref, _, _, mc = _run([np.array([f1, f0, f1, f0, f1])], T3, (9, 9), None, None, 9, name="five faces, two distinct")
    assert mc[2:].tolist() == [0, 0, 0]


def test_padding():
    hm = (9, 9)
    boxes = [np.array([[10.0, 8.0, 30.0, 34.0], [3.0, 30.0, 12.0, 41.0], [40.0, 40.0, 70.0, 71.0]])]
    near = [[22, 20, 71, 71]]                                           # pads the cells nearest to the first two faces
    for flip in (0, 1):
        ref, _, _, _ = _run(boxes, T3, hm, near, [flip], 9, name=f"nearest cells padded, flip {flip}")
    pad = atss_ref.padding(T3, near[0], 0, otgt.RF, hm)
    rects = (~pad).sum(axis=(0, 1)).tolist()
    assert len(set(rects)) == 3 and min(rects) > 0                      # templates with different unpadded rectangles
    one = [[0, 0, 30, 30]]                                              # the 33 x 41 template fits nowhere, the 17 x 21 one on a single cell
    pad = atss_ref.padding(T3, one[0], 0, otgt.RF, hm)
    assert (~pad).sum(axis=(0, 1)).tolist()[2] == 0 and (~pad).sum() > 0
    _run(boxes, T3, hm, one, [0], 9, name="a template without unpadded cells")
    _run(boxes, T3, hm, one, [1], 2, name="a template without unpadded cells, mirrored")
    none = [[30, 30, 34, 34]]
    assert bool(atss_ref.padding(T3, none[0], 0, otgt.RF, hm).all())
    ref, cm, rm, mc = _run(boxes, T3, hm, none, [0], 9, name="no unpadded cell")
    assert bool((cm == -1).all()) and not bool(rm.any()) and mc.tolist() == [0, 0, 0]


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5])
def test_batches_of_one_to_five_images(B):
    """An image without faces first, in the middle and last; each image's slice equals the single-image call."""
    from tinyfaces import ops
    rng = np.random.RandomState(40 + B)
    hm = (9, 9)
    empty = {1: (), 2: (0,), 3: (1,), 4: (3,), 5: (0, 2, 4)}[B]
    boxes = [np.zeros((0, 4)) if b in empty else _faces(rng, 3 + b, hm) for b in range(B)]
    if B == 1:
        boxes = [_faces(rng, 4, hm)]
    pastes = [[2 * b, 3, 70 - b, 68] for b in range(B)]
    flips = [b % 2 for b in range(B)]
    ref, cm, rm, mc = _run(boxes, T3, hm, pastes, flips, 9, name=f"batch {B}")
    at = 0
    for b in range(B):
        cm1, rm1, mc1 = ops.atss_targets([boxes[b]], T3, heatmap_size=hm, paste_boxes=[pastes[b]], flips=[flips[b]], topk=9, return_match_count=True)
        n = mc1.numel()
        assert torch.equal(cm1[0], cm[b]) and torch.equal(rm1[0], rm[b]) and torch.equal(mc1, mc[at:at + n])
        at += n
    assert at == mc.numel()


def _golden_batch():
    """63 x 63 x 25: faces from 6 to 300 px over three images (one mirrored, one with a tight paste box), and an empty one."""
    rng = np.random.RandomState(11)
    sizes = np.array([6, 8, 12, 16, 24, 40, 80, 160, 300, 7, 10, 33], dtype=np.float64)
    w = sizes * rng.uniform(0.9, 1.1, sizes.size)
    h = w * rng.uniform(1.1, 1.4, sizes.size)
    x, y = rng.uniform(0, 500 - w), rng.uniform(0, np.maximum(500 - h, 1))
    b = np.round(np.stack([x, y, x + w, y + h], 1), 3)
    boxes = [b[:5], np.zeros((0, 4)), b[5:9], b[9:]]
    pastes = [[0, 0, 500, 500], [0, 0, 500, 500], [91, 93, 491, 493], [7, 3, 450, 433]]
    return boxes, pastes, [0, 1, 1, 0]


def test_golden_geometry_batch(templates):
    boxes, pastes, flips = _golden_batch()
    ref, cm, rm, mc = _run(boxes, templates, (63, 63), pastes, flips, 9, name="golden batch")
    assert int(mc.min()) >= 1 and int((cm == 1).sum()) == int(mc.sum()) > 100


@pytest.mark.parametrize("nt,k", [(17, 15), (16, 16), (25, 11), (25, 16)])
def test_candidate_lists_around_the_chunk(templates, nt, k):
    """n = k * nt = 255, 256, 275 and 400 candidates per face (257: test_one_candidate_past_the_chunk) around K_CHUNK = 256, the chunk in which the list passes through LDS for the two
    serial sums (the kernel's only tile: it has one workgroup per face, so no number of faces crosses anything; 37 faces here walk the
    face-to-image search over a few hundred slots all the same)."""
    assert (k * nt - K_CHUNK) in (-1, 0, 19, 144)
    rng = np.random.RandomState(nt * 100 + k)
    s = np.exp(rng.uniform(np.log(8), np.log(200), 37))
    x, y = rng.uniform(0, 480, 37), rng.uniform(0, 480, 37)
    boxes = [np.round(np.stack([x, y, x + 0.8 * s, y + s], 1), 3)]
    _run(boxes, templates[:nt], (63, 63), [[0, 0, 500, 500]], [0], k, name=f"n = {k * nt}")


def _raw_call(boxes, t, hm, pastes, flips, k, ws_boxes=None):
    """tf_targets_atss called directly, every operand and the workspace between guard bands; class map, regression map and match_count arrive
    filled with 0xFF (NaN / -1).  ws_boxes: size the workspace for that many boxes instead of the batch's own number; the outputs are then
    returned as they are, unchecked."""
    from tinyfaces import _hip
    dev = torch.device("cuda")
    kept = [lc.valid(b) for b in boxes]
    offs = np.cumsum([0] + [x.shape[0] for x in kept]).astype(np.int32)
    total, B, (vsy, vsx), nt = int(offs[-1]), len(boxes), hm, t.shape[0]
    g = lambda a: redzone.guarded_like(torch.from_numpy(np.ascontiguousarray(a)), dev)
    boxes_d = g(np.concatenate(kept) if total else np.zeros((1, 4)))
    offs_d, t_d = g(offs), g(np.asarray(t, dtype=np.float64))
    paste_d, flips_d = g(np.asarray(pastes, dtype=np.int32).reshape(B, 4)), g(np.asarray(flips, dtype=np.int32))
    cls = redzone.guarded((B, nt, vsy, vsx), torch.float32, dev)
    reg = redzone.guarded((B, 4 * nt, vsy, vsx), torch.float32, dev)
    mc = redzone.guarded((max(total, 1),), torch.int32, dev)
    l = _hip.lib()
    wsb = l.tf_targets_atss_workspace_bytes(total if ws_boxes is None else ws_boxes, B, nt, vsy, vsx)
    ws = redzone.guarded_workspace(wsb, dev)
    p = _hip.ptr
    rc = l.tf_targets_atss(p(boxes_d), p(offs_d), B, p(t_d), nt, t.shape[1], vsy, vsx, -1, -1, 8, 8, p(paste_d), p(flips_d), k, p(mc), p(cls), p(reg),
                           p(ws), wsb, _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    for name, x in dict(boxes=boxes_d, offsets=offs_d, templates=t_d, paste=paste_d, flips=flips_d, class_map=cls, reg_map=reg, match_count=mc,
                        workspace=ws).items():
        redzone.assert_guards(x, name)
    if ws_boxes is not None:
        return cls, reg, mc
    redzone.assert_written(cls, what="class_map")
    redzone.assert_written(reg, what="reg_map")
    if total:
        redzone.assert_written(mc, what="match_count")
    else:
        assert int(mc[0]) == -1                                          # no face: nothing to write
    return cls, reg, mc[:total]


@pytest.mark.parametrize("which", ["small", "golden"])
def test_guard_bands_and_garbage_outputs(templates, which):
    rng = np.random.RandomState(5)
    if which == "small":
        hm, t, k = (9, 9), T3, 16
        boxes = [_faces(rng, 5, hm), np.zeros((0, 4)), _faces(rng, 9, hm)]
        pastes, flips = [[0, 0, 72, 72], [3, 3, 60, 60], [6, 4, 67, 67]], [0, 1, 1]
    else:
        hm, t, k = (63, 63), templates, 9
        boxes, pastes, flips = _golden_batch()
    cls, reg, mc = _raw_call(boxes, t, hm, pastes, flips, k)
    _hold(cls, reg, mc, _reference(boxes, t, hm, pastes, flips, k), f"raw {which}")
    # no box in the whole batch: every label -1, every regression value 0, nothing else touched
    cls, reg, mc = _raw_call([np.zeros((0, 4))] * 2, t, hm, pastes[:2], flips[:2], k)
    assert bool((cls == -1).all()) and not bool(reg.any())


def test_workspace_too_small_for_the_device_total_writes_nothing():
    """The number of boxes is only known on the device: a workspace sized for fewer boxes than box_offsets[B] says makes every kernel return
    without writing -- the outputs keep the 0xFF they arrived with, the workspace and every guard band are untouched."""
    rng = np.random.RandomState(8)
    hm = (9, 9)
    boxes = [_faces(rng, 4, hm), np.zeros((0, 4)), _faces(rng, 3, hm)]
    pastes, flips = [[0, 0, 72, 72], [3, 3, 60, 60], [6, 4, 67, 67]], [0, 1, 1]
    for ws_boxes in (1, 6):                                              # 7 boxes on the device
        cls, reg, mc = _raw_call(boxes, T3, hm, pastes, flips, 9, ws_boxes=ws_boxes)
        for name, x in (("class_map", cls), ("reg_map", reg), ("match_count", mc)):
            n, _ = redzone.unwritten(x)
            assert n == x.numel(), f"{name}: {x.numel() - n} elements written with a workspace for {ws_boxes} boxes"
    cls, reg, mc = _raw_call(boxes, T3, hm, pastes, flips, 9, ws_boxes=7)      # exactly enough: the call of the other tests
    assert redzone.unwritten(cls)[0] == 0 and redzone.unwritten(reg)[0] == 0 and redzone.unwritten(mc)[0] == 0


def test_a_nan_box_stays_inside_its_image():
    """A box with a NaN coordinate passes the degenerate-box filter (comparisons with NaN are false).  Its image's maps are unspecified, but
    the rank key stays total (the cell index orders NaN distances), so every slot of its candidate list holds a valid anchor: nothing outside
    the operands is written, every element of the maps is, and the other image of the batch is the rule's."""
    hm = (9, 9)
    rng = np.random.RandomState(21)
    good = _faces(rng, 4, hm)
    boxes = [np.array([[10.0, 12.0, float("nan"), 40.0], [20.0, 18.0, 33.0, 36.0]]), good]
    pastes, flips = [[0, 0, 72, 72], [4, 2, 70, 66]], [0, 1]
    for k in (1, 9, 16):
        cls, reg, mc = _raw_call(boxes, T3, hm, pastes, flips, k)
        ref = atss_ref.atss_maps(good, T3, pastes[1], 1, k, hm=hm)
        assert np.array_equal(_hwc(cls)[1], ref[0]) and np.array_equal(_hwc(reg)[1], ref[1]) and np.array_equal(mc[2:].cpu().numpy(), ref[2])


def test_one_candidate_past_the_chunk():
    """n = K_CHUNK + 1 = 257 candidates: 257 is prime, so k = 1 with 257 templates (widths 9 to 41 px in steps of 1 / 8 px)."""
    nt = K_CHUNK + 1
    w = 4.0 + np.arange(nt) / 16.0
    t = np.stack([-w, -np.round(1.25 * w, 3), w, np.round(1.25 * w, 3), np.ones(nt)], 1)
    rng = np.random.RandomState(257)
    boxes = [_faces(rng, 5, (9, 9)), _faces(rng, 3, (9, 9))]
    ref, _, _, mc = _run(boxes, t, (9, 9), [[0, 0, 72, 72], [4, 2, 70, 66]], [0, 1], 1, name="n = 257")
    assert int(mc.sum()) > 0


def test_resident_entry_and_two_calls(templates):
    """The resident-operand entry against the list entry, out= included; two consecutive calls give the same bits."""
    from tinyfaces import ops
    boxes, pastes, flips = _golden_batch()
    cm, rm, mc = ops.atss_targets(boxes, templates, paste_boxes=pastes, flips=flips, topk=9, return_match_count=True)
    cm2, rm2, mc2 = ops.atss_targets(boxes, templates, paste_boxes=pastes, flips=flips, topk=9, return_match_count=True)
    assert torch.equal(cm, cm2) and torch.equal(rm, rm2) and torch.equal(mc, mc2)
    kept = [lc.valid(b) for b in boxes]
    offs = np.cumsum([0] + [x.shape[0] for x in kept])
    r = dict(boxes_d=torch.from_numpy(np.concatenate(kept)).cuda(), offs_d=torch.tensor(offs, dtype=torch.int32).cuda(), total_boxes=int(offs[-1]),
             templates_d=torch.from_numpy(np.ascontiguousarray(templates)).cuda(), paste_d=torch.tensor(pastes, dtype=torch.int32).cuda(),
             flips_d=torch.tensor(flips, dtype=torch.int32).cuda())
    dcm, drm, dmc = ops.atss_targets_device(topk=9, return_match_count=True, **r)
    assert torch.equal(dcm, cm) and torch.equal(drm, rm) and torch.equal(dmc, mc)
    out = (torch.full_like(cm, float("nan")), torch.full_like(rm, float("nan")))
    res = ops.atss_targets_device(topk=9, out=out, **r)
    assert len(res) == 2 and res[0] is out[0] and res[1] is out[1] and torch.equal(out[0], cm) and torch.equal(out[1], rm)
    other = ops.atss_targets_device(topk=1, **r)
    assert int((other[0] == 1).sum()) < int((cm == 1).sum())


def test_default_call_is_the_old_call(templates, monkeypatch):
    """Without the new keywords dense_overlap_targets makes the library calls it made; atss_targets makes its own two."""
    from tinyfaces import _hip, ops
    m = lc.mixed_batch()
    real = _hip.lib()
    seen = []

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)

    want = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=9)
    monkeypatch.setattr(ops, "lib", lambda: Spy())
    got = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=9)
    assert seen == ["tf_targets_workspace_bytes", "tf_dense_overlap_targets"] and len(got) == 2
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    del seen[:]
    from tinyfaces.datasets import TargetAssigner
    TargetAssigner(templates)(m["boxes"], paste_boxes=m["paste"], flips=m["flips"])
    assert seen == ["tf_targets_workspace_bytes", "tf_dense_overlap_targets"]
    del seen[:]
    ops.atss_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"])
    assert seen == ["tf_targets_atss_workspace_bytes", "tf_targets_atss"]
    del seen[:]
    ops.atss_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], ignore_boxes=[np.array([[5.0, 5.0, 90.0, 90.0]])] * 6)
    assert seen == ["tf_targets_atss_workspace_bytes", "tf_targets_atss", "tf_targets_apply_ignore"]


def test_ignore_pass_behind_atss(templates):
    """ignore_boxes behind ATSS = tests/ignore_ref.py applied to the restatement's map; the faces themselves with ("iou", t) make a grey band."""
    from tinyfaces import ops
    boxes, pastes, flips = _golden_batch()
    ref = _reference(boxes, templates, (63, 63), pastes, flips, 9)
    for ign, what in ((("iou", 0.3), boxes), (("iof", 0.5), [np.array([[100.0, 100.0, 260.0, 300.0]])] * 4)):
        cm, rm, mc, ic = ops.atss_targets(boxes, templates, paste_boxes=pastes, flips=flips, topk=9, return_match_count=True, ignore_boxes=what, ignore=ign,
                                          return_ignored_count=True)
        got = _hwc(cm)
        turned = []
        for b in range(4):
            want, n = ignore_ref.apply_ignore(ref[b][0], templates, what[b], ign[0], ign[1])
            assert np.array_equal(got[b], want), (ign, b)
            assert np.array_equal(_hwc(rm)[b], ref[b][1])
            turned.append(n)
        assert ic.tolist() == turned and sum(turned) > 0 and np.array_equal(mc.cpu().numpy(), np.concatenate([r[2] for r in ref]))
        assert int((cm == 1).sum()) == int(mc.sum())                      # positives stay


def test_synthetic_faces_and_engine_steps(templates, capsys):
    """SyntheticFaces(assigner="atss") feeds one fused step under the soft-margin criterion and one under focal + GIoU; the loss is finite and
    the line the training loop prints carries the restatement's counts."""
    from types import SimpleNamespace
    from tinyfaces import trainer
    from tinyfaces.datasets import SyntheticFaces
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion
    ds = SyntheticFaces(templates, length=2, seed=0, assigner="atss", atss_topk=9)
    plain = SyntheticFaces(templates, length=2, seed=0)
    batch = [ds[0], ds[1]]
    img, cm, rm = ds.collate(batch)
    img0, _, _ = plain.collate([plain[0], plain[1]])
    assert torch.equal(img, img0)
    ref = _reference([b[1] for b in batch], templates, (63, 63), [[0, 0, 500, 500]] * 2, [0, 0], 9)
    counts = np.concatenate([r[2] for r in ref])
    got_cm, got_rm = _hwc(cm), _hwc(rm)
    for b in range(2):
        assert np.array_equal(got_cm[b], ref[b][0]) and np.array_equal(got_rm[b], ref[b][1])
    trainer.print_compensation(0, 0, 1, SimpleNamespace(dataset=plain))
    assert capsys.readouterr().out == ""
    trainer.print_compensation(0, 0, 1, SimpleNamespace(dataset=ds), lag=1)           # the only batch is still "in flight"
    assert capsys.readouterr().out == ""
    trainer.print_compensation(0, 0, 1, SimpleNamespace(dataset=ds))
    assert capsys.readouterr().out == (f"Epoch: [0][0/1]\tATSS: {int((counts <= 3).sum())} of {counts.size} faces won at most 3 positives, "
                                       f"{int((counts == 0).sum())} of them none\n")
    assert ds.compensation_stats.pop() is None
    for kw in (dict(), dict(cls_loss="focal", reg_loss="giou")):
        m = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25).set_compute_dtype(torch.bfloat16)
        m.freeze_batchnorm(True)
        eng = TrainEngine(m, DetectionCriterion(25, **kw), lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cuda")
        loss = eng.step(img.float(), cm, rm)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(torch.as_tensor(loss)).all()), kw
        eng.close()
