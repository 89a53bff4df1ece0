"""-m gpu: the device WIDER evaluator against the host one, exactly.  The match kernel's counted / recalled are integers and must be
array_equal to wider_eval.image_evaluation per setting; the PR kernel's table must equal the sum of wider_eval.image_pr_info as integers;
DeviceEvaluator's AP must be `==` evaluate_setting(norm_scores(...))'s and its curve array_equal.  No tolerance anywhere: the host
evaluator is the reference.  Shapes are the edges of csrc/wider_eval.hip: N around the 64-lane wave and the 256-thread chunk, G around the
LDS tile (ops.WIDER_GT_TILE), segment counts around the 256 segments of one launch, empty segments first, in the middle and last."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import wider_ref
from gpu_util import report
from redzone import assert_guards, assert_written, guarded, guarded_like, guarded_workspace

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
DEV = "cuda"


def _match(images, iou_thresh=0.5):
    from tinyfaces import ops
    rows, doff, gt, goff, keep = wider_ref.concat(images)
    counted, recalled = ops.wider_match_batched(torch.from_numpy(rows).to(DEV), doff, torch.from_numpy(gt).to(DEV), goff,
                                                torch.from_numpy(keep).to(DEV), iou_thresh)
    assert counted.dtype == recalled.dtype == torch.int32 and tuple(counted.shape) == tuple(recalled.shape) == (keep.shape[0], rows.shape[0])
    return counted.cpu().numpy().astype(np.int64), recalled.cpu().numpy().astype(np.int64)


def _check(images, what):
    got_c, got_r = _match(images)
    want_c, want_r = wider_ref.host_counts_batched(images)
    assert np.array_equal(got_c, want_c), what
    assert np.array_equal(got_r, want_r), what
    return want_c, want_r


# --------------------------------------------------------------------------- the match kernel
@pytest.mark.parametrize("nset", [1, 3])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 1025])
def test_match_detection_counts(N, nset):
    rng = np.random.RandomState(100 + N)
    c, r = _check([wider_ref.random_image(rng, N, 9, nset)], (N, nset))
    if N >= 63:
        assert r[:, -1].max() > 0 and (np.diff(c, axis=1) == 0).any()          # boxes were recalled and detections were ignored


@pytest.mark.parametrize("nset", [1, 3])
@pytest.mark.parametrize("G", [0, 1, 2, "tile-1", "tile", "tile+1", "2*tile+3"])
def test_match_ground_truth_counts_around_the_lds_tile(G, nset):
    from tinyfaces import ops
    tile = ops.WIDER_GT_TILE
    G = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2*tile+3": 2 * tile + 3}.get(G, G)
    rng = np.random.RandomState(200 + G)
    rows, gt, keep = wider_ref.random_image(rng, 65, G, nset)
    if G > tile:                                                                   # a duplicate across the tile boundary: the lower index, in the EARLIER tile, wins
        gt[tile] = gt[tile - 1] = [1000, 1000, 20, 20]
        gt[G - 1] = gt[G - 1] if G - 1 == tile else [2000, 2000, 20, 20]
        rows[0, :4], rows[1, :4] = gt[tile], gt[G - 1]                             # ... and a best box that is the last of the last tile
    c, r = _check([(rows, gt, keep)], (G, nset))
    if G == 0:
        assert np.array_equal(c, np.tile(np.arange(1, 66), (nset, 1))) and not r.any()
    if G > tile:
        best = wider_ref.best_match(rows, gt)
        assert best[0] == tile - 1 and best[1] == (tile - 1 if G - 1 == tile else G - 1)


@pytest.mark.parametrize("S", [1, 2, 70, 258])
def test_match_segments_of_mixed_lengths_with_empty_ones(S):
    rng = np.random.RandomState(300 + S)
    lens = [int(rng.choice([0, 1, 5, 64, 70, 130])) for _ in range(S)]
    glens = [int(rng.choice([0, 1, 3, 11])) for _ in range(S)]
    if S >= 2:
        lens[0] = lens[-1] = 0                                                     # empty first and last
    if S >= 70:
        lens[S // 2] = 0; glens[S // 2 + 1] = 0; lens[S // 2 + 1] = 7             # empty in the middle; detections without boxes
        lens[255 % S] = 300; glens[255 % S] = 300                                  # more than one chunk of detections and one LDS tile of boxes
    images = [wider_ref.random_image(rng, n, g, 3) for n, g in zip(lens, glens)]
    _check(images, S)


def test_match_exact_half_iou_duplicates_ignored_boxes_and_touching_boxes():
    rows, gt, keep = wider_ref.half_iou_image()
    from tinyfaces import wider_eval as we
    # the host reference says "match" at exactly 0.5, and so must the kernel: pred_recall counts gt 0 and gt 1 in setting 0
    assert we.image_evaluation(rows, gt, keep[0])[0].tolist() == [1, 2, 3, 3, 3, 3, 3, 3]
    c, r = _check([(rows, gt, keep)], "half")
    assert r[0].tolist() == [1, 2, 3, 3, 3, 3, 3, 3]
    assert c[1].tolist() == [1, 1, 2, 3, 4, 5, 6, 7] and r[1].tolist() == [1, 1, 2, 2, 2, 2, 2, 2]     # gt 1 ignored in setting 1 only
    assert c[2].tolist() == [0, 1, 1, 1, 1, 2, 2, 3] and r[2].tolist() == [0, 1, 1, 1, 1, 1, 1, 1]     # the duplicate gt 3 is kept, but gt 2 wins every tie
    # the same image between others, and a threshold of its own
    rng = np.random.RandomState(7)
    images = [wider_ref.random_image(rng, 40, 6, 3), (rows, gt, keep), wider_ref.random_image(rng, 3, 2, 3)]
    _check(images, "half among others")
    for thr in (0.4, 0.5000000000000001, 1.0):
        got_c, got_r = _match(images, thr)
        want_c, want_r = wider_ref.host_counts_batched(images, thr)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_r, want_r), thr


# --------------------------------------------------------------------------- the PR kernel
def _pr_case(seed, T, scores_of=None):
    rng = np.random.RandomState(seed)
    images = [wider_ref.random_image(rng, n, g, 2, quantum=16) for n, g in ((0, 3), (40, 5), (1, 1), (0, 0), (300, 9), (7, 0), (64, 4), (0, 2))]
    if scores_of is not None:
        images = [(np.column_stack([r[:, :4], scores_of(r.shape[0], i)]), g, k) for i, (r, g, k) in enumerate(images)]
        images = [(r[np.argsort(-r[:, 4], kind="stable")], g, k) for r, g, k in images]
    rows, doff, gt, goff, keep = wider_ref.concat(images)
    counted, recalled = wider_ref.host_counts_batched(images)
    return rows[:, 4].copy(), doff, counted, recalled


def _pr_device(scores, doff, counted, recalled, lo, d, T, start=None):
    from tinyfaces import ops
    pr = torch.zeros(counted.shape[0], T, 2, dtype=torch.int64, device=DEV) if start is None else torch.from_numpy(start.copy()).to(DEV)
    thresh = torch.tensor([1 - (t + 1) / T for t in range(T)], dtype=torch.float64).to(DEV)
    out = ops.wider_pr_accumulate(torch.from_numpy(scores).to(DEV), doff, torch.from_numpy(counted.astype(np.int32)).to(DEV),
                                  torch.from_numpy(recalled.astype(np.int32)).to(DEV), torch.tensor([lo, d], dtype=torch.float64).to(DEV), thresh, pr)
    assert out is pr
    return pr.cpu().numpy()


@pytest.mark.parametrize("T", [1, 7, 1000])
def test_pr_table_is_the_sum_of_image_pr_info(T):
    # scores on a grid of sixteenths: ties inside and across segments
    scores, doff, counted, recalled = _pr_case(400 + T, T)
    lo, hi = float(scores.min()), float(scores.max())
    d = hi - lo if hi > lo else 1.0
    want = wider_ref.host_pr_table(scores, doff, counted, recalled, lo, d, T)
    got = _pr_device(scores, doff, counted, recalled, lo, d, T)
    assert np.array_equal(got, want) and want.any()
    # a table that arrives non-zero is added to, not overwritten
    start = np.arange(counted.shape[0] * T * 2, dtype=np.int64).reshape(-1, T, 2) * 3 + (1 << 40)
    assert np.array_equal(_pr_device(scores, doff, counted, recalled, lo, d, T, start=start), start + want)


@pytest.mark.parametrize("T", [7, 1000])
def test_pr_scores_on_a_threshold_and_all_equal(T):
    # scores that ARE thresholds after the normalisation: lo = 0 and hi = 1 are in the set, so (s - 0) / 1 == s == 1 - (t + 1) / T
    on = np.array([1 - (t + 1) / T for t in range(T)])
    pick = lambda n, i: np.concatenate([[0.0, 1.0], on[(np.arange(n) * 37 + i) % T]])[:n] if n else np.zeros(0)      # noqa: E731
    scores, doff, counted, recalled = _pr_case(500 + T, T, scores_of=pick)
    assert scores.min() == 0.0 and scores.max() == 1.0 and np.isin(scores, on).sum() > 100
    want = wider_ref.host_pr_table(scores, doff, counted, recalled, 0.0, 1.0, T)
    assert np.array_equal(_pr_device(scores, doff, counted, recalled, 0.0, 1.0, T), want)
    # all scores equal: d = 1, every normalised score is 0 and only the last threshold (1 - T / T == 0) sees them
    scores, doff, counted, recalled = _pr_case(600 + T, T, scores_of=lambda n, i: np.full(n, 0.625))
    want = wider_ref.host_pr_table(scores, doff, counted, recalled, 0.625, 1.0, T)
    got = _pr_device(scores, doff, counted, recalled, 0.625, 1.0, T)
    assert np.array_equal(got, want) and not got[:, :-1].any() and got[:, -1].all()


# --------------------------------------------------------------------------- DeviceEvaluator
def _feed(ev, preds, gtb, keeps, batch, shuffle=None):
    names = sorted(set(preds["ev"]) | set(gtb["ev"]))
    for first in range(0, len(names), batch):
        chunk = names[first:first + batch]
        rows = [preds["ev"].get(n, np.zeros((0, 5))) for n in chunk]
        if shuffle is not None:
            rows = [r[shuffle.permutation(r.shape[0])] for r in rows]
        gts = [gtb["ev"].get(n, np.zeros((0, 4))) for n in chunk]
        ev.add(rows, gts, [[k["ev"].get(n, []) for n in chunk] for k in keeps])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_device_evaluator_equals_evaluate_setting(seed):
    from tinyfaces import wider_eval as we
    preds, gtb, keeps = wider_ref.synthetic_set(seed, n_img=[40, 23, 8][seed - 1])
    settings = ("easy", "medium", "hard")
    normed = we.norm_scores(preds)
    want = {s: we.evaluate_setting(normed, gtb, keeps[k]) for k, s in enumerate(settings)}
    assert any(0.0 < ap < 1.0 for ap, _ in want.values())
    results = []
    for batch, shuffle in ((1000, None), (7, None), (7, np.random.RandomState(seed)), (1000, None)):
        ev = we.DeviceEvaluator(settings, device=DEV)
        _feed(ev, preds, gtb, keeps, batch, shuffle)
        got = ev.finish()
        for s in settings:
            assert got[s][0] == want[s][0], (s, batch, got[s][0], want[s][0])
            assert np.array_equal(got[s][1], want[s][1]), (s, batch)
        results.append(got)
    for s in settings:                                                             # two runs: the same bits
        assert results[0][s][1].tobytes() == results[3][s][1].tobytes() and results[0][s][0] == results[3][s][0]
    report(f"device_evaluator[{seed}]", **{s: want[s][0] for s in settings})
    # tensors on the device are taken as they are; nothing added: zeros
    ev = we.DeviceEvaluator(settings, thresh_num=7, device=DEV)
    assert all(ap == 0.0 and not curve.any() for ap, curve in ev.finish().values())
    ev = we.DeviceEvaluator(settings, device=DEV)
    names = sorted(gtb["ev"])
    ev.add([torch.from_numpy(preds["ev"][n]).to(DEV) for n in names], [torch.from_numpy(gtb["ev"][n]) for n in names],
           {s: [keeps[k]["ev"][n] for n in names] for k, s in enumerate(settings)})
    ev.add([preds["ev"]["stray"]], [np.zeros((0, 4))], [[[]], [[]], [[]]])
    got = ev.finish()
    assert all(got[s][0] == want[s][0] for s in settings)


# --------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("N,G,nset", [(1, 1, 1), (65, "tile+1", 3)])
def test_kernels_write_only_their_outputs(hip, N, G, nset):
    from tinyfaces import ops
    l = hip.lib()
    G = ops.WIDER_GT_TILE + 1 if G == "tile+1" else G
    rng = np.random.RandomState(900 + N)
    images = [wider_ref.random_image(rng, N, G, nset), wider_ref.random_image(rng, 0, 2, nset), wider_ref.random_image(rng, N, 0, nset)]
    rows, doff, gt, goff, keep = wider_ref.concat(images)
    n, g, S = rows.shape[0], gt.shape[0], len(doff) - 1
    rows_d, gt_d, keep_d = guarded_like(torch.from_numpy(rows), DEV), guarded_like(torch.from_numpy(gt), DEV), guarded_like(torch.from_numpy(keep), DEV)
    counted, recalled = guarded((nset, n), torch.int32, DEV), guarded((nset, n), torch.int32, DEV)
    wsb = l.tf_wider_match_workspace_bytes(n, g)
    ws = guarded_workspace(wsb, DEV)
    hd, hg = (C.c_int32 * (S + 1))(*doff), (C.c_int32 * (S + 1))(*goff)
    rc = l.tf_wider_match_f64_batched(rows_d.data_ptr(), hd, gt_d.data_ptr(), hg, S, keep_d.data_ptr(), nset, 0.5, counted.data_ptr(), recalled.data_ptr(),
                                      ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for t, what in ((counted, "counted"), (recalled, "recalled"), (ws, "workspace"), (rows_d, "rows"), (gt_d, "gt"), (keep_d, "keep")):
        assert_guards(t, what)
    assert_written(counted, what="counted"); assert_written(recalled, what="recalled")
    want_c, want_r = wider_ref.host_counts_batched(images)
    assert np.array_equal(counted.cpu().numpy(), want_c) and np.array_equal(recalled.cpu().numpy(), want_r)
    assert torch.equal(rows_d.cpu(), torch.from_numpy(rows)) and torch.equal(gt_d.cpu(), torch.from_numpy(gt)) and torch.equal(keep_d.cpu(), torch.from_numpy(keep))
    # the PR kernel: the table alone
    T = 7
    scores = guarded_like(torch.from_numpy(rows[:, 4].copy()), DEV)
    lo, hi = float(rows[:, 4].min()), float(rows[:, 4].max())
    d = hi - lo if hi > lo else 1.0
    lo_d = guarded_like(torch.tensor([lo, d], dtype=torch.float64), DEV)
    thresh = guarded_like(torch.tensor([1 - (t + 1) / T for t in range(T)], dtype=torch.float64), DEV)
    pr = guarded_like(torch.zeros(nset, T, 2, dtype=torch.int64), DEV)
    c0, r0 = counted.cpu(), recalled.cpu()
    rc = l.tf_wider_pr_accumulate(scores.data_ptr(), hd, S, counted.data_ptr(), recalled.data_ptr(), nset, lo_d.data_ptr(), thresh.data_ptr(), T, pr.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for t, what in ((pr, "pr"), (scores, "scores"), (counted, "counted"), (recalled, "recalled"), (lo_d, "lo_d"), (thresh, "thresh")):
        assert_guards(t, what)
    assert torch.equal(counted.cpu(), c0) and torch.equal(recalled.cpu(), r0)
    assert np.array_equal(pr.cpu().numpy(), wider_ref.host_pr_table(rows[:, 4], doff, want_c, want_r, lo, d, T))


# --------------------------------------------------------------------------- the command lines
def _run(args, cwd, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    return r.stdout


def _faces_ground_truth():
    from tinyfaces.datasets.synthetic import SyntheticFaces
    from tinyfaces.datasets.templates import load_templates
    gt = {"faces": SyntheticFaces(load_templates(), length=8, seed=0, train=False).ground_truth()}
    return gt, {"faces": {k: np.arange(v.shape[0]) for k, v in gt["faces"].items()}}


def test_evaluate_model_ap_equals_the_host_evaluator_on_its_result_tree(tmp_path):
    from bench import tame_init_
    from tinyfaces import wider_eval as we
    from tinyfaces.models.model import DetectionModel
    m = tame_init_(DetectionModel(num_objects=1, num_templates=25), seed=3)
    ck = tmp_path / "tame.pth"
    torch.save({"epoch": 1, "batch_size": 4, "model": m.state_dict(), "optimizer": {}}, ck)
    results = tmp_path / "res"
    # untrained scores sit at sigmoid(~0): a threshold of 0.4 passes about every anchor; the two limits keep the lists short
    out = _run([os.path.join(PKG, "evaluate_model.py"), "synthetic-faces", "--num-images", "8", "--ap", "--mask-axis", "template", "--checkpoint", str(ck),
                "--prob_thresh", "0.4", "--pre-nms-topk", "3000", "--max-detections", "60", "--results_dir", str(results)], tmp_path)
    printed = re.findall(r"^AP (\S+) = (\S+)$", out, re.M)
    assert [s for s, _ in printed] == ["all"], out[-2000:]
    gt, keep = _faces_ground_truth()
    raw = we.read_predictions(str(results))
    assert sorted(raw["faces"]) == sorted(gt["faces"])             # the result files are still written, one per image
    ndet = sum(v.shape[0] for v in raw["faces"].values())
    assert ndet > 8
    ap, _ = we.evaluate_setting(we.norm_scores(raw), gt, keep)
    report("evaluate_model_ap", printed=printed[0][1], host=repr(ap), detections=ndet)
    assert float(printed[0][1]) == ap


def test_main_val_every_prints_stores_and_does_not_disturb_training(tmp_path):
    """`main.py --val-every 1` on the configuration tests/test_gpu_e2e.py trains, two epochs: two `Val:` lines, "val_ap" in the checkpoint,
    checkpoint_best.pth, nothing for a run without the flag -- and validation does not disturb training, bit for bit.

    How "does not disturb" is checked.  Comparing the final state_dict with that of a second run without --val-every cannot decide it: this
    training configuration does not repeat itself from run to run (the weight-gradient kernels sum with fp32 atomics).  Measured on the MI355X
    with this very command line, two runs WITHOUT validation: 476 of 571 tensors differ (all the trained ones and the running statistics;
    final loss_cls 4.653 vs 4.956), the same 476 between a run with and a run without.  So the check is made where it is decidable: inside
    ONE run (tests/val_state_worker.py), everything the steps that follow depend on is digested right before and right after every validation
    pass -- parameters, momentum, accumulator, EMA, the model's whole state_dict with the BatchNorm buffers and counters, every scalar
    attribute of engine, model and criterion (modes, counters, learning rate, workspace generation, packed-weights key), the train / eval flag
    of every module, requires_grad of every parameter, the address and size of the model's workspace, the torch / numpy / random generators on
    host and device, the library's global statistic-row setting -- and must be identical, sha256 for sha256."""
    import json
    main = os.path.join(PKG, "main.py")
    common = ["synthetic-faces", "synthetic-faces", "--epochs", "2", "--synthetic-len", "3200", "--batch_size", "32", "--lr", "2e-4", "--save-every", "2",
              "--dtype", "bf16", "--ohem-thresh", "0"]
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    os.environ["VAL_STATE_OUT"] = str(tmp_path / "state.json")
    try:
        out = _run([os.path.join(ROOT, "tests", "val_state_worker.py")] + common + ["--save-path", str(tmp_path / "a" / "weights"), "--val-every", "1",
                                                                                    "--val-prob-thresh", "0.1", "--model-ema", "0.99"], tmp_path / "a")
    finally:
        del os.environ["VAL_STATE_OUT"]
    passes = json.load(open(tmp_path / "state.json"))["passes"]
    assert len(passes) == 2
    for i, p in enumerate(passes):
        assert sorted(p["before"]) == sorted(p["after"])
        moved = [k for k in p["before"] if p["before"][k] != p["after"][k]]
        assert not moved, (i, moved, [(k, p["before"][k], p["after"][k]) for k in moved if k not in ("state_dict",)][:3])
        assert len(p["before"]["state_dict"]) == 571 and p["before"]["ema"] is not None and True in p["before"]["training"]
    assert passes[0]["before"]["flat_p"] != passes[1]["before"]["flat_p"]          # ... while training itself moved them in between
    vals = re.findall(r"^Val: \[(\d+)\] AP all (\S+) \(model EMA\)$", out, re.M)
    assert [e for e, _ in vals] == ["0", "1"], out[-3000:]
    with_val = torch.load(tmp_path / "a" / "weights" / "checkpoint_2.pth", map_location="cpu")
    assert with_val["val_ap"] == {"all": float(vals[1][1])}
    best = torch.load(tmp_path / "a" / "weights" / "checkpoint_best.pth", map_location="cpu")
    aps = [float(v) for _, v in vals]
    assert best["val_ap"]["all"] == max(aps) and best["epoch"] == 1 + aps.index(max(aps)) and "model" in best and "optimizer" in best
    assert not list((tmp_path / "a").glob("*results*"))            # no result file was written
    report("main_val_every", ap_epoch0=aps[0], ap_epoch1=aps[1])
    # the live weights without --model-ema, and the default: one short epoch each on the same data
    short = ["synthetic-faces", "synthetic-faces", "--epochs", "1", "--synthetic-len", "64", "--batch_size", "32", "--lr", "2e-4", "--save-every", "1",
             "--dtype", "bf16", "--ohem-thresh", "0"]
    out = _run([main] + short + ["--save-path", str(tmp_path / "b" / "weights"), "--val-every", "1", "--val-num-images", "2"], tmp_path / "b")
    assert len(re.findall(r"^Val: \[0\] AP all (\S+)$", out, re.M)) == 1
    assert "val_ap" in torch.load(tmp_path / "b" / "weights" / "checkpoint_best.pth", map_location="cpu")
    out = _run([main] + short + ["--save-path", str(tmp_path / "b" / "plain")], tmp_path / "b")
    assert "Val:" not in out and not (tmp_path / "b" / "plain" / "checkpoint_best.pth").exists()
    assert "val_ap" not in torch.load(tmp_path / "b" / "plain" / "checkpoint_1.pth", map_location="cpu")
