"""CPU: host-side logic of the drop-in surface (no GPU compute)."""
import numpy as np
import pytest
import torch


def test_template_masks_reproduce_reference_d1(templates):
    from tinyfaces import ops
    from oracle.decode import invalid_template_ids
    for scale in (0.25, 0.5, 1, 2):
        inv = invalid_template_ids(templates, scale)
        vx, vt = ops.template_masks(templates, scale, 40, "w")
        assert sorted(np.where(vx == 0)[0].tolist()) == sorted(inv.tolist()) and vt.all()
        vx, vt = ops.template_masks(templates, scale, 40, "template")
        assert sorted(np.where(vt == 0)[0].tolist()) == sorted(inv.tolist()) and vx.all()
    with pytest.raises(IndexError):
        ops.template_masks(templates, 1, 20, "w")


def test_templates_equal_reference_values(templates):
    from tinyfaces.datasets.templates import load_templates
    assert np.array_equal(load_templates(25), templates)      # fixture = np.round(reference templates.json, 8)


def test_criterion_constants_and_meters():
    from tinyfaces.models.loss import AvgMeter, DetectionCriterion
    c = DetectionCriterion(25)
    assert (c.max_pos, c.max_neg, c.ohem_thresh) == (128, 128, 0.03)
    a = AvgMeter()
    a.update(10.0, 2); a.update(20.0, 2)
    assert a.average == 7.5 and a.num_averaged == 4                 # loss.py:13-17 semantics (sum / images)


def test_print_state_format(capsys):
    from tinyfaces.trainer import print_state
    print_state(3, 1, 10, 1.5, 2.25)
    assert capsys.readouterr().out == "Epoch: [1][3/10]\t\tloss_cls: 1.500000\tloss_reg: 2.250000\n"


def test_write_results_format(tmp_path):
    from tinyfaces.evaluation import write_results
    dets = np.array([[10.4, 20.6, 50.2, 80.9, 0.75]])
    write_results(dets, "0--Parade/img_1.jpg", "val", tmp_path)
    txt = (tmp_path / "0--Parade" / "img_1.txt").read_text().split("\n")
    assert txt[0] == "img_1.jpg" and txt[1] == "1" and txt[2] == "10 21 41 61 0.75"      # evaluation.py:106-112


def test_transforms_match_oracle_restatement():
    from oracle import refstub
    from tinyfaces import transforms
    g = torch.Generator().manual_seed(0)
    img = torch.rand(3, 37, 53, generator=g)
    a, b = transforms.to_pil_image(img), refstub.to_pil_image(img)
    assert np.array_equal(np.array(a), np.array(b))
    for s in (20, 74):
        assert np.array_equal(np.array(transforms.resize(a, s)), np.array(refstub.resize(b, s)))
    tf1 = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    tf2 = refstub.Compose([refstub.ToTensor(), refstub.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    assert torch.equal(tf1(a), tf2(b))


def test_engine_bucket_ranges_partition_the_flat_gradient():
    """TrainEngine.bucket_ranges (data-parallel overlap): the four buckets tile the flat gradient buffer exactly, follow the
    backward order (heads + late layer3 first, stem last) and every parameter lies inside exactly one bucket."""
    import torch
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.model import DetectionModel
    m = DetectionModel(num_templates=25)
    flat = m.flatten_parameters()
    seg = m._segments
    ranges = TrainEngine.bucket_ranges(seg, flat.numel())
    assert [r[0] for r in ranges] == [22, 14, 7, -1]
    assert ranges[0][2] == flat.numel() and ranges[-1][1] == 0
    for (_, s0, e0), (_, s1, e1) in zip(ranges, ranges[1:]):
        assert e1 == s0 and s1 < e1                              # contiguous, descending, non-empty
    def bucket_of(name):
        o, n = seg[name]
        hit = [k for k, (_, s, e) in enumerate(ranges) if s <= o and o + n <= e]
        assert len(hit) == 1, name
        return hit[0]
    assert bucket_of("score_res3.weight") == 0 and bucket_of("score_res4.bias") == 0 and bucket_of("score4_upsample.weight") == 0
    assert bucket_of("model.layer3.22.conv3.weight") == 0 and bucket_of("model.layer3.15.conv1.weight") == 0
    assert bucket_of("model.layer3.14.bn3.bias") == 1 and bucket_of("model.layer3.7.conv1.weight") == 1
    assert bucket_of("model.layer3.6.conv3.weight") == 2 and bucket_of("model.layer3.0.downsample.0.weight") == 2
    assert bucket_of("model.layer2.3.conv3.weight") == 3 and bucket_of("model.conv1.weight") == 3 and bucket_of("model.layer1.0.conv1.weight") == 3
    for name in seg:
        bucket_of(name)
    sizes = [(e - s) * 4 / 2**20 for _, s, e in ranges]
    assert all(20 < x < 45 for x in sizes[:3]) and sizes[3] < 10, sizes      # three ~35 MB messages + a small tail
    # the default cut of round 2 (8-12 buckets of ~10 MB in layer 3): >= bucket_mb each, contiguous, tail = layer1/2 + stem
    firsts = TrainEngine.auto_first_blocks(seg, flat.numel(), 10)
    r10 = TrainEngine.bucket_ranges(seg, flat.numel(), firsts)
    assert firsts[-1] == 7 and list(firsts) == sorted(firsts, reverse=True) and 8 <= len(firsts) <= 12
    assert r10[0][2] == flat.numel() and r10[-1][:2] == (-1, 0)
    for (_, s0, e0), (_, s1, e1) in zip(r10, r10[1:]):
        assert e1 == s0 and s1 < e1
    mb = [(e - s) * 4 / 2**20 for _, s, e in r10]
    assert all(10 <= x < 16 for x in mb[:-1]) and mb[-1] < 10, mb


def test_group_slices_of_the_buckets_tile_every_trained_parameter_once():
    """TrainEngine.group_slices (r3, per-bucket SGD): cutting every gradient bucket at the parameter-group boundaries (model.py:67-87) gives
    slices that carry the group's lr multiplier, never overlap, skip the lr-0 upsample group, and together cover exactly the three trained
    groups -- i.e. the per-bucket update touches every trained element once with the factor the at-the-end update uses."""
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.model import DetectionModel
    m = DetectionModel(num_templates=25)
    flat = m.flatten_parameters()
    groups = m.group_ranges()
    assert [g[2] for g in groups] == [1.0, 0.1, 1.0, 0.0]
    ranges = TrainEngine.bucket_ranges(m._segments, flat.numel(), TrainEngine.auto_first_blocks(m._segments, flat.numel(), 10))
    cover = np.zeros(flat.numel(), dtype=np.int8)
    mult_of = np.zeros(flat.numel(), dtype=np.float32)
    for _, start, end in ranges:
        for a, b, mult in TrainEngine.group_slices(groups, start, end):
            assert start <= a < b <= end and mult != 0.0
            cover[a:b] += 1
            mult_of[a:b] = mult
    want = np.zeros_like(cover)
    for s, e, mult in groups:
        if mult != 0.0:
            want[s:e] = 1
            assert np.all(mult_of[s:e] == np.float32(mult))
    assert np.array_equal(cover, want)
    assert TrainEngine.group_slices(groups, 0, 0) == [] and TrainEngine.group_slices([(0, 8, 0.0)], 0, 8) == []


def test_forward_levels_lane_assignment():
    """DetectionModel.assign_lanes (r3, evaluation pyramid on several HIP streams): the largest level owns lane 0 (the caller's stream and
    the model's workspace), the others go, by decreasing size, to the least loaded lane; every level gets exactly one lane; one lane or
    one level degenerate to the sequential loop."""
    from tinyfaces.models.model import DetectionModel
    f = DetectionModel.assign_lanes
    px = [480 * 640, 960 * 1280, 1920 * 2560]                       # configs[1], in pyramid order (small -> large)
    order, lane = f(px, 3)
    assert order == [2, 1, 0] and lane == {2: 0, 1: 1, 0: 2}
    order, lane = f(px, 2)
    assert lane == {2: 0, 1: 1, 0: 1}                                # both small levels beside the large one
    px4 = [120 * 160, 240 * 320, 480 * 640, 960 * 1280]              # the reference's default scales (-2, -1, 0, 1)
    order, lane = f(px4, 3)
    assert order == [3, 2, 1, 0] and lane[3] == 0 and lane[2] == 1 and lane[1] == 2 and lane[0] == 2
    assert sorted(lane) == [0, 1, 2, 3]
    assert f([5, 5, 5], 3)[0] == [0, 1, 2]                           # ties keep the list order
    assert f([7], 3) == ([0], {0: 0}) and set(f(px, 1)[1].values()) == {0}


def test_wider_annotation_parser_vs_reference_golden(golden, tmp_path):
    """tinyfaces.datasets.wider_face.parse_annotations == the reference's WIDERFace.load (wider_face.py:65-121) on an annotation
    file with an empty image (placeholder line), zero-size boxes, negative numbers and attributes."""
    from tinyfaces.datasets.wider_face import parse_annotations
    g = golden("augment")
    f = tmp_path / "ann.txt"
    f.write_text(str(g["ann_text"]))
    data = parse_annotations(f, "train")
    assert [d["img_path"] for d in data] == g["ann_paths"].tolist()
    for i, d in enumerate(data):
        assert d["bboxes"].shape == g[f"ann{i}_bboxes"].shape and np.array_equal(d["bboxes"], g[f"ann{i}_bboxes"])
        attrs = np.stack([d[k] for k in ("blur", "expression", "illumination", "invalid", "occlusion", "pose")])
        assert np.array_equal(attrs, g[f"ann{i}_attrs"])
    test = tmp_path / "test.txt"
    test.write_text("0--Parade/x.jpg\n1--H/y.jpg\n")
    assert parse_annotations(test, "test") == [{"img_path": "0--Parade/x.jpg"}, {"img_path": "1--H/y.jpg"}]


def test_wider_val_and_test_splits_yield_image_and_path(tmp_path):
    """wider_face.py:224-239: val -> (ToTensor(image), path) without normalisation; test -> (transforms(image), path).  Host only."""
    from types import SimpleNamespace
    from PIL import Image
    import torch
    from tinyfaces import transforms
    from tinyfaces.datasets import get_dataloader
    arr = (np.arange(40 * 50 * 3) % 251).astype(np.uint8).reshape(40, 50, 3)
    for split in ("val", "test"):
        d = tmp_path / f"WIDER_{split}" / "images" / "3--Riot"
        d.mkdir(parents=True)
        Image.fromarray(arr, "RGB").save(d / "p.png")
    (tmp_path / "val.txt").write_text("3--Riot/p.png\n1\n4 5 10 12 0 0 0 0 0 0\n")
    (tmp_path / "test.txt").write_text("3--Riot/p.png\n")
    tf = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    args = SimpleNamespace(batch_size=1, workers=0, dataset_root=str(tmp_path), debug=False)
    loader, templates = get_dataloader(tmp_path / "val.txt", args, img_transforms=tf, train=False, split="val")
    (img, path), = list(loader)                 # batched like torch's default collate: (1,3,H,W) + [path] (evaluate_model.py:60-68)
    assert path == ["3--Riot/p.png"] and img.shape == (1, 3, 40, 50) and img.dtype == torch.float32
    assert torch.equal(img[0], torch.from_numpy(arr.transpose(2, 0, 1).copy()).float().div(255))
    assert loader.dataset.rf == {"size": [859, 859], "stride": [8, 8], "offset": [-1, -1]}
    loader, _ = get_dataloader(tmp_path / "test.txt", args, img_transforms=tf, train=False, split="test")
    (img, path), = list(loader)
    assert path[0] == "3--Riot/p.png" and torch.allclose(img[0], tf(arr))


def _wider_case(rng, n_img=6):
    gt, keep, preds = {"ev": {}}, {"ev": {}}, {"ev": {}}
    for k in range(n_img):
        G = rng.randint(0, 6)
        xy = rng.uniform(0, 300, (G, 2)); wh = rng.uniform(10, 80, (G, 2))
        g = np.column_stack([xy, wh])
        kp = np.nonzero(rng.rand(G) > 0.3)[0]
        N = rng.randint(0, 9)
        rows = []
        for _ in range(N):
            if G and rng.rand() < 0.6:                        # a jittered copy of a ground-truth box
                b = g[rng.randint(G)] + rng.uniform(-6, 6, 4)
            else:
                b = np.concatenate([rng.uniform(0, 300, 2), rng.uniform(10, 80, 2)])
            rows.append(np.concatenate([b, [rng.rand()]]))
        p = np.array(rows).reshape(-1, 5)
        p = p[np.argsort(-p[:, 4], kind="stable")]
        gt["ev"][f"i{k}"], keep["ev"][f"i{k}"], preds["ev"][f"i{k}"] = g, kp, p
    return preds, gt, keep


def test_wider_evaluator_hand_cases_and_bruteforce():
    """tinyfaces.wider_eval (the MATLAB eval_tools protocol, parity unpinned): exact on hand-computable cases and equal to a
    brute-force per-threshold re-derivation (thresholded detection sets evaluated from scratch) on random cases."""
    from tinyfaces import wider_eval as we
    # one image, two kept faces, perfect detections -> AP 1; one missed -> AP 0.5; ignored face never hurts precision
    gt = {"e": {"a": np.array([[10, 10, 20, 20], [100, 100, 30, 30.0]])}}
    keep = {"e": {"a": np.array([0, 1])}}
    perfect = {"e": {"a": np.array([[10, 10, 20, 20, 1.0], [100, 100, 30, 30, 0.5]])}}
    assert abs(we.evaluate_setting(we.norm_scores(perfect), gt, keep)[0] - 1.0) < 1e-12
    half = {"e": {"a": np.array([[10, 10, 20, 20, 1.0], [300, 300, 30, 30, 0.5]])}}
    ap_half = we.evaluate_setting(we.norm_scores(half), gt, keep)[0]
    assert abs(ap_half - 0.5) < 1e-12
    keep_one = {"e": {"a": np.array([0])}}                   # second face ignored: its detection is dropped, not a false positive
    assert abs(we.evaluate_setting(we.norm_scores(perfect), gt, keep_one)[0] - 1.0) < 1e-12
    assert we.voc_ap(np.array([0.5, 1.0]), np.array([1.0, 0.5])) == 0.75

    def brute(preds, gt, keep, T=we.THRESH_NUM):
        pr, faces = np.zeros((T, 2)), 0
        for name, g in gt["ev"].items():
            faces += len(keep["ev"][name])
            p = preds["ev"][name]
            if g.shape[0] == 0 or p.shape[0] == 0:
                continue
            mask = np.zeros(g.shape[0], bool); mask[keep["ev"][name]] = True
            for t in range(T):
                sel = p[p[:, 4] >= 1 - (t + 1) / T]
                if sel.shape[0] == 0:
                    continue
                pred_recall, proposal = we.image_evaluation(sel, g, mask)       # greedy matching restarted on the thresholded prefix
                pr[t, 0] += int((proposal == 1).sum()); pr[t, 1] += pred_recall[-1]
        prec = np.divide(pr[:, 1], pr[:, 0], out=np.zeros(T), where=pr[:, 0] > 0)
        return we.voc_ap(pr[:, 1] / max(faces, 1), prec)

    rng = np.random.RandomState(0)
    for _ in range(5):
        preds, gt2, keep2 = _wider_case(rng)
        preds = we.norm_scores(preds)
        ap, curve = we.evaluate_setting(preds, gt2, keep2)
        assert 0.0 <= ap <= 1.0 and curve.shape == (we.THRESH_NUM, 2)
        assert np.all(np.diff(curve[:, 1]) >= -1e-12)                           # recall never decreases as the threshold drops
        assert abs(ap - brute(preds, gt2, keep2)) < 1e-12


def test_wider_evaluator_reads_write_results_tree(tmp_path):
    from tinyfaces import wider_eval as we
    from tinyfaces.evaluation import write_results
    dets = np.array([[10.0, 20.0, 29.0, 49.0, 0.25], [5.0, 5.0, 14.0, 14.0, 0.9]])       # x1 y1 x2 y2 score
    write_results(dets, "0--Parade/0_Parade_x_1.jpg", "val", results_dir=tmp_path)
    p = we.read_predictions(tmp_path)
    rows = p["0--Parade"]["0_Parade_x_1"]
    assert rows.shape == (2, 5) and rows[0, 4] == 0.9 and rows[1, 4] == 0.25          # sorted by score
    assert rows[0, :4].tolist() == [5.0, 5.0, 10.0, 10.0]                               # x y w h with the +1 of evaluation.py:108-109


def test_bench_cross_checks_launch_durations_with_the_committed_rocprof_summary():
    """roofline.rocprof_avg_launch_us: the true kernel duration of the dominant kernel in the committed rocprofv3 --stats summary of
    the bench command, next to the HIP-event average measured live; a summary without that kernel must fail loudly."""
    import importlib.util
    import os
    import tempfile
    import pytest
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    us = bench.rocprof_avg_us(13)
    assert us is not None and 5.0 < us < 200.0                   # tens of microseconds per conv launch
    assert bench.rocprof_avg_us(6) is not None and bench.rocprof_avg_us(14) is not None
    assert bench.rocprof_avg_us(5) is None
    old = bench.ROCPROF_STATS_FILE
    try:
        with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as f:
            f.write('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n"some_other_kernel()",3,300,100,100,90,110,1\n')
        bench.ROCPROF_STATS_FILE = f.name
        with pytest.raises(RuntimeError, match="regenerate"):
            bench.rocprof_avg_us(13)
    finally:
        bench.ROCPROF_STATS_FILE = old
        os.unlink(f.name)


def test_bench_reads_committed_pmc_traffic():
    """bench.py's roofline.traffic comes from the committed rocprofv3 --pmc passes: the file must parse and give a per-launch byte
    count of the dominant kernel that is of the order of its algorithmic bytes (tens of MB), never silently zero."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t = bench.pmc_traffic(13)
    assert t is not None and 2e7 < t < 3e8
    assert bench.pmc_traffic(14) is not None                     # weight-gradient rows exist too
    assert bench.pmc_traffic(5) is None                          # a kernel kind with no pattern: None, not an exception
    # the whole step (roofline_step): tens of GB, i.e. several milliseconds of HBM time at bs = 12 -- the step is nearer to that roof
    step = bench.pmc_step_traffic()
    assert step is not None and 1.5e10 < step < 6e10
    # a file whose kernel names no longer match the binary must fail loudly, not report a stale number
    import json
    import pytest
    stale = dict(json.load(open(bench.PMC_TRAFFIC_FILE)))
    stale["kernels"] = {"some_renamed_kernel<1>": next(iter(stale["kernels"].values()))}
    old = bench.PMC_TRAFFIC_FILE
    try:
        import tempfile
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump(stale, f)
        bench.PMC_TRAFFIC_FILE = f.name
        with pytest.raises(RuntimeError, match="regenerate"):
            bench.pmc_traffic(13)
    finally:
        bench.PMC_TRAFFIC_FILE = old


def test_template_clustering_vs_reference_golden(golden):
    """tinyfaces.clustering == the reference's centralize_bbox / compute_distances / local kMedoids under the same
    np.random seed (tests/golden/clustering.npz)."""
    from tinyfaces import clustering as cl
    g = golden("clustering")
    shapes = cl.centralize_bbox(g["boxes"])
    assert np.array_equal(shapes, g["shapes"])
    dist = cl.compute_distances(shapes)
    assert np.allclose(dist, g["dist"], rtol=0, atol=1e-15)
    for k in (3, 7):
        med, member = cl.k_medoids(g["dist"], k, rng=np.random.RandomState(40 + k))
        assert np.array_equal(med, g[f"k{k}_medoids"]) and np.array_equal(member, g[f"k{k}_member"])
    res = cl.compute_kmedoids(g["boxes"], 1, option="local", indices=4, max_clusters=5, rng=np.random.RandomState(0))
    assert [len(r) for r in res[:4]] == [0, 0, 0, 0] and [r["n_clusters"] for r in res[4:]] == [4, 5]
    assert all(len(r["medoids"]) == r["n_clusters"] for r in res[4:])
    import pytest
    with pytest.raises(NotImplementedError):
        cl.compute_kmedoids(g["boxes"], 1, option="pyclustering")


def test_entry_script_flags_match_the_reference(golden):
    """main.py / evaluate_model.py accept the reference's command line: same option names, same defaults (tests/golden/cli.npz holds
    what the reference's own argparse resolves).  One documented deviation: --resume takes a path (the reference declares it
    store_true but reads it as a path, main.py:33,74), so its empty default is '' instead of False."""
    import importlib.util
    import json
    import os
    g = golden("cli")
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiny-faces-pytorch_amd")

    def ours(script, argv):
        spec = importlib.util.spec_from_file_location("our_cli_" + script[:-3], os.path.join(pkg, script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return vars(mod.arguments(argv))
    ref = json.loads(str(g["main"]))
    got = ours("main.py", ["TRAIN", "VAL"])
    for k, v in ref.items():
        if k == "resume":
            assert got[k] == "" and v is False
        else:
            assert got[k] == v, k
    assert set(got) - set(ref) == {"fused", "dtype", "synthetic_len", "seed", "pretrained", "init", "save_path", "ohem_thresh"}      # r6: --init, --save-path, --ohem-thresh (default = loss.py:62)
    assert got["ohem_thresh"] == 0.03
    ref = json.loads(str(g["evaluate_model"]))
    got = ours("evaluate_model.py", ["DATA"])
    assert {k: got[k] for k in ref} == ref
    assert set(got) - set(ref) == {"num_images", "mask_axis"} and got["mask_axis"] == "w"       # r6: --mask-axis (default = the reference's behaviour, defect D1)


def test_wider_evaluator_reads_official_mat_layout_and_filters_by_setting(tmp_path):
    """tinyfaces.wider_eval.evaluate end to end on a hand-built ground truth in the layout of the WIDER `eval_tools/ground_truth`
    files (wider_face_val.mat: event_list / file_list / face_bbx_list cell arrays; wider_{easy,medium,hard}_val.mat: gt_list of
    1-BASED keep indices) and a result tree written by the product's write_results.  Two events, three images; the settings keep
    different subsets, one face is ignored in every setting, one image has no faces, one image has no result file.
    Expected APs are computed by hand below (VOC envelope over the 1000 thresholds)."""
    from scipy.io import savemat
    from tinyfaces import wider_eval as we
    from tinyfaces.evaluation import write_results

    def cell(items):
        c = np.empty((len(items), 1), dtype=object)
        for i, it in enumerate(items):
            c[i, 0] = it
        return c

    events = ["0--Parade", "1--Handshaking"]
    files = [["0_Parade_a_1", "0_Parade_b_2"], ["1_Handshaking_c_3"]]
    # x y w h
    boxes = [[np.array([[10, 10, 40, 40], [100, 20, 30, 30], [200, 200, 8, 8.0]]), np.zeros((0, 4))],
             [np.array([[50, 60, 20, 25], [150, 160, 60, 70.0]])]]
    keep = {"easy": [[[1], []], [[2]]],                         # only the big faces
            "medium": [[[1, 2], []], [[2]]],
            "hard": [[[1, 2], []], [[1, 2]]]}                   # face 3 of image a (8x8 px) is ignored everywhere
    gt_dir = tmp_path / "ground_truth"
    gt_dir.mkdir()
    savemat(gt_dir / "wider_face_val.mat", {
        "event_list": cell([np.array([e]) for e in events]),
        "file_list": cell([cell([np.array([f]) for f in fl]) for fl in files]),
        "face_bbx_list": cell([cell(bl) for bl in boxes])})
    for s, kl in keep.items():
        savemat(gt_dir / f"wider_{s}_val.mat", {"gt_list": cell([cell([np.array(k, dtype=np.float64).reshape(-1, 1) for k in ke]) for ke in kl])})

    # detections (x1, y1, x2, y2, score) as get_detections returns them; write_results converts to x y w h (evaluation.py:108-110)
    res = tmp_path / "val_results"
    dets_a = np.array([[10, 10, 49, 49, 0.9],                   # face 1 of a: IoU 1
                       [200, 200, 207, 207, 0.8],               # the ignored 8x8 face: dropped from the precision count
                       [300, 300, 340, 340, 0.7],               # false positive
                       [100, 20, 129, 49, 0.6]])                # face 2 of a
    write_results(dets_a, "0--Parade/0_Parade_a_1.jpg", "val", res)
    write_results(np.array([[5, 5, 30, 30, 0.5]]), "0--Parade/0_Parade_b_2.jpg", "val", res)      # image without faces: a false positive
    # (no result file for 1_Handshaking_c_3: both of its faces are misses)
    ap = we.evaluate(str(res), str(gt_dir))

    # by hand.  Scores are min-max normalised over the set: 0.9 -> 1, 0.8 -> .75, 0.7 -> .5, 0.6 -> .25, 0.5 -> 0.
    # hard: 4 counted faces (a1, a2, c1, c2).  Walking down the thresholds: after a1: P=1/1 R=1/4; the ignored detection adds
    # nothing; after the FP: P=1/2; after a2: P=2/3 R=2/4; after the FP of image b (score 0): P=2/4 R=2/4.
    # envelope: precision 1 up to R=.25, then max(2/3, 2/4) = 2/3 up to R=.5, 0 beyond -> AP = .25*1 + .25*(2/3)
    assert abs(ap["hard"] - (0.25 + 0.25 * 2 / 3)) < 1e-9
    # medium: faces a1, a2, c2 (3).  Same detection walk: R = 1/3 at P=1, R = 2/3 at P=2/3 -> AP = 1/3 + (1/3)(2/3)
    assert abs(ap["medium"] - (1 / 3 + (1 / 3) * (2 / 3))) < 1e-9
    # easy: faces a1, c2 (2).  a2 is now IGNORED too: its detection no longer counts.  R = 1/2 at P=1, then only false positives.
    assert abs(ap["easy"] - 0.5) < 1e-9


def test_lds_swizzle_of_the_mfma_fragment_reads_is_bank_conflict_free():
    """The XOR swizzle of the conv kernels' LDS image (csrc/conv_dma.hip, csrc/conv3x3h.hip: 128-byte rows, 16-byte slots, slot ^ h(row))
    restated on the host and checked against the ds_read_b128 service model of gfx950 (/opt/skills/guides/MI355X_MICROARCH.md, section
    LDS: four groups of 16 lanes per instruction, bank = (byte address / 4) mod 64; a group is conflict-free when its 16 lanes x 4
    dwords touch 64 distinct banks): the 16x16x32 and 32x32x16 fragment reads at every fragment base, and the tap-shifted reads of the
    halo-resident 3x3 kernel, which start at ARBITRARY rows of the 6 x 34-pixel frame."""
    def swz(row):
        return ((row >> 1) & 1) ^ (((row >> 2) & 1) << 2) ^ (((row >> 3) & 1) * 6)

    def off(row, slot):
        return row * 128 + ((slot ^ swz(row)) << 4)

    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    groups += [[l + 32 for l in g] for g in groups]
    assert sorted(sum(groups, [])) == list(range(64))

    def conflict_free(addr_of_lane):
        for g in groups:
            banks = [((addr_of_lane(l) >> 2) + j) % 64 for l in g for j in range(4)]
            if len(set(banks)) != 64:
                return False
        return True

    # 16x16x32 fragments (MmaD<bf16>::stage): lane l -> row base + (l & 15), slot ks*4 + (l >> 4)
    for base in range(0, 128, 16):
        for ks in range(2):
            assert conflict_free(lambda l: off(base + (l & 15), ks * 4 + (l >> 4))), (16, base, ks)
    # 32x32x16 fragments (stage32 / conv3x3h weights): lane l -> row base + (l & 31), slot ks*2 + (l >> 5)
    for base in range(0, 128, 32):
        for ks in range(4):
            assert conflict_free(lambda l: off(base + (l & 31), ks * 2 + (l >> 5))), (32, base, ks)
    # conv3x3h input fragments: 32 consecutive frame rows starting anywhere (output row + tap shift), both K halves
    FW, FR = 34, 6 * 34
    for tr in range(4):
        for tap in range(9):
            for sign in (1, -1):
                base = (tr + 1) * FW + 1 + sign * ((tap // 3 - 1) * FW + (tap % 3 - 1))
                assert 0 <= base and base + 31 < FR
                for slot0 in range(0, 8, 2):
                    assert conflict_free(lambda l: off(base + (l & 31), slot0 + (l >> 5))), (tr, tap, sign, slot0)
    # the swizzle is applied on the SOURCE side of the LDS-DMA: lane (row r, physical slot p) fetches logical slot p ^ h(r) -- a bijection per row
    for r in range(256):
        assert sorted(p ^ swz(r) for p in range(8)) == list(range(8))


def test_conv3x3h_operand_pipeline_protocol():
    """The counted-vmcnt protocol of csrc/conv3x3h.hip restated as a queue model: a wave's LDS-DMA instructions retire in issue order,
    `s_waitcnt vmcnt(N)` returns when at most N are outstanding.  For every chunk count: at stage st (= chunk * 9 + tap) the wait of
    the kernel guarantees that weight stage st and the input frame of its chunk have landed, and no DMA is issued into a ring slot /
    frame buffer whose previous content is still to be read."""
    WPASS, XPASS = 2, 4
    for cpt in range(1, 7):
        nst = 9 * cpt
        q = []                                                    # issue order: (kind, index) per DMA instruction
        issue = lambda kind, idx, n: q.extend([(kind, idx)] * n)
        issue("X", 0, XPASS); issue("W", 0, WPASS); issue("W", 1, WPASS)
        w_slot = {0: 0, 1: 1}                                     # ring slot -> weight stage it holds (or will hold)
        x_buf = {0: 0}                                            # frame buffer -> chunk
        for st in range(nst):
            chunk, tap = divmod(st, 9)
            more = chunk + 1 < cpt
            if tap == 8:
                n = WPASS if more else 0
            elif tap == 1:
                n = WPASS + XPASS if more else WPASS
            else:
                n = WPASS
            landed = set(q[:len(q) - n]) if n else set(q)
            assert ("W", st) in landed and ("X", chunk) in landed, (cpt, st)
            assert w_slot[st % 3] == st and x_buf[chunk & 1] == chunk     # what the stage reads is what its buffers hold
            # after the barrier of stage st every wave has finished reading stage st-1: the slots of stages <= st-1 are free
            if tap == 0 and more:
                assert x_buf.get((chunk + 1) & 1, -1) < chunk             # the other frame buffer held chunk-1 (or nothing)
                x_buf[(chunk + 1) & 1] = chunk + 1
                issue("X", chunk + 1, XPASS)
            if tap < 7 or more:
                assert w_slot.get((st + 2) % 3, -1) <= st - 1             # slot of stage st+2 == slot of stage st-1
                w_slot[(st + 2) % 3] = st + 2
                issue("W", st + 2, WPASS)
        assert {i for k, i in q if k == "W"} == set(range(nst)) and {i for k, i in q if k == "X"} == set(range(cpt))


def test_wgrad3x3_running_offsets_and_raster_walk():
    """Two pieces of host-checkable arithmetic of csrc/wgrad3x3.hip (v3): (1) the 18 fragment offsets of a lane into the 512-row circular
    X image advance by (o + 8192) & 0xFFFF per 64-pixel stage and must equal the offset re-derived from scratch (row * 128 + swizzled
    slot), because the swizzle term only depends on row bits 1-2; (2) the branch-free +64 step of the padded-raster walk
    (PadPos::advance: q64 rows + r64 columns with carries by select) equals stepping one padded pixel 64 times."""
    import numpy as np
    fsw = lambda row: ((row >> 1) & 3) << 1
    rng = np.random.RandomState(3)
    for _ in range(200):
        Wp, hb = int(rng.randint(3, 128)), int(rng.randint(1, 3))
        lane = int(rng.randint(64)); li, lg = lane & 15, lane >> 4
        frow, fhalf, fs = lg * 4 + (li >> 2), (li & 1) << 3, (li & 3) >> 1
        slot0 = int(rng.randint(4)) * 2
        for t in range(9):
            for k in range(2):
                shift = (t // 3 - 1) * Wp + (t % 3 - 1)
                derive = lambda st: (lambda row: row * 128 + (((slot0 + fs) ^ fsw(row)) << 4) + fhalf)((64 * (st + hb) + k * 32 + shift + frow) & 511)
                o = derive(0)
                for st in range(1, 20):
                    o = (o + 8192) & 0xFFFF
                    assert o == derive(st), (Wp, hb, lane, t, k, st)
                    assert ((o + 2048) & 0xFFFF) == (lambda row: row * 128 + (((slot0 + fs) ^ fsw(row)) << 4) + fhalf)(
                        ((64 * (st + hb) + k * 32 + shift + frow) + 16) & 511)
    for _ in range(300):
        H, W, N = int(rng.randint(1, 130)), int(rng.randint(1, 130)), int(rng.randint(1, 4))
        Hp, Wp = H + 2, W + 2
        q64, r64, small = 64 // Wp, 64 % Wp, Hp <= 64 // Wp + 1
        p = int(rng.randint(0, N * Hp * Wp))
        n, rem = divmod(p, Hp * Wp); hp, wp = divmod(rem, Wp)
        for _ in range(5):
            wp += r64
            c = 1 if wp >= Wp else 0
            wp -= c * Wp; hp += q64 + c
            if small:
                while hp >= Hp:
                    hp -= Hp; n += 1
            else:
                c2 = 1 if hp >= Hp else 0
                hp -= c2 * Hp; n += c2
            p += 64
            n_ref, rem = divmod(p, Hp * Wp); hp_ref, wp_ref = divmod(rem, Wp)
            assert (n, hp, wp) == (n_ref, hp_ref, wp_ref), (H, W, p)


def test_nms_batched_splits_calls_under_a_mask_budget(monkeypatch):
    """ops.nms_batched groups consecutive segments so that the suppression bit matrices of one tf_nms_f64_batched call stay under a byte
    budget (a 64-image batch at prob_thresh 0.03 would otherwise ask for tens of GB); indices stay those of the caller's
    concatenated list.  Host logic only: the device call is replaced by a recorder."""
    import torch
    from tinyfaces import ops
    calls = []

    def fake(boxes, scores, offs, thr):
        calls.append((boxes.shape[0], list(offs)))
        return [torch.arange(a, b) for a, b in zip(offs, offs[1:])]
    monkeypatch.setattr(ops, "_nms_batched_call", fake)
    b, s = torch.zeros(1000, 4), torch.zeros(1000)
    offs = [0, 100, 400, 400, 1000]
    out = ops.nms_batched(b, s, offs, 0.3, mask_budget_bytes=ops._mask_bytes(300) + ops._mask_bytes(100))
    assert calls == [(400, [0, 100, 400, 400]), (600, [0, 600])]
    assert [(int(k[0]) if len(k) else None, len(k)) for k in out] == [(0, 100), (100, 300), (None, 0), (400, 600)]
    calls.clear()
    ops.nms_batched(b, s, offs, 0.3)                              # default budget: one call
    assert calls == [(1000, offs)]
    calls.clear()
    ops.nms_batched(b, s, offs, 0.3, mask_budget_bytes=1)         # every segment over the budget: one call each, never an empty group
    assert [c[0] for c in calls] == [100, 300, 0, 600]



def test_reference_helper_names_of_models_utils():
    """tinyfaces/models/utils.py:79-163 under their own names (VERDICT r3 missing 4): shuffle_index / balance_sampling consume np.random like
    the reference (same labels as the oracle's restatement under one seed), regression_refinement returns the reference's (1, N, 4) array."""
    import numpy as np
    from oracle import criterion as ocrit
    from tinyfaces.models import utils
    rng = np.random.RandomState(3)
    lab = rng.choice([-1, 0, 1], size=(25, 9, 11), p=[0.5, 0.2, 0.3]).astype(np.float32)
    np.random.seed(11)
    want = ocrit.balance_sampling(lab.copy(), 0.5, 256)
    np.random.seed(11)
    got = utils.balance_sampling(lab.copy(), 0.5, 256)
    assert np.array_equal(got, want) and int((got == 1).sum()) == 128 and int((got == -1).sum()) == 128
    # a NON-contiguous label array: edited in place through index assignment like the reference, same survivors
    nc = np.ascontiguousarray(lab.transpose(2, 0, 1)).transpose(1, 2, 0)
    assert not nc.flags.c_contiguous and np.array_equal(nc, lab)
    np.random.seed(11)
    back = utils.balance_sampling(nc, 0.5, 256)
    assert back is nc and np.array_equal(nc, want)
    np.random.seed(11)
    pk, nk = utils.balance_sampling_keep(lab, 0.5, 256)
    flat = lab.reshape(-1).copy()
    flat[np.flatnonzero(flat == 1)[pk == 0]] = 0
    flat[np.flatnonzero(flat == -1)[nk == 0]] = 0
    assert np.array_equal(flat.reshape(lab.shape), want)
    np.random.seed(5); a = utils.shuffle_index(10, 4)
    np.random.seed(5); b = np.random.permutation(10)[:4]
    assert np.array_equal(a, b) and utils.shuffle_index(0, 3).size == 0 and utils.shuffle_index(7, 0).size == 0
    # regression_refinement against the formula of utils.py:79-100, N = 3 candidates
    t = rng.randn(4, 1, 5, 6, 25).astype(np.float32)
    idx = (np.zeros(3, int), np.array([0, 2, 4]), np.array([1, 3, 5]), np.array([0, 7, 24]))
    cx, cy, cw, ch = rng.rand(3) * 50, rng.rand(3) * 50, rng.rand(3) * 20 + 5, rng.rand(3) * 20 + 5
    out = utils.regression_refinement(t[0], t[1], t[2], t[3], cx, cy, cw, ch, idx)
    assert out.shape == (1, 3, 4)
    rcx, rcw = cx + cw * t[0][idx], cw * np.exp(t[2][idx])
    assert np.array_equal(out[0, :, 0], rcx - rcw / 2) and np.array_equal(out[0, :, 2], rcx + rcw / 2)


def test_wider_parser_names_the_malformed_record(tmp_path):
    """a record line with a missing field must fail AT that line (the reference assigns per line), not shift boxes between images."""
    import pytest
    from tinyfaces.datasets.wider_face import parse_annotations
    good = "a/1.jpg\n2\n1 2 30 40 0 0 0 0 0 0\n5 6 70 80 0 0 0 0 0 0\nb/2.jpg\n1\n9 9 10 10 0 0 0 0 0 0\n"
    f = tmp_path / "ok.txt"; f.write_text(good)
    assert [d["bboxes"].shape[0] for d in parse_annotations(str(f), "train")] == [2, 1]
    bad = good.replace("5 6 70 80 0 0 0 0 0 0", "5 6 70 80 0 0 0 0 0")          # nine fields
    f = tmp_path / "bad.txt"; f.write_text(bad)
    with pytest.raises(ValueError, match="record 1 of 'a/1.jpg'"):
        parse_annotations(str(f), "train")


def test_frozen_parameter_tables_skip_the_walk_until_the_module_moves():
    """DetectionModel._sync_tables (r4): an owner that pins the storages (TrainEngine after flatten_parameters) freezes the pointer tables, so a
    step does not walk the 571 tensors; anything that can move a storage (`_apply`: .to() / .float() / .cuda(), or flatten_parameters itself)
    unfreezes and rebuilds them."""
    import torch
    from tinyfaces.models.model import DetectionModel
    m = DetectionModel(num_templates=25)
    dev = torch.device("cpu")
    m._sync_tables(dev)                                   # builds the tables (host-side only: pointers and shapes)
    key = m._table_key
    assert key is not None and len(m._names) == 475
    walks = []
    orig = m._named_tensors
    m._named_tensors = lambda: (walks.append(1), orig())[1]
    m._sync_tables(dev)
    assert len(walks) == 1 and m._table_key == key        # not frozen: the identity walk runs (and finds nothing changed)
    m._tables_frozen = True
    m._sync_tables(dev); m._sync_tables(dev)
    assert len(walks) == 1                                # frozen: no walk
    m.float()                                             # nn.Module._apply: storages may move
    assert m._tables_frozen is False and m._table_key is None
    m._sync_tables(dev)
    assert len(walks) == 2 and m._table_key is not None
    m._tables_frozen = True
    flat = m.flatten_parameters()                         # re-points every parameter: must rebuild even when frozen
    assert len(walks) >= 3 and m._table_key != key and flat.numel() > 27_000_000
    # a frozen table notices ANY replaced tensor, not only the first / middle / last one
    import pickle
    m._tables_frozen = True
    m._sync_tables(dev); n0 = len(walks)
    m._sync_tables(dev)
    assert len(walks) == n0                               # frozen again: no walk
    bn = m.model.layer2[1].bn2
    bn.running_var = torch.ones_like(bn.running_var)      # a buffer somewhere in the middle, replaced through Module.__setattr__
    m._sync_tables(dev)
    assert len(walks) == n0 + 1
    conv = m.model.layer3[7].conv2
    conv.weight = torch.nn.Parameter(conv.weight.detach().clone())       # a Parameter object replaced
    m._sync_tables(dev)
    assert len(walks) == n0 + 2
    m.model.layer1[2].bn3.bias.data = torch.zeros(256)    # .data re-pointed: same object, new storage
    m._sync_tables(dev)
    assert len(walks) == n0 + 3
    m._sync_tables(dev)
    assert len(walks) == n0 + 3
    # no lambdas, no ctypes tables in the pickled state: a copy rebuilds its own.  (A fresh, un-flattened model: plain pickle writes the whole
    # storage of every view, i.e. the 108 MB flat buffer once per parameter.)
    f = DetectionModel(num_templates=25)
    f._sync_tables(dev)
    f._tables_frozen = True
    f2 = pickle.loads(pickle.dumps(f))
    assert f2._table_key is None and not f2._tables_frozen
    f2._sync_tables(dev)
    assert f2._table_key is not None and f2._table_key != f._table_key


def test_stem_wgrad_patch_copies_address_the_right_input_pixels():
    """csrc/stem_conv.hip (r4), the operand layout of the direct conv1 weight gradient, restated in numpy: the input patch of a 4 x 32-pixel tile
    is staged split by column parity q and in four copies shifted by s elements, copy(s, q)[row][i] = patch[row][2 (i + s) + q]; a lane that owns
    k = (c, kh, kw) reads, for tile row ph and pixel quad pw0 (a multiple of 4), the four CONSECUTIVE elements i = pw0 .. pw0 + 3 of row
    (c, 2 ph + kh) of copy (kw >> 1, kw & 1) -- and must get the input pixels (2 ph + kh, 2 pw + kw) of output pixels pw = pw0 .. pw0 + 3,
    i.e. what im2col column k holds for them.  Also: every element a fragment can touch is written by the staging (12-column segments)."""
    TH, TW, PR, PCOLS, PC, SEG = 4, 32, 13, 69, 72, 12
    rng = np.random.RandomState(0)
    patch = np.zeros((3 * PR, PC), np.float64)
    patch[:, :PCOLS] = rng.rand(3 * PR, PCOLS) + 1.0          # > 0: an unwritten copy element (0) is detectable
    copies = np.zeros((4, 2, 3 * PR, TW), np.float64)
    written = np.zeros_like(copies, dtype=bool)
    for prow in range(3 * PR):                                # the kernel's staging: thread -> (row, 12-column segment)
        for pseg in range(PC // SEG):
            for qq in range(SEG):
                par, h = qq & 1, pseg * (SEG // 2) + (qq >> 1)
                for sft in range(4):
                    i = h - sft
                    if 0 <= i < TW:
                        copies[sft, par, prow, i] = patch[prow, pseg * SEG + qq]
                        written[sft, par, prow, i] = True
    assert written.all()
    for k in range(147):
        c, kh, kw = k // 49, (k % 49) // 7, k % 7
        for ph in range(TH):
            row = c * PR + 2 * ph + kh
            for pw0 in range(0, TW, 4):
                got = copies[kw >> 1, kw & 1, row, pw0:pw0 + 4]
                want = patch[row, [2 * pw + kw for pw in range(pw0, pw0 + 4)]]
                assert np.array_equal(got, want), (k, ph, pw0)
    # the forward kernel's gather table: offset of k inside the (c, row, column) patch raster, output pixel (ph, pw) at base 2 ph PC + 2 pw
    flat = patch.reshape(-1)
    for k in (0, 6, 7, 48, 49, 100, 146):
        c, kh, kw = k // 49, (k % 49) // 7, k % 7
        off = (c * PR + kh) * PC + kw
        for ph, pw in ((0, 0), (3, 31), (2, 17)):
            assert flat[off + 2 * ph * PC + 2 * pw] == patch[c * PR + 2 * ph + kh, 2 * pw + kw]
    assert 2 * (TH - 1) * PC + 2 * (TW - 1) < 512             # ZPAD: the zero region behind the patch covers every pixel base offset


def test_bench_roofline_bound_is_decided_per_kernel_and_gpus_n_self_launches(monkeypatch, capsys):
    """VERDICT r4 items 2 + 6: (a) `roofline.bound` is argmax(flops / MFMA peak, bytes / 8 TB/s) of the launch's ALGORITHMIC work and the
    fields are stated against that roof -- the r4 dominant kernel (7.121 GFLOP, 70.5 MB, 30.6 us) is HBM-bound at 0.29, not MFMA-bound at
    0.093; (b) `python bench.py --gpus N` outside a launcher re-executes itself through torch.distributed.run on 127.0.0.1 with the same
    arguments, and says why when no GPU is visible."""
    import importlib.util, os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    r = bench.roof_of(7.121e9, 70.5e6, 30.6e-6, 2500.0)
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - 0.288) < 2e-3 and abs(r["frac_mfma"] - 0.0931) < 1e-3 and r["frac"] == r["frac_hbm"]
    assert abs(r["achieved"] - 2303.9) < 1.0
    r = bench.roof_of(2 * 12288 * 256 * 2304.0, (12288 * 256 * 2 + 256 * 2304) * 2.0, 25e-6, 2500.0)      # a layer-3 3x3 conv: 1060 FLOP/B
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["frac"] == r["frac_mfma"] > r["frac_hbm"]
    # (b) the launcher
    import subprocess
    import torch
    seen = {}

    class R:
        returncode = 0
    monkeypatch.setattr(subprocess, "run", lambda cmd, env=None, **kw: (seen.update(cmd=cmd, env=env), R())[1])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "2"])
    assert bench.self_launch(4) == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    assert cmd[-6:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"] and os.path.basename(cmd[-7]) == "bench.py"
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)          # fewer devices than ranks: refused with a reason, nothing launched
    seen.clear()
    assert bench.self_launch(4) == 3 and not seen and "only 1 GPU" in capsys.readouterr().err


def test_bench_flags_profiles_taken_with_another_library_as_stale():
    """r6: the committed PMC traffic file and the rocprof summary carry the identity of the library they were measured on
    (scripts/pmc_traffic.py / scripts/stamp_profiles.py: tf_version, source digest, sha256 of the .so); bench.py reports them stale when the
    loaded library's source digest differs or the stamp is missing."""
    import importlib.util
    import json
    import os
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    ident = {"tf_version": 600, "build_id": "0123456789abcdef", "so_sha256": "f" * 64}
    with tempfile.TemporaryDirectory() as d:
        traffic, stamp = os.path.join(d, "t.json"), os.path.join(d, "s.json")
        json.dump({"kernels": {}, "library": ident}, open(traffic, "w"))
        json.dump(ident, open(stamp, "w"))
        r = bench.profile_staleness(ident, traffic, stamp)
        assert r["traffic_stale"] is False and r["rocprof_stale"] is False and r["library"]["build_id"] == ident["build_id"]
        other = dict(ident, build_id="fedcba9876543210")
        r = bench.profile_staleness(other, traffic, stamp)
        assert r["traffic_stale"] is True and r["rocprof_stale"] is True
        json.dump({"kernels": {}}, open(traffic, "w"))                 # an unstamped file (rounds 1-5) is stale by definition
        assert bench.profile_staleness(ident, traffic, stamp)["traffic_stale"] is True
        assert bench.profile_staleness(ident, traffic, os.path.join(d, "missing.json"))["rocprof_stale"] is True


def test_library_build_id_is_the_digest_of_its_sources():
    """tf_build_id() = build.py's sha256 over csrc/*, the public header and the compiler flags: the stamp of every committed profile."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("tf_build", os.path.join(root, "tiny-faces-pytorch_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    from tinyfaces import _hip
    ident = _hip.identity()
    assert ident["build_id"] == build.source_digest() and len(ident["build_id"]) == 16
    assert ident["tf_version"] >= 600 and len(ident["so_sha256"]) == 64


def test_library_reads_its_environment_in_one_place():
    """r6: every run-time knob of the kernel library is a field of tf::Tuning (csrc/tuning.h), parsed from the environment once
    in csrc/tuning.hip; no other translation unit calls getenv().  The struct holds exactly the knobs named here (what qualifies: the header of
    tuning.h); each is assigned once from the variable its comment names, tuning.hip names no other variable, and every field has a reader."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiny-faces-pytorch_amd", "csrc")
    code = {f: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read()) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    offenders = [f for f in code if f != "tuning.hip" and re.search(r"\bgetenv\s*\(", code[f])]
    assert not offenders, offenders
    header = open(os.path.join(csrc, "tuning.h")).read()
    fields = dict(re.findall(r"^\s+(?:bool|int|long) (\w+) = [^;]+;\s+// (\w+)\b", header, re.M))
    assert len(fields) == len(re.findall(r"^\s+(?:bool|int|long) \w+ = ", header, re.M))          # every field names its variable
    assert set(fields) == {
        "ew_blocks", "ew_blocks_small", "ew_small_mb", "wgrad_blocks", "wgrad3_blocks", "stem_wgrad_blocks", "pool_stats_blocks",     # block counts, size thresholds
        "comm_fail_init", "comm_fail_bucket", "dbg_group_refuse", "dbg_skip_wgrad", "grad_memset_full",                                # tests, fault injections
        "single_stream", "profile_bracket",                                                                                           # measurement switches
        "conv_dbg", "conv3h_dbg", "wgrad3_dbg"}                                                                                       # ablation masks (kernel arguments)
    parsed = code["tuning.hip"]
    assigned = re.findall(r'\bt\.(\w+) = [^;"]*"(\w+)"[^;]*;', parsed)                             # (field, variable) of every parse line
    assert sorted(assigned) == sorted(fields.items()) and len(re.findall(r"\bt\.\w+ = ", parsed)) == len(fields)       # once each, nothing else
    assert set(re.findall(r"\b(?:TINYFACES|TF)_[A-Z0-9_]+\b", parsed)) == set(fields.values())      # (the stderr messages included)
    others = "".join(src for name, src in code.items() if name not in ("tuning.h", "tuning.hip"))
    unread = [f for f in fields if not re.search(r"\btuning\(\)\.%s\b" % f, others)]
    assert not unread, unread


def test_synthetic_faces_dataset_is_fixed_and_consistent():
    """tinyfaces/datasets/synthetic.py: SyntheticFaces (r6, the data set of the learn-and-detect test): the image list is a function of the seed alone,
    the validation view is the training image at twice the size with boxes scaled alike, and no two faces of an image overlap."""
    import numpy as np
    import torch
    from tinyfaces.datasets.synthetic import SyntheticFaces
    from tinyfaces.datasets.templates import load_templates
    t = load_templates()
    a, b = SyntheticFaces(t, length=800, seed=0, train=False), SyntheticFaces(t, length=8, seed=0, train=False)
    assert len(a) == 800 and len(a.samples) == 8 and len(b.samples) == 8
    x0, name0 = a[0]
    x8, name8 = a[8]                                             # sample i = image i % 8
    z = SyntheticFaces.VAL_ZOOM
    assert name0 == name8 == "faces/img_0.jpg" and bool((x0 == x8).all()) and tuple(x0.shape) == (3, 500 * z, 500 * z)
    assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a.samples, b.samples))
    gt = b.ground_truth()
    # the training view: the SAME faces on a background of its own per sample, at zoom x1 / x0.5 / x2 (boxes follow the zoom)
    tr = SyntheticFaces(t, length=800, seed=0, train=True)
    views = [tr[8 * k] for k in range(4)]                       # the four views of layout 0: the evaluation image, x0.5, x2, x0.25
    assert bool((views[0][0] == torch.from_numpy(np.stack([SyntheticFaces._LUTN[c][b.samples[0][0][:, :, c]] for c in range(3)]))).all())
    assert all(tuple(v[0].shape) == (3, 500, 500) for v in views)
    sizes = sorted({round(float(v[1][0, 2] - v[1][0, 0]) / float(b.samples[0][1][0, 2] - b.samples[0][1][0, 0]), 1) for v in views if v[1].shape[0] == b.samples[0][1].shape[0]})
    assert set(sizes) <= {0.2, 0.3, 0.5, 1.0, 2.0} and len(sizes) >= 2, sizes
    assert not bool((views[0][0] == views[1][0]).all())
    for i, (u8, boxes) in enumerate(b.samples):
        assert u8.shape == (500, 500, 3) and u8.dtype == np.uint8 and 1 <= boxes.shape[0] <= 5
        g = gt[f"img_{i}"]
        assert np.allclose(g[:, :2], z * boxes[:, :2]) and np.allclose(g[:, 2], z * (boxes[:, 2] - boxes[:, 0]) + 1)
        for p in range(boxes.shape[0]):
            for q in range(p):
                iw = min(boxes[p, 2], boxes[q, 2]) - max(boxes[p, 0], boxes[q, 0])
                ih = min(boxes[p, 3], boxes[q, 3]) - max(boxes[p, 1], boxes[q, 1])
                assert iw < 0 or ih < 0
        # the validation view is pixel replication (x VAL_ZOOM) of the stored pixels
        v = (a[i][0] * 255).round().byte().permute(1, 2, 0).numpy()
        assert np.array_equal(v[::z, ::z], u8) and np.array_equal(v[z - 1::z, z - 1::z], u8)
