"""ResNet-50 / ResNet-152 trunks of DetectionModel(base_model=...) on the host side: parameter tables of the executor, trunk detection,
checkpoints and the gradient buckets of the fused engine.  The GPU side is tests/test_gpu_trunks.py."""
import ctypes as C

import pytest
import torch
from torch import nn

from oracle.model import OracleDetectionModel
from oracle.resnet import ResNet

BLOCKS = {"resnet50": (3, 4, 6), "resnet101": (3, 4, 23), "resnet152": (3, 8, 36)}


def oracle_model(blocks, num_templates=25):
    """The CPU oracle with another depth: torchvision's ResNet of these block counts (layer4 deleted) in place of resnet101."""
    om = OracleDetectionModel(num_templates=num_templates)
    om.model = ResNet(tuple(blocks) + (3,))
    del om.model.layer4
    return om


def _arg(blocks):
    return None if blocks is None else (C.c_int * 3)(*blocks)


def _table(l, blocks, nout=125):
    tr = _arg(blocks)
    n = l.tf_detnet_trunk_num_params(tr)
    return [(l.tf_detnet_trunk_param_name(tr, i).decode(), l.tf_detnet_trunk_param_numel(tr, i, nout)) for i in range(n)]


@pytest.mark.parametrize("name,entries", [("resnet50", 265), ("resnet101", 571), ("resnet152", 877)])
def test_state_dict_matches_the_oracle_of_that_depth(name, entries):
    from tinyfaces.models import model as mm
    m = mm.DetectionModel(base_model=getattr(mm, name), num_templates=25)
    om = oracle_model(BLOCKS[name])
    sd, osd = m.state_dict(), om.state_dict()
    assert m.trunk == BLOCKS[name] and m.trunk_name == name
    assert list(sd) == list(osd) and len(sd) == entries
    assert all(sd[k].shape == osd[k].shape for k in sd)
    m.load_state_dict(osd)                                  # the oracle's weights load into the model (and back: same keys, same shapes)
    assert torch.equal(m.model.layer3[-1].conv3.weight, om.model.layer3[-1].conv3.weight)


@pytest.mark.parametrize("name,entries", [("resnet50", 220), ("resnet152", 730)])
def test_executor_trunk_table_covers_the_state_dict(hip, name, entries):
    """Every tensor of the trunk is in the executor's table with its numel, and nothing else of the state_dict is left out but the dead
    `model.fc.*` and the BatchNorm counters: no layer is silently skipped (ResNet-152 ran as ResNet-101 before)."""
    from tinyfaces.models import model as mm
    m = mm.DetectionModel(base_model=getattr(mm, name), num_templates=25)
    sd = m.state_dict()
    table = _table(hip.lib(), m.trunk)
    names = [k for k, _ in table]
    assert len(table) == len(set(names)) == entries
    for k, numel in table:
        assert k in sd and sd[k].numel() == numel, k
    rest = [k for k in sd if k not in set(names)]
    assert all(k.startswith("model.fc.") or k.endswith("num_batches_tracked") for k in rest)
    last = f"model.layer3.{BLOCKS[name][2] - 1}.bn3.running_var"
    assert last in names and f"model.layer3.{BLOCKS[name][2]}.conv1.weight" not in sd


def test_resnet101_table_is_unchanged_through_both_entry_points(hip):
    l = hip.lib()
    legacy = [(l.tf_detnet_param_name(i).decode(), l.tf_detnet_param_numel(i, 125)) for i in range(l.tf_detnet_num_params())]
    assert len(legacy) == 475
    assert _table(l, (3, 4, 23)) == legacy and _table(l, None) == legacy
    for dtype in (hip.TF_BF16, hip.TF_F32):
        for training in (0, 1):
            assert l.tf_detnet_trunk_workspace_bytes(_arg((3, 4, 23)), dtype, 12, 500, 500, 125, training) == \
                l.tf_detnet_workspace_bytes(dtype, 12, 500, 500, 125, training)
        assert l.tf_detnet_trunk_param_region_bytes(_arg((3, 4, 23)), dtype, 125, 0) == l.tf_detnet_param_region_bytes(dtype, 125, 0)
    assert l.tf_version() >= 610


def test_workspace_grows_with_depth_and_other_block_counts_are_refused(hip):
    l = hip.lib()
    ws = [l.tf_detnet_trunk_workspace_bytes(_arg(b), hip.TF_BF16, 12, 500, 500, 125, 1) for b in BLOCKS.values()]
    assert 0 < ws[0] < ws[1] < ws[2]
    pr = [l.tf_detnet_trunk_param_region_bytes(_arg(b), hip.TF_BF16, 125, 0) for b in BLOCKS.values()]
    assert 0 < pr[0] < pr[1] < pr[2]
    for bad in ((3, 4, 5), (2, 2, 2), (3, 4, 36), (0, 0, 0)):
        tr = _arg(bad)
        assert l.tf_detnet_trunk_num_params(tr) == -3                 # TF_ERR_UNSUPPORTED
        assert l.tf_detnet_trunk_param_name(tr, 0) is None
        assert l.tf_detnet_trunk_param_numel(tr, 0, 125) == -3
        assert l.tf_detnet_trunk_workspace_bytes(tr, hip.TF_BF16, 2, 64, 64, 125, 1) == 0
        assert l.tf_detnet_trunk_param_region_bytes(tr, hip.TF_BF16, 125, 0) == 0


class _BasicBlock(nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None


class _Resnet18Like(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.layer1 = nn.Sequential(_BasicBlock(64, 64, 1), _BasicBlock(64, 64, 1))
        self.layer2 = nn.Sequential(_BasicBlock(64, 128, 2), _BasicBlock(128, 128, 1))
        self.layer3 = nn.Sequential(_BasicBlock(128, 256, 2), _BasicBlock(256, 256, 1))
        self.layer4 = nn.Sequential(_BasicBlock(256, 512, 2))


def _resnext_like(weights=None):
    from tinyfaces.models.model import resnet50
    t = resnet50()
    for layer in (t.layer1, t.layer2, t.layer3):
        for b in layer:
            c = b.conv2
            b.conv2 = nn.Conv2d(c.in_channels, c.out_channels, 3, stride=c.stride, padding=1, groups=32, bias=False)
    return t


def _wide_like(weights=None):
    from tinyfaces.models.model import resnet50
    t = resnet50()
    b = t.layer1[1]
    b.conv1 = nn.Conv2d(256, 128, 1, bias=False)
    b.conv2 = nn.Conv2d(128, 128, 3, padding=1, bias=False)
    b.conv3 = nn.Conv2d(128, 256, 1, bias=False)
    return t


def _depth_34_like(weights=None):
    from tinyfaces.models.model import _BottleneckTrunk
    return _BottleneckTrunk((3, 4, 5))


@pytest.mark.parametrize("base", [lambda weights=None: _Resnet18Like(), _resnext_like, _wide_like, _depth_34_like],
                         ids=["basicblock", "grouped", "wide", "other-depth"])
def test_unsupported_trunks_raise_at_construction(base):
    from tinyfaces.models.model import DetectionModel
    with pytest.raises(ValueError, match="resnet50.*resnet101.*resnet152"):
        DetectionModel(base_model=base, num_templates=25)


def test_a_foreign_module_of_a_supported_shape_is_accepted():
    """A module that is not one of the stand-ins (e.g. a real torchvision resnet50, layer4 and all) is read by its shape."""
    from tinyfaces.models.model import DetectionModel
    m = DetectionModel(base_model=lambda weights=None: ResNet((3, 4, 6, 3)), num_templates=25)
    assert m.trunk == (3, 4, 6) and not hasattr(m.model, "layer4")


def test_get_model_picks_the_trunk_of_a_checkpoint(tmp_path):
    from tinyfaces.evaluation import get_model
    from tinyfaces.models import model as mm
    for name in ("resnet50", "resnet152", "resnet101"):
        torch.manual_seed(3)
        m = mm.DetectionModel(base_model=getattr(mm, name), num_templates=25)
        torch.save({"epoch": 1, "model": m.state_dict()}, tmp_path / f"{name}.pth")
        loaded = get_model(str(tmp_path / f"{name}.pth"), num_templates=25)
        assert loaded.trunk == BLOCKS[name]
        a, b = m.state_dict(), loaded.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert get_model(None, num_templates=25).trunk == BLOCKS["resnet101"]


def test_pretrained_weights_must_match_the_trunk(tmp_path):
    from tinyfaces.models import model as mm
    torch.manual_seed(4)
    trunk = mm.resnet50()
    sd = dict(trunk.state_dict())
    sd["layer4.0.conv1.weight"] = torch.zeros(512, 1024, 1, 1)      # torchvision files carry layer4: dropped
    torch.save(sd, tmp_path / "resnet50.pth")
    m = mm.DetectionModel(base_model=mm.resnet50, pretrained_weights=str(tmp_path / "resnet50.pth"), num_templates=25)
    assert torch.equal(m.model.layer3[5].conv3.weight, trunk.layer3[5].conv3.weight)
    with pytest.raises(ValueError, match="resnet50"):
        mm.DetectionModel(base_model=mm.resnet101, pretrained_weights=str(tmp_path / "resnet50.pth"), num_templates=25)
    with pytest.raises(ValueError, match="resnet152"):
        mm.DetectionModel(base_model=mm.resnet50, pretrained_weights=_save(tmp_path, mm.resnet152()), num_templates=25)


def _save(tmp_path, trunk):
    p = tmp_path / "other.pth"
    torch.save(trunk.state_dict(), p)
    return str(p)


@pytest.mark.parametrize("name", ["resnet50", "resnet152"])
def test_engine_buckets_follow_the_trunk(name):
    """TrainEngine's gradient buckets (data-parallel overlap): block ids in executor order of THIS trunk, the flat gradient tiled exactly,
    every parameter in one bucket, the last bucket = layer1/2 + stem; the coarse cut splits layer 3 in thirds."""
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    m = mm.DetectionModel(base_model=getattr(mm, name), num_templates=25)
    flat = m.flatten_parameters()
    seg = m._segments
    blocks = BLOCKS[name]
    l3, nblk = blocks[0] + blocks[1], sum(blocks)
    assert TrainEngine.trunk_of(seg) == blocks
    names = TrainEngine.block_names(blocks)
    assert len(names) == nblk and names[l3] == "model.layer3.0." and names[-1] == f"model.layer3.{blocks[2] - 1}."
    for firsts in (TrainEngine.auto_first_blocks(seg, flat.numel(), 10), TrainEngine.coarse_first_blocks(blocks)):
        assert firsts[-1] == l3 and list(firsts) == sorted(set(firsts), reverse=True) and firsts[0] < nblk
        ranges = TrainEngine.bucket_ranges(seg, flat.numel(), firsts)
        assert ranges[0][2] == flat.numel() and ranges[-1][:2] == (-1, 0)
        for (_, s0, e0), (_, s1, e1) in zip(ranges, ranges[1:]):
            assert e1 == s0 and s1 < e1
        for k, (o, n) in seg.items():
            hit = [b for b, s, e in ranges if s <= o and o + n <= e]
            assert len(hit) == 1, k
            if k.startswith("model.layer3."):
                i = l3 + int(k.split(".")[2])
                assert hit[0] == max(f for f in firsts if f <= i), k
            elif k.startswith("model."):
                assert hit[0] == -1, k
    assert TrainEngine.bucket_ranges(seg, flat.numel()) == TrainEngine.bucket_ranges(seg, flat.numel(), TrainEngine.coarse_first_blocks(blocks))


def test_engine_buckets_of_resnet101_are_unchanged():
    from tinyfaces.engine import TrainEngine
    assert TrainEngine.coarse_first_blocks((3, 4, 23)) == (22, 14, 7)
    assert TrainEngine.block_names((3, 4, 23)) == tuple(f"model.{l}.{i}." for l, n in (("layer1", 3), ("layer2", 4), ("layer3", 23)) for i in range(n))


def test_main_takes_the_trunk_flag():
    import main
    assert main.trunk_arguments(["synthetic", "synthetic"]).base_model == "resnet101"
    args = main.trunk_arguments(["synthetic", "--base-model", "resnet50", "synthetic", "--epochs", "1"])
    assert (args.base_model, args.traindata, args.valdata, args.epochs) == ("resnet50", "synthetic", "synthetic", 1)
    with pytest.raises(SystemExit):
        main.trunk_arguments(["synthetic", "synthetic", "--base-model", "resnet18"])
    assert "base_model" not in vars(main.arguments(["synthetic", "synthetic"]))       # the reference's command line stays as it was


def test_main_pretrained_is_checked_against_the_trunk(tmp_path):
    import main
    from tinyfaces.models import model as mm
    m = mm.DetectionModel(base_model=mm.resnet152, num_templates=25)
    with pytest.raises(SystemExit, match="resnet50"):
        main.load_pretrained_trunk(m, _save(tmp_path, mm.resnet50()))
    assert main.load_pretrained_trunk(m, _save(tmp_path, mm.resnet152())) == []
