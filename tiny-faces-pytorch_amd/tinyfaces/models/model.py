"""DetectionModel -- same call surface as the reference's tinyfaces/models/model.py:7-128,
executed by the native HIP graph executor (csrc/detnet.hip) on MI355X.

What is kept from the reference:
  * constructor signature (model.py:12-16), `.forward(x)` (:89), `.learnable_parameters(lr)` (:67-87)
  * the exact state_dict (571 entries: torchvision resnet101 names under `model.` incl. the dead
    `model.fc.*` that model.py:23 leaves behind, `score_res3.*`, `score_res4.*`,
    `score4_upsample.weight` initialised to the bilinear kernel of model.py:45-65)
  * the trunk parameter `base_model` (model.py:12-23): resnet101 by default, resnet50 / resnet152
    (265 / 877 state_dict entries) or a torchvision module of the same shape -- see TRUNKS
  * real nn.Parameters, so torch.optim.SGD / StepLR (main.py:67-83) work unchanged.
What is different: forward/backward never run torch ops.  One C-ABI call per pass launches the
hand-written gfx950 kernels; a CPU tensor raises (there is no CPU fallback).
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch
from torch import nn

from .. import _hip
from .._hip import check, lib, ptr, stream

TF_DETNET_WEIGHTS_READY = 1      # include/tinyfaces_hip.h


class _Bottleneck(nn.Module):
    """Parameter container with torchvision's Bottleneck attribute names (never called)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


# Bottleneck block counts of layers 1-3 of the trunks the executor takes (torchvision's Bottleneck ResNets with groups=1 and width 64;
# `layer4` is deleted like model.py:23).  Every bottleneck has the shape of the same bottleneck of resnet101, only the counts differ.
TRUNKS = {"resnet50": (3, 4, 6), "resnet101": (3, 4, 23), "resnet152": (3, 8, 36)}
_TRUNK_NAMES = {v: k for k, v in TRUNKS.items()}
_TRUNK_ARGS = {}                 # block counts -> the `const int blocks[3]` argument of the tf_detnet_trunk_* entry points


def _trunk_arg(blocks):
    if blocks not in _TRUNK_ARGS:
        _TRUNK_ARGS[blocks] = (C.c_int * 3)(*blocks)
    return _TRUNK_ARGS[blocks]


class _BottleneckTrunk(nn.Module):
    """Parameter container with torchvision resnet50 / resnet101 / resnet152's names; `layer4` is deleted by the owner
    exactly like model.py:23, `avgpool`/`fc` stay (dead, but part of the checkpoint contract)."""

    def __init__(self, blocks=TRUNKS["resnet101"]):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, blocks[0])
        self.layer2 = self._make_layer(128, blocks[1], stride=2)
        self.layer3 = self._make_layer(256, blocks[2], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, 1000)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * 4))
        layers = [_Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * 4
        layers += [_Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


def resnet50(weights=None, **_):
    """Stand-in for `torchvision.models.resnet50` (the same names and initialisation)."""
    return _BottleneckTrunk(TRUNKS["resnet50"])


def resnet101(weights=None, **_):
    """Stand-in for `torchvision.models.resnet101` in the constructor signature (model.py:13)."""
    return _BottleneckTrunk(TRUNKS["resnet101"])


def resnet152(weights=None, **_):
    """Stand-in for `torchvision.models.resnet152` (the same names and initialisation)."""
    return _BottleneckTrunk(TRUNKS["resnet152"])


def trunk_blocks(trunk):
    """The Bottleneck block counts of layers 1-3 of `trunk` (the module `base_model` returned, layer4 deleted or not), or ValueError when the
    executor does not take it: BasicBlock trunks (resnet18 / 34), grouped (resnext) or wider (wide_resnet) bottlenecks, other depths."""
    supported = ", ".join(f"{k} {v}" for k, v in TRUNKS.items())

    def refuse(why):
        raise ValueError(f"DetectionModel: unsupported trunk ({why}). Supported: torchvision Bottleneck ResNets with groups=1 and width 64, "
                         f"block counts of layers 1-3: {supported}")
    stem = getattr(trunk, "conv1", None)
    if not isinstance(stem, nn.Conv2d) or stem.out_channels != 64 or stem.kernel_size != (7, 7):
        refuse("no 7x7 / 64-channel conv1")
    counts = []
    for L, planes in enumerate((64, 128, 256), start=1):
        layer = getattr(trunk, f"layer{L}", None)
        if not isinstance(layer, nn.Sequential) or len(layer) == 0:
            refuse(f"no layer{L}")
        for i, b in enumerate(layer):
            convs = [getattr(b, n, None) for n in ("conv1", "conv2", "conv3")]
            if not all(isinstance(c, nn.Conv2d) for c in convs):
                refuse(f"layer{L}.{i} is not a Bottleneck")
            c1, c2, c3 = convs
            if any(c.groups != 1 for c in convs):
                refuse(f"layer{L}.{i} has grouped convolutions")
            if (c1.out_channels, c2.out_channels, c3.out_channels) != (planes, planes, 4 * planes):
                refuse(f"layer{L}.{i} is not 64 wide")
            stride = 2 if i == 0 and L > 1 else 1
            if c2.kernel_size != (3, 3) or c2.stride != (stride, stride) or c1.stride != (1, 1):
                refuse(f"layer{L}.{i} does not stride on its 3x3")
            if (getattr(b, "downsample", None) is not None) != (i == 0):
                refuse(f"layer{L}.{i}: a downsample branch on a block other than the first")
        counts.append(len(layer))
    if tuple(counts) not in _TRUNK_NAMES:
        refuse(f"block counts {tuple(counts)}")
    return tuple(counts)


def _state_dict_blocks(sd, prefix):
    """Block counts of layers 1-3 in a state_dict (keys `<prefix>layerL.i.`), None when it has no such keys."""
    counts = [0, 0, 0]
    for k in sd:
        parts = k[len(prefix):].split(".") if k.startswith(prefix) else ()
        if len(parts) > 2 and parts[0] in ("layer1", "layer2", "layer3") and parts[1].isdigit():
            L = int(parts[0][-1]) - 1
            counts[L] = max(counts[L], int(parts[1]) + 1)
    return tuple(counts) if any(counts) else None


def base_model_of(sd):
    """The stand-in (resnet50 / resnet101 / resnet152) of the trunk a DetectionModel state_dict holds (`model.layerL.i.` keys);
    resnet101 when it has none."""
    blocks = _state_dict_blocks(sd, "model.")
    if blocks is None:
        return resnet101
    if blocks not in _TRUNK_NAMES:
        raise ValueError(f"state_dict holds a trunk with block counts {blocks}; supported: {TRUNKS}")
    return {"resnet50": resnet50, "resnet101": resnet101, "resnet152": resnet152}[_TRUNK_NAMES[blocks]]


class _DetNetFunction(torch.autograd.Function):
    """forward = tf_detnet_forward, backward = tf_detnet_backward (csrc/detnet.hip)."""

    @staticmethod
    def forward(ctx, x, owner, *params):
        out = owner._run_forward(x, training=True)
        ctx.owner = owner
        ctx.save_for_backward(x)
        ctx.ws_generation = owner._ws_generation
        return out

    @staticmethod
    def backward(ctx, gout):
        owner = ctx.owner
        (x,) = ctx.saved_tensors
        if ctx.ws_generation != owner._ws_generation:
            raise RuntimeError("DetectionModel: the activation arena was reused by a later forward before this "
                               "backward ran (one in-flight training step per model)")
        grads = owner._run_backward(x, gout.contiguous().float())
        if owner._ws_mode == _hip.TF_DETNET_FROZEN_BN:         # frozen BatchNorm: weight / bias have NO gradient (FrozenBatchNorm2d) ...
            keep = owner._trainable_set(True, owner._ws_trainable)      # ... and neither has a conv weight of a frozen stage (set_trainable_layers)
            grads = [g if k in keep or k == _UPSAMPLE else None for k, g in zip(owner._grad_names, grads)]
        return (None, None) + tuple(grads)


# The trunk's stages from the top, as set_trainable_layers counts them: torchvision's ["layer4", "layer3", "layer2", "layer1", "conv1"] without
# the deleted layer4; `trainable_layers = k` trains the heads and the first k of these
_STAGES = ("model.layer3.", "model.layer2.", "model.layer1.", "model.conv1.")
_UPSAMPLE = "score4_upsample.weight"     # lr 0 (model.py:84): not trained, its gradient is DEFINED as zero in every mode


# Every register_parameter / register_buffer of ANY module in the process (Module.__setattr__ goes through them too) bumps this counter: a frozen
# pointer table (DetectionModel._sync_tables) is only trusted while nothing was registered since it was built.
_REGISTRATIONS = [0]


def _count_registration(module, name, value):
    _REGISTRATIONS[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_count_registration)
torch.nn.modules.module.register_module_buffer_registration_hook(_count_registration)


def _invalidate_tables(module, incompatible_keys):
    """load_state_dict post-hook (a module-level function: the model stays picklable)."""
    module._table_key = None


class DetectionModel(nn.Module):
    """Hybrid-resolution Tiny Faces detector (model.py:7-128) on the MI355X executor."""

    def __init__(self, base_model=resnet101, pretrained_weights=None, num_templates=1, num_objects=1):
        super().__init__()
        output = (num_objects + 4) * num_templates                       # model.py:19
        self.num_out = output
        self.model = base_model(weights=None) if callable(base_model) else _BottleneckTrunk()
        if hasattr(self.model, "layer4"):
            del self.model.layer4                                        # model.py:23
        self.trunk = trunk_blocks(self.model)                            # what the executor runs (ValueError: a trunk it does not take)
        self.score_res3 = nn.Conv2d(512, output, 1)                      # model.py:25-28
        self.score_res4 = nn.Conv2d(1024, output, 1)                     # model.py:29-32
        self.score4_upsample = nn.ConvTranspose2d(output, output, 4, stride=2, padding=1, bias=False)   # :34-39
        self._init_bilinear()
        self.compute_dtype = _hip.tf_dtype(os.environ.get("TINYFACES_DTYPE", "bf16"))
        self._ws = None
        self._ws_generation = 0
        self._table_key = None
        self._frozen_tensors, self._frozen_version = (), -1
        self._bn_frozen = False          # freeze_batchnorm(): a mode like train() / eval(), not part of the state_dict
        self._trainable_layers = 4       # set_trainable_layers(): a mode too
        self._ws_trainable = 4           # ... and its value at the forward whose activations sit in the workspace
        self._ws_mode = 0                # the executor mode (0 eval, 1 batch statistics, 2 frozen BN) of the forward whose activations sit in the workspace
        self._session_depth = 0          # constant_weights() nesting
        self._ready_key = None           # (workspace ptr, dtype, table key) whose packed eval weights sit in the workspace
        self._lanes = []                 # forward_levels: extra (workspace, HIP stream, ready key) triples beside the model's own
        # load_state_dict(assign=True) re-points parameters without _apply: the pointer tables are rebuilt on the next call
        self.register_load_state_dict_post_hook(_invalidate_tables)
        if isinstance(pretrained_weights, (str, os.PathLike)):           # no network here: a local file only
            sd = torch.load(pretrained_weights, map_location="cpu", weights_only=True)
            sd = sd.get("model", sd)
            self.check_trunk_of(sd, pretrained_weights)
            if any(k.startswith("model.") for k in sd):
                self.load_state_dict(sd, strict=False)
            else:                                                        # a bare torchvision resnet101 state_dict
                self.model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("layer4.")}, strict=False)
        elif pretrained_weights is not None:
            # the reference's default (ResNet101_Weights.IMAGENET1K_V1, model.py:13-14) is a download: impossible here.  Say so
            # loudly instead of silently training from random weights with the reference's schedule.
            import warnings
            warnings.warn(f"DetectionModel: pretrained_weights={pretrained_weights!r} is not a local file -- ignored, the trunk "
                          "keeps its RANDOM kaiming initialisation (no network to download ImageNet weights). Pass a path to a "
                          "torchvision resnet101 state_dict instead.", RuntimeWarning, stacklevel=2)

    @property
    def trunk_name(self):
        """"resnet50", "resnet101" or "resnet152"."""
        return _TRUNK_NAMES[self.trunk]

    def check_trunk_of(self, sd, what="state_dict"):
        """ValueError when `sd` (a torchvision trunk state_dict, or a checkpoint with `model.`-prefixed keys) holds another trunk than this model's."""
        got = _state_dict_blocks(sd, "model." if any(k.startswith("model.") for k in sd) else "")
        if got is not None and got != self.trunk:
            name = _TRUNK_NAMES.get(got, f"a trunk with block counts {got}")
            raise ValueError(f"{what}: holds {name}, the model is {self.trunk_name} {self.trunk}")

    # ---- reference surface ---------------------------------------------------------------
    def _init_bilinear(self):
        """model.py:45-65: diagonal bilinear kernel [.25,.75,.75,.25] (x) [.25,.75,.75,.25]."""
        k = self.score4_upsample.kernel_size[0]
        factor = np.floor((k + 1) / 2)
        center = factor if k % 2 == 1 else factor + 0.5
        c = np.arange(1, k + 1)
        v = np.ones((1, k)) - (np.abs(c - center) / factor)
        f = np.zeros((self.score4_upsample.in_channels, self.score4_upsample.out_channels, k, k))
        idx = np.arange(self.score4_upsample.out_channels)
        f[idx, idx] = v.T @ v
        self.score4_upsample.weight = nn.Parameter(torch.Tensor(f))

    def learnable_parameters(self, lr):
        """model.py:67-87: 4 SGD groups (trunk lr, score_res3 0.1*lr, score_res4 lr, upsample 0)."""
        return [{"params": self.model.parameters(), "lr": lr},
                {"params": self.score_res3.parameters(), "lr": 0.1 * lr},
                {"params": self.score_res4.parameters(), "lr": 1 * lr},
                {"params": self.score4_upsample.parameters(), "lr": 0}]

    def freeze_batchnorm(self, on=True):
        """Fine-tune on the statistics and affine the trunk was pretrained with (torchvision's FrozenBatchNorm2d; `bn.eval()` on every
        BatchNorm2d with its parameters `requires_grad = False`): every BatchNorm is the constant map v -> v * s + h with
        s = weight / sqrt(running_var + eps), h = bias - running_mean * s.  A mode like train() / eval(): it is not part of the
        state_dict and survives .train(), .eval() and .to().  While it is on

        * train() with gradients enabled runs the folded-BN graph forward AND backward (the forward is the evaluation forward bit for bit);
          running_mean, running_var, num_batches_tracked, weight and bias of every BatchNorm are read, never written; BN weight / bias get
          no gradient (`.grad` stays None, TrainEngine applies neither weight decay nor momentum to them); every conv weight and the head
          weights / biases get the gradient autograd gives the reference model with its BatchNorm2d modules in eval();
        * train() under no_grad runs the folded forward and writes nothing;
        * eval() is unchanged.

        Per-module modes are NOT honoured: the executor looks at the model's own flags only, `model.model.layer1[0].bn1.eval()` is
        ignored exactly as without this switch.  fp16 stays an inference-only operand type.  set_trainable_layers(k) freezes the stem
        and the lowest stages of the trunk on top of this mode.  Returns self."""
        self._bn_frozen = bool(on)
        return self

    @property
    def batchnorm_frozen(self):
        """True while freeze_batchnorm() is on."""
        return self._bn_frozen

    def set_trainable_layers(self, k):
        """Fine-tune the heads and the top `k` of the trunk's four stages -- from the top: layer3, layer2, layer1, stem (conv1 + bn1) -- and
        keep the rest on their pretrained weights: torchvision's `trainable_backbone_layers` (its list without the deleted layer4), Detectron's
        FREEZE_AT.  4 (the default) trains everything, 0 the two score heads only.  A mode like freeze_batchnorm(): not part of the
        state_dict, it survives train(), eval(), .to() and pickling and does not travel with load_state_dict.

        Partial freezing is defined on the frozen-BN graph only (in torchvision frozen stages always sit on frozen BatchNorm): with k < 4
        and batchnorm_frozen False a train() forward with gradients enabled raises RuntimeError (call freeze_batchnorm(); the order of the
        two setters does not matter); eval() and no_grad forwards never look at k.  While k < 4 and BatchNorm is frozen

        * the training forward is the frozen (= evaluation) forward, bit for bit;
        * the backward pass stops where the trained part begins: no data or weight gradient of a frozen stage is launched;
        * the conv weights of the frozen stages get no gradient (`.grad` stays None like a BN weight's, so torch.optim.SGD skips them: no
          update, no weight decay, no momentum; TrainEngine does the same); every trained tensor gets the gradient autograd gives the
          reference model with its BatchNorm2d in eval() and requires_grad_(False) on every parameter of the frozen stages;
        * `requires_grad` flags are not touched and learnable_parameters() stays the reference's four groups.

        Per-module flags are still NOT honoured (see freeze_batchnorm): the executor looks at the model's own modes only.  Returns self."""
        if type(k) is not int or not 0 <= k <= 4:
            raise ValueError(f"set_trainable_layers: k must be one of the ints 0, 1, 2, 3, 4 (got {k!r})")
        self._trainable_layers = k
        return self

    @property
    def trainable_layers(self):
        """How many of the trunk's stages (layer3, layer2, layer1, stem) are trained: set_trainable_layers()."""
        return getattr(self, "_trainable_layers", 4)

    def _executor_names(self):
        names = getattr(self, "_names", None)
        if not names:
            tr = _trunk_arg(self.trunk)
            names = [lib().tf_detnet_trunk_param_name(tr, i).decode() for i in range(lib().tf_detnet_trunk_num_params(tr))]
        return names

    def trainable_parameter_names(self):
        """The names of the tensors that receive a gradient under the current two modes (freeze_batchnorm, set_trainable_layers), in
        executor order: the head weights and biases, the conv weights of the trained stages and, unless BatchNorm is frozen, the BN weights
        and biases.  score4_upsample.weight is never among them: it is not trained (lr 0) and its gradient is defined as zero."""
        return self._trainable_names(self._bn_frozen, self.trainable_layers)

    def _trainable_names(self, bn_frozen, k):
        cache = self.__dict__.setdefault("_trainable_cache", {})
        if (bn_frozen, k) not in cache:
            params = dict(self.named_parameters())
            bn = frozenset(f"{n}.{w}" for n, m in self.named_modules() if isinstance(m, nn.BatchNorm2d) for w in ("weight", "bias"))
            cut = _STAGES[k:] if bn_frozen else ()            # (partial freezing exists on the frozen-BN graph only)
            cache[(bn_frozen, k)] = tuple(n for n in self._executor_names() if n in params and n != _UPSAMPLE and not (bn_frozen and n in bn)
                                          and not n.startswith(cut))
        return list(cache[(bn_frozen, k)])

    def _trainable_set(self, bn_frozen, k):
        cache = self.__dict__.setdefault("_trainable_set_cache", {})
        if (bn_frozen, k) not in cache:
            cache[(bn_frozen, k)] = frozenset(self._trainable_names(bn_frozen, k))
        return cache[(bn_frozen, k)]

    def _first_block(self, k):
        """tf_detnet_trunk_backward_frozen_from_ctx's first_block for `k` trainable stages: the lowest bottleneck with weight gradients."""
        n1, n2, n3 = self.trunk
        return (n1 + n2 + n3, n1 + n2, n1, 0, -1)[k]

    def _check_partial_freeze(self):
        if self.trainable_layers < 4 and not self._bn_frozen:
            raise RuntimeError(f"DetectionModel: set_trainable_layers({self.trainable_layers}) freezes stages of the trunk, which is defined on the "
                               "frozen-BatchNorm graph only: call freeze_batchnorm() as well (or set_trainable_layers(4))")

    def set_compute_dtype(self, dtype):
        """torch.float32 (exact-fp32 MFMA, parity path), torch.bfloat16 (fast path, training and inference) or torch.float16
        (fp16 MFMA operands, inference only: the hard-setting evaluation of BASELINE.json configs[4])."""
        self.compute_dtype = _hip.tf_dtype(dtype)
        return self

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("DetectionModel.forward: input is on the CPU. This build has no CPU path: the forward/"
                               "backward of the detector only exist as HIP kernels for MI355X (gfx950).")
        x = x.contiguous().float()
        self._sync_tables(x.device)
        if self.training and torch.is_grad_enabled():
            self._check_partial_freeze()                 # (before anything is launched or written)
            params = [p for p in self._grad_params]
            return _DetNetFunction.apply(x, self, *params)
        # (frozen BatchNorm under no_grad: the folded forward, nothing written -- not the statistics update of a plain train() forward)
        return self._run_forward(x, training=self.training and not self._bn_frozen)

    def forward_levels(self, xs, lanes=None):
        """`[self(x) for x in xs]` for the pyramid levels of ONE image (evaluation.py:49-68 runs them one after the other), eval mode only,
        with the levels spread over `lanes` HIP streams so that they run SIDE BY SIDE: the forward of a 1/4- or 1/16-size level is a chain
        of ~110 launches of 10-20 us each that fill a fraction of the 256 CUs (M = 1200-4800 pixels at layer 3: latency-bound whatever the
        kernel), and it hides completely beside the full-size level, which is throughput-bound.  Every lane owns a workspace (its packed
        weights + its activations: the executor is stateless beyond `ws`), the largest level runs on the caller's stream in the model's
        own workspace, the rest are dealt to the other lanes by decreasing size; the caller's stream waits for all lanes at the end.
        The outputs are those of the sequential loop bit for bit (same kernels, same launch geometry; tests/test_gpu_model.py).
        TINYFACES_EVAL_LANES (default 3) / lanes=1: the sequential loop."""
        xs = list(xs)
        n_lanes = int(os.environ.get("TINYFACES_EVAL_LANES", "3")) if lanes is None else int(lanes)
        if self.training or len(xs) < 2 or n_lanes < 2 or self._session_depth == 0:
            return [self(x) for x in xs]
        for x in xs:
            if not x.is_cuda:
                raise RuntimeError("DetectionModel.forward_levels: input is on the CPU (no CPU path)")
        xs = [x.contiguous().float() for x in xs]
        dev = xs[0].device
        self._sync_tables(dev)
        order, lane_of = self.assign_lanes([x.shape[0] * x.shape[2] * x.shape[3] for x in xs], n_lanes)
        while len(self._lanes) < n_lanes - 1:
            self._lanes.append({"ws": None, "stream": torch.cuda.Stream(device=dev, priority=int(os.environ.get("TINYFACES_EVAL_LANE_PRIO", "0"))), "ready": None})
        cur = torch.cuda.current_stream(dev)
        inputs_ready = cur.record_event()                                 # the level tensors were produced on the caller's stream
        outs = [None] * len(xs)
        used = set()
        big_first = os.environ.get("TINYFACES_EVAL_LANES_ORDER", "big") == "big"
        for i in (order if big_first else order[::-1]):                   # by decreasing size: the full-size level is enqueued first
            ln = lane_of[i]
            if ln == 0:
                outs[i] = self._run_forward(xs[i], training=False)
                continue
            lane = self._lanes[ln - 1]
            if ln not in used:
                lane["stream"].wait_event(inputs_ready)
                used.add(ln)
            outs[i] = self._run_eval_lane(xs[i], lane)
        for ln in used:
            cur.wait_stream(self._lanes[ln - 1]["stream"])
        return outs

    @staticmethod
    def assign_lanes(sizes, n_lanes):
        """(order, lane_of) for forward_levels: levels by decreasing size (ties: list order); the largest goes to lane 0 -- the caller's
        stream and the model's own workspace --, every further one to the lane with the least pixels so far (ties: lowest lane)."""
        order = sorted(range(len(sizes)), key=lambda i: (-sizes[i], i))
        load = [0] * n_lanes
        lane_of = {}
        for i in order:
            ln = 0 if not lane_of else min(range(n_lanes), key=lambda k: (load[k], k))
            lane_of[i] = ln
            load[ln] += sizes[i]
        return order, lane_of

    def _run_eval_lane(self, x, lane):
        """Eval-mode tf_detnet_forward of one level on a lane's own stream and workspace (forward_levels)."""
        N, _, H, W = x.shape
        H3, W3 = C.c_int(), C.c_int()
        lib().tf_detnet_out_shape(H, W, C.byref(H3), C.byref(W3))
        nbytes = lib().tf_detnet_trunk_workspace_bytes(_trunk_arg(self.trunk), self.compute_dtype, N, H, W, self.num_out, 0)
        if lane["ws"] is None or lane["ws"].device != x.device or lane["ws"].numel() < nbytes:
            lane["ws"] = None
            lane["ws"] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        ws = lane["ws"]
        out = torch.empty(N, self.num_out, H3.value, W3.value, dtype=torch.float32, device=x.device)
        key = (ws.data_ptr(), self.compute_dtype, self._table_key, self._session_serial)
        flags = TF_DETNET_WEIGHTS_READY if key == lane["ready"] else 0
        lane["ready"] = key
        bn = self.model.bn1
        with torch.cuda.device(x.device):
            check(lib().tf_detnet_trunk_forward_ctx(_trunk_arg(self.trunk), self._ctx(x.device), int(self.single_stream), self.compute_dtype, 0, ptr(x),
                                                    N, H, W, self.num_out, self._param_ptrs, float(bn.eps), float(bn.momentum), ptr(out), ptr(ws),
                                                    ws.numel(), flags, lane["stream"].cuda_stream),
                  "tf_detnet_trunk_forward_ctx")
        return out

    # ---- executor plumbing ---------------------------------------------------------------
    def _named_tensors(self):
        d = dict(self.named_parameters())
        d.update(dict(self.named_buffers()))
        return d

    def __getstate__(self):
        # pickling / copy.deepcopy: the executor's derived state (ctypes pointer tables, workspaces, streams) belongs to THIS object's storages;
        # a copy rebuilds it on its first call
        d = dict(self.__dict__)
        d.update(_table_key=None, _tables_frozen=False, _frozen_tensors=(), _frozen_version=-1, _ws=None, _ready_key=None, _lanes=[], _session_depth=0,
                 _ws_mode=0)
        for k in ("_param_ptrs", "_grad_params", "_bn_modules", "_bn_param_names", "_trainable_cache", "_trainable_set_cache"):
            d.pop(k, None)
        return d

    def _apply(self, fn, *a, **kw):
        # .to() / .cuda() / .float(): every storage may move -> the pointer tables are rebuilt on the next call even when frozen
        self._table_key = None
        self._tables_frozen = False
        return super()._apply(fn, *a, **kw)

    def _sync_tables(self, device):
        """(Re)build the device-pointer tables the executor reads, keyed on storage identity.  The check itself walks 571 tensors
        (~0.4 ms of Python): an owner that pins the storages (TrainEngine after flatten_parameters) sets `_tables_frozen` and the walk is
        skipped until something moves the module (`_apply`, flatten_parameters)."""
        # (a constant_weights() session is the same promise as a frozen owner: the cheap check instead of the walk for every image of an evaluation loop)
        if (getattr(self, "_tables_frozen", False) or self._session_depth > 0) and self._table_key is not None:
            # frozen: no walk over the module tree, but EVERY tensor of the table is still checked (three sentinels missed a
            # replaced tensor in between).  Replacing a Parameter or a buffer anywhere registers it with its module, which bumps the global
            # registration counter below; re-pointing `.data` keeps the object and moves its storage, which the pointer comparison over the
            # cached tensor objects sees (571 data_ptr() calls, ~40 us); load_state_dict(assign=True) is caught by the post-hook
            if self._frozen_version == _REGISTRATIONS[0] and all(t.data_ptr() == p for t, p in zip(self._frozen_tensors, self._table_key)):
                return
        named = self._named_tensors()
        tr = _trunk_arg(self.trunk)
        n = lib().tf_detnet_trunk_num_params(tr)
        names = self._names if getattr(self, "_names", None) and len(self._names) == n else [lib().tf_detnet_trunk_param_name(tr, i).decode() for i in range(n)]
        key = tuple(named[k].data_ptr() for k in names)
        if key == self._table_key:
            return
        for i, k in enumerate(names):
            t = named[k]
            if t.device != device:
                raise RuntimeError(f"parameter {k} is on {t.device}, input on {device}: call model.to(device) first")
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise RuntimeError(f"parameter {k} must be contiguous float32")
            want = lib().tf_detnet_trunk_param_numel(tr, i, self.num_out)
            if t.numel() != want:
                raise RuntimeError(f"parameter {k}: {t.numel()} elements, executor expects {want}")
        up = self.score4_upsample.weight.detach()
        off = up.clone()
        idx = torch.arange(self.num_out, device=up.device)
        off[idx, idx] = 0
        if float(off.abs().sum()) != 0.0:
            raise RuntimeError("score4_upsample.weight has off-diagonal entries: the executor implements the frozen "
                               "per-channel bilinear upsample of model.py:45-65 (lr=0, model.py:84) only")
        self._names = names
        self._param_ptrs = (C.c_void_p * n)(*[named[k].data_ptr() for k in names])
        self._grad_names = [k for k in names if k in dict(self.named_parameters())]
        pd = dict(self.named_parameters())
        self._grad_params = [pd[k] for k in self._grad_names]
        self._grad_numels = [pd[k].numel() for k in self._grad_names]
        self._bn_modules = [m for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
        self._bn_param_names = frozenset(f"{n}.{w}" for n, m in self.named_modules() if isinstance(m, nn.BatchNorm2d) for w in ("weight", "bias"))
        self._table_key = key
        self._frozen_tensors = [named[k] for k in names]
        self._frozen_version = _REGISTRATIONS[0]

    def _named_tensor(self, dotted):
        obj = self
        for part in dotted.split("."):
            obj = getattr(obj, part)
        return obj

    def flatten_parameters(self):
        """Re-point every parameter the executor trains into ONE flat fp32 buffer (executor order, each
        segment 16-byte aligned) and all BatchNorm counters into one int64 buffer.  The nn.Parameter objects
        keep their identity (optimizers stay valid); afterwards a whole parameter group is one contiguous
        range, so the fused SGD step and the RCCL all-reduce work on a handful of large segments."""
        dev = next(self.parameters()).device
        self._sync_tables(dev)
        pd = dict(self.named_parameters())
        total = sum((n + 3) // 4 * 4 for n in self._grad_numels)
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._segments, o = {}, 0
        for k, n in zip(self._grad_names, self._grad_numels):
            p = pd[k]
            flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat[o:o + n].view_as(p)
            self._segments[k] = (o, n)
            o += (n + 3) // 4 * 4
        self._flat_params = flat
        nbt = [m for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
        cnt = torch.zeros(len(nbt), dtype=torch.int64, device=dev)
        for i, m in enumerate(nbt):
            cnt[i] = m.num_batches_tracked
            m.num_batches_tracked = cnt[i]
            m._buffers["num_batches_tracked"] = cnt[i:i + 1].view(())
        self._flat_nbt = cnt
        self._grad_flat_persistent = torch.zeros(total, dtype=torch.float32, device=dev)
        self._table_key = None
        self._sync_tables(dev)
        return flat

    def group_ranges(self):
        """[(start, end, lr_multiplier)] of the 4 reference parameter groups (model.py:67-87) inside the flat buffer."""
        seg = self._segments
        def span(prefix):
            ks = [k for k in self._grad_names if k.startswith(prefix)]
            return seg[ks[0]][0], seg[ks[-1]][0] + (seg[ks[-1]][1] + 3) // 4 * 4
        return [span("model.") + (1.0,), span("score_res3.") + (0.1,), span("score_res4.") + (1.0,), span("score4_upsample.") + (0.0,)]

    def _ctx(self, device):
        """The executor context of this model on `device` (include/tinyfaces_hip.h: tf_detnet_ctx -- second stream + event pool): created on
        first use with that device current, destroyed with the model.  Two models never share a stream or an event."""
        ctxs = self.__dict__.setdefault("_exec_ctx", {})
        key = (device.type, device.index)
        if key not in ctxs:
            h = C.c_void_p()
            with torch.cuda.device(device):
                check(lib().tf_detnet_ctx_create(C.byref(h)), "tf_detnet_ctx_create")
            ctxs[key] = h
        return ctxs[key]

    def __del__(self):
        for h in self.__dict__.get("_exec_ctx", {}).values():
            try:
                lib().tf_detnet_ctx_destroy(h)
            except Exception:
                pass

    single_stream = False            # True: weight gradients on the caller's stream (A/B + race-screen tests)

    def _workspace(self, device, nbytes):
        if self._ws is None or self._ws.device != device or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    @contextlib.contextmanager
    def constant_weights(self, reserve=None):
        """Promise that no parameter/buffer value changes inside the block (eval mode): the executor packs the weights
        and folds the BN statistics on the first forward and reuses them for every later one, whatever the image size.
        The pyramid of get_detections (evaluation.py:49-82) is 3-5 forwards on constant weights.  `reserve=(N, H, W)` sizes
        the workspace for the largest input up front so that it is not re-allocated (which would drop the packed copy)."""
        if reserve is not None:
            dev = next(self.parameters()).device
            self._workspace(dev, lib().tf_detnet_trunk_workspace_bytes(_trunk_arg(self.trunk), self.compute_dtype, *reserve, self.num_out, 0))
        if self._session_depth == 0:
            self._ready_key = None
            self._session_serial = getattr(self, "_session_serial", 0) + 1     # the lanes of forward_levels re-pack once per session too
        self._session_depth += 1
        try:
            yield self
        finally:
            self._session_depth -= 1
            if self._session_depth == 0:
                self._ready_key = None

    def _run_forward(self, x, training):
        N, _, H, W = x.shape
        H3, W3 = C.c_int(), C.c_int()
        lib().tf_detnet_out_shape(H, W, C.byref(H3), C.byref(W3))
        # the executor mode: 0 evaluation, 1 batch statistics, 2 frozen BatchNorm (the evaluation forward + what its backward needs)
        mode = (_hip.TF_DETNET_FROZEN_BN if getattr(self, "_bn_frozen", False) else 1) if training else 0
        nbytes = lib().tf_detnet_trunk_workspace_bytes(_trunk_arg(self.trunk), self.compute_dtype, N, H, W, self.num_out, mode)
        ws = self._workspace(x.device, nbytes)
        self._ws_generation += 1
        self._ws_mode = mode
        self._ws_trainable = self.trainable_layers if mode == _hip.TF_DETNET_FROZEN_BN else 4
        self._ws_shape = (N, H, W)
        out = torch.empty(N, self.num_out, H3.value, W3.value, dtype=torch.float32, device=x.device)
        bn = self.model.bn1
        flags = 0
        if training:
            self._ready_key = None
        elif self._session_depth > 0:
            key = (ws.data_ptr(), self.compute_dtype, self._table_key)
            if key == self._ready_key:
                flags = TF_DETNET_WEIGHTS_READY
            self._ready_key = key
        with torch.cuda.device(x.device):
            check(lib().tf_detnet_trunk_forward_ctx(_trunk_arg(self.trunk), self._ctx(x.device), int(self.single_stream), self.compute_dtype, mode,
                                                    ptr(x), N, H, W, self.num_out, self._param_ptrs, float(bn.eps), float(bn.momentum), ptr(out), ptr(ws),
                                                    ws.numel(), flags, stream()),
                  "tf_detnet_trunk_forward_ctx")
        if mode == 1:                                                     # (frozen BatchNorm: the counters are not written either)
            if getattr(self, "_flat_nbt", None) is not None:
                self._flat_nbt += 1                                      # all 94 counters in one launch
            else:
                for m in self._bn_modules:                               # BatchNorm2d bookkeeping
                    if m.num_batches_tracked is not None:
                        m.num_batches_tracked += 1
        return out

    def _run_backward(self, x, gout, persistent=False):
        """persistent=False (autograd path): a fresh flat gradient buffer per call, returned as per-parameter views.
        persistent=True (fused trainer): gradients land in self._grad_flat_persistent (same layout as the flat
        parameter buffer); returns that buffer."""
        N, _, H, W = x.shape
        assert (N, H, W) == self._ws_shape
        total = sum((n + 3) // 4 * 4 for n in self._grad_numels)       # every segment 16-byte aligned
        if persistent:
            gflat = self._grad_flat_persistent
            cache = getattr(self, "_persist_table", None)
        else:
            gflat = torch.zeros(total, dtype=torch.float32, device=x.device)
            cache = None
        if cache is None or cache[0] != gflat.data_ptr():
            ptrs, o = {}, 0
            for k, n in zip(self._grad_names, self._grad_numels):
                ptrs[k] = gflat.data_ptr() + 4 * o
                o += (n + 3) // 4 * 4
            table = (C.c_void_p * len(self._names))(*[ptrs.get(k, 0) for k in self._names])
            if persistent:
                self._persist_table = (gflat.data_ptr(), table)
        else:
            table = cache[1]
        # gradient-ready hooks of a data-parallel TrainEngine live in THIS model (`_grad_events`, `_grad_callback`, set by the engine that
        # owns it) and travel as an ARGUMENT of this model's own backward call (tf_detnet_hooks, r4): nothing is registered process-wide,
        # several models / engines / threads never see each other's events.  The callback reduces slices of the PERSISTENT flat buffer, so
        # the autograd path (fresh buffer per call; trainer.train reduces behind the backward pass, parallel.GradientReducer) never gets it.
        ev = getattr(self, "_grad_events", None)
        cb = getattr(self, "_grad_callback", None) if (ev is not None and persistent) else None
        hooks = _hip.DetnetHooks()
        if ev is not None:
            hooks.blocks, hooks.events, hooks.n = C.cast(ev[0], C.POINTER(C.c_int)), C.cast(ev[1], C.POINTER(C.c_void_p)), ev[2]
        hooks.fn = C.cast(cb, C.c_void_p) if cb is not None else None
        hooks.user = getattr(self, "_grad_callback_user", None) if cb is not None else None
        hooks.single_stream = int(self.single_stream)
        frozen = self._ws_mode == _hip.TF_DETNET_FROZEN_BN                # the graph the forward ran decides, not the flag at backward time
        entry = lib().tf_detnet_trunk_backward_frozen_from_ctx if frozen else lib().tf_detnet_trunk_backward_ctx
        cut = (self._first_block(getattr(self, "_ws_trainable", 4)),) if frozen else ()       # (what was set when the forward ran)
        with torch.cuda.device(x.device):
            check(entry(_trunk_arg(self.trunk), self._ctx(x.device), C.byref(hooks), self.compute_dtype, ptr(x), N, H, W,
                        self.num_out, self._param_ptrs, table, ptr(gout), ptr(gflat), gflat.numel() * 4, ptr(self._ws),
                        self._ws.numel(), stream(), *cut), "tf_detnet_trunk_backward_frozen_from_ctx" if frozen else "tf_detnet_trunk_backward_ctx")
        self._last_grad_flat = gflat
        if persistent:
            return gflat
        pd = dict(self.named_parameters())
        views, o = [], 0
        for k, n in zip(self._grad_names, self._grad_numels):
            views.append(gflat[o:o + n].view_as(pd[k]))
            o += (n + 3) // 4 * 4
        return views
