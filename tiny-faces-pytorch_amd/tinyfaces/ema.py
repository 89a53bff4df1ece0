"""Model EMA: an exponential moving average of the weights, kept on the device next to the flat parameter buffer.

What torchvision's `--model-ema`, `torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))` and timm's `ModelEmaV2` keep:
after every optimizer step  e <- e + (1 - d_t) * (p - e), and the averaged weights are the ones evaluated and shipped.  Here the average
lives in ONE flat fp32 buffer laid out like `DetectionModel.flatten_parameters()`, and one update is one launch per 128 ranges
(tf_ema_update_segments) or no launch of its own at all (TrainEngine(ema_decay=...): fused into the SGD kernels).

Arithmetic: e = fmaf(w, p - e, e) in fp32 with w = float32(1 - d_t), d_t computed in double -- torch.lerp(e, p, w) for w < 0.5.
Schedule: d_t = min(decay, (1 + t) / (10 + t)), t = updates taken so far (the warm-up of timm / tensorflow); warmup=False: d_t = decay."""
from collections import OrderedDict

import numpy as np
import torch

from . import ops


def ema_decay_at(decay, t, warmup=True):
    """d_t for the update that follows `t` earlier ones.  0 < decay < 1, anything else is a ValueError."""
    decay = float(decay)
    if not 0.0 < decay < 1.0:                                  # (a NaN fails both comparisons)
        raise ValueError(f"the EMA decay must lie strictly between 0 and 1, got {decay}")
    if not warmup:
        return decay
    return min(decay, (1.0 + t) / (10.0 + t))


class ModelEma:
    """The averaged weights of `model` (a DetectionModel on the GPU).

    flat      the average: a clone of the model's flat parameter buffer taken here (AveragedModel's first update_parameters copies too)
    updates   how many updates were taken (the `t` of the warm-up)

    The model is flattened if it is not yet (flatten_parameters keeps the nn.Parameter objects, so an optimizer built earlier stays valid).
    Only the tensors of `trainable_parameter_names()` are averaged: frozen stages, BatchNorm vectors under frozen BatchNorm and the lr-0
    upsample weight never move and stay equal to the clone.

    BatchNorm buffers (running_mean, running_var, num_batches_tracked) are NOT averaged: state_dict() takes them from the live model at the
    time of the call.  The running statistics are already exponential averages, and they belong to the live weights; re-estimating them for
    the averaged weights (torch.optim.swa_utils.update_bn) is left to the caller.  Under frozen BatchNorm the question does not arise."""

    def __init__(self, model, decay, warmup=True):
        ema_decay_at(decay, 0, warmup)
        p = next(model.parameters())
        if p.device.type != "cuda":
            raise RuntimeError(f"ModelEma: device {p.device}; the tiny-faces hot path only exists as HIP kernels for MI355X (gfx950) -- "
                               "there is no CPU fallback.")
        self.model, self.decay, self.warmup = model, float(decay), bool(warmup)
        if not self._lives_in(getattr(model, "_flat_params", None)):
            model.flatten_parameters()
        self._src = model._flat_params
        self.flat = self._src.detach().clone()
        self.updates = 0
        self._segs_key = self._segs = None

    def _lives_in(self, flat):
        """Do the model's parameters (the first and the last of the flat layout) point into `flat`?"""
        seg = getattr(self.model, "_segments", None)
        if flat is None or not seg:
            return False
        names = list(seg)
        params = dict(self.model.named_parameters())
        return all(params[k].device == flat.device and params[k].data_ptr() == flat.data_ptr() + 4 * seg[k][0] for k in (names[0], names[-1]))

    def next_weight(self):
        """float32(1 - d_t) of the next update, as a Python float; advances `updates`."""
        w = float(np.float32(1.0 - ema_decay_at(self.decay, self.updates, self.warmup)))
        self.updates += 1
        return w

    def segments(self):
        """[(start, end)] of the averaged tensors inside the flat buffer, ascending."""
        m = self.model
        key = (id(m._segments), m.batchnorm_frozen, m.trainable_layers)
        if self._segs_key != key:
            seg = m._segments
            self._segs, self._segs_key = sorted((seg[k][0], seg[k][0] + seg[k][1]) for k in m.trainable_parameter_names()), key
        return self._segs

    def update(self, clip_state=None):
        """One update from the model's current parameters: behind optimizer.step() on the autograd path (trainer.train(..., ema=)).  No host
        sync.  clip_state: a state that says skip leaves the average alone on the device (`updates` still advances)."""
        if self.model._flat_params is not self._src or not self._lives_in(self._src):
            raise RuntimeError("ModelEma.update: the model's parameters no longer live in the flat buffer this average was built on "
                               "(the model was moved or flattened again): build a new ModelEma")
        ops.ema_update_segments(self.flat, self._src, self.segments(), self.next_weight(), clip_state=clip_state)

    def state_dict(self):
        """The model's state_dict with the parameters taken from the average and the buffers from the LIVE model (see the class docstring)."""
        seg = self.model._segments
        out = OrderedDict()
        for k, v in self.model.state_dict().items():
            if k in seg:
                o, n = seg[k]
                out[k] = self.flat[o:o + n].view(v.shape).clone()
            else:
                out[k] = v.detach().clone()
        return out

    def load_state_dict(self, sd, updates):
        """The average from a state_dict written by state_dict() (a checkpoint's "model_ema") and the number of updates behind it."""
        seg = self.model._segments
        missing = [k for k in seg if k not in sd]
        if missing:
            raise KeyError(f"ModelEma.load_state_dict: {len(missing)} parameters are missing, e.g. {missing[0]}")
        for k, (o, n) in seg.items():
            if sd[k].numel() != n:
                raise ValueError(f"ModelEma.load_state_dict: {k} has {sd[k].numel()} elements, expected {n}")
            self.flat[o:o + n].copy_(sd[k].reshape(-1).to(self.flat.device, torch.float32))
        updates = int(updates)
        if updates < 0:
            raise ValueError(f"ModelEma.load_state_dict: updates must not be negative, got {updates}")
        self.updates = updates
        return self

    def copy_to(self, model):
        """Write the averaged parameters into `model` (this model or another DetectionModel of the same trunk); buffers are left alone."""
        params = dict(model.named_parameters())
        with torch.no_grad():
            for k, (o, n) in self.model._segments.items():
                params[k].copy_(self.flat[o:o + n].view(params[k].shape))
        return model

    def settings(self):
        """{"decay", "warmup", "updates"}: what a checkpoint stores next to "model_ema"."""
        return {"decay": self.decay, "warmup": self.warmup, "updates": self.updates}
