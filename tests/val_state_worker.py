"""Child process of tests/test_gpu_wider_eval.py: `main.py <argv>` in this process with tinyfaces.validation.Validator.run wrapped, so that
everything the rest of the training run depends on is digested right before and right after every validation pass.  Writes
{"passes": [{"before": {...}, "after": {...}}, ...]} to the path in VAL_STATE_OUT.

What is digested: the engine's flat parameters, momentum (or moments), accumulator and EMA; the training model's whole state_dict (the
BatchNorm buffers and counters with it); every scalar attribute of the engine, the model and the criterion (mode flags, step counters, the
learning rate, seeds, the workspace generation and the packed-weights key); the address and size of the model's workspace; the host and
device random generators (torch, numpy, random); the library's global statistic-row setting."""
import gc
import hashlib
import json
import os
import random
import sys

import numpy as np
import torch

import main as train_main
from tinyfaces import _hip, validation
from tinyfaces.engine import TrainEngine


def _digest(t):
    return None if t is None else hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _scalars(obj):
    return {k: repr(v) for k, v in sorted(vars(obj).items()) if isinstance(v, (int, float, bool, str, type(None), tuple))}


def training_state():
    engines = [o for o in gc.get_objects() if isinstance(o, TrainEngine)]
    assert len(engines) == 1, len(engines)
    eng = engines[0]
    model = eng.model
    torch.cuda.synchronize()
    ws = getattr(model, "_ws", None)
    return {
        "flat_p": _digest(eng.flat_p), "flat_m": _digest(eng.flat_m), "accum": _digest(eng._accum),
        "ema": _digest(eng.ema.flat) if eng.ema is not None else None,
        "adam": [_digest(v) for k, v in sorted(vars(eng).items()) if isinstance(v, torch.Tensor) and k not in ("flat_p", "flat_m", "_accum")],
        "state_dict": {k: _digest(v) for k, v in model.state_dict().items()},
        "engine": _scalars(eng), "model": _scalars(model), "criterion": _scalars(eng.criterion),
        "training": [bool(m.training) for m in model.modules()],
        "requires_grad": [bool(p.requires_grad) for p in model.parameters()],
        "workspace": None if ws is None else [ws.data_ptr(), ws.numel()],
        "rng_torch": _digest(torch.get_rng_state()), "rng_cuda": _digest(torch.cuda.get_rng_state()),
        "rng_numpy": hashlib.sha256(repr(np.random.get_state()).encode()).hexdigest(), "rng_random": hashlib.sha256(repr(random.getstate()).encode()).hexdigest(),
        "stat_rows": int(_hip.lib().tf_get_stat_rows()),
    }


def run():
    passes = []
    inner = validation.Validator.run

    def wrapped(self, state_dict):
        before = training_state()
        out = inner(self, state_dict)
        passes.append({"before": before, "after": training_state()})
        return out

    validation.Validator.run = wrapped
    train_main.main()
    with open(os.environ["VAL_STATE_OUT"], "w") as f:
        json.dump({"passes": passes}, f)


if __name__ == "__main__":
    sys.argv = ["main.py"] + sys.argv[1:]
    run()
