"""-m gpu: the target front end is ONE path.  The list entries of ops, its resident entries (with and without out=) and the loaders' TargetAssigner
must return the same bits for every assigner x ignore configuration, and each configuration must make exactly its own library calls.
Every case is loss_cases.mixed_batch(): six images, among them empty ones and ones with degenerate boxes, on the 63 x 63 map."""
import numpy as np
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

ASSIGNERS = {"plain": {}, "comp": {"compensate": (3, 0.1)}, "atss": {"assigner": "atss", "atss_topk": 9}}      # TargetAssigner's keywords
IGNORE = ("iof", 0.5)
CONFIGS = [(a, ign) for a in ASSIGNERS for ign in (False, True)]
# the library calls of a configuration, in order (+ tf_targets_apply_ignore when the batch has an ignore box)
CALLS = {"plain": ["tf_targets_workspace_bytes", "tf_dense_overlap_targets"],
         "comp": ["tf_targets_comp_workspace_bytes", "tf_dense_overlap_targets_comp"],
         "atss": ["tf_targets_atss_workspace_bytes", "tf_targets_atss"]}


def _ignore_boxes(m):
    return [np.array([[5.0, 5.0, 90.0, 90.0]])] * len(m["boxes"])


def _list_entry(ops, name, ign, m, templates, seed):
    """The ops call a TargetAssigner of this configuration stands for, every counter the configuration has asked for."""
    kw = dict(paste_boxes=m["paste"], flips=m["flips"])
    if ign:
        kw.update(ignore_boxes=_ignore_boxes(m), ignore=IGNORE, return_ignored_count=True)
    if name == "atss":
        return ops.atss_targets(m["boxes"], templates, topk=9, return_match_count=True, **kw)
    if name == "comp":
        kw.update(compensate=(3, 0.1), return_match_count=True)
    return ops.dense_overlap_targets(m["boxes"], templates, seed=seed, **kw)


def _resident_entry(ops, name, ign, m, templates, seed, out=None):
    dev = torch.device("cuda")
    boxes_d, offs_d, total = ops._upload_boxes(m["boxes"], dev)
    kw = dict(paste_d=torch.tensor(m["paste"], dtype=torch.int32, device=dev), flips_d=torch.tensor(m["flips"], dtype=torch.int32, device=dev), out=out)
    if ign:
        ign_d, ioffs_d, total_ignore = ops._upload_boxes(_ignore_boxes(m), dev)
        kw.update(ignore_d=ign_d, ignore_offs_d=ioffs_d, total_ignore=total_ignore, ignore=IGNORE, return_ignored_count=True)
    t_d = ops._upload_templates(templates, dev)
    assert ops._upload_templates(t_d, dev) is t_d                     # a resident float64 table is not copied
    if name == "atss":
        return ops.atss_targets_device(boxes_d, offs_d, total, t_d, topk=9, return_match_count=True, **kw)
    if name == "comp":
        kw.update(compensate=(3, 0.1), return_match_count=True)
    return ops.dense_overlap_targets_device(boxes_d, offs_d, total, t_d, seed=seed, **kw)


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x, y), f"{what}: returned tensor {i} differs"


def test_paths_agree(templates):
    """List entry == resident entry == resident entry into a NaN-filled out= == TargetAssigner, in every returned tensor, for all six configurations."""
    for name, ign in CONFIGS:
        _paths_agree(templates, name, ign)


def _paths_agree(templates, name, ign):
    from tinyfaces import ops
    from tinyfaces.datasets import TargetAssigner
    m = lc.mixed_batch()
    ta = TargetAssigner(templates, seed=3, ignore=IGNORE if ign else None, **ASSIGNERS[name])
    assert (ta.stats is None) == (name == "plain") and (ta.ignore_stats is None) == (not ign)
    pushed = {"match": [], "ignored": []}
    for st, key in ((ta.stats, "match"), (ta.ignore_stats, "ignored")):
        if st is not None:
            st.push = lambda t, key=key, push=st.push: (pushed[key].append(t), push(t))[1]
    for call, (seed, given) in enumerate(((3 * 1000003 + 1, None), (77, 77))):                 # TargetAssigner's own seed of its first call, then one passed in
        want = _list_entry(ops, name, ign, m, templates, seed)
        assert len(want) == 2 + (name != "plain") + ign
        _same(_resident_entry(ops, name, ign, m, templates, seed), want, f"{name} ignore={ign}: resident entry")
        out = (torch.full_like(want[0], float("nan")), torch.full_like(want[1], float("nan")))
        got = _resident_entry(ops, name, ign, m, templates, seed, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        _same(got, want, f"{name} ignore={ign}: resident entry with out=")
        kw = {} if given is None else {"seed": given}
        pair = ta(m["boxes"], paste_boxes=m["paste"], flips=m["flips"], ignore_boxes=_ignore_boxes(m) if ign else None, **kw)
        _same(pair, want[:2], f"{name} ignore={ign}: TargetAssigner call {call + 1}")
        assert ta.calls == call + 1
        # the stats objects have received exactly the counters the ops call returns
        assert len(pushed["match"]) == (call + 1) * (name != "plain") and len(pushed["ignored"]) == (call + 1) * ign
        if name != "plain":
            assert torch.equal(pushed["match"][-1], want[2])
        if ign:
            assert torch.equal(pushed["ignored"][-1], want[-1]) and int(want[-1].sum()) > 0
    # ... and what they pop is those counters summed over the two calls (pushed[...] was held equal to the ops results above)
    if name != "plain":
        below = 1 if name == "atss" else 3
        mcs = pushed["match"]
        assert ta.stats.pop() == (sum(c.numel() for c in mcs), sum(int((c <= 3).sum()) for c in mcs), sum(int((c < below).sum()) for c in mcs))
    if ign:
        ics = pushed["ignored"]
        assert ta.ignore_stats.pop() == (sum(c.numel() for c in ics), sum(int(c.sum()) for c in ics), sum(int((c > 0).sum()) for c in ics))


def test_call_sequences(templates, monkeypatch):
    """Every configuration makes the library calls of its row of the table, in order, and no other: through TargetAssigner, as the loaders do."""
    from tinyfaces import _hip, ops
    from tinyfaces.datasets import TargetAssigner
    m = lc.mixed_batch()
    real = _hip.lib()
    seen = []

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(ops, "lib", lambda: Spy())
    none = [np.zeros((0, 4))] * len(m["boxes"])
    degenerate = [np.array([[40.0, 40.0, 40.0, 90.0]])] * len(m["boxes"])          # dropped like a degenerate face: the batch has no ignore box
    for name in ASSIGNERS:
        for ignore, boxes, extra in ((None, None, []), (IGNORE, _ignore_boxes(m), ["tf_targets_apply_ignore"]),
                                     (IGNORE, none, []), (IGNORE, degenerate, []), (IGNORE, None, [])):
            del seen[:]
            TargetAssigner(templates, seed=3, ignore=ignore, **ASSIGNERS[name])(m["boxes"], paste_boxes=m["paste"], flips=m["flips"], ignore_boxes=boxes)
            assert seen == CALLS[name] + extra, (name, ignore, None if boxes is None else len(boxes[0]))
