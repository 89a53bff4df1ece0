"""Call surface of the reference's tinyfaces/trainer.py (train, save_checkpoint, print_state).

`train` keeps the reference's step order (trainer.py:72-90).  Data-parallel training hides behind
the same signature: when torch.distributed is initialised (one process per GPU, RCCL over xGMI)
gradients are averaged across ranks before optimizer.step() (tinyfaces/parallel.py)."""
from pathlib import Path

import torch

from . import ops, parallel

_LOSS_FMT = "\tloss_cls: {:.6f}\tloss_reg: {:.6f}"


def print_state(idx, epoch, size, loss_cls, loss_reg):
    """One progress line in the reference's format (trainer.py:9-17): training lines carry the epoch, validation lines
    (epoch < 0) do not."""
    head = f"Epoch: [{epoch}][{idx}/{size}]\t" if epoch >= 0 else f"Val: [{idx}/{size}]\t"
    print(head + _LOSS_FMT.format(loss_cls, loss_reg))


def print_quality(idx, epoch, size, loss_fn):
    """One line per logged interval when the criterion trains with the quality focal loss (`cls_loss="qfl"`): the mean IoU of the predicted boxes
    of all positives seen so far with their targets (DetectionCriterion.quality_average), the quantity the scores are trained towards.  The
    meter is fed by the loss meters' own host read, so nothing waits here.  With the other losses, or before a positive was seen: nothing.
    With TaskAligned(aligned_targets=True) the meter holds the mean aligned TARGET of the positives, and the line says so."""
    meter = getattr(loss_fn, "quality_average", None)
    if getattr(loss_fn, "cls_loss", None) != "qfl" or meter is None or meter.num_averaged == 0:
        return
    if getattr(loss_fn, "aligned_targets", False):
        print(f"Epoch: [{epoch}][{idx}/{size}]\tmean aligned target of positives {meter.average:.4f} ({meter.num_averaged} positives)")
        return
    print(f"Epoch: [{epoch}][{idx}/{size}]\tmean IoU of positives {meter.average:.4f} ({meter.num_averaged} positives)")


def print_compensation(idx, epoch, size, dataloader, lag=0):
    """One line per logged interval when the loader's data set runs the scale-compensated matching (`compensation_stats`, datasets/synthetic.py):
    how many faces of the batches read so far the stage looked after.  The counters sit on the device behind the targets of their batch, which
    the loss meters' read has already waited for (`lag` as in DetectionCriterion.flush_meters).  Without the stage: nothing."""
    stats = getattr(getattr(dataloader, "dataset", None), "compensation_stats", None)
    if stats is None:
        return
    got = stats.pop(lag)
    if got is not None:
        faces, at_most, below = got
        if getattr(stats, "atss", False):                 # the ATSS assigner pushes its match counts into the same object
            print(f"Epoch: [{epoch}][{idx}/{size}]\t{getattr(stats, 'label', 'ATSS')}: {at_most} of {faces} faces won at most {stats.n} positives, {below} of them none")
            return
        print(f"Epoch: [{epoch}][{idx}/{size}]\tanchor compensation: {at_most} of {faces} faces hold at most N = {stats.n} positives after the stage, "
              f"{below} of them fewer (their candidates ran out)")


def print_ignore(idx, epoch, size, dataloader, lag=0):
    """One line per logged interval when the loader's data set applies ignore regions (`ignore_stats`, datasets/synthetic.py: IgnoreStats): the
    mean number of anchors turned from negative to ignored per image, and the share of images with any.  Read like `print_compensation`,
    behind the loss meters' own host read.  Without the feature: nothing."""
    stats = getattr(getattr(dataloader, "dataset", None), "ignore_stats", None)
    if stats is None:
        return
    got = stats.pop(lag)
    if got is not None:
        images, turned, with_any = got
        print(f"Epoch: [{epoch}][{idx}/{size}]\tignore regions: {turned / images:.1f} anchors per image turned from negative to ignored, "
              f"{100.0 * with_any / images:.0f} % of {images} images with any")


def save_checkpoint(state, filename="checkpoint.pth", save_path="weights"):
    """trainer.py:20-26: `state` goes to <save_path>/<filename>; the directory is created on first use."""
    target = Path(save_path)
    target.mkdir(exist_ok=True)
    torch.save(state, str(target / filename))


def _is_logging_rank():
    return parallel.rank() == 0 or not parallel.is_distributed()


def warmup_factor(step, iters, factor):
    """Linear learning-rate warm-up in closed form: factor + (1 - factor) * min(step, iters) / iters for the optimizer step `step` (0-based,
    counted from the start of training), 1 when iters is 0 (off).  torch.optim.lr_scheduler.LinearLR(start_factor=factor,
    total_iters=iters) after `step` calls of its step(); a resumed run lands on the same value."""
    iters, factor = int(iters), float(factor)
    if iters < 0:
        raise ValueError(f"warm-up iterations must be >= 0, got {iters}")
    if not 0.0 < factor <= 1.0:
        raise ValueError(f"warm-up factor must lie in (0, 1], got {factor}")
    if iters == 0:
        return 1.0
    return factor + (1.0 - factor) * min(int(step), iters) / iters


def train(model, loss_fn, optimizer, dataloader, epoch, device, max_grad_norm=None, skip_nonfinite=False, ema=None, accum_steps=1,
          accum_average=False, warmup=None, deterministic=False):
    """One epoch with the reference's step order (trainer.py:68-90): forward, criterion, zero_grad, backward, [all-reduce],
    optimizer step, progress line.

    max_grad_norm / skip_nonfinite (keyword additions behind the reference's signature): ops.clip_grad_norm_ over the gradients of the
    optimizer's parameters between the averaging and optimizer.step(), the spot torch.nn.utils.clip_grad_norm_ takes in a training loop
    (trainer.py:86-87), without a host round trip.  skip_nonfinite alone (max_grad_norm None) only guards.  On a step the guard skips the
    gradient is scaled to ZERO, and torch.optim.SGD still applies weight decay and momentum to the parameters: that is what torch's
    optimizer does with a zero gradient.  Only the fused engine (TrainEngine(skip_nonfinite=True)) leaves a skipped step untouched.
    Under torch.optim.AdamW a zero gradient likewise still decays the weights and moves them along exp_avg (and advances `step`).

    ema (a tinyfaces.ema.ModelEma of `model`): ema.update() right behind optimizer.step(), the spot of AveragedModel.update_parameters in a
    torch training loop -- one launch per 128 trained tensors on the device, no host sync.

    accum_steps = N > 1: one optimizer step per window of N batches.  zero_grad() runs at the start of a window only, so autograd sums the
    window's gradients in `.grad`; the window ends when it is full or with the loader's last batch, and only there follow the averaging over
    ranks, the 1 / k scaling of accum_average (k batches in the window: the mean instead of the sum), the clip, optimizer.step() and
    ema.update(), in that order.  With the default the loop is the one above, call for call.

    warmup = (N, F, first_T): linear learning-rate warm-up.  Before the k-th optimizer.step() of this call every group's lr is set to the lr
    this call found there times warmup_factor(first_T + k, N, F); the found values are put back at the end (the epoch scheduler goes on
    from them).  first_T is the global index of this epoch's first optimizer step.  None or N = 0: the groups are not touched.

    A batch of four elements (a loader with assigner="tal") hands its fourth, the ResidentFaces record, to `loss_fn(..., faces=)`.

    deterministic: the library's deterministic switch (ops.set_deterministic) is on for the duration of the call and put back at its end: the
    native forward and backward under autograd then run without floating-point atomics (what torch's own optimizer and losses do is theirs).
    False (the default): no new call."""
    if not isinstance(deterministic, bool):
        raise ValueError(f"deterministic must be True or False, got {deterministic!r}")
    net = model.to(device).train()
    reducer = parallel.reducer_for(net)
    n_batches = len(dataloader)
    clip = max_grad_norm is not None or skip_nonfinite
    if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
        raise ValueError(f"max_grad_norm must be positive or None, got {max_grad_norm}")
    accum_steps = int(accum_steps)
    if accum_steps < 1:
        raise ValueError(f"accum_steps must be >= 1, got {accum_steps}")
    average = bool(accum_average) and accum_steps > 1
    clipped = [p for g in optimizer.param_groups for p in g["params"]] if clip or average else None
    window = 0                                  # batches whose gradients `.grad` holds
    found = [g["lr"] for g in optimizer.param_groups] if warmup is not None and int(warmup[0]) > 0 else None
    applied = 0                                 # optimizer steps taken by this call
    det_prev = ops.set_deterministic(True) if deterministic else None
    try:
        for step, batch in enumerate(dataloader):
            image, cls_target, reg_target = (t.float().to(device, non_blocking=True) for t in batch[:3])
            if len(batch) > 3:                  # a loader with assigner="tal": the resident faces travel as they are; the criterion assigns
                loss = loss_fn(net(image), cls_target, reg_target, faces=batch[3].to(device, non_blocking=True))
            else:
                loss = loss_fn(net(image), cls_target, reg_target)
            if window == 0:
                optimizer.zero_grad()
            loss.backward()
            window += 1
            if window == accum_steps or step + 1 == n_batches:
                if reducer is not None:
                    reducer.average_gradients()
                if average and window > 1:
                    torch._foreach_mul_([p.grad for p in clipped if p.grad is not None], 1.0 / window)      # (this path's update is torch's own, too)
                if clip:
                    ops.clip_grad_norm_(clipped, float("inf") if max_grad_norm is None else max_grad_norm, skip_nonfinite=skip_nonfinite)
                if found is not None:
                    factor = warmup_factor(int(warmup[2]) + applied, warmup[0], warmup[1])
                    for g, lr in zip(optimizer.param_groups, found):
                        g["lr"] = lr * factor
                optimizer.step()
                applied += 1
                if ema is not None:
                    ema.update()
                window = 0
            if _is_logging_rank():
                flush = getattr(loss_fn, "flush_meters", None)
                if flush is not None:
                    flush()
                print_state(step, epoch, n_batches, loss_fn.class_average.average, loss_fn.reg_average.average)
                print_quality(step, epoch, n_batches, loss_fn)
                print_compensation(step, epoch, n_batches, dataloader)
                print_ignore(step, epoch, n_batches, dataloader)
            elif getattr(loss_fn, "_pending", None):
                loss_fn._pending.clear()            # lazy meters are only ever read on the logging rank: do not pin device scalars elsewhere
    finally:
        if deterministic:
            ops.set_deterministic(det_prev)
        if found is not None:
            for g, lr in zip(optimizer.param_groups, found):
                g["lr"] = lr
