"""Fused training engine: one reference training step (tinyfaces/trainer.py:72-87) with no autograd graph,
no per-parameter Python loop and no host sync:

    targets (HIP) -> forward (HIP executor) -> criterion fwd+bwd (HIP) -> backward (HIP executor)
    -> [RCCL all-reduce of the flat gradient, overlapped with the backward pass]
    -> [global gradient norm -> clip coefficient / non-finite verdict, in device memory] -> fused SGD (one launch per group)
       [+ the model EMA of the updated parameters, inside the same launches]

Gradient accumulation (accum_steps = N > 1): the first N - 1 calls of a window stop behind the backward pass and add their gradient into
one more flat buffer (ops.grad_accumulate); the N-th adds that buffer into its own gradient and runs the tail above on the sum.

Data-parallel overlap: the flat gradient is cut along the backward order into buckets of ~`bucket_mb` MB (default 10: heads +
layer3.21-22 first, then THREE layer-3 bottlenecks of 4.46 MB each per bucket (two stay under 10 MB), ..., finally layer1/2 + stem: SURVEY.md 8e asks for
8-12 buckets of ~10 MB in layer 3).  When a bucket's gradients are enqueued the executor calls back with the stream that carries
them (tf_detnet_set_grad_callback, r3; rounds 1-2: an event + a communication stream waiting on it, still available) and that bucket's
all-reduce is issued there, while the remaining bottlenecks are still being differentiated: only the last, small bucket is exposed.

Semantics are those of main.py:67-70 (SGD momentum 0.9, weight decay 5e-4, the 4 learning-rate groups of
model.py:67-87) and of DetectionCriterion (loss.py).  `trainer.train` (autograd + torch.optim) remains the
drop-in path; this engine is what bench.py and the bundled main.py use."""
import ctypes as C
import os

import torch
import torch.distributed as dist

from . import ops, parallel
from ._hip import lib
from .ema import ModelEma


class TrainEngine:
    def __init__(self, model, criterion, lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cuda", bucket_mb=10, native_exchange=None,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=True, accum_steps=1, accum_average=False,
                 optimizer="sgd", betas=(0.9, 0.999), eps=1e-8, deterministic=False):
        """max_grad_norm: clip the global L2 norm of the (rank-averaged) gradient of the trained tensors to this value before the update, as
        torch.nn.utils.clip_grad_norm_ between backward() and optimizer.step() would (tinyfaces/trainer.py:86-87).  skip_nonfinite: a step
        whose gradient norm is NaN or Inf changes neither the parameters nor the momentum (`skipped_steps` counts them; what the FORWARD
        pass of that step wrote -- the running BatchNorm statistics of a batch-statistics step -- stays written).  Both decisions
        are taken and applied on the device: the step stays free of host syncs.  With the defaults (None, False) a step launches exactly
        what it launched before these arguments existed.
        ema_decay: keep an exponential moving average of the weights (`self.ema`, a tinyfaces.ema.ModelEma: torchvision's --model-ema,
        AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))), updated INSIDE the SGD launches of every step from the parameter those launches
        have just computed: one more flat fp32 buffer, no further launch, no host sync; frozen slices never move.  ema_warmup: the decay of
        update t is min(ema_decay, (1 + t) / (10 + t)).  `ema.updates` advances on EVERY step, one the non-finite guard drops included (the
        device leaves the average alone on such a step, but the host cannot know without a sync): the warm-up is indexed by steps taken.
        Data-parallel runs need no collective for it: every rank applies the same update to the same parameters.  None (the default):
        `self.ema` is None, no buffer, no new call.
        accum_steps: one optimizer step covers this many calls of step() (micro-batches), what a torch loop does when it calls
        loss.backward() N times between optimizer.zero_grad() and optimizer.step().  The applied gradient is the SUM over the window, added
        left to right in fp32 -- the loss is a sum over the batch (loss.py:87), so under frozen BatchNorm N micro-batches of B images are
        the step of one batch of N * B images up to summation order; accum_average=True applies the mean instead (the `loss / N` habit),
        folded into the grad_scale the norm and SGD launches take.  Clipping, the guard, the exchange between ranks (one per window, behind
        the last backward pass, not overlapped with it, through torch.distributed) and the model EMA act once per window, on the
        accumulated gradient; BatchNorm running statistics and the loss meters advance with every micro-batch.  One more flat fp32 buffer,
        allocated when first used; fixed for the engine's life.  1 (the default): no buffer, no new call.
        optimizer: "sgd" (the default: nothing new is allocated or launched) or "adamw", torch.optim.AdamW's single-tensor arithmetic
        (include/tinyfaces_hip.h) with `betas` and `eps`; `weight_decay` is then decoupled, `momentum` unused, `flat_m` is exp_avg and
        `flat_v`, one more flat fp32 buffer, exp_avg_sq.  The step counter of the bias correction lives on the device (`adam_state`, an
        ops.AdamState) and does not advance on a step the non-finite guard drops.  The groups, their lr multipliers, the trained segments,
        the fused EMA and the clip state are the ones SGD uses.
        deterministic: every step() runs with the library's deterministic switch on (ops.set_deterministic: unfolded BatchNorm statistic rows,
        the slab forms of the weight gradients -- no floating-point atomics) and puts back what it found, so that a deterministic and a default
        engine can alternate in one process.  The same weights, optimizer state and batches in give the same weights out, bit for bit, per
        process; the loss meters of the soft-margin criterion and the order inside a multi-rank exchange are not covered.  Slower than the
        default step (README).  False (the default): no new call."""
        if not isinstance(deterministic, bool):
            raise ValueError(f"deterministic must be True or False, got {deterministic!r}")
        self.deterministic = deterministic
        self.device = torch.device(device)
        self.model = model.to(self.device).train()
        self.criterion = criterion
        if parallel.is_distributed():
            parallel.broadcast_module(self.model)
        self.flat_p = self.model.flatten_parameters()
        # the engine owns the flat storages from here on: the per-step identity walk over the 571 tensors is skipped (model._sync_tables;
        # anything that moves the module -- .to(), flatten_parameters -- unfreezes it).  TINYFACES_SYNC_TABLES_ALWAYS=1: the walk of rounds 1-3
        self.model._tables_frozen = os.environ.get("TINYFACES_SYNC_TABLES_ALWAYS") is None
        self.flat_m = torch.zeros_like(self.flat_p)
        self.ema = None if ema_decay is None else ModelEma(self.model, ema_decay, warmup=ema_warmup)     # (behind the broadcast: every rank's clone is rank 0's)
        self._ema_weight = None               # float32(1 - d_t) of the step under way: taken once per step, not once per group
        self.groups = self.model.group_ranges()
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        if optimizer not in ("sgd", "adamw"):
            raise ValueError(f"optimizer must be 'sgd' or 'adamw', got {optimizer!r}")
        self.optimizer = optimizer
        if optimizer == "adamw":
            b1, b2 = (float(b) for b in betas)
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
                raise ValueError(f"betas must lie in [0, 1), got {betas!r}")
            if not float(eps) > 0.0:
                raise ValueError(f"eps must be positive, got {eps!r}")
            if os.environ.get("TINYFACES_SGD_PER_BUCKET"):
                raise ValueError("optimizer='adamw' cannot be combined with TINYFACES_SGD_PER_BUCKET: the per-bucket update is an SGD experiment")
            self.betas, self.eps = (b1, b2), float(eps)
            self.flat_v = torch.zeros_like(self.flat_p)          # exp_avg_sq; flat_m is exp_avg
            self.adam_state = ops.AdamState(self.device)
        self.bucket_elems = int(bucket_mb * (1 << 20) // 4)
        self.steps = 0                        # optimizer steps
        self.micro_steps = 0                  # calls of step(): equal to `steps` unless gradients are accumulated
        self.accum_steps = int(accum_steps)
        if self.accum_steps < 1:
            raise ValueError(f"accum_steps must be >= 1, got {accum_steps}")
        self.accum_average = bool(accum_average)
        self._accum = None                    # the accumulator: flat fp32 like flat_m, allocated by the first micro-batch that is not applied
        self._accum_segs = None               # the ranges the open window accumulates over
        self._window = 0                      # micro-batches in the accumulator
        # r6: None = the default rule (_want_native): the library's own RCCL hook when the world is larger than one rank and librccl resolves,
        # the torch.distributed callback otherwise and whenever the native set-up or a native step reports an error
        self.native_exchange = native_exchange
        self.native_fallbacks = 0             # how often the engine left the native exchange (set-up refused / a bucket's collective failed)
        self.skip_allreduce = False          # measurement knob (bench.py): a step without the exchange, to size what the overlap hides
        self._overlap = None
        self._native = None
        # r3 experiment, NEGATIVE, opt-in (TINYFACES_SGD_PER_BUCKET=1): the gradient buckets (and the events the executor records when a
        # bucket is final) also drive the optimizer -- the SGD update of a bucket on the communication stream as soon as the bucket is
        # final (after its all-reduce when data-parallel), beside the rest of the backward pass, instead of over all 42.5 M parameters
        # at the end of the step.  Same numbers bit for bit; 1113-1117 img/s against 1118-1123 at the end (A/B on one box): the update
        # is HBM-bound (850 MB) and takes from the backward pass what it saves at the tail.
        self.sgd_per_bucket = bool(os.environ.get("TINYFACES_SGD_PER_BUCKET"))
        self.skip_nonfinite = bool(skip_nonfinite)
        self._clip_state = None               # ops.ClipState, allocated by the first step that needs it
        self.set_max_grad_norm(max_grad_norm)
        if self._clip_on() and self.sgd_per_bucket:
            raise ValueError("max_grad_norm / skip_nonfinite cannot be combined with TINYFACES_SGD_PER_BUCKET: a bucket cannot be applied "
                             "before the global gradient norm exists")
        if self.accum_steps > 1 and self.sgd_per_bucket:
            raise ValueError("accum_steps > 1 cannot be combined with TINYFACES_SGD_PER_BUCKET: a bucket cannot be applied before the "
                             "window's last micro-batch")
        if parallel.is_distributed() or self.sgd_per_bucket:
            self._setup_overlap()

    # The bottlenecks in executor order (the block ids of the gradient-ready hooks) and the bucket cuts are those of the model's trunk
    # (DetectionModel.trunk: block counts of layers 1-3), read off the flat-gradient segments.  ResNet-101: layer1 0-2, layer2 3-6, layer3 7-29.
    @staticmethod
    def block_names(blocks):
        """["model.layer1.0.", ...]: the state_dict prefix of every bottleneck, in executor order."""
        return tuple(f"model.layer{L + 1}.{i}." for L, n in enumerate(blocks) for i in range(n))

    @staticmethod
    def trunk_of(segments):
        """Block counts of layers 1-3 of the trunk whose parameters `segments` ({state_dict key: (offset, numel)}) holds."""
        counts = [0, 0, 0]
        for k in segments:
            parts = k.split(".")
            if len(parts) > 3 and parts[0] == "model" and parts[1] in ("layer1", "layer2", "layer3"):
                L = int(parts[1][-1]) - 1
                counts[L] = max(counts[L], int(parts[2]) + 1)
        return tuple(counts)

    @staticmethod
    def coarse_first_blocks(blocks):
        """The coarse 4-bucket cut of round 1, kept as an explicit choice (bucket_mb=0): first bottleneck of each bucket in backward order,
        layer 3 in thirds (ResNet-101: 22, 14, 7)."""
        l3, n3 = blocks[0] + blocks[1], blocks[2]
        return (l3 + 2 * n3 // 3, l3 + n3 // 3, l3)

    @classmethod
    def auto_first_blocks(cls, segments, total, bucket_mb):
        """First bottleneck of each bucket (backward order) so that every bucket but the last carries >= bucket_mb MB of fp32
        gradient: walk the bottlenecks from the last one of layer 3 down, close a bucket as soon as it is big enough; layer 1/2 + stem
        (6 MB for ResNet-101) always form the final bucket (event -1 = end of the backward pass)."""
        blocks = cls.trunk_of(segments)
        names, l3 = cls.block_names(blocks), blocks[0] + blocks[1]
        want = bucket_mb * (1 << 20) / 4
        firsts, end = [], total
        for b in range(len(names) - 1, l3 - 1, -1):                   # layer 3 only (ResNet-101: 29 .. 7)
            start = min(o for k, (o, _) in segments.items() if k.startswith(names[b]))
            if end - start >= want:
                firsts.append(b)
                end = start
        if not firsts or firsts[-1] != l3:
            firsts.append(l3)                                           # whatever is left of layer 3
        return tuple(firsts)

    @classmethod
    def bucket_ranges(cls, segments, total, first_blocks=None):
        """[(event block, start, end)] in backward order: bucket k covers the flat-gradient elements of every bottleneck
        >= first_blocks[k] not covered by an earlier bucket (plus the heads for k = 0); the last bucket (block -1 = "end
        of the backward pass") takes the rest (layer1, layer2, stem).  `segments` = DetectionModel._segments
        ({state_dict key: (offset, numel)} in executor order); first_blocks None = the coarse cut of the segments' trunk."""
        blocks = cls.trunk_of(segments)
        names = cls.block_names(blocks)
        if first_blocks is None:
            first_blocks = cls.coarse_first_blocks(blocks)
        ranges, end = [], total
        for b in first_blocks:
            start = min(o for k, (o, _) in segments.items() if k.startswith(names[b]))
            ranges.append((b, start, end))
            end = start
        ranges.append((-1, 0, end))
        return ranges

    def _setup_overlap(self):
        total = self.flat_p.numel()
        firsts = (self.auto_first_blocks(self.model._segments, total, self.bucket_elems * 4 / (1 << 20)) if self.bucket_elems > 0
                  else self.coarse_first_blocks(self.model.trunk))
        ranges = [r for r in self.bucket_ranges(self.model._segments, total, firsts) if r[2] > r[1]]
        events = []
        for _ in ranges:
            ev = torch.cuda.Event()
            ev.record()                                   # materialises the hipEvent_t handle
            events.append(ev)
        blocks = (C.c_int * len(ranges))(*[r[0] for r in ranges])
        handles = (C.c_void_p * len(ranges))(*[int(ev.cuda_event) for ev in events])
        # the events belong to this engine's MODEL: DetectionModel._run_backward hands them to the executor for the duration of its
        # own backward call (r3: no process-wide registration any more, several engines per process are fine)
        self.model._grad_events = (blocks, handles, len(ranges))
        # r3: the all-reduce of a bucket is issued from INSIDE the backward call (tf_detnet_set_grad_callback), under the stream that
        # carries the bucket's last gradient kernel; the process group orders its own stream behind that point.  No communication stream
        # of ours any more (TINYFACES_ALLREDUCE_COMM_STREAM=1 brings the event-waiting stream of rounds 1-2 back).  Checked on one GPU with
        # a 1-rank RCCL group (TINYFACES_FORCE_DIST=1): 1106 img/s against 1124 without the collectives.
        self._use_comm_stream = bool(os.environ.get("TINYFACES_ALLREDUCE_COMM_STREAM")) or bool(os.environ.get("TINYFACES_ALLREDUCE_ON_MAIN"))
        # r4: the NATIVE exchange (TINYFACES_ALLREDUCE_NATIVE=1 / native_exchange=True): the executor's gradient hook is the library's own
        # tf_comm_allreduce_hook -- ncclAllReduce issued from C on the communicator's stream, no Python (no GIL) inside the backward enqueue,
        # the path a maintainer binding only the C ABI gets (include/tinyfaces_hip.h: tf_comm_*).  The communicator's identifier travels
        # through the torch.distributed group that already exists (any backend).  Opt-in: like the torch path it has only ever seen a
        # 1-rank group on hardware (tests/test_gpu_dist.py); the default stays the torch.distributed callback below.
        self._native = None
        if self._want_native() and not self._use_comm_stream and not self.sgd_per_bucket and self.accum_steps == 1:
            self._native = self._setup_native(ranges)
        self._works, self._cb_error, self._ext_streams = [], None, {}
        self._block_range = {r[0]: (r[1], r[2]) for r in ranges}
        self._cb = C.CFUNCTYPE(None, C.c_int, C.c_void_p, C.c_void_p)(self._on_bucket)
        # accum_steps > 1: no gradient-ready hook on any micro-batch, the window's one exchange is issued behind its last backward pass
        self.model._grad_callback = None if self._use_comm_stream or self.accum_steps > 1 else self._cb
        self.model._grad_callback_user = None
        if self._native is not None:          # the C hook + its plan instead of the ctypes callback
            self.model._grad_callback = C.cast(lib().tf_comm_allreduce_hook, C.c_void_p)
            self.model._grad_callback_user = C.cast(C.pointer(self._native["plan"]), C.c_void_p)
        self._overlap = dict(ranges=ranges, events=events, comm=torch.cuda.Stream(device=self.device) if self._use_comm_stream or self.sgd_per_bucket else None,
                             keep=(blocks, handles))

    def _want_native(self):
        """Which exchange (r6).  An explicit choice wins: `native_exchange=True / False`, TINYFACES_ALLREDUCE_NATIVE=1 / 0.
        Otherwise the C hook (ncclAllReduce issued by the library itself, no Python inside the backward enqueue) is the default as soon as there
        is more than one rank; `_setup_native` falls back to the torch.distributed callback when RCCL refuses (no librccl, ranks sharing a
        device, a failing ncclCommInitRank), and every rank takes the same decision."""
        env = os.environ.get("TINYFACES_ALLREDUCE_NATIVE")
        if self.native_exchange is not None:
            return bool(self.native_exchange)
        if env is not None:
            return env not in ("", "0")
        return parallel.is_distributed() and parallel.world_size() > 1

    def _all_ranks_ok(self, ok):
        """The same verdict on every rank: MIN over the torch.distributed group that carried us here (any backend)."""
        if not (dist.is_initialized() and dist.get_world_size() > 1):
            return bool(ok)
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(int(t.item()))

    def _setup_native(self, ranges):
        """The communicator + the hook's plan, or None (= use the torch.distributed callback) when any rank could not set it up."""
        from . import _hip
        explicit = self.native_exchange is True or os.environ.get("TINYFACES_ALLREDUCE_NATIVE") not in (None, "", "0")
        if not self._all_ranks_ok(bool(lib().tf_comm_available())):
            if explicit:
                raise RuntimeError("TINYFACES_ALLREDUCE_NATIVE: librccl.so could not be resolved at run time")
            self.native_fallbacks += 1
            return None
        ident = [bytes(_hip.TF_COMM_ID_BYTES)]
        if parallel.rank() == 0:
            buf = C.create_string_buffer(_hip.TF_COMM_ID_BYTES)
            if lib().tf_comm_unique_id(buf) == 0:
                ident = [buf.raw]
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.broadcast_object_list(ident, src=0)
        comm = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = lib().tf_comm_init(ident[0], parallel.rank(), parallel.world_size(), C.byref(comm)) if any(ident[0]) else -1
        if not self._all_ranks_ok(rc == 0):
            if rc == 0:
                lib().tf_comm_destroy(comm)
            if explicit:
                raise RuntimeError(f"native exchange: tf_comm_init failed on a rank (this rank: rc = {rc})")
            if parallel.rank() == 0:
                print("tinyfaces: the native RCCL exchange could not be set up (tf_comm_init); using the torch.distributed exchange", flush=True)
            self.native_fallbacks += 1
            return None
        n = len(ranges)
        blocks = (C.c_int * n)(*[r[0] for r in ranges])
        start = (C.c_int64 * n)(*[r[1] for r in ranges])
        end = (C.c_int64 * n)(*[r[2] for r in ranges])
        plan = _hip.CommPlan()
        plan.comm, plan.grad_flat, plan.n = comm, self.model._grad_flat_persistent.data_ptr(), n
        plan.blocks, plan.start, plan.end = C.cast(blocks, C.POINTER(C.c_int)), C.cast(start, C.POINTER(C.c_int64)), C.cast(end, C.POINTER(C.c_int64))
        plan.rc, plan.issued = 0, 0
        status = (C.c_int * n)()
        plan.status = C.cast(status, C.POINTER(C.c_int))
        return dict(comm=comm, plan=plan, keep=(blocks, start, end, status), n=n, status=status, ranges=ranges)

    def _on_bucket(self, block, stream_ptr, _user):
        """Called by the executor while it enqueues the backward pass: bucket `block` is final at the tail of `stream_ptr`."""
        try:
            if not (parallel.is_distributed() and not self.skip_allreduce) or self.sgd_per_bucket or self.accum_steps > 1:
                return
            start, end = self._block_range[block]
            g = self.model._grad_flat_persistent
            cur = torch.cuda.current_stream(self.device)
            if (stream_ptr or 0) == cur.cuda_stream:
                self._works.append(dist.all_reduce(g[start:end], op=dist.ReduceOp.SUM, async_op=True))
                return
            ext = self._ext_streams.get(stream_ptr)
            if ext is None:
                ext = self._ext_streams[stream_ptr] = torch.cuda.ExternalStream(stream_ptr, device=self.device)
            with torch.cuda.stream(ext):
                self._works.append(dist.all_reduce(g[start:end], op=dist.ReduceOp.SUM, async_op=True))
        except BaseException as e:       # an exception must not unwind through the C frames of the executor
            self._cb_error = e

    def _leave_native(self):
        """From the C hook back to the ctypes callback (same buckets, same events): after a native step that reported an error."""
        if self._native is not None:
            lib().tf_comm_destroy(self._native["comm"])
            self._native = None
        self.native_fallbacks += 1
        self.model._grad_callback = self._cb
        self.model._grad_callback_user = None

    def _drain_exchange(self):
        """Error path of step(): whatever the gradient hooks issued before the backward call failed is waited for, so that neither the
        communicator's stream nor torch's work objects outlive the step (a peer that did NOT fail is released by the group's timeout)."""
        try:
            if self._native is not None:
                with torch.cuda.device(self.device):
                    lib().tf_comm_join(self._native["comm"], torch.cuda.current_stream(self.device).cuda_stream)
                self._native["plan"].issued, self._native["plan"].rc = 0, 0
            works, self._works = getattr(self, "_works", []), []
            for w in works:
                w.wait()
        except Exception:
            pass

    def close(self):
        """Detach the gradient-ready events from the model (they are owned by this engine: the executor must not record
        handles that are about to be destroyed) and hand the pointer tables back to the per-call identity walk."""
        if getattr(self, "model", None) is not None:
            self.model._tables_frozen = False
        if self._overlap is not None:
            if getattr(self.model, "_grad_events", None) is not None and self.model._grad_events[0] is self._overlap["keep"][0]:
                self.model._grad_events = None
                self.model._grad_callback = None
                self.model._grad_callback_user = None
            if getattr(self, "_native", None) is not None:
                lib().tf_comm_destroy(self._native["comm"])
                self._native = None
            self._overlap = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_lr(self, lr):
        self.lr = lr

    # ---- gradient-norm clipping and the non-finite-step guard ----------------------------------------------------------
    def set_max_grad_norm(self, max_grad_norm):
        """None: no clipping.  Otherwise a positive number, the largest global L2 norm the applied gradient may have."""
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError(f"max_grad_norm must be positive or None, got {max_grad_norm}")
            if getattr(self, "sgd_per_bucket", False):
                raise ValueError("max_grad_norm cannot be combined with TINYFACES_SGD_PER_BUCKET")
        self.max_grad_norm = max_grad_norm
        return self

    def _clip_on(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    @property
    def last_grad_norm(self):
        """Global L2 norm of the gradient the last clipped / guarded step saw (after the average over ranks, before clipping): a 0-d
        float64 DEVICE tensor that shares the state's memory -- reading it synchronises, asking for it does not.  None before such a step."""
        return None if self._clip_state is None else self._clip_state.norm_tensor()

    @property
    def last_clip_coef(self):
        """The coefficient the last clipped step multiplied its gradient with (1: not clipped, 0: skipped).  Synchronises."""
        return None if self._clip_state is None else self._clip_state.coef()

    @property
    def skipped_steps(self):
        """How many steps the non-finite guard has skipped so far (reads the device counter: synchronises)."""
        return 0 if self._clip_state is None else self._clip_state.skipped()

    def _norm_segments(self):
        """The ranges the gradient norm is taken over: _trained_segments(), each extended over the alignment pad of its own slot (the
        backward pass zeroes the pads with the rest of the flat gradient, and the group-wide SGD launch walks them too) and joined where they
        touch -- a 4-aligned table takes the kernel's 16-byte path, and the batch-statistics step needs a handful of ranges instead of one
        per tensor.  The frozen slices in between stay outside."""
        trained = self._trained_segments()
        if getattr(self, "_norm_key", None) is not trained:
            out = []
            for s, e in trained:
                e = (e + 3) // 4 * 4
                if out and out[-1][1] == s:
                    out[-1][1] = e
                else:
                    out.append([s, e])
            self._norm_segs, self._norm_key = [tuple(r) for r in out], trained
        return self._norm_segs

    def _clip_coef(self, gflat, scale):
        """Enqueue norm -> coefficient -> verdict behind the (joined) gradient exchange; `scale` = 1 / world makes it the norm of the
        AVERAGED gradient, what clip_grad_norm_ behind a DDP all-reduce sees.  Every rank computes it from the same summed gradient, so a
        NaN on one rank makes every rank skip the same step without a further collective."""
        if self._clip_state is None:
            self._clip_state = ops.ClipState(gflat.device)
        return ops.grad_clip_coef(gflat, self._norm_segments(), self._clip_state, grad_scale=scale, max_norm=self.max_grad_norm,
                                  skip_nonfinite=self.skip_nonfinite)

    # ---- checkpoint interop with torch.optim.SGD (main.py:67-76,97-102) ------------------------------------------------
    def _group_params(self):
        """[(lr multiplier, [(state_dict key, nn.Parameter)])] in the order of DetectionModel.learnable_parameters
        (model.py:67-87), i.e. the parameter numbering torch.optim.SGD(model.learnable_parameters(lr)) uses."""
        m = self.model
        name_of = {id(p): k for k, p in m.named_parameters()}
        mults = (1.0, 0.1, 1.0, 0.0)
        return [(mult, [(name_of[id(p)], p) for p in g["params"]]) for mult, g in zip(mults, m.learnable_parameters(1.0))]

    def optimizer_state_dict(self, base_lr=None):
        """The engine's SGD state in the format of `torch.optim.SGD(model.learnable_parameters(lr), ...).state_dict()`, so that
        the reference's resume path (`optimizer.load_state_dict(checkpoint['optimizer'])`, main.py:76) accepts a checkpoint
        written by the fused trainer: one `momentum_buffer` per trained parameter (a slice of the flat momentum buffer), the
        four parameter groups with lr / initial_lr (StepLR needs it when constructed with last_epoch >= 0, main.py:81-83)."""
        if self._window:
            raise RuntimeError(f"optimizer_state_dict: {self._window} of {self.accum_steps} micro-batches are accumulated and not applied; "
                               "finish the window first (step(..., apply=True))")
        base_lr = self.lr if base_lr is None else base_lr
        if self.optimizer == "adamw":
            return self._adamw_state_dict(base_lr)          # torch.optim.AdamW's format instead
        seg = self.model._segments
        state, groups, idx = {}, [], 0
        for mult, params in self._group_params():
            ids = []
            for k, p in params:
                if k in seg and mult != 0.0 and self.steps > 0:
                    o, n = seg[k]
                    state[idx] = {"momentum_buffer": self.flat_m[o:o + n].view_as(p).detach().clone().cpu()}
                ids.append(idx)
                idx += 1
            groups.append({"lr": self.lr * mult, "momentum": self.momentum, "dampening": 0, "weight_decay": self.weight_decay,
                           "nesterov": False, "maximize": False, "foreach": None, "differentiable": False, "fused": None,
                           "initial_lr": base_lr * mult, "params": ids})
        return {"state": state, "param_groups": groups}

    def load_optimizer_state_dict(self, sd):
        """Inverse of optimizer_state_dict: also accepts the state_dict of a real torch.optim.SGD built from
        model.learnable_parameters (the reference's own checkpoints, main.py:97-102).  Parameters without a
        momentum_buffer (never stepped, `model.fc.*`, lr-0 upsample) start from zero like torch does."""
        if not sd or not sd.get("param_groups"):
            return False
        theirs = "adamw" if "betas" in sd["param_groups"][0] else "sgd"
        if self.optimizer == "adamw" or theirs == "adamw":
            return self._load_adamw_state_dict(sd, theirs)
        seg = self.model._segments
        flat = [kp for _, params in self._group_params() for kp in params]
        ids = [i for g in sd["param_groups"] for i in g["params"]]
        if len(ids) != len(flat):
            raise ValueError(f"optimizer state has {len(ids)} parameters, the model has {len(flat)}")
        self.flat_m.zero_()
        loaded = 0
        for i, (k, p) in zip(ids, flat):
            st = sd["state"].get(i)
            buf = None if st is None else st.get("momentum_buffer")
            if buf is None or k not in seg:
                continue
            o, n = seg[k]
            if buf.numel() != n:
                raise ValueError(f"momentum_buffer of {k}: {buf.numel()} elements, expected {n}")
            self.flat_m[o:o + n].copy_(buf.reshape(-1).to(self.flat_m.device, torch.float32))
            loaded += 1
        g0 = sd["param_groups"][0]
        self.momentum = float(g0.get("momentum", self.momentum))
        self.weight_decay = float(g0.get("weight_decay", self.weight_decay))
        self.steps = max(self.steps, 1 if loaded else 0)
        return True

    # ---- the same interop with torch.optim.AdamW ----------------------------------------------------------------------
    def _adamw_state_dict(self, base_lr):
        """optimizer_state_dict() under optimizer="adamw": the format of `torch.optim.AdamW(model.learnable_parameters(lr), betas=, eps=,
        weight_decay=).state_dict()` as the installed torch writes it -- the group keys are taken from a real instance -- with `step` (a 0-d
        float32 CPU tensor holding the DEVICE step count, read here and nowhere else), `exp_avg` and `exp_avg_sq` per trained parameter.
        Frozen tensors and the lr-0 group have no state: torch creates state lazily, on the first step with a gradient."""
        keys = torch.optim.AdamW([torch.zeros(1)], lr=1.0, betas=self.betas, eps=self.eps,
                                 weight_decay=self.weight_decay).state_dict()["param_groups"][0]
        seg = self.model._segments
        trained = set(self.model.trainable_parameter_names())
        t = float(self.adam_state.step()) if self.steps > 0 else 0.0
        state, groups, idx = {}, [], 0
        for mult, params in self._group_params():
            ids = []
            for k, p in params:
                if k in seg and k in trained and mult != 0.0 and self.steps > 0:
                    o, n = seg[k]
                    state[idx] = {"step": torch.tensor(t, dtype=torch.float32),
                                  "exp_avg": self.flat_m[o:o + n].view_as(p).detach().clone().cpu(),
                                  "exp_avg_sq": self.flat_v[o:o + n].view_as(p).detach().clone().cpu()}
                ids.append(idx)
                idx += 1
            group = dict(keys)
            group.update(lr=self.lr * mult, initial_lr=base_lr * mult, params=ids)
            groups.append(group)
        return {"state": state, "param_groups": groups}

    def _load_adamw_state_dict(self, sd, theirs):
        """load_optimizer_state_dict() when the engine or the state dict (`theirs`) is AdamW.  Both AdamW: the moments are copied into the flat
        buffers and the device step is set (the bias corrections follow from it at the next step).  One of each: the moments start from
        zero and rank 0 says so -- an SGD momentum buffer is not an exp_avg."""
        self.flat_m.zero_()
        if self.optimizer == "adamw":
            self.flat_v.zero_()
            self.adam_state.set_step(0)
        if theirs != self.optimizer:
            if parallel.rank() == 0 or not parallel.is_distributed():
                print(f"WARNING: the checkpoint holds the state of optimizer {theirs}, this run uses {self.optimizer}: "
                      f"the moments of {self.optimizer} start from zero")
            return True
        seg = self.model._segments
        flat = [kp for _, params in self._group_params() for kp in params]
        ids = [i for g in sd["param_groups"] for i in g["params"]]
        if len(ids) != len(flat):
            raise ValueError(f"optimizer state has {len(ids)} parameters, the model has {len(flat)}")
        loaded, t = 0, 0
        for i, (k, p) in zip(ids, flat):
            st = sd["state"].get(i)
            if st is None or k not in seg or st.get("exp_avg") is None or st.get("exp_avg_sq") is None:
                continue
            o, n = seg[k]
            for name, dst in (("exp_avg", self.flat_m), ("exp_avg_sq", self.flat_v)):
                if st[name].numel() != n:
                    raise ValueError(f"{name} of {k}: {st[name].numel()} elements, expected {n}")
                dst[o:o + n].copy_(st[name].reshape(-1).to(dst.device, torch.float32))
            t = max(t, int(float(st.get("step", 0))))
            loaded += 1
        self.adam_state.set_step(t)
        g0 = sd["param_groups"][0]
        self.betas = tuple(float(b) for b in g0.get("betas", self.betas))
        self.eps = float(g0.get("eps", self.eps))
        self.weight_decay = float(g0.get("weight_decay", self.weight_decay))
        self.steps = max(self.steps, 1 if loaded else 0)
        return True

    def _allreduce(self, gflat):
        """Per bucket: the communication stream waits for the executor's gradient-ready event, then the all-reduce is
        issued from it (RCCL's own stream orders itself after the issuing stream); the compute stream only waits at
        the end.  Without the events (not set up): few large buckets after the whole backward pass."""
        if os.environ.get("TINYFACES_ALLREDUCE_ON_MAIN"):      # diagnostic: no communication stream, one synchronous collective per bucket behind the backward pass
            for (_, start, end) in (self._overlap["ranges"] if self._overlap is not None else [(0, 0, gflat.numel())]):
                dist.all_reduce(gflat[start:end], op=dist.ReduceOp.SUM)
            return
        if self.accum_steps > 1:
            # no hook ran (a window has one exchange, behind its last backward pass): the engine's bucket ranges, issued here and waited for
            ranges = [(start, end) for _, start, end in self._overlap["ranges"]] if self._overlap is not None else [(0, gflat.numel())]
            works = [dist.all_reduce(gflat[start:end], op=dist.ReduceOp.SUM, async_op=True) for start, end in ranges]
            for w in works:
                w.wait()
            return
        if self._native is not None:
            # the collectives were issued by tf_comm_allreduce_hook during the backward call: the training stream waits for the communicator
            nat = self._native
            plan = nat["plan"]
            issued, rc = plan.issued, plan.rc
            status = list(nat["status"])
            plan.issued, plan.rc = 0, 0
            for k in range(nat["n"]):
                nat["status"][k] = 0
            from . import _hip
            with torch.cuda.device(self.device):
                _hip.check(lib().tf_comm_join(nat["comm"], torch.cuda.current_stream(self.device).cuda_stream), "tf_comm_join")
            if rc != 0 or issued != nat["n"]:
                # r6: a bucket whose collective could not be issued (or whose hook never ran) is reduced HERE through torch.distributed, behind the
                # join (the training stream has the whole gradient by now), and the engine leaves the native exchange for good: from the next
                # step on the ctypes callback issues every bucket.  (The hook fails on every rank alike or not at all -- an ncclAllReduce that one
                # rank cannot enqueue leaves its peers waiting in theirs, which only the group's timeout ends.)
                missing = [k for k in range(nat["n"]) if status[k] != 1]
                for k in missing:
                    _, start, end = nat["ranges"][k]
                    dist.all_reduce(gflat[start:end], op=dist.ReduceOp.SUM)
                if parallel.rank() == 0:
                    print(f"tinyfaces: native exchange: {len(missing)} of {nat['n']} gradient buckets were not issued (rc = {rc}); reduced through "
                          "torch.distributed, which carries the exchange from here on", flush=True)
                self._leave_native()
            return
        if self._overlap is not None and not self._use_comm_stream:
            # the collectives were issued by _on_bucket during the backward call: the training stream waits for them here
            works, self._works = self._works, []
            err, self._cb_error = self._cb_error, None
            if err is not None:
                raise err
            if len(works) != len(self._overlap["ranges"]):
                raise RuntimeError(f"data-parallel step: {len(works)} of {len(self._overlap['ranges'])} gradient buckets were reduced")
            for w in works:
                w.wait()
            return
        if self._overlap is not None:
            ov, works = self._overlap, []
            comm, cur = ov["comm"], torch.cuda.current_stream(self.device)
            sync_ops = not os.environ.get("TINYFACES_ALLREDUCE_ASYNC_OPS")
            for (_, start, end), ev in zip(ov["ranges"], ov["events"]):
                with torch.cuda.stream(comm):
                    comm.wait_event(ev)
                    # a SYNCHRONOUS collective issued under the communication stream: ProcessGroupNCCL (torch >= 2.8) launches it on the
                    # current stream, i.e. on `comm` itself, stream-ordered behind the event wait, and the host does not block
                    w = dist.all_reduce(gflat[start:end], op=dist.ReduceOp.SUM, async_op=not sync_ops)
                    if w is not None:
                        works.append(w)
            for w in works:
                w.wait()
            cur.wait_stream(comm)
            return
        works, end = [], gflat.numel()
        while end > 0:
            start = max(0, end - self.bucket_elems)
            works.append(dist.all_reduce(gflat[start:end], op=dist.ReduceOp.SUM, async_op=True))
            end = start
        for w in works:
            w.wait()

    @staticmethod
    def group_slices(groups, start, end):
        """[(a, b, lr multiplier)]: the parts of the flat range [start, end) that belong to a parameter group with a non-zero learning
        rate (model.py:67-87) -- a gradient bucket may straddle group boundaries (layer 3 | score_res3 | score_res4 | upsample)."""
        out = []
        for s, e, mult in groups:
            a, b = max(s, start), min(e, end)
            if mult != 0.0 and b > a:
                out.append((a, b, mult))
        return out

    def _bucket_updates(self, gflat, scale, reduce):
        """Per bucket, on the second stream: wait for the executor's gradient-ready event, all-reduce the bucket (data-parallel), then
        the SGD update of the bucket's parameters -- every (group ∩ bucket) range with the group's lr multiplier (model.py:67-87); the
        compute stream waits for that stream once, at the end of the step.  The masters of a bucket are only read again by the NEXT
        step's weight packing (the backward pass works on the packed copies and has left the bucket's layers when the event fires)."""
        ov = self._overlap
        comm, cur = ov["comm"], torch.cuda.current_stream(self.device)
        works = []
        for (_, start, end), ev in zip(ov["ranges"], ov["events"]):
            with torch.cuda.stream(comm):
                comm.wait_event(ev)
                works.append(dist.all_reduce(gflat[start:end], op=dist.ReduceOp.SUM, async_op=True) if reduce else None)
        for (_, start, end), w in zip(ov["ranges"], works):
            with torch.cuda.stream(comm):
                if w is not None:
                    w.wait()                              # the second stream (not the host, with RCCL) waits for this bucket's sum
                for a, b, mult in self.group_slices(self.groups, start, end):
                    self._sgd(gflat, a, b, mult, scale)
        cur.wait_stream(comm)

    def _trained_segments(self):
        """Frozen BatchNorm: [(start, end)] of the flat buffer that the optimizer touches, ascending -- the segments of
        DetectionModel.trainable_parameter_names(): every tensor that is neither a BatchNorm weight / bias nor a conv weight of a stage
        set_trainable_layers() froze.  The frozen vectors sit in between (the trunk group is ONE range): a plain tf_sgd_step over the group
        would decay them through weight decay although their gradient is zero."""
        key = (id(self.model._segments), self.model.batchnorm_frozen, self.model.trainable_layers)
        if getattr(self, "_trained_key", None) != key:
            seg = self.model._segments
            self._trained = sorted((seg[k][0], seg[k][0] + seg[k][1]) for k in self.model.trainable_parameter_names())
            self._trained_key = key
        return self._trained

    def _sgd(self, gflat, a, b, mult, scale, clip=None):
        """The SGD update of the flat range [a, b) (inside one parameter group, lr multiplier `mult`).  With the model's BatchNorm frozen
        only the trained segments of the range are touched, in one launch per TF_SGD_MAX_SEGMENTS segments (ops.sgd_step_segments).
        clip: the ClipState of this step (_clip_coef) -- the clipped / guarded forms of the same two launches.
        optimizer="adamw": the AdamW launches over the same ranges (ops.adamw_step / ops.adamw_step_segments)."""
        kw = {} if clip is None else {"clip_state": clip}       # (the default step calls the ops exactly as it always did)
        if self.ema is not None:
            kw["ema_weight"] = self._ema_weight
        if self.optimizer == "adamw":
            hyper = (self.lr * mult, self.betas, self.eps, self.weight_decay, scale)
            if not self.model.batchnorm_frozen:
                if self.ema is not None:
                    kw["ema"] = self.ema.flat[a:b]
                ops.adamw_step(self.flat_p[a:b], gflat[a:b], self.flat_m[a:b], self.flat_v[a:b], self.adam_state, *hyper, **kw)
                return
            if self.ema is not None:
                kw["ema"] = self.ema.flat
            segs = [(max(s, a), min(e, b)) for s, e in self._trained_segments() if e > a and s < b]
            ops.adamw_step_segments(self.flat_p, gflat, self.flat_m, self.flat_v, self.adam_state, segs, *hyper, **kw)
            return
        if not self.model.batchnorm_frozen:
            if self.ema is not None:
                kw["ema"] = self.ema.flat[a:b]
            ops.sgd_step(self.flat_p[a:b], gflat[a:b], self.flat_m[a:b], self.lr * mult, self.momentum, self.weight_decay, scale, **kw)
            return
        if self.ema is not None:
            kw["ema"] = self.ema.flat
        segs = [(max(s, a), min(e, b)) for s, e in self._trained_segments() if e > a and s < b]
        ops.sgd_step_segments(self.flat_p, gflat, self.flat_m, segs, self.lr * mult, self.momentum, self.weight_decay, scale, **kw)

    @property
    def pending_micro_batches(self):
        """Micro-batches accumulated and not yet applied (0: no window is open)."""
        return self._window

    def _applies(self, apply):
        """Whether the micro-batch about to run ends its window.  None: when the window is full; True: now; False: never, which the micro-batch
        that would fill the window cannot ask for (a window never holds more than accum_steps micro-batches)."""
        full = self._window + 1 >= self.accum_steps
        if apply is None:
            return full
        if not apply and full:
            raise ValueError(f"step(apply=False): this micro-batch fills the window of accum_steps = {self.accum_steps}; it has to be applied")
        return bool(apply)

    def _accumulate(self, gflat, last):
        """The gradient the backward pass has just left in `gflat` joins the window: STORE / ADD into the accumulator, or, for the window's
        last micro-batch, FINISH -- the accumulator added into `gflat`, where the tail of the step reads it.  Over _norm_segments(): what the
        norm and the update read, pads included."""
        segs = self._norm_segments()
        if self._window == 0:
            if last:
                return                                    # a window of one micro-batch: the plain step, no launch
            if self._accum is None:
                self._accum = torch.empty_like(self.flat_m)      # never read before STORE has written it
            self._accum_segs = segs
        elif segs is not self._accum_segs:
            raise RuntimeError("TrainEngine.step: the trained tensors changed (freeze_batchnorm / set_trainable_layers) while a window of "
                               "accumulated gradients is open")
        mode = ops.ACCUM_FINISH if last else ops.ACCUM_STORE if self._window == 0 else ops.ACCUM_ADD
        ops.grad_accumulate(self._accum, gflat, segs, mode)

    def step(self, x, class_map, regression_map, apply=None):
        """x (B,3,H,W) f32, class_map, regression_map, apply: see _step.  With deterministic=True the library's switch is on for the duration of
        the call and is then put back to what it was."""
        if not self.deterministic:
            return self._step(x, class_map, regression_map, apply)
        prev = ops.set_deterministic(True)
        try:
            return self._step(x, class_map, regression_map, apply)
        finally:
            ops.set_deterministic(prev)

    def step_with_faces(self, x, class_map, regression_map, faces, apply=None):
        """`step` for a criterion with assigner=TaskAligned(...): faces is the ResidentFaces of the batch (tinyfaces/datasets/targets.py), the
        two maps arrive as the base maps and the criterion completes them in place from the forward output before its loss pass (see _step).
        A method of its own: `step` keeps the signature it had."""
        if faces is None:
            raise ValueError("TrainEngine.step_with_faces: faces (the ResidentFaces of the batch) is required; without an assigner call step()")
        if not self.deterministic:
            return self._step(x, class_map, regression_map, apply, faces)
        prev = ops.set_deterministic(True)
        try:
            return self._step(x, class_map, regression_map, apply, faces)
        finally:
            ops.set_deterministic(prev)

    def _step(self, x, class_map, regression_map, apply=None, faces=None):
        """x (B,3,H,W) f32, class_map (B,nt,h,w) f32 (mined in place by the soft-margin criterion; only read with cls_loss="focal" / "qfl"), regression_map (B,4nt,h,w) f32: all on the device.
        Returns the device tensor [sum cls loss, sum reg loss] (float64) without synchronising; with cls_loss="qfl" it has two more elements,
        [..., sum of the quality targets q over the positives, number of positives] (whatever the criterion's _fwd_bwd returns goes to its meters).
        The step follows the model's BatchNorm mode (DetectionModel.freeze_batchnorm): frozen, the forward and backward run the folded-BN
        graph, and the update skips the BatchNorm vectors (no weight decay, no momentum: their momentum buffers stay zero) and, with
        DetectionModel.set_trainable_layers(k < 4), the conv weights of the frozen stages; the bucket plan of the gradient exchange stays
        as it is (frozen ranges are reduced as zeros).
        With max_grad_norm / skip_nonfinite the update is clipped / guarded on the device (see __init__); a skipped step still counts in
        `steps` and still returns its loss.  With ema_decay the same launches also advance `self.ema` (see __init__).
        With accum_steps = N > 1 every call is one micro-batch (`micro_steps`), and the N-th of a window is the optimizer step (`steps`) on
        the sum of the window's gradients.  apply=True: apply now, over the k <= N micro-batches accumulated (the last batch of an epoch);
        apply=False: accumulate only (ValueError on the micro-batch that fills the window); None: apply when the window is full.
        faces: the ResidentFaces of the batch, for a criterion with assigner=TaskAligned(...): the two maps arrive as the base maps and the
        criterion completes them from the forward output, in place, before its loss pass (DetectionCriterion._fwd_bwd)."""
        m, c = self.model, self.criterion
        accumulating = self.accum_steps > 1
        applies = self._applies(apply) if accumulating or apply is not None else True
        m._check_partial_freeze()
        m._sync_tables(x.device)
        out = m._run_forward(x, training=True)
        if faces is None:
            loss2, grad, _ = c._fwd_bwd(out, class_map, regression_map)
        else:
            loss2, grad, _ = c._fwd_bwd(out, class_map, regression_map, faces=faces)
        if self._native is not None:         # (bench.py measures a step without the exchange: the C hook is simply not installed for it)
            m._grad_callback = None if self.skip_allreduce else C.cast(lib().tf_comm_allreduce_hook, C.c_void_p)
            self._native["plan"].issued, self._native["plan"].rc = 0, 0       # a step that raised half-way must not poison the next one
        self._works, self._cb_error = [], None
        try:
            gflat = m._run_backward(x, grad, persistent=True)
        except BaseException:
            self._drain_exchange()               # collectives already queued by the hooks are joined before the error travels on
            raise
        self.micro_steps += 1
        if hasattr(c, "_pending") and (parallel.rank() == 0 or not parallel.is_distributed()):
            c._pending.append((loss2, x.shape[0]))       # only the logging rank ever flushes the meters
        if accumulating:
            self._accumulate(gflat, applies)
            if not applies:
                self._window += 1
                return loss2
        scale = 1.0
        reduce = parallel.is_distributed() and not self.skip_allreduce
        if reduce:
            scale = 1.0 / parallel.world_size()          # average over ranks, folded into the SGD kernel
        if accumulating:
            if self.accum_average:
                scale = scale * (1.0 / (self._window + 1))       # the mean over the micro-batches actually accumulated
            self._window = 0
        if self.ema is not None:
            if self.ema._src is not self.flat_p or m._flat_params is not self.flat_p:
                raise RuntimeError("TrainEngine.step: the model was flattened again after the engine was built; its model EMA would follow a "
                                   "buffer the parameters have left: build a new engine")
            self._ema_weight = self.ema.next_weight()
        if self.sgd_per_bucket and self._overlap is not None:
            self._bucket_updates(gflat, scale, reduce)
        else:
            if reduce:
                self._allreduce(gflat)
            clip = self._clip_coef(gflat, scale) if self._clip_on() else None      # behind the join: the norm of the summed gradient
            if self.optimizer == "adamw":
                ops.adamw_advance(self.adam_state, self.betas, clip)      # once per optimizer step; a skipped step leaves the counter alone
            for s, e, mult in self.groups:
                if mult == 0.0:
                    continue                              # score4_upsample: lr 0 (model.py:84) -> nothing to do
                self._sgd(gflat, s, e, mult, scale, clip)
        self.steps += 1
        return loss2
