"""One training step of the reference's hot loop on one GPU of a data-parallel job.

  forward (conv stack -> projection -> SpecAugment mask -> encoder -> pooling -> AAM/CE head)
  -> hand-written backward -> [RCCL all-reduce of gradient buckets on a side HIP stream, overlapped
  with the rest of backward] -> fused optimiser step (Adam or SGD, optional weight decay and gradient-norm clipping)
  with the schedule's lr / beta1-or-momentum of this step.

Data parallelism is one process per GPU (``torch.distributed``, backend "nccl" == RCCL over xGMI):
every rank holds a full replica, draws its own minibatch, and the only collective is the SUM
all-reduce of the flat gradient buffer, issued bucket by bucket in the order backward finishes them
(ref: PL ``accelerator: ddp``, config/trainer/trainer.yaml:6-12).  The 1/world of the
gradient mean is folded into the Adam kernel.  LayerDrop-skipped layers contribute zero gradients, so
every rank issues identical collectives regardless of its own LayerDrop draws.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import Plan
from .optim import OptimConfig, fused
from .params import ParamStore
from .spec_augment import compute_mask_indices


class GradBucketReducer:
    """What the bucket reducers share (BucketAllReducer below, comm.CAbiBucketAllReducer): which contiguous slice of the
    flat gradient arena each firing bucket covers, and the side stream its collective runs on."""

    def __init__(self, store: ParamStore, world: int, bucket_merge: int):
        self.store, self.world = store, world
        self.ranges, self.members = self.merge_buckets(store.grad_buckets(), bucket_merge)
        self.comm_stream = torch.cuda.Stream() if store.device.type == "cuda" else None
        self.buffer = None         # the arena bucket_ready() reduces; None = store.grad (a trainer that accumulates over
                                   # several micro-batches points it at store.grad_acc)

    @staticmethod
    def merge_buckets(raw: List[Tuple[str, int, int]], bucket_merge: int):
        """Merge neighbouring layer buckets so each collective carries >= ~2 layers (xGMI rings are per-link bound:
        fewer, larger messages; SURVEY 5 "Distributed comm backend").  Returns (ranges: firing bucket -> (start, end),
        members: firing bucket -> raw buckets its collective covers; it fires when the LAST member is final)."""
        ranges, members = {}, {}
        i = 0
        while i < len(raw):
            n, s, e = raw[i]
            j = i
            if n.startswith("layer"):
                while j + 1 < len(raw) and raw[j + 1][0].startswith("layer") and (j - i + 1) < bucket_merge:
                    j += 1
                e = raw[j][2]
            ranges[raw[j][0]] = (s, e)
            members[raw[j][0]] = [raw[k][0] for k in range(i, j + 1)]
            i = j + 1
        return ranges, members

    def ready_slice(self, name: str) -> Optional[torch.Tensor]:
        """The arena slice to all-reduce now that bucket ``name`` is final on the compute stream, with the side stream
        already ordered behind that stream; None when nothing is to be sent (one rank, a bucket that does not fire, an
        empty range)."""
        if self.world == 1 or name not in self.ranges:
            return None
        s, e = self.ranges[name]
        if e <= s:
            return None
        if self.comm_stream is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self.comm_stream.wait_event(ev)
        return (self.buffer if self.buffer is not None else self.store.grad)[s:e]


class BucketAllReducer(GradBucketReducer):
    """All-reduce contiguous slices of the flat gradient buffer on a side stream as they become final."""

    def __init__(self, store: ParamStore, process_group=None, bucket_merge: int = 2):
        import torch.distributed as dist
        self.dist = dist
        self.pg = process_group
        super().__init__(store, dist.get_world_size(process_group) if dist.is_initialized() else 1, bucket_merge)
        self.works = []

    def bucket_ready(self, name: str) -> None:
        view = self.ready_slice(name)
        if view is None:
            return
        with torch.cuda.stream(self.comm_stream):          # (no stream on the CPU / gloo test path: a no-op)
            self.works.append(self.dist.all_reduce(view, op=self.dist.ReduceOp.SUM, group=self.pg, async_op=True))

    def broadcast_parameters(self, root: int = 0, host_counters: Optional[Sequence[int]] = None) -> List[int]:
        """Start-up broadcast (ref: config/trainer/trainer.yaml:6-12 -- PL's DDP wrapper broadcasts the
        module state of rank 0 when it wraps the model): master parameters, optimiser moments and the loss-scale record
        of ``root`` replace every other rank's, then the 16-bit operand copies are rebuilt.  The HOST side of the
        optimiser state travels with them: the store's Adam step counts (bias corrections) and whatever
        ``host_counters`` the caller adds (schedule position, freeze counter) -- returned as ``root`` had them, so that
        a checkpoint loaded on rank 0 only leaves every replica at the same step.  Ranks that have no Adam moments yet
        must not differ from root in that respect (a collective: same tensors on every rank)."""
        extra = [int(c) for c in (host_counters or ())]
        if self.world == 1:
            return extra
        dev = self.store.flat.device
        counts = torch.tensor([len(self.store.replica_state()), len(extra)], device=dev, dtype=torch.int64)
        lo, hi = counts.clone(), counts.clone()
        self.dist.all_reduce(lo, op=self.dist.ReduceOp.MIN, group=self.pg)
        self.dist.all_reduce(hi, op=self.dist.ReduceOp.MAX, group=self.pg)
        if not torch.equal(lo, hi):
            raise RuntimeError("broadcast_parameters: ranks disagree on which state tensors exist (optimiser moments / "
                               "loss scale / host counters); create or load them on every rank first")
        src = self.dist.get_global_rank(self.pg, root) if self.pg is not None else root
        for t in self.store.replica_state():
            self.dist.broadcast(t, src=src, group=self.pg)
        host = torch.tensor([self.store.step_head, self.store.step_body] + extra, device=dev, dtype=torch.int64)
        self.dist.broadcast(host, src=src, group=self.pg)
        host = [int(v) for v in host.tolist()]
        self.store.set_step_counts(host[0], host[1])
        self.store.sync_lowp()
        return host[2:]

    def wait(self) -> None:
        for w in self.works:
            w.wait()                      # makes the current (compute) stream wait for the collective
        self.works = []
        if self.comm_stream is not None and self.world > 1:
            torch.cuda.current_stream().wait_stream(self.comm_stream)


class SpeakerTrainer(fused.WindowedTrainer):
    def __init__(self, store: ParamStore, plan: Plan, schedule, process_group=None, beta2: float = 0.999,
                 eps: float = 1e-8, layerdrop_seed: int = 1234, mask_seed: int = 7, reducer=None,
                 optimizer: Optional[OptimConfig] = None, gradient_clip_val: float = 0.0,
                 accumulate_grad_batches: int = 1, margin_schedule=None):
        """margin_schedule: an ``optim.schedule.MarginSchedule`` (any callable step -> margin) for the AAM head's margin,
        see optim.fused.WindowedTrainer._apply_margin.  reducer: an object with bucket_ready(name) / wait() / world (default: BucketAllReducer over
        torch.distributed; comm.CAbiBucketAllReducer runs the collective through the C ABI alone).
        optimizer: the optimiser description (ref: config/optim/algo/*.yaml); None = Adam with this constructor's
        ``beta2`` / ``eps`` and no weight decay.  The schedule's second value is beta1 under Adam and the momentum under
        SGD (what torch's OneCycleLR cycles for each).  gradient_clip_val: PL's ``trainer.gradient_clip_val`` (global
        norm; 0 = off), applied to the all-reduced, unscaled gradient inside the optimiser launch.
        accumulate_grad_batches: PL's ``trainer.accumulate_grad_batches`` = N (ref: config/trainer/trainer.yaml:33), see
        optim.fused.WindowedTrainer; only the N-th call of a window all-reduces (PL's ``no_sync`` on the others)."""
        assert plan.train
        self.reducer = reducer if reducer is not None else BucketAllReducer(store, process_group)
        super().__init__(store, schedule, optimizer if optimizer is not None else OptimConfig(beta2=beta2, eps=eps),
                         gradient_clip_val, accumulate_grad_batches, self.reducer.world)
        self.plan, self.beta2, self.eps = plan, beta2, eps
        self.margin_schedule = margin_schedule
        if self.accumulate_grad_batches > 1 and self.world > 1:
            if not hasattr(self.reducer, "buffer"):
                raise TypeError("accumulate_grad_batches > 1 on several ranks needs a reducer with a `buffer` attribute "
                                "(the arena bucket_ready() reduces; None = store.grad): this one would all-reduce "
                                "store.grad instead of the accumulated store.grad_acc")
            at = 0
            for s, e in sorted(self.reducer.ranges.values()):
                assert s == at and e >= s, "the reducer's ranges must cover [0, n_train) exactly once"
                at = e
            assert at == store.n_train, "the reducer's ranges must cover [0, n_train) exactly once"
        self._ld_rng = np.random.RandomState(layerdrop_seed)
        self._mask_rng = np.random.RandomState(mask_seed)

    def broadcast_state(self, root: int = 0, host_counters: Optional[Sequence[int]] = None) -> List[int]:
        """Every replica takes ``root``'s parameters, moments, loss scale AND step position (this trainer's ``step`` =
        the lr / beta1 schedule index, the store's Adam step counts, plus the caller's ``host_counters``, returned as
        root had them).  What a rank-0-only checkpoint load needs before the first step."""
        got = self.reducer.broadcast_parameters(root, [self.step] + [int(c) for c in (host_counters or ())])
        self.step = got[0]
        return got[1:]

    def sample_layerdrop(self) -> Tuple[int, ...]:
        """HF:698-709: each layer is skipped with probability ``layerdrop`` (host RNG)."""
        p = self.plan.reg.layerdrop
        if p <= 0:
            return ()
        u = self._ld_rng.rand(self.plan.cfg.num_hidden_layers)
        return tuple(int(i) for i in np.nonzero(u < p)[0])

    def sample_time_mask(self) -> Optional[torch.Tensor]:
        reg, plan = self.plan.reg, self.plan
        if reg.mask_time_prob <= 0 or plan.cls or plan.paired:
            return None
        m = compute_mask_indices((plan.B, plan.T0), reg.mask_time_prob, reg.mask_time_length,
                                 plan.cfg.mask_time_min_masks, rng=self._mask_rng)
        return torch.from_numpy(m.astype(np.uint8)).to(plan.dev, non_blocking=True)

    def sample_feature_mask(self) -> Optional[torch.Tensor]:
        """HF:1294-1304: [B, hidden_size] mask of feature channels, drawn AFTER the time mask from the same stream."""
        reg, plan = self.plan.reg, self.plan
        if reg.mask_feature_prob <= 0 or plan.cls or plan.paired:
            return None
        m = compute_mask_indices((plan.B, plan.cfg.hidden_size), reg.mask_feature_prob, reg.mask_feature_length,
                                 getattr(plan.cfg, "mask_feature_min_masks", 0), rng=self._mask_rng)
        return torch.from_numpy(m.astype(np.uint8)).to(plan.dev, non_blocking=True)

    def train_step_frozen_encoder(self, frozen_plan: Plan, wav: torch.Tensor, label: torch.Tensor, triplets=None,
                                  transcript=None):
        """``triplets``: see train_step.  Step while the whole wav2vec2 network is frozen (ref: wav2vec2_fc.py:339-347 + PL ``freeze()`` =
        requires_grad False AND eval mode): eval-mode forward, head forward/backward, Adam on the head only."""
        store = self.store
        self._apply_margin(frozen_plan)
        if self.accumulate_grad_batches > 1:
            return self._micro_batch_frozen_encoder(frozen_plan, wav, label, triplets=triplets, transcript=transcript)
        store.zero_grad()
        frozen_plan.embed(wav, None, (), self.step)
        loss, softmax = self._head(frozen_plan, label, triplets, transcript)
        self.reducer.bucket_ready("head")
        self.reducer.wait()
        self._optimizer_step(head_only=True)
        self.stepped = True
        return loss, softmax

    def train_step(self, wav: torch.Tensor, label: torch.Tensor, mask: Optional[torch.Tensor] = None,
                   skip_layers: Optional[Sequence[int]] = None, feature_mask: Optional[torch.Tensor] = None,
                   triplets=None, transcript=None):
        """ref: speaker_recognition_module.py:207-220 (_train_step_ce_loss) + PL backward/optimizer step.
        The "letter" head (ref: speech_recognition_module.py:100-116): ``label`` None and ``transcript`` = (targets
        [B, width], target lengths [B], sample counts [B]) on the host, see Plan.head_forward_backward; returns (loss, None).
        Returns (loss, softmax) as device tensors; no host sync.  Triplet heads (store.head "triplet" / "triplet_ce",
        ref: :269-294): ``triplets`` = (pos, neg), the positive and negative batch row of every row
        (heads.sample_triplets); None lets the head draw them from ``label.tolist()`` (heads.TripletHead, the one place
        that draws) -- a host synchronisation when the label is on the device, which a caller that still holds the labels
        on the host avoids by passing them.  "triplet"
        returns (loss, None)."""
        plan, store = self.plan, self.store
        self._apply_margin(plan)
        if skip_layers is None:
            skip_layers = self.sample_layerdrop()
        if mask is None:
            mask = self.sample_time_mask()
        if feature_mask is None:
            feature_mask = self.sample_feature_mask()
        if self.accumulate_grad_batches > 1:
            return self._micro_batch(wav, label, mask, skip_layers, feature_mask, triplets=triplets, transcript=transcript)
        store.zero_grad(tuple(skip_layers) if plan.grouped else None)
        plan.embed(wav, mask, skip_layers, self.step, feature_mask)
        loss, softmax = self._head(plan, label, triplets, transcript)
        plan.backward(on_bucket_ready=self.reducer.bucket_ready)
        self.reducer.wait()
        self._optimizer_step()
        self.stepped = True
        return loss, softmax

    # ------------------------------------------------------------------ accumulate_grad_batches > 1
    # A window is the N consecutive micro-batches of one optimiser step.  Every backward writes store.grad as it always
    # did; the window's sum is kept in store.grad_acc (w2v2_grad_accumulate: the first micro-batch overwrites, so nothing
    # is zeroed), unscaled -- 1 / (world * N) rides in the optimiser's grad_scale, next to the loss scale and the clip
    # coefficient, so the clip sees the averaged gradient as torch's clip_grad_norm_ does.  The loss-scale record is only
    # touched by optimizer_step, i.e. constant over a window like torch's GradScaler between update() calls.
    @staticmethod
    def _head(plan: Plan, label: torch.Tensor, triplets, transcript=None):
        """The head of every step function.  Without triplets the call is ``head_forward_backward(label)``, the form it
        has always had (callers replace that method with one-argument functions of their own)."""
        if transcript is not None:
            return plan.head_forward_backward(label, triplets=triplets, transcript=transcript)
        if triplets is None:
            return plan.head_forward_backward(label)
        return plan.head_forward_backward(label, triplets=triplets)

    def _micro_batch(self, wav, label, mask, skip_layers, feature_mask, triplets=None, transcript=None):
        plan, store, N = self.plan, self.store, self.accumulate_grad_batches
        if store.accum_count > 0 and store.accum_head_only:
            raise RuntimeError("this accumulation window was opened by a frozen-encoder micro-batch; a window cannot mix "
                               "frozen and unfrozen micro-batches (flush() first)")
        last = store.accum_count == N - 1
        store.zero_grad(tuple(skip_layers) if plan.grouped else None)
        plan.embed(wav, mask, skip_layers, self.step * N + store.accum_count, feature_mask)    # a dropout seed per micro-batch
        loss, softmax = self._head(plan, label, triplets, transcript)
        if last and self.world > 1:
            plan.backward(on_bucket_ready=self._accumulate_and_reduce)     # the all-reduce of grad_acc overlaps backward
        else:
            plan.backward()                                                # no collective (PL: no_sync)
            fused.accumulate(store, 0, store.stepped_size())
        store.accum_count += 1
        store.accum_head_only = False
        self.stepped = last
        if last:
            self._close_window()
        return loss, softmax

    def _accumulate_and_reduce(self, name: str) -> None:
        """Bucket callback of a window's last backward: the firing bucket's merged range is final in store.grad -- add it
        into grad_acc on the compute stream, then hand that slice of grad_acc to the reducer."""
        if name in self.reducer.ranges:
            fused.accumulate(self.store, *self.reducer.ranges[name])
            self.reducer.buffer = self.store.grad_acc
        self.reducer.bucket_ready(name)

    def _micro_batch_frozen_encoder(self, frozen_plan: Plan, wav, label, triplets=None, transcript=None):
        store, N = self.store, self.accumulate_grad_batches
        if store.accum_count > 0 and not store.accum_head_only:
            raise RuntimeError("this accumulation window was opened by an unfrozen micro-batch; a window cannot mix frozen "
                               "and unfrozen micro-batches (flush() first)")
        last = store.accum_count == N - 1
        store.zero_grad()
        frozen_plan.embed(wav, None, (), self.step * N + store.accum_count)
        loss, softmax = self._head(frozen_plan, label, triplets, transcript)
        fused.accumulate(store, 0, store.head_size())
        store.accum_count += 1
        store.accum_head_only = True
        self.stepped = last
        if last:
            self._reduce_window()
            self._close_window()
        return loss, softmax

    def _close_window(self) -> None:
        self.reducer.wait()
        super()._close_window(self.store.accum_head_only)

    def _reduce_window(self) -> None:
        """Hand every bucket of the open window's arena (the head's alone when its micro-batches ran with the encoder
        frozen) to the reducer."""
        if self.world > 1:
            self.reducer.buffer = self.store.grad_acc
            for name in (("head",) if self.store.accum_head_only else tuple(self.reducer.ranges)):
                self.reducer.bucket_ready(name)
