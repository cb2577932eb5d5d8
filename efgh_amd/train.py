"""Training step around the hot path (reference iterater.py:35-43, main.py:127,181-183):
forward -> efghloss -> backward -> gradient all-reduce over RCCL -> fused Adam.

One process per GPU.  All parameters (and their gradients) are views into ONE flat fp32 buffer each,
so the data-parallel exchange is a bucketed all-reduce of 191 MB whose buckets are launched from
parameter hooks while backward is still running, and the optimizer is one kernel launch instead of 353.
`DataParallel` semantics (one loss over the global batch, batch-mean terms) == mean of the per-rank
gradients for equal per-rank batches."""
import contextlib
import os

import torch
import torch.distributed as dist

from . import _C, ops


class FlatParams:
    """Re-homes every parameter of `model` (and its .grad) inside flat buffers, keeping names/shapes."""

    def __init__(self, model):
        self.frozen = tuple(bool(p.requires_grad) for p in model.parameters())      # checked by Trainer.step
        self.all_params = list(model.parameters())
        ps = [p for p in model.parameters() if p.requires_grad]
        bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)
               and m.num_batches_tracked is not None]
        self._home(ps, bns)

    @classmethod
    def from_params(cls, params):
        """the same flat buffers over a plain list of parameters, in that order (optim.Adam: there is no model, so BatchNorm's
        counters stay in their modules and `frozen` / `all_params` describe the list alone)"""
        ps = list(params)
        if not ps:
            raise _C.EfghError('FlatParams.from_params: no parameters')
        seen = set()
        for i, p in enumerate(ps):
            if not torch.is_tensor(p) or p.dtype != torch.float32 or p.device != ps[0].device or not p.requires_grad \
                    or not p.is_leaf:
                raise _C.EfghError('FlatParams.from_params: parameter %d must be a float32 leaf tensor that requires a gradient, on '
                                   '%s (filter frozen parameters out as main.py:178-180 does)' % (i, ps[0].device))
            if id(p) in seen:
                raise _C.EfghError('FlatParams.from_params: parameter %d appears twice' % i)
            seen.add(id(p))
        self = cls.__new__(cls)
        self.frozen, self.all_params = tuple(True for _ in ps), list(ps)
        self._home(ps, [])
        return self

    def _home(self, ps, bns):
        dev, n = ps[0].device, sum(p.numel() for p in ps)
        self.n = n
        self.w = torch.cat([p.data.reshape(-1).float() for p in ps])          # (one launch, not one copy per parameter)
        self.g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.offsets = []
        off = 0
        for p in ps:
            k = p.numel()
            p.data = self.w[off:off + k].view(p.shape)
            p.grad = self.g[off:off + k].view(p.shape)
            self.offsets.append((off, k))
            off += k
        self.params = ps
        # gradients written straight into the flat slices by the layer backward (nets/fn.py `claim_grad`) instead of handed to
        # autograd's AccumulateGrad (which costs an allocation, a copy and an `add` launch per parameter).  `arrived[i]` is set
        # by whichever route delivers parameter i's gradient first; later deliveries in the same step go through autograd and
        # accumulate, so shared parameters keep their meaning.  A direct write OVERWRITES its slice: gradients of several backward
        # calls are summed by draining this buffer into a second one in between (GradAccumulator), not by leaving them here.
        self.direct = True
        # BatchNorm's `num_batches_tracked` counters re-homed as views of ONE int64 vector: a training forward notes which layers
        # ran (GemmLayerFn.forward -> tick) and Trainer.step adds the whole step's counts with one launch instead of one per layer
        self.nbt = torch.stack([m.num_batches_tracked.to(dev) for m in bns]).clone() if bns else None
        self.ticks, self.collect_ticks = [0] * len(bns), False
        self._bns = bns
        for j, m in enumerate(bns):
            m.num_batches_tracked = self.nbt[j]
            m._efgh_nbt = (self, j)
        self.arrived = [False] * len(ps)
        # uses[i]: how many layers of the current forward consume parameter i (nets/fn.py note_use).  A parameter with more than
        # one consumer is never claimed: all of its contributions go through autograd, which sums them and fires the
        # post-accumulate hook once - a direct write by the first consumer (on the weight-gradient stream) would be unordered
        # with the accumulation of the second, and would count the all-reduce bucket down before the second has arrived.
        self.uses = [0] * len(ps)
        self.listeners = []               # callables(index), e.g. the overlapped all-reduce's bucket countdown
        # content epoch of the flat weight buffer (FusedAdam rewrites it through raw pointers): the packed-weight / folded-BN caches
        # of THESE parameters key on it, and their batched repack is registered on it (ops.Epoch)
        self.epoch = ops.Epoch()
        ops.HOLDER_GEN[0] += 1
        for i, p in enumerate(ps):
            p._efgh_flat = (self, i)
            p._efgh_epoch = self.epoch
            p.register_post_accumulate_grad_hook(self._make_hook(i))

    def _make_hook(self, i):
        def hook(param):
            self.deliver(i)
        return hook

    def deliver(self, i, stream=None):
        """parameter i's gradient for this backward pass is (enqueued to be) in the flat buffer; `stream`: the stream the write was
        enqueued on when that is not the current one (weight gradients on the weight-gradient stream, nets/fn.py)"""
        first, self.arrived[i] = not self.arrived[i], True
        if first:
            for fn in self.listeners:
                fn(i, stream)

    def claim(self, p, i):
        """the flat gradient view of parameter i if a backward may overwrite it now (zeroed, nothing delivered yet), else None"""
        if not self.direct or self.arrived[i] or self.uses[i] > 1:
            return None
        return p.grad if self.grad_in_place(i) else None

    def grad_in_place(self, i):
        """parameter i's .grad is still its slice of the flat gradient buffer (autograd replaces .grad when it accumulates)"""
        grad = self.params[i].grad
        return grad is not None and grad.data_ptr() == self.g.data_ptr() + 4 * self.offsets[i][0]

    def rearm(self):
        """before a backward into a zeroed flat gradient: nothing has arrived, every .grad is its flat slice again"""
        self.arrived = [False] * len(self.params)
        for i, (p, (off, k)) in enumerate(zip(self.params, self.offsets)):
            if not self.grad_in_place(i):
                p.grad = self.g[off:off + k].view(p.shape)

    def tick(self, j):
        self.ticks[j] += 1

    def flush_ticks(self):
        self.collect_ticks = False
        if any(self.ticks):
            # a model.to() / .double() / rebinding after the Trainer was built breaks the aliasing of num_batches_tracked with
            # self.nbt silently: count on the module's own buffer then
            base, item = self.nbt.data_ptr(), self.nbt.element_size()
            for j, m in enumerate(self._bns):
                if m.num_batches_tracked.data_ptr() != base + j * item:
                    if self.ticks[j]:
                        m.num_batches_tracked += self.ticks[j]
                    m._efgh_nbt = None
                    self.ticks[j] = 0
            if not any(self.ticks):
                return
            k = self.ticks[0]
            if all(t == k for t in self.ticks):
                self.nbt += k
            else:
                self.nbt += torch.tensor(self.ticks, dtype=self.nbt.dtype).to(self.nbt.device)
            self.ticks = [0] * len(self.ticks)

    def zero_grad(self):
        self.g.zero_()
        self.rearm()


class GradAccumulator:
    """Sum of the flat gradient over the micro-batches of one optimizer step, in a second flat buffer `acc` (same shape and device
    as flat.g, allocated on first use: 191 MB for the full net).  After every micro-batch's backward `drain()` moves flat.g into
    acc - acc = g for the first micro-batch (acc is not read), acc = acc + g after that, one fp32 add per element - and leaves
    flat.g zeroed and re-armed for the next backward, in ONE launch (efgh_grad_drain) and without an aten op.  The 1 / k factor is
    not applied here: the optimizer reads acc with grad_scale = 1 / (k * world).  CPU tensors (the gloo plumbing tests run
    FlatParams on the CPU) take copy_ / add_ / zero_, the same arithmetic."""

    def __init__(self, flat):
        self.flat, self.acc, self.count = flat, None, 0

    def drain(self):
        f = self.flat
        if self.acc is None or self.acc.shape != f.g.shape or self.acc.device != f.g.device:
            self.acc = torch.empty_like(f.g)
        ops.join_side_streams(f.g)                     # weight gradients are written on side streams (see Trainer.step)
        if f.g.is_cuda:
            ops.grad_drain(self.acc, f.g, self.count == 0)
        else:
            if self.count == 0:
                self.acc.copy_(f.g)
            else:
                self.acc.add_(f.g)
            f.g.zero_()
        f.rearm()
        self.count += 1
        return self.count

    def reset(self):
        """ends an optimizer step: the next drain() starts a new sum (acc keeps its contents until then)"""
        self.count = 0


class BnTransaction:
    """The BatchNorm state a training forward writes - running_mean / running_var of every `_BatchNorm` module that tracks running
    statistics (frozen sub-networks included: they update theirs in train mode too) and the num_batches_tracked counters - held so
    that a skipped optimizer step can put it back (Trainer(skip_nonfinite=True, transactional=True)).

    The float buffers are re-homed as views of ONE fp32 vector `live`, as FlatParams re-homes the counters in `flat.nbt`: values
    bit for bit, state_dict names / shapes / order unchanged, and load_state_dict / Trainer.load_checkpoint keep working because
    they copy in place.  Every buffer starts on a 512-byte boundary of `live` (ALIGN elements: the alignment its own allocation
    had, so no kernel that reads it through a raw pointer sees anything new); the padding is zero, is never written and belongs to
    the buffer in front of it.  `shadow_f` / `shadow_c` hold the snapshot, `starts` (device, int64) the buffer starts.

    Per optimizer step: snapshot() before the first forward, probe() after the last one, resolve() between the guard's decision
    and the Adam launch - one HIP launch each (efgh_txn_*), no host read, no aten op.  CPU tensors (the host suite) take plain
    torch operations with the same arithmetic, and the block is a host struct.  snapshot() checks by data_ptr that every view
    still aliases `live` / `flat.nbt`: a model.to() / .double() / rebinding after construction raises EfghError naming the
    buffer - there is no silent fall-back, the point is a guarantee."""
    ALIGN = 128

    def __init__(self, model, flat):
        bns = flat._bns
        if not bns:
            raise _C.EfghError('transactional: the model has no BatchNorm layer that tracks running statistics')
        prefix = {id(m): (name + '.' if name else '') for name, m in model.named_modules()}
        dev = flat.nbt.device
        self.flat, self.bns, self.names, self.slots = flat, bns, [], []
        off = 0
        for m in bns:
            for attr in ('running_mean', 'running_var'):
                b = getattr(m, attr)
                name = prefix[id(m)] + attr
                if not torch.is_tensor(b) or b.dtype != torch.float32 or b.device != dev:
                    raise _C.EfghError('transactional: %s must be a float32 tensor on %s' % (name, dev))
                self.names.append(name)
                self.slots.append((m, attr, off, b.numel()))
                off += -(-b.numel() // self.ALIGN) * self.ALIGN
        self.nf = off
        self.live = torch.zeros(off, dtype=torch.float32, device=dev)
        for m, attr, a, k in self.slots:
            b = getattr(m, attr)
            self.live[a:a + k].copy_(b.detach().reshape(-1))
            setattr(m, attr, self.live[a:a + k].view(b.shape))
        self.shadow_f = torch.zeros_like(self.live)
        self.shadow_c = torch.zeros_like(flat.nbt)
        self._starts = [a for _, _, a, _ in self.slots] + [off]
        self.starts = torch.tensor(self._starts, dtype=torch.int64).to(dev)
        self.cuda = self.live.is_cuda
        # the efgh_txn_state: a device block (FusedAdam re-points it behind its guard block, so that guard_stats() reads both
        # with one copy), or a host struct for CPU tensors
        self.block = torch.zeros(_C.ctypes.sizeof(_C.TxnState), dtype=torch.uint8, device=dev) if self.cuda else None
        self.host = None if self.cuda else _C.TxnState()

    def forward_count(self):
        """txn->forward_nonfinite as a one-element int64 view of the device block (the data-parallel all-reduce's operand)"""
        off = _C.TxnState.forward_nonfinite.offset
        return self.block[off:off + 8].view(torch.int64)

    def check(self):
        base, cbase = self.live.data_ptr(), self.flat.nbt.data_ptr()
        for name, (m, attr, a, k) in zip(self.names, self.slots):
            if getattr(m, attr).data_ptr() != base + 4 * a:
                raise _C.EfghError('transactional: %s no longer aliases the transaction\'s buffer (model.to() / .double() / a '
                                   'rebinding after the Trainer was built): build the Trainer last' % name)
        for j, m in enumerate(self.bns):
            if m.num_batches_tracked.data_ptr() != cbase + 8 * j:
                name = self.names[2 * j].rsplit('running_mean', 1)[0] + 'num_batches_tracked'
                raise _C.EfghError('transactional: %s no longer aliases the flat counter vector (model.to() / a rebinding after '
                                   'the Trainer was built): build the Trainer last' % name)

    def snapshot(self):
        """before the first forward of an optimizer step, on the stream the forward is called on (its side streams fork from
        that stream afterwards, and the previous step joined them): shadow = live, per-step fields cleared"""
        self.check()
        if self.cuda:
            ops.txn_snapshot(self.live, self.shadow_f, self.flat.nbt, self.shadow_c, self.block)
            return
        self.shadow_f.copy_(self.live)
        self.shadow_c.copy_(self.flat.nbt)
        self.host.forward_nonfinite, self.host.first_bad, self.host.vetoed = 0, -1, 0

    def probe(self, losses=None, k=0, stride=1, offset=0):
        """after the last forward, side streams joined: counts the elements of `live` that are inf / NaN now and were finite at the
        snapshot, plus the non-finite ones of the k float32 scalars losses.reshape(-1)[offset + j * stride] (losses contiguous)"""
        if self.cuda:
            ops.txn_probe(self.live, self.shadow_f, self.starts, self.block, losses, k, stride, offset)
            return
        new = ~torch.isfinite(self.live) & torch.isfinite(self.shadow_f)
        count = int(new.sum())
        if count:
            first = int(torch.nonzero(new)[0])
            seg = max(s for s, a in enumerate(self._starts[:-1]) if a <= first)
            self.host.first_bad = seg if self.host.first_bad < 0 else min(self.host.first_bad, seg)
        if k:
            count += int((~torch.isfinite(losses.detach().reshape(-1)[offset:offset + (k - 1) * stride + 1:stride])).sum())
        self.host.forward_nonfinite += count

    def resolve(self, guard=None, betas=(0.9, 0.999), skip=None):
        """between the guard's decision and the Adam launch.  GPU: `guard` is the device block efgh_grad_guard_measure wrote; a
        non-finite forward vetoes the step there.  CPU: `skip` is the guard's own decision (a bool), the final one is returned."""
        if self.cuda:
            ops.txn_resolve(self.live, self.shadow_f, self.flat.nbt, self.shadow_c, guard, self.block, betas[0], betas[1])
            return None
        h = self.host
        if h.forward_nonfinite != 0 and not skip:
            h.vetoed, h.vetoed_total, skip = 1, h.vetoed_total + 1, True
        if skip:
            self.live.copy_(self.shadow_f)
            self.flat.nbt.copy_(self.shadow_c)
            h.rolled_back += 1
        return bool(skip)

    def stats(self, st=None):
        """the four transactional keys of guard_stats() from an efgh_txn_state (None: this object's own block, one device read)"""
        if st is None:
            st = self.host if not self.cuda else _C.TxnState.from_buffer_copy(self.block.cpu().numpy().tobytes())
        named = st.forward_nonfinite != 0 and 0 <= st.first_bad < len(self.names)
        return {'forward_nonfinite': int(st.forward_nonfinite), 'vetoed': int(st.vetoed), 'rolled_back': int(st.rolled_back),
                'first_bad_buffer': self.names[st.first_bad] if named else None}


def split_micro_batches(pc, img, calib, A, gt, k):
    """(pc, img, calib, A, gt) of batch size B -> k tuples of batch size B / k (slices of dimension 0, no copies).  Every entry of
    `gt` must be a tensor or array with leading dimension B."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise _C.EfghError('micro_batches must be an integer >= 1 (or None), got %r' % (k,))
    B = int(pc.shape[0])
    if B % k != 0:
        raise _C.EfghError('micro_batches=%d does not divide the batch size %d' % (k, B))
    for name, t in (('img', img), ('calib', calib), ('A', A)):
        if not hasattr(t, 'shape') or len(t.shape) < 1 or int(t.shape[0]) != B:
            raise _C.EfghError('micro_batches: %s has no leading batch dimension of %d (shape %s)'
                               % (name, B, tuple(getattr(t, 'shape', ()))))
    for name, t in gt.items():
        if not hasattr(t, 'shape') or len(t.shape) < 1 or int(t.shape[0]) != B:
            raise _C.EfghError("micro_batches: gt['%s'] has no leading batch dimension of %d (%s)"
                               % (name, B, 'shape %s' % (tuple(t.shape),) if hasattr(t, 'shape') else type(t).__name__))
    b = B // k
    return [(pc[i * b:(i + 1) * b], img[i * b:(i + 1) * b], calib[i * b:(i + 1) * b], A[i * b:(i + 1) * b],
             {name: t[i * b:(i + 1) * b] for name, t in gt.items()}) for i in range(k)]


def allreduce_mean_(flat_g, world, bucket_elems=8 * 1024 * 1024):
    """sum all-reduce in ~32 MB buckets (fully connected xGMI: large messages, few of them); the 1/world
    factor is folded into the optimizer kernel.  No-op for world == 1."""
    if world <= 1:
        return []
    works = []
    for s in range(0, flat_g.numel(), bucket_elems):
        works.append(dist.all_reduce(flat_g[s:s + bucket_elems], op=dist.ReduceOp.SUM, async_op=True))
    for w in works:
        w.wait()
    return works


class OverlappedAllReduce:
    """Gradient all-reduce overlapped with backward: the flat gradient buffer is cut into ~32 MB buckets of
    whole parameters; every delivered parameter gradient (FlatParams.deliver: from
    autograd's post-accumulate hook or from a layer backward that wrote the flat slice itself) counts its bucket down and launches the bucket's asynchronous
    sum all-reduce (RCCL on its own stream) as soon as the last gradient of the bucket has been written - backward produces
    the gradients back to front, so the tail buckets are on the wire while the front of the network is still being
    differentiated.  `finish()` launches whatever is left (parameters without a gradient) and waits."""

    def __init__(self, flat, world, bucket_elems=8 * 1024 * 1024):
        self.flat, self.world = flat, world
        self.buckets = []                 # [start, end) element ranges of the flat buffer
        self.bucket_of = []               # parameter index -> bucket index
        s = 0
        for i, (off, k) in enumerate(flat.offsets):
            if off + k - s > bucket_elems and off > s:
                self.buckets.append((s, off))
                s = off
            self.bucket_of.append(len(self.buckets))
        self.buckets.append((s, flat.n))
        self.sizes = [0] * len(self.buckets)
        for b in self.bucket_of:
            self.sizes[b] += 1
        self.pending, self.works, self.launched = list(self.sizes), [], [False] * len(self.buckets)
        self.next_b, self.order = len(self.buckets) - 1, []
        self.main_stream = None           # the stream backward() is called on (set by start_step)
        self.written = [[] for _ in self.buckets]         # per bucket: events recorded behind the gradient writes into it
        # set while gradients are accumulated over micro-batches (Trainer.step_accumulated): flat.g then holds ONE micro-batch's
        # gradient, which must not go on the wire - deliveries are ignored and finish() issues nothing
        self.paused = False
        if world > 1:
            flat.listeners.append(self._arrived)

    def _arrived(self, i, stream=None):
        if self.paused:
            return
        b = self.bucket_of[i]
        if self.flat.g.is_cuda:
            # an event right behind the write, on the stream that carries it: the bucket's all-reduce waits for exactly the work
            # that produced its gradients, not for everything else that happens to be enqueued on the branch streams
            ev = torch.cuda.Event()
            ev.record(stream if stream is not None else torch.cuda.current_stream())
            self.written[b].append(ev)
        self.pending[b] -= 1
        self._launch_ready()

    def _launch_ready(self):
        """collectives must be issued in the SAME order on every rank (RCCL matches them by issue order, not by buffer): buckets
        go out strictly from the last to the first - the order backward completes them in - and a bucket that becomes complete
        early waits for its successors, so the order cannot depend on how autograd happens to schedule a rank's hooks"""
        while self.next_b >= 0 and self.pending[self.next_b] <= 0:
            self._launch(self.next_b)
            self.next_b -= 1

    def _launch(self, b):
        if self.launched[b]:
            return
        self.launched[b] = True
        if self.flat.g.is_cuda:
            cur = torch.cuda.current_stream()     # (a hook may run with any branch stream current)
            if self.pending[b] <= 0:
                for ev in self.written[b]:        # every parameter of the bucket was delivered: wait for those writes only
                    cur.wait_event(ev)
            else:                                 # finish(): parameters without a gradient this step - join everything
                for st in ops.side_streams() + ([self.main_stream] if self.main_stream is not None else []):
                    if st != cur:
                        cur.wait_stream(st)
        s, e = self.buckets[b]
        self.order.append(b)
        self.works.append(dist.all_reduce(self.flat.g[s:e], op=dist.ReduceOp.SUM, async_op=True))

    def start_step(self):
        self.main_stream = torch.cuda.current_stream() if self.flat.g.is_cuda else None
        self.pending, self.works, self.launched = list(self.sizes), [], [False] * len(self.buckets)
        self.next_b, self.order = len(self.buckets) - 1, []
        self.written = [[] for _ in self.buckets]

    def finish(self):
        if self.world <= 1 or self.paused:
            return
        for b in range(len(self.buckets) - 1, -1, -1):          # whatever is left (parameters without a gradient), same order
            self._launch(b)
        for w in self.works:
            w.wait()


def _check_real(value, ok, message):
    """None, or a real number (no bool) for which `ok` holds (a NaN fails every comparison) -> None | float"""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not ok(float(value)):
        raise _C.EfghError(message % (value,))
    return float(value)


def check_max_grad_norm(value):
    """`max_grad_norm` of FusedAdam / Trainer: None (no clipping) or a real number > 0 (`inf`: measure only) -> None | float"""
    return _check_real(value, lambda v: v > 0.0, 'max_grad_norm must be a real number > 0 (or None), got %r')


def check_ema_decay(value):
    """`ema_decay` of Trainer / WeightEma: None (no average) or a real number in (0, 1) -> None | float"""
    return _check_real(value, lambda v: 0.0 < v < 1.0, 'ema_decay must be a real number in (0, 1) (or None), got %r')


class WeightEma:
    """Exponential moving average of the trainable weights (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn, over
    the parameters only) in ONE flat fp32 buffer `buf` next to flat.w: 4n bytes more memory (191 MB for the full net).  It starts
    as a copy of flat.w; `update(opt)` is one launch (efgh_ema_update) behind the optimizer's on the same stream, without an aten
    op or a host read:
        t = Adam's step count, d = min(decay, (1 + t) / (10 + t)) (warmup; else d = decay), buf = fma(1 - d, w - buf, buf)
    With a guarded optimizer t and the skip flag are read from its device state block: a skipped step is not averaged and does not
    count towards the warm-up.  CPU tensors (the host suite) take lerp_."""

    def __init__(self, flat, decay, warmup=True):
        self.decay = check_ema_decay(decay)
        if self.decay is None:
            raise _C.EfghError('WeightEma needs ema_decay: a real number in (0, 1)')
        self.flat, self.warmup = flat, bool(warmup)
        self.buf = flat.w.clone()

    def update(self, opt):
        if opt.guarded:
            ops.ema_update(self.buf, self.flat.w, self.decay, self.warmup, 0, opt.state)
        else:
            ops.ema_update(self.buf, self.flat.w, self.decay, self.warmup, opt._t)

    def reset(self):
        """the average becomes a copy of the current weights again (after a load that brought no average of its own)"""
        self.buf.copy_(self.flat.w)

    def views(self):
        """the averaged values of the trainable parameters as views of `buf`, in flat order: [(parameter, view)]"""
        return [(p, self.buf[off:off + k].view(p.shape)) for p, (off, k) in zip(self.flat.params, self.flat.offsets)]


def name_segments(names, sizes, limit=_C.GUARD_MAX_SEGMENTS):
    """segments of a flat parameter buffer for the gradient guard's per-segment norms: the consecutive runs of equal top-level
    module name (`E.bcn1.weight` -> `E`) in flat order, as [(name, start, end)]; one segment `all` when there would be more than
    `limit` runs (or no parameters have names)"""
    segs, off = [], 0
    for name, k in zip(names, sizes):
        top = name.split('.')[0]
        if k > 0:
            if segs and segs[-1][0] == top:
                segs[-1][2] = off + k
            else:
                segs.append([top, off, off + k])
        off += k
    if not segs or len(segs) > limit:
        return [('all', 0, off)]
    return [tuple(s) for s in segs]


def adam_segment_table(sizes, group_of, limit=_C.ADAM_MAX_SEGMENTS):
    """segment table of efgh_adam_step_groups for parameters of `sizes` elements laid out one after the other, parameter i in group
    group_of[i]: (ends, group ids) with adjacent parameters of one group merged and empty parameters dropped - ends strictly
    ascending, the last one the total size"""
    ends, gids, off = [], [], 0
    for k, gi in zip(sizes, group_of):
        off += int(k)
        if k <= 0:
            continue
        if gids and gids[-1] == gi:
            ends[-1] = off
        else:
            ends.append(off)
            gids.append(int(gi))
    if not ends or len(ends) > limit:
        raise _C.EfghError('parameter groups cut the flat buffer into %d segments; 1..%d are supported (order the parameters so '
                           'that those of one group lie together)' % (len(ends), limit))
    return ends, gids


def _group_name(k, group):
    return 'group %d%s' % (k, ' (%s)' % group['name'] if isinstance(group, dict) and group.get('name') else '')


def check_group_value(what, name, value):
    """a group's `lr` / `weight_decay`: anything float() converts (a Python or numpy number, a one-element tensor; no bool) that is
    finite and >= 0 -> float"""
    try:
        v = float(value) if not isinstance(value, bool) else None
    except (TypeError, ValueError):
        v = None
    if v is None or not 0.0 <= v < float('inf'):
        raise _C.EfghError('%s: %s must be a finite real number >= 0, got %r' % (name, what, value))
    return v


def normalize_adam_groups(nparams, groups, lr, weight_decay, betas, eps, decoupled=False):
    """FusedAdam's `groups` -> (param_groups, group_of): plain dicts {'name', 'params', 'lr', 'weight_decay', 'decoupled'} with the
    constructor's values filled in, and the group of every parameter index.  EfghError naming the group for anything refused."""
    groups = list(groups)
    if not 1 <= len(groups) <= _C.ADAM_MAX_GROUPS:
        raise _C.EfghError('%d parameter groups: 1..%d are supported (group %d is one too many)'
                           % (len(groups), _C.ADAM_MAX_GROUPS, _C.ADAM_MAX_GROUPS) if groups else 'no parameter groups')
    group_of, out = [None] * nparams, []
    for k, gr in enumerate(groups):
        name = _group_name(k, gr)
        if not isinstance(gr, dict) or 'params' not in gr:
            raise _C.EfghError("%s: expected a dict with 'params' (indices into flat.params)" % name)
        unknown = set(gr) - {'name', 'params', 'lr', 'weight_decay', 'decoupled', 'betas', 'eps', 'amsgrad', 'maximize'}
        if unknown:
            raise _C.EfghError('%s: unknown keys %s' % (name, sorted(unknown)))
        for flag in ('amsgrad', 'maximize'):
            if gr.get(flag):
                raise _C.EfghError('%s: %s is not supported by the fused step' % (name, flag))
        if 'betas' in gr and tuple(float(b) for b in gr['betas']) != tuple(float(b) for b in betas):
            raise _C.EfghError('%s: betas %r differ from the optimizer\'s %r (betas are shared by all groups)'
                               % (name, tuple(gr['betas']), tuple(betas)))
        if 'eps' in gr and float(gr['eps']) != float(eps):
            raise _C.EfghError('%s: eps %r differs from the optimizer\'s %r (eps is shared by all groups)' % (name, gr['eps'], eps))
        idx = list(gr['params'])
        if not idx:
            raise _C.EfghError('%s is empty' % name)
        for i in idx:
            if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < nparams:
                raise _C.EfghError('%s: %r is not an index into the %d flat parameters' % (name, i, nparams))
            if group_of[i] is not None:
                raise _C.EfghError('%s: parameter %d is in %s already' % (name, i, _group_name(group_of[i], groups[group_of[i]])))
            group_of[i] = k
        out.append({'name': gr.get('name'), 'params': idx,
                    'lr': check_group_value('lr', name, gr.get('lr', lr)),
                    'weight_decay': check_group_value('weight_decay', name, gr.get('weight_decay', weight_decay)),
                    'decoupled': bool(gr.get('decoupled', decoupled))})
    missing = [i for i, k in enumerate(group_of) if k is None]
    if missing:
        raise _C.EfghError('parameter %d is in no group (%d parameters are not: every parameter belongs to exactly one)'
                           % (missing[0], len(missing)))
    return out, group_of


class FusedAdam:
    """torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8, weight_decay) on a FlatParams, one HIP launch.

    Gradient guard (off by default; with both options off `step` is the single efgh_adam_step launch and nothing below exists):
      max_grad_norm   `torch.nn.utils.clip_grad_norm_(params, max_grad_norm)` in front of the update; `float('inf')` measures only
      skip_nonfinite  a step whose gradient holds an inf or NaN leaves weights and moments untouched and does not count as a step
                      (`optimizer.step()` not called); without it non-finite values propagate as in torch
      segments        [(name, start, end)] cutting [0, n) into at most 8 contiguous pieces whose norms are reported separately
      txn             a BnTransaction (needs skip_nonfinite): its resolve launch runs between decide and Adam, so a non-finite forward
                      skips the step too and every skipped step restores BatchNorm's running statistics and counters; its state
                      block lives behind the guard's, and guard_stats() reports both from its one read
    A guarded step is three launches (measure, decide, Adam): the norm, the clip coefficient and the skip decision stay in a
    device-resident state block, nothing is read back.  In a data-parallel run the measure pass sees the all-reduced (summed)
    gradient, which is bit-identical on every rank, so every rank takes the same decision.  `guard_stats()` reads the block.
    With skip_nonfinite the step count `t` lives on the device too (reading `opt.t` costs one device read).

    Parameter groups (`groups=None`, the default: none of the following exists and the launches are those above):
      groups          [{'params': [indices into flat.params], 'lr':, 'weight_decay':, 'decoupled':, 'name':}, ...], at most 16; every
                      key besides `params` is optional and defaults to the constructor's value; every parameter is in exactly one
                      group.  `decoupled` selects torch.optim.AdamW's decay (w *= 1 - lr * weight_decay) for the group.
    With groups the Adam launch of `step` is efgh_adam_step_groups (one launch still; the measure, decide and resolve launches of a
    guarded step are unchanged, and clipping is by the global norm over all groups, as clip_grad_norm_ over all parameters is).
    `opt.param_groups` holds one plain dict per group whose `lr` / `weight_decay` are read at every step: writing
    `param_group['lr']` between steps takes effect at the next launch, nothing is uploaded.  betas and eps are shared by all
    groups BY DESIGN (one pair of moment buffers, one bias correction per step, one step count): a group that asks for its own is
    refused, as are amsgrad and maximize.  The segment table (runs of consecutive parameters of one group) goes to the device once,
    here.
    All three launches share one written-out update (csrc/adam.hip), which rounds m and v twice (a product and a sum, not a fused
    multiply-add) in the last `length & 3` elements of a buffer - and, with groups, of every segment: up to 3 elements per segment
    may differ in the last bit of m and v from an ungrouped FusedAdam over the whole buffer.  (From zero moments the two forms
    coincide: b * 0 is exact.)"""

    def __init__(self, flat, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 skip_nonfinite=False, segments=None, txn=None, groups=None):
        self.max_grad_norm = check_max_grad_norm(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        if txn is not None and not self.skip_nonfinite:
            raise _C.EfghError('a transactional step needs skip_nonfinite=True: only a skipped step is rolled back')
        self.txn = txn
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self.flat, self.lr, self.betas, self.eps, self.wd = flat, lr, betas, eps, weight_decay
        self.m = torch.zeros_like(flat.w)
        self.v = torch.zeros_like(flat.w)
        self._t = 0
        self.segments = self.state = self.workspace = None
        self.param_groups = None
        if groups is not None:
            self.param_groups, self.group_of = normalize_adam_groups(len(flat.params), groups, lr, weight_decay, betas, eps)
            ends, gids = adam_segment_table([k for _, k in flat.offsets], self.group_of)
            self.seg_table = (ends, gids)
            self._seg_ends_host = (_C.c_int64 * len(ends))(*ends)
            self._seg_gids_host = (_C.ctypes.c_uint8 * len(gids))(*gids)
            self._seg_ends = torch.tensor(ends, dtype=torch.int64).to(flat.w.device)
            self._seg_gids = torch.tensor(gids, dtype=torch.uint8).to(flat.w.device)
            self._hp = _C.AdamGroups()
        if self.guarded:
            segs = [(str(a), int(b), int(c)) for a, b, c in segments] if segments is not None else [('all', 0, flat.n)]
            ends = [0] + [c for _, _, c in segs]
            if not (1 <= len(segs) <= _C.GUARD_MAX_SEGMENTS) or ends[-1] != flat.n or \
                    any(b != e0 or c <= b for (_, b, c), e0 in zip(segs, ends)):
                raise _C.EfghError('segments must cut [0, %d) into 1..%d non-empty contiguous pieces in order, got %r'
                                   % (flat.n, _C.GUARD_MAX_SEGMENTS, segs))
            self.segments = segs
            self._bounds = (_C.c_int64 * (len(segs) + 1))(*ends)
            nbytes = _C.lib().efgh_grad_guard_workspace(flat.n)
            if nbytes < 0:
                raise _C.EfghError('the gradient guard handles 1 <= n < 2^31 parameters, got %d' % flat.n)
            nstate = _C.ctypes.sizeof(_C.GuardState)
            self.state = torch.zeros(nstate + (_C.ctypes.sizeof(_C.TxnState) if txn is not None else 0), dtype=torch.uint8,
                                     device=flat.w.device)
            if txn is not None and txn.cuda:
                txn.block = self.state[nstate:]
            self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=flat.w.device)
            self._grad_scale = 1.0

    @property
    def t(self):
        """Adam's step count: a host integer, except with skip_nonfinite, where the device decides which steps count (one read)"""
        if self.skip_nonfinite:
            self._t = int(self._read_state().applied)
        return self._t

    @t.setter
    def t(self, value):
        self._t = int(value)
        if self.skip_nonfinite:
            off = _C.GuardState.applied.offset
            self.state[off:off + 8].view(torch.int64).fill_(self._t)

    def _read_raw(self):
        return self.state.cpu().numpy().tobytes()

    def _read_state(self):
        return _C.GuardState.from_buffer_copy(self._read_raw())

    def guard_stats(self):
        """what the guard saw at the last step and did so far, from ONE device read: applied / skipped step counts, `norm` (global
        2-norm of the gradient as applied, i.e. of the mean gradient over the ranks), `norms` per segment, the clip coefficient
        `coef` and the number of non-finite gradient elements.  With a BnTransaction also `forward_nonfinite` (BatchNorm statistics
        that became non-finite in the last step's forwards + non-finite losses; summed over the ranks), `vetoed` (1: the last step
        was skipped because of the forward alone), `rolled_back` (steps restored so far) and `first_bad_buffer` (state_dict key of
        the first spoiled buffer on THIS rank, or None)"""
        if not self.guarded:
            raise _C.EfghError('guard_stats(): the gradient guard is off (construct with max_grad_norm= and / or skip_nonfinite=True)')
        raw = self._read_raw()
        st = _C.GuardState.from_buffer_copy(raw)
        gs = self._grad_scale
        out = {'applied': int(st.applied), 'skipped': int(st.skipped), 'norm': float(st.norm),
               'norms': {name: float(st.sumsq[i]) ** 0.5 * gs for i, (name, _, _) in enumerate(self.segments)},
               'coef': float(st.coef), 'nonfinite': int(st.nonfinite_total)}
        if self.txn is not None:
            out.update(self.txn.stats(_C.TxnState.from_buffer_copy(raw, _C.ctypes.sizeof(_C.GuardState)) if self.txn.cuda else None))
        return out

    def step(self, grad_scale=1.0, grad=None):
        """`grad`: a flat fp32 buffer to read the gradient from instead of flat.g (GradAccumulator.acc: the sum over the
        micro-batches, with grad_scale = 1 / (micro-batches * world)); None, the default, is flat.g"""
        _C.require_cuda(self.flat.w)
        g = self.flat.g if grad is None else self._check_grad(grad)
        if self.guarded:
            return self._step_guarded(grad_scale, g)
        self.t += 1
        self._launch_adam(g, grad_scale, None)

    def _launch_adam(self, g, grad_scale, state):
        """the step's one Adam launch - grouped, guarded (`state`: the guard's block) or plain - and what follows every one of them"""
        f, lib = self.flat, _C.lib()
        if self.param_groups is not None:
            self._launch_groups(g, grad_scale, state)
        elif state is not None:
            _C.check(lib.efgh_adam_step_guarded(f.w.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), f.n, self.lr,
                                                self.betas[0], self.betas[1], self.eps, self.wd, state.data_ptr(), _C.stream_ptr()))
        else:
            _C.check(lib.efgh_adam_step(_C.ptr(f.w), _C.ptr(g), _C.ptr(self.m), _C.ptr(self.v), f.n, self.lr, self.betas[0],
                                        self.betas[1], self.eps, self.wd, self.t, grad_scale, _C.stream_ptr()))
        # packed-weight / folded-BN caches are stale now (also after a skipped step: the host does not know, a repack is harmless)
        ops.bump_epoch(f.epoch)

    def _launch_groups(self, g, grad_scale, state, grid=0):
        """efgh_adam_step_groups with the groups' values as they are NOW (a host struct passed by value: no upload)"""
        f, hp = self.flat, self._hp
        hp.n_groups, hp.step, hp.grad_scale = len(self.param_groups), self._t, grad_scale
        hp.beta1, hp.beta2, hp.eps = self.betas[0], self.betas[1], self.eps
        for k, gr in enumerate(self.param_groups):
            lr = check_group_value('lr', _group_name(k, gr), gr['lr'])
            wd = check_group_value('weight_decay', _group_name(k, gr), gr['weight_decay'])
            hp.lr[k], hp.weight_decay[k], hp.decoupled[k] = lr, wd, 1 if gr['decoupled'] else 0
            hp.decay[k] = 1.0 - lr * wd             # (float64 product and difference, rounded once by the assignment)
        _C.check(_C.lib().efgh_adam_step_groups(f.w.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), f.n,
                                                self._seg_ends.data_ptr(), self._seg_gids.data_ptr(), len(self._seg_ends_host),
                                                self._seg_ends_host, self._seg_gids_host, _C.ctypes.byref(hp),
                                                state.data_ptr() if state is not None else None, grid, _C.stream_ptr()))

    def _check_grad(self, grad):
        w = self.flat.w
        if not (torch.is_tensor(grad) and grad.dtype == w.dtype and grad.device == w.device and grad.dim() == 1
                and grad.numel() == self.flat.n and grad.is_contiguous()):
            raise _C.EfghError('FusedAdam.step(grad=): expected a contiguous flat float32 buffer of %d elements on %s'
                               % (self.flat.n, w.device))
        return grad

    def _step_guarded(self, grad_scale, g):
        f, lib, stream = self.flat, _C.lib(), _C.stream_ptr()
        if not self.skip_nonfinite:
            self._t += 1                           # (with skip_nonfinite the device counts: a skipped step is not one)
        self._grad_scale = _C.c_float(grad_scale).value      # as the kernels see it (an fp32 argument: 1/3 is not 1/3.0)
        max_norm = self.max_grad_norm if self.max_grad_norm is not None else float('inf')
        _C.check(lib.efgh_grad_guard_measure(g.data_ptr(), f.n, self._bounds, len(self.segments), max_norm, grad_scale,
                                             int(self.skip_nonfinite), self.betas[0], self.betas[1], self._t,
                                             self.workspace.data_ptr(), self.state.data_ptr(), 0, stream))
        if self.txn is not None:                   # veto / restore: after decide, before Adam reads state->skip, same stream
            self.txn.resolve(self.state, self.betas)
        self._launch_adam(g, grad_scale, self.state)


def named_param_groups(names, specs):
    """Trainer's `param_groups` -> FusedAdam's `groups` over the trainable parameters `names` (in flat order): parameter i joins the
    first spec whose 'names' - a list of prefixes, one prefix, or a predicate of the name - matches; the unmatched ones form a
    last, default group (no keys of its own).  A spec nothing matches stays in the list, empty: FusedAdam refuses it by name."""
    specs = list(specs)
    groups = []
    for k, spec in enumerate(specs):
        if not isinstance(spec, dict) or 'names' not in spec:
            raise _C.EfghError("param_groups[%d]: expected a dict with 'names' (prefixes of state_dict names, or a predicate)" % k)
        sel = spec['names']
        label = getattr(sel, '__name__', 'predicate') if callable(sel) else ','.join([sel] if isinstance(sel, str) else list(sel))
        groups.append(dict({key: v for key, v in spec.items() if key != 'names'}, name=spec.get('name', label), params=[]))
    default = []
    for i, name in enumerate(names):
        for spec, group in zip(specs, groups):
            sel = spec['names']
            if sel(name) if callable(sel) else name.startswith((sel,) if isinstance(sel, str) else tuple(sel)):
                group['params'].append(i)
                break
        else:
            default.append(i)
    if default:
        groups.append({'name': 'default', 'params': default})
    return groups


def adjust_learning_rate(base_lr, it, every=50000, gamma=0.7):
    """common/helper.py:28-38"""
    return base_lr * (gamma ** (it // every))


class Trainer:
    """one data-parallel training step; `world`/`rank` from torch.distributed when initialised.

    `max_grad_norm` / `skip_nonfinite` switch on FusedAdam's gradient guard (global-norm clipping, skipping of steps with an inf /
    NaN gradient; both off by default, and then nothing changes).  The guard measures the gradient after `comm.finish()`, i.e. the
    all-reduced sum, which holds the same bits on every rank: all ranks clip by the same coefficient and skip the same steps, so
    no rank waits for another's `optimizer.step()`.  The norms are reported per sub-network (`E`, `H`, `F`, `G`: the runs of
    equal top-level module name in flat parameter order; one segment `all` if there were more than 8).  `step` never reads the
    guard's state; `guard_stats()` does, once per call.

    On its own the guard protects weights, moments and the step count from non-finite GRADIENTS; BatchNorm's running statistics
    and num_batches_tracked have been written by the forward (of every micro-batch) before it runs, and the deferred activations
    can hide a NaN forward from the loss altogether.  `transactional=True` (needs skip_nonfinite=True, off by default: nothing is
    allocated, re-homed or launched then) makes a skipped step all or nothing: the BatchNorm state is snapshotted before the first
    forward (BnTransaction), a probe after the last forward counts running statistics that became inf / NaN and non-finite `total`
    losses - such a step is skipped even when its gradient came out finite - and a skipped step restores statistics and counters,
    for an accumulated step those of ALL its micro-batches.  Three more launches per optimizer step, no host read; with world > 1
    one 8-byte all-reduce of the count, so that every rank takes the same decision and restores its own buffers.  `guard_stats()`
    then also reports `forward_nonfinite`, `vetoed`, `rolled_back` and `first_bad_buffer`.  Only BatchNorm buffers are rolled back.

    `ema_decay` (None, the default: nothing is allocated or launched) keeps an exponential moving average of the trainable weights
    (WeightEma: 4n bytes, one launch per optimizer step right behind Adam; `ema_warmup` ramps the decay as (1 + t) / (10 + t) over
    Adam's step count).  A step the guard skips - a transactional veto included - leaves the average bit-unchanged, decided on the
    device.  The ranks of a data-parallel run average bit-identical weights, so no collective is needed.  `ema_state_dict()` gives
    the model's state_dict with the averaged parameters (BatchNorm buffers and frozen parameters keep their live values);
    `with trainer.ema_weights():` puts the averaged weights under the model in place for validation; save_checkpoint(ema=trainer.ema)
    / load_checkpoint carry the average.

    `param_groups` (None, the default: one set of hyper-parameters, the launches above) gives FusedAdam's parameter groups by name:
    a list of {'names': prefixes or a predicate, 'lr':, 'weight_decay':, 'decoupled':} matched against the state_dict names of the
    trainable parameters - a parameter joins the FIRST entry one of whose prefixes its name starts with (or whose predicate holds);
    those no entry matches form a default group with the Trainer's own `lr` / `weight_decay`.  A lower rate on a pre-trained
    sub-network ({'names': ['G.'], 'lr': 1e-5}) or no decay on BatchNorm and bias is one entry each.  The step schedule multiplies
    every group's own base rate.  betas and eps are shared (see FusedAdam)."""

    def __init__(self, model, criterion, lr=1e-4, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False, transactional=False,
                 ema_decay=None, ema_warmup=True, param_groups=None):
        max_grad_norm = check_max_grad_norm(max_grad_norm)                       # (before anything is re-homed or broadcast)
        ema_decay = check_ema_decay(ema_decay)
        if transactional and not skip_nonfinite:
            raise _C.EfghError('transactional=True needs skip_nonfinite=True: only a skipped step is rolled back')
        self.model, self.criterion = model, criterion
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.flat = FlatParams(model)
        if self.world > 1:                                  # identical start on every rank: trainable, FROZEN and buffers
            dist.broadcast(self.flat.w, 0)
            flat_ids = {id(p) for p in self.flat.params}
            for t in list(model.parameters()) + list(model.buffers()):
                if id(t) not in flat_ids:
                    dist.broadcast(t.data, 0)
        segments = None
        if max_grad_norm is not None or skip_nonfinite:
            names = [k for k, p in model.named_parameters() if p.requires_grad]
            segments = name_segments(names, [k for _, k in self.flat.offsets])
        self.txn = BnTransaction(model, self.flat) if transactional else None     # (after the broadcast: it copies the values)
        groups = None
        if param_groups is not None:
            groups = named_param_groups([k for k, p in model.named_parameters() if p.requires_grad], param_groups)
        self.opt = FusedAdam(self.flat, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                             skip_nonfinite=skip_nonfinite, segments=segments, txn=self.txn, groups=groups)
        # the step schedule multiplies every group's OWN base rate
        self.group_base_lr = [g['lr'] for g in self.opt.param_groups] if groups is not None else None
        self.comm = OverlappedAllReduce(self.flat, self.world)
        if self.world > 1:
            ops.reserve_comm_queue()
        self.base_lr, self.it = lr, 0
        self.accum = None                                   # GradAccumulator of step_accumulated, built on first use
        # (after the broadcast: every rank starts from, and then averages, bit-identical weights)
        self.ema = WeightEma(self.flat, ema_decay, ema_warmup) if ema_decay is not None else None
        self._ema_scope = False

    def _need_ema(self, what):
        if self.ema is None:
            raise _C.EfghError('%s: the weight average is off (construct the Trainer with ema_decay=)' % what)

    def _not_in_ema_scope(self, what):
        if self._ema_scope:
            raise _C.EfghError('%s inside `with trainer.ema_weights():` - the averaged weights are under the model' % what)

    def ema_state_dict(self):
        """model.state_dict() - same names, shapes and order - with the entries of the trainable parameters replaced by clones of
        their averaged values.  Frozen parameters and all buffers keep their live values (BatchNorm's running statistics are
        averages already: AveragedModel's use_buffers=False)."""
        self._need_ema('ema_state_dict()')
        self._not_in_ema_scope('ema_state_dict()')
        sd = self.model.state_dict()
        avg = {id(p): v for p, v in self.ema.views()}
        for name, p in self.model.named_parameters(remove_duplicate=False):
            if id(p) in avg and name in sd:
                sd[name] = avg[id(p)].clone()
        return sd

    def _ema_exchange(self):
        ops.join_side_streams(self.flat.w)                  # a forward's branch streams read the weights too
        ops.ema_swap(self.flat.w, self.ema.buf)
        ops.bump_epoch(self.flat.epoch)                     # packed-weight / folded-BN caches are stale now

    @contextlib.contextmanager
    def ema_weights(self):
        """scope in which the model computes with the averaged weights: flat.w and the average's buffer are exchanged in place (one
        launch, then the content epoch moves so that packed and folded weights are rebuilt) and exchanged back on exit, also after
        an exception.  train() / eval() mode is the caller's business.  `step`, `step_accumulated`, `load_checkpoint` and a nested
        scope raise EfghError inside."""
        self._need_ema('ema_weights()')
        self._not_in_ema_scope('ema_weights()')
        self._ema_exchange()
        self._ema_scope = True
        try:
            yield self
        finally:
            self._ema_scope = False
            self._ema_exchange()

    def guard_stats(self):
        """FusedAdam.guard_stats(): {'applied', 'skipped', 'norm', 'norms': {segment: norm}, 'coef', 'nonfinite'} of the last step
        (with transactional=True also 'forward_nonfinite', 'vetoed', 'rolled_back', 'first_bad_buffer'), from one device read made
        here and nowhere else; EfghError when the guard is off"""
        return self.opt.guard_stats()

    def _probe(self, losses, k, stride, offset=0):
        """the transaction's probe over the k `total` losses of this optimizer step, called by _apply (the step core's comment
        argues why it sits behind the join of the side streams and in front of the resolve launch).  world > 1: the counts are summed
        over the ranks (one 8-byte collective), so that all ranks veto together; each restores its own buffers, `first_bad` stays
        rank-local."""
        _C.require_f32(losses)
        self.txn.probe(losses, k, stride, offset)
        if self.world > 1:
            dist.all_reduce(self.txn.forward_count(), op=dist.ReduceOp.SUM)

    def load_checkpoint(self, ckpt):
        """resume from a checkpoint in the reference's layout (common/helper.py:40-61, main.py:149-160,190-198): model state,
        Adam moments and the iteration counter, so that the step-wise decay 0.7^(iter // 50000) continues where it stopped.
        (The reference re-evaluates the schedule once per iterater() call, iterater.py:21, i.e. per epoch; here it is evaluated
        every step from the same formula - the learning rate changes at iteration 50000*k exactly instead of at the next epoch
        boundary.)  With a weight average: the file's average is restored when it has one (EfghError on a name or shape mismatch; the
        decay and warm-up stay the Trainer's own), otherwise the average restarts as a copy of the loaded weights."""
        from .io import checkpoint as ck
        self._not_in_ema_scope('load_checkpoint')
        if isinstance(ckpt, (str, bytes)) or hasattr(ckpt, '__fspath__'):
            ckpt = torch.load(ckpt, map_location='cpu')
        has_ema = self.ema is not None and isinstance(ckpt, dict) and 'ema' in ckpt
        if has_ema:
            ck.check_ema_state(self.ema, self.model, ckpt['ema'])       # (before anything is written)
        ck.load_model_state(self.model, ckpt)
        if 'optimizer' in ckpt:
            ck.load_adam_state(self.opt, ckpt['optimizer'])
        if has_ema:
            ck.load_ema_state(self.ema, self.model, ckpt['ema'])
        elif self.ema is not None:
            self.ema.reset()                  # (it would still describe the weights from before the load)
        self.it = int(ckpt.get('iter', -1)) + 1
        ops.bump_epoch(self.flat.epoch)
        ops.bump_epoch()
        return self.it

    def _check_frozen(self):
        if tuple(bool(p.requires_grad) for p in self.flat.all_params) != self.flat.frozen:
            raise _C.EfghError('the set of trainable parameters changed after the Trainer was built (FlatParams snapshots '
                               'requires_grad): freeze parameters first, then construct the Trainer')

    def _raw_size(self):
        """(H, W) of the raw camera image: the criterion's, or - behind a wrapper that does not forward attributes - the model's"""
        for owner in [self.criterion] + list(self.model.modules()):
            raw = getattr(owner, 'raw_cam_img_size', None)
            if raw is not None:
                return int(raw[0]), int(raw[1])
        raise _C.EfghError('step_accumulated(exact_depth_mean=True) needs raw_cam_img_size on the criterion or the model')

    def depth_weights(self, micro_batches):
        """g_depth weights of the micro-batches, w_i = n_i / mean(n) over all micro-batches (and ranks), as an fp32 device vector
        [k]; 1 everywhere when no pixel is valid at all.  n_i, the valid pixels of micro-batch i, depends on its inputs only (point
        cloud, cam_T_velo, img_mask): the ground-truth depth image is rasterised here as compute_loss will rasterise it, and
        counted by efgh_gimg_valid_count into one int64 vector - all-reduced once when world > 1.  Nothing is read back."""
        rawH, rawW = self._raw_size()
        dev = self.flat.w.device
        counts = torch.zeros(len(micro_batches), dtype=torch.int64, device=dev)
        with torch.no_grad():
            for i, (pc, _img, _calib, _A, gt) in enumerate(micro_batches):
                gdep, _ = ops.depth_image(pc, torch.as_tensor(gt['cam_T_velo']).to(dev).float(), rawH, rawW)
                imask = torch.as_tensor(gt['img_mask']).to(dev).to(torch.uint8).contiguous()
                ops.gimg_valid_count(gdep, imask, counts[i:i + 1])
                del gdep, imask
            total = counts
            if self.world > 1:                         # one small all-reduce per optimizer step (element i: micro-batch i of every rank)
                total = counts.clone()
                dist.all_reduce(total, op=dist.ReduceOp.SUM)
            # float64 on the device (counts are exact there), ONE rounding to fp32; the zero-mean rule of _dp_weight_masked_mean
            n = counts.double()
            mean = total.sum().double() / float(len(micro_batches) * self.world)
            w = torch.where(mean > 0, n / mean.clamp_min(1e-300), torch.ones_like(n))
        return w.float()

    # ---- the step core: `step` and `step_accumulated` are _begin, k x (_forward_loss, backward, join), _apply, and differ only in
    # where the gradient lives (flat.g / the accumulator) and when it goes on the wire (from the hooks during backward / once after
    # the last drain).  Ordering, all on the current stream: _begin enqueues the snapshot before any forward forks its branch streams
    # (BatchNorm statistics are written there too; the forward joins its branches before it returns what depends on them); after
    # every backward the current stream waits for EVERY side stream (ops.join_side_streams: in `step`, and at the head of drain());
    # _apply enqueues the probe behind that join, the resolve launch (inside opt.step, between decide and Adam) behind the probe,
    # the average behind Adam - and the next _begin's snapshot behind them all.
    def _begin(self, what, depth_weights_of=None):
        """checks, learning rate, train mode, the g_depth weights of the micro-batches `depth_weights_of` (if any; returned), and
        then the transaction's ONE snapshot of this optimizer step"""
        self._not_in_ema_scope(what)
        self._check_frozen()
        self.opt.lr = adjust_learning_rate(self.base_lr, self.it)
        if self.group_base_lr is not None:
            for group, base in zip(self.opt.param_groups, self.group_base_lr):
                group['lr'] = adjust_learning_rate(base, self.it)
        self.model.train()
        weights = self.depth_weights(depth_weights_of) if depth_weights_of is not None else None
        if self.txn is not None:
            self.txn.snapshot()               # on the current stream, before the forward forks its branch streams from it
        return weights

    def _forward_loss(self, pc, img, calib, A, gt, depth_weight=None):
        """forward and loss of one (micro-)batch -> (losses, gt, pred) as the criterion and the model return them"""
        self.flat.uses = [0] * len(self.flat.params)
        self.flat.collect_ticks = True
        try:
            pred = self.model(pc, img, calib, A)
        finally:
            self.flat.flush_ticks()
        ops.TLS.depth_weight = depth_weight
        try:
            losses, gt = self.criterion.compute_loss(pc, img, calib, A, gt, pred)
        finally:
            ops.TLS.depth_weight = None
        return losses, gt, pred

    def _apply(self, k, totals, grad=None):
        """probe, Adam, average and `it` for the gradient of k (micro-)batches.  `totals`: (tensor, stride, offset) of the k `total`
        losses, read only with a transaction.  `grad`: the accumulator, all-reduced here, or None: flat.g, which `comm` reduced"""
        if self.txn is not None:
            self._probe(totals[0], k, totals[1], totals[2])
        if grad is not None:
            allreduce_mean_(grad, self.world)
        self.opt.step(grad_scale=1.0 / (k * self.world), grad=grad)
        if self.ema is not None:
            self.ema.update(self.opt)         # right behind Adam on the same stream; reads the guard's skip decision there
        self.it += 1

    def step(self, pc, img, calib, A, gt, micro_batches=None):
        """one optimizer step on one batch, through the step core (the comment above `_begin` argues its order).  `micro_batches=k`:
        the batch is cut into k equal chunks along dimension 0 whose gradients are accumulated (step_accumulated): the activation
        memory of B / k samples, the update of B."""
        if micro_batches is not None:
            return self.step_accumulated(split_micro_batches(pc, img, calib, A, gt, micro_batches))
        self._begin('step')
        losses, gt, pred = self._forward_loss(pc, img, calib, A, gt)
        self.flat.zero_grad()
        self.comm.start_step()
        losses['total'].backward()            # bucket all-reduces start from the parameter hooks during this call
        # the point branch runs on a side stream (nets/efghbackbone.py) and so does its backward; autograd joins the streams of the
        # AccumulateGrad nodes it ran, but gradients written directly into the flat buffer have no such node: join explicitly
        ops.join_side_streams(self.flat.g)
        self.comm.finish()
        self._apply(1, (losses['total'], 1, 0))
        return losses, pred

    def step_accumulated(self, micro_batches, exact_depth_mean=True):
        """ONE optimizer step on the gradient accumulated over k >= 1 micro-batches, a sequence of (pc, img, calib, A, gt) tuples
        of equal batch size, through the step core of `step` (ordering: the comment above `_begin`): per micro-batch forward, loss
        and backward into the zeroed flat gradient, then GradAccumulator.drain(); each micro-batch's graph is gone before the next
        forward, so the activation memory is that of ONE micro-batch.  After the last drain the sum is all-reduced once (world > 1;
        not overlapped with backward - the bucket listeners are paused meanwhile) and read with grad_scale = 1 / (k * world).

        The meaning is that of k data-parallel ranks (`torch.nn.DataParallel` replicas): one loss over the global batch, BatchNorm
        statistics per micro-batch.  Every term of efghloss is a batch mean except g_depth, a mean over the valid pixels of the
        whole batch: with `exact_depth_mean` micro-batch i's term is weighted by n_i / mean(n) (depth_weights: counted on the
        device before the first forward, no host read); False takes the plain mean of the micro-batch losses.

        Once per call: `it`, the learning-rate schedule and Adam's step count advance.  Per micro-batch, as torch would: BatchNorm's
        running statistics and num_batches_tracked.  With skip_nonfinite a non-finite value in any micro-batch's gradient reaches
        the sum and the whole accumulated step is skipped.  With transactional=True a skipped step - a non-finite gradient, loss
        or BatchNorm statistic in ANY micro-batch - also undoes what ALL k micro-batches did to the running statistics and counters.
        -> (losses, preds): the criterion's `loss_name` entries as detached device scalars of the global batch (the mean over the
        micro-batches of their weighted terms), and the list of the k prediction dicts (detached)."""
        mbs = [tuple(mb) for mb in micro_batches]
        if not mbs or any(len(mb) != 5 for mb in mbs):
            raise _C.EfghError('step_accumulated takes a sequence of k >= 1 tuples (pc, img, calib, A, gt)')
        sizes = [int(mb[0].shape[0]) for mb in mbs]
        if len(set(sizes)) != 1:
            raise _C.EfghError('step_accumulated: the micro-batches must have equal batch sizes, got %s' % sizes)
        k = len(mbs)
        weights = self._begin('step_accumulated', mbs if exact_depth_mean else None)   # ONE snapshot for the k micro-batches
        acc = self.accum = self.accum or GradAccumulator(self.flat)
        acc.reset()
        names = list(getattr(self.criterion, 'loss_name', None) or [])
        rows, preds, totals = [], [], []
        paused, self.comm.paused = self.comm.paused, True
        try:
            for i, mb in enumerate(mbs):
                losses, pred = self._forward_loss(*mb, depth_weight=weights[i] if weights is not None else 1.0)[::2]
                if i == 0:
                    self.flat.zero_grad()             # (later micro-batches find the buffer zeroed and re-armed by drain)
                losses['total'].backward()
                acc.drain()                           # (joins the side streams first, as `step` does after backward)
                names = names or list(losses)
                rows.append(torch.stack([losses[n].detach().reshape(()) for n in names]))
                preds.append({n: (v.detach() if torch.is_tensor(v) else v) for n, v in pred.items()})
                if self.txn is not None and 'total' not in names:
                    totals.append(losses['total'].detach().reshape(()))
                del losses, pred
        finally:
            self.comm.paused = paused
        stacked = rows[0] if k == 1 else torch.stack(rows)
        # ONE probe after the last drain: a running statistic that went inf / NaN in an earlier micro-batch stays so under
        # (1 - momentum) * running + momentum * batch, so the end state shows it; the k totals are read where they already are
        where = None
        if self.txn is not None:
            where = (stacked, len(names), names.index('total')) if 'total' in names else (torch.stack(totals), 1, 0)
        self._apply(k, where, grad=acc.acc)
        acc.reset()
        mean = stacked if k == 1 else stacked.sum(0) / k
        return {n: mean[j] for j, n in enumerate(names)}, preds
