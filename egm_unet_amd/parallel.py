"""Data-parallel gradient exchange: one process per GPU, RCCL all-reduce over xGMI via torch.distributed ("nccl").

The reference never wires DDP (train.py is single-device; only the metric reducers of
train_utils/distributed_utils.py:107-167 use collectives), so this is new functionality built for MI355X:

 * the 333 parameter gradients (6.30 M fp32 = 25.2 MB for EGM-UNet base_c=32) are packed into TWO flat buckets in
   backward order - bucket 0 = out_conv, up4..up1, attn1 (ready first), bucket 1 = down4..down1, in_conv;
 * as soon as the last gradient of a bucket has been accumulated (post-accumulate-grad hooks) the bucket is gathered by
   one multi-tensor HIP copy and all-reduced (SUM) on a SIDE stream, so bucket 0's exchange overlaps the encoder
   backward; 25 MB over 7 x ~153 GB/s xGMI links is latency-bound (~0.1-0.3 ms), hence few large messages;
 * the optimizer reads the reduced gradients straight from the buckets (no scatter back) with grad_scale = 1/world.
BatchNorm statistics stay per-rank (bs 8/GPU reproduces the reference's bs 8 regime; the reference has no SyncBN).
"""
import torch
import torch.distributed as dist

from ._lib import lib, ptr

BUCKET0_PREFIXES = ("out_conv", "up4", "up3", "up2", "up1", "attn1")


def _hip_gather(entries, device, stream_handle, table):
    """entries: [(dst_view, src_grad)] -> one multi-tensor copy on the given stream.  `table`: the ops.DeviceTable that carries the
    (dst, src, count) rows to the device -- uploaded from a pinned staging buffer only when a pointer changed, ordered behind the
    previous upload, one set of buffers per table namespace (so a captured graph owns the bytes it re-copies on replay)."""
    import struct
    blob = b"".join(struct.pack("<qqq", d.data_ptr(), s.data_ptr(), s.numel()) for d, s in entries)
    dev_table = table.get(blob, device)
    lib().call("egm_copy_multi", ptr(dev_table), len(entries), stream_handle)


class GradAllReducer:
    def __init__(self, model, world_size=None, gather_fn=None, use_side_stream=None, broadcast=True):
        self.world = world_size if world_size is not None else (dist.get_world_size() if dist.is_initialized() else 1)
        if self.world > 1 and not dist.is_initialized():
            raise RuntimeError("GradAllReducer(world_size=%d) needs an initialised torch.distributed process group" % self.world)
        if dist.is_initialized() and self.world != dist.get_world_size():
            # the collective below spans the whole process group: a reducer that believes in another world size would SUM over N ranks
            # while its caller scales by 1/world_size (and hang if not every rank builds one)
            raise RuntimeError("GradAllReducer(world_size=%d) inside a process group of %d ranks: pass world_size=None or the group's size"
                               % (self.world, dist.get_world_size()))
        # The collective is issued whenever a process group exists, ALSO at world size 1: a one-rank all-reduce is a valid RCCL
        # call and exercises the same stream / event / Work interplay with the graph replays as the N-rank step (the only way
        # a one-GPU box can run it).  Without a process group (plain single-process training) there is nothing to call.
        self.collective = dist.is_initialized()
        self.collectives_issued = 0               # all-reduces enqueued since construction (tests assert on it)
        if broadcast and dist.is_initialized() and dist.get_world_size() > 1:
            # every rank starts from rank 0's parameters and buffers (what DistributedDataParallel does at construction): ranks
            # that initialised differently would otherwise average gradients of different models and drift apart silently
            with torch.no_grad():
                for t in list(model.parameters()) + list(model.buffers()):
                    dist.broadcast(t, src=0)
            if next(model.parameters()).is_cuda:
                from . import ops
                ops.bump_weight_generation()
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        self.buckets = [[], []]
        for n, p in named:
            self.buckets[0 if n.startswith(BUCKET0_PREFIXES) else 1].append(p)
        if not self.buckets[0] or not self.buckets[1]:          # models without that naming: one bucket
            self.buckets = [[p for _, p in named]]
        dev = named[0][1].device
        self.device = dev
        self.flat, self.views, self.bucket_of = [], {}, {}
        for b, ps in enumerate(self.buckets):
            flat = torch.zeros(sum(p.numel() for p in ps), dtype=torch.float32, device=dev)
            off = 0
            for p in ps:
                self.views[p] = flat[off:off + p.numel()].view_as(p)
                self.bucket_of[p] = b
                off += p.numel()
            self.flat.append(flat)
        self.gather_fn = gather_fn
        cuda = dev.type == "cuda"
        self._tables = None
        if cuda and gather_fn is None:
            from . import ops
            self._tables = [ops.DeviceTable() for _ in self.buckets]
            for tb in self._tables:
                tb.reserve(dev)
        self.side = torch.cuda.Stream(device=dev) if (cuda and (use_side_stream is None or use_side_stream)) else None
        self._pending = [len(ps) for ps in self.buckets]
        self._works, self._keep = [], []
        self.hooks_enabled = True            # switched off while a fwd+bwd hipGraph is being captured
        self._hooks = [p.register_post_accumulate_grad_hook(self._on_grad) for _, p in named]

    # ---- called by autograd as each parameter's gradient lands
    def _on_grad(self, p):
        if not self.hooks_enabled:
            return
        b = self.bucket_of[p]
        self._pending[b] -= 1
        if self._pending[b] == 0:
            self._launch(b)

    def _launch(self, b):
        # conv weight gradients are finished by one deferred multi-conv reduction (ops._BackwardRun.flush, normally when backward ends):
        # bring the ones of this bucket up to date before they are gathered
        if self.device.type == "cuda":
            from . import ops
            ops.flush_ready_wgrads()
        entries = [(self.views[p], p.grad) for p in self.buckets[b]]
        if self.side is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.side):
                self.side.wait_event(ev)
                self._gather(entries, b)
                self._all_reduce(b)
        else:
            self._gather(entries, b)
            self._all_reduce(b)

    def _all_reduce(self, b):
        """SUM all-reduce of flat bucket b on the current stream (async Work kept for join()/finish()); returns True if enqueued."""
        if not self.collective:
            return False
        self._works.append(dist.all_reduce(self.flat[b], op=dist.ReduceOp.SUM, async_op=True))
        self.collectives_issued += 1
        return True

    def _gather(self, entries, b):
        if self.gather_fn is not None:
            self.gather_fn(entries)
        else:
            import ctypes
            h = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _hip_gather(entries, self.device, h, self._tables[b])

    # ---- explicit phases for a step captured as hipGraphs (graph.GraphedTrainStep): the gathers are captured inside the graphs, the
    # collectives run between the replays on the side stream
    def gather_bucket(self, b):
        """Copy bucket b's parameter gradients into its flat buffer on the CURRENT stream (legal inside a hipGraph capture)."""
        self._gather([(self.views[p], p.grad) for p in self.buckets[b]], b)

    def exchange_bucket(self, b, side, cur):
        """All-reduce flat bucket b on `side` once everything queued on `cur` so far (the graph that filled it) has finished.
        Returns True when a collective was actually enqueued (a process group exists)."""
        ev = torch.cuda.Event()
        ev.record(cur)
        with torch.cuda.stream(side):
            side.wait_event(ev)
            return self._all_reduce(b)

    def join(self, side, cur):
        """Make the reduced buckets visible to `cur`."""
        with torch.cuda.stream(side):
            for w in self._works:
                w.wait()
        cur.wait_stream(side)
        self._works = []

    def reduce_now(self):
        """Gradients already complete (e.g. after a captured fwd+bwd graph replay): exchange every bucket now."""
        for b in range(len(self.buckets)):
            self._pending[b] = 0
            self._launch(b)
        return self.finish()

    def finish(self):
        """After loss.backward(): make the reduced buckets visible to the current stream; returns {param: reduced grad}."""
        for b, n in enumerate(self._pending):
            if n != 0 and n != len(self.buckets[b]):
                raise RuntimeError("GradAllReducer: some parameters of a bucket received no gradient")
            if n == len(self.buckets[b]):
                raise RuntimeError("GradAllReducer: backward() did not reach bucket %d" % b)
        if self.side is not None:
            with torch.cuda.stream(self.side):
                for w in self._works:
                    w.wait()
            torch.cuda.current_stream(self.device).wait_stream(self.side)
        else:
            for w in self._works:
                w.wait()
        self._works, self._keep = [], []
        self._pending = [len(ps) for ps in self.buckets]
        return self.views

    def remove(self):
        for h in self._hooks:
            h.remove()
