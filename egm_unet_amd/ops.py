"""Autograd operators over the HIP library: every arithmetic step of the model goes through libegm_hip.so.

Activations are NHWC tensors ``[N, H, W, C]`` (fp32 or bf16, C a multiple of 8, possibly a channel-slice view of a
wider buffer).  torch is used for memory (torch.empty / views), streams and autograd bookkeeping only.
"""
import ctypes
import os
import struct
import threading
import weakref
from collections import namedtuple

import torch
from torch.autograd import Function, Variable

from ._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, dtype_code, lib, ptr, stream  # noqa: F401


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def _nhwc(t: torch.Tensor):
    """-> (tensor usable by the kernels, ld).  Accepts dense NHWC tensors and channel-slice views of them."""
    assert t.dim() == 4, t.shape
    N, H, W, C = t.shape
    s = t.stride()
    ok = (s[3] == 1 and s[2] % 8 == 0 and s[2] >= C and s[1] == W * s[2] and s[0] == H * W * s[2]
          and t.data_ptr() % 16 == 0 and C % 8 == 0)
    if not ok:
        if C % 8:
            raise RuntimeError(f"egm_unet_amd: channel count {C} is not a multiple of 8")
        t = t.contiguous()
        s = t.stride()
    return t, s[2]


def _npix(t):
    return t.shape[0] * t.shape[1] * t.shape[2]


def _f32(n, device, zero=False):
    return (torch.zeros if zero else torch.empty)(n, dtype=torch.float32, device=device)


class _Switch:
    """An A/B switch of this module (a bool).  `.on` is what the code here reads; calling the object is the public get / set.
    The environment variable is read once, where the switch is defined (import time)."""

    def __init__(self, env, default, doc=None):
        self.on, self.__doc__ = os.environ.get(env, default) != "0", doc

    def __call__(self, enabled=None):
        if enabled is not None:
            self.on = bool(enabled)
        return self.on


_zero_pools = {}


def _zero_grad_vec(n, device):
    """An all-zero fp32 gradient of n elements for a parameter whose gradient is identically zero (a conv bias in front of a train-mode
    BatchNorm): a slice of a zero buffer per device, allocated OUTSIDE any capture, instead of a fill kernel per parameter and step
    (14 launches per EGM-UNet step).  Every caller gets storage of its own: when a buffer is used up the next one is allocated (the
    slices handed out keep the old one alive), never a slice that somebody else already holds -- a user-side in-place write to such a
    gradient (p.grad.add_(), foreach optimizers with weight decay + maximize, gradient noise) then touches that one bias only.
    A captured graph never refills its slices, so writes to them persist across replays: use them read-only under graph replay."""
    pool = _zero_pools.get(device)
    if pool is None or pool[0].numel() < pool[1] + n:
        if torch.cuda.is_current_stream_capturing():
            return torch.zeros(n, dtype=torch.float32, device=device)      # the need arises inside a capture: plain fill this time
        pool = _zero_pools[device] = [torch.zeros(max(1 << 16, 4 * n), dtype=torch.float32, device=device), 0]
    off = pool[1]
    pool[1] = off + n
    return pool[0][off:off + n]


def _bn_conv_bias_grad(Cout, dy, training, device):
    """Gradient of a conv bias in front of a BatchNorm: identically zero when the BatchNorm normalises with batch statistics (the mean
    subtraction removes the bias), sum(dy) over the pixels when it is frozen (eval mode with grad enabled)."""
    return _zero_grad_vec(Cout, device) if training else _channel_sum(dy)[0, :Cout]


def _slot_or_new(out_slot, shape, dtype, device):
    """Output placement: `out_slot` is None or a one-element list holding a kernel-addressable NHWC view (a channel slice of a wider
    buffer, e.g. of a concat destination) the result is written into -- the concat copy and its extra tensor write disappear.  The
    list keeps the tensor out of autograd's sight: it is returned as a fresh output, not as an input passed through."""
    if out_slot is None:
        t = torch.empty(shape, dtype=dtype, device=device)
        return t, shape[3]
    t = out_slot[0]
    v, ld = _nhwc(t)
    if v.data_ptr() != t.data_ptr() or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
        raise RuntimeError(f"egm_unet_amd: output slot {tuple(t.shape)}/{t.dtype} does not fit result {tuple(shape)}/{dtype}")
    return t, ld


def cat_slots(N, H, W, channels, dtype, device):
    """A concat destination [N, H, W, sum(channels)] and its channel-slice views, for producers that write in place."""
    buf = torch.empty((N, H, W, sum(channels)), dtype=dtype, device=device)
    views, off = [], 0
    for c in channels:
        views.append(buf[..., off:off + c])
        off += c
    return buf, views


# ----------------------------------------------------------------------------------------------------------
# layout conversion at the module boundary
# ----------------------------------------------------------------------------------------------------------
class _ToNHWC(Function):
    @staticmethod
    def forward(ctx, x_nchw, dtype):
        x = x_nchw.contiguous().float()
        N, C, H, W = x.shape
        out = torch.empty((N, H, W, pad8(C)), dtype=dtype, device=x.device)
        lib().call("egm_nchw_to_nhwc", dtype_code(dtype), ptr(x), ptr(out), pad8(C), N, C, H, W, stream())
        ctx.C = C
        return out

    @staticmethod
    def backward(ctx, g):
        g, ld = _nhwc(g)
        N, H, W, _ = g.shape
        out = torch.empty((N, ctx.C, H, W), dtype=torch.float32, device=g.device)
        lib().call("egm_nhwc_to_nchw", dtype_code(g.dtype), ptr(g), ld, ptr(out), N, ctx.C, H, W, stream())
        return out, None


class _ToNCHW(Function):
    @staticmethod
    def forward(ctx, x, C):
        x, ld = _nhwc(x)
        N, H, W, CP = x.shape
        out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
        lib().call("egm_nhwc_to_nchw", dtype_code(x.dtype), ptr(x), ld, ptr(out), N, C, H, W, stream())
        ctx.dtype, ctx.CP = x.dtype, CP
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().float()
        N, C, H, W = g.shape
        out = torch.empty((N, H, W, ctx.CP), dtype=ctx.dtype, device=g.device)
        lib().call("egm_nchw_to_nhwc", dtype_code(ctx.dtype), ptr(g), ptr(out), ctx.CP, N, C, H, W, stream())
        return out, None


def to_nhwc(x_nchw, dtype):
    return _ToNHWC.apply(x_nchw, dtype)


def to_nchw(x_nhwc, C):
    return _ToNCHW.apply(x_nhwc, C)


# ----------------------------------------------------------------------------------------------------------
# descriptor tables for the multi-tensor kernels
# ----------------------------------------------------------------------------------------------------------
# Pointer tables are uploaded through pinned staging buffers.  A captured hipGraph re-copies the SAME pinned bytes on every replay, so
# the tables a capture uses must never be rewritten by anybody else (an eager step between replays, another capture): everything
# issued under table_namespace(tag) -- GraphedTrainStep runs its warm-up and its capture under one tag -- gets buffers of its own.
_table_tag = [None]


class table_namespace:
    def __init__(self, tag):
        self.tag, self.prev = tag, None

    def __enter__(self):
        self.prev, _table_tag[0] = _table_tag[0], self.tag

    def __exit__(self, *a):
        _table_tag[0] = self.prev


_all_tables = weakref.WeakSet()


def drop_table_namespace(tag):
    """Forget the buffers every DeviceTable holds for `tag` (a captured graph that no longer exists)."""
    for t in list(_all_tables):
        t.slots.pop(tag, None)


class DeviceTable:
    """Packed C structs on the device.  Re-uploaded only when the bytes change; the upload is an async copy from a pinned
    staging buffer, so it is legal inside hipGraph capture (replays re-copy the same bytes).  One set of buffers per table namespace.

    Inside a capture a table may be needed with SEVERAL contents (the data-parallel step flushes the deferred weight gradients once
    per captured backward half): a replay re-reads the pinned bytes at replay time, so each distinct content gets a buffer pair of its
    own from a small pool reserved before the capture (pinned allocation is not legal while capturing)."""
    POOL = 4

    def __init__(self):
        self.slots = {}                      # tag -> [key, pinned, device, upload event, spare pairs, {blob: device} of this capture]
        _all_tables.add(self)

    def _slot(self):
        return self.slots.setdefault(_table_tag[0], [None, None, None, None, [], {}])

    def reserve(self, device, n=65536):
        """Allocate the staging buffers now (pinned allocation is not legal inside a hipGraph capture)."""
        sl = self._slot()
        if sl[1] is None or sl[1].numel() < n:
            cap = max(n, 65536)
            sl[1] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            sl[2] = torch.empty(cap, dtype=torch.uint8, device=device)
            sl[0] = sl[3] = None
            sl[4] = [(torch.empty(cap, dtype=torch.uint8).pin_memory(), torch.empty(cap, dtype=torch.uint8, device=device))
                     for _ in range(self.POOL - 1)] if _table_tag[0] is not None else []
            sl[5] = {}

    def get(self, blob: bytes, device):
        sl = self._slot()
        if blob == sl[0]:
            return sl[2]
        n = len(blob)
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            # inside a capture the primary pair is never rewritten (it may serve a content captured earlier): every further content
            # takes a spare pair, whose pinned bytes are written once, here
            hit = sl[5].get(blob)
            if hit is not None:
                return hit
            if not sl[4] or sl[4][0][0].numel() < n:
                raise RuntimeError("egm_unet_amd: table pool exhausted inside a hipGraph capture (DeviceTable.POOL)")
            pinned, dev_buf = sl[4].pop(0)
            pinned[:n] = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
            dev_buf[:n].copy_(pinned[:n], non_blocking=True)
            sl[5][blob] = dev_buf
            sl.append((pinned, dev_buf))                       # the pair lives as long as the namespace
            return dev_buf
        self.reserve(device, n)
        upload_pinned(sl, 1, 2, 3, torch.frombuffer(bytearray(blob), dtype=torch.uint8), n)
        sl[0] = blob
        return sl[2]


def upload_pinned(slot, i_pinned, i_device, i_event, host_values, n):
    """Rewrite the first n elements of a pinned staging buffer and copy them to its device twin (async).  The host write must not
    overtake the previous upload from the same buffer (the copy engine may not have read it yet when the host runs ahead of the
    GPU), so every upload records an event and the next rewrite waits for it.  Inside a hipGraph capture neither is possible nor
    needed: a capture owns its table namespace, whose buffers are written once."""
    capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
    ev = slot[i_event]
    if ev is not None and not capturing:
        ev.synchronize()
    slot[i_pinned][:n] = host_values
    slot[i_device][:n].copy_(slot[i_pinned][:n], non_blocking=True)
    if not capturing and slot[i_device].is_cuda:
        if ev is None:
            ev = slot[i_event] = torch.cuda.Event()
        ev.record()


# ----------------------------------------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------------------------------------
_pack_cache = {}
_weight_generation = [0]


def bump_weight_generation():
    """Called by optimizers that update parameters through raw pointers (no torch version bump)."""
    _weight_generation[0] += 1


def _packed_weights(weight, groups, dtype):
    """fp32 OIHW parameter -> (wf, wd) operand packs; cached on (storage, version) so eval loops don't repack."""
    key = (weight.data_ptr(), weight._version, _weight_generation[0], dtype, groups, tuple(weight.shape))
    hit = _pack_cache.get(id(weight))
    if hit is not None and hit[0] == key and hit[3]() is weight:    # the weakref guards against id()/address reuse by a new tensor
        return hit[1], hit[2]
    Cout, Cin_g, KH, KW = weight.shape
    Cin = Cin_g * groups
    wf = torch.empty((KH * KW, pad8(Cout), pad8(Cin)), dtype=dtype, device=weight.device)
    wd = torch.empty((KH * KW, pad8(Cin), pad8(Cout)), dtype=dtype, device=weight.device)
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    lib().call("egm_conv_pack", dtype_code(dtype), ptr(w), ptr(wf), ptr(wd), Cout, Cin, KH, KW, groups, stream())
    _pack_cache[id(weight)] = (key, wf, wd, weakref.ref(weight))
    return wf, wd


_PACK_ENTRY = struct.Struct("<10Q10i")     # the table entry of egm_conv_pack_multi (include/egm_hip.h)
_derived_packs = {}                         # id(first real parameter) -> (stamp, weak reference to it, out, bout, wf, wd): see _prepacked


def _derived_stamp(reals, dtype):
    return (_weight_generation[0], dtype, tuple(p._version for p in reals), tuple(p.data_ptr() for p in reals))


def _prepacked(reals, dtype):
    """(out, bout, wf, wd) when the model-wide prepack has built the weight derived from `reals` for `dtype` and none of them has changed
    since (weight generation, versions, addresses), else None.  The buffers belong to the prepack state: callers hand out aliases."""
    hit = _derived_packs.get(id(reals[0]))
    if hit is None or hit[1]() is not reals[0] or hit[0] != _derived_stamp(reals, dtype):
        return None
    return hit[2:]


def prepack_model(model, dtype):
    """Pack every nn.Conv2d weight of `model` (except holders flagged _egm_no_prepack) in ONE kernel launch.  The same launch builds
    the derived weights of the modules that name them (a method _egm_derived_weights() -> [(kind, real parameters)], kind "fold2":
    (weight,), "merge357": (w3, w5, w7, b3, b5, b7)) and their packs: ops.fold2 / ops.merge357 then launch nothing."""
    st = getattr(model, "_egm_prepack", None)
    if st is None or st["dtype"] != dtype:
        convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d) and not getattr(m, "_egm_no_prepack", False)
                 and m.weight.dim() == 4 and m.weight.is_cuda]
        bufs = []
        for m in convs:
            Cout, Cin_g, KH, KW = m.weight.shape
            Cin = Cin_g * m.groups
            bufs.append((torch.empty((KH * KW, pad8(Cout), pad8(Cin)), dtype=dtype, device=m.weight.device),
                         torch.empty((KH * KW, pad8(Cin), pad8(Cout)), dtype=dtype, device=m.weight.device)))
        derived = []
        for m in (model.modules() if isinstance(model, torch.nn.Module) else ()):
            for kind, reals in (m._egm_derived_weights() if hasattr(m, "_egm_derived_weights") else ()):
                if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in reals):
                    continue
                dev = reals[0].device
                if kind == "fold2":
                    Co, Ci, taps = reals[0].shape[0], reals[0].shape[1] // 2, 1
                    out, bout = torch.empty((Co, Ci, 1, 1), dtype=torch.float32, device=dev), None
                else:
                    Co, Ci, taps = reals[2].shape[0], reals[2].shape[1], 49
                    out = torch.empty((Co, Ci, 7, 7), dtype=torch.float32, device=dev)
                    bout = torch.empty((Co,), dtype=torch.float32, device=dev)
                derived.append((kind, tuple(reals), Co, Ci, taps, out, bout,
                                torch.empty((taps, pad8(Co), pad8(Ci)), dtype=dtype, device=dev),
                                torch.empty((taps, pad8(Ci), pad8(Co)), dtype=dtype, device=dev)))
        st = model._egm_prepack = {"dtype": dtype, "convs": convs, "bufs": bufs, "derived": derived, "table": DeviceTable(), "stamp": None}
    convs, bufs, derived = st["convs"], st["bufs"], st.get("derived", ())
    if not convs and not derived:
        return
    held = [m.weight for m in convs] + [p for d in derived for p in d[1]]
    stamp = (_weight_generation[0], tuple(p._version for p in held), tuple(p.data_ptr() for p in held))
    if stamp == st["stamp"]:
        return
    L = lib()
    chunk = L.cdll.egm_conv_pack_chunk()
    blob, chunks = bytearray(), 0
    for m, (wf, wd) in zip(convs, bufs):
        Cout, Cin_g, KH, KW = m.weight.shape
        Cin = Cin_g * m.groups
        blob += _PACK_ENTRY.pack(m.weight.data_ptr(), wf.data_ptr(), wd.data_ptr(), 0, 0, 0, 0, 0, 0, 0, Cout, Cin, pad8(Cout), pad8(Cin),
                                 KH, KW, m.groups, chunks, 0, 0)       # chunks = index of the entry's first workgroup
        chunks += (KH * KW * pad8(Cout) * pad8(Cin) + chunk - 1) // chunk
    for kind, reals, Co, Ci, taps, out, bout, wf, wd in derived:
        if kind == "fold2":
            blob += _PACK_ENTRY.pack(reals[0].data_ptr(), wf.data_ptr(), wd.data_ptr(), 0, 0, 0, 0, 0, out.data_ptr(), 0, Co, Ci, pad8(Co),
                                     pad8(Ci), 1, 1, 1, chunks, 1, 0)
        else:
            w3, w5, w7, b3, b5, b7 = reals
            blob += _PACK_ENTRY.pack(w7.data_ptr(), wf.data_ptr(), wd.data_ptr(), w5.data_ptr(), w3.data_ptr(), b7.data_ptr(), b5.data_ptr(),
                                     b3.data_ptr(), out.data_ptr(), bout.data_ptr(), Co, Ci, pad8(Co), pad8(Ci), 7, 7, 1, chunks, 2, 0)
        chunks += (taps * pad8(Co) * pad8(Ci) + chunk - 1) // chunk
    dev = held[0].device
    table = st["table"].get(bytes(blob), dev)
    L.call("egm_conv_pack_multi", dtype_code(dtype), ptr(table), len(convs) + len(derived), chunks, stream())
    for m, (wf, wd) in zip(convs, bufs):
        w = m.weight
        key = (w.data_ptr(), w._version, _weight_generation[0], dtype, m.groups, tuple(w.shape))
        _pack_cache[id(w)] = (key, wf, wd, weakref.ref(w))
    if len(_derived_packs) > 64:                                      # drop the buffers of models that are gone
        for k in [k for k, v in _derived_packs.items() if v[1]() is None]:
            del _derived_packs[k]
    for kind, reals, Co, Ci, taps, out, bout, wf, wd in derived:
        _derived_packs[id(reals[0])] =(_derived_stamp(reals, dtype), weakref.ref(reals[0]), out, bout, wf, wd)
    st["stamp"] = stamp


# ----------------------------------------------------------------------------------------------------------
# deferred work of a backward run
# ----------------------------------------------------------------------------------------------------------
# A backward pass postpones four kinds of work to its end, all of it held by ONE _BackwardRun record per autograd-engine run:
#   slabs    the slab kernels of deferred weight gradients, launched together, four of one kernel instantiation to a launch
#   wgrads   the reductions of those slabs, ONE multi-conv launch (egm_wgrad_reduce_multi)
#   bgrads   db = sum over pixels of dy for every nn.Conv2d bias that no BatchNorm follows, ONE pair of launches (egm_bias_grad_multi)
#   dz       data gradients that a BatchNorm backward computes itself from a stand-in tensor (csrc/bn_dz_fused.hip)
# (`derived` holds the open stand-ins of convs on derived weights, whose wgrads / bgrads entries still wait for the real destinations.)
# Deferring a weight (bias) gradient hands autograd a tensor that is filled later, which is only sound when that tensor is the
# parameter's ONLY contribution in this backward (autograd would otherwise sum unfilled buffers): _conv_uses counts the conv forwards a
# weight has taken part in since its gradients were last produced, and a weight used more than once takes the immediate path.  That
# count is written in forward, so it is keyed by weight, not by run.
_conv_uses = {}                           # id(weight) -> [weakref, weight generation, forwards awaiting their backward, peak of that]


def _note_conv_use(weight):
    ent = _conv_uses.get(id(weight))
    if ent is None or ent[0]() is not weight or ent[1] != _weight_generation[0]:
        ent = _conv_uses[id(weight)] = [weakref.ref(weight), _weight_generation[0], 0, 0]
        if len(_conv_uses) > 4096:                                    # drop entries of dead tensors
            for k in [k for k, v in _conv_uses.items() if v[0]() is None]:
                del _conv_uses[k]
    ent[2] += 1
    ent[3] = max(ent[3], ent[2])


def _sole_conv_use(weight):
    """True when `weight` fed exactly one conv forward that still awaits its backward (the one running now); consumes that use."""
    ent = _conv_uses.get(id(weight))
    if ent is None or ent[0]() is not weight:
        return False
    sole = ent[3] == 1
    ent[2] -= 1
    if ent[2] <= 0:
        del _conv_uses[id(weight)]
    return sole


_DEFER_WGRAD = os.environ.get("EGM_DEFER_WGRAD", "1") != "0"
merge_wgrads = _Switch("EGM_MERGE_WGRAD", "1",
                       """Get / set whether the slab kernels of deferred weight gradients are launched together when backward ends (merged
                       launches).""")
defer_bgrads = _Switch("EGM_DEFER_BGRAD", "1",
                       """Get / set whether conv bias gradients are left to the one multi-tensor pass at the end of backward.""")
fuse_dz = _Switch("EGM_FUSE_DZ", "1",
                  """Get / set whether BatchNorm backward computes dz on the fly from the classifier / MCALayer behind it (tests compare both
                  ways).""")
defer_derived = _Switch("EGM_DEFER_DERIVED", "1",
                        """Get / set whether the gradients of a conv whose weight is derived from real parameters (ops.fold2, ops.merge357)
                        join the deferred work of the backward run: the end-of-backward reduction then writes the real parameters'
                        gradients itself (tests compare both ways).""")


def _wgrad_deferrable(weight):
    """True when the slab reduction of this weight's gradient may be left to the ONE multi-conv launch at the end of backward: a leaf
    parameter whose only gradient contribution this is (not when a tensor hook may replace the returned buffer, nor under create_graph:
    both hand autograd something it copies).  Consumes the conv-use note of the weight: call once per backward of a conv."""
    return (_DEFER_WGRAD and _sole_conv_use(weight) and weight.is_leaf and weight.grad is None
            and not weight._backward_hooks and not torch.is_grad_enabled())


# Derived weights (ops.fold2 / ops.merge357): non-leaf tensors computed from real parameters by an autograd node of this module.  The
# side table says which, so that the backward of the conv that consumes one can defer like a conv on a leaf weight: its slab reduction
# (and the merged bias sum) then write the gradients of the REAL parameters, and the node in between launches nothing.
_Derived = namedtuple("_Derived", "ref kind reals")      # kind: "fold2" | "merge357" | "bias3"; reals in the kernel's destination order
_derived = {}                                             # id(derived tensor) -> _Derived
WRED_PLAIN, WRED_FOLD2, WRED_MERGE357, WRED_WIDE = 0, 1, 2, 4     # egm_wgrad_reduce_multi: entry modes


def _register_derived(t, kind, reals):
    """`t` was computed from the parameters `reals`; each of them takes part in one more conv forward that awaits its backward."""
    if not t.requires_grad:
        return
    if len(_derived) > 256:
        for k in [k for k, v in _derived.items() if v.ref() is None]:
            del _derived[k]
    _derived[id(t)] = _Derived(weakref.ref(t), kind, tuple(reals))
    for p in reals:
        _note_conv_use(p)


def _derived_of(t):
    d = _derived.get(id(t)) if t is not None else None
    return d if d is not None and d.ref() is t else None


def _fillable(p):
    """A leaf parameter whose gradient autograd will adopt as it is returned (see _wgrad_deferrable)."""
    return p.is_leaf and p.requires_grad and p.grad is None and not p._backward_hooks


def _wgrad_deferral(weight, bias=None):
    """The answer of _wgrad_deferrable for the weight of a conv whose backward runs now; for a derived weight the _Derived record
    instead of True when every real parameter behind it (and behind `bias`, when that is derived too and wanted) would pass on its own
    terms.  Consumes the use notes of the weight and of the real parameters: call once per backward of a conv."""
    d = _derived_of(weight)
    if d is None:
        return _wgrad_deferrable(weight)
    db = _derived_of(bias)
    ok = _sole_conv_use(weight)
    reals = d.reals + (db.reals if db is not None else ())
    sole = [_sole_conv_use(p) for p in reals]                        # (a list: every note is consumed)
    ok = (ok and all(sole) and all(_fillable(p) for p in reals) and _DEFER_WGRAD and defer_derived.on and merge_wgrads.on
          and (db is None or defer_bgrads.on) and (bias is None or db is not None or bias.is_leaf) and not torch.is_grad_enabled())
    return d if ok else False


# The tables outlive every run on purpose: a captured hipGraph re-uploads their bytes on every replay.  The *_partial twins serve the
# mid-backward flushes (eager gradient exchange), which must never disturb the bytes a captured graph re-uploads.
_wgrad_table, _wgrad_table_partial, _bgrad_table, _bgrad_table_partial = DeviceTable(), DeviceTable(), DeviceTable(), DeviceTable()
_BSUM_ENTRY = struct.Struct("<3Qq6i")       # egm_bsum_entry
_WGRAD_DESC = struct.Struct("<3Q14i")       # egm_conv_wgrad_desc
_WRED_ENTRY = struct.Struct("<4Q10i")       # the table entry of egm_wgrad_reduce_multi (include/egm_hip.h)
_wgrad_names = {}


def _wgrad_kernel_of(dt, N, H, W, CinP, CoutP, KH, KW, dil):
    key = (dt, N, H, W, CinP, CoutP, KH, KW, dil)
    name = _wgrad_names.get(key)
    if name is None:
        buf = ctypes.create_string_buffer(96)
        lib().cdll.egm_conv_wgrad_kernel_name(dt, N, H, W, CinP, CoutP, KH, KW, dil, ctypes.cast(buf, ctypes.c_void_p), 96)
        name = _wgrad_names[key] = buf.value
    return name


# queue entries (they keep the tensors their launch reads alive).  `dests` lists the gradients the launch writes as (parameter, weak
# reference to the unfilled tensor backward() returned for it, that tensor's address): one for a leaf weight / bias; for a derived
# weight or bias `ndest` of them, the real parameters behind it, attached by the backward of the deriving node (_attach_derived) --
# until then the list is short and the entry is not ready.
_Slab = namedtuple("_Slab", "dt x ldx gy ldg ws N H W CinP CoutP Cin Cout KH KW dil groups")
_Wgrad = namedtuple("_Wgrad", "ws nslab taps CoutP CinP Cout Cin groups mode ndest dests")
_Bgrad = namedtuple("_Bgrad", "gy ldg npix C Cout ndest dests")


def _unfilled(shape, device):
    """A gradient tensor that the end-of-backward launches fill (tests replace this to see an unfilled one)."""
    return torch.empty(shape, dtype=torch.float32, device=device)


def _handed_over(queue, ready_only, name):
    """The hand-over protocol of the deferred weight and bias gradients.  The unfilled tensor backward() returned was handed to autograd
    with no reference kept here, so that it is adopted as param.grad without a copy (backward()) or returned to the caller as is
    (torch.autograd.grad()); it is still reachable through the weak reference or as the storage param.grad now shares.
    -> [(entry, destination addresses, None for a discarded one)] to fill now; `queue` keeps the entries for later (ready_only: autograd
    has not adopted the tensor yet).  An entry with several destinations is taken when ALL of them can be written, and is never dropped
    while one of them is still to come."""
    todo, later = [], []
    for ent in queue:
        ptrs, pending = [], len(ent.dests) < ent.ndest             # a derived entry whose stand-in has not reached its node yet
        for param, gref, gptr in ent.dests:
            grad = param.grad
            if gref() is not None or (grad is not None and grad.data_ptr() == gptr):
                ptrs.append(gptr)
            elif ready_only:
                pending = True
            elif grad is not None:
                # the unfilled buffer is gone but the parameter HAS a gradient: autograd copied or transformed the buffer instead of
                # adopting it (a tensor hook returning a new tensor, a non-stealable gradient), so param.grad holds whatever the
                # uninitialised buffer contained.  The deferring code refuses in the cases it can see; anything else must not train on.
                raise RuntimeError(f"deferred conv {name} gradient lost its destination: {name}.grad exists but is not the buffer backward() "
                                   f"returned (tensor hook / gradient copy); set EGM_DEFER_{name[0].upper()}GRAD=0 for this model")
            else:
                # nobody holds the gradient and the parameter has none (torch.autograd.grad() result dropped, or the parameter was not
                # among backward(inputs=...)): it was discarded, nothing to finish
                ptrs.append(None)
        if pending:
            if not ready_only:
                raise RuntimeError(f"deferred conv {name} gradient of a derived {name} never reached its real parameters")
            later.append(ent)
        elif any(q is not None for q in ptrs):
            todo.append((ent, ptrs))
    queue[:] = later
    return todo


_runs = {}                                # autograd graph-task id -> weak reference to its _BackwardRun; gone when the record dies


class _BackwardRun:
    """The deferred work of ONE autograd-engine run.  The engine owns it: the only strong reference is the end-of-run callback
    (`finish`) queued on the run's graph task, _runs finds it by graph-task id while the run lasts.  A backward that raises never runs
    its callbacks, the engine drops the graph task and the record (with the tensors its entries pin) goes with it; a backward nested in
    another one (a Function whose backward calls backward, re-entrant checkpointing) has a graph task and hence a record of its own,
    finished when IT ends, and leaves the outer run's entries alone.
    The DeviceTables are shared by all runs.  Outside a capture that is safe under nesting (uploads are ordered on the stream, a rewrite
    of the pinned bytes waits for the previous upload: upload_pinned); inside a hipGraph capture every distinct content takes one buffer
    pair of DeviceTable.POOL, so nested runs inside a capture are bounded by that pool (exhaustion raises)."""
    __slots__ = ("id", "slabs", "wgrads", "bgrads", "dz", "derived", "__weakref__")

    def __init__(self, run_id):
        self.id, self.slabs, self.wgrads, self.bgrads, self.dz, self.derived = run_id, [], [], [], {}, {}

    def finish(self):
        _runs.pop(self.id, None)
        if self.dz:
            kinds = [v[1][0] for v in self.dz.values()]
            self.dz.clear()
            raise RuntimeError(f"egm_unet_amd: deferred BatchNorm gradients {kinds} were never consumed (the tensor between the producer and "
                               "its BatchNorm had another consumer); call ops.fuse_dz(False)")
        if self.derived:
            # stand-ins whose deriving node never ran in this run: autograd had no use for the derived tensor's gradient (its real
            # parameters are not among backward(inputs=...): the decoder half of the split data-parallel step runs the encoder's
            # FusionConv convs for their data gradients only) and dropped it.  Nothing to finish, as for a plain weight whose returned
            # gradient was discarded.  (A node that DOES run while a stand-in of its own is open, but receives something else, raises
            # there and then: _no_open_standin.)
            dead = [v[1] for v in self.derived.values()]
            self.derived.clear()
            gone = lambda e: any(e is d for d in dead)
            self.slabs = [s for s in self.slabs if not any(s.ws is d.ws for d in dead if isinstance(d, _Wgrad))]
            self.wgrads, self.bgrads = [e for e in self.wgrads if not gone(e)], [e for e in self.bgrads if not gone(e)]
        self.flush()

    def flush(self, ready_only=False):
        """ready_only=True (a gradient bucket is about to be gathered mid-backward, parallel.GradAllReducer) finishes the gradients whose
        tensor autograd has already adopted and leaves the others pending."""
        self.flush_bgrads(ready_only)
        self.launch_slabs()
        self.reduce_wgrads(ready_only)

    def flush_bgrads(self, ready_only=False):
        todo = _handed_over(self.bgrads, ready_only, "bias") if self.bgrads else None
        if not todo:
            return
        L = lib()
        by_dtype = {}
        for e, ptrs in todo:
            by_dtype.setdefault(e.gy.dtype, []).append((e, [q for q in ptrs if q is not None]))
        for dtype, ents in by_dtype.items():
            dev = ents[0][0].gy.device
            nblks = [L.query("egm_channel_partials_blocks", e.npix, e.C) for e, _ in ents]
            ws = torch.empty(sum(nb * 2 * e.C for nb, (e, _) in zip(nblks, ents)), dtype=torch.float32, device=dev)
            blob1, blob2, b1, b2, off = bytearray(), bytearray(), 0, 0, 0
            for nb, (e, outs) in zip(nblks, ents):
                part = ws.data_ptr() + 4 * off
                # one pass over dy per tensor; a sum with several destinations (the merged bias of merge357: the same number for three
                # parameters) takes one stage-2 entry per destination, all reading the same partials, and as many stage-1 entries, the
                # extra ones without blocks (the block search never lands on an entry that shares its first block with its successor)
                for j, out in enumerate(outs):
                    blob1 += _BSUM_ENTRY.pack(e.gy.data_ptr(), part, out, e.npix, e.ldg, e.C, e.Cout, nb if j == 0 else 0, b1, 0)
                    blob2 += _BSUM_ENTRY.pack(e.gy.data_ptr(), part, out, e.npix, e.ldg, e.C, e.Cout, nb, b2, 0)
                    b1 += nb if j == 0 else 0; b2 += e.C // 8
                off += nb * 2 * e.C
            _bgrad_table.reserve(dev); _bgrad_table_partial.reserve(dev)
            table = (_bgrad_table_partial if ready_only else _bgrad_table).get(bytes(blob1 + blob2), dev)
            L.call("egm_bias_grad_multi", dtype_code(dtype), ptr(table), len(blob2) // _BSUM_ENTRY.size, b1, b2, stream())

    def launch_slabs(self):
        """The queued slab kernels, in queue order, those of one kernel instantiation four to a launch (egm_conv_wgrad_multi)."""
        if not self.slabs:
            return
        L, st = lib(), stream()
        todo, self.slabs = self.slabs, []
        buckets = {}
        for e in todo:
            buckets.setdefault((e.dt, _wgrad_kernel_of(e.dt, e.N, e.H, e.W, e.CinP, e.CoutP, e.KH, e.KW, e.dil)), []).append(e)
        per = 4                                                            # EGM_WGRAD_MULTI_MAX
        for (dt, _name), ents in buckets.items():
            for i in range(0, len(ents), per):
                blob = b"".join(_WGRAD_DESC.pack(e.x.data_ptr(), e.gy.data_ptr(), e.ws.data_ptr(), e.ldx, e.ldg, e.N, e.H, e.W, e.CinP, e.CoutP,
                                                 e.Cin, e.Cout, e.KH, e.KW, e.dil, e.groups, 0) for e in ents[i:i + per])
                L.call("egm_conv_wgrad_multi", dt, blob, len(ents[i:i + per]), st)

    def reduce_wgrads(self, ready_only=False):
        """Finish the deferred weight gradients with ONE multi-conv reduction."""
        todo = _handed_over(self.wgrads, ready_only, "weight") if self.wgrads else None
        if not todo:
            return
        blob, chunks = bytearray(), 0
        per, per_wide = lib().cdll.egm_wgrad_reduce_chunk(), lib().cdll.egm_wgrad_reduce_chunk_wide()
        for e, ptrs in todo:
            d = [q or 0 for q in ptrs] + [0, 0]
            blob += _WRED_ENTRY.pack(e.ws.data_ptr(), d[0], d[1], d[2], e.nslab, e.taps, e.CoutP, e.CinP, e.Cout, e.Cin, e.groups, 0, chunks,
                                     e.mode)
            n = per_wide if e.mode & WRED_WIDE else per
            chunks += (e.taps * e.CoutP * e.CinP + n - 1) // n
        dev = todo[0][0].ws.device
        _wgrad_table.reserve(dev); _wgrad_table_partial.reserve(dev)      # both exist before any capture can need them
        table = (_wgrad_table_partial if ready_only else _wgrad_table).get(bytes(blob), dev)
        lib().call("egm_wgrad_reduce_multi", ptr(table), len(todo), chunks, stream())


def _run(create=True):
    """The record of the backward run this is called from (create=False: None when the run has deferred nothing so far)."""
    run_id = torch._C._current_graph_task_id()
    ref = _runs.get(run_id)                 # (a plain dict, half the cost of a WeakValueDictionary: backward nodes look up on every call)
    run = None if ref is None else ref()
    if run is None and create:
        run = _BackwardRun(run_id)
        _runs[run_id] = weakref.ref(run, lambda _ref: _runs.pop(run_id, None))
        Variable._execution_engine.queue_callback(run.finish)          # the one strong reference: the run's graph task
    return run


def flush_ready_wgrads():
    """Mid-backward (a gradient hook): finish what the current run has deferred and autograd has already adopted."""
    run = _run(create=False)
    if run is not None:
        run.flush(ready_only=True)


def _queue_wgrad(ws, weight, nslab, taps, CoutP, CinP, Cout, Cin, groups, gw, defer=True):
    """Queue the slab reduction of a conv whose backward returns the unfilled `gw` for `weight`.  defer = the _Derived record of a derived
    weight (_wgrad_deferral): gw is then a stand-in on its way to the deriving node, which names the real destinations
    (_attach_derived); a layer whose own reduction is the many-slab kernel keeps that summation order."""
    run = _run()
    if defer is True:
        run.wgrads.append(_Wgrad(ws, nslab, taps, CoutP, CinP, Cout, Cin, groups, WRED_PLAIN, 1, [(weight, weakref.ref(gw), gw.data_ptr())]))
        return
    mode, ndest = (WRED_FOLD2, 1) if defer.kind == "fold2" else (WRED_MERGE357, 3)
    if lib().cdll.egm_wgrad_reduce_is_wide(nslab, taps, CoutP, CinP):
        mode |= WRED_WIDE
    ent = _Wgrad(ws, nslab, taps, CoutP, CinP, Cout, Cin, groups, mode, ndest, [])
    run.wgrads.append(ent)
    run.derived[gw.data_ptr()] = (gw, ent, defer.reals[0])         # the stand-in stays alive: its address cannot be recycled meanwhile


def _queue_derived_bgrad(gy, Cout, derived):
    """The merged bias of merge357 (`derived`: its _Derived record) behind a conv that defers: one pass over gy at the end of backward
    writes all three real biases.  -> the stand-in for the derived bias's gradient."""
    gy, ldg = _nhwc(gy)
    gb = torch.empty(Cout, dtype=torch.float32, device=gy.device)
    ent = _Bgrad(gy, ldg, _npix(gy), gy.shape[3], Cout, 3, [])
    run = _run()
    run.bgrads.append(ent)
    run.derived[gb.data_ptr()] = (gb, ent, derived.reals[0])
    return gb


def _take_derived(g):
    """The queue entry when the incoming gradient `g` is a stand-in registered in this run, else None.  Creates no record."""
    run = _run(create=False)
    pend = run.derived.pop(g.data_ptr(), None) if run is not None and run.derived and g is not None else None
    return None if pend is None else pend[1]


def _no_open_standin(reals):
    """Called by a deriving node whose incoming gradient is NOT a stand-in: no stand-in for a tensor derived from `reals` may be open in
    this run -- the derived tensor then had a consumer besides its conv, autograd summed the stand-in into something else, and the
    gradient at hand is garbage."""
    run = _run(create=False)
    if run is not None and run.derived and any(v[2] is p for v in run.derived.values() for p in reals):
        raise RuntimeError("egm_unet_amd: the deferred gradient of a derived weight was never consumed (the derived tensor had a consumer "
                           "besides its conv); call ops.defer_derived(False)")


def _attach_derived(ent, params, grads):
    """Name the real destinations of a derived entry: `grads` are the unfilled tensors the deriving node returns for `params`."""
    ent.dests.extend((p, weakref.ref(g), g.data_ptr()) for p, g in zip(params, grads))


# deferred dz: the producer's backward (the 1x1 classifier's data gradient; the MCALayer's last step; a conv behind a concat) does not
# run its kernel, or writes elsewhere: it returns a STAND-IN tensor of the right shape and registers what the consumer needs under the
# stand-in's address; _ConvBN.backward / _UpCat.backward pick it up.  Only used where the model code knows the tensor between the two
# nodes has exactly one consumer (so autograd hands the stand-in through unchanged); an entry nobody consumed by the end of the backward
# run is an error (_BackwardRun.finish), not a silent garbage gradient.
def _defer_dz(standin, payload):
    _run().dz[standin.data_ptr()] = (standin, payload)             # the stand-in stays alive: its address cannot be recycled meanwhile


def _take_dz(g):
    """(stand-in, payload) when the incoming gradient `g` is a stand-in registered in this run, else None.  Creates no record."""
    run = _run(create=False)
    return run.dz.pop(g.data_ptr(), None) if run is not None and run.dz else None


def _bias_grad(gy, Cout, bias=None, defer=False):
    """db[c] = sum over pixels of gy[..., c] (gy NHWC, channels padded) -> fp32 [Cout].  defer: the conv's weight gradient is being
    deferred in this backward (so this is the only use of the layer in it) -- the bias gradient then joins the end-of-backward pass:
    an unfilled [Cout] tensor is returned, the queue entry keeps gy alive."""
    if (defer and defer_bgrads.on and bias is not None and bias.is_leaf and bias.grad is None and not bias._backward_hooks
            and not torch.is_grad_enabled()):
        gy, ldg = _nhwc(gy)
        gb = torch.empty(Cout, dtype=torch.float32, device=gy.device)
        _run().bgrads.append(_Bgrad(gy, ldg, _npix(gy), gy.shape[3], Cout, 1, [(bias, weakref.ref(gb), gb.data_ptr())]))
        return gb
    return _channel_sum(gy)[0, :Cout]


def _channel_sum(t):
    """sum over pixels of an NHWC tensor -> fp32 [2, C] (row 0 = sum, row 1 = sum of squares)."""
    t, ld = _nhwc(t)
    C, npix = t.shape[3], _npix(t)
    nb = lib().query("egm_channel_partials_blocks", npix, C)
    part = _f32(nb * 2 * C, t.device)
    out = _f32((2, C), t.device)
    lib().call("egm_channel_sums", dtype_code(t.dtype), ptr(t), ld, npix, C, ptr(part), stream())
    lib().call("egm_reduce_tiles", ptr(part), nb, C, ptr(out), stream())
    return out


class Lazy:
    """A logical activation z = act(scale*y + shift) that has NOT been written to memory: `y` is the raw conv output (the autograd
    stand-in: its gradient is, by convention, dL/dz), `coef` the fp32 [4, C] rows scale | shift | mean | rstd of the BatchNorm.
    Handed to a consumer whose first pass applies the BatchNorm itself and writes the tensor on the way (the MCALayer's statistics pass,
    the classifier inside the apply pass, the fused skip-connection pool); everything else calls materialize().
    (Rounds 2-3 also let convolutions consume it through operand prologues; measured slower three times -- DESIGN.md 6.2, 6.4, 6.5 --
    and removed in round 4.)"""
    __slots__ = ("y", "coef", "act")

    def __init__(self, y, coef, act):
        self.y, self.coef, self.act = y, coef, act

    shape = property(lambda self: self.y.shape)
    dtype = property(lambda self: self.y.dtype)
    device = property(lambda self: self.y.device)

    def materialize(self, out=None):
        return _Materialize.apply(self.y, self.coef, self.act, None if out is None else [out])


def materialize(x, out=None):
    """Lazy -> tensor (optionally into the destination view `out`); tensors pass through (copied only if `out` is another place)."""
    if isinstance(x, Lazy):
        return x.materialize(out)
    if out is not None and not (x.data_ptr() == out.data_ptr() and x.stride() == out.stride()):
        return _axpby(x, 1.0, None, 0.0, out)
    return x


class _Materialize(Function):
    """z = act(scale*y + shift) as a tensor.  The gradient of the stand-in y IS dL/dz (see Lazy), so backward is the identity:
    the activation derivative and the BatchNorm backward both happen in the producing _ConvBN node."""

    @staticmethod
    def forward(ctx, y, coef, act, out_slot):
        y, ldy = _nhwc(y)
        N, H, W, CP = y.shape
        z, ldz = _slot_or_new(out_slot, (N, H, W, CP), y.dtype, y.device)
        lib().call("egm_bn_act_fwd", dtype_code(y.dtype), ptr(y), ldy, ptr(coef[0]), ptr(coef[1]), act, ptr(z), ldz, _npix(y), CP, stream())
        return z

    @staticmethod
    def backward(ctx, g):
        return g, None, None, None


def _unlazy(x):
    """-> (tensor, coef or None, act): a consumer's memory operand and the BatchNorm + activation it has to apply to it"""
    if isinstance(x, Lazy):
        return x.y, x.coef, x.act
    return x, None, ACT_NONE


group_convs = _Switch("EGM_GROUP_CONVS", "1",
                      """Get / set whether conv_group() merges launches (tests compare both ways).""")


class conv_group:
    """`with conv_group():` -- the egm_conv_fwd* launches issued inside are recorded by the library and launched together on exit, those
    of one kernel instantiation as ONE launch (csrc/group.h).  Only for convolutions that are independent of each other and whose
    outputs are first used after the block.  EGM_GROUP_CONVS=0 turns it into a no-op."""

    depth = 0                                 # open conv_group blocks, whether or not merging is switched on (bench.py's bookkeeping)
    serial = 0                                # number of the outermost block that is open / was opened last

    def __enter__(self):
        self.on = group_convs.on
        conv_group.depth += 1
        if conv_group.depth == 1:
            conv_group.serial += 1
        if self.on:
            lib().call("egm_group_begin")
        return self

    def __exit__(self, et, ev, tb):
        conv_group.depth -= 1
        if self.on:
            if et is None:
                lib().call("egm_group_end", stream())
            else:
                lib().cdll.egm_group_abort()
        return False


def _conv_forward(x, ldx, weight, bias, dil, groups, want_stats):
    """The conv launch shared by _Conv2d and _ConvBN: y = conv(x, weight) (+bias), optional BN partial statistics."""
    N, H, W, CinP = x.shape
    Cout, Cin_g, KH, KW = weight.shape
    Cin = Cin_g * groups
    if pad8(Cin) != CinP:
        raise RuntimeError(f"conv2d: input has {CinP} channels, weight expects {Cin} (padded {pad8(Cin)})")
    CoutP = pad8(Cout)
    L, dt = lib(), dtype_code(x.dtype)
    wf, wd = _packed_weights(weight, groups, x.dtype)
    y = torch.empty((N, H, W, CoutP), dtype=x.dtype, device=x.device)
    stats = None
    if want_stats:
        ntiles = L.query("egm_conv_stats_tiles", dt, N, H, W, CinP, CoutP, KH, KW, dil)
        stats = _f32((ntiles, 2, CoutP), x.device)
    b = bias.detach() if bias is not None else None
    L.call("egm_conv_fwd", dt, ptr(x), ldx, ptr(wf), ptr(b), Cout if b is not None else 0, ptr(y), CoutP, ptr(stats), N, H, W, CinP, CoutP,
           KH, KW, dil, stream())
    return y, stats, wd


# ---- 1x1 convolutions: data gradient + weight-gradient slabs in ONE pass over dy and x (csrc/conv1x1_bwd.hip, egm_conv1x1_bwd) ---
_C1_DESC = struct.Struct("<5Qq6i")
_C1_MAXC = int(os.environ.get("EGM_CONV1X1_BWD_MAXC", "64"))


fuse_c1 = _Switch("EGM_CONV1X1_BWD", "1",
                  """Get / set whether the backward of a 1x1 conv runs as one fused launch (dx + weight-gradient slabs) where that applies.""")


def _c1_shape_ok(x, gy, weight, dil, groups):
    # measured (profiles/r04_*): <= 64 channels on both sides 32-43 us against 60 us for the pair at 8 x 256^2 x 64; at 128 channels the
    # fused kernel needs one workgroup per CU and two column blocks and LOSES (73 us against 43 us), so those keep the pair
    return (fuse_c1.on and weight.shape[2] == 1 and weight.shape[3] == 1 and groups == 1 and x.shape[3] <= _C1_MAXC and gy.shape[3] <= _C1_MAXC
            and bool(lib().cdll.egm_conv1x1_bwd_supported(dtype_code(x.dtype), x.shape[3], gy.shape[3])))


def _conv1x1_bwd(items):
    """items: up to 4 tuples (x, ldx, dy, lddy, weight, wd, need_gx, defer) of 1x1 convs -> [(gx, gw)].  ONE launch writes every dx and
    every slab set; the slabs of a deferrable weight join the deferred multi-conv reduction like _conv_wgrad's, the others are reduced
    at once.  (The kernel choice must not depend on `defer`: a weight is not deferrable when its conv's backward runs a second time --
    the split data-parallel step re-runs the bottleneck -- and both runs have to produce the same dx bit for bit.)"""
    L, st = lib(), stream()
    descs, res, now = [], [], []
    dt = dtype_code(items[0][0].dtype)
    for x, ldx, dy, lddy, weight, wd, need_gx, defer in items:
        N, H, W, CinP = x.shape
        CoutP, npix = dy.shape[3], _npix(x)
        Cout, Cin = weight.shape[0], weight.shape[1]
        nslab = L.query("egm_conv1x1_bwd_slabs", npix)
        ws = torch.empty(nslab * CoutP * CinP + 4, dtype=torch.float32, device=x.device)
        gx = torch.empty((N, H, W, CinP), dtype=x.dtype, device=x.device) if need_gx else None
        gw = torch.empty_like(weight)
        descs.append(_C1_DESC.pack(x.data_ptr(), dy.data_ptr(), wd.data_ptr(), 0 if gx is None else gx.data_ptr(), ws.data_ptr(), npix, ldx, lddy,
                                   CinP, CinP, CoutP, 0))
        if defer:
            _queue_wgrad(ws, weight, nslab, 1, CoutP, CinP, Cout, Cin, 1, gw, defer)
        else:
            now.append((ws, gw, nslab, CoutP, CinP, Cout, Cin))
        res.append((gx, gw))
    L.call("egm_conv1x1_bwd", dt, b"".join(descs), len(descs), st)
    for ws, gw, nslab, CoutP, CinP, Cout, Cin in now:
        L.call("egm_wgrad_reduce", ptr(ws), ptr(gw), nslab, 1, CoutP, CinP, Cout, Cin, 1, 0, st)
    return res


def _conv_grads(x, ldx, dy, weight, wd, dil, groups, Cin, Cout, need_gx, need_gw, x_split=0, c1=True):
    """(data gradient, weight gradient) of a conv from a materialised dy [N, H, W, CoutP] (contiguous): one fused launch for a 1x1 conv
    whose weight gradient is deferrable (c1=False: never, the caller's launch sequence is the pair), the weight-gradient slab kernel
    followed by the data-gradient conv otherwise."""
    N, H, W, CinP = x.shape
    CoutP = dy.shape[3]
    if c1 and need_gw and not x_split and _c1_shape_ok(x, dy, weight, dil, groups):
        return _conv1x1_bwd([(x, ldx, dy, CoutP, weight, wd, need_gx, _wgrad_deferrable(weight))])[0]
    gx = gw = None
    if need_gw:
        gw = _conv_wgrad(x, ldx, dy, CoutP, weight, dil, groups, Cin, Cout)
    if need_gx:
        gx = _conv_dgrad(dy, wd, N, H, W, CoutP, CinP, weight.shape[2], weight.shape[3], dil, x_split)
    return gx, gw


def _conv_wgrad(x, ldx, gy, ldg, weight, dil, groups, Cin, Cout, defer=None):
    """Weight gradient of one conv; deferred slab reduction when that is safe."""
    N, H, W, CinP = x.shape
    CoutP = gy.shape[3]
    KH, KW = weight.shape[2], weight.shape[3]
    L, dt, st = lib(), dtype_code(x.dtype), stream()
    gw = torch.empty_like(weight)
    nbytes = L.query("egm_conv_wgrad_workspace", N, H, W, CinP, CoutP, KH, KW)
    ws = torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=x.device)
    if defer is None:                     # (a caller that asked already -- _wgrad_deferrable consumes the use note -- passes the answer)
        defer = _wgrad_deferrable(weight)
    if defer and merge_wgrads.on:
        # nothing reads the slabs before the end-of-backward reduction: the launch itself waits for it too and shares launches with the
        # other deferred ones (_BackwardRun.launch_slabs); x and gy stay alive in the queue entry
        _run().slabs.append(_Slab(dt, x, ldx, gy, ldg, ws, N, H, W, CinP, CoutP, Cin, Cout, KH, KW, dil, groups))
    else:
        L.call("egm_conv_wgrad", dt, ptr(x), ldx, ptr(gy), ldg, None if defer else ptr(gw), ptr(ws), N, H, W, CinP, CoutP, Cin, Cout, KH, KW,
               dil, groups, 0, st)
    if defer:
        nslab = L.query("egm_conv_wgrad_slabs", dt, N, H, W, CinP, CoutP, KH, KW, dil)
        _queue_wgrad(ws, weight, nslab, KH * KW, CoutP, CinP, Cout, Cin, groups, gw, defer)
    return gw


def _dz_fusable(C):
    return fuse_dz.on and C % 8 == 0 and C <= 1024 and 256 % (C // 8) == 0


class _Conv2d(Function):
    """nn.Conv2d (stride 1, same padding) on NHWC activations; weight stays the fp32 OIHW nn.Parameter."""

    @staticmethod
    def forward(ctx, x, weight, bias, dil, groups, want_stats, bias_grad_zero=False, defer_dgrad=False):
        x, ldx = _nhwc(x)
        Cout, Cin_g = weight.shape[0], weight.shape[1]
        y, stats, wd = _conv_forward(x, ldx, weight, bias, dil, groups, want_stats)
        if ctx.needs_input_grad[1]:
            _note_conv_use(weight)
        ctx.save_for_backward(x, weight, wd)
        ctx.meta = (dil, groups, bias is not None, Cin_g * groups, Cout)
        ctx.bias_grad_zero = bias_grad_zero
        ctx.bias = bias                                 # (a leaf parameter: looked at in backward for the deferred bias gradient)
        # the caller vouches that x is the materialised output of a conv -> BatchNorm(+act) node and has no other consumer
        ctx.defer_dgrad = bool(defer_dgrad and weight.shape[2] == 1 and weight.shape[3] == 1 and groups == 1
                               and Cout <= 8 and weight.is_contiguous() and _dz_fusable(x.shape[3]))
        ctx.set_materialize_grads(False)                # no zero-filled "gradient" for the non-differentiable stats output
        if want_stats:
            ctx.mark_non_differentiable(stats)
            return y, stats
        return y

    @staticmethod
    def backward(ctx, gy, *_):
        if gy is None:
            return (None,) * 8
        x, weight, wd = ctx.saved_tensors
        dil, groups, has_bias, Cin, Cout = ctx.meta
        gy, ldg = _nhwc(gy)
        x, ldx = _nhwc(x)
        N, H, W, CinP = x.shape
        CoutP = gy.shape[3]
        KH, KW = weight.shape[2], weight.shape[3]
        L, dt, st = lib(), dtype_code(x.dtype), stream()
        gx = gw = gb = None
        need_gx, need_gw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_gb = has_bias and ctx.needs_input_grad[2]
        # (consumes the weight's use note: asked once per backward.  True, or the _Derived record of a derived weight that defers)
        defer = _wgrad_deferral(weight, ctx.bias if want_gb and not ctx.bias_grad_zero else None) if need_gw else False
        if want_gb:
            if ctx.bias_grad_zero:
                gb = _zero_grad_vec(Cout, x.device)
            elif defer is not True and defer and _derived_of(ctx.bias) is not None:
                gb = _queue_derived_bgrad(gy, Cout, _derived_of(ctx.bias))                  # the merged bias: its three real biases from one pass over gy
            else:
                gb = _bias_grad(gy, Cout, ctx.bias, bool(defer))
        if need_gw and not (need_gx and ctx.defer_dgrad and fuse_dz.on) and _c1_shape_ok(x, gy, weight, dil, groups):
            # 1x1: data gradient + weight-gradient slabs from ONE pass over gy and x
            gx, gw = _conv1x1_bwd([(x, ldx, gy, ldg, weight, wd, need_gx, defer)])[0]
            return gx, gw, gb, None, None, None, None, None
        if need_gx:
            gx = torch.empty((N, H, W, CinP), dtype=x.dtype, device=x.device)
            if ctx.defer_dgrad and fuse_dz.on:
                # never written: the BatchNorm backward in front computes dz = gy * W per vector itself (egm_bn_cls_bwd_*)
                _defer_dz(gx, ("cls", gy, ldg, weight.detach(), Cout, Cin))
            else:
                L.call("egm_conv_fwd", dt, ptr(gy), ldg, ptr(wd), None, 0, ptr(gx), CinP, None, N, H, W, CoutP, CinP, KH, KW, dil, st)
        if need_gw and gw is None:
            gw = _conv_wgrad(x, ldx, gy, ldg, weight, dil, groups, Cin, Cout, defer=defer)
        return gx, gw, gb, None, None, None, None, None


def conv2d(x, weight, bias=None, dil=1, groups=1, want_stats=False, bias_grad_zero=False, defer_dgrad=False):
    """x: NHWC tensor (a Lazy is materialised first).
    defer_dgrad: x is the materialised result of ops.conv_bn_act and feeds nothing else -- a 1x1 conv to <= 8 channels (the classifier)
    then leaves its data gradient to that BatchNorm's backward (see _defer_dz)."""
    return _Conv2d.apply(materialize(x), weight, bias, dil, groups, want_stats, bias_grad_zero, defer_dgrad)


def _conv_dgrad(dy, wd, N, H, W, CoutP, CinP, KH, KW, dil, x_split):
    """Data gradient of a conv from dy [N,H,W,CoutP] (contiguous).  x_split > 0: written as two dense tensors (the gradients of the
    two concatenated inputs) when the kernel supports it; the returned tensor is then a never-written stand-in registered for the
    concat's backward."""
    L, dt, st = lib(), dtype_code(dy.dtype), stream()
    gx = torch.empty((N, H, W, CinP), dtype=dy.dtype, device=dy.device)
    if x_split and fuse_dz.on and L.cdll.egm_conv_split_ok(dt, N, H, W, CoutP, CinP, KH, KW, dil, x_split):
        ga = torch.empty((N, H, W, x_split), dtype=dy.dtype, device=dy.device)
        gb = torch.empty((N, H, W, CinP - x_split), dtype=dy.dtype, device=dy.device)
        L.call("egm_conv_fwd_split", dt, ptr(dy), CoutP, ptr(wd), ptr(ga), x_split, ptr(gb), CinP - x_split, x_split, N, H, W, CoutP, CinP,
               KH, KW, dil, st)
        _defer_dz(gx, ("split", ga, gb))
    else:
        L.call("egm_conv_fwd", dt, ptr(dy), CoutP, ptr(wd), None, 0, ptr(gx), CinP, None, N, H, W, CoutP, CinP, KH, KW, dil, st)
    return gx


fuse_cls = _Switch("EGM_FUSE_CLS", "1",
                   """Get / set whether the 1x1 classifier runs inside the BatchNorm apply pass of the layer in front (tests compare both ways).""")


class _BnActCls(Function):
    """Lazy (conv -> BatchNorm -> act stand-in) -> 1x1 classifier -> fp32 NCHW logits as ONE node (OutConv behind up4's DoubleConv,
    src/EGM-UNet.py:952-956 + :1536-1540): the BatchNorm apply pass writes z (kept for the classifier's weight gradient) and computes
    the logits from it (egm_bn_act_cls_fwd).  backward: classifier weight / bias gradients from (z, dlogits); the data gradient is
    left to the BatchNorm backward in front (_defer_dz "cls") or, with that switched off, computed by the conv kernel."""

    @staticmethod
    def forward(ctx, y, coef, act, weight, bias):
        y, ldy = _nhwc(y)
        N, H, W, C = y.shape
        nc, Cin = weight.shape[0], weight.shape[1]
        L, dt, st, dev = lib(), dtype_code(y.dtype), stream(), y.device
        z = torch.empty((N, H, W, C), dtype=y.dtype, device=dev)
        logits = torch.empty((N, nc, H, W), dtype=torch.float32, device=dev)
        L.call("egm_bn_act_cls_fwd", dt, ptr(y), ldy, ptr(coef[0]), ptr(coef[1]), act, ptr(z), C, ptr(weight.detach()), nc, Cin,
               ptr(bias.detach()) if bias is not None else None, ptr(logits), N, H, W, C, st)
        if ctx.needs_input_grad[3]:
            _note_conv_use(weight)
        ctx.save_for_backward(z, weight)
        ctx.meta = (nc, Cin, bias is not None)
        ctx.bias = bias
        return logits

    @staticmethod
    def backward(ctx, g):
        z, weight = ctx.saved_tensors
        nc, Cin, has_bias = ctx.meta
        N, H, W, C = z.shape
        L, dt, st, dev = lib(), dtype_code(z.dtype), stream(), z.device
        g = g.contiguous().float()
        dl = torch.empty((N, H, W, 8), dtype=z.dtype, device=dev)            # NHWC, channels nc..7 zero-filled
        L.call("egm_nchw_to_nhwc", dt, ptr(g), ptr(dl), 8, N, nc, H, W, st)
        gy = gw = gb = None
        defer = _wgrad_deferrable(weight) if ctx.needs_input_grad[3] else False
        if ctx.needs_input_grad[3]:
            gw = _conv_wgrad(z, C, dl, 8, weight, 1, 1, Cin, nc, defer=defer)
        if has_bias and ctx.needs_input_grad[4]:
            gb = _bias_grad(dl, nc, ctx.bias, defer)
        if ctx.needs_input_grad[0]:
            gy = torch.empty((N, H, W, C), dtype=z.dtype, device=dev)
            if fuse_dz.on and _dz_fusable(C):
                _defer_dz(gy, ("cls", dl, 8, weight.detach(), nc, Cin))     # never written: see _defer_dz
            else:
                _, wd = _packed_weights(weight, 1, z.dtype)
                L.call("egm_conv_fwd", dt, ptr(dl), 8, ptr(wd), None, 0, ptr(gy), C, None, N, H, W, 8, C, 1, 1, 1, st)
        return gy, None, None, gw, gb


def bn_act_cls_ok(x, weight):
    """True when ops.bn_act_cls applies: x an ops.Lazy, a 1x1 classifier to <= 8 classes, channel count a power of two <= 512."""
    C = x.shape[3] if isinstance(x, Lazy) else 0
    return (fuse_cls.on and isinstance(x, Lazy) and weight.dim() == 4 and weight.shape[2] == 1 and weight.shape[3] == 1 and weight.shape[0] <= 8
            and pad8(weight.shape[1]) == C and C % 8 == 0 and C // 8 <= 64 and (C // 8) & (C // 8 - 1) == 0 and weight.is_contiguous())


def bn_act_cls(x, weight, bias):
    """Lazy x -> fp32 NCHW logits of the 1x1 classifier (weight, bias); x's only consumer."""
    return _BnActCls.apply(x.y, x.coef, x.act, weight, bias)


# ----------------------------------------------------------------------------------------------------------
# conv -> BatchNorm (+ activation): the steps every such node shares
# ----------------------------------------------------------------------------------------------------------
def _bn_step(bn):
    """The per-forward bookkeeping of an nn.BatchNorm2d used as the parameter / buffer holder: bumps num_batches_tracked (an int64
    counter, as nn.BatchNorm2d does; not where a graphed step keeps it) -> (training, momentum) for the kernels."""
    if bn.training and bn.num_batches_tracked is not None and not getattr(bn, "_egm_counter_managed", False):
        bn.num_batches_tracked.add_(1)
    return bn.training or bn.running_mean is None, 0.1 if bn.momentum is None else bn.momentum


def _rows(coef):
    return ptr(coef[0]), ptr(coef[1]), ptr(coef[2]), ptr(coef[3])


def _bn_coef(stats, npix, gamma, beta, running_mean, running_var, eps, momentum, training, CP, C, dev):
    """-> coef, fp32 [4, CP] rows scale | shift | save_mean | save_rstd (see Lazy): from the per-tile batch statistics `stats` when
    training (the running statistics are updated on the way), from the running statistics otherwise."""
    L, coef = lib(), _f32((4, CP), dev)
    if training:
        L.call("egm_bn_finalize", ptr(stats), stats.shape[0], npix, ptr(gamma.detach()), ptr(beta.detach()), eps, momentum,
               ptr(running_mean), ptr(running_var), *_rows(coef), CP, C, stream())
    else:
        L.call("egm_bn_eval_coeffs", ptr(gamma.detach()), ptr(beta.detach()), ptr(running_mean), ptr(running_var), eps, *_rows(coef), CP, C,
               stream())
    return coef


def _bn_bwd_buffers(y, nb=None):
    """The temporaries of a BatchNorm backward over the conv output y -> (nb, part, sums, cf4, dy): `nb` blocks write their partial sums
    to `part`; sums = fp32 [2, CP] rows sum(dz) | sum(dz * xhat), which are dbeta | dgamma; cf4 the per-channel coefficients of dy."""
    CP, dev = y.shape[3], y.device
    if nb is None:
        nb = lib().query("egm_channel_partials_blocks", _npix(y), CP)
    return nb, _f32(nb * 2 * CP, dev), _f32((2, CP), dev), _f32((4, CP), dev), torch.empty(tuple(y.shape), dtype=y.dtype, device=dev)


def _bn_backward(family, lead, geo, y, coef, act, training, nb=None):
    """What a conv -> BatchNorm node does in backward before the conv's own gradients: partial sums over (dz, y) -> egm_bn_bwd_coefs ->
    dy in one apply pass.  -> (dy, sums).  The kernel family says where dz comes from: `family` is the entry-point prefix, `lead` its
    leading arguments (the dtype and the tensors dz is read or computed from), `geo` its trailing geometry arguments:
        egm_bn_act   dz is a tensor                                           (dt, dz, lddz)                      (npix, CP)
        egm_bn_pool  dz = gskip + scatter(gpool), see _ConvBNPool             (dt, gskip, ldg, gpool, ldp)        (N, H, W, CP)
        egm_bn_cls   dz = dlogits * W, see _defer_dz "cls"                    (dt, dl, lddl, w, nc, ldw)          (npix, CP)
        egm_bn_mca   dz from the MCALayer's gates, see _defer_dz "mca"        (dt, dxo, ld, gates, mcoef, ns)     geometry + (CP,)
    nb: the number of partial-sum blocks where the family has a decomposition of its own (egm_bn_pool_bwd_blocks)."""
    L, st = lib(), stream()
    y, ldy = _nhwc(y)
    CP, npix = y.shape[3], _npix(y)
    nb, part, sums, cf4, dy = _bn_bwd_buffers(y, nb)
    rows, train = _rows(coef), 1 if training else 0
    L.call(family + "_bwd_reduce", *lead, ptr(y), ldy, *rows, act, ptr(part), *geo, st)
    L.call("egm_bn_bwd_coefs", ptr(part), nb, npix, *rows, train, ptr(sums), ptr(cf4), CP, st)
    L.call(family + "_bwd_apply", *lead, ptr(y), ldy, *rows, act, train, ptr(sums), ptr(dy), CP, *geo, st)
    return dy, sums


def _conv_bn_grads(need, x, ldx, dy, weight, wd, sums, dil, groups, has_bias, Cin, Cout, training, x_split=0, c1=True, conv_grads=None):
    """The tail of a conv -> BatchNorm backward: (gx, gw, gb, ggamma, gbeta) from the conv's gradient dy and the BatchNorm's `sums`.
    need: needs_input_grad of (x, weight, bias, gamma, beta).  conv_grads: (gx, gw) where the caller has launched them already
    (_MultiConvBN groups the launches of its members); c1 as in _conv_grads."""
    if conv_grads is None:
        conv_grads = _conv_grads(x, ldx, dy, weight, wd, dil, groups, Cin, Cout, need[0], need[1], x_split, c1)
    gx, gw = conv_grads
    gb = _bn_conv_bias_grad(Cout, dy, training, dy.device) if (has_bias and need[2]) else None
    return gx, gw, gb, sums[1, :Cout] if need[3] else None, sums[0, :Cout] if need[4] else None


class _ConvBN(Function):
    """conv -> BatchNorm (-> act, applied by whoever consumes the result) as ONE autograd node.

    forward : y = conv(x) with the BN statistics from the conv epilogue; egm_bn_finalize -> coef.  Returns the RAW conv output y as the
              stand-in of the logical z = act(scale*y + shift), and coef (see Lazy).
    backward: receives dL/dz (or a stand-in whose producer left dz to this node, see _defer_dz).  Partial sums (dz, y) ->
              egm_bn_bwd_coefs -> dy in one apply pass -> the conv's weight and data gradients."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, eps, momentum, act, training, dil, groups, x_split=0):
        """x_split = Cs > 0: x is a channel concatenation [Cs | rest] with no other consumer (ops.upcat): backward writes the gradient
        as two dense tensors where the kernel can (egm_conv_fwd_split) and hands them to the concat's backward (see _defer_dz)."""
        x, ldx = _nhwc(x)
        ctx.x_split = int(x_split) if (x_split and 0 < x_split < x.shape[3] and x_split % 8 == 0) else 0
        Cout, Cin_g = weight.shape[0], weight.shape[1]
        y, stats, wd = _conv_forward(x, ldx, weight, bias, dil, groups, training)
        coef = _bn_coef(stats, _npix(y), gamma, beta, running_mean, running_var, eps, momentum, training, y.shape[3], Cout, y.device)
        if ctx.needs_input_grad[1]:
            _note_conv_use(weight)
        ctx.save_for_backward(x, weight, wd, y, coef)
        ctx.meta = (dil, groups, bias is not None, Cin_g * groups, Cout, act, training)
        ctx.mark_non_differentiable(coef)
        ctx.set_materialize_grads(False)
        return y, coef

    @staticmethod
    def backward(ctx, gz, _):
        if gz is None:
            return (None,) * 14
        x, weight, wd, y, coef = ctx.saved_tensors
        dil, groups, has_bias, Cin, Cout, act, training = ctx.meta
        pend = _take_dz(gz)                                  # not None: gz is a stand-in, dz comes from its producer's inputs
        gz, ldg = _nhwc(gz)
        x, ldx = _nhwc(x)
        CoutP, npix, dt = y.shape[3], _npix(y), dtype_code(x.dtype)
        if pend is None:
            family = ("egm_bn_act", (dt, ptr(gz), ldg), (npix, CoutP))
        elif pend[1][0] == "cls":
            _, dl, lddl, wcls, nc, ldw = pend[1]
            family = ("egm_bn_cls", (dt, ptr(dl), lddl, ptr(wcls), nc, ldw), (npix, CoutP))
        else:
            _, dxo, ldd, gates, mcoef, ns, geo = pend[1]
            family = ("egm_bn_mca", (dt, ptr(dxo), ldd, ptr(gates), ptr(mcoef), ns), geo + (CoutP,))
        dy, sums = _bn_backward(*family, y, coef, act, training)
        return _conv_bn_grads(ctx.needs_input_grad, x, ldx, dy, weight, wd, sums, dil, groups, has_bias, Cin, Cout, training,
                              ctx.x_split) + (None,) * 9


fuse_mca_bwd = _Switch("EGM_FUSE_MCA_BWD", "1",
                       """Get / set whether the MCALayer backward computes du and dxo in one tiled launch (bf16; egm_mca_bwd_dudxo).""")


fuse_mca_bn = _Switch("EGM_FUSE_MCA_BN", "1",
                      """Get / set whether the BatchNorm+ReLU in front of an MCALayer is applied by the layer's statistics pass
                      (egm_mca_reduce_bn).""")


# the max pool at a skip connection fused into its producer / consumer (csrc/pool_fused.hip)
fuse_pool = _Switch("EGM_FUSE_POOL", "1",
                    """Get / set whether the skip-connection max pool is fused into the kernels on either side of it (tests compare both
                    ways).""")


class _ConvBNPool(Function):
    """conv -> BatchNorm -> act -> (z for the skip connection, maxpool2(z)) as ONE autograd node (the encoder's top level:
    src/EGM-UNet.py:44-55 followed by :908).  forward: the BatchNorm apply writes z and the pooled tensor in one pass
    (egm_bn_act_fwd_pool).  backward: receives the skip gradient and the pooled gradient; the BatchNorm backward passes compute
    dz = gskip + scatter(gpool) on the fly (egm_bn_pool_bwd_*), so the pool's scatter pass and the tensor it wrote do not exist."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, eps, momentum, act, training, dil, groups, out_slot):
        x, ldx = _nhwc(x)
        Cout, Cin_g = weight.shape[0], weight.shape[1]
        y, stats, wd = _conv_forward(x, ldx, weight, bias, dil, groups, training)
        N, H, W, CoutP = y.shape
        L, dt, st, dev = lib(), dtype_code(y.dtype), stream(), y.device
        coef = _bn_coef(stats, _npix(y), gamma, beta, running_mean, running_var, eps, momentum, training, CoutP, Cout, dev)
        z, ldz = _slot_or_new(out_slot, (N, H, W, CoutP), y.dtype, dev)
        pooled = torch.empty((N, H // 2, W // 2, CoutP), dtype=y.dtype, device=dev)
        L.call("egm_bn_act_fwd_pool", dt, ptr(y), CoutP, ptr(coef[0]), ptr(coef[1]), act, ptr(z), ldz, ptr(pooled), CoutP, N, H, W, CoutP, st)
        if ctx.needs_input_grad[1]:
            _note_conv_use(weight)
        ctx.save_for_backward(x, weight, wd, y, coef, z)
        ctx.meta = (dil, groups, bias is not None, Cin_g * groups, Cout, act, training)
        ctx.set_materialize_grads(False)
        return z, pooled

    @staticmethod
    def backward(ctx, gz, gpool):
        if gz is None and gpool is None:
            return (None,) * 14
        x, weight, wd, y, coef, z = ctx.saved_tensors
        dil, groups, has_bias, Cin, Cout, act, training = ctx.meta
        x, ldx = _nhwc(x)
        N, H, W, CoutP = y.shape
        L, dt = lib(), dtype_code(x.dtype)
        if gz is not None and gpool is not None:
            gz, ldg = _nhwc(gz)
            gpool, ldp = _nhwc(gpool)
            family = ("egm_bn_pool", (dt, ptr(gz), ldg, ptr(gpool), ldp), (N, H, W, CoutP))
            nb = L.query("egm_bn_pool_bwd_blocks", N, H, W, CoutP)
        else:
            # only one of the two consumers produced a gradient: the separate kernels
            if gz is None:
                zk, ldzk = _nhwc(z)
                gpool, ldp = _nhwc(gpool)
                gz = torch.empty((N, H, W, CoutP), dtype=x.dtype, device=y.device)
                L.call("egm_maxpool2_bwd", dt, ptr(zk), ldzk, ptr(gpool), ldp, ptr(gz), CoutP, N, H, W, CoutP, stream())
            gz, ldg = _nhwc(gz)
            family, nb = ("egm_bn_act", (dt, ptr(gz), ldg), (_npix(y), CoutP)), None
        dy, sums = _bn_backward(*family, y, coef, act, training, nb)
        # c1=False: this node issues the weight-gradient kernel and the data-gradient conv for a 1x1 conv too, never the fused launch
        return _conv_bn_grads(ctx.needs_input_grad, x, ldx, dy, weight, wd, sums, dil, groups, has_bias, Cin, Cout, training,
                              c1=False) + (None,) * 9


def conv_bn_lazy(x, conv, bn, act, dil=1, groups=1):
    """conv -> BatchNorm -> activation as an ops.Lazy: for a consumer whose first pass materialises the tensor itself (ops.mca_layer:
    BatchNorm apply + the three-axis statistics in one pass)."""
    if _fold_packs() is not None:
        return _fold_conv(x, conv, act, dil)            # folded: the layer's statistics pass reads the finished tensor
    training, momentum = _bn_step(bn)
    y, coef = _ConvBN.apply(materialize(x), conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, momentum, act,
                            training, dil, groups)
    return Lazy(y, coef, act)


def conv_bn_act_pool(x, conv, bn, act, dil=1, groups=1, out=None):
    """conv -> BatchNorm -> activation -> (result, maxpool2(result)): the skip-connection tensor (into the destination view `out` when
    given) and its pooled copy from one BatchNorm apply pass, one autograd node (see _ConvBNPool).  H and W must be even; callers fall
    back to conv_bn_act + fork_maxpool2 otherwise (pool_fusable)."""
    if _fold_packs() is not None:
        z = _fold_conv(x, conv, act, dil, out)
        return z, maxpool2(z)
    training, momentum = _bn_step(bn)
    x = materialize(x)
    return _ConvBNPool.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, momentum, act,
                             training, dil, groups, None if out is None else [out])


def pool_fusable(x):
    """True when the fused skip-connection pool applies to the NHWC tensor / Lazy x (switch on, even H and W, <= 1024 channels)."""
    return fuse_pool.on and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0 and x.shape[1] >= 2 and x.shape[2] >= 2 and x.shape[3] <= 1024


# ----------------------------------------------------------------------------------------------------------
# BatchNorm (+ activation)
# ----------------------------------------------------------------------------------------------------------
class _BnAct(Function):
    @staticmethod
    def forward(ctx, y, stats, gamma, beta, running_mean, running_var, eps, momentum, act, training, out_slot=None):
        y, ldy = _nhwc(y)
        N, H, W, CP = y.shape
        C, npix, dev = gamma.shape[0], _npix(y), y.device
        L, dt, st = lib(), dtype_code(y.dtype), stream()
        if training and stats is None:
            nb = L.query("egm_channel_partials_blocks", npix, CP)
            stats = _f32((nb, 2, CP), dev)
            L.call("egm_channel_sums", dt, ptr(y), ldy, npix, CP, ptr(stats), st)
        coef = _bn_coef(stats, npix, gamma, beta, running_mean, running_var, eps, momentum, training, CP, C, dev)
        z, ldz = _slot_or_new(out_slot, (N, H, W, CP), y.dtype, dev)
        L.call("egm_bn_act_fwd", dt, ptr(y), ldy, ptr(coef[0]), ptr(coef[1]), act, ptr(z), ldz, npix, CP, st)
        ctx.save_for_backward(y, coef)
        ctx.meta = (act, training, C)
        return z

    @staticmethod
    def backward(ctx, gz):
        y, coef = ctx.saved_tensors
        act, training, C = ctx.meta
        gz, ldg = _nhwc(gz)
        y, ldy = _nhwc(y)
        N, H, W, CP = y.shape
        npix, dev = _npix(y), y.device
        L, dt, st = lib(), dtype_code(y.dtype), stream()
        # the egm_bn_act family without _bn_backward: no conv behind it, so the sums need no egm_bn_bwd_coefs (egm_reduce_tiles), and
        # the apply pass runs only when the input wants a gradient
        rows = _rows(coef)
        nb = L.query("egm_channel_partials_blocks", npix, CP)
        part = _f32(nb * 2 * CP, dev)
        sums = _f32((2, CP), dev)
        L.call("egm_bn_act_bwd_reduce", dt, ptr(gz), ldg, ptr(y), ldy, *rows, act, ptr(part), npix, CP, st)
        L.call("egm_reduce_tiles", ptr(part), nb, CP, ptr(sums), st)
        gy = None
        if ctx.needs_input_grad[0]:
            gy = torch.empty((N, H, W, CP), dtype=y.dtype, device=dev)
            L.call("egm_bn_act_bwd_apply", dt, ptr(gz), ldg, ptr(y), ldy, *rows, act, 1 if training else 0, ptr(sums), ptr(gy), CP, npix, CP, st)
        ggamma = sums[1, :C] if ctx.needs_input_grad[2] else None
        gbeta = sums[0, :C] if ctx.needs_input_grad[3] else None
        return gy, None, ggamma, gbeta, None, None, None, None, None, None, None


# ----------------------------------------------------------------------------------------------------------
# several independent conv -> BatchNorm(+act) layers as one autograd node with multi-tensor BatchNorm passes
# ----------------------------------------------------------------------------------------------------------
BN_MULTI_MAX = 4
_BN_FINALIZE, _BN_FWD, _BN_BWD_REDUCE, _BN_BWD_COEFS, _BN_BWD_APPLY = range(5)    # enum egm_bn_multi_pass
fuse_bn_multi = _Switch("EGM_BN_MULTI", "1")


def _bn_desc(y=None, z=None, dz=None, dy=None, coef=None, stats=None, gamma=None, beta=None, rm=None, rv=None, partials=None, sums=None,
             cf4=None, npix=0, ldy=0, ldz=0, lddz=0, lddy=0, ntiles=0, nblocks=0, C=0, C_real=0, act=0, train=0, eps=0.0, momentum=0.0):
    """one packed egm_bn_desc (include/egm_hip.h)"""
    dp = lambda t: 0 if t is None else t.data_ptr()
    return struct.pack("<13Qq10i2f", dp(y), dp(z), dp(dz), dp(dy), dp(coef), dp(stats), dp(gamma), dp(beta), dp(rm), dp(rv), dp(partials),
                       dp(sums), dp(cf4), npix, ldy, ldz, lddz, lddy, ntiles, nblocks, C, C_real, act, train, eps, momentum)


# one member of a _MultiConvBN node in backward; need: needs_input_grad of its (x, weight, bias, gamma, beta)
_Member = namedtuple("_Member", "x ldx weight wd dy sums need alive")


class _MultiConvBN(Function):
    """K <= 4 INDEPENDENT conv -> BatchNorm -> activation layers (the parallel branches of EdgeEnhancedGRFB at equal depth) as one
    autograd node: the K convolutions are launched back to back, then ONE finalize launch and ONE apply launch serve all K BatchNorms;
    backward: ONE partial-sum launch, ONE coefficient launch, ONE apply launch, then the K data and weight gradients.  Every tensor
    goes through exactly the arithmetic of conv_bn_act (same kernels' bodies, same block decomposition), so results are bit-identical
    to K separate nodes; what disappears is 2 x (K - 1) forward and 3 x (K - 1) backward launches of 5 us each on tensors whose
    passes take about as long as a launch."""

    @staticmethod
    def forward(ctx, meta, *flat):
        K = len(meta)
        L, st = lib(), stream()
        saved, descs_fin, descs_fwd, outs, keep = [], b"", b"", [], []
        ctx.meta = []
        convs = []
        with conv_group():                                    # the K convolutions: one launch per kernel instantiation
            for k, mk in enumerate(meta):
                x, weight, bias = flat[5 * k:5 * k + 3]
                x, ldx = _nhwc(x)
                convs.append((x, ldx) + _conv_forward(x, ldx, weight, bias, mk[6], mk[7], mk[5]))
        for k, mk in enumerate(meta):
            x, weight, bias, gamma, beta = flat[5 * k:5 * k + 5]
            rm, rv, eps, momentum, act, training, dil, groups, out_slot = mk
            Cout, Cin_g = weight.shape[0], weight.shape[1]
            x, ldx, y, stats, wd = convs[k]
            CoutP, npix, dev = y.shape[3], _npix(y), y.device
            if training:                                      # one finalize launch for all members (below) instead of _bn_coef's
                coef = _f32((4, CoutP), dev)
                descs_fin += _bn_desc(coef=coef, stats=stats, gamma=gamma.detach(), beta=beta.detach(), rm=rm, rv=rv, npix=npix,
                                      ntiles=stats.shape[0], C=CoutP, C_real=Cout, eps=eps, momentum=momentum)
                keep.append(stats)
            else:
                coef = _bn_coef(None, npix, gamma, beta, rm, rv, eps, momentum, False, CoutP, Cout, dev)
            z, ldz = _slot_or_new(out_slot, tuple(y.shape), y.dtype, dev)
            descs_fwd += _bn_desc(y=y, z=z, coef=coef, npix=npix, ldy=CoutP, ldz=ldz, C=CoutP, act=act)
            if ctx.needs_input_grad[1 + 5 * k + 1]:
                _note_conv_use(weight)
            saved += [x, weight, wd, y, coef]
            outs.append(z)
            ctx.meta.append((dil, groups, bias is not None, Cin_g * groups, Cout, act, training))
        dt = dtype_code(outs[0].dtype)
        if descs_fin:
            L.call("egm_bn_multi", dt, _BN_FINALIZE, descs_fin, len(descs_fin) // 160, st)
        L.call("egm_bn_multi", dt, _BN_FWD, descs_fwd, K, st)
        ctx.save_for_backward(*saved)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gz):
        K = len(ctx.meta)
        L, st = lib(), stream()
        sv = ctx.saved_tensors
        mem, d_red, d_coef, d_app = [], b"", b"", b""
        for k in range(K):
            x, weight, wd, y, coef = sv[5 * k:5 * k + 5]
            dil, groups, has_bias, Cin, Cout, act, training = ctx.meta[k]
            g, ldg = _nhwc(gz[k])
            x, ldx = _nhwc(x)
            CoutP = y.shape[3]
            nb, part, sums, cf4, dy = _bn_bwd_buffers(y)
            common = dict(y=y, dz=g, coef=coef, partials=part, sums=sums, cf4=cf4, npix=_npix(y), ldy=CoutP, lddz=ldg, nblocks=nb, C=CoutP,
                          act=act, train=1 if training else 0)
            d_red += _bn_desc(**common)
            d_coef += _bn_desc(**common)
            d_app += _bn_desc(dy=dy, lddy=CoutP, **common)
            # every temporary stays referenced (`alive`) until the launches that use it are enqueued (freed earlier, the caching
            # allocator would hand its memory to the next layer's temporaries: the kernels are not in the stream yet)
            mem.append(_Member(x, ldx, weight, wd, dy, sums, ctx.needs_input_grad[1 + 5 * k:6 + 5 * k], (g, part, cf4)))
        dt = dtype_code(mem[0].x.dtype)
        L.call("egm_bn_multi", dt, _BN_BWD_REDUCE, d_red, K, st)
        L.call("egm_bn_multi", dt, _BN_BWD_COEFS, d_coef, K, st)
        L.call("egm_bn_multi", dt, _BN_BWD_APPLY, d_app, K, st)
        gxs, gws = [None] * K, [None] * K
        # the 1x1 members (deferrable weight gradients): data gradient + weight-gradient slabs of all of them in ONE fused launch
        fused = [k for k, m in enumerate(mem) if m.need[1] and _c1_shape_ok(m.x, m.dy, m.weight, ctx.meta[k][0], ctx.meta[k][1])]
        if fused:
            res = _conv1x1_bwd([(m.x, m.ldx, m.dy, m.dy.shape[3], m.weight, m.wd, m.need[0], _wgrad_deferrable(m.weight))
                                for m in (mem[k] for k in fused)])
            for k, r in zip(fused, res):
                gxs[k], gws[k] = r
        rest = [(k, m) for k, m in enumerate(mem) if k not in fused]
        with conv_group():                                    # the other data gradients: one launch per kernel instantiation
            for k, m in rest:
                if m.need[0]:
                    N, H, W, CinP = m.x.shape
                    gxs[k] = _conv_dgrad(m.dy, m.wd, N, H, W, m.dy.shape[3], CinP, m.weight.shape[2], m.weight.shape[3], ctx.meta[k][0], 0)
        with conv_group():                                    # ... and their weight gradients (slab kernels)
            for k, m in rest:
                dil, groups, has_bias, Cin, Cout, act, training = ctx.meta[k]
                if m.need[1]:
                    gws[k] = _conv_wgrad(m.x, m.ldx, m.dy, m.dy.shape[3], m.weight, dil, groups, Cin, Cout)
        grads = (None,)
        for k, m in enumerate(mem):
            dil, groups, has_bias, Cin, Cout, act, training = ctx.meta[k]
            grads += _conv_bn_grads(m.need, m.x, m.ldx, m.dy, m.weight, m.wd, m.sums, dil, groups, has_bias, Cin, Cout, training,
                                    conv_grads=(gxs[k], gws[k]))
        return grads


def multi_conv_bn_act(items):
    """items: K <= 4 tuples (x, conv, bn, act, dil, groups, out) of INDEPENDENT layers (x: NHWC tensor or Lazy) -> list of K outputs.
    With the BatchNorm passes shared between the layers (_MultiConvBN); falls back to K conv_bn_act calls when disabled or K == 1."""
    if _fold_packs() is not None:
        with conv_group():                                # folded: the K convolutions are all there is, one launch per instantiation
            return [_fold_conv(x, conv, act, dil, out) for x, conv, bn, act, dil, groups, out in items]
    if not fuse_bn_multi.on or len(items) == 1 or len(items) > BN_MULTI_MAX:
        return [conv_bn_act(x, conv, bn, act, dil=dil, groups=groups, out=out) for x, conv, bn, act, dil, groups, out in items]
    meta, flat = [], []
    for x, conv, bn, act, dil, groups, out in items:
        training, momentum = _bn_step(bn)
        meta.append((bn.running_mean, bn.running_var, bn.eps, momentum, act, training, dil, groups, None if out is None else [out]))
        flat += [materialize(x), conv.weight, conv.bias, bn.weight, bn.bias]
    return list(_MultiConvBN.apply(meta, *flat))


EW_GATE, EW_SAR = 0, 1                     # enum egm_ew_mode


fuse_bn_ew = _Switch("EGM_FUSE_BN_EW", "1",
                     """Get / set whether BatchNorm + the element-wise op behind it run as the fused kernels of csrc/bn_fused.hip.""")


class _ConvBNEw(Function):
    """conv -> BatchNorm(+act) -> element-wise consumer as ONE autograd node (csrc/bn_fused.hip):
         EW_GATE  out = p*(1 + sigmoid(BN(conv(e))))       EdgeAwareFeatureEnhancer   (src/EGM-UNet.py:872-886)
         EW_SAR   out = relu(alpha*p + BN(conv(x_sc)))     EdgeEnhancedGRFB tail      (:1315-1317)
    The BatchNorm output z and its gradient dz never exist in memory: forward reads (y, p) and writes out; backward computes the
    BatchNorm partial sums from (g, p|out, y), then dy and dp in one pass, then the conv's weight and data gradients."""

    @staticmethod
    def forward(ctx, x, p, weight, bias, gamma, beta, running_mean, running_var, eps, momentum, act, training, mode, alpha, out_slot):
        x, ldx = _nhwc(x)
        p, ldp = _nhwc(p)
        Cout, Cin_g = weight.shape[0], weight.shape[1]
        y, stats, wd = _conv_forward(x, ldx, weight, bias, 1, 1, training)
        CoutP, npix, dev = y.shape[3], _npix(y), y.device
        if tuple(p.shape) != tuple(y.shape):
            raise RuntimeError(f"conv_bn_ew: element-wise operand {tuple(p.shape)} does not match the conv output {tuple(y.shape)}")
        L, dt, st = lib(), dtype_code(y.dtype), stream()
        coef = _bn_coef(stats, npix, gamma, beta, running_mean, running_var, eps, momentum, training, CoutP, Cout, dev)
        out, ldo = _slot_or_new(out_slot, tuple(y.shape), y.dtype, dev)
        L.call("egm_bn_ew_fwd", dt, mode, ptr(y), CoutP, ptr(coef[0]), ptr(coef[1]), act, ptr(p), ldp, float(alpha), ptr(out), ldo, npix,
               CoutP, st)
        if ctx.needs_input_grad[2]:
            _note_conv_use(weight)
        # GATE needs p for its backward, SAR the output (ReLU mask)
        ctx.save_for_backward(x, weight, wd, y, coef, p if mode == EW_GATE else out)
        ctx.meta = (bias is not None, Cin_g, Cout, act, training, mode, float(alpha))
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, wd, y, coef, q = ctx.saved_tensors
        has_bias, Cin, Cout, act, training, mode, alpha = ctx.meta
        g, ldg = _nhwc(g)
        x, ldx = _nhwc(x)
        q, ldq = _nhwc(q)
        CoutP, npix = y.shape[3], _npix(y)
        L, dt, st = lib(), dtype_code(x.dtype), stream()
        # the steps of _bn_backward with the egm_bn_ew kernels, whose signatures differ: alpha, the apply pass reads cf4 and writes dp too
        nb, part, sums, cf4, dy = _bn_bwd_buffers(y)
        dp = torch.empty_like(dy)
        rows = _rows(coef)
        L.call("egm_bn_ew_bwd_reduce", dt, mode, ptr(g), ldg, ptr(q), ldq, ptr(y), CoutP, *rows, act, alpha, ptr(part), npix, CoutP, st)
        L.call("egm_bn_bwd_coefs", ptr(part), nb, npix, *rows, 1 if training else 0, ptr(sums), ptr(cf4), CoutP, st)
        L.call("egm_bn_ew_bwd_apply", dt, mode, ptr(g), ldg, ptr(q), ldq, ptr(y), CoutP, ptr(cf4), act, alpha, ptr(dy), CoutP, ptr(dp),
               CoutP, npix, CoutP, st)
        need = ctx.needs_input_grad
        gx, gw, gb, ggamma, gbeta = _conv_bn_grads((need[0],) + need[2:6], x, ldx, dy, weight, wd, sums, 1, 1, has_bias, Cin, Cout, training)
        return (gx, dp if need[1] else None, gw, gb, ggamma, gbeta) + (None,) * 9


def conv_bn_ew(x, conv, bn, act, p, mode, alpha=1.0, out=None):
    """F(p, act(BN(conv(x)))) with F = EW_GATE: p*(1+z) or EW_SAR: relu(alpha*p + z); 1x1 convs (the two users in EdgeEnhancedGRFB)."""
    if conv.weight.shape[2] != 1 or conv.weight.shape[3] != 1 or conv.groups != 1:
        raise RuntimeError("conv_bn_ew: 1x1 ungrouped convolutions only")
    if _fold_packs() is not None:
        return _fold_conv_ew(x, conv, act, p, mode, alpha, out)
    if not fuse_bn_ew.on:
        z = conv_bn_act(x, conv, bn, act)
        if mode == EW_GATE:
            return gate_mul(p, z) if out is None else materialize(gate_mul(p, z), out)
        r = scale_add_relu(p, alpha, z)
        return r if out is None else materialize(r, out)
    training, momentum = _bn_step(bn)
    return _ConvBNEw.apply(materialize(x), materialize(p), conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                           momentum, act, training, mode, alpha, None if out is None else [out])


def bn_act(y, bn, act, stats=None, out=None):
    """bn: an nn.BatchNorm2d used as the parameter/buffer holder."""
    training, momentum = _bn_step(bn)
    return _BnAct.apply(y, stats, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, momentum, act, training,
                        None if out is None else [out])


def conv_bn_act(x, conv, bn, act, dil=1, groups=1, out=None, lazy=False):
    """conv -> BatchNorm -> activation (statistics from the conv epilogue).  x: NHWC tensor (a Lazy is materialised first).
    lazy="force" returns the result as a Lazy for a consumer that applies the BatchNorm in a pass of its own (MCALayer statistics, the
    classifier inside the apply pass); otherwise the result is materialised, into the destination view `out` when given."""
    if _fold_packs() is not None:
        z = _fold_conv(x, conv, act, dil, out)
        return Lazy(z, _fold_identity(z.shape[3]), ACT_NONE) if out is None and lazy == "force" else z
    training, momentum = _bn_step(bn)
    x = materialize(x)
    y, coef = _ConvBN.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, momentum, act,
                            training, dil, groups, getattr(x, "_egm_split", 0))
    z = Lazy(y, coef, act)
    if out is None and lazy == "force":                 # the consumer materialises the tensor in a pass of its own
        return z
    return z.materialize(out)


# ----------------------------------------------------------------------------------------------------------
# folded inference (egm_unet_amd/infer.py): BatchNorm folded into the conv in front of it, the activation in the conv epilogue
# ----------------------------------------------------------------------------------------------------------
_fold_state = threading.local()


class folded_inference:
    """`with folded_inference(packs):` -- on THIS thread the conv -> BatchNorm entry points (conv_bn_act, conv_bn_lazy, conv_bn_act_pool,
    conv_bn_ew, multi_conv_bn_act) run the eval-mode forward with every BatchNorm folded into its convolution.  packs: {conv holder:
    (wf, bias)} from egm_conv_fold_pack_multi, plus "identity": fp32 [4, >= C] rows 1 | 0 | 0 | 1 (written before any capture).
    No pass exists only to apply a BatchNorm: passes that fuse it with element-wise work (the EdgeAware gate, the GRFB residual tail,
    the skip pool, the classifier) keep their launch with identity coefficients or become the plain element-wise kernel.  Entered by
    infer.Predictor only; off, nothing changes."""

    def __init__(self, packs):
        self.packs, self.prev = packs, None

    def __enter__(self):
        self.prev = getattr(_fold_state, "packs", None)
        _fold_state.packs = self.packs
        return self

    def __exit__(self, *a):
        _fold_state.packs = self.prev
        return False


def _fold_packs():
    return getattr(_fold_state, "packs", None)


def _fold_identity(C):
    ident = _fold_state.packs["identity"]
    if ident.shape[1] < C:
        raise RuntimeError(f"folded_inference: identity coefficients cover {ident.shape[1]} channels, {C} needed")
    return ident[:, :C]


def _fold_conv(x, conv, act, dil=1, out=None):
    """act(conv(x) * s + b') with the folded pack of `conv` (egm_conv_fwd_act), into the destination view `out` when given"""
    hit = _fold_state.packs.get(conv)
    if hit is None:
        raise RuntimeError("folded_inference: no folded pack for this convolution (not followed by a BatchNorm in the model)")
    wf, bias = hit
    x, ldx = _nhwc(materialize(x))
    N, H, W, CinP = x.shape
    Cout, Cin_g, KH, KW = conv.weight.shape
    if pad8(Cin_g * conv.groups) != CinP:
        raise RuntimeError(f"conv_bn: input has {CinP} channels, weight expects {Cin_g * conv.groups}")
    CoutP = pad8(Cout)
    z, ldz = _slot_or_new(None if out is None else [out], (N, H, W, CoutP), x.dtype, x.device)
    lib().call("egm_conv_fwd_act", dtype_code(x.dtype), ptr(x), ldx, ptr(wf), ptr(bias), CoutP, ptr(z), ldz, N, H, W, CinP, CoutP, KH, KW,
               1 if KH == 1 and KW == 1 else dil, act, stream())
    return z


def _fold_conv_ew(x, conv, act, p, mode, alpha, out):
    """conv_bn_ew folded: the element-wise pass stays (it is real work), with identity BatchNorm coefficients"""
    y = _fold_conv(x, conv, ACT_NONE)
    p, ldp = _nhwc(materialize(p))
    if tuple(p.shape) != tuple(y.shape):
        raise RuntimeError(f"conv_bn_ew: element-wise operand {tuple(p.shape)} does not match the conv output {tuple(y.shape)}")
    CoutP = y.shape[3]
    o, ldo = _slot_or_new(None if out is None else [out], tuple(y.shape), y.dtype, y.device)
    coef = _fold_identity(CoutP)
    lib().call("egm_bn_ew_fwd", dtype_code(y.dtype), mode, ptr(y), CoutP, ptr(coef[0]), ptr(coef[1]), act, ptr(p), ldp, float(alpha), ptr(o),
               ldo, _npix(y), CoutP, stream())
    return o


def claim_prepack(st):
    """Point the packed-weight cache at the buffers of the prepack state `st` (a prepack_model state dict that is current), so the
    convolutions without a BatchNorm take exactly these buffers -- the ones a captured graph keeps reading."""
    for m, (wf, wd) in zip(st["convs"], st["bufs"]):
        w = m.weight
        _pack_cache[id(w)] = ((w.data_ptr(), w._version, _weight_generation[0], st["dtype"], m.groups, tuple(w.shape)), wf, wd, weakref.ref(w))


# ----------------------------------------------------------------------------------------------------------
# pooling / upsample + concat
# ----------------------------------------------------------------------------------------------------------
class _MaxPool2(Function):
    @staticmethod
    def forward(ctx, x):
        x, ldx = _nhwc(x)
        N, H, W, C = x.shape
        y = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
        lib().call("egm_maxpool2_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(y), C, N, H, W, C, stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        x, ldx = _nhwc(x)
        gy, ldg = _nhwc(gy)
        N, H, W, C = x.shape
        gx = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
        lib().call("egm_maxpool2_bwd", dtype_code(x.dtype), ptr(x), ldx, ptr(gy), ldg, ptr(gx), C, N, H, W, C, stream())
        return gx


def maxpool2(x):
    return _MaxPool2.apply(x)


class _ForkMaxPool2(Function):
    """x -> (alias of x for the skip connection, maxpool2(x)): one autograd node, so that backward adds the skip gradient while it
    scatters the pooled one (egm_maxpool2_bwd_add) instead of a scatter pass followed by an axpby pass."""

    @staticmethod
    def forward(ctx, x):
        xk, ldx = _nhwc(x)
        N, H, W, C = xk.shape
        y = torch.empty((N, H // 2, W // 2, C), dtype=xk.dtype, device=xk.device)
        lib().call("egm_maxpool2_fwd", dtype_code(xk.dtype), ptr(xk), ldx, ptr(y), C, N, H, W, C, stream())
        ctx.save_for_backward(xk)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, gskip, gy):
        (x,) = ctx.saved_tensors
        x, ldx = _nhwc(x)
        N, H, W, C = x.shape
        if gy is None:
            return gskip
        gy, ldg = _nhwc(gy)
        gx = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
        dt = dtype_code(x.dtype)
        if gskip is None:
            lib().call("egm_maxpool2_bwd", dt, ptr(x), ldx, ptr(gy), ldg, ptr(gx), C, N, H, W, C, stream())
        elif (H | W) & 1:                                       # odd sizes: the zero-tail pass, then the sum
            lib().call("egm_maxpool2_bwd", dt, ptr(x), ldx, ptr(gy), ldg, ptr(gx), C, N, H, W, C, stream())
            gx = _axpby(gx, 1.0, gskip, 1.0)
        else:
            gs, lds = _nhwc(gskip)
            lib().call("egm_maxpool2_bwd_add", dt, ptr(x), ldx, ptr(gy), ldg, ptr(gs), lds, ptr(gx), C, N, H, W, C, stream())
        return gx


def fork_maxpool2(x):
    """(x for the skip connection, maxpool2(x)) with the two gradients of x summed inside the pooling backward."""
    return _ForkMaxPool2.apply(x)


fuse_bn_up = _Switch("EGM_FUSE_BN_UP", "1",
                     """Get / set whether the bilinear upsample of an Up block applies the BatchNorm+ReLU of the Up block in front itself
                     (bf16; egm_bn_act_upcat_fwd), so that block's low-resolution output is never written (tests compare both ways).""")


def _upcat_forward(ctx, skip, low, catbuf, low_bn=None):
    """low_bn = (coef, act): `low` is a Lazy's stand-in and the kernel applies its BatchNorm + activation on the way"""
    skip, lds = _nhwc(skip)
    low, ldl = _nhwc(low)
    N, Hs, Ws, Cs = skip.shape
    _, Hl, Wl, Cl = low.shape
    inplace = False
    if catbuf is not None:
        # the skip tensor was produced straight into the first Cs channels of the concat destination: only the upsampled half is
        # written (a tensor write costs about twice a read on this part, and the skip copy was two thirds of this kernel's bytes)
        cb = catbuf[0]
        inplace = (cb.is_contiguous() and tuple(cb.shape) == (N, Hs, Ws, Cs + Cl) and cb.dtype == skip.dtype
                   and cb.data_ptr() == skip.data_ptr() and lds == Cs + Cl)
    out = cb if inplace else torch.empty((N, Hs, Ws, Cs + Cl), dtype=skip.dtype, device=skip.device)
    src = None if inplace else ptr(skip)
    if low_bn is None:
        lib().call("egm_upcat_fwd", dtype_code(skip.dtype), src, lds, ptr(low), ldl, ptr(out), Cs + Cl, N, Hs, Ws, Cs, Hl, Wl, Cl, stream())
    else:
        coef, act = low_bn
        lib().call("egm_bn_act_upcat_fwd", dtype_code(skip.dtype), src, lds, ptr(low), ldl, ptr(coef[0]), ptr(coef[1]), act, ptr(out), Cs + Cl,
                   N, Hs, Ws, Cs, Hl, Wl, Cl, stream())
    ctx.shape = (N, Hs, Ws, Cs, Hl, Wl, Cl)
    return out


def _upcat_backward(ctx, g):
    """-> (gskip, glow); inputs 0 and 1 of the node are skip and low (or low's stand-in)"""
    N, Hs, Ws, Cs, Hl, Wl, Cl = ctx.shape
    pend = _take_dz(g)
    gskip = glow = None
    if pend is not None:                           # the conv behind the concat wrote the two halves of its gradient as dense tensors
        _, ga, gb = pend[1]
        if ctx.needs_input_grad[0]:
            gskip = ga
        if ctx.needs_input_grad[1]:
            glow = torch.empty((N, Hl, Wl, Cl), dtype=gb.dtype, device=gb.device)
            lib().call("egm_upcat_bwd_low", dtype_code(gb.dtype), ptr(gb), Cl, ptr(glow), Cl, N, Hs, Ws, 0, Hl, Wl, Cl, stream())
        return gskip, glow
    g, ldo = _nhwc(g)
    if ctx.needs_input_grad[0]:
        gskip = g[..., :Cs]                        # a view: consumers take (ptr, ld)
    if ctx.needs_input_grad[1]:
        glow = torch.empty((N, Hl, Wl, Cl), dtype=g.dtype, device=g.device)
        lib().call("egm_upcat_bwd_low", dtype_code(g.dtype), ptr(g), ldo, ptr(glow), Cl, N, Hs, Ws, Cs, Hl, Wl, Cl, stream())
    return gskip, glow


class _UpCat(Function):
    """cat([skip, pad(bilinear_x2(low))], channel)"""

    @staticmethod
    def forward(ctx, skip, low, catbuf=None):
        return _upcat_forward(ctx, skip, low, catbuf)

    @staticmethod
    def backward(ctx, g):
        return _upcat_backward(ctx, g) + (None,)


class _UpCatBn(Function):
    """_UpCat of low = act(scale*y + shift) given as a Lazy's (y, coef, act): the upsample applies the BatchNorm itself
    (egm_bn_act_upcat_fwd) and the low-resolution tensor is never written.  backward is _UpCat's: the gradient of the stand-in y is
    dL/dlow (see Lazy)."""

    @staticmethod
    def forward(ctx, skip, y, coef, act, catbuf=None):
        return _upcat_forward(ctx, skip, y, catbuf, (coef, act))

    @staticmethod
    def backward(ctx, g):
        return _upcat_backward(ctx, g) + (None, None, None)


def _bn_up_ok(dtype):
    """the fused upsample takes this activation type (switch on, bf16): what ops.upcat itself decides on"""
    return fuse_bn_up.on and dtype == torch.bfloat16


def bn_up_fusable(dtype):
    """True when an Up block may hand its result to the next Up's ops.upcat as a Lazy (_bn_up_ok and BatchNorm not folded)."""
    return _bn_up_ok(dtype) and _fold_packs() is None


def upcat(skip, low, catbuf=None):
    """catbuf: the concat destination whose first channels ARE `skip` (see cat_slots), or None for a fresh tensor + copy.
    low: NHWC tensor, or a Lazy this is the only consumer of."""
    if isinstance(low, Lazy) and not (_bn_up_ok(low.dtype) and skip.dtype == low.dtype):
        low = low.materialize()
    if isinstance(low, Lazy):
        out = _UpCatBn.apply(skip, low.y, low.coef, low.act, None if catbuf is None else [catbuf])
    else:
        out = _UpCat.apply(skip, low, None if catbuf is None else [catbuf])
    # a hint for the conv that consumes the concatenation (its only consumer in Up.forward, src/EGM-UNet.py:947-949): the gradient may come
    # back as two dense tensors, split at this channel (ops._conv_dgrad).  Lost -- harmlessly -- if the tensor passes through anything else.
    out._egm_split = skip.shape[3]
    return out


class _Fork2(Function):
    """A tensor consumed twice: the two gradients are summed by the HIP axpby kernel (not by autograd's add)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None:
            return gb
        if gb is None:
            return ga
        ga, lda = _nhwc(ga)
        gb, ldb = _nhwc(gb)
        out = torch.empty(ga.shape, dtype=ga.dtype, device=ga.device)
        lib().call("egm_axpby", dtype_code(ga.dtype), ptr(ga), lda, 1.0, ptr(gb), ldb, 1.0, ptr(out), out.shape[3], _npix(ga),
                   ga.shape[3], stream())
        return out


def fork2(x):
    return _Fork2.apply(x)


# ----------------------------------------------------------------------------------------------------------
# fan-out / channel split / concat (gradient plumbing done by the HIP axpby kernel, never by autograd's add)
# ----------------------------------------------------------------------------------------------------------
def _axpby(a, alpha, b, beta, out=None):
    a, lda = _nhwc(a)
    ldb = 0
    if b is not None:
        b, ldb = _nhwc(b)
    if out is None:
        out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    o, ldo = _nhwc(out)
    assert o.data_ptr() == out.data_ptr(), "axpby: output view must be kernel-addressable"
    lib().call("egm_axpby", dtype_code(a.dtype), ptr(a), lda, float(alpha), ptr(b), ldb, float(beta), ptr(o), ldo, _npix(a),
               a.shape[3], stream())
    return out


class _Fork(Function):
    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        acc = gs[0]
        rest = gs[1:]
        while rest:
            if len(rest) >= 2:                          # 3-4 gradients summed in one pass
                take, rest = rest[:3], rest[3:]
                ts = [_nhwc(t) for t in [acc] + take]
                out = torch.empty(ts[0][0].shape, dtype=ts[0][0].dtype, device=ts[0][0].device)
                d = ts[3] if len(ts) > 3 else (None, 0)
                lib().call("egm_sum4", dtype_code(out.dtype), ptr(ts[0][0]), ts[0][1], ptr(ts[1][0]), ts[1][1], ptr(ts[2][0]), ts[2][1],
                           ptr(d[0]), d[1], ptr(out), out.shape[3], _npix(out), out.shape[3], stream())
                acc = out
            else:
                acc = _axpby(acc, 1.0, rest[0], 1.0)
                rest = rest[1:]
        return acc, None


def fork(x, n):
    """n autograd aliases of x whose gradients are summed in one pass; a Lazy forks into n Lazies over aliases of its stand-in."""
    if isinstance(x, Lazy):
        return tuple(Lazy(y, x.coef, x.act) for y in _Fork.apply(x.y, n))
    return _Fork.apply(x, n)


class _SplitC(Function):
    """x[..., :c0], x[..., c0:] as views (c0 multiple of 8); backward re-assembles one dense gradient."""

    @staticmethod
    def forward(ctx, x, c0):
        ctx.c0 = c0
        return x[..., :c0], x[..., c0:]

    @staticmethod
    def backward(ctx, ga, gb):
        c0 = ctx.c0
        ref = ga if ga is not None else gb
        N, H, W = ref.shape[:3]
        Ca = c0
        Cb = (gb.shape[3] if gb is not None else 0)
        if ga is None or gb is None:
            raise RuntimeError("split_channels: both halves must receive a gradient")
        out = torch.empty((N, H, W, Ca + Cb), dtype=ref.dtype, device=ref.device)
        _axpby(ga, 1.0, None, 0.0, out[..., :Ca])
        _axpby(gb, 1.0, None, 0.0, out[..., Ca:])
        return out, None


def split_channels(x, c0):
    return _SplitC.apply(x, c0)


class _CatC(Function):
    @staticmethod
    def forward(ctx, buf_slot, *xs):
        N, H, W = xs[0].shape[:3]
        cs = [x.shape[3] for x in xs]
        buf = buf_slot[0] if buf_slot is not None else None
        if buf is not None and not (buf.is_contiguous() and tuple(buf.shape) == (N, H, W, sum(cs)) and buf.dtype == xs[0].dtype):
            raise RuntimeError("cat_channels: destination buffer does not match the inputs")
        out = buf if buf is not None else torch.empty((N, H, W, sum(cs)), dtype=xs[0].dtype, device=xs[0].device)
        off = 0
        for x, c in zip(xs, cs):
            dst = out[..., off:off + c]
            # an input that was produced straight into its slot (bn_act / gate3 with out=) needs no copy
            if not (x.data_ptr() == dst.data_ptr() and x.stride() == dst.stride()):
                _axpby(x, 1.0, None, 0.0, dst)
            off += c
        ctx.cs = cs
        return out

    @staticmethod
    def backward(ctx, g):
        outs, off = [None], 0
        for c in ctx.cs:
            outs.append(g[..., off:off + c])
            off += c
        return tuple(outs)


def cat_channels(xs, buf=None):
    """buf: optional destination from cat_slots(); inputs already living in their slot are not copied."""
    return _CatC.apply(None if buf is None else [buf], *xs)


# ----------------------------------------------------------------------------------------------------------
# elementwise pieces of the EGM blocks
# ----------------------------------------------------------------------------------------------------------
def _hp(x):
    x, ldx = _nhwc(x)
    N, H, W, C = x.shape
    out = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
    lib().call("egm_highpass3", dtype_code(x.dtype), ptr(x), ldx, ptr(out), C, N, H, W, C, stream())
    return out


class _Highpass3(Function):
    @staticmethod
    def forward(ctx, x):
        return _hp(x)

    @staticmethod
    def backward(ctx, g):
        return _hp(g)           # x - avg3(x) with zero padding is self-adjoint


def highpass3(x):
    return _Highpass3.apply(x)


class _ForkHighpass(Function):
    """x -> (highpass3(x), n aliases of x) as one node: backward computes highpass3(g_hp) + sum of the other gradients in ONE pass
    (egm_sum4_hp) instead of a stencil pass that writes its result and a fan-in pass that reads it back."""

    @staticmethod
    def forward(ctx, x, n):
        return (_hp(x),) + tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, ghp, *gs):
        return _fork_highpass_backward(ctx, ghp, gs), None


def _fork_highpass_backward(ctx, ghp, gs):
    """-> highpass3(ghp) + sum(gs): the gradient of the forked tensor"""
    gs = [g for g in gs if g is not None]
    if ghp is None:
        return _Fork.backward(ctx, *gs)[0] if gs else None
    if not gs:
        return _hp(ghp)
    while len(gs) > 3:                                    # more than three other consumers: pre-sum the tail
        gs = gs[:2] + [_Fork.backward(ctx, *gs[2:])[0]]
    a, lda = _nhwc(ghp)
    N, H, W, C = a.shape
    ts = [_nhwc(t) for t in gs] + [(None, 0)] * (3 - len(gs))
    out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    lib().call("egm_sum4_hp", dtype_code(a.dtype), ptr(a), lda, ptr(ts[0][0]), ts[0][1], ptr(ts[1][0]), ts[1][1], ptr(ts[2][0]), ts[2][1],
               ptr(out), C, N, H, W, C, stream())
    return out


fuse_bn_hp = _Switch("EGM_FUSE_BN_HP", "1",
                     """Get / set whether the EdgeEnhancedGRFB's entry high-pass applies the BatchNorm+ReLU of the DoubleConv1 conv in front
                     itself (bf16; egm_bn_act_hp_fwd): the tensor is written and its edge map formed in one pass (tests compare both ways).""")


class _ForkHighpassBn(Function):
    """_ForkHighpass of z = act(scale*y + shift) given as a Lazy's (y, coef, act): one pass writes z (into the destination view when
    given) and highpass3(z) (egm_bn_act_hp_fwd).  backward is _ForkHighpass's: the gradient of the stand-in y is dL/dz (see Lazy)."""

    @staticmethod
    def forward(ctx, y, coef, act, n, out_slot):
        y, ldy = _nhwc(y)
        N, H, W, C = y.shape
        z, ldz = _slot_or_new(out_slot, (N, H, W, C), y.dtype, y.device)
        edge = torch.empty((N, H, W, C), dtype=y.dtype, device=y.device)
        lib().call("egm_bn_act_hp_fwd", dtype_code(y.dtype), ptr(y), ldy, ptr(coef[0]), ptr(coef[1]), act, ptr(z), ldz, ptr(edge), C,
                   N, H, W, C, stream())
        return (edge,) + tuple(z.view_as(z) for _ in range(n))

    @staticmethod
    def backward(ctx, ghp, *gs):
        return _fork_highpass_backward(ctx, ghp, gs), None, None, None, None


def _bn_hp_ok(dtype):
    """the fused high-pass takes this activation type (switch on, bf16): what ops.fork_highpass3 itself decides on"""
    return fuse_bn_hp.on and dtype == torch.bfloat16


def bn_hp_fusable(dtype):
    """True when DoubleConv1 may hand its result to the GRFB's ops.fork_highpass3 as a Lazy (_bn_hp_ok and BatchNorm not folded)."""
    return _bn_hp_ok(dtype) and _fold_packs() is None


def fork_highpass3(x, n, out=None):
    """(highpass3(x), alias_1, ..., alias_n): the edge extractor of EdgeAwareFeatureEnhancer together with x's other consumers.
    x: NHWC tensor, or a Lazy this is the only consumer of; out: optional destination view (a concat slot) the tensor of a Lazy is
    written into -- the aliases then live there."""
    if isinstance(x, Lazy):
        if _bn_hp_ok(x.dtype):
            return _ForkHighpassBn.apply(x.y, x.coef, x.act, n, None if out is None else [out])
        x = x.materialize(out)
    elif out is not None:
        x = materialize(x, out)
    return _ForkHighpass.apply(x, n)


class _GateMul(Function):
    @staticmethod
    def forward(ctx, x, w):
        x, ldx = _nhwc(x)
        w, ldw = _nhwc(w)
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        lib().call("egm_gate_mul_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(w), ldw, ptr(out), x.shape[3], _npix(x), x.shape[3], stream())
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        x, ldx = _nhwc(x); w, ldw = _nhwc(w); g, ldg = _nhwc(g)
        C = x.shape[3]
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        dw = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        lib().call("egm_gate_mul_bwd", dtype_code(x.dtype), ptr(g), ldg, ptr(x), ldx, ptr(w), ldw, ptr(dx), C, ptr(dw), C, _npix(x), C, stream())
        return dx, dw


def gate_mul(x, w):
    return _GateMul.apply(x, w)


class _ScaleAddRelu(Function):
    @staticmethod
    def forward(ctx, a, alpha, b):
        a, lda = _nhwc(a); b, ldb = _nhwc(b)
        C = a.shape[3]
        out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
        lib().call("egm_scale_add_relu_fwd", dtype_code(a.dtype), ptr(a), lda, float(alpha), ptr(b), ldb, ptr(out), C, _npix(a), C, stream())
        ctx.save_for_backward(out)
        ctx.alpha = float(alpha)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        out, ldo = _nhwc(out); g, ldg = _nhwc(g)
        C = out.shape[3]
        da = torch.empty(out.shape, dtype=out.dtype, device=out.device)
        db = torch.empty(out.shape, dtype=out.dtype, device=out.device)
        lib().call("egm_scale_add_relu_bwd", dtype_code(out.dtype), ptr(g), ldg, ptr(out), ldo, ctx.alpha, ptr(da), C, ptr(db), C, _npix(out), C,
                   stream())
        return da, None, db


def scale_add_relu(a, alpha, b):
    return _ScaleAddRelu.apply(a, alpha, b)


class _Gate3(Function):
    @staticmethod
    def forward(ctx, x, t, out_slot=None):
        x, ldx = _nhwc(x); t, ldt = _nhwc(t)
        C = x.shape[3]
        out, ldo = _slot_or_new(out_slot, tuple(x.shape), x.dtype, x.device)
        lib().call("egm_gate3_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(t), ldt, ptr(out), ldo, _npix(x), C, stream())
        ctx.save_for_backward(x, t)
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        x, ldx = _nhwc(x); t, ldt = _nhwc(t); g, ldg = _nhwc(g)
        C = x.shape[3]
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        dt = torch.empty(t.shape[:3] + (8,), dtype=x.dtype, device=x.device)
        lib().call("egm_gate3_bwd", dtype_code(x.dtype), ptr(g), ldg, ptr(x), ldx, ptr(t), ldt, ptr(dx), C, ptr(dt), 8, _npix(x), C, stream())
        return dx, dt, None


def gate3(x, t, out=None):
    return _Gate3.apply(x, t, None if out is None else [out])


class _Gate3Pool(Function):
    """gate3 followed by the skip-connection fork + max pool as ONE node: -> (out, maxpool2(out)); backward takes both gradients and
    never materialises their sum (egm_gate3_pool_bwd; EdgeEnhancedGRFB's last op, src/EGM-UNet.py:1319-1321, behind :908)."""

    @staticmethod
    def forward(ctx, x, t, out_slot=None):
        x, ldx = _nhwc(x); t, ldt = _nhwc(t)
        N, H, W, C = x.shape
        out, ldo = _slot_or_new(out_slot, tuple(x.shape), x.dtype, x.device)
        pooled = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
        lib().call("egm_gate3_fwd_pool", dtype_code(x.dtype), ptr(x), ldx, ptr(t), ldt, ptr(out), ldo, ptr(pooled), C, N, H, W, C, stream())
        ctx.save_for_backward(x, t, out)
        ctx.set_materialize_grads(False)
        return out, pooled

    @staticmethod
    def backward(ctx, gskip, gpool):
        if gskip is None and gpool is None:
            return None, None, None
        x, t, out = ctx.saved_tensors
        x, ldx = _nhwc(x); t, ldt = _nhwc(t)
        N, H, W, C = x.shape
        L, dt_, st = lib(), dtype_code(x.dtype), stream()
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        dt = torch.empty(t.shape[:3] + (8,), dtype=x.dtype, device=x.device)
        if gskip is not None and gpool is not None:
            gs, lds = _nhwc(gskip); gp, ldp = _nhwc(gpool)
            L.call("egm_gate3_pool_bwd", dt_, ptr(gs), lds, ptr(gp), ldp, ptr(x), ldx, ptr(t), ldt, ptr(dx), C, ptr(dt), 8, N, H, W, C, st)
            return dx, dt, None
        if gskip is None:                                       # only the pooled branch was used: the separate scatter
            ok, ldo = _nhwc(out); gp, ldp = _nhwc(gpool)
            gskip = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            L.call("egm_maxpool2_bwd", dt_, ptr(ok), ldo, ptr(gp), ldp, ptr(gskip), C, N, H, W, C, st)
        g, ldg = _nhwc(gskip)
        L.call("egm_gate3_bwd", dt_, ptr(g), ldg, ptr(x), ldx, ptr(t), ldt, ptr(dx), C, ptr(dt), 8, _npix(x), C, st)
        return dx, dt, None


def gate3_pool(x, t, out=None):
    """-> (gate3(x, t) [into `out`], maxpool2 of it); see _Gate3Pool.  Callers check pool_fusable(x) first."""
    return _Gate3Pool.apply(x, t, None if out is None else [out])


class _BcastGate(Function):
    @staticmethod
    def forward(ctx, a, gl):
        a, lda = _nhwc(a); gl, ldg = _nhwc(gl)
        C = a.shape[3]
        out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
        lib().call("egm_bcast_gate_fwd", dtype_code(a.dtype), ptr(a), lda, ptr(gl), ldg, ptr(out), C, _npix(a), C, stream())
        ctx.save_for_backward(a, gl)
        return out

    @staticmethod
    def backward(ctx, g):
        a, gl = ctx.saved_tensors
        a, lda = _nhwc(a); gl, ldgl = _nhwc(gl); g, ldg = _nhwc(g)
        C = a.shape[3]
        da = torch.empty(a.shape, dtype=a.dtype, device=a.device)
        dgl = torch.empty(gl.shape[:3] + (8,), dtype=a.dtype, device=a.device)
        lib().call("egm_bcast_gate_bwd", dtype_code(a.dtype), ptr(g), ldg, ptr(a), lda, ptr(gl), ldgl, ptr(da), C, ptr(dgl), 8, _npix(a), C,
                   stream())
        return da, dgl


def bcast_gate(a, gl):
    return _BcastGate.apply(a, gl)


class _Gelu(Function):
    @staticmethod
    def forward(ctx, x):
        x, ldx = _nhwc(x)
        C = x.shape[3]
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        lib().call("egm_gelu_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(out), C, _npix(x), C, stream())
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        x, ldx = _nhwc(x); g, ldg = _nhwc(g)
        C = x.shape[3]
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        lib().call("egm_gelu_bwd", dtype_code(x.dtype), ptr(g), ldg, ptr(x), ldx, ptr(dx), C, _npix(x), C, stream())
        return dx


def gelu(x):
    return _Gelu.apply(x)


class _Act(Function):
    """Standalone activation (the ReLU inside ChannelAttentionModule.fc) through the BN-apply kernels with unit scale."""

    @staticmethod
    def forward(ctx, x, act):
        x, ldx = _nhwc(x)
        C = x.shape[3]
        coef = torch.zeros((4, C), dtype=torch.float32, device=x.device)
        lib().call("egm_fill_f32", ptr(coef[0]), 1.0, C, stream())
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        lib().call("egm_bn_act_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(coef[0]), ptr(coef[1]), act, ptr(out), C, _npix(x), C, stream())
        ctx.save_for_backward(x, coef)
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, g):
        x, coef = ctx.saved_tensors
        x, ldx = _nhwc(x); g, ldg = _nhwc(g)
        C = x.shape[3]
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        lib().call("egm_bn_act_bwd_apply", dtype_code(x.dtype), ptr(g), ldg, ptr(x), ldx, ptr(coef[0]), ptr(coef[1]), ptr(coef[2]),
                   ptr(coef[3]), ctx.act, 0, ptr(coef[2]), ptr(dx), C, _npix(x), C, stream())
        return dx, None


def act(x, code):
    return _Act.apply(x, code)


class _ChanMeanMax(Function):
    @staticmethod
    def forward(ctx, x, c_real):
        x, ldx = _nhwc(x)
        out = torch.empty(x.shape[:3] + (8,), dtype=x.dtype, device=x.device)
        lib().call("egm_chan_meanmax_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(out), 8, _npix(x), x.shape[3], c_real, stream())
        ctx.save_for_backward(x)
        ctx.c_real = c_real
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        x, ldx = _nhwc(x); g, ldg = _nhwc(g)
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        lib().call("egm_chan_meanmax_bwd", dtype_code(x.dtype), ptr(g), ldg, ptr(x), ldx, ptr(dx), x.shape[3], _npix(x), x.shape[3], ctx.c_real,
                   stream())
        return dx, None


def chan_meanmax(x, c_real):
    return _ChanMeanMax.apply(x, c_real)


class _GlobalAvgMax(Function):
    """-> [2N, 1, 1, C]: rows 0..N-1 adaptive_avg_pool2d(x, 1), rows N..2N-1 adaptive_max_pool2d(x, 1)."""

    @staticmethod
    def forward(ctx, x):
        x, ldx = _nhwc(x)
        N, H, W, C = x.shape
        L = lib()
        out = torch.empty((2 * N, 1, 1, C), dtype=x.dtype, device=x.device)
        argidx = torch.empty((N, C), dtype=torch.int32, device=x.device)
        ws = torch.empty(L.query("egm_global_pool_workspace", N, H * W, C) // 4 + 4, dtype=torch.float32, device=x.device)
        L.call("egm_global_avgmax_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(out), ptr(argidx), ptr(ws), N, H * W, C, stream())
        ctx.save_for_backward(argidx)
        ctx.shape = (N, H, W, C)
        return out

    @staticmethod
    def backward(ctx, g):
        (argidx,) = ctx.saved_tensors
        N, H, W, C = ctx.shape
        g = g.contiguous()
        dx = torch.empty((N, H, W, C), dtype=g.dtype, device=g.device)
        lib().call("egm_global_avgmax_bwd", dtype_code(g.dtype), ptr(g), ptr(argidx), ptr(dx), C, N, H * W, C, stream())
        return dx


def global_avgmax(x):
    return _GlobalAvgMax.apply(x)


class _CaMlp(Function):
    """ChannelAttentionModule.fc on the pooled rows [R,1,1,C]: W2 . relu(W0 . p) as one launch forward, one backward (egm_ca_mlp_*)."""

    @staticmethod
    def forward(ctx, pooled, w0, w2):
        R, Cp = pooled.shape[0], pooled.shape[3]
        Cr, C = w0.shape[0], w0.shape[1]
        pooled = pooled.contiguous()
        w0c, w2c = w0.detach().contiguous(), w2.detach().contiguous()
        h = torch.empty((R, Cr), dtype=torch.float32, device=pooled.device)
        out = (torch.empty if Cp == C else torch.zeros)((R, 1, 1, Cp), dtype=pooled.dtype, device=pooled.device)
        lib().call("egm_ca_mlp_fwd", dtype_code(pooled.dtype), ptr(pooled), Cp, ptr(w0c), ptr(w2c), ptr(h), ptr(out), Cp, R, C, Cr, stream())
        ctx.save_for_backward(pooled, h, w0c, w2c)
        return out

    @staticmethod
    def backward(ctx, g):
        pooled, h, w0, w2 = ctx.saved_tensors
        R, Cp = pooled.shape[0], pooled.shape[3]
        Cr, C = w0.shape[0], w0.shape[1]
        g = g.contiguous()
        dw0, dw2 = torch.empty_like(w0), torch.empty_like(w2)
        dp = (torch.empty if Cp == C else torch.zeros)(pooled.shape, dtype=pooled.dtype, device=pooled.device)
        lib().call("egm_ca_mlp_bwd", dtype_code(pooled.dtype), ptr(g), Cp, ptr(pooled), Cp, ptr(h), ptr(w0), ptr(w2), ptr(dw0), ptr(dw2),
                   ptr(dp), Cp, R, C, Cr, stream())
        return dp, dw0, dw2


def ca_mlp(pooled, w0, w2):
    return _CaMlp.apply(pooled, w0, w2)


class _FusionCombine(Function):
    """f + s*sigmoid(sa[...,0])*sigmoid(ca_avg + ca_max); ca: [2N,1,1,C]."""

    @staticmethod
    def forward(ctx, f, s, sa, ca):
        f, ldf = _nhwc(f); s, lds = _nhwc(s); sa, ldsa = _nhwc(sa)
        ca = ca.contiguous()
        N, H, W, C = f.shape
        out = torch.empty(f.shape, dtype=f.dtype, device=f.device)
        lib().call("egm_fusion_combine_fwd", dtype_code(f.dtype), ptr(f), ldf, ptr(s), lds, ptr(sa), ldsa, ptr(ca), ptr(out), C, N, H * W, C,
                   stream())
        ctx.save_for_backward(s, sa, ca)
        return out

    @staticmethod
    def backward(ctx, g):
        s, sa, ca = ctx.saved_tensors
        s, lds = _nhwc(s); sa, ldsa = _nhwc(sa); g, ldg = _nhwc(g)
        N, H, W, C = s.shape
        L, dev = lib(), s.device
        ds = torch.empty(s.shape, dtype=s.dtype, device=dev)
        dsa = torch.empty((N, H, W, 8), dtype=s.dtype, device=dev)
        nb = L.query("egm_fusion_combine_blocks", H * W, C)
        part = _f32((N, nb, 2, C), dev)
        L.call("egm_fusion_combine_bwd", dtype_code(s.dtype), ptr(g), ldg, ptr(s), lds, ptr(sa), ldsa, ptr(ca), ptr(ds), C, ptr(dsa), 8,
               ptr(part), N, H * W, C, stream())
        red = _f32((N, 2, C), dev)
        L.call("egm_reduce_tiles_batched", ptr(part), N, nb, C, ptr(red), stream())
        # d(ca_avg) = d(ca_max) = dca  ->  [2N,1,1,C] in the activation dtype
        dca = torch.empty((2 * N, 1, 1, C), dtype=s.dtype, device=dev)
        _f32_rows_to_act(red, dca, N, C)
        return g, ds, dsa, dca


def _f32_rows_to_act(red, dca, N, C):
    """red fp32 [N][2][C] (row 0 = dca) -> dca[n] and dca[N+n] in the activation dtype (one launch)."""
    lib().call("egm_rows_dup", dtype_code(dca.dtype), ptr(red), ptr(dca), C, N, C, stream())


def fusion_combine(f, s, sa, ca):
    return _FusionCombine.apply(f, s, sa, ca)


def _register_pack(weight, dtype, wf, wd):
    """Operand packs produced together with a derived weight (fold2 / merge357): what _packed_weights would build for it."""
    key = (weight.data_ptr(), weight._version, _weight_generation[0], dtype, 1, tuple(weight.shape))
    _pack_cache[id(weight)] = (key, wf, wd, weakref.ref(weight))


class _Fold2(Function):
    @staticmethod
    def forward(ctx, w, pack_dtype, pre=None):             # [rows, 2K, 1, 1] -> [rows, K, 1, 1]
        rows, K2 = w.shape[0], w.shape[1]
        K = K2 // 2
        ctx.real = w
        if pre is not None:                                # built by the model-wide prepack (prepack_model): no launch
            _Fold2.packs = (pre[2], pre[3])
            return pre[0].detach()                         # (an alias: every forward returns a tensor object of its own)
        out = torch.empty((rows, K, 1, 1), dtype=torch.float32, device=w.device)
        if pack_dtype is None:
            lib().call("egm_fold2_fwd", ptr(w.detach().contiguous()), ptr(out), rows, K, stream())
            _Fold2.packs = None
        else:                                              # the conv operand packs of the folded weight from the same launch
            wf = torch.empty((1, pad8(rows), pad8(K)), dtype=pack_dtype, device=w.device)
            wd = torch.empty((1, pad8(K), pad8(rows)), dtype=pack_dtype, device=w.device)
            lib().call("egm_fold2_pack", dtype_code(pack_dtype), ptr(w.detach().contiguous()), ptr(out), ptr(wf), ptr(wd), rows, K, stream())
            _Fold2.packs = (wf, wd)
        return out

    @staticmethod
    def backward(ctx, g):
        rows, K = g.shape[0], g.shape[1]
        pend = _take_derived(g)
        if pend is not None:                               # a stand-in: the conv's deferred reduction writes both halves itself
            dw = _unfilled((rows, 2 * K, 1, 1), g.device)
            _attach_derived(pend, (ctx.real,), (dw,))
            return dw, None, None
        _no_open_standin((ctx.real,))
        dw = torch.empty((rows, 2 * K, 1, 1), dtype=torch.float32, device=g.device)
        lib().call("egm_fold2_bwd", ptr(g.contiguous()), ptr(dw), rows, K, stream())
        return dw, None, None


def fold2(w, pack_dtype=None):
    """w[:, :K] + w[:, K:]; pack_dtype: also build the conv operand packs of the result for that activation dtype (one launch, none
    when the model-wide prepack has built them already)."""
    out = _Fold2.apply(w, pack_dtype, _prepacked((w,), pack_dtype) if pack_dtype is not None else None)
    if pack_dtype is not None and _Fold2.packs is not None:
        _register_pack(out, pack_dtype, *_Fold2.packs)
        _Fold2.packs = None
    _register_derived(out, "fold2", (w,))
    return out


class _SpreadCols(Function):
    """[rows, sum(real), 1, 1] -> [rows, sum(pad8(real)), 1, 1]: the input-channel columns of a 1x1 weight moved to where the channels sit
    after each source tensor was padded to a multiple of 8 on its own (zeros in the gaps).  Backward gathers the columns back."""

    @staticmethod
    def forward(ctx, w, real):
        rows, st = w.shape[0], stream()
        tot_r, tot_p = sum(real), sum(pad8(c) for c in real)
        out = torch.zeros((rows, tot_p, 1, 1), dtype=torch.float32, device=w.device)
        wc = w.detach().contiguous()
        o_r = o_p = 0
        for c in real:
            lib().call("egm_copy_cols_f32", ptr(wc), tot_r, o_r, ptr(out), tot_p, o_p, rows, c, st)
            o_r, o_p = o_r + c, o_p + pad8(c)
        ctx.real = tuple(real)
        return out

    @staticmethod
    def backward(ctx, g):
        real = ctx.real
        rows, st = g.shape[0], stream()
        tot_r, tot_p = sum(real), sum(pad8(c) for c in real)
        gc = g.contiguous()
        dw = torch.empty((rows, tot_r, 1, 1), dtype=torch.float32, device=g.device)
        o_r = o_p = 0
        for c in real:
            lib().call("egm_copy_cols_f32", ptr(gc), tot_p, o_p, ptr(dw), tot_r, o_r, rows, c, st)
            o_r, o_p = o_r + c, o_p + pad8(c)
        return dw, None


def spread_cols(w, real):
    return _SpreadCols.apply(w, real)


class _Merge357(Function):
    @staticmethod
    def forward(ctx, w3, w5, w7, b3, b5, b7, pack_dtype, pre=None):
        Co, Ci = w7.shape[0], w7.shape[1]
        ctx.shape = (Co, Ci)
        ctx.real = (w3, w5, w7, b3, b5, b7)
        if pre is not None:                                # built by the model-wide prepack (prepack_model): no launch
            _Merge357.packs = (pre[2], pre[3])
            return pre[0].detach(), pre[1].detach()
        w = torch.empty((Co, Ci, 7, 7), dtype=torch.float32, device=w7.device)
        b = torch.empty((Co,), dtype=torch.float32, device=w7.device)
        args = (ptr(w3.detach().contiguous()), ptr(w5.detach().contiguous()), ptr(w7.detach().contiguous()), ptr(b3.detach()),
                ptr(b5.detach()), ptr(b7.detach()), ptr(w), ptr(b))
        if pack_dtype is None:
            lib().call("egm_merge357_fwd", *args, Co, Ci, stream())
            _Merge357.packs = None
        else:
            wf = torch.empty((49, pad8(Co), pad8(Ci)), dtype=pack_dtype, device=w7.device)
            wd = torch.empty((49, pad8(Ci), pad8(Co)), dtype=pack_dtype, device=w7.device)
            lib().call("egm_merge357_pack", dtype_code(pack_dtype), *args, ptr(wf), ptr(wd), Co, Ci, stream())
            _Merge357.packs = (wf, wd)
        return w, b

    @staticmethod
    def backward(ctx, gw, gb):
        Co, Ci = ctx.shape
        dev = gw.device
        w3, w5, w7, b3, b5, b7 = ctx.real
        pw = _take_derived(gw)
        if pw is not None:
            # stand-ins: the conv's deferred reduction scatters into the three kernels itself, the deferred bias sum writes all three
            # biases (the conv defers both or neither, _wgrad_deferral)
            d3, d5, d7 = _unfilled((Co, Ci, 3, 3), dev), _unfilled((Co, Ci, 5, 5), dev), _unfilled((Co, Ci, 7, 7), dev)
            _attach_derived(pw, (w7, w5, w3), (d7, d5, d3))           # the order of the reduction's destinations dw, dw2, dw3
            if gb is None or not any(ctx.needs_input_grad[3:6]):
                return d3, d5, d7, None, None, None, None, None
            pb = _take_derived(gb)
            if pb is None:
                raise RuntimeError("egm_unet_amd: merge357 received a deferred weight gradient with a bias gradient that is not")
            gb3 = _unfilled((3, Co), dev)
            rows = (gb3[0], gb3[1], gb3[2])
            _attach_derived(pb, (b3, b5, b7), rows)
            return d3, d5, d7, rows[0], rows[1], rows[2], None, None
        _no_open_standin(ctx.real)
        d3 = torch.empty((Co, Ci, 3, 3), dtype=torch.float32, device=dev)
        d5 = torch.empty((Co, Ci, 5, 5), dtype=torch.float32, device=dev)
        d7 = torch.empty((Co, Ci, 7, 7), dtype=torch.float32, device=dev)
        # the bias gradient goes to three parameters: handed out as three tensors (the same tensor three times makes autograd clone it
        # twice: two copy launches per FusionConv)
        gb3 = None
        if gb is not None:
            gb3 = torch.empty((3, Co), dtype=torch.float32, device=dev)
        lib().call("egm_merge357_bwd", ptr(gw.contiguous()), ptr(d3), ptr(d5), ptr(d7), ptr(gb), ptr(gb3), Co, Ci, stream())
        if gb3 is None:
            return d3, d5, d7, None, None, None, None, None
        return d3, d5, d7, gb3[0], gb3[1], gb3[2], None, None


def merge357(w3, w5, w7, b3, b5, b7, pack_dtype=None):
    reals = (w3, w5, w7, b3, b5, b7)
    w, b = _Merge357.apply(*reals, pack_dtype, _prepacked(reals, pack_dtype) if pack_dtype is not None else None)
    if pack_dtype is not None and _Merge357.packs is not None:
        _register_pack(w, pack_dtype, *_Merge357.packs)
        _Merge357.packs = None
    _register_derived(w, "merge357", (w7, w5, w3))
    _register_derived(b, "bias3", (b3, b5, b7))
    return w, b


class _DwConv3(Function):
    """(depthwise3x3(x, w) + b) * scale   (RecursiveGatedAttention.dwconv and the learnable scale)"""

    @staticmethod
    def forward(ctx, x, w, b, scale):
        x, ldx = _nhwc(x)
        N, H, W, C = x.shape
        y = torch.empty((N, H, W, C), dtype=x.dtype, device=x.device)
        wd, bd, sd = w.detach().contiguous(), b.detach().contiguous(), scale.detach().reshape(1).contiguous()
        lib().call("egm_dwconv3_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(wd), ptr(bd), ptr(sd), ptr(y), C, N, H, W, C, stream())
        ctx.save_for_backward(x, wd, bd, sd)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, b, sc = ctx.saved_tensors
        x, ldx = _nhwc(x); g, ldg = _nhwc(g)
        N, H, W, C = x.shape
        L, dev = lib(), x.device
        dx = torch.empty(x.shape, dtype=x.dtype, device=dev)
        dw = torch.empty((C, 1, 3, 3), dtype=torch.float32, device=dev)
        db = torch.empty((C,), dtype=torch.float32, device=dev)
        ds = torch.empty((1,), dtype=torch.float32, device=dev)
        ws = torch.empty(L.query("egm_dwconv3_bwd_workspace", N, H, W, C) // 4 + 4, dtype=torch.float32, device=dev)
        L.call("egm_dwconv3_bwd", dtype_code(x.dtype), ptr(x), ldx, ptr(g), ldg, ptr(w), ptr(b), ptr(sc), ptr(dx), C, ptr(dw), ptr(db), ptr(ds),
               ptr(ws), N, H, W, C, stream())
        return dx, dw, db, ds.reshape(())


def dwconv3(x, w, b, scale):
    return _DwConv3.apply(x, w, b, scale)


# ----------------------------------------------------------------------------------------------------------
# ConvTranspose2d(k=2, s=2) of Up(bilinear=False)
# ----------------------------------------------------------------------------------------------------------
class _ConvTPack(Function):
    """[Cin][Cout][2][2] parameter -> OIHW [4*CoutP, Cin, 1, 1] matrix of the equivalent 1x1 conv (rows ordered (i, j, co))"""

    @staticmethod
    def forward(ctx, w):
        Cin, Cout = w.shape[0], w.shape[1]
        CoutP = pad8(Cout)
        w4 = torch.empty((4 * CoutP, Cin, 1, 1), dtype=torch.float32, device=w.device)
        lib().call("egm_convT2x2_pack", ptr(w.detach().contiguous()), ptr(w4), Cin, Cout, CoutP, 1, stream())
        ctx.shape = tuple(w.shape)
        return w4

    @staticmethod
    def backward(ctx, g):
        Cin, Cout = ctx.shape[0], ctx.shape[1]
        dw = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        lib().call("egm_convT2x2_pack", ptr(dw), ptr(g.contiguous()), Cin, Cout, pad8(Cout), 0, stream())
        return dw


class _Shuffle2x2(Function):
    @staticmethod
    def forward(ctx, y4, bias, C, Ho, Wo):
        y4, ld4 = _nhwc(y4)
        N, H, W, _ = y4.shape
        CP = pad8(C)
        oy, ox = (Ho - 2 * H) // 2, (Wo - 2 * W) // 2          # F.pad(x1, [dx//2, dx - dx//2, dy//2, dy - dy//2])
        out = torch.empty((N, Ho, Wo, CP), dtype=y4.dtype, device=y4.device)
        lib().call("egm_shuffle2x2_fwd", dtype_code(y4.dtype), ptr(y4), ld4, ptr(bias.detach() if bias is not None else None), C, ptr(out), CP,
                   N, H, W, CP, Ho, Wo, oy, ox, stream())
        ctx.meta = (N, H, W, CP, Ho, Wo, oy, ox, C, bias is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        N, H, W, CP, Ho, Wo, oy, ox, C, has_bias = ctx.meta
        g, ldg = _nhwc(g)
        d4 = torch.empty((N, H, W, 4 * CP), dtype=g.dtype, device=g.device)
        lib().call("egm_shuffle2x2_bwd", dtype_code(g.dtype), ptr(g), ldg, ptr(d4), 4 * CP, N, H, W, CP, Ho, Wo, oy, ox, stream())
        db = None
        if has_bias and ctx.needs_input_grad[1]:
            # frame positions outside the shuffled image get no bias: sum the gradient over the image region only = over d4
            db4 = _channel_sum(d4)[0]
            db = _fold4(db4, CP)[:C]
        return d4, db, None, None, None


def _fold4(v, CP):
    """v [4*CP] fp32 -> [CP]: sum of the four (i, j) slices, on the device with the axpby kernel (no torch arithmetic)."""
    t = v.reshape(1, 1, 4, CP)
    a = _axpby(t[:, :, 0:1], 1.0, t[:, :, 1:2], 1.0)
    b = _axpby(t[:, :, 2:3], 1.0, t[:, :, 3:4], 1.0)
    return _axpby(a, 1.0, b, 1.0).reshape(CP)


def conv_transpose2x2(x, convT, out_hw):
    """nn.ConvTranspose2d(Cin, Cout, 2, stride=2) + F.pad to out_hw (src/unet.py:36,40-47).  x NHWC -> [N, Ho, Wo, pad8(Cout)]"""
    w4 = _ConvTPack.apply(convT.weight)
    y4 = conv2d(x, w4)
    return _Shuffle2x2.apply(y4, convT.bias, convT.weight.shape[1], out_hw[0], out_hw[1])


# ----------------------------------------------------------------------------------------------------------
# HEGDC pieces (src/EGM-UNet.py:210-340)
# ----------------------------------------------------------------------------------------------------------
@torch.no_grad()
def hegdc_edge_features(x, c_real):
    """The block's no_grad branch -> [N, H, W, 8] (5 real channels: scharr_x, scharr_y, sobel_x, sobel_y, blended magnitude)."""
    x, ldx = _nhwc(x)
    N, H, W, _ = x.shape
    L = lib()
    ws = torch.empty(L.query("egm_hegdc_edge_workspace", N, H, W) // 4 + 4, dtype=torch.float32, device=x.device)
    feats = torch.empty((N, H, W, 8), dtype=x.dtype, device=x.device)
    L.call("egm_hegdc_edge_features", dtype_code(x.dtype), ptr(x), ldx, c_real, ptr(feats), ptr(ws), N, H, W, stream())
    return feats


class _ScaleSigmoid(Function):
    """w * sigmoid(den): conv1_weight * Phi with Phi = phi_base (ones) * sigmoid(den)  (src/EGM-UNet.py:262-265,325-327)"""

    @staticmethod
    def forward(ctx, w, den):
        wc = w.detach().contiguous()
        out = torch.empty_like(wc)
        lib().call("egm_scale_sigmoid_fwd", ptr(wc), ptr(den.detach()), ptr(out), wc.numel(), stream())
        ctx.save_for_backward(wc, den)
        return out

    @staticmethod
    def backward(ctx, g):
        w, den = ctx.saved_tensors
        g = g.contiguous()
        dw, dden = torch.empty_like(w), torch.empty_like(den, dtype=torch.float32)
        part = _f32(256, w.device)
        lib().call("egm_scale_sigmoid_bwd", ptr(g), ptr(w), ptr(den.detach()), ptr(dw), ptr(dden), ptr(part), w.numel(), stream())
        return dw, dden.reshape(den.shape)


def scale_sigmoid(w, den):
    return _ScaleSigmoid.apply(w, den)


class _Mul2Scalar(Function):
    """a * b * alpha (alpha: learnable scalar parameter)  (src/EGM-UNet.py:332)"""

    @staticmethod
    def forward(ctx, a, b, alpha):
        a, lda = _nhwc(a); b, ldb = _nhwc(b)
        out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
        al = alpha.detach().reshape(1).float()
        lib().call("egm_mul2_scalar_fwd", dtype_code(a.dtype), ptr(a), lda, ptr(b), ldb, ptr(al), ptr(out), a.shape[3], _npix(a), a.shape[3], stream())
        ctx.save_for_backward(a, b, al)
        ctx.ashape = alpha.shape
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, al = ctx.saved_tensors
        a, lda = _nhwc(a); b, ldb = _nhwc(b); g, ldg = _nhwc(g)
        C = a.shape[3]
        da = torch.empty(a.shape, dtype=a.dtype, device=a.device)
        db = torch.empty(b.shape, dtype=b.dtype, device=b.device) if ctx.needs_input_grad[1] else None
        dalpha, part = _f32(1, a.device), _f32(1024, a.device)
        lib().call("egm_mul2_scalar_bwd", dtype_code(a.dtype), ptr(g), ldg, ptr(a), lda, ptr(b), ldb, ptr(al), ptr(da), C, ptr(db), C, ptr(dalpha),
                   ptr(part), _npix(a), C, stream())
        return da, db, dalpha.reshape(ctx.ashape)


def mul2_scalar(a, b, alpha):
    return _Mul2Scalar.apply(a, b, alpha)


# ----------------------------------------------------------------------------------------------------------
# ELA (Efficient Local Attention, src/EGM-UNet.py:56-79)
# ----------------------------------------------------------------------------------------------------------
class _ELA(Function):
    @staticmethod
    def forward(ctx, x, conv_w, gamma, beta, groups, eps):
        x, ldx = _nhwc(x)
        N, H, W, C = x.shape
        L, dt, st, dev = lib(), dtype_code(x.dtype), stream(), x.device
        ks = conv_w.shape[-1]
        cw = conv_w.detach().reshape(C, ks).contiguous()
        mh, mw = _f32((N, H, C), dev), _f32((N, W, C), dev)
        L.call("egm_ela_strip_means", dt, ptr(x), ldx, ptr(mh), ptr(mw), N, H, W, C, st)
        yh, yw, gh, gw = _f32((N, H, C), dev), _f32((N, W, C), dev), _f32((N, H, C), dev), _f32((N, W, C), dev)
        stats = _f32((N, 2, groups, 2), dev)
        L.call("egm_ela_gates_fwd", ptr(mh), ptr(mw), ptr(cw), ks, ptr(gamma.detach()), ptr(beta.detach()), float(eps), ptr(yh), ptr(yw), ptr(gh),
               ptr(gw), ptr(stats), N, H, W, C, groups, st)
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=dev)
        L.call("egm_ela_apply", dt, ptr(x), ldx, ptr(gh), ptr(gw), ptr(out), C, N, H, W, C, st)
        ctx.save_for_backward(x, mh, mw, yh, yw, gh, gw, stats, cw, gamma)
        ctx.meta = (groups, ks, conv_w.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        x, mh, mw, yh, yw, gh, gw, stats, cw, gamma = ctx.saved_tensors
        groups, ks, wshape = ctx.meta
        x, ldx = _nhwc(x); g, ldg = _nhwc(g)
        N, H, W, C = x.shape
        L, dt, st, dev = lib(), dtype_code(x.dtype), stream(), x.device
        ws = torch.empty(L.query("egm_ela_bwd_workspace", N, H, W, C, ks) // 4 + 4, dtype=torch.float32, device=dev)
        dx = torch.empty((N, H, W, C), dtype=x.dtype, device=dev)
        dcw, dgamma, dbeta = _f32((C, ks), dev), _f32(C, dev), _f32(C, dev)
        L.call("egm_ela_bwd", dt, ptr(g), ldg, ptr(x), ldx, ptr(mh), ptr(mw), ptr(yh), ptr(yw), ptr(gh), ptr(gw), ptr(stats), ptr(cw), ks,
               ptr(gamma.detach()), ptr(dx), C, ptr(dcw), ptr(dgamma), ptr(dbeta), ptr(ws), N, H, W, C, groups, st)
        return dx, dcw.reshape(wshape), dgamma, dbeta, None, None


def ela(x, conv, gn):
    """conv: nn.Conv1d(C, C, k, padding=k//2, groups=C, bias=False); gn: nn.GroupNorm(G, C) -- parameter holders"""
    return _ELA.apply(x, conv.weight, gn.weight, gn.bias, gn.num_groups, gn.eps)


# ----------------------------------------------------------------------------------------------------------
# MCALayer
# ----------------------------------------------------------------------------------------------------------
class _MCALayer(Function):
    """wc / kc None: MCALayer(no_spatial=True) -- two gates, x_out = x*(g_h+g_w)/2 (src/EGM-UNet.py:766-771)"""

    @staticmethod
    def forward(ctx, x, x_coef, x_act, wh, kh, ww, kw, wc, kc, training, exclusive=False):
        """x_coef / x_act: x is a Lazy's stand-in (the raw output of the conv in front; ops.Lazy): its BatchNorm + activation is applied
        by the statistics pass, which writes the materialised tensor on the way (egm_mca_reduce_bn)."""
        x, ldx = _nhwc(x)
        N, H, W, C = x.shape
        L, dt, st, dev = lib(), dtype_code(x.dtype), stream(), x.device
        Lax = H + W + C
        ws = torch.empty(L.query("egm_mca_reduce_workspace", N, H, W, C) // 4 + 4, dtype=torch.float32, device=dev)
        sums = _f32((N, Lax, 2), dev)
        if x_coef is not None:
            z = torch.empty((N, H, W, C), dtype=x.dtype, device=dev)
            L.call("egm_mca_reduce_bn", dt, ptr(x), ldx, ptr(x_coef[0]), ptr(x_coef[1]), x_act, ptr(z), C, ptr(sums), ptr(ws), N, H, W, C, st)
            x, ldx = z, C
        else:
            L.call("egm_mca_reduce", dt, 0, ptr(x), ldx, None, 0, ptr(sums), ptr(ws), N, H, W, C, st)
        stats, o, gates = _f32((N, Lax, 2), dev), _f32((N, Lax), dev), _f32((N, Lax), dev)
        ps = [t.detach().contiguous() for t in (wh, kh, ww, kw, wc, kc) if t is not None]
        ns = int(wc is None)
        ks = (kh.numel(), kw.numel(), 0 if ns else kc.numel())
        pc = (None, None) if ns else (ptr(ps[4]), ptr(ps[5]))
        L.call("egm_mca_gates_fwd", ptr(sums), ptr(ps[0]), ptr(ps[1]), ks[0], ptr(ps[2]), ptr(ps[3]), ks[1], pc[0], pc[1], ks[2],
               ptr(stats), ptr(o), ptr(gates), N, H, W, C, st)
        # x_out = x * gate, the 3x3 stencils (range, squared high-pass, its average), the channel shuffle and the sum: one fused pass
        xo = torch.empty((N, H, W, C), dtype=x.dtype, device=dev) if training else None
        codes = torch.empty((N, H, W, C), dtype=torch.uint8, device=dev) if training else None
        out = torch.empty((N, H, W, C), dtype=x.dtype, device=dev)
        L.call("egm_mca_fused_fwd", dt, ptr(x), ldx, ptr(gates), ptr(xo), C, ptr(out), C, ptr(codes), N, H, W, C, ns, st)
        if training:
            ctx.save_for_backward(x, xo, codes, stats, o, gates, *ps)
            ctx.ks = ks
            # exclusive: the caller vouches that the conv -> BatchNorm stand-in this layer materialised feeds nothing else, so the last
            # backward step (dx) can be left to that BatchNorm's backward (see _defer_dz)
            ctx.defer_dx = bool(exclusive and x_coef is not None and _dz_fusable(C))
        return out

    @staticmethod
    def backward(ctx, g):
        x, xo, codes, stats, o, gates, wh, kh, ww, kw, *pc = ctx.saved_tensors
        ks = ctx.ks
        ns = int(not pc)
        x, ldx = _nhwc(x); g, ldg = _nhwc(g)
        N, H, W, C = x.shape
        L, dt, st, dev = lib(), dtype_code(x.dtype), stream(), x.device
        Lax = H + W + C
        dxo = torch.empty_like(xo)
        if fuse_mca_bwd.on and x.dtype == torch.bfloat16:
            # du and dxo in one tiled pass: the 3 x 3 neighbourhoods come from LDS, du never reaches memory
            L.call("egm_mca_bwd_dudxo", dt, ptr(codes), ptr(xo), C, ptr(g), ldg, ptr(dxo), C, N, H, W, C, st)
        else:
            du = torch.empty_like(xo)
            L.call("egm_mca_bwd_du", dt, ptr(xo), C, ptr(g), ldg, ptr(du), C, N, H, W, C, st)
            L.call("egm_mca_bwd_dxo", dt, ptr(codes), ptr(g), ldg, ptr(du), C, ptr(dxo), C, N, H, W, C, st)
        ws = torch.empty(L.query("egm_mca_reduce_workspace", N, H, W, C) // 4 + 4, dtype=torch.float32, device=dev)
        dG = _f32((N, Lax, 2), dev)
        L.call("egm_mca_reduce", dt, 1, ptr(dxo), C, ptr(x), ldx, ptr(dG), ptr(ws), N, H, W, C, st)
        dz = _f32((N, Lax), dev)
        coef = _f32((N, Lax, 2), dev)
        dwts = _f32((3, 2), dev)
        dks = _f32((3, 8), dev)                                  # zeroed by the kernel itself
        L.call("egm_mca_gates_bwd", ptr(dG), ptr(stats), ptr(o), ptr(gates), ptr(wh), ptr(kh), ks[0], ptr(ww), ptr(kw), ks[1],
               None if ns else ptr(pc[0]), None if ns else ptr(pc[1]), ks[2], ptr(dz), ptr(coef), ptr(dwts), ptr(dks), N, H, W, C, st)
        if ctx.defer_dx and fuse_dz.on:
            dx = dxo                                            # stand-in: the BatchNorm backward in front evaluates dx per vector itself
            _defer_dz(dxo, ("mca", dxo, C, gates, coef, ns, (N, H, W)))
        else:
            dx = torch.empty((N, H, W, C), dtype=x.dtype, device=dev)
            L.call("egm_mca_bwd_dx", dt, ptr(dxo), C, ptr(x), ldx, ptr(gates), ptr(coef), ptr(dx), C, N, H, W, C, ns, st)
        gk = [dks[a, :ks[a]].reshape(1, 1, 1, ks[a]) for a in range(2 if ns else 3)]
        if ns:
            return dx, None, None, dwts[0], gk[0], dwts[1], gk[1], None, None, None, None
        return dx, None, None, dwts[0], gk[0], dwts[1], gk[1], dwts[2], gk[2], None, None


def mca_layer(x, layer, training, exclusive=False):
    """layer: an MCALayer parameter holder with gates h_cw, w_hc and -- unless layer.no_spatial -- c_hw
    (each: .weight [2], .conv.weight [1,1,1,k])."""
    c = (None, None) if layer.no_spatial else (layer.c_hw.weight, layer.c_hw.conv.weight)
    xt, xc, xa = _unlazy(x)                   # a Lazy (conv_bn_lazy) is materialised by the layer's own statistics pass
    C = xt.shape[3]
    if xc is not None and not (8 <= C <= 512 and (C & (C - 1)) == 0):
        xt, xc, xa = materialize(x), None, ACT_NONE
    return _MCALayer.apply(xt, xc, xa, layer.h_cw.weight, layer.h_cw.conv.weight, layer.w_hc.weight, layer.w_hc.conv.weight, c[0], c[1],
                           training, exclusive and xc is not None)


class _SAConv7(Function):
    """SpatialAttentionModule.conv1 (7x7, 2->1) on the (mean, max) map as a direct stencil."""

    @staticmethod
    def forward(ctx, x, w):
        x, ldx = _nhwc(x)
        N, H, W, _ = x.shape
        wd = w.detach().contiguous()
        y = torch.empty((N, H, W, 8), dtype=x.dtype, device=x.device)
        lib().call("egm_sa_conv7_fwd", dtype_code(x.dtype), ptr(x), ldx, ptr(wd), ptr(y), 8, N, H, W, stream())
        ctx.save_for_backward(x, wd)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        x, ldx = _nhwc(x); g, ldg = _nhwc(g)
        N, H, W, _ = x.shape
        L, dev = lib(), x.device
        dx = torch.empty((N, H, W, 8), dtype=x.dtype, device=dev)
        dw = torch.empty((1, 2, 7, 7), dtype=torch.float32, device=dev)
        ws = torch.empty(L.query("egm_sa_conv7_bwd_workspace", N, H, W) // 4 + 4, dtype=torch.float32, device=dev)
        L.call("egm_sa_conv7_bwd", dtype_code(x.dtype), ptr(x), ldx, ptr(g), ldg, ptr(w), ptr(dx), 8, ptr(dw), ptr(ws), N, H, W, stream())
        return dx, dw


def sa_conv7(x, w):
    return _SAConv7.apply(x, w)
