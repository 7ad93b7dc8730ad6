"""Boundary loss (Kervadec et al., MIDL 2019 / Medical Image Analysis 2021) on the HIP library: the signed distance maps of the int64
target are made on the device (csrc/sdf.hip, two launches), so the term works on batches that never sat on the host and inside a
captured training step.

    b = BoundaryLoss(classes=(1,), weight=0.01, ignore_index=255)
    loss = criterion(model(x), target, lw, num_classes=2, ignore_index=255, boundary=b)      # five terms + w * L_B
    for epoch in range(epochs):
        b.set_weight(b.schedule(epoch))          # the paper's linear increase; a replayed graph follows it without a new capture
        train_one_epoch(model, opt, loader, device, epoch, 2, sched, boundary=b)

s_k(p) (signed_distance2) is the exact signed squared Euclidean distance of pixel p to the contour of class k: negative inside, positive
outside, 0 at an ignored pixel and on a plane without a contour (a class that is absent, or that has no valid pixel outside it).
phi_k = sqrt(s) outside, -(sqrt(-s) - 1) inside (the official one_hot2dist);
L_B = (1/D) sum phi_k(p) softmax(x)[class k](p), D = K * max(1, valid pixels of the batch): DESIGN.md 6.29."""
import ctypes

import torch
from torch.autograd import Function

from .._lib import lib, ptr, require_gpu, stream

MAX_CLASSES = 4            # kSdfMaxK of csrc/sdf.hip
MAX_SIDE = 32767           # kSdfMaxSide: |s| < 2^31 and a row distance fits 16 bits


def _class_ids(classes):
    ids = tuple(int(c) for c in classes)
    if not 1 <= len(ids) <= MAX_CLASSES:
        raise ValueError(f"boundary loss: {len(ids)} classes, between 1 and {MAX_CLASSES} are supported")
    if len(set(ids)) != len(ids) or min(ids) < 0:
        raise ValueError(f"boundary loss: class ids {ids} must be distinct and non-negative")
    return ids


def _c_ids(ids):
    return (ctypes.c_int * len(ids))(*ids)


def _target(name, target):
    if not target.is_cuda:
        raise RuntimeError(f"{name}: the target must live on the GPU")
    if target.dim() != 3:
        raise RuntimeError(f"{name}: the target must be [N, H, W], got {tuple(target.shape)}")
    if target.shape[1] > MAX_SIDE or target.shape[2] > MAX_SIDE:
        raise ValueError(f"{name}: {target.shape[1]} x {target.shape[2]} pixels, at most {MAX_SIDE} rows and columns are supported")
    return target.contiguous().to(torch.int64)


def signed_distance2(target, classes=(1,), ignore_index=255):
    """int64 CUDA target [N, H, W] -> int32 [N, K, H, W]: the exact signed squared distance of every pixel to the contour of each of
    the K classes (see the module's text).  Two launches, nothing waits for the device."""
    require_gpu()
    ids = _class_ids(classes)
    t = _target("signed_distance2", target)
    N, H, W = t.shape
    K, L = len(ids), lib()
    ws = torch.empty(L.query("egm_sdf_workspace", N, H, W, K), dtype=torch.uint8, device=t.device)
    s = torch.empty((N, K, H, W), dtype=torch.int32, device=t.device)
    L.call("egm_target_sdf_i64", ptr(t), N, H, W, _c_ids(ids), K, int(ignore_index), ptr(ws), ptr(s), stream())
    return s


def distance_maps(target, classes=(1,), ignore_index=255):
    """fp32 [N, K, H, W]: phi of the official one_hot2dist from signed_distance2, for inspection and tests (the loss never stores it)."""
    s = signed_distance2(target, classes, ignore_index)
    phi = torch.empty(s.shape, dtype=torch.float32, device=s.device)
    lib().call("egm_sdf_phi_f32", ptr(s), s.numel(), ptr(phi), stream())
    return phi


class _BoundaryTerm(Function):
    @staticmethod
    def forward(ctx, logits, target, sdf, ids, ignore_index, w_dev):
        x = logits.contiguous().float()
        N, C, H, W = x.shape
        K, L, dev = len(ids), lib(), x.device
        ws = torch.empty(L.query("egm_bloss_workspace", N, C, H, W), dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        L.call("egm_bloss_fwd", ptr(x), ptr(sdf), ptr(target), _c_ids(ids), K, N, C, H, W, int(ignore_index), ptr(w_dev), ptr(ws), ptr(out),
               stream())
        ctx.save_for_backward(x, sdf, ws, w_dev)
        ctx.ids = ids
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return out[0], out

    @staticmethod
    def backward(ctx, g, _g2):
        if g is None:
            return None, None, None, None, None, None
        x, sdf, ws, w_dev = ctx.saved_tensors
        N, C, H, W = x.shape
        dl = torch.empty_like(x)
        g = g.contiguous().float()
        lib().call("egm_bloss_bwd", ptr(x), ptr(sdf), _c_ids(ctx.ids), len(ctx.ids), N, C, H, W, ptr(ws), ptr(g), ptr(w_dev), ptr(dl), stream())
        return dl, None, None, None, None, None


class BoundaryLoss:
    """The boundary term for `criterion`, `train_one_epoch` and `GraphedTrainStep` (their `boundary=` argument).  The weight lives in a
    device scalar (`weight_dev`) that the kernels read, as the optimizer's learning rate does, so `set_weight` before an epoch is
    followed by a step that was captured earlier."""

    def __init__(self, classes=(1,), weight=0.01, ignore_index=255):
        self.classes = _class_ids(classes)
        self.ignore_index = int(ignore_index)
        self.weight = float(weight)
        self.weight_dev = None              # made on the first use, on the device of the logits
        self.raw = None                     # the last unweighted L_B, a device scalar
        self._pinned = None
        self._events = [None, None]
        self._turn = 0

    @staticmethod
    def schedule(epoch, start=0.01, step=0.01, cap=1.0):
        """The paper's linear increase of the weight over the epochs."""
        return min(float(cap), float(start) + float(step) * int(epoch))

    def _ensure(self, device):
        if self.weight_dev is None:
            require_gpu()
            self.weight_dev = torch.zeros(1, dtype=torch.float32, device=device)
            self._pinned = [torch.zeros(1, dtype=torch.float32).pin_memory() for _ in range(2)]
            self._upload()

    def _upload(self):
        # two pinned scalars used in turn, each rewritten only after the upload that last read it has executed (the device runs behind
        # the host): train_one_epoch's rule for the learning rate
        k = self._turn
        self._turn ^= 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._pinned[k][0] = self.weight
        self.weight_dev.copy_(self._pinned[k], non_blocking=True)
        if self._events[k] is None:
            self._events[k] = torch.cuda.Event()
        self._events[k].record()

    def set_weight(self, w):
        """A new weight for the steps enqueued after this call: an asynchronous upload, no wait for the device."""
        self.weight = float(w)
        if self.weight_dev is not None:
            self._upload()

    def sdf(self, target):
        return signed_distance2(target, self.classes, self.ignore_index)

    def loss(self, logits, target, sdf=None):
        """-> the weighted scalar w * L_B (an autograd node); `sdf` = signed_distance2 of this target made ahead by the caller."""
        require_gpu()
        if not (logits.is_cuda and target.is_cuda):
            raise RuntimeError("boundary loss: logits and target must live on the GPU")
        t = _target("boundary loss", target)
        N, C, H, W = logits.shape
        if t.shape != (N, H, W):
            raise RuntimeError(f"boundary loss: target shape {tuple(t.shape)} does not match logits {tuple(logits.shape)}")
        if max(self.classes) >= C:
            raise ValueError(f"boundary loss: class ids {self.classes} outside [0, {C})")
        if sdf is None:
            sdf = self.sdf(t)
        elif sdf.dtype != torch.int32 or sdf.shape != (N, len(self.classes), H, W) or not sdf.is_cuda:
            raise RuntimeError(f"boundary loss: sdf must be an int32 CUDA tensor of shape {(N, len(self.classes), H, W)}")
        self._ensure(logits.device)
        loss, both = _BoundaryTerm.apply(logits, t, sdf.contiguous(), self.classes, self.ignore_index, self.weight_dev)
        self.raw = both[1]
        return loss
