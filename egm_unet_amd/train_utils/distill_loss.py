"""Knowledge distillation (Hinton, Vinyals, Dean 2015) on the HIP library: a student is trained against the logits of a frozen teacher
(csrc/distill.hip).  The teacher's forward runs inside the captured training step, so a step stays one graph replay.

    t = ModelTeacher(big_unet)                                   # or EnsembleTeacher(unet, clipseg, prompts, alpha, ...)
    d = Distill(t, temperature=2.0, weight=1.0, ignore_index=255, min_confidence=0.0)
    train_one_epoch(student, opt, loader, device, epoch, 2, sched, distill=d)
    # by hand: d.refresh(); d.prepare(x); loss = criterion(student(x), target, lw, num_classes=2, ignore_index=255, distill=d)

With q = softmax(x / T) of the student, p = softmax(z / T) of the teacher and V the valid pixels of the batch

    L_KD = T^2 / max(1, V) * sum over the valid pixels of sum_c p_c (log p_c - log q_c)

A pixel is valid when its target is not ignore_index (no target, or ignore_index=None: every pixel) and the teacher's confidence
max_c softmax(z)_c at T = 1 is at least min_confidence (0 switches the floor off).  DESIGN.md 6.35.

Unlabelled photos need no entry point of their own: after d.prepare(x), d.pseudo_target() gives the teacher's hard labels where it is
confident and ignore_index elsewhere, which every term of the criterion takes as a target:

    d.refresh(); d.prepare(x)
    target = d.pseudo_target()                                   # or d.pseudo_target(partial_target): its ignored pixels stay ignored
    loss = criterion(student(x), target, lw, num_classes=2, ignore_index=255, distill=d)

(a loader of unlabelled photos yields an all-ignore_index target: with Distill(ignore_index=None) the KD term then trains on every
pixel while the five supervised terms see no valid pixel).

Whether distillation raises the student's mIoU on the crack data set is not measured here."""
import torch
from torch.autograd import Function

from .._lib import dtype_code, lib, ptr, require_gpu, stream

MAX_CLASSES = 16           # kDistillMaxC of csrc/distill.hip


def _teacher_logits(name, z):
    if not isinstance(z, torch.Tensor) or z.dim() != 4:
        raise RuntimeError(f"{name}: teacher logits must be a tensor [N, C, H, W]")
    if not z.is_cuda:
        raise RuntimeError(f"{name}: teacher logits must live on the GPU")
    if z.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"{name}: teacher logits must be float32 or bfloat16, got {z.dtype}")
    if z.shape[1] > MAX_CLASSES:
        raise ValueError(f"{name}: {z.shape[1]} classes, at most {MAX_CLASSES} are supported")
    return z.detach().contiguous()


class _DistillTerm(Function):
    @staticmethod
    def forward(ctx, logits, z, target, ignore_index, temperature, w_dev, tau_dev):
        x = logits.contiguous().float()
        N, C, H, W = x.shape
        L, dev = lib(), x.device
        ws = torch.empty(L.query("egm_distill_workspace", N, C, H, W), dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        valid = torch.empty(1, dtype=torch.int64, device=dev)
        has_ignore = ignore_index is not None
        ctx.args = (dtype_code(z.dtype), N, C, H, W, int(has_ignore), int(ignore_index) if has_ignore else 0, float(temperature))
        L.call("egm_distill_fwd", ptr(x), ptr(z), ctx.args[0], ptr(target), *ctx.args[1:], ptr(w_dev), ptr(tau_dev), ptr(ws), ptr(out),
               ptr(valid), stream())
        ctx.target = target                                    # (int64: not a tensor autograd has to track)
        ctx.save_for_backward(x, z, ws, w_dev, tau_dev)
        ctx.mark_non_differentiable(out, valid)
        ctx.set_materialize_grads(False)
        return out[0], out, valid

    @staticmethod
    def backward(ctx, g, _g2, _g3):
        if g is None:
            return None, None, None, None, None, None, None
        x, z, ws, w_dev, tau_dev = ctx.saved_tensors
        dl = torch.empty_like(x)
        g = g.contiguous().float()
        lib().call("egm_distill_bwd", ptr(x), ptr(z), ctx.args[0], ptr(ctx.target), *ctx.args[1:], ptr(w_dev), ptr(tau_dev), ptr(ws), ptr(g),
                   ptr(dl), stream())
        return dl, None, None, None, None, None, None


class Distill:
    """The distillation term for `criterion`, `train_one_epoch` and `GraphedTrainStep` (their `distill=` argument).  The weight and the
    confidence floor live in device scalars (`weight_dev`, `tau_dev`) that the kernels read, so `set_weight` and `set_min_confidence`
    are followed by a step that was captured earlier.  `raw` is the last unweighted L_KD and `valid` the last count of valid pixels,
    both device scalars.

    teacher: a callable x -> logits [N, C, H, W] (ModelTeacher, EnsembleTeacher) with a refresh() method, or None when the logits
    come from set_teacher_logits (computed ahead of time)."""

    def __init__(self, teacher=None, temperature=2.0, weight=1.0, ignore_index=255, min_confidence=0.0):
        if not float(temperature) > 0.0:
            raise ValueError(f"distillation: temperature must be > 0, got {temperature}")
        if not 0.0 <= float(min_confidence) <= 1.0:
            raise ValueError(f"distillation: min_confidence must lie in [0, 1], got {min_confidence}")
        self.teacher = teacher
        self.temperature = float(temperature)
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.weight = float(weight)
        self.min_confidence = float(min_confidence)
        self.weight_dev = None              # both scalars are made on the first use, on the device of the logits
        self.tau_dev = None
        self.raw = None                     # the last unweighted L_KD, a device scalar
        self.valid = None                   # the last count of valid pixels, a device scalar (int64)
        self.logits = None                  # the teacher's logits of the prepared batch
        self._scalars = None
        self._pinned = None
        self._events = [None, None]
        self._turn = 0

    # ---- device scalars
    def _ensure(self, device):
        if self.weight_dev is None:
            require_gpu()
            self._scalars = torch.zeros(2, dtype=torch.float32, device=device)
            self.weight_dev, self.tau_dev = self._scalars[0:1], self._scalars[1:2]
            self._pinned = [torch.zeros(2, dtype=torch.float32).pin_memory() for _ in range(2)]
            self._upload()

    def _upload(self):
        # two pinned buffers used in turn, each rewritten only after the upload that last read it has executed (the device runs behind
        # the host): train_one_epoch's rule for the learning rate
        k = self._turn
        self._turn ^= 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._pinned[k][0] = self.weight
        self._pinned[k][1] = self.min_confidence
        self._scalars.copy_(self._pinned[k], non_blocking=True)
        if self._events[k] is None:
            self._events[k] = torch.cuda.Event()
        self._events[k].record()

    def set_weight(self, w):
        """A new weight for the steps enqueued after this call: an asynchronous upload, no wait for the device."""
        self.weight = float(w)
        if self.weight_dev is not None:
            self._upload()

    def set_min_confidence(self, tau):
        """A new confidence floor for the steps (and pseudo_target calls) enqueued after this call, likewise."""
        if not 0.0 <= float(tau) <= 1.0:
            raise ValueError(f"distillation: min_confidence must lie in [0, 1], got {tau}")
        self.min_confidence = float(tau)
        if self.weight_dev is not None:
            self._upload()

    # ---- the teacher
    def bind(self, student):
        """Refuse a teacher whose model (its `model` attribute) is `student` or shares parameters with it; GraphedTrainStep and
        train_one_epoch call this with the model they train."""
        tm = getattr(self.teacher, "model", None)
        if tm is not None:
            refuse_student(tm, student)

    def refresh(self):
        """Bring the teacher's folded weights up to date (outside any graph; nothing to do without a teacher object)."""
        if self.teacher is not None and hasattr(self.teacher, "refresh"):
            self.teacher.refresh()

    def prepare(self, image):
        """Run the teacher on the student's batch under torch.no_grad() and keep its logits for the next loss() calls (eager, or being
        captured: GraphedTrainStep calls it inside its graph, ahead of the student's forward)."""
        if self.teacher is None:
            raise RuntimeError("distillation: prepare() needs a teacher; pass one, or hand precomputed logits to set_teacher_logits()")
        with torch.no_grad():
            z = self.teacher(image)
        if isinstance(z, dict):
            z = z["out"]
        self.logits = _teacher_logits("distillation", z)
        return self.logits

    def set_teacher_logits(self, z):
        """Precomputed teacher logits [N, C, H, W] (float32 or bfloat16, on the GPU) for the next loss() calls."""
        self.logits = _teacher_logits("distillation", z)

    # ---- the term
    def loss(self, logits, target=None):
        """-> the weighted scalar w * L_KD (an autograd node) of the student's logits against the prepared teacher logits."""
        if self.logits is None:
            raise RuntimeError("distillation: no teacher logits prepared (call prepare(image) or set_teacher_logits(z) first)")
        if not logits.is_cuda or (target is not None and not target.is_cuda):
            raise RuntimeError("distillation: logits and target must live on the GPU")
        z = self.logits
        if logits.dim() != 4 or tuple(logits.shape) != tuple(z.shape):
            raise RuntimeError(f"distillation: student logits {tuple(logits.shape)} and teacher logits {tuple(z.shape)} must have one shape "
                               "[N, C, H, W] (the same class count)")
        N, C, H, W = logits.shape
        if C > MAX_CLASSES:
            raise ValueError(f"distillation: {C} classes, at most {MAX_CLASSES} are supported")
        if target is not None:
            if tuple(target.shape) != (N, H, W):
                raise RuntimeError(f"distillation: target shape {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
            target = target.contiguous().to(torch.int64)
        require_gpu()
        self._ensure(logits.device)
        loss, both, valid = _DistillTerm.apply(logits, z, target, self.ignore_index, self.temperature, self.weight_dev, self.tau_dev)
        self.raw, self.valid = both[1], valid[0]
        return loss

    def pseudo_target(self, target=None, ignore_index=255):
        """int64 [N, H, W] from the prepared teacher logits: the argmax class (ties to the lowest class) where the teacher's confidence
        is at least min_confidence, ignore_index elsewhere and wherever `target` (an existing int64 target) is ignore_index.  One
        launch, nothing waits for the device."""
        if self.logits is None:
            raise RuntimeError("distillation: no teacher logits prepared (call prepare(image) or set_teacher_logits(z) first)")
        require_gpu()
        z = self.logits
        N, C, H, W = z.shape
        if target is not None:
            if not target.is_cuda or tuple(target.shape) != (N, H, W):
                raise RuntimeError(f"distillation: pseudo_target needs a CUDA target of shape {(N, H, W)}")
            target = target.contiguous().to(torch.int64)
        self._ensure(z.device)
        out = torch.empty((N, H, W), dtype=torch.int64, device=z.device)
        lib().call("egm_pseudo_target_i64", ptr(z), dtype_code(z.dtype), ptr(target), N, C, H, W, int(ignore_index), ptr(self.tau_dev),
                   ptr(out), stream())
        return out


def refuse_student(teacher_model, student):
    """ValueError when the teacher's model is the student object or shares parameters with it: the predictor's forward switches the
    training flags of its model off and on, and the student's update would move the teacher."""
    core = student.module if hasattr(student, "module") else student
    objs = {id(p) for p in core.parameters()}
    addrs = {p.data_ptr() for p in core.parameters() if p.numel()}
    if core is teacher_model or any(id(p) in objs or (p.numel() and p.data_ptr() in addrs) for p in teacher_model.parameters()):
        raise ValueError("distillation: the teacher is the student itself or shares parameters with it; pass a separate frozen copy")


class ModelTeacher:
    """A frozen GRFBUNet / UNet as the teacher: the folded eval forward of an infer.Predictor(model, graph=False), made to run inside
    the training step's graph.  The constructor sets requires_grad_(False) on the model's parameters: a teacher never gets a gradient.

    Distill.bind(student), called by GraphedTrainStep and train_one_epoch, refuses a teacher whose model is the student object or
    shares parameters with it (refuse_student)."""

    def __init__(self, model, dtype=None):
        from ..infer import Predictor
        self._pred = Predictor(model, dtype=dtype, graph=False)
        self.model = self._pred.model
        for p in self.model.parameters():
            p.requires_grad_(False)

    def refresh(self):
        self._pred.refresh()

    def __call__(self, x):
        with torch.no_grad():
            return self._pred._forward(x)


class EnsembleTeacher:
    """The CLIPSeg (+) UNet ensemble as the teacher, on the student's own batch: EnsemblePredictor._run_batch without its uint8 front end
    and its mask tail.  x is the student's crop, normalised with (unet_mean, unet_std):

        fuse_logits(clipseg._decode_multi(renorm_resize(x), condT).view(N, K, ch, cw), Predictor(unet)(x), alpha)

    One prompt per class of the UNet (strings or a [K, 512] tensor).  alpha lives in a device scalar: `t.alpha = 2.0` is followed by a
    captured step.  refresh() refolds the UNet and, when the CLIPSeg model's stamp changed (parameters, compute dtype, the generation
    counters of raw-pointer optimizers), recomputes the conditionals and raises `stale`: the cast-weight buffers a captured graph
    points at have moved, so GraphedTrainStep turns the flag into an error.  Both models are set to requires_grad_(False)."""

    def __init__(self, unet, clipseg, prompts, alpha=0.5, unet_mean=(0.709, 0.381, 0.224), unet_std=(0.127, 0.079, 0.043),
                 clip_mean=(0.485, 0.456, 0.406), clip_std=(0.229, 0.224, 0.225), clip_size=352, clip_antialias=True, dtype=None):
        from ..infer import Predictor
        require_gpu()
        self._unet = Predictor(unet, dtype=dtype, graph=False)
        self.model = self._unet.model
        self.clipseg = clipseg
        for p in list(self.model.parameters()) + list(clipseg.parameters()):
            p.requires_grad_(False)
        dev = next(self.model.parameters()).device
        self.num_classes = int(self.model.num_classes)
        self._prompts = prompts if isinstance(prompts, torch.Tensor) else list([prompts] if isinstance(prompts, str) else prompts)
        K = self._prompts.shape[0] if isinstance(self._prompts, torch.Tensor) else len(self._prompts)
        if K != self.num_classes:
            raise ValueError(f"EnsembleTeacher: {K} prompts for a UNet with {self.num_classes} classes (one prompt per class)")
        self.unet_mean, self.unet_std, self.clip_mean, self.clip_std = tuple(unet_mean), tuple(unet_std), tuple(clip_mean), tuple(clip_std)
        self.clip_size = (clip_size, clip_size) if isinstance(clip_size, int) else (int(clip_size[0]), int(clip_size[1]))
        self.clip_antialias = bool(clip_antialias)
        self._alpha = torch.empty(1, dtype=torch.float32, device=dev)
        self._alpha_value = None
        self.alpha = alpha
        self._clip_tensors = list(clipseg.parameters()) + list(clipseg.buffers())
        self._clip_stamp = None
        self._condT = None
        self.stale = False                  # the CLIPSeg stamp changed after the first refresh: graphs that hold this teacher are invalid

    @property
    def alpha(self):
        return self._alpha_value

    @alpha.setter
    def alpha(self, v):
        self._alpha_value = float(v)
        self._alpha.fill_(self._alpha_value)               # a fill kernel with the value as its argument: no host wait

    def refresh(self):
        from ..clip import ops as clip_ops
        self._unet.refresh()
        cs = self.clipseg
        # the stamp of EnsemblePredictor._refresh without ops._weight_generation: the student's optimizer bumps that counter every step,
        # and a frozen CLIPSeg is written by nobody (an optimizer that did write it through raw pointers bumps clip_ops._cast_generation)
        stamp = (cs.compute_dtype, clip_ops._cast_generation[0], tuple((t._version, t.data_ptr()) for t in self._clip_tensors))
        if stamp != self._clip_stamp:
            with torch.no_grad():
                self._condT = cs._cond_in_dtype(cs._multi_cond(self._prompts))
            self.stale = self._clip_stamp is not None
            self._clip_stamp = stamp

    def __call__(self, x):
        from .. import data
        from ..ensemble import fuse_logits
        if self._condT is None:
            raise RuntimeError("EnsembleTeacher: refresh() must run before the first forward (outside any graph)")
        with torch.no_grad():
            N = x.shape[0]
            xc = data.renorm_resize(x, self.clip_size, self.unet_mean, self.unet_std, self.clip_mean, self.clip_std, self.clip_antialias)
            out = self.clipseg._decode_multi(xc, self._condT)
            clip_l = out.view(N, self._condT.shape[0], out.shape[-2], out.shape[-1])
            return fuse_logits(clip_l, self._unet._forward(x), self._alpha)
