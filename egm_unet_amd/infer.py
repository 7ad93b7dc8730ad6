"""Inference path of GRFBUNet / UNet: BatchNorm folded into the convolutions, the activation in the conv epilogue, the forward replayed
as a hipGraph per input shape (the reference's predict.py:64-75 / predict_CLIPseg.py:478-490 time exactly this: model.eval() at batch 1).

    from egm_unet_amd.infer import Predictor, evaluate
    pred = Predictor(model)                      # dtype None = model.compute_dtype
    out = pred(x)["out"]                         # like model.eval()(x)["out"]: fp32 NCHW logits
    mask = pred.predict_mask(x, lut=None)        # uint8 [N, H, W]
    confmat, dice = evaluate(model, val_loader, device, num_classes)

The predictor always uses the running statistics, whatever model.training is, and leaves the model as it found it (training flags,
parameters, buffers, num_batches_tracked).  model(x) itself is unchanged in train and eval mode.
"""
import struct
import types

import torch
import torch.nn as nn

from . import ops
from ._lib import dtype_code, lib, ptr, require_gpu, stream
from .replay import ReplayCache

_FOLD_ENTRY = struct.Struct("<8Qf9i")             # egm_conv_fold_pack_multi table entry (include/egm_hip.h), 104 bytes
_MISSING = object()


def lut256(lut, C, device, who="lut"):
    """A colour map (None, or a sequence / tensor of C..256 values) as the 256-entry uint8 table on the device the mask kernels read."""
    if lut is None:
        return None
    lt = torch.as_tensor(lut).to(torch.uint8).flatten()
    if lt.numel() < C or lt.numel() > 256:
        raise ValueError(f"{who} must have between {C} and 256 entries, got {lt.numel()}")
    return torch.cat([lt.cpu(), torch.zeros(256 - lt.numel(), dtype=torch.uint8)]).to(device)


def _conv_bn_pairs(model):
    """(conv, bn) holders where the model's forward runs conv -> BatchNorm through ops' conv -> BatchNorm entry points: nn.Sequential
    runs [Conv2d, BatchNorm2d] (DoubleConv, DoubleConv1, the EdgeAware weight generator) and blocks holding .conv and .bn (BasicConv, Conv)."""
    pairs = []
    for m in model.modules():
        if isinstance(getattr(m, "conv", None), nn.Conv2d) and isinstance(getattr(m, "bn", None), nn.BatchNorm2d):
            pairs.append((m.conv, m.bn))
        if isinstance(m, nn.Sequential):
            kids = list(m)
            for a, b in zip(kids, kids[1:]):
                if isinstance(a, nn.Conv2d) and isinstance(b, nn.BatchNorm2d):
                    pairs.append((a, b))
    seen, out = set(), []
    for c, b in pairs:
        if id(c) not in seen:
            seen.add(id(c))
            out.append((c, b))
    return out


class Predictor:
    """Eval-mode forward of a GRFBUNet / UNet (use_mca=False twin included) with folded BatchNorm, replayed as a hipGraph.

    dtype: activation dtype (None = model.compute_dtype).  graph: capture one hipGraph per (N, H, W, dtype) -- the first call at a shape
    runs the folded forward eagerly (the warm-up), the second captures and replays; at most max_graphs are kept, least recently used
    first out.  graph=False always runs the folded forward eagerly.

    The returned logits of a graph replay are the graph's static output: the next call at the same shape overwrites them.  Pass
    clone=True (or clone the tensor) to keep them.  Every call compares a stamp of the parameters and buffers: after load_state_dict, an
    optimizer step or an in-place edit of a running statistic the fold and the weight packs are recomputed outside any graph into the
    same buffers, so no graph is captured again (num_captures counts the captures)."""

    def __init__(self, model, dtype=None, graph=True, max_graphs=4):
        if isinstance(model, (nn.parallel.DistributedDataParallel, nn.DataParallel)):
            model = model.module
        if not hasattr(model, "compute_dtype") or not hasattr(model, "_enter"):
            raise TypeError("Predictor: expects an egm_unet_amd GRFBUNet or UNet")
        params = list(model.parameters())
        if not params or not all(p.is_cuda for p in params):
            raise RuntimeError("egm_unet_amd models run on the GPU only: move the model to cuda before building a Predictor")
        require_gpu()
        self.model = model
        self.dtype = model.compute_dtype if dtype is None else dtype
        dtype_code(self.dtype)
        self.graph = bool(graph)
        self._replay = ReplayCache("infer", max_graphs)
        self._graphs = self._replay.entries          # (N, H, W, dtype) -> {"tag", "graph", "src", "out"}
        self._tensors = params + list(model.buffers())
        self._stamp = None
        dev = params[0].device
        # folded packs: forward operand pack of w*s and the fp32 bias, per conv holder with a BatchNorm behind it
        pairs = _conv_bn_pairs(model)
        self._pairs = pairs
        self._packs = {}
        cmax = 8
        for conv, bn in pairs:
            Cout, Cin_g, KH, KW = conv.weight.shape
            Cin = Cin_g * conv.groups
            self._packs[conv] = (torch.empty((KH * KW, ops.pad8(Cout), ops.pad8(Cin)), dtype=self.dtype, device=dev),
                                 torch.zeros(ops.pad8(Cout), dtype=torch.float32, device=dev))
            cmax = max(cmax, ops.pad8(Cout), ops.pad8(Cin))
        ident = torch.zeros((4, max(cmax, 1024)), dtype=torch.float32, device=dev)
        ident[0].fill_(1.0)
        ident[3].fill_(1.0)
        self._packs["identity"] = ident
        self._fold_table = ops.DeviceTable()
        # the model's prepack for the convolutions WITHOUT a BatchNorm behind them, in buffers of this predictor (a graph reads them)
        folded = set(id(c) for c, _ in pairs)
        convs = [m for m in model.modules() if isinstance(m, nn.Conv2d) and not getattr(m, "_egm_no_prepack", False) and m.weight.dim() == 4
                 and id(m) not in folded]
        bufs = []
        for m in convs:
            Cout, Cin_g, KH, KW = m.weight.shape
            Cin = Cin_g * m.groups
            bufs.append((torch.empty((KH * KW, ops.pad8(Cout), ops.pad8(Cin)), dtype=self.dtype, device=dev),
                         torch.empty((KH * KW, ops.pad8(Cin), ops.pad8(Cout)), dtype=self.dtype, device=dev)))
        self._prepack = {"dtype": self.dtype, "convs": convs, "bufs": bufs, "table": ops.DeviceTable(), "stamp": None}
        self._holder = types.SimpleNamespace(_egm_prepack=self._prepack)

    # ---- weights
    def _refresh(self):
        """Refold and repack when any parameter or buffer changed (outside any graph; the same buffers are rewritten)."""
        stamp = (ops._weight_generation[0], tuple((t._version, t.data_ptr()) for t in self._tensors))
        if stamp != self._stamp:
            L = lib()
            chunk = L.cdll.egm_conv_fold_chunk()
            blob, chunks, keep = bytearray(), 0, []
            for conv, bn in self._pairs:
                wf, bias = self._packs[conv]
                Cout, Cin_g, KH, KW = conv.weight.shape
                Cin = Cin_g * conv.groups
                w = conv.weight.detach()
                if not w.is_contiguous():
                    w = w.contiguous()
                    keep.append(w)
                if bn.running_mean is None or bn.running_var is None:
                    raise RuntimeError("Predictor: BatchNorm layers without running statistics cannot be folded")
                dp = lambda t: 0 if t is None else t.detach().data_ptr()
                blob += _FOLD_ENTRY.pack(w.data_ptr(), dp(conv.bias), dp(bn.weight), dp(bn.bias), dp(bn.running_mean), dp(bn.running_var),
                                         wf.data_ptr(), bias.data_ptr(), float(bn.eps), Cout, Cin, ops.pad8(Cout), ops.pad8(Cin), KH, KW,
                                         conv.groups, chunks, 0)
                chunks += (KH * KW * ops.pad8(Cout) * ops.pad8(Cin) + chunk - 1) // chunk
            if self._pairs:
                table = self._fold_table.get(bytes(blob), wf.device)
                L.call("egm_conv_fold_pack_multi", dtype_code(self.dtype), ptr(table), len(self._pairs), chunks, stream())
            ops.prepack_model(self._holder, self.dtype)
            self._stamp = stamp
        ops.claim_prepack(self._prepack)

    def refresh(self):
        """Bring the folded packs up to date with the model's parameters and buffers now (what every call does first).  For callers that
        run this predictor's forward inside a graph of their own: call it before each replay, outside the graph."""
        with torch.no_grad():
            self._refresh()

    # ---- forward
    def _forward(self, x):
        """One folded eval forward of the model (eager, or being captured): training flags off, this predictor's packs swapped in."""
        m = self.model
        flags = [(mod, mod.training) for mod in m.modules()]
        saved = (m.__dict__.get("_egm_prepack", _MISSING), m.__dict__.get("compute_dtype", _MISSING))
        try:
            for mod, _ in flags:
                mod.training = False
            m._egm_prepack = self._prepack
            m.compute_dtype = self.dtype
            with ops.folded_inference(self._packs):
                return m(x)["out"]
        finally:
            for mod, t in flags:
                mod.training = t
            for name, v in zip(("_egm_prepack", "compute_dtype"), saved):
                if v is _MISSING:
                    m.__dict__.pop(name, None)
                else:
                    setattr(m, name, v)

    def __call__(self, x, clone=False):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("egm_unet_amd models run on the GPU only: move the input (and the model) to cuda")
        if x.dim() != 4:
            raise RuntimeError(f"expected input [N,C,H,W], got {tuple(x.shape)}")
        with torch.no_grad():
            self._refresh()
            if not self.graph:
                out = self._forward(x)
            else:
                out = self._replay((x.shape[0], x.shape[2], x.shape[3], self.dtype), x, self._forward)
        return {"out": out.clone() if clone else out}

    max_graphs = property(lambda self: self._replay.max_graphs)
    num_captures = property(lambda self: self._replay.num_captures)

    def reset_graphs(self):
        """Forget every captured graph (the next call at each shape warms up again)."""
        self._replay.reset()

    def predict_mask(self, x, lut=None):
        """-> uint8 [N, H, W] class ids (argmax over the logits, ties to the lowest class), mapped through lut when given (a sequence
        or tensor of <= 256 values, e.g. predict.py's color_map {0: 0, 1: 255} as [0, 255])."""
        logits = self(x)["out"]
        N, C, H, W = logits.shape
        lt = lut256(lut, C, logits.device, "predict_mask: lut")
        mask = torch.empty((N, H, W), dtype=torch.uint8, device=logits.device)
        lib().call("egm_argmax_u8", ptr(logits), ptr(lt), ptr(mask), N, C, H, W, stream())
        return mask


def evaluate(model, data_loader, device, num_classes, predictor=None):
    """train_utils.evaluate through a Predictor: -> (ConfusionMatrix, mean foreground Dice).  model.training is left as it is."""
    from .train_utils import distributed_utils as utils
    pred = Predictor(model) if predictor is None else predictor
    confmat = utils.ConfusionMatrix(num_classes)
    dice = utils.DiceCoefficient(num_classes=num_classes, ignore_index=255)
    metric_logger = utils.MetricLogger(delimiter="  ")
    with torch.no_grad():
        for image, target in metric_logger.log_every(data_loader, 100, "Test:"):
            image, target = image.to(device), target.to(device)
            output = pred(image)["out"]                    # consumed on the stream before the next replay overwrites it
            confmat.update_from_logits(target, output)
            dice.update(output, target)
        confmat.reduce_from_all_processes()
        dice.reduce_from_all_processes()
    return confmat, dice.value.item()
