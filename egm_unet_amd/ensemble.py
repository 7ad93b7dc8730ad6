"""CLIPSeg (+) UNet logit ensemble: fused prediction and the validation alpha grid search
(predict_CLIPseg.py:501-525, eval_CLIPseg.py:656-723; best_alpha.txt holds the reference's result, 10.0), and the whole per-image
pipeline of predict_CLIPseg.py -- decoded uint8 photo on the device in, uint8 mask at the photo's size out -- as one replayed graph:

    ens = EnsemblePredictor(unet, clipseg, ["background", "crack"], alpha=0.5)
    mask = ens(img_u8)                      # uint8 [H0, W0] on the device; img_u8 is [H0, W0, 3] uint8 cuda
    clip_l, unet_l = ens.logits(img_u8)     # what predict_CLIPseg.py / eval_CLIPseg.py append to their lists
    best, best_miou, mious = ens.search_alpha(images, labels)

and the same for photos in batches (B photos of one size per replayed graph, both models at batch B):

    masks = ens.predict_batch(imgs_u8)      # uint8 [B, H0, W0]; imgs_u8 is [B, H0, W0, 3] uint8 cuda, or a list of B photos
    masks = ens.predict_many(photos, 8)     # photos of any sizes -> their masks in input order, grouped by plan_batches
"""
import collections
import itertools

import numpy as np
import torch

from . import data, ops
from .clip import ops as clip_ops
from ._lib import lib, ptr, require_gpu, stream
from .infer import Predictor

_serial = itertools.count()


def fuse_predict(clip_logits, unet_logits, alpha, return_fused=False):
    """clip_logits [N,C,hc,wc] (e.g. 352x352), unet_logits [N,C,H,W] -> argmax mask int64 [N,H,W] (and fused logits)."""
    require_gpu()
    c, u = clip_logits.contiguous().float(), unet_logits.contiguous().float()
    N, C, hc, wc = c.shape
    _, _, H, W = u.shape
    pred = torch.empty((N, H, W), dtype=torch.int64, device=u.device)
    fused = torch.empty((N, C, H, W), dtype=torch.float32, device=u.device) if return_fused else None
    lib().call("egm_ensemble_fuse", ptr(c), ptr(u), float(alpha), N, C, hc, wc, H, W, ptr(pred), ptr(fused), stream())
    return (pred, fused) if return_fused else pred


def search_best_alpha(clip_logits_list, unet_logits_list, labels_list, search_scale=(0.1, 10.0), search_step=100, num_classes=2):
    """-> (best_alpha, best_miou, miou per alpha).  Global confusion matrix over all images per alpha; first maximum wins,
    like the reference's strict `>` update."""
    require_gpu()
    alphas = np.linspace(search_scale[0], search_scale[1], search_step)
    dev = unet_logits_list[0].device
    a_dev = torch.tensor(alphas, dtype=torch.float32, device=dev)
    hist = torch.zeros(search_step * num_classes * num_classes, dtype=torch.int64, device=dev)
    for c, u, t in zip(clip_logits_list, unet_logits_list, labels_list):
        c, u = c.contiguous().float().to(dev), u.contiguous().float().to(dev)
        t = torch.as_tensor(t).to(dev).to(torch.int64).reshape(u.shape[0], u.shape[2], u.shape[3]).contiguous()
        lib().call("egm_ensemble_alpha_hist", ptr(c), ptr(u), ptr(t), ptr(a_dev), search_step, u.shape[0], u.shape[1], c.shape[2], c.shape[3],
                   u.shape[2], u.shape[3], ptr(hist), stream())
    miou = torch.empty(search_step, dtype=torch.float32, device=dev)
    lib().call("egm_ensemble_miou", ptr(hist), search_step, num_classes, ptr(miou), stream())
    m = miou.cpu().numpy()
    best, best_miou = 0.0, 0.0
    for a, v in zip(alphas, m):
        if v > best_miou:
            best_miou, best = float(v), float(a)
    return best, best_miou, m


def _lut256(lut, C, device):
    if lut is None:
        return None
    lt = torch.as_tensor(lut).to(torch.uint8).flatten()
    if lt.numel() < C or lt.numel() > 256:
        raise ValueError(f"lut must have between {C} and 256 entries, got {lt.numel()}")
    return torch.cat([lt.cpu(), torch.zeros(256 - lt.numel(), dtype=torch.uint8)]).to(device)


def fuse_mask(clip_logits, unet_logits, alpha, out_size, lut=None, out=None):
    """predict_CLIPseg.py:501-534 behind the models: fused = bilinear(clip_logits -> UNet size) + alpha * unet_logits -> argmax ->
    cv2.resize(pred, (W0, H0), interpolation=cv2.INTER_NEAREST) -> colour map, as one kernel -> uint8 [N, H0, W0].
    Bit-identical to lut[fuse_predict(...)][:, yidx][:, :, xidx] with the tables of data.cv_nearest_table (OpenCV's rule restated from
    its source, not checked against a cv2 build).  alpha: a number or a one-element fp32 CUDA tensor (read on the device, so a captured
    graph follows its value); lut: None (class ids) or a sequence / tensor of C..256 values, e.g. (0, 255); a 256-entry uint8 CUDA
    tensor is used as it is."""
    require_gpu()
    c, u = clip_logits.contiguous().float(), unet_logits.contiguous().float()
    N, C, hc, wc = c.shape
    if u.dim() != 4 or u.shape[0] != N or u.shape[1] != C:
        raise ValueError(f"fuse_mask: clip_logits {tuple(c.shape)} and unet_logits {tuple(u.shape)} must agree in N and C")
    H, W = u.shape[2:]
    H0, W0 = int(out_size[0]), int(out_size[1])
    if not (isinstance(alpha, torch.Tensor) and alpha.is_cuda and alpha.dtype == torch.float32 and alpha.numel() == 1):
        alpha = torch.full((1,), float(alpha), dtype=torch.float32, device=u.device)
    if not (isinstance(lut, torch.Tensor) and lut.is_cuda and lut.dtype == torch.uint8 and lut.numel() == 256):
        lut = _lut256(lut, C, u.device)
    if out is None:
        out = torch.empty((N, H0, W0), dtype=torch.uint8, device=u.device)
    lib().call("egm_ensemble_mask_u8", ptr(c), ptr(u), ptr(alpha), N, C, hc, wc, H, W, ptr(data.cv_nearest_table(H, H0, u.device)),
               ptr(data.cv_nearest_table(W, W0, u.device)), ptr(lut), ptr(out), H0, W0, stream())
    return out


def plan_batches(sizes, batch_size):
    """Group photos by size for batched inference: sizes is a sequence of (H0, W0), one per photo -> a list of
    (size, input indices, pad count), one per batch.  A batch holds photos of one size only, in input order; sizes come in the order
    of their first photo; every input index appears exactly once; a batch has len(indices) + pad == batch_size, with pad > 0 only in
    a size's last batch (the caller repeats that batch's last photo pad times, so every batch of a size has the same shape).
    Pure host code."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"plan_batches: batch_size must be at least 1, got {batch_size}")
    groups = collections.OrderedDict()
    for i, size in enumerate(sizes):
        groups.setdefault((int(size[0]), int(size[1])), []).append(i)
    plan = []
    for size, idx in groups.items():
        for k in range(0, len(idx), batch_size):
            part = idx[k:k + batch_size]
            plan.append((size, part, batch_size - len(part)))
    return plan


class EnsemblePredictor:
    """predict_CLIPseg.py per image (:438-534) as one object: a decoded uint8 photo [H0, W0, 3] already on the device goes in, the uint8
    mask [H0, W0] comes out.

      UNet branch    data.resize_bilinear(img, base_size) (Pillow-exact, transforms.Resize(base_size) of the PIL image) -> data.augment
                     (ToTensor, Normalize(unet_mean, unet_std)) -> the folded forward of an infer.Predictor
      CLIPSeg branch data.clip_preprocess (ToTensor, Normalize(clip_mean, clip_std), Resize((clip_size, clip_size)) of the tensor) ->
                     the model's multi-prompt decoder on one backbone pass, in the model's compute dtype
      tail           fuse_mask: clip + alpha * unet -> argmax -> nearest resize to the photo's size -> lut

    prompts: K strings or a [K, 512] tensor, K = the UNet's class count; the conditional vectors are computed once.  dtype: the UNet's
    activation dtype (None = unet.compute_dtype).  graph=True: the first call at a photo size runs eagerly (it fills the table, positional
    embedding and cast-weight caches), the second captures everything from the static input buffer to the static mask into one graph on one
    stream (no forked branches), later calls copy the image in and replay; at most max_graphs sizes are kept, least recently used first
    out.  The returned mask (and logits) of a replay are the graph's buffers: the next call at that size overwrites them; clone=True keeps
    them.  Nothing in a call waits for the device.

    alpha lives in a device scalar: `ens.alpha = 2.0` is followed by the captured graphs without a new capture.  Changes of the UNet's
    weights are folded again before each replay into the same buffers (Predictor.refresh); a change of the CLIPSeg model's parameters
    or compute dtype (stamp of _version, data_ptr and the generation counters that raw-pointer optimizers such as clip.train_ops.AdamW
    bump) drops the captured graphs and recomputes the conditionals, because the cast-weight
    caches move to new buffers then.

    predict_batch / logits_batch / predict_many run B photos of one size through the same pipeline at batch B (_run_batch) under the
    same protocol, keyed by (B, H0, W0): batched and per-image entries share max_graphs and its eviction order, alpha, the lut, the
    conditionals and every drop rule above.  Results are per image: nothing in either model reduces over the batch."""

    def __init__(self, unet, clipseg, prompts, alpha=0.5, unet_mean=(0.709, 0.381, 0.224), unet_std=(0.127, 0.079, 0.043), base_size=565,
                 clip_size=352, clip_antialias=True, lut=(0, 255), dtype=None, graph=True, max_graphs=4, clip_mean=(0.485, 0.456, 0.406),
                 clip_std=(0.229, 0.224, 0.225)):
        require_gpu()
        self._unet = Predictor(unet, dtype=dtype, graph=False)
        self.clipseg = clipseg
        dev = next(self._unet.model.parameters()).device
        self.device = dev
        self.num_classes = int(self._unet.model.num_classes)
        self._prompts = prompts if isinstance(prompts, torch.Tensor) else list([prompts] if isinstance(prompts, str) else prompts)
        K = self._prompts.shape[0] if isinstance(self._prompts, torch.Tensor) else len(self._prompts)
        if K != self.num_classes:
            raise ValueError(f"EnsemblePredictor: {K} prompts for a UNet with {self.num_classes} classes (one prompt per class)")
        self.unet_mean, self.unet_std, self.clip_mean, self.clip_std = tuple(unet_mean), tuple(unet_std), tuple(clip_mean), tuple(clip_std)
        self.base_size = int(base_size)
        self.clip_size = (clip_size, clip_size) if isinstance(clip_size, int) else (int(clip_size[0]), int(clip_size[1]))
        self.clip_antialias = bool(clip_antialias)
        self._lut = _lut256(lut, self.num_classes, dev)
        self._alpha = torch.empty(1, dtype=torch.float32, device=dev)
        self._alpha_value = None
        self.alpha = alpha
        self.graph = bool(graph)
        self.max_graphs = max(1, int(max_graphs))
        self.num_captures = 0
        # (H0, W0) of a photo or (B, H0, W0) of a batch -> {"tag", "graph", "img", "out": (mask, clip logits, unet logits)}
        self._graphs = collections.OrderedDict()
        self._clip_tensors = list(clipseg.parameters()) + list(clipseg.buffers())
        self._clip_stamp = None
        self._condT = None

    # ---- alpha: a device scalar the fuse kernel reads
    @property
    def alpha(self):
        return self._alpha_value

    @alpha.setter
    def alpha(self, v):
        self._alpha_value = float(v)
        self._alpha.fill_(self._alpha_value)               # a fill kernel with the value as its argument: no host wait

    # ---- weights
    def _refresh(self):
        self._unet.refresh()
        cs = self.clipseg
        # (the two generation counters: optimizers that write parameters through raw pointers bump them instead of _version, and
        # the cast-weight caches move to new buffers on either)
        stamp = (cs.compute_dtype, clip_ops._cast_generation[0], ops._weight_generation[0],
                 tuple((t._version, t.data_ptr()) for t in self._clip_tensors))
        if stamp != self._clip_stamp:
            self.reset_graphs()
            self._condT = cs._cond_in_dtype(cs._multi_cond(self._prompts))
            self._clip_stamp = stamp

    # ---- the pipeline (eager, or being captured)
    def _run(self, img):
        H0, W0, _ = img.shape
        r = data.resize_bilinear(img, self.base_size)
        x, _ = data.augment(r, None, False, False, 0, 0, r.shape[0], r.shape[1], self.unet_mean, self.unet_std)
        unet_l = self._unet(x.unsqueeze(0))["out"]
        xc = data.clip_preprocess(img, self.clip_size, self.clip_mean, self.clip_std, self.clip_antialias)
        out = self.clipseg._decode_multi(xc, self._condT)
        clip_l = out.view(1, self._condT.shape[0], out.shape[-2], out.shape[-1])
        mask = fuse_mask(clip_l, unet_l, self._alpha, (H0, W0), self._lut)
        return mask[0], clip_l, unet_l

    def _run_batch(self, imgs):
        """_run for B photos of one size [B, H0, W0, 3]: both preprocessing chains in launches that cover the whole batch, both models
        at batch B, the tail at N = B -> (masks [B, H0, W0], clip logits [B, K, ch, cw], unet logits [B, C, h, w])."""
        B, H0, W0, _ = imgs.shape
        x = data.unet_preprocess_batch(imgs, self.base_size, self.unet_mean, self.unet_std)
        unet_l = self._unet(x)["out"]
        xc = data.clip_preprocess_batch(imgs, self.clip_size, self.clip_mean, self.clip_std, self.clip_antialias)
        out = self.clipseg._decode_multi(xc, self._condT)
        clip_l = out.view(B, self._condT.shape[0], out.shape[-2], out.shape[-1])
        mask = fuse_mask(clip_l, unet_l, self._alpha, (H0, W0), self._lut)
        return mask, clip_l, unet_l

    def _replayed(self, key, src, run):
        """The graph protocol of every entry: `run(src)` eagerly (graph=False), or per key the warm-up call, the capturing call and the
        replays.  key: (H0, W0) for one photo, (B, H0, W0) for a batch; both kinds share the table, its limit and its eviction order."""
        with torch.no_grad():
            self._refresh()
            if not self.graph:
                return run(src)
            ent = self._graphs.get(key)
            if ent is None:
                while len(self._graphs) >= self.max_graphs:
                    self._drop(next(iter(self._graphs)))
                ent = {"tag": ("ensemble", next(_serial)), "graph": None, "img": None, "out": None}
                try:
                    with ops.table_namespace(ent["tag"]):          # warm-up: tables, positional embedding, cast weights, allocator
                        out = run(src)
                except BaseException:
                    ops.drop_table_namespace(ent["tag"])
                    raise
                self._graphs[key] = ent                            # only a size that warmed up is captured by the next call
                return out
            self._graphs.move_to_end(key)
            if ent["graph"] is None:
                ent["img"] = src.detach().clone(memory_format=torch.contiguous_format)
                g = torch.cuda.CUDAGraph(keep_graph=True)
                with ops.table_namespace(ent["tag"]), torch.cuda.graph(g):
                    ent["out"] = run(ent["img"])
                g.instantiate()
                ent["graph"] = g
                self.num_captures += 1
            else:
                ent["img"].copy_(src)
            ent["graph"].replay()
            return ent["out"]

    def _call(self, img):
        img = data._check_u8(img, 3)
        if img.shape[2] != 3:
            raise RuntimeError("EnsemblePredictor: RGB images ([H0, W0, 3] uint8) expected")
        return self._replayed((img.shape[0], img.shape[1]), img, self._run)

    def _call_batch(self, imgs):
        if isinstance(imgs, (list, tuple)):
            if len(imgs) == 0:
                raise RuntimeError("EnsemblePredictor: an empty batch")
            imgs = torch.stack([data._check_u8(im, 3) for im in imgs])         # photos of one size, stacked on the device
        imgs = data._check_u8(imgs, 4)
        if imgs.shape[0] == 0 or imgs.shape[3] != 3:
            raise RuntimeError("EnsemblePredictor: a non-empty batch of RGB images ([B, H0, W0, 3] uint8, or a list of [H0, W0, 3]) expected")
        return self._replayed(tuple(imgs.shape[:3]), imgs, self._run_batch)

    def __call__(self, img_u8, clone=False):
        mask = self._call(img_u8)[0]
        return mask.clone() if clone else mask

    def logits(self, img_u8, clone=False):
        """-> (clip_logits [1, K, clip_h, clip_w], unet_logits [1, C, h, w]) fp32, the tensors predict_CLIPseg.py:497-499 and
        eval_CLIPseg.py collect per image."""
        _, c, u = self._call(img_u8)
        return (c.clone(), u.clone()) if clone else (c, u)

    def predict_batch(self, imgs_u8, clone=False):
        """B photos of one size, uint8 [B, H0, W0, 3] on the device (or a list of B [H0, W0, 3] tensors) -> uint8 masks [B, H0, W0];
        row b is what the per-image call computes for photo b, whatever else is in the batch.  The graph protocol of __call__, keyed
        by (B, H0, W0): warm-up, capture, replays; a replay returns the graph's buffer unless clone=True."""
        mask = self._call_batch(imgs_u8)[0]
        return mask.clone() if clone else mask

    def logits_batch(self, imgs_u8, clone=False):
        """-> (clip_logits [B, K, clip_h, clip_w], unet_logits [B, C, h, w]) fp32 of a batch as for predict_batch."""
        _, c, u = self._call_batch(imgs_u8)
        return (c.clone(), u.clone()) if clone else (c, u)

    def predict_many(self, photos, batch_size=8):
        """A folder's worth of photos: a sequence of [H0, W0, 3] uint8 device tensors of any sizes -> their uint8 masks [H0, W0] in
        input order, each a tensor of its own.  Photos are grouped by size (plan_batches) and go through predict_batch in groups of
        batch_size; a short last group is filled up with its last photo, so every batch of a size replays the same graph."""
        photos = list(photos)
        masks = [None] * len(photos)
        for _, idx, pad in plan_batches([tuple(p.shape[:2]) for p in photos], batch_size):
            out = self.predict_batch([photos[i] for i in idx] + [photos[idx[-1]]] * pad)
            for row, i in enumerate(idx):
                masks[i] = out[row].clone()
        return masks

    def _drop(self, key):
        ent = self._graphs.pop(key)
        ent["graph"] = None
        ops.drop_table_namespace(ent["tag"])

    def reset_graphs(self):
        """Forget every captured graph (the next call at each photo size warms up again)."""
        for key in list(self._graphs):
            self._drop(key)

    def captured_graph(self, size):
        """The captured torch.cuda.CUDAGraph of photo size (H0, W0), or of the batch (B, H0, W0), or None (for tools that count its
        kernel nodes)."""
        ent = self._graphs.get(tuple(int(v) for v in size))
        return None if ent is None else ent["graph"]

    def search_alpha(self, images, labels, search_scale=(0.1, 10.0), search_step=100, batch_size=None):
        """eval_CLIPseg.py:656-723 over this pipeline: the logits of every image go through the alpha grid search (one confusion matrix per
        alpha over all images, first maximum wins); labels at the UNet's size [h, w].  batch_size=None collects the logits image by
        image; a number collects them through logits_batch over plan_batches (the grid search still gets them per image, in input
        order).  Sets self.alpha. -> (best, best_miou, miou per alpha)"""
        images = list(images)
        cl, ul = [None] * len(images), [None] * len(images)
        if batch_size is None:
            for i, img in enumerate(images):
                cl[i], ul[i] = self.logits(img, clone=True)
        else:
            for _, idx, pad in plan_batches([tuple(im.shape[:2]) for im in images], batch_size):
                c, u = self.logits_batch([images[i] for i in idx] + [images[idx[-1]]] * pad)
                for row, i in enumerate(idx):
                    cl[i], ul[i] = c[row:row + 1].clone(), u[row:row + 1].clone()
        best, best_miou, m = search_best_alpha(cl, ul, labels, search_scale, search_step, self.num_classes)
        self.alpha = best
        return best, best_miou, m
