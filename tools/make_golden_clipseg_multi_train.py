#!/usr/bin/env python3
"""Generate tests/golden/clipseg_multi_train.npz by running the REFERENCE on CPU: one decoder training step of the repeat form, K = 3
prompts on each of B = 2 images (the image fed once per prompt through CLIPDensePredT.forward, models/clipseg.py:436-496), BCE-with-logits
loss over the [B, K, 352, 352] logits, parameter gradients.  It is what CLIPDenseBase.forward_multi_train has to reproduce.

Build container only (needs the reference checkout, path in REF).  Modelled on tools/make_golden_clip.py: the same inert stand-ins
(stub_modules), the backbone of oracle.clip_ref (seed 0) through the reference's own loader, the decoder of
oracle.clip_ref.make_decoder_state (seed 0), the images of tests/golden/clipseg_fwd.npz.  The reference runs in eval mode with autograd on
(no dropout), as for clipseg_train.npz.  Written, in the layout of clipseg_train.npz: the loss, the conditionals, the target's seed and,
per parameter with a gradient, its norm and a 257-element probe.  Only data is written; no reference source is copied.
Re-run:  python tools/make_golden_clipseg_multi_train.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_clip import PROMPTS, stub_modules  # noqa: E402
from oracle import clip_ref as C  # noqa: E402

MULTI_PROMPTS = [PROMPTS[0], PROMPTS[3], PROMPTS[4]]
CLIP_SEED, DECODER_SEED, TARGET_SEED = 0, 0, 13


def main():
    fx = dict(np.load(os.path.join(OUT, "clipseg_fwd.npz")))
    stub_modules()
    sys.path.insert(0, REF)
    scratch = tempfile.mkdtemp(prefix="clipgold_multi_train_")
    os.makedirs(os.path.join(scratch, "weights"))
    torch.save({k: v.clone() for k, v in C.make_clip_state(seed=CLIP_SEED).items()}, os.path.join(scratch, "weights", "longclip-B.pt"))
    os.chdir(scratch)                                     # models/clipseg.py:147 loads the relative path weights/longclip-B.pt
    from models.clipseg import CLIPDensePredT

    torch.manual_seed(0)
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64)
    res = m.load_state_dict(C.make_decoder_state(seed=DECODER_SEED), strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    m.eval()                                              # eval mode with autograd on: the reference's dropout switched off

    img = torch.from_numpy(fx["img"].astype(np.float32))
    B, K = img.shape[0], len(MULTI_PROMPTS)
    with torch.no_grad():
        cond = m.compute_conditional(MULTI_PROMPTS)
    for p_ in m.parameters():
        p_.grad = None
    out = torch.stack([m(img[b:b + 1].repeat(K, 1, 1, 1), cond)[0][:, 0] for b in range(B)])          # [B, K, 352, 352]
    target = (torch.rand(B, K, 352, 352, generator=torch.Generator().manual_seed(TARGET_SEED)) < 0.3).float()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out, target)
    loss.backward()
    tr = {"loss": loss.detach().numpy(), "cond": cond.numpy(), "target_seed": np.array(TARGET_SEED)}
    for name, p_ in m.named_parameters():
        if p_.grad is None:
            continue
        gflat = p_.grad.flatten()
        tr["norm/" + name] = gflat.norm().numpy()
        tr["probe/" + name] = gflat[:: max(1, gflat.numel() // 257)][:257].numpy()
    path = os.path.join(OUT, "clipseg_multi_train.npz")
    np.savez_compressed(path, **tr)
    print("multi-prompt train fixture: loss", float(loss.detach()), "params with grad", sum(1 for k in tr if k.startswith("norm/")),
          "| npz bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
