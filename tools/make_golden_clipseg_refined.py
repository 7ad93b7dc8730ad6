#!/usr/bin/env python3
"""Generate tests/golden/clipseg_refined.npz + clipseg_refined_manifest.json by running the REFERENCE CLIPSeg with
complex_trans_conv=True (the rd64-uni-refined configuration, experiments/phrasecut.yaml:74) on CPU.

Build container only (needs the reference checkout, path in REF).  Modelled on tools/make_golden_clip.py: the same inert stand-ins for
packages the reference imports but never reaches, the backbone and decoder weights of oracle.clip_ref (seed 0) through the
reference's own loader, the same inputs (tests/golden/clipseg_fwd.npz: images and conditional vectors).  Only the six tensors of the
refinement head (trans_conv.{0,2,4}.{weight,bias}) are new; they come from a seeded generator here and are stored in the npz.
Written: the head weights, the head's input grid (forward pre-hook on trans_conv) and the subsampled / cropped mask logits at
352^2 and 224^2, and one decoder training step (BCE with logits): loss, gradient norms and probes of every decoder parameter.
Only data is written; no reference source is copied.  Re-run:  python tools/make_golden_clipseg_refined.py
"""
import json
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
from make_golden_clip import stub_modules  # noqa: E402
from oracle import clip_ref as C  # noqa: E402

RD = 64
HEAD_SEED = 21
TARGET_SEED = 11


def head_state(rd=RD, seed=HEAD_SEED):
    """trans_conv.{0,2,4}.{weight,bias}: fan-in scaled normals, so that both ReLUs stay partly active."""
    g = torch.Generator().manual_seed(seed)
    return {"trans_conv.0.weight": torch.randn(rd, rd, 3, 3, generator=g) / (9 * rd) ** 0.5,
            "trans_conv.0.bias": 0.05 * torch.randn(rd, generator=g),
            "trans_conv.2.weight": torch.randn(rd, rd // 2, 4, 4, generator=g) / rd ** 0.5,
            "trans_conv.2.bias": 0.05 * torch.randn(rd // 2, generator=g),
            "trans_conv.4.weight": torch.randn(rd // 2, 1, 4, 4, generator=g) / (rd // 2) ** 0.5,
            "trans_conv.4.bias": 0.05 * torch.randn(1, generator=g)}


def main():
    fx = dict(np.load(os.path.join(OUT, "clipseg_fwd.npz")))
    stub_modules()
    sys.path.insert(0, REF)
    scratch = tempfile.mkdtemp(prefix="clipgold_refined_")
    os.makedirs(os.path.join(scratch, "weights"))
    torch.save({k: v.clone() for k, v in C.make_clip_state(seed=0).items()}, os.path.join(scratch, "weights", "longclip-B.pt"))
    os.chdir(scratch)                                     # models/clipseg.py:147 loads the relative path weights/longclip-B.pt
    from models.clipseg import CLIPDensePredT

    torch.manual_seed(0)
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=RD, complex_trans_conv=True)
    dec = {k: v for k, v in C.make_decoder_state(seed=0, reduce_dim=RD).items() if not k.startswith("trans_conv.")}
    head = head_state()
    res = m.load_state_dict({**dec, **head}, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.startswith(("clip_model.", "model.")) for k in res.missing_keys), [k for k in res.missing_keys if not k.startswith(("clip_model.", "model."))]
    json.dump({k: list(v.shape) for k, v in m.state_dict().items()}, open(os.path.join(OUT, "clipseg_refined_manifest.json"), "w"))
    m.eval()

    grids = []
    hook = m.trans_conv.register_forward_pre_hook(lambda mod, inp: grids.append(inp[0].detach().clone()))
    img = torch.from_numpy(fx["img"].astype(np.float32))
    img224 = torch.from_numpy(fx["img224"].astype(np.float32))
    cond = torch.from_numpy(fx["cond"])
    with torch.no_grad():
        out = m(img, cond)[0]
        out224 = m(img224, cond[:1])[0]
    hook.remove()
    assert out.shape == (2, 1, 352, 352) and out224.shape == (1, 1, 224, 224)
    d = {"head/" + k: v.numpy() for k, v in head.items()}
    d.update({"grid": grids[0].numpy(), "grid224": grids[1].numpy(),
              "out": out[:, :, ::4, ::4].numpy(), "out_crop": out[:, :, 100:164, 100:164].numpy(),
              "out224": out224[:, :, ::4, ::4].numpy(), "out224_crop": out224[:, :, 64:128, 64:128].numpy()})

    # ---- decoder training step (eval mode = no dropout, autograd on), as clipseg_train.npz
    target = (torch.rand(2, 1, 352, 352, generator=torch.Generator().manual_seed(TARGET_SEED)) < 0.3).float()
    for p_ in m.parameters():
        p_.grad = None
    loss = torch.nn.functional.binary_cross_entropy_with_logits(m(img, cond)[0], target)
    loss.backward()
    d.update({"loss": loss.detach().numpy(), "target_seed": np.array(TARGET_SEED)})
    n = 0
    for name, p_ in m.named_parameters():
        if p_.grad is None:
            continue
        gflat = p_.grad.flatten()
        d["norm/" + name] = gflat.norm().numpy()
        d["probe/" + name] = gflat[:: max(1, gflat.numel() // 257)][:257].numpy()
        n += 1
    np.savez_compressed(os.path.join(OUT, "clipseg_refined.npz"), **d)
    print("refined: out", tuple(out.shape), float(out.mean()), float(out.std()), "positive", float((out > 0).float().mean()),
          "| loss", float(loss), "params with grad", n)


if __name__ == "__main__":
    main()
