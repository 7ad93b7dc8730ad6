#!/usr/bin/env python3
"""Generate tests/golden/clipseg_baseline.npz + clipseg_baseline_manifest.json by running the REFERENCE CLIPDenseBaseline
(models/clipseg.py:529-590; experiments/phrasecut.yaml:81 baseline3-vit16-phrasecut) on CPU.

Build container only (needs the reference checkout, path in REF).  Modelled on tools/make_golden_clipseg_refined.py: the same inert
stand-ins for packages the reference imports but never reaches, the backbone of oracle.clip_ref (seed 0) through the reference's own
loader, the same inputs (tests/golden/clipseg_fwd.npz).  film_mul / film_add / reduce come from oracle.clip_ref.make_decoder_state
(seed 0); reduce2 and trans_conv from a seeded generator here, scaled so that the ReLU stays partly active, and stored in the npz.  Written: subsampled / cropped mask logits at 352^2 and 224^2, the 224^2 layer-9 activation, visual_q
(return_features=True), and one decoder training step (BCE with logits): loss, gradient norms and probes of every decoder parameter.
Only data is written; no reference source is copied.  Re-run:  python tools/make_golden_clipseg_baseline.py
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

RD, RD2 = 64, 64
HEAD_SEED = 23
TARGET_SEED = 11
DECODER_KEYS = ("film_mul.", "film_add.", "reduce.", "reduce2.", "trans_conv.")


def head_state(rd=RD, rd2=RD2, seed=HEAD_SEED):
    """reduce2.{0,2} and trans_conv: fan-in scaled normals, biases small, so that the ReLU stays partly active."""
    g = torch.Generator().manual_seed(seed)
    return {"reduce2.0.weight": torch.randn(rd2, rd, generator=g) / rd ** 0.5,
            "reduce2.0.bias": 0.05 * torch.randn(rd2, generator=g),
            "reduce2.2.weight": torch.randn(rd, rd2, generator=g) / rd2 ** 0.5,
            "reduce2.2.bias": 0.05 * torch.randn(rd, generator=g),
            "trans_conv.weight": torch.randn(rd, 1, 16, 16, generator=g) / rd ** 0.5,
            "trans_conv.bias": 0.05 * torch.randn(1, generator=g)}


def main():
    fx = dict(np.load(os.path.join(OUT, "clipseg_fwd.npz")))
    stub_modules()
    sys.path.insert(0, REF)
    scratch = tempfile.mkdtemp(prefix="clipgold_baseline_")
    os.makedirs(os.path.join(scratch, "weights"))
    torch.save({k: v.clone() for k, v in C.make_clip_state(seed=0).items()}, os.path.join(scratch, "weights", "longclip-B.pt"))
    os.chdir(scratch)                                     # models/clipseg.py:147 loads the relative path weights/longclip-B.pt
    from models.clipseg import CLIPDenseBaseline

    torch.manual_seed(0)
    m = CLIPDenseBaseline(version="ViT-B/16", reduce_dim=RD, reduce2_dim=RD2)
    dec = {k: v for k, v in C.make_decoder_state(seed=0, reduce_dim=RD).items() if k.startswith(("film_mul.", "film_add.", "reduce."))}
    dec.update(head_state())
    res = m.load_state_dict(dec, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.startswith(("clip_model.", "model.")) for k in res.missing_keys), [k for k in res.missing_keys if not k.startswith(("clip_model.", "model."))]
    json.dump({k: list(v.shape) for k, v in m.state_dict().items()}, open(os.path.join(OUT, "clipseg_baseline_manifest.json"), "w"))
    m.eval()

    img = torch.from_numpy(fx["img"].astype(np.float32))
    img224 = torch.from_numpy(fx["img224"].astype(np.float32))
    cond = torch.from_numpy(fx["cond"])
    with torch.no_grad():
        out, visual_q, _, acts = m(img, cond, return_features=True)
        out224, _, _, acts224 = m(img224, cond[:1], return_features=True)
    assert out.shape == (2, 1, 352, 352) and out224.shape == (1, 1, 224, 224)
    d = {"head/" + k: v.numpy() for k, v in head_state().items()}      # film_* / reduce: make_decoder_state(seed=0), not stored
    d.update({"act224": acts224[0].permute(1, 0, 2).contiguous().numpy(),          # [1, 197, 768] batch-first, layer 9
              "visual_q": visual_q.numpy(),
              "out": out[:, :, ::4, ::4].numpy(), "out_crop": out[:, :, 100:164, 100:164].numpy(),
              "out224": out224[:, :, ::4, ::4].numpy(), "out224_crop": out224[:, :, 64:128, 64:128].numpy()})

    # ---- decoder training step (no dropout in this model), as clipseg_refined.npz
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
        assert name.startswith(DECODER_KEYS), name
        gflat = p_.grad.flatten()
        d["norm/" + name] = gflat.norm().numpy()
        d["probe/" + name] = gflat[:: max(1, gflat.numel() // 257)][:257].numpy()
        n += 1
    np.savez_compressed(os.path.join(OUT, "clipseg_baseline.npz"), **d)
    print("baseline: out", tuple(out.shape), float(out.mean()), float(out.std()), "positive", float((out > 0).float().mean()),
          "| loss", float(loss.detach()), "params with grad", n, "| state_dict keys", len(m.state_dict()))


if __name__ == "__main__":
    main()
