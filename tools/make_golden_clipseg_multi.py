#!/usr/bin/env python3
"""Generate tests/golden/clipseg_multi.npz + clipseg_multi_manifest.json by running the REFERENCE on CPU: the repeat form of its ensemble
scripts (predict_CLIPseg.py:495, eval_CLIPseg.py:879: the image repeated once per prompt) and its own CLIPSegMultiLabel
(models/clipseg.py:592-625).

Build container only (needs the reference checkout, path in REF).  Modelled on tools/make_golden_clipseg_baseline.py: the same inert
stand-ins (stub_modules), the backbone of oracle.clip_ref (seed 0) through the reference's own loader, the decoder of
oracle.clip_ref.make_decoder_state (seed 0), the inputs of tests/golden/clipseg_fwd.npz.  CLIPSegMultiLabel imports two modules its tree
does not ship; they get stand-ins here: third_party.JoEm.data_loader (VOC = 'background' + datasets/pascal_classes.json in id order,
get_seen_idx, get_unseen_idx) and general_utils.load_model (returns the reference CLIPDensePredT above).  With those, the reference's own
__init__ and forward run.  Written: the repeat-form logits for B = 2 images x K = 3 prompts (subsampled ::4 and a 64^2 crop), the
MultiLabel output for image 0 (subsampled ::8 and a 32^2 crop) with the per-class logits it was computed from (recorded inside the
reference's forward), the class list, prompts and seeds.  Only data is written; no reference source is copied.
Re-run:  python tools/make_golden_clipseg_multi.py
"""
import json
import os
import sys
import tempfile
import types

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
CLIP_SEED, DECODER_SEED = 0, 0


def main():
    fx = dict(np.load(os.path.join(OUT, "clipseg_fwd.npz")))
    with open(os.path.join(REF, "datasets", "pascal_classes.json")) as f:
        classes = ["background"] + [c["synonyms"][0] for c in sorted(json.load(f), key=lambda c: c["id"])]
    assert len(classes) == 21
    stub_modules()
    sys.path.insert(0, REF)
    scratch = tempfile.mkdtemp(prefix="clipgold_multi_")
    os.makedirs(os.path.join(scratch, "weights"))
    torch.save({k: v.clone() for k, v in C.make_clip_state(seed=CLIP_SEED).items()}, os.path.join(scratch, "weights", "longclip-B.pt"))
    os.chdir(scratch)                                     # models/clipseg.py:147 loads the relative path weights/longclip-B.pt
    from models.clipseg import CLIPDensePredT, CLIPSegMultiLabel

    torch.manual_seed(0)
    m = CLIPDensePredT(version="ViT-B/16", reduce_dim=64)
    res = m.load_state_dict(C.make_decoder_state(seed=DECODER_SEED), strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    m.eval()

    # stand-ins for the two modules CLIPSegMultiLabel.__init__ imports
    tp, joem, dl = types.ModuleType("third_party"), types.ModuleType("third_party.JoEm"), types.ModuleType("third_party.JoEm.data_loader")
    dl.VOC = list(classes)
    dl.get_seen_idx = lambda *a, **k: list(range(len(classes)))
    dl.get_unseen_idx = lambda *a, **k: []
    tp.JoEm, joem.data_loader = joem, dl
    gu = types.ModuleType("general_utils")
    gu.load_model = lambda name, strict=False: m
    sys.modules.update({"third_party": tp, "third_party.JoEm": joem, "third_party.JoEm.data_loader": dl, "general_utils": gu})

    img = torch.from_numpy(fx["img"].astype(np.float32))
    K = len(MULTI_PROMPTS)
    with torch.no_grad():
        rep = torch.stack([m(img[b:b + 1].repeat(K, 1, 1, 1), MULTI_PROMPTS)[0][:, 0] for b in range(img.shape[0])])      # [B, K, 352, 352]

        ml = CLIPSegMultiLabel("rd64-uni")
        assert ml.clipseg is m
        seen = []
        fwd = m.forward
        m.forward = lambda *a, **k: seen.append(fwd(*a, **k)) or seen[-1]             # record the per-class logits inside the forward
        multi = ml(img[:1])                                                           # [1, 21, 352, 352]
        m.forward = fwd
    assert multi.shape == (1, 21, 352, 352) and len(seen) == 21
    logits = torch.stack([o[0][:, 0] for o in seen], 1)                               # [1, 21, 352, 352]
    d = {"rep": rep[:, :, ::4, ::4].numpy(), "rep_crop": rep[:, :, 100:164, 100:164].numpy(),
         "multi": multi[:, :, ::8, ::8].numpy(), "multi_crop": multi[:, :, 160:192, 160:192].numpy(),
         "multi_logits": logits[:, :, ::8, ::8].numpy(), "multi_logits_crop": logits[:, :, 160:192, 160:192].numpy(),
         "clip_seed": np.array(CLIP_SEED), "decoder_seed": np.array(DECODER_SEED)}
    np.savez_compressed(os.path.join(OUT, "clipseg_multi.npz"), **d)
    json.dump({"classes": classes, "prompts": MULTI_PROMPTS, "clip_seed": CLIP_SEED, "decoder_seed": DECODER_SEED,
               "images": "clipseg_fwd.npz img", "rep": "[B=2, K=3, 352, 352][..., ::4, ::4]", "rep_crop": "[..., 100:164, 100:164]",
               "multi": "image 0, [1, 21, 352, 352][..., ::8, ::8]", "multi_crop": "[..., 160:192, 160:192]"},
              open(os.path.join(OUT, "clipseg_multi_manifest.json"), "w"), indent=1)
    print("repeat form", tuple(rep.shape), float(rep.mean()), float(rep.std()), "| multilabel", tuple(multi.shape), float(multi.mean()),
          "| npz bytes", os.path.getsize(os.path.join(OUT, "clipseg_multi.npz")))


if __name__ == "__main__":
    main()
