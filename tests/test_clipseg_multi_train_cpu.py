"""CPU: the multi-prompt decoder-training fixture (tests/golden/clipseg_multi_train.npz, written by tools/make_golden_clipseg_multi_train.py
from the reference's repeat form: K = 3 prompts on each of B = 2 images) loads, and the torch oracle of the decoder reproduces its loss and
gradients -- which pins the fixture that tests/test_gpu_clipseg_multi_train.py holds CLIPDenseBase.forward_multi_train against."""
import numpy as np
import torch

from helpers import load_fixture
from oracle import clip_ref as C

B, K = 2, 3


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_fixture_layout():
    tr = load_fixture("clipseg_multi_train")
    norms = [k for k in tr if k.startswith("norm/")]
    assert len(norms) == 48
    for k in norms:
        probe = tr["probe/" + k[5:]]
        assert probe.ndim == 1 and 1 <= probe.shape[0] <= 257 and probe.dtype == np.float32, k
    assert tr["cond"].shape == (K, 512) and int(tr["target_seed"]) == 13 and tr["loss"].shape == ()
    assert not any(k[5:].startswith("clip_model.") for k in norms)                     # the backbone is frozen in the reference too


def test_oracle_decoder_reproduces_fixture():
    """The repeat form through oracle.clip_ref under torch autograd, with the criteria of the GPU fixture test."""
    fx, tr = load_fixture("clipseg_fwd"), load_fixture("clipseg_multi_train")
    img = torch.from_numpy(fx["img"].astype(np.float32))
    with torch.no_grad():
        _, acts = C.visual_forward(C.make_clip_state(seed=0), img, extract_layers=[0, 3, 6, 9])
    dec = {k: v.clone().requires_grad_(True) for k, v in C.make_decoder_state(seed=0).items()}
    cond = torch.from_numpy(tr["cond"])
    # sequence b*K + k = image b with prompt k: each image once per prompt
    out = C.clipseg_decoder(dec, [a.repeat_interleave(K, 0) for a in acts[1:]], cond.repeat(B, 1)).view(B, K, 352, 352)
    target = (torch.rand(B, K, 352, 352, generator=torch.Generator().manual_seed(int(tr["target_seed"]))) < 0.3).float()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out, target)
    loss.backward()
    assert abs(float(loss.detach()) - float(tr["loss"])) < 5e-5, float(loss.detach())
    n = 0
    for k in tr:
        if k.startswith("norm/"):
            name = k[5:]
            g = dec[name].grad.flatten()
            ref_norm = float(tr[k])
            assert abs(float(g.norm()) - ref_norm) <= 5e-3 * ref_norm + 1e-7, (name, float(g.norm()), ref_norm)
            assert rel(g[:: max(1, g.numel() // 257)][:257], torch.from_numpy(tr["probe/" + name])) < 2e-2, name
            n += 1
    assert n == 48
