"""Guided upsampling without a GPU: what the rule's numbers (refine.GuidedUpsample, as the kernels get them) do in the
numpy restatement, the rule's validation and the entry points' host-side argument checks.

Measured with tests/guided_oracle.py on its four scenes (nearest IoU -> float64 guided IoU; max |q32 - q64|; share of pixels with a
float64 margin |q1 - q0| below 1e-3; mask differences float32 against float64):
    scene 1   0.8415 -> 0.9850   5.8e-06   0.008 %   0
    scene 2   0.8475 -> 0.9968   3.8e-05   0.008 %   0
    scene 3   0.7271 -> 0.9556   5.8e-07   0.009 %   0
    scene 4   0.8562 -> 0.9514   3.4e-05   0.000 %   0
"""
import ctypes
import functools

import numpy as np
import pytest

import guided_oracle as O

F32, F64 = np.float32, np.float64


def _guided(photos, G, S, r, eps, dt):
    """The restatement's chain on the numbers the package's rule hands to the kernels -> q [N, C, H0, W0]."""
    from egm_unet_amd.refine import GuidedUpsample
    rule = GuidedUpsample(r, eps)
    A, _ = O.coefs(G, S, rule.radius, rule.eps3, dt)
    return O.apply(photos, A, rule.scale3, rule.offset3, dt)


@functools.lru_cache(maxsize=None)
def _scene(k):
    """Scene k and its float64 and float32 results, computed once and shared (read only)."""
    H, W, f, r, eps, seed = O.SCENES[k]
    sc = O.scene(H, W, f, seed)
    ph, G, S = sc["photo"][None], sc["guide"][None], sc["scores"][None]
    return sc, _guided(ph, G, S, r, eps, F64), _guided(ph, G.astype(F32), S.astype(F32), r, eps, F32)


def test_constant_scores_give_the_constant():
    """S_c = k_c everywhere: every v_i is 0 up to the rounding of the means, so a = 0 and b = k_c, whatever the guide and the photo."""
    rng = np.random.default_rng(0)
    G = rng.normal(size=(2, 3, 20, 30))
    consts = (0.25, -3.0, 7.5)
    S = np.broadcast_to(np.asarray(consts)[None, :, None, None], (2, 3, 20, 30))
    photos = rng.integers(0, 256, (2, 47, 61, 3), dtype=np.uint8)
    for r in (1, 3):
        q = _guided(photos, G, S, r, 1e-3, F64)
        for c, k in enumerate(consts):
            dev = float(np.abs(q[:, c] - k).max())
            print(f"r={r} class {c}: max |q - {k}| = {dev:.3g}")
            assert dev <= 1e-12


@pytest.mark.parametrize("k", range(len(O.SCENES)))
def test_guided_beats_nearest(k):
    sc, q64, _ = _scene(k)
    f = O.SCENES[k][2]
    near, guided = O.iou(O.nearest_mask(sc["scores"], f), sc["truth"]), O.iou(O.mask(q64)[0], sc["truth"])
    print(f"scene {k + 1}: nearest IoU {near:.4f}, guided IoU {guided:.4f}")
    assert guided >= near + 0.05


@pytest.mark.parametrize("k", range(len(O.SCENES)))
def test_float32_restatement_against_float64(k):
    """The float32 mask equals the float64 mask wherever the float64 margin is at least 1e-3; at most 0.1 % of the pixels are closer."""
    _, q64, q32 = _scene(k)
    assert q32.dtype == F32 and q64.dtype == F64
    margin = np.abs(q64[0, 1] - q64[0, 0])
    close = margin < 1e-3
    m64, m32 = O.mask(q64)[0], O.mask(q32)[0]
    print(f"scene {k + 1}: max |q32 - q64| = {float(np.abs(q32 - q64).max()):.3g}, close pixels {100.0 * close.mean():.4f} %, "
          f"mask differences {int((m64 != m32).sum())}")
    assert close.mean() <= 1e-3
    assert np.array_equal(m64[~close], m32[~close])


def test_class_map_source_equals_one_hot_scores():
    from egm_unet_amd.refine import GuidedUpsample
    rng = np.random.default_rng(5)
    G = rng.normal(size=(2, 3, 17, 23)).astype(F32)
    cls = rng.integers(0, 3, (2, 17, 23), dtype=np.uint8)
    S = O.one_hot(cls, 3, F32)
    assert S.shape == (2, 3, 17, 23) and np.array_equal(S.sum(1), np.ones((2, 17, 23), F32)) and np.array_equal(np.argmax(S, 1), cls)
    eps3 = GuidedUpsample(2, 1e-3).eps3
    A_cls, _ = O.coefs(G, O.one_hot(cls, 3, F32), 2, eps3, F32)
    want = np.zeros((2, 3, 17, 23), F32)
    for c in range(3):
        want[:, c][cls == c] = 1
    A_hot, _ = O.coefs(G, want, 2, eps3, F32)
    assert A_cls.dtype == F32 and A_cls.tobytes() == A_hot.tobytes()


def test_rule_validation():
    from egm_unet_amd.refine import GuidedUpsample
    rule = GuidedUpsample()
    assert (rule.radius, rule.eps, rule.mean, rule.std) == (4, 1e-3, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    for radius in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            GuidedUpsample(radius=radius)
    for eps in (0, 0.0, -1e-3, float("nan"), float("inf"), None, 1e-60):
        with pytest.raises(ValueError):
            GuidedUpsample(eps=eps)
    for std in ((1, 0, 1), (1, 1), (1, -1, 1), (1, float("nan"), 1), 1.0):
        with pytest.raises(ValueError):
            GuidedUpsample(std=std)
    for mean in ((0, 0), (0, float("inf"), 0)):
        with pytest.raises(ValueError):
            GuidedUpsample(mean=mean)
    assert GuidedUpsample(1).radius == 1 and GuidedUpsample(16).radius == 16
    mean, std = (0.709, 0.381, 0.224), (0.127, 0.079, 0.043)
    rule = GuidedUpsample(2, 1e-3, mean, std)
    scale3, offset3, eps3 = O.rule_numbers(1e-3, mean, std)
    assert rule.scale3 == tuple(float(v) for v in scale3) and rule.offset3 == tuple(float(v) for v in offset3)
    assert rule.eps3 == tuple(float(v) for v in eps3)
    assert rule == GuidedUpsample(2, 1e-3).with_norm(mean, std) and rule != GuidedUpsample(2, 1e-3) and hash(rule) == hash(rule.with_norm(mean, std))
    with pytest.raises(AttributeError):
        rule.radius = 3


def test_argument_validation_without_gpu():
    """Host-side checks run before any launch: bad arguments return EGM_ERR_ARG with a message.  (The pointers are never followed.)"""
    from egm_unet_amd import build
    from egm_unet_amd._lib import lib
    build.build(verbose=False)
    L = lib()
    err = L.cdll.egm_last_error
    ws, co, ap, fu = L.cdll.egm_guided_workspace, L.cdll.egm_guided_coefs_f32, L.cdll.egm_guided_apply_u8, L.cdll.egm_ensemble_fuse_dev_f32
    p = ctypes.c_void_p(4096)                                   # stands for a device pointer
    N, C, h, w, r = 2, 2, 37, 53, 2
    e3 = (1e-3, 1e-3, 1e-3)
    assert ws(N, C, h, w) == N * h * w * 4 * C * 4 and ws(1, 1, 1, 1) > 0 and ws(8, 8, 565, 753) > 0
    assert ws(0, C, h, w) == -1 and b"bad shape" in err()
    assert ws(N, 9, h, w) == -1 and b"classes" in err() and ws(N, 0, h, w) == -1 and b"classes" in err()
    assert ws(N, C, 32768, w) == -1 and b"32767" in err()
    # coefs: guide, scores, cls, N, C, h, w, r, eps x 3, A_out, workspace, stream
    assert co(None, p, None, N, C, h, w, r, *e3, p, p, None) == -1 and b"null pointer" in err()
    assert co(p, p, None, N, C, h, w, r, *e3, None, p, None) == -1 and b"null pointer" in err()
    assert co(p, p, None, N, C, h, w, r, *e3, p, None, None) == -1 and b"null pointer" in err()
    assert co(p, None, None, N, C, h, w, r, *e3, p, p, None) == -1 and b"neither" in err()
    assert co(p, p, p, N, C, h, w, r, *e3, p, p, None) == -1 and b"both" in err()
    assert co(p, p, None, N, C, h, w, 17, *e3, p, p, None) == -1 and b"radius 17" in err()
    assert co(p, None, p, N, C, h, w, 0, *e3, p, p, None) == -1 and b"radius 0" in err()
    assert co(p, p, None, N, 9, h, w, r, *e3, p, p, None) == -1 and b"9 classes" in err()
    assert co(p, p, None, N, 0, h, w, r, *e3, p, p, None) == -1 and b"classes" in err()
    assert co(p, p, None, 0, C, h, w, r, *e3, p, p, None) == -1 and b"bad shape" in err()
    assert co(p, p, None, N, C, h, 32768, r, *e3, p, p, None) == -1 and b"32767" in err()
    for k in range(3):
        for bad in (0.0, -1e-3, float("nan"), float("inf")):
            eps = list(e3)
            eps[k] = bad
            assert co(p, p, None, N, C, h, w, r, *eps, p, p, None) == -1 and b"eps[%d]" % k in err()
    assert co(p, p, None, N, C, h, w, r, *e3, ctypes.c_void_p(4100), p, None) == -1 and b"aligned" in err()
    # apply: imgs, N, H0, W0, A, C, h, w, yi, yl, xi, xl, scale x 3, offset x 3, lut, mask_out, q_out, stream
    H0, W0 = 149, 211
    so = (1 / 255, 1 / 255, 1 / 255, 0.0, 0.0, 0.0)
    assert ap(None, N, H0, W0, p, C, h, w, p, p, p, p, *so, None, p, None, None) == -1 and b"null pointer" in err()
    assert ap(p, N, H0, W0, None, C, h, w, p, p, p, p, *so, None, p, None, None) == -1 and b"null pointer" in err()
    assert ap(p, N, H0, W0, p, C, h, w, p, p, p, p, *so, None, None, p, None) == -1 and b"null pointer" in err()
    for k in range(4):
        tabs = [p] * 4
        tabs[k] = None
        assert ap(p, N, H0, W0, p, C, h, w, *tabs, *so, None, p, None, None) == -1 and b"null pointer" in err()
    assert ap(p, N, H0, W0, p, 9, h, w, p, p, p, p, *so, None, p, None, None) == -1 and b"9 classes" in err()
    assert ap(p, N, 0, W0, p, C, h, w, p, p, p, p, *so, None, p, None, None) == -1 and b"bad shape" in err()
    assert ap(p, N, H0, W0, p, C, 0, w, p, p, p, p, *so, None, p, None, None) == -1 and b"bad shape" in err()
    assert ap(p, N, H0, 32768, p, C, h, w, p, p, p, p, *so, None, p, None, None) == -1 and b"32767" in err()
    assert ap(p, N, H0, W0, ctypes.c_void_p(4100), C, h, w, p, p, p, p, *so, None, p, None, None) == -1 and b"aligned" in err()
    # fuse: clip, unet, alpha_dev, N, C, hc, wc, H, W, fused, stream
    for k in (0, 1, 2, 9):
        args = [p, p, p, 1, 2, 8, 8, 16, 16, p]
        args[k] = None
        assert fu(*args, None) == -1 and b"null pointer" in err()
    assert fu(p, p, p, 0, 2, 8, 8, 16, 16, p, None) == -1 and b"bad shape" in err()
    assert fu(p, p, p, 1, 2, 8, 0, 16, 16, p, None) == -1 and b"bad shape" in err()
