"""GPU: the surface distances at the masks' own size -- csrc/surface.hip (egm_mask_surface_dist_u8) through ensemble.surface_counts_u8,
surface_dist2_u8, surface_report and EnsemblePredictor.evaluate(surface=...).

Everything is integers, so every comparison is exact (torch.equal / np.array_equal) against the numpy restatement of the rules in
tests/surface_oracle.py: the [N, C, 2, 260] counts and the d^2 maps of both sides.  The shapes are the smallest that cross each width at
which the kernels change path: the row pass's 16 pixels per lane and 1024 per step, the column pass's 4 columns per lane, 256 per wave
and SURFACE_ROWS rows per wave; the long-distance cases go past what a byte holds (the 254 pixels of csrc/contour.hip), along a row,
along a column and along a diagonal."""
import numpy as np
import pytest
import torch

import contour_oracle as O
import surface_oracle as S
from test_contour_cpu import far_pairs, shifted_pair
from test_gpu_boundary import _ens, _photos_and_masks, _stack, models  # noqa: F401  (models is a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SURFACE_ROWS = 16                  # kSurfaceRows of csrc/surface.hip, restated: image rows per wave of the column pass
FIELDS = 260


def _tables(C, pv, lv):
    from egm_unet_amd.ensemble import class_table
    return torch.from_numpy(class_table(pv, C)).to(DEV), torch.from_numpy(class_table(lv, C)).to(DEV)


def _native(pred, label, C, pv=None, lv=None):
    """One call of the raw entry point with all three outputs -> (counts int64 [N, C, 2, 260], d2 of pred, d2 of label)."""
    from egm_unet_amd._lib import lib, ptr, stream
    N, H, W = pred.shape
    L = lib()
    ws = torch.empty(L.query("egm_surface_workspace", N, H, W, C), dtype=torch.uint8, device=DEV)
    pt, lt = _tables(C, pv, lv)
    counts = torch.zeros((N, C, 2, FIELDS), dtype=torch.int64, device=DEV)
    dp, dl = (torch.full((N, H, W), 0x6EEEEEEE, dtype=torch.int32, device=DEV) for _ in range(2))
    L.call("egm_mask_surface_dist_u8", ptr(pred), ptr(label), N, H, W, ptr(pt), ptr(lt), C, ptr(ws), ptr(counts), ptr(dp), ptr(dl), stream())
    return counts, dp, dl


def _check(pred_np, label_np, C, pv=None, lv=None):
    """All outputs of the kernel pair and of the Python entry points against the oracle, exactly -> (counts, d2 of pred, d2 of label)."""
    from egm_unet_amd.ensemble import surface_counts_u8, surface_dist2_u8
    if pred_np.ndim == 2:                                                      # one image: a batch of one
        pred_np, label_np = pred_np[None], label_np[None]
    want = S.counts(pred_np, label_np, C, pv, lv)
    wp, wl = (torch.from_numpy(m.astype(np.int32)) for m in S.d2_maps(pred_np, label_np, C, pv, lv))
    pred, label = torch.from_numpy(pred_np).to(DEV), torch.from_numpy(label_np).to(DEV)
    tag = (tuple(pred_np.shape), C)
    counts, dp, dl = _native(pred, label, C, pv, lv)
    assert torch.equal(dp.cpu(), wp), tag
    assert torch.equal(dl.cpu(), wl), tag
    assert torch.equal(counts.cpu(), torch.from_numpy(want)), (tag, np.argwhere(counts.cpu().numpy() != want)[:8].tolist())
    got = surface_counts_u8(pred, label, C, pv, lv)
    assert got.dtype == torch.int64 and got.shape == (pred.shape[0], C, 2, FIELDS) and torch.equal(got, counts), tag
    gp, gl = surface_dist2_u8(pred, label, C, pv, lv)
    assert gp.dtype == torch.int32 and gp.shape == pred.shape and torch.equal(gp, dp) and torch.equal(gl, dl), tag
    return want, wp.numpy(), wl.numpy()


def _f_counts_agree(pred_np, label_np, counts, C, pv=None, lv=None, thetas=(1, 2, 7, 254)):
    """On the device, against the existing kernel: the bins summed up to theta are contour_f_counts_u8(theta)'s mp and mg."""
    from egm_unet_amd.ensemble import contour_f_counts_u8
    pred, label = torch.from_numpy(pred_np).to(DEV), torch.from_numpy(label_np).to(DEV)
    for theta in thetas:
        f = contour_f_counts_u8(pred, label, theta, C, pv, lv).cpu().numpy()
        cum = counts[..., 4:5 + theta].sum(-1)
        assert np.array_equal(cum[:, :, 0], f[:, :, 0]) and np.array_equal(cum[:, :, 1], f[:, :, 2]), theta
        assert np.array_equal(counts[:, :, 0, 0], f[:, :, 1]) and np.array_equal(counts[:, :, 1, 0], f[:, :, 3]), theta


SHAPES = [(1, 1), (1, 37), (37, 1), (37, 53)]
SHAPES += [(5, W) for W in (15, 16, 17, 255, 256, 257, 1025)]                                # the row pass's vector and chunk widths
SHAPES += [(H, 21) for H in (SURFACE_ROWS - 1, SURFACE_ROWS, SURFACE_ROWS + 1, 2 * SURFACE_ROWS + 1)]  # the column pass's tile height


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_counts_and_maps(shape):
    H, W = shape
    pred, label = _stack(H, W, 2, seed=H * 10007 + W * 31)                    # zeros, ones, row, column, checker, blobs, holes
    want, wp, wl = _check(pred, label, 2)
    _f_counts_agree(pred, label, want, 2, thetas=(1, 2, 254))
    assert not want[0, :, 0].any() and (wp[0] == -1).all() and (wp[1] == -1).all()        # zeros and ones have no contour: nothing asks
    assert want[0, :, 1, 1:].sum() == 0 and (wl[0] == -1).all()                            # ... and nobody finds one: n alone
    assert np.array_equal(want[0, :, 1, 0], [int((O.contours(label[0], 2) >> k & 1).sum()) for k in range(2)])
    if H >= 3:                                                                 # pred = the row image, label = the ones: one side empty
        assert want[2, 1, 0].tolist() == [W] + [0] * (FIELDS - 1) and want[2, 1, 1].sum() == 0


@pytest.mark.parametrize("name", ["300x40", "5x1300", "70x1300"])
def test_distances_beyond_a_byte(name):
    """The 255 cap of the 6.18 kernels would fail all three: every distance of class 1 is above 254."""
    from egm_unet_amd.ensemble import surface_report
    a, b = far_pairs()[name]
    pred, label = np.stack([a, b]), np.stack([b, a])
    want, wp, wl = _check(pred, label, 2)
    assert want[:, 1, :, 3].min() > 254 * 254 and (want[:, 1, :, 4 + 255] == want[:, 1, :, 0]).all() and want[:, 1, :, 0].min() > 0
    assert want[:, 1, :, 4:4 + 255].sum() == 0
    _f_counts_agree(pred, label, want, 2, thetas=(254,))
    rep = surface_report(want)
    assert rep["hd95_capped"][:, 1].all() and (rep["hd_images"][:, 1] > 254).all() and (rep["nsd_images"][:, 1] == 0).all()
    for key, val in S.report(want).items():
        assert np.array_equal(np.asarray(rep[key]), np.asarray(val), equal_nan=True), key


def test_analytic_cases():
    from egm_unet_amd.ensemble import surface_counts_u8, surface_dist2_u8, surface_report
    blob = O.blobs(np.random.default_rng(11), 37, 53, density=0.02, grow=4)
    t = torch.from_numpy(blob).to(DEV)
    cnt = surface_counts_u8(t, t).cpu().numpy()                                # a mask against itself
    k = O.contours(blob, 2)
    assert cnt.shape == (1, 2, 2, FIELDS) and (cnt[0, :, :, 1:4] == 0).all() and (cnt[0, :, :, 5:] == 0).all()
    assert np.array_equal(cnt[0, :, 0, 0], cnt[0, :, 0, 4]) and cnt[0, :, 0, 0].tolist() == [int((k & 1).sum()), int((k >> 1).sum())]
    dp, dl = surface_dist2_u8(t, t)
    assert torch.equal(dp, dl) and np.array_equal(dp.cpu().numpy(), np.where(k > 0, 0, -1))
    rep = surface_report(cnt)
    assert rep["hd"].tolist() == [0.0, 0.0] and rep["assd"].tolist() == [0.0, 0.0] and rep["nsd"].tolist() == [1.0, 1.0]
    # three rows lower.  Away from the frame every contour pixel of the blob class has its partner exactly 3 away, so HD95 is 3; the
    # whole image's HD is 6, not 3: a blob that the top frame cuts has no contour there, its shifted copy has one at row 3, and the
    # bottom rows lose theirs (the oracle, which agrees with scipy's distance transform, gives d^2 = 25 and 36 for the two directions)
    pred, label = shifted_pair()
    want, wp, wl = _check(pred, label, 2)
    rep = surface_report(want, tolerance=3)
    inner = np.zeros(pred.shape, dtype=bool)
    inner[4:-4, 4:-4] = True
    kp, kl = (O.contours(pred, 2) >> 1).astype(bool), (O.contours(label, 2) >> 1).astype(bool)
    assert wp[0][kp & inner].max() == 9 and wl[0][kl & inner].max() == 9 and want[0, 1, :, 3].tolist() == [25, 36]
    assert rep["hd"][1] == 6.0 and rep["hd95"][1] == 3.0 and 0 < rep["assd"][1] < 3.0 and not rep["hd95_capped"].any()
    box, low = np.zeros((40, 50), dtype=np.uint8), np.zeros((40, 50), dtype=np.uint8)
    box[10:20, 10:30], low[13:23, 10:30] = 255, 255                            # a shape the frame does not cut, three rows lower: HD = 3
    rep = surface_report(_check(box, low, 2)[0], tolerance=3)
    assert rep["hd"].tolist() == [3.0, 3.0] and rep["hd95"].tolist() == [3.0, 3.0] and rep["nsd"].tolist() == [1.0, 1.0]
    one, two = np.zeros((9, 11), dtype=np.uint8), np.zeros((9, 11), dtype=np.uint8)
    one[2, 3], two[5, 7] = 255, 255                                            # a single pixel pair at offset (3, 4)
    want, wp, wl = _check(one, two, 2)
    cell = [0] * FIELDS
    cell[0], cell[1], cell[2], cell[3], cell[4 + 5] = 1, 1280, 25, 25, 1
    assert want[0, 1, 0].tolist() == cell and want[0, 1, 1].tolist() == cell and wp[0, 2, 3] == 25 and wl[0, 5, 7] == 25
    rep = surface_report(want)
    assert rep["hd"][1] == 5.0 and rep["assd"][1] == 5.0 and rep["rmsd"][1] == 5.0 and rep["hd95"][1] == 5.0 and rep["nsd"][1] == 0.0


def test_empty_sides():
    H, W = 21, 30
    rng = np.random.default_rng(4)
    blob = O.blobs(rng, H, W, density=0.03, grow=3)
    zeros, ones = np.zeros((H, W), dtype=np.uint8), np.full((H, W), 255, dtype=np.uint8)
    pred, label = np.stack([blob, zeros, zeros, ones]), np.stack([zeros, blob, ones, zeros])
    want, wp, wl = _check(pred, label, 2)
    k = O.contours(blob, 2)
    n = [int((k & 1).sum()), int((k >> 1).sum())]
    assert min(n) > 0 and want[0, :, 0, 0].tolist() == n and want[1, :, 1, 0].tolist() == n      # n is counted ...
    assert want[..., 1:].sum() == 0 and want[2:].sum() == 0                    # ... and nothing else; both sides empty: all zero
    assert (wp == -1).all() and (wl == -1).all()


def test_batch_images_do_not_bleed():
    """test_gpu_contour.py's construction: image n ends in a contour and image n + 1 begins with one.  A walk that crossed the image
    border would find the next image's line three rows away; inside the image the nearest contour is farther."""
    H, W = 40, 50
    rng = np.random.default_rng(5)
    pred = np.zeros((4, H, W), dtype=np.uint8)
    pred[0, H - 12:, :] = 255
    pred[1, :12, :] = 255
    pred[1, H - 9:, 10:40] = 255
    pred[2, H - 2, 5:45] = 255                                                  # a line two rows above ...
    pred[3] = O.blobs(rng, H, W, density=0.02, grow=4)
    label = np.stack([pred[1], O.blobs(rng, H, W, density=0.02, grow=4), pred[0], np.zeros((H, W), dtype=np.uint8)])
    label[3, 1, 5:45] = 255                                                     # ... the line of the NEXT image's label
    want, wp, wl = _check(pred, label, 2)
    assert want[2, 1, 0, 0] == 40 and want[2, 1, 0, 3] == 100 and want[2, 1, 0, 4 + 10] == 40 # image 2's line: ten rows below its label's edge,
    assert (wp[2][H - 2, 5:45] == 100).all()                                    # three rows above the next image's line
    assert len({tuple(want[n].flatten().tolist()) for n in range(4)}) == 4
    for n in range(4):                                                          # every image alone gives its own row of the batch
        assert np.array_equal(S.counts(pred[n], label[n], 2)[0], want[n])


@pytest.mark.parametrize("C,pv,lv", [(1, (255,), (7,)), (2, (0, 255), (255, 0)), (2, None, None), (3, (0, 255, 100), (255, 7, 0)),
                                     (4, (0, 255, 7, 100), (100, 0, 255, 7))])
def test_classes_and_tables(C, pv, lv):
    """Blobs of several byte values with stray bytes on top: a byte its side's table does not list is in no class and in no contour,
    and counts as "not k" for the classes around it."""
    H, W = 45, 70
    rng = np.random.default_rng(100 + C)
    vals = np.array([0, 255, 7, 100, 128, 254], dtype=np.uint8)

    def image():
        img = np.zeros((H, W), dtype=np.uint8)
        for v in (255, 7, 100):
            img = np.where(O.blobs(rng, H, W, density=0.006, grow=4) > 0, v, img).astype(np.uint8)
        return np.where(rng.random((H, W)) < 0.01, vals[rng.integers(0, len(vals), (H, W))], img).astype(np.uint8)

    pred, label = np.stack([image(), image()]), np.stack([image(), image()])
    if pv is None:                                                             # the default tables are for 0/255 masks
        pred, label = np.where(pred == 255, 255, 0).astype(np.uint8), np.where(label == 255, 255, 0).astype(np.uint8)
    want, wp, wl = _check(pred, label, C, pv, lv)
    _f_counts_agree(pred, label, want, C, pv, lv, thetas=(1, 3))
    for k in range(C):
        assert want[:, k, :, 0].min() > 0 and want[:, k, :, 3].max() > 0        # every class has contours and distances on both sides
    if pv is not None:
        dropped = O.class_table(pv, C)[pred] == 255
        assert dropped.any() and (wp[dropped] == -1).all()


def test_alignment_and_sliced_batch():
    """Images at odd byte offsets of larger buffers (counts, maps and workspace at the alignment of their element types), a batch that
    is a slice of a larger one and a view that is not contiguous."""
    from egm_unet_amd._lib import lib, ptr, stream
    from egm_unet_amd.ensemble import surface_counts_u8, surface_dist2_u8
    N, H, W, C, pv, lv = 2, 13, 37, 3, (0, 255, 100), (255, 7, 0)
    npix = N * H * W
    rng = np.random.default_rng(77)
    vals = np.array([0, 255, 7, 100, 128], dtype=np.uint8)
    src = [np.where(rng.random((N + 2, H, W)) < 0.05, vals[rng.integers(0, 5, (N + 2, H, W))],
                    np.stack([O.blobs(rng, H, W, density=0.03, grow=3) for _ in range(N + 2)])).astype(np.uint8) for _ in range(2)]
    want = torch.from_numpy(S.counts(src[0][:N], src[1][:N], C, pv, lv))
    wp, wl = (torch.from_numpy(m.astype(np.int32)) for m in S.d2_maps(src[0][:N], src[1][:N], C, pv, lv))
    bufs = [torch.zeros(npix + 64, dtype=torch.uint8, device=DEV) for _ in range(2)]
    outs = [torch.zeros(npix + 16, dtype=torch.int32, device=DEV) for _ in range(2)]
    L = lib()
    ws = torch.empty(L.query("egm_surface_workspace", N, H, W, C) + 16, dtype=torch.uint8, device=DEV)
    pt, lt = _tables(C, pv, lv)
    for po, lo, mo in ((0, 0, 0), (1, 3, 1), (3, 15, 2), (15, 1, 3)):
        p, t = bufs[0][po:po + npix].view(N, H, W), bufs[1][lo:lo + npix].view(N, H, W)
        p.copy_(torch.from_numpy(src[0][:N]))
        t.copy_(torch.from_numpy(src[1][:N]))
        for o in outs:
            o.fill_(0x6EEEEEEE)
        dp, dl = outs[0][mo:mo + npix].view(N, H, W), outs[1][(mo + 1) % 4:(mo + 1) % 4 + npix].view(N, H, W)
        counts = torch.zeros((N, C, 2, FIELDS), dtype=torch.int64, device=DEV)
        L.call("egm_mask_surface_dist_u8", ptr(p), ptr(t), N, H, W, ptr(pt), ptr(lt), C, ptr(ws[po:]), ptr(counts), ptr(dp), ptr(dl), stream())
        assert torch.equal(counts.cpu(), want) and torch.equal(dp.cpu(), wp) and torch.equal(dl.cpu(), wl), (po, lo, mo)
        for o, off in ((outs[0], mo), (outs[1], (mo + 1) % 4)):                 # nothing written around the maps
            assert bool((o[:off] == 0x6EEEEEEE).all()) and bool((o[off + npix:] == 0x6EEEEEEE).all()), (po, lo, mo)
        assert torch.equal(surface_counts_u8(p, t, C, pv, lv).cpu(), want), (po, lo)
    big_p, big_t = torch.from_numpy(src[0]).to(DEV), torch.from_numpy(src[1]).to(DEV)
    for lo in (1, 2):                                                           # images lo, lo + 1 of a batch of four
        w = S.counts(src[0][lo:lo + 2], src[1][lo:lo + 2], C, pv, lv)
        assert torch.equal(surface_counts_u8(big_p[lo:lo + 2], big_t[lo:lo + 2], C, pv, lv).cpu(), torch.from_numpy(w))
    cp, ct = big_p[:2, :, 3:30], big_t[:2, :, 3:30]                             # not contiguous: copied by the Python layer
    w = S.counts(src[0][:2, :, 3:30], src[1][:2, :, 3:30], C, pv, lv)
    assert torch.equal(surface_counts_u8(cp, ct, C, pv, lv).cpu(), torch.from_numpy(w))
    gp, _ = surface_dist2_u8(cp, ct, C, pv, lv)
    assert gp.shape == cp.shape and np.array_equal(gp.cpu().numpy(), S.d2_maps(src[0][:2, :, 3:30], src[1][:2, :, 3:30], C, pv, lv)[0])


def test_out_accumulates_and_validation():
    from egm_unet_amd.ensemble import surface_counts_u8, surface_dist2_u8, surface_workspace
    rng = np.random.default_rng(9)
    H, W = 60, 110
    a, b, c = (np.stack([O.blobs(rng, H, W, density=0.004, grow=5) for _ in range(2)]) for _ in range(3))
    ta, tb, tc = (torch.from_numpy(x).to(DEV) for x in (a, b, c))
    w1, w2 = S.counts(a, b, 2), S.counts(c, b, 2)
    acc = surface_counts_u8(ta, tb)
    assert acc.shape == (2, 2, 2, FIELDS) and torch.equal(acc.cpu(), torch.from_numpy(w1))
    assert surface_counts_u8(tc, tb, out=acc) is acc                            # out= accumulates and is returned
    both = w1 + w2
    both[..., 3] = np.maximum(w1[..., 3], w2[..., 3])                           # the maximum is combined with max, not add
    assert torch.equal(acc.cpu(), torch.from_numpy(both))
    assert (w1[..., 3] > w2[..., 3]).any() and (w1[..., 3] < w2[..., 3]).any() and (np.minimum(w1[..., 3], w2[..., 3]) > 0).all()
    one = surface_counts_u8(ta[0], tb[0])                                       # [H, W] -> [1, C, 2, 260]
    assert one.shape == (1, 2, 2, FIELDS) and torch.equal(one[0], surface_counts_u8(ta, tb)[0])
    dp, dl = surface_dist2_u8(ta[1], tb[1])
    assert dp.shape == (H, W) and dl.shape == (H, W) and torch.equal(dp, surface_dist2_u8(ta, tb)[0][1])
    for bad in (lambda: surface_counts_u8(ta.cpu(), tb), lambda: surface_counts_u8(ta.long(), tb), lambda: surface_counts_u8(ta, tb[:1]),
                lambda: surface_counts_u8(ta[:0], tb[:0]), lambda: surface_counts_u8(ta, tb, 5), lambda: surface_counts_u8(ta, tb, 0),
                lambda: surface_counts_u8(ta, tb, out=torch.zeros((2, 2, 2, 256), dtype=torch.int64, device=DEV)),
                lambda: surface_counts_u8(ta, tb, out=torch.zeros((2, 2, 2, FIELDS), dtype=torch.int32, device=DEV)),
                lambda: surface_counts_u8(ta, tb, out=torch.zeros((2, 2, 2, FIELDS), dtype=torch.int64)),
                lambda: surface_counts_u8(ta, tb, workspace=surface_workspace(1, H, W, 2, DEV)),
                lambda: surface_dist2_u8(ta, tb.cpu()), lambda: surface_dist2_u8(ta, tb, 2, (0, 0)),
                lambda: surface_counts_u8(torch.zeros((1, 32768), dtype=torch.uint8, device=DEV), torch.zeros((1, 32768), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            bad()


def test_workspace_cache_is_bounded_and_caller_workspace():
    from egm_unet_amd import ensemble as E
    rng = np.random.default_rng(21)
    want = {}
    n_contour = len(E._workspace_caches["contour"])
    for W in range(30, 30 + E._BOUNDARY_WORKSPACES + 3):                        # more shapes than the module keeps
        a, b = O.blobs(rng, 20, W, density=0.03, grow=3), O.blobs(rng, 20, W, density=0.03, grow=3)
        want[W] = (a, b, S.counts(a, b, 2))
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        assert torch.equal(E.surface_counts_u8(ta, tb).cpu(), torch.from_numpy(want[W][2]))
        assert len(E._workspace_caches["surface"]) <= E._BOUNDARY_WORKSPACES
    dev = str(torch.device(DEV, torch.cuda.current_device()))
    assert (1, 20, 30, 2, dev) not in E._workspace_caches["surface"] and (1, 20, 36, 2, dev) in E._workspace_caches["surface"]     # the oldest went first
    assert len(E._workspace_caches["contour"]) == n_contour                         # the contour kernels' cache is its own
    a, b, cnt = want[30]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ws = E.surface_workspace(1, 20, 30, 2, DEV)
    assert ws.numel() == E.lib().query("egm_surface_workspace", 1, 20, 30, 2) and ws.dtype == torch.uint8
    keys = list(E._workspace_caches["surface"])
    assert torch.equal(E.surface_counts_u8(ta, tb, workspace=ws).cpu(), torch.from_numpy(cnt))
    assert torch.equal(E.surface_dist2_u8(ta, tb, workspace=ws)[0], E.surface_dist2_u8(ta, tb)[0])
    assert list(E._workspace_caches["surface"])[:len(keys) - 1] == keys[1:]          # only the call without a workspace touched the cache
    for bad in (ws[:16], ws.cpu(), ws.to(torch.int8), E.contour_workspace(1, 20, 30, 2, DEV)):    # (the contour workspace is too small)
        with pytest.raises(ValueError):
            E.surface_counts_u8(ta, tb, workspace=bad)
        with pytest.raises(ValueError):
            E.surface_dist2_u8(ta, tb, workspace=bad)


def test_graph_capture():
    """The call (two launches) captured once on one stream on the caller's workspace and replayed on new content."""
    from egm_unet_amd.ensemble import surface_counts_u8, surface_workspace
    N, H, W = 2, 61, 83
    rng = np.random.default_rng(13)
    contents = [tuple(np.stack([O.blobs(rng, H, W, density=0.02, grow=4) for _ in range(N)]) for _ in range(2)) for _ in range(3)]
    pred, label = torch.from_numpy(contents[0][0]).to(DEV), torch.from_numpy(contents[0][1]).to(DEV)
    out = torch.zeros((N, 2, 2, FIELDS), dtype=torch.int64, device=DEV)
    ws = surface_workspace(N, H, W, 2, DEV)                                     # the graph keeps its address: owned here, not the module's
    surface_counts_u8(pred, label, out=out, workspace=ws)                       # warm-up: the tables are uploaded here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        surface_counts_u8(pred, label, out=out, workspace=ws)
    for p_np, t_np in contents[1:]:
        pred.copy_(torch.from_numpy(p_np))
        label.copy_(torch.from_numpy(t_np))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(S.counts(p_np, t_np, 2)))


# ---------------------------------------------------------------- the predictor
@pytest.mark.parametrize("cleanup", [False, True], ids=["plain", "cleanup"])
def test_predictor_evaluate_surface(models, cleanup):  # noqa: F811
    from egm_unet_amd.ensemble import MaskCleanup, contour_radius, plan_batches, score_report
    photos, masks = _photos_and_masks()
    kw = dict(alpha=0.7, cleanup=MaskCleanup(min_area=8)) if cleanup else dict(alpha=0.7)
    ens = _ens(models, **kw)
    keys = {"hd", "hd95", "assd", "rmsd", "nsd", "hd_images", "hd95_images", "assd_images", "rmsd_images", "nsd_images", "hd95_capped",
            "undefined", "one_empty", "n_images"}
    for batch_size in (None, 2):
        if batch_size is None:
            preds = [ens(im, clone=True) for im in photos]
        else:                                                                   # the batches evaluate() forms, from the same plan
            preds = [None] * len(photos)
            for _, idx, pad in plan_batches([tuple(im.shape[:2]) for im in photos], batch_size):
                rows = ens.predict_batch([photos[i] for i in idx] + [photos[idx[-1]]] * pad, clone=True)
                for row, i in enumerate(idx):
                    preds[i] = rows[row]
        want = np.concatenate([S.counts(p.cpu().numpy(), m, 2, (0, 255), None) for p, m in zip(preds, masks)])
        for tol in (3, 0.02):                                                   # pixels, and a ratio of each photo's own diagonal
            taus = [contour_radius(*m.shape, tol) for m in masks]
            rep = ens.evaluate(photos, masks, batch_size=batch_size, surface=tol)
            wrep = S.report(want, taus)
            assert set(rep["surface"]) == keys and rep["skipped"] == 0 and rep["surface"]["n_images"] == len(photos)
            for key in wrep:                                                    # in input order
                assert np.array_equal(np.asarray(rep["surface"][key]), np.asarray(wrep[key]), equal_nan=True), (batch_size, tol, key)
        assert len(set(contour_radius(*m.shape, 0.02) for m in masks)) == 2     # the ratio gave the two sizes two tolerances
        assert want[:, 1, 1, 0].min() > 0                                       # every ground truth has a contour
        # beside the other scores: theirs are unchanged and the surface's too
        rep_all = ens.evaluate(photos, masks, batch_size=batch_size, boundary=3, boundary_metric="euclid", contour_f=2, surface=3)
        rep_two = ens.evaluate(photos, masks, batch_size=batch_size, boundary=3, boundary_metric="euclid", contour_f=2)
        rep_one = ens.evaluate(photos, masks, batch_size=batch_size, surface=3)
        assert set(rep_all) == set(rep_two) | {"surface"} and "boundary" not in rep_one and "contour_f" not in rep_one
        assert np.array_equal(rep_all["boundary"]["counts"], rep_two["boundary"]["counts"])
        assert np.array_equal(rep_all["contour_f"]["f_images"], rep_two["contour_f"]["f_images"], equal_nan=True)
        for key in keys:
            assert np.array_equal(np.asarray(rep_all["surface"][key]), np.asarray(rep_one["surface"][key]), equal_nan=True), key
        # a ground truth of another size is skipped
        short = masks[:3] + [np.ascontiguousarray(masks[3][:70, :90])]
        rep2 = ens.evaluate(photos, short, batch_size=batch_size, surface=3)
        wrep = S.report(want[:3], 3)
        assert rep2["skipped"] == 1 and rep2["surface"]["hd_images"].shape == (3, 2)
        for key in wrep:
            assert np.array_equal(np.asarray(rep2["surface"][key]), np.asarray(wrep[key]), equal_nan=True), key
        # with the default: today's keys, and the same region scores
        rep3 = ens.evaluate(photos, masks, batch_size=batch_size)
        assert set(rep3) == set(score_report(np.zeros((2, 2), dtype=np.int64))) | {"skipped"}
        assert np.array_equal(rep3["hist"], rep_one["hist"]) and rep3["miou"] == rep_one["miou"]
    for bad in (dict(surface=1.5), dict(surface=255), dict(surface=0), dict(surface=True), dict(surface="2")):
        with pytest.raises(ValueError):
            ens.evaluate(photos, masks, **bad)
