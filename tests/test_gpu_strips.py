"""GPU: the epilogue that tile_blend_kernel, tta_merge_mean_kernel and tta_merge_prob_kernel share (csrc/strip_out.h):
with want="both" the mask a kernel writes is lut[argmax_c] of the logits the same launch writes, bit for bit, the argmax being
torch.argmax (the first maximum, so ties go to the lowest class).  The widths cross every store path: 5 (dword and byte tails only),
8 (full vectors), 257 (a second column group that is all tail) and 260 (a second column group with a full vector); the raw entry points
are called once more with the mask 1 byte off a 4-byte boundary, which takes the byte stores where W % 4 == 0.  The inputs are small
integers times a power of two, mirrored or cut from one image, so every covering tile or view agrees and the classes really tie."""
import pytest
import torch

from test_gpu_tta import _descriptors

pytestmark = pytest.mark.gpu
DEV = "cuda"
CS, HS, WS = (1, 3, 8), (1, 5), (5, 8, 257, 260)


def _image(N, C, H, W):
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W + N)
    return (torch.randint(-2, 3, (N, C, H, W), generator=g).float() * 2.0 ** (W % 5 - 2)).to(DEV)


def _expect(logits, lut):
    """-> (lut[argmax_c logits] as uint8 on the CPU, the number of pixels whose maximum is reached by two classes or more)."""
    lc = logits.cpu()
    arg = lc.argmax(1)
    ties = int(((lc == lc.max(1, keepdim=True).values).sum(1) > 1).sum())
    return (arg if lut is None else torch.tensor(lut)[arg]).to(torch.uint8), ties


def _raw_mask(call, N, C, H, W, lt):
    """call(lt, logits, mask) runs a raw entry point -> (logits, the mask it wrote 1 byte off alignment); the bytes around it kept."""
    n = N * H * W
    logits = torch.empty((N, C, H, W), device=DEV)
    mbuf = torch.full((n + 8,), 77, dtype=torch.uint8, device=DEV)
    mo = mbuf[1:1 + n]
    assert mbuf.data_ptr() % 4 == 0 and mo.data_ptr() % 4 == 1
    call(lt, logits, mo)
    assert bool((mbuf[:1] == 77).all()) and bool((mbuf[1 + n:] == 77).all())
    return logits, mo.view(N, H, W)


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("kind", ["blend", "mean", "prob"])
def test_mask_is_lut_of_argmax_of_the_logits(kind, N):
    from egm_unet_amd import tiled, tta
    from egm_unet_amd._lib import lib, ptr, stream
    from egm_unet_amd.infer import lut256
    ties = 0
    for C in CS:
        lut = [(37 * c + 11) % 256 for c in range(C)]
        for H in HS:
            for W in WS:
                x = _image(N, C, H, W)
                if kind == "blend":
                    plan = tiled.TilePlan(N, H, W, window=(4, 130), stride=(3, 127))       # 1 or 2 rows of 1, 2 or 3 tiles, overlapping
                    parts = tiled.gather_tiles(x, plan)
                    ys, xs, wy, wx = tiled._tables(plan, "gaussian", x.device)

                    def run(lu, want):
                        return tiled.blend_tiles(parts, plan, "gaussian", lut=lu, want=want)

                    def raw(lt, logits, mask):
                        lib().call("egm_tile_blend_f32", ptr(parts), N, C, H, W, ptr(ys), plan.ny, ptr(xs), plan.nx, plan.h, plan.w, ptr(wy),
                                   ptr(wx), ptr(lt), ptr(logits), ptr(mask), stream())
                else:
                    plan = tta.TTAPlan(N, H, W, scales=(1.0,), flips=("", "h"))            # two mirrored copies: the merge gives x back
                    vs = tta.make_views(x, plan, 0)
                    parts = [vs[f * N:(f + 1) * N] for f in range(plan.F)]
                    table = _descriptors(parts, plan)

                    def run(lu, want):
                        return tta.merge_views(parts, plan, kind, lut=lu, want=want)

                    def raw(lt, logits, mask):
                        lib().call("egm_tta_merge_f32", ptr(table), plan.V, N, C, H, W, tta.MERGE_MODES.index(kind), ptr(lt), ptr(logits),
                                   ptr(mask), stream())
                for lu in (None, lut):
                    logits, mask = run(lu, "both")
                    exp, t = _expect(logits, lu)
                    ties += t
                    assert mask.dtype == torch.uint8 and torch.equal(mask.cpu(), exp), (C, H, W, lu)
                    assert torch.equal(run(lu, "mask"), mask), (C, H, W, lu)               # the mask alone is the same mask
                    rl, rm = _raw_mask(raw, N, C, H, W, None if lu is None else lut256(lu, C, x.device, "lut"))
                    assert torch.equal(rl, logits) and torch.equal(rm.cpu(), exp), (C, H, W, lu)
                if kind == "mean":
                    assert torch.equal(logits, x)
    assert ties > 0                                                                        # the inputs do tie
