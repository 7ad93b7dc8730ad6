"""Inference operators of the CLIP / CLIPSeg path over libegm_hip.so (no autograd: the CLIP backbone is frozen in the
reference, models/clipseg.py:155-156, and only forward passes are used by predict_CLIPseg.py / eval_CLIPseg.py)."""
import math
from types import SimpleNamespace

import torch

from .._lib import dtype_code, lib, ptr, stream

_cast_cache = {}
_cast_generation = [0]


def bump_cast_generation():
    """Called by optimizers that update parameters through raw pointers (no torch version bump)."""
    _cast_generation[0] += 1


def cast_weight(w: torch.Tensor, dtype):
    """fp32 parameter -> contiguous matrix in the activation dtype (cached on storage + version)."""
    if dtype == torch.float32:
        return w.detach().contiguous()
    # a view of a parameter (weight.reshape(...), a slice of in_proj_weight) is a new tensor object on every call: the cache entry hangs on
    # the base tensor + offset + shape, so those hit too (they re-cast every step before: 17 cast launches per CLIPSeg forward)
    base = w._base if w._base is not None else w
    slot = (id(base), w.storage_offset(), tuple(w.shape), tuple(w.stride()))
    key = (w.data_ptr(), base._version, _cast_generation[0], dtype)
    hit = _cast_cache.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    src = w.detach().contiguous()
    out = torch.empty(src.shape, dtype=dtype, device=w.device)
    lib().call("egm_cast_f32", dtype_code(dtype), ptr(src), ptr(out), src.numel(), stream())
    _cast_cache[slot] = (key, out)
    return out


def gemm(A, lda, B, ldb, transB, C, ldc, M, N, K, dtype, bias=None, act=0, R=None, ldr=0, alpha=1.0, c_f32=False, nb1=1, nb2=1,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), sR=(0, 0), offA=0, offB=0, offC=0):
    """Thin wrapper over egm_gemm; A/B/C/R are tensors, off* element offsets into them."""
    es = 2 if dtype == torch.bfloat16 else 4
    ces = 4 if c_f32 else es
    import ctypes
    pa = ctypes.c_void_p(A.data_ptr() + offA * es)
    pb = ctypes.c_void_p(B.data_ptr() + offB * es)
    pc = ctypes.c_void_p(C.data_ptr() + offC * ces)
    lib().call("egm_gemm", dtype_code(dtype), pa, lda, pb, ldb, 1 if transB else 0, pc, ldc, 1 if c_f32 else 0, ptr(bias), act, ptr(R), ldr,
               float(alpha), M, N, K, nb1, nb2, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], sR[0], sR[1], stream())


def linear(x, weight, bias=None, act=0, residual=None):
    """x [..., K] (dtype T) @ weight[N, K]^T (+bias) -> [..., N]; act: 0 none, 1 ReLU, 2 QuickGELU; residual added after act."""
    K = x.shape[-1]
    N = weight.shape[0]
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    w = cast_weight(weight, x.dtype)
    b = bias.detach().float().contiguous() if bias is not None else None
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    r2 = residual.reshape(-1, N) if residual is not None else None
    gemm(x2, K, w, K, True, out, N, M, N, K, x.dtype, bias=b, act=act, R=r2, ldr=N)
    return out.reshape(*x.shape[:-1], N)


def matmul_kn(x, w_kn):
    """x [M, K] @ w[K, N] (weight stored [K][N], e.g. visual.proj / text_projection)."""
    M, K = x.shape
    N = w_kn.shape[1]
    w = cast_weight(w_kn, x.dtype)
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    gemm(x, K, w, N, False, out, N, M, N, K, x.dtype)
    return out


def layernorm(x, ln):
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    y = torch.empty_like(x2)
    lib().call("egm_layernorm", dtype_code(x.dtype), ptr(x2), D, ptr(ln.weight.detach().float()), ptr(ln.bias.detach().float()), float(ln.eps),
               ptr(y), D, x2.shape[0], D, stream())
    return y.reshape(x.shape)


def attention(qkv, n_heads, mode, cls_mask=None):
    """qkv [B, L, 3D] -> [B, L, D].  mode: 'csa' (softmax(qq^T s) + softmax(kk^T s)), 'causal', 'full'.
    cls_mask [nmask, L-1] fp32: multiplies the class token's attention row, head bh taking row bh % nmask (the reference's pairing,
    models/clipseg.py:111-117); runs on the unfused path (the probabilities are materialised)."""
    B, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // n_heads
    Lp = (L + 7) // 8 * 8
    dt, dev = qkv.dtype, qkv.device
    if dt == torch.bfloat16 and dh == 64 and qkv.is_contiguous() and cls_mask is None:
        # fused path: scores and probabilities stay on chip (csrc/vit.hip attention_fused_kernel)
        out = torch.empty((B, L, D), dtype=dt, device=dev)
        lib().call("egm_attention_fused", dtype_code(dt), ptr(qkv), D3, B, L, n_heads, dh, {"full": 0, "causal": 1, "csa": 2}[mode], ptr(out), D,
                   stream())
        return out
    S = torch.empty((B * n_heads, L, Lp), dtype=torch.float32, device=dev)
    P = torch.empty((B * n_heads, L, Lp), dtype=dt, device=dev)
    scale = dh ** -0.5
    L_, code = lib(), dtype_code(dt)

    def scores(off_a, off_b):
        gemm(qkv, D3, qkv, D3, True, S, Lp, L, L, dh, dt, alpha=scale, c_f32=True, nb1=B, nb2=n_heads, sA=(L * D3, dh), sB=(L * D3, dh),
             sC=(n_heads * L * Lp, L * Lp), offA=off_a, offB=off_b)

    if mode == "csa":
        scores(0, 0)
        L_.call("egm_softmax_rows", code, ptr(S), Lp, ptr(P), Lp, B * n_heads * L, L, 0, 0, stream())
        scores(D, D)
        L_.call("egm_softmax_rows", code, ptr(S), Lp, ptr(P), Lp, B * n_heads * L, L, 0, 1, stream())
    else:
        scores(0, D)
        L_.call("egm_softmax_rows", code, ptr(S), Lp, ptr(P), Lp, B * n_heads * L, L, 1 if mode == "causal" else 0, 0, stream())
    if cls_mask is not None:
        m = cls_mask.float().contiguous()
        if m.shape[1] != L - 1:
            raise RuntimeError(f"attention: class-token mask has {m.shape[1]} entries, the sequence {L - 1} patch tokens")
        L_.call("egm_attn_mask_cls", code, ptr(P), Lp, L * Lp, ptr(m), m.shape[0], B * n_heads, L - 1, stream())
    out = torch.empty((B, L, D), dtype=dt, device=dev)
    gemm(P, Lp, qkv, D3, False, out, D, L, dh, L, dt, nb1=B, nb2=n_heads, sA=(n_heads * L * Lp, L * Lp), sB=(L * D3, dh), sC=(L * D, dh), offB=2 * D)
    return out


_refine_cache = {}
REFINE_PATCH = 16


def refine_packed(w0, w1, w2, dtype):
    """The refined head's three weights (Conv2d [rd,rd,3,3], ConvTranspose2d [rd,rd/2,4,4], [rd/2,1,4,4]) in the operand layouts of
    csrc/clipseg_refine.hip, in the activation dtype; cached like cast_weight (parameter storage + version + cast generation)."""
    rd = w0.shape[0]
    slot = tuple(id(w) for w in (w0, w1, w2))
    key = tuple((w.data_ptr(), w._version) for w in (w0, w1, w2)) + (_cast_generation[0], dtype)
    hit = _refine_cache.get((slot, dtype))
    if hit is not None and hit[0] == key:
        return hit[1]
    n = lib().query("egm_refine_packed_elems", rd, REFINE_PATCH)
    out = torch.empty(n, dtype=dtype, device=w0.device)
    src = [w.detach().float().contiguous() for w in (w0, w1, w2)]
    lib().call("egm_refine_pack", dtype_code(dtype), ptr(src[0]), ptr(src[1]), ptr(src[2]), ptr(out), rd, REFINE_PATCH, stream())
    _refine_cache[(slot, dtype)] = (key, out)
    return out


def refine_head(a, w0, b0, w1, b1, w2, b2, tok_off=1, h=None):
    """complex_trans_conv head (models/clipseg.py:405-411) on a [B, Ltot, rd] (tok_off leading tokens skipped) -> fp32 [B, 1, 16g, 16g].
    h: optional [B, g*g, rd] tensor in a's dtype that receives the first ReLU's output (kept by the training backward)."""
    B, Ltot, rd = a.shape
    g = int(math.isqrt(Ltot - tok_off))
    if g * g != Ltot - tok_off:
        raise RuntimeError(f"refine_head: {Ltot - tok_off} grid tokens do not form a square grid")
    a = a.contiguous()
    pk = refine_packed(w0, w1, w2, a.dtype)
    out = torch.empty((B, 1, g * REFINE_PATCH, g * REFINE_PATCH), dtype=torch.float32, device=a.device)
    lib().call("egm_refine_fwd", dtype_code(a.dtype), ptr(a), tok_off, Ltot, ptr(pk), ptr(b0.detach().float().contiguous()),
               ptr(b1.detach().float().contiguous()), ptr(b2.detach().float().contiguous()), ptr(h), ptr(out), B, g, rd, REFINE_PATCH, stream())
    return out


_baseline_cache = {}
BASELINE_PATCH = 16


def baseline_supported(rd, rd2, patch, dtype):
    """True when csrc/clipseg_baseline.hip takes the shape (patch 16, rd / rd2 multiples of 16 up to 128) in this dtype (bf16)."""
    return dtype == torch.bfloat16 and lib().cdll.egm_baseline_supported(rd, rd2, patch) == 1


def baseline_packed(w_red, w1, w2, wt):
    """CLIPDenseBaseline's four head weights (reduce [rd,768], reduce2.0 [rd2,rd], reduce2.2 [rd,rd2], trans_conv [rd,1,16,16]) in the bf16
    operand layouts of csrc/clipseg_baseline.hip; cached like cast_weight (parameter storage + version + cast generation)."""
    ws = (w_red, w1, w2, wt)
    slot = tuple(id(w) for w in ws)
    key = tuple((w.data_ptr(), w._version) for w in ws) + (_cast_generation[0],)
    hit = _baseline_cache.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    rd, rd2 = w_red.shape[0], w1.shape[0]
    out = torch.empty(lib().query("egm_baseline_packed_elems", rd, rd2, BASELINE_PATCH), dtype=torch.bfloat16, device=w_red.device)
    src = [w.detach().float().contiguous() for w in ws]
    lib().call("egm_baseline_pack", dtype_code(torch.bfloat16), ptr(src[0]), ptr(src[1]), ptr(src[2]), ptr(src[3]), ptr(out), rd, rd2,
               BASELINE_PATCH, stream())
    _baseline_cache[slot] = (key, out)
    return out


def _baseline_fwd(multi, x, mul, add, w_red, b_red, w1, b1, w2, b2, wt, bt, tok_off, u, h, prompts_per_group):
    """The two forward entries of csrc/clipseg_baseline.hip behind baseline_head (multi = False) and baseline_head_multi."""
    B, Ltot, _ = x.shape
    K = mul.shape[0] if multi else 1
    g = int(math.isqrt(Ltot - tok_off))
    if g * g != Ltot - tok_off:
        raise RuntimeError(f"baseline_head{'_multi' if multi else ''}: {Ltot - tok_off} grid tokens do not form a square grid")
    x = x.contiguous()
    pk = baseline_packed(w_red, w1, w2, wt)
    out = torch.empty((B, K, g * BASELINE_PATCH, g * BASELINE_PATCH), dtype=torch.float32, device=x.device)
    f32 = [t.detach().float().contiguous() for t in (b_red, b1, b2, bt)]
    mul, add = mul.contiguous(), add.contiguous()
    tail = (ptr(out), B, K, g, w_red.shape[0], w1.shape[0], BASELINE_PATCH, int(prompts_per_group)) if multi else \
        (ptr(u), ptr(h), ptr(out), B, g, w_red.shape[0], w1.shape[0], BASELINE_PATCH)
    lib().call("egm_baseline_fwd_multi" if multi else "egm_baseline_fwd", dtype_code(x.dtype), ptr(x), tok_off, Ltot, ptr(mul), ptr(add), ptr(pk),
               ptr(f32[0]), ptr(f32[1]), ptr(f32[2]), ptr(f32[3]), *tail, stream())
    return out


def baseline_head(x, mul, add, w_red, b_red, w1, b1, w2, b2, wt, bt, tok_off=1, u=None, h=None):
    """CLIPDenseBaseline's head (models/clipseg.py:567-583) as ONE launch: x [B, Ltot, 768] bf16 (tok_off leading tokens skipped),
    mul / add [B, rd] bf16 (film_mul / film_add of the conditional) -> fp32 [B, 1, 16g, 16g].  u [B, g*g, rd] / h [B, g*g, rd2] (bf16,
    both or neither) receive reduce's output and the ReLU output for the training backward."""
    return _baseline_fwd(False, x, mul, add, w_red, b_red, w1, b1, w2, b2, wt, bt, tok_off, u, h, 0)


def baseline_head_multi(x, mul, add, w_red, b_red, w1, b1, w2, b2, wt, bt, tok_off=1, prompts_per_group=0):
    """baseline_head for K prompts on each of B activations, ONE launch: x [B, Ltot, 768] bf16, mul / add [K, rd] bf16 -> fp32
    [B, K, 16g, 16g] (out[b, k] = baseline_head(x[b:b+1], mul[k:k+1], add[k:k+1])[0, 0], bit for bit).  reduce runs once per token
    tile and prompt group; prompts_per_group <= 0 lets the library choose the groups."""
    return _baseline_fwd(True, x, mul, add, w_red, b_red, w1, b1, w2, b2, wt, bt, tok_off, None, None, prompts_per_group)


def film_fanout(r, mul, add):
    """FiLM at the decoder's cond_layer for K prompts: r [B, L, D], mul / add [K, D] (r's dtype) -> [B*K, L, D] with
    out[b*K + k] = mul[k] * r[b] + add[k] (sequence order b-major)."""
    B, L, D = r.shape
    K = mul.shape[0]
    r, mul, add = r.contiguous(), mul.contiguous(), add.contiguous()
    out = torch.empty((B * K, L, D), dtype=r.dtype, device=r.device)
    lib().call("egm_film_fanout", dtype_code(r.dtype), ptr(r), ptr(mul), ptr(add), ptr(out), B, K, L, D, stream())
    return out


def bcast_add_(a, r):
    """a [B*K, L, D] += r [B, L, D] broadcast over the K prompts of each image (in place; returns a)."""
    B, L, D = r.shape
    K = a.shape[0] // B
    if a.shape != (B * K, L, D) or not a.is_contiguous():
        raise RuntimeError(f"bcast_add_: a {tuple(a.shape)} is not a contiguous [B*K, L, D] for r {tuple(r.shape)}")
    r = r.contiguous()
    lib().call("egm_bcast_add", dtype_code(a.dtype), ptr(a), ptr(r), B, K, L, D, stream())
    return a


def bcast_add(a, r):
    """a [B*K, L, D] + r [B, L, D] broadcast over the K prompts of each image -> a new [B*K, L, D] (bcast_add_ out of place, same bits)."""
    B, L, D = r.shape
    K = a.shape[0] // B
    if a.shape != (B * K, L, D):
        raise RuntimeError(f"bcast_add: a {tuple(a.shape)} is not [B*K, L, D] for r {tuple(r.shape)}")
    a, r = a.contiguous(), r.contiguous()
    out = torch.empty_like(a)
    lib().call("egm_bcast_add_out", dtype_code(a.dtype), ptr(a), ptr(r), ptr(out), B, K, L, D, stream())
    return out


def sigmoid_affine_(x, scale, offset):
    """x fp32 [N, C, H, W] <- offset + scale[c] * sigmoid(x) in place (scale fp32 [C] on x's device); returns x."""
    N, C, H, W = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous() or scale.shape != (C,):
        raise RuntimeError("sigmoid_affine_: x must be contiguous fp32 [N, C, H, W] and scale [C]")
    lib().call("egm_sigmoid_affine", ptr(x), ptr(scale.float().contiguous()), float(offset), N, C, H * W, stream())
    return x


def trans_conv(a, weight, bias):
    """ConvTranspose2d(rd -> 1, P, stride P) on a [B, 1 + g*g, rd] (token 0 dropped) as a per-token GEMM + pixel shuffle -> fp32 NCHW."""
    bs, Ltot, rd = a.shape
    P, dt, dev = weight.shape[-1], a.dtype, a.device
    g = int(math.isqrt(Ltot - 1))
    y = torch.empty((bs * Ltot, P * P), dtype=dt, device=dev)          # per-token rd -> P x P patch (ConvTranspose2d as a GEMM)
    gemm(a.reshape(-1, rd), rd, cast_weight(weight.reshape(rd, P * P), dt), P * P, False, y, P * P, bs * Ltot, P * P, rd, dt)
    out = torch.empty((bs, 1, g * P, g * P), dtype=torch.float32, device=dev)
    lib().call("egm_pixel_shuffle", dtype_code(dt), ptr(y), P * P, 1, Ltot, ptr(bias.detach().float()), ptr(out), bs, g, P, stream())
    return out


# ---- the decoder's operator set, inference form (clip/train_ops.DECODER is the autograd form: same names, same positional parameters;
# clipseg.py's one decode loop per model class runs on either).  p is the dropout probability: 0 here.
def _no_dropout(p):
    if p:
        raise RuntimeError(f"the inference operators have no dropout (p = {p})")


def _self_attention(qkv, n_heads, p_drop):
    _no_dropout(p_drop)
    return attention(qkv, n_heads, "full")


def _linear_dropout(x, weight, bias, p, act=0, residual=None):
    """residual + dropout(act(linear(x)), p)"""
    _no_dropout(p)
    return linear(x, weight, bias, act=act, residual=residual)


def _film_(a, mul, add):
    """a [B, L, D] <- mul[b] * a + add[b] in place; returns a."""
    lib().call("egm_film", dtype_code(a.dtype), ptr(a), ptr(mul), ptr(add), a.shape[0], a.shape[1], a.shape[2], stream())
    return a


def _refine_seq(a, seq):
    """refine_head over the reference's nn.Sequential(Conv2d, ReLU, ConvTranspose2d, ReLU, ConvTranspose2d)."""
    return refine_head(a, seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias)


def _baseline_fused(x, mul, add, reduce, reduce2, trans_conv, fan):
    """The fused baseline head over the reference's modules; fan: mul / add hold K prompts for every image (-> [B, K, 16g, 16g])."""
    return (baseline_head_multi if fan else baseline_head)(x, mul, add, reduce.weight, reduce.bias, reduce2[0].weight, reduce2[0].bias,
                                                           reduce2[2].weight, reduce2[2].bias, trans_conv.weight, trans_conv.bias)


DECODER = SimpleNamespace(training=False, linear=linear, layernorm=layernorm, self_attention=_self_attention, linear_dropout=_linear_dropout,
                          film=_film_, film_fan=film_fanout, add_fan=bcast_add_, trans_conv=trans_conv, refine=_refine_seq,
                          baseline_fused=_baseline_fused)
