"""Tensor-level wrappers over the C ABI (include/pclip.h).  PyTorch is used only to own device memory
and streams; every arithmetic step below is a libpclip kernel.  All functions require CUDA (ROCm)
tensors and raise PclipError otherwise — there is deliberately no CPU path."""
import contextvars
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_cuda, stream

_ws_cache = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Scratch for one call (the C ABI never allocates).  Outside graph capture: a grow-only buffer per (device, stream) — calls
    on one stream are ordered, so they can share it.  During a hipGraph capture nothing is cached: the buffer comes from the
    capture's private memory pool and must belong to THAT graph only (a cached pointer would be baked into later captures whose
    pool does not own it); torch's caching allocator reuses the block between the calls of one capture."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def evict_workspace(stream_obj):
    """Forget the scratch buffer cached for `stream_obj` (a torch.cuda.Stream that will not be used again)."""
    for key in [k for k in _ws_cache if k[1] == stream_obj.cuda_stream]:
        del _ws_cache[key]


def release_workspaces():
    """Drop the cached scratch buffers (e.g. after a warm-up on a side stream that will not be used again)."""
    _ws_cache.clear()


def _f16c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float16:
        raise _lib.PclipError(f"expected a float16 tensor, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def l2norm_rows(x: torch.Tensor, out: torch.Tensor = None, want_sq: bool = False):
    """r16(x / r16(||x||)) per row — utils.py:352, main.py:182-185, 408-409."""
    require_cuda(x)
    x = _f16c(x)
    R, D = x.shape
    y = torch.empty_like(x) if out is None else out
    sq = torch.empty(R, dtype=torch.float32, device=x.device) if want_sq else None
    check(_lib.load().pclip_l2norm_rows_f16(ptr(x), ptr(y), R, D, ptr(sq), stream()), "pclip_l2norm_rows_f16")
    return (y, sq) if want_sq else y


def row_sqnorm(x: torch.Tensor) -> torch.Tensor:
    require_cuda(x)
    x = _f16c(x)
    sq = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(_lib.load().pclip_row_sqnorm_f16(ptr(x), x.shape[0], x.shape[1], ptr(sq), stream()), "pclip_row_sqnorm_f16")
    return sq


def transpose(x: torch.Tensor) -> torch.Tensor:
    """Materialised fp16 transpose (bank layout [D, N*K] <-> [N*K, D], utils.py:320)."""
    require_cuda(x)
    x = _f16c(x)
    R, C = x.shape
    y = torch.empty(C, R, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_transpose_f16(ptr(x), R, C, ptr(y), stream()), "pclip_transpose_f16")
    return y


def proto_build(mem: torch.Tensor, N: int, K: int, per_shot_norm: bool = True, fp32_out: bool = False,
                want_sq: bool = False):
    """Prototype reduction (main.py:399-402 eval / 260-264 train / 173-176 zero-shot init).
    mem [N*K, D] fp16 -> proto [N, D] (fp16, or fp32 un-rounded for the train path)."""
    require_cuda(mem)
    mem = _f16c(mem)
    if mem.shape[0] != N * K:
        raise _lib.PclipError(f"memory bank has {mem.shape[0]} rows, expected N*K={N * K}")
    D = mem.shape[1]
    p16 = None if fp32_out else torch.empty(N, D, dtype=torch.float16, device=mem.device)
    p32 = torch.empty(N, D, dtype=torch.float32, device=mem.device) if fp32_out else None
    sq = torch.empty(N, dtype=torch.float32, device=mem.device) if want_sq else None
    check(_lib.load().pclip_proto_build_f16(ptr(mem), N, K, D, int(per_shot_norm), ptr(p16), ptr(p32), ptr(sq),
                                            stream()), "pclip_proto_build_f16")
    out = p32 if fp32_out else p16
    return (out, sq) if want_sq else out


def bank_reduce(feats: torch.Tensor, perm: torch.Tensor = None) -> torch.Tensor:
    """feats [A, R, D] fp16 -> normalise(r16(mean_A)) rows, optionally gathered by perm (utils.py:318-326)."""
    require_cuda(feats, perm)
    feats = _f16c(feats)
    A, R, D = feats.shape
    if perm is not None:
        perm = perm.to(torch.int32).contiguous()
    keys = torch.empty(R, D, dtype=torch.float16, device=feats.device)
    check(_lib.load().pclip_bank_reduce_f16(ptr(feats), A, R, D, ptr(perm), ptr(keys), stream()),
          "pclip_bank_reduce_f16")
    return keys


def partial_sums(mem: torch.Tensor, labels: torch.Tensor, N: int, per_shot_norm: bool = True):
    """This rank's fp32 per-class sums [N, D] + int32 counts [N] (labels must be non-decreasing)."""
    require_cuda(mem, labels)
    mem = _f16c(mem)
    labels = labels.to(torch.int32).contiguous()
    R, D = mem.shape
    sums = torch.empty(N, D, dtype=torch.float32, device=mem.device)
    counts = torch.empty(N, dtype=torch.int32, device=mem.device)
    check(_lib.load().pclip_partial_sums_f16(ptr(mem), ptr(labels), R, N, D, int(per_shot_norm), ptr(sums),
                                             ptr(counts), stream()), "pclip_partial_sums_f16")
    return sums, counts


def proto_finalize(sums: torch.Tensor, counts: torch.Tensor, fp32_out: bool = False, want_sq: bool = False):
    """sums [W, N, D] fp32, counts [W, N] int32 (rank-major) -> prototypes as proto_build."""
    require_cuda(sums, counts)
    if sums.dim() == 2:
        sums, counts = sums[None], counts[None]
    sums, counts = sums.contiguous(), counts.contiguous()
    W, N, D = sums.shape
    p16 = None if fp32_out else torch.empty(N, D, dtype=torch.float16, device=sums.device)
    p32 = torch.empty(N, D, dtype=torch.float32, device=sums.device) if fp32_out else None
    sq = torch.empty(N, dtype=torch.float32, device=sums.device) if want_sq else None
    check(_lib.load().pclip_proto_finalize(ptr(sums), ptr(counts), W, N, D, ptr(p16), ptr(p32), ptr(sq), stream()),
          "pclip_proto_finalize")
    out = p32 if fp32_out else p16
    return (out, sq) if want_sq else out


def padded_ld(N: int) -> int:
    return (N + 63) // 64 * 64


def sqdist(q: torch.Tensor, zi: torch.Tensor, zt: torch.Tensor = None, q_sq=None, zi_sq=None, zt_sq=None):
    """Squared distances of fp16 queries to both prototype banks: fp32 [Q, ldd] each (cdist(...)**2 of
    utils.py:230-233).  Returns (d2i, d2t, ldd); columns >= N are unspecified padding."""
    require_cuda(q, zi, zt)
    q, zi = _f16c(q), _f16c(zi)
    zt = None if zt is None else _f16c(zt)
    Q, D = q.shape
    N = zi.shape[0]
    ldd = padded_ld(N)
    d2i = torch.empty(Q, ldd, dtype=torch.float32, device=q.device)
    d2t = torch.empty(Q, ldd, dtype=torch.float32, device=q.device) if zt is not None else None
    nws = _lib.workspace_bytes(_lib.OP_SQDIST, Q, N, D)
    ws = _workspace(nws, q.device)
    check(_lib.load().pclip_sqdist_f16(ptr(q), ptr(zi), ptr(zt), Q, N, D, ptr(q_sq), ptr(zi_sq), ptr(zt_sq),
                                       ptr(d2i), ptr(d2t), ldd, ptr(ws), ws.numel(), stream()), "pclip_sqdist_f16")
    return d2i, d2t, ldd


def sqdist_f32(q: torch.Tensor, zi: torch.Tensor, zt: torch.Tensor = None):
    """fp32-operand squared distances (training path: fp32 prototypes / adapted queries, main.py:262-281)."""
    require_cuda(q, zi, zt)
    q, zi = q.float().contiguous(), zi.float().contiguous()
    zt = None if zt is None else zt.float().contiguous()
    Q, D = q.shape
    N = zi.shape[0]
    ldd = padded_ld(N)
    d2i = torch.empty(Q, ldd, dtype=torch.float32, device=q.device)
    d2t = torch.empty(Q, ldd, dtype=torch.float32, device=q.device) if zt is not None else None
    check(_lib.load().pclip_sqdist_f32(ptr(q), ptr(zi), ptr(zt), Q, N, D, ptr(d2i), ptr(d2t), ldd, stream()),
          "pclip_sqdist_f32")
    return d2i, d2t, ldd


def fuse_probs(d2i, d2t, N: int, alpha: float, beta: float, want_p=True, want_argmax=False, topk: int = 0):
    """alpha*softmax(-beta*d2i) + (1-alpha)*softmax(-beta*d2t) (utils.py:236-242) + argmax / top-k."""
    require_cuda(d2i, d2t)
    Q, ldd = d2i.shape
    dev = d2i.device
    p = torch.empty(Q, N, dtype=torch.float32, device=dev) if want_p else None
    am = torch.empty(Q, dtype=torch.int32, device=dev) if want_argmax else None
    tp = torch.empty(Q, topk, dtype=torch.float32, device=dev) if topk else None
    ti = torch.empty(Q, topk, dtype=torch.int32, device=dev) if topk else None
    # the reference forms (1 - alpha) in Python double precision and lets torch cast it to fp32
    a32, oma32 = float(np.float32(alpha)), float(np.float32(1 - float(alpha)))
    check(_lib.load().pclip_fuse_probs(ptr(d2i), ptr(d2t), Q, N, ldd, a32, oma32, float(np.float32(beta)), ptr(p),
                                       ptr(am), ptr(tp), ptr(ti), topk, stream()), "pclip_fuse_probs")
    return p, am, tp, ti


def classify(q, zi, zt, alpha: float, beta: float, want_p=False, want_argmax=True, topk: int = 0,
             q_sq=None, zi_sq=None, zt_sq=None):
    """One-call classification (sqdist + fuse) with distances kept in scratch."""
    require_cuda(q, zi, zt)
    q, zi, zt = _f16c(q), _f16c(zi), _f16c(zt)
    Q, D = q.shape
    N = zi.shape[0]
    dev = q.device
    p = torch.empty(Q, N, dtype=torch.float32, device=dev) if want_p else None
    am = torch.empty(Q, dtype=torch.int32, device=dev) if want_argmax else None
    tp = torch.empty(Q, topk, dtype=torch.float32, device=dev) if topk else None
    ti = torch.empty(Q, topk, dtype=torch.int32, device=dev) if topk else None
    # the library is told this shape's own workspace size, not the cached buffer's (which grows with whatever ran before on the stream): the route it
    # takes — the fused row panels only if their scratch fits in that size — is then a function of the shape and the context's routing flags alone, the one
    # `classify_route` reports
    nws = _lib.workspace_bytes(_lib.OP_CLASSIFY, Q, N, D)
    ws = _workspace(nws, dev)
    a32, oma32 = float(np.float32(alpha)), float(np.float32(1 - float(alpha)))
    check(_lib.load().pclip_classify_ex_f16(ptr(q), ptr(zi), ptr(zt), Q, N, D, ptr(q_sq), ptr(zi_sq), ptr(zt_sq), a32,
                                            oma32, float(np.float32(beta)), ptr(p), ptr(am), ptr(tp), ptr(ti), topk,
                                            _classify_flags.get(), ptr(ws), nws, stream()), "pclip_classify_ex_f16")
    return p, am, tp, ti


def proto_classify(mem, N: int, K: int, q, zt, alpha: float, beta: float, per_shot_norm: bool = True, want_p=False, want_argmax=True, topk: int = 0):
    """main.py:399-405 + utils.py:225-244 + main.py:190: prototypes from the memory bank and the classification of q against them.  Returns
    (z_img_proto [N, D] fp16, p, argmax, topk_p, topk_i): `proto_build` followed by `classify` (4.0 + 6.4 us at EuroSAT's size).  (A one-launch form — builder and
    consumer workgroups in one grid — was built in round 5 and measured SLOWER, 12.8 - 16.8 us: the cross-XCD hand-over of the prototype rows costs more than the
    launch it saves; removed in round 6, profiles/r05_c2_phases.txt.)"""
    require_cuda(mem, q, zt)
    mem, q, zt = _f16c(mem), _f16c(q), _f16c(zt)
    if mem.shape[0] != N * K:
        raise _lib.PclipError(f"memory bank has {mem.shape[0]} rows, expected N*K={N * K}")
    zi = proto_build(mem, N, K, per_shot_norm)
    return (zi,) + tuple(classify(q, zi, zt, alpha, beta, want_p=want_p, want_argmax=want_argmax, topk=topk))


def _f16_rows(t: torch.Tensor, what: str) -> torch.Tensor:
    """A 2-D fp16 operand whose rows may be strided (a column slice of a wider buffer): taken as it is when the kernel can address it
    (unit column stride, row stride a multiple of 8 halves, 16-byte aligned), copied otherwise."""
    if t.dtype != torch.float16:
        raise _lib.PclipError(f"{what}: expected a float16 tensor, got {t.dtype}")
    if t.dim() != 2:
        raise _lib.PclipError(f"{what}: expected a 2-D tensor, got shape {tuple(t.shape)}")
    bad_cols = t.shape[1] > 1 and t.stride(1) != 1
    bad_rows = t.shape[0] > 1 and (t.stride(0) < t.shape[1] or t.stride(0) % 8)                      # (a single row has no row stride to speak of)
    if bad_cols or bad_rows or t.data_ptr() % 16:
        return t.clone(memory_format=torch.contiguous_format)                                       # (.contiguous() would hand a dense but misaligned view back)
    return t


def cosine_logits(a, b, scale: float, normalize_a: bool = False, normalize_b: bool = False, want_logits: bool = True,
                  want_argmax: bool = False, topk: int = 0, out: torch.Tensor = None):
    """logits[m, t] = r16(sum_d r16(scale * a'[m, d]) * b'[t, d]) — clip/model.py:359-367 and the zero-shot `100. * features @ clip_weights`.
    a [M, D], b [T, D] fp16 (row-strided views are read in place); a' / b' are the rows, L2-normalised as `l2norm_rows` does when asked.  `scale` is applied
    in fp32 as given (CLIP.forward passes the fp16-rounded logit scale, as the reference's arithmetic does).  Returns (logits [M, T] fp16 | None,
    argmax [M] int32 | None, topk_v [M, k] fp16 | None, topk_i [M, k] int32 | None); without `want_logits` the matrix is never written.
    out: optional [M, >= T] fp16 buffer (row stride a multiple of 8) that receives the logits in its first T columns.
    The logits returned are the first T columns of the buffer the kernel wrote, whose row stride is T rounded up to 8 halves: a dense tensor when T % 8 == 0,
    a strided view otherwise (`CLIP.forward` and `utils.clip_logits` return `.contiguous()` of it)."""
    require_cuda(a, b, out)
    a, b = _f16_rows(a, "cosine_logits: a"), _f16_rows(b, "cosine_logits: b")
    (M, D), (T, Db) = a.shape, b.shape
    if D != Db:
        raise _lib.PclipError(f"cosine_logits: a has {D} columns, b has {Db}")
    if M < 1 or T < 1:
        raise _lib.PclipError(f"cosine_logits: empty operand (M={M}, T={T})")
    dev = a.device
    lda, ldb = (a.stride(0) if M > 1 else D), (b.stride(0) if T > 1 else D)
    logits, ldl = None, 0
    if want_logits:
        if out is None:
            ldl = (T + 7) // 8 * 8
            out = torch.empty(M, ldl, dtype=torch.float16, device=dev)
        else:
            if out.dtype != torch.float16 or out.dim() != 2 or out.shape[0] != M or out.shape[1] < T or out.stride(1) != 1:
                raise _lib.PclipError(f"cosine_logits: out must be a float16 [M={M}, >= T={T}] tensor with unit column stride")
            ldl = out.stride(0) if M > 1 else (T + 7) // 8 * 8
        logits = out[:, :T]
    k = int(topk)
    am = torch.empty(M, dtype=torch.int32, device=dev) if want_argmax else None
    tv = torch.empty(M, k, dtype=torch.float16, device=dev) if k else None
    ti = torch.empty(M, k, dtype=torch.int32, device=dev) if k else None
    flags = (_lib.LOGITS_NORMALIZE_A if normalize_a else 0) | (_lib.LOGITS_NORMALIZE_B if normalize_b else 0)
    nws = _lib.workspace_bytes(_lib.OP_LOGITS, M, T, D) if normalize_b else 0
    ws = _workspace(nws, dev) if nws else None
    check(_lib.load().pclip_cosine_logits_f16(ptr(a), lda, M, ptr(b), ldb, T, D, float(np.float32(scale)), flags, ptr(out if want_logits else None), ldl,
                                              ptr(am), ptr(tv), ptr(ti), k, ptr(ws), nws, stream()), "pclip_cosine_logits_f16")
    return logits, am, tv, ti


def _cosine_ce_args(what, a, b, labels, symmetric, normalize_a, normalize_b):
    """The operands of the two cosine cross-entropy calls as the kernels take them: (a, b, lda, ldb, M, T, D, labels, flags)."""
    require_cuda(a, b, labels)
    a, b = _f16_rows(a, f"{what}: a"), _f16_rows(b, f"{what}: b")
    (M, D), (T, Db) = a.shape, b.shape
    if D != Db:
        raise _lib.PclipError(f"{what}: a has {D} columns, b has {Db}")
    if M < 1 or T < 1:
        raise _lib.PclipError(f"{what}: empty operand (M={M}, T={T})")
    flags = (_lib.CE_NORMALIZE_A if normalize_a else 0) | (_lib.CE_NORMALIZE_B if normalize_b else 0)
    if symmetric:
        if labels is not None:
            raise _lib.PclipError(f"{what}: symmetric mode takes no labels (the targets are the diagonal)")
        flags |= _lib.CE_SYMMETRIC
    else:
        if labels is None or labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1 or labels.shape[0] != M:
            raise _lib.PclipError(f"{what}: labels must be an int32 / int64 tensor of {M} entries (or symmetric=True)")
        labels = labels.contiguous()
        flags |= _lib.CE_LABELS_I64 if labels.dtype == torch.int64 else 0
    return a, b, (a.stride(0) if M > 1 else D), (b.stride(0) if T > 1 else D), M, T, D, labels, flags


def cosine_cross_entropy(a, b, scale: float, labels=None, symmetric: bool = False, normalize_a: bool = False, normalize_b: bool = False, want_rows: bool = False):
    """Cross-entropy over s = scale * a' @ b'^T without the [M, T] matrix (the logits of clip/model.py:356-370, for training): a [M, D], b [T, D] fp16,
    a' / b' the rows or their `l2norm_rows`; s stays fp32 — nothing is rounded to fp16 as the inference kernel `cosine_logits` does.
    labels [M] int32 / int64: loss = mean_m (lse_t s[m, :] - s[m, y_m]); a label outside [0, T) is never used as an index: its row's term is the lse alone.
    symmetric (M == T, no labels): CLIP's loss, 1/2 (mean of the row terms + mean of the column terms), targets on the diagonal.
    Returns (loss 0-dim fp32, lse_row [M] fp32, lse_col [T] fp32 | None), and the per-row loss terms [M] as a fourth value with `want_rows`."""
    a, b, lda, ldb, M, T, D, labels, flags = _cosine_ce_args("cosine_cross_entropy", a, b, labels, symmetric, normalize_a, normalize_b)
    dev = a.device
    lse_row = torch.empty(M, dtype=torch.float32, device=dev)
    lse_col = torch.empty(T, dtype=torch.float32, device=dev) if symmetric else None
    rows = torch.empty(M, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    nws = _lib.workspace_bytes(_lib.OP_COSINE_CE, M, T, D)
    ws = _workspace(nws, dev)
    check(_lib.load().pclip_cosine_ce_f16(ptr(a), lda, M, ptr(b), ldb, T, D, float(np.float32(scale)), flags, ptr(labels), ptr(lse_row), ptr(lse_col),
                                          ptr(rows), ptr(loss), ptr(ws), nws, stream()), "pclip_cosine_ce_f16")
    return (loss, lse_row, lse_col, rows) if want_rows else (loss, lse_row, lse_col)


def cosine_cross_entropy_backward(a, b, scale: float, lse_row, lse_col=None, labels=None, symmetric: bool = False, normalize_a: bool = False,
                                  normalize_b: bool = False, want_a: bool = True, want_b: bool = True, want_scale: bool = True, grad: float = 1.0,
                                  mean_over: int = None):
    """The gradients of `cosine_cross_entropy` from its lse vectors: (dL/da [M, D] fp32 | None, dL/db [T, D] fp32 | None, dL/dscale 0-dim fp32 | None).
    Logit tiles are recomputed and fed to a second matrix product; the exp tile is rounded to fp16 on the way, the weights and the scale act in fp32.
    With normalize_a / normalize_b the gradient is chained in fp32 through the normalisation (the fp16 rounding of the normalised rows taken as the identity).
    grad: the upstream gradient as a number; mean_over: the row count the loss was averaged over when the rows are a slice of a larger batch (default M) —
    in labelled mode a row of dL/da has the same bits in any batch with the same `grad / mean_over`."""
    a, b, lda, ldb, M, T, D, labels, flags = _cosine_ce_args("cosine_cross_entropy_backward", a, b, labels, symmetric, normalize_a, normalize_b)
    require_cuda(lse_row, lse_col)
    for name, t, n in (("lse_row", lse_row, M), ("lse_col", lse_col, T)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous()):
            raise _lib.PclipError(f"cosine_cross_entropy_backward: {name} must be a contiguous float32 tensor of {n} entries")
    if lse_row is None or (lse_col is None) == bool(symmetric):
        raise _lib.PclipError("cosine_cross_entropy_backward: lse_row is required, lse_col goes with symmetric mode and only with it")
    dev = a.device
    weight = float(grad) / ((mean_over or M) * (2 if symmetric else 1))
    nws = _lib.workspace_bytes(_lib.OP_COSINE_CE_BACKWARD, M, T, D)
    ws = _workspace(nws, dev)
    ds = torch.empty((), dtype=torch.float32, device=dev) if want_scale else None
    walks = [(0, M, want_a or (want_scale and not want_b)), (1, T, want_b)]          # (dscale is a by-product of a gradient walk: of dL/da's if no other runs)
    grads, ds_left = [], ds
    for direction, rows, run in walks:
        if not run:
            grads.append(None)
            continue
        g = torch.empty(rows, D, dtype=torch.float32, device=dev)
        check(_lib.load().pclip_cosine_ce_backward_f16(ptr(a), lda, M, ptr(b), ldb, T, D, float(np.float32(scale)), flags, ptr(labels), ptr(lse_row), ptr(lse_col),
                                                       float(np.float32(weight)), direction, ptr(g), ptr(ds_left), ptr(ws), nws, stream()),
              "pclip_cosine_ce_backward_f16")
        ds_left = None
        grads.append(g)
    return (grads[0] if want_a else None), grads[1], ds


def _cosine_kd_args(what, a, b, scale, ta, tb, tscale, normalize_a, normalize_b, normalize_ta, normalize_tb):
    """The operands of the two distillation calls as the kernels take them: (a, lda, b, ldb, ta, ldta, tb, ldtb, M, T, D, Dt, scale, tscale, flags).
    A teacher operand that IS the student's tensor stays that tensor (one checked copy at the most)."""
    require_cuda(a, b, ta, tb)
    same_a, same_b = ta is a, tb is b
    a, b = _f16_rows(a, f"{what}: a"), _f16_rows(b, f"{what}: b")
    ta = a if same_a else _f16_rows(ta, f"{what}: ta")
    tb = b if same_b else _f16_rows(tb, f"{what}: tb")
    (M, D), (T, Db), (Mt, Dt), (Tt, Dtb) = a.shape, b.shape, ta.shape, tb.shape
    if D != Db:
        raise _lib.PclipError(f"{what}: a has {D} columns, b has {Db}")
    if Dt != Dtb:
        raise _lib.PclipError(f"{what}: ta has {Dt} columns, tb has {Dtb}")
    if M < 1 or T < 1:
        raise _lib.PclipError(f"{what}: empty operand (M={M}, T={T})")
    if Mt != M or Tt != T:
        raise _lib.PclipError(f"{what}: the teacher's logits are [{Mt}, {Tt}], the student's [{M}, {T}]")
    scale, tscale = float(np.float32(scale)), float(np.float32(tscale))
    if not (np.isfinite(scale) and np.isfinite(tscale)):
        raise _lib.PclipError(f"{what}: scale={scale} and tscale={tscale} must be finite")
    flags = (_lib.KD_NORMALIZE_A if normalize_a else 0) | (_lib.KD_NORMALIZE_B if normalize_b else 0)
    flags |= (_lib.KD_NORMALIZE_TA if normalize_ta else 0) | (_lib.KD_NORMALIZE_TB if normalize_tb else 0)
    ld = lambda t, rows, cols: t.stride(0) if rows > 1 else cols
    return a, ld(a, M, D), b, ld(b, T, D), ta, ld(ta, M, Dt), tb, ld(tb, T, Dt), M, T, D, Dt, scale, tscale, flags


def cosine_kd(a, b, scale: float, ta, tb, tscale: float, normalize_a: bool = False, normalize_b: bool = False, normalize_ta: bool = False,
              normalize_tb: bool = False, want_rows: bool = False):
    """Distillation loss over cosine logits without either [M, T] matrix (pclip_cosine_kd_f16): the student's s = scale * a' @ b'^T (a [M, D], b [T, D] fp16)
    against the teacher's z = tscale * ta' @ tb'^T (ta [M, Dt], tb [T, Dt] fp16, its own width and normalise flags; `ta is a` / `tb is b` are the common case).
    loss = mean_m KL(softmax z[m, :] || softmax s[m, :]), in fp32 from unrounded logits; it is not clamped at zero (teacher == student gives a value within
    a few units of its rounding error of 0, on either side).  A temperature is the caller's: divide both scales by it (autograd.cosine_kd does).
    Returns (loss 0-dim fp32, lse_row [M] fp32, tlse_row [M] fp32) — the lse vectors have the bits of `cosine_cross_entropy`'s on the same operands —
    and the per-row terms [M] as a fourth value with `want_rows`."""
    a, lda, b, ldb, ta, ldta, tb, ldtb, M, T, D, Dt, scale, tscale, flags = _cosine_kd_args("cosine_kd", a, b, scale, ta, tb, tscale, normalize_a, normalize_b,
                                                                                           normalize_ta, normalize_tb)
    dev = a.device
    lse_row = torch.empty(M, dtype=torch.float32, device=dev)
    tlse_row = torch.empty(M, dtype=torch.float32, device=dev)
    rows = torch.empty(M, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    nws = _lib.workspace_bytes(_lib.OP_COSINE_KD, M, T, max(D, Dt))
    ws = _workspace(nws, dev)
    check(_lib.load().pclip_cosine_kd_f16(ptr(a), lda, M, ptr(b), ldb, T, D, scale, ptr(ta), ldta, ptr(tb), ldtb, Dt, tscale, flags, ptr(lse_row), ptr(tlse_row),
                                          ptr(rows), ptr(loss), ptr(ws), nws, stream()), "pclip_cosine_kd_f16")
    return (loss, lse_row, tlse_row, rows) if want_rows else (loss, lse_row, tlse_row)


def cosine_kd_backward(a, b, scale: float, ta, tb, tscale: float, lse_row, tlse_row, normalize_a: bool = False, normalize_b: bool = False,
                       normalize_ta: bool = False, normalize_tb: bool = False, want_a: bool = True, want_b: bool = True, want_scale: bool = True,
                       grad: float = 1.0, mean_over: int = None):
    """The student's gradients of `cosine_kd` from its two lse vectors: (dL/da [M, D] fp32 | None, dL/db [T, D] fp32 | None, dL/dscale 0-dim fp32 | None);
    the teacher receives none.  Logit tiles of both are recomputed; the signed tile softmax(s) - softmax(z) enters the second matrix product rounded to
    fp16 as 2^14 times itself, the weight and the scale act in fp32; under normalize_a / normalize_b the gradient is chained in fp32 through the
    normalisation.  grad: the upstream gradient (and a temperature's square) as a number; mean_over: the row count of the mean (default M) — a row of
    dL/da has the same bits in any batch with the same `grad / mean_over`."""
    what = "cosine_kd_backward"
    a, lda, b, ldb, ta, ldta, tb, ldtb, M, T, D, Dt, scale, tscale, flags = _cosine_kd_args(what, a, b, scale, ta, tb, tscale, normalize_a, normalize_b,
                                                                                           normalize_ta, normalize_tb)
    require_cuda(lse_row, tlse_row)
    for name, t in (("lse_row", lse_row), ("tlse_row", tlse_row)):
        if t is None or t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != M or not t.is_contiguous():
            raise _lib.PclipError(f"{what}: {name} must be a contiguous float32 tensor of {M} entries")
    dev = a.device
    weight = float(grad) / (mean_over or M)
    nws = _lib.workspace_bytes(_lib.OP_COSINE_KD_BACKWARD, M, T, max(D, Dt))
    ws = _workspace(nws, dev)
    ds = torch.empty((), dtype=torch.float32, device=dev) if want_scale else None
    walks = [(0, M, want_a or (want_scale and not want_b)), (1, T, want_b)]          # (dscale is a by-product of a gradient walk: of dL/da's if no other runs)
    grads, ds_left = [], ds
    for direction, rows, run in walks:
        if not run:
            grads.append(None)
            continue
        g = torch.empty(rows, D, dtype=torch.float32, device=dev)
        check(_lib.load().pclip_cosine_kd_backward_f16(ptr(a), lda, M, ptr(b), ldb, T, D, scale, ptr(ta), ldta, ptr(tb), ldtb, Dt, tscale, flags, ptr(lse_row),
                                                       ptr(tlse_row), float(np.float32(weight)), direction, ptr(g), ptr(ds_left), ptr(ws), nws, stream()),
              "pclip_cosine_kd_backward_f16")
        ds_left = None
        grads.append(g)
    return (grads[0] if want_a else None), grads[1], ds


_FREG_MODES = {"l1": _lib.FREG_L1, "cos": _lib.FREG_COS, "cosine": _lib.FREG_COS}


def _feature_reg_args(what, x, t, mode, normalize_t):
    """The operands of the two feature-regulariser calls as the kernels take them: (x, ldx, t, ldt, M, D, mode, normalize_t).  Refusals come before any
    launch; an operand the kernel cannot address in place (a misaligned or oddly strided view) is copied once."""
    if not isinstance(mode, str) or mode not in _FREG_MODES:
        raise _lib.PclipError(f"{what}: mode={mode!r} is neither 'l1' nor 'cos'")
    for name, v in (("x", x), ("t", t)):
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float16 or v.dim() != 2:
            raise _lib.PclipError(f"{what}: {name} must be a 2-D float16 tensor, got {getattr(v, 'dtype', type(v))} {tuple(getattr(v, 'shape', ()))}")
    if x.shape != t.shape:
        raise _lib.PclipError(f"{what}: x is {tuple(x.shape)}, the target {tuple(t.shape)}")
    M, D = x.shape
    if D % 8 or not 8 <= D <= 4096:
        raise _lib.PclipError(f"{what}: D={D} must be a multiple of 8 in 8..4096")
    require_cuda(x, t)
    x, t = _f16_rows(x, f"{what}: x"), _f16_rows(t, f"{what}: t")
    return x, (x.stride(0) if M > 1 else D), t, (t.stride(0) if M > 1 else D), M, D, _FREG_MODES[mode], 1 if normalize_t else 0


def feature_reg(x, t, mode: str = "l1", normalize_t: bool = False, want_rows: bool = False):
    """The distance of the L2-normalised rows of x [M, D] fp16 (a tower's un-normalised output) from the constant t [M, D] fp16 — as it is, or normalised as x
    is with `normalize_t` — in one row pass (pclip_feature_reg_f16); row-strided views are read in place.
      mode "l1":  F.l1_loss(x / x.norm(dim=-1, keepdim=True), t', reduction="mean")       PromptSRC's feature regularisers
      mode "cos": 1 - F.cosine_similarity(x, t', dim=-1).mean()                           KgCoOp's
    The normalised rows stay fp32 (torch on fp16 tensors rounds them to fp16 before the loss).  A zero row of x gives NaN, in its own term and the loss only.
    Returns (loss 0-dim fp32, inv_norm [M] fp32 = 1 / ||x_m||), and the per-row terms [M] fp32 as a third value with `want_rows`.  M == 0: +0, no launch."""
    x, ldx, t, ldt, M, D, mode, nt = _feature_reg_args("feature_reg", x, t, mode, normalize_t)
    dev = x.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    rows = torch.empty(M, dtype=torch.float32, device=dev)
    inv = torch.empty(M, dtype=torch.float32, device=dev)
    nws = int(_lib.load().pclip_feature_reg_workspace(M))
    ws = _workspace(nws, dev) if nws else None
    check(_lib.load().pclip_feature_reg_f16(ptr(x), ldx, ptr(t), ldt, M, D, mode, nt, ptr(loss), ptr(rows), ptr(inv), ptr(ws), nws, stream()),
          "pclip_feature_reg_f16")
    return (loss, inv, rows) if want_rows else (loss, inv)


def feature_reg_backward(x, t, inv_norm, mode: str, normalize_t: bool, grad: float = 1.0, mean_over: int = None):
    """The gradient of `feature_reg` with respect to x: [M, D] fp32 (the target is a constant).  dn = w sgn(n - t') with sgn(0) = 0 ("l1", w = grad /
    (mean_over D)) or -w t' ("cos", w = grad / mean_over), dx = (dn - n (n . dn)) / ||x||, all fp32; n and t' are recomputed from x and t by the forward's
    instruction sequence.  inv_norm: the forward's [M] vector — it identifies the forward this belongs to and is checked, the kernel recomputes its bits.
    grad: the upstream gradient as a number; mean_over: the row count of the mean (default M) — a row of dx has the same bits in any batch with the same
    grad / mean_over."""
    what = "feature_reg_backward"
    x, ldx, t, ldt, M, D, mode, nt = _feature_reg_args(what, x, t, mode, normalize_t)
    if not isinstance(inv_norm, torch.Tensor) or inv_norm.dtype != torch.float32 or inv_norm.dim() != 1 or inv_norm.shape[0] != M:
        raise _lib.PclipError(f"{what}: inv_norm must be the forward's float32 vector of {M} entries")
    require_cuda(x, inv_norm)
    over = M if mean_over is None else int(mean_over)
    if over < 1 and M > 0:
        raise _lib.PclipError(f"{what}: mean_over={mean_over} must be positive")
    dx = torch.empty(M, D, dtype=torch.float32, device=x.device)
    if M == 0:
        return dx
    weight = float(grad) / (over * D if mode == _lib.FREG_L1 else over)
    check(_lib.load().pclip_feature_reg_backward_f16(ptr(x), ldx, ptr(t), ldt, M, D, mode, nt, float(np.float32(weight)), ptr(dx), stream()),
          "pclip_feature_reg_backward_f16")
    return dx


def _f16_groups(t: torch.Tensor, what: str):
    """A checked 3-D fp16 device operand [G, R, D] as the grouped kernels address it: (tensor, row pitch, group stride) in halves.  Taken as it is — a view
    into a larger buffer included — when the kernel can address it (unit stride along D, row pitch >= D and group stride multiples of 8 halves, 16-byte
    aligned), copied otherwise."""
    G, R, D = t.shape
    bad_cols = D > 1 and t.stride(2) != 1
    bad_rows = R > 1 and (t.stride(1) < D or t.stride(1) % 8)
    bad_groups = G > 1 and t.stride(0) % 8
    if bad_cols or bad_rows or bad_groups or t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t, (t.stride(1) if R > 1 else D), (t.stride(0) if G > 1 else R * D)


def _cosine_ce_grouped_args(what, a, b, labels, normalize_a, normalize_b):
    """The operands of the two grouped cosine cross-entropy calls as the kernels take them: (a, lda, gsa, b, ldb, gsb, G, M, T, D, labels, flags).
    Types and shapes are checked first, each refusal naming its argument, then the device."""
    if isinstance(a, torch.Tensor) and a.dim() == 2:
        a = a.unsqueeze(1)                                                                          # [G, D]: one row per group
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float16:
            raise _lib.PclipError(f"{what}: {name}: expected a float16 tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 3 or min(t.shape) < 1:
            raise _lib.PclipError(f"{what}: {name}: expected a non-empty 3-D tensor [G, rows, D], got shape {tuple(t.shape)}")
    (G, M, D), (Gb, T, Db) = a.shape, b.shape
    if G != Gb:
        raise _lib.PclipError(f"{what}: a has {G} groups, b has {Gb}")
    if D != Db:
        raise _lib.PclipError(f"{what}: a has {D} columns, b has {Db}")
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int32, torch.int64) or tuple(labels.shape) not in ((G, M),) + (((G,),) if M == 1 else ()):
        raise _lib.PclipError(f"{what}: labels must be an int32 / int64 tensor of shape [G={G}, M={M}], got {getattr(labels, 'dtype', None)} "
                              f"{tuple(getattr(labels, 'shape', ()))}")
    for name, t in (("a", a), ("b", b), ("labels", labels)):
        if not t.is_cuda:
            raise _lib.PclipError(f"{what}: {name}: expected a device tensor, got a CPU tensor (libpclip has no CPU fallback)")
    require_cuda(a, b, labels)
    a, lda, gsa = _f16_groups(a, f"{what}: a")
    b, ldb, gsb = _f16_groups(b, f"{what}: b")
    flags = (_lib.CE_NORMALIZE_A if normalize_a else 0) | (_lib.CE_NORMALIZE_B if normalize_b else 0)
    flags |= _lib.CE_LABELS_I64 if labels.dtype == torch.int64 else 0
    return a, lda, gsa, b, ldb, gsb, G, M, T, D, labels.contiguous(), flags


def cosine_cross_entropy_grouped(a, b, scale: float, labels, normalize_a: bool = False, normalize_b: bool = False):
    """G independent labelled `cosine_cross_entropy` problems of one shape in one call (pclip_cosine_ce_grouped_f16): a [G, M, D] (or [G, D]: M = 1),
    b [G, T, D] fp16, labels [G, M] int32 / int64 indexing the rows of the group's own b[g].  Group and row strides are taken from the tensors: a view into
    a larger buffer is read in place.  Returns (loss [G] fp32 — loss[g] the mean of group g's M terms —, lse_row [G, M] fp32, rows [G, M] fp32, the terms).
    Group g's numbers are the bits of `cosine_cross_entropy(a[g], b[g], scale, labels[g], ...)`; the number of launches does not depend on G."""
    a, lda, gsa, b, ldb, gsb, G, M, T, D, labels, flags = _cosine_ce_grouped_args("cosine_cross_entropy_grouped", a, b, labels, normalize_a, normalize_b)
    dev = a.device
    lse_row = torch.empty(G, M, dtype=torch.float32, device=dev)
    rows = torch.empty(G, M, dtype=torch.float32, device=dev)
    loss = torch.empty(G, dtype=torch.float32, device=dev)
    lib = _lib.load()
    nws = int(lib.pclip_cosine_ce_grouped_workspace(0, G, M, T, D))
    ws = _workspace(nws, dev)
    check(lib.pclip_cosine_ce_grouped_f16(ptr(a), lda, gsa, M, ptr(b), ldb, gsb, T, D, G, float(np.float32(scale)), flags, ptr(labels), ptr(lse_row), ptr(rows),
                                          ptr(loss), ptr(ws), nws, stream()), "pclip_cosine_ce_grouped_f16")
    return loss, lse_row, rows


def cosine_cross_entropy_grouped_backward(a, b, scale: float, lse_row, labels, normalize_a: bool = False, normalize_b: bool = False, want_a: bool = True,
                                          want_b: bool = True, want_scale: bool = True, grad: float = 1.0, mean_over: int = None):
    """The gradients of `cosine_cross_entropy_grouped` from its lse rows, of every group's OWN loss: (dL_g/da [G, M, D] fp32 | None,
    dL_g/db [G, T, D] fp32 | None, dL_g/dscale [G] fp32 | None) — group by group the bits of `cosine_cross_entropy_backward` on that group alone.
    grad: the upstream gradient as a number, the same for every group; mean_over: the row count a group's loss was averaged over (default M)."""
    what = "cosine_cross_entropy_grouped_backward"
    a, lda, gsa, b, ldb, gsb, G, M, T, D, labels, flags = _cosine_ce_grouped_args(what, a, b, labels, normalize_a, normalize_b)
    if not isinstance(lse_row, torch.Tensor) or lse_row.dtype != torch.float32 or lse_row.numel() != G * M or not lse_row.is_contiguous():
        raise _lib.PclipError(f"{what}: lse_row must be a contiguous float32 tensor of G * M = {G * M} entries")
    require_cuda(a, lse_row)
    dev = a.device
    weight = float(grad) / (mean_over or M)
    lib = _lib.load()
    nws = int(lib.pclip_cosine_ce_grouped_workspace(1, G, M, T, D))
    ws = _workspace(nws, dev)
    ds = torch.empty(G, dtype=torch.float32, device=dev) if want_scale else None
    walks = [(0, M, want_a or (want_scale and not want_b)), (1, T, want_b)]          # (dscale is a by-product of a gradient walk: of dL/da's if no other runs)
    grads, ds_left = [], ds
    for direction, rows, run in walks:
        if not run:
            grads.append(None)
            continue
        g = torch.empty(G, rows, D, dtype=torch.float32, device=dev)
        check(lib.pclip_cosine_ce_grouped_backward_f16(ptr(a), lda, gsa, M, ptr(b), ldb, gsb, T, D, G, float(np.float32(scale)), flags, ptr(labels), ptr(lse_row),
                                                       float(np.float32(weight)), direction, ptr(g), ptr(ds_left), ptr(ws), nws, stream()),
              "pclip_cosine_ce_grouped_backward_f16")
        ds_left = None
        grads.append(g)
    return (grads[0] if want_a else None), grads[1], ds


def _cosine_sigmoid_args(what, a, b, scale, bias, ids_a, ids_b, normalize_a, normalize_b):
    """The operands of the two sigmoid-loss calls as the kernels take them: (a, b, lda, ldb, M, T, D, scale, bias, ids_a, ids_b, flags)."""
    require_cuda(a, b, ids_a, ids_b)
    a, b = _f16_rows(a, f"{what}: a"), _f16_rows(b, f"{what}: b")
    (M, D), (T, Db) = a.shape, b.shape
    if D != Db:
        raise _lib.PclipError(f"{what}: a has {D} columns, b has {Db}")
    if M < 1 or T < 1:
        raise _lib.PclipError(f"{what}: empty operand (M={M}, T={T})")
    scale, bias = float(np.float32(scale)), float(np.float32(bias))
    if not (math.isfinite(scale) and math.isfinite(bias)):
        raise _lib.PclipError(f"{what}: scale={scale} and bias={bias} must be finite")
    flags = (_lib.SIG_NORMALIZE_A if normalize_a else 0) | (_lib.SIG_NORMALIZE_B if normalize_b else 0)
    if (ids_a is None) != (ids_b is None):
        raise _lib.PclipError(f"{what}: ids_a and ids_b go together (both None: the diagonal)")
    if ids_a is None:
        if M != T:
            raise _lib.PclipError(f"{what}: without ids the positives are the diagonal, which needs M == T (M={M}, T={T})")
    else:
        for name, t, n in (("ids_a", ids_a, M), ("ids_b", ids_b, T)):
            if t.dtype not in (torch.int32, torch.int64) or t.dim() != 1 or t.shape[0] != n:
                raise _lib.PclipError(f"{what}: {name} must be an int32 / int64 tensor of {n} entries")
        if ids_a.dtype != ids_b.dtype:
            raise _lib.PclipError(f"{what}: ids_a is {ids_a.dtype}, ids_b is {ids_b.dtype}: both int32 or both int64")
        ids_a, ids_b = ids_a.contiguous(), ids_b.contiguous()
        flags |= _lib.SIG_IDS_I64 if ids_a.dtype == torch.int64 else 0
    return a, b, (a.stride(0) if M > 1 else D), (b.stride(0) if T > 1 else D), M, T, D, scale, bias, ids_a, ids_b, flags


def cosine_sigmoid(a, b, scale: float, bias: float, ids_a=None, ids_b=None, normalize_a: bool = False, normalize_b: bool = False, want_rows: bool = False):
    """SigLIP's pairwise sigmoid loss over x = scale * a' @ b'^T + bias without the [M, T] matrix: loss = 1/M sum_m sum_t softplus(-z x), z = +1 on positive
    pairs, -1 elsewhere.  a [M, D], b [T, D] fp16 (row-strided views are read in place), a' / b' the rows or their `l2norm_rows`; x stays fp32.
    ids_a [M], ids_b [T], both int32 or both int64: (m, t) is positive iff ids_a[m] == ids_b[t] >= 0 — any number of positives per row or column; a negative id
    matches nothing; an id is compared, never used as an index.  Without ids the positives are the diagonal (M == T).
    Returns the loss (0-dim fp32), and the per-row sums [M] (whose mean the loss is) as a second value with `want_rows`."""
    a, b, lda, ldb, M, T, D, scale, bias, ids_a, ids_b, flags = _cosine_sigmoid_args("cosine_sigmoid", a, b, scale, bias, ids_a, ids_b, normalize_a, normalize_b)
    dev = a.device
    rows = torch.empty(M, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    nws = _lib.workspace_bytes(_lib.OP_COSINE_SIGMOID, M, T, D)
    ws = _workspace(nws, dev)
    check(_lib.load().pclip_cosine_sigmoid_f16(ptr(a), lda, M, ptr(b), ldb, T, D, scale, bias, flags, ptr(ids_a), ptr(ids_b), ptr(rows), ptr(loss), ptr(ws), nws,
                                               stream()), "pclip_cosine_sigmoid_f16")
    return (loss, rows) if want_rows else loss


def cosine_sigmoid_backward(a, b, scale: float, bias: float, ids_a=None, ids_b=None, normalize_a: bool = False, normalize_b: bool = False, want_a: bool = True,
                            want_b: bool = True, want_scale: bool = True, want_bias: bool = True, grad: float = 1.0, mean_over: int = None):
    """The gradients of `cosine_sigmoid`: (dL/da [M, D] fp32 | None, dL/db [T, D] fp32 | None, dL/dscale 0-dim fp32 | None, dL/dbias 0-dim fp32 | None).
    Nothing is kept from the forward: logit tiles are recomputed and fed to a second matrix product; the sigmoid tile is rounded to fp16 on the way, the target
    term, the weight and the scale act in fp32.  With normalize_a / normalize_b the gradient is chained in fp32 through the normalisation.
    grad: the upstream gradient as a number; mean_over: the row count the loss was averaged over when the rows are a slice of a larger batch (default M) — a row
    of dL/da has the same bits in any batch with the same b, ids and `grad / mean_over`."""
    a, b, lda, ldb, M, T, D, scale, bias, ids_a, ids_b, flags = _cosine_sigmoid_args("cosine_sigmoid_backward", a, b, scale, bias, ids_a, ids_b, normalize_a,
                                                                                    normalize_b)
    dev = a.device
    weight = float(np.float32(float(grad) / (mean_over or M)))
    if not math.isfinite(weight):
        raise _lib.PclipError(f"cosine_sigmoid_backward: grad / mean_over = {weight} must be finite")
    nws = _lib.workspace_bytes(_lib.OP_COSINE_SIGMOID_BACKWARD, M, T, D)
    ws = _workspace(nws, dev)
    ds = torch.empty((), dtype=torch.float32, device=dev) if want_scale else None
    dbi = torch.empty((), dtype=torch.float32, device=dev) if want_bias else None
    walks = [(0, M, want_a or ((want_scale or want_bias) and not want_b)), (1, T, want_b)]      # (the scalars are by-products of a gradient walk: of dL/da's if no other runs)
    grads, ds_left, db_left = [], ds, dbi
    for direction, rows, run in walks:
        if not run:
            grads.append(None)
            continue
        g = torch.empty(rows, D, dtype=torch.float32, device=dev)
        check(_lib.load().pclip_cosine_sigmoid_backward_f16(ptr(a), lda, M, ptr(b), ldb, T, D, scale, bias, flags, ptr(ids_a), ptr(ids_b), weight, direction,
                                                            ptr(g), ptr(ds_left), ptr(db_left), ptr(ws), nws, stream()), "pclip_cosine_sigmoid_backward_f16")
        ds_left = db_left = None
        grads.append(g)
    return (grads[0] if want_a else None), grads[1], ds, dbi


def _tip_segment_table(t: torch.Tensor, N=None):
    """The checks and the table of `tip_segments` on whatever device `t` lives on: (seg [N + 1] int32, N).  One host transfer."""
    if t.dim() == 2:
        if N is not None and int(N) != t.shape[1]:
            raise _lib.PclipError(f"tip_segments: cache_values {tuple(t.shape)} has {t.shape[1]} classes, N={N} was given")
        N = t.shape[1]
        if N < 1:
            raise _lib.PclipError(f"tip_segments: cache_values {tuple(t.shape)} has no classes")
        onehot = (((t == 0) | (t == 1)).all(1) & ((t != 0).sum(1) == 1)).all() if t.shape[0] else torch.ones((), dtype=torch.bool, device=t.device)
        labels = t.argmax(1) if t.shape[0] else torch.zeros(0, dtype=torch.int64, device=t.device)
    elif t.dim() == 1:
        if t.dtype not in (torch.int32, torch.int64):
            raise _lib.PclipError(f"tip_segments: a label vector must be int32 / int64, got {t.dtype}")
        onehot, labels = torch.ones((), dtype=torch.bool, device=t.device), t.long()
    else:
        raise _lib.PclipError(f"tip_segments: expected one-hot cache_values [NK, N] or labels [NK], got shape {tuple(t.shape)}")
    NK = labels.shape[0]
    if NK:
        ordered = (labels[1:] >= labels[:-1]).all()
        facts = torch.stack([onehot.long(), ordered.long(), labels.min(), labels.max()]).cpu().tolist()          # the one synchronisation
    else:
        facts = [1, 1, 0, 0]
    if not facts[0]:
        raise _lib.PclipError("tip_segments: cache_values is not one-hot (every row needs exactly one 1 among zeros; soft cache values are not supported)")
    if N is None:
        N = facts[3] + 1
    N = int(N)
    if N < 1 or facts[2] < 0 or facts[3] >= N:
        raise _lib.PclipError(f"tip_segments: labels span [{facts[2]}, {facts[3]}], outside [0, N={N})")
    if not facts[1]:
        raise _lib.PclipError("tip_segments: the cache rows are not sorted by class (build_cache_model sorts them; sort keys and values with the same permutation)")
    # seg[n] = the number of rows whose class is below n: a search in the sorted labels (no second synchronisation, unlike a bincount on the device)
    seg = torch.searchsorted(labels, torch.arange(N + 1, dtype=labels.dtype, device=t.device)).int()
    return seg, N


def tip_segments(cache_values_or_labels: torch.Tensor, N: int = None) -> torch.Tensor:
    """Segment offsets of a Tip-Adapter cache: int32 [N + 1] on the device, class n owns key rows seg[n] .. seg[n + 1] - 1 (ragged; empty classes allowed).
    Takes upstream's one-hot `cache_values` [NK, N] or the label vector [NK]; raises PclipError if a row is not one-hot or the rows are not sorted by class.
    Synchronises once: compute it once per cache and pass it on (`tip_logits(..., seg)`)."""
    require_cuda(cache_values_or_labels)
    return _tip_segment_table(cache_values_or_labels, N)[0]


def _tip_coef(what: str, name: str, v) -> float:
    """alpha / beta as the fp32 number the kernel takes: finite and >= 0."""
    if isinstance(v, torch.Tensor):
        if v.requires_grad:
            raise NotImplementedError(f"{what}: {name} requires grad — no gradient is produced for it (upstream trains only the cache keys)")
        v = v.item()
    v = float(np.float32(v))
    if not math.isfinite(v) or v < 0:
        raise _lib.PclipError(f"{what}: {name}={v} must be finite and >= 0")
    return v


def _tip_args(what, features, cache_keys, seg, clip_rows, layout, N=None):
    """Shape and envelope checks first (they need no device), then the device checks: (f, key rows, seg, w, ldf, ldk, ldw, Q, NK, N, D).
    clip_rows None (the key gradient, which has no zero-shot term): N is given instead."""
    if layout not in (None, "dn", "nd"):
        raise _lib.PclipError(f"{what}: layout={layout!r}: expected 'dn' (cache_keys [D, NK], as build_cache_model returns), 'nd' ([NK, D] rows) or None")
    for name, t in (("features", features), ("cache_keys", cache_keys), ("clip weight rows", clip_rows)):
        if t is not None and (t.dtype != torch.float16 or t.dim() != 2):
            raise _lib.PclipError(f"{what}: {name} must be a 2-D float16 tensor, got {t.dtype} {tuple(t.shape)}")
    Q, D = features.shape
    if D % 64 or D < 64 or D > _lib.TIP_MAX_D:
        raise _lib.PclipError(f"{what}: D={D} must be a multiple of 64, <= {_lib.TIP_MAX_D}")
    if Q < 1:
        raise _lib.PclipError(f"{what}: no query rows")
    N = clip_rows.shape[0] if clip_rows is not None else int(N)
    if clip_rows is not None and clip_rows.shape[1] != D:
        raise _lib.PclipError(f"{what}: clip weight rows {tuple(clip_rows.shape)} are not [N, D={D}]")
    if N < 1 or N > _lib.TIP_MAX_CLASSES:
        raise _lib.PclipError(f"{what}: N={N} must be in [1, {_lib.TIP_MAX_CLASSES}] (the fused argmax's cap)")
    if layout is None:                                                  # the rule of utils._clip_weight_rows: told from the shape, a square tensor read as upstream's [D, NK]
        if D not in cache_keys.shape:
            raise _lib.PclipError(f"{what}: cache_keys {tuple(cache_keys.shape)} matches neither [D={D}, NK] nor [NK, D]")
        layout = "dn" if cache_keys.shape[0] == D else "nd"
    if cache_keys.shape[0 if layout == "dn" else 1] != D:
        raise _lib.PclipError(f"{what}: cache_keys {tuple(cache_keys.shape)} is not {'[D, NK]' if layout == 'dn' else '[NK, D]'} with D={D}")
    NK = cache_keys.shape[1 if layout == "dn" else 0]
    if seg.dtype != torch.int32 or seg.dim() != 1 or seg.shape[0] != N + 1 or not seg.is_contiguous():
        raise _lib.PclipError(f"{what}: seg must be a contiguous int32 tensor of N + 1 = {N + 1} entries (ops.tip_segments), got {seg.dtype} {tuple(seg.shape)}")
    require_cuda(features, cache_keys, seg, clip_rows)
    f = _f16_rows(features, f"{what}: features")
    w = _f16_rows(clip_rows, f"{what}: clip weight rows") if clip_rows is not None else None
    if NK == 0:
        keys = None
    else:
        keys = transpose(cache_keys) if layout == "dn" else _f16_rows(cache_keys, f"{what}: cache_keys")
    ldk = keys.stride(0) if NK > 1 else D
    return f, keys, seg, w, (f.stride(0) if Q > 1 else D), ldk, (w.stride(0) if w is not None and N > 1 else D), Q, NK, N, D


def tip_logits(features, cache_keys, seg, clip_rows, alpha, beta, scale: float = 100., want_logits: bool = True, want_f32: bool = False,
               want_argmax: bool = False, layout=None):
    """Tip-Adapter's logits `scale * features @ clip_rows^T + alpha * exp(-(beta - beta * features @ keys^T)) @ one_hot` on the fused kernel (pclip_tip_logits_f16):
    features [Q, D], clip_rows [N, D] fp16; cache_keys upstream's [D, NK] (one `transpose`) or [NK, D] rows (`layout` "dn" / "nd" / None = told from the shape, a
    square tensor read as [D, NK]); seg from `tip_segments`.  Returns (logits [Q, N] fp16 | None, logits32 [Q, N] fp32 | None, argmax [Q] int32 | None); with the
    argmax alone no matrix is written.  The fp16 logits are the first N columns of a buffer whose rows are N rounded up to 8 halves apart."""
    what = "tip_logits"
    alpha, beta = _tip_coef(what, "alpha", alpha), _tip_coef(what, "beta", beta)
    if not (want_logits or want_f32 or want_argmax):
        raise _lib.PclipError(f"{what}: no output requested")
    f, keys, seg, w, ldf, ldk, ldw, Q, NK, N, D = _tip_args(what, features, cache_keys, seg, clip_rows, layout)
    dev = f.device
    ldl = (N + 7) // 8 * 8
    buf = torch.empty(Q, ldl, dtype=torch.float16, device=dev) if want_logits else None
    l32 = torch.empty(Q, N, dtype=torch.float32, device=dev) if want_f32 else None
    am = torch.empty(Q, dtype=torch.int32, device=dev) if want_argmax else None
    check(_lib.load().pclip_tip_logits_f16(ptr(f), ldf, Q, ptr(keys), ldk, NK, ptr(seg), ptr(w), ldw, N, D, float(np.float32(scale)), alpha, beta,
                                           ptr(buf), ldl, ptr(l32), ptr(am), stream()), "pclip_tip_logits_f16")
    return (buf[:, :N] if want_logits else None), l32, am


def tip_grid(features, cache_keys, seg, clip_rows, betas, alphas, labels, scale: float = 100., layout=None) -> torch.Tensor:
    """Tip-Adapter's `search_hp` counts on one launch (pclip_tip_grid_f16): int32 [nb, na] on the device, [ib, ia] = the number of queries whose `tip_logits`
    argmax under (betas[ib], alphas[ia]) equals their label — exactly what nb x na single calls count.  betas / alphas: sequences of numbers (na <= 32);
    labels [Q] int32 / int64, one outside [0, N) matches nothing."""
    what = "tip_grid"
    betas = [_tip_coef(what, f"betas[{i}]", b) for i, b in enumerate(betas)]
    alphas = [_tip_coef(what, f"alphas[{i}]", a) for i, a in enumerate(alphas)]
    if not betas or not alphas or len(alphas) > _lib.TIP_MAX_ALPHAS:
        raise _lib.PclipError(f"{what}: {len(betas)} betas x {len(alphas)} alphas: at least one of each, at most {_lib.TIP_MAX_ALPHAS} alphas")
    if labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1 or labels.shape[0] != features.shape[0]:
        raise _lib.PclipError(f"{what}: labels must be an int32 / int64 tensor of {features.shape[0]} entries")
    f, keys, seg, w, ldf, ldk, ldw, Q, NK, N, D = _tip_args(what, features, cache_keys, seg, clip_rows, layout)
    require_cuda(f, labels)
    dev = f.device
    lab = torch.where((labels >= 0) & (labels < N), labels, torch.full_like(labels, -1)).int().contiguous()
    bt = torch.tensor(betas, dtype=torch.float32).to(dev)
    at = torch.tensor(alphas, dtype=torch.float32).to(dev)
    correct = torch.empty(len(betas), len(alphas), dtype=torch.int32, device=dev)
    check(_lib.load().pclip_tip_grid_f16(ptr(f), ldf, Q, ptr(keys), ldk, NK, ptr(seg), ptr(w), ldw, N, D, float(np.float32(scale)), ptr(bt), len(betas),
                                         ptr(at), len(alphas), ptr(lab), ptr(correct), stream()), "pclip_tip_grid_f16")
    return correct


def tip_keys_backward(features, cache_keys, seg, dlogits, alpha, beta, layout=None, out: torch.Tensor = None) -> torch.Tensor:
    """The gradient of a loss with respect to the cache KEY ROWS from its gradient `dlogits` [Q, N] fp32 with respect to the fp32 logits of `tip_logits`
    (pclip_tip_keys_backward_f16): fp32 [NK, D], dkeys[j] = alpha beta sum_q dlogits[q, class(j)] E[q, j] features[q].  E is recomputed; nothing of the forward is
    kept.  Nothing else gets a gradient (upstream's Tip-Adapter-F trains the keys only).  cache_keys / layout as in `tip_logits`.
    out: an optional contiguous float32 [NK, D] tensor (16-byte aligned) that receives the gradient."""
    what = "tip_keys_backward"
    alpha, beta = _tip_coef(what, "alpha", alpha), _tip_coef(what, "beta", beta)
    if dlogits.dtype != torch.float32 or dlogits.dim() != 2 or dlogits.shape[0] != features.shape[0] or dlogits.shape[1] != seg.shape[0] - 1:
        raise _lib.PclipError(f"{what}: dlogits must be a float32 [Q={features.shape[0]}, N={seg.shape[0] - 1}] tensor, got {dlogits.dtype} {tuple(dlogits.shape)}")
    N = dlogits.shape[1]
    f, keys, seg, _, ldf, ldk, _, Q, NK, N, D = _tip_args(what, features, cache_keys, seg, None, layout, N=N)
    require_cuda(f, dlogits)
    dl = dlogits.contiguous()
    if out is None:
        dkeys = torch.empty(NK, D, dtype=torch.float32, device=f.device)
    else:
        if out.dtype != torch.float32 or tuple(out.shape) != (NK, D) or not out.is_contiguous() or not out.is_cuda or out.data_ptr() % 16:
            raise _lib.PclipError(f"{what}: out must be a contiguous, 16-byte aligned float32 [NK={NK}, D={D}] device tensor")
        dkeys = out
    nws = _lib.workspace_bytes(_lib.OP_TIP_BACKWARD, Q, NK, D)
    ws = _workspace(nws, f.device)
    check(_lib.load().pclip_tip_keys_backward_f16(ptr(f), ldf, Q, ptr(keys), ldk, NK, ptr(seg), N, D, alpha, beta, ptr(dl), ptr(dkeys), ptr(ws), nws, stream()),
          "pclip_tip_keys_backward_f16")
    return dkeys


CLASSIFY_ROUTES = ("two stages", "one launch, small N", "one launch, mid N", "fused row panels")


def classify_route(Q: int, N: int, D: int, alpha: float, beta: float, want_p=False, want_argmax=True, topk: int = 0, has_zt: bool = True) -> str:
    """The kernels `classify` takes for a call of this shape under the current context's routing (pclip_classify_route_ex).  The routes differ in fp32 summation
    order only — at a near-tie of p (top-2 margin < ~1e-6) the argmax may depend on the route, i.e. on the batch size; `classify_two_stage()` pins one arithmetic."""
    a32, oma32 = float(np.float32(alpha)), float(np.float32(1 - float(alpha)))
    r = _lib.load().pclip_classify_route_ex(Q, N, D, a32, oma32, float(np.float32(beta)), int(has_zt), int(bool(want_p)), int(bool(want_argmax)), topk,
                                            _classify_flags.get(), _lib.workspace_bytes(_lib.OP_CLASSIFY, Q, N, D))
    return CLASSIFY_ROUTES[r]


# The routing flags (pclip_classify_ex_f16) of the `classify` calls made in this context — per thread and per asyncio task.  Each context manager below replaces
# only its own bits and restores the previous word on exit, so they nest: `classify_panel_passes` inside `classify_fused` keeps both.
_classify_flags = contextvars.ContextVar("pclip_classify_flags", default=0)
_MID = _lib.CLASSIFY_NO_MID | _lib.CLASSIFY_FORCE_MID
_PANELS = _lib.CLASSIFY_NO_PANELS | _lib.CLASSIFY_FORCE_PANELS
_PASSES = _lib.CLASSIFY_PANEL_TWO_PASS | _lib.CLASSIFY_PANEL_FORCE_SECOND


class _classify_routing:
    mask = bits = 0

    def __enter__(self):
        self._token = _classify_flags.set(_classify_flags.get() & ~self.mask | self.bits)
        return self

    def __exit__(self, *exc):
        _classify_flags.reset(self._token)
        return False


class classify_mid(_classify_routing):
    """`with ops.classify_mid(mode):` — routing of the one-launch mid-N kernel (16 < N <= 256): 0 off (two stages), 1 by size (default), 2 every shape it can run."""
    def __init__(self, mode: int):
        self.mode = mode
        self.mask = _MID if mode >= 0 else 0
        self.bits = {0: _lib.CLASSIFY_NO_MID, 2: _lib.CLASSIFY_FORCE_MID}.get(mode, 0)


class classify_two_stage(_classify_routing):
    """`with ops.classify_two_stage():` — classification through pclip_sqdist_f16 + pclip_fuse_probs instead of the fused row-panel kernel / the one-launch mid-N
    kernel (their reference)."""
    mask, bits = _MID | _PANELS, _lib.CLASSIFY_NO_MID | _lib.CLASSIFY_NO_PANELS


class classify_fused(_classify_routing):
    """`with ops.classify_fused():` — the fused row-panel kernel for EVERY argmax-only call it can run (by default only calls with enough panels to fill the chip;
    the one-launch mid-N kernel, which would take N <= 256 first, is switched off inside)."""
    mask, bits = _MID | _PANELS, _lib.CLASSIFY_NO_MID | _lib.CLASSIFY_FORCE_PANELS


class classify_panel_passes(_classify_routing):
    """`with ops.classify_panel_passes(mode):` — 0 one pass + candidates with proof (default), 1 always two passes, 2 candidates computed, second pass forced (tests)."""
    def __init__(self, mode: int):
        self.mode = mode
        self.mask = _PASSES if mode >= 0 else 0
        self.bits = {1: _lib.CLASSIFY_PANEL_TWO_PASS, 2: _lib.CLASSIFY_PANEL_FORCE_SECOND}.get(mode, 0)


class classify_panel_exact(_classify_routing):
    """`with ops.classify_panel_exact():` — the fused row-panel kernel keeps torch.cdist's sqrt -> square round trip (bit-identical distances, a third slower)."""
    def __init__(self, exact: bool = True):
        self.mask, self.bits = _lib.CLASSIFY_PANEL_EXACT, _lib.CLASSIFY_PANEL_EXACT if exact else 0


def classify_panel_stats(reset: bool = False, tiles: bool = False):
    """(panels classified by the fused kernel, panels that needed a second pass[, class tiles those second passes walked]) since the last reset; synchronises."""
    import ctypes
    out = (ctypes.c_int * 3)()
    check(_lib.load().pclip_classify_panel_stats(ctypes.cast(out, ctypes.c_void_p), int(reset)), "pclip_classify_panel_stats")
    return (int(out[0]), int(out[1]), int(out[2])) if tiles else (int(out[0]), int(out[1]))


def classify_panel_distances(q, zi, zt, exact: bool = False):
    """Test hook: the distances the fused row-panel kernel forms for its first tile, ([256, 128] visual, [256, 128] textual) fp32; exact: with the sqrt round trip."""
    require_cuda(q, zi, zt)
    Q, D = q.shape
    N = zi.shape[0]
    dump = torch.empty(2, 256, 128, dtype=torch.float32, device=q.device)
    ws = _workspace(_lib.workspace_bytes(_lib.OP_CLASSIFY, max(Q, 4096), N, D), q.device)
    check(_lib.load().pclip_classify_panel_dump_f16(ptr(q), ptr(zi), ptr(zt), Q, N, D, ptr(dump), int(exact), ptr(ws), ws.numel(), stream()), "pclip_classify_panel_dump_f16")
    return dump[0], dump[1]


def hp_sweep(d2i, d2t, N: int, labels, alphas, betas) -> torch.Tensor:
    """Correct-counts int32 [na, nb] for every (alpha, beta) pair (main.py:187-199 / 419-430)."""
    require_cuda(d2i, d2t, labels)
    Q, ldd = d2i.shape
    dev = d2i.device
    a = np.asarray(alphas, dtype=np.float64)
    a32 = torch.tensor(a.astype(np.float32), device=dev)
    oma32 = torch.tensor((1 - a).astype(np.float32), device=dev)
    b32 = torch.tensor(np.asarray(betas, dtype=np.float64).astype(np.float32), device=dev)
    labels = labels.to(torch.int32).contiguous()
    correct = torch.zeros(len(a), len(b32), dtype=torch.int32, device=dev)
    check(_lib.load().pclip_hp_sweep(ptr(d2i), ptr(d2t), ptr(labels), Q, N, ldd, ptr(a32), ptr(oma32), len(a),
                                     ptr(b32), len(b32), ptr(correct), stream()), "pclip_hp_sweep")
    return correct


def adapter_fc(x, w1, g1, b1, w2, g2, b2, ratio: float = 0.2, l2norm_out: bool = False, want_sq: bool = False):
    """Adapter_FC.forward (model.py:91-95), optionally fused with the following row normalise."""
    require_cuda(x, w1, w2)
    x = _f16c(x)
    B, D = x.shape
    H = w1.shape[0]
    y = torch.empty_like(x)
    sq = torch.empty(B, dtype=torch.float32, device=x.device) if want_sq else None
    ws = _workspace(_lib.workspace_bytes(_lib.OP_ADAPTER_FC, B, H, D), x.device)
    r32, omr32 = float(np.float32(ratio)), float(np.float32(1 - ratio))
    check(_lib.load().pclip_adapter_fc_f16(ptr(x), B, D, H, ptr(_f16c(w1)), ptr(_f16c(g1)), ptr(_f16c(b1)),
                                           ptr(_f16c(w2)), ptr(_f16c(g2)), ptr(_f16c(b2)), r32, omr32,
                                           int(l2norm_out), ptr(y), ptr(sq), ptr(ws), ws.numel(), stream()),
          "pclip_adapter_fc_f16")
    return (y, sq) if want_sq else y


def layernorm_blend(h, gamma, beta, x, ratio: float = 0.2, l2norm_out: bool = False, eps: float = 1e-5, want_sq: bool = False, out=None):
    """r16(r16(ratio * LN(h)) + r16((1 - ratio) * x)) — the last stage of Adapter_FC.forward (model.py:92-95) on its own, optionally followed by the
    row normalise.  want_sq (as adapter_fc's): also the fp32 squared norms of the rows as stored, (y, sq)."""
    require_cuda(h, gamma, beta, x)
    h, x = _f16c(h), _f16c(x)
    R, D = h.shape
    y = torch.empty_like(h) if out is None else out
    sq = torch.empty(R, dtype=torch.float32, device=h.device) if want_sq else None
    r32, omr32 = float(np.float32(ratio)), float(np.float32(1 - ratio))
    check(_lib.load().pclip_layernorm_blend_f16(ptr(h), ptr(_f16c(gamma)), ptr(_f16c(beta)), eps, ptr(x), r32, omr32, int(l2norm_out),
                                                ptr(y), ptr(sq), R, D, stream()), "pclip_layernorm_blend_f16")
    return (y, sq) if want_sq else y


ADAPTER_WIDTHS = (8, 16, 24, 32)      # conv adapter widths the kernels are instantiated for (csrc/pclip_adapter.hip: 16, pclip_adapter_w.hip: the rest)


def _adapter_width(conv1):
    width = int(conv1.shape[0])
    if width not in ADAPTER_WIDTHS:
        raise _lib.PclipError(f"conv adapter width {width}: the gfx950 adapter kernels are built for widths {ADAPTER_WIDTHS}")
    return width


def adapter_conv(x, three_x: bool, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b,
                 l2norm_out: bool = False, want_sq: bool = False):
    """Adapter.forward (model.py:49-78): conv-2x / conv-3x feature adapter, whole pipeline in one kernel.  The width is conv1's
    channel count."""
    require_cuda(x, conv1)
    x = _f16c(x)
    B, D = x.shape
    width = _adapter_width(conv1)
    y = torch.empty_like(x)
    sq = torch.empty(B, dtype=torch.float32, device=x.device) if want_sq else None
    f = lambda t: None if t is None else ptr(_f16c(t))
    check(_lib.load().pclip_adapter_conv_w_f16(ptr(x), B, D, int(three_x), width, f(conv1), f(ln1w), f(ln1b), f(conv2),
                                               f(ln2w), f(ln2b), f(conv3), f(ln3w), f(ln3b), int(l2norm_out), ptr(y),
                                               ptr(sq), stream()), "pclip_adapter_conv_w_f16")
    return (y, sq) if want_sq else y


# ---- encoder building blocks -------------------------------------------------------------------

def gemm(a, w, bias=None, act: int = 0, residual=None, out=None):
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T) — nn.Linear with fused bias/QuickGELU/residual.  K a multiple of 8 (K % 64 != 0 runs
    the K-tail instantiations: the columns beyond K are never read)."""
    require_cuda(a, w)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=a.device)
    lib = _lib.load()
    if residual is None and M <= _SPLITK_MAX_M and _SPLITK:
        need = lib.pclip_gemm_splitk_workspace(M, N, K)
        if need and a.stride(0) % 8 == 0 and w.stride(0) % 8 == 0 and out.stride(0) % 8 == 0 and \
                not ((a.data_ptr() | w.data_ptr() | out.data_ptr()) & 15) and (bias is None or not (bias.data_ptr() & 15)):
            ws = _workspace(need, a.device)
            check(lib.pclip_gemm_splitk_f16(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias), act,
                                            ptr(ws), ws.numel(), stream()), "pclip_gemm_splitk_f16")
            return out
    check(lib.pclip_gemm_f16(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K,
                             ptr(bias), act, ptr(residual), stream()), "pclip_gemm_f16")
    return out


def gemm4w(a, w, bias=None, act: int = 0, residual=None, out=None, var: int = 0):
    """ops.gemm on the four-wave asm-loop kernel explicitly (csrc/pclip_gemm4w.hip; ops.gemm routes its 256 x 256 tiles there by itself).  var: the kernel build — 0 product,
    1 race-stress (its own K-loop statement), 6 the product loop without the epilogue (stores nothing), 8 the product loop with time stamps (pclip_gemm4w_stamp_buffer);
    6 and 8 need a bias, without one they run 0.  Raises PclipError for shapes outside the kernel (N % 256, K % 64, K >= 192)."""
    require_cuda(a, w)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=a.device)
    check(_lib.load().pclip_gemm4w_var_f16(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias), act, ptr(residual), var,
                                           stream()), "pclip_gemm4w_f16")
    return out


ROUTE_AUTO, ROUTE_GENERIC, ROUTE_RING = _lib.ROUTE_AUTO, _lib.ROUTE_GENERIC, _lib.ROUTE_RING      # cfg of gemm_route (0 .. 4: 128x128, 256x128, 256x256, 256x64, 256x32 tiles)


def gemm_route(a, w, bias=None, act: int = 0, residual=None, scale=None, shift=None, out=None, cfg: int = ROUTE_AUTO, may_split: bool = True,
               band: int = 0, band_n: int = 0, rev: int = 2, use4w: int = 1, cus: int = 0):
    """Test entry (pclip_gemm_route_f16): ops.gemm / gemm_bn / gemm_bn_res_relu through the product's dispatch with the route taken from THIS call — act 0 / 1
    (bias, residual), 2 / 3 BatchNorm (+ReLU), 5 BatchNorm + residual + ReLU; cfg, row split, tile order, the 256 x 256 kernel and `cus`, which stands in for the
    device's CU count (0: the device's).  Returns (out, launches): one dict per kernel launch — family (a name of _lib.ROUTE_RAN), kt, rows, rev, band."""
    require_cuda(a, w, bias, residual, scale, shift, out)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=a.device)
    lib = _lib.load()
    fields, cap = _lib.ROUTE_FIELDS, 8
    report = (ctypes.c_int * (1 + fields * cap))()
    check(lib.pclip_gemm_route_f16(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias), act, ptr(residual), ptr(scale), ptr(shift),
                                   cfg, int(may_split), band, band_n, rev, use4w, cus or lib.pclip_device_cus(), report, len(report), stream()), "pclip_gemm_route_f16")
    if report[0] > cap:
        raise _lib.PclipError(f"pclip_gemm_route_f16: {report[0]} launches, the report holds {cap}")
    launches = []
    for i in range(report[0]):
        family, kt, rows, rv, bd = report[1 + fields * i:1 + fields * (i + 1)]
        launches.append(dict(family=_lib.ROUTE_RAN[family], kt=bool(kt), rows=rows, rev=bool(rv), band=bd))
    return out, launches


class gemm_eight_wave:
    """`with ops.gemm_eight_wave():` — ops.gemm's 256 x 256 tiles on the eight-wave kernel (the four-wave kernel's bit-identity reference)."""
    def __enter__(self):
        self.before = _lib.load().pclip_gemm4w_config(0)
        return self

    def __exit__(self, *exc):
        _lib.load().pclip_gemm4w_config(1 if self.before != 0 else 0)
        return False


# split-K for small M (serving requests).  Opt-in (`with ops.low_latency():`, or PCLIP_GEMM_SPLITK=1): a split call sums K in
# slices, so its last fp16 bit can differ from the unsplit kernel's — the batch paths keep one arithmetic for every batch size,
# the serving entry takes the latency.
_SPLITK = os.environ.get("PCLIP_GEMM_SPLITK", "0") == "1"
_SPLITK_MAX_M = 4096


def splitk_active(M: int) -> bool:
    """True when ops.gemm would consider the split-K kernel for an M-row call (low-latency mode and a small M)."""
    return _SPLITK and M <= _SPLITK_MAX_M


class low_latency:
    """Context manager: inside it, ops.gemm uses pclip_gemm_splitk_f16 for the shapes pclip_gemm_splitk_workspace accepts."""

    def __init__(self, enabled: bool = True):
        self.enabled = enabled

    def __enter__(self):
        global _SPLITK
        self.prev, _SPLITK = _SPLITK, self.enabled
        return self

    def __exit__(self, *exc):
        global _SPLITK
        _SPLITK = self.prev
        return False


def gemm_bn(a, w, scale, shift, relu: bool = True, out=None):
    """relu?(bn(a @ w.T)) with eval-mode BatchNorm folded to fp32 per-column scale / shift — conv + bn (+ relu) of the ResNet
    tower in one launch (clip/model.py:43-52).  K a multiple of 8."""
    require_cuda(a, w, scale, shift)
    a, w = _f16c(a), _f16c(w)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=a.device)
    check(_lib.load().pclip_gemm_bn_f16(ptr(a), K, ptr(w), w.shape[1], ptr(out), N, M, N, K, ptr(scale), ptr(shift), int(relu),
                                        stream()), "pclip_gemm_bn_f16")
    return out


def gemm_bn_res_relu(a, w, scale, shift, residual, out=None):
    """relu(bn(a @ w.T) + residual): conv3 + bn3 + identity add + ReLU of a bottleneck in one launch where the fused epilogue
    applies (N % 64 == 0, K % 8 == 0, aligned operands), otherwise GEMM followed by bn_act — the same values either way."""
    require_cuda(a, w, scale, shift, residual)
    a, w, residual = _f16c(a), _f16c(w), _f16c(residual)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=a.device)
    if N % 64 == 0 and K % 8 == 0 and not ((a.data_ptr() | w.data_ptr() | out.data_ptr() | residual.data_ptr() | scale.data_ptr() | shift.data_ptr()) & 15):
        check(_lib.load().pclip_gemm_bn_res_f16(ptr(a), K, ptr(w), w.shape[1], ptr(out), N, M, N, K, ptr(scale), ptr(shift), ptr(residual),
                                                stream()), "pclip_gemm_bn_res_f16")
        return out
    gemm(a, w, out=out)
    return bn_act(out, scale, shift, residual=residual, relu=True, out=out)


_zero_line = {}


def conv3x3_bn(x, w, scale, shift, B: int, H: int, W: int, Cin: int, relu: bool = True):
    """relu?(bn(conv3x3(x))) (stride 1, pad 1) on NHWC rows x [B*H*W, Cin] with w [Cout, 9*Cin] in (ky, kx, Cin) order:
    implicit GEMM, no im2col buffer.  Cin and Cout multiples of 8; the rows of w are zero-padded to a multiple of 64 (round_up(9 Cin, 64)
    columns).  Cin outside {8, 16, 32, 64k} or Cout outside {32, 64k} run the convolution's tail instantiations (RN50x4 / RN50x16)."""
    require_cuda(x, w, scale, shift)
    x, w = _f16c(x), _f16c(w)
    Cout = w.shape[0]
    if w.shape[1] != (9 * Cin + 63) // 64 * 64 or x.numel() != B * H * W * Cin:
        raise _lib.PclipError("conv3x3_bn: shape mismatch")
    z = _zero_line.get(x.device)
    if z is None:
        z = _zero_line[x.device] = torch.zeros(64, dtype=torch.float16, device=x.device)
    y = torch.empty(B * H * W, Cout, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_conv3x3_bn_f16(ptr(x), ptr(w), ptr(z), B, H, W, Cin, Cout, ptr(scale), ptr(shift), int(relu), ptr(y),
                                           stream()), "pclip_conv3x3_bn_f16")
    return y


class conv_strip:
    """`with ops.conv_strip(on):` — routing of the narrow 3x3 convolutions (Cin, Cout in {32, 64} at 56 x 56 / 112 x 112) to csrc/pclip_conv_strip.hip (default on)
    or to the implicit-GEMM kernel (off: its reference in the tests)."""
    def __init__(self, on: bool):
        self.mode = int(bool(on))

    def __enter__(self):
        self.before = _lib.load().pclip_conv3x3_strip_config(self.mode)
        return self

    def __exit__(self, *exc):
        _lib.load().pclip_conv3x3_strip_config(self.before)
        return False


def conv_strip_applies(B: int, H: int, W: int, Cin: int, Cout: int) -> bool:
    return bool(_lib.load().pclip_conv3x3_strip_applies(B, H, W, Cin, Cout))


def conv3x3_pool_applies(H: int, W: int, Cin: int, Cout: int) -> bool:
    return bool(_lib.load().pclip_conv3x3_pool_applies(H, W, Cin, Cout))


def conv3x3_bn_pool(x, w, scale, shift, B: int, H: int, W: int, Cin: int):
    """avgpool2(relu(bn(conv3x3(x)))) in one launch: [B * (H / 2) * (W / 2), Cout] (the stem's tail, clip/model.py:104-105, 142-143)."""
    require_cuda(x, w, scale, shift)
    x, w = _f16c(x), _f16c(w)
    Cout = w.shape[0]
    if w.shape[1] != (9 * Cin + 63) // 64 * 64 or x.numel() != B * H * W * Cin:
        raise _lib.PclipError("conv3x3_bn_pool: shape mismatch")
    y = torch.empty(B * (H // 2) * (W // 2), Cout, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_conv3x3_bn_pool_f16(ptr(x), ptr(w), B, H, W, Cin, Cout, ptr(scale), ptr(shift), ptr(y), stream()), "pclip_conv3x3_bn_pool_f16")
    return y


def stem_conv_applies(R: int, Cout: int) -> bool:
    return bool(_lib.load().pclip_stem_conv_applies(R, Cout))


def stem_conv_bn(img, w, scale, shift, relu: bool = True):
    """relu?(bn(conv3x3 stride 2 pad 1)) of NCHW images [B, 3, R, R] (fp32 or fp16) -> NHWC rows [B * Ho * Ho, Cout] fp16, w [Cout, 64] in im2col column order
    (clip/model.py:100-102, 138): no im2col matrix, no separate cast."""
    require_cuda(img, w, scale, shift)
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3] or img.dtype not in (torch.float32, torch.float16) or w.shape[1] != 64:
        raise _lib.PclipError("stem_conv_bn: images [B, 3, R, R] fp32 / fp16 and w [Cout, 64] expected")
    img, w = img.contiguous(), _f16c(w)
    B, R, Cout = img.shape[0], img.shape[2], w.shape[0]
    Ho = (R - 1) // 2 + 1
    y = torch.empty(B * Ho * Ho, Cout, dtype=torch.float16, device=img.device)
    check(_lib.load().pclip_stem_conv_bn_f16(ptr(img), int(img.dtype == torch.float32), B, R, ptr(w), Cout, ptr(scale), ptr(shift), int(relu), ptr(y), stream()),
          "pclip_stem_conv_bn_f16")
    return y


def layernorm(x, gamma, beta, eps: float = 1e-5, out=None, rows: int = None, ld: int = None):
    """fp16 in/out LayerNorm with fp32 statistics and fp32 affine (clip/model.py:155-161)."""
    require_cuda(x, gamma, beta)
    D = x.shape[-1]
    R = x.numel() // D if rows is None else rows
    ld = D if ld is None else ld
    if out is None:
        out = torch.empty(R, D, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_layernorm_f16(ptr(x), ld, ptr(gamma), ptr(beta), eps, ptr(out), R, D, stream()),
          "pclip_layernorm_f16")
    return out


def add_layernorm(x, delta, gamma, beta, eps: float = 1e-5, out=None, update_x: bool = True, rows: int = None,
                  ld: int = None):
    """xs = r16(x + delta) (written back into x when update_x) and returns r16(LayerNorm(xs)): the residual add of
    clip/model.py:188-189 fused into the LayerNorm that consumes it."""
    require_cuda(x, delta, gamma, beta)
    D = x.shape[-1]
    R = x.numel() // D if rows is None else rows
    ld = D if ld is None else ld
    if out is None:
        out = torch.empty(R, D, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_add_layernorm_f16(ptr(x), ptr(delta), ld, ptr(x) if update_x else None, ptr(gamma), ptr(beta),
                                              eps, ptr(out), R, D, stream()), "pclip_add_layernorm_f16")
    return out


ATT_SHORT_MAX_L = 288      # pclip_attention_f16 / _q_f16 keep K / V resident in LDS up to here; pclip_attention_long_q_f16 streams them (non-causal, L <= 4096)


def attention(qkv, B: int, L: int, H: int, causal: bool = False, out=None):
    """softmax(q k^T / 8) v per head on a fused QKV buffer [B*L, 3W].  The kernel follows L alone: L <= 288 the resident-K/V
    kernels, longer (non-causal) sequences the streamed one — bit-identical to each other where both apply."""
    require_cuda(qkv)
    W = H * 64
    if out is None:
        out = torch.empty(B * L, W, dtype=torch.float16, device=qkv.device)
    if L > ATT_SHORT_MAX_L:
        check(_lib.load().pclip_attention_long_q_f16(ptr(qkv), 3 * W, L * 3 * W, ptr(qkv), 3 * W, W, 2 * W, ptr(out), B, L, L, H, 64,
                                                     int(causal), stream()), "pclip_attention_long_q_f16")
        return out
    check(_lib.load().pclip_attention_f16(ptr(qkv), ptr(out), B, L, H, 64, int(causal), stream()),
          "pclip_attention_f16")
    return out


def attention_first_queries(q, kv, B: int, L: int, Lq: int, H: int):
    """Attention output of the first Lq tokens only: q [B*Lq, W] (projected queries of those tokens), kv [B*L, 2W] (keys |
    values of every token).  Same arithmetic per query row as `attention`, and the same kernel choice (by L alone)."""
    require_cuda(q, kv)
    W = H * 64
    out = torch.empty(B * Lq, W, dtype=torch.float16, device=q.device)
    fn = "pclip_attention_long_q_f16" if L > ATT_SHORT_MAX_L else "pclip_attention_q_f16"
    check(getattr(_lib.load(), fn)(ptr(q), W, Lq * W, ptr(kv), 2 * W, 0, W, ptr(out), B, L, Lq, H, 64, 0, stream()), fn)
    return out


def cast_f16(x: torch.Tensor) -> torch.Tensor:
    require_cuda(x)
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_cast_f32_f16(ptr(x), ptr(y), x.numel(), stream()), "pclip_cast_f32_f16")
    return y


def im2col_patches(img: torch.Tensor, P: int) -> torch.Tensor:
    require_cuda(img)
    B, C, R, _ = img.shape
    G = R // P
    ld = (3 * P * P + 63) // 64 * 64        # K padded to the GEMM's K-tile (ViT-L/14: 588 -> 640)
    cols = torch.empty(B * G * G, ld, dtype=torch.float16, device=img.device)
    if img.dtype == torch.float32:             # fused with the cast to fp16 (clip/model.py:339)
        check(_lib.load().pclip_im2col_patches_f32(ptr(img), B, R, P, ptr(cols), ld, stream()), "pclip_im2col_patches_f32")
        return cols
    check(_lib.load().pclip_im2col_patches_f16(ptr(img), B, R, P, ptr(cols), ld, stream()),
          "pclip_im2col_patches_f16")
    return cols


def vit_assemble_tokens(patch_emb, class_emb, pos_emb, B: int, G2: int, W: int) -> torch.Tensor:
    tokens = torch.empty(B * (G2 + 1), W, dtype=torch.float16, device=patch_emb.device)
    check(_lib.load().pclip_vit_assemble_tokens_f16(ptr(patch_emb), ptr(class_emb), ptr(pos_emb), B, G2, W,
                                                    ptr(tokens), stream()), "pclip_vit_assemble_tokens_f16")
    return tokens


def vit_embed_ln(patch_emb, class_emb, pos_emb, B: int, G2: int, W: int, g_pre, b_pre, g_1, b_1, eps: float = 1e-5):
    """(x0, h) = (ln_pre(tokens), ln_1(x0)) with tokens = [class ; patches] + pos, one pass (clip/model.py:225-227, 188)."""
    R = B * (G2 + 1)
    x0 = torch.empty(R, W, dtype=torch.float16, device=patch_emb.device)
    f = lambda t: t if t is None or t.dtype == torch.float32 else t.float()
    g_pre, b_pre, g_1, b_1 = f(g_pre), f(b_pre), f(g_1), f(b_1)
    h = torch.empty_like(x0)
    check(_lib.load().pclip_vit_embed_ln_f16(ptr(patch_emb), ptr(class_emb), ptr(pos_emb), B, G2, W, ptr(g_pre), ptr(b_pre), ptr(g_1),
                                             ptr(b_1), eps, ptr(x0), ptr(h), stream()), "pclip_vit_embed_ln_f16")
    return x0, h


def text_embed(tokens, tok_emb, pos_emb) -> torch.Tensor:
    require_cuda(tokens, tok_emb)
    B, L = tokens.shape
    vocab, W = tok_emb.shape
    tokens = tokens.to(torch.int64).contiguous()
    x = torch.empty(B * L, W, dtype=torch.float16, device=tok_emb.device)
    check(_lib.load().pclip_text_embed_f16(ptr(tokens), ptr(tok_emb), ptr(pos_emb), B, L, W, vocab, ptr(x),
                                           stream()), "pclip_text_embed_f16")
    return x


EMBED_BWD_CHUNK = _lib.EMBED_BWD_CHUNK      # sorted rows per chunk of text_embed_backward's segmented reduction (PCLIP_EMBED_BWD_CHUNK)
EMBED_BWD_MAX_L, EMBED_BWD_MAX_W = 4096, 2048


def _embed_bwd_envelope(what: str, B: int, L: int, W: int):
    if not (B >= 1 and 1 <= L <= EMBED_BWD_MAX_L and W >= 64 and W % 64 == 0 and W <= EMBED_BWD_MAX_W):
        raise _lib.PclipError(f"{what}: B={B} L={L} W={W} outside the envelope (B >= 1, 1 <= L <= {EMBED_BWD_MAX_L}, W % 64 == 0, W <= {EMBED_BWD_MAX_W})")


def text_embed_backward(dx, tokens, vocab: int, want_emb: bool = True, want_pos: bool = True):
    """Backward of `text_embed` from dx [B * L, W] fp16 and tokens [B, L] int64: (dE [vocab, W], dpos [L, W]), fp32, None where not wanted
    (pclip_text_embed_backward).  dE is dense: a row whose id does not occur is exactly zero.  torch's stable sort of the flat ids is the plumbing
    of the segmented reduction (no host synchronisation); ids are clamped to the vocabulary as the forward clamps them."""
    require_cuda(dx, tokens)
    dx = _f16c(dx)
    if tokens.dim() != 2 or tokens.dtype != torch.int64:
        raise _lib.PclipError(f"text_embed_backward: tokens must be int64 [B, L], got {tokens.dtype} {tuple(tokens.shape)}")
    B, L = tokens.shape
    W = dx.shape[-1]
    _embed_bwd_envelope("text_embed_backward", B, L, W)
    if dx.dim() != 2 or dx.shape[0] != B * L:
        raise _lib.PclipError(f"text_embed_backward: dx {tuple(dx.shape)} does not hold B * L = {B * L} rows")
    if vocab < 1:
        raise _lib.PclipError(f"text_embed_backward: vocab={vocab}")
    if not (want_emb or want_pos):
        return None, None
    dE = ids = order = part = None
    if want_emb:
        ids, order = torch.sort(tokens.reshape(-1).clamp(0, vocab - 1), stable=True)
        dE = torch.empty(vocab, W, dtype=torch.float32, device=dx.device)
        part = torch.empty((B * L + EMBED_BWD_CHUNK - 1) // EMBED_BWD_CHUNK, 2, W, dtype=torch.float32, device=dx.device)
    dpos = torch.empty(L, W, dtype=torch.float32, device=dx.device) if want_pos else None
    check(_lib.load().pclip_text_embed_backward(ptr(dx), ptr(ids), ptr(order), B, L, W, vocab, ptr(dE), ptr(dpos), ptr(part), stream()),
          "pclip_text_embed_backward")
    return dE, dpos


def vit_embed_backward(dt, B: int, L: int, want_pos: bool = True, want_patch: bool = True):
    """Backward of `vit_assemble_tokens` from dt [B * L, W] fp16 (the gradient of the assembled tokens), one pass: (dpos [L, W] fp32 — row 0 is also
    the class embedding's gradient —, dpatch [B * (L - 1), W] fp16, bit-exact copies of the non-class rows), None where not wanted
    (pclip_vit_embed_backward_f16)."""
    require_cuda(dt)
    dt = _f16c(dt)
    W = dt.shape[-1]
    _embed_bwd_envelope("vit_embed_backward", B, L, W)
    if dt.numel() != B * L * W:
        raise _lib.PclipError(f"vit_embed_backward: dt {tuple(dt.shape)} does not hold B * L = {B * L} rows")
    if not (want_pos or want_patch):
        return None, None
    dpos = torch.empty(L, W, dtype=torch.float32, device=dt.device) if want_pos else None
    dpatch = torch.empty(B * (L - 1), W, dtype=torch.float16, device=dt.device) if want_patch else None
    if dpos is None and L == 1:                 # no patch rows and no sum wanted: nothing to launch
        return None, dpatch
    check(_lib.load().pclip_vit_embed_backward_f16(ptr(dt), B, L, W, ptr(dpos), ptr(dpatch) if want_patch and L > 1 else None, stream()),
          "pclip_vit_embed_backward_f16")
    return dpos, dpatch


def _prompt_ctx_shape(ctx, N: int, W: int):
    """(n_ctx, class_specific) of a context tensor: fp32 [n_ctx, W] shared, or [N, n_ctx, W]."""
    if ctx.dtype != torch.float32:
        raise _lib.PclipError(f"prompt context must be float32, got {ctx.dtype}")
    if ctx.dim() not in (2, 3) or ctx.shape[-1] != W or (ctx.dim() == 3 and ctx.shape[0] != N):
        raise _lib.PclipError(f"prompt context {tuple(ctx.shape)} is neither [n_ctx, {W}] nor [{N}, n_ctx, {W}]")
    return ctx.shape[-2], ctx.dim() == 3


def prompt_embed(ctx, tokens, tok_emb, pos_emb, L_out: int = None) -> torch.Tensor:
    """Embedded prompts [N * L_out, W] fp16 with the fp32 context rows `ctx` ([n_ctx, W] shared or [N, n_ctx, W]) at positions 1 .. n_ctx and the
    token embeddings elsewhere, plus the positional embedding (pclip_prompt_embed_f16).  L_out <= tokens.shape[1]: the first L_out positions only."""
    require_cuda(ctx, tokens, tok_emb, pos_emb)
    N, L_tok = tokens.shape
    vocab, W = tok_emb.shape
    L_out = L_tok if L_out is None else int(L_out)
    n_ctx, per_class = _prompt_ctx_shape(ctx, N, W)
    if not 1 <= L_out <= L_tok or pos_emb.shape[0] < L_out or pos_emb.shape[1] != W:
        raise _lib.PclipError(f"prompt_embed: L_out={L_out} with tokens {tuple(tokens.shape)} and positional rows {tuple(pos_emb.shape)}")
    tokens = tokens.to(torch.int64).contiguous()
    ctx, tok_emb, pos_emb = ctx.contiguous(), _f16c(tok_emb), _f16c(pos_emb)
    x = torch.empty(N * L_out, W, dtype=torch.float16, device=tok_emb.device)
    check(_lib.load().pclip_prompt_embed_f16(ptr(tokens), L_tok, ptr(tok_emb), ptr(pos_emb), ptr(ctx), int(per_class), n_ctx, N, L_out, W, vocab,
                                             ptr(x), stream()), "pclip_prompt_embed_f16")
    return x


def prompt_ctx_grad(dx, N: int, L_out: int, n_ctx: int, class_specific: bool = False) -> torch.Tensor:
    """Gradient of `prompt_embed` wrt the context from dx [N * L_out, W] fp16: fp32 [n_ctx, W] (summed over the classes by the slice-sum rule, `rows_grad`
    at off = 1) or, class specific, [N, n_ctx, W] (pclip_prompt_ctx_grad_f32).  A context row at 1 + j >= L_out is not read: its gradient is 0."""
    require_cuda(dx)
    dx = _f16c(dx)
    W = dx.shape[1]
    if dx.shape[0] != N * L_out:
        raise _lib.PclipError(f"prompt_ctx_grad: dx has {dx.shape[0]} rows, expected N * L_out = {N * L_out}")
    if class_specific:
        dctx = torch.empty(N, n_ctx, W, dtype=torch.float32, device=dx.device)
        part, nslice = None, 0
    else:
        dctx = torch.empty(n_ctx, W, dtype=torch.float32, device=dx.device)
        nslice = (N + _lib.PROMPT_CTX_SLICE - 1) // _lib.PROMPT_CTX_SLICE
        part = torch.empty(nslice, n_ctx * W, dtype=torch.float32, device=dx.device) if nslice > 1 else None
    check(_lib.load().pclip_prompt_ctx_grad_f32(ptr(dx), N, L_out, n_ctx, W, int(class_specific), ptr(dctx), ptr(part), nslice, stream()),
          "pclip_prompt_ctx_grad_f32")
    return dctx


def _vpt_ctx(who: str, ctx, W: int):
    """The fp32 [P, W] prompt rows of one layer, contiguous."""
    if ctx.dtype != torch.float32:
        raise _lib.PclipError(f"{who}: visual prompt rows must be float32, got {ctx.dtype}")
    if ctx.dim() != 2 or ctx.shape[1] != W or ctx.shape[0] < 1:
        raise _lib.PclipError(f"{who}: visual prompt rows {tuple(ctx.shape)} are not [P, {W}] with P >= 1")
    return ctx.contiguous()


def vpt_append(t, ctx, B: int, L0: int) -> torch.Tensor:
    """[B * (L0 + P), W] fp16: every sequence's L0 rows of t [B * L0, W] followed by the fp32 prompt rows ctx [P, W] rounded once to fp16 — the bits of
    torch.cat([t.view(B, L0, W), ctx.half().expand(B, P, W)], 1) (pclip_vpt_append_f16).  L0 == 0 (t may be None): the broadcast rows alone."""
    require_cuda(t, ctx)
    W = ctx.shape[-1]
    ctx = _vpt_ctx("vpt_append", ctx, W)
    P = ctx.shape[0]
    if L0 > 0:
        t = _f16c(t)
        if t.dim() != 2 or t.shape != (B * L0, W):
            raise _lib.PclipError(f"vpt_append: t {tuple(t.shape)} is not [B * L0, W] = [{B * L0}, {W}]")
    out = torch.empty(B * (L0 + P), W, dtype=torch.float16, device=ctx.device)
    check(_lib.load().pclip_vpt_append_f16(ptr(t) if L0 > 0 else None, ptr(ctx), B, L0, P, W, ptr(out), stream()), "pclip_vpt_append_f16")
    return out


def vpt_replace_(x, ctx, B: int, L0: int) -> torch.Tensor:
    """In place on the stream x [B * (L0 + P), W] fp16: the last P rows of every sequence become the fp32 rows ctx [P, W] rounded once to fp16
    (pclip_vpt_replace_f16): `rows_replace_` at L = L0 + P, off = L0.  Returns x."""
    require_cuda(x, ctx)
    W = x.shape[-1]
    ctx = _vpt_ctx("vpt_replace_", ctx, W)
    P = ctx.shape[0]
    if x.dtype != torch.float16 or not x.is_contiguous() or x.dim() != 2 or x.shape[0] != B * (L0 + P):
        raise _lib.PclipError(f"vpt_replace_: x {x.dtype} {tuple(x.shape)} is not a contiguous float16 [B * (L0 + P), W] = [{B * (L0 + P)}, {W}]")
    check(_lib.load().pclip_vpt_replace_f16(ptr(x), ptr(ctx), B, L0, P, W, stream()), "pclip_vpt_replace_f16")
    return x


def vpt_grad(g, B: int, L0: int, P: int, clear: bool = False) -> torch.Tensor:
    """fp32 [P, W]: the prompt rows (L0 .. L0 + P - 1 of every sequence) of the gradient stream g [B * (L0 + P), W] fp16 summed over the B sequences
    by the slice-sum rule (`rows_grad` at L = L0 + P, off = L0; pclip_vpt_grad_f32).  L0 == 0: g is a compact [B * P, W].  clear: the pass also writes
    exact zeros over those rows of g, IN PLACE."""
    require_cuda(g)
    if g.dtype != torch.float16 or not g.is_contiguous() or g.dim() != 2 or g.shape[0] != B * (L0 + P):
        raise _lib.PclipError(f"vpt_grad: g {g.dtype} {tuple(g.shape)} is not a contiguous float16 [B * (L0 + P), W] with B={B}, L0={L0}, P={P}")
    W = g.shape[1]
    dctx = torch.empty(P, W, dtype=torch.float32, device=g.device) if B > 0 else torch.zeros(P, W, dtype=torch.float32, device=g.device)
    nslice = (B + _lib.VPT_SLICE - 1) // _lib.VPT_SLICE
    part = torch.empty(nslice, P * W, dtype=torch.float32, device=g.device) if nslice > 1 else None      # the kernel's workspace
    check(_lib.load().pclip_vpt_grad_f32(ptr(g), B, L0, P, W, int(bool(clear)), ptr(dctx), ptr(part), nslice, stream()), "pclip_vpt_grad_f32")
    return dctx


def _rows_window(who: str, t, B: int, L: int, off: int, P: int):
    """The stream operand of the rows-at-an-offset passes: contiguous fp16 [B * L, W] with the window off .. off + P - 1 inside a sequence."""
    if t.dtype != torch.float16 or not t.is_contiguous() or t.dim() != 2 or t.shape[0] != B * L:
        raise _lib.PclipError(f"{who}: {t.dtype} {tuple(t.shape)} is not a contiguous float16 [B * L, W] with B={B}, L={L}")
    if off < 0 or P < 1 or off + P > L:
        raise _lib.PclipError(f"{who}: rows off .. off + P - 1 = {off} .. {off + P - 1} do not lie inside a sequence of L={L} rows")


def rows_replace_(x, ctx, B: int, L: int, off: int) -> torch.Tensor:
    """In place on the stream x [B * L, W] fp16: rows off .. off + P - 1 of every sequence become the fp32 rows ctx [P, W] rounded once to fp16
    (pclip_rows_replace_f16); every other row keeps its bits.  Returns x.  The deep-prompt pack of the taped tower (autograd.TowerTailFn) goes through
    this entry for either tower; off = L - P is `vpt_replace_`."""
    require_cuda(x, ctx)
    W = x.shape[-1]
    ctx = _vpt_ctx("rows_replace_", ctx, W)
    P = ctx.shape[0]
    B, L, off = int(B), int(L), int(off)
    _rows_window("rows_replace_: x", x, B, L, off, P)
    check(_lib.load().pclip_rows_replace_f16(ptr(x), ptr(ctx), B, L, off, P, W, stream()), "pclip_rows_replace_f16")
    return x


def rows_grad(g, B: int, L: int, off: int, P: int, clear: bool = False) -> torch.Tensor:
    """fp32 [P, W]: rows off .. off + P - 1 of every sequence of the gradient stream g [B * L, W] fp16 summed over the B sequences by the slice-sum rule
    (pclip_rows_grad_f32; include/pclip.h states the rule: slices of 16 sequences in ascending order, then the slices in ascending order, fp32).  clear: the
    pass also writes exact zeros over those rows of g, IN PLACE — the rows of a replaced deep prompt pass no gradient to the block below; rows outside the
    window are neither read nor written.  off = L - P is `vpt_grad`."""
    require_cuda(g)
    B, L, off, P = int(B), int(L), int(off), int(P)
    _rows_window("rows_grad: g", g, B, L, off, P)
    W = g.shape[1]
    dctx = torch.empty(P, W, dtype=torch.float32, device=g.device) if B > 0 else torch.zeros(P, W, dtype=torch.float32, device=g.device)
    nslice = (B + _lib.VPT_SLICE - 1) // _lib.VPT_SLICE
    part = torch.empty(nslice, P * W, dtype=torch.float32, device=g.device) if nslice > 1 else None      # the kernel's workspace
    check(_lib.load().pclip_rows_grad_f32(ptr(g), B, L, off, P, W, int(bool(clear)), ptr(dctx), ptr(part), nslice, stream()), "pclip_rows_grad_f32")
    return dctx


def _couple_f32(who: str, name: str, t, shape):
    """An fp32 operand of the coupling function: dtype and shape checked, contiguous."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise _lib.PclipError(f"{who}: {name} must be float32, got {getattr(t, 'dtype', type(t))}")
    if tuple(t.shape) != tuple(shape):
        raise _lib.PclipError(f"{who}: {name} {tuple(t.shape)} is not {list(shape)}")
    return t.contiguous()


def _couple_dims(who: str, rows, weight):
    if rows.dim() != 3 or weight.dim() != 3:
        raise _lib.PclipError(f"{who}: rows {tuple(rows.shape)} / weight {tuple(weight.shape)} are not [depth, P, W] / [depth, Wv, Wt]")
    return rows.shape[0], rows.shape[1], weight.shape[2], weight.shape[1]


def couple(x, weight, bias) -> torch.Tensor:
    """The coupling function of every depth in one launch: y [depth, P, Wv] fp32 = x[d] @ weight[d].T + bias[d] for x [depth, P, Wt], weight
    [depth, Wv, Wt], bias [depth, Wv], all fp32 (pclip_couple_fwd_f32: 1 <= P <= 16, Wt % 64 == 0, Wv % 8 == 0; one fixed summation order)."""
    require_cuda(x, weight, bias)
    depth, P, Wt, Wv = _couple_dims("couple", x, weight)
    x = _couple_f32("couple", "x", x, (depth, P, Wt))
    weight = _couple_f32("couple", "weight", weight, (depth, Wv, Wt))
    bias = _couple_f32("couple", "bias", bias, (depth, Wv))
    y = torch.empty(depth, P, Wv, dtype=torch.float32, device=x.device)
    check(_lib.load().pclip_couple_fwd_f32(ptr(x), ptr(weight), ptr(bias), depth, P, Wt, Wv, ptr(y), stream()), "pclip_couple_fwd_f32")
    return y


def couple_backward(dy, x, weight, want_x: bool = True, want_weight: bool = True, want_bias: bool = True):
    """(dx, dweight, dbias) of `couple` from dy [depth, P, Wv] fp32 — dx = dy[d] @ weight[d], dweight = dy[d].T @ x[d], dbias = dy[d].sum(0) — each
    None when not wanted: nothing is launched or allocated for it (pclip_couple_bwd_f32: at most two launches and one merge)."""
    require_cuda(dy, x, weight)
    depth, P, Wt, Wv = _couple_dims("couple_backward", x, weight)
    dy = _couple_f32("couple_backward", "dy", dy, (depth, P, Wv))
    x = _couple_f32("couple_backward", "x", x, (depth, P, Wt))
    weight = _couple_f32("couple_backward", "weight", weight, (depth, Wv, Wt))
    dev = dy.device
    dx = torch.empty(depth, P, Wt, dtype=torch.float32, device=dev) if want_x else None
    dw = torch.empty(depth, Wv, Wt, dtype=torch.float32, device=dev) if want_weight else None
    db = torch.empty(depth, Wv, dtype=torch.float32, device=dev) if want_bias else None
    nslice = (Wv + _lib.COUPLE_SLICE - 1) // _lib.COUPLE_SLICE
    part = torch.empty(depth, nslice, P * Wt, dtype=torch.float32, device=dev) if want_x and nslice > 1 else None      # the kernel's workspace
    if want_x or want_weight or want_bias:
        check(_lib.load().pclip_couple_bwd_f32(ptr(dy), ptr(x), ptr(weight), depth, P, Wt, Wv, ptr(dw), ptr(db), ptr(dx), ptr(part), nslice, stream()),
              "pclip_couple_bwd_f32")
    return dx, dw, db


def _metanet_dims(who: str, f, w1, w2):
    """(B, E, Hd, Wt) of a meta-net call, with the envelope of pclip_metanet_fwd_f32 checked on the host (the shapes alone: before any device is asked
    for)."""
    if f.dim() != 2 or w1.dim() != 2 or w2.dim() != 2:
        raise _lib.PclipError(f"{who}: features {tuple(f.shape)} / W1 {tuple(w1.shape)} / W2 {tuple(w2.shape)} are not [B, E] / [Hd, E] / [Wt, Hd]")
    B, E = f.shape
    Hd, Wt = w1.shape[0], w2.shape[0]
    if w1.shape[1] != E or w2.shape[1] != Hd:
        raise _lib.PclipError(f"{who}: W1 {tuple(w1.shape)} / W2 {tuple(w2.shape)} do not chain with features of E={E} (W1 [Hd, E], W2 [Wt, Hd])")
    if E < 64 or E % 64 != 0:
        raise _lib.PclipError(f"{who}: E={E} must be a positive multiple of 64 (a quarter wave reads 64 columns per step)")
    if not 4 <= Hd <= 256 or Hd % 4 != 0:
        raise _lib.PclipError(f"{who}: Hd={Hd} must be a multiple of 4 in 4 .. 256")
    if Wt < 8 or Wt % 8 != 0:
        raise _lib.PclipError(f"{who}: Wt={Wt} must be a positive multiple of 8")
    if not 1 <= B <= _lib.COCOOP_MAX_B:
        raise _lib.PclipError(f"{who}: B={B} images outside 1 .. {_lib.COCOOP_MAX_B} (chunk the images; cocoop.ConditionalPromptLearner does)")
    return B, E, Hd, Wt


def metanet(f, w1, b1, w2, b2):
    """CoCoOp's meta-net: (h [B, Hd], pi [B, Wt]) fp32 = (relu(f @ w1.T + b1), h @ w2.T + b2) for f [B, E] fp16 (normalised features, a constant) and
    fp32 w1 [Hd, E], b1 [Hd], w2 [Wt, Hd], b2 [Wt] (pclip_metanet_fwd_f32: 1 <= B <= 16, E % 64 == 0, Hd % 4 == 0 in 4 .. 256, Wt % 8 == 0; two
    launches, one fixed summation order).  h is what `metanet_backward` reads."""
    B, E, Hd, Wt = _metanet_dims("metanet", f, w1, w2)
    require_cuda(f, w1, b1, w2, b2)
    f = _f16c(f)
    w1, b1 = _couple_f32("metanet", "w1", w1, (Hd, E)), _couple_f32("metanet", "b1", b1, (Hd,))
    w2, b2 = _couple_f32("metanet", "w2", w2, (Wt, Hd)), _couple_f32("metanet", "b2", b2, (Wt,))
    h = torch.empty(B, Hd, dtype=torch.float32, device=f.device)
    pi = torch.empty(B, Wt, dtype=torch.float32, device=f.device)
    check(_lib.load().pclip_metanet_fwd_f32(ptr(f), ptr(w1), ptr(b1), ptr(w2), ptr(b2), B, E, Hd, Wt, ptr(h), ptr(pi), stream()), "pclip_metanet_fwd_f32")
    return h, pi


def metanet_backward(dpi, f, h, w1, w2, want_w1: bool = True, want_b1: bool = True, want_w2: bool = True, want_b2: bool = True):
    """(dw1, db1, dw2, db2) of `metanet` from dpi [B, Wt] fp32 — dw2 = dpi.T @ h, db2 = dpi.sum(0), dpre = (dpi @ w2) * (h > 0), dw1 = dpre.T @ f,
    db1 = dpre.sum(0) — each None when not wanted: nothing is launched or allocated for it (pclip_metanet_bwd_f32: at most three launches).  f is a
    constant and gets no gradient."""
    B, E, Hd, Wt = _metanet_dims("metanet_backward", f, w1, w2)
    require_cuda(dpi, f, h, w1, w2)
    f = _f16c(f)
    dpi = _couple_f32("metanet_backward", "dpi", dpi, (B, Wt))
    h = _couple_f32("metanet_backward", "h", h, (B, Hd))
    w2 = _couple_f32("metanet_backward", "w2", w2, (Wt, Hd))
    dev = dpi.device
    new = lambda want, *shape: torch.empty(*shape, dtype=torch.float32, device=dev) if want else None      # noqa: E731
    dw1, db1, dw2, db2 = new(want_w1, Hd, E), new(want_b1, Hd), new(want_w2, Wt, Hd), new(want_b2, Wt)
    dpre = new(want_w1 or want_b1, B, Hd)                                        # the kernel's workspace
    if want_w1 or want_b1 or want_w2 or want_b2:
        check(_lib.load().pclip_metanet_bwd_f32(ptr(dpi), ptr(f), ptr(h), ptr(w2), B, E, Hd, Wt, ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), ptr(dpre),
                                                stream()), "pclip_metanet_bwd_f32")
    return dw1, db1, dw2, db2


def _cond_ctx(who: str, ctx, pi, W: int):
    """(n_ctx, B) of a conditional assembly: the shared fp32 context [n_ctx, W] and the per-image shifts [B, W]."""
    for name, t in (("ctx", ctx), ("pi", pi)):
        if t.dtype != torch.float32:
            raise _lib.PclipError(f"{who}: {name} must be float32, got {t.dtype}")
    if ctx.dim() != 2 or ctx.shape[1] != W or ctx.shape[0] < 1 or pi.dim() != 2 or pi.shape[1] != W:
        raise _lib.PclipError(f"{who}: ctx {tuple(ctx.shape)} / pi {tuple(pi.shape)} are not [n_ctx, {W}] / [B, {W}]")
    B = pi.shape[0]
    if not 1 <= B <= _lib.COCOOP_MAX_B:
        raise _lib.PclipError(f"{who}: B={B} images outside 1 .. {_lib.COCOOP_MAX_B} (chunk the images; cocoop.ConditionalPromptLearner does)")
    return ctx.shape[0], B


def prompt_embed_cond(ctx, pi, tokens, tok_emb, pos_emb, L_out: int = None) -> torch.Tensor:
    """Embedded prompts [B * N * L_out, W] fp16 of B images x N classes: `prompt_embed` with the context rows r16(ctx[j] + pi[b]) — ctx fp32 [n_ctx, W]
    shared, pi fp32 [B, W] per image — in the prompts b * N .. b * N + N - 1 (pclip_prompt_embed_cond_f16).  tokens [N, L_tok] are shared by the images."""
    N, L_tok = tokens.shape
    vocab, W = tok_emb.shape
    L_out = L_tok if L_out is None else int(L_out)
    n_ctx, B = _cond_ctx("prompt_embed_cond", ctx, pi, W)
    if not 1 <= L_out <= L_tok or pos_emb.shape[0] < L_out or pos_emb.shape[1] != W or N < 1:
        raise _lib.PclipError(f"prompt_embed_cond: L_out={L_out} with tokens {tuple(tokens.shape)} and positional rows {tuple(pos_emb.shape)}")
    require_cuda(ctx, pi, tokens, tok_emb, pos_emb)
    tokens = tokens.to(torch.int64).contiguous()
    ctx, pi, tok_emb, pos_emb = ctx.contiguous(), pi.contiguous(), _f16c(tok_emb), _f16c(pos_emb)
    x = torch.empty(B * N * L_out, W, dtype=torch.float16, device=tok_emb.device)
    check(_lib.load().pclip_prompt_embed_cond_f16(ptr(tokens), L_tok, ptr(tok_emb), ptr(pos_emb), ptr(ctx), ptr(pi), n_ctx, B, N, L_out, W, vocab, ptr(x),
                                                  stream()), "pclip_prompt_embed_cond_f16")
    return x


def prompt_cond_grad(dx, B: int, N: int, L_out: int, n_ctx: int):
    """(dctx [n_ctx, W], dpi [B, W], dshift [B, n_ctx, W]) fp32, the gradient of `prompt_embed_cond` from dx [B * N * L_out, W] fp16: dshift[b] is
    `prompt_ctx_grad` of image b's N prompts (the slice-sum rule), dctx its sum over the images in ascending order, dpi[b] its sum over the context rows
    in ascending order (pclip_prompt_cond_grad_f32: two launches).  A context row at 1 + j >= L_out is not read: its dshift is 0."""
    B, N, L_out, n_ctx = int(B), int(N), int(L_out), int(n_ctx)
    if not 1 <= B <= _lib.COCOOP_MAX_B:
        raise _lib.PclipError(f"prompt_cond_grad: B={B} images outside 1 .. {_lib.COCOOP_MAX_B}")
    if dx.dim() != 2 or dx.shape[0] != B * N * L_out or N < 1 or L_out < 1 or n_ctx < 1:
        raise _lib.PclipError(f"prompt_cond_grad: dx {tuple(dx.shape)} has not B * N * L_out = {B} * {N} * {L_out} rows (n_ctx={n_ctx})")
    require_cuda(dx)
    dx = _f16c(dx)
    W = dx.shape[1]
    dev = dx.device
    dshift = torch.empty(B, n_ctx, W, dtype=torch.float32, device=dev)
    dctx = torch.empty(n_ctx, W, dtype=torch.float32, device=dev)
    dpi = torch.empty(B, W, dtype=torch.float32, device=dev)
    nslice = (N + _lib.PROMPT_CTX_SLICE - 1) // _lib.PROMPT_CTX_SLICE
    part = torch.empty(B, nslice, n_ctx * W, dtype=torch.float32, device=dev) if nslice > 1 else None      # the kernel's workspace
    check(_lib.load().pclip_prompt_cond_grad_f32(ptr(dx), B, N, L_out, n_ctx, W, ptr(dshift), ptr(dctx), ptr(dpi), ptr(part), nslice, stream()),
          "pclip_prompt_cond_grad_f32")
    return dctx, dpi, dshift


def gather_eot(x, tokens, B: int, L: int, W: int) -> torch.Tensor:
    tokens = tokens.to(torch.int64).contiguous()
    out = torch.empty(B, W, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_gather_eot_f16(ptr(x), ptr(tokens), B, L, W, ptr(out), stream()), "pclip_gather_eot_f16")
    return out


# ---- ModifiedResNet building blocks (activations NHWC fp16) ---------------------------------------------

def im2col3x3(x, strides, B: int, H: int, W: int, C: int, stride: int = 1) -> torch.Tensor:
    """[B*Ho*Wo, round_up(9*C, 64)] fp16 rows for a 3x3 / pad 1 convolution; `strides` = element strides
    (batch, y, x, channel) of the input buffer."""
    require_cuda(x)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    ld = (9 * C + 63) // 64 * 64
    cols = torch.empty(B * Ho * Wo, ld, dtype=torch.float16, device=x.device)
    sb, sh, sw, sc = strides
    check(_lib.load().pclip_im2col3x3_f16(ptr(x), sb, sh, sw, sc, B, H, W, C, stride, ptr(cols), ld, stream()),
          "pclip_im2col3x3_f16")
    return cols


def bn_act(x, scale, shift, residual=None, relu: bool = True, out=None) -> torch.Tensor:
    require_cuda(x, scale, shift, residual)
    rows, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(_lib.load().pclip_bn_act_f16(ptr(x), ptr(scale), ptr(shift), ptr(residual), int(relu), ptr(out), rows, C, stream()),
          "pclip_bn_act_f16")
    return out


def avgpool_nhwc(x, B: int, H: int, W: int, C: int, k: int) -> torch.Tensor:
    require_cuda(x)
    y = torch.empty(B * (H // k) * (W // k), C, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_avgpool_nhwc_f16(ptr(x), B, H, W, C, k, ptr(y), stream()), "pclip_avgpool_nhwc_f16")
    return y


def attnpool_tokens(x, pos16, B: int, HW: int, C: int) -> torch.Tensor:
    require_cuda(x, pos16)
    t = torch.empty(B * (HW + 1), C, dtype=torch.float16, device=x.device)
    check(_lib.load().pclip_attnpool_tokens_f16(ptr(x), ptr(pos16), B, HW, C, ptr(t), stream()), "pclip_attnpool_tokens_f16")
    return t


# ---------------------------------------------------------------- training step (csrc/pclip_train.hip) ----------
def cast_f32(x: torch.Tensor) -> torch.Tensor:
    """fp16 -> fp32 copy (`.float()`)."""
    require_cuda(x)
    x = _f16c(x)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(_lib.load().pclip_cast_f16_f32(ptr(x), ptr(y), x.numel(), stream()), "pclip_cast_f16_f32")
    return y


def _f32_rows(who: str, name: str, t: torch.Tensor, shape=None):
    """Refuse an operand that is not a device fp32 tensor with unit stride along its last axis (and of `shape`, when given): the entries take a pointer and a
    row stride only."""
    require_cuda(t)
    if t.dtype != torch.float32 or (shape is not None and tuple(t.shape) != tuple(shape)) or (t.dim() > 0 and t.stride(-1) != 1 and t.shape[-1] > 1):
        want = "fp32" + (f" {list(shape)}" if shape is not None else "")
        raise _lib.PclipError(f"{who}: `{name}` must be a {want} tensor with unit column stride (got {t.dtype} {list(t.shape)}, strides {list(t.stride())})")


def gemm_f32(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False, alpha: float = 1.0,
             out: torch.Tensor = None, beta: float = 0.0) -> torch.Tensor:
    """out = alpha * op(a) @ op(b) + beta * out in fp32 on the fp32 MFMA; a, b are 2-D row-major (unit column stride, any
    row stride) fp16 or fp32."""
    require_cuda(a, b)
    for t in (a, b):
        if t.dtype not in (torch.float16, torch.float32) or t.dim() != 2 or t.stride(1) != 1:
            raise _lib.PclipError("gemm_f32 takes row-major 2-D fp16/fp32 tensors")
    M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    Kb, N = (b.shape[1], b.shape[0]) if trans_b else b.shape
    if K != Kb:
        raise _lib.PclipError(f"gemm_f32: inner dimensions differ ({K} vs {Kb})")
    rsa, csa = (1, a.stride(0)) if trans_a else (a.stride(0), 1)
    rsb, csb = (1, b.stride(0)) if trans_b else (b.stride(0), 1)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
        beta = 0.0
    else:
        _f32_rows("gemm_f32", "out", out, (M, N))
    ws = _workspace(32 * M * N * 4, a.device) if K >= 1024 and ((M + 63) // 64) * ((N + 63) // 64) <= 128 else None
    check(_lib.load().pclip_gemm_f32(ptr(a), int(a.dtype == torch.float16), rsa, csa, ptr(b), int(b.dtype == torch.float16),
                                     rsb, csb, ptr(out), out.stride(0), M, N, K, alpha, beta, ptr(ws),
                                     ws.numel() if ws is not None else 0, stream()), "pclip_gemm_f32")
    return out


def colsum_f32(x: torch.Tensor, rows: int = None, cols: int = None, scale: float = 1.0, out: torch.Tensor = None) -> torch.Tensor:
    """scale * x.sum(0) for a 2-D fp32 tensor (leading dimension = x.stride(0)); deterministic.  With `out` the sum is
    ADDED to it."""
    require_cuda(x)
    R = x.shape[0] if rows is None else rows
    C = x.shape[1] if cols is None else cols
    acc = out is not None
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=x.device)
    else:
        require_cuda(out)
        if out.dtype != torch.float32 or out.numel() != C or not out.is_contiguous():
            raise _lib.PclipError(f"colsum_f32: `out` must be a contiguous fp32 tensor of {C} elements (got {out.dtype} {list(out.shape)}, strides {list(out.stride())})")
    ws = _workspace(64 * C * 4, x.device) if R > 128 else None
    check(_lib.load().pclip_colsum_f32(ptr(x), x.stride(0), R, C, scale, ptr(out), int(acc), ptr(ws), ws.numel() if ws is not None else 0,
                                       stream()), "pclip_colsum_f32")
    return out


def addscaled_rows_(c: torch.Tensor, x: torch.Tensor, rowscale: torch.Tensor, s: float) -> torch.Tensor:
    """c[r, :] += s * rowscale[r] * x[r, :] in place (fp32)."""
    require_cuda(c, x, rowscale)
    if c.dim() != 2:
        raise _lib.PclipError(f"addscaled_rows_: `c` must be a 2-D fp32 tensor (got {list(c.shape)})")
    R, D = c.shape
    _f32_rows("addscaled_rows_", "c", c)
    _f32_rows("addscaled_rows_", "x", x, (R, D))
    _f32_rows("addscaled_rows_", "rowscale", rowscale, (R,))
    check(_lib.load().pclip_addscaled_rows_f32(ptr(c), c.stride(0), ptr(x), x.stride(0), ptr(rowscale), s, R, D, stream()),
          "pclip_addscaled_rows_f32")
    return c


def nll_grad(d2i, d2t, labels, N: int, alpha: float, beta: float, q_total: int = None):
    """From the distance rows of sqdist_f32: gradients (gi, gt) of mean NLL(log P) wrt them, rowsum(gi + gt), the per-query
    -log p[y], max probability and argmax — the lowest index among equal maxima — (utils.py:84-93).  gi / gt are padded like the distance rows; the kernel leaves
    their columns >= N untouched."""
    require_cuda(d2i, d2t, labels)
    Q, ldd = d2i.shape
    gi, gt = torch.empty_like(d2i), torch.empty_like(d2t)
    rs, nll, pmax = (torch.empty(Q, dtype=torch.float32, device=d2i.device) for _ in range(3))
    am = torch.empty(Q, dtype=torch.int32, device=d2i.device)
    lab = labels.to(torch.int32)
    check(_lib.load().pclip_nll_grad(ptr(d2i), ptr(d2t), ptr(lab), Q, Q if q_total is None else q_total, N, ldd, alpha, 1.0 - alpha, beta, ptr(gi), ptr(gt),
                                     ptr(rs), ptr(nll), ptr(pmax), ptr(am), stream()), "pclip_nll_grad")
    return gi, gt, rs, nll, pmax, am


def fuse_probs_backward(d2i, d2t, dp, N: int, alpha: float, beta: float):
    """Backward of `fuse_probs` for an arbitrary upstream dp [Q, N] fp32: (gi, gt) wrt the two distance rows (padded like them;
    the kernel leaves columns >= N untouched, here they hold whatever the fresh buffers held) and rowsum(gi + gt) — the autograd-transparent utils.P."""
    require_cuda(d2i, d2t, dp)
    Q, ldd = d2i.shape
    if dp.dtype != torch.float32 or dp.shape != (Q, N) or dp.stride(1) != 1:
        raise _lib.PclipError("fuse_probs_backward: dp must be a row-major fp32 [Q, N] tensor")
    gi, gt = torch.empty_like(d2i), torch.empty_like(d2t)
    rs = torch.empty(Q, dtype=torch.float32, device=d2i.device)
    a32, oma32 = float(np.float32(alpha)), float(np.float32(1 - float(alpha)))
    check(_lib.load().pclip_fuse_probs_backward(ptr(d2i), ptr(d2t), ptr(dp), dp.stride(0), Q, N, ldd, a32, oma32, float(np.float32(beta)),
                                                ptr(gi), ptr(gt), ptr(rs), stream()), "pclip_fuse_probs_backward")
    return gi, gt, rs


def nll_mean_backward(p: torch.Tensor, labels: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """dp of nn.NLLLoss()(torch.log(p), labels) for the upstream gradient g (fp32 device scalar)."""
    require_cuda(p, labels, g)
    Q, N = p.shape
    dp = torch.empty(Q, N, dtype=torch.float32, device=p.device)
    g = g.reshape(1).float().contiguous()
    lab = labels.to(torch.int32)                                    # held in a name: the converted copy must outlive the launch
    check(_lib.load().pclip_nll_mean_backward(ptr(p), p.stride(0), ptr(lab), Q, N, ptr(g), ptr(dp), N, stream()),
          "pclip_nll_mean_backward")
    return dp


def nll_rows(p: torch.Tensor, labels: torch.Tensor):
    """(-log p[q, y_q], max_c p[q, c], argmax_c p[q, c]) per row of a materialised fp32 p [Q, N] (utils.py:84-93)."""
    require_cuda(p, labels)
    if p.dtype != torch.float32 or p.dim() != 2 or p.stride(1) != 1:
        raise _lib.PclipError("nll_rows: p must be a row-major fp32 [Q, N] tensor")
    Q, N = p.shape
    nll, pmax = (torch.empty(Q, dtype=torch.float32, device=p.device) for _ in range(2))
    am = torch.empty(Q, dtype=torch.int32, device=p.device)
    lab = labels.to(torch.int32)
    check(_lib.load().pclip_nll_rows(ptr(p), p.stride(0), ptr(lab), Q, N, ptr(nll), ptr(pmax), ptr(am), stream()), "pclip_nll_rows")
    return nll, pmax, am


def softmax_ce_rows(S: torch.Tensor, scale: float):
    """Rows of S as logits against the diagonal: (per-row loss, scale * (softmax - I))."""
    require_cuda(S)
    R, C = S.shape
    dS = torch.empty_like(S)
    loss = torch.empty(R, dtype=torch.float32, device=S.device)
    check(_lib.load().pclip_softmax_ce_rows(ptr(S), S.stride(0), R, C, scale, ptr(dS), dS.stride(0), ptr(loss), stream()),
          "pclip_softmax_ce_rows")
    return loss, dS


def proto_backward(mem: torch.Tensor, g: torch.Tensor, N: int, K: int, per_shot_norm: bool, final_norm: bool) -> torch.Tensor:
    """Gradient wrt the fp16 rows `mem` [N*K, D] of the prototype chain given g [N, D] fp32 wrt its fp32 output."""
    require_cuda(mem, g)
    mem = _f16c(mem)
    D = mem.shape[1]
    if g.dtype != torch.float32 or g.shape != (N, D) or not g.is_contiguous():
        raise _lib.PclipError("proto_backward: g must be a contiguous fp32 [N, D] tensor")
    dmem = torch.empty_like(mem)
    check(_lib.load().pclip_proto_backward_f16(ptr(mem), ptr(g), N, K, D, int(per_shot_norm), int(final_norm), ptr(dmem),
                                               stream()), "pclip_proto_backward_f16")
    return dmem


def layernorm_backward(x, gamma, dy, eps: float = 1e-5, dy_scale: float = 1.0):
    """fp16 LayerNorm backward over the last dimension: (dx fp16, dgamma fp32 [D], dbeta fp32 [D])."""
    require_cuda(x, gamma, dy)
    x, gamma, dy = _f16c(x), _f16c(gamma), _f16c(dy)
    R, D = x.shape
    nblk = max(1, min(256, (R + 3) // 4))
    dx = torch.empty_like(x)
    part = torch.empty(nblk, 2, D, dtype=torch.float32, device=x.device)
    check(_lib.load().pclip_layernorm_backward_f16(ptr(x), D, ptr(gamma), ptr(dy), D, R, D, eps, dy_scale, ptr(dx), D, ptr(part),
                                                   nblk, stream()), "pclip_layernorm_backward_f16")
    sums = colsum_f32(part.view(nblk, 2 * D))
    return dx, sums[:D], sums[D:]


def attention_backward(qkv, dout, B: int, L: int, H: int, causal: bool = False, dh: int = 64):
    """Gradient of `attention` wrt the fused QKV buffer: qkv [B*L, 3W], dout [B*L, W] -> dqkv [B*L, 3W], fp16 (pclip_attention_backward_f16: S and P are
    recomputed, deterministic).  L <= 288 and head dim 64, like the forward's resident kernels."""
    require_cuda(qkv, dout)
    qkv, dout = _f16c(qkv), _f16c(dout)
    W = H * dh
    if qkv.numel() != B * L * 3 * W or dout.numel() != B * L * W:
        raise _lib.PclipError(f"attention_backward: qkv {tuple(qkv.shape)} / dout {tuple(dout.shape)} do not match B={B} L={L} H={H} dh={dh}")
    dqkv = torch.empty_like(qkv)
    check(_lib.load().pclip_attention_backward_f16(ptr(qkv), ptr(dout), ptr(dqkv), B, L, H, dh, int(causal), stream()),
          "pclip_attention_backward_f16")
    return dqkv


def quick_gelu_backward(u, dy):
    """du = r16(dy * QuickGELU'(u)) on the fp16 pre-activation u (clip/model.py:164-166), derivative in fp32."""
    require_cuda(u, dy)
    u, dy = _f16c(u), _f16c(dy)
    if u.shape != dy.shape:
        raise _lib.PclipError(f"quick_gelu_backward: shapes differ ({tuple(u.shape)} vs {tuple(dy.shape)})")
    du = torch.empty_like(u)
    check(_lib.load().pclip_quick_gelu_backward_f16(ptr(u), ptr(dy), ptr(du), u.numel(), stream()), "pclip_quick_gelu_backward_f16")
    return du


def colsum_f16(x: torch.Tensor) -> torch.Tensor:
    """x.sum(0) of a 2-D fp16 matrix in fp32 (the bias gradient of a linear), in a fixed summation order."""
    require_cuda(x)
    x = _f16c(x)
    R, C = x.shape
    if R == 0:
        return torch.zeros(C, dtype=torch.float32, device=x.device)
    nslice = max(1, min(128, (R + 31) // 32))
    part = torch.empty(nslice, C, dtype=torch.float32, device=x.device)
    check(_lib.load().pclip_colsum_f16(ptr(x), x.stride(0), R, C, ptr(part), nslice, stream()), "pclip_colsum_f16")
    return colsum_f32(part)


def layernorm_backward_f32(x, gamma, dy, eps: float = 1e-5, residual=None):
    """Backward of `layernorm` (fp16 x / dy, fp32 gamma, fp32 statistics): (dx fp16, dgamma fp32 [D], dbeta fp32 [D]); with `residual` (fp16, the
    gradient that passes the LayerNorm on the residual stream) dx = r16(residual + dLN)."""
    require_cuda(x, gamma, dy, residual)
    x, dy = _f16c(x), _f16c(dy)
    if gamma.dtype != torch.float32:
        raise _lib.PclipError(f"layernorm_backward_f32: fp32 gamma expected, got {gamma.dtype}")
    gamma = gamma.contiguous()
    residual = None if residual is None else _f16c(residual)
    R, D = x.shape
    nblk = max(1, min(256, (R + 3) // 4))
    dx = torch.empty_like(x)
    part = torch.empty(nblk, 2, D, dtype=torch.float32, device=x.device)
    check(_lib.load().pclip_layernorm_backward_g32_f16(ptr(x), D, ptr(gamma), ptr(dy), D, ptr(residual), D, R, D, eps, ptr(dx), D, ptr(part),
                                                       nblk, stream()), "pclip_layernorm_backward_g32_f16")
    sums = colsum_f32(part.view(nblk, 2 * D))
    return dx, sums[:D], sums[D:]


def adamw_(p, g, m, v, lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-4,
           weight_decay: float = 0.05):
    """In-place torch.optim.AdamW step on an fp16 parameter with fp16 moments (main.py:134-135)."""
    require_cuda(p, g, m, v)
    for t in (p, g, m, v):
        if t.dtype != torch.float16 or not t.is_contiguous():
            raise _lib.PclipError("adamw_: fp16 contiguous tensors expected")
    check(_lib.load().pclip_adamw_f16(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step,
                                      stream()), "pclip_adamw_f16")
    return p


def _tower_tables(what, table, ntensors, nchunks, state=None, partials=None, hyper=None):
    require_cuda(table, state, partials, hyper)
    if table is not None and (table.dtype != torch.int64 or not table.is_contiguous() or table.numel() < 8 * ntensors):
        raise _lib.PclipError(f"{what}: table must be a contiguous int64 tensor of {ntensors} rows of 8 words")
    if state is not None and (state.dtype != torch.uint8 or not state.is_contiguous() or state.numel() < _lib.TOWER_STATE_BYTES or state.data_ptr() % 8):
        raise _lib.PclipError(f"{what}: state must be a contiguous, 8-byte aligned uint8 tensor of {_lib.TOWER_STATE_BYTES} bytes")
    if partials is not None and (partials.dtype != torch.float32 or not partials.is_contiguous() or partials.numel() < nchunks):
        raise _lib.PclipError(f"{what}: partials must be a contiguous fp32 tensor of at least {nchunks} elements")
    if hyper is not None and (hyper.dtype != torch.float32 or not hyper.is_contiguous() or hyper.numel() < 2 * ntensors):
        raise _lib.PclipError(f"{what}: hyper must be a contiguous fp32 tensor of {ntensors} (lr, weight_decay) pairs")


def tower_grad_sumsq(table, ntensors: int, nchunks: int, partials):
    """Launch 1 of the tower optimizer (optim.TowerAdamW): per-chunk fp32 sums of squares of the raw gradients the table points at."""
    _tower_tables("tower_grad_sumsq", table, ntensors, nchunks, partials=partials)
    check(_lib.load().pclip_tower_grad_sumsq(ptr(table), ntensors, nchunks, ptr(partials), stream()), "pclip_tower_grad_sumsq")
    return partials


def tower_optim_finish(partials, nchunks: int, state, max_norm: float, beta1: float, beta2: float, growth: float = 2.0, backoff: float = 0.5,
                       growth_interval: int = 2000, dynamic: bool = True):
    """Launch 2: overflow flag, unscaled gradient norm, clip coefficient, bias corrections and the loss-scale update, into the state block."""
    _tower_tables("tower_optim_finish", None, 0, nchunks, state=state, partials=partials)
    check(_lib.load().pclip_tower_optim_finish(ptr(partials), nchunks, ptr(state), max_norm, beta1, beta2, growth, backoff, growth_interval,
                                               int(dynamic), stream()), "pclip_tower_optim_finish")
    return state


def tower_adamw_(table, hyper, ntensors: int, nchunks: int, state, beta1: float, beta2: float, eps: float):
    """Launch 3: the fp32 AdamW update of every tensor in the table, in place (nothing when the state block reports an overflow)."""
    _tower_tables("tower_adamw_", table, ntensors, nchunks, state=state, hyper=hyper)
    check(_lib.load().pclip_tower_adamw(ptr(table), ptr(hyper), ntensors, nchunks, ptr(state), beta1, beta2, eps, stream()), "pclip_tower_adamw")


def l2norm_rows_f32(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """F.normalize(x, dim=-1) on fp32 rows."""
    require_cuda(x)
    R, D = x.shape
    y = torch.empty_like(x)
    check(_lib.load().pclip_l2norm_rows_f32(ptr(x), ptr(y), R, D, eps, stream()), "pclip_l2norm_rows_f32")
    return y


def l2norm_rows_backward_f32_(gx: torch.Tensor, x: torch.Tensor, gy: torch.Tensor, eps: float = 1e-12, accumulate: bool = True):
    """gx (+)= backward of F.normalize(x) for upstream gy (all fp32 [R, D])."""
    require_cuda(gx, x, gy)
    R, D = x.shape
    check(_lib.load().pclip_l2norm_rows_backward_f32(ptr(x), ptr(gy), ptr(gx), R, D, eps, int(accumulate), stream()),
          "pclip_l2norm_rows_backward_f32")
    return gx


def adapter_conv_backward(x, g, three_x: bool, conv1, ln1w, ln1b, conv2, ln2w, ln2b, conv3, ln3w, ln3b, chunk: int = 512):
    """Parameter gradients (fp32, shaped like the parameters) of the conv adapter for upstream g = dL/d(output); rows are
    processed `chunk` at a time (per-row contributions live in scratch, then a deterministic column sum).  The width is
    conv1's channel count."""
    require_cuda(x, g)
    x, g = _f16c(x), _f16c(g)
    B, D = x.shape
    W = _adapter_width(conv1)
    s = int(math.ceil(math.sqrt(D)))
    s2, n1, n2 = s * s, W * s * s, W * W * 9
    dev = x.device
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
    out = {"conv1.weight": f32(W), "conv3.weight": f32(W), "bn1.weight": f32(n1), "bn1.bias": f32(n1), "bn3.weight": f32(s2),
           "bn3.bias": f32(s2)}
    if three_x:
        out.update({"conv2.weight": f32(n2), "bn2.weight": f32(n1), "bn2.bias": f32(n1)})
    lib = _lib.load()
    # rows of partial sums a launch over nb rows writes: the persistent MFMA kernel (width 16, conv-3x, D <= 576) one per workgroup — then the whole
    # batch is ONE launch + one column sum per parameter; the per-row kernels one per input row — then the batch is walked in chunks of `chunk` rows
    # (fewer at the wider stacks: a row's contributions are up to 0.5 MB)
    rows_of = lambda nb: lib.pclip_adapter_conv_w_backward_partials(nb, D, int(three_x), W)
    persistent = B > 0 and rows_of(B) < B
    c = max(B, 1) if persistent else min(max(chunk * 16 // W, 1), max(B, 1))
    rmax = max(rows_of(c), 1)
    sc = lambda n: torch.empty(rmax, n, dtype=torch.float32, device=dev)
    pw1, pw3, pg1, pb1, pg3, pb3 = sc(W), sc(W), sc(n1), sc(n1), sc(s2), sc(s2)
    pw2, pg2, pb2 = (sc(n2), sc(n1), sc(n1)) if three_x else (None, None, None)
    for lo in range(0, B, c):
        nb = min(c, B - lo)
        check(lib.pclip_adapter_conv_w_backward_f16(
            ptr(x[lo:lo + nb]), ptr(g[lo:lo + nb]), nb, D, int(three_x), W, ptr(conv1), ptr(ln1w), ptr(ln1b),
            ptr(conv2) if three_x else None, ptr(ln2w) if three_x else None, ptr(ln2b) if three_x else None, ptr(conv3), ptr(ln3w),
            ptr(pw1), ptr(pw2), ptr(pw3), ptr(pg1), ptr(pb1), ptr(pg2), ptr(pb2), ptr(pg3), ptr(pb3), stream()),
            "pclip_adapter_conv_w_backward_f16")
        for name, part in (("conv1.weight", pw1), ("conv3.weight", pw3), ("bn1.weight", pg1), ("bn1.bias", pb1), ("bn3.weight", pg3),
                           ("bn3.bias", pb3), ("conv2.weight", pw2), ("bn2.weight", pg2), ("bn2.bias", pb2)):
            if part is not None:
                colsum_f32(part, rows=rows_of(nb), out=out[name])
    shapes = {"conv1.weight": (W, 1, 1, 1), "conv3.weight": (1, W, 1, 1), "conv2.weight": (W, W, 3, 3), "bn1.weight": (W, s, s),
              "bn1.bias": (W, s, s), "bn2.weight": (W, s, s), "bn2.bias": (W, s, s), "bn3.weight": (1, s, s), "bn3.bias": (1, s, s)}
    return {k: v.view(shapes[k]) for k, v in out.items()}
