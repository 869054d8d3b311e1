"""Thin ctypes wrappers over the ViT kernels of libmemhip.so (include/memhip.h).

These take torch CUDA tensors only as (pointer, shape) carriers; all arithmetic happens in the
hand-written HIP kernels.  Everything is enqueued on torch's current stream.
"""
import ctypes as C

import torch

from ._lib import check, declare, f32, f64, i32, i64, lib, ptr, stream_ptr, sz, vp
from .vae_model import pack_convt_weight  # noqa: F401  (the host side of convt2d_nhwc's weight layout, next to the encoder's _pack)

EPI_BIAS_BF16, EPI_BIAS_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_F32, EPI_PATCH_EMBED, EPI_BIAS_GELU_DG, EPI_MUL_AUX = range(8)
EPI_RESIDUAL_DROP = 8


class Dropout(C.Structure):
    """== memhip_dropout_t (the mask contract: include/memhip.h)."""
    _fields_ = [("key0", C.c_uint32), ("key1", C.c_uint32), ("site", C.c_uint32), ("thr", C.c_uint32), ("scale", f32),
                ("row0", i32)]


def dropout_params(key0, key1, site, p, row0=0):
    """memhip_dropout_t of element-wise dropout with probability p (0 <= p < 1) at `site` under the key (key0, key1)."""
    assert 0.0 <= p < 1.0, p
    return Dropout(int(key0) & 0xFFFFFFFF, int(key1) & 0xFFFFFFFF, int(site), int(round(p * 65536)), 1.0 / (1.0 - p), int(row0))


def with_row0(d, row0):
    """The same dropout addressed from residual-stream row row0 (a buffer whose row 0 is that row)."""
    return None if d is None else Dropout(d.key0, d.key1, d.site, d.thr, d.scale, int(row0))


class GemmArgs(C.Structure):
    """== memhip_gemm_args_t."""
    _fields_ = [("A", vp), ("B", vp), ("lda", i64), ("ldb", i64),
                ("M", i32), ("N", i32), ("K", i32), ("epilogue", i32),
                ("out0", vp), ("ldo0", i64), ("out1", vp), ("ldo1", i64),
                ("bias", vp), ("vec1", vp), ("resid", vp), ("ldr", i64),
                ("aux", vp), ("ldaux", i64), ("rowmask", vp), ("keep_prob", f32),
                ("colscale", f32), ("colscale_n", i32), ("rows_per_sample", i32), ("accumulate", i32),
                ("colsum", vp), ("sample_map", vp), ("colsum_copies", i32), ("reserved0", i32),
                ("dropout", vp)]


class Branch(C.Structure):
    """== memhip_branch_t: the residual branch whose output gradient a row call produces."""
    _fields_ = [("y", vp), ("ldy", i64), ("gamma", vp), ("rowmask", vp), ("keep_prob", f32), ("rows_per_sample", i32),
                ("dy", vp), ("lddy", i64), ("dgamma", vp), ("dbias", vp), ("out_map", vp), ("dropout", vp)]


class BranchBwdArgs(C.Structure):
    """== memhip_branch_bwd_args_t."""
    _fields_ = [("dx", vp), ("lddx", i64), ("M", i32), ("D", i32), ("branch", Branch)]


class LnBwdBranchArgs(C.Structure):
    """== memhip_ln_bwd_branch_args_t."""
    _fields_ = [("dy", vp), ("lddy", i64), ("x", vp), ("ldx", i64), ("R", i32), ("D", i32), ("gamma", vp), ("mean", vp),
                ("rstd", vp), ("dres", vp), ("lddres", i64), ("dgamma", vp), ("dbeta", vp), ("in_map", vp), ("branch", Branch)]


class AttnBwdArgs(C.Structure):
    """== memhip_attn_bwd_args_t."""
    _fields_ = [("qkv", vp), ("ldqkv", i64), ("dout", vp), ("ldo", i64), ("out", vp), ("ldout", i64), ("lse", vp), ("delta", vp),
                ("table", vp), ("window_h", i32), ("window_w", i32), ("B", i32), ("T", i32), ("D", i32), ("heads", i32),
                ("scale", f32), ("reserved0", i32), ("dqkv", vp), ("lddqkv", i64), ("dtable", vp), ("dq_bias", vp),
                ("dv_bias", vp), ("ws", vp), ("ws_bytes", i64)]


class NtLaunch(C.Structure):
    """== memhip_nt_launch_t."""
    _fields_ = [(n, i32) for n in ("kind", "row0", "rows", "tail_rows", "guard", "copy", "grid", "tail_grid")]


class NtPlan(C.Structure):
    """== memhip_nt_plan_t."""
    _fields_ = [("count", i32), ("l", NtLaunch * 2)]


declare({"memhip_gemm_bf16_nt": (i32, [C.POINTER(GemmArgs), vp]),
         "memhip_branch_bwd": (i32, [C.POINTER(BranchBwdArgs), vp]),
         "memhip_layernorm_bwd_branch": (i32, [C.POINTER(LnBwdBranchArgs), vp]),
         "memhip_attn_bwd": (i32, [C.POINTER(AttnBwdArgs), vp]),
         "memhip_gemm_bf16_nt_plan": (i32, [C.POINTER(GemmArgs), i32, i32, C.POINTER(NtPlan)])})


def _p(t):
    return None if t is None else t.data_ptr()


# Optional live timing of every GEMM launch with HIP events on the launch stream (bench.py's
# roofline leg): set GEMM_TIMER to a list; entries are (start_event, end_event, flops, epilogue).
GEMM_TIMER = None
# Events for the timer, created AND recorded once before the timed region (bench.py): creating / first-recording a few
# hundred timing events inside the region grows the runtime's signal pool there, seen as ~14 ms stalls some steps later.
GEMM_EVENT_POOL = []


def _timer_event():
    return GEMM_EVENT_POOL.pop() if GEMM_EVENT_POOL else torch.cuda.Event(enable_timing=True)


def _timed(code, flops, fn):
    """Run fn() between two HIP events on the launch stream when the per-launch timer is armed (bench.py)."""
    if GEMM_TIMER is None:
        fn()
        return
    e0, e1 = _timer_event(), _timer_event()
    e0.record()
    fn()
    e1.record()
    GEMM_TIMER.append((e0, e1, flops, code))


def gemm_args(A, B, M, N, K, epi, out0=None, out1=None, bias=None, vec1=None, resid=None, aux=None,
              rowmask=None, keep_prob=1.0, colscale=1.0, colscale_n=0, rows_per_sample=1, accumulate=False, colsum=None,
              lda=None, ldb=None, ldo0=None, ldo1=None, ldr=None, ldaux=None, sample_map=None, colsum_copies=0, dropout=None):
    """The memhip_gemm_args_t of gemm_nt (same parameters)."""
    a = GemmArgs()
    a.A, a.B = _p(A), _p(B)
    a.lda = A.stride(0) if lda is None else lda
    a.ldb = B.stride(0) if ldb is None else ldb
    a.M, a.N, a.K, a.epilogue = M, N, K, epi
    a.out0 = _p(out0)
    a.ldo0 = (out0.stride(0) if out0 is not None else 0) if ldo0 is None else ldo0
    a.out1 = _p(out1)
    a.ldo1 = (out1.stride(0) if out1 is not None else 0) if ldo1 is None else ldo1
    a.bias, a.vec1, a.resid = _p(bias), _p(vec1), _p(resid)
    a.ldr = (resid.stride(0) if resid is not None else 0) if ldr is None else ldr
    a.aux = _p(aux)
    a.ldaux = (aux.stride(0) if (aux is not None and aux.dim() > 1) else 0) if ldaux is None else ldaux
    a.rowmask = _p(rowmask)
    a.keep_prob, a.colscale, a.colscale_n = keep_prob, colscale, colscale_n
    a.rows_per_sample, a.accumulate = rows_per_sample, int(accumulate)
    a.colsum = _p(colsum)
    a.sample_map = _p(sample_map)
    a.colsum_copies = colsum_copies
    a.dropout = None if dropout is None else C.addressof(dropout)
    return a


def gemm_nt(A, B, M, N, K, epi, *args, **kw):
    """C[M,N] = A[M,K] @ B[N,K]^T with a fused epilogue (keywords: gemm_args).  A/B bf16, row-major, K contiguous.
    colsum_copies > 1: `colsum` is a zeroed [copies, N] workspace, folded into the bias gradient by colsum_fold.
    dropout: a Dropout (epilogue EPI_RESIDUAL_DROP only)."""
    a = gemm_args(A, B, M, N, K, epi, *args, **kw)
    _timed(epi, 2.0 * M * N * K, lambda: check(lib.memhip_gemm_bf16_nt(C.byref(a), stream_ptr()), "gemm_bf16_nt"))


NT_128, NT_G256, NT_P8_256, NT_P8_128, NT_P8_PAIR = range(5)


def gemm_nt_plan(a, stream_cus=None, device_cus=None):
    """The launches memhip_gemm_bf16_nt makes for the GemmArgs `a` under the current options, as a list of NtLaunch (kind
    NT_*, rows [row0, row0 + rows), tail_rows, guard, copy, grid, tail_grid).  Nothing is launched; no device is needed
    when both CU counts are given (default: the current device's, no reservation)."""
    if stream_cus is None or device_cus is None:
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        stream_cus = cus if stream_cus is None else stream_cus
        device_cus = cus if device_cus is None else device_cus
    plan = NtPlan()
    check(lib.memhip_gemm_bf16_nt_plan(C.byref(a), stream_cus, device_cus, C.byref(plan)), "gemm_bf16_nt_plan")
    return [plan.l[i] for i in range(plan.count)]


declare({
    "memhip_layernorm_fwd": (i32, [vp, i64, vp, i32, i32, vp, vp, f32, vp, i64, vp, vp, vp]),
    "memhip_layernorm_bwd": (i32, [vp, i64, vp, i64, vp, i32, i32, vp, vp, vp, vp, i64, i32, vp, vp, vp]),
    "memhip_layerscale_grad": (i32, [vp, i64, vp, i64, vp, vp, vp, i32, i32, vp, vp]),
    "memhip_embed_bwd": (i32, [vp, i64, vp, i32, i32, i32, vp, i64, vp, vp, vp]),
    "memhip_cross_entropy": (i32, [vp, i64, vp, i32, i32, f32, vp, vp, i32, vp, vp]),
    "memhip_attn_tokens_padded": (i32, [i32]),
    "memhip_relpos_gather": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
    "memhip_attn_fwd": (i32, [vp, i64, i32, i32, i32, i32, vp, i32, i32, vp, i64, vp, vp]),
    "memhip_attn_delta": (i32, [vp, vp, i64, i64, i32, vp, vp]),
    "memhip_attn_bwd_workspace": (i64, [i32, i32, i32, i32, i32]),
    "memhip_cast_f32_bf16": (i32, [vp, vp, i64, vp]),
    "memhip_copy_samples_f32": (i32, [vp, vp, vp, i32, i64, vp]),
    "memhip_zero": (i32, [vp, i64, vp]),
    "memhip_stream_reserve_cus": (i32, [vp, i32]),
    "memhip_zero_ranges": (i32, [vp, vp, i32, i64, vp]),
    "memhip_transpose_cast_f32_bf16": (i32, [vp, i64, i32, i32, vp, i64, vp]),
    "memhip_transpose_bf16": (i32, [vp, i64, i32, i32, vp, i64, i32, vp, i32, i32, vp, i32, i32, vp]),
    "memhip_im2col_bf16": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    "memhip_fill_cls": (i32, [vp, i64, i32, i32, i32, vp, vp]),
    "memhip_gemv_bf16_acc": (i32, [vp, i64, i32, i32, vp, vp, vp, vp, vp]),
    "memhip_nchw_to_padded_nhwc4": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, i64, i32, vp]),
    "memhip_argmax_rows": (i32, [vp, i32, i64, i32, i32, vp, vp, vp, vp, i32, vp]),
    "memhip_tok_flag_samples": (i32, [vp, vp, i32, i32, f32, vp, vp, vp, vp]),
    "memhip_tok_gather_images_f32": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp]),
    "memhip_tok_scatter_ids": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    "memhip_grad_norm_workspace": (sz, []),
    "memhip_grad_norm": (i32, [vp, i64, vp, vp, sz, vp]),
    "memhip_adamw": (i32, [vp, vp, vp, vp, i64, vp, f64, f64, f64, f64, f64, i32, vp, f64, vp]),
    "memhip_transpose_cast_batched": (i32, [vp, vp, i32, i32, vp]),
    "memhip_adamw_groups": (i32, [vp, vp, vp, vp, i64, vp, vp, i32, f64, f64, f64, i32, vp, f64, vp]),
    "memhip_dropout_mask": (i32, [C.POINTER(Dropout), i32, i32, i32, vp, vp]),
    "memhip_dropout_rows_f32": (i32, [C.POINTER(Dropout), vp, i64, i32, i32, vp]),
})


def dropout_mask(d, row0, rows, cols, out):
    """out u8 [rows, cols] = keep bits of residual-stream rows d.row0 + row0 .. (memhip_dropout_mask)."""
    check(lib.memhip_dropout_mask(C.byref(d), row0, rows, cols, ptr(out), stream_ptr()), "dropout_mask")


def dropout_rows(d, x, rows, D):
    """x f32 [rows, D] *= keep * scale in place (pos_drop; and its backward on the gradient)."""
    check(lib.memhip_dropout_rows_f32(C.byref(d), ptr(x), x.stride(0), rows, D, stream_ptr()), "dropout_rows_f32")


def layernorm_fwd(x, gamma, beta, y, mean, rstd, R, D, eps=1e-6, row_idx=None):
    check(lib.memhip_layernorm_fwd(ptr(x), x.stride(0), ptr(row_idx), R, D, ptr(gamma), ptr(beta), eps,
                                   ptr(y), y.stride(0), ptr(mean), ptr(rstd), stream_ptr()), "layernorm_fwd")


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, R, D, accumulate=True, row_idx=None):
    check(lib.memhip_layernorm_bwd(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(row_idx), R, D, ptr(gamma),
                                   ptr(mean), ptr(rstd), ptr(dres), dres.stride(0), int(accumulate),
                                   ptr(dgamma), ptr(dbeta), stream_ptr()), "layernorm_bwd")


def _branch(y, gamma, rowmask, keep_prob, rows_per_sample, dy, dgamma, dbias, out_map, dropout):
    """The Branch of the two row wrappers.  `dropout` (a Dropout) is referenced, not copied: the library reads it on the host
    inside the call, and the wrapper's frame holds it until then."""
    return Branch(_p(y), y.stride(0) if y is not None else 0, _p(gamma), _p(rowmask), keep_prob, rows_per_sample, _p(dy),
                  dy.stride(0), _p(dgamma), _p(dbias), _p(out_map), None if dropout is None else C.addressof(dropout))


def layernorm_bwd_branch(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, R, D, y_b, gamma_b, dy_b, dgamma_b, dbias_b,
                         rowmask=None, keep_prob=1.0, rows_per_sample=1, in_map=None, out_map=None, dropout=None):
    """layernorm_bwd(accumulate=True) + the branch_bwd that reads the updated dres, in one pass.  in_map / out_map (i32
    [samples], -1 = dropped): work-skipping stochastic depth, dy / mean / rstd and dy_b then hold kept samples only.
    dropout: the Dropout of the branch whose gradient dy_b is."""
    a = LnBwdBranchArgs(_p(dy), dy.stride(0), _p(x), x.stride(0), R, D, _p(gamma), _p(mean), _p(rstd), _p(dres), dres.stride(0),
                        _p(dgamma), _p(dbeta), _p(in_map),
                        _branch(y_b, gamma_b, rowmask, keep_prob, rows_per_sample, dy_b, dgamma_b, dbias_b, out_map, dropout))
    check(lib.memhip_layernorm_bwd_branch(C.byref(a), stream_ptr()), "layernorm_bwd_branch")


def layerscale_grad(W16, dW, bias, dbias, gamma, N, K, dgamma):
    """dgamma[N] = (rowdot(W16, dW) + bias * dbias) / gamma  (overwrites dgamma)."""
    check(lib.memhip_layerscale_grad(ptr(W16), W16.stride(0), ptr(dW), dW.stride(0), ptr(bias), ptr(dbias), ptr(gamma),
                                     N, K, ptr(dgamma), stream_ptr()), "layerscale_grad")


def branch_bwd(dx, y, gamma, dy, dgamma, dbias, M, D, rowmask=None, keep_prob=1.0, rows_per_sample=1, out_map=None, dropout=None):
    a = BranchBwdArgs(_p(dx), dx.stride(0), M, D,
                      _branch(y, gamma, rowmask, keep_prob, rows_per_sample, dy, dgamma, dbias, out_map, dropout))
    check(lib.memhip_branch_bwd(C.byref(a), stream_ptr()), "branch_bwd")


def gemv_acc(W, N, K, x, y, x_acc=None, zero=None):
    """y[N] += W[N,K] (bf16) @ x[K]; optionally x_acc += x and zero[:] = 0."""
    check(lib.memhip_gemv_bf16_acc(ptr(W), W.stride(0), N, K, ptr(x), ptr(y), ptr(x_acc), ptr(zero), stream_ptr()),
          "gemv_bf16_acc")


CONV_MODES = ("bf16", "fp32", "fp16x2")                  # MEMHIP_CONV_*; the precisions of HipTokenizer
_CONV_MODE = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 2}     # index of CONV_MODES by the dtype of the activations
_F16X2 = 2


class ConvArgs(C.Structure):
    """== memhip_conv_args_t."""
    _fields_ = [("mode", i32), ("reserved0", i32), ("in", vp), ("in_plane", i64), ("weight", vp), ("w_plane", i64),
                ("bias", vp), ("add", vp), ("add_plane", i64), ("out", vp), ("out_plane", i64)] + \
               [(n, i32) for n in ("B", "H", "W", "Cin", "Cout", "ksize", "stride", "pad", "relu", "out_padded", "out_f32",
                                   "reserved1")] + [("n_active", vp)]


declare({"memhip_conv2d_nhwc": (i32, [C.POINTER(ConvArgs), vp])})


def conv_args(mode, B, H, W, Cin, Cout, ksize, stride, pad, x=None, weight=None, bias=None, out=None, relu=False, add=None,
              out_padded=True, out_f32=False, n_active=None, planes=(0, 0, 0, 0)):
    """The memhip_conv_args_t of conv2d_nhwc / conv_plan: mode is an index of CONV_MODES, the tensors are addresses or None,
    planes = (in, weight, add, out) plane strides (fp16x2)."""
    return ConvArgs(mode, 0, x, planes[0], weight, planes[1], bias, add, planes[2], out, planes[3], B, H, W, Cin, Cout, ksize,
                    stride, pad, int(relu), int(out_padded), int(out_f32), 0, n_active)


def conv2d_nhwc(x_pad, weight, bias, out, B, H, W, Cin, Cout, ksize, stride, pad, relu=False, add=None, out_padded=True,
                n_active=None):
    """x_pad [B,H+2,W+2,Cin] -> out [B,Ho+2,Wo+2,Cout] interior (or dense [B*Ho*Wo,Cout]); bf16, fp32 or fp16x2 by x_pad.dtype.
    fp16x2: x_pad, weight, add, out are fp16 [2 (hi / lo plane), ...], or out is the dense fp32 logit matrix.
    n_active (fp32 only): device int32 [1], the number of live samples of the capacity B."""
    mode = _CONV_MODE[x_pad.dtype]
    out_f32 = mode == _F16X2 and out.dtype == torch.float32
    assert weight.dtype == x_pad.dtype and (out_f32 or out.dtype == x_pad.dtype) and (add is None or add.dtype == x_pad.dtype)
    planes = (0, 0, 0, 0) if mode != _F16X2 else (x_pad.stride(0), weight.stride(0), 0 if add is None else add.stride(0),
                                             0 if out_f32 else out.stride(0))
    a = conv_args(mode, B, H, W, Cin, Cout, ksize, stride, pad, _p(x_pad), _p(weight), _p(bias), _p(out), relu, _p(add),
                  out_padded and not out_f32, out_f32, _p(n_active), planes)
    check(lib.memhip_conv2d_nhwc(C.byref(a), stream_ptr()), "conv2d_nhwc")


def nchw_to_padded_nhwc4(x, out, mean=None, std=None):
    """x f32 [B, C<=4, H, W] -> the interior of out [B, H+2, W+2, 4] (fp16: [2, B, ...]), the mode by out.dtype."""
    B, Cc, H, W = x.shape
    mode = _CONV_MODE[out.dtype]
    check(lib.memhip_nchw_to_padded_nhwc4(ptr(x), B, Cc, H, W, ptr(mean), ptr(std), ptr(out), out.stride(0) if mode == _F16X2 else 0,
                                          mode, stream_ptr()), "nchw_to_padded_nhwc4")


def argmax_rows(logits, M, N, ids, gap=None, rms=None, n_samples=None, rows_per_sample=0):
    check(lib.memhip_argmax_rows(ptr(logits), _CONV_MODE[logits.dtype], logits.stride(0), M, N, ptr(ids), ptr(gap), ptr(rms),
                                 ptr(n_samples), rows_per_sample, stream_ptr()), "argmax_rows")


declare({
    "memhip_convt2d_nhwc": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "memhip_kl_uniform_rows": (i32, [vp, i32, i64, i32, i32, vp, vp]),
})


def convt2d_nhwc(x_pad, weight, bias, out, B, H, W, Cin, Cout, relu=False):
    """ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1) (+ bias, optional ReLU; vae_model.py:92) on the tokenizer's format:
    x_pad bf16 [B, H+2, W+2, Cin] with a zero border -> the interior of out bf16 [B, 2H+2, 2W+2, Cout] (its border ring is
    not written).  weight = pack_convt_weight(w) in bf16, bias f32 [Cout] or None.  Cin % 64 == 0, Cout % 8 == 0."""
    assert x_pad.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
    assert B == 0 or (x_pad.numel() >= B * (H + 2) * (W + 2) * Cin and weight.numel() == 16 * Cin * Cout and
                      out.numel() >= B * (2 * H + 2) * (2 * W + 2) * Cout and (bias is None or bias.numel() == Cout))
    check(lib.memhip_convt2d_nhwc(_p(x_pad), _p(weight), _p(bias), _p(out), B, H, W, Cin, Cout, int(relu), stream_ptr()),
          "convt2d_nhwc")


def kl_uniform_rows(logits, M, N, out=None):
    """f32 [M]: KL(softmax(logits[m]) || uniform) = sum_n q log q + log N of the first M rows of logits (bf16 or fp32,
    [rows, ld]) in one pass per row -- F.kl_div(log_uniform, F.log_softmax(logits, -1), reduction='none',
    log_target=True).sum(-1) (vae_model.py:203-206) without the [M, N] log_softmax matrix."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] >= M and logits.shape[1] >= N
    if out is None:
        out = torch.empty((M,), dtype=torch.float32, device=logits.device)
    assert out.dtype == torch.float32 and out.numel() >= M
    check(lib.memhip_kl_uniform_rows(ptr(logits), _CONV_MODE[logits.dtype], logits.stride(0), M, N, ptr(out), stream_ptr()),
          "kl_uniform_rows")
    return out[:M]


def tok_flag_samples(gap, rms, B, hw, kappa, lst, count, stats=None):
    check(lib.memhip_tok_flag_samples(ptr(gap), ptr(rms), B, hw, float(kappa), ptr(lst), ptr(count), ptr(stats), stream_ptr()),
          "tok_flag_samples")


def tok_gather_images(x, mean, std, lst, count, offset, R, out, n_round):
    _, Cc, H, W = x.shape
    check(lib.memhip_tok_gather_images_f32(ptr(x), Cc, H, W, ptr(mean), ptr(std), ptr(lst), ptr(count), offset, R, ptr(out),
                                           ptr(n_round), stream_ptr()), "tok_gather_images_f32")


def tok_scatter_ids(ids_in, lst, n_round, offset, R, hw, ids_out):
    check(lib.memhip_tok_scatter_ids(ptr(ids_in), ptr(lst), ptr(n_round), offset, R, hw, ptr(ids_out), stream_ptr()),
          "tok_scatter_ids")


def embed_bwd(dx, mask_u8, B, L, D, dy, dcls, dmask_token):
    check(lib.memhip_embed_bwd(ptr(dx), dx.stride(0), ptr(mask_u8), B, L, D, ptr(dy), dy.stride(0), ptr(dcls),
                               ptr(dmask_token), stream_ptr()), "embed_bwd")


def cross_entropy(logits, labels, M, V, grad_scale, row_loss, row_correct, out2, write_grad=True):
    check(lib.memhip_cross_entropy(ptr(logits), logits.stride(0), ptr(labels), M, V, grad_scale, ptr(row_loss),
                                   ptr(row_correct), int(write_grad), ptr(out2), stream_ptr()), "cross_entropy")


def attn_tokens_padded(T):
    return lib.memhip_attn_tokens_padded(T)


def relpos_gather(table, index_i32, T, TP, heads, bias_pad, biasT_pad=None):
    check(lib.memhip_relpos_gather(ptr(table), ptr(index_i32), T, TP, heads, ptr(bias_pad), ptr(biasT_pad),
                                   stream_ptr()), "relpos_gather")


def attn_fwd(qkv, B, T, D, heads, table, window, out, lse):
    _timed(200, 4.0 * B * T * T * D, lambda: check(
        lib.memhip_attn_fwd(ptr(qkv), qkv.stride(0), B, T, D, heads, ptr(table), window[0], window[1], ptr(out),
                            out.stride(0), ptr(lse), stream_ptr()), "attn_fwd"))


def attn_delta(dout, out, rows, heads, delta):
    check(lib.memhip_attn_delta(ptr(dout), ptr(out), out.stride(0), rows, heads, ptr(delta), stream_ptr()),
          "attn_delta")


def attn_bwd_workspace(B, T, heads, window):
    """Bytes of scratch the dS-storing backward of the long-window kernels wants for this shape (0: no such form)."""
    return int(lib.memhip_attn_bwd_workspace(B, T, heads, window[0], window[1]))


ATTN_16, ATTN_SMALL, ATTN_WIN, ATTN_WIN_DS, ATTN_STREAM = range(1, 6)
# kernel names of AttnLaunch.kernel (MEMHIP_ATTN_K_*), as they appear in a kernel trace
ATTN_KERNELS = ("attn_stats_zero_kernel", "attn_delta_kernel", "attn_fwd_kernel", "attn_bwd_kv_kernel", "attn_bwd_q_kernel",
                "attn16_fwd_kernel", "attn16_bwd_kernel", "attn_win_stats_kernel", "attn_fwd_win_kernel", "attn_bwd_kv_win_kernel",
                "attn_bwd_q_win_kernel", "attn_bwd_kvs_win_kernel", "attn_bwd_qs_win_kernel", "attn_fwd_stream_kernel",
                "attn_bwd_kv_stream_kernel", "attn_bwd_q_stream_kernel")


class AttnLaunch(C.Structure):
    """== memhip_attn_launch_t."""
    _fields_ = [(n, i32) for n in ("kernel", "grid_x", "grid_y", "grid_z", "block", "lds")]


class AttnPlan(C.Structure):
    """== memhip_attn_plan_t."""
    _fields_ = [(n, i32) for n in ("family", "n", "ww", "vb", "dt", "fd", "spb", "nwg", "groups", "nbz", "nbq", "nbs", "qgroups",
                                   "qs", "stream_spb", "lds_over", "count")] + [("l", AttnLaunch * 5)]

    @property
    def launches(self):
        """[(kernel name, (grid x, y, z), workgroup size, dynamic LDS bytes)], in launch order."""
        return [(ATTN_KERNELS[l.kernel], (l.grid_x, l.grid_y, l.grid_z), l.block, l.lds) for l in self.l[:self.count]]


declare({"memhip_attn_plan_fwd": (i32, [i32, i32, i32, i32, i32, i32, i32, C.POINTER(AttnPlan)]),
         "memhip_attn_plan_bwd": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i64, i32, C.POINTER(AttnPlan)])})


def attn_plan(B, T, heads, window, backward=False, dtable=True, dv_bias=False, out=False, ws=None, ws_bytes=0, stream_cus=None):
    """The AttnPlan of attn_fwd (backward=False) or attn_bwd for this shape under the current options: family ATTN_*, template
    choices, samples-per-workgroup numbers and `.launches`.  dtable / dv_bias / out: the call gives them; ws: a tensor, or an
    address with ws_bytes.  Nothing is launched; no device is needed when stream_cus is given (default: the current
    device's CU count, no reservation)."""
    if stream_cus is None:
        stream_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    plan = AttnPlan()
    if not backward:
        check(lib.memhip_attn_plan_fwd(B, T, 64 * heads, heads, window[0], window[1], stream_cus, C.byref(plan)), "attn_plan_fwd")
        return plan
    if ws is not None and not isinstance(ws, int):
        ws, ws_bytes = ptr(ws), ws.numel() * ws.element_size()
    check(lib.memhip_attn_plan_bwd(B, T, 64 * heads, heads, window[0], window[1], int(dtable), int(dv_bias), int(out), ws, ws_bytes,
                                   stream_cus, C.byref(plan)), "attn_plan_bwd")
    return plan


def attn_bwd(qkv, dout, lse, delta, table, window, B, T, D, heads, scale, dqkv, dtable, dq_bias=None, dv_bias=None, out=None, ws=None):
    """out = the forward output: rowsum(dout * out) is computed by the library (inside the fused 14 x 14 kernel when it
    applies); without it `delta` must have been filled by attn_delta.  ws = a uint8 scratch tensor of at least
    attn_bwd_workspace(...) bytes: the long-window backward then stores dS instead of computing it twice."""
    a = AttnBwdArgs(_p(qkv), qkv.stride(0), _p(dout), dout.stride(0), _p(out), out.stride(0) if out is not None else 0, _p(lse),
                    _p(delta), _p(table), window[0], window[1], B, T, D, heads, scale, 0, _p(dqkv), dqkv.stride(0), _p(dtable),
                    _p(dq_bias), _p(dv_bias), _p(ws), ws.numel() * ws.element_size() if ws is not None else 0)
    _timed(201, 10.0 * B * T * T * D, lambda: check(lib.memhip_attn_bwd(C.byref(a), stream_ptr()), "attn_bwd"))


def residual_rows(x, rows_i32, y, gamma, rowkeep, keep_prob, R, D, out):
    """out[i] = x[rows[i]] + drop_path(gamma * y[i]) (the RESIDUAL epilogue's arithmetic on compact rows)."""
    check(lib.memhip_residual_rows(ptr(x), x.stride(0), ptr(rows_i32), ptr(y), y.stride(0), ptr(gamma), ptr(rowkeep), keep_prob,
                                   R, D, ptr(out), out.stride(0), stream_ptr()), "residual_rows")


def scatter_rows(src, rows_i32, R, D, dst):
    check(lib.memhip_scatter_rows_f32(ptr(src), src.stride(0), ptr(rows_i32), R, D, ptr(dst), dst.stride(0), stream_ptr()),
          "scatter_rows")


def copy_samples(src, dst, ids_i32, n, n_per_sample):
    check(lib.memhip_copy_samples_f32(ptr(src), ptr(dst), ptr(ids_i32), n, n_per_sample, stream_ptr()), "copy_samples")


def stream_reserve_cus(stream, cus):
    """Launches on `stream` (a torch.cuda.Stream) size their persistent grids for `cus` CUs fewer (0 clears it)."""
    check(lib.memhip_stream_reserve_cus(C.c_void_p(stream.cuda_stream), int(cus)), "stream_reserve_cus")


def zero_(t):
    """t.zero_() by the library's fill kernel (t contiguous, 16-byte aligned, a multiple of 16 bytes)."""
    nb = t.numel() * t.element_size()
    assert t.is_contiguous() and nb % 16 == 0
    check(lib.memhip_zero(ptr(t), nb, stream_ptr()), "zero")


def zero_ranges(base, ranges_dev, n, total_bytes):
    check(lib.memhip_zero_ranges(ptr(base), ptr(ranges_dev), n, total_bytes, stream_ptr()), "zero_ranges")


def cast_f32_bf16(src, dst, n):
    check(lib.memhip_cast_f32_bf16(ptr(src), ptr(dst), n, stream_ptr()), "cast")


def transpose_cast(src_f32, R, Cc, dst_bf16, ldout=None):
    check(lib.memhip_transpose_cast_f32_bf16(ptr(src_f32), src_f32.stride(0), R, Cc, ptr(dst_bf16),
                                             dst_bf16.stride(0) if ldout is None else ldout, stream_ptr()),
          "transpose_cast")


def transpose_cast_batched(desc_dev, prefix_dev, n, total_tiles):
    check(lib.memhip_transpose_cast_batched(ptr(desc_dev), ptr(prefix_dev), n, total_tiles, stream_ptr()),
          "transpose_cast_batched")


def transpose_bf16(src, R, Cc, dst, R_pad, colsum0=None, c0=(0, 0), colsum1=None, c1=(0, 0)):
    check(lib.memhip_transpose_bf16(ptr(src), src.stride(0), R, Cc, ptr(dst), dst.stride(0), R_pad, ptr(colsum0),
                                    c0[0], c0[1], ptr(colsum1), c1[0], c1[1], stream_ptr()), "transpose_bf16")


def im2col(x, B, Cc, H, W, ph, pw, out):
    check(lib.memhip_im2col_bf16(ptr(x), B, Cc, H, W, ph, pw, ptr(out), stream_ptr()), "im2col")


def fill_cls(x, B, T, D, cls):
    check(lib.memhip_fill_cls(ptr(x), x.stride(0), B, T, D, ptr(cls), stream_ptr()), "fill_cls")


def grad_norm(g, n, norm_out, ws):
    check(lib.memhip_grad_norm(ptr(g), n, ptr(norm_out), ptr(ws), ws.numel() * ws.element_size(), stream_ptr()),
          "grad_norm")


def adamw(p, g, m, v, n, wd_flags, lr, beta1, beta2, eps, wd, step, gnorm=None, max_norm=0.0):
    check(lib.memhip_adamw(ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(wd_flags), lr, beta1, beta2, eps, wd, step,
                           ptr(gnorm), max_norm if max_norm else 0.0, stream_ptr()), "adamw")


def adamw_groups(p, g, m, v, n, group_of_chunk, group_table, n_groups, beta1, beta2, eps, step, gnorm=None, max_norm=0.0):
    check(lib.memhip_adamw_groups(ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(group_of_chunk), ptr(group_table), n_groups, beta1,
                                  beta2, eps, step, ptr(gnorm), max_norm if max_norm else 0.0, stream_ptr()), "adamw_groups")


declare({
    "memhip_gemm_bf16_tn": (i32, [vp, i64, vp, i64, i32, i32, i32, vp, i64, i32, vp, sz, vp]),
    "memhip_gemm_bf16_tn_workspace": (sz, [i32, i32, i32]),
    "memhip_gemm_bf16_tn_group_workspace": (sz, [vp, i32]),
    "memhip_gemm_bf16_tn_group": (i32, [vp, i32, i32, vp, sz, vp]),
    "memhip_colsum_bf16": (i32, [vp, i64, i32, i32, vp, vp]),
    "memhip_colsum_fold": (i32, [vp, i32, i32, vp, vp]),
    "memhip_residual_rows": (i32, [vp, i64, vp, vp, i64, vp, vp, f32, i32, i32, vp, i64, vp]),
    "memhip_scatter_rows_f32": (i32, [vp, i64, vp, i32, i32, vp, i64, vp]),
})


_TN_WS_CACHE = {}       # (the library plans up to 32 split counts per query, and the engine asks in front of every weight-gradient launch;
                        # the answer depends on the shape only: it is sized for every CU of the device whatever a stream has reserved)


def gemm_tn_workspace(R, N, K):
    key = (R, N, K)
    v = _TN_WS_CACHE.get(key)
    if v is None:
        v = _TN_WS_CACHE[key] = int(lib.memhip_gemm_bf16_tn_workspace(R, N, K))
    return v


def _ws_arg(workspace):
    """(pointer, bytes) of an optional uint8 scratch tensor"""
    return (None, 0) if workspace is None else (ptr(workspace), workspace.numel() * workspace.element_size())


def gemm_tn(A, B, R, N, K, out, accumulate=True, workspace=None):
    """out[N,K] (+)= A[R,N]^T @ B[R,K]  (weight gradient; A = dY, B = X, token-major bf16).  `workspace`:
    optional uint8 scratch tensor of >= gemm_tn_workspace(R,N,K) bytes (plain-store partial tiles)."""
    ws, wsb = _ws_arg(workspace)
    _timed(100, 2.0 * R * N * K, lambda: check(
        lib.memhip_gemm_bf16_tn(ptr(A), A.stride(0), ptr(B), B.stride(0), R, N, K, ptr(out), out.stride(0),
                                int(accumulate), ws, wsb, stream_ptr()), "gemm_bf16_tn"))


class TnProblem(C.Structure):
    """memhip_tn_problem_t (include/memhip.h)"""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("B", C.c_void_p), ("ldb", C.c_int64), ("out", C.c_void_p),
                ("ldo", C.c_int64), ("R", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("reserved0", C.c_int32)]


def _tn_problems(problems):
    arr = (TnProblem * len(problems))()
    for q, (A, B, R, N, K, out) in zip(arr, problems):
        q.A, q.lda, q.B, q.ldb, q.out, q.ldo = A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), out.data_ptr(), out.stride(0)
        q.R, q.N, q.K, q.reserved0 = R, N, K, 0
    return arr


def _tn_shapes(shapes):
    """TnProblem array of the shapes [(R, N, K), ...] with dense leading dimensions and no pointers (workspace queries)"""
    arr = (TnProblem * len(shapes))()
    for q, (R, N, K) in zip(arr, shapes):
        q.R, q.N, q.K, q.lda, q.ldb, q.ldo = R, N, K, N, K, K
    return arr


def gemm_tn_group_workspace(shapes):
    """bytes of scratch for gemm_tn_group over products of the shapes [(R, N, K), ...]"""
    key = tuple(shapes)
    if key in _TN_WS_CACHE:
        return _TN_WS_CACHE[key]
    v = _TN_WS_CACHE[key] = int(lib.memhip_gemm_bf16_tn_group_workspace(_tn_shapes(shapes), len(shapes)))
    return v


def gemm_tn_group(problems, accumulate=True, workspace=None):
    """The weight gradients [(A = dY, B = X, R, N, K, out f32 [N, K]), ...] of up to four layers as ONE launch
    (memhip_gemm_bf16_tn_group); each product has the contract of gemm_tn."""
    ws, wsb = _ws_arg(workspace)
    arr = _tn_problems(problems)
    _timed(100 + len(problems), sum(2.0 * R * N * K for _, _, R, N, K, _ in problems), lambda: check(   # 102..104: a group
        lib.memhip_gemm_bf16_tn_group(arr, len(problems), int(accumulate), ws, wsb, stream_ptr()), "gemm_bf16_tn_group"))


TN_128, TN_P8_ATOMIC, TN_P8_WS, TN_P8_GROUP = range(4)


class TnPart(C.Structure):
    """== memhip_tn_part_t."""
    _fields_ = [(n, i32) for n in ("problem", "tiles", "splits", "rows_per_split", "wg_begin", "quad_begin")] + [("ws_offset", i64)]


class TnLaunch(C.Structure):
    """== memhip_tn_launch_t."""
    _fields_ = [(n, i32) for n in ("kind", "count", "grid", "reduce_grid", "memset_first", "use_atomics")] + \
               [("ws_bytes", i64), ("p", TnPart * 4)]


class TnPlan(C.Structure):
    """== memhip_tn_plan_t."""
    _fields_ = [("count", i32), ("reserved0", i32), ("l", TnLaunch * 4)]


declare({"memhip_gemm_bf16_tn_plan": (i32, [vp, i32, i32, vp, sz, i32, C.POINTER(TnPlan)]),
         "memhip_gemm_bf16_tn_plan_workspace": (sz, [vp, i32, i32])})


def gemm_tn_plan(problems, accumulate=True, workspace=None, stream_cus=None):
    """The launches gemm_tn_group (one problem: gemm_tn) makes under the current options, as a list of TnLaunch (kind TN_*,
    grid, reduce_grid, memset_first, use_atomics, ws_bytes, and per product p[i]: problem, tiles, splits, rows_per_split,
    wg_begin, quad_begin, ws_offset).  problems: as for gemm_tn_group, or a TnProblem array; workspace: a tensor, None or
    (address, bytes).  Nothing is launched; with stream_cus no device is needed (default: the default stream's CUs)."""
    arr = problems if isinstance(problems, C.Array) else _tn_problems(problems)
    ws, wsb = workspace if isinstance(workspace, tuple) else _ws_arg(workspace)
    plan = TnPlan()
    check(lib.memhip_gemm_bf16_tn_plan(arr, len(arr), int(accumulate), ws, wsb, -1 if stream_cus is None else stream_cus,
                                       C.byref(plan)), "gemm_bf16_tn_plan")
    return [plan.l[i] for i in range(plan.count)]


def gemm_tn_plan_workspace(problems, device_cus):
    """gemm_tn_group_workspace as it answers on a device of device_cus CUs, for a TnProblem array (one product with ldo = K:
    gemm_tn_workspace).  No device is needed."""
    return int(lib.memhip_gemm_bf16_tn_plan_workspace(problems, len(problems), device_cus))


def colsum_fold(ws, copies, N, out):
    """out[N] += the `copies` accumulator copies in ws (a GEMM with colsum_copies > 1 filled them); ws is zeroed again."""
    check(lib.memhip_colsum_fold(ptr(ws), copies, N, ptr(out), stream_ptr()), "colsum_fold")


def colsum_bf16(x, R, Cc, out):
    check(lib.memhip_colsum_bf16(ptr(x), x.stride(0), R, Cc, ptr(out), stream_ptr()), "colsum_bf16")


# ---------------------------------------------------------------- fp32 parity mode (csrc/fp32_path.hip)
declare({
    "memhip_f32_gemm_nt": (i32, [C.POINTER(GemmArgs), vp]),
    "memhip_f32_transpose": (i32, [vp, i64, i32, i32, vp, i64, vp]),
    "memhip_f32_layernorm_fwd": (i32, [vp, i64, vp, i32, i32, vp, vp, f32, vp, i64, vp, vp, vp]),
    "memhip_f32_layernorm_bwd": (i32, [vp, i64, vp, i64, vp, i32, i32, vp, vp, vp, vp, i64, i32, vp, vp, vp]),
    "memhip_f32_branch_bwd": (i32, [vp, i64, vp, i64, vp, vp, f32, i32, i32, i32, vp, i64, vp, vp, vp]),
    "memhip_f32_embed_bwd": (i32, [vp, i64, vp, i32, i32, i32, vp, i64, vp, vp, vp]),
    "memhip_f32_cross_entropy": (i32, [vp, i64, vp, i32, i32, f32, vp, vp, i32, vp, vp]),
    "memhip_f32_colsum": (i32, [vp, i64, i32, i32, vp, vp]),
    "memhip_f32_im2col": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    "memhip_f32_attn_fwd": (i32, [vp, i64, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp]),
    "memhip_f32_attn_bwd": (i32, [vp, i64, vp, i64, i32, i32, i32, i32, f32, vp, vp, vp, i64, vp, vp]),
})


def f32_gemm_nt(A, B, M, N, K, epi, out0=None, out1=None, bias=None, vec1=None, resid=None, aux=None, rowmask=None,
                keep_prob=1.0, colscale=1.0, colscale_n=0, rows_per_sample=1, accumulate=False, colsum=None, ldaux=None):
    """fp32 twin of gemm_nt (A, B, out0, out1, DGELU aux are fp32)."""
    a = GemmArgs()
    a.A, a.B, a.lda, a.ldb = _p(A), _p(B), A.stride(0), B.stride(0)
    a.M, a.N, a.K, a.epilogue = M, N, K, epi
    a.out0, a.ldo0 = _p(out0), (out0.stride(0) if out0 is not None else 0)
    a.out1, a.ldo1 = _p(out1), (out1.stride(0) if out1 is not None else 0)
    a.bias, a.vec1, a.resid = _p(bias), _p(vec1), _p(resid)
    a.ldr = resid.stride(0) if resid is not None else 0
    a.aux = _p(aux)
    a.ldaux = (aux.stride(0) if (aux is not None and aux.dim() > 1) else 0) if ldaux is None else ldaux
    a.rowmask = _p(rowmask)
    a.keep_prob, a.colscale, a.colscale_n = keep_prob, colscale, colscale_n
    a.rows_per_sample, a.accumulate = rows_per_sample, int(accumulate)
    a.colsum = _p(colsum)
    check(lib.memhip_f32_gemm_nt(C.byref(a), stream_ptr()), "f32_gemm_nt")


def f32_transpose(src, R, Cc, dst):
    check(lib.memhip_f32_transpose(ptr(src), src.stride(0), R, Cc, ptr(dst), dst.stride(0), stream_ptr()), "f32_transpose")


def f32_layernorm_fwd(x, gamma, beta, y, mean, rstd, R, D, eps=1e-6, row_idx=None):
    check(lib.memhip_f32_layernorm_fwd(ptr(x), x.stride(0), ptr(row_idx), R, D, ptr(gamma), ptr(beta), eps, ptr(y),
                                       y.stride(0), ptr(mean), ptr(rstd), stream_ptr()), "f32_layernorm_fwd")


def f32_layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, R, D, accumulate=True, row_idx=None):
    check(lib.memhip_f32_layernorm_bwd(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(row_idx), R, D, ptr(gamma), ptr(mean),
                                       ptr(rstd), ptr(dres), dres.stride(0), int(accumulate), ptr(dgamma), ptr(dbeta),
                                       stream_ptr()), "f32_layernorm_bwd")


def f32_branch_bwd(dx, y, gamma, dy, dgamma, dbias, M, D, rowmask=None, keep_prob=1.0, rows_per_sample=1):
    check(lib.memhip_f32_branch_bwd(ptr(dx), dx.stride(0), ptr(y), y.stride(0) if y is not None else 0, ptr(gamma), ptr(rowmask),
                                    keep_prob, rows_per_sample, M, D, ptr(dy), dy.stride(0), ptr(dgamma), ptr(dbias),
                                    stream_ptr()), "f32_branch_bwd")


def f32_embed_bwd(dx, mask_u8, B, L, D, dy, dcls, dmask_token):
    check(lib.memhip_f32_embed_bwd(ptr(dx), dx.stride(0), ptr(mask_u8), B, L, D, ptr(dy), dy.stride(0), ptr(dcls),
                                   ptr(dmask_token), stream_ptr()), "f32_embed_bwd")


def f32_cross_entropy(logits, labels, M, V, grad_scale, row_loss, row_correct, out2, write_grad=True):
    check(lib.memhip_f32_cross_entropy(ptr(logits), logits.stride(0), ptr(labels), M, V, grad_scale, ptr(row_loss),
                                       ptr(row_correct), int(write_grad), ptr(out2), stream_ptr()), "f32_cross_entropy")


def f32_colsum(x, R, Cc, out):
    check(lib.memhip_f32_colsum(ptr(x), x.stride(0), R, Cc, ptr(out), stream_ptr()), "f32_colsum")


def f32_im2col(x, B, Cc, H, W, ph, pw, out):
    check(lib.memhip_f32_im2col(ptr(x), B, Cc, H, W, ph, pw, ptr(out), stream_ptr()), "f32_im2col")


def f32_attn_fwd(qkv, B, T, D, heads, table, index, out, lse=None):
    check(lib.memhip_f32_attn_fwd(ptr(qkv), qkv.stride(0), B, T, D, heads, ptr(table), ptr(index), ptr(out), out.stride(0),
                                  ptr(lse), stream_ptr()), "f32_attn_fwd")


def f32_attn_bwd(qkv, dout, B, T, D, heads, scale, table, index, dqkv, dtable):
    check(lib.memhip_f32_attn_bwd(ptr(qkv), qkv.stride(0), ptr(dout), dout.stride(0), B, T, D, heads, scale, ptr(table),
                                  ptr(index), ptr(dqkv), dqkv.stride(0), ptr(dtable), stream_ptr()), "f32_attn_bwd")


# ---------------------------------------------------------------- MAE plumbing (csrc/fp32_path.hip)
declare({
    "memhip_mae_enc_assemble": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "memhip_mae_enc_assemble_bwd": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "memhip_mae_dec_assemble": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "memhip_mae_dec_assemble_bwd": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "memhip_mae_loss": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
})


def mae_enc_assemble(xe, pos, cls, ids_keep, B, L, K, D, out):
    check(lib.memhip_mae_enc_assemble(ptr(xe), ptr(pos), ptr(cls), ptr(ids_keep), B, L, K, D, ptr(out), stream_ptr()), "mae_enc_assemble")


def mae_enc_assemble_bwd(dx, ids_keep, B, L, K, D, dxe, dcls):
    check(lib.memhip_mae_enc_assemble_bwd(ptr(dx), ptr(ids_keep), B, L, K, D, ptr(dxe), ptr(dcls), stream_ptr()), "mae_enc_assemble_bwd")


def mae_dec_assemble(y, mask_token, dpos, ids_restore, B, L, K, D, out):
    check(lib.memhip_mae_dec_assemble(ptr(y), ptr(mask_token), ptr(dpos), ptr(ids_restore), B, L, K, D, ptr(out), stream_ptr()),
          "mae_dec_assemble")


def mae_dec_assemble_bwd(dxd, ids_restore, B, L, K, D, dy, dmask_token):
    check(lib.memhip_mae_dec_assemble_bwd(ptr(dxd), ptr(ids_restore), B, L, K, D, ptr(dy), ptr(dmask_token), stream_ptr()),
          "mae_dec_assemble_bwd")


def mae_loss(pred, img, mask, B, Cc, H, W, patch, only_masked, row_loss, dpred, scratch2):
    check(lib.memhip_mae_loss(ptr(pred), ptr(img), ptr(mask), B, Cc, H, W, patch, int(only_masked), ptr(row_loss), ptr(dpred),
                              ptr(scratch2), stream_ptr()), "mae_loss")


# ---------------------------------------------------------------- the dispatch of the tokenizer convolutions (csrc/conv_plan.cpp)
# kernel names of ConvLaunch.kernel (MEMHIP_CONV_K_*), as they appear in a kernel trace
CONV_KERNELS = ("conv_gemm_kernel", "conv_gemm_f32_kernel", "conv_gemm_f32_m32_kernel", "conv_gemm_f16x2_kernel<4>",
                "conv_gemm_f16x2_kernel<8>", "conv_gemm_f16x2_wide_kernel", "conv_gemm_f16x2_first_kernel", "convt_gemm_kernel")


class ConvLaunch(C.Structure):
    """== memhip_conv_launch_t."""
    _fields_ = [(n, i32) for n in ("kernel", "grid", "block", "lds", "dyn_lo", "dyn_hi")]

    @property
    def name(self):
        return CONV_KERNELS[self.kernel]


class ConvPlan(C.Structure):
    """== memhip_conv_plan_t."""
    _fields_ = [(n, i32) for n in ("Hp", "Wp", "Ho", "Wo", "K", "off")] + [("M", i64), ("count", i32), ("l", ConvLaunch * 2)]

    @property
    def launches(self):
        """[(kernel name, grid, workgroup size, dynamic LDS bytes, dyn_lo, dyn_hi)], in launch order."""
        return [(l.name, l.grid, l.block, l.lds, l.dyn_lo, l.dyn_hi) for l in self.l[:self.count]]


declare({"memhip_conv_plan": (i32, [C.POINTER(ConvArgs), i32, C.POINTER(ConvPlan)])})


def conv_plan(mode, B, H, W, Cin, Cout, ksize, stride, pad, add=False, out_f32=False, out_padded=True, dynamic=False,
              device_cus=None):
    """The ConvPlan of conv2d_nhwc (mode "bf16" / "fp32" / "fp16x2"; dynamic: with n_active) for this layer under the current
    `conv_waves` option: geometry and `.launches`.  The query takes the struct of the call (conv_args; a dummy address stands
    for `add` / `n_active`, nothing is dereferenced) and validates like the call (fp16x2: out_f32 goes with out_padded=False,
    the dense logit matrix).  Nothing is launched; no device is needed when device_cus is given (default: the library asks
    the current device)."""
    a = conv_args(CONV_MODES.index(mode), B, H, W, Cin, Cout, ksize, stride, pad, add=16 if add else None,
                  out_padded=out_padded, out_f32=out_f32, n_active=16 if dynamic else None)
    plan = ConvPlan()
    check(lib.memhip_conv_plan(C.byref(a), -1 if device_cus is None else device_cus, C.byref(plan)), "conv_plan")
    return plan


declare({"memhip_convt_plan": (i32, [i32, i32, i32, i32, i32, i32, C.POINTER(ConvPlan)])})


def convt_plan(B, H, W, Cin, Cout, device_cus=None):
    """The ConvPlan of convt2d_nhwc for this layer: Hp, Wp of the input, Ho = 2H, Wo = 2W, K = 4 Cin, off = 0, M = B H W and one
    launch of convt_gemm_kernel over 4 (phases) x tiles workgroups.  Validates like the call; nothing is launched and no device
    is needed."""
    plan = ConvPlan()
    check(lib.memhip_convt_plan(B, H, W, Cin, Cout, -1 if device_cus is None else device_cus, C.byref(plan)), "convt_plan")
    return plan


# ---------------------------------------------------------------- dVAE training: weight gradients (csrc/conv_wgrad.hip)
class ConvWgradArgs(C.Structure):
    """== memhip_conv_wgrad_args_t."""
    _fields_ = [("small", vp), ("big", vp), ("grad", vp), ("workspace", vp), ("workspace_bytes", sz)] + \
               [(n, i32) for n in ("B", "Hs", "Ws", "C", "N", "ksize", "stride", "pad", "small_padded", "accumulate")]


class ConvWgradPlan(C.Structure):
    """== memhip_conv_wgrad_plan_t."""
    _fields_ = [("M", i64), ("ws_bytes", i64)] + \
               [(n, i32) for n in ("K", "Hbp", "Wbp", "tiles_n", "tiles_k", "splits", "rows_per_split", "grid", "block",
                                   "lds_bytes", "fold_grid", "reserved")]


declare({
    "memhip_conv_wgrad_nhwc": (i32, [C.POINTER(ConvWgradArgs), vp]),
    "memhip_conv_wgrad_plan": (i32, [C.POINTER(ConvWgradArgs), i32, C.POINTER(ConvWgradPlan)]),
    "memhip_conv_wgrad_workspace": (sz, [C.POINTER(ConvWgradArgs), i32]),
    "memhip_relu_bwd_colsum": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, sz, vp]),
    "memhip_relu_bwd_colsum_workspace": (sz, [i32, i32, i32, i32]),
})


def conv_wgrad_args(B, Hs, Ws, C_, N, ksize, stride, pad, small=None, big=None, grad=None, small_padded=True, accumulate=False,
                    workspace=None, workspace_bytes=0):
    """The memhip_conv_wgrad_args_t of conv_wgrad / conv_wgrad_plan; the tensors are addresses or None."""
    return ConvWgradArgs(small, big, grad, workspace, workspace_bytes, B, Hs, Ws, C_, N, ksize, stride, pad, int(small_padded),
                         int(accumulate))


def conv_wgrad_plan(B, Hs, Ws, C_, N, ksize, stride, pad, small_padded=True, device_cus=None):
    """The ConvWgradPlan of conv_wgrad for this layer: tiles, slices of the pixel range, grid, LDS and workspace bytes.
    Validates like the call; nothing is launched, and no device is needed when device_cus is given."""
    plan = ConvWgradPlan()
    a = conv_wgrad_args(B, Hs, Ws, C_, N, ksize, stride, pad, small_padded=small_padded)
    check(lib.memhip_conv_wgrad_plan(C.byref(a), -1 if device_cus is None else device_cus, C.byref(plan)), "conv_wgrad_plan")
    return plan


def conv_wgrad_workspace(B, Hs, Ws, C_, N, ksize, stride, pad, small_padded=True, device_cus=None):
    """Workspace bytes conv_wgrad needs for this layer (0: one slice, no workspace)."""
    a = conv_wgrad_args(B, Hs, Ws, C_, N, ksize, stride, pad, small_padded=small_padded)
    return int(lib.memhip_conv_wgrad_workspace(C.byref(a), -1 if device_cus is None else device_cus))


def conv_wgrad(small, big, grad, B, Hs, Ws, C_, N, ksize, stride, pad, small_padded=True, accumulate=False, workspace=None):
    """grad f32 [N, k*k*C] (+)= sum over the pixels (b, y, x) of the Hs x Ws grid of
    small[b, y, x, n] * big_pad[b, s*y + ky + 1 - pad, s*x + kx + 1 - pad, c]: the weight gradient of Conv2d (small = g of the
    pre-activation, big = the layer's input), of ConvTranspose2d(4, 2, 1) (small = the layer's input, big = g of its output:
    torch's dW[ci, co, ky, kx] = grad[ci, (ky, kx, co)]) and of the 1x1 heads (small dense, small_padded=False).
    small bf16 padded [B, Hs+2, Ws+2, N] or dense [B*Hs*Ws, N]; big bf16 padded [B, s*Hs+2, s*Ws+2, C] with a ZERO ring.
    workspace: a 16-byte aligned tensor of >= conv_wgrad_workspace(...) bytes (None only when that is 0).  No atomics: two
    calls give the same bits."""
    assert small.dtype == torch.bfloat16 and big.dtype == torch.bfloat16 and grad.dtype == torch.float32
    assert small.is_contiguous() and big.is_contiguous() and grad.is_contiguous()
    assert small.numel() >= (B * (Hs + 2) * (Ws + 2) * N if small_padded else B * Hs * Ws * N)
    assert big.numel() >= B * (stride * Hs + 2) * (stride * Ws + 2) * C_ and grad.numel() >= N * ksize * ksize * C_
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    a = conv_wgrad_args(B, Hs, Ws, C_, N, ksize, stride, pad, _p(small), _p(big), _p(grad), small_padded, accumulate,
                        _p(workspace), ws_bytes)
    check(lib.memhip_conv_wgrad_nhwc(C.byref(a), stream_ptr()), "conv_wgrad")


def relu_bwd_colsum_workspace(B, H, W, C_):
    return int(lib.memhip_relu_bwd_colsum_workspace(B, H, W, C_))


def relu_bwd_colsum(g, y, B, H, W, C_, padded=True, colsum=None, accumulate=False, workspace=None):
    """In place g *= (y > 0) over the B*H*W pixels of a bf16 buffer of C channels (padded [B, H+2, W+2, C]: the ring is not
    touched; or dense [B*H*W, C]); y None: no mask.  colsum f32 [C] (+)= the column sums of the masked g (the bias gradient),
    through per-workgroup partial sums in `workspace` (>= relu_bwd_colsum_workspace bytes) folded in a fixed order."""
    assert g.dtype == torch.bfloat16 and g.is_contiguous() and (y is None or (y.dtype == torch.bfloat16 and y.is_contiguous()))
    n = B * (H + 2) * (W + 2) * C_ if padded else B * H * W * C_
    assert g.numel() >= n and (y is None or y.numel() >= n)
    assert colsum is None or (colsum.dtype == torch.float32 and colsum.numel() >= C_)
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    check(lib.memhip_relu_bwd_colsum(_p(g), _p(y), int(padded), B, H, W, C_, _p(colsum), int(accumulate), _p(workspace), ws_bytes,
                                     stream_ptr()), "relu_bwd_colsum")


# ---------------------------------------------------------------- finetuning recipe (csrc/finetune_recipe.hip)
declare({
    "memhip_mixup": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "memhip_mix_targets": (i32, [vp, vp, i32, i32, C.c_double, vp, i64, vp]),
    "memhip_ce_soft": (i32, [vp, i32, i64, vp, i64, vp, f32, i32, i32, f32, vp, i64, vp, vp, i32, vp, vp]),
    "memhip_ema_update": (i32, [vp, vp, i64, C.c_double, vp]),
})


def mixup(x, lam, box, lam_host=None, box_host=None):
    """x f32 [B, C, H, W] mixed in place with its flipped self; lam f32 [B], box i32 [B, 4] (yl, yh, xl, xh) on the device;
    lam_host / box_host: numpy copies of the same values, validated before the launch."""
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4, "mixup: contiguous fp32 [B, C, H, W]"
    assert lam.dtype == torch.float32 and box.dtype == torch.int32 and lam.numel() == x.shape[0] and box.numel() == 4 * x.shape[0]
    B, Cc, H, W = x.shape
    check(lib.memhip_mixup(ptr(x), B, Cc, H, W, ptr(lam), ptr(box),
                           None if lam_host is None else lam_host.ctypes.data_as(vp),
                           None if box_host is None else box_host.ctypes.data_as(vp), stream_ptr()), "mixup")


def mix_targets(labels, lam, V, smoothing, out):
    """out f32 [B, V] = lam * onehot(labels) + (1 - lam) * onehot(labels.flip(0)), smoothed one-hots (timm mixup_target)."""
    assert labels.dtype == torch.int64 and labels.is_contiguous() and lam.dtype == torch.float32
    assert out.dtype == torch.float32 and out.stride(1) == 1 and out.shape == (labels.numel(), V)
    check(lib.memhip_mix_targets(ptr(labels), ptr(lam), labels.numel(), V, float(smoothing), ptr(out), out.stride(0),
                                 stream_ptr()), "mix_targets")


def ce_soft(logits, row_loss, row_correct, out2, target=None, labels=None, smoothing=0.0, grad_scale=1.0, dlogits=None):
    """Soft-target (target f32 [M, V]) or label-smoothing (labels i64 [M]) cross-entropy of bf16 / fp32 logits [M, V], any
    V >= 2; out2 = {mean loss, top-1 accuracy}; dlogits (may be the logits) = grad_scale * d(sum of row losses)/dlogits."""
    assert logits.dtype in (torch.bfloat16, torch.float32) and logits.dim() == 2 and logits.stride(1) == 1
    M, V = logits.shape
    if target is not None:
        assert target.dtype == torch.float32 and target.shape == (M, V) and target.stride(1) == 1
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.numel() == M and labels.is_contiguous()
    if dlogits is not None:
        assert dlogits.dtype == logits.dtype and dlogits.shape == (M, V) and dlogits.stride(1) == 1
    check(lib.memhip_ce_soft(ptr(logits), int(logits.dtype == torch.float32), logits.stride(0), ptr(target),
                             target.stride(0) if target is not None else 0, ptr(labels), float(smoothing), M, V,
                             float(grad_scale), ptr(dlogits), dlogits.stride(0) if dlogits is not None else 0,
                             ptr(row_loss), ptr(row_correct), int(dlogits is not None), ptr(out2), stream_ptr()), "ce_soft")


def ema_update(ema, p, decay):
    """ema = decay * ema + (1 - decay) * p over two flat fp32 buffers of equal length."""
    assert ema.dtype == torch.float32 and p.dtype == torch.float32 and ema.numel() == p.numel()
    assert ema.is_contiguous() and p.is_contiguous()
    check(lib.memhip_ema_update(ptr(ema), ptr(p), ema.numel(), float(decay), stream_ptr()), "ema_update")


# ---------------------------------------------------------------- token pooling of the finetuning head (csrc/pool.hip)
declare({
    "memhip_pool_tokens": (i32, [vp, i64, i32, i32, i32, vp, vp]),
    "memhip_pool_tokens_bwd": (i32, [vp, i32, i32, i32, vp, vp]),
})


def pool_tokens(x, B, T, out=None):
    """x f32 [>= B*T, D] (row stride >= D) -> out f32 [B, D]: mean of each sample's rows 1 .. T-1 (the cls row is skipped;
    modeling_finetune.py:349-354), fixed summation order."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] >= B * T
    D = x.shape[1]
    if out is None:
        out = torch.empty((B, D), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.shape == (B, D) and out.is_contiguous()
    check(lib.memhip_pool_tokens(ptr(x), x.stride(0), B, T, D, ptr(out), stream_ptr()), "pool_tokens")
    return out


def pool_tokens_bwd(dout, T, dx=None):
    """dout f32 [B, D] -> dx f32 [B*T, D]: dout[b] / (T - 1) on the token rows, 0 on the cls rows (every element written)."""
    assert dout.dtype == torch.float32 and dout.dim() == 2 and dout.is_contiguous()
    B, D = dout.shape
    if dx is None:
        dx = torch.empty((B * T, D), dtype=torch.float32, device=dout.device)
    assert dx.dtype == torch.float32 and dx.is_contiguous() and dx.numel() == B * T * D
    check(lib.memhip_pool_tokens_bwd(ptr(dout), B, T, D, ptr(dx), stream_ptr()), "pool_tokens_bwd")
    return dx


# ---------------------------------------------------------------- dense per-block feature maps (csrc/dense.hip)
declare({
    "memhip_tokens_to_maps": (i32, [vp, i64, i32, i32, i32, i32, vp, vp]),
    "memhip_maps_to_tokens_add": (i32, [vp, i32, i32, i32, i32, vp, i64, vp]),
})


def tokens_to_maps(x, B, T, out=None, b0=0, b1=None):
    """x f32 [>= B*T, D] (row stride >= D) -> out f32 [B, D, T-1]: out[b, d, l] = x[b*T + 1 + l, d] for the samples
    b0 <= b < b1 (default: all B); the cls row is skipped (semantic_segmentation/backbone/mem.py:439-441)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] >= B * T
    D = x.shape[1]
    if out is None:
        out = torch.empty((B, D, T - 1), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * D * (T - 1)
    b1 = B if b1 is None else b1
    assert 0 <= b0 < b1 <= B, (b0, b1, B)
    check(lib.memhip_tokens_to_maps(ptr(x), x.stride(0), b0, b1, T, D, ptr(out), stream_ptr()), "tokens_to_maps")
    return out


def maps_to_tokens_add(dmap, dx, B, T, b0=0, b1=None):
    """dx f32 [>= B*T, D] (row stride >= D): dx[b*T + 1 + l, d] += dmap[b, d, l] (dmap f32 [B, D, T-1] contiguous, any
    trailing shape of T-1 elements) for b0 <= b < b1; cls rows untouched, one fp32 add per element."""
    assert dx.dtype == torch.float32 and dx.dim() == 2 and dx.stride(1) == 1 and dx.shape[0] >= B * T
    D = dx.shape[1]
    assert dmap.dtype == torch.float32 and dmap.is_contiguous() and dmap.numel() == B * D * (T - 1)
    b1 = B if b1 is None else b1
    assert 0 <= b0 < b1 <= B, (b0, b1, B)
    check(lib.memhip_maps_to_tokens_add(ptr(dmap), b0, b1, T, D, ptr(dx), dx.stride(0), stream_ptr()), "maps_to_tokens_add")
    return dx


# ---------------------------------------------------------------- feature-pyramid necks (csrc/necks.hip)
declare({
    "memhip_neck_maps_to_rows": (i32, [vp, i32, i32, i32, i32, i32, vp, vp]),
    "memhip_neck_rows_to_maps": (i32, [vp, i32, i32, i32, i32, i32, vp, vp]),
    "memhip_neck_sums_workspace": (sz, [i32]),
    "memhip_neck_colstats": (i32, [vp, i64, i32, vp, vp, sz, vp, vp]),
    "memhip_neck_bn_gelu_fwd": (i32, [vp, i64, i32, vp, vp, vp, vp, vp, vp]),
    "memhip_neck_bn_gelu_bwd_sums": (i32, [vp, vp, i64, i32, vp, vp, vp, vp, vp, sz, vp, vp]),
    "memhip_neck_bn_gelu_bwd_apply": (i32, [vp, vp, i64, i32, vp, vp, vp, vp, vp, f32, vp, vp]),
})
NECK_GROUPS = 128        # == MEMHIP_NECK_GROUPS: the most partials per channel of the two-stage column sums


def _neck_rows_shape(B, D, Hp, Wp, level):
    R0 = B * Hp * Wp
    return (R0, D) if level == 0 else (R0 * 4 ** (level - 1), 4 * D)


def neck_maps_to_rows(x, level, out=None):
    """x f32 [B, D, 2^level Hp, 2^level Wp] contiguous -> bf16 rows: [B Hp Wp, D] (level 0) or the interleaved
    [B Hp Wp 4^(level-1), 4D] of a map upsampled `level` times (include/memhip.h: the nested row / column order)."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and level in (0, 1, 2)
    B, D = x.shape[:2]
    Hp, Wp = x.shape[2] >> level, x.shape[3] >> level
    assert (Hp << level, Wp << level) == tuple(x.shape[2:]), (tuple(x.shape), level)
    shape = _neck_rows_shape(B, D, Hp, Wp, level)
    if out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == shape
    check(lib.memhip_neck_maps_to_rows(ptr(x), B, D, Hp, Wp, level, ptr(out), stream_ptr()), "neck_maps_to_rows")
    return out


def neck_rows_to_maps(rows, B, D, Hp, Wp, level, out=None):
    """The inverse of neck_maps_to_rows: bf16 rows -> f32 [B, D, 2^level Hp, 2^level Wp]."""
    assert rows.dtype == torch.bfloat16 and rows.is_contiguous() and tuple(rows.shape) == _neck_rows_shape(B, D, Hp, Wp, level)
    shape = (B, D, Hp << level, Wp << level)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=rows.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape
    check(lib.memhip_neck_rows_to_maps(ptr(rows), B, D, Hp, Wp, level, ptr(out), stream_ptr()), "neck_rows_to_maps")
    return out


def _sums_out(out, rows, C_, device):
    """The f32 [rows, C] output of a two-stage column sum ([3, C]: count, sum, sum of squares; [2, C]: sum g, sum g xhat)."""
    if out is None:
        out = torch.empty((rows, C_), dtype=torch.float32, device=device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == rows * C_
    return out


def neck_sums_workspace(D, device):
    return torch.empty(int(lib.memhip_neck_sums_workspace(D)) // 4, dtype=torch.float32, device=device)


def neck_colstats(y, shift, ws, out=None):
    """y bf16 [R, 4D] interleaved, shift f32 [D] -> out f32 [3, D]: count, sum (x - shift), sum (x - shift)^2 per channel."""
    R, D = y.shape[0], y.shape[1] // 4
    assert y.dtype == torch.bfloat16 and y.is_contiguous() and shift.dtype == torch.float32 and shift.numel() == D
    out = _sums_out(out, 3, D, y.device)
    check(lib.memhip_neck_colstats(ptr(y), R, D, ptr(shift), ptr(ws), ws.numel() * 4, ptr(out), stream_ptr()), "neck_colstats")
    return out


def neck_bn_gelu_fwd(y, mean, rstd, gamma, beta, out=None):
    """y bf16 [R, 4D] interleaved -> bf16 [4R, D] = gelu(gamma (y - mean) rstd + beta), de-interleaved."""
    R, D = y.shape[0], y.shape[1] // 4
    assert y.dtype == torch.bfloat16 and y.is_contiguous()
    assert all(v.dtype == torch.float32 and v.numel() == D and v.is_contiguous() for v in (mean, rstd, gamma, beta))
    if out is None:
        out = torch.empty((4 * R, D), dtype=torch.bfloat16, device=y.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (4 * R, D)
    check(lib.memhip_neck_bn_gelu_fwd(ptr(y), R, D, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(out), stream_ptr()),
          "neck_bn_gelu_fwd")
    return out


def neck_bn_gelu_bwd_sums(da, y, mean, rstd, gamma, beta, ws, out=None):
    """out f32 [2, D] = per channel sum g, sum g xhat with g = da gelu'(gamma xhat + beta) (da bf16 [4R, D], y bf16 [R, 4D])."""
    R, D = y.shape[0], y.shape[1] // 4
    assert y.dtype == torch.bfloat16 and y.is_contiguous() and da.dtype == torch.bfloat16 and da.is_contiguous()
    assert tuple(da.shape) == (4 * R, D)
    assert all(v.dtype == torch.float32 and v.numel() == D and v.is_contiguous() for v in (mean, rstd, gamma, beta))
    out = _sums_out(out, 2, D, y.device)
    check(lib.memhip_neck_bn_gelu_bwd_sums(ptr(da), ptr(y), R, D, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(ws),
                                           ws.numel() * 4, ptr(out), stream_ptr()), "neck_bn_gelu_bwd_sums")
    return out


def neck_bn_gelu_bwd_apply(da, y, mean, rstd, gamma, beta, sums, inv_n, out=None):
    """dy bf16 [R, 4D] interleaved = gamma rstd (g - sums[0] inv_n - xhat sums[1] inv_n)."""
    R, D = y.shape[0], y.shape[1] // 4
    assert y.dtype == torch.bfloat16 and y.is_contiguous() and da.dtype == torch.bfloat16 and da.is_contiguous()
    assert tuple(da.shape) == (4 * R, D) and sums.dtype == torch.float32 and sums.is_contiguous() and sums.numel() == 2 * D
    assert all(v.dtype == torch.float32 and v.numel() == D and v.is_contiguous() for v in (mean, rstd, gamma, beta))
    if out is None:
        out = torch.empty((R, 4 * D), dtype=torch.bfloat16, device=y.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (R, 4 * D)
    check(lib.memhip_neck_bn_gelu_bwd_apply(ptr(da), ptr(y), R, D, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(sums),
                                            float(inv_n), ptr(out), stream_ptr()), "neck_bn_gelu_bwd_apply")
    return out


# ---------------------------------------------------------------- segmentation loss and metrics (csrc/seg_loss.hip, seg_plan.cpp)
class SegArgs(C.Structure):
    """== memhip_seg_args_t."""
    _fields_ = [("logits", vp), ("sb", i64), ("sc", i64), ("sy", i64), ("sx", i64), ("labels", vp)] + \
               [(n, i32) for n in ("B", "C", "h", "w", "H", "W", "ignore_index", "align_corners", "avg_non_ignore")] + \
               [("loss_weight", f32)] + \
               [(n, vp) for n in ("y_i0", "y_w1", "y_lo", "y_hi", "x_i0", "x_w1", "x_lo", "x_hi", "dz")] + \
               [(n, i64) for n in ("db", "dc", "dy", "dx")] + \
               [("loss", vp), ("stats", vp), ("workspace", vp), ("workspace_bytes", sz), ("confusion", vp)]


class SegPlan(C.Structure):
    """== memhip_seg_plan_t."""
    _fields_ = [(n, i32) for n in ("tile_h", "tile_w", "tiles_y", "tiles_x", "grid", "block", "chunk", "max_fh", "max_fw",
                                   "tables_in_lds", "lds_bytes", "slot_bytes", "conf_grid", "conf_block", "conf_lds_bytes",
                                   "reserved")] + [("ws_bytes", C.c_uint64)]


declare({
    "memhip_seg_axis_table": (i32, [i32, i32, i32, vp, vp, vp, vp]),
    "memhip_seg_plan": (i32, [C.POINTER(SegArgs), C.POINTER(SegPlan)]),
    "memhip_seg_ce": (i32, [C.POINTER(SegArgs), vp]),
    "memhip_seg_confusion": (i32, [C.POINTER(SegArgs), vp]),
})


def seg_axis_table(n_in, n_out, align_corners):
    """The bilinear table of one axis as host arrays (i0 i32 [out], w1 f32 [out], lo i32 [in], hi i32 [in]): output y reads
    inputs i0[y] and min(i0[y] + 1, in - 1) with weights 1 - w1[y] and w1[y]; lo[i] .. hi[i] are the outputs that read input i.
    No device needed."""
    import numpy as np
    i0, w1 = np.empty(max(n_out, 0), np.int32), np.empty(max(n_out, 0), np.float32)
    lo, hi = np.empty(max(n_in, 0), np.int32), np.empty(max(n_in, 0), np.int32)
    check(lib.memhip_seg_axis_table(n_in, n_out, int(align_corners), i0.ctypes.data, w1.ctypes.data, lo.ctypes.data,
                                    hi.ctypes.data), "seg_axis_table")
    return i0, w1, lo, hi


_SEG_TABLES = {}


def seg_tables(n_in, n_out, align_corners, device):
    """The table of seg_axis_table on the device: one i32 tensor [2 out + 2 in] = i0 | bits of w1 | lo | hi, uploaded once
    per (in, out, align_corners, device) and kept."""
    key = (n_in, n_out, bool(align_corners), str(device))
    t = _SEG_TABLES.get(key)
    if t is None:
        import numpy as np
        i0, w1, lo, hi = seg_axis_table(n_in, n_out, align_corners)
        t = _SEG_TABLES[key] = torch.from_numpy(np.concatenate([i0, w1.view(np.int32), lo, hi])).to(device)
    return t


def _table_ptrs(t, n_in, n_out):
    p = t.data_ptr()
    return p, p + 4 * n_out, p + 8 * n_out, p + 8 * n_out + 4 * n_in


def seg_args(B, C_, h, w, H, W, ignore_index=255, align_corners=False, avg_non_ignore=False, loss_weight=1.0, **fields):
    """The memhip_seg_args_t of seg_ce / seg_confusion / seg_plan; pointer fields are addresses or None."""
    a = SegArgs(B=B, C=C_, h=h, w=w, H=H, W=W, ignore_index=-1 if ignore_index is None else int(ignore_index),
                align_corners=int(align_corners), avg_non_ignore=int(avg_non_ignore), loss_weight=float(loss_weight))
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def seg_plan(B, C_, h, w, H, W, align_corners=False):
    """The SegPlan of a call with these shapes: tiles, grid, LDS bytes, workspace bytes.  Validates like the call; no device."""
    plan = SegPlan()
    check(lib.memhip_seg_plan(C.byref(seg_args(B, C_, h, w, H, W, align_corners=align_corners)), C.byref(plan)), "seg_plan")
    return plan


def _seg_common(logits, labels, ignore_index, align_corners, **kw):
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4, "logits: a CUDA f32 tensor [B, C, h, w] (any strides)"
    assert labels.is_cuda and labels.dtype == torch.uint8 and labels.dim() == 3 and labels.is_contiguous(), \
        "labels: a contiguous CUDA u8 tensor [B, H, W]"
    B, C_, h, w = logits.shape
    assert labels.shape[0] == B, (tuple(logits.shape), tuple(labels.shape))
    H, W = labels.shape[1:]
    a = seg_args(B, C_, h, w, H, W, ignore_index, align_corners, logits=logits.data_ptr(), labels=labels.data_ptr(), **kw)
    a.sb, a.sc, a.sy, a.sx = logits.stride()
    ty, tx = seg_tables(h, H, align_corners, logits.device), seg_tables(w, W, align_corners, logits.device)
    a.y_i0, a.y_w1, a.y_lo, a.y_hi = _table_ptrs(ty, h, H)
    a.x_i0, a.x_w1, a.x_lo, a.x_hi = _table_ptrs(tx, w, W)
    return a, (ty, tx)


def seg_ce(logits, labels, dz, loss, stats, workspace, ignore_index=255, align_corners=False, avg_non_ignore=False, loss_weight=1.0):
    """Bilinear resize of logits f32 [B, C, h, w] (any strides) to the labels' size + cross entropy, nothing upsampled in
    memory.  labels u8 [B, H, W]; dz f32 [B, C, h, w] (any non-overlapping strides) <- the UNSCALED gradient sum of weight *
    (softmax - onehot); loss f32 [3] <- loss, loss_weight / N, loss_sum; stats i64 [3] <- n_valid, n_correct, n_bad;
    workspace: >= seg_plan(...).ws_bytes bytes.  The gradient of `loss` with respect to the logits is dz * loss[1]."""
    assert dz.dtype == torch.float32 and tuple(dz.shape) == tuple(logits.shape) and dz.is_cuda
    assert loss.dtype == torch.float32 and loss.numel() >= 3 and loss.is_contiguous()
    assert stats.dtype == torch.int64 and stats.numel() >= 3 and stats.is_contiguous()
    a, keep = _seg_common(logits, labels, ignore_index, align_corners, avg_non_ignore=int(avg_non_ignore),
                          loss_weight=float(loss_weight), dz=dz.data_ptr(), loss=loss.data_ptr(), stats=stats.data_ptr(),
                          workspace=workspace.data_ptr(), workspace_bytes=workspace.numel() * workspace.element_size())
    a.db, a.dc, a.dy, a.dx = dz.stride()
    check(lib.memhip_seg_ce(C.byref(a), stream_ptr()), "seg_ce")


def seg_confusion(logits, labels, confusion, ignore_index=255, align_corners=False):
    """confusion i64 [C, C] (row = label, column = argmax of the resized logits, ties to the lowest class) += the counts of
    this batch; ignored labels and labels >= C are skipped."""
    C_ = logits.shape[1]
    assert confusion.dtype == torch.int64 and tuple(confusion.shape) == (C_, C_) and confusion.is_contiguous() and confusion.is_cuda
    a, keep = _seg_common(logits, labels, ignore_index, align_corners, confusion=confusion.data_ptr())
    check(lib.memhip_seg_confusion(C.byref(a), stream_ptr()), "seg_confusion")


# ---------------------------------------------------------------- class weights and OHEM in the fused loss (csrc/seg_ohem.hip, seg_loss.hip)
SEG_SAMPLER_NONE, SEG_SAMPLER_THRESH, SEG_SAMPLER_TOPK = 0, 1, 2


class SegOhemArgs(C.Structure):
    """== memhip_segohem_args_t."""
    _fields_ = [("seg", SegArgs), ("class_weight", vp), ("sampler", i32), ("thresh", f32), ("min_kept", i64), ("keys", vp),
                ("threshold", vp)]


class SegOhemPlan(C.Structure):
    """== memhip_segohem_plan_t."""
    _fields_ = [("seg", SegPlan)] + \
               [(n, i32) for n in ("keys_grid", "keys_block", "select_grid", "select_block", "select_passes", "select_bins",
                                   "select_lds_bytes", "reserved")] + \
               [(n, C.c_uint64) for n in ("select_ws_offset", "select_ws_bytes", "ws_bytes")]


declare({
    "memhip_seg_ohem_plan": (i32, [C.POINTER(SegOhemArgs), C.POINTER(SegOhemPlan)]),
    "memhip_seg_ohem_keys": (i32, [C.POINTER(SegOhemArgs), vp]),
    "memhip_seg_ohem_select": (i32, [C.POINTER(SegOhemArgs), vp]),
    "memhip_seg_ce_w": (i32, [C.POINTER(SegOhemArgs), vp]),
})


def seg_ohem_args(seg, sampler=0, thresh=None, min_kept=0, **fields):
    """The memhip_segohem_args_t around a SegArgs; sampler: 0 none, 1 thresh, 2 top-k; pointer fields are addresses or None."""
    a = SegOhemArgs(seg=seg, sampler=int(sampler), thresh=0.0 if thresh is None else float(thresh), min_kept=int(min_kept))
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def seg_ohem_plan(B, C_, h, w, H, W, align_corners=False, sampler=0, thresh=None, min_kept=0):
    """The SegOhemPlan of calls with these shapes and this sampler: the training kernel's plan, the grids of the key and
    selection passes, and the workspace bytes (the selection's part behind the partials).  Validates like the calls; no device."""
    keys = 0x1000 if sampler else None                  # the query wants to know that they will be there, not where
    a = seg_ohem_args(seg_args(B, C_, h, w, H, W, align_corners=align_corners), sampler, thresh, min_kept, keys=keys, threshold=keys)
    plan = SegOhemPlan()
    check(lib.memhip_seg_ohem_plan(C.byref(a), C.byref(plan)), "seg_ohem_plan")
    return plan


def _f32_ptr(t, n, name):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, "%s: a contiguous CUDA f32 tensor of %d" % (name, n)
    return t.data_ptr()


def _seg_ohem_common(logits, labels, ignore_index, align_corners, sampler, thresh, min_kept, class_weight, keys, threshold, **kw):
    a, keep = _seg_common(logits, labels, ignore_index, align_corners, **kw)
    B, C_ = logits.shape[:2]
    f = {}
    if class_weight is not None:
        f["class_weight"] = _f32_ptr(class_weight, C_, "class_weight")
    if keys is not None:
        f["keys"] = _f32_ptr(keys, labels.numel(), "keys")
    if threshold is not None:
        f["threshold"] = _f32_ptr(threshold, 1, "threshold")
    return seg_ohem_args(a, sampler, thresh, min_kept, **f), keep


def seg_ohem_keys(logits, labels, keys, threshold, sampler, class_weight=None, ignore_index=255, align_corners=False):
    """keys f32 [B, H, W] <- the sampler's key of every output pixel of the resized logits: sampler 1 softmax[label], sampler 2
    class_weight[label] * nll (class_weight f32 [C] or None: ones); -1.0 where the label is ignored or >= C.  threshold f32 [1]
    is the sampler's (the three calls of a sampler take one struct); this call does not touch it."""
    a, keep = _seg_ohem_common(logits, labels, ignore_index, align_corners, sampler, 1.0, 0, class_weight, keys, threshold)
    check(lib.memhip_seg_ohem_keys(C.byref(a), stream_ptr()), "seg_ohem_keys")
    return keys


def seg_ohem_select(keys, threshold, stats, workspace, sampler, thresh=None, min_kept=100000, logits_shape=None):
    """threshold f32 [1] <- the sampler's threshold over the keys >= 0 of keys f32 [B, H, W] (batch = B; K = min_kept * B):
    sampler 1: max(the key of ascending rank min(K, n - 1), thresh), kept are the keys below it (-inf: none); sampler 2: the
    K-th largest key, kept are the keys >= it, ties included (+inf: none).  stats i64 [4]: stats[3] <- n_kept.  workspace: >=
    seg_ohem_plan(...).ws_bytes bytes for logits_shape = (C, h, w), cleared by the call where it needs it cleared; the
    selection reads no logits, and without logits_shape the smallest map stands in (the selection's part of the workspace
    lies behind the partials of that shape).  Exact, no host synchronisation."""
    assert keys.is_cuda and keys.dtype == torch.float32 and keys.is_contiguous() and keys.dim() == 3
    assert stats.dtype == torch.int64 and stats.numel() >= 4 and stats.is_contiguous() and stats.is_cuda
    assert workspace.is_cuda
    B, H, W = keys.shape
    C_, h, w = (2, 1, 1) if logits_shape is None else logits_shape
    seg = seg_args(B, C_, h, w, H, W, stats=stats.data_ptr(), workspace=workspace.data_ptr(),
                   workspace_bytes=workspace.numel() * workspace.element_size())
    a = seg_ohem_args(seg, sampler, thresh, min_kept, keys=keys.data_ptr(), threshold=_f32_ptr(threshold, 1, "threshold"))
    check(lib.memhip_seg_ohem_select(C.byref(a), stream_ptr()), "seg_ohem_select")
    return threshold


def seg_ce_w(logits, labels, dz, loss, stats, workspace, ignore_index=255, align_corners=False, avg_non_ignore=False, loss_weight=1.0,
             class_weight=None, sampler=0, keys=None, threshold=None):
    """seg_ce with class weights and the sampler's pixel weight: q and the loss term of a valid pixel are multiplied by
    class_weight[label] * s, s = 1 without a sampler, else [key < threshold] (sampler 1) or [key >= threshold] (sampler 2) on
    the stored keys f32 [B, H, W] and threshold f32 [1] of seg_ohem_keys / seg_ohem_select.  stats i64 [4] <- n_valid, n_correct,
    n_bad, n_kept.  With neither, or with weights of 1.0, loss, dz and stats[:3] are seg_ce's bits.  workspace: >=
    seg_ohem_plan(...).ws_bytes bytes."""
    assert dz.dtype == torch.float32 and tuple(dz.shape) == tuple(logits.shape) and dz.is_cuda
    assert loss.dtype == torch.float32 and loss.numel() >= 3 and loss.is_contiguous()
    assert stats.dtype == torch.int64 and stats.numel() >= 4 and stats.is_contiguous()
    a, keep = _seg_ohem_common(logits, labels, ignore_index, align_corners, sampler, 1.0, 0, class_weight, keys, threshold,
                               avg_non_ignore=int(avg_non_ignore), loss_weight=float(loss_weight), dz=dz.data_ptr(),
                               loss=loss.data_ptr(), stats=stats.data_ptr(), workspace=workspace.data_ptr(),
                               workspace_bytes=workspace.numel() * workspace.element_size())
    a.seg.db, a.seg.dc, a.seg.dy, a.seg.dx = dz.stride()
    check(lib.memhip_seg_ce_w(C.byref(a), stream_ptr()), "seg_ce_w")


# ---------------------------------------------------------------- segmentation inference (csrc/seg_predict.hip, seg_predict_plan.cpp)
class SegPredictArgs(C.Structure):
    """== memhip_segpredict_args_t."""
    _fields_ = [("logits", vp)] + [(n, i64) for n in ("sv", "sb", "sc", "sy", "sx")] + [("rects", vp)] + \
               [(n, i32) for n in ("V", "B", "C", "h", "w", "hc", "wc", "H", "W", "align_corners", "ignore_index", "reserved0")] + \
               [(n, vp) for n in ("y_i0", "y_w1", "x_i0", "x_w1", "pred", "prob", "labels", "confusion")]


class SegPredictPlan(C.Structure):
    """== memhip_segpredict_plan_t."""
    _fields_ = [(n, i32) for n in ("tile_h", "tile_w", "tiles_y", "tiles_x", "grid", "block", "lds_bytes", "pixels_per_thread",
                                   "padded_classes", "passes", "max_count", "pred_dwords")]


declare({
    "memhip_seg_predict": (i32, [C.POINTER(SegPredictArgs), vp]),
    "memhip_seg_predict_plan": (i32, [C.POINTER(SegPredictArgs), C.POINTER(SegPredictPlan)]),
})


def seg_predict_args(rects, B, C_, hw, window, out_size, align_corners=False, ignore_index=255, **fields):
    """The memhip_segpredict_args_t of seg_predict / seg_predict_plan.  rects: [(y1, x1, flip)] per view, kept in HOST memory
    (the returned ``keep`` must outlive the call); pointer fields are addresses or None."""
    import numpy as np
    r = np.ascontiguousarray(np.asarray(rects, dtype=np.int32).reshape(-1, 3))
    a = SegPredictArgs(V=int(r.shape[0]), B=B, C=C_, h=int(hw[0]), w=int(hw[1]), hc=int(window[0]), wc=int(window[1]),
                       H=int(out_size[0]), W=int(out_size[1]), align_corners=int(align_corners),
                       ignore_index=-1 if ignore_index is None else int(ignore_index), rects=r.ctypes.data)
    for k, v in fields.items():
        setattr(a, k, v)
    return a, r


def seg_predict_plan(rects, B, C_, hw, window, out_size, align_corners=False, **fields):
    """The SegPredictPlan of a call with these shapes and rectangles: tiles, grid, LDS bytes, passes and the largest count.
    Validates like the call (outputs included: pass dummy addresses as ``pred=...``); no device."""
    a, keep = seg_predict_args(rects, B, C_, hw, window, out_size, align_corners, **fields)
    plan = SegPredictPlan()
    check(lib.memhip_seg_predict_plan(C.byref(a), C.byref(plan)), "seg_predict_plan")
    return plan


def seg_predict(logits, rects, window, out_size, pred=None, prob=None, labels=None, confusion=None, align_corners=False,
                ignore_index=255):
    """The label map of a segmentation model from the logits of V views (mmseg's slide_inference / whole_inference ->
    softmax -> flip -> mean over the passes -> argmax), nothing upsampled in memory.

    logits f32 [V, B, C, h, w], or [V B, C, h, w] with the views stacked in the batch (any strides: NCHW or the heads' pixel
    rows); rects [(y1, x1, flip)] per view, flipped views in the coordinates of the flipped canvas; window (hc, wc) of every
    view; out_size (H, W).  Outputs, each optional: pred u8 [B, H, W]; prob f32 [B, C, H, W]; labels u8 [B, H, W] with
    confusion i64 [C, C] (+= the counts, ignore_index and labels >= C skipped).  Returns pred."""
    V = len(rects)
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() in (4, 5), "logits: a CUDA f32 tensor [V, B, C, h, w] or [V B, C, h, w]"
    if logits.dim() == 5:
        assert logits.shape[0] == V, (tuple(logits.shape), V)
        B, C_, h, w = logits.shape[1:]
        sv, (sb, sc, sy, sx) = logits.stride(0), logits.stride()[1:]
    else:
        assert V >= 1 and logits.shape[0] % V == 0, (tuple(logits.shape), V)
        B, C_, h, w = logits.shape[0] // V, logits.shape[1], logits.shape[2], logits.shape[3]
        sb, sc, sy, sx = logits.stride()
        sv = B * sb
    H, W = int(out_size[0]), int(out_size[1])
    dev = logits.device
    f = {}
    if pred is not None:
        assert pred.is_cuda and pred.dtype == torch.uint8 and pred.is_contiguous() and tuple(pred.shape) == (B, H, W), "pred: CUDA u8 [B, H, W]"
        f["pred"] = pred.data_ptr()
    if prob is not None:
        assert prob.is_cuda and prob.dtype == torch.float32 and prob.is_contiguous() and tuple(prob.shape) == (B, C_, H, W), \
            "prob: CUDA f32 [B, C, H, W]"
        f["prob"] = prob.data_ptr()
    if labels is not None:
        assert labels.is_cuda and labels.dtype == torch.uint8 and labels.is_contiguous() and tuple(labels.shape) == (B, H, W), \
            "labels: CUDA u8 [B, H, W]"
        f["labels"] = labels.data_ptr()
    if confusion is not None:
        assert confusion.is_cuda and confusion.dtype == torch.int64 and confusion.is_contiguous() and tuple(confusion.shape) == (C_, C_), \
            "confusion: CUDA i64 [C, C]"
        f["confusion"] = confusion.data_ptr()
    a, keep = seg_predict_args(rects, B, C_, (h, w), window, (H, W), align_corners, ignore_index, logits=logits.data_ptr(), **f)
    a.sv, a.sb, a.sc, a.sy, a.sx = sv, sb, sc, sy, sx
    if B > 0 and 1 <= h <= a.hc and 1 <= w <= a.wc:        # (a shape the tables cannot be made for is rejected by the call)
        ty, tx = seg_tables(h, a.hc, align_corners, dev), seg_tables(w, a.wc, align_corners, dev)
        a.y_i0, a.y_w1 = _table_ptrs(ty, h, a.hc)[:2]
        a.x_i0, a.x_w1 = _table_ptrs(tx, w, a.wc)[:2]
    check(lib.memhip_seg_predict(C.byref(a), stream_ptr()), "seg_predict")
    return pred


# ---------------------------------------------------------------- FCN decode head (csrc/seg_head.hip, seg_head_plan.cpp)
DROPOUT_SITE_HEAD = 0x48454144       # == MEMHIP_DROPOUT_SITE_HEAD: Dropout2d of decode head i is site DROPOUT_SITE_HEAD + i
BN_GROUPS = 128                      # == MEMHIP_BN_GROUPS


class BnHeadArgs(C.Structure):
    """== memhip_bnhead_args_t."""
    _fields_ = [(n, vp) for n in ("y", "mean", "rstd", "gamma", "beta", "wcls", "bias")] + [("dropout", C.POINTER(Dropout))] + \
               [(n, i32) for n in ("B", "C", "K", "h", "w", "reserved0")] + \
               [("logits", vp), ("ld", i64), ("dlogit", vp), ("db", i64), ("dk", i64), ("dy", i64), ("dx", i64),
                ("sums", vp), ("dwcls", vp), ("dbias", vp), ("workspace", vp), ("workspace_bytes", sz),
                ("tot", vp), ("inv_n", f32), ("reserved1", i32), ("dy_out", vp)]


class BnHeadPlan(C.Structure):
    """== memhip_bnhead_plan_t."""
    _fields_ = [("R", i64)] + \
               [(n, i32) for n in ("kp", "block", "fwd_grid", "fwd_lds_bytes", "sums_grid_x", "sums_grid_y", "sums_lds_bytes",
                                   "apply_grid_x", "apply_grid_y", "apply_lds_bytes", "slot_floats", "fold_grid")] + \
               [("ws_bytes", C.c_uint64)]


declare({
    "memhip_map_to_nhwc_pad": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    "memhip_nhwc_pad_to_map": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    "memhip_bn_stats_workspace": (sz, [i32]),
    "memhip_bn_stats_nhwc": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, sz, vp, vp]),
    "memhip_bnhead_fwd": (i32, [C.POINTER(BnHeadArgs), vp]),
    "memhip_bnhead_bwd_sums": (i32, [C.POINTER(BnHeadArgs), vp]),
    "memhip_bnhead_bwd_apply": (i32, [C.POINTER(BnHeadArgs), vp]),
    "memhip_bnhead_plan": (i32, [C.POINTER(BnHeadArgs), C.POINTER(BnHeadPlan)]),
})


def map_to_nhwc_pad(x, out):
    """x f32 [B, D, h, w] contiguous -> the interior of out bf16 [B, h+2, w+2, D] (round to nearest even; the ring is not
    written)."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
    B, D, h, w = x.shape
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (B, h + 2, w + 2, D)
    check(lib.memhip_map_to_nhwc_pad(ptr(x), B, D, h, w, ptr(out), stream_ptr()), "map_to_nhwc_pad")
    return out


def nhwc_pad_to_map(x_pad, out=None):
    """The inverse: the interior of x_pad bf16 [B, h+2, w+2, D] -> f32 [B, D, h, w] (exact)."""
    assert x_pad.dtype == torch.bfloat16 and x_pad.dim() == 4 and x_pad.is_contiguous()
    B, h, w, D = x_pad.shape[0], x_pad.shape[1] - 2, x_pad.shape[2] - 2, x_pad.shape[3]
    if out is None:
        out = torch.empty((B, D, h, w), dtype=torch.float32, device=x_pad.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, D, h, w)
    check(lib.memhip_nhwc_pad_to_map(ptr(x_pad), B, D, h, w, ptr(out), stream_ptr()), "nhwc_pad_to_map")
    return out


def bn_stats_workspace(C_, device):
    return torch.empty(int(lib.memhip_bn_stats_workspace(C_)) // 4, dtype=torch.float32, device=device)


def bn_stats_chain(R):
    """The longest chain of fp32 roundings behind one output of bn_stats_nhwc over R pixels (include/memhip.h)."""
    G = min(-(-R // 32), BN_GROUPS)
    return -(-R // (32 * G)) + 32 + G


def bn_stats_nhwc(x, B, h, w, C_, ws, shift=None, padded=True, out=None):
    """x bf16 padded [B, h+2, w+2, C] (interiors only) or dense [B h w, C] -> out f32 [3, C]: count, sum (x - shift),
    sum (x - shift)^2 per channel; shift f32 [C] or None (zero)."""
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    assert x.numel() >= (B * (h + 2) * (w + 2) * C_ if padded else B * h * w * C_)
    assert shift is None or (shift.dtype == torch.float32 and shift.numel() == C_ and shift.is_contiguous())
    out = _sums_out(out, 3, C_, x.device)
    check(lib.memhip_bn_stats_nhwc(ptr(x), int(padded), B, h, w, C_, ptr(shift), ptr(ws), ws.numel() * 4, ptr(out), stream_ptr()),
          "bn_stats_nhwc")
    return out


def bnhead_args(B, C_, K, h, w, dropout=None, **fields):
    """The memhip_bnhead_args_t of bnhead_fwd / _bwd_sums / _bwd_apply / bnhead_plan; pointer fields are addresses or None,
    dropout a Dropout struct or None."""
    a = BnHeadArgs(B=B, C=C_, K=K, h=h, w=w)
    if dropout is not None:
        a.dropout = C.pointer(dropout)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def bnhead_plan(B, C_, K, h, w, **fields):
    """The BnHeadPlan of the three calls at these shapes: grids, LDS bytes, workspace bytes.  Validates like the calls; no
    device."""
    plan = BnHeadPlan()
    check(lib.memhip_bnhead_plan(C.byref(bnhead_args(B, C_, K, h, w, **fields)), C.byref(plan)), "bnhead_plan")
    return plan


def _bnhead_common(y, B, C_, K, h, w, mean, rstd, gamma, beta, wcls, dropout):
    assert y.dtype == torch.bfloat16 and y.is_contiguous() and y.numel() >= B * (h + 2) * (w + 2) * C_
    assert all(v.dtype == torch.float32 and v.numel() == C_ and v.is_contiguous() for v in (mean, rstd, gamma, beta))
    assert wcls.dtype == torch.float32 and wcls.is_contiguous() and wcls.numel() == K * C_
    return bnhead_args(B, C_, K, h, w, dropout, y=y.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(), gamma=gamma.data_ptr(),
                       beta=beta.data_ptr(), wcls=wcls.data_ptr())


def _dlogit_fields(a, dlogit, B, K, h, w):
    assert dlogit.dtype == torch.float32 and tuple(dlogit.shape) == (B, K, h, w) and dlogit.is_cuda
    a.dlogit = dlogit.data_ptr()
    a.db, a.dk, a.dy, a.dx = dlogit.stride()


def bnhead_fwd(y, B, C_, K, h, w, mean, rstd, gamma, beta, wcls, bias, logits, dropout=None):
    """logits f32 [B h w, ld] = bias + relu(gamma (y - mean) rstd + beta) keep scale @ wcls^T over y bf16 [B, h+2, w+2, C]."""
    a = _bnhead_common(y, B, C_, K, h, w, mean, rstd, gamma, beta, wcls, dropout)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] >= B * h * w
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == K and bias.is_contiguous())
    a.bias, a.logits, a.ld = _p(bias), logits.data_ptr(), logits.stride(0)
    check(lib.memhip_bnhead_fwd(C.byref(a), stream_ptr()), "bnhead_fwd")
    return logits


def bnhead_bwd_sums(dlogit, y, B, C_, K, h, w, mean, rstd, gamma, beta, wcls, sums, dwcls, dbias, workspace, dropout=None):
    """sums f32 [2, C] = sum g, sum g xhat; dwcls f32 [K, C]; dbias f32 [K] from dlogit f32 [B, K, h, w] (any strides)."""
    a = _bnhead_common(y, B, C_, K, h, w, mean, rstd, gamma, beta, wcls, dropout)
    _dlogit_fields(a, dlogit, B, K, h, w)
    for v, n in ((sums, 2 * C_), (dwcls, K * C_), (dbias, K)):
        assert v.dtype == torch.float32 and v.is_contiguous() and v.numel() == n
    a.sums, a.dwcls, a.dbias = sums.data_ptr(), dwcls.data_ptr(), dbias.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    check(lib.memhip_bnhead_bwd_sums(C.byref(a), stream_ptr()), "bnhead_bwd_sums")


def bnhead_bwd_apply(dlogit, y, B, C_, K, h, w, mean, rstd, gamma, beta, wcls, tot, inv_n, dy_out, dropout=None):
    """The interior of dy_out bf16 [B, h+2, w+2, C] = gamma rstd (g - tot[0] inv_n - xhat tot[1] inv_n); tot None: eval
    statistics, no correction terms."""
    a = _bnhead_common(y, B, C_, K, h, w, mean, rstd, gamma, beta, wcls, dropout)
    _dlogit_fields(a, dlogit, B, K, h, w)
    assert dy_out.dtype == torch.bfloat16 and dy_out.is_contiguous() and dy_out.numel() >= B * (h + 2) * (w + 2) * C_
    assert tot is None or (tot.dtype == torch.float32 and tot.is_contiguous() and tot.numel() == 2 * C_)
    a.tot, a.inv_n, a.dy_out = _p(tot), float(inv_n), dy_out.data_ptr()
    check(lib.memhip_bnhead_bwd_apply(C.byref(a), stream_ptr()), "bnhead_bwd_apply")
    return dy_out


# ---------------------------------------------------------------- pyramid pooling of the PSP head (csrc/ppm.hip, ppm_plan.cpp)
PPM_MAX_SCALES = 4                   # == MEMHIP_PPM_MAX_SCALES
PPM_MAX_SCALE = 8                    # == MEMHIP_PPM_MAX_SCALE
_vp4, _i32x4 = vp * PPM_MAX_SCALES, i32 * PPM_MAX_SCALES


class PpmArgs(C.Structure):
    """== memhip_ppm_args_t."""
    _fields_ = [(n, i32) for n in ("B", "Cin", "C", "h", "w", "n")] + [("scales", _i32x4), ("map", vp), ("P", _vp4), ("Y", _vp4)] + \
               [(n, vp) for n in ("mean", "rstd", "gamma", "beta")] + \
               [(n, _vp4) for n in ("y_i0", "y_w1", "y_lo", "y_hi", "x_i0", "x_w1", "x_lo", "x_hi")] + \
               [("xcat", vp), ("dxcat", vp), ("g", _vp4), ("sums", vp), ("tot", vp), ("inv_n", f32 * PPM_MAX_SCALES),
                ("dY", _vp4), ("dP", _vp4), ("dmap", vp)]


class PpmPlan(C.Structure):
    """== memhip_ppm_plan_t."""
    _fields_ = [("R", i64), ("block", i32), ("ct", i32), ("bins", i32), ("rows", _i32x4), ("row_tile0", _i32x4)] + \
               [(n, i32) for n in ("pool_grid", "pool_lds_bytes", "concat_grid_x", "concat_grid_y", "gather_grid_x", "gather_grid_y",
                                   "sums_grid_x", "sums_grid_y", "dmap_grid_x", "dmap_grid_y", "tile_lds_bytes")] + \
               [("ws_bytes", C.c_uint64)]


declare({
    "memhip_ppm_bins": (i32, [i32, i32, vp, vp]),
    "memhip_ppm_plan": (i32, [C.POINTER(PpmArgs), C.POINTER(PpmPlan)]),
    "memhip_ppm_pool": (i32, [C.POINTER(PpmArgs), vp]),
    "memhip_ppm_concat_fwd": (i32, [C.POINTER(PpmArgs), vp]),
    "memhip_ppm_concat_bwd_sums": (i32, [C.POINTER(PpmArgs), vp]),
    "memhip_ppm_bwd_apply": (i32, [C.POINTER(PpmArgs), vp]),
    "memhip_ppm_dmap": (i32, [C.POINTER(PpmArgs), vp]),
})


def ppm_bins(n, s):
    """The adaptive-average-pooling bins of s over n pixels as host arrays (start i32 [s], end i32 [s]): bin i is
    [floor(i n / s), ceil((i + 1) n / s)), the kernels' own arithmetic.  No device needed."""
    import numpy as np
    start, end = np.empty(max(s, 0), np.int32), np.empty(max(s, 0), np.int32)
    check(lib.memhip_ppm_bins(n, s, start.ctypes.data, end.ctypes.data), "ppm_bins")
    return start, end


def ppm_args(B, Cin, C_, h, w, scales, **fields):
    """The memhip_ppm_args_t of the five ppm calls and ppm_plan.  Fields: a pointer field takes an address or None, a
    per-scale field a sequence of them (or of floats: inv_n)."""
    a = PpmArgs(B=B, Cin=Cin, C=C_, h=h, w=w, n=len(scales))
    if len(scales) <= PPM_MAX_SCALES:                      # (more: the plan refuses n)
        a.scales = _i32x4(*[int(s) for s in scales])
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            v = type(getattr(a, k))(*v)
        setattr(a, k, v)
    return a


def ppm_plan(B, Cin, C_, h, w, scales, **fields):
    """The PpmPlan of the five calls at these shapes: grids, LDS bytes.  Validates like the calls; no device."""
    plan = PpmPlan()
    check(lib.memhip_ppm_plan(C.byref(ppm_args(B, Cin, C_, h, w, scales, **fields)), C.byref(plan)), "ppm_plan")
    return plan


def _ppm_pads(bufs, B, scales, ch):
    for t, s in zip(bufs, scales):
        assert t.dtype == torch.bfloat16 and t.is_contiguous() and t.is_cuda and tuple(t.shape) == (B, s + 2, s + 2, ch), (tuple(t.shape), s, ch)
    return [t.data_ptr() for t in bufs]


def _ppm_vectors(a, vecs, n, C_):
    for name, v in zip(("mean", "rstd", "gamma", "beta"), vecs):
        assert v.dtype == torch.float32 and v.is_contiguous() and v.is_cuda and tuple(v.shape) == (n, C_), name
        setattr(a, name, v.data_ptr())


def _ppm_tables(a, scales, h, w, align_corners, device):
    """the axis tables of every scale, (s -> h) and (s -> w), as seg_tables keeps them"""
    keep = []
    for name, n_out in (("y", h), ("x", w)):
        ptrs = []
        for s in scales:
            t = seg_tables(s, n_out, align_corners, device)
            keep.append(t)
            ptrs.append(_table_ptrs(t, s, n_out))
        for j, f in enumerate(("i0", "w1", "lo", "hi")):
            setattr(a, name + "_" + f, _vp4(*[p[j] for p in ptrs]))
    return keep


def ppm_pool(x, scales, P):
    """x f32 [B, Cin, h, w] contiguous -> the interiors of P[i] bf16 [B, s+2, s+2, Cin], every scale in one launch: the mean
    over the bin (fp32 sum in row-major order / the count), rounded to bf16."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.is_cuda
    B, Cin, h, w = x.shape
    a = ppm_args(B, Cin, 64, h, w, scales, map=x.data_ptr(), P=_ppm_pads(P, B, scales, Cin))
    check(lib.memhip_ppm_pool(C.byref(a), stream_ptr()), "ppm_pool")
    return P


def ppm_concat_fwd(x, scales, Y, mean, rstd, gamma, beta, xcat, align_corners=False):
    """The interior of xcat bf16 [B, h+2, w+2, Cin + n C]: channels < Cin the map (the bits of map_to_nhwc_pad), channel
    Cin + i C + c the bilinear resize of relu(gamma (Y[i] - mean) rstd + beta); vectors f32 [n, C]."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.is_cuda
    B, Cin, h, w = x.shape
    n, C_ = len(scales), Y[0].shape[-1]
    assert xcat.dtype == torch.bfloat16 and xcat.is_contiguous() and tuple(xcat.shape) == (B, h + 2, w + 2, Cin + n * C_)
    a = ppm_args(B, Cin, C_, h, w, scales, map=x.data_ptr(), Y=_ppm_pads(Y, B, scales, C_), xcat=xcat.data_ptr())
    _ppm_vectors(a, (mean, rstd, gamma, beta), n, C_)
    keep = _ppm_tables(a, scales, h, w, align_corners, x.device)
    check(lib.memhip_ppm_concat_fwd(C.byref(a), stream_ptr()), "ppm_concat_fwd")
    del keep
    return xcat


def ppm_concat_bwd_sums(dxcat, Cin, scales, Y, mean, rstd, gamma, beta, g, sums, align_corners=False):
    """From dxcat bf16 [B, h+2, w+2, Cin + n C] (channels >= Cin): g[i] f32 [B s^2, C] = the transposed resize, gated by
    u > 0; sums f32 [n, 2, C] = sum g, sum g xhat."""
    B, h, w = dxcat.shape[0], dxcat.shape[1] - 2, dxcat.shape[2] - 2
    n, C_ = len(scales), Y[0].shape[-1]
    assert dxcat.dtype == torch.bfloat16 and dxcat.is_contiguous() and dxcat.is_cuda and dxcat.shape[3] == Cin + n * C_
    for t, s in zip(g, scales):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B * s * s, C_)
    assert sums.dtype == torch.float32 and sums.is_contiguous() and tuple(sums.shape) == (n, 2, C_)
    a = ppm_args(B, Cin, C_, h, w, scales, dxcat=dxcat.data_ptr(), Y=_ppm_pads(Y, B, scales, C_), g=[t.data_ptr() for t in g],
                 sums=sums.data_ptr())
    _ppm_vectors(a, (mean, rstd, gamma, beta), n, C_)
    keep = _ppm_tables(a, scales, h, w, align_corners, dxcat.device)
    check(lib.memhip_ppm_concat_bwd_sums(C.byref(a), stream_ptr()), "ppm_concat_bwd_sums")
    del keep
    return g, sums


def ppm_bwd_apply(g, scales, Y, mean, rstd, gamma, beta, tot, inv_n, dY, hw):
    """The interiors of dY[i] bf16 [B, s+2, s+2, C] = gamma rstd (g - tot[i, 0] inv_n[i] - xhat tot[i, 1] inv_n[i]); tot f32
    [n, 2, C] or None: eval statistics, no correction terms; inv_n: a float per scale; hw = (h, w) of the map."""
    n, C_ = len(scales), Y[0].shape[-1]
    B = Y[0].shape[0]
    for t, s in zip(g, scales):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B * s * s, C_)
    assert tot is None or (tot.dtype == torch.float32 and tot.is_contiguous() and tuple(tot.shape) == (n, 2, C_))
    a = ppm_args(B, 64, C_, hw[0], hw[1], scales, Y=_ppm_pads(Y, B, scales, C_), g=[t.data_ptr() for t in g], tot=_p(tot),
                 inv_n=[float(v) for v in inv_n], dY=_ppm_pads(dY, B, scales, C_))
    _ppm_vectors(a, (mean, rstd, gamma, beta), n, C_)
    check(lib.memhip_ppm_bwd_apply(C.byref(a), stream_ptr()), "ppm_bwd_apply")
    return dY


def ppm_dmap(dxcat, Cin, scales, dP, out):
    """out f32 [B, Cin, h, w] = dxcat[.., :Cin] + the transposed pooling of dP[i] bf16 [B, s+2, s+2, Cin] (each bin's value
    / its pixel count to every pixel of the bin), added in the order scale, bin row, bin column."""
    B, h, w = dxcat.shape[0], dxcat.shape[1] - 2, dxcat.shape[2] - 2
    assert dxcat.dtype == torch.bfloat16 and dxcat.is_contiguous() and dxcat.is_cuda and dxcat.shape[3] >= Cin
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, Cin, h, w)
    C_ = (dxcat.shape[3] - Cin) // len(scales)
    assert C_ * len(scales) == dxcat.shape[3] - Cin
    a = ppm_args(B, Cin, C_, h, w, scales, dxcat=dxcat.data_ptr(), dP=_ppm_pads(dP, B, scales, Cin), dmap=out.data_ptr())
    check(lib.memhip_ppm_dmap(C.byref(a), stream_ptr()), "ppm_dmap")
    return out


# ---------------------------------------------------------------- the FPN part of the UPerNet head (csrc/fpn.hip, fpn_plan.cpp)
FPN_MAX_LEVELS = 4                   # == MEMHIP_FPN_MAX_LEVELS
_FPN_TABLES = [ax + "_" + f for ax in ("cy", "cx", "ty", "tx") for f in ("i0", "w1", "lo", "hi")]


class FpnArgs(C.Structure):
    """== memhip_fpn_args_t."""
    _fields_ = [(n, i32) for n in ("B", "C", "L", "level")] + [("h", _i32x4), ("w", _i32x4), ("Y", _vp4)] + \
               [(n, vp) for n in ("mean", "rstd", "gamma", "beta")] + [(n, _vp4) for n in _FPN_TABLES] + \
               [(n, vp) for n in ("src", "T", "xcat", "own", "dxcat", "fine_rows")] + [("slice", i32), ("reserved0", i32)] + \
               [("rows", vp), ("sums", vp), ("workspace", vp), ("workspace_bytes", sz), ("tot", vp), ("inv_n", f32),
                ("reserved1", i32), ("dY", vp)]


class FpnPlan(C.Structure):
    """== memhip_fpn_plan_t."""
    _fields_ = [("R", i64 * FPN_MAX_LEVELS)] + [(n, i32) for n in ("block", "ct", "grid_y", "concat_grid_x", "concat_grid_y")] + \
               [(n, _i32x4) for n in ("topdown_grid_x", "resize_grid_x", "sums_grid_x", "apply_grid_x")] + \
               [(n, i32) for n in ("sums_lds_bytes", "slot_floats", "fold_grid")] + [("ws_bytes", C.c_uint64)]


declare({
    "memhip_fpn_plan": (i32, [C.POINTER(FpnArgs), C.POINTER(FpnPlan)]),
    "memhip_fpn_topdown_fwd": (i32, [C.POINTER(FpnArgs), vp]),
    "memhip_fpn_concat_fwd": (i32, [C.POINTER(FpnArgs), vp]),
    "memhip_fpn_resize_bwd": (i32, [C.POINTER(FpnArgs), vp]),
    "memhip_fpn_bn_bwd_sums": (i32, [C.POINTER(FpnArgs), vp]),
    "memhip_fpn_bn_bwd_apply": (i32, [C.POINTER(FpnArgs), vp]),
})


def fpn_args(B, C_, sizes, level=0, **fields):
    """The memhip_fpn_args_t of the five fpn calls and fpn_plan; sizes = [(h_l, w_l)], finest first.  Fields: a pointer field
    takes an address or None, a per-level field a sequence of them."""
    a = FpnArgs(B=B, C=C_, L=len(sizes), level=level)
    if len(sizes) <= FPN_MAX_LEVELS:                       # (more: the plan refuses L)
        a.h, a.w = _i32x4(*[int(s[0]) for s in sizes]), _i32x4(*[int(s[1]) for s in sizes])
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            v = type(getattr(a, k))(*v)
        setattr(a, k, v)
    return a


def fpn_plan(B, C_, sizes, level=0, **fields):
    """The FpnPlan of the five calls at these shapes, every level: grids, workspace bytes.  Validates like the calls; no device."""
    plan = FpnPlan()
    check(lib.memhip_fpn_plan(C.byref(fpn_args(B, C_, sizes, level, **fields)), C.byref(plan)), "fpn_plan")
    return plan


def fpn_sums_workspace(C_, device):
    """the workspace of fpn_bn_bwd_sums: BN_GROUPS partials of [2, C], whatever the level"""
    return torch.empty(BN_GROUPS * 2 * C_, dtype=torch.float32, device=device)


def _fpn_pad(t, B, hw, ch, name):
    assert t.dtype == torch.bfloat16 and t.is_contiguous() and t.is_cuda and tuple(t.shape) == (B, hw[0] + 2, hw[1] + 2, ch), \
        (name, tuple(t.shape), B, hw, ch)
    return t.data_ptr()


def _fpn_vectors(a, vecs, L, C_):
    for name, v in zip(("mean", "rstd", "gamma", "beta"), vecs):
        assert v.dtype == torch.float32 and v.is_contiguous() and v.is_cuda and tuple(v.shape) == (L, C_), name
        setattr(a, name, v.data_ptr())


def _fpn_tables(a, family, sizes, levels, align_corners, device):
    """family "c": the tables (level l -> level 0) at index l; "t": (level l + 1 -> level l) at index l, as seg_tables keeps
    them; only the indices in ``levels`` are set"""
    keep = []
    for j, ax in enumerate("yx"):
        ptrs = [(None,) * 4] * FPN_MAX_LEVELS
        for l in levels:
            n_in, n_out = (sizes[l][j], sizes[0][j]) if family == "c" else (sizes[l + 1][j], sizes[l][j])
            t = seg_tables(n_in, n_out, align_corners, device)
            keep.append(t)
            ptrs[l] = _table_ptrs(t, n_in, n_out)
        for k, f in enumerate(("i0", "w1", "lo", "hi")):
            setattr(a, "%s%s_%s" % (family, ax, f), _vp4(*[p[k] for p in ptrs]))
    return keep


def _fpn_rows(t, n, C_, name):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda and tuple(t.shape) == (n, C_), (name, tuple(t.shape), n, C_)
    return t.data_ptr()


def fpn_topdown_fwd(level, sizes, Y, vecs, src, T, align_corners=False):
    """The interior of T bf16 [B, h_l+2, w_l+2, C] = bf16(relu(bn(Y)) + bilinear(level + 1 -> level)(src)); Y the lateral's
    stored output of ``level``; src the stored T of level + 1, or (level == L - 2) a tuple ``(Ysrc,)``: the stored output whose
    relu(bn(.)) with row level + 1 of the vectors is the source.  vecs = (mean, rstd, gamma, beta) f32 [L, C]."""
    B, C_, L = Y.shape[0], Y.shape[-1], len(sizes)
    a = fpn_args(B, C_, sizes, level, T=_fpn_pad(T, B, sizes[level], C_, "T"))
    ys = [None] * FPN_MAX_LEVELS
    ys[level] = _fpn_pad(Y, B, sizes[level], C_, "Y")
    if isinstance(src, tuple):
        ys[level + 1] = _fpn_pad(src[0], B, sizes[level + 1], C_, "Ysrc")
    else:
        a.src = _fpn_pad(src, B, sizes[level + 1], C_, "src")
    a.Y = _vp4(*ys)
    _fpn_vectors(a, vecs, L, C_)
    keep = _fpn_tables(a, "t", sizes, [level], align_corners, Y.device)
    check(lib.memhip_fpn_topdown_fwd(C.byref(a), stream_ptr()), "fpn_topdown_fwd")
    del keep
    return T


def fpn_concat_fwd(sizes, Y, vecs, xcat, align_corners=False):
    """The interior of xcat bf16 [B, h_0+2, w_0+2, L C]: channel l C + c = bf16(bilinear(level l -> level 0)(relu(bn_l(Y[l]))))."""
    B, C_, L = Y[0].shape[0], Y[0].shape[-1], len(sizes)
    a = fpn_args(B, C_, sizes, 0, xcat=_fpn_pad(xcat, B, sizes[0], L * C_, "xcat"),
                 Y=[_fpn_pad(y, B, s, C_, "Y") for y, s in zip(Y, sizes)])
    _fpn_vectors(a, vecs, L, C_)
    keep = _fpn_tables(a, "c", sizes, range(L), align_corners, xcat.device)
    check(lib.memhip_fpn_concat_fwd(C.byref(a), stream_ptr()), "fpn_concat_fwd")
    del keep
    return xcat


def fpn_resize_bwd(level, sizes, C_, rows, own=None, dxcat=None, slice_=0, fine_rows=None, align_corners=False):
    """rows f32 [B h_d w_d, C] (d = level) = own (bf16 padded, the destination's size) + the transposed resize of channel slice
    ``slice_`` of dxcat bf16 [B, h_0+2, w_0+2, L C] + the transposed resize of fine_rows f32 [B h_{d-1} w_{d-1}, C], in that
    order; each term optional.  Ungated."""
    L, (h, w) = len(sizes), sizes[level]
    B = rows.shape[0] // (h * w)
    a = fpn_args(B, C_, sizes, level, rows=_fpn_rows(rows, B * h * w, C_, "rows"), slice=slice_)
    keep = []
    if own is not None:
        a.own = _fpn_pad(own, B, sizes[level], C_, "own")
    if dxcat is not None:
        a.dxcat = _fpn_pad(dxcat, B, sizes[0], L * C_, "dxcat")
        keep += _fpn_tables(a, "c", sizes, [level], align_corners, rows.device)
    if fine_rows is not None:
        a.fine_rows = _fpn_rows(fine_rows, B * sizes[level - 1][0] * sizes[level - 1][1], C_, "fine_rows")
        keep += _fpn_tables(a, "t", sizes, [level - 1], align_corners, rows.device)
    check(lib.memhip_fpn_resize_bwd(C.byref(a), stream_ptr()), "fpn_resize_bwd")
    del keep
    return rows


def _fpn_bn_common(level, sizes, Y, vecs, rows):
    B, C_, L, (h, w) = Y.shape[0], Y.shape[-1], len(sizes), sizes[level]
    ys = [None] * FPN_MAX_LEVELS
    ys[level] = _fpn_pad(Y, B, sizes[level], C_, "Y")
    a = fpn_args(B, C_, sizes, level, Y=ys, rows=_fpn_rows(rows, B * h * w, C_, "rows"))
    _fpn_vectors(a, vecs, L, C_)
    return a, C_


def fpn_bn_bwd_sums(level, sizes, Y, vecs, rows, sums, workspace):
    """sums f32 [2, C] = sum g, sum g xhat over the level's pixels, g = rows (u > 0), u and xhat from Y and row ``level`` of
    the vectors; workspace: fpn_sums_workspace."""
    a, C_ = _fpn_bn_common(level, sizes, Y, vecs, rows)
    assert sums.dtype == torch.float32 and sums.is_contiguous() and sums.is_cuda and tuple(sums.shape) == (2, C_)
    assert workspace.is_cuda and workspace.is_contiguous()
    a.sums, a.workspace, a.workspace_bytes = sums.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size()
    check(lib.memhip_fpn_bn_bwd_sums(C.byref(a), stream_ptr()), "fpn_bn_bwd_sums")
    return sums


def fpn_bn_bwd_apply(level, sizes, Y, vecs, rows, tot, inv_n, dY):
    """The interior of dY bf16 [B, h_l+2, w_l+2, C] = gamma rstd (g - tot[0] inv_n - xhat tot[1] inv_n); tot f32 [2, C] or
    None: eval statistics, no correction terms."""
    a, C_ = _fpn_bn_common(level, sizes, Y, vecs, rows)
    assert tot is None or (tot.dtype == torch.float32 and tot.is_contiguous() and tot.is_cuda and tuple(tot.shape) == (2, C_))
    a.tot, a.inv_n, a.dY = _p(tot), float(inv_n), _fpn_pad(dY, Y.shape[0], sizes[level], C_, "dY")
    check(lib.memhip_fpn_bn_bwd_apply(C.byref(a), stream_ptr()), "fpn_bn_bwd_apply")
    return dY


# ---------------------------------------------------------------- segmentation data chain (csrc/seg_data.hip)
class SegDataArgs(C.Structure):
    """== memhip_segdata_args_t."""
    _fields_ = [(n, i32) for n in ("B", "H", "W", "max_h", "max_w", "crop_h", "crop_w", "net_h", "net_w", "out_f32", "in_f32",
                                   "reserved0")] + \
               [("num_stds", f64), ("planes", vp), ("offs", vp), ("dims", vp), ("img_u8", vp), ("img_f32", vp), ("img_elems", i64),
                ("hist", vp), ("crop", vp), ("out", vp), ("labels", vp), ("label_out", vp)]


declare({
    "memhip_segdata_resize_hist": (i32, [C.POINTER(SegDataArgs), vp]),
    "memhip_segdata_norm": (i32, [C.POINTER(SegDataArgs), vp]),
    "memhip_segdata_geom": (i32, [C.POINTER(SegDataArgs), vp]),
})


def _segdata_common(offs, dims, max_hw, **fields):
    B = dims.shape[0]
    assert dims.is_cuda and dims.dtype == torch.int32 and dims.is_contiguous() and tuple(dims.shape) == (B, 2), "dims: CUDA i32 [B, 2]"
    assert offs.is_cuda and offs.dtype == torch.int64 and offs.is_contiguous() and tuple(offs.shape) == (B,), "offs: CUDA i64 [B]"
    a = SegDataArgs(B=B, max_h=int(max_hw[0]), max_w=int(max_hw[1]), offs=offs.data_ptr(), dims=dims.data_ptr())
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _segdata_buf(t, dtype, name):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.dim() == 1, f"{name}: a flat contiguous CUDA {dtype} tensor"
    return t.data_ptr()


def segdata_resize_hist(planes, offs, dims, max_hw, img_u8, hist):
    """planes u8 [B, 3, H, W] -> the exact-integer bilinear resize of sample b to dims[b] = (h_b, w_b) (<= max_hw), stored
    densely as [3, h_b, w_b] at byte offs[b] of the flat u8 buffer img_u8; hist u32 [B, 2, 256] <- H_val (values of channels
    0 and 2 of the resized image), H_pmax (max(ch0, ch2) per pixel)."""
    B, _, H, W = planes.shape
    assert planes.is_cuda and planes.dtype == torch.uint8 and planes.is_contiguous() and planes.shape[1] == 3
    assert hist.is_cuda and hist.dtype == torch.int32 and hist.is_contiguous() and tuple(hist.shape) == (B, 2, 256), \
        "hist: CUDA i32 [B, 2, 256] (the u32 counts)"
    a = _segdata_common(offs, dims, max_hw, H=H, W=W, planes=planes.data_ptr(), img_u8=_segdata_buf(img_u8, torch.uint8, "img_u8"),
                        img_elems=img_u8.numel(), hist=hist.data_ptr())
    check(lib.memhip_segdata_resize_hist(C.byref(a), stream_ptr()), "segdata_resize_hist")


def segdata_norm(offs, dims, max_hw, img_u8, hist, num_stds=10.0, img_f32=None):
    """Hot-pixel removal and (v / m) * 255 from the histograms of segdata_resize_hist: in place in img_u8 (truncated), or with
    img_f32 (a flat f32 buffer of as many elements) unrounded to img_f32 at the same element offsets."""
    B = dims.shape[0]
    assert hist.is_cuda and hist.dtype == torch.int32 and hist.is_contiguous() and tuple(hist.shape) == (B, 2, 256)
    a = _segdata_common(offs, dims, max_hw, img_u8=_segdata_buf(img_u8, torch.uint8, "img_u8"), img_elems=img_u8.numel(),
                        hist=hist.data_ptr(), num_stds=float(num_stds))
    if img_f32 is not None:
        assert img_f32.numel() >= img_u8.numel()
        a.img_f32, a.out_f32 = _segdata_buf(img_f32, torch.float32, "img_f32"), 1
    check(lib.memhip_segdata_norm(C.byref(a), stream_ptr()), "segdata_norm")


def segdata_geom(offs, dims, max_hw, img, crop, crop_size, net_size=None, out=None, labels=None, label_out=None):
    """crop i32 [B, 3] = {top, left, flip}.  Image: img (flat u8 or f32 buffer, samples at offs / dims) -> out f32
    [B, 3, net_h, net_w]: crop, flip, channel swap, zero pad to crop_size, bilinear resize to net_size.  Labels: labels u8
    [B, H, W] -> label_out u8 [B, crop_h, crop_w]: nearest resize to dims[b], the same crop and flip, pad 255."""
    B = dims.shape[0]
    assert crop.is_cuda and crop.dtype == torch.int32 and crop.is_contiguous() and tuple(crop.shape) == (B, 3), "crop: CUDA i32 [B, 3]"
    a = _segdata_common(offs, dims, max_hw, crop=crop.data_ptr(), crop_h=int(crop_size[0]), crop_w=int(crop_size[1]))
    if out is not None:
        assert img.dtype in (torch.uint8, torch.float32)
        a.in_f32 = int(img.dtype == torch.float32)
        p = _segdata_buf(img, img.dtype, "img")
        if a.in_f32:
            a.img_f32 = p
        else:
            a.img_u8 = p
        a.img_elems = img.numel()
        a.net_h, a.net_w = int(net_size[0]), int(net_size[1])
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, 3, a.net_h, a.net_w)
        a.out = out.data_ptr()
    else:
        a.img_elems = int(img.numel()) if img is not None else (1 << 62)     # labels only: offs are not dereferenced
    if label_out is not None:
        assert labels.is_cuda and labels.dtype == torch.uint8 and labels.is_contiguous() and labels.dim() == 3 and labels.shape[0] == B
        assert label_out.is_cuda and label_out.dtype == torch.uint8 and label_out.is_contiguous() \
            and tuple(label_out.shape) == (B, a.crop_h, a.crop_w)
        a.H, a.W = int(labels.shape[1]), int(labels.shape[2])
        a.labels, a.label_out = labels.data_ptr(), label_out.data_ptr()
    check(lib.memhip_segdata_geom(C.byref(a), stream_ptr()), "segdata_geom")
