"""The feature-pyramid necks of the segmentation backbone on the fused HIP path (``EvBEiT(necks="fused")``): fpn1 =
ConvTranspose2d(2, 2) -> SyncBatchNorm -> GELU -> ConvTranspose2d(2, 2) and fpn2 = ConvTranspose2d(2, 2)
(mem/semantic_segmentation/backbone/mem.py:331-346), forward and backward, on the parameters and buffers of the torch
modules (the state dict is theirs in both modes).

A ConvTranspose2d with kernel = stride = 2 has no overlap: ``out[b, co, 2y+i, 2x+j] = bias[co] + sum_ci in[b, ci, y, x] *
W[ci, co, i, j]``.  With pixel rows ``X [R, D]`` (row = (b, y, x)) and the weight read as the ``[D, 4D]`` matrix it is in
memory (``weight_matrix``: column 4 co + q, q = 2i + j) that is ``Y = X W``, one NT GEMM on the transposed bf16 copy of W.
The column order is kept everywhere: the dgrad product ``dX = dY W^T`` takes the bf16 shadow ``W16 [D, 4D]`` as it lies,
the weight gradient ``X^T dY`` lands in ``W.grad``'s own layout, the bias operand is ``bias.repeat_interleave(4)`` and the
bias gradient the column sums of dY folded by 4.  A row of Y holds the four output pixels of one input pixel per channel
("interleaved"); as plain rows the same values are ``Z [4R, D]``, ``Z[4r + q, co] = Y[r, 4 co + q]``.  Two levels nest:
row ``4 r0 + (2 ia + ja)``, column ``(co, 2 ib + jb)`` is the pixel ``(4y + 2 ia + ib, 4x + 2 ja + jb)``.  The torch
expressions of these orders (``map_to_rows`` / ``rows_to_map``) specify the kernels of csrc/necks.hip, which move the
data: nothing de-interleaves in a pass of its own.

Precision: the placement torch's bf16 autocast would use.  GEMM operands bf16 with fp32 accumulation, every transposed
convolution's output rounded to bf16 once, batch statistics and normalise -> affine -> GELU in fp32 rounded to bf16 once, the
returned maps fp32.
"""
import torch

from . import ops
from .syncbn import BufferCache, add_affine_grads, all_reduce_sum, backward_totals, batch_vectors

# ---------------------------------------------------------------------------------------------- packing (pure torch)
def weight_matrix(weight):
    """ConvTranspose2d weight [D_in, D_out, 2, 2] as the [D_in, 4 D_out] matrix it is in memory: column 4 co + 2i + j."""
    assert weight.dim() == 4 and tuple(weight.shape[2:]) == (2, 2), tuple(weight.shape)
    return weight.reshape(weight.shape[0], 4 * weight.shape[1])


def bias_operand(bias):
    """The bias of the [R, 4D] product: bias[co] at the columns 4 co .. 4 co + 3."""
    return bias.repeat_interleave(4)


def fold4(v):
    """Column sums of an interleaved [.., 4D] matrix -> per channel [D] (the bias gradient of the transposed convolution)."""
    return v.reshape(-1, 4).sum(1)


def map_to_rows(x, level):
    """x [B, D, 2^level Hp, 2^level Wp] -> level 0: the pixel rows [B Hp Wp, D]; level 1 / 2: the interleaved rows
    [B Hp Wp 4^(level-1), 4D] of a map upsampled ``level`` times, in the nested order of the module docstring."""
    B, D, H, W = x.shape
    if level == 0:
        return x.flatten(2).transpose(1, 2).reshape(B * H * W, D)
    if level == 1:                                   # (b, co, y, i, x, j) -> (b, y, x | co, i, j)
        return x.reshape(B, D, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // 2) * (W // 2), 4 * D)
    assert level == 2, level                         # (b, co, y, ia, ib, x, ja, jb) -> (b, y, x, ia, ja | co, ib, jb)
    return x.reshape(B, D, H // 4, 2, 2, W // 4, 2, 2).permute(0, 2, 5, 3, 6, 1, 4, 7).reshape(B * (H // 4) * (W // 4) * 4, 4 * D)


def rows_to_map(rows, B, D, Hp, Wp, level):
    """The inverse of map_to_rows: -> [B, D, 2^level Hp, 2^level Wp]."""
    if level == 0:
        return rows.reshape(B, Hp * Wp, D).transpose(1, 2).reshape(B, D, Hp, Wp)
    if level == 1:
        return rows.reshape(B, Hp, Wp, D, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, D, 2 * Hp, 2 * Wp)
    assert level == 2, level
    return rows.reshape(B, Hp, Wp, 2, 2, D, 2, 2).permute(0, 5, 1, 3, 6, 2, 4, 7).reshape(B, D, 4 * Hp, 4 * Wp)


# ---------------------------------------------------------------------------------------------- autograd entry points
class _Fpn2Function(torch.autograd.Function):
    """fpn2: the engine's fp32 map [B, D, Hp, Wp] -> fp32 [B, D, 2Hp, 2Wp].  The parameters are inputs so that a call
    under a frozen trunk still records; their gradients are accumulated into ``p.grad`` by the backward itself."""

    @staticmethod
    def forward(ctx, necks, x, weight, bias):
        ctx.necks = necks
        out, ctx.saved = necks._fpn2_forward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        return None, ctx.necks._fpn2_backward(ctx.saved, dout, ctx.needs_input_grad[1]), None, None


class _Fpn1Function(torch.autograd.Function):
    """fpn1: the engine's fp32 map [B, D, Hp, Wp] -> fp32 [B, D, 4Hp, 4Wp]."""

    @staticmethod
    def forward(ctx, necks, x, w0, b0, gamma, beta, w3, b3):
        ctx.necks = necks
        out, ctx.saved = necks._fpn1_forward(x, keep=True)
        return out

    @staticmethod
    def backward(ctx, dout):
        return (None, ctx.necks._fpn1_backward(ctx.saved, dout, ctx.needs_input_grad[1])) + (None,) * 6


class FusedNecks(BufferCache):
    """fpn1 and fpn2 of an EvBEiT on the HIP path.  Holds no parameter of its own: it reads the torch modules' parameters
    and buffers (``fpn1.0`` ConvTranspose2d, ``fpn1.1`` SyncBatchNorm, ``fpn1.3`` ConvTranspose2d, ``fpn2.0``
    ConvTranspose2d) and, when the model has an engine, the engine's bf16 shadow ``flat_w16`` of the weights.

    Everything runs on the current stream.  Buffers are allocated per shape and reused: an output (and what a backward
    needs) is valid until this object's next call of the same neck with that shape, like the engine's maps."""

    def __init__(self, fpn1, fpn2, engine=None, prefix=("fpn1.", "fpn2.")):
        self.fpn1, self.fpn2 = fpn1, fpn2
        self.engine = engine                 # callable -> the model's ViTEngine, or None: own bf16 copies
        self.prefix = prefix
        self.reduce = all_reduce_sum
        self._bufs = {}
        self._w = None
        self._stamp = None
        self._tn_ws = None

    # ------------------------------------------------------------------ buffers and weights
    def _buf_device(self):
        return self.fpn2[0].weight.device

    def _convs(self):
        return ((self.prefix[0] + "0", self.fpn1[0]), (self.prefix[0] + "3", self.fpn1[3]), (self.prefix[1] + "0", self.fpn2[0]))

    def _weights_stamp(self, eng):
        if eng is not None:
            return ("engine", eng.w16_version)
        return tuple((p._version, p.data_ptr()) for _, c in self._convs() for p in (c.weight, c.bias))

    def _weights(self):
        """Per transposed convolution: w16 [D, 4D] (the dgrad operand), wT16 [4D, D] (the forward operand), bias4 [4D].
        Refreshed when the weights have changed -- with an engine that is where it refreshes its own bf16 copies, once per
        optimizer step (ViTEngine.w16_version) -- never per forward."""
        eng = self.engine() if self.engine is not None else None
        stamp = self._weights_stamp(eng)
        if self._w is not None and stamp == self._stamp:
            return self._w
        w = {}
        for name, conv in self._convs():
            D = conv.weight.shape[0]
            assert tuple(conv.weight.shape) == (D, D, 2, 2) and conv.weight.is_contiguous(), name
            master = weight_matrix(conv.weight.detach())
            old = self._w[name] if self._w is not None else None
            if eng is not None:
                w16 = eng.W16(name + ".weight", D, 4 * D)
            else:
                w16 = old[0] if old is not None else torch.empty((D, 4 * D), dtype=torch.bfloat16, device=master.device)
                ops.cast_f32_bf16(master, w16, master.numel())
            wT16 = old[1] if old is not None else torch.empty((4 * D, D), dtype=torch.bfloat16, device=master.device)
            ops.transpose_cast(master, D, 4 * D, wT16)
            w[name] = (w16, wT16, bias_operand(conv.bias.detach()).contiguous())
        self._w, self._stamp = w, stamp
        return w

    def refresh(self):
        """Drop the bf16 weight copies (a caller that changed the weights behind torch's version counters)."""
        self._stamp = None

    def _wgrad(self, conv, X, dY, R, D):
        """Accumulate the gradients of a transposed convolution from its input rows X [R, D] and dY [R, 4D]."""
        if conv.weight.requires_grad:
            need = ops.gemm_tn_workspace(R, D, 4 * D)
            if need and (self._tn_ws is None or self._tn_ws.numel() < need):
                self._tn_ws = torch.empty(need, dtype=torch.uint8, device=X.device)
            ops.gemm_tn(X, dY, R, D, 4 * D, weight_matrix(self._grad(conv.weight)), accumulate=True,
                        workspace=self._tn_ws if need else None)
        if conv.bias.requires_grad:
            cs = self._buf("colsum", (4 * D,), torch.float32)
            ops.zero_(cs)
            ops.colsum_bf16(dY, R, 4 * D, cs)
            self._grad(conv.bias).add_(fold4(cs))

    def _attach(self):
        if self.engine is not None:
            self.engine().attach_grads()         # p.grad = the views of the flat gradient buffer (zero_grad may have dropped them)

    @staticmethod
    def _check_map(x):
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4, "the necks take the engine's fp32 map [B, D, Hp, Wp]"
        return x.contiguous()

    # ------------------------------------------------------------------ fpn2
    def _fpn2_forward(self, x):
        B, D, Hp, Wp = x.shape
        R = B * Hp * Wp
        w16, wT16, bias4 = self._weights()[self.prefix[1] + "0"]
        X0 = ops.neck_maps_to_rows(x, 0, out=self._buf("f2.x0", (R, D)))
        Y = self._buf("f2.y", (R, 4 * D))
        ops.gemm_nt(X0, wT16, R, 4 * D, D, ops.EPI_BIAS_BF16, out0=Y, bias=bias4)
        out = ops.neck_rows_to_maps(Y, B, D, Hp, Wp, 1, out=self._buf("f2.out", (B, D, 2 * Hp, 2 * Wp), torch.float32))
        return out.detach(), (X0, (B, D, Hp, Wp))       # a fresh tensor on the buffer: autograd marks what a Function returns

    def _fpn2_backward(self, saved, dout, need_dx):
        X0, (B, D, Hp, Wp) = saved
        R = B * Hp * Wp
        self._attach()
        conv = self.fpn2[0]
        dY = ops.neck_maps_to_rows(dout.float().contiguous(), 1, out=self._buf("f2.dy", (R, 4 * D)))
        self._wgrad(conv, X0, dY, R, D)
        if not need_dx:
            return None
        dX = self._buf("f2.dx", (R, D))
        ops.gemm_nt(dY, self._weights()[self.prefix[1] + "0"][0], R, D, 4 * D, ops.EPI_BIAS_BF16, out0=dX)
        return ops.neck_rows_to_maps(dX, B, D, Hp, Wp, 0, out=self._buf("f2.dmap", (B, D, Hp, Wp), torch.float32)).detach()

    def fpn2_apply(self, x):
        x = self._check_map(x)
        conv = self.fpn2[0]
        if torch.is_grad_enabled() and self.fpn2.training and (x.requires_grad or conv.weight.requires_grad or conv.bias.requires_grad):
            return _Fpn2Function.apply(self, x, conv.weight, conv.bias)
        return self._fpn2_forward(x.detach())[0]

    # ------------------------------------------------------------------ fpn1
    def _colstats(self, Y1, D, bias):
        ws = self._buf("sums.ws", (ops.NECK_GROUPS * 2 * D,), torch.float32)
        return ops.neck_colstats(Y1, bias, ws, out=self._buf("stats", (3, D), torch.float32))

    def _fpn1_forward(self, x, keep):
        B, D, Hp, Wp = x.shape
        R = B * Hp * Wp
        w = self._weights()
        c0, bn, c3 = self.fpn1[0], self.fpn1[1], self.fpn1[3]
        X0 = ops.neck_maps_to_rows(x, 0, out=self._buf("f1.x0", (R, D)))
        Y1 = self._buf("f1.y1", (R, 4 * D))
        ops.gemm_nt(X0, w[self.prefix[0] + "0"][1], R, 4 * D, D, ops.EPI_BIAS_BF16, out0=Y1, bias=w[self.prefix[0] + "0"][2])
        with torch.no_grad():
            bias = c0.bias.detach()                            # the shift of the sums is the convolution's bias
            mean, rstd, inv_n = batch_vectors(bn, lambda: self._colstats(Y1, D, bias), self.reduce, shift=bias)
            gamma, beta = bn.weight.detach().contiguous(), bn.bias.detach().contiguous()
        Z1 = ops.neck_bn_gelu_fwd(Y1, mean, rstd, gamma, beta, out=self._buf("f1.z1", (4 * R, D)))
        Y2 = self._buf("f1.y2", (4 * R, 4 * D))
        ops.gemm_nt(Z1, w[self.prefix[0] + "3"][1], 4 * R, 4 * D, D, ops.EPI_BIAS_BF16, out0=Y2, bias=w[self.prefix[0] + "3"][2])
        out = ops.neck_rows_to_maps(Y2, B, D, Hp, Wp, 2, out=self._buf("f1.out", (B, D, 4 * Hp, 4 * Wp), torch.float32))
        return out.detach(), ((X0, Y1, Z1, mean, rstd, inv_n, (B, D, Hp, Wp)) if keep else None)

    def _fpn1_backward(self, saved, dout, need_dx):
        X0, Y1, Z1, mean, rstd, inv_n, (B, D, Hp, Wp) = saved
        R = B * Hp * Wp
        self._attach()
        w = self._weights()
        c0, bn, c3 = self.fpn1[0], self.fpn1[1], self.fpn1[3]
        gamma, beta = bn.weight.detach().contiguous(), bn.bias.detach().contiguous()
        dY2 = ops.neck_maps_to_rows(dout.float().contiguous(), 2, out=self._buf("f1.dy2", (4 * R, 4 * D)))
        self._wgrad(c3, Z1, dY2, 4 * R, D)
        da = self._buf("f1.da", (4 * R, D))
        ops.gemm_nt(dY2, w[self.prefix[0] + "3"][0], 4 * R, D, 4 * D, ops.EPI_BIAS_BF16, out0=da)
        ws = self._buf("sums.ws", (ops.NECK_GROUPS * 2 * D,), torch.float32)
        sums = ops.neck_bn_gelu_bwd_sums(da, Y1, mean, rstd, gamma, beta, ws, out=self._buf("bwd.sums", (2, D), torch.float32))
        add_affine_grads(bn, sums)
        tot = backward_totals(sums, inv_n, self.reduce)
        dY1 = ops.neck_bn_gelu_bwd_apply(da, Y1, mean, rstd, gamma, beta, tot, 1.0, out=self._buf("f1.dy1", (R, 4 * D)))
        self._wgrad(c0, X0, dY1, R, D)
        if not need_dx:
            return None
        dX = self._buf("f1.dx", (R, D))
        ops.gemm_nt(dY1, w[self.prefix[0] + "0"][0], R, D, 4 * D, ops.EPI_BIAS_BF16, out0=dX)
        return ops.neck_rows_to_maps(dX, B, D, Hp, Wp, 0, out=self._buf("f1.dmap", (B, D, Hp, Wp), torch.float32)).detach()

    def fpn1_apply(self, x):
        x = self._check_map(x)
        params = [self.fpn1[0].weight, self.fpn1[0].bias, self.fpn1[1].weight, self.fpn1[1].bias, self.fpn1[3].weight,
                  self.fpn1[3].bias]
        if torch.is_grad_enabled() and self.fpn1[1].training and (x.requires_grad or any(p.requires_grad for p in params)):
            return _Fpn1Function.apply(self, x, *params)
        return self._fpn1_forward(x.detach(), keep=False)[0]
