"""Training the event dVAE tokenizer on the HIP path (reference: eventvae/vae/vae_model.py:173-213 the training forward,
eventvae/train_vae.py:220,335-337 Adam with gradient clipping).

`DVAEEngine` has an explicit forward and backward, like ViTEngine: no autograd runs through the HIP segments.

  forward   nchw_to_padded_nhwc4(norm) -> the bf16 encoder (csrc/conv.hip), every activation KEPT -> bf16 token logits [M, T],
            rows (b, y, x) -> the sampling segment in fp32 torch ops, softmax((logits + gumbel) / temp), with `straight_through`
            the hard one-hot forward with the soft gradient -> sampled = soft @ codebook (memhip_gemm_bf16_nt) -> the bf16
            decoder (conv.hip, convt.hip), kept -> the dense reconstruction head -> recon_loss = loss_fn(norm(img), out) and
            kl_div (ops.kl_uniform_rows).
  backward  the two losses and the sampling segment are leaf segments differentiated by torch.autograd on their own inputs;
            dsoft = dsampled @ codebook^T (NT GEMM on the codebook as stored), dcodebook = soft^T @ dsampled (gemm_tn with
            workspace); every data gradient of a convolution is a FORWARD kernel with a re-read weight
            (vae_model.pack_dgrad_weight), every weight gradient one ops.conv_wgrad call (csrc/conv_wgrad.hip), every ReLU
            backward / bias gradient one ops.relu_bwd_colsum call.  Those two use no atomics.  The codebook gradient goes through
            memhip_gemm_bf16_tn, which folds its slices through the workspace where its plan allows (the ViT-B tokenizer's shape)
            and adds them with fp32 atomics otherwise.

KL convention: the project's one definition (eval_tokenizer.evaluate), kl_div = sum over the token rows / batch size.  The
reference's F.kl_div(log_uniform[1], ..., 'batchmean') divides by 1, not by the batch size: its figure -- and the weight its
kl_div_loss_weight effectively has -- is B x ours.

fp32 masters and gradients are two flat buffers; the module's parameters become views of the masters and their .grad views of
the gradient buffer (bound again in front of every backward, so optimizer.zero_grad() may set them to None), so any torch
optimizer, clip_grad_norm_, state_dict() and the reference checkpoint format keep working.
`step` is memhip_grad_norm + memhip_adamw with weight_decay 0: Adam with the clip folded in.  Single GPU."""
from contextlib import contextmanager

import torch
import torch.nn.functional as F
from torch import nn

from .vae_model import ResBlock, pack_conv_weight, pack_convt_weight, pack_dgrad_weight

BF = torch.bfloat16


def _pad_to(n, m):
    return -(-n // m) * m


class DVAEEngine:
    def __init__(self, vae, seed=0):
        first = vae.encoder[0][0]
        self.hid, self.channels = first.out_channels, first.in_channels
        self.T, self.cd = vae.codebook.weight.shape
        # what the kernels cannot take, by name -- before anything touches a device
        if self.hid % 64:
            raise ValueError(f"DVAEEngine: hidden_dim={self.hid} must be a multiple of 64 (the bf16 convolutions' C_in)")
        if self.channels > 4:
            raise ValueError(f"DVAEEngine: channels={self.channels} > 4 (the first layer reads the 4-channel NHWC format)")
        if self.T % 64:
            raise ValueError(f"DVAEEngine: num_tokens={self.T} must be a multiple of 64 (the K of the codebook GEMMs)")
        from . import ops
        from ._lib import require_gpu
        require_gpu()
        self.ops, self.vae = ops, vae
        dev = next(vae.parameters()).device
        assert dev.type == "cuda", "DVAEEngine needs the model on the GPU"
        self.dev, self.H, self.W = dev, vae.input_H, vae.input_W
        self.cpad = _pad_to(self.cd, 64)
        self.cout8 = _pad_to(self.channels, 8)
        self.norm = None
        if vae.normalization is not None:
            self.norm = tuple(torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous() for t in vae.normalization)
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self._flatten()
        hid = self.hid
        self.enc, self.dec = [], []
        cin = 4
        for m in vae.encoder:
            if isinstance(m, nn.Sequential):
                self.enc.append({"kind": "conv", "m": m[0], "cin": cin, "cout": hid})
                cin = hid
            elif isinstance(m, ResBlock):
                self.enc.append({"kind": "res", "m": (m.net[0], m.net[2], m.net[4]), "ch": hid})
            else:
                self.enc.append({"kind": "head", "m": m, "cin": hid, "cout": self.T})
        cin = self.cpad
        for m in vae.decoder:
            if isinstance(m, nn.Sequential):
                self.dec.append({"kind": "convt", "m": m[0], "cin": cin, "cout": hid})
                cin = hid
            elif isinstance(m, ResBlock):
                self.dec.append({"kind": "res", "m": (m.net[0], m.net[2], m.net[4]), "ch": hid})
            elif m is vae.decoder[-1]:
                self.dec.append({"kind": "head", "m": m, "cin": hid, "cout": self.cout8})
            else:
                self.dec.append({"kind": "conv1", "m": m, "cin": cin, "cout": hid})
                cin = hid
        self.B = 0
        self.t = 0
        self.wg_ws = None
        self.relu_ws = None
        self.last_hard_ids = None
        self.timers = None          # tools/bench_dvae_train.py: {segment: [(start event, end event)]}
        self.sh = {}

    @contextmanager
    def _seg(self, name):
        """A leaf segment of the step between two device events, when self.timers is a dict (the A/B tool's step split)."""
        if self.timers is None:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        self.timers.setdefault(name, []).append((e0, e1))

    def _mark(self, name):
        """The coarse phases of a step: everything up to the next mark belongs to `name` (None closes the last one)."""
        if self.timers is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.timers.setdefault("_marks", []).append((name, e))

    def _dconv(self, *a, **kw):
        with self._seg("dgrad"):
            self.ops.conv2d_nhwc(*a, **kw)

    # ---------------------------------------------------------------- parameters: flat masters, flat gradients
    def _flatten(self):
        params = list(self.vae.parameters())
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += _pad_to(p.numel(), 1024)                  # the optimizer kernels work on chunks of 1024
        self.n, self.params, self.offs = n, params, offs
        self.master = torch.zeros(n, dtype=torch.float32, device=self.dev)
        self.gflat = torch.zeros(n, dtype=torch.float32, device=self.dev)
        self.m, self.v = torch.zeros_like(self.master), torch.zeros_like(self.master)
        for p, o in zip(params, offs):
            view = self.master[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
        self._bind_grads()
        self.wd_flags = torch.zeros(n // 1024, dtype=torch.uint8, device=self.dev)
        self.gnorm = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.norm_ws = torch.zeros(1024, dtype=torch.float64, device=self.dev)

    def _bind_grads(self):
        """Every parameter's .grad is its view of the flat gradient buffer.  Called in front of every backward: a torch
        optimizer's zero_grad() (set_to_none=True by default) drops the views."""
        for p, o in zip(self.params, self.offs):
            g = p.grad
            if g is None or g.data_ptr() != self.gflat.data_ptr() + 4 * o:
                p.grad = self.gflat[o:o + p.numel()].view(p.shape)

    def _repack(self):
        """The bf16 shadows of one step: every weight in its forward layout and in the layout of the kernel that computes the
        layer's data gradient.  Plain torch on the masters."""
        sh = {}

        def bf(t):
            return t.to(BF).contiguous()
        for i, L in enumerate(self.enc):
            if L["kind"] == "conv":
                w = L["m"].weight.detach()
                wf = F.pad(w, (0, 0, 0, 0, 0, L["cin"] - w.shape[1]))
                sh[L["m"]] = (bf(pack_conv_weight(wf)), None if i == 0 else bf(pack_dgrad_weight("conv4s2", w)))
            elif L["kind"] == "head":
                w = L["m"].weight.detach()
                sh[L["m"]] = (bf(pack_conv_weight(w)), bf(pack_dgrad_weight("conv1", w)))
        for L in self.dec:
            w = L["m"].weight.detach() if L["kind"] != "res" else None
            if L["kind"] == "convt":
                sh[L["m"]] = (bf(pack_convt_weight(w, cin_pad=L["cin"])), bf(pack_dgrad_weight("convt", w, cout_pad=L["cin"])))
            elif L["kind"] == "conv1":
                wf = F.pad(w, (0, 0, 0, 0, 0, L["cin"] - w.shape[1]))
                sh[L["m"]] = (bf(pack_conv_weight(wf)), bf(pack_dgrad_weight("conv1", w, cout_pad=L["cin"])))
            elif L["kind"] == "head":
                wf = F.pad(w, (0, 0, 0, 0, 0, 0, 0, L["cout"] - w.shape[0]))
                sh[L["m"]] = (bf(pack_conv_weight(wf)), bf(pack_dgrad_weight("conv1", w, cin_pad=64)))
                self.head_bias = F.pad(L["m"].bias.detach().float(), (0, L["cout"] - w.shape[0])).contiguous()
        for L in self.enc + self.dec:
            if L["kind"] == "res":
                c1, c2, c3 = L["m"]
                for c, kind in ((c1, "conv3"), (c2, "conv3"), (c3, "conv1")):
                    sh[c] = (bf(pack_conv_weight(c.weight.detach())), bf(pack_dgrad_weight(kind, c.weight.detach())))
        cb = F.pad(self.vae.codebook.weight.detach(), (0, self.cpad - self.cd))
        self.cb16, self.cbT16 = bf(cb), bf(cb.t())
        self.sh = sh

    # ---------------------------------------------------------------- buffers
    def _zeros(self, B, h, w, c):
        return torch.zeros((B, h + 2, w + 2, c), dtype=BF, device=self.dev)

    def _alloc(self, B):
        """Zero-bordered activation buffers for batch B, one per activation (nothing is rotated: the backward reads them all);
        gradient buffers come from a pool per shape."""
        if B == self.B:
            return
        self.B, dev = B, self.dev
        self.gpool = {}
        h, w = self.H, self.W
        self.x0 = self._zeros(B, h, w, 4)
        for L in self.enc:
            if L["kind"] == "conv":
                h, w = h // 2, w // 2
                L["y"] = self._zeros(B, h, w, L["cout"])
            elif L["kind"] == "res":
                L["t1"], L["t2"], L["y"] = (self._zeros(B, h, w, L["ch"]) for _ in range(3))
        self.h, self.w = h, w
        M = B * h * w
        self.logits = torch.empty((M, self.T), dtype=BF, device=dev)
        self.glogits = torch.empty((M, self.T), dtype=BF, device=dev)
        self.sampled = torch.empty((M, self.cpad), dtype=BF, device=dev)
        self.dsoft = torch.empty((M, self.T), dtype=torch.float32, device=dev)
        self.gcb = torch.empty((self.T, self.cpad), dtype=torch.float32, device=dev)
        self.dx0 = self._zeros(B, h, w, self.cpad)
        for L in self.dec:
            if L["kind"] == "convt":
                h, w = 2 * h, 2 * w
                L["y"] = self._zeros(B, h, w, L["cout"])
            elif L["kind"] == "conv1":
                L["y"] = self._zeros(B, h, w, L["cout"])
            elif L["kind"] == "res":
                L["t1"], L["t2"], L["y"] = (self._zeros(B, h, w, L["ch"]) for _ in range(3))
        Mo = B * self.H * self.W
        self.rec = torch.empty((Mo, self.cout8), dtype=BF, device=dev)
        self.grec64 = torch.zeros((Mo, 64), dtype=BF, device=dev)       # the head's g, zero-padded to the NT GEMM's K
        self.dense = torch.empty((max(Mo, M), self.hid), dtype=BF, device=dev)
        wide = max(self.hid, self.cpad)
        self.G = torch.empty(max(16 * self.hid * wide, self.T * self.hid), dtype=torch.float32, device=dev)    # the largest [N, k*k*C]
        self.csum = torch.empty(max(wide, self.T), dtype=torch.float32, device=dev)
        tn = self.ops.gemm_tn_workspace(M, self.T, self.cpad)
        self.tn_ws = torch.empty(tn, dtype=torch.uint8, device=dev) if tn else None

    def _gbuf(self, h, w, c, exclude=()):
        pool = self.gpool.setdefault((h, w, c), [])
        for t in pool:
            if not any(t is e for e in exclude):
                return t
        pool.append(self._zeros(self.B, h, w, c))
        return pool[-1]

    # ---------------------------------------------------------------- the per-layer pieces of the backward
    def _wgrad(self, small, big, hs, ws_, C_, N, k, s, p, small_padded=True):
        """ops.conv_wgrad into the scratch G -> f32 [N, k, k, C]."""
        ops, B = self.ops, self.B
        need = ops.conv_wgrad_workspace(B, hs, ws_, C_, N, k, s, p, small_padded=small_padded)
        if need and (self.wg_ws is None or self.wg_ws.numel() * 4 < need):
            self.wg_ws = torch.empty(need // 4, dtype=torch.float32, device=self.dev)
        G = self.G[: N * k * k * C_]
        with self._seg("conv_wgrad k%d s%d M=%d C=%d N=%d" % (k, s, B * hs * ws_, C_, N)):
            ops.conv_wgrad(small, big, G, B, hs, ws_, C_, N, k, s, p, small_padded=small_padded, accumulate=False,
                           workspace=self.wg_ws if need else None)
        return G.view(N, k, k, C_)

    def _conv_wgrad(self, conv, g, x, hs, ws_, cin, k, s, p, small_padded=True):
        """weight.grad of a Conv2d [Co, Ci, k, k] from g (its pre-activation's gradient, N channels) and its input x (cin)."""
        co, ci = conv.weight.shape[:2]
        N = g.shape[-1]
        G = self._wgrad(g, x, hs, ws_, cin, N, k, s, p, small_padded)
        with self._seg("grad_layout"):
            conv.weight.grad.copy_(G[:co, :, :, :ci].permute(0, 3, 1, 2))

    def _relu_bias(self, g, y, bias, h, w, c, padded=True):
        """g *= (y > 0) in place (y None: no mask) and bias.grad = the column sums of the masked g."""
        n = bias.numel()
        direct = n == c
        cs = bias.grad if direct else self.csum[:c]
        need = self.ops.relu_bwd_colsum_workspace(self.B, h, w, c)      # of THIS call: the row-block count is not monotone in the size
        if self.relu_ws is None or self.relu_ws.numel() * 4 < need:
            self.relu_ws = torch.empty(need // 4, dtype=torch.float32, device=self.dev)
        with self._seg("relu_bwd_colsum"):
            self.ops.relu_bwd_colsum(g, y, self.B, h, w, c, padded=padded, colsum=cs, accumulate=False, workspace=self.relu_ws)
            if not direct:
                bias.grad.copy_(cs[:n])

    def _res_fwd(self, L, x, h, w):
        conv, sh, B, ch = self.ops.conv2d_nhwc, self.sh, self.B, L["ch"]
        c1, c2, c3 = L["m"]
        conv(x, sh[c1][0], c1.bias.data, L["t1"], B, h, w, ch, ch, 3, 1, 1, relu=True)
        conv(L["t1"], sh[c2][0], c2.bias.data, L["t2"], B, h, w, ch, ch, 3, 1, 1, relu=True)
        conv(L["t2"], sh[c3][0], c3.bias.data, L["y"], B, h, w, ch, ch, 1, 1, 0, relu=False, add=x)      # net(x) + x
        L["x"] = x
        return L["y"]

    def _res_bwd(self, L, g, h, w):
        """g = the gradient of net(x) + x -> the gradient of x; fills the six parameter gradients of the block."""
        conv, sh, B, ch = self._dconv, self.sh, self.B, L["ch"]
        c1, c2, c3 = L["m"]
        x, t1, t2 = L["x"], L["t1"], L["t2"]
        self._relu_bias(g, None, c3.bias, h, w, ch)
        self._conv_wgrad(c3, g, t2, h, w, ch, 1, 1, 0)
        g2 = self._gbuf(h, w, ch, exclude=(g,))
        conv(g, sh[c3][1], None, g2, B, h, w, ch, ch, 1, 1, 0)
        self._relu_bias(g2, t2, c2.bias, h, w, ch)
        self._conv_wgrad(c2, g2, t1, h, w, ch, 3, 1, 1)
        g1 = self._gbuf(h, w, ch, exclude=(g, g2))
        conv(g2, sh[c2][1], None, g1, B, h, w, ch, ch, 3, 1, 1)
        self._relu_bias(g1, t1, c1.bias, h, w, ch)
        self._conv_wgrad(c1, g1, x, h, w, ch, 3, 1, 1)
        conv(g1, sh[c1][1], None, g2, B, h, w, ch, ch, 3, 1, 1, add=g)            # dX = dgrad_c1(g1) + g; g2 is free again
        return g2

    # ---------------------------------------------------------------- one step
    def forward_backward(self, images, temp, noise=None, hard_ids=None):
        """loss, recon_loss, kl_div (0-dim tensors on the device) of vae_model.py:184-208 in training mode, with every parameter's
        .grad filled (overwritten).  images f32 [B, C, H, W] on the GPU; noise: f32 [M, T] Gumbel noise, rows (b, y, x) (default:
        drawn on the device from the engine's generator); hard_ids (straight_through only): i64 [M] the one-hot ids to use
        instead of the argmax.  kl_div = sum over the token rows / B (see the module docstring)."""
        ops, vae = self.ops, self.vae
        conv = ops.conv2d_nhwc
        assert images.is_cuda and images.dtype == torch.float32 and images.shape[1:] == (self.channels, self.H, self.W)
        images = images.contiguous()
        B = images.shape[0]
        self._alloc(B)
        self._bind_grads()
        self._mark("repack")
        self._repack()
        sh = self.sh
        self._mark("encoder_fwd")
        # ---- encoder, kept
        ops.nchw_to_padded_nhwc4(images, self.x0, *(self.norm or (None, None)))
        cur, h, w = self.x0, self.H, self.W
        for L in self.enc:
            m = L["m"]
            if L["kind"] == "conv":
                L["x"] = cur
                conv(cur, sh[m][0], m.bias.data, L["y"], B, h, w, L["cin"], L["cout"], 4, 2, 1, relu=True)
                cur, h, w = L["y"], h // 2, w // 2
            elif L["kind"] == "res":
                cur = self._res_fwd(L, cur, h, w)
            else:
                L["x"] = cur
                conv(cur, sh[m][0], m.bias.data, self.logits, B, h, w, L["cin"], L["cout"], 1, 1, 0, relu=False, out_padded=False)
        M, T = B * h * w, self.T
        # ---- the sampling segment: fp32 torch ops, differentiated on its own leaf
        self._mark("sampling_fwd")
        lg = self.logits.float().requires_grad_(True)
        if noise is None:
            noise = -torch.empty((M, T), dtype=torch.float32, device=self.dev).exponential_(generator=self.gen).log()
        assert noise.shape == (M, T)
        soft = torch.softmax((lg + noise) / temp, dim=-1)
        y = soft
        if vae.straight_through:
            ids = soft.argmax(-1) if hard_ids is None else hard_ids.reshape(-1).to(self.dev)
            self.last_hard_ids = ids.detach().clone()
            hard = torch.zeros_like(soft).scatter_(1, ids[:, None], 1.0)
            y = hard - soft.detach() + soft
        else:
            assert hard_ids is None, "hard_ids goes with straight_through"
        y16 = y.detach().to(BF)
        ops.gemm_nt(y16, self.cbT16, M, self.cpad, T, ops.EPI_BIAS_BF16, out0=self.sampled)       # sampled = soft @ codebook
        self.dx0[:, 1:-1, 1:-1] = self.sampled.view(B, h, w, self.cpad)
        # ---- decoder, kept
        self._mark("decoder_fwd")
        cur = self.dx0
        for L in self.dec:
            m = L["m"]
            if L["kind"] == "conv1":
                L["x"] = cur
                conv(cur, sh[m][0], m.bias.data, L["y"], B, h, w, L["cin"], L["cout"], 1, 1, 0, relu=False)
                cur = L["y"]
            elif L["kind"] == "res":
                cur = self._res_fwd(L, cur, h, w)
            elif L["kind"] == "convt":
                L["x"] = cur
                ops.convt2d_nhwc(cur, sh[m][0], m.bias.data, L["y"], B, h, w, L["cin"], L["cout"], relu=True)
                cur, h, w = L["y"], 2 * h, 2 * w
            else:
                L["x"] = cur
                conv(cur, sh[m][0], self.head_bias, self.rec, B, h, w, L["cin"], L["cout"], 1, 1, 0, relu=False, out_padded=False)
        # ---- the two losses (leaf segments)
        self._mark("losses")
        C_ = self.channels
        o = self.rec.float().requires_grad_(True)
        out = o[:, :C_].view(B, self.H, self.W, C_).permute(0, 3, 1, 2)
        recon_loss = vae.loss_fn(vae.norm(images), out)
        recon_loss.backward()
        kl_div = ops.kl_uniform_rows(self.logits, M, T).sum() / B
        loss = recon_loss.detach() + kl_div * vae.kl_div_loss_weight
        # ---- decoder backward
        self._mark("decoder_bwd")
        self.grec64[:, : self.cout8] = o.grad.to(BF)
        g = self._dec_backward(h, w)
        self._mark("sampling_bwd")
        dsampled = g[:, 1:-1, 1:-1].reshape(M, self.cpad).contiguous()
        ops.gemm_nt(dsampled, self.cb16, M, T, self.cpad, ops.EPI_F32, out0=self.dsoft)           # dsoft = dsampled @ codebook^T
        ops.gemm_tn(y16, dsampled, M, T, self.cpad, self.gcb, accumulate=False, workspace=self.tn_ws)    # dcodebook = soft^T @ dsampled
        vae.codebook.weight.grad.copy_(self.gcb[:, : self.cd])
        # ---- back through the sampling segment, plus the KL gradient on the logits
        tail = (y * self.dsoft).sum()
        if vae.kl_div_loss_weight:
            lq = F.log_softmax(lg, dim=-1)
            tail = tail + (lq.exp() * lq).sum() * (vae.kl_div_loss_weight / B)
        tail.backward()
        self.glogits.copy_(lg.grad)
        self._mark("encoder_bwd")
        self._enc_backward()
        self._mark(None)
        return loss, recon_loss.detach(), kl_div

    def _dec_backward(self, h, w):
        """From self.grec64 (the dense gradient of the reconstruction) to the gradient of the sampled embeddings (padded)."""
        ops, sh, B = self.ops, self.sh, self.B
        conv = self._dconv
        g = None
        for L in reversed(self.dec):
            m = L["m"]
            if L["kind"] == "head":
                Mo, c8, hid = B * h * w, L["cout"], L["cin"]
                grec = self.grec64[:, :c8].contiguous()
                self._relu_bias(grec, None, m.bias, h, w, c8, padded=False)
                self._conv_wgrad(m, grec, L["x"], h, w, hid, 1, 1, 0, small_padded=False)
                g = self._gbuf(h, w, hid)
                with self._seg("dgrad"):
                    ops.gemm_nt(self.grec64, sh[m][1], Mo, hid, 64, ops.EPI_BIAS_BF16, out0=self.dense)
                    g[:, 1:-1, 1:-1] = self.dense[:Mo].view(B, h, w, hid)
            elif L["kind"] == "convt":
                cin, cout = L["cin"], L["cout"]
                self._relu_bias(g, L["y"], m.bias, h, w, cout)
                h, w = h // 2, w // 2
                G = self._wgrad(L["x"], g, h, w, cout, cin, 4, 2, 1)                  # roles swapped: G[ci, (ky, kx, co)]
                with self._seg("grad_layout"):
                    m.weight.grad.copy_(G[: m.weight.shape[0]].permute(0, 3, 1, 2))
                dx = self._gbuf(h, w, cin)
                conv(g, sh[m][1], None, dx, B, 2 * h, 2 * w, cout, cin, 4, 2, 1)
                g = dx
            elif L["kind"] == "res":
                g = self._res_bwd(L, g, h, w)
            else:                                                                 # the 1x1 behind the codebook
                cin, cout = L["cin"], L["cout"]
                self._relu_bias(g, None, m.bias, h, w, cout)
                self._conv_wgrad(m, g, L["x"], h, w, cin, 1, 1, 0)
                dx = self._gbuf(h, w, cin)
                conv(g, sh[m][1], None, dx, B, h, w, cout, cin, 1, 1, 0)
                g = dx
        return g

    def _enc_backward(self):
        ops, sh, B = self.ops, self.sh, self.B
        h, w = self.h, self.w
        M = B * h * w
        g = None
        for i in reversed(range(len(self.enc))):
            L = self.enc[i]
            m = L["m"]
            if L["kind"] == "head":
                hid, T = L["cin"], L["cout"]
                self._relu_bias(self.glogits, None, m.bias, h, w, T, padded=False)
                self._conv_wgrad(m, self.glogits, L["x"], h, w, hid, 1, 1, 0, small_padded=False)
                g = self._gbuf(h, w, hid)
                with self._seg("dgrad"):
                    ops.gemm_nt(self.glogits, sh[m][1], M, hid, T, ops.EPI_BIAS_BF16, out0=self.dense)
                    g[:, 1:-1, 1:-1] = self.dense[:M].view(B, h, w, hid)
            elif L["kind"] == "res":
                g = self._res_bwd(L, g, h, w)
            else:
                cin, cout = L["cin"], L["cout"]
                self._relu_bias(g, L["y"], m.bias, h, w, cout)
                self._conv_wgrad(m, g, L["x"], h, w, cin, 4, 2, 1)
                if i > 0:                                                         # the first layer needs no data gradient
                    dx = self._gbuf(2 * h, 2 * w, cin)
                    with self._seg("dgrad"):
                        ops.convt2d_nhwc(g, sh[m][1], None, dx, B, h, w, cout, cin)
                    g = dx
                h, w = 2 * h, 2 * w

    def step(self, lr, max_norm=0.0):
        """Adam (betas 0.9 / 0.999, eps 1e-8, no weight decay: train_vae.py:220) on the flat masters, with
        clip_grad_norm_(max_norm) folded in (train_vae.py:335-337; 0: no clipping).  Returns the gradient norm (device scalar)."""
        ops = self.ops
        self.t += 1
        self._mark("optimizer")
        ops.grad_norm(self.gflat, self.n, self.gnorm, self.norm_ws)
        ops.adamw(self.master, self.gflat, self.m, self.v, self.n, self.wd_flags, lr, 0.9, 0.999, 1e-8, 0.0, self.t,
                  gnorm=self.gnorm if max_norm else None, max_norm=max_norm)
        self._mark(None)
        return self.gnorm[0]

    # ---------------------------------------------------------------- the optimizer state in torch.optim.Adam's format
    def optimizer_state_dict(self, lr):
        """The Adam moments as a torch.optim.Adam(vae.parameters()) state dict (the 'optimizer' entry of a checkpoint)."""
        state = {}
        if self.t > 0:
            for i, (p, o) in enumerate(zip(self.params, self.offs)):
                sl = slice(o, o + p.numel())
                state[i] = {"step": torch.tensor(float(self.t)), "exp_avg": self.m[sl].view(p.shape).cpu().clone(),
                            "exp_avg_sq": self.v[sl].view(p.shape).cpu().clone()}
        group = {"lr": lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
                 "capturable": False, "differentiable": False, "fused": None, "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        for i, st in sd.get("state", {}).items():
            p, o = self.params[i], self.offs[i]
            sl = slice(o, o + p.numel())
            self.m[sl].copy_(st["exp_avg"].reshape(-1))
            self.v[sl].copy_(st["exp_avg_sq"].reshape(-1))
            self.t = int(st["step"])
