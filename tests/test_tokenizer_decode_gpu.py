"""The tokenizer's decoder on the HIP path (csrc/convt.hip, HipTokenizer.decode / reconstruct, mem_amd/eval_tokenizer.py)
against torch (reference: eventvae/vae/vae_model.py:92 ConvTranspose2d(4, s2, p1), :160-171 decode, :203-206 KL, :216-266
evaluate).

Layer level: an exact one-hot probe (one non-zero product per output: no rounding) and random layers at the project's bar for
bf16 convolution layers.  Model level: `decode` against the torch module in float64, held to twice the error of torch's own
bf16 evaluation of the same module (both round every activation to bf16 and accumulate in fp32, in different orders).
kl_uniform_rows: held to 4 x the error of the same torch expression in fp32.  Measured pairs: DESIGN.md section 2."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _run_convt(xb, wb, bias, relu, out=None):
    """xb bf16 [B, Cin, H, W], wb bf16 [Cin, Cout, 4, 4] on the GPU -> the padded output buffer [B, 2H+2, 2W+2, Cout].  A fresh
    buffer is pre-filled with 7 inside and 0 on the border ring: a pixel the kernel skips, and a stray border write, both show."""
    from mem_amd import ops
    B, Cin, H, W = xb.shape
    Cout = wb.shape[1]
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.bfloat16, device="cuda")
    xp[:, 1:-1, 1:-1] = xb.permute(0, 2, 3, 1)
    wp = ops.pack_convt_weight(wb.float()).bfloat16().contiguous()           # bf16 values: the packing is exact
    if out is None:
        out = torch.full((B, 2 * H + 2, 2 * W + 2, Cout), 7.0, dtype=torch.bfloat16, device="cuda")
        out[:, 0] = 0
        out[:, -1] = 0
        out[:, :, 0] = 0
        out[:, :, -1] = 0
    ops.convt2d_nhwc(xp, wp, bias, out, B, H, W, Cin, Cout, relu=relu)
    return out


def _ring_is_zero(out):
    return all(float(t.float().abs().max()) == 0.0 for t in (out[:, 0], out[:, -1], out[:, :, 0], out[:, :, -1]))


def test_convt_one_hot_probe_is_exact():
    """A single 1.0 at (b, y, x, c): the output is exactly W[c, :, ky, kx] on the 4x4 footprint rows 2y-1 .. 2y+2, cols
    2x-1 .. 2x+2 (clipped to the image) and exactly 0 elsewhere, the border ring included.  M = 105 < one 128-row tile, H != W,
    C_out ragged in the N tile, two K-tiles per tap.  Catches phase / tap permutations, a y / x swap, any border write."""
    B, H, W, Cin, Cout = 3, 5, 7, 128, 72
    g = torch.Generator(device="cuda").manual_seed(11)
    wb = torch.randn(Cin, Cout, 4, 4, generator=g, device="cuda").bfloat16()
    probes = [(0, 0, 0, 0), (B - 1, H - 1, W - 1, Cin - 1), (0, 0, W - 1, 3), (1, H - 1, 0, 64), (1, 0, 3, 5), (2, 2, 0, 127),
              (1, 2, 3, 70), (B - 1, 3, 5, Cin - 1)]          # four corners, edges, interior; b = B-1, c = Cin-1, both K-tiles
    for b, y, x, c in probes:
        xb = torch.zeros(B, Cin, H, W, dtype=torch.bfloat16, device="cuda")
        xb[b, c, y, x] = 1.0
        out = _run_convt(xb, wb, None, relu=False)
        want = torch.zeros_like(out)
        for ky in range(4):
            for kx in range(4):
                oy, ox = 2 * y - 1 + ky, 2 * x - 1 + kx
                if 0 <= oy < 2 * H and 0 <= ox < 2 * W:
                    want[b, 1 + oy, 1 + ox] = wb[c, :, ky, kx]
        assert torch.equal(out, want), (b, y, x, c, int((out != want).sum()))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(3, 5, 7, 64, 64), (2, 9, 11, 128, 136), (2, 14, 14, 384, 384)])
def test_convt_random_layers_vs_torch(B, H, W, Cin, Cout, relu):
    """F.conv_transpose2d in fp32 on the bf16-rounded operands (on the CPU), rounded to bf16; the bar of the bf16 convolution
    layers (tests/test_tokenizer_gpu.py).  (2, 9, 11, 128, 136): two row tiles, the second ragged, C_out over one N tile."""
    g = torch.Generator().manual_seed(Cin + Cout + H)
    xb = torch.randn(B, Cin, H, W, generator=g).bfloat16()
    wb = (torch.randn(Cin, Cout, 4, 4, generator=g) * 0.05).bfloat16()
    bias = torch.randn(Cout, generator=g)
    ref = F.conv_transpose2d(xb.float(), wb.float(), bias, stride=2, padding=1)
    if relu:
        ref = torch.relu(ref)
    out = _run_convt(xb.cuda(), wb.cuda(), bias.cuda(), relu)
    first = out.clone()
    assert _ring_is_zero(out)
    got = out[:, 1:-1, 1:-1].permute(0, 3, 1, 2).float().cpu()
    torch.testing.assert_close(got, ref.bfloat16().float(), rtol=2e-2, atol=2e-2)
    _run_convt(xb.cuda(), wb.cuda(), bias.cuda(), relu, out=out)             # again, into the same buffer
    assert torch.equal(out, first)


def _module(cfg, seed=0, **kw):
    from mem_amd.vae_model import DiscreteVAE
    from oracle.vae_ref import fill_vae_by_name
    m = DiscreteVAE(**dict(cfg, **kw)).eval()
    m.load_state_dict(fill_vae_by_name(m.state_dict(), seed=seed))
    return m


def _rel(a, truth):
    return float((a.double() - truth).norm() / truth.norm())


@pytest.mark.parametrize("variant", ["tiny", "non_square", "no_resblocks"])
def test_decode_small_models(variant):
    """`decode` of random ids vs the torch module's decode in float64 on the CPU: e_hip <= 2 e_ref, e_ref = the error of torch's
    own bf16 evaluation of the module (on the CPU: no MIOpen).  And decode is independent of the chunking, bit for bit."""
    from mem_amd.vae_model import HipTokenizer
    from oracle.vae_ref import TINY_VAE
    kw = {"tiny": {}, "non_square": dict(input_H=32, input_W=64), "no_resblocks": dict(num_resnet_blocks=0)}[variant]
    m = _module(TINY_VAE, **kw)
    B, hw = 6, (m.input_H >> m.num_layers) * (m.input_W >> m.num_layers)
    ids = torch.randint(0, m.num_tokens, (B, hw), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        truth = copy.deepcopy(m).double().decode(ids)
        e_ref = _rel(copy.deepcopy(m).bfloat16().decode(ids), truth)
    tok = HipTokenizer(m.cuda(), max_batch=B, precision="bf16")
    got = tok.decode(ids.cuda())
    assert got.shape == truth.shape and got.dtype == torch.float32
    e_hip = _rel(got.cpu(), truth)
    print(f"decode {variant}: e_hip = {e_hip:.3e}  e_ref (torch bf16, CPU) = {e_ref:.3e}")
    assert e_hip <= 2 * e_ref, (e_hip, e_ref)
    chunks = tok.decode(ids.cuda(), decode_batch=4)                          # 4 + 2 samples
    assert torch.equal(chunks, got)
    assert torch.equal(torch.cat([tok.decode(ids[:4].cuda()), tok.decode(ids[4:].cuda())]), got)


def test_decode_base_vae():
    """The ViT-B tokenizer shape, B = 1, against the torch module in fp32 on the GPU; e_ref from torch's bf16 autocast on the
    GPU (or, if that arm raises on this build, from module.bfloat16() on the CPU)."""
    from mem_amd.vae_model import HipTokenizer
    from oracle.vae_ref import BASE_VAE
    import time
    t0 = time.time()
    m = _module(BASE_VAE).cuda()
    ids = torch.randint(0, m.num_tokens, (1, 196), generator=torch.Generator().manual_seed(6)).cuda()
    torch.cuda.synchronize()
    t1 = time.time()
    with torch.no_grad():
        truth = m.decode(ids).double()
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ref16 = m.decode(ids)
            arm = "torch bf16 autocast, GPU"
        except RuntimeError as e:
            print(f"bf16 autocast raised ({str(e)[:80]}): e_ref from module.bfloat16() on the CPU")
            ref16 = copy.deepcopy(m).cpu().bfloat16().decode(ids.cpu()).cuda()
            arm = "torch bf16, CPU"
    e_ref = _rel(ref16, truth)
    t2 = time.time()
    tok = HipTokenizer(m, max_batch=1, precision="bf16")
    e_hip = _rel(tok.decode(ids), truth)
    print(f"decode BASE_VAE: e_hip = {e_hip:.3e}  e_ref ({arm}) = {e_ref:.3e}   "
          f"[s: module {t1 - t0:.1f}, torch arms {t2 - t1:.1f}, hip {time.time() - t2:.1f}]")
    assert e_hip <= 2 * e_ref, (e_hip, e_ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [512, 8192])
def test_kl_uniform_rows(N, dtype):
    """Against F.kl_div(log_uniform, log_softmax(logits.double())) summed over the row; bar: 4 x the error of the same
    expression in fp32.  Logits at the tokenizer's spread (std 1.8), one row of equal logits (KL = 0), one near one-hot."""
    from mem_amd import ops
    M = 300
    g = torch.Generator(device="cuda").manual_seed(N)
    x = torch.randn(M, N, generator=g, device="cuda") * 1.8
    x[0] = 0.37
    x[1, 17] += 40.0
    x = x.to(dtype)

    def kl(t):
        log_uniform = torch.log(torch.tensor([1.0 / N], dtype=t.dtype, device="cuda"))
        return F.kl_div(log_uniform, F.log_softmax(t, dim=-1), reduction="none", log_target=True).sum(-1)
    truth = kl(x.double())
    err_torch = float((kl(x.float()).double() - truth).abs().max())
    got = ops.kl_uniform_rows(x, M, N)
    err_hip = float((got.double() - truth).abs().max())
    print(f"kl_uniform_rows N={N} {dtype}: err_hip = {err_hip:.3e}  err_torch_fp32 = {err_torch:.3e}  "
          f"(KL mean {float(truth.mean()):.3f}, equal-logit row {float(got[0]):.3e}, one-hot row {float(got[1]):.4f})")
    assert abs(float(got[0])) <= 1e-6 and abs(float(got[1]) - float(truth[1])) <= 1e-5
    assert err_hip <= 4 * err_torch, (err_hip, err_torch)


def test_eval_tokenizer_evaluate():
    """evaluate on a two-batch loader (batch sizes 4 and 2): the four numbers, and one encoder run per batch."""
    from mem_amd import eval_tokenizer
    from mem_amd.vae_model import HipTokenizer
    from oracle.vae_ref import TINY_VAE
    weight = 0.5
    m = _module(TINY_VAE, kl_div_loss_weight=weight, loss="smooth_l1", normalization=((0.5,) * 3, (0.25,) * 3)).cuda()
    g = torch.Generator().manual_seed(9)
    loader = [(torch.rand(4, 3, 64, 64, generator=g), torch.zeros(4)), (torch.rand(2, 3, 64, 64, generator=g), torch.zeros(2))]
    tok = HipTokenizer(m, max_batch=4, precision="fp32")
    # expected, batch by batch (the tokenizer is deterministic); the reference meter weighs a batch by 1 + its size
    ids_all, recon_v, kl_v, wts = [], [], [], []
    for images, _ in loader:
        images = images.cuda()
        ids, recon = tok.reconstruct(images)
        ids_all.append(ids.reshape(-1))
        recon_v.append(float(m.loss_fn(m.norm(images), recon)))
        logits = tok.logits[: ids.numel()].double()
        log_uniform = torch.log(torch.tensor([1.0 / m.num_tokens], dtype=torch.float64, device="cuda"))
        kl_v.append(float(F.kl_div(log_uniform, F.log_softmax(logits, -1), reduction="sum", log_target=True))
                    / images.shape[0])                                     # summed over tokens and ids, per sample
        wts.append(1 + images.shape[0])
    avg = lambda v: sum(a * b for a, b in zip(v, wts)) / sum(wts)
    calls = []
    inner = tok.get_codebook_indices
    tok.get_codebook_indices = lambda images: (calls.append(1), inner(images))[1]
    stats = eval_tokenizer.evaluate(loader, tok, torch.device("cuda"))
    assert len(calls) == len(loader)                                        # the KL read the logits of that call
    assert set(stats) == {"loss", "recon_loss", "kl_div", "codebook_indices"}
    assert stats["codebook_indices"] == len(torch.unique(torch.cat(ids_all)))
    assert stats["recon_loss"] == pytest.approx(avg(recon_v), rel=1e-6)
    assert stats["kl_div"] == pytest.approx(avg(kl_v), rel=1e-5) and stats["kl_div"] > 0
    assert stats["loss"] == pytest.approx(stats["recon_loss"] + stats["kl_div"] * weight, rel=1e-6)
    assert stats["loss"] != pytest.approx(stats["recon_loss"], rel=1e-3)    # the weight is not zero
