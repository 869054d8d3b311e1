"""Training the dVAE tokenizer on the HIP path (mem_amd/vae_train.py DVAEEngine, python -m mem_amd.train_vae) against a torch
restatement of the training loss (reference: eventvae/vae/vae_model.py:184-208, eventvae/train_vae.py:220,304-396).

The restatement below is written for these tests: the module's own encoder / decoder with the Gumbel noise injected as rows
(b, y, x) and the project's KL convention (sum over the token rows / batch size).  Truth is the restatement in float64 on the
CPU; e_ref is the error of the same restatement on module.bfloat16() (torch's own bf16 arithmetic, sampling segment in fp32
like the engine's).  The engine is held to twice that: globally e_hip <= 2 e_ref, per tensor e_hip[k] <= 2 max(e_ref[k], e_ref)."""
import copy
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _module(cfg, seed=0, **kw):
    from mem_amd.vae_model import DiscreteVAE
    from oracle.vae_ref import fill_vae_by_name
    m = DiscreteVAE(**dict(cfg, **kw))
    m.load_state_dict(fill_vae_by_name(m.state_dict(), seed=seed))
    return m


def restated_loss(m, img, temp, noise, hard_ids=None):
    """(loss, recon_loss, kl_div) of vae_model.py:184-208 on module `m` in m's dtype; noise f32/f64 [M, T], rows (b, y, x).  The
    sampling segment and the losses run in at least fp32.  kl_div = sum over rows / B."""
    dt = m.codebook.weight.dtype
    hi = torch.float64 if dt == torch.float64 else torch.float32
    B = img.shape[0]
    x = m.norm(img.to(dt))
    logits = m.encoder(x)
    _, T, h, w = logits.shape
    rows = logits.permute(0, 2, 3, 1).reshape(-1, T).to(hi)
    soft = torch.softmax((rows + noise.to(hi)) / temp, dim=-1)
    y = soft
    if m.straight_through:
        hard = torch.zeros_like(soft).scatter_(1, hard_ids.reshape(-1, 1), 1.0)
        y = hard - soft.detach() + soft
    sampled = (y.to(dt) @ m.codebook.weight).view(B, h, w, -1).permute(0, 3, 1, 2)
    out = m.decoder(sampled)
    recon = m.loss_fn(x.to(hi), out.to(hi))
    lq = F.log_softmax(rows, dim=-1)
    kl = ((lq.exp() * lq).sum(-1) + math.log(T)).sum() / B
    return recon + kl * m.kl_div_loss_weight, recon, kl


def _grads(m, img, temp, noise, hard_ids=None):
    m.zero_grad()
    loss, recon, kl = restated_loss(m, img, temp, noise, hard_ids)
    loss.backward()
    return {k: p.grad.detach().double() for k, p in m.named_parameters()}, [float(v.detach()) for v in (loss, recon, kl)]


def _errors(got, truth):
    per = {k: float((got[k] - truth[k]).norm() / truth[k].norm()) for k in truth}
    glob = math.sqrt(sum(float((got[k] - truth[k]).norm()) ** 2 for k in truth)) / math.sqrt(sum(float(truth[k].norm()) ** 2 for k in truth))
    return per, glob


@pytest.mark.parametrize("variant", ["tiny", "non_square", "no_resblocks", "tiny_straight_through"])
def test_gradient_parity(variant):
    from mem_amd.vae_train import DVAEEngine
    from oracle.vae_ref import TINY_VAE
    kw = {"tiny": {}, "non_square": dict(input_H=32, input_W=64), "no_resblocks": dict(num_resnet_blocks=0),
          "tiny_straight_through": dict(straight_through=True)}[variant]
    m = _module(TINY_VAE, kl_div_loss_weight=0.01, **kw)
    B, temp = 3, 0.9
    M = B * (m.input_H >> m.num_layers) * (m.input_W >> m.num_layers)
    gen = torch.Generator().manual_seed(17)
    img = torch.rand(B, 3, m.input_H, m.input_W, generator=gen)
    noise = -torch.empty(M, m.num_tokens).exponential_(generator=gen).log()
    eng = DVAEEngine(copy.deepcopy(m).cuda())
    loss, recon, kl = eng.forward_backward(img.cuda(), temp, noise=noise.cuda())
    got = {k: p.grad.detach().double().cpu() for k, p in eng.vae.named_parameters()}
    got_l = [float(v.detach()) for v in (loss, recon, kl)]
    ids = eng.last_hard_ids.cpu() if m.straight_through else None
    truth, truth_l = _grads(copy.deepcopy(m).double(), img.double(), temp, noise.double(), ids)
    ref, ref_l = _grads(copy.deepcopy(m).bfloat16(), img, temp, noise, ids)
    e_ref, e_ref_g = _errors(ref, truth)
    e_hip, e_hip_g = _errors(got, truth)
    print(variant, "global e_hip %.3e e_ref %.3e" % (e_hip_g, e_ref_g))
    for k in truth:
        print("  %-28s e_hip %.3e  e_ref %.3e" % (k, e_hip[k], e_ref[k]))
    for name, a, r, t in zip(("loss", "recon_loss", "kl_div"), got_l, ref_l, truth_l):
        print("  %-10s hip %.6f ref %.6f truth %.6f" % (name, a, r, t))
    assert all(torch.isfinite(v).all() for v in got.values())
    assert e_hip_g <= 2 * e_ref_g
    for k in truth:
        assert e_hip[k] <= 2 * max(e_ref[k], e_ref_g), (k, e_hip[k], e_ref[k], e_ref_g)
    for name, a, r, t in zip(("loss", "recon_loss", "kl_div"), got_l, ref_l, truth_l):
        assert abs(a - t) / abs(t) <= 2 * max(abs(r - t) / abs(t), e_ref_g), (name, a, r, t)
    if m.straight_through:
        assert ids.shape == (M,) and ids.dtype == torch.int64


def _noise_seq(steps, M, T):
    return [-torch.empty(M, T).exponential_(generator=torch.Generator().manual_seed(100 + t)).log() for t in range(steps)]


def test_training_reduces_the_loss_like_fp32_adam():
    """30 steps on one batch with a fixed noise sequence: engine.step(1e-3, max_norm=1e-3) against the fp32 restatement with
    torch.optim.Adam + clip_grad_norm_ -- the mean of the last five losses covers at least 90 % of the fp32 arm's descent."""
    from mem_amd.vae_train import DVAEEngine
    from oracle.vae_ref import TINY_VAE
    m = _module(TINY_VAE)
    B, temp, steps = 4, 0.9, 30
    M = B * (m.input_H >> m.num_layers) * (m.input_W >> m.num_layers)
    img = torch.rand(B, 3, m.input_H, m.input_W, generator=torch.Generator().manual_seed(3))
    noises = _noise_seq(steps, M, m.num_tokens)
    ref = copy.deepcopy(m)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    ref_losses = []
    for t in range(steps):
        opt.zero_grad()
        loss, _, _ = restated_loss(ref, img, temp, noises[t])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1e-3)
        opt.step()
        ref_losses.append(float(loss.detach()))
    eng = DVAEEngine(copy.deepcopy(m).cuda())
    losses = []
    imgd = img.cuda()
    for t in range(steps):
        loss, _, _ = eng.forward_backward(imgd, temp, noise=noises[t].cuda())
        eng.step(1e-3, max_norm=1e-3)
        losses.append(float(loss))
    L0, L_fp32, L_hip = ref_losses[0], sum(ref_losses[-5:]) / 5, sum(losses[-5:]) / 5
    print("fp32 %.4f -> %.4f   hip %.4f -> %.4f" % (L0, L_fp32, losses[0], L_hip))
    assert L_fp32 < L0
    assert L_hip <= L0 - 0.9 * (L0 - L_fp32)


def test_engine_step_is_clip_plus_adam():
    """One engine.step == clip_grad_norm_ + torch.optim.Adam.step on the same parameters and gradients (the bar of
    tests/test_kernels_gpu.py::test_grad_norm_and_adamw_match_torch); and the module's parameters ARE the masters."""
    from mem_amd.vae_train import DVAEEngine
    from oracle.vae_ref import TINY_VAE
    m = _module(TINY_VAE, num_resnet_blocks=0, input_H=32, input_W=32)
    eng = DVAEEngine(m.cuda())
    B = 2
    M = B * (m.input_H >> m.num_layers) * (m.input_W >> m.num_layers)
    img = torch.rand(B, 3, m.input_H, m.input_W, generator=torch.Generator().manual_seed(4)).cuda()
    eng.forward_backward(img, 0.9, noise=_noise_seq(1, M, m.num_tokens)[0].cuda())
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in m.parameters()]
    for c, p in zip(cpu, m.parameters()):
        c.grad = p.grad.detach().cpu().clone()
    want_norm = torch.linalg.vector_norm(torch.cat([c.grad.double().reshape(-1) for c in cpu])).float()
    torch.nn.utils.clip_grad_norm_(cpu, 1e-3)
    torch.optim.Adam(cpu, lr=1e-3).step()
    norm = eng.step(1e-3, max_norm=1e-3)
    torch.testing.assert_close(norm.cpu(), want_norm, rtol=1e-6, atol=0)
    for c, p in zip(cpu, m.parameters()):
        torch.testing.assert_close(p.detach().cpu(), c.detach(), rtol=2e-6, atol=2e-7)
    assert all(p.data_ptr() >= eng.master.data_ptr() and p.data_ptr() < eng.master.data_ptr() + eng.n * 4 for p in m.parameters())
    assert set(m.state_dict()) == set(_module(TINY_VAE, num_resnet_blocks=0, input_H=32, input_W=32).state_dict())


def test_a_torch_optimizer_with_zero_grad_keeps_working():
    """optimizer.zero_grad() sets every .grad to None by default: the next forward_backward binds the views of the flat gradient
    buffer again, and torch.optim.Adam then steps on the engine's gradients (the masters move)."""
    from mem_amd.vae_train import DVAEEngine
    from oracle.vae_ref import TINY_VAE
    m = _module(TINY_VAE, num_resnet_blocks=1, input_H=32, input_W=32)
    eng = DVAEEngine(m.cuda())
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    img = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(6)).cuda()
    noise = _noise_seq(1, 2 * 2 * 2, m.num_tokens)[0].cuda()
    eng.forward_backward(img, 0.9, noise=noise)
    first = eng.gflat.clone()
    opt.zero_grad()
    assert all(p.grad is None for p in m.parameters())
    eng.forward_backward(img, 0.9, noise=noise)
    assert torch.equal(eng.gflat, first)                           # the same step: the same bits
    lo, hi = eng.gflat.data_ptr(), eng.gflat.data_ptr() + 4 * eng.n
    assert all(p.grad is not None and lo <= p.grad.data_ptr() < hi for p in m.parameters())
    before = eng.master.clone()
    opt.step()
    assert not torch.equal(eng.master, before)


def test_vit_b_tokenizer_shape():
    """BASE_VAE (224 x 224, hidden 384, 8192 tokens), B = 2: one forward_backward; the loss and every gradient are finite and no
    gradient is identically zero.  (No float64 arm at this size.)"""
    from mem_amd.vae_train import DVAEEngine
    from oracle.vae_ref import BASE_VAE
    m = _module(BASE_VAE, kl_div_loss_weight=0.01)
    eng = DVAEEngine(m.cuda())
    img = torch.rand(2, 3, 224, 224, generator=torch.Generator().manual_seed(8)).cuda()
    loss, recon, kl = eng.forward_backward(img, 0.9)
    assert all(math.isfinite(float(v)) for v in (loss, recon, kl))
    for k, p in m.named_parameters():
        assert torch.isfinite(p.grad).all(), k
        assert float(p.grad.abs().max()) > 0, k
    again = eng.forward_backward(img, 0.9)
    assert all(math.isfinite(float(v)) for v in again)


def test_cli_round_trip(tmp_path):
    """Three steps of python -m mem_amd.train_vae on synthetic data; utils.create_d_vae loads the checkpoint; a bf16 HipTokenizer
    built from it returns the ids the engine's own encoder logits give by argmax; eval_tokenizer.evaluate runs on it."""
    from mem_amd import eval_tokenizer, utils
    from mem_amd.vae_model import HipTokenizer
    from mem_amd.vae_train import DVAEEngine
    out = str(tmp_path / "run")
    cmd = [sys.executable, "-m", "mem_amd.train_vae", "--data_path", "synthetic", "--output_dir", out, "--input_H", "32", "--input_W", "32",
           "--num_layers", "2", "--num_tokens", "128", "--emb_dim", "32", "--hidden_dim", "64", "--num_resnet_blocks", "1",
           "--batch_size", "4", "--epochs", "1", "--max_steps", "3", "--num_workers", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    path = os.path.join(out, "checkpoint-final.pt")
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) >= {"hparams", "epoch", "optimizer", "args", "weights"}
    steps = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"step"' in l]
    assert len(steps) == 3 and all(math.isfinite(s["loss"]) for s in steps)
    vae = utils.create_d_vae(weight_path=path, d_vae_type="event", device=torch.device("cuda"), image_size=(32, 32))
    img = torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    tok = HipTokenizer(vae.eval(), max_batch=4, precision="bf16")
    ids = tok.get_codebook_indices(img)
    eng = DVAEEngine(copy.deepcopy(vae).train())
    eng.forward_backward(img, 0.9)
    # the two encoders are the same kernels on the same packed weights: the same logits, bit for bit, and the tokenizer's ids are
    # an argmax of the engine's logits (bf16 rows can hold exact ties: compared by value, not by tie-breaking order)
    assert torch.equal(tok.logits[: ids.numel()], eng.logits)
    assert torch.equal(eng.logits.gather(1, ids.reshape(-1, 1))[:, 0], eng.logits.max(1).values)
    stats = eval_tokenizer.evaluate([(img, torch.zeros(4))], tok, torch.device("cuda"))
    assert all(math.isfinite(stats[k]) for k in ("loss", "recon_loss", "kl_div")) and 1 <= stats["codebook_indices"] <= 128
