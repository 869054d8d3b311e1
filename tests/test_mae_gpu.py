"""-m gpu: the MAE variant (mem_amd/modeling_mae.py -> csrc/fp32_path.hip: fp32 GEMMs, generic attention with 64- and
32-wide heads, token gather / mask-token un-shuffle, per-patch MSE loss) against the REFERENCE's MaskedAutoencoderViT
(tests/golden/mae_tiny.npz, oracle/gen_golden_mae.py: fp32 CPU, timm Block / PatchEmbed restated): same-seed weights
equal, loss 2e-6 rel, pred 2e-5, mask equal, every gradient rel-L2 <= 2e-5; both loss modes; the bf16 engine
(mem_amd/mae_engine.py) against the reference under autocast; a short training run through engine_for_pretraining.train_one_epoch(MAE=True); the ViT-B MAE factory shapes.
Reference: mem/modeling_mae.py:101-313, mem/run_mem_pretraining.py:231-232,275-276, mem/engine_for_pretraining.py:141-149."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _tiny(mode, seed=3, precision="fp32"):
    from mem_amd.modeling_mae import MaskedAutoencoderViT
    from oracle.mae_ref import TINY_MAE
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(seed)
        m = MaskedAutoencoderViT(**dict(TINY_MAE, LOSS_ONLY_MASKED_MAE=mode))
    m.precision = precision
    return m


def _check_bf16(m, g, tag, imgs, noise, sample, grad_tol, pred_tol):
    loss, img, mask = m(imgs.cuda(), noise=noise.cuda())
    ref_loss = float(g[f"{tag}__loss"])
    assert abs(loss.item() / ref_loss - 1) <= 5e-3, (loss.item(), ref_loss)
    assert np.array_equal(mask.cpu().numpy(), g[f"{tag}__mask"])
    pred = m.patchify(img).cpu().numpy()[:, :24]
    assert np.abs(pred - g[f"{tag}__pred_head"]).max() <= pred_tol, np.abs(pred - g[f"{tag}__pred_head"]).max()
    m.forward_loss(imgs.cuda(), noise=noise.cuda())
    m.backward()
    worst, dot, n1, n2, checked = (0.0, ""), 0.0, 0.0, 0.0, 0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        ref = torch.from_numpy(g[f"{tag}__grad__{k}"]).cuda()
        got = sample(p.grad).float()
        assert got.shape == ref.shape, k
        rel = ((got - ref).norm() / (ref.norm() + 1e-20)).item()
        worst = max(worst, (rel, k))
        assert rel <= grad_tol, (k, rel)
        gn, rn = p.grad.double().norm().item(), float(g[f"{tag}__gnorm__{k}"])
        assert abs(gn / rn - 1) <= 3e-2, (k, gn, rn)
        dot += float((got.double() * ref.double()).sum()); n1 += float((got.double() ** 2).sum()); n2 += float((ref.double() ** 2).sum())
        checked += 1
    cos = dot / (n1 * n2) ** 0.5
    print("MAE bf16 %s: loss %.6f (reference %.6f), worst gradient rel-L2 %.3e (%s), pooled cosine %.6f, %d tensors"
          % (tag, loss.item(), ref_loss, worst[0], worst[1], cos, checked))
    assert cos >= 0.9995
    return checked


@pytest.mark.parametrize("fuse", [True, False])
def test_mae_bf16_tiny_vs_reference_autocast_golden(fuse):
    """f4 on the fast path: the bf16 MFMA engine (what `--mae 1` trains with) against the REFERENCE MaskedAutoencoderViT under
    bf16 autocast (tests/golden/mae_bf16.npz, oracle/gen_golden_mae.py), tiny config (2-wide decoder heads of 32: the
    padded-head path; every gradient whole; two blocks per stack: all three positions of the fused LayerNorm backward), with
    the LayerNorm backward fused into the branch backward (FUSE_LN_BRANCH, the default) and in the two-kernel form: one
    golden, one set of bars.  Loss 5e-3 rel, prediction, mask equal, every gradient rel-L2 <= 3e-2 (VERDICT bar), per-tensor
    norms 3 %, pooled cosine >= 0.9995."""
    from oracle.gen_golden_mae import sample
    from oracle.mae_ref import TINY_MAE, mae_inputs
    g = np.load(os.path.join(GOLDEN, "mae_bf16.npz"))
    m = _tiny(True, precision="bf16").cuda().train()
    assert type(m.engine).__name__ == "MaeEngineBF16"
    m.engine.FUSE_LN_BRANCH = fuse                               # on the instance: nothing global to restore
    imgs, noise = mae_inputs(TINY_MAE, 4, 21)
    assert _check_bf16(m, g, "tiny", imgs, noise, sample, 3e-2, 0.03) >= 40


def test_mae_bf16_engine_vs_reference_autocast_golden():
    """The same against the ViT-B factory at B = 2 (12 x 768 encoder on 99 tokens, 8 x 512 decoder with 16 heads of 32 on 197
    tokens; loss, a block of the prediction, every gradient's norm, small gradients whole, big ones on every 32nd row), same
    bars; the padded head slots stay exact zeros."""
    from mem_amd.modeling_mae import mae_vit_base_patch16_dec512d8b
    from oracle.gen_golden_mae import BASE_MAE_B, sample
    from oracle.mae_ref import mae_inputs
    g = np.load(os.path.join(GOLDEN, "mae_bf16.npz"))
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(3)
        b = mae_vit_base_patch16_dec512d8b(norm_pix_loss=0, LOSS_ONLY_MASKED_MAE=True, img_size=224)
    assert b.precision == "bf16"
    b = b.cuda().train()
    assert type(b.engine).__name__ == "MaeEngineBF16"
    cfg = dict(img_size=224, patch_size=16)
    imgs, noise = mae_inputs(cfg, BASE_MAE_B, 33)
    assert _check_bf16(b, g, "base", imgs, noise, sample, 3e-2, 0.05) >= 200
    # padded head slots stay exact zeros end to end (decoder: 16 heads of 32 in 64-wide slots)
    qkv = b.engine.da["a"][0]["qkv"][: BASE_MAE_B * 197].view(-1, 3, 16, 64)
    assert float(qkv[..., 32:].abs().max()) == 0.0 and float(qkv[..., :32].abs().max()) > 0.0


@pytest.mark.parametrize("mode", [True, False])
def test_mae_tiny_vs_reference_golden(mode):
    from oracle.mae_ref import TINY_MAE, RefMAE, mae_inputs
    g = np.load(os.path.join(GOLDEN, "mae_tiny.npz"))
    tag = "masked" if mode else "all"
    m = _tiny(mode)
    assert list(m.state_dict().keys()) == list(g["keys"])
    torch.manual_seed(3)
    ora = RefMAE(**dict(TINY_MAE, LOSS_ONLY_MASKED_MAE=mode))          # same seed -> same initial weights as the reference
    for (k, a), (_, b) in zip(m.state_dict().items(), ora.state_dict().items()):
        assert torch.equal(a, b), k
    m = m.cuda().train()
    imgs, noise = mae_inputs(TINY_MAE, 4, 21)
    loss, img, mask = m(imgs.cuda(), noise=noise.cuda())
    assert abs(loss.item() / float(g[f"{tag}__loss"]) - 1) <= 2e-6, (loss.item(), float(g[f"{tag}__loss"]))
    assert np.array_equal(mask.cpu().numpy(), g[f"{tag}__mask"])
    assert np.abs(m.patchify(img).cpu().numpy() - g[f"{tag}__pred"]).max() <= 2e-5
    m.forward_loss(imgs.cuda(), noise=noise.cuda())
    m.backward()
    checked = 0
    for k, p in m.named_parameters():
        key = f"{tag}__grad__{k}"
        if key not in g.files:
            continue
        ref = torch.from_numpy(g[key]).cuda()
        rel = ((p.grad - ref).norm() / (ref.norm() + 1e-20)).item()
        assert rel <= 2e-5, (k, rel)
        checked += 1
    assert checked >= (40 if mode else 5)
    assert m.pos_embed.grad is None and not m.pos_embed.requires_grad


def test_mae_training_loop_and_factory(tmp_path):
    """train_one_epoch(MAE=True) on a small model: loss decreases; the base factory has the reference's shapes."""
    from mem_amd import engine_for_pretraining as E
    from mem_amd.modeling_mae import mae_vit_base_patch16_dec512d8b
    from mem_amd.optim_factory import create_optimizer
    from mem_amd.utils import NativeScalerWithGradNormCount
    m = _tiny(True, precision="bf16").cuda()

    class A:
        opt = "adamw"; weight_decay = 0.05; lr = 1e-3; opt_eps = 1e-8; opt_betas = [0.9, 0.999]; momentum = 0.9
    with contextlib.redirect_stdout(io.StringIO()):
        opt = create_optimizer(A(), m)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(8, 3, 64, 64, generator=g)
    batches = [((x, x, torch.zeros(8, 4, 4, dtype=torch.int64)), 0)] * 40
    lr = np.full(40, 1e-3)
    with contextlib.redirect_stdout(io.StringIO()):
        stats = E.train_one_epoch(m, None, batches[:20], opt, torch.device("cuda"), 0, NativeScalerWithGradNormCount(), 1.0,
                                  lr_schedule_values=lr, start_steps=0, MAE=True)
        stats2 = E.train_one_epoch(m, None, batches[20:], opt, torch.device("cuda"), 1, NativeScalerWithGradNormCount(), 1.0,
                                   lr_schedule_values=lr, start_steps=20, MAE=True)
        ev = E.evaluate(batches[:2], m, None, torch.device("cuda"), None, MAE=True)
    assert np.isfinite(stats["loss"]) and stats2["loss"] < stats["loss"] and stats["mlm_acc"] == 0
    assert np.isfinite(ev["loss"])
    with contextlib.redirect_stdout(io.StringIO()):
        b = mae_vit_base_patch16_dec512d8b(norm_pix_loss=0, LOSS_ONLY_MASKED_MAE=True)
    sd = b.state_dict()
    assert sd["pos_embed"].shape == (1, 197, 768) and sd["decoder_pos_embed"].shape == (1, 197, 512)
    assert sd["decoder_blocks.7.attn.qkv.weight"].shape == (1536, 512) and sd["decoder_pred.weight"].shape == (768, 512)
    assert len(b.blocks) == 12 and b.decoder_blocks[0].attn.num_heads == 16 and b.norm.eps == 1e-6


def test_cli_mae_flag(tmp_path):
    """`--mae 1` through the entrypoint (run_mem_pretraining.py:231-232,275-276): ViT-B MAE factory on 112^2 synthetic
    event frames, one short epoch + eval, checkpoint and log written."""
    import json
    from mem_amd.run_mem_pretraining import get_args, main
    out = tmp_path / "run"
    out.mkdir()
    args = get_args(["--expweek", "t", "--mae", "1", "--data_path", "synthetic", "--input_H", "112", "--input_W", "112",
                     "--batch_size", "4", "--epochs", "1", "--warmup_epochs", "0", "--synthetic_samples", "8",
                     "--num_workers", "0", "--output_dir", str(out), "--color_jitter", "0", "--rand_aug", "0",
                     "--slice_max_evs", "5000", "--clip_grad", "3.0"])
    main(args)
    log = [json.loads(l) for l in open(out / "log.txt")]
    assert len(log) == 1 and np.isfinite(log[0]["train_loss"]) and log[0]["train_mlm_acc"] == 0
    sd = torch.load(next(p for p in out.iterdir() if p.name.startswith("checkpoint-")), map_location="cpu", weights_only=False)
    assert "decoder_blocks.7.mlp.fc2.weight" in sd["model"] and "pos_embed" in sd["model"]
