"""-m gpu: mem_amd.run_semseg on the device: one optimizer step of both halves of SegOptimizer against Adam's first step, and
a short training / evaluation / resume / eval-only run on the synthetic source."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# the 128-wide configuration the head tests use, on a 48 x 64 canvas; 96 x 128 pixels: the coarsest map is 3 x 4, what
# pool scale 3 needs
TINY = ["--vit", "tiny", "--embed_dim", "128", "--num_heads", "2", "--depth", "4", "--net_size", "96", "128", "--decode_channels", "64",
        "--aux_channels", "64", "--pool_scales", "1", "2", "3", "--canvas", "48", "64", "--crop_size", "48", "64",
        "--ratio_range", "1.0", "1.05", "--slice_max_evs", "5000", "--synthetic_samples", "8", "--synthetic_events", "8000",
        "--workers_per_gpu", "0", "--samples_per_gpu", "2", "--log_interval", "1"]


def test_one_step_moves_every_element_by_its_groups_lr():
    """Weight decay 0, one step: Adam's first step is lr g / (|g| + eps), so for every element with |g| > 1e-6 the move
    |dp| equals lr |g| / (|g| + eps) of ITS group within 1e-3 relative (eps / |g| is up to 1e-2 at the smallest gradients
    taken, so the factor is kept in the expected value).  This checks name -> layer -> lr on the device for the flat half
    (trunk and necks, memhip_adamw_groups) and for the torch half (the heads).  Base lr 1e-2: the smallest group lr is
    1e-2 * 0.65^5 = 1.2e-3, so half an ulp of an fp32 weight of size 1 (3e-8) is 3e-5 of the step.  The loss is scaled by 2^12
    for the backward: Adam's first step does not depend on the gradient's scale, and a freshly initialised model (classifier
    weights of std 0.01, LayerScale 0.1) leaves the blocks' gradients below the 1e-6 the check starts at."""
    from mem_amd import run_semseg as R
    args = R.get_args(TINY + ["--drop", "0.0"])
    torch.manual_seed(3)
    model = R.build_model(args).cuda().train()
    model.backbone.engine
    base_lr, eps = 1e-2, 1e-8
    groups = R.layer_decay_groups(model, args.num_layers, 0.65, base_lr, weight_decay=0.0)
    assert len({g["lr"] for g in groups}) == 6
    opt = R.SegOptimizer(model, groups, lr=base_lr, betas=(0.9, 0.999), eps=eps)
    g = torch.Generator().manual_seed(5)
    img = (torch.rand((2, 3, 96, 128), generator=g) * 255).cuda()
    label = torch.randint(0, 11, (2, 48, 64), generator=g, dtype=torch.uint8).cuda()
    opt.zero_grad()
    losses = model.forward_train(img, label)
    loss = sum(v.float() for k, v in losses.items() if "loss" in k)
    assert set(losses) == {"decode.loss_seg", "decode.acc_seg", "aux.loss_seg", "aux.acc_seg"} and math.isfinite(float(loss.detach()))
    (loss * 4096.0).backward()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    grads = {n: p.grad.detach().clone().float() for n, p in model.named_parameters() if p.grad is not None}
    opt.step()
    torch.cuda.synchronize()
    after = dict(model.named_parameters())
    checked = {}
    worst = (0.0, None)
    for grp in opt.param_groups:
        for n in grp["param_names"]:
            if n not in grads:
                continue
            gr = grads[n].double()
            mask = gr.abs() > 1e-6
            if not bool(mask.any()):
                continue
            want = grp["lr"] * gr.abs() / (gr.abs() + eps)
            got = (after[n].detach().double() - before[n].double()).abs()
            rel = ((got - want).abs() / want)[mask]
            assert bool(((after[n].detach().double() - before[n].double()) * gr)[mask].max() < 0), n      # against the gradient
            if float(rel.max()) > worst[0]:
                worst = (float(rel.max()), n)
            assert float(rel.max()) <= 1e-3, (n, grp["group_name"], float(rel.max()))
            half = "flat" if n.startswith("backbone.") else "torch"
            checked[(grp["group_name"], half)] = checked.get((grp["group_name"], half), 0) + int(mask.sum())
    print("largest |dp| error / expected %.3e (%s); elements checked per group: %s" % (worst[0], worst[1], checked))
    # every layer of the trunk, the necks and both heads took part
    names = {k[0] for k in checked}
    assert {"layer_%d_decay" % i for i in range(6)} <= names and {"layer_%d_no_decay" % i for i in range(1, 6)} <= names
    assert checked[("layer_5_decay", "flat")] > 0 and checked[("layer_5_decay", "torch")] > 0
    moved = [n for n in grads if n.startswith(("decode_head.", "auxiliary_head.")) and not torch.equal(after[n].detach(), before[n])]
    assert len(moved) >= 30


def test_training_evaluation_resume_and_eval_only(tmp_path, capsys):
    from mem_amd import run_semseg as R
    work = str(tmp_path / "work")
    common = TINY + ["--data_root", "synthetic", "--work_dir", work, "--warmup_iters", "2", "--seed", "1"]
    out = R.main(R.get_args(common + ["--max_iters", "6", "--eval_interval", "3"]))
    # losses are finite, one record per iteration
    assert [r["iter"] for r in out["train"]] == [1, 2, 3, 4, 5, 6]
    for r in out["train"]:
        assert all(math.isfinite(r[k]) for k in ("loss", "decode.loss_seg", "aux.loss_seg", "decode.acc_seg", "aux.acc_seg")), r
        assert math.isclose(r["loss"], r["decode.loss_seg"] + r["aux.loss_seg"], rel_tol=1e-5)
        assert math.isclose(r["lr"], R.poly_lr(5e-4, r["iter"] - 1, 6, warmup_iters=2), rel_tol=1e-12)
    # the evaluation lines: at iterations 3 and 6, with the metric keys, printed as JSON
    assert [r["iter"] for r in out["eval"]] == [3, 6]
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{"iter"') and "mIoU" in l]
    assert len(printed) == 2
    for r in printed:
        assert {"aAcc", "mIoU", "mAcc", "IoU"} <= set(r) and len(r["IoU"]) == 11 and 0.0 <= r["mIoU"] <= 1.0 and 0.0 <= r["aAcc"] <= 1.0
    # the checkpoint: mmseg's layout and keys, strict load into a fresh model
    assert out["checkpoints"] == [work + "/iter_6.pth"]
    ckpt = torch.load(out["checkpoints"][0], map_location="cpu", weights_only=False)
    assert set(ckpt) == {"meta", "state_dict", "optimizer"} and ckpt["meta"]["iter"] == 6
    assert {k.split(".")[0] for k in ckpt["state_dict"]} == {"backbone", "decode_head", "auxiliary_head"}
    fresh = R.build_model(R.get_args(common))
    fresh.load_state_dict(ckpt["state_dict"], strict=True)
    opt_sd = ckpt["optimizer"]
    n_params = sum(1 for p in fresh.parameters() if p.requires_grad)
    assert sum(len(g["params"]) for g in opt_sd["param_groups"]) == n_params
    assert all({"param_names", "lr_scale", "group_name", "initial_lr", "lr", "weight_decay"} <= set(g) for g in opt_sd["param_groups"])
    assert all(float(st["step"]) == 6.0 for st in opt_sd["state"].values()) and len(opt_sd["state"]) > 0.9 * n_params
    # --resume continues at iteration 6 with the schedule's lr for that iteration
    more = R.main(R.get_args(common + ["--max_iters", "8", "--eval_interval", "100", "--resume", out["checkpoints"][0]]))
    assert [r["iter"] for r in more["train"]] == [7, 8] and more["iter"] == 8
    assert math.isclose(more["train"][0]["lr"], R.poly_lr(5e-4, 6, 8, warmup_iters=2), rel_tol=1e-12)
    assert all(math.isfinite(r["loss"]) for r in more["train"])
    again = torch.load(more["checkpoints"][-1], map_location="cpu", weights_only=False)
    assert again["meta"]["iter"] == 8 and all(float(st["step"]) == 8.0 for st in again["optimizer"]["state"].values())
    assert not torch.equal(again["meta"]["drop_path_rng"], ckpt["meta"]["drop_path_rng"])                # the mask stream moved on
    # --eval_only on the checkpoint repeats the last mIoU exactly
    only = R.main(R.get_args(common + ["--eval_only", "--resume", out["checkpoints"][0]]))
    assert only["train"] == [] and only["eval"][0]["iter"] == 6
    assert only["eval"][0]["mIoU"] == out["eval"][-1]["mIoU"] and only["eval"][0]["IoU"] == out["eval"][-1]["IoU"]
    with pytest.raises(ValueError, match="--eval_only needs --resume"):
        R.main(R.get_args(common + ["--eval_only"]))
