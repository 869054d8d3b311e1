"""-m "not gpu": the host side of mem_amd.run_semseg: parameter groups (LayerDecayOptimizerConstructor, literally), the poly
schedule against its closed form, flag defaults, and every refusal."""
import math

import pytest
import torch

TINY = ["--vit", "tiny", "--embed_dim", "128", "--num_heads", "2", "--depth", "4", "--net_size", "64", "96", "--decode_channels", "64",
        "--aux_channels", "64", "--pool_scales", "1", "2", "3", "--necks", "torch"]


def _tiny_model():
    from mem_amd import run_semseg as R
    args = R.get_args(TINY)
    return R.build_model(args), args


def test_defaults_are_the_reference_config():
    from mem_amd import run_semseg as R
    a = R.get_args([])
    assert (a.embed_dim, a.num_heads, a.depth, a.out_indices, a.net_size) == (768, 12, 12, [8, 9, 10, 11], [512, 512])
    assert (a.drop, a.init_values, a.num_classes, a.decode_channels, a.aux_channels, a.pool_scales, a.aux_loss_weight) == \
        (0.1, 0.1, 11, 512, 256, [1, 2, 3, 6], 0.4)
    assert (a.lr, a.betas, a.weight_decay, a.layer_decay_rate, a.num_layers) == (5e-4, [0.9, 0.999], 0.05, 0.65, 12)
    assert (a.power, a.min_lr, a.warmup_iters, a.warmup_ratio, a.max_iters) == (1.0, 0.0, 1500, 1e-6, 160000)
    assert (a.checkpoint_interval, a.eval_interval, a.samples_per_gpu, a.workers_per_gpu) == (4501, 113, 16, 8)
    assert (a.canvas, a.crop_size, a.ratio_range, a.slice_max_evs, a.cat_max_ratio) == ([440, 640], [440, 640], [1.0, 1.01], 180000, 1.0)
    assert [R.get_args(["--vit", v]).embed_dim for v in ("base", "small", "tiny")] == [768, 384, 192]
    assert [R.get_args(["--vit", v]).num_heads for v in ("base", "small", "tiny")] == [12, 6, 3]


def test_model_is_the_reference_segmentor():
    from mem_amd.seg_heads import FCNHead, SegModel, UPerHead
    from mem_amd.semseg_backbone import EvBEiT
    m, args = _tiny_model()
    assert isinstance(m, SegModel) and isinstance(m.backbone, EvBEiT) and isinstance(m.decode_head, UPerHead) \
        and isinstance(m.auxiliary_head, FCNHead)
    assert m.backbone.out_indices == (0, 1, 2, 3) and m.backbone.pos_embed is None
    assert m.decode_head.in_index == (0, 1, 2, 3) and m.auxiliary_head.in_index == 2
    assert m.decode_head.loss_decode.loss_weight == 1.0 and m.auxiliary_head.loss_decode.loss_weight == 0.4
    assert m.decode_head.dropout_ratio == m.auxiliary_head.dropout_ratio == 0.1
    assert {k.split(".")[0] for k in m.state_dict()} == {"backbone", "decode_head", "auxiliary_head"}


def test_layer_decay_groups_are_the_constructors():
    from mem_amd import run_semseg as R
    m, args = _tiny_model()
    groups = R.layer_decay_groups(m, num_layers=4, layer_decay_rate=0.65, base_lr=5e-4, weight_decay=0.05)
    by_name = {n: g for g in groups for n in g["param_names"]}
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert sorted(by_name) == sorted(names) and sum(len(g["params"]) for g in groups) == len(names)
    params = dict(m.named_parameters())
    for g in groups:
        assert [id(p) for p in g["params"]] == [id(params[n]) for n in g["param_names"]]
        layer = int(g["group_name"].split("_")[1])
        assert g["lr_scale"] == 0.65 ** (5 - layer) and g["lr"] == g["lr_scale"] * 5e-4              # 4 + 2 = 6 ids: 0 .. 5
        assert g["weight_decay"] == (0.0 if g["group_name"].endswith("no_decay") else 0.05)
        assert set(g) == {"weight_decay", "params", "param_names", "lr_scale", "group_name", "lr"}

    def where(n):
        return by_name[n]["group_name"]
    # the embeddings: layer 0.  The constructor's `name in ('pos_embed', 'cls_token')` never matches under the prefix, so the
    # 3-d cls_token DOES decay
    assert where("backbone.cls_token") == "layer_0_decay" and params["backbone.cls_token"].ndim == 3
    assert where("backbone.patch_embed.proj.weight") == "layer_0_decay" and where("backbone.patch_embed.proj.bias") == "layer_0_no_decay"
    # block i: layer i + 1
    for i in range(4):
        assert where("backbone.blocks.%d.attn.qkv.weight" % i) == "layer_%d_decay" % (i + 1)
        assert where("backbone.blocks.%d.mlp.fc2.bias" % i) == "layer_%d_no_decay" % (i + 1)
        assert where("backbone.blocks.%d.gamma_1" % i) == "layer_%d_no_decay" % (i + 1)                 # ndim 1
        assert where("backbone.blocks.%d.attn.relative_position_bias_table" % i) == "layer_%d_decay" % (i + 1)
    # everything else, the necks and both heads: the last layer, scale 1
    assert where("backbone.fpn1.0.weight") == "layer_5_decay" and where("backbone.fpn1.1.weight") == "layer_5_no_decay"
    assert where("backbone.fpn2.0.bias") == "layer_5_no_decay"
    assert where("decode_head.conv_seg.weight") == "layer_5_decay" and where("decode_head.fpn_bottleneck.bn.weight") == "layer_5_no_decay"
    assert where("auxiliary_head.convs.0.conv.weight") == "layer_5_decay" and where("auxiliary_head.conv_seg.bias") == "layer_5_no_decay"
    assert by_name["decode_head.conv_seg.weight"]["lr_scale"] == 1.0
    # groups appear in the order of their first parameter
    firsts = [names.index(g["param_names"][0]) for g in groups]
    assert firsts == sorted(firsts)
    # the reference config: 14 ids, the last is 13
    assert R.get_num_layer_for_vit("backbone.blocks.11.mlp.fc1.weight", 14) == 12
    assert R.get_num_layer_for_vit("backbone.fpn4.weight", 14) == 13 and R.get_num_layer_for_vit("decode_head.x", 14) == 13
    assert R.get_num_layer_for_vit("backbone.pos_embed", 14) == 0 and R.get_num_layer_for_vit("backbone.mask_token", 14) == 0
    # a frozen parameter is in no group
    params["decode_head.conv_seg.bias"].requires_grad = False
    assert "decode_head.conv_seg.bias" not in {n for g in R.layer_decay_groups(m, 4) for n in g["param_names"]}


def _closed_form(base, i, max_iters=160000, power=1.0, min_lr=0.0, warmup_iters=1500, warmup_ratio=1e-6):
    regular = (base - min_lr) * (1 - i / max_iters) ** power + min_lr
    if i < warmup_iters:
        return regular * (1 - (1 - i / warmup_iters) * (1 - warmup_ratio))
    return regular


@pytest.mark.parametrize("base", [5e-4, 5e-4 * 0.65 ** 13])
def test_poly_schedule_against_the_closed_form(base):
    from mem_amd import run_semseg as R
    for i in (0, 1, 1499, 1500, 160000 - 1):
        got, want = R.poly_lr(base, i, 160000), _closed_form(base, i)
        assert math.isclose(got, want, rel_tol=1e-12), (i, got, want)
    # the warmup starts at ratio (1 - (1 - 1e-6) cancels: 2^-53 / 1e-6 = 1.1e-10 relative in the closed form itself)
    assert math.isclose(R.poly_lr(base, 0, 160000), base * 1e-6, rel_tol=1e-9)
    assert math.isclose(R.poly_lr(base, 1500, 160000), base * (1 - 1500 / 160000), rel_tol=1e-12)     # and ends on the poly line
    assert math.isclose(R.poly_lr(base, 159999, 160000), base / 160000, rel_tol=1e-9)
    assert R.poly_lr(base, 1499, 160000) < R.poly_lr(base, 1500, 160000)
    # power and min_lr
    got = R.poly_lr(1e-3, 3000, 10000, power=0.9, min_lr=1e-4, warmup_iters=0)
    assert math.isclose(got, (1e-3 - 1e-4) * 0.7 ** 0.9 + 1e-4, rel_tol=1e-12)


def test_set_lr_keeps_each_groups_base_value():
    from mem_amd import run_semseg as R

    class Opt:
        param_groups = [{"lr": 1e-3}, {"lr": 2e-4}]
    args = R.get_args(["--max_iters", "100", "--warmup_iters", "10"])
    for it in (0, 5, 10, 99):
        R.set_lr(Opt, it, args)
        assert [g["initial_lr"] for g in Opt.param_groups] == [1e-3, 2e-4]
        assert [g["lr"] for g in Opt.param_groups] == [_closed_form(b, it, 100, warmup_iters=10) for b in (1e-3, 2e-4)]


@pytest.mark.parametrize("argv, text", [
    (["--launcher", "pytorch"], "--launcher pytorch"),
    (["--launcher", "slurm"], "--launcher slurm"),
    (["--distributed"], "--distributed"),
    (["--world_size", "8"], "--world_size 8"),
    (["--gpus", "2"], "--gpus 2"),
    (["--deepspeed"], "--deepspeed"),
    (["--enable_deepspeed"], "--enable_deepspeed"),
    (["--aug-test"], "--aug_test"),
    (["--aug_test"], "--aug_test"),
    (["--test_mode", "slide"], "--test_mode slide"),
    (["--cat_max_ratio", "0.75"], "--cat_max_ratio 0.75"),
])
def test_refused_by_name(argv, text):
    from mem_amd import run_semseg as R
    with pytest.raises(NotImplementedError) as e:
        R.get_args(argv)
    assert text in str(e.value)


def test_eval_only_needs_a_checkpoint_and_unknown_flags_fail():
    from mem_amd import run_semseg as R
    with pytest.raises(SystemExit):
        R.get_args(["--no_such_flag"])
    with pytest.raises(SystemExit):
        R.get_args(["--vit", "large"])


def test_optimizer_halves_and_state_layout_on_stand_ins():
    """SegOptimizer's bookkeeping without a device: the flat half is replaced by a recorder, the torch half is real."""
    from mem_amd import optim_factory, run_semseg as R

    class FakeFlat:
        def __init__(self, model, groups, lr, betas, eps):
            self.param_groups = [dict(g) for g in groups]
            self.steps, self.calls = 0, []

        def zero_grad(self):
            self.calls.append("zero")

        def step(self):
            self.steps += 1
            self.calls.append(("step", [g["lr"] for g in self.param_groups]))

        def state_dict(self):
            ps = [p for g in self.param_groups for p in g["params"]]
            st = {i: {"step": torch.tensor(float(self.steps)), "exp_avg": torch.full_like(p, 1.0), "exp_avg_sq": torch.full_like(p, 2.0)}
                  for i, p in enumerate(ps)} if self.steps else {}
            return {"state": st, "param_groups": [{**{k: v for k, v in g.items() if k != "params"}, "params": []} for g in self.param_groups]}

        def load_state_dict(self, sd):
            self.loaded = sd

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = torch.nn.Linear(3, 2)
            self.decode_head = torch.nn.Linear(2, 2)
    m = M()
    groups = [{"params": [m.backbone.weight, m.decode_head.weight], "param_names": ["backbone.weight", "decode_head.weight"],
               "lr": 1e-3, "weight_decay": 0.0, "lr_scale": 1.0, "group_name": "layer_1_decay"},
              {"params": [m.backbone.bias], "param_names": ["backbone.bias"], "lr": 5e-4, "weight_decay": 0.0, "lr_scale": 0.5,
               "group_name": "layer_0_no_decay"},
              {"params": [m.decode_head.bias], "param_names": ["decode_head.bias"], "lr": 1e-3, "weight_decay": 0.0, "lr_scale": 1.0,
               "group_name": "layer_1_no_decay"}]
    real, optim_factory.FlatAdamW = optim_factory.FlatAdamW, FakeFlat
    try:
        opt = R.SegOptimizer(m, groups, lr=1e-3)
    finally:
        optim_factory.FlatAdamW = real
    assert [[id(p) for p in g["params"]] for g in opt.flat.param_groups] == [[id(m.backbone.weight)], [id(m.backbone.bias)]]
    assert [[id(p) for p in g["params"]] for g in opt.head.param_groups] == [[id(m.decode_head.weight)], [id(m.decode_head.bias)]]
    assert opt.head.defaults["betas"] == (0.9, 0.999)
    m.decode_head(m.backbone(torch.ones(1, 3))).sum().backward()
    opt.param_groups[0]["lr"], opt.param_groups[1]["lr"], opt.param_groups[2]["lr"] = 1e-4, 2e-4, 3e-4      # a schedule's writes
    before = m.decode_head.weight.detach().clone()
    opt.step()
    assert opt.flat.calls == [("step", [1e-4, 2e-4])] and [g["lr"] for g in opt.head.param_groups] == [1e-4, 3e-4]
    delta = (m.decode_head.weight.detach() - before).abs()
    # Adam's first step without decay: |dp| = lr (the weights are O(1): half an ulp of fp32 is 3e-8 = 3e-4 of the step)
    assert torch.allclose(delta[m.decode_head.weight.grad != 0], torch.tensor(1e-4), rtol=2e-3)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3]
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1], [2], [3]]
    assert sd["param_groups"][0]["param_names"] == ["backbone.weight", "decode_head.weight"] and sd["param_groups"][1]["lr"] == 2e-4
    assert float(sd["state"][0]["exp_avg"].mean()) == 1.0 and sd["state"][1]["exp_avg"].shape == m.decode_head.weight.shape
    assert float(sd["state"][1]["exp_avg"].abs().max()) > 0 and float(sd["state"][1]["exp_avg"].mean()) != 1.0
    opt.zero_grad()
    assert opt.flat.calls[-1] == "zero" and m.decode_head.weight.grad is None
    # and back
    sd["param_groups"][2]["lr"] = 7e-4
    opt.load_state_dict(sd)
    assert sorted(opt.flat.loaded["state"]) == [0, 1] and float(opt.flat.loaded["state"][1]["exp_avg_sq"].mean()) == 2.0
    assert opt.param_groups[2]["lr"] == 7e-4 and opt.head.param_groups[1]["lr"] == 7e-4
    assert torch.equal(opt.head.state[m.decode_head.weight]["exp_avg"], sd["state"][1]["exp_avg"])


def test_pretrained_backbone_loads_through_the_position_table_resampling(tmp_path):
    """a stage-3 style checkpoint ({"model": ...}, trained at 64 x 64 pixels: 4 x 4 windows) into a 96 x 96 backbone: tables
    are resampled to the 6 x 6 window, the classifier's keys are left out, the necks keep their initialisation"""
    from mem_amd import run_semseg as R
    from mem_amd.modeling_finetune import ft_vit
    src = ft_vit(img_size=(64, 64), patch_size=(16, 16), in_chans=3, embed_dim=128, depth=4, num_heads=2, num_classes=5,
                 use_rel_pos_bias=True, use_abs_pos_emb=False, init_values=0.1)
    path = str(tmp_path / "stage3.pth")
    torch.save({"model": src.state_dict()}, path)
    model = R.build_model(R.get_args(TINY + ["--net_size", "96", "96"]))
    before = model.backbone.fpn1[0].weight.detach().clone()
    R.load_pretrained(model.backbone, path)
    sd = model.backbone.state_dict()
    assert torch.equal(sd["blocks.2.mlp.fc1.weight"], src.state_dict()["blocks.2.mlp.fc1.weight"])
    assert torch.equal(sd["patch_embed.proj.weight"], src.state_dict()["patch_embed.proj.weight"])
    assert torch.equal(model.backbone.fpn1[0].weight.detach(), before)
    # the three extra rows (cls to token, token to cls, cls to cls) travel unchanged; the body is resampled, not copied
    old = src.state_dict()["blocks.0.attn.relative_position_bias_table"]
    assert old.shape[0] == 7 ** 2 + 3 and torch.equal(sd["blocks.0.attn.relative_position_bias_table"][-3:], old[-3:])
    assert sd["blocks.0.attn.relative_position_bias_table"].shape[0] == (2 * 6 - 1) ** 2 + 3
