"""-m gpu: dense per-block feature maps on the device -- memhip_tokens_to_maps / memhip_maps_to_tokens_add bit-exact against
the torch expressions they replace, the engine's exports against its own snapshots (keep=True / keep=False, drop path in
both forms, dropout, the two-stream split), forward_dense and its backward against the fp32 reference arithmetic
(oracle.vit_ref.RefFtViT with forward hooks on its blocks), and the segmentation backbone end to end."""
import contextlib
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, Hp, Wp, D, ldx): one tile and less, D tiles x a padded leading dimension, ViT-B geometry (4 ragged token tiles x 12),
# 1200 tokens (19 token tiles, the last ragged); and 5 x 5 = 25 tokens: not a multiple of 4, the map side's 4-byte path
SHAPES = [(1, 4, 6, 64, 64), (3, 4, 6, 128, 192), (2, 14, 14, 768, 768), (2, 30, 40, 128, 128), (2, 5, 5, 64, 96)]
GUARD = 256


def _ranges(B):
    return [(0, B)] + ([(1, B)] if B > 1 else [])


def _guarded(n, fill):
    """n floats between two guard bands of GUARD NaNs; `fill` makes the n values."""
    big = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    big[GUARD:GUARD + n] = fill(n)
    return big, big[GUARD:GUARD + n]


@pytest.mark.parametrize("B,Hp,Wp,D,ldx", SHAPES)
def test_tokens_to_maps_bit_exact(B, Hp, Wp, D, ldx):
    from mem_amd import ops
    L = Hp * Wp
    T = L + 1
    g = torch.Generator().manual_seed(B * 1000 + L + D)
    xb = torch.randn((B * T, ldx), generator=g).cuda()
    want = xb.view(B, T, ldx)[:, 1:, :D].permute(0, 2, 1)
    for b0, b1 in _ranges(B):
        big, out = _guarded(B * D * L, lambda n: torch.full((n,), float("nan"), device="cuda"))
        out = out.view(B, D, L)
        ops.tokens_to_maps(xb[:, :D], B, T, out=out, b0=b0, b1=b1)
        assert torch.equal(out[b0:b1], want[b0:b1])
        assert torch.isnan(out[:b0]).all() and torch.isnan(out[b1:]).all()            # samples outside the range
        assert torch.isnan(big[:GUARD]).all() and torch.isnan(big[-GUARD:]).all()      # the guard bands


@pytest.mark.parametrize("B,Hp,Wp,D,ldx", SHAPES)
def test_maps_to_tokens_add_bit_exact(B, Hp, Wp, D, ldx):
    from mem_amd import ops
    L = Hp * Wp
    T = L + 1
    g = torch.Generator().manual_seed(B * 1000 + L + D + 1)
    dmap = torch.randn((B, D, Hp, Wp), generator=g).cuda()
    dx0 = torch.randn((B * T, ldx), generator=g).cuda()
    for b0, b1 in _ranges(B):
        big, dxf = _guarded(B * T * ldx, lambda n: dx0.flatten())
        dx = dxf.view(B * T, ldx)
        ops.maps_to_tokens_add(dmap, dx[:, :D], B, T, b0=b0, b1=b1)
        want = dx0.clone().view(B, T, ldx)
        want[b0:b1, 1:, :D] = dx0.view(B, T, ldx)[b0:b1, 1:, :D] + dmap.flatten(2).transpose(1, 2)[b0:b1]   # one fp32 add
        got = dx.view(B, T, ldx)
        assert torch.equal(got, want)
        # (spelled out: cls rows, the columns behind D and the samples outside the range keep their bits)
        assert torch.equal(got[:, 0], dx0.view(B, T, ldx)[:, 0]) and torch.equal(got[:, :, D:], dx0.view(B, T, ldx)[:, :, D:])
        assert torch.equal(got[:b0], dx0.view(B, T, ldx)[:b0]) and torch.equal(got[b1:], dx0.view(B, T, ldx)[b1:])
        assert torch.isnan(big[:GUARD]).all() and torch.isnan(big[-GUARD:]).all()


def test_dense_entries_reject_bad_arguments():
    """D % 64 != 0, T < 2, a leading dimension below D and null pointers: MEMHIP_EINVAL with a message, nothing launched."""
    from mem_amd import _lib, ops  # noqa: F401
    lib = _lib.lib
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()

    def bad(rc, word):
        assert rc == -1, rc
        assert word.encode() in lib.memhip_last_error(), lib.memhip_last_error()
    bad(lib.memhip_tokens_to_maps(p, 96, 0, 2, 5, 96, p, None), "bad shape")
    bad(lib.memhip_tokens_to_maps(p, 64, 0, 2, 1, 64, p, None), "bad shape")
    bad(lib.memhip_tokens_to_maps(p, 32, 0, 2, 5, 64, p, None), "ldx=")
    bad(lib.memhip_tokens_to_maps(None, 64, 0, 2, 5, 64, p, None), "null pointer")
    bad(lib.memhip_tokens_to_maps(p, 64, 0, 2, 5, 64, None, None), "null pointer")
    bad(lib.memhip_maps_to_tokens_add(p, 0, 2, 5, 96, p, 96, None), "bad shape")
    bad(lib.memhip_maps_to_tokens_add(p, 0, 2, 1, 64, p, 64, None), "bad shape")
    bad(lib.memhip_maps_to_tokens_add(p, 0, 2, 5, 64, p, 32, None), "lddx=")
    bad(lib.memhip_maps_to_tokens_add(None, 0, 2, 5, 64, p, 64, None), "null pointer")
    bad(lib.memhip_maps_to_tokens_add(p, 0, 2, 5, 64, None, 64, None), "null pointer")
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- engine consistency
def _cfgs():
    from oracle.gen_golden_ft import FT_A, FT_B
    big = dict(FT_A, img_size=(224, 224), embed_dim=768, depth=2, num_heads=12)
    return dict(a=FT_A, b=FT_B, big=big)


def _idx(cfg):
    """A non-final index and the last block."""
    return (cfg["depth"] - 2, cfg["depth"] - 1)


def _model(cfg, seed=5):
    from mem_amd.modeling_finetune import ft_vit
    from oracle.vit_ref import fill_by_name
    m = ft_vit(**cfg)
    sd = fill_by_name(m.state_dict(), seed=seed)
    m.load_state_dict(sd)
    return m.cuda(), sd


def _snap_maps(eng, B, idx):
    """The engine's own snapshots of the blocks' outputs (keep=True), as maps."""
    return [eng.cur["x"][2 * i + 2][: B * eng.T].view(B, eng.T, eng.D)[:, 1:].permute(0, 2, 1).reshape(B, eng.D, *eng.window).clone()
            for i in idx]


def _seed_stream(m, seed):
    from mem_amd.utils import DropPathStream
    m._dp_stream = DropPathStream()
    m._dp_stream.seed(seed)


@pytest.mark.parametrize("tag", ["a", "big"])
@pytest.mark.parametrize("mode", ["plain", "skip", "masked"])
def test_forward_dense_equals_the_engines_snapshots(tag, mode):
    """train(): the keep=True maps are the engine's snapshots x[2i + 2] transposed, and the forward-only (keep=False) maps
    are the same bits -- plain, and with dropout + drop path in the work-skipping and the masked form."""
    from oracle.gen_golden_ft import ft_inputs
    cfg = _cfgs()[tag]
    if mode != "plain":
        cfg = dict(cfg, drop_path_rate=0.2, drop_rate=0.1)
    B, idx = 8, _idx(cfg)
    m, _ = _model(cfg)
    m.train()
    eng = m.engine
    eng.dp_skip = mode == "skip"
    x, _ = ft_inputs(cfg, B, 7)
    masks = None
    if mode != "plain":
        masks = (torch.rand(2 * cfg["depth"], B, generator=torch.Generator().manual_seed(2)) > 0.3).float()
        masks = masks if mode == "skip" else masks.cuda()
    _seed_stream(m, 5)
    maps = m.forward_dense(x.cuda(), idx, drop_path_masks=masks)
    assert eng.cur["keep"] and (eng.cur["plan"] is not None) == (mode == "skip")
    assert (eng.cur["drop_key"] is not None) == (mode != "plain")
    key = eng.cur["drop_key"]
    assert all(mp.shape == (B, eng.D, *eng.window) and mp.dtype == torch.float32 and mp.requires_grad for mp in maps)
    want = _snap_maps(eng, B, idx)
    got = [mp.detach().clone() for mp in maps]
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    _seed_stream(m, 5)
    with torch.no_grad():
        maps2 = m.forward_dense(x.cuda(), idx, drop_path_masks=masks)
    assert not eng.cur["keep"] and eng.cur["drop_key"] == key
    for g, w in zip(maps2, want):
        assert torch.equal(g, w)
    if mode != "plain":                                     # the draws were live: the maps differ from the eval() ones
        m.eval()
        assert not torch.equal(m.forward_dense(x.cuda(), idx)[0], want[0])


def test_forward_dense_two_stream_split_exports_each_half():
    """B = 160 at ViT-B width: the second part of the split (>= 4096 rows) exports its own samples on its own stream."""
    from oracle.gen_golden_ft import ft_inputs
    cfg = dict(_cfgs()["big"], drop_rate=0.1)
    B, idx = 160, (0, 1)
    m, _ = _model(cfg, seed=3)
    m.train()
    eng = m.engine
    x, _ = ft_inputs(cfg, B, 7)
    res = {}
    for two in (False, True):
        eng.fwd_two_streams = two
        assert (0 < eng._split_point(B) < B)
        for keep in (True, False):
            _seed_stream(m, 5)
            with contextlib.nullcontext() if keep else torch.no_grad():
                maps = m.forward_dense(x.cuda(), idx)
            torch.cuda.synchronize()
            assert eng.cur["keep"] == keep
            res[two, keep] = [mp.detach().clone() for mp in maps]
            if keep:
                for g, w in zip(res[two, keep], _snap_maps(eng, B, idx)):
                    assert torch.equal(g, w)
    for k in ((False, False), (True, True), (True, False)):
        for g, w in zip(res[k], res[False, True]):
            assert torch.equal(g, w)


@pytest.mark.parametrize("tag", ["a", "big"])
def test_intermediate_layers_and_logits_around_a_dense_call(tag):
    """get_intermediate_layers = the keep=True snapshots, cls row included (eval() and no_grad both run forward-only), and
    forward(x) gives the same logits before and after a forward_dense call on the same model."""
    from oracle.gen_golden_ft import ft_inputs
    cfg = _cfgs()[tag]
    B = 8
    m, _ = _model(cfg)
    eng = m.engine
    x, _ = ft_inputs(cfg, B, 11)
    xc = x.cuda()
    m.eval()
    with torch.no_grad():
        lo0 = m(xc).clone()
    m.train()                                               # (no drop path, no dropout in these configs: train() = eval() bits)
    m.forward_dense(xc, _idx(cfg))
    assert eng.cur["keep"]
    snaps = [eng.cur["x"][2 * i + 2][: B * eng.T].view(B, eng.T, eng.D).clone() for i in range(eng.depth)]
    m.eval()
    feats = m.get_intermediate_layers(xc)
    assert not eng.cur["keep"] and len(feats) == eng.depth
    for f, s in zip(feats, snaps):
        assert f.shape == (B, eng.T, eng.D) and torch.equal(f, s)
    m.train()
    with torch.no_grad():
        feats2 = m.get_intermediate_layers(xc)
    for f, s in zip(feats2, snaps):
        assert torch.equal(f, s)
    m.eval()
    with torch.no_grad():
        maps = m.forward_dense(xc, _idx(cfg))
        assert torch.equal(maps[-1], snaps[-1][:, 1:].permute(0, 2, 1).reshape(maps[-1].shape))
        assert torch.equal(m(xc), lo0)


# ---------------------------------------------------------------------------------------------- against the reference


def _reference(cfg, sd, x, idx, R, only=None):
    """oracle.vit_ref.RefFtViT in fp32, forward hooks on its blocks; loss = sum_k <map_k, R_k> over `only` (default: idx)."""
    from oracle.vit_ref import RefFtViT
    o = RefFtViT(**cfg)
    o.load_state_dict(sd)
    outs = {}
    for i, blk in enumerate(o.blocks):
        blk.register_forward_hook(lambda mod, a, out, i=i: outs.__setitem__(i, out))
    o(x)
    B = x.shape[0]
    maps = [outs[i][:, 1:].permute(0, 2, 1).reshape(B, cfg["embed_dim"], *o.patch_embed.patch_shape) for i in idx]
    loss = sum((mp * r).sum() for mp, r, i in zip(maps, R, idx) if only is None or i in only)
    loss.backward()
    return o, [mp.detach() for mp in maps]


def _compare_grads(m, o, names):
    ref = dict(o.named_parameters())
    flat_g, flat_r = [], []
    for k, p in m.named_parameters():
        if k not in names:
            continue
        r = ref[k].grad
        rel = ((p.grad.cpu() - r).norm() / (r.norm() + 1e-12)).item()
        print("  grad %-50s rel %.3e" % (k, rel))
        assert rel <= 4e-2, (k, rel)
        flat_g.append(p.grad.flatten().cpu())
        flat_r.append(r.flatten())
    cos = torch.nn.functional.cosine_similarity(torch.cat(flat_g).double(), torch.cat(flat_r).double(), dim=0).item()
    print("  flat cosine %.6f" % cos)
    assert cos >= 0.999, cos


def _trunk_names(m):
    return [k for k, _ in m.named_parameters() if not k.startswith(("head.", "fc_norm.", "norm."))]


@pytest.mark.parametrize("tag", ["a", "b", "big"])
def test_forward_dense_vs_reference(tag):
    """forward_dense on the engine against the fp32 reference: loss = sum_k <map_k, R_k> with fixed random R_k over a
    non-final block and the last one; per-parameter gradient relative error <= 4e-2 and flat cosine >= 0.999 over the trunk
    (the bars of test_finetune_dropout_vs_reference; head, fc_norm and the final norm take no part).  The maps themselves:
    relative L2 error per map against the fp32 oracle (bf16 GEMM operands, fp32 residual stream: a measurement, not a
    derivation); the bar is 3 x the largest value measured on MI355X over the three configurations.
    Measured (block: error): FT_A 1: 2.874e-3, 2: 2.921e-3; FT_B 1: 5.039e-3, 2: 5.329e-3; 224^2 / D 768 / depth 2
    0: 2.933e-3, 1: 3.076e-3.  Largest 5.329e-3, bar 1.599e-2."""
    from oracle.gen_golden_ft import ft_inputs
    cfg = _cfgs()[tag]
    B, idx = (8 if tag == "big" else 5), _idx(cfg)
    m, sd = _model(cfg)
    m.train()
    eng = m.engine
    x, _ = ft_inputs(cfg, B, 31)
    g = torch.Generator().manual_seed(17)
    R = [torch.randn((B, cfg["embed_dim"], *eng.window), generator=g) for _ in idx]
    maps = m.forward_dense(x.cuda(), idx)
    sum((mp * r.cuda()).sum() for mp, r in zip(maps, R)).backward()
    got = [mp.detach().cpu() for mp in maps]
    o, want = _reference(cfg, sd, x, idx, R)
    rels = [((gm - wm).norm() / wm.norm()).item() for gm, wm in zip(got, want)]
    for i, rel in zip(idx, rels):
        print("config %s block %d: map relative L2 error %.3e" % (tag, i, rel))
    _compare_grads(m, o, _trunk_names(m))
    assert max(rels) <= MAP_BAR, (idx, rels)


def test_gradient_at_one_intermediate_index_only():
    """Only the map of block 0 of FT_A (depth 3) carries a gradient (the last block's map arrives as None and is skipped):
    blocks 1 and 2 get exactly zero gradients, block 0 and the embedding the reference's."""
    from oracle.gen_golden_ft import ft_inputs
    cfg = _cfgs()["a"]
    B, idx = 5, (0, 2)
    m, sd = _model(cfg)
    m.train()
    eng = m.engine
    x, _ = ft_inputs(cfg, B, 31)
    g = torch.Generator().manual_seed(17)
    R = [torch.randn((B, cfg["embed_dim"], *eng.window), generator=g) for _ in idx]
    maps = m.forward_dense(x.cuda(), idx)
    (maps[0] * R[0].cuda()).sum().backward()
    later = [k for k in _trunk_names(m) if k.startswith(("blocks.1.", "blocks.2."))]
    assert later
    for k, p in m.named_parameters():
        if k in later:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    o, _ = _reference(cfg, sd, x, idx, R, only=(0,))
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for k, p in o.named_parameters() if k in later)
    _compare_grads(m, o, [k for k in _trunk_names(m) if k not in later])


# ---------------------------------------------------------------------------------------------- the segmentation backbone
def test_evbeit_shapes_and_one_training_step():
    from mem_amd import optim_factory as OF
    from mem_amd.semseg_backbone import EvBEiT
    from oracle.gen_golden_ft import ft_inputs
    from oracle.vit_ref import fill_by_name
    cfg = dict(img_size=(64, 96), patch_size=16, in_chans=3, embed_dim=128, depth=4, num_heads=2, out_indices=(0, 1, 2, 3),
               use_rel_pos_bias=True, use_abs_pos_emb=False, init_values=0.1, drop_path_rate=0.1)
    m = EvBEiT(**cfg)
    trunk = {k: v for k, v in m.state_dict().items() if not k.startswith("fpn")}
    m.load_state_dict(fill_by_name(trunk, seed=5), strict=False)
    m = m.cuda().train()
    B, D, Hp, Wp = 4, 128, 4, 6
    x, _ = ft_inputs(dict(in_chans=3, img_size=(64, 96), num_classes=2), B, 3)
    with contextlib.redirect_stdout(io.StringIO()):
        groups = OF.get_parameter_groups(m, 0.05, m.no_weight_decay())
    opt = OF.FlatAdamW(m, groups, lr=1e-3)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    outs = m(x.cuda())
    assert [tuple(o.shape) for o in outs] == [(B, D, 4 * Hp, 4 * Wp), (B, D, 2 * Hp, 2 * Wp), (B, D, Hp, Wp), (B, D, Hp // 2, Wp // 2)]
    sum(o.float().square().mean() for o in outs).backward()
    opt.step()
    torch.cuda.synchronize()
    moved = {k: not torch.equal(p.detach(), before[k]) for k, p in m.named_parameters()}
    assert all(torch.isfinite(p).all() for p in m.parameters())
    for k in ("fpn1.0.weight", "fpn1.1.weight", "fpn1.3.bias", "fpn2.0.weight", "patch_embed.proj.weight", "cls_token",
              "blocks.0.attn.qkv.weight", "blocks.3.mlp.fc2.weight", "blocks.3.gamma_2", "blocks.1.attn.relative_position_bias_table"):
        assert moved[k], k
    m.eval()
    with torch.no_grad():
        outs = m(x.cuda())
    assert [tuple(o.shape) for o in outs][0] == (B, D, 4 * Hp, 4 * Wp) and all(torch.isfinite(o).all() for o in outs)


MAP_BAR = 3 * 5.329e-3   # 3 x the largest measured map error (docstring of test_forward_dense_vs_reference)
