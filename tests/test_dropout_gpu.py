"""-m gpu: element-wise dropout of the finetuning model on the HIP engine: the exported mask against the numpy restatement of
the contract, the residual-dropout GEMM epilogue on its dispatch rows, the dropout backward row kernels against float64, and
ft_vit(drop_rate > 0) against the reference model with the same masks."""
import numpy as np
import pytest
import torch

from test_dropout_cpu import keep_mask

pytestmark = pytest.mark.gpu


def _mask(d, row0, rows, cols):
    from mem_amd import ops
    out = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    ops.dropout_mask(d, row0, rows, cols, out)
    return out


def test_dropout_mask_matches_contract():
    from mem_amd import ops
    for (k0, k1, site, p, d_row0, row0, rows, cols) in [(0, 0, 0, 0.1, 0, 0, 64, 64), (0xDEADBEEF, 12345, 5, 0.1, 0, 7, 300, 768),
                                                         (1, 2, 24, 0.5, 1000, 3, 97, 128), (M := 0xFFFFFFFF, M, 3, 0.3, 0, 0, 16, 8)]:
        d = ops.dropout_params(k0, k1, site, p, d_row0)
        got = _mask(d, row0, rows, cols).cpu().numpy()
        want = keep_mask(k0, k1, site, p, d_row0 + row0, rows, cols)
        assert np.array_equal(got, want), (k0, k1, site, p)
    for p in (0.1, 0.5):
        m = _mask(ops.dropout_params(99, 7, 1, p), 0, 4096, 768).float()
        q = 1.0 - round(p * 65536) / 65536
        assert abs(m.mean().item() - q) <= 5 * np.sqrt(q * (1 - q) / m.numel()), (p, m.mean().item())
    assert bool(_mask(ops.dropout_params(3, 4, 0, 0.0), 0, 256, 256).all())


def test_dropout_rows_applies_the_mask():
    from mem_amd import ops
    x = torch.randn(333, 256, device="cuda")
    d = ops.dropout_params(11, 22, 4, 0.25, 17)
    want = x * _mask(d, 0, 333, 256).float() * d.scale
    ops.dropout_rows(d, x, 333, 256)
    assert torch.equal(x, want)


@pytest.mark.parametrize("shape", ["small_m", "k_not_128", "p8_whole_tiles", "p8_ragged_n768"])
@pytest.mark.parametrize("variant", ["plain", "gamma_inplace", "rowmask", "sample_map"])
def test_residual_dropout_epilogue(shape, variant):
    """EPI_RESIDUAL_DROP = the RESIDUAL arithmetic with y * mask * scale for y, on every dispatch row: small M (gemm_nt), K not
    a multiple of 128 (gemm256), whole 256-row tiles and a ragged N = 768 product (gemm_p8, 128-row form).  The restatement
    takes y from the same product with the BIAS_BF16 epilogue (same kernels, same accumulation) and the exported mask."""
    from mem_amd import ops
    M, N, K = {"small_m": (300, 256, 256), "k_not_128": (4096, 1024, 192), "p8_whole_tiles": (8192, 768, 768),
               "p8_ragged_n768": (24 * 197 * 2, 768, 768)}[shape]
    T = {"small_m": 20, "k_not_128": 128, "p8_whole_tiles": 128, "p8_ragged_n768": 197}[shape]
    g = torch.Generator(device="cuda").manual_seed(3)
    A = (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    Bw = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    gamma = (torch.rand(N, device="cuda", generator=g) + 0.5) if variant != "plain" else None
    x_in = torch.randn(M, N, device="cuda", generator=g)
    y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    ops.gemm_nt(A, Bw, M, N, K, ops.EPI_BIAS_BF16, out0=y, bias=bias)
    d = ops.dropout_params(0x1234, 0x9876, 7, 0.1, 5)
    nsamp = M // T
    keep = 0.8
    kw = {}
    rows_map = torch.arange(M, device="cuda")
    scale_row = torch.ones(M, 1, device="cuda")
    Mg = M
    if variant == "rowmask":
        rm = (torch.rand(nsamp, device="cuda", generator=g) > 0.3).float()
        kw = dict(rowmask=rm, keep_prob=keep, rows_per_sample=T)
        scale_row = (rm / keep).repeat_interleave(T)[:, None]
    if variant == "sample_map":
        kept = torch.nonzero(torch.rand(nsamp, device="cuda", generator=g) > 0.3).flatten().int()
        smap = torch.zeros((nsamp + 256,), dtype=torch.int32, device="cuda")
        smap[: kept.numel()] = kept
        Mg = kept.numel() * T
        rows_map = (kept.long()[:, None] * T + torch.arange(T, device="cuda")[None, :]).flatten()
        kw = dict(sample_map=smap, keep_prob=keep, rows_per_sample=T)
        scale_row = torch.full((Mg, 1), 1.0 / keep, device="cuda")
        # y of the compact rows = the GEMM of the gathered A rows
        A = A[rows_map].contiguous()
        ops.gemm_nt(A, Bw, Mg, N, K, ops.EPI_BIAS_BF16, out0=y, bias=bias)
    inplace = variant in ("gamma_inplace",)
    mask = _mask(d, 0, M, N).float()
    z = y[:Mg].float() * (mask[rows_map] * d.scale)
    t = z * gamma if gamma is not None else z
    t = t * scale_row if variant == "rowmask" else (t / keep if variant == "sample_map" else t)
    want = x_in.clone()
    want[rows_map] = x_in[rows_map] + t
    resid = x_in.clone() if inplace else torch.zeros_like(x_in)
    ops.gemm_nt(A, Bw, Mg, N, K, ops.EPI_RESIDUAL_DROP, resid=resid, aux=None if inplace else x_in,
                ldaux=None if inplace else N, bias=bias, vec1=gamma, dropout=d, **kw)
    err = (resid[rows_map] - want[rows_map]).abs().max().item()
    ref = want[rows_map].abs().max().item()
    print("%s/%s: max |diff| %.3e of max %.3e" % (shape, variant, err, ref))
    assert err <= 2e-6 * ref, (err, ref)       # fp32 round-off (reassociation of the division in the restatement)


@pytest.mark.parametrize("form", ["branch", "branch_map", "ln_branch"])
def test_dropout_backward_row_kernels(form):
    """dy = bf16(dt * keep * scale * gamma), dbias = sum dy against float64 autograd of the forward x + drop_path(gamma * z)."""
    from mem_amd import ops
    T, B, D = 197, 6, 768
    M = B * T
    g = torch.Generator(device="cuda").manual_seed(9)
    dx = torch.randn(M, D, device="cuda", generator=g)
    gamma = torch.rand(D, device="cuda", generator=g) + 0.5
    d = ops.dropout_params(77, 88, 3, 0.1)
    mask = _mask(d, 0, M, D).double()
    dy = torch.zeros(M, D, dtype=torch.bfloat16, device="cuda")
    dbias = torch.zeros(D, device="cuda")
    out_rows = torch.arange(M, device="cuda")
    if form == "branch":
        ops.branch_bwd(dx, None, gamma, dy, None, dbias, M, D, rows_per_sample=T, dropout=d)
        dt = dx.double()
    elif form == "branch_map":
        cmap = torch.tensor([0, -1, 1, 2, -1, 3], dtype=torch.int32, device="cuda")
        ops.branch_bwd(dx, None, gamma, dy, None, dbias, M, D, keep_prob=0.75, rows_per_sample=T, out_map=cmap, dropout=d)
        kept = torch.tensor([0, 2, 3, 5], device="cuda")
        out_rows = (kept[:, None] * T + torch.arange(T, device="cuda")[None, :]).flatten()
        dt = dx.double() / 0.75
    else:
        x = torch.randn(M, D, device="cuda", generator=g)
        lw, lb = torch.rand(D, device="cuda", generator=g) + 0.5, torch.randn(D, device="cuda", generator=g) * 0.1
        mean, rstd = x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-6)
        dyl = (torch.randn(M, D, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
        dres = dx.clone()
        dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        ops.layernorm_bwd_branch(dyl, x, lw, mean, rstd, dres, dg, db, M, D, None, gamma, dy, None, dbias, rows_per_sample=T,
                                 dropout=d)
        xd = x.double().requires_grad_(True)
        yln = torch.nn.functional.layer_norm(xd, (D,), lw.double(), lb.double(), 1e-6)
        (gx,) = torch.autograd.grad(yln, xd, dyl.double())
        dt = dx.double() + gx
        assert torch.allclose(dres.double(), dt, rtol=1e-5, atol=1e-5)
    # forward: x + gamma * (y * mask * scale) (/ keep): d/dy = dt * mask * scale * gamma
    rows = out_rows if form == "branch_map" else torch.arange(M, device="cuda")
    want = dt[rows] * mask[rows] * d.scale * gamma.double()
    got = dy[: rows.numel()].double()
    rel = ((got - want).norm() / want.norm()).item()
    assert rel <= 3e-3, rel                                        # bf16 rounding of dy
    assert ((got == 0) == (want == 0)).all()
    dbw = got.sum(0)
    assert torch.allclose(dbias.double(), dbw, rtol=1e-4, atol=1e-3)


def _ref_with_masks(cfg, sd, x, key, p, depth, T, D):
    """oracle.vit_ref.RefFtViT in fp32 with the engine's masks injected: pos_drop as a forward-pre-hook of blocks[0], the
    branch masks as forward hooks of blk.attn / blk.mlp (before gamma and drop path, as the reference's proj_drop / Mlp.drop)."""
    from mem_amd import ops
    from oracle.vit_ref import RefFtViT
    o = RefFtViT(**cfg)
    o.load_state_dict(sd)
    B = x.shape[0]

    def mk(site):
        d = ops.dropout_params(key[0], key[1], site, p)
        return (_mask(d, 0, B * T, D).float() * d.scale).cpu().view(B, T, D)
    o.blocks[0].register_forward_pre_hook(lambda m, a, mm=mk(2 * depth): (a[0] * mm,) + tuple(a[1:]))
    for i, blk in enumerate(o.blocks):
        blk.attn.register_forward_hook(lambda m, a, out, mm=mk(2 * i): out * mm)
        blk.mlp.register_forward_hook(lambda m, a, out, mm=mk(2 * i + 1): out * mm)
    return o


@pytest.mark.parametrize("tag", ["a", "b", "big"])
def test_finetune_dropout_vs_reference(tag):
    """ft_vit(drop_rate=0.1) on the engine against the fp32 reference with the same masks: logits, per-parameter gradients
    (gamma_1 / gamma_2 included) and the flat cosine, at the bars of test_finetune_model_vs_reference_golden."""
    from mem_amd.modeling_finetune import ft_vit
    from oracle.gen_golden_ft import FT_A, FT_B, ft_inputs
    from oracle.vit_ref import fill_by_name
    if tag == "big":
        cfg = dict(FT_A, img_size=(224, 224), embed_dim=768, depth=2, num_heads=12)
        B = 24
    else:
        cfg = FT_A if tag == "a" else FT_B
        B = 5
    m = ft_vit(**dict(cfg, drop_rate=0.1))
    sd = fill_by_name(m.state_dict(), seed=5)
    m.load_state_dict(sd)
    m = m.cuda().train()
    x, y = ft_inputs(cfg, B, 31)
    lo = m(x.cuda())
    eng = m.engine
    key = eng.cur["drop_key"]
    assert key is not None
    loss = torch.nn.CrossEntropyLoss()(lo.float(), y.cuda())
    loss.backward()
    o = _ref_with_masks(cfg, sd, x, key, 0.1, len(m.blocks), eng.T, eng.D)
    lr = o(x)
    torch.nn.CrossEntropyLoss()(lr, y).backward()
    assert (lo.float().cpu() - lr.detach()).abs().max().item() <= 0.03
    ref = dict(o.named_parameters())
    flat_g, flat_r = [], []
    for k, p in m.named_parameters():
        r = ref[k].grad
        rel = ((p.grad.cpu() - r).norm() / (r.norm() + 1e-12)).item()
        assert rel <= 4e-2, (k, rel)
        flat_g.append(p.grad.flatten().cpu())
        flat_r.append(r.flatten())
    cos = torch.nn.functional.cosine_similarity(torch.cat(flat_g), torch.cat(flat_r), dim=0).item()
    assert cos >= 0.999, cos


@pytest.mark.parametrize("fuse", [True, False])
def test_dropout_work_skipping_equals_masked_and_two_streams(fuse):
    """With dropout on: work-skipping drop path = masked drop path (same residual stream, gradients to split-order noise), and
    the two-stream forward split = the one-stream forward (bit-equal)."""
    from mem_amd.modeling_finetune import ft_vit
    from oracle.gen_golden_ft import FT_A, ft_inputs
    from oracle.vit_ref import fill_by_name
    cfg = dict(FT_A, img_size=(224, 224), embed_dim=768, depth=2, num_heads=12, drop_path_rate=0.2, drop_rate=0.1)
    B = 160                                    # (the two-stream split needs a second part of >= 4096 rows)
    x, y = ft_inputs(cfg, B, 7)
    masks = (torch.rand(4, B, generator=torch.Generator().manual_seed(2)) > 0.3).float()
    res = {}
    for mode in ("masked", "skip", "two"):
        m = ft_vit(**cfg)
        m.load_state_dict(fill_by_name(m.state_dict(), seed=3))
        m = m.cuda().train()
        eng = m.engine
        eng.dp_skip = mode == "skip"
        eng.fuse_ln_branch = fuse
        eng.fwd_two_streams = mode == "two"
        m._dp_stream = None
        from mem_amd.utils import DropPathStream
        m._dp_stream = DropPathStream()
        m._dp_stream.seed(5)
        lo = m(x.cuda(), drop_path_masks=masks if mode == "skip" else masks.cuda())
        torch.nn.CrossEntropyLoss()(lo.float(), y.cuda()).backward()
        torch.cuda.synchronize()
        assert (eng.cur["plan"] is not None) == (mode == "skip")
        res[mode] = (eng.x[2 * 2][: B * eng.T].clone(), torch.cat([p.grad.flatten() for p in m.parameters()]), eng.cur["drop_key"])
        del m, eng
    (x0, g0, k0), (x1, g1, k1), (x2, g2, k2) = res["masked"], res["skip"], res["two"]
    assert k0 == k1 == k2
    assert torch.equal(x0, x1)
    assert torch.equal(x0, x2)
    cos = (torch.dot(g0, g1) / (g0.norm() * g1.norm())).item()
    assert cos >= 0.99999, cos
    assert ((g0 - g1).norm() / g0.norm()).item() <= 2e-3


def test_dropout_eval_and_key_reproduction():
    """eval() applies no dropout (logits bit-equal to a drop_rate = 0 model with the same weights); restoring the drop-path
    stream reproduces the step's key and its logits; the next step draws another key."""
    from mem_amd.modeling_finetune import ft_vit
    from mem_amd.utils import DropPathStream
    from oracle.gen_golden_ft import FT_A, ft_inputs
    from oracle.vit_ref import fill_by_name
    m1 = ft_vit(**dict(FT_A, drop_rate=0.1))
    sd = fill_by_name(m1.state_dict(), seed=4)
    m1.load_state_dict(sd)
    m0 = ft_vit(**FT_A)
    m0.load_state_dict(sd)
    m0, m1 = m0.cuda().eval(), m1.cuda().eval()
    x, y = ft_inputs(FT_A, 6, 3)
    with torch.no_grad():
        assert torch.equal(m0(x.cuda()), m1(x.cuda()))
    m1.train()
    m1._dp_stream = DropPathStream()
    m1._dp_stream.seed(11)
    st = m1._dp_stream.state()
    lo_a = m1(x.cuda()).float()
    ka = m1.engine.cur["drop_key"]
    m1._dp_stream.load_state(st)
    lo_b = m1(x.cuda()).float()
    assert m1.engine.cur["drop_key"] == ka
    assert torch.equal(lo_a, lo_b)
    lo_c = m1(x.cuda()).float()
    assert m1.engine.cur["drop_key"] != ka and not torch.equal(lo_a, lo_c)
