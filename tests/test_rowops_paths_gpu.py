"""-m gpu: the code paths of the pipelined row kernels (rowops.hip) at the smallest shapes that reach them.

The row loops of layernorm_bwd_branch / layernorm_bwd / branch_bwd walk only the rows that take full part, keep the sample
and the offset of a row by increments (stride = q * rps + rem), request a row one step ahead and let the wave's last row
request itself again; rows of samples that one branch dropped go through a second pass.  Widths that are a multiple of 256
run guard-free instantiations, the others a guarded one.  What can go wrong there is a row skipped, done twice, sent to
the wrong compact row, or a lane past the width touched: the exact layouts of test_rowops_gpu.py (bit-equal to float64
whatever the grid, NaN canaries on everything that must stay unwritten) show each of these, so this file reuses them at
  widths 256, 768, 1024 (guard-free), 260, 320 (ragged last chunk: one lane, a quarter wave), 128 (less than a chunk),
  rows per sample 1, 5, 197 (and 4, the one at which a stride can EQUAL rps) x samples 1, 2, 9: R from 1 to 1773, below four
  waves, not a multiple of 4, stride (4 x grid) above R (the default grid), a multiple of rps and equal to rps (forced
  through ln_bwd_grid),
  sample maps with the first / the last sample dropped by one branch, the other, both; two consecutive samples dropped by
  both; the last row of the launch in a dropped sample; in_map alone, out_map alone, no map.
Bars are those of test_rowops_gpu.py: exact layouts bit for bit; random rows 2^-18 of their scale (fp32), one bf16 ulp
(bf16), column sums 2^-14 of sum |terms|."""
import pytest
import torch

import test_rowops_gpu as T

pytestmark = pytest.mark.gpu

WIDTHS = [256, 768, 1024, 260, 320, 128]
SHAPES = [(B, rps) for rps in (1, 5, 197) for B in (1, 2, 9)] + [(9, 4)]


def _grids(R, rps):
    """1, 7, the shipped value (stride >= R for these R), and the grids whose stride 4 * grid is rps or a multiple of it"""
    gs = [1, 7, None]
    if rps % 4 == 0:
        gs.append(rps // 4)                                  # stride == rps
    gs.append(rps)                                           # stride == 4 * rps
    return gs


def _patterns(B):
    """name -> (kept by the LayerNorm'ed branch, kept by the output branch); None = no map"""
    one = lambda: torch.ones(B, dtype=torch.bool, device="cuda")

    def drop(idx):
        k = one()
        k[[i for i in idx if 0 <= i < B]] = False
        return k
    ends, mid, last = [0, B - 1], [B // 2 - 1, B // 2], [B - 1]
    pats = {
        "no_map": (None, None),
        "in_only": (drop(ends), None),
        "out_only": (None, drop(ends)),
        "ends_in": (drop(ends), one()),
        "ends_out": (one(), drop(ends)),
        "ends_both": (drop(ends), drop(ends)),
        "two_consecutive_both": (drop(mid), drop(mid)),
        "last_both": (drop(last), drop(last)),
        "crossed": (drop([0] + mid), drop(mid + last)),      # a row of every kind next to one of another kind
    }
    if B < 3:                                                # with one or two samples the patterns coincide
        pats = {k: pats[k] for k in ("no_map", "in_only", "out_only", "ends_out", "last_both")}
    return pats


def _fused_case(D, B, rps, pat, exact, seed, monkeypatch):
    monkeypatch.setattr(T, "_sample_patterns", lambda B_, mode, g: pat)
    return T._lnb_case(D, B, rps, "paths", exact, seed)


@pytest.mark.parametrize("D", WIDTHS)
def test_fused_backward_paths_exact(D, monkeypatch):
    """layernorm_bwd_branch, exact layout: bit-equal to float64 on every grid, row outputs the same bits across grids,
    canaries intact."""
    for B, rps in SHAPES:
        for pi, (name, pat) in enumerate(_patterns(B).items()):
            c = _fused_case(D, B, rps, pat, True, 7000 + 13 * pi + B + rps, monkeypatch)
            T._exact_sums_fit(torch.stack(c["sums_abs"]))
            R, Ro, lv = c["R"], c["Ro"], c["live"]
            first = None
            for gr in _grids(R, rps):
                with T._Grid(gr):
                    dres, dyo, accs = T._lnb_run(c)
                what = (D, B, rps, name, gr)
                assert torch.equal(dres[:R, :D][lv].double(), c["dres_exp"][lv]), (what, "dres")
                assert torch.equal(dyo[:Ro, :D].double(), c["dyo_exp"]), (what, "dy of the branch")
                assert torch.equal(accs[0][:D].double(), c["exp"][0]), (what, "dgamma")
                assert torch.equal(accs[1][:D].double(), c["exp"][1]), (what, "dbeta")
                assert torch.equal(accs[3][:D].double(), c["acc0"][3] + dyo[:Ro, :D].double().sum(0)), (what, "dbias")
                T._lnb_canaries(c, dres, dyo, accs)
                bits = (T._bits(dres).clone(), T._bits(dyo).clone())
                if first is None:
                    first = bits
                else:
                    assert torch.equal(bits[0], first[0]) and torch.equal(bits[1], first[1]), (what, "bits across grids")


@pytest.mark.parametrize("D", [768, 260])
def test_fused_backward_paths_random(D, monkeypatch):
    """layernorm_bwd_branch, random values against float64 at the largest of the small shapes (both passes, every grid)."""
    B, rps = 9, 197
    for pi, name in enumerate(("crossed", "ends_both", "no_map")):
        c = _fused_case(D, B, rps, _patterns(B)[name], False, 7100 + pi, monkeypatch)
        R, Ro, lv = c["R"], c["Ro"], c["live"]
        for gr in _grids(R, rps):
            with T._Grid(gr):
                dres, dyo, accs = T._lnb_run(c)
            print("layernorm_bwd_branch D=%d %s grid %s" % (D, name, gr))
            T._check_bar(dres[:R, :D][lv], c["dres_exp"][lv], c["dres_sc"][lv], 18, "dres")
            T._check_bf16(dyo[:Ro, :D], c["dyo_exp"], c["dyo_sc"] * 2.0 ** -18, "dy of the branch")
            T._check_bar(accs[0][:D], c["exp"][0], c["sums_abs"][0], 14, "dgamma")
            T._check_bar(accs[1][:D], c["exp"][1], c["sums_abs"][1], 14, "dbeta")
            T._lnb_canaries(c, dres, dyo, accs)


@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_bwd_and_branch_bwd_paths(D):
    """layernorm_bwd (row_idx and identity, accumulate 0 and 1, grids 1 / 7 / shipped) and branch_bwd (rowmask, y, out_map
    mixed / all / none) through the checks of test_rowops_gpu.py, at R = 2 .. 1773 (their sample patterns need two samples)."""
    for B, rps in [(2, 1), (9, 1), (2, 5), (9, 5), (2, 197), (9, 197)]:
        T.test_layernorm_bwd(D, B, rps, True)
        T.test_branch_bwd(D, B, rps, True)
    T.test_layernorm_bwd(D, 9, 197, False)
    T.test_branch_bwd(D, 9, 197, False)


def test_single_row_backward():
    """R = 1 (one wave of one workgroup has a row, and it is the last): layernorm_bwd and branch_bwd."""
    from mem_amd import ops
    for D in (768, 260):
        g = T._gen(7200 + D)
        dy, x, gamma, mean, rstd = T._ln_inputs(1, D, g, True)
        d, xh, _ = T._ln_ref(dy, x, gamma, mean, rstd)
        prev = T._ri(-4, 4, (1, D), g)
        for acc in (1, 0):
            dres0 = T._canvas(3, D + 8, torch.float32)
            if acc:
                dres0[0, :D] = prev[0].float()
            dres = dres0.clone()
            dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
            ops.layernorm_bwd(dy.bfloat16().contiguous(), x.float().contiguous(), gamma.float(), mean.float(), rstd.float(), dres,
                              dg, db, 1, D, accumulate=bool(acc))
            torch.cuda.synchronize()
            assert torch.equal(dres[0, :D].double(), (d + prev if acc else d)[0]), (D, acc)
            assert torch.equal(dg.double(), (dy * xh).sum(0)) and torch.equal(db.double(), dy.sum(0)), (D, acc)
            w = torch.zeros(dres.shape, dtype=torch.bool, device="cuda")
            w[0, :D] = True
            assert T._untouched(dres, dres0, w) == 0
        dx = T._ri(-16, 16, (1, D), g)
        gam = T._pow2(-1, 1, (D,), g, signed=True)
        dyo0 = T._canvas(3, D + 12, torch.bfloat16)
        dyo, dbias = dyo0.clone(), torch.zeros(D, device="cuda")
        ops.branch_bwd(dx.float().contiguous(), None, gam.float(), dyo, None, dbias, 1, D)
        torch.cuda.synchronize()
        assert torch.equal(dyo[0, :D].double(), (dx * gam)[0]), D
        assert torch.equal(dbias.double(), (dx * gam)[0]), D
        w = torch.zeros(dyo.shape, dtype=torch.bool, device="cuda")
        w[0, :D] = True
        assert T._untouched(dyo, dyo0, w) == 0


# ------------------------------------------------------------------------------------------------ layernorm_fwd
def _fwd_run(x_d, ridx, R, D, gamma, beta, eps):
    from mem_amd import ops
    ldy = D + 12
    y0 = T._canvas(R + 2, ldy, torch.bfloat16)
    m0, r0 = T._canvas(1, R + 4, torch.float32)[0], T._canvas(1, R + 4, torch.float32)[0]
    y, mean, rstd = y0.clone(), m0.clone(), r0.clone()
    ops.layernorm_fwd(x_d, gamma.float(), beta.float(), y, mean, rstd, R, D, eps=eps, row_idx=ridx)
    torch.cuda.synchronize()
    w = torch.zeros(y.shape, dtype=torch.bool, device="cuda")
    w[:R, :D] = True
    assert T._untouched(y, y0, w) == 0, "y written into ld padding or past row R"
    assert torch.equal(T._bits(mean[R:]), T._bits(m0[R:])) and torch.equal(T._bits(rstd[R:]), T._bits(r0[R:]))
    return y[:R, :D], mean[:R], rstd[:R]


def _row_orders(R, Rsrc, g):
    """None (identity), a row_idx that repeats a row, one in descending order"""
    rep = torch.randint(0, Rsrc, (R,), generator=g, device="cuda").int()
    rep[R // 2] = rep[0]
    desc = torch.arange(Rsrc - 1, Rsrc - 1 - R, -1, device="cuda").int()
    return [("identity", None), ("repeat", rep), ("descending", desc)]


@pytest.mark.parametrize("D", [128, 260, 768, 2048])
def test_layernorm_fwd_paths(D):
    """Exact layout: x = mean +- 2^k (half the columns each sign), so mean is an integer and var = 4^k exactly; eps = 3 * 4^k
    makes var + eps = 4^(k+1) and rstd = 2^-(k+1) exact in any order of operations; gamma a power of two, beta a small integer:
    y, mean and rstd must equal float64 bit for bit.  Then random rows against float64."""
    for R in (1, 3, 4, 5, 1773):
        g = T._gen(7300 + D + R)
        Rsrc = R + 3
        k = 1
        mean = T._ri(-8, 8, (Rsrc,), g)
        sign = torch.ones(D, dtype=torch.float64, device="cuda")
        sign[torch.randperm(D, generator=g, device="cuda")[: D // 2]] = -1.0
        x = mean[:, None] + sign[None, :] * 2.0 ** k
        gamma, beta = T._pow2(-1, 1, (D,), g, signed=True), T._ri(-3, 3, (D,), g)
        eps = 3.0 * 4.0 ** k
        x_d = T._canvas(Rsrc + 1, D + 4, torch.float32)
        x_d[:Rsrc, :D] = x.float()
        for name, ridx in _row_orders(R, Rsrc, g):
            src = torch.arange(R, device="cuda") if ridx is None else ridx.long()
            y, mu, rs = _fwd_run(x_d, ridx, R, D, gamma, beta, eps)
            what = (D, R, name)
            assert torch.equal(mu.double(), mean[src]), (what, "mean")
            assert torch.equal(rs.double(), torch.full((R,), 2.0 ** -(k + 1), dtype=torch.float64, device="cuda")), (what, "rstd")
            assert torch.equal(y.double(), T._bf((x[src] - mean[src][:, None]) * 2.0 ** -(k + 1) * gamma + beta)), (what, "y")
        # random rows
        xr = (0.5 + T._randn((Rsrc, D), g, 2.0) + T._randn((Rsrc, 1), g)).float().double()
        gam, bet = (1 + T._randn((D,), g, 0.1)).float().double(), T._randn((D,), g, 0.1).float().double()
        x_d[:Rsrc, :D] = xr.float()
        for name, ridx in _row_orders(R, Rsrc, g):
            src = torch.arange(R, device="cuda") if ridx is None else ridx.long()
            y, mu, rs = _fwd_run(x_d, ridx, R, D, gam, bet, 1e-6)
            xs = xr[src]
            m64 = xs.mean(1)
            v64 = xs.var(1, unbiased=False)
            r64 = 1.0 / torch.sqrt(v64 + 1e-6)
            print("layernorm_fwd D=%d R=%d %s" % (D, R, name))
            T._check_bar(mu, m64, xs.abs().mean(1), 18, "mean")
            T._check_bar(rs, r64, r64, 18, "rstd")
            xh = (xs - m64[:, None]) * r64[:, None]
            ref = xh * gam + bet
            # the fp32 error of xhat * gamma + beta ahead of the bf16 rounding: 2^-18 of (|xhat| + rstd * mean|x|) |gamma| + |beta|
            extra = ((xh.abs() + (r64 * xs.abs().mean(1))[:, None]) * gam.abs() + bet.abs()) * 2.0 ** -18
            T._check_bf16(y, ref, extra, "y")
