"""-m "not gpu": the optimizer tail's float64 reference (step_tail_ref.py) checked against itself, and the argument
validation of the step-tail entry points.

  (a) the bound covers the arithmetic and no more: a numpy fp32 restatement of adamw_kernel's operation order (numpy
      rounds every fp32 operation to nearest, no contraction) stays within 1.0 x the bound on every input family and step
      the GPU test uses, clipped and unclipped;
  (b) the bound has teeth: five plausible wrong formulas, evaluated in float64, leave it by more than 10 x on more than
      1 % of the elements of at least one family -- and all five do so at step 1 of the small-gradient family, where eps
      is visible next to sqrt(v): that family is why the GPU test can tell them apart;
  (c) the entry points refuse bad arguments before any launch (no GPU here), and return OK on empty work."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_tail_ref as R

N = 1024 * 8
F32 = np.float32


@pytest.fixture(scope="module")
def states():
    """family -> (g, flags per element, {step: (p, m, v)}), computed once"""
    out = {}
    for fi, (ps, gs) in enumerate(R.FAMILIES):
        p, g = R.family_inputs(N, ps, gs, 100 + fi)
        fe = R.seeded_flags(N // 1024, 7).bool().repeat_interleave(1024)
        out[fi] = (g, fe, R.teacher_states(p, g, fe, R.STEPS))
    return out


def _kernel_f32(p, g, m, v, sc, decay, coef):
    """adamw_kernel's UPD() in numpy fp32, operation by operation in the kernel's order"""
    p, g, m, v, decay = (np.asarray(x, dtype=F32) for x in (p, g, m, v, decay))
    b2, omb1, omb2, eps, bc2s, step = (F32(sc[k]) for k in ("b2", "omb1", "omb2", "eps", "bc2_sqrt", "step_size"))
    gr = g * F32(coef) if coef is not None else g
    pp = p * decay
    mm = m + (gr - m) * omb1
    vv = v * b2 + (omb2 * gr) * gr
    denom = np.sqrt(vv) / bc2s + eps
    pp = pp - step * (mm / denom)
    assert pp.dtype == F32 and mm.dtype == F32 and vv.dtype == F32
    return pp, mm, vv


def test_fp32_restatement_stays_within_the_bound(states):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    worst_clip = dict(worst)
    for fi in states:
        g, fe, st = states[fi]
        for step, (p, m, v) in st.items():
            sc = R.host_scalars(step=step, **R.HYPER)
            gt = R.grad_at(g, step)
            decay = torch.where(fe, torch.full_like(p, sc["decay"]), torch.ones_like(p))
            gnorm = F32(float(gt.norm()))
            for max_norm in (0.0, 0.37 * float(gnorm)):
                coef, on = R.coef_ref(gnorm, max_norm)
                c32 = None
                if on:
                    c32 = min(F32(max_norm) / (gnorm + F32(1e-6)), F32(1.0))
                    assert c32.dtype == F32 and c32 < 1
                got = _kernel_f32(p.numpy(), gt.numpy(), m.numpy(), v.numpy(), sc, decay.numpy(), c32)
                ref, err = R.adamw_ref(p, gt, m, v, dict(sc, coef=coef), decay, sc["step_size"], on)
                for k, gk, rk, ek in zip("pmv", got, ref, err):
                    r = R.worst_ratio(torch.from_numpy(gk), rk, ek, R.TINY)
                    w = worst_clip if on else worst
                    w[k] = max(w[k], r)
                    assert r <= 1.0, (R.FAMILIES[fi], step, max_norm, k, r)
    print("\n  fp32 restatement, worst |err| / bound: unclipped p %.3f m %.3f v %.3f, clipped p %.3f m %.3f v %.3f (bar 1)"
          % (worst["p"], worst["m"], worst["v"], worst_clip["p"], worst_clip["m"], worst_clip["v"]))
    assert min(worst.values()) > 0.25, worst          # and it is a bound of this arithmetic, not a blanket


def _mutant(kind, p, g, m, v, sc, hyper):
    """p' of a WRONG AdamW in float64 (weight decay on every element, no clipping)"""
    b1m, b2, omb2, eps, bc2s, step, decay = sc["omb1"], sc["b2"], sc["omb2"], sc["eps"], sc["bc2_sqrt"], sc["step_size"], sc["decay"]
    gr = g + hyper["wd"] * p if kind == "l2_in_gradient" else g
    m1 = m + (gr - m) * b1m
    v1 = v * b2 + omb2 * gr * gr
    if kind == "eps_inside_sqrt":
        den = torch.sqrt(v1 + eps) / bc2s
    elif kind == "eps_before_division":
        den = (torch.sqrt(v1) + eps) / bc2s
    elif kind == "no_second_bias_correction":
        den = torch.sqrt(v1) + eps
    else:
        den = torch.sqrt(v1) / bc2s + eps
    if kind == "decay_after_update":
        return (p - step * (m1 / den)) * decay
    if kind == "l2_in_gradient":
        return p - step * (m1 / den)
    return p * decay - step * (m1 / den)


MUTANTS = ("eps_inside_sqrt", "eps_before_division", "no_second_bias_correction", "decay_after_update", "l2_in_gradient")


def test_five_wrong_formulas_leave_the_bound(states):
    share = {k: {} for k in MUTANTS}
    for fi in states:
        g, _, st = states[fi]
        for step, (p, m, v) in st.items():
            sc = R.host_scalars(step=step, **R.HYPER)
            gt = R.grad_at(g, step)
            (rp, _, _), (ep, _, _) = R.adamw_ref(p, gt, m, v, sc, sc["decay"], sc["step_size"], False)
            same = _mutant("none", p, gt, m, v, sc, R.HYPER)
            assert float(((same - rp).abs() / ep.clamp_min(1e-300)).max()) < 1e-3        # the mutants' frame is the reference's
            for k in MUTANTS:
                d = (_mutant(k, p, gt, m, v, sc, R.HYPER) - rp).abs()
                share[k][(fi, step)] = float((d > 10 * ep).double().mean())
    print("\n  share of elements beyond 10 x bound   " + "  ".join("|p|%g,|g|%g" % f for f in R.FAMILIES) + "   (rows: steps %s)" % (R.STEPS,))
    for k in MUTANTS:
        print("  %-28s" % k)
        for step in R.STEPS:
            print("      step %-5d" % step + "  ".join("%14.3f" % share[k][(fi, step)] for fi in range(len(R.FAMILIES))))
        assert max(share[k].values()) > 0.01, (k, share[k])
        assert share[k][(2, 1)] > 0.01, (k, "small-gradient family, step 1", share[k][(2, 1)])


# ------------------------------------------------------------------------------------------------ (c) refusals
def _lib():
    from mem_amd import _lib, ops  # noqa: F401  (ops declares the signatures)
    return _lib.lib


def _bad(rc, lib, word, code=-1):
    assert rc == code, rc
    assert word.encode() in lib.memhip_last_error(), lib.memhip_last_error()


def test_step_tail_entries_validate_before_any_launch():
    """Bad shapes / steps / missing pointers return MEMHIP_EINVAL (MEMHIP_EWORKSPACE for the short workspace) with a
    message; nothing is launched (no GPU here).  The pointers are host buffers nobody dereferences."""
    lib = _lib()
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert p.value % 16 == 0
    hp = (0.001, 0.9, 0.95, 1e-8, 0.05)
    # adamw
    _bad(lib.memhip_adamw(p, p, p, p, 1000, p, *hp, 1, None, 0.0, None), lib, "multiple of 1024")
    _bad(lib.memhip_adamw(p, p, p, p, -1024, p, *hp, 1, None, 0.0, None), lib, "multiple of 1024")
    _bad(lib.memhip_adamw(p, p, p, p, 1024, p, *hp, 0, None, 0.0, None), lib, "bad arguments")
    _bad(lib.memhip_adamw(p, p, p, p, 1024, None, *hp, 1, None, 0.0, None), lib, "bad arguments")
    _bad(lib.memhip_adamw(p, p, p, p, 1024, p, *hp, 1, None, 1.0, None), lib, "clipping needs gnorm")
    assert lib.memhip_adamw(None, None, None, None, 0, None, *hp, 0, None, 1.0, None) == 0          # n == 0: OK first
    # adamw_groups
    gp = (0.9, 0.95, 1e-8)
    _bad(lib.memhip_adamw_groups(p, p, p, p, 1000, p, p, 2, *gp, 1, None, 0.0, None), lib, "multiple of 1024")
    _bad(lib.memhip_adamw_groups(p, p, p, p, 1024, p, p, 2, *gp, 0, None, 0.0, None), lib, "bad arguments")
    _bad(lib.memhip_adamw_groups(p, p, p, p, 1024, p, p, 0, *gp, 1, None, 0.0, None), lib, "bad arguments")
    _bad(lib.memhip_adamw_groups(p, p, p, p, 1024, p, p, 257, *gp, 1, None, 0.0, None), lib, "bad arguments")
    _bad(lib.memhip_adamw_groups(p, p, p, p, 1024, p, None, 2, *gp, 1, None, 0.0, None), lib, "bad arguments")
    _bad(lib.memhip_adamw_groups(p, p, p, p, 1024, p, p, 256, *gp, 1, None, 1.0, None), lib, "clipping needs gnorm")
    assert lib.memhip_adamw_groups(None, None, None, None, 0, None, None, 0, *gp, 0, None, 0.0, None) == 0
    # grad_norm
    need = lib.memhip_grad_norm_workspace()
    assert need == 1024 * 8
    _bad(lib.memhip_grad_norm(p, 6, p, p, need, None), lib, "bad arguments")
    _bad(lib.memhip_grad_norm(p, -4, p, p, need, None), lib, "bad arguments")
    _bad(lib.memhip_grad_norm(p, 8, p, None, need, None), lib, "bad arguments")
    _bad(lib.memhip_grad_norm(p, 8, p, p, need - 8, None), lib, "workspace too small", code=-2)
    # cast
    _bad(lib.memhip_cast_f32_bf16(p, p, 6, None), lib, "multiple of 4")
    _bad(lib.memhip_cast_f32_bf16(p, None, 8, None), lib, "null pointer")
    assert lib.memhip_cast_f32_bf16(None, None, 0, None) == 0
    # transpose_cast: ldout a multiple of 8 and >= R
    _bad(lib.memhip_transpose_cast_f32_bf16(p, 8, 8, 8, p, 12, None), lib, "ldout")
    _bad(lib.memhip_transpose_cast_f32_bf16(p, 8, 16, 8, p, 8, None), lib, "ldout")
    _bad(lib.memhip_transpose_cast_f32_bf16(p, 8, 0, 8, p, 8, None), lib, "bad arguments")
    # transpose_cast_batched
    _bad(lib.memhip_transpose_cast_batched(p, p, -1, 1, None), lib, "bad arguments")
    _bad(lib.memhip_transpose_cast_batched(None, p, 1, 1, None), lib, "null pointer")
    assert lib.memhip_transpose_cast_batched(None, None, 0, 5, None) == 0
    assert lib.memhip_transpose_cast_batched(p, p, 3, 0, None) == 0
    # transpose_bf16: R_pad a multiple of 64, >= R, <= ldout
    _bad(lib.memhip_transpose_bf16(p, 8, 8, 8, p, 72, 72, None, 0, 0, None, 0, 0, None), lib, "R_pad=72")
    _bad(lib.memhip_transpose_bf16(p, 8, 70, 8, p, 64, 64, None, 0, 0, None, 0, 0, None), lib, "R_pad=64")
    _bad(lib.memhip_transpose_bf16(p, 8, 8, 8, p, 56, 64, None, 0, 0, None, 0, 0, None), lib, "R_pad=64")
    _bad(lib.memhip_transpose_bf16(p, 8, 8, 0, p, 64, 64, None, 0, 0, None, 0, 0, None), lib, "bad arguments")
    assert lib.memhip_transpose_bf16(p, 8, 0, 8, p, 64, 0, None, 0, 0, None, 0, 0, None) == 0      # nothing to write
    # zero
    _bad(lib.memhip_zero(p, 24, None), lib, "multiples of 16")
    _bad(lib.memhip_zero(C.c_void_p(p.value + 4), 16, None), lib, "multiples of 16")
    _bad(lib.memhip_zero(None, 16, None), lib, "null pointer")
    assert lib.memhip_zero(p, 0, None) == 0
