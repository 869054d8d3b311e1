"""Float64 reference of the optimizer tail (optim.hip) with a running first-order error bound -- no tests in here.

adamw_ref evaluates exactly the expression in the comment above adamw_kernel,

    p *= decay ; m = m + (gr - m) * (1 - b1) ; v = v * b2 + ((1 - b2) * gr) * gr ;
    denom = sqrt(v) / sqrt(bc2) + eps ; p -= step_size * (m / denom)          with gr = g * coef,

in float64 on torch tensors (CPU tensors from numpy arrays, or device tensors), from the SAME fp32 scalars the host entry
hands to the kernel (host_scalars), taken as exact.  Next to every value it carries a bound on what an fp32 evaluation of
the same expression can be off by: every fp32 operation adds u * |its exact result| (u = 2^-24, round to nearest), and
the errors of its operands are propagated to first order:

    sum / difference  a +- b     e = e_a + e_b + u |a +- b|
    product           a * b      e = |b| e_a + |a| e_b + u |a b|          (scalars are exact: e_b = 0)
    sqrt              s = sqrt(a)  e = e_a / (2 s) + u s                  (0 at a == 0: every operand is then exactly 0)
    quotient          z = a / b  e = e_a / |b| + |z| e_b / |b| + u |z|

Clipping (coef_on): gr = g * coef with coef = min(1, max_norm / (gnorm + 1e-6)) formed in fp32 by the kernel (the add, the
division, the product: 3u |gr|) and in float64 here from the fp32 norm the device holds.  Without clipping gr = g, exact.
Contraction of a product and a sum into one FMA only removes a rounding, so the bound holds with or without it.  The
bound is in absolute units; results in the fp32 denormal range additionally move by up to 2^-149 (the caller's bar)."""
import math
import struct

import torch

U = 2.0 ** -24
TINY = 2.0 ** -149


def f32(x):
    """the double nearest-even rounded to fp32, as a Python float (== the C cast (float)x)"""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def host_scalars(lr, b1, b2, eps, wd, step):
    """The fp32 scalars memhip_adamw computes on the host (in double, cast once), as exact Python floats.
    decay / step_size are the per-call values; memhip_adamw_groups reads them from its table instead."""
    bc1 = 1.0 - math.pow(b1, float(step))
    bc2 = 1.0 - math.pow(b2, float(step))
    fb1, fb2 = f32(b1), f32(b2)
    return dict(b1=fb1, b2=fb2, omb1=f32(1.0 - fb1), omb2=f32(1.0 - fb2),        # 1.0f - b1: one fp32 subtraction
                eps=f32(eps), bc2_sqrt=f32(math.sqrt(bc2)), decay=f32(1.0 - lr * wd), step_size=f32(lr / bc1), coef=1.0)


def coef_ref(gnorm_f32, max_norm):
    """clip_grad_norm_'s factor in float64 from the fp32 norm on the device; (coef, coef_on)"""
    mn = f32(max_norm)
    if not mn > 0.0:
        return 1.0, False
    return min(1.0, mn / (float(gnorm_f32) + f32(1e-6))), True


def adamw_ref(p, g, m, v, scal, decay, step_size, coef_on, bounds=True):
    """(p', m', v') in float64 and, with bounds, (e_p, e_m, e_v).  p, g, m, v: float64 tensors holding fp32 values;
    decay, step_size: Python floats or per-element float64 tensors (fp32 values); scal: host_scalars() with coef set."""
    b2, omb1, omb2, eps, bc2s = scal["b2"], scal["omb1"], scal["omb2"], scal["eps"], scal["bc2_sqrt"]
    gr = g * scal["coef"] if coef_on else g
    p1 = p * decay
    d = gr - m
    t = d * omb1
    m1 = m + t
    a = v * b2
    b = omb2 * gr
    c = b * gr
    v1 = a + c
    s = torch.sqrt(v1)
    q = s / bc2s
    den = q + eps
    z = m1 / den
    w = step_size * z
    p2 = p1 - w
    if not bounds:
        return p2, m1, v1
    e_gr = 3 * U * gr.abs() if coef_on else torch.zeros_like(gr)
    e_p1 = U * p1.abs()
    e_d = e_gr + U * d.abs()
    e_t = omb1 * e_d + U * t.abs()
    e_m = e_t + U * m1.abs()
    e_a = U * a.abs()
    e_b = omb2 * e_gr + U * b.abs()
    e_c = gr.abs() * e_b + b.abs() * e_gr + U * c.abs()
    e_v = e_a + e_c + U * v1.abs()
    e_s = torch.where(s > 0, e_v / (2 * s).clamp_min(1e-300), torch.zeros_like(s)) + U * s
    e_q = e_s / bc2s + U * q
    e_den = e_q + U * den
    e_z = e_m / den + z.abs() * e_den / den + U * z.abs()
    e_w = step_size * e_z + U * w.abs()
    e_p = e_p1 + e_w + U * p2.abs()
    return (p2, m1, v1), (e_p, e_m, e_v)


def worst_ratio(got, ref, bound, floor=0.0):
    """max (|got - ref| - floor)+ / bound as a float: got passes a bar of k x bound + floor iff this is <= k
    (0 for an empty tensor, inf where got is not finite)"""
    if got.numel() == 0:
        return 0.0
    r = ((got.double() - ref).abs() - floor).clamp_min(0.0) / bound.clamp_min(1e-300)
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return float(r.max().item())


# ------------------------------------------------------------------------------------------------ shared inputs
FAMILIES = ((0.02, 1e-3), (1.0, 3.0), (0.02, 1e-7))       # (|p|, |g|): pretraining, the thin test's, eps-visible
STEPS = (1, 2, 3, 50, 1000)
HYPER = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.05)


def family_inputs(n, p_scale, g_scale, seed, device="cpu"):
    """(p, g) fp32 values as float64: normal deviates at the family's scales, every 97th gradient exactly 0"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    p = (torch.randn(n, generator=gen, dtype=torch.float64) * p_scale).float().double()
    g = (torch.randn(n, generator=gen, dtype=torch.float64) * g_scale).float().double()
    g[::97] = 0.0
    return p.to(device), g.to(device)


def grad_at(g, step):
    """the gradient of a step of the teacher-forced chain: a rotation of g (the exact zeros move) at a varying scale"""
    return (torch.roll(g, step) * (1.0 + 0.25 * math.cos(step))).float().double()


def seeded_flags(nchunks, seed, device="cpu"):
    """u8 [nchunks]: a seeded, non-periodic 0/1 pattern that holds both values"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    f = torch.randint(0, 2, (nchunks,), generator=gen, dtype=torch.uint8)
    if nchunks >= 2:
        f[0], f[1] = 1, 0
    return f.to(device)


def teacher_states(p, g, flags_elem, steps, hyper=HYPER):
    """{step: (p, m, v)}: the state BEFORE `step`, reached by step - 1 unclipped reference steps from m = v = 0, each
    rounded to fp32 (teacher forcing: a kernel step is always fed the reference's state, never its own)."""
    out = {}
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t in range(1, max(steps) + 1):
        if t in steps:
            out[t] = (p, m, v)
        sc = host_scalars(hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"], hyper["wd"], t)
        decay = torch.where(flags_elem, torch.full_like(p, sc["decay"]), torch.ones_like(p))
        p, m, v = (x.float().double() for x in adamw_ref(p, grad_at(g, t), m, v, sc, decay, sc["step_size"], False, bounds=False))
    return out
