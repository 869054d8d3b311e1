"""-m "not gpu": class weights and OHEM pixel sampling in the segmentation loss, everything that needs no device: the layout of
the two new structs, every validation rule of memhip_seg_ohem_keys / _select / memhip_seg_ce_w and of their plan query (dummy
addresses, nothing is dereferenced, no case reaches a launch), the torch arm of SegCrossEntropy and of a head's loss_decode=
against a float64 oracle written here from the definition (sort-based), the entrypoint's flags and tools/seg_class_weights.py."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "memhip.h")
P = 0x1000          # a dummy, 16-byte aligned, non-NULL address
IGN = 255


# ---------------------------------------------------------------- layout
def _host_cc():
    for cc in (shutil.which("cc"), "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        if cc and os.path.exists(cc):
            return cc
    return None


def test_struct_layout_matches_header(tmp_path):
    from mem_amd import ops
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    mirrors = {"memhip_segohem_args_t": ops.SegOhemArgs, "memhip_segohem_plan_t": ops.SegOhemPlan}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "memhip.h"', "int main(void) {"]
    for name, cls in mirrors.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f[0], name, f[0]) for f in cls._fields_]
    lines += ['  printf("seg_args %zu\\n", sizeof(memhip_seg_args_t));', '  printf("seg_plan %zu\\n", sizeof(memhip_seg_plan_t));',
              "  return 0;", "}"]
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(src, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]                 # a mirror's field that the header lacks does not compile
    got = dict(line.split() for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == int(got[name]), (name, C.sizeof(cls), got[name])
        covered = 0
        for field, ctype in cls._fields_:
            assert getattr(cls, field).offset == int(got["%s.%s" % (name, field)]), (name, field)
            covered += C.sizeof(ctype)
        assert covered == C.sizeof(cls), (name, "padding or a field of the header without a mirror")
    # the loss's own struct is the first member, unchanged: a caller compiled against it passes the size it always passed
    assert ops.SegOhemArgs.seg.offset == 0 and C.sizeof(ops.SegArgs) == int(got["seg_args"])
    assert ops.SegOhemPlan.seg.offset == 0 and C.sizeof(ops.SegPlan) == int(got["seg_plan"])


def test_symbols_old_and_new_and_the_abi_number():
    from mem_amd import _lib
    for name in ("memhip_seg_axis_table", "memhip_seg_plan", "memhip_seg_ce", "memhip_seg_confusion", "memhip_seg_predict",
                 "memhip_seg_predict_plan", "memhip_seg_ohem_plan", "memhip_seg_ohem_keys", "memhip_seg_ohem_select", "memhip_seg_ce_w"):
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.memhip_abi_version() == 10


# ---------------------------------------------------------------- validation, the three calls and the plan query alike
ENTRIES = ("memhip_seg_ohem_keys", "memhip_seg_ohem_select", "memhip_seg_ce_w")


def _args(sampler=1, thresh=0.7, min_kept=100, **kw):
    """a complete, acceptable struct on dummy addresses, with the given fields replaced"""
    from mem_amd import ops
    shape = dict(B=2, C_=11, h=9, w=17, H=36, W=68, ignore_index=255, align_corners=False, avg_non_ignore=False, loss_weight=1.0)
    seg = dict(logits=P, labels=P, dz=P, loss=P, stats=P, workspace=P, workspace_bytes=1 << 30,
               y_i0=P, y_w1=P, y_lo=P, y_hi=P, x_i0=P, x_w1=P, x_lo=P, x_hi=P)
    own = dict(class_weight=P, keys=P, threshold=P)
    for k, v in kw.items():
        (shape if k in shape else seg if k in seg else own)[k] = v
    return ops.seg_ohem_args(ops.seg_args(**shape, **seg), sampler, thresh, min_kept, **own)


def _call(fn, a):
    from mem_amd import _lib
    rc = getattr(_lib.lib, fn)(None if a is None else C.byref(a), None)
    return rc, _lib.lib.memhip_last_error().decode()


def _query(a):
    from mem_amd import _lib, ops
    rc = _lib.lib.memhip_seg_ohem_plan(C.byref(a), C.byref(ops.SegOhemPlan()))
    return rc, _lib.lib.memhip_last_error().decode()


BAD = {
    "null keys": (dict(keys=None), "null pointer (keys, threshold) with sampler=1"),
    "null threshold": (dict(threshold=None), "null pointer (keys, threshold) with sampler=1"),
    "null keys top-k": (dict(sampler=2, keys=None), "null pointer (keys, threshold) with sampler=2"),
    "thresh=0": (dict(thresh=0.0), "thresh=0 must lie in (0, 1]"),
    "thresh<0": (dict(thresh=-0.5), "thresh=-0.5 must lie in (0, 1]"),
    "thresh>1": (dict(thresh=1.5), "thresh=1.5 must lie in (0, 1]"),
    "thresh nan": (dict(thresh=float("nan")), "must lie in (0, 1]"),
    "min_kept<0": (dict(min_kept=-1), "min_kept=-1"),
    "min_kept<0 top-k": (dict(sampler=2, min_kept=-7), "min_kept=-7"),
    "min_kept huge": (dict(min_kept=(1 << 40) + 1), "min_kept="),
    "sampler=3": (dict(sampler=3), "sampler=3 must be 0 (none), 1 (thresh) or 2 (top-k)"),
    "sampler=-1": (dict(sampler=-1), "sampler=-1 must be"),
    "keys unaligned": (dict(keys=P + 2), "not 4-byte aligned"),
    # the loss's own rules come first, with the loss's messages
    "C=33": (dict(C_=33), "seg: bad shape C=33 (2 <= C <= 32)"),
    "H<h": (dict(H=8), "seg: bad shape H=8 W=68 for logits of 9x17"),
    "ignore_index=256": (dict(ignore_index=256), "seg: ignore_index=256"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_every_rule_rejects_before_any_launch_and_the_plan_agrees(case):
    kw, needle = BAD[case]
    want = _query(_args(**kw))
    assert want[0] == -1 and needle in want[1], (case, want)
    for fn in ENTRIES:
        assert _call(fn, _args(**kw)) == want, (case, fn)


def test_workspace_one_short_is_its_own_code_everywhere():
    from mem_amd import ops
    for sampler in (1, 2):
        plan = ops.seg_ohem_plan(2, 11, 9, 17, 36, 68, sampler=sampler, thresh=0.7 if sampler == 1 else None, min_kept=5)
        base = ops.seg_plan(2, 11, 9, 17, 36, 68)
        need = int(plan.ws_bytes)
        assert plan.seg.ws_bytes == base.ws_bytes == 2 * 2 * 3 * 24 and plan.select_ws_offset == base.ws_bytes
        assert plan.select_ws_bytes == 3 * 2048 * 8 + 40 and need == plan.select_ws_offset + plan.select_ws_bytes
        short = _args(sampler=sampler, workspace_bytes=need - 1)
        want = _query(short)
        assert want[0] == -2 and "workspace %d < %d" % (need - 1, need) in want[1]
        for fn in ENTRIES:
            assert _call(fn, _args(sampler=sampler, workspace_bytes=need - 1)) == want, fn
        assert _query(_args(sampler=sampler, workspace_bytes=need))[0] == 0
        assert _query(_args(sampler=sampler, workspace=None, workspace_bytes=0))[0] == 0      # no workspace, no comparison
    # without a sampler the selection needs nothing: the loss's workspace, and its lds with the staged weights
    plan = ops.seg_ohem_plan(2, 11, 9, 17, 36, 68)
    assert plan.select_ws_bytes == 0 and plan.ws_bytes == 2 * 2 * 3 * 24
    assert plan.seg.lds_bytes == ops.seg_plan(2, 11, 9, 17, 36, 68).lds_bytes + 32 * 4
    assert _call("memhip_seg_ce_w", _args(sampler=0, workspace_bytes=plan.ws_bytes - 1))[0] == -2


def test_what_only_a_call_needs():
    """device pointers of the loss's struct may be NULL in the query; each call names the ones it misses"""
    assert _query(_args(logits=None, labels=None, dz=None, loss=None, stats=None, y_i0=None))[0] == 0
    for field in ("logits", "labels"):
        for fn in ("memhip_seg_ohem_keys", "memhip_seg_ce_w"):
            rc, err = _call(fn, _args(**{field: None}))
            assert rc == -1 and "seg: null pointer (logits, labels)" in err, (fn, field, err)
    rc, err = _call("memhip_seg_ohem_keys", _args(x_w1=None))
    assert rc == -1 and "seg: null pointer (axis tables)" in err
    for field in ("dz", "loss", "stats", "workspace"):
        rc, err = _call("memhip_seg_ce_w", _args(**{field: None}))
        assert rc == -1 and "seg_ce: null pointer" in err, (field, err)
    for field in ("stats", "workspace"):
        rc, err = _call("memhip_seg_ohem_select", _args(**{field: None}))
        assert rc == -1 and "seg_ohem_select: null pointer (stats, workspace)" in err, (field, err)
    rc, err = _call("memhip_seg_ohem_select", _args(workspace=P + 4))
    assert rc == -1 and "not 8-byte aligned" in err
    rc, err = _call("memhip_seg_ce_w", _args(loss_weight=float("inf")))
    assert rc == -1 and "loss_weight" in err
    # sampler 0: nothing to select, and keys / threshold / class_weight may be NULL in memhip_seg_ce_w
    for fn in ENTRIES[:2]:
        rc, err = _call(fn, _args(sampler=0))
        assert rc == -1 and "sampler=0 has no keys" in err, (fn, err)
    assert _query(_args(sampler=0, keys=None, threshold=None, class_weight=None))[0] == 0
    for fn in ENTRIES:
        assert _call(fn, None) == (-1, "seg: null args")
    from mem_amd import _lib
    assert _lib.lib.memhip_seg_ohem_plan(C.byref(_args()), None) == -1


def test_plan_as_data():
    from mem_amd import ops
    plan = ops.seg_ohem_plan(16, 11, 110, 160, 440, 640, sampler=1, thresh=0.7, min_kept=100000)
    assert (plan.keys_grid, plan.keys_block) == (2048, 256) and (plan.select_grid, plan.select_block) == (1024, 256)
    assert (plan.select_passes, plan.select_bins, plan.select_lds_bytes) == (3, 2048, 8192)
    assert plan.seg.grid == 16 * 14 * 20 and plan.select_ws_offset % 8 == 0
    small = ops.seg_ohem_plan(1, 2, 1, 1, 1, 2, sampler=2, min_kept=0)
    assert (small.keys_grid, small.select_grid) == (1, 1)
    assert ops.seg_ohem_plan(3, 5, 9, 17, 36, 68, sampler=2).select_grid == (3 * 36 * 68 + 255) // 256


# ---------------------------------------------------------------- the float64 oracle, from the definition
def oracle(z, lab, cw=None, T=None, m=None, loss_weight=1.0, avg_non_ignore=False, align=False):
    """float64: (loss, dz, keep mask, threshold, counts) -- interpolate, log-softmax, sort.  m None: no sampler."""
    z = z.detach().double().requires_grad_()
    B, Cc = z.shape[:2]
    lab = lab.long()
    up = F.interpolate(z, size=tuple(lab.shape[1:]), mode="bilinear", align_corners=align)
    valid = (lab != IGN) & (lab < Cc)
    tgt = torch.where(valid, lab, torch.zeros_like(lab))
    logp = F.log_softmax(up, 1)
    nll = -logp.gather(1, tgt[:, None])[:, 0]
    w = torch.ones(Cc, dtype=torch.float64) if cw is None else torch.as_tensor(cw, dtype=torch.float64)
    wl = w[tgt]
    n = int(valid.sum())
    keep, t = valid.clone(), None
    if m is not None:
        K = m * B
        if T is not None:
            key = logp.exp().gather(1, tgt[:, None])[:, 0].detach()
            if n == 0:
                keep, t = torch.zeros_like(valid), -math.inf
            else:
                a = torch.sort(key[valid]).values
                t = max(float(a[min(K, n - 1)]), T)
                keep = valid & (key < t)
        else:
            key = (wl * nll).detach()
            Kp = min(K, n)
            if Kp == 0:
                keep, t = torch.zeros_like(valid), math.inf
            else:
                t = float(torch.sort(key[valid], descending=True).values[Kp - 1])
                keep = valid & (key >= t)
    N = max(n, 1) if avg_non_ignore else lab.numel()
    loss = (wl * nll)[keep].sum() * loss_weight / N
    loss.backward()
    counts = dict(n_valid=n, n_correct=int(((up.argmax(1) == lab) & valid).sum()), n_bad=int(((lab != IGN) & ~valid).sum()),
                  n_kept=int(keep.sum()))
    return loss.detach(), z.grad, keep, t, counts


def make_case(seed, B, Cc, h, w, H, W, p_ignore=0.2):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn((B, Cc, h, w), generator=gen) * 3
    lab = torch.randint(0, Cc, (B, H, W), generator=gen)
    lab[torch.rand((B, H, W), generator=gen) < p_ignore] = IGN
    lab.view(-1)[5] = Cc                                           # a bad label
    cw = torch.rand(Cc, generator=gen) * 3
    cw[1] = 0.0
    return z, lab, cw


MODES = [("weights", dict(T=None, m=None)), ("thresh", dict(T=0.7, m=40)), ("topk", dict(T=None, m=40))]


def _sampler(T, m):
    from mem_amd.seg_loss import OHEMPixelSampler
    return None if m is None else OHEMPixelSampler(thresh=T, min_kept=m)


@pytest.mark.parametrize("name,mode", MODES)
@pytest.mark.parametrize("avg", [False, True])
def test_torch_arm_of_the_loss_against_the_oracle(name, mode, avg):
    from mem_amd.seg_loss import SegCrossEntropy
    B, Cc = 2, 5
    z, lab, cw = make_case(1, B, Cc, 6, 7, 24, 28)
    ref = oracle(z, lab, cw, mode["T"], mode["m"], 0.4, avg)
    mod = SegCrossEntropy(loss_weight=0.4, avg_non_ignore=avg, class_weight=cw.tolist(), sampler=_sampler(**mode), impl="torch")
    zz = z.double().requires_grad_()
    loss = mod(zz, lab.unsqueeze(1))                               # mmseg's [B, 1, H, W]
    loss.backward()
    s = mod.last_stats
    print(name, avg, "loss", float(loss.detach()), float(ref[0]), "kept", int(s["n_kept"]), ref[4]["n_kept"], "t", s["threshold"], ref[3])
    assert float(loss.detach()) == pytest.approx(float(ref[0]), rel=1e-12) and torch.allclose(zz.grad, ref[1], rtol=1e-10, atol=1e-15)
    assert torch.equal(s["keep"], ref[2])
    assert {k: int(s[k]) for k in ("n_valid", "n_correct", "n_bad", "n_kept")} == ref[4]
    assert 0 < ref[4]["n_kept"] < ref[4]["n_valid"] or mode["m"] is None
    if mode["m"] is None:
        assert s["threshold"] is None
    else:
        assert float(s["threshold"]) == pytest.approx(ref[3], rel=1e-12)
    assert float(mod.acc_seg()) == 100.0 * ref[4]["n_correct"] / ref[4]["n_valid"]
    # float32 on the same inputs: the same definition, fp32 roundings away
    m32 = SegCrossEntropy(loss_weight=0.4, avg_non_ignore=avg, class_weight=cw, sampler=_sampler(**mode), impl="torch")
    assert float(m32(z, lab)) == pytest.approx(float(ref[0]), rel=1e-5)


def test_plain_torch_arm_is_the_unweighted_loss():
    from mem_amd.seg_loss import SegCrossEntropy
    z, lab, _ = make_case(2, 2, 4, 5, 5, 10, 15)
    ref = oracle(z, lab)
    mod = SegCrossEntropy(impl="torch")
    loss = mod(z.double(), lab)
    assert float(loss) == pytest.approx(float(ref[0]), rel=1e-12) and int(mod.last_stats["n_kept"]) == ref[4]["n_valid"]
    want = F.cross_entropy(F.interpolate(z.double(), size=(10, 15), mode="bilinear"), torch.where(lab < 4, lab, -100), reduction="sum") / lab.numel()
    assert float(loss) == pytest.approx(float(want), rel=1e-12)


@pytest.mark.parametrize("T", [0.7, None])
def test_torch_arm_edges(T):
    from mem_amd.seg_loss import OHEMPixelSampler, SegCrossEntropy
    B, Cc = 2, 5
    z, lab, cw = make_case(3, B, Cc, 4, 5, 8, 10)
    n = int(((lab != IGN) & (lab < Cc)).sum())

    def run(m, labels=lab):
        mod = SegCrossEntropy(class_weight=cw, sampler=OHEMPixelSampler(T, m), impl="torch")
        zz = z.double().requires_grad_()
        loss = mod(zz, labels)
        loss.backward()
        return loss.detach(), zz.grad, mod.last_stats

    # m = 0: top-k keeps nothing; thresh keeps what lies below max(the smallest key, T)
    loss, grad, s = run(0)
    ref = oracle(z, lab, cw, T, 0)
    assert int(s["n_kept"]) == ref[4]["n_kept"] and float(loss) == pytest.approx(float(ref[0]), rel=1e-12, abs=0)
    if T is None:
        assert int(s["n_kept"]) == 0 and float(loss) == 0.0 and not bool(grad.any()) and float(s["threshold"]) == math.inf
    # K >= n: top-k keeps every valid pixel, the weighted loss without a sampler; thresh: all below max(the largest key, T)
    for m in ((n + B - 1) // B, n):
        assert m * B >= n
        loss, grad, s = run(m)
        ref = oracle(z, lab, cw, T, m)
        assert torch.equal(s["keep"], ref[2]) and float(loss) == pytest.approx(float(ref[0]), rel=1e-12)
        if T is None:
            plain = oracle(z, lab, cw)
            assert int(s["n_kept"]) == n and float(loss) == pytest.approx(float(plain[0]), rel=1e-12) and torch.allclose(grad, plain[1], rtol=1e-10, atol=0)
    # everything ignored: nothing kept, loss 0, gradient 0, no NaN
    loss, grad, s = run(5, torch.full_like(lab, IGN))
    assert float(loss) == 0.0 and not bool(grad.any()) and int(s["n_kept"]) == 0 and int(s["n_valid"]) == 0
    assert float(s["threshold"]) == (-math.inf if T is not None else math.inf)


def test_topk_keeps_every_key_that_ties_with_the_last():
    """logits constant over the map and labels in blocks: every pixel of a class has the same key.  Class 0 is the hardest
    (3 pixels), class 1 next (4 pixels): K = 5 ends inside class 1's ties, and all 7 are kept, not 5."""
    from mem_amd.seg_loss import OHEMPixelSampler, SegCrossEntropy
    z = torch.tensor([-2.0, 0.0, 3.0], dtype=torch.float64).view(1, 3, 1, 1).expand(1, 3, 2, 2).contiguous()
    lab = torch.full((1, 4, 4), 2, dtype=torch.long)
    lab.view(-1)[:3] = 0
    lab.view(-1)[3:7] = 1
    lab.view(-1)[15] = IGN
    for K, kept in ((1, 3), (3, 3), (4, 7), (5, 7), (7, 7), (8, 15), (100, 15)):
        mod = SegCrossEntropy(sampler=OHEMPixelSampler(None, K), impl="torch")
        mod(z, lab)
        ref = oracle(z, lab, None, None, K)
        assert int(mod.last_stats["n_kept"]) == kept == ref[4]["n_kept"], (K, int(mod.last_stats["n_kept"]))
        assert torch.equal(mod.last_stats["keep"], ref[2])


# ---------------------------------------------------------------- arguments
def test_sampler_and_class_weight_arguments():
    from mem_amd.seg_loss import OHEMPixelSampler, SegCrossEntropy, make_sampler
    s = OHEMPixelSampler()
    assert (s.thresh, s.min_kept, s.mode) == (None, 100000, 2)                     # mmseg's defaults
    d = make_sampler(dict(type="OHEMPixelSampler", thresh=0.7, min_kept=50))
    assert (d.thresh, d.min_kept, d.mode) == (0.7, 50, 1) and make_sampler(None) is None and make_sampler(s) is s
    for bad in (dict(thresh=0.0), dict(thresh=1.5), dict(min_kept=-1), dict(min_kept=2.5)):
        with pytest.raises(ValueError):
            OHEMPixelSampler(**bad)
    with pytest.raises(NotImplementedError, match="UniformSampler"):
        make_sampler(dict(type="UniformSampler"))
    with pytest.raises(TypeError, match="context"):
        make_sampler(dict(type="OHEMPixelSampler", context=1))
    for bad in ([1.0, float("nan")], [1.0, -0.5], []):
        with pytest.raises(ValueError, match="class_weight"):
            SegCrossEntropy(class_weight=bad)
    mod = SegCrossEntropy(class_weight=[1.0, 2.0, 3.0], impl="torch")
    assert "class_weight" not in mod.state_dict() and mod.class_weight.dtype == torch.float32
    assert mod.double().class_weight.dtype == torch.float64                        # a buffer: .to() moves it
    with pytest.raises(ValueError, match="3 weights for logits of 4 classes"):
        mod(torch.zeros(1, 4, 2, 2, dtype=torch.float64), torch.zeros(1, 4, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="impl"):
        SegCrossEntropy(impl="cuda")


# ---------------------------------------------------------------- heads
def _head_cases():
    from mem_amd.seg_heads import FCNHead, PSPHead, UPerHead
    return [(FCNHead, dict(in_channels=10, channels=6, in_index=1), lambda x: (None, x)),
            (PSPHead, dict(in_channels=10, channels=6, in_index=0, pool_scales=(1, 2)), lambda x: (x,)),
            (UPerHead, dict(in_channels=(10, 10), channels=6, in_index=(0, 1), pool_scales=(1, 2)), lambda x: (x, x[:, :, ::2, ::2].contiguous()))]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_torch_head_with_loss_decode_against_the_oracle(which):
    cls, kw, inputs = _head_cases()[which]
    gen = torch.Generator().manual_seed(20 + which)
    cw = [0.5, 2.0, 0.0, 1.5]
    cfg = dict(type="CrossEntropyLoss", use_sigmoid=False, loss_weight=0.4, class_weight=cw, avg_non_ignore=True,
               sampler=dict(type="OHEMPixelSampler", thresh=0.7, min_kept=20))
    head = cls(num_classes=4, dropout_ratio=0.0, impl="torch", ignore_index=IGN, loss_decode=cfg, **kw).double().train()
    ld = head.loss_decode
    assert (ld.impl, ld.loss_weight, ld.avg_non_ignore, ld.ignore_index, ld.align_corners) == ("torch", 0.4, True, IGN, False)
    assert (ld.sampler.thresh, ld.sampler.min_kept) == (0.7, 20) and ld.class_weight.tolist() == cw
    assert not any("loss_decode" in k for k in head.state_dict())
    with torch.no_grad():
        head.conv_seg.weight.mul_(300.0)                           # confident logits: some probabilities above the threshold
    x = torch.randn(2, 10, 6, 8, generator=gen, dtype=torch.float64)
    lab = torch.randint(0, 4, (2, 1, 24, 32), generator=gen)
    lab[torch.rand(lab.shape, generator=gen) < 0.2] = IGN
    out = head.forward_train(inputs(x), lab)
    logits = head(inputs(x)).detach()                              # training mode, no dropout: the logits of that call
    ref = oracle(logits, lab[:, 0], cw, 0.7, 20, 0.4, True)
    assert float(out["loss_seg"]) == pytest.approx(float(ref[0]), rel=1e-10)
    assert float(out["acc_seg"]) == pytest.approx(100.0 * ref[4]["n_correct"] / ref[4]["n_valid"])
    assert int(ld.last_stats["n_kept"]) == ref[4]["n_kept"] and 0 < ref[4]["n_kept"] < ref[4]["n_valid"]
    out["loss_seg"].backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in head.parameters())


@pytest.mark.parametrize("which", [0, 1, 2])
def test_heads_keywords_and_loss_decode_refusals(which):
    from mem_amd.seg_loss import OHEMPixelSampler, SegCrossEntropy
    cls, kw, _ = _head_cases()[which]
    kw = dict(num_classes=4, impl="torch", **kw)
    with pytest.raises(NotImplementedError, match="class_weight"):
        cls(class_weight=[1.0] * 4, **kw)
    with pytest.raises(NotImplementedError, match="sampler"):
        cls(sampler=dict(type="OHEMPixelSampler"), **kw)
    with pytest.raises(ValueError, match="loss_weight=0.7"):
        cls(loss_decode=dict(type="CrossEntropyLoss", loss_weight=1.0), loss_weight=0.7, **kw)
    with pytest.raises(NotImplementedError, match="use_sigmoid"):
        cls(loss_decode=dict(type="CrossEntropyLoss", use_sigmoid=True), **kw)
    with pytest.raises(NotImplementedError, match="DiceLoss"):
        cls(loss_decode=dict(type="DiceLoss"), **kw)
    with pytest.raises(TypeError, match="bogus"):
        cls(loss_decode=dict(type="CrossEntropyLoss", bogus=1), **kw)
    mine = SegCrossEntropy(ignore_index=7, align_corners=True, loss_weight=0.3, sampler=OHEMPixelSampler(0.5, 10), impl="torch")
    head = cls(loss_decode=mine, ignore_index=IGN, **kw)
    assert head.loss_decode is mine and (mine.ignore_index, mine.align_corners, mine.loss_weight) == (IGN, False, 0.3)
    plain = cls(**kw)                                               # without loss_decode: the plain loss, as before
    assert plain.loss_decode.sampler is None and plain.loss_decode.class_weight is None and plain.loss_decode.impl == "hip"
    assert plain.loss_decode.loss_weight == (0.4 if which == 0 else 1.0)


# ---------------------------------------------------------------- the entrypoint's flags
def test_run_semseg_flags(tmp_path):
    from mem_amd import run_semseg as R
    a = R.get_args([])
    assert (a.class_weight, a.ohem_min_kept, a.ohem_thresh) == (None, None, None)         # off by default
    a = R.get_args(["--num_classes", "3", "--class_weight", "1,2.5,0", "--ohem_min_kept", "1000", "--ohem_thresh", "0.7"])
    assert (a.class_weight, a.ohem_min_kept, a.ohem_thresh) == ([1.0, 2.5, 0.0], 1000, 0.7)
    assert R.get_args(["--ohem_min_kept", "5"]).ohem_thresh is None                       # top-k
    as_list, as_obj = tmp_path / "w.json", tmp_path / "o.json"
    as_list.write_text(json.dumps([1, 2, 3.5]))
    as_obj.write_text(json.dumps({"pixel_counts": [1, 2, 3], "class_weight": [0.5, 1.0, 0.0]}))
    assert R.get_args(["--num_classes", "3", "--class_weight", str(as_list)]).class_weight == [1.0, 2.0, 3.5]
    assert R.get_args(["--num_classes", "3", "--class_weight", str(as_obj)]).class_weight == [0.5, 1.0, 0.0]
    (tmp_path / "bad.json").write_text(json.dumps({"weights": [1, 2, 3]}))
    for flags, needle in ((["--class_weight", "1,2,3"], "--num_classes is 11"), (["--num_classes", "3", "--class_weight", "1,x,3"], "neither"),
                          (["--num_classes", "3", "--class_weight", "1,-2,3"], ">= 0"), (["--ohem_thresh", "0.7"], "--ohem_min_kept"),
                          (["--ohem_min_kept", "-1"], "--ohem_min_kept"), (["--ohem_min_kept", "5", "--ohem_thresh", "1.5"], "--ohem_thresh"),
                          (["--num_classes", "3", "--class_weight", str(tmp_path / "bad.json")], "class_weight")):
        with pytest.raises(ValueError, match=needle):
            R.get_args(flags)


def test_run_semseg_builds_the_heads_losses():
    from mem_amd import run_semseg as R
    small = ["--vit", "tiny", "--depth", "4", "--net_size", "64", "64", "--decode_channels", "64", "--aux_channels", "64", "--num_classes", "3"]
    m = R.build_model(R.get_args(small))
    for head, lw in ((m.decode_head, 1.0), (m.auxiliary_head, 0.4)):
        assert head.loss_decode.class_weight is None and head.loss_decode.sampler is None and head.loss_decode.loss_weight == lw
    m = R.build_model(R.get_args(small + ["--class_weight", "1,2,0", "--ohem_min_kept", "50", "--ohem_thresh", "0.7", "--aux_loss_weight", "0.3"]))
    d, a = m.decode_head.loss_decode, m.auxiliary_head.loss_decode
    assert d.class_weight.tolist() == [1.0, 2.0, 0.0] == a.class_weight.tolist() and (d.loss_weight, a.loss_weight) == (1.0, 0.3)
    assert (d.sampler.thresh, d.sampler.min_kept) == (0.7, 50) and a.sampler is None and d.impl == a.impl == "hip"
    m = R.build_model(R.get_args(small + ["--ohem_min_kept", "50"]))
    assert m.decode_head.loss_decode.sampler.mode == 2 and m.auxiliary_head.loss_decode.sampler is None
    assert m.auxiliary_head.loss_decode.class_weight is None


# ---------------------------------------------------------------- tools/seg_class_weights.py
def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_seg_class_weights", os.path.join(ROOT, "tools", "seg_class_weights.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_class_weights_on_a_toy_set_by_hand():
    T = _tool()
    labels = [np.array([[0, 0, 0, 0], [1, 1, 255, 255]], np.uint8), np.array([[0, 0, 0, 0], [2, 3, 9, 255]], np.uint8),
              np.array([[1, 1, 0, 0]], np.uint8)]
    assert T.count_pixels(labels, 4).tolist() == [10, 4, 1, 1]       # 255 and 9 are left out
    counts3 = T.count_pixels(labels, 3)                              # and so is 3 when there are three classes
    assert counts3.tolist() == [10, 4, 1]
    freq, weight = T.median_frequency_weights(counts3)
    assert freq.tolist() == [10 / 15, 4 / 15, 1 / 15]
    assert weight.tolist() == pytest.approx([0.4, 1.0, 4.0])         # median frequency 4/15
    freq, weight = T.median_frequency_weights([6, 0, 2, 0])          # absent classes: weight 0, outside the median
    assert freq.tolist() == [0.75, 0.0, 0.25, 0.0] and weight.tolist() == pytest.approx([0.5 / 0.75, 0.0, 2.0, 0.0])
    assert T.median_frequency_weights([0, 0])[1].tolist() == [0.0, 0.0]


def test_class_weights_tool_on_the_synthetic_root(tmp_path):
    from mem_amd import run_semseg as R
    from mem_amd.seg_data import EventSegDataset, SegPipelineConfig
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "seg_class_weights.py"), "--data_root", "synthetic", "--num_classes", "5",
                        "--synthetic_samples", "3", "--canvas", "44", "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    ds = EventSegDataset("synthetic", "train", SegPipelineConfig(canvas=(44, 64), img_scale=(44, 64), crop_size=(44, 64)), n_synthetic=3, num_classes=5)
    want = np.zeros(5, np.int64)
    for i in range(3):
        lab = ds.load(i)[1]
        want += np.bincount(lab[lab != 255].astype(np.int64), minlength=5)
    assert rec["pixel_counts"] == want.tolist() and rec["samples"] == 3 and rec["num_classes"] == 5
    assert sum(rec["pixel_counts"]) == 3 * 44 * (64 - 1)             # the ignored band of one column
    freq = want / want.sum()
    med = np.median(freq[freq > 0])
    assert rec["frequencies"] == pytest.approx(freq.tolist())
    assert rec["class_weight"] == pytest.approx([med / f if f > 0 else 0.0 for f in freq])
    out = tmp_path / "cw.json"
    out.write_text(lines[0])
    assert R.get_args(["--num_classes", "5", "--class_weight", str(out)]).class_weight == rec["class_weight"]
