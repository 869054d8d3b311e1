"""-m "not gpu": the finetuning recipe's host side -- ABI 7 symbols and argument validation of the four entry points, the
Mixup parameter draws against a plain-numpy restatement of timm's published draw order, and the stage-3 argument parser."""
import os

import numpy as np
import pytest

NEW = ("memhip_mixup", "memhip_mix_targets", "memhip_ce_soft", "memhip_ema_update")


def _lib():
    from mem_amd import _lib, ops  # noqa: F401  (ops declares the signatures)
    return _lib.lib


def test_abi7_exports_the_recipe_symbols():
    lib = _lib()
    assert lib.memhip_abi_version() == 10                                       # (the recipe came with 7; 8: the struct entry points; 9: the tokenizer's args struct; 10: the rasterizer's)
    for name in NEW:
        assert hasattr(lib, name), name


def _bad(rc, lib, word):
    assert rc == -1, rc
    assert word.encode() in lib.memhip_last_error(), lib.memhip_last_error()


def test_entries_validate_before_any_launch():
    """Null pointers and bad shapes return MEMHIP_EINVAL with a message; nothing is launched (no GPU here)."""
    import ctypes as C
    lib = _lib()
    _bad(lib.memhip_mixup(None, 2, 3, 8, 8, None, None, None, None, None), lib, "null pointer")
    _bad(lib.memhip_mixup(None, 0, 3, 8, 8, None, None, None, None, None), lib, "bad shape")
    box = np.array([[0, 4, 0, 4], [5, 3, 0, 4]], dtype=np.int32)            # second box: yh < yl
    lam = np.array([0.5, 0.5], dtype=np.float32)
    _bad(lib.memhip_mixup(None, 2, 3, 8, 8, None, None, lam.ctypes.data_as(C.c_void_p), box.ctypes.data_as(C.c_void_p), None),
         lib, "bad box[1]")
    box[1] = (0, 9, 0, 4)                                                       # beyond H = 8
    _bad(lib.memhip_mixup(None, 2, 3, 8, 8, None, None, None, box.ctypes.data_as(C.c_void_p), None), lib, "bad box[1]")
    lam[0] = 1.5
    _bad(lib.memhip_mixup(None, 2, 3, 8, 8, None, None, lam.ctypes.data_as(C.c_void_p), None, None), lib, "lam[0]")
    _bad(lib.memhip_mix_targets(None, None, 4, 1, 0.1, None, 1, None), lib, "bad shape")
    _bad(lib.memhip_mix_targets(None, None, 0, 10, 0.1, None, 10, None), lib, "bad shape")
    _bad(lib.memhip_mix_targets(None, None, 4, 10, 0.1, None, 10, None), lib, "null pointer")
    _bad(lib.memhip_ce_soft(None, 0, 8, None, 0, None, 0.0, 4, 1, 1.0, None, 0, None, None, 0, None, None), lib, "bad shape")
    _bad(lib.memhip_ce_soft(None, 0, 8, None, 0, None, 0.0, 0, 8, 1.0, None, 0, None, None, 0, None, None), lib, "bad shape")
    _bad(lib.memhip_ce_soft(None, 0, 4, None, 0, None, 0.0, 4, 8, 1.0, None, 0, None, None, 0, None, None), lib, "ld=")
    _bad(lib.memhip_ce_soft(None, 1, 101, None, 0, None, 0.0, 4, 101, 1.0, None, 0, None, None, 0, None, None), lib, "null pointer")
    _bad(lib.memhip_ema_update(None, None, 0, 0.5, None), lib, "n=0")
    _bad(lib.memhip_ema_update(None, None, 16, 0.5, None), lib, "null pointer")
    buf = np.zeros(8, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    _bad(lib.memhip_ema_update(p, p, 8, 1.5, None), lib, "decay")
    # ce_soft wants exactly one target form
    lab = np.zeros(4, dtype=np.int64).ctypes.data_as(C.c_void_p)
    _bad(lib.memhip_ce_soft(p, 1, 2, p, 2, lab, 0.0, 4, 2, 1.0, None, 0, p, p, 0, p, None), lib, "not both")


# ------------------------------------------------------------------ Mixup draws: a plain-numpy restatement, seeded identically
def _ref_box(r, H, W, lam, minmax, correct):
    if minmax is not None:
        ch = r.randint(int(H * minmax[0]), int(H * minmax[1]))
        cw = r.randint(int(W * minmax[0]), int(W * minmax[1]))
        yl = r.randint(0, H - ch)
        xl = r.randint(0, W - cw)
        yh, xh = yl + ch, xl + cw
    else:
        ratio = np.sqrt(1 - lam)
        ch, cw = int(H * ratio), int(W * ratio)
        cy = r.randint(0, H)
        cx = r.randint(0, W)
        yl, yh = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
        xl, xh = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
    if correct or minmax is not None:
        lam = 1. - (yh - yl) * (xh - xl) / float(H * W)
    return (yl, yh, xl, xh), lam


def _ref_draw(r, B, H, W, mode, ma, ca, minmax, prob, switch, correct):
    if minmax is not None:
        ca = 1.0
    lam = np.ones(B, np.float32)
    box = np.zeros((B, 4), np.int32)
    if mode == "batch":
        if not r.rand() < prob:
            return lam, box
        if ma > 0 and ca > 0:
            cut = r.rand() < switch
            l = r.beta(ca, ca) if cut else r.beta(ma, ma)
        elif ma > 0:
            cut, l = False, r.beta(ma, ma)
        else:
            cut, l = True, r.beta(ca, ca)
        l = float(l)
        if l != 1. and cut:
            b, l = _ref_box(r, H, W, l, minmax, correct)
            box[:] = b
        lam[:] = l
        return lam, box
    n = B if mode == "elem" else B // 2
    if ma > 0 and ca > 0:
        cut = r.rand(n) < switch
        lc = r.beta(ca, ca, size=n)
        lm = r.beta(ma, ma, size=n)
        mix = np.where(cut, lc, lm)
    elif ma > 0:
        cut, mix = np.zeros(n, bool), r.beta(ma, ma, size=n)
    else:
        cut, mix = np.ones(n, bool), r.beta(ca, ca, size=n)
    ln = np.where(r.rand(n) < prob, mix.astype(np.float32), np.float32(1)).astype(np.float32)
    for i in range(n):
        if ln[i] != 1 and cut[i]:
            b, l = _ref_box(r, H, W, ln[i], minmax, correct)
            box[i] = b
            ln[i] = l
    lam[:n] = ln
    if mode == "pair":
        for i in range(n):
            lam[B - 1 - i] = ln[i]
            box[B - 1 - i] = box[i]
    return lam, box


CASES = [dict(ma=0.8, ca=0.0), dict(ma=0.0, ca=1.0), dict(ma=0.8, ca=1.0), dict(ma=0.0, ca=0.0, minmax=(0.2, 0.8)),
         dict(ma=0.8, ca=1.0, correct=False), dict(ma=0.4, ca=0.0, minmax=(0.1, 0.5))]


@pytest.mark.parametrize("mode", ["batch", "elem", "pair"])
@pytest.mark.parametrize("prob", [0.0, 0.5, 1.0])
def test_mixup_draws_equal_the_restatement_bit_for_bit(mode, prob):
    from mem_amd.mixup import Mixup
    B, H, W = 8, 64, 96
    seen = {"mixup": 0, "cutmix": 0, "identity": 0}
    for ci, c in enumerate(CASES):
        seed = 100 * ci + 7
        m = Mixup(mixup_alpha=c["ma"], cutmix_alpha=c["ca"], cutmix_minmax=c.get("minmax"), prob=prob, switch_prob=0.5,
                  mode=mode, correct_lam=c.get("correct", True), rng=np.random.RandomState(seed))
        r = np.random.RandomState(seed)
        for _ in range(12):
            lam, box = m.draw(B, H, W)
            rl, rb = _ref_draw(r, B, H, W, mode, c["ma"], c["ca"], c.get("minmax"), prob, 0.5, c.get("correct", True))
            assert lam.dtype == np.float32 and box.dtype == np.int32 and lam.shape == (B,) and box.shape == (B, 4)
            assert np.array_equal(lam.view(np.uint32), rl.view(np.uint32)), (c, lam, rl)
            assert np.array_equal(box, rb), (c, box, rb)
            area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
            assert (box[:, 0] >= 0).all() and (box[:, 1] <= H).all() and (box[:, 2] >= 0).all() and (box[:, 3] <= W).all()
            seen["cutmix"] += int((area > 0).any())
            seen["mixup"] += int(((area == 0) & (lam < 1)).any())
            # (per sample in elem / pair: a whole batch of B = 8 left alone at prob 0.5 is a 1-in-256 event)
            same = (lam == 1) & (area == 0)
            seen["identity"] += int(same.all() if mode == "batch" else same.any())
    # no branch passes by never being taken
    if prob > 0:
        assert seen["mixup"] > 0 and seen["cutmix"] > 0, seen
    if prob < 1:
        assert seen["identity"] > 0, seen
    if prob == 0:
        assert seen["mixup"] == 0 and seen["cutmix"] == 0


def test_mixup_default_stream_is_numpy_global_state():
    """Like timm: without rng= the draws come from numpy's global state, so seeding numpy reproduces the sequence."""
    from mem_amd.mixup import Mixup
    m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem")
    np.random.seed(11)
    a = [m.draw(6, 32, 32) for _ in range(3)]
    r = np.random.RandomState(11)
    for lam, box in a:
        rl, rb = _ref_draw(r, 6, 32, 32, "elem", 0.8, 1.0, None, 1.0, 0.5, True)
        assert np.array_equal(lam, rl) and np.array_equal(box, rb)
    with pytest.raises(AssertionError):
        Mixup()(__import__("torch").zeros(3, 3, 8, 8), None)                    # odd batch, as timm asserts


# ------------------------------------------------------------------ stage-3 argument parser
def test_get_args_parses_the_ncaltech_key_set(tmp_path):
    from mem_amd.run_class_finetuning import get_args
    from conftest import GOLDEN
    conf = os.path.join(GOLDEN, "ncaltech_keys.conf")
    a = get_args(["--config", str(conf), "--class_layer_decay", "0.75", "--nb_classes", "101"])
    assert (a.epochs, a.update_freq, a.batch_size, a.lr, a.warmup_epochs, a.drop, a.weight_decay, a.save_ckpt_freq) == \
        (300, 2, 1024, 4e-3, 20, 0.1, 5e-2, 25)
    assert (a.input_H, a.input_W, a.data_set, a.max_random_shift_evs, a.transformer_emb, a.expweek) == (224, 224, "npy", 8, 768,
                                                                                                       "2023-01")
    assert a.layer_decay == 0.75 and a.nb_classes == 101
    # the reference's defaults of the recipe
    assert a.model_ema is True and a.model_ema_decay == 0.9999 and a.smoothing == 0.1 and a.mixup == 0.8 and a.cutmix == 1.0
    assert a.mixup_prob == 0.0 and a.mixup_mode == "batch" and a.auto_resume is True and a.eval is False
    b = get_args(["--expweek", "x", "--lr", "1e-3", "--eval", "--no_auto_resume", "--mixup_prob", "1.0"])
    assert b.lr == 1e-3 and b.eval and not b.auto_resume and b.mixup_prob == 1.0


@pytest.mark.parametrize("flag,argv", [
    ("enable_deepspeed", ["--enable_deepspeed"]), ("linear_probe", ["--linear_probe"]),
    ("attn_drop_rate", ["--attn_drop_rate", "0.1"]), ("model_ema_force_cpu", ["--model_ema_force_cpu"]),
    ("data_set", ["--data_set", "IMNET"]), ("data_set", ["--data_set", "CIFAR"]), ("data_set", ["--data_set", "image_folder"]),
    ("data_set", ["--data_set", "dsec_semseg"]), ("aa", ["--aa", "rand-m9-mstd0.5-inc1"]), ("reprob", ["--reprob", "0.25"])])
def test_not_carried_flags_raise_with_their_own_name(flag, argv):
    from mem_amd.run_class_finetuning import get_args
    with pytest.raises(NotImplementedError) as e:
        get_args(["--expweek", "x"] + argv)
    msg = str(e.value)
    assert msg.startswith("--" + flag) and "\n" not in msg, msg


def test_criterion_follows_the_three_way_choice():
    import torch
    from mem_amd.loss import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    from mem_amd.run_class_finetuning import build_criterion, get_args
    a = get_args(["--expweek", "x"])
    assert isinstance(build_criterion(a, object()), SoftTargetCrossEntropy)
    c = build_criterion(a, None)
    assert isinstance(c, LabelSmoothingCrossEntropy) and c.smoothing == 0.1
    a.smoothing = 0.0
    assert isinstance(build_criterion(a, None), torch.nn.CrossEntropyLoss)


def test_model_ema_refuses_cpu():
    from mem_amd import utils
    with pytest.raises(NotImplementedError, match="no CPU path"):
        utils.ModelEma(object(), device="cpu")
