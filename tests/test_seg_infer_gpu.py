"""-m gpu: mem_amd.infer_semseg on the device, on a checkpoint that mem_amd.run_semseg trains in two iterations: whole-image
evaluation repeats run_semseg's figures exactly; sliding windows with the flipped pass give the label maps of a float64 torch
restatement (mmseg's slide_inference -> softmax -> flip -> mean -> argmax) of the same encode_decode logits; the dump, the
class-index PNGs and the painted PNGs have the right count, size and mode."""
import json
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the 128-wide configuration of tests/test_semseg_run_gpu.py, on a 48 x 64 canvas; 96 x 128 pixels: the coarsest map is 3 x 4,
# what pool scale 3 needs
TINY = ["--vit", "tiny", "--embed_dim", "128", "--num_heads", "2", "--depth", "4", "--net_size", "96", "128", "--decode_channels", "64",
        "--aux_channels", "64", "--pool_scales", "1", "2", "3", "--canvas", "48", "64", "--crop_size", "48", "64",
        "--ratio_range", "1.0", "1.05", "--slice_max_evs", "5000", "--synthetic_samples", "8", "--synthetic_events", "8000",
        "--workers_per_gpu", "0", "--samples_per_gpu", "2", "--log_interval", "1"]
MODEL_DATA = TINY[:TINY.index("--log_interval")]          # the tool takes run_semseg's model and data flags, not its training flags
SLIDE = ["--test_mode", "slide", "--slide_crop", "32", "32", "--slide_stride", "16", "24", "--flip"]
MARGIN, LEFT_OUT = 1e-5, 1e-3


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """(the flags both entrypoints share, the checkpoint of a 2-iteration run).  The two steps are taken at lr 1e-2 without
    warm-up: at the default 5e-4 the classifier stays at its initialisation (std 0.01), the logits within 0.1 of each other,
    every softmax within 1e-2 of 1 / 11, and 0.55 % of the float64 margins below 1e-5 -- a model that decides nothing cannot
    meet the 0.1 % condition of the label comparison below."""
    from mem_amd import run_semseg as R
    work = str(tmp_path_factory.mktemp("seg_infer") / "work")
    source = ["--data_root", "synthetic", "--seed", "1"]
    out = R.main(R.get_args(TINY + source + ["--work_dir", work, "--lr", "1e-2", "--warmup_iters", "0", "--max_iters", "2", "--eval_interval", "100"]))
    assert out["checkpoints"] == [work + "/iter_2.pth"]
    return MODEL_DATA + source, out["checkpoints"][0]


def test_whole_mode_repeats_run_semsegs_evaluation_exactly(trained, capsys):
    from mem_amd import infer_semseg as T, run_semseg as R
    common, ckpt = trained
    want = R.main(R.get_args(common + ["--eval_only", "--resume", ckpt]))["eval"][0]
    capsys.readouterr()
    rec = T.main(T.get_args(common + ["--checkpoint", ckpt, "--eval"]))
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{") and "mIoU" in l]
    assert printed == [rec]
    assert (rec["test_mode"], rec["windows"], rec["flip"], rec["samples"], rec["iter"]) == ("whole", 1, False, 2, 2)
    for k in ("aAcc", "mIoU", "mAcc", "IoU"):
        assert rec[k] == want[k], (k, rec[k], want[k])
    assert len(rec["IoU"]) == 11 and 0.0 < rec["aAcc"] <= 1.0


def _restate(logits, rects, window, canvas):
    """float64: (P [B, C, H, W], its top-2 margin)"""
    V = len(rects)
    lg = logits.double().cpu()
    lg = lg.view((V, lg.shape[0] // V) + tuple(lg.shape[1:]))
    (H, W), (hc, wc) = canvas, window
    total = 0
    for f in (0, 1):
        preds = lg.new_zeros((lg.shape[1], lg.shape[2], H, W))
        count = lg.new_zeros((1, 1, H, W))
        for v, (y1, x1, vf) in enumerate(rects):
            if vf == f:
                preds += F.pad(F.interpolate(lg[v], size=(hc, wc), mode="bilinear", align_corners=False), (x1, W - x1 - wc, y1, H - y1 - hc))
                count[:, :, y1:y1 + hc, x1:x1 + wc] += 1
        Pf = F.softmax(preds / count, dim=1)
        total = total + (Pf.flip(3) if f else Pf)
    P = total / 2
    top = torch.topk(P, 2, dim=1).values
    return P, (top[:, 0] - top[:, 1]).numpy()


def test_slide_with_flip_against_the_restatement_and_the_tools_outputs(trained, tmp_path, capsys):
    from PIL import Image
    from mem_amd import infer_semseg as T
    from mem_amd.run_semseg import _loader
    common, ckpt = trained
    show, fmt, out = tmp_path / "show", tmp_path / "fmt", str(tmp_path / "res.pkl")
    # max_views_per_call 16 < 12 views x 2 samples: the model runs in two chunks into the stacked buffer
    rec = T.main(T.get_args(common + SLIDE + ["--checkpoint", ckpt, "--eval", "--out", out, "--show-dir", str(show)]))
    assert (rec["test_mode"], rec["windows"], rec["crop"], rec["stride"], rec["flip"]) == ("slide", 6, [32, 32], [16, 24], True)
    assert 0.0 <= rec["mIoU"] <= 1.0 and rec["shown"] == 2 and rec["out"] == out
    results = pickle.load(open(out, "rb"))
    assert len(results) == 2 and all(r.shape == (48, 64) and r.dtype == np.uint8 and int(r.max()) < 11 for r in results)
    pngs = sorted(show.glob("*.png"))
    assert [p.name for p in pngs] == ["synthetic_000000.png", "synthetic_000001.png"]
    for p in pngs:
        im = Image.open(p)
        assert im.size == (64, 48) and im.mode == "RGB"
    rec2 = T.main(T.get_args(common + SLIDE + ["--checkpoint", ckpt, "--format-only", "--imgfile_prefix", str(fmt)]))
    assert rec2["formatted"] == 2 and "mIoU" not in rec2
    for i, p in enumerate(sorted(fmt.glob("*.png"))):
        im = Image.open(p)
        assert im.size == (64, 48) and im.mode == "L" and np.array_equal(np.asarray(im), results[i])      # the same label maps
    assert len(list(fmt.glob("*.png"))) == 2
    # the label maps against the float64 restatement of the same logits (the same chunks as the tool's run above)
    args = T.get_args(common + SLIDE + ["--checkpoint", ckpt, "--eval"])
    inf, dataset, _ = T.build_inferencer(args)
    events, offsets, labels, draws = next(iter(_loader(dataset, [[(0, 0), (1, 0)]], 0)))
    logits, _ = inf.view_logits(events, offsets, draws)
    assert logits.shape[0] == 12 * 2 and logits.shape[1] == 11
    P, margin = _restate(logits, inf.rects, inf.window, inf.canvas)
    pred, prob = inf.predict(events, offsets, draws, return_prob=True)
    pred, prob = pred.cpu().numpy(), prob.cpu().double()
    sure = margin >= MARGIN
    left_out = 1.0 - float(sure.mean())
    err = float((prob - P).abs().max())
    print("slide + flip: left out %.4f %%, prob error %.3e, wrong on the margin %d; margin quantiles 1 %% / 50 %%: %.3e / %.3e" %
          (100 * left_out, err, int((pred[sure] != np.argmax(P.numpy(), 1)[sure]).sum()), np.quantile(margin, 0.01), np.quantile(margin, 0.5)))
    assert left_out <= LEFT_OUT
    assert np.array_equal(pred[sure], np.argmax(P.numpy(), 1)[sure])
    assert err <= MARGIN                                     # below the margin no counted label can flip; test_seg_predict_gpu.py
                                                             # holds prob to the project's rule
    for b in range(2):
        assert np.array_equal(pred[b][sure[b]], results[b][sure[b]])
