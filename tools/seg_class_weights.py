"""Class weights for the segmentation loss from the training labels, by median-frequency balancing.

Walks the label maps of ``EventSegDataset(root, "train")`` (``root/anns/train/*.png``, or the procedural samples of
``root="synthetic"``), counts the pixels of every class (``ignore_index`` and labels >= the number of classes are left out) and
prints one JSON object::

    {"num_classes": K, "classes": [...], "samples": n, "ignore_index": 255,
     "pixel_counts": [..K..], "frequencies": [..K..], "class_weight": [..K..]}

``frequencies[c]`` = pixels of class c / counted pixels; ``class_weight[c]`` = median(freq over the classes that occur) /
freq[c], and 0 for a class that does not occur (it has no pixel to weigh).  The file is what ``python -m mem_amd.run_semseg
--class_weight <file>`` takes.  CPU only.

    python tools/seg_class_weights.py --data_root synthetic --num_classes 11 > class_weight.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def count_pixels(labels, num_classes, ignore_index=255):
    """int64 [num_classes]: the pixels of every class over an iterable of integer label maps"""
    counts = np.zeros(num_classes, dtype=np.int64)
    for lab in labels:
        lab = np.asarray(lab).reshape(-1).astype(np.int64)
        lab = lab[(lab != ignore_index) & (lab >= 0) & (lab < num_classes)]
        counts += np.bincount(lab, minlength=num_classes)
    return counts


def median_frequency_weights(counts):
    """(frequencies, class_weight) from pixel counts: median(freq of the classes that occur) / freq[c], 0 where freq[c] == 0"""
    counts = np.asarray(counts, dtype=np.float64)
    total = counts.sum()
    freq = counts / total if total > 0 else np.zeros_like(counts)
    present = freq > 0
    weight = np.zeros_like(freq)
    if present.any():
        weight[present] = np.median(freq[present]) / freq[present]
    return freq, weight


def dataset_labels(dataset):
    """the label map of every sample, without the events where files hold them"""
    if dataset.synthetic:
        for i in range(len(dataset)):
            yield dataset.load(i)[1]
    else:
        from PIL import Image
        for _, ann in dataset.pairs:
            yield np.asarray(Image.open(ann))


def class_weights(root, num_classes=11, ignore_index=255, n_synthetic=32, canvas=(440, 640)):
    from mem_amd.seg_data import EventSegDataset, SegPipelineConfig
    cfg = SegPipelineConfig(canvas=tuple(canvas), img_scale=tuple(canvas), crop_size=tuple(canvas))
    ds = EventSegDataset(root, "train", cfg, n_synthetic=n_synthetic, synthetic_events=16, num_classes=num_classes)
    K = len(ds.CLASSES)
    counts = count_pixels(dataset_labels(ds), K, ignore_index)
    freq, weight = median_frequency_weights(counts)
    return {"num_classes": K, "classes": list(ds.CLASSES), "samples": len(ds), "ignore_index": ignore_index,
            "pixel_counts": [int(c) for c in counts], "frequencies": [float(f) for f in freq],
            "class_weight": [float(w) for w in weight]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--data_root", default="synthetic", help="folder with imgs/train, anns/train, labels.txt, or 'synthetic'")
    ap.add_argument("--num_classes", type=int, default=11, help="synthetic root only; a folder's labels.txt names the classes")
    ap.add_argument("--ignore_index", type=int, default=255)
    ap.add_argument("--synthetic_samples", type=int, default=32)
    ap.add_argument("--canvas", type=int, nargs=2, default=[440, 640])
    a = ap.parse_args(argv)
    print(json.dumps(class_weights(a.data_root, a.num_classes, a.ignore_index, a.synthetic_samples, a.canvas)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
