"""Inputs for the config entry points: seeded synthetic images, `ImageListFiles`, real pairs from the reference's `lq hq label`
list files, `CorruptedImageFiles`, clean images corrupted on the GPU (unirestore_amd.corrupt), and `JpegImageFiles`, clean images
JPEG-compressed on the GPU at a list of qualities (unirestore_amd.jpeg), and `DistortedImageFiles`, CorruptedImageFiles for glass blur,
snow and elastic transform (unirestore_amd.distort).  The last three share `_DegradedImageFiles`: the constructor checks and the load /
degrade / yield loop are written once there.  The four file datasets take `labels=True`: gt is then the int64 labels of the list's
third column (what a classifier is scored against) instead of None; `labels="map"`: the third column is the path of a label PNG
and gt the int64 [B,H,W] label maps (what a segmenter is scored against), Cityscapes labelIds mapped to trainIds by default;
`labels="boxes"`: the third column is the path of an annotation JSON and gt a list of {boxes, labels} (what a detector is scored
against), the names mapped to COCO ids by `box_classes`.

`SyntheticImages` yields the evaluator's batch tuple `(lq, hq, gt, fname, task)` (reference
src/core/base/eval_image_restoration.py:56) from seeded random images: hq = torch.rand (what the reference's own smoke
test feeds, src/modules/diffuie/autoencoder.py:209), lq = hq under one of three cost-neutral degradations
(SURVEY.md 8d): additive N(0, 0.1) noise, haze 0.5*x + 0.5, low light 0.3*x.  Content does not change the cost of the path.
"""
from typing import Iterator, List, Sequence, Tuple

import torch

from . import corrupt, distort, jpeg

DEGRADATIONS = ("noise", "haze", "lowlight")


def degrade(hq: torch.Tensor, kind: str, generator: torch.Generator = None) -> torch.Tensor:
    if kind == "noise":
        return (hq + 0.1 * torch.randn(hq.shape, generator=generator, device=hq.device)).clamp(0, 1)
    if kind == "haze":
        return 0.5 * hq + 0.5
    if kind == "lowlight":
        return 0.3 * hq
    raise ValueError(f"unknown degradation {kind!r}: choose from {DEGRADATIONS}")


class SyntheticImages:
    def __init__(self, task: str = "ir", resolution: Sequence[int] = (512, 512), batch_size: int = 8, num_batches: int = 5,
                 degradations: Sequence[str] = ("noise",), seed: int = 42):
        for d in degradations:
            if d not in DEGRADATIONS:
                raise ValueError(f"unknown degradation {d!r}: choose from {DEGRADATIONS}")
        if isinstance(resolution, int):
            resolution = (resolution, resolution)
        self.task, self.resolution, self.batch_size, self.num_batches = task, tuple(resolution), int(batch_size), int(num_batches)
        self.degradations, self.seed = list(degradations), seed

    def __len__(self):
        return self.num_batches

    def batches(self, rank: int = 0, world: int = 1, device="cpu") -> Iterator[Tuple[torch.Tensor, torch.Tensor, None, List[str], str]]:
        """Rank `rank`'s contiguous shard of every global batch (sizes differ by at most one image)."""
        from .dist import shard_range
        h, w = self.resolution
        lo, hi = shard_range(self.batch_size, rank, world)
        for b in range(self.num_batches):
            g = torch.Generator().manual_seed(self.seed + b)          # the GLOBAL batch is the same whatever the world size
            hq = torch.rand(self.batch_size, 3, h, w, generator=g)
            lq = torch.stack([degrade(hq[i], self.degradations[i % len(self.degradations)], g) for i in range(self.batch_size)])
            names = [f"syn_{b:04d}_{i:03d}" for i in range(lo, hi)]
            yield lq[lo:hi].to(device), hq[lo:hi].to(device), None, names, self.task


def read_labels(list_file: str) -> List[int]:
    """The integer labels of an `lq hq label` list, one per pair line in file order (blank and `#` lines skipped, as every reader of
    these lists does).  ValueError naming file and line for a line without a third column or with one that is no integer, and
    for a folder: labels exist in three-column lists only."""
    import os
    if os.path.isdir(list_file):
        raise ValueError(f"{list_file!r}: labels: true needs an `lq hq label` list file; a folder carries no labels")
    out = []
    with open(list_file) as f:
        for ln, line in enumerate(f, 1):
            cols = line.split()
            if not cols or cols[0].startswith("#"):
                continue
            if len(cols) < 3:
                raise ValueError(f"{list_file}:{ln}: labels: true needs `lq hq label`, got {line.strip()!r} (no label column)")
            try:
                out.append(int(cols[2]))
            except ValueError:
                raise ValueError(f"{list_file}:{ln}: the label {cols[2]!r} is not an integer") from None
    return out


LABEL_ENCODINGS = ("cityscapes", "train_id")
# the public Cityscapes labelId -> trainId table (cityscapesScripts, labels.py): the 19 evaluated classes; every other id is 255
CITYSCAPES_TRAIN_ID = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15,
                       31: 16, 32: 17, 33: 18}


BOX_CLASSES = ("rtts", "coco")
# the reference's two name -> COCO id tables (dataset_det.py): RTTS's five classes, and the 91-entry COCO category list by position
RTTS_COCO_IDS = {"person": 1, "bicycle": 2, "car": 3, "bus": 6, "motorbike": 4}
COCO_NAMES = ("__background__", "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light",
              "fire hydrant", "N/A", "stop sign", "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow", "elephant", "bear",
              "zebra", "giraffe", "N/A", "backpack", "umbrella", "N/A", "N/A", "handbag", "tie", "suitcase", "frisbee", "skis", "snowboard",
              "sports ball", "kite", "baseball bat", "baseball glove", "skateboard", "surfboard", "tennis racket", "bottle", "N/A",
              "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple", "sandwich", "orange", "broccoli", "carrot", "hot dog",
              "pizza", "donut", "cake", "chair", "couch", "potted plant", "bed", "N/A", "dining table", "N/A", "N/A", "toilet", "N/A", "tv",
              "laptop", "mouse", "remote", "keyboard", "cell phone", "microwave", "oven", "toaster", "sink", "refrigerator", "N/A", "book",
              "clock", "vase", "scissors", "teddy bear", "hair drier", "toothbrush")
COCO_IDS = {name: i for i, name in enumerate(COCO_NAMES)}


def check_labels_arg(labels, label_encoding, box_classes="rtts"):
    if labels not in (False, True, "map", "boxes"):
        raise ValueError("labels must be false, true (an integer per line), \"map\" (a label PNG per line) or \"boxes\" (an annotation "
                         f"JSON per line), got {labels!r}")
    if label_encoding not in LABEL_ENCODINGS:
        raise ValueError(f"unknown label_encoding {label_encoding!r}: choose from {LABEL_ENCODINGS}")
    if box_classes not in BOX_CLASSES:
        raise ValueError(f"unknown box_classes {box_classes!r}: choose from {BOX_CLASSES}")


def load_boxes(path: str, box_classes: str, where: str) -> dict:
    """One annotation JSON in the reference's format as {boxes float32 [n,4] (xmin, ymin, xmax, ymax), labels int64 [n]}: every
    top-level key that contains `object` holds {"name", "bndbox": {xmin, ymin, xmax, ymax}}; a box with xmax <= xmin or ymax <= ymin
    is skipped.  ValueError naming `where` (file:line of the list) when the file is missing or malformed, a name is not in the
    class table, or no box is left (the reference refuses such an image as well)."""
    import json
    import os
    if not os.path.isfile(path):
        raise ValueError(f"{where}: the annotation file {path!r} does not exist")
    table = RTTS_COCO_IDS if box_classes == "rtts" else COCO_IDS
    boxes, labels = [], []
    try:
        with open(path) as f:
            ann = json.load(f)
        for key, v in ann.items():
            if "object" not in key:
                continue
            bb = v["bndbox"]
            try:
                x0, y0, x1, y1 = (float(bb[k]) for k in ("xmin", "ymin", "xmax", "ymax"))
            except ValueError as e:
                raise TypeError(f"a coordinate of {key!r} is no number: {e}") from None
            if x1 > x0 and y1 > y0:
                if v["name"] not in table:
                    raise ValueError(f"{where}: {path!r}: the class {v['name']!r} is not in the {box_classes!r} table")
                boxes.append([x0, y0, x1, y1])
                labels.append(table[v["name"]])
    except (KeyError, TypeError, AttributeError, json.JSONDecodeError) as e:
        raise ValueError(f"{where}: {path!r} is no annotation file of the expected form ({type(e).__name__}: {e})") from None
    if not boxes:
        raise ValueError(f"{where}: {path!r} holds no valid box")
    return {"boxes": torch.tensor(boxes, dtype=torch.float32).view(-1, 4), "labels": torch.tensor(labels, dtype=torch.int64)}


def crop_boxes(gt: list, top: int, left: int, height: int, width: int) -> list:
    """The targets of a batch under a crop of its images to rows top .. top + height, columns left .. left + width: the boxes
    shifted by the offset and clipped to the crop; a box left without area is dropped with its label."""
    out = []
    for t in gt:
        b = t["boxes"].clone().view(-1, 4)
        b[:, 0::2] = (b[:, 0::2] - left).clamp(0, width)
        b[:, 1::2] = (b[:, 1::2] - top).clamp(0, height)
        keep = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
        out.append({"boxes": b[keep], "labels": t["labels"][keep]})
    return out


def read_label_paths(list_file: str) -> List[Tuple[str, int]]:
    """(path, line number) of the label map of every pair line of an `lq hq label.png` list, in file order; a relative path is taken
    from the list file's folder, exactly as the first two columns are.  ValueError naming file and line for a line without a third
    column, and for a folder: label maps exist in three-column lists only."""
    import os
    if os.path.isdir(list_file):
        raise ValueError(f"{list_file!r}: labels: map needs an `lq hq label.png` list file; a folder carries no labels")
    base = os.path.dirname(os.path.abspath(list_file))
    out = []
    with open(list_file) as f:
        for ln, line in enumerate(f, 1):
            cols = line.split()
            if not cols or cols[0].startswith("#"):
                continue
            if len(cols) < 3:
                raise ValueError(f"{list_file}:{ln}: labels: map needs `lq hq label.png`, got {line.strip()!r} (no label column)")
            out.append((cols[2] if os.path.isabs(cols[2]) else os.path.join(base, cols[2]), ln))
    return out


def load_label_map(path: str, encoding: str, hw, where: str) -> torch.Tensor:
    """One label PNG (8-bit, one channel) as int64 [H,W].  encoding "cityscapes": labelIds 0..33 go through CITYSCAPES_TRAIN_ID,
    everything else becomes 255; "train_id": the values as they are.  ValueError naming `where` (file:line of the list) when the
    file is missing, is no single-channel 8-bit image or differs in size from its image (hw)."""
    import os

    import numpy as np
    from PIL import Image
    if not os.path.isfile(path):
        raise ValueError(f"{where}: the label map {path!r} does not exist")
    with Image.open(path) as im:
        if im.mode not in ("L", "P"):
            raise ValueError(f"{where}: the label map {path!r} has mode {im.mode}, expected a single-channel 8-bit image")
        a = torch.from_numpy(np.array(im, dtype=np.uint8))
    if tuple(a.shape) != tuple(hw):
        raise ValueError(f"{where}: the label map {path!r} is {a.shape[0]} x {a.shape[1]}, its image {hw[0]} x {hw[1]}")
    if encoding == "cityscapes":
        lut = torch.full((256,), 255, dtype=torch.int64)
        for k, v in CITYSCAPES_TRAIN_ID.items():
            lut[k] = v
        return lut[a.long()]
    return a.long()


class _Labels:
    """The `labels` / `label_encoding` arguments of the file datasets: gt of a batch from the list's third column."""

    def __init__(self, list_file, labels, label_encoding, box_classes="rtts"):
        check_labels_arg(labels, label_encoding, box_classes)
        self.kind, self.encoding, self.list_file, self.box_classes = labels, label_encoding, list_file, box_classes
        self.values = read_label_paths(list_file) if labels in ("map", "boxes") else read_labels(list_file) if labels else None

    def gt(self, idx, hw):
        if self.values is None:
            return None
        if self.kind == "boxes":
            return [load_boxes(self.values[i][0], self.box_classes, f"{self.list_file}:{self.values[i][1]}") for i in idx]
        if self.kind == "map":
            return torch.stack([load_label_map(self.values[i][0], self.encoding, hw, f"{self.list_file}:{self.values[i][1]}") for i in idx])
        return torch.tensor([self.values[i] for i in idx], dtype=torch.int64)


class ImageListFiles:
    """Real pairs for `validate` (`data.class_path: unirestore_amd.data.ImageListFiles`): a text file with one `lq hq [label]`
    line per pair, paths relative to the list file's folder.  Yields the evaluator's tuple `(lq, hq, gt, fname, task)` with lq / hq
    fp32 NCHW in [0, 1] (u8 / 255, the reference's ToDtype(scale=True)); pairs are grouped by shape, list order kept inside a
    group, so every batch is one tensor (the evaluator's centre crop makes nearly everything 512 x 512).  labels=True: gt is an
    int64 [B] tensor of the lines' third column (a classifier's targets) instead of None.  labels="map": the third column is the
    path of a label PNG of the lq image's size and gt the int64 [B,H,W] maps (a segmenter's targets); label_encoding "cityscapes"
    (the default) maps labelIds to trainIds, 255 for the rest, "train_id" takes the values as they are.  labels="boxes": the third
    column is the path of an annotation JSON (load_boxes) and gt a list of {boxes float32 [n,4], labels int64 [n]} (a detector's
    targets), the class names mapped to COCO ids by box_classes "rtts" (the default) or "coco".  The three degrading datasets take
    the same two arguments; a degradation never touches the boxes."""

    def __init__(self, list_file: str, batch_size: int = 8, task: str = "ir", num_batches: int = None, labels=False,
                 label_encoding: str = "cityscapes", box_classes: str = "rtts"):
        import os
        self.list_file, self.batch_size, self.task, self.num_batches = list_file, int(batch_size), task, num_batches
        self._labels = _Labels(list_file, labels, label_encoding, box_classes)
        self.labels = self._labels.values
        base = os.path.dirname(os.path.abspath(list_file))
        self.pairs = []
        with open(list_file) as f:
            for ln, line in enumerate(f, 1):
                cols = line.split()
                if not cols or cols[0].startswith("#"):
                    continue
                if len(cols) < 2:
                    raise ValueError(f"{list_file}:{ln}: expected `lq hq [label]`, got {line.strip()!r}")
                self.pairs.append(tuple(c if os.path.isabs(c) else os.path.join(base, c) for c in cols[:2]))
        if not self.pairs:
            raise ValueError(f"{list_file}: no `lq hq [label]` line")

    def _plan(self):
        from .imageio import scan
        groups = {}
        for i, (_, hw) in enumerate(scan(lq for lq, _ in self.pairs)):
            groups.setdefault(hw, []).append(i)
        cuts = [idx[s:s + self.batch_size] for idx in groups.values() for s in range(0, len(idx), self.batch_size)]
        cuts.sort(key=lambda c: c[0])
        return cuts[:self.num_batches]

    def __len__(self):
        return len(self._plan())

    def batches(self, rank: int = 0, world: int = 1, device="cpu") -> Iterator[Tuple[torch.Tensor, torch.Tensor, None, List[str], str]]:
        import os

        from .imageio import load_u8
        if world != 1:
            raise ValueError("ImageListFiles does not shard a batch over ranks (batches of real files differ in size): run "
                             "`validate` on one GPU, or restore the files with `cli restore`, which spreads batches over ranks")

        def nchw(paths):
            return torch.stack([load_u8(p).permute(2, 0, 1) for p in paths]).float().div(255).to(device)
        for idx in self._plan():
            lq, hq = nchw([self.pairs[i][0] for i in idx]), nchw([self.pairs[i][1] for i in idx])
            if lq.shape != hq.shape:
                raise ValueError(f"{self.list_file}: lq and hq of {self.pairs[idx[0]][0]!r}... differ in size: {tuple(lq.shape)} vs {tuple(hq.shape)}")
            gt = self._labels.gt(idx, lq.shape[2:])
            yield lq, hq, gt, [os.path.splitext(os.path.basename(self.pairs[i][0]))[0] for i in idx], self.task


class _DegradedImageFiles:
    """Clean image files degraded on the GPU, what the three datasets below share: the common constructor arguments, the plan's
    length and the loop over it.  A subclass gives `_plan()` -> the batches, each a tuple that ends in the batch's file indices,
    and `_degrade(hq, stems, *what)` -> (lq, label): `what` is the rest of that tuple, `label` what `last` holds after the batch."""

    def __init__(self, source, batch_size, task, seed, num_batches, resize, min_side, labels=False, label_encoding="cityscapes",
                 box_classes="rtts"):
        from . import resize as rz
        self.resize = None if resize is None else rz.check_range(resize, min_side)
        self.source, self.batch_size, self.task, self.seed, self.num_batches = source, int(batch_size), task, int(seed), num_batches
        if self.batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        self.paths = corrupt.check_inputs(source)
        self._labels = _Labels(source, labels, label_encoding, box_classes)         # one per line of the list, the order of `paths`
        self.labels = self._labels.values
        self.last = None

    def __len__(self):
        return len(self._plan())

    def batches(self, rank: int = 0, world: int = 1, device="cpu") -> Iterator[Tuple[torch.Tensor, torch.Tensor, None, List[str], str]]:
        from .imageio import load_u8
        if world != 1:
            raise ValueError(f"{type(self).__name__} does not shard a batch over ranks (batches of real files differ in size): run "
                             "`validate` on one GPU")
        # u8 / 255 as the host computes it, the values ImageListFiles yields for the same bytes (a device division by a scalar may
        # multiply by the reciprocal and differ in the last bit)
        unit = (torch.arange(256, dtype=torch.float32) / 255).to(device)

        def nchw(t):
            return unit.index_select(0, t.permute(0, 3, 1, 2).reshape(-1).int()).view(t.shape[0], 3, t.shape[1], t.shape[2])
        for *what, idx in self._plan():
            stems = [corrupt.stem_of(self.paths[i]) for i in idx]
            hq = torch.stack([load_u8(self.paths[i]) for i in idx]).to(device)
            lq, self.last = self._degrade(hq, stems, *what)
            gt = self._labels.gt(idx, hq.shape[1:3])                   # a label map passes through untouched: only the image is degraded
            yield nchw(lq), nchw(hq), gt, stems, self.task


class CorruptedImageFiles(_DegradedImageFiles):
    """Clean images corrupted on the GPU for `validate` (`data.class_path: unirestore_amd.data.CorruptedImageFiles`): `source` is a
    folder, a list file of clean images or an `lq hq [label]` list, of which only the hq column is read.  `corruptions` is a subset
    name (unirestore_amd.corrupt.SUBSETS), a name, or a comma-separated string / list of names ("clean" only when it is named);
    `severity` an integer 1..5 or "mixed", the reference's per-image draw.  Every image's corruption, severity and randomness come
    from sha256 of (seed, file stem) alone.  Images are grouped by (shape, corruption, severity), so a batch is homogeneous; hq is
    uploaded as u8 and corrupted there.  Yields `(lq, hq, gt, names, task)` with fp32 NCHW tensors in [0, 1], gt None or, with
    labels=True (an `lq hq label` list only), the int64 [B] labels of the list's third column, or with labels="map" the int64 [B,H,W]
    label maps it names (see ImageListFiles; a map is never degraded); `last` holds the
    (corruption, severity) of the batch just yielded and `skipped` the subset members that are not built.  `resize` = [lo, hi]
    (lo >= 32) turns on the reference's resize-down / resize-back wrapper (corrupt.degrade): every image's short edge is drawn
    from [lo, hi) by (seed, stem) as well, lq keeps hq's shape; the reference's own range is [resolution // 4, resolution)."""

    _planner = corrupt                             # the module whose expand / degrade this class uses (DistortedImageFiles: distort)

    def __init__(self, source: str, corruptions="common", severity=3, batch_size: int = 8, task: str = "ir", seed: int = 42,
                 num_batches: int = None, labels=False, label_encoding: str = "cityscapes", box_classes: str = "rtts", resize=None):
        super().__init__(source, batch_size, task, seed, num_batches, resize, 32, labels, label_encoding, box_classes)
        self.names = self._planner.expand(corruptions)
        self.skipped = corrupt.skipped(corruptions)
        self.severity = severity if severity == "mixed" else corrupt.check_severity(severity)

    def _plan(self):
        from .imageio import scan
        sizes = [hw for _, hw in scan(self.paths)]
        return corrupt.plan_files(self.paths, sizes, self.names, self.severity, self.seed, self.batch_size)[:self.num_batches]

    def _degrade(self, hq, stems, name, sev):
        return self._planner.degrade(hq, name, sev, self.seed, stems, self.resize), (name, sev)


class DistortedImageFiles(CorruptedImageFiles):
    """CorruptedImageFiles for glass blur, snow and elastic transform (unirestore_amd.distort; `data.class_path:
    unirestore_amd.data.DistortedImageFiles`): `corruptions` is "all", a name, or a comma-separated string / list of names of
    distort.NAMES; everything else - `source`, `severity`, `seed`, `resize`, the grouping, what is yielded and `last` - is the base
    class's, with distort.degrade in the place of corrupt.degrade.  `skipped` is empty: a name that is not built is refused."""
    _planner = distort

    def __init__(self, source: str, corruptions="all", severity=3, batch_size: int = 8, task: str = "ir", seed: int = 42,
                 num_batches: int = None, labels=False, label_encoding: str = "cityscapes", box_classes: str = "rtts", resize=None):
        super().__init__(source, corruptions, severity, batch_size, task, seed, num_batches, labels, label_encoding, box_classes, resize)
        self.skipped = []


class JpegImageFiles(_DegradedImageFiles):
    """Clean images JPEG-compressed on the GPU for `validate` (`data.class_path: unirestore_amd.data.JpegImageFiles`): `source` is
    read as CorruptedImageFiles reads it (a folder, a list file of clean images, or the hq column of an `lq hq [label]` list).
    `quality` is one quality or a list of them (unirestore_amd.jpeg.quality_of: integers 1..100 or "s1".."s5"); EVERY image is
    taken at EVERY listed quality.  Images are grouped by (shape, quality), uploaded as u8 and compressed there (4:2:0, Pillow's
    and the reference's default).  Yields `(lq, hq, None, names, task)` with fp32 NCHW tensors in [0, 1], the values
    ImageListFiles yields for the same bytes; `last` holds ("jpeg", quality) of the batch just yielded.  `resize` = [lo, hi]
    (lo >= 16) turns on the reference's resize-down / resize-back wrapper (jpeg.degrade): every image's short edge is drawn from
    [lo, hi) by (`seed`, stem), the only use of `seed`; lq keeps hq's shape."""

    def __init__(self, source: str, quality=(10, 25, 50), batch_size: int = 8, task: str = "ir", num_batches: int = None,
                 labels=False, label_encoding: str = "cityscapes", box_classes: str = "rtts", resize=None, seed: int = 42):
        super().__init__(source, batch_size, task, seed, num_batches, resize, jpeg.MIN_SIDE, labels, label_encoding, box_classes)
        specs = [s for s in quality.split(",") if s] if isinstance(quality, str) else \
            list(quality) if isinstance(quality, (list, tuple)) else [quality]
        self.qualities = []
        for s in specs:
            q = jpeg.quality_of(s)
            if q not in self.qualities:
                self.qualities.append(q)
        if not self.qualities:
            raise ValueError("quality: name at least one quality")

    def _plan(self):
        from .imageio import scan
        sizes = [hw for _, hw in scan(self.paths)]
        return jpeg.plan_files(sizes, self.qualities, self.batch_size)[:self.num_batches]

    def _degrade(self, hq, stems, q):
        return jpeg.degrade(hq, q, self.seed, stems, self.resize), ("jpeg", q)
