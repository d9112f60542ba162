"""Caller side of the hot path: what `LitUniFIE.forward` and `ImageRestorationEvaluator.validation_step` do around
`DiffUIE.forward` (reference src/core/engine_unifie.py:227-236, src/core/base/eval_image_restoration.py:53-72,113-136),
without Lightning.  The centre crop is index arithmetic on the caller's tensor; resize / pad / un-pad / 8-bit
quantisation run as HIP kernels inside the model's graph (`DiffUIE.forward(..., quantize=True)`).
"""
from typing import List, Sequence

import torch


def crop_box(h: int, w: int, upper_h: int = 512, upper_w: int = 512):
    """crop_tensor's window (eval_image_restoration.py:113-136): (top, bottom, left, right) of the centre crop.
    Note the reference's `h//2 - crop_h//2 : h//2 + crop_h//2` drops one row/column when the crop size is odd."""
    ch, cw = min(h, upper_h), min(w, upper_w)
    return h // 2 - ch // 2, h // 2 + ch // 2, w // 2 - cw // 2, w // 2 + cw // 2


DEFAULT_CROP = (512, 512)                               # the IR evaluator's; the reference's seg / multi-task ones use (960, 1664)


def crop_tensor(image: torch.Tensor, crop=DEFAULT_CROP) -> torch.Tensor:
    if image.ndim not in (3, 4):
        raise NotImplementedError                       # the reference raises here as well (:136)
    t, b, l, r = crop_box(image.shape[-2], image.shape[-1], crop[0], crop[1])
    return image[..., t:b, l:r]


def check_crop(crop):
    """(h, w) of a `crop` argument: two integers >= 1."""
    if not (isinstance(crop, (tuple, list)) and len(crop) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in crop)):
        raise ValueError(f"crop must be two integers (H, W) >= 1, got {crop!r}")
    return int(crop[0]), int(crop[1])


@torch.inference_mode()
def forward(model, inputs: Sequence[torch.Tensor], task: str, quantize: bool = False) -> List[torch.Tensor]:
    """LitUniFIE.forward: inputs = [hq, lq] (any subset) -> [enh_hq, enh_lq]; one model.forward per list item."""
    return [model.forward(imgs, task, quantize=quantize) for imgs in inputs]


@torch.inference_mode()
def forward_tasks(model, inputs: Sequence[torch.Tensor], tasks: Sequence[str], quantize: bool = False) -> List[dict]:
    """`forward` for several tasks: one model.forward_tasks per list item -> [{task: enh}, ...] (each item restored ONCE, decoded
    per task)."""
    return [model.forward_tasks(imgs, tasks, quantize=quantize) for imgs in inputs]


@torch.inference_mode()
def validation_step(model, lq: torch.Tensor, hq: torch.Tensor = None, task: str = "ir", need_crop: bool = True,
                    eval_types: Sequence[str] = ("lq",), tasks: Sequence[str] = None, crop=DEFAULT_CROP):
    """Steps 1-2 of ImageRestorationEvaluator.validation_step: crop, restore, quantise to 8 bit.  Returns (preds, hq).
    tasks: restore with `forward_tasks` instead - preds is then a list of {task: images}."""
    if need_crop:
        lq = crop_tensor(lq, crop) if "lq" in eval_types else lq
        hq = crop_tensor(hq, crop) if (hq is not None and "hq" in eval_types) else hq
    inputs = ([hq] if "hq" in eval_types and hq is not None else []) + ([lq] if "lq" in eval_types else [])
    if tasks is not None:
        return forward_tasks(model, inputs, tasks, quantize=True), hq
    return forward(model, inputs, task, quantize=True), hq


def psnr_per_image(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """PSNR of every image of the batch (fp64 [N]): skimage's peak_signal_noise_ratio per sample - what the reference's SKPSNR sums
    before dividing by the image count (eval_image_restoration.py:266-278)."""
    d = (pred.double().cpu() - target.double().cpu()) ** 2
    mse = d.reshape(d.shape[0], -1).mean(dim=1)
    return 10.0 * torch.log10(data_range ** 2 / mse)


def psnr(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> float:
    """`val_lq/psnr` of a batch: the MEAN OF THE PER-IMAGE PSNRs (not the PSNR of the batch-mean MSE: the two differ as soon as
    the images differ; eval_image_restoration.py:102-104,181,266-278)."""
    return float(psnr_per_image(pred, target, data_range).mean())


def ssim(pred: torch.Tensor, target: torch.Tensor, data_range: float = 1.0, win: int = 7) -> float:
    """Mean structural similarity, scikit-image's defaults (`structural_similarity`: uniform 7x7 window, K1 0.01, K2 0.03,
    sample covariance, borders of (win-1)//2 pixels dropped), averaged over channels and the batch - what the reference's
    `SKSSIM(data_range=1.0)` metric reports (eval_image_restoration.py:182)."""
    import torch.nn.functional as F
    x, y = pred.double().cpu(), target.double().cpu()
    c = x.shape[1]
    k = torch.full((c, 1, win, win), 1.0 / (win * win), dtype=torch.float64)
    filt = lambda t: F.conv2d(t, k, groups=c)                     # 'valid' = the cropped interior skimage averages over
    npx = win * win
    cov_norm = npx / (npx - 1.0)
    ux, uy = filt(x), filt(y)
    vx = cov_norm * (filt(x * x) - ux * ux)
    vy = cov_norm * (filt(y * y) - uy * uy)
    vxy = cov_norm * (filt(x * y) - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return float(s.mean())


# where the evaluator's PSNR / SSIM run: "cpu" = psnr_per_image / ssim above (host fp64); "gpu" = ops.image_metrics (HIP, fp64,
# totals kept on the device: no host sync per batch)
METRICS_DEVICES = ("cpu", "gpu")


class LitUniFIE:
    """The caller the reference builds around the path (`LitUniFIE{IR,MTL}`, src/core/engine_unifie.py:29-42,227-236 +
    ImageRestorationEvaluator.validation_step) without Lightning: owns a `DiffUIE`, maps `forward` over the input list and
    runs the evaluator's crop / restore / quantise / metric steps on a batch tuple `(lq, hq, gt, fname, task)`."""

    def __init__(self, model_kwargs: dict, save_image: bool = False, eval_mode: str = "FR", need_crop: bool = True,
                 dtype: str = "bf16", hf_root: str = None, model=None, metrics_device: str = "cpu", lpips_weights=None,
                 classifiers=None, segmenters=None, crop=DEFAULT_CROP, niqe_params=None, detectors=None, det_score: float = 0.05,
                 det_iou: float = 0.5, **_ignored):
        from . import checkpoint
        if metrics_device not in METRICS_DEVICES:
            raise ValueError(f"metrics_device={metrics_device!r}: choose from {METRICS_DEVICES}")
        self.metrics_device = metrics_device
        self.crop = check_crop(crop)                       # the centre crop's upper size (need_crop)
        self.model_kwargs, self.need_crop, self.eval_mode = model_kwargs, need_crop, eval_mode
        tedit = model_kwargs.get("tedit") or {}
        self.task_dict = tedit.get("task", [])
        self.model = model if model is not None else checkpoint.build_from_config(model_kwargs, hf_root=hf_root, dtype=dtype)
        self.totals = dict(psnr=0.0, ssim=0.0, images=0)
        # LPIPS (AlexNet, exact fp32 HIP kernels) is off unless weights are given: a (alexnet_path, lin_path) pair or a loaded
        # lpips.LpipsWeights.  It runs on the GPU whatever metrics_device says - the product has no CPU implementation of it.
        self.lpips_weights = None
        if lpips_weights is not None:
            from . import lpips
            self.lpips_weights = lpips_weights if isinstance(lpips_weights, lpips.LpipsWeights) else lpips.load_weights(*lpips_weights)
            self.totals["lpips"] = torch.zeros((), dtype=torch.float64, device=self.lpips_weights.device)
        # Classifier scoring of the "cls" output (ResNet top-1 accuracy, exact fp32 HIP kernels) is off unless classifiers are given:
        # {name: (arch, state-dict path) | classify.ClassifierWeights}.  Per name the totals hold the accuracy's counts as an int64
        # [3, classes] device tensor (tp_c, targets_c, predicted_c) for the restored images ("cls/<name>") and for the unrestored
        # inputs ("cls_input/<name>").  A total is REPLACED by a new tensor, never changed in place: callers keep the old one to
        # take differences.  A vit.ViTWeights, or an (arch, path) whose arch is one of vit.ARCHS, is a VisionTransformer under the same
        # keys, a swin.SwinWeights or an arch of swin.ARCHS a Swin-V2, an rvt.RVTWeights or an arch of rvt.ARCHS a Robust Vision
        # Transformer, a vgg.VGGWeights or an arch of vgg.ARCHS a VGG: update_classification tells the networks apart by the weights' type.
        self.classifiers = {}
        for name, spec in (classifiers or {}).items():
            from . import classify, rvt, swin, vgg, vit
            w = spec
            if not isinstance(spec, (classify.ClassifierWeights, vit.ViTWeights, swin.SwinWeights, rvt.RVTWeights, vgg.VGGWeights)):      # (arch, path): the arch's table names its module
                module = next((m for m in (vit, swin, rvt, vgg) if isinstance(spec[0], str) and spec[0] in m.ARCHS), classify)
                w = module.load_weights(*spec)
            self.classifiers[name] = w
            for key in self.classifier_keys(name):
                self.totals[key] = torch.zeros(3, w.num_classes, dtype=torch.int64, device=w.device)

        # Segmenter scoring of the "seg" output (RefineNet-LW mIoU, exact fp32 HIP kernels) is off unless segmenters are given:
        # {name: (arch, state-dict path) | segment.SegmenterWeights}.  Per name the totals hold the confusion matrix conf[target][pred]
        # as an int64 [classes, classes] device tensor for the restored images ("seg/<name>") and for the unrestored inputs
        # ("seg_input/<name>"); replaced, never changed in place, like the classifiers' counts.  A deeplab.DeepLabWeights, or an
        # (arch, path) whose arch is one of deeplab.ARCHS, is the reference's other segmenter (DeepLabV3+) under the same keys.
        self.segmenters = {}
        for name, spec in (segmenters or {}).items():
            from . import deeplab, segment
            w = spec
            if not isinstance(spec, (segment.SegmenterWeights, deeplab.DeepLabWeights)):      # (arch, path): the arch's table names its module
                w = (deeplab if isinstance(spec[0], str) and spec[0] in deeplab.ARCHS else segment).load_weights(*spec)
            self.segmenters[name] = w
            for key in self.segmenter_keys(name):
                self.totals[key] = torch.zeros(w.num_classes, w.num_classes, dtype=torch.int64, device=w.device)

        # Detector scoring of the "det" output (RetinaNet mAP at one IoU threshold, exact fp32 HIP kernels; the metric itself is host
        # fp64) is off unless detectors are given: {name: (arch, state-dict path) | detect.DetectorWeights}.  Per name the totals hold
        # a detect.MeanAP for the restored images ("det/<name>") and one for the unrestored inputs ("det_input/<name>");
        # det_nonfinite counts the images of either kind whose detector outputs were not finite (they have no detections).
        self.detectors, self.det_score, self.det_iou, self.det_nonfinite = {}, float(det_score), float(det_iou), [0, 0]
        for name, spec in (detectors or {}).items():
            from . import detect
            self.detectors[name] = spec if isinstance(spec, detect.DetectorWeights) else detect.load_weights(*spec)
            for key in self.detector_keys(name):
                self.totals[key] = detect.MeanAP(self.det_iou)

        # NIQE (no reference, fp64 HIP kernels) is off unless a pristine model is given: a path niqe.load_params reads or a loaded
        # niqe.NiqeParams.  It needs no hq and runs whatever eval_mode says.  totals["niqe"] (the restored images) and
        # totals["niqe_input"] (the unrestored inputs) are fp64 [2] device tensors, the sum of the finite scores and their count -
        # replaced, never changed in place; niqe_seen counts the images handed to update_niqe.
        self.niqe_params, self.niqe_seen = None, 0
        if niqe_params is not None:
            from . import niqe
            self.niqe_params = niqe_params if isinstance(niqe_params, niqe.NiqeParams) else niqe.load_params(niqe_params)
            for key in self.NIQE_KEYS:
                self.totals[key] = torch.zeros(2, dtype=torch.float64, device=self.niqe_params.device)

    NIQE_KEYS = ("niqe", "niqe_input")                  # the `totals` keys of the restored images' and the unrestored inputs' NIQE

    @staticmethod
    def segmenter_keys(name: str):
        """The two `totals` keys of segmenter `name`: the restored images' confusion matrix, the unrestored inputs'."""
        return f"seg/{name}", f"seg_input/{name}"

    @staticmethod
    def detector_keys(name: str):
        """The two `totals` keys of detector `name`: the restored images' MeanAP state, the unrestored inputs'."""
        return f"det/{name}", f"det_input/{name}"

    def _crop(self, t):
        return crop_tensor(t, self.crop)

    @staticmethod
    def classifier_keys(name: str):
        """The two `totals` keys of classifier `name`: the restored images' counts, the unrestored inputs' counts."""
        return f"cls/{name}", f"cls_input/{name}"

    def forward(self, inputs: Sequence[torch.Tensor], task: str, quantize: bool = False) -> List[torch.Tensor]:
        return forward(self.model, inputs, task, quantize=quantize)

    def forward_tasks(self, inputs: Sequence[torch.Tensor], tasks: Sequence[str], quantize: bool = False) -> List[dict]:
        return forward_tasks(self.model, inputs, tasks, quantize=quantize)

    def validation_step(self, batch, eval_types: Sequence[str] = ("lq",), metrics: bool = True, tasks: Sequence[str] = None):
        """tasks (a list that holds "ir"): every input is restored once and decoded for each task (`forward_tasks`); the return
        value is then a list of {task: images}, and PSNR / SSIM still come from the "ir" output."""
        lq, hq, gt, _fname, _task = batch
        if self.classifiers and metrics and (tasks is None or "cls" not in tasks):
            raise ValueError(f"tasks={None if tasks is None else list(tasks)}: the classifiers score the 'cls' output - pass tasks "
                             "with 'cls' in it")
        if self.segmenters and metrics and (tasks is None or "seg" not in tasks):
            raise ValueError(f"tasks={None if tasks is None else list(tasks)}: the segmenters score the 'seg' output - pass tasks "
                             "with 'seg' in it")
        if self.detectors and metrics and (tasks is None or "det" not in tasks):
            raise ValueError(f"tasks={None if tasks is None else list(tasks)}: the detectors score the 'det' output - pass tasks "
                             "with 'det' in it")
        if tasks is not None:
            if "ir" not in tasks:
                raise ValueError(f"tasks={list(tasks)}: PSNR / SSIM are computed on the 'ir' output - add 'ir' to the list")
            outs, _ = validation_step(self.model, lq, hq, need_crop=self.need_crop, eval_types=eval_types, tasks=tasks, crop=self.crop)
            if metrics and hq is not None:
                self.update_metrics(outs[-1]["ir"], hq)
            if metrics and self.classifiers:
                self.update_classification(outs[-1]["cls"], lq, gt)
            if metrics and self.segmenters:
                self.update_segmentation(outs[-1]["seg"], lq, gt)
            if metrics and self.detectors:
                self.update_detection(outs[-1]["det"], lq, gt)
            if metrics:
                self.update_niqe(outs[-1]["ir"], lq)
            return outs
        # the IR evaluator always restores with the "ir" prompt (eval_image_restoration.py:70: self.forward(inputs, 'ir')), whatever
        # task tag the batch carries; task-driven decoding belongs to the downstream (MTL) evaluators, which are out of scope
        preds, hq_c = validation_step(self.model, lq, hq, task="ir", need_crop=self.need_crop, eval_types=eval_types, crop=self.crop)
        if metrics and hq_c is not None and self.eval_mode in ("FR", "ALL") and preds[-1].shape == (self._crop(hq) if self.need_crop else hq).shape:
            tgt = self._crop(hq) if self.need_crop else hq
            n = preds[-1].shape[0]
            if self.metrics_device == "gpu":
                self._add_gpu_metrics(preds[-1], tgt)
            else:
                self.totals["psnr"] += float(psnr_per_image(preds[-1], tgt).sum())          # sum over images (SKPSNR state)
                self.totals["ssim"] += ssim(preds[-1], tgt) * n
            self._add_lpips(preds[-1], tgt)
            self.totals["images"] += n
        if metrics:
            self.update_niqe(preds[-1], lq)
        return preds

    def _add_gpu_metrics(self, preds: torch.Tensor, tgt: torch.Tensor):
        """Per-image PSNR / SSIM sums of the batch into fp64 device totals (0-d tensors): no device-to-host copy per batch."""
        from . import ops
        ps, ss = ops.image_metrics(preds.contiguous(), tgt.contiguous())
        self.totals["psnr"] = self.totals["psnr"] + ps.sum()
        self.totals["ssim"] = self.totals["ssim"] + ss.sum()

    def _add_lpips(self, preds: torch.Tensor, tgt: torch.Tensor):
        """Sum of the batch's per-image LPIPS into the fp64 device total (nothing when LPIPS is off)."""
        if self.lpips_weights is None:
            return
        from . import ops
        dev = self.lpips_weights.device
        self.totals["lpips"] = self.totals["lpips"] + ops.lpips(preds.to(dev).contiguous(), tgt.to(dev).contiguous(), self.lpips_weights).sum()

    # ---- the training step's FORWARD halves (engine_unifie.py:135-191), values only: the HIP path has no autograd ------------
    @torch.no_grad()
    def fr_training_fwd(self, hq, lq):
        """AE encoder (+CFRM on the degraded input): (h0, h0_mids, l0, l0_mids) - engine_unifie.py:135-148."""
        h0, h0_mids = self.model.ae.encode(hq, enable_fr=False, noise=self._noise(hq))        # (ae.encode re-asserts the model's dtype)
        l0, l0_mids = self.model.ae.encode(lq, enable_fr=bool(self.model_kwargs.get("frenc")), noise=self._noise(lq))
        return h0, h0_mids, l0, l0_mids

    @staticmethod
    def fr_loss_fn(h0, h0_mids, l0, l0_mids):
        """Feature-MSE taps of the CFRM stage: 0.1 * L1 + 0.1 * L2 + 0.01 * L3 (+ the latent MSE it logs) - :150-168."""
        mse = lambda a, b: torch.mean((a.float() - b.float()) ** 2)
        layers = [mse(a, b) for a, b in zip(l0_mids, h0_mids)]
        return dict(loss_layer1=layers[0], loss_layer2=layers[1], loss_layer3=layers[2], loss_enc=mse(l0, h0),
                    loss_frenc=0.1 * layers[0] + 0.1 * layers[1] + 0.01 * layers[2])

    @torch.no_grad()
    def cn_training_fwd(self, h0, l0, timesteps=None, noise=None):
        """Controller + SC-Tuner + UNet: diffuse the clean latent, predict z0 under the degraded latent's control - :170-178."""
        zt, _, ts = self.model.diffuse(h0, timesteps, noise)
        return self.model.predict_z0(zt, conditions=l0, timesteps=ts)

    @staticmethod
    def cn_loss_fn(pred_z0, h0):
        return torch.mean((pred_z0.float() - h0.float().to(pred_z0.device)) ** 2)

    @torch.no_grad()
    def te_training_fwd(self, pred_z0, l0_mids, task):
        """AE decoder + TFA on the predicted latent - :186-191."""
        return self.model.ae.decode(pred_z0, l0_mids, task)

    noise_seed = None          # set to an int to make the VAE's posterior sampling reproducible (tests)

    def _noise(self, img):
        if self.noise_seed is None:
            return None
        g = torch.Generator().manual_seed(self.noise_seed + int(img.shape[-1]))
        return torch.randn(img.shape[0], self.model.ae.vae.latent_channels, img.shape[-2] // 8, img.shape[-1] // 8, generator=g)

    def update_metrics(self, preds: torch.Tensor, hq: torch.Tensor):
        """Metric states for one batch of restored images vs their clean targets (for callers that time the forward separately)."""
        tgt = self._crop(hq) if self.need_crop else hq
        if self.eval_mode in ("FR", "ALL") and preds.shape == tgt.shape:
            n = preds.shape[0]
            if self.metrics_device == "gpu":
                self._add_gpu_metrics(preds, tgt)
            else:
                self.totals["psnr"] += float(psnr_per_image(preds, tgt).sum())
                self.totals["ssim"] += ssim(preds, tgt) * n
            self._add_lpips(preds, tgt)
            self.totals["images"] += n

    def update_classification(self, cls_preds: torch.Tensor, inputs: torch.Tensor, labels: torch.Tensor):
        """The accuracy counts of one batch, for every classifier: of `cls_preds`, the quantised "cls" output (the tensor the
        reference's evaluator hands to its classifiers), and of `inputs`, the unrestored lq images it was restored from (centre-
        cropped as the restoration's input is when need_crop is on), so the two accuracies cover the same pixels.  labels: the
        batch's int64 [N] targets.  Nothing when no classifier is configured."""
        if not self.classifiers:
            return
        if labels is None:
            raise ValueError("the classifiers need the batch's labels (gt is None): build the dataset with labels: true on an "
                             "`lq hq label` list")
        from . import ops, rvt, swin, vgg, vit
        if self.need_crop:
            inputs = self._crop(inputs)
        for name, w in self.classifiers.items():
            predict = (ops.vit if isinstance(w, vit.ViTWeights) else ops.swin if isinstance(w, swin.SwinWeights)
                       else ops.rvt if isinstance(w, rvt.RVTWeights) else ops.vgg if isinstance(w, vgg.VGGWeights)
                       else ops.classify)                 # each takes its own weights class
            for key, images in zip(self.classifier_keys(name), (cls_preds, inputs)):
                logits = predict(images.to(device=w.device, dtype=torch.float32).contiguous(), w)
                _pred, tp, targets, predicted = ops.top1(logits, labels)
                self.totals[key] = self.totals[key] + torch.stack([tp, targets, predicted])

    def update_segmentation(self, seg_preds: torch.Tensor, inputs: torch.Tensor, label_maps: torch.Tensor):
        """The confusion matrices of one batch, for every segmenter: of `seg_preds`, the quantised "seg" output (the tensor the
        reference's evaluator hands to its segmenters), and of `inputs`, the unrestored lq images it was restored from.  Inputs and
        label maps are centre-cropped with the restoration's own box when need_crop is on, so both sides are scored on the same
        pixels.  label_maps: the batch's [N,H,W] integer trainId maps (255 = ignore).  Nothing when no segmenter is configured."""
        if not self.segmenters:
            return
        if label_maps is None or not torch.is_tensor(label_maps) or label_maps.ndim != 3:
            raise ValueError("the segmenters need the batch's label maps (gt is None or no [N,H,W] tensor): build the dataset with "
                             "labels: map on an `lq hq label.png` list")
        from . import ops, segment
        if self.need_crop:
            inputs, label_maps = self._crop(inputs), self._crop(label_maps)
        if tuple(label_maps.shape) != (seg_preds.shape[0], *seg_preds.shape[2:]):
            raise ValueError(f"the label maps are {tuple(label_maps.shape)}, the seg output {tuple(seg_preds.shape)}")
        for name, w in self.segmenters.items():
            # the targets are checked once per batch; ops.segment's / ops.deeplab's own predictions always lie in [0, classes)
            target = ops.checked_targets(label_maps.to(device=w.device, dtype=torch.int64).contiguous(), w.num_classes)
            predict = getattr(ops, w.name)                           # ops.segment or ops.deeplab: each takes its own weights class
            for key, images in zip(self.segmenter_keys(name), (seg_preds, inputs)):
                pred = predict(images.to(device=w.device, dtype=torch.float32).contiguous(), w)
                self.totals[key] = self.totals[key] + segment.confusion(pred, target, w.num_classes)

    def update_detection(self, det_preds: torch.Tensor, inputs: torch.Tensor, targets) -> dict:
        """The mAP states of one batch, for every detector: of `det_preds`, the quantised "det" output (the tensor the reference's
        evaluator hands to its detector), and of `inputs`, the unrestored lq images it was restored from.  targets: the batch's list
        of {boxes [n,4], labels [n]} in the uncropped images' coordinates; with need_crop the inputs are centre-cropped with the
        restoration's own box and the boxes shifted by its offset, clipped to it and dropped when nothing is left.  The metric
        update is host fp64 (untimed, like NIQE's algebra).  Returns {totals key: this batch's own detect.MeanAP} - what a caller
        that splits the totals by batch merges elsewhere; {} when no detector is configured."""
        if not self.detectors:
            return {}
        if not isinstance(targets, (list, tuple)) or len(targets) != det_preds.shape[0] or not all(isinstance(t, dict) for t in targets):
            raise ValueError("the detectors need the batch's boxes (gt is no list of {boxes, labels}, one per image): build the dataset "
                             "with labels: boxes on an `lq hq annotation.json` list")
        from . import data, detect
        if self.need_crop:
            t, b, l, r = crop_box(inputs.shape[-2], inputs.shape[-1], self.crop[0], self.crop[1])
            inputs, targets = self._crop(inputs), data.crop_boxes(targets, t, l, b - t, r - l)
        if tuple(inputs.shape[2:]) != tuple(det_preds.shape[2:]):
            raise ValueError(f"the inputs are {tuple(inputs.shape)}, the det output {tuple(det_preds.shape)}")
        batch = {}
        for name, w in self.detectors.items():
            for j, (key, images) in enumerate(zip(self.detector_keys(name), (det_preds, inputs))):
                dets, bad = detect.forward(images.to(device=w.device, dtype=torch.float32).contiguous(), w, score_thresh=self.det_score)
                self.det_nonfinite[j] += int(bad.sum())
                batch[key] = detect.MeanAP(self.det_iou)
                batch[key].update(dets, targets)
                self.totals[key].merge(batch[key])
        return batch

    def update_niqe(self, preds: torch.Tensor, lq: torch.Tensor):
        """The NIQE states of one batch: of `preds`, the quantised "ir" output, and of `lq`, the unrestored inputs it was restored
        from (centre-cropped as the restoration's input is when need_crop is on), so the two scores cover the same pixels.  An
        image whose score is not finite (fewer than two NaN-free blocks: a black image) is left out of the sum and the count and
        shows up in metrics()["niqe_skipped"].  Needs no hq.  Nothing when no pristine model is configured."""
        if self.niqe_params is None:
            return
        from . import ops
        if self.need_crop:
            lq = self._crop(lq)
        dev = self.niqe_params.device
        for key, images in zip(self.NIQE_KEYS, (preds, lq)):
            s = ops.niqe(images.to(device=dev, dtype=torch.float32).contiguous(), self.niqe_params)
            ok = torch.isfinite(s)
            self.totals[key] = self.totals[key] + torch.stack([torch.where(ok, s, torch.zeros_like(s)).sum(), ok.sum().double()])
        self.niqe_seen += preds.shape[0]

    def metrics(self) -> dict:
        n = max(self.totals["images"], 1)
        psnr_sum, ssim_sum = float(self.totals["psnr"]), float(self.totals["ssim"])     # (the one device read of the "gpu" totals)
        res = {"val_lq/psnr": psnr_sum / n, "val_lq/ssim": ssim_sum / n, "images": self.totals["images"]}
        if self.lpips_weights is not None:
            res["val_lq/lpips"] = float(self.totals["lpips"]) / n
        for name in self.classifiers:                     # macro = the reference's MulticlassAccuracy(top_k=1); _top1 = micro
            from .classify import accuracy
            for prefix, key in zip(("val_lq", "val_input"), self.classifier_keys(name)):
                res[f"{prefix}/{name}"], res[f"{prefix}/{name}_top1"] = accuracy(*self.totals[key])
        for name in self.segmenters:                      # mIoU = the reference's MulticlassJaccardIndex(19, ignore_index=255)
            from .segment import miou
            for prefix, key in zip(("val_lq", "val_input"), self.segmenter_keys(name)):
                res[f"{prefix}/{name}"], res[f"{prefix}/{name}_acc"] = miou(self.totals[key])[:2]
        for name in self.detectors:                       # mAP = the reference's MeanAveragePrecision(iou_thresholds=[det_iou])
            for prefix, key in zip(("val_lq", "val_input"), self.detector_keys(name)):
                res[f"{prefix}/{name}"] = self.totals[key].compute()["map"]
        if self.detectors:
            res["det_nonfinite"] = list(self.det_nonfinite)
        if self.niqe_params is not None:                  # the mean over the images with a finite score; the others are counted
            res["niqe_skipped"] = []
            for prefix, key in zip(("val_lq", "val_input"), self.NIQE_KEYS):
                total, count = self.totals[key].tolist()
                res[f"{prefix}/niqe"] = total / count if count else float("nan")
                res["niqe_skipped"].append(self.niqe_seen - int(count))
        return res
