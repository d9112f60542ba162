"""Config entry point: `python -m unirestore_amd.cli validate --config configs/<file>.yaml [--set a.b.c=value ...]`, and
`python -m unirestore_amd.cli restore --config CFG --input DIR_OR_LISTFILE --output DIR` for image files.  Three commands take no
config and write degraded copies of clean images, `python -m unirestore_amd.cli COMMAND --input DIR_OR_LISTFILE --output DIR` with
`corrupt --corruptions NAMES_OR_SUBSET` (unirestore_amd.corrupt), `distort --corruptions glass_blur,snow|all` (glass blur, snow and
elastic transform: unirestore_amd.distort) or `jpeg --quality 10,25,s3` (what the images' JPEGs of those qualities decode to):
one argument check (`_check_file_args`), one writer (`_write_degraded`) and one dispatch in `main` serve all three.

Resolves a LightningCLI-style YAML (the key schema of the reference's configs/*.yaml: `seed_everything`, `trainer.{accelerator,
devices,precision}`, `model.class_path` + `init_args.model_kwargs.{frenc,cnet,tedit}`, `data.class_path` + `init_args`;
reference src/main.py:17-28, configs/val.yaml:47-67, src/core/engine_unifie.py:29-42) into the MI355X path: model
(`checkpoint.build_from_config`), caller (`runner.LitUniFIE`), synthetic data (`data.SyntheticImages`), and runs the
validation loop.  One process per GPU: under `torch.distributed.run` the global batch is sharded over the ranks, the
weights are broadcast from rank 0 and the restored shards all-gathered over RCCL.  There is no CPU path: `accelerator: cpu`
is an error, not a fallback.  Prints one JSON line on rank 0.  `validate --lpips` adds LPIPS, `validate --tasks ir,cls --classify
NAME=ARCH:WEIGHTS.pth` the top-1 accuracy of a user-supplied ResNet on the `cls` output (unirestore_amd.classify), `--vit
NAME=ARCH:WEIGHTS.pth` that of a user-supplied VisionTransformer (unirestore_amd.vit), `--swin NAME=ARCH:WEIGHTS.pth` that of a
user-supplied Swin-V2 (unirestore_amd.swin), `--rvt NAME=ARCH:WEIGHTS.pth` that of a user-supplied Robust Vision Transformer
(unirestore_amd.rvt), `--vgg NAME=ARCH:WEIGHTS.pth` that of a user-supplied torchvision VGG (unirestore_amd.vgg), `validate --tasks
ir,seg --segment NAME=ARCH:WEIGHTS.pth` the mIoU of a user-supplied RefineNet-LW on the `seg` output (unirestore_amd.segment) and
`--deeplab NAME=ARCH:WEIGHTS.pth` that of a user-supplied DeepLabV3+ (unirestore_amd.deeplab), `validate --tasks ir,det --detect
NAME=ARCH:WEIGHTS.pth` the mAP of a user-supplied torchvision RetinaNet on the `det` output (unirestore_amd.detect), `validate --niqe PARAMS` the no-reference NIQE score of the restored images and of the
inputs against a user-supplied pristine model (unirestore_amd.niqe); all opt-in.
"""
import argparse
import json
import os
import sys
import time

import yaml

# class paths the reference's files name -> the Lightning-free callers of this package
MODEL_CLASSES = {
    "core.engine_unifie.LitUniFIEIR": "unirestore_amd.runner.LitUniFIE",
    "core.engine_unifie.LitUniFIEMTL": "unirestore_amd.runner.LitUniFIE",
    "core.engine_unifie.LitUniFIE": "unirestore_amd.runner.LitUniFIE",
    "unirestore_amd.runner.LitUniFIE": "unirestore_amd.runner.LitUniFIE",
}
DATA_CLASSES = {"unirestore_amd.data.SyntheticImages": "unirestore_amd.data.SyntheticImages",
                "unirestore_amd.data.ImageListFiles": "unirestore_amd.data.ImageListFiles",
                "unirestore_amd.data.CorruptedImageFiles": "unirestore_amd.data.CorruptedImageFiles",
                "unirestore_amd.data.JpegImageFiles": "unirestore_amd.data.JpegImageFiles",
                "unirestore_amd.data.DistortedImageFiles": "unirestore_amd.data.DistortedImageFiles",
                "data.DatasetEngine": "unirestore_amd.data.SyntheticImages"}      # datasets are out of scope: synthetic stand-in
PRECISIONS = {"bf16-mixed": "bf16", "bf16": "bf16", "bf16-true": "bf16", "16-mixed": "fp16", "16": "fp16", "16-true": "fp16",
              "fp16": "fp16"}
# precision: 32 (the reference's shipped val.yaml default) has no fp32 matrix path here.  It is REFUSED unless the caller opts into
# the closest 16-bit type (fp16 storage / MFMA operands, fp32 accumulation, statistics, softmax and DDIM state: outputs within
# 1e-3 rel-L2 of the fp32 reference) with --allow-16bit / allow_16bit=True - never silently.
PRECISIONS_32 = ("32", "32-true")


def load_config(path: str, overrides=()) -> dict:
    with open(path) as f:
        cfg = yaml.safe_load(f)
    for ov in overrides:
        key, _, val = ov.partition("=")
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = yaml.safe_load(val)
    return cfg


COLOR_FIX_CHOICES = ("none", "wavelet", "adain")


def apply_color_fix(cfg: dict, flag) -> dict:
    """--color-fix {none,wavelet,adain} overrides the config's `cnet.color_fix` ("none" turns a configured fix off); flag None
    leaves the config as it is.  Returns cfg."""
    if flag is None:
        return cfg
    if flag not in COLOR_FIX_CHOICES:
        raise ValueError(f"--color-fix {flag!r}: choose from {list(COLOR_FIX_CHOICES)}")
    mk = cfg["model"].setdefault("init_args", {}).setdefault("model_kwargs", {})
    if not mk.get("cnet"):
        raise ValueError("--color-fix: the config has no model_kwargs.cnet section to carry cnet.color_fix")
    mk["cnet"]["color_fix"] = None if flag == "none" else flag
    return cfg


def resolve(cfg: dict, allow_16bit: bool = False) -> dict:
    """Validate a config and reduce it to what the runner needs (raises ValueError / KeyError on unknown pieces)."""
    tr, mo, da = cfg.get("trainer", {}), cfg["model"], cfg.get("data", {})
    if str(tr.get("accelerator", "gpu")) not in ("gpu", "cuda", "auto"):
        raise ValueError(f"trainer.accelerator={tr.get('accelerator')!r}: the MI355X path has no CPU fallback (use accelerator: gpu)")
    prec = str(tr.get("precision", "bf16-mixed"))
    if prec in PRECISIONS_32:
        allow_16bit = allow_16bit or os.environ.get("UR_ALLOW_16BIT", "0") == "1"      # opt-in without editing the command line
        if not allow_16bit:
            raise ValueError(f"trainer.precision={prec!r}: this path computes with 16-bit MFMA operands (fp32 accumulation); pass "
                             "--allow-16bit (allow_16bit=True, or UR_ALLOW_16BIT=1 in the environment) to run the config in fp16, or set precision to bf16-mixed / 16-mixed")
        import warnings
        warnings.warn(f"trainer.precision={prec!r} runs as fp16 storage + fp32 accumulation (no fp32 matrix path on this backend)")
        dtype = "fp16"
    elif prec in PRECISIONS:
        dtype = PRECISIONS[prec]
    else:
        raise ValueError(f"trainer.precision={prec!r} not supported: choose from {sorted(PRECISIONS) + list(PRECISIONS_32)}")
    if mo["class_path"] not in MODEL_CLASSES:
        raise KeyError(f"model.class_path {mo['class_path']!r} is not a caller of the restoration path: {sorted(MODEL_CLASSES)}")
    init = dict(mo.get("init_args", {}))
    mk = init.pop("model_kwargs")
    for k in ("frenc", "cnet", "tedit"):
        if mk.get(k) and str(mk[k].get("ckpt_path", "")).startswith("$"):      # "$path_to_stage1_ckpt$" placeholders of val.yaml
            mk[k] = dict(mk[k], ckpt_path=None)
    cn = mk.get("cnet") or {}
    if cn.get("tile_size") is not None or cn.get("tile_stride") is not None:     # tiled latent sampling (opt-in)
        from .tiling import check_tile_stride, default_tile_stride
        if cn.get("tile_size") is None:
            raise ValueError("cnet.tile_stride needs cnet.tile_size (the latent tile edge, e.g. 64)")
        tile = int(cn["tile_size"])
        stride = int(cn["tile_stride"]) if cn.get("tile_stride") is not None else default_tile_stride(tile)
        check_tile_stride(tile, stride)
        mk["cnet"] = dict(cn, tile_size=tile, tile_stride=stride)
    if cn.get("color_fix") is not None and cn["color_fix"] not in ("wavelet", "adain"):      # colour fix of the outputs (opt-in)
        raise ValueError(f"cnet.color_fix={cn['color_fix']!r}: choose wavelet, adain or null")
    dcp = da.get("class_path", "unirestore_amd.data.SyntheticImages")
    if dcp not in DATA_CLASSES:
        raise KeyError(f"data.class_path {dcp!r} unknown: {sorted(DATA_CLASSES)}")
    dargs = dict(da.get("init_args", {}))
    if dcp == "data.DatasetEngine":                       # the reference's key layout -> the synthetic stand-in's arguments
        val, train = dargs.get("val", {}), dargs.get("train", {})
        res = train.get("resolution", 512)
        dargs = dict(task={"mtl": "ir"}.get(dargs.get("task", "ir"), dargs.get("task", "ir")), resolution=[res, res],
                     batch_size=val.get("batch_size", 1), num_batches=4)
    devices = tr.get("devices", 1)
    n_dev = len(devices) if isinstance(devices, (list, tuple)) else (int(devices) if str(devices).isdigit() else 1)
    return dict(seed=cfg.get("seed_everything", 42), dtype=dtype, devices=n_dev, model_kwargs=mk,
                caller_args={k: init[k] for k in ("save_image", "eval_mode", "need_crop") if k in init}, data_args=dargs,
                data_class=DATA_CLASSES[dcp])


def _ranks():
    """(rank, world size, local rank) of this process under torch.distributed.run; (0, 1, 0) without it."""
    return int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))


def _start(r: dict, hf_root, random_init, model, **caller_args):
    """What `validate` and `restore` do before their loops: this rank's device, the process group, the caller with the config's
    model (or `model`), seeded random weights on rank 0 when no checkpoint is reachable, the weights broadcast, `refresh`.
    r = resolve(cfg) -> (rank, world, device, torch.distributed or None, the LitUniFIE)."""
    import torch
    rank, world, local = _ranks()
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the restoration path runs on MI355X only (no CPU fallback)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    torch.manual_seed(r["seed"])
    from . import runner
    from .dist import broadcast_weights_sharded
    lit = runner.LitUniFIE(r["model_kwargs"], dtype=r["dtype"], hf_root=hf_root, model=model, **caller_args)
    no_ckpt = not any((r["model_kwargs"].get(k) or {}).get("ckpt_path") for k in ("frenc", "cnet", "tedit")) and not hf_root
    if model is not None:
        model.set_dtype(r["dtype"])
        model.set_color_fix((r["model_kwargs"].get("cnet") or {}).get("color_fix"))
    elif no_ckpt and random_init and rank == 0:             # no checkpoint reachable: seeded random weights of the architecture
        from .init import init_random_
        init_random_(lit.model, r["seed"], "cpu")
    if world > 1:
        broadcast_weights_sharded(lit.model.to(dev), src=0)
    lit.model.refresh()
    return rank, world, dev, dist, lit


def check_lpips_arg(lpips):
    """--lpips ALEXNET.pth,LIN.pth (or a pair of paths) -> (alexnet_path, lin_path); ValueError unless both files exist."""
    parts = [p for p in lpips.split(",")] if isinstance(lpips, str) else list(lpips)
    if len(parts) != 2 or not all(parts):
        raise ValueError("--lpips takes two files: ALEXNET.pth,LIN.pth (torchvision's AlexNet state dict, the LPIPS v0.1 linear layers)")
    for p in parts:
        if not os.path.isfile(p):
            raise ValueError(f"--lpips: no such file: {p}")
    return parts[0], parts[1]


def check_niqe_arg(niqe):
    """--niqe PARAMS (or a loaded niqe.NiqeParams, returned as it is) -> the path; ValueError unless the file exists and its
    extension is one niqe.load_params reads (.pt / .pth / .npz / .mat with the keys mu_prisparam and cov_prisparam)."""
    from .niqe import EXTENSIONS, NiqeParams
    if isinstance(niqe, NiqeParams):
        return niqe
    if not isinstance(niqe, (str, os.PathLike)) or not str(niqe):
        raise ValueError(f"--niqe takes one file of NIQE model parameters ({', '.join(EXTENSIONS)}); got {type(niqe).__name__}")
    path = str(niqe)
    if not os.path.isfile(path):
        raise ValueError(f"--niqe: no such file: {path}")
    if os.path.splitext(path)[1].lower() not in EXTENSIONS:
        raise ValueError(f"--niqe: {path}: unknown extension, expected one of {', '.join(EXTENSIONS)}")
    return path


def check_niqe_run(crop, r: dict):
    """What a NIQE run needs besides its parameters, checked before the model is built: an evaluator crop (the given one or the
    default, when the config's need_crop is on) that holds at least two 96 x 96 blocks.  r = resolve(cfg)."""
    from .niqe import BLOCK, MIN_BLOCKS
    from .runner import DEFAULT_CROP
    if not r["caller_args"].get("need_crop", True):
        return
    ch, cw = DEFAULT_CROP if crop is None else crop
    if (ch // BLOCK) * (cw // BLOCK) < MIN_BLOCKS:
        raise ValueError(f"--niqe: the evaluator's crop {ch} x {cw} holds {(ch // BLOCK) * (cw // BLOCK)} block(s) of {BLOCK} x {BLOCK}; "
                         f"the score needs at least {MIN_BLOCKS} (pass a larger --crop)")


LABELLED_DATA = ("ImageListFiles", "CorruptedImageFiles", "DistortedImageFiles", "JpegImageFiles")      # take `labels: true`


def _check_scorer_arg(flag, value, archs, what):
    """`flag` NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | loaded weights) -> {name: (arch, path) |
    weights}.  ValueError for a malformed item, an arch outside `archs`, a missing file or a name given twice.  what: the kind of
    file, for the usage text."""
    form = f"{flag} takes NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:WEIGHTS.pth]: a result name, one of {sorted(archs)}, {what}"
    if isinstance(value, str):
        items = []
        for part in value.split(","):
            name, eq, spec = part.partition("=")
            arch, colon, path = spec.partition(":")
            if not (name and eq and arch and colon and path):
                raise ValueError(f"{form}; got {part!r}")
            items.append((name, (arch, path)))
    elif isinstance(value, dict):
        items = list(value.items())
    else:
        raise ValueError(f"{form}; got {type(value).__name__}")
    if not items:
        raise ValueError(form)
    out = {}
    for name, spec in items:
        if name in out:
            raise ValueError(f"{flag}: the name {name!r} is given twice")
        if isinstance(spec, (tuple, list)):
            if len(spec) != 2:
                raise ValueError(f"{form}; got {name!r}: {spec!r}")
            arch, path = spec
            if not isinstance(arch, str) or arch not in archs:
                raise ValueError(f"{flag} {name}: unknown arch {arch!r}, choose from {sorted(archs)}")
            if not os.path.isfile(path):
                raise ValueError(f"{flag} {name}: no such file: {path}")
            spec = (arch, path)
        out[name] = spec
    return out


def check_classify_arg(classify):
    """--classify NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | a loaded classify.ClassifierWeights)
    -> {name: (arch, path) | ClassifierWeights}.  ValueError for a malformed item, an unknown arch, a missing file or a name given
    twice.  ARCH is one of classify.ARCHS (torchvision's resnet18 / resnet50 / resnet101); the weights are the user's."""
    from .classify import ARCHS
    return _check_scorer_arg("--classify", classify, ARCHS, "a torchvision state dict")


def check_classify_run(classify, tasks, r: dict, flag="--classify"):
    """What a classifier run needs besides its weights, checked before the model is built: `cls` among the tasks (it is not added
    silently, and `ir` stays required for PSNR) and a dataset that yields labels.  r = resolve(cfg).  flag: the option the errors
    name (--vit has the same needs)."""
    if tasks is None or "cls" not in tasks:
        raise ValueError(f"{flag} scores the 'cls' output: pass --tasks with 'cls' in it, e.g. ir,cls (got "
                         f"{'none' if tasks is None else ','.join(tasks)}; it is not added silently)")
    cls_name = r["data_class"].rsplit(".", 1)[1]
    if cls_name not in LABELLED_DATA or not r["data_args"].get("labels") or r["data_args"].get("labels") == "map":
        raise ValueError(f"{flag} needs labels, and data.{cls_name} yields none as configured: use an `lq hq label` list with one of "
                         f"{list(LABELLED_DATA)} and set `labels: true` in data.init_args")


def check_vit_arg(vit, classify=None):
    """--vit NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | a loaded vit.ViTWeights) -> {name: (arch,
    path) | ViTWeights}.  ValueError for a malformed item, an unknown arch, a missing file, a name given twice or a name that
    `classify` (the checked --classify argument) already uses: both write val_lq/NAME.  ARCH is one of vit.ARCHS (torchvision's
    vit_b_16 / vit_b_32 / vit_l_16 / vit_l_32); the weights are the user's."""
    from .vit import ARCHS
    out = _check_scorer_arg("--vit", vit, ARCHS, "a torchvision VisionTransformer state dict")
    both = sorted(set(out) & set(classify or {}))
    if both:
        raise ValueError(f"--vit: the name {both[0]!r} is used by --classify too; every classifier needs a name of its own")
    return out


def check_swin_arg(swin, classify=None, vit=None):
    """--swin NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | a loaded swin.SwinWeights) -> {name: (arch,
    path) | SwinWeights}.  ValueError for a malformed item, an unknown arch, a missing file, a name given twice or a name that
    `classify` or `vit` (the checked --classify and --vit arguments) already uses: all write val_lq/NAME.  ARCH is one of swin.ARCHS
    (torchvision's swin_v2_t / swin_v2_s / swin_v2_b); the weights are the user's."""
    from .swin import ARCHS
    out = _check_scorer_arg("--swin", swin, ARCHS, "a torchvision SwinTransformer V2 state dict")
    for flag, other in (("--classify", classify), ("--vit", vit)):
        both = sorted(set(out) & set(other or {}))
        if both:
            raise ValueError(f"--swin: the name {both[0]!r} is used by {flag} too; every classifier needs a name of its own")
    return out


def check_rvt_arg(rvt, classify=None, vit=None, swin=None):
    """--rvt NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | a loaded rvt.RVTWeights) -> {name: (arch,
    path) | RVTWeights}.  ValueError for a malformed item, an unknown arch, a missing file, a name given twice or a name that
    `classify`, `vit` or `swin` (the checked --classify, --vit and --swin arguments) already uses: all write val_lq/NAME.  ARCH is
    one of rvt.ARCHS (the reference's rvt_tiny / rvt_small / rvt_base and their _plus variants); the weights are the user's."""
    from .rvt import ARCHS
    out = _check_scorer_arg("--rvt", rvt, ARCHS, "an RVT checkpoint")
    for flag, other in (("--classify", classify), ("--vit", vit), ("--swin", swin)):
        both = sorted(set(out) & set(other or {}))
        if both:
            raise ValueError(f"--rvt: the name {both[0]!r} is used by {flag} too; every classifier needs a name of its own")
    return out


def check_vgg_arg(vgg, classify=None, vit=None, swin=None, rvt=None):
    """--vgg NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | a loaded vgg.VGGWeights) -> {name: (arch,
    path) | VGGWeights}.  ValueError for a malformed item, an unknown arch, a missing file, a name given twice or a name that
    `classify`, `vit`, `swin` or `rvt` (the checked arguments of those options) already uses: all write val_lq/NAME.  ARCH is one of
    vgg.ARCHS (torchvision's vgg11 / vgg13 / vgg16 / vgg19 and their _bn variants); the weights are the user's."""
    from .vgg import ARCHS
    out = _check_scorer_arg("--vgg", vgg, ARCHS, "a torchvision VGG state dict")
    for flag, other in (("--classify", classify), ("--vit", vit), ("--swin", swin), ("--rvt", rvt)):
        both = sorted(set(out) & set(other or {}))
        if both:
            raise ValueError(f"--vgg: the name {both[0]!r} is used by {flag} too; every classifier needs a name of its own")
    return out


def check_classifiers_arg(classify, vit, swin=None, rvt=None, vgg=None):
    """The checked --classify, --vit, --swin, --rvt and --vgg arguments (each may be None) as the one dict of classifiers the
    evaluator takes - it tells the networks apart - and the option that errors about the run name: (None, None) when none is given."""
    if classify is None and vit is None and swin is None and rvt is None and vgg is None:
        return None, None
    flag = ("--classify" if classify is not None else "--vit" if vit is not None else "--swin" if swin is not None
            else "--rvt" if rvt is not None else "--vgg")
    classify = {} if classify is None else check_classify_arg(classify)
    vit = {} if vit is None else check_vit_arg(vit, classify)
    swin = {} if swin is None else check_swin_arg(swin, classify, vit)
    rvt = {} if rvt is None else check_rvt_arg(rvt, classify, vit, swin)
    vgg = {} if vgg is None else check_vgg_arg(vgg, classify, vit, swin, rvt)
    return {**classify, **vit, **swin, **rvt, **vgg}, flag


def check_segment_arg(segment):
    """--segment NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | a loaded segment.SegmenterWeights)
    -> {name: (arch, path) | SegmenterWeights}.  ValueError for a malformed item, an unknown arch, a missing file or a name given
    twice.  ARCH is one of segment.ARCHS (RefineNet-LW on ResNet-50 / 101 / 152); the weights are the user's."""
    from .segment import ARCHS
    return _check_scorer_arg("--segment", segment, ARCHS, "a RefineNet-LW state dict")


def check_segment_run(segment, tasks, r: dict, flag="--segment"):
    """What a segmenter run needs besides its weights, checked before the model is built: `seg` among the tasks (it is not added
    silently, and `ir` stays required for PSNR) and a dataset that yields label maps.  r = resolve(cfg).  flag: the option the
    errors name (--deeplab has the same needs)."""
    if tasks is None or "seg" not in tasks:
        raise ValueError(f"{flag} scores the 'seg' output: pass --tasks with 'seg' in it, e.g. ir,seg (got "
                         f"{'none' if tasks is None else ','.join(tasks)}; it is not added silently)")
    cls_name = r["data_class"].rsplit(".", 1)[1]
    if cls_name not in LABELLED_DATA or r["data_args"].get("labels") != "map":
        raise ValueError(f"{flag} needs label maps, and data.{cls_name} yields none as configured: use an `lq hq label.png` list with "
                         f"one of {list(LABELLED_DATA)} and set `labels: map` in data.init_args")


def check_deeplab_arg(deeplab, segment=None):
    """--deeplab NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | a loaded deeplab.DeepLabWeights)
    -> {name: (arch, path) | DeepLabWeights}.  ValueError for a malformed item, an unknown arch, a missing file, a name given
    twice or a name that `segment` (the checked --segment argument) already uses: both write val_lq/NAME.  ARCH is one of
    deeplab.ARCHS (DeepLabV3+ on ResNet-50 / 101, output stride 16); the weights are the user's."""
    from .deeplab import ARCHS
    out = _check_scorer_arg("--deeplab", deeplab, ARCHS, "a DeepLabV3+ checkpoint")
    both = sorted(set(out) & set(segment or {}))
    if both:
        raise ValueError(f"--deeplab: the name {both[0]!r} is used by --segment too; every segmenter needs a name of its own")
    return out


def check_segmenters_arg(segment, deeplab):
    """The checked --segment and --deeplab arguments (either may be None) as the one dict of segmenters the evaluator takes - it
    tells the two networks apart - and the option that errors about the run name: (None, None) when neither is given."""
    if segment is None and deeplab is None:
        return None, None
    flag = "--deeplab" if segment is None else "--segment"
    segment = {} if segment is None else check_segment_arg(segment)
    deeplab = {} if deeplab is None else check_deeplab_arg(deeplab, segment)
    return {**segment, **deeplab}, flag


def check_detect_arg(detect, det_score=0.05, det_iou=0.5):
    """--detect NAME=ARCH:WEIGHTS.pth[,NAME=ARCH:OTHER.pth] (or a dict NAME -> (ARCH, path) | a loaded detect.DetectorWeights) ->
    {name: (arch, path) | DetectorWeights}.  ValueError for a malformed item, an unknown arch, a missing file or a name given twice,
    a --det-score outside [0, 1) or a --det-iou outside (0, 1].  ARCH is one of detect.ARCHS (torchvision's
    retinanet_resnet50_fpn_v2); the weights are the user's."""
    from .detect import ARCHS
    out = _check_scorer_arg("--detect", detect, ARCHS, "a torchvision RetinaNet state dict")
    if not (isinstance(det_score, (int, float)) and 0.0 <= float(det_score) < 1.0):
        raise ValueError(f"--det-score {det_score!r}: the score threshold must be in [0, 1)")
    if not (isinstance(det_iou, (int, float)) and 0.0 < float(det_iou) <= 1.0):
        raise ValueError(f"--det-iou {det_iou!r}: the IoU threshold must be in (0, 1]")
    return out


def check_detect_run(detect, tasks, r: dict, flag="--detect"):
    """What a detector run needs besides its weights, checked before the model is built: `det` among the tasks (it is not added
    silently, and `ir` stays required for PSNR), a config whose task editor knows `det`, and a dataset that yields boxes.
    r = resolve(cfg)."""
    if tasks is None or "det" not in tasks:
        raise ValueError(f"{flag} scores the 'det' output: pass --tasks with 'det' in it, e.g. ir,det (got "
                         f"{'none' if tasks is None else ','.join(tasks)}; it is not added silently)")
    known = list((r["model_kwargs"].get("tedit") or {}).get("task") or [])
    if "det" not in known:
        raise ValueError(f"{flag} needs the 'det' output, and the config's task editor knows {known}: add det to model tedit.task")
    cls_name = r["data_class"].rsplit(".", 1)[1]
    if cls_name not in LABELLED_DATA or r["data_args"].get("labels") != "boxes":
        raise ValueError(f"{flag} needs boxes, and data.{cls_name} yields none as configured: use an `lq hq annotation.json` list with "
                         f"one of {list(LABELLED_DATA)} and set `labels: boxes` in data.init_args")


def merge_detection_states(everyone, det_iou):
    """The detector states of every rank as one: everyone[q] = (rank q's {totals key: detect.MeanAP}, its [restored, input] counts
    of non-finite images, its {"fog/3": {totals key: MeanAP}}), merged in rank order into fresh states -> (totals, det_nonfinite,
    by_corruption).  The per-class lists are concatenated, so the result is what one rank would hold had it seen every batch."""
    from .detect import MeanAP
    totals, bad, by = {}, [0, 0], {}
    for totals_q, bad_q, by_q in everyone:
        for k, ap in totals_q.items():
            totals.setdefault(k, MeanAP(det_iou)).merge(ap)
        bad = [a + b for a, b in zip(bad, bad_q)]
        for c, aps in by_q.items():
            for k, ap in aps.items():
                by.setdefault(c, {}).setdefault(k, MeanAP(det_iou)).merge(ap)
    return totals, bad, by


def check_crop_arg(crop):
    """--crop H,W (or a pair of integers) -> (H, W): the evaluator's centre crop, 512,512 unless given (the reference's seg and
    multi-task evaluators use 960,1664)."""
    if isinstance(crop, str):
        try:
            crop = tuple(int(v) for v in crop.split(","))
        except ValueError:
            raise ValueError(f"--crop takes H,W, two integers >= 1; got {crop!r}") from None
    from .runner import check_crop
    return check_crop(crop)


def validate(cfg: dict, hf_root=None, max_batches=None, random_init=True, allow_16bit=False, metrics_device="cpu", tasks=None,
             model=None, lpips=None, classify=None, segment=None, crop=None, niqe=None, deeplab=None, vit=None, swin=None, rvt=None,
             vgg=None, detect=None, det_score=0.05, det_iou=0.5) -> dict:
    """tasks: a list of task names - every batch is restored once and decoded for each of them (DiffUIE.forward_tasks).  PSNR / SSIM
    come from the "ir" output, so the list must hold "ir"; images_per_s counts input images.  model: a ready DiffUIE to use instead
    of building the config's.  With data.CorruptedImageFiles (and data.DistortedImageFiles: "snow/3") the result also holds by_corruption ("fog/3" -> psnr, ssim, images)
    and skipped (the subset members that are not built); with data.JpegImageFiles it holds by_corruption ("jpeg/10", the quality);
    with either, resize = [lo, hi] when the data's resize-down / resize-back wrapper is on.
    lpips: "ALEXNET.pth,LIN.pth", a pair of paths or a loaded lpips.LpipsWeights - the result gains val_lq/lpips and every
    by_corruption entry lpips (AlexNet LPIPS in fp32 on the GPU; the weights are the user's, none ship with the project).
    classify: "NAME=ARCH:WEIGHTS.pth,..." or {NAME: (ARCH, path) | classify.ClassifierWeights} - ResNet top-1 accuracy of the "cls"
    output against the data's labels (tasks must hold "cls", the data must be built with labels: true): the result and every
    by_corruption entry gain, per NAME, the macro accuracy (the reference's MulticlassAccuracy) and NAME_top1 (micro) of the
    restored images (val_lq/NAME; by_corruption: NAME) and of the unrestored inputs (val_input/NAME; by_corruption: input/NAME).
    vit: the same form with vit.ARCHS and vit.ViTWeights - a VisionTransformer scored under the same keys (a name may be used by only
    one of the two).  swin: the same form with swin.ARCHS and swin.SwinWeights - a Swin-V2, likewise (a name may be used by only
    one of the three).  rvt: the same form with rvt.ARCHS and rvt.RVTWeights - a Robust Vision Transformer, likewise (a name may be
    used by only one of the four).  vgg: the same form with vgg.ARCHS and vgg.VGGWeights - a torchvision VGG, likewise (a name may be
    used by only one of the five).
    segment: "NAME=ARCH:WEIGHTS.pth,..." or {NAME: (ARCH, path) | segment.SegmenterWeights} - RefineNet-LW mIoU of the "seg" output
    against the data's label maps (tasks must hold "seg", the data must be built with labels: map): the result and every
    by_corruption entry gain, per NAME, the mIoU (the reference's MulticlassJaccardIndex(19, ignore_index=255)) and NAME_acc (pixel
    accuracy) of the restored images (val_lq/NAME; by_corruption: NAME) and of the unrestored inputs (val_input/NAME;
    by_corruption: input/NAME).  deeplab: the same form with deeplab.ARCHS and deeplab.DeepLabWeights - the reference's other
    segmenter, DeepLabV3+, scored under the same keys (a name may be used by only one of the two).
    detect: "NAME=ARCH:WEIGHTS.pth,..." or {NAME: (ARCH, path) | detect.DetectorWeights} - RetinaNet mAP of the "det" output against
    the data's boxes (tasks must hold "det", the config's tedit.task too, the data must be built with labels: boxes): the result and
    every by_corruption entry gain, per NAME, the mAP at the one IoU threshold det_iou (0.5; the reference's
    MeanAveragePrecision(iou_thresholds=[t])) of the restored images (val_lq/NAME; by_corruption: NAME) and of the unrestored inputs
    (val_input/NAME; by_corruption: input/NAME) over the detections scoring above det_score (0.05, torchvision's default), and
    det_nonfinite = [restored, input], the images whose detector outputs were not finite.
    crop: (H, W) or "H,W", the centre crop's size instead of 512 x 512.
    niqe: a file of NIQE model parameters (.pt / .pth / .npz / .mat with mu_prisparam and cov_prisparam; the user's, none ship with
    the project) or a loaded niqe.NiqeParams - the no-reference NIQE score (fp64 on the GPU) of the restored images (val_lq/niqe;
    by_corruption: niqe) and of the unrestored inputs (val_input/niqe; by_corruption: input/niqe), each the mean over the images
    with a finite score, and niqe_skipped = [restored, input], the images without one.  The crop must hold two 96 x 96 blocks."""
    import torch
    if niqe is not None:
        niqe = check_niqe_arg(niqe)                       # before the model is built
    if lpips is not None and isinstance(lpips, (str, tuple, list)):
        lpips = check_lpips_arg(lpips)                    # before the model is built
    classify, cls_flag = check_classifiers_arg(classify, vit, swin, rvt, vgg)  # before the model is built; from here on one dict of classifiers
    segment, seg_flag = check_segmenters_arg(segment, deeplab)      # from here on one dict of segmenters
    det_args = {}
    if detect is not None:
        detect = check_detect_arg(detect, det_score, det_iou)     # before the model is built
        det_args = dict(detectors=detect, det_score=det_score, det_iou=det_iou)
    crop_args = {} if crop is None else dict(crop=check_crop_arg(crop))
    r = resolve(cfg, allow_16bit=allow_16bit)
    if tasks is not None:
        tasks = list(tasks)
        if "ir" not in tasks:
            raise ValueError(f"--tasks {','.join(tasks)}: PSNR / SSIM are computed on the 'ir' output; add 'ir' to the list "
                             "(it is not added silently)")
    if classify is not None:
        check_classify_run(classify, tasks, r, flag=cls_flag)
    if segment is not None:
        check_segment_run(segment, tasks, r, flag=seg_flag)
    if detect is not None:
        check_detect_run(detect, tasks, r)
    niqe_args = {}
    if niqe is not None:
        check_niqe_run(crop_args.get("crop"), r)
        niqe_args = dict(niqe_params=niqe)
    from . import data as data_mod
    from .dist import all_gather_images, shard_range
    rank, world, dev, dist, lit = _start(r, hf_root, random_init, model, metrics_device=metrics_device, lpips_weights=lpips,
                                         classifiers=classify, segmenters=segment, **crop_args, **niqe_args, **det_args,
                                         **r["caller_args"])
    pairs = lit.NIQE_KEYS if niqe is not None else ()     # the NIQE states: fp64 [2] device tensors (sum of finite scores, count)
    sums = ("psnr", "ssim") + (("lpips",) if lpips is not None else ())          # the metric states, in all-reduce order
    counts = [k for name in (classify or {}) for k in lit.classifier_keys(name)]  # the classifiers' int64 [3, classes] count states
    counts += [k for name in (segment or {}) for k in lit.segmenter_keys(name)]   # the segmenters' int64 [classes, classes] matrices
    data = getattr(data_mod, r["data_class"].rsplit(".", 1)[1])(**r["data_args"])
    if data.batch_size < world:
        raise ValueError(f"data batch_size {data.batch_size} < world size {world}: every rank needs at least one image per batch")
    sizes = [shard_range(data.batch_size, q, world)[1] - shard_range(data.batch_size, q, world)[0] for q in range(world)]
    n_img, secs, finite = 0, 0.0, True
    # a dataset of files degraded on the GPU says what its last batch was: "fog/3" (data.JpegImageFiles: "jpeg/10", the quality)
    # -> metric sums of its batches
    by_corruption = {} if hasattr(data, "last") else None
    det_by = {}                                           # "fog/3" -> {totals key: detect.MeanAP of its batches}
    for i, batch in enumerate(data.batches(rank, world, dev)):
        if max_batches is not None and i >= max_batches:
            break
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        preds = lit.validation_step(batch, metrics=False, tasks=tasks)          # forward only inside the timed region
        by_task = preds[-1] if tasks is not None else {"ir": preds[-1]}
        out = by_task["ir"]
        if world > 1:
            out = all_gather_images(out, sizes)
        torch.cuda.synchronize()
        if i >= 1:                                        # batch 0 captures the hipGraph: time from the second one
            secs += time.perf_counter() - t0
            n_img += out.shape[0]
        finite = finite and bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(v).all()) for v in by_task.values())
        before = dict(lit.totals)
        lit.update_metrics(by_task["ir"], batch[1])           # this rank's shard; reduced over the ranks below (fp64 PSNR / SSIM: untimed)
        if classify is not None:
            lit.update_classification(by_task["cls"], batch[0], batch[2])
        if segment is not None:
            lit.update_segmentation(by_task["seg"], batch[0], batch[2])
        if detect is not None:                            # the metric update is host fp64, untimed like the others
            batch_ap = lit.update_detection(by_task["det"], batch[0], batch[2])
            if by_corruption is not None:
                mine = det_by.setdefault("%s/%d" % data.last, {})
                for k, ap in batch_ap.items():
                    mine[k] = mine[k].merge(ap) if k in mine else ap
        lit.update_niqe(by_task["ir"], batch[0])              # (nothing without --niqe)
        if by_corruption is not None:                     # the batch is homogeneous: its increment of the totals belongs to one key
            acc = by_corruption.setdefault("%s/%d" % data.last, dict({k: 0.0 for k in sums}, **{k: 0 for k in counts},
                                                                     **{k: 0.0 for k in pairs}, images=0))
            for k in acc:
                acc[k] = acc[k] + (lit.totals[k] - before[k])
    if world > 1:                                         # the reference's metric states reduce with dist_reduce_fx="sum"
        # the totals are host floats (metrics_device "cpu") or 0-d fp64 device tensors ("gpu")
        tot = torch.stack([torch.as_tensor(v, dtype=torch.float64, device=dev)
                           for v in [lit.totals[k] for k in sums] + [float(lit.totals["images"])]])
        dist.all_reduce(tot)
        lit.totals.update({k: float(tot[i]) for i, k in enumerate(sums)}, images=int(tot[-1]))
        if counts:                                        # appended to the reduced states: one more all-reduce, of integers
            flat = torch.cat([lit.totals[k].to(dev).reshape(-1) for k in counts])
            dist.all_reduce(flat)
            for k, part in zip(counts, flat.split([lit.totals[k].numel() for k in counts])):
                lit.totals[k] = part.view_as(lit.totals[k])
        if detect is not None:                            # the per-class (score, tp) lists: every rank's, merged in rank order
            mine = ({k: lit.totals[k] for name in detect for k in lit.detector_keys(name)}, lit.det_nonfinite, det_by)
            everyone = [None] * world
            dist.all_gather_object(everyone, mine)
            totals, lit.det_nonfinite, det_by = merge_detection_states(everyone, det_iou)
            lit.totals.update(totals)
        if pairs:                                         # the NIQE sums and counts, and the images they were asked for
            flat = torch.cat([lit.totals[k].to(dev) for k in pairs] + [torch.tensor([lit.niqe_seen], dtype=torch.float64, device=dev)])
            dist.all_reduce(flat)
            for j, k in enumerate(pairs):
                lit.totals[k] = flat[2 * j:2 * j + 2].clone()
            lit.niqe_seen = int(flat[-1])
    res = dict(config=r["data_args"], dtype=r["dtype"], n_gpus=world, denoise_steps=r["model_kwargs"]["cnet"]["num_inference_steps"],
               images_per_s=(n_img / secs) if secs > 0 else None, output_finite=finite, **lit.metrics())
    if tasks is not None:
        res["tasks"] = tasks
    if by_corruption is not None:
        res["by_corruption"] = {k: dict({m: float(v[m]) / v["images"] for m in sums}, images=int(v["images"]))
                                for k, v in by_corruption.items()}
        from .classify import accuracy
        for k, v in by_corruption.items():
            for name in (classify or {}):
                for prefix, key in zip(("", "input/"), lit.classifier_keys(name)):
                    res["by_corruption"][k][f"{prefix}{name}"], res["by_corruption"][k][f"{prefix}{name}_top1"] = accuracy(*v[key])
            for name in (segment or {}):
                from .segment import miou
                for prefix, key in zip(("", "input/"), lit.segmenter_keys(name)):
                    res["by_corruption"][k][f"{prefix}{name}"], res["by_corruption"][k][f"{prefix}{name}_acc"] = miou(v[key])[:2]
            for name in (detect or {}):
                for prefix, key in zip(("", "input/"), lit.detector_keys(name)):
                    res["by_corruption"][k][f"{prefix}{name}"] = det_by[k][key].compute()["map"]
            for prefix, key in zip(("", "input/"), pairs):    # the mean over this key's images with a finite score
                total, count = v[key].tolist()
                res["by_corruption"][k][f"{prefix}niqe"] = total / count if count else float("nan")
        if hasattr(data, "skipped"):
            res["skipped"] = list(data.skipped)
        if data.resize is not None:
            res["resize"] = list(data.resize)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return res if rank == 0 else None


def check_restore_args(r: dict, inp, output, task=None, tasks=None, batch=8):
    """Everything about a `restore` call that can be wrong without looking at a GPU -> (input paths, a task name or a tuple
    of names).  r = resolve(cfg).  Every message names the offending argument."""
    from . import imageio
    if task is not None and tasks is not None:
        raise ValueError("--task and --tasks exclude each other: one output folder, or one sub-folder per task")
    names = [t for t in tasks.split(",") if t] if isinstance(tasks, str) else (list(tasks) if tasks is not None else None)
    if names is not None and (not names or len(set(names)) != len(names)):
        raise ValueError(f"--tasks {tasks!r}: needs at least one task name, each once")
    known = list((r["model_kwargs"].get("tedit") or {}).get("task") or [])
    for t in (names if names is not None else [task or "ir"]):
        if known and t not in known:
            raise KeyError(f"--task{'s' if names is not None else ''}: unknown task {t!r}; the config's task editor knows {known}")
    if int(batch) < 1:
        raise ValueError(f"--batch {batch}: must be >= 1")
    if not inp or not os.path.exists(inp):
        raise FileNotFoundError(f"--input {inp!r}: no such folder or list file")
    if not output:
        raise ValueError("--output: a folder for the restored PNGs is required")
    if os.path.isdir(inp) and os.path.realpath(inp) == os.path.realpath(output):
        raise ValueError(f"--output {output!r} is the --input folder: the restored files would overwrite or join the inputs")
    paths = imageio.list_inputs(inp)
    if not paths:
        raise ValueError(f"--input {inp!r}: no image file found (extensions PIL can read; a folder is not searched recursively)")
    missing = [p for p in paths if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError(f"--input {inp!r}: {len(missing)} listed file(s) do not exist, first {missing[0]!r}")
    stems = {}
    for p in paths:
        stem = os.path.splitext(os.path.basename(p))[0]
        if stem in stems:
            raise ValueError(f"--input {inp!r}: {stems[stem]!r} and {p!r} would both be written to {stem}.png")
        stems[stem] = p
    return paths, (tuple(names) if names is not None else (task or "ir"))


NOISE_MODES = ("batch", "image")


def image_seed(seed: int, stem: str, sample: int = 0) -> int:
    """The 64-bit noise seed of sample `sample` of the input named `stem` under the config's seed_everything (--noise image): a
    pure function of the three, so a file's noise does not depend on the other files, their order, --batch or the world size."""
    import hashlib
    return int.from_bytes(hashlib.sha256(f"{seed}\0{stem}\0{sample}".encode()).digest()[:8], "little")


def check_noise_args(noise="batch", samples=1):
    """--noise / --samples of a `restore` call -> (noise mode, K); ValueError names the offending argument."""
    if noise not in NOISE_MODES:
        raise ValueError(f"--noise {noise!r}: choose from {list(NOISE_MODES)}")
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise ValueError(f"--samples {samples!r}: must be an integer >= 1")
    if samples > 1 and noise != "image":
        raise ValueError(f"--samples {samples} needs --noise image: with --noise batch a file's noise belongs to its batch, "
                         "so its samples cannot be told apart")
    return noise, samples


def plan_samples(paths, samples=1):
    """Every input K times, consecutively: [(path, stem, k)] in the order the batches are planned in."""
    return [(p, os.path.splitext(os.path.basename(p))[0], k) for p in paths for k in range(samples)]


def output_name(stem: str, sample: int, samples: int) -> str:
    """<stem>.png for one sample per input, <stem>.s<k>.png for several."""
    return f"{stem}.png" if samples == 1 else f"{stem}.s{sample}.png"


def batch_seeds(seed: int, units, members):
    """The seeds of a batch's slots under --noise image: units = plan_samples(...), members = the batch's indices into it.  A slot
    that a padded batch repeats carries the repeated image's seed."""
    return [image_seed(seed, units[i][1], units[i][2]) for i in members]


def restore_noise(seed: int, index: int, n: int, canvas, latent_channels: int = 4):
    """The two noise tensors of batch `index` of a restore plan: a host generator seeded from the config's seed_everything and
    the batch's index in the plan of ALL ranks, so a rerun draws the same noise whatever the world size."""
    import torch
    g = torch.Generator().manual_seed(int(seed) * 1000003 + int(index))
    shape = (n, latent_channels, canvas[0] // 8, canvas[1] // 8)
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def restore(cfg: dict, inp, output, task=None, tasks=None, batch=8, hf_root=None, allow_16bit=False, random_init=True,
            model=None, noise="batch", samples=1) -> dict:
    """Restore image files: OUTPUT/<stem>.png (OUTPUT/<task>/<stem>.png with tasks), each the size of its input.  Files are
    grouped by canvas (imageio.plan_batches) and every batch is one DiffUIE.forward_u8 call: uint8 in, uint8 out, one captured
    graph per (batch size, canvas).  Under torch.distributed.run rank r restores batches r, r + world, ... of the same plan and
    writes its own files; no collective runs inside the loop.  model: a ready DiffUIE to use instead of building the config's.
    noise "batch": one host draw per batch (restore_noise), a file's noise depends on its batch and slot.  noise "image": every
    file's noise is generated on the device from image_seed(seed_everything, stem, k) alone; samples = K then restores every
    input K times (k = 0..K-1) into <stem>.s<k>.png."""
    import torch
    noise, samples = check_noise_args(noise, samples)
    r = resolve(cfg, allow_16bit=allow_16bit)
    paths, which = check_restore_args(r, inp, output, task, tasks, batch)
    from . import imageio
    sizes = [hw for _, hw in imageio.scan(paths) for _k in range(samples)]
    units = plan_samples(paths, samples)                   # what the plan's indices mean: (path, stem, sample)
    paths = [u[0] for u in units]
    rank, world, _ = _ranks()
    plan = imageio.plan_batches(sizes, int(batch), rank, world)
    rank, world, dev, dist, lit = _start(r, hf_root, random_init, model)
    model = lit.model
    out_dirs = {t: os.path.join(output, t) for t in which} if isinstance(which, tuple) else {which: output}
    for d in out_dirs.values():
        os.makedirs(d, exist_ok=True)
    captures_before, saves = model.graph_captures, []
    n_img, n_timed, secs, finite = 0, 0, 0.0, True
    t_all = time.perf_counter()
    with imageio.io_pool() as pool:
        for b, images in imageio.Prefetcher(plan, paths, pool):
            if noise == "image":                            # a repeated slot of a padded batch carries the repeated image's seed
                draws = dict(seeds=batch_seeds(r["seed"], units, b.members))
            else:
                draws = dict(noise=restore_noise(r["seed"], b.index, len(b.members), b.canvas, model.ae.vae.latent_channels))
            torch.cuda.synchronize()
            captures, t0 = model.graph_captures, time.perf_counter()
            preds = model.forward_u8(images, which, **draws)
            by_task = preds if isinstance(which, tuple) else {which: preds}
            host = {t: [x.cpu() for x in v[:b.valid]] for t, v in by_task.items()}      # the repeats of a padded batch are dropped
            dt = time.perf_counter() - t0
            finite = finite and not any(model.u8_nonfinite())
            if model.graph_captures == captures:          # a batch that captured its graph is not timed (validate: batch 0)
                secs += dt
                n_timed += b.valid
            n_img += b.valid
            while len(saves) > 4 * int(batch):            # bounded: encoding must not fall behind without limit
                saves.pop(0).result()
            for t, imgs in host.items():
                for i, x in zip(b.members, imgs):
                    name = output_name(units[i][1], units[i][2], samples)
                    saves.append(pool.submit(imageio.save_u8, x, os.path.join(out_dirs[t], name)))
        for f in saves:
            f.result()
    total_s = time.perf_counter() - t_all
    graphs = model.graph_captures - captures_before
    counts = torch.tensor([n_img, n_timed, graphs, 0 if finite else 1], dtype=torch.float64, device=dev)
    times = torch.tensor([secs, total_s], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(counts)
        dist.all_reduce(times, op=dist.ReduceOp.MAX)
    n_img, n_timed, graphs, bad = (int(v) for v in counts.tolist())
    secs, total_s = times.tolist()
    res = dict(images=n_img, input_sizes=len(set(sizes)), canvases=len({imageio.canvas_of(h, w) for h, w in sizes}),
               graphs_captured=graphs, batch=int(batch), tasks=list(which) if isinstance(which, tuple) else [which],
               dtype=r["dtype"], n_gpus=world, denoise_steps=r["model_kwargs"]["cnet"]["num_inference_steps"],
               images_per_s=(n_timed / secs) if secs > 0 else None, images_timed=n_timed, seconds_total=total_s,
               output_finite=not bad, output=output, noise=noise, samples=samples)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return res if rank == 0 else None


def check_resize_arg(resize, minimum: int):
    """--resize LO,HI (or a pair of integers, or None) -> (lo, hi) or None; the message names --resize."""
    from . import resize as rz
    if resize is None:
        return None
    try:
        return rz.check_range(resize, minimum)
    except ValueError as e:
        raise ValueError(f"--{e}") from None


def _check_file_args(inp, output, batch, what: str):
    """What the corrupt, distort and jpeg commands check alike: --batch, --input and --output, a folder for `what` -> the clean
    image paths.  Every message names the offending argument."""
    from . import corrupt as cr
    if int(batch) < 1:
        raise ValueError(f"--batch {batch}: must be >= 1")
    if not inp or not os.path.exists(inp):
        raise FileNotFoundError(f"--input {inp!r}: no such folder or list file")
    if not output:
        raise ValueError(f"--output: a folder for the {what} is required")
    if os.path.isdir(inp) and os.path.realpath(inp) == os.path.realpath(output):
        raise ValueError(f"--output {output!r} is the --input folder")
    try:
        return cr.check_inputs(inp)
    except ValueError as e:
        raise ValueError(f"--input {e}") from None


def _check_severity_arg(severity):
    """--severity -> an integer 1..5 or "mixed" as it was given."""
    if str(severity) == "mixed":
        return severity
    if str(severity) not in ("1", "2", "3", "4", "5"):
        raise ValueError(f"--severity {severity!r}: choose 1..5 or mixed")
    return int(severity)


def _write_degraded(degrade, paths, sizes, jobs, batch, output):
    """OUTPUT/<folder>/<stem>.png and OUTPUT/<folder>/pairs.txt (one `lq hq` line per file, in input order).  jobs[i] lists what
    becomes of paths[i], of size sizes[i], as (folder name, key) pairs, equally many for every file; the files are grouped by
    (shape, folder, key), the groups cut into batches, and a batch is degrade(hq, key, stems).  -> (the folder names in the
    order they were begun, seconds)."""
    import torch
    from . import corrupt as cr
    from . import imageio
    dev = torch.device("cuda", torch.cuda.current_device())
    stems = [cr.stem_of(p) for p in paths]
    groups = {}
    for k in range(len(jobs[0])):                         # job by job, a job's groups in the order of their first file
        for i, hw in enumerate(sizes):
            groups.setdefault((hw, *jobs[i][k]), []).append(i)
    t0, folders = time.perf_counter(), {}
    for (_, name, key), idx in groups.items():
        folder = os.path.join(output, name)
        os.makedirs(folder, exist_ok=True)
        for s in range(0, len(idx), int(batch)):
            cut = idx[s:s + int(batch)]
            hq = torch.stack([imageio.load_u8(paths[i]) for i in cut]).to(dev)
            lq = degrade(hq, key, [stems[i] for i in cut]).cpu()
            for i, img in zip(cut, lq):
                imageio.save_u8(img, os.path.join(folder, stems[i] + ".png"))
        folders.setdefault(folder, []).extend(idx)
    for folder, idx in folders.items():
        with open(os.path.join(folder, "pairs.txt"), "w") as f:
            for i in sorted(idx):
                f.write(f"{stems[i]}.png {os.path.abspath(paths[i])}\n")
    return [os.path.basename(d) for d in folders], time.perf_counter() - t0


def _check_corruption_args(planner, hint, inp, output, corruptions, severity, batch, resize):
    """`check_corrupt_args` / `check_distort_args`: planner is unirestore_amd.corrupt or .distort, hint what --corruptions may name."""
    check_resize_arg(resize, 32)
    if not corruptions:
        raise ValueError("--corruptions: name at least one " + hint)
    try:
        names = planner.expand(corruptions)
    except ValueError as e:
        raise ValueError(f"--corruptions {corruptions!r}: {e}") from None
    if "clean" in names:                                  # (corrupt only: distort.expand knows no such name)
        raise ValueError("--corruptions: 'clean' writes nothing new; name corruptions only")
    severity = _check_severity_arg(severity)
    return _check_file_args(inp, output, batch, "corrupted PNGs"), names, severity


def check_corrupt_args(inp, output, corruptions, severity=3, batch=8, resize=None):
    """Everything about a `corrupt` call that can be wrong without looking at a GPU -> (clean image paths, corruption names, an
    integer severity or "mixed").  Every message names the offending argument.  resize: None, "LO,HI" or (lo, hi), checked only."""
    from . import corrupt as cr
    return _check_corruption_args(cr, "corruption or subset (" + ", ".join(sorted(cr.SUBSETS)) + ")", inp, output, corruptions, severity,
                                  batch, resize)


def check_distort_args(inp, output, corruptions, severity=3, batch=8, resize=None):
    """`check_corrupt_args` for a `distort` call: the names are unirestore_amd.distort's (glass_blur, snow, elastic_transform, all)."""
    from . import distort as ds
    return _check_corruption_args(ds, "of " + ", ".join(ds.NAMES) + " or all", inp, output, corruptions, severity, batch, resize)


def _corruption_files(check, degrade, skipped, inp, output, corruptions, severity, seed, batch, resize):
    """`corrupt_files` / `distort_files`: check is the command's argument check, degrade corrupt.degrade or distort.degrade,
    skipped(corruptions) the subset members that are not built."""
    import torch
    from . import corrupt as cr
    from . import imageio
    paths, names, severity = check(inp, output, corruptions, severity, batch, resize)
    resize = check_resize_arg(resize, 32)
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the corruptions run on MI355X only (no CPU fallback)")
    sevs = [cr.draw_severity(seed, cr.stem_of(p)) if severity == "mixed" else severity for p in paths]
    folders, seconds = _write_degraded(lambda hq, key, stems: degrade(hq, *key, seed, stems, resize), paths,
                                       [hw for _, hw in imageio.scan(paths)],
                                       [[(f"{name}_{sev}", (name, sev)) for name in names] for sev in sevs], batch, output)
    return dict(images=len(paths), corruptions=names, skipped=skipped(corruptions), severity=severity, seed=seed, folders=sorted(folders),
                output=output, seconds_total=seconds, **({"resize": list(resize)} if resize is not None else {}))


def corrupt_files(inp, output, corruptions, severity=3, seed=42, batch=8, resize=None) -> dict:
    """Corrupt clean image files on the GPU: OUTPUT/<name>_<severity>/<stem>.png for every named corruption and input, and
    OUTPUT/<name>_<severity>/pairs.txt with one `lq hq` line per file (what data.ImageListFiles and the reference's list datasets
    read).  A file's bytes depend on (seed, stem, name, severity) alone - not on the other files, their order or --batch.
    resize = "LO,HI" or (lo, hi): every file is corrupted inside the resize-down / resize-back wrapper (corrupt.degrade), its short
    edge drawn from [lo, hi) by (seed, stem); the folders and pairs.txt are what they are without it."""
    from . import corrupt as cr
    return _corruption_files(check_corrupt_args, cr.degrade, cr.skipped, inp, output, corruptions, severity, seed, batch, resize)


def distort_files(inp, output, corruptions, severity=3, seed=42, batch=8, resize=None) -> dict:
    """`corrupt_files` for glass_blur, snow and elastic_transform (unirestore_amd.distort): the same folders, pairs.txt and result,
    a file's bytes depending on (seed, stem, name, severity) alone."""
    from . import distort as ds
    return _corruption_files(check_distort_args, ds.degrade, lambda c: [], inp, output, corruptions, severity, seed, batch, resize)


def check_jpeg_args(inp, output, quality, subsampling="4:2:0", batch=8, resize=None):
    """Everything about a `jpeg` call that can be wrong without looking at a GPU -> (clean image paths, the qualities as integers,
    each once, the subsampling code).  Every message names the offending argument.  resize: None, "LO,HI" or (lo, hi), checked only."""
    from . import jpeg
    check_resize_arg(resize, jpeg.MIN_SIDE)
    specs = [s for s in str(quality).split(",") if s.strip()] if quality is not None else []
    if not specs:
        raise ValueError("--quality: name at least one quality (1..100, or s1..s5 for the reference's severities), e.g. 10,25,s3")
    qualities = []
    for s in specs:
        try:
            q = jpeg.quality_of(s)
        except ValueError as e:
            raise ValueError(f"--quality {quality!r}: {e}") from None
        if q not in qualities:
            qualities.append(q)
    try:
        code = jpeg.subsampling_code(subsampling)
    except ValueError as e:
        raise ValueError(f"--subsampling: {e}") from None
    return _check_file_args(inp, output, batch, "compressed images' PNGs"), qualities, code


def jpeg_files(inp, output, quality, subsampling="4:2:0", batch=8, resize=None, seed=42) -> dict:
    """JPEG-compress clean image files on the GPU: OUTPUT/jpeg_q<Q>/<stem>.png (the decoded bytes, stored losslessly) for every
    quality and input, and OUTPUT/jpeg_q<Q>/pairs.txt with one `lq hq` line per file (what data.ImageListFiles reads).  A file's
    bytes depend on (the clean file, quality, subsampling) alone - there is no seed - unless resize = "LO,HI" or (lo, hi) puts the
    round trip inside the resize-down / resize-back wrapper (jpeg.degrade): the short edge is then drawn from [lo, hi) by
    (seed, stem)."""
    import torch
    paths, qualities, code = check_jpeg_args(inp, output, quality, subsampling, batch, resize)
    from . import imageio, jpeg
    resize = check_resize_arg(resize, jpeg.MIN_SIDE)
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the JPEG round trip runs on MI355X only (no CPU fallback)")
    sizes = [hw for _, hw in imageio.scan(paths)]
    small = [p for p, hw in zip(paths, sizes) if min(hw) < jpeg.MIN_SIDE]
    if small:
        raise ValueError(f"--input: {len(small)} image(s) smaller than {jpeg.MIN_SIDE} x {jpeg.MIN_SIDE}, first {small[0]!r}")
    folders, seconds = _write_degraded(lambda hq, q, stems: jpeg.degrade(hq, q, seed, stems, resize, code), paths, sizes,
                                       [[(f"jpeg_q{q}", q) for q in qualities]] * len(paths), batch, output)
    return dict(images=len(paths), qualities=qualities, subsampling={2: "4:2:0", 0: "4:4:4"}[code], folders=folders, output=output,
                seconds_total=seconds, **({"resize": list(resize), "seed": seed} if resize is not None else {}))


# the commands that write degraded copies of clean files: (the argument check, the command, what the check may raise)
FILE_COMMANDS = {"corrupt": (check_corrupt_args, corrupt_files, (ValueError, FileNotFoundError, NotImplementedError)),
                 "distort": (check_distort_args, distort_files, (ValueError, FileNotFoundError, NotImplementedError)),
                 "jpeg": (check_jpeg_args, jpeg_files, (ValueError, FileNotFoundError))}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unirestore_amd.cli")
    ap.add_argument("command", choices=["validate", "print_config", "restore", "corrupt", "jpeg", "distort"])
    ap.add_argument("--config", default=None, help="validate / print_config / restore: the YAML config (required there)")
    ap.add_argument("--set", action="append", default=[], metavar="a.b.c=value", help="override a config key")
    ap.add_argument("--hf-root", default=None, help="folder with unet/ and vae/ diffusion_pytorch_model.safetensors (sd-turbo)")
    ap.add_argument("--max-batches", type=int, default=None)
    ap.add_argument("--allow-16bit", action="store_true", help="run a `precision: 32` config in fp16 (fp32 accumulation) instead of refusing it")
    ap.add_argument("--metrics-device", choices=["cpu", "gpu"], default="cpu",
                    help="where PSNR / SSIM run: cpu = host fp64 (default), gpu = the HIP metric kernels (fp64, no per-batch host sync)")
    ap.add_argument("--lpips", default=None, metavar="ALEXNET.pth,LIN.pth",
                    help="validate: also report LPIPS (AlexNet, fp32, on the GPU) from these two user-supplied weight files")
    ap.add_argument("--classify", default=None, metavar="NAME=ARCH:WEIGHTS.pth[,...]",
                    help="validate: also report ResNet top-1 accuracy of the 'cls' output (fp32, on the GPU) against the data's labels; "
                         "ARCH is resnet18, resnet50 or resnet101, WEIGHTS a user-supplied torchvision state dict; needs --tasks with "
                         "cls and a dataset built with labels: true")
    ap.add_argument("--vit", default=None, metavar="NAME=ARCH:WEIGHTS.pth[,...]",
                    help="validate: also report ViT top-1 accuracy of the 'cls' output (fp32, on the GPU) against the data's labels; ARCH "
                         "is vit_b_16, vit_b_32, vit_l_16 or vit_l_32, WEIGHTS a user-supplied torchvision state dict; needs --tasks "
                         "with cls and a dataset built with labels: true; a NAME may not be one of --classify's")
    ap.add_argument("--swin", default=None, metavar="NAME=ARCH:WEIGHTS.pth[,...]",
                    help="validate: also report Swin-V2 top-1 accuracy of the 'cls' output (fp32, on the GPU) against the data's labels; "
                         "ARCH is swin_v2_t, swin_v2_s or swin_v2_b, WEIGHTS a user-supplied torchvision state dict; needs --tasks "
                         "with cls and a dataset built with labels: true; a NAME may not be one of --classify's or --vit's")
    ap.add_argument("--rvt", default=None, metavar="NAME=ARCH:WEIGHTS.pth[,...]",
                    help="validate: also report Robust Vision Transformer top-1 accuracy of the 'cls' output (fp32, on the GPU) against "
                         "the data's labels; ARCH is rvt_tiny, rvt_small, rvt_base or one of their _plus variants, WEIGHTS a user-supplied "
                         "RVT checkpoint; needs --tasks with cls and a dataset built with labels: true; a NAME may not be one of "
                         "--classify's, --vit's or --swin's")
    ap.add_argument("--vgg", default=None, metavar="NAME=ARCH:WEIGHTS.pth[,...]",
                    help="validate: also report VGG top-1 accuracy of the 'cls' output (fp32, on the GPU) against the data's labels; ARCH "
                         "is vgg11, vgg13, vgg16, vgg19 or one of their _bn variants, WEIGHTS a user-supplied torchvision state dict; "
                         "needs --tasks with cls and a dataset built with labels: true; a NAME may not be one of --classify's, --vit's, "
                         "--swin's or --rvt's")
    ap.add_argument("--segment", default=None, metavar="NAME=ARCH:WEIGHTS.pth[,...]",
                    help="validate: also report RefineNet-LW mIoU and pixel accuracy of the 'seg' output (fp32, on the GPU) against the "
                         "data's label maps; ARCH is rflw50, rflw101 or rflw152, WEIGHTS a user-supplied state dict; needs --tasks with "
                         "seg and a dataset built with labels: map")
    ap.add_argument("--deeplab", default=None, metavar="NAME=ARCH:WEIGHTS.pth[,...]",
                    help="validate: also report DeepLabV3+ (output stride 16) mIoU and pixel accuracy of the 'seg' output (fp32, on the "
                         "GPU) against the data's label maps; ARCH is dlv3pr50 or dlv3pr101, WEIGHTS a user-supplied checkpoint; needs "
                         "--tasks with seg and a dataset built with labels: map; a NAME may not be one of --segment's")
    ap.add_argument("--detect", default=None, metavar="NAME=ARCH:WEIGHTS.pth[,...]",
                    help="validate: also report RetinaNet mAP of the 'det' output (fp32, on the GPU; the metric in fp64 on the host) "
                         "against the data's boxes; ARCH is retinanet_resnet50_fpn_v2, WEIGHTS a user-supplied torchvision state dict; "
                         "needs --tasks with det, a config whose tedit.task holds det and a dataset built with labels: boxes")
    ap.add_argument("--det-score", type=float, default=None, metavar="T",
                    help="validate --detect: the detector's score threshold (default 0.05, torchvision's own)")
    ap.add_argument("--det-iou", type=float, default=None, metavar="T",
                    help="validate --detect: the IoU threshold of the mAP (default 0.5)")
    ap.add_argument("--crop", default=None, metavar="H,W",
                    help="validate: the evaluator's centre crop (default 512,512; the reference's seg evaluator uses 960,1664)")
    ap.add_argument("--niqe", default=None, metavar="PARAMS",
                    help="validate: also report the no-reference NIQE score (fp64, on the GPU) of the restored images and of the inputs; "
                         "PARAMS is a user-supplied file of model parameters (.pt / .pth / .npz / .mat with mu_prisparam and "
                         "cov_prisparam); the crop must hold two 96 x 96 blocks")
    ap.add_argument("--tasks", default=None, metavar="ir,cls,seg,det",
                    help="restore every batch once and decode it for each of these tasks (forward_tasks); validate: must hold 'ir', which "
                         "feeds PSNR / SSIM; restore: one sub-folder of --output per task")
    ap.add_argument("--task", default=None, help="restore: the task to decode for (default ir)")
    ap.add_argument("--input", default=None, help="restore: a folder of images, or a text file with one path (or `lq hq label`) per line")
    ap.add_argument("--output", default=None, help="restore: folder for <stem>.png")
    ap.add_argument("--color-fix", choices=list(COLOR_FIX_CHOICES), default=None,
                    help="validate / restore: colour fix of the restored images against the inputs (DiffUIE.set_color_fix); overrides "
                         "the config's cnet.color_fix, none turns it off")
    ap.add_argument("--batch", type=int, default=8, help="restore: images per forward (images of a batch share a canvas)")
    ap.add_argument("--noise", choices=list(NOISE_MODES), default="batch",
                    help="restore: batch = one host draw per batch (a file's noise depends on its batch and slot); image = every file's "
                         "noise is generated on the GPU from (seed_everything, file stem, sample) alone")
    ap.add_argument("--samples", type=int, default=1, metavar="K",
                    help="restore: K restorations of every input, written as <stem>.s<k>.png (K > 1 needs --noise image)")
    ap.add_argument("--corruptions", default=None, metavar="fog,motion_blur|SUBSET",
                    help="corrupt: corruption names and / or subsets (common, validation, all, noise, blur, weather, digital); "
                         "distort: glass_blur, snow, elastic_transform or all")
    ap.add_argument("--severity", default="3", help="corrupt / distort: 1..5, or mixed for the reference's per-image draw")
    ap.add_argument("--seed", type=int, default=42, help="corrupt / distort: with a file's stem, the seed of all its randomness; jpeg: of the --resize draw")
    ap.add_argument("--resize", default=None, metavar="LO,HI",
                    help="corrupt / distort / jpeg: degrade inside the reference's wrapper - resize every image so that its short edge is an integer "
                         "drawn from [LO, HI) by (seed, stem), degrade at that size, resize back (the reference draws from [128, 512))")
    ap.add_argument("--quality", default=None, metavar="10,25,s3", help="jpeg: qualities 1..100 and / or s1..s5 (the reference's severities)")
    ap.add_argument("--subsampling", default="4:2:0", help="jpeg: 4:2:0 (Pillow's and the reference's default) or 4:4:4")
    a = ap.parse_args(argv)
    for flag in ("classify", "vit", "swin", "rvt", "vgg", "segment", "deeplab", "crop", "niqe", "detect", "det_score", "det_iou"):
        if getattr(a, flag) is not None and a.command != "validate":
            ap.error(f"--{flag.replace('_', '-')} belongs to validate")
    if a.detect is None and (a.det_score is not None or a.det_iou is not None):
        ap.error("--det-score and --det-iou belong to --detect")
    a.det_score = 0.05 if a.det_score is None else a.det_score
    a.det_iou = 0.5 if a.det_iou is None else a.det_iou
    if a.command in FILE_COMMANDS:
        check, run, errors = FILE_COMMANDS[a.command]
        kw = dict(inp=a.input, output=a.output, batch=a.batch, resize=a.resize)
        kw.update(dict(quality=a.quality, subsampling=a.subsampling) if a.command == "jpeg" else
                  dict(corruptions=a.corruptions, severity=a.severity))
        try:
            check(**kw)
        except errors as e:
            ap.error(str(e))
        print(json.dumps(run(seed=a.seed, **kw)))
        return 0
    if a.config is None:
        ap.error("the following arguments are required: --config")
    if a.command == "restore":
        try:
            check_noise_args(a.noise, a.samples)
        except ValueError as e:
            ap.error(str(e))
    if a.lpips is not None:
        if a.command != "validate":
            ap.error("--lpips belongs to validate")
        try:
            a.lpips = check_lpips_arg(a.lpips)
        except ValueError as e:
            ap.error(str(e))
    tasks = [t for t in a.tasks.split(",") if t] if a.tasks is not None else None
    cfg = apply_color_fix(load_config(a.config, a.set), a.color_fix)
    try:
        classifiers, cls_flag = check_classifiers_arg(a.classify, a.vit, a.swin, a.rvt, a.vgg)
        if classifiers is not None:
            check_classify_run(classifiers, tasks, resolve(cfg, allow_16bit=a.allow_16bit), flag=cls_flag)
    except ValueError as e:
        ap.error(str(e))
    try:
        segmenters, seg_flag = check_segmenters_arg(a.segment, a.deeplab)
        if segmenters is not None:
            check_segment_run(segmenters, tasks, resolve(cfg, allow_16bit=a.allow_16bit), flag=seg_flag)
        if a.detect is not None:
            check_detect_run(check_detect_arg(a.detect, a.det_score, a.det_iou), tasks, resolve(cfg, allow_16bit=a.allow_16bit))
        if a.crop is not None:
            a.crop = check_crop_arg(a.crop)
        if a.niqe is not None:
            a.niqe = check_niqe_arg(a.niqe)
            check_niqe_run(a.crop, resolve(cfg, allow_16bit=a.allow_16bit))
    except ValueError as e:
        ap.error(str(e))
    if a.command == "print_config":
        print(yaml.safe_dump(cfg, sort_keys=False))
        print(json.dumps(resolve(cfg, allow_16bit=a.allow_16bit)))
        return 0
    if a.command == "restore":
        res = restore(cfg, a.input, a.output, task=a.task, tasks=a.tasks, batch=a.batch, hf_root=a.hf_root, allow_16bit=a.allow_16bit,
                      noise=a.noise, samples=a.samples)
        if res is not None:
            print(json.dumps(res))
        return 0
    res = validate(cfg, hf_root=a.hf_root, max_batches=a.max_batches, allow_16bit=a.allow_16bit, metrics_device=a.metrics_device,
                   tasks=tasks, lpips=a.lpips, classify=a.classify, segment=a.segment, crop=a.crop, niqe=a.niqe, deeplab=a.deeplab, vit=a.vit, swin=a.swin,
                   rvt=a.rvt, vgg=a.vgg, detect=a.detect, det_score=a.det_score, det_iou=a.det_iou)
    if res is not None:
        print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
