"""Generate tests/golden/dlv3_0.npz by running the reference's own DeepLabV3+ (`ResNet` / `Bottleneck` with
replace_stride_with_dilation=[False, False, True], `IntermediateLayerGetter`, `DeepLabHeadV3Plus`, `DeepLabV3`) in fp64.

    python tools/gen_golden_dlv3.py <reference>/src/modules/segmentation/deeplabv3

Runs ONLY where the reference checkout is at hand.  The reference Python never travels: only the produced vectors are committed.
The three modules are loaded by path - `modeling.py`, which pulls in every backbone, is not - under a stand-in package; torchvision
is not installed, and backbone/resnet.py falls back to torch.hub for the one name it wants from it.  The network is the
depth-(1, 1, 1, 1), 19-class one with deeplab.random_state_dict((1, 1, 1, 1), WEIGHT_SEED), loaded with strict=True, so every key
and shape of the stand-in layout is the reference module's.  The fixture holds the seeds, the 8-bit image, one fp64 checksum per
weight tensor (to tell a drift of the random generator from a wrong restatement), the model's output at scale 1 (every ROW_STEP-th row and
COL_STEP-th column of it) and the three-scale argmax map - nothing else.  The image is 64 x 320: its 1/16 map is 4 x 20, wider than the largest dilation, so every
horizontal ASPP tap is live somewhere.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden", "dlv3_0.npz")
WEIGHT_SEED, IMAGE_SEED, SHAPE = 31, 32, (1, 3, 64, 320)
DEPTHS, CLASSES, SCALES = (1, 1, 1, 1), 19, (1, 0.8, 0.6)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ROW_STEP, COL_STEP = 3, 7                                # the stored sub-grid of the model's output (the fixture stays below 256 KiB)


def _load(ref_dir):
    for pkg_name, path in (("refdlv3", ref_dir), ("refdlv3.backbone", os.path.join(ref_dir, "backbone"))):
        pkg = types.ModuleType(pkg_name)
        pkg.__path__ = [path]
        sys.modules[pkg_name] = pkg
    mods = {}
    for name, rel in (("refdlv3.utils", "utils.py"), ("refdlv3._deeplab", "_deeplab.py"), ("refdlv3.backbone.resnet", "backbone/resnet.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_dir, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[name.rsplit(".", 1)[1]] = mod
    return mods


def image():
    """uint8: smooth colour blobs plus noise, so that several classes appear."""
    g = torch.Generator().manual_seed(IMAGE_SEED)
    coarse = torch.rand(SHAPE[0], 3, 4, 12, generator=g)
    x = F.interpolate(coarse, size=SHAPE[2:], mode="bilinear", align_corners=True) + 0.2 * (torch.rand(SHAPE, generator=g) - 0.5)
    return torch.round(x.clamp(0, 1) * 255).to(torch.uint8)


def checksums(sd):
    """key -> sum of the tensor's values times 1, 2, 3, ... in fp64 (order-sensitive), for every floating-point tensor."""
    return {k: float((v.double().flatten() * torch.arange(1, v.numel() + 1, dtype=torch.float64)).sum())
            for k, v in sorted(sd.items()) if v.is_floating_point()}


def main(ref_dir):
    sys.path.insert(0, ROOT)
    from unirestore_amd import deeplab
    ref = _load(ref_dir)
    sd = deeplab.random_state_dict(DEPTHS, WEIGHT_SEED, CLASSES)
    backbone = ref["resnet"].ResNet(ref["resnet"].Bottleneck, list(DEPTHS), replace_stride_with_dilation=[False, False, True])
    backbone = ref["utils"].IntermediateLayerGetter(backbone, return_layers={"layer4": "out", "layer1": "low_level"})
    net = ref["_deeplab"].DeepLabV3(backbone, ref["_deeplab"].DeepLabHeadV3Plus(2048, 256, CLASSES, [6, 12, 18]))
    net.load_state_dict(sd, strict=True)
    net = net.double().eval()
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (MEAN, STD))
    u8 = image()
    x = u8.double() / 255
    h, w = x.shape[2:]
    with torch.no_grad():
        logits = net((x - mean) / std)
        ups = []
        for s in SCALES:
            xs = F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=True)
            ups.append(F.interpolate(net((xs - mean) / std), size=(h, w), mode="bilinear", align_corners=True))
        pred = torch.stack(ups).mean(0).argmax(dim=1)
    sums = checksums(sd)
    logits = logits[:, :, ::ROW_STEP, ::COL_STEP]                        # the full fp64 output would be 3 MB: every 3rd row, 7th column
    np.savez_compressed(OUT, weight_seed=WEIGHT_SEED, image_seed=IMAGE_SEED, depths=np.array(DEPTHS), scales=np.array(SCALES),
                        image=u8.numpy(), checksum_keys=np.array(list(sums)), row_step=ROW_STEP, col_step=COL_STEP,
                        checksums=np.array(list(sums.values()), dtype=np.float64), logits=logits.numpy(), pred=pred.to(torch.uint8).numpy())
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, logits {tuple(logits.shape)} |max| {float(logits.abs().max()):.2f}, "
          f"classes {sorted(set(pred.flatten().tolist()))}")


if __name__ == "__main__":
    main(sys.argv[1])
