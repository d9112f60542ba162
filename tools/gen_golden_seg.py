"""Generate tests/golden/rflw_0.npz by running the reference's own `ResNetLW` / `Bottleneck` (RefineNet-LightWeight) in fp64.

    python tools/gen_golden_seg.py <reference>/src/modules/segmentation/refinenetlw

Runs ONLY where the reference checkout is at hand.  The reference Python never travels: only the produced vectors are committed.
One shim makes refinenetlw.py importable without torchvision (not installed): torchvision.transforms.v2 with `Compose`, `Lambda`
and `Normalize`, the three transforms its preprocess uses.  The network is the depth-(1, 1, 1, 1), 19-class one with
segment.random_state_dict((1, 1, 1, 1), WEIGHT_SEED), loaded with strict=True, so every key and shape of the stand-in layout is
the reference module's.  The fixture holds the seeds, the 8-bit image, one fp64 checksum per weight tensor (to tell a drift of the
random generator from a wrong restatement), the scale-1 logits and the three-scale argmax map - nothing else.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden", "rflw_0.npz")
WEIGHT_SEED, IMAGE_SEED, SHAPE = 21, 22, (1, 3, 64, 80)
DEPTHS, CLASSES, SCALES = (1, 1, 1, 1), 19, (1, 0.8, 0.6)


def _shim():
    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class Lambda:
        def __init__(self, fn):
            self.fn = fn

        def __call__(self, x):
            return self.fn(x)

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, x):
            mean = torch.tensor(self.mean, dtype=x.dtype).view(1, -1, 1, 1)
            std = torch.tensor(self.std, dtype=x.dtype).view(1, -1, 1, 1)
            return (x - mean) / std

    tv, tr, v2 = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.v2")
    v2.Compose, v2.Lambda, v2.Normalize = Compose, Lambda, Normalize
    tv.transforms, tr.v2 = tr, v2
    for name, mod in (("torchvision", tv), ("torchvision.transforms", tr), ("torchvision.transforms.v2", v2)):
        sys.modules.setdefault(name, mod)


def _load(ref_dir):
    pkg = types.ModuleType("refrflw")
    pkg.__path__ = [ref_dir]
    sys.modules["refrflw"] = pkg
    for name in ("layer_factory", "refinenetlw"):
        spec = importlib.util.spec_from_file_location(f"refrflw.{name}", os.path.join(ref_dir, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"refrflw.{name}"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["refrflw.refinenetlw"]


def image():
    """uint8: smooth colour blobs plus noise, so that several classes appear."""
    g = torch.Generator().manual_seed(IMAGE_SEED)
    coarse = torch.rand(SHAPE[0], 3, 4, 5, generator=g)
    x = F.interpolate(coarse, size=SHAPE[2:], mode="bilinear", align_corners=True) + 0.2 * (torch.rand(SHAPE, generator=g) - 0.5)
    return torch.round(x.clamp(0, 1) * 255).to(torch.uint8)


def checksums(sd):
    """key -> sum of the tensor's values times 1, 2, 3, ... in fp64 (order-sensitive), for every floating-point tensor."""
    return {k: float((v.double().flatten() * torch.arange(1, v.numel() + 1, dtype=torch.float64)).sum())
            for k, v in sorted(sd.items()) if v.is_floating_point()}


def main(ref_dir):
    sys.path.insert(0, ROOT)
    from unirestore_amd import segment
    _shim()
    ref = _load(ref_dir)
    sd = segment.random_state_dict(DEPTHS, WEIGHT_SEED, CLASSES)
    net = ref.ResNetLW(ref.Bottleneck, list(DEPTHS), num_classes=CLASSES)
    net.load_state_dict(sd, strict=True)
    net = net.double().eval()
    u8 = image()
    x = u8.double() / 255
    h, w = x.shape[2:]
    with torch.no_grad():
        logits = net(x)
        ups = []
        for s in SCALES:
            xs = F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=True)
            ups.append(F.interpolate(net(xs), size=(h, w), mode="bilinear", align_corners=True))
        pred = torch.stack(ups).mean(0).argmax(dim=1)
    sums = checksums(sd)
    np.savez_compressed(OUT, weight_seed=WEIGHT_SEED, image_seed=IMAGE_SEED, depths=np.array(DEPTHS), scales=np.array(SCALES),
                        image=u8.numpy(), checksum_keys=np.array(list(sums)),
                        checksums=np.array(list(sums.values()), dtype=np.float64), logits=logits.numpy(), pred=pred.to(torch.uint8).numpy())
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, logits {tuple(logits.shape)} |max| {float(logits.abs().max()):.2f}, "
          f"classes {sorted(set(pred.flatten().tolist()))}")


if __name__ == "__main__":
    main(sys.argv[1])
