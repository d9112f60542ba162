"""Generate tests/golden/rvt_0.npz by running the reference's own RVT (`PoolingTransformer` of src/modules/rvt/robust_models.py) in
fp64.

    python tools/gen_golden_rvt.py <reference>/src/modules/rvt/robust_models.py

Runs ONLY where the reference checkout is at hand.  The reference Python never travels: only the produced vectors are committed.
The module is loaded by path under stand-in `timm.data`, `timm.models.layers`, `timm.models.registry` and
`timm.models.vision_transformer` modules (timm is not installed; the module takes from it two constants it never uses, DropPath -
an identity at drop_path = 0 and in eval mode -, trunc_normal_, the register_model decorator and _cfg); einops is installed.  The
two networks are the GOLDEN_CASES of tests/rvt_reference.py - a two-stage one with head dimension 32, the convolutional MLP, a
gated and a plain block at 196 tokens, the head pooling and 49 tokens, and a 768-wide one with head dimension 64 and the Linear
MLP - each with rvt.random_state_dict loaded with strict=True, so every key and shape of the stand-in layout is the reference
module's.  The fixture holds, per network, the configuration, the seeds, one order-sensitive fp64 checksum per weight tensor (to
tell a drift of the random generator from a wrong restatement), the checksum of the seeded input and the module's logits - nothing
else.
"""
import importlib.util
import os
import sys
import time
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden", "rvt_0.npz")


def _load(path):
    """robust_models.py as a module, under stand-ins for the four timm modules it imports from."""
    def register_model(fn):
        return fn
    stubs = {"timm": {}, "timm.data": dict(IMAGENET_DEFAULT_MEAN=(0.485, 0.456, 0.406), IMAGENET_DEFAULT_STD=(0.229, 0.224, 0.225)),
             "timm.models": {}, "timm.models.layers": dict(DropPath=lambda *a, **k: nn.Identity(), trunc_normal_=nn.init.trunc_normal_),
             "timm.models.registry": dict(register_model=register_model), "timm.models.vision_transformer": dict(_cfg=lambda **k: {})}
    for name, attrs in stubs.items():
        mod = types.ModuleType(name)
        mod.__path__ = []
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("ref_robust_models", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import rvt_reference as R
    from unirestore_amd import rvt
    ref = _load(path)
    out = {"cases": np.array(R.GOLDEN_CASES)}
    for name in R.GOLDEN_CASES:
        spec, classes, wseed, iseed, n = R.NET_CASES[name]
        size, base_dims, depth, heads, mlp_ratio, use_mask, masked_block = spec
        sd = rvt.random_state_dict(rvt.RVTConfig(*spec), wseed, classes)
        net = ref.PoolingTransformer(image_size=size, patch_size=16, stride=16, base_dims=list(base_dims), depth=list(depth), heads=list(heads),
                                     mlp_ratio=mlp_ratio, num_classes=classes, use_mask=use_mask, masked_block=masked_block)
        net.load_state_dict(sd, strict=True)
        net = net.double().eval()
        x = R.net_input(name)
        t0 = time.time()
        with torch.no_grad():
            logits = net(x.double())
        dt = time.time() - t0
        assert tuple(logits.shape) == (n, classes)
        sums = {k: R.checksum(v) for k, v in sorted(sd.items()) if v.is_floating_point()}
        out.update({f"{name}/image_size": size, f"{name}/base_dims": np.array(base_dims), f"{name}/depth": np.array(depth),
                    f"{name}/heads": np.array(heads), f"{name}/mlp_ratio": mlp_ratio, f"{name}/use_mask": use_mask,
                    f"{name}/masked_block": masked_block, f"{name}/classes": classes, f"{name}/weight_seed": wseed,
                    f"{name}/image_seed": iseed, f"{name}/n": n, f"{name}/checksum_keys": np.array(list(sums)),
                    f"{name}/checksums": np.array(list(sums.values()), dtype=np.float64), f"{name}/input_checksum": R.checksum(x),
                    f"{name}/logits": logits.numpy()})
        print(f"{name}: {len(sums)} tensors, {dt:.2f} s, logits {tuple(logits.shape)} |max| {float(logits.abs().max()):.2f}, "
              f"classes {logits.argmax(dim=1).tolist()}")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
