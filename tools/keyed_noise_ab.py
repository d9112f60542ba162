"""Measured, not gated (profiles/keyed_noise_ab.txt): `cli restore --noise image` (both draws generated on the device inside the graph)
against `--noise batch` (one host draw per batch, copied into the graph's inputs - the only path before --noise existed): 64 PNGs
of 512 x 512, --batch 8, full-size model, bf16, 20 steps, one process, the two modes alternating.  `python tools/keyed_noise_ab.py`
on an MI355X."""
import json, os, shutil, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import bench
from unirestore_amd import cli, imageio

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
model = bench.build_model(20, dev, 0, 1, "bf16")
g = torch.Generator().manual_seed(0)
tmp = tempfile.mkdtemp()
src = os.path.join(tmp, "in"); os.makedirs(src)
for i in range(64):
    imageio.save_u8(torch.randint(0, 256, (512, 512, 3), generator=g, dtype=torch.uint8), os.path.join(src, f"img_{i:03d}.png"))
cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_512_b8_20step_bf16.yaml"))
cli.restore(cfg, src, os.path.join(tmp, "warm"), batch=8, model=model)             # warm: weights packed, files in the page cache
print("64 PNGs of 512x512, --batch 8, bf16, 20 steps, full-size model; images_per_s is over the 56 images of the 7 batches that replay")
for rep in range(3):
    for mode in ("batch", "image"):
        res = cli.restore(cfg, src, os.path.join(tmp, f"{mode}{rep}"), batch=8, model=model, noise=mode)
        print(f"restore --noise {mode} (pass {rep}):", json.dumps({k: res[k] for k in ("noise", "images", "images_timed", "images_per_s",
                                                                                      "seconds_total", "graphs_captured", "output_finite")}))
shutil.rmtree(tmp)
