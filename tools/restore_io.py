"""Measured, not gated (profiles/restore_io.txt): forward_u8 against forward(quantize=True) host to host at B = 8, 512 x 512, and a
folder of 64 PNGs through `cli restore` and one file at a time.  `python tools/restore_io.py` on an MI355X."""
import json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import bench
from unirestore_amd import cli, imageio

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
model = bench.build_model(20, dev, 0, 1, "bf16")
g = torch.Generator().manual_seed(0)
noise = (torch.randn(8, 4, 64, 64, generator=g), torch.randn(8, 4, 64, 64, generator=g))
noise = tuple(n.cuda() for n in noise)
u8 = [torch.randint(0, 256, (512, 512, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(8)]
f32 = (torch.stack(u8).permute(0, 3, 1, 2).float() / 255).contiguous().pin_memory()


def run_a():
    torch.cuda.synchronize(); t = time.perf_counter()
    y = model(f32, "ir", noise=noise, quantize=True).cpu()
    return (time.perf_counter() - t) * 1e3, y


def run_b():
    torch.cuda.synchronize(); t = time.perf_counter()
    y = [o.cpu() for o in model.forward_u8(u8, "ir", noise=noise)]
    return (time.perf_counter() - t) * 1e3, y


for _ in range(2):
    ya, yb = run_a()[1], run_b()[1]
same = torch.equal(ya.mul(255).round().to(torch.uint8).permute(0, 2, 3, 1), torch.stack(yb))
ta, tb = [], []
for _ in range(8):
    ta.append(run_a()[0]); tb.append(run_b()[0])
fmt = lambda v: f"mean {sum(v) / len(v):.2f} ms, min {min(v):.2f}, max {max(v):.2f} (n={len(v)})"
print("B=8 512x512 bf16 20 steps, full-size model, host to host, alternating, warmed")
print("  A forward(quantize=True) fp32 pinned host -> fp32 host :", fmt(ta))
print("  B forward_u8 uint8 pinned host -> uint8 host           :", fmt(tb))
print("  same 8-bit result:", same)

# ---- a folder of 64 PNGs: 12 sizes, 3 canvases
SIZES = [(512, 512), (256, 256), (128, 128), (384, 384), (512, 700), (256, 350), (384, 525), (512, 680),
         (300, 500), (480, 800), (500, 850), (512, 896)]
tmp = tempfile.mkdtemp()
src = os.path.join(tmp, "in"); os.makedirs(src)
for i in range(64):
    h, w = SIZES[i % len(SIZES)]
    imageio.save_u8(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8), os.path.join(src, f"img_{i:03d}.png"))
cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_512_b8_20step_bf16.yaml"))
model._graphs.clear()
res = cli.restore(cfg, src, os.path.join(tmp, "out"), batch=8, model=model)
print("restore --batch 8:", json.dumps(res))
plan = imageio.plan_batches([hw for _, hw in imageio.scan(imageio.list_inputs(src))], 8)
print("  plan:", [(b.canvas, len(b.members), b.valid) for b in plan])

model._graphs.clear()
c0 = model.graph_captures
os.makedirs(os.path.join(tmp, "one"))
torch.cuda.synchronize(); t0 = time.perf_counter()
for p in imageio.list_inputs(src):
    x = imageio.load_u8(p).permute(2, 0, 1)[None].float() / 255
    y = model(x, "ir", quantize=True)
    imageio.save_u8(y[0].mul(255).round().to(torch.uint8).permute(1, 2, 0), os.path.join(tmp, "one", os.path.basename(p)))
t1 = time.perf_counter() - t0
print(f"one file at a time through forward: 64 images in {t1:.2f} s = {64 / t1:.2f} images/s including {model.graph_captures - c0} graph captures")
torch.cuda.synchronize(); t0 = time.perf_counter()
for p in imageio.list_inputs(src):
    x = imageio.load_u8(p).permute(2, 0, 1)[None].float() / 255
    y = model(x, "ir", quantize=True)
    imageio.save_u8(y[0].mul(255).round().to(torch.uint8).permute(1, 2, 0), os.path.join(tmp, "one", os.path.basename(p)))
t2 = time.perf_counter() - t0
print(f"  second pass (UR_MAX_GRAPHS = 8 graphs kept, 12 shapes): {t2:.2f} s = {64 / t2:.2f} images/s, captures so far {model.graph_captures - c0}")
res2 = cli.restore(cfg, src, os.path.join(tmp, "out_b"), batch=8, model=model)
print("restore --batch 8, second run in the same process:", json.dumps(res2))
shutil.rmtree(tmp)
