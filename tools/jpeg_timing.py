"""Measured, not gated (profiles/jpeg_timing.txt): the JPEG round trip per 512 x 512 image on an MI355X (B = 8, HIP events around
`reps` back-to-back calls of jpeg.roundtrip after a warm-up, so the workspace allocation of a call is inside the figure) at quality
10 and 75 in both subsamplings, Pillow's save + open of the same eight images on one host core of the same box, and `validate` on
the same 64 clean PNGs through data.JpegImageFiles against data.ImageListFiles reading pairs that `cli jpeg` wrote beforehand
(full-size model, bf16, 20 steps, batch 8).  `python tools/jpeg_timing.py [--reps 20] [--no-validate]` prints the report; redirect
it into profiles/jpeg_timing.txt."""
import argparse, io, json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
os.environ.setdefault("OMP_NUM_THREADS", "1")
import numpy as np
import torch
from PIL import Image
from unirestore_amd import cli, imageio, jpeg

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-validate", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
torch.set_num_threads(1)
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
B, RES = 8, 512
g = torch.Generator().manual_seed(0)
# smooth content plus noise (what a photograph is closer to than uniform bytes: Pillow's entropy coder works on what survives)
yy, xx = np.mgrid[0:RES, 0:RES]
base = np.stack([128 + 100 * np.sin(0.02 * (i + 1) * xx + i) * np.cos(0.015 * (i + 2) * yy) for i in range(3)], -1)
x = torch.stack([torch.from_numpy(np.clip(np.roll(base, 37 * n, 1) + np.random.default_rng(n).normal(0, 6, base.shape), 0, 255).astype(np.uint8))
                 for n in range(B)])
xd = x.to(dev)
print(f"{torch.cuda.get_device_name(0)}; B = {B}, {RES} x {RES}; GPU: HIP events around {a.reps} calls of jpeg.roundtrip, ms per image; host: "
      "Pillow save(JPEG) + open + load of the same images, one core, best of 3 passes, ms per image")
for sub_name, sub in jpeg.SUBSAMPLINGS.items():
    for q in (10, 75):
        for _ in range(3):
            y = jpeg.roundtrip(xd, q, sub_name)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            jpeg.roundtrip(xd, q, sub_name)
        e1.record()
        torch.cuda.synchronize()
        gpu_ms = e0.elapsed_time(e1) / a.reps / B
        best, equal = float("inf"), True
        for _ in range(3):
            t0 = time.perf_counter()
            outs = []
            for n in range(B):
                buf = io.BytesIO()
                Image.fromarray(x[n].numpy()).save(buf, "JPEG", quality=q, subsampling=sub)
                buf.seek(0)
                outs.append(np.asarray(Image.open(buf).convert("RGB")))
            best = min(best, (time.perf_counter() - t0) * 1e3 / B)
        equal = bool(np.array_equal(np.stack(outs), y.cpu().numpy()))
        print(json.dumps(dict(quality=q, subsampling=sub_name, gpu_ms_per_image=round(gpu_ms, 4), pillow_ms_per_image=round(best, 2),
                              equal_to_pillow=equal)))
if not a.no_validate:
    import bench
    model = bench.build_model(20, dev, 0, 1, "bf16")
    tmp = tempfile.mkdtemp()
    src = os.path.join(tmp, "clean")
    os.makedirs(src)
    for i in range(64):
        imageio.save_u8(torch.from_numpy(np.ascontiguousarray(np.roll(x[i % B].numpy(), 11 * i, 0))), os.path.join(src, f"img_{i:03d}.png"))
    cli.jpeg_files(src, os.path.join(tmp, "lq"), "10", batch=8)
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_512_b8_20step_bf16.yaml"))
    runs = {"JpegImageFiles": dict(class_path="unirestore_amd.data.JpegImageFiles", init_args=dict(source=src, quality=[10], batch_size=8)),
            "ImageListFiles": dict(class_path="unirestore_amd.data.ImageListFiles",
                                   init_args=dict(list_file=os.path.join(tmp, "lq", "jpeg_q10", "pairs.txt"), batch_size=8))}
    print("validate, 64 PNGs of 512 x 512, JPEG quality 10, batch 8, bf16, 20 steps, full-size model, the two data classes alternating; "
          "images_per_s is the forward's (batches 2..8), wall_s the whole call (file reading, compression, metrics)")
    for rep in range(2):
        for label, data in runs.items():
            cfg["data"] = data
            t0 = time.perf_counter()
            res = cli.validate(cfg, model=model, metrics_device="gpu")
            print(f"{label} (pass {rep}):", json.dumps(dict(images=res["images"], images_per_s=res["images_per_s"], wall_s=round(time.perf_counter() - t0, 3),
                                                            psnr=res["val_lq/psnr"], ssim=res["val_lq/ssim"])))
    shutil.rmtree(tmp)
