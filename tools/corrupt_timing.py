"""Measured, not gated (profiles/corrupt_timing.txt): the corruption kernels per 512 x 512 image on an MI355X (B = 8, HIP events around
`reps` back-to-back calls of corrupt.corrupt after a warm-up, so the host-side table building and uploads of a call are inside the
figure), the numpy fp64 reference of tests/corrupt_reference.py on one host core (one image, one run), and `validate` on the same 64
clean PNGs through data.CorruptedImageFiles against data.ImageListFiles reading pairs that `cli corrupt` wrote beforehand (full-size
model, bf16, 20 steps, batch 8).  `python tools/corrupt_timing.py [--reps 20] [--no-validate]` prints the report; redirect it into
profiles/corrupt_timing.txt."""
import argparse, json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("OMP_NUM_THREADS", "1")
import numpy as np
import torch
import corrupt_reference as ref
from unirestore_amd import cli, corrupt, imageio

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
x = torch.randint(0, 256, (B, RES, RES, 3), generator=g, dtype=torch.uint8)
xd, stems = x.to(dev), [f"img_{i:03d}" for i in range(B)]
print(f"{torch.cuda.get_device_name(0)}; B = {B}, {RES} x {RES}; GPU: HIP events around {a.reps} calls of corrupt.corrupt (tables built and "
      "uploaded per call), ms per image; host: the numpy fp64 reference, one image, one core, one run, ms")
for name in corrupt.NAMES:
    for sev in (3, 5):
        for _ in range(3):
            corrupt.corrupt(xd, name, sev, 42, stems)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            corrupt.corrupt(xd, name, sev, 42, stems)
        e1.record()
        torch.cuda.synchronize()
        gpu_ms = e0.elapsed_time(e1) / a.reps / B
        t0 = time.perf_counter()
        ref.run(name, x[0].numpy(), sev, key=corrupt.corruption_seed(42, stems[0]), angle=corrupt.motion_angle(42, stems[0]),
                table=corrupt.poisson_table(ref.C["shot_noise"][sev - 1]))
        host_ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(corruption=name, severity=sev, gpu_ms_per_image=round(gpu_ms, 4), host_ms_per_image=round(host_ms, 1))))
if not a.no_validate:
    import bench
    model = bench.build_model(20, dev, 0, 1, "bf16")
    tmp = tempfile.mkdtemp()
    src = os.path.join(tmp, "clean")
    os.makedirs(src)
    for i in range(64):
        imageio.save_u8(torch.randint(0, 256, (RES, RES, 3), generator=g, dtype=torch.uint8), os.path.join(src, f"img_{i:03d}.png"))
    cli.corrupt_files(src, os.path.join(tmp, "lq"), "fog", 3, seed=42, batch=8)
    cfg = cli.load_config(os.path.join(ROOT, "configs", "val_pir_512_b8_20step_bf16.yaml"))
    runs = {"CorruptedImageFiles": dict(class_path="unirestore_amd.data.CorruptedImageFiles",
                                        init_args=dict(source=src, corruptions="fog", severity=3, batch_size=8, seed=42)),
            "ImageListFiles": dict(class_path="unirestore_amd.data.ImageListFiles",
                                   init_args=dict(list_file=os.path.join(tmp, "lq", "fog_3", "pairs.txt"), batch_size=8))}
    print("validate, 64 PNGs of 512 x 512, fog / 3, batch 8, bf16, 20 steps, full-size model, the two data classes alternating; images_per_s "
          "is the forward's (batches 2..8), wall_s the whole call (file reading, corruption, metrics)")
    for rep in range(2):
        for label, data in runs.items():
            cfg["data"] = data
            t0 = time.perf_counter()
            res = cli.validate(cfg, model=model, metrics_device="gpu")
            print(f"{label} (pass {rep}):", json.dumps(dict(images=res["images"], images_per_s=res["images_per_s"], wall_s=round(time.perf_counter() - t0, 3),
                                                            psnr=res["val_lq/psnr"], ssim=res["val_lq/ssim"])))
    shutil.rmtree(tmp)
