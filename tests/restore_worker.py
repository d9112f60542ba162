"""`cli restore` on the tiny model, for a launch through `python -m torch.distributed.run` (tests/test_restore_gpu.py):
restore_worker.py INPUT OUTPUT BATCH -> the command's JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def tiny_cfg():
    from tiny_cfg import model_kwargs
    return dict(seed_everything=7, trainer=dict(precision="bf16-mixed"),
                model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=model_kwargs(2))))


def tiny_model(seed=3):
    import torch
    from tiny_cfg import TINY, model_kwargs, randomise_
    import unirestore_amd.modules as M
    torch.manual_seed(seed)
    return randomise_(M.DiffUIE(**model_kwargs(2), **TINY).eval(), seed)


if __name__ == "__main__":
    from unirestore_amd import cli
    res = cli.restore(tiny_cfg(), sys.argv[1], sys.argv[2], batch=int(sys.argv[3]), model=tiny_model())
    if res is not None:
        print(json.dumps(res))
