"""The JPEG kernels (csrc/jpeg.hip) against the numpy restatement of jpeg_reference.py, byte for byte, and the layers above them
(ops.jpeg_roundtrip, jpeg.roundtrip, data.JpegImageFiles, cli.validate, cli jpeg).  The cases are jpeg_cases.py; test_jpeg_cpu.py
holds the restatement against Pillow.  Every launch goes through the C ABI on guarded buffers: guards and the input untouched, and a
second launch into a dirtied output and a dirtied workspace bit-identical (nothing in the workspace is read before it is written).
The quantisation tables travel by value in the launch, so there is no device table to guard."""
import json
import os

import numpy as np
import pytest
import torch

import jpeg_cases as cases
import jpeg_reference as ref
from test_boundary_launchers_gpu import Buf

pytestmark = pytest.mark.gpu

_REF = {}                       # (shape, kind, quality, subsampling) -> the restatement's bytes: computed once, shared, read-only


@pytest.fixture(scope="module")
def capi():
    from unirestore_amd import capi as c
    return c


def _stream():
    return torch.cuda.current_stream().cuda_stream


def reference(shape, kind, q, sub):
    key = (shape, kind, q, sub)
    if key not in _REF:
        _REF[key] = ref.roundtrip(cases.images(shape, kind), q, sub)
        _REF[key].setflags(write=False)
    return _REF[key]


def launch(capi, x, q, sub, dirt=None, stream=None):
    """ur_jpeg_roundtrip of the host u8 batch x on guarded buffers; dirt: a byte to fill the output and the workspace with first.
    -> (out on the host, the input untouched and all guards intact)."""
    n, h, w, _ = x.shape
    xb = Buf(tuple(x.shape), torch.uint8, fill=x.cuda())
    out = Buf(tuple(x.shape), torch.uint8)
    nbytes = capi.lib.ur_jpeg_roundtrip_ws_bytes(n, h, w, sub)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = Buf((nbytes,), torch.uint8)                 # (64 guard bytes in front: still 8-byte aligned)
    if dirt is not None:
        out.t.fill_(dirt)
        ws.t.fill_(dirt)
    torch.cuda.synchronize()
    rc = capi.lib.ur_jpeg_roundtrip(xb.ptr, out.ptr, n, h, w, q, sub, ws.ptr, nbytes, _stream() if stream is None else stream)
    assert rc == 0, (x.shape, q, sub, capi.lib.ur_last_error())
    torch.cuda.synchronize()
    ok = xb.guards_ok() and out.guards_ok() and ws.guards_ok() and torch.equal(xb.t.cpu(), x)
    return out.t.cpu(), ok


@pytest.mark.parametrize("shape", cases.SHAPES)
@pytest.mark.parametrize("subsampling", cases.SUBSAMPLINGS)
def test_equals_the_restatement_in_every_byte(capi, subsampling, shape):
    for kind in cases.KINDS:
        x = torch.from_numpy(cases.images(shape, kind))
        for q in cases.QUALITIES:
            what = (shape, kind, q, subsampling)
            got, ok = launch(capi, x, q, subsampling)
            again, ok2 = launch(capi, x, q, subsampling, dirt=0x3C + q)
            assert ok and ok2, what
            want = reference(shape, kind, q, subsampling)
            wrong = int((got.numpy() != want).sum())
            assert wrong == 0, (what, wrong, int(np.abs(got.numpy().astype(int) - want).max()))
            assert torch.equal(got, again), what


def test_an_image_alone_equals_itself_in_a_batch(capi):
    from unirestore_amd import jpeg
    x = torch.from_numpy(cases.images((3, 40, 32), "smooth"))
    for sub in cases.SUBSAMPLINGS:
        for q in (10, 75):
            batch, ok = launch(capi, x, q, sub)
            alone, ok2 = launch(capi, x[2:3].contiguous(), q, sub)
            assert ok and ok2 and torch.equal(batch[2:3], alone) and not torch.equal(batch[0], batch[2]), (sub, q)
            assert float((batch != x).float().mean()) > 0.5, (sub, q)              # not a copy of the input
    dev = x.cuda()
    assert torch.equal(jpeg.roundtrip(dev, "s4")[2:3], jpeg.roundtrip(dev[2:3].contiguous(), 10))


def test_wrapper_planner_and_stream_equal_the_raw_call(capi):
    from unirestore_amd import jpeg, ops
    x = torch.from_numpy(cases.images((2, 33, 47), "random"))
    dev = x.cuda()
    side = torch.cuda.Stream()
    for name, sub in (("4:2:0", 2), ("4:4:4", 0)):
        for q in (7, 50, 95):
            raw, ok = launch(capi, x, q, sub)
            assert ok
            got = ops.jpeg_roundtrip(dev, q, sub)
            assert got.dtype == torch.uint8 and got.shape == dev.shape and got.is_contiguous() and torch.equal(got.cpu(), raw), (name, q)
            into = torch.full_like(dev, 9)
            assert ops.jpeg_roundtrip(dev, q, sub, out=into) is into and torch.equal(into.cpu(), raw), (name, q)
            assert torch.equal(jpeg.roundtrip(dev, q, name).cpu(), raw) and torch.equal(jpeg.roundtrip(dev, str(q), sub).cpu(), raw), (name, q)
            with torch.cuda.stream(side):            # the wrapper launches on the current stream
                on_side = jpeg.roundtrip(dev, q, name)
            side.synchronize()
            assert torch.equal(on_side.cpu(), raw), (name, q)
            by_hand, ok = launch(capi, x, q, sub, stream=side.cuda_stream)
            assert ok and torch.equal(by_hand, raw), (name, q)
    assert torch.equal(jpeg.roundtrip(dev, "s1").cpu(), launch(capi, x, 25, 2)[0])          # 4:2:0 is the default
    with pytest.raises(ValueError, match="16"):
        jpeg.roundtrip(torch.zeros(1, 40, 15, 3, dtype=torch.uint8, device="cuda"), 50)
    with pytest.raises(ValueError, match="out"):
        ops.jpeg_roundtrip(dev, 50, out=torch.zeros(2, 33, 47, 3, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        ops.jpeg_roundtrip(dev, 50, out=dev)
    with pytest.raises(ValueError, match="subsampling"):
        ops.jpeg_roundtrip(dev, 50, 1)


SIZES = [("a0", (40, 32)), ("a1", (33, 47)), ("b0", (40, 32)), ("a2", (33, 47)), ("a3", (40, 32)), ("b1", (64, 96)), ("a4", (40, 32))]


def _folder(path, entries=SIZES):
    from unirestore_amd import imageio
    path.mkdir()
    for stem, hw in entries:
        x = cases.images((1, *hw), "smooth" if sum(map(ord, stem)) % 2 else "random")[0]
        x = np.roll(x, sum(map(ord, stem)), axis=1)                               # files of one size differ
        imageio.save_u8(torch.from_numpy(np.ascontiguousarray(x)), str(path / f"{stem}.png"))
    return path


def test_jpeg_image_files(tmp_path):
    from unirestore_amd import data, imageio, jpeg
    src = _folder(tmp_path / "clean")
    d = data.JpegImageFiles(str(src), quality=(10, "s1"), batch_size=2)
    seen = []
    for lq, hq, gt, names, task in d.batches(device="cuda"):
        kind, q = d.last
        assert kind == "jpeg" and q in (10, 25) and gt is None and task == "ir" and len(names) <= 2
        assert lq.shape == hq.shape and lq.dtype == torch.float32 and lq.shape[1] == 3 and hq.is_cuda and lq.is_contiguous()
        u8 = torch.stack([imageio.load_u8(str(src / f"{st}.png")) for st in names])
        assert torch.equal(hq.cpu(), u8.permute(0, 3, 1, 2).float().div(255))            # the values ImageListFiles yields
        assert torch.equal(lq.cpu(), jpeg.roundtrip(u8.cuda(), q).cpu().permute(0, 3, 1, 2).float().div(255))
        assert all(dict(SIZES)[st] == tuple(hq.shape[2:]) for st in names)
        seen += [(st, q) for st in names]
    assert sorted(seen) == sorted((st, q) for st, _ in SIZES for q in (10, 25))
    lst = tmp_path / "list.txt"                      # an `lq hq label` list: the hq column
    lst.write_text("".join(f"nowhere/{st}.png clean/{st}.png 0\n" for st, _ in SIZES[:3]))
    d2 = data.JpegImageFiles(str(lst), quality=75, batch_size=8)
    got = list(d2.batches(device="cuda"))
    assert sorted(n for b in got for n in b[3]) == ["a0", "a1", "b0"] and d2.last == ("jpeg", 75)


def test_validate_reports_by_quality(tmp_path):
    from restore_worker import tiny_cfg, tiny_model
    from unirestore_amd import cli
    src = _folder(tmp_path / "clean", [(f"v{i}", (64, 64)) for i in range(3)])
    cfg = tiny_cfg()
    cfg["data"] = dict(class_path="unirestore_amd.data.JpegImageFiles", init_args=dict(source=str(src), quality=[10, 50], batch_size=2))
    res = cli.validate(cfg, model=tiny_model())
    print("validate:", json.dumps(res))
    by = res["by_corruption"]
    assert sorted(by) == ["jpeg/10", "jpeg/50"] and by["jpeg/10"]["images"] == by["jpeg/50"]["images"] == 3
    assert res["images"] == 6 == sum(v["images"] for v in by.values()) and res["output_finite"] and "skipped" not in res
    assert abs(sum(v["psnr"] * v["images"] for v in by.values()) / 6 - res["val_lq/psnr"]) < 1e-9
    assert abs(sum(v["ssim"] * v["images"] for v in by.values()) / 6 - res["val_lq/ssim"]) < 1e-9
    json.dumps(res)


def _read(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def test_cli_jpeg_writes_files_that_depend_on_the_file_alone(tmp_path, capsys):
    from unirestore_amd import cli, data, imageio
    entries = [("X", (40, 32)), ("Y", (40, 32)), ("Z", (33, 47))]
    xy = _folder(tmp_path / "xy", entries[:2])
    xyz = _folder(tmp_path / "xyz", entries)
    yx = tmp_path / "yx.txt"
    yx.write_text("xy/Y.png\nxy/X.png\n")
    res = cli.jpeg_files(str(xy), str(tmp_path / "o1"), "10,s1,s4", batch=2)
    cli.jpeg_files(str(yx), str(tmp_path / "o2"), "10,25", batch=1)
    cli.jpeg_files(str(xyz), str(tmp_path / "o3"), "25,10", batch=3)
    assert res["images"] == 2 and res["qualities"] == [10, 25] and res["subsampling"] == "4:2:0"
    assert sorted(os.listdir(tmp_path / "o1")) == sorted(res["folders"]) == ["jpeg_q10", "jpeg_q25"]
    clean = imageio.load_u8(str(xy / "X.png")).numpy()
    for q in (10, 25):
        f = f"jpeg_q{q}"
        a, b, c = _read(tmp_path / "o1" / f), _read(tmp_path / "o2" / f), _read(tmp_path / "o3" / f)
        assert sorted(a) == ["X.png", "Y.png", "pairs.txt"] and a["X.png"] == b["X.png"] == c["X.png"] and a["Y.png"] == c["Y.png"]
        # the PNG holds exactly what Pillow's own JPEG round trip of X gives
        assert np.array_equal(imageio.load_u8(str(tmp_path / "o1" / f / "X.png")).numpy(), ref.pillow_roundtrip(clean, q)), q
        pairs = data.ImageListFiles(str(tmp_path / "o1" / f / "pairs.txt"), batch_size=4)
        for lq, hq, _, names, _ in pairs.batches(device="cuda"):
            assert lq.shape == hq.shape and not torch.equal(lq, hq) and sorted(names) == ["X", "Y"]
    assert cli.main(["jpeg", "--input", str(xy), "--output", str(tmp_path / "o4"), "--quality", "s3", "--subsampling", "4:4:4", "--batch", "1"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["folders"] == ["jpeg_q15"] and line["subsampling"] == "4:4:4"
    assert np.array_equal(imageio.load_u8(str(tmp_path / "o4" / "jpeg_q15" / "X.png")).numpy(), ref.pillow_roundtrip(clean, 15, 0))
