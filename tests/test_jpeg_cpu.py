"""CPU-side checks of the JPEG round trip: the numpy restatement of the specification (jpeg_reference.py) against Pillow byte for
byte on every case of jpeg_cases.py, known answers of unirestore_amd.jpeg, every refusal of the C ABI and of `cli jpeg` (all before
any HIP call), the plan of data.JpegImageFiles, and that unirestore_amd.corrupt is what it was."""
import os

import numpy as np
import pytest

import jpeg_cases as cases
import jpeg_reference as ref
from unirestore_amd import jpeg


def _pillow_reads_jpeg():
    try:
        from PIL import features
        return bool(features.check("jpg"))
    except Exception:
        return False


@pytest.mark.skipif(not _pillow_reads_jpeg(), reason="this Pillow reports no JPEG support")
@pytest.mark.parametrize("subsampling", cases.SUBSAMPLINGS)
def test_restatement_equals_pillow_byte_for_byte(subsampling):
    """No case may be left out: the cap on mismatching (image, quality) pairs is zero."""
    wrong, pairs = [], 0
    for shape in cases.SHAPES:
        for kind in cases.KINDS:
            x = cases.images(shape, kind)
            for q in cases.QUALITIES:
                mine = ref.roundtrip(x, q, subsampling)
                for i in range(shape[0]):
                    pairs += 1
                    theirs = ref.pillow_roundtrip(x[i], q, subsampling)
                    if not np.array_equal(mine[i], theirs):
                        wrong.append((shape, kind, q, i, int((mine[i] != theirs).sum())))
    print(f"subsampling {subsampling}: {pairs} (image, quality) pairs, {len(wrong)} differ from Pillow")
    assert pairs == 9 * len(cases.KINDS) * len(cases.QUALITIES) and not wrong, wrong[:10]


def test_known_answers():
    assert jpeg.quant_tables(25)[0][0, 0] == 32 and jpeg.quant_tables(50)[0][0, 0] == 16 and jpeg.quant_tables(50)[1][0, 0] == 17
    lo = jpeg.quant_tables(7)
    assert lo[0].max() == 255 and lo[1].max() == 255 and (lo[1][4:] == 255).all() and lo[0][0, 0] == 114
    assert all((t == 1).all() for t in jpeg.quant_tables(100))
    assert jpeg.quant_tables(1)[0].min() == 255
    for q in cases.QUALITIES:
        for mine, theirs in zip(jpeg.quant_tables(q), ref.quant_tables(q)):
            assert mine.dtype == np.int32 and mine.shape == (8, 8) and np.array_equal(mine, theirs), q
    assert jpeg.SEVERITY_QUALITY == (25, 18, 15, 10, 7)
    assert [jpeg.quality_of(f"s{i}") for i in range(1, 6)] == [25, 18, 15, 10, 7] and jpeg.quality_of("s4") == 10
    assert jpeg.quality_of(1) == 1 and jpeg.quality_of(100) == 100 and jpeg.quality_of("75") == 75 and jpeg.quality_of(np.int64(30)) == 30
    for bad in (0, 101, -3, "0", "101", "s0", "s6", "ten", "", "2.5", 2.5, True, None):
        with pytest.raises(ValueError, match="quality"):
            jpeg.quality_of(bad)
    assert jpeg.subsampling_code("4:2:0") == 2 and jpeg.subsampling_code("4:4:4") == 0 and jpeg.subsampling_code(0) == 0
    for bad in ("4:2:2", 1, 3, None, True):
        with pytest.raises(ValueError, match="subsampling"):
            jpeg.subsampling_code(bad)
    import torch
    with pytest.raises(ValueError, match="16"):
        jpeg.roundtrip(torch.zeros(1, 15, 40, 3, dtype=torch.uint8), 50)
    with pytest.raises(ValueError, match="quality"):
        jpeg.roundtrip(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="uint8"):
        jpeg.roundtrip(torch.zeros(1, 16, 16, 3), 50)


def test_a_round_trip_is_not_a_copy():
    """A kernel that stored its input would pass every shape check: at quality 25 the smooth image changes in > 90 % of its bytes."""
    x = cases.images((2, 33, 47), "smooth")
    y = ref.roundtrip(x, 25)
    changed = float((y != x).mean())
    print(f"bytes changed at quality 25: {changed:.4f}")
    assert changed > 0.9 and np.abs(y.astype(int) - x).max() < 80
    assert float((ref.roundtrip(x, 100, 0) != x).mean()) < changed         # quality 100 without subsampling stays closest


def test_c_abi_refuses_wrong_arguments_before_the_gpu():
    from unirestore_amd import capi
    size = capi.lib.ur_jpeg_roundtrip_ws_bytes
    rows = cases.refusals(size)
    labels = [label for label, _ in rows]
    for must in ("null x", "null out", "null workspace", "N = 0", "H = 0", "W = 0", "H = 15", "W = 15", "quality = 0", "quality = 101",
                 "subsampling = 1", "subsampling = 3", "workspace one byte short"):
        assert must in labels, must
    for label, args in rows:
        assert capi.lib.ur_jpeg_roundtrip(*args) == capi.UR_E_INVALID, label
        assert b"ur_jpeg_roundtrip" in capi.lib.ur_last_error(), (label, capi.lib.ur_last_error())
    # the planes: Y padded to multiples of 8; chroma ceil(./2) padded to multiples of 8 (4:2:0) or like Y (4:4:4)
    assert size(2, 33, 47, 2) == 2 * (40 * 48 + 2 * 24 * 24) and size(2, 33, 47, 0) == 2 * 3 * 40 * 48
    assert size(1, 16, 16, 2) == 256 + 2 * 64 and size(3, 40, 32, 2) == 3 * (40 * 32 + 2 * 24 * 16)
    assert size(0, 16, 16, 2) == 0 and size(1, -1, 16, 2) == 0 and size(1, 16, 0, 0) == 0 and size(1, 16, 16, 1) == 0 and size(1, 16, 16, 3) == 0


def _png(path, shape=(32, 40), seed=0):
    from PIL import Image
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (*shape, 3), dtype=np.uint8)).save(path)


def test_cli_jpeg_argument_errors(tmp_path, capsys):
    from unirestore_amd import cli
    src = tmp_path / "clean"
    src.mkdir()
    _png(src / "a.png")
    _png(src / "b.png", seed=1)
    out = str(tmp_path / "out")
    paths, qualities, code = cli.check_jpeg_args(str(src), out, "10,25,s3,s4")
    assert [os.path.basename(p) for p in paths] == ["a.png", "b.png"] and qualities == [10, 25, 15] and code == 2      # s4 = 10: once
    assert cli.check_jpeg_args(str(src), out, "75", "4:4:4")[1:] == ([75], 0)
    for bad in ("0", "101", "s6", "ten", "", None, "10,,ten", ","):
        with pytest.raises(ValueError, match="--quality"):
            cli.check_jpeg_args(str(src), out, bad)
    for bad in ("4:2:2", "420", ""):
        with pytest.raises(ValueError, match="--subsampling"):
            cli.check_jpeg_args(str(src), out, "10", bad)
    with pytest.raises(ValueError, match="--batch"):
        cli.check_jpeg_args(str(src), out, "10", batch=0)
    with pytest.raises(FileNotFoundError, match="--input"):
        cli.check_jpeg_args(str(tmp_path / "nowhere"), out, "10")
    with pytest.raises(FileNotFoundError, match="--input"):
        cli.check_jpeg_args(None, out, "10")
    with pytest.raises(ValueError, match="--output"):
        cli.check_jpeg_args(str(src), None, "10")
    with pytest.raises(ValueError, match="--output"):
        cli.check_jpeg_args(str(src), str(src), "10")
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no image"):
        cli.check_jpeg_args(str(empty), out, "10")
    lst = tmp_path / "pairs.txt"                     # an `lq hq label` list: only the hq column is read
    lst.write_text("lq/a.png clean/a.png 0\nlq/b.png clean/b.png 1\n")
    assert cli.check_jpeg_args(str(lst), out, "s1")[:2] == ([str(src / "a.png"), str(src / "b.png")], [25])
    lst.write_text("x/a.png clean/a.png\ny/a.png clean/a.png\n")
    with pytest.raises(ValueError, match="stem"):
        cli.check_jpeg_args(str(lst), out, "10")
    lst.write_text("clean/a.png\nclean/missing.png\n")
    with pytest.raises(FileNotFoundError, match="missing"):
        cli.check_jpeg_args(str(lst), out, "10")
    # `jpeg` needs no --config and refuses a wrong call before it looks for a GPU
    for argv in (["jpeg", "--input", str(src), "--output", out], ["jpeg", "--input", str(src), "--output", out, "--quality", "s9"],
                 ["jpeg", "--input", str(tmp_path / "nowhere"), "--output", out, "--quality", "10"],
                 ["jpeg", "--input", str(src), "--output", out, "--quality", "10", "--subsampling", "4:1:1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    err = capsys.readouterr().err
    assert "arguments are required: --config" not in err and "--quality" in err and "--subsampling" in err and "--input" in err


def test_jpeg_image_files_plans_without_a_gpu(tmp_path):
    from unirestore_amd import cli, data
    src = tmp_path / "clean"
    src.mkdir()
    for i in range(7):
        _png(src / f"im{i}.png", shape=(32, 40) if i % 3 else (36, 32), seed=i)
    d = data.JpegImageFiles(str(src), quality=(10, "s1", 50, "25"), batch_size=2)
    assert d.qualities == [10, 25, 50] and len(d) == len(d._plan())
    plan = d._plan()
    assert sorted((i, q) for q, idx in plan for i in idx) == sorted((i, q) for i in range(7) for q in (10, 25, 50))      # each pair once
    from unirestore_amd import imageio
    sizes = [hw for _, hw in imageio.scan(d.paths)]
    assert all(1 <= len(idx) <= 2 and len({sizes[i] for i in idx}) == 1 for _, idx in plan)                           # homogeneous
    assert data.JpegImageFiles(str(src)).qualities == [10, 25, 50] and data.JpegImageFiles(str(src), quality="s5,90").qualities == [7, 90]
    assert data.JpegImageFiles(str(src), quality=30).qualities == [30]
    assert len(data.JpegImageFiles(str(src), batch_size=2, num_batches=3)) == 3
    with pytest.raises(ValueError, match="shard"):
        next(d.batches(0, 2))
    with pytest.raises(ValueError, match="quality"):
        data.JpegImageFiles(str(src), quality=(10, 0))
    with pytest.raises(ValueError, match="quality"):
        data.JpegImageFiles(str(src), quality=())
    with pytest.raises(ValueError, match="batch_size"):
        data.JpegImageFiles(str(src), batch_size=0)
    with pytest.raises(ValueError, match="no image"):
        (tmp_path / "empty").mkdir()
        data.JpegImageFiles(str(tmp_path / "empty"))
    assert cli.DATA_CLASSES["unirestore_amd.data.JpegImageFiles"].endswith("JpegImageFiles")
    cfg = dict(model=dict(class_path="unirestore_amd.runner.LitUniFIE", init_args=dict(model_kwargs=dict(cnet=dict(num_inference_steps=1)))),
               data=dict(class_path="unirestore_amd.data.JpegImageFiles", init_args=dict(source=str(src), quality=[10, 50])))
    assert cli.resolve(cfg)["data_class"].endswith("JpegImageFiles")


def test_corrupt_module_is_what_it_was():
    from unirestore_amd import corrupt as cr
    assert cr.UNBUILT == ("glass_blur", "snow", "frost", "spatter", "elastic_transform", "jpeg_compression")
    assert len(cr.NAMES) == 13 and "jpeg_compression" not in cr.NAMES and cr.skipped("digital")[-1] == "jpeg_compression"
    with pytest.raises(NotImplementedError, match="jpeg_compression") as e:
        cr.corrupt(None, "jpeg_compression", 3, 42)
    assert "cli jpeg" in str(e.value) and "jpeg.roundtrip" in str(e.value)
    with pytest.raises(NotImplementedError, match="snow") as e:
        cr.expand("snow")
    assert "jpeg" not in str(e.value).replace("jpeg_compression", "")
