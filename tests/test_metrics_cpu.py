"""GPU metric kernels, host side: the C ABI exports, argument validation before any HIP call (null / dummy pointers are
never dereferenced), the workspace size, and LitUniFIE's `metrics_device` switch."""
import ctypes

import pytest

from unirestore_amd import capi

DUMMY = 0x1000        # never dereferenced: every check below fails before the library touches the GPU


def _lib():
    from unirestore_amd import build
    return ctypes.CDLL(build.build(verbose=False))


def test_library_exports_the_metric_entry_points():
    lib = _lib()
    assert hasattr(lib, "ur_image_metrics")
    assert hasattr(lib, "ur_image_metrics_ws_size")
    assert "ur_image_metrics" in capi.SIGNATURES and "ur_image_metrics_ws_size" in capi.SIGNATURES


def _call(pred=DUMMY, target=DUMMY, N=2, C=3, H=32, W=40, win=7, data_range=1.0, psnr=DUMMY, ssim=DUMMY, ws=DUMMY,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 20
    return capi.lib.ur_image_metrics(pred, target, N, C, H, W, win, data_range, psnr, ssim, ws, ws_bytes, None)


INVALID = [
    (dict(N=0), "N and C"), (dict(C=0), "N and C"), (dict(N=-1), "N and C"),
    (dict(H=6), "H and W"), (dict(W=6), "H and W"), (dict(H=10, W=10, win=11), "H and W"),
    (dict(win=8), "win"), (dict(win=1), "win"), (dict(win=2), "win"), (dict(win=-3), "win"),
    (dict(data_range=0.0), "data_range"), (dict(data_range=-1.0), "data_range"), (dict(data_range=float("nan")), "data_range"),
    (dict(ws_bytes=0), "workspace"), (dict(ws_bytes=8), "workspace"),
    (dict(pred=None), "null"), (dict(target=None), "null"), (dict(psnr=None), "null"), (dict(ssim=None), "null"),
    (dict(ws=None), "null"),
]


@pytest.mark.parametrize("kw,word", INVALID, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in INVALID])
def test_invalid_arguments_are_rejected_before_any_hip_call(kw, word):
    assert _call(**kw) == capi.UR_E_INVALID
    msg = capi.lib.ur_last_error().decode()
    assert "ur_image_metrics" in msg and word in msg, msg


def test_workspace_one_byte_short_is_rejected():
    need = capi.lib.ur_image_metrics_ws_size(2, 3, 67, 91, 7)
    assert _call(H=67, W=91, ws_bytes=need - 1) == capi.UR_E_INVALID
    assert "workspace too small" in capi.lib.ur_last_error().decode()


def test_workspace_size():
    ws = capi.lib.ur_image_metrics_ws_size
    smallest = ws(1, 1, 7, 7, 7)
    assert smallest > 0 and smallest % 8 == 0
    base = ws(1, 1, 64, 64, 7)
    assert ws(2, 1, 64, 64, 7) == 2 * base and ws(1, 3, 64, 64, 7) == 3 * base and ws(4, 3, 64, 64, 7) == 12 * base
    assert ws(1, 1, 512, 512, 7) > ws(1, 1, 256, 256, 7) > base                     # more tiles, more partials
    assert ws(1, 1, 64, 512, 7) > ws(1, 1, 64, 64, 7) and ws(1, 1, 512, 64, 7) > ws(1, 1, 64, 64, 7)
    for bad in ((0, 1, 7, 7, 7), (1, 0, 7, 7, 7), (1, 1, 6, 7, 7), (1, 1, 7, 7, 4), (1, 1, 7, 7, 1)):
        assert ws(*bad) == capi.UR_E_INVALID
        assert "ur_image_metrics_ws_size" in capi.lib.ur_last_error().decode()


class _StubModel:
    pass


def test_litunifie_metrics_device_switch():
    from unirestore_amd.runner import LitUniFIE
    assert LitUniFIE({}, model=_StubModel()).metrics_device == "cpu"
    assert LitUniFIE({}, model=_StubModel(), metrics_device="gpu").metrics_device == "gpu"
    for bad in ("cuda", "GPU", "", None):
        with pytest.raises(ValueError, match="metrics_device"):
            LitUniFIE({}, model=_StubModel(), metrics_device=bad)


def test_litunifie_metrics_of_an_empty_run():
    from unirestore_amd.runner import LitUniFIE
    for dev in ("cpu", "gpu"):
        assert LitUniFIE({}, model=_StubModel(), metrics_device=dev).metrics() == {"val_lq/psnr": 0.0, "val_lq/ssim": 0.0, "images": 0}


def test_cli_metrics_device_flag():
    import inspect

    from unirestore_amd import cli
    assert inspect.signature(cli.validate).parameters["metrics_device"].default == "cpu"
    with pytest.raises(SystemExit):
        cli.main(["validate", "--config", "configs/val_pir_256_4step.yaml", "--metrics-device", "tpu"])
