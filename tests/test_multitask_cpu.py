"""Host side of DiffUIE.forward_tasks: the task-chunk rule and the C ABI of the two fan-out kernels (no GPU needed)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1 << 31          # ur_conv2d_nhwc refuses N*H*W*ld >= 2^31 elements (csrc/igemm.hip)


def _elems(n, n_images, h, w, c):
    return n * n_images * h * w * c


def _check_cover(chunks, n_tasks):
    assert [f for f, _ in chunks] == [sum(n for _, n in chunks[:i]) for i in range(len(chunks))]      # consecutive, from 0
    assert sum(n for _, n in chunks) == n_tasks and all(n >= 1 for _, n in chunks)


def test_task_chunks_named_cases():
    from unirestore_amd.tiling import task_chunks
    assert task_chunks(8, 3, 512, 512, 256) == [(0, 3)]                       # the reference's three tasks at B = 8: 24 images fit
    assert task_chunks(8, 4, 512, 512, 256) == [(0, 2), (2, 2)]               # 32 images do not: two chunks of two
    assert task_chunks(1, 3, 1024, 1024, 256) == [(0, 3)]
    seven = task_chunks(8, 7, 512, 512, 256)
    _check_cover(seven, 7)
    sizes = [n for _, n in seven]
    assert max(sizes) - min(sizes) <= 1
    assert all(_elems(n, 8, 512, 512, 256) < LIMIT for n in sizes)


@pytest.mark.parametrize("n_images", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("n_tasks", [1, 2, 3, 4, 5, 7, 8, 13])
@pytest.mark.parametrize("hw,c", [((512, 512), 256), ((1024, 1024), 256), ((640, 512), 128), ((64, 128), 64), ((2048, 2048), 256)])
def test_task_chunks_properties(n_images, n_tasks, hw, c):
    """Every chunk satisfies the < 2^31 inequality (where a single task can), the chunks cover 0..K-1 once in order, differ by at
    most one task, and are the fewest: merging any two neighbours breaks the bound, or the list has length 1."""
    from unirestore_amd.tiling import task_chunks
    chunks = task_chunks(n_images, n_tasks, hw[0], hw[1], c)
    _check_cover(chunks, n_tasks)
    sizes = [n for _, n in chunks]
    assert max(sizes) - min(sizes) <= 1
    if _elems(1, n_images, *hw, c) >= LIMIT:                # a single task does not fit: one task per chunk, the launcher refuses it
        assert sizes == [1] * n_tasks
        return
    assert all(_elems(n, n_images, *hw, c) < LIMIT for n in sizes)
    assert len(chunks) == 1 or all(_elems(a + b, n_images, *hw, c) >= LIMIT for a, b in zip(sizes, sizes[1:]))


def test_task_chunks_rejects_empty_sizes():
    from unirestore_amd.tiling import task_chunks
    with pytest.raises(ValueError):
        task_chunks(8, 0, 512, 512, 256)


def test_fanout_exports_are_declared_bound_and_exported():
    """The two new kernels go through the C ABI like every other: declared in the header, listed in capi.SIGNATURES (the
    existing symbol test compares the two lists and loads the library), and exported by the built library."""
    import ctypes
    from unirestore_amd import build, capi
    src = open(os.path.join(ROOT, "include", "unirestore_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ur_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("ur_scale_channels_fanout", "ur_tfa_prompt_update_fanout"):
        assert name in declared and name in capi.SIGNATURES and hasattr(lib, name), name
    assert sorted(capi.SIGNATURES) == sorted(declared)


def test_fanout_extent_of_the_production_decoder():
    """(out_h, out_w, widest_channels) from the decoder's configuration: at 512 x 512 the 256-channel maps at full resolution
    (and, equally, TFA level 2's 512-channel input at 256 x 256) bound the fanned-out batch."""
    import torch
    from unirestore_amd.modules import AutoencoderKL, SkipConnectedAutoEncoder
    with torch.device("meta"):
        ae = SkipConnectedAutoEncoder(AutoencoderKL(), "CFRM", dict(type="TFA", prompt_len=1, task=["ir", "cls", "seg"]))
    assert ae.fanout_extent(64, 64) == (512, 512, 256)
    assert ae.fanout_extent(128, 128) == (1024, 1024, 256)
