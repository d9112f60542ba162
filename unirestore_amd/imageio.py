"""Image files for `cli restore`: header scan, batches that share a canvas, 8-bit decode / encode on a small thread pool.

Pure Python + PIL.  The model only ever sees an image's *canvas* (`canvas_of`: min side scaled up to 512, then padded to a
multiple of 64), so files are grouped by canvas: every batch of a group goes through one captured graph
(`DiffUIE.forward_u8`), whatever the sizes of its members.
"""
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Iterable, Iterator, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from .modules.model import canvas_of

IO_THREADS = 4          # PIL releases the GIL while it decodes / encodes; more threads than this only fight the GPU driver thread
QUEUE_DEPTH = 2         # decoded batches waiting for the GPU


def extensions() -> frozenset:
    """Lower-case file extensions PIL can open."""
    Image.init()
    return frozenset(e.lower() for e, fmt in Image.registered_extensions().items() if fmt in Image.OPEN)


def list_inputs(path: str) -> List[str]:
    """A folder -> its files with a PIL-readable extension, sorted by name, not recursive.  A text file -> one path per line
    (relative to the list file's folder); of a `lq hq label` line the first column is used."""
    if os.path.isdir(path):
        ext = extensions()
        return [os.path.join(path, f) for f in sorted(os.listdir(path))
                if os.path.splitext(f)[1].lower() in ext and os.path.isfile(os.path.join(path, f))]
    if not os.path.isfile(path):
        raise FileNotFoundError(f"--input {path!r}: no such folder or list file")
    base = os.path.dirname(os.path.abspath(path))
    out = []
    with open(path) as f:
        for line in f:
            cols = line.split()
            if cols and not cols[0].startswith("#"):
                out.append(cols[0] if os.path.isabs(cols[0]) else os.path.join(base, cols[0]))
    return out


def scan(paths: Iterable[str]) -> List[Tuple[str, Tuple[int, int]]]:
    """[(path, (H, W))] from the file headers only (no decode).  EXIF orientation is not applied: the output has the stored size."""
    out = []
    for p in paths:
        with Image.open(p) as im:
            w, h = im.size
        out.append((p, (h, w)))
    return out


class Batch(NamedTuple):
    index: int                  # position in the plan (of all ranks): the noise seed of the batch derives from it
    canvas: Tuple[int, int]
    members: Tuple[int, ...]    # input indices, one per slot; a padded batch repeats its last image
    valid: int                  # the first `valid` slots are written out


def plan_batches(sizes: Sequence[Tuple[int, int]], batch: int, rank: int = 0, world: int = 1) -> List[Batch]:
    """Rank `rank`'s batches of the inputs with the given (H, W): grouped by canvas, input order kept inside a group, groups cut
    into batches of at most `batch`, batches ordered by their first member's input index; rank r gets batches r, r + world, ...
    A group's short last batch is padded to `batch` by repeating its last image when the group had a full batch before it (the
    `batch`-sized graph of that canvas exists anyway; the repeats are dropped on output) and runs at its own size otherwise.
    A pure function of its arguments; membership, slot order, padding and `index` do not depend on `world`."""
    if batch < 1:
        raise ValueError(f"batch must be >= 1, got {batch}")
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"need 0 <= rank < world, got rank {rank}, world {world}")
    groups = {}
    for i, (h, w) in enumerate(sizes):
        groups.setdefault(canvas_of(int(h), int(w)), []).append(i)
    cuts = []
    for canvas, idx in groups.items():
        for s in range(0, len(idx), batch):
            m = idx[s:s + batch]
            valid = len(m)
            if valid < batch and s > 0:
                m = m + [m[-1]] * (batch - valid)
            cuts.append((canvas, tuple(m), valid))
    cuts.sort(key=lambda c: c[1][0])
    plan = [Batch(i, c, m, v) for i, (c, m, v) in enumerate(cuts)]
    return plan[rank::world]


def graphs_implied(plan: Sequence[Batch]) -> int:
    """Number of graphs a process captures for these batches: one per distinct (slots, canvas)."""
    return len({(len(b.members), b.canvas) for b in plan})


def load_u8(path: str) -> torch.Tensor:
    """File -> uint8 [H, W, 3] host tensor; anything that is not plain RGB goes through PIL's convert("RGB")."""
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(arr.copy())


def save_u8(tensor: torch.Tensor, path: str) -> None:
    """uint8 [H, W, 3] tensor (host or device) -> PNG."""
    if tensor.dtype != torch.uint8 or tensor.ndim != 3 or tensor.shape[2] != 3:
        raise ValueError(f"save_u8: expected a uint8 tensor [H, W, 3], got {tensor.dtype} {tuple(tensor.shape)}")
    Image.fromarray(tensor.cpu().contiguous().numpy(), "RGB").save(path, format="PNG")


class Prefetcher:
    """Decodes the batches of a plan ahead of the consumer: `for batch, images in Prefetcher(plan, paths)`.  One feeder thread
    submits the decodes of a batch to the pool and puts the finished batch into a bounded queue, so the thread that drives the
    GPU never waits on a file while a batch is ready."""

    def __init__(self, plan: Sequence[Batch], paths: Sequence[str], pool: ThreadPoolExecutor, depth: int = QUEUE_DEPTH):
        self.plan, self.paths, self.pool = list(plan), paths, pool
        self.q = queue.Queue(maxsize=depth)
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self._feed, daemon=True)
        self.thread.start()

    def _put(self, item):
        while not self.stop.is_set():
            try:
                self.q.put(item, timeout=0.1)
                return
            except queue.Full:
                pass

    def _feed(self):
        try:
            for b in self.plan:
                if self.stop.is_set():
                    return
                distinct = {i: self.pool.submit(load_u8, self.paths[i]) for i in dict.fromkeys(b.members)}
                self._put((b, [distinct[i].result() for i in b.members]))
            self._put(None)
        except BaseException as e:            # handed to the consumer: a file that cannot be read ends the run there
            self._put(e)

    def __iter__(self) -> Iterator[Tuple[Batch, List[torch.Tensor]]]:
        try:
            while True:
                item = self.q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            self.stop.set()


def io_pool() -> ThreadPoolExecutor:
    return ThreadPoolExecutor(max_workers=IO_THREADS, thread_name_prefix="ur-imageio")
