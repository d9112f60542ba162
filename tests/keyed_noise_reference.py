"""Reference of the keyed noise (ur_keyed_noise / ops.keyed_noise): Philox4x32-10 in numpy integers and Box-Muller in fp64.

Written from the specification alone (include/unirestore_hip.h; Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
SC'11) - it shares no code with csrc/noise.hip.  The words are exact; the normals are the fp64 value of the formula the kernel
evaluates in fp32, so they bound the kernel's rounding error.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl constants
MASK = np.uint64(0xFFFFFFFF)
MAX_ABS = float(np.sqrt(48 * np.log(2)))  # sqrt(-2 ln 2^-24) ~ 5.768: the largest |value| the smallest uniform gives


def philox4x32_10(counter, key):
    """counter uint32 [..., 4], key uint32 [..., 2] (broadcast against each other) -> the 4 output words uint32 [..., 4]."""
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def key_of(seed: int):
    assert 0 <= seed < 1 << 64
    return np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)


def words(seed: int, draw: int, count: int) -> np.ndarray:
    """uint32 [count]: element e takes word e & 3 of the counter (e >> 2, draw, 0, 0) under the seed's key."""
    nctr = (count + 3) // 4
    ctr = np.zeros((nctr, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(nctr, dtype=np.uint64).astype(np.uint32)
    ctr[:, 1] = draw
    return philox4x32_10(ctr, key_of(seed)).reshape(-1)[:count]


def uniforms(w: np.ndarray) -> np.ndarray:
    """fp64 ((w >> 9) + 0.5) * 2^-23 - the same number the kernel holds in fp32 (24 significant bits)."""
    return ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(seed: int, draw: int, count: int) -> np.ndarray:
    """fp64 [count]: Box-Muller on the word pairs (0,1), (2,3) of every counter; even word r cos(theta), odd word r sin(theta)."""
    nctr = (count + 3) // 4
    u = uniforms(words(seed, draw, 4 * nctr)).reshape(-1, 2)
    r, theta = np.sqrt(-2.0 * np.log(u[:, 0])), 2.0 * np.pi * u[:, 1]
    return np.stack([r * np.cos(theta), r * np.sin(theta)], -1).reshape(-1)[:count]


def keyed_noise(seeds, draw: int, shape, kind="normal") -> np.ndarray:
    """[N, C, H, W]: uint32 words ("bits") or fp64 normals ("normal"), image n from seeds[n] alone."""
    count = int(np.prod(shape))
    one = words if kind == "bits" else normals
    return np.stack([one(int(s), draw, count) for s in seeds]).reshape(len(seeds), *shape)
