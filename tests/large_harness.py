"""Periodic-tensor harness of the large-tensor tests (tests/test_large_tensors_gpu.py; self-test in tests/test_large_tensors_cpu.py).

A launch on a 2 - 4 GiB tensor cannot be compared with an fp64 reference of the whole tensor, but every op under test is per image
(or per row), so the input is PERIODIC: unit i (an image, or a row of a Linear) is a copy of unit i mod P for a small odd P.  The fp64
reference and the per-element bound are computed for the P distinct units only, by the existing reference modules, and every unit
of the output is compared with reference unit i mod P:

  * tile_periodic(dst, src): dst[i] = src[i mod P] by chunked device copies (doubling: log2 of the unit count copies);
  * check_periodic(y, ref, bnd): |y[i] - ref[i mod P]| <= bnd[i mod P] for every element of every unit, in chunks whose temporaries
    stay below a fixed size; plain torch ops on views of at most CHUNK_ELEMS elements, so the check itself never relies on torch's
    handling of tensors of more than 2^31 elements.  NaN never satisfies a bound.  Returns the largest |err| / bound;
  * check_fill(bits, value): every element of a guard region still holds the fill pattern;
  * equal_chunked(a, b): two launches gave the same bits;
  * spot_units / host_check: a few units copied to the host and compared there (never a whole tensor).

All functions work on any device (the CPU self-test runs them on small tensors).
"""
import torch

COPY_ELEMS = 1 << 28           # elements per device copy of tile_periodic
CHUNK_ELEMS = 1 << 24          # elements per comparison chunk: two fp64 temporaries of 128 MiB and a mask alive at a time (< 1 GiB)


def tile_periodic(dst, src):
    """dst [U, ...] <- src [P, ...] repeated along dim 0 (dst[i] = src[i % P]); same trailing shape, dtype and device."""
    U, P = dst.shape[0], src.shape[0]
    assert dst.shape[1:] == src.shape[1:] and dst.dtype == src.dtype
    n = min(U, P)
    dst[:n].copy_(src[:n])
    unit = max(1, dst[0].numel())
    cap = max(1, COPY_ELEMS // (unit * P)) * P          # units per copy: whole periods, at most COPY_ELEMS elements (one period if larger)
    while n < U:                       # n stays a multiple of P and every copy starts at unit 0, so the phase is preserved
        m = min(n, U - n, cap)
        dst[n:n + m].copy_(dst[:m])
        n += m
    return dst


def _chunks(U, P, R, width, chunk_elems):
    """(first unit, unit count, first row, row count) pieces covering [0, U) x [0, R): every piece starts at a multiple of P units
    and, but for the tail, is whole periods; a period larger than chunk_elems is cut into row blocks."""
    rows = min(R, max(1, chunk_elems // max(1, P * width)))
    per = max(1, chunk_elems // max(1, rows * width * P)) * P
    for i in range(0, U, per):
        for r0 in range(0, R, rows):
            yield i, min(per, U - i), r0, min(rows, R - r0)


def check_periodic(y, ref, bnd, what="", chunk_elems=CHUNK_ELEMS):
    """y [U, R, ld] (any float dtype; columns >= ref.shape[-1] are not looked at), ref / bnd fp64 [P, R, width] on y's device.
    Asserts |y[i] - ref[i % P]| <= bnd[i % P] element-wise for every unit; returns max |err| / bnd (0 where both are 0)."""
    U, R, _ = y.shape
    P, R2, width = ref.shape
    assert R == R2 and bnd.shape == ref.shape and ref.dtype == torch.float64
    worst = 0.0
    safe = bnd.clamp_min(1e-300)
    for i0, k, r0, nr in _chunks(U, P, R, width, chunk_elems):
        q, r = divmod(k, P)
        rows = slice(r0, r0 + nr)
        for lo, cnt, per in ((i0, q * P, P), (i0 + q * P, r, r)):
            if cnt == 0:
                continue
            rr, bb, ss = ref[:per, rows], bnd[:per, rows], safe[:per, rows]
            got = y[lo:lo + cnt, rows, :width].double().view(cnt // per, per, nr, width)
            err = (got - rr).abs()
            ok = err <= bb
            if not bool(ok.all()):
                bad = (~ok).nonzero()[:6].tolist()
                det = "; ".join(f"unit {lo + b[0] * per + b[1]} (period unit {b[1]}) row {r0 + b[2]} col {b[3]}: got "
                                f"{float(got[tuple(b)]):.6g} ref {float(rr[b[1], b[2], b[3]]):.6g} bound {float(bb[b[1], b[2], b[3]]):.3g}"
                                for b in bad)
                raise AssertionError(f"{what}: {int((~ok).sum())} elements of units [{lo}, {lo + cnt}) outside the bound - {det}")
            del got, ok
            err.div_(ss).masked_fill_(bb <= 0, 0.0)               # in place: |err| / bound, 0 where both are 0
            worst = max(worst, float(err.max()))
            del err
    return worst


def check_fill(bits, value, what="", chunk_elems=CHUNK_ELEMS):
    """Every element of the integer view `bits` (any shape; dim 0 is chunked) equals `value`."""
    if bits.numel() == 0:
        return
    rows = bits.shape[0]
    per = max(1, chunk_elems // max(1, bits[0].numel()))
    for i in range(0, rows, per):
        blk = bits[i:i + per]
        if not bool((blk == value).all()):
            raise AssertionError(f"{what}: {int((blk != value).sum())} guard elements overwritten in rows [{i}, {min(rows, i + per)})")


def equal_chunked(a, b, what="", chunk_elems=CHUNK_ELEMS):
    """Bit equality of two flat integer views of one size."""
    assert a.shape == b.shape and a.dim() == 1
    for i in range(0, a.numel(), chunk_elems):
        if not bool((a[i:i + chunk_elems] == b[i:i + chunk_elems]).all()):
            raise AssertionError(f"{what}: two launches differ in elements [{i}, {min(a.numel(), i + chunk_elems)})")


def spot_units(U, *unit_bytes):
    """Units to copy to the host: the first, the last, and for each tensor of the launch (bytes per unit given) the unit that
    straddles byte 2^31 of that tensor, where it has one."""
    s = {0, U - 1}
    for nb in unit_bytes:
        i = (1 << 31) // nb
        if 0 < i < U:
            s.add(i)
    return sorted(s)


def host_check(y, ref_cpu, bnd_cpu, units, what=""):
    """The same bound on the host for a few units of y (each copied alone)."""
    P, _, width = ref_cpu.shape
    worst = 0.0
    for i in units:
        got = y[i, :, :width].cpu().double()
        err = (got - ref_cpu[i % P]).abs()
        ok = err <= bnd_cpu[i % P]
        assert bool(ok.all()), f"{what}: unit {i}: {int((~ok).sum())} elements outside the bound on the host"
        worst = max(worst, float(torch.where(bnd_cpu[i % P] > 0, err / bnd_cpu[i % P].clamp_min(1e-300), torch.zeros_like(err)).max()))
    return worst
