"""Two identities the pair gathers of csrc/cn_common.hpp rely on, restated on the host (no GPU).

1. ONE parity bit per cell.  The table index of corner (x, y, z) is ``x ^ y m1 ^ z m2`` (masked), with the products taken as
   24-bit multiplies (``__umul24``) and the upper corners formed by adding m1 / m2 to them (``hash_cell``).  ``make_grid_dev``
   gives every level multipliers of ONE parity: the two hash primes (odd) or 2^b and 2^2b with b >= 1 (even).  Bit 0 of the
   index -- which entry of an aligned pair is the lower-x corner -- is then the same for the (y, z) rows ff and cc, the same
   for cf and fc, and the two differ exactly when m1 is odd: rows (ff, cf, fc, cc) carry (p, p ^ f, p ^ f, p), f = m1 & 1.
2. The floor-free cell (``hash_cell<., true>``).  For a float32 x >= 0 the conversion to int (round toward zero) is
   floor(x), and x - floor(x) -- what v_fract_f32 returns -- is exact in float32: it IS the fractional part.
"""

from __future__ import annotations

import numpy as np
import pytest

CN_P1, CN_P2 = 2654435761, 805459861  # csrc/cn_common.hpp
MAX_DENSE_BITS = 9  # check_grid: a dense level has at most 9 bits per axis


def level_multipliers(bits: int):
    """(m1, m2) of make_grid_dev for level_bits = bits (0: a hashed level)."""
    return (1 << bits, 1 << (2 * bits)) if bits else (CN_P1, CN_P2)


def umul24(a: np.ndarray, b: int) -> np.ndarray:
    """__umul24: the low 32 bits of the product of the operands' low 24 bits."""
    return ((a.astype(np.uint64) & 0xFFFFFF) * np.uint64(b & 0xFFFFFF) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def row_indices(ix, iy, iz, m1: int, m2: int, mask: int):
    """Masked indices of the lower-x corner of the four (y, z) rows ff, cf, fc, cc, as hash_cell / hash_level_xpair_issue form them."""
    hx0 = ix.astype(np.uint32)
    hy0 = umul24(iy, m1)
    hy1 = hy0 + np.uint32(m1 & 0xFFFFFFFF)  # uint32 wrap-around
    hz0 = umul24(iz, m2)
    hz1 = hz0 + np.uint32(m2 & 0xFFFFFFFF)
    hyz = (hy0 ^ hz0, hy1 ^ hz0, hy0 ^ hz1, hy1 ^ hz1)
    return [(hx0 ^ h) & np.uint32(mask) for h in hyz]


_AX = np.arange(64, dtype=np.uint32)
IX, IY, IZ = (a.reshape(-1) for a in np.meshgrid(_AX, _AX, _AX, indexing="ij"))

LEVELS = [("hashed T=2^4", 0, (1 << 4) - 1), ("hashed T=2^19", 0, (1 << 19) - 1)] + \
         [(f"dense b={b}", b, (1 << (3 * b)) - 1) for b in (1, 2, 5)]


@pytest.mark.parametrize("name,bits,mask", LEVELS, ids=[l[0] for l in LEVELS])
def test_the_four_rows_parities_follow_from_one_bit(name, bits, mask):
    m1, m2 = level_multipliers(bits)
    with np.errstate(over="ignore"):
        rows = row_indices(IX, IY, IZ, m1, m2, mask)
    p = rows[0] & 1
    f = np.uint32(m1 & 1)
    want = (p, p ^ f, p ^ f, p)
    for r, (got, w) in enumerate(zip(rows, want)):
        assert np.array_equal(got & 1, w), f"{name}: row {r}"
    # both values of the bit occur (the rule is not checked on a constant), and the pair of an entry is entry & ~1
    assert 0 < int(p.sum()) < p.size
    if bits == 0:
        assert int(f) == 1 and not np.array_equal(rows[0] & 1, rows[1] & 1)
    else:
        assert int(f) == 0 and np.array_equal(p, IX & 1), "dense level: x sits in the low bits"


def test_multipliers_share_their_parity_for_every_admitted_level_bits():
    for bits in range(0, MAX_DENSE_BITS + 1):
        m1, m2 = level_multipliers(bits)
        assert (m1 ^ m2) & 1 == 0, f"level_bits {bits}: m1 {m1}, m2 {m2}"
        assert (m1 & 1) == (1 if bits == 0 else 0)


def _default_grid_scales():
    """(scale, pos_offset) of every level of the default grid in both layouts."""
    from cropnerf_amd import config as PC

    out = [(s, 0.0) for s in PC.GridSpec().scalings()]
    out += [(s, 0.5) for s in PC.GridSpec(layout="tcnn").scalings()]
    assert len(out) == 32
    return out


def test_fraction_and_truncation_equal_the_floor_form_for_non_negative_coordinates():
    rng = np.random.default_rng(7)
    one_below = np.nextafter(np.float32(1.0), np.float32(0.0))
    for scale, off in _default_grid_scales():
        s = np.float32(scale)
        assert s > 0
        ints = np.arange(0, int(scale) + 1, dtype=np.float32)
        pos = np.concatenate([np.array([0.0, one_below, np.float32(2.0 ** -20), np.float32(0.5)], dtype=np.float32),
                              ints / s,  # products that land on (or next to) integers
                              np.nextafter(ints / s, np.float32(0.0)).astype(np.float32).clip(0.0, None),
                              np.nextafter(ints / s, np.float32(2.0)).astype(np.float32).clip(None, one_below),
                              rng.random(4096, dtype=np.float32)])
        pos = pos[(pos >= 0) & (pos < 1)]
        # fmaf(p, scale, pos_offset): the float64 product of two floats is exact, one rounding to float32 at the end
        x = (pos.astype(np.float64) * np.float64(s) + np.float64(off)).astype(np.float32)
        x = np.concatenate([x, ints, np.nextafter(ints[1:], np.float32(0.0)), np.nextafter(ints, np.float32(1e9))]).astype(np.float32)
        assert (x >= 0).all()
        # exact integers are among the coordinates, 0 included
        assert (x == np.floor(x)).sum() >= ints.size and (x == 0).any()
        fl = np.floor(x)
        assert np.array_equal(np.trunc(x), fl), "round toward zero is the floor"
        assert np.array_equal(x.astype(np.int32), fl.astype(np.int32)), "the conversion to int is the floor"
        frac32 = x - fl  # float32 arithmetic: the present form
        assert frac32.dtype == np.float32
        exact = x.astype(np.float64) - np.floor(x.astype(np.float64))  # the fractional part, exactly
        assert np.array_equal(frac32.astype(np.float64), exact), "x - floor(x) is exact in float32"
        fpart, ipart = np.modf(x)
        assert np.array_equal(fpart, frac32) and np.array_equal(ipart, fl)
        assert (frac32 >= 0).all() and (frac32 < 1).all()
