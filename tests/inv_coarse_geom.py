"""The precondition of the three-coarse-levels inverse launch (pypwt_amd/csrc/launch_dwt2_inv_coarse.hip), re-derived from the
synthesis index rule alone -- output position g of a level needs the coefficients floor((g + S) / 2) - C .. + H2 - 1 of the level
below; column origins round down, extents up, to multiples of 4 -- so that the tests know which planes a tile shape must take and
which it must decline without asking the code under test (tests/test_emu_inv_coarse.py, tests/test_gpu_inv_coarse.py)."""

SHAPES = {0: (64, 32), 1: (128, 16), 2: (64, 16), 3: (128, 8), 4: (16, 4)}  # index -> (TX, TY): coefficients of level l per tile
LEVELS = 3


def region_fits(hlen, TX, TY, shape):
    """Do the planes of the three levels under a `shape` (rows, columns) output hold the regions a TX x TY tile stages?"""
    H2 = hlen // 2
    Cc, S = H2 // 2, 0 if H2 & 1 else 1
    padl = (4 - (Cc & 3)) & 3
    y, r = -Cc, TY + H2 + 1
    x, w = -Cc - padl, (padl + TX + H2 + 1 + 3) & ~3
    nr, nc = shape
    for _ in range(LEVELS):
        nr, nc = nr // 2, nc // 2
        if nr < r or nr < -y or nc < w or nc < -x:
            return False
        y, r = (y + S) // 2 - Cc, (y + r - 1 + S) // 2 - Cc + H2 - ((y + S) // 2 - Cc)
        x0 = ((x + S) // 2 - Cc) // 4 * 4
        x, w = x0, ((x + w - 1 + S) // 2 - Cc + H2 - x0 + 3) & ~3
    return True


def supported(hlen, shape):
    """dwt2_inv_coarse3_supported: even filters of at most 8 taps, rows a multiple of 8, columns of 32, some tile shape fits."""
    if hlen & 1 or not 2 <= hlen <= 8 or shape[0] % 8 or shape[1] % 32:
        return False
    return any(region_fits(hlen, TX, TY, shape) for TX, TY in SHAPES.values())
