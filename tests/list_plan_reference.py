"""Which kernel variant the index-driven ops run (grouping, interpolate, aggregate, kpconv backward): the plan of
csrc/chan_block.hpp restated from DESIGN.md and the header text of include/pcc_test_hooks.h (group_path, interp_path) --
never obtained from the library.  The names are exact launch-profile names: ``base<lds> cb=N`` and ``base<direct>``."""

LDS_WG = 160 * 1024       # LDS a workgroup may take: the direct path where not one channel row of n floats fits
LDS_HALF_CU = 64 * 1024   # rows (or bins) of a workgroup where two should share a CU: what the channel block is fitted to


def fit_cb(row_bytes, cb_max=8, room=LDS_HALF_CU):
    """Channels per workgroup: the largest of cb_max, cb_max / 2, ..., 1 of which ``row_bytes`` each fit ``room`` (1 if none)."""
    cb = cb_max
    while cb > 1 and cb * row_bytes > room:
        cb //= 2
    return cb


def plan(b, c, n, forced=0, tile_words=0, spread_cus=None):
    """-> ('lds', cb) or ('direct', None) for rows of ``n`` floats.  ``forced``: the op's path switch (1 = LDS, ignored
    where not one row fits; 2 = direct).  ``tile_words``: further words of LDS per channel (the staged tile of
    pcc_aggregate_points' forward) -- where they no longer fit beside the rows, the direct path.  ``spread_cus``: the
    compute units of the device for the backwards that halve the block while they have fewer workgroups than that."""
    cb = fit_cb(4 * n)
    if cb * 4 * n > LDS_WG or forced == 2 or cb * 4 * n + cb * tile_words * 4 > LDS_WG:
        return 'direct', None
    if spread_cus is not None:
        while cb > 1 and b * -(-c // cb) < spread_cus:
            cb //= 2
    return 'lds', cb


def kernel_of(base, b, c, n, forced=0, tile_words=0, spread_cus=None):
    path, cb = plan(b, c, n, forced, tile_words, spread_cus)
    return f'{base}<lds> cb={cb}' if path == 'lds' else f'{base}<direct>'
